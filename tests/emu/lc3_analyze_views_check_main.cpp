// TEST INFRASTRUCTURE -- a stand-alone program over the check header of lc3gpu_analyze_mixed_views (lc3_host_analyze_views.h) and the plan
// it shares with the inspector, built with -fsanitize=address,undefined and run as a child process by tests/test_emu_analyze_views.py over
// the extreme view lists that test also gives to the emulator library.  Host code only; nothing here touches a GPU.
//
// usage: <program> <case file>.  The file: int32 n_cases, then per case
//   int32 n_streams, int32 descs[n_streams][3] (fs_hz, frame_us, nbytes), int32 max_views, int32 max_frames, int32 n_views,
//   lc3gpu_view views[n_views], uint64 bounds[10] (in base, in bytes, flags base, n_flags, energy base, n_energy, bands base, n_bands,
//   spec base, n_spec; base 0 = not given), int32 want
// For every case the check must return `want`; an accepted case is then planned with the analyzer's frames per workgroup and walked with the
// kernel's look-ups (all lanes up to a million frames, the first and the last workgroup of every bucket beyond): every lane's frame, flag,
// float and rows must lie inside the extents and its scratch column below max_frames.  Prints "ok <cases> <lanes walked>" and exits 0, or
// says what differed and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../lc3-codec_amd/csrc/lc3_host_analyze_views.h"

namespace {
struct Reader {
    std::vector<unsigned char> data;
    size_t pos = 0;
    void get(void *dst, size_t n) {
        if (pos + n > data.size()) {
            fprintf(stderr, "case file too short\n");
            exit(1);
        }
        memcpy(dst, data.data() + pos, n);
        pos += n;
    }
    int32_t i32() {
        int32_t v;
        get(&v, 4);
        return v;
    }
};
bool inside(uint64_t first, uint64_t len, uint64_t size) { return first < size && len <= size - first; }
}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    Reader R;
    {
        FILE *f = fopen(argv[1], "rb");
        if (!f) return 2;
        unsigned char buf[65536];
        size_t n;
        while ((n = fread(buf, 1, sizeof(buf), f)) > 0) R.data.insert(R.data.end(), buf, buf + n);
        fclose(f);
    }
    const int n_cases = R.i32();
    unsigned long long walked = 0;
    lc3_iv_plan P;  // one plan object for all cases, as an analyzer keeps one for all calls
    for (int ci = 0; ci < n_cases; ci++) {
        const int n_streams = R.i32();
        std::vector<lc3_iv_stream> streams((size_t)n_streams);
        for (int i = 0; i < n_streams; i++) {
            const int fs = R.i32(), us = R.i32(), nb = R.i32();
            if (lc3_iv_config(us, fs, streams[(size_t)i])) {
                fprintf(stderr, "case %d: bad descriptor\n", ci);
                return 1;
            }
            streams[(size_t)i].nbytes = nb;
        }
        const int max_views = R.i32(), max_frames = R.i32(), n_views = R.i32();
        std::vector<lc3_iview> views((size_t)(n_views > 0 ? n_views : 0));
        if (n_views > 0) R.get(views.data(), views.size() * sizeof(lc3_iview));
        uint64_t b[10];
        R.get(b, sizeof(b));
        const int want = R.i32();
        lc3_av_bounds B;
        B.in_base = b[0], B.in_bytes = b[1], B.flags_base = b[2], B.n_flags = b[3];
        B.energy_base = b[4], B.n_energy = b[5], B.bands_base = b[6], B.n_bands = b[7], B.spec_base = b[8], B.n_spec = b[9];
        B.use_flags = b[2] != 0, B.use_energy = b[4] != 0, B.use_bands = b[6] != 0, B.use_spec = b[8] != 0;
        int frames = 0, max_nb = 0;
        static const lc3_iview none = {};  // (a list of no views is still a list)
        const int rc = lc3_aviews_check(streams.data(), n_streams, max_views, max_frames, n_views > 0 ? views.data() : &none, n_views, B, &frames, &max_nb);
        if (rc != want) {
            fprintf(stderr, "case %d: the check returned %d, expected %d\n", ci, rc, want);
            return 1;
        }
        if (rc || n_views == 0) continue;
        const int fpb = (int)lc3_av_fpb(max_nb);
        if (lc3_av_lds_bytes(max_nb) > 65536) {
            fprintf(stderr, "case %d: %zu bytes of LDS\n", ci, lc3_av_lds_bytes(max_nb));
            return 1;
        }
        std::vector<lc3_iv_row> rows((size_t)n_views);
        std::vector<lc3_iv_bucket> buckets((size_t)n_views);
        lc3_iviews_build(streams.data(), views.data(), n_views, fpb, rows.data(), buckets.data(), P);
        long long seen = 0;
        for (int bi = 0; bi < P.n_buckets; bi++) {
            const lc3_iv_bucket &bk = buckets[(size_t)bi];
            const int n_wg = (int)(((unsigned)bk.n_frames + (unsigned)fpb - 1u) / (unsigned)fpb);
            seen += bk.n_frames;
            for (int w = 0; w < n_wg; w++) {
                if (frames > 1000000 && w != 0 && w != n_wg - 1) continue;
                const int wg = bk.wg0 + w;
                if (lc3_iv_find_bucket(buckets.data(), P.n_buckets, wg) != bi) {
                    fprintf(stderr, "case %d: workgroup %d does not find bucket %d\n", ci, wg, bi);
                    return 1;
                }
                const int nfr = lc3_iv_wg_frames(bk, wg, fpb);
                if (nfr < 1 || nfr > fpb) {
                    fprintf(stderr, "case %d: workgroup %d has %d frames\n", ci, wg, nfr);
                    return 1;
                }
                for (int tid = 0; tid < nfr; tid++, walked++) {
                    uint64_t src, dst;
                    lc3_iv_lane_place(rows.data(), bk, wg, tid, fpb, src, dst);
                    const long long column = (long long)bk.frame0 + (long long)(wg - bk.wg0) * fpb + tid;
                    if (!inside(src, (uint64_t)bk.nbytes, B.in_bytes) || (B.use_flags && !inside(dst, 1, B.n_flags)) ||
                        (B.use_energy && !inside(dst, 1, B.n_energy)) || (B.use_bands && !inside(dst, 1, B.n_bands)) ||
                        (B.use_spec && !inside(dst, 1, B.n_spec)) || column < 0 || column >= max_frames) {
                        fprintf(stderr, "case %d: workgroup %d lane %d is outside the extents\n", ci, wg, tid);
                        return 1;
                    }
                }
            }
        }
        if (seen != frames || P.n_wg < P.n_buckets) {
            fprintf(stderr, "case %d: the buckets hold %lld frames of %d\n", ci, seen, frames);
            return 1;
        }
    }
    printf("ok %d %llu\n", n_cases, walked);
    return 0;
}
