// TEST INFRASTRUCTURE -- a stand-alone program over the check and row header of lc3gpu_measure_mixed_views (lc3_host_measure_views.h) and
// the placement of the lane body (lc3_dev_level.h), built with -fsanitize=address,undefined and run as a child process by
// tests/test_emu_meter_views.py over the hostile lists that test also gives to the emulator library.  Host code only; nothing here touches
// a GPU.
//
// usage: <program> <case file>.  The file: int32 n_cases, then per case
//   int32 n_channels, int32 descs[n_channels][6] (fs_hz, frame_us, attack_q15, release_q15, threshold, hang_frames), int32 max_views,
//   int32 n_views, lc3gpu_view views[n_views],
//   uint64 bounds[8] (pcm base, pcm elements, active base, active bytes, levels base, levels records, use_active, use_levels), int32 want
// For every case the check must return `want`; an accepted case with views is then built into rows and walked as the kernel walks it (all
// frames of a view of up to 100 000 frames, the first and the last one beyond): the first and the last sample of every frame, the word
// before the last sample and every output index must lie inside the extents, and the rows must say what the channels say.  This runs twice
// through one state: fresh, and advanced.  Prints "ok <cases> <frames walked>" and exits 0, or says what differed and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../lc3-codec_amd/csrc/lc3_dev_level.h"

namespace {
struct Reader {
    std::vector<unsigned char> data;
    size_t pos = 0;
    void get(void *dst, size_t n) {
        if (pos + n > data.size()) {
            fprintf(stderr, "case file too short\n");
            exit(1);
        }
        if (n) memcpy(dst, data.data() + pos, n);
        pos += n;
    }
    int32_t i32() {
        int32_t v;
        get(&v, 4);
        return v;
    }
};
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
    for (int ci = 0; ci < n_cases; ci++) {
        const int n_channels = R.i32();
        lc3_mt_state St;
        St.channels.resize((size_t)n_channels);
        for (int i = 0; i < n_channels; i++) {
            int32_t d[6];
            R.get(d, sizeof(d));
            if (lc3_mt_make_channel(d[0], d[1], d[2], d[3], (uint32_t)d[4], d[5], St.channels[(size_t)i])) {
                fprintf(stderr, "case %d: descriptor %d is refused\n", ci, i);
                return 1;
            }
        }
        const int max_views = R.i32();
        const int n_views = R.i32();
        std::vector<lc3_iview> views((size_t)(n_views > 0 ? n_views : 0) + 1);
        if (n_views > 0) R.get(views.data(), (size_t)n_views * sizeof(lc3_iview));
        uint64_t b[8];
        R.get(b, sizeof(b));
        const int want = R.i32();
        lc3_mt_bounds B = {b[0], b[1], b[2], b[3], b[4], b[5], (int)b[6], (int)b[7]};
        for (int round = 0; round < 2; round++) {
            const int rc = lc3_mviews_check(St, max_views, views.data(), n_views, B);
            if (rc != want) {
                fprintf(stderr, "case %d: the check returned %d, expected %d\n", ci, rc, want);
                return 1;
            }
            if (rc || n_views <= 0) continue;
            std::vector<lc3_mt_row> rows((size_t)n_views);
            lc3_mviews_build(St, views.data(), n_views, rows.data());
            for (int vi = 0; vi < n_views; vi++) {
                const lc3_mt_row &r = rows[(size_t)vi];
                const lc3_iview &v = views[(size_t)vi];
                const lc3_mt_channel &c = St.channels[(size_t)v.channel];
                if (r.channel != v.channel || r.nf != c.nf || r.n_frames != v.n_frames || r.stride != v.pcm_stride || r.pitch < r.nf * r.stride || r.flag_pitch < 1 ||
                    r.attack != c.attack || r.release != c.release || r.threshold != c.threshold || r.hang_frames != c.hang_frames ||
                    r.fresh != (round == 0) || c.fresh != 0 || (r.nf & 3) != 0 || r.nf < 60 || r.nf > 480) {
                    fprintf(stderr, "case %d: row %d is out of order\n", ci, vi);
                    return 1;
                }
                uint64_t base = r.pcm_off, dst = r.flag_off;
                for (int t = 0; t < r.n_frames; t++, base += (uint64_t)(uint32_t)r.pitch, dst += (uint64_t)(uint32_t)r.flag_pitch) {
                    if (r.n_frames > 100000 && t != 0 && t != r.n_frames - 1) continue;
                    walked++;
                    const uint64_t far = (uint64_t)(r.nf - 1) * (uint64_t)r.stride;
                    const bool in = base < B.pcm_elems && far < B.pcm_elems - base;
                    const bool aligned = r.stride != 1 || (((B.pcm_base >> 1) + base) & 1u) == 0;  // (a 32-bit word of a stride-1 frame)
                    const bool out = (!B.use_active || dst < B.n_active) && (!B.use_levels || dst < B.n_levels);
                    if (!in || !aligned || !out) {
                        fprintf(stderr, "case %d: row %d, frame %d is outside the extents\n", ci, vi, t);
                        return 1;
                    }
                }
            }
        }
    }
    printf("ok %d %llu\n", n_cases, walked);
    return 0;
}
