// TEST INFRASTRUCTURE -- a stand-alone program over the check and plan header of lc3gpu_mix_mixed_views (lc3_host_mix_views.h) and the
// placement of the lane body (lc3_dev_mix.h), built with -fsanitize=address,undefined and run as a child process by
// tests/test_emu_mix_views.py over the extreme lists that test also gives to the emulator library.  Host code only; nothing here touches a
// GPU.
//
// usage: <program> <case file>.  The file: int32 n_cases, then per case
//   int32 n_streams, int32 descs[n_streams][3] (fs_hz, frame_us, nbytes), int32 max_views,
//   int32 n_in, lc3gpu_view in_views[n_in], lc3gpu_mix_in ins[n_in], int32 n_out, lc3gpu_view out_views[n_out], lc3gpu_mix_out outs[n_out],
//   uint64 bounds[4] (in base, in elements, out base, out elements), int32 want
// For every case the check must return `want`; an accepted case with outputs is then planned and walked with the kernel's look-up (all
// workgroups of a bus of up to a million samples, the first and the last one beyond): every lane's pair of every row must lie inside the
// extents, and the workgroups of a bus must hold its S samples exactly.  First the multiplier that divides by nf is held against the
// division for every frame length, at both ends of the sample range and around every multiple of 2^k.  Prints "ok <cases> <pairs walked>"
// and exits 0, or says what differed and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../lc3-codec_amd/csrc/lc3_dev_mix.h"

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
bool pair_inside(uint64_t at, int stride, uint64_t size) { return at < size && (uint64_t)stride < size - at; }

int check_division() {
    static const int rates[6] = {8000, 16000, 24000, 32000, 44100, 48000};
    for (int k = 0; k < 6; k++)
        for (int us = 7500; us <= 10000; us += 2500) {
            const int nf = lc3_mx_nf(us, rates[k]);
            lc3_iv_stream c;
            if (lc3_iv_config(us, rates[k], c) || nf < 60 || nf > 480 || (nf & 3)) return 1;
            const uint64_t magic = lc3_mx_magic(nf);
            auto same = [&](uint64_t s) { return s > 0x7fffffffull || lc3_mx_div((uint32_t)s, magic) == (uint32_t)(s / (uint64_t)nf); };
            for (uint64_t s = 0; s < 100000; s++)
                if (!same(s) || !same(0x7fffffffull - s)) return 1;
            for (int b = 8; b < 31; b++)
                for (int64_t d = -1000; d <= 1000; d++)
                    if (!same((uint64_t)(((int64_t)1 << b) + d))) return 1;
            // around the multiples of nf nearest the top of the range: where a multiplier that is too large fails first
            const uint64_t top = (0x7fffffffull / (uint64_t)nf) * (uint64_t)nf;
            for (uint64_t q = 0; q < 2000; q++)
                if (!same(top - q * (uint64_t)nf) || !same(top - q * (uint64_t)nf - 1) || !same(top - q * (uint64_t)nf + 1)) return 1;
        }
    return 0;
}
}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    if (check_division()) {
        fprintf(stderr, "the multiplier does not divide\n");
        return 1;
    }
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
        const int n_streams = R.i32();
        std::vector<lc3_mx_stream> streams((size_t)n_streams);
        for (int i = 0; i < n_streams; i++) {
            const int fs = R.i32(), us = R.i32();
            (void)R.i32();
            lc3_mx_make_stream(us, fs, streams[(size_t)i]);
        }
        const int max_views = R.i32();
        const int n_in = R.i32();
        std::vector<lc3_iview> vin((size_t)(n_in > 0 ? n_in : 0) + 1);  // (a list of no views is still a list)
        std::vector<lc3_mix_in_t> tin((size_t)(n_in > 0 ? n_in : 0) + 1);
        if (n_in > 0) R.get(vin.data(), (size_t)n_in * sizeof(lc3_iview)), R.get(tin.data(), (size_t)n_in * sizeof(lc3_mix_in_t));
        const int n_out = R.i32();
        std::vector<lc3_iview> vout((size_t)(n_out > 0 ? n_out : 0) + 1);
        std::vector<lc3_mix_out_t> tout((size_t)(n_out > 0 ? n_out : 0) + 1);
        if (n_out > 0) R.get(vout.data(), (size_t)n_out * sizeof(lc3_iview)), R.get(tout.data(), (size_t)n_out * sizeof(lc3_mix_out_t));
        uint64_t b[4];
        R.get(b, sizeof(b));
        const int want = R.i32();
        lc3_mx_bounds B = {b[0], b[1], b[2], b[3]};
        lc3_mx_plan P(max_views);  // (max_views >= 1 in every case)
        for (int round = 0; round < 2; round++) {  // twice through one plan object: what a call leaves behind must not matter to the next
            const int rc = lc3_mviews_check(streams.data(), n_streams, max_views, vin.data(), tin.data(), n_in, vout.data(), tout.data(), n_out, B, P);
            if (rc != want) {
                fprintf(stderr, "case %d: the check returned %d, expected %d\n", ci, rc, want);
                return 1;
            }
            if (rc || n_out == 0) {
                P.clear();
                continue;
            }
            std::vector<lc3_mx_row> rin((size_t)n_in + 1), rout((size_t)n_out);
            std::vector<lc3_mx_bus> buses((size_t)n_out);
            lc3_mviews_build(streams.data(), vin.data(), tin.data(), n_in, vout.data(), tout.data(), n_out, rin.data(), rout.data(), buses.data(), P);
            if (!P.touched.empty()) {
                fprintf(stderr, "case %d: the plan keeps its buses\n", ci);
                return 1;
            }
            int rows_in = 0, rows_out = 0, wgs = 0;
            for (int bi = 0; bi < P.n_buses; bi++) {
                const lc3_mx_bus &bk = buses[(size_t)bi];
                const int n_wg = (int)(((unsigned)bk.S + LC3_MX_SPW - 1u) / LC3_MX_SPW);
                if (bk.wg0 != wgs || bk.first_out != rows_out || bk.first_in < rows_in || bk.n_out < 1 || bk.n_in < 0 || bk.n_in > LC3_MX_MAX_BUS_INPUTS ||
                    bk.first_in + bk.n_in > n_in || bk.S < 2 || (bk.S & 1)) {
                    fprintf(stderr, "case %d: bus row %d is out of order\n", ci, bi);
                    return 1;
                }
                wgs += n_wg, rows_out += bk.n_out, rows_in = bk.first_in + bk.n_in;
                long long pairs = 0;
                for (int w = 0; w < n_wg; w++) {
                    const uint32_t s0 = (uint32_t)w * LC3_MX_SPW;
                    if (bk.S > 1000000 && w != 0 && w != n_wg - 1) {
                        pairs += LC3_MX_LANES;
                        continue;
                    }
                    if (lc3_mx_find_bus(buses.data(), P.n_buses, bk.wg0 + w) != bi) {
                        fprintf(stderr, "case %d: workgroup %d does not find bus row %d\n", ci, bk.wg0 + w, bi);
                        return 1;
                    }
                    for (int tid = 0; tid < LC3_MX_LANES; tid++) {
                        const uint32_t s = s0 + 2u * (uint32_t)tid;
                        if (s >= (uint32_t)bk.S) continue;
                        pairs++, walked++;
                        for (int i = 0; i < bk.n_in; i++) {
                            const lc3_mx_row &r = rin[(size_t)(bk.first_in + i)];
                            if (!pair_inside(lc3_mx_place(r, s), r.stride, B.in_elems) || r.aux < -32768 || r.aux > 32767 || (bk.planar && r.stride != 1)) {
                                fprintf(stderr, "case %d: input row %d, sample %u is outside the extents\n", ci, bk.first_in + i, s);
                                return 1;
                            }
                        }
                        for (int o = 0; o < bk.n_out; o++) {
                            const lc3_mx_row &r = rout[(size_t)(bk.first_out + o)];
                            if (!pair_inside(lc3_mx_place(r, s), r.stride, B.out_elems) || r.aux < -1 || r.aux >= bk.n_in || (bk.planar && r.stride != 1)) {
                                fprintf(stderr, "case %d: output row %d, sample %u is outside the extents\n", ci, bk.first_out + o, s);
                                return 1;
                            }
                        }
                    }
                }
                if (pairs * 2 != bk.S) {
                    fprintf(stderr, "case %d: bus row %d holds %lld samples of %d\n", ci, bi, pairs * 2, bk.S);
                    return 1;
                }
            }
            if (wgs != P.n_wg || rows_out != n_out) {
                fprintf(stderr, "case %d: %d workgroups of %d, %d output rows of %d\n", ci, wgs, P.n_wg, rows_out, n_out);
                return 1;
            }
        }
    }
    printf("ok %d %llu\n", n_cases, walked);
    return 0;
}
