// TEST INFRASTRUCTURE -- a stand-alone program over the check and plan header of lc3gpu_resample_mixed_views (lc3_host_resample_views.h)
// and the placement of the lane body (lc3_dev_resample.h), built with -fsanitize=address,undefined and run as a child process by
// tests/test_emu_resample_views.py over the extreme lists that test also gives to the emulator library.  Host code only; nothing here
// touches a GPU.
//
// usage: <program> <case file>.  The file: int32 n_cases, then per case
//   int32 n_channels, int32 descs[n_channels][3] (fs_in_hz, fs_out_hz, frame_us), int32 max_views,
//   int32 n_views, lc3gpu_view in_views[n_views], lc3gpu_view out_views[n_views],
//   uint64 bounds[4] (in base, in elements, out base, out elements), int32 want
// For every case the check must return `want`; an accepted case with views is then planned and walked with the kernel's look-up (all
// workgroups of a view of up to a million output samples, the first and the last one beyond): every pair of the window and every pair of
// output samples must lie inside the extents, the window inside the LDS array, the histories inside the history array and apart, and the
// workgroups of a view must hold its S_out samples exactly.  This runs twice through one state: fresh, and advanced.  First the two
// multipliers are held against the divisions.  Prints "ok <cases> <pairs walked>" and exits 0, or says what differed and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../lc3-codec_amd/csrc/lc3_dev_resample.h"

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
            const int nf = lc3_rs_nf(us, rates[k]);
            if (nf < 60 || nf > 480 || (nf & 3)) return 1;
            const uint64_t magic = lc3_rs_magic(nf);
            auto same = [&](uint64_t s) { return s > 0x7fffffffull || lc3_rs_div((uint32_t)s, magic) == (uint32_t)(s / (uint64_t)nf); };
            for (uint64_t s = 0; s < 100000; s++)
                if (!same(s) || !same(0x7fffffffull - s)) return 1;
            for (int b = 8; b < 31; b++)
                for (int64_t d = -1000; d <= 1000; d++)
                    if (!same((uint64_t)(((int64_t)1 << b) + d))) return 1;
            const uint64_t top = (0x7fffffffull / (uint64_t)nf) * (uint64_t)nf;
            for (uint64_t q = 0; q < 2000; q++)
                if (!same(top - q * (uint64_t)nf) || !same(top - q * (uint64_t)nf - 1) || !same(top - q * (uint64_t)nf + 1)) return 1;
        }
    for (int L = 1; L <= 6; L++)
        for (uint32_t u = 0; u <= (uint32_t)LC3_RS_CHUNK * 6u; u++)
            if (lc3_rs_div_l(u, 65536 / L + 1) != u / (uint32_t)L) return 1;
    return 0;
}
}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    if (check_division()) {
        fprintf(stderr, "a multiplier does not divide\n");
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
        const int n_channels = R.i32();
        lc3_rs_state St;
        St.channels.resize((size_t)n_channels);
        for (int i = 0; i < n_channels; i++) {
            const int fi = R.i32(), fo = R.i32(), us = R.i32();
            if (lc3_rs_make_channel(fi, fo, us, St.channels[(size_t)i])) {
                fprintf(stderr, "case %d: descriptor %d is refused\n", ci, i);
                return 1;
            }
        }
        const int hist_len = n_channels * 2 * LC3_RS_HIST;
        const int max_views = R.i32();
        const int n_views = R.i32();
        std::vector<lc3_iview> vin((size_t)(n_views > 0 ? n_views : 0) + 1), vout((size_t)(n_views > 0 ? n_views : 0) + 1);
        if (n_views > 0) R.get(vin.data(), (size_t)n_views * sizeof(lc3_iview)), R.get(vout.data(), (size_t)n_views * sizeof(lc3_iview));
        uint64_t b[4];
        R.get(b, sizeof(b));
        const int want = R.i32();
        lc3_rs_bounds B = {b[0], b[1], b[2], b[3]};
        for (int round = 0; round < 2; round++) {
            const int rc = lc3_rviews_check(St, max_views, vin.data(), vout.data(), n_views, B);
            if (rc != want) {
                fprintf(stderr, "case %d: the check returned %d, expected %d\n", ci, rc, want);
                return 1;
            }
            if (rc || n_views <= 0) continue;
            std::vector<lc3_rs_row> rows((size_t)n_views);
            lc3_rviews_build(St, vin.data(), vout.data(), n_views, rows.data());
            int wgs = 0;
            for (int vi = 0; vi < n_views; vi++) {
                const lc3_rs_row &r = rows[(size_t)vi];
                const lc3_rs_channel &c = St.channels[(size_t)vin[(size_t)vi].channel];
                const int n_wg = (int)(((unsigned)r.S_out + LC3_RS_CHUNK - 1u) / LC3_RS_CHUNK);
                const bool copy = r.coef_off < 0;
                if (r.wg0 != wgs || r.S_out < 2 || (r.S_out & 1) || (r.S_in & 1) || (int64_t)r.S_out * r.M != (int64_t)r.S_in * r.L || r.L * r.T > LC3_RS_MAX_COEF ||
                    r.T - 1 > LC3_RS_HIST || (copy ? (r.T != 1 || r.L != 1 || r.M != 1) : (r.coef_off + r.L * r.T > LC3_RS_COEF_TOTAL)) || r.hist_wr < 0 ||
                    r.hist_wr + LC3_RS_HIST > hist_len || r.hist_rd + LC3_RS_HIST > hist_len || (r.hist_rd >= 0 && r.hist_rd == r.hist_wr) ||
                    (!copy && (round == 0) != (r.hist_rd < 0)) || (!copy && (c.fresh || r.hist_wr != vin[(size_t)vi].channel * 2 * LC3_RS_HIST + c.cur * LC3_RS_HIST))) {
                    fprintf(stderr, "case %d: row %d is out of order\n", ci, vi);
                    return 1;
                }
                wgs += n_wg;
                long long outs = 0;
                for (int w = 0; w < n_wg; w++) {
                    if (r.S_out > 1000000 && w != 0 && w != n_wg - 1) {
                        outs += LC3_RS_CHUNK;
                        continue;
                    }
                    if (lc3_rs_find_row(rows.data(), n_views, r.wg0 + w) != vi) {
                        fprintf(stderr, "case %d: workgroup %d does not find row %d\n", ci, r.wg0 + w, vi);
                        return 1;
                    }
                    const lc3_rs_chunk k = lc3_rs_chunk_of(r, w);
                    const int64_t b0 = (int64_t)k.m0 * r.M / r.L, b_last = ((int64_t)k.m0 + k.n_out - 1) * r.M / r.L;
                    if (k.n_out < 2 || k.n_out > LC3_RS_CHUNK || (k.n_out & 1) || (int64_t)k.m0 * r.M % r.L != 0 || k.b0 != b0 || b_last >= r.S_in ||
                        k.kw0 > b0 - (r.T - 1) || k.kw0 < b0 - r.T || (k.kw0 & 1) || 2 * k.n_pairs > LC3_RS_MAX_WINDOW || b_last - k.kw0 >= 2 * k.n_pairs) {
                        fprintf(stderr, "case %d: row %d, chunk %d is out of order\n", ci, vi, w);
                        return 1;
                    }
                    for (int i = 0; i < k.n_pairs; i++) {
                        const int s = k.kw0 + 2 * i;
                        walked++;
                        if (s < 0 || s >= r.S_in) continue;
                        if (!pair_inside(lc3_rs_place(r.in_off, r.in_magic, r.nf_in, r.in_pitch, r.in_stride, (uint32_t)s), r.in_stride, B.in_elems)) {
                            fprintf(stderr, "case %d: row %d, input sample %d is outside the extents\n", ci, vi, s);
                            return 1;
                        }
                    }
                    for (int i = 0; 2 * i < k.n_out; i++) {
                        walked++;
                        if (!pair_inside(lc3_rs_place(r.out_off, r.out_magic, r.nf_out, r.out_pitch, r.out_stride, (uint32_t)(k.m0 + 2 * i)), r.out_stride,
                                         B.out_elems)) {
                            fprintf(stderr, "case %d: row %d, output sample %d is outside the extents\n", ci, vi, k.m0 + 2 * i);
                            return 1;
                        }
                    }
                    outs += k.n_out;
                }
                if (outs != r.S_out) {
                    fprintf(stderr, "case %d: row %d holds %lld samples of %d\n", ci, vi, outs, r.S_out);
                    return 1;
                }
            }
            if (wgs != St.n_wg) {
                fprintf(stderr, "case %d: %d workgroups of %d\n", ci, wgs, St.n_wg);
                return 1;
            }
        }
    }
    printf("ok %d %llu\n", n_cases, walked);
    return 0;
}
