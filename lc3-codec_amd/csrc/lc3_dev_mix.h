// The lane body of lc3gpu_mix_mixed_views (include/lc3gpu.h): one lane, one pair of samples (s, s + 1) of one bus, s even.  Compiled by
// the companion library's kernel (lc3gpu_mixer.hip) and, unchanged, by the CPU emulation (tests/emu/lc3_emu_mix_views.cpp).
//
// A frame length is even for every configuration, so a pair never straddles a frame: both samples lie in frame s / nf.  For pcm_stride 1
// the pair is ONE 32-bit access (the contract holds pcm_off and the pitch even and the base 4-byte aligned), otherwise two 16-bit ones.
// The lane walks the bus's inputs once, two int32 totals in registers, then the bus's outputs: it reads an output's minus input again (a
// cache hit: the lane itself read that very address a moment ago), recomputes that term, subtracts, clamps and stores.  A room of M
// participants therefore costs M reads and M writes per sample, not M * M.  The rows are the same for every lane of a workgroup.
//
// The bound that keeps everything in int32: gain_q14 lies in -32768..32767, so |in * gain + 8192| <= 2^30 + 2^13 and |term| <= 65536; a bus
// holds at most 16384 inputs (LC3_MX_MAX_BUS_INPUTS), so |total| <= 2^30, and |total - term| <= 2^30 + 2^16 < 2^31.
//
// A bus of thousands of inputs is one serial walk per lane: correct, not tuned.  The shape that matters is rooms of 2 to 8.
#pragma once
#include "lc3_host_mix_views.h"

// where the pair (s, s + 1) of a view starts: s / nf by the row's multiplier (lc3_mx_div), exact for every s < 2^31
LC3_IV_HD uint64_t lc3_mx_place(const lc3_mx_row &r, uint32_t s) {
    const uint32_t t = lc3_mx_div(s, r.magic);
    const uint32_t n = s - t * (uint32_t)r.nf;
    return r.off + (uint64_t)t * (uint64_t)(uint32_t)r.pitch + (uint64_t)(n * (uint32_t)r.stride);  // (n * stride < 480 * 8)
}
// PLANAR: every row of the bus has pcm_stride 1 (the bus row says so), and no lane tests a stride: without that branch between them the
// loads of a walk's unrolled steps are issued together.  Otherwise the stride is tested row by row (the same for every lane of a workgroup)
template <int PLANAR>
LC3_IV_HD void lc3_mx_load_pair(const int16_t *d, const lc3_mx_row &r, uint32_t s, int32_t &a, int32_t &b) {
    const int16_t *p = d + lc3_mx_place(r, s);
    if (PLANAR || r.stride == 1) {
        uint32_t w;
        __builtin_memcpy(&w, __builtin_assume_aligned(p, 4), 4);
        a = (int16_t)(w & 0xffffu);
        b = (int16_t)(w >> 16);
    } else {
        a = p[0];
        b = p[r.stride];
    }
}
// term(i, s): round to nearest, ties upward (an arithmetic shift)
LC3_IV_HD int32_t lc3_mx_term(int32_t x, int32_t gain) { return (x * gain + 8192) >> 14; }
LC3_IV_HD int32_t lc3_mx_clamp(int32_t v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

// rows_in / rows_out: the bus's own rows (n_in may be 0).  s: even, below the bus's sample count
template <int PLANAR>
LC3_IV_HD void lc3_mix_pair(const lc3_mx_row *rows_in, int n_in, const lc3_mx_row *rows_out, int n_out, const int16_t *pcm_in,
                            int16_t *pcm_out, uint32_t s) {
    int32_t t0 = 0, t1 = 0;
#pragma unroll 4
    for (int i = 0; i < n_in; i++) {
        int32_t a, b;
        lc3_mx_load_pair<PLANAR>(pcm_in, rows_in[i], s, a, b);
        t0 += lc3_mx_term(a, rows_in[i].aux);
        t1 += lc3_mx_term(b, rows_in[i].aux);
    }
    for (int o = 0; o < n_out; o++) {
        const lc3_mx_row &r = rows_out[o];
        int32_t m0 = 0, m1 = 0;
        if (r.aux >= 0) {
            const lc3_mx_row &own = rows_in[r.aux];
            int32_t a, b;
            lc3_mx_load_pair<PLANAR>(pcm_in, own, s, a, b);
            m0 = lc3_mx_term(a, own.aux);
            m1 = lc3_mx_term(b, own.aux);
        }
        const int32_t v0 = lc3_mx_clamp(t0 - m0), v1 = lc3_mx_clamp(t1 - m1);
        int16_t *p = pcm_out + lc3_mx_place(r, s);
        if (PLANAR || r.stride == 1) {
            const uint32_t w = ((uint32_t)v0 & 0xffffu) | ((uint32_t)v1 << 16);
            __builtin_memcpy(__builtin_assume_aligned(p, 4), &w, 4);
        } else {
            p[0] = (int16_t)v0;
            p[r.stride] = (int16_t)v1;
        }
    }
}
// the pair at s of bus b: the form without stride tests where the plan has found every row of the bus planar
LC3_IV_HD void lc3_mix_bus_pair(const lc3_mx_bus &b, const lc3_mx_row *rows_in, const lc3_mx_row *rows_out, const int16_t *pcm_in, int16_t *pcm_out,
                                uint32_t s) {
    if (b.planar) lc3_mix_pair<1>(rows_in + b.first_in, b.n_in, rows_out + b.first_out, b.n_out, pcm_in, pcm_out, s);
    else lc3_mix_pair<0>(rows_in + b.first_in, b.n_in, rows_out + b.first_out, b.n_out, pcm_in, pcm_out, s);
}
