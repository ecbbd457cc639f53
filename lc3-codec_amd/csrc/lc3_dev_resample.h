// The lane body of lc3gpu_resample_mixed_views (include/lc3gpu.h): one workgroup, one chunk of LC3_RS_CHUNK consecutive output samples of
// one view, in three phases with a barrier between them.  Compiled by the companion library's kernel (lc3gpu_resampler.hip) and, unchanged,
// by the CPU emulation (tests/emu/lc3_emu_resample_views.cpp), which runs every lane of a phase before the next phase begins.
//
//   stage    the chunk's input window -- x[b0 - (T - 1)] .. x[b_last], the samples before 0 from the channel's history (or zeros) -- into
//            LDS as int16, a PAIR of samples per lane and step: a frame length is even, so a pair (k, k + 1), k even, never straddles a
//            frame; for pcm_stride 1 the pair is ONE 32-bit access (the contract holds pcm_off and the pitch even and the base 4-byte
//            aligned), otherwise two 16-bit ones.  And the ratio's table, widened to int32 and TRANSPOSED to [j][p]: lanes of one step differ
//            in their phase p, and at one tap j their L coefficients lie in L consecutive banks.
//   compute  one output sample per lane per step: acc = sum_j c[p][j] * x[b - j] in int32 by plain multiply-adds, rounded, shifted and
//            clamped, into the chunk's output samples in LDS.
//   store    the output samples as pairs again, 32-bit stores for pcm_stride 1; and the workgroup of chunk 0 writes the channel's NEW
//            history, into the buffer no workgroup of this launch reads (lc3_host_resample_views.h).
//
// The bound that keeps acc in int32: every phase's sum |c| <= 65535 (the committed table's worst is 60988; tests/test_resample_tables.py
// holds it), so |acc| <= 32768 * 65535 < 2^31 - 16384, and the rounding add cannot wrap either.
//
// LDS reads of the inner loop: the window is read 16 bits at a time at a lane stride of M / L samples (1 / 6 .. 6): lanes that share a
// sample or a word are served together, a stride of 2 or 6 samples is conflict-free, a stride of 4 samples (32 -> 8 kHz) is 2-way.
#pragma once
#include "lc3_host_resample_views.h"

struct lc3_rs_lds {
    int32_t coef[LC3_RS_MAX_COEF];     // [j][p]
    int16_t win[LC3_RS_MAX_WINDOW];    // win[i] = x[kw0 + i]
    int16_t out[LC3_RS_CHUNK];
};

// what every phase derives from the row and the chunk's number (the same for every lane of the workgroup)
struct lc3_rs_chunk {
    int m0, n_out;  // the chunk's first output sample and how many it holds (1 .. LC3_RS_CHUNK)
    int b0;         // the input sample under output m0's tap 0 (phase 0)
    int kw0;        // the window's first input sample: b0 - (T - 1) rounded down to even (may be negative: history)
    int n_pairs;    // pairs of the window
};
LC3_IV_HD lc3_rs_chunk lc3_rs_chunk_of(const lc3_rs_row &r, int chunk) {
    lc3_rs_chunk c;
    c.m0 = chunk * LC3_RS_CHUNK;  // (below S_out <= 2^31 - 1)
    const int left = r.S_out - c.m0;
    c.n_out = left < LC3_RS_CHUNK ? left : LC3_RS_CHUNK;
    c.b0 = chunk * (int)lc3_rs_div_l((uint32_t)(LC3_RS_CHUNK * r.M), r.inv);  // (m0 * M / L exactly: below S_in)
    c.kw0 = (c.b0 - (r.T - 1)) & ~1;
    const int b_last = c.b0 + (int)lc3_rs_div_l((uint32_t)((c.n_out - 1) * r.M), r.inv);
    c.n_pairs = (b_last - c.kw0 + 2) >> 1;
    return c;
}
LC3_IV_HD int32_t lc3_rs_clamp(int32_t v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

// x[k] for k < 0: the channel's history (hist[T - 1 + k]), zeros when fresh and for the one sample before an odd-length history
LC3_IV_HD int16_t lc3_rs_before(const lc3_rs_row &r, const int16_t *hist, int k) {
    const int i = r.T - 1 + k;
    return (r.hist_rd < 0 || i < 0) ? (int16_t)0 : hist[r.hist_rd + i];
}

LC3_IV_HD void lc3_rs_stage(const lc3_rs_row &r, const lc3_rs_chunk &c, int tid, lc3_rs_lds &lds, const int16_t *pcm_in, const int16_t *hist) {
    // the table: coef[j * L + p] = c[p][j]
    const int n_coef = r.L * r.T;
    if (r.coef_off < 0) {
        if (tid == 0) lds.coef[0] = 32768;  // a copy: (32768 * x + 16384) >> 15 == x
    } else {
        for (int i = tid; i < n_coef; i += LC3_RS_LANES) {
            int p = 0, j = i;
            while (j >= r.T) j -= r.T, p++;  // (p < L <= 6)
            lds.coef[j * r.L + p] = lc3_rs_coef[r.coef_off + i];
        }
    }
    for (int i = tid; i < c.n_pairs; i += LC3_RS_LANES) {
        const int k = c.kw0 + 2 * i;  // even
        int16_t a, b;
        if (k < 0) {
            a = lc3_rs_before(r, hist, k);
            b = lc3_rs_before(r, hist, k + 1);
        } else if (k < r.S_in) {  // (S_in is even: k + 1 < S_in too)
            const int16_t *p = pcm_in + lc3_rs_place(r.in_off, r.in_magic, r.nf_in, r.in_pitch, r.in_stride, (uint32_t)k);
            if (r.in_stride == 1) {
                uint32_t w;
                __builtin_memcpy(&w, __builtin_assume_aligned(p, 4), 4);
                a = (int16_t)(w & 0xffffu);
                b = (int16_t)(w >> 16);
            } else {
                a = p[0];
                b = p[r.in_stride];
            }
        } else {
            a = b = 0;  // (no output of the view reaches beyond its input)
        }
        lds.win[2 * i] = a;
        lds.win[2 * i + 1] = b;
    }
}

LC3_IV_HD void lc3_rs_compute(const lc3_rs_row &r, const lc3_rs_chunk &c, int tid, lc3_rs_lds &lds) {
    const int d = c.b0 - c.kw0;  // T - 1 or T: where x[b0] lies in the window
    for (int ml = tid; ml < c.n_out; ml += LC3_RS_LANES) {
        const uint32_t u = (uint32_t)(ml * r.M);
        const int q = (int)lc3_rs_div_l(u, r.inv), p = (int)u - q * r.L;
        const int16_t *x = lds.win + d + q;
        const int32_t *cf = lds.coef + p;
        int32_t acc = 0;
#pragma unroll 4
        for (int j = 0; j < r.T; j++) acc += cf[j * r.L] * (int32_t)x[-j];
        lds.out[ml] = (int16_t)lc3_rs_clamp((acc + 16384) >> 15);
    }
}

LC3_IV_HD void lc3_rs_store(const lc3_rs_row &r, const lc3_rs_chunk &c, int chunk, int tid, const lc3_rs_lds &lds, const int16_t *pcm_in,
                            int16_t *pcm_out, int16_t *hist) {
    for (int i = tid; 2 * i < c.n_out; i += LC3_RS_LANES) {  // (n_out is even: S_out and LC3_RS_CHUNK are)
        int16_t *p = pcm_out + lc3_rs_place(r.out_off, r.out_magic, r.nf_out, r.out_pitch, r.out_stride, (uint32_t)(c.m0 + 2 * i));
        const int16_t v0 = lds.out[2 * i], v1 = lds.out[2 * i + 1];
        if (r.out_stride == 1) {
            const uint32_t w = ((uint32_t)(uint16_t)v0) | ((uint32_t)(uint16_t)v1 << 16);
            __builtin_memcpy(__builtin_assume_aligned(p, 4), &w, 4);
        } else {
            p[0] = v0;
            p[r.out_stride] = v1;
        }
    }
    // the new history: the last T - 1 samples of (old history ++ x)
    if (chunk == 0) {
        for (int i = tid; i < r.T - 1; i += LC3_RS_LANES) {
            const int k = r.S_in - (r.T - 1) + i;
            hist[r.hist_wr + i] =
                k < 0 ? lc3_rs_before(r, hist, k) : pcm_in[lc3_rs_place(r.in_off, r.in_magic, r.nf_in, r.in_pitch, r.in_stride, (uint32_t)k)];
        }
    }
}
