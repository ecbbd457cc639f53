// Frame analysis (lc3gpu_analyze_mixed_views, include/lc3gpu.h): a frame's reconstructed spectrum, its band energies and its total
// energy, ONE LANE PER FRAME.
//
// Everything the decoder does up to the input of its inverse transform (reference decoder/lc3_decoder.rs:99-131) reads the frame and the
// configuration only, so the lane body is the parser's own, unchanged: lc3_parse_frame<1> and lc3_reconstruct_frame
// (lc3_dev_dec_parse.h) into the lane's scratch column, with the configuration as four integers.  What this header adds is the pass
// behind them: the encoder's band-energy formula (reference encoder/modified_dct.rs:140-152) and the sum of squares over the column's
// lines, both in ascending line order, one f32 operation at a time (multiply, divide, add: the unit is compiled without contraction).
//
// The column after lc3_analyze_frame returned 1: words [LC3_PLANE_X, + ne) the spectrum (f32), words [LC3_PLANE_LEV, + 64) the band
// energies (f32, zero from nb on; the level words are free once the frame is parsed).  The lane copies both out from there.
#pragma once
#include "lc3_dev_dec_parse.h"

// what lc3_reconstruct_frame reads of a configuration
struct lc3_an_cfg {
    int ne, fs_ind, n_ms_10, nb;
};

// The energy pass over a reconstructed column.  ifs: the configuration's band index table (nb + 1 entries, ifs[nb] == ne).  want_bands
// (launch-uniform): 0 leaves the band words alone and skips the divisions.  Returns the total energy.
// The lines are fetched four at a time, two groups ahead of their use (as lc3_reconstruct_frame fetches its integers); the band of a line
// follows from the table by stepping, and an empty band (there is none in the standard tables) would get 0.
__device__ __forceinline__ float lc3_analyze_energy(int32_t *plane, const uint16_t *ifs, const lc3_an_cfg &cfg, int want_bands) {
    const int ne = cfg.ne;  // a multiple of 4
    const lc3_f4 *x4 = (const lc3_f4 *)(plane + LC3_PLANE_X);
    float *eb = (float *)(plane + LC3_PLANE_LEV);
    const int last = ne / 4 - 1;
    lc3_f4 cur = x4[0], n1 = x4[1 < last ? 1 : last];
    int bi = 0, band_end = (int)ifs[1];
    float width = (float)(band_end - (int)ifs[0]), e_band = 0.0f, e = 0.0f;
    for (int k0 = 0; k0 < ne; k0 += 4) {
        const int g2 = k0 / 4 + 2;
        const lc3_f4 n2 = x4[g2 < last ? g2 : last];
        // (the four lines spelled out: a line's band is found by stepping, and a group held as an array would live in scratch)
#define LC3_AN_LINE(j, val)                                            \
    do {                                                               \
        const int k = k0 + (j);                                        \
        while (k >= band_end) { /* wave-uniform: a workgroup has one configuration */ \
            if (want_bands) eb[bi] = e_band;                           \
            e_band = 0.0f;                                             \
            bi++;                                                      \
            band_end = (int)ifs[bi + 1];                               \
            width = (float)(band_end - (int)ifs[bi]);                  \
        }                                                              \
        const float sq = (val) * (val);                                \
        e += sq;                                                       \
        if (want_bands) e_band += sq / width;                          \
    } while (0)
        LC3_AN_LINE(0, cur.x);
        LC3_AN_LINE(1, cur.y);
        LC3_AN_LINE(2, cur.z);
        LC3_AN_LINE(3, cur.w);
#undef LC3_AN_LINE
        cur = n1;
        n1 = n2;
    }
    if (want_bands) {
        eb[bi] = e_band;
        for (int b = bi + 1; b < 64; b++) eb[b] = 0.0f;
    }
    return e;
}

// One frame of an analysis call: c.bytes / c.len / c.lookup / c.cf / c.tns / c.plane set by the caller (c.stride = 1, c.dbg = nullptr).
// Returns 1 for a good frame -- the frames lc3_inspect_record gives status 0: the parser's verdict is the inspector's, and the two checks
// lc3_reconstruct_frame still makes (residual bits beyond the frame, more than 480 of them) cannot fail once the side information parsed
// (lc3_dev_dec_inspect.h) -- with the column as described above and the total energy in `energy`; 0 for a frame the decoder would conceal.
__device__ __forceinline__ int lc3_analyze_frame(lc3_parse_ctx &c, const lc3_recon_ctx &r, const lc3_an_cfg &cfg, int want_bands, float &energy) {
    c.head = 0;
    c.tail = 0;
    int ok = lc3_parse_frame<1>(c, cfg.ne, cfg.fs_ind, cfg.n_ms_10) == 0;
    if (ok) ok = lc3_reconstruct_frame(c, r, cfg);
    if (ok) energy = lc3_analyze_energy(c.plane, r.ifs, cfg, want_bands);
    return ok;
}
