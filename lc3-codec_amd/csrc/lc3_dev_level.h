// The lane body of lc3gpu_measure_mixed_views (include/lc3gpu.h): one wave, one view, its frames in order.  Compiled by the companion
// library's kernel (lc3gpu_meter.hip) and, unchanged, by the CPU emulation (tests/emu/lc3_emu_meter_views.cpp).
//
//   partial  a lane's share of one frame: sum_sq, sum, min, max, n_clipped, n_cross over the samples the lane owns.  For pcm_stride 1 a lane
//            owns the two samples of 32-bit word `lane + 64 * i` (the contract holds pcm_off and the pitch even and the base 4-byte aligned,
//            and a frame length is even, so a word never straddles a frame); otherwise sample `lane + 64 * i`, a 16-bit access.  A lane that
//            owns sample n reads x[n - 1] ITSELF -- the neighbour element, or for n = 0 the value the wave holds for it (the last sample of
//            the frame before, or the state's `last`) -- so the body has no cross-lane traffic and is the same code in the emulation.
//   combine  integer, associative and commutative: sums add, min and max fold.  The kernel applies it across the wave; the emulation folds
//            the lanes in descending order.
//   finish   ms, the envelope, the gate and the record's eight words, by lane 0.
//
// Widths.  A lane holds up to eight samples (240 words over 64 lanes: four passes of two), and eight squares of -32768 reach 2^33: sum_sq is
// 64 bits in the lane already.  One square is at most 2^30 and fits int32.  sum_sq of a frame is at most 480 * 2^30 < 2^39, |sum| <= 480 *
// 32768 = 15 728 640, ms = sum_sq / nf <= 2^30, |d * k| <= 2^30 * 2^15 = 2^45, and env lies between env0 and ms inclusive, so it stays in
// 0 .. 2^30.
#pragma once
#include "lc3_host_measure_views.h"

struct lc3_lvl_partial {
    uint64_t sum_sq;
    int32_t sum;
    int32_t min, max;
    uint32_t n_clipped, n_cross;
};
// what a wave carries from frame to frame (and, through the channel's record, from call to call)
struct lc3_lvl_state {
    int32_t last;
    uint32_t env;
    int32_t hang;
};

LC3_IV_HD lc3_lvl_partial lc3_lvl_empty() {
    lc3_lvl_partial p;
    p.sum_sq = 0;
    p.sum = 0;
    p.min = 32767;
    p.max = -32768;
    p.n_clipped = 0;
    p.n_cross = 0;
    return p;
}
// one sample x behind the sample before
LC3_IV_HD void lc3_lvl_add(lc3_lvl_partial &p, int32_t x, int32_t before) {
    p.sum_sq += (uint64_t)(uint32_t)(x * x);  // (x * x <= 2^30)
    p.sum += x;
    p.min = x < p.min ? x : p.min;
    p.max = x > p.max ? x : p.max;
    p.n_clipped += (uint32_t)(x == 32767 || x == -32768);
    p.n_cross += (uint32_t)((x < 0) != (before < 0));
}
LC3_IV_HD lc3_lvl_partial lc3_lvl_combine(const lc3_lvl_partial &a, const lc3_lvl_partial &b) {
    lc3_lvl_partial p;
    p.sum_sq = a.sum_sq + b.sum_sq;
    p.sum = a.sum + b.sum;
    p.min = a.min < b.min ? a.min : b.min;
    p.max = a.max > b.max ? a.max : b.max;
    p.n_clipped = a.n_clipped + b.n_clipped;
    p.n_cross = a.n_cross + b.n_cross;
    return p;
}
// lane `lane` (0 .. 63) of the wave's share of the frame whose sample 0 is pcm[base]; before0 = x[-1]
LC3_IV_HD lc3_lvl_partial lc3_lvl_lane(const int16_t *pcm, uint64_t base, int stride, int nf, int lane, int32_t before0) {
    lc3_lvl_partial p = lc3_lvl_empty();
    const int16_t *f = pcm + base;
    if (stride == 1) {
        const int words = nf >> 1;
        for (int w = lane; w < words; w += LC3_MT_WAVE) {
            uint32_t u;
            __builtin_memcpy(&u, f + 2 * w, 4);
            const int32_t x0 = (int16_t)(u & 0xffffu), x1 = (int16_t)(u >> 16);
            const int32_t before = w == 0 ? before0 : (int32_t)f[2 * w - 1];
            lc3_lvl_add(p, x0, before);
            lc3_lvl_add(p, x1, x0);
        }
    } else {
        for (int n = lane; n < nf; n += LC3_MT_WAVE) {
            const int32_t x = f[(size_t)n * (size_t)stride];
            const int32_t before = n == 0 ? before0 : (int32_t)f[(size_t)(n - 1) * (size_t)stride];
            lc3_lvl_add(p, x, before);
        }
    }
    return p;
}
// the last sample of the frame whose sample 0 is pcm[base], at its own placement: the state's `last` after the frame, and x[-1] of the
// view's next frame (every lane reads it itself: one address for the wave)
LC3_IV_HD int32_t lc3_lvl_last(const int16_t *pcm, const lc3_mt_row &r, uint64_t base) {
    return pcm[base + (uint64_t)(uint32_t)((r.nf - 1) * r.stride)];
}
// the frame's whole partial -> its record w[0 .. 7] (the 32 bytes of lc3gpu_level, little-endian) and the state after the frame
LC3_IV_HD void lc3_lvl_finish(const lc3_lvl_partial &p, const lc3_mt_row &r, int32_t last, lc3_lvl_state &st, uint32_t *w) {
    const int64_t ms = (int64_t)(p.sum_sq / (uint64_t)(uint32_t)r.nf);
    const int64_t d = ms - (int64_t)st.env;
    const int64_t k = d > 0 ? r.attack : r.release;
    const uint32_t env = (uint32_t)((int64_t)st.env + ((d * k + 16384) >> 15));
    int32_t hang;
    uint32_t active;
    if (env >= r.threshold) hang = r.hang_frames, active = 1;
    else if (st.hang > 0) hang = st.hang - 1, active = 1;
    else hang = 0, active = 0;
    st.last = last;
    st.env = env;
    st.hang = hang;
    w[0] = (uint32_t)p.sum_sq;
    w[1] = (uint32_t)(p.sum_sq >> 32);
    w[2] = env;
    w[3] = (uint32_t)p.sum;
    w[4] = ((uint32_t)p.min & 0xffffu) | ((uint32_t)p.max << 16);
    w[5] = (p.n_clipped & 0xffffu) | (p.n_cross << 16);
    w[6] = ((uint32_t)hang & 0xffffu) | (active << 16);
    w[7] = 0;
}
