// Decoder batches with a frame size per frame (lc3gpu_decode_vbr): what the reference's buf_in.len() is for one frame of one channel
// (decoder/lc3_decoder.rs:85).  The entry of frame (s, t) is nb[s * T + t]; an entry above the slot is treated as 0, and 0 is an empty
// buf_in, which the reference conceals (nbits = 0 in the post-filter's gain).  The size enters the parser (lc3_parse_ctx::len), the
// reconstruction of every form (nbits of the noise level, the residual-bit bound) and the synthesis (the post-filter gain, also for a
// concealed frame).  The decoder has no workgroup barrier after its table staging, so none of these per-frame choices meets one.
#ifndef LC3_DEV_DEC_VBR_H_
#define LC3_DEV_DEC_VBR_H_

__device__ __forceinline__ int lc3_vbr_dec_size(const uint16_t *nb, size_t idx, int slot) {
    const int v = (int)nb[idx];
    return v > slot ? 0 : v;
}

// lc3_decode_stream_wave with a size per frame: nb_row = the stream's T entries, slot = the bound above which an entry reads as 0
LC3_CFG_TEMPLATE_AND(class PROLOGUE = lc3_no_prologue)
__device__ __forceinline__ void lc3_decode_stream_wave_vbr(LC3_CFG_PARAM, lc3_dec_lds &L, int lane, const uint16_t *nb_row, int slot,
                                                           const int32_t *planes, size_t fbase, int n_frames, lc3_dec_state *g, int valid,
                                                           int16_t *pcm0, size_t frame_step, int stride, int late = 0,
                                                           PROLOGUE prologue = PROLOGUE(), int fresh_in_prologue = 0) {
    LC3_CFG_BIND;
    const auto &c0 = c;
    lc3_plane_fetch cur, nxt;
    if (n_frames > 0) lc3_dec_issue_frame(c0, lane, LC3_PLANE_COL(planes, fbase, LC3_PLANE_WORDS), cur, late);
    int t_good = -1, last_ok = 1;
    lc3_ola5 ola = lc3_dec_ola_load(c0, lane, g);
    prologue();
    if (LC3_UNIFORM_I32(fresh_in_prologue)) {
#pragma unroll
        for (int r = 0; r < 5; r++) ola.v[r] = 0.0f;
    }
    for (int t = 0; t < n_frames; t++) {
        const size_t f = fbase + (size_t)t;
        if (t + 1 < n_frames) lc3_dec_issue_frame(c0, lane, LC3_PLANE_COL(planes, f + 1, LC3_PLANE_WORDS), nxt, late);
        int16_t *out = pcm0 + (size_t)t * frame_step;
        const float *plc_src = (t_good >= 0 && !late) ? (const float *)(LC3_PLANE_COL(planes, fbase + (size_t)t_good, LC3_PLANE_WORDS) + LC3_PLANE_X * LC3_PLANE_STRIDE)
                                           : (const float *)g->plc_last_good;
        const int nbytes = lc3_vbr_dec_size(nb_row, (size_t)t, slot);
        last_ok = lc3_decode_frame_wave(LC3_CFG_PASS, L, lane, nbytes, out, cur, g, valid, stride, plc_src, late || t == n_frames - 1, ola, late);
        if (last_ok) t_good = t;
        cur = nxt;
    }
    lc3_dec_ola_store(c0, lane, g, valid, ola);
    if (valid && !last_ok && t_good >= 0 && !late) {
        LC3_HBM_CONST(float) src = (LC3_HBM_CONST(float))(LC3_PLANE_COL(planes, fbase + (size_t)t_good, LC3_PLANE_WORDS) + LC3_PLANE_X * LC3_PLANE_STRIDE);
        for (int k = lane; k < c0.ne; k += LC3_WAVE) g->plc_last_good[k] = src[k];
    }
}

#endif  // LC3_DEV_DEC_VBR_H_
