// Encoder batches with a frame size per frame (lc3gpu_encode_vbr): what the reference's buf_out.len() is for one frame of one channel
// (encoder/lc3_encoder.rs:65, "may change per call").  The uniform kernels take one launch-wide nbytes; the sized kernels read the
// size of frame (s, t) from the caller's table nb[s * T + t] and hand it to the SAME stage functions -- the size enters
//   front half   lc3_enc_attack (detector activation) and lc3_enc_ltpf (gain_ltpf_on), through lc3_encode_front_wave's nbytes
//   back half    lc3_enc_tns_lev (lpc_weighting of a chunk), lc3_enc_tns_apply / lc3_enc_quant / residual bits (lc3_encode_back_analyse)
//   packer       lc3_pack_ctx::nbytes per lane
// Barrier rule: the only workgroup barriers of the encoder are the gathered blocks of the LTPF stage (LC3_SERIAL_BEGIN/END), which run for
// the four streams of a workgroup at once.  Four streams of one workgroup may have four sizes in one frame, so no size-dependent branch
// may hold such a block unless its condition is the same for the whole workgroup.  The one such branch is the normalised-correlation
// shortcut (skip_nc, bit 8 of ltpf_phase): lc3_vbr_front_phase sets that bit only when EVERY stream of the workgroup keeps the filter off
// at frames t, t + 1 and t + 2 (the frames whose decisions read frame t's nc, through mem_nc / mem_mem_nc).  The back half has no
// workgroup barrier after its table staging; its size-dependent choices (the TNS chunk split below) are per wave.
#ifndef LC3_DEV_ENC_VBR_H_
#define LC3_DEV_ENC_VBR_H_

#define LC3_VBR_MIN_BYTES 20

// frame (s, t)'s size clamped into [20, slot]; *clamped = 1 when the table's entry lay outside
__device__ __forceinline__ int lc3_vbr_enc_size(const uint16_t *nb, size_t idx, int slot, int *clamped) {
    const int v = (int)nb[idx];
    const int lo = LC3_VBR_MIN_BYTES;
    *clamped = v < lo || v > slot;
    return v < lo ? lo : (v > slot ? slot : v);
}
__device__ __forceinline__ int lc3_vbr_enc_size(const uint16_t *nb, size_t idx, int slot) {
    int unused;
    return lc3_vbr_enc_size(nb, idx, slot, &unused);
}

// lc3_enc_ltpf's gain_ltpf_on for a frame of `nbytes` (long_term_post_filter.rs:143-146)
template <class CC>
__device__ __forceinline__ int lc3_vbr_gain_ltpf_on(const CC &c, int nbytes) {
    const int nbits = nbytes * 8;
    int t_nbits = nbits;
    if (!c.n_ms_10) {
        double v = (double)nbits * 10.0 / 7.5;
        t_nbits = (int)(v + 0.5);
    }
    return t_nbits < 560 + c.fs_ind * 80;
}

// ltpf_phase of frame t (as lc3_enc_front_body): the frame's number modulo the workgroup's waves, and bit 8 only where it is workgroup-
// uniformly safe to skip the normalised correlation.  wg_s0: the workgroup's first stream in the launch; n_streams: the launch's streams
// (the shadow waves of a partial workgroup run the last stream's sizes).  Every wave computes the same value from the same table words.
template <class CC>
__device__ __forceinline__ int lc3_vbr_front_phase(const CC &c, const uint16_t *nb, int slot, int wg_s0, int n_streams, int t, int n_frames,
                                                   int n_waves) {
    int phase = t % n_waves;
    if (t + 2 >= n_frames) return phase;  // the last two frames' nc is what the state keeps for the next launch
    int off = 0;
    for (int w = 0; w < n_waves; w++) {
        const int s_raw = wg_s0 + w, s = s_raw < n_streams ? s_raw : n_streams - 1;
        for (int u = t; u <= t + 2; u++) off |= lc3_vbr_gain_ltpf_on(c, lc3_vbr_enc_size(nb, (size_t)s * (size_t)n_frames + (size_t)u, slot));
    }
    return phase + (off ? 0 : 0x100);
}

// lpc_weighting of lc3_enc_tns_lev / lc3_enc_tns_apply for a frame of `nbytes`
template <class CC>
__device__ __forceinline__ int lc3_vbr_lpc_weighting(const CC &c, int nbytes) {
    const int nbits = nbytes * 8;
    return c.n_ms_10 ? (nbits < 480) : (nbits < 360);
}

// lc3_encode_back_stream with a size per frame: nb_row = the stream's T sizes (already offset to the stream), slot = the clamp bound.
// A chunk of the TNS recursions runs with ONE nbits, which only matters through lpc_weighting: a chunk is cut where the weighting changes,
// so every frame of it has its own weighting.  (A chunk's length only decides how the work is grouped, not what it computes.)
LC3_CFG_TEMPLATE __device__ __forceinline__ void lc3_encode_back_stream_vbr(LC3_CFG_PARAM, lc3_enc_lds &L, int lane, const float *mid,
                                                                           int32_t *planes, size_t fbase, int n_frames, const uint16_t *nb_row,
                                                                           int slot, int store, float *dbg) {
    LC3_CFG_BIND;
    lc3_mid_fetch cur, nxt;
    if (n_frames > 0) lc3_mid_issue(c, lane, mid + fbase * (size_t)MP_WORDS, cur);
    nxt = cur;
    for (int t0 = 0; t0 < n_frames;) {
        const int nb0 = lc3_vbr_enc_size(nb_row, (size_t)t0, slot);
        const int w0 = lc3_vbr_lpc_weighting(c, nb0);
        int nc = 1;
        while (nc < LC3_TNS_CHUNK && t0 + nc < n_frames && lc3_vbr_lpc_weighting(c, lc3_vbr_enc_size(nb_row, (size_t)(t0 + nc), slot)) == w0) nc++;
        if (nc > 1) {
            for (int u = 0; u < nc; u++) {
                const int tn = u + 1 < nc ? t0 + u + 1 : t0;
                lc3_mid_issue(c, lane, mid + (fbase + (size_t)tn) * (size_t)MP_WORDS, nxt);
                lc3_encode_back_pickup(LC3_CFG_PASS, L, lane, cur);
                lc3_enc_tns_acf(LC3_CFG_PASS, LC3_LDS_PASS lane, L.ism[MPF_BW], L.ism[MPF_NEAR_NYQUIST], u);
                cur = nxt;
            }
            lc3_enc_tns_lev(LC3_CFG_PASS, LC3_LDS_PASS lane, nb0 * 8, nc);
        }
        for (int u = 0; u < nc; u++) {
            const int t = t0 + u;
            const int nbt = lc3_vbr_enc_size(nb_row, (size_t)t, slot);
            if (t + 1 < n_frames) lc3_mid_issue(c, lane, mid + (fbase + (size_t)t + 1) * (size_t)MP_WORDS, nxt);
            lc3_encode_back_pickup(LC3_CFG_PASS, L, lane, cur);
            if (nc == 1) {
                lc3_enc_tns_acf(LC3_CFG_PASS, LC3_LDS_PASS lane, L.ism[MPF_BW], L.ism[MPF_NEAR_NYQUIST], 0);
                lc3_enc_tns_lev(LC3_CFG_PASS, LC3_LDS_PASS lane, nbt * 8, 1);
            }
            const lc3_back_res r = lc3_encode_back_analyse(LC3_CFG_PASS, L, lane, nbt, u, dbg);
            lc3_encode_back_store(LC3_CFG_PASS, L, lane, r, LC3_PLANE_COL(planes, fbase + (size_t)t, EP_WORDS), LC3_PLANE_STRIDE, store, dbg);
            cur = nxt;
        }
        t0 += nc;
    }
}

#endif  // LC3_DEV_ENC_VBR_H_
