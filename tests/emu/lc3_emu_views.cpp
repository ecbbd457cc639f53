// TEST INFRASTRUCTURE -- the CPU wave emulator for the views calls on mixed-configuration handles (lc3gpu_encode_mixed_views /
// lc3gpu_decode_mixed_views): every item with the placement of its PCM, its frames and its flags.  lc3_emu_mc_items.cpp is included
// unchanged (the emulated handle, the items and mc plans the views plan is compared with); the per-call plan and the host checks are
// lc3_mviews_build / lc3_mviews_check of lc3_host_mixed_list.h, the header the library's host side uses.  The two stream bodies with a
// stride AND a frame pitch, lc3_list_front_stream_view and lc3_list_synth_stream_view (lc3_dev_list.h), run under four emulated waves per
// workgroup as lc3_enc_front_view_items_kernel and lc3_decode_view_items(_late)_kernel call them: stride and pitch come from the stream's
// lc3_view_io row; the back half is the items call's.  The lane-per-frame stages address frame (s, t) as the IOABS = 3 bodies do: bytes
// at byte_off + t * byte_pitch, the flag at flag_off + t * flag_pitch.  Build: tests/test_emu_views.py.
#include "lc3_emu_mc_items.cpp"

namespace {
struct VwJob {
    MlJob j;
    int stride, pitch;
};

void *vw_lane_main(void *arg) {
    VwJob *m = (VwJob *)arg;
    MlJob *j = &m->j;
    tl_wave = j->wave;
    if (j->kind == 1)
        lc3_list_front_stream_view(*j->cfg, j->EL[j->wave], j->lane, j->est, j->fresh, j->valid, j->pcm_s, m->stride, m->pitch, j->mid, j->eplanes,
                                   j->fbase, j->nbytes, j->T, 0, 1);
    else if (j->kind == 2)
        lc3_list_back_stream(*j->cfg, j->EL[j->wave], j->lane, j->est, j->valid, j->mid, j->eplanes, j->fbase, j->nbytes, j->T, 0);
    else
        lc3_list_synth_stream_view(*j->cfg, j->DL[j->wave], j->lane, j->dst, j->fresh, j->valid, j->nbytes, j->dplanes, j->fbase, j->T, j->pcm_out_s,
                                   m->stride, m->pitch, j->late);
    return 0;
}

void run_wg_vw(const VwJob *protos) {
    static pthread_t th[LC3_WG_WAVES * LC3_WAVE];
    static VwJob jobs[LC3_WG_WAVES * LC3_WAVE];
    for (int w = 0; w < LC3_WG_WAVES; w++) pthread_barrier_init(&g_wave_bar[w], 0, LC3_WAVE);
    pthread_barrier_init(&g_wg_bar, 0, LC3_WG_WAVES * LC3_WAVE);
    for (int w = 0; w < LC3_WG_WAVES; w++)
        for (int i = 0; i < LC3_WAVE; i++) {
            VwJob &q = jobs[w * LC3_WAVE + i];
            q = protos[w];
            q.j.lane = i;
            q.j.wave = w;
            pthread_create(&th[w * LC3_WAVE + i], 0, vw_lane_main, &q);
        }
    for (int i = 0; i < LC3_WG_WAVES * LC3_WAVE; i++) pthread_join(th[i], 0);
    for (int w = 0; w < LC3_WG_WAVES; w++) pthread_barrier_destroy(&g_wave_bar[w]);
    pthread_barrier_destroy(&g_wg_bar);
}

void run_stream_kernel_vw(const MlCtx &x, const lc3_groups &G, unsigned wg_stream, const int32_t *entries, const lc3_view_io *rows, MlJob j,
                          const int16_t *pcm, int16_t *pcm_out, float *mid, int32_t *eplanes, const int32_t *dplanes) {
    for (unsigned wg = 0; wg < wg_stream; wg++) {
        const lc3_group &g = G.g[find_group(G, wg)];
        const MlGroup &mgp = cfg_of_row(x, g);
        VwJob protos[LC3_WG_WAVES];
        if (j.EL) memset(j.EL, 0xFF, LC3_WG_WAVES * sizeof(lc3_enc_lds));
        if (j.DL) memset(j.DL, 0xFF, LC3_WG_WAVES * sizeof(lc3_dec_lds));
        for (int w = 0; w < LC3_WG_WAVES; w++) {
            const int s_raw = (int)(wg - (unsigned)g.wg_stream) * LC3_WG_WAVES + w;
            const int valid = s_raw < g.n_streams;
            const int s = valid ? s_raw : g.n_streams - 1;
            const int pos = g.first_stream + s;
            const int entry = lc3_list_entry(entries, pos);
            MlJob &q = protos[w].j;
            q = j;
            q.cfg = &mgp.cfg;
            q.valid = valid;
            q.fresh = lc3_list_fresh(entry);
            q.nbytes = g.nbytes;
            q.T = g.n_frames;
            q.fbase = (size_t)s * (size_t)g.n_frames;
            q.est = x.est + lc3_list_channel(entry);
            q.dst = x.dst + lc3_list_channel(entry);
            q.pcm_s = pcm ? pcm + (size_t)rows[pos].pcm_off : nullptr;
            q.pcm_out_s = pcm_out ? pcm_out + (size_t)rows[pos].pcm_off : nullptr;
            q.mid = mid ? mid + (size_t)g.frame_base * (size_t)MP_WORDS : nullptr;
            q.eplanes = eplanes ? eplanes + (size_t)g.frame_base * (size_t)EP_WORDS : nullptr;
            q.dplanes = dplanes ? dplanes + (size_t)g.frame_base * (size_t)LC3_PLANE_WORDS : nullptr;
            protos[w].stride = lc3_list_entry(&rows[pos].stride, 0);
            protos[w].pitch = lc3_list_entry(&rows[pos].pcm_pitch, 0);
        }
        run_wg_vw(protos);
    }
}

struct VwPlan {
    std::vector<int32_t> entries;
    std::vector<lc3_view_io> rows;
    ItPlan it;  // (P only: it_info reads it)
};
void vw_plan(const MlCtx &x, const lc3_mview *views, int n, int use_flags, const uint8_t *fresh, VwPlan &p) {
    std::vector<uint8_t> fr((size_t)x.N, 0);
    for (int c = 0; c < x.N; c++) fr[(size_t)x.ms[(size_t)c].internal] = fresh[c];
    p.entries.assign((size_t)n, 0);
    p.rows.assign((size_t)n, lc3_view_io());
    lc3_mviews_build(x.mg.data(), x.ms.data(), fr.data(), views, n, use_flags, p.entries.data(), p.rows.data(), p.it.P);
}
}  // namespace

extern "C" {
int lc3emu_vw_view_size() { return (int)sizeof(lc3_mview); }
int lc3emu_vw_row_size() { return (int)sizeof(lc3_view_io); }

// lc3_mviews_check as the library calls it.  views: lc3gpu_view[n].  Returns its code
int lc3emu_vw_check(void *h, const void *views, int n, uint64_t pcm_base, uint64_t pcm_elems, uint64_t io_bytes, uint64_t n_flags, int use_flags,
                    int min_bytes) {
    MlCtx &x = *(MlCtx *)h;
    std::vector<uint32_t> seen((size_t)x.N, 0u);
    const lc3_mviews_bounds B = {pcm_base, pcm_elems, io_bytes, n_flags, use_flags, min_bytes};
    size_t frames = 0;
    int most = 0;
    return lc3_mviews_check(x.mg.data(), x.ms.data(), x.N, (const lc3_mview *)views, n, B, seen.data(), 1u, &frames, &most);
}

// The plan alone (host only).  rows int32[n_buckets][8] as lc3emu_it_plan; tab_of int64[n][8] by VIEW: launch position, pcm_off, byte_off,
// flag_off, stride, pcm_pitch, byte_pitch, flag_pitch of its row.  Returns the number of buckets
int lc3emu_vw_plan(void *h, const void *views_, int n, int use_flags, int32_t *rows, int max_buckets, int64_t *tab_of) {
    MlCtx &x = *(MlCtx *)h;
    const lc3_mview *views = (const lc3_mview *)views_;
    std::vector<uint8_t> fresh((size_t)x.N, 0);
    VwPlan p;
    vw_plan(x, views, n, use_flags, fresh.data(), p);
    if ((int)p.it.P.buckets.size() > max_buckets) return -1;
    int nb = 0;
    for (int k = 0; k < lc3_mitems_sets(p.it.P); k++) {
        int b0, b1;
        lc3_mitems_set(p.it.P, k, b0, b1);
        lc3_groups G;
        unsigned ws, wf;
        lc3_mitems_rows(x.mg.data(), p.it.P, b0, b1, LC3_WG_WAVES, 64u, G, ws, wf);
        for (int r = 0; r < G.n; r++, nb++) {
            const lc3_group &g = G.g[r];
            const int32_t row[8] = {k, r, g.slot, g.nbytes, g.n_frames, g.first_stream, g.n_streams, (int32_t)g.frame_base};
            memcpy(rows + 8 * nb, row, sizeof row);
        }
    }
    for (int i = 0; i < n; i++) {
        const int internal = x.ms[(size_t)views[i].channel].internal;
        for (int pos = 0; pos < n; pos++)
            if (lc3_list_channel(p.entries[(size_t)pos]) == internal) {
                const lc3_view_io &t = p.rows[(size_t)pos];
                const int64_t row[8] = {pos, t.pcm_off, t.byte_off, t.flag_off, t.stride, t.pcm_pitch, t.byte_pitch, t.flag_pitch};
                memcpy(tab_of + 8 * i, row, sizeof row);
            }
    }
    return nb;
}

// views lc3gpu_view[n] (already checked); pcm / bytes: the caller's whole buffers, read and written where the views say
int lc3emu_vw_encode(void *h, const void *views, int n, const uint8_t *fresh, const int16_t *pcm, uint8_t *bytes, int32_t *info) {
    MlCtx &x = *(MlCtx *)h;
    VwPlan p;
    vw_plan(x, (const lc3_mview *)views, n, 0, fresh, p);
    const lc3_mitems_plan &P = p.it.P;
    const size_t frames = (size_t)P.frames, cols = frames + SPARE;
    std::vector<int32_t> planes(cols * EP_WORDS, (int32_t)PATTERN);
    std::vector<uint32_t> midw(cols * MP_WORDS, PATTERN);
    float *mid = (float *)midw.data();
    lc3_enc_lds *L = (lc3_enc_lds *)aligned_alloc(16, LC3_WG_WAVES * sizeof(lc3_enc_lds));
    std::vector<uint32_t> cf(64 * 17);
    for (int q = 0; q < 64; q++)
        for (int r = 0; r < 17; r++) cf[(size_t)q * 17 + r] = (uint32_t)(int)LC3T_AC_SPEC_CUMFREQ[q][r] | ((uint32_t)(int)LC3T_AC_SPEC_FREQ[q][r] << 16);
    static uint32_t tns_models[LC3_TNS_MODEL_WORDS];
    for (int i = 0; i < LC3_TNS_MODEL_WORDS; i++) tns_models[i] = lc3_tns_model_word(i);
    unsigned wgs = 0;
    for (int stage = 0; stage < 4; stage++)
        for (int k = 0; k < lc3_mitems_sets(P); k++) {
            int b0, b1;
            lc3_mitems_set(P, k, b0, b1);
            lc3_groups G;
            unsigned wg_stream, wg_frame;
            lc3_mitems_rows(x.mg.data(), P, b0, b1, LC3_WG_WAVES, 64u, G, wg_stream, wg_frame);
            MlJob j;
            memset(&j, 0, sizeof(j));
            j.EL = L;
            if (stage == 0) {  // lc3_enc_front_view_items_kernel
                j.kind = 1;
                wgs += wg_stream;
                run_stream_kernel_vw(x, G, wg_stream, p.entries.data(), p.rows.data(), j, pcm, nullptr, mid, planes.data(), nullptr);
            } else if (stage == 1) {  // lc3_sns_vq_items_kernel
                for (int gi = 0; gi < G.n; gi++) {
                    const lc3_group &g = G.g[gi];
                    for (size_t fl = 0; fl < (size_t)g.n_streams * (size_t)g.n_frames; fl++) {
                        const size_t f = (size_t)g.frame_base + fl;
                        lc3_vq_ctx v;
                        v.mid = mid + f * (size_t)MP_WORDS;
                        v.gains = mid + f * (size_t)MP_WORDS + MP_G;
                        v.plane = LC3_PLANE_COL(planes.data(), f, EP_WORDS);
                        v.stride = LC3_PLANE_STRIDE;
                        v.mpvq = &LC3T_MPVQ_OFFSETS[0][0];
                        v.nb = g.nb;
                        v.spec_flags = 0;
                        lc3_sns_vq_frame(v);
                    }
                }
            } else if (stage == 2) {  // lc3_enc_back_items_kernel (plane columns only: stride and pitch are not used)
                j.kind = 2;
                run_stream_kernel_vw(x, G, wg_stream, p.entries.data(), p.rows.data(), j, nullptr, nullptr, mid, planes.data(), nullptr);
            } else {  // lc3_pack_view_items_kernel
                for (int gi = 0; gi < G.n; gi++) {
                    const lc3_group &g = G.g[gi];
                    const size_t T = (size_t)g.n_frames;
                    for (size_t fl = 0; fl < (size_t)g.n_streams * T; fl++) {
                        const size_t f = (size_t)g.frame_base + fl, s = fl / T, t = fl % T;
                        const lc3_view_io &io = p.rows[(size_t)g.first_stream + s];
                        lc3_pack_ctx c;
                        uint8_t sink = 0;
                        std::vector<uint8_t> frame((size_t)g.nbytes, 0);  // (the kernel packs into LDS and copies the frame's own bytes out)
                        c.buf = frame.data();
                        c.sink = &sink;
                        c.tns = tns_models;
                        c.nbytes = g.nbytes;
                        c.lookup = LC3T_AC_SPEC_LOOKUP;
                        c.cf = cf.data();
                        c.plane = LC3_PLANE_COL(planes.data(), f, EP_WORDS);
                        c.stride = LC3_PLANE_STRIDE;
                        lc3_pack_frame(c, g.ne);
                        memcpy(bytes + (size_t)io.byte_off + t * (size_t)io.byte_pitch, frame.data(), (size_t)g.nbytes);
                    }
                }
            }
        }
    free(L);
    int changed = 0;
    for (size_t i = frames * EP_WORDS; i < planes.size(); i++) changed += planes[i] != (int32_t)PATTERN;
    for (size_t i = frames * MP_WORDS; i < midw.size(); i++) changed += midw[i] != PATTERN;
    it_info(p.it, changed, 0, wgs, info);
    return 0;
}

// bytes / bad (or NULL) / pcm: the caller's whole buffers; late as lc3emu_ml_decode
int lc3emu_vw_decode(void *h, const void *views, int n, const uint8_t *fresh, const uint8_t *bytes, const uint8_t *bad, int16_t *pcm, int late,
                     int32_t *info) {
    MlCtx &x = *(MlCtx *)h;
    VwPlan p;
    vw_plan(x, (const lc3_mview *)views, n, bad != nullptr, fresh, p);
    const lc3_mitems_plan &P = p.it.P;
    const size_t frames = (size_t)P.frames, cols = frames + SPARE;
    std::vector<int32_t> planes(cols * LC3_PLANE_WORDS, (int32_t)PATTERN);
    alignas(16) static uint32_t cf[64 * LC3_DCF_ROW_WORDS];
    for (int i = 0; i < 64 * LC3_DCF_ROW_WORDS; i++) cf[i] = lc3_dcf_word(i);
    std::vector<uint32_t> tns(LC3_TNS_MODEL_WORDS);
    for (int i = 0; i < LC3_TNS_MODEL_WORDS; i++) tns[(size_t)i] = lc3_tns_model_word(i);
    lc3_dec_lds *L = (lc3_dec_lds *)aligned_alloc(16, LC3_WG_WAVES * sizeof(lc3_dec_lds));
    unsigned wgs = 0;
    for (int stage = 0; stage < 2; stage++)
        for (int k = 0; k < lc3_mitems_sets(P); k++) {
            int b0, b1;
            lc3_mitems_set(P, k, b0, b1);
            lc3_groups G;
            unsigned wg_stream, wg_frame;
            lc3_mitems_rows(x.mg.data(), P, b0, b1, LC3_WG_WAVES, 64u, G, wg_stream, wg_frame);
            if (stage == 0) {  // lc3_parse_view_items_kernel
                for (int gi = 0; gi < G.n; gi++) {
                    const lc3_group &g = G.g[gi];
                    const lc3_cfg &c = cfg_of_row(x, g).cfg;
                    const size_t T = (size_t)g.n_frames;
                    for (size_t fl = 0; fl < (size_t)g.n_streams * T; fl++) {
                        const size_t f = (size_t)g.frame_base + fl, s = fl / T, t = fl % T;
                        const lc3_view_io &io = p.rows[(size_t)g.first_stream + s];
                        lc3_parse_ctx q;
                        q.dbg = nullptr;
                        q.tns = tns.data();
                        q.bytes = bytes + (size_t)io.byte_off + t * (size_t)io.byte_pitch;
                        q.len = g.nbytes;
                        q.lookup = LC3T_AC_SPEC_LOOKUP;
                        q.cf = cf;
                        q.plane = LC3_PLANE_COL(planes.data(), f, LC3_PLANE_WORDS);
                        q.stride = LC3_PLANE_STRIDE;
                        q.head = 0;
                        q.tail = 0;
                        const int rc = (bad && bad[(size_t)io.flag_off + t * (size_t)io.flag_pitch]) ? -100 : lc3_parse_frame<1>(q, c.ne, c.fs_ind, c.n_ms_10);
                        int ok = rc == 0;
                        if (ok && late) {
                            ok = lc3_reconstruct_prepare_late(q);
                        } else if (ok) {
                            float scf[16];
                            lc3_recon_ctx r;
                            r.scf = scf;
                            r.sstride = 1;
                            r.mpvq = &LC3T_MPVQ_OFFSETS[0][0];
                            r.ifs = lc3_band_index(c);
                            ok = lc3_reconstruct_frame(q, r, c, nullptr);
                        }
                        lc3_px_set(q, AD_OK, ok);
                    }
                }
            } else {  // lc3_decode_view_items_kernel / lc3_decode_view_items_late_kernel
                MlJob j;
                memset(&j, 0, sizeof(j));
                j.DL = L;
                j.late = late ? 1 : 0;
                j.kind = 3;
                wgs += wg_stream;
                run_stream_kernel_vw(x, G, wg_stream, p.entries.data(), p.rows.data(), j, nullptr, pcm, nullptr, nullptr, planes.data());
            }
        }
    free(L);
    int changed = 0;
    for (size_t i = frames * LC3_PLANE_WORDS; i < planes.size(); i++) changed += planes[i] != (int32_t)PATTERN;
    it_info(p.it, changed, 0, wgs, info);
    return 0;
}
}
