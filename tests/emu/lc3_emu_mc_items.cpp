// TEST INFRASTRUCTURE -- the CPU wave emulator for the multi-channel items calls on mixed-configuration handles
// (lc3gpu_encode_mixed_mc_items / lc3gpu_decode_mixed_mc_items): WAV sample order in, the channels' frames back to back out.
// lc3_emu_items.cpp is included unchanged (the emulated handle, the rows, the lane-per-frame stage loops' ingredients); the per-call plan
// is lc3_mcitems_build of lc3_host_mixed_list.h, the header the library's host side builds it with.  The two stream bodies with a sample
// stride, lc3_list_front_stream_mc and lc3_list_synth_stream_mc (lc3_dev_list.h), run under four emulated waves per workgroup as
// lc3_enc_front_mc_items_kernel and lc3_decode_mc_items(_late)_kernel call them: the stride is the table row's spare word, read per
// stream, so the four waves of a workgroup may run at strides 1, 2 and 3 side by side; the back half is the items call's.  The lane-per-
// frame stages address frame (s, t) as the IOABS = 2 bodies do: bytes at byte_off1 + t * C * nbytes, the flag at flag_idx + t * C.
// A workgroup barrier steered by the stride deadlocks here, which the test turns into a failure with a time limit.
// Build: tests/test_emu_mc_items.py.
#include "lc3_emu_items.cpp"

namespace {
struct McJob {
    MlJob j;
    int stride;
};

void *mc_lane_main(void *arg) {
    McJob *m = (McJob *)arg;
    MlJob *j = &m->j;
    tl_wave = j->wave;
    if (j->kind == 1)
        lc3_list_front_stream_mc(*j->cfg, j->EL[j->wave], j->lane, j->est, j->fresh, j->valid, j->pcm_s, m->stride, j->mid, j->eplanes, j->fbase,
                                 j->nbytes, j->T, 0, 1);
    else if (j->kind == 2)
        lc3_list_back_stream(*j->cfg, j->EL[j->wave], j->lane, j->est, j->valid, j->mid, j->eplanes, j->fbase, j->nbytes, j->T, 0);
    else
        lc3_list_synth_stream_mc(*j->cfg, j->DL[j->wave], j->lane, j->dst, j->fresh, j->valid, j->nbytes, j->dplanes, j->fbase, j->T, j->pcm_out_s,
                                 m->stride, j->late);
    return 0;
}

void run_wg_mc(const McJob *protos) {
    static pthread_t th[LC3_WG_WAVES * LC3_WAVE];
    static McJob jobs[LC3_WG_WAVES * LC3_WAVE];
    for (int w = 0; w < LC3_WG_WAVES; w++) pthread_barrier_init(&g_wave_bar[w], 0, LC3_WAVE);
    pthread_barrier_init(&g_wg_bar, 0, LC3_WG_WAVES * LC3_WAVE);
    for (int w = 0; w < LC3_WG_WAVES; w++)
        for (int i = 0; i < LC3_WAVE; i++) {
            McJob &q = jobs[w * LC3_WAVE + i];
            q = protos[w];
            q.j.lane = i;
            q.j.wave = w;
            pthread_create(&th[w * LC3_WAVE + i], 0, mc_lane_main, &q);
        }
    for (int i = 0; i < LC3_WG_WAVES * LC3_WAVE; i++) pthread_join(th[i], 0);
    for (int w = 0; w < LC3_WG_WAVES; w++) pthread_barrier_destroy(&g_wave_bar[w]);
    pthread_barrier_destroy(&g_wg_bar);
}

// strides[k] counts the workgroups that held k different strides among their valid waves
void run_stream_kernel_mc(const MlCtx &x, const lc3_groups &G, unsigned wg_stream, const int32_t *entries, const lc3_stream_io *tab, MlJob j,
                          const int16_t *pcm, int16_t *pcm_out, float *mid, int32_t *eplanes, const int32_t *dplanes, int *mid_grid_partials,
                          int *mixed_strides) {
    for (unsigned wg = 0; wg < wg_stream; wg++) {
        const lc3_group &g = G.g[find_group(G, wg)];
        const MlGroup &mgp = cfg_of_row(x, g);
        McJob protos[LC3_WG_WAVES];
        if (j.EL) memset(j.EL, 0xFF, LC3_WG_WAVES * sizeof(lc3_enc_lds));
        if (j.DL) memset(j.DL, 0xFF, LC3_WG_WAVES * sizeof(lc3_dec_lds));
        int shadows = 0, seen = 0;
        for (int w = 0; w < LC3_WG_WAVES; w++) {
            const int s_raw = (int)(wg - (unsigned)g.wg_stream) * LC3_WG_WAVES + w;
            const int valid = s_raw < g.n_streams;
            const int s = valid ? s_raw : g.n_streams - 1;
            const int pos = g.first_stream + s;
            const int entry = lc3_list_entry(entries, pos);
            shadows += !valid;
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
            q.pcm_s = pcm ? pcm + (size_t)tab[pos].pcm_off1 : nullptr;  // the channel's first sample
            q.pcm_out_s = pcm_out ? pcm_out + (size_t)tab[pos].pcm_off1 : nullptr;
            q.mid = mid ? mid + (size_t)g.frame_base * (size_t)MP_WORDS : nullptr;
            q.eplanes = eplanes ? eplanes + (size_t)g.frame_base * (size_t)EP_WORDS : nullptr;
            q.dplanes = dplanes ? dplanes + (size_t)g.frame_base * (size_t)LC3_PLANE_WORDS : nullptr;
            protos[w].stride = lc3_list_entry(&tab[pos].pad, 0);
            if (valid) seen |= 1 << protos[w].stride;
        }
        if (shadows && wg + 1 < wg_stream && mid_grid_partials) *mid_grid_partials += 1;
        if (mixed_strides && (seen & (seen - 1))) *mixed_strides += 1;
        run_wg_mc(protos);
    }
}

struct McPlan {
    std::vector<int32_t> entries;
    std::vector<lc3_stream_io> tab;
    ItPlan it;  // (P only: it_info reads it)
    int n_list = 0;
};
void mc_plan(const MlCtx &x, const int32_t *items, int n, const uint8_t *fresh, McPlan &p) {
    std::vector<uint8_t> fr((size_t)x.N, 0);
    for (int c = 0; c < x.N; c++) fr[(size_t)x.ms[(size_t)c].internal] = fresh[c];
    p.n_list = (int)lc3_mcitems_channels((const lc3_mcitem *)items, n);
    p.entries.assign((size_t)p.n_list, 0);
    p.tab.assign((size_t)p.n_list, lc3_stream_io());
    lc3_mcitems_build(x.mg.data(), x.ms.data(), fr.data(), (const lc3_mcitem *)items, n, p.entries.data(), p.tab.data(), p.it.P);
}
}  // namespace

extern "C" {
// The plan alone (host only).  items int32[n][4] = lc3gpu_mc_item.  rows int32[n_buckets][8] as lc3emu_it_plan; tab_of int64[channels][5],
// one row per (item, channel) in list order: launch position, pcm_off1, byte_off1, flag_idx, pad.  Returns the number of buckets
int lc3emu_mc_plan(void *h, const int32_t *items, int n, int32_t *rows, int max_buckets, int64_t *tab_of) {
    MlCtx &x = *(MlCtx *)h;
    std::vector<uint8_t> fresh((size_t)x.N, 0);
    McPlan p;
    mc_plan(x, items, n, fresh.data(), p);
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
    int k = 0;
    for (int i = 0; i < n; i++)
        for (int c = 0; c < items[4 * i + 1]; c++, k++) {
            const int internal = x.ms[(size_t)(items[4 * i] + c)].internal;
            for (int pos = 0; pos < p.n_list; pos++)
                if (lc3_list_channel(p.entries[(size_t)pos]) == internal) {
                    const lc3_stream_io &t = p.tab[(size_t)pos];
                    const int64_t row[5] = {pos, t.pcm_off1, t.byte_off1, t.flag_idx, t.pad};
                    memcpy(tab_of + 5 * k, row, sizeof row);
                }
        }
    return nb;
}

// items int32[n][4]; pcm int16[T][nf][C] per item, compact in list order -> bytes uint8[T][C][nbytes] per item.  info as lc3emu_it_encode,
// [7] workgroups of the front half whose valid waves ran at more than one stride
int lc3emu_mc_encode(void *h, const int32_t *items, int n, const uint8_t *fresh, const int16_t *pcm, uint8_t *bytes, int32_t *info) {
    MlCtx &x = *(MlCtx *)h;
    McPlan p;
    mc_plan(x, items, n, fresh, p);
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
    int partials = 0, mixed = 0;
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
            if (stage == 0) {  // lc3_enc_front_mc_items_kernel
                j.kind = 1;
                wgs += wg_stream;
                run_stream_kernel_mc(x, G, wg_stream, p.entries.data(), p.tab.data(), j, pcm, nullptr, mid, planes.data(), nullptr, &partials, &mixed);
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
            } else if (stage == 2) {  // lc3_enc_back_items_kernel
                j.kind = 2;
                run_stream_kernel_mc(x, G, wg_stream, p.entries.data(), p.tab.data(), j, nullptr, nullptr, mid, planes.data(), nullptr, nullptr, nullptr);
            } else {  // lc3_pack_mc_items_kernel
                for (int gi = 0; gi < G.n; gi++) {
                    const lc3_group &g = G.g[gi];
                    const size_t T = (size_t)g.n_frames;
                    for (size_t fl = 0; fl < (size_t)g.n_streams * T; fl++) {
                        const size_t f = (size_t)g.frame_base + fl, s = fl / T, t = fl % T;
                        const lc3_stream_io &io = p.tab[(size_t)g.first_stream + s];
                        lc3_pack_ctx c;
                        uint8_t sink = 0;
                        c.buf = bytes + (size_t)io.byte_off1 + t * (size_t)io.pad * (size_t)g.nbytes;
                        memset(c.buf, 0, (size_t)g.nbytes);
                        c.sink = &sink;
                        c.tns = tns_models;
                        c.nbytes = g.nbytes;
                        c.lookup = LC3T_AC_SPEC_LOOKUP;
                        c.cf = cf.data();
                        c.plane = LC3_PLANE_COL(planes.data(), f, EP_WORDS);
                        c.stride = LC3_PLANE_STRIDE;
                        lc3_pack_frame(c, g.ne);
                    }
                }
            }
        }
    free(L);
    int changed = 0;
    for (size_t i = frames * EP_WORDS; i < planes.size(); i++) changed += planes[i] != (int32_t)PATTERN;
    for (size_t i = frames * MP_WORDS; i < midw.size(); i++) changed += midw[i] != PATTERN;
    it_info(p.it, changed, partials, wgs, info);
    info[7] = mixed;
    return 0;
}

// bytes uint8[T][C][nbytes] per item, bad uint8[T][C] per item or NULL -> pcm int16[T][nf][C] per item; late as lc3emu_ml_decode
int lc3emu_mc_decode(void *h, const int32_t *items, int n, const uint8_t *fresh, const uint8_t *bytes, const uint8_t *bad, int16_t *pcm, int late,
                     int32_t *info) {
    MlCtx &x = *(MlCtx *)h;
    McPlan p;
    mc_plan(x, items, n, fresh, p);
    const lc3_mitems_plan &P = p.it.P;
    const size_t frames = (size_t)P.frames, cols = frames + SPARE;
    std::vector<int32_t> planes(cols * LC3_PLANE_WORDS, (int32_t)PATTERN);
    alignas(16) static uint32_t cf[64 * LC3_DCF_ROW_WORDS];
    for (int i = 0; i < 64 * LC3_DCF_ROW_WORDS; i++) cf[i] = lc3_dcf_word(i);
    std::vector<uint32_t> tns(LC3_TNS_MODEL_WORDS);
    for (int i = 0; i < LC3_TNS_MODEL_WORDS; i++) tns[(size_t)i] = lc3_tns_model_word(i);
    lc3_dec_lds *L = (lc3_dec_lds *)aligned_alloc(16, LC3_WG_WAVES * sizeof(lc3_dec_lds));
    int partials = 0, mixed = 0;
    unsigned wgs = 0;
    for (int stage = 0; stage < 2; stage++)
        for (int k = 0; k < lc3_mitems_sets(P); k++) {
            int b0, b1;
            lc3_mitems_set(P, k, b0, b1);
            lc3_groups G;
            unsigned wg_stream, wg_frame;
            lc3_mitems_rows(x.mg.data(), P, b0, b1, LC3_WG_WAVES, 64u, G, wg_stream, wg_frame);
            if (stage == 0) {  // lc3_parse_mc_items_kernel
                for (int gi = 0; gi < G.n; gi++) {
                    const lc3_group &g = G.g[gi];
                    const lc3_cfg &c = cfg_of_row(x, g).cfg;
                    const size_t T = (size_t)g.n_frames;
                    for (size_t fl = 0; fl < (size_t)g.n_streams * T; fl++) {
                        const size_t f = (size_t)g.frame_base + fl, s = fl / T, t = fl % T;
                        const lc3_stream_io &io = p.tab[(size_t)g.first_stream + s];
                        lc3_parse_ctx q;
                        q.dbg = nullptr;
                        q.tns = tns.data();
                        q.bytes = bytes + (size_t)io.byte_off1 + t * (size_t)io.pad * (size_t)g.nbytes;
                        q.len = g.nbytes;
                        q.lookup = LC3T_AC_SPEC_LOOKUP;
                        q.cf = cf;
                        q.plane = LC3_PLANE_COL(planes.data(), f, LC3_PLANE_WORDS);
                        q.stride = LC3_PLANE_STRIDE;
                        q.head = 0;
                        q.tail = 0;
                        const int rc = (bad && bad[(size_t)io.flag_idx + t * (size_t)io.pad]) ? -100 : lc3_parse_frame<1>(q, c.ne, c.fs_ind, c.n_ms_10);
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
            } else {  // lc3_decode_mc_items_kernel / lc3_decode_mc_items_late_kernel
                MlJob j;
                memset(&j, 0, sizeof(j));
                j.DL = L;
                j.late = late ? 1 : 0;
                j.kind = 3;
                wgs += wg_stream;
                run_stream_kernel_mc(x, G, wg_stream, p.entries.data(), p.tab.data(), j, nullptr, pcm, nullptr, nullptr, planes.data(), &partials, &mixed);
            }
        }
    free(L);
    int changed = 0;
    for (size_t i = frames * LC3_PLANE_WORDS; i < planes.size(); i++) changed += planes[i] != (int32_t)PATTERN;
    it_info(p.it, changed, partials, wgs, info);
    info[7] = mixed;
    return 0;
}
}
