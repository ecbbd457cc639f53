// TEST INFRASTRUCTURE -- the CPU wave emulator for the items calls on mixed-configuration handles (lc3gpu_encode_mixed_items /
// lc3gpu_decode_mixed_items): a frame count and a frame size per listed stream.  lc3_emu_mixed_list.cpp is included unchanged (the
// emulated handle, the workgroup runner); the per-call plan is lc3_mitems_build / lc3_mitems_rows of lc3_host_mixed_list.h, the header
// the library's host side builds it with, and a call with more buckets than LC3_MAX_GROUPS runs as the library runs it: one launch set
// after the other.  The stream bodies of lc3_dev_list.h run as lc3_enc_front_items_kernel, lc3_enc_back_items_kernel and
// lc3_decode_items(_late)_kernel call them: the frame count comes from the group ROW, the PCM from the table's ABSOLUTE offset, a shadow
// wave repeats the last stream of its own row.  The lane-per-frame stages are loops over each row's columns with frame -> (stream, t) by
// the row's count and the table's offsets taken with a factor of one.  A workgroup barrier under a per-stream branch on the frame count
// deadlocks here, which the test turns into a failure with a time limit.  Build: tests/test_emu_items.py.
#include "lc3_emu_mixed_list.cpp"

namespace {
const MlGroup &cfg_of_row(const MlCtx &x, const lc3_group &g) {  // (a row's size may be any: the configuration is found by its slot)
    for (size_t i = 0; i < x.mg.size(); i++)
        if (x.mg[i].slot == g.slot) return *x.groups[i];
    abort();
}

void run_stream_kernel_items(const MlCtx &x, const lc3_groups &G, unsigned wg_stream, const int32_t *entries, const lc3_stream_io *tab, MlJob j,
                             const int16_t *pcm, int16_t *pcm_out, float *mid, int32_t *eplanes, const int32_t *dplanes, int *mid_grid_partials) {
    for (unsigned wg = 0; wg < wg_stream; wg++) {
        const lc3_group &g = G.g[find_group(G, wg)];
        const MlGroup &mgp = cfg_of_row(x, g);
        MlJob protos[LC3_WG_WAVES];
        if (j.EL) memset(j.EL, 0xFF, LC3_WG_WAVES * sizeof(lc3_enc_lds));
        if (j.DL) memset(j.DL, 0xFF, LC3_WG_WAVES * sizeof(lc3_dec_lds));
        int shadows = 0;
        for (int w = 0; w < LC3_WG_WAVES; w++) {
            const int s_raw = (int)(wg - (unsigned)g.wg_stream) * LC3_WG_WAVES + w;
            const int valid = s_raw < g.n_streams;
            const int s = valid ? s_raw : g.n_streams - 1;
            const int pos = g.first_stream + s;
            const int entry = lc3_list_entry(entries, pos);
            shadows += !valid;
            MlJob &q = protos[w];
            q = j;
            q.cfg = &mgp.cfg;
            q.valid = valid;
            q.fresh = lc3_list_fresh(entry);
            q.nbytes = g.nbytes;
            q.T = g.n_frames;  // the row's
            q.fbase = (size_t)s * (size_t)g.n_frames;
            q.est = x.est + lc3_list_channel(entry);
            q.dst = x.dst + lc3_list_channel(entry);
            q.pcm_s = pcm ? pcm + (size_t)tab[pos].pcm_off1 : nullptr;  // absolute
            q.pcm_out_s = pcm_out ? pcm_out + (size_t)tab[pos].pcm_off1 : nullptr;
            q.mid = mid ? mid + (size_t)g.frame_base * (size_t)MP_WORDS : nullptr;
            q.eplanes = eplanes ? eplanes + (size_t)g.frame_base * (size_t)EP_WORDS : nullptr;
            q.dplanes = dplanes ? dplanes + (size_t)g.frame_base * (size_t)LC3_PLANE_WORDS : nullptr;
        }
        if (shadows && wg + 1 < wg_stream && mid_grid_partials) *mid_grid_partials += 1;
        run_wg_ml(protos);
    }
}

struct ItPlan {
    std::vector<int32_t> entries;
    std::vector<lc3_stream_io> tab;
    lc3_mitems_plan P;
};
void it_plan(const MlCtx &x, const int32_t *items, int n, const uint8_t *fresh, ItPlan &p) {
    std::vector<uint8_t> fr((size_t)x.N, 0);
    for (int c = 0; c < x.N; c++) fr[(size_t)x.ms[(size_t)c].internal] = fresh[c];
    p.entries.assign((size_t)n, 0);
    p.tab.assign((size_t)n, lc3_stream_io());
    lc3_mitems_build(x.mg.data(), x.ms.data(), fr.data(), (const lc3_mitem *)items, n, p.entries.data(), p.tab.data(), p.P);
}
void it_info(const ItPlan &p, int changed, int partials, unsigned wgs, int32_t *info) {
    info[0] = changed;
    info[1] = partials;
    info[2] = (int)wgs;
    info[3] = (int)p.P.buckets.size();
    info[4] = lc3_mitems_sets(p.P);
    info[5] = (int)p.P.frames;
    info[6] = p.P.max_frames;
}
}  // namespace

extern "C" {
// The plan alone (host only).  items int32[n][4] = lc3gpu_item.  out int32[n_buckets][8] = (set, row in set, slot, nbytes, n_frames, first,
// count, frame_base) as lc3_mitems_rows lays the rows out; pos_of int32[n]: the launch position of item i; tab int64[n][3] by ITEM:
// its pcm / byte / flag offsets.  Returns the number of buckets (<= max_buckets, else -1)
int lc3emu_it_plan(void *h, const int32_t *items, int n, int32_t *out, int max_buckets, int32_t *pos_of, int64_t *tab_of) {
    MlCtx &x = *(MlCtx *)h;
    std::vector<uint8_t> fresh((size_t)x.N, 0);
    ItPlan p;
    it_plan(x, items, n, fresh.data(), p);
    if ((int)p.P.buckets.size() > max_buckets) return -1;
    int nb = 0;
    for (int k = 0; k < lc3_mitems_sets(p.P); k++) {
        int b0, b1;
        lc3_mitems_set(p.P, k, b0, b1);
        lc3_groups G;
        unsigned ws, wf;
        lc3_mitems_rows(x.mg.data(), p.P, b0, b1, LC3_WG_WAVES, 64u, G, ws, wf);
        if (G.n > LC3_MAX_GROUPS || G.n != b1 - b0) return -2;
        for (int r = 0; r < G.n; r++, nb++) {
            const lc3_group &g = G.g[r];
            const int32_t row[8] = {k, r, g.slot, g.nbytes, g.n_frames, g.first_stream, g.n_streams, (int32_t)g.frame_base};
            memcpy(out + 8 * nb, row, sizeof row);
        }
    }
    for (int pos = 0; pos < n; pos++) {  // which item sits at launch position pos: the one whose channel the entry names
        const int internal = lc3_list_channel(p.entries[(size_t)pos]);
        for (int i = 0; i < n; i++)
            if (x.ms[(size_t)items[4 * i]].internal == internal) {
                pos_of[i] = pos;
                tab_of[3 * i] = p.tab[(size_t)pos].pcm_off1;
                tab_of[3 * i + 1] = p.tab[(size_t)pos].byte_off1;
                tab_of[3 * i + 2] = p.tab[(size_t)pos].flag_idx;
            }
    }
    return nb;
}

// items int32[n][4]; pcm ragged compact in list order -> bytes ragged compact in list order.  info int32[8]: [0] spare plane words that
// changed, [1] partial workgroups in the middle of a grid, [2] workgroups, [3] buckets, [4] launch sets, [5] frames, [6] largest count
int lc3emu_it_encode(void *h, const int32_t *items, int n, const uint8_t *fresh, const int16_t *pcm, uint8_t *bytes, int32_t *info) {
    MlCtx &x = *(MlCtx *)h;
    ItPlan p;
    it_plan(x, items, n, fresh, p);
    const size_t frames = (size_t)p.P.frames, cols = frames + SPARE;
    std::vector<int32_t> planes(cols * EP_WORDS, (int32_t)PATTERN);
    std::vector<uint32_t> midw(cols * MP_WORDS, PATTERN);
    float *mid = (float *)midw.data();
    lc3_enc_lds *L = (lc3_enc_lds *)aligned_alloc(16, LC3_WG_WAVES * sizeof(lc3_enc_lds));
    std::vector<uint32_t> cf(64 * 17);
    for (int q = 0; q < 64; q++)
        for (int r = 0; r < 17; r++) cf[(size_t)q * 17 + r] = (uint32_t)(int)LC3T_AC_SPEC_CUMFREQ[q][r] | ((uint32_t)(int)LC3T_AC_SPEC_FREQ[q][r] << 16);
    static uint32_t tns_models[LC3_TNS_MODEL_WORDS];
    for (int i = 0; i < LC3_TNS_MODEL_WORDS; i++) tns_models[i] = lc3_tns_model_word(i);
    int partials = 0;
    unsigned wgs = 0;
    // stage by stage over the launch sets, as the library queues them
    for (int stage = 0; stage < 4; stage++)
        for (int k = 0; k < lc3_mitems_sets(p.P); k++) {
            int b0, b1;
            lc3_mitems_set(p.P, k, b0, b1);
            lc3_groups G;
            unsigned wg_stream, wg_frame;
            lc3_mitems_rows(x.mg.data(), p.P, b0, b1, LC3_WG_WAVES, 64u, G, wg_stream, wg_frame);
            MlJob j;
            memset(&j, 0, sizeof(j));
            j.EL = L;
            if (stage == 0) {
                j.kind = 1;
                wgs += wg_stream;
                run_stream_kernel_items(x, G, wg_stream, p.entries.data(), p.tab.data(), j, pcm, nullptr, mid, planes.data(), nullptr, &partials);
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
            } else if (stage == 2) {
                j.kind = 2;
                run_stream_kernel_items(x, G, wg_stream, p.entries.data(), p.tab.data(), j, nullptr, nullptr, mid, planes.data(), nullptr, nullptr);
            } else {  // lc3_pack_items_kernel
                for (int gi = 0; gi < G.n; gi++) {
                    const lc3_group &g = G.g[gi];
                    const size_t T = (size_t)g.n_frames;
                    for (size_t fl = 0; fl < (size_t)g.n_streams * T; fl++) {
                        const size_t f = (size_t)g.frame_base + fl, s = fl / T, t = fl % T;
                        lc3_pack_ctx c;
                        uint8_t sink = 0;
                        c.buf = bytes + (size_t)p.tab[(size_t)g.first_stream + s].byte_off1 + t * (size_t)g.nbytes;
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
    it_info(p, changed, partials, wgs, info);
    return 0;
}

// bytes ragged compact in list order, bad one flag per frame in item order or NULL -> pcm ragged compact in list order; late as
// lc3emu_ml_decode.  info as lc3emu_it_encode
int lc3emu_it_decode(void *h, const int32_t *items, int n, const uint8_t *fresh, const uint8_t *bytes, const uint8_t *bad, int16_t *pcm, int late,
                     int32_t *info) {
    MlCtx &x = *(MlCtx *)h;
    ItPlan p;
    it_plan(x, items, n, fresh, p);
    const size_t frames = (size_t)p.P.frames, cols = frames + SPARE;
    std::vector<int32_t> planes(cols * LC3_PLANE_WORDS, (int32_t)PATTERN);
    alignas(16) static uint32_t cf[64 * LC3_DCF_ROW_WORDS];
    for (int i = 0; i < 64 * LC3_DCF_ROW_WORDS; i++) cf[i] = lc3_dcf_word(i);
    std::vector<uint32_t> tns(LC3_TNS_MODEL_WORDS);
    for (int i = 0; i < LC3_TNS_MODEL_WORDS; i++) tns[(size_t)i] = lc3_tns_model_word(i);
    lc3_dec_lds *L = (lc3_dec_lds *)aligned_alloc(16, LC3_WG_WAVES * sizeof(lc3_dec_lds));
    int partials = 0;
    unsigned wgs = 0;
    for (int stage = 0; stage < 2; stage++)
        for (int k = 0; k < lc3_mitems_sets(p.P); k++) {
            int b0, b1;
            lc3_mitems_set(p.P, k, b0, b1);
            lc3_groups G;
            unsigned wg_stream, wg_frame;
            lc3_mitems_rows(x.mg.data(), p.P, b0, b1, LC3_WG_WAVES, 64u, G, wg_stream, wg_frame);
            if (stage == 0) {  // lc3_parse_items_kernel
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
                        q.bytes = bytes + (size_t)io.byte_off1 + t * (size_t)g.nbytes;
                        q.len = g.nbytes;
                        q.lookup = LC3T_AC_SPEC_LOOKUP;
                        q.cf = cf;
                        q.plane = LC3_PLANE_COL(planes.data(), f, LC3_PLANE_WORDS);
                        q.stride = LC3_PLANE_STRIDE;
                        q.head = 0;
                        q.tail = 0;
                        const int rc = (bad && bad[(size_t)io.flag_idx + t]) ? -100 : lc3_parse_frame<1>(q, c.ne, c.fs_ind, c.n_ms_10);
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
            } else {
                MlJob j;
                memset(&j, 0, sizeof(j));
                j.DL = L;
                j.late = late ? 1 : 0;
                j.kind = 3;
                wgs += wg_stream;
                run_stream_kernel_items(x, G, wg_stream, p.entries.data(), p.tab.data(), j, nullptr, pcm, nullptr, nullptr, planes.data(), &partials);
            }
        }
    free(L);
    int changed = 0;
    for (size_t i = frames * LC3_PLANE_WORDS; i < planes.size(); i++) changed += planes[i] != (int32_t)PATTERN;
    it_info(p, changed, partials, wgs, info);
    return 0;
}
}
