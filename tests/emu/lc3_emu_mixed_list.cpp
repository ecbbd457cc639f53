// TEST INFRASTRUCTURE -- the CPU wave emulator (lc3_emu.cpp, included unchanged) for the list calls on mixed-configuration handles
// (lc3gpu_encode_mixed_list / lc3gpu_decode_mixed_list).  The per-call plan is built by lc3_host_mixed_list.h, the header the library's
// host side builds it with; lc3_dev_list.h is included as it is and its three stream bodies run under four emulated waves per workgroup
// exactly as lc3_enc_front_mixed_list_kernel, lc3_enc_back_mixed_list_kernel and lc3_decode_mixed_list(_late)_kernel (lc3gpu.hip) call
// them: a workgroup finds its group from its index (the loop of lc3_find_group), wave w takes launch position first_stream + s of that
// group, its state through the entry, its PCM through the per-call table; a shadow wave (valid = 0) repeats the group's last listed stream.
// The lane-per-frame stages (vector quantiser, packer, parser) are plain loops over each group's compact plane columns, addressing the
// caller's buffers through tab[first_stream + s] as the mixed kernels do.
// A barrier, or a branch around one, on a per-stream condition deadlocks here (the pthread barrier waits for all four waves), which the
// test turns into a failure with a time limit.  LDS starts every workgroup as 0xFF bytes.  The planes are allocated with spare columns
// and pre-filled with a pattern: a column outside the listed frames that changes is counted.  Build: tests/test_emu_mixed_list.py.
#include "lc3_emu.cpp"

#include <algorithm>

#include "../../lc3-codec_amd/csrc/lc3_dev_list.h"
#include "../../lc3-codec_amd/csrc/lc3_host_mixed_list.h"

namespace {
struct MlGroup {
    lc3_cfg cfg;
    lc3_host_plan pl;
    std::vector<float> poly, lw;
    std::vector<uint8_t> lb;
};
struct MlCtx {
    int N = 0;
    std::vector<MlGroup *> groups;  // by the handle's group index
    std::vector<lc3_mlist_group> mg;
    std::vector<lc3_mlist_stream> ms;  // per caller stream
    lc3_enc_state *est = nullptr;      // [N], INTERNAL order, persistent over the calls
    lc3_dec_state *dst = nullptr;
};
struct MlJob {
    const lc3_cfg *cfg;
    int lane, wave, valid, kind;  // 1 front half, 2 back half, 3 synthesis
    int fresh, T, late, nbytes;
    size_t fbase;
    lc3_enc_state *est;
    lc3_dec_state *dst;
    lc3_enc_lds *EL;
    lc3_dec_lds *DL;
    const int16_t *pcm_s;
    float *mid;
    int32_t *eplanes;
    const int32_t *dplanes;
    int16_t *pcm_out_s;
};

void *ml_lane_main(void *arg) {
    MlJob *j = (MlJob *)arg;
    tl_wave = j->wave;
    if (j->kind == 1)
        lc3_list_front_stream(*j->cfg, j->EL[j->wave], j->lane, j->est, j->fresh, j->valid, j->pcm_s, j->mid, j->eplanes, j->fbase, j->nbytes, j->T, 0, 1);
    else if (j->kind == 2)
        lc3_list_back_stream(*j->cfg, j->EL[j->wave], j->lane, j->est, j->valid, j->mid, j->eplanes, j->fbase, j->nbytes, j->T, 0);
    else
        lc3_list_synth_stream(*j->cfg, j->DL[j->wave], j->lane, j->dst, j->fresh, j->valid, j->nbytes, j->dplanes, j->fbase, j->T, j->pcm_out_s, j->late);
    return 0;
}

void run_wg_ml(const MlJob *protos) {
    static pthread_t th[LC3_WG_WAVES * LC3_WAVE];
    static MlJob jobs[LC3_WG_WAVES * LC3_WAVE];
    for (int w = 0; w < LC3_WG_WAVES; w++) pthread_barrier_init(&g_wave_bar[w], 0, LC3_WAVE);
    pthread_barrier_init(&g_wg_bar, 0, LC3_WG_WAVES * LC3_WAVE);
    for (int w = 0; w < LC3_WG_WAVES; w++)
        for (int i = 0; i < LC3_WAVE; i++) {
            MlJob &q = jobs[w * LC3_WAVE + i];
            q = protos[w];
            q.lane = i;
            q.wave = w;
            pthread_create(&th[w * LC3_WAVE + i], 0, ml_lane_main, &q);
        }
    for (int i = 0; i < LC3_WG_WAVES * LC3_WAVE; i++) pthread_join(th[i], 0);
    for (int w = 0; w < LC3_WG_WAVES; w++) pthread_barrier_destroy(&g_wave_bar[w]);
    pthread_barrier_destroy(&g_wg_bar);
}

// lc3_find_group (lc3gpu.hip), stream kernels
int find_group(const lc3_groups &G, unsigned wg) {
    int gi = 0;
    while (gi + 1 < G.n && wg >= (unsigned)G.g[gi + 1].wg_stream) gi++;
    return gi;
}

const MlGroup &group_of_row(const MlCtx &x, const lc3_group &g) {  // the handle's group a row of the per-call table stands for
    for (size_t i = 0; i < x.mg.size(); i++)
        if (x.mg[i].slot == g.slot && x.mg[i].nbytes == g.nbytes) return *x.groups[i];
    abort();
}

// every workgroup of a wave-per-stream kernel of the tick; info[1] counts the partial workgroups that are not the grid's last
void run_stream_kernel(const MlCtx &x, const lc3_groups &G, unsigned wg_stream, const int32_t *entries, const lc3_stream_io *tab, MlJob j,
                       const int16_t *pcm, int16_t *pcm_out, float *mid, int32_t *eplanes, const int32_t *dplanes, int *mid_grid_partials) {
    for (unsigned wg = 0; wg < wg_stream; wg++) {
        const lc3_group &g = G.g[find_group(G, wg)];
        const MlGroup &mgp = group_of_row(x, g);
        MlJob protos[LC3_WG_WAVES];
        if (j.EL) memset(j.EL, 0xFF, LC3_WG_WAVES * sizeof(lc3_enc_lds));  // LDS is not zeroed on the GPU
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
            q.fbase = (size_t)s * (size_t)j.T;
            q.est = x.est + lc3_list_channel(entry);
            q.dst = x.dst + lc3_list_channel(entry);
            q.pcm_s = pcm ? pcm + (size_t)j.T * (size_t)tab[pos].pcm_off1 : nullptr;
            q.pcm_out_s = pcm_out ? pcm_out + (size_t)j.T * (size_t)tab[pos].pcm_off1 : nullptr;
            q.mid = mid ? mid + (size_t)g.frame_base * (size_t)MP_WORDS : nullptr;
            q.eplanes = eplanes ? eplanes + (size_t)g.frame_base * (size_t)EP_WORDS : nullptr;
            q.dplanes = dplanes ? dplanes + (size_t)g.frame_base * (size_t)LC3_PLANE_WORDS : nullptr;
        }
        if (shadows && wg + 1 < wg_stream && mid_grid_partials) *mid_grid_partials += 1;
        run_wg_ml(protos);
    }
}

const uint32_t PATTERN = 0x5A5AC3C3u;
const size_t SPARE = 8;  // columns beyond the tick's frames
}  // namespace

extern "C" {
// descs int32[n][3] = (fs_hz, frame_us, nbytes) in the caller's order; the handle sorts them as build_mixed (lc3gpu.hip) does: stable, by
// (configuration slot, frame bytes)
void *lc3emu_ml_new(int n, const int32_t *descs) {
    static const int fs_tab[6] = {8000, 16000, 24000, 32000, 44100, 48000};
    MlCtx *x = new MlCtx();
    x->N = n;
    struct Key { int slot, nbytes, idx; };
    std::vector<Key> keys;
    for (int i = 0; i < n; i++) {
        int k = -1;
        for (int q = 0; q < 6; q++)
            if (fs_tab[q] == descs[3 * i]) k = q;
        if (k < 0) return nullptr;
        keys.push_back({2 * k + (descs[3 * i + 1] == 10000), descs[3 * i + 2], i});
    }
    std::stable_sort(keys.begin(), keys.end(), [](const Key &a, const Key &b) { return a.slot != b.slot ? a.slot < b.slot : a.nbytes < b.nbytes; });
    x->ms.resize((size_t)n);
    for (int jn = 0; jn < n; jn++) {
        const Key &k = keys[(size_t)jn];
        if (x->mg.empty() || x->mg.back().slot != k.slot || x->mg.back().nbytes != k.nbytes) {
            MlGroup *g = new MlGroup();
            if (lc3_make_config(g->cfg, descs[3 * k.idx + 1], descs[3 * k.idx]) || lc3_make_plan(g->cfg, g->pl)) return nullptr;
            lc3_cfg &c = g->cfg;
            c.fft_tw = g->pl.fft_tw.data();
            c.dct_tw = g->pl.dct_tw.data();
            c.perm = g->pl.perm.data();
            g->poly.resize((size_t)c.p_up * (size_t)c.resamp_stride);
            for (size_t i = 0; i < g->poly.size(); i++) g->poly[i] = lc3_resamp_poly_value(c.p_up, c.resamp_lim, c.resamp_stride, (int)i);
            c.resamp_poly = g->poly.data();
            g->lw.resize((size_t)c.ne);
            for (int q = 0; q < c.ne; q++) g->lw[(size_t)q] = lc3_line_width_value(c, q);
            c.line_width = g->lw.data();
            g->lb.resize((size_t)c.nf + 16);
            for (int q = 0; q < c.nf; q++) g->lb[(size_t)q] = (uint8_t)lc3_line_band_value(c, q);
            c.line_band = g->lb.data();
            x->groups.push_back(g);
            x->mg.push_back({k.slot, 0, k.nbytes, c.ne, c.nb, c.nf});  // (the view is the device's business: the emulator runs the run-time view)
        }
        x->ms[(size_t)k.idx] = {(int)x->mg.size() - 1, jn};
    }
    if (x->mg.size() > LC3_MAX_GROUPS) return nullptr;
    x->est = (lc3_enc_state *)aligned_alloc(16, (size_t)n * sizeof(lc3_enc_state));
    x->dst = (lc3_dec_state *)aligned_alloc(16, (size_t)n * sizeof(lc3_dec_state));
    memset(x->est, 0xEE, (size_t)n * sizeof(lc3_enc_state));  // (hipMalloc hands out anything: a fresh launch must not depend on it)
    memset(x->dst, 0, (size_t)n * sizeof(lc3_dec_state));     // (decoder_alloc zeroes the blobs once)
    return x;
}
void lc3emu_ml_free(void *h) {
    MlCtx *x = (MlCtx *)h;
    for (MlGroup *g : x->groups) delete g;
    free(x->est);
    free(x->dst);
    delete x;
}
int lc3emu_ml_n_groups(void *h) { return (int)((MlCtx *)h)->mg.size(); }
int lc3emu_ml_group_of(void *h, int channel) { return ((MlCtx *)h)->ms[(size_t)channel].group; }
int lc3emu_ml_state_size(int decoder) { return decoder ? (int)sizeof(lc3_dec_state) : (int)sizeof(lc3_enc_state); }
void lc3emu_ml_state(void *h, int decoder, int channel, void *out) {  // channel: the caller's index
    MlCtx *x = (MlCtx *)h;
    const int in = x->ms[(size_t)channel].internal;
    if (decoder) memcpy(out, x->dst + in, sizeof(lc3_dec_state));
    else memcpy(out, x->est + in, sizeof(lc3_enc_state));
}

// the plan of a tick, as the library builds it.  fresh: uint8 per CALLER channel (the library keeps its record in internal order)
static void ml_plan(const MlCtx &x, const int32_t *channels, int n, const uint8_t *fresh, std::vector<int32_t> &entries, std::vector<lc3_stream_io> &tab,
                    lc3_mlist_plan &P) {
    std::vector<uint8_t> fr((size_t)x.N, 0);
    for (int c = 0; c < x.N; c++) fr[(size_t)x.ms[(size_t)c].internal] = fresh[c];
    entries.assign((size_t)n, 0);
    tab.assign((size_t)n, lc3_stream_io());
    lc3_mlist_build(x.mg.data(), (int)x.mg.size(), x.ms.data(), fr.data(), channels, n, entries.data(), tab.data(), P);
}

// channels int32[n] (caller indices), pcm ragged compact in list order -> bytes ragged compact in list order.
// info int32[4]: [0] spare plane words that changed, [1] partial workgroups in the middle of the grid, [2] workgroups, [3] groups launched
int lc3emu_ml_encode(void *h, const int32_t *channels, int n, const uint8_t *fresh, int T, const int16_t *pcm, uint8_t *bytes, int32_t *info) {
    MlCtx &x = *(MlCtx *)h;
    std::vector<int32_t> entries;
    std::vector<lc3_stream_io> tab;
    lc3_mlist_plan P;
    ml_plan(x, channels, n, fresh, entries, tab, P);
    lc3_groups G;
    unsigned wg_stream, wg_frame;
    lc3_mlist_groups(x.mg.data(), (int)x.mg.size(), P, T, LC3_WG_WAVES, 64u, G, wg_stream, wg_frame);
    const size_t frames = (size_t)n * (size_t)T, cols = frames + SPARE;
    std::vector<int32_t> planes(cols * EP_WORDS, (int32_t)PATTERN);
    std::vector<uint32_t> midw(cols * MP_WORDS, PATTERN);
    float *mid = (float *)midw.data();
    lc3_enc_lds *L = (lc3_enc_lds *)aligned_alloc(16, LC3_WG_WAVES * sizeof(lc3_enc_lds));
    MlJob j;
    memset(&j, 0, sizeof(j));
    j.T = T;
    j.EL = L;
    j.kind = 1;
    int partials = 0;
    run_stream_kernel(x, G, wg_stream, entries.data(), tab.data(), j, pcm, nullptr, mid, planes.data(), nullptr, &partials);
    for (int gi = 0; gi < G.n; gi++) {  // lc3_sns_vq_mixed_kernel, unchanged on the compact planes
        const lc3_group &g = G.g[gi];
        for (size_t fl = 0; fl < (size_t)g.n_streams * (size_t)T; fl++) {
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
    j.kind = 2;
    run_stream_kernel(x, G, wg_stream, entries.data(), tab.data(), j, nullptr, nullptr, mid, planes.data(), nullptr, nullptr);
    free(L);
    std::vector<uint32_t> cf(64 * 17);
    for (int p = 0; p < 64; p++)
        for (int q = 0; q < 17; q++)
            cf[(size_t)p * 17 + q] = (uint32_t)(int)LC3T_AC_SPEC_CUMFREQ[p][q] | ((uint32_t)(int)LC3T_AC_SPEC_FREQ[p][q] << 16);
    static uint32_t tns_models[LC3_TNS_MODEL_WORDS];
    for (int i = 0; i < LC3_TNS_MODEL_WORDS; i++) tns_models[i] = lc3_tns_model_word(i);
    for (int gi = 0; gi < G.n; gi++) {  // lc3_pack_mixed_kernel
        const lc3_group &g = G.g[gi];
        for (size_t fl = 0; fl < (size_t)g.n_streams * (size_t)T; fl++) {
            const size_t f = (size_t)g.frame_base + fl, s = fl / (size_t)T, t = fl % (size_t)T;
            lc3_pack_ctx p;
            uint8_t sink = 0;
            p.buf = bytes + (size_t)T * (size_t)tab[(size_t)g.first_stream + s].byte_off1 + t * (size_t)g.nbytes;
            memset(p.buf, 0, (size_t)g.nbytes);
            p.sink = &sink;
            p.tns = tns_models;
            p.nbytes = g.nbytes;
            p.lookup = LC3T_AC_SPEC_LOOKUP;
            p.cf = cf.data();
            p.plane = LC3_PLANE_COL(planes.data(), f, EP_WORDS);
            p.stride = LC3_PLANE_STRIDE;
            lc3_pack_frame(p, g.ne);
        }
    }
    int changed = 0;
    for (size_t i = frames * EP_WORDS; i < planes.size(); i++) changed += planes[i] != (int32_t)PATTERN;
    for (size_t i = frames * MP_WORDS; i < midw.size(); i++) changed += midw[i] != PATTERN;
    info[0] = changed;
    info[1] = partials;
    info[2] = (int)wg_stream;
    info[3] = G.n;
    return 0;
}

// bytes ragged compact in list order, bad uint8[n][T] in list order or NULL -> pcm ragged compact in list order; late = 0: the
// reconstruction in the parser (full batches), 1: in the synthesis body (small launches).  info as lc3emu_ml_encode
int lc3emu_ml_decode(void *h, const int32_t *channels, int n, const uint8_t *fresh, int T, const uint8_t *bytes, const uint8_t *bad, int16_t *pcm,
                     int late, int32_t *info) {
    MlCtx &x = *(MlCtx *)h;
    std::vector<int32_t> entries;
    std::vector<lc3_stream_io> tab;
    lc3_mlist_plan P;
    ml_plan(x, channels, n, fresh, entries, tab, P);
    lc3_groups G;
    unsigned wg_stream, wg_frame;
    lc3_mlist_groups(x.mg.data(), (int)x.mg.size(), P, T, LC3_WG_WAVES, 64u, G, wg_stream, wg_frame);
    const size_t frames = (size_t)n * (size_t)T, cols = frames + SPARE;
    std::vector<int32_t> planes(cols * LC3_PLANE_WORDS, (int32_t)PATTERN);
    alignas(16) static uint32_t cf[64 * LC3_DCF_ROW_WORDS];
    for (int i = 0; i < 64 * LC3_DCF_ROW_WORDS; i++) cf[i] = lc3_dcf_word(i);
    std::vector<uint32_t> tns(LC3_TNS_MODEL_WORDS);
    for (int i = 0; i < LC3_TNS_MODEL_WORDS; i++) tns[(size_t)i] = lc3_tns_model_word(i);
    for (int gi = 0; gi < G.n; gi++) {  // lc3_parse_mixed_kernel, unchanged on the compact buffers
        const lc3_group &g = G.g[gi];
        const lc3_cfg &c = group_of_row(x, g).cfg;
        for (size_t fl = 0; fl < (size_t)g.n_streams * (size_t)T; fl++) {
            const size_t f = (size_t)g.frame_base + fl, s = fl / (size_t)T, t = fl % (size_t)T;
            const lc3_stream_io &io = tab[(size_t)g.first_stream + s];
            lc3_parse_ctx p;
            p.dbg = nullptr;
            p.tns = tns.data();
            p.bytes = bytes + (size_t)T * (size_t)io.byte_off1 + t * (size_t)g.nbytes;
            p.len = g.nbytes;
            p.lookup = LC3T_AC_SPEC_LOOKUP;
            p.cf = cf;
            p.plane = LC3_PLANE_COL(planes.data(), f, LC3_PLANE_WORDS);
            p.stride = LC3_PLANE_STRIDE;
            p.head = 0;
            p.tail = 0;
            const int rc = (bad && bad[(size_t)io.flag_idx * (size_t)T + t]) ? -100 : lc3_parse_frame<1>(p, c.ne, c.fs_ind, c.n_ms_10);
            int ok = rc == 0;
            if (ok && late) {
                ok = lc3_reconstruct_prepare_late(p);
            } else if (ok) {
                float scf[16];
                lc3_recon_ctx r;
                r.scf = scf;
                r.sstride = 1;
                r.mpvq = &LC3T_MPVQ_OFFSETS[0][0];
                r.ifs = lc3_band_index(c);
                ok = lc3_reconstruct_frame(p, r, c, nullptr);
            }
            lc3_px_set(p, AD_OK, ok);
        }
    }
    lc3_dec_lds *L = (lc3_dec_lds *)aligned_alloc(16, LC3_WG_WAVES * sizeof(lc3_dec_lds));
    MlJob j;
    memset(&j, 0, sizeof(j));
    j.T = T;
    j.DL = L;
    j.late = late ? 1 : 0;
    j.kind = 3;
    int partials = 0;
    run_stream_kernel(x, G, wg_stream, entries.data(), tab.data(), j, nullptr, pcm, nullptr, nullptr, planes.data(), &partials);
    free(L);
    int changed = 0;
    for (size_t i = frames * LC3_PLANE_WORDS; i < planes.size(); i++) changed += planes[i] != (int32_t)PATTERN;
    info[0] = changed;
    info[1] = partials;
    info[2] = (int)wg_stream;
    info[3] = G.n;
    return 0;
}
}
