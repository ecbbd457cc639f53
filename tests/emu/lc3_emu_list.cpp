// TEST INFRASTRUCTURE -- the CPU wave emulator (lc3_emu.cpp, included unchanged) for the list calls (lc3gpu_encode_list /
// lc3gpu_decode_list): lc3_dev_list.h is included as it is and its three stream bodies -- what lc3_enc_front_list_kernel,
// lc3_enc_back_list_kernel and lc3_decode_list_kernel (lc3gpu.hip) call after staging their tables -- run under four emulated waves per
// workgroup, over a persistent array of channel states, with the lane-per-frame stages (vector quantiser, packer, parser) as plain loops
// over the compact buffers.  A list entry is channel | LC3_LIST_FRESH, as the library's host side writes it.
// A barrier, or a branch around one, on a per-stream condition deadlocks here (the pthread barrier waits for all four waves), which the
// tests turn into a failure with a time limit.  LDS starts every workgroup as 0xFF bytes: a fresh stream that read what the previous
// owner of its wave -- or of its channel -- left would not match the oracle.  Build: tests/test_emu_list.py.
#include "lc3_emu.cpp"

#include "../../lc3-codec_amd/csrc/lc3_dev_list.h"

namespace {
struct ListCtx {
    lc3_cfg cfg;
    lc3_host_plan pl;
    std::vector<float> poly, lw;
    std::vector<uint8_t> lb;
    int N, nbytes;
    lc3_enc_state *est;  // [N], persistent over the calls
    lc3_dec_state *dst;
};
struct ListJob {
    const ListCtx *x;
    int lane, wave, valid, kind;  // 1 front half, 2 back half, 3 synthesis
    int s, T, late;
    const int32_t *list;
    lc3_enc_lds *EL;
    lc3_dec_lds *DL;
    const int16_t *pcm;
    float *mid;
    int32_t *eplanes;
    const int32_t *dplanes;
    int16_t *pcm_out;
};

void *list_lane_main(void *arg) {
    ListJob *j = (ListJob *)arg;
    const ListCtx &x = *j->x;
    const int lane = j->lane, nf = x.cfg.nf;
    tl_wave = j->wave;
    const int entry = lc3_list_entry(j->list, j->s);
    const int ch = lc3_list_channel(entry), fresh = lc3_list_fresh(entry);
    const size_t fbase = (size_t)j->s * (size_t)j->T;
    if (j->kind == 1)
        lc3_list_front_stream(x.cfg, j->EL[j->wave], lane, x.est + ch, fresh, j->valid, j->pcm + fbase * (size_t)nf, j->mid, j->eplanes, fbase, x.nbytes,
                              j->T, 0, 0);
    else if (j->kind == 2)
        lc3_list_back_stream(x.cfg, j->EL[j->wave], lane, x.est + ch, j->valid, j->mid, j->eplanes, fbase, x.nbytes, j->T, 0);
    else
        lc3_list_synth_stream(x.cfg, j->DL[j->wave], lane, x.dst + ch, fresh, j->valid, x.nbytes, j->dplanes, fbase, j->T,
                              j->pcm_out + fbase * (size_t)nf, j->late);
    return 0;
}

void run_wg_list(const ListJob *protos) {
    static pthread_t th[LC3_WG_WAVES * LC3_WAVE];
    static ListJob jobs[LC3_WG_WAVES * LC3_WAVE];
    for (int w = 0; w < LC3_WG_WAVES; w++) pthread_barrier_init(&g_wave_bar[w], 0, LC3_WAVE);
    pthread_barrier_init(&g_wg_bar, 0, LC3_WG_WAVES * LC3_WAVE);
    for (int w = 0; w < LC3_WG_WAVES; w++)
        for (int i = 0; i < LC3_WAVE; i++) {
            ListJob &q = jobs[w * LC3_WAVE + i];
            q = protos[w];
            q.lane = i;
            q.wave = w;
            pthread_create(&th[w * LC3_WAVE + i], 0, list_lane_main, &q);
        }
    for (int i = 0; i < LC3_WG_WAVES * LC3_WAVE; i++) pthread_join(th[i], 0);
    for (int w = 0; w < LC3_WG_WAVES; w++) pthread_barrier_destroy(&g_wave_bar[w]);
    pthread_barrier_destroy(&g_wg_bar);
}

// every workgroup of a wave-per-stream kernel over the n streams of the list
void run_stream_kernel(ListJob j, int n) {
    for (int s0 = 0; s0 < n; s0 += LC3_WG_WAVES) {
        ListJob protos[LC3_WG_WAVES];
        if (j.EL) memset(j.EL, 0xFF, LC3_WG_WAVES * sizeof(lc3_enc_lds));  // LDS is not zeroed on the GPU
        if (j.DL) memset(j.DL, 0xFF, LC3_WG_WAVES * sizeof(lc3_dec_lds));
        for (int w = 0; w < LC3_WG_WAVES; w++) {
            const int valid = s0 + w < n;
            protos[w] = j;
            protos[w].valid = valid;
            protos[w].s = valid ? s0 + w : n - 1;  // the waves past the end shadow the last stream and store nothing
        }
        run_wg_list(protos);
    }
}
}  // namespace

extern "C" {
// a handle of N channels: the states as the library allocates them (decoder blobs zeroed once; every channel is fresh until a caller's
// entry says otherwise -- the freshness record is the caller's, as it is the host side's in the library)
void *lc3emu_list_new(int fs_hz, int frame_us, int nbytes, int N) {
    ListCtx *x = new ListCtx();
    if (lc3_make_config(x->cfg, frame_us, fs_hz) || lc3_make_plan(x->cfg, x->pl)) {
        delete x;
        return nullptr;
    }
    lc3_cfg &c = x->cfg;
    c.fft_tw = x->pl.fft_tw.data();
    c.dct_tw = x->pl.dct_tw.data();
    c.perm = x->pl.perm.data();
    x->poly.resize((size_t)c.p_up * (size_t)c.resamp_stride);
    for (size_t i = 0; i < x->poly.size(); i++) x->poly[i] = lc3_resamp_poly_value(c.p_up, c.resamp_lim, c.resamp_stride, (int)i);
    c.resamp_poly = x->poly.data();
    x->lw.resize((size_t)c.ne);
    for (int k = 0; k < c.ne; k++) x->lw[(size_t)k] = lc3_line_width_value(c, k);
    c.line_width = x->lw.data();
    x->lb.resize((size_t)c.nf + 16);
    for (int k = 0; k < c.nf; k++) x->lb[(size_t)k] = (uint8_t)lc3_line_band_value(c, k);
    c.line_band = x->lb.data();
    x->N = N;
    x->nbytes = nbytes;
    x->est = (lc3_enc_state *)aligned_alloc(16, (size_t)N * sizeof(lc3_enc_state));
    x->dst = (lc3_dec_state *)aligned_alloc(16, (size_t)N * sizeof(lc3_dec_state));
    memset(x->est, 0xEE, (size_t)N * sizeof(lc3_enc_state));  // (hipMalloc hands out anything: a fresh launch must not depend on it)
    memset(x->dst, 0, (size_t)N * sizeof(lc3_dec_state));     // (decoder_alloc zeroes the blobs once)
    return x;
}
void lc3emu_list_free(void *h) {
    ListCtx *x = (ListCtx *)h;
    free(x->est);
    free(x->dst);
    delete x;
}
// the state blob of one channel, for "untouched means untouched"
int lc3emu_list_state_size(int decoder) { return decoder ? (int)sizeof(lc3_dec_state) : (int)sizeof(lc3_enc_state); }
void lc3emu_list_state(void *h, int decoder, int channel, void *out) {
    ListCtx *x = (ListCtx *)h;
    if (decoder) memcpy(out, x->dst + channel, sizeof(lc3_dec_state));
    else memcpy(out, x->est + channel, sizeof(lc3_enc_state));
}

// list int32[n] (channel | LC3_LIST_FRESH), pcm int16[n][T][nf] -> bytes uint8[n][T][nbytes]
int lc3emu_list_encode(void *h, const int32_t *list, int n, int T, const int16_t *pcm, uint8_t *bytes) {
    ListCtx *x = (ListCtx *)h;
    const lc3_cfg &c = x->cfg;
    const int nbytes = x->nbytes;
    const size_t frames = (size_t)n * (size_t)T;
    std::vector<int32_t> planes(((frames + 63) / 64) * 64 * EP_WORDS, 0);
    lc3_enc_lds *L = (lc3_enc_lds *)aligned_alloc(16, LC3_WG_WAVES * sizeof(lc3_enc_lds));
    float *mid = (float *)aligned_alloc(16, frames * (size_t)MP_WORDS * sizeof(float));
    memset(mid, 0, frames * (size_t)MP_WORDS * sizeof(float));
    ListJob j;
    memset(&j, 0, sizeof(j));
    j.x = x;
    j.T = T;
    j.list = list;
    j.EL = L;
    j.pcm = pcm;
    j.mid = mid;
    j.eplanes = planes.data();
    j.kind = 1;
    run_stream_kernel(j, n);
    for (size_t f = 0; f < frames; f++) {  // lc3_sns_vq_kernel, unchanged on the compact planes
        lc3_vq_ctx v;
        v.mid = mid + f * (size_t)MP_WORDS;
        v.gains = mid + f * (size_t)MP_WORDS + MP_G;
        v.plane = LC3_PLANE_COL(planes.data(), f, EP_WORDS);
        v.stride = LC3_PLANE_STRIDE;
        v.mpvq = &LC3T_MPVQ_OFFSETS[0][0];
        v.nb = c.nb;
        v.spec_flags = 0;
        lc3_sns_vq_frame(v);
    }
    j.kind = 2;
    run_stream_kernel(j, n);
    free(L);
    free(mid);
    std::vector<uint32_t> cf(64 * 17);
    for (int p = 0; p < 64; p++)
        for (int q = 0; q < 17; q++)
            cf[(size_t)p * 17 + q] = (uint32_t)(int)LC3T_AC_SPEC_CUMFREQ[p][q] | ((uint32_t)(int)LC3T_AC_SPEC_FREQ[p][q] << 16);
    static uint32_t tns_models[LC3_TNS_MODEL_WORDS];
    for (int i = 0; i < LC3_TNS_MODEL_WORDS; i++) tns_models[i] = lc3_tns_model_word(i);
    memset(bytes, 0, frames * (size_t)nbytes);
    for (size_t f = 0; f < frames; f++) {  // lc3_pack_kernel
        lc3_pack_ctx p;
        uint8_t sink = 0;
        p.buf = bytes + f * (size_t)nbytes;
        p.sink = &sink;
        p.tns = tns_models;
        p.nbytes = nbytes;
        p.lookup = LC3T_AC_SPEC_LOOKUP;
        p.cf = cf.data();
        p.plane = LC3_PLANE_COL(planes.data(), f, EP_WORDS);
        p.stride = LC3_PLANE_STRIDE;
        lc3_pack_frame(p, c.ne);
    }
    return 0;
}

// bytes uint8[n][T][nbytes], bad uint8[n][T] or NULL -> pcm int16[n][T][nf]; late = 0: the reconstruction in the parser (full batches),
// 1: in the synthesis body (small launches)
int lc3emu_list_decode(void *h, const int32_t *list, int n, int T, const uint8_t *bytes, const uint8_t *bad, int16_t *pcm, int late) {
    ListCtx *x = (ListCtx *)h;
    const lc3_cfg &c = x->cfg;
    const int nbytes = x->nbytes;
    const size_t frames = (size_t)n * (size_t)T;
    std::vector<int32_t> planes(((frames + 63) / 64) * 64 * LC3_PLANE_WORDS, 0);
    alignas(16) static uint32_t cf[64 * LC3_DCF_ROW_WORDS];
    for (int i = 0; i < 64 * LC3_DCF_ROW_WORDS; i++) cf[i] = lc3_dcf_word(i);
    std::vector<uint32_t> tns(LC3_TNS_MODEL_WORDS);
    for (int i = 0; i < LC3_TNS_MODEL_WORDS; i++) tns[(size_t)i] = lc3_tns_model_word(i);
    for (size_t f = 0; f < frames; f++) {  // lc3_parse_kernel, unchanged on the compact buffers
        lc3_parse_ctx p;
        p.dbg = nullptr;
        p.tns = tns.data();
        p.bytes = bytes + f * (size_t)nbytes;
        p.len = nbytes;
        p.lookup = LC3T_AC_SPEC_LOOKUP;
        p.cf = cf;
        p.plane = LC3_PLANE_COL(planes.data(), f, LC3_PLANE_WORDS);
        p.stride = LC3_PLANE_STRIDE;
        p.head = 0;
        p.tail = 0;
        const int rc = (bad && bad[f]) ? -100 : lc3_parse_frame<1>(p, c.ne, c.fs_ind, c.n_ms_10);
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
    lc3_dec_lds *L = (lc3_dec_lds *)aligned_alloc(16, LC3_WG_WAVES * sizeof(lc3_dec_lds));
    ListJob j;
    memset(&j, 0, sizeof(j));
    j.x = x;
    j.T = T;
    j.list = list;
    j.DL = L;
    j.dplanes = planes.data();
    j.pcm_out = pcm;
    j.late = late ? 1 : 0;
    j.kind = 3;
    run_stream_kernel(j, n);
    free(L);
    return 0;
}
}
