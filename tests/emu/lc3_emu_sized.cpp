// TEST INFRASTRUCTURE -- the CPU wave emulator (lc3_emu.cpp, included unchanged) with a frame size per frame: the bodies of
// lc3_enc_front_vbr_kernel and lc3_enc_back_vbr_kernel (lc3gpu.hip) over the device headers, four emulated waves per workgroup, then the
// packer's per-frame code (lc3_pack_frame at the frame's size) one frame at a time.  The sized packer KERNEL's own block code -- LDS staging
// at tid * slot, the size table, the guarded copy-out -- is not emulated here; the GPU tests check it with a sentinel in every slot.
// A size-dependent branch around a workgroup barrier deadlocks here (the pthread barrier waits for all four waves), which the tests turn
// into a failure with a time limit.  Build: tests/test_emu_sized.py.
#include "lc3_emu.cpp"

#include "../../lc3-codec_amd/csrc/lc3_dev_enc_vbr.h"

namespace {
struct SizedJob {
    lc3_cfg cfg;
    int lane, wave, valid, phase_kind;  // 1 front half, 2 back half
    int s, wg_s0, S, T, slot, spec_flags;
    const uint16_t *nb;
    lc3_enc_lds *EL;
    lc3_enc_state *est;
    const int16_t *pcm_in;  // this stream's frames
    float *mid;
    int32_t *planes;
    unsigned long long *clamps;
};

void *sized_lane_main(void *arg) {
    SizedJob *j = (SizedJob *)arg;
    const int lane = j->lane;
    tl_wave = j->wave;
    lc3_enc_lds &L = j->EL[j->wave];
    const size_t fbase = (size_t)j->s * (size_t)j->T;
    if (lane == 0) L.spec_flags = j->spec_flags;
    if (j->phase_kind == 1) {  // as lc3_enc_front_vbr_kernel
        lc3_enc_state_init(L, lane, j->est, j->valid);
        for (int t = 0; t < j->T; t++) {
            const size_t f = fbase + (size_t)t;
            int32_t *plane = j->valid ? LC3_PLANE_COL(j->planes, f, EP_WORDS) : nullptr;
            float *mcol = j->valid ? j->mid + f * (size_t)MP_WORDS : nullptr;
            const int16_t *frame = j->pcm_in + (size_t)t * j->cfg.nf;
            const int16_t *hist = t > 0 ? frame - j->cfg.nf + j->cfg.z : nullptr;
            int clamped;
            const int nbytes = lc3_vbr_enc_size(j->nb, f, j->slot, &clamped);
            if (j->valid && clamped && lane == 0) __atomic_add_fetch(j->clamps, 1ull, __ATOMIC_RELAXED);
            const int phase = lc3_vbr_front_phase(j->cfg, j->nb, j->slot, j->wg_s0, j->S, t, j->T, LC3_WG_WAVES);
            lc3_encode_front_wave(j->cfg, L, lane, frame, hist, j->est, mcol, plane, LC3_PLANE_STRIDE, nbytes, nullptr, 1, 1, phase);
        }
        if (j->valid) lc3_enc_state_store(j->cfg, L, lane, j->est, j->pcm_in + (size_t)(j->T - 1) * j->cfg.nf);
    } else {  // as lc3_enc_back_vbr_kernel
        lc3_enc_state_load(L, lane, j->est);
        lc3_encode_back_stream_vbr(j->cfg, L, lane, j->mid, j->planes, fbase, j->T, j->nb + fbase, j->slot, j->valid, nullptr);
        if (j->valid) lc3_enc_state_store(j->cfg, L, lane, j->est, nullptr);
    }
    return 0;
}

void run_wg_sized(const SizedJob *protos) {
    static pthread_t th[LC3_WG_WAVES * LC3_WAVE];
    static SizedJob jobs[LC3_WG_WAVES * LC3_WAVE];
    for (int w = 0; w < LC3_WG_WAVES; w++) pthread_barrier_init(&g_wave_bar[w], 0, LC3_WAVE);
    pthread_barrier_init(&g_wg_bar, 0, LC3_WG_WAVES * LC3_WAVE);
    for (int w = 0; w < LC3_WG_WAVES; w++)
        for (int i = 0; i < LC3_WAVE; i++) {
            SizedJob &q = jobs[w * LC3_WAVE + i];
            q = protos[w];
            q.lane = i;
            q.wave = w;
            pthread_create(&th[w * LC3_WAVE + i], 0, sized_lane_main, &q);
        }
    for (int i = 0; i < LC3_WG_WAVES * LC3_WAVE; i++) pthread_join(th[i], 0);
    for (int w = 0; w < LC3_WG_WAVES; w++) pthread_barrier_destroy(&g_wave_bar[w]);
    pthread_barrier_destroy(&g_wg_bar);
}
}  // namespace

extern "C" {
// pcm int16[S][T][nf], nb uint16[S][T] -> bytes uint8[S][T][slot] (frame (s, t) in the first clamp(nb[s][t]) bytes of its slot, the rest
// untouched); every stream starts fresh; *clamps += the sizes clamped into [20, slot]
int lc3emu_encode_sized(int fs_hz, int frame_us, int slot, int S, int T, const int16_t *pcm, const uint16_t *nb, uint8_t *bytes,
                        unsigned long long *clamps) {
    SizedJob j;
    memset(&j, 0, sizeof(j));
    lc3_host_plan pl;
    if (lc3_make_config(j.cfg, frame_us, fs_hz) || lc3_make_plan(j.cfg, pl)) return -1;
    j.cfg.fft_tw = pl.fft_tw.data();
    j.cfg.dct_tw = pl.dct_tw.data();
    j.cfg.perm = pl.perm.data();
    std::vector<float> poly((size_t)j.cfg.p_up * (size_t)j.cfg.resamp_stride);
    for (size_t i = 0; i < poly.size(); i++) poly[i] = lc3_resamp_poly_value(j.cfg.p_up, j.cfg.resamp_lim, j.cfg.resamp_stride, (int)i);
    j.cfg.resamp_poly = poly.data();
    std::vector<float> lw((size_t)j.cfg.ne);
    for (int k = 0; k < j.cfg.ne; k++) lw[(size_t)k] = lc3_line_width_value(j.cfg, k);
    j.cfg.line_width = lw.data();
    std::vector<uint8_t> lb((size_t)j.cfg.nf + 16);
    for (int k = 0; k < j.cfg.nf; k++) lb[(size_t)k] = (uint8_t)lc3_line_band_value(j.cfg, k);
    j.cfg.line_band = lb.data();
    const size_t frames = (size_t)S * (size_t)T;
    std::vector<int32_t> planes(((frames + 63) / 64) * 64 * EP_WORDS, 0);
    lc3_enc_lds *L = (lc3_enc_lds *)aligned_alloc(16, LC3_WG_WAVES * sizeof(lc3_enc_lds));
    lc3_enc_state *st = (lc3_enc_state *)aligned_alloc(16, (size_t)S * sizeof(lc3_enc_state));
    float *mid = (float *)aligned_alloc(16, frames * (size_t)MP_WORDS * sizeof(float));
    memset(st, 0, (size_t)S * sizeof(lc3_enc_state));
    memset(mid, 0, frames * (size_t)MP_WORDS * sizeof(float));
    j.S = S;
    j.T = T;
    j.slot = slot;
    j.nb = nb;
    j.EL = L;
    j.mid = mid;
    j.planes = planes.data();
    j.clamps = clamps;
    for (int phase = 1; phase <= 2; phase++) {
        for (int s0 = 0; s0 < S; s0 += LC3_WG_WAVES) {
            SizedJob protos[LC3_WG_WAVES];
            memset(L, 0xFF, LC3_WG_WAVES * sizeof(lc3_enc_lds));
            for (int w = 0; w < LC3_WG_WAVES; w++) {
                const int valid = s0 + w < S, s = valid ? s0 + w : S - 1;
                protos[w] = j;
                protos[w].phase_kind = phase;
                protos[w].valid = valid;
                protos[w].s = s;
                protos[w].wg_s0 = s0;
                protos[w].est = st + s;
                protos[w].pcm_in = pcm + (size_t)s * T * j.cfg.nf;
            }
            run_wg_sized(protos);
        }
        if (phase == 1) {
            for (size_t f = 0; f < frames; f++) {  // lc3_sns_vq_kernel
                lc3_vq_ctx v;
                v.mid = mid + f * (size_t)MP_WORDS;
                v.gains = mid + f * (size_t)MP_WORDS + MP_G;
                v.plane = LC3_PLANE_COL(planes.data(), f, EP_WORDS);
                v.stride = LC3_PLANE_STRIDE;
                v.mpvq = &LC3T_MPVQ_OFFSETS[0][0];
                v.nb = j.cfg.nb;
                v.spec_flags = 0;
                lc3_sns_vq_frame(v);
            }
        }
    }
    free(L);
    free(st);
    free(mid);
    // the packer's per-frame code at each frame's size (lc3_pack_vbr_kernel's block staging and copy-out are not emulated)
    std::vector<uint32_t> cf(64 * 17);
    for (int p = 0; p < 64; p++)
        for (int q = 0; q < 17; q++)
            cf[(size_t)p * 17 + q] = (uint32_t)(int)LC3T_AC_SPEC_CUMFREQ[p][q] | ((uint32_t)(int)LC3T_AC_SPEC_FREQ[p][q] << 16);
    static uint32_t tns_models[LC3_TNS_MODEL_WORDS];
    for (int i = 0; i < LC3_TNS_MODEL_WORDS; i++) tns_models[i] = lc3_tns_model_word(i);
    std::vector<uint8_t> stage((size_t)slot);
    for (size_t f = 0; f < frames; f++) {
        const int n = lc3_vbr_enc_size(nb, f, slot);
        lc3_pack_ctx c;
        uint8_t sink = 0;
        memset(stage.data(), 0, (size_t)slot);
        c.buf = stage.data();
        c.sink = &sink;
        c.tns = tns_models;
        c.nbytes = n;
        c.lookup = LC3T_AC_SPEC_LOOKUP;
        c.cf = cf.data();
        c.plane = LC3_PLANE_COL(planes.data(), f, EP_WORDS);
        c.stride = LC3_PLANE_STRIDE;
        lc3_pack_frame(c, j.cfg.ne);
        memcpy(bytes + f * (size_t)slot, stage.data(), (size_t)n);
    }
    return 0;
}
}
