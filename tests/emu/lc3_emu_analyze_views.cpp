// TEST INFRASTRUCTURE -- lc3gpu_analyze_mixed_views on the CPU: the shared check header (lc3_host_analyze_views.h over
// lc3_host_inspect_views.h, both included unchanged: what the companion library runs on the host, and the look-ups its kernel makes in the
// uploaded tables) and the kernel's lane body (lc3_analyze_frame, lc3_dev_dec_analyze.h) driven THROUGH the plan: workgroup by workgroup,
// lane by lane, every lane finding its frame and its scratch column the way the kernel's lane does.  The kernel's own block code (LDS
// staging, the rows' stores) is checked by the GPU tests.  Build: tests/test_emu_analyze_views.py.
#include "lc3_emu.cpp"

#include "../../lc3-codec_amd/csrc/lc3_dev_dec_analyze.h"
#include "../../lc3-codec_amd/csrc/lc3_host_analyze_views.h"

static_assert(LC3_AV_LDS_FIXED == 4096 + 64 * LC3_DCF_ROW_WORDS * 4 + 16 * 11 * 4 + LC3_TNS_MODEL_WORDS * 4 + 144, "fixed LDS");
static_assert(LC3_AV_COLUMN_WORDS == LC3_PLANE_WORDS && LC3_AV_SPEC_LINES == LC3_MAX_NE, "the column");

namespace {
// descs int32[n][3] = (fs_hz, frame_us, nbytes) -> the analyzer's streams, as lc3ana_create makes them; 0 or the create call's code
int make_streams(const int32_t *descs, int n, std::vector<lc3_iv_stream> &out) {
    out.resize((size_t)n);
    for (int i = 0; i < n; i++) {
        if (lc3_iv_config(descs[3 * i + 1], descs[3 * i], out[(size_t)i])) return LC3_IV_EINVAL;
        if (descs[3 * i + 2] < 1 || descs[3 * i + 2] > LC3_IV_MAX_NBYTES) return LC3_IV_ELENGTH;
        out[(size_t)i].nbytes = descs[3 * i + 2];
        lc3_cfg c;  // the plan's own configuration constants, the band count included, are the codec's
        if (lc3_make_config(c, descs[3 * i + 1], descs[3 * i]) || c.ne != out[(size_t)i].ne || c.fs_ind != out[(size_t)i].fs_ind ||
            c.n_ms_10 != out[(size_t)i].n_ms_10 || c.nb != lc3_av_bands(c.fs_ind, c.n_ms_10))
            return -100;
    }
    return 0;
}
lc3_av_bounds make_bounds(const uint64_t *b) {
    lc3_av_bounds B;
    B.in_base = b[0], B.in_bytes = b[1], B.flags_base = b[2], B.n_flags = b[3];
    B.energy_base = b[4], B.n_energy = b[5], B.bands_base = b[6], B.n_bands = b[7], B.spec_base = b[8], B.n_spec = b[9];
    B.use_flags = b[2] != 0, B.use_energy = b[4] != 0, B.use_bands = b[6] != 0, B.use_spec = b[8] != 0;
    return B;
}
}  // namespace

extern "C" {
// bounds uint64[10] = in base, in bytes, flags base, n_flags, energy base, n_energy, bands base, n_bands, spec base, n_spec (a base of 0: the
// array is not given).  Only addresses: nothing is read.  out int32[2] = frames, max_nbytes.  max_frames < 1: the create call's refusal
int lc3emu_av_check(const int32_t *descs, int n_streams, int max_views, int max_frames, const void *views, int n_views, const uint64_t *bounds,
                    int32_t *out) {
    std::vector<lc3_iv_stream> streams;
    const int rc = make_streams(descs, n_streams, streams);
    if (rc) return rc;
    if (max_views < 1 || max_frames < 1) return LC3_IV_EINVAL;
    int frames = 0, max_nb = 0;
    const int r = lc3_aviews_check(streams.data(), n_streams, max_views, max_frames, (const lc3_iview *)views, n_views, make_bounds(bounds), &frames,
                                   &max_nb);
    out[0] = frames;
    out[1] = max_nb;
    return r;
}
int lc3emu_av_fpb(int max_nbytes) { return (int)lc3_av_fpb(max_nbytes); }
long long lc3emu_av_lds(int max_nbytes) { return (long long)lc3_av_lds_bytes(max_nbytes); }

// The whole call on host arrays: check, plan, then every workgroup's lanes with the kernel's lane body, each in the scratch column the
// kernel gives it.  energy / bands / spec may be null (not all three), bad may be null.  Returns the call's code; a refused call writes
// nothing.  -1000: a lane's column would lie beyond max_frames columns
int lc3emu_av_run(const int32_t *descs, int n_streams, int max_views, int max_frames, const void *views, int n_views, const uint8_t *in,
                  uint64_t in_bytes, const uint8_t *bad, uint64_t n_flags, float *energy, uint64_t n_energy, float *bands, uint64_t n_bands,
                  float *spec, uint64_t n_spec) {
    std::vector<lc3_iv_stream> streams;
    int rc = make_streams(descs, n_streams, streams);
    if (rc) return rc;
    const uint64_t bounds[10] = {(uint64_t)(uintptr_t)in,     in_bytes, (uint64_t)(uintptr_t)bad,   n_flags, (uint64_t)(uintptr_t)energy, n_energy,
                                 (uint64_t)(uintptr_t)bands, n_bands,  (uint64_t)(uintptr_t)spec, n_spec};
    int frames = 0, max_nb = 0;
    rc = lc3_aviews_check(streams.data(), n_streams, max_views, max_frames, (const lc3_iview *)views, n_views, make_bounds(bounds), &frames, &max_nb);
    if (rc || n_views == 0) return rc;
    const int fpb = (int)lc3_av_fpb(max_nb);
    std::vector<lc3_iv_row> rows((size_t)n_views);
    std::vector<lc3_iv_bucket> buckets((size_t)n_views);
    lc3_iv_plan P;
    lc3_iviews_build(streams.data(), (const lc3_iview *)views, n_views, fpb, rows.data(), buckets.data(), P);
    alignas(16) static uint32_t cf[64 * LC3_DCF_ROW_WORDS];
    for (int i = 0; i < 64 * LC3_DCF_ROW_WORDS; i++) cf[i] = lc3_dcf_word(i);
    static uint32_t tns[LC3_TNS_MODEL_WORDS];
    for (int i = 0; i < LC3_TNS_MODEL_WORDS; i++) tns[i] = lc3_tns_model_word(i);
    // the analyzer's columns: max_frames of them, never cleared between frames or calls (stale words of another frame must not matter)
    int32_t *columns = (int32_t *)aligned_alloc(16, (size_t)max_frames * LC3_PLANE_WORDS * sizeof(int32_t));
    if (!columns) return -1001;
    memset(columns, 0xA5, (size_t)max_frames * LC3_PLANE_WORDS * sizeof(int32_t));
    std::vector<uint8_t> bytes;
    float scf[16];
    int ret = 0;
    for (int wg = 0; wg < P.n_wg && !ret; wg++) {
        const lc3_iv_bucket &b = buckets[(size_t)lc3_iv_find_bucket(buckets.data(), P.n_buckets, wg)];
        const int nfr = lc3_iv_wg_frames(b, wg, fpb);
        lc3_an_cfg cfg;
        cfg.ne = b.ne, cfg.fs_ind = b.fs_ind_ms & 0xff, cfg.n_ms_10 = b.fs_ind_ms >> 8;
        cfg.nb = lc3_av_bands(cfg.fs_ind, cfg.n_ms_10);
        const long long f0 = (long long)b.frame0 + (long long)(wg - b.wg0) * fpb;
        for (int tid = 0; tid < nfr; tid++) {
            if (f0 + tid >= max_frames) {
                ret = -1000;
                break;
            }
            uint64_t src, dst;
            lc3_iv_lane_place(rows.data(), b, wg, tid, fpb, src, dst);
            bytes.assign(in + src, in + src + b.nbytes);  // (the lane's LDS slot)
            int32_t *col = columns + (size_t)(f0 + tid) * LC3_PLANE_WORDS;
            int ok = 0;
            float e = -1.0f;
            if (!(bad && bad[dst])) {
                lc3_parse_ctx c;
                c.dbg = nullptr;
                c.bytes = bytes.data();
                c.len = b.nbytes;
                c.lookup = LC3T_AC_SPEC_LOOKUP;
                c.cf = cf;
                c.tns = tns;
                c.plane = col;
                c.stride = LC3_PLANE_STRIDE;
                lc3_recon_ctx r;
                r.scf = scf;
                r.sstride = 1;
                r.mpvq = &LC3T_MPVQ_OFFSETS[0][0];
                r.ifs = lc3_band_index(cfg);
                float got = 0.0f;
                ok = lc3_analyze_frame(c, r, cfg, bands != nullptr, got);
                e = ok ? got : -1.0f;
            }
            if (energy) energy[dst] = e;
            if (spec)
                for (int k = 0; k < LC3_AV_SPEC_LINES; k++) spec[dst * LC3_AV_SPEC_LINES + k] = (ok && k < cfg.ne) ? ((const float *)(col + LC3_PLANE_X))[k] : 0.0f;
            if (bands)
                for (int q = 0; q < LC3_AV_BANDS; q++) bands[dst * LC3_AV_BANDS + q] = ok ? ((const float *)(col + LC3_PLANE_LEV))[q] : 0.0f;
        }
    }
    free(columns);
    return ret;
}
}
