// TEST INFRASTRUCTURE -- lc3gpu_inspect_mixed_views on the CPU: the shared check and plan header (lc3_host_inspect_views.h, included
// unchanged: what the companion library runs on the host, and the two look-ups its kernel makes in the uploaded tables) and the kernel's
// lane body (lc3_inspect_record over lc3_dev_dec_inspect.h) driven THROUGH the plan: workgroup by workgroup, lane by lane, every lane
// finding its frame the way the kernel's lane does.  The kernel's own block code (LDS staging, the record copy-out) is checked by the GPU
// tests.  Build: tests/test_emu_inspect_views.py.
#include "lc3_emu.cpp"

#include "../../lc3-codec_amd/csrc/lc3_dev_dec_inspect.h"
#include "../../lc3-codec_amd/csrc/lc3_host_inspect_views.h"

static_assert(LC3_IV_LDS_FIXED == 4096 + 64 * LC3_DCF_ROW_WORDS * 4 + LC3_TNS_MODEL_WORDS * 4, "fixed LDS");
static_assert(LC3_IV_LDS_PER_FRAME == 4 * LC3_FI_WORDS + 8 + 4 * LC3_INSPECT_BITS_WORDS, "LDS per frame");

namespace {
// descs int32[n][3] = (fs_hz, frame_us, nbytes) -> the inspector's streams, as lc3insp_create makes them; 0 or the create call's code
int make_streams(const int32_t *descs, int n, std::vector<lc3_iv_stream> &out) {
    out.resize((size_t)n);
    for (int i = 0; i < n; i++) {
        if (lc3_iv_config(descs[3 * i + 1], descs[3 * i], out[(size_t)i])) return LC3_IV_EINVAL;
        if (descs[3 * i + 2] < 1 || descs[3 * i + 2] > LC3_IV_MAX_NBYTES) return LC3_IV_ELENGTH;
        out[(size_t)i].nbytes = descs[3 * i + 2];
        lc3_cfg c;  // the plan's own configuration constants are the codec's
        if (lc3_make_config(c, descs[3 * i + 1], descs[3 * i]) || c.ne != out[(size_t)i].ne || c.fs_ind != out[(size_t)i].fs_ind ||
            c.n_ms_10 != out[(size_t)i].n_ms_10)
            return -100;
    }
    return 0;
}
lc3_iv_bounds make_bounds(const uint64_t *b) {
    lc3_iv_bounds B;
    B.in_base = b[0], B.in_bytes = b[1], B.flags_base = b[2], B.n_flags = b[3];
    B.status_base = b[4], B.n_status = b[5], B.info_base = b[6], B.n_info = b[7];
    B.use_flags = b[2] != 0, B.use_status = b[4] != 0, B.use_info = b[6] != 0;
    return B;
}
}  // namespace

extern "C" {
// bounds uint64[8] = in base, in bytes, flags base, n_flags, status base, n_status, info base, n_info (a base of 0: the array is not given).
// Only addresses: nothing is read.  out int32[2] = frames, max_nbytes
int lc3emu_iv_check(const int32_t *descs, int n_streams, int max_views, const void *views, int n_views, const uint64_t *bounds, int32_t *out) {
    std::vector<lc3_iv_stream> streams;
    const int rc = make_streams(descs, n_streams, streams);
    if (rc) return rc;
    int frames = 0, max_nb = 0;
    const int r = lc3_iviews_check(streams.data(), n_streams, max_views, (const lc3_iview *)views, n_views, make_bounds(bounds), &frames, &max_nb);
    out[0] = frames;
    out[1] = max_nb;
    return r;
}
int lc3emu_iv_fpb(int max_nbytes) { return (int)lc3_iv_fpb(max_nbytes); }
long long lc3emu_iv_lds(int max_nbytes) { return (long long)lc3_iv_lds_bytes(max_nbytes); }

// The plan of checked views with `fpb` frames per workgroup (0: the call's own), spelled out lane by lane with the kernel's look-ups:
// lanes int64[frames][4] = (workgroup, lane, src, dst) in launch order, wgs int32[n_wg][5] = (bucket, frames, nbytes, ne, fs_ind_ms).
// out int32[3] = n_buckets, n_wg, fpb.  Returns 0, or -1 when lanes / wgs are too short (max_lanes, max_wgs)
int lc3emu_iv_plan(const int32_t *descs, int n_streams, const void *views, int n_views, int fpb, int max_nbytes, int64_t *lanes, long long max_lanes,
                   int32_t *wgs, int max_wgs, int32_t *out) {
    std::vector<lc3_iv_stream> streams;
    if (make_streams(descs, n_streams, streams)) return -2;
    if (fpb == 0) fpb = (int)lc3_iv_fpb(max_nbytes);
    std::vector<lc3_iv_row> rows((size_t)n_views);
    std::vector<lc3_iv_bucket> buckets((size_t)n_views);
    static lc3_iv_plan P;  // (kept across calls, as the inspector keeps its plan: a call must leave the counters clean)
    lc3_iviews_build(streams.data(), (const lc3_iview *)views, n_views, fpb, rows.data(), buckets.data(), P);
    for (int k : P.key_views)
        if (k) return -3;
    for (int k : P.key_frames)
        if (k) return -3;
    out[0] = P.n_buckets, out[1] = P.n_wg, out[2] = fpb;
    if (P.n_wg > max_wgs) return -1;
    long long n = 0;
    for (int wg = 0; wg < P.n_wg; wg++) {
        const int bi = lc3_iv_find_bucket(buckets.data(), P.n_buckets, wg);
        const lc3_iv_bucket &b = buckets[(size_t)bi];
        const int nfr = lc3_iv_wg_frames(b, wg, fpb);
        wgs[5 * wg] = bi, wgs[5 * wg + 1] = nfr, wgs[5 * wg + 2] = b.nbytes, wgs[5 * wg + 3] = b.ne, wgs[5 * wg + 4] = b.fs_ind_ms;
        for (int tid = 0; tid < nfr; tid++, n++) {
            if (n >= max_lanes) return -1;
            uint64_t src, dst;
            lc3_iv_lane_place(rows.data(), b, wg, tid, fpb, src, dst);
            lanes[4 * n] = wg, lanes[4 * n + 1] = tid, lanes[4 * n + 2] = (int64_t)src, lanes[4 * n + 3] = (int64_t)dst;
        }
    }
    return 0;
}

// The whole call on host arrays: check, plan, then every workgroup's lanes with the kernel's lane body.  status / info may be null (not
// both), bad may be null.  Returns the call's code; a refused call writes nothing.
int lc3emu_iv_run(const int32_t *descs, int n_streams, int max_views, const void *views, int n_views, const uint8_t *in, uint64_t in_bytes,
                  const uint8_t *bad, uint64_t n_flags, uint8_t *status, uint64_t n_status, int32_t *info, uint64_t n_info) {
    std::vector<lc3_iv_stream> streams;
    int rc = make_streams(descs, n_streams, streams);
    if (rc) return rc;
    const uint64_t bounds[8] = {(uint64_t)(uintptr_t)in,     in_bytes, (uint64_t)(uintptr_t)bad,  n_flags,
                                (uint64_t)(uintptr_t)status, n_status, (uint64_t)(uintptr_t)info, n_info};
    int frames = 0, max_nb = 0;
    rc = lc3_iviews_check(streams.data(), n_streams, max_views, (const lc3_iview *)views, n_views, make_bounds(bounds), &frames, &max_nb);
    if (rc || n_views == 0) return rc;
    const int fpb = (int)lc3_iv_fpb(max_nb);
    std::vector<lc3_iv_row> rows((size_t)n_views);
    std::vector<lc3_iv_bucket> buckets((size_t)n_views);
    lc3_iv_plan P;
    lc3_iviews_build(streams.data(), (const lc3_iview *)views, n_views, fpb, rows.data(), buckets.data(), P);
    alignas(16) static uint32_t cf[64 * LC3_DCF_ROW_WORDS];
    for (int i = 0; i < 64 * LC3_DCF_ROW_WORDS; i++) cf[i] = lc3_dcf_word(i);
    static uint32_t tns[LC3_TNS_MODEL_WORDS];
    for (int i = 0; i < LC3_TNS_MODEL_WORDS; i++) tns[i] = lc3_tns_model_word(i);
    std::vector<uint8_t> bytes;
    uint32_t bits[LC3_INSPECT_BITS_WORDS];
    int32_t rec[LC3_FI_WORDS];
    for (int wg = 0; wg < P.n_wg; wg++) {
        const lc3_iv_bucket &b = buckets[(size_t)lc3_iv_find_bucket(buckets.data(), P.n_buckets, wg)];
        const int nfr = lc3_iv_wg_frames(b, wg, fpb);
        for (int tid = 0; tid < nfr; tid++) {
            uint64_t src, dst;
            lc3_iv_lane_place(rows.data(), b, wg, tid, fpb, src, dst);
            bytes.assign(in + src, in + src + b.nbytes);  // (the lane's LDS slot)
            memset(bits, 0xA5, sizeof(bits));             // stale flags from another frame must not matter
            for (int w = 0; w < LC3_FI_WORDS; w++) rec[w] = (int32_t)0xDEADBEEF;
            lc3_parse_ctx c;
            c.dbg = nullptr;
            c.bytes = bytes.data();
            c.lookup = LC3T_AC_SPEC_LOOKUP;
            c.cf = cf;
            c.tns = tns;
            lc3_inspect_record(c, bad && bad[dst], b.nbytes, rec, bits, 1, b.ne, b.fs_ind_ms & 0xff, b.fs_ind_ms >> 8);
            if (status) status[dst] = (uint8_t)rec[LC3_FI_STATUS];
            if (info) memcpy(info + dst * LC3_FI_WORDS, rec, sizeof(rec));
        }
    }
    return 0;
}
}
