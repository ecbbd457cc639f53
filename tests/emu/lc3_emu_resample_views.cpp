// TEST INFRASTRUCTURE -- lc3gpu_resample_mixed_views on the CPU: the shared check and plan header (lc3_host_resample_views.h over
// lc3_host_inspect_views.h, both included unchanged: what the companion library runs on the host, and the look-up its kernel makes in the
// uploaded rows) and the kernel's lane body (lc3_rs_stage / lc3_rs_compute / lc3_rs_store, lc3_dev_resample.h) driven THROUGH the plan:
// workgroup by workgroup, every lane of a phase before the next phase begins, as the barriers order them.  An object holds what the
// resampler holds: the channels' book-keeping and the two history buffers per channel.  Build: tests/test_emu_resample_views.py.
#include <climits>
#include <cstdint>
#include <cstring>

#include "../../lc3-codec_amd/csrc/lc3_dev_resample.h"

namespace {
struct Emu {
    int max_views = 0;
    lc3_rs_state state;
    std::vector<int16_t> hist;
    std::vector<lc3_rs_row> rows;
};
}  // namespace

extern "C" {
// out int32[4] = output samples per workgroup, lanes, samples of a history buffer, samples of the LDS window
void lc3emu_rs_info(int32_t *out) {
    out[0] = LC3_RS_CHUNK, out[1] = LC3_RS_LANES, out[2] = LC3_RS_HIST, out[3] = LC3_RS_MAX_WINDOW;
}
unsigned lc3emu_rs_div(int nf, unsigned s) { return lc3_rs_div(s, lc3_rs_magic(nf)); }
unsigned lc3emu_rs_div_l(int L, unsigned u) { return lc3_rs_div_l(u, 65536 / L + 1); }

// descs int32[n][3] = (fs_in_hz, fs_out_hz, frame_us): what lc3rs_create checks before it looks for a device.  *rc = 0 or its code
void *lc3emu_rs_new(const int32_t *descs, int n, int max_views, int32_t *rc) {
    *rc = LC3_IV_EINVAL;
    if (!descs || n < 1 || max_views < 1) return nullptr;
    *rc = LC3_IV_ELENGTH;
    if (n > INT_MAX / (2 * LC3_RS_HIST)) return nullptr;
    Emu *e = new Emu();
    e->max_views = max_views;
    e->state.channels.resize((size_t)n);
    for (int i = 0; i < n; i++)
        if ((*rc = lc3_rs_make_channel(descs[3 * i], descs[3 * i + 1], descs[3 * i + 2], e->state.channels[(size_t)i])) != 0) {
            delete e;
            return nullptr;
        }
    e->hist.assign((size_t)n * 2 * LC3_RS_HIST, (int16_t)0x7e7e);  // (never read before it is written: a fresh channel reads zeros)
    e->rows.resize((size_t)max_views);
    *rc = 0;
    return e;
}
void lc3emu_rs_free(void *h) { delete (Emu *)h; }
// n < 0: all channels.  As lc3rs_reset / lc3rs_reset_channels
int lc3emu_rs_reset(void *h, const int32_t *channels, int n) {
    Emu *e = (Emu *)h;
    if (n < 0) {
        for (lc3_rs_channel &c : e->state.channels) lc3_rs_reset_channel(c);
        return 0;
    }
    for (int i = 0; i < n; i++)
        if (channels[i] < 0 || channels[i] >= (int)e->state.channels.size()) return LC3_IV_ECHANNEL;
    for (int i = 0; i < n; i++) lc3_rs_reset_channel(e->state.channels[(size_t)channels[i]]);
    return 0;
}
// out int32[n_channels][2] = (cur, fresh) of every channel, and the histories as they lie (int16[n_channels][2][LC3_RS_HIST])
void lc3emu_rs_state(void *h, int32_t *out, int16_t *hist) {
    Emu *e = (Emu *)h;
    for (size_t i = 0; i < e->state.channels.size(); i++) out[2 * i] = e->state.channels[i].cur, out[2 * i + 1] = e->state.channels[i].fresh;
    if (hist) memcpy(hist, e->hist.data(), e->hist.size() * sizeof(int16_t));
}

// bounds uint64[4] = in base, in elements, out base, out elements.  Only addresses: nothing is read, and the state is left as it was
// (an accepted call is planned on a copy of it).  *n_wg = workgroups of the plan
int lc3emu_rs_check(void *h, const void *in_views, const void *out_views, int n_views, const uint64_t *bounds, int32_t *n_wg) {
    Emu *e = (Emu *)h;
    lc3_rs_bounds B = {bounds[0], bounds[1], bounds[2], bounds[3]};
    *n_wg = 0;
    const int rc = lc3_rviews_check(e->state, e->max_views, (const lc3_iview *)in_views, (const lc3_iview *)out_views, n_views, B);
    if (rc || n_views == 0) return rc;
    lc3_rs_state copy = e->state;
    lc3_rviews_build(copy, (const lc3_iview *)in_views, (const lc3_iview *)out_views, n_views, e->rows.data());
    *n_wg = copy.n_wg;
    return rc;
}

// The whole call on host arrays: check, plan, then every workgroup with the kernel's lane body.  Returns the call's code; a refused call
// writes nothing and advances nothing.  hits (may be null): uint8[out_elems], incremented for every output sample a workgroup's store
// phase names -- what the coverage test reads; with hits given nothing is computed, pcm_out is not written and the state is left as it
// was.  -1000: a lane would read or write outside the extents, the histories or the LDS arrays
int lc3emu_rs_run(void *h, const void *in_views, const int16_t *pcm_in, uint64_t in_elems, const void *out_views, int16_t *pcm_out,
                  uint64_t out_elems, int n_views, uint8_t *hits) {
    Emu *e = (Emu *)h;
    lc3_rs_bounds B = {(uint64_t)(uintptr_t)pcm_in, in_elems, (uint64_t)(uintptr_t)pcm_out, out_elems};
    const lc3_iview *vi = (const lc3_iview *)in_views, *vo = (const lc3_iview *)out_views;
    const int rc = lc3_rviews_check(e->state, e->max_views, vi, vo, n_views, B);
    if (rc || n_views == 0) return rc;
    lc3_rs_state before = e->state;
    lc3_rviews_build(e->state, vi, vo, n_views, e->rows.data());
    const int n_wg = e->state.n_wg;
    if (hits) e->state = before;
    static lc3_rs_lds lds;
    const int hist_len = (int)e->hist.size();
    for (int wg = 0; wg < n_wg; wg++) {
        const lc3_rs_row &r = e->rows[(size_t)lc3_rs_find_row(e->rows.data(), n_views, wg)];
        const int chunk = wg - r.wg0;
        const lc3_rs_chunk c = lc3_rs_chunk_of(r, chunk);
        // where the lane body will go, looked at before it goes there
        if (c.n_out < 1 || c.n_out > LC3_RS_CHUNK || (c.n_out & 1) || c.m0 + c.n_out > r.S_out || 2 * c.n_pairs > LC3_RS_MAX_WINDOW ||
            r.L * r.T > LC3_RS_MAX_COEF || r.T - 1 > LC3_RS_HIST || c.kw0 < -r.T || c.b0 - c.kw0 < r.T - 1)
            return -1000;
        if (r.hist_rd >= hist_len || r.hist_rd + LC3_RS_HIST > hist_len || r.hist_wr < 0 || r.hist_wr + LC3_RS_HIST > hist_len ||
            (r.hist_rd >= 0 && r.hist_rd == r.hist_wr))
            return -1000;
        for (int i = 0; i < c.n_pairs; i++) {
            const int k = c.kw0 + 2 * i;
            if (k < 0 || k >= r.S_in) continue;
            const uint64_t at = lc3_rs_place(r.in_off, r.in_magic, r.nf_in, r.in_pitch, r.in_stride, (uint32_t)k);
            if (at >= in_elems || (uint64_t)r.in_stride >= in_elems - at) return -1000;
        }
        // (the last output's tap 0 lies inside the window and inside the view)
        const int b_last = c.b0 + (int)(((int64_t)(c.n_out - 1) * r.M) / r.L);
        if (b_last >= r.S_in || b_last - c.kw0 >= 2 * c.n_pairs) return -1000;
        for (int i = 0; 2 * i < c.n_out; i++) {
            const uint64_t at = lc3_rs_place(r.out_off, r.out_magic, r.nf_out, r.out_pitch, r.out_stride, (uint32_t)(c.m0 + 2 * i));
            if (at >= out_elems || (uint64_t)r.out_stride >= out_elems - at) return -1000;
            if (hits) hits[at]++, hits[at + (uint64_t)r.out_stride]++;
        }
        if (hits) continue;
        for (int tid = 0; tid < LC3_RS_LANES; tid++) lc3_rs_stage(r, c, tid, lds, pcm_in, e->hist.data());
        for (int tid = 0; tid < LC3_RS_LANES; tid++) lc3_rs_compute(r, c, tid, lds);
        for (int tid = 0; tid < LC3_RS_LANES; tid++) lc3_rs_store(r, c, chunk, tid, lds, pcm_in, pcm_out, e->hist.data());
    }
    return 0;
}
}
