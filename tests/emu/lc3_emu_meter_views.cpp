// TEST INFRASTRUCTURE -- lc3gpu_measure_mixed_views on the CPU: the shared check and row header (lc3_host_measure_views.h over
// lc3_host_inspect_views.h, both included unchanged: what the companion library runs on the host) and the kernel's lane body
// (lc3_lvl_lane / lc3_lvl_combine / lc3_lvl_finish, lc3_dev_level.h) driven THROUGH the rows: workgroup by workgroup, wave by wave, the
// wave's frames in order, the lanes' partials folded in DESCENDING lane order (the combine is associative and commutative: the kernel's
// shuffle tree and this fold give the same record).  An object holds what the meter holds: the channels' book-keeping and one state record
// per channel.  Build: tests/test_emu_meter_views.py.
#include <climits>
#include <cstdint>
#include <cstring>

#include "../../lc3-codec_amd/csrc/lc3_dev_level.h"

namespace {
struct Emu {
    int max_views = 0;
    lc3_mt_state state;
    std::vector<lc3_mt_dstate> dstate;
    std::vector<lc3_mt_row> rows;
};
}  // namespace

extern "C" {
// out int32[5] = waves per workgroup, lanes per workgroup, lanes of a wave, bytes of a state, bytes of a row
void lc3emu_mt_info(int32_t *out) {
    out[0] = LC3_MT_WAVES_PER_WG, out[1] = LC3_MT_LANES, out[2] = LC3_MT_WAVE, out[3] = LC3_MT_STATE_BYTES, out[4] = (int32_t)sizeof(lc3_mt_row);
}

// descs int32[n][6] = (fs_hz, frame_us, attack_q15, release_q15, threshold (its bits), hang_frames): what lc3mtr_create checks before it
// looks for a device.  *rc = 0 or its code
void *lc3emu_mt_new(const int32_t *descs, int n, int max_views, int32_t *rc) {
    *rc = LC3_IV_EINVAL;
    if (!descs || n < 1 || max_views < 1) return nullptr;
    Emu *e = new Emu();
    e->max_views = max_views;
    e->state.channels.resize((size_t)n);
    for (int i = 0; i < n; i++) {
        const int32_t *d = descs + 6 * i;
        if ((*rc = lc3_mt_make_channel(d[0], d[1], d[2], d[3], (uint32_t)d[4], d[5], e->state.channels[(size_t)i])) != 0) {
            delete e;
            return nullptr;
        }
    }
    lc3_mt_dstate junk = {0x7e7e7e7e, 0x7e7e7e7eu, 0x7e7e7e7e, 0x7e7e7e7e};  // (never read before it is written: a fresh channel starts from zeros)
    e->dstate.assign((size_t)n, junk);
    e->rows.resize((size_t)max_views);
    *rc = 0;
    return e;
}
void lc3emu_mt_free(void *h) { delete (Emu *)h; }
// n < 0: all channels.  As lc3mtr_reset / lc3mtr_reset_channels
int lc3emu_mt_reset(void *h, const int32_t *channels, int n) {
    Emu *e = (Emu *)h;
    if (n < 0) {
        for (lc3_mt_channel &c : e->state.channels) lc3_mt_reset_channel(c);
        return 0;
    }
    for (int i = 0; i < n; i++)
        if (channels[i] < 0 || channels[i] >= (int)e->state.channels.size()) return LC3_IV_ECHANNEL;
    for (int i = 0; i < n; i++) lc3_mt_reset_channel(e->state.channels[(size_t)channels[i]]);
    return 0;
}
// out int32[n_channels][4] = (fresh, last, env, hang) of every channel: the host's flag and the record as it lies
void lc3emu_mt_state(void *h, int32_t *out) {
    Emu *e = (Emu *)h;
    for (size_t i = 0; i < e->state.channels.size(); i++) {
        out[4 * i] = e->state.channels[i].fresh;
        out[4 * i + 1] = e->dstate[i].last, out[4 * i + 2] = (int32_t)e->dstate[i].env, out[4 * i + 3] = e->dstate[i].hang;
    }
}

// bounds uint64[8] = pcm base, pcm elements, active base, active bytes, levels base, levels records, use_active, use_levels.  Only
// addresses: nothing is read, and the state is left as it was
int lc3emu_mt_check(void *h, const void *views, int n_views, const uint64_t *b) {
    Emu *e = (Emu *)h;
    lc3_mt_bounds B = {b[0], b[1], b[2], b[3], b[4], b[5], (int)b[6], (int)b[7]};
    return lc3_mviews_check(e->state, e->max_views, (const lc3_iview *)views, n_views, B);
}

// The whole call on host arrays: check, rows, then every wave of every workgroup with the kernel's lane body.  Returns the call's code; a
// refused call writes nothing and advances nothing.  -1000: a lane would read or write outside the extents or the states
int lc3emu_mt_run(void *h, const void *views, int n_views, const int16_t *pcm, uint64_t pcm_elems, uint8_t *active, uint64_t n_active, uint8_t *levels,
                  uint64_t n_levels) {
    Emu *e = (Emu *)h;
    lc3_mt_bounds B = {(uint64_t)(uintptr_t)pcm, pcm_elems, (uint64_t)(uintptr_t)active, n_active, (uint64_t)(uintptr_t)levels, n_levels, active != nullptr,
                       levels != nullptr};
    const lc3_iview *vi = (const lc3_iview *)views;
    const int rc = lc3_mviews_check(e->state, e->max_views, vi, n_views, B);
    if (rc || n_views == 0) return rc;
    lc3_mviews_build(e->state, vi, n_views, e->rows.data());
    const int n_wg = (n_views + LC3_MT_WAVES_PER_WG - 1) / LC3_MT_WAVES_PER_WG;
    for (int wg = 0; wg < n_wg; wg++)
        for (int wave = 0; wave < LC3_MT_WAVES_PER_WG; wave++) {
            const int v = wg * LC3_MT_WAVES_PER_WG + wave;
            if (v >= n_views) continue;
            const lc3_mt_row r = e->rows[(size_t)v];
            if (r.channel < 0 || (size_t)r.channel >= e->dstate.size()) return -1000;
            lc3_lvl_state st = {0, 0u, 0};
            if (!r.fresh) {
                const lc3_mt_dstate s = e->dstate[(size_t)r.channel];
                st.last = s.last, st.env = s.env, st.hang = s.hang;
            }
            uint64_t base = r.pcm_off, dst = r.flag_off;
            int32_t before = st.last;
            for (int t = 0; t < r.n_frames; t++) {
                // where the lane body will go, looked at before it goes there
                const uint64_t far = (uint64_t)(r.nf - 1) * (uint64_t)r.stride;
                if (base >= pcm_elems || far >= pcm_elems - base) return -1000;
                if ((active && dst >= n_active) || (levels && dst >= n_levels)) return -1000;
                lc3_lvl_partial lanes[LC3_MT_WAVE];
                for (int lane = 0; lane < LC3_MT_WAVE; lane++) lanes[lane] = lc3_lvl_lane(pcm, base, r.stride, r.nf, lane, before);
                const int32_t last = lc3_lvl_last(pcm, r, base);
                lc3_lvl_partial p = lc3_lvl_empty();
                for (int lane = LC3_MT_WAVE - 1; lane >= 0; lane--) p = lc3_lvl_combine(p, lanes[lane]);
                uint32_t w[8];
                lc3_lvl_finish(p, r, last, st, w);
                if (levels) memcpy(levels + dst * LC3_MT_RECORD_BYTES, w, LC3_MT_RECORD_BYTES);
                if (active) active[dst] = (uint8_t)((w[6] >> 16) & 1u);
                before = last;
                base += (uint64_t)(uint32_t)r.pitch;
                dst += (uint64_t)(uint32_t)r.flag_pitch;
            }
            lc3_mt_dstate s = {st.last, st.env, st.hang, 0};
            e->dstate[(size_t)r.channel] = s;
        }
    return 0;
}
}
