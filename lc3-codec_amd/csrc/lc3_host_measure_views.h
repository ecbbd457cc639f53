// PCM levels over a list of views (lc3gpu_measure_mixed_views, include/lc3gpu.h): the channel table, the host check, the row builder and the
// channels' state book-keeping.  Pure C++ with no HIP call and no device header, shared by the companion library (lc3gpu_meter.hip) and by
// the CPU tests (tests/emu/lc3_emu_meter_views.cpp, tests/emu/lc3_meter_views_check_main.cpp): what the tests drive is the code the library
// runs.  lc3_host_inspect_views.h is included unchanged for the view itself (lc3_iview), the stream constants (lc3_iv_config), the
// non-wrapping extent test (lc3_iv_inside) and the range test (lc3_iv_ranges_overlap).
//
// The call's views carry caller-given offsets: the check (lc3_mviews_check) is the only thing between a typo and a stray access on the
// device.  It runs before the rows are built, in unsigned 64-bit arithmetic that cannot wrap, and a refused call builds, uploads and
// launches nothing and changes no channel's state.
//
// The plan.  One ROW per view, in the caller's order: the placement with the pitches resolved, the frame length, the channel's coefficients
// and whether the channel starts fresh.  O(views) bytes whatever the frame counts are.  One WAVE owns one row (four rows a workgroup), so a
// wave finds its row by its own number: no bisection is needed.
//
// The state.  One 16-byte record per channel on the device (last, env, hang).  A channel may be named once per call, one wave owns one view,
// so only that wave reads and writes that channel's record in a launch: ONE buffer per channel is enough, no double buffer.  A pending reset
// is no device work at all: the row says "start fresh".
#pragma once
#include "lc3_host_inspect_views.h"

#define LC3_MT_WAVE 64
#define LC3_MT_WAVES_PER_WG 4
#define LC3_MT_LANES (LC3_MT_WAVE * LC3_MT_WAVES_PER_WG)
#define LC3_MT_STATE_BYTES 16
#define LC3_MT_RECORD_BYTES 32
#define LC3_MT_MAX_Q15 32768
#define LC3_MT_MAX_THRESHOLD ((uint32_t)1 << 30)
#define LC3_MT_MAX_HANG 65535

// device rows (64 bytes each)
struct lc3_mt_row {
    uint64_t pcm_off, flag_off;  // sample 0 of frame 0 in d_pcm; frame 0's index in d_active / d_levels
    int pitch, flag_pitch;       // resolved (never 0)
    int stride, nf;
    int n_frames, channel;
    int attack, release;         // Q15, 0 .. 32768
    uint32_t threshold;
    int hang_frames;
    int fresh;                   // 1: the channel starts from last = 0, env = 0, hang = 0 instead of its record
    int reserved;
};
static_assert(sizeof(lc3_mt_row) == 64, "rows are 64 bytes");
// a channel's record on the device
struct lc3_mt_dstate {
    int32_t last;   // the last sample of the last frame measured
    uint32_t env;   // 0 .. 2^30
    int32_t hang;   // 0 .. hang_frames
    int32_t reserved;
};
static_assert(sizeof(lc3_mt_dstate) == LC3_MT_STATE_BYTES, "a state is 16 bytes");

// ---- host only -------------------------------------------------------------------------------------------------------------------------------
// frame length of a stream (common/config.rs:42-100)
static inline int lc3_mt_nf(int frame_us, int fs_hz) {
    const int nf10 = fs_hz == 44100 ? 480 : fs_hz / 100;
    return frame_us == 10000 ? nf10 : nf10 * 3 / 4;
}

// one channel of the meter: what its rows are made of (fixed at creation) and its state's book-keeping
struct lc3_mt_channel {
    int nf;
    int attack, release;
    uint32_t threshold;
    int hang_frames;
    int fresh;  // 1: the next listed call starts from zeros (at creation, and after a reset)
    int seen;   // the number of the last check that named the channel (the named-twice rule)
};
// the descriptor's six fields -> the channel; LC3_IV_EINVAL for anything outside their sets
static inline int lc3_mt_make_channel(int fs_hz, int frame_us, int32_t attack_q15, int32_t release_q15, uint32_t threshold, int32_t hang_frames,
                                      lc3_mt_channel &c) {
    lc3_iv_stream s;
    if (lc3_iv_config(frame_us, fs_hz, s)) return LC3_IV_EINVAL;
    if (attack_q15 < 0 || attack_q15 > LC3_MT_MAX_Q15 || release_q15 < 0 || release_q15 > LC3_MT_MAX_Q15) return LC3_IV_EINVAL;
    if (threshold > LC3_MT_MAX_THRESHOLD) return LC3_IV_EINVAL;
    if (hang_frames < 0 || hang_frames > LC3_MT_MAX_HANG) return LC3_IV_EINVAL;
    c.nf = lc3_mt_nf(frame_us, fs_hz);
    c.attack = attack_q15;
    c.release = release_q15;
    c.threshold = threshold;
    c.hang_frames = hang_frames;
    c.fresh = 1;
    c.seen = 0;
    return LC3_IV_OK;
}

// the caller's arrays: base ADDRESSES (for the alignment and overlap checks: nothing is read) and extents in samples, bytes and records; an
// output that is not given has use_* == 0 and is checked against nothing
struct lc3_mt_bounds {
    uint64_t pcm_base, pcm_elems;
    uint64_t active_base, n_active;
    uint64_t levels_base, n_levels;
    int use_active, use_levels;
};
// the meter's host state: its channels and the numbering of its checks
struct lc3_mt_state {
    std::vector<lc3_mt_channel> channels;
    int checks = 0;
};

// Every check of the call but `mt` itself.  Changes nothing of the state but the numbering of the checks (St.checks and the channels'
// `seen`), which no result depends on.
static inline int lc3_mviews_check(lc3_mt_state &St, int max_views, const lc3_iview *views, int n_views, const lc3_mt_bounds &B) {
    if (n_views < 0) return LC3_IV_EINVAL;
    if (n_views == 0) return LC3_IV_OK;
    if (!views || B.pcm_base == 0) return LC3_IV_EINVAL;
    if (!B.use_active && !B.use_levels) return LC3_IV_EINVAL;
    if (B.use_levels && (B.levels_base & 15u) != 0) return LC3_IV_EINVAL;
    const uint64_t pcm_len = B.pcm_elems > UINT64_MAX / 2 ? UINT64_MAX : B.pcm_elems * 2;
    const uint64_t levels_len = B.n_levels > UINT64_MAX / LC3_MT_RECORD_BYTES ? UINT64_MAX : B.n_levels * LC3_MT_RECORD_BYTES;
    if (B.use_active && lc3_iv_ranges_overlap(B.active_base, B.n_active, B.pcm_base, pcm_len)) return LC3_IV_EINVAL;
    if (B.use_levels && lc3_iv_ranges_overlap(B.levels_base, levels_len, B.pcm_base, pcm_len)) return LC3_IV_EINVAL;
    if (B.use_active && B.use_levels && lc3_iv_ranges_overlap(B.active_base, B.n_active, B.levels_base, levels_len)) return LC3_IV_EINVAL;
    if (n_views > max_views) return LC3_IV_ELENGTH;
    if (St.checks == INT32_MAX) {  // (the numbering starts over: once in 2^31 calls)
        for (lc3_mt_channel &c : St.channels) c.seen = 0;
        St.checks = 0;
    }
    const int mark = ++St.checks;
    const int n_channels = (int)St.channels.size();
    for (int i = 0; i < n_views; i++) {
        const lc3_iview &v = views[i];
        if (v.channel < 0 || v.channel >= n_channels) return LC3_IV_ECHANNEL;
        if (v.n_frames < 1) return LC3_IV_ELENGTH;
        lc3_mt_channel &c = St.channels[(size_t)v.channel];
        const int nf = c.nf;
        if (v.reserved[0] != 0 || v.reserved[1] != 0 || v.reserved[2] != 0) return LC3_IV_EINVAL;
        if (v.pcm_stride < 1 || v.pcm_stride > 8) return LC3_IV_EINVAL;
        if (v.pcm_off < 0 || v.flag_off < 0) return LC3_IV_EINVAL;
        if (v.pcm_pitch != 0 && v.pcm_pitch < nf * v.pcm_stride) return LC3_IV_EINVAL;
        if (v.flag_pitch < 0) return LC3_IV_EINVAL;
        const int pitch = v.pcm_pitch ? v.pcm_pitch : nf * v.pcm_stride, fp = v.flag_pitch ? v.flag_pitch : 1;
        if (v.pcm_stride == 1) {
            if ((v.pcm_off & 1) != 0 || (pitch & 1) != 0 || (B.pcm_base & 3u) != 0) return LC3_IV_EINVAL;
        } else if ((B.pcm_base & 1u) != 0) {
            return LC3_IV_EINVAL;
        }
        const uint64_t samples = (uint64_t)v.n_frames * (uint64_t)nf;
        if (samples > (uint64_t)0x7fffffff) return LC3_IV_ELENGTH;
        if (!lc3_iv_inside(v.pcm_off, v.n_frames, pitch, (uint64_t)(nf - 1) * (uint64_t)v.pcm_stride, B.pcm_elems)) return LC3_IV_ELENGTH;
        if (B.use_active && !lc3_iv_inside(v.flag_off, v.n_frames, fp, 0, B.n_active)) return LC3_IV_ELENGTH;
        if (B.use_levels && !lc3_iv_inside(v.flag_off, v.n_frames, fp, 0, B.n_levels)) return LC3_IV_ELENGTH;
        if (c.seen == mark) return LC3_IV_ECHANNEL;  // named twice
        c.seen = mark;
    }
    return LC3_IV_OK;
}

// Views already checked, n_views >= 1.  rows: n_views of them.  ADVANCES THE STATE: every listed channel's pending reset is consumed; the
// caller launches what the rows say (or, where it cannot, calls lc3_mviews_unbuild with the same list).
static inline void lc3_mviews_build(lc3_mt_state &St, const lc3_iview *views, int n_views, lc3_mt_row *rows) {
    for (int i = 0; i < n_views; i++) {
        const lc3_iview &v = views[i];
        lc3_mt_channel &c = St.channels[(size_t)v.channel];
        lc3_mt_row &r = rows[i];
        r.pcm_off = (uint64_t)v.pcm_off;
        r.flag_off = (uint64_t)v.flag_off;
        r.pitch = v.pcm_pitch ? v.pcm_pitch : c.nf * v.pcm_stride;
        r.flag_pitch = v.flag_pitch ? v.flag_pitch : 1;
        r.stride = v.pcm_stride;
        r.nf = c.nf;
        r.n_frames = v.n_frames;
        r.channel = v.channel;
        r.attack = c.attack;
        r.release = c.release;
        r.threshold = c.threshold;
        r.hang_frames = c.hang_frames;
        r.fresh = c.fresh;
        r.reserved = 0;
        c.fresh = 0;
    }
}
// takes back what lc3_mviews_build did to the state (the launch could not be queued): rows are what it filled
static inline void lc3_mviews_unbuild(lc3_mt_state &St, const lc3_iview *views, int n_views, const lc3_mt_row *rows) {
    for (int i = 0; i < n_views; i++) St.channels[(size_t)views[i].channel].fresh = rows[i].fresh;
}
static inline void lc3_mt_reset_channel(lc3_mt_channel &c) { c.fresh = 1; }
