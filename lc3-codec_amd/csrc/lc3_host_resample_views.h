// Rate conversion over two lists of views (lc3gpu_resample_mixed_views, include/lc3gpu.h): the host check, the plan, the channels' state
// book-keeping and the look-up the kernel makes in the plan's rows.  Pure C++ with no HIP call and no device header, shared by the companion
// library (lc3gpu_resampler.hip) and by the CPU tests (tests/emu/lc3_emu_resample_views.cpp, tests/emu/lc3_resample_views_check_main.cpp):
// what the tests drive is the code the library runs.  lc3_host_inspect_views.h is included unchanged for the view itself (lc3_iview), the
// stream constants (lc3_iv_config), the non-wrapping extent test (lc3_iv_inside), the range test (lc3_iv_ranges_overlap) and the form of the
// bisection.
//
// The call's views carry caller-given offsets: the check (lc3_rviews_check) is the only thing between a typo and a stray access on the
// device.  It runs before the plan is built, in unsigned 64-bit arithmetic that cannot wrap, and a refused call builds, uploads and launches
// nothing and changes no channel's state.
//
// The plan.  One ROW per pair of views, in the caller's order: both placements with the pitches resolved, the frame lengths with the
// multipliers that divide by them, the ratio's figures and where the channel's history is read and written: O(views) bytes whatever the
// frame counts are.  Row i owns workgroups [wg0, wg0 + ceil(S_out / LC3_RS_CHUNK)); a workgroup finds its row by bisection over wg0
// (wave-uniform) and owns LC3_RS_CHUNK consecutive output samples of it.  LC3_RS_CHUNK is a multiple of every L, so every chunk starts at
// phase 0 and at input sample chunk * (LC3_RS_CHUNK * M / L) exactly.
//
// The history.  Every chunk of a view may read the channel's history (the T - 1 samples before the view), and exactly one workgroup writes
// the new one.  Every channel therefore has TWO history buffers: a call reads buffer `cur` and writes buffer `cur ^ 1`, and the host flips
// `cur` for every channel a call lists (lc3_rviews_build).  No workgroup of a launch writes what another one of it reads, and a pending
// reset is no device work at all: the row says "read zeros" (hist_rd < 0).
#pragma once
#include "lc3_host_inspect_views.h"

#include "../../tables/lc3_resample_tables.h"

#define LC3_RS_LANES 256
#define LC3_RS_CHUNK 768     // output samples of a view per workgroup: 3 per lane, a multiple of 12 (of every L: 1, 2, 3, 4, 6)
#define LC3_RS_HIST 96       // samples of one history buffer (LC3_RS_MAX_T - 1)
#define LC3_RS_MAX_WINDOW (LC3_RS_CHUNK * 6 + LC3_RS_HIST + 2)  // input samples a workgroup stages, at most (M / L <= 6; + 2: pairs)
#define LC3_RS_MAGIC_SHIFT 36
static_assert(LC3_RS_CHUNK % 12 == 0 && LC3_RS_CHUNK % LC3_RS_LANES == 0 && LC3_RS_HIST == LC3_RS_MAX_T - 1 && LC3_RS_HIST % 2 == 0, "the plan's figures");

// device rows (96 bytes each)
struct lc3_rs_row {
    uint64_t in_off, out_off;      // sample 0 of either view in its array
    uint64_t in_magic, out_magic;  // floor(2^36 / (nf / 4)) + 1: lc3_rs_div(s, magic) == s / nf for every s < 2^31
    int in_pitch, out_pitch;       // resolved (never 0)
    int in_stride, out_stride;
    int nf_in, nf_out;
    int S_in, S_out;               // samples of either view; S_out * M == S_in * L
    int wg0;                       // first workgroup of the row
    int L, M, T;                   // the ratio and its taps per phase (a copy: 1, 1, 1)
    int coef_off;                  // the ratio's table in lc3_rs_coef, or -1: a copy (the one coefficient is 32768)
    int hist_rd, hist_wr;          // the channel's histories, in samples from the start of the history array; hist_rd < 0: zeros
    int inv;                       // floor(2^16 / L) + 1: (u * inv) >> 16 == u / L for every u <= LC3_RS_CHUNK * 6
};
static_assert(sizeof(lc3_rs_row) == 96, "rows are 96 bytes");

// ---- the kernel's look-ups (and the emulator's) ------------------------------------------------------------------------------------------
// the row of workgroup wg: the last one whose wg0 <= wg (rows[0].wg0 == 0)
LC3_IV_HD int lc3_rs_find_row(const lc3_rs_row *rows, int n_rows, int wg) {
    int lo = 0, hi = n_rows;  // invariant: rows[lo].wg0 <= wg, rows[hi].wg0 > wg (hi == n_rows: beyond)
    while (hi - lo > 1) {
        const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
        if (rows[mid].wg0 <= wg) lo = mid;
        else hi = mid;
    }
    return lo;
}
// s / nf without a division.  Every frame length is a multiple of 4, so s / nf == (s >> 2) / (nf / 4).  With q = s >> 2 < 2^29, d = nf / 4
// (15 .. 120) and e = magic * d - 2^36, 1 <= e <= d <= 120 <= 2^(36 - 29): by the round-up theorem of division by invariant integers,
// floor(q * magic / 2^36) == floor(q / d) for every q < 2^29; q * magic stays below 2^29 * (2^36 / 15 + 1) < 2^62.
LC3_IV_HD uint32_t lc3_rs_div(uint32_t s, uint64_t magic) { return (uint32_t)(((uint64_t)(s >> 2) * magic) >> LC3_RS_MAGIC_SHIFT); }
// where sample s of a view lies
LC3_IV_HD uint64_t lc3_rs_place(uint64_t off, uint64_t magic, int nf, int pitch, int stride, uint32_t s) {
    const uint32_t t = lc3_rs_div(s, magic);
    const uint32_t n = s - t * (uint32_t)nf;
    return off + (uint64_t)t * (uint64_t)(uint32_t)pitch + (uint64_t)(n * (uint32_t)stride);  // (n * stride < 480 * 8)
}
// u / L for u <= LC3_RS_CHUNK * 6 = 4608: e = inv * L - 2^16 lies in 1 .. L <= 6, and u * e <= 27648 < 2^16
LC3_IV_HD uint32_t lc3_rs_div_l(uint32_t u, int inv) { return (u * (uint32_t)inv) >> 16; }

// ---- host only -------------------------------------------------------------------------------------------------------------------------------
static inline uint64_t lc3_rs_magic(int nf) { return (((uint64_t)1 << LC3_RS_MAGIC_SHIFT) / (uint64_t)(nf / 4)) + 1u; }
static inline int lc3_rs_gcd(int a, int b) {
    while (b) {
        const int t = a % b;
        a = b;
        b = t;
    }
    return a;
}
// frame length of a stream (common/config.rs:42-100)
static inline int lc3_rs_nf(int frame_us, int fs_hz) {
    const int nf10 = fs_hz == 44100 ? 480 : fs_hz / 100;
    return frame_us == 10000 ? nf10 : nf10 * 3 / 4;
}
enum { LC3_RS_EUNSUPPORTED = -7 };  // = LC3GPU_EUNSUPPORTED

// one channel of the resampler: what its rows are made of (fixed at creation) and its state's book-keeping
struct lc3_rs_channel {
    int nf_in, nf_out;
    uint64_t in_magic, out_magic;
    int L, M, T, coef_off, inv;
    int cur;      // the history buffer the next listed call reads (0 / 1)
    int fresh;    // 1: the next listed call reads zeros instead (at creation, and after a reset)
    int seen;     // the number of the last check that named the channel (the named-twice rule)
};
// (fs_in_hz, fs_out_hz, frame_us) -> the channel; LC3_IV_EINVAL for an unknown rate or duration, LC3_RS_EUNSUPPORTED for a conversion to or
// from 44.1 kHz
static inline int lc3_rs_make_channel(int fs_in, int fs_out, int frame_us, lc3_rs_channel &c) {
    lc3_iv_stream s;
    if (lc3_iv_config(frame_us, fs_in, s) || lc3_iv_config(frame_us, fs_out, s)) return LC3_IV_EINVAL;
    if (fs_in != fs_out && (fs_in == 44100 || fs_out == 44100)) return LC3_RS_EUNSUPPORTED;
    c.nf_in = lc3_rs_nf(frame_us, fs_in);
    c.nf_out = lc3_rs_nf(frame_us, fs_out);
    c.in_magic = lc3_rs_magic(c.nf_in);
    c.out_magic = lc3_rs_magic(c.nf_out);
    const int g = lc3_rs_gcd(fs_in, fs_out);
    c.L = fs_out / g;
    c.M = fs_in / g;
    c.T = 1;
    c.coef_off = -1;
    if (fs_in != fs_out) {
        int k = -1;
        for (int i = 0; i < LC3_RS_RATIOS; i++)
            if (lc3_rs_ratios[i].L == c.L && lc3_rs_ratios[i].M == c.M) k = i;
        if (k < 0) return LC3_RS_EUNSUPPORTED;  // (cannot happen among the five rates)
        c.T = lc3_rs_ratios[k].T;
        c.coef_off = lc3_rs_ratios[k].off;
    }
    c.inv = 65536 / c.L + 1;
    c.cur = 0;
    c.fresh = 1;
    c.seen = 0;
    return LC3_IV_OK;
}

// the caller's two arrays: base ADDRESSES (for the alignment and overlap checks: nothing is read) and extents in elements
struct lc3_rs_bounds {
    uint64_t in_base, in_elems;
    uint64_t out_base, out_elems;
};
// the resampler's host state: its channels and the numbering of its checks
struct lc3_rs_state {
    std::vector<lc3_rs_channel> channels;
    int checks = 0;
    int n_wg = 0;  // of the last plan
};

// one view against its array
static inline int lc3_rs_check_view(const lc3_iview &v, int nf, uint64_t base, uint64_t elems) {
    if (v.reserved[0] != 0 || v.reserved[1] != 0 || v.reserved[2] != 0) return LC3_IV_EINVAL;
    if (v.pcm_stride < 1 || v.pcm_stride > 8) return LC3_IV_EINVAL;
    if (v.pcm_off < 0) return LC3_IV_EINVAL;
    if (v.pcm_pitch != 0 && v.pcm_pitch < nf * v.pcm_stride) return LC3_IV_EINVAL;
    const int pitch = v.pcm_pitch ? v.pcm_pitch : nf * v.pcm_stride;
    if (v.pcm_stride == 1) {
        if ((v.pcm_off & 1) != 0 || (pitch & 1) != 0 || (base & 3u) != 0) return LC3_IV_EINVAL;
    } else if ((base & 1u) != 0) {
        return LC3_IV_EINVAL;
    }
    const uint64_t samples = (uint64_t)v.n_frames * (uint64_t)nf;
    if (samples > (uint64_t)0x7fffffff) return LC3_IV_ELENGTH;  // (sample numbers are 32-bit on the device)
    if (!lc3_iv_inside(v.pcm_off, v.n_frames, pitch, (uint64_t)(nf - 1) * (uint64_t)v.pcm_stride, elems)) return LC3_IV_ELENGTH;
    return LC3_IV_OK;
}

// Every check of the call but `rs` itself.  Changes nothing of the state but the numbering of the checks (St.checks and the channels'
// `seen`), which no result depends on.
static inline int lc3_rviews_check(lc3_rs_state &St, int max_views, const lc3_iview *in_views, const lc3_iview *out_views, int n_views,
                                   const lc3_rs_bounds &B) {
    if (n_views < 0) return LC3_IV_EINVAL;
    if (n_views == 0) return LC3_IV_OK;
    if (!in_views || !out_views || B.in_base == 0 || B.out_base == 0) return LC3_IV_EINVAL;
    const uint64_t in_len = B.in_elems > UINT64_MAX / 2 ? UINT64_MAX : B.in_elems * 2;
    const uint64_t out_len = B.out_elems > UINT64_MAX / 2 ? UINT64_MAX : B.out_elems * 2;
    if (lc3_iv_ranges_overlap(B.in_base, in_len, B.out_base, out_len)) return LC3_IV_EINVAL;
    if (n_views > max_views) return LC3_IV_ELENGTH;
    if (St.checks == INT32_MAX) {  // (the numbering starts over: once in 2^31 calls)
        for (lc3_rs_channel &c : St.channels) c.seen = 0;
        St.checks = 0;
    }
    const int mark = ++St.checks;
    const int n_channels = (int)St.channels.size();
    uint64_t wgs = 0;
    for (int i = 0; i < n_views; i++) {
        const lc3_iview &a = in_views[i], &b = out_views[i];
        if (a.channel < 0 || a.channel >= n_channels || b.channel < 0 || b.channel >= n_channels) return LC3_IV_ECHANNEL;
        if (a.n_frames < 1 || b.n_frames < 1) return LC3_IV_ELENGTH;
        if (a.channel != b.channel || a.n_frames != b.n_frames) return LC3_IV_EINVAL;
        lc3_rs_channel &c = St.channels[(size_t)a.channel];
        int rc = lc3_rs_check_view(a, c.nf_in, B.in_base, B.in_elems);
        if (!rc) rc = lc3_rs_check_view(b, c.nf_out, B.out_base, B.out_elems);
        if (rc) return rc;
        if (c.seen == mark) return LC3_IV_ECHANNEL;  // named twice
        c.seen = mark;
        wgs += ((uint64_t)b.n_frames * (uint64_t)c.nf_out + LC3_RS_CHUNK - 1) / LC3_RS_CHUNK;
    }
    if (wgs > (uint64_t)0x7fffffff) return LC3_IV_ELENGTH;  // (workgroup numbers are 32-bit)
    return LC3_IV_OK;
}

// Views already checked, n_views >= 1.  rows: n_views of them.  ADVANCES THE STATE: every listed channel's buffers are flipped and its
// pending reset is consumed; the caller launches what the rows say (or, where it cannot, calls lc3_rviews_unbuild with the same lists).
static inline void lc3_rviews_build(lc3_rs_state &St, const lc3_iview *in_views, const lc3_iview *out_views, int n_views, lc3_rs_row *rows) {
    int wg = 0;
    for (int i = 0; i < n_views; i++) {
        const lc3_iview &a = in_views[i], &b = out_views[i];
        lc3_rs_channel &c = St.channels[(size_t)a.channel];
        lc3_rs_row &r = rows[i];
        r.in_off = (uint64_t)a.pcm_off;
        r.out_off = (uint64_t)b.pcm_off;
        r.in_magic = c.in_magic;
        r.out_magic = c.out_magic;
        r.in_pitch = a.pcm_pitch ? a.pcm_pitch : c.nf_in * a.pcm_stride;
        r.out_pitch = b.pcm_pitch ? b.pcm_pitch : c.nf_out * b.pcm_stride;
        r.in_stride = a.pcm_stride;
        r.out_stride = b.pcm_stride;
        r.nf_in = c.nf_in;
        r.nf_out = c.nf_out;
        r.S_in = a.n_frames * c.nf_in;
        r.S_out = b.n_frames * c.nf_out;
        r.wg0 = wg;
        r.L = c.L, r.M = c.M, r.T = c.T;
        r.coef_off = c.coef_off;
        const int base = a.channel * 2 * LC3_RS_HIST;
        r.hist_rd = c.fresh ? -1 : base + c.cur * LC3_RS_HIST;
        r.hist_wr = base + (c.cur ^ 1) * LC3_RS_HIST;
        r.inv = c.inv;
        wg += (int)(((unsigned)r.S_out + (unsigned)LC3_RS_CHUNK - 1u) / (unsigned)LC3_RS_CHUNK);
        if (c.T > 1) {  // (a copy has no state)
            c.cur ^= 1;
            c.fresh = 0;
        }
    }
    St.n_wg = wg;
}
// takes back what lc3_rviews_build did to the state (the launch could not be queued): rows are what it filled
static inline void lc3_rviews_unbuild(lc3_rs_state &St, const lc3_iview *in_views, int n_views, const lc3_rs_row *rows) {
    for (int i = 0; i < n_views; i++) {
        lc3_rs_channel &c = St.channels[(size_t)in_views[i].channel];
        if (c.T > 1) {
            c.cur ^= 1;
            c.fresh = rows[i].hist_rd < 0;
        }
    }
}
static inline void lc3_rs_reset_channel(lc3_rs_channel &c) { c.fresh = 1; }
