// Frame inspection over a list of views (lc3gpu_inspect_mixed_views, include/lc3gpu.h): the host check, the plan and the two look-ups
// the kernel makes in the plan's tables.  Pure C++ with no HIP call and no device header, shared by the companion library
// (lc3gpu_inspector.hip) and by the CPU tests (tests/emu/lc3_emu_inspect_views.cpp, tests/emu/lc3_inspect_views_check_main.cpp), the way
// lc3_host_mixed_list.h is shared: what the tests drive is the code the library runs.
//
// The call has no handle to lean on, and its views carry caller-given offsets: the extent check (lc3_iviews_check) is the only thing
// between a typo and a stray access on the device.  It runs before the plan is built, in unsigned 64-bit arithmetic that cannot wrap, and
// a refused call builds, uploads and launches nothing.
//
// The plan.  A frame's lane body (lc3_inspect_record) takes the configuration's ne / fs_ind / n_ms_10 and the frame size as plain integers,
// and a workgroup's LDS slots have one pitch; so a workgroup is kept UNIFORM in (configuration, effective nbytes) by planning:
//   - the views are counting-sorted by that key into BUCKETS (at most one per view, at most 12 * 400);
//   - the frames of the sorted order are numbered consecutively; consecutive frames go to consecutive lanes;
//   - workgroups are cut at bucket borders: bucket b owns workgroups [wg0, wg0 + ceil(n_frames / fpb)), the last one partly filled.
// What is uploaded is one ROW per view (its frames' places with the pitches resolved -- the kernel holds no `0 = default` test -- and the
// number of its first frame) and one row per bucket: O(views) bytes whatever the frame counts are, which is what lets max_views size the
// pinned ring and the device tables once.  No per-frame and no per-workgroup table exists: a workgroup finds its bucket by bisection over
// the buckets' wg0 (wave-uniform), a lane its view by bisection over the bucket's rows' frame0.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef LC3_IV_HD  // (the HIP unit: __host__ __device__)
#define LC3_IV_HD static inline
#endif

#define LC3_IV_MAX_NBYTES 400
#define LC3_IV_CONFIGS 12
#define LC3_IV_RECORD_BYTES 128
// what lc3_iviews_check returns: the values of LC3GPU_OK / LC3GPU_EINVAL / LC3GPU_ECHANNEL / LC3GPU_ELENGTH (include/lc3gpu.h)
enum { LC3_IV_OK = 0, LC3_IV_EINVAL = -1, LC3_IV_ECHANNEL = -2, LC3_IV_ELENGTH = -3 };

struct lc3_iview {  // = lc3gpu_view (include/lc3gpu.h)
    int32_t channel, n_frames, nbytes, pcm_stride;
    int64_t pcm_off, byte_off, flag_off;
    int32_t pcm_pitch, byte_pitch, flag_pitch;
    int32_t reserved[3];
};
static_assert(sizeof(lc3_iview) == 64, "lc3_iview is lc3gpu_view");
// one stream of the inspector: what the lane body needs of its configuration, the configuration's number (0 .. 11: rate index * 2 +
// (10 ms)) and the descriptor's frame size
struct lc3_iv_stream {
    int ne, fs_ind, n_ms_10, cfg, nbytes;
};
// device rows (32 bytes each)
struct lc3_iv_row {
    uint64_t byte_off, flag_off;   // frame 0 of the view in d_in, and in d_bad_frame / d_status / d_info
    int byte_pitch, flag_pitch;    // resolved (never 0)
    int frame0, n_frames;          // the view's frames are frames frame0 .. frame0 + n_frames - 1 of the sorted order
};
struct lc3_iv_bucket {
    int wg0;               // first workgroup of the bucket
    int frame0, n_frames;  // its frames in the sorted order
    int view0, n_views;    // its rows
    int nbytes, ne;        // frame size and number of coded lines
    int fs_ind_ms;         // fs_ind | n_ms_10 << 8
};
static_assert(sizeof(lc3_iv_row) == 32 && sizeof(lc3_iv_bucket) == 32, "rows are 32 bytes");

// ---- the kernel's look-ups (and the emulator's) ------------------------------------------------------------------------------------------
// the bucket of workgroup wg: the last one whose wg0 <= wg (buckets[0].wg0 == 0)
LC3_IV_HD int lc3_iv_find_bucket(const lc3_iv_bucket *buckets, int n_buckets, int wg) {
    int lo = 0, hi = n_buckets;  // invariant: buckets[lo].wg0 <= wg, buckets[hi].wg0 > wg (hi == n_buckets: beyond)
    while (hi - lo > 1) {
        const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
        if (buckets[mid].wg0 <= wg) lo = mid;
        else hi = mid;
    }
    return lo;
}
// frames of workgroup wg of bucket b (1 .. fpb)
LC3_IV_HD int lc3_iv_wg_frames(const lc3_iv_bucket &b, int wg, int fpb) {
    const int left = b.n_frames - (wg - b.wg0) * fpb;  // (wg - wg0) * fpb < n_frames <= 2^31 - 1
    return left < fpb ? left : fpb;
}
// the row of frame f of the sorted order among rows [v0, v0 + nv): the last one whose frame0 <= f (rows[v0].frame0 <= f)
LC3_IV_HD int lc3_iv_find_view(const lc3_iv_row *rows, int v0, int nv, int f) {
    int lo = v0, hi = v0 + nv;
    while (hi - lo > 1) {
        const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
        if (rows[mid].frame0 <= f) lo = mid;
        else hi = mid;
    }
    return lo;
}
// lane `tid` (< lc3_iv_wg_frames) of workgroup wg of bucket b: where its frame's bytes start and the index of its flag and outputs.
// Unsigned: an offset may lie anywhere below 2^63 and a view may span up to 2^62 more; the check has seen to it that both stay inside the
// caller's extents
LC3_IV_HD void lc3_iv_lane_place(const lc3_iv_row *rows, const lc3_iv_bucket &b, int wg, int tid, int fpb, uint64_t &src, uint64_t &dst) {
    const int f = b.frame0 + (wg - b.wg0) * fpb + tid;
    const lc3_iv_row &r = rows[lc3_iv_find_view(rows, b.view0, b.n_views, f)];
    const uint64_t t = (uint64_t)(f - r.frame0);
    src = r.byte_off + t * (uint64_t)r.byte_pitch;
    dst = r.flag_off + t * (uint64_t)r.flag_pitch;
}

// Frames per workgroup and dynamic LDS: the rule of the main library's lane-per-frame kernels (256 lanes, halved down to 64 while the fixed
// part, the frames' part and 8 bytes of slack pass 64 KB), for the call's largest frame size.  Fixed part: the parser's lookup (4096), the
// spectral model (64 rows of 20 words) and the TNS models (152 words); per frame: its record (128), the index of its outputs (8), the
// lsb-mode flags (14 words) and its bytes.  (lc3gpu_inspector.hip asserts the figures against the device headers.)
#define LC3_IV_LDS_FIXED 9824
#define LC3_IV_LDS_PER_FRAME 192
LC3_IV_HD unsigned lc3_iv_fpb(int max_nbytes) {
    unsigned fpb = 256u;
    while (fpb > 64u && LC3_IV_LDS_FIXED + (size_t)fpb * (size_t)(LC3_IV_LDS_PER_FRAME + max_nbytes) + 8 > 65536u) fpb >>= 1;
    return fpb;
}
LC3_IV_HD size_t lc3_iv_lds_bytes(int max_nbytes) {
    return LC3_IV_LDS_FIXED + (size_t)lc3_iv_fpb(max_nbytes) * (size_t)(LC3_IV_LDS_PER_FRAME + max_nbytes) + 8;
}

// ---- host only -----------------------------------------------------------------------------------------------------------------------------
#include <algorithm>
#include <vector>

static inline int lc3_iv_rate(int k) {  // k = 0 .. 5
    static const int fs_tab[6] = {8000, 16000, 24000, 32000, 44100, 48000};
    return fs_tab[k];
}
// (frame_us, fs_hz) -> the stream's constants (common/config.rs:42-100); -1 for an unknown configuration
static inline int lc3_iv_config(int frame_us, int fs_hz, lc3_iv_stream &s) {
    static const int ind_tab[6] = {0, 1, 2, 3, 4, 4};
    static const int nf10[6] = {80, 160, 240, 320, 480, 480};
    int k = -1;
    for (int i = 0; i < 6; i++)
        if (lc3_iv_rate(i) == fs_hz) k = i;
    if (k < 0 || (frame_us != 7500 && frame_us != 10000)) return -1;
    s.n_ms_10 = frame_us == 10000;
    s.fs_ind = ind_tab[k];
    const int nf = s.n_ms_10 ? nf10[k] : nf10[k] * 3 / 4, cap = s.n_ms_10 ? 400 : 300;
    s.ne = nf < cap ? nf : cap;
    s.cfg = k * 2 + s.n_ms_10;
    return 0;
}

// the caller's arrays: base ADDRESSES (for the alignment and overlap checks: nothing is read) and extents in bytes, flags, status bytes
// and records; an array that is not given has base 0 and is checked against nothing
struct lc3_iv_bounds {
    uint64_t in_base, in_bytes;
    uint64_t flags_base, n_flags;
    uint64_t status_base, n_status;
    uint64_t info_base, n_info;
    int use_flags, use_status, use_info;
};
// do [a, a + la) and [b, b + lb) share an address?  No sum is formed: a range may end at 2^64
static inline bool lc3_iv_ranges_overlap(uint64_t a, uint64_t la, uint64_t b, uint64_t lb) {
    if (la == 0 || lb == 0) return false;
    return a <= b ? b - a < la : a - b < lb;
}
// [off, off + (T - 1) * pitch + last] inside [0, size): T < 2^31 and pitch < 2^31, so the span stays below 2^62 + 2^31 and no step wraps
static inline bool lc3_iv_inside(int64_t off, int T, int pitch, uint64_t last, uint64_t size) {
    if ((uint64_t)off >= size) return false;  // (off >= 0: checked by the caller)
    const uint64_t span = (uint64_t)(T - 1) * (uint64_t)pitch + last;
    return span < size - (uint64_t)off;
}
// the checks of the arrays themselves (everything of the table in include/lc3gpu.h that does not look at a view)
static inline int lc3_iviews_check_arrays(const lc3_iv_bounds &B) {
    if (B.in_base == 0) return LC3_IV_EINVAL;
    if (!B.use_status && !B.use_info) return LC3_IV_EINVAL;
    if (B.use_info && (B.info_base & 3u) != 0) return LC3_IV_EINVAL;
    const uint64_t info_len = B.n_info > UINT64_MAX / LC3_IV_RECORD_BYTES ? UINT64_MAX : B.n_info * LC3_IV_RECORD_BYTES;
    if (B.use_status) {
        if (lc3_iv_ranges_overlap(B.status_base, B.n_status, B.in_base, B.in_bytes)) return LC3_IV_EINVAL;
        if (B.use_flags && lc3_iv_ranges_overlap(B.status_base, B.n_status, B.flags_base, B.n_flags)) return LC3_IV_EINVAL;
        if (B.use_info && lc3_iv_ranges_overlap(B.status_base, B.n_status, B.info_base, info_len)) return LC3_IV_EINVAL;
    }
    if (B.use_info) {
        if (lc3_iv_ranges_overlap(B.info_base, info_len, B.in_base, B.in_bytes)) return LC3_IV_EINVAL;
        if (B.use_flags && lc3_iv_ranges_overlap(B.info_base, info_len, B.flags_base, B.n_flags)) return LC3_IV_EINVAL;
    }
    return LC3_IV_OK;
}
// Every check of the call but `insp` itself.  views may be null only to be refused.  frames / max_nbytes: the call's total and its largest
// effective frame size.  Nothing is written but those two.
static inline int lc3_iviews_check(const lc3_iv_stream *streams, int n_streams, int max_views, const lc3_iview *views, int n_views,
                                   const lc3_iv_bounds &B, int *frames, int *max_nbytes) {
    *frames = 0;
    *max_nbytes = 0;
    if (!views || n_views < 0) return LC3_IV_EINVAL;
    const int rc = lc3_iviews_check_arrays(B);
    if (rc) return rc;
    if (n_views > max_views) return LC3_IV_ELENGTH;
    uint64_t total = 0;
    int most = 0;
    for (int i = 0; i < n_views; i++) {
        const lc3_iview &v = views[i];
        if (v.channel < 0 || v.channel >= n_streams) return LC3_IV_ECHANNEL;
        if (v.n_frames < 1) return LC3_IV_ELENGTH;
        if (v.nbytes != 0 && (v.nbytes < 1 || v.nbytes > LC3_IV_MAX_NBYTES)) return LC3_IV_ELENGTH;
        if (v.reserved[0] != 0 || v.reserved[1] != 0 || v.reserved[2] != 0) return LC3_IV_EINVAL;
        if (v.byte_off < 0 || v.flag_off < 0) return LC3_IV_EINVAL;
        const int nb = v.nbytes ? v.nbytes : streams[v.channel].nbytes;
        if (v.byte_pitch != 0 && v.byte_pitch < nb) return LC3_IV_EINVAL;
        if (v.flag_pitch < 0) return LC3_IV_EINVAL;
        const int bp = v.byte_pitch ? v.byte_pitch : nb, fp = v.flag_pitch ? v.flag_pitch : 1;
        if (!lc3_iv_inside(v.byte_off, v.n_frames, bp, (uint64_t)(nb - 1), B.in_bytes)) return LC3_IV_ELENGTH;
        if (B.use_flags && !lc3_iv_inside(v.flag_off, v.n_frames, fp, 0, B.n_flags)) return LC3_IV_ELENGTH;
        if (B.use_status && !lc3_iv_inside(v.flag_off, v.n_frames, fp, 0, B.n_status)) return LC3_IV_ELENGTH;
        if (B.use_info && !lc3_iv_inside(v.flag_off, v.n_frames, fp, 0, B.n_info)) return LC3_IV_ELENGTH;
        total += (uint64_t)v.n_frames;
        if (total > (uint64_t)0x7fffffff) return LC3_IV_ELENGTH;  // (frame numbers are 32-bit on the device)
        if (nb > most) most = nb;
    }
    *frames = (int)total;
    *max_nbytes = most;
    return LC3_IV_OK;
}

// The plan of one call: scratch that lives with the inspector (nothing is allocated in the steady state) and what the launch needs
struct lc3_iv_plan {
    std::vector<int> key_views, key_frames;  // per key (cfg * 400 + nb - 1): views and frames of this call; all zero between calls
    std::vector<int> keys;                   // the keys this call uses, ascending
    int n_buckets = 0, n_wg = 0, fpb = 0;
    lc3_iv_plan() : key_views(LC3_IV_CONFIGS * LC3_IV_MAX_NBYTES, 0), key_frames(LC3_IV_CONFIGS * LC3_IV_MAX_NBYTES, 0) {}
};
// views: already checked (lc3_iviews_check), n_views >= 1.  rows: n_views of them, buckets: room for min(n_views, 12 * 400).  fpb: frames per
// workgroup (lc3_iv_fpb of the call's largest frame size).  Views of one bucket keep the caller's order.
static inline void lc3_iviews_build(const lc3_iv_stream *streams, const lc3_iview *views, int n_views, int fpb, lc3_iv_row *rows,
                                    lc3_iv_bucket *buckets, lc3_iv_plan &P) {
    auto key_of = [&](const lc3_iview &v) {
        const lc3_iv_stream &s = streams[v.channel];
        return s.cfg * LC3_IV_MAX_NBYTES + (v.nbytes ? v.nbytes : s.nbytes) - 1;
    };
    P.keys.clear();
    for (int i = 0; i < n_views; i++) {
        const int k = key_of(views[i]);
        if (P.key_views[(size_t)k]++ == 0) P.keys.push_back(k);
        P.key_frames[(size_t)k] += views[i].n_frames;  // (the call's total is below 2^31)
    }
    std::sort(P.keys.begin(), P.keys.end());
    P.n_buckets = (int)P.keys.size();
    P.fpb = fpb;
    int wg = 0, frame = 0, view = 0;
    for (int b = 0; b < P.n_buckets; b++) {
        const int k = P.keys[(size_t)b];
        lc3_iv_bucket &B = buckets[b];
        B.wg0 = wg;
        B.frame0 = frame;
        B.n_frames = P.key_frames[(size_t)k];
        B.view0 = view;
        B.n_views = P.key_views[(size_t)k];
        B.nbytes = k % LC3_IV_MAX_NBYTES + 1;
        lc3_iv_stream c;
        (void)lc3_iv_config((k / LC3_IV_MAX_NBYTES) & 1 ? 10000 : 7500, lc3_iv_rate((k / LC3_IV_MAX_NBYTES) >> 1), c);
        B.ne = c.ne;
        B.fs_ind_ms = c.fs_ind | (c.n_ms_10 << 8);
        wg += (int)(((unsigned)B.n_frames + (unsigned)fpb - 1u) / (unsigned)fpb);
        frame += B.n_frames;
        view += B.n_views;
        // from here on the key's counters are the bucket's cursors: the next free row and the number of that row's first frame
        P.key_views[(size_t)k] = B.view0;
        P.key_frames[(size_t)k] = B.frame0;
    }
    P.n_wg = wg;
    for (int i = 0; i < n_views; i++) {
        const lc3_iview &v = views[i];
        const lc3_iv_stream &s = streams[v.channel];
        const int k = key_of(v), nb = v.nbytes ? v.nbytes : s.nbytes;
        lc3_iv_row &r = rows[P.key_views[(size_t)k]++];
        r.byte_off = (uint64_t)v.byte_off;
        r.flag_off = (uint64_t)v.flag_off;
        r.byte_pitch = v.byte_pitch ? v.byte_pitch : nb;
        r.flag_pitch = v.flag_pitch ? v.flag_pitch : 1;
        r.frame0 = P.key_frames[(size_t)k];
        r.n_frames = v.n_frames;
        P.key_frames[(size_t)k] += v.n_frames;
    }
    for (int b = 0; b < P.n_buckets; b++) {
        const int k = P.keys[(size_t)b];
        P.key_views[(size_t)k] = 0;
        P.key_frames[(size_t)k] = 0;
    }
}
