// Room mixes over two lists of views (lc3gpu_mix_mixed_views, include/lc3gpu.h): the host check, the plan and the look-up the kernel makes
// in the plan's tables.  Pure C++ with no HIP call and no device header, shared by the companion library (lc3gpu_mixer.hip) and by the CPU
// tests (tests/emu/lc3_emu_mix_views.cpp, tests/emu/lc3_mix_views_check_main.cpp): what the tests drive is the code the library runs.
// lc3_host_inspect_views.h is included unchanged for the view itself (lc3_iview), the stream constants (lc3_iv_config), the non-wrapping
// extent test (lc3_iv_inside), the range test (lc3_iv_ranges_overlap) and the form of the bisection.
//
// The call has no handle to lean on, and its views carry caller-given offsets: the check (lc3_mviews_check) is the only thing between a typo
// and a stray access on the device.  It runs before the plan is built, in unsigned 64-bit arithmetic that cannot wrap, and a refused call
// builds, uploads and launches nothing.
//
// The plan.  Inputs and outputs are counting-sorted by bus; what is uploaded is one ROW per view (its samples' place with the pitch resolved,
// its frame length with the multiplier that divides by it, and its gain or the position of its minus input within the bus) and one row per
// bus THAT HAS OUTPUTS: O(views) bytes whatever the frame counts are.  Bus b owns workgroups [wg0, wg0 + ceil(S / LC3_MX_SPW)); a workgroup
// finds its bus by bisection over wg0 (wave-uniform) and owns LC3_MX_SPW consecutive samples of it, a lane two of them.  A bus without
// outputs takes no workgroup and no bus row.
#pragma once
#include "lc3_host_inspect_views.h"

#define LC3_MX_LANES 256
#define LC3_MX_SPW (2 * LC3_MX_LANES)  // samples of a bus per workgroup: a lane owns the pair (s, s + 1), s even
#define LC3_MX_MAX_BUS_INPUTS 16384
#define LC3_MX_MAGIC_SHIFT 36

struct lc3_mix_in_t {  // = lc3gpu_mix_in
    int32_t bus, gain_q14;
};
struct lc3_mix_out_t {  // = lc3gpu_mix_out
    int32_t bus, minus;
};
static_assert(sizeof(lc3_mix_in_t) == 8 && sizeof(lc3_mix_out_t) == 8, "the room tables' entries are 8 bytes");

// device rows (32 bytes each)
struct lc3_mx_row {
    uint64_t off;    // sample 0 of the view in its array
    uint64_t magic;  // floor(2^36 / (nf / 4)) + 1: lc3_mx_div(s, magic) == s / nf for every s < 2^31 (lc3_mx_magic)
    int pitch;       // resolved (never 0)
    int stride, nf;
    int aux;         // input row: gain_q14.  output row: position of its minus input among the bus's input rows, or -1
};
struct lc3_mx_bus {
    int first_in, n_in;    // its input rows (n_in may be 0: the outputs are zeros)
    int first_out, n_out;  // its output rows (n_out >= 1)
    int S;                 // samples per view
    int wg0;               // first workgroup of the bus
    int planar;            // 1: every one of its rows has stride 1 (lc3_mix_pair<1>)
    int reserved;
};
static_assert(sizeof(lc3_mx_row) == 32 && sizeof(lc3_mx_bus) == 32, "rows are 32 bytes");

// ---- the kernel's look-up (and the emulator's) ---------------------------------------------------------------------------------------------
// the bus of workgroup wg: the last one whose wg0 <= wg (buses[0].wg0 == 0)
LC3_IV_HD int lc3_mx_find_bus(const lc3_mx_bus *buses, int n_buses, int wg) {
    int lo = 0, hi = n_buses;  // invariant: buses[lo].wg0 <= wg, buses[hi].wg0 > wg (hi == n_buses: beyond)
    while (hi - lo > 1) {
        const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
        if (buses[mid].wg0 <= wg) lo = mid;
        else hi = mid;
    }
    return lo;
}

// s / nf without a division (the kernel does it once per row and pair).  Every frame length is a multiple of 4, so s / nf ==
// (s >> 2) / (nf / 4).  With q = s >> 2 < 2^29, d = nf / 4 (15 .. 120) and e = magic * d - 2^36 = d - (2^36 mod d), 1 <= e <= d <= 120 <=
// 2^(36 - 29): by the round-up theorem of division by invariant integers, floor(q * magic / 2^36) == floor(q / d) for every q < 2^29;
// q * magic stays below 2^29 * (2^36 / 15 + 1) < 2^62.
LC3_IV_HD uint32_t lc3_mx_div(uint32_t s, uint64_t magic) { return (uint32_t)(((uint64_t)(s >> 2) * magic) >> LC3_MX_MAGIC_SHIFT); }

// ---- host only -------------------------------------------------------------------------------------------------------------------------------
static inline uint64_t lc3_mx_magic(int nf) { return (((uint64_t)1 << LC3_MX_MAGIC_SHIFT) / (uint64_t)(nf / 4)) + 1u; }
// frame length of a stream (common/config.rs:42-100): ne is min(nf, 400 or 300), so it is taken from the rate
static inline int lc3_mx_nf(int frame_us, int fs_hz) {
    const int nf10 = fs_hz == 44100 ? 480 : fs_hz / 100;
    return frame_us == 10000 ? nf10 : nf10 * 3 / 4;
}
// one stream of the mixer: its frame length, its rate and the multiplier that divides by the frame length (made once, at creation: a
// 64-bit division per view and call is what the host would otherwise spend most of a large tick's plan on)
struct lc3_mx_stream {
    int nf, fs_hz;
    uint64_t magic;
};
static inline void lc3_mx_make_stream(int frame_us, int fs_hz, lc3_mx_stream &s) {
    s.nf = lc3_mx_nf(frame_us, fs_hz);
    s.fs_hz = fs_hz;
    s.magic = lc3_mx_magic(s.nf);
}

// the caller's two arrays: base ADDRESSES (for the alignment and overlap checks: nothing is read) and extents in elements
struct lc3_mx_bounds {
    uint64_t in_base, in_elems;
    uint64_t out_base, out_elems;
};

// The plan of one call and the scratch of its check: lives with the mixer, sized once by max_views (nothing is allocated in the steady
// state).  The per-bus columns are all zero between calls.
struct lc3_mx_plan {
    std::vector<int> bus_in, bus_out, bus_S, bus_fs;  // per bus: inputs, outputs, sample count and rate of this call
    std::vector<int> bus_row;                         // per bus: cursor of the counting sort
    std::vector<int> bus_strided;                     // per bus: views with a stride above 1
    std::vector<int> touched;                         // the buses this call names
    std::vector<int> in_pos;                          // per input view: its row
    int n_buses = 0, n_wg = 0;
    explicit lc3_mx_plan(int max_views)
        : bus_in((size_t)max_views, 0), bus_out((size_t)max_views, 0), bus_S((size_t)max_views, 0), bus_fs((size_t)max_views, 0),
          bus_row((size_t)max_views, 0), bus_strided((size_t)max_views, 0), in_pos((size_t)max_views, 0) {
        touched.reserve((size_t)max_views);
    }
    void clear() {
        for (int b : touched) bus_in[(size_t)b] = bus_out[(size_t)b] = bus_S[(size_t)b] = bus_fs[(size_t)b] = bus_strided[(size_t)b] = 0;
        touched.clear();
    }
};

// one view of either list against its array; S: its sample count
static inline int lc3_mx_check_view(const lc3_mx_stream *streams, int n_streams, const lc3_iview &v, uint64_t base, uint64_t elems, int *S) {
    if (v.channel < 0 || v.channel >= n_streams) return LC3_IV_ECHANNEL;
    if (v.n_frames < 1) return LC3_IV_ELENGTH;
    if (v.reserved[0] != 0 || v.reserved[1] != 0 || v.reserved[2] != 0) return LC3_IV_EINVAL;
    if (v.pcm_stride < 1 || v.pcm_stride > 8) return LC3_IV_EINVAL;
    if (v.pcm_off < 0) return LC3_IV_EINVAL;
    const int nf = streams[v.channel].nf;
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
    *S = (int)samples;
    return LC3_IV_OK;
}

// Every check of the call but `mx` itself.  On LC3_IV_OK the plan's per-bus columns hold this call's counts (lc3_mviews_build reads and
// clears them); on a refusal they are cleared here.  Nothing else is written.
static inline int lc3_mviews_check(const lc3_mx_stream *streams, int n_streams, int max_views, const lc3_iview *in_views,
                                   const lc3_mix_in_t *ins, int n_in, const lc3_iview *out_views, const lc3_mix_out_t *outs, int n_out,
                                   const lc3_mx_bounds &B, lc3_mx_plan &P) {
    if (n_in < 0 || n_out < 0) return LC3_IV_EINVAL;
    if (n_in > 0 && (!in_views || !ins || B.in_base == 0)) return LC3_IV_EINVAL;
    if (n_out > 0 && (!out_views || !outs || B.out_base == 0)) return LC3_IV_EINVAL;
    const uint64_t in_len = B.in_elems > UINT64_MAX / 2 ? UINT64_MAX : B.in_elems * 2;
    const uint64_t out_len = B.out_elems > UINT64_MAX / 2 ? UINT64_MAX : B.out_elems * 2;
    if (B.in_base != 0 && B.out_base != 0 && lc3_iv_ranges_overlap(B.in_base, in_len, B.out_base, out_len)) return LC3_IV_EINVAL;
    if ((uint64_t)n_in + (uint64_t)n_out > (uint64_t)max_views) return LC3_IV_ELENGTH;
    int rc = LC3_IV_OK;
    // a view joins its bus: the first one sets the bus's sample count and rate, every other one must have them
    auto join = [&](int bus, int S, int fs, int stride) {
        if (P.bus_S[(size_t)bus] == 0) {
            P.bus_S[(size_t)bus] = S;
            P.bus_fs[(size_t)bus] = fs;
            P.touched.push_back(bus);
        } else {
            if (P.bus_fs[(size_t)bus] != fs) return LC3_IV_EINVAL;
            if (P.bus_S[(size_t)bus] != S) return LC3_IV_ELENGTH;
        }
        P.bus_strided[(size_t)bus] += stride > 1;
        return LC3_IV_OK;
    };
    for (int i = 0; i < n_in && !rc; i++) {
        int S = 0;
        if (ins[i].bus < 0 || ins[i].bus >= max_views) rc = LC3_IV_EINVAL;
        else if (ins[i].gain_q14 < -32768 || ins[i].gain_q14 > 32767) rc = LC3_IV_EINVAL;
        else if ((rc = lc3_mx_check_view(streams, n_streams, in_views[i], B.in_base, B.in_elems, &S)) == 0 &&
                 (rc = join(ins[i].bus, S, streams[in_views[i].channel].fs_hz, in_views[i].pcm_stride)) == 0 && ++P.bus_in[(size_t)ins[i].bus] > LC3_MX_MAX_BUS_INPUTS)
            rc = LC3_IV_ELENGTH;
    }
    uint64_t wgs = 0;
    for (int o = 0; o < n_out && !rc; o++) {
        int S = 0;
        const int bus = outs[o].bus, m = outs[o].minus;
        if (bus < 0 || bus >= max_views) rc = LC3_IV_EINVAL;
        else if (m < -1 || m >= n_in || (m >= 0 && ins[m].bus != bus)) rc = LC3_IV_EINVAL;
        else if ((rc = lc3_mx_check_view(streams, n_streams, out_views[o], B.out_base, B.out_elems, &S)) == 0 &&
                 (rc = join(bus, S, streams[out_views[o].channel].fs_hz, out_views[o].pcm_stride)) == 0 && P.bus_out[(size_t)bus]++ == 0)
            wgs += ((uint64_t)S + LC3_MX_SPW - 1) / LC3_MX_SPW;
    }
    if (!rc && wgs > (uint64_t)0x7fffffff) rc = LC3_IV_ELENGTH;  // (workgroup numbers are 32-bit: more than 2^40 samples of buses in one call)
    if (rc) P.clear();
    return rc;
}

// Views and tables already checked (lc3_mviews_check has left its counts in P), n_out >= 1.  rows_in: n_in rows, rows_out: n_out rows,
// buses: room for n_out.  Views of one bus keep the caller's order; the buses lie in the order the call first names them (inputs, then
// outputs).  Leaves P's per-bus columns all zero.
static inline void lc3_mviews_build(const lc3_mx_stream *streams, const lc3_iview *in_views, const lc3_mix_in_t *ins, int n_in,
                                    const lc3_iview *out_views, const lc3_mix_out_t *outs, int n_out, lc3_mx_row *rows_in,
                                    lc3_mx_row *rows_out, lc3_mx_bus *buses, lc3_mx_plan &P) {
    auto fill = [&](lc3_mx_row &r, const lc3_iview &v, int aux) {
        const int nf = streams[v.channel].nf;
        r.off = (uint64_t)v.pcm_off;
        r.magic = streams[v.channel].magic;
        r.pitch = v.pcm_pitch ? v.pcm_pitch : nf * v.pcm_stride;
        r.stride = v.pcm_stride;
        r.nf = nf;
        r.aux = aux;
    };
    // the bus rows, and the input rows behind their buses' cursors
    int row = 0, orow = 0, wg = 0, nb = 0;
    for (int b : P.touched) {
        if (P.bus_out[(size_t)b] > 0) {
            lc3_mx_bus &R = buses[nb++];
            R.first_in = row;
            R.n_in = P.bus_in[(size_t)b];
            R.first_out = orow;
            R.n_out = P.bus_out[(size_t)b];
            R.S = P.bus_S[(size_t)b];
            R.wg0 = wg;
            R.planar = P.bus_strided[(size_t)b] == 0;
            R.reserved = 0;
            wg += (int)(((unsigned)R.S + (unsigned)LC3_MX_SPW - 1u) / (unsigned)LC3_MX_SPW);
            orow += R.n_out;
        }
        P.bus_row[(size_t)b] = row;
        P.bus_fs[(size_t)b] = row;  // (from here on: the bus's first input row)
        row += P.bus_in[(size_t)b];
    }
    P.n_buses = nb;
    P.n_wg = wg;
    for (int i = 0; i < n_in; i++) {
        const int at = P.bus_row[(size_t)ins[i].bus]++;
        P.in_pos[(size_t)i] = at;
        fill(rows_in[at], in_views[i], ins[i].gain_q14);
    }
    // the output rows: the cursors start over at the buses' first output rows
    orow = 0;
    for (int b : P.touched) {
        P.bus_row[(size_t)b] = orow;
        orow += P.bus_out[(size_t)b];
    }
    for (int o = 0; o < n_out; o++) {
        const int b = outs[o].bus, m = outs[o].minus;
        fill(rows_out[P.bus_row[(size_t)b]++], out_views[o], m >= 0 ? P.in_pos[(size_t)m] - P.bus_fs[(size_t)b] : -1);
    }
    P.clear();
}
