// Host-side plan of ONE call over a list of a mixed-configuration handle's channels (lc3gpu_encode_mixed_list /
// lc3gpu_decode_mixed_list), and the plain tables a mixed launch reads on the device (lc3_stream_io, lc3_group, lc3_groups).
// Pure C++ (no HIP calls), like lc3_host_plan.h, so that the C ABI layer and the CPU wave emulator used by the tests
// (tests/emu/lc3_emu_mixed_list.cpp) build the very same plan.
//
// A mixed handle keeps its streams sorted by configuration ("internal" order); a group is one run of streams of equal (rate, duration,
// frame bytes).  A list call names any subset of the caller's stream indices in any order.  The plan buckets the list by group, in a
// stable order (two listed streams of a group keep the order the caller gave them), which fixes every listed stream's LAUNCH POSITION:
//   entries[pos]   the stream's internal index | LC3_LIST_FRESH (lc3_dev_list.h): where its carried state lives, whether it starts fresh
//   tab[pos]       where its PCM, its bytes and its flags are in the caller's buffers: ragged and compact IN LIST ORDER, i.e.
//                  pcm_off1 / byte_off1 are prefix sums of nf / nbytes over the list items in front of it, flag_idx its list position
//   lc3_groups     one row per group WITH listed streams (a group without takes no row and no workgroup): first_stream = the group's
//                  first launch position, n_streams = its listed count; the plane columns of launch position p are [p * T, (p + 1) * T)
// Every kernel of the tick is then one launch: the wave-per-stream kernels find state through entries and PCM through tab, the lane-per-
// frame kernels of a mixed batch run unchanged (they index tab[first_stream + s] and plane columns by launch position only).
#pragma once
#include <cstddef>
#include <cstdint>
#include <algorithm>
#include <vector>

// How a launch finds a stream's PCM, frame bytes and bad-frame flags in the ragged layout of a mixed-configuration handle: stream i's PCM
// at element T * tab[i].pcm_off1, its bytes at T * tab[i].byte_off1, its flags at tab[i].flag_idx * T
struct lc3_stream_io {
    long long pcm_off1, byte_off1;  // per frame of the batch: sum of nf / of nbytes over the caller's earlier streams
    int flag_idx, pad;              // the stream's index in the caller's order; pad: 0 (an mc-items call: the sample stride, lc3_mcitems_build)
};
#define LC3_MAX_GROUPS 24
struct lc3_group {
    int slot, fixed;              // configuration slot; the compile-time view that applies (lc3_cfg_views.h: 1..4), 0 = the run-time view
    int first_stream, n_streams;  // [first_stream, first_stream + n_streams) in the handle's internal order (a list call: launch positions)
    int wg_stream, wg_frame;      // the group's first workgroup in a stream-kernel / frame-kernel launch
    int nbytes, ne, nb;
    int n_frames;                 // an items call (lc3_mitems_*): frames per stream of this row; every other call: 0, the launch's argument holds
    long long frame_base;         // first plane column of the group
};
struct lc3_groups {
    int n, pad;
    lc3_group g[LC3_MAX_GROUPS];
};

// what the plan needs to know of a handle: per group its configuration, per caller stream its group and internal index
struct lc3_mlist_group {
    int slot, view, nbytes, ne, nb, nf;
};
struct lc3_mlist_stream {
    int group, internal;
};
struct lc3_mlist_plan {
    int count[LC3_MAX_GROUPS];  // listed streams per group of the handle
    int first[LC3_MAX_GROUPS];  // the group's first launch position
    int n_list, max_nbytes;
};

// Builds entries[n_list] and tab[n_list] (both in launch order) and the per-group counts.  channels: the caller's list, already checked
// (every index in range, none twice).  fresh: per INTERNAL index, 1 = the channel starts from the constructed state.
static inline void lc3_mlist_build(const lc3_mlist_group *groups, int n_groups, const lc3_mlist_stream *streams, const uint8_t *fresh,
                                   const int32_t *channels, int n_list, int32_t *entries, lc3_stream_io *tab, lc3_mlist_plan &P) {
    for (int g = 0; g < LC3_MAX_GROUPS; g++) P.count[g] = P.first[g] = 0;
    P.n_list = n_list;
    P.max_nbytes = 0;
    for (int i = 0; i < n_list; i++) P.count[streams[channels[i]].group] += 1;
    int next[LC3_MAX_GROUPS];
    for (int g = 0, pos = 0; g < n_groups; g++) {
        P.first[g] = next[g] = pos;
        pos += P.count[g];
        if (P.count[g] && groups[g].nbytes > P.max_nbytes) P.max_nbytes = groups[g].nbytes;
    }
    long long po = 0, bo = 0;  // prefix sums in the caller's LIST order
    for (int i = 0; i < n_list; i++) {
        const lc3_mlist_stream &st = streams[channels[i]];
        const int pos = next[st.group]++;  // (stable: the list's order inside a group)
        entries[pos] = (int32_t)((uint32_t)st.internal | (fresh[st.internal] ? 0x80000000u : 0u));
        tab[pos].pcm_off1 = po;
        tab[pos].byte_off1 = bo;
        tab[pos].flag_idx = i;
        tab[pos].pad = 0;
        po += groups[st.group].nf;
        bo += groups[st.group].nbytes;
    }
}

// The group table of the launches of one tick: T frames per stream, wg_waves streams per workgroup of the wave-per-stream kernels, fpb
// frames per workgroup of the lane-per-frame kernels.  Groups without a listed stream are left out.
static inline void lc3_mlist_groups(const lc3_mlist_group *groups, int n_groups, const lc3_mlist_plan &P, int T, unsigned wg_waves, unsigned fpb,
                                    lc3_groups &G, unsigned &wg_stream, unsigned &wg_frame) {
    G.n = 0;
    G.pad = 0;
    wg_stream = wg_frame = 0;
    for (int i = 0; i < n_groups; i++) {
        if (!P.count[i]) continue;
        lc3_group &g = G.g[G.n++];
        g.slot = groups[i].slot;
        g.fixed = groups[i].view;
        g.first_stream = P.first[i];
        g.n_streams = P.count[i];
        g.wg_stream = (int)wg_stream;
        g.wg_frame = (int)wg_frame;
        g.nbytes = groups[i].nbytes;
        g.ne = groups[i].ne;
        g.nb = groups[i].nb;
        g.n_frames = 0;
        g.frame_base = (long long)P.first[i] * (long long)T;
        wg_stream += ((unsigned)P.count[i] + wg_waves - 1) / wg_waves;
        wg_frame += (unsigned)(((size_t)P.count[i] * (size_t)T + fpb - 1) / fpb);
    }
}

// ---- a frame count and a frame size per listed stream (lc3gpu_encode_mixed_items / lc3gpu_decode_mixed_items) -------------------------
// An item names a channel, how many frames it gets in this call and at which size (0: the descriptor's).  The plan buckets the items by
// (configuration, effective nbytes, n_frames) -- the frame count is part of the key because a workgroup of the wave-per-stream kernels
// holds four streams of ONE bucket and these meet at workgroup barriers whose number depends on the frame count.  Buckets are ordered by
// that key, the items inside a bucket keep the caller's order (stable), which fixes every item's LAUNCH POSITION as in a list call:
//   entries[pos]   internal index | LC3_LIST_FRESH
//   tab[pos]       ABSOLUTE offsets into the caller's ragged compact buffers: pcm_off1 in elements (sum of n_frames * nf over the items in
//                  front), byte_off1 in bytes (sum of n_frames * nbytes), flag_idx in frames (sum of n_frames).  The kernels of the items
//                  path reach them with a factor of one where the other calls' kernels multiply by the launch's frame count
//   buckets[b]     first launch position, count, and frame_base = the running sum of count * n_frames: the bucket's first plane column
// A bucket becomes one lc3_group row (n_frames in the row).  A launch takes at most LC3_MAX_GROUPS rows, so a call with more buckets runs
// as consecutive launch sets (lc3_mitems_rows over [b0, b1)): one launch per kernel per 24 buckets, one upload, one host check.
struct lc3_mitem {  // = lc3gpu_item (include/lc3gpu.h)
    int32_t channel, n_frames, nbytes, reserved;
};
struct lc3_mitems_bucket {
    int group;             // a group of the handle with the bucket's configuration (slot, view, ne, nb, nf are its)
    int nbytes, n_frames;  // effective frame size, frames per stream
    int first, count;      // launch positions [first, first + count)
    int next;              // (chain of the buckets of one (slot, nbytes) cell while the plan is built)
    long long frame_base;
};
struct lc3_mitems_plan {
    std::vector<lc3_mitems_bucket> buckets;  // in launch order
    std::vector<int> cell, bucket_of;        // scratch: head bucket per (slot, nbytes); bucket per item
    std::vector<lc3_mitem> flat;             // scratch of lc3_mcitems_build: the items' channels as items of one channel each,
    std::vector<int> pos_of;                 // and their launch positions (kept here so that a tick allocates nothing once they have grown)
    int n_items = 0, max_frames = 0;         // max_frames: the largest per-item count
    long long frames = 0;                    // of the whole call
};
#define LC3_MITEMS_SLOTS 12
#define LC3_MITEMS_MAX_NBYTES 400

// items: already checked (channel in range and not twice, n_frames >= 1, nbytes 0 or in range).  fresh: per INTERNAL index.
// pos_of: when given, item i's launch position.  ITEM: anything with the fields channel, n_frames, nbytes -- lc3_mitem, or the view of a
// views call (lc3_mview below), which is bucketed as it lies in the caller's array; tab: may be null there (a views call has rows of its own).
template <class ITEM>
static inline void lc3_mitems_build_of(const lc3_mlist_group *groups, const lc3_mlist_stream *streams, const uint8_t *fresh, const ITEM *items,
                                       int n_items, int32_t *entries, lc3_stream_io *tab, lc3_mitems_plan &P, int *pos_of) {
    P.buckets.clear();
    P.cell.assign((size_t)LC3_MITEMS_SLOTS * (LC3_MITEMS_MAX_NBYTES + 1), -1);
    P.bucket_of.resize((size_t)n_items);
    P.n_items = n_items;
    P.max_frames = 0;
    P.frames = 0;
    for (int i = 0; i < n_items; i++) {  // pass 1: the item's bucket, in order of first appearance
        const int gi = streams[items[i].channel].group;
        const int nbytes = items[i].nbytes ? items[i].nbytes : groups[gi].nbytes, T = items[i].n_frames;
        int &head = P.cell[(size_t)groups[gi].slot * (LC3_MITEMS_MAX_NBYTES + 1) + (size_t)nbytes];
        int b = head;
        while (b >= 0 && P.buckets[(size_t)b].n_frames != T) b = P.buckets[(size_t)b].next;
        if (b < 0) {
            b = (int)P.buckets.size();
            P.buckets.push_back({gi, nbytes, T, 0, 0, head, 0});
            head = b;
        }
        P.buckets[(size_t)b].count += 1;
        P.bucket_of[(size_t)i] = b;
        if (T > P.max_frames) P.max_frames = T;
    }
    // the buckets in key order; rank[b]: where bucket b of pass 1 went
    const int nb = (int)P.buckets.size();
    std::vector<int> order((size_t)nb), rank((size_t)nb), next((size_t)nb);
    for (int b = 0; b < nb; b++) order[(size_t)b] = b;
    std::sort(order.begin(), order.end(), [&](int a, int b) {
        const lc3_mitems_bucket &x = P.buckets[(size_t)a], &y = P.buckets[(size_t)b];
        if (groups[x.group].slot != groups[y.group].slot) return groups[x.group].slot < groups[y.group].slot;
        if (x.nbytes != y.nbytes) return x.nbytes < y.nbytes;
        return x.n_frames < y.n_frames;
    });
    std::vector<lc3_mitems_bucket> sorted((size_t)nb);
    int pos = 0;
    for (int r = 0; r < nb; r++) {
        lc3_mitems_bucket &b = sorted[(size_t)r];
        b = P.buckets[(size_t)order[(size_t)r]];
        rank[(size_t)order[(size_t)r]] = r;
        b.first = next[(size_t)r] = pos;
        b.next = -1;
        b.frame_base = P.frames;
        pos += b.count;
        P.frames += (long long)b.count * (long long)b.n_frames;
    }
    P.buckets.swap(sorted);
    long long po = 0, bo = 0, fo = 0;  // pass 2: absolute prefix sums in the caller's LIST order
    for (int i = 0; i < n_items; i++) {
        const lc3_mlist_stream &st = streams[items[i].channel];
        const int r = rank[(size_t)P.bucket_of[(size_t)i]];
        const lc3_mitems_bucket &b = P.buckets[(size_t)r];
        const int p = next[(size_t)r]++;  // (stable: the list's order inside a bucket)
        entries[p] = (int32_t)((uint32_t)st.internal | (fresh[st.internal] ? 0x80000000u : 0u));
        if (tab) {
            tab[p].pcm_off1 = po;
            tab[p].byte_off1 = bo;
            tab[p].flag_idx = (int)fo;
            tab[p].pad = 0;
        }
        if (pos_of) pos_of[i] = p;  // (lc3_mcitems_build, lc3_mviews_build: the item's launch position)
        po += (long long)b.n_frames * (long long)groups[b.group].nf;
        bo += (long long)b.n_frames * (long long)b.nbytes;
        fo += b.n_frames;
    }
}
static inline void lc3_mitems_build(const lc3_mlist_group *groups, const lc3_mlist_stream *streams, const uint8_t *fresh, const lc3_mitem *items,
                                    int n_items, int32_t *entries, lc3_stream_io *tab, lc3_mitems_plan &P, int *pos_of = nullptr) {
    lc3_mitems_build_of(groups, streams, fresh, items, n_items, entries, tab, P, pos_of);
}

// ---- items of several channels in WAV sample order (lc3gpu_encode_mixed_mc_items / lc3gpu_decode_mixed_mc_items) ------------------------
// An mc item names C consecutive descriptors -- one stream's channels -- with one frame count and one frame size for all of them; its PCM
// is int16[T][nf][C] (L R L R), its bytes uint8[T][C][nbytes], its flags uint8[T][C], the items compact in list order.  The plan expands
// every item into its C channels and buckets THOSE exactly as lc3_mitems_build does (the channel count is no part of the key: a workgroup
// may hold channels of items with C = 1, 2 and 3 side by side).  Channel c of an item whose running bases are po, bo, fo gets
//   tab[pos] = { pcm_off1 = po + c, byte_off1 = bo + c * nbytes, flag_idx = fo + c, pad = C }
// -- absolute, as an items call's -- and pad, 0 in every other call's table, carries the sample stride: frame t of the channel has its
// samples at pcm_off1 + (t * nf + n) * C, its bytes at byte_off1 + t * C * nbytes, its flag at flag_idx + t * C.  Buckets, launch sets and
// rows (lc3_mitems_rows) are those of an items call over the expanded list.
struct lc3_mcitem {  // = lc3gpu_mc_item (include/lc3gpu.h)
    int32_t first_channel, n_channels, n_frames, nbytes;
};
#define LC3_MCITEMS_MAX_CHANNELS 8
// the expanded list's length
static inline size_t lc3_mcitems_channels(const lc3_mcitem *items, int n_items) {
    size_t n = 0;
    for (int i = 0; i < n_items; i++) n += (size_t)items[i].n_channels;
    return n;
}
// items: already checked (channel ranges inside the handle and disjoint, n_channels 1..8, one configuration per item, n_frames >= 1, nbytes
// in range or 0 with equal descriptors).  entries / tab: one per CHANNEL (lc3_mcitems_channels).  fresh: per INTERNAL index.
static inline void lc3_mcitems_build(const lc3_mlist_group *groups, const lc3_mlist_stream *streams, const uint8_t *fresh, const lc3_mcitem *items,
                                     int n_items, int32_t *entries, lc3_stream_io *tab, lc3_mitems_plan &P) {
    std::vector<lc3_mitem> &flat = P.flat;
    flat.clear();
    for (int i = 0; i < n_items; i++)
        for (int c = 0; c < items[i].n_channels; c++) flat.push_back({items[i].first_channel + c, items[i].n_frames, items[i].nbytes, 0});
    // buckets and launch positions are the items plan's over the expanded list; its offsets are replaced below
    std::vector<int> &pos_of = P.pos_of;
    pos_of.resize(flat.size());
    lc3_mitems_build(groups, streams, fresh, flat.data(), (int)flat.size(), entries, tab, P, pos_of.data());
    long long po = 0, bo = 0, fo = 0;
    size_t k = 0;
    for (int i = 0; i < n_items; i++) {
        const int C = items[i].n_channels, T = items[i].n_frames;
        int nb = 0, nf = 0;
        for (int c = 0; c < C; c++, k++) {
            const int p = pos_of[k], gi = streams[flat[k].channel].group;
            nb = flat[k].nbytes ? flat[k].nbytes : groups[gi].nbytes;  // (equal over the item's channels: checked)
            nf = groups[gi].nf;
            tab[p].pcm_off1 = po + c;
            tab[p].byte_off1 = bo + (long long)c * (long long)nb;
            tab[p].flag_idx = (int)(fo + c);
            tab[p].pad = C;
        }
        po += (long long)T * (long long)nf * (long long)C;
        bo += (long long)T * (long long)C * (long long)nb;
        fo += (long long)T * (long long)C;
    }
}

// ---- every item with a placement of its own (lc3gpu_encode_mixed_views / lc3gpu_decode_mixed_views) --------------------------------------
// A view is an item (channel, n_frames, nbytes) that also says WHERE its data lies: sample n of frame t at element
// pcm_off + t * pcm_pitch + n * pcm_stride, frame t's bytes at byte_off + t * byte_pitch, its flag at flag_off + t * flag_pitch.  One
// descriptor covers the compact items layout (stride 1, pitches 0 = the defaults), one channel of an mc item (stride C, pitches C * nf,
// C * nbytes, C), a slot ring and a sub-channel of a wide capture buffer.  Buckets, launch positions, launch sets and rows are those of an
// items call over the views' (channel, n_frames, nbytes): placement is no part of the key.  What differs is the per-stream device row:
//   rows[pos]      lc3_view_io: the three offsets, the stride and the three RESOLVED pitches (the 0 = default of the caller's view is
//                  filled in here, so the kernels test nothing).  A row type of its own: lc3_stream_io is read by every other kernel
// With caller-given offsets the extent check (lc3_mviews_check) is the only thing between a typo and a stray access on the device: it
// runs before the plan is built, in unsigned 64-bit arithmetic that cannot overflow, and a refused call builds and sends nothing.
struct lc3_mview {  // = lc3gpu_view (include/lc3gpu.h)
    int32_t channel, n_frames, nbytes, pcm_stride;
    int64_t pcm_off, byte_off, flag_off;
    int32_t pcm_pitch, byte_pitch, flag_pitch;
    int32_t reserved[3];
};
struct lc3_view_io {
    long long pcm_off, byte_off, flag_off;  // elements, bytes, flags: frame 0 of the stream in the caller's buffers
    int stride;                             // elements between two samples of a frame (1: the 32-bit PCM path; >= 2: the 16-bit one)
    int pcm_pitch, byte_pitch, flag_pitch;  // from frame t to frame t + 1, resolved (never 0)
};
#define LC3_MVIEWS_MAX_STRIDE 8
// what lc3_mviews_check returns: the values of LC3GPU_OK / LC3GPU_EINVAL / LC3GPU_ECHANNEL / LC3GPU_ELENGTH (include/lc3gpu.h)
enum { LC3_MVIEWS_OK = 0, LC3_MVIEWS_EINVAL = -1, LC3_MVIEWS_ECHANNEL = -2, LC3_MVIEWS_ELENGTH = -3 };
// the caller's buffers: the PCM base ADDRESS (its alignment is checked, nothing is read), the element / byte / flag counts the views must
// stay inside, whether flags are read at all (a decoder with d_bad_frame), and the smallest frame size (20 encoder, 1 decoder)
struct lc3_mviews_bounds {
    uint64_t pcm_base, pcm_elems, io_bytes, n_flags;
    int use_flags, min_bytes;
};
// [off, off + (T - 1) * pitch + last] inside [0, size): T < 2^31 and pitch < 2^31, so the span stays below 2^62 + 2^31 and no step wraps
static inline bool lc3_mviews_inside(int64_t off, int T, int pitch, uint64_t last, uint64_t size) {
    if ((uint64_t)off >= size) return false;  // (off >= 0: checked by the caller)
    const uint64_t span = (uint64_t)(T - 1) * (uint64_t)pitch + last;
    return span < size - (uint64_t)off;
}
// Every check of a views call but the handle's own (null pointers, uniform handle, bound stream).  seen / call: per channel the number of
// the call that named it last, and this call's number (the repeated-channel check of the list calls).  frames / max_frames: the call's
// total and its largest per-view count.  Nothing is written but seen[].
static inline int lc3_mviews_check(const lc3_mlist_group *groups, const lc3_mlist_stream *streams, int n_channels, const lc3_mview *views,
                                   int n_views, const lc3_mviews_bounds &B, uint32_t *seen, uint32_t call, size_t *frames, int *max_frames) {
    uint64_t total = 0;
    int most = 0;
    for (int i = 0; i < n_views; i++) {
        const lc3_mview &v = views[i];
        if (v.channel < 0 || v.channel >= n_channels || seen[v.channel] == call) return LC3_MVIEWS_ECHANNEL;
        seen[v.channel] = call;
        if (v.n_frames < 1) return LC3_MVIEWS_ELENGTH;
        if (v.nbytes != 0 && (v.nbytes < B.min_bytes || v.nbytes > LC3_MITEMS_MAX_NBYTES)) return LC3_MVIEWS_ELENGTH;
        if (v.reserved[0] != 0 || v.reserved[1] != 0 || v.reserved[2] != 0) return LC3_MVIEWS_EINVAL;
        if (v.pcm_stride < 1 || v.pcm_stride > LC3_MVIEWS_MAX_STRIDE) return LC3_MVIEWS_EINVAL;
        if (v.pcm_off < 0 || v.byte_off < 0 || (B.use_flags && v.flag_off < 0)) return LC3_MVIEWS_EINVAL;
        const lc3_mlist_group &g = groups[streams[v.channel].group];
        const int nbytes = v.nbytes ? v.nbytes : g.nbytes, min_pitch = g.nf * v.pcm_stride;  // (<= 480 * 8)
        if (v.pcm_pitch != 0 && v.pcm_pitch < min_pitch) return LC3_MVIEWS_EINVAL;
        if (v.byte_pitch != 0 && v.byte_pitch < nbytes) return LC3_MVIEWS_EINVAL;
        if (B.use_flags && v.flag_pitch < 0) return LC3_MVIEWS_EINVAL;
        if (v.pcm_stride == 1) {  // the 32-bit path: every frame's first sample on a 4-byte boundary
            if ((v.pcm_off & 1) != 0 || (v.pcm_pitch & 1) != 0 || (B.pcm_base & 3u) != 0) return LC3_MVIEWS_EINVAL;
        } else if ((B.pcm_base & 1u) != 0) return LC3_MVIEWS_EINVAL;
        const int pp = v.pcm_pitch ? v.pcm_pitch : min_pitch, bp = v.byte_pitch ? v.byte_pitch : nbytes, fp = v.flag_pitch ? v.flag_pitch : 1;
        if (!lc3_mviews_inside(v.pcm_off, v.n_frames, pp, (uint64_t)(g.nf - 1) * (uint64_t)v.pcm_stride, B.pcm_elems)) return LC3_MVIEWS_ELENGTH;
        if (!lc3_mviews_inside(v.byte_off, v.n_frames, bp, (uint64_t)(nbytes - 1), B.io_bytes)) return LC3_MVIEWS_ELENGTH;
        if (B.use_flags && !lc3_mviews_inside(v.flag_off, v.n_frames, fp, 0, B.n_flags)) return LC3_MVIEWS_ELENGTH;
        total += (uint64_t)v.n_frames;
        if (total > (uint64_t)0x7fffffff) return LC3_MVIEWS_ELENGTH;  // (frame counts are 32-bit on the device)
        if (v.n_frames > most) most = v.n_frames;
    }
    *frames = (size_t)total;
    *max_frames = most;
    return LC3_MVIEWS_OK;
}
// views: already checked (lc3_mviews_check).  entries / rows: one per view, in launch order.  fresh: per INTERNAL index.  use_flags == 0
// (no flags are read): the rows' flag fields are 0 / 1 whatever the views hold
static inline void lc3_mviews_build(const lc3_mlist_group *groups, const lc3_mlist_stream *streams, const uint8_t *fresh, const lc3_mview *views,
                                    int n_views, int use_flags, int32_t *entries, lc3_view_io *rows, lc3_mitems_plan &P) {
    // buckets and launch positions are the items plan's over the views as they lie (no copy of the list, no compact offsets)
    P.pos_of.resize((size_t)n_views);
    lc3_mitems_build_of(groups, streams, fresh, views, n_views, entries, (lc3_stream_io *)nullptr, P, P.pos_of.data());
    for (int i = 0; i < n_views; i++) {
        const lc3_mview &v = views[i];
        const lc3_mlist_group &g = groups[streams[v.channel].group];
        lc3_view_io &r = rows[P.pos_of[(size_t)i]];
        r.pcm_off = v.pcm_off;
        r.byte_off = v.byte_off;
        r.flag_off = use_flags ? v.flag_off : 0;
        r.stride = v.pcm_stride;
        r.pcm_pitch = v.pcm_pitch ? v.pcm_pitch : g.nf * v.pcm_stride;
        r.byte_pitch = v.byte_pitch ? v.byte_pitch : (v.nbytes ? v.nbytes : g.nbytes);
        r.flag_pitch = (use_flags && v.flag_pitch) ? v.flag_pitch : 1;
    }
}

// launch sets: buckets [b0, b1) with b1 - b0 <= LC3_MAX_GROUPS; set k of the call is [k * LC3_MAX_GROUPS, ...)
static inline int lc3_mitems_sets(const lc3_mitems_plan &P) { return ((int)P.buckets.size() + LC3_MAX_GROUPS - 1) / LC3_MAX_GROUPS; }
static inline void lc3_mitems_set(const lc3_mitems_plan &P, int k, int &b0, int &b1) {
    b0 = k * LC3_MAX_GROUPS;
    b1 = std::min((int)P.buckets.size(), b0 + LC3_MAX_GROUPS);
}
// the largest frame size of a launch set: what sizes the LDS of its packer / parser launches
static inline int lc3_mitems_max_nbytes(const lc3_mitems_plan &P, int b0, int b1) {
    int m = 0;
    for (int b = b0; b < b1; b++) m = std::max(m, P.buckets[(size_t)b].nbytes);
    return m;
}
// The group table of one launch set (as lc3_mlist_groups): one row per bucket, its frame count in the row, frame_base the bucket's own --
// the launch sets of a call use disjoint plane columns of the same planes
static inline void lc3_mitems_rows(const lc3_mlist_group *groups, const lc3_mitems_plan &P, int b0, int b1, unsigned wg_waves, unsigned fpb,
                                   lc3_groups &G, unsigned &wg_stream, unsigned &wg_frame) {
    G.n = 0;
    G.pad = 0;
    wg_stream = wg_frame = 0;
    for (int i = b0; i < b1; i++) {
        const lc3_mitems_bucket &b = P.buckets[(size_t)i];
        const lc3_mlist_group &cfg = groups[b.group];
        lc3_group &g = G.g[G.n++];
        g.slot = cfg.slot;
        g.fixed = cfg.view;
        g.first_stream = b.first;
        g.n_streams = b.count;
        g.wg_stream = (int)wg_stream;
        g.wg_frame = (int)wg_frame;
        g.nbytes = b.nbytes;
        g.ne = cfg.ne;
        g.nb = cfg.nb;
        g.n_frames = b.n_frames;
        g.frame_base = b.frame_base;
        wg_stream += ((unsigned)b.count + wg_waves - 1) / wg_waves;
        wg_frame += (unsigned)(((size_t)b.count * (size_t)b.n_frames + fpb - 1) / fpb);
    }
}
