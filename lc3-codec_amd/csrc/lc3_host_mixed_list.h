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

// How a launch finds a stream's PCM, frame bytes and bad-frame flags in the ragged layout of a mixed-configuration handle: stream i's PCM
// at element T * tab[i].pcm_off1, its bytes at T * tab[i].byte_off1, its flags at tab[i].flag_idx * T
struct lc3_stream_io {
    long long pcm_off1, byte_off1;  // per frame of the batch: sum of nf / of nbytes over the caller's earlier streams
    int flag_idx, pad;              // the stream's index in the caller's order
};
#define LC3_MAX_GROUPS 24
struct lc3_group {
    int slot, fixed;              // configuration slot; the compile-time view that applies (lc3_cfg_views.h: 1..4), 0 = the run-time view
    int first_stream, n_streams;  // [first_stream, first_stream + n_streams) in the handle's internal order (a list call: launch positions)
    int wg_stream, wg_frame;      // the group's first workgroup in a stream-kernel / frame-kernel launch
    int nbytes, ne, nb, pad;
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
        g.pad = 0;
        g.frame_base = (long long)P.first[i] * (long long)T;
        wg_stream += ((unsigned)P.count[i] + wg_waves - 1) / wg_waves;
        wg_frame += (unsigned)(((size_t)P.count[i] * (size_t)T + fpb - 1) / fpb);
    }
}
