// lc3gpu_meter -- the companion library of lc3gpu_measure_mixed_views (include/lc3gpu.h): the meter object and its one kernel.
// gfx950 only.  Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fno-fast-math -fPIC -shared (build_native in
// lc3-codec_amd/api.py) -> liblc3gpu_meter.so, which the main library links; the main library's lc3gpu_meter_api.cpp forwards the five
// public entry points here.
//
// Why a library of its own: as for the inspector, the analyzer, the mixer and the resampler (lc3gpu_inspector.hip).  Every kernel of the main
// library and the four other companions' kernels are pinned, name and resource figures, to committed listings; a level measure needs no
// codec handle, only where the samples lie and a small state per channel, so its device code lives here.
//
// The kernel: ONE WAVE PER VIEW, four views per workgroup of LC3_MT_LANES lanes, one launch per call.  The wave walks its view's frames in
// order: the lanes read the frame coalesced and keep a partial each (lc3_dev_level.h), a shuffle reduction folds the partials into lane 0,
// lane 0 finishes the frame -- ms, envelope, gate -- keeps last / env / hang in registers and writes the record as two 16-byte stores and
// the activity byte; after the last frame it writes the channel's state.  No LDS, no barrier.  A view of thousands of frames is one serial
// wave: that is correct, not tuned; the shapes that matter are tens of thousands of views of one to four frames.
//
// Only the wave of a channel's one view touches that channel's state in a launch (a channel may be named once per call), so one state
// buffer per channel is enough (lc3_host_measure_views.h).
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/lc3gpu.h"

#define LC3_IV_HD static __host__ __device__ inline
#include "lc3_dev_level.h"

static_assert(sizeof(lc3gpu_view) == sizeof(lc3_iview), "lc3_iview is lc3gpu_view");
static_assert(sizeof(lc3gpu_meter_desc) == 24, "lc3gpu_meter_desc is six 32-bit fields");
static_assert(sizeof(lc3gpu_level) == LC3_MT_RECORD_BYTES, "lc3gpu_level is the record lc3_lvl_finish fills");

static __device__ inline lc3_lvl_partial lc3_lvl_from_lane(const lc3_lvl_partial &p, int off) {
    lc3_lvl_partial q;
    const uint32_t lo = (uint32_t)__shfl_down((int)(uint32_t)p.sum_sq, off, LC3_MT_WAVE);
    const uint32_t hi = (uint32_t)__shfl_down((int)(uint32_t)(p.sum_sq >> 32), off, LC3_MT_WAVE);
    q.sum_sq = ((uint64_t)hi << 32) | lo;
    q.sum = __shfl_down(p.sum, off, LC3_MT_WAVE);
    q.min = __shfl_down(p.min, off, LC3_MT_WAVE);
    q.max = __shfl_down(p.max, off, LC3_MT_WAVE);
    q.n_clipped = (uint32_t)__shfl_down((int)p.n_clipped, off, LC3_MT_WAVE);
    q.n_cross = (uint32_t)__shfl_down((int)p.n_cross, off, LC3_MT_WAVE);
    return q;
}

// rows: the call's table (lc3_mviews_build), one per view.  Wave w of workgroup blockIdx.x owns row 4 * blockIdx.x + w.  pcm overlaps
// neither output (the host refuses a call where it does); state is the meter's own.  active / levels: either may be null, not both.
__global__ __launch_bounds__(LC3_MT_LANES) void lc3_level_views_kernel(const lc3_mt_row *__restrict__ rows, int n_views, const int16_t *__restrict__ pcm,
                                                                       uint8_t *__restrict__ active, uint4 *__restrict__ levels,
                                                                       lc3_mt_dstate *__restrict__ state) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / LC3_MT_WAVE)), lane = (int)(threadIdx.x % LC3_MT_WAVE);
    const int v = (int)blockIdx.x * LC3_MT_WAVES_PER_WG + wave;
    if (v >= n_views) return;
    const lc3_mt_row r = rows[v];
    lc3_lvl_state st = {0, 0u, 0};
    if (!r.fresh) {
        const lc3_mt_dstate s = state[r.channel];
        st.last = s.last, st.env = s.env, st.hang = s.hang;
    }
    uint64_t base = r.pcm_off, dst = r.flag_off;
    int32_t before = st.last;
    for (int t = 0; t < r.n_frames; t++) {
        lc3_lvl_partial p = lc3_lvl_lane(pcm, base, r.stride, r.nf, lane, before);
        const int32_t last = lc3_lvl_last(pcm, r, base);
        for (int off = LC3_MT_WAVE / 2; off > 0; off >>= 1) p = lc3_lvl_combine(p, lc3_lvl_from_lane(p, off));
        if (lane == 0) {
            uint32_t w[8];
            lc3_lvl_finish(p, r, last, st, w);
            if (levels) {
                levels[2 * dst] = make_uint4(w[0], w[1], w[2], w[3]);
                levels[2 * dst + 1] = make_uint4(w[4], w[5], w[6], w[7]);
            }
            if (active) active[dst] = (uint8_t)((w[6] >> 16) & 1u);
        }
        before = last;
        base += (uint64_t)(uint32_t)r.pitch;
        dst += (uint64_t)(uint32_t)r.flag_pitch;
    }
    if (lane == 0) {
        lc3_mt_dstate s;
        s.last = st.last, s.env = st.env, s.hang = st.hang, s.reserved = 0;
        state[r.channel] = s;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
#include "lc3_host_ring.h"

struct lc3gpu_meter {
    int max_views = 0;
    lc3_mt_state state;
    lc3_mt_dstate *d_state = nullptr;  // [n_channels]: ONE record per channel (only one wave of a launch touches it)
    // a call's rows (at most max_views), uploaded through the ring (lc3_host_ring.h); ordered: on another stream than the previous call's,
    // a call waits for it on the device, since both kernels read and write the same states
    lc3_host_ring ring;
};

extern "C" {
int lc3mtr_destroy(lc3gpu_meter *p) {
    if (!p) return LC3GPU_EINVAL;
    OnDevice on(p->ring.device);
    lc3_ring_destroy(p->ring);
    if (p->d_state) (void)hipFree(p->d_state);
    delete p;
    return LC3GPU_OK;
}

int lc3mtr_create(lc3gpu_meter **out, int n_channels, const lc3gpu_meter_desc *descs, int max_views) {
    if (!out) return LC3GPU_EINVAL;
    *out = nullptr;
    if (!descs || n_channels < 1 || max_views < 1) return LC3GPU_EINVAL;
    std::vector<lc3_mt_channel> channels((size_t)n_channels);
    for (int i = 0; i < n_channels; i++) {
        const lc3gpu_meter_desc &d = descs[i];
        const int rc = lc3_mt_make_channel(d.fs_hz, d.frame_us, d.attack_q15, d.release_q15, d.threshold, d.hang_frames, channels[(size_t)i]);
        if (rc) return rc;
    }
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
        (void)hipGetLastError();
        return LC3GPU_ENODEVICE;
    }
    lc3gpu_meter *p = new (std::nothrow) lc3gpu_meter();
    if (!p) return LC3GPU_EHIP;
    p->max_views = max_views;
    p->state.channels.swap(channels);
    const size_t state_bytes = (size_t)n_channels * sizeof(lc3_mt_dstate);
    hipError_t e = lc3_ring_create(p->ring, (size_t)max_views * sizeof(lc3_mt_row));
    if (e == hipSuccess) e = hipMalloc((void **)&p->d_state, state_bytes);
    if (e == hipSuccess) e = hipMemset(p->d_state, 0, state_bytes);  // (never read before it is written: every channel starts fresh)
    if (e != hipSuccess) {
        (void)hipGetLastError();
        (void)lc3mtr_destroy(p);
        return LC3GPU_EHIP;
    }
    *out = p;
    return LC3GPU_OK;
}

// no wait and no launch: the named channels start from zeros inside their next launch
int lc3mtr_reset(lc3gpu_meter *p) {
    if (!p) return LC3GPU_EINVAL;
    for (lc3_mt_channel &c : p->state.channels) lc3_mt_reset_channel(c);
    return LC3GPU_OK;
}

int lc3mtr_reset_channels(lc3gpu_meter *p, const int32_t *channels, int n) {
    if (!p || n < 0 || (n > 0 && !channels)) return LC3GPU_EINVAL;
    const int n_channels = (int)p->state.channels.size();
    for (int i = 0; i < n; i++)
        if (channels[i] < 0 || channels[i] >= n_channels) return LC3GPU_ECHANNEL;  // (before any channel is reset)
    for (int i = 0; i < n; i++) lc3_mt_reset_channel(p->state.channels[(size_t)channels[i]]);
    return LC3GPU_OK;
}

int lc3mtr_mixed_views(lc3gpu_meter *p, const lc3gpu_view *views, int n_views, const int16_t *d_pcm, size_t pcm_elems, uint8_t *d_active,
                       size_t n_active, lc3gpu_level *d_levels, size_t n_levels, void *hip_stream) {
    if (!p) return LC3GPU_EINVAL;
    lc3_mt_bounds B;
    B.pcm_base = (uint64_t)(uintptr_t)d_pcm;
    B.pcm_elems = (uint64_t)pcm_elems;
    B.active_base = (uint64_t)(uintptr_t)d_active;
    B.n_active = (uint64_t)n_active;
    B.levels_base = (uint64_t)(uintptr_t)d_levels;
    B.n_levels = (uint64_t)n_levels;
    B.use_active = d_active != nullptr;
    B.use_levels = d_levels != nullptr;
    const lc3_iview *vi = (const lc3_iview *)views;
    const int rc = lc3_mviews_check(p->state, p->max_views, vi, n_views, B);
    if (rc) return rc;
    if (n_views == 0) return LC3GPU_OK;
    OnDevice on(p->ring.device);
    const hipStream_t stream = (hipStream_t)hip_stream;
    uint8_t *h_slot, *d_slot;
    LC3_HIP_TRY(lc3_ring_acquire(p->ring, stream, true, h_slot, d_slot));
    lc3_mt_row *rows = (lc3_mt_row *)h_slot;
    lc3_mviews_build(p->state, vi, n_views, rows);
    hipError_t e = hipMemcpyAsync(d_slot, rows, (size_t)n_views * sizeof(lc3_mt_row), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) {
        const unsigned n_wg = ((unsigned)n_views + LC3_MT_WAVES_PER_WG - 1u) / LC3_MT_WAVES_PER_WG;
        hipLaunchKernelGGL(lc3_level_views_kernel, dim3(n_wg), dim3(LC3_MT_LANES), 0, stream, (const lc3_mt_row *)d_slot, n_views, d_pcm, d_active,
                           (uint4 *)d_levels, p->d_state);
        e = hipGetLastError();
    }
    if (e != hipSuccess) {  // nothing was launched: no channel has advanced
        (void)hipGetLastError();
        lc3_mviews_unbuild(p->state, vi, n_views, rows);
        return LC3GPU_EHIP;
    }
    LC3_HIP_TRY(lc3_ring_commit(p->ring, stream));
    return LC3GPU_OK;
}

// tests and tools: the plan's figures (waves of a workgroup = views of a workgroup, lanes per workgroup, the ring's slots, bytes of a
// channel's state on the device)
int lc3mtr_plan_info(int *waves_per_wg, int *lanes, int *ring_slots, int *state_bytes) {
    if (waves_per_wg) *waves_per_wg = LC3_MT_WAVES_PER_WG;
    if (lanes) *lanes = LC3_MT_LANES;
    if (ring_slots) *ring_slots = lc3_host_ring::slots;
    if (state_bytes) *state_bytes = LC3_MT_STATE_BYTES;
    return LC3GPU_OK;
}
}
