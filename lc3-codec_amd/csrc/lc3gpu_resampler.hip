// lc3gpu_resampler -- the companion library of lc3gpu_resample_mixed_views (include/lc3gpu.h): the resampler object and its one kernel.
// gfx950 only.  Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fno-fast-math -fPIC -shared (build_native in
// lc3-codec_amd/api.py) -> liblc3gpu_resampler.so, which the main library links; the main library's lc3gpu_resampler_api.cpp forwards the
// five public entry points here.
//
// Why a library of its own: as for the inspector, the analyzer and the mixer (lc3gpu_inspector.hip).  Every kernel of the main library and
// the three other companions' kernels are pinned, name and resource figures, to committed listings; a rate conversion needs no codec handle,
// only where the samples lie, a coefficient table of its own (tables/lc3_resample_tables.h) and a FIR history per channel, so its device
// code lives here.  The kernel's name says "rate", not "resample": the main library holds the encoder's LTPF resampler.
//
// The kernel: ONE WORKGROUP PER CHUNK of LC3_RS_CHUNK output samples of a view, one launch per call, LC3_RS_LANES lanes, workgroups uniform
// in their view by the plan (lc3_host_resample_views.h).  The three phases of the lane body (lc3_dev_resample.h) with two barriers between
// them: the input window and the ratio's table into LDS, one output sample per lane and step out of LDS into LDS, pairs of output samples
// to memory.  11 356 bytes of static LDS: fourteen workgroups' worth fit a CU's 160 KB, the waves are the limit, not the LDS.
//
// The history hazard is designed out by two buffers per channel (lc3_host_resample_views.h): a launch reads one and writes the other.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/lc3gpu.h"

#define LC3_IV_HD static __host__ __device__ inline
#define LC3_RS_COEF_QUAL static __device__ const
#include "lc3_dev_resample.h"

static_assert(sizeof(lc3gpu_view) == sizeof(lc3_iview), "lc3_iview is lc3gpu_view");
static_assert(sizeof(lc3gpu_rate_desc) == 12, "lc3gpu_rate_desc is three ints");
static_assert(LC3_RS_EUNSUPPORTED == LC3GPU_EUNSUPPORTED, "the codes of include/lc3gpu.h");

// rows: the call's table (lc3_rviews_build).  Workgroup blockIdx.x owns output samples [(wg - wg0) * LC3_RS_CHUNK, + LC3_RS_CHUNK) of its
// row's view.  pcm_in and pcm_out do not overlap (the host refuses a call where they do); hist is the resampler's own.
__global__ __launch_bounds__(LC3_RS_LANES) void lc3_rate_views_kernel(const lc3_rs_row *__restrict__ rows, int n_rows, const int16_t *pcm_in,
                                                                      int16_t *pcm_out, int16_t *hist) {
    __shared__ lc3_rs_lds lds;
    const int wg = blockIdx.x, tid = threadIdx.x;
    const lc3_rs_row &r = rows[lc3_rs_find_row(rows, n_rows, wg)];
    const int chunk = wg - r.wg0;
    const lc3_rs_chunk c = lc3_rs_chunk_of(r, chunk);
    lc3_rs_stage(r, c, tid, lds, pcm_in, hist);
    __syncthreads();
    lc3_rs_compute(r, c, tid, lds);
    __syncthreads();
    lc3_rs_store(r, c, chunk, tid, lds, pcm_in, pcm_out, hist);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
#include "lc3_host_ring.h"

struct lc3gpu_resampler {
    int max_views = 0;
    lc3_rs_state state;
    int16_t *d_hist = nullptr;  // [n_channels][2][LC3_RS_HIST]
    // a call's rows (at most max_views), uploaded through the ring (lc3_host_ring.h); ordered: on another stream than the previous call's,
    // a call waits for it on the device, since both kernels read and write the same histories
    lc3_host_ring ring;
};

extern "C" {
int lc3rs_destroy(lc3gpu_resampler *p) {
    if (!p) return LC3GPU_EINVAL;
    OnDevice on(p->ring.device);
    lc3_ring_destroy(p->ring);
    if (p->d_hist) (void)hipFree(p->d_hist);
    delete p;
    return LC3GPU_OK;
}

int lc3rs_create(lc3gpu_resampler **out, int n_channels, const lc3gpu_rate_desc *descs, int max_views) {
    if (!out) return LC3GPU_EINVAL;
    *out = nullptr;
    if (!descs || n_channels < 1 || max_views < 1) return LC3GPU_EINVAL;
    if (n_channels > INT_MAX / (2 * LC3_RS_HIST)) return LC3GPU_ELENGTH;  // (places in the history array are 32-bit)
    std::vector<lc3_rs_channel> channels((size_t)n_channels);
    for (int i = 0; i < n_channels; i++) {
        const int rc = lc3_rs_make_channel(descs[i].fs_in_hz, descs[i].fs_out_hz, descs[i].frame_us, channels[(size_t)i]);
        if (rc) return rc;
    }
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
        (void)hipGetLastError();
        return LC3GPU_ENODEVICE;
    }
    lc3gpu_resampler *p = new (std::nothrow) lc3gpu_resampler();
    if (!p) return LC3GPU_EHIP;
    p->max_views = max_views;
    p->state.channels.swap(channels);
    const size_t hist_bytes = (size_t)n_channels * 2 * LC3_RS_HIST * sizeof(int16_t);
    hipError_t e = lc3_ring_create(p->ring, (size_t)max_views * sizeof(lc3_rs_row));
    if (e == hipSuccess) e = hipMalloc((void **)&p->d_hist, hist_bytes);
    if (e == hipSuccess) e = hipMemset(p->d_hist, 0, hist_bytes);  // (never read before it is written: every channel starts fresh)
    if (e != hipSuccess) {
        (void)hipGetLastError();
        (void)lc3rs_destroy(p);
        return LC3GPU_EHIP;
    }
    *out = p;
    return LC3GPU_OK;
}

// no wait and no launch: the named channels read zeros inside their next launch
int lc3rs_reset(lc3gpu_resampler *p) {
    if (!p) return LC3GPU_EINVAL;
    for (lc3_rs_channel &c : p->state.channels) lc3_rs_reset_channel(c);
    return LC3GPU_OK;
}

int lc3rs_reset_channels(lc3gpu_resampler *p, const int32_t *channels, int n) {
    if (!p || n < 0 || (n > 0 && !channels)) return LC3GPU_EINVAL;
    const int n_channels = (int)p->state.channels.size();
    for (int i = 0; i < n; i++)
        if (channels[i] < 0 || channels[i] >= n_channels) return LC3GPU_ECHANNEL;  // (before any channel is reset)
    for (int i = 0; i < n; i++) lc3_rs_reset_channel(p->state.channels[(size_t)channels[i]]);
    return LC3GPU_OK;
}

int lc3rs_mixed_views(lc3gpu_resampler *p, const lc3gpu_view *in_views, const int16_t *d_pcm_in, size_t in_elems, const lc3gpu_view *out_views,
                      int16_t *d_pcm_out, size_t out_elems, int n_views, void *hip_stream) {
    if (!p) return LC3GPU_EINVAL;
    lc3_rs_bounds B;
    B.in_base = (uint64_t)(uintptr_t)d_pcm_in;
    B.in_elems = (uint64_t)in_elems;
    B.out_base = (uint64_t)(uintptr_t)d_pcm_out;
    B.out_elems = (uint64_t)out_elems;
    const lc3_iview *vi = (const lc3_iview *)in_views, *vo = (const lc3_iview *)out_views;
    const int rc = lc3_rviews_check(p->state, p->max_views, vi, vo, n_views, B);
    if (rc) return rc;
    if (n_views == 0) return LC3GPU_OK;
    OnDevice on(p->ring.device);
    const hipStream_t stream = (hipStream_t)hip_stream;
    uint8_t *h_slot, *d_slot;
    LC3_HIP_TRY(lc3_ring_acquire(p->ring, stream, true, h_slot, d_slot));
    lc3_rs_row *rows = (lc3_rs_row *)h_slot;
    lc3_rviews_build(p->state, vi, vo, n_views, rows);
    hipError_t e = hipMemcpyAsync(d_slot, rows, (size_t)n_views * sizeof(lc3_rs_row), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(lc3_rate_views_kernel, dim3((unsigned)p->state.n_wg), dim3(LC3_RS_LANES), 0, stream, (const lc3_rs_row *)d_slot, n_views,
                           d_pcm_in, d_pcm_out, p->d_hist);
        e = hipGetLastError();
    }
    if (e != hipSuccess) {  // nothing was launched: no channel has advanced
        (void)hipGetLastError();
        lc3_rviews_unbuild(p->state, vi, n_views, rows);
        return LC3GPU_EHIP;
    }
    LC3_HIP_TRY(lc3_ring_commit(p->ring, stream));
    return LC3GPU_OK;
}

// tests and tools: the plan's figures (output samples of a view per workgroup, lanes per workgroup, the ring's slots, history samples)
int lc3rs_plan_info(int *samples_per_wg, int *lanes, int *ring_slots, int *hist_samples) {
    if (samples_per_wg) *samples_per_wg = LC3_RS_CHUNK;
    if (lanes) *lanes = LC3_RS_LANES;
    if (ring_slots) *ring_slots = lc3_host_ring::slots;
    if (hist_samples) *hist_samples = LC3_RS_HIST;
    return LC3GPU_OK;
}
}
