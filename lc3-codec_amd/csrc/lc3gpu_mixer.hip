// lc3gpu_mixer -- the companion library of lc3gpu_mix_mixed_views (include/lc3gpu.h): the mixer object and its one kernel.  gfx950 only.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fno-fast-math -fPIC -shared (build_native in lc3-codec_amd/api.py) ->
// liblc3gpu_mixer.so, which the main library links; the main library's lc3gpu_mixer_api.cpp forwards the three public entry points here.
//
// Why a library of its own: as for the inspector and the analyzer (lc3gpu_inspector.hip).  Every kernel of the main library and the two
// other companions' kernels are pinned, name and resource figures, to committed listings; a mix needs no handle, no configuration slot and
// no table, only where the samples lie, so its device code lives here.
//
// The kernel: ONE LANE PER PAIR OF SAMPLES of a bus, one launch per call, LC3_MX_LANES lanes per workgroup, workgroups uniform in their bus
// by the plan (lc3_host_mix_views.h).  No LDS, no barrier: the rows are read through the pointers as they are, the same for every lane
// of a workgroup (scalar loads), and the lane body (lc3_mix_pair, lc3_dev_mix.h) keeps its two totals in registers; a bus whose rows are
// all planar takes the form of it that tests no stride.  It is a pure data-movement kernel: 4 bytes per lane per access for planar views,
// consecutive lanes on consecutive words (a wave reads and writes 256 contiguous bytes), 2 bytes per lane per access for strided ones.  A
// wider form (8 or 16 bytes per lane where a view's alignment allows) is not built: it would need a second lane body beside this one, and
// the contract guarantees 4-byte alignment only.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/lc3gpu.h"

#define LC3_IV_HD static __host__ __device__ inline
#include "lc3_dev_mix.h"

static_assert(sizeof(lc3gpu_view) == sizeof(lc3_iview), "lc3_iview is lc3gpu_view");
static_assert(sizeof(lc3gpu_mix_in) == sizeof(lc3_mix_in_t) && sizeof(lc3gpu_mix_out) == sizeof(lc3_mix_out_t), "the room tables of include/lc3gpu.h");

// rows_in / rows_out / buses: the call's tables (lc3_mviews_build).  Workgroup blockIdx.x owns samples [(wg - wg0) * LC3_MX_SPW, + LC3_MX_SPW)
// of its bus, lane tid the pair at 2 * tid of them; (wg - wg0) * LC3_MX_SPW < S <= 2^31 - 1, and S is even, so a pair that starts below S
// ends below S.  pcm_in and pcm_out do not overlap (the host refuses a call where they do).
__global__ __launch_bounds__(LC3_MX_LANES) void lc3_mix_views_kernel(const lc3_mx_row *__restrict__ rows_in, const lc3_mx_row *__restrict__ rows_out,
                                                                     const lc3_mx_bus *__restrict__ buses, int n_buses,
                                                                     const int16_t *__restrict__ pcm_in, int16_t *__restrict__ pcm_out) {
    const int wg = blockIdx.x;
    const lc3_mx_bus &b = buses[lc3_mx_find_bus(buses, n_buses, wg)];
    const uint32_t s = (uint32_t)(wg - b.wg0) * (uint32_t)LC3_MX_SPW + 2u * threadIdx.x;
    if (s >= (uint32_t)b.S) return;
    lc3_mix_bus_pair(b, rows_in, rows_out, pcm_in, pcm_out, s);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
#include "lc3_host_ring.h"

struct lc3gpu_mixer {
    int max_views = 0;
    std::vector<lc3_mx_stream> streams;
    lc3_mx_plan plan;
    // a call's input rows, its output rows, then its bus rows (at most max_views rows and max_views buses), uploaded through the ring
    // (lc3_host_ring.h); not ordered: the mixer keeps nothing on the device between calls
    lc3_host_ring ring;
    explicit lc3gpu_mixer(int mv) : max_views(mv), plan(mv) {}
};

extern "C" {
int lc3mix_destroy(lc3gpu_mixer *p) {
    if (!p) return LC3GPU_EINVAL;
    lc3_ring_destroy(p->ring);
    delete p;
    return LC3GPU_OK;
}

int lc3mix_create(lc3gpu_mixer **out, int n_streams, const lc3gpu_stream_desc *descs, int max_views) {
    if (!out) return LC3GPU_EINVAL;
    *out = nullptr;
    if (!descs || n_streams < 1 || max_views < 1) return LC3GPU_EINVAL;
    std::vector<lc3_mx_stream> streams((size_t)n_streams);
    for (int i = 0; i < n_streams; i++) {
        lc3_iv_stream c;
        if (lc3_iv_config(descs[i].frame_us, descs[i].fs_hz, c)) return LC3GPU_EINVAL;
        if (descs[i].nbytes < 1 || descs[i].nbytes > LC3_IV_MAX_NBYTES) return LC3GPU_ELENGTH;
        lc3_mx_make_stream(descs[i].frame_us, descs[i].fs_hz, streams[(size_t)i]);
    }
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
        (void)hipGetLastError();
        return LC3GPU_ENODEVICE;
    }
    lc3gpu_mixer *p = new (std::nothrow) lc3gpu_mixer(max_views);
    if (!p) return LC3GPU_EHIP;
    p->streams.swap(streams);
    if (lc3_ring_create(p->ring, (size_t)max_views * (sizeof(lc3_mx_row) + sizeof(lc3_mx_bus))) != hipSuccess) {
        (void)hipGetLastError();
        (void)lc3mix_destroy(p);
        return LC3GPU_EHIP;
    }
    *out = p;
    return LC3GPU_OK;
}

int lc3mix_mixed_views(lc3gpu_mixer *p, const lc3gpu_view *in_views, const lc3gpu_mix_in *ins, int n_in, const int16_t *d_pcm_in,
                       size_t in_elems, const lc3gpu_view *out_views, const lc3gpu_mix_out *outs, int n_out, int16_t *d_pcm_out,
                       size_t out_elems, void *hip_stream) {
    if (!p) return LC3GPU_EINVAL;
    lc3_mx_bounds B;
    B.in_base = (uint64_t)(uintptr_t)d_pcm_in;
    B.in_elems = (uint64_t)in_elems;
    B.out_base = (uint64_t)(uintptr_t)d_pcm_out;
    B.out_elems = (uint64_t)out_elems;
    const lc3_iview *vi = (const lc3_iview *)in_views, *vo = (const lc3_iview *)out_views;
    const lc3_mix_in_t *ti = (const lc3_mix_in_t *)ins;
    const lc3_mix_out_t *to = (const lc3_mix_out_t *)outs;
    const int rc = lc3_mviews_check(p->streams.data(), (int)p->streams.size(), p->max_views, vi, ti, n_in, vo, to, n_out, B, p->plan);
    if (rc) return rc;
    if (n_out == 0) {
        p->plan.clear();
        return LC3GPU_OK;
    }
    OnDevice on(p->ring.device);
    const hipStream_t stream = (hipStream_t)hip_stream;
    uint8_t *h_slot, *d_slot;
    if (lc3_ring_acquire(p->ring, stream, false, h_slot, d_slot) != hipSuccess) {
        (void)hipGetLastError();
        p->plan.clear();  // (the check's counts: the plan that would have consumed them is not built)
        return LC3GPU_EHIP;
    }
    const size_t in_bytes = (size_t)n_in * sizeof(lc3_mx_row), out_bytes = (size_t)n_out * sizeof(lc3_mx_row);
    lc3_mviews_build(p->streams.data(), vi, ti, n_in, vo, to, n_out, (lc3_mx_row *)h_slot, (lc3_mx_row *)(h_slot + in_bytes),
                     (lc3_mx_bus *)(h_slot + in_bytes + out_bytes), p->plan);
    // one upload: the input rows, the output rows and, right behind them, the bus rows
    const size_t bus_bytes = (size_t)p->plan.n_buses * sizeof(lc3_mx_bus);
    LC3_HIP_TRY(hipMemcpyAsync(d_slot, h_slot, in_bytes + out_bytes + bus_bytes, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(lc3_mix_views_kernel, dim3((unsigned)p->plan.n_wg), dim3(LC3_MX_LANES), 0, stream, (const lc3_mx_row *)d_slot,
                       (const lc3_mx_row *)(d_slot + in_bytes), (const lc3_mx_bus *)(d_slot + in_bytes + out_bytes), p->plan.n_buses, d_pcm_in,
                       d_pcm_out);
    LC3_HIP_TRY(hipGetLastError());
    LC3_HIP_TRY(lc3_ring_commit(p->ring, stream));
    return LC3GPU_OK;
}

// tests and tools: the plan's figures (samples of a bus per workgroup, lanes per workgroup, the ring's slots)
int lc3mix_plan_info(int *samples_per_wg, int *lanes, int *ring_slots) {
    if (samples_per_wg) *samples_per_wg = LC3_MX_SPW;
    if (lanes) *lanes = LC3_MX_LANES;
    if (ring_slots) *ring_slots = lc3_host_ring::slots;
    return LC3GPU_OK;
}
}
