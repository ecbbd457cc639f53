// lc3gpu_inspector -- the companion library of lc3gpu_inspect_mixed_views (include/lc3gpu.h): the inspector object, its one kernel and
// its tables.  gfx950 only.  Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fno-fast-math -fPIC -shared (build_native in
// lc3-codec_amd/api.py) -> liblc3gpu_inspector.so, which the main library links; the main library's lc3gpu_inspector_api.cpp forwards the
// three public entry points here.
//
// Why a library of its own: every kernel of the main library is pinned, name and resource figures, to committed listings, and a kernel
// added to one of its modules can move the register allocation of its neighbours.  Inspection needs nothing of the main library -- no
// handle, no configuration slot, no device-filled table: the lane body (lc3_inspect_record, lc3_dev_dec_inspect.h) takes the
// configuration as three integers and reads compile-time tables only -- so its device code lives here, with its own copies of those
// tables, and the main library's modules are what they were.
//
// The kernel: ONE LANE PER FRAME, one launch per call.  The plan (lc3_host_inspect_views.h) keeps every workgroup uniform in
// configuration and frame size; a workgroup finds its bucket row, a lane its view row, both by bisection in the uploaded tables.  Dynamic
// LDS: the parser's lookup, spectral and TNS models, then per frame its 128-byte record (lane-major), the index of its outputs, 14 words
// of lsb-mode flags (word-major) and its bytes at the bucket's pitch.  Every lane copies its own frame from where it lies into its slot;
// the status byte goes out from the lane, the records leave through LDS, eight lanes per record, 16 bytes per store.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/lc3gpu.h"

// what the device headers take from their translation unit (lc3_dev_common.h): the inspection walk runs every lane on its own, so only
// the compiler-level ordering point and the 24-bit multiply are supplied; the rest are the headers' own defaults
#define LC3_SYNC()                                            \
    do {                                                      \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); \
        __builtin_amdgcn_wave_barrier();                      \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); \
    } while (0)
#define LC3_MUL24(a, b) __umul24((a), (b))
#include "lc3_dev_dec_inspect.h"

#define LC3_IV_HD static __host__ __device__ inline
#include "lc3_host_inspect_views.h"

static_assert(LC3_IV_LDS_FIXED == 4096 + 64 * LC3_DCF_ROW_WORDS * 4 + LC3_TNS_MODEL_WORDS * 4, "the plan's fixed LDS is the kernel's");
static_assert(LC3_IV_LDS_PER_FRAME == 4 * LC3_FI_WORDS + 8 + 4 * LC3_INSPECT_BITS_WORDS, "the plan's LDS per frame is the kernel's");
static_assert(LC3_IV_LDS_FIXED % 16 == 0, "the records are read back 16 bytes at a time");
static_assert(LC3_IV_RECORD_BYTES == 4 * LC3_FI_WORDS && LC3_IV_MAX_NBYTES == LC3_MAX_NE, "the plan's record and size limits are the kernel's");

// rows / buckets: the call's tables (lc3_iviews_build).  bad, status, info: any may be null (the host sees to it that status or info is
// not).  Workgroup blockIdx.x of blockDim.x = fpb lanes; a workgroup with fewer frames than lanes reaches both barriers with all of them.
__global__ __launch_bounds__(256) void lc3_inspect_views_kernel(const lc3_iv_row *__restrict__ rows, const lc3_iv_bucket *__restrict__ buckets,
                                                                int n_buckets, const uint8_t *__restrict__ in, const uint8_t *__restrict__ bad,
                                                                uint8_t *__restrict__ status, int32_t *__restrict__ info) {
    __builtin_amdgcn_s_setprio(1);  // (as the main library's lane-per-frame kernels: they keep their pace beside a wave-per-stream kernel)
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x, fpb = blockDim.x, wg = blockIdx.x;
    const lc3_iv_bucket &b = buckets[lc3_iv_find_bucket(buckets, n_buckets, wg)];
    const int nb = b.nbytes, ne = b.ne, fs_ind = b.fs_ind_ms & 0xff, n_ms_10 = b.fs_ind_ms >> 8;
    const int nfr = lc3_iv_wg_frames(b, wg, fpb);
    uint8_t *s_lookup = smem;
    uint32_t *s_cf = (uint32_t *)(smem + 4096);
    uint32_t *s_tns = (uint32_t *)(smem + 4096 + 64 * LC3_DCF_ROW_WORDS * 4);
    int32_t *s_rec = (int32_t *)(smem + LC3_IV_LDS_FIXED);
    uint64_t *s_dst = (uint64_t *)(smem + LC3_IV_LDS_FIXED + 4 * LC3_FI_WORDS * fpb);
    uint32_t *s_bits = (uint32_t *)(smem + LC3_IV_LDS_FIXED + (4 * LC3_FI_WORDS + 8) * fpb);
    uint8_t *s_bytes = smem + LC3_IV_LDS_FIXED + (4 * LC3_FI_WORDS + 8 + 4 * LC3_INSPECT_BITS_WORDS) * fpb;
    {
        for (int i = tid; i < LC3_TNS_MODEL_WORDS; i += fpb) s_tns[i] = lc3_tns_model_word(i);
        const uint32_t *lk32 = (const uint32_t *)LC3T_AC_SPEC_LOOKUP;
        uint32_t *d32 = (uint32_t *)s_lookup;
        for (int i = tid; i < 1024; i += fpb) d32[i] = lk32[i];
        for (int i = tid; i < 64 * LC3_DCF_ROW_WORDS; i += fpb) s_cf[i] = lc3_dcf_word(i);
    }
    int flagged = 0;
    if (tid < nfr) {
        uint64_t src, dst;
        lc3_iv_lane_place(rows, b, wg, tid, fpb, src, dst);
        s_dst[tid] = dst;
        flagged = bad ? (int)bad[dst] : 0;
        // the lane's own frame, from where it lies: four bytes at a time, whatever the two addresses' alignment
        const uint8_t *g = in + src;
        uint8_t *s = s_bytes + tid * nb;
        int k = 0;
        for (; k + 4 <= nb; k += 4) {
            uint32_t w;
            __builtin_memcpy(&w, g + k, 4);
            __builtin_memcpy(s + k, &w, 4);
        }
        for (; k < nb; k++) s[k] = g[k];
    }
    __syncthreads();
    if (tid < nfr) {
        lc3_parse_ctx c;
        c.dbg = nullptr;
        c.bytes = s_bytes + tid * nb;
        c.lookup = s_lookup;
        c.cf = s_cf;
        c.tns = s_tns;
        int32_t *rec = s_rec + tid * LC3_FI_WORDS;
        lc3_inspect_record(c, flagged, nb, rec, s_bits + tid, fpb, ne, fs_ind, n_ms_10);
        if (status) status[s_dst[tid]] = (uint8_t)rec[LC3_FI_STATUS];
    }
    __syncthreads();
    if (info) {  // (uniform: without records nothing but the status bytes leaves the workgroup)
        if ((((uintptr_t)info) & 15u) == 0) {
            for (int i = tid; i < nfr * (LC3_FI_WORDS / 4); i += fpb) {
                const int j = i / (LC3_FI_WORDS / 4), q = i % (LC3_FI_WORDS / 4);
                ((lc3_i4 *)(info + s_dst[j] * LC3_FI_WORDS))[q] = ((const lc3_i4 *)s_rec)[i];
            }
        } else {
            for (int i = tid; i < nfr * LC3_FI_WORDS; i += fpb) info[s_dst[i / LC3_FI_WORDS] * LC3_FI_WORDS + i % LC3_FI_WORDS] = s_rec[i];
        }
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
#include "lc3_host_ring.h"

struct lc3gpu_inspector {
    int max_views = 0;
    std::vector<lc3_iv_stream> streams;
    lc3_iv_plan plan;
    // a call's view rows, then its bucket rows, uploaded through the ring (lc3_host_ring.h); not ordered: the inspector keeps nothing on
    // the device between calls
    lc3_host_ring ring;
};

extern "C" {
int lc3insp_destroy(lc3gpu_inspector *p) {
    if (!p) return LC3GPU_EINVAL;
    lc3_ring_destroy(p->ring);
    delete p;
    return LC3GPU_OK;
}

int lc3insp_create(lc3gpu_inspector **out, int n_streams, const lc3gpu_stream_desc *descs, int max_views) {
    if (!out) return LC3GPU_EINVAL;
    *out = nullptr;
    if (!descs || n_streams < 1 || max_views < 1) return LC3GPU_EINVAL;
    std::vector<lc3_iv_stream> streams((size_t)n_streams);
    for (int i = 0; i < n_streams; i++) {
        if (lc3_iv_config(descs[i].frame_us, descs[i].fs_hz, streams[(size_t)i])) return LC3GPU_EINVAL;
        if (descs[i].nbytes < 1 || descs[i].nbytes > LC3_IV_MAX_NBYTES) return LC3GPU_ELENGTH;
        streams[(size_t)i].nbytes = descs[i].nbytes;
    }
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
        (void)hipGetLastError();
        return LC3GPU_ENODEVICE;
    }
    lc3gpu_inspector *p = new (std::nothrow) lc3gpu_inspector;
    if (!p) return LC3GPU_EHIP;
    p->streams.swap(streams);
    p->max_views = max_views;
    const size_t max_buckets = (size_t)(max_views < LC3_IV_CONFIGS * LC3_IV_MAX_NBYTES ? max_views : LC3_IV_CONFIGS * LC3_IV_MAX_NBYTES);
    if (lc3_ring_create(p->ring, (size_t)max_views * sizeof(lc3_iv_row) + max_buckets * sizeof(lc3_iv_bucket)) != hipSuccess) {
        (void)hipGetLastError();
        (void)lc3insp_destroy(p);
        return LC3GPU_EHIP;
    }
    *out = p;
    return LC3GPU_OK;
}

int lc3insp_mixed_views(lc3gpu_inspector *p, const lc3gpu_view *views, int n_views, const uint8_t *d_in, size_t in_bytes,
                        const uint8_t *d_bad_frame, size_t n_flags, uint8_t *d_status, size_t n_status, lc3gpu_frame_info *d_info, size_t n_info,
                        void *hip_stream) {
    static_assert(sizeof(lc3gpu_view) == sizeof(lc3_iview), "lc3_iview is lc3gpu_view");
    if (!p) return LC3GPU_EINVAL;
    lc3_iv_bounds B;
    B.in_base = (uint64_t)(uintptr_t)d_in;
    B.in_bytes = (uint64_t)in_bytes;
    B.flags_base = (uint64_t)(uintptr_t)d_bad_frame;
    B.n_flags = (uint64_t)n_flags;
    B.status_base = (uint64_t)(uintptr_t)d_status;
    B.n_status = (uint64_t)n_status;
    B.info_base = (uint64_t)(uintptr_t)d_info;
    B.n_info = (uint64_t)n_info;
    B.use_flags = d_bad_frame != nullptr;
    B.use_status = d_status != nullptr;
    B.use_info = d_info != nullptr;
    int frames = 0, max_nbytes = 0;
    const lc3_iview *v = (const lc3_iview *)views;
    const int rc = lc3_iviews_check(p->streams.data(), (int)p->streams.size(), p->max_views, v, n_views, B, &frames, &max_nbytes);
    if (rc) return rc;
    if (n_views == 0) return LC3GPU_OK;
    OnDevice on(p->ring.device);
    const hipStream_t stream = (hipStream_t)hip_stream;
    uint8_t *h_slot, *d_slot;
    LC3_HIP_TRY(lc3_ring_acquire(p->ring, stream, false, h_slot, d_slot));
    lc3_iv_row *rows = (lc3_iv_row *)h_slot;
    const size_t rows_bytes = (size_t)n_views * sizeof(lc3_iv_row);
    lc3_iv_bucket *buckets = (lc3_iv_bucket *)(h_slot + rows_bytes);  // (at most one bucket per view)
    const unsigned fpb = lc3_iv_fpb(max_nbytes);
    const size_t lds = lc3_iv_lds_bytes(max_nbytes);
    lc3_iviews_build(p->streams.data(), v, n_views, (int)fpb, rows, buckets, p->plan);
    // one upload: the rows and, right behind them, the bucket rows
    const size_t buckets_bytes = (size_t)p->plan.n_buckets * sizeof(lc3_iv_bucket);
    LC3_HIP_TRY(hipMemcpyAsync(d_slot, rows, rows_bytes + buckets_bytes, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(lc3_inspect_views_kernel, dim3((unsigned)p->plan.n_wg), dim3(fpb), lds, stream, (const lc3_iv_row *)d_slot,
                       (const lc3_iv_bucket *)(d_slot + rows_bytes), p->plan.n_buckets, d_in, d_bad_frame, d_status, (int32_t *)d_info);
    LC3_HIP_TRY(hipGetLastError());
    LC3_HIP_TRY(lc3_ring_commit(p->ring, stream));
    return LC3GPU_OK;
}

// tests and tools: the plan's figures for a frame size (frames per workgroup, dynamic LDS bytes) and the ring's slots
int lc3insp_plan_info(int max_nbytes, int *fpb, size_t *lds_bytes, int *ring_slots) {
    if (max_nbytes < 1 || max_nbytes > LC3_IV_MAX_NBYTES) return LC3GPU_ELENGTH;
    if (fpb) *fpb = (int)lc3_iv_fpb(max_nbytes);
    if (lds_bytes) *lds_bytes = lc3_iv_lds_bytes(max_nbytes);
    if (ring_slots) *ring_slots = lc3_host_ring::slots;
    return LC3GPU_OK;
}
}
