// lc3gpu_analyzer -- the companion library of lc3gpu_analyze_mixed_views (include/lc3gpu.h): the analyzer object, its one kernel, its
// tables and its scratch columns.  gfx950 only.  Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fno-fast-math -fPIC -shared
// (build_native in lc3-codec_amd/api.py) -> liblc3gpu_analyzer.so, which the main library links; the main library's
// lc3gpu_analyzer_api.cpp forwards the three public entry points here.
//
// Why a library of its own: as for the inspector (lc3gpu_inspector.hip).  Every kernel of the main library and the inspector's one kernel
// are pinned, name and resource figures, to committed listings; analysis needs no handle, no configuration slot and no device-filled table
// -- the lane body (lc3_analyze_frame, lc3_dev_dec_analyze.h) takes the configuration as four integers, and without the main unit's table
// macros the device headers compute 10^(k / 28) and the TNS sines by the very functions the main library's tables are filled from -- so
// its device code lives here, with its own copies of the compile-time tables.
//
// The kernel: ONE LANE PER FRAME, one launch per call, workgroups uniform in configuration and frame size by the inspector's plan
// (lc3_host_inspect_views.h; lc3_host_analyze_views.h adds the analyzer's LDS figures and checks).  Dynamic LDS: the parser's lookup,
// spectral model and TNS models, the MPVQ offsets and the bucket's band index table, then per frame 16 scale factors (lane-major), the
// index of its outputs and its bytes at the bucket's pitch.  A lane copies its frame from where it lies, parses it and rebuilds its
// spectrum in its scratch column in HBM (lc3_parse_frame<1>, lc3_reconstruct_frame: the parse kernel's late == 0 branch), walks the column
// once for the energies, and stores its float and its two rows ITSELF, 16 bytes per store.  The other form -- a second barrier and the
// rows leaving through the columns, all lanes of the workgroup copying one frame's row after the other in whole cache lines -- was built
// and measured first: 2 % slower with all three outputs given (0.555 against 0.545 ms per 65 532 frames), since every
// row is then read once more by lanes that did not write it.  So the kernel has ONE workgroup barrier.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/lc3gpu.h"

// what the device headers take from their translation unit (lc3_dev_common.h): the compiler-level ordering point, the 24-bit multiply and
// the wave vote of the lane-per-frame reconstruction (a wave skips the TNS lattice and the residual refinement when none of its lanes
// needs them), as the main library's unit defines them; the rest are the headers' own defaults
#define LC3_SYNC()                                            \
    do {                                                      \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); \
        __builtin_amdgcn_wave_barrier();                      \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); \
    } while (0)
#define LC3_MUL24(a, b) __umul24((a), (b))
#define LC3_WAVE_ANY(pred) (__ballot((pred) != 0) != 0ull)
#include "lc3_dev_dec_analyze.h"

#define LC3_IV_HD static __host__ __device__ inline
#include "lc3_host_analyze_views.h"

#define LC3_AV_LDS_TABLES (4096 + 64 * LC3_DCF_ROW_WORDS * 4 + 16 * 11 * 4 + LC3_TNS_MODEL_WORDS * 4)
static_assert(LC3_AV_LDS_FIXED == LC3_AV_LDS_TABLES + 144, "the plan's fixed LDS is the kernel's");
static_assert(LC3_AV_LDS_PER_FRAME == 16 * 4 + 8, "the plan's LDS per frame is the kernel's");
static_assert(LC3_AV_LDS_FIXED % 16 == 0 && LC3_AV_LDS_PER_FRAME % 8 == 0, "the scale factors and the output indices are aligned");
static_assert(LC3_AV_COLUMN_WORDS == LC3_PLANE_WORDS && LC3_AV_SPEC_LINES == LC3_MAX_NE && LC3_IV_MAX_NBYTES == LC3_MAX_NE, "the plan's column is the parser's");
static_assert(LC3_AV_BANDS == LC3GPU_BANDS && LC3_AV_SPEC_LINES == LC3GPU_SPEC_LINES, "the rows of include/lc3gpu.h");
static_assert(LC3_PLANE_X % 4 == 0 && LC3_PLANE_LEV % 4 == 0 && LC3_PLANE_WORDS % 4 == 0 && LC3_PLANE_LEV + LC3_AV_BANDS <= LC3_PLANE_WORDS,
              "the rows leave the column 16 bytes at a time");

// rows / buckets: the call's tables (lc3_iviews_build).  columns: one column of LC3_PLANE_WORDS words per frame of the call, frame f of the
// sorted order at columns + f * LC3_PLANE_WORDS.  bad, energy, bands, spec: any may be null (the host sees to it that one output is not);
// spec is 16-byte aligned.  Workgroup blockIdx.x of blockDim.x = fpb lanes; a workgroup with fewer frames than lanes, or with flagged
// frames, reaches the barrier with all of its lanes.
__global__ __launch_bounds__(256) void lc3_analyze_views_kernel(const lc3_iv_row *__restrict__ rows, const lc3_iv_bucket *__restrict__ buckets,
                                                                int n_buckets, const uint8_t *__restrict__ in, const uint8_t *__restrict__ bad,
                                                                int32_t *__restrict__ columns, float *__restrict__ energy,
                                                                float *__restrict__ bands, float *__restrict__ spec) {
    __builtin_amdgcn_s_setprio(1);  // (as the main library's lane-per-frame kernels)
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x, fpb = blockDim.x, wg = blockIdx.x;
    const lc3_iv_bucket &b = buckets[lc3_iv_find_bucket(buckets, n_buckets, wg)];
    const int nbytes = b.nbytes;
    lc3_an_cfg cfg;
    cfg.ne = b.ne;
    cfg.fs_ind = b.fs_ind_ms & 0xff;
    cfg.n_ms_10 = b.fs_ind_ms >> 8;
    cfg.nb = lc3_av_bands(cfg.fs_ind, cfg.n_ms_10);
    const int nfr = lc3_iv_wg_frames(b, wg, fpb);
    uint8_t *s_lookup = smem;
    uint32_t *s_cf = (uint32_t *)(smem + 4096);
    uint32_t *s_mpvq = (uint32_t *)(smem + 4096 + 64 * LC3_DCF_ROW_WORDS * 4);
    uint32_t *s_tns = (uint32_t *)(smem + 4096 + 64 * LC3_DCF_ROW_WORDS * 4 + 16 * 11 * 4);
    uint16_t *s_ifs = (uint16_t *)(smem + LC3_AV_LDS_TABLES);  // 65 entries, 144 bytes reserved
    float *s_scf = (float *)(smem + LC3_AV_LDS_FIXED);
    uint64_t *s_dst = (uint64_t *)(smem + LC3_AV_LDS_FIXED + 16 * 4 * fpb);
    uint8_t *s_bytes = smem + LC3_AV_LDS_FIXED + LC3_AV_LDS_PER_FRAME * fpb;
    // the workgroup's columns: its first frame's number in the sorted order is below the call's frame count, which the host holds to max_frames
    int32_t *col0 = columns + (size_t)(b.frame0 + (wg - b.wg0) * fpb) * (size_t)LC3_PLANE_WORDS;
    {
        for (int i = tid; i < 16 * 11; i += fpb) s_mpvq[i] = LC3T_MPVQ_OFFSETS[i / 11][i % 11];
        for (int i = tid; i < LC3_TNS_MODEL_WORDS; i += fpb) s_tns[i] = lc3_tns_model_word(i);
        const uint16_t *ifs = lc3_band_index(cfg);
        for (int i = tid; i <= cfg.nb; i += fpb) s_ifs[i] = ifs[i];
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
        uint8_t *s = s_bytes + tid * nbytes;
        int k = 0;
        for (; k + 4 <= nbytes; k += 4) {
            uint32_t w;
            __builtin_memcpy(&w, g + k, 4);
            __builtin_memcpy(s + k, &w, 4);
        }
        for (; k < nbytes; k++) s[k] = g[k];
    }
    __syncthreads();
    int ok = 0;
    float e = -1.0f;
    int32_t *col = col0 + (size_t)tid * (size_t)LC3_PLANE_WORDS;
    if (tid < nfr && !flagged) {  // (a lane without a frame, or with a flagged one, stays out of the whole walk: the wave votes are among the lanes inside)
        lc3_parse_ctx c;
        c.dbg = nullptr;
        c.bytes = s_bytes + tid * nbytes;
        c.len = nbytes;
        c.lookup = s_lookup;
        c.cf = s_cf;
        c.tns = s_tns;
        c.plane = col;
        c.stride = LC3_PLANE_STRIDE;
        lc3_recon_ctx r;
        r.scf = s_scf + tid;
        r.sstride = fpb;
        r.mpvq = s_mpvq;
        r.ifs = s_ifs;
        float got = 0.0f;
        ok = lc3_analyze_frame(c, r, cfg, bands != nullptr, got);
        e = ok ? got : -1.0f;
    }
    if (tid < nfr) {  // the lane's own float and rows: a frame the decoder would conceal leaves -1 and zeros
        const lc3_i4 zero = {0, 0, 0, 0};  // (four 0.0f; the builtin vector stays in registers)
        const uint64_t dst = s_dst[tid];
        if (energy) energy[dst] = e;
        if (spec) {
            lc3_i4 *o = (lc3_i4 *)(spec + dst * LC3_AV_SPEC_LINES);
            const lc3_i4 *x4 = (const lc3_i4 *)(col + LC3_PLANE_X);
            for (int q = 0; q < LC3_AV_SPEC_LINES / 4; q++) o[q] = (ok && 4 * q < cfg.ne) ? x4[q] : zero;
        }
        if (bands) {
            float *o = bands + dst * LC3_AV_BANDS;
            if ((((uintptr_t)bands) & 15u) == 0) {  // (uniform; a row is 256 bytes)
                const lc3_i4 *e4 = (const lc3_i4 *)(col + LC3_PLANE_LEV);
                for (int q = 0; q < LC3_AV_BANDS / 4; q++) ((lc3_i4 *)o)[q] = ok ? e4[q] : zero;
            } else {
                const float *eb = (const float *)(col + LC3_PLANE_LEV);
                for (int q = 0; q < LC3_AV_BANDS; q++) o[q] = ok ? eb[q] : 0.0f;
            }
        }
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
#include "lc3_host_ring.h"

struct lc3gpu_analyzer {
    int max_views = 0, max_frames = 0;
    std::vector<lc3_iv_stream> streams;
    lc3_iv_plan plan;
    // the scratch columns: max_frames of LC3_PLANE_WORDS words, shared by every call of this analyzer
    int32_t *d_columns = nullptr;
    // a call's view rows, then its bucket rows, uploaded through the ring (lc3_host_ring.h); ordered: on another stream than the previous
    // call's, a call waits for it on the device, since both kernels write the same columns
    lc3_host_ring ring;
};

extern "C" {
int lc3ana_destroy(lc3gpu_analyzer *p) {
    if (!p) return LC3GPU_EINVAL;
    OnDevice on(p->ring.device);
    lc3_ring_destroy(p->ring);
    if (p->d_columns) (void)hipFree(p->d_columns);
    delete p;
    return LC3GPU_OK;
}

int lc3ana_create(lc3gpu_analyzer **out, int n_streams, const lc3gpu_stream_desc *descs, int max_views, int max_frames) {
    if (!out) return LC3GPU_EINVAL;
    *out = nullptr;
    if (!descs || n_streams < 1 || max_views < 1 || max_frames < 1) return LC3GPU_EINVAL;
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
    lc3gpu_analyzer *p = new (std::nothrow) lc3gpu_analyzer;
    if (!p) return LC3GPU_EHIP;
    p->streams.swap(streams);
    p->max_views = max_views;
    p->max_frames = max_frames;
    const size_t max_buckets = (size_t)(max_views < LC3_IV_CONFIGS * LC3_IV_MAX_NBYTES ? max_views : LC3_IV_CONFIGS * LC3_IV_MAX_NBYTES);
    hipError_t e = lc3_ring_create(p->ring, (size_t)max_views * sizeof(lc3_iv_row) + max_buckets * sizeof(lc3_iv_bucket));
    if (e == hipSuccess) e = hipMalloc((void **)&p->d_columns, (size_t)max_frames * LC3_PLANE_WORDS * sizeof(int32_t));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        (void)lc3ana_destroy(p);
        return LC3GPU_EHIP;
    }
    *out = p;
    return LC3GPU_OK;
}

int lc3ana_mixed_views(lc3gpu_analyzer *p, const lc3gpu_view *views, int n_views, const uint8_t *d_in, size_t in_bytes,
                       const uint8_t *d_bad_frame, size_t n_flags, float *d_energy, size_t n_energy, float *d_bands, size_t n_bands,
                       float *d_spec, size_t n_spec, void *hip_stream) {
    static_assert(sizeof(lc3gpu_view) == sizeof(lc3_iview), "lc3_iview is lc3gpu_view");
    if (!p) return LC3GPU_EINVAL;
    lc3_av_bounds B;
    B.in_base = (uint64_t)(uintptr_t)d_in;
    B.in_bytes = (uint64_t)in_bytes;
    B.flags_base = (uint64_t)(uintptr_t)d_bad_frame;
    B.n_flags = (uint64_t)n_flags;
    B.energy_base = (uint64_t)(uintptr_t)d_energy;
    B.n_energy = (uint64_t)n_energy;
    B.bands_base = (uint64_t)(uintptr_t)d_bands;
    B.n_bands = (uint64_t)n_bands;
    B.spec_base = (uint64_t)(uintptr_t)d_spec;
    B.n_spec = (uint64_t)n_spec;
    B.use_flags = d_bad_frame != nullptr;
    B.use_energy = d_energy != nullptr;
    B.use_bands = d_bands != nullptr;
    B.use_spec = d_spec != nullptr;
    int frames = 0, max_nbytes = 0;
    const lc3_iview *v = (const lc3_iview *)views;
    const int rc = lc3_aviews_check(p->streams.data(), (int)p->streams.size(), p->max_views, p->max_frames, v, n_views, B, &frames, &max_nbytes);
    if (rc) return rc;
    if (n_views == 0) return LC3GPU_OK;
    OnDevice on(p->ring.device);
    const hipStream_t stream = (hipStream_t)hip_stream;
    uint8_t *h_slot, *d_slot;
    LC3_HIP_TRY(lc3_ring_acquire(p->ring, stream, true, h_slot, d_slot));
    lc3_iv_row *rows = (lc3_iv_row *)h_slot;
    const size_t rows_bytes = (size_t)n_views * sizeof(lc3_iv_row);
    lc3_iv_bucket *buckets = (lc3_iv_bucket *)(h_slot + rows_bytes);  // (at most one bucket per view)
    const unsigned fpb = lc3_av_fpb(max_nbytes);
    const size_t lds = lc3_av_lds_bytes(max_nbytes);
    lc3_iviews_build(p->streams.data(), v, n_views, (int)fpb, rows, buckets, p->plan);
    // one upload: the rows and, right behind them, the bucket rows
    const size_t buckets_bytes = (size_t)p->plan.n_buckets * sizeof(lc3_iv_bucket);
    LC3_HIP_TRY(hipMemcpyAsync(d_slot, rows, rows_bytes + buckets_bytes, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(lc3_analyze_views_kernel, dim3((unsigned)p->plan.n_wg), dim3(fpb), lds, stream, (const lc3_iv_row *)d_slot,
                       (const lc3_iv_bucket *)(d_slot + rows_bytes), p->plan.n_buckets, d_in, d_bad_frame, p->d_columns, d_energy, d_bands, d_spec);
    LC3_HIP_TRY(hipGetLastError());
    LC3_HIP_TRY(lc3_ring_commit(p->ring, stream));
    return LC3GPU_OK;
}

// tests and tools: the plan's figures for a frame size (frames per workgroup, dynamic LDS bytes), the ring's slots and the words of a
// frame's scratch column
int lc3ana_plan_info(int max_nbytes, int *fpb, size_t *lds_bytes, int *ring_slots, int *column_words) {
    if (max_nbytes < 1 || max_nbytes > LC3_IV_MAX_NBYTES) return LC3GPU_ELENGTH;
    if (fpb) *fpb = (int)lc3_av_fpb(max_nbytes);
    if (lds_bytes) *lds_bytes = lc3_av_lds_bytes(max_nbytes);
    if (ring_slots) *ring_slots = lc3_host_ring::slots;
    if (column_words) *column_words = LC3_PLANE_WORDS;
    return LC3GPU_OK;
}
}
