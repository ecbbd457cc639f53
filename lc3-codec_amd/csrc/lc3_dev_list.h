// Batch calls over a LIST of a handle's channels (lc3gpu_encode_list / lc3gpu_decode_list): the reference's caller decides per call which
// channel gets a frame (examples/encode.rs:97-115), so a tick of a many-stream server names a scattered subset of the handle's channels.
// The launch's stream s -- its PCM, its plane columns, its bytes: everything the lane-per-frame kernels see -- is item s of the caller's
// compact buffers; only the stream's carried STATE is found through the list: entry s = channel index | LC3_LIST_FRESH.  The wave-per-
// stream kernels of a list launch differ from their uniform twins in exactly these two things:
//   channel lookup       states[lc3_list_channel(entry)] instead of states[first_channel + s]: one scalar load per wave (the list is
//                        constant for the launch: read through the constant address space, bound by v_readfirstlane like the configuration);
//   per-stream freshness lc3_list_fresh(entry) instead of a launch-wide `fresh`: a channel reset by lc3gpu_*_reset_channels starts from the
//                        constructed state beside carried streams of the same workgroup, with no zero-frame launch in front.
// Barrier rule (front half): the gathered LTPF blocks (LC3_SERIAL_BEGIN/END) are the encoder's only workgroup barriers after the table
// staging, and the four streams of a workgroup may differ in freshness.  lc3_enc_state_init / lc3_enc_state_load hold wave-level fences
// only and the gathered blocks work on the streams' LDS alone, so the per-stream branch below holds no barrier and nothing after it
// branches on freshness (the MDCT history pointer is data, not control).
// Ring rule (synthesis): the post-filter's output ring is fetched lazily from the state blob (lc3_dec_lds::ring_loaded).  A fresh stream
// runs lc3_dec_state_init, which zeroes the wave's whole core -- ring, ltpf_active_prev, PLC count -- and marks the ring loaded and fully
// written: whatever the previous owner of the channel left in the blob (a filter that was on when the channel was reset) is never read
// and is overwritten at the end of the launch.  The ring flags live in the stream's own LDS, so a carried stream beside it is untouched.
// Included by lc3gpu.hip and by the CPU wave emulator (tests/emu/lc3_emu_list.cpp), which runs these bodies as they are.
#ifndef LC3_DEV_LIST_H_
#define LC3_DEV_LIST_H_

#define LC3_LIST_FRESH 0x80000000u

// entry s of the launch's list, the same for every lane of the wave (s is wave-uniform).  The handle's device copy of the list is written
// by a copy that precedes the launch in stream order and by nothing else: constant memory as far as the kernel is concerned
#if defined(__HIP_DEVICE_COMPILE__)
#define LC3_LIST_CONST(T) const __attribute__((address_space(4))) T *
#else
#define LC3_LIST_CONST(T) const T *
#endif
__device__ __forceinline__ int lc3_list_entry(const int32_t *channel_of, int s) {
    return LC3_UNIFORM_I32(((LC3_LIST_CONST(int32_t))channel_of)[s]);
}
__device__ __forceinline__ int lc3_list_channel(int entry) { return entry & 0x7fffffff; }
__device__ __forceinline__ int lc3_list_fresh(int entry) { return (int)((uint32_t)entry >> 31); }

// Analysis front half of stream s: pcm_s = the stream's n_frames frames (planar, compact), fbase = s * n_frames its first plane column.
// The caller has staged the workgroup's tables (the last workgroup barrier that is not a gathered block).
LC3_CFG_TEMPLATE __device__ __forceinline__ void lc3_list_front_stream(LC3_CFG_PARAM, lc3_enc_lds &L, int lane, lc3_enc_state *gst, int fresh,
                                                                      int valid, const int16_t *pcm_s, float *mid, int32_t *planes, size_t fbase,
                                                                      int nbytes, int n_frames, int spec_flags, int outline_ltpf) {
    LC3_CFG_BIND;
    const int nf = c.nf, z = c.z;
    if (lane == 0) L.spec_flags = spec_flags;
    if (LC3_UNIFORM_I32(fresh)) lc3_enc_state_init(L, lane, gst, valid);  // (wave-level fences only: see the barrier rule)
    else lc3_enc_state_load(L, lane, gst);
    for (int t = 0; t < n_frames; t++) {
        const size_t f = fbase + (size_t)t;
        int32_t *plane = valid ? LC3_PLANE_COL(planes, f, EP_WORDS) : nullptr;
        float *mcol = valid ? mid + f * (size_t)MP_WORDS : nullptr;
        const int16_t *frame = pcm_s + (size_t)t * (size_t)nf;
        const int16_t *hist = t > 0 ? frame - (size_t)(nf - z) : (fresh ? nullptr : gst->hist);
        // (the phase depends on t and n_frames alone, as in lc3_enc_front_body: workgroup-uniform)
        lc3_encode_front_wave(LC3_CFG_PASS, L, lane, frame, hist, gst, mcol, plane, LC3_PLANE_STRIDE, nbytes, nullptr, 1, 1,
                              (t % LC3_WG_WAVES) + (t + 2 < n_frames ? 0x100 : 0), outline_ltpf);
    }
    if (valid) lc3_enc_state_store(c, L, lane, gst, n_frames > 0 ? pcm_s + (size_t)(n_frames - 1) * (size_t)nf : nullptr, 1);
}

// Analysis back half of stream s (the front half of the same launch has stored or initialised the scalars: no freshness here)
LC3_CFG_TEMPLATE __device__ __forceinline__ void lc3_list_back_stream(LC3_CFG_PARAM, lc3_enc_lds &L, int lane, lc3_enc_state *gst, int valid,
                                                                     const float *mid, int32_t *planes, size_t fbase, int nbytes, int n_frames,
                                                                     int spec_flags) {
    LC3_CFG_BIND;
    if (lane == 0) L.spec_flags = spec_flags;
    lc3_enc_state_load(L, lane, gst);
    lc3_encode_back_stream(LC3_CFG_PASS, L, lane, mid, planes, fbase, n_frames, nbytes, valid, nullptr);
    if (valid) lc3_enc_state_store(c, L, lane, gst, nullptr);
}

// Synthesis of stream s: pcm_s = where the stream's n_frames frames go.  tables(): the kernel's hook that writes the workgroup's transform
// tables to LDS (it may hold a workgroup barrier: it runs for every wave, outside the per-stream branch).  late as lc3_decode_stream_wave.
LC3_CFG_TEMPLATE_AND(class TABLES = lc3_no_prologue)
__device__ __forceinline__ void lc3_list_synth_stream(LC3_CFG_PARAM, lc3_dec_lds &L, int lane, lc3_dec_state *gst, int fresh, int valid, int nbytes,
                                                      const int32_t *planes, size_t fbase, int n_frames, int16_t *pcm_s, int late,
                                                      TABLES tables = TABLES()) {
    LC3_CFG_BIND;
    lc3_i4 st_regs = {0, 0, 0, 0};
    if (!LC3_UNIFORM_I32(fresh)) st_regs = lc3_dec_state_issue(lane, gst);
    lc3_decode_stream_wave(LC3_CFG_PASS, L, lane, nbytes, planes, fbase, n_frames, gst, valid, pcm_s, (size_t)c.nf, 1, late, nullptr, 0,
                           [&]() {
                               tables();
                               if (LC3_UNIFORM_I32(fresh)) lc3_dec_state_init(L, lane, gst, valid);  // (see the ring rule)
                               else lc3_dec_state_commit(L, lane, st_regs);
                           },
                           fresh);
    if (valid) lc3_dec_state_store(c, L, lane, gst);
}

// ---- a stream that is one channel of C in WAV sample order (lc3gpu_*_mixed_mc_items) -----------------------------------------------------
// pcm_s = the channel's first sample; sample n of frame t is pcm_s[(t * nf + n) * stride], stride = C, the item's channel count, per-
// stream data read with the list entry.  stride == 1 is the planar stream above, on its 32-bit loads and stores; stride >= 2 takes the
// 16-bit path of lc3_enc_mdct / lc3_enc_state_store / lc3_dec_store_strided (a channel of several is 2-byte aligned only).
// Barrier rule: the four streams of a workgroup may differ in stride.  The stride selects between two load (store) sequences inside
// lc3_enc_mdct, lc3_enc_state_store and lc3_decode_frame_wave, none of which holds a workgroup barrier, and is otherwise an address
// factor: no gathered block, no table staging and no prologue hook depends on it.
LC3_CFG_TEMPLATE __device__ __forceinline__ void lc3_list_front_stream_mc(LC3_CFG_PARAM, lc3_enc_lds &L, int lane, lc3_enc_state *gst, int fresh,
                                                                         int valid, const int16_t *pcm_s, int stride, float *mid, int32_t *planes,
                                                                         size_t fbase, int nbytes, int n_frames, int spec_flags,
                                                                         int outline_ltpf) {
    LC3_CFG_BIND;
    const int nf = c.nf, z = c.z;
    if (lane == 0) L.spec_flags = spec_flags;
    if (LC3_UNIFORM_I32(fresh)) lc3_enc_state_init(L, lane, gst, valid);  // (wave-level fences only: see the barrier rule)
    else lc3_enc_state_load(L, lane, gst);
    for (int t = 0; t < n_frames; t++) {
        const size_t f = fbase + (size_t)t;
        int32_t *plane = valid ? LC3_PLANE_COL(planes, f, EP_WORDS) : nullptr;
        float *mcol = valid ? mid + f * (size_t)MP_WORDS : nullptr;
        const int16_t *frame = pcm_s + (size_t)t * (size_t)nf * (size_t)stride;
        // the history inside the call is the previous frame's tail at the channel's stride; the state blob's copy is planar
        const int16_t *hist = t > 0 ? frame - (size_t)(nf - z) * (size_t)stride : (fresh ? nullptr : gst->hist);
        lc3_encode_front_wave(LC3_CFG_PASS, L, lane, frame, hist, gst, mcol, plane, LC3_PLANE_STRIDE, nbytes, nullptr, stride, t > 0 ? stride : 1,
                              (t % LC3_WG_WAVES) + (t + 2 < n_frames ? 0x100 : 0), outline_ltpf);
    }
    if (valid)
        lc3_enc_state_store(c, L, lane, gst, n_frames > 0 ? pcm_s + (size_t)(n_frames - 1) * (size_t)nf * (size_t)stride : nullptr, stride);
}

LC3_CFG_TEMPLATE_AND(class TABLES = lc3_no_prologue)
__device__ __forceinline__ void lc3_list_synth_stream_mc(LC3_CFG_PARAM, lc3_dec_lds &L, int lane, lc3_dec_state *gst, int fresh, int valid,
                                                         int nbytes, const int32_t *planes, size_t fbase, int n_frames, int16_t *pcm_s, int stride,
                                                         int late, TABLES tables = TABLES()) {
    LC3_CFG_BIND;
    lc3_i4 st_regs = {0, 0, 0, 0};
    if (!LC3_UNIFORM_I32(fresh)) st_regs = lc3_dec_state_issue(lane, gst);
    lc3_decode_stream_wave(LC3_CFG_PASS, L, lane, nbytes, planes, fbase, n_frames, gst, valid, pcm_s, (size_t)c.nf * (size_t)stride, stride, late,
                           nullptr, 0,
                           [&]() {
                               tables();
                               if (LC3_UNIFORM_I32(fresh)) lc3_dec_state_init(L, lane, gst, valid);  // (see the ring rule)
                               else lc3_dec_state_commit(L, lane, st_regs);
                           },
                           fresh);
    if (valid) lc3_dec_state_store(c, L, lane, gst);
}

// ---- a stream whose frames lie where the caller says (lc3gpu_*_mixed_views) ---------------------------------------------------------------
// pcm_s = sample 0 of frame 0; sample n of frame t is pcm_s[t * pitch + n * stride]: stride as above, pitch >= nf * stride the elements
// from one frame to the next (ring slots, a capture buffer wider than the stream), both per-stream data read with the list entry and
// wave-uniform.  The frames of a stream need not be contiguous, so the MDCT history of frame t > 0 is taken from where frame t - 1 LIES:
// its samples z .. nf-1, at prev + z * stride -- not from frame - (nf - z) * stride, which is the gap in front of the frame.  Only a
// frame's own nf samples are read (written); what lies between the frames is never touched.
// Barrier rule: the four streams of a workgroup may differ in stride AND pitch.  The stride selects a load (store) sequence as above; the
// pitch is an address term of the frame pointer and nothing else: no gathered block, no table staging and no prologue hook depends on it.
// Ring rule: unchanged -- freshness and the ring flags are the stream's own, the pitch moves only where lc3_decode_frame_wave stores.
// stride == 1 keeps the 32-bit path: the host admits only even pcm_off and even pitch there, so every frame starts on a 4-byte boundary.
LC3_CFG_TEMPLATE __device__ __forceinline__ void lc3_list_front_stream_view(LC3_CFG_PARAM, lc3_enc_lds &L, int lane, lc3_enc_state *gst, int fresh,
                                                                           int valid, const int16_t *pcm_s, int stride, int pitch, float *mid,
                                                                           int32_t *planes, size_t fbase, int nbytes, int n_frames, int spec_flags,
                                                                           int outline_ltpf) {
    LC3_CFG_BIND;
    const int z = c.z;
    if (lane == 0) L.spec_flags = spec_flags;
    if (LC3_UNIFORM_I32(fresh)) lc3_enc_state_init(L, lane, gst, valid);  // (wave-level fences only: see the barrier rule)
    else lc3_enc_state_load(L, lane, gst);
    for (int t = 0; t < n_frames; t++) {
        const size_t f = fbase + (size_t)t;
        int32_t *plane = valid ? LC3_PLANE_COL(planes, f, EP_WORDS) : nullptr;
        float *mcol = valid ? mid + f * (size_t)MP_WORDS : nullptr;
        const int16_t *frame = pcm_s + (size_t)t * (size_t)pitch;
        // the history inside the call is the tail of the previous frame where that frame lies; the state blob's copy is planar
        const int16_t *hist =
            t > 0 ? pcm_s + (size_t)(t - 1) * (size_t)pitch + (size_t)z * (size_t)stride : (fresh ? nullptr : gst->hist);
        lc3_encode_front_wave(LC3_CFG_PASS, L, lane, frame, hist, gst, mcol, plane, LC3_PLANE_STRIDE, nbytes, nullptr, stride, t > 0 ? stride : 1,
                              (t % LC3_WG_WAVES) + (t + 2 < n_frames ? 0x100 : 0), outline_ltpf);
    }
    if (valid) lc3_enc_state_store(c, L, lane, gst, n_frames > 0 ? pcm_s + (size_t)(n_frames - 1) * (size_t)pitch : nullptr, stride);
}

LC3_CFG_TEMPLATE_AND(class TABLES = lc3_no_prologue)
__device__ __forceinline__ void lc3_list_synth_stream_view(LC3_CFG_PARAM, lc3_dec_lds &L, int lane, lc3_dec_state *gst, int fresh, int valid,
                                                           int nbytes, const int32_t *planes, size_t fbase, int n_frames, int16_t *pcm_s, int stride,
                                                           int pitch, int late, TABLES tables = TABLES()) {
    LC3_CFG_BIND;
    lc3_i4 st_regs = {0, 0, 0, 0};
    if (!LC3_UNIFORM_I32(fresh)) st_regs = lc3_dec_state_issue(lane, gst);
    lc3_decode_stream_wave(LC3_CFG_PASS, L, lane, nbytes, planes, fbase, n_frames, gst, valid, pcm_s, (size_t)pitch, stride, late, nullptr, 0,
                           [&]() {
                               tables();
                               if (LC3_UNIFORM_I32(fresh)) lc3_dec_state_init(L, lane, gst, valid);  // (see the ring rule)
                               else lc3_dec_state_commit(L, lane, st_regs);
                           },
                           fresh);
    if (valid) lc3_dec_state_store(c, L, lane, gst);
}

#endif  // LC3_DEV_LIST_H_
