// lc3_host_ring -- the upload ring of the companion libraries: what stands between a pinned slot that a call fills again and the copy of
// an earlier call that may still be reading it.  Host only: no kernel, no device code, nothing of the codec; every companion includes it
// into its one unit, below its device code.
//
// A ring is kRingSlots slots of slot_bytes of pinned host memory, as many bytes of device memory each, and one event per slot that lies
// behind the kernel that read the slot last.  A call on a companion is
//
//     acquire      waits on the host for slot `next`'s event if one was recorded (it returns at once unless kRingSlots calls are still in
//                  flight), and, for an ORDERED ring, queues a device-side wait behind the previous call's kernel when the stream differs
//     ...          the companion fills the host slot, queues its one upload and its one launch on the stream
//     commit       records the slot's event on the stream, marks the slot, remembers stream and slot, advances `next`
//
// A call that fails between the two and does not commit leaves the ring as acquire found it: `next` not advanced, the slot not marked,
// last_stream / last_slot unchanged -- also where the upload was queued and the launch then failed.
//
// ordered: the companions that keep device-side state of their own between calls (scratch, histories, states) pass true -- two kernels
// of theirs on two streams touch the same memory; the stateless ones pass false and never wait across streams.
//
// Not thread-safe, as the objects that hold one.
#ifndef LC3_HOST_RING_H
#define LC3_HOST_RING_H

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

// a failed HIP call inside a C entry point: clear the runtime's last error and return LC3GPU_EHIP (the including unit's include/lc3gpu.h)
#define LC3_HIP_TRY(expr)                  \
    do {                                   \
        if ((expr) != hipSuccess) {        \
            (void)hipGetLastError();       \
            return LC3GPU_EHIP;            \
        }                                  \
    } while (0)

namespace {
// calls in flight before a call waits for the oldest of its own uploads
constexpr int kRingSlots = 8;

// makes an object's device current for the scope of a call
struct OnDevice {
    int prev = -1, dev;
    bool switched = false;
    explicit OnDevice(int d) : dev(d) {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) switched = hipSetDevice(dev) == hipSuccess;
    }
    ~OnDevice() {
        if (switched) (void)hipSetDevice(prev);
    }
};

struct lc3_host_ring {
    static constexpr int slots = kRingSlots;  // (what the owners' plan figures report)
    int device = 0;  // the device current at creation: the ring's, and its owner's
    size_t slot_bytes = 0;
    uint8_t *h_ring = nullptr, *d_ring = nullptr;
    hipEvent_t done[kRingSlots] = {};
    bool recorded[kRingSlots] = {};
    int next = 0;
    // the stream of the previous committed call and the slot whose event lies behind its kernel
    hipStream_t last_stream = nullptr;
    int last_slot = -1;
};

// under the ring's device: waits for the recorded events only, then frees everything.  Harmless on a ring that was never created, whose
// creation failed, or that was destroyed before.
inline void lc3_ring_destroy(lc3_host_ring &r) {
    OnDevice on(r.device);
    for (int k = 0; k < kRingSlots; k++) {
        if (!r.done[k]) continue;
        if (r.recorded[k]) (void)hipEventSynchronize(r.done[k]);
        (void)hipEventDestroy(r.done[k]);
        r.done[k] = nullptr;
        r.recorded[k] = false;
    }
    if (r.d_ring) (void)hipFree(r.d_ring);
    if (r.h_ring) (void)hipHostFree(r.h_ring);
    r.d_ring = r.h_ring = nullptr;
    r.last_slot = -1;
}

// on the current device, which becomes the ring's.  On a failure everything made so far is freed again and the ring stays destroyable.
inline hipError_t lc3_ring_create(lc3_host_ring &r, size_t slot_bytes) {
    r.slot_bytes = slot_bytes;
    hipError_t e = hipGetDevice(&r.device);
    if (e == hipSuccess) e = hipHostMalloc((void **)&r.h_ring, slot_bytes * kRingSlots, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc((void **)&r.d_ring, slot_bytes * kRingSlots);
    for (int k = 0; k < kRingSlots && e == hipSuccess; k++) e = hipEventCreateWithFlags(&r.done[k], hipEventDisableTiming);
    if (e != hipSuccess) lc3_ring_destroy(r);
    return e;
}

// slot `next`, safe to fill: h_slot and d_slot are its slot_bytes of pinned host and of device memory.  The slot is not advanced.
inline hipError_t lc3_ring_acquire(lc3_host_ring &r, hipStream_t stream, bool ordered, uint8_t *&h_slot, uint8_t *&d_slot) {
    const int k = r.next;
    if (r.recorded[k]) {  // (returns at once unless kRingSlots calls are still in flight)
        const hipError_t e = hipEventSynchronize(r.done[k]);
        if (e != hipSuccess) return e;
    }
    // the owner's device-side state is the object's, not the call's: on another stream than the previous call's, behind that call's kernel
    if (ordered && r.last_slot >= 0 && r.last_stream != stream) {
        const hipError_t e = hipStreamWaitEvent(stream, r.done[r.last_slot], 0);
        if (e != hipSuccess) return e;
    }
    h_slot = r.h_ring + (size_t)k * r.slot_bytes;
    d_slot = r.d_ring + (size_t)k * r.slot_bytes;
    return hipSuccess;
}

// behind the call's launch on `stream`: the acquired slot's event, then the bookkeeping -- none of it unless the record succeeded
inline hipError_t lc3_ring_commit(lc3_host_ring &r, hipStream_t stream) {
    const int k = r.next;
    const hipError_t e = hipEventRecord(r.done[k], stream);
    if (e != hipSuccess) return e;
    r.recorded[k] = true;
    r.last_stream = stream;
    r.last_slot = k;
    r.next = (k + 1) % kRingSlots;
    return hipSuccess;
}
}  // namespace

#endif
