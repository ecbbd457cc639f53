// The upload ring of the companion libraries (lc3-codec_amd/csrc/lc3_host_ring.h) against FAKE HIP calls: a stand-alone program.
//
// The ring is ordering and nothing else: when the host waits for a slot's event before it fills the slot again, when a call on another
// stream is queued behind the previous call's kernel, and what a call that fails leaves behind.  A GPU test that compares results after a
// wait passes with one of these missing almost every time (tests/hb/lc3_pipeline_hb_main.cpp says why).  Here the header itself is
// compiled with the host compiler and linked with fake definitions of the twelve hip* functions it calls: nothing executes, every call is
// logged, live allocations and events are counted, and the Nth call of one function can be told to fail.  The program never opens a GPU
// and is never loaded into Python; the CPU suite builds it with -fsanitize=address,undefined and runs it as a child process
// (tests/test_host_ring.py), once on the header as it is and once per mutant of it.
//
// The header comes from the include path (-I), so that a mutant's copy is what gets compiled.
#include <hip/hip_runtime_api.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#define LC3GPU_EHIP (-5)  // what LC3_HIP_TRY returns (include/lc3gpu.h)
#include "lc3_host_ring.h"

namespace {
enum Fn { GET_DEVICE, SET_DEVICE, HOST_MALLOC, MALLOC, HOST_FREE, FREE, EVENT_CREATE, EVENT_DESTROY, EVENT_SYNC, EVENT_RECORD, STREAM_WAIT, GET_LAST_ERROR, N_FN };
const char *const FN_NAME[N_FN] = {"hipGetDevice", "hipSetDevice", "hipHostMalloc", "hipMalloc", "hipHostFree", "hipFree", "hipEventCreateWithFlags",
                                   "hipEventDestroy", "hipEventSynchronize", "hipEventRecord", "hipStreamWaitEvent", "hipGetLastError"};
struct Call {
    Fn fn;
    const void *a, *b;  // the event / pointer, the stream
    long n;             // a size, a device or flags
};

struct Fake {
    std::vector<Call> log;
    std::set<void *> host, dev, events;  // live objects
    int device = 0;
    int count[N_FN] = {};
    int fail_fn = -1, fail_nth = 0;  // the fail_nth'th call (from 1) of fail_fn returns hipErrorUnknown and does nothing
    std::vector<std::string> errors;  // what the fakes themselves object to: a free of what is not live
} F;

void fake_error(const char *fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    F.errors.push_back(buf);
}

// logs the call; true when it is the one that has to fail
bool enter(Fn fn, const void *a = nullptr, const void *b = nullptr, long n = 0) {
    F.log.push_back({fn, a, b, n});
    return ++F.count[fn] == F.fail_nth && fn == F.fail_fn;
}

void release(std::set<void *> &live, void *p, const char *what) {
    if (!live.erase(p)) {
        fake_error("%s of %p, which is not live (freed twice, or never made)", what, p);
        return;
    }
    free(p);
}
}  // namespace

extern "C" {
hipError_t hipGetDevice(int *d) {
    if (enter(GET_DEVICE)) return hipErrorUnknown;
    *d = F.device;
    return hipSuccess;
}
hipError_t hipSetDevice(int d) {
    if (enter(SET_DEVICE, nullptr, nullptr, d)) return hipErrorUnknown;
    F.device = d;
    return hipSuccess;
}
hipError_t hipHostMalloc(void **p, size_t n, unsigned flags) {
    if (enter(HOST_MALLOC, nullptr, nullptr, (long)n)) return hipErrorUnknown;
    (void)flags;
    F.host.insert(*p = malloc(n));
    return hipSuccess;
}
hipError_t hipMalloc(void **p, size_t n) {
    if (enter(MALLOC, nullptr, nullptr, (long)n)) return hipErrorUnknown;
    F.dev.insert(*p = malloc(n));
    return hipSuccess;
}
hipError_t hipHostFree(void *p) {
    enter(HOST_FREE, p);
    release(F.host, p, "hipHostFree");
    return hipSuccess;
}
hipError_t hipFree(void *p) {
    enter(FREE, p);
    release(F.dev, p, "hipFree");
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned flags) {
    if (enter(EVENT_CREATE, nullptr, nullptr, (long)flags)) return hipErrorUnknown;
    void *p = malloc(1);
    F.events.insert(p);
    *e = (hipEvent_t)p;
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) {
    enter(EVENT_DESTROY, e);
    release(F.events, (void *)e, "hipEventDestroy");
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t e) {
    if (enter(EVENT_SYNC, e)) return hipErrorUnknown;
    if (!F.events.count((void *)e)) fake_error("hipEventSynchronize of %p, which is not live", (void *)e);
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) {
    if (enter(EVENT_RECORD, e, s)) return hipErrorUnknown;
    if (!F.events.count((void *)e)) fake_error("hipEventRecord of %p, which is not live", (void *)e);
    return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned flags) {
    if (enter(STREAM_WAIT, e, s, (long)flags)) return hipErrorUnknown;
    if (!F.events.count((void *)e)) fake_error("hipStreamWaitEvent for %p, which is not live", (void *)e);
    return hipSuccess;
}
hipError_t hipGetLastError(void) {
    enter(GET_LAST_ERROR);
    return hipSuccess;
}
}

namespace {
std::vector<std::string> failures;  // of the scenario that runs

void check(bool ok, const char *fmt, ...) {
    if (ok) return;
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    failures.push_back(buf);
}
#define CHECK(cond) check((cond), "line %d: %s", __LINE__, #cond)

hipStream_t stream(int k) { return (hipStream_t)(uintptr_t)(0x1000 + 0x100 * k); }
int calls(Fn fn) { return F.count[fn]; }
size_t live() { return F.host.size() + F.dev.size() + F.events.size(); }

// one call of a companion: acquire, (fill, upload, launch), commit.  -> the log index where the call began
size_t call(lc3_host_ring &r, hipStream_t s, bool ordered, uint8_t **h = nullptr, uint8_t **d = nullptr) {
    const size_t at = F.log.size();
    uint8_t *hs = nullptr, *ds = nullptr;
    CHECK(lc3_ring_acquire(r, s, ordered, hs, ds) == hipSuccess);
    if (hs) memset(hs, 0x5a, r.slot_bytes);  // (the whole slot is the caller's: the sanitizer sees a slot that is too small)
    if (ds) memset(ds, 0xa5, r.slot_bytes);
    CHECK(lc3_ring_commit(r, s) == hipSuccess);
    if (h) *h = hs;
    if (d) *d = ds;
    return at;
}

int try_macro(hipError_t e) {
    LC3_HIP_TRY(e);
    return 0;
}

void no_early_wait() {
    lc3_host_ring r;
    CHECK(lc3_ring_create(r, 48) == hipSuccess);
    CHECK(calls(HOST_MALLOC) == 1 && calls(MALLOC) == 1 && calls(EVENT_CREATE) == kRingSlots && kRingSlots == 8);
    for (const Call &c : F.log) {
        if (c.fn == HOST_MALLOC || c.fn == MALLOC) CHECK(c.n == 48 * kRingSlots);
        if (c.fn == EVENT_CREATE) CHECK(c.n == (long)hipEventDisableTiming);
    }
    uint8_t *h0 = nullptr, *d0 = nullptr, *h = nullptr, *d = nullptr;
    for (int k = 0; k < kRingSlots; k++) {
        call(r, stream(0), true, &h, &d);
        CHECK(h == r.h_ring + 48 * k && d == r.d_ring + 48 * k);
        if (k == 0) h0 = h, d0 = d;
        CHECK(r.recorded[k] && r.next == (k + 1) % kRingSlots && r.last_slot == k && r.last_stream == stream(0));
    }
    CHECK(calls(EVENT_SYNC) == 0 && calls(EVENT_RECORD) == kRingSlots);
    // the ninth: slot 0 again, its event synchronised once, before the pointers are handed out (the first thing acquire does)
    const size_t at = F.log.size();
    uint8_t *h9 = nullptr, *d9 = nullptr;
    CHECK(lc3_ring_acquire(r, stream(0), true, h9, d9) == hipSuccess);
    CHECK(F.log.size() == at + 1 && F.log[at].fn == EVENT_SYNC && F.log[at].a == r.done[0]);
    CHECK(h9 == h0 && d9 == d0);
    CHECK(lc3_ring_commit(r, stream(0)) == hipSuccess);
    CHECK(calls(EVENT_SYNC) == 1 && r.next == 1);
    for (size_t i = at; i < F.log.size(); i++)
        if (F.log[i].fn == EVENT_RECORD) CHECK(F.log[i].a == r.done[0] && F.log[i].b == stream(0));
    lc3_ring_destroy(r);
    CHECK(live() == 0);
}

void cross_stream(bool ordered) {
    lc3_host_ring r;
    CHECK(lc3_ring_create(r, 16) == hipSuccess);
    call(r, stream(0), ordered);
    call(r, stream(0), ordered);
    CHECK(calls(STREAM_WAIT) == 0);  // the first call has no previous one; the second is on its stream
    size_t at = call(r, stream(1), ordered);
    if (ordered) {  // one wait, for the previous call's event (slot 1), on the new stream, before anything else of the call
        CHECK(calls(STREAM_WAIT) == 1 && F.log[at].fn == STREAM_WAIT && F.log[at].a == r.done[1] && F.log[at].b == stream(1));
    } else {
        CHECK(calls(STREAM_WAIT) == 0);
    }
    call(r, stream(1), ordered);
    CHECK(calls(STREAM_WAIT) == (ordered ? 1 : 0));
    at = call(r, stream(0), ordered);  // back on the first
    if (ordered) {
        CHECK(calls(STREAM_WAIT) == 2 && F.log[at].fn == STREAM_WAIT && F.log[at].a == r.done[3] && F.log[at].b == stream(0));
    } else {
        CHECK(calls(STREAM_WAIT) == 0);
    }
    // the null stream is a stream like any other
    call(r, nullptr, ordered);
    CHECK(calls(STREAM_WAIT) == (ordered ? 3 : 0));
    CHECK(calls(EVENT_SYNC) == 0);
    // a wait that fails: the error is returned and the ring is what it was
    if (ordered) {
        F.fail_fn = STREAM_WAIT, F.fail_nth = 4;
        uint8_t *h = nullptr, *d = nullptr;
        const int next = r.next;
        CHECK(lc3_ring_acquire(r, stream(2), true, h, d) == hipErrorUnknown);
        CHECK(r.next == next && r.last_slot == next - 1 && r.last_stream == nullptr && calls(EVENT_RECORD) == next);
    }
    lc3_ring_destroy(r);
    CHECK(live() == 0);
}
void cross_stream_ordered() { cross_stream(true); }
void cross_stream_unordered() { cross_stream(false); }

void acquire_without_commit() {
    lc3_host_ring r;
    CHECK(lc3_ring_create(r, 16) == hipSuccess);
    call(r, stream(0), true);
    uint8_t *h1 = nullptr, *d1 = nullptr, *h2 = nullptr, *d2 = nullptr;
    CHECK(lc3_ring_acquire(r, stream(1), true, h1, d1) == hipSuccess);  // (the call then fails: its upload or its launch)
    CHECK(r.next == 1 && !r.recorded[1] && r.last_slot == 0 && r.last_stream == stream(0) && calls(EVENT_RECORD) == 1);
    CHECK(lc3_ring_acquire(r, stream(1), true, h2, d2) == hipSuccess);
    CHECK(h2 == h1 && d2 == d1 && h1 == r.h_ring + 16 && d1 == r.d_ring + 16);
    CHECK(r.next == 1 && !r.recorded[1] && r.last_slot == 0 && r.last_stream == stream(0) && calls(EVENT_RECORD) == 1);
    CHECK(calls(EVENT_SYNC) == 0);  // the slot was never marked: nothing to wait for
    CHECK(lc3_ring_commit(r, stream(1)) == hipSuccess);
    CHECK(r.next == 2 && r.recorded[1] && r.last_slot == 1 && r.last_stream == stream(1));
    lc3_ring_destroy(r);
    CHECK(live() == 0);
}

void commit_failing() {
    lc3_host_ring r;
    CHECK(lc3_ring_create(r, 16) == hipSuccess);
    call(r, stream(0), true);
    uint8_t *h = nullptr, *d = nullptr;
    CHECK(lc3_ring_acquire(r, stream(1), true, h, d) == hipSuccess);
    F.fail_fn = EVENT_RECORD, F.fail_nth = 2;
    CHECK(lc3_ring_commit(r, stream(1)) == hipErrorUnknown);
    CHECK(r.next == 1 && !r.recorded[1] && r.last_slot == 0 && r.last_stream == stream(0));
    // the next call takes slot 1 again and waits for nothing: no event of that slot lies behind a kernel
    call(r, stream(0), true);
    CHECK(calls(EVENT_SYNC) == 0 && r.next == 2 && r.recorded[1]);
    // round to slot 0, whose event was recorded: a synchronise that fails is returned, no pointer is handed out, the ring is what it was
    for (int k = 2; k < kRingSlots; k++) call(r, stream(0), true);
    CHECK(calls(EVENT_SYNC) == 0 && r.next == 0);
    F.fail_fn = EVENT_SYNC, F.fail_nth = 1;
    h = d = nullptr;
    CHECK(lc3_ring_acquire(r, stream(0), true, h, d) == hipErrorUnknown && !h && !d && r.next == 0 && r.last_slot == kRingSlots - 1);
    CHECK(calls(EVENT_SYNC) == 1 && F.log.back().fn == EVENT_SYNC && F.log.back().a == r.done[0]);
    // the try macro: the runtime's error is cleared and the unit's code returned
    const int cleared = calls(GET_LAST_ERROR);
    CHECK(try_macro(hipSuccess) == 0 && calls(GET_LAST_ERROR) == cleared);
    CHECK(try_macro(hipErrorUnknown) == LC3GPU_EHIP && calls(GET_LAST_ERROR) == cleared + 1);
    lc3_ring_destroy(r);
    CHECK(live() == 0);
}

void create_failing_at_each_step() {
    const struct {
        Fn fn;
        int nth;
    } steps[] = {{GET_DEVICE, 1}, {HOST_MALLOC, 1}, {MALLOC, 1}, {EVENT_CREATE, 1}, {EVENT_CREATE, 2}, {EVENT_CREATE, 3}, {EVENT_CREATE, 4},
                 {EVENT_CREATE, 5}, {EVENT_CREATE, 6}, {EVENT_CREATE, 7}, {EVENT_CREATE, 8}};
    for (const auto &s : steps) {
        F = Fake();
        F.fail_fn = s.fn, F.fail_nth = s.nth;
        lc3_host_ring r;
        check(lc3_ring_create(r, 32) == hipErrorUnknown, "%s #%d: the error is returned", FN_NAME[s.fn], s.nth);
        check(live() == 0, "%s #%d: %zu objects live after the failed create", FN_NAME[s.fn], s.nth, live());
        check(calls(EVENT_SYNC) == 0, "%s #%d: no event was recorded, none is waited for", FN_NAME[s.fn], s.nth);
        const size_t n = F.log.size();
        lc3_ring_destroy(r);  // harmless: frees nothing a second time
        for (size_t i = n; i < F.log.size(); i++)
            check(F.log[i].fn == GET_DEVICE || F.log[i].fn == SET_DEVICE, "%s #%d: destroy after the failed create calls %s", FN_NAME[s.fn], s.nth,
                  FN_NAME[F.log[i].fn]);
        lc3_ring_destroy(r);
        for (const std::string &e : F.errors) check(false, "%s #%d: %s", FN_NAME[s.fn], s.nth, e.c_str());
        F.errors.clear();
    }
}

void destroy() {
    lc3_host_ring r;
    CHECK(lc3_ring_create(r, 16) == hipSuccess);
    for (int k = 0; k < 3; k++) call(r, stream(k & 1), true);
    const size_t at = F.log.size();
    lc3_ring_destroy(r);
    // the three recorded events are waited for, each before it is destroyed; the five others are not
    int syncs = 0;
    for (size_t i = at; i < F.log.size(); i++) {
        if (F.log[i].fn != EVENT_SYNC) continue;
        syncs++;
        bool destroyed_before = false;
        for (size_t j = at; j < i; j++) destroyed_before |= F.log[j].fn == EVENT_DESTROY && F.log[j].a == F.log[i].a;
        CHECK(!destroyed_before);
    }
    CHECK(syncs == 3 && calls(EVENT_DESTROY) == kRingSlots && calls(FREE) == 1 && calls(HOST_FREE) == 1 && live() == 0);
    lc3_ring_destroy(r);  // twice is harmless
    CHECK(calls(EVENT_DESTROY) == kRingSlots && calls(FREE) == 1 && calls(HOST_FREE) == 1);
    lc3_host_ring never;  // and so is a ring that was never created
    lc3_ring_destroy(never);
    CHECK(calls(EVENT_DESTROY) == kRingSlots && calls(FREE) == 1 && calls(HOST_FREE) == 1);
}

void device_guard() {
    F.device = 3;
    lc3_host_ring r;
    CHECK(lc3_ring_create(r, 16) == hipSuccess && r.device == 3);
    {
        OnDevice on(r.device);  // the same device: looked up, not set
        CHECK(F.device == 3);
    }
    CHECK(calls(SET_DEVICE) == 0);
    F.device = 1;
    {
        OnDevice on(r.device);
        CHECK(F.device == 3 && calls(SET_DEVICE) == 1);
    }
    CHECK(F.device == 1 && calls(SET_DEVICE) == 2);
    // destroy works under the ring's device and leaves the caller's current
    const size_t at = F.log.size();
    lc3_ring_destroy(r);
    int dev_at_free = -1, d = 1;
    for (size_t i = at; i < F.log.size(); i++) {
        if (F.log[i].fn == SET_DEVICE) d = (int)F.log[i].n;
        if (F.log[i].fn == FREE) dev_at_free = d;
    }
    CHECK(dev_at_free == 3 && F.device == 1 && live() == 0);
}

const struct {
    const char *name;
    void (*run)();
} SCENARIOS[] = {{"no_early_wait", no_early_wait},
                 {"cross_stream_ordered", cross_stream_ordered},
                 {"cross_stream_unordered", cross_stream_unordered},
                 {"acquire_without_commit", acquire_without_commit},
                 {"commit_failing", commit_failing},
                 {"create_failing_at_each_step", create_failing_at_each_step},
                 {"destroy", destroy},
                 {"device_guard", device_guard}};
}  // namespace

int main() {
    int bad = 0, n = 0;
    for (const auto &s : SCENARIOS) {
        F = Fake();
        failures.clear();
        s.run();
        for (const std::string &e : F.errors) failures.push_back("the fakes: " + e);
        if (live()) failures.push_back("objects left live at the scenario's end");
        n++;
        if (failures.empty()) {
            printf("ok %s\n", s.name);
            continue;
        }
        bad++;
        for (const std::string &f : failures) printf("FAIL %s: %s\n", s.name, f.c_str());
    }
    if (bad) {
        printf("failed %d of %d scenarios\n", bad, n);
        return 1;
    }
    printf("ok %d scenarios\n", n);
    return 0;
}
