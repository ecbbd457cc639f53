// The ordering of lc3gpu_pipeline (lc3-codec_amd/csrc/lc3gpu_pipeline.cpp) against a happens-before model: a stand-alone program.
//
// The pipeline object is ordering and nothing else: which HIP stream a piece of work goes to, which event waits are queued between the
// streams, which of them the hipEventQuery shortcut drops.  A GPU test compares results after a wait, and a missing wait passes such a
// test almost every time (kernels usually finish in submission order anyway).  Here the pipeline's own object file is linked with FAKE
// definitions of the 13 hip* and 18 lc3gpu_* functions it calls: nothing executes, every call is logged as a node of a trace, and a
// checker computes happens-before over the trace.  The program never opens a GPU and is never loaded into Python; the CPU suite builds it
// with -fsanitize=address,undefined and runs it as a child process (tests/test_pipeline_hb.py), once on the source as it is and once per
// mutant of it.
//
// The model of the HIP runtime, each assumption with the sentence of the HIP API documentation (hip_runtime_api.h) it rests on:
//   A1  A stream is a FIFO queue: an operation starts after everything queued on the same stream before it has completed.
//       hipEventRecord: "Events which are recorded in a non-NULL stream will transition to from recording to "recorded" state when they
//       reach the head of the specified stream, after all previous commands in that stream have completed executing."
//   A2  hipEventRecord(e, s) snapshots the position of s at the time of the call; a later record of the same event replaces the snapshot.
//       "If hipEventRecord() has been previously called on this event, then this call will overwrite any existing state in event."
//   A3  hipStreamWaitEvent(s, e) captures e's latest record AT THE TIME OF THE CALL and orders the future work of s behind it.
//       "This function inserts a wait operation into the specified stream.  All future work submitted to stream will wait until event
//       reports completion before beginning execution."
//   A4  An event that was never recorded orders nothing: a wait for it is no edge, a query or a synchronise of it returns at once.
//       "If this function [hipEventRecord] is not called before use hipEventQuery() or hipEventSynchronize(), hipSuccess is returned,
//       meaning no pending event in the stream."
//   A5  hipEventSynchronize(e) returns when e's record and everything before it has completed: the host then KNOWS that.
//       "This function will block until the event is ready, waiting for all previous work in the stream specified when event was recorded
//       with hipEventRecord()."
//   A6  hipStreamSynchronize(s) likewise for everything queued on s.
//       "This command is host-synchronous : the host will block until all operations on the specified stream with its associated device
//       are completed."
//   A7  hipEventQuery(e) == hipSuccess is host knowledge of the same kind; hipErrorNotReady is no knowledge at all.
//       "This function will return hipSuccess if all commands in the appropriate stream (specified to hipEventRecord()) have completed.
//       If any execution has not completed, then hipErrorNotReady is returned."
//   A8  What the host knows to have completed happens-before everything the host queues afterwards (program order of the one host thread
//       that drives a pipeline; the pipeline's streams are hipStreamNonBlocking, so the NULL stream orders nothing).
// Happens-before is the closure of: stream order (A1), record-to-wait edges (A2, A3), host knowledge (A5 to A8).  It is kept as a vector
// clock per node: clock[s] = the last position of stream s that happens-before (or is) the node.
//
// What "the device" does between the calls is a policy:
//   none    nothing completes until the host synchronises: every needed wait must be queued
//   all     everything completes at once: the query shortcut drops every wait, and host knowledge alone must order the work
//   random  seeded random progress, stream by stream, that respects FIFO order and the queued waits
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <array>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/lc3gpu.h"

namespace {
constexpr int MAX_STREAMS = 48;
typedef std::array<int, MAX_STREAMS> Clock;
enum Policy { P_NONE = 0, P_ALL = 1, P_RANDOM = 2 };
const char *const POLICY_NAME[3] = {"none", "all", "random"};
enum Kind { K_OP = 0, K_RECORD = 1, K_WAIT = 2 };

struct Range {
    uintptr_t lo, hi;
    bool write;
};
struct Node {
    int stream = 0, pos = 0, kind = K_OP;
    int pred_stream = -1, pred_pos = 0;  // K_WAIT: the record it waits for
    Clock clock{};
    int owner = -1, group = -1, role = -1, call = -1;  // owner = the pipeline (>= 0) the work belongs to; -1 a caller's own operation
    std::vector<Range> mem;
    const char *what = "";
};
struct StreamTag {
    int id;
};
struct EventTag {
    int rec = -1;  // node of the latest record
};

struct World {
    Policy policy = P_NONE;
    uint64_t rng = 1, dev_rng = 1;  // the caller program's choices and the device's progress draw from generators of their own
    std::vector<std::unique_ptr<StreamTag>> streams;  // (identities outlive a scenario: the pipeline keeps its streams for the process)
    std::vector<std::vector<int>> on_stream;          // node ids per stream, in queue order
    std::vector<int> done;                            // per stream: the position up to which the device has completed
    Clock host{};                                     // what the host knows to have completed
    std::vector<Node> nodes;
    std::vector<int> mem_nodes;
    long n_waits = 0, n_queries = 0;
    std::vector<long> waits_on;  // hipStreamWaitEvent calls per stream
    int cur_owner = -1, cur_call = 0;
    bool failed = false;
    std::string why;
    long total_nodes = 0;
} W;

void fail(const char *fmt, ...) {
    if (W.failed) return;  // (the first violation of a run names it; what follows is usually its consequence)
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    W.failed = true;
    W.why = buf;
}
uint32_t rnd() {
    W.rng = W.rng * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(W.rng >> 33);
}
int rnd_n(int n) { return (int)(rnd() % (uint32_t)n); }
int dev_rnd_n(int n) {
    W.dev_rng = W.dev_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (int)((uint32_t)(W.dev_rng >> 33) % (uint32_t)n);
}
template <class T, size_t N>
T pick(const T (&a)[N]) {
    return a[rnd_n((int)N)];
}

int new_stream() {
    if ((int)W.streams.size() >= MAX_STREAMS) {
        fprintf(stderr, "the model has room for %d streams\n", MAX_STREAMS);
        exit(2);
    }
    W.streams.push_back(std::unique_ptr<StreamTag>(new StreamTag{(int)W.streams.size()}));
    W.on_stream.emplace_back();
    W.done.push_back(0);
    W.waits_on.push_back(0);
    return (int)W.streams.size() - 1;
}
hipStream_t stream_handle(int s) { return reinterpret_cast<hipStream_t>(W.streams[(size_t)s].get()); }
int stream_id(hipStream_t s) {
    if (!s) {
        fail("the NULL stream was used");
        return 0;
    }
    return reinterpret_cast<StreamTag *>(s)->id;
}
void world_reset(Policy policy, uint64_t seed) {
    W.total_nodes += (long)W.nodes.size();
    W.policy = policy;
    W.rng = seed * 2654435761ull + 12345;
    W.dev_rng = seed * 40503ull + 977;
    for (auto &v : W.on_stream) v.clear();
    std::fill(W.done.begin(), W.done.end(), 0);
    std::fill(W.waits_on.begin(), W.waits_on.end(), 0);
    W.host.fill(0);
    W.nodes.clear();
    W.mem_nodes.clear();
    W.n_waits = W.n_queries = 0;
    W.cur_owner = -1;
    W.cur_call = 0;
    W.failed = false;
    W.why.clear();
}
void clock_max(Clock &a, const Clock &b) {
    for (int i = 0; i < MAX_STREAMS; i++) a[(size_t)i] = std::max(a[(size_t)i], b[(size_t)i]);
}
bool hb_node(const Node &a, const Node &b) { return b.clock[(size_t)a.stream] >= a.pos; }
bool hb_host(const Node &a) { return W.host[(size_t)a.stream] >= a.pos; }
const Node &node_at(int s, int pos) { return W.nodes[(size_t)W.on_stream[(size_t)s][(size_t)pos - 1]]; }

// the device completes one more node of stream s if FIFO order and the node's wait allow it
bool device_step(int s) {
    if (W.done[(size_t)s] >= (int)W.on_stream[(size_t)s].size()) return false;
    const Node &n = node_at(s, W.done[(size_t)s] + 1);
    if (n.kind == K_WAIT && n.pred_stream >= 0 && W.done[(size_t)n.pred_stream] < n.pred_pos) return false;
    W.done[(size_t)s]++;
    return true;
}
void device_progress() {
    if (W.policy == P_ALL) {
        for (size_t s = 0; s < W.done.size(); s++) W.done[s] = (int)W.on_stream[s].size();
    } else if (W.policy == P_RANDOM) {
        for (int i = dev_rnd_n(6); i > 0; i--) device_step(dev_rnd_n((int)W.done.size()));
    }
}
// the host learns that `c` has completed (a synchronise that returned, a query that said so)
void host_learns(const Clock &c) {
    clock_max(W.host, c);
    for (size_t s = 0; s < W.done.size(); s++) W.done[s] = std::max(W.done[s], c[s]);
}

int add_node(int s, Node n) {
    n.stream = s;
    n.pos = (int)W.on_stream[(size_t)s].size() + 1;
    n.clock = W.host;  // A8
    if (n.pos > 1) clock_max(n.clock, node_at(s, n.pos - 1).clock);  // A1
    if (n.kind == K_WAIT && n.pred_stream >= 0) clock_max(n.clock, node_at(n.pred_stream, n.pred_pos).clock);  // A3
    n.clock[(size_t)s] = n.pos;
    n.call = W.cur_call;
    if (!n.mem.empty()) {
        // every two accesses to overlapping addresses, at least one of them a write, are ordered, and in submission order
        for (int id : W.mem_nodes) {
            const Node &a = W.nodes[(size_t)id];
            if (hb_node(a, n)) continue;
            for (const Range &x : a.mem)
                for (const Range &y : n.mem)
                    if ((x.write || y.write) && x.lo < y.hi && y.lo < x.hi) {
                        fail("race: %s (pipeline %d group %d, call %d, stream %d) and %s (pipeline %d group %d, call %d, stream %d) touch [%#zx, %#zx) unordered",
                             a.what, a.owner, a.group, a.call, a.stream, n.what, n.owner, n.group, n.call, s, (size_t)std::max(x.lo, y.lo),
                             (size_t)std::min(x.hi, y.hi));
                        break;
                    }
        }
        W.mem_nodes.push_back((int)W.nodes.size());
    }
    W.nodes.push_back(std::move(n));
    W.on_stream[(size_t)s].push_back((int)W.nodes.size() - 1);
    return (int)W.nodes.size() - 1;
}
}  // namespace

// ---- the fake HIP runtime: the 13 functions the pipeline calls -------------------------------------------------------------------------
extern "C" {
hipError_t hipGetDevice(int *d) {
    *d = 0;
    return hipSuccess;
}
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
hipError_t hipDeviceGetStreamPriorityRange(int *least, int *greatest) {
    *least = 1;
    *greatest = -1;
    return hipSuccess;
}
hipError_t hipStreamCreateWithPriority(hipStream_t *s, unsigned int, int) {
    *s = stream_handle(new_stream());
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t) { return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) {
    *e = reinterpret_cast<hipEvent_t>(new EventTag());
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) {
    delete reinterpret_cast<EventTag *>(e);
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) {
    device_progress();
    Node n;
    n.kind = K_RECORD;
    n.what = "record";
    reinterpret_cast<EventTag *>(e)->rec = add_node(stream_id(s), n);  // A2
    return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned int) {
    device_progress();
    W.n_waits++;
    W.waits_on[(size_t)stream_id(s)]++;
    Node n;
    n.kind = K_WAIT;
    n.what = "wait";
    const int rec = reinterpret_cast<EventTag *>(e)->rec;
    if (rec >= 0) {  // A3 (A4: a never-recorded event orders nothing)
        n.pred_stream = W.nodes[(size_t)rec].stream;
        n.pred_pos = W.nodes[(size_t)rec].pos;
    }
    add_node(stream_id(s), n);
    return hipSuccess;
}
hipError_t hipEventQuery(hipEvent_t e) {
    device_progress();
    W.n_queries++;
    const int rec = reinterpret_cast<EventTag *>(e)->rec;
    if (rec < 0) return hipSuccess;  // A4
    const Node &r = W.nodes[(size_t)rec];
    if (W.done[(size_t)r.stream] < r.pos) return hipErrorNotReady;
    host_learns(r.clock);  // A7
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t e) {
    device_progress();
    const int rec = reinterpret_cast<EventTag *>(e)->rec;
    if (rec >= 0) host_learns(W.nodes[(size_t)rec].clock);  // A5
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t s) {
    device_progress();
    const int id = stream_id(s);
    if (!W.on_stream[(size_t)id].empty()) host_learns(node_at(id, (int)W.on_stream[(size_t)id].size()).clock);  // A6
    return hipSuccess;
}
}  // extern "C"

// ---- the fake handles: the 18 lc3gpu_* functions the pipeline calls ---------------------------------------------------------------------
// A batch call logs ONE operation: its stream, the ranges it reads and writes, and the handle's state as a written resource.  A handle
// refuses every stream but the bound one, and carries the pair flag (LC3GPU_EPAIR once, nothing logged), as lc3gpu.hip's order_begin.
struct FakeHandle {
    bool is_enc = false;
    int n = 0, nf = 0;                   // uniform: channels, samples per frame
    bool mixed = false;
    size_t pcm_own = 0, bytes_own = 0;   // mixed: samples / bytes of one frame of every stream
    hipStream_t bound = nullptr;
    bool pair = false;
    int owner = -1, group = -1;
    long calls = 0;
};
struct lc3gpu_encoder : FakeHandle {};
struct lc3gpu_decoder : FakeHandle {};

namespace {
int g_enc_made = 0, g_dec_made = 0;  // per pipeline under construction: the group a new handle belongs to
std::vector<FakeHandle *> g_handles;

int fake_nf(int frame_us, int fs_hz) { return (fs_hz == 44100 ? 48000 : fs_hz) / 100 * (frame_us == 7500 ? 3 : 4) / 4; }
bool fake_cfg_ok(int frame_us, int fs_hz) {
    return (frame_us == 7500 || frame_us == 10000) && (fs_hz == 8000 || fs_hz == 16000 || fs_hz == 24000 || fs_hz == 32000 || fs_hz == 44100 || fs_hz == 48000);
}
template <class H>
int fake_create(H **out, bool is_enc, int n, int frame_us, int fs_hz, const lc3gpu_stream_desc *descs) {
    if (!out || n <= 0) return LC3GPU_EINVAL;
    H *h = new H();
    h->is_enc = is_enc;
    h->n = n;
    if (descs) {
        h->mixed = true;
        for (int i = 0; i < n; i++) {
            if (!fake_cfg_ok(descs[i].frame_us, descs[i].fs_hz) || descs[i].nbytes < 20 || descs[i].nbytes > 400) {
                delete h;
                return LC3GPU_EINVAL;
            }
            h->pcm_own += (size_t)fake_nf(descs[i].frame_us, descs[i].fs_hz);
            h->bytes_own += (size_t)descs[i].nbytes;
        }
    } else {
        if (!fake_cfg_ok(frame_us, fs_hz)) {
            delete h;
            return LC3GPU_EINVAL;
        }
        h->nf = fake_nf(frame_us, fs_hz);
    }
    h->owner = W.cur_owner;
    h->group = is_enc ? g_enc_made++ : g_dec_made++;
    g_handles.push_back(h);
    *out = h;
    return LC3GPU_OK;
}
int fake_destroy(FakeHandle *h) {
    g_handles.erase(std::remove(g_handles.begin(), g_handles.end(), h), g_handles.end());
    return LC3GPU_OK;
}
// one batch call: the refusals of the real call in its order (lc3gpu.hip: encode_launch / decode_launch, lc3gpu_encode_mixed /
// lc3gpu_decode_mixed -- null pointers, the kind of handle, the lengths with the ENCODER's 20..400 and the DECODER's 1..400 bytes per frame,
// the 4-byte alignment of planar PCM; then order_begin's pair flag and bound stream), then the log entry
int fake_batch(FakeHandle *h, const void *d_pcm, const void *d_bytes, const void *d_bad, int nbytes, int n_frames, void *hip_stream) {
    if (!h || !d_pcm || !d_bytes) return LC3GPU_EINVAL;
    if (h->mixed != (nbytes < 0)) return LC3GPU_EINVAL;
    if (n_frames <= 0) return LC3GPU_ELENGTH;
    if (!h->mixed && (nbytes < (h->is_enc ? 20 : 1) || nbytes > 400)) return LC3GPU_ELENGTH;
    if (((uintptr_t)d_pcm & 3u) != 0) return LC3GPU_EINVAL;
    if (h->pair) {
        h->pair = false;
        return LC3GPU_EPAIR;
    }
    if (!h->bound || (hipStream_t)hip_stream != h->bound) return LC3GPU_EINVAL;
    device_progress();
    const size_t pcm_len = 2 * (h->mixed ? h->pcm_own : (size_t)h->n * (size_t)h->nf) * (size_t)n_frames;
    const size_t bytes_len = (h->mixed ? h->bytes_own : (size_t)h->n * (size_t)nbytes) * (size_t)n_frames;
    Node n;
    n.owner = h->owner;
    n.group = h->group;
    n.role = h->is_enc ? 0 : 1;
    n.what = h->is_enc ? "encode" : "decode";
    n.mem.push_back(Range{(uintptr_t)d_pcm, (uintptr_t)d_pcm + pcm_len, !h->is_enc});
    n.mem.push_back(Range{(uintptr_t)d_bytes, (uintptr_t)d_bytes + bytes_len, h->is_enc});
    if (d_bad) n.mem.push_back(Range{(uintptr_t)d_bad, (uintptr_t)d_bad + (size_t)h->n * (size_t)n_frames, false});
    n.mem.push_back(Range{(uintptr_t)h, (uintptr_t)h + 1, true});  // the handle's state blobs and scratch planes
    add_node(stream_id((hipStream_t)hip_stream), n);
    h->calls++;
    return LC3GPU_OK;
}
}  // namespace

extern "C" {
int lc3gpu_device_count(void) { return 1; }
int lc3gpu_config(int frame_us, int fs_hz, int out[7]) {
    if (!fake_cfg_ok(frame_us, fs_hz)) return LC3GPU_EINVAL;
    for (int i = 0; i < 7; i++) out[i] = 0;
    out[5] = fake_nf(frame_us, fs_hz);
    return LC3GPU_OK;
}
int lc3gpu_encoder_create(lc3gpu_encoder **out, int n, int frame_us, int fs_hz) { return fake_create(out, true, n, frame_us, fs_hz, nullptr); }
int lc3gpu_decoder_create(lc3gpu_decoder **out, int n, int frame_us, int fs_hz) { return fake_create(out, false, n, frame_us, fs_hz, nullptr); }
int lc3gpu_encoder_create_mixed(lc3gpu_encoder **out, int n, const lc3gpu_stream_desc *d) { return d ? fake_create(out, true, n, 0, 0, d) : LC3GPU_EINVAL; }
int lc3gpu_decoder_create_mixed(lc3gpu_decoder **out, int n, const lc3gpu_stream_desc *d) { return d ? fake_create(out, false, n, 0, 0, d) : LC3GPU_EINVAL; }
int lc3gpu_encoder_destroy(lc3gpu_encoder *e) {
    fake_destroy(e);
    delete e;
    return LC3GPU_OK;
}
int lc3gpu_decoder_destroy(lc3gpu_decoder *d) {
    fake_destroy(d);
    delete d;
    return LC3GPU_OK;
}
int lc3gpu_encoder_bind_stream(lc3gpu_encoder *e, void *s, int bind) {
    e->bound = bind ? (hipStream_t)s : nullptr;
    return LC3GPU_OK;
}
int lc3gpu_decoder_bind_stream(lc3gpu_decoder *d, void *s, int bind) {
    d->bound = bind ? (hipStream_t)s : nullptr;
    return LC3GPU_OK;
}
int lc3gpu_encoder_reset(lc3gpu_encoder *e) { return e ? LC3GPU_OK : LC3GPU_EINVAL; }  // (a flag on the host: the next call starts afresh)
int lc3gpu_decoder_reset(lc3gpu_decoder *d) { return d ? LC3GPU_OK : LC3GPU_EINVAL; }
int lc3gpu_encoder_pair_pending(const lc3gpu_encoder *e) { return e ? (e->pair ? 1 : 0) : LC3GPU_EINVAL; }
int lc3gpu_decoder_pair_pending(const lc3gpu_decoder *d) { return d ? (d->pair ? 1 : 0) : LC3GPU_EINVAL; }
int lc3gpu_encode(lc3gpu_encoder *e, const int16_t *d_pcm, uint8_t *d_out, int nbytes, int n_frames, void *s) {
    return nbytes < 0 ? LC3GPU_ELENGTH : fake_batch(e, d_pcm, d_out, nullptr, nbytes, n_frames, s);
}
int lc3gpu_decode(lc3gpu_decoder *d, const uint8_t *d_in, const uint8_t *d_bad, int16_t *d_pcm, int nbytes, int n_frames, void *s) {
    return nbytes < 0 ? LC3GPU_ELENGTH : fake_batch(d, d_pcm, d_in, d_bad, nbytes, n_frames, s);
}
int lc3gpu_encode_mixed(lc3gpu_encoder *e, const int16_t *d_pcm, uint8_t *d_out, int n_frames, void *s) {
    return fake_batch(e, d_pcm, d_out, nullptr, -1, n_frames, s);
}
int lc3gpu_decode_mixed(lc3gpu_decoder *d, const uint8_t *d_in, const uint8_t *d_bad, int16_t *d_pcm, int n_frames, void *s) {
    return fake_batch(d, d_pcm, d_in, d_bad, -1, n_frames, s);
}
}  // extern "C"

// ---- a caller of the pipeline: always legal under the contract of include/lc3gpu.h -----------------------------------------------------
// Byte buffers are the pipeline's to order (that is its promise).  PCM buffers and everything a caller's own stream touches are the
// caller's: a producer or consumer on the caller's stream goes behind lc3gpu_pipeline_join, the pipeline call that touches what such an
// operation touched goes behind lc3gpu_pipeline_follow, an output buffer that is written again with another n_frames (the groups' slices
// move) or that an encoder has read (a transcoding chain) goes behind lc3gpu_pipeline_wait.
namespace {
enum { ENC = 1, DEC = 2, BOTH = 3 };
int g_caller_stream[2] = {-1, -1};  // one stream of the caller's per pipeline
int g_next_owner = 0;

struct Pipe {
    lc3gpu_pipeline *p = nullptr;
    int owner = 0, cs = 0;
    bool mixed = false;
    int S = 0, nf = 0, n_groups = 0;
    size_t pcm_frame = 0, bytes_frame = 0;  // samples per frame of all streams; mixed: bytes per frame of all streams
    std::vector<FakeHandle *> enc, dec;      // per group
    bool unseen[2] = {false, false};          // the caller's stream holds work the encoder / decoder streams have not been told to follow
    int out_nf[4] = {0, 0, 0, 0};             // the n_frames of the unwaited writes of every output buffer (0: none)
    bool out_read[4] = {false, false, false, false};  // an encoder in flight may read it
    int steps = 0;

    uintptr_t buf(int kind, int i) const { return 0x100000000000ull + ((uintptr_t)owner << 40) + ((uintptr_t)kind << 36) + ((uintptr_t)i << 31); }
    int16_t *pcm_in(int i) const { return (int16_t *)buf(1, i); }
    uint8_t *bytes(int i) const { return (uint8_t *)buf(2, i); }
    int16_t *pcm_out(int i) const { return (int16_t *)buf(3, i); }
    size_t pcm_len(int n_frames) const { return 2 * pcm_frame * (size_t)n_frames; }
    size_t bytes_len(int nbytes, int n_frames) const { return (mixed ? bytes_frame : (size_t)S * (size_t)nbytes) * (size_t)n_frames; }

    void collect() {
        owner = W.cur_owner;
        cs = g_caller_stream[owner & 1];
        n_groups = lc3gpu_pipeline_groups(p);
        int covered = 0;
        for (int g = 0; g < n_groups; g++) {
            int first = -1, n = 0;
            lc3gpu_encoder *e = nullptr;
            lc3gpu_decoder *d = nullptr;
            if (lc3gpu_pipeline_group(p, g, &first, &n, &e, &d) != LC3GPU_OK || first != covered || n <= 0 || !e || !d || e->n != n || d->n != n)
                fail("group %d of %d: the table is not a partition of the channels", g, n_groups);
            covered += n;
            enc.push_back(e);
            dec.push_back(d);
        }
        if (covered != S) fail("the groups hold %d of %d channels", covered, S);
    }
    static Pipe uniform(int S, int n_groups, int frame_us = 10000, int fs_hz = 48000) {
        Pipe q;
        W.cur_owner = g_next_owner++;
        g_enc_made = g_dec_made = 0;
        q.S = S;
        q.nf = fake_nf(frame_us, fs_hz);
        q.pcm_frame = (size_t)S * (size_t)q.nf;
        const int rc = lc3gpu_pipeline_create(&q.p, S, frame_us, fs_hz, n_groups);
        if (rc) fail("lc3gpu_pipeline_create(%d channels, %d groups) = %d", S, n_groups, rc);
        else q.collect();
        return q;
    }
    static Pipe mixed_of(const std::vector<lc3gpu_stream_desc> &descs, int n_groups, const std::vector<int> *group_first) {
        Pipe q;
        W.cur_owner = g_next_owner++;
        g_enc_made = g_dec_made = 0;
        q.mixed = true;
        q.S = (int)descs.size();
        for (const lc3gpu_stream_desc &d : descs) {
            q.pcm_frame += (size_t)fake_nf(d.frame_us, d.fs_hz);
            q.bytes_frame += (size_t)d.nbytes;
        }
        // (the arrays are exactly as long as the contract says: a read past them is the sanitizer's to report)
        std::unique_ptr<lc3gpu_stream_desc[]> d(new lc3gpu_stream_desc[descs.size()]);
        std::copy(descs.begin(), descs.end(), d.get());
        std::unique_ptr<int[]> gf;
        if (group_first) {
            gf.reset(new int[group_first->size()]);
            std::copy(group_first->begin(), group_first->end(), gf.get());
        }
        const int rc = lc3gpu_pipeline_create_mixed(&q.p, q.S, d.get(), n_groups, gf.get());
        if (rc) fail("lc3gpu_pipeline_create_mixed(%d streams, %d groups) = %d", q.S, n_groups, rc);
        else q.collect();
        return q;
    }
    void close() {
        if (p) lc3gpu_pipeline_destroy(p);
        p = nullptr;
    }

    // a caller's own operation on its stream
    void caller_op(const char *what, uintptr_t lo, size_t len, bool write) {
        device_progress();
        Node n;
        n.what = what;
        n.mem.push_back(Range{lo, lo + len, write});
        add_node(cs, n);
        unseen[0] = unseen[1] = true;
    }
    bool mine(const Node &n) const { return n.owner == owner && n.kind == K_OP; }

    // one pipeline call with what the contract asks of the caller around it; `expect` the return code
    void call(int what, const int16_t *in, uint8_t *by, int16_t *out, int out_i, int nbytes, int n_frames, const uint8_t *bad = nullptr) {
        if (!p) return;
        if ((what & DEC) && out_i >= 0 && ((out_nf[out_i] && out_nf[out_i] != n_frames) || out_read[out_i])) wait();
        if (((what & ENC) && unseen[0]) || ((what & DEC) && unseen[1])) follow();
        bool flagged = false;
        for (int g = 0; g < n_groups; g++) flagged = flagged || ((what & ENC) && enc[(size_t)g]->pair) || ((what & DEC) && dec[(size_t)g]->pair);
        for (int attempt = 0; attempt < 1 + 2 * n_groups; attempt++) {
            W.cur_call++;
            const size_t nodes_before = W.nodes.size();
            int rc;
            if (mixed)
                rc = what == BOTH ? lc3gpu_pipeline_submit_mixed(p, in, by, out, n_frames)
                                  : what == ENC ? lc3gpu_pipeline_encode_mixed(p, in, by, n_frames) : lc3gpu_pipeline_decode_mixed(p, by, bad, out, n_frames);
            else
                rc = what == BOTH ? lc3gpu_pipeline_submit(p, in, by, out, nbytes, n_frames)
                                  : what == ENC ? lc3gpu_pipeline_encode(p, in, by, nbytes, n_frames) : lc3gpu_pipeline_decode(p, by, bad, out, nbytes, n_frames);
            if (rc == LC3GPU_EPAIR && flagged) {
                // "the call that returns it has launched nothing and may be repeated": nothing at all may have been queued
                if (W.nodes.size() != nodes_before) fail("a pipeline call that returned LC3GPU_EPAIR queued %zu operations", W.nodes.size() - nodes_before);
                continue;
            }
            if (rc) fail("pipeline call %d (what %d, nbytes %d, n_frames %d) = %d", W.cur_call, what, nbytes, n_frames, rc);
            break;
        }
        for (int g = 0; g < n_groups; g++)
            if (((what & ENC) && enc[(size_t)g]->pair) || ((what & DEC) && dec[(size_t)g]->pair)) fail("a raised pair flag of group %d survived the call", g);
        if (what & ENC) unseen[0] = false;
        if (what & DEC) unseen[1] = false;
        if ((what & DEC) && out_i >= 0) out_nf[out_i] = n_frames;
        steps++;
    }
    void submit(int in_i, int by_i, int out_i, int nbytes, int n_frames) { call(BOTH, pcm_in(in_i), bytes(by_i), pcm_out(out_i), out_i, nbytes, n_frames); }
    void encode(int in_i, int by_i, int nbytes, int n_frames) { call(ENC, pcm_in(in_i), bytes(by_i), nullptr, -1, nbytes, n_frames); }
    void decode(int by_i, int out_i, int nbytes, int n_frames, bool with_bad = false) {
        call(DEC, nullptr, bytes(by_i), pcm_out(out_i), out_i, nbytes, n_frames, with_bad ? (const uint8_t *)buf(4, 0) : nullptr);
    }
    void follow() {
        if (lc3gpu_pipeline_follow(p, stream_handle(cs))) fail("lc3gpu_pipeline_follow failed");
    }
    // after lc3gpu_pipeline_wait returns, every logged operation happens-before the host
    void wait() {
        if (!p) return;
        if (lc3gpu_pipeline_wait(p)) fail("lc3gpu_pipeline_wait failed");
        for (const Node &n : W.nodes)
            if (mine(n) && !hb_host(n)) {
                fail("after lc3gpu_pipeline_wait the %s of group %d (call %d) is not known to have completed", n.what, n.group, n.call);
                break;
            }
        for (int i = 0; i < 4; i++) {
            out_nf[i] = 0;
            out_read[i] = false;
        }
    }
    // after lc3gpu_pipeline_join(s), every logged operation happens-before the next operation on s
    void join_then(const char *what, uintptr_t lo, size_t len, bool write) {
        if (!p) return;
        if (lc3gpu_pipeline_join(p, stream_handle(cs))) fail("lc3gpu_pipeline_join failed");
        caller_op(what, lo, len, write);
        const Node &c = W.nodes.back();
        for (const Node &n : W.nodes)
            if (mine(n) && !hb_node(n, c)) {
                fail("after lc3gpu_pipeline_join the caller's %s does not follow the %s of group %d (call %d)", what, n.what, n.group, n.call);
                break;
            }
    }
    // after lc3gpu_pipeline_mark(e) and a host synchronise of e, every operation of the last group queued before the mark has completed
    void mark_and_sync() {
        if (!p) return;
        hipEvent_t e = nullptr;
        (void)hipEventCreateWithFlags(&e, 0);
        const size_t before = W.nodes.size();
        if (lc3gpu_pipeline_mark(p, e)) fail("lc3gpu_pipeline_mark failed");
        (void)hipEventSynchronize(e);
        for (size_t i = 0; i < before; i++) {
            const Node &n = W.nodes[i];
            if (mine(n) && n.group == n_groups - 1 && !hb_host(n)) {
                fail("the mark fired before the %s of the last group (call %d) was done", n.what, n.call);
                break;
            }
        }
        (void)hipEventDestroy(e);
    }
    void reset() {
        if (p && lc3gpu_pipeline_reset(p)) fail("lc3gpu_pipeline_reset failed");
    }
    void finish() {
        wait();
        close();
    }
};

long waits_of(const Pipe &q, int g, int role) {
    const FakeHandle *h = role == 0 ? q.enc[(size_t)g] : q.dec[(size_t)g];
    return W.waits_on[(size_t)stream_id(h->bound)];
}

// ---- scripted caller programs ---------------------------------------------------------------------------------------------------------
// The steady round trip with two alternating byte buffers, the benchmark's path.  Under "none" exactly one hipStreamWaitEvent and one
// hipEventQuery per role, group and submission (the comment above wait_for_other_role: "the encoder of submission k behind the decoder of
// k - 2, the decoder behind its own encoder"; the first two encoders have nothing to wait for); under "all" the same queries and no wait.
void steady(int S, int n_groups, int n_frames) {
    Pipe q = Pipe::uniform(S, n_groups);
    if (!q.p) return;
    for (int k = 0; k < 7; k++) {
        std::vector<long> w_enc, w_dec;
        for (int g = 0; g < q.n_groups; g++) {
            w_enc.push_back(waits_of(q, g, 0));
            w_dec.push_back(waits_of(q, g, 1));
        }
        const long q0 = W.n_queries;
        q.submit(0, k & 1, k & 1, 150, n_frames);
        const long enc_want = k >= 2 ? 1 : 0;
        if (W.n_queries - q0 != (enc_want + 1) * q.n_groups)
            fail("steady state: submission %d asked hipEventQuery %ld times, %d expected", k, W.n_queries - q0, (int)(enc_want + 1) * q.n_groups);
        if (W.policy == P_RANDOM) continue;
        for (int g = 0; g < q.n_groups; g++) {
            const long de = waits_of(q, g, 0) - w_enc[(size_t)g], dd = waits_of(q, g, 1) - w_dec[(size_t)g];
            const long we = W.policy == P_NONE ? enc_want : 0, wd = W.policy == P_NONE ? 1 : 0;
            if (de != we || dd != wd)
                fail("steady state: submission %d group %d queued %ld / %ld waits on its encoder / decoder stream, %ld / %ld expected", k, g, de, dd, we, wd);
        }
    }
    if (W.policy == P_ALL && W.n_waits != 0) fail("steady state: %ld waits queued although every event had completed", W.n_waits);
    q.finish();
}
void sc_steady_8() { steady(8, 2, 2); }
void sc_steady_8200() { steady(8200, 0, 4); }
void sc_steady_8_groups() { steady(64, 8, 1); }

void sc_one_byte_buffer() {
    Pipe q = Pipe::uniform(8, 2);
    for (int k = 0; k < 5; k++) q.submit(0, 0, k % 3, 150, 2);
    q.finish();
}
void sc_three_byte_buffers() {
    Pipe q = Pipe::uniform(8200, 2);
    for (int k = 0; k < 8; k++) q.submit(k & 1, k % 3, k % 4, 150, 4);
    q.finish();
}
void sc_four_byte_buffers() {
    Pipe q = Pipe::uniform(9, 3);
    for (int k = 0; k < 11; k++) q.submit(k & 1, k % 4, k % 4, 20, 1);
    q.finish();
}
void sc_halves_in_another_order() {
    Pipe q = Pipe::uniform(64, 3);
    for (int k = 0; k < 3; k++) q.encode(0, k, 150, 4);
    const int order[3] = {2, 0, 1};
    for (int k : order) q.decode(k, k, 150, 4, k == 0);
    for (int k = 0; k < 3; k++) q.encode(1, k, 150, 4);  // (every encoder overwrites what a decoder two or three calls back reads)
    q.finish();
}
void sc_encode_only_then_wait() {
    Pipe q = Pipe::uniform(8, 2);
    q.submit(0, 0, 0, 150, 2);
    q.encode(1, 1, 150, 2);
    q.wait();
    q.decode(1, 1, 150, 2);
    q.finish();
}
void sc_encode_only_then_join() {
    Pipe q = Pipe::uniform(8, 2);
    q.submit(0, 0, 0, 150, 2);
    q.encode(1, 1, 150, 2);
    q.join_then("copy of the bytes", (uintptr_t)q.bytes(1), q.bytes_len(150, 2), false);
    q.submit(0, 1, 1, 150, 2);  // (overwrites what the copy reads: behind a follow)
    q.join_then("copy of the PCM", (uintptr_t)q.pcm_out(1), q.pcm_len(2), false);
    q.finish();
}
void sc_bytes_arrive_on_a_caller_stream() {
    Pipe q = Pipe::uniform(8, 2);
    q.caller_op("upload of the bytes", (uintptr_t)q.bytes(0), q.bytes_len(150, 2), true);
    q.decode(0, 0, 150, 2);
    q.join_then("upload of the bytes", (uintptr_t)q.bytes(0), q.bytes_len(150, 2), true);
    q.decode(0, 1, 150, 2);
    q.finish();
}
void sc_pcm_arrives_on_a_caller_stream() {
    Pipe q = Pipe::uniform(5, 2);
    for (int k = 0; k < 4; k++) {
        q.join_then("upload of the PCM", (uintptr_t)q.pcm_in(2), q.pcm_len(2), true);
        if (k & 1) q.encode(2, k & 1, 150, 2);
        else q.submit(2, k & 1, 0, 150, 2);
    }
    q.finish();
}
void sc_marks() {
    Pipe q = Pipe::uniform(8, 2);
    q.submit(0, 0, 0, 150, 2);
    q.mark_and_sync();
    q.submit(0, 1, 1, 150, 2);
    q.encode(1, 2, 150, 2);  // the latest work is the encoder's
    q.mark_and_sync();
    q.encode(0, 0, 150, 2);
    q.decode(3, 2, 150, 2);  // bytes from elsewhere: the latest work is on both streams
    q.mark_and_sync();
    q.reset();
    q.finish();
    Pipe e = Pipe::uniform(4, 1);
    e.encode(0, 0, 150, 1);
    e.mark_and_sync();
    e.finish();
    Pipe d = Pipe::uniform(4, 1);
    d.decode(0, 0, 150, 1);
    d.mark_and_sync();
    d.finish();
}
// a group's slice of the byte buffer depends on n_frames and nbytes: group 1's encoder writes what group 0's decoder of the submission
// before reads, and the other way round
void sc_changing_geometry_one_buffer() {
    const int nfs[6] = {4, 2, 4, 1, 2, 4}, nbs[6] = {150, 150, 150, 150, 400, 20};
    for (int groups = 2; groups <= 3; groups++) {
        Pipe q = Pipe::uniform(12, groups);
        for (int k = 0; k < 6; k++) q.submit(0, 0, k % 4, nbs[k], nfs[k]);
        q.finish();
    }
}
void sc_changing_geometry_halves() {
    Pipe q = Pipe::uniform(8, 2);
    q.submit(0, 0, 0, 150, 4);
    q.decode(0, 1, 150, 2);  // another reading of the same bytes: group 1 reads what group 0's encoder wrote
    q.encode(0, 0, 150, 2);  // group 0 writes what group 1's decoder of the call before does not read, group 1 what group 0's does
    q.encode(0, 0, 400, 1);
    q.decode(0, 2, 400, 1);
    q.submit(1, 0, 3, 150, 4);
    q.finish();
}
void sc_shifted_views_of_one_allocation() {
    Pipe q = Pipe::uniform(8, 2);
    q.submit(0, 0, 0, 150, 2);
    q.call(ENC, q.pcm_in(0), q.bytes(0) + 150, nullptr, -1, 150, 2);  // one frame further: every slice overlaps its old self and its neighbour
    q.call(BOTH, q.pcm_in(0), q.bytes(0) + 4 * 2 * 150, q.pcm_out(1), 1, 150, 2);  // group 0 where group 1 was
    q.call(DEC, nullptr, q.bytes(0) + 150, q.pcm_out(2), 2, 150, 2);
    q.finish();
}
void sc_many_byte_buffers() {
    Pipe q = Pipe::uniform(8, 2);
    for (int k = 0; k < 14; k++) q.submit(0, k % 7, k % 4, 150, 2);
    // more buffers than the pipeline remembers, then a view into one of them, shifted by a group: group 0 where group 1 was three calls back
    q.call(BOTH, q.pcm_in(0), q.bytes(4) + 4 * 2 * 150, q.pcm_out(2), 2, 150, 2);
    q.finish();
}
void sc_pair_flags() {
    for (int role = 0; role < 2; role++)
        for (int g = 0; g < 3; g++) {
            Pipe q = Pipe::uniform(12, 3);
            if (!q.p) return;
            q.submit(0, 0, 0, 150, 2);
            (role == 0 ? q.enc : q.dec)[(size_t)g]->pair = true;
            q.submit(0, 1, 1, 150, 2);
            (role == 0 ? q.enc : q.dec)[(size_t)g]->pair = true;
            if (role == 0) q.encode(1, 0, 150, 2);
            else q.decode(1, 2, 150, 2);
            q.enc[0]->pair = q.dec[2]->pair = true;  // two flags: one refusal each
            q.submit(0, 0, 0, 150, 2);
            for (int h = 0; h < 3; h++)
                if (q.enc[(size_t)h]->calls != 3 + (role == 0) || q.dec[(size_t)h]->calls != 3 + (role == 1))
                    fail("group %d ran %ld encodes and %ld decodes", h, q.enc[(size_t)h]->calls, q.dec[(size_t)h]->calls);
            q.finish();
        }
}
std::vector<lc3gpu_stream_desc> some_descs(int n, bool sorted);
// arguments the handles would refuse -- some of them only group 0's decoder, after group 0's encoder has launched -- are refused before
// anything is queued; what a decoder takes and an encoder does not (nbytes 1..19) is taken by a decode alone
void sc_refused_arguments() {
    Pipe q = Pipe::uniform(8, 2);
    if (!q.p) return;
    q.submit(0, 0, 0, 150, 2);
    const size_t queued = W.nodes.size();
    int16_t *odd_in = (int16_t *)((uintptr_t)q.pcm_in(0) + 2), *odd_out = (int16_t *)((uintptr_t)q.pcm_out(1) + 2);
    const struct {
        int rc, want;
        const char *what;
    } refusals[] = {
        {lc3gpu_pipeline_submit(q.p, q.pcm_in(0), q.bytes(1), odd_out, 150, 2), LC3GPU_EINVAL, "submit with d_pcm_out 2-byte aligned"},
        {lc3gpu_pipeline_submit(q.p, odd_in, q.bytes(1), q.pcm_out(1), 150, 2), LC3GPU_EINVAL, "submit with d_pcm 2-byte aligned"},
        {lc3gpu_pipeline_decode(q.p, q.bytes(0), nullptr, odd_out, 150, 2), LC3GPU_EINVAL, "decode with d_pcm_out 2-byte aligned"},
        {lc3gpu_pipeline_encode(q.p, odd_in, q.bytes(1), 150, 2), LC3GPU_EINVAL, "encode with d_pcm 2-byte aligned"},
        {lc3gpu_pipeline_submit(q.p, q.pcm_in(0), q.bytes(1), q.pcm_out(1), 19, 2), LC3GPU_ELENGTH, "submit with nbytes 19"},
        {lc3gpu_pipeline_encode(q.p, q.pcm_in(0), q.bytes(1), 19, 2), LC3GPU_ELENGTH, "encode with nbytes 19"},
        {lc3gpu_pipeline_decode(q.p, q.bytes(0), nullptr, q.pcm_out(1), 0, 2), LC3GPU_ELENGTH, "decode with nbytes 0"},
        {lc3gpu_pipeline_submit(q.p, q.pcm_in(0), q.bytes(1), q.pcm_out(1), 401, 2), LC3GPU_ELENGTH, "submit with nbytes 401"},
        {lc3gpu_pipeline_submit(q.p, q.pcm_in(0), q.bytes(1), q.pcm_out(1), 150, 0), LC3GPU_ELENGTH, "submit with n_frames 0"},
        {lc3gpu_pipeline_submit_mixed(q.p, q.pcm_in(0), q.bytes(1), q.pcm_out(1), 2), LC3GPU_EINVAL, "submit_mixed on a uniform pipeline"},
    };
    for (const auto &r : refusals)
        if (r.rc != r.want) fail("%s = %d, %d expected", r.what, r.rc, r.want);
    for (int g = 0; g < q.n_groups; g++)
        if (q.enc[(size_t)g]->calls != 1 || q.dec[(size_t)g]->calls != 1) fail("a refused call reached the handles of group %d", g);
    if (W.nodes.size() != queued) fail("refused calls queued %zu operations, waits or records", W.nodes.size() - queued);
    q.decode(1, 1, 1, 2);   // (a decoder takes 1..400 bytes per frame)
    q.decode(1, 2, 19, 4);
    q.submit(0, 0, 0, 20, 2);
    q.finish();
    Pipe m = Pipe::mixed_of(some_descs(6, true), 2, nullptr);
    if (!m.p) return;
    const size_t queued_m = W.nodes.size();
    if (lc3gpu_pipeline_submit_mixed(m.p, m.pcm_in(0), m.bytes(0), (int16_t *)((uintptr_t)m.pcm_out(0) + 2), 2) != LC3GPU_EINVAL ||
        lc3gpu_pipeline_encode_mixed(m.p, (int16_t *)((uintptr_t)m.pcm_in(0) + 2), m.bytes(0), 2) != LC3GPU_EINVAL ||
        lc3gpu_pipeline_submit(m.p, m.pcm_in(0), m.bytes(0), m.pcm_out(0), 150, 2) != LC3GPU_EINVAL)
        fail("a mixed pipeline took arguments its handles refuse");
    if (W.nodes.size() != queued_m || m.enc[0]->calls || m.dec[0]->calls || m.enc[1]->calls || m.dec[1]->calls) fail("a refused call reached the handles of a mixed pipeline");
    m.submit(0, 0, 0, -1, 2);
    m.finish();
}
std::vector<lc3gpu_stream_desc> some_descs(int n, bool sorted) {
    const int fs[5] = {16000, 24000, 32000, 44100, 48000}, us[2] = {7500, 10000}, nb[3] = {20, 150, 400};
    std::vector<lc3gpu_stream_desc> d;
    for (int i = 0; i < n; i++) d.push_back(sorted ? lc3gpu_stream_desc{fs[i % 5], us[i % 2], nb[i % 3]} : lc3gpu_stream_desc{pick(fs), pick(us), pick(nb)});
    return d;
}
int create_mixed_rc(int n_streams, int n_groups, const std::vector<int> *gf) {
    std::vector<lc3gpu_stream_desc> descs = some_descs(n_streams, true);
    std::unique_ptr<lc3gpu_stream_desc[]> d(new lc3gpu_stream_desc[descs.size()]);
    std::copy(descs.begin(), descs.end(), d.get());
    std::unique_ptr<int[]> g;
    if (gf) {
        g.reset(new int[gf->size()]);
        std::copy(gf->begin(), gf->end(), g.get());
    }
    lc3gpu_pipeline *p = nullptr;
    W.cur_owner = g_next_owner++;
    g_enc_made = g_dec_made = 0;
    const int rc = lc3gpu_pipeline_create_mixed(&p, n_streams, d.get(), n_groups, g.get());
    if (p) lc3gpu_pipeline_destroy(p);
    return rc;
}
void sc_mixed_boundaries() {
    const std::vector<int> one = {0}, two = {0, 2}, five = {0, 1, 2, 3, 4}, bad = {0, 2, 2}, late = {1, 2};
    if (create_mixed_rc(4, 0, &one) != LC3GPU_EINVAL) fail("group_first with n_groups = 0 was not refused");
    if (create_mixed_rc(4, 5, &five) != LC3GPU_EINVAL) fail("group_first with n_groups > n_streams was not refused");
    if (create_mixed_rc(4, 3, &bad) != LC3GPU_EINVAL || create_mixed_rc(4, 2, &late) != LC3GPU_EINVAL) fail("boundaries that do not ascend from 0 were not refused");
    if (create_mixed_rc(4, 2, &two) != LC3GPU_OK || create_mixed_rc(4, 0, nullptr) != LC3GPU_OK || create_mixed_rc(3, 8, nullptr) != LC3GPU_OK ||
        create_mixed_rc(1, 1, &one) != LC3GPU_OK)
        fail("a legal mixed pipeline was refused");
}
void sc_mixed_round_trips() {
    const std::vector<int> gf = {0, 2, 3, 7};
    for (int given = 0; given < 2; given++) {
        Pipe q = Pipe::mixed_of(some_descs(9, true), given ? 4 : 3, given ? &gf : nullptr);
        const int nfs[6] = {2, 2, 4, 1, 4, 4};
        for (int k = 0; k < 6; k++) q.submit(0, k & 1, k % 3, -1, nfs[k]);
        q.encode(1, 0, -1, 2);
        q.mark_and_sync();
        q.decode(0, 0, -1, 2);
        q.join_then("copy of the PCM", (uintptr_t)q.pcm_out(0), q.pcm_len(2), false);
        q.finish();
    }
}
void sc_two_pipelines_share_the_streams() {
    Pipe a = Pipe::uniform(8, 2), b = Pipe::uniform(9, 3);
    for (int k = 0; k < 6; k++) {
        a.submit(0, k & 1, k & 1, 150, 2);
        b.submit(0, 0, k % 3, 400, k % 3 == 2 ? 1 : 4);
        if (k == 2) a.mark_and_sync();
        if (k == 3) b.join_then("copy of the PCM", (uintptr_t)b.pcm_out(0), b.pcm_len(4), false);
    }
    a.wait();
    b.encode(1, 1, 20, 2);
    b.finish();
    a.finish();
}
// d_pcm_out of one submission is d_pcm of the next: PCM is the caller's to order, with a wait or with join + follow
void sc_transcoding_chain() {
    Pipe q = Pipe::uniform(8, 2);
    q.submit(0, 0, 0, 150, 2);
    q.wait();
    q.call(BOTH, q.pcm_out(0), q.bytes(1), q.pcm_out(1), 1, 150, 2);
    q.join_then("nothing", (uintptr_t)q.buf(5, 0), 1, true);  // join + follow: the pipeline's next call is behind everything it holds now
    q.call(BOTH, q.pcm_out(1), q.bytes(0), q.pcm_out(2), 2, 150, 2);
    q.out_read[1] = true;
    q.submit(0, 1, 1, 150, 2);  // (writes what the encoder of the call before reads: the caller waits first)
    q.finish();
}

// ---- seeded random caller programs ----------------------------------------------------------------------------------------------------
Pipe random_pipe() {
    const int channels[8] = {1, 3, 4, 5, 8, 9, 64, 8200};
    if (rnd_n(3) == 0) {
        const int n = pick(channels);
        std::vector<lc3gpu_stream_desc> d = some_descs(n, false);
        if (rnd_n(2)) {
            const int groups = 1 + rnd_n(std::min(8, n));
            std::vector<int> gf = {0};  // `groups` ascending boundaries from 0
            while ((int)gf.size() < groups) {
                const int v = 1 + rnd_n(n - 1);
                if (std::find(gf.begin(), gf.end(), v) == gf.end()) gf.push_back(v);
            }
            std::sort(gf.begin(), gf.end());
            return Pipe::mixed_of(d, groups, &gf);
        }
        return Pipe::mixed_of(d, rnd_n(9), nullptr);
    }
    const int us[2] = {7500, 10000}, fs[3] = {16000, 44100, 48000};
    return Pipe::uniform(pick(channels), rnd_n(9), pick(us), pick(fs));
}
void sc_random() {
    const int nfs[3] = {1, 2, 4}, nbs[3] = {20, 150, 400};
    std::vector<Pipe> pipes;
    pipes.push_back(random_pipe());
    if (rnd_n(4) == 0) pipes.push_back(random_pipe());
    struct Plan {
        int n_bytes, n_out, nf, nb, k = 0;
        std::vector<int> enc_nf, enc_nb;  // per byte buffer: the geometry of its latest encode (0: none)
    };
    std::vector<Plan> plans;
    for (size_t i = 0; i < pipes.size(); i++) {
        Plan pl;
        pl.n_bytes = 1 + rnd_n(4);
        pl.n_out = 1 + rnd_n(3);
        pl.nf = pick(nfs);
        pl.nb = pick(nbs);
        pl.enc_nf.assign(4, 0);
        pl.enc_nb.assign(4, 0);
        plans.push_back(pl);
    }
    const int steps = 10 + rnd_n(25);
    const int change = rnd_n(3) == 0 ? 1000 : 2 + rnd_n(6);  // how often the geometry changes (some programs never change it)
    for (int step = 0; step < steps && !W.failed; step++) {
        const size_t i = (size_t)rnd_n((int)pipes.size());
        Pipe &q = pipes[i];
        Plan &pl = plans[i];
        if (!q.p) break;
        if (rnd_n(change) == 0) pl.nf = pick(nfs);
        if (rnd_n(change) == 0) pl.nb = pick(nbs);
        const int nb = q.mixed ? -1 : pl.nb, by = pl.k % pl.n_bytes, out = rnd_n(pl.n_out);
        const int act = rnd_n(100);
        if (act < 45) {
            q.submit(rnd_n(2), by, out, nb, pl.nf);
            pl.enc_nf[(size_t)by] = pl.nf;
            pl.enc_nb[(size_t)by] = nb;
            pl.k++;
        } else if (act < 57) {
            q.encode(rnd_n(2), by, nb, pl.nf);
            pl.enc_nf[(size_t)by] = pl.nf;
            pl.enc_nb[(size_t)by] = nb;
            pl.k++;
        } else if (act < 69) {  // a decode of an earlier encode, in another buffer order (or of bytes from elsewhere), read as they were written or otherwise
            const int b = rnd_n(pl.n_bytes);
            const bool as_written = pl.enc_nf[(size_t)b] && rnd_n(4) != 0;
            q.decode(b, out, as_written ? pl.enc_nb[(size_t)b] : nb, as_written ? pl.enc_nf[(size_t)b] : pl.nf, rnd_n(4) == 0);
        } else if (act < 75) {
            q.wait();
        } else if (act < 81) {
            if (rnd_n(2)) q.join_then("copy of the PCM", (uintptr_t)q.pcm_out(out), q.pcm_len(4), false);
            else q.join_then("copy of the bytes", (uintptr_t)q.bytes(by), q.bytes_len(400, 4), false);
        } else if (act < 87) {  // input that arrives on the caller's stream: PCM for an encode, bytes for a decode
            if (rnd_n(2)) {
                q.join_then("upload of the PCM", (uintptr_t)q.pcm_in(2), q.pcm_len(pl.nf), true);
                q.encode(2, by, nb, pl.nf);
                pl.enc_nf[(size_t)by] = pl.nf;
                pl.enc_nb[(size_t)by] = nb;
                pl.k++;
            } else {
                q.join_then("upload of the bytes", (uintptr_t)q.bytes(by), q.bytes_len(400, 4), true);
                q.decode(by, out, nb, pl.nf);
            }
        } else if (act < 92) {
            q.mark_and_sync();
        } else if (act < 95) {
            q.reset();
        } else {
            (rnd_n(2) ? q.enc : q.dec)[(size_t)rnd_n(q.n_groups)]->pair = true;
        }
    }
    for (Pipe &q : pipes) q.finish();
}

struct Scenario {
    const char *name;
    void (*fn)();
};
const Scenario SCRIPTED[] = {
    {"steady_two_buffers_8_channels", sc_steady_8},
    {"steady_two_buffers_8200_channels", sc_steady_8200},
    {"steady_two_buffers_8_groups", sc_steady_8_groups},
    {"one_byte_buffer", sc_one_byte_buffer},
    {"three_byte_buffers", sc_three_byte_buffers},
    {"four_byte_buffers", sc_four_byte_buffers},
    {"halves_in_another_order", sc_halves_in_another_order},
    {"encode_only_then_wait", sc_encode_only_then_wait},
    {"encode_only_then_join", sc_encode_only_then_join},
    {"bytes_arrive_on_a_caller_stream", sc_bytes_arrive_on_a_caller_stream},
    {"pcm_arrives_on_a_caller_stream", sc_pcm_arrives_on_a_caller_stream},
    {"marks", sc_marks},
    {"changing_geometry_one_buffer", sc_changing_geometry_one_buffer},
    {"changing_geometry_halves", sc_changing_geometry_halves},
    {"shifted_views_of_one_allocation", sc_shifted_views_of_one_allocation},
    {"many_byte_buffers", sc_many_byte_buffers},
    {"pair_flags", sc_pair_flags},
    {"refused_arguments", sc_refused_arguments},
    {"mixed_boundaries", sc_mixed_boundaries},
    {"mixed_round_trips", sc_mixed_round_trips},
    {"two_pipelines_share_the_streams", sc_two_pipelines_share_the_streams},
    {"transcoding_chain", sc_transcoding_chain},
};
}  // namespace

// usage: pipeline_hb [n_random_programs]
// prints one line per (scenario, policy) -- "ok" or "FAIL" and the first violation -- and a last line "ok <runs> <nodes>" or "failed <runs>";
// exit status 0 only if every run was clean
int main(int argc, char **argv) {
    const int n_random = argc > 1 ? atoi(argv[1]) : 150;
    g_caller_stream[0] = new_stream();
    g_caller_stream[1] = new_stream();
    int runs = 0, bad = 0;
    auto run = [&](const char *name, void (*fn)(), Policy pol, uint64_t seed) {
        world_reset(pol, seed);
        g_next_owner = 0;
        fn();
        if (!g_handles.empty()) fail("%zu handles outlive their pipelines", g_handles.size());
        runs++;
        if (W.failed) {
            bad++;
            printf("FAIL %s policy=%s: %s\n", name, POLICY_NAME[pol], W.why.c_str());
        } else printf("ok %s policy=%s nodes=%zu\n", name, POLICY_NAME[pol], W.nodes.size());
    };
    for (const Scenario &s : SCRIPTED)
        for (int pol = 0; pol < 3; pol++) run(s.name, s.fn, (Policy)pol, 7);
    for (int i = 0; i < n_random; i++)
        for (int pol = 0; pol < 3; pol++) {
            char name[32];
            snprintf(name, sizeof name, "random_%03d", i);
            run(name, sc_random, (Policy)pol, 1000 + (uint64_t)i);
        }
    world_reset(P_NONE, 0);
    if (bad) printf("failed %d of %d\n", bad, runs);
    else printf("ok %d %ld\n", runs, W.total_nodes);
    return bad ? 1 : 0;
}
