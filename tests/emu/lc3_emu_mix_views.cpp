// TEST INFRASTRUCTURE -- lc3gpu_mix_mixed_views on the CPU: the shared check and plan header (lc3_host_mix_views.h over
// lc3_host_inspect_views.h, both included unchanged: what the companion library runs on the host, and the look-up its kernel makes in the
// uploaded tables) and the kernel's lane body (lc3_mix_pair, lc3_dev_mix.h) driven THROUGH the plan: workgroup by workgroup, lane by lane,
// every lane finding its bus and its pair the way the kernel's lane does.  Build: tests/test_emu_mix_views.py.
#include <cstdint>
#include <cstring>

#include "../../lc3-codec_amd/csrc/lc3_dev_mix.h"

namespace {
// descs int32[n][3] = (fs_hz, frame_us, nbytes) -> the mixer's streams, as lc3mix_create makes them; 0 or the create call's code
int make_streams(const int32_t *descs, int n, int max_views, std::vector<lc3_mx_stream> &out) {
    if (!descs || n < 1 || max_views < 1) return LC3_IV_EINVAL;
    out.resize((size_t)n);
    for (int i = 0; i < n; i++) {
        lc3_iv_stream c;
        if (lc3_iv_config(descs[3 * i + 1], descs[3 * i], c)) return LC3_IV_EINVAL;
        if (descs[3 * i + 2] < 1 || descs[3 * i + 2] > LC3_IV_MAX_NBYTES) return LC3_IV_ELENGTH;
        lc3_mx_make_stream(descs[3 * i + 1], descs[3 * i], out[(size_t)i]);
    }
    return 0;
}
struct Tables {
    std::vector<lc3_mx_row> rows_in, rows_out;
    std::vector<lc3_mx_bus> buses;
};
}  // namespace

extern "C" {
int lc3emu_mx_spw(void) { return LC3_MX_SPW; }
int lc3emu_mx_lanes(void) { return LC3_MX_LANES; }
int lc3emu_mx_nf(int frame_us, int fs_hz) { return lc3_mx_nf(frame_us, fs_hz); }
// s / nf by the row's multiplier
unsigned lc3emu_mx_div(int nf, unsigned s) { return lc3_mx_div(s, lc3_mx_magic(nf)); }

// bounds uint64[4] = in base, in elements, out base, out elements.  Only addresses: nothing is read.  out int32[2] = buses with outputs and
// workgroups of the plan (an accepted call with outputs is planned too)
int lc3emu_mx_check(const int32_t *descs, int n_streams, int max_views, const void *in_views, const void *ins, int n_in, const void *out_views,
                    const void *outs, int n_out, const uint64_t *bounds, int32_t *out) {
    std::vector<lc3_mx_stream> streams;
    int rc = make_streams(descs, n_streams, max_views, streams);
    if (rc) return rc;
    lc3_mx_bounds B = {bounds[0], bounds[1], bounds[2], bounds[3]};
    lc3_mx_plan P(max_views);
    rc = lc3_mviews_check(streams.data(), n_streams, max_views, (const lc3_iview *)in_views, (const lc3_mix_in_t *)ins, n_in,
                          (const lc3_iview *)out_views, (const lc3_mix_out_t *)outs, n_out, B, P);
    out[0] = out[1] = 0;
    if (rc || n_out == 0) return rc;
    Tables T;
    T.rows_in.resize((size_t)n_in + 1), T.rows_out.resize((size_t)n_out), T.buses.resize((size_t)n_out);
    lc3_mviews_build(streams.data(), (const lc3_iview *)in_views, (const lc3_mix_in_t *)ins, n_in, (const lc3_iview *)out_views,
                     (const lc3_mix_out_t *)outs, n_out, T.rows_in.data(), T.rows_out.data(), T.buses.data(), P);
    out[0] = P.n_buses;
    out[1] = P.n_wg;
    return rc;
}

// The whole call on host arrays: check, plan, then every workgroup's lanes with the kernel's lane body.  Returns the call's code; a refused
// call writes nothing.  hits (may be null): uint8[out_elems], incremented for every sample a lane's output row names -- what the coverage
// test reads; with hits given nothing is mixed and pcm_out is not written.  -1000: a lane would read or write outside the extents
int lc3emu_mx_run(const int32_t *descs, int n_streams, int max_views, const void *in_views, const void *ins, int n_in, const int16_t *pcm_in,
                  uint64_t in_elems, const void *out_views, const void *outs, int n_out, int16_t *pcm_out, uint64_t out_elems, uint8_t *hits) {
    std::vector<lc3_mx_stream> streams;
    int rc = make_streams(descs, n_streams, max_views, streams);
    if (rc) return rc;
    lc3_mx_bounds B = {(uint64_t)(uintptr_t)pcm_in, in_elems, (uint64_t)(uintptr_t)pcm_out, out_elems};
    lc3_mx_plan P(max_views);
    rc = lc3_mviews_check(streams.data(), n_streams, max_views, (const lc3_iview *)in_views, (const lc3_mix_in_t *)ins, n_in,
                          (const lc3_iview *)out_views, (const lc3_mix_out_t *)outs, n_out, B, P);
    if (rc || n_out == 0) {
        P.clear();
        return rc;
    }
    Tables T;
    T.rows_in.resize((size_t)n_in + 1), T.rows_out.resize((size_t)n_out), T.buses.resize((size_t)n_out);
    lc3_mviews_build(streams.data(), (const lc3_iview *)in_views, (const lc3_mix_in_t *)ins, n_in, (const lc3_iview *)out_views,
                     (const lc3_mix_out_t *)outs, n_out, T.rows_in.data(), T.rows_out.data(), T.buses.data(), P);
    for (int wg = 0; wg < P.n_wg; wg++) {
        const lc3_mx_bus &b = T.buses[(size_t)lc3_mx_find_bus(T.buses.data(), P.n_buses, wg)];
        for (int tid = 0; tid < LC3_MX_LANES; tid++) {
            const uint32_t s = (uint32_t)(wg - b.wg0) * (uint32_t)LC3_MX_SPW + 2u * (uint32_t)tid;
            if (s >= (uint32_t)b.S) continue;
            // where the lane body will go, looked at before it goes there
            for (int i = 0; i < b.n_in; i++) {
                const lc3_mx_row &r = T.rows_in[(size_t)(b.first_in + i)];
                const uint64_t at = lc3_mx_place(r, s);
                if (at >= in_elems || (uint64_t)r.stride >= in_elems - at || (b.planar && r.stride != 1)) return -1000;
            }
            for (int o = 0; o < b.n_out; o++) {
                const lc3_mx_row &r = T.rows_out[(size_t)(b.first_out + o)];
                const uint64_t at = lc3_mx_place(r, s);
                if (at >= out_elems || (uint64_t)r.stride >= out_elems - at || r.aux < -1 || r.aux >= b.n_in) return -1000;
                if (b.planar && r.stride != 1) return -1000;
                if (hits) hits[at]++, hits[at + (uint64_t)r.stride]++;
            }
            if (!hits) lc3_mix_bus_pair(b, T.rows_in.data(), T.rows_out.data(), pcm_in, pcm_out, s);
        }
    }
    return 0;
}
}
