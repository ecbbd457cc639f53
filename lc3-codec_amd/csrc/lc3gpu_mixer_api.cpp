// lc3gpu_mixer -- the entry points of the mixer (include/lc3gpu.h: lc3gpu_mixer_create, lc3gpu_mixer_destroy, lc3gpu_mix_mixed_views) in
// the main library.  Host code only: the mixer's kernel and its upload ring live in the companion library (lc3gpu_mixer.hip ->
// liblc3gpu_mixer.so), which the main library links with an $ORIGIN run path.  The main library's own device code -- every kernel of
// lc3gpu.hip -- is therefore what it was before the mixer existed.
#include "../../include/lc3gpu.h"

extern "C" {
// the companion library's entry points (lc3gpu_mixer.hip)
int lc3mix_create(lc3gpu_mixer **out, int n_streams, const lc3gpu_stream_desc *descs, int max_views);
int lc3mix_destroy(lc3gpu_mixer *mx);
int lc3mix_mixed_views(lc3gpu_mixer *mx, const lc3gpu_view *in_views, const lc3gpu_mix_in *ins, int n_in, const int16_t *d_pcm_in,
                       size_t in_elems, const lc3gpu_view *out_views, const lc3gpu_mix_out *outs, int n_out, int16_t *d_pcm_out,
                       size_t out_elems, void *hip_stream);

int lc3gpu_mixer_create(lc3gpu_mixer **out, int n_streams, const lc3gpu_stream_desc *descs, int max_views) {
    return lc3mix_create(out, n_streams, descs, max_views);
}
int lc3gpu_mixer_destroy(lc3gpu_mixer *mx) { return lc3mix_destroy(mx); }
int lc3gpu_mix_mixed_views(lc3gpu_mixer *mx, const lc3gpu_view *in_views, const lc3gpu_mix_in *ins, int n_in, const int16_t *d_pcm_in,
                           size_t in_elems, const lc3gpu_view *out_views, const lc3gpu_mix_out *outs, int n_out, int16_t *d_pcm_out,
                           size_t out_elems, void *hip_stream) {
    return lc3mix_mixed_views(mx, in_views, ins, n_in, d_pcm_in, in_elems, out_views, outs, n_out, d_pcm_out, out_elems, hip_stream);
}
}
