// lc3gpu_resampler -- the entry points of the resampler (include/lc3gpu.h: lc3gpu_resampler_create, lc3gpu_resampler_destroy,
// lc3gpu_resampler_reset, lc3gpu_resampler_reset_channels, lc3gpu_resample_mixed_views) in the main library.  Host code only: the
// resampler's kernel, its histories and its upload ring live in the companion library (lc3gpu_resampler.hip -> liblc3gpu_resampler.so),
// which the main library links with an $ORIGIN run path.  The main library's own device code -- every kernel of lc3gpu.hip -- is therefore
// what it was before the resampler existed.
#include "../../include/lc3gpu.h"

extern "C" {
// the companion library's entry points (lc3gpu_resampler.hip)
int lc3rs_create(lc3gpu_resampler **out, int n_channels, const lc3gpu_rate_desc *descs, int max_views);
int lc3rs_destroy(lc3gpu_resampler *rs);
int lc3rs_reset(lc3gpu_resampler *rs);
int lc3rs_reset_channels(lc3gpu_resampler *rs, const int32_t *channels, int n);
int lc3rs_mixed_views(lc3gpu_resampler *rs, const lc3gpu_view *in_views, const int16_t *d_pcm_in, size_t in_elems, const lc3gpu_view *out_views,
                      int16_t *d_pcm_out, size_t out_elems, int n_views, void *hip_stream);

int lc3gpu_resampler_create(lc3gpu_resampler **out, int n_channels, const lc3gpu_rate_desc *descs, int max_views) {
    return lc3rs_create(out, n_channels, descs, max_views);
}
int lc3gpu_resampler_destroy(lc3gpu_resampler *rs) { return lc3rs_destroy(rs); }
int lc3gpu_resampler_reset(lc3gpu_resampler *rs) { return lc3rs_reset(rs); }
int lc3gpu_resampler_reset_channels(lc3gpu_resampler *rs, const int32_t *channels, int n) { return lc3rs_reset_channels(rs, channels, n); }
int lc3gpu_resample_mixed_views(lc3gpu_resampler *rs, const lc3gpu_view *in_views, const int16_t *d_pcm_in, size_t in_elems,
                                const lc3gpu_view *out_views, int16_t *d_pcm_out, size_t out_elems, int n_views, void *hip_stream) {
    return lc3rs_mixed_views(rs, in_views, d_pcm_in, in_elems, out_views, d_pcm_out, out_elems, n_views, hip_stream);
}
}
