// lc3gpu_meter -- the entry points of the meter (include/lc3gpu.h: lc3gpu_meter_create, lc3gpu_meter_destroy, lc3gpu_meter_reset,
// lc3gpu_meter_reset_channels, lc3gpu_measure_mixed_views) in the main library.  Host code only: the meter's kernel, its channels' states
// and its upload ring live in the companion library (lc3gpu_meter.hip -> liblc3gpu_meter.so), which the main library links with an $ORIGIN
// run path.  The main library's own device code -- every kernel of lc3gpu.hip -- is therefore what it was before the meter existed.
#include "../../include/lc3gpu.h"

extern "C" {
// the companion library's entry points (lc3gpu_meter.hip)
int lc3mtr_create(lc3gpu_meter **out, int n_channels, const lc3gpu_meter_desc *descs, int max_views);
int lc3mtr_destroy(lc3gpu_meter *mt);
int lc3mtr_reset(lc3gpu_meter *mt);
int lc3mtr_reset_channels(lc3gpu_meter *mt, const int32_t *channels, int n);
int lc3mtr_mixed_views(lc3gpu_meter *mt, const lc3gpu_view *views, int n_views, const int16_t *d_pcm, size_t pcm_elems, uint8_t *d_active,
                       size_t n_active, lc3gpu_level *d_levels, size_t n_levels, void *hip_stream);

int lc3gpu_meter_create(lc3gpu_meter **out, int n_channels, const lc3gpu_meter_desc *descs, int max_views) {
    return lc3mtr_create(out, n_channels, descs, max_views);
}
int lc3gpu_meter_destroy(lc3gpu_meter *mt) { return lc3mtr_destroy(mt); }
int lc3gpu_meter_reset(lc3gpu_meter *mt) { return lc3mtr_reset(mt); }
int lc3gpu_meter_reset_channels(lc3gpu_meter *mt, const int32_t *channels, int n) { return lc3mtr_reset_channels(mt, channels, n); }
int lc3gpu_measure_mixed_views(lc3gpu_meter *mt, const lc3gpu_view *views, int n_views, const int16_t *d_pcm, size_t pcm_elems, uint8_t *d_active,
                               size_t n_active, lc3gpu_level *d_levels, size_t n_levels, void *hip_stream) {
    return lc3mtr_mixed_views(mt, views, n_views, d_pcm, pcm_elems, d_active, n_active, d_levels, n_levels, hip_stream);
}
}
