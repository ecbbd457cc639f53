// lc3gpu_analyzer -- the entry points of the analyzer (include/lc3gpu.h: lc3gpu_analyzer_create, lc3gpu_analyzer_destroy,
// lc3gpu_analyze_mixed_views) in the main library.  Host code only: the analyzer's kernel, its device tables, its scratch columns and its
// upload ring live in the companion library (lc3gpu_analyzer.hip -> liblc3gpu_analyzer.so), which the main library links with an $ORIGIN
// run path.  The main library's own device code -- every kernel of lc3gpu.hip -- is therefore what it was before the analyzer existed.
#include "../../include/lc3gpu.h"

extern "C" {
// the companion library's entry points (lc3gpu_analyzer.hip)
int lc3ana_create(lc3gpu_analyzer **out, int n_streams, const lc3gpu_stream_desc *descs, int max_views, int max_frames);
int lc3ana_destroy(lc3gpu_analyzer *an);
int lc3ana_mixed_views(lc3gpu_analyzer *an, const lc3gpu_view *views, int n_views, const uint8_t *d_in, size_t in_bytes,
                       const uint8_t *d_bad_frame, size_t n_flags, float *d_energy, size_t n_energy, float *d_bands, size_t n_bands,
                       float *d_spec, size_t n_spec, void *hip_stream);

int lc3gpu_analyzer_create(lc3gpu_analyzer **out, int n_streams, const lc3gpu_stream_desc *descs, int max_views, int max_frames) {
    return lc3ana_create(out, n_streams, descs, max_views, max_frames);
}
int lc3gpu_analyzer_destroy(lc3gpu_analyzer *an) { return lc3ana_destroy(an); }
int lc3gpu_analyze_mixed_views(lc3gpu_analyzer *an, const lc3gpu_view *views, int n_views, const uint8_t *d_in, size_t in_bytes,
                               const uint8_t *d_bad_frame, size_t n_flags, float *d_energy, size_t n_energy, float *d_bands, size_t n_bands,
                               float *d_spec, size_t n_spec, void *hip_stream) {
    return lc3ana_mixed_views(an, views, n_views, d_in, in_bytes, d_bad_frame, n_flags, d_energy, n_energy, d_bands, n_bands, d_spec, n_spec,
                              hip_stream);
}
}
