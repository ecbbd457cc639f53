// lc3gpu_inspector -- the entry points of the inspector (include/lc3gpu.h: lc3gpu_inspector_create, lc3gpu_inspector_destroy,
// lc3gpu_inspect_mixed_views) in the main library.  Host code only: the inspector's kernel, its device tables and its upload ring live in
// the companion library (lc3gpu_inspector.hip -> liblc3gpu_inspector.so), which the main library links with an $ORIGIN run path.  The
// main library's own device code -- every kernel of lc3gpu.hip -- is therefore what it was before the inspector existed.
#include "../../include/lc3gpu.h"

extern "C" {
// the companion library's entry points (lc3gpu_inspector.hip)
int lc3insp_create(lc3gpu_inspector **out, int n_streams, const lc3gpu_stream_desc *descs, int max_views);
int lc3insp_destroy(lc3gpu_inspector *insp);
int lc3insp_mixed_views(lc3gpu_inspector *insp, const lc3gpu_view *views, int n_views, const uint8_t *d_in, size_t in_bytes,
                        const uint8_t *d_bad_frame, size_t n_flags, uint8_t *d_status, size_t n_status, lc3gpu_frame_info *d_info, size_t n_info,
                        void *hip_stream);

int lc3gpu_inspector_create(lc3gpu_inspector **out, int n_streams, const lc3gpu_stream_desc *descs, int max_views) {
    return lc3insp_create(out, n_streams, descs, max_views);
}
int lc3gpu_inspector_destroy(lc3gpu_inspector *insp) { return lc3insp_destroy(insp); }
int lc3gpu_inspect_mixed_views(lc3gpu_inspector *insp, const lc3gpu_view *views, int n_views, const uint8_t *d_in, size_t in_bytes,
                               const uint8_t *d_bad_frame, size_t n_flags, uint8_t *d_status, size_t n_status, lc3gpu_frame_info *d_info,
                               size_t n_info, void *hip_stream) {
    return lc3insp_mixed_views(insp, views, n_views, d_in, in_bytes, d_bad_frame, n_flags, d_status, n_status, d_info, n_info, hip_stream);
}
}
