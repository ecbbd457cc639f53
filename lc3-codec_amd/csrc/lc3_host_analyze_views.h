// Frame analysis over a list of views (lc3gpu_analyze_mixed_views, include/lc3gpu.h): what differs from the inspector's check and plan
// (lc3_host_inspect_views.h, included unchanged).  Pure C++ with no HIP call and no device header, shared by the companion library
// (lc3gpu_analyzer.hip) and by the CPU tests (tests/emu/lc3_emu_analyze_views.cpp, tests/emu/lc3_analyze_views_check_main.cpp).
//
// The views, the rows and buckets, the counting sort (lc3_iviews_build), the two bisections and the non-wrapping extent test
// (lc3_iv_inside) are the inspector's: a frame of a view has the same place and the same output index in both calls.  What is the
// analyzer's own:
//   - three outputs instead of two -- one float, a row of LC3_AV_BANDS floats and a row of LC3_AV_SPEC_LINES floats per output index --,
//     each checked against its own extent, its alignment and every other array's address range;
//   - a bound on the frames of one call (max_frames): every frame of a call owns one scratch column of LC3_AV_COLUMN_WORDS words, which
//     the parse writes its integers into and the reconstruction its lines, and the columns are allocated once, at creation;
//   - the LDS of a workgroup: the parser's tables plus the reconstruction's (MPVQ offsets, the bucket's band index table), and per frame
//     its 16 scale factors, the index of its outputs and its bytes.
#pragma once
#include "lc3_host_inspect_views.h"

#define LC3_AV_BANDS 64
#define LC3_AV_SPEC_LINES 400
#define LC3_AV_COLUMN_WORDS 648  // LC3_PLANE_WORDS (lc3_dev_dec_parse.h; lc3gpu_analyzer.hip asserts it)

// Frames per workgroup and dynamic LDS, by the rule of lc3_iv_fpb.  Fixed part: the parser's lookup (4096), the spectral model (64 rows of
// 20 words), the MPVQ offsets (16 x 11 words), the TNS models (152 words) and the band index table (144 bytes); per frame: its scale
// factors (16 floats), the index of its outputs (8) and its bytes.
#define LC3_AV_LDS_FIXED 10672
#define LC3_AV_LDS_PER_FRAME 72
LC3_IV_HD unsigned lc3_av_fpb(int max_nbytes) {
    unsigned fpb = 256u;
    while (fpb > 64u && LC3_AV_LDS_FIXED + (size_t)fpb * (size_t)(LC3_AV_LDS_PER_FRAME + max_nbytes) + 8 > 65536u) fpb >>= 1;
    return fpb;
}
LC3_IV_HD size_t lc3_av_lds_bytes(int max_nbytes) {
    return LC3_AV_LDS_FIXED + (size_t)lc3_av_fpb(max_nbytes) * (size_t)(LC3_AV_LDS_PER_FRAME + max_nbytes) + 8;
}
// number of bands of a configuration (common/config.rs:42-100: 60 at 8 kHz / 7.5 ms, 64 everywhere else)
LC3_IV_HD int lc3_av_bands(int fs_ind, int n_ms_10) { return (fs_ind == 0 && !n_ms_10) ? 60 : 64; }

// ---- host only -----------------------------------------------------------------------------------------------------------------------------
// the caller's arrays: base ADDRESSES (nothing is read) and extents in bytes, flags, floats, band rows and spectrum rows; an array that is
// not given has base 0 and is checked against nothing
struct lc3_av_bounds {
    uint64_t in_base, in_bytes;
    uint64_t flags_base, n_flags;
    uint64_t energy_base, n_energy;
    uint64_t bands_base, n_bands;
    uint64_t spec_base, n_spec;
    int use_flags, use_energy, use_bands, use_spec;
};
// n elements of `each` bytes as a byte length; a product beyond 2^64 is taken to the end of the address space
static inline uint64_t lc3_av_len(uint64_t n, uint64_t each) { return n > UINT64_MAX / each ? UINT64_MAX : n * each; }

// the checks of the arrays themselves (everything of the table in include/lc3gpu.h that does not look at a view)
static inline int lc3_aviews_check_arrays(const lc3_av_bounds &B) {
    if (B.in_base == 0) return LC3_IV_EINVAL;
    if (!B.use_energy && !B.use_bands && !B.use_spec) return LC3_IV_EINVAL;
    if (B.use_energy && (B.energy_base & 3u) != 0) return LC3_IV_EINVAL;
    if (B.use_bands && (B.bands_base & 3u) != 0) return LC3_IV_EINVAL;
    if (B.use_spec && (B.spec_base & 15u) != 0) return LC3_IV_EINVAL;
    const uint64_t base[3] = {B.energy_base, B.bands_base, B.spec_base};
    const uint64_t len[3] = {lc3_av_len(B.n_energy, 4), lc3_av_len(B.n_bands, 4 * LC3_AV_BANDS), lc3_av_len(B.n_spec, 4 * LC3_AV_SPEC_LINES)};
    const int use[3] = {B.use_energy, B.use_bands, B.use_spec};
    for (int a = 0; a < 3; a++) {
        if (!use[a]) continue;
        if (lc3_iv_ranges_overlap(base[a], len[a], B.in_base, B.in_bytes)) return LC3_IV_EINVAL;
        if (B.use_flags && lc3_iv_ranges_overlap(base[a], len[a], B.flags_base, B.n_flags)) return LC3_IV_EINVAL;
        for (int o = a + 1; o < 3; o++)
            if (use[o] && lc3_iv_ranges_overlap(base[a], len[a], base[o], len[o])) return LC3_IV_EINVAL;
    }
    return LC3_IV_OK;
}
// Every check of the call but `an` itself, in the inspector's order (lc3_iviews_check) with the frame bound behind the views.  views may be
// null only to be refused.  frames / max_nbytes: the call's total and its largest effective frame size.  Nothing is written but those two.
static inline int lc3_aviews_check(const lc3_iv_stream *streams, int n_streams, int max_views, int max_frames, const lc3_iview *views,
                                   int n_views, const lc3_av_bounds &B, int *frames, int *max_nbytes) {
    *frames = 0;
    *max_nbytes = 0;
    if (!views || n_views < 0) return LC3_IV_EINVAL;
    const int rc = lc3_aviews_check_arrays(B);
    if (rc) return rc;
    if (n_views > max_views) return LC3_IV_ELENGTH;
    uint64_t total = 0;
    int most = 0;
    for (int i = 0; i < n_views; i++) {
        const lc3_iview &v = views[i];
        if (v.channel < 0 || v.channel >= n_streams) return LC3_IV_ECHANNEL;
        if (v.n_frames < 1) return LC3_IV_ELENGTH;
        if (v.nbytes != 0 && (v.nbytes < 1 || v.nbytes > LC3_IV_MAX_NBYTES)) return LC3_IV_ELENGTH;
        if (v.reserved[0] != 0 || v.reserved[1] != 0 || v.reserved[2] != 0) return LC3_IV_EINVAL;
        if (v.byte_off < 0 || v.flag_off < 0) return LC3_IV_EINVAL;
        const int nb = v.nbytes ? v.nbytes : streams[v.channel].nbytes;
        if (v.byte_pitch != 0 && v.byte_pitch < nb) return LC3_IV_EINVAL;
        if (v.flag_pitch < 0) return LC3_IV_EINVAL;
        const int bp = v.byte_pitch ? v.byte_pitch : nb, fp = v.flag_pitch ? v.flag_pitch : 1;
        if (!lc3_iv_inside(v.byte_off, v.n_frames, bp, (uint64_t)(nb - 1), B.in_bytes)) return LC3_IV_ELENGTH;
        if (B.use_flags && !lc3_iv_inside(v.flag_off, v.n_frames, fp, 0, B.n_flags)) return LC3_IV_ELENGTH;
        if (B.use_energy && !lc3_iv_inside(v.flag_off, v.n_frames, fp, 0, B.n_energy)) return LC3_IV_ELENGTH;
        if (B.use_bands && !lc3_iv_inside(v.flag_off, v.n_frames, fp, 0, B.n_bands)) return LC3_IV_ELENGTH;
        if (B.use_spec && !lc3_iv_inside(v.flag_off, v.n_frames, fp, 0, B.n_spec)) return LC3_IV_ELENGTH;
        total += (uint64_t)v.n_frames;
        if (total > (uint64_t)0x7fffffff) return LC3_IV_ELENGTH;  // (frame numbers are 32-bit on the device)
        if (nb > most) most = nb;
    }
    if (total > (uint64_t)max_frames) return LC3_IV_ELENGTH;  // (a frame beyond max_frames has no scratch column)
    *frames = (int)total;
    *max_nbytes = most;
    return LC3_IV_OK;
}
