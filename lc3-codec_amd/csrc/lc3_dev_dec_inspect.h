// Frame inspection (lc3gpu_inspect, include/lc3gpu.h): a frame's side information and decode status, ONE LANE PER FRAME.
//
// The decoder's parser (lc3_dev_dec_parse.h) decides whether a frame is concealed: it conceals exactly when the reference's read_frame
// returns Err (decoder/lc3_decoder.rs:138-141, 165-178).  This walk is that parser without its products: it decodes every symbol of the
// frame (which is what validates it, and what the residual-bit count, the noise-filling seed and the zero-frame flag depend on) with the
// same primitives, but keeps no spectrum -- no 648-word plane column, no reconstruction.  What the lsb-mode refinement walk needs of the
// spectrum is two bits per pair, kept in LDS.
//
// The fast path's checks are deferred and sticky, as the parser's are: it knows THAT the TNS or spectral data failed, not which check the
// reference meets first.  A frame it finds broken there is walked once more by lc3_inspect_classify, out of line, with every read checked
// in the reference's order: only failing frames pay for it.
#pragma once
#include "../../include/lc3gpu.h"
#include "lc3_dev_dec_parse.h"

// words of the record (lc3gpu_frame_info).  The side information is SI_* words 0 .. 19 in the parser's order, which is also the order of
// the reference's SideInfo fields (decoder/side_info.rs:20-31): the parser's side-information reader writes them in place.
enum {
    LC3_FI_STATUS = 0, LC3_FI_NBYTES = 1, LC3_FI_SI = 2, LC3_FI_RC_ORDER = LC3_FI_SI + SI_NF + 1, LC3_FI_NRES = LC3_FI_RC_ORDER + 2,
    LC3_FI_SEED, LC3_FI_ZERO, LC3_FI_RCI /* 16 bytes */, LC3_FI_RESERVED = LC3_FI_RCI + 4, LC3_FI_WORDS
};
static_assert(sizeof(lc3gpu_frame_info) == 4 * LC3_FI_WORDS, "lc3gpu_frame_info is 32 words");
static_assert(offsetof(lc3gpu_frame_info, bandwidth) == 4 * (LC3_FI_SI + SI_BW), "side information in SI_* order");
static_assert(offsetof(lc3gpu_frame_info, sns_ls_inda) == 4 * (LC3_FI_SI + SI_LS_A), "side information in SI_* order");
static_assert(offsetof(lc3gpu_frame_info, noise_factor) == 4 * (LC3_FI_SI + SI_NF), "side information in SI_* order");
static_assert(offsetof(lc3gpu_frame_info, rc_order) == 4 * LC3_FI_RC_ORDER, "arithmetic data");
static_assert(offsetof(lc3gpu_frame_info, is_zero_frame) == 4 * LC3_FI_ZERO, "arithmetic data");
static_assert(offsetof(lc3gpu_frame_info, rc_i) == 4 * LC3_FI_RCI, "arithmetic data");
static_assert(offsetof(lc3gpu_frame_info, reserved) == 4 * LC3_FI_RESERVED, "arithmetic data");

// The lsb-mode flags of one lane, word w at bits[w * bstride]: words 0 .. 6 bit t = pair t was coded with escape levels (save_lev[t] > 0),
// words 7 .. 13 bit k = line k is non-zero after the spectral data.  The refinement walk (decode_residual_bits :184-206) reads both for
// k < ntup <= 200 only: save_lev is written by PAIR index and read by LINE index.
#define LC3_INSPECT_BITS_WORDS 14
#define LC3_INSPECT_BITS_NZ 7
#define LC3_INSPECT_BITS_LIMIT 224

__device__ __forceinline__ int lc3_inspect_bit(const uint32_t *bits, int bstride, int word0, int i) {
    return (int)((bits[(word0 + (i >> 5)) * bstride] >> (i & 31)) & 1u);
}
__device__ __forceinline__ void lc3_inspect_set(uint32_t *bits, int bstride, int word0, int i) {
    bits[(word0 + (i >> 5)) * bstride] |= 1u << (i & 31);
}

// read_res_bit (decoder/arithmetic_codec.rs:339-383) on a line that is non-zero when `nz`: only |x| (+1 per refinement: the noise-filling
// seed) and whether the line becomes non-zero matter here
__device__ __forceinline__ int lc3_inspect_res_bit(lc3_parse_ctx &c, int idx, int &nz, int &nres, int &cont) {
    int bit;
    if (nres == 0) { cont = 0; return 0; }
    if (lc3_p_bool(c, bit)) return -1;
    nres -= 1;
    if (bit) {
        if (!nz) {
            if (nres == 0) { cont = 0; return 0; }
            if (lc3_p_bool(c, bit)) return -1;
            nres -= 1;
            nz = 1;
        }
        c.seed += (uint32_t)idx;
    }
    cont = 1;
    return 0;
}

// The fast path over a frame of c.len >= 1 bytes (c.head = c.tail = 0).  rec: the lane's 32 record words, zero on entry; fills words 2 .. 30
// and returns the status: LC3GPU_FRAME_OK, LC3GPU_FRAME_SIDE_INFO + k (the side-information reader is sequential: its k is exact),
// LC3GPU_FRAME_ARITH + k for the checks it makes exactly (1, 6, 7), and LC3GPU_FRAME_ARITH alone when the TNS or spectral data failed
// (the caller classifies).  Arithmetic words are left for the caller to clear when the status is not OK.
//
// ArithmeticDecodeError 1 (ac_dec_init), 7 (a residual bit beyond the frame) and 8 (more than 480 residual bits) cannot occur after the
// side information parsed: the side information is at least 53 bits of a frame of at least 7 bytes; a residual bit is read only while
// nres > 0, which keeps the tail cursor below 8 * (len - head) + 22 (< 8 * len, head >= 3) where the reader's own bound is
// 8 * (len - head + 3); at most one residual bit per non-zero line of at most 400.  The first two are still checked, the third is not.
__device__ __forceinline__ int lc3_inspect_fast(lc3_parse_ctx &c, int32_t *rec, uint32_t *bits, int bstride, int ne, int fs_ind, int n_ms_10,
                                                int &tail_si) {
    int lastnz = 0, lsb_mode = 0, num_tns = 0, ord[2];
    c.nnz = 0;
    c.seed = 0;
    c.plane = rec + LC3_FI_SI;  // side_info_reader::read writes the SI_* words straight into the record
    c.stride = 1;
    const int rc = lc3_parse_side_info<1>(c, fs_ind, ne, lastnz, lsb_mode, num_tns, ord);
    if (rc) return LC3GPU_FRAME_SIDE_INFO - rc;
    tail_si = c.tail;
    const int nbits = c.len * 8;
    // ac_dec_init :57-65
    if (!(c.head + 2 < c.len)) return LC3GPU_FRAME_ARITH + 1;
    lc3_acdec st;
    st.low = ((uint32_t)c.bytes[c.head] << 16) | ((uint32_t)c.bytes[c.head + 1] << 8) | (uint32_t)c.bytes[c.head + 2];
    c.head += 3;
    st.range = 0x00ffffffu;
    lc3_p_prime(c);
    int err = 0, order_out[2];
    // decode_tns_data :304-337
    {
        uint8_t *rci = (uint8_t *)(rec + LC3_FI_RCI);
        const int wt = nbits < (n_ms_10 ? 480 : 360);
        for (int f = 0; f < 2; f++) {
            int order = ord[f];
            if (f < num_tns && order > 0) {
                order = lc3_p_ac_decode_sel<7, 3>(c, st, c.tns + wt * 8, err) + 1;
                for (int k = 0; k < order; k++) rci[f * 8 + k] = (uint8_t)lc3_p_ac_decode_sel<16, 5>(c, st, c.tns + 16 + k * 17, err);
            }
            order_out[f] = order;
        }
        if (err) return LC3GPU_FRAME_ARITH;
    }
    // decode_spectral_data :211-302: lc3_parse_frame's symbol loop without the pair stores
    const int ntup = lastnz / 2;
    int nz01 = 0;  // lines 0 and 1 (the zero-frame test, :146-148)
    if (lsb_mode)
        for (int w = 0; w < LC3_INSPECT_BITS_WORDS; w++) bits[w * bstride] = 0u;
    {
        const int rate_flag = nbits > (160 + fs_ind * 160) ? 512 : 0;
        int cctx = 0, tup = 0, lev = 0, sym = 0, slack = 0x7fffffff;
        int32_t xk = 0, xk1 = 0;
        const int hi_from = ne / 2;
        const uint32_t *row = c.cf + (int)c.lookup[rate_flag + (0 > hi_from ? 256 : 0)] * LC3_DCF_ROW_WORDS;
        lc3_i4 pv = ((const lc3_i4 *)row)[4];
        while (tup < ntup) {
            if (lev < 14) sym = lc3_p_ac_decode_spec_sel(c, st, row, pv, err);
            const int esc = sym >= 16 && lev < 14;
            const int a = sym & 3, b = sym >> 2;
            const int lv = lev < 3 ? lev : 3;
            const int32_t m0 = xk + (int32_t)((uint32_t)a << lev), m1 = xk1 + (int32_t)((uint32_t)b << lev);
            const int want_e = !lsb_mode || lev > 0;
            int bit0, bit1;
            lc3_p_bool2_sel(c, esc ? want_e : m0 > 0, esc ? want_e : m1 > 0, slack, bit0, bit1);
            const int n_cctx = esc ? cctx : (cctx & 15) * 16 + (lv <= 1 ? 1 + ((a + b) << lv) : 12 + lv);
            const int n_tup = tup + !esc, n_lev = esc ? lev + 1 : 0;
            const int n_lv = n_lev < 3 ? n_lev : 3;
            const int n_row = (int)c.lookup[n_cctx + rate_flag + ((n_tup * 2) > hi_from ? 256 : 0) + n_lv * 1024];
            if (lsb_mode && !esc) {  // save_lev[tup] > 0 and the pair's non-zero lines, for the refinement walk
                if (lev > 0) lc3_inspect_set(bits, bstride, 0, tup);
                if (2 * tup < LC3_INSPECT_BITS_LIMIT) {
                    if (m0 != 0) lc3_inspect_set(bits, bstride, LC3_INSPECT_BITS_NZ, 2 * tup);
                    if (m1 != 0) lc3_inspect_set(bits, bstride, LC3_INSPECT_BITS_NZ, 2 * tup + 1);
                }
            }
            nz01 |= (tup == 0 && !esc) ? (int)((m0 | m1) != 0) : 0;
            row = c.cf + n_row * LC3_DCF_ROW_WORDS;
            pv = ((const lc3_i4 *)row)[4];
            lc3_p_head_refill(c);
            asm volatile("" ::: "memory");
            c.nnz += esc ? 0u : (uint32_t)(m0 != 0) + (uint32_t)(m1 != 0);
            c.seed += esc ? 0u : (uint32_t)m0 * (uint32_t)(2 * tup) + (uint32_t)m1 * (uint32_t)(2 * tup + 1);
            cctx = n_cctx;
            xk = esc ? xk + (int32_t)((uint32_t)bit0 << lev) : 0;
            xk1 = esc ? xk1 + (int32_t)((uint32_t)bit1 << lev) : 0;
            tup = n_tup;
            lev = n_lev;
        }
        err |= (c.head > c.len) | (slack < 0) | (c.len - ((c.tail - 1) >> 3) - 1 < 0);
        if (err) return LC3GPU_FRAME_ARITH;
    }
    // calc_num_residual_bits :385-405
    const int nbits_side = c.tail - 8;
    const int nbits_ari = (c.head + 1 - 3) * 8 + 25 - lc3_ilog2(st.range);
    if (nbits < nbits_side + nbits_ari) return LC3GPU_FRAME_ARITH + 6;  // NegativeResidualNumBits
    int nres = nbits - nbits_side - nbits_ari, n_residual = 0;
    if (!lsb_mode) {
        // decode_residual_bits :160-183 takes one bit per non-zero line while bits are left
        n_residual = (int)c.nnz < nres ? (int)c.nnz : nres;
    } else {
        // :184-206: refines |x| of lines k, k + 1 for every even k whose save_lev[k] > 0
        int stop = 0, cont;
        for (int k = 0; k < ntup && !stop; k += 2) {
            if (lc3_inspect_bit(bits, bstride, 0, k)) {
                int nz0 = lc3_inspect_bit(bits, bstride, LC3_INSPECT_BITS_NZ, k), nz1 = lc3_inspect_bit(bits, bstride, LC3_INSPECT_BITS_NZ, k + 1);
                if (lc3_inspect_res_bit(c, k, nz0, nres, cont)) return LC3GPU_FRAME_ARITH + 7;
                if (!cont) stop = 1;
                else if (lc3_inspect_res_bit(c, k + 1, nz1, nres, cont)) return LC3GPU_FRAME_ARITH + 7;
                else if (!cont) stop = 1;
                if (k == 0) nz01 |= nz0 | nz1;
            }
        }
    }
    rec[LC3_FI_RC_ORDER] = order_out[0];
    rec[LC3_FI_RC_ORDER + 1] = order_out[1];
    rec[LC3_FI_NRES] = n_residual;
    rec[LC3_FI_SEED] = (int32_t)(c.seed & 0xFFFFu);  // :140-145
    rec[LC3_FI_ZERO] = lastnz == 2 && !nz01 && rec[LC3_FI_SI + SI_GG] == 0;  // :146-148
    return LC3GPU_FRAME_OK;
}

// arithmetic_codec::decode (:109-158) from the cursors after the side information up to calc_num_residual_bits, every read checked where
// and in the order the reference checks it (the oracle's lc3o_dec_arith).  Returns k of the first ArithmeticDecodeError k it meets
// (2 TNS order, 3 TNS coefficient, 4 spectral symbol, 5 spectral tail bit, 6 negative residual bit count), 0 when it meets none.
// Out of line: only frames the fast path found broken come here.
static __device__ __noinline__ int lc3_inspect_classify(const uint8_t *bytes, int len, const uint8_t *lookup, const uint32_t *cf,
                                                        const uint32_t *tns, int tail, int ne, int fs_ind, int n_ms_10, int lastnz,
                                                        int lsb_mode, int num_tns, int ord0, int ord1) {
    int head = 0;
    if (!(head + 2 < len)) return 1;  // read_head_u24 :52-60
    uint32_t low = ((uint32_t)bytes[0] << 16) | ((uint32_t)bytes[1] << 8) | (uint32_t)bytes[2], range = 0x00ffffffu;
    head = 3;
    // ac_decode :67-97 over a packed (cum | freq << 16) model row of nsym symbols
    auto decode = [&](const uint32_t *row, int nsym, int &sym) -> int {
        const uint32_t tmp = range >> 10;
        if (low >= (tmp << 10)) return -1;
        int val = nsym - 1;
        while (low < tmp * (row[val] & 0xffffu)) val--;
        low -= tmp * (row[val] & 0xffffu);
        range = tmp * (row[val] >> 16);
        while (range < 0x10000u) {
            if (head >= len) return -1;  // read_head_byte :42-50
            low = ((low << 8) & 0x00ffffffu) + (uint32_t)bytes[head++];
            range <<= 8;
        }
        sym = val;
        return 0;
    };
    // read_tail_bool :100-116
    auto tail_bit = [&](int &bit) -> int {
        const int byte_index = tail >> 3;
        if (len - head - byte_index + 2 < 0) return -1;
        const int from = len - byte_index - 1;
        if (from < 0) return -1;
        bit = (int)(((uint32_t)bytes[from] >> (tail & 7)) & 1u);
        tail += 1;
        return 0;
    };
    const int nbits = len * 8;
    int sym = 0, bit = 0;
    {  // decode_tns_data :304-337
        const int wt = nbits < (n_ms_10 ? 480 : 360);
        for (int f = 0; f < num_tns; f++) {
            if ((f ? ord1 : ord0) > 0) {
                if (decode(tns + wt * 8, 8, sym)) return 2;
                const int order = sym + 1;
                for (int k = 0; k < order; k++)
                    if (decode(tns + 16 + k * 17, 17, sym)) return 3;
            }
        }
    }
    {  // decode_spectral_data :211-302
        const int rate_flag = nbits > (160 + fs_ind * 160) ? 512 : 0;
        int cctx = 0;
        for (int tup = 0; tup < lastnz / 2; tup++) {
            const int t = cctx + rate_flag + ((tup * 2) > (ne / 2) ? 256 : 0);
            int lev = 0;
            uint32_t xk = 0, xk1 = 0;
            sym = 0;
            while (lev < 14) {
                const int pki = (int)lookup[t + (lev < 3 ? lev : 3) * 1024];
                if (decode(cf + pki * LC3_DCF_ROW_WORDS, 17, sym)) return 4;
                if (sym < 16) break;
                if (!lsb_mode || lev > 0) {
                    if (tail_bit(bit)) return 5;
                    xk += (uint32_t)bit << lev;
                    if (tail_bit(bit)) return 5;
                    xk1 += (uint32_t)bit << lev;
                }
                lev += 1;
            }
            const int a = sym & 3, b = sym >> 2;
            xk += (uint32_t)a << lev;
            xk1 += (uint32_t)b << lev;
            if (xk > 0 && tail_bit(bit)) return 5;
            if (xk1 > 0 && tail_bit(bit)) return 5;
            lev = lev < 3 ? lev : 3;
            cctx = (cctx & 15) * 16 + (lev <= 1 ? 1 + (a + b) * (lev + 1) : 12 + lev);
        }
    }
    // calc_num_residual_bits :385-405
    if (nbits < (tail - 8) + (head + 1 - 3) * 8 + 25 - lc3_ilog2(range)) return 6;
    return 0;
}

// One frame of an inspection batch: the status by precedence (flagged, empty, then the frame's own), its size and the record.
// size = what the decoder takes for this frame's length (0: empty); rec: the lane's 32 words (written whole here).
__device__ __forceinline__ void lc3_inspect_record(lc3_parse_ctx &c, int flagged, int size, int32_t *rec, uint32_t *bits, int bstride, int ne,
                                                   int fs_ind, int n_ms_10) {
    for (int w = 0; w < LC3_FI_WORDS; w++) rec[w] = 0;
    int status;
    if (flagged) status = LC3GPU_FRAME_FLAGGED;
    else if (size == 0) status = LC3GPU_FRAME_EMPTY;
    else {
        int tail_si = 0;
        c.len = size;
        c.head = 0;
        c.tail = 0;
        status = lc3_inspect_fast(c, rec, bits, bstride, ne, fs_ind, n_ms_10, tail_si);
        if (status == LC3GPU_FRAME_ARITH)
            status += lc3_inspect_classify(c.bytes, size, c.lookup, c.cf, c.tns, tail_si, ne, fs_ind, n_ms_10, rec[LC3_FI_SI + SI_LASTNZ],
                                           rec[LC3_FI_SI + SI_LSB_MODE], rec[LC3_FI_SI + SI_NUM_TNS], rec[LC3_FI_SI + SI_ORD0],
                                           rec[LC3_FI_SI + SI_ORD1]);
        if (status > LC3GPU_FRAME_SIDE_INFO && status <= LC3GPU_FRAME_SIDE_INFO + 5)
            for (int w = LC3_FI_SI; w < LC3_FI_RC_ORDER; w++) rec[w] = 0;  // (the reader writes some words before it fails)
        if (status != LC3GPU_FRAME_OK)
            for (int w = LC3_FI_RC_ORDER; w < LC3_FI_RESERVED; w++) rec[w] = 0;
    }
    rec[LC3_FI_STATUS] = status;
    rec[LC3_FI_NBYTES] = size;
}
