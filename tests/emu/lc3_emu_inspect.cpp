// TEST INFRASTRUCTURE -- the CPU wave emulator (lc3_emu.cpp, included unchanged) running the frame inspection (lc3gpu_inspect): the lane
// body of lc3_inspect_kernel (lc3gpu.hip) -- lc3_inspect_record over the device header lc3_dev_dec_inspect.h -- one frame at a time, with
// the tables the kernel stages in LDS.  The kernel's own block code (byte staging, the record copy-out) is checked by the GPU tests.
// Build: tests/test_emu_inspect.py.
#include "lc3_emu.cpp"

#include "../../lc3-codec_amd/csrc/lc3_dev_dec_vbr.h"
#include "../../lc3-codec_amd/csrc/lc3_dev_dec_inspect.h"

extern "C" {
// in uint8[n][slot], nb uint16[n] or null, bad uint8[n] or null -> info int32[n][32] (lc3gpu_frame_info); 0, or -1 for a bad configuration
int lc3emu_inspect(int fs_hz, int frame_us, const uint8_t *in, const uint16_t *nb, const uint8_t *bad, int slot, int n, int32_t *info) {
    lc3_cfg cfg;
    if (lc3_make_config(cfg, frame_us, fs_hz) || slot < 1 || slot > LC3_MAX_NE) return -1;
    alignas(16) static uint32_t cf[64 * LC3_DCF_ROW_WORDS];
    for (int i = 0; i < 64 * LC3_DCF_ROW_WORDS; i++) cf[i] = lc3_dcf_word(i);
    static uint32_t tns[LC3_TNS_MODEL_WORDS];
    for (int i = 0; i < LC3_TNS_MODEL_WORDS; i++) tns[i] = lc3_tns_model_word(i);
    std::vector<uint8_t> bytes((size_t)slot);
    uint32_t bits[LC3_INSPECT_BITS_WORDS];
    for (int f = 0; f < n; f++) {
        memcpy(bytes.data(), in + (size_t)f * (size_t)slot, (size_t)slot);  // (the kernel's LDS copy of the slot)
        memset(bits, 0xA5, sizeof(bits));  // stale flags from another frame must not matter
        lc3_parse_ctx c;
        c.dbg = nullptr;
        c.bytes = bytes.data();
        c.lookup = LC3T_AC_SPEC_LOOKUP;
        c.cf = cf;
        c.tns = tns;
        const int size = nb ? lc3_vbr_dec_size(nb, (size_t)f, slot) : slot;
        int32_t *rec = info + (size_t)f * LC3_FI_WORDS;
        for (int w = 0; w < LC3_FI_WORDS; w++) rec[w] = (int32_t)0xDEADBEEF;  // (the kernel's staging area is not cleared either)
        lc3_inspect_record(c, bad && bad[f], size, rec, bits, 1, cfg.ne, cfg.fs_ind, cfg.n_ms_10);
    }
    return 0;
}
}
