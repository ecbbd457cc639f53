// lc3gpu.hpp -- header-only C++ facade over the C ABI (lc3gpu.h) with the reference's type and method names
// (ninjasource/lc3-codec v0.2.0: src/encoder/lc3_encoder.rs:117-209, src/decoder/lc3_decoder.rs:181-244,
// src/common/config.rs:1-15).  The reference lends caller-allocated working buffers to the codec object; the GPU
// engine owns device memory instead, calc_working_buffer_lengths() is kept for API parity.
#pragma once
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include "lc3gpu.h"

namespace lc3gpu {

enum class SamplingFrequency : int { Hz8000 = 8000, Hz16000 = 16000, Hz24000 = 24000, Hz32000 = 32000, Hz44100 = 44100, Hz48000 = 48000 };
enum class FrameDuration : int { SevenPointFiveMs = 7500, TenMs = 10000 };

struct Error : std::runtime_error {
    int code;
    explicit Error(int c, const char *what) : std::runtime_error(std::string(what) + ": " + lc3gpu_strerror(c)), code(c) {}
};
// Lc3DecoderError::Only16BitsPerAudioSampleSupported (lc3_decoder.rs:36-42)
struct Only16BitsPerAudioSampleSupported : Error { using Error::Error; };

class Lc3Encoder {
public:
    // (integer_len, scaler_len, complex_len), lc3_encoder.rs:194-209
    static std::tuple<size_t, size_t, size_t> calc_working_buffer_lengths(size_t num_channels, FrameDuration d, SamplingFrequency f) {
        int64_t o[3];
        int rc = lc3gpu_encoder_working_buffer_lengths((int)num_channels, (int)d, (int)f, o);
        if (rc) throw Error(rc, "calc_working_buffer_lengths");
        return {(size_t)o[0], (size_t)o[1], (size_t)o[2]};
    }
    // spec_flags: LC3GPU_SPEC_* corrections of the reference's deviations from the specification (0 = the reference's behaviour)
    Lc3Encoder(size_t num_channels, FrameDuration d, SamplingFrequency f, int spec_flags = 0) {
        int rc = lc3gpu_encoder_create_spec(&h_, (int)num_channels, (int)d, (int)f, spec_flags);
        if (rc) throw Error(rc, "Lc3Encoder::new");
    }
    // one handle for streams of different configurations (one launch per kernel for the whole mixed batch)
    explicit Lc3Encoder(const std::vector<lc3gpu_stream_desc> &streams, int spec_flags = 0) {
        int rc = lc3gpu_encoder_create_mixed_spec(&h_, (int)streams.size(), streams.data(), spec_flags);
        if (rc) throw Error(rc, "Lc3Encoder::mixed");
    }
    ~Lc3Encoder() { lc3gpu_encoder_destroy(h_); }
    Lc3Encoder(const Lc3Encoder &) = delete;
    Lc3Encoder &operator=(const Lc3Encoder &) = delete;
    // encode_frame(channel_index, samples_in, buf_out): buf_out.size() selects the bitrate (lc3_encoder.rs:65)
    void encode_frame(size_t channel_index, const std::vector<int16_t> &samples_in, std::vector<uint8_t> &buf_out) {
        int rc = lc3gpu_encode_frame(h_, (int)channel_index, samples_in.data(), (int)samples_in.size(), buf_out.data(), (int)buf_out.size());
        if (rc) throw Error(rc, "encode_frame");  // the reference panics here; Err() is impossible (empty enum)
    }
    // batch: device pointers, stream-major, asynchronous on `hip_stream`
    void encode(const int16_t *d_pcm, uint8_t *d_out, int nbytes, int n_frames, void *hip_stream = nullptr,
                int layout = LC3GPU_LAYOUT_PLANAR) {
        int rc = lc3gpu_encode_layout(h_, layout, d_pcm, d_out, nbytes, n_frames, hip_stream);
        if (rc) throw Error(rc, "encode");
    }
    // mixed handle: ragged buffers in descriptor order (lc3gpu.h)
    void encode_mixed(const int16_t *d_pcm, uint8_t *d_out, int n_frames, void *hip_stream = nullptr) {
        int rc = lc3gpu_encode_mixed(h_, d_pcm, d_out, n_frames, hip_stream);
        if (rc) throw Error(rc, "encode_mixed");
    }
    // a frame size per frame (DEVICE buffers): d_nbytes[channel][frame] is that frame's buf_out.len(), written to the first d_nbytes bytes
    // of its slot of slot_bytes; sizes outside [20, slot_bytes] are clamped and counted (size_clamps)
    void encode_vbr(const int16_t *d_pcm, uint8_t *d_out, const uint16_t *d_nbytes, int slot_bytes, int n_frames, void *hip_stream = nullptr) {
        int rc = lc3gpu_encode_vbr(h_, d_pcm, d_out, d_nbytes, slot_bytes, n_frames, hip_stream);
        if (rc) throw Error(rc, "encode_vbr");
    }
    // a list of channels (HOST indices, any order, none twice): DEVICE buffers compact in list order; the other channels are left as they were
    void encode_list(const std::vector<int32_t> &channels, const int16_t *d_pcm, uint8_t *d_out, int nbytes, int n_frames, void *hip_stream = nullptr) {
        int rc = lc3gpu_encode_list(h_, channels.data(), (int)channels.size(), d_pcm, d_out, nbytes, n_frames, hip_stream);
        if (rc) throw Error(rc, "encode_list");
    }
    // mixed handle: a list of its streams (HOST descriptor indices, any order, none twice); ragged DEVICE buffers compact in LIST order,
    // every stream at its descriptor's frame size; the streams not listed are left as they were
    void encode_mixed_list(const std::vector<int32_t> &channels, const int16_t *d_pcm, uint8_t *d_out, int n_frames, void *hip_stream = nullptr) {
        int rc = lc3gpu_encode_mixed_list(h_, channels.data(), (int)channels.size(), d_pcm, d_out, n_frames, hip_stream);
        if (rc) throw Error(rc, "encode_mixed_list");
    }
    // mixed handle: a list of items, each a stream with its own frame count and frame size for this call (lc3gpu_item; nbytes 0 = the
    // descriptor's); ragged DEVICE buffers compact in list order, item i's PCM at element offset sum n_frames_j * nf_j
    void encode_mixed_items(const std::vector<lc3gpu_item> &items, const int16_t *d_pcm, uint8_t *d_out, void *hip_stream = nullptr) {
        int rc = lc3gpu_encode_mixed_items(h_, items.data(), (int)items.size(), d_pcm, d_out, hip_stream);
        if (rc) throw Error(rc, "encode_mixed_items");
    }
    // mixed handle: multi-channel items (lc3gpu_mc_item: the C descriptors of one stream), PCM int16[T][nf][C], bytes uint8[T][C][nbytes]
    // per item (lc3gpu_encode_mixed_mc_items)
    void encode_mixed_mc_items(const std::vector<lc3gpu_mc_item> &items, const int16_t *d_pcm, uint8_t *d_out, void *hip_stream = nullptr) {
        int rc = lc3gpu_encode_mixed_mc_items(h_, items.data(), (int)items.size(), d_pcm, d_out, hip_stream);
        if (rc) throw Error(rc, "encode_mixed_mc_items");
    }
    // mixed handle: views (lc3gpu_view: an item with the placement of its PCM and its frames), read and written in place; pcm_elems /
    // out_bytes are the buffers' extents, which every view is checked against (lc3gpu_encode_mixed_views)
    void encode_mixed_views(const std::vector<lc3gpu_view> &views, const int16_t *d_pcm, size_t pcm_elems, uint8_t *d_out, size_t out_bytes,
                            void *hip_stream = nullptr) {
        int rc = lc3gpu_encode_mixed_views(h_, views.data(), (int)views.size(), d_pcm, pcm_elems, d_out, out_bytes, hip_stream);
        if (rc) throw Error(rc, "encode_mixed_views");
    }
    // back to the freshly constructed state from the next call on: every channel, or the named ones (a new EncoderChannel); no wait
    void reset() {
        int rc = lc3gpu_encoder_reset(h_);
        if (rc) throw Error(rc, "reset");
    }
    void reset(const std::vector<int32_t> &channels) {
        int rc = lc3gpu_encoder_reset_channels(h_, channels.data(), (int)channels.size());
        if (rc) throw Error(rc, "reset");
    }
    // state blobs of the named channels (blob i belongs to channels[i]; the format of lc3gpu_encoder_state_save)
    std::vector<uint8_t> state_save(const std::vector<int32_t> &channels) {
        std::vector<uint8_t> buf(lc3gpu_encoder_state_size(h_) * channels.size());
        int rc = lc3gpu_encoder_state_save_channels(h_, channels.data(), (int)channels.size(), buf.data(), buf.size());
        if (rc) throw Error(rc, "state_save");
        return buf;
    }
    void state_load(const std::vector<uint8_t> &buf, const std::vector<int32_t> &channels) {
        int rc = lc3gpu_encoder_state_load_channels(h_, channels.data(), (int)channels.size(), buf.data(), buf.size());
        if (rc) throw Error(rc, "state_load");
    }
    uint64_t size_clamps() {
        uint64_t v = 0;
        int rc = lc3gpu_encoder_size_clamps(h_, &v);
        if (rc) throw Error(rc, "size_clamps");
        return v;
    }
    uint64_t pair_timeouts() {
        uint64_t v = 0;
        int rc = lc3gpu_encoder_pair_timeouts(h_, &v);
        if (rc) throw Error(rc, "pair_timeouts");
        return v;
    }
    // the handle's next batch call would return LC3GPU_EPAIR (looked at, not lowered)
    bool pair_pending() const {
        int rc = lc3gpu_encoder_pair_pending(h_);
        if (rc < 0) throw Error(rc, "pair_pending");
        return rc != 0;
    }
    lc3gpu_encoder *handle() { return h_; }

private:
    lc3gpu_encoder *h_ = nullptr;
};

class Lc3Decoder {
public:
    // (scaler_len, complex_len), lc3_decoder.rs:236-244
    static std::tuple<size_t, size_t> calc_working_buffer_lengths(size_t num_channels, FrameDuration d, SamplingFrequency f) {
        int64_t o[2];
        int rc = lc3gpu_decoder_working_buffer_lengths((int)num_channels, (int)d, (int)f, o);
        if (rc) throw Error(rc, "calc_working_buffer_lengths");
        return {(size_t)o[0], (size_t)o[1]};
    }
    Lc3Decoder(size_t num_channels, FrameDuration d, SamplingFrequency f) {
        int rc = lc3gpu_decoder_create(&h_, (int)num_channels, (int)d, (int)f);
        if (rc) throw Error(rc, "Lc3Decoder::new");
    }
    explicit Lc3Decoder(const std::vector<lc3gpu_stream_desc> &streams) {
        int rc = lc3gpu_decoder_create_mixed(&h_, (int)streams.size(), streams.data());
        if (rc) throw Error(rc, "Lc3Decoder::mixed");
    }
    ~Lc3Decoder() { lc3gpu_decoder_destroy(h_); }
    Lc3Decoder(const Lc3Decoder &) = delete;
    Lc3Decoder &operator=(const Lc3Decoder &) = delete;
    // decode_frame(num_bits_per_audio_sample, channel_index, buf_in, samples_out); corrupt frames are concealed
    void decode_frame(size_t num_bits_per_audio_sample, size_t channel_index, const std::vector<uint8_t> &buf_in, std::vector<int16_t> &samples_out) {
        int rc = lc3gpu_decode_frame(h_, (int)num_bits_per_audio_sample, (int)channel_index, buf_in.data(), (int)buf_in.size(), samples_out.data(), (int)samples_out.size());
        if (rc == LC3GPU_EBITS) throw Only16BitsPerAudioSampleSupported(rc, "decode_frame");
        if (rc) throw Error(rc, "decode_frame");
    }
    void decode(const uint8_t *d_in, int16_t *d_pcm, int nbytes, int n_frames, void *hip_stream = nullptr, const uint8_t *d_bad_frame = nullptr,
                int layout = LC3GPU_LAYOUT_PLANAR) {
        int rc = lc3gpu_decode_layout(h_, layout, d_in, d_bad_frame, d_pcm, nbytes, n_frames, hip_stream);
        if (rc) throw Error(rc, "decode");
    }
    void decode_mixed(const uint8_t *d_in, int16_t *d_pcm, int n_frames, void *hip_stream = nullptr, const uint8_t *d_bad_frame = nullptr) {
        int rc = lc3gpu_decode_mixed(h_, d_in, d_bad_frame, d_pcm, n_frames, hip_stream);
        if (rc) throw Error(rc, "decode_mixed");
    }
    // a list of channels (HOST indices, any order, none twice): DEVICE buffers compact in list order; the other channels keep state and PLC count
    void decode_list(const std::vector<int32_t> &channels, const uint8_t *d_in, int16_t *d_pcm, int nbytes, int n_frames, void *hip_stream = nullptr,
                     const uint8_t *d_bad_frame = nullptr) {
        int rc = lc3gpu_decode_list(h_, channels.data(), (int)channels.size(), d_in, d_bad_frame, d_pcm, nbytes, n_frames, hip_stream);
        if (rc) throw Error(rc, "decode_list");
    }
    // mixed handle: a list of its streams, buffers (and flags) compact in LIST order; the streams not listed keep state and PLC count
    void decode_mixed_list(const std::vector<int32_t> &channels, const uint8_t *d_in, int16_t *d_pcm, int n_frames, void *hip_stream = nullptr,
                           const uint8_t *d_bad_frame = nullptr) {
        int rc = lc3gpu_decode_mixed_list(h_, channels.data(), (int)channels.size(), d_in, d_bad_frame, d_pcm, n_frames, hip_stream);
        if (rc) throw Error(rc, "decode_mixed_list");
    }
    // mixed handle: a list of items (see Encoder::encode_mixed_items); d_bad_frame one flag per frame in item order
    void decode_mixed_items(const std::vector<lc3gpu_item> &items, const uint8_t *d_in, int16_t *d_pcm, void *hip_stream = nullptr,
                            const uint8_t *d_bad_frame = nullptr) {
        int rc = lc3gpu_decode_mixed_items(h_, items.data(), (int)items.size(), d_in, d_bad_frame, d_pcm, hip_stream);
        if (rc) throw Error(rc, "decode_mixed_items");
    }
    // mixed handle: multi-channel items (see Encoder::encode_mixed_mc_items); d_bad_frame uint8[T][C] per item
    void decode_mixed_mc_items(const std::vector<lc3gpu_mc_item> &items, const uint8_t *d_in, int16_t *d_pcm, void *hip_stream = nullptr,
                               const uint8_t *d_bad_frame = nullptr) {
        int rc = lc3gpu_decode_mixed_mc_items(h_, items.data(), (int)items.size(), d_in, d_bad_frame, d_pcm, hip_stream);
        if (rc) throw Error(rc, "decode_mixed_mc_items");
    }
    // mixed handle: views (see Encoder::encode_mixed_views); d_bad_frame / n_flags the flag array and its length, or nullptr / 0
    void decode_mixed_views(const std::vector<lc3gpu_view> &views, const uint8_t *d_in, size_t in_bytes, int16_t *d_pcm, size_t pcm_elems,
                            void *hip_stream = nullptr, const uint8_t *d_bad_frame = nullptr, size_t n_flags = 0) {
        int rc = lc3gpu_decode_mixed_views(h_, views.data(), (int)views.size(), d_in, in_bytes, d_bad_frame, n_flags, d_pcm, pcm_elems, hip_stream);
        if (rc) throw Error(rc, "decode_mixed_views");
    }
    // every channel, or the named ones (a new DecoderChannel; their PLC counts go to zero); no wait
    void reset() {
        int rc = lc3gpu_decoder_reset(h_);
        if (rc) throw Error(rc, "reset");
    }
    void reset(const std::vector<int32_t> &channels) {
        int rc = lc3gpu_decoder_reset_channels(h_, channels.data(), (int)channels.size());
        if (rc) throw Error(rc, "reset");
    }
    std::vector<uint8_t> state_save(const std::vector<int32_t> &channels) {
        std::vector<uint8_t> buf(lc3gpu_decoder_state_size(h_) * channels.size());
        int rc = lc3gpu_decoder_state_save_channels(h_, channels.data(), (int)channels.size(), buf.data(), buf.size());
        if (rc) throw Error(rc, "state_save");
        return buf;
    }
    void state_load(const std::vector<uint8_t> &buf, const std::vector<int32_t> &channels) {
        int rc = lc3gpu_decoder_state_load_channels(h_, channels.data(), (int)channels.size(), buf.data(), buf.size());
        if (rc) throw Error(rc, "state_load");
    }
    uint64_t plc_events() {
        uint64_t v = 0;
        int rc = lc3gpu_decoder_plc_events(h_, &v);
        if (rc) throw Error(rc, "plc_events");
        return v;
    }
    // a frame size per frame (DEVICE buffers): d_nbytes[channel][frame] is that frame's buf_in.len(), its bytes the first d_nbytes of its
    // slot of slot_bytes; 0 or above slot_bytes: concealed
    void decode_vbr(const uint8_t *d_in, const uint16_t *d_nbytes, int16_t *d_pcm, int slot_bytes, int n_frames, void *hip_stream = nullptr,
                    const uint8_t *d_bad_frame = nullptr) {
        int rc = lc3gpu_decode_vbr(h_, d_in, d_nbytes, d_bad_frame, d_pcm, slot_bytes, n_frames, hip_stream);
        if (rc) throw Error(rc, "decode_vbr");
    }
    uint64_t pair_timeouts() {
        uint64_t v = 0;
        int rc = lc3gpu_decoder_pair_timeouts(h_, &v);
        if (rc) throw Error(rc, "pair_timeouts");
        return v;
    }
    // the handle's next batch call would return LC3GPU_EPAIR (looked at, not lowered)
    bool pair_pending() const {
        int rc = lc3gpu_decoder_pair_pending(h_);
        if (rc < 0) throw Error(rc, "pair_pending");
        return rc != 0;
    }
    lc3gpu_decoder *handle() { return h_; }

private:
    lc3gpu_decoder *h_ = nullptr;
};

// Frame inspection (lc3gpu_inspect): the side information and decode status of n_frames frames; DEVICE pointers, no handle needed
inline void inspect(FrameDuration d, SamplingFrequency f, const uint8_t *d_in, lc3gpu_frame_info *d_info, int slot_bytes, int n_frames,
                    const uint16_t *d_nbytes = nullptr, const uint8_t *d_bad_frame = nullptr, void *hip_stream = nullptr) {
    int rc = lc3gpu_inspect((int)d, (int)f, d_in, d_nbytes, d_bad_frame, slot_bytes, n_frames, d_info, hip_stream);
    if (rc) throw Error(rc, "inspect");
}

// The inspector (lc3gpu_inspect_mixed_views): the status and the side information of every frame of a tick, for the very views the tick
// passes to Lc3Decoder::decode_mixed_views; streams = the array of Lc3Decoder(streams), max_views the most views one call may name.
// Independent of every codec handle
class Lc3Inspector {
public:
    Lc3Inspector(const std::vector<lc3gpu_stream_desc> &streams, size_t max_views) {
        int rc = lc3gpu_inspector_create(&h_, (int)streams.size(), streams.data(), (int)max_views);
        if (rc) throw Error(rc, "Lc3Inspector::new");
    }
    ~Lc3Inspector() { lc3gpu_inspector_destroy(h_); }
    Lc3Inspector(const Lc3Inspector &) = delete;
    Lc3Inspector &operator=(const Lc3Inspector &) = delete;
    // frame t of a view: its status byte at d_status[flag_off + t * flag_pitch], its record at d_info[the same index]; either output may be
    // nullptr (with extent 0), not both; d_bad_frame / n_flags the flag array and its length, or nullptr / 0
    void inspect_mixed_views(const std::vector<lc3gpu_view> &views, const uint8_t *d_in, size_t in_bytes, uint8_t *d_status, size_t n_status,
                             lc3gpu_frame_info *d_info = nullptr, size_t n_info = 0, const uint8_t *d_bad_frame = nullptr, size_t n_flags = 0,
                             void *hip_stream = nullptr) {
        int rc = lc3gpu_inspect_mixed_views(h_, views.data(), (int)views.size(), d_in, in_bytes, d_bad_frame, n_flags, d_status, n_status, d_info,
                                            n_info, hip_stream);
        if (rc) throw Error(rc, "inspect_mixed_views");
    }
    lc3gpu_inspector *handle() { return h_; }

private:
    lc3gpu_inspector *h_ = nullptr;
};

// The analyzer (lc3gpu_analyze_mixed_views): the reconstructed spectrum, the 64 band energies and the total energy of every frame of a
// tick, for the very views the tick passes to Lc3Decoder::decode_mixed_views, without decoding to PCM; streams = the array of
// Lc3Decoder(streams), max_views / max_frames the most views one call may name and the most frames it may hold.  Independent of every codec
// handle and of the inspector
class Lc3Analyzer {
public:
    Lc3Analyzer(const std::vector<lc3gpu_stream_desc> &streams, size_t max_views, size_t max_frames) {
        int rc = lc3gpu_analyzer_create(&h_, (int)streams.size(), streams.data(), (int)max_views, (int)max_frames);
        if (rc) throw Error(rc, "Lc3Analyzer::new");
    }
    ~Lc3Analyzer() { lc3gpu_analyzer_destroy(h_); }
    Lc3Analyzer(const Lc3Analyzer &) = delete;
    Lc3Analyzer &operator=(const Lc3Analyzer &) = delete;
    // frame t of a view, i = flag_off + t * flag_pitch: its energy at d_energy[i] (-1 for a frame the decoder would conceal), its band row at
    // d_bands[i * LC3GPU_BANDS], its spectrum row at d_spec[i * LC3GPU_SPEC_LINES] (16-byte aligned); any output may be nullptr (with extent
    // 0), not all three; d_bad_frame / n_flags the flag array and its length, or nullptr / 0
    void analyze_mixed_views(const std::vector<lc3gpu_view> &views, const uint8_t *d_in, size_t in_bytes, float *d_energy, size_t n_energy,
                             float *d_bands = nullptr, size_t n_bands = 0, float *d_spec = nullptr, size_t n_spec = 0,
                             const uint8_t *d_bad_frame = nullptr, size_t n_flags = 0, void *hip_stream = nullptr) {
        int rc = lc3gpu_analyze_mixed_views(h_, views.data(), (int)views.size(), d_in, in_bytes, d_bad_frame, n_flags, d_energy, n_energy, d_bands,
                                            n_bands, d_spec, n_spec, hip_stream);
        if (rc) throw Error(rc, "analyze_mixed_views");
    }
    lc3gpu_analyzer *handle() { return h_; }

private:
    lc3gpu_analyzer *h_ = nullptr;
};

// The mixer (lc3gpu_mix_mixed_views): the room mixes of a tick, the PCM read where Lc3Decoder::decode_mixed_views wrote it and written
// where Lc3Encoder::encode_mixed_views reads it, in one launch; streams = the array of Lc3Decoder(streams) (only fs_hz and frame_us are
// used), max_views the most input plus output views one call may name and the number of buses.  Independent of every codec handle, of the
// inspector and of the analyzer
class Lc3Mixer {
public:
    Lc3Mixer(const std::vector<lc3gpu_stream_desc> &streams, size_t max_views) {
        int rc = lc3gpu_mixer_create(&h_, (int)streams.size(), streams.data(), (int)max_views);
        if (rc) throw Error(rc, "Lc3Mixer::new");
    }
    ~Lc3Mixer() { lc3gpu_mixer_destroy(h_); }
    Lc3Mixer(const Lc3Mixer &) = delete;
    Lc3Mixer &operator=(const Lc3Mixer &) = delete;
    // ins[i] belongs to in_views[i], outs[o] to out_views[o]: output o gets the clamped sum of its bus's inputs, each scaled by its gain_q14
    // (16384 = unity), less the term of input outs[o].minus (-1: none).  d_pcm_in and d_pcm_out may not overlap
    void mix_mixed_views(const std::vector<lc3gpu_view> &in_views, const std::vector<lc3gpu_mix_in> &ins, const int16_t *d_pcm_in, size_t in_elems,
                         const std::vector<lc3gpu_view> &out_views, const std::vector<lc3gpu_mix_out> &outs, int16_t *d_pcm_out, size_t out_elems,
                         void *hip_stream = nullptr) {
        if (ins.size() != in_views.size() || outs.size() != out_views.size()) throw Error(LC3GPU_EINVAL, "mix_mixed_views");
        int rc = lc3gpu_mix_mixed_views(h_, in_views.data(), ins.data(), (int)in_views.size(), d_pcm_in, in_elems, out_views.data(), outs.data(),
                                        (int)out_views.size(), d_pcm_out, out_elems, hip_stream);
        if (rc) throw Error(rc, "mix_mixed_views");
    }
    lc3gpu_mixer *handle() { return h_; }

private:
    lc3gpu_mixer *h_ = nullptr;
};

// The resampler (lc3gpu_resample_mixed_views): the rate conversions of a tick -- up before the mix, down after it --, the PCM read where
// one view array says and written where a second says, in one launch, with a FIR history per channel; channels = one (fs_in_hz, fs_out_hz,
// frame_us) each, max_views the most pairs of views one call may name.  Independent of every codec handle and of the three other companions
class Lc3Resampler {
public:
    Lc3Resampler(const std::vector<lc3gpu_rate_desc> &channels, size_t max_views) {
        int rc = lc3gpu_resampler_create(&h_, (int)channels.size(), channels.data(), (int)max_views);
        if (rc) throw Error(rc, "Lc3Resampler::new");
    }
    ~Lc3Resampler() { lc3gpu_resampler_destroy(h_); }
    Lc3Resampler(const Lc3Resampler &) = delete;
    Lc3Resampler &operator=(const Lc3Resampler &) = delete;
    // in_views[i] and out_views[i] belong together (same channel, same n_frames; a channel once per call).  d_pcm_in and d_pcm_out may not
    // overlap.  Every listed channel's history advances
    void resample_mixed_views(const std::vector<lc3gpu_view> &in_views, const int16_t *d_pcm_in, size_t in_elems, const std::vector<lc3gpu_view> &out_views,
                              int16_t *d_pcm_out, size_t out_elems, void *hip_stream = nullptr) {
        if (in_views.size() != out_views.size()) throw Error(LC3GPU_EINVAL, "resample_mixed_views");
        int rc = lc3gpu_resample_mixed_views(h_, in_views.data(), d_pcm_in, in_elems, out_views.data(), d_pcm_out, out_elems, (int)in_views.size(),
                                             hip_stream);
        if (rc) throw Error(rc, "resample_mixed_views");
    }
    // the channels read a zero history in their next call; nothing waits, nothing is launched
    void reset() {
        int rc = lc3gpu_resampler_reset(h_);
        if (rc) throw Error(rc, "resampler_reset");
    }
    void reset_channels(const std::vector<int32_t> &channels) {
        int rc = lc3gpu_resampler_reset_channels(h_, channels.data(), (int)channels.size());
        if (rc) throw Error(rc, "resampler_reset_channels");
    }
    lc3gpu_resampler *handle() { return h_; }

private:
    lc3gpu_resampler *h_ = nullptr;
};

// The meter (lc3gpu_measure_mixed_views): the PCM levels and the speech gate of a tick, the PCM read where one view array says it lies, in
// one launch, with a small state per channel (last sample, envelope, hang-over); channels = one lc3gpu_meter_desc each, max_views the most
// views one call may name.  Independent of every other object
class Lc3Meter {
public:
    Lc3Meter(const std::vector<lc3gpu_meter_desc> &channels, size_t max_views) {
        int rc = lc3gpu_meter_create(&h_, (int)channels.size(), channels.data(), (int)max_views);
        if (rc) throw Error(rc, "Lc3Meter::new");
    }
    ~Lc3Meter() { lc3gpu_meter_destroy(h_); }
    Lc3Meter(const Lc3Meter &) = delete;
    Lc3Meter &operator=(const Lc3Meter &) = delete;
    // frame t of a view gets its activity byte and its record at index flag_off + t * flag_pitch; either output may be null, not both; a
    // channel once per call.  Every listed channel's state advances
    void measure_mixed_views(const std::vector<lc3gpu_view> &views, const int16_t *d_pcm, size_t pcm_elems, uint8_t *d_active, size_t n_active,
                             lc3gpu_level *d_levels, size_t n_levels, void *hip_stream = nullptr) {
        int rc = lc3gpu_measure_mixed_views(h_, views.data(), (int)views.size(), d_pcm, pcm_elems, d_active, n_active, d_levels, n_levels, hip_stream);
        if (rc) throw Error(rc, "measure_mixed_views");
    }
    // the channels start from last = 0, env = 0, hang = 0 in their next call; nothing waits, nothing is launched
    void reset() {
        int rc = lc3gpu_meter_reset(h_);
        if (rc) throw Error(rc, "meter_reset");
    }
    void reset_channels(const std::vector<int32_t> &channels) {
        int rc = lc3gpu_meter_reset_channels(h_, channels.data(), (int)channels.size());
        if (rc) throw Error(rc, "meter_reset_channels");
    }
    lc3gpu_meter *handle() { return h_; }

private:
    lc3gpu_meter *h_ = nullptr;
};

// ---- the reference's no_std / no-alloc API shape (lc3_encoder.rs:37-40,212-303, lc3_decoder.rs:56-60,247-310): the
// number of channels is a compile-time constant instead of a constructor argument (`Lc3Encoder::<NUM_CH>::new(duration,
// frequency, ..)`, `Lc3Encoder::<NUM_CH>::calc_working_buffer_lengths(duration, frequency)`; default 2 as in the
// reference).  Same engine underneath; the caller-lent working buffers of the reference have no counterpart here.
template <size_t NUM_CHANNELS = 2>
class Lc3EncoderStatic : public Lc3Encoder {
public:
    static constexpr size_t num_channels = NUM_CHANNELS;
    static std::tuple<size_t, size_t, size_t> calc_working_buffer_lengths(FrameDuration d, SamplingFrequency f) {
        return Lc3Encoder::calc_working_buffer_lengths(NUM_CHANNELS, d, f);
    }
    Lc3EncoderStatic(FrameDuration d, SamplingFrequency f) : Lc3Encoder(NUM_CHANNELS, d, f) {}
};
template <size_t NUM_CHANNELS = 2>
class Lc3DecoderStatic : public Lc3Decoder {
public:
    static constexpr size_t num_channels = NUM_CHANNELS;
    static std::tuple<size_t, size_t> calc_working_buffer_lengths(FrameDuration d, SamplingFrequency f) {
        return Lc3Decoder::calc_working_buffer_lengths(NUM_CHANNELS, d, f);
    }
    Lc3DecoderStatic(FrameDuration d, SamplingFrequency f) : Lc3Decoder(NUM_CHANNELS, d, f) {}
};

}  // namespace lc3gpu
