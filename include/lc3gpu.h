/* lc3gpu -- C ABI of the MI355X-native batched LC3 codec (liblc3gpu.so).
 *
 * Drop-in boundary for the per-frame hot path of ninjasource/lc3-codec v0.2.0:
 *   Lc3Encoder::{calc_working_buffer_lengths,new,encode_frame}   reference src/encoder/lc3_encoder.rs:117-209
 *   Lc3Decoder::{calc_working_buffer_lengths,new,decode_frame}   reference src/decoder/lc3_decoder.rs:181-244
 * A handle owns N independent codec channels ("streams") on one HIP device; each stream is one
 * reference EncoderChannel / DecoderChannel with its own carried state.  The batch calls process
 * `n_streams x n_frames` frames per launch: one CDNA4 wavefront per stream, frames of a stream in
 * time order -- all channels, a contiguous range, or a list of channels in any order (lc3gpu_*_list, with
 * per-channel resets and state blobs: lc3gpu_*_reset_channels, lc3gpu_*_state_{save,load}_channels).  The *_frame calls are the n_streams = 1, n_frames = 1 case with host buffers and
 * have the reference's argument meaning (slice lengths select the frame size / bitrate).
 *
 * Plain C types only (pointers + sizes); no torch / C++ types cross this boundary.
 * All functions return LC3GPU_OK (0) or a negative LC3GPU_E* code; nothing aborts across the ABI:
 * where the reference panics (bad channel index, wrong slice length: lc3_encoder.rs:181-190,
 * encoder/modified_dct.rs:109-111) an error code is returned instead.  Corrupt frames are NOT
 * errors: as in the reference (lc3_decoder.rs:138-141) they are concealed (PLC) and counted.
 * Handles are not thread-safe (mirrors `&mut self`); distinct handles may be used concurrently.
 * A handle is bound to the HIP device that was current when it was created; every call switches to that device for its
 * duration.  Batch calls are asynchronous on the HIP stream they are given; a handle's launches share its scratch planes, so
 * a call on another stream than the handle's previous one is ordered after it (an event wait on the GPU, no host
 * synchronisation).  State load / reset calls wait for the handle's work in flight.
 */
#ifndef LC3GPU_H_
#define LC3GPU_H_
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LC3GPU_OK 0
#define LC3GPU_EINVAL -1        /* bad argument (unsupported fs / duration, null pointer, size mismatch) */
#define LC3GPU_ECHANNEL -2      /* channel index out of range (reference: panic, lc3_encoder.rs:185-189) */
#define LC3GPU_ELENGTH -3       /* samples / buffer length mismatch (reference: assert_eq! panic); also: a frame size outside
                                   20 ... 400 bytes on the encoder (1 ... 400 on the decoder) -- a deliberate deviation: the reference's
                                   encode_frame takes any buf_out.len() (src/encoder/lc3_encoder.rs:65), LC3 defines this range */
#define LC3GPU_EBITS -4         /* Lc3DecoderError::Only16BitsPerAudioSampleSupported (lc3_decoder.rs:80-82) */
#define LC3GPU_EHIP -5          /* HIP runtime error; see lc3gpu_last_hip_error() */
#define LC3GPU_ENODEVICE -6     /* no usable HIP device */
#define LC3GPU_EUNSUPPORTED -7  /* configuration the reference cannot run (8 kHz encode: bandwidth_detector.rs:36-37) */
#define LC3GPU_EPAIR -8         /* a producer / consumer wave pair of an EARLIER batch call of this handle gave up on its partner (see
                                   lc3gpu_*_pair_timeouts): that call's frames are zero-filled (encoder) or concealed (decoder).  Returned
                                   once, by the first batch call that notices (read from pinned host memory: no synchronisation); the call
                                   that returns it has launched nothing and may be repeated */

/* Opt-in corrections of the reference's deviations from the LC3 specification, one bit each, for interop with
 * other LC3 codecs.  Default 0: every deviation is reproduced, and only then do the bit-exactness claims against the
 * reference hold (with a bit set there is no reference behaviour; the CPU oracle implements the same switches). */
#define LC3GPU_SPEC_8KHZ_ENCODE 1     /* 8 kHz encoders can be created (reference: constructor panics, bandwidth_detector.rs:36-37) */
#define LC3GPU_SPEC_TNS_SSWB_STOP 2   /* 10 ms, bandwidth index 2: TNS filters lines 12..240 (reference: ..200, temporal_noise_shaping.rs:134-140) */
#define LC3GPU_SPEC_BW_CUTOFF_DB 4    /* bandwidth cut-off test on 10 log10(eps + ratio) (reference: raw ratio, bandwidth_detector.rs:106-115) */
#define LC3GPU_SPEC_SNS_LAST_GAIN 8   /* SNS gain search includes the last gain of every shape (reference: spectral_noise_shaping.rs:495-503) */
#define LC3GPU_SPEC_NBITS_SPEC_OLD 16 /* nbits_spec_old is updated (reference: stays 0, spectral_quantization.rs:59,97-100) */
#define LC3GPU_SPEC_ALL 31

typedef struct lc3gpu_encoder lc3gpu_encoder;
typedef struct lc3gpu_decoder lc3gpu_decoder;

/* Buffer layouts of the batch calls (C = the handle's channel count, T = n_frames):
 *   PLANAR       int16[C][T][nf], uint8[C][T][nbytes], flags uint8[C][T]: what the reference's per-channel calls see after
 *                the caller has de-interleaved (examples/encode.rs:95-102)
 *   INTERLEAVED  int16[T][nf][C], uint8[T][C][nbytes], flags uint8[T][C]: the WAV sample order and the .lc3 file order
 *                (frames in time order, channels inside a frame: examples/encode.rs:105-115, examples/decode.rs:86-112); the
 *                kernels de-interleave on load and interleave on store */
#define LC3GPU_LAYOUT_PLANAR 0
#define LC3GPU_LAYOUT_INTERLEAVED 1

/* One stream of a mixed-configuration handle: the reference builds one Lc3Encoder / Lc3Decoder per configuration
 * (lc3_encoder.rs:117-124, common/config.rs:42-100) and takes the frame size from the slice length of every call
 * (lc3_encoder.rs:65); a mixed handle fixes all three per stream so that ONE launch per kernel serves every stream. */
typedef struct lc3gpu_stream_desc {
    int fs_hz;    /* 8000 (decoder only), 16000, 24000, 32000, 44100, 48000 */
    int frame_us; /* 7500 or 10000 */
    int nbytes;   /* bytes per frame */
} lc3gpu_stream_desc;

/* library / device */
int lc3gpu_version(void);
const char *lc3gpu_strerror(int code);
int lc3gpu_last_hip_error(void);
int lc3gpu_device_count(void);

/* common/config.rs:42-100 -- out[7] = {fs_ind, fs, ne, n_ms_is_10, nb, nf, z} */
int lc3gpu_config(int frame_us, int fs_hz, int out[7]);

/* Lc3Encoder::calc_working_buffer_lengths (lc3_encoder.rs:194-209): out = {i16_len, f32_len, complex_len}.
 * Kept for API parity; the GPU engine allocates its own device memory. */
int lc3gpu_encoder_working_buffer_lengths(int num_channels, int frame_us, int fs_hz, int64_t out[3]);
/* Lc3Decoder::calc_working_buffer_lengths (lc3_decoder.rs:236-244): out = {f32_len, complex_len} */
int lc3gpu_decoder_working_buffer_lengths(int num_channels, int frame_us, int fs_hz, int64_t out[2]);

/* ---- encoder ------------------------------------------------------------------------------------ */
/* Lc3Encoder::new (lc3_encoder.rs:117-173): num_channels fresh channels on the current HIP device. */
int lc3gpu_encoder_create(lc3gpu_encoder **out, int num_channels, int frame_us, int fs_hz);
/* the same with LC3GPU_SPEC_* corrections switched on (spec_flags = 0: identical to lc3gpu_encoder_create) */
int lc3gpu_encoder_create_spec(lc3gpu_encoder **out, int num_channels, int frame_us, int fs_hz, int spec_flags);
int lc3gpu_encoder_destroy(lc3gpu_encoder *enc);
/* back to the freshly constructed state (all channels).  Costs no synchronisation: work in flight completes as it is, the NEXT call starts
 * every channel from the constructed state (lc3gpu_decoder_reset likewise) */
int lc3gpu_encoder_reset(lc3gpu_encoder *enc);

/* Lc3Encoder::encode_frame (lc3_encoder.rs:175-191), host buffers.
 * samples_in: n_samples (must be nf) planar i16; buf_out: nbytes (= buf_out.len(), selects the bitrate). */
int lc3gpu_encode_frame(lc3gpu_encoder *enc, int channel_index, const int16_t *samples_in, int n_samples,
                        uint8_t *buf_out, int nbytes);

/* Batch: every channel encodes n_frames consecutive frames.  DEVICE pointers, stream-major:
 *   d_pcm  int16[num_channels][n_frames][nf]      (4-byte aligned)
 *   d_out  uint8[num_channels][n_frames][nbytes]
 * Asynchronous on hip_stream (a hipStream_t, may be NULL for the default stream). */
int lc3gpu_encode(lc3gpu_encoder *enc, const int16_t *d_pcm, uint8_t *d_out, int nbytes, int n_frames,
                  void *hip_stream);
/* same, restricted to channels [first_channel, first_channel + n_channels); buffers hold only those channels */
int lc3gpu_encode_range(lc3gpu_encoder *enc, int first_channel, int n_channels, const int16_t *d_pcm,
                        uint8_t *d_out, int nbytes, int n_frames, void *hip_stream);
/* Batch over a LIST of the handle's channels: the reference's caller decides per call which channel gets a frame (examples/encode.rs:97-115,
 * one encode_frame per channel it chooses), so a tick of a many-stream server -- only some streams have a frame, in any order -- is ONE call.
 *   channels  HOST int32[n_list]: entry i names the channel whose frames are item i of the buffers; any order, no channel twice.  The array
 *             may be reused as soon as the call returns (the handle copies it to pinned memory of its own and from there to the device in
 *             stream order: no host synchronisation)
 *   d_pcm     DEVICE int16[n_list][n_frames][nf] (4-byte aligned), d_out DEVICE uint8[n_list][n_frames][nbytes]: planar, compact in list order
 * Checked on the host before anything is queued: an index outside [0, num_channels) or a channel named twice: LC3GPU_ECHANNEL; null pointers,
 * a negative n_list, misaligned PCM, a mixed handle: LC3GPU_EINVAL; nbytes / n_frames as lc3gpu_encode (LC3GPU_ELENGTH).  A call that returns
 * an error has launched nothing and changed no channel; n_list = 0 launches nothing and returns LC3GPU_OK.  A bound handle takes the call on its
 * bound stream only; LC3GPU_EPAIR as for the other batch calls.  Every listed channel advances by n_frames frames exactly as under
 * lc3gpu_encode; every channel not listed is left byte for byte as it was.  List, uniform, range, sized and *_frame calls may alternate on
 * a handle; a list 0 .. num_channels-1 gives the bytes of lc3gpu_encode, a contiguous ascending run those of lc3gpu_encode_range.  Channels
 * reset by lc3gpu_encoder_reset_channels start from the constructed state inside the same launch as the carried ones.  Asynchronous on
 * hip_stream, ordered after the handle's earlier work.
 * NOT provided (out of scope): lists on mixed handles (they have calls of their own: lc3gpu_encode_mixed_list / lc3gpu_decode_mixed_list),
 * with the interleaved layout, with a frame size per frame (lc3gpu_*_vbr), on the host-resident calls (lc3gpu_*_host) and in the pipeline
 * object. */
int lc3gpu_encode_list(lc3gpu_encoder *enc, const int32_t *channels, int n_list, const int16_t *d_pcm, uint8_t *d_out, int nbytes,
                       int n_frames, void *hip_stream);
/* The named channels (HOST int32[n]) are back in the freshly constructed state from their next call on -- the reference builds a new
 * EncoderChannel; channels not named are untouched.  Like lc3gpu_encoder_reset it waits for nothing and launches nothing.  LC3GPU_ECHANNEL
 * for an index out of range, LC3GPU_EINVAL for null / negative; a channel named twice is harmless. */
int lc3gpu_encoder_reset_channels(lc3gpu_encoder *enc, const int32_t *channels, int n);
/* same as lc3gpu_encode with the buffers in `layout` (LC3GPU_LAYOUT_*); interleaved PCM needs 2-byte alignment only */
int lc3gpu_encode_layout(lc3gpu_encoder *enc, int layout, const int16_t *d_pcm, uint8_t *d_out, int nbytes, int n_frames,
                         void *hip_stream);

/* Batch encode with a frame size per frame: d_nbytes[c][t] is what the reference's buf_out.len() is for frame t of channel c
 * (lc3_encoder.rs:65, it may change per call), so every channel may change its bitrate in every frame of one launch.  DEVICE pointers,
 * planar, every channel of the handle:
 *   d_pcm     int16[num_channels][n_frames][nf]          as lc3gpu_encode (4-byte aligned)
 *   d_nbytes  uint16[num_channels][n_frames]
 *   d_out     uint8[num_channels][n_frames][slot_bytes]  frame (c, t) is written to the first d_nbytes[c][t] bytes of its slot; the rest
 *                                                        of the slot is left untouched
 * slot_bytes 20 ... 400, else LC3GPU_ELENGTH.  Null pointers, misaligned PCM and mixed handles: LC3GPU_EINVAL.  A bound handle takes the
 * call on its bound stream only.  The sizes are device data, so they are checked on the device: an entry outside [20, slot_bytes] is
 * clamped into that range, the frame is encoded (and the channel's state advanced) at the clamped size, and the clamp is counted
 * (lc3gpu_encoder_size_clamps).  The carried state is that of the uniform calls: sized and uniform calls may alternate on a handle, and a
 * sized call whose sizes all equal n gives the bytes of lc3gpu_encode at nbytes = n.  The call always runs unsplit (LC3GPU_SPLIT is
 * ignored) with the one-lane-per-frame packer (LC3GPU_PACK_PC is ignored).  Asynchronous on hip_stream. */
int lc3gpu_encode_vbr(lc3gpu_encoder *enc, const int16_t *d_pcm, uint8_t *d_out, const uint16_t *d_nbytes, int slot_bytes,
                      int n_frames, void *hip_stream);
/* sticky count of the frame sizes lc3gpu_encode_vbr has clamped into [20, slot_bytes] on this handle (waits for the handle's work in flight) */
int lc3gpu_encoder_size_clamps(lc3gpu_encoder *enc, uint64_t *out);

/* Mixed-configuration encoder: n_streams streams, each with its own rate, frame duration and frame size; 8 kHz streams are
 * refused (LC3GPU_EUNSUPPORTED, as lc3gpu_encoder_create).  lc3gpu_encode_mixed encodes n_frames frames of every stream
 * with one launch per kernel.  Ragged DEVICE buffers, streams in descriptor order, each stream planar:
 *   d_pcm  stream i at element offset n_frames * sum_{j<i} nf_j      (int16[n_frames][nf_i]; 4-byte aligned base)
 *   d_out  stream i at byte offset    n_frames * sum_{j<i} nbytes_j  (uint8[n_frames][nbytes_i])
 * The per-frame calls, state blobs and timing work on a mixed handle as on a uniform one (channel index = descriptor
 * index); lc3gpu_encode / _range / _layout do not (LC3GPU_EINVAL). */
int lc3gpu_encoder_create_mixed(lc3gpu_encoder **out, int n_streams, const lc3gpu_stream_desc *descs);
int lc3gpu_encoder_create_mixed_spec(lc3gpu_encoder **out, int n_streams, const lc3gpu_stream_desc *descs, int spec_flags);
int lc3gpu_encode_mixed(lc3gpu_encoder *enc, const int16_t *d_pcm, uint8_t *d_out, int n_frames, void *hip_stream);
/* Batch over a LIST of a mixed handle's streams: the contract of lc3gpu_encode_list carried over to the mixed handle's buffers.  A server
 * that holds 7.5 ms and 10 ms streams side by side cannot advance them by the same number of frames per call (four 7.5 ms frames fall into
 * the 30 ms of three 10 ms frames): every tick it names the streams that are due, of any configurations, and gets ONE launch per kernel.
 *   channels  HOST int32[n_list]: entry i is a descriptor index (the mixed handle's channel index); any order, no channel twice.  The array
 *             may be reused as soon as the call returns (pinned copy of the handle's own, sent in stream order: no host synchronisation)
 *   d_pcm     DEVICE, ragged and compact IN LIST ORDER -- the layout of lc3gpu_encode_mixed with the call's list in place of the descriptor
 *             list: item i at element offset n_frames * sum_{j<i} nf(channels[j]), int16[n_frames][nf_i]; 4-byte aligned base
 *   d_out     DEVICE: item i at byte offset n_frames * sum_{j<i} nbytes(channels[j]), uint8[n_frames][nbytes_i]; every stream is encoded
 *             at the frame size of its descriptor (no nbytes argument)
 * Checked on the host before anything is queued: an index outside [0, n_streams) or named twice: LC3GPU_ECHANNEL; null pointers, a negative
 * n_list, misaligned PCM, a UNIFORM handle: LC3GPU_EINVAL; n_frames <= 0: LC3GPU_ELENGTH.  A call that returns an error has launched nothing,
 * written nothing and changed no channel; n_list = 0 launches nothing and returns LC3GPU_OK.  A bound handle takes the call on its bound
 * stream only; LC3GPU_EPAIR as for the other batch calls.  Every listed channel advances by n_frames frames exactly as under
 * lc3gpu_encode_mixed; every channel not listed keeps its state blob byte for byte.  Channels reset by lc3gpu_encoder_reset_channels start
 * from the constructed state inside the same launch as the carried ones (no extra launch).  Mixed-list, lc3gpu_encode_mixed and *_frame
 * calls may alternate on a handle; a list 0 .. n_streams-1 gives the bytes of lc3gpu_encode_mixed.  Groups of the handle without a listed
 * stream take no workgroups.  8 kHz streams: refused at encoder creation as ever, allowed on the decoder.  Asynchronous on hip_stream,
 * ordered after the handle's earlier work.
 * NOT provided by the mixed-list calls (out of scope): the interleaved layout, a frame size per frame (lc3gpu_*_vbr), the host-resident
 * calls (lc3gpu_*_host) and the pipeline object.  (n_frames holds for every item of a call and every stream is coded at its
 * descriptor's size; a frame count per listed channel and a frame size per call are what lc3gpu_encode_mixed_items /
 * lc3gpu_decode_mixed_items below provide.)  The interleaved layout is what lc3gpu_encode_mixed_mc_items / lc3gpu_decode_mixed_mc_items
 * provide. */
int lc3gpu_encode_mixed_list(lc3gpu_encoder *enc, const int32_t *channels, int n_list, const int16_t *d_pcm, uint8_t *d_out, int n_frames,
                             void *hip_stream);
/* Batch over a list of ITEMS of a mixed handle: a frame count and a frame size per listed stream.  The reference's caller calls
 * encode_frame / decode_frame once per (channel, frame) with a slice whose length selects the size (encoder/lc3_encoder.rs:65,175-191,
 * decoder/lc3_decoder.rs:85,217-234); a 30 ms tick of a server -- four frames of every 7.5 ms stream, three of every 10 ms stream --, a
 * decoder behind jitter buffers that owes one stream one frame and another three, a stream whose bitrate adapts: each is ONE call.
 * The contract of lc3gpu_encode_mixed_list, with these differences:
 *   items     HOST lc3gpu_item[n_items], any order, no channel twice; may be reused as soon as the call returns.  Item i: `channel` a
 *             descriptor index, `n_frames` >= 1 the frames of this stream in this call, `nbytes` the frame size of ALL of them (0 = the
 *             descriptor's; the state and the state blob do not depend on the size, so a stream may change it from call to call),
 *             `reserved` 0
 *   buffers   DEVICE, ragged and compact in list order.  With nf_j / nbytes_j the frame length / effective frame size of item j:
 *               d_pcm  item i at element offset sum_{j<i} n_frames_j * nf_j,     int16[n_frames_i][nf_i]
 *               d_out  item i at byte offset    sum_{j<i} n_frames_j * nbytes_j, uint8[n_frames_i][nbytes_i]
 *               flags  (decoder) item i at      sum_{j<i} n_frames_j,            uint8[n_frames_i], one per frame
 *             nf is even for every configuration, so a 4-byte aligned d_pcm base keeps every item aligned
 *   checks    everything on the host before anything is queued; a refused call has launched nothing, written nothing, advanced no
 *             channel and consumed no pending reset:
 *               channel out of range or named twice                  LC3GPU_ECHANNEL
 *               n_frames < 1                                         LC3GPU_ELENGTH
 *               nbytes not 0 and outside 20..400 (encoder)           LC3GPU_ELENGTH
 *               nbytes not 0 and outside 1..400 (decoder)            LC3GPU_ELENGTH
 *               more than 2^31 - 1 frames in one call                LC3GPU_ELENGTH
 *               reserved != 0, a null pointer, n_items < 0,
 *               misaligned PCM, a UNIFORM handle, a bound handle
 *               on another stream                                    LC3GPU_EINVAL
 *               n_items == 0                                         LC3GPU_OK (nothing launched)
 *             LC3GPU_EPAIR and LC3GPU_EUNSUPPORTED (a group without a compile-time view) as for lc3gpu_*_mixed_list
 *   state     a listed channel advances by its own n_frames, exactly as that many reference calls at that size advance it; channels not
 *             listed keep their blob (and their PLC count) byte for byte; channels reset by lc3gpu_*_reset_channels start fresh inside
 *             the same launch
 *   mixing    items, mixed-list, lc3gpu_*_mixed and *_frame calls may alternate on a handle; a call whose items all have n_frames = T
 *             and nbytes = 0 gives the bytes and the PCM of lc3gpu_*_mixed_list with n_frames = T
 *   launches  the items are bucketed by (configuration, effective nbytes, n_frames); ONE launch per kernel per 24 buckets (a call with
 *             more buckets runs as consecutive launch sets on the same stream, with one upload and one host check for all of them)
 * NOT provided (out of scope): a size per FRAME within an item, the interleaved layout, the host-resident calls, the pipeline object,
 * uniform handles.  The interleaved layout is what lc3gpu_encode_mixed_mc_items / lc3gpu_decode_mixed_mc_items below provide. */
typedef struct lc3gpu_item {
    int32_t channel;  /* descriptor index of the mixed handle */
    int32_t n_frames; /* >= 1: frames of this stream in this call */
    int32_t nbytes;   /* frame size for this call; 0 = the descriptor's */
    int32_t reserved; /* 0 */
} lc3gpu_item;
#ifdef __cplusplus
static_assert(sizeof(lc3gpu_item) == 16, "lc3gpu_item is 16 bytes");
#else
_Static_assert(sizeof(lc3gpu_item) == 16, "lc3gpu_item is 16 bytes");
#endif
int lc3gpu_encode_mixed_items(lc3gpu_encoder *enc, const lc3gpu_item *items, int n_items, const int16_t *d_pcm, uint8_t *d_out,
                              void *hip_stream);
/* Batch over a list of MULTI-CHANNEL items of a mixed handle: WAV sample order in, frame order out.  A stereo or multi-channel stream's
 * PCM arrives as L R L R and its frames leave as the channels' frames back to back -- the order the reference's file drivers read and
 * write (examples/encode.rs:96-115, examples/decode.rs:93-118) and the order of a multi-channel LC3 SDU.  An mc item names the C
 * descriptors of one such stream; the kernels read and write the interleaved buffers themselves, so a tick needs no de-interleave or
 * multiplex pass around the call.  The contract of lc3gpu_encode_mixed_items (which see), with these differences:
 *   items     HOST lc3gpu_mc_item[n_items], any order, no channel in two items; may be reused as soon as the call returns.  Item i:
 *             descriptors `first_channel` .. `first_channel + n_channels - 1` are the stream's channels 0 .. C-1, `n_channels` 1..8,
 *             `n_frames` >= 1 the frames of EVERY channel of the stream in this call, `nbytes` the frame size of every channel for this
 *             call (0 = the descriptors', which must then be equal)
 *   buffers   DEVICE, compact in list order, each item in the layout of LC3GPU_LAYOUT_INTERLEAVED.  With C_j, T_j, nf_j, nb_j the
 *             channel count, frame count, frame length and effective frame size of item j:
 *               d_pcm  item i at element sum_{j<i} T_j * nf_j * C_j,  int16[T_i][nf_i][C_i]
 *               d_out  item i at byte    sum_{j<i} T_j * C_j * nb_j,  uint8[T_i][C_i][nb_i]
 *               flags  (decoder) item i at sum_{j<i} T_j * C_j,       uint8[T_i][C_i]
 *             nf is even, so a 4-byte aligned d_pcm base keeps every item's base 4-byte aligned; a single channel of an item with
 *             C > 1 is only 2-byte aligned and is read and written with 16-bit accesses, as in lc3gpu_*_layout
 *   checks    on the host before anything is queued; a refused call has launched nothing, written nothing, advanced no channel and
 *             consumed no pending reset:
 *               a channel range outside [0, n_streams), a channel
 *               named by two items                                   LC3GPU_ECHANNEL
 *               n_channels outside 1..8                              LC3GPU_EINVAL
 *               channels of one item that differ in fs_hz or
 *               frame_us (lc3_encoder.rs:117-124: one configuration) LC3GPU_EINVAL
 *               nbytes == 0 while the item's descriptors differ in
 *               nbytes (one num_bytes_per_channel)                   LC3GPU_ELENGTH
 *               n_frames < 1                                         LC3GPU_ELENGTH
 *               nbytes not 0 and outside 20..400 (encoder)           LC3GPU_ELENGTH
 *               nbytes not 0 and outside 1..400 (decoder)            LC3GPU_ELENGTH
 *               more than 2^31 - 1 channel-frames in one call        LC3GPU_ELENGTH
 *               a null pointer, n_items < 0, misaligned PCM, a
 *               UNIFORM handle, a bound handle on another stream     LC3GPU_EINVAL
 *               n_items == 0                                         LC3GPU_OK (nothing launched)
 *             LC3GPU_EPAIR and LC3GPU_EUNSUPPORTED as for lc3gpu_*_mixed_items
 *   state     every channel of an item advances exactly as under an items call that lists it alone with the same n_frames and nbytes:
 *             an mc call gives the bytes, the PCM and the per-channel blobs of lc3gpu_*_mixed_items on the de-interleaved buffers, and
 *             the results of the items call itself when every n_channels is 1.  Channels not listed keep their blob and their PLC
 *             count byte for byte; channels noted by lc3gpu_*_reset_channels start fresh inside the same launch
 *   mixing    mc-items, items, mixed-list, lc3gpu_*_mixed and *_frame calls may alternate on a handle
 *   launches  as for the items calls: the items' CHANNELS are bucketed by (configuration, effective nbytes, n_frames), ONE launch per
 *             kernel per 24 buckets; the channel count is not part of the key
 * NOT provided (out of scope): a size per frame, the host-resident calls, the pipeline object, uniform handles (their interleaved
 * layout is lc3gpu_encode_layout / lc3gpu_decode_layout). */
typedef struct lc3gpu_mc_item {
    int32_t first_channel; /* descriptor index of the stream's channel 0 */
    int32_t n_channels;    /* 1..8: descriptors first_channel .. first_channel + n_channels - 1 */
    int32_t n_frames;      /* >= 1: frames of EVERY channel of the stream in this call */
    int32_t nbytes;        /* frame size of every channel for this call; 0 = the descriptors' (then all equal) */
} lc3gpu_mc_item;
#ifdef __cplusplus
static_assert(sizeof(lc3gpu_mc_item) == 16, "lc3gpu_mc_item is 16 bytes");
#else
_Static_assert(sizeof(lc3gpu_mc_item) == 16, "lc3gpu_mc_item is 16 bytes");
#endif
int lc3gpu_encode_mixed_mc_items(lc3gpu_encoder *enc, const lc3gpu_mc_item *items, int n_items, const int16_t *d_pcm, uint8_t *d_out,
                                 void *hip_stream);
/* Batch over a list of VIEWS of a mixed handle: frames and PCM read and written IN PLACE.  A server's data never lies compact in list
 * order: received frames sit in per-stream jitter rings of fixed-size slots behind packet headers, PCM sits in per-stream rings or in a
 * capture buffer with more channels than the stream uses, and which streams are due changes every tick.  A view is an item that also
 * says where its data lies, so a tick needs no gather or scatter pass around the call.  The contract of lc3gpu_encode_mixed_items (which
 * see), with these differences:
 *   views     HOST lc3gpu_view[n_views], any order, no channel twice; may be reused as soon as the call returns.  `channel`, `n_frames`
 *             and `nbytes` as in lc3gpu_item; the other fields place the view's frames
 *   placement with nf the frame length and nb the effective frame size of the view:
 *               sample n of frame t   d_pcm[pcm_off + t * pcm_pitch + n * pcm_stride]
 *               frame t's bytes       d_out / d_in [byte_off + t * byte_pitch ..  + nb)
 *               frame t's flag        d_bad_frame[flag_off + t * flag_pitch]   (decoder, and only when d_bad_frame is given)
 *             a pitch of 0 stands for the compact one: nf * pcm_stride, nb, 1.  pcm_stride 1 is a planar stream and is read and written
 *             with 32-bit accesses (pcm_off and pcm_pitch even, d_pcm 4-byte aligned); pcm_stride C >= 2 is one channel of C in WAV
 *             sample order, 16-bit accesses (d_pcm 2-byte aligned).  The encoder's history for frame t > 0 is the tail of frame t-1
 *             wherever that frame lies.  Only a frame's own nb bytes and nf samples are written: every byte and sample between and
 *             around them is left as it was
 *   sizes     pcm_elems, out_bytes / in_bytes, n_flags: the extents of the caller's buffers in elements, bytes and flags.  EVERY sample,
 *             byte and flag of every frame of every view is checked against them on the host, in 64-bit arithmetic that cannot
 *             overflow; a call that would touch anything outside is refused and never reaches the device
 *   overlap   inputs may overlap freely (two views may read the same PCM).  Output ranges of different views may INTERLEAVE: a stereo SDU
 *             is two views with byte_pitch = 2 * nb whose byte_off are nb apart.  Frames that truly overlap on output are the caller's
 *             error: the content of the overlapping bytes or samples is then unspecified; every write is still inside the checked extents
 *   checks    on the host before anything is queued; a refused call has launched nothing, written nothing, advanced no channel and
 *             consumed no pending reset:
 *               channel out of range or named twice                  LC3GPU_ECHANNEL
 *               n_frames < 1                                         LC3GPU_ELENGTH
 *               nbytes not 0 and outside 20..400 (encoder)           LC3GPU_ELENGTH
 *               nbytes not 0 and outside 1..400 (decoder)            LC3GPU_ELENGTH
 *               more than 2^31 - 1 frames in one call                LC3GPU_ELENGTH
 *               any sample, byte or flag of any frame of a view
 *               outside [0, pcm_elems), [0, out_bytes / in_bytes)
 *               or [0, n_flags)                                      LC3GPU_ELENGTH
 *               pcm_stride outside 1..8                              LC3GPU_EINVAL
 *               a negative offset                                    LC3GPU_EINVAL
 *               a non-zero pitch below its minimum (nf * pcm_stride,
 *               nb, 1)                                               LC3GPU_EINVAL
 *               reserved != 0                                        LC3GPU_EINVAL
 *               pcm_stride == 1 with an odd pcm_off, an odd
 *               pcm_pitch or a d_pcm base not 4-byte aligned         LC3GPU_EINVAL
 *               pcm_stride >= 2 with a d_pcm base not 2-byte aligned LC3GPU_EINVAL
 *               a null pointer, n_views < 0, a UNIFORM handle, a
 *               bound handle on another stream                       LC3GPU_EINVAL
 *               n_views == 0                                         LC3GPU_OK (nothing launched)
 *             LC3GPU_EPAIR and LC3GPU_EUNSUPPORTED as for lc3gpu_*_mixed_items
 *   state     exactly that of the items calls.  Two equivalences are part of the contract: views whose placements are the items call's
 *             prefix sums (pcm_stride 1, all pitches 0) give the bytes, the PCM, the state blobs and the PLC counts of
 *             lc3gpu_*_mixed_items; views that spell out an mc item's channels (channel c of C at bases P, B, F: pcm_off = P + c,
 *             pcm_stride = C, pcm_pitch = nf * C, byte_off = B + c * nb, byte_pitch = C * nb, flag_off = F + c, flag_pitch = C) give
 *             those of lc3gpu_*_mixed_mc_items
 *   mixing    views, mc-items, items, mixed-list, lc3gpu_*_mixed and *_frame calls may alternate on a handle
 *   launches  as for the items calls: the bucket key is (configuration, effective nbytes, n_frames), placement is no part of it; ONE
 *             launch per kernel per 24 buckets, one upload, one host check
 * NOT provided (out of scope): a size per frame within a view, ring wrap inside one view (the caller sizes the ring so that a tick does
 * not wrap, or names the two parts in two calls), strides above 8, the host-resident calls, the pipeline object, uniform handles. */
typedef struct lc3gpu_view {
    int32_t channel;     /* descriptor index of the mixed handle */
    int32_t n_frames;    /* >= 1 */
    int32_t nbytes;      /* frame size this call; 0 = the descriptor's */
    int32_t pcm_stride;  /* elements between two samples of a frame: 1..8 (1 = planar; C = one channel of C in WAV order) */
    int64_t pcm_off;     /* element index of sample 0 of frame 0 in d_pcm */
    int64_t byte_off;    /* byte index of frame 0 in d_out / d_in */
    int64_t flag_off;    /* decoder: index of frame 0's flag in d_bad_frame (ignored when that is NULL, and by the encoder) */
    int32_t pcm_pitch;   /* elements from frame t to frame t+1; 0 = nf * pcm_stride; otherwise >= nf * pcm_stride */
    int32_t byte_pitch;  /* bytes from frame t to frame t+1; 0 = effective nbytes; otherwise >= effective nbytes */
    int32_t flag_pitch;  /* 0 = 1; otherwise >= 1 */
    int32_t reserved[3]; /* 0 */
} lc3gpu_view;
#ifdef __cplusplus
static_assert(sizeof(lc3gpu_view) == 64, "lc3gpu_view is 64 bytes");
#else
_Static_assert(sizeof(lc3gpu_view) == 64, "lc3gpu_view is 64 bytes");
#endif
int lc3gpu_encode_mixed_views(lc3gpu_encoder *enc, const lc3gpu_view *views, int n_views, const int16_t *d_pcm, size_t pcm_elems,
                              uint8_t *d_out, size_t out_bytes, void *hip_stream);

/* per-channel state blobs (checkpoint / CPU cross-checks): size per channel, device->host copy, host->device.
 * nbytes must equal state_size * num_channels (LC3GPU_ELENGTH otherwise); both calls synchronise the device.  A channel's blob
 * starts with a 16-byte header {magic "LC3E" / "LC3D", layout version, payload size, fs_hz, frame duration, spec_flags}: loading
 * a blob saved by a handle of another configuration, another stream-descriptor order, the other side or another library version
 * returns LC3GPU_EINVAL instead of decoding garbage. */
size_t lc3gpu_encoder_state_size(const lc3gpu_encoder *enc);
int lc3gpu_encoder_state_save(lc3gpu_encoder *enc, void *host_dst, size_t nbytes);
int lc3gpu_encoder_state_load(lc3gpu_encoder *enc, const void *host_src, size_t nbytes);
/* the same for the channels named in a HOST list: blob i (state_size bytes, the format above) belongs to channels[i]; nbytes must be
 * n * state_size (LC3GPU_ELENGTH).  A slice of a whole-handle save loads through here and the other way round: a stream moves to another
 * handle.  The header check applies per blob, before any channel is written.  LC3GPU_ECHANNEL for an index out of range; they synchronise
 * the device as the whole-handle calls do. */
int lc3gpu_encoder_state_save_channels(lc3gpu_encoder *enc, const int32_t *channels, int n, void *host_dst, size_t nbytes);
int lc3gpu_encoder_state_load_channels(lc3gpu_encoder *enc, const int32_t *channels, int n, const void *host_src, size_t nbytes);

/* ---- decoder ------------------------------------------------------------------------------------ */
/* Lc3Decoder::new (lc3_decoder.rs:181-215) */
int lc3gpu_decoder_create(lc3gpu_decoder **out, int num_channels, int frame_us, int fs_hz);
int lc3gpu_decoder_destroy(lc3gpu_decoder *dec);
int lc3gpu_decoder_reset(lc3gpu_decoder *dec);

/* Lc3Decoder::decode_frame (lc3_decoder.rs:217-234), host buffers.  num_bits_per_audio_sample must be 16. */
int lc3gpu_decode_frame(lc3gpu_decoder *dec, int num_bits_per_audio_sample, int channel_index,
                        const uint8_t *buf_in, int nbytes, int16_t *samples_out, int n_samples);

/* Batch decode, DEVICE pointers, stream-major:
 *   d_in   uint8[num_channels][n_frames][nbytes]
 *   d_pcm  int16[num_channels][n_frames][nf]      (4-byte aligned)
 *   d_bad_frame  optional uint8[num_channels][n_frames]: non-zero marks a lost frame -> concealment
 *                (external bad-frame indicator; NULL = none) */
int lc3gpu_decode(lc3gpu_decoder *dec, const uint8_t *d_in, const uint8_t *d_bad_frame, int16_t *d_pcm, int nbytes,
                  int n_frames, void *hip_stream);
int lc3gpu_decode_range(lc3gpu_decoder *dec, int first_channel, int n_channels, const uint8_t *d_in,
                        const uint8_t *d_bad_frame, int16_t *d_pcm, int nbytes, int n_frames, void *hip_stream);
/* Batch decode over a LIST of channels: the contract of lc3gpu_encode_list (which see: host list, compact planar device buffers, host-side
 * checks, out-of-scope list) with d_in uint8[n_list][n_frames][nbytes], d_bad_frame uint8[n_list][n_frames] or NULL, d_pcm
 * int16[n_list][n_frames][nf]; nbytes / n_frames as lc3gpu_decode.  Channels not listed keep their state and their PLC count. */
int lc3gpu_decode_list(lc3gpu_decoder *dec, const int32_t *channels, int n_list, const uint8_t *d_in, const uint8_t *d_bad_frame,
                       int16_t *d_pcm, int nbytes, int n_frames, void *hip_stream);
/* as lc3gpu_encoder_reset_channels (the reference builds a new DecoderChannel); the channels' PLC counts go to zero with their reset */
int lc3gpu_decoder_reset_channels(lc3gpu_decoder *dec, const int32_t *channels, int n);
/* Batch decode with a frame size per frame: d_nbytes[c][t] is what the reference's buf_in.len() is for frame t of channel c
 * (lc3_decoder.rs:85).  DEVICE pointers, planar, every channel of the handle:
 *   d_in      uint8[num_channels][n_frames][slot_bytes]  frame (c, t) is the first d_nbytes[c][t] bytes of its slot
 *   d_nbytes  uint16[num_channels][n_frames]
 *   d_bad_frame, d_pcm                                   as lc3gpu_decode
 * slot_bytes 1 ... 400, else LC3GPU_ELENGTH.  Null d_in / d_nbytes / d_pcm, misaligned PCM and mixed handles: LC3GPU_EINVAL.  An entry of
 * 0 is an empty buf_in: the frame is concealed (the reference does the same, with nbits = 0 in the post-filter); an entry above
 * slot_bytes is treated as 0.  A frame flagged in d_bad_frame is concealed with its own size as nbits.  Concealed frames count in
 * lc3gpu_decoder_plc_events.  The carried state is that of the uniform calls (they may alternate on a handle), and a sized call whose
 * entries all equal n gives the PCM of lc3gpu_decode at nbytes = n.  The call always runs unsplit (LC3GPU_SPLIT is ignored) with the
 * one-lane-per-frame parser (LC3GPU_PARSE_PC is ignored); LC3GPU_RECON selects the reconstruction form as for lc3gpu_decode. */
int lc3gpu_decode_vbr(lc3gpu_decoder *dec, const uint8_t *d_in, const uint16_t *d_nbytes, const uint8_t *d_bad_frame, int16_t *d_pcm,
                      int slot_bytes, int n_frames, void *hip_stream);
/* Frame inspection: the side information and the decode status of every frame of a batch, without a handle (the reference's
 * side_info_reader::read, decoder/side_info_reader.rs:29, needs only the configuration; read_frame, decoder/lc3_decoder.rs:165-178, returns
 * the error that decode swallows at :138).  DEVICE pointers, a flat list of n_frames frames:
 *   d_in         uint8[n_frames][slot_bytes]  frame i is the first d_nbytes[i] bytes of slot i (every frame slot_bytes long when d_nbytes is
 *                                             NULL): planar and interleaved batches and the slots of the _vbr calls alike
 *   d_nbytes     uint16[n_frames] or NULL
 *   d_bad_frame  uint8[n_frames] or NULL      as lc3gpu_decode
 *   d_info       lc3gpu_frame_info[n_frames]  one 128-byte record per frame
 * Any of the 12 configurations (8 kHz included).  slot_bytes 1 ... 400, else LC3GPU_ELENGTH; null d_in / d_info, a negative n_frames or an
 * unknown configuration: LC3GPU_EINVAL; n_frames = 0 launches nothing.  Asynchronous on hip_stream, like the batch calls.
 *
 * The status of a frame, by precedence: FLAGGED (d_bad_frame[i] != 0: its bytes are not read), EMPTY (a d_nbytes entry of 0 or above
 * slot_bytes), then the frame's own: OK, SIDE_INFO + k for SideInfoError k, ARITH + k for ArithmeticDecodeError k (enum order of the
 * reference: 1 BufferReaderError, 2 BandwidthIdxOutOfRange, 3 LastNonZeroTupleGreaterThanYLen, 4 PlcTriggerSns1OutOfRange,
 * 5 PlcTriggerSns2OutOfRange; 1 ArithmeticCodec, 2 TnsOrder, 3 TnsCoef, 4 SpectralData, 5 SpectralBoolData, 6 NegativeResidualNumBits,
 * 7 ResidualData, 8 ResidualBoolDataOverflow -- 1, 7 and 8 cannot occur once the side information has parsed).
 * The contract: status != 0 exactly when lc3gpu_decode / lc3gpu_decode_vbr conceal that frame, given the same bytes, sizes and flags.  The
 * one exception is a parser wave pair that gave up on its partner, which lc3gpu_decoder_pair_timeouts reports. */
#define LC3GPU_FRAME_OK 0
#define LC3GPU_FRAME_FLAGGED 1
#define LC3GPU_FRAME_EMPTY 2
#define LC3GPU_FRAME_SIDE_INFO 16
#define LC3GPU_FRAME_ARITH 32
typedef struct lc3gpu_frame_info {
    int32_t status; /* LC3GPU_FRAME_* */
    int32_t nbytes; /* the size the decoder takes for this frame: slot_bytes or d_nbytes[i]; 0 for EMPTY */
    /* side_info_reader::read (decoder/side_info.rs:20-31): valid when status is OK or LC3GPU_FRAME_ARITH + k, else 0 */
    int32_t bandwidth, lastnz, lsb_mode, global_gain_index, num_tns_filters, rc_order_ari_input[2];
    int32_t sns_ind_lf, sns_ind_hf, sns_ls_inda, sns_ls_indb;
    uint32_t sns_idx_a, sns_idx_b;
    int32_t sns_submode_lsb, sns_submode_msb, sns_g_ind;
    int32_t pitch_present, ltpf_active, pitch_index, noise_factor;
    /* arithmetic_codec::decode (decoder/arithmetic_codec.rs:99-107): valid when status is OK, else 0 */
    int32_t rc_order[2], n_residual_bits, noise_filling_seed, is_zero_frame;
    uint8_t rc_i[16];
    int32_t reserved; /* 0 */
} lc3gpu_frame_info;
#ifdef __cplusplus
static_assert(sizeof(lc3gpu_frame_info) == 128, "lc3gpu_frame_info is 128 bytes");
#else
_Static_assert(sizeof(lc3gpu_frame_info) == 128, "lc3gpu_frame_info is 128 bytes");
#endif
int lc3gpu_inspect(int frame_us, int fs_hz, const uint8_t *d_in, const uint16_t *d_nbytes, const uint8_t *d_bad_frame, int slot_bytes,
                   int n_frames, lc3gpu_frame_info *d_info, void *hip_stream);
/* same as lc3gpu_decode with the buffers (and the flag array) in `layout` (LC3GPU_LAYOUT_*) */
int lc3gpu_decode_layout(lc3gpu_decoder *dec, int layout, const uint8_t *d_in, const uint8_t *d_bad_frame, int16_t *d_pcm,
                         int nbytes, int n_frames, void *hip_stream);

/* Mixed-configuration decoder (see lc3gpu_encoder_create_mixed; 8 kHz streams are allowed).  Ragged buffers as there:
 * d_in like the encoder's d_out, d_pcm like its d_pcm; d_bad_frame (optional) uint8[n_streams][n_frames] in descriptor order. */
int lc3gpu_decoder_create_mixed(lc3gpu_decoder **out, int n_streams, const lc3gpu_stream_desc *descs);
int lc3gpu_decode_mixed(lc3gpu_decoder *dec, const uint8_t *d_in, const uint8_t *d_bad_frame, int16_t *d_pcm, int n_frames,
                        void *hip_stream);
/* Batch decode over a LIST of a mixed handle's streams: the contract of lc3gpu_encode_mixed_list (which see: host list of descriptor
 * indices, ragged device buffers compact in list order, host-side checks, what is out of scope) with d_in like that call's d_out, d_pcm like
 * its d_pcm and d_bad_frame uint8[n_list][n_frames] in list order or NULL.  Channels not listed keep their state and their PLC count;
 * channels reset by lc3gpu_decoder_reset_channels start from the constructed state inside the same launch, without the device
 * synchronisation lc3gpu_decode_mixed spends on materialising them. */
int lc3gpu_decode_mixed_list(lc3gpu_decoder *dec, const int32_t *channels, int n_list, const uint8_t *d_in, const uint8_t *d_bad_frame,
                             int16_t *d_pcm, int n_frames, void *hip_stream);
/* Batch decode over a list of ITEMS of a mixed handle: the contract of lc3gpu_encode_mixed_items (which see) with d_in like that call's
 * d_out, d_pcm like its d_pcm, d_bad_frame one flag per frame in item order or NULL, and frame sizes 1..400 (a frame too short to hold
 * side information is concealed and counted, as everywhere). */
int lc3gpu_decode_mixed_items(lc3gpu_decoder *dec, const lc3gpu_item *items, int n_items, const uint8_t *d_in, const uint8_t *d_bad_frame,
                              int16_t *d_pcm, void *hip_stream);
/* Batch decode over a list of MULTI-CHANNEL items of a mixed handle: the contract of lc3gpu_encode_mixed_mc_items (which see) with d_in
 * like that call's d_out (uint8[T][C][nbytes] per item), d_pcm like its d_pcm (int16[T][nf][C] per item), d_bad_frame uint8[T][C] per
 * item or NULL, and frame sizes 1..400. */
int lc3gpu_decode_mixed_mc_items(lc3gpu_decoder *dec, const lc3gpu_mc_item *items, int n_items, const uint8_t *d_in,
                                 const uint8_t *d_bad_frame, int16_t *d_pcm, void *hip_stream);
/* Batch decode over a list of VIEWS of a mixed handle: the contract of lc3gpu_encode_mixed_views (which see) with d_in / in_bytes like that
 * call's d_out / out_bytes, d_pcm written where it reads, d_bad_frame / n_flags the flag array and its length (NULL: no flags are read and
 * flag_off, flag_pitch and n_flags are ignored), and frame sizes 1..400. */
int lc3gpu_decode_mixed_views(lc3gpu_decoder *dec, const lc3gpu_view *views, int n_views, const uint8_t *d_in, size_t in_bytes,
                              const uint8_t *d_bad_frame, size_t n_flags, int16_t *d_pcm, size_t pcm_elems, void *hip_stream);
/* Frame inspection over a list of VIEWS: the status and the side information of every frame of a tick, read where the frames lie and
 * written where their flags lie -- what lc3gpu_inspect reports, for the very lc3gpu_view array the tick passes to
 * lc3gpu_decode_mixed_views, in one launch and without a gather or scatter pass around it.  Inspection needs no codec handle (the
 * reference's side_info_reader::read needs only the configuration), so the streams' configurations are fixed once in an INSPECTOR, which
 * also owns the pinned upload ring and the device tables a handle-less call has nowhere to keep.
 *   create    descs: the array the caller passes to lc3gpu_decoder_create_mixed (copied): fs_hz one of the six rates (8 kHz included),
 *             frame_us 7500 or 10000 (LC3GPU_EINVAL otherwise), nbytes 1..400 (LC3GPU_ELENGTH otherwise); n_streams >= 1.  max_views >= 1
 *             is the most views one call may name (it sizes the ring and the tables once; LC3GPU_EINVAL below 1).  The inspector is bound
 *             to the device that is current at creation, is not thread-safe and is independent of every codec handle.  No device:
 *             LC3GPU_ENODEVICE
 *   views     HOST lc3gpu_view[n_views], any order; may be reused as soon as the call returns.  Read: channel (the descriptor index),
 *             n_frames, nbytes (0 = the descriptor's), byte_off, byte_pitch, flag_off, flag_pitch and reserved (0), each with the meaning
 *             it has in the decode call.  NOT read: pcm_stride, pcm_off, pcm_pitch -- a view the decode call would refuse for its PCM
 *             placement is not refused here
 *   placement with nb the effective frame size of the view:
 *               frame t's bytes        d_in[byte_off + t * byte_pitch ..  + nb)
 *               frame t's flag         d_bad_frame[flag_off + t * flag_pitch]   (when d_bad_frame is given)
 *               frame t's status byte  d_status[flag_off + t * flag_pitch]      (when d_status is given)
 *               frame t's record       d_info[flag_off + t * flag_pitch]        (when d_info is given; 128 bytes)
 *             the outputs follow the flag placement; a pitch of 0 stands for the compact one (nb, 1).  At least one of d_status and d_info
 *             must be given.  Only a frame's own status byte and record are written: every byte between and around them is left as it was
 *   repeats   a channel MAY be named by several views (inspection carries no state): the two parts of a ring that wraps are two views
 *             of one call.  Two views that write the same output index are the caller's error: the content there is unspecified, every
 *             write is still inside the checked extents
 *   written   two equivalences are part of the contract.  The record of a frame is, byte for byte, the record lc3gpu_inspect writes when
 *             called with the descriptor's (frame_us, fs_hz), slot_bytes = nb, d_nbytes = NULL, that frame's nb bytes and its flag
 *             (LC3GPU_FRAME_EMPTY therefore cannot occur); the status byte is that record's `status` (every status value fits a byte).
 *             And, as for lc3gpu_inspect: status != 0 exactly for the frames lc3gpu_decode_mixed_views conceals, given the same
 *             descriptors, views, bytes and flags (the pair-give-up exception stated there applies)
 *   checks    on the host before anything is queued; a refused call has launched nothing and written nothing:
 *               channel outside [0, n_streams)                       LC3GPU_ECHANNEL
 *               n_frames < 1                                         LC3GPU_ELENGTH
 *               nbytes not 0 and outside 1..400                      LC3GPU_ELENGTH
 *               more than 2^31 - 1 frames in one call                LC3GPU_ELENGTH
 *               n_views > max_views                                  LC3GPU_ELENGTH
 *               any byte, flag, status byte or record of any frame
 *               outside [0, in_bytes), [0, n_flags), [0, n_status),
 *               [0, n_info)                                          LC3GPU_ELENGTH
 *               a negative byte_off or flag_off                      LC3GPU_EINVAL
 *               a non-zero pitch below its minimum (nb, 1)           LC3GPU_EINVAL
 *               reserved != 0                                        LC3GPU_EINVAL
 *               both outputs NULL                                    LC3GPU_EINVAL
 *               null insp, views or d_in                             LC3GPU_EINVAL
 *               n_views < 0                                          LC3GPU_EINVAL
 *               d_info not 4-byte aligned                            LC3GPU_EINVAL
 *               an output array's address range ([d_status,
 *               + n_status), [d_info, + n_info * 128)) overlapping
 *               d_in's, d_bad_frame's or the other output's          LC3GPU_EINVAL
 *               n_views == 0                                         LC3GPU_OK (nothing launched)
 *             the extent check works in unsigned 64-bit arithmetic that cannot wrap; extents are checked only against the arrays that are
 *             given (n_flags, n_status, n_info of a NULL array are ignored).  HIP errors: LC3GPU_EHIP
 *   order     asynchronous on hip_stream, ordered as any kernel on that stream.  In the steady state the call does not synchronise the
 *             host; it waits for the oldest of its own uploads only when more calls are in flight than the ring has slots
 *   launches  ONE launch and ONE upload of O(views + workgroups) bytes per call, whatever mix of configurations, sizes and frame counts
 *             the views hold; with d_info == NULL one byte per frame leaves the device's compute units instead of 128
 * NOT provided (out of scope): a size per frame within a view, uniform handles and flat batches (lc3gpu_inspect is theirs), the pipeline
 * object, host-resident buffers. */
typedef struct lc3gpu_inspector lc3gpu_inspector;
int lc3gpu_inspector_create(lc3gpu_inspector **out, int n_streams, const lc3gpu_stream_desc *descs, int max_views);
int lc3gpu_inspector_destroy(lc3gpu_inspector *insp);
int lc3gpu_inspect_mixed_views(lc3gpu_inspector *insp, const lc3gpu_view *views, int n_views, const uint8_t *d_in, size_t in_bytes,
                               const uint8_t *d_bad_frame, size_t n_flags, uint8_t *d_status, size_t n_status, lc3gpu_frame_info *d_info,
                               size_t n_info, void *hip_stream);
/* Frame analysis over a list of VIEWS: the reconstructed spectrum, the 64 band energies and the total energy of every frame of a tick, read
 * where the frames lie and written at the frames' flag indices -- for the very lc3gpu_view array the tick passes to
 * lc3gpu_decode_mixed_views and lc3gpu_inspect_mixed_views, in one launch, without decoding to PCM.  Everything the decoder does up to the
 * input of its inverse transform (residual bits, noise filling, global gain, TNS synthesis, SNS gains: reference
 * decoder/lc3_decoder.rs:99-131) reads the frame and the configuration only, so the call needs no codec handle: the streams' configurations
 * are fixed once in an ANALYZER, which also owns the pinned upload ring, the device tables and the scratch columns the frames are rebuilt in.
 *   create    descs, n_streams and max_views exactly as for lc3gpu_inspector_create: fs_hz one of the six rates (8 kHz included), frame_us
 *             7500 or 10000 (LC3GPU_EINVAL otherwise), nbytes 1..400 (LC3GPU_ELENGTH otherwise); n_streams >= 1; max_views >= 1 is the
 *             most views one call may name (LC3GPU_EINVAL below 1).  max_frames >= 1 is the most frames one call may hold: it sizes,
 *             once, the scratch columns (one column of 648 words per frame, in device memory; LC3GPU_EINVAL below 1).  The analyzer is
 *             bound to the device that is current at creation, is not thread-safe and is independent of every codec handle and of the
 *             inspector.  No device: LC3GPU_ENODEVICE
 *   views     HOST lc3gpu_view[n_views], any order; may be reused as soon as the call returns.  Read and NOT read exactly as in
 *             lc3gpu_inspect_mixed_views: read are channel, n_frames, nbytes (0 = the descriptor's), byte_off, byte_pitch, flag_off,
 *             flag_pitch and reserved (0); NOT read: pcm_stride, pcm_off, pcm_pitch
 *   placement with nb the effective frame size of the view and i = flag_off + t * flag_pitch the OUTPUT INDEX of frame t:
 *               frame t's bytes         d_in[byte_off + t * byte_pitch ..  + nb)
 *               frame t's flag          d_bad_frame[i]                              (when d_bad_frame is given)
 *               frame t's energy        d_energy[i]                                 (when d_energy is given)
 *               frame t's band row      d_bands[i * LC3GPU_BANDS ..  + 64)           (when d_bands is given)
 *               frame t's spectrum row  d_spec[i * LC3GPU_SPEC_LINES ..  + 400)      (when d_spec is given)
 *             a pitch of 0 stands for the compact one (nb, 1).  At least one of the three outputs must be given.  Only a frame's own float
 *             and rows are written: everything between and around them is left as it was
 *   repeats   a channel MAY be named by several views (analysis carries no state): the two parts of a ring that wraps are two views of
 *             one call.  Two views that write the same output index are the caller's error: the content there is unspecified, every write
 *             is still inside the checked extents
 *   written   for a GOOD frame -- one for which lc3gpu_inspect_mixed_views reports status 0 -- with ne and nb its configuration's numbers of
 *             coded lines and of bands, I[] its band index table and x[k] the reference's x_hat after spectral_noise_shaping::decode:
 *               d_spec[i * 400 + k]  = x[k] for k < ne, 0.0f for ne <= k < 400: bit for bit the LC3GPU_DBG_SPEC dump of
 *                                      lc3gpu_decode_frame_debug
 *               d_bands[i * 64 + b]  = the encoder's band-energy formula applied to x (reference encoder/modified_dct.rs:140-152):
 *                                      e = 0.0f; for k in I[b] .. I[b + 1] - 1 ascending: e += x[k] * x[k] / (float)(I[b + 1] - I[b]);
 *                                      0.0f for nb <= b < 64
 *               d_energy[i]          = e = 0.0f; for k in 0 .. ne - 1 ascending: e += x[k] * x[k]
 *             in f32, one operation at a time: multiply, then divide, then add; nothing fused.  For a frame the decoder would CONCEAL
 *             (status != 0: flagged, side-information or arithmetic error): d_energy[i] = -1.0f -- an energy is never negative, so this is
 *             the marker -- and the frame's d_bands and d_spec rows are all 0.0f.  The analyzer does not conceal: concealment is the
 *             decoder's carried state, and this call has none.  Part of the contract: d_energy[i] < 0 exactly where
 *             lc3gpu_inspect_mixed_views writes a non-zero status, given the same descriptors, views, bytes and flags
 *   checks    on the host before anything is queued; a refused call has launched nothing and written nothing.  The whole refusal table of
 *             lc3gpu_inspect_mixed_views applies, with the three outputs in place of d_status / d_info:
 *               channel outside [0, n_streams)                       LC3GPU_ECHANNEL
 *               n_frames < 1                                         LC3GPU_ELENGTH
 *               nbytes not 0 and outside 1..400                      LC3GPU_ELENGTH
 *               more than 2^31 - 1 frames in one call                LC3GPU_ELENGTH
 *               more than max_frames frames in one call              LC3GPU_ELENGTH
 *               n_views > max_views                                  LC3GPU_ELENGTH
 *               any byte, flag, energy, band row or spectrum row of
 *               any frame outside [0, in_bytes), [0, n_flags),
 *               [0, n_energy), [0, n_bands), [0, n_spec)             LC3GPU_ELENGTH
 *               a negative byte_off or flag_off                      LC3GPU_EINVAL
 *               a non-zero pitch below its minimum (nb, 1)           LC3GPU_EINVAL
 *               reserved != 0                                        LC3GPU_EINVAL
 *               all three outputs NULL                               LC3GPU_EINVAL
 *               null an, views or d_in                               LC3GPU_EINVAL
 *               n_views < 0                                          LC3GPU_EINVAL
 *               d_energy or d_bands not 4-byte aligned               LC3GPU_EINVAL
 *               d_spec not 16-byte aligned                           LC3GPU_EINVAL
 *               an output array's address range ([d_energy,
 *               + n_energy * 4), [d_bands, + n_bands * 256), [d_spec,
 *               + n_spec * 1600)) overlapping d_in's, d_bad_frame's
 *               or another output's                                  LC3GPU_EINVAL
 *               n_views == 0                                         LC3GPU_OK (nothing launched)
 *             the extent check works in unsigned 64-bit arithmetic that cannot wrap; extents are checked only against the arrays that are
 *             given (n_flags, n_energy, n_bands, n_spec of a NULL array are ignored).  HIP errors: LC3GPU_EHIP
 *   order     asynchronous on hip_stream, ordered as any kernel on that stream.  In the steady state the call does not synchronise the
 *             host; it waits for the oldest of its own uploads only when more calls are in flight than the ring has slots.  The calls of
 *             ONE analyzer share its scratch columns: a call on another stream than the analyzer's previous call is ordered behind that
 *             call on the device (an event wait), as the codec handles order theirs
 *   launches  ONE launch and ONE upload of O(views) bytes per call, whatever mix of configurations, sizes and frame counts the views hold
 * NOT provided (out of scope): a size per frame within a view, uniform handles and flat batches, PCM-domain measures, concealed spectra,
 * host-resident buffers, the pipeline object. */
#define LC3GPU_BANDS 64        /* row length of d_bands (nb <= 64 for every configuration) */
#define LC3GPU_SPEC_LINES 400  /* row length of d_spec  (ne <= 400) */
typedef struct lc3gpu_analyzer lc3gpu_analyzer;
int lc3gpu_analyzer_create(lc3gpu_analyzer **out, int n_streams, const lc3gpu_stream_desc *descs, int max_views, int max_frames);
int lc3gpu_analyzer_destroy(lc3gpu_analyzer *an);
int lc3gpu_analyze_mixed_views(lc3gpu_analyzer *an, const lc3gpu_view *views, int n_views, const uint8_t *d_in, size_t in_bytes,
                               const uint8_t *d_bad_frame, size_t n_flags,
                               float *d_energy, size_t n_energy,   /* one float per output index, or NULL */
                               float *d_bands, size_t n_bands,     /* n_bands rows of LC3GPU_BANDS floats, or NULL */
                               float *d_spec, size_t n_spec,       /* n_spec rows of LC3GPU_SPEC_LINES floats, or NULL */
                               void *hip_stream);
/* Room mixes over two lists of VIEWS: the middle step of a mixing server's tick -- decode what every participant sent
 * (lc3gpu_decode_mixed_views), mix per room, encode what every participant gets (lc3gpu_encode_mixed_views) -- on the tick's own view
 * arrays, the PCM read where the decoder wrote it and written where the encoder reads it, in one launch: no gather or scatter pass runs
 * around the call.  The reference has no mixer; the anchor is what a reference caller does between decode_frame and encode_frame
 * (decoder/lc3_decoder.rs:217-234, encoder/lc3_encoder.rs:175-191): it sums the i16 samples it got in i32 and clamps to i16 as
 * decoder/output_scaling.rs:24 clamps.  The definition is all-integer, so the result does not depend on the order of summation.
 *   create    descs and n_streams are checked exactly as by lc3gpu_inspector_create: fs_hz one of the six rates (8 kHz included), frame_us
 *             7500 or 10000 (LC3GPU_EINVAL otherwise), nbytes 1..400 (LC3GPU_ELENGTH otherwise); n_streams >= 1.  Only fs_hz and frame_us
 *             are used afterwards.  max_views >= 1 bounds n_in + n_out of one call and sizes the pinned upload ring and its device twin
 *             once (LC3GPU_EINVAL below 1).  The mixer is bound to the device that is current at creation, is not thread-safe and is
 *             independent of every codec handle, of the inspector and of the analyzer.  No device: LC3GPU_ENODEVICE
 *   views     in_views and out_views are HOST arrays and may be reused as soon as the call returns: the arrays the tick passes to
 *             lc3gpu_decode_mixed_views and lc3gpu_encode_mixed_views.  Read: channel (index into the mixer's descriptors, giving the frame
 *             length nf and the rate), n_frames, pcm_off, pcm_stride, pcm_pitch and reserved (0).  NOT read: nbytes, byte_off, byte_pitch,
 *             flag_off, flag_pitch.  ins[i] belongs to in_views[i], outs[o] to out_views[o].  A mix carries no state: a channel and a
 *             placement may be named by any number of input views, so one stream can feed two rooms.  Two outputs that write the same
 *             sample are the caller's error: the content there is unspecified, every write is still inside the checked extents
 *   bus       a bus is a room: 0 <= bus < max_views.  All views of a bus, inputs and outputs, have the same fs_hz and the same sample
 *             count S = n_frames * nf: at one rate four 7.5 ms frames and three 10 ms frames mix; a 24 kHz / 10 ms and a 32 kHz / 7.5 ms
 *             stream (240 samples per frame both) do not, nor do 44.1 kHz and 48 kHz
 *   placement sample s of a view, 0 <= s < S, is d[pcm_off + (s / nf) * pitch + (s % nf) * pcm_stride] with pitch = pcm_pitch ? pcm_pitch
 *             : nf * pcm_stride: exactly the views calls' rule
 *   written   for every output o on bus b and every s, with in(i, s) the sample of input i:
 *               term(i, s)  = ((int32)in(i, s) * gain_q14[i] + 8192) >> 14      (arithmetic shift: round to nearest, ties upward)
 *               total(b, s) = sum of term(i, s) over the inputs i of bus b      (int32; 0 for a bus without inputs)
 *               out(o, s)   = clamp(total(b, s) - (minus[o] >= 0 ? term(minus[o], s) : 0), -32768, 32767)
 *             gain_q14 = 16384 is unity and gives term == in exactly.  minus is the index in in_views of the input this output does not
 *             hear -- the participant's own, which makes the N-1 mix --, -1 for none.  Only the S samples of an output view are written:
 *             everything between and around them is left as it was.  gain_q14 lies in -32768..32767, so |term| <= 65536; a bus holds at
 *             most 16384 inputs, so |total| <= 2^30 and the subtraction cannot leave int32
 *   checks    on the host before anything is queued; a refused call has launched nothing and written nothing:
 *               channel outside [0, n_streams)                       LC3GPU_ECHANNEL
 *               n_frames < 1                                         LC3GPU_ELENGTH
 *               more than 2^31 - 1 samples in one view               LC3GPU_ELENGTH
 *               any sample of any view outside [0, in_elems) /
 *               [0, out_elems)                                       LC3GPU_ELENGTH
 *               n_in + n_out > max_views                             LC3GPU_ELENGTH
 *               more than 16384 inputs on one bus                    LC3GPU_ELENGTH
 *               views of one bus with different S                    LC3GPU_ELENGTH
 *               views of one bus with different fs_hz                LC3GPU_EINVAL
 *               bus outside [0, max_views)                           LC3GPU_EINVAL
 *               gain_q14 outside -32768..32767                       LC3GPU_EINVAL
 *               minus outside [-1, n_in), or naming an input of
 *               another bus                                          LC3GPU_EINVAL
 *               pcm_stride outside 1..8                              LC3GPU_EINVAL
 *               a negative pcm_off                                   LC3GPU_EINVAL
 *               a non-zero pitch below nf * pcm_stride               LC3GPU_EINVAL
 *               reserved != 0                                        LC3GPU_EINVAL
 *               pcm_stride == 1 with an odd pcm_off, an odd pitch
 *               or a base not 4-byte aligned                         LC3GPU_EINVAL
 *               pcm_stride >= 2 with a base not 2-byte aligned       LC3GPU_EINVAL
 *               [d_pcm_in, + 2 * in_elems) and [d_pcm_out,
 *               + 2 * out_elems) overlapping                         LC3GPU_EINVAL
 *               a null mx; a null array whose count is not 0; a
 *               null PCM array whose views are not 0; negative counts LC3GPU_EINVAL
 *               n_out == 0                                           LC3GPU_OK (nothing launched)
 *               n_in == 0 with outputs                               LC3GPU_OK (the outputs are zeros)
 *             the extent check works in unsigned 64-bit arithmetic that cannot wrap.  The two arrays may not overlap because a workgroup
 *             must never overwrite what another still reads.  HIP errors: LC3GPU_EHIP
 *   order     asynchronous on hip_stream, ordered as any kernel on that stream.  The host waits for the oldest of its own uploads only
 *             when more calls are in flight than the ring has slots, as with the inspector
 *   launches  ONE launch and ONE upload of O(views) bytes per call, whatever mix of rates, durations, frame counts and room sizes
 * NOT provided (out of scope): resampling between rates, a gain per output, ramps across a tick, float or wider PCM, host-resident
 * buffers, the pipeline object, uniform handles. */
typedef struct lc3gpu_mixer lc3gpu_mixer;
typedef struct lc3gpu_mix_in {
    int32_t bus;      /* the room this input is heard in */
    int32_t gain_q14; /* -32768..32767; 16384 = unity */
} lc3gpu_mix_in;
typedef struct lc3gpu_mix_out {
    int32_t bus;   /* the room this output hears */
    int32_t minus; /* index in in_views of the input it does not hear (its own); -1 = none */
} lc3gpu_mix_out;
#ifdef __cplusplus
static_assert(sizeof(lc3gpu_mix_in) == 8, "lc3gpu_mix_in is 8 bytes");
static_assert(sizeof(lc3gpu_mix_out) == 8, "lc3gpu_mix_out is 8 bytes");
#else
_Static_assert(sizeof(lc3gpu_mix_in) == 8, "lc3gpu_mix_in is 8 bytes");
_Static_assert(sizeof(lc3gpu_mix_out) == 8, "lc3gpu_mix_out is 8 bytes");
#endif
int lc3gpu_mixer_create(lc3gpu_mixer **out, int n_streams, const lc3gpu_stream_desc *descs, int max_views);
int lc3gpu_mixer_destroy(lc3gpu_mixer *mx);
int lc3gpu_mix_mixed_views(lc3gpu_mixer *mx, const lc3gpu_view *in_views, const lc3gpu_mix_in *ins, int n_in, const int16_t *d_pcm_in,
                           size_t in_elems, const lc3gpu_view *out_views, const lc3gpu_mix_out *outs, int n_out, int16_t *d_pcm_out,
                           size_t out_elems, void *hip_stream);
/* Rate conversion over two lists of VIEWS: the step a room with a 16 kHz headset and a 48 kHz laptop needs on both sides of its mix --
 * decode (lc3gpu_decode_mixed_views), resample up, mix (lc3gpu_mix_mixed_views), resample down, encode (lc3gpu_encode_mixed_views) -- on
 * the tick's own view arrays, the PCM read where one array says and written where a second says, in one launch.  The reference has no
 * resampler between streams (its only one is the encoder's LTPF analysis); the definition below is all-integer, its result does not
 * depend on the order of summation, and tables/lc3_resample_tables.h (tools/gen_resample_tables.py) is part of it.
 *   create    frame_us is 7500 or 10000, fs_in_hz and fs_out_hz are each one of the six rates (LC3GPU_EINVAL otherwise).  fs_in_hz ==
 *             fs_out_hz is allowed for all six and is an exact copy: no delay, no state.  fs_in_hz != fs_out_hz with either side at 44100
 *             is LC3GPU_EUNSUPPORTED: an LC3 44.1 kHz frame is not 10 ms long, so such streams tick at another pace.  n_channels >= 1.
 *             max_views >= 1 bounds n_views of one call and sizes the pinned upload ring and its device twin once (LC3GPU_EINVAL below
 *             1).  The resampler is bound to the device that is current at creation, is not thread-safe and is independent of every codec
 *             handle, of the inspector, of the analyzer and of the mixer.  No device: LC3GPU_ENODEVICE
 *   views     in_views and out_views are HOST arrays and may be reused as soon as the call returns; in_views[i] and out_views[i] belong
 *             together.  Read from both: channel (index into the resampler's descriptors), n_frames, pcm_off, pcm_stride, pcm_pitch and
 *             reserved (0).  channel and n_frames must be equal in both (LC3GPU_EINVAL otherwise).  NOT read: nbytes, byte_off,
 *             byte_pitch, flag_off, flag_pitch: in_views can be the very array the tick gave lc3gpu_decode_mixed_views.  The resampler
 *             carries state, so a channel may be named once per call: twice is LC3GPU_ECHANNEL
 *   placement sample s of a view is d[pcm_off + (s / nf) * pitch + (s % nf) * pcm_stride] with pitch = pcm_pitch ? pcm_pitch : nf *
 *             pcm_stride: exactly the views calls' rule, with nf = nf_in, the frame length of (fs_in_hz, frame_us), for the input view and
 *             nf = nf_out, that of (fs_out_hz, frame_us), for the output view
 *   written   with g = gcd(fs_in_hz, fs_out_hz), L = fs_out_hz / g, M = fs_in_hz / g (twelve ratios, L and M in 1..6), S_in = n_frames *
 *             nf_in, S_out = n_frames * nf_out (S_out * M == S_in * L), T the ratio's taps per phase and c[p][j] its table; x[k], 0 <= k <
 *             S_in, the view's input in time order and x[k], -(T - 1) <= k < 0, the channel's history (zeros when fresh):
 *               for m in 0 .. S_out - 1:  u = m * M;  p = u % L;  b = u / L
 *                   acc(m) = sum over j in 0 .. T - 1 of c[p][j] * x[b - j]            (int32)
 *                   out(m) = clamp((acc(m) + 16384) >> 15, -32768, 32767)              (arithmetic shift)
 *               new history = the last T - 1 samples of (old history ++ x)
 *             Only the S_out samples of an output view are written: everything between and around them is left as it was.  A call always
 *             starts at phase 0, so frames may be split over calls and over views' n_frames in any way without changing one output
 *             sample.  The group delay is 8 samples of the lower of the two rates.  Every phase of every table sums to exactly 32768 (a
 *             constant stays that constant) and has sum |c| <= 65535 (60988 at most), so |acc| < 2^31 - 16384 and nothing wraps
 *   table     per ratio Q = max(L, M), N = 16 Q + 1, the prototype in float64 h[n] = L * 2 fc * sinc(2 fc (n - 8 Q)) * kaiser(N, beta =
 *             6.0)[n] with fc = 0.92 * 0.5 / Q; T = ceil(N / L); phase p, tap j is h[p + L j] (0 beyond N); each phase is scaled to sum
 *             1, times 32768, rounded to nearest, and the rounding residual is added to the phase's tap of largest magnitude.  The
 *             COMMITTED table is the definition
 *   state     a listed channel advances; a channel not listed keeps its history byte for byte.  lc3gpu_resampler_reset (all channels) and
 *             lc3gpu_resampler_reset_channels (LC3GPU_ECHANNEL for an index out of range, and then none is reset) wait for nothing and
 *             launch nothing: the named channels read a zero history inside their next launch.  A refused call has launched nothing,
 *             written nothing, advanced no channel and consumed no pending reset
 *   checks    on the host before anything is queued, for both views of every pair:
 *               channel outside [0, n_channels)                      LC3GPU_ECHANNEL
 *               a channel named twice in one call                    LC3GPU_ECHANNEL
 *               n_frames < 1                                         LC3GPU_ELENGTH
 *               more than 2^31 - 1 samples in one view               LC3GPU_ELENGTH
 *               any sample of any view outside [0, in_elems) /
 *               [0, out_elems)                                       LC3GPU_ELENGTH
 *               n_views > max_views                                  LC3GPU_ELENGTH
 *               more than 2^31 - 1 workgroups in the plan            LC3GPU_ELENGTH
 *               channel or n_frames differing within a pair          LC3GPU_EINVAL
 *               pcm_stride outside 1..8                              LC3GPU_EINVAL
 *               a negative pcm_off                                   LC3GPU_EINVAL
 *               a non-zero pitch below nf * pcm_stride               LC3GPU_EINVAL
 *               reserved != 0                                        LC3GPU_EINVAL
 *               pcm_stride == 1 with an odd pcm_off, an odd pitch
 *               or a base not 4-byte aligned                         LC3GPU_EINVAL
 *               pcm_stride >= 2 with a base not 2-byte aligned       LC3GPU_EINVAL
 *               [d_pcm_in, + 2 * in_elems) and [d_pcm_out,
 *               + 2 * out_elems) overlapping                         LC3GPU_EINVAL
 *               a null rs; a null array with n_views > 0; n_views < 0 LC3GPU_EINVAL
 *               n_views == 0                                         LC3GPU_OK (nothing launched)
 *             the extent check works in unsigned 64-bit arithmetic that cannot wrap.  HIP errors: LC3GPU_EHIP
 *   order     asynchronous on hip_stream.  Calls of one resampler share its histories: a call on another stream than the previous one's
 *             is ordered behind it by an event wait on the device, as the analyzer orders its calls.  The host waits for the oldest of
 *             its own uploads only when more calls are in flight than the ring has slots
 *   launches  ONE launch and ONE upload of O(views) bytes per call, whatever mix of ratios, durations and frame counts
 * NOT provided (out of scope): 44.1 kHz conversion, arbitrary ratios, state blobs, a channel twice in a call, float or wider PCM,
 * host-resident buffers, the pipeline object, uniform handles. */
typedef struct lc3gpu_rate_desc {
    int fs_in_hz;
    int fs_out_hz;
    int frame_us;
} lc3gpu_rate_desc; /* 12 bytes */
#ifdef __cplusplus
static_assert(sizeof(lc3gpu_rate_desc) == 12, "lc3gpu_rate_desc is 12 bytes");
#else
_Static_assert(sizeof(lc3gpu_rate_desc) == 12, "lc3gpu_rate_desc is 12 bytes");
#endif
typedef struct lc3gpu_resampler lc3gpu_resampler;
int lc3gpu_resampler_create(lc3gpu_resampler **out, int n_channels, const lc3gpu_rate_desc *descs, int max_views);
int lc3gpu_resampler_destroy(lc3gpu_resampler *rs);
int lc3gpu_resampler_reset(lc3gpu_resampler *rs); /* all channels */
int lc3gpu_resampler_reset_channels(lc3gpu_resampler *rs, const int32_t *channels, int n);
int lc3gpu_resample_mixed_views(lc3gpu_resampler *rs, const lc3gpu_view *in_views, const int16_t *d_pcm_in, size_t in_elems,
                                const lc3gpu_view *out_views, int16_t *d_pcm_out, size_t out_elems, int n_views, void *hip_stream);
/* PCM levels over a list of VIEWS: what decides WHAT a tick mixes -- who is speaking, whether a capture clips, whether a room's mix hits
 * the clamp of lc3gpu_mix_mixed_views -- measured on the tick's own view arrays, the PCM read where one array says it lies, with a smoothed
 * level and a hang-over carried from tick to tick so that a speaker is not dropped between words.  lc3gpu_analyze_mixed_views measures
 * coded frames before the decode; this call sees PCM that was never coded (capture buffers), PCM that is no longer what was coded (mixes,
 * resampled streams) and what carries over from one tick to the next.  The reference has no meter; the definition below is all-integer, so
 * the result does not depend on the order of summation.
 *   create    fs_hz is one of the six rates (8 kHz and 44.1 kHz included), frame_us is 7500 or 10000, attack_q15 and release_q15 lie in
 *             0..32768, threshold in 0..2^30, hang_frames in 0..65535 (LC3GPU_EINVAL otherwise).  n_channels >= 1.  max_views >= 1 bounds
 *             n_views of one call and sizes the pinned upload ring and its device twin once (LC3GPU_EINVAL below 1).  The descriptors are
 *             checked before a device is looked for.  The meter is bound to the device that is current at creation, is not thread-safe
 *             and is independent of every other object.  No device: LC3GPU_ENODEVICE
 *   views     views is a HOST array and may be reused as soon as the call returns.  Read: channel (index into the meter's descriptors),
 *             n_frames, pcm_off, pcm_stride, pcm_pitch, flag_off, flag_pitch and reserved (0).  NOT read: nbytes, byte_off, byte_pitch.
 *             So the array can be the very array the tick gave lc3gpu_decode_mixed_views, or the one it will give
 *             lc3gpu_encode_mixed_views, whose flag_off that call ignores and this one uses.  The meter carries state, so a channel may be
 *             named once per call: twice is LC3GPU_ECHANNEL
 *   placement sample n of frame t of a view is d_pcm[pcm_off + t * pitch + n * pcm_stride] with pitch = pcm_pitch ? pcm_pitch : nf *
 *             pcm_stride: exactly the views calls' rule, nf the frame length of (fs_hz, frame_us).  Frame t's outputs are d_active[flag_off
 *             + t * fp] and d_levels[flag_off + t * fp] with fp = flag_pitch ? flag_pitch : 1.  At least one output must be given.  Only a
 *             frame's own byte and record are written: everything between and around them is left as it was
 *   written   for frame t of a view, in order t = 0, 1, ...: x[0 .. nf) its samples, x[-1] the sample before it in the channel's stream (the
 *             last sample of frame t - 1 of the view, or for t = 0 the state's last), env0 and hang0 the state before the frame:
 *               sum_sq = sum of x[n]^2 (int64)      sum = sum of x[n]      min, max
 *               n_clipped = the number of n with x[n] == 32767 or x[n] == -32768
 *               n_cross   = the number of n in 0 .. nf - 1 with (x[n] < 0) != (x[n - 1] < 0)
 *               ms  = sum_sq / nf                                 (floor; <= 2^30)
 *               d   = ms - env0;  k = d > 0 ? attack_q15 : release_q15
 *               env = env0 + ((d * k + 16384) >> 15)              (int64, arithmetic shift)
 *               if env >= threshold:  hang = hang_frames, active = 1
 *               else if hang0 > 0:    hang = hang0 - 1,   active = 1
 *               else:                 hang = 0,           active = 0
 *               state after the frame: last = x[nf - 1], env, hang
 *             sum_sq <= 480 * 2^30 < 2^39, |sum| <= 15 728 640, |d * k| <= 2^45, and env always lies between env0 and ms inclusive, so it
 *             stays in 0..2^30 (checked with Python integers over two million random and corner triples).  A coefficient of 32768 reaches
 *             ms exactly, a coefficient of 0 never moves.  Because x[-1] and the recurrence run through the state, frames may be split
 *             over calls and over views' n_frames in any way without changing one record
 *   state     a fresh channel has last = 0, env = 0, hang = 0.  A listed channel advances; a channel not listed keeps its state.
 *             lc3gpu_meter_reset (all channels) and lc3gpu_meter_reset_channels (LC3GPU_ECHANNEL for an index out of range, and then none
 *             is reset) wait for nothing and launch nothing: the named channels read a fresh state inside their next launch.  A refused
 *             call has launched nothing, written nothing, advanced no channel and consumed no pending reset
 *   checks    on the host before anything is queued:
 *               channel outside [0, n_channels)                      LC3GPU_ECHANNEL
 *               a channel named twice in one call                    LC3GPU_ECHANNEL
 *               n_frames < 1                                         LC3GPU_ELENGTH
 *               more than 2^31 - 1 samples in one view               LC3GPU_ELENGTH
 *               any sample of any view outside [0, pcm_elems)        LC3GPU_ELENGTH
 *               any output index of any frame outside [0, n_active)
 *               / [0, n_levels) of a GIVEN output                    LC3GPU_ELENGTH
 *               n_views > max_views                                  LC3GPU_ELENGTH
 *               pcm_stride outside 1..8                              LC3GPU_EINVAL
 *               a negative pcm_off or flag_off                       LC3GPU_EINVAL
 *               a non-zero pitch below nf * pcm_stride               LC3GPU_EINVAL
 *               flag_pitch < 0                                       LC3GPU_EINVAL
 *               reserved != 0                                        LC3GPU_EINVAL
 *               pcm_stride == 1 with an odd pcm_off, an odd pitch
 *               or a base not 4-byte aligned                         LC3GPU_EINVAL
 *               pcm_stride >= 2 with a base not 2-byte aligned       LC3GPU_EINVAL
 *               both outputs NULL                                    LC3GPU_EINVAL
 *               d_levels not 16-byte aligned                         LC3GPU_EINVAL
 *               an output's address range overlapping d_pcm's or
 *               the other output's                                   LC3GPU_EINVAL
 *               a null mt; null views or d_pcm with n_views > 0;
 *               n_views < 0                                          LC3GPU_EINVAL
 *               n_views == 0                                         LC3GPU_OK (nothing launched)
 *             the extent check works in unsigned 64-bit arithmetic that cannot wrap.  HIP errors: LC3GPU_EHIP
 *   order     asynchronous on hip_stream.  Calls of one meter share its states: a call on another stream than the previous one's is
 *             ordered behind it by an event wait on the device, as the resampler orders its calls.  The host waits for the oldest of its
 *             own uploads only when more calls are in flight than the ring has slots
 *   launches  ONE launch and ONE upload of O(views) bytes per call, whatever mix of rates, durations, strides and frame counts.  One wave
 *             walks one view: a view of thousands of frames is one serial wave, which is correct, not tuned
 * NOT provided (out of scope): state blobs, a channel twice in a call, float or wider PCM, loudness weighting (K-weighting, LUFS),
 * per-sample envelopes, host-resident buffers, the pipeline object, uniform handles. */
typedef struct lc3gpu_meter_desc {
    int fs_hz;            /* one of the six rates */
    int frame_us;         /* 7500 or 10000 */
    int32_t attack_q15;   /* 0..32768: share of the way the envelope rises towards a louder frame */
    int32_t release_q15;  /* 0..32768: share of the way it falls towards a quieter one */
    uint32_t threshold;   /* 0..2^30, in the envelope's unit (mean square of int16 samples) */
    int32_t hang_frames;  /* 0..65535: frames the gate stays open after the envelope fell below threshold */
} lc3gpu_meter_desc; /* 24 bytes */
typedef struct lc3gpu_level {
    int64_t sum_sq;       /* sum of x*x over the frame */
    uint32_t env;         /* the envelope after this frame */
    int32_t sum;          /* sum of x (DC) */
    int16_t min, max;
    uint16_t n_clipped;   /* samples equal to 32767 or -32768 */
    uint16_t n_cross;     /* sign changes, the one into the frame's first sample included */
    uint16_t hang;        /* the hang-over counter after this frame */
    uint8_t active;       /* 1 or 0 */
    uint8_t reserved0;    /* 0 */
    uint32_t reserved1;   /* 0 */
} lc3gpu_level; /* 32 bytes, one per frame */
#ifdef __cplusplus
static_assert(sizeof(lc3gpu_meter_desc) == 24, "lc3gpu_meter_desc is 24 bytes");
static_assert(sizeof(lc3gpu_level) == 32, "lc3gpu_level is 32 bytes");
#else
_Static_assert(sizeof(lc3gpu_meter_desc) == 24, "lc3gpu_meter_desc is 24 bytes");
_Static_assert(sizeof(lc3gpu_level) == 32, "lc3gpu_level is 32 bytes");
#endif
typedef struct lc3gpu_meter lc3gpu_meter;
int lc3gpu_meter_create(lc3gpu_meter **out, int n_channels, const lc3gpu_meter_desc *descs, int max_views);
int lc3gpu_meter_destroy(lc3gpu_meter *mt);
int lc3gpu_meter_reset(lc3gpu_meter *mt); /* all channels */
int lc3gpu_meter_reset_channels(lc3gpu_meter *mt, const int32_t *channels, int n);
int lc3gpu_measure_mixed_views(lc3gpu_meter *mt, const lc3gpu_view *views, int n_views, const int16_t *d_pcm, size_t pcm_elems,
                               uint8_t *d_active, size_t n_active,      /* one byte per output index, or NULL */
                               lc3gpu_level *d_levels, size_t n_levels, /* one record per output index, or NULL */
                               void *hip_stream);

size_t lc3gpu_decoder_state_size(const lc3gpu_decoder *dec);
int lc3gpu_decoder_state_save(lc3gpu_decoder *dec, void *host_dst, size_t nbytes);
int lc3gpu_decoder_state_load(lc3gpu_decoder *dec, const void *host_src, size_t nbytes);
int lc3gpu_decoder_state_save_channels(lc3gpu_decoder *dec, const int32_t *channels, int n, void *host_dst, size_t nbytes);
int lc3gpu_decoder_state_load_channels(lc3gpu_decoder *dec, const int32_t *channels, int n, const void *host_src, size_t nbytes);
/* total number of frames concealed so far over all channels (synchronises the device) */
int lc3gpu_decoder_plc_events(lc3gpu_decoder *dec, uint64_t *out);
/* Full batches run the bit packer and the bitstream parser as producer / consumer pairs of wavefronts.  A half that waits 2^24 polls for
 * its partner gives up (a partner that died: never seen): a parser pair then conceals its frames as the reference conceals a frame whose
 * read_frame failed (decoder/lc3_decoder.rs:138-141; they count as PLC events too), a packer pair leaves its frames ZERO-FILLED -- the
 * reference has no such case (`Lc3EncoderError` is empty, encoder/lc3_encoder.rs:29-30), so it is made visible here: *out = the number of
 * pair halves that ever gave up on this handle (sticky; 0 in every run so far).  Waits for the handle's work in flight.
 * A caller need not poll: the handle's next batch call returns LC3GPU_EPAIR (once) when a pair half of an earlier call gave up. */
int lc3gpu_encoder_pair_timeouts(lc3gpu_encoder *enc, uint64_t *out);
int lc3gpu_decoder_pair_timeouts(lc3gpu_decoder *dec, uint64_t *out);
/* A look at the flag behind LC3GPU_EPAIR that changes nothing: 1 if the handle's next batch call would return LC3GPU_EPAIR, else 0
 * (read from pinned host memory: no synchronisation, no wait).  For a caller that drives several handles as one unit and must know
 * that all of them can take a call before the first one launches (the pipeline object does). */
int lc3gpu_encoder_pair_pending(const lc3gpu_encoder *enc);
int lc3gpu_decoder_pair_pending(const lc3gpu_decoder *dec);
/* tests only: make the device do what a pair half that gives up does (count + host flag), so that the LC3GPU_EPAIR path can be exercised */
int lc3gpu_encoder_debug_pair_giveup(lc3gpu_encoder *enc);
int lc3gpu_decoder_debug_pair_giveup(lc3gpu_decoder *dec);

/* A caller that runs a handle on ONE HIP stream for the handle's whole life (the pipeline object does) can say so: bind = 1 binds the
 * handle to `hip_stream` -- which must outlive the handle or the binding --, bind = 0 releases it.  A bound handle takes batch calls on
 * that stream only (LC3GPU_EINVAL otherwise; the *_frame, *_host and diagnostic calls are not for bound handles) and records no event of
 * its own per call: "the handle's work in flight" is the stream.  Both calls wait for the handle's work in flight. */
int lc3gpu_encoder_bind_stream(lc3gpu_encoder *enc, void *hip_stream, int bind);
int lc3gpu_decoder_bind_stream(lc3gpu_decoder *dec, void *hip_stream, int bind);

/* ---- host-resident batches ----------------------------------------------------------------------- */
/* The reference's callers keep PCM and frame bytes in HOST memory and walk them frame by frame, channel by channel
 * (examples/encode.rs:73-116: read samples, de-interleave, encode_frame per channel, write; examples/decode.rs:60-112 the mirror).
 * These two calls take such buffers whole -- planar, as the batch calls: pcm int16[num_channels][n_frames][nf], bytes
 * uint8[num_channels][n_frames][nbytes], bad_frame (optional) uint8[num_channels][n_frames] -- and return when the results are in host
 * memory: the handle's channels go through the device in ranges of >= 32 768 frames, the copy-in of one range, the kernels of another and
 * the copy-out of a third at the same time (three internal HIP streams).  State is carried as by the batch calls.  The PCIe link bounds them (960 + 150 bytes per 48 kHz / 10 ms frame each way);
 * buffers from lc3gpu_host_alloc (pinned) copy at the link's rate, any other host memory through the runtime's staging copies. */
int lc3gpu_encode_host(lc3gpu_encoder *enc, const int16_t *pcm, uint8_t *out, int nbytes, int n_frames);
int lc3gpu_decode_host(lc3gpu_decoder *dec, const uint8_t *in, const uint8_t *bad_frame, int16_t *pcm, int nbytes, int n_frames);
int lc3gpu_host_alloc(void **out, size_t nbytes);
int lc3gpu_host_free(void *p);

/* ---- pipeline: the caller loop as an object -------------------------------------------------------- */
/* The reference's caller owns the loop "for every frame, for every channel: encode_frame" (examples/encode.rs:97-115) and its mirror
 * (examples/decode.rs:93-112).  On the GPU the arrangement of that loop decides a fifth of the throughput (kernels of different calls share
 * the chip): a pipeline owns the arrangement that measured best -- the channels in `n_groups` groups (0 = the default,
 * two), every group with an encoder handle on a HIP stream of the higher priority and a decoder handle on a stream of the default
 * priority, two submissions in flight per group, the groups never joining -- so that a C / Rust caller gets it from three calls.
 * Buffers: DEVICE pointers, planar like lc3gpu_encode / lc3gpu_decode (int16[num_channels][n_frames][nf], uint8[num_channels][n_frames][nbytes]).
 * Every call is asynchronous on the pipeline's own streams:
 *   lc3gpu_pipeline_submit   one round trip: encode d_pcm -> d_bytes, decode d_bytes -> d_pcm_out (the decoder of a group starts when its
 *                            encoder has finished, and the encoder of the NEXT submission runs beside it).  A submission's encoder waits
 *                            for the decoders of the two submissions before it only where it would overwrite bytes they still read:
 *                            alternate two byte buffers and nothing waits.
 *   lc3gpu_pipeline_encode / lc3gpu_pipeline_decode   the halves alone (d_bad_frame as for lc3gpu_decode, may be NULL)
 *   lc3gpu_pipeline_wait     the host waits for everything submitted
 *   lc3gpu_pipeline_join     `hip_stream` (the caller's) waits for everything submitted -- results may be consumed on that stream
 *   lc3gpu_pipeline_follow   the NEXT submission waits for what `hip_stream` holds now (e.g. the kernel that produces d_pcm)
 *   lc3gpu_pipeline_mark     records `hip_event` (a hipEvent_t of the caller's) on the LAST group's stream behind its latest work: a
 *                            progress mark / timing point that costs the pipeline nothing -- `join` puts event waits on a further stream, and
 *                            a waiting stream can hold up a pipeline stream that shares its hardware queue (measured: -10 % with a join
 *                            after every submission).  The groups are not tied to each other: the mark says nothing about the other groups.
 *                            "Latest work" is the encoder's and the decoder's: after a round trip the decoder stream is behind both and
 *                            the mark is a bare event record; where the group's decoder stream is not behind its encoder's latest work
 *                            (an lc3gpu_pipeline_encode after a decode, halves on unrelated buffers) the decoder stream first waits for
 *                            it, unless it has completed -- the one case in which a mark queues a wait on a pipeline stream
 *   lc3gpu_pipeline_group    the channel range and the handles of a group (borrowed: state blobs, PLC / health counters, timing,
 *                            stage events; never destroy them, never call their batch functions while the pipeline has work in flight)
 *   lc3gpu_pipeline_reset    every channel back to the freshly constructed state from the next submission on (no wait; the decoders of a
 *                            MIXED pipeline carry the reset out at their next decode, which synchronises the device once per group)
 * What the pipeline orders: the BYTE buffers.  An encoder never overwrites bytes that a decoder of an earlier submission still reads or
 * that another encoder still writes, a decoder never reads bytes before the encoder that writes them has finished -- whichever group
 * queued the earlier work, also when the base pointer, n_frames or nbytes change between submissions into the same memory (a group's
 * slice of a buffer depends on all three; a submission whose geometry does not fit the ones before it puts every stream's next work
 * behind the other groups' latest work once, on the device).  Up to four byte buffers of one n_frames and nbytes in rotation cost nothing.
 * What the caller orders: the PCM buffers, d_bad_frame, and whatever its own streams do.  d_pcm must be complete when the submission
 * that reads it is queued, or be produced on a stream that lc3gpu_pipeline_follow names right before that submission; d_pcm_out may be
 * consumed after lc3gpu_pipeline_wait or on a stream behind lc3gpu_pipeline_join, and the submission that overwrites it while such a
 * consumer may still read goes behind a follow of that stream.  A transcoding chain (d_pcm_out of one submission as d_pcm of a later
 * one) needs join + follow through a stream of the caller's, or a wait, between the two; so does an output buffer that an encoder in
 * flight reads.  An output buffer written again with another n_frames (the groups' slices move) needs a wait first.
 * Errors as the batch calls (nbytes 20..400 where the call encodes, 1..400 for a decode alone; d_pcm and d_pcm_out 4-byte aligned), and
 * all or nothing: the arguments and every group's pair flag are looked at before the first group launches, so a call that refuses its
 * arguments, or returns LC3GPU_EPAIR for a flag that was up when the call began, has queued nothing on any group and may be repeated;
 * with flags up on several handles there is one refusal each.  The device raises a flag from work in flight: one that rises DURING a
 * call is reported by the call after it, or -- if it rises after the look and before that group's own turn -- by this one with
 * earlier groups already launched (no such window when nothing is in flight, i.e. after lc3gpu_pipeline_wait).  After LC3GPU_EHIP
 * some groups may have launched and others not: the pipeline must be reset (lc3gpu_pipeline_reset) before further use.
 * Mixed configurations (lc3gpu_pipeline_create_mixed, BASELINE config 4 through the pipeline): streams of different rates, durations and frame
 * sizes, descriptors and ragged buffers as for lc3gpu_*_create_mixed / lc3gpu_encode_mixed (8 kHz streams are refused: a pipeline encodes and
 * decodes); group g takes the descriptors [group_first[g], group_first[g + 1]) (group_first[0] = 0, ascending, n_groups entries; NULL: equal
 * shares of the list; with boundaries given, n_groups is theirs: 0 or more than n_streams is LC3GPU_EINVAL) -- order the list so that every
 * group holds a share of every configuration.  The *_mixed calls take the place of submit / encode / decode (LC3GPU_EINVAL for the
 * other kind); everything else is common. */
typedef struct lc3gpu_pipeline lc3gpu_pipeline;
int lc3gpu_pipeline_create(lc3gpu_pipeline **out, int num_channels, int frame_us, int fs_hz, int n_groups);
int lc3gpu_pipeline_create_mixed(lc3gpu_pipeline **out, int n_streams, const lc3gpu_stream_desc *descs, int n_groups, const int *group_first);
int lc3gpu_pipeline_submit_mixed(lc3gpu_pipeline *p, const int16_t *d_pcm, uint8_t *d_bytes, int16_t *d_pcm_out, int n_frames);
int lc3gpu_pipeline_encode_mixed(lc3gpu_pipeline *p, const int16_t *d_pcm, uint8_t *d_bytes, int n_frames);
int lc3gpu_pipeline_decode_mixed(lc3gpu_pipeline *p, const uint8_t *d_bytes, const uint8_t *d_bad_frame, int16_t *d_pcm_out, int n_frames);
int lc3gpu_pipeline_destroy(lc3gpu_pipeline *p);
int lc3gpu_pipeline_reset(lc3gpu_pipeline *p);
int lc3gpu_pipeline_submit(lc3gpu_pipeline *p, const int16_t *d_pcm, uint8_t *d_bytes, int16_t *d_pcm_out, int nbytes, int n_frames);
int lc3gpu_pipeline_encode(lc3gpu_pipeline *p, const int16_t *d_pcm, uint8_t *d_bytes, int nbytes, int n_frames);
int lc3gpu_pipeline_decode(lc3gpu_pipeline *p, const uint8_t *d_bytes, const uint8_t *d_bad_frame, int16_t *d_pcm_out, int nbytes, int n_frames);
int lc3gpu_pipeline_wait(lc3gpu_pipeline *p);
int lc3gpu_pipeline_join(lc3gpu_pipeline *p, void *hip_stream);
int lc3gpu_pipeline_follow(lc3gpu_pipeline *p, void *hip_stream);
int lc3gpu_pipeline_mark(lc3gpu_pipeline *p, void *hip_event);
int lc3gpu_pipeline_groups(const lc3gpu_pipeline *p);
int lc3gpu_pipeline_group(lc3gpu_pipeline *p, int group, int *first_channel, int *n_channels, lc3gpu_encoder **enc, lc3gpu_decoder **dec);
int lc3gpu_pipeline_last_hip_error(const lc3gpu_pipeline *p);

/* ---- diagnostics -------------------------------------------------------------------------------- */
/* encode one frame of channel 0 from host PCM (the frame IS a frame of that channel: its state advances) and also return stage dumps,
 * so that an encoder stage can be checked against the reference's own stage vectors (encoder/modified_dct.rs:191-337,
 * attack_detector.rs:138-180, spectral_noise_shaping.rs:658-801, temporal_noise_shaping.rs:359-471, long_term_post_filter.rs:479-843,
 * spectral_quantization.rs:404-480, noise_level_estimation.rs:65-137):
 * dbg float[LC3GPU_ENC_DBG_FLOATS] = spectrum after MDCT [0,480), after SNS [480,960), after TNS [960,1440); scalars from
 * LC3GPU_ENC_DBG_SCALARS: +0 bandwidth index, +1 attack flag, +2 ind_lf, +3 ind_hf, +4 shape_j, +5 gind, +6 / +7 TNS orders, +8 nbits_tns,
 * +9 pitch_index, +10 pitch_present, +11 ltpf_active, +12 gg_ind, +13 lastnz_trunc, +14 nbits_lsb, +15 lsb_mode, +16 residual bits,
 * +17 noise factor, +18 global gain, +19 nbits_spec, +20 nbits_trunc, +21 near-Nyquist flag, +22 ls_inda, +23 / +24 index_joint_j low /
 * high 16 bits; the 64 band energies from LC3GPU_ENC_DBG_EB; the attack detector's state after the frame from LC3GPU_ENC_DBG_ATTACK
 * (energy_last, max_energy_last, attack_pos_last, downsampled sample t-1, t-2) */
#define LC3GPU_ENC_DBG_SCALARS 1440
#define LC3GPU_ENC_DBG_EB 1472
#define LC3GPU_ENC_DBG_ATTACK 1536
#define LC3GPU_ENC_DBG_FLOATS 1600
int lc3gpu_encode_frame_debug(lc3gpu_encoder *enc, const int16_t *samples_in, int n_samples, uint8_t *buf_out,
                              int nbytes, float *dbg);
/* decode one frame of channel 0 (uniform handles) from host bytes like lc3gpu_decode_frame and also return stage dumps, so that a
 * decoder stage can be checked on its own (the reference tests every one: decoder/arithmetic_codec.rs:415-474,
 * residual_spectrum.rs:47-107, noise_filling.rs:65-146, temporal_noise_shaping.rs:147-238, spectral_noise_shaping.rs:244-350,
 * modified_dct.rs:174-329, long_term_post_filter.rs:504-1199).  dbg float[LC3GPU_DBG_FLOATS], NaN where a form has no such value:
 *   [LC3GPU_DBG_INT, +ne)    integers after the range decoder            [LC3GPU_DBG_GAIN, +ne)  after residual bits, noise filling, global gain
 *   [LC3GPU_DBG_TNS, +ne)    after the TNS filter                        [LC3GPU_DBG_SPEC, +ne)  after the SNS band gains (input of the IMDCT)
 *   [LC3GPU_DBG_IMDCT, +nf)  after IMDCT, window, overlap-add            [LC3GPU_DBG_LTPF, +nf)  after the long-term post-filter
 * recon_form selects which of the library's three forms of the spectrum reconstruction runs: LC3GPU_RECON_LANE (in the parse
 * kernel, what full batches use), LC3GPU_RECON_LATE (in the synthesis kernel, what lc3gpu_decode_frame and small launches use),
 * LC3GPU_RECON_WAVE (the wave-per-frame kernels; no GAIN / TNS dumps). */
#define LC3GPU_DBG_INT 0
#define LC3GPU_DBG_SPEC 400
#define LC3GPU_DBG_IMDCT 800
#define LC3GPU_DBG_LTPF 1280
#define LC3GPU_DBG_GAIN 1760
#define LC3GPU_DBG_TNS 2160
#define LC3GPU_DBG_FLOATS 2560
#define LC3GPU_RECON_LANE 0
#define LC3GPU_RECON_LATE 1
#define LC3GPU_RECON_WAVE 2
int lc3gpu_decode_frame_debug(lc3gpu_decoder *dec, int recon_form, const uint8_t *buf_in, int nbytes, int16_t *samples_out, int n_samples,
                              float *dbg);
/* the synthesis half alone on channel 0: `in` is a reconstructed spectrum (time_in = 0, n_in = ne: IMDCT -> LTPF -> PCM) or the
 * time samples that enter the long-term post-filter (time_in = 1, n_in = nf: LTPF -> PCM), with the frame's post-filter side
 * information and its size (nbits = 8 * nbytes selects the filter gain; pitch_index 0 .. 511 as in the bitstream, LC3GPU_EINVAL otherwise).
 * dbg as above (IMDCT and LTPF dumps).  Like lc3gpu_decode_frame_debug this ADVANCES channel 0's state (overlap memory, post-filter
 * memories): a diagnostic call is a frame of that channel. */
int lc3gpu_decoder_synth_debug(lc3gpu_decoder *dec, int time_in, const float *in, int n_in, int ltpf_active, int pitch_index, int nbytes,
                               int16_t *samples_out, int n_samples, float *dbg);
/* tests only: the float routines the codec's bit-exactness rests on, evaluated on the device as the kernels compile them.
 * which: 0 x / d by the quantiser's reciprocal sequence, 1 x / d by the compiler's IEEE division, 2 log2f, 3 log10f, 4 exp2f, 5 asinf,
 * 6 fast-math exp2_raw, 7 10^x, 8 sinf (|x| small), 9 the device-filled tables (n = 866: 512 gains 10^(k/28), k = -256..255, 320 tilt
 * factors, 17 + 17 TNS sines).  x, d, out: HOST arrays of n floats (d only for 0 and 1, neither for 9). */
int lc3gpu_selftest_math(int which, const float *x, const float *d, int n, float *out);
/* per-kernel timing of the batch calls with HIP events recorded on the launch stream.  An encoder batch call runs four
 * kernels: analysis front half (wave per stream), SNS vector quantiser (lane per frame), analysis back half (wave per
 * stream), bitstream packing (lane per frame); a decoder batch call two: frame parsing with the spectrum reconstruction on the
 * lane that parsed the frame (full batches; launches of a few frames reconstruct inside the synthesis kernel instead), synthesis
 * (wave per stream) -- or four when LC3GPU_RECON=wave selects the measured-but-not-default form with two reconstruction kernels of
 * their own (wave per frame and, for the TNS lattice, lane per frame).  With LC3GPU_SPLIT=1 (opt-in; measured slower) a call runs as
 * two halves of its streams on two internal HIP streams: a kernel's figure is then the sum over both launches.  `enable` = 0 switches recording off, 1 on for every batch call,
 * n > 1 on for every n-th batch call from now on (an event after every kernel costs the stream a few microseconds: sampling keeps a
 * long timed run undisturbed); the call synchronises and returns the per-kernel milliseconds accumulated since the previous call
 * followed by the number of batch calls that were timed:
 * encoder out[5] = {front, vq, back, pack, calls}, decoder out[3] = {parse + reconstruction, synthesis, calls},
 * lc3gpu_decoder_timing_kernels out[5] = {parse, reconstruction kernel, TNS kernel (both 0 where the launch has none), synthesis, calls}. */
int lc3gpu_encoder_timing(lc3gpu_encoder *enc, int enable, double out[5]);
int lc3gpu_decoder_timing(lc3gpu_decoder *dec, int enable, double out[3]);
int lc3gpu_decoder_timing_kernels(lc3gpu_decoder *dec, int enable, double out[5]);
/* Stage events (an extension without a counterpart in the reference: its caller loop, examples/encode.rs:97-115 / examples/decode.rs:93-112,
 * has no stages to observe).  `hip_event` is a hipEvent_t of the CALLER (NULL clears the slot); from then on every batch call of the handle
 * records it on the call's stream right behind the kernel(s) of the stage, so that a caller who runs several handles on several HIP streams
 * can make another stream wait (hipStreamWaitEvent) for a chosen point INSIDE this handle's call -- e.g. start a decoder's parser when the
 * encoder's back half has ended, beside the encoder's packer (both leave most of the chip's workgroup slots free) instead of beside its
 * front half (which fills them): bench.py's `staggered` arrangement, INTEGRATION.md section 4.  The event completes no earlier than the
 * stage; a call that runs as two halves (LC3GPU_SPLIT=1) records every stage event at its end.  The event must stay valid while it is
 * set.  LC3GPU_EINVAL for an unknown stage. */
#define LC3GPU_MAX_STAGES 4
#define LC3GPU_ENC_STAGE_FRONT 0 /* analysis front half done */
#define LC3GPU_ENC_STAGE_VQ 1    /* ... and the SNS vector quantiser */
#define LC3GPU_ENC_STAGE_BACK 2  /* ... and the back half: only the packer is left */
#define LC3GPU_DEC_STAGE_PARSE 0 /* frames parsed and spectra rebuilt: only the synthesis kernel is left */
int lc3gpu_encoder_stage_event(lc3gpu_encoder *enc, int stage, void *hip_event);
int lc3gpu_decoder_stage_event(lc3gpu_decoder *dec, int stage, void *hip_event);
/* diagnostic build (liblc3gpu_prof.so, -DLC3_PROFILE) only: per-stage shader-clock cycle sums since the last call.
 * slots 1..9 = encoder stages (mdct, bw+attack, sns, tns, ltpf, quant, residual+noise, bitstream, store),
 * slots 17..25 = decoder stages (names in tools/stage_profile.py); 32/33/34 = encoder whole-wave time sum / max / waves,
 * 35/36/37 the same for the decoder, 40..46 = sections of the parse kernel (side info, TNS data, spectral data,
 * zero fill + residual bits, reconstruction set-up, reconstruction pass, rest), 48..54 = sections of the pack kernel
 * (staging, side info, TNS data, spectral data, residual bits, finish, barrier wait + copy-out), 55 = its waves.
 * LC3GPU_EUNSUPPORTED in the normal build. */
int lc3gpu_prof_read(unsigned long long out[64]);
/* measurement aid (bench.py's sustained leg): one wave on `stream` stamps the shader-cycle counter and the constant 100 MHz counter around
 * `spin` dependent vector additions; asynchronous, d_out (DEVICE memory, 3 x uint64) <- {shader cycles, 100 MHz ticks, unused}.  The clock the
 * chip runs at while the probe is in flight = 100 MHz x cycles / ticks (launch it on a stream beside the codec's). */
int lc3gpu_clock_probe(void *stream, unsigned long long *d_out, int spin);
/* kernel resource report as the loaded code object has it: out = {static lds_bytes, vgprs, 0, scratch_bytes, max_threads} for the six kernels
 * a full batch of the headline configuration launches: which = 0 analysis back half, 1 synthesis (the numbers these two had when they
 * were the only ones), 2 analysis front half, 3 SNS vector quantiser, 4 packer (pair form), 5 parser (pair form); LC3GPU_EINVAL beyond.
 * (tests/test_kernel_resources.py reads the same, and the spill counts, from the built library's metadata without a GPU and holds them
 * to the register budgets the kernels are tuned for.) */
int lc3gpu_kernel_info(int which, int out[5]);

#ifdef __cplusplus
}
#endif
#endif /* LC3GPU_H_ */
