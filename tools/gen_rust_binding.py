#!/usr/bin/env python3
"""Writes bindings/lc3gpu.rs: the Rust side of the drop-in boundary.

The reference is a Rust crate (ninjasource/lc3-codec v0.2.0); BASELINE.json's north star asks for "Rust host code calling a thin C-ABI
HIP layer".  There is no Rust toolchain in this image, so the file is shipped UNCOMPILED -- but it is not hand-copied either: the
`extern "C"` block is generated from include/lc3gpu.h declaration by declaration (tests/test_abi.py regenerates it and compares, and
checks that every symbol the header declares is bound), and the safe wrappers below it are the reference's own surface
(`Lc3Encoder::new / encode_frame`, src/encoder/lc3_encoder.rs:117-191; `Lc3Decoder::new / decode_frame`, src/decoder/lc3_decoder.rs:181-234)
plus the batch, host-batch and pipeline calls.

usage: gen_rust_binding.py [out.rs]"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lc3gpu.h")

OPAQUE = {"lc3gpu_encoder": "Lc3GpuEncoder", "lc3gpu_decoder": "Lc3GpuDecoder", "lc3gpu_pipeline": "Lc3GpuPipeline",
          "lc3gpu_stream_desc": "Lc3GpuStreamDesc", "lc3gpu_frame_info": "Lc3GpuFrameInfo", "lc3gpu_item": "Lc3GpuItem", "lc3gpu_mc_item": "Lc3GpuMcItem",
          "lc3gpu_view": "Lc3GpuView", "lc3gpu_inspector": "Lc3GpuInspector", "lc3gpu_analyzer": "Lc3GpuAnalyzer",
          "lc3gpu_mixer": "Lc3GpuMixer", "lc3gpu_mix_in": "Lc3GpuMixIn", "lc3gpu_mix_out": "Lc3GpuMixOut",
          "lc3gpu_resampler": "Lc3GpuResampler", "lc3gpu_rate_desc": "Lc3GpuRateDesc",
          "lc3gpu_meter": "Lc3GpuMeter", "lc3gpu_meter_desc": "Lc3GpuMeterDesc", "lc3gpu_level": "Lc3GpuLevel"}
SCALAR = {"int": "i32", "unsigned": "u32", "unsigned int": "u32", "float": "f32", "double": "f64", "size_t": "usize",
          "int16_t": "i16", "uint16_t": "u16", "uint8_t": "u8", "int32_t": "i32", "uint32_t": "u32", "int64_t": "i64", "uint64_t": "u64",
          "unsigned long long": "u64", "char": "c_char", "void": "c_void"}


def strip_comments(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def rust_type(ctype):
    """'const int16_t *' -> '*const i16', 'lc3gpu_encoder **' -> '*mut *mut Lc3GpuEncoder', 'int' -> 'i32'"""
    t = ctype.strip()
    stars = t.count("*")
    t = t.replace("*", " ").strip()
    const = False
    words = [w for w in t.split() if w]
    if words and words[0] == "const":
        const, words = True, words[1:]
    if words and words[0] == "struct":
        words = words[1:]
    base = " ".join(words)
    r = OPAQUE.get(base) or SCALAR.get(base)
    if r is None:
        raise ValueError("unmapped C type: %r" % ctype)
    for i in range(stars):
        r = ("*const " if (const and i == 0) else "*mut ") + r  # (the innermost pointer carries the const of `const T *`)
    if stars == 0 and base == "void":
        return None
    return r


def parse_param(p):
    p = p.strip()
    if p == "void" or not p:
        return None
    m = re.match(r"^(.*?)(\w+)\s*(\[\s*\d*\s*\])?$", p)
    ctype, name, arr = m.group(1), m.group(2), m.group(3)
    if arr:
        ctype += "*"
    if name in ("in", "out", "type", "fn", "ref", "box", "move", "match", "loop", "where", "dyn"):
        name += "_"
    return name, rust_type(ctype)


def declarations():
    text = strip_comments(open(HEADER).read())
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    out = []
    for m in re.finditer(r"([\w\s\*]+?)\b(lc3gpu_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S):
        ret, name, params = m.group(1).strip(), m.group(2), m.group(3)
        if "typedef" in ret:
            continue
        ps = [parse_param(p) for p in " ".join(params.split()).split(",")]
        ps = [p for p in ps if p]
        out.append((name, ps, rust_type(ret)))
    return out


def constants():
    text = strip_comments(open(HEADER).read())
    out = []
    for m in re.finditer(r"^#define\s+(LC3GPU_\w+)\s+(-?\d+)\s*$", text, flags=re.M):
        if m.group(1) != "LC3GPU_H_":
            out.append((m.group(1), int(m.group(2))))
    return out


def frame_info_fields():
    """(name, rust type) of every field of lc3gpu_frame_info, in the header's order"""
    text = strip_comments(open(HEADER).read())
    body = re.search(r"typedef struct lc3gpu_frame_info \{(.*?)\} lc3gpu_frame_info;", text, flags=re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        ctype, names = decl.split(" ", 1)
        for name in names.split(","):
            m = re.match(r"^\s*(\w+)\s*(?:\[(\d+)\])?\s*$", name)
            t = SCALAR[ctype]
            out.append((m.group(1), "[%s; %s]" % (t, m.group(2)) if m.group(2) else t))
    return out


WRAPPERS = r'''
// ------------------------------------------------------------------------------------------------------------------
// Safe surface: what a maintainer adds beside src/encoder/lc3_encoder.rs:175-180 / src/decoder/lc3_decoder.rs:217-223 under
// `#[cfg(feature = "mi355x")]`.  Same names and argument meaning as the CPU types; the working buffers the CPU objects borrow
// (lc3_encoder.rs:117-173) are not needed -- device memory belongs to the handle.
// ------------------------------------------------------------------------------------------------------------------
use crate::common::config::{FrameDuration, SamplingFrequency};
use crate::decoder::lc3_decoder::Lc3DecoderError;
use crate::encoder::lc3_encoder::Lc3EncoderError;

fn frame_us(d: FrameDuration) -> i32 {
    match d {
        FrameDuration::SevenPointFiveMs => 7500,
        FrameDuration::TenMs => 10000,
    }
}
fn fs_hz(f: SamplingFrequency) -> i32 {
    match f {
        SamplingFrequency::Hz8000 => 8000,
        SamplingFrequency::Hz16000 => 16000,
        SamplingFrequency::Hz24000 => 24000,
        SamplingFrequency::Hz32000 => 32000,
        SamplingFrequency::Hz44100 => 44100,
        SamplingFrequency::Hz48000 => 48000,
    }
}

/// `Lc3Encoder` (encoder/lc3_encoder.rs:33-40,117-191) on the GPU: `num_channels` independent channels resident on the current HIP device.
pub struct Lc3EncoderGpu {
    h: *mut Lc3GpuEncoder,
    num_channels: usize,
}
impl Lc3EncoderGpu {
    /// lc3_encoder.rs:194-209 (kept for API parity: the numbers are the reference's, the buffers are not used)
    pub fn calc_working_buffer_lengths(num_channels: usize, d: FrameDuration, f: SamplingFrequency) -> (usize, usize, usize) {
        let mut out = [0i64; 3];
        let rc = unsafe { lc3gpu_encoder_working_buffer_lengths(num_channels as i32, frame_us(d), fs_hz(f), out.as_mut_ptr()) };
        assert_eq!(rc, LC3GPU_OK);
        (out[0] as usize, out[1] as usize, out[2] as usize)
    }
    /// lc3_encoder.rs:117-173.  Panics where the reference's constructor panics (8 kHz: encoder/bandwidth_detector.rs:36-37).
    pub fn new(num_channels: usize, d: FrameDuration, f: SamplingFrequency) -> Self {
        let mut h = core::ptr::null_mut();
        let rc = unsafe { lc3gpu_encoder_create(&mut h, num_channels as i32, frame_us(d), fs_hz(f)) };
        assert_eq!(rc, LC3GPU_OK, "lc3gpu_encoder_create: {}", rc);
        Self { h, num_channels }
    }
    /// lc3_encoder.rs:175-191: `buf_out.len()` selects the bit rate; cannot fail (`Lc3EncoderError` is empty), panics where the
    /// reference panics (channel index, slice length).
    pub fn encode_frame(&mut self, channel_index: usize, samples_in: &[i16], buf_out: &mut [u8]) -> Result<(), Lc3EncoderError> {
        let rc = unsafe {
            lc3gpu_encode_frame(self.h, channel_index as i32, samples_in.as_ptr(), samples_in.len() as i32, buf_out.as_mut_ptr(), buf_out.len() as i32)
        };
        if rc != LC3GPU_OK {
            panic!("encode_frame: lc3gpu error {}", rc)
        }
        Ok(())
    }
    /// The caller loop of examples/encode.rs:97-115 over host buffers in one call: `pcm` = [channel][frame][nf], `out` = [channel][frame][nbytes].
    pub fn encode_host(&mut self, pcm: &[i16], out: &mut [u8], nbytes: usize, n_frames: usize) -> i32 {
        assert_eq!(out.len(), self.num_channels * n_frames * nbytes);
        unsafe { lc3gpu_encode_host(self.h, pcm.as_ptr(), out.as_mut_ptr(), nbytes as i32, n_frames as i32) }
    }
    /// The same loop over DEVICE buffers, asynchronous on `hip_stream`.
    ///
    /// # Safety
    /// `d_pcm` / `d_out` must be device allocations of [channel][frame][nf] i16 / [channel][frame][nbytes] u8 that outlive the call's work.
    pub unsafe fn encode_device(&mut self, d_pcm: *const i16, d_out: *mut u8, nbytes: usize, n_frames: usize, hip_stream: *mut c_void) -> i32 {
        lc3gpu_encode(self.h, d_pcm, d_out, nbytes as i32, n_frames as i32, hip_stream)
    }
    /// a frame size per frame: d_nbytes[channel][frame] is that frame's buf_out.len(); frame (c, t) goes to the first d_nbytes[c][t]
    /// bytes of slot (c, t) of slot_bytes bytes (device pointers, include/lc3gpu.h)
    pub unsafe fn encode_vbr_device(&mut self, d_pcm: *const i16, d_out: *mut u8, d_nbytes: *const u16, slot_bytes: usize, n_frames: usize,
                                    hip_stream: *mut c_void) -> i32 {
        lc3gpu_encode_vbr(self.h, d_pcm, d_out, d_nbytes, slot_bytes as i32, n_frames as i32, hip_stream)
    }
    /// The caller's choice of channel per `encode_frame` call (examples/encode.rs:97-115) for many channels in one launch: item i of the
    /// compact buffers holds the frames of channel `channels[i]` (any order, none twice); the other channels are left as they were.
    ///
    /// # Safety
    /// `d_pcm` / `d_out` must be device allocations of [channels.len()][frame][nf] i16 / [channels.len()][frame][nbytes] u8 that outlive
    /// the call's work; `channels` is host memory and free again when the call returns.
    pub unsafe fn encode_list_device(&mut self, channels: &[i32], d_pcm: *const i16, d_out: *mut u8, nbytes: usize, n_frames: usize,
                                     hip_stream: *mut c_void) -> i32 {
        lc3gpu_encode_list(self.h, channels.as_ptr(), channels.len() as i32, d_pcm, d_out, nbytes as i32, n_frames as i32, hip_stream)
    }
    /// The same choice on a mixed-configuration handle (several `Lc3Encoder` objects of different configurations driven as one): item i of
    /// the ragged buffers, compact in list order, holds the frames of stream `channels[i]` at its descriptor's frame size.
    ///
    /// # Safety
    /// `d_pcm` / `d_out` must be device allocations laid out as include/lc3gpu.h states for lc3gpu_encode_mixed_list that outlive the
    /// call's work; `channels` is host memory and free again when the call returns.
    pub unsafe fn encode_mixed_list_device(&mut self, channels: &[i32], d_pcm: *const i16, d_out: *mut u8, n_frames: usize,
                                           hip_stream: *mut c_void) -> i32 {
        lc3gpu_encode_mixed_list(self.h, channels.as_ptr(), channels.len() as i32, d_pcm, d_out, n_frames as i32, hip_stream)
    }
    /// A frame count and a frame size per listed stream of a mixed-configuration handle: the reference's caller calls `encode_frame` once
    /// per (channel, frame) with a slice whose length selects the size (encoder/lc3_encoder.rs:175-191).
    ///
    /// # Safety
    /// `d_pcm` / `d_out` must be device allocations laid out as include/lc3gpu.h states for lc3gpu_encode_mixed_items that outlive the
    /// call's work; `items` is host memory and free again when the call returns.
    pub unsafe fn encode_mixed_items_device(&mut self, items: &[Lc3GpuItem], d_pcm: *const i16, d_out: *mut u8, hip_stream: *mut c_void) -> i32 {
        lc3gpu_encode_mixed_items(self.h, items.as_ptr(), items.len() as i32, d_pcm, d_out, hip_stream)
    }
    /// Multi-channel items of a mixed-configuration handle: WAV sample order in, the channels' frames back to back out, the order
    /// examples/encode.rs:96-115 reads and writes.
    ///
    /// # Safety
    /// `d_pcm` / `d_out` must be device allocations laid out as include/lc3gpu.h states for lc3gpu_encode_mixed_mc_items that outlive the
    /// call's work; `items` is host memory and free again when the call returns.
    pub unsafe fn encode_mixed_mc_items_device(&mut self, items: &[Lc3GpuMcItem], d_pcm: *const i16, d_out: *mut u8, hip_stream: *mut c_void) -> i32 {
        lc3gpu_encode_mixed_mc_items(self.h, items.as_ptr(), items.len() as i32, d_pcm, d_out, hip_stream)
    }
    /// Views of a mixed-configuration handle: every item with the placement of its PCM and its frames, read and written in place
    /// (jitter rings, a capture buffer wider than the stream).
    ///
    /// # Safety
    /// `d_pcm` / `d_out` must be device allocations of at least `pcm_elems` elements / `out_bytes` bytes that outlive the call's work;
    /// every view is checked against these extents on the host.  `views` is host memory and free again when the call returns.
    pub unsafe fn encode_mixed_views_device(&mut self, views: &[Lc3GpuView], d_pcm: *const i16, pcm_elems: usize, d_out: *mut u8, out_bytes: usize,
                                            hip_stream: *mut c_void) -> i32 {
        lc3gpu_encode_mixed_views(self.h, views.as_ptr(), views.len() as i32, d_pcm, pcm_elems, d_out, out_bytes, hip_stream)
    }
    /// a new `EncoderChannel` for each named channel (from its next call on; no wait); the others are untouched
    pub fn reset_channels(&mut self, channels: &[i32]) -> Result<(), i32> {
        let rc = unsafe { lc3gpu_encoder_reset_channels(self.h, channels.as_ptr(), channels.len() as i32) };
        if rc == 0 { Ok(()) } else { Err(rc) }
    }
    /// frame sizes encode_vbr_device has clamped into [20, slot_bytes] (sticky)
    pub fn size_clamps(&mut self) -> Result<u64, i32> {
        let mut v: u64 = 0;
        let rc = unsafe { lc3gpu_encoder_size_clamps(self.h, &mut v) };
        if rc == 0 { Ok(v) } else { Err(rc) }
    }
}
impl Drop for Lc3EncoderGpu {
    fn drop(&mut self) {
        unsafe {
            lc3gpu_encoder_destroy(self.h);
        }
    }
}

/// `Lc3Decoder` (decoder/lc3_decoder.rs:51-69,181-234) on the GPU.
pub struct Lc3DecoderGpu {
    h: *mut Lc3GpuDecoder,
    num_channels: usize,
}
impl Lc3DecoderGpu {
    /// lc3_decoder.rs:236-244
    pub fn calc_working_buffer_lengths(num_channels: usize, d: FrameDuration, f: SamplingFrequency) -> (usize, usize) {
        let mut out = [0i64; 2];
        let rc = unsafe { lc3gpu_decoder_working_buffer_lengths(num_channels as i32, frame_us(d), fs_hz(f), out.as_mut_ptr()) };
        assert_eq!(rc, LC3GPU_OK);
        (out[0] as usize, out[1] as usize)
    }
    /// lc3_decoder.rs:181-215
    pub fn new(num_channels: usize, d: FrameDuration, f: SamplingFrequency) -> Self {
        let mut h = core::ptr::null_mut();
        let rc = unsafe { lc3gpu_decoder_create(&mut h, num_channels as i32, frame_us(d), fs_hz(f)) };
        assert_eq!(rc, LC3GPU_OK, "lc3gpu_decoder_create: {}", rc);
        Self { h, num_channels }
    }
    /// lc3_decoder.rs:217-234: corrupt frames are concealed and `Ok(())` comes back (:138-141); the only error is the sample width.
    pub fn decode_frame(&mut self, num_bits_per_audio_sample: usize, channel_index: usize, buf_in: &[u8], samples_out: &mut [i16]) -> Result<(), Lc3DecoderError> {
        let rc = unsafe {
            lc3gpu_decode_frame(self.h, num_bits_per_audio_sample as i32, channel_index as i32, buf_in.as_ptr(), buf_in.len() as i32,
                                samples_out.as_mut_ptr(), samples_out.len() as i32)
        };
        match rc {
            LC3GPU_OK => Ok(()),
            LC3GPU_EBITS => Err(Lc3DecoderError::Only16BitsPerAudioSampleSupported),
            e => panic!("decode_frame: lc3gpu error {}", e),
        }
    }
    /// The caller loop of examples/decode.rs:93-112 over host buffers; `bad_frame` = one flag per (channel, frame), non-zero = lost.
    pub fn decode_host(&mut self, data: &[u8], bad_frame: Option<&[u8]>, pcm: &mut [i16], nbytes: usize, n_frames: usize) -> i32 {
        assert_eq!(data.len(), self.num_channels * n_frames * nbytes);
        let bad = bad_frame.map_or(core::ptr::null(), |b| b.as_ptr());
        unsafe { lc3gpu_decode_host(self.h, data.as_ptr(), bad, pcm.as_mut_ptr(), nbytes as i32, n_frames as i32) }
    }
    /// a frame size per frame: frame (c, t) is the first d_nbytes[c][t] bytes of slot (c, t) of slot_bytes bytes (its buf_in.len(); 0 or
    /// above slot_bytes: concealed); device pointers, include/lc3gpu.h
    pub unsafe fn decode_vbr_device(&mut self, d_in: *const u8, d_nbytes: *const u16, d_bad_frame: *const u8, d_pcm: *mut i16, slot_bytes: usize,
                                    n_frames: usize, hip_stream: *mut c_void) -> i32 {
        lc3gpu_decode_vbr(self.h, d_in, d_nbytes, d_bad_frame, d_pcm, slot_bytes as i32, n_frames as i32, hip_stream)
    }
    /// The caller's choice of channel per `decode_frame` call (examples/decode.rs:93-112) for many channels in one launch: item i of the
    /// compact buffers holds the frames of channel `channels[i]` (any order, none twice); the other channels keep state and PLC count.
    ///
    /// # Safety
    /// device allocations of [channels.len()][frame][nbytes] u8, [channels.len()][frame] u8 flags or null, [channels.len()][frame][nf] i16
    /// that outlive the call's work; `channels` is host memory and free again when the call returns.
    pub unsafe fn decode_list_device(&mut self, channels: &[i32], d_in: *const u8, d_bad_frame: *const u8, d_pcm: *mut i16, nbytes: usize,
                                     n_frames: usize, hip_stream: *mut c_void) -> i32 {
        lc3gpu_decode_list(self.h, channels.as_ptr(), channels.len() as i32, d_in, d_bad_frame, d_pcm, nbytes as i32, n_frames as i32, hip_stream)
    }
    /// The same choice on a mixed-configuration handle: ragged buffers (and flags) compact in list order, include/lc3gpu.h.
    ///
    /// # Safety
    /// device allocations laid out as include/lc3gpu.h states for lc3gpu_decode_mixed_list that outlive the call's work; `channels` is
    /// host memory and free again when the call returns.
    pub unsafe fn decode_mixed_list_device(&mut self, channels: &[i32], d_in: *const u8, d_bad_frame: *const u8, d_pcm: *mut i16,
                                           n_frames: usize, hip_stream: *mut c_void) -> i32 {
        lc3gpu_decode_mixed_list(self.h, channels.as_ptr(), channels.len() as i32, d_in, d_bad_frame, d_pcm, n_frames as i32, hip_stream)
    }
    /// A frame count and a frame size per listed stream (decoder/lc3_decoder.rs:217-234 once per (channel, frame)).
    ///
    /// # Safety
    /// device allocations laid out as include/lc3gpu.h states for lc3gpu_decode_mixed_items that outlive the call's work; `items` is host
    /// memory and free again when the call returns.
    pub unsafe fn decode_mixed_items_device(&mut self, items: &[Lc3GpuItem], d_in: *const u8, d_bad_frame: *const u8, d_pcm: *mut i16,
                                            hip_stream: *mut c_void) -> i32 {
        lc3gpu_decode_mixed_items(self.h, items.as_ptr(), items.len() as i32, d_in, d_bad_frame, d_pcm, hip_stream)
    }
    /// Multi-channel items: the channels' frames back to back in, WAV sample order out (examples/decode.rs:93-118).
    ///
    /// # Safety
    /// device allocations laid out as include/lc3gpu.h states for lc3gpu_decode_mixed_mc_items that outlive the call's work; `items` is
    /// host memory and free again when the call returns.
    pub unsafe fn decode_mixed_mc_items_device(&mut self, items: &[Lc3GpuMcItem], d_in: *const u8, d_bad_frame: *const u8, d_pcm: *mut i16,
                                               hip_stream: *mut c_void) -> i32 {
        lc3gpu_decode_mixed_mc_items(self.h, items.as_ptr(), items.len() as i32, d_in, d_bad_frame, d_pcm, hip_stream)
    }
    /// Views: frames read where they lie, PCM written where it belongs, nothing else touched (lc3gpu_decode_mixed_views).
    ///
    /// # Safety
    /// device allocations of at least `in_bytes` bytes, `n_flags` flags (or a null `d_bad_frame`) and `pcm_elems` elements that outlive
    /// the call's work; `views` is host memory and free again when the call returns.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn decode_mixed_views_device(&mut self, views: &[Lc3GpuView], d_in: *const u8, in_bytes: usize, d_bad_frame: *const u8, n_flags: usize,
                                            d_pcm: *mut i16, pcm_elems: usize, hip_stream: *mut c_void) -> i32 {
        lc3gpu_decode_mixed_views(self.h, views.as_ptr(), views.len() as i32, d_in, in_bytes, d_bad_frame, n_flags, d_pcm, pcm_elems, hip_stream)
    }
    /// a new `DecoderChannel` for each named channel (from its next call on; no wait; its PLC count goes to zero)
    pub fn reset_channels(&mut self, channels: &[i32]) -> Result<(), i32> {
        let rc = unsafe { lc3gpu_decoder_reset_channels(self.h, channels.as_ptr(), channels.len() as i32) };
        if rc == 0 { Ok(()) } else { Err(rc) }
    }
    /// frames concealed so far (decoder/packet_loss_concealment.rs:63-85)
    pub fn plc_events(&mut self) -> u64 {
        let mut v = 0u64;
        unsafe { lc3gpu_decoder_plc_events(self.h, &mut v) };
        v
    }
}
impl Drop for Lc3DecoderGpu {
    fn drop(&mut self) {
        unsafe {
            lc3gpu_decoder_destroy(self.h);
        }
    }
}

/// lc3gpu_inspect (include/lc3gpu.h): the side information and decode status of `n_frames` frames, no handle needed.  A status of
/// LC3GPU_FRAME_SIDE_INFO + k is `Lc3DecoderError::SideInfo`, LC3GPU_FRAME_ARITH + k `Lc3DecoderError::ArithmeticDecode` (INTEGRATION.md).
///
/// # Safety
/// device allocations: `d_in` of n_frames * slot_bytes bytes, `d_info` of n_frames records, `d_nbytes` / `d_bad_frame` of n_frames
/// entries or null; they must stay valid until the work on `hip_stream` is done.
pub unsafe fn inspect_device(d: FrameDuration, f: SamplingFrequency, d_in: *const u8, d_nbytes: *const u16, d_bad_frame: *const u8, slot_bytes: usize,
                             n_frames: usize, d_info: *mut Lc3GpuFrameInfo, hip_stream: *mut c_void) -> i32 {
    lc3gpu_inspect(frame_us(d), fs_hz(f), d_in, d_nbytes, d_bad_frame, slot_bytes as i32, n_frames as i32, d_info, hip_stream)
}

/// The inspector (include/lc3gpu.h): the status and the side information of every frame of a tick, read where the frames lie and written
/// where their flags lie -- for the very views the tick passes to `decode_mixed_views_device`.  Independent of every codec handle.
pub struct Lc3InspectorGpu {
    h: *mut Lc3GpuInspector,
}
impl Lc3InspectorGpu {
    /// `descs`: the array the caller passes to lc3gpu_decoder_create_mixed; `max_views`: the most views one call may name
    pub fn new(descs: &[Lc3GpuStreamDesc], max_views: usize) -> Result<Self, i32> {
        let mut h = core::ptr::null_mut();
        let rc = unsafe { lc3gpu_inspector_create(&mut h, descs.len() as i32, descs.as_ptr(), max_views as i32) };
        if rc == LC3GPU_OK { Ok(Self { h }) } else { Err(rc) }
    }
    /// One launch over all views: frame t of a view gets its status byte at `d_status[flag_off + t * flag_pitch]` and its 128-byte record at
    /// `d_info[...]` of the same index; either output may be null, not both.
    ///
    /// # Safety
    /// device allocations of at least `in_bytes` bytes, `n_flags` flags (or a null `d_bad_frame`), `n_status` bytes and `n_info` records
    /// (either may be null) that outlive the call's work; every view is checked against these extents on the host.  `views` is host memory
    /// and free again when the call returns.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn inspect_mixed_views_device(&mut self, views: &[Lc3GpuView], d_in: *const u8, in_bytes: usize, d_bad_frame: *const u8, n_flags: usize,
                                             d_status: *mut u8, n_status: usize, d_info: *mut Lc3GpuFrameInfo, n_info: usize,
                                             hip_stream: *mut c_void) -> i32 {
        lc3gpu_inspect_mixed_views(self.h, views.as_ptr(), views.len() as i32, d_in, in_bytes, d_bad_frame, n_flags, d_status, n_status, d_info, n_info,
                                   hip_stream)
    }
}
impl Drop for Lc3InspectorGpu {
    fn drop(&mut self) {
        unsafe {
            lc3gpu_inspector_destroy(self.h);
        }
    }
}

/// The analyzer (include/lc3gpu.h): the reconstructed spectrum, the 64 band energies and the total energy of every frame of a tick, read
/// where the frames lie and written at the frames' flag indices -- for the very views the tick passes to `decode_mixed_views_device`,
/// without decoding to PCM.  Independent of every codec handle and of the inspector.
pub struct Lc3AnalyzerGpu {
    h: *mut Lc3GpuAnalyzer,
}
impl Lc3AnalyzerGpu {
    /// `descs`: the array the caller passes to lc3gpu_decoder_create_mixed; `max_views` / `max_frames`: the most views one call may name
    /// and the most frames it may hold (one scratch column per frame is allocated here)
    pub fn new(descs: &[Lc3GpuStreamDesc], max_views: usize, max_frames: usize) -> Result<Self, i32> {
        let mut h = core::ptr::null_mut();
        let rc = unsafe { lc3gpu_analyzer_create(&mut h, descs.len() as i32, descs.as_ptr(), max_views as i32, max_frames as i32) };
        if rc == LC3GPU_OK { Ok(Self { h }) } else { Err(rc) }
    }
    /// One launch over all views: frame t of a view, with i = flag_off + t * flag_pitch, gets its energy at `d_energy[i]` (-1.0 for a frame
    /// the decoder would conceal), its LC3GPU_BANDS band energies at `d_bands[i * 64 ..]` and its LC3GPU_SPEC_LINES lines at
    /// `d_spec[i * 400 ..]`; any output may be null, not all three.
    ///
    /// # Safety
    /// device allocations of at least `in_bytes` bytes, `n_flags` flags (or a null `d_bad_frame`), `n_energy` floats, `n_bands` rows of 64
    /// floats and `n_spec` rows of 400 floats (16-byte aligned; each may be null) that outlive the call's work; every view is checked
    /// against these extents on the host.  `views` is host memory and free again when the call returns.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn analyze_mixed_views_device(&mut self, views: &[Lc3GpuView], d_in: *const u8, in_bytes: usize, d_bad_frame: *const u8, n_flags: usize,
                                             d_energy: *mut f32, n_energy: usize, d_bands: *mut f32, n_bands: usize, d_spec: *mut f32, n_spec: usize,
                                             hip_stream: *mut c_void) -> i32 {
        lc3gpu_analyze_mixed_views(self.h, views.as_ptr(), views.len() as i32, d_in, in_bytes, d_bad_frame, n_flags, d_energy, n_energy, d_bands, n_bands,
                                   d_spec, n_spec, hip_stream)
    }
}
impl Drop for Lc3AnalyzerGpu {
    fn drop(&mut self) {
        unsafe {
            lc3gpu_analyzer_destroy(self.h);
        }
    }
}

/// The mixer (include/lc3gpu.h): the room mixes of a tick, the PCM read where `decode_mixed_views_device` wrote it and written where
/// `encode_mixed_views_device` reads it, in one launch.  Independent of every codec handle, of the inspector and of the analyzer.
pub struct Lc3MixerGpu {
    h: *mut Lc3GpuMixer,
}
impl Lc3MixerGpu {
    /// `descs`: the array the caller passes to lc3gpu_decoder_create_mixed (only fs_hz and frame_us are used); `max_views`: the most
    /// input plus output views one call may name, and the number of buses
    pub fn new(descs: &[Lc3GpuStreamDesc], max_views: usize) -> Result<Self, i32> {
        let mut h = core::ptr::null_mut();
        let rc = unsafe { lc3gpu_mixer_create(&mut h, descs.len() as i32, descs.as_ptr(), max_views as i32) };
        if rc == LC3GPU_OK { Ok(Self { h }) } else { Err(rc) }
    }
    /// One launch over all rooms: output o gets, sample by sample, the clamped sum of its bus's inputs (each scaled by its gain_q14,
    /// rounded to nearest) less the term of input `outs[o].minus`.  `ins[i]` belongs to `in_views[i]`, `outs[o]` to `out_views[o]`.
    ///
    /// # Safety
    /// device allocations of at least `in_elems` and `out_elems` elements that do not overlap and outlive the call's work; every view is
    /// checked against these extents on the host.  The four slices are host memory and free again when the call returns.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn mix_mixed_views_device(&mut self, in_views: &[Lc3GpuView], ins: &[Lc3GpuMixIn], d_pcm_in: *const i16, in_elems: usize,
                                         out_views: &[Lc3GpuView], outs: &[Lc3GpuMixOut], d_pcm_out: *mut i16, out_elems: usize,
                                         hip_stream: *mut c_void) -> i32 {
        assert_eq!(in_views.len(), ins.len());
        assert_eq!(out_views.len(), outs.len());
        lc3gpu_mix_mixed_views(self.h, in_views.as_ptr(), ins.as_ptr(), in_views.len() as i32, d_pcm_in, in_elems, out_views.as_ptr(),
                               outs.as_ptr(), out_views.len() as i32, d_pcm_out, out_elems, hip_stream)
    }
}
impl Drop for Lc3MixerGpu {
    fn drop(&mut self) {
        unsafe {
            lc3gpu_mixer_destroy(self.h);
        }
    }
}

/// The resampler (include/lc3gpu.h): the rate conversions of a tick, the PCM read where one view array says and written where a second
/// says, in one launch, a FIR history per channel.  Independent of every codec handle and of the three other companions.
pub struct Lc3ResamplerGpu {
    h: *mut Lc3GpuResampler,
}
impl Lc3ResamplerGpu {
    /// `descs`: one (fs_in_hz, fs_out_hz, frame_us) per channel; `max_views`: the most pairs of views one call may name
    pub fn new(descs: &[Lc3GpuRateDesc], max_views: usize) -> Result<Self, i32> {
        let mut h = core::ptr::null_mut();
        let rc = unsafe { lc3gpu_resampler_create(&mut h, descs.len() as i32, descs.as_ptr(), max_views as i32) };
        if rc == LC3GPU_OK { Ok(Self { h }) } else { Err(rc) }
    }
    /// Every channel reads a zero history in its next call; waits for nothing, launches nothing.
    pub fn reset(&mut self) -> i32 {
        unsafe { lc3gpu_resampler_reset(self.h) }
    }
    /// The named channels read a zero history in their next call.
    pub fn reset_channels(&mut self, channels: &[i32]) -> i32 {
        unsafe { lc3gpu_resampler_reset_channels(self.h, channels.as_ptr(), channels.len() as i32) }
    }
    /// One launch over all listed channels: `in_views[i]` and `out_views[i]` belong together (same channel, same n_frames, a channel once
    /// per call); every output sample is the clamped, rounded int32 FIR sum over the view's input and the channel's history.
    ///
    /// # Safety
    /// device allocations of at least `in_elems` and `out_elems` elements that do not overlap and outlive the call's work; every view is
    /// checked against these extents on the host.  The two slices are host memory and free again when the call returns.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn resample_mixed_views_device(&mut self, in_views: &[Lc3GpuView], d_pcm_in: *const i16, in_elems: usize, out_views: &[Lc3GpuView],
                                              d_pcm_out: *mut i16, out_elems: usize, hip_stream: *mut c_void) -> i32 {
        assert_eq!(in_views.len(), out_views.len());
        lc3gpu_resample_mixed_views(self.h, in_views.as_ptr(), d_pcm_in, in_elems, out_views.as_ptr(), d_pcm_out, out_elems,
                                    in_views.len() as i32, hip_stream)
    }
}
impl Drop for Lc3ResamplerGpu {
    fn drop(&mut self) {
        unsafe {
            lc3gpu_resampler_destroy(self.h);
        }
    }
}

/// The meter (include/lc3gpu.h): the PCM levels and the speech gate of a tick, the PCM read where one view array says it lies, in one
/// launch, a small state per channel carried from call to call.  Independent of every other object.
pub struct Lc3MeterGpu {
    h: *mut Lc3GpuMeter,
}
impl Lc3MeterGpu {
    /// `descs`: one descriptor per channel; `max_views`: the most views one call may name
    pub fn new(descs: &[Lc3GpuMeterDesc], max_views: usize) -> Result<Self, i32> {
        let mut h = core::ptr::null_mut();
        let rc = unsafe { lc3gpu_meter_create(&mut h, descs.len() as i32, descs.as_ptr(), max_views as i32) };
        if rc == LC3GPU_OK { Ok(Self { h }) } else { Err(rc) }
    }
    /// Every channel starts from last = 0, env = 0, hang = 0 in its next call; waits for nothing, launches nothing.
    pub fn reset(&mut self) -> i32 {
        unsafe { lc3gpu_meter_reset(self.h) }
    }
    /// The named channels start fresh in their next call.
    pub fn reset_channels(&mut self, channels: &[i32]) -> i32 {
        unsafe { lc3gpu_meter_reset_channels(self.h, channels.as_ptr(), channels.len() as i32) }
    }
    /// One launch over all listed channels (a channel once per call): frame t of a view gets its activity byte at `d_active[flag_off + t *
    /// flag_pitch]` and its 32-byte record at `d_levels[...]` of the same index; either output may be null, not both.
    ///
    /// # Safety
    /// device allocations of at least `pcm_elems` elements, `n_active` bytes and `n_levels` records (16-byte aligned; either output may be
    /// null) that do not overlap and outlive the call's work; every view is checked against these extents on the host.  `views` is host
    /// memory and free again when the call returns.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn measure_mixed_views_device(&mut self, views: &[Lc3GpuView], d_pcm: *const i16, pcm_elems: usize, d_active: *mut u8, n_active: usize,
                                             d_levels: *mut Lc3GpuLevel, n_levels: usize, hip_stream: *mut c_void) -> i32 {
        lc3gpu_measure_mixed_views(self.h, views.as_ptr(), views.len() as i32, d_pcm, pcm_elems, d_active, n_active, d_levels, n_levels, hip_stream)
    }
}
impl Drop for Lc3MeterGpu {
    fn drop(&mut self) {
        unsafe {
            lc3gpu_meter_destroy(self.h);
        }
    }
}

/// Encode + decode of many channels in the arrangement that measured fastest (include/lc3gpu.h, "pipeline"): device buffers, asynchronous.
pub struct Lc3PipelineGpu {
    h: *mut Lc3GpuPipeline,
}
impl Lc3PipelineGpu {
    pub fn new(num_channels: usize, d: FrameDuration, f: SamplingFrequency) -> Self {
        let mut h = core::ptr::null_mut();
        let rc = unsafe { lc3gpu_pipeline_create(&mut h, num_channels as i32, frame_us(d), fs_hz(f), 0) };
        assert_eq!(rc, LC3GPU_OK, "lc3gpu_pipeline_create: {}", rc);
        Self { h }
    }
    /// # Safety
    /// device pointers of [channel][frame][nf] i16, [channel][frame][nbytes] u8, [channel][frame][nf] i16 that stay valid until `wait`.
    pub unsafe fn submit(&mut self, d_pcm: *const i16, d_bytes: *mut u8, d_pcm_out: *mut i16, nbytes: usize, n_frames: usize) -> i32 {
        lc3gpu_pipeline_submit(self.h, d_pcm, d_bytes, d_pcm_out, nbytes as i32, n_frames as i32)
    }
    pub fn wait(&mut self) -> i32 {
        unsafe { lc3gpu_pipeline_wait(self.h) }
    }
}
impl Drop for Lc3PipelineGpu {
    fn drop(&mut self) {
        unsafe {
            lc3gpu_pipeline_destroy(self.h);
        }
    }
}
'''


def generate():
    lines = [
        "// bindings/lc3gpu.rs -- Rust binding of liblc3gpu.so (include/lc3gpu.h), GENERATED by tools/gen_rust_binding.py: do not edit.",
        "//",
        "// Drop it into the reference crate as src/gpu.rs behind `#[cfg(feature = \"mi355x\")]`; build.rs:",
        "//   println!(\"cargo:rustc-link-search=native=<repo>/lc3-codec_amd/lib\"); println!(\"cargo:rustc-link-lib=dylib=lc3gpu\");",
        "// Not compiled in this repository (the image has no Rust toolchain); tests/test_abi.py checks that the extern block binds every",
        "// symbol include/lc3gpu.h declares, with the header's parameter lists, and that this file is what the generator writes.",
        "#![allow(dead_code, non_camel_case_types, clippy::too_many_arguments, clippy::missing_safety_doc)]",
        "use core::ffi::{c_char, c_void};",
        "",
    ]
    for c, r in sorted(OPAQUE.items()):
        if c in ("lc3gpu_stream_desc", "lc3gpu_frame_info", "lc3gpu_item", "lc3gpu_mc_item", "lc3gpu_view", "lc3gpu_mix_in", "lc3gpu_mix_out",
                 "lc3gpu_rate_desc", "lc3gpu_meter_desc", "lc3gpu_level"):
            continue
        lines += ["#[repr(C)]", "pub struct %s {" % r, "    _private: [u8; 0],", "}"]
    lines += ["/// one stream of a mixed-configuration handle (lc3gpu_stream_desc)", "#[repr(C)]", "#[derive(Clone, Copy, Debug)]",
              "pub struct Lc3GpuStreamDesc {", "    pub fs_hz: i32,", "    pub frame_us: i32,", "    pub nbytes: i32,", "}"]
    lines += ["/// one item of the *_mixed_items calls (lc3gpu_item, 16 bytes): a stream, its frames in this call and their size (0 = the",
              "/// descriptor's)", "#[repr(C)]", "#[derive(Clone, Copy, Debug, Default)]", "pub struct Lc3GpuItem {", "    pub channel: i32,",
              "    pub n_frames: i32,", "    pub nbytes: i32,", "    pub reserved: i32,", "}",
              "const _: () = assert!(core::mem::size_of::<Lc3GpuItem>() == 16);"]
    lines += ["/// one item of the *_mixed_mc_items calls (lc3gpu_mc_item, 16 bytes): the channels of one stream, its frames in this call and their",
              "/// size (0 = the descriptors')", "#[repr(C)]", "#[derive(Clone, Copy, Debug, Default)]", "pub struct Lc3GpuMcItem {",
              "    pub first_channel: i32,", "    pub n_channels: i32,", "    pub n_frames: i32,", "    pub nbytes: i32,", "}",
              "const _: () = assert!(core::mem::size_of::<Lc3GpuMcItem>() == 16);"]
    lines += ["/// one view of the *_mixed_views calls (lc3gpu_view, 64 bytes): an item -- channel, frames in this call, their size (0 = the",
              "/// descriptor's) -- with the placement of its PCM, its frames and its flags in the caller's buffers; a pitch of 0 = the compact one",
              "#[repr(C)]", "#[derive(Clone, Copy, Debug, Default)]", "pub struct Lc3GpuView {", "    pub channel: i32,", "    pub n_frames: i32,",
              "    pub nbytes: i32,", "    pub pcm_stride: i32,", "    pub pcm_off: i64,", "    pub byte_off: i64,", "    pub flag_off: i64,",
              "    pub pcm_pitch: i32,", "    pub byte_pitch: i32,", "    pub flag_pitch: i32,", "    pub reserved: [i32; 3],", "}",
              "const _: () = assert!(core::mem::size_of::<Lc3GpuView>() == 64);"]
    lines += ["/// one input of lc3gpu_mix_mixed_views (lc3gpu_mix_in, 8 bytes): the room it is heard in and its gain (16384 = unity)",
              "#[repr(C)]", "#[derive(Clone, Copy, Debug, Default)]", "pub struct Lc3GpuMixIn {", "    pub bus: i32,", "    pub gain_q14: i32,", "}",
              "const _: () = assert!(core::mem::size_of::<Lc3GpuMixIn>() == 8);"]
    lines += ["/// one output of lc3gpu_mix_mixed_views (lc3gpu_mix_out, 8 bytes): the room it hears and the input it does not hear (-1 = none)",
              "#[repr(C)]", "#[derive(Clone, Copy, Debug, Default)]", "pub struct Lc3GpuMixOut {", "    pub bus: i32,", "    pub minus: i32,", "}",
              "const _: () = assert!(core::mem::size_of::<Lc3GpuMixOut>() == 8);"]
    lines += ["/// one channel of lc3gpu_resampler_create (lc3gpu_rate_desc, 12 bytes): the rate it comes at, the rate it leaves at, the duration",
              "#[repr(C)]", "#[derive(Clone, Copy, Debug, Default)]", "pub struct Lc3GpuRateDesc {", "    pub fs_in_hz: i32,", "    pub fs_out_hz: i32,",
              "    pub frame_us: i32,", "}", "const _: () = assert!(core::mem::size_of::<Lc3GpuRateDesc>() == 12);"]
    lines += ["/// one channel of lc3gpu_meter_create (lc3gpu_meter_desc, 24 bytes): rate, duration, the envelope's two coefficients (Q15), the gate's",
              "/// threshold (mean square of i16 samples, 0..2^30) and its hang-over in frames", "#[repr(C)]", "#[derive(Clone, Copy, Debug, Default)]",
              "pub struct Lc3GpuMeterDesc {", "    pub fs_hz: i32,", "    pub frame_us: i32,", "    pub attack_q15: i32,", "    pub release_q15: i32,",
              "    pub threshold: u32,", "    pub hang_frames: i32,", "}", "const _: () = assert!(core::mem::size_of::<Lc3GpuMeterDesc>() == 24);"]
    lines += ["/// one frame's record of lc3gpu_measure_mixed_views (lc3gpu_level, 32 bytes)", "#[repr(C)]", "#[derive(Clone, Copy, Debug, Default)]",
              "pub struct Lc3GpuLevel {", "    pub sum_sq: i64,", "    pub env: u32,", "    pub sum: i32,", "    pub min: i16,", "    pub max: i16,",
              "    pub n_clipped: u16,", "    pub n_cross: u16,", "    pub hang: u16,", "    pub active: u8,", "    pub reserved0: u8,",
              "    pub reserved1: u32,", "}", "const _: () = assert!(core::mem::size_of::<Lc3GpuLevel>() == 32);"]
    lines += ["/// one frame's record of lc3gpu_inspect (lc3gpu_frame_info, 128 bytes): status LC3GPU_FRAME_*, the side information",
              "/// (decoder/side_info.rs:20-31) and the arithmetic data (decoder/arithmetic_codec.rs:99-107)", "#[repr(C)]",
              "#[derive(Clone, Copy, Debug, Default)]", "pub struct Lc3GpuFrameInfo {"]
    lines += ["    pub %s: %s," % f for f in frame_info_fields()]
    lines += ["}", "const _: () = assert!(core::mem::size_of::<Lc3GpuFrameInfo>() == 128);", ""]
    for name, val in constants():
        lines.append("pub const %s: i32 = %d;" % (name, val))
    lines += ["", "#[link(name = \"lc3gpu\")]", "extern \"C\" {"]
    for name, ps, ret in declarations():
        sig = ", ".join("%s: %s" % p for p in ps)
        lines.append("    pub fn %s(%s)%s;" % (name, sig, (" -> " + ret) if ret else ""))
    lines.append("}")
    return "\n".join(lines) + "\n" + WRAPPERS


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "bindings", "lc3gpu.rs")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(generate())


if __name__ == "__main__":
    main()
