"""The byte output as files: a baseline-JPEG encoder on the GPU (tg_jpeg_coeffs, tg_jpeg_segment_bytes, tg_jpeg_write, csrc/jpeg.hip) and a Motion-JPEG AVI writer
in plain Python around it (the container itself: avi.py; the frame contract: frames.py); DESIGN.md §8k.  No reference code: the header's comment is the definition, tests/jpeg_ref.py restates it, tests/avi_ref.py walks the file.

    from tokensgen_amd.jpeg import encode_jpeg, save_jpeg, MJPEGWriter, write_mjpeg_avi

`encode_jpeg` turns uint8 frames on the device into one device buffer that holds every frame's JPEG and the host offsets that cut it.  Integer arithmetic, the
standard Huffman tables, every restart segment coded on its own: a frame is one exact byte string, the same alone and in a batch.  The size pass and the write pass are
separated by the one host read of an encode, the total size.  `MJPEGWriter` puts the frames into an AVI 1.0 file with an index (no OpenDML: a file stays below 2 GiB).

uint8 frames only ("uint8" of video_io.VideoProcessor).  Every refusal comes before any kernel call.  There is no CPU path.

And back: a baseline-JPEG decoder on the GPU (tg_jpeg_find_segments, tg_jpeg_decode_coeffs, tg_jpeg_idct_rgb, csrc/jpeg_decode.hip) behind a header
parser in plain Python, and an AVI 1.0 reader around it; tests/jpeg_dec_ref.py restates the definition.

    from tokensgen_amd.jpeg import parse_jpeg, decode_jpeg, load_jpeg, MJPEGReader, read_mjpeg_avi

`parse_jpeg` holds every refusal (progressive, arithmetic coding, 12-bit, other sampling factors, ...), `decode_jpeg` turns a batch of streams into uint8 frames on the
device with one copy up and one wait, `MJPEGReader` reads our own files and any other baseline Motion-JPEG AVI.  Streams without restart markers, what most
encoders write, are decoded in parallel inside the frame (tg_jpeg_decode_coeffs_sync, csrc/jpeg_decode_sync.hip): `entropy_plan` says when."""
import functools
import os
import re
import struct
from typing import NamedTuple

import numpy as np
import torch

from . import avi
from . import kernels as K
from .frames import check_device, check_frames, gpu_device, is_int, single_frame, split_bytes

SUBSAMPLINGS = tuple(K.JPEG_SUBSAMPLINGS)


def check_params(quality, subsampling, restart_interval, who):
    if not is_int(quality) or not 1 <= quality <= 100:
        raise ValueError(f"{who}: quality must be an integer in 1..100, got {quality!r}")
    if subsampling not in SUBSAMPLINGS:
        raise ValueError(f"{who}: subsampling must be one of {SUBSAMPLINGS}, got {subsampling!r}")
    if not is_int(restart_interval) or not 1 <= restart_interval <= 65535:
        raise ValueError(f"{who}: restart_interval must be an integer in 1..65535, got {restart_interval!r}")


def check_jpeg_frames(frames, who, dims=(4, 5)):
    """frames.check_frames and what is JPEG's own: SOF0 holds a frame's sides in 16 bits"""
    check_frames(frames, who, dims)
    if frames.shape[-3] > 65535 or frames.shape[-2] > 65535:
        raise ValueError(f"{who}: a JPEG frame is at most 65535 x 65535, got {frames.shape[-3]} x {frames.shape[-2]}")


def stream_offsets(seg_bytes, header):
    """The prefix sums between the size pass and the write pass, on the device: seg_bytes int32 [F, n_seg] -> (where every segment starts in the buffer, int64
    [F, n_seg]; where every frame starts, int64 [F]; where it ends, int64 [F])."""
    ends = torch.cumsum(seg_bytes, 1, dtype=torch.int64)                       # of a frame's segments, from the end of its header
    totals = ends[:, -1] + header
    frame_ends = torch.cumsum(totals, 0)
    frame_offsets = frame_ends - totals
    return ((frame_offsets + header)[:, None] + (ends - seg_bytes)).contiguous(), frame_offsets.contiguous(), frame_ends


def encode_jpeg(frames, quality=90, subsampling="420", restart_interval=1):
    """uint8 [F, H, W, 3] (or [B, T, H, W, 3], frames in order) on the device -> (data, offsets): data a uint8 device tensor of exactly offsets[-1] bytes, offsets int64
    [F + 1] on the host; frame f is data[offsets[f]:offsets[f + 1]], a complete baseline JPEG.  subsampling "420" or "444"; restart_interval in MCUs: 1 (the default)
    gives the entropy pass one lane per MCU, a larger one a smaller file and less parallel work.  A view that is not contiguous is copied first."""
    check_jpeg_frames(frames, "encode_jpeg")
    check_params(quality, subsampling, restart_interval, "encode_jpeg")
    check_device(frames, "encode_jpeg")
    H, W = frames.shape[-3:-1]
    src = frames.contiguous().reshape(-1, H, W, 3)
    header = K.L.load().tg_jpeg_header_bytes()
    coef = K.jpeg_coeffs(src, quality, subsampling)
    seg = K.jpeg_segment_bytes(coef, H, W, subsampling, restart_interval)
    seg_offsets, frame_offsets, frame_ends = stream_offsets(seg, header)
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), frame_ends.cpu()])  # the one wait of the call
    data = torch.empty(int(offsets[-1]), dtype=torch.uint8, device=frames.device)
    K.jpeg_write(coef, H, W, quality, subsampling, restart_interval, seg_offsets, frame_offsets, data)
    return data, offsets


def jpeg_bytes(frames, quality=90, subsampling="420", restart_interval=1):
    """encode_jpeg, copied to the host and cut: a list of one `bytes` per frame."""
    return split_bytes(*encode_jpeg(frames, quality, subsampling, restart_interval))


def save_jpeg(frame, path, quality=90, subsampling="420", restart_interval=1):
    """One frame, uint8 [H, W, 3] (or [1, H, W, 3]) on the device, as a .jpg file."""
    check_jpeg_frames(frame, "save_jpeg", dims=(3, 4))
    one = single_frame(frame, "save_jpeg")
    check_params(quality, subsampling, restart_interval, "save_jpeg")
    check_device(frame, "save_jpeg")
    (b,) = jpeg_bytes(one, quality, subsampling, restart_interval)
    with open(path, "wb") as fh:
        fh.write(b)
    return path


class MJPEGWriter(avi.AVIWriter):
    """A Motion-JPEG AVI 1.0 file, written as the frames arrive (the container: avi.AVIWriter).  `write(frames)` (uint8 [F, H, W, 3] or [B, T, H, W, 3] on the
    device) or `write_jpegs` any number of times, then `close()`, which writes the index and the counts and sizes of the headers; or use it as a context manager.
    All frames of a file have one size.  fps is any positive number: dwRate / dwScale = Fraction(fps).limit_denominator(65535).  A `write` that would take the file
    past MAX_FILE_BYTES (2^31 - 1: no OpenDML) is refused whole with a ValueError, and `close()` still leaves a valid file of the frames before it."""

    BATCH = 64                                  # frames per encode call: bounds the coefficient workspace of a long video

    def __init__(self, path, fps, quality=90, subsampling="420", restart_interval=1):
        check_params(quality, subsampling, restart_interval, "MJPEGWriter")
        super().__init__(path, fps)
        self.quality, self.subsampling, self.restart_interval = quality, subsampling, restart_interval

    def write(self, frames):
        if self._fh is None:
            raise ValueError("MJPEGWriter.write: the file is closed")
        check_jpeg_frames(frames, "MJPEGWriter.write")
        H, W = frames.shape[-3:-1]
        self.check_size(H, W)
        check_device(frames, "MJPEGWriter.write")
        src = frames.reshape(-1, H, W, 3)
        chunks = []
        for i in range(0, src.shape[0], self.BATCH):
            chunks += jpeg_bytes(src[i:i + self.BATCH], self.quality, self.subsampling, self.restart_interval)
        return self.write_jpegs(chunks, H, W)


def write_mjpeg_avi(path, frames, fps, quality=90, subsampling="420", restart_interval=1):
    """All frames of one tensor as one Motion-JPEG AVI file; returns the path."""
    check_jpeg_frames(frames, "write_mjpeg_avi")
    check_device(frames, "write_mjpeg_avi")
    with MJPEGWriter(path, fps, quality, subsampling, restart_interval) as w:
        w.write(frames)
    return path


# ---- reading: the header parser, the decoder's host side and the AVI reader ------------------------------------------------------------------------

ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
# Annex K.3, what a frame without DHT uses (the AVI MJPG convention): (class << 4 | slot) -> (BITS, HUFFVAL)
_K3_AC0 = bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748494a535455565758595a636465666768696a"
    "737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")
_K3_AC1 = bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445464748494a535455565758595a636465666768696a"
    "737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")
STD_HUFFMAN = {0x00: (bytes([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]), bytes(range(12))),
               0x01: (bytes([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]), bytes(range(12))),
               0x10: (bytes([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d]), _K3_AC0),
               0x11: (bytes([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]), _K3_AC1)}
_SOF_NAMES = {0xc1: "SOF1 (extended sequential DCT)", 0xc2: "SOF2 (progressive DCT)", 0xc3: "SOF3 (lossless)", 0xc5: "SOF5 (differential sequential)",
              0xc6: "SOF6 (differential progressive)", 0xc7: "SOF7 (differential lossless)", 0xc9: "SOF9 (arithmetic coding)", 0xca: "SOF10 (arithmetic coding)",
              0xcb: "SOF11 (arithmetic coding)", 0xcd: "SOF13 (arithmetic coding)", 0xce: "SOF14 (arithmetic coding)", 0xcf: "SOF15 (arithmetic coding)"}
_SCAN_END = re.compile(rb"\xff[^\x00\xd0-\xd7\xff]")


class JpegInfo(NamedTuple):
    """What `parse_jpeg` reads from one frame's headers.  qtables: per component (Y, Cb, Cr) the 64 quantisers in natural order; huffman: per component
    ((BITS, HUFFVAL) of its DC table, (BITS, HUFFVAL) of its AC table); restart_interval 0: no markers; scan: (begin, end) of the entropy data in the frame's bytes."""
    height: int
    width: int
    subsampling: str
    restart_interval: int
    scan: tuple
    qtables: tuple
    huffman: tuple


def parse_jpeg(data, index=0):
    """The headers of one baseline JPEG frame (bytes-like) -> JpegInfo; pure Python, no device.  What the decoder does not take (progressive and the other SOFn,
    arithmetic coding, 12-bit samples, 16-bit DQT, one or four components, other sampling factors, several scans, Adobe RGB) raises NotImplementedError naming it; a
    stream that is malformed at the header level raises ValueError naming the frame `index`.  A scan without an EOI (a file cut short) parses: its range ends with the
    bytes, and the decoder reports what is missing."""
    d = bytes(data) if not isinstance(data, bytes) else data
    who = f"parse_jpeg: frame {index}"
    bad = lambda what: ValueError(f"{who}: {what}")
    if d[:2] != b"\xff\xd8":
        raise bad("no SOI (FF D8) at the start")
    pos, n = 2, len(d)
    qt, ht, sof, ri, adobe = {}, {}, None, 0, None
    while True:
        if pos + 2 > n:
            raise bad("the bytes end before SOS")
        if d[pos] != 0xff:
            raise bad(f"expected a marker at byte {pos}, found {d[pos]:#04x}")
        while pos < n and d[pos] == 0xff:                                       # fill bytes before a marker
            pos += 1
        if pos >= n:
            raise bad("the bytes end before SOS")
        m = d[pos]
        pos += 1
        if m == 0x01 or 0xd0 <= m <= 0xd7:                                      # TEM, a stray RSTn: no length
            continue
        if m == 0xd9:
            raise bad("EOI before SOS")
        if m == 0xd8:
            raise bad("a second SOI")
        if pos + 2 > n:
            raise bad(f"marker FF {m:02X} has no length")
        ln = struct.unpack_from(">H", d, pos)[0]
        if ln < 2 or pos + ln > n:
            raise bad(f"the segment of marker FF {m:02X} ({ln} bytes) runs past the end")
        seg = d[pos + 2:pos + ln]
        if m in _SOF_NAMES:
            raise NotImplementedError(f"{who}: {_SOF_NAMES[m]}; baseline sequential DCT (SOF0) only")
        if m == 0xcc:
            raise NotImplementedError(f"{who}: DAC (arithmetic coding); baseline Huffman only")
        if m == 0xc0:
            if sof is not None:
                raise bad("a second SOF0")
            if len(seg) < 6:
                raise bad("SOF0 is too short")
            prec, h, w, nc = struct.unpack_from(">BHHB", seg, 0)
            if prec != 8:
                raise NotImplementedError(f"{who}: {prec}-bit precision; 8-bit samples only")
            if nc != 3:
                raise NotImplementedError(f"{who}: {nc} component{'s' if nc != 1 else ' (grey scale)'}; three components (Y Cb Cr) only")
            if len(seg) != 6 + 3 * nc:
                raise bad("the length of SOF0 does not match its components")
            if h < 1 or w < 1:
                raise bad(f"a frame of {h} x {w} (a height given later by DNL is not read)")
            comps = [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(3)]     # id, h, v, quantiser slot
            samp = tuple((c[1], c[2]) for c in comps)
            if samp == ((2, 2), (1, 1), (1, 1)):
                sub = "420"
            elif samp == ((1, 1), (1, 1), (1, 1)):
                sub = "444"
            else:
                name = {((2, 1), (1, 1), (1, 1)): "4:2:2 ", ((1, 2), (1, 1), (1, 1)): "4:4:0 ", ((4, 1), (1, 1), (1, 1)): "4:1:1 "}.get(samp, "")
                raise NotImplementedError(f"{who}: sampling factors {name}({', '.join(f'{a}x{b}' for a, b in samp)}); (2x2, 1x1, 1x1) or all 1x1 only")
            if len({c[0] for c in comps}) != 3:
                raise bad("two components of SOF0 share an id")
            sof = (h, w, sub, comps)
        elif m == 0xdb:
            p = 0
            while p < len(seg):
                pq, slot = seg[p] >> 4, seg[p] & 15
                if pq != 0:
                    raise NotImplementedError(f"{who}: a 16-bit DQT; 8-bit quantisation tables only")
                if slot > 3 or p + 65 > len(seg):
                    raise bad("a DQT table that does not fit its segment, or a slot above 3")
                nat = [0] * 64
                for k in range(64):
                    nat[ZIGZAG[k]] = seg[p + 1 + k]
                if 0 in nat:
                    raise bad("a quantiser of 0")
                qt[slot] = tuple(nat)
                p += 65
        elif m == 0xc4:
            p = 0
            while p < len(seg):
                if p + 17 > len(seg):
                    raise bad("a DHT table that does not fit its segment")
                tc, slot, bits = seg[p] >> 4, seg[p] & 15, seg[p + 1:p + 17]
                cnt = sum(bits)
                if tc > 1 or slot > 3 or cnt > 256 or p + 17 + cnt > len(seg):
                    raise bad("a DHT table that does not fit its segment, a class above 1 or a slot above 3")
                ht[(tc << 4) | slot] = (bytes(bits), bytes(seg[p + 17:p + 17 + cnt]))
                p += 17 + cnt
        elif m == 0xdd:
            if len(seg) != 2:
                raise bad("DRI is not 4 bytes")
            ri = struct.unpack(">H", seg)[0]
        elif m == 0xee and seg[:5] == b"Adobe" and len(seg) >= 12:
            adobe = seg[11]
        elif m == 0xda:
            if sof is None:
                raise bad("SOS before SOF")
            if len(seg) < 1 or len(seg) != 4 + 2 * seg[0]:
                raise bad("the length of SOS does not match its components")
            if seg[0] != 3:
                raise NotImplementedError(f"{who}: more than one scan (a scan of {seg[0]} component{'s' if seg[0] != 1 else ''}); one interleaved scan only")
            h, w, sub, comps = sof
            if [seg[1 + 2 * i] for i in range(3)] != [c[0] for c in comps]:
                raise bad("the components of SOS are not those of SOF0, in its order")
            if tuple(seg[7:10]) != (0, 63, 0):
                raise NotImplementedError(f"{who}: a scan with Ss {seg[7]}, Se {seg[8]}, Ah/Al {seg[9]:#04x} (progressive); Ss 0, Se 63, Ah = Al = 0 only")
            if adobe == 0:
                raise NotImplementedError(f"{who}: Adobe APP14 with transform 0 (RGB components); Y Cb Cr only")
            tables = ht if ht else STD_HUFFMAN
            qtables, huffman = [], []
            for i in range(3):
                td, ta = seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15
                if comps[i][3] not in qt:
                    raise bad(f"quantisation table slot {comps[i][3]} is missing")
                if td not in tables or (0x10 | ta) not in tables:
                    raise bad(f"Huffman table slot DC {td} or AC {ta} is missing")
                qtables.append(qt[comps[i][3]])
                huffman.append((tables[td], tables[0x10 | ta]))
            begin = pos + ln
            hit = _SCAN_END.search(d, begin)
            if hit is None:
                end = n
            else:
                end = hit.start()
                while end > begin and d[end - 1] == 0xff:                       # fill bytes before the marker
                    end -= 1
                nxt = d[hit.start() + 1]
                if nxt != 0xd9:
                    what = "more than one scan" if nxt in (0xda, 0xc4, 0xdb, 0xdd) else f"marker FF {nxt:02X} after the scan"
                    raise NotImplementedError(f"{who}: {what}; one interleaved scan only")
            return JpegInfo(h, w, sub, ri, (begin, end), tuple(qtables), tuple(huffman))
        # APPn, COM and everything else with a length: skipped
        pos += ln


def _status_text(bits):
    return "; ".join(text for bit, text in K.JPEG_STATUS.items() if bits & bit) or f"status {bits}"


@functools.lru_cache(maxsize=64)
def _huffman_set(huffman):
    """the 6 x 912 bytes of one frame's tables: component c's DC at 2 c, AC at 2 c + 1"""
    return b"".join(K.jpeg_huff_table(*t) for comp in huffman for t in comp)


def _frames_of(data, offsets, who):
    """-> (list of bytes, the device tensor that already holds them or None, offsets list)"""
    if isinstance(data, torch.Tensor):
        if data.dtype != torch.uint8 or data.dim() != 1:
            raise ValueError(f"{who}: a tensor of streams is uint8 [n] with `offsets` as encode_jpeg returns them, got {data.dtype} {tuple(data.shape)}")
        if offsets is None:
            raise ValueError(f"{who}: a tensor of streams needs `offsets` (int64 [F + 1])")
        o = [int(v) for v in (offsets.tolist() if isinstance(offsets, torch.Tensor) else offsets)]
        if len(o) < 2 or o[0] < 0 or o[-1] > data.numel() or any(b <= a for a, b in zip(o, o[1:])):
            raise ValueError(f"{who}: offsets must rise from >= 0 to <= {data.numel()}, with at least one frame")
        host = data.cpu().numpy().tobytes()                                     # the headers are parsed on the host: one copy down
        return [host[a:b] for a, b in zip(o, o[1:])], (data if data.is_cuda else None), o
    if offsets is not None:
        raise ValueError(f"{who}: `offsets` goes with a tensor of streams, not with a list")
    if isinstance(data, (bytes, bytearray, memoryview)):
        data = [data]
    if not isinstance(data, (list, tuple)) or len(data) < 1 or any(not isinstance(c, (bytes, bytearray, memoryview)) for c in data):
        raise ValueError(f"{who}: expected a list of at least one `bytes`, or a uint8 tensor with offsets")
    chunks = [bytes(c) for c in data]
    o = [0]
    for c in chunks:
        o.append(o[-1] + len(c))
    return chunks, None, o


class JpegDecodeError(ValueError):
    """What decode_jpeg raises when the device reports a damaged stream: `frames` holds the decoded batch (the damaged restart segments are grey), `status` the int32
    [F] bits of include/tokensgen_hip.h on the host."""
    frames = None
    status = None


ENTROPY_MODES = ("auto", "segment", "sync")
# Set from profiles/jpeg_sync_bench.json (tools/bench_jpeg_decode.py --sync, 49 frames of 480 x 720).  SYNC_MIN_MCUS: the fewest MCUs per restart segment, of the
# intervals measured, from which tg_jpeg_decode_coeffs_sync beat one lane per segment on all four clips with the min - max ranges apart (at 90 it won on the two
# 4:2:0 clips only, at 45 on none).  SYNC_SUB_BYTES: 128 was the fastest of 64 / 128 / 256 on both smooth clips without markers and within a third of the fastest (256) on noise.
SYNC_MIN_MCUS = 270
SYNC_SUB_BYTES = 128


def entropy_plan(H, W, subsampling, restart_interval):
    """Which entropy launch decode_jpeg(entropy="auto") uses for frames of this geometry: ("segment", None), one lane per restart segment (tg_jpeg_decode_coeffs), or
    ("sync", sub_bytes), parallel decoding inside every segment (tg_jpeg_decode_coeffs_sync).  A pure function of the geometry, no device call.  "sync" where a
    segment holds at least SYNC_MIN_MCUS MCUs; a frame that is one segment (no markers, or an interval of at least its MCUs) qualifies from two MCUs on: one MCU is too
    small to cut.  restart_interval 0: no markers."""
    if not is_int(restart_interval) or not 0 <= restart_interval <= 65535:
        raise ValueError(f"entropy_plan: restart_interval must be an integer in 0..65535, got {restart_interval!r}")
    rows, cols, _, _ = K.jpeg_geometry(H, W, subsampling)
    n_mcu = rows * cols
    per_segment = n_mcu if restart_interval == 0 else min(restart_interval, n_mcu)
    if per_segment >= SYNC_MIN_MCUS or (per_segment == n_mcu and n_mcu >= 2):
        return ("sync", SYNC_SUB_BYTES)
    return ("segment", None)


def decode_jpeg(data, offsets=None, device=None, entropy="auto"):
    """Baseline JPEG frames -> uint8 [F, H, W, 3] on the device.  data: a list of `bytes` (one frame each), or a uint8 tensor holding all frames with `offsets` (int64
    [F + 1]) as encode_jpeg returns them; a device tensor is copied to the host once, for the header parsing, and decoded where it is.  All frames of a call share
    height, width, subsampling and restart interval (ValueError otherwise); their tables may differ.  The headers are parsed here (parse_jpeg), the bytes go up in one
    copy with the tables behind them, and after the launches the host reads status [F]: the one wait of a decode.  A non-zero entry raises JpegDecodeError (a
    ValueError) naming the first bad frame and the condition.
    entropy: "segment" decodes one lane per restart segment, so a stream without restart markers decodes with one lane per frame; "sync" decodes in parallel inside
    every segment and reads status and the decoder's own verdict `clean` in the same one wait; "auto" (the default) follows entropy_plan.  The result
    is the same byte array either way.  Where "sync" does not vouch for every frame (a damaged stream, or junk behind the last MCU that the serial decoder never
    reads), the call is decoded again by "segment", and that run's frames, status and JpegDecodeError are the result: a second wait, on that path only."""
    who = "decode_jpeg"
    if entropy not in ENTROPY_MODES:
        raise ValueError(f"{who}: entropy must be one of {ENTROPY_MODES}, got {entropy!r}")
    chunks, on_device, o = _frames_of(data, offsets, who)
    F = len(chunks)
    infos = [parse_jpeg(c, i) for i, c in enumerate(chunks)]
    first = infos[0]
    for i, info in enumerate(infos):
        if info[:4] != first[:4]:
            raise ValueError(f"{who}: all frames of a call share size, subsampling and restart interval; frame 0 is {first.height} x {first.width} {first.subsampling} "
                             f"interval {first.restart_interval}, frame {i} is {info.height} x {info.width} {info.subsampling} interval {info.restart_interval}")
    H, W, sub, ri = first[:4]
    dev = gpu_device(device if device is not None else (on_device.device if on_device is not None else None), who)
    hsets, qsets, hidx, qidx = {}, {}, [], []
    for i, info in enumerate(infos):
        try:
            hidx.append(hsets.setdefault(_huffman_set(info.huffman), len(hsets)))
        except ValueError as e:
            raise ValueError(f"{who}: frame {i}: {e}") from None
        qidx.append(qsets.setdefault(info.qtables, len(qsets)))
    # everything the kernels read beside the streams, as one 16-byte aligned record: scan_begin, scan_end int64 [F]; htab_index, qtab_index int32 [F]; the table sets
    meta = [np.array([o[i] + info.scan[0] for i, info in enumerate(infos)], np.int64), np.array([o[i] + info.scan[1] for i, info in enumerate(infos)], np.int64),
            np.array(hidx, np.int32), np.array(qidx, np.int32), np.frombuffer(b"".join(hsets), np.uint8), np.array(list(qsets), np.uint16).reshape(-1)]
    at, pos = [], 0 if on_device is not None else o[-1]
    for m in meta:
        pos += -pos % 16
        at.append(pos)
        pos += m.nbytes
    host = np.zeros(pos, np.uint8)
    if on_device is None:
        for i, c in enumerate(chunks):
            host[o[i]:o[i + 1]] = np.frombuffer(c, np.uint8)
    for a, m in zip(at, meta):
        host[a:a + m.nbytes] = m.view(np.uint8)
    up = torch.from_numpy(host).to(dev)                                         # the one copy up
    cut = lambda i, dtype: up[at[i]:at[i] + meta[i].nbytes].view(dtype)
    stream_dev = on_device.contiguous() if on_device is not None else up[:o[-1]]
    scan_begin, scan_end, htab_index, qtab_index = cut(0, torch.int64), cut(1, torch.int64), cut(2, torch.int32), cut(3, torch.int32)
    htabs, qtabs = cut(4, torch.uint8).view(len(hsets), -1), cut(5, torch.uint16).view(len(qsets), 3, 64)
    n_seg = K.jpeg_decode_segments(H, W, sub, ri)
    mode, sub_bytes = entropy_plan(H, W, sub, ri) if entropy == "auto" else (entropy, SYNC_SUB_BYTES)

    def launch(status, entropy_launch):
        """find the segments (which stores status), decode their coefficients by `entropy_launch`, transform: three launches, no wait"""
        seg_begin, seg_end = K.jpeg_find_segments(stream_dev, scan_begin, scan_end, n_seg, status)
        coef = entropy_launch(stream_dev, seg_begin, seg_end, H, W, sub, ri, htabs, htab_index)
        return K.jpeg_idct_rgb(coef, H, W, sub, qtabs, qtab_index)

    if mode == "sync":
        flags = torch.empty(3 * F, dtype=torch.int32, device=dev)               # status, clean and rounds: one buffer, one read
        out = launch(flags[:F], lambda *args: K.jpeg_decode_coeffs_sync(*args, sub_bytes, flags[F:2 * F], flags[2 * F:]))
        got = flags.cpu()                                                       # the one wait of the call
        if not bool(got[:F].any()) and bool((got[F:2 * F] == 1).all()):
            return out
        # not vouched for: the serial decoder decides, and its status, frames and error text are the result
    status = torch.empty(F, dtype=torch.int32, device=dev)
    out = launch(status, lambda *args: K.jpeg_decode_coeffs(*args, status))
    st = status.cpu()                                                           # the one wait of the call
    if bool(st.any()):
        f = int(torch.nonzero(st)[0])
        err = JpegDecodeError(f"{who}: frame {f}: {_status_text(int(st[f]))}" + (f" ({int((st != 0).sum())} damaged frames in all)" if int((st != 0).sum()) > 1 else ""))
        err.frames, err.status = out, st
        raise err
    return out


def load_jpeg(path, device=None):
    """One baseline .jpg file -> uint8 [H, W, 3] on the device; a file without restart markers is decoded in parallel inside the frame (entropy_plan)."""
    with open(path, "rb") as fh:
        return decode_jpeg([fh.read()], device=device)[0]


class MJPEGReader(avi.AVIReader):
    """A Motion-JPEG AVI 1.0 file (ours, or any baseline MJPG AVI; the container and what it takes and refuses: avi.AVIReader): `.frames` / len(), `.size` (H, W),
    `.fps` (a Fraction, dwRate / dwScale), `get_avg_fps()`; `get_batch(indices)` and `read(start=0, stop=None)` return uint8 [n, H, W, 3] on the device, decoded at
    most BATCH frames per decode_jpeg call (entropy "auto": frames without restart markers are decoded in parallel inside the frame); an index may repeat.  The
    constructor reads the headers, the index and the first frame's headers, which say the size; the frames are read from the file when asked for.  A context
    manager."""

    BATCH = 64

    def __init__(self, path, device=None):
        super().__init__(path)
        self.device = device
        if self._entries:
            try:
                info = parse_jpeg(self._read_at(*self._entries[0], "the first frame"), 0)
            except BaseException:
                self.close()
                raise
            self.size = (info.height, info.width)

    def get_batch(self, indices):
        """uint8 [len(indices), H, W, 3] on the device"""
        n, idx = len(self), []
        for i in indices:
            i = int(i)
            if not -n <= i < n:
                raise IndexError(f"MJPEGReader: frame {i} of {n}")
            idx.append(i % n)
        if not idx:
            raise ValueError("MJPEGReader.get_batch: no frame asked for")
        parts = []
        for s in range(0, len(idx), self.BATCH):
            piece = idx[s:s + self.BATCH]
            uniq = sorted(set(piece))                                           # a repeated index is decoded once
            try:
                dec = decode_jpeg(self.frame_bytes(uniq), device=self.device)
            except JpegDecodeError as e:
                bad = int(torch.nonzero(e.status)[0])
                raise ValueError(f"MJPEGReader: {self.path}: frame {uniq[bad]}: {_status_text(int(e.status[bad]))}") from None
            if uniq != piece:
                where = {u: k for k, u in enumerate(uniq)}
                dec = dec[torch.tensor([where[p] for p in piece], device=dec.device)]
            parts.append(dec)
        return parts[0] if len(parts) == 1 else torch.cat(parts)

    def read(self, start=0, stop=None):
        return self.get_batch(range(*slice(start, stop).indices(len(self))))


def read_mjpeg_avi(path, device=None):
    """All frames of one Motion-JPEG AVI file: (uint8 [F, H, W, 3] on the device, fps as a Fraction)."""
    with MJPEGReader(path, device) as r:
        return r.read(), r.fps


def load_video(video_path, output_res, nf_per_chunk, pad_to_fit, sample_fps, start_t, end_t, max_num_chunks, crop_to_fit=False, device=None):
    """video_io.load_video: see there."""
    from . import video_io
    ext = os.path.splitext(str(video_path))[1].lower()
    if ext != ".avi":
        raise ValueError(f"load_video: {video_path!r}: only the Motion-JPEG .avi format and numbered .png sequences are read (no {ext or 'suffix-less'} decoder here)")
    with MJPEGReader(video_path, device) as r:
        idx = video_io.sample_frame_indices(len(r), r.get_avg_fps(), nf_per_chunk, sample_fps, start_t, end_t, max_num_chunks)
        frames = r.get_batch(idx.tolist())
    return video_io.prepare_video(frames, output_res, crop_to_fit, pad_to_fit, device)


def export_to_video(video_frames, output_video_path, fps=8, quality=90):
    """video_io.export_to_video: see there."""
    ext = os.path.splitext(str(output_video_path))[1].lower()
    if ext != ".avi":
        raise ValueError(f"export_to_video: {output_video_path!r}: only the Motion-JPEG .avi format is written (no {ext or 'suffix-less'} encoder here)")
    check_jpeg_frames(video_frames, "export_to_video")
    if video_frames.dim() == 5 and video_frames.shape[0] != 1:
        raise ValueError(f"export_to_video: one video per file, got a batch of {video_frames.shape[0]}; pass video[i]")
    check_device(video_frames, "export_to_video")
    return write_mjpeg_avi(output_video_path, video_frames, fps, quality)
