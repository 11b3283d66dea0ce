"""The byte output as files: a baseline-JPEG encoder on the GPU (tg_jpeg_coeffs, tg_jpeg_segment_bytes, tg_jpeg_write, csrc/jpeg.hip) and a Motion-JPEG AVI writer
in plain Python around it; DESIGN.md §8k.  No reference code: the header's comment is the definition, tests/jpeg_ref.py restates it, tests/avi_ref.py walks the file.

    from tokensgen_amd.jpeg import encode_jpeg, save_jpeg, MJPEGWriter, write_mjpeg_avi

`encode_jpeg` turns uint8 frames on the device into one device buffer that holds every frame's JPEG and the host offsets that cut it.  Integer arithmetic, the
standard Huffman tables, every restart segment coded on its own: a frame is one exact byte string, the same alone and in a batch.  The size pass and the write pass are
separated by the one host read of an encode, the total size.  `MJPEGWriter` puts the frames into an AVI 1.0 file with an index (no OpenDML: a file stays below 2 GiB).

uint8 frames only ("uint8" of video_io.VideoProcessor).  Every refusal comes before any kernel call.  There is no CPU path."""
import os
import struct
from fractions import Fraction

import torch

from . import kernels as K

SUBSAMPLINGS = tuple(K.JPEG_SUBSAMPLINGS)


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def check_params(quality, subsampling, restart_interval, who):
    if not _is_int(quality) or not 1 <= quality <= 100:
        raise ValueError(f"{who}: quality must be an integer in 1..100, got {quality!r}")
    if subsampling not in SUBSAMPLINGS:
        raise ValueError(f"{who}: subsampling must be one of {SUBSAMPLINGS}, got {subsampling!r}")
    if not _is_int(restart_interval) or not 1 <= restart_interval <= 65535:
        raise ValueError(f"{who}: restart_interval must be an integer in 1..65535, got {restart_interval!r}")


def check_frames(frames, who, dims=(4, 5)):
    """The shape contract of every entry point, checked before any kernel call."""
    if not isinstance(frames, torch.Tensor):
        raise ValueError(f"{who}: expected a tensor of frames")
    if frames.dtype != torch.uint8:
        raise NotImplementedError(f"{who}: uint8 frames only (video_io's \"uint8\" output), got {frames.dtype}")
    want = " or ".join({3: "[H, W, 3]", 4: "[F, H, W, 3]", 5: "[B, T, H, W, 3]"}[d] for d in dims)
    if frames.dim() not in dims or frames.shape[-1] != 3 or frames.numel() < 1:
        raise ValueError(f"{who}: expected {want} (RGB, three channels) with at least one pixel, got {tuple(frames.shape)}")
    if frames.shape[-3] > 65535 or frames.shape[-2] > 65535:
        raise ValueError(f"{who}: a JPEG frame is at most 65535 x 65535, got {frames.shape[-3]} x {frames.shape[-2]}")


def check_device(frames, who):
    """after every other check, so that a wrong argument is named with or without a device"""
    if not frames.is_cuda:
        raise RuntimeError(f"{who}: expected a GPU tensor (tokensgen_amd has no CPU path)")


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
    check_frames(frames, "encode_jpeg")
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
    data, offsets = encode_jpeg(frames, quality, subsampling, restart_interval)
    host, o = data.cpu().numpy().tobytes(), offsets.tolist()
    return [host[o[i]:o[i + 1]] for i in range(len(o) - 1)]


def save_jpeg(frame, path, quality=90, subsampling="420", restart_interval=1):
    """One frame, uint8 [H, W, 3] (or [1, H, W, 3]) on the device, as a .jpg file."""
    check_frames(frame, "save_jpeg", dims=(3, 4))
    if frame.dim() == 4 and frame.shape[0] != 1:
        raise ValueError(f"save_jpeg: one frame per file, got {frame.shape[0]}")
    check_params(quality, subsampling, restart_interval, "save_jpeg")
    check_device(frame, "save_jpeg")
    (b,) = jpeg_bytes(frame.reshape(1, *frame.shape[-3:]), quality, subsampling, restart_interval)
    with open(path, "wb") as fh:
        fh.write(b)
    return path


AVIF_HASINDEX, AVIIF_KEYFRAME = 0x10, 0x10
_MOVI_FOURCC = 220                              # RIFF 12, LIST hdrl 8 + 192, LIST movi 8: where the 'movi' fourcc stands; the first chunk follows at 224


class MJPEGWriter:
    """A Motion-JPEG AVI 1.0 file, written as the frames arrive: RIFF 'AVI ' { LIST 'hdrl' { avih, LIST 'strl' { strh vids/MJPG, strf BITMAPINFOHEADER } }, LIST 'movi'
    { 00dc chunks, padded to even length }, idx1 }.  `write(frames)` (uint8 [F, H, W, 3] or [B, T, H, W, 3] on the device) any number of times, then `close()`, which
    writes the index and the counts and sizes of the headers; or use it as a context manager.  All frames of a file have one size.  fps is any positive number:
    dwRate / dwScale = Fraction(fps).limit_denominator(65535).  A `write` that would take the file past MAX_FILE_BYTES (2^31 - 1: no OpenDML) is refused whole with
    a ValueError, and `close()` still leaves a valid file of the frames before it."""

    MAX_FILE_BYTES = (1 << 31) - 1
    BATCH = 64                                  # frames per encode call: bounds the coefficient workspace of a long video

    def __init__(self, path, fps, quality=90, subsampling="420", restart_interval=1):
        check_params(quality, subsampling, restart_interval, "MJPEGWriter")
        if isinstance(fps, bool) or not isinstance(fps, (int, float, Fraction)) or not 0 < fps < float("inf"):
            raise ValueError(f"MJPEGWriter: fps must be a positive finite number, got {fps!r}")
        rate = Fraction(fps).limit_denominator(65535)
        if rate <= 0 or rate.numerator >= 1 << 32:
            raise ValueError(f"MJPEGWriter: fps {fps!r} has no dwRate / dwScale")
        self.path, self.rate, self.quality, self.subsampling, self.restart_interval = path, rate, quality, subsampling, restart_interval
        self.size = None                        # (H, W) of the first frame
        self._index = []                        # (offset from the 'movi' fourcc, bytes) per frame
        self._pos = _MOVI_FOURCC + 4            # file position == bytes so far
        self._fh = open(path, "wb")
        self._fh.write(b"\0" * self._pos)       # the headers are written by close(), when the counts are known

    @property
    def frames(self):
        return len(self._index)

    def _final_bytes(self, pos, n):
        return pos + 8 + 16 * n

    def write(self, frames):
        if self._fh is None:
            raise ValueError("MJPEGWriter.write: the file is closed")
        check_frames(frames, "MJPEGWriter.write")
        H, W = frames.shape[-3:-1]
        if self.size is not None and self.size != (H, W):
            raise ValueError(f"MJPEGWriter: all frames of a file have one size; the file holds {self.size[0]} x {self.size[1]}, got {H} x {W}")
        check_device(frames, "MJPEGWriter.write")
        src = frames.reshape(-1, H, W, 3)
        chunks = []
        for i in range(0, src.shape[0], self.BATCH):
            chunks += jpeg_bytes(src[i:i + self.BATCH], self.quality, self.subsampling, self.restart_interval)
        return self.write_jpegs(chunks, H, W)

    def write_jpegs(self, chunks, height, width):
        """Frames that are JPEG streams already (a list of bytes, each of a height x width frame; what `jpeg_bytes` returns), as `write` appends them."""
        if self._fh is None:
            raise ValueError("MJPEGWriter.write_jpegs: the file is closed")
        H, W = int(height), int(width)
        if not 1 <= H <= 65535 or not 1 <= W <= 65535 or any(not isinstance(c, (bytes, bytearray)) or c[:2] != b"\xff\xd8" or c[-2:] != b"\xff\xd9" for c in chunks):
            raise ValueError("MJPEGWriter.write_jpegs: expected JPEG streams (SOI .. EOI) of one height x width in 1..65535")
        if self.size is not None and self.size != (H, W):
            raise ValueError(f"MJPEGWriter: all frames of a file have one size; the file holds {self.size[0]} x {self.size[1]}, got {H} x {W}")
        pos = self._pos + sum(8 + len(c) + (len(c) & 1) for c in chunks)
        if self._final_bytes(pos, len(self._index) + len(chunks)) > self.MAX_FILE_BYTES:
            raise ValueError(f"MJPEGWriter: {len(chunks)} more frames would take {self.path} past {self.MAX_FILE_BYTES} bytes (AVI 1.0, no OpenDML); "
                             f"the file keeps its {len(self._index)} frames")
        self.size = (H, W)
        for c in chunks:
            self._index.append((self._pos - _MOVI_FOURCC, len(c)))
            self._fh.write(b"00dc" + struct.pack("<I", len(c)) + bytes(c) + b"\0" * (len(c) & 1))
            self._pos += 8 + len(c) + (len(c) & 1)
        return len(chunks)

    def close(self):
        if self._fh is None:
            return
        fh, self._fh = self._fh, None
        n, (H, W) = len(self._index), self.size or (0, 0)
        largest = max((s for _, s in self._index), default=0)
        fh.write(b"idx1" + struct.pack("<I", 16 * n) + b"".join(b"00dc" + struct.pack("<III", AVIIF_KEYFRAME, o, s) for o, s in self._index))
        total = self._final_bytes(self._pos, n)
        rate, scale = self.rate.numerator, self.rate.denominator
        avih = struct.pack("<14I", round(1e6 * scale / rate), min(int(largest * rate / scale) + 1, 0xffffffff) if n else 0, 0, AVIF_HASINDEX, n, 0, 1, largest, W, H,
                           0, 0, 0, 0)
        strh = b"vidsMJPG" + struct.pack("<IHHIIIIIIIIhhhh", 0, 0, 0, 0, scale, rate, 0, n, largest, 0xffffffff, 0, 0, 0, min(W, 32767),
                                        min(H, 32767))
        strf = struct.pack("<IiiHH4sIiiII", 40, W, H, 1, 24, b"MJPG", min(3 * W * H, 0xffffffff), 0, 0, 0, 0)
        strl = b"LIST" + struct.pack("<I", 4 + 8 + len(strh) + 8 + len(strf)) + b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + \
            struct.pack("<I", len(strf)) + strf
        hdrl = b"LIST" + struct.pack("<I", 4 + 8 + len(avih) + len(strl)) + b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + strl
        head = b"RIFF" + struct.pack("<I", total - 8) + b"AVI " + hdrl + b"LIST" + struct.pack("<I", self._pos - _MOVI_FOURCC) + b"movi"
        assert len(head) == _MOVI_FOURCC + 4
        fh.seek(0)
        fh.write(head)
        fh.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def write_mjpeg_avi(path, frames, fps, quality=90, subsampling="420", restart_interval=1):
    """All frames of one tensor as one Motion-JPEG AVI file; returns the path."""
    check_frames(frames, "write_mjpeg_avi")
    check_device(frames, "write_mjpeg_avi")
    with MJPEGWriter(path, fps, quality, subsampling, restart_interval) as w:
        w.write(frames)
    return path


def export_to_video(video_frames, output_video_path, fps=8, quality=90):
    """video_io.export_to_video: see there."""
    ext = os.path.splitext(str(output_video_path))[1].lower()
    if ext != ".avi":
        raise ValueError(f"export_to_video: {output_video_path!r}: only the Motion-JPEG .avi format is written (no {ext or 'suffix-less'} encoder here)")
    check_frames(video_frames, "export_to_video")
    if video_frames.dim() == 5 and video_frames.shape[0] != 1:
        raise ValueError(f"export_to_video: one video per file, got a batch of {video_frames.shape[0]}; pass video[i]")
    check_device(video_frames, "export_to_video")
    return write_mjpeg_avi(output_video_path, video_frames, fps, quality)
