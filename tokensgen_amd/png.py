"""The byte output as lossless files: a PNG encoder on the GPU (tg_png_filter, tg_png_band_plan, tg_png_write, csrc/png.hip, csrc/png_deflate.h); DESIGN.md §8n.  No
reference code: the header's comment is the definition, tests/png_ref.py restates it and decodes the files again.

    from tokensgen_amd.png import encode_png, png_bytes, save_png, save_png_sequence, png_geometry

`encode_png` turns uint8 frames on the device into one device buffer that holds every frame's PNG file and the host offsets that cut it, the conventions of
jpeg.encode_jpeg.  Row filters, run-length tokens and one Huffman block per band of rows, all in integers: a frame is one exact byte string, the same alone and in a
batch, and any PNG reader returns the frame's bytes exactly.  The sizing pass and the writing pass are separated by the one host read of an encode, the total size.

uint8 RGB frames only ("uint8" of video_io.VideoProcessor; the contract: frames.py).  Every refusal comes before any kernel call.  There is no CPU path.  Not here: APNG, reading PNG, 16-bit,
palette, alpha and grey images, LZ77 matches beyond distance 1."""
import os
from typing import NamedTuple

import torch

from . import kernels as K
from .frames import check_device, check_frames, is_int, single_frame, split_bytes

FILTERS = tuple(K.PNG_FILTERS)
MAX_BAND_BYTES = 65535
MAX_WIDTH = 21844                               # a filtered row, 1 + 3 W bytes, fits one band
MAX_HEIGHT = 65535
DEFAULT_ROWS_PER_BLOCK = 16
FILE_HEADER_BYTES, FILE_TRAILER_BYTES = 33, 12  # signature and IHDR; IEND


class PngGeometry(NamedTuple):
    """rows_per_block: the rows of a band (the default resolved); bands of a frame; bytes of a filtered row (1 + 3 W) and of a full band; max_file_bytes: what no file of
    such a frame exceeds (every band stored)."""
    rows_per_block: int
    bands: int
    row_bytes: int
    band_bytes: int
    max_file_bytes: int


def png_geometry(H, W, rows_per_block=None):
    """How an H x W frame is cut into bands; pure Python, no device.  rows_per_block None: min(DEFAULT_ROWS_PER_BLOCK, what fits MAX_BAND_BYTES)."""
    if not is_int(H) or not is_int(W) or not 1 <= H <= MAX_HEIGHT or W < 1:
        raise ValueError(f"png: a frame is 1..{MAX_HEIGHT} rows of at least one pixel, got {H!r} x {W!r}")
    if W > MAX_WIDTH:
        raise ValueError(f"png: a row of {W} pixels is {1 + 3 * W} filtered bytes; a band is at most {MAX_BAND_BYTES} bytes, so W <= {MAX_WIDTH}")
    row = 1 + 3 * W
    if rows_per_block is None:
        rows_per_block = min(DEFAULT_ROWS_PER_BLOCK, MAX_BAND_BYTES // row)
    if not is_int(rows_per_block) or rows_per_block < 1 or rows_per_block * row > MAX_BAND_BYTES:
        raise ValueError(f"png: rows_per_block must be an integer in 1..{MAX_BAND_BYTES // row} for W = {W} (a band is at most {MAX_BAND_BYTES} bytes), "
                         f"got {rows_per_block!r}")
    bands = -(-H // rows_per_block)
    return PngGeometry(rows_per_block, bands, row, rows_per_block * row, FILE_HEADER_BYTES + FILE_TRAILER_BYTES + 8 + bands * 17 + H * row)


def check_params(filter, who):
    if filter not in FILTERS:
        raise ValueError(f"{who}: filter must be one of {FILTERS}, got {filter!r}")


def band_offsets(band_bytes):
    """The prefix sums between the sizing pass and the writing pass, on the device: band_bytes int32 [F, bands] -> (where every band's chunk starts in the buffer, int64
    [F, bands]; where every frame ends, int64 [F])."""
    ends = torch.cumsum(band_bytes, 1, dtype=torch.int64)
    totals = ends[:, -1] + (FILE_HEADER_BYTES + FILE_TRAILER_BYTES)
    frame_ends = torch.cumsum(totals, 0)
    return ((frame_ends - totals + FILE_HEADER_BYTES)[:, None] + (ends - band_bytes)).contiguous(), frame_ends


def encode_png(frames, filter="adaptive", rows_per_block=None):
    """uint8 [F, H, W, 3] (or [B, T, H, W, 3], frames in order) on the device -> (data, offsets): data a uint8 device tensor of exactly offsets[-1] bytes, offsets int64
    [F + 1] on the host; frame f is data[offsets[f]:offsets[f + 1]], a complete PNG file.  filter: "adaptive" (per row the type with the smallest sum of
    min(v, 256 - v)) or one of "none", "sub", "up", "average", "paeth"; rows_per_block: the rows of a band, the unit of parallel work and of one Huffman block
    (png_geometry).  A view that is not contiguous is copied first."""
    check_frames(frames, "encode_png")
    check_params(filter, "encode_png")
    H, W = frames.shape[-3:-1]
    R = png_geometry(H, W, rows_per_block).rows_per_block
    check_device(frames, "encode_png")
    src = frames.contiguous().reshape(-1, H, W, 3)
    filtered = K.png_filter(src, filter, R)
    plans, sizes = K.png_band_plan(filtered, H, W, R)
    offs, frame_ends = band_offsets(sizes)
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), frame_ends.cpu()])  # the one wait of the call
    data = torch.empty(int(offsets[-1]), dtype=torch.uint8, device=frames.device)
    K.png_write(filtered, plans, H, W, R, offs, data)
    return data, offsets


def png_bytes(frames, filter="adaptive", rows_per_block=None):
    """encode_png, copied to the host and cut: a list of one `bytes` per frame."""
    return split_bytes(*encode_png(frames, filter, rows_per_block))


def save_png(frame, path, filter="adaptive", rows_per_block=None):
    """One frame, uint8 [H, W, 3] (or [1, H, W, 3]) on the device, as a .png file; returns the path."""
    check_frames(frame, "save_png", dims=(3, 4))
    one = single_frame(frame, "save_png")
    check_params(filter, "save_png")
    png_geometry(frame.shape[-3], frame.shape[-2], rows_per_block)
    check_device(frame, "save_png")
    (b,) = png_bytes(one, filter, rows_per_block)
    with open(path, "wb") as fh:
        fh.write(b)
    return path


def sequence_paths(pattern, n, start=0):
    """pattern.format(start), ..., pattern.format(start + n - 1); refused where the pattern does not give n different names"""
    if not isinstance(pattern, (str, os.PathLike)) or not is_int(start) or start < 0:
        raise ValueError(f"save_png_sequence: pattern must be a path with one number field such as 'frame_{{:05d}}.png' and start an integer >= 0, got {pattern!r}, {start!r}")
    try:
        paths = [os.fspath(pattern).format(start + i) for i in range(n)]
    except (IndexError, KeyError, ValueError) as e:
        raise ValueError(f"save_png_sequence: pattern {pattern!r} must have exactly one positional number field such as '{{:05d}}' ({e})") from None
    if len(set(paths)) != n:
        raise ValueError(f"save_png_sequence: pattern {pattern!r} gives the same name for different frames; it needs a number field such as '{{:05d}}'")
    return paths


def save_png_sequence(frames, pattern, start=0, filter="adaptive", rows_per_block=None):
    """uint8 [F, H, W, 3] or [B, T, H, W, 3] on the device as numbered files: frame i goes to pattern.format(start + i), e.g. "out/frame_{:05d}.png".  One encode and
    one device-to-host copy for the whole clip; the directory must exist.  Returns the paths."""
    check_frames(frames, "save_png_sequence")
    check_params(filter, "save_png_sequence")
    png_geometry(frames.shape[-3], frames.shape[-2], rows_per_block)
    paths = sequence_paths(pattern, frames.numel() // (3 * frames.shape[-3] * frames.shape[-2]), start)
    check_device(frames, "save_png_sequence")
    for path, b in zip(paths, png_bytes(frames, filter, rows_per_block)):
        with open(path, "wb") as fh:
            fh.write(b)
    return paths
