"""The byte output as lossless files: a PNG encoder on the GPU (tg_png_filter, tg_png_band_plan, tg_png_write, csrc/png.hip, csrc/png_deflate.h); DESIGN.md §8n.  No
reference code: the header's comment is the definition, tests/png_ref.py restates it and decodes the files again.

    from tokensgen_amd.png import encode_png, png_bytes, save_png, save_png_sequence, png_geometry

`encode_png` turns uint8 frames on the device into one device buffer that holds every frame's PNG file and the host offsets that cut it, the conventions of
jpeg.encode_jpeg.  Row filters, run-length tokens and one Huffman block per band of rows, all in integers: a frame is one exact byte string, the same alone and in a
batch, and any PNG reader returns the frame's bytes exactly.  The sizing pass and the writing pass are separated by the one host read of an encode, the total size.

uint8 RGB frames only ("uint8" of video_io.VideoProcessor; the contract: frames.py).  Every refusal comes before any kernel call.  There is no CPU path.  Not here: APNG, 16-bit,
palette, alpha and grey images, LZ77 matches beyond distance 1.

Reading (tg_png_inflate, tg_png_unfilter, csrc/png_decode.hip, csrc/png_inflate.h; tests/png_dec_ref.py restates it): `decode_png`, `load_png`,
`load_png_sequence`, `PNGSequenceReader`, with `parse_png` and `inflate_plan` on the host.  8-bit RGB and RGBA files of any writer, exact; the alpha is dropped."""
import os
import struct
import zlib
from fractions import Fraction
from typing import NamedTuple

import numpy as np
import torch

from . import kernels as K
from .frames import check_device, check_frames, gpu_device, is_int, single_frame, split_bytes

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


# ---- reading -----------------------------------------------------------------------------------------------------------------------------------------
SIGNATURE = b"\x89PNG\r\n\x1a\n"
INFLATE_MODES = ("auto", "chunk", "stream")
_SYNC_TAIL = b"\x00\x00\xff\xff"                # what an empty stored block ends with: where a payload ends so, a block ended with it and the next starts on a byte


class PngInfo(NamedTuple):
    """height, width; color_type 2 (RGB) or 6 (RGB and alpha), 8 bits a sample; idat: the payloads of the IDAT chunks in order: together the frame's zlib stream"""
    height: int
    width: int
    color_type: int
    idat: tuple


class PngDecodeError(ValueError):
    """What decode_png raises when the device reports a damaged stream: `frames` holds the decoded batch (a damaged frame is zeros, or, with a filter type above 4
    alone, decoded with that row read as unfiltered), `status` the int32 [F] bits of include/tokensgen_hip.h on the host."""
    frames = None
    status = None


def _status_text(bits):
    return "; ".join(text for bit, text in K.PNG_STATUS.items() if bits & bit) or f"status {bits}"


def _stream_ends(idat):
    """the first two and the last four bytes of the joined payloads (at least six bytes in all), without joining them: an IDAT may be a single byte or empty"""
    head, tail = b"", b""
    for p in idat:
        head += p[:2 - len(head)]
        if len(head) == 2:
            break
    for p in reversed(idat):
        tail = p[max(0, len(p) - (4 - len(tail))):] + tail
        if len(tail) == 4:
            break
    return head, tail


def parse_png(data, index=0):
    """The container of one file, on the host -> PngInfo.  Checks the signature, IHDR, every chunk's CRC-32, that the IDATs are consecutive and IEND ends the file, and
    the zlib header (method 8, a window of at most 32 KiB, no preset dictionary, the check bits).  Ancillary chunks are skipped.  NotImplementedError, by name, for what
    is a PNG file but not read here: interlace, 16-bit and sub-byte depths, palette, grey and grey-alpha, an unknown critical chunk.  ValueError naming the frame and
    the condition for a damaged container.  No pixel is touched."""
    who = f"parse_png: frame {index}"
    d = bytes(data)
    bad = lambda what: ValueError(f"{who}: {what}")
    if d[:8] != SIGNATURE:
        raise bad("not a PNG file (the signature is missing)")
    pos, head, idat, seen_idat, closed, ended = 8, None, [], False, False, False
    while pos < len(d):
        if len(d) - pos < 12:
            raise bad(f"the file is truncated inside a chunk header at byte {pos}")
        n, kind = struct.unpack(">I4s", d[pos:pos + 8])
        if len(d) - pos < 12 + n:
            raise bad(f"the file is truncated inside the {kind!r} chunk at byte {pos}")
        body = d[pos + 8:pos + 8 + n]
        if zlib.crc32(d[pos + 4:pos + 8 + n]) != struct.unpack(">I", d[pos + 8 + n:pos + 12 + n])[0]:
            raise bad(f"the CRC-32 of the {kind!r} chunk at byte {pos} does not match")
        if head is None and kind != b"IHDR":
            raise bad("the first chunk is not IHDR")
        if kind == b"IHDR":
            if head is not None or n != 13:
                raise bad("a second IHDR, or one that is not 13 bytes")
            head = struct.unpack(">IIBBBBB", body)
            W, H, depth, ct, comp, filt, lace = head
            if W < 1 or H < 1 or W >= 1 << 31 or H >= 1 << 31 or ct not in (0, 2, 3, 4, 6) or comp != 0 or filt != 0 or lace > 1:
                raise bad(f"an IHDR that is no PNG header (W {W}, H {H}, colour type {ct}, compression {comp}, filter {filt}, interlace {lace})")
            if lace:
                raise NotImplementedError(f"{who}: an interlaced (Adam7) file; non-interlaced files only")
            if depth != 8:
                raise NotImplementedError(f"{who}: a bit depth of {depth}; 8 bits a sample only (no 16-bit and no sub-byte depths)")
            if ct not in (2, 6):
                raise NotImplementedError(f"{who}: colour type {ct} ({ {0: 'grey', 3: 'palette', 4: 'grey with alpha'}[ct]}); RGB (2) and RGB with alpha (6) only")
        elif kind == b"IDAT":
            if closed:
                raise bad("the IDAT chunks are not consecutive")
            seen_idat = True
            idat.append(body)
        elif kind == b"IEND":
            ended = True
            pos += 12 + n
            break
        else:
            if seen_idat:
                closed = True
            if not kind[0] & 0x20:
                raise NotImplementedError(f"{who}: the critical chunk {kind!r} is not known here")
        pos += 12 + n
    if head is None:
        raise bad("no IHDR")
    if not ended:
        raise bad("the file is truncated: no IEND")
    if pos != len(d):
        raise bad("bytes behind IEND")
    if not idat:
        raise bad("no IDAT chunk")
    if sum(map(len, idat)) < 6:
        raise bad("the zlib stream is shorter than its header and checksum")
    cmf, flg = _stream_ends(idat)[0]
    if cmf & 15 != 8 or cmf >> 4 > 7 or flg & 0x20 or (cmf << 8 | flg) % 31:
        raise bad(f"a zlib header that is not deflate with a window of at most 32 KiB and no preset dictionary ({cmf:02x} {flg:02x})")
    return PngInfo(head[1], head[0], head[3], tuple(idat))


def _whole_blocks(payload, first):
    """True where an IDAT payload (all but the last of a frame) ends on a block boundary that falls on a byte, as far as its bytes alone can say: it ends with an
    empty stored block (00 00 FF FF), or it is exactly one stored block (00, LEN, ~LEN, LEN bytes): the two forms of a band of encode_png"""
    if payload[-4:] == _SYNC_TAIL:
        return True
    body = payload[2:] if first else payload
    return len(body) >= 5 and body[0] == 0 and body[1] ^ body[3] == 0xff and body[2] ^ body[4] == 0xff and len(body) == 5 + (body[1] | body[2] << 8)


def _eligible(info):
    """the structural rule of the chunk route, and why not where not"""
    if len(info.idat) < 2:
        return "one IDAT chunk"
    if any(len(p) == 0 for p in info.idat):
        return "an empty IDAT chunk"
    if len(info.idat[0]) < 2 or len(info.idat[-1]) < 4:
        return "an IDAT boundary inside the zlib header or the checksum"
    if not all(_whole_blocks(p, k == 0) for k, p in enumerate(info.idat[:-1])):
        return "an IDAT chunk that neither ends with an empty stored block (00 00 FF FF) nor is one stored block"
    return None


def inflate_plan(pngs):
    """Which route decode_png(inflate="auto") takes for these files (a list of `bytes`, or of PngInfo), and why: ("chunk", reason) where every frame has at least two
    IDAT chunks, none empty, and every one but the last ends with 00 00 FF FF (a block boundary on a byte: what a sync or full flush per chunk leaves, and what
    encode_png writes behind a compressed band) or is exactly one stored block (encode_png's other band), so that every IDAT may be one independent piece; else ("stream", the first frame that is not and why).  A pure function: no device call.
    Whether the pieces are independent indeed (no distance across a boundary) only the decode can say; where they are not, decode_png falls back to "stream"."""
    infos = [p if isinstance(p, PngInfo) else parse_png(p, i) for i, p in enumerate(pngs)]
    if not infos:
        raise ValueError("inflate_plan: no frame")
    for i, info in enumerate(infos):
        why = _eligible(info)
        if why is not None:
            return "stream", f"frame {i}: {why}"
    return "chunk", f"every IDAT chunk of {len(infos)} frame{'s' if len(infos) != 1 else ''} ends on a block boundary"


def _streams_of(data, offsets, who):
    """-> list of bytes, the device the tensor form was on (or None)"""
    if isinstance(data, torch.Tensor):
        if data.dtype != torch.uint8 or data.dim() != 1:
            raise ValueError(f"{who}: a tensor of files is uint8 [n] with `offsets` as encode_png returns them, got {data.dtype} {tuple(data.shape)}")
        if offsets is None:
            raise ValueError(f"{who}: a tensor of files needs `offsets` (int64 [F + 1])")
        o = [int(v) for v in (offsets.tolist() if isinstance(offsets, torch.Tensor) else offsets)]
        if len(o) < 2 or o[0] < 0 or o[-1] > data.numel() or any(b <= a for a, b in zip(o, o[1:])):
            raise ValueError(f"{who}: offsets must rise from >= 0 to <= {data.numel()}, with at least one frame")
        host = data.cpu().numpy().tobytes()                                     # the containers are parsed on the host: one copy down
        return [host[a:b] for a, b in zip(o, o[1:])], (data.device if data.is_cuda else None)
    if offsets is not None:
        raise ValueError(f"{who}: `offsets` goes with a tensor of files, not with a list")
    if isinstance(data, (bytes, bytearray, memoryview)):
        data = [data]
    if not isinstance(data, (list, tuple)) or len(data) < 1 or any(not isinstance(c, (bytes, bytearray, memoryview)) for c in data):
        raise ValueError(f"{who}: expected a list of at least one `bytes`, or a uint8 tensor with offsets")
    return [bytes(c) for c in data], None


def decode_png(data, offsets=None, device=None, inflate="auto"):
    """PNG files -> uint8 [F, H, W, 3] on the device, exact; no pixel is touched on the host.  data: a list of `bytes` (one file each), or encode_png's (data, offsets)
    tensor form; a device tensor is copied to the host once, for the parsing.  All frames of a call share size and colour type (ValueError otherwise); the alpha of
    colour type 6 is dropped.  The containers are parsed here (parse_png), every frame's IDAT payloads go up joined, in one copy with the ranges behind them, and after
    the launches the host reads status [F]: the one wait of a decode.  A non-zero entry raises PngDecodeError (a ValueError) naming the first bad frame and the
    condition.
    inflate: "stream" decodes every frame's zlib stream serially, one wave per frame; "chunk" decodes every IDAT chunk as an independent piece, one wave each (a size
    pass, a prefix sum on the device, a writing pass), which needs the structure inflate_plan describes: forced on a file without it, a ValueError before any launch;
    "auto" (the default) is inflate_plan over the whole call.  The result is the same byte array either way.  Where the device finds that a piece was not independent
    after all (a distance across a chunk boundary, as a sync flush leaves; or any damage), the call is decoded again by "stream", and that run's frames, status and
    PngDecodeError are the result: a second wait, on that path only."""
    who = "decode_png"
    if inflate not in INFLATE_MODES:
        raise ValueError(f"{who}: inflate must be one of {INFLATE_MODES}, got {inflate!r}")
    files, on = _streams_of(data, offsets, who)
    infos = [parse_png(c, i) for i, c in enumerate(files)]
    first = infos[0]
    for i, info in enumerate(infos):
        if info[:3] != first[:3]:
            raise ValueError(f"{who}: all frames of a call share size and colour type; frame 0 is {first.height} x {first.width} colour type {first.color_type}, "
                             f"frame {i} is {info.height} x {info.width} colour type {info.color_type}")
    H, W, bpp, F = first.height, first.width, 3 if first.color_type == 2 else 4, len(infos)
    if H * (1 + bpp * W) >= 1 << 31 or 3 * H * W >= 1 << 31:
        raise ValueError(f"{who}: a frame of {H} x {W} is too large: its filtered bytes, H (1 + {bpp} W), stay below 2^31")
    route, why = inflate_plan(infos)
    if inflate == "chunk" and route != "chunk":
        raise ValueError(f"{who}: inflate=\"chunk\" needs files cut into independent pieces; {why}")
    if inflate != "auto":
        route = inflate
    dev = gpu_device(device if device is not None else on, who)
    # the streams joined, 16-byte aligned records behind them: the pieces of both routes (begin, end int64; frame, last int32), frame_first int32, expect (Adler-32)
    parts, begins, pos = [], [], 0
    for info in infos:
        begins.append(pos)
        for p in info.idat:
            parts.append(p)
            pos += len(p)
    total = pos

    def pieces_of(chunked):
        b, e, fr, last, ff = [], [], [], [], [0]
        for i, info in enumerate(infos):
            at = begins[i]
            size = sum(map(len, info.idat))
            if not chunked:
                b.append(at + 2), e.append(at + size - 4), fr.append(i), last.append(1)
            else:
                for k, p in enumerate(info.idat):
                    b.append(at + (2 if k == 0 else 0)), e.append(at + len(p) - (4 if k == len(info.idat) - 1 else 0)), fr.append(i), last.append(int(k == len(info.idat) - 1))
                    at += len(p)
            ff.append(len(b))
        return [np.array(b, np.int64), np.array(e, np.int64), np.array(fr, np.int32), np.array(last, np.int32), np.array(ff, np.int32)]

    expect = np.array([struct.unpack(">I", _stream_ends(info.idat)[1])[0] for info in infos], np.uint32).view(np.int32)
    meta = pieces_of(False) + (pieces_of(True) if route == "chunk" else []) + [expect]
    at = []
    for m in meta:
        pos += -pos % 16
        at.append(pos)
        pos += m.nbytes
    host = np.zeros(pos, np.uint8)
    host[:total] = np.frombuffer(b"".join(parts), np.uint8)
    for a, m in zip(at, meta):
        host[a:a + m.nbytes] = m.view(np.uint8)
    up = torch.from_numpy(host).to(dev)                                         # the one copy up
    cut = lambda i: up[at[i]:at[i] + meta[i].nbytes].view(torch.int64 if meta[i].dtype == np.int64 else torch.int32)
    streams = up[:total]
    frame_bytes = K.png_decode_geometry(H, W, bpp)[1]
    filtered = torch.empty(F, frame_bytes, dtype=torch.uint8, device=dev)
    if route == "chunk":
        status = torch.zeros(F, dtype=torch.int32, device=dev)
        pieces, ff = tuple(cut(i) for i in range(5, 9)), cut(9)
        sizes = K.png_inflate(streams, pieces, "chunk_size", filtered, H, W, bpp, status)
        ends = torch.cumsum(sizes, 0, dtype=torch.int64)                        # exclusive inside every frame: minus what the frames before end with
        ff64 = ff.to(torch.int64)
        before = torch.where(ff64[:-1] > 0, ends[(ff64[:-1] - 1).clamp(min=0)], torch.zeros_like(ff64[:-1]))
        piece_at = (ends - sizes - before[pieces[2].to(torch.int64)]).contiguous()
        adler3 = K.png_inflate(streams, pieces, "chunk_write", filtered, H, W, bpp, status, piece_at)
        out = K.png_unfilter(filtered, H, W, bpp, ff, adler3, cut(len(meta) - 1), status)
        if not bool(status.cpu().any()):                                        # the one wait of the call
            return out
        # a piece was not independent, or something is damaged: the serial decoder decides, and its status, frames and error text are the result
    status = torch.zeros(F, dtype=torch.int32, device=dev)
    pieces, ff = tuple(cut(i) for i in range(4)), cut(4)
    adler3 = K.png_inflate(streams, pieces, "stream", filtered, H, W, bpp, status)
    out = K.png_unfilter(filtered, H, W, bpp, ff, adler3, cut(len(meta) - 1), status)
    st = status.cpu()                                                           # the one wait of the call
    if bool(st.any()):
        f = int(torch.nonzero(st)[0])
        err = PngDecodeError(f"{who}: frame {f}: {_status_text(int(st[f]))}" + (f" ({int((st != 0).sum())} damaged frames in all)" if int((st != 0).sum()) > 1 else ""))
        err.frames, err.status = out, st
        raise err
    return out


def load_png(path, device=None):
    """One .png file -> uint8 [H, W, 3] on the device."""
    with open(path, "rb") as fh:
        return decode_png([fh.read()], device=device)[0]


def _existing(pattern, start, count, who):
    """the paths pattern.format(start), pattern.format(start + 1), ...: `count` of them, or while files exist"""
    if count is not None:
        if not is_int(count) or count < 1:
            raise ValueError(f"{who}: count must be a positive integer or None, got {count!r}")
        return sequence_paths(pattern, count, start)
    paths = []
    while True:
        (p,) = sequence_paths(pattern, 1, start + len(paths))
        if (paths and p == paths[-1]) or not os.path.exists(p):
            break
        paths.append(p)
    if not paths:
        raise FileNotFoundError(f"{who}: no file {sequence_paths(pattern, 1, start)[0]!r}: the sequence {pattern!r} is empty from {start}")
    return paths


def _read(path):
    with open(path, "rb") as fh:
        return fh.read()


def load_png_sequence(pattern, start=0, count=None, device=None):
    """Numbered files, the pattern save_png_sequence takes ("out/frame_{:05d}.png"), from number `start`: `count` files, or with None as many as exist in a row ->
    uint8 [F, H, W, 3] on the device, PNGSequenceReader.BATCH files per decode."""
    with PNGSequenceReader(pattern, start=start, device=device, count=count) as r:
        return r.read()


class PNGSequenceReader:
    """A directory of numbered PNG frames with the surface of jpeg.MJPEGReader: `.frames` / len(), `.size` (H, W), `.fps` (a Fraction: a sequence has no rate of its
    own, the caller gives it), `get_avg_fps()`; `get_batch(indices)` and `read(start=0, stop=None)` return uint8 [n, H, W, 3] on the device, decoded at most BATCH
    frames per decode_png call; an index may repeat and is decoded once.  The constructor lists the files and parses the first one's container, which says the size; the
    files are read when asked for.  A context manager (it holds no open file)."""

    BATCH = 64

    def __init__(self, pattern, fps=8, start=0, device=None, count=None):
        try:
            self.fps = Fraction(fps)
        except (TypeError, ValueError):
            raise ValueError(f"PNGSequenceReader: fps must be a positive number, got {fps!r}") from None
        if self.fps <= 0:
            raise ValueError(f"PNGSequenceReader: fps must be a positive number, got {fps!r}")
        self.pattern, self.device = pattern, device
        self.paths = _existing(pattern, start, count, "PNGSequenceReader")
        self.frames = len(self.paths)
        info = parse_png(_read(self.paths[0]), 0)
        self.size = (info.height, info.width)

    def __len__(self):
        return self.frames

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        pass

    def get_avg_fps(self):
        return float(self.fps)

    def frame_bytes(self, indices):
        return [_read(self.paths[i]) for i in indices]

    def get_batch(self, indices):
        """uint8 [len(indices), H, W, 3] on the device"""
        n, idx = len(self), []
        for i in indices:
            i = int(i)
            if not -n <= i < n:
                raise IndexError(f"PNGSequenceReader: frame {i} of {n}")
            idx.append(i % n)
        if not idx:
            raise ValueError("PNGSequenceReader.get_batch: no frame asked for")
        parts = []
        for s in range(0, len(idx), self.BATCH):
            piece = idx[s:s + self.BATCH]
            uniq = sorted(set(piece))                                           # a repeated index is decoded once
            try:
                dec = decode_png(self.frame_bytes(uniq), device=self.device)
            except PngDecodeError as e:
                bad = int(torch.nonzero(e.status)[0])
                raise ValueError(f"PNGSequenceReader: {self.paths[uniq[bad]]}: frame {uniq[bad]}: {_status_text(int(e.status[bad]))}") from None
            if uniq != piece:
                where = {u: k for k, u in enumerate(uniq)}
                dec = dec[torch.tensor([where[p] for p in piece], device=dec.device)]
            parts.append(dec)
        return parts[0] if len(parts) == 1 else torch.cat(parts)

    def read(self, start=0, stop=None):
        return self.get_batch(range(*slice(start, stop).indices(len(self))))
