"""The baseline-JPEG decoding definition of include/tokensgen_hip.h restated in numpy, with a plain loop for the entropy decoder: the yardstick of
csrc/jpeg_decode.hip.  It has its own small header reader (valid, accepted streams only: it asserts, it does not diagnose), so that tokensgen_amd.jpeg.parse_jpeg is
checked against something it did not write.  `decode` returns the quantised coefficients and the picture; `wrong` switches on one deliberately wrong rule so that a
test can show that the rule matters."""
import functools
import re
import struct
from collections import namedtuple

import numpy as np

from jpeg_ref import AC_BITS, AC_VALS, DC_BITS, DC_VALS, DCT_A, ZIGZAG, geometry

Decoded = namedtuple("Decoded", "coef rgb")
Header = namedtuple("Header", "height width sub ri scan q huff")     # q: three int64 [64] in natural order; huff: three ((BITS, VALS) DC, (BITS, VALS) AC)
STD = {0x00: (bytes(DC_BITS[0]), bytes(DC_VALS)), 0x01: (bytes(DC_BITS[1]), bytes(DC_VALS)), 0x10: (bytes(AC_BITS[0]), bytes(AC_VALS[0])),
       0x11: (bytes(AC_BITS[1]), bytes(AC_VALS[1]))}
_MARKER = re.compile(rb"\xff[^\x00\xff]")


def parse(data):
    assert data[:2] == b"\xff\xd8"
    pos, qt, ht, ri, sof = 2, {}, {}, 0, None
    while True:
        assert data[pos] == 0xff
        while data[pos] == 0xff:
            pos += 1
        m = data[pos]
        pos += 1
        ln = struct.unpack_from(">H", data, pos)[0]
        seg = data[pos + 2:pos + ln]
        if m == 0xdb:
            for p in range(0, len(seg), 65):
                assert seg[p] >> 4 == 0
                q = np.zeros(64, np.int64)
                q[ZIGZAG] = np.frombuffer(seg[p + 1:p + 65], np.uint8)
                qt[seg[p] & 15] = q
        elif m == 0xc4:
            p = 0
            while p < len(seg):
                n = sum(seg[p + 1:p + 17])
                ht[seg[p]] = (bytes(seg[p + 1:p + 17]), bytes(seg[p + 17:p + 17 + n]))
                p += 17 + n
        elif m == 0xdd:
            ri = struct.unpack(">H", seg)[0]
        elif m == 0xc0:
            prec, h, w, nc = struct.unpack_from(">BHHB", seg, 0)
            assert prec == 8 and nc == 3
            comps = [(seg[6 + 3 * i], seg[7 + 3 * i], seg[8 + 3 * i]) for i in range(3)]
            sub = {(0x22, 0x11, 0x11): "420", (0x11, 0x11, 0x11): "444"}[tuple(c[1] for c in comps)]
            sof = (h, w, sub, comps)
        elif m == 0xda:
            assert seg[0] == 3 and tuple(seg[7:10]) == (0, 63, 0)
            h, w, sub, comps = sof
            tables = ht or STD
            huff = tuple((tables[seg[2 + 2 * i] >> 4], tables[0x10 | (seg[2 + 2 * i] & 15)]) for i in range(3))
            begin = pos + ln
            end = begin
            while True:                                                         # the first marker that is no restart marker ends the scan
                hit = _MARKER.search(data, end)
                assert hit is not None, "no EOI"
                end = hit.start()
                if not 0xd0 <= data[end + 1] <= 0xd7:
                    break
                end += 2
            assert data[end + 1] == 0xd9
            return Header(h, w, sub, ri, (begin, end), tuple(qt[c[2]] for c in comps), huff)
        else:
            assert m >= 0xe0 or m == 0xfe, f"marker FF {m:02X}"
        pos += ln


@functools.lru_cache(maxsize=64)
def lookup(bits, vals):
    """Annex C: the next 16 bits -> length << 8 | symbol (0: no code), as a list"""
    lut = np.zeros(65536, np.int64)
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            lut[code << (16 - length):(code + 1) << (16 - length)] = (length << 8) | vals[k]
            code += 1
            k += 1
        code <<= 1
    return lut.tolist()


def segment_ranges(data, hdr=None):
    """(begins, ends) of the restart segments' entropy data in the frame's bytes, markers excluded; and the marker bytes between them"""
    hdr = hdr or parse(data)
    b, e = hdr.scan
    begins, ends, markers = [b], [], []
    for hit in re.finditer(rb"\xff[\xd0-\xd7]", data[b:e]):
        ends.append(b + hit.start())
        begins.append(b + hit.start() + 2)
        markers.append(data[b + hit.start() + 1])
    ends.append(e)
    return begins, ends, markers


ST_INVALID_CODE, ST_COEF_INDEX, ST_CATEGORY, ST_OUT_OF_BITS, ST_RST_COUNT, ST_RST_NUMBER, ST_RANGE = 1, 2, 4, 8, 16, 32, 64


def device_segments(data, begin, end, n_seg):
    """tg_jpeg_find_segments restated for any bytes, damaged ones included: every FF D0 .. D7 pair of data[begin:end] is a marker; marker k ends segment k and segment
    k + 1 starts behind it; entries the stream has no marker for are the empty range at `end`; markers past n_seg - 1 are counted, not stored.
    -> (begins, ends, status bits)"""
    begins, ends, status, found = [begin] + [end] * (n_seg - 1), [end] * n_seg, 0, 0
    for hit in re.finditer(rb"\xff[\xd0-\xd7]", data[begin:end]):
        p = begin + hit.start()
        if found < n_seg - 1:
            ends[found], begins[found + 1] = p, p + 2
            if data[p + 1] & 7 != found & 7:
                status |= ST_RST_NUMBER
        found += 1
    if found != n_seg - 1:
        status |= ST_RST_COUNT
    return begins, ends, status


def damaged_streams():
    """Three damaged 33 x 47 frames for the decoder's error paths: name -> (the damaged bytes, the status bits the decoder reports for it, the restart interval of
    the stream).  tests/test_jpeg_decode_cpu.py runs their segments through the host program under the sanitizers and holds the bits to what it reports; the GPU test
    decodes them between two sound frames."""
    from jpeg_ref import encode, sample_image
    a = sample_image(33, 47)
    s3, s0 = encode(a, 90, "420", 3), encode(a, 90, "420", 65535)
    b3, e3 = parse(s3).scan
    b0, _ = parse(s0).scan
    flipped = bytearray(s0)
    flipped[b0 + FLIP[0]] = FLIP[1]
    first = s3.index(b"\xff\xd0", b3)
    return {"cut": (s3[:b3 + (e3 - b3) // 2], ST_OUT_OF_BITS | ST_RST_COUNT, 3),
            "flipped": (bytes(flipped), ST_INVALID_CODE, 65535),
            "no_marker": (s3[:first] + s3[first + 2:], ST_OUT_OF_BITS | ST_RST_COUNT | ST_RST_NUMBER, 3)}


FLIP = (5, 0x7f)        # byte 5 of the scan of sample_image(33, 47) at quality 90, 4:2:0, no markers, set to 7F: the decoder meets a run of ones that is no code


def _windows(raw):
    """the 16 bits from every bit position of the un-stuffed bytes, zeros past the end"""
    bits = np.concatenate([np.unpackbits(np.frombuffer(raw, np.uint8)), np.zeros(32, np.uint8)]).astype(np.int64)
    n = len(bits) - 15
    w = np.zeros(n, np.int64)
    for j in range(16):
        w += bits[j:j + n] << (15 - j)
    return w.tolist()


def decode_segment(raw, luts, bpm, n_mcus, pred, out):
    """raw: a segment's bytes; luts: per component (DC, AC) lookups; pred: the three running DC values (changed in place); out [n_mcus, bpm, 64]"""
    w = _windows(raw.replace(b"\xff\x00", b"\xff"))
    pos = 0
    for m in range(n_mcus):
        for k in range(bpm):
            comp = 0 if k < bpm - 2 else k - (bpm - 3)
            dc, ac = luts[comp]
            e = dc[w[pos]]
            assert e, "invalid code"
            pos += e >> 8
            s = e & 255
            assert s <= 11
            if s:
                v = w[pos] >> (16 - s)
                pos += s
                pred[comp] += v if v >= 1 << (s - 1) else v - (1 << s) + 1
            out[m, k, 0] = min(max(pred[comp], -32768), 32767)
            i = 1
            while i < 64:
                e = ac[w[pos]]
                assert e, "invalid code"
                pos += e >> 8
                r, s = (e & 255) >> 4, e & 15
                if s == 0:
                    if r == 0:
                        break
                    assert r == 15, "invalid code"
                    i += 16
                    assert i <= 64
                    continue
                assert s <= 10
                i += r
                assert i <= 63
                v = w[pos] >> (16 - s)
                pos += s
                out[m, k, i] = v if v >= 1 << (s - 1) else v - (1 << s) + 1
                i += 1
    assert pos <= 8 * len(raw.replace(b"\xff\x00", b"\xff")), "out of bits"


def coefficients(data, hdr=None, wrong=None):
    """the quantised coefficients in zigzag order, int64 [MCUs, blocks per MCU, 64]"""
    hdr = hdr or parse(data)
    _, bpm, rows, cols = geometry(hdr.height, hdr.width, hdr.sub)
    total = rows * cols
    r = hdr.ri or total
    begins, ends, markers = segment_ranges(data, hdr)
    assert len(begins) == -(-total // r) and markers == [0xd0 + (k & 7) for k in range(len(markers))]
    luts = [(lookup(*dc), lookup(*ac)) for dc, ac in hdr.huff]
    out = np.zeros((total, bpm, 64), np.int64)
    pred = [0, 0, 0]
    for s, (b, e) in enumerate(zip(begins, ends)):
        if wrong != "no_dc_reset":
            pred = [0, 0, 0]
        decode_segment(data[b:e], luts, bpm, min((s + 1) * r, total) - s * r, pred, out[s * r:])
    return out


def idct(coef, q):
    """coef int64 [.., 64] in zigzag order, q [64] natural -> samples [.., 8 (y), 8 (x)]"""
    nat = np.zeros_like(coef)
    nat[..., ZIGZAG] = coef
    d = np.clip(nat * q, -2048, 2047).reshape(coef.shape[:-1] + (8, 8))         # [v][u]
    t = (np.einsum("ux,...vu->...vx", DCT_A, d) + 512) >> 10
    p = (np.einsum("vy,...vx->...yx", DCT_A, t) + 32768) >> 16
    return np.clip(p + 128, 0, 255)


def upsample(c, wrong=None):
    """libjpeg's triangle filter, 2 x in both directions, the plane's edges repeated"""
    if wrong == "box":
        return np.repeat(np.repeat(c, 2, 0), 2, 1)
    p = np.pad(c, 1, mode="edge")
    s = np.empty((2 * c.shape[0], c.shape[1] + 2), np.int64)
    s[0::2] = 3 * p[1:-1] + p[:-2]                                              # even rows: the row above is the far one
    s[1::2] = 3 * p[1:-1] + p[2:]
    out = np.empty((2 * c.shape[0], 2 * c.shape[1]), np.int64)
    out[:, 0::2] = (3 * s[:, 1:-1] + s[:, :-2] + 8) >> 4
    out[:, 1::2] = (3 * s[:, 1:-1] + s[:, 2:] + 7) >> 4
    return out


def reconstruct(coef, hdr, wrong=None):
    """coefficients -> uint8 [H, W, 3]"""
    h, w, sub = hdr.height, hdr.width, hdr.sub
    _, bpm, rows, cols = geometry(h, w, sub)
    c = coef.reshape(rows, cols, bpm, 64)
    if sub == "420":
        y = idct(c[:, :, :4], hdr.q[0]).reshape(rows, cols, 2, 2, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(rows * 16, cols * 16)
    else:
        y = idct(c[:, :, 0], hdr.q[0]).transpose(0, 2, 1, 3).reshape(rows * 8, cols * 8)
    cb, cr = (idct(c[:, :, bpm - 3 + i], hdr.q[i]).transpose(0, 2, 1, 3).reshape(rows * 8, cols * 8) for i in (1, 2))
    if sub == "420":
        if wrong != "padded":
            cb, cr = (p[:(h + 1) // 2, :(w + 1) // 2] for p in (cb, cr))          # the real chroma plane
        cb, cr = upsample(cb, wrong), upsample(cr, wrong)
    y, cb, cr = y[:h, :w], cb[:h, :w] - 128, cr[:h, :w] - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def decode(data, wrong=None):
    """one frame's bytes -> Decoded(coef int64 [MCUs, blocks per MCU, 64], rgb uint8 [H, W, 3]).  wrong: None, "no_dc_reset" (the DC predictor carried over a restart
    marker), "box" (chroma repeated instead of the triangle filter) or "padded" (the filter run on the MCU-padded chroma plane)."""
    if wrong is None:
        return _decode_cached(bytes(data))
    hdr = parse(data)
    return Decoded(*(lambda c: (c, reconstruct(c, hdr, wrong)))(coefficients(data, hdr, wrong)))


@functools.lru_cache(maxsize=1024)
def _decode_cached(data):
    hdr = parse(data)
    coef = coefficients(data, hdr)
    rgb = reconstruct(coef, hdr)
    coef.setflags(write=False)
    rgb.setflags(write=False)
    return Decoded(coef, rgb)
