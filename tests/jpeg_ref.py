"""The baseline-JPEG definition of include/tokensgen_hip.h restated in numpy, with plain loops for the entropy coder: the yardstick of
csrc/jpeg.hip.  `encode` returns one frame's exact bytes; `trace` (a dict) counts what the stream contains, `wrong` switches on one deliberately wrong rule so that a
test can show that the rule matters."""
import functools
import struct

import numpy as np

HEADER_BYTES = 629
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
# Annex K.1, natural order
Q_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                   18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
Q_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)
# Annex K.3: BITS and HUFFVAL of the DC and AC tables for luminance and chrominance
DC_BITS = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0])
DC_VALS = list(range(12))
AC_BITS = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77])
AC_VALS = (
    [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1,
     0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a,
     0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
     0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa],
    [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1,
     0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
     0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
     0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])


def canonical_codes(bits, vals):
    """Annex C: symbol -> (code, length)"""
    code, k, table = 0, 0, {}
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            table[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return table


HUFF = tuple((canonical_codes(DC_BITS[t], DC_VALS), canonical_codes(AC_BITS[t], AC_VALS[t])) for t in range(2))     # [luma | chroma] -> (DC, AC)

_u, _x = np.arange(8)[:, None], np.arange(8)[None, :]
DCT_A = np.rint(8192 * 0.5 * np.where(_u == 0, 1 / np.sqrt(2), 1.0) * np.cos((2 * _x + 1) * _u * np.pi / 16)).astype(np.int64)     # A[u][x]


def sample_image(h, w, seed=0):
    """smooth plus noise, uint8 [h, w, 3]"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.stack([127 + 100 * np.sin(xx / 7.0 + yy / 13.0 + seed), 127 + 100 * np.cos(xx / 11.0 - yy / 5.0), (xx * 3 + yy * 2 + 40 * seed) % 256], -1)
    return np.clip(a + rng.normal(0, 6, a.shape), 0, 255).astype(np.uint8)


def quant_table(base, quality):
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((base * s + 50) // 100, 1, 255)


def ycc(rgb):
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def fdct(p):
    """p int64 [.., 8 (y), 8 (x)], samples minus 128 -> coef [.., 8 (v), 8 (u)]"""
    t = (np.einsum("ux,...yx->...yu", DCT_A, p) + 512) >> 10
    return (np.einsum("vy,...yu->...vu", DCT_A, t) + 32768) >> 16


def quantise(c, q, truncate=False):
    """c [.., 8, 8], q [64] natural order; AC clamped to +-1023"""
    q = q.reshape(8, 8)
    a = np.abs(c) // q if truncate else (np.abs(c) + q // 2) // q
    dc = a[..., 0, 0].copy()
    a = np.minimum(a, 1023)
    a[..., 0, 0] = dc
    return np.sign(c) * a


def _blocks(p):
    h, w = p.shape
    return p.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)


def geometry(h, w, sub):
    """(MCU size, blocks per MCU, MCU rows, MCU columns)"""
    m = {"420": 16, "444": 8}[sub]
    return m, {"420": 6, "444": 3}[sub], -(-h // m), -(-w // m)


def coefficients(rgb, quality=90, sub="420", truncate=False):
    """uint8 [H, W, 3] -> int64 [MCUs, blocks per MCU, 64]: the quantised coefficients in zigzag order, MCUs in raster order (what tg_jpeg_coeffs produces)"""
    h, w, _ = rgb.shape
    m, bpm, rows, cols = geometry(h, w, sub)
    p = np.pad(rgb, ((0, rows * m - h), (0, cols * m - w), (0, 0)), mode="edge")
    y, cb, cr = ycc(p)
    if sub == "420":
        cb, cr = ((c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2 for c in (cb, cr))
    ql, qc = quant_table(Q_LUMA, quality), quant_table(Q_CHROMA, quality)
    by, bcb, bcr = (quantise(fdct(_blocks(c - 128)), q, truncate).reshape(c.shape[0] // 8, c.shape[1] // 8, 64)[..., ZIGZAG] for c, q in ((y, ql), (cb, qc), (cr, qc)))
    if sub == "420":
        by = by.reshape(rows, 2, cols, 2, 64).transpose(0, 2, 1, 3, 4).reshape(rows, cols, 4, 64)      # the four Y blocks of an MCU in raster order
    else:
        by = by[:, :, None]
    return np.concatenate([by, bcb[:, :, None], bcr[:, :, None]], 2).reshape(rows * cols, bpm, 64)


def header(h, w, quality, sub, ri):
    ql, qc = quant_table(Q_LUMA, quality), quant_table(Q_CHROMA, quality)
    o = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i, q in enumerate((ql, qc)):
        o += b"\xff\xdb\x00\x43" + bytes([i]) + bytes(q[ZIGZAG].astype(np.uint8))
    o += b"\xff\xc0\x00\x11\x08" + struct.pack(">HH", h, w) + bytes([3, 1, 0x22 if sub == "420" else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])
    for t in range(2):
        o += b"\xff\xc4" + struct.pack(">H", 19 + 12) + bytes([t]) + bytes(DC_BITS[t]) + bytes(DC_VALS)
        o += b"\xff\xc4" + struct.pack(">H", 19 + 162) + bytes([0x10 | t]) + bytes(AC_BITS[t]) + bytes(AC_VALS[t])
    o += b"\xff\xdd\x00\x04" + struct.pack(">H", ri)
    o += b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"
    assert len(o) == HEADER_BYTES
    return bytes(o)


class BitWriter:
    def __init__(self, stuffing=True):
        self.out, self.acc, self.n, self.stuffing, self.stuffed = bytearray(), 0, 0, stuffing, 0

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 255
            self.out.append(b)
            if b == 255:
                self.stuffed += 1
                if self.stuffing:
                    self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _category(v):
    n = int(abs(v)).bit_length()
    return n, (v if v >= 0 else v + (1 << n) - 1)


def encode_block(bw, z, pred, tables, trace):
    """z: 64 coefficients in zigzag order; returns the new DC predictor"""
    dc, ac = tables
    n, bits = _category(int(z[0]) - pred)
    bw.put(*dc[n])
    if n:
        bw.put(bits, n)
    run = 0
    for k in range(1, 64):
        v = int(z[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            bw.put(*ac[0xf0])
            trace["zrl"] = trace.get("zrl", 0) + 1
            run -= 16
        n, bits = _category(v)
        bw.put(*ac[(run << 4) | n])
        bw.put(bits, n)
        run = 0
    if run:
        bw.put(*ac[0])
        trace["eob"] = trace.get("eob", 0) + 1
    return int(z[0])


def entropy(coef, bpm, ri, trace=None, wrong=None):
    """coef [MCUs, bpm, 64] -> the scan and EOI; a list of the restart segments' lengths goes to trace["segments"]"""
    trace = {} if trace is None else trace
    bw, pred, total, lengths, start = BitWriter(stuffing=wrong != "no_stuffing"), [0, 0, 0], coef.shape[0], [], 0
    for m in range(total):
        for k in range(bpm):
            comp = 0 if k < bpm - 2 else k - (bpm - 3)
            pred[comp] = encode_block(bw, coef[m, k], pred[comp], HUFF[comp != 0], trace)
        if (m + 1) % ri == 0 and m + 1 < total:
            bw.flush()
            bw.out += bytes([0xff, 0xd0 + (((m + 1) // ri - 1) & 7)])
            if wrong != "no_dc_reset":
                pred = [0, 0, 0]
            lengths.append(len(bw.out) - start)
            start = len(bw.out)
    bw.flush()
    bw.out += b"\xff\xd9"
    lengths.append(len(bw.out) - start)
    trace["segments"], trace["stuffed"] = lengths, bw.stuffed
    return bytes(bw.out)


@functools.lru_cache(maxsize=256)
def _coefficients_cached(raw, shape, quality, sub):
    return coefficients(np.frombuffer(raw, np.uint8).reshape(shape), quality, sub)


def encode(rgb, quality=90, sub="420", ri=1, trace=None, wrong=None):
    """uint8 [H, W, 3] -> the frame's bytes.  wrong: None, "truncate" (a truncating quantiser), "no_dc_reset" (DC prediction carried over a marker) or "no_stuffing"."""
    rgb = np.ascontiguousarray(rgb)
    h, w, _ = rgb.shape
    coef = coefficients(rgb, quality, sub, True) if wrong == "truncate" else _coefficients_cached(rgb.tobytes(), rgb.shape, quality, sub)
    return header(h, w, quality, sub, ri) + entropy(coef, geometry(h, w, sub)[1], ri, trace, wrong)


def encode_many(frames, quality=90, sub="420", ri=1):
    """uint8 [F, H, W, 3] -> (all frames' bytes, offsets [F + 1]): what encode_jpeg returns"""
    parts = [encode(f, quality, sub, ri) for f in frames]
    return b"".join(parts), np.cumsum([0] + [len(p) for p in parts]).astype(np.int64)
