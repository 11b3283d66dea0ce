"""The PNG files of tokensgen_amd.png restated in numpy and plain Python, byte for byte (the definition is the comment of include/tokensgen_hip.h), and a
small PNG decoder (chunks and their CRCs, zlib.decompress, the five filters undone in numpy) so that no test needs an imaging library.

A file: signature, IHDR (8 bits, colour type 2, no interlace), one IDAT per band of `rows_per_block` rows, IEND.  A band's filtered bytes are cut into maximal runs, a
run becomes a literal and distance-1 matches (run_tokens), the band is one dynamic-Huffman block closed by an empty stored block, or one stored block where that is not
smaller.  Every open detail of the definition is decided here, once:
  * code lengths (build_lengths): the symbols that occur, sorted by (count, symbol) ascending, are the leaves of a Huffman tree built with two queues (of two equal
    weights the leaf is taken before the internal node); the leaves' depths are counted, depths above the limit are cut to the limit, and while the Kraft sum
    exceeds 1 (by k units of 2^-limit: k times) the step of zlib's gen_bitlen repays one unit: a leaf of the deepest level below the limit that has one becomes an
    internal node with two children, one leaf of the limit goes; then the sorted symbols receive the lengths from the longest to the shortest.  One symbol alone
    gets length 1.
  * the code-length sequence is the literal/length lengths up to the last used symbol followed by the one distance length, as ONE sequence; a run of r zeros is coded
    with 18 (up to 138 at a time) while r >= 11, then 17 if r >= 3, then single zeros; a run of r equal non-zero lengths is the length itself, then 16 (up to 6 at a
    time) while r >= 3 remain, then the length itself for what is left.
  * the zlib header is 78 01."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
FILTERS = ("none", "sub", "up", "average", "paeth")
MAX_BAND_BYTES = 65535
MAX_WIDTH = 21844
DEFAULT_ROWS = 16
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
ZLIB_HEADER = b"\x78\x01"
FINAL_BLOCK = b"\x03\x00"
SYNC_BLOCK = b"\x00\x00\xff\xff"


def geometry(H, W, rows_per_block=None):
    """(rows per band, bands, bytes of a filtered row, bytes of a full band)"""
    row = 1 + 3 * W
    if W > MAX_WIDTH:
        raise ValueError("a row does not fit one band")
    R = min(DEFAULT_ROWS, MAX_BAND_BYTES // row) if rows_per_block is None else rows_per_block
    if R < 1 or R * row > MAX_BAND_BYTES:
        raise ValueError("a band does not fit 65535 bytes")
    return R, -(-H // R), row, R * row


# ---- filtering -------------------------------------------------------------------------------------------------------------------------------------------------------

def filtered_rows(frame):
    """uint8 [H, W, 3] -> uint8 [5, H, 3 W]: every row under every filter type; the row above row 0 and the pixel left of pixel 0 are zeros"""
    H, W, _ = frame.shape
    x = frame.reshape(H, 3 * W).astype(np.int32)
    a = np.zeros_like(x)
    a[:, 3:] = x[:, :-3]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, 3:] = x[:-1, :-3]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    return np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]).astype(np.uint8)


def filter_costs(rows5):
    """[5, H, n] -> int64 [5, H]: the sum of min(v, 256 - v) over a filtered row"""
    v = rows5.astype(np.int64)
    return np.minimum(v, 256 - v).sum(-1)


def filter_frame(frame, filter="adaptive", tie="lowest"):
    """uint8 [H, W, 3] -> uint8 [H, 1 + 3 W]: the filter type and the filtered bytes of every row"""
    H = frame.shape[0]
    rows5 = filtered_rows(frame)
    if filter == "adaptive":
        cost = filter_costs(rows5)
        types = np.argmin(cost, 0) if tie == "lowest" else 4 - np.argmin(cost[::-1], 0)
    else:
        types = np.full(H, FILTERS.index(filter))
    out = np.empty((H, 1 + rows5.shape[2]), np.uint8)
    out[:, 0] = types
    out[:, 1:] = rows5[types, np.arange(H)]
    return out


# ---- tokens ----------------------------------------------------------------------------------------------------------------------------------------------------------

def runs(d):
    """the maximal runs of equal bytes: (values, lengths)"""
    d = np.asarray(d, np.uint8)
    starts = np.flatnonzero(np.concatenate([[True], d[1:] != d[:-1]]))
    return d[starts], np.diff(np.concatenate([starts, [len(d)]]))


def run_tokens(v, L, run_cap=258):
    """one run -> its tokens: ("lit", v) and ("match", length), all matches at distance 1"""
    out = [("lit", int(v))]
    rest = L - 1
    while rest >= run_cap:
        out.append(("match", run_cap))
        rest -= run_cap
    return out + ([("match", rest)] if rest >= 3 else [("lit", int(v))] * rest)


def tokens(d, run_cap=258):
    out = []
    for v, L in zip(*runs(d)):
        out += run_tokens(v, int(L), run_cap)
    return out


def length_symbol(n):
    """a match length 3 .. 258 -> (literal/length symbol, extra bits, their value)"""
    l = n - 3
    if l < 8:
        return 257 + l, 0, 0
    if l == 255:
        return 285, 0, 0
    eb = l.bit_length() - 3
    return 261 + 4 * eb + ((l >> eb) & 3), eb, l & ((1 << eb) - 1)


# ---- Huffman codes ---------------------------------------------------------------------------------------------------------------------------------------------------

def build_lengths(counts, max_len):
    n = len(counts)
    order = sorted((s for s in range(n) if counts[s] > 0), key=lambda s: (counts[s], s))
    m = len(order)
    lens = [0] * n
    if m == 0:
        return lens
    if m == 1:
        lens[order[0]] = 1
        return lens
    weight = [counts[s] for s in order] + [0] * (m - 1)
    parent = [0] * (2 * m - 1)
    leaf, node = 0, m
    for new in range(m, 2 * m - 1):
        for _ in range(2):
            if leaf < m and (node >= new or weight[leaf] <= weight[node]):
                pick, leaf = leaf, leaf + 1
            else:
                pick, node = node, node + 1
            parent[pick] = new
            weight[new] += weight[pick]
    depth = [0] * (2 * m - 1)
    for i in range(2 * m - 3, -1, -1):
        depth[i] = depth[parent[i]] + 1
    bl = [0] * (max_len + 1)
    for i in range(m):
        bl[min(depth[i], max_len)] += 1
    excess = sum(bl[b] << (max_len - b) for b in range(1, max_len + 1)) - (1 << max_len)      # the Kraft sum over 1, in units of 2^-max_len
    for _ in range(excess):
        bits = max_len - 1
        while bl[bits] == 0:
            bits -= 1
        bl[bits] -= 1
        bl[bits + 1] += 2
        bl[max_len] -= 1
    i = 0
    for bits in range(max_len, 0, -1):
        for _ in range(bl[bits]):
            lens[order[i]] = bits
            i += 1
    return lens


def canonical_codes(lens, max_len):
    """RFC 1951 3.2.2, each code bit-reversed: the stream takes Huffman codes from their most significant bit"""
    bl = [0] * (max_len + 2)
    for l in lens:
        bl[l] += 1
    bl[0] = 0
    nxt, code = [0] * (max_len + 2), 0
    for b in range(1, max_len + 1):
        code = (code + bl[b - 1]) << 1
        nxt[b] = code
    out = []
    for l in lens:
        if l == 0:
            out.append(0)
            continue
        c, nxt[l] = nxt[l], nxt[l] + 1
        out.append(int(format(c, f"0{l}b")[::-1], 2))
    return out


def code_length_symbols(seq):
    """the code-length sequence -> [(symbol of the code-length alphabet, extra bits, their value)]"""
    out, i = [], 0
    while i < len(seq):
        v, r = seq[i], 1
        while i + r < len(seq) and seq[i + r] == v:
            r += 1
        i += r
        if v == 0:
            while r >= 11:
                k = min(r, 138)
                out.append((18, 7, k - 11))
                r -= k
            if r >= 3:
                out.append((17, 3, r - 3))
                r = 0
            out += [(0, 0, 0)] * r
        else:
            out.append((v, 0, 0))
            r -= 1
            while r >= 3:
                k = min(r, 6)
                out.append((16, 2, k - 3))
                r -= k
            out += [(v, 0, 0)] * r
    return out


class Bits:
    """least significant bit first"""

    def __init__(self):
        self.out, self.acc, self.n, self.total = bytearray(), 0, 0, 0

    def put(self, value, nbits):
        self.acc |= value << self.n
        self.n += nbits
        self.total += nbits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def pad(self):
        if self.n:
            self.put(0, 8 - self.n)


def band_plan(d, run_cap=258):
    """a band's bytes -> (tokens, literal/length lengths [286], code-length lengths [19])"""
    toks = tokens(d, run_cap)
    counts = [0] * 286
    counts[256] = 1
    for kind, v in toks:
        counts[v if kind == "lit" else length_symbol(v)[0]] += 1
    ll = build_lengths(counts, 15)
    hlit = max(s for s in range(286) if ll[s]) + 1
    cl_counts = [0] * 19
    for s, _, _ in code_length_symbols(ll[:hlit] + [1]):
        cl_counts[s] += 1
    return toks, ll, build_lengths(cl_counts, 7)


def dynamic_block(d, run_cap=258, sync=True):
    """the band as one dynamic block (BFINAL 0) and the empty stored block after it"""
    toks, ll, cl = band_plan(d, run_cap)
    hlit = max(s for s in range(286) if ll[s]) + 1
    hclen = max(max(i for i in range(19) if cl[CL_ORDER[i]]) + 1, 4)
    ll_code, cl_code = canonical_codes(ll, 15), canonical_codes(cl, 7)
    w = Bits()
    w.put(0, 1)
    w.put(2, 2)
    w.put(hlit - 257, 5)
    w.put(0, 5)
    w.put(hclen - 4, 4)
    for i in range(hclen):
        w.put(cl[CL_ORDER[i]], 3)
    for s, eb, ev in code_length_symbols(ll[:hlit] + [1]):
        w.put(cl_code[s], cl[s])
        w.put(ev, eb)
    for kind, v in toks:
        if kind == "lit":
            w.put(ll_code[v], ll[v])
        else:
            s, eb, ev = length_symbol(v)
            w.put(ll_code[s], ll[s])
            w.put(ev, eb)
            w.put(0, 1)                                                          # the one distance code: symbol 0, distance 1
    w.put(ll_code[256], ll[256])
    if sync:
        w.put(0, 3)
        w.pad()
        return bytes(w.out) + SYNC_BLOCK
    w.pad()
    return bytes(w.out)


def stored_block(d):
    return b"\x00" + struct.pack("<HH", len(d), len(d) ^ 0xffff) + bytes(d)


def band_bytes(d, run_cap=258, sync=True):
    """the deflate bytes of one band: the dynamic form, or the stored form where the dynamic one is not smaller"""
    dyn, sto = dynamic_block(d, run_cap, sync), stored_block(d)
    return dyn if len(dyn) < len(sto) else sto


# ---- the file --------------------------------------------------------------------------------------------------------------------------------------------------------

def chunk(kind, payload):
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload))


def encode_png(frame, filter="adaptive", rows_per_block=None, tie="lowest", run_cap=258, sync=True):
    """uint8 [H, W, 3] -> the file's bytes.  tie / run_cap / sync are the rules that the tests break on purpose."""
    frame = np.asarray(frame, np.uint8)
    H, W, _ = frame.shape
    R, n_bands, row, _ = geometry(H, W, rows_per_block)
    filt = filter_frame(frame, filter, tie)
    out = SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0))
    for b in range(n_bands):
        payload = band_bytes(filt[b * R:(b + 1) * R].reshape(-1), run_cap, sync)
        if b == 0:
            payload = ZLIB_HEADER + payload
        if b == n_bands - 1:
            payload += FINAL_BLOCK + struct.pack(">I", zlib.adler32(filt.tobytes()))
        out += chunk(b"IDAT", payload)
    return out + chunk(b"IEND", b"")


def encode_clip(frames, **kw):
    """uint8 [F, H, W, 3] -> (all files in one uint8 array, int64 offsets [F + 1])"""
    files = [encode_png(f, **kw) for f in np.asarray(frames).reshape(-1, *np.asarray(frames).shape[-3:])]
    return np.frombuffer(b"".join(files), np.uint8), np.cumsum([0] + [len(s) for s in files]).astype(np.int64)


# ---- a decoder -------------------------------------------------------------------------------------------------------------------------------------------------------

def chunks(data):
    """[(type, payload)]; asserts the signature, every length and every CRC"""
    assert data[:8] == SIGNATURE
    pos, out = 8, []
    while pos < len(data):
        n, kind = struct.unpack_from(">I4s", data, pos)
        payload = data[pos + 8:pos + 8 + n]
        assert len(payload) == n and struct.unpack_from(">I", data, pos + 8 + n)[0] == zlib.crc32(kind + payload), f"chunk {kind!r} at byte {pos}"
        out.append((kind, payload))
        pos += 12 + n
    assert pos == len(data) and out[0][0] == b"IHDR" and out[-1] == (b"IEND", b"")
    return out


def filtered_bytes(data):
    """the file's filtered bytes, as zlib inflates them, and (W, H)"""
    ch = chunks(data)
    W, H, depth, colour, comp, flt, lace = struct.unpack(">IIBBBBB", ch[0][1])
    assert (depth, colour, comp, flt, lace) == (8, 2, 0, 0, 0)
    raw = zlib.decompress(b"".join(p for k, p in ch if k == b"IDAT"))
    assert len(raw) == H * (1 + 3 * W)
    return raw, W, H


def decode_png(data):
    """the file -> uint8 [H, W, 3]"""
    raw, W, H = filtered_bytes(bytes(data))
    rows = np.frombuffer(raw, np.uint8).reshape(H, 1 + 3 * W)
    out = np.zeros((H, 3 * W), np.int32)
    prev = np.zeros(3 * W, np.int32)
    for y in range(H):
        t, f = int(rows[y, 0]), rows[y, 1:].astype(np.int32)
        assert t < 5
        if t == 0:
            cur = f
        elif t == 2:
            cur = (f + prev) & 255
        elif t == 1:
            cur = (np.cumsum(f.reshape(W, 3), 0) & 255).reshape(-1)
        else:
            cur = np.zeros(3 * W, np.int32)
            for x in range(3 * W):
                a = cur[x - 3] if x >= 3 else 0
                b, c = prev[x], (prev[x - 3] if x >= 3 else 0)
                if t == 1:
                    pred = a
                elif t == 3:
                    pred = (a + b) >> 1
                else:
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if pa <= pb and pa <= pc else b if pb <= pc else c
                cur[x] = (f[x] + pred) & 255
        out[y] = prev = cur
    return out.astype(np.uint8).reshape(H, W, 3)
