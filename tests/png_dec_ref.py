"""The PNG reader restated in plain Python and numpy (include/tokensgen_hip.h, "Reading PNG"; tokensgen_amd/csrc/png_inflate.h): an inflate that returns the bytes, the
status bits of the header's list and a trace of what the stream contained; the filter inverses; the whole decode of a file; and writers of foreign files and of
hand-made streams for the cases of tests/png_dec_cases.py.  Not a test module."""
import struct
import zlib

import numpy as np

BAD_BLOCK, BAD_LENGTHS, BAD_SYMBOL, BAD_DISTANCE, TRUNCATED, BAD_SIZE, BAD_ADLER, BAD_FILTER, NOT_INDEPENDENT, BAD_RANGE = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
SIGNATURE = b"\x89PNG\r\n\x1a\n"
KIND_CL, KIND_LL, KIND_D = 0, 1, 2


def length_base(sym):
    """symbol 257 .. 285 -> (base, extra bits)"""
    if sym < 265:
        return sym - 254, 0
    if sym == 285:
        return 258, 0
    eb = (sym - 261) >> 2
    return 3 + ((4 + ((sym - 261) & 3)) << eb), eb


def distance_base(sym):
    """symbol 0 .. 29 -> (base, extra bits)"""
    if sym < 4:
        return 1 + sym, 0
    eb = (sym >> 1) - 1
    return 1 + ((2 + (sym & 1)) << eb), eb


class Trace:
    """what a stream contained"""

    def __init__(self):
        self.blocks = []                        # 0 stored, 1 fixed, 2 dynamic, in order
        self.block_bit_starts = []              # the bit at which every block's header starts
        self.stored_lengths = []
        self.max_code_length = 0                # over the literal/length and distance codes of the dynamic blocks
        self.max_distance = 0
        self.max_length = 0
        self.length_symbols = set()             # the literal/length symbols above 256 that occurred
        self.overlap = False                    # a copy with distance < length
        self.repeat_crossed = False             # a repeat of the code-length sequence ran from the literal/length lengths into the distance lengths
        self.cl_symbols = set()                 # the symbols 16, 17, 18 that occurred
        self.distance_codes = []                # per dynamic block: how many distance symbols have a code


def build_code(lens, kind):
    """-> (table {(length, code): symbol}, ok): zlib's inflate_table rules"""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    left = 1
    for l in range(1, 16):
        left = (left << 1) - count[l]
        if left < 0:
            return None, False
    codes = len(lens) - count[0]
    ok = left == 0
    if kind == KIND_D:
        ok = left == 0 or codes == 0 or (codes == 1 and count[1] == 1)
    if kind == KIND_LL and ok:
        ok = lens[256] != 0
    table, code = {}, 0
    for l in range(1, 16):
        for s, sl in enumerate(lens):
            if sl == l:
                table[(l, code)] = s
                code += 1
        code <<= 1
    return table, ok


class Bits:
    def __init__(self, data, begin, end):
        self.data, self.pos, self.end = data, 8 * begin, 8 * end

    @property
    def left(self):
        return self.end - self.pos

    def take(self, k):
        if self.left < k:
            return None
        v = 0
        for i in range(k):
            p = self.pos + i
            v |= ((self.data[p >> 3] >> (p & 7)) & 1) << i
        self.pos += k
        return v

    def symbol(self, table):
        """-> (symbol, 0) or (None, status bit)"""
        code, left = 0, self.left
        for l in range(1, 16):
            p = self.pos + l - 1
            code = (code << 1) | (((self.data[p >> 3] >> (p & 7)) & 1) if p < self.end else 0)
            s = table.get((l, code))
            if s is not None:
                if l > left:
                    return None, TRUNCATED
                self.pos += l
                return s, 0
        return None, TRUNCATED if left < 15 else BAD_SYMBOL


FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32


def inflate(data, cap, begin=0, end=None, mode="stream", last=True, at=0, trace=None):
    """Raw deflate data[begin:end] -> (the bytes produced until the end or the first error, status).  mode "stream": the whole stream of a frame of `cap` filtered
    bytes; mode "chunk": one independent piece whose output starts at `at` (pi_inflate's rules)."""
    end = len(data) if end is None else end
    tr = trace if trace is not None else Trace()
    b, out = Bits(data, begin, end), bytearray()
    chunk = mode != "stream"

    def finish(status, final_seen=False):
        if not chunk:
            if not status and len(out) != cap:
                status = BAD_SIZE
        else:
            if not status and (final_seen != last or (last and at + len(out) != cap)):
                status = NOT_INDEPENDENT
            if status:
                status |= NOT_INDEPENDENT
        return bytes(out), status

    if at < 0 or at > cap:
        return finish(BAD_RANGE)
    while True:
        start = b.pos
        head = b.take(3)
        if head is None:
            return finish(TRUNCATED)
        typ = head >> 1
        tr.blocks.append(typ)
        tr.block_bit_starts.append(start - 8 * begin)
        if typ == 3:
            return finish(BAD_BLOCK)
        if typ == 0:
            b.pos += -b.pos % 8
            ln, nln = b.take(16), b.take(16)
            if ln is None or nln is None:
                return finish(TRUNCATED)
            if ln ^ 0xffff != nln:
                return finish(BAD_BLOCK)
            if b.left < 8 * ln:
                return finish(TRUNCATED)
            if at + len(out) + ln > cap:
                return finish(BAD_SIZE)
            out += data[b.pos >> 3:(b.pos >> 3) + ln]
            b.pos += 8 * ln
            tr.stored_lengths.append(ln)
        else:
            if typ == 1:
                ll, _ = build_code(FIXED_LL, KIND_LL)
                dd, _ = build_code(FIXED_D, KIND_D)
            else:
                hlit, hdist, hclen = b.take(5), b.take(5), b.take(4)
                if hlit is None or hdist is None or hclen is None:
                    return finish(TRUNCATED)
                nlen, ndist = 257 + hlit, 1 + hdist
                if nlen > 286 or ndist > 30:
                    return finish(BAD_LENGTHS)
                cl = [0] * 19
                for i in range(4 + hclen):
                    v = b.take(3)
                    if v is None:
                        return finish(TRUNCATED)
                    cl[CL_ORDER[i]] = v
                clt, ok = build_code(cl, KIND_CL)
                if not ok:
                    return finish(BAD_LENGTHS)
                lens = []
                while len(lens) < nlen + ndist:
                    s, st = b.symbol(clt)
                    if s is None:
                        return finish(st)
                    if s < 16:
                        lens.append(s)
                        continue
                    v = b.take({16: 2, 17: 3, 18: 7}[s])
                    if v is None:
                        return finish(TRUNCATED)
                    if s == 16:
                        if not lens:
                            return finish(BAD_LENGTHS)
                        val, rep = lens[-1], 3 + v
                    else:
                        val, rep = 0, (3 if s == 17 else 11) + v
                    if len(lens) + rep > nlen + ndist:
                        return finish(BAD_LENGTHS)
                    tr.cl_symbols.add(s)
                    if len(lens) < nlen < len(lens) + rep:
                        tr.repeat_crossed = True
                    lens += [val] * rep
                ll, ok = build_code(lens[:nlen], KIND_LL)
                if not ok:
                    return finish(BAD_LENGTHS)
                dd, ok = build_code(lens[nlen:], KIND_D)
                if not ok:
                    return finish(BAD_LENGTHS)
                tr.max_code_length = max(tr.max_code_length, max(lens))
                tr.distance_codes.append(sum(1 for v in lens[nlen:] if v))
            while True:
                s, st = b.symbol(ll)
                if s is None:
                    return finish(st)
                if s < 256:
                    if at + len(out) >= cap:
                        return finish(BAD_SIZE)
                    out.append(s)
                    continue
                if s == 256:
                    break
                if s > 285:
                    return finish(BAD_SYMBOL)
                base, eb = length_base(s)
                v = b.take(eb) if eb else 0
                if v is None:
                    return finish(TRUNCATED)
                length = base + v
                ds, st = b.symbol(dd)
                if ds is None:
                    return finish(st)
                if ds > 29:
                    return finish(BAD_SYMBOL)
                base, eb = distance_base(ds)
                v = b.take(eb) if eb else 0
                if v is None:
                    return finish(TRUNCATED)
                dist = base + v
                if dist > len(out):
                    return finish(NOT_INDEPENDENT if chunk else BAD_DISTANCE)
                if at + len(out) + length > cap:
                    return finish(BAD_SIZE)
                tr.max_distance, tr.max_length = max(tr.max_distance, dist), max(tr.max_length, length)
                tr.length_symbols.add(s)
                tr.overlap |= dist < length
                src = len(out) - dist
                if dist >= length:
                    out += out[src:src + length]
                else:
                    out += bytes(out[src + i % dist] for i in range(length))
        if head & 1:
            return finish(BAD_SIZE if b.left >= 8 else 0, True)
        if chunk and b.left == 0:
            return finish(0)


def paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else b if pb <= pc else c


def unfilter(filtered, H, W, bpp):
    """filtered bytes, H rows of 1 + bpp W -> (uint8 [H, W, 3], status): the header's definitions; a filter type above 4 is read as 0 and reported"""
    rows = np.frombuffer(bytes(filtered), np.uint8).reshape(H, 1 + bpp * W)
    out = np.zeros((H, W * bpp), np.int64)
    status = 0
    for y in range(H):
        t, x = int(rows[y, 0]), rows[y, 1:].astype(np.int64)
        up = out[y - 1] if y else np.zeros(W * bpp, np.int64)
        if t > 4:
            status |= BAD_FILTER
            t = 0
        if t == 0:
            out[y] = x
        elif t == 2:
            out[y] = (x + up) & 255
        elif t == 1:
            out[y] = (np.cumsum(x.reshape(W, bpp), 0) & 255).reshape(-1)
        else:
            cur = [0] * (W * bpp)
            xs, ups = x.tolist(), up.tolist()
            for i in range(W * bpp):
                a = cur[i - bpp] if i >= bpp else 0
                c = ups[i - bpp] if i >= bpp else 0
                cur[i] = (xs[i] + ((a + ups[i]) >> 1 if t == 3 else paeth(a, ups[i], c))) & 255
            out[y] = cur
    return out.reshape(H, W, bpp)[:, :, :3].astype(np.uint8), status


def filter_rows(frame, types):
    """uint8 [H, W, bpp] and one filter type per row (a type above 4 is written as it is over the raw row) -> the filtered bytes"""
    H, W, bpp = frame.shape
    raw = frame.reshape(H, W * bpp).astype(np.int64)
    out = bytearray()
    for y in range(H):
        t = types[y]
        cur, up = raw[y], raw[y - 1] if y else np.zeros(W * bpp, np.int64)
        a = np.concatenate([np.zeros(bpp, np.int64), cur[:-bpp]])
        c = np.concatenate([np.zeros(bpp, np.int64), up[:-bpp]])
        if t == 1:
            pred = a
        elif t == 2:
            pred = up
        elif t == 3:
            pred = (a + up) >> 1
        elif t == 4:
            pred = np.array([paeth(int(p), int(q), int(r)) for p, q, r in zip(a, up, c)], np.int64)
        else:
            pred = 0
        out.append(t)
        out += ((cur - pred) & 255).astype(np.uint8).tobytes()
    return bytes(out)


# ---- the container ----------------------------------------------------------------------------------------------------------------------------------------------------
def chunk(kind, payload):
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload))


def make_png(H, W, color_type, zstream, cuts=(), extra=()):
    """The file around a zlib stream, its IDATs cut at `cuts` (positions in the stream; equal neighbours give an empty IDAT); extra: chunks (kind, payload) put in
    front of the first IDAT."""
    edges = [0] + sorted(cuts) + [len(zstream)]
    body = b"".join(chunk(k, p) for k, p in extra) + b"".join(chunk(b"IDAT", zstream[a:b]) for a, b in zip(edges, edges[1:]))
    return SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, color_type, 0, 0, 0)) + body + chunk(b"IEND", b"")


STRATEGIES = {"default": zlib.Z_DEFAULT_STRATEGY, "fixed": zlib.Z_FIXED, "huffman": zlib.Z_HUFFMAN_ONLY, "rle": zlib.Z_RLE, "filtered": zlib.Z_FILTERED}


def zlib_stream(raw, level=6, strategy="default", flush=None, pieces=1, wbits=15):
    """-> (the zlib stream of raw, the cut points behind every flushed piece): `raw` is fed in `pieces` parts with compressobj.flush(flush) behind each but the last"""
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, STRATEGIES[strategy])
    step = -(-len(raw) // pieces)
    out, cuts = b"", []
    for k in range(pieces):
        out += co.compress(raw[k * step:(k + 1) * step])
        if k + 1 < pieces and flush is not None:
            out += co.flush(flush)
            cuts.append(len(out))
    return out + co.flush(), cuts


def write_png(frame, types=None, level=6, strategy="default", cuts=(), flush=None, pieces=1):
    """A foreign file of uint8 [H, W, 3] or [H, W, 4]; types: the filter of every row (default: all none); with `flush` the stream is cut where it was flushed."""
    H, W, bpp = frame.shape
    z, at = zlib_stream(filter_rows(frame, types or [0] * H), level, strategy, flush, pieces)
    return make_png(H, W, 2 if bpp == 3 else 6, z, at if flush is not None else cuts)


def zlib_wrap(deflate, raw):
    return b"\x78\x9c" + deflate + struct.pack(">I", zlib.adler32(raw))


class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, bits):
        """least significant bit first"""
        self.acc |= value << self.n
        self.n += bits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, length):
        """a Huffman code: most significant bit first"""
        self.put(int(format(code, f"0{length}b")[::-1], 2), length)

    def done(self):
        if self.n:
            self.put(0, 8 - self.n)
        return bytes(self.out)


class FixedWriter(BitWriter):
    """one fixed-Huffman block from hand-made tokens"""

    def __init__(self, final=True):
        super().__init__()
        self.put(1 if final else 0, 1)
        self.put(1, 2)

    def symbol(self, s):
        if s < 144:
            self.code(0x30 + s, 8)
        elif s < 256:
            self.code(0x190 + s - 144, 9)
        elif s < 280:
            self.code(s - 256, 7)
        else:
            self.code(0xc0 + s - 280, 8)

    def literal(self, v):
        self.symbol(v)

    def match(self, length, dist, long_258=False):
        """long_258: length 258 as symbol 284 with extra bits 31, the other of its two codings"""
        sym = 284 if long_258 and length == 258 else next(s for s in range(285, 256, -1) if length_base(s)[0] <= length and (s == 285) == (length == 258))
        base, eb = length_base(sym)
        self.symbol(sym)
        self.put(length - base, eb)
        ds = next(s for s in range(29, -1, -1) if distance_base(s)[0] <= dist)
        base, eb = distance_base(ds)
        self.code(ds, 5)
        self.put(dist - base, eb)

    def end(self):
        self.symbol(256)
        return self.done()


# ---- a whole file -----------------------------------------------------------------------------------------------------------------------------------------------------
def read_container(data):
    """the minimum a test needs: (H, W, colour type, the IDAT payloads); no check"""
    pos, idat, head = 8, [], None
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", data[pos + 8:pos + 8 + n])
        if kind == b"IDAT":
            idat.append(data[pos + 8:pos + 8 + n])
        pos += 12 + n
    return head[1], head[0], head[3], idat


def decode(data, trace=None):
    """A file -> (uint8 [H, W, 3] or None, status): the stream route, and what tg_png_unfilter adds: the Adler comparison if the stream decoded, the filters if it
    matched."""
    H, W, ct, idat = read_container(data)
    bpp = 3 if ct == 2 else 4
    z = b"".join(idat)
    out, status = inflate(z, H * (1 + bpp * W), 2, len(z) - 4, trace=trace)
    if status:
        return None, status
    if zlib.adler32(out) != struct.unpack(">I", z[-4:])[0]:
        return None, BAD_ADLER
    frame, status = unfilter(out, H, W, bpp)
    return frame, status


def decode_chunks(data):
    """The chunk route: every IDAT a piece -> (the filtered bytes or None, the status of the frame: the OR of the pieces')"""
    H, W, ct, idat = read_container(data)
    cap = H * (1 + (3 if ct == 2 else 4) * W)
    out, status = b"", 0
    for k, p in enumerate(idat):
        lo, hi = (2 if k == 0 else 0), len(p) - (4 if k == len(idat) - 1 else 0)
        got, st = inflate(p, cap, lo, hi, "chunk", k == len(idat) - 1, len(out))
        out += got
        status |= st
    return (out if not status else None), status


# ---- hand-made dynamic blocks -------------------------------------------------------------------------------------------------------------------------------------------
CL_LENGTHS = [4] * 13 + [5] * 6                 # a complete code over the 19 symbols: 13/16 + 6/32


def canonical(lens):
    """{symbol: (code, length)} of a set of lengths that is not over-subscribed"""
    out, code = {}, 0
    for l in range(1, 16):
        for s, sl in enumerate(lens):
            if sl == l:
                out[s] = (code, l)
                code += 1
        code <<= 1
    return out


def rle_sequence(seq):
    """a code-length sequence in the code-length alphabet, runs taken greedily over the WHOLE sequence: [(symbol, extra value)]"""
    out, i = [], 0
    while i < len(seq):
        v, r = seq[i], 1
        while i + r < len(seq) and seq[i + r] == v:
            r += 1
        if v == 0 and r >= 3:
            k = min(r, 138)
            out.append((18, k - 11) if k >= 11 else (17, k - 3))
            i += k
        elif v != 0 and r >= 4:
            k = min(r - 1, 6)
            out += [(v, 0), (16, k - 3)]
            i += 1 + k
        else:
            out.append((v, 0))
            i += 1
    return out


def dynamic_block(ll, dd, tokens=None, final=True, sequence=None):
    """One dynamic block with the literal/length lengths ll (257 .. 286 of them) and the distance lengths dd, as bytes (zeros to the byte).  tokens: ("lit", v),
    ("match", length, distance) or ("sym", s); None: the header alone.  sequence: the coded lengths as [(symbol, extra value)] instead of rle_sequence(ll + dd)."""
    w = BitWriter()
    w.put(1 if final else 0, 1)
    w.put(2, 2)
    w.put(len(ll) - 257, 5)
    w.put(len(dd) - 1, 5)
    w.put(15, 4)
    for s in CL_ORDER:
        w.put(CL_LENGTHS[s], 3)
    clc = canonical(CL_LENGTHS)
    for s, ev in (sequence if sequence is not None else rle_sequence(list(ll) + list(dd))):
        w.code(*clc[s])
        if s >= 16:
            w.put(ev, {16: 2, 17: 3, 18: 7}[s])
    if tokens is not None:
        llc, ddc = canonical(ll), canonical(dd)
        for t in tokens:
            if t[0] == "lit" or t[0] == "sym":
                w.code(*llc[t[1]])
            else:
                sym = next(s for s in range(285, 256, -1) if length_base(s)[0] <= t[1] and (s == 285) == (t[1] == 258))
                base, eb = length_base(sym)
                w.code(*llc[sym])
                w.put(t[1] - base, eb)
                ds = next(s for s in range(29, -1, -1) if distance_base(s)[0] <= t[2])
                base, eb = distance_base(ds)
                w.code(*ddc[ds])
                w.put(t[2] - base, eb)
        w.code(*llc[256])
    return w.done()
