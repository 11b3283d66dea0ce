"""One list of clean and damaged PNG files for the reader's CPU and GPU tests (tests/test_png_decode_cpu.py, tests/test_png_decode_gpu.py).  Every clean case states what
its stream contains and asserts it from the restatement's trace; every damaged case states the status bit it is there for.  Not a test module."""
import functools
import struct
import zlib
from typing import NamedTuple

import numpy as np

import png_dec_ref as R


class Case(NamedTuple):
    name: str
    data: bytes                                 # the file
    frame: object                               # uint8 [H, W, 3], the pixels a reader returns; None for a damaged file
    status: int                                 # what the restatement reports


def noise(H, W, bpp=3, seed=0, hi=256):
    return np.random.default_rng(seed).integers(0, hi, (H, W, bpp), dtype=np.uint8)


def smooth(H, W, bpp=3, seed=0):
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([(3 * x + y) % 256, (x + 2 * y) % 256, (x * y) % 256, (x + y) % 256][:bpp], -1)
    return ((base + np.random.default_rng(seed).integers(0, 3, (H, W, bpp))) % 256).astype(np.uint8)


def fibonacci_frame():
    """the skewed counts of test_png_cpu.band_cases as one row of pixels: literal counts that ask for codes longer than 15 bits.  The counts are changed from there:
    the filter byte and the end of block are the two ones of the Fibonacci sequence and every later number is one symbol's count (the last less one, for whole
    pixels), which makes the tree one chain; 28654 bytes in all, so that zlib puts them into ONE block (its symbol buffer holds 32767)"""
    fib = [1, 1]
    while len(fib) < 21:
        fib.append(fib[-1] + fib[-2])
    fib[-1] -= 1
    band = np.concatenate([np.full(c, 10 * i + 7, np.uint8) for i, c in enumerate(fib[2:])])
    return band.reshape(1, len(band) // 3, 3)


def _clean(name, data, frame, claim):
    tr = R.Trace()
    got, status = R.decode(data, tr)
    assert status == 0 and np.array_equal(got, frame[:, :, :3]), (name, status)
    assert claim(tr), (name, vars(tr))
    return Case(name, data, np.ascontiguousarray(frame[:, :, :3]), 0)


def _damaged(name, data, bit):
    _, status = R.decode(data)
    assert status & bit and status != 0, (name, status, bit)
    return Case(name, data, None, status)


def distance_stream():
    """(160, 85): 40960 filtered bytes in rows of 256, every byte 0 .. 4 so that any byte may stand in front of a row; fixed-Huffman tokens by hand: distances up to
    exactly 32768, which zlib never emits, and 258 under both of its codings"""
    rng = np.random.default_rng(5)
    w = R.FixedWriter()
    lits = rng.integers(0, 5, 32768).tolist()
    for v in lits:
        w.literal(v)
    tokens = [(258, 32768, False), (258, 32768, True), (100, 32507), (3, 32767), (200, 3), (258, 1, True)]
    n = 32768 + sum(t[0] for t in tokens)
    while n < 40960:
        k = min(258, 40960 - n)
        if k < 3:
            break
        tokens.append((k, 32768 - (n % 7), False))
        n += k
    for t in tokens:
        w.match(*t)
    for _ in range(40960 - n):
        w.literal(2)
    deflate = w.end()
    raw = zlib.decompressobj(-15).decompress(deflate)
    assert len(raw) == 40960
    return R.zlib_wrap(deflate, raw), raw


LL_CROSS = [8] * 254 + [9] * 4 + [0] * 28       # literals, end of block and length 3; the lengths 4 .. 258 sent as zeros
D_CROSS = [0, 0, 0, 0, 1, 1]                    # distances 5 .. 8


@functools.lru_cache(maxsize=1)
def clean_cases():
    out = []
    f35, f3347, f1786 = noise(3, 5, seed=1), smooth(33, 47, seed=2), smooth(17, 86, 4, seed=3)
    out.append(_clean("stored", R.write_png(f35, level=0), f35, lambda t: t.blocks == [0]))
    big = noise(160, 160, seed=4)
    out.append(_clean("two_stored", R.write_png(big, level=0), big, lambda t: len(t.blocks) >= 2 and set(t.blocks) == {0} and sum(t.stored_lengths) > 65535))
    out.append(_clean("fixed", R.write_png(f3347, [y % 5 for y in range(33)], strategy="fixed"), f3347, lambda t: set(t.blocks) == {1}))
    rep = np.concatenate([smooth(20, 47, seed=6), np.zeros((13, 47, 3), np.uint8)])
    out.append(_clean("dynamic_16_17_18", R.write_png(rep, [y % 5 for y in range(33)], level=9), rep, lambda t: 2 in t.blocks and t.cl_symbols == {16, 17, 18}))
    # a hand-made block whose run of zero lengths starts in the literal/length lengths and ends in the distance lengths
    toks = [("lit", v) for v in (0, 7, 9, 200, 31, 5, 6, 9)] + [("match", 3, 8), ("match", 3, 6), ("lit", 9), ("lit", 9)]   # one row of 5 pixels, filter none
    body = R.dynamic_block(LL_CROSS, D_CROSS, toks)
    want = zlib.decompressobj(-15).decompress(body)
    frame = np.frombuffer(want[1:], np.uint8).reshape(1, 5, 3)
    out.append(_clean("repeat_across_alphabets", R.make_png(1, 5, 2, R.zlib_wrap(body, want)), frame, lambda t: t.repeat_crossed and t.blocks == [2]))
    fibf = fibonacci_frame()
    out.append(_clean("code_of_15_bits", R.write_png(fibf, strategy="huffman"), fibf, lambda t: t.max_code_length == 15))
    lits = bytes([0]) + bytes(range(40, 55))
    body = R.dynamic_block([8] * 254 + [9] * 4, [0], [("lit", v) for v in lits])
    out.append(_clean("no_distance_code", R.make_png(1, 5, 2, R.zlib_wrap(body, lits)), np.frombuffer(lits[1:], np.uint8).reshape(1, 5, 3),
                      lambda t: t.distance_codes == [0]))
    import png_ref
    flat = np.zeros((9, 40, 3), np.uint8)
    flat[:, 20:] = 77
    out.append(_clean("single_distance_code", png_ref.encode_png(flat), flat,
                      lambda t: 1 in t.distance_codes))
    const = np.full((9, 200, 3), 131, np.uint8)
    out.append(_clean("distance_1_length_258", R.write_png(const, strategy="rle"), const, lambda t: t.max_distance == 1 and t.max_length == 258 and t.overlap))
    z, raw = distance_stream()
    frame, st = R.unfilter(raw, 160, 85, 3)
    assert st == 0
    out.append(_clean("distance_32768", R.make_png(160, 85, 2, z), frame,
                      lambda t: t.max_distance == 32768 and {284, 285} <= t.length_symbols and t.max_length == 258 and t.overlap))
    multi = noise(160, 85, seed=7, hi=64)                                       # 40960 literals of 6 bits: more than one block's 32767 symbols
    out.append(_clean("blocks_not_byte_aligned", R.write_png(multi, [y % 3 for y in range(160)], level=6), multi,
                      lambda t: len(t.blocks) >= 2 and any(s % 8 for s in t.block_bit_starts[1:])))
    z, _ = R.zlib_stream(R.filter_rows(f35, [1, 2, 4]))
    out.append(_clean("idats_of_one_byte", R.make_png(3, 5, 2, z, list(range(1, len(z)))), f35, lambda t: True))
    out.append(_clean("empty_idat", R.make_png(3, 5, 2, z, [5, 5]), f35, lambda t: True))
    out.append(_clean("five_filters_rgb", R.write_png(f3347, [y % 5 for y in range(33)]), f3347, lambda t: True))
    out.append(_clean("five_filters_rgba", R.write_png(f1786, [(y + 1) % 5 for y in range(17)]), f1786, lambda t: True))
    return out


def _png_of(deflate, adler=1, H=1, W=5):
    return R.make_png(H, W, 2, b"\x78\x9c" + deflate + struct.pack(">I", adler))


@functools.lru_cache(maxsize=1)
def damaged_cases():
    out = []
    f = smooth(9, 11, seed=9)
    raw = R.filter_rows(f, [y % 5 for y in range(9)])
    z = zlib.compress(raw, 6)
    good = lambda zs: R.make_png(9, 11, 2, zs)
    out.append(_damaged("block_type_3", _png_of(b"\x07"), R.BAD_BLOCK))
    out.append(_damaged("len_nlen", good(b"\x78\x01\x01" + struct.pack("<HH", len(raw), (len(raw) ^ 0xffff) ^ 0x0100) + raw + z[-4:]), R.BAD_BLOCK))
    out.append(_damaged("over_subscribed", _png_of(R.dynamic_block([8] * 257, [1, 1])), R.BAD_LENGTHS))
    out.append(_damaged("incomplete", _png_of(R.dynamic_block([8] * 254 + [9] * 3, [1, 1])), R.BAD_LENGTHS))
    out.append(_damaged("incomplete_distances", _png_of(R.dynamic_block([8] * 254 + [9] * 4, [2, 2])), R.BAD_LENGTHS))
    out.append(_damaged("no_end_of_block", _png_of(R.dynamic_block([8] * 254 + [9, 9, 0, 9, 9], [1, 1])), R.BAD_LENGTHS))
    out.append(_damaged("repeat_of_nothing", _png_of(R.dynamic_block([8] * 254 + [9] * 4, [1, 1], sequence=[(16, 0)])), R.BAD_LENGTHS))
    out.append(_damaged("repeat_past_the_end", _png_of(R.dynamic_block([8] * 254 + [9] * 4, [1, 1], sequence=[(18, 127), (18, 127)])), R.BAD_LENGTHS))
    w = R.FixedWriter()
    w.literal(0)
    w.symbol(286)
    out.append(_damaged("length_symbol_286", _png_of(w.end()), R.BAD_SYMBOL))
    w = R.FixedWriter()
    for v in (0, 1, 2, 3):
        w.literal(v)
    w.symbol(257)
    w.code(30, 5)
    out.append(_damaged("distance_symbol_30", _png_of(w.end()), R.BAD_SYMBOL))
    lits = bytes([0]) + bytes(range(40, 55))
    body = R.dynamic_block([8] * 254 + [9] * 4, [0], [("lit", 0), ("lit", 1), ("lit", 2), ("sym", 257)])
    out.append(_damaged("distance_without_a_code", _png_of(body + b"\xff\xff"), R.BAD_SYMBOL))
    w = R.FixedWriter()
    w.literal(0)
    w.literal(9)
    w.match(14, 3)
    out.append(_damaged("distance_before_the_start", _png_of(w.end()), R.BAD_DISTANCE))
    out.append(_damaged("truncated", good(z[:len(z) // 2]), R.TRUNCATED))
    out.append(_damaged("one_byte_too_many", good(z[:-4] + b"\x00" + z[-4:]), R.BAD_SIZE))
    out.append(_damaged("output_too_long", R.make_png(8, 11, 2, z), R.BAD_SIZE))
    out.append(_damaged("output_too_short", R.make_png(10, 11, 2, z), R.BAD_SIZE))
    out.append(_damaged("wrong_adler", good(z[:-1] + bytes([z[-1] ^ 1])), R.BAD_ADLER))
    bad = bytearray(raw)
    bad[2 * (1 + 33)] = 5
    out.append(_damaged("filter_type_5", good(zlib.compress(bytes(bad), 6)), R.BAD_FILTER))
    noisy = R.filter_rows(noise(9, 11, seed=10), [0] * 9)
    zn = bytearray(zlib.compress(noisy, 6))
    zn[len(zn) // 2] ^= 0x10
    out.append(_damaged("flipped_bit", good(bytes(zn)), 0xffff))                # the CRC is that of the damaged payload: only the stream is wrong
    return out


def all_cases():
    return clean_cases() + damaged_cases()
