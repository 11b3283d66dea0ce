"""CPU: the PNG definition as tests/png_ref.py restates it (its files decode to the source through its own decoder and through Pillow, every CRC-32 and the Adler-32
are zlib's, three wrong rules change the bytes or break the file, the adaptive choice is a brute-force search per row, the size conditions), tokensgen_amd.png's
geometry and every refusal that needs no device, the argument validation of the C entry points of csrc/png.hip (before any launch), and the deflate pieces of
csrc/png_deflate.h as a host program under the address and undefined-behaviour sanitizers, line by line against the restatement."""
import ctypes
import io
import os
import shutil
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_ref as P
from tokensgen_amd import png

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (1, 2), (2, 1), (3, 5), (33, 47), (17, 86)]


def noise(shape, seed=0):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def smooth(H, W, seed=0):
    y, x = np.mgrid[0:H, 0:W]
    f = np.stack([2 * x + y, 255 - x // 2, (x * y) // 7 + 3 * seed], -1)
    f[H // 3:, W // 4:W // 2] = 40 + seed
    f[:, 3 * W // 4:] += np.random.default_rng(seed).integers(0, 3, (H, W - 3 * W // 4, 3))
    return (f & 255).astype(np.uint8)


def sources(H, W):
    return {"smooth": smooth(H, W), "noise": noise((H, W, 3)), "flat": np.full((H, W, 3), 131, np.uint8), "zeros": np.zeros((H, W, 3), np.uint8)}


@pytest.fixture(scope="module")
def files():
    """(size, source name, filter, rows_per_block) -> (frame, file): computed once for the tests that read them"""
    out = {}
    for H, W in SIZES:
        for name, frame in sources(H, W).items():
            for flt, R in [("adaptive", None), ("adaptive", 1), ("adaptive", 3), ("none", None), ("sub", 3), ("up", None), ("average", 1), ("paeth", None)]:
                out[(H, W), name, flt, R] = (frame, P.encode_png(frame, flt, R))
    return out


def test_files_decode_to_the_source(files):
    for key, (frame, data) in files.items():
        assert np.array_equal(P.decode_png(data), frame), key


def test_pillow_decodes_to_the_source(files):
    Image = pytest.importorskip("PIL.Image")
    for key, (frame, data) in files.items():
        im = Image.open(io.BytesIO(data))
        assert im.mode == "RGB" and im.size == (frame.shape[1], frame.shape[0]), key
        assert np.array_equal(np.array(im.convert("RGB")), frame), key


def test_checksums_and_container(files):
    """every chunk's CRC-32 is zlib.crc32 of type and payload, the stream's last four bytes zlib.adler32 of the filtered bytes; one IDAT per band; the band's framing"""
    for ((H, W), name, flt, R), (frame, data) in files.items():
        chunks = P.chunks(data)                                                 # asserts every CRC against zlib.crc32
        pos = 8
        for kind, payload in chunks:
            assert struct.unpack_from(">I", data, pos + 8 + len(payload))[0] == zlib.crc32(kind + payload)
            pos += 12 + len(payload)
        idat = [p for k, p in chunks if k == b"IDAT"]
        rows, bands, row, _ = P.geometry(H, W, R)
        filtered = P.filter_frame(frame, flt)
        assert [k for k, _ in chunks] == [b"IHDR"] + [b"IDAT"] * bands + [b"IEND"]
        assert chunks[0][1] == struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)
        assert idat[0][:2] == b"\x78\x01" and idat[-1][-6:-4] == b"\x03\x00"
        assert struct.unpack(">I", idat[-1][-4:])[0] == zlib.adler32(filtered.tobytes())
        assert P.filtered_bytes(data)[0] == filtered.tobytes()
        for b, payload in enumerate(idat):                                      # every band inflates alone: no token refers across a band
            body = payload[2 if b == 0 else 0:len(payload) - (6 if b == bands - 1 else 0)]
            assert zlib.decompressobj(-15).decompress(body + b"\x03\x00") == filtered[b * rows:(b + 1) * rows].tobytes()
            assert body[-4:] == b"\x00\x00\xff\xff" or body[:1] == b"\x00"      # the empty stored block, or the band itself stored


def test_three_wrong_rules():
    """each rule of the definition matters: the tie to the highest filter type, a run cap of 259, a missing empty stored block"""
    frame = np.zeros((17, 86, 3), np.uint8)
    frame[5:] = smooth(12, 86)
    good = P.encode_png(frame)
    assert np.array_equal(P.decode_png(good), frame)
    tie = P.encode_png(frame, tie="highest")                                    # rows of zeros cost 0 under every type: type 4 instead of 0
    assert tie != good and np.array_equal(P.decode_png(tie), frame)
    assert P.filter_frame(frame)[0, 0] == 0 and P.filter_frame(frame, tie="highest")[0, 0] == 4
    cap = P.encode_png(frame, run_cap=259)                                      # a row of zeros is 259 bytes: one match of 259, a length deflate does not have
    assert cap != good
    with pytest.raises((zlib.error, AssertionError)):
        assert np.array_equal(P.decode_png(cap), frame)
    sync = P.encode_png(frame, rows_per_block=3, sync=False)                    # bands that end inside a byte cannot be concatenated
    assert sync != P.encode_png(frame, rows_per_block=3)
    with pytest.raises((zlib.error, AssertionError)):
        assert np.array_equal(P.decode_png(sync), frame)


def test_adaptive_choice_is_the_brute_force_minimum():
    """per row and per type in plain Python: predict, subtract, sum min(v, 256 - v); the lowest type of the smallest sum"""
    def paeth(a, b, c):
        p = a + b - c
        pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
        return a if pa <= pb and pa <= pc else b if pb <= pc else c

    for frame in (smooth(9, 14), noise((6, 5, 3), 2), np.zeros((3, 4, 3), np.uint8), smooth(33, 47, 3)[:12]):
        H, W, _ = frame.shape
        raw = frame.reshape(H, 3 * W).astype(int).tolist()
        got = P.filter_frame(frame)
        seen = set()
        for y in range(H):
            best = None
            for t in range(5):
                out = []
                for i in range(3 * W):
                    a = raw[y][i - 3] if i >= 3 else 0
                    b = raw[y - 1][i] if y else 0
                    c = raw[y - 1][i - 3] if y and i >= 3 else 0
                    out.append((raw[y][i] - (0, a, b, (a + b) // 2, paeth(a, b, c))[t]) & 255)
                cost = sum(min(v, 256 - v) for v in out)
                if best is None or cost < best[0]:
                    best = (cost, t, out)
            assert got[y, 0] == best[1] and got[y, 1:].tolist() == best[2], (frame.shape, y)
            seen.add(best[1])
        for name in P.FILTERS:                                                  # and the forced types are that type's row
            assert (P.filter_frame(frame, name)[:, 0] == P.FILTERS.index(name)).all()
    assert len(seen) >= 2


def test_size_conditions():
    """what is known of the sizes without a measurement"""
    overhead = png.FILE_HEADER_BYTES + png.FILE_TRAILER_BYTES + 2 + 6           # signature, IHDR, IEND, the zlib header, the final block and Adler-32
    for H, W in [(17, 86), (33, 47), (64, 96), (40, 300), (5, 21844)]:
        for R in (None, 1, 3):
            if R is not None and R * (1 + 3 * W) > 65535:
                continue
            bands = P.geometry(H, W, R)[1]
            flat = P.encode_png(np.full((H, W, 3), 200, np.uint8), rows_per_block=R)
            assert len(flat) <= H * (-(-3 * W // 258) + 8) + 64 * bands + 100, (H, W, R)
    for H, W in [(33, 47), (17, 86), (3, 5), (1, 1)]:
        for R in (None, 1, 3):
            bands = P.geometry(H, W, R)[1]
            for frame in (noise((H, W, 3), 7), smooth(H, W), np.zeros((H, W, 3), np.uint8)):
                data = P.encode_png(frame, rows_per_block=R)
                assert len(data) <= H * (1 + 3 * W) + bands * (5 + 5 + 12) + overhead
                assert len(data) <= png.png_geometry(H, W, R).max_file_bytes
    stored = P.encode_png(noise((33, 47, 3), 7))
    assert len(stored) == 33 * 142 + 3 * 17 + overhead == png.png_geometry(33, 47).max_file_bytes
    for seed in range(3):                                                       # a smooth clip's files are smaller than raw
        assert len(P.encode_png(smooth(48, 64, seed))) < 48 * 64 * 3


def test_code_lengths_rule():
    """build_lengths: complete codes within the limit, the limit reached on skewed counts, one symbol alone gets one bit, ties by symbol"""
    fib = [1, 1]
    while len(fib) < 30:
        fib.append(fib[-1] + fib[-2])
    for counts, limit in [(fib + [0] * 256, 15), (fib[:19], 7), ([5] * 286, 15), ([0, 3, 0, 3], 7), ([1, 2, 4, 8, 16, 32, 64, 128, 256], 7)]:
        lens = P.build_lengths(counts, limit)
        used = [l for l in lens if l]
        assert max(used) <= limit and sum(2.0 ** -l for l in used) == 1.0 and all((l > 0) == (c > 0) for l, c in zip(lens, counts))
        order = sorted((s for s in range(len(counts)) if counts[s]), key=lambda s: (counts[s], s))
        assert [lens[s] for s in order] == sorted(used, reverse=True)           # rarer symbols never get shorter codes
    assert max(P.build_lengths(fib + [0] * 256, 15)) == 15 and max(P.build_lengths(fib[:19], 7)) == 7
    assert P.build_lengths([0, 0, 9, 0], 7) == [0, 0, 1, 0]
    assert P.build_lengths([1, 1, 1], 7) == [2, 2, 1]                           # equal counts: the later symbol is the later leaf, the last pair merges first
    assert [P.length_symbol(n) for n in (3, 10, 11, 12, 13, 18, 19, 114, 115, 227, 257, 258)] == [
        (257, 0, 0), (264, 0, 0), (265, 1, 0), (265, 1, 1), (266, 1, 0), (268, 1, 1), (269, 2, 0), (279, 4, 15), (280, 4, 0), (284, 5, 0), (284, 5, 30), (285, 0, 0)]
    assert P.code_length_symbols([0] * 139 + [5] * 8 + [0] * 4 + [3, 3, 0, 0]) == [(18, 7, 127), (0, 0, 0), (5, 0, 0), (16, 2, 3), (5, 0, 0), (17, 3, 1), (3, 0, 0),
                                                                                 (3, 0, 0), (0, 0, 0), (0, 0, 0)]
    assert P.run_tokens(7, 1) == [("lit", 7)] and P.run_tokens(7, 3) == [("lit", 7)] * 3 and P.run_tokens(7, 4) == [("lit", 7), ("match", 3)]
    assert P.run_tokens(7, 259) == [("lit", 7), ("match", 258)] and P.run_tokens(7, 261) == [("lit", 7), ("match", 258), ("lit", 7), ("lit", 7)]
    assert P.run_tokens(7, 520) == [("lit", 7), ("match", 258), ("match", 258), ("match", 3)]


# ---- tokensgen_amd.png without a device ----------------------------------------------------------------------------------------------------------------------------

def test_png_geometry():
    assert png.png_geometry(480, 720) == (16, 30, 2161, 34576, 33 + 12 + 8 + 30 * 17 + 480 * 2161)
    assert png.png_geometry(480, 720, 30)[:4] == (30, 16, 2161, 64830)
    assert png.png_geometry(33, 47, 3)[:4] == (3, 11, 142, 426) and png.png_geometry(1, 1)[:4] == (16, 1, 4, 64)
    assert png.png_geometry(1, 21844)[:4] == (1, 1, 65533, 65533) and png.png_geometry(5, 1366)[:4] == (15, 1, 4099, 61485)
    assert png.png_geometry(65535, 1, 1).bands == 65535
    assert png.MAX_WIDTH == P.MAX_WIDTH and png.MAX_BAND_BYTES == P.MAX_BAND_BYTES and png.DEFAULT_ROWS_PER_BLOCK == P.DEFAULT_ROWS
    for H, W, R in [(480, 720, None), (33, 47, 3), (1, 21844, None), (7, 5000, 4), (9, 5000, None)]:
        assert tuple(png.png_geometry(H, W, R)[:4]) == P.geometry(H, W, R)
    with pytest.raises(ValueError, match="W <= 21844"):
        png.png_geometry(1, 21845)
    for H, W, R in [(0, 5, None), (65536, 5, None), (5, 0, None), (5, 5, 0), (5, 5, -1), (5, 5, 4096), (5, 720, 31), (5, 5, 2.0), (5, 5, True), (5.0, 5, None)]:
        with pytest.raises(ValueError, match="png: "):
            png.png_geometry(H, W, R)


def test_refusals_need_no_device(tmp_path):
    """every refusal names its entry point and comes before any kernel call: these tensors are on the CPU"""
    u8 = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    for fn, args in [(png.encode_png, ()), (png.png_bytes, ()), (png.save_png_sequence, (str(tmp_path / "f_{:03d}.png"),))]:
        who = "encode_png" if fn is png.png_bytes else fn.__name__
        with pytest.raises(NotImplementedError, match=f"{who}: uint8 frames only"):
            fn(u8.float(), *args)
        with pytest.raises(ValueError, match=f"{who}: expected .*three channels"):
            fn(torch.zeros(2, 8, 8, 4, dtype=torch.uint8), *args)
        with pytest.raises(ValueError, match=f"{who}: expected .*three channels"):
            fn(torch.zeros(8, 8, 3, dtype=torch.uint8), *args)
        with pytest.raises(ValueError, match=f"{who}: expected a tensor"):
            fn(u8.numpy(), *args)
        with pytest.raises(ValueError, match=f"{who}: filter must be one of"):
            fn(u8, *args, filter="best")
        with pytest.raises(ValueError, match="rows_per_block must be an integer in 1..2621 "):
            fn(u8, *args, rows_per_block=2622)
        with pytest.raises(ValueError, match="W <= 21844"):
            fn(torch.zeros(1, 1, 21845, 3, dtype=torch.uint8), *args)
        with pytest.raises(RuntimeError, match=f"{who}: expected a GPU tensor"):
            fn(u8, *args)
    with pytest.raises(NotImplementedError, match="save_png: uint8 frames only"):
        png.save_png(u8[0].half(), str(tmp_path / "a.png"))
    with pytest.raises(ValueError, match="save_png: one frame per file, got 2"):
        png.save_png(u8, str(tmp_path / "a.png"))
    with pytest.raises(ValueError, match="save_png: filter"):
        png.save_png(u8[0], str(tmp_path / "a.png"), filter=3)
    with pytest.raises(ValueError, match="rows_per_block"):
        png.save_png(u8[0], str(tmp_path / "a.png"), rows_per_block=0)
    with pytest.raises(RuntimeError, match="save_png: expected a GPU tensor"):
        png.save_png(u8[0], str(tmp_path / "a.png"))
    for pattern, start in [("frame.png", 0), ("f_{}_{}.png", 0), ("f_{name}.png", 0), ("f_{:03d}.png", -1), ("f_{:03d}.png", 1.5), (7, 0)]:
        with pytest.raises(ValueError, match="save_png_sequence: pattern"):
            png.save_png_sequence(u8, pattern if not isinstance(pattern, str) else str(tmp_path / pattern), start)
    assert not os.listdir(tmp_path)                                             # nothing was written
    assert png.sequence_paths("out/frame_{:05d}.png", 3, 9) == ["out/frame_00009.png", "out/frame_00010.png", "out/frame_00011.png"]


def test_band_offsets():
    """the prefix sums between the two passes: plain torch, here on the CPU"""
    sizes = torch.tensor([[20, 30, 25], [14, 14, 40], [100, 1, 1]], dtype=torch.int32)
    offs, ends = png.band_offsets(sizes)
    assert ends.tolist() == [120, 233, 380] and offs.dtype == torch.int64 and offs.is_contiguous()
    assert offs.tolist() == [[33, 53, 83], [153, 167, 181], [266, 366, 367]]


def test_c_abi_validates_before_any_launch():
    """one argument wrong at a time; the calls never reach a launch"""
    from tokensgen_amd import kernels as K
    from tokensgen_amd import lib as L
    lib = L.load()
    err = lambda: lib.tg_last_error_string().decode()
    buf = ctypes.create_string_buffer(16384)
    p = ctypes.addressof(buf) + (16 - ctypes.addressof(buf) % 16)
    geo = lib.tg_png_geometry
    assert tuple(geo(480, 720, 0, w) for w in range(9)) == (16, 30, 2161, 30 * 34576, 352, png.png_geometry(480, 720).max_file_bytes, 33, 12, 0)
    assert tuple(geo(33, 47, 3, w) for w in range(4)) == (3, 11, 142, 11 * 432) and geo(1, 21844, 0, 0) == 1 and geo(1, 21844, 0, 3) == 65536
    assert geo(0, 8, 0, 0) == geo(65536, 8, 0, 0) == geo(8, 0, 0, 0) == geo(8, 21845, 0, 0) == geo(8, 8, -1, 0) == geo(8, 720, 31, 0) == 0
    for H, W, R in [(480, 720, None), (33, 47, 3), (1, 21844, None), (9, 5000, None), (65535, 1, 1)]:
        g, c = png.png_geometry(H, W, R), K.png_geometry(H, W, R or 0)
        assert (g.rows_per_block, g.bands, g.row_bytes, g.max_file_bytes) == (c[0], c[1], c[2], c[5]) and c[3] % 16 == 0 and c[3] >= g.bands * g.band_bytes
        assert (c[6], c[7]) == (png.FILE_HEADER_BYTES, png.FILE_TRAILER_BYTES)
    with pytest.raises(ValueError, match="png: a frame of"):
        K.png_geometry(8, 21845)
    assert K.PNG_FILTERS == {name: i for i, name in enumerate(P.FILTERS + ("adaptive",))}
    fl = dict(frames=p, F=1, H=16, W=16, filter=5, rows_per_block=0, filtered=p + 4096, stream=None)
    call = lambda **kw: lib.tg_png_filter(*{**fl, **kw}.values())
    for name in ("frames", "filtered"):
        assert call(**{name: None}) == -1 and "null pointer" in err()
    assert call(filter=-1) == -1 and call(filter=6) == -1 and "0..4" in err()
    assert call(F=0) == -2 and call(H=0) == -2 and call(H=65536) == -2 and call(W=0) == -2 and call(W=21845) == -2 and "1..21844" in err()
    assert call(rows_per_block=-1) == -2 and call(rows_per_block=1338) == -2 and "at most 65535" in err()
    assert call(filtered=p + 4100) == -3 and "16-byte" in err()
    bp = dict(filtered=p, F=1, H=16, W=16, rows_per_block=0, plans=p + 4096, band_bytes=p + 8192, stream=None)
    call = lambda **kw: lib.tg_png_band_plan(*{**bp, **kw}.values())
    for name in ("filtered", "plans", "band_bytes"):
        assert call(**{name: None}) == -1 and "null pointer" in err()
    assert call(F=0) == -2 and call(H=65536) == -2 and call(W=21845) == -2 and call(rows_per_block=1338) == -2
    assert call(filtered=p + 8) == -3 and call(plans=p + 4098) == -3 and call(band_bytes=p + 8193) == -3 and "4-byte" in err()
    wr = dict(filtered=p, plans=p + 4096, F=1, H=16, W=16, rows_per_block=0, band_offsets=p + 8192, data=p + 8448, data_bytes=4096, stream=None)
    call = lambda **kw: lib.tg_png_write(*{**wr, **kw}.values())
    for name in ("filtered", "plans", "band_offsets", "data"):
        assert call(**{name: None}) == -1 and "null pointer" in err()
    assert call(F=0) == -2 and call(H=0) == -2 and call(W=21845) == -2 and call(rows_per_block=-3) == -2
    assert call(data_bytes=44) == -2 and "cannot hold 1 files" in err() and call(F=3, data_bytes=134) == -2
    assert call(filtered=p + 4) == -3 and call(plans=p + 4097) == -3 and call(band_offsets=p + 8196) == -3 and "8-byte" in err()


# ---- the deflate pieces as a host program under the sanitizers ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ for the host build of csrc/png_deflate.h")
    exe = tmp_path_factory.mktemp("png_deflate_host") / "png_deflate_host"
    r = subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + os.path.join(ROOT, "tokensgen_amd", "csrc"), os.path.join(ROOT, "tests", "csrc", "png_deflate_host.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(bands):
        """bands: uint8 arrays -> per band (tokens, ll, cl, (header bits, token bits, dynamic bytes, stored), the deflate bytes, crc, adler); the sanitizers must stay
        silent"""
        blob = struct.pack("<I", len(bands)) + b"".join(struct.pack("<I", len(b)) + b.tobytes() for b in bands)
        path = exe.parent / "jobs.bin"
        path.write_bytes(blob)
        r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-3000:])
        lines, out = iter(r.stdout.splitlines()), []
        for _ in bands:
            rec = []
            for word in ("tokens", "ll", "cl", "plan", "bytes", "sums"):
                head, *rest = next(lines).split()
                assert head == word
                rec.append(rest)
            out.append((rec[0], [int(v) for v in rec[1]], [int(v) for v in rec[2]], tuple(int(v) for v in rec[3]), bytes.fromhex(rec[4][0]), int(rec[5][0]), int(rec[5][1])))
        assert next(lines, None) is None
        return out

    return run


def band_cases():
    rng = np.random.default_rng(1)
    bands = []
    for n in (1, 2, 3, 4, 5, 259, 260, 261, 262, 263, 517, 1000, 65535):
        bands += [np.full(n, 9, np.uint8), rng.integers(0, 256, n, dtype=np.uint8), (rng.integers(0, 4, n) * 60).astype(np.uint8),
                  np.repeat(rng.integers(0, 256, n // 7 + 1, dtype=np.uint8), 7)[:n]]
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    bands.append(np.concatenate([np.tile(np.array([i, 255 - i], np.uint8), c) for i, c in enumerate(fib)])[:65534])     # skewed counts: the limit of 15 bits
    for H, W in [(33, 47), (17, 86)]:                                           # real bands: the filtered rows of the frames of the other tests
        for frame in sources(H, W).values():
            bands.append(P.filter_frame(frame)[:16].reshape(-1))
    return bands


def test_host_program_equals_the_restatement(host_program):
    """tokens, code lengths and block bytes of csrc/png_deflate.h are png_ref's; its CRC-32 and Adler-32, put together from three parts, are zlib's"""
    bands = band_cases()
    limit = 0
    for band, (toks, ll, cl, plan, data, crc, adler) in zip(bands, host_program(bands)):
        want_toks, want_ll, want_cl = P.band_plan(band)
        assert toks == [("L%d" if kind == "lit" else "M%d") % v for kind, v in want_toks], len(band)
        assert ll == want_ll and cl == want_cl, len(band)
        dynamic = P.dynamic_block(band)
        assert plan[2] == len(dynamic) and plan[0] + plan[1] + ll[256] + 3 + 7 >> 3 == len(dynamic) - 4 and plan[3] == (len(dynamic) >= 5 + len(band))
        assert data == P.band_bytes(band), len(band)
        assert zlib.decompressobj(-15).decompress(data + b"\x03\x00") == band.tobytes()
        assert crc == zlib.crc32(band.tobytes()) and adler == zlib.adler32(band.tobytes())
        limit = max(limit, max(ll))
    assert limit == 15
