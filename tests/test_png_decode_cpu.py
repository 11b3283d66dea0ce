"""CPU: the PNG reader's definition as tests/png_dec_ref.py restates it (it decodes Pillow's files and tests/png_ref.py's files to the source and agrees with zlib on
every clean case of tests/png_dec_cases.py; a stream flushed with Z_SYNC_FLUSH per chunk is not independent, one flushed with Z_FULL_FLUSH is),
tokensgen_amd.png.parse_png with every refusal, inflate_plan, the refusals of decode_png before any device call, the index arithmetic of video_io.load_video for a
.png pattern through a stub reader, the argument validation of the C entry points of csrc/png_decode.hip (before any launch), and the shared decoder of
csrc/png_inflate.h as a host program under the address and undefined-behaviour sanitizers, on clean and on damaged streams."""
import ctypes
import io
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest
import torch

import png_dec_cases as C
import png_dec_ref as R
import png_ref
from tokensgen_amd import png, video_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pillow_png(frame, **kw):
    Image = pytest.importorskip("PIL.Image")
    buf = io.BytesIO()
    Image.fromarray(frame, "RGB" if frame.shape[2] == 3 else "RGBA").save(buf, "PNG", **kw)
    return buf.getvalue()


def test_restatement_decodes_pillow_and_our_own_files():
    for H, W, bpp in [(1, 1, 3), (3, 5, 4), (33, 47, 3), (17, 86, 4)]:
        for frame in (C.smooth(H, W, bpp, seed=H), C.noise(H, W, bpp, seed=W)):
            got, status = R.decode(pillow_png(frame))
            assert status == 0 and np.array_equal(got, frame[:, :, :3])
    for H, W, rows in [(1, 1, None), (33, 47, 3), (33, 47, 1), (17, 86, None)]:
        for frame in (C.smooth(H, W, seed=1), C.noise(H, W, seed=2)):
            data = png_ref.encode_png(frame, rows_per_block=rows)
            got, status = R.decode(data)
            assert status == 0 and np.array_equal(got, frame)
            filtered, status = R.decode_chunks(data)                            # every band of ours is an independent piece
            assert status == 0 and np.array_equal(R.unfilter(filtered, H, W, 3)[0], frame)


def test_restatement_agrees_with_zlib_on_every_clean_case():
    for case in C.clean_cases():
        H, W, ct, idat = R.read_container(case.data)
        z = b"".join(idat)
        out, status = R.inflate(z, H * (1 + (3 if ct == 2 else 4) * W), 2, len(z) - 4)
        assert status == 0 and out == zlib.decompress(z), case.name
        assert png.parse_png(case.data).idat == tuple(idat) and np.array_equal(R.decode(case.data)[0], case.frame)
    names = [c.name for c in C.all_cases()]
    assert len(set(names)) == len(names)
    bits = 0
    for case in C.damaged_cases():
        bits |= case.status
        assert case.frame is None and case.status
    assert bits & 255 == 255                                                    # every bit a file can show; 256 and 512 are not a file's (chunk mode; ranges)


def test_sync_flush_is_not_independent_and_full_flush_is():
    """Z_SYNC_FLUSH ends every piece on a byte but keeps the window: later pieces point back across the cut.  Z_FULL_FLUSH forgets the window."""
    frame = np.tile(C.smooth(8, 47, seed=3), (4, 1, 1))                         # the rows repeat: matches reach back across the flushes
    sync = R.write_png(frame, [0] * 32, flush=zlib.Z_SYNC_FLUSH, pieces=4)
    full = R.write_png(frame, [0] * 32, flush=zlib.Z_FULL_FLUSH, pieces=4)
    for data in (sync, full):
        assert png.inflate_plan([data])[0] == "chunk" and len(png.parse_png(data).idat) == 4
        assert np.array_equal(R.decode(data)[0], frame)
    filtered, status = R.decode_chunks(sync)
    assert status & R.NOT_INDEPENDENT and filtered is None
    filtered, status = R.decode_chunks(full)
    assert status == 0 and np.array_equal(R.unfilter(filtered, 32, 47, 3)[0], frame)


def rechunk(data, edit):
    """the file with its chunk list edited: edit([(kind, payload)]) -> the same"""
    pos, chunks = 8, []
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        chunks.append((kind, data[pos + 8:pos + 8 + n]))
        pos += 12 + n
    return R.SIGNATURE + b"".join(R.chunk(k, p) for k, p in edit(chunks))


def test_parse_png():
    frame = C.smooth(9, 11, seed=1)
    good = R.write_png(frame, cuts=[7, 30])
    info = png.parse_png(good)
    assert (info.height, info.width, info.color_type) == (9, 11, 2) and len(info.idat) == 3 and b"".join(info.idat) == b"".join(R.read_container(good)[3])
    assert png.parse_png(R.write_png(C.smooth(4, 5, 4))).color_type == 6
    with_text = rechunk(good, lambda c: c[:1] + [(b"tEXt", b"k\0v"), (b"pHYs", bytes(9))] + c[1:-1] + [(b"tIME", bytes(7))] + c[-1:])
    assert png.parse_png(with_text) == info                                     # ancillary chunks are skipped
    ihdr = lambda **kw: rechunk(good, lambda c: [(b"IHDR", struct.pack(">IIBBBBB", *{**dict(W=11, H=9, d=8, ct=2, c=0, f=0, i=0), **kw}.values()))] + c[1:])
    for data, word in [(ihdr(i=1), "interlaced"), (ihdr(d=16), "bit depth of 16"), (ihdr(d=4, ct=0), "bit depth of 4"), (ihdr(ct=3), "palette"), (ihdr(ct=0), "grey"),
                       (ihdr(ct=4), "grey with alpha"), (rechunk(good, lambda c: c[:1] + [(b"XyZw", b"")] + c[1:]), "critical chunk")]:
        with pytest.raises(NotImplementedError, match=word):
            png.parse_png(data, 3)
    flipped = bytearray(good)
    flipped[60] ^= 1
    split = rechunk(good, lambda c: c[:2] + [(b"tEXt", b"k\0v")] + c[2:])
    zbad = lambda b0, b1: rechunk(good, lambda c: c[:1] + [(b"IDAT", bytes([b0, b1]) + c[1][1][2:])] + c[2:])
    for data, word in [(b"\x89PNX" + good[4:], "signature"), (bytes(flipped), "CRC-32"), (good[:-5], "truncated"), (good[:40], "truncated"), (good[:-12], "no IEND"),
                       (split, "not consecutive"), (rechunk(good, lambda c: c[:1] + c[-1:]), "no IDAT"), (good + b"\0", "behind IEND"),
                       (rechunk(good, lambda c: c[1:]), "not IHDR"), (ihdr(W=0), "no PNG header"), (ihdr(ct=5), "no PNG header"),
                       (zbad(0x79, 0x9c), "zlib header"), (zbad(0x88, 0x1c), "zlib header"), (zbad(0x78, 0xbb), "zlib header"), (zbad(0x78, 0x9d), "zlib header"),
                       (R.make_png(9, 11, 2, b"\x78\x9c\x03"), "shorter than")]:
        with pytest.raises(ValueError, match=word) as e:
            png.parse_png(data, 3)
        assert "frame 3" in str(e.value) and not isinstance(e.value, png.PngDecodeError)


def test_inflate_plan():
    frame = C.smooth(33, 47, seed=1)
    ours = png_ref.encode_png(frame, rows_per_block=3)
    pillow = pillow_png(frame)
    assert png.inflate_plan([ours, ours])[0] == "chunk"
    stored = png_ref.encode_png(C.noise(33, 47, seed=5), rows_per_block=3)      # every band one stored block: whole blocks as well
    assert all(p[-4:] != b"\0\0\xff\xff" for p in png.parse_png(stored).idat[:-1]) and png.inflate_plan([stored, ours])[0] == "chunk"
    route, why = png.inflate_plan([ours, pillow])
    assert route == "stream" and "frame 1" in why and "one IDAT" in why
    z = b"".join(png.parse_png(pillow).idat)
    assert png.inflate_plan([R.make_png(33, 47, 2, z, [100])])[0] == "stream" and "00 00 FF FF" in png.inflate_plan([R.make_png(33, 47, 2, z, [100])])[1]
    bands = png.parse_png(ours).idat
    cut = len(bands[0]) + len(bands[1])
    zo = b"".join(bands)
    assert "empty" in png.inflate_plan([R.make_png(33, 47, 2, zo, [cut, cut])])[1]
    assert png.inflate_plan([R.make_png(33, 47, 2, zo, [cut])])[0] == "chunk"   # two bands in one IDAT: still whole blocks
    assert "checksum" in png.inflate_plan([R.make_png(33, 47, 2, zo, [cut, len(zo) - 2])])[1]
    assert png.inflate_plan([png.parse_png(ours)]) == png.inflate_plan([ours])
    with pytest.raises(ValueError, match="no frame"):
        png.inflate_plan([])


def test_every_refusal_comes_before_any_device_call(monkeypatch, tmp_path):
    from tokensgen_amd import kernels as K

    def never(*a, **k):
        raise AssertionError("a device call")

    for name in ("png_inflate", "png_unfilter", "png_decode_geometry"):
        monkeypatch.setattr(K, name, never)
    monkeypatch.setattr(png, "gpu_device", never)
    a, b = R.write_png(C.smooth(9, 11)), R.write_png(C.smooth(9, 12))
    with pytest.raises(ValueError, match="share size"):
        png.decode_png([a, b])
    with pytest.raises(ValueError, match="share size"):
        png.decode_png([a, R.write_png(C.smooth(9, 11, 4))])
    with pytest.raises(ValueError, match="inflate must be"):
        png.decode_png([a], inflate="sync")
    with pytest.raises(ValueError, match="independent pieces.*frame 0: one IDAT"):
        png.decode_png([a], inflate="chunk")
    with pytest.raises(ValueError, match="offsets"):
        png.decode_png(torch.zeros(8, dtype=torch.uint8))
    with pytest.raises(ValueError, match="offsets must rise"):
        png.decode_png(torch.zeros(8, dtype=torch.uint8), [0, 9])
    with pytest.raises(ValueError, match="goes with a tensor"):
        png.decode_png([a], [0, 1])
    with pytest.raises(ValueError, match="expected a list"):
        png.decode_png([])
    with pytest.raises(ValueError, match="frame 1: .*CRC-32"):
        png.decode_png([a, a[:50] + bytes([a[50] ^ 1]) + a[51:]])
    with pytest.raises(NotImplementedError, match="frame 0: .*interlaced"):
        png.decode_png([rechunk(a, lambda c: [(b"IHDR", c[0][1][:12] + b"\1")] + c[1:])])
    with pytest.raises(FileNotFoundError, match="is empty"):
        png.load_png_sequence(str(tmp_path / "f_{:03d}.png"))
    with pytest.raises(ValueError, match="number field"):
        png.load_png_sequence(str(tmp_path / "f.png"), count=2)
    with pytest.raises(ValueError, match="fps"):
        png.PNGSequenceReader(str(tmp_path / "f_{:03d}.png"), fps=0)
    for i in (0, 1, 2, 4):                                                      # 3 is missing: the sequence ends there
        (tmp_path / f"f_{i:03d}.png").write_bytes(a)
    with png.PNGSequenceReader(str(tmp_path / "f_{:03d}.png"), fps=12) as r:
        assert len(r) == 3 and r.size == (9, 11) and r.fps == 12 and r.get_avg_fps() == 12.0 and r.BATCH == 64
        with pytest.raises(IndexError):
            r.get_batch([3])
        with pytest.raises(ValueError, match="no frame"):
            r.get_batch([])
    assert len(png.PNGSequenceReader(str(tmp_path / "f_{:03d}.png"), start=4)) == 1


def test_load_video_of_a_png_pattern_through_a_stub_reader(monkeypatch, tmp_path):
    """load_video asks the sequence reader, opened at 8 frames a second, for exactly sample_frame_indices(len, 8, ...); load_image_sequence passes fps and start on;
    every other suffix is refused as before"""
    class Asked(Exception):
        pass

    class Stub:
        def __init__(self, pattern, fps=8, start=0, device=None):
            self.args = (pattern, fps, start)

        def __len__(self):
            return 97

        def get_avg_fps(self):
            return float(self.args[1])

        def get_batch(self, indices):
            raise Asked(self.args, list(indices))

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return False

    monkeypatch.setattr(png, "PNGSequenceReader", Stub)
    pattern = str(tmp_path / "clip_{:04d}.PNG")
    for nf, fps, t0, t1, chunks in ((13, -1, 0, -1, 1), (13, 4, 0, -1, 3), (8, 8, 1.0, 3.5, 2), (49, -1, 0, -1, 1)):
        with pytest.raises(Asked) as e:
            video_io.load_video(pattern, (48, 64), nf, False, fps, t0, t1, chunks)
        assert e.value.args[0] == (pattern, 8, 0) and e.value.args[1] == video_io.sample_frame_indices(97, 8.0, nf, fps, t0, t1, chunks).tolist()
    with pytest.raises(Asked) as e:
        video_io.load_image_sequence(pattern, (48, 64), 13, False, -1, 0, -1, 2, fps=24, start=5)
    assert e.value.args[0] == (pattern, 24, 5) and e.value.args[1] == video_io.sample_frame_indices(97, 24.0, 13, -1, 0, -1, 2).tolist()
    for name in ("v.mp4", "v.gif", "v"):
        with pytest.raises(ValueError, match="Motion-JPEG .avi"):
            video_io.load_video(str(tmp_path / name), (48, 64), 13, False, -1, 0, -1, 1)


def test_c_abi_validates_before_any_launch():
    """one argument wrong at a time; the calls never reach a launch"""
    from tokensgen_amd import kernels as K
    from tokensgen_amd import lib as L
    lib = L.load()
    err = lambda: lib.tg_last_error_string().decode()
    buf = ctypes.create_string_buffer(16384)
    p = ctypes.addressof(buf) + (16 - ctypes.addressof(buf) % 16)
    geo = lib.tg_png_decode_geometry
    assert tuple(geo(480, 720, 3, w) for w in range(5)) == (2161, 480 * 2161, 64, 65536, 0) and geo(1, 21844, 4, 0) == 87377
    assert geo(0, 8, 3, 0) == geo(8, 0, 3, 0) == geo(8, 8, 2, 0) == geo(8, 8, 5, 0) == geo(65535, 21844, 3, 0) == 0
    assert set(K.PNG_STATUS) == {1 << k for k in range(10)} and K.PNG_INFLATE_MODES == {"stream": 0, "chunk_size": 1, "chunk_write": 2}
    inf = dict(data=p, data_bytes=100, piece_begin=p + 1024, piece_end=p + 2048, piece_frame=p + 3072, piece_last=p + 4096, pieces=2, mode=2, piece_at=p + 5120,
               filtered=p + 6144, F=1, H=4, W=4, bpp=3, piece_bytes=p + 7168, adler3=p + 8192, status=p + 9216, stream=None)
    call = lambda **kw: lib.tg_png_inflate(*{**inf, **kw}.values())
    for name in ("data", "piece_begin", "piece_end", "piece_frame", "piece_last", "filtered", "status", "piece_at", "adler3"):
        assert call(**{name: None}) == -1 and "null pointer" in err(), name
    assert call(mode=1, piece_bytes=None) == -1 and call(mode=0, adler3=None) == -1 and "null pointer" in err()
    assert call(mode=-1) == -1 and call(mode=3) == -1 and "mode must be" in err()
    assert call(F=0) == -2 and call(pieces=0) == -2 and call(F=3) == -2 and call(data_bytes=0) == -2 and call(H=0) == -2 and call(W=0) == -2 and call(bpp=2) == -2
    assert call(H=65535, W=21844) == -2 and "below 2^31" in err()
    assert call(piece_begin=p + 1028) == -3 and call(piece_at=p + 5124) == -3 and call(piece_frame=p + 3073) == -3 and call(status=p + 9218) == -3 and "8-byte" in err()
    unf = dict(filtered=p, F=1, H=4, W=4, bpp=4, frame_first=p + 1024, adler3=p + 2048, expect=p + 3072, status=p + 4096, rgb=p + 5120, stream=None)
    call = lambda **kw: lib.tg_png_unfilter(*{**unf, **kw}.values())
    for name in ("filtered", "frame_first", "adler3", "expect", "status", "rgb"):
        assert call(**{name: None}) == -1 and "null pointer" in err(), name
    assert call(F=0) == -2 and call(H=0) == -2 and call(W=-1) == -2 and call(bpp=1) == -2 and "3 or 4" in err()
    assert call(frame_first=p + 1025) == -3 and call(expect=p + 3074) == -3 and "4-byte" in err()


# ---- the decoder as a host program under the sanitizers --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ for the host build of csrc/png_inflate.h")
    exe = tmp_path_factory.mktemp("png_inflate_host") / "png_inflate_host"
    r = subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + os.path.join(ROOT, "tokensgen_amd", "csrc"), os.path.join(ROOT, "tests", "csrc", "png_inflate_host.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(jobs):
        """jobs: (kind, file) -> per job (status after the pieces, bytes per piece, filtered or None, final status, rgb or None); the sanitizers must stay silent"""
        blob = struct.pack("<I", len(jobs))
        for kind, data in jobs:
            H, W, ct, idat = R.read_container(data)
            z = b"".join(idat)
            if kind == 0:
                pieces = [z[2:-4]]
            else:
                pieces = [p[(2 if k == 0 else 0):len(p) - (4 if k == len(idat) - 1 else 0)] for k, p in enumerate(idat)]
            blob += struct.pack("<6I", kind, H, W, 3 if ct == 2 else 4, struct.unpack(">I", z[-4:])[0], len(pieces))
            blob += b"".join(struct.pack("<I", len(p)) + p for p in pieces)
        path = exe.parent / "jobs.bin"
        path.write_bytes(blob)
        r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-3000:])
        lines, out = iter(r.stdout.splitlines()), []
        for _ in jobs:
            rec = []
            for word in ("inflate", "filtered", "final", "rgb"):
                head, *rest = next(lines).split()
                assert head == word
                rec.append(rest)
            blob_of = lambda v: None if v == ["-"] else bytes.fromhex(v[0])
            out.append((int(rec[0][0]), [int(v) for v in rec[0][1:]], blob_of(rec[1]), int(rec[2][0]), blob_of(rec[3])))
        assert next(lines, None) is None
        return out

    return run


def test_host_program_equals_the_restatement_on_every_case(host_program):
    """bytes, sizes and status of csrc/png_inflate.h are the restatement's on every clean and every damaged case, and the sanitizers see nothing"""
    cases = C.all_cases()
    for case, (st, produced, filtered, final, rgb) in zip(cases, host_program([(0, c.data) for c in cases])):
        H, W, ct, idat = R.read_container(case.data)
        z = b"".join(idat)
        want, want_st = R.inflate(z, H * (1 + (3 if ct == 2 else 4) * W), 2, len(z) - 4)
        assert st == want_st and produced == [len(want)], case.name
        assert final == case.status, case.name
        if case.frame is not None:
            assert filtered == want and rgb == case.frame.tobytes(), case.name
        elif st == 0 and final == R.BAD_FILTER:
            assert rgb == R.unfilter(want, H, W, 3)[0].tobytes(), case.name


def test_host_program_chunk_route(host_program):
    """our own files and a full-flushed stream decode piece by piece; a sync-flushed one is reported not independent, and so is a damaged piece"""
    frame = np.tile(C.smooth(8, 47, seed=3), (4, 1, 1))
    own = [png_ref.encode_png(f, rows_per_block=r) for f, r in ((C.smooth(33, 47, seed=1), 3), (C.noise(33, 47, seed=2), None), (frame, 1))]
    full = R.write_png(frame, [y % 5 for y in range(32)], flush=zlib.Z_FULL_FLUSH, pieces=4)
    sync = R.write_png(frame, [0] * 32, flush=zlib.Z_SYNC_FLUSH, pieces=4)
    hurt = bytearray(own[0])
    at = own[0].index(b"IDAT", own[0].index(b"IDAT") + 4) + 9
    hurt[at] ^= 0x40
    hurt = rechunk(bytes(hurt), lambda c: c)                                    # the CRCs again
    files = own + [full, sync, hurt]
    for data, (st, produced, filtered, final, rgb) in zip(files, host_program([(1, d) for d in files])):
        want, want_st = R.decode_chunks(data)
        assert bool(st) == bool(want_st) and (st == 0 or st & R.NOT_INDEPENDENT)
        if want_st == 0:
            H, W, _, _ = R.read_container(data)
            assert filtered == want and final == 0 and rgb == R.decode(data)[0].tobytes() and sum(produced) == len(want)
    assert R.decode_chunks(sync)[1] and R.decode_chunks(hurt)[1] and not R.decode_chunks(full)[1]
