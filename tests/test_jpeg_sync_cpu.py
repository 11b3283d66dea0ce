"""CPU: the self-synchronising entropy decoder of csrc/jpeg_entropy_sync.h as a host program under the address and undefined-behaviour sanitizers
(tests/csrc/jpeg_sync_host.cpp emulates the lanes of csrc/jpeg_decode_sync.hip round by round), on valid and on damaged streams; tokensgen_amd.jpeg.entropy_plan;
the argument validation of tg_jpeg_decode_coeffs_sync before any launch; decode_jpeg's refusal of an unknown `entropy`.  tests/jpeg_dec_ref.py is the expected value.

The bounds are the algorithm's own: the coefficients are the serial decoder's, bit for bit; a valid stream is vouched for (clean = 1: nothing is left to the
fallback); rounds lie in 1 .. lanes of a chunk; clean = 0 wherever the serial decoder reports anything."""
import ctypes
import io
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import jpeg_dec_ref as D
import jpeg_ref as R
from tokensgen_amd import jpeg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUBS = ["420", "444"]
CONFIGS = [(16, 64), (16, 1024), (128, 64), (128, 1024)]                        # (sub_bytes, lanes)


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ for the host build of csrc/jpeg_entropy_sync.h")
    exe = tmp_path_factory.mktemp("jpeg_sync_host") / "jpeg_sync_host"
    r = subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + os.path.join(ROOT, "tokensgen_amd", "csrc"), os.path.join(ROOT, "tests", "csrc", "jpeg_sync_host.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(jobs):
        """jobs: (blocks per MCU, MCUs, print, sub_bytes, lanes, the three (DC, AC) table pairs, segment bytes) -> per job a dict of the verdict line's figures, with
        "coef" int [MCUs, blocks per MCU, 64] where print was asked for; the sanitizers must stay silent and the program must return"""
        blob = struct.pack("<I", len(jobs))
        for bpm, mcus, show, sub_bytes, lanes, huff, seg in jobs:
            blob += struct.pack("<IIIII", bpm, mcus, show, sub_bytes, lanes)
            for pair in huff:
                for bits, vals in pair:
                    blob += bytes(bits) + struct.pack("<I", len(vals)) + bytes(vals)
            blob += struct.pack("<I", len(seg)) + bytes(seg)
        path = exe.parent / "jobs.bin"
        path.write_bytes(blob)
        r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-3000:])
        lines, out = iter(r.stdout.splitlines()), []
        for bpm, mcus, show, *_ in jobs:
            words = next(lines).split()
            got = {k: int(v) for k, v in zip(words[0::2], words[1::2])}
            assert sorted(got) == ["chunks", "clean", "multi", "rounds", "same", "serial"]
            if show:
                got["coef"] = np.array([[int(v) for v in next(lines).split()] for _ in range(mcus * bpm)]).reshape(mcus, bpm, 64)
            out.append(got)
        assert next(lines, None) is None
        return out

    return run


def segments_of(s):
    """(blocks per MCU, MCUs, tables, bytes) per restart segment of the frame s, cut where tg_jpeg_find_segments cuts, and its status bits"""
    info = jpeg.parse_jpeg(s)
    _, bpm, rows, cols = R.geometry(info.height, info.width, info.subsampling)
    total = rows * cols
    r = min(info.restart_interval or total, total)
    n_seg = -(-total // r)
    begins, ends, status = D.device_segments(s, *info.scan, n_seg)
    return [(bpm, min((k + 1) * r, total) - k * r, info.huffman, s[b:e]) for k, (b, e) in enumerate(zip(begins, ends))], status


def split_pairs(seg, sub_bytes):
    """FF | 00 pairs that a subsequence boundary splits: the 00 is a subsequence's first byte"""
    return sum(1 for p in range(sub_bytes, len(seg), sub_bytes) if seg[p] == 0 and seg[p - 1] == 0xff)


def pillow_stream(a, **kw):
    from PIL import Image
    bio = io.BytesIO()
    Image.fromarray(a).save(bio, "JPEG", **kw)
    return bio.getvalue()


def check_valid(host_program, streams, configs=CONFIGS):
    """every segment of every stream at every (sub_bytes, lanes): the restatement's coefficients (printed at the first configuration, equal to jd_decode_segment's at
    all), clean = 1, rounds in 1 .. lanes wherever a chunk has more than one subsequence (the program itself refuses a chunk outside that)"""
    jobs, owner = [], []
    for n, s in enumerate(streams):
        segs, status = segments_of(s)
        assert status == 0
        for c, (sub_bytes, lanes) in enumerate(configs):
            for k, (bpm, mcus, huff, seg) in enumerate(segs):
                jobs.append((bpm, mcus, int(c == 0), sub_bytes, lanes, huff, seg))
                owner.append((n, c, k))
    got = host_program(jobs)
    printed = {}
    for (n, c, k), job, res in zip(owner, jobs, got):
        sub_bytes, lanes, seg = job[3], job[4], job[6]
        assert res["serial"] == 0 and res["same"] == 1 and res["clean"] == 1, (n, c, k, res)       # clean = 1: no valid stream is left to the fallback
        assert res["chunks"] == -(-len(seg) // (sub_bytes * lanes))
        if len(seg) > sub_bytes:
            assert res["multi"] >= 1 and 1 <= res["rounds"] <= min(lanes, -(-len(seg) // sub_bytes)), (n, c, k, res)
        else:
            assert res["rounds"] == 1
        if c == 0:
            printed.setdefault(n, []).append(res["coef"])
    for n, s in enumerate(streams):
        assert np.array_equal(np.concatenate(printed[n]), D.decode(s).coef), n
    return got, jobs


def test_valid_streams(host_program):
    """item 1 of the issue: our streams as one segment and as one MCU row per segment, Pillow's optimised tables, the flat frame, noise"""
    streams = []
    for h, w in ((9, 7), (33, 47), (120, 184)):
        a = R.sample_image(h, w)
        for sub in SUBS:
            for q in (50, 100):
                for ri in (65535, R.geometry(h, w, sub)[3]):
                    streams.append(R.encode(a, q, sub, ri))
    rng = np.random.default_rng(0)
    noise = rng.integers(0, 256, (120, 184, 3), dtype=np.uint8)
    flat = np.full((120, 184, 3), 77, np.uint8)
    for sub in SUBS:
        streams += [R.encode(noise, 90, sub, 65535), R.encode(flat, 90, sub, 65535)]
    try:
        for a in (R.sample_image(120, 184), noise, flat, R.sample_image(33, 47)):
            for code in (0, 2):
                streams.append(pillow_stream(a, quality=85, subsampling=code, optimize=True))
        streams.append(pillow_stream(R.sample_image(120, 184), quality=85))
    except ImportError:
        pass
    got, jobs = check_valid(host_program, streams)
    print("rounds, most per configuration:", {cfg: max(r["rounds"] for r, j in zip(got, jobs) if (j[3], j[4]) == cfg) for cfg in CONFIGS})


def test_split_stuffing_pairs_both_endings_and_chunking(host_program):
    """items 2 - 4: FF | 00 pairs split by a subsequence boundary (counted from the bytes, at least one at both sizes and both subsamplings); a stream that ends in
    padding bits and one that ends on a byte boundary; a scan of at least three chunks at sub_bytes 16 for any lane count up to 1024"""
    a = R.sample_image(120, 184)
    streams = [R.encode(a, 100, sub, 65535) for sub in SUBS]
    for s in streams:
        (_, _, _, seg), = segments_of(s)[0]
        for sub_bytes in (16, 128):
            assert split_pairs(seg, sub_bytes) >= 1, sub_bytes
    (_, _, _, seg), = segments_of(streams[1])[0]
    assert len(seg) >= 3 * 16 * 1024                                            # 4:4:4, quality 100: three chunks of 1024 lanes at 16 bytes
    got, jobs = check_valid(host_program, streams)
    assert all(r["chunks"] >= 3 for r, j in zip(got, jobs) if j[3] == 16 and len(j[6]) == len(seg))
    # the endings, from the bytes: the restated bit count of the scan against its length
    def padding_bits(s):
        (bpm, mcus, huff, seg), = segments_of(s)[0]
        raw = seg.replace(b"\xff\x00", b"\xff")
        luts = [(D.lookup(*dc), D.lookup(*ac)) for dc, ac in huff]
        w, pos = D._windows(raw), 0
        for _ in range(mcus):
            for k in range(bpm):
                dc, ac = luts[0 if k < bpm - 2 else k - (bpm - 3)]
                e = dc[w[pos]]
                pos += (e >> 8) + (e & 255)
                i = 1
                while i < 64:
                    e = ac[w[pos]]
                    pos += (e >> 8) + (e & 15)
                    if e & 255 == 0:
                        break
                    i += 16 if e & 255 == 0xf0 else ((e & 255) >> 4) + 1
        return 8 * len(raw) - pos
    whole = R.encode(a, 50, "444", 65535)
    padded = R.encode(a, 50, "420", 65535)
    assert padding_bits(whole) == 0 and 1 <= padding_bits(padded) <= 7
    check_valid(host_program, [whole, padded])


def test_damaged_streams(host_program):
    """item 5: the three damaged frames of jpeg_dec_ref and the 200 seeded single-byte changes of the sibling test, at both subsequence sizes: clean is 0 whenever
    the serial status is non-zero, wherever clean is 1 the coefficients are the serial decoder's, the sanitizers stay silent and the program returns"""
    s = R.encode(R.sample_image(33, 47), 90, "420", 65535)
    info = jpeg.parse_jpeg(s)
    b, e = info.scan
    rng = np.random.default_rng(0)
    jobs = []
    for _ in range(200):
        p, v = int(rng.integers(b, e)), int(rng.integers(0, 256))
        while v == s[p]:
            v = int(rng.integers(0, 256))
        for sub_bytes, lanes in ((16, 8), (128, 1024)):                         # 8 lanes: the 33 x 47 scan is several chunks
            jobs.append((6, 9, 0, sub_bytes, lanes, info.huffman, s[b:p] + bytes([v]) + s[p + 1:e]))
    for cut in (e - 2, (b + e) // 2, b + 1, b):
        jobs.append((6, 9, 0, 16, 8, info.huffman, s[b:cut]))
    for name, (bad, want, ri) in D.damaged_streams().items():
        segs, status = segments_of(bad)
        for bpm, mcus, huff, seg in segs:
            for sub_bytes, lanes in ((16, 8), (128, 1024)):
                jobs.append((bpm, mcus, 0, sub_bytes, lanes, huff, seg))
    got = host_program(jobs)
    bad = sum(1 for r in got if r["serial"])
    print(f"{len(got)} damaged segments: serial status non-zero in {bad}, clean in {sum(r['clean'] for r in got)}, "
          f"sound to the serial decoder but not vouched for in {sum(1 for r in got if not r['serial'] and not r['clean'])}")
    assert bad >= 40
    for r, j in zip(got, jobs):
        assert not (r["serial"] and r["clean"]), (r, j[3:5])
        assert not r["clean"] or r["same"], (r, j[3:5])
    # the three damaged frames: a segment of each is refused by both decoders
    at = 2 * 200 + 4
    for name, (bad, want, ri) in D.damaged_streams().items():
        n = 2 * len(segments_of(bad)[0])
        if want & 0xf:
            assert any(r["serial"] for r in got[at:at + n]) and not all(r["clean"] for r in got[at:at + n]), name
        at += n
    assert at == len(got)


def test_entropy_plan():
    """a pure function of the geometry: "sync" from SYNC_MIN_MCUS MCUs per segment on, and for every frame that is one segment of at least two MCUs"""
    assert jpeg.SYNC_SUB_BYTES in (64, 128, 256) and jpeg.SYNC_MIN_MCUS >= 2
    assert jpeg.entropy_plan(480, 720, "420", 0) == ("sync", jpeg.SYNC_SUB_BYTES) == jpeg.entropy_plan(480, 720, "444", 0)
    assert jpeg.entropy_plan(480, 720, "420", 65535) == ("sync", jpeg.SYNC_SUB_BYTES)          # an interval of more than the frame's 1350 MCUs: one segment
    assert jpeg.entropy_plan(480, 720, "420", 1) == ("segment", None)
    assert jpeg.entropy_plan(33, 47, "420", 0) == ("sync", jpeg.SYNC_SUB_BYTES)                # nine MCUs, no markers
    assert jpeg.entropy_plan(16, 16, "420", 0) == ("segment", None) == jpeg.entropy_plan(8, 8, "444", 0)      # one MCU: too small to cut
    assert jpeg.entropy_plan(16, 16, "444", 0) == ("sync", jpeg.SYNC_SUB_BYTES)                # four MCUs
    big = 16 * 4096
    assert jpeg.entropy_plan(big - 1, big - 1, "420", jpeg.SYNC_MIN_MCUS) == ("sync", jpeg.SYNC_SUB_BYTES)
    if jpeg.SYNC_MIN_MCUS > 2:
        assert jpeg.entropy_plan(big - 1, big - 1, "420", jpeg.SYNC_MIN_MCUS - 1) == ("segment", None)
    for bad in (-1, 65536, 1.5, True):
        with pytest.raises(ValueError, match="restart_interval"):
            jpeg.entropy_plan(480, 720, "420", bad)
    with pytest.raises(ValueError):
        jpeg.entropy_plan(480, 720, "422", 0)
    with pytest.raises(ValueError):
        jpeg.entropy_plan(0, 720, "420", 0)


def test_decode_jpeg_refuses_an_unknown_entropy():
    """before anything else, with or without a device"""
    s = R.encode(R.sample_image(9, 7), 50, "420", 1)
    for bad in ("parallel", None, 1, "SYNC"):
        with pytest.raises(ValueError, match="entropy must be one of"):
            jpeg.decode_jpeg([s], entropy=bad)
        with pytest.raises(ValueError, match="entropy must be one of"):
            jpeg.decode_jpeg([], entropy=bad)
    assert jpeg.ENTROPY_MODES == ("auto", "segment", "sync")


def test_c_abi_validates_before_any_launch():
    """one argument wrong at a time; the calls never reach a launch"""
    from tokensgen_amd import lib as L
    lib = L.load()
    err = lambda: lib.tg_last_error_string().decode()
    buf = ctypes.create_string_buffer(32768)
    p = ctypes.addressof(buf) + (16 - ctypes.addressof(buf) % 16)
    ws = lib.tg_jpeg_sync_ws_bytes
    assert ws(1, 480, 720, 420, 0) == 8 and ws(49, 480, 720, 420, 45) == 8 * 49 * 30 and ws(2, 33, 47, 444, 1) == 8 * 2 * 30
    assert ws(0, 8, 8, 420, 0) == ws(65536, 8, 8, 420, 0) == ws(1, 8, 8, 422, 0) == ws(1, 0, 8, 420, 0) == ws(1, 8, 8, 420, -1) == ws(1, 8, 8, 420, 65536) == 0
    args = dict(data=p, data_bytes=4096, seg_begin=p + 4096, seg_end=p + 4160, F=1, H=16, W=16, subsampling=420, restart_interval=0, htabs=p + 4224, n_sets=1,
                htab_index=p + 9800, sub_bytes=128, ws=p + 9808, ws_bytes=8, coef=p + 9856, clean=p + 9840, rounds=p + 9844, stream=None)
    call = lambda **kw: lib.tg_jpeg_decode_coeffs_sync(*{**args, **kw}.values())
    for name in ("data", "seg_begin", "seg_end", "htabs", "htab_index", "ws", "coef", "clean", "rounds"):
        assert call(**{name: None}) == -1 and "null pointer" in err(), name
    assert call(restart_interval=-1) == -1 and call(restart_interval=65536) == -1 and "0..65535" in err()
    assert call(n_sets=0) == -1 and "table set" in err()
    for bad in (0, 8, 15, 48, 100, 512, -128):
        assert call(sub_bytes=bad) == -1 and "16, 32, 64, 128 or 256" in err(), bad
    assert call(data_bytes=0) == -2 and call(F=0) == -2 and call(F=65536) == -2 and call(H=0) == -2 and call(W=65536) == -2 and call(subsampling=422) == -2 and "420 or 444" in err()
    assert call(ws_bytes=7) == -2 and "needs 8 bytes" in err() and call(restart_interval=1, ws_bytes=8 * 1 - 1) == -2
    assert call(coef=p + 9864) == -3 and call(seg_begin=p + 4100) == -3 and call(htabs=p + 4226) == -3 and call(clean=p + 9842) == -3 and call(rounds=p + 9846) == -3
    assert call(ws=p + 9810) == -3 and "16-byte" in err()
    assert "tg_jpeg_decode_coeffs_sync" in L.PROTOTYPES and "tg_jpeg_sync_ws_bytes" in L.QUERIES
