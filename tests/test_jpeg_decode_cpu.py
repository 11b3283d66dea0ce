"""CPU: the JPEG decoding definition as tests/jpeg_dec_ref.py restates it (it inverts tests/jpeg_ref.py's entropy coder exactly, its picture is Pillow's to a few
levels, three wrong rules change the picture), tokensgen_amd.jpeg.parse_jpeg with every refusal, the AVI reader on files made from restated frames, the index
arithmetic of video_io.load_video through a stub reader, the argument validation of the C entry points of csrc/jpeg_decode.hip (before any launch), and the shared
entropy decoder of csrc/jpeg_entropy_dec.h as a host program under the address and undefined-behaviour sanitizers, on valid and on damaged streams.

`python tests/test_jpeg_decode_cpu.py` measures the parity with Pillow's decoder on Pillow-encoded streams and writes profiles/jpeg_decode_parity.json, whose worst
level difference plus one is the bound of test_pillow_encoded_streams."""
import ctypes
import io
import json
import os
import shutil
import struct
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))          # for `python tests/test_jpeg_decode_cpu.py`; pytest has it already
import avi_ref
import jpeg_dec_ref as D
import jpeg_ref as R
from tokensgen_amd import jpeg, video_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY = os.path.join(ROOT, "profiles", "jpeg_decode_parity.json")
SIZES = [(16, 16), (9, 7), (33, 47), (48, 80), (120, 184)]
SUBS = ["420", "444"]
QUALITIES = [1, 50, 90, 100]


def psnr(a, b):
    return 10 * np.log10(255.0 ** 2 / max(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2), 1e-12))


def intervals(h, w, sub):
    return (1, 3, R.geometry(h, w, sub)[3], 65535)


def pil_decode(s):
    from PIL import Image
    return np.array(Image.open(io.BytesIO(s)).convert("RGB"))


def pillow_streams():
    """name -> bytes: what Pillow's encoder writes for the two sizes: default tables without markers, optimised tables, both subsamplings, restart markers where this
    Pillow has them"""
    from PIL import Image
    variants = {"default": {}, "optimize": dict(optimize=True), "444": dict(subsampling=0), "420": dict(subsampling=2), "444_optimize": dict(subsampling=0, optimize=True),
                "restart_blocks": dict(restart_marker_blocks=2), "restart_rows": dict(restart_marker_rows=1)}
    out = {}
    for h, w in ((33, 47), (120, 184)):
        a = R.sample_image(h, w)
        plain = None
        for name, kw in variants.items():
            bio = io.BytesIO()
            Image.fromarray(a).save(bio, "JPEG", quality=85, **kw)
            if name == "default":
                plain = bio.getvalue()
            elif name.startswith("restart") and bio.getvalue() == plain:       # a Pillow without that option ignores it
                continue
            out[f"{h}x{w}_{name}"] = bio.getvalue()
    return out


def measure_pillow_parity():
    res = {}
    for name, s in pillow_streams().items():
        mine, pil = D.decode(s).rgb, pil_decode(s)
        res[name] = {"worst_level_difference": int(np.abs(mine.astype(int) - pil.astype(int)).max()), "psnr_db": round(float(psnr(mine, pil)), 2)}
    return res


def test_the_restatement_inverts_the_encoder():
    """coefficients equal to jpeg_ref.coefficients for every restart interval, and one picture whatever the interval; parse_jpeg reads the same headers"""
    for h, w in SIZES:
        a = R.sample_image(h, w, seed=h)
        for sub in SUBS:
            for q in QUALITIES:
                want, pics = R.coefficients(a, q, sub), []
                for ri in intervals(h, w, sub):
                    s = R.encode(a, q, sub, ri)
                    d = D.decode(s)
                    assert np.array_equal(d.coef, want), (h, w, sub, q, ri)
                    pics.append(d.rgb)
                    info, hdr = jpeg.parse_jpeg(s), D.parse(s)
                    assert info[:5] == (h, w, sub, ri, hdr.scan) and info.huffman == hdr.huff
                    assert all(np.array_equal(np.array(x), y) for x, y in zip(info.qtables, hdr.q))
                assert pics[0].shape == a.shape and pics[0].dtype == np.uint8 and all(np.array_equal(pics[0], p) for p in pics[1:]), (h, w, sub, q)


def test_picture_against_pillows_decoder():
    """every pixel within 4 levels and PSNR >= 52 dB of Pillow's decode of the same stream (measured: 3 levels, 55.6 dB; the margin is for another libjpeg build's
    IDCT rounding).  The gap between the two decoders' PSNR to the source is printed, not asserted: it is below 0.15 dB except where that PSNR is itself
    above 50 dB (quality 100), where one level on a few pixels moves it by 0.3 dB"""
    pytest.importorskip("PIL.Image")
    worst, low, gap = 0, 1e9, 0.0
    for h, w in SIZES:
        a = R.sample_image(h, w)
        for sub in SUBS:
            for q in QUALITIES:
                s = R.encode(a, q, sub, 65535)
                mine, pil = D.decode(s).rgb, pil_decode(s)
                worst = max(worst, int(np.abs(mine.astype(int) - pil.astype(int)).max()))
                low = min(low, psnr(mine, pil))
                gap = max(gap, abs(psnr(a, mine) - psnr(a, pil)))
    print(f"worst level difference to Pillow's decoder: {worst}, lowest PSNR {low:.2f} dB, PSNR-to-source gap {gap:.3f} dB")
    assert worst <= 4 and low >= 52.0


def test_pillow_encoded_streams():
    """Pillow's own streams (no markers, optimised tables, both subsamplings, restart markers): parse_jpeg reads what the restatement reads, and the restated picture is
    Pillow's to the worst difference recorded in profiles/jpeg_decode_parity.json plus one level (3 + 1: after entropy decoding the arithmetic is that of
    test_picture_against_pillows_decoder)"""
    pytest.importorskip("PIL.Image")
    recorded = json.load(open(PARITY))
    bound = recorded["worst_level_difference"] + 1
    assert bound == 4
    streams = pillow_streams()
    assert {"33x47_default", "33x47_optimize", "120x184_444", "120x184_420"} <= set(streams)
    got = measure_pillow_parity()
    print({k: v["worst_level_difference"] for k, v in got.items()})
    for name, s in streams.items():
        info, hdr = jpeg.parse_jpeg(s), D.parse(s)
        assert info[:5] == hdr[:5] and info.huffman == hdr.huff, name
        assert got[name]["worst_level_difference"] <= bound, (name, got[name])
    assert jpeg.parse_jpeg(streams["33x47_optimize"]).huffman != jpeg.parse_jpeg(streams["33x47_default"]).huffman
    assert jpeg.parse_jpeg(streams["33x47_default"]).restart_interval == 0


def test_flat_frames_at_quality_100_decode_exactly():
    for v in (0, 255, 128, 77):
        for sub in SUBS:
            a = np.full((16, 24, 3), v, np.uint8)
            assert np.array_equal(D.decode(R.encode(a, 100, sub, 1)).rgb, a), (v, sub)


def test_idct_sums_fit_int32():
    """sum_u |A[u][x]| <= 31015; with d clamped to -2048 .. 2047 the first sum stays below 6.4e7 and the second below 1.93e9 + 32768 < 2^31, over the 64 sign patterns
    that push one output sample to its extreme, and by the triangle inequality for every input"""
    A = R.DCT_A
    assert int(np.abs(A).sum(0).max()) <= 31015                                 # the table's own column sums are 21641: the bound has room
    first = 31015 * 2048 + 512
    assert first <= 6.4e7
    assert 31015 * (first >> 10) <= 1.93e9 and 1.93e9 + 32768 < 2 ** 31
    for y in range(8):
        for x in range(8):
            for sign in (1, -1):
                pattern = sign * np.outer(A[:, y], A[:, x])                     # [v][u]: the sign of A[v][y] A[u][x]
                d = np.where(pattern >= 0, 2047, -2048).astype(np.int64)
                t = np.einsum("ux,vu->vx", A, d)
                assert np.abs(t).max() + 512 <= 6.4e7
                p = np.einsum("vy,vx->yx", A, (t + 512) >> 10)
                assert np.abs(p).max() + 32768 <= 1.93e9
    # the clamp is what holds the bound: a DC of 32767 times Q = 255 would not fit
    assert 31015 * 32767 * 255 > 2 ** 31


def test_three_wrong_rules_each_change_the_picture():
    a = R.sample_image(120, 184)
    s = R.encode(a, 90, "420", 3)
    good = D.decode(s)
    carried = D.decode(s, wrong="no_dc_reset")
    assert not np.array_equal(carried.coef, good.coef) and not np.array_equal(carried.rgb, good.rgb)
    whole = R.encode(a, 90, "420", 65535)
    assert np.array_equal(D.decode(whole, wrong="no_dc_reset").coef, D.decode(whole).coef)     # without a marker the rule has nothing to do
    assert not np.array_equal(D.decode(s, wrong="box").rgb, good.rgb)
    padded = D.decode(s, wrong="padded").rgb
    assert not np.array_equal(padded, good.rgb)
    assert np.array_equal(padded[:119, :183], good.rgb[:119, :183])             # only where the filter reaches the padding: the real chroma plane is 60 x 92 inside 64 x 96
    assert not np.array_equal(padded[:, 183], good.rgb[:, 183]) and not np.array_equal(padded[119], good.rgb[119])
    b = R.sample_image(48, 80)                                                  # whole MCUs: the padded plane is the real one
    sb = R.encode(b, 90, "420", 1)
    assert np.array_equal(D.decode(sb, wrong="padded").rgb, D.decode(sb).rgb)
    assert np.array_equal(D.decode(R.encode(b, 90, "444", 1), wrong="box").rgb, D.decode(R.encode(b, 90, "444", 1)).rgb)


def strip_dht(s):
    out, pos = bytearray(s[:2]), 2
    while s[pos + 1] != 0xda:
        ln = struct.unpack_from(">H", s, pos + 2)[0]
        if s[pos + 1] != 0xc4:
            out += s[pos:pos + 2 + ln]
        pos += 2 + ln
    return bytes(out) + s[pos:]


def test_frames_without_dht_use_the_annex_k_tables():
    for sub in SUBS:
        s = R.encode(R.sample_image(33, 47), 90, sub, 3)
        bare = strip_dht(s)
        assert len(bare) == len(s) - 4 * 2 - 2 * (19 + 12) - 2 * (19 + 162) and b"\xff\xc4" not in bare[:200]
        assert np.array_equal(D.decode(bare).rgb, D.decode(s).rgb)
        assert jpeg.parse_jpeg(bare).huffman == jpeg.parse_jpeg(s).huffman == D.parse(s).huff
    assert {k: (bytes(b), bytes(v)) for k, (b, v) in jpeg.STD_HUFFMAN.items()} == D.STD and list(jpeg.ZIGZAG) == R.ZIGZAG.tolist()


def replace_segment(s, marker, fn):
    """the stream with fn(payload) in place of the first segment of that marker"""
    pos = 2
    while s[pos + 1] != marker:
        pos += 2 + struct.unpack_from(">H", s, pos + 2)[0]
    ln = struct.unpack_from(">H", s, pos + 2)[0]
    new = fn(bytes(s[pos + 4:pos + 2 + ln]))
    return s[:pos + 2] + struct.pack(">H", len(new) + 2) + new + s[pos + 2 + ln:]


def test_parse_jpeg_refuses_by_name():
    Image = pytest.importorskip("PIL.Image")
    a = R.sample_image(33, 47)
    s = R.encode(a, 90, "420", 3)

    def pil(**kw):
        bio = io.BytesIO()
        kw.pop("image", Image.fromarray(a)).save(bio, "JPEG", quality=85, **kw)
        return bio.getvalue()

    refused = {"4:2:2 \\(2x1, 1x1, 1x1\\)": pil(subsampling=1), "SOF2 \\(progressive": pil(progressive=True), "1 component \\(grey scale\\)": pil(image=Image.fromarray(a[..., 0])),
               "4 components": pil(image=Image.fromarray(np.dstack([a, a[..., :1]]), "CMYK")),
               "SOF1": s.replace(b"\xff\xc0\x00\x11", b"\xff\xc1\x00\x11"), "SOF9 \\(arithmetic": s.replace(b"\xff\xc0\x00\x11", b"\xff\xc9\x00\x11"),
               "12-bit precision": s.replace(b"\xff\xc0\x00\x11\x08", b"\xff\xc0\x00\x11\x0c"),
               "16-bit DQT": replace_segment(s, 0xdb, lambda p: b"\x10" + b"".join(b"\0" + bytes([v]) for v in p[1:])),
               "more than one scan": replace_segment(s, 0xda, lambda p: b"\x01\x01\x00\x00\x3f\x00"),
               "more than one scan; ": s[:-2] + b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00\x00\xff\xd9",
               "Ss 0, Se 5": replace_segment(s, 0xda, lambda p: p[:7] + b"\x00\x05\x00"),
               "Adobe APP14 with transform 0": s[:2] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00" + s[2:],
               "DAC \\(arithmetic": s[:2] + b"\xff\xcc\x00\x04\x00\x10" + s[2:]}
    for match, stream in refused.items():
        with pytest.raises(NotImplementedError, match=match):
            jpeg.parse_jpeg(stream)
    # an Adobe segment with transform 1 (Y Cb Cr), APPn, COM and fill bytes before a marker are read over; bytes after EOI are ignored
    ok = s[:2] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x01" + b"\xff\xfe\x00\x05abc" + b"\xff\xff\xff" + s[3:] + b"trailing \xff\xd9 bytes"
    assert jpeg.parse_jpeg(ok)[:4] == (33, 47, "420", 3) and jpeg.parse_jpeg(ok).scan[1] - jpeg.parse_jpeg(ok).scan[0] == D.parse(s).scan[1] - D.parse(s).scan[0]
    filled = s[:-2] + b"\xff\xff\xff\xd9"                                        # fill bytes before EOI do not belong to the scan
    assert jpeg.parse_jpeg(filled).scan == D.parse(s).scan
    swapped = s.replace(b"\x03\x01\x22\x00\x02\x11\x01\x03\x11\x01", b"\x03\x52\x22\x00\x47\x11\x01\x09\x11\x01").replace(b"\x03\x01\x00\x02\x11\x03\x11", b"\x03\x52\x00\x47\x11\x09\x11")
    assert swapped != s and jpeg.parse_jpeg(swapped) == jpeg.parse_jpeg(s)      # component ids are free
    malformed = {"no SOI": s[1:], "runs past the end": s[:300], "quantisation table slot 1 is missing": replace_segment(s, 0xdb, lambda p: p).replace(
                     b"\xff\xdb\x00\x43\x01", b"\xff\xdb\x00\x43\x02"), "SOS before SOF": s.replace(b"\xff\xc0\x00\x11", b"\xff\xe5\x00\x11"),
                 "Huffman table slot": s.replace(b"\xff\xc4\x00\xb5\x11", b"\xff\xc4\x00\xb5\x12"), "the bytes end before SOS": s[:20],
                 "EOI before SOS": s[:20] + b"\xff\xd9", "expected a marker": s[:20] + b"\x00" + s[20:]}
    for match, stream in malformed.items():
        with pytest.raises(ValueError, match=f"frame 7: .*{match}"):
            jpeg.parse_jpeg(stream, 7)
    assert jpeg.parse_jpeg(s[:-40]).scan[1] == len(s) - 40                      # a scan cut short parses; the decoder reports it
    # what decode_jpeg refuses before it needs a device
    with pytest.raises(ValueError, match="frame 1 is 48 x 80"):
        jpeg.decode_jpeg([s, R.encode(R.sample_image(48, 80), 90, "420", 3)])
    with pytest.raises(ValueError, match="share size, subsampling and restart interval"):
        jpeg.decode_jpeg([s, R.encode(a, 90, "420", 1)])
    with pytest.raises(ValueError, match="frame 1: .*no SOI"):
        jpeg.decode_jpeg([s, b"junk"])
    with pytest.raises(ValueError, match="list of at least one"):
        jpeg.decode_jpeg([])
    import torch
    with pytest.raises(ValueError, match="needs `offsets`"):
        jpeg.decode_jpeg(torch.zeros(10, dtype=torch.uint8))
    with pytest.raises(ValueError, match="offsets must rise"):
        jpeg.decode_jpeg(torch.zeros(10, dtype=torch.uint8), [0, 11])
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU path"):
            jpeg.decode_jpeg([s])
    with pytest.raises(RuntimeError, match="no CPU path"):
        jpeg.decode_jpeg([s], device="cpu")


# ---- the AVI reader ------------------------------------------------------------------------------------------------------------------------------------------------

def restated_frames(n=4, size=(33, 47)):
    return [R.encode(R.sample_image(*size, seed), 90, "420", 1) for seed in range(n)]


def write_avi(path, frames, fps=8, size=(33, 47)):
    with jpeg.MJPEGWriter(path, fps) as w:
        w.write_jpegs(frames, *size)
    return path.read_bytes()


def rebuild(raw, chunks, index="relative", rec=False):
    """the file `raw` (MJPEGWriter's: 'movi' fourcc at 220) with these (fourcc, payload) chunks instead of its own; index "relative" (to the 'movi' fourcc), "absolute"
    (to the file) or None (no idx1); rec: the chunks wrapped in LIST 'rec ' pairs"""
    body, entries = bytearray(), []
    for i, (cc, payload) in enumerate(chunks):
        if rec and i % 2 == 0:
            group = chunks[i:i + 2]
            body += b"LIST" + struct.pack("<I", 4 + sum(8 + len(p) + (len(p) & 1) for _, p in group)) + b"rec "
        entries.append((cc, 4 + len(body), len(payload)))
        body += cc + struct.pack("<I", len(payload)) + payload + b"\0" * (len(payload) & 1)
    head = bytearray(raw[:224])
    head[216:220] = struct.pack("<I", 4 + len(body))
    idx = b""
    if index is not None:
        base = 220 if index == "absolute" else 0
        idx = b"idx1" + struct.pack("<I", 16 * len(entries)) + b"".join(cc + struct.pack("<III", 0x10, base + off, n) for cc, off, n in entries)
    out = bytes(head) + bytes(body) + idx
    return out[:4] + struct.pack("<I", len(out) - 8) + out[8:]


def test_avi_reader_on_restated_frames(tmp_path):
    frames = restated_frames()
    raw = write_avi(tmp_path / "a.avi", frames)
    walked = avi_ref.walk(raw)
    with jpeg.MJPEGReader(tmp_path / "a.avi") as r:
        assert len(r) == r.frames == 4 and r.size == (33, 47) and r.fps == Fraction(8) and r.get_avg_fps() == 8.0
        assert [(p - 8 - walked.movi, n) for p, n in r._entries] == [(off, n) for _, off, n in walked.index]          # its index is the walker's
        assert r.frame_bytes(range(4)) == walked.frames == frames
        assert r.frame_bytes([3, 0, 3, -1]) == [frames[3], frames[0], frames[3], frames[3]]
        with pytest.raises(IndexError):
            r.frame_bytes([4])
    with pytest.raises(ValueError, match="closed"):
        r.frame_bytes([0])
    for fps in (8, 29.97, Fraction(30000, 1001)):
        write_avi(tmp_path / "f.avi", frames[:1], fps)
        with jpeg.MJPEGReader(tmp_path / "f.avi") as r:
            assert r.fps == Fraction(fps).limit_denominator(65535) and abs(r.get_avg_fps() - float(fps)) < 1e-9
    video = [(b"00dc", f) for f in frames]
    audio = (b"01wb", b"\1\2\3\4\5")
    variants = {"no idx1": rebuild(raw, video, index=None), "absolute idx1": rebuild(raw, video, index="absolute"),
                "audio, indexed": rebuild(raw, [video[0], audio, video[1], audio, video[2], video[3]]),
                "audio, walked": rebuild(raw, [video[0], audio, video[1], audio, video[2], video[3]], index=None),
                "rec lists": rebuild(raw, [video[0], audio, video[1], audio, video[2], audio, video[3], audio], index=None, rec=True),
                "uncompressed tag": rebuild(raw, [(b"00db", f) for f in frames])}
    for name, data in variants.items():
        (tmp_path / "v.avi").write_bytes(data)
        with jpeg.MJPEGReader(tmp_path / "v.avi") as r:
            assert r.frame_bytes(range(len(r))) == frames, name
    # a zero-length chunk repeats the frame before it; as the first frame it is an error
    (tmp_path / "z.avi").write_bytes(rebuild(raw, [video[0], (b"00dc", b""), video[1], (b"00dc", b"")]))
    with jpeg.MJPEGReader(tmp_path / "z.avi") as r:
        assert r.frame_bytes(range(len(r))) == [frames[0], frames[0], frames[1], frames[1]]
    for index in ("relative", None):
        (tmp_path / "z.avi").write_bytes(rebuild(raw, [(b"00dc", b""), video[0]], index=index))
        with pytest.raises(ValueError, match="zero-length"):
            jpeg.MJPEGReader(tmp_path / "z.avi")
    # letter case of the codec; another codec; another stream type first
    lower = raw.replace(b"vidsMJPG", b"vidsmjpg").replace(b"\x18\x00MJPG", b"\x18\x00mjpg")
    assert lower != raw and lower.count(b"MJPG") == 0
    (tmp_path / "l.avi").write_bytes(lower)
    with jpeg.MJPEGReader(tmp_path / "l.avi") as r:
        assert r.frame_bytes([2]) == [frames[2]]
    (tmp_path / "h.avi").write_bytes(raw.replace(b"vidsMJPG", b"vidsH264").replace(b"\x18\x00MJPG", b"\x18\x00H264"))
    with pytest.raises(NotImplementedError, match="H264"):
        jpeg.MJPEGReader(tmp_path / "h.avi")
    (tmp_path / "s.avi").write_bytes(raw.replace(b"vidsMJPG", b"audsMJPG"))
    with pytest.raises(NotImplementedError, match="no video stream"):
        jpeg.MJPEGReader(tmp_path / "s.avi")
    # truncation, with and without the index
    for cut in (len(raw) - 30, len(raw) - 16 * 4 - 8 - 100, 300, 100, 10):
        (tmp_path / "t.avi").write_bytes(raw[:cut])
        with pytest.raises(ValueError, match="truncated"):
            jpeg.MJPEGReader(tmp_path / "t.avi")
    walked_only = rebuild(raw, video, index=None)
    (tmp_path / "t.avi").write_bytes(walked_only[:4] + struct.pack("<I", len(walked_only) - 108) + walked_only[8:-100])
    with pytest.raises(ValueError, match="truncated"):
        jpeg.MJPEGReader(tmp_path / "t.avi")
    (tmp_path / "n.avi").write_bytes(b"RIFF" + struct.pack("<I", 4) + b"WAVE")
    with pytest.raises(ValueError, match="not a RIFF 'AVI ' file"):
        jpeg.MJPEGReader(tmp_path / "n.avi")
    # OpenDML, by name
    (tmp_path / "o.avi").write_bytes(raw + b"RIFF" + struct.pack("<I", 4) + b"AVIX")
    with pytest.raises(NotImplementedError, match="OpenDML.*AVIX"):
        jpeg.MJPEGReader(tmp_path / "o.avi")
    (tmp_path / "o.avi").write_bytes(rebuild(raw, video + [(b"ix00", b"\0" * 32)], index=None))
    with pytest.raises(NotImplementedError, match="OpenDML.*ix00"):
        jpeg.MJPEGReader(tmp_path / "o.avi")
    strl_end = raw.index(b"LIST", 12 + 8 + 4 + 8 + 56)                           # the strl list: its size grows by an 'indx' chunk
    grown = bytearray(raw[:212] + b"indx" + struct.pack("<I", 8) + b"\0" * 8 + raw[212:])
    for at in (4, 16, strl_end + 4):
        grown[at:at + 4] = struct.pack("<I", struct.unpack_from("<I", grown, at)[0] + 16)
    (tmp_path / "o.avi").write_bytes(bytes(grown))
    with pytest.raises(NotImplementedError, match="OpenDML.*indx"):
        jpeg.MJPEGReader(tmp_path / "o.avi")


def test_load_video_index_arithmetic_through_a_stub_reader(monkeypatch, tmp_path):
    """load_video asks the reader for exactly sample_frame_indices(len, avg_fps, ...); any suffix but .avi is refused by name"""
    import inspect

    class Asked(Exception):
        pass

    class Stub:
        def __init__(self, path, device=None):
            self.path = path

        def __len__(self):
            return 97

        def get_avg_fps(self):
            return 24.0

        def get_batch(self, indices):
            raise Asked(list(indices))

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return False

    monkeypatch.setattr(jpeg, "MJPEGReader", Stub)
    for nf, fps, t0, t1, chunks in ((13, -1, 0, -1, 1), (13, 12, 0, -1, 3), (8, 8, 1.0, 3.5, 2), (49, -1, 0, -1, 1), (5, 6.5, 0.5, 100, 4)):
        with pytest.raises(Asked) as e:
            video_io.load_video(str(tmp_path / "clip.AVI"), (48, 64), nf, False, fps, t0, t1, chunks)
        want = video_io.sample_frame_indices(97, 24.0, nf, fps, t0, t1, chunks)
        assert e.value.args[0] == want.tolist() and all(isinstance(i, int) for i in e.value.args[0])
    with pytest.raises(AssertionError):
        video_io.load_video(str(tmp_path / "clip.avi"), (48, 64), 13, False, -1, 5.0, 4.0, 1)
    for name in ("v.mp4", "v.gif", "v"):
        with pytest.raises(ValueError, match="Motion-JPEG .avi"):
            video_io.load_video(str(tmp_path / name), (48, 64), 13, False, -1, 0, -1, 1)
    assert list(inspect.signature(video_io.load_video).parameters) == ["video_path", "output_res", "nf_per_chunk", "pad_to_fit", "sample_fps", "start_t", "end_t",
                                                                       "max_num_chunks", "crop_to_fit", "device"]
    assert inspect.signature(video_io.load_video).parameters["crop_to_fit"].default is False


def test_c_abi_validates_before_any_launch():
    """one argument wrong at a time; the calls never reach a launch"""
    from tokensgen_amd import kernels as K
    from tokensgen_amd import lib as L
    lib = L.load()
    err = lambda: lib.tg_last_error_string().decode()
    buf = ctypes.create_string_buffer(16384)
    p = ctypes.addressof(buf) + (16 - ctypes.addressof(buf) % 16)
    assert lib.tg_jpeg_huff_table_bytes() == 912
    seg = lib.tg_jpeg_decode_segments
    assert (seg(480, 720, 420, 1), seg(480, 720, 420, 45), seg(480, 720, 420, 0), seg(480, 720, 444, 65535), seg(33, 47, 420, 2)) == (1350, 30, 1, 1, 5)
    assert seg(0, 8, 420, 1) == seg(8, 8, 422, 1) == seg(8, 8, 420, -1) == seg(8, 8, 420, 65536) == 0
    ws = lib.tg_jpeg_idct_ws_bytes
    assert ws(1, 33, 47, 420) == 48 * 48 + 2 * 24 * 24 and ws(2, 33, 47, 444) == 2 * 3 * 40 * 48 and ws(0, 8, 8, 420) == ws(1, 8, 8, 411) == 0
    # the table builder, a pure host function
    table = K.jpeg_huff_table(*jpeg.STD_HUFFMAN[0x10])
    assert len(table) == 912
    maxcode, valoff = struct.unpack_from("<18i", table, 0), struct.unpack_from("<18i", table, 72)
    look, vals = struct.unpack_from("<256H", table, 144), table[656:]
    codes = R.HUFF[0][1]
    assert maxcode[2] == 1 and maxcode[1] == -1 and maxcode[16] == 0xfffe and maxcode[17] == 0x7fffffff and vals[:162] == bytes(R.AC_VALS[0])
    for sym, (code, n) in codes.items():
        assert vals[code + valoff[n]] == sym and code <= maxcode[n]
        if n <= 8:
            assert all(look[(code << (8 - n)) + j] == (n << 8 | sym) for j in range(1 << (8 - n)))
    assert sum(1 for e in look if e == 0) == 256 - sum((1 << (8 - n)) for _, n in codes.values() if n <= 8)
    with pytest.raises(ValueError, match="over-subscribed"):
        K.jpeg_huff_table(bytes([3] + [0] * 15), bytes([0, 1, 2]))
    with pytest.raises(ValueError, match="over-subscribed"):
        K.jpeg_huff_table(bytes([1, 1, 3] + [0] * 13), bytes(range(5)))
    with pytest.raises(ValueError, match="do not add up"):
        K.jpeg_huff_table(bytes([0, 2] + [0] * 14), bytes([0, 1, 2]))
    with pytest.raises(ValueError, match="16 counts"):
        K.jpeg_huff_table(bytes([0, 2]), bytes([0, 1]))
    assert lib.tg_jpeg_huff_table(None, None, 0, None) == -1 and lib.tg_jpeg_huff_table(p, p, 0, p + 2) == -3
    fs = dict(data=p, data_bytes=4096, scan_begin=p + 4096, scan_end=p + 4160, F=1, n_seg=3, seg_begin=p + 4224, seg_end=p + 4352, status=p + 4480, stream=None)
    call = lambda **kw: lib.tg_jpeg_find_segments(*{**fs, **kw}.values())
    for name in ("data", "scan_begin", "scan_end", "seg_begin", "seg_end", "status"):
        assert call(**{name: None}) == -1 and "null pointer" in err()
    assert call(data_bytes=0) == -2 and call(F=0) == -2 and call(F=65536) == -2 and call(n_seg=0) == -2 and "n_seg=0" in err()
    assert call(scan_begin=p + 4100) == -3 and call(seg_end=p + 4356) == -3 and call(status=p + 4482) == -3 and "8-byte" in err()
    dc = dict(data=p, data_bytes=4096, seg_begin=p + 4096, seg_end=p + 4160, F=1, H=16, W=16, subsampling=420, restart_interval=1, htabs=p + 4224, n_sets=1,
              htab_index=p + 9800, coef=p + 9856, status=p + 9840, stream=None)
    call = lambda **kw: lib.tg_jpeg_decode_coeffs(*{**dc, **kw}.values())
    for name in ("data", "seg_begin", "seg_end", "htabs", "htab_index", "coef", "status"):
        assert call(**{name: None}) == -1 and "null pointer" in err()
    assert call(restart_interval=-1) == -1 and call(restart_interval=65536) == -1 and "0..65535" in err()
    assert call(n_sets=0) == -1 and "table set" in err()
    assert call(data_bytes=0) == -2 and call(F=0) == -2 and call(F=65536) == -2 and call(H=0) == -2 and call(W=65536) == -2 and call(subsampling=422) == -2 and "420 or 444" in err()
    assert call(coef=p + 9864) == -3 and call(seg_begin=p + 4100) == -3 and call(htabs=p + 4226) == -3 and call(status=p + 9842) == -3 and "16-byte" in err()
    ir = dict(coef=p, F=1, H=16, W=16, subsampling=420, qtabs=p + 1024, n_qsets=1, qtab_index=p + 2048, ws=p + 4096, ws_bytes=384, rgb=p + 8192, rgb_bytes=768, stream=None)
    call = lambda **kw: lib.tg_jpeg_idct_rgb(*{**ir, **kw}.values())
    for name in ("coef", "qtabs", "qtab_index", "ws", "rgb"):
        assert call(**{name: None}) == -1 and "null pointer" in err()
    assert call(n_qsets=0) == -1
    assert call(F=0) == -2 and call(H=65536) == -2 and call(subsampling=0) == -2
    assert call(ws_bytes=383) == -2 and "needs 384 bytes" in err() and call(rgb_bytes=0) == -2
    assert call(coef=p + 8) == -3 and call(ws=p + 4100) == -3 and call(qtab_index=p + 2050) == -3 and call(qtabs=p + 1025) == -3
    # the status bits of the header are the restatement's and the wrapper's texts
    hdr = open(os.path.join(ROOT, "include", "tokensgen_hip.h")).read()
    import re
    bits = {name: int(v) for name, v in re.findall(r"#define TG_JPEG_ST_([A-Z_]+) (\d+)", hdr)}
    assert bits == {"INVALID_CODE": D.ST_INVALID_CODE, "COEF_INDEX": D.ST_COEF_INDEX, "CATEGORY": D.ST_CATEGORY, "OUT_OF_BITS": D.ST_OUT_OF_BITS,
                    "RST_COUNT": D.ST_RST_COUNT, "RST_NUMBER": D.ST_RST_NUMBER, "RANGE": D.ST_RANGE} and sorted(K.JPEG_STATUS) == sorted(bits.values())


# ---- the shared entropy decoder as a host program under the sanitizers ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ for the host build of csrc/jpeg_entropy_dec.h")
    exe = tmp_path_factory.mktemp("jpeg_entropy_host") / "jpeg_entropy_host"
    r = subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + os.path.join(ROOT, "tokensgen_amd", "csrc"), os.path.join(ROOT, "tests", "csrc", "jpeg_entropy_host.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(jobs):
        """jobs: (blocks per MCU, MCUs, print, the three (DC, AC) table pairs, segment bytes) -> per job ("status", bits, coefficients or None) or ("table", index, code);
        the sanitizers must stay silent"""
        blob = struct.pack("<I", len(jobs))
        for bpm, mcus, show, huff, seg in jobs:
            blob += struct.pack("<III", bpm, mcus, show)
            for pair in huff:
                for bits, vals in pair:
                    blob += bytes(bits) + struct.pack("<I", len(vals)) + bytes(vals)
            blob += struct.pack("<I", len(seg)) + bytes(seg)
        path = exe.parent / "jobs.bin"
        path.write_bytes(blob)
        r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-3000:])
        lines, out = iter(r.stdout.splitlines()), []
        for bpm, mcus, show, _, _ in jobs:
            kind, *rest = next(lines).split()
            if kind == "table":
                out.append(("table", int(rest[0]), int(rest[1])))
            else:
                coef = np.array([[int(v) for v in next(lines).split()] for _ in range(mcus * bpm)]).reshape(mcus, bpm, 64) if show else None
                out.append(("status", int(rest[0]), coef))
        assert next(lines, None) is None
        return out

    return run


def segment_jobs(s, show=1, n_seg=None):
    """one job per restart segment of the frame s, cut where tg_jpeg_find_segments cuts"""
    info = jpeg.parse_jpeg(s)
    _, bpm, rows, cols = R.geometry(info.height, info.width, info.subsampling)
    total = rows * cols
    r = info.restart_interval or total
    n_seg = -(-total // r)
    begins, ends, status = D.device_segments(s, *info.scan, n_seg)
    return [(bpm, min((k + 1) * r, total) - k * r, show, info.huffman, s[b:e]) for k, (b, e) in enumerate(zip(begins, ends))], status


def test_host_program_on_valid_streams(host_program):
    """the coefficients it prints are the restatement's: our streams at every restart interval, the special inputs of the encoder's tests, Pillow's optimised tables"""
    rng = np.random.default_rng(0)
    noise = rng.integers(0, 256, (32, 32, 3), dtype=np.uint8)
    c = np.cos((2 * np.arange(8) + 1) * 7 * np.pi / 16)
    g = np.rint(128 + 100 * np.outer(c, c)).astype(np.uint8)
    streams = [R.encode(R.sample_image(h, w), q, sub, ri) for (h, w), q in (((33, 47), 90), ((9, 7), 1), ((48, 80), 100)) for sub in SUBS for ri in intervals(h, w, sub)]
    streams += [R.encode(a, q, sub, ri) for a in (noise, np.zeros((16, 16, 3), np.uint8), np.tile(np.stack([g, g, g], -1), (2, 2, 1))) for q in (50, 100) for sub in SUBS
                for ri in (1, 65535)]
    try:
        streams += [s for name, s in pillow_streams().items() if name.startswith("33x47")]
    except ImportError:
        pass
    jobs, cuts = [], []
    for s in streams:
        j, status = segment_jobs(s)
        assert status == 0
        jobs += j
        cuts.append(len(j))
    got, at = host_program(jobs), 0
    for s, n in zip(streams, cuts):
        assert all(kind == "status" and bits == 0 for kind, bits, _ in got[at:at + n])
        assert np.array_equal(np.concatenate([c for _, _, c in got[at:at + n]]), D.decode(s).coef)
        at += n


def test_host_program_on_damaged_streams(host_program):
    """a status and silent sanitizers: the scan cut inside, 200 seeded single-byte changes of the entropy data of a 33 x 47 stream, the three damaged frames of
    jpeg_dec_ref (whose recorded status bits are what the program reports), a table with an over-subscribed code"""
    s = R.encode(R.sample_image(33, 47), 90, "420", 65535)
    info = jpeg.parse_jpeg(s)
    b, e = info.scan
    for cut in (e - 2, (b + e) // 2, b + 1, b):
        (kind, bits, coef), = host_program([(6, 9, 1, info.huffman, s[b:cut])])
        assert kind == "status" and bits & D.ST_OUT_OF_BITS and not coef[-1, -1].any()
    rng = np.random.default_rng(0)
    jobs = []
    for _ in range(200):
        p, v = int(rng.integers(b, e)), int(rng.integers(0, 256))
        while v == s[p]:
            v = int(rng.integers(0, 256))
        jobs.append((6, 9, 0, info.huffman, s[b:p] + bytes([v]) + s[p + 1:e]))
    bits = [r[1] for r in host_program(jobs)]
    print({k: bits.count(k) for k in sorted(set(bits))})
    assert sum(1 for v in bits if v) >= 20 and all(v & ~0xf == 0 for v in bits)
    # as the GPU test decodes them: three segments of three MCUs with markers, and one of nine without
    for name, (bad, want, ri) in D.damaged_streams().items():
        jobs, status = segment_jobs(bad, 0)
        for kind, got, _ in host_program(jobs):
            assert kind == "status"
            status |= got
        assert status == want, (name, status, want)
    over = ((bytes([3] + [0] * 15), bytes([0, 1, 2])), info.huffman[0][1])
    assert host_program([(6, 9, 0, (info.huffman[0], over, info.huffman[2]), s[b:e])]) == [("table", 2, 2)]
    # 16 ones where a code should start: an invalid code, not a read past the end; a category above 11
    only = (bytes([1] + [0] * 15), bytes([0]))                                   # one code, "0"
    (kind, bits, _), = host_program([(3, 1, 0, ((only, only),) * 3, b"\xff\x00\xff\x00\xff\x00")])
    assert (kind, bits) == ("status", D.ST_INVALID_CODE)
    big = (bytes([1] + [0] * 15), bytes([12]))
    (kind, bits, _), = host_program([(3, 1, 0, ((big, only),) * 3, b"\x00\x00\x00")])
    assert (kind, bits) == ("status", D.ST_CATEGORY)
    run15 = (bytes([2] + [0] * 15), bytes([0xf0, 0xf1]))                         # "0": ZRL, "1": run 15 size 1
    (kind, bits, _), = host_program([(3, 1, 0, ((only, run15),) * 3, b"\x00\x00\x00")])      # DC, then ZRL x 4 takes the index to 65
    assert (kind, bits) == ("status", D.ST_COEF_INDEX)


if __name__ == "__main__":
    import PIL
    res = measure_pillow_parity()
    out = {"what": "tests/jpeg_dec_ref.py against Pillow's decoder on Pillow-encoded streams (quality 85), per stream", "pillow": PIL.__version__, "streams": res,
           "worst_level_difference": max(v["worst_level_difference"] for v in res.values()), "lowest_psnr_db": min(v["psnr_db"] for v in res.values())}
    with open(PARITY, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
    print(json.dumps(out))
