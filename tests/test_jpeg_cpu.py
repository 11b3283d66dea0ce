"""CPU: the JPEG definition as tests/jpeg_ref.py restates it (the streams decode, the restart interval does not change the picture, the quality is that of a
standard encoder, the special inputs contain what they are meant to provoke, three wrong rules change the bytes), the AVI walker of tests/avi_ref.py on a file made
from restated frames, every refusal of tokensgen_amd.jpeg / video_io that is raised before a device is needed, and the argument validation of the C entry points of
csrc/jpeg.hip (which happens before any launch)."""
import ctypes
import io
import struct

import numpy as np
import pytest
import torch

import avi_ref
import jpeg_ref as R

SIZES = [(16, 16), (9, 7), (33, 47), (48, 80), (120, 184)]
SUBS = ["420", "444"]


def psnr(a, b):
    return 10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


def mcus(h, w, sub):
    _, _, rows, cols = R.geometry(h, w, sub)
    return rows, cols


def special_inputs():
    rng = np.random.default_rng(0)
    return {"black": np.zeros((16, 16, 3), np.uint8), "white": np.full((16, 16, 3), 255, np.uint8), "noise": rng.integers(0, 256, (32, 32, 3), dtype=np.uint8)}


def zrl_picture():
    """8 x 8 grey: 100 cos((2 x + 1) 7 pi / 16) cos((2 y + 1) 7 pi / 16) around 128"""
    c = np.cos((2 * np.arange(8) + 1) * 7 * np.pi / 16)
    g = np.rint(128 + 100 * np.outer(c, c)).astype(np.uint8)
    return np.stack([g, g, g], -1)


def test_tables_and_header():
    """the literal DCT matrix of the kernel file is the formula's; the Huffman tables are complete prefix codes of the right sizes; the header is 629 bytes"""
    literal = [[2896] * 8, [4017, 3406, 2276, 799, -799, -2276, -3406, -4017], [3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784],
               [3406, -799, -4017, -2276, 2276, 4017, 799, -3406], [2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896], [2276, -4017, 799, 3406, -3406, -799, 4017, -2276],
               [1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567], [799, -2276, 3406, -4017, 4017, -3406, 2276, -799]]
    assert R.DCT_A.tolist() == literal
    assert sorted(R.ZIGZAG.tolist()) == list(range(64))
    for dc, ac in R.HUFF:
        assert len(dc) == 12 and len(ac) == 162
        for table in (dc, ac):
            codes = sorted((format(c, f"0{n}b") for c, n in table.values()), key=len)
            assert not any(b.startswith(a) for i, a in enumerate(codes) for b in codes[i + 1:])
    assert R.quant_table(R.Q_LUMA, 50).tolist() == R.Q_LUMA.tolist() and set(R.quant_table(R.Q_LUMA, 100).tolist()) == {1}
    assert R.quant_table(R.Q_CHROMA, 1).max() == 255 and R.quant_table(R.Q_LUMA, 1).min() == 255
    h = R.header(480, 720, 90, "420", 1)
    assert len(h) == 629 and h[:4] == b"\xff\xd8\xff\xe0" and h[-14:-12] == b"\xff\xda" and h[615 - 6:615] == b"\xff\xdd\x00\x04\x00\x01"
    assert struct.unpack(">HH", h[163:167]) == (480, 720)


def test_dct_range_and_dc_of_a_flat_block():
    """a flat block has one coefficient, 8 (v - 128) to the rounding of the two shifts; the extreme sign patterns stay inside -1024 .. 1020 and inside int32"""
    for v in (0, 1, 127, 128, 200, 255):
        c = R.fdct(np.full((8, 8), v - 128, np.int64))
        assert abs(int(c[0, 0]) - 8 * (v - 128)) <= 1 and not c.reshape(-1)[1:].any()
    lo, hi = 0, 0
    for u in range(8):
        for v in range(8):
            basis = np.sign(np.outer(R.DCT_A[v], R.DCT_A[u]))
            for s in (1, -1):
                p = np.where(s * basis > 0, 127, -128).astype(np.int64)
                t = np.einsum("ux,yx->yu", R.DCT_A, p)
                assert np.abs(t).max() < 2 ** 31 and np.abs(np.einsum("vy,yu->vu", R.DCT_A, (t + 512) >> 10)).max() < 2 ** 31 - 32768
                c = R.fdct(p)
                lo, hi = min(lo, int(c.min())), max(hi, int(c.max()))
    assert (lo, hi) == (-1024, 1020)


def test_restart_interval_changes_markers_not_coefficients():
    """the segment lengths add up; the k-th marker is FF D0 + (k mod 8) and wraps past 7 on the 9 MCUs of 33 x 47"""
    a = R.sample_image(33, 47)
    assert mcus(33, 47, "420") == (3, 3)
    tr = {}
    s = R.encode(a, 90, "420", 1, trace=tr)
    assert len(tr["segments"]) == 9 and sum(tr["segments"]) == len(s) - R.HEADER_BYTES
    pos, found = R.HEADER_BYTES, []
    for n in tr["segments"]:
        pos += n
        assert s[pos - 2] == 0xff
        found.append(s[pos - 1])
    assert found == [0xd0, 0xd1, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd9]
    a = R.sample_image(48, 80)
    tr = {}
    s = R.encode(a, 50, "444", 1, trace=tr)
    assert len(tr["segments"]) == 60
    ends = np.cumsum(tr["segments"]) + R.HEADER_BYTES
    assert [s[e - 1] for e in ends[:10]] == [0xd0, 0xd1, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd0, 0xd1] and s[-2:] == b"\xff\xd9"
    tr3 = {}
    R.encode(a, 50, "444", 3, trace=tr3)
    assert len(tr3["segments"]) == 20
    one = {}
    whole = R.encode(a, 50, "444", 65535, trace=one)
    assert len(one["segments"]) == 1 and len(whole) < len(s)


def test_special_inputs_contain_what_they_provoke():
    sp = special_inputs()
    tr = {}
    s = R.encode(sp["noise"], 100, "420", 1, trace=tr)
    assert tr["stuffed"] == 10                                                  # FF bytes of entropy data, each followed by 00
    scan = s[R.HEADER_BYTES:]
    assert scan.count(b"\xff\x00") == 10
    # one block whose only AC coefficient is the last of the zigzag: three ZRL codes and no end-of-block
    coef = np.zeros((1, 3, 64), np.int64)
    coef[0, 0, 0], coef[0, 0, 63] = 5, -3
    tr = {}
    R.entropy(coef, 3, 1, trace=tr)
    assert tr["zrl"] == 3 and tr["eob"] == 2                                    # the two chroma blocks end at once, the luma block has no end-of-block
    dc, ac = R.HUFF[0]
    assert dc[3] == (0b100, 3) and ac[0xf0] == (0b11111111001, 11) and ac[0x00] == (0b1010, 4) and R.HUFF[1][1][0x00] == (0b00, 2)     # the codes every table lists
    bw = R.BitWriter(stuffing=False)
    assert R.encode_block(bw, coef[0, 0], 0, R.HUFF[0], {}) == 5
    bw.flush()
    want = "100" + "101" + "11111111001" * 3 + format(ac[0xe2][0], f"0{ac[0xe2][1]}b") + "00"      # DC size 3, +5; ZRL x 3 (48 of the 62 zeros); (run 14, size 2); -3 as 00; no 1010
    assert "".join(format(b, "08b") for b in bw.out) == want + "1" * (-len(want) % 8)
    # a picture that produces such a block: the highest basis function alone, grey, strong enough to survive Q = 99 at quality 50
    g = zrl_picture()
    c = R.coefficients(g, 50, "444")
    assert c[0, 0, 63] != 0 and not c[0, 0, :63].any() and not c[0, 1:].any()
    tr = {}
    R.encode(g, 50, "444", 1, trace=tr)
    assert tr["zrl"] == 3 and tr["eob"] == 2


def test_three_wrong_rules_each_change_the_bytes():
    a = R.sample_image(48, 80)
    good = R.encode(a, 50, "420", 1)
    assert R.encode(a, 50, "420", 1, wrong="truncate") != good
    assert R.encode(a, 50, "420", 1, wrong="no_dc_reset") != good
    assert R.encode(a, 50, "420", 65535, wrong="no_dc_reset") == R.encode(a, 50, "420", 65535)        # without a marker the rule has nothing to do
    noise = special_inputs()["noise"]
    assert R.encode(noise, 100, "420", 1, wrong="no_stuffing") != R.encode(noise, 100, "420", 1)


def test_streams_decode_and_match_a_standard_encoder():
    """Pillow (libjpeg) decodes every stream; the picture does not depend on the restart interval; PSNR is within 1.0 dB of Pillow's own encoder (0.35 dB measured:
    the rest of the margin is for the different DCT rounding and the unbiased chroma mean); flat frames at quality 100 decode exactly."""
    Image = pytest.importorskip("PIL.Image")
    dec = lambda s: np.array(Image.open(io.BytesIO(s)).convert("RGB"))
    worst = 0.0
    for h, w in SIZES:
        a = R.sample_image(h, w)
        for sub in SUBS:
            rows, cols = mcus(h, w, sub)
            for q in (50, 90, 100):
                pics = [dec(R.encode(a, q, sub, ri)) for ri in (1, 3, cols, 65535)]
                assert pics[0].shape == a.shape and all(np.array_equal(pics[0], p) for p in pics[1:]), (h, w, sub, q)
                bio = io.BytesIO()
                Image.fromarray(a).save(bio, "JPEG", quality=q, subsampling={"420": 2, "444": 0}[sub])
                gap = psnr(a, dec(bio.getvalue())) - psnr(a, pics[0])
                worst = max(worst, gap)
                assert gap <= 1.0, (h, w, sub, q, gap)
    print(f"worst PSNR gap to Pillow's encoder: {worst:.3f} dB")
    for name, a in special_inputs().items():
        for sub in SUBS:
            for q in (1, 100):
                d = dec(R.encode(a, q, sub, 1))
                assert d.shape == a.shape
                if name != "noise" and q == 100:
                    assert np.array_equal(d, a), (name, sub)


def test_avi_walker_on_restated_frames(tmp_path):
    from tokensgen_amd.jpeg import MJPEGWriter
    frames = [R.encode(R.sample_image(33, 47, seed), 90, "420", 1) for seed in range(3)]
    assert any(len(f) & 1 for f in frames) or len(R.encode(R.sample_image(33, 47, 3), 90, "420", 1)) & 1       # an odd chunk needs its pad byte
    path = tmp_path / "a.avi"
    with MJPEGWriter(path, 29.97) as w:
        assert w.write_jpegs(frames[:1], 33, 47) == 1 and w.write_jpegs(frames[1:], 33, 47) == 2 and w.frames == 3
        with pytest.raises(ValueError, match="one size"):
            w.write_jpegs(frames[:1], 32, 47)
        with pytest.raises(ValueError, match="JPEG streams"):
            w.write_jpegs([b"not a jpeg"], 33, 47)
    w.close()                                                                   # a second close does nothing
    with pytest.raises(ValueError, match="closed"):
        w.write_jpegs(frames[:1], 33, 47)
    a = avi_ref.walk(path.read_bytes())
    assert a.frames == frames and a.movi == 220
    assert (a.avih["width"], a.avih["height"], a.avih["total_frames"]) == (47, 33, 3) and a.avih["suggested_buffer"] == max(map(len, frames))
    assert (a.strh["rate"], a.strh["scale"]) == (2997, 100) and a.avih["us_per_frame"] == 33367
    assert a.strh["frame"] == (0, 0, 47, 33) and a.strf["size_image"] == 3 * 33 * 47
    # the walker notices a broken file
    raw = bytearray(path.read_bytes())
    raw[4:8] = struct.pack("<I", len(raw))
    with pytest.raises(AssertionError):
        avi_ref.walk(bytes(raw))
    # an empty file is a valid file
    with MJPEGWriter(tmp_path / "e.avi", 8):
        pass
    e = avi_ref.walk((tmp_path / "e.avi").read_bytes())
    assert e.frames == [] and e.avih["total_frames"] == 0


def test_avi_size_limit_refuses_the_write_that_crosses_it(tmp_path):
    from tokensgen_amd.jpeg import MJPEGWriter
    frames = [R.encode(R.sample_image(16, 16, seed), 50, "420", 1) for seed in range(4)]
    chunk = lambda f: 8 + len(f) + (len(f) & 1)
    w = MJPEGWriter(tmp_path / "l.avi", 8)
    w.MAX_FILE_BYTES = 224 + sum(map(chunk, frames[:3])) + 8 + 16 * 3           # exactly three frames fit
    assert w.write_jpegs(frames[:2], 16, 16) == 2
    with pytest.raises(ValueError, match="OpenDML"):
        w.write_jpegs(frames[2:], 16, 16)                                       # two more: refused whole
    assert w.write_jpegs(frames[2:3], 16, 16) == 1
    with pytest.raises(ValueError, match="OpenDML"):
        w.write_jpegs(frames[3:], 16, 16)
    w.close()
    raw = (tmp_path / "l.avi").read_bytes()
    assert len(raw) == w.MAX_FILE_BYTES and avi_ref.walk(raw).frames == frames[:3]
    assert MJPEGWriter.MAX_FILE_BYTES == 2 ** 31 - 1


def test_refusals_before_any_device(tmp_path):
    from tokensgen_amd import jpeg, video_io
    u8 = torch.zeros(2, 16, 16, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        jpeg.encode_jpeg(u8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        jpeg.jpeg_bytes(u8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        jpeg.save_jpeg(u8[0], tmp_path / "a.jpg")
    with pytest.raises(NotImplementedError, match="uint8"):
        jpeg.encode_jpeg(u8.float())
    with pytest.raises(ValueError, match="three channels"):
        jpeg.encode_jpeg(u8[..., :2])
    with pytest.raises(ValueError, match="three channels"):
        jpeg.encode_jpeg(u8[0])
    with pytest.raises(ValueError, match="at least one pixel"):
        jpeg.encode_jpeg(u8[:0])
    with pytest.raises(ValueError, match="65535"):
        jpeg.encode_jpeg(torch.zeros(1, 65536, 1, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="tensor"):
        jpeg.encode_jpeg([u8])
    for bad in (0, 101, 50.0, True, None):
        with pytest.raises(ValueError, match="quality"):
            jpeg.encode_jpeg(u8, quality=bad)
    for bad in ("422", 420, None):
        with pytest.raises(ValueError, match="subsampling"):
            jpeg.encode_jpeg(u8, subsampling=bad)
    for bad in (0, 65536, 1.0, False):
        with pytest.raises(ValueError, match="restart_interval"):
            jpeg.encode_jpeg(u8, restart_interval=bad)
    with pytest.raises(ValueError, match="one frame per file"):
        jpeg.save_jpeg(u8, tmp_path / "a.jpg")
    for bad in (0, -1, float("inf"), float("nan"), "8", True):
        with pytest.raises(ValueError, match="fps"):
            jpeg.MJPEGWriter(tmp_path / "b.avi", bad)
    with pytest.raises(ValueError, match="quality"):
        jpeg.MJPEGWriter(tmp_path / "b.avi", 8, quality=0)
    assert not (tmp_path / "b.avi").exists()                                    # refused before the file is made
    with jpeg.MJPEGWriter(tmp_path / "c.avi", 8) as w:
        with pytest.raises(RuntimeError, match="no CPU path"):
            w.write(u8)
        with pytest.raises(NotImplementedError):
            w.write(u8.float())
    for name in ("v.mp4", "v.gif", "v"):
        with pytest.raises(ValueError, match="Motion-JPEG .avi"):
            video_io.export_to_video(u8, str(tmp_path / name))
    with pytest.raises(RuntimeError, match="no CPU path"):
        video_io.export_to_video(u8, str(tmp_path / "v.avi"))
    with pytest.raises(ValueError, match="one video per file"):
        jpeg.export_to_video(torch.zeros(2, 2, 8, 8, 3, dtype=torch.uint8), str(tmp_path / "v.avi"))
    import inspect
    assert list(inspect.signature(video_io.export_to_video).parameters) == ["video_frames", "output_video_path", "fps", "quality"]
    assert inspect.signature(video_io.export_to_video).parameters["fps"].default == 8


def test_jpeg_is_imported_lazily():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); from tokensgen_amd import video_io, metrics; video_io.VideoProcessor(); assert 'tokensgen_amd.jpeg' not in sys.modules\n"
            "try:\n    video_io.export_to_video(None, 'x.avi')\nexcept ValueError:\n    pass\nassert 'tokensgen_amd.jpeg' in sys.modules") % root
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]


def test_c_abi_validates_before_any_launch():
    """one argument wrong at a time; the calls never reach a launch"""
    from tokensgen_amd import lib as L
    lib = L.load()
    err = lambda: lib.tg_last_error_string().decode()
    buf = ctypes.create_string_buffer(8192)
    p = ctypes.addressof(buf) + (16 - ctypes.addressof(buf) % 16)
    assert lib.tg_jpeg_header_bytes() == R.HEADER_BYTES
    geo = lambda *a: tuple(lib.tg_jpeg_geometry(*a, what) for what in range(6))
    assert geo(480, 720, 420, 1) == (30, 45, 6, 1350, 1350 * 6 * 64, 0) and geo(480, 720, 444, 100) == (60, 90, 3, 54, 5400 * 3 * 64, 0)
    assert geo(9, 7, 420, 65535) == (1, 1, 6, 1, 384, 0) and geo(33, 47, 420, 2) == (3, 3, 6, 5, 9 * 384, 0) and geo(65535, 65535, 444, 1)[:2] == (8192, 8192)
    for bad in ((0, 8, 420, 1), (8, 65536, 420, 1), (8, 8, 422, 1), (8, 8, 420, 0), (8, 8, 420, 65536)):
        assert geo(*bad) == (0,) * 6
    co = dict(frames=p, F=1, H=16, W=16, subsampling=420, quality=90, coef=p + 1024, stream=None)
    call = lambda **kw: lib.tg_jpeg_coeffs(*{**co, **kw}.values())
    assert call(frames=None) == -1 and call(coef=None) == -1 and "null pointer" in err()
    assert call(quality=0) == -1 and call(quality=101) == -1 and "1..100" in err()
    assert call(F=0) == -2 and call(H=0) == -2 and call(W=65536) == -2 and call(subsampling=422) == -2 and "420 or 444" in err()
    assert call(coef=p + 1032) == -3 and "16-byte" in err()
    assert call(F=1 << 20, H=65535, W=65535, subsampling=444) == -2 and "too many strips" in err()
    sb = dict(coef=p, F=1, H=16, W=16, subsampling=420, restart_interval=1, seg_bytes=p + 1024, stream=None)
    call = lambda **kw: lib.tg_jpeg_segment_bytes(*{**sb, **kw}.values())
    assert call(coef=None) == -1 and call(seg_bytes=None) == -1
    assert call(restart_interval=0) == -1 and call(restart_interval=65536) == -1 and "1..65535" in err()
    assert call(F=0) == -2 and call(H=65536) == -2 and call(subsampling=0) == -2
    assert call(coef=p + 8) == -3 and call(seg_bytes=p + 1026) == -3
    wr = dict(coef=p, F=1, H=16, W=16, subsampling=420, quality=90, restart_interval=1, seg_offsets=p + 1024, frame_offsets=p + 2048, data=p + 4096, data_bytes=4096,
              stream=None)
    call = lambda **kw: lib.tg_jpeg_write(*{**wr, **kw}.values())
    assert call(coef=None) == -1 and call(seg_offsets=None) == -1 and call(frame_offsets=None) == -1 and call(data=None) == -1
    assert call(quality=0) == -1 and call(restart_interval=0) == -1
    assert call(F=0) == -2 and call(W=0) == -2 and call(subsampling=411) == -2
    assert call(data_bytes=630) == -2 and call(F=3, data_bytes=1892) == -2 and "cannot hold" in err()
    assert call(coef=p + 4) == -3 and call(seg_offsets=p + 1028) == -3 and call(frame_offsets=p + 2052) == -3
