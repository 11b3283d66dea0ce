"""GPU: csrc/jpeg.hip through tokensgen_amd.jpeg and video_io.export_to_video.  A JPEG frame is one exact byte string: every check of coefficients, segment sizes,
offsets and bytes is torch.equal (or ==) against tests/jpeg_ref.py; the AVI files are walked by tests/avi_ref.py.

Sizes: 16 x 16 a single 4:2:0 MCU; 9 x 7 a single partial MCU whose 189 bytes end inside a dword; 33 x 47 nine 4:2:0 MCUs, partial on both axes, the marker index
wraps past 7; 48 x 80 whole MCUs, more than one 64-pixel strip; 120 x 184 three strips, the last one short at 4:4:4 (23 MCU columns = 8 + 8 + 7)."""
import numpy as np
import pytest
import torch

import avi_ref
import jpeg_ref as R
from tokensgen_amd import jpeg, video_io
from tokensgen_amd import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [(16, 16), (9, 7), (33, 47), (48, 80), (120, 184)]
SUBS = ["420", "444"]
QUALITIES = [1, 50, 90, 100]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def as_bytes(data, offsets):
    host, o = data.cpu().numpy().tobytes(), offsets.tolist()
    return [host[o[i]:o[i + 1]] for i in range(len(o) - 1)]


def check_against_ref(frames_np, quality, sub, ri):
    """encode_jpeg of uint8 [F, H, W, 3] == the restatement, data and offsets"""
    data, offsets = jpeg.encode_jpeg(dev(frames_np), quality, sub, ri)
    want, want_off = R.encode_many(frames_np, quality, sub, ri)
    assert offsets.dtype == torch.int64 and offsets.device.type == "cpu" and torch.equal(offsets, torch.from_numpy(want_off))
    assert data.dtype == torch.uint8 and data.is_cuda and data.numel() == int(offsets[-1])
    assert torch.equal(data.cpu(), torch.frombuffer(bytearray(want), dtype=torch.uint8)), (frames_np.shape, quality, sub, ri)
    return data, offsets


@pytest.mark.parametrize("quality", QUALITIES)
@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("size", SIZES)
def test_bytes_equal_the_restatement(size, sub, quality):
    """coefficients, segment sizes and the stream, for restart intervals 1, 3, one MCU row and 65 535 (no marker at all)"""
    H, W = size
    a = R.sample_image(H, W, seed=H)
    _, bpm, rows, cols = R.geometry(H, W, sub)
    assert K.jpeg_geometry(H, W, sub, 3) == (rows, cols, bpm, -(-rows * cols // 3))
    coef = K.jpeg_coeffs(dev(a)[None], quality, sub)
    assert coef.dtype == torch.int16 and torch.equal(coef[0].cpu().long(), torch.from_numpy(R.coefficients(a, quality, sub)))
    for ri in (1, 3, cols, 65535):
        tr = {}
        R.encode(a, quality, sub, ri, trace=tr)
        seg = K.jpeg_segment_bytes(coef, H, W, sub, ri)
        assert seg.dtype == torch.int32 and seg[0].tolist() == tr["segments"]
        check_against_ref(a[None], quality, sub, ri)


@pytest.mark.parametrize("sub", SUBS)
def test_special_inputs(sub):
    """flat black and white; uniform noise at quality 100 (stuffed FF 00 pairs, the longest codes); a block whose only AC coefficient is the last of the zigzag (three
    ZRL codes, no end-of-block)"""
    rng = np.random.default_rng(0)
    noise = rng.integers(0, 256, (32, 32, 3), dtype=np.uint8)
    tr = {}
    R.encode(noise, 100, sub, 1, trace=tr)
    assert tr["stuffed"] >= 5
    for a in (np.zeros((16, 16, 3), np.uint8), np.full((16, 16, 3), 255, np.uint8), noise):
        for q in (1, 100):
            for ri in (1, 65535):
                check_against_ref(a[None], q, sub, ri)
    c = np.cos((2 * np.arange(8) + 1) * 7 * np.pi / 16)
    g = np.rint(128 + 100 * np.outer(c, c)).astype(np.uint8)
    g = np.stack([g, g, g], -1)
    tr = {}
    R.encode(g, 50, "444", 1, trace=tr)
    assert tr["zrl"] == 3
    check_against_ref(np.tile(g, (2, 2, 1))[None], 50, sub, 1)


def test_batches_views_and_reproducibility():
    """F = 3 with different content: a frame's bytes are the same alone and in a batch; [B, T, ..] input; a view that is not contiguous; input at another alignment;
    two runs bitwise equal"""
    H, W = 33, 47
    frames = np.stack([R.sample_image(H, W, seed) for seed in range(3)])
    for sub in SUBS:
        data, offsets = check_against_ref(frames, 90, sub, 1)
        batch = as_bytes(data, offsets)
        assert len(set(batch)) == 3
        for f in range(3):
            d1, o1 = jpeg.encode_jpeg(dev(frames[f:f + 1]), 90, sub, 1)
            assert as_bytes(d1, o1) == [batch[f]]
        again, off2 = jpeg.encode_jpeg(dev(frames), 90, sub, 1)
        assert torch.equal(again, data) and torch.equal(off2, offsets)
        assert jpeg.jpeg_bytes(dev(frames), 90, sub, 1) == batch
    six = np.stack([R.sample_image(H, W, seed) for seed in range(6)])
    d5, o5 = jpeg.encode_jpeg(dev(six).reshape(2, 3, H, W, 3), 75, "420", 2)
    d4, o4 = jpeg.encode_jpeg(dev(six), 75, "420", 2)
    assert torch.equal(d5, d4) and torch.equal(o5, o4) and o5.numel() == 7
    wide = dev(np.concatenate([six, six], 2))[:, :, 5:5 + W]                    # a view: rows 3 * 47 bytes out of 3 * 94
    assert not wide.is_contiguous()
    dv, ov = jpeg.encode_jpeg(wide, 75, "420", 2)
    dc, oc = jpeg.encode_jpeg(wide.contiguous(), 75, "420", 2)
    assert torch.equal(dv, dc) and torch.equal(ov, oc)
    for off in (1, 2, 3):                                                       # the frames' first byte at every phase of a dword
        buf = torch.empty(six.size + off, dtype=torch.uint8, device=DEV)
        v = buf[off:].view(six.shape)
        v.copy_(dev(six))
        dm, om = jpeg.encode_jpeg(v, 75, "420", 2)
        assert torch.equal(dm, d4) and torch.equal(om, o4)


def test_mjpeg_writer_and_files(tmp_path):
    """a file fed in two pieces equals the file from one call and walks clean; its chunks are jpeg_bytes; save_jpeg writes the frame's bytes"""
    H, W = 48, 80
    frames = dev(np.stack([R.sample_image(H, W, seed) for seed in range(5)]))
    one = jpeg.write_mjpeg_avi(tmp_path / "one.avi", frames, 8, quality=80, subsampling="444", restart_interval=10)
    with jpeg.MJPEGWriter(tmp_path / "two.avi", 8, quality=80, subsampling="444", restart_interval=10) as w:
        assert w.write(frames[:2]) == 2 and w.write(frames[2:].reshape(1, 3, H, W, 3)) == 3 and w.frames == 5
        with pytest.raises(ValueError, match="one size"):
            w.write(frames[:, :32])
    raw = (tmp_path / "two.avi").read_bytes()
    assert raw == open(one, "rb").read()
    a = avi_ref.walk(raw)
    assert a.frames == jpeg.jpeg_bytes(frames, 80, "444", 10) == [R.encode(f, 80, "444", 10) for f in frames.cpu().numpy()]
    assert (a.avih["width"], a.avih["height"], a.strh["rate"], a.strh["scale"]) == (W, H, 8, 1)
    old = jpeg.MJPEGWriter.BATCH
    jpeg.MJPEGWriter.BATCH = 2                                                  # several encode calls per write: the same file
    try:
        jpeg.write_mjpeg_avi(tmp_path / "three.avi", frames, 8, quality=80, subsampling="444", restart_interval=10)
    finally:
        jpeg.MJPEGWriter.BATCH = old
    assert (tmp_path / "three.avi").read_bytes() == raw
    path = jpeg.save_jpeg(frames[1], tmp_path / "f.jpg", quality=80, subsampling="444", restart_interval=10)
    assert open(path, "rb").read() == a.frames[1]
    assert open(jpeg.save_jpeg(frames[1:2], tmp_path / "g.jpg"), "rb").read() == R.encode(frames[1].cpu().numpy(), 90, "420", 1)


def test_export_to_video_of_the_video_processor_output(tmp_path):
    g = torch.Generator().manual_seed(50)
    video = (torch.rand(1, 3, 5, 32, 48, generator=g) * 2 - 1).to(torch.bfloat16).to(DEV)
    frames = video_io.VideoProcessor().postprocess_video(video, "uint8")
    assert frames.shape == (1, 5, 32, 48, 3)
    path = video_io.export_to_video(frames, str(tmp_path / "v.avi"), fps=12)
    assert path == str(tmp_path / "v.avi")
    a = avi_ref.walk(open(path, "rb").read())
    assert a.frames == [R.encode(f, 90, "420", 1) for f in frames[0].cpu().numpy()] and (a.strh["rate"], a.strh["scale"]) == (12, 1)
    video_io.export_to_video(frames[0], str(tmp_path / "w.avi"), 12, 90)        # diffusers' positional order; [T, H, W, 3]
    assert (tmp_path / "w.avi").read_bytes() == open(path, "rb").read()
    low = avi_ref.walk(open(video_io.export_to_video(frames, str(tmp_path / "q.AVI"), quality=30), "rb").read())
    assert low.frames == [R.encode(f, 30, "420", 1) for f in frames[0].cpu().numpy()] and low.strh["rate"] == 8


def test_refusals_on_the_device(tmp_path):
    u8 = torch.zeros(2, 16, 16, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(NotImplementedError, match="uint8"):
        jpeg.encode_jpeg(u8.float())
    with pytest.raises(NotImplementedError, match="uint8"):
        jpeg.encode_jpeg(u8.to(torch.bfloat16))
    with pytest.raises(ValueError, match="three channels"):
        jpeg.encode_jpeg(u8[..., :2])
    with pytest.raises(ValueError, match="three channels"):
        jpeg.encode_jpeg(torch.zeros(2, 16, 16, 4, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="three channels"):
        jpeg.encode_jpeg(u8[0])
    with pytest.raises(ValueError, match="at least one pixel"):
        jpeg.encode_jpeg(u8[:0])
    with pytest.raises(RuntimeError, match="no CPU path"):
        jpeg.encode_jpeg(u8.cpu())
    for kw in (dict(quality=0), dict(quality=101), dict(quality=90.0), dict(subsampling="422"), dict(subsampling=420), dict(restart_interval=0),
               dict(restart_interval=65536), dict(restart_interval=2.0)):
        for fn in (jpeg.encode_jpeg, jpeg.jpeg_bytes):
            with pytest.raises(ValueError, match=next(iter(kw))):
                fn(u8, **kw)
        with pytest.raises(ValueError, match=next(iter(kw))):
            jpeg.save_jpeg(u8[0], tmp_path / "a.jpg", **kw)
        with pytest.raises(ValueError, match=next(iter(kw))):
            jpeg.write_mjpeg_avi(tmp_path / "a.avi", u8, 8, **kw)
    assert not (tmp_path / "a.jpg").exists() and not (tmp_path / "a.avi").exists()
    with pytest.raises(ValueError, match="one frame per file"):
        jpeg.save_jpeg(u8, tmp_path / "a.jpg")
    with pytest.raises(ValueError, match="fps"):
        jpeg.write_mjpeg_avi(tmp_path / "a.avi", u8, 0)
    with pytest.raises(ValueError, match="Motion-JPEG .avi"):
        video_io.export_to_video(u8, str(tmp_path / "a.mp4"))
    with pytest.raises(ValueError, match="one video per file"):
        video_io.export_to_video(u8.reshape(2, 1, 16, 16, 3), str(tmp_path / "a.avi"))
    with pytest.raises(NotImplementedError, match="uint8"):
        video_io.export_to_video(u8.float(), str(tmp_path / "a.avi"))
    # the wrapper layer below refuses what only it can see
    coef = K.jpeg_coeffs(u8, 90, "420")
    with pytest.raises(ValueError, match="coef must be contiguous"):
        K.jpeg_segment_bytes(coef, 32, 16, "420", 1)
    with pytest.raises(ValueError, match="seg_offsets"):
        K.jpeg_write(coef, 16, 16, 90, "420", 1, torch.zeros(2, 2, dtype=torch.int64, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV),
                     torch.zeros(4096, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="jpeg"):
        K.jpeg_geometry(16, 16, "411")


def test_write_stays_inside_the_buffer():
    """offsets that point past the end, or a buffer shorter than the stream, lose bytes but never store outside: the guard words around the buffer stay"""
    a = R.sample_image(33, 47)
    want = R.encode(a, 90, "420", 1)
    coef = K.jpeg_coeffs(dev(a)[None], 90, "420")
    seg = K.jpeg_segment_bytes(coef, 33, 47, "420", 1)
    ends = torch.cumsum(seg, 1, dtype=torch.int64)
    seg_off = (ends - seg + R.HEADER_BYTES).contiguous()
    frame_off = torch.zeros(1, dtype=torch.int64, device=DEV)
    short = len(want) - 37
    tail = len(want) + 64                                                       # room for everything a missing guard would store: a failed assertion, no fault
    buf = torch.full((64 + short + tail,), 0xa5, dtype=torch.uint8, device=DEV)
    K.jpeg_write(coef, 33, 47, 90, "420", 1, seg_off, frame_off, buf[64:64 + short])
    host = buf.cpu().numpy().tobytes()
    assert host[:64] == b"\xa5" * 64 and host[64 + short:] == b"\xa5" * tail and host[64:64 + short] == want[:short]
    buf.fill_(0xa5)
    K.jpeg_write(coef, 33, 47, 90, "420", 1, seg_off + short + 8, frame_off - 5, buf[64:64 + short])
    assert bool((buf == 0xa5).all())
