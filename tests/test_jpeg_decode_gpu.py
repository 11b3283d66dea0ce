"""GPU: csrc/jpeg_decode.hip through tokensgen_amd.jpeg and video_io.load_video.  A decoded frame is one exact byte array: every check of segment ranges,
coefficients, status and RGB bytes is torch.equal against tests/jpeg_dec_ref.py.

Sizes: 16 x 16 a single 4:2:0 MCU; 9 x 7 a single partial MCU whose real chroma plane is 5 x 4 (odd on one axis); 33 x 47 nine 4:2:0 MCUs, the marker number wraps
past 7; 48 x 80 whole MCUs (the real chroma plane is the padded one); 120 x 184 a real chroma plane of 60 x 92 inside a padded 64 x 96, and more than one workgroup of
the transform at either subsampling."""
import io

import numpy as np
import pytest
import torch

import jpeg_dec_ref as D
import jpeg_ref as R
from tokensgen_amd import jpeg, video_io
from tokensgen_amd import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [(16, 16), (9, 7), (33, 47), (48, 80), (120, 184)]
SUBS = ["420", "444"]
QUALITIES = [1, 50, 90, 100]


def host(a):
    return torch.from_numpy(np.array(a))                                        # a copy: the restatement's cached arrays and `bytes` are read-only


def dev(a):
    return host(a).to(DEV)


def stages(streams):
    """the three launch functions by hand, as decode_jpeg calls them: -> (seg_begin, seg_end, coef, status, rgb) and the frames' offsets in the buffer"""
    infos = [jpeg.parse_jpeg(s, i) for i, s in enumerate(streams)]
    H, W, sub, ri = infos[0][:4]
    off = np.cumsum([0] + [len(s) for s in streams])
    data = dev(np.frombuffer(b"".join(streams), np.uint8))
    scan_begin = dev(np.array([o + i.scan[0] for o, i in zip(off, infos)], np.int64))
    scan_end = dev(np.array([o + i.scan[1] for o, i in zip(off, infos)], np.int64))
    sets = list(dict.fromkeys(i.huffman for i in infos))
    htabs = dev(np.frombuffer(b"".join(jpeg._huffman_set(h) for h in sets), np.uint8).reshape(len(sets), -1))
    htab_index = dev(np.array([sets.index(i.huffman) for i in infos], np.int32))
    qsets = list(dict.fromkeys(i.qtables for i in infos))
    qtabs = dev(np.array(qsets, np.uint16))
    qtab_index = dev(np.array([qsets.index(i.qtables) for i in infos], np.int32))
    status = torch.full((len(streams),), -1, dtype=torch.int32, device=DEV)     # find_segments stores it: the -1 does not survive
    n_seg = K.jpeg_decode_segments(H, W, sub, ri)
    seg_begin, seg_end = K.jpeg_find_segments(data, scan_begin, scan_end, n_seg, status)
    coef = K.jpeg_decode_coeffs(data, seg_begin, seg_end, H, W, sub, ri, htabs, htab_index, status)
    rgb = K.jpeg_idct_rgb(coef, H, W, sub, qtabs, qtab_index)
    return seg_begin, seg_end, coef, status, rgb, off


def check_against_ref(streams):
    """every stage's output == the restatement's, and decode_jpeg == the last stage"""
    seg_begin, seg_end, coef, status, rgb, off = stages(streams)
    assert seg_begin.dtype == seg_end.dtype == torch.int64 and coef.dtype == torch.int16 and rgb.dtype == torch.uint8 and rgb.is_cuda
    assert status.tolist() == [0] * len(streams)
    for f, s in enumerate(streams):
        begins, ends, _ = D.segment_ranges(s)
        assert seg_begin[f].tolist() == [off[f] + b for b in begins] and seg_end[f].tolist() == [off[f] + e for e in ends], f
        want = D.decode(s)
        assert torch.equal(coef[f].cpu().long(), host(want.coef)), f
        assert torch.equal(rgb[f].cpu(), host(want.rgb)), f
    out = jpeg.decode_jpeg(streams)
    assert out.dtype == torch.uint8 and out.is_cuda and torch.equal(out, rgb)
    return out


@pytest.mark.parametrize("quality", QUALITIES)
@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("size", SIZES)
def test_every_stage_equals_the_restatement(size, sub, quality):
    """segment ranges, coefficients, status and RGB bytes, for restart intervals 1, 3, one MCU row and 65 535 (no marker at all)"""
    H, W = size
    a = R.sample_image(H, W, seed=H)
    for ri in (1, 3, R.geometry(H, W, sub)[3], 65535):
        check_against_ref([R.encode(a, quality, sub, ri)])


@pytest.mark.parametrize("sub", SUBS)
def test_round_trips_on_the_device(sub):
    """tg_jpeg_decode_coeffs(encode_jpeg(x)) == tg_jpeg_coeffs(x); decode_jpeg(*encode_jpeg(x)) == the restatement's picture of the restated stream"""
    H, W = 120, 184
    frames = np.stack([R.sample_image(H, W, seed) for seed in range(3)])
    x = dev(frames)
    for ri in (1, 12, 65535):
        data, offsets = jpeg.encode_jpeg(x, 90, sub, ri)
        raw, o = data.cpu().numpy().tobytes(), offsets.tolist()
        streams = [raw[o[i]:o[i + 1]] for i in range(3)]
        assert torch.equal(stages(streams)[2], K.jpeg_coeffs(x, 90, sub))
        out = jpeg.decode_jpeg(data, offsets)
        assert torch.equal(out.cpu(), host(np.stack([D.decode(R.encode(f, 90, sub, ri)).rgb for f in frames])))
        assert torch.equal(jpeg.decode_jpeg(streams), out)                      # device `data` + `offsets` against a list of `bytes`
        assert torch.equal(jpeg.decode_jpeg(data.cpu(), offsets), out)


@pytest.mark.parametrize("sub", SUBS)
def test_special_inputs(sub):
    """flat black and white; uniform noise at quality 100 (stuffed FF 00 pairs, the longest codes); a block whose only AC coefficient is the last of the zigzag (three
    ZRL codes, no end-of-block)"""
    rng = np.random.default_rng(0)
    noise = rng.integers(0, 256, (32, 32, 3), dtype=np.uint8)
    assert R.encode(noise, 100, sub, 1).count(b"\xff\x00") >= 5
    for a in (np.zeros((16, 16, 3), np.uint8), np.full((16, 16, 3), 255, np.uint8), noise):
        for q in (1, 100):
            for ri in (1, 65535):
                out = check_against_ref([R.encode(a, q, sub, ri)])
                if q == 100 and a is not noise:
                    assert torch.equal(out[0].cpu(), host(a))       # flat frames at quality 100 decode exactly
    c = np.cos((2 * np.arange(8) + 1) * 7 * np.pi / 16)
    g = np.rint(128 + 100 * np.outer(c, c)).astype(np.uint8)
    g = np.stack([g, g, g], -1)
    tr = {}
    R.encode(g, 50, "444", 1, trace=tr)
    assert tr["zrl"] == 3
    check_against_ref([R.encode(np.tile(g, (2, 2, 1)), 50, sub, 1)])


def pillow_stream(a, **kw):
    from PIL import Image
    bio = io.BytesIO()
    Image.fromarray(a).save(bio, "JPEG", **kw)
    return bio.getvalue()


def test_pillow_streams_with_a_table_set_per_frame():
    """Pillow-encoded frames: optimised Huffman tables and another quality per frame in one call, so htab_index and qtab_index both matter; no restart markers"""
    pytest.importorskip("PIL.Image")
    for sub, code in (("420", 2), ("444", 0)):
        streams = [pillow_stream(R.sample_image(33, 47, seed), quality=q, subsampling=code, optimize=opt) for seed, (q, opt) in enumerate(((85, True), (40, True), (85, False),
                                                                                                                                             (95, True)))]
        infos = [jpeg.parse_jpeg(s) for s in streams]
        assert len({i.huffman for i in infos}) == 4 and len({i.qtables for i in infos}) == 3 and infos[0].restart_interval == 0 and infos[0].subsampling == sub
        check_against_ref(streams)
    # a frame without any DHT uses the Annex K tables
    s = R.encode(R.sample_image(33, 47), 90, "420", 3)
    bare = bytearray()
    pos = 2
    while s[pos + 1] != 0xda:
        ln = int.from_bytes(s[pos + 2:pos + 4], "big")
        if s[pos + 1] != 0xc4:
            bare += s[pos:pos + 2 + ln]
        pos += 2 + ln
    bare = s[:2] + bytes(bare) + s[pos:]
    assert b"\xff\xc4" not in bare[:300] and torch.equal(jpeg.decode_jpeg([bare]), jpeg.decode_jpeg([s]))


def test_batches_and_reproducibility():
    """three frames alone and in a batch; two runs bitwise equal; load_jpeg reads a file"""
    frames = [R.sample_image(33, 47, seed) for seed in range(3)]
    for sub in SUBS:
        streams = [R.encode(f, 90, sub, 2) for f in frames]
        batch = check_against_ref(streams)
        assert len({bytes(b.cpu().numpy().tobytes()) for b in batch}) == 3
        for f in range(3):
            assert torch.equal(jpeg.decode_jpeg(streams[f:f + 1])[0], batch[f])
        assert torch.equal(jpeg.decode_jpeg(streams), batch)
        assert torch.equal(jpeg.decode_jpeg(streams[0]), batch[:1])             # one `bytes` is a list of one


def test_load_jpeg(tmp_path):
    a = R.sample_image(48, 80)
    path = jpeg.save_jpeg(dev(a), tmp_path / "f.jpg", quality=80)
    got = jpeg.load_jpeg(path)
    assert got.shape == (48, 80, 3) and torch.equal(got.cpu(), host(D.decode(R.encode(a, 80, "420", 1)).rgb))


def test_damaged_streams_raise_and_spare_the_other_frames():
    """the three damaged frames that tests/test_jpeg_decode_cpu.py has run through the host program under the sanitizers: the scan cut short, one flipped byte that
    yields an invalid code, a missing restart marker.  decode_jpeg raises a ValueError that names the frame and the condition; the frames around it decode as alone."""
    for name, (bad, want, ri) in D.damaged_streams().items():
        good = [R.encode(R.sample_image(33, 47, seed), 90, "420", ri) for seed in (1, 2)]
        with pytest.raises(ValueError, match="decode_jpeg: frame 1: ") as e:
            jpeg.decode_jpeg([good[0], bad, good[1]])
        err = e.value
        assert isinstance(err, jpeg.JpegDecodeError) and err.status.tolist() == [0, want, 0], (name, err.status.tolist())
        for bit, text in K.JPEG_STATUS.items():
            assert (text in str(err)) == bool(want & bit), (name, str(err))
        assert torch.equal(err.frames[0].cpu(), host(D.decode(good[0]).rgb)) and torch.equal(err.frames[2].cpu(), host(D.decode(good[1]).rgb))
        with pytest.raises(ValueError, match="frame 0: "):
            jpeg.decode_jpeg([bad])
    # what is left of a damaged frame: the segments before the damage decode, the blocks after it are zero (grey), never old memory
    whole = D.decode(R.encode(R.sample_image(33, 47), 90, "420", 3)).rgb
    with pytest.raises(jpeg.JpegDecodeError) as e:
        jpeg.decode_jpeg([D.damaged_streams()["cut"][0]])
    got = e.value.frames[0].cpu().numpy()
    assert np.array_equal(got[:15], whole[:15]) and not np.array_equal(got, whole)      # segment 0 is MCU row 0; row 15 takes chroma from the damaged MCU row below
    with pytest.raises(jpeg.JpegDecodeError) as e:
        jpeg.decode_jpeg([D.damaged_streams()["flipped"][0]])
    assert bool((e.value.frames[0, 17:] == 128).all())                          # the damage is in the first MCU: every later block of the one segment is zero


def test_output_store_guard():
    """an output buffer shorter than the frames loses bytes but nothing is stored outside: the guard bytes around it stay"""
    for sub, size in (("420", (33, 47)), ("444", (16, 24))):                   # 3 x 47 bytes per row: the byte path; 3 x 24: the dword path
        H, W = size
        s = R.encode(R.sample_image(H, W), 90, sub, 1)
        want = D.decode(s).rgb.tobytes()
        coef = stages([s])[2]
        info = jpeg.parse_jpeg(s)
        qtabs, qidx = dev(np.array([info.qtables], np.uint16)), torch.zeros(1, dtype=torch.int32, device=DEV)
        for short in (len(want) - 37, len(want) - 12, 5):
            tail = len(want) + 64                                               # room for everything a missing guard would store: a failed assertion, no fault
            buf = torch.full((64 + short + tail,), 0xa5, dtype=torch.uint8, device=DEV)
            K.jpeg_idct_rgb(coef, H, W, sub, qtabs, qidx, out=buf[64:64 + short])
            host = buf.cpu().numpy().tobytes()
            assert host[:64] == b"\xa5" * 64 and host[64 + short:] == b"\xa5" * tail and host[64:64 + short] == want[:short], (sub, short)
    # the wrapper layer refuses what only it can see
    with pytest.raises(ValueError, match="coef must be contiguous"):
        K.jpeg_idct_rgb(coef, 32, 24, "444", qtabs, qidx)
    with pytest.raises(ValueError, match="qtabs"):
        K.jpeg_idct_rgb(coef, 16, 24, "444", qtabs[0], qidx)
    with pytest.raises(ValueError, match="jpeg"):
        K.jpeg_decode_segments(16, 16, "411", 1)


@pytest.fixture(scope="module")
def exported(tmp_path_factory):
    """a file from export_to_video: 12 frames of 48 x 80 at 8 fps; -> (path, the frames on the device, the restated decode of the file's frames)"""
    H, W = 48, 80
    frames = dev(np.stack([R.sample_image(H, W, seed) for seed in range(12)]))
    path = video_io.export_to_video(frames, str(tmp_path_factory.mktemp("avi") / "v.avi"), fps=8, quality=85)
    restated = np.stack([D.decode(R.encode(f, 85, "420", 1)).rgb for f in frames.cpu().numpy()])
    return path, frames, restated


def test_mjpeg_reader_on_an_exported_file(exported):
    path, frames, restated = exported
    with jpeg.MJPEGReader(path) as r:
        assert len(r) == 12 and r.size == (48, 80) and r.fps == 8
        everything = r.read()
        assert torch.equal(everything, jpeg.decode_jpeg(jpeg.jpeg_bytes(frames, 85))) and torch.equal(everything.cpu(), host(restated))
        idx = [0, 3, 3, 11, 7, -1]
        one = r.get_batch(idx)
        assert torch.equal(one, everything[idx]) and torch.equal(torch.cat([r.get_batch(idx[:2]), r.get_batch(idx[2:])]), one)
        assert torch.equal(r.read(4, 9), everything[4:9])
        old = jpeg.MJPEGReader.BATCH
        jpeg.MJPEGReader.BATCH = 5                                              # several decode calls per read: the same frames
        try:
            assert torch.equal(r.read(), everything) and torch.equal(r.get_batch(idx), one)
        finally:
            jpeg.MJPEGReader.BATCH = old
    got, fps = jpeg.read_mjpeg_avi(path)
    assert torch.equal(got, everything) and fps == 8


@pytest.mark.parametrize("crop_to_fit", [True, False])
@pytest.mark.parametrize("sample_fps", [-1, 4])
def test_load_video_of_an_exported_file(exported, crop_to_fit, sample_fps):
    """file -> device frames -> prepare_video: torch.equal to prepare_video of the restated frames at the sampled indices"""
    path, _, restated = exported
    out = video_io.load_video(path, (32, 48), 5, True, sample_fps, 0, -1, 2, crop_to_fit=crop_to_fit)
    idx = video_io.sample_frame_indices(12, 8.0, 5, sample_fps, 0, -1, 2)
    assert len(idx) == (10 if sample_fps == -1 else 5)
    want = video_io.prepare_video(restated[idx], (32, 48), crop_to_fit, True)
    assert out.dtype == torch.bfloat16 and out.shape == (1, len(idx), 3, 32, 48) and out.is_cuda and torch.equal(out, want)
