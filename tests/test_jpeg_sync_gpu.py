"""GPU: csrc/jpeg_decode_sync.hip, parallel entropy decoding inside a restart segment, through kernels.jpeg_decode_coeffs_sync, decode_jpeg's
`entropy` keyword and video_io.load_video.  The coefficients are those of the serial launch and of tests/jpeg_dec_ref.py, bit for bit (torch.equal); every valid
stream is vouched for (clean = 1), so none is left to the fallback; rounds lie in 1 .. lanes of a chunk (1024 lanes, or the subsequences the longest segment has).

Sizes: 9 x 7 and 16 x 16 a single MCU; 33 x 47 nine 4:2:0 MCUs; 120 x 184 at quality 100 a scan of 49 418 bytes at 4:4:4 (four chunks of 1024 lanes at sub_bytes 16, so
the carried state and block count are used) with FF | 00 pairs split by subsequence boundaries at 16 and at 128 bytes; at quality 50 one stream that ends on a byte
boundary and one that ends in padding bits; one MCU row per segment and one MCU per segment: segments shorter than a subsequence."""
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
SUBS = ["420", "444"]
LANES = 1024
PATTERN = 0x5a5a5a5a


def host(a):
    return torch.from_numpy(np.array(a))


def dev(a):
    return host(a).to(DEV)


def pillow_stream(a, **kw):
    from PIL import Image
    bio = io.BytesIO()
    Image.fromarray(a).save(bio, "JPEG", **kw)
    return bio.getvalue()


def noise_image(h=120, w=184):
    return np.random.default_rng(0).integers(0, 256, (h, w, 3), dtype=np.uint8)


def launch(streams, sub_bytes, coef=None):
    """find_segments, then the serial and the parallel entropy launch on the same ranges -> (coef of the parallel launch, coef of the serial one, status of the serial
    one, clean, rounds, the longest segment in bytes).  status, clean and rounds are thirds of one buffer, as decode_jpeg holds them; the status third is filled with
    a pattern before the parallel launch and must keep it."""
    infos = [jpeg.parse_jpeg(s, i) for i, s in enumerate(streams)]
    H, W, sub, ri = infos[0][:4]
    F = len(streams)
    off = np.cumsum([0] + [len(s) for s in streams])
    data = dev(np.frombuffer(b"".join(streams), np.uint8))
    scan_begin = dev(np.array([o + i.scan[0] for o, i in zip(off, infos)], np.int64))
    scan_end = dev(np.array([o + i.scan[1] for o, i in zip(off, infos)], np.int64))
    sets = list(dict.fromkeys(i.huffman for i in infos))
    htabs = dev(np.frombuffer(b"".join(jpeg._huffman_set(h) for h in sets), np.uint8).reshape(len(sets), -1))
    htab_index = dev(np.array([sets.index(i.huffman) for i in infos], np.int32))
    status = torch.empty(F, dtype=torch.int32, device=DEV)
    n_seg = K.jpeg_decode_segments(H, W, sub, ri)
    seg_begin, seg_end = K.jpeg_find_segments(data, scan_begin, scan_end, n_seg, status)
    serial = K.jpeg_decode_coeffs(data, seg_begin, seg_end, H, W, sub, ri, htabs, htab_index, status)
    flags = torch.full((3 * F,), PATTERN, dtype=torch.int32, device=DEV)
    got = K.jpeg_decode_coeffs_sync(data, seg_begin, seg_end, H, W, sub, ri, htabs, htab_index, sub_bytes, flags[F:2 * F], flags[2 * F:], coef=coef)
    assert flags[:F].tolist() == [PATTERN] * F                                  # a status next to clean is not touched
    longest = int((seg_end - seg_begin).max())
    return got, serial, status, flags[F:2 * F].tolist(), flags[2 * F:].tolist(), longest


def check(streams, sub_bytes):
    """the parallel launch == the serial launch == the restatement; clean all 1; rounds within the bound"""
    got, serial, status, clean, rounds, longest = launch(streams, sub_bytes)
    assert status.tolist() == [0] * len(streams) and clean == [1] * len(streams), (clean, status.tolist())
    assert got.dtype == torch.int16 and got.shape == serial.shape and torch.equal(got, serial)
    for f, s in enumerate(streams):
        assert torch.equal(got[f].cpu().long(), host(D.decode(s).coef)), f
    bound = min(LANES, max(1, -(-longest // sub_bytes)))
    assert all(1 <= r <= bound for r in rounds), (rounds, bound)
    return rounds


@pytest.mark.parametrize("sub_bytes", [16, 128])
@pytest.mark.parametrize("sub", SUBS)
def test_grid_through_the_kernel(sub, sub_bytes):
    """our streams as one segment and as one MCU row per segment, the flat frame and noise, Pillow's optimised tables"""
    pytest.importorskip("PIL.Image")
    for h, w in ((9, 7), (33, 47), (120, 184)):
        a = R.sample_image(h, w)
        for q in (50, 100):
            for ri in (65535, R.geometry(h, w, sub)[3]):
                check([R.encode(a, q, sub, ri)], sub_bytes)
    code = {"444": 0, "420": 2}[sub]
    flat = np.full((120, 184, 3), 77, np.uint8)
    worst = 0
    for a in (noise_image(), flat):
        worst = max(worst, *check([R.encode(a, 90, sub, 65535)], sub_bytes), *check([pillow_stream(a, quality=85, subsampling=code, optimize=True)], sub_bytes))
    check([pillow_stream(R.sample_image(120, 184), quality=85, subsampling=code, optimize=True)], sub_bytes)
    print(f"{sub} sub_bytes {sub_bytes}: most rounds on noise and flat frames {worst}")


def test_small_cases():
    """split FF | 00 pairs (counted from the bytes), both endings, at least three chunks, segments shorter than one subsequence, one-MCU frames; every sub_bytes the
    entry takes on one stream"""
    a = R.sample_image(120, 184)
    for sub in SUBS:
        s = R.encode(a, 100, sub, 65535)
        b, e = jpeg.parse_jpeg(s).scan
        for sub_bytes in (16, 128):
            assert sum(1 for p in range(b + sub_bytes, e, sub_bytes) if s[p] == 0 and s[p - 1] == 0xff) >= 1
            check([s], sub_bytes)
    s = R.encode(a, 100, "444", 65535)
    b, e = jpeg.parse_jpeg(s).scan
    assert e - b >= 3 * 16 * LANES                                              # three chunks at sub_bytes 16
    whole, padded = R.encode(a, 50, "444", 65535), R.encode(a, 50, "420", 65535)       # tests/test_jpeg_sync_cpu.py counts their padding bits: 0 and 1 .. 7
    for sub_bytes in K.JPEG_SYNC_SUB_BYTES:
        check([whole], sub_bytes)
        check([padded], sub_bytes)
    for sub in SUBS:
        for ri in (1, 3):
            s = R.encode(R.sample_image(33, 47), 50, sub, ri)
            begins, ends, _ = D.segment_ranges(s)
            assert max(e - b for b, e in zip(begins, ends)) < 256
            assert check([s], 256) == [1]                                       # one subsequence per segment: one round
            check([s], 16)
    for sub, size in (("420", (16, 16)), ("420", (9, 7)), ("444", (8, 8))):
        for sub_bytes in (16, 256):
            check([R.encode(R.sample_image(*size), 90, sub, 65535)], sub_bytes)
            check([R.encode(np.zeros(size + (3,), np.uint8), 50, sub, 65535)], sub_bytes)


def test_store_guard():
    """a coefficient buffer with guard words before and after it keeps them, on the three damaged streams and on three valid ones; a damaged frame is not vouched for"""
    cases = [(s, False) for s, _, _ in D.damaged_streams().values()]
    cases += [(R.encode(R.sample_image(33, 47), 90, "420", 65535), True), (R.encode(R.sample_image(33, 47), 100, "444", 5), True),
              (R.encode(noise_image(48, 80), 90, "420", 65535), True)]
    for s, valid in cases:
        info = jpeg.parse_jpeg(s)
        rows, cols, bpm, _ = K.jpeg_geometry(info.height, info.width, info.subsampling)
        n = rows * cols * bpm * 64
        for sub_bytes in (16, 128):
            buf = torch.full((4096 + n + 4096,), 0x5a5a, dtype=torch.int16, device=DEV)
            got, serial, status, clean, _, _ = launch([s], sub_bytes, coef=buf[4096:4096 + n].view(1, rows * cols, bpm, 64))
            assert bool((buf[:4096] == 0x5a5a).all()) and bool((buf[4096 + n:] == 0x5a5a).all())
            assert clean == [1 if valid else 0] and (status.tolist() == [0]) == valid
            if valid:
                assert torch.equal(got, serial)
            assert not bool((got == 0x5a5a).all(-1).any())                      # every block was written: zeros at the least
    with pytest.raises(ValueError, match="sub_bytes"):
        launch([cases[3][0]], 48)
    with pytest.raises(ValueError, match="coef"):
        launch([cases[3][0]], 128, coef=torch.zeros(1, 9, 6, 32, dtype=torch.int16, device=DEV))


def test_batches_and_reproducibility():
    """three frames with a table set each, alone, in a batch and twice: the same bits"""
    pytest.importorskip("PIL.Image")
    for sub, code in (("420", 2), ("444", 0)):
        streams = [pillow_stream(R.sample_image(120, 184, seed), quality=q, subsampling=code, optimize=True) for seed, q in enumerate((85, 40, 95))]
        assert len({jpeg.parse_jpeg(s).huffman for s in streams}) == 3 and jpeg.parse_jpeg(streams[0]).restart_interval == 0
        batch = launch(streams, 128)
        assert batch[3] == [1, 1, 1] and torch.equal(batch[0], batch[1])
        again = launch(streams, 128)
        assert torch.equal(again[0], batch[0]) and again[4] == batch[4]
        for f in range(3):
            alone = launch(streams[f:f + 1], 128)
            assert torch.equal(alone[0][0], batch[0][f]) and alone[4] == batch[4][f:f + 1]
        check(streams, 64)


def test_decode_jpeg_on_pillow_streams(monkeypatch):
    """marker-less Pillow streams: entropy "sync" == "segment" == "auto" == the restated RGB bytes, and "sync" never reaches the serial launch: no fallback"""
    pytest.importorskip("PIL.Image")
    for sub, code in (("420", 2), ("444", 0)):
        streams = [pillow_stream(R.sample_image(120, 184, seed), quality=q, subsampling=code, optimize=opt) for seed, (q, opt) in enumerate(((85, True), (40, False), (95, True)))]
        assert jpeg.entropy_plan(120, 184, sub, 0)[0] == "sync" and all(jpeg.parse_jpeg(s).restart_interval == 0 for s in streams)
        want = jpeg.decode_jpeg(streams, entropy="segment")
        assert torch.equal(want.cpu(), host(np.stack([D.decode(s).rgb for s in streams])))
        with monkeypatch.context() as m:
            m.setattr(K, "jpeg_decode_coeffs", lambda *a, **k: pytest.fail("a valid stream fell back to the serial launch"))
            assert torch.equal(jpeg.decode_jpeg(streams, entropy="sync"), want) and torch.equal(jpeg.decode_jpeg(streams), want)
            assert torch.equal(jpeg.decode_jpeg(streams[1]), want[1:2])
    # with restart markers "sync" is still the same picture; "auto" takes the serial launch for short segments
    s = R.encode(R.sample_image(48, 80), 90, "420", 2)
    assert jpeg.entropy_plan(48, 80, "420", 2) == ("segment", None)
    assert torch.equal(jpeg.decode_jpeg([s], entropy="sync"), jpeg.decode_jpeg([s])) and torch.equal(jpeg.decode_jpeg([s]).cpu()[0], host(D.decode(s).rgb))


def test_what_the_serial_decoder_accepts_still_decodes():
    """junk behind the last MCU: the serial decoder never reads it, the parallel one does not vouch for the frame, decode_jpeg falls back and returns the picture"""
    s = R.encode(R.sample_image(33, 47), 90, "420", 65535)
    junk = s[:-2] + b"\x12\x34\x56\x78\x9a" + s[-2:]
    got, serial, status, clean, _, _ = launch([junk], 16)
    assert status.tolist() == [0] and clean == [0]
    for entropy in ("auto", "sync", "segment"):
        assert torch.equal(jpeg.decode_jpeg([junk], entropy=entropy).cpu()[0], host(D.decode(s).rgb))


def test_damaged_streams_raise_what_the_serial_path_raises():
    """the three damaged frames between two sound ones: "auto" and "sync" raise what "segment" raises: message, .status and .frames"""
    for name, (bad, want, ri) in D.damaged_streams().items():
        good = [R.encode(R.sample_image(33, 47, seed), 90, "420", ri) for seed in (1, 2)]
        with pytest.raises(jpeg.JpegDecodeError) as ref:
            jpeg.decode_jpeg([good[0], bad, good[1]], entropy="segment")
        assert ref.value.status.tolist() == [0, want, 0]
        for entropy in ("auto", "sync"):
            with pytest.raises(jpeg.JpegDecodeError) as e:
                jpeg.decode_jpeg([good[0], bad, good[1]], entropy=entropy)
            assert str(e.value) == str(ref.value) and torch.equal(e.value.status, ref.value.status) and torch.equal(e.value.frames, ref.value.frames), (name, entropy)
    assert jpeg.entropy_plan(33, 47, "420", 65535)[0] == "sync"                # the flipped frame went through the parallel launch under "auto"


def test_load_video_of_pillow_encoded_frames(tmp_path):
    """an AVI of Pillow-encoded frames (no restart markers), written through MJPEGWriter.write_jpegs -> load_video == prepare_video of the restated frames"""
    pytest.importorskip("PIL.Image")
    H, W = 48, 80
    streams = [pillow_stream(R.sample_image(H, W, seed), quality=85) for seed in range(12)]
    assert jpeg.parse_jpeg(streams[0]).restart_interval == 0 and jpeg.entropy_plan(H, W, "420", 0)[0] == "sync"
    path = str(tmp_path / "pillow.avi")
    with jpeg.MJPEGWriter(path, 8) as w:
        w.write_jpegs(streams, H, W)
    restated = np.stack([D.decode(s).rgb for s in streams])
    out = video_io.load_video(path, (32, 48), 5, True, -1, 0, -1, 2)
    idx = video_io.sample_frame_indices(12, 8.0, 5, -1, 0, -1, 2)
    assert out.shape == (1, len(idx), 3, 32, 48) and torch.equal(out, video_io.prepare_video(restated[idx], (32, 48), False, True))
    frames, fps = jpeg.read_mjpeg_avi(path)
    assert fps == 8 and torch.equal(frames.cpu(), host(restated))
