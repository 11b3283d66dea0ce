"""GPU: tokensgen_amd.png.decode_png, torch.equal to the source pixels, on the smallest shapes where a kernel of csrc/png_decode.hip can go wrong: our own files by
both routes, Pillow's files, every clean case of tests/png_dec_cases.py, the fallback from "chunk" to "stream", the sequence reader and load_video; and every damaged
case of that list raises PngDecodeError with the status tests/png_dec_ref.py gives (all of them passed the host program under the sanitizers first:
tests/test_png_decode_cpu.py).  Nothing here is meant to fault: a damaged stream is an error return."""
import io
import os
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_dec_cases as C
import png_dec_ref as R
import png_ref
from tokensgen_amd import kernels as K
from tokensgen_amd import png, video_io

pytestmark = pytest.mark.gpu
SIZES = [(1, 1), (1, 2), (2, 1), (3, 5), (33, 47), (17, 86), (160, 85), (1, 21844)]


def sources(H, W, bpp=3):
    flat = np.full((H, W, bpp), 131, np.uint8)
    mixed = C.smooth(H, W, bpp, seed=1)
    mixed[H // 2:] = C.noise(H - H // 2, W, bpp, seed=2)
    return [C.smooth(H, W, bpp, seed=3), C.noise(H, W, bpp, seed=4), flat, mixed]


def pillow_png(frame, **kw):
    Image = pytest.importorskip("PIL.Image")
    buf = io.BytesIO()
    Image.fromarray(frame, "RGB" if frame.shape[2] == 3 else "RGBA").save(buf, "PNG", **kw)
    return buf.getvalue()


def equal(files, frames, **kw):
    out = png.decode_png(files, **kw)
    want = torch.from_numpy(np.stack([f[:, :, :3] for f in frames]))
    assert out.dtype == torch.uint8 and out.is_cuda and out.shape == want.shape
    got = out.cpu()
    if not torch.equal(got, want):
        bad = torch.nonzero((got != want).flatten(1).any(1)).flatten().tolist()
        raise AssertionError(f"frames {bad} differ; the first at {torch.nonzero(got[bad[0]] != want[bad[0]])[0].tolist()}")
    return out


def test_smallest_clean_file_first():
    """one pixel, one stored block: the first contact with the device"""
    frame = np.array([[[7, 130, 255]]], np.uint8)
    equal([R.write_png(frame, level=0)], [frame])


@pytest.mark.parametrize("H,W", SIZES)
def test_our_own_files_by_both_routes(H, W):
    """png_ref's files (every band a dynamic or a stored block and an empty stored block): by "chunk", and the same bytes forced to "stream" """
    frames = sources(H, W)
    rows = [None] if H == 1 else [1, 3, None]
    for r in rows:
        if r is not None and r * (1 + 3 * W) > 65535:
            continue
        files = [png_ref.encode_png(f, rows_per_block=r) for f in frames]
        if len(png.parse_png(files[0]).idat) > 1:                               # a frame of one band is one IDAT: "stream"
            assert png.inflate_plan(files)[0] == "chunk"
            equal(files, frames, inflate="chunk")
        else:
            assert png.inflate_plan(files)[0] == "stream"
        equal(files, frames, inflate="stream")
        equal(files, frames)


def test_short_last_band_and_mixed_band_kinds():
    frame = sources(33, 47)[3]                                                  # smooth bands are dynamic blocks, noisy ones stored; 33 rows in bands of 16: a last band of one row
    data = png_ref.encode_png(frame)
    kinds = {p[2 if k == 0 else 0] & 6 for k, p in enumerate(png.parse_png(data).idat)}
    assert kinds == {0, 4} and png.inflate_plan([data])[0] == "chunk"
    equal([data], [frame], inflate="chunk")
    equal([data], [frame], inflate="stream")


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("bpp", [3, 4])
def test_pillow_files(H, W, bpp):
    frames = sources(H, W, bpp)
    files = [pillow_png(f) for f in frames]
    assert png.inflate_plan(files)[0] == "stream" or H * W * bpp > 60000        # Pillow cuts its IDATs anywhere, every 64 KiB
    equal(files, frames)


@pytest.mark.parametrize("case", C.clean_cases(), ids=lambda c: c.name)
def test_clean_cases(case):
    equal([case.data], [case.frame])
    equal([case.data], [case.frame], inflate="stream")


def test_sync_flushed_file_comes_back_through_the_fallback():
    frame = np.tile(C.smooth(8, 47, seed=3), (4, 1, 1))
    sync = R.write_png(frame, [0] * 32, flush=zlib.Z_SYNC_FLUSH, pieces=4)
    full = R.write_png(frame, [y % 5 for y in range(32)], flush=zlib.Z_FULL_FLUSH, pieces=4)
    assert png.inflate_plan([sync])[0] == "chunk" and R.decode_chunks(sync)[1] & R.NOT_INDEPENDENT and R.decode_chunks(full)[1] == 0
    equal([sync], [frame])
    equal([full], [frame], inflate="chunk")
    equal([full, sync, full], [frame] * 3)                                      # one frame of the call sends the whole call to "stream"


def test_six_frames_at_unaligned_offsets():
    frames = [C.smooth(33, 47, seed=s) if s % 2 else C.noise(33, 47, seed=s) for s in range(6)]
    files = [R.write_png(f, [(y + s) % 5 for y in range(33)], level=1 + s) for s, f in enumerate(frames)]
    assert len({len(f) % 16 for f in files}) > 1
    equal(files, frames)
    own = [png_ref.encode_png(f, rows_per_block=5) for f in frames]
    equal(own, frames)
    equal(list(reversed(own)), list(reversed(frames)), inflate="chunk")


def test_round_trip_on_the_device():
    frames = torch.from_numpy(np.stack(sources(33, 47) + sources(33, 47)[::-1])).cuda()
    data, offsets = png.encode_png(frames)
    assert torch.equal(png.decode_png(data, offsets), frames)
    assert torch.equal(png.decode_png(data, offsets, inflate="stream"), frames)
    assert torch.equal(png.decode_png(data.cpu(), offsets.tolist(), device="cuda"), frames)
    assert torch.equal(png.decode_png(png.png_bytes(frames, "paeth", 2)), frames)


def test_sequence_reader_and_load_video(tmp_path):
    frames = torch.from_numpy(np.stack([C.smooth(48, 80, seed=s) for s in range(12)])).cuda()
    pattern = str(tmp_path / "frame_{:04d}.png")
    png.save_png_sequence(frames, pattern, start=3)
    assert torch.equal(png.load_png(pattern.format(5)), frames[2])
    assert torch.equal(png.load_png_sequence(pattern, start=3), frames) and torch.equal(png.load_png_sequence(pattern, start=5, count=4), frames[2:6])
    with png.PNGSequenceReader(pattern, fps=12, start=3) as r:
        assert len(r) == 12 and r.size == (48, 80) and r.fps == 12
        idx = [5, 0, 5, -1, 11, 0]
        assert torch.equal(r.get_batch(idx), frames[idx]) and torch.equal(r.read(2, 9), frames[2:9])
    png.save_png_sequence(frames, pattern)                                      # from 0: what load_video reads
    for crop, fps in ((False, -1), (True, 4)):
        out = video_io.load_video(pattern, (32, 48), 5, True, fps, 0, -1, 2, crop_to_fit=crop)
        idx = video_io.sample_frame_indices(12, 8.0, 5, fps, 0, -1, 2)
        assert out.shape == (1, len(idx), 3, 32, 48) and torch.equal(out, video_io.prepare_video(frames[idx], (32, 48), crop, True))
    out = video_io.load_image_sequence(pattern, (32, 48), 5, True, -1, 0, -1, 2, fps=4, start=2)
    assert torch.equal(out, video_io.prepare_video(frames[2:][video_io.sample_frame_indices(10, 4.0, 5, -1, 0, -1, 2)], (32, 48), False, True))


@pytest.mark.parametrize("case", C.damaged_cases(), ids=lambda c: c.name)
def test_damaged_cases_raise(case):
    """an error return with the restatement's status, alone and as frame 1 of three; never a fault"""
    with pytest.raises(png.PngDecodeError, match="frame 0: ") as e:
        png.decode_png([case.data])
    assert e.value.status.tolist() == [case.status] and e.value.frames.shape[0] == 1
    for bit, text in K.PNG_STATUS.items():
        assert (text in str(e.value)) == bool(case.status & bit)
    H, W, _, _ = R.read_container(case.data)
    good = R.write_png(C.smooth(H, W, seed=1), cuts=[3])
    with pytest.raises(png.PngDecodeError, match="frame 1: ") as e:
        png.decode_png([good, case.data, good])
    assert e.value.status.tolist() == [0, case.status, 0]
    assert torch.equal(e.value.frames[0].cpu(), torch.from_numpy(C.smooth(H, W, seed=1))) and torch.equal(e.value.frames[0], e.value.frames[2])


def test_a_damaged_band_of_our_own_file():
    """the chunk route's verdict sends the call to "stream", whose status is the answer"""
    frame = C.smooth(33, 47, seed=1)
    data = png_ref.encode_png(frame, rows_per_block=3)
    at = data.index(b"IDAT", data.index(b"IDAT") + 4) + 9
    hurt = bytearray(data)
    hurt[at] ^= 0x40
    pos, chunks = 8, []
    while pos < len(hurt):
        n = int.from_bytes(hurt[pos:pos + 4], "big")
        chunks.append((bytes(hurt[pos + 4:pos + 8]), bytes(hurt[pos + 8:pos + 8 + n])))
        pos += 12 + n
    hurt = R.SIGNATURE + b"".join(R.chunk(k, p) for k, p in chunks)
    want = R.decode(hurt)[1]
    assert want and png.inflate_plan([hurt])[0] == "chunk"
    with pytest.raises(png.PngDecodeError, match="frame 1: ") as e:
        png.decode_png([data, hurt])
    assert e.value.status.tolist() == [0, want] and torch.equal(e.value.frames[0].cpu(), torch.from_numpy(frame))


def test_a_range_outside_the_buffer_is_status_512():
    """the kernel checks a piece's range and frame index before it reads a byte"""
    frame = C.smooth(3, 5, seed=1)
    z = b"".join(png.parse_png(R.write_png(frame)).idat)
    data = torch.frombuffer(bytearray(z), dtype=torch.uint8).cuda()
    filtered = torch.zeros(1, 3 * 16, dtype=torch.uint8, device="cuda")
    i64, i32 = lambda v: torch.tensor(v, dtype=torch.int64, device="cuda"), lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")
    for begin, end, fr in [(2, len(z) + 1, 0), (-1, len(z) - 4, 0), (9, 8, 0), (2, len(z) - 4, 1), (2, len(z) - 4, -1)]:
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        K.png_inflate(data, (i64([begin]), i64([end]), i32([fr]), i32([1])), "stream", filtered, 3, 5, 3, status)
        assert status.tolist() == [512] and not bool(filtered.any())
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    K.png_inflate(data, (i64([2]), i64([len(z) - 4]), i32([0]), i32([1])), "stream", filtered, 3, 5, 3, status)
    assert status.tolist() == [0] and filtered.cpu().numpy().tobytes() == zlib.decompress(z)
