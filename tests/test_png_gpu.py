"""GPU: tokensgen_amd.png.encode_png against tests/png_ref.py, byte for byte, and the files decoded again by png_ref's decoder (zlib.decompress and the filters undone
in numpy), on the smallest shapes where a kernel of csrc/png.hip can go wrong."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_ref as P
from tokensgen_amd import png

pytestmark = pytest.mark.gpu


def noise(shape, seed=0):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def smooth(H, W, seed=0):
    """gradients with a little noise: long and short runs, every filter type somewhere"""
    y, x = np.mgrid[0:H, 0:W]
    f = np.stack([2 * x + y, 255 - x // 2, (x * y) // 7 + 3 * seed], -1)
    f[H // 3:, W // 4:W // 2] = 40 + seed                                        # a flat patch
    f[:, 3 * W // 4:] += np.random.default_rng(seed).integers(0, 3, (H, W - 3 * W // 4, 3))
    return (f & 255).astype(np.uint8)


def mixed(H, W):
    """flat bands and noisy bands in one frame"""
    f = np.full((H, W, 3), 200, np.uint8)
    f[H // 4:H // 2] = noise((H // 2 - H // 4, W, 3), 5)
    f[3 * H // 4:] = smooth(H - 3 * H // 4, W, 2)
    return f


def check(frames, filter="adaptive", rows_per_block=None, decode=True):
    """frames uint8 [..., H, W, 3] (numpy): the device's bytes and offsets are the restatement's; the files decode to the frames"""
    dev = torch.from_numpy(frames).cuda()
    data, offsets = png.encode_png(dev, filter, rows_per_block)
    want, want_offsets = P.encode_clip(frames, filter=filter, rows_per_block=rows_per_block)
    assert offsets.dtype == torch.int64 and not offsets.is_cuda and offsets.tolist() == want_offsets.tolist()
    assert data.dtype == torch.uint8 and data.is_cuda and data.dim() == 1
    got = data.cpu()
    if not torch.equal(got, torch.from_numpy(want.copy())):
        bad = np.flatnonzero(got.numpy() != want)
        raise AssertionError(f"{len(bad)} of {len(want)} bytes differ, the first at {bad[0]} (frame {np.searchsorted(want_offsets, bad[0], 'right') - 1})")
    if decode:
        flat = frames.reshape(-1, *frames.shape[-3:])
        o = offsets.tolist()
        for i in range(len(flat)):
            assert np.array_equal(P.decode_png(got.numpy()[o[i]:o[i + 1]].tobytes()), flat[i])
    return got.numpy(), offsets


@pytest.mark.parametrize("H,W", [(1, 1), (1, 2), (2, 1), (3, 5), (33, 47), (17, 86)])
def test_sizes(H, W):
    """(17, 86): a row is 259 bytes, a flat one a literal and one match of exactly 258"""
    check(np.stack([smooth(H, W), noise((H, W, 3)), np.full((H, W, 3), 131, np.uint8), np.zeros((H, W, 3), np.uint8)]))


def test_widest_row():
    """H = 1 at W = 21844: one band of 65533 bytes, two short of the limit of a stored block; smooth (dynamic) and noise (stored)"""
    W = P.MAX_WIDTH
    assert P.geometry(1, W)[3] == 65533 and P.geometry(1, W)[0] == 1
    check(np.stack([smooth(1, W), noise((1, W, 3))]))


@pytest.mark.parametrize("H,W,rest", [(1, 86, 0), (2, 43, 1), (3, 86, 2), (1, 87, 3)])
def test_flat_remainders(H, W, rest):
    """a frame of zeros under "none" is one run of H (1 + 3 W) bytes in one band: after the literal and the matches of 258, `rest` bytes remain"""
    frame = np.zeros((1, H, W, 3), np.uint8)
    _, lengths = P.runs(P.filter_frame(frame[0], "none").reshape(-1))
    assert len(lengths) == 1 and (lengths[0] - 1) % 258 == rest
    check(frame, "none", H)
    check(frame)


def test_noise_is_stored():
    frames = noise((2, 33, 47, 3), 3)
    data, offsets = check(frames)
    bands, row = P.geometry(33, 47)[1:3]
    assert len(data) == offsets[-1] == 2 * (33 * row + 17 * bands + 53)         # nothing to gain: every band is one stored block


def test_flat_and_noisy_bands():
    check(mixed(40, 52)[None], rows_per_block=5)
    check(mixed(40, 52)[None])


@pytest.mark.parametrize("rows_per_block", [1, 3, None])
def test_rows_per_block(rows_per_block):
    """H = 35 is no multiple of 1 .. 16 but 1: the last band is short"""
    check(np.stack([smooth(35, 29), mixed(35, 29)]), rows_per_block=rows_per_block)


@pytest.mark.parametrize("filter", P.FILTERS)
def test_forced_filters(filter):
    check(np.stack([smooth(19, 23), noise((19, 23, 3), 1)]), filter)


def test_batch_offsets_and_alignment():
    """three different frames in one call, the same frames as [B, T, ...], and every frame alone: the same bytes; files start at aligned and at unaligned offsets"""
    frames = np.stack([smooth(21, 34, 0), mixed(21, 34), noise((21, 34, 3), 2), smooth(21, 34, 1), np.zeros((21, 34, 3), np.uint8), smooth(21, 34, 4)])
    data, offsets = check(frames)
    starts = offsets[:-1].numpy() % 4
    assert (starts == 0).sum() >= 2 and (starts != 0).any(), starts
    check(frames[:3])
    data5, offsets5 = check(frames.reshape(2, 3, 21, 34, 3), decode=False)
    assert np.array_equal(data5, data) and torch.equal(offsets5, offsets)
    o = offsets.tolist()
    for i in (1, 4):
        alone, _ = check(frames[i:i + 1], decode=False)
        assert np.array_equal(alone, data[o[i]:o[i + 1]])


def test_files_and_views(tmp_path):
    """png_bytes, save_png, save_png_sequence and a view that is not contiguous"""
    frames = np.stack([smooth(12, 20, s) for s in range(3)])
    dev = torch.from_numpy(frames).cuda()
    files = png.png_bytes(dev)
    assert files == [P.encode_png(f) for f in frames]
    assert open(png.save_png(dev[1], str(tmp_path / "one.png"), "paeth", 5), "rb").read() == P.encode_png(frames[1], "paeth", 5)
    paths = png.save_png_sequence(dev, str(tmp_path / "f_{:03d}.png"), start=7)
    assert [os.path.basename(p) for p in paths] == ["f_007.png", "f_008.png", "f_009.png"] and [open(p, "rb").read() for p in paths] == files
    view = dev[:, ::2, 1:-1]
    assert png.png_bytes(view) == [P.encode_png(f) for f in frames[:, ::2, 1:-1]]
