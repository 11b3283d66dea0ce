"""CPU: the definitions of block-matching motion (tests/motion_ref.py) on inputs with known answers, mutations of those definitions that the inputs must notice,
motion.summarize against hand-computed numbers, and every refusal of the public interface, raised before any kernel call.  No GPU."""
import math

import pytest
import torch

import motion_ref as R
from tokensgen_amd import metrics, motion


@pytest.fixture(scope="module")
def known():
    """name -> (frames, block, radius, reference result), computed once"""
    out = {}
    for name, make in R.KNOWN.items():
        frames, block, radius = make()
        out[name] = (frames, block, radius, R.block_motion(frames, block, radius))
    return out


def test_shifted_texture(known):
    frames, block, radius, r = known["shifted_texture"]
    assert frames.shape == (2, 43, 61, 3) and (block, radius) == (8, 7) and r["mv"].shape == (1, 5, 7, 2) and r["mv"].dtype == torch.int16
    assert (frames[1] == 0).sum() > 500                       # zero bytes in the reference frame
    mv, sad = r["mv"][0], r["sad"][0]
    inside = torch.zeros(5, 7, dtype=torch.bool)
    for by in range(5):
        for bx in range(7):
            y, x = by * 8 + 3, bx * 8 - 5
            inside[by, bx] = 0 <= y and y + 8 <= 43 and 0 <= x and x + 8 <= 61
    assert int(inside.sum()) == 30 and torch.equal(inside, torch.tensor([[False] + [True] * 6] * 5))
    hit = (mv[..., 0] == 3) & (mv[..., 1] == -5) & (sad == 0)
    assert torch.equal(hit, inside)                           # exactly the blocks whose displaced block lies inside the frame
    assert (sad[~inside] > 0).all() and (r["sad0"][0] > 0).all()


def test_constant_frames(known):
    _, _, _, r = known["constant_frames"]
    assert r["mv"].shape == (1, 3, 5, 2) and not r["mv"].any() and not r["sad"].any() and not r["sad0"].any()


def test_black_against_white(known):
    _, _, _, r = known["black_white"]
    assert r["mv"].tolist() == [[[[0, 0]]]] and r["sad"].tolist() == [[[65280]]] and r["sad0"].tolist() == [[[65280]]]
    assert r["sad"].dtype == torch.int32 and r["sad0"].dtype == torch.int32


def test_period_four_stripes(known):
    frames, block, radius, r = known["stripes"]
    y = R.luma(frames)
    cur, ref = y[0, 8:16, 16:24], y[1]
    for dx in (1, -3, 5):
        assert int((cur - ref[8:16, 16 + dx:24 + dx]).abs().sum()) == 0
    assert int((cur - ref[8:16, 16:24]).abs().sum()) > 0
    inner = r["mv"][0, :, 1:-1]                               # blocks that admit dx = 1 (all but the last column) and more: the shortest vector wins
    assert (inner[..., 0] == 0).all() and (inner[..., 1] == 1).all() and not r["sad"][0, :, :-1].any()
    assert (r["mv"][0, :, -1, 1] == -3).all()                 # the last column of blocks cannot move right: x + 1 + 8 > 48


def test_hand_built_four_way_tie(known):
    frames, block, radius, r = known["hand_built"]
    y = R.luma(frames)
    cost = lambda dy, dx: int((y[0, 8:16, 8:16] - y[1, 8 + dy:16 + dy, 8 + dx:16 + dx]).abs().sum())
    assert [cost(*v) for v in ((-1, 0), (0, -1), (0, 1), (1, 0))] == [600] * 4 and cost(0, 0) == 1000
    assert min(cost(dy, dx) for dy in range(-3, 4) for dx in range(-3, 4)) == 600
    assert r["mv"][0, 1, 1].tolist() == [-1, 0] and int(r["sad"][0, 1, 1]) == 600 and int(r["sad0"][0, 1, 1]) == 1000
    assert r["mv"][0, 0, 0].tolist() == [0, 0] and int(r["sad"][0, 0, 0]) == 77 * (64 - 25)


def test_diagonal_stripes_prefer_the_euclidean_shortest(known):
    _, _, _, r = known["diagonal_stripes"]
    assert r["mv"][0, 1:4, 1:4].reshape(-1, 2).tolist() == [[-2, 2]] * 9 and not r["sad"][0, 1:4, 1:4].any()


@pytest.mark.parametrize("variant", ["luma_no_round", "l1", "raster", "clamp"])
def test_mutations_are_noticed(known, variant):
    """a wrong rule must change mv or sad on at least one known-answer input, otherwise the inputs are too weak"""
    changed = []
    for name, (frames, block, radius, good) in known.items():
        bad = R.block_motion(frames, block, radius, variant=variant)
        if not (torch.equal(bad["mv"], good["mv"]) and torch.equal(bad["sad"], good["sad"])):
            changed.append(name)
    print(variant, "changes", changed)
    assert changed


def test_reference_batches_refs_and_warp():
    g = torch.Generator().manual_seed(5)
    v = torch.randint(0, 256, (2, 3, 19, 27, 3), generator=g, dtype=torch.uint8)
    r = R.block_motion(v, 8, 3)
    assert r["mv"].shape == (2, 2, 2, 3, 2)
    for b in range(2):                                        # no pair crosses batch items
        one = R.block_motion(v[b], 8, 3)
        assert all(torch.equal(r[k][b], one[k]) for k in r)
    pr = R.block_motion(v[0], 8, 3, ref=v[1])
    assert pr["mv"].shape == (3, 2, 3, 2) and torch.equal(pr["sad0"][1], R.block_motion(torch.stack([v[0, 1], v[1, 1]]), 8, 3)["sad0"][0])
    # warp error: own vectors are never clamped, sse <= sse0 need not hold per block but sse0 is the plain squared difference
    w = R.warp_sse(v, r["mv"], 8)
    assert int(w["status"]) == 0 and w["sse"].shape == (2, 2, 2, 3)
    d = (v[0, 0, :8, 8:16].long() - v[0, 1, :8, 8:16].long()) ** 2
    assert int(w["sse0"][0, 0, 0, 1]) == int(d.sum())
    mv = torch.zeros_like(r["mv"])
    mv[1, 0, 1, 2] = torch.tensor([5, -30], dtype=torch.int16)          # block at (8, 16): (13, -14) -> clamped to (11, 0)
    w2 = R.warp_sse(v, mv, 8)
    d = (v[1, 0, 8:16, 16:24].long() - v[1, 1, 11:19, 0:8].long()) ** 2
    assert int(w2["status"]) == 1 and int(w2["sse"][1, 0, 1, 2]) == int(d.sum()) and torch.equal(w2["sse0"], w["sse0"])


def test_summarize_hand_computed():
    mv = torch.zeros(2, 2, 3, 2, dtype=torch.int16)
    mv[0, 0, 1] = torch.tensor([3, -4])
    mv[0, 1, 2] = torch.tensor([0, 2])
    sad = torch.arange(12, dtype=torch.int32).reshape(2, 2, 3) * 100
    sad0 = sad + 255
    s = motion.summarize(mv, sad, sad0, 8, top_fraction=0.05)
    assert all(v.dtype == torch.float64 and v.shape == (2,) for v in s.values())
    assert s["magnitude"].tolist() == [7.0 / 6, 0.0] and s["magnitude_top"].tolist() == [5.0, 0.0]           # ceil(0.05 * 6) = 1 block
    assert s["static_fraction"].tolist() == [4.0 / 6, 1.0]
    norm = 255.0 * 6 * 64
    assert s["residual"].tolist() == [1500 / norm, 5100 / norm] and s["flicker"].tolist() == [(1500 + 6 * 255) / norm, (5100 + 6 * 255) / norm]
    assert motion.summarize(mv, sad, sad0, 8, top_fraction=0.2)["magnitude_top"].tolist() == [3.5, 0.0]       # ceil(1.2) = 2 blocks: (5 + 2) / 2
    assert motion.summarize(mv, sad, sad0, 8, top_fraction=1.0)["magnitude_top"].tolist() == [7.0 / 6, 0.0]
    assert [motion.top_count(f, n) for f, n in ((0.05, 6), (0.05, 20), (0.05, 21), (0.05, 60), (0.05, 1350), (0.5, 3), (1.0, 7))] == [1, 1, 2, 3, 68, 2, 7]
    assert motion.top_count(0.07, 100) == math.ceil(7.000000000000001 - 1e-9) == 7        # 0.07 * 100 lands above 7 in float64: the guard keeps it at 7
    # a one-block frame, block 16
    one = motion.summarize(torch.tensor([[[[-6, 8]]]], dtype=torch.int16), torch.tensor([[[510]]], dtype=torch.int32), torch.tensor([[[65280]]], dtype=torch.int32), 16)
    assert {k: v.tolist() for k, v in one.items()} == {"magnitude": [10.0], "magnitude_top": [10.0], "static_fraction": [0.0], "flicker": [1.0],
                                                       "residual": [510 / (255.0 * 256)]}
    with pytest.raises(ValueError):
        motion.summarize(mv, sad[:1], sad0, 8)
    with pytest.raises(ValueError):
        motion.summarize(mv, sad, sad0, 4)
    with pytest.raises(ValueError):
        motion.summarize(mv, sad, sad0, 8, top_fraction=0.0)


def test_refusals_come_before_any_kernel_call():
    """on CPU tensors: a call that reached a kernel wrapper would raise RuntimeError (no CPU path), so every ValueError / NotImplementedError here was raised first"""
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    ok = u8(3, 32, 48, 3)
    calls = [lambda f, **kw: motion.block_motion(f, **kw), lambda f, **kw: metrics.video_motion(f, **kw), lambda f, **kw: metrics.video_warp_error(f, **kw)]
    for call in calls:
        with pytest.raises(NotImplementedError):
            call(ok.float())
        with pytest.raises(NotImplementedError):
            call(ok.to(torch.bfloat16))
        for bad in (u8(1, 32, 48, 3), u8(2, 1, 32, 48, 3), u8(3, 32, 48), u8(3, 3, 32, 48), u8(3, 32, 48, 4), u8(0, 32, 48, 3)):
            with pytest.raises(ValueError):
                call(bad)
        for kw in (dict(block=4), dict(block=32), dict(block=12), dict(block=16.0), dict(radius=0), dict(radius=33), dict(radius=2.5), dict(radius=-1)):
            with pytest.raises(ValueError):
                call(ok, **kw)
        with pytest.raises(ValueError):
            call(u8(3, 15, 48, 3), block=16)
        with pytest.raises(ValueError):
            call(u8(3, 32, 7, 3), block=8)
        with pytest.raises(RuntimeError, match="GPU"):          # a valid call reaches the kernels, and those have no CPU path
            call(ok)
    with pytest.raises(ValueError):
        motion.block_motion(ok, ref=u8(3, 32, 40, 3))
    with pytest.raises(NotImplementedError):
        motion.block_motion(ok, ref=ok.float())
    with pytest.raises(ValueError):
        metrics.video_warp_error(ok, motion_from=u8(4, 32, 48, 3))
    with pytest.raises(NotImplementedError):
        metrics.video_warp_error(ok, motion_from=ok.float())
    with pytest.raises(ValueError):
        metrics.video_motion(ok, top_fraction=0.0)
    assert motion.block_motion.__defaults__ == (16, 16, None)
    # warp_sse: the vectors must describe the frames' blocks
    mv = torch.zeros(2, 2, 3, 2, dtype=torch.int16)
    for bad in (mv.int(), mv[..., :1], torch.zeros(2, 2, 4, 2, dtype=torch.int16), torch.zeros(3, 2, 3, 2, dtype=torch.int16), mv[0]):
        with pytest.raises(ValueError):
            motion.warp_sse(ok, bad)
    with pytest.raises(NotImplementedError):
        motion.warp_sse(ok.float(), mv)
    with pytest.raises(RuntimeError, match="GPU"):
        motion.warp_sse(ok, mv)
    # the streaming class
    with pytest.raises(ValueError):
        metrics.VideoMotion(block=12)
    with pytest.raises(ValueError):
        metrics.VideoMotion(radius=40)
    vm = metrics.VideoMotion(block=16, radius=4)
    with pytest.raises(ValueError):
        vm.update(u8(1, 3, 32, 48, 3))
    with pytest.raises(NotImplementedError):
        vm.update(ok.float())
    with pytest.raises(ValueError):
        vm.update(ok, motion_from=u8(2, 32, 48, 3))
    with pytest.raises(RuntimeError):
        vm.finalize()
    vm.update(u8(1, 32, 48, 3))                                 # one frame: carried, no pair yet, no kernel
    with pytest.raises(ValueError):
        vm.new_video()                                          # a video of one frame
    import sys
    assert "longvgen" not in sys.modules or not hasattr(sys.modules["longvgen"], "motion")
