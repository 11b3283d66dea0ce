"""CPU: the definitions of motion-compensated interpolation (tests/mci_ref.py) on inputs with known answers, wrong rules that those inputs must
notice, every refusal of the public interface (raised before any kernel call), the untouched default of VideoProcessor and the argument checks of the two exports.
No GPU.  The kernels are held to the restatement in tests/test_mci_gpu.py."""
import ctypes

import pytest
import torch

import mci_ref as R
import motion_ref as MR
from tokensgen_amd import metrics, motion, video_io

RADIUS = 12          # holds the largest total motion of the translating textures, (6, 10)
TEXTURES = [(block, step) for block in (8, 16) for step in ((2, -4), (3, 5))]


@pytest.fixture(scope="module")
def textures():
    """(block, step, bidirectional) -> (the three frames, the interpolation of frames 0 and 2 at 1 / 2), computed once"""
    out = {}
    for block, step in TEXTURES:
        f = R.translating_texture(block, step)
        for bi in (True, False):
            out[block, step, bi] = (f, R.interpolate_frames(f[::2], 2, block, RADIUS, bi))
    return out


@pytest.mark.parametrize("bi", [True, False])
@pytest.mark.parametrize("block,step", TEXTURES)
def test_translating_texture_gives_back_the_held_out_frame(textures, block, step, bi):
    f, r = textures[block, step, bi]
    H, W = 6 * block + 3, 8 * block + 5
    assert f.shape == (3, H, W, 3) and r["video"].shape == (3, H, W, 3) and r["video"].dtype == torch.uint8
    assert r["mvi"].shape == (1, 1, 6, 8, 2) and r["mvi"].dtype == torch.int16 and r["cost"].shape == (1, 1, 6, 8) and r["cost"].dtype == torch.int32
    assert torch.equal(r["video"][0], f[0]) and torch.equal(r["video"][2], f[2])                  # the originals, byte for byte
    mid, e = r["video"][1], 2 * block
    assert torch.equal(mid[e:-e, e:-e], f[1][e:-e, e:-e])                                          # exact at least two blocks from every edge
    total = torch.tensor([2 * step[0], 2 * step[1]], dtype=torch.int16)
    assert (r["mvi"][0, 0, 2:-2, 2:-2] == total).all() and not r["cost"][0, 0, 2:-2, 2:-2].any()
    mc, bl = R.psnr(mid, f[1]), R.psnr(R.blend(f[0], f[2]), f[1])
    print(f"block {block} step {step} bidirectional {bi}: cost == 0 in {int((r['cost'] == 0).sum())} of 48 blocks, mc_psnr {mc:.2f} dB, blend_psnr {bl:.2f} dB")
    assert mc > bl


def test_still_video_and_flat_frames():
    g = torch.Generator().manual_seed(31)
    one = torch.randint(0, 256, (1, 27, 37, 3), generator=g, dtype=torch.uint8)
    still = one.expand(3, -1, -1, -1)
    for n in (2, 5):
        r = R.interpolate_frames(still, n, 8, 3)
        assert r["video"].shape == (2 * n + 1, 27, 37, 3) and all(torch.equal(fr, one[0]) for fr in r["video"])
        assert not r["mvi"].any() and not r["cost"].any()
    # all 0 against all 255, factor 4: (1024 * (4 - k) * 0 + 1024 * k * 255 + 2048) // 4096 = (255 k + 2) // 4 -> 64, 128, 191
    bw, block, _ = MR.black_white()
    r = R.interpolate_frames(bw, 4, block, 16)
    want = [(4 * block * block * k * 255 + 2 * 4 * block * block) // (4 * 4 * block * block) for k in (1, 2, 3)]
    assert want == [64, 128, 191]
    assert r["video"].shape == (5, 16, 16, 3) and [int(fr.unique()) for fr in r["video"]] == [0] + want + [255]
    assert r["cost"].flatten().tolist() == [65280] * 3 and not r["mvi"].any()                      # the largest cost; one block admits only (0, 0)


def test_one_block_frame_admits_only_zero():
    g = torch.Generator().manual_seed(32)
    for block in (8, 16):
        f = torch.randint(0, 256, (2, block, block, 3), generator=g, dtype=torch.uint8)
        fake = torch.full((1, 1, 1, 2), 3, dtype=torch.int16)                                      # a field that says (3, 3): no room for it
        r = R.interpolate_frames(f, 3, block, 4, field_pair=(fake, fake))
        assert not r["mvi"].any() and r["mvi"].shape == (1, 2, 1, 1, 2)
        y = MR.luma(f)
        assert r["cost"].flatten().tolist() == [int((y[0] - y[1]).abs().sum())] * 2
        for k in (1, 2):                                                                           # every neighbour clamps to the one block: a plain (3 - k) : k mix
            want = ((3 - k) * f[0].long() + k * f[1].long()) * 4 * block * block
            assert torch.equal(r["video"][k].long(), (want + 6 * block * block) // (12 * block * block))


def test_rnd_by_hand():
    # 1 * (-3) / 2 = -1.5 -> -1 (the half goes up); truncation of (2 k d + n) / (2 n) = -4 / 4 gives the same here, but -5 / 2 -> (-10 + 2) / 4 = -2 both ways and
    # k d / n = -7 / 3 = -2.33 -> (2 * -7 + 3) // 6 = -11 // 6 = -2, truncated -1
    assert R.rnd(1, -3, 2) == -1 and R.rnd(1, 3, 2) == 2 and R.rnd(1, -5, 2) == -2 and R.rnd(1, -1, 2) == 0 and R.rnd(1, 1, 2) == 1
    assert R.rnd(1, -7, 3) == -2 and R.rnd(1, -7, 3, "trunc") == -1
    assert R.rnd(3, -5, 8) == -2 and R.rnd(7, -1, 8) == -1 and R.rnd(4, -1, 8) == 0 and R.rnd(4, 1, 8) == 1            # -1.875, -0.875, -0.5, 0.5
    d = torch.tensor([-7, -4, -3, -2, -1, 0, 1, 2, 3])
    # d / 2 = -3.5, -2, -1.5, -1, -0.5, 0, 0.5, 1, 1.5 and d / 3 = -2.33, -1.33, -1, -0.67, -0.33, 0, 0.33, 0.67, 1
    assert R.rnd(1, d, 2).tolist() == [-3, -2, -1, -1, 0, 0, 1, 1, 2] and R.rnd(1, d, 2, "trunc").tolist() == [-3, -1, -1, 0, 0, 0, 1, 1, 2]
    assert R.rnd(1, d, 3).tolist() == [-2, -1, -1, -1, 0, 0, 0, 1, 1] and R.rnd(1, d, 3, "trunc").tolist() == [-1, 0, 0, 0, 0, 0, 0, 1, 1]


def test_border_pixel_sent_outside_is_clamped():
    frames, mvi = R.border_case()
    out = R.render_frames(frames[:1], frames[1:], mvi, 2, 8)[0, 0]
    p, q = frames[0].long(), frames[1].long()
    # pixel (0, 5): rows: c = -7, r0 = -1, f = 9: block rows clamp(-1) = 0 (weight 7) and 0 (weight 9): 16 on block row 0.  columns: c = 3, r0 = 0, f = 3: block
    # column 0 weighs 13, column 1 weighs 3.  Block (0, 0) holds (0, 0): P = prev[0][5], N = next[0][5].  Block (0, 1) holds (-12, -12), a = (-6, -6):
    # P = prev[6][11], N = next[6 - 12][11 - 12] = next[-6][-1] -> clamped to next[0][0].
    want = (16 * 13 * (p[0, 5] + q[0, 5]) + 16 * 3 * (p[6, 11] + q[0, 0]) + 256) // 512
    assert torch.equal(out[0, 5].long(), want)
    # pixel (2, 9): rows as above (c = -3, r0 = -1: block row 0 alone); columns: c = 11, r0 = 0, f = 11: 5 on column 0, 11 on column 1; N = next[2 + 6 - 12][9 + 6 - 12] = next[-4][3] -> next[0][3]
    want = (16 * 5 * (p[2, 9] + q[2, 9]) + 16 * 11 * (p[8, 15] + q[0, 3]) + 256) // 512
    assert torch.equal(out[2, 9].long(), want)
    # far from block (0, 1) nothing moves: the plain rounded mean
    assert torch.equal(out[20:, :4].long(), (p[20:, :4] + q[20:, :4] + 1) >> 1)


@pytest.mark.parametrize("variant", ["trunc", "nearest", "clamp"])
def test_wrong_rules_are_noticed(textures, variant):
    """a wrong rule must change mvi, cost or the frames on at least one of the translating textures, otherwise the inputs are too weak"""
    changed = []
    for (block, step, bi), (f, good) in textures.items():
        if not bi:
            continue
        bad = R.interpolate_frames(f[::2], 2, block, RADIUS, True, variant=variant)
        if not all(torch.equal(bad[k], good[k]) for k in good):
            changed.append((block, step))
    print(variant, "changes", changed)
    assert changed


def test_reference_batches_streaming_and_one_direction():
    g = torch.Generator().manual_seed(33)
    v = torch.randint(0, 256, (2, 3, 19, 27, 3), generator=g, dtype=torch.uint8)
    r = R.interpolate_frames(v, 3, 8, 3)
    assert r["video"].shape == (2, 7, 19, 27, 3) and r["mvi"].shape == (2, 2, 2, 2, 3, 2) and r["cost"].shape == (2, 2, 2, 2, 3)
    for b in range(2):                                        # no pair crosses batch items
        one = R.interpolate_frames(v[b], 3, 8, 3)
        assert all(torch.equal(r[k][b], one[k]) for k in r)
    two = R.interpolate_frames(v[0, 1:], 3, 8, 3)             # a pair's frames come from its two frames alone
    assert torch.equal(two["video"], r["video"][0, 3:]) and torch.equal(two["mvi"][0], r["mvi"][0, 1])
    fwd_only = R.interpolate_frames(v, 3, 8, 3, bidirectional=False)
    assert (fwd_only["cost"] >= r["cost"]).all()              # fewer candidates never cost less


def test_refusals_come_before_any_kernel_call():
    """on CPU tensors: a call that reached a kernel wrapper would raise RuntimeError (no CPU path), so every ValueError / NotImplementedError here was raised first"""
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    ok = u8(3, 32, 48, 3)
    calls = [lambda f, **kw: motion.interpolate_frames(f, **kw), lambda f, **kw: metrics.video_motion_smoothness(f, **kw)]
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
    for factor in (1, 0, 9, -2, 2.0, True, None):
        with pytest.raises(ValueError):
            motion.interpolate_frames(ok, factor=factor)
        with pytest.raises(ValueError):
            motion.FrameRateUpsampler(factor=factor)
    with pytest.raises(ValueError):
        metrics.video_motion_smoothness(u8(2, 32, 48, 3))       # two frames hold out none
    with pytest.raises(ValueError):
        metrics.video_motion_smoothness(u8(3, 8, 48, 3), block=8)               # below video_metrics' window
    assert motion.interpolate_frames.__defaults__ == (2, 16, 16, True, False)
    # the streaming class
    with pytest.raises(ValueError):
        motion.FrameRateUpsampler(block=12)
    with pytest.raises(ValueError):
        motion.FrameRateUpsampler(radius=40)
    up = motion.FrameRateUpsampler(factor=3, block=16, radius=4)
    with pytest.raises(ValueError):
        up.update(u8(1, 3, 32, 48, 3))
    with pytest.raises(NotImplementedError):
        up.update(ok.float())
    with pytest.raises(ValueError):
        up.update(u8(2, 8, 48, 3))
    first = torch.full((1, 32, 48, 3), 7, dtype=torch.uint8)
    got = up.update(first)                                      # one frame: final at once, carried, no pair yet, no kernel
    assert torch.equal(got, first)
    with pytest.raises(ValueError):
        up.update(u8(2, 32, 40, 3))                             # another frame size inside one video
    with pytest.raises(RuntimeError, match="GPU"):
        up.update(ok)
    up.new_video()
    assert torch.equal(up.update(first), first)
    import sys
    assert "longvgen" not in sys.modules or not hasattr(sys.modules["longvgen"], "motion")


def test_video_processor_default_is_untouched(monkeypatch):
    """VideoProcessor() neither imports nor calls the interpolation: with the motion entry point replaced by a stub that raises, every output type still passes its
    frames through from tg_video_to_uint8's wrapper (stubbed too: no GPU here) unchanged; with a factor the float outputs are refused before any kernel call."""
    import inspect
    sig = inspect.signature(video_io.VideoProcessor.__init__)
    assert list(sig.parameters) == ["self", "frame_rate_factor", "block", "radius", "bidirectional"] and sig.parameters["frame_rate_factor"].default == 1
    calls = []

    def fake_to_uint8(video, layout, kind, rounding=0):
        calls.append((kind, rounding))
        return torch.full((1, 2, 4, 4, 3), 9, dtype=torch.uint8)

    def boom(*a, **kw):
        raise AssertionError("the default VideoProcessor reached the interpolation")

    monkeypatch.setattr(video_io.K, "video_to_uint8", fake_to_uint8)
    monkeypatch.setattr(motion, "interpolate_frames", boom)
    monkeypatch.setattr(motion, "check_block", boom)
    vp = video_io.VideoProcessor()
    assert vp.frame_rate_factor == 1
    video = torch.zeros(1, 3, 2, 4, 4, dtype=torch.bfloat16)
    out = vp.postprocess_video(video, "uint8")
    assert out.shape == (1, 2, 4, 4, 3) and int(out.unique()) == 9
    pil = vp.postprocess_video(video, "pil")
    assert len(pil) == 1 and len(pil[0]) == 2
    vp.postprocess_video(video, "pt"), vp.postprocess_video(video, "np")
    assert calls == [(video_io.K.VIDEO_U8, 0), (video_io.K.VIDEO_U8, 1), (video_io.K.VIDEO_BF16_PLANAR, 0), (video_io.K.VIDEO_F32, 0)]
    with pytest.raises(ValueError):
        vp.postprocess_video(video, "gif")
    monkeypatch.undo()
    for bad in (0, 9, 2.0, True, None):
        with pytest.raises(ValueError):
            video_io.VideoProcessor(frame_rate_factor=bad)
    with pytest.raises(ValueError):
        video_io.VideoProcessor(frame_rate_factor=2, block=12)
    with pytest.raises(ValueError):
        video_io.VideoProcessor(frame_rate_factor=2, radius=0)
    vp2 = video_io.VideoProcessor(frame_rate_factor=2, block=8, radius=4)
    for kind in ("pt", "np"):
        with pytest.raises(ValueError, match="uint8"):
            vp2.postprocess_video(video, kind)
    seen = []
    monkeypatch.setattr(video_io.K, "video_to_uint8", fake_to_uint8)
    monkeypatch.setattr(motion, "interpolate_frames", lambda f, *a: seen.append(a) or f)
    vp2.postprocess_video(video, "uint8")
    assert seen == [(2, 8, 4, True)]


def test_export_argument_checks_without_a_launch():
    """tg_mci_select and tg_mci_render validate every argument before they touch HIP: one 32 x 32 pair, block 16, n = 2, and one argument wrong at a time"""
    from tokensgen_amd import lib as L
    lib = L.load()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf) + (16 - ctypes.addressof(buf) % 16)
    err = lambda: lib.tg_last_error_string().decode()
    rgb = dict(so=0, si=3072, sr=96, sp=3, sc=1)

    def select(**kw):
        a = dict(prev=p, prev_so=0, prev_si=1024, next=p, next_so=0, next_si=1024, fwd=p, bwd=p, n_outer=1, n_inner=1, H=32, W=32, pitch=32, block=16, n=2, mvi=p,
                 cost=p, stream=None)
        assert set(kw) <= set(a)
        a.update(kw)
        return lib.tg_mci_select(*a.values())

    def render(**kw):
        a = dict(prev=p, **{"a_" + k: v for k, v in rgb.items()}, next=p, **{"b_" + k: v for k, v in rgb.items()}, mvi=p, n_outer=1, n_inner=1, H=32, W=32, block=16,
                 n=2, out=p, out_so=3 * 3072, out_sf=3072, stream=None)
        assert set(kw) <= set(a)
        a.update(kw)
        return lib.tg_mci_render(*a.values())

    for name in ("prev", "next", "fwd", "mvi", "cost"):
        assert select(**{name: None}) == -1 and "null pointer" in err(), name
    for kw, code, text in ((dict(block=12), -1, "block must be 8 or 16"), (dict(n=1), -1, "n must be in 2..8"), (dict(n=9), -1, "n must be in 2..8"),
                           (dict(H=15), -2, "bad shape"), (dict(W=8), -2, "bad shape"), (dict(n_outer=0), -2, "bad shape"), (dict(n_inner=0), -2, "bad shape"),
                           (dict(pitch=31), -2, "pitch"), (dict(pitch=1 << 30), -2, "pitch"), (dict(prev_si=-4), -2, "pitch"), (dict(next_so=-4), -2, "pitch"),
                           (dict(n_outer=1 << 20, n_inner=1 << 20, H=64, W=64, pitch=64), -2, "too many blocks"),
                           (dict(cost=p + 2), -3, "aligned"), (dict(mvi=p + 1), -3, "aligned"), (dict(fwd=p + 1), -3, "aligned"), (dict(bwd=p + 1), -3, "aligned")):
        assert select(**kw) == code and text in err(), (kw, err())
    for name in ("prev", "next", "mvi", "out"):
        assert render(**{name: None}) == -1 and "null pointer" in err(), name
    for kw, code, text in ((dict(block=4), -1, "block must be 8 or 16"), (dict(n=1), -1, "n must be in 2..8"), (dict(n=9), -1, "n must be in 2..8"),
                           (dict(H=8), -2, "bad shape"), (dict(W=15), -2, "bad shape"), (dict(n_outer=0), -2, "bad shape"), (dict(n_inner=0), -2, "bad shape"),
                           (dict(a_sr=-96), -2, "negative stride"), (dict(b_sc=-1), -2, "negative stride"),
                           (dict(out_sf=3071), -2, "out_sf"), (dict(n_outer=2, out_so=3 * 3072 - 1), -2, "out_so"),
                           (dict(H=1 << 15, W=1 << 15, out_sf=1 << 40), -2, "2^31"),
                           (dict(n_outer=1 << 15, n_inner=1 << 15, out_so=1 << 50), -2, "too many tiles"), (dict(mvi=p + 1), -3, "aligned")):
        assert render(**kw) == code and text in err(), (kw, err())


