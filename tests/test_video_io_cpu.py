"""tokensgen_amd.video_io without a GPU: the antialias filter tables against F.interpolate on the CPU, the plan geometry against hand-computed answers, the frame
index arithmetic of `load_video`, the display restatement of tests/video_ref.py against known answers, and the argument checks of the two exports (no launch).  The
kernels are held to the fp64 restatements in tests/test_video_io_gpu.py."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import video_ref as VR

MODES = ("bicubic", "bilinear")


def _dense(n_in, n_out, mode):
    from tokensgen_amd.video_io import aa_weights
    first, count, w = aa_weights(n_in, n_out, mode)
    assert first.dtype == np.int32 and count.dtype == np.int32 and w.dtype == np.float32 and w.shape == (n_out, count.max())
    assert (first >= 0).all() and (first + count <= n_in).all() and (count >= 1).all()
    return VR.densify(first, count, w, n_in)


def _interp_gap(in_hw, out_hw, mode, seed):
    """max |Dy x Dx^T - F.interpolate(x, antialias=True)| on a random fp32 image in [0, 1]"""
    x = torch.rand(1, 1, *in_hw, generator=torch.Generator().manual_seed(seed))
    want = Fn.interpolate(x, size=out_hw, mode=mode, align_corners=False, antialias=True)[0, 0].double()
    got = _dense(in_hw[0], out_hw[0], mode) @ x[0, 0].double() @ _dense(in_hw[1], out_hw[1], mode).T
    return (got - want).abs().max().item()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("in_hw,out_hw", [((37, 53), (16, 23)), ((23, 31), (48, 64)), ((90, 160), (40, 71))])
def test_aa_weights_match_interpolate_small(mode, in_hw, out_hw):
    """Bound 1e-5: about four times what torch's own fp32 arithmetic leaves at these sizes (aten forms the filter centre in fp32)."""
    gap = _interp_gap(in_hw, out_hw, mode, 1)
    print("gap", mode, in_hw, out_hw, gap)
    assert gap < 1e-5


@pytest.mark.parametrize("mode", MODES)
def test_aa_weights_match_interpolate_1080p(mode):
    """One 1080 x 1920 -> 480 x 853 frame; bound 2e-4 (the gap grows with the coordinate's magnitude: fp32 centres in aten)."""
    gap = _interp_gap((1080, 1920), (480, 853), mode, 2)
    print("gap", mode, gap)
    assert gap < 2e-4


@pytest.mark.parametrize("mode", MODES)
def test_aa_weights_agree_with_the_independent_restatement(mode):
    for n_in, n_out in ((53, 23), (31, 64), (100, 71), (324, 72), (60, 60)):
        assert (_dense(n_in, n_out, mode) - VR.dense_aa(n_in, n_out, mode)).abs().max().item() < 2.0 ** -24


def test_bicubic_table_is_the_identity_at_scale_one():
    from tokensgen_amd.video_io import aa_weights
    first, count, w = aa_weights(48, 48, "bicubic")
    assert np.array_equal(first, np.arange(48)) and (count == 1).all() and w.shape == (48, 1) and (w == 1.0).all()
    first, count, w = aa_weights(7, 7, "bilinear")
    assert np.array_equal(first, np.arange(7)) and (count == 1).all() and (w == 1.0).all()
    with pytest.raises(ValueError):
        aa_weights(7, 7, "nearest")


def test_plan_geometry_against_hand_computed_answers():
    from tokensgen_amd.video_io import resample_plan
    p = resample_plan((1080, 1920), (480, 720), crop_to_fit=True)
    assert (p.resized_hw, p.top, p.left, p.mode) == ((480, 853), 0, 66, "bicubic") and p.pad_x == p.pad_y == 0
    assert p.tables[0].shape == (480,) and p.tables[3].shape == (720,) and p.tables[5].shape[0] == 720
    p = resample_plan((1920, 1080), (480, 720), crop_to_fit=True)
    assert (p.resized_hw, p.top, p.left) == ((1280, 720), 400, 0)
    p = resample_plan((45, 100), (32, 48), crop_to_fit=True)
    assert (p.resized_hw, p.top, p.left) == ((32, 71), 0, 11)
    # the sliced tables are rows left .. left + ow of the full ones
    from tokensgen_amd.video_io import aa_weights
    x0, nx, wx = aa_weights(100, 71, "bicubic")
    assert np.array_equal(p.tables[3], x0[11:59]) and np.array_equal(p.tables[4], nx[11:59]) and np.array_equal(p.tables[5], wx[11:59, :p.taps[1]])
    p = resample_plan((480, 720), (480, 720), crop_to_fit=True)
    assert (p.resized_hw, p.top, p.left, p.taps) == ((480, 720), 0, 0, (1, 1))
    p = resample_plan((60, 60), (32, 48), pad_to_fit=True)
    assert (p.padded_hw, p.pad_x, p.pad_y, p.mode, p.resized_hw) == ((60, 90), 15, 0, "bilinear", (32, 48))
    assert p.tables[3][0] < 0 and p.tables[3][-1] + p.tables[4][-1] > 60          # the outermost columns draw on the pad
    p = resample_plan((90, 60), (48, 48), pad_to_fit=True)                         # tall source: Pad((nw - iw) // 2, 0) again
    assert (p.padded_hw, p.pad_x, p.pad_y) == ((90, 90), 15, 0)
    p = resample_plan((40, 90), (48, 48), pad_to_fit=True)                         # wide source: Pad((0, (nh - ih) // 2))
    assert (p.padded_hw, p.pad_x, p.pad_y) == ((90, 90), 0, 25)
    p = resample_plan((50, 70), (32, 48))                                          # no flag: the aspect ratio changes, nothing is cropped or padded
    assert (p.resized_hw, p.top, p.left, p.pad_x, p.pad_y, p.padded_hw, p.mode) == ((32, 48), 0, 0, 0, 0, (50, 70), "bilinear")
    assert p.tables[0][0] == 0 and p.tables[0][-1] + p.tables[1][-1] == 50 and p.tables[3][0] == 0 and p.tables[3][-1] + p.tables[4][-1] == 70
    assert resample_plan((50, 70), (32, 48)) is p                                  # cached per shape
    with pytest.raises(ValueError, match="taps"):
        resample_plan((2160, 3840), (32, 48), crop_to_fit=True)                    # 67x: more taps than the kernel takes


def test_plan_tables_agree_with_the_restated_operators():
    """Every branch of the plan (crop from the left / from the top, pad on either axis, plain squeeze) as dense operators against tests/video_ref.py's own geometry."""
    from tokensgen_amd.video_io import resample_plan
    for in_hw, res, crop, pad in (((45, 100), (32, 48), True, False), ((100, 45), (32, 48), True, False), ((60, 60), (32, 48), False, True),
                                  ((40, 90), (48, 48), False, True), ((50, 70), (32, 48), False, False), ((20, 30), (32, 48), True, False)):
        p = resample_plan(in_hw, res, crop, pad)
        Dy, Dx = VR.operators(in_hw, res, crop, pad)
        y0, ny, wy, x0, nx, wx = p.tables
        assert (VR.densify(y0, ny, wy, in_hw[0]) - Dy).abs().max().item() < 2.0 ** -24, (in_hw, res)
        assert (VR.densify(x0, nx, wx, in_hw[1]) - Dx).abs().max().item() < 2.0 ** -24, (in_hw, res)


def test_sample_frame_indices():
    from tokensgen_amd.video_io import sample_frame_indices
    idx = sample_frame_indices(300, 30.0, 49, sample_fps=10, start_t=0, end_t=-1, max_num_chunks=12)
    assert idx.dtype == np.int64 and np.array_equal(idx, 3 * np.arange(98))          # 100 samples -> 2 whole chunks of 49
    idx = sample_frame_indices(300, 30.0, 49, sample_fps=-1, start_t=0, end_t=-1, max_num_chunks=12)
    assert np.array_equal(idx, np.arange(294))                                       # the clip's own rate: 6 chunks
    assert len(sample_frame_indices(300, 30.0, 49, sample_fps=-1, max_num_chunks=2)) == 98
    idx = sample_frame_indices(300, 30.0, 10, sample_fps=10, start_t=2, end_t=1000, max_num_chunks=100)   # end_t beyond the clip: cut to 10 s
    assert np.array_equal(idx, 60 + 3 * np.arange(80))
    with pytest.raises(AssertionError, match="empty"):
        sample_frame_indices(30, 30.0, 49, sample_fps=10)                            # 10 samples: not one whole chunk
    with pytest.raises(AssertionError):
        sample_frame_indices(300, 30.0, 49, start_t=11)                              # starts past the end


def test_display_restatement_known_answers():
    v = torch.tensor([-1.0, 1.0, 0.0, 2.0, -3.0, float("nan")], dtype=torch.bfloat16)
    assert VR.display_ref(v, 0).tolist() == [0, 255, 127, 255, 0, 0]
    assert VR.display_ref(v, 1).tolist() == [0, 255, 128, 255, 0, 0]
    allv = VR.all_bf16_patterns()
    assert allv.shape == (65536,) and allv.view(torch.int16)[40000].item() == 40000 - 65536
    fin = allv[torch.isfinite(allv.float())]
    assert fin.numel() == 65280
    frac = (VR.display_ref(fin, 0) != VR.display_ref(fin, 1)).float().mean().item()
    print("truncation and rounding differ on", frac)
    assert 0.46 < frac < 0.48                                                        # 47 %: a test that mixes the two up cannot pass
    # the single rounding the kernel uses equals torch's two bf16 operations on every finite pattern
    one = (fin.float() * 0.5 + 0.5).to(torch.bfloat16).clamp(0, 1)
    assert torch.equal(one, VR.display_unit_ref(fin))
    # ... and fp32 arithmetic throughout does not
    assert ((fin.float() * 0.5 + 0.5).clamp(0, 1) * 255).to(torch.uint8).ne(VR.display_ref(fin, 0)).float().mean().item() > 1e-3


def test_refined_reciprocal_equals_the_division_on_every_byte_value():
    """csrc/video.hip forms float(u8) / 255.0f as q0 = v * rcp, r = fma(-q0, 255, v), q = fma(r, rcp, q0) with rcp = fp32(1 / 255).  In exact rational arithmetic,
    each step rounded once to fp32 (ties to even), q is the IEEE quotient for all 256 inputs, where the bare product v * rcp is not."""
    from fractions import Fraction as Fr
    f32 = np.float32

    def rnd(x):
        c = f32(float(x))
        cands = [c, np.nextafter(c, f32(np.inf)), np.nextafter(c, f32(-np.inf))]
        d = sorted((abs(Fr(float(k)) - x), i) for i, k in enumerate(cands))
        if d[0][0] == d[1][0] and d[0][0] != 0:
            a, b = cands[d[0][1]], cands[d[1][1]]
            return a if (a.view(np.uint32) & 1) == 0 else b
        return cands[d[0][1]]
    rcp = f32(1.0) / f32(255.0)
    bare = 0
    for v in range(256):
        want = f32(v) / f32(255.0)
        q0 = rnd(Fr(v) * Fr(float(rcp)))
        r = Fr(v) - Fr(float(q0)) * 255
        assert Fr(float(rnd(r))) == r                                               # the residual is exact in fp32
        assert rnd(Fr(float(q0)) + r * Fr(float(rcp))) == want, v
        bare += q0 != want
    assert bare > 100                                                               # a multiplication by the reciprocal alone misses on about half of them


def test_video_io_refuses_cpu_and_bad_arguments():
    from tokensgen_amd import video_io as VIO
    frames = torch.zeros(2, 20, 30, 3, dtype=torch.uint8)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="GPU"):
            VIO.prepare_video(frames, (32, 48), crop_to_fit=True)
    with pytest.raises(RuntimeError, match="GPU"):
        VIO.prepare_video(frames, (32, 48), crop_to_fit=True, device="cpu")
    with pytest.raises(TypeError):
        VIO.prepare_video(frames.float(), (32, 48))
    with pytest.raises(RuntimeError, match="GPU"):
        VIO.frames_to_uint8(torch.zeros(1, 3, 2, 4, 4, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="GPU"):
        VIO.VideoProcessor().postprocess_video(torch.zeros(1, 3, 2, 4, 4, dtype=torch.bfloat16), "uint8")
    with pytest.raises(ValueError):
        VIO.frames_to_uint8(torch.zeros(1, 3, 2, 4, 4, dtype=torch.bfloat16), layout="hwc")


def test_new_exports_validate_their_arguments_without_a_launch():
    from tokensgen_amd import lib as L
    lib = L.load()
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.addressof(buf) + (16 - ctypes.addressof(buf) % 16)
    err = lambda: lib.tg_last_error_string().decode()
    rs_args = dict(src=p, F=1, H=8, W=8, dst=p, oh=4, ow=4, y0=p, ny=p, wy=p, taps_y=4, x0=p, nx=p, wx=p, taps_x=4, stream=None)      # in the order of the prototype
    rs = lambda **kw: lib.tg_video_resample(*{**rs_args, **kw}.values())
    for name in ("src", "dst", "y0", "ny", "wy", "x0", "nx", "wx"):
        assert rs(**{name: None}) == -1 and "null pointer" in err(), name
    for name in ("F", "H", "W", "oh", "ow", "taps_y", "taps_x"):
        assert rs(**{name: 0}) == -2 and "bad shape" in err(), name
    for name in ("taps_y", "taps_x"):
        assert rs(**{name: 65}) == -2 and "at most 64 taps" in err(), name
    assert rs(dst=p + 2) == -3
    u8_args = dict(src=p, sb=48, sc=16, st=4, B=1, T=1, H=2, W=2, dst=p, kind=0, rounding=0, stream=None)
    u8 = lambda **kw: lib.tg_video_to_uint8(*{**u8_args, **kw}.values())
    for name in ("src", "dst"):
        assert u8(**{name: None}) == -1 and "null pointer" in err(), name
    for name in ("B", "T", "H", "W"):
        assert u8(**{name: 0}) == -2 and "bad shape" in err(), name
    assert u8(sb=-1) == -2
    assert u8(kind=3) == -1 and u8(rounding=2) == -1
    assert u8(src=p + 1) == -3 and u8(kind=1, dst=p + 2) == -3
