"""GPU: csrc/color.hip through tokensgen_amd.color, the colour metrics of tokensgen_amd.metrics and VideoProcessor.set_color_match.  Histograms, tables and mapped
bytes are integers: every check of them is torch.equal against tests/color_ref.py.  The L*a*b* sums are float64 on both sides.

Bound of the float64 checks: absolute 1e-9 on per-frame means.  Values stay below 260 and a few hundred float64 operations amplify a rounding of 1.1e-16 by at most
500 each, so a float64 implementation sits near 1e-12; an fp32 slip anywhere shows at about 1e-5 (6e-8 x 260).  1e-9 separates the two: a condition, not a
measurement.  The largest deviation seen goes to the parity report (profiles/color_parity.json is its copy)."""
import functools

import numpy as np
import pytest
import torch

import color_ref as R
from tokensgen_amd import color, metrics, motion, video_io
from tokensgen_amd import kernels as K
from tokensgen_amd import lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-9
SIZES = [(43, 61), (1, 1), (16, 16), (128, 96)]      # 43 x 61: 7 869 bytes per frame, odd, every later frame misaligned; 128 x 96: more than one workgroup's strip


def noise(seed, *shape):
    """seeded uint8 noise [.., H, W, 3] with exact zeros sprinkled in (test_mci_gpu.py's)"""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
    v[..., 1::7, ::3, :] = 0
    return v.to(DEV)


def at_offset(t, off):
    """a contiguous copy of t whose first byte sits `off` bytes into a fresh allocation: another alignment mod 16"""
    buf = torch.empty(t.numel() + off, dtype=torch.uint8, device=t.device)
    v = buf[off:].view(t.shape)
    v.copy_(t)
    return v


def drifting(seed, T, H, W):
    """a smooth-ish video whose channels drift by a different gain and offset per frame"""
    g = torch.Generator().manual_seed(seed)
    base = torch.randint(40, 200, (1, H, W, 3), generator=g).float()
    t = torch.arange(T).float()[:, None, None, None]
    gain = 1.0 + t * torch.tensor([0.04, -0.02, 0.07])
    offs = t * torch.tensor([3.0, -2.0, 1.0])
    jitter = torch.randint(-9, 10, (T, H, W, 3), generator=g).float()
    return ((base + jitter) * gain + offs).round().clamp(0, 255).to(torch.uint8).to(DEV)


@pytest.mark.parametrize("F", [1, 5])
@pytest.mark.parametrize("size", SIZES)
def test_histograms(size, F):
    """against bincount; noise with zeros, the same frames at another alignment, and one flat frame per value 0, 7 and 255 (every lane on one bin)"""
    H, W = size
    assert 128 * 96 * 3 > L.load().tg_color_strip_bytes(0) > 0
    f = noise(11 * H + F, F, H, W, 3)
    flat = torch.stack([torch.full((H, W, 3), v, dtype=torch.uint8, device=DEV) for v in (0, 7, 255)])
    for frames in (f, at_offset(f, 3), flat, at_offset(torch.cat([flat, f]), 9)):
        got = color.color_histograms(frames)
        assert got.dtype == torch.int32 and got.shape == (frames.shape[0], 3, 256)
        assert torch.equal(got.long(), R.histograms(frames))
        assert bool((got.sum(-1) == H * W).all())
    got = color.color_histograms(f)
    for k in range(F):                                                          # a frame's counts depend on that frame alone
        assert torch.equal(color.color_histograms(f[k:k + 1])[0], got[k])
    assert torch.equal(color.color_histograms(f[None])[0], got)                # [B, T, H, W, 3]


@pytest.mark.parametrize("F", [1, 5])
@pytest.mark.parametrize("size", SIZES)
def test_apply(size, F):
    """against torch.gather with random tables, not monotone and different per frame and channel; out of place (same and different alignment of input and output)
    and in place"""
    H, W = size
    assert 128 * 96 * 3 > L.load().tg_color_strip_bytes(1) > 0
    f = noise(13 * H + F, F, H, W, 3)
    g = torch.Generator().manual_seed(F + W)
    luts = torch.randint(0, 256, (F, 3, 256), generator=g, dtype=torch.uint8).to(DEV)
    want = R.apply_luts(f, luts)
    assert torch.equal(color.apply_luts(f, luts), want)
    for off_in, off_out in ((3, 3), (0, 5), (7, 0), (1, 14)):
        src = at_offset(f, off_in)
        dst = at_offset(torch.zeros_like(f), off_out)
        assert color.apply_luts(src, luts, out=dst) is dst and torch.equal(dst, want) and torch.equal(src, f)
    for off in (0, 11):
        buf = at_offset(f, off)
        assert color.apply_luts(buf, luts, out=buf) is buf and torch.equal(buf, want)


def table_cases():
    """name -> (hist int32 [F, 3, 256], anchor int64 [3, 256]) on the CPU"""
    vid = drifting(3, 8, 24, 40).cpu()
    hist = R.histograms(vid).to(torch.int32)
    wide = R.histograms(noise(5, 2, 16, 16, 3).cpu()).sum(0)                   # std about 74: a gain far above 1.5
    narrow = R.histograms(torch.randint(118, 124, (1, 16, 16, 3), generator=torch.Generator().manual_seed(6), dtype=torch.uint8)).sum(0)
    flat = R.histograms(torch.full((3, 5, 7, 3), 77, dtype=torch.uint8)).to(torch.int32)
    one = R.histograms(torch.tensor([[[[3, 200, 255]]], [[[0, 0, 9]]]], dtype=torch.uint8)).to(torch.int32)          # two frames of 1 x 1
    return {"drift_own": (hist, hist[:2].long().sum(0)), "drift_wide": (hist, wide), "drift_narrow": (hist, narrow), "flat_source": (flat, wide),
            "flat_anchor": (hist, flat[0].long()), "one_pixel": (one, wide), "one_pixel_anchor": (hist, one[0].long())}


@pytest.mark.parametrize("mode", ["meanstd", "histogram"])
def test_tables(mode):
    """bit for bit against the restatement: both sides do the same IEEE operations in the same order.  max_gain 1.5 is hit from above (wide anchor) and from
    below (narrow, flat and one-pixel anchors)"""
    for name, (hist, anchor) in table_cases().items():
        hd, ad = hist.to(DEV), anchor.to(DEV)
        for strength in (1.0, 0.5, 0.3):
            for window in (1, 3):
                for max_gain in ((1.5, 4.0) if mode == "meanstd" else (4.0,)):
                    status = torch.zeros(1, dtype=torch.int32, device=DEV)
                    got = color.match_luts(hd, ad, mode, strength, window, max_gain, status=status)
                    want = R.match_luts(hist, anchor, mode, strength, window, max_gain)
                    assert got.dtype == torch.uint8 and torch.equal(got.cpu(), want), (name, strength, window, max_gain, int((got.cpu() != want).sum()))
                    assert int(status) == 0
    hist, anchor = table_cases()["drift_wide"]
    hd, ad = hist.to(DEV), anchor.to(DEV)
    whole = color.match_luts(hd, ad, mode, 0.5, 3, 2.0)
    assert torch.equal(color.match_luts(hd[5:], ad, mode, 0.5, 3, 2.0, history=hd[3:5]), whole[5:])          # carried histograms
    assert torch.equal(color.match_luts(hd[1:], ad, mode, 0.5, 3, 2.0, history=hd[:1]), whole[1:])           # fewer than window - 1: the video starts there
    assert torch.equal(color.match_luts(hd[4:5], ad, mode, 0.5, 1, 2.0), color.match_luts(hd, ad, mode, 0.5, 1, 2.0)[4:5])
    # what the host cannot judge without waiting is refused on the device: identity tables and a count
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    empty = torch.zeros(2, 3, 256, dtype=torch.int32, device=DEV)
    got = color.match_luts(empty, ad, mode, 1.0, 1, 4.0, status=status)
    assert int(status) == 6 and torch.equal(got, torch.arange(256, dtype=torch.uint8, device=DEV).expand(2, 3, 256))
    huge = ad.clone()
    huge[1, 0] = 1 << 31
    got = color.match_luts(hd, huge, mode, 1.0, 1, 4.0, status=status)
    assert int(status) == 6 + hd.shape[0] and torch.equal(got[:, 1], torch.arange(256, dtype=torch.uint8, device=DEV).expand(hd.shape[0], 256))
    assert torch.equal(got[:, 0].cpu(), R.match_luts(hist, anchor, mode, 1.0, 1, 4.0)[:, 0])


@pytest.mark.parametrize("mode", ["meanstd", "histogram"])
def test_match_colors_end_to_end(mode):
    vid = drifting(7, 14, 43, 61)
    other = noise(8, 3, 20, 33, 3)
    anchors = {"frames": other, "hist": R.histograms(other).sum(0), "none": None}
    for name, anchor in anchors.items():
        for strength, window in ((1.0, 1), (0.5, 3)):
            got, luts = color.match_colors(vid, anchor, 8, mode, strength, window, 2.0, return_luts=True)
            want, want_luts = R.match_colors(vid.cpu(), None if anchor is None else anchor.cpu(), 8, mode, strength, window, 2.0)
            assert torch.equal(luts.cpu(), want_luts), name
            assert got.dtype == torch.uint8 and got.shape == vid.shape and torch.equal(got.cpu(), want), name
    assert not torch.equal(color.match_colors(vid, other, mode=mode), vid)
    # identities
    assert torch.equal(color.match_colors(vid, other, mode=mode, strength=0.0), vid)
    assert torch.equal(color.match_colors(vid[:1], None, mode="histogram"), vid[:1])                         # the anchor is the source
    assert torch.equal(color.match_colors(vid[:1], R.histograms(vid[:1])[0] * 3, mode="histogram"), vid[:1])  # ... at another total
    # [B, T, H, W, 3]: every item its own video
    two = torch.stack([vid[:6], noise(9, 6, 43, 61, 3)])
    got, luts = color.match_colors(two, None, 2, mode, 0.7, 3, 3.0, return_luts=True)
    assert got.shape == two.shape and luts.shape == (2, 6, 3, 256)
    for b in range(2):
        g1, l1 = color.match_colors(two[b], None, 2, mode, 0.7, 3, 3.0, return_luts=True)
        assert torch.equal(got[b], g1) and torch.equal(luts[b], l1)
    # a view that is not contiguous
    assert torch.equal(color.match_colors(vid[::2], other, mode=mode), color.match_colors(vid[::2].contiguous(), other, mode=mode))


@pytest.mark.parametrize("mode", ["meanstd", "histogram"])
def test_color_matcher_streams(mode):
    vid = drifting(10, 14, 27, 37)
    whole = color.match_colors(vid, None, 8, mode, 0.8, 3, 2.0)
    cm = color.ColorMatcher(mode, 0.8, 3, 2.0, anchor=None, anchor_frames=8)
    pieces = torch.cat([cm.update(vid[0:8]), cm.update(vid[8:9]), cm.update(vid[9:14])])
    assert torch.equal(pieces, whole)
    cm.new_video()                                                              # forgets the anchor and the carried histograms
    vid2 = noise(12, 9, 27, 37, 3)
    assert torch.equal(cm.update(vid2), color.match_colors(vid2, None, 8, mode, 0.8, 3, 2.0))
    cm.new_video()
    with pytest.raises(ValueError, match="anchor frames"):
        cm.update(vid[:7])
    other = noise(13, 2, 9, 11, 3)
    given = color.ColorMatcher(mode, 0.8, 3, 2.0, anchor=other)
    assert torch.equal(torch.cat([given.update(vid[:1]), given.update(vid[1:14])]), color.match_colors(vid, other, 8, mode, 0.8, 3, 2.0))
    given.new_video(anchor=R.histograms(vid2).sum(0))
    assert torch.equal(given.update(vid[:3]), color.match_colors(vid[:3], R.histograms(vid2).sum(0), 8, mode, 0.8, 3, 2.0))


def check_means(parity, got, want, what):
    assert got.dtype == torch.float64 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    parity(float((got - want).abs().max()), TOL, what)


def test_lab_every_8bit_colour(parity):
    """256 frames of 256 x 256 with R = frame, G = row, B = column: every 8-bit colour once.  Per-frame means against the restatement on the device"""
    r = torch.arange(256, dtype=torch.uint8, device=DEV)
    cube = torch.stack([r[:, None, None].expand(256, 256, 256), r[None, :, None].expand(256, 256, 256), r[None, None, :].expand(256, 256, 256)], dim=-1).contiguous()
    got = K.lab_metrics(cube, None, "hwc")[0] / 65536.0
    want = torch.cat([R.lab_means(cube[i:i + 32]) for i in range(0, 256, 32)])
    check_means(parity, got, want, "L, a, b, C means of every 8-bit colour")
    assert float(got[:, 0].min()) >= 0.0 and float(got[:, 0].max()) <= 100.0 + 1e-9
    alone = K.lab_metrics(cube[200:201], None, "hwc")[0] / 65536.0            # bitwise the same alone and inside the larger call
    assert torch.equal(alone[0], got[200])


@functools.lru_cache(maxsize=None)
def pair_u8():
    return noise(21, 2, 3, 43, 61, 3), noise(22, 2, 3, 43, 61, 3)


LAYOUT_CASES = [("uint8", "hwc5"), ("uint8", "hwc4"), ("fp32", "chw"), ("fp32", "bcthw"), ("bf16", "chw"), ("bf16", "bcthw"), ("fp32", "hwc_as_chw_view")]


@pytest.mark.parametrize("crop_border", [0, 3])
@pytest.mark.parametrize("dtype,layout", LAYOUT_CASES)
def test_delta_eab_layouts(parity, dtype, layout, crop_border):
    """two-input dE on 43 x 61 noise pairs: interleaved uint8, planar and [B, 3, T, H, W] floats (also as a permuted view of interleaved memory)"""
    a8, b8 = pair_u8()                                                          # [2, 3, 43, 61, 3]
    if dtype == "uint8":
        a, b = (a8, b8) if layout == "hwc5" else (a8[0], b8[0])
        ra, rb = (R.channels_last(t, "hwc") for t in (a, b))
        shape = a.shape[:-3]
    else:
        dt = torch.float32 if dtype == "fp32" else torch.bfloat16
        fa, fb = ((t.float() / 255.0 + (0.2 * (t > 250) if i else -0.1 * (t < 20))).to(dt) for i, t in enumerate((a8, b8)))      # some values outside [0, 1]: clamped
        if layout == "bcthw":
            a, b = (t.permute(0, 4, 1, 2, 3).contiguous() for t in (fa, fb))
            shape = (2, 3)
        elif layout == "chw":
            a, b = (t[1].permute(0, 3, 1, 2).contiguous() for t in (fa, fb))
            shape = (3,)
        else:
            a, b = (t[0].permute(0, 3, 1, 2) for t in (fa, fb))                 # (n, 3, h, w) strides over interleaved memory
            shape = (3,)
        ra, rb = (R.channels_last(t, "bcthw" if layout == "bcthw" else "chw") for t in (a, b))
    got = metrics.video_delta_eab(a, b, crop_border)
    want = R.lab_means(R.crop(ra, crop_border), R.crop(rb, crop_border))
    assert got["per_frame"].shape == shape
    check_means(parity, got["per_frame"].reshape(-1), want[:, 8], f"dE {dtype} {layout} crop {crop_border}")
    assert abs(float(got["delta_eab"]) - float(want[:, 8].mean())) < TOL
    same = metrics.video_delta_eab(a, a.clone(), crop_border)
    assert float(same["per_frame"].abs().max()) == 0.0 and float(same["delta_eab"]) == 0.0                  # identical inputs: exactly 0
    raw = K.lab_metrics(a, b, metrics._layout(a), crop_border)                  # all nine sums
    px = (43 - 2 * crop_border) * (61 - 2 * crop_border)
    check_means(parity, raw.reshape(-1, 9) / px, want, f"nine means {dtype} {layout} crop {crop_border}")
    one = K.lab_metrics(a, None, metrics._layout(a), crop_border)
    assert torch.equal(one.reshape(-1, 4), raw.reshape(-1, 9)[:, :4])           # the first input's sums do not depend on the second


def test_lab_frame_alone_and_in_a_call():
    a8, b8 = pair_u8()
    a, b = a8.reshape(6, 43, 61, 3), b8.reshape(6, 43, 61, 3)
    whole = K.lab_metrics(a, b, "hwc", 0)[0]
    for i in (0, 4, 5):
        assert torch.equal(K.lab_metrics(a[i:i + 1], b[i:i + 1], "hwc", 0)[0, 0], whole[i])
    assert torch.equal(K.lab_metrics(a[None, 2:5], b[None, 2:5], "hwc", 0)[0], whole[2:5])
    tall = noise(23, 1, 70, 130, 3)                                             # three tile rows, three tile columns
    got = K.lab_metrics(tall, None, "hwc")[0, 0] / (70 * 130)
    assert float((got - R.lab_means(tall)[0]).abs().max()) < TOL


def ramp_clip():
    """12 frames of one textured picture under a per-frame gain ramp (the exposure creeps up)"""
    g = torch.Generator().manual_seed(31)
    base = torch.randint(30, 150, (1, 32, 48, 3), generator=g).float() * torch.tensor([1.0, 0.8, 0.6])
    gain = 1.0 + 0.05 * torch.arange(12).float()[:, None, None, None]
    return (base * gain).round().clamp(0, 255).to(torch.uint8).to(DEV)


def test_color_drift_and_metric_entry_points(parity):
    clip = ramp_clip()
    got = metrics.video_color_drift(clip, anchor_frames=2)
    want = R.color_drift(clip, 2)
    for k in ("lab_mean", "chroma", "drift"):
        check_means(parity, got[k], want[k], f"video_color_drift {k}")
    for k in ("drift_mean", "drift_max", "chroma_ratio"):
        assert got[k].dim() == 0 and abs(float(got[k]) - float(want[k])) < TOL
    d = metrics.video_color_drift(clip)["drift"]
    assert float(d[0]) == 0.0 and bool((d[1:] > d[:-1]).all())                 # the ramp: drift rises monotonically
    fixed = color.match_colors(clip, None, 1, "meanstd")
    assert float(metrics.video_color_drift(fixed)["drift_max"]) < float(metrics.video_color_drift(clip)["drift_max"])
    planar = (clip.permute(0, 3, 1, 2).float() / 255.0).contiguous()          # fp32 (n, 3, h, w): v / 255 rounded to fp32, so its own reference
    check_means(parity, metrics.video_color_drift(planar, 2)["drift"], R.color_drift(planar.permute(0, 2, 3, 1), 2)["drift"], "video_color_drift fp32 planar")
    # streaming: pieces give the bits of the whole; two videos
    acc = metrics.VideoColorDrift(anchor_frames=2)
    acc.update(clip[:5]); acc.update(clip[5:6]); acc.update(clip[6:])
    acc.new_video()
    other = noise(32, 3, 20, 24, 3)
    acc.update(other)
    out = acc.finalize()
    assert out["videos"] == 2 and all(torch.equal(out[k][0], got[k]) for k in ("lab_mean", "chroma", "drift"))
    assert torch.equal(out["drift_mean"][0], got["drift_mean"]) and torch.equal(out["drift_max"][0], got["drift_max"]) and torch.equal(out["chroma_ratio"][0], got["chroma_ratio"])
    second = R.color_drift(other, 2)
    check_means(parity, out["drift"][1], second["drift"], "VideoColorDrift second video")
    assert abs(float(out["drift_mean_pooled"]) - (float(want["drift_mean"]) + float(second["drift_mean"])) / 2) < TOL
    # calculate_delta_Eab: one pair, HWC and CHW, bytes and floats
    a, b = clip[3], fixed[9]
    ref = R.lab_means(a[None], b[None])[0, 8]
    e = metrics.calculate_delta_Eab(a, b, 0)
    assert e.dim() == 0 and e.dtype == torch.float64 and e.is_cuda
    parity(abs(float(e) - float(ref)), TOL, "calculate_delta_Eab HWC uint8")
    parity(abs(float(metrics.calculate_delta_Eab(a.permute(2, 0, 1), b.permute(2, 0, 1), 0, input_order="CHW")) - float(ref)), TOL, "calculate_delta_Eab CHW view")
    fa, fb = a.float() / 255.0, b.float() / 255.0
    ref4 = R.lab_means(fa[None, 4:-4, 4:-4], fb[None, 4:-4, 4:-4])[0, 8]
    parity(abs(float(metrics.calculate_delta_Eab(fa, fb, 4)) - float(ref4)), TOL, "calculate_delta_Eab fp32 crop 4")
    assert float(metrics.calculate_delta_Eab(a, a, 0)) == 0.0


def test_video_metrics_delta_eab_flag(parity):
    a, b = ramp_clip(), color.match_colors(ramp_clip(), None, 1, "histogram")
    plain = metrics.VideoMetrics()
    plain.update(a, b)
    assert sorted(plain.finalize()) == ["frames", "mse", "psnr", "psnr_pooled", "ssim", "ssim_pooled"]      # exactly the parent's keys
    vm = metrics.VideoMetrics(crop_border=2)
    assert vm.delta_eab is False
    vm.delta_eab = True                                                        # an attribute: the constructor's parameter list is what it was
    first = vm.update(a[:5], b[:5])
    vm.update(a[5:], b[5:])
    out = vm.finalize()
    assert sorted(out) == ["delta_eab", "delta_eab_pooled", "frames", "mse", "psnr", "psnr_pooled", "ssim", "ssim_pooled"]
    want = R.lab_means(R.crop(a, 2), R.crop(b, 2))[:, 8]
    check_means(parity, out["delta_eab"], want, "VideoMetrics delta_eab")
    assert torch.equal(first["delta_eab"], out["delta_eab"][:5]) and abs(float(out["delta_eab_pooled"]) - float(want.mean())) < TOL
    base = metrics.VideoMetrics(crop_border=2)
    base.update(a, b)
    assert all(torch.equal(base.finalize()[k], out[k]) for k in ("mse", "ssim", "psnr"))


def test_video_processor_color_match():
    g = torch.Generator().manual_seed(40)
    video = (torch.rand(2, 3, 5, 32, 48, generator=g) * torch.linspace(0.5, 1.0, 5)[None, None, :, None, None] * 2 - 1).to(torch.bfloat16).to(DEV)
    plain = video_io.VideoProcessor().postprocess_video(video, "uint8")
    assert torch.equal(plain, K.video_to_uint8(video, 1, K.VIDEO_U8, 0))      # the default construction: the parent's bytes
    vp = video_io.VideoProcessor().set_color_match("histogram", anchor_frames=2, strength=0.75, window=2)
    got = vp.postprocess_video(video, "uint8")
    want = color.match_colors(plain, None, 2, "histogram", 0.75, 2)
    assert got.shape == plain.shape and torch.equal(got, want) and not torch.equal(got, plain)
    anchor = noise(41, 2, 10, 12, 3)
    both = video_io.VideoProcessor(frame_rate_factor=2, block=8, radius=4).set_color_match("meanstd", anchor=anchor)
    assert torch.equal(both.postprocess_video(video, "uint8"), motion.interpolate_frames(color.match_colors(plain, anchor, mode="meanstd"), 2, 8, 4))
    pil = vp.postprocess_video(video, "pil")
    rounded = color.match_colors(video_io.frames_to_uint8(video, "bcthw", 1), None, 2, "histogram", 0.75, 2).cpu()
    assert len(pil) == 2 and len(pil[0]) == 5 and all(torch.equal(torch.from_numpy(np.array(im)), rounded[1, i]) for i, im in enumerate(pil[1]))
    with pytest.raises(ValueError, match="color_match"):
        vp.postprocess_video(video, "np")


def test_byte_offsets_past_2_31():
    """three frames of 16384 x 16384: 805 306 368 bytes each, the last one spans byte 2^31 of the call.  Its counts and bytes against the frame alone and the restatement"""
    g = torch.Generator(device=DEV).manual_seed(50)
    big = torch.randint(0, 256, (3, 16384, 16384, 3), generator=g, device=DEV, dtype=torch.uint8)
    assert big.numel() > 1 << 31 > 2 * big[0].numel()
    hist = color.color_histograms(big)
    assert torch.equal(hist[2], color.color_histograms(big[2:3])[0]) and torch.equal(hist[2].long(), R.histograms(big[2:3])[0])
    assert bool((hist.sum(-1) == 16384 * 16384).all())
    luts = torch.randint(0, 256, (3, 3, 256), generator=torch.Generator().manual_seed(51), dtype=torch.uint8).to(DEV)
    out = color.apply_luts(big, luts)
    assert torch.equal(out[2:3], R.apply_luts(big[2:3], luts[2:3])) and torch.equal(out[0, :64], R.apply_luts(big[:1, :64], luts[:1])[0])
