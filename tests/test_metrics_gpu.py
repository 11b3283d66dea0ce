"""GPU: tokensgen_amd.metrics on the HIP path.  tg_image_metrics against the float64 restatement of tests/metrics_ref.py, for EVERY frame and channel of every case.

Sum of squared differences.  uint8 RGB: the terms are integers <= 65 025 and the sum stays below 2^53, so every order of addition gives the same float64: compared
with ==.  Float and Y inputs: |got - ref| <= n_terms 2^-52 ref (each term carries two roundings, each of the two summations at most n_terms - 1 more, unit roundoff 2^-53).

SSIM.  The per-plane mean of the map is held to SSIM_BOUND + n_positions 2^-52, derived here, with u = 2^-53, pixel values <= 255 and their products <= 65 025, and a
window of positive taps that sum to 1:
  * a windowed moment: the kernel adds 11 + 11 fused multiply-adds and (float and Y inputs) one rounded product; the restatement adds 121 terms of a rounded product
    with a rounded 2-D tap; the two sets of taps are roundings of the same numbers through exp, a sum and a division (a few u each way, 10 u allowed).  Each of these
    K = 22 + 1 + 122 + 10 = 155 (160 used) roundings moves the moment by at most u times the largest magnitude in play:
        d_mu = K u 255                    d_E = K u 65 025
  * mu^2 and mu1 mu2:  d_musq = 2 * 255 * d_mu + 2 u 65 025 (both sides round the product);   sigma = E - mu^2:  d_sigma = d_E + d_musq (+ u 65 025, inside the 160)
  * luminance term l = (2 mu1 mu2 + c1) / (mu1^2 + mu2^2 + c1), 0 < l <= 1, denominator >= c1 = 6.5025:      d_l = (2 d_musq + l * 2 d_musq) / c1 <= 4 d_musq / c1
  * contrast term cs = (2 s12 + c2) / (s1 + s2 + c2), |cs| <= 1 (|2 s12| <= s1 + s2), denominator >= c2 = 58.5225:      d_cs <= 4 d_sigma / c2
  * map value l cs:  d <= d_l + d_cs (the few roundings of the quotients and the product, u each, are below 1e-15); the mean of the map moves by no more than its
    largest term, plus the two summations over the positions: n_positions 2^-52 (|map| <= 1).
That is 1.43e-9 + 0.24e-9 = 1.67e-9 (asserted below to be under 1e-8).  No measured figure enters.  The kernel's own tile (tg_image_metrics_tile) gives the two shapes
"exactly one tile" and "one row and one column more"."""
import pytest
import torch

import metrics_ref as MR

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
U = 2.0 ** -53
K_ROUNDINGS = 160
D_MU, D_E = K_ROUNDINGS * U * 255.0, K_ROUNDINGS * U * 65025.0
D_MUSQ = 2 * 255.0 * D_MU + 2 * U * 65025.0
SSIM_BOUND = 4 * D_MUSQ / MR.C1 + 4 * (D_E + D_MUSQ) / MR.C2
assert 1e-9 < SSIM_BOUND < 1e-8


def _tile():
    from tokensgen_amd import lib as L
    return L.load().tg_image_metrics_tile(0), L.load().tg_image_metrics_tile(1)


def _shapes():
    th, tw = _tile()
    return [(11, 11), (12, 75), (26, 138), (43, 139), (77, 203), (120, 184), (th + 10, tw + 10), (th + 11, tw + 11)]


SHAPE_NAMES = ["11x11_one_window", "12x75", "26x138", "43x139", "77x203_rows_of_609_bytes", "120x184_several_tiles", "one_tile_exactly", "one_tile_plus_a_row_and_a_column"]
DTYPES = {"uint8": torch.uint8, "fp32": torch.float32, "bf16": BF}


def _pair(dtype, n, C, H, W, seed):
    """Two related pictures (smooth ramp + noise, the second one disturbed): SSIM well inside (0, 1).  uint8: [n, H, W, 3]; floats: [n, C, H, W] in [0, 1]."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    base = (0.5 + 0.3 * torch.sin(yy / 5.0 + torch.arange(n).view(n, 1, 1, 1)) * torch.cos(xx / 7.0 + torch.arange(C).view(1, C, 1, 1))) + 0.1 * torch.randn(n, C, H, W, generator=g)
    a = base.clamp(0, 1)
    b = (base + 0.08 * torch.randn(n, C, H, W, generator=g)).clamp(0, 1)
    if dtype == torch.uint8:
        assert C == 3
        return tuple((t * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous() for t in (a, b))
    return a.to(dtype), b.to(dtype)


def _check(got, ref, exact_sse, parity, what):
    """got: [n, planes, 2] from the kernel; ref: metrics_ref's dict.  Every plane."""
    got = got.reshape(-1, got.shape[-2], 2).cpu()
    assert got.shape[:2] == ref["sse"].shape and got.dtype == torch.float64
    if exact_sse:
        assert torch.equal(got[..., 0], ref["sse"]), what
    else:
        gap = (got[..., 0] - ref["sse"]).abs()
        assert bool((gap <= ref["n_pixels"] * 2.0 ** -52 * ref["sse"]).all()), (what, gap.max().item())
    ssim = got[..., 1] / ref["n_positions"]
    worst = ((ssim - ref["ssim_mean"]).abs() / (SSIM_BOUND + ref["n_positions"] * 2.0 ** -52)).max().item()
    print(what, "ssim", ref["ssim_mean"].min().item(), "..", ref["ssim_mean"].max().item(), "worst ratio", worst)
    parity(worst, 1.0, f"image_metrics {what}: worst |ssim - fp64 restatement| / derived bound")


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("si", range(8), ids=SHAPE_NAMES)
def test_every_plane_within_the_derived_bound(si, dt, parity):
    """Every shape with every dtype; frames 1 / 3 / 5 and crop_border 0 / 4 rotate over the cases; per case C = 3 per channel, C = 3 as Y and (floats) C = 1."""
    from tokensgen_amd import kernels as K
    dtype, d = DTYPES[dt], list(DTYPES).index(dt)
    h, w = _shapes()[si]
    n, cb = (1, 3, 5)[(si + d) % 3], (0, 4)[(si + d // 2) % 2]
    H, W = h + 2 * cb, w + 2 * cb                                       # the plane the kernel sees is h x w: the listed shape
    variants = [(3, False), (3, True)] + ([(1, False)] if dtype != torch.uint8 else [])
    for C, y in variants:
        a, b = _pair(dtype, n, C, H, W, seed=100 * si + 10 * d + C + y)
        ref = MR.metrics_ref(a, b, cb, y)
        assert 0.05 < ref["ssim_mean"].mean().item() < 0.99
        got = K.image_metrics(a.to(DEV), b.to(DEV), "hwc" if dtype == torch.uint8 else "chw", cb, y)
        assert got.shape == (1, n, 1 if y else C, 2) and got.is_cuda
        _check(got, ref, dtype == torch.uint8 and not y, parity, f"{SHAPE_NAMES[si]} {dt} n={n} C={C} crop={cb} y={y}")


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_strided_bcthw_view_needs_no_copy(dt, parity):
    """[B, 3, T, H, W] as a window of a larger buffer (rows not contiguous, nothing contiguous but the pixels) against a contiguous second input, through video_metrics."""
    from tokensgen_amd.metrics import video_metrics
    dtype = DTYPES[dt]
    B, T, H, W = 2, 3, 29, 45
    a, b = _pair(dtype, B * T, 3, H, W, seed=77)
    a5, b5 = (t.view(B, T, 3, H, W).permute(0, 2, 1, 3, 4).contiguous() for t in (a, b))          # [B, 3, T, H, W]
    big = torch.zeros(B, 3, T + 1, H + 3, W + 5, dtype=dtype, device=DEV)
    big[:, :, 1:, 2:2 + H, 4:4 + W] = a5.to(DEV)
    view = big[:, :, 1:, 2:2 + H, 4:4 + W]
    assert not view.is_contiguous() and view.stride(3) == W + 5
    for cb, y in ((0, False), (4, True)):
        m = video_metrics(view, b5.to(DEV), cb, y)
        ref = MR.metrics_ref(a5, b5, cb, y)
        assert m["ssim"].shape == (B, T) and m["mse"].dtype == torch.float64
        assert torch.equal(m["ssim"], video_metrics(a5.to(DEV), b5.to(DEV), cb, y)["ssim"])     # the view and its contiguous copy: the same bits
        worst = ((m["ssim"].cpu().reshape(-1) - ref["ssim"]).abs() / (SSIM_BOUND + ref["n_positions"] * 2.0 ** -52)).max().item()
        parity(worst, 1.0, f"video_metrics strided bcthw {dt} crop={cb} y={y}: worst |ssim - fp64| / derived bound")
        assert bool(((m["mse"].cpu().reshape(-1) - ref["mse"]).abs() <= 3 * ref["n_pixels"] * 2.0 ** -52 * ref["mse"]).all())
        assert abs(m["psnr_pooled"].item() - ref["psnr_pooled"].item()) < 1e-9 and abs(m["ssim_pooled"].item() - ref["ssim_pooled"].item()) < SSIM_BOUND + 1e-12


def test_closed_forms_on_the_device(parity):
    from tokensgen_amd import kernels as K
    from tokensgen_amd.metrics import video_metrics
    th, tw = _tile()
    H, W = th + 19, 2 * tw + 13                                         # 2 x 3 tiles
    a, _ = _pair(torch.uint8, 2, 3, H, W, seed=5)
    same = video_metrics(a.to(DEV), a.clone().to(DEV))
    assert same["ssim"].tolist() == [1.0, 1.0] and same["mse"].tolist() == [0.0, 0.0] and abs(same["psnr_pooled"].item() - 80.0) < 1e-9
    for dtype in (torch.float32, BF):
        af, _ = _pair(dtype, 2, 3, H, W, seed=6)
        for y in (False, True):
            s = video_metrics(af.to(DEV), af.clone().to(DEV), 0, y)
            assert s["ssim"].tolist() == [1.0, 1.0] and s["mse"].tolist() == [0.0, 0.0]
    # flat 0 against flat 255: l = c1 / (255^2 + c1), cs = 1, mse = 1
    z, o = torch.zeros(1, H, W, 3, dtype=torch.uint8), torch.full((1, H, W, 3), 255, dtype=torch.uint8)
    flat = video_metrics(z.to(DEV), o.to(DEV))
    parity(abs(flat["ssim_pooled"].item() - 9.999000099990003e-05) / SSIM_BOUND, 1.0, "flat 0 against flat 255: |ssim - c1 / (255^2 + c1)| / derived bound")
    assert flat["mse"].tolist() == [1.0] and abs(flat["psnr_pooled"].item() - 10 * torch.log10(torch.tensor(1 / (1 + 1e-8), dtype=torch.float64)).item()) < 1e-12
    # a checkerboard against its inverse: negative, and what the restatement says
    cb = MR.checkerboard(2, 1, H, W).to(torch.float32)
    got = K.image_metrics(cb.to(DEV), (1 - cb).to(DEV), "chw")
    ref = MR.metrics_ref(cb, 1 - cb)
    assert (got[..., 1] < 0).all()
    _check(got, ref, True, parity, "checkerboard against its inverse")


def test_bitwise_properties():
    """Run to run; a frame of a 5-frame call against the same frame alone; the reference-named functions against video_metrics; VideoMetrics against one call."""
    from tokensgen_amd import kernels as K
    from tokensgen_amd.metrics import VideoMetrics, calculate_psnr_pt, calculate_ssim_pt, video_metrics
    th, tw = _tile()
    H, W = 2 * th + 15, tw + 21
    a, b = (t.to(DEV) for t in _pair(torch.uint8, 5, 3, H, W, seed=8))
    whole = K.image_metrics(a, b, "hwc", 0, False)
    assert torch.equal(whole, K.image_metrics(a, b, "hwc", 0, False))
    for f in range(5):
        assert torch.equal(whole[:, f], K.image_metrics(a[f:f + 1], b[f:f + 1], "hwc", 0, False)[:, 0]), f
    af, bf = (t.to(DEV) for t in _pair(torch.float32, 5, 3, H, W, seed=9))
    for cb, y in ((0, False), (4, True)):
        wf = K.image_metrics(af, bf, "chw", cb, y)
        assert torch.equal(wf, K.image_metrics(af, bf, "chw", cb, y))
        assert torch.equal(wf[:, 3], K.image_metrics(af[3:4], bf[3:4], "chw", cb, y)[:, 0])
        m = video_metrics(af, bf, cb, y)
        assert calculate_psnr_pt(af, bf, cb, test_y_channel=y).equal(m["psnr_pooled"]) and calculate_ssim_pt(af, bf, cb, test_y_channel=y).equal(m["ssim_pooled"])
        assert m["psnr_pooled"].dim() == 0 and m["psnr_pooled"].dtype == torch.float64 and m["psnr_pooled"].is_cuda
    u8 = video_metrics(a, b)
    # [B, T, H, W, 3] and two updates of a running VideoMetrics against one call on the concatenation
    m5 = video_metrics(a.view(1, 5, H, W, 3), b.view(1, 5, H, W, 3))
    assert m5["ssim"].shape == (1, 5) and torch.equal(m5["ssim"][0], u8["ssim"]) and torch.equal(m5["mse"][0], u8["mse"])
    run = VideoMetrics()
    run.update(a[:2], b[:2])
    run.update(a[2:].view(1, 3, H, W, 3), b[2:].view(1, 3, H, W, 3))
    fin = run.finalize()
    assert fin["frames"] == 5 and torch.equal(fin["mse"], u8["mse"]) and torch.equal(fin["ssim"], u8["ssim"])
    assert torch.equal(fin["psnr_pooled"], u8["psnr_pooled"]) and torch.equal(fin["ssim_pooled"], u8["ssim_pooled"]) and torch.equal(fin["psnr"], u8["psnr"])


def test_decoded_clip_against_itself():
    """What a run hands over: bf16 [B, 3, T, H, W] through VideoProcessor.postprocess_video(output_type="uint8"), compared with itself and with a disturbed decode."""
    from tokensgen_amd.metrics import video_metrics
    from tokensgen_amd.video_io import VideoProcessor
    v = (torch.randn(1, 3, 5, 24, 40, generator=torch.Generator().manual_seed(12)) * 0.5).to(BF).to(DEV)
    vp = VideoProcessor()
    u8 = vp.postprocess_video(v, "uint8")
    m = video_metrics(u8, u8.clone())
    assert m["ssim"].shape == (1, 5) and (m["ssim"] == 1).all() and m["ssim_pooled"].item() == 1.0 and abs(m["psnr_pooled"].item() - 80.0) < 1e-9
    other = vp.postprocess_video((v.float() * 0.9).to(BF), "uint8")
    m2 = video_metrics(u8, other)
    ref = MR.metrics_ref(u8.cpu(), other.cpu())
    assert 0 < m2["ssim_pooled"].item() < 1 and torch.equal(m2["mse"].cpu().reshape(-1), ref["mse"])
    assert (m2["ssim"].cpu().reshape(-1) - ref["ssim"]).abs().max().item() < SSIM_BOUND + ref["n_positions"] * 2.0 ** -52
