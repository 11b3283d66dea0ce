"""tokensgen_amd.metrics without a GPU: the window, the float64 restatement of tests/metrics_ref.py against the literal float64 F.conv2d chain and against closed forms,
the wrapper's argument checks, and the argument checks of the export (no launch).  The kernel is held to the restatement in tests/test_metrics_gpu.py."""
import ctypes

import pytest
import torch
import torch.nn.functional as Fn

import metrics_ref as MR

F64 = torch.float64


def test_window_digits_and_sum():
    w = MR.gaussian_window()
    want = [0.00102838, 0.00759876, 0.03600077, 0.10936069, 0.21300554, 0.26601172]
    assert w.dtype == F64 and w.shape == (11,)
    assert all(abs(w[i].item() - want[i]) < 5e-9 for i in range(6)) and torch.equal(w, w.flip(0))
    assert abs(w.sum().item() - 1.0) < 2.0 ** -50
    assert abs(MR.window_2d().sum().item() - 1.0) < 2.0 ** -48
    # the taps the kernel is launched with (formed on the host by the library) are the same numbers, to the rounding of exp and of the normalisation
    from tokensgen_amd import lib as L
    taps = (ctypes.c_double * 11)()
    assert L.load().tg_image_metrics_window(taps) == 0
    assert max(abs(taps[i] - w[i].item()) / w[i].item() for i in range(11)) < 8 * 2.0 ** -53


def _literal(img, img2, crop_border, test_y_channel):
    """The chain of operations on float64 inputs in [0, 1]: crop, Y, * 255, five grouped 121-tap conv2d's, the map, the means."""
    if crop_border:
        img, img2 = (t[:, :, crop_border:-crop_border, crop_border:-crop_border] for t in (img, img2))
    if test_y_channel:
        wt = torch.tensor([[65.481], [128.553], [24.966]], dtype=F64)
        img, img2 = ((torch.matmul(t.permute(0, 2, 3, 1), wt).permute(0, 3, 1, 2) + 16.0) / 255.0 for t in (img, img2))
    mse = torch.mean((img - img2) ** 2, dim=[1, 2, 3])
    psnr = 10.0 * torch.log10(1.0 / (torch.mean(mse) + 1e-8))
    a, b = img * 255.0, img2 * 255.0
    ch = a.shape[1]
    win = MR.window_2d().view(1, 1, 11, 11).expand(ch, 1, 11, 11)
    conv = lambda t: Fn.conv2d(t, win, stride=1, padding=0, groups=ch)
    mu1, mu2 = conv(a), conv(b)
    s1, s2, s12 = conv(a * a) - mu1.pow(2), conv(b * b) - mu2.pow(2), conv(a * b) - mu1 * mu2
    m = ((2 * mu1 * mu2 + MR.C1) / (mu1.pow(2) + mu2.pow(2) + MR.C1)) * ((2 * s12 + MR.C2) / (s1 + s2 + MR.C2))
    return mse, psnr, m.mean([1, 2, 3])


@pytest.mark.parametrize("C,y,crop", [(3, False, 0), (3, True, 0), (1, False, 0), (3, False, 4), (3, True, 3)])
def test_restatement_agrees_with_the_literal_conv2d_chain(C, y, crop):
    g = torch.Generator().manual_seed(10 * C + crop)
    a = torch.rand(3, C, 37, 52, generator=g, dtype=F64)
    b = (a + 0.1 * torch.randn(3, C, 37, 52, generator=g, dtype=F64)).clamp(0, 1)
    ref = MR.metrics_ref(a, b, crop, y)
    mse, psnr, ssim = _literal(a, b, crop, y)
    gaps = ((ref["mse"] - mse).abs().max().item(), abs(ref["psnr_pooled"].item() - psnr.item()), (ref["ssim"] - ssim).abs().max().item())
    print("gaps", gaps)
    assert max(gaps) < 1e-12 and 0.2 < ssim.mean().item() < 0.999
    assert ref["sse"].shape == (3, 1 if y else C) and ref["n_positions"] == (37 - 2 * crop - 10) * (52 - 2 * crop - 10)


def test_closed_forms():
    g = torch.Generator().manual_seed(1)
    a = torch.randint(0, 256, (2, 20, 31, 3), generator=g, dtype=torch.uint8)
    same = MR.metrics_ref(a, a.clone())
    assert (same["ssim"] - 1).abs().max().item() < 1e-12 and same["sse"].eq(0).all() and abs(same["psnr_pooled"].item() - 80.0) < 1e-9
    flat = MR.metrics_ref(torch.zeros(1, 3, 14, 17, dtype=F64), torch.ones(1, 3, 14, 17, dtype=F64))
    assert abs(flat["ssim_pooled"].item() - 9.999000099990003e-05) < 1e-15 and abs(MR.C1 / (255.0 ** 2 + MR.C1) - 9.999000099990003e-05) < 1e-18
    assert flat["mse"].tolist() == [1.0]
    cb = MR.checkerboard(2, 1, 24, 30)
    inv = MR.metrics_ref(cb, 1 - cb)
    assert inv["ssim"].max().item() < 0 and inv["mse"].tolist() == [1.0, 1.0]
    # luma of black, white and of a uint8 frame: 16, 235, and the same through the float form
    assert MR.luma(torch.zeros(1, 3, 1, 1, dtype=F64)).item() == 16.0 and abs(MR.luma(torch.full((1, 3, 1, 1), 255.0, dtype=F64)).item() - 235.0) < 1e-12
    yu = MR.metrics_ref(a, a.flip(1), y=True)
    yf = MR.metrics_ref(a.permute(0, 3, 1, 2).to(F64) / 255.0, a.flip(1).permute(0, 3, 1, 2).to(F64) / 255.0, y=True)
    assert (yu["ssim"] - yf["ssim"]).abs().max().item() < 1e-12 and yu["sse"].shape == (2, 1)


def test_wrapper_refuses_bad_arguments_and_cpu_tensors():
    from tokensgen_amd import kernels as K
    from tokensgen_amd import metrics as M
    z = torch.zeros
    with pytest.raises(ValueError, match="smaller than the 11 x 11 window"):
        K.image_metrics(z(1, 3, 10, 40), z(1, 3, 10, 40), "chw")
    with pytest.raises(ValueError, match="smaller than the 11 x 11 window"):
        M.video_metrics(z(2, 18, 40, 3, dtype=torch.uint8), z(2, 18, 40, 3, dtype=torch.uint8), crop_border=4)
    with pytest.raises(TypeError):
        K.image_metrics(z(1, 3, 16, 16, dtype=torch.float16), z(1, 3, 16, 16, dtype=torch.float16), "chw")
    with pytest.raises(TypeError):
        K.image_metrics(z(1, 3, 16, 16), z(1, 3, 16, 16, dtype=torch.bfloat16), "chw")
    with pytest.raises(ValueError, match="shapes are different"):
        K.image_metrics(z(1, 3, 16, 16), z(1, 3, 16, 17), "chw")
    for fn in (M.calculate_psnr_pt, M.calculate_ssim_pt):
        with pytest.raises(AssertionError, match="Image shapes are different"):
            fn(z(1, 3, 16, 16), z(1, 3, 16, 17), 0)
    with pytest.raises(AssertionError, match="Image shapes are different"):
        M.video_metrics(z(1, 3, 16, 16), z(2, 3, 16, 16))
    with pytest.raises(ValueError):
        K.image_metrics(z(1, 2, 16, 16), z(1, 2, 16, 16), "chw")                   # 1 or 3 channels
    with pytest.raises(ValueError):
        M.calculate_ssim_pt(z(1, 1, 16, 16), z(1, 1, 16, 16), 0, test_y_channel=True)
    with pytest.raises(ValueError):
        K.image_metrics(z(1, 3, 16, 16), z(1, 3, 16, 16), "hwc3")
    with pytest.raises(ValueError):
        M.video_metrics(z(16, 16, 3, dtype=torch.uint8), z(16, 16, 3, dtype=torch.uint8))
    for fn in (M.calculate_psnr_pt, M.calculate_ssim_pt):
        with pytest.raises(RuntimeError, match="GPU"):
            fn(z(1, 3, 16, 16), z(1, 3, 16, 16), 0)
    with pytest.raises(RuntimeError, match="GPU"):
        M.VideoMetrics().update(z(2, 16, 16, 3, dtype=torch.uint8), z(2, 16, 16, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no update"):
        M.VideoMetrics().finalize()


def test_new_export_validates_its_arguments_without_a_launch():
    from tokensgen_amd import lib as L
    lib = L.load()
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.addressof(buf) + (16 - ctypes.addressof(buf) % 16)
    err = lambda: lib.tg_last_error_string().decode()
    args = dict(a=p, a_so=0, a_si=768, a_sc=256, a_sr=16, a_sp=1, b=p, b_so=0, b_si=768, b_sc=256, b_sr=16, b_sp=1, dtype=1, n_outer=1, n_inner=1, C=3, h=16, w=16, y_only=0,
                ws=p, out=p, stream=None)                                           # in the order of the prototype
    im = lambda **kw: lib.tg_image_metrics(*{**args, **kw}.values())
    for name in ("a", "b", "ws", "out"):
        assert im(**{name: None}) == -1 and "null pointer" in err(), name
    assert im(dtype=3) == -1 and im(dtype=-1) == -1 and im(y_only=2) == -1
    for name in ("n_outer", "n_inner", "C"):
        assert im(**{name: 0}) == -2 and "bad shape" in err(), name
    assert im(C=2) == -2 and im(C=1, y_only=1) == -2
    for name in ("h", "w"):
        assert im(**{name: 10}) == -2 and "smaller than the 11 x 11 window" in err(), name
    for name in ("a_so", "a_si", "a_sc", "a_sr", "a_sp", "b_so", "b_si", "b_sc", "b_sr", "b_sp"):
        assert im(**{name: -1}) == -2 and "negative stride" in err(), name
    assert im(a=p + 2) == -3 and im(dtype=2, b=p + 1) == -3 and im(ws=p + 4) == -3 and im(dtype=0, a=p + 1, out=p + 4) == -3
    assert lib.tg_image_metrics_window(None) == -1 and "null pointer" in err()
    # the workspace: one pair per tile of window positions
    th, tw = lib.tg_image_metrics_tile(0), lib.tg_image_metrics_tile(1)
    assert th >= 1 and tw >= 1 and lib.tg_image_metrics_tile(2) == 0
    assert lib.tg_image_metrics_ws_doubles(1, 11, 11) == 2 and lib.tg_image_metrics_ws_doubles(5, th + 10, tw + 10) == 10
    assert lib.tg_image_metrics_ws_doubles(5, th + 11, tw + 10) == 20 and lib.tg_image_metrics_ws_doubles(5, th + 11, tw + 11) == 40
    assert lib.tg_image_metrics_ws_doubles(0, 16, 16) == 0 and lib.tg_image_metrics_ws_doubles(1, 10, 16) == 0
