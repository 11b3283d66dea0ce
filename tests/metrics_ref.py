"""float64 restatement, with torch on the CPU, of what tokensgen_amd.metrics computes: PSNR and SSIM of two image batches on the 0..255 scale.  Written from the formulas
(the 11-tap gaussian of sigma 1.5 as a 2-D 121-tap window, applied "valid"; the SSIM map from the five windowed moments; BT.601 luma), as plain sums of shifted slices:
no convolution routine, no library metric.  tests/test_metrics_cpu.py holds it to the literal float64 F.conv2d chain, tests/test_metrics_gpu.py holds the kernel to it."""
import math

import torch

TAPS = 11
C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
F64 = torch.float64


def gaussian_window():
    """w[i] = exp(-(i - 5)^2 / (2 * 1.5^2)), normalised in float64 to sum 1"""
    w = torch.tensor([math.exp(-((i - TAPS // 2) ** 2) / (2 * 1.5 ** 2)) for i in range(TAPS)], dtype=F64)
    return w / w.sum()


def window_2d():
    w = gaussian_window()
    return w[:, None] * w[None, :]


def to_255(x):
    """A batch in one of the forms the module takes -> float64 [n, C, H, W] on the 0..255 scale (n = all leading axes flattened, frame-major).
    uint8 [..., H, W, 3] as it is; fp32 / bf16 (n, C, H, W) or [B, C, T, H, W] in [0, 1] times 255."""
    if x.dtype == torch.uint8:
        return x.reshape(-1, *x.shape[-3:]).permute(0, 3, 1, 2).to(F64)
    if x.dim() == 5:
        x = x.permute(0, 2, 1, 3, 4)
        x = x.reshape(-1, *x.shape[-3:])
    return x.to(F64) * 255.0


def luma(x255):
    """[n, 3, H, W] on the 0..255 scale -> Y [n, 1, H, W] on the same scale"""
    r, g, b = x255[:, 0:1], x255[:, 1:2], x255[:, 2:3]
    return (65.481 * r + 128.553 * g + 24.966 * b) / 255.0 + 16.0


def windowed(x):
    """sum_ij w2[i][j] x[.., y + i, x + j] over the valid positions: 121 terms, row-major"""
    w2 = window_2d()
    ho, wo = x.shape[-2] - TAPS + 1, x.shape[-1] - TAPS + 1
    acc = torch.zeros(*x.shape[:-2], ho, wo, dtype=F64)
    for i in range(TAPS):
        for j in range(TAPS):
            acc += w2[i, j] * x[..., i:i + ho, j:j + wo]
    return acc


def ssim_map(a, b):
    mu1, mu2 = windowed(a), windowed(b)
    s1, s2, s12 = windowed(a * a) - mu1 * mu1, windowed(b * b) - mu2 * mu2, windowed(a * b) - mu1 * mu2
    return ((2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)) * ((2 * s12 + C2) / (s1 + s2 + C2))


def prepare(a, b, crop_border=0, y=False):
    a, b = to_255(a), to_255(b)
    if crop_border:
        a, b = (t[..., crop_border:-crop_border, crop_border:-crop_border] for t in (a, b))
    if y:
        a, b = luma(a), luma(b)
    return a, b


def metrics_ref(a, b, crop_border=0, y=False):
    """dict of float64 tensors: per plane "sse" and "ssim_mean" [n, planes] (0..255 scale); per image "mse" (on the [0, 1] scale), "psnr", "ssim" [n]; pooled scalars
    "psnr_pooled", "ssim_pooled"; "n_pixels" and "n_positions" per plane"""
    a, b = prepare(a, b, crop_border, y)
    sse = ((a - b) ** 2).sum(dim=(-2, -1))
    sm = ssim_map(a, b)
    npix, npos = a.shape[-2] * a.shape[-1], sm.shape[-2] * sm.shape[-1]
    mse = sse.sum(-1) / (a.shape[1] * npix * 255.0 * 255.0)
    ssim = sm.mean(dim=(1, 2, 3))
    return {"sse": sse, "ssim_mean": sm.mean(dim=(-2, -1)), "mse": mse, "psnr": 10 * torch.log10(1 / (mse + 1e-8)), "ssim": ssim,
            "psnr_pooled": 10 * torch.log10(1 / (mse.mean() + 1e-8)), "ssim_pooled": ssim.mean(), "n_pixels": npix, "n_positions": npos}


def checkerboard(n, C, H, W):
    """uint8-valued 0 / 255 checkerboard, float64 [n, C, H, W] in [0, 1]"""
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    return ((yy + xx) % 2).to(F64).expand(n, C, H, W).clone()
