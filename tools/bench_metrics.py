#!/usr/bin/env python3
"""tokensgen_amd.metrics.video_metrics at a user's size next to the torch route on the same device, in the same process, alternating:

  video_metrics     49 frames of 480 x 720 x 3, as uint8 [49, 480, 720, 3] and as fp32 [49, 3, 480, 720]: one tg_image_metrics call (two launches)
  torch route       the reference's chain on the GPU: `.to(float64)` of both videos, `* 255.`, three full-size products, five depthwise 11 x 11 float64 conv2d's, the
                    SSIM map and its means, and the float64 squared error (longvgen/metrics/psnr_ssim.py calculate_psnr_pt + calculate_ssim_pt, restated)

Times are device events around `reps` back-to-back calls after a warm-up, the median of `rounds` alternating rounds; peak memory is torch's allocator peak over one call
of the route, above what the inputs hold.  There is no pass / fail threshold: the parent commit has no such path and the torch route is the yardstick.  The figures go
to profiles/metrics_bench.json.

    python tools/bench_metrics.py [--frames 49] [--out profiles/metrics_bench.json]"""
import argparse
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as Fn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tokensgen_amd import metrics as M  # noqa: E402

C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def torch_route(img, img2):
    """img, img2 (n, 3, h, w) in [0, 1], any float dtype -> (psnr, ssim) as the reference computes them"""
    a, b = img.to(torch.float64), img2.to(torch.float64)
    mse = torch.mean(torch.mean((a - b) ** 2, dim=[1, 2, 3]))
    psnr = 10.0 * torch.log10(1.0 / (mse + 1e-8))
    a, b = a * 255.0, b * 255.0
    w = torch.tensor([math.exp(-((i - 5) ** 2) / (2 * 1.5 ** 2)) for i in range(11)], dtype=torch.float64, device=a.device)
    w = w / w.sum()
    win = (w[:, None] * w[None, :]).view(1, 1, 11, 11).expand(a.shape[1], 1, 11, 11)
    conv = lambda t: Fn.conv2d(t, win, stride=1, padding=0, groups=t.shape[1])
    mu1, mu2 = conv(a), conv(b)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1, s2, s12 = conv(a * a) - mu1_sq, conv(b * b) - mu2_sq, conv(a * b) - mu1_mu2
    cs = (2 * s12 + C2) / (s1 + s2 + C2)
    ssim = (((2 * mu1_mu2 + C1) / (mu1_sq + mu2_sq + C1)) * cs).mean([1, 2, 3])
    return psnr, ssim.mean()


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - before


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=49)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-reps", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics.py measures on the GPU: no device found")
    dev, F, H, W = torch.device("cuda", 0), a.frames, 480, 720
    g = torch.Generator(device=dev).manual_seed(1)
    # a picture-like pair: smooth content plus noise, the second video disturbed (the time does not depend on the values)
    base = Fn.interpolate(torch.rand(F, 3, H // 16, W // 16, generator=g, device=dev), size=(H, W), mode="bilinear")
    va = (base * 0.8 + 0.2 * torch.rand(F, 3, H, W, generator=g, device=dev)).clamp(0, 1)
    vb = (va + 0.05 * torch.randn(F, 3, H, W, generator=g, device=dev)).clamp(0, 1)
    del base
    u8a, u8b = ((t * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous() for t in (va, vb))
    f32a, f32b = u8a.permute(0, 3, 1, 2).float() / 255, u8b.permute(0, 3, 1, 2).float() / 255      # the same pictures: what a pipeline holds after `/ 255.`
    del va, vb
    routes = {
        "uint8": lambda: M.video_metrics(u8a, u8b),
        "uint8_torch": lambda: torch_route(u8a.permute(0, 3, 1, 2).to(torch.float64) / 255.0, u8b.permute(0, 3, 1, 2).to(torch.float64) / 255.0),
        "fp32": lambda: M.video_metrics(f32a, f32b),
        "fp32_torch": lambda: torch_route(f32a, f32b),
        "fp32_y": lambda: M.video_metrics(f32a, f32b, test_y_channel=True),
    }
    agree = {}
    for k in ("uint8", "fp32"):
        ours, (psnr, ssim) = routes[k](), routes[k + "_torch"]()
        agree[k] = {"psnr": ours["psnr_pooled"].item(), "psnr_torch": psnr.item(), "ssim": ours["ssim_pooled"].item(), "ssim_torch": ssim.item(),
                    "abs_gap_psnr": abs(ours["psnr_pooled"].item() - psnr.item()), "abs_gap_ssim": abs(ours["ssim_pooled"].item() - ssim.item())}
        del ours, psnr, ssim
    peak = {k: peak_bytes(fn) for k, fn in routes.items()}
    t = {k: [] for k in routes}
    for _ in range(a.rounds):                                  # alternate: drift of the shared machine hits every route alike
        for k, fn in routes.items():
            t[k].append(timed(fn, a.torch_reps if k.endswith("_torch") else a.reps))
    med = {k: statistics.median(v) for k, v in t.items()}
    nbytes = {"uint8": 2 * u8a.numel(), "fp32": 2 * f32a.numel() * 4, "fp32_y": 2 * f32a.numel() * 4}
    positions = F * 3 * (H - 10) * (W - 10)
    res = {"device": torch.cuda.get_device_name(0), "frames": F, "shape": [F, H, W, 3], "reps": a.reps, "torch_reps": a.torch_reps, "rounds": a.rounds, "median_ms": med,
           "all_rounds_ms": t, "peak_bytes_above_inputs": peak, "agreement": agree, "input_bytes": nbytes,
           "speedup_vs_torch": {k: med[k + "_torch"] / med[k] for k in ("uint8", "fp32")},
           "peak_memory_ratio_torch_over_ours": {k: peak[k + "_torch"] / max(peak[k], 1) for k in ("uint8", "fp32")},
           "input_bytes_per_s": {k: nbytes[k] / (med[k] * 1e-3) for k in nbytes},
           "fp64_fma_per_s": {k: positions * 110 * (1 / 3 if k == "fp32_y" else 1) * 1.3 / (med[k] * 1e-3) for k in nbytes}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps({k: v for k, v in res.items() if k != "all_rounds_ms"}))


if __name__ == "__main__":
    main()
