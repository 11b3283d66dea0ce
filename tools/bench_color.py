#!/usr/bin/env python3
"""The four kernels of csrc/color.hip and tokensgen_amd.color.match_colors at a user's size next to a torch route on the same device, in the same process, alternating:

  hist         49 frames of 480 x 720 x 3 uint8: tg_color_hist_u8 on noise, on a picture-like clip and on a flat black clip (every lane on one bin: the contention
               case); torch: `bincount` per frame and channel, and one `bincount` over (frame, channel, value) keys
  lut          tg_color_match_lut, both modes, window 3; torch: the definitions batched over frames and channels (cumsum, a [F, 3, 256, 256] comparison)
  apply        tg_color_apply_lut out of place and in place; torch: `torch.gather` on the int64 bytes
  lab          tg_lab_metrics, one input (colour drift) and two (dE), uint8; torch: the float64 Lab chain elementwise
  match_colors the whole call (histograms, tables, apply), both modes; torch: the three torch routes above chained

Times are device events around `reps` back-to-back calls after a warm-up, the median of `rounds` alternating rounds.  There is no pass / fail threshold: the parent
commit has no such path.  The tool checks that both routes agree (integers exactly, the Lab means to 1e-9) and records next to the times the memory floor at 8 TB/s:
the clip read once for the histogram and the Lab sums, read and written for the apply.  The figures go to profiles/color_bench.json.

    python tools/bench_color.py [--frames 49] [--out profiles/color_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as Fn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tokensgen_amd import color  # noqa: E402
from tokensgen_amd import kernels as K  # noqa: E402

HBM_BYTES_PER_S = 8e12


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def torch_hist_loop(frames):
    F = frames.shape[0]
    return torch.stack([torch.stack([torch.bincount(frames[f, :, :, c].reshape(-1).long(), minlength=256) for c in range(3)]) for f in range(F)])


def torch_hist_fused(frames):
    F = frames.shape[0]
    key = frames.reshape(F, -1, 3).long() + (torch.arange(F, device=frames.device)[:, None, None] * 3 + torch.arange(3, device=frames.device)[None, None, :]) * 256
    return torch.bincount(key.reshape(-1), minlength=F * 768).reshape(F, 3, 256)


def torch_window(hist, window):
    c = torch.cat([torch.zeros_like(hist[:1]), hist.cumsum(0)])
    t = torch.arange(hist.shape[0], device=hist.device)
    return c[t + 1] - c[(t - window + 1).clamp_min(0)]


def torch_luts(hist, anchor, mode, strength, window, max_gain):
    S = torch_window(hist.long(), window)                                       # [F, 3, 256]
    v = torch.arange(256, device=hist.device)
    if mode == "histogram":
        cs, cr = S.cumsum(-1), anchor.cumsum(-1)
        m = ((cr * cs[..., 255:])[:, :, None, :] < (cs * cr[..., 255:])[..., None]).sum(-1)
        return (v.double() + strength * (m - v).double()).round().clamp(0, 255).to(torch.uint8)

    def mom(h):
        n, s1, s2 = h.sum(-1).double(), (v * h).sum(-1).double(), (v * v * h).sum(-1).double()
        mean = s1 / n
        return mean, (s2 / n - mean * mean).clamp_min(0).sqrt()

    (ms, ss), (mr, sr) = mom(S), mom(anchor)
    g = torch.where(ss > 0, sr / ss, torch.ones_like(ss)).clamp(1.0 / max_gain, max_gain)
    g2, m2 = 1.0 + strength * (g - 1.0), ms + strength * (mr - ms)
    return ((v.double() - ms[..., None]) * g2[..., None] + m2[..., None]).round().clamp(0, 255).to(torch.uint8)


def torch_apply(frames, luts):
    F, H, W, _ = frames.shape
    idx = frames.reshape(F, H * W, 3).permute(0, 2, 1).long()
    return torch.gather(luts, 2, idx).permute(0, 2, 1).reshape(F, H, W, 3).contiguous()


def torch_lab(frames):
    """uint8 [F, H, W, 3] -> float64 [F, H, W, 3] L, a, b"""
    c = frames.double() / 255.0
    lin = torch.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055).pow(2.4))
    R, G, B = lin[..., 0], lin[..., 1], lin[..., 2]
    X = (0.412453 * R + 0.357580 * G + 0.180423 * B) / 0.950456
    Y = 0.212671 * R + 0.715160 * G + 0.072169 * B
    Z = (0.019334 * R + 0.119193 * G + 0.950227 * B) / 1.088754
    f = lambda t: torch.where(t > 0.008856, t.pow(1.0 / 3.0), 7.787 * t + 16.0 / 116.0)
    fy = f(Y)
    return torch.stack([torch.where(Y > 0.008856, 116.0 * fy - 16.0, 903.3 * Y), 500.0 * (f(X) - fy), 200.0 * (fy - f(Z))], -1)


def torch_lab_means(frames):
    lab = torch_lab(frames)
    return torch.cat([lab.mean((1, 2)), lab[..., 1:].pow(2).sum(-1).sqrt().mean((1, 2))[:, None]], 1)


def torch_delta_e(a, b):
    return (torch_lab(a) - torch_lab(b)).pow(2).sum(-1).sqrt().mean((1, 2))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=49)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-reps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "color_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_color.py measures on the GPU: no device found")
    dev, F, H, W = torch.device("cuda", 0), a.frames, 480, 720
    g = torch.Generator(device=dev).manual_seed(1)
    noise = torch.randint(0, 256, (F, H, W, 3), generator=g, device=dev, dtype=torch.uint8)
    black = torch.zeros(F, H, W, 3, dtype=torch.uint8, device=dev)
    # a picture-like clip whose exposure and white balance drift (what match_colors is for)
    base = Fn.interpolate(torch.rand(1, 3, 40, 56, generator=g, device=dev), size=(H, W), mode="bicubic")[0].clamp(0, 1)
    gain = 1.0 + torch.arange(F, device=dev)[:, None, None, None] * torch.tensor([0.006, 0.002, -0.004], device=dev)[None, :, None, None]
    picture = ((base[None] * gain * 0.8 + 0.02 * torch.randn(F, 3, H, W, generator=g, device=dev)).clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    other = noise[:F].roll(1, 0).contiguous()
    hist = K.color_hist_u8(picture)
    anchor = hist[:8].sum(0, dtype=torch.int64)
    luts = {m: K.color_match_lut(hist, anchor, m, 1.0, 3, 4.0)[0] for m in ("meanstd", "histogram")}
    scratch = picture.clone()

    agree = {
        "hist_noise": torch.equal(K.color_hist_u8(noise).long(), torch_hist_fused(noise)), "hist_black": torch.equal(K.color_hist_u8(black).long(), torch_hist_fused(black)),
        "hist_picture": torch.equal(hist.long(), torch_hist_loop(picture)),
        "lut_meanstd": torch.equal(luts["meanstd"], torch_luts(hist, anchor, "meanstd", 1.0, 3, 4.0)),
        "lut_histogram": torch.equal(luts["histogram"], torch_luts(hist, anchor, "histogram", 1.0, 3, 4.0)),
        "apply": torch.equal(K.color_apply_lut(picture, luts["histogram"]), torch_apply(picture, luts["histogram"])),
        "lab_means_max_abs": float((K.lab_metrics(picture, None, "hwc")[0] / (H * W) - torch_lab_means(picture)).abs().max()),
        "delta_e_max_abs": float((K.lab_metrics(picture, other, "hwc")[0, :, 8] / (H * W) - torch_delta_e(picture, other)).abs().max()),
        "match_colors_meanstd": torch.equal(color.match_colors(picture, None, 8, "meanstd", 1.0, 3), torch_apply(picture, torch_luts(torch_hist_fused(picture), anchor, "meanstd", 1.0, 3, 4.0))),
    }
    routes = {
        "hist_noise": lambda: K.color_hist_u8(noise), "hist_picture": lambda: K.color_hist_u8(picture), "hist_black": lambda: K.color_hist_u8(black),
        "hist_noise_torch": lambda: torch_hist_loop(noise), "hist_black_torch": lambda: torch_hist_loop(black),
        "hist_noise_torch_fused": lambda: torch_hist_fused(noise), "hist_black_torch_fused": lambda: torch_hist_fused(black),
        "lut_meanstd": lambda: K.color_match_lut(hist, anchor, "meanstd", 1.0, 3, 4.0), "lut_meanstd_torch": lambda: torch_luts(hist, anchor, "meanstd", 1.0, 3, 4.0),
        "lut_histogram": lambda: K.color_match_lut(hist, anchor, "histogram", 1.0, 3, 4.0), "lut_histogram_torch": lambda: torch_luts(hist, anchor, "histogram", 1.0, 3, 4.0),
        "apply": lambda: K.color_apply_lut(picture, luts["histogram"]), "apply_in_place": lambda: K.color_apply_lut(scratch, luts["histogram"], scratch),
        "apply_noise": lambda: K.color_apply_lut(noise, luts["histogram"]), "apply_torch": lambda: torch_apply(picture, luts["histogram"]),
        "lab_one": lambda: K.lab_metrics(picture, None, "hwc"), "lab_one_torch": lambda: torch_lab_means(picture),
        "lab_two": lambda: K.lab_metrics(picture, other, "hwc"), "lab_two_torch": lambda: torch_delta_e(picture, other),
    }
    for m in ("meanstd", "histogram"):
        routes[f"match_colors_{m}"] = lambda m=m: color.match_colors(picture, None, 8, m, 1.0, 3)
        routes[f"match_colors_{m}_torch"] = lambda m=m: torch_apply(picture, torch_luts((h := torch_hist_fused(picture)), h[:8].sum(0), m, 1.0, 3, 4.0))
    for fn in routes.values():                                 # warm-up
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in routes}
    for _ in range(a.rounds):                                  # alternate: drift of the shared machine hits every route alike
        for k, fn in routes.items():
            t[k].append(timed(fn, a.torch_reps if "_torch" in k else a.reps))
    med = {k: statistics.median(v) for k, v in t.items()}
    clip = F * H * W * 3
    floor_ms = {"hist": clip / HBM_BYTES_PER_S * 1e3, "apply": 2 * clip / HBM_BYTES_PER_S * 1e3, "lab_one": clip / HBM_BYTES_PER_S * 1e3, "lab_two": 2 * clip / HBM_BYTES_PER_S * 1e3}
    pairs = [(k, k + "_torch") for k in routes if k + "_torch" in routes] + [("hist_noise", "hist_noise_torch_fused"), ("hist_black", "hist_black_torch_fused"),
                                                                              ("apply_in_place", "apply_torch")]
    speed = {f"{k}_vs_{ref}": med[ref] / med[k] for k, ref in pairs}
    res = {"device": torch.cuda.get_device_name(0), "shape": [F, H, W, 3], "clip_bytes": clip, "reps": a.reps, "torch_reps": a.torch_reps, "rounds": a.rounds,
           "median_ms": med, "all_rounds_ms": t, "agreement": agree, "speedup_vs_torch": speed, "memory_floor_ms_at_8TBps": floor_ms,
           "fraction_of_floor": {"hist_noise": floor_ms["hist"] / med["hist_noise"], "hist_black": floor_ms["hist"] / med["hist_black"],
                                 "apply": floor_ms["apply"] / med["apply"], "lab_one": floor_ms["lab_one"] / med["lab_one"], "lab_two": floor_ms["lab_two"] / med["lab_two"]},
           "hist_black_over_noise": med["hist_black"] / med["hist_noise"]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps({k: v for k, v in res.items() if k != "all_rounds_ms"}))


if __name__ == "__main__":
    main()
