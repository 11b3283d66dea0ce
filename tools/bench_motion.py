#!/usr/bin/env python3
"""tokensgen_amd.metrics.video_motion and video_warp_error at a user's size next to the torch route on the same device, in the same process, alternating:

  video_motion       49 frames of 480 x 720 x 3 uint8, block 16, radius 16 and 32: tg_luma_u8 + tg_block_motion (two launches) and the summary arithmetic
  video_warp_error   the same search, then tg_block_warp_sse
  torch route        the same definitions with torch on the GPU: integer luma, then one pass per candidate (dy, dx): a shifted `abs` of the difference, `avg_pool2d`
                     times block^2 for the block sums (exact in fp32: at most 65 280), the packed 64-bit key and a running `minimum`; the warp error by a gather

Times are device events around `reps` back-to-back calls after a warm-up, the median of `rounds` alternating rounds.  There is no pass / fail threshold: the parent
commit has no such path and the torch route is the yardstick.  The tool checks that both routes give the same vectors and costs, and records next to the times the
count of byte absolute differences the shape implies (every candidate of every block, legal or not: what the kernel evaluates is reported separately) and the
achieved rate.  The figures go to profiles/motion_bench.json.

    python tools/bench_motion.py [--frames 49] [--out profiles/motion_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as Fn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tokensgen_amd import metrics as M  # noqa: E402
from tokensgen_amd import motion  # noqa: E402


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def torch_search(frames, block, R):
    """uint8 [F, H, W, 3] -> (mv int16 [F - 1, Hb, Wb, 2], sad, sad0 int32): the definitions, one pass per candidate"""
    f = frames.to(torch.int32)
    y = ((77 * f[..., 0] + 150 * f[..., 1] + 29 * f[..., 2] + 128) >> 8).to(torch.float32)
    P, H, W = y.shape[0] - 1, y.shape[1], y.shape[2]
    Hb, Wb = H // block, W // block
    cur = y[:-1, :Hb * block, :Wb * block]
    pad = Fn.pad(y[1:], (R, R, R, R))
    ys = torch.arange(Hb, device=y.device)[:, None] * block
    xs = torch.arange(Wb, device=y.device)[None, :] * block
    best = torch.full((P, Hb, Wb), torch.iinfo(torch.int64).max, dtype=torch.int64, device=y.device)
    sad0 = None
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            sad = (Fn.avg_pool2d((cur - pad[:, R + dy:R + dy + Hb * block, R + dx:R + dx + Wb * block]).abs()[:, None], block)[:, 0] * (block * block)).round().to(torch.int64)
            if dy == 0 and dx == 0:
                sad0 = sad
            legal = (ys + dy >= 0) & (ys + dy + block <= H) & (xs + dx >= 0) & (xs + dx + block <= W)
            key = (sad << 26) | ((dy * dy + dx * dx) << 14) | ((dy + 64) << 7) | (dx + 64)
            best = torch.minimum(best, torch.where(legal[None], key, best))
    mv = torch.stack([((best >> 7) & 127) - 64, (best & 127) - 64], -1).to(torch.int16)
    return mv, (best >> 26).to(torch.int32), sad0.to(torch.int32)


def torch_warp(frames, mv, block):
    """(sse, sse0) int64 [F - 1, Hb, Wb] by a gather of the displaced blocks"""
    cur, oth = frames[:-1].to(torch.int64), frames[1:].to(torch.int64)
    P, H, W, _ = cur.shape
    Hb, Wb = H // block, W // block
    dev = frames.device
    i = torch.arange(block, device=dev)
    v = mv.to(torch.int64)
    ry = (torch.arange(Hb, device=dev) * block)[None, :, None] + v[..., 0]
    rx = (torch.arange(Wb, device=dev) * block)[None, None, :] + v[..., 1]
    rows = (ry[..., None] + i)[..., :, None].expand(P, Hb, Wb, block, block)
    cols = (rx[..., None] + i)[..., None, :].expand(P, Hb, Wb, block, block)
    pidx = torch.arange(P, device=dev)[:, None, None, None, None].expand_as(rows)
    tiles = lambda t: t[:, :Hb * block, :Wb * block].reshape(P, Hb, block, Wb, block, 3).permute(0, 1, 3, 2, 4, 5)
    a = tiles(cur)
    return ((a - oth[pidx, rows, cols]) ** 2).sum((3, 4, 5)), ((a - tiles(oth)) ** 2).sum((3, 4, 5))


def torch_motion(frames, block, R, top_fraction=0.05):
    mv, sad, sad0 = torch_search(frames, block, R)
    return motion.summarize(mv, sad, sad0, block, top_fraction)


def torch_warp_error(frames, block, R):
    mv, _, _ = torch_search(frames, block, R)
    sse, sse0 = torch_warp(frames, mv, block)
    norm = 3.0 * sse.shape[-2] * sse.shape[-1] * block * block * 255.0 * 255.0
    return sse.flatten(-2).sum(-1).double() / norm, sse0.flatten(-2).sum(-1).double() / norm


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=49)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-reps", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_motion.py measures on the GPU: no device found")
    dev, F, H, W, block = torch.device("cuda", 0), a.frames, 480, 720, 16
    g = torch.Generator(device=dev).manual_seed(1)
    # a picture-like video: smooth content that drifts by a few pixels per frame, plus noise (the kernel's time does not depend on the values)
    base = Fn.interpolate(torch.rand(1, 3, 40, 56, generator=g, device=dev), size=(H + 128, W + 128), mode="bicubic")[0]
    frames = torch.stack([base[:, 64 + (3 * t) % 23:64 + (3 * t) % 23 + H, 64 - (5 * t) % 31:64 - (5 * t) % 31 + W] for t in range(F)])
    frames = ((frames + 0.03 * torch.randn(frames.shape, generator=g, device=dev)).clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    del base
    Hb, Wb, P = H // block, W // block, F - 1
    routes, agree = {}, {}
    for R in (16, 32):
        routes[f"motion_r{R}"] = lambda R=R: M.video_motion(frames, block, R)
        routes[f"motion_r{R}_torch"] = lambda R=R: torch_motion(frames, block, R)
        routes[f"warp_r{R}"] = lambda R=R: M.video_warp_error(frames, None, block, R)
        routes[f"warp_r{R}_torch"] = lambda R=R: torch_warp_error(frames, block, R)
        ours, (mv, sad, sad0) = motion.block_motion(frames, block, R), torch_search(frames, block, R)
        w, (sse, sse0) = motion.warp_sse(frames, ours["mv"]), torch_warp(frames, mv, block)
        agree[f"r{R}"] = {"mv": torch.equal(ours["mv"], mv), "sad": torch.equal(ours["sad"], sad), "sad0": torch.equal(ours["sad0"], sad0),
                          "sse": torch.equal(w["sse"].long(), sse), "sse0": torch.equal(w["sse0"].long(), sse0),
                          "magnitude_mean": M.video_motion(frames, block, R)["magnitude_mean"].item()}
        del ours, mv, sad, sad0, w, sse, sse0
    for k, fn in routes.items():                               # warm-up
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in routes}
    for _ in range(a.rounds):                                  # alternate: drift of the shared machine hits every route alike
        for k, fn in routes.items():
            t[k].append(timed(fn, a.torch_reps if k.endswith("_torch") else a.reps))
    med = {k: statistics.median(v) for k, v in t.items()}
    search_only = {f"r{R}": statistics.median(timed(lambda R=R: motion.block_motion(frames, block, R), a.reps) for _ in range(a.rounds)) for R in (16, 32)}
    # byte absolute differences: implied by the shape (every candidate of every block) and what the kernel's lanes evaluate (4 x 4 candidate groups, rounded up)
    implied = {f"r{R}": P * Hb * Wb * block * block * (2 * R + 1) ** 2 for R in (16, 32)}
    evaluated = {f"r{R}": P * Hb * Wb * block * block * (4 * ((2 * R + 4) // 4)) * (4 * ((((R + 3) // 4) * 4 + R) // 4 + 1)) for R in (16, 32)}
    res = {"device": torch.cuda.get_device_name(0), "frames": F, "shape": [F, H, W, 3], "block": block, "reps": a.reps, "torch_reps": a.torch_reps, "rounds": a.rounds,
           "median_ms": med, "all_rounds_ms": t, "agreement": agree, "search_only_median_ms": search_only,
           "speedup_vs_torch": {k: med[k + "_torch"] / med[k] for k in routes if not k.endswith("_torch")},
           "byte_sads_implied": implied, "byte_sads_evaluated": evaluated,
           "byte_sads_per_s_implied": {k: implied[k] / (search_only[k] * 1e-3) for k in implied},
           "byte_sads_per_s_evaluated": {k: evaluated[k] / (search_only[k] * 1e-3) for k in evaluated}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps({k: v for k, v in res.items() if k != "all_rounds_ms"}))


if __name__ == "__main__":
    main()
