#!/usr/bin/env python3
"""tokensgen_amd.lpips.video_lpips at a user's size next to the torch route on the same device, in the same process, alternating:

  video_lpips       49 frames of 480 x 720 x 3 as uint8 [49, 480, 720, 3], two clips: per chunk of 8 frames per clip tg_lpips_conv_in x 2, 12 tg_conv3d_cl (bf16, fp32
                    accumulation), 4 tg_relu_maxpool2_cl, 7 tg_relu_cl, 5 tg_lpips_head
  torch route       the fp32 restatement of tests/lpips_ref.py (F.conv2d, F.relu, F.max_pool2d, the head) on the GPU, in chunks of --torch-chunk frames per clip so
                    that its activations fit: what `lpips.LPIPS(net='vgg')` runs, restated (that package and torchvision are absent)

Needs `tests/lpips_ref.py` beside it (the restatement is the torch route; `tests/` is put on the import path).  Random weights (the time does not depend on the values).
The two routes run with different chunk sizes (8 and --torch-chunk = 4 frames per clip): the peak-memory ratio is that of these two choices.  Times are device events around `reps` back-to-back calls after a warm-up, the median of `rounds` alternating
rounds; peak memory is torch's allocator peak over one call of the route, above what the inputs and the weights hold.  There is no pass / fail threshold: the parent
commit has no such path and the torch route is the yardstick.  With --profile the per-kernel split of one video_lpips call (device events per launch) is added.  The
figures go to profiles/lpips_bench.json.

    python tools/bench_lpips.py [--frames 49] [--out profiles/lpips_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as Fn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lpips_ref as LR  # noqa: E402
from tokensgen_amd import kernels as K  # noqa: E402
from tokensgen_amd.lpips import LPIPS, video_lpips  # noqa: E402

LR.DETERMINISTIC = False                      # the yardstick runs as a user's torch does: the library's own choice of convolution algorithm

# multiply-adds of VGG16 up to relu5_3 per pixel of the input: conv1_1, then each stage's convolutions at its resolution
MACS_PER_PIXEL = 27 * 64 + sum(9 * ci * co / 4 ** (stage - 1) for _, ci, co, stage in LR.CONVS[1:])


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


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
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--torch-reps", type=int, default=1)
    ap.add_argument("--torch-chunk", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lpips.py measures on the GPU: no device found")
    dev, F, H, W = torch.device("cuda", 0), a.frames, 480, 720
    g = torch.Generator(device=dev).manual_seed(1)
    base = Fn.interpolate(torch.rand(F, 3, H // 16, W // 16, generator=g, device=dev), size=(H, W), mode="bilinear")
    va = (base * 0.8 + 0.2 * torch.rand(F, 3, H, W, generator=g, device=dev)).clamp(0, 1)
    vb = (va + 0.05 * torch.randn(F, 3, H, W, generator=g, device=dev)).clamp(0, 1)
    u8a, u8b = ((t * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous() for t in (va, vb))
    del base, va, vb
    weights = LR.random_weights(0)
    wdev = {k: v.to(dev) for k, v in weights.items()}
    model = LPIPS(dev)
    model.load_state_dict(LR.as_state_dict(weights))

    def torch_route():
        out = []
        for i in range(0, F, a.torch_chunk):
            fa, fb = (2 * (t[i:i + a.torch_chunk].permute(0, 3, 1, 2).float() / 255) - 1 for t in (u8a, u8b))
            out.append(LR.lpips_ref(fa, fb, wdev, torch.float32).view(-1))
        return torch.cat(out)

    routes = {"uint8": lambda: video_lpips(u8a, u8b, model)["lpips"], "uint8_torch": torch_route}
    ours, ref = routes["uint8"]().double(), routes["uint8_torch"]().double()
    agree = {"lpips_pooled": ours.mean().item(), "lpips_pooled_torch": ref.mean().item(), "max_rel_gap_per_frame": ((ours - ref).abs() / ref).max().item()}
    peak = {k: peak_bytes(fn) for k, fn in routes.items()}
    t = {k: [] for k in routes}
    for _ in range(a.rounds):                                  # alternate: drift of the shared machine hits every route alike
        for k, fn in routes.items():
            t[k].append(timed(fn, a.torch_reps if k.endswith("_torch") else a.reps))
    med = {k: statistics.median(v) for k, v in t.items()}
    flop = 2.0 * MACS_PER_PIXEL * H * W * 2 * F
    res = {"device": torch.cuda.get_device_name(0), "frames": F, "shape": [F, H, W, 3], "frames_per_launch": model.frames_per_launch, "torch_chunk": a.torch_chunk,
           "reps": a.reps, "torch_reps": a.torch_reps, "rounds": a.rounds, "median_ms": med, "all_rounds_ms": t, "peak_bytes_above_inputs": peak, "agreement": agree,
           "flop_per_pair_of_clips": flop, "gflop_per_image": 2.0 * MACS_PER_PIXEL * H * W / 1e9,
           "effective_tflops": {k: flop / (med[k] * 1e-3) / 1e12 for k in med}, "speedup_vs_torch": med["uint8_torch"] / med["uint8"],
           "peak_memory_ratio_torch_over_ours": peak["uint8_torch"] / max(peak["uint8"], 1)}
    if a.profile:
        K.PROFILE.clear()
        K.PROFILE_ON[0] = True
        routes["uint8"]()
        K.PROFILE_ON[0] = False
        res["per_kernel_ms_one_call"] = {k: {"total_ms": v["total_ms"], "launches": v["n"]} for k, v in sorted(K.profile_summary().items(), key=lambda kv: -kv[1]["total_ms"])}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps({k: v for k, v in res.items() if k != "all_rounds_ms"}))


if __name__ == "__main__":
    main()
