#!/usr/bin/env python3
"""The two kernels of tokensgen_amd.video_io at a user's size, each next to the torch route on the same device, in the same process, alternating:

  prepare_video     49 frames of 1080 x 1920 and of 720 x 1280 -> 480 x 720 with crop_to_fit (one tg_video_resample launch), against
                    `.float() / 255` -> F.interpolate(bicubic, antialias=True) -> crop -> `* 2 - 1` -> `.to(bf16)`
  frames_to_uint8   49 x 480 x 720 decoded bf16 frames [1, 3, 49, 480, 720] -> uint8 [1, 49, 480, 720, 3] (one tg_video_to_uint8 launch), against the bf16 chain
                    `(v * 0.5 + 0.5).clamp(0, 1)` -> `.float() * 255` -> `.to(uint8)` -> permute

Times are device events around `reps` back-to-back calls after a warm-up, the median of `rounds` alternating rounds.  bytes/s is the ALGORITHMIC traffic (the source
window the taps touch, read once, plus the result, written once) over the kernel's time, against 8 TB/s.  There is no pass / fail threshold: the parent commit has no
such path, the torch route is the yardstick, and the figures go to profiles/video_io_bench.json.

    python tools/bench_video_io.py [--frames 49] [--also NAME=other_build.so] [--out profiles/video_io_bench.json]

--also times tg_video_resample of another build of the library in the same alternating rounds and records whether its result is bitwise the shipped one."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as Fn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tokensgen_amd import lib as L  # noqa: E402
from tokensgen_amd import video_io as VIO  # noqa: E402

PEAK_HBM = 8.0e12


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=49)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--also", action="append", default=[], metavar="NAME=LIB", help="time tg_video_resample of another build of the library in the same rounds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "video_io_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_video_io.py measures on the GPU: no device found")
    dev, F, res = torch.device("cuda", 0), a.frames, (480, 720)
    g = torch.Generator(device=dev).manual_seed(1)
    others = {}
    for spec in a.also:
        name, path = spec.split("=", 1)
        other = ctypes.CDLL(os.path.abspath(path))
        other.tg_video_resample.argtypes, other.tg_video_resample.restype = L.PROTOTYPES["tg_video_resample"], ctypes.c_int
        others[name] = other
    routes, agree, meta = {}, {}, {}
    for H, W in ((1080, 1920), (720, 1280)):
        tag = f"resample_{H}x{W}"
        # smooth content plus noise: a picture-like source (the time does not depend on the values)
        base = Fn.interpolate(torch.rand(F, 3, H // 16, W // 16, generator=g, device=dev), size=(H, W), mode="bilinear")
        frames = ((base * 0.8 + 0.2 * torch.rand(F, 3, H, W, generator=g, device=dev)) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        del base
        plan = VIO.resample_plan((H, W), res, crop_to_fit=True)
        tabs = VIO._device_tables(plan, dev)
        y0, ny, wy, x0, nx, wx = plan.tables
        rows = min(H, int(y0[-1] + ny[-1])) - max(0, int(y0[0]))
        cols = min(W, int(x0[-1] + nx[-1])) - max(0, int(x0[0]))
        nbytes = F * rows * cols * 3 + F * 3 * res[0] * res[1] * 2
        meta[tag] = {"in_hw": [H, W], "resized_hw": list(plan.resized_hw), "top_left": [plan.top, plan.left], "taps": list(plan.taps), "algorithmic_bytes": nbytes}

        def ours(frames=frames):
            return VIO.prepare_video(frames, res, crop_to_fit=True)

        def torch_route(frames=frames, plan=plan):
            x = frames.permute(0, 3, 1, 2).float() / 255
            x = Fn.interpolate(x, size=plan.resized_hw, mode="bicubic", align_corners=False, antialias=True)
            x = x[:, :, plan.top:plan.top + res[0], plan.left:plan.left + res[1]]
            return (x * 2 - 1).to(torch.bfloat16)[None]
        got, want = ours(), torch_route()
        torch.cuda.synchronize()
        diff = (got.float() - want.float()).abs()
        agree[tag] = {"max_abs_vs_torch": diff.max().item(), "elements_differing": (diff > 0).float().mean().item()}
        routes[tag] = (ours, nbytes)
        routes[tag + "_torch"] = (torch_route, None)
        for name, other in others.items():
            out = torch.empty_like(got[0])
            stream = torch.cuda.current_stream().cuda_stream

            def run(other=other, frames=frames, tabs=tabs, out=out, H=H, W=W):
                assert other.tg_video_resample(frames.data_ptr(), F, H, W, out.data_ptr(), res[0], res[1], tabs[0].data_ptr(), tabs[1].data_ptr(), tabs[2].data_ptr(),
                                               tabs[2].shape[1], tabs[3].data_ptr(), tabs[4].data_ptr(), tabs[5].data_ptr(), tabs[5].shape[1], stream) == 0
            run()
            torch.cuda.synchronize()
            agree[f"{tag}_{name}_bitwise_equal"] = bool(torch.equal(out, got[0]))
            routes[f"{tag}_{name}"] = (run, nbytes)
        del got, want, diff
    video = (torch.randn(1, 3, F, res[0], res[1], generator=g, device=dev) * 0.6).to(torch.bfloat16)

    def ours_u8():
        return VIO.frames_to_uint8(video, "bcthw", 0)

    def torch_u8():
        r = (video * 0.5 + 0.5).clamp(0, 1)
        return (r.float() * 255).to(torch.uint8).permute(0, 2, 3, 4, 1).contiguous()
    agree["to_uint8_equal_torch"] = bool(torch.equal(ours_u8(), torch_u8()))
    nb = video.numel() * 2 + video.numel()
    meta["to_uint8"] = {"shape": list(video.shape), "algorithmic_bytes": nb}
    routes["to_uint8"] = (ours_u8, nb)
    routes["to_uint8_torch"] = (torch_u8, None)

    for fn, _ in routes.values():
        timed(fn, 2)
    t = {k: [] for k in routes}
    for _ in range(a.rounds):                                 # alternate: drift of the shared machine hits every route alike
        for k, (fn, _) in routes.items():
            t[k].append(timed(fn, a.reps if not k.endswith("_torch") else max(1, a.reps // 2)))
    med = {k: statistics.median(v) for k, v in t.items()}
    res_json = {"device": torch.cuda.get_device_name(0), "frames": F, "output_res": list(res), "reps": a.reps, "rounds": a.rounds, "median_ms": med, "all_rounds_ms": t,
                "shapes": meta, "agreement": agree, "peak_hbm_bytes_per_s": PEAK_HBM,
                "speedup_vs_torch": {k: med[k + "_torch"] / med[k] for k in routes if k + "_torch" in routes},
                "algorithmic_bytes_per_s": {k: nbytes / (med[k] * 1e-3) for k, (_, nbytes) in routes.items() if nbytes},
                "fraction_of_8TBps": {k: nbytes / (med[k] * 1e-3) / PEAK_HBM for k, (_, nbytes) in routes.items() if nbytes}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res_json, f, indent=1, sort_keys=True)
    print(json.dumps({k: v for k, v in res_json.items() if k != "all_rounds_ms"}))


if __name__ == "__main__":
    main()
