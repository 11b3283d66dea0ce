#!/usr/bin/env python3
"""tokensgen_amd.jpeg.encode_jpeg at a user's size: 49 frames of 480 x 720 x 3 uint8, a smooth-plus-noise clip and uniform noise (the worst case for size), quality 90,
both subsamplings, restart interval 1.  Per clip and subsampling:

  encode        encode_jpeg end to end (host clock, the call's one wait included)
  coeffs / segment_bytes / write    each launch function by device events; `offsets`: the torch prefix sums between the two passes
  to_host       the copy of `data` to the host
  host_route    what a user has without this module: the frames copied to the host and PIL.Image.save(.., "JPEG") per frame at the same quality and subsampling,
                where Pillow imports; otherwise recorded as absent
  bytes         the stream's size, Pillow's, and the size with restart interval 65535 (no markers) for the cost of restart interval 1

The routes alternate and the median of `rounds` is taken.  There is no pass / fail threshold: the parent commit has no such path.  Beside the times stands the memory
floor at 8 TB/s: one read of the clip plus one write of the stream.  The figures go to profiles/jpeg_bench.json.

    python tools/bench_jpeg.py [--frames 49] [--out profiles/jpeg_bench.json]"""
import argparse
import io
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tokensgen_amd import jpeg  # noqa: E402
from tokensgen_amd import kernels as K  # noqa: E402

HBM_BYTES_PER_S = 8e12
QUALITY = 90


def device_ms(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def host_ms(fn, reps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / reps


def smooth_clip(F, H, W, dev, g):
    t = torch.arange(F, device=dev, dtype=torch.float32)[:, None, None]
    yy = torch.arange(H, device=dev, dtype=torch.float32)[None, :, None]
    xx = torch.arange(W, device=dev, dtype=torch.float32)[None, None, :]
    a = torch.stack([127 + 100 * torch.sin(xx / 7.0 + yy / 13.0 + t / 5.0), 127 + 100 * torch.cos(xx / 11.0 - yy / 5.0 + t / 9.0), (xx * 3 + yy * 2 + t * 4) % 256], -1)
    return (a + 6 * torch.randn(a.shape, generator=g, device=dev)).clamp(0, 255).to(torch.uint8)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=49)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg.py measures on the GPU: no device found")
    try:
        from PIL import Image
    except ImportError:
        Image = None
    dev, F, H, W = torch.device("cuda", 0), a.frames, 480, 720
    g = torch.Generator(device=dev).manual_seed(1)
    clips = {"smooth": smooth_clip(F, H, W, dev, g), "noise": torch.randint(0, 256, (F, H, W, 3), generator=g, device=dev, dtype=torch.uint8)}
    header = K.L.load().tg_jpeg_header_bytes()
    clip_bytes = F * H * W * 3
    res = {"device": torch.cuda.get_device_name(0), "shape": [F, H, W, 3], "clip_bytes": clip_bytes, "quality": QUALITY, "restart_interval": 1, "reps": a.reps,
           "rounds": a.rounds, "pillow": None if Image is None else __import__("PIL").__version__, "cases": {}}
    for name, frames in clips.items():
        for sub in ("420", "444"):
            coef = K.jpeg_coeffs(frames, QUALITY, sub)
            seg = K.jpeg_segment_bytes(coef, H, W, sub, 1)
            seg_off, frame_off, frame_ends = jpeg.stream_offsets(seg, header)
            data, offsets = jpeg.encode_jpeg(frames, QUALITY, sub, 1)
            assert int(frame_ends[-1]) == data.numel() == int(offsets[-1])
            whole, _ = jpeg.encode_jpeg(frames, QUALITY, sub, 65535)

            def pil_route():
                host = frames.cpu().numpy()
                n = 0
                for f in host:
                    bio = io.BytesIO()
                    Image.fromarray(f).save(bio, "JPEG", quality=QUALITY, subsampling={"420": 2, "444": 0}[sub])
                    n += bio.tell()
                return n

            routes = {
                "encode": (host_ms, lambda: jpeg.encode_jpeg(frames, QUALITY, sub, 1), a.reps),
                "coeffs": (device_ms, lambda: K.jpeg_coeffs(frames, QUALITY, sub), a.reps),
                "segment_bytes": (device_ms, lambda: K.jpeg_segment_bytes(coef, H, W, sub, 1), a.reps),
                "offsets": (device_ms, lambda: jpeg.stream_offsets(seg, header), a.reps),
                "write": (device_ms, lambda: K.jpeg_write(coef, H, W, QUALITY, sub, 1, seg_off, frame_off, data), a.reps),
                "to_host": (host_ms, lambda: data.cpu(), a.reps),
                "encode_no_markers": (host_ms, lambda: jpeg.encode_jpeg(frames, QUALITY, sub, 65535), 1),
            }
            if Image is not None:
                routes["host_route"] = (host_ms, pil_route, 1)
            for _, fn, _ in routes.values():                   # warm-up
                fn()
            t = {k: [] for k in routes}
            for _ in range(a.rounds):                          # alternate: drift of the shared machine hits every route alike
                for k, (clock, fn, reps) in routes.items():
                    t[k].append(clock(fn, reps))
            med = {k: statistics.median(v) for k, v in t.items()}
            floor = (clip_bytes + data.numel()) / HBM_BYTES_PER_S * 1e3
            launches = med["coeffs"] + med["segment_bytes"] + med["write"]
            case = {"median_ms": med, "all_rounds_ms": t, "per_frame_ms": {k: v / F for k, v in med.items()}, "bytes": data.numel(), "bytes_no_markers": whole.numel(),
                    "restart_1_size_cost": data.numel() / whole.numel() - 1.0, "bytes_pillow": pil_route() if Image is not None else None,
                    "memory_floor_ms_at_8TBps": floor, "launches_ms": launches, "floor_over_launches": floor / launches,
                    "entropy_share_of_launches": (med["segment_bytes"] + med["write"]) / launches}
            if Image is not None:
                case["size_vs_pillow"] = data.numel() / case["bytes_pillow"]
                case["host_route_over_encode_plus_copy"] = med["host_route"] / (med["encode"] + med["to_host"])
            res["cases"][f"{name}_{sub}"] = case
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps({k: ({c: {x: y for x, y in v.items() if x != "all_rounds_ms"} for c, v in res["cases"].items()} if k == "cases" else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
