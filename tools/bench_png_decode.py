#!/usr/bin/env python3
"""tokensgen_amd.png.decode_png at a user's size: 49 frames of 480 x 720 x 3 uint8, the smooth-plus-noise clip and the uniform noise of tools/bench_png.py.  Per clip
three kinds of file:

  own_chunk     encode_png's files by the chunk route (inflate="auto" takes it: every band an independent piece)
  own_stream    the same files forced to inflate="stream": one wave per frame
  pillow_stream Pillow's default files (one zlib stream cut anywhere): the stream route, the only one they have

Each variant alternates in the same process with the route a user has without this module, `host_route`: PIL.Image.open per frame -> numpy -> one upload.  Per
variant: decode_png end to end from `bytes` on the host to frames on the device (host clock, the call's one wait included), every launch by device events
(kernels.PROFILE), and the host's share measured apart: `parse` (parse_png of every file: the chunk walk and the CRC-32s), and `host_total`, the end-to-end time less
the launches.  The median of `rounds` with min and max; `ranges_apart_from_host_route` says whether the variant's range and the host route's do not meet, and
`faster_than_host_route` which way.  There is no pass / fail threshold: the parent commit has no such path.  The figures go to profiles/png_decode_bench.json.

    python tools/bench_png_decode.py [--frames 49] [--out profiles/png_decode_bench.json]"""
import argparse
import io
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tokensgen_amd import kernels as K  # noqa: E402
from tokensgen_amd import png  # noqa: E402
from tools.bench_jpeg import host_ms, smooth_clip  # noqa: E402


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def launches_ms(fn):
    """every launch of one call of fn by device events: {name: [ms, ...] in launch order}"""
    K.PROFILE.clear()
    K.PROFILE_ON[0] = True
    try:
        fn()
        torch.cuda.synchronize()
        return {name: [s.elapsed_time(e) for s, e in ev] for name, ev in K.PROFILE.items()}
    finally:
        K.PROFILE_ON[0] = False
        K.PROFILE.clear()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=49)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_decode_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_png_decode.py measures on the GPU: no device found")
    from PIL import Image
    dev, F, H, W = torch.device("cuda", 0), a.frames, 480, 720
    g = torch.Generator(device=dev).manual_seed(1)
    clips = {"smooth": smooth_clip(F, H, W, dev, g), "noise": torch.randint(0, 256, (F, H, W, 3), generator=g, device=dev, dtype=torch.uint8)}
    res = {"device": torch.cuda.get_device_name(0), "shape": [F, H, W, 3], "clip_bytes": F * H * W * 3, "reps": a.reps, "rounds": a.rounds,
           "pillow": __import__("PIL").__version__, "cases": {}}
    for name, frames in clips.items():
        own = png.png_bytes(frames)
        pil = []
        for f in frames.cpu().numpy():
            bio = io.BytesIO()
            Image.fromarray(f).save(bio, "PNG")
            pil.append(bio.getvalue())
        variants = {"own_chunk": (own, "auto"), "own_stream": (own, "stream"), "pillow_stream": (pil, "auto")}
        assert png.inflate_plan(own)[0] == "chunk" and png.inflate_plan(pil)[0] == "stream"

        def host_route(files):
            return torch.from_numpy(np.stack([np.asarray(Image.open(io.BytesIO(b)).convert("RGB")) for b in files])).to(dev)

        routes = {}
        for v, (files, mode) in variants.items():
            assert torch.equal(png.decode_png(files, device=dev, inflate=mode), frames) and torch.equal(host_route(files), frames)
            routes[v] = (lambda files=files, mode=mode: png.decode_png(files, device=dev, inflate=mode))
            routes[v + "/parse"] = (lambda files=files: [png.parse_png(c, i) for i, c in enumerate(files)])
            routes[v + "/host_route"] = (lambda files=files: host_route(files))
        t = {k: [] for k in routes}
        per_launch = {v: [] for v in variants}
        for _ in range(a.rounds):                          # alternate: drift of the shared machine hits every route alike
            for k, fn in routes.items():
                t[k].append(host_ms(fn, a.reps))
            for v in variants:
                per_launch[v].append(launches_ms(routes[v]))
        case = {}
        for v, (files, mode) in variants.items():
            names = list(per_launch[v][0])
            launch = {n: [stats([r[n][k] for r in per_launch[v]]) for k in range(len(per_launch[v][0][n]))] for n in names}
            launch_total = [sum(sum(x) for x in r.values()) for r in per_launch[v]]
            ours, theirs = t[v], t[v + "/host_route"]
            case[v] = {"file_bytes": sum(map(len, files)), "route": png.inflate_plan(files)[0] if mode == "auto" else mode, "decode_ms": stats(ours),
                       "launch_ms": launch, "launches_total_ms": stats(launch_total), "parse_ms": stats(t[v + "/parse"]),
                       "host_total_ms": stats([o - l for o, l in zip(ours, launch_total)]), "host_route_ms": stats(theirs),
                       "ranges_apart_from_host_route": max(ours) < min(theirs) or max(theirs) < min(ours),
                       "faster_than_host_route": statistics.median(ours) < statistics.median(theirs),
                       "host_route_over_decode": statistics.median(theirs) / statistics.median(ours), "all_rounds_ms": {"decode": ours, "host_route": theirs}}
        res["cases"][name] = case
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps({c: {v: {k: x for k, x in r.items() if k not in ("all_rounds_ms", "launch_ms")} for v, r in case.items()} for c, case in res["cases"].items()}))


if __name__ == "__main__":
    main()
