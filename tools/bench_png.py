#!/usr/bin/env python3
"""tokensgen_amd.png.encode_png at a user's size: 49 frames of 480 x 720 x 3 uint8, the smooth-plus-noise clip of tools/bench_jpeg.py and uniform noise (nothing to gain:
every band stored), adaptive filter.  Per clip:

  encode        encode_png end to end at the default rows_per_block (host clock, the call's one wait included)
  filter / band_plan / write    each launch function by device events; `offsets`: the torch prefix sums between the two passes
  to_host       the copy of `data` to the host
  host_route    what a user has without this module: the frames copied to the host and PIL.Image.save(.., "PNG") per frame at Pillow's default level, where Pillow
                imports; otherwise recorded as absent
  by_rows_per_block   for R in 4, 8, 16, 30: encode end to end, the three launches, and the clip's bytes against two references: zlib.compressobj(6,
                strategy=zlib.Z_RLE) over the same filtered bytes plus the same container overhead of one IDAT (the same token model without per-band trees and sync
                blocks), and Pillow's default files

The routes alternate in one process and the median of `rounds` is taken, with min and max; `ranges_overlap` says whether the host route's range meets the range of encode
plus to_host.  There is no pass / fail threshold: the parent commit has no such path.  The figures go to profiles/png_bench.json.

    python tools/bench_png.py [--frames 49] [--out profiles/png_bench.json]"""
import argparse
import io
import json
import os
import statistics
import sys
import time
import zlib

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tokensgen_amd import kernels as K  # noqa: E402
from tokensgen_amd import png  # noqa: E402
from tools.bench_jpeg import device_ms, host_ms, smooth_clip  # noqa: E402

HBM_BYTES_PER_S = 8e12
ROWS = (4, 8, 16, 30)


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=49)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_png.py measures on the GPU: no device found")
    try:
        from PIL import Image
    except ImportError:
        Image = None
    dev, F, H, W = torch.device("cuda", 0), a.frames, 480, 720
    g = torch.Generator(device=dev).manual_seed(1)
    clips = {"smooth": smooth_clip(F, H, W, dev, g), "noise": torch.randint(0, 256, (F, H, W, 3), generator=g, device=dev, dtype=torch.uint8)}
    clip_bytes = F * H * W * 3
    default_rows = png.png_geometry(H, W).rows_per_block
    res = {"device": torch.cuda.get_device_name(0), "shape": [F, H, W, 3], "clip_bytes": clip_bytes, "filter": "adaptive", "default_rows_per_block": default_rows,
           "reps": a.reps, "rounds": a.rounds, "pillow": None if Image is None else __import__("PIL").__version__, "cases": {}}
    for name, frames in clips.items():
        def pil_route():
            host = frames.cpu().numpy()
            n = 0
            for f in host:
                bio = io.BytesIO()
                Image.fromarray(f).save(bio, "PNG")
                n += bio.tell()
            return n

        def parts(R):
            filtered = K.png_filter(frames, "adaptive", R)
            plans, sizes = K.png_band_plan(filtered, H, W, R)
            offs, ends = png.band_offsets(sizes)
            data, offsets = png.encode_png(frames, "adaptive", R)
            assert int(ends[-1]) == data.numel() == int(offsets[-1])
            return filtered, plans, sizes, offs, data

        filtered, plans, sizes, offs, data = parts(default_rows)
        geo = png.png_geometry(H, W, default_rows)
        rows = filtered.reshape(F, geo.bands, -1)[:, :, :geo.band_bytes].reshape(F, -1)[:, :H * geo.row_bytes].cpu().numpy()
        rle_bytes = 0
        for r in rows:                                                          # one zlib stream per frame, in one IDAT: 33 + 12 + 12 bytes around it
            c = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_RLE)
            rle_bytes += len(c.compress(r.tobytes()) + c.flush()) + 57
        routes = {
            "encode": (host_ms, lambda: png.encode_png(frames), a.reps),
            "filter": (device_ms, lambda: K.png_filter(frames, "adaptive", default_rows), a.reps),
            "band_plan": (device_ms, lambda: K.png_band_plan(filtered, H, W, default_rows), a.reps),
            "offsets": (device_ms, lambda: png.band_offsets(sizes), a.reps),
            "write": (device_ms, lambda: K.png_write(filtered, plans, H, W, default_rows, offs, data), a.reps),
            "to_host": (host_ms, lambda: data.cpu(), a.reps),
        }
        per_rows = {}
        for R in ROWS:
            fR, pR, sR, oR, dR = parts(R)
            per_rows[R] = {"bytes": dR.numel()}
            routes[f"encode_R{R}"] = (host_ms, lambda R=R: png.encode_png(frames, "adaptive", R), a.reps)
            routes[f"band_plan_R{R}"] = (device_ms, lambda R=R, fR=fR: K.png_band_plan(fR, H, W, R), a.reps)
            routes[f"write_R{R}"] = (device_ms, lambda R=R, fR=fR, pR=pR, oR=oR, dR=dR: K.png_write(fR, pR, H, W, R, oR, dR), a.reps)
        if Image is not None:
            routes["host_route"] = (host_ms, pil_route, 1)
        for _, fn, _ in routes.values():                   # warm-up
            fn()
        t = {k: [] for k in routes}
        for _ in range(a.rounds):                          # alternate: drift of the shared machine hits every route alike
            for k, (clock, fn, reps) in routes.items():
                t[k].append(clock(fn, reps))
        ms = {k: stats(v) for k, v in t.items()}
        launches = ms["filter"]["median"] + ms["band_plan"]["median"] + ms["write"]["median"]
        floor = (clip_bytes + data.numel()) / HBM_BYTES_PER_S * 1e3
        pil_bytes = pil_route() if Image is not None else None
        for R in ROWS:
            per_rows[R].update(encode_ms=ms[f"encode_R{R}"], band_plan_ms=ms[f"band_plan_R{R}"], write_ms=ms[f"write_R{R}"],
                               bytes_over_zlib_rle=per_rows[R]["bytes"] / rle_bytes, bytes_over_raw=per_rows[R]["bytes"] / clip_bytes,
                               bytes_over_pillow=None if pil_bytes is None else per_rows[R]["bytes"] / pil_bytes)
        case = {"ms": {k: v for k, v in ms.items() if "_R" not in k}, "all_rounds_ms": t, "bytes": data.numel(), "bytes_zlib_rle_level6": rle_bytes,
                "bytes_pillow": pil_bytes, "by_rows_per_block": per_rows, "launches_ms": launches, "memory_floor_ms_at_8TBps": floor,
                "floor_over_launches": floor / launches}
        if Image is not None:
            ours = [e + c for e, c in zip(t["encode"], t["to_host"])]
            case["host_route_over_encode_plus_copy"] = ms["host_route"]["median"] / (ms["encode"]["median"] + ms["to_host"]["median"])
            case["encode_plus_copy_ms"] = stats(ours)
            case["ranges_overlap"] = not (max(ours) < ms["host_route"]["min"] or ms["host_route"]["max"] < min(ours))
        res["cases"][name] = case
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps({k: ({c: {x: y for x, y in v.items() if x != "all_rounds_ms"} for c, v in res["cases"].items()} if k == "cases" else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
