#!/usr/bin/env python3
"""tokensgen_amd.jpeg.decode_jpeg at a user's size: 49 frames of 480 x 720, a smooth-plus-noise clip and uniform noise (the worst case for size), encoded by encode_jpeg
at quality 90, both subsamplings, restart interval 1, 45 (one MCU row at 4:2:0) and none (65535: one lane per frame, what Pillow and most cameras write).  Per case:

  decode        decode_jpeg of the list of `bytes` end to end (host clock: header parsing, the one copy up, the launches and the one wait)
  find_segments / decode_coeffs / idct_rgb    each launch function by device events around back-to-back calls
  load_video    video_io.load_video of the same frames as a .avi file in the page cache: index, file reads, decode, prepare_video to 480 x 720
  host_route    what a user has without this module: PIL.Image.open per frame -> numpy -> one upload, where Pillow imports; otherwise recorded as absent

The routes alternate and the median of `rounds` is taken; the marker-less decode and the host route run once per round.  There is no pass / fail threshold: the parent
commit has no such path.  Beside the times stands the memory floor at 8 TB/s: the stream read once plus the frames written once.  The decoded frames are compared
with the host route's (a few levels apart, as tests/test_jpeg_decode_cpu.py holds) before anything is timed.  The figures go to profiles/jpeg_decode_bench.json.

    python tools/bench_jpeg_decode.py [--frames 49] [--out profiles/jpeg_decode_bench.json]

These routes pin entropy="segment", the launch sequence the figures above were taken with.  `--sync` measures the parallel entropy decoder of DESIGN.md §8m instead
(see sync_main) and writes profiles/jpeg_sync_bench.json."""
import argparse
import io
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_jpeg import HBM_BYTES_PER_S, QUALITY, device_ms, host_ms, smooth_clip  # noqa: E402
from tokensgen_amd import jpeg, video_io  # noqa: E402
from tokensgen_amd import kernels as K  # noqa: E402


def launch_inputs(streams, dev):
    """what decode_jpeg hands the three launch functions, built once so that each can be timed alone"""
    infos = [jpeg.parse_jpeg(s, i) for i, s in enumerate(streams)]
    H, W, sub, ri = infos[0][:4]
    off = np.cumsum([0] + [len(s) for s in streams])
    data = torch.from_numpy(np.frombuffer(b"".join(streams), np.uint8).copy()).to(dev)
    up = lambda a: torch.from_numpy(a).to(dev)
    scan_begin = up(np.array([o + i.scan[0] for o, i in zip(off, infos)], np.int64))
    scan_end = up(np.array([o + i.scan[1] for o, i in zip(off, infos)], np.int64))
    htabs = up(np.frombuffer(jpeg._huffman_set(infos[0].huffman), np.uint8).copy().reshape(1, -1))
    qtabs = up(np.array([infos[0].qtables], np.uint16))
    zero = torch.zeros(len(streams), dtype=torch.int32, device=dev)
    return dict(H=H, W=W, sub=sub, ri=ri, n_seg=K.jpeg_decode_segments(H, W, sub, ri), data=data, scan_begin=scan_begin, scan_end=scan_end, htabs=htabs, qtabs=qtabs,
                index=zero, status=torch.zeros_like(zero))


SYNC_SUB_BYTES = (64, 128, 256)
SYNC_INTERVALS = (1, 2, 4, 8, 16, 32, 45, 90, 270, 65535)


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def sync_main(a):
    """`--sync`: decode_jpeg(entropy="sync") against entropy="segment" and against the Pillow host route on the four clips of the record, without restart markers and
    at interval 45, in one process, alternating, median of `rounds` with min - max.  Beside them the launches alone by device events: tg_jpeg_decode_coeffs_sync at
    sub_bytes 64, 128 and 256 with its `rounds`, tg_jpeg_decode_coeffs; and both launches over restart intervals from 1 to none, which gives the fewest MCUs per segment
    from which the parallel launch is the faster one on every clip.  jpeg.SYNC_MIN_MCUS and jpeg.SYNC_SUB_BYTES are set from this file.  The two decodes are compared
    bit for bit before anything is timed."""
    try:
        from PIL import Image
    except ImportError:
        Image = None
    dev, F, H, W = torch.device("cuda", 0), a.frames, 480, 720
    g = torch.Generator(device=dev).manual_seed(1)
    clips = {"smooth": smooth_clip(F, H, W, dev, g), "noise": torch.randint(0, 256, (F, H, W, 3), generator=g, device=dev, dtype=torch.uint8)}
    res = {"device": torch.cuda.get_device_name(0), "shape": [F, H, W, 3], "quality": QUALITY, "rounds": a.rounds, "pillow": None if Image is None else __import__("PIL").__version__,
           "sync_min_mcus_in_use": jpeg.SYNC_MIN_MCUS, "sync_sub_bytes_in_use": jpeg.SYNC_SUB_BYTES, "cases": {}, "intervals": {}}

    def launches(streams):
        x = launch_inputs(streams, dev)
        seg_begin, seg_end = K.jpeg_find_segments(x["data"], x["scan_begin"], x["scan_end"], x["n_seg"], x["status"])
        flags = torch.zeros(2 * len(streams), dtype=torch.int32, device=dev)
        clean, rounds = flags[:len(streams)], flags[len(streams):]
        serial = lambda: K.jpeg_decode_coeffs(x["data"], seg_begin, seg_end, H, W, x["sub"], x["ri"], x["htabs"], x["index"], x["status"])
        sync = lambda sb: K.jpeg_decode_coeffs_sync(x["data"], seg_begin, seg_end, H, W, x["sub"], x["ri"], x["htabs"], x["index"], sb, clean, rounds)
        return x, serial, sync, clean, rounds

    for name, frames in clips.items():
        for sub in ("420", "444"):
            for ri in (65535, 45):
                streams = jpeg.jpeg_bytes(frames, QUALITY, sub, ri)
                x, serial, sync, clean, rounds = launches(streams)
                want = jpeg.decode_jpeg(streams, entropy="segment")
                assert torch.equal(jpeg.decode_jpeg(streams, entropy="sync"), want)
                ref, seen = serial(), {}
                for sb in SYNC_SUB_BYTES:
                    assert torch.equal(sync(sb), ref) and clean.tolist() == [1] * F
                    seen[sb] = {"most": int(rounds.max()), "mean": float(rounds.float().mean())}

                def pil_route():
                    host = np.stack([np.asarray(Image.open(io.BytesIO(s)).convert("RGB")) for s in streams])
                    return torch.from_numpy(host).to(dev)

                routes = {"decode_sync": (host_ms, lambda: jpeg.decode_jpeg(streams, entropy="sync")), "decode_segment": (host_ms, lambda: jpeg.decode_jpeg(streams, entropy="segment")),
                          "launch_segment": (device_ms, serial)}
                for sb in SYNC_SUB_BYTES:
                    routes[f"launch_sync_{sb}"] = (device_ms, lambda sb=sb: sync(sb))
                if Image is not None:
                    routes["host_route"] = (host_ms, pil_route)
                for _, fn in routes.values():
                    fn()
                t = {k: [] for k in routes}
                for _ in range(a.rounds):
                    for k, (clock, fn) in routes.items():
                        t[k].append(clock(fn, 1))
                case = {"ms": {k: spread(v) for k, v in t.items()}, "all_rounds_ms": t, "stream_bytes": sum(map(len, streams)), "segments_per_frame": x["n_seg"],
                        "sync_rounds": seen}
                if Image is not None:
                    case["sync_faster_than_host_route_ranges_apart"] = max(t["decode_sync"]) < min(t["host_route"])
                case["sync_faster_than_segment_ranges_apart"] = max(t["decode_sync"]) < min(t["decode_segment"])
                res["cases"][f"{name}_{sub}_ri{ri}"] = case
            # the two entropy launches over the restart interval: MCUs per segment from 1 to the whole frame (1350 at 4:2:0, 5400 at 4:4:4)
            sweep = {}
            for ri in SYNC_INTERVALS:
                x, serial, sync, clean, rounds = launches(jpeg.jpeg_bytes(frames, QUALITY, sub, ri))
                reps = 1 if ri > 90 else 5
                serial(), sync(jpeg.SYNC_SUB_BYTES)
                assert clean.tolist() == [1] * F
                ts, ty = [], []
                for _ in range(a.rounds):
                    ts.append(device_ms(serial, reps))
                    ty.append(device_ms(lambda: sync(jpeg.SYNC_SUB_BYTES), reps))
                sweep[str(ri)] = {"segment_ms": spread(ts), "sync_ms": spread(ty), "sync_wins_ranges_apart": max(ty) < min(ts)}
            res["intervals"][f"{name}_{sub}"] = sweep
    wins = [min((ri for ri in SYNC_INTERVALS if all(v[str(r)]["sync_wins_ranges_apart"] for r in SYNC_INTERVALS if r >= ri)), default=None) for v in res["intervals"].values()]
    res["fewest_mcus_per_segment_where_sync_wins_on_every_clip"] = None if None in wins else max(wins)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    brief = {c: {"ms": v["ms"], "sync_rounds": v["sync_rounds"], "stream_bytes": v["stream_bytes"]} for c, v in res["cases"].items()}
    print(json.dumps({"cases": brief, "intervals": res["intervals"], "fewest_mcus_per_segment_where_sync_wins_on_every_clip": res["fewest_mcus_per_segment_where_sync_wins_on_every_clip"]}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=49)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sync", action="store_true", help="measure the parallel entropy decoder (DESIGN.md §8m) and write profiles/jpeg_sync_bench.json")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "jpeg_sync_bench.json" if a.sync else "jpeg_decode_bench.json")
    if a.sync:
        if not torch.cuda.is_available():
            raise SystemExit("bench_jpeg_decode.py measures on the GPU: no device found")
        return sync_main(a)
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg_decode.py measures on the GPU: no device found")
    try:
        from PIL import Image
    except ImportError:
        Image = None
    dev, F, H, W = torch.device("cuda", 0), a.frames, 480, 720
    g = torch.Generator(device=dev).manual_seed(1)
    clips = {"smooth": smooth_clip(F, H, W, dev, g), "noise": torch.randint(0, 256, (F, H, W, 3), generator=g, device=dev, dtype=torch.uint8)}
    frame_bytes = F * H * W * 3
    res = {"device": torch.cuda.get_device_name(0), "shape": [F, H, W, 3], "frame_bytes": frame_bytes, "quality": QUALITY, "reps": a.reps, "rounds": a.rounds,
           "pillow": None if Image is None else __import__("PIL").__version__, "cases": {}}
    tmp = tempfile.mkdtemp(prefix="bench_jpeg_decode_")
    for name, frames in clips.items():
        for sub in ("420", "444"):
            for ri in (1, 45, 65535):
                slow = ri == 65535                                             # one lane per frame: once per round
                reps = 1 if slow else a.reps
                streams = jpeg.jpeg_bytes(frames, QUALITY, sub, ri)
                n_stream = sum(map(len, streams))
                x = launch_inputs(streams, dev)
                seg_begin, seg_end = K.jpeg_find_segments(x["data"], x["scan_begin"], x["scan_end"], x["n_seg"], x["status"])
                coef = K.jpeg_decode_coeffs(x["data"], seg_begin, seg_end, H, W, sub, x["ri"], x["htabs"], x["index"], x["status"])
                out = jpeg.decode_jpeg(streams, entropy="segment")
                assert int(x["status"].abs().sum()) == 0 and torch.equal(K.jpeg_idct_rgb(coef, H, W, sub, x["qtabs"], x["index"]), out)
                path = os.path.join(tmp, f"{name}_{sub}_{ri}.avi")
                with jpeg.MJPEGWriter(path, 8) as w:
                    w.write_jpegs(streams, H, W)
                with open(path, "rb") as fh:                                   # into the page cache
                    fh.read()
                loaded = video_io.load_video(path, (H, W), F, False, -1, 0, -1, 1)
                assert loaded.shape == (1, F, 3, H, W)

                def pil_route():
                    host = np.stack([np.asarray(Image.open(io.BytesIO(s)).convert("RGB")) for s in streams])
                    return torch.from_numpy(host).to(dev)

                routes = {
                    "decode": (host_ms, lambda: jpeg.decode_jpeg(streams, entropy="segment"), reps),
                    "find_segments": (device_ms, lambda: K.jpeg_find_segments(x["data"], x["scan_begin"], x["scan_end"], x["n_seg"], x["status"]), a.reps),
                    "decode_coeffs": (device_ms, lambda: K.jpeg_decode_coeffs(x["data"], seg_begin, seg_end, H, W, sub, x["ri"], x["htabs"], x["index"], x["status"]), reps),
                    "idct_rgb": (device_ms, lambda: K.jpeg_idct_rgb(coef, H, W, sub, x["qtabs"], x["index"]), a.reps),
                    "load_video": (host_ms, lambda: video_io.load_video(path, (H, W), F, False, -1, 0, -1, 1), reps),
                }
                worst = None
                if Image is not None:
                    routes["host_route"] = (host_ms, pil_route, 1)
                    worst = int((pil_route().int() - out.int()).abs().max())
                for _, fn, _ in routes.values():                               # warm-up
                    fn()
                t = {k: [] for k in routes}
                for _ in range(a.rounds):                                      # alternate: drift of the shared machine hits every route alike
                    for k, (clock, fn, n) in routes.items():
                        t[k].append(clock(fn, n))
                med = {k: statistics.median(v) for k, v in t.items()}
                floor = (n_stream + frame_bytes) / HBM_BYTES_PER_S * 1e3
                launches = med["find_segments"] + med["decode_coeffs"] + med["idct_rgb"]
                case = {"median_ms": med, "all_rounds_ms": t, "per_frame_ms": {k: v / F for k, v in med.items()}, "stream_bytes": n_stream, "segments_per_frame": x["n_seg"],
                        "memory_floor_ms_at_8TBps": floor, "launches_ms": launches, "floor_over_launches": floor / launches,
                        "entropy_share_of_launches": med["decode_coeffs"] / launches, "host_side_ms": med["decode"] - launches,
                        "worst_level_difference_to_pillow": worst}
                if Image is not None:
                    case["host_route_over_decode"] = med["host_route"] / med["decode"]
                res["cases"][f"{name}_{sub}_ri{ri}"] = case
                os.remove(path)
    os.rmdir(tmp)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps({k: ({c: {x: y for x, y in v.items() if x != "all_rounds_ms"} for c, v in res["cases"].items()} if k == "cases" else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
