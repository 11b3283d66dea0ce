#!/usr/bin/env python3
"""Fit pca.pt / mean.pt / std.pt for the T2To stage from a directory of per-video condensed-token files, in two streaming passes on the GPU
(tokensgen_amd/token_stats.py).  Every `*.pt` file under DIR holds one video's tokens, bf16 [F, C, h, w] (F = chunks x temporal queries), as the Resampler
of the To2V stage produced them; all of a file's frames count.

    python tools/fit_token_stats.py DIR --out OUT [--components 16]

OUT then holds the three files `train_t2to` / `pipeline_t2to` (and the reference's train_cogvideo_t2to.py / pipeline_cogvideox_t2to.py) load."""
import argparse
import glob
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def videos(directory, device):
    for path in sorted(glob.glob(os.path.join(directory, "**", "*.pt"), recursive=True)):
        tok = torch.load(path, map_location="cpu", weights_only=True)
        if tok.dim() != 4:
            raise SystemExit(f"{path}: expected [F, C, h, w], got {tuple(tok.shape)}")
        yield tok.to(device, torch.bfloat16)[None]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("dir", metavar="DIR", help="directory of per-video token files (*.pt, bf16 [F, C, h, w])")
    ap.add_argument("--out", required=True, help="directory that receives pca.pt, mean.pt and std.pt")
    ap.add_argument("--components", type=int, default=16, help="PCA components kept (the T2To model samples 16; at most 64)")
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args()
    from tokensgen_amd.token_stats import TokenStats
    stats = None
    for tok in videos(a.dir, a.device):
        stats = stats or TokenStats(tok.shape[2], a.device)
        stats.update(tok)
    if stats is None:
        raise SystemExit(f"no *.pt files under {a.dir}")
    coef = stats.fit(a.components)
    for tok in videos(a.dir, a.device):
        coef.update(tok)
    coef.finalize().save(a.out)
    print(f"{stats.n} token rows x {stats.dim} -> {a.out}/pca.pt ({coef.d} components), mean.pt, std.pt")


if __name__ == "__main__":
    main()
