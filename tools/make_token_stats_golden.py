#!/usr/bin/env python3
"""Generate tests/golden/token_stats_tiny.pt: a tiny condensed-token set and what the REFERENCE's own pca.PCA (pca.py, imported from the reference tree on
the build machine, CPU only) fits on its valid rows, in fp64 and in fp32.  The fixture holds data only: the tokens, the expected values of both runs, and
the distance of the fp32 run from the fp64 run per quantity, the yardstick tests/test_token_stats_gpu.py holds the streaming fit to.

    python tools/make_token_stats_golden.py

Tokens bf16 [4, 8, 128, 4, 6] (2 chunks x 4 temporal queries; 192 rows per item), valid_chunks [2, 1, 2, 2] -> 672 valid rows.  Data: Gaussian with a
geometric spectrum (standard deviations 0.8^k, floor 1e-2) under a random rotation, plus a per-channel offset of about 0.3, rounded to bf16.  The seed is
the first that gives (a) eigenvalue ratios lambda_k / lambda_{k+1} >= 1.25 for the first 17 components and (b) for every kept component a margin >= 1.001
between the two largest |y| whenever their signs differ: a sign that hangs on a tie would test nothing."""
import importlib.util
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ref_shim  # noqa: E402

B, F, C, H, W, NTQ, D16 = 4, 8, 128, 4, 6, 4, 16
VALID = [2, 1, 2, 2]


def load_ref_pca():
    spec = importlib.util.spec_from_file_location("pca", os.path.join(ref_shim.REFERENCE_ROOT, "pca.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.PCA


def make_tokens(seed):
    g = torch.Generator().manual_seed(seed)
    n = B * F * H * W
    scale = torch.clamp(0.8 ** torch.arange(C, dtype=torch.float64), min=1e-2)
    q, _ = torch.linalg.qr(torch.randn(C, C, generator=g, dtype=torch.float64))
    offset = 0.3 + 0.05 * torch.randn(C, generator=g, dtype=torch.float64)
    x = (torch.randn(n, C, generator=g, dtype=torch.float64) * scale) @ q.T + offset
    return x.reshape(B, F, H, W, C).permute(0, 1, 4, 2, 3).contiguous().to(torch.bfloat16)


def valid_rows(tokens):
    return torch.cat([tokens[b, :v * NTQ].permute(0, 2, 3, 1).reshape(-1, C) for b, v in enumerate(VALID)])


def conditions(x64, pca64):
    z = x64 - x64.mean(0, keepdim=True)
    lam = torch.linalg.svdvals(z) ** 2
    ratio = (lam[:17] / lam[1:18]).min().item()
    y = pca64.transform(x64).abs()
    top = torch.topk(y, 2, dim=0)
    ysgn = torch.sign(pca64.transform(x64))
    margin = 1e9
    for j in range(D16):
        i0, i1 = top.indices[0, j], top.indices[1, j]
        if ysgn[i0, j] != ysgn[i1, j]:
            margin = min(margin, (top.values[0, j] / top.values[1, j]).item())
    return ratio, margin


def main():
    PCA = load_ref_pca()
    for seed in range(1000):
        tokens = make_tokens(seed)
        x64 = valid_rows(tokens).to(torch.float64)
        p64 = PCA(D16).fit(x64.clone())
        ratio, margin = conditions(x64, p64)
        if ratio >= 1.25 and margin >= 1.001:
            break
    else:
        raise SystemExit("no seed meets the conditions")
    assert x64.shape == (672, C)
    x32 = x64.to(torch.float32)
    p32 = PCA(D16).fit(x32.clone())
    y64, y32 = p64.transform(x64), p32.transform(x32)
    same_sign = ((p32.components_.double() * p64.components_).sum(1) > 0)
    assert bool(same_sign.all()), "the reference's fp32 and fp64 runs disagree on a sign: pick another seed"
    out = dict(
        tokens=tokens, valid_chunks=torch.tensor(VALID), num_temporal_queries=NTQ, n_components=D16, seed=seed, eig_ratio_min=ratio, extreme_margin_min=margin,
        components64=p64.components_.clone(), mean64=p64.mean_.clone(), coef_mean64=y64.mean(0), coef_std64=y64.std(0),
        components32=p32.components_.clone(), mean32=p32.mean_.clone(), coef_mean32=y32.mean(0), coef_std32=y32.std(0))
    # the reference's own fp32 error per quantity
    out["yard_components"] = (out["components32"].double() - out["components64"]).abs().max().item()
    out["yard_mean"] = (out["mean32"].double() - out["mean64"]).abs().max().item()
    out["yard_coef_mean"] = (out["coef_mean32"].double() - out["coef_mean64"]).abs().max().item()
    out["yard_coef_std"] = ((out["coef_std32"].double() - out["coef_std64"]).abs() / out["coef_std64"]).max().item()
    path = os.path.join(ROOT, "tests", "golden", "token_stats_tiny.pt")
    torch.save(out, path)
    print(f"token_stats_tiny.pt seed {seed}: eig ratio >= {ratio:.3f}, extreme margin >= {margin:.4f}, {os.path.getsize(path)} bytes; yardsticks "
          + ", ".join(f"{k[5:]} {out[k]:.3e}" for k in ("yard_components", "yard_mean", "yard_coef_mean", "yard_coef_std")))


if __name__ == "__main__":
    main()
