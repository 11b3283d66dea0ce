#!/usr/bin/env python3
"""The two kernels of the token-statistics fit at a user's size, each next to the route a user has today on the same device, in the same process, alternating:

  tg_gram_accumulate  rows = 36 864 (8 videos x 12 chunks x 384 tokens), D = 3072, against `G64 += (Xc.float().T @ Xc.float()).double()` per fold-sized chunk
  tg_pca_coef_stats   same rows, ncoef = 64, against `((X.float() - mu) @ V.T)` followed by the reductions (sum, sum of squares, signed extreme)

Times are device events around `reps` back-to-back calls after a warm-up, the median of `rounds` alternating rounds.  The half product is rows * D * (D + 128)
multiply-adds (the 300 upper 128 x 128 tiles at D = 3072); its share of the 2.5 PFLOP/s dense bf16 peak is recorded.  There is no pass / fail threshold:
the figures go to profiles/token_stats_bench.json and the README row quotes them.

    python tools/bench_token_stats.py [--rows 36864] [--dim 3072] [--also NAME=other_build.so] [--out profiles/token_stats_bench.json]

--also times tg_gram_accumulate of another build of the library in the same alternating rounds and records whether its totals are bitwise the shipped ones."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tokensgen_amd import lib as L  # noqa: E402

PEAK_BF16 = 2.5e15


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
    ap.add_argument("--rows", type=int, default=36864)
    ap.add_argument("--dim", type=int, default=3072)
    ap.add_argument("--ncoef", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--also", action="append", default=[], metavar="NAME=LIB",
                    help="time tg_gram_accumulate of another build of the library in the same rounds (an A/B of a kernel variant); recorded under gram_variants_ms")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "token_stats_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_token_stats.py measures on the GPU: no device found")
    dev, lib = "cuda", L.load()
    rows, D, nc = a.rows, a.dim, a.ncoef
    F = lib.tg_gram_fold_rows()
    g = torch.Generator(device=dev).manual_seed(1)
    X = (torch.randn(rows, D, generator=g, device=dev) * 0.5 + 0.3).to(torch.bfloat16)
    stream = torch.cuda.current_stream().cuda_stream

    gram, colsum = torch.zeros(D, D, dtype=torch.float64, device=dev), torch.zeros(D, dtype=torch.float64, device=dev)
    g_ref, c_ref = torch.zeros_like(gram), torch.zeros_like(colsum)

    def ours_gram():
        L.check(lib.tg_gram_accumulate(X.data_ptr(), D, rows, D, gram.data_ptr(), colsum.data_ptr(), stream), "tg_gram_accumulate")

    def torch_gram():
        for r0 in range(0, rows, F):
            xc = X[r0:r0 + F].float()
            g_ref.add_((xc.T @ xc).double())
            c_ref.add_(xc.sum(0).double())

    variants = {}
    for spec in a.also:                                       # same arguments, another build's kernel
        name, path = spec.split("=", 1)
        other = ctypes.CDLL(os.path.abspath(path))
        other.tg_gram_accumulate.argtypes, other.tg_gram_accumulate.restype = L.PROTOTYPES["tg_gram_accumulate"], ctypes.c_int
        gv, cv = torch.zeros_like(gram), torch.zeros_like(colsum)

        def run(other=other, gv=gv, cv=cv):
            assert other.tg_gram_accumulate(X.data_ptr(), D, rows, D, gv.data_ptr(), cv.data_ptr(), stream) == 0
        variants[name] = (run, gv)

    mu = (X[:4096].float().mean(0)).contiguous()
    q, _ = torch.linalg.qr(torch.randn(D, nc, generator=g, device=dev))
    V = q.T.contiguous()
    s, s2 = torch.zeros(nc, dtype=torch.float64, device=dev), torch.zeros(nc, dtype=torch.float64, device=dev)
    ex = torch.zeros(nc, dtype=torch.float32, device=dev)
    ws = torch.empty(lib.tg_pca_coef_stats_ws_floats(rows, nc), dtype=torch.float32, device=dev)
    t_s, t_s2, t_ex = torch.zeros_like(s), torch.zeros_like(s2), torch.zeros_like(ex)

    def ours_coef():
        L.check(lib.tg_pca_coef_stats(X.data_ptr(), D, rows, D, V.data_ptr(), nc, mu.data_ptr(), s.data_ptr(), s2.data_ptr(), ex.data_ptr(), ws.data_ptr(), stream),
                "tg_pca_coef_stats")

    def torch_coef():
        y = (X.float() - mu) @ V.T
        yd = y.double()
        t_s.add_(yd.sum(0))
        t_s2.add_((yd * yd).sum(0))
        cand = y.gather(0, y.abs().argmax(0, keepdim=True))[0]
        t_ex.copy_(torch.where(cand.abs() > t_ex.abs(), cand, t_ex))

    # one call each first: same results (the sizes that are timed), and the warm-up
    ours_gram(); torch_gram(); ours_coef(); torch_coef()
    torch.cuda.synchronize()
    agree = {"gram_rel_l2_vs_torch": ((gram - g_ref).norm() / g_ref.norm()).item(), "colsum_rel_l2_vs_torch": ((colsum - c_ref).norm() / c_ref.norm()).item(),
             "coef_sumsq_rel_vs_torch": ((s2 - t_s2).abs() / t_s2).max().item(), "extreme_equal_sign": bool((torch.sign(ex) == torch.sign(t_ex)).all())}
    for name, (run, gv) in variants.items():
        run()
        torch.cuda.synchronize()
        agree[f"gram_{name}_bitwise_equal"] = bool(torch.equal(gv, gram))
    for fn in [ours_gram, torch_gram, ours_coef, torch_coef] + [run for run, _ in variants.values()]:
        timed(fn, 2)
    t = {k: [] for k in ["gram", "gram_torch", "coef", "coef_torch"] + [f"gram_{n}" for n in variants]}
    for _ in range(a.rounds):                                 # alternate: drift of the shared machine hits both routes alike
        t["gram"].append(timed(ours_gram, a.reps)); t["gram_torch"].append(timed(torch_gram, max(1, a.reps // 2)))
        t["coef"].append(timed(ours_coef, a.reps)); t["coef_torch"].append(timed(torch_coef, max(1, a.reps // 2)))
        for name, (run, _) in variants.items():
            t[f"gram_{name}"].append(timed(run, a.reps))
    med = {k: statistics.median(v) for k, v in t.items()}
    half_flops = 2.0 * rows * D * (D + 128) / 2
    res = {
        "device": torch.cuda.get_device_name(0), "rows": rows, "D": D, "ncoef": nc, "fold_rows": F, "reps": a.reps, "rounds": a.rounds,
        "tg_gram_accumulate_ms": med["gram"], "torch_fp32_gram_per_fold_chunk_ms": med["gram_torch"], "gram_speedup": med["gram_torch"] / med["gram"],
        "gram_half_product_tflops": half_flops / (med["gram"] * 1e-3) / 1e12, "gram_fraction_of_2.5PF": half_flops / (med["gram"] * 1e-3) / PEAK_BF16,
        "tg_pca_coef_stats_ms": med["coef"], "torch_fp32_project_and_reduce_ms": med["coef_torch"], "coef_speedup": med["coef_torch"] / med["coef"],
        "gram_variants_ms": {n: med[f"gram_{n}"] for n in variants}, "all_rounds_ms": t, "agreement": agree,
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps({k: v for k, v in res.items() if k != "all_rounds_ms"}))


if __name__ == "__main__":
    main()
