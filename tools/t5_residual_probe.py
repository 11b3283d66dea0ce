"""The T5 block's o / wo projection with its residual: tg_gemm_bf16 + tg_residual_add against TG_EPI_BIAS_GATE_RES with a gate of ones (the choice recorded at
tg_residual_add in include/tokensgen_hip.h).  [1 | 3, 226] rows, 24 different weights per pass (no cache reuse between launches), same process, alternating,
median of 7 passes.

    python tools/t5_residual_probe.py            # writes profiles/t5_residual_probe.json"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tokensgen_amd import kernels as K
from tokensgen_amd import lib as L

DEV, BF = "cuda", torch.bfloat16
res = {}
for B in (1, 3):
    for Kd in (4096, 10240):
        S, N = 226, 4096
        g = torch.Generator(device=DEV).manual_seed(1)
        a = torch.randn(B, S, Kd, generator=g, device=DEV).to(BF)
        ws = [(torch.randn(N, Kd, generator=g, device=DEV) * Kd ** -0.5).to(BF) for _ in range(24)]      # 24 layers' weights: no L2 / MALL reuse between launches
        x0 = torch.randn(B, S, N, generator=g, device=DEV).to(BF)
        o = torch.empty_like(x0)
        ones = torch.ones(1, 1, N, dtype=BF, device=DEV).expand(B, 1, N)
        table = K.GroupTable(ones, torch.zeros(S, dtype=torch.uint8, device=DEV), [0], [0], [0], [0])

        def two(x):
            for w in ws:
                K.gemm(a, w, None, o)
                K.residual_add(x, o, x)

        def fused(x):
            for w in ws:
                K.gemm(a, w, None, x, epilogue=L.EPI_BIAS_GATE_RES, residual=x, gate=table)

        def t(fn):
            x = x0.clone()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record(); fn(x); e.record(); torch.cuda.synchronize()
            return s.elapsed_time(e), x
        for fn in (two, fused):
            t(fn), t(fn)
        ms = {"two": [], "fused": []}
        for _ in range(7):
            ms["two"].append(t(two)[0]); ms["fused"].append(t(fused)[0])
        xa, xb = t(two)[1], t(fused)[1]
        res[f"B{B}_K{Kd}"] = dict(two_ms=statistics.median(ms["two"]), fused_ms=statistics.median(ms["fused"]), two_runs=ms["two"], fused_runs=ms["fused"],
                                  rel_diff=((xa.float() - xb.float()).norm() / xa.float().norm()).item())
        print(f"B{B}_K{Kd}", res[f"B{B}_K{Kd}"], flush=True)
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "t5_residual_probe.json")
json.dump(res, open(out, "w"), indent=1)
