"""LoRA on one MI355X, same process, alternating, device events.  Two legs, one JSON line (`--out PATH` also writes it; the committed record is
profiles/lora_bench.json):

  wgrad: tg_lora_wgrad at the training shape (M = 2 x 17 776 token rows, N = 3072, R = 128: dB of one target, fp32 straight into an accumulator, beta = 1)
         against the route the tree had before it — train.linear_backward on the same [M, 3072] / [M, 128] operands (two transposes + tg_gemm_bf16 with a bf16
         result; its bias column sum is part of that function and is timed with it) + tg_grad_accumulate into the same accumulator.  Also R = 384
         (the three dA of to_q | to_k | to_v in one launch).  Algorithmic bytes of the new kernel: Y and T read once.
  step:  To2V micro-steps at the BASELINE config 5 shapes (batch 2, 13 latent frames of 60 x 90, 226 text + 480 vip tokens; the vip tokens are handed over
         directly, the Resampler is not part of this comparison) with a trainable rank-128 adapter against the same trainer with lora=None: ms, %, and the
         difference of the peak memory during a micro-step."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BF = torch.bfloat16


def _time(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def wgrad_leg(rounds):
    from tokensgen_amd import kernels as K
    from tokensgen_amd import lib as L
    from tokensgen_amd import train
    dev = "cuda"
    M, N = 2 * 17776, 3072
    g = torch.Generator(device=dev).manual_seed(1)
    y = (torch.randn(M, N, generator=g, device=dev) * 0.5).to(BF)
    rec = {"M": M, "N": N, "rounds": rounds}
    lib = L.load()
    for R in (128, 384):
        t = (torch.randn(M, R, generator=g, device=dev) * 0.5).to(BF)
        acc_new, acc_old = torch.zeros(N, R, device=dev), torch.zeros(N, R, device=dev)

        def new():
            K.lora_wgrad(y, t, acc_new, scale=0.5, beta=1.0)

        def old():
            dW, _, _ = train.linear_backward(t, y)               # dW = y^T t [N, R] bf16
            L.check(lib.tg_grad_accumulate(dW.contiguous().data_ptr(), 1, acc_old.data_ptr(), dW.numel(), 0.5, 0, K._stream()), "tg_grad_accumulate")
        ms = {"new": [], "old": []}
        for r in range(rounds + 1):                              # round 0: warm-up
            for name, fn in (("old", old), ("new", new)):
                v = _time(fn)
                if r:
                    ms[name].append(v)
        byt = 2 * M * (N + R)
        best = min(ms["new"])
        rec[f"R{R}"] = {"new_ms": [round(v, 4) for v in ms["new"]], "old_ms": [round(v, 4) for v in ms["old"]], "new_ms_median": round(statistics.median(ms["new"]), 4),
                        "old_ms_median": round(statistics.median(ms["old"]), 4), "speedup_median": round(statistics.median(ms["old"]) / statistics.median(ms["new"]), 2),
                        "algorithmic_bytes": byt, "new_TBs_at_min": round(byt / best / 1e9, 3),
                        "agreement_rel_l2": float(((acc_new - acc_old).norm() / acc_old.norm()).item())}
    return rec


def step_leg(layers, rounds):
    import bench
    from tokensgen_amd import lora, optim, train
    from tokensgen_amd import rope as R
    from tokensgen_amd.scheduler import CogVideoXDPMScheduler
    dev = torch.device("cuda")
    model = bench.build_model(dev, layers)
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    lcfg = lora.LoraConfig(rank=128, lora_alpha=64)
    ad = lora.init_adapter(lcfg, sd, torch.Generator().manual_seed(5))
    g = torch.Generator().manual_seed(6)
    for k in ad:                                                 # a trained adapter: B is not zero
        if k.endswith("lora_B.weight"):
            ad[k] = (torch.randn(ad[k].shape, generator=g) * 0.01).to(BF)
    acp = CogVideoXDPMScheduler(prediction_type="v_prediction", rescale_betas_zero_snr=True, snr_shift_scale=1.0, timestep_spacing="trailing").alphas_cumprod.to(torch.float32)
    legs = {}
    for name, cfg in (("base", None), ("lora", lcfg)):
        s = dict(sd)
        if cfg is not None:
            s.update({k: v.to(dev) for k, v in ad.items()})
        tr = train.To2VTrainer(s, 48, layers, patch_size=2, vip_scale=1.0, lora=cfg)
        arena = optim.ParamArena({k: s[k] for k in tr.trainable}, optim.arena_order(tr.trainable, layers), dev)
        tr.use_arena(arena)
        opt = optim.AdamW(arena, lr=2e-4, betas=(0.9, 0.95), eps=1e-8, weight_decay=1e-4, max_grad_norm=1.0)
        legs[name] = (tr, arena, train.To2VTrainStep(tr, arena, opt, acp, accumulation_steps=9))
    gd = torch.Generator(device=dev).manual_seed(7)
    B, nf, C, H, W = 2, 13, 16, 60, 90
    x0, noise = (torch.randn(B, nf, C, H, W, generator=gd, device=dev, dtype=torch.float32).to(BF) for _ in range(2))
    text = (torch.randn(B, 226, 4096, generator=gd, device=dev, dtype=torch.float32) * 0.1).to(BF)
    vip = (torch.randn(B, 480, sd["patch_embed.vip_proj.weight"].shape[1], generator=gd, device=dev, dtype=torch.float32) * 0.5).to(BF)
    f32 = np.float32
    rope = R.rope_3d_crop(64, (0, 0, 0), (nf, 30, 45), (nf, 30, 45))
    crope = R.rope_3d(64, np.linspace(1000, 1016.25, 5, dtype=f32), np.linspace(0, 30, 8, endpoint=False, dtype=f32), np.linspace(0, 45, 12, endpoint=False, dtype=f32))
    ts = torch.tensor([400, 700])
    ms, peak = {"base": [], "lora": []}, {}
    for r in range(rounds + 1):                                  # round 0: warm-up (frozen transposes, workspaces, code objects)
        for name, (tr, arena, step) in legs.items():
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            m0 = torch.cuda.memory_allocated()
            v = _time(lambda: step.micro_step(x0, noise, ts, text, vip, rope, rope, crope))
            if r:
                ms[name].append(v)
                peak[name] = torch.cuda.max_memory_allocated() - m0
    mb, ml = statistics.median(ms["base"]), statistics.median(ms["lora"])
    n_ad = sum(v.numel() for v in ad.values())
    return {"layers": layers, "rounds": rounds, "base_ms": [round(v, 2) for v in ms["base"]], "lora_ms": [round(v, 2) for v in ms["lora"]],
            "base_ms_median": round(mb, 2), "lora_ms_median": round(ml, 2), "overhead_ms": round(ml - mb, 2), "overhead_pct": round(100 * (ml - mb) / mb, 2),
            "blocks_kept": {n: legs[n][0].blocks_kept for n in legs}, "adapter_params": n_ad,
            "peak_during_micro_step_bytes": peak, "peak_delta_bytes": peak["lora"] - peak["base"],
            "adapter_arena_bytes": n_ad * (2 + 4 + 4 + 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--layers", type=int, default=42)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rec = {"what": "LoRA: tg_lora_wgrad against the transpose + GEMM + accumulate route, and the To2V micro-step with / without a trainable rank-128 adapter "
                   "(one MI355X, same process, alternating, device events)", "device": torch.cuda.get_device_name(0)}
    rec["wgrad"] = wgrad_leg(a.rounds)
    if not a.skip_step:
        rec["step"] = step_leg(a.layers, a.step_rounds)
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
