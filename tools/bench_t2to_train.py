#!/usr/bin/env python3
"""T2To training step at the yaml's shape (cogvideo_5b_vaevip_4x8x12_t2to.yaml: per_gpu_batch_size 3, max_num_chunks 24 -> 96 latent frames of
8 x 12 tokens + 226 text tokens = 9 442 tokens per item, 42 blocks of width 3072, gradient_accumulation_steps 5, AdamW8bit) on synthetic weights.

For both activation schedules (blocks keep their activations while memory allows / the yaml's per-block recompute) it times one warm-up micro-step
and then one whole accumulation window, and reports ms per micro-step (the window's micro-steps without the optimizer), ms per window, the optimizer
step (clip + AdamW8bit over 5.57 B parameters), the peak device memory, the transformer TFLOP of a micro-step counted from the shapes and
step_mfma_frac = TFLOP / time / 2.5 PFLOP/s.  Prints one JSON line; --out also writes it to a file.  The recompute schedule runs on the weights the
first schedule's optimizer step left (random weights after one AdamW step: its losses differ; the times do not depend on the values).

    python tools/bench_t2to_train.py [--layers 42] [--out profiles/t2to_train_bench.json]

--lora: adapter-only training (transformer_trainable_modules [], a rank-128 adapter on to_q | to_k | to_v | to_out.0, the base frozen) against full
fine-tuning IN THE SAME PROCESS, alternating, `--rounds` rounds (median reported): ms per micro-step (forward + masked loss + backward + gradient accumulation,
no optimizer step), peak device memory, arena bytes; the adapter-only micro-step with the low-rank tail folded into the projection GEMMs (kernels.gemm_lora)
and in the two-launch form; and the kernel A/B itself, gemm_lora against gemm + the accumulating tail GEMM at [28 326, 3072] -> 9216, R = 128 and at the shapes
the trainer launches.  --parent-json: a result line of this tool run from the PARENT commit on the same box just before (its full fine-tuning micro-step is
copied into the record next to this tree's).

    python tools/bench_t2to_train.py --lora [--parent-json FILE] [--out profiles/t2to_lora_bench.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

PEAK_BF16 = 2.5e15


def synthetic_state_dict(D, heads, layers, te, text_dim, dev):
    """Random bf16 weights under the reference's key names (the T2To DiT: patch 1, 16 channels in and out)."""
    g = torch.Generator(device=dev).manual_seed(0)
    sd = {}

    def lin(n, o, i, s=0.02):
        sd[n + ".weight"] = (torch.randn(o, i, device=dev, generator=g) * s).to(torch.bfloat16)
        sd[n + ".bias"] = (torch.randn(o, device=dev, generator=g) * s).to(torch.bfloat16)

    def ln(n, d):
        sd[n + ".weight"] = (1 + 0.1 * torch.randn(d, device=dev, generator=g)).to(torch.bfloat16)
        sd[n + ".bias"] = (0.1 * torch.randn(d, device=dev, generator=g)).to(torch.bfloat16)
    sd["patch_embed.proj.weight"] = (torch.randn(D, 16, 1, 1, device=dev, generator=g) * 0.1).to(torch.bfloat16)
    sd["patch_embed.proj.bias"] = torch.zeros(D, dtype=torch.bfloat16, device=dev)
    lin("patch_embed.text_proj", D, text_dim)
    lin("time_embedding.linear_1", te, D)
    lin("time_embedding.linear_2", te, te)
    for i in range(layers):
        b = f"transformer_blocks.{i}"
        for n in ("norm1", "norm2"):
            lin(f"{b}.{n}.linear", 6 * D, te)
            ln(f"{b}.{n}.norm", D)
        for n in ("to_q", "to_k", "to_v", "to_out.0"):
            lin(f"{b}.attn1.{n}", D, D)
        ln(f"{b}.attn1.norm_q", 64)
        ln(f"{b}.attn1.norm_k", 64)
        lin(f"{b}.ff.net.0.proj", 4 * D, D)
        lin(f"{b}.ff.net.2", D, 4 * D)
    ln("norm_final", D)
    lin("norm_out.linear", 2 * D, te)
    ln("norm_out.norm", D)
    lin("proj_out", 16, D)
    return sd


def micro_step_flops(B, N, D, layers, recomputed):
    """Transformer FLOP of one micro-step from the shapes: per block the forward GEMMs 24 B N D^2 (QKV 6, to_out 2, FF 16) and attention
    4 B N^2 D, the backward twice the GEMMs (dgrad + wgrad) and 2.5 x the attention; every recomputed block adds one more forward."""
    fwd = 24 * B * N * D * D + 4 * B * N * N * D
    bwd = 48 * B * N * D * D + 10 * B * N * N * D
    return layers * (fwd + bwd) + recomputed * fwd


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def kernel_ab(M, N, Kd, R, rounds, reps=8, dev="cuda"):
    """gemm_lora against the two-launch form (gemm EPI_BIAS + the accumulating gemm EPI_BIAS_GATE_RES with the scale in a gate table), interleaved: per round
    `reps` back-to-back launches of each form between two events; the median round of each."""
    from tokensgen_amd import kernels as K
    from tokensgen_amd import lib as L
    g = torch.Generator(device=dev).manual_seed(3)
    rnd = lambda *s, sc=1.0: (torch.randn(*s, device=dev, generator=g) * sc).to(torch.bfloat16)
    x, w, b, t, bm = rnd(1, M, Kd), rnd(N, Kd, sc=0.02), rnd(N), rnd(1, M, R), rnd(N, R, sc=0.02)
    out = torch.empty(1, M, N, dtype=torch.bfloat16, device=dev)
    tab = K.GroupTable(torch.full((1, 1, N), 0.5, dtype=torch.bfloat16, device=dev), torch.zeros(M, dtype=torch.uint8, device=dev), [0], [0], [0], [0])

    def fused():
        K.gemm_lora(x, w, b, t, bm, 0.5, out)

    def two():
        K.gemm(x, w, b, out, L.EPI_BIAS)
        K.gemm(t, bm, None, out, L.EPI_BIAS_GATE_RES, residual=out, gate=tab)

    def plain():
        K.gemm(x, w, b, out, L.EPI_BIAS)
    ms = {"gemm_lora": [], "two_launch": [], "plain_gemm": []}
    for fn in (fused, two, plain):
        fn()
    for _ in range(rounds):
        for name, fn in (("gemm_lora", fused), ("two_launch", two), ("plain_gemm", plain)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / reps)
    return dict(M=M, N=N, K=Kd, R=R, rounds=ms, gemm_lora_ms=_median(ms["gemm_lora"]), two_launch_ms=_median(ms["two_launch"]),
                plain_gemm_ms=_median(ms["plain_gemm"]), gemm_lora_over_two_launch=_median(ms["gemm_lora"]) / _median(ms["two_launch"]))


def lora_ab(a):
    """Adapter-only against full fine-tuning, alternating in one process (see the module docstring)."""
    from oracle import scheduler_ref as S
    from tokensgen_amd import lora
    from tokensgen_amd.train_t2to import T2ToTrainer, T2ToTrainStep, make_arena, t2to_rope
    dev = "cuda"
    D, H, te, Nt, text_dim = 3072, 48, 512, 226, 4096
    B, Fr = a.batch, 4 * a.chunks
    N = Nt + Fr * 96
    res = dict(metric="T2To micro-step: adapter-only (rank-128 LoRA on to_q|to_k|to_v|to_out.0, frozen base) vs full fine-tuning, same process, alternating",
               device=torch.cuda.get_device_name(0), batch=B, latent_frames=Fr, tokens_per_item=N, layers=a.layers, width=D, rounds=a.rounds)
    res["kernel_ab"] = [kernel_ab(B * N, 3 * D, D, 128, a.rounds),                                   # the issue's shape: the whole fused q|k|v projection
                        kernel_ab(B * N, D, D, 128, a.rounds),                                       # what the trainer launches: a third / to_out (forward), to_out's dgrad
                        kernel_ab(B * N, D, 3 * D, 384, a.rounds)]                                   # ... and the q|k|v input gradient (K = 3D, R = 3r)
    print(json.dumps(res["kernel_ab"]), file=sys.stderr, flush=True)
    sd = synthetic_state_dict(D, H, a.layers, te, text_dim, dev)
    yaml = dict(optimizer="adamw", use_8bit_adam=True, learning_rate=3e-4, adam_beta1=0.9, adam_beta2=0.95, adam_epsilon=1e-8,
                adam_weight_decay=1e-4, max_grad_norm=1.0)
    _, ac = S.alphas_cumprod()
    acp = torch.as_tensor(ac, dtype=torch.float32)
    full = T2ToTrainer(sd, H, a.layers)
    arena_f, opt_f = make_arena(full, yaml)
    lcfg = lora.LoraConfig(rank=128, lora_alpha=64)
    ad = lora.init_adapter(lcfg, sd, torch.Generator().manual_seed(2), device=dev)
    g = torch.Generator(device=dev).manual_seed(1)
    for k in ad:                                                                                     # a trained adapter: B is not zero
        if k.endswith("lora_B.weight"):
            ad[k] = (torch.randn(ad[k].shape, device=dev, generator=g) * 0.02).to(torch.bfloat16)
    lo = T2ToTrainer({**sd, **ad}, H, a.layers, trainable_modules=[], lora=lcfg)                      # the base tensors are the full trainer's arena views: one copy
    arena_l, opt_l = make_arena(lo, yaml)
    never = 1 << 30                                                                                  # no window ends: micro-steps only
    steps = {"full": T2ToTrainStep(full, arena_f, opt_f, acp, accumulation_steps=never), "lora": T2ToTrainStep(lo, arena_l, opt_l, acp, accumulation_steps=never)}
    rope = t2to_rope(Fr, device=dev)
    x0 = torch.randn(B, Fr, 16, 8, 12, device=dev, generator=g).to(torch.bfloat16)
    noise, text = torch.randn_like(x0), torch.randn(B, Nt, text_dim, device=dev, generator=g).to(torch.bfloat16)
    ts = torch.tensor([37, 512, 901, 250, 700, 90][:B])

    def micro(which, fused_tail=True):
        lo.fused_tail = fused_tail                                                                   # (the blocks keep their frozen weights' transposes across the switch)
        tr = steps[which].tr
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        loss, _ = steps[which].micro_step(noise, ts, text, rope, [a.chunks] * B, model_input=x0)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, torch.cuda.max_memory_allocated() / 1e9, tr.blocks_kept, float(loss)
    modes = (("full", "full", True), ("lora_gemm_lora", "lora", True), ("lora_two_launch", "lora", False))
    for _, which, ft in modes:                                                                       # warm-up: workspaces, the frozen weights' kept transposes
        micro(which, ft)
    runs = {m: [] for m, _, _ in modes}
    for r in range(a.rounds):
        for m, which, ft in modes:
            runs[m].append(micro(which, ft))
            print(json.dumps({m: runs[m][-1]}), file=sys.stderr, flush=True)
    for m in runs:
        res[m] = dict(ms_per_micro_step=_median([x[0] for x in runs[m]]), ms_rounds=[x[0] for x in runs[m]], peak_mem_gb=max(x[1] for x in runs[m]),
                      blocks_kept=runs[m][-1][2], loss=runs[m][-1][3])
    only_full = (arena_f.grad.numel() * 4 + sum(t.numel() * t.element_size() for t in vars(opt_f).values() if torch.is_tensor(t))) / 1e9
    res["arena"] = dict(full_params=arena_f.param.numel(), full_param_bytes=arena_f.param.numel() * 2, full_grad_bytes=arena_f.grad.numel() * 4,
                        lora_params=arena_l.param.numel(), lora_param_bytes=arena_l.param.numel() * 2, lora_grad_bytes=arena_l.grad.numel() * 4)
    res["note_memory"] = ("both trainers are resident: the adapter-only peaks include the full trainer's gradient arena and optimizer state, "
                          f"{only_full:.1f} GB that an adapter-only process does not hold (the bf16 parameter arena doubles as the frozen base)")
    res["full_trainer_only_state_gb"] = only_full
    res["lora_over_full"] = res["lora_gemm_lora"]["ms_per_micro_step"] / res["full"]["ms_per_micro_step"]
    res["gemm_lora_over_two_launch_micro_step"] = res["lora_gemm_lora"]["ms_per_micro_step"] / res["lora_two_launch"]["ms_per_micro_step"]
    if a.parent_json and os.path.exists(a.parent_json):
        with open(a.parent_json) as f:
            par = json.loads(f.read().strip().splitlines()[-1])
        res["parent_commit_full_fine_tuning"] = {k: par[k] for k in ("kept", "recompute", "layers", "batch", "tokens_per_item", "accumulation_steps") if k in par}
        res["full_over_parent_kept"] = res["full"]["ms_per_micro_step"] / par["kept"]["ms_per_micro_step"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=42)
    ap.add_argument("--batch", type=int, default=3)
    ap.add_argument("--chunks", type=int, default=24)
    ap.add_argument("--accum", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--lora", action="store_true", help="adapter-only vs full fine-tuning, alternating (see the module docstring)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-json", default=None)
    a = ap.parse_args()
    if a.lora:
        return lora_ab(a)
    from oracle import scheduler_ref as S
    from tokensgen_amd.train_t2to import T2ToTrainer, T2ToTrainStep, make_arena, t2to_rope
    dev = "cuda"
    D, H, te, Nt, text_dim = 3072, 48, 512, 226, 4096
    B, Fr = a.batch, 4 * a.chunks
    N = Nt + Fr * 96
    sd = synthetic_state_dict(D, H, a.layers, te, text_dim, dev)
    tr = T2ToTrainer(sd, H, a.layers)
    n_train = sum(sd[n].numel() for n in tr.trainable)
    yaml = dict(optimizer="adamw", use_8bit_adam=True, learning_rate=3e-4, adam_beta1=0.9, adam_beta2=0.95, adam_epsilon=1e-8,
                adam_weight_decay=1e-4, max_grad_norm=1.0)
    arena, opt = make_arena(tr, yaml)
    _, ac = S.alphas_cumprod()
    step = T2ToTrainStep(tr, arena, opt, torch.as_tensor(ac, dtype=torch.float32), accumulation_steps=a.accum)
    real_step, opt_ms = opt.step, []

    def timed_step(*args, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        real_step(*args, **kw)
        e1.record()
        e1.synchronize()
        opt_ms.append(e0.elapsed_time(e1))
    opt.step = timed_step
    g = torch.Generator(device=dev).manual_seed(1)
    rope = t2to_rope(Fr, device=dev)

    def batch():
        x0 = torch.randn(B, Fr, 16, 8, 12, device=dev, generator=g).to(torch.bfloat16)
        text = torch.randn(B, Nt, text_dim, device=dev, generator=g).to(torch.bfloat16)
        ts = torch.randint(0, 1000, (B,), generator=torch.Generator().manual_seed(int(step.micro)))
        return x0, torch.randn_like(x0), text, ts
    res = dict(metric="T2To training step (CogVideoX-5B T2To DiT, full fine-tuning, AdamW8bit)", device=torch.cuda.get_device_name(0),
               batch=B, latent_frames=Fr, tokens_per_item=N, layers=a.layers, width=D, accumulation_steps=a.accum, trainable_params=n_train,
               arena_param_gb=arena.param.numel() * 2 / 1e9, arena_grad_gb=arena.grad.numel() * 4 / 1e9)
    for name, budget in (("kept", None), ("recompute", 0)):
        tr.activation_budget_bytes = budget
        arena.grad.zero_()
        step.micro = 0
        x0, noise, text, ts = batch()
        step.micro_step(noise, ts, text, rope, [a.chunks] * B, model_input=x0)          # warm-up (not a window's last micro-step)
        torch.cuda.synchronize()
        arena.grad.zero_()
        step.micro = 0
        opt_ms.clear()
        torch.cuda.reset_peak_memory_stats()
        ms, losses = [], []
        t_win = time.perf_counter()
        for i in range(a.accum):
            x0, noise, text, ts = batch()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss, stepped = step.micro_step(noise, ts, text, rope, [a.chunks] * B, model_input=x0)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
            losses.append(float(loss))
        win = (time.perf_counter() - t_win) * 1e3
        assert stepped and len(opt_ms) == 1
        flops = micro_step_flops(B, N, D, a.layers, a.layers - tr.blocks_kept)
        micro = sum(ms[:-1]) / len(ms[:-1])
        res[name] = dict(ms_per_micro_step=micro, ms_per_window=win, ms_micro_steps=ms, optimizer_step_ms=opt_ms[0],
                         peak_mem_gb=torch.cuda.max_memory_allocated() / 1e9, blocks_kept=tr.blocks_kept, micro_step_tflop=flops / 1e12,
                         step_mfma_frac=flops / (micro * 1e-3) / PEAK_BF16, losses=losses)
        print(json.dumps({name: res[name]}), file=sys.stderr, flush=True)
    res["optimizer_step_ms"] = res["recompute"]["optimizer_step_ms"]
    res["tflop_per_micro_step_no_recompute"] = micro_step_flops(B, N, D, a.layers, 0) / 1e12
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
