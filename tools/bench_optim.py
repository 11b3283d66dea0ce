"""Optimizer step at the full To2V trainable layout (42 layers of vip_ tensors + the Resampler, 1.97 B parameters): optim.AdamW (fp32 moments) against
optim.AdamW8bit (block-wise 8-bit moments) and optim.Prodigy in the same process, alternating, timed with device events.  Each step = clip
coefficient (one read of the clipped gradient) + the optimizer's launches; algorithmic bytes of the AdamW pass: 28 B / element fp32 (bf16 parameter
read + write, fp32 gradient read + zero, both fp32 moments read + written), 16 B / element 8-bit (the moments as 1-byte codes); Prodigy 56 B /
element: pass 1 36 (g, m, v, s, delta read; m, v, s written, g zeroed), pass 2 20 (m, v, delta, p0 read; delta, param written).  Also the
optimizer-state memory of each, measured as torch.cuda.memory_allocated deltas.  After the timed steps Prodigy's delta must be non-zero inside the
LAST tensor of the arena (the 64-bit element indexing, which no small test reaches).  Prints one JSON line; `--out PATH` also writes it to a file (the
committed records are profiles/r7_optim_step.json and profiles/prodigy_step.json).

`--stochastic-round`: instead, what the stochastic bf16 parameter write (stochastic_round=True: tg_adamw_step_sr / tg_adamw8bit_step_sr, one
Philox4x32-10 call per 8 elements) costs AdamW and AdamW8bit at the same layout: ONE optimizer per kind on one arena, the switch flipped off / on /
off / on ... in the same process, device events, median of `--sr-rounds` (5) per setting after a warm-up round of both; reports the on : off ratio per
optimizer (the committed record is profiles/sr_optim_step.json)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM = 8.0e12          # MI355X HBM3E peak, bytes / s


def layout_params(dev):
    import bench
    model = bench.build_model(dev, 42)
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    params = {k: sd[k] for k in sorted(k for k in sd if "vip_" in k)}
    rsd, _, _ = bench.build_resampler_sd(dev)
    params.update({"resampler." + k: v for k, v in rsd.items()})
    return model, params


def _emit(rec, out):
    line = json.dumps(rec)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


def _timed_step(opt):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    opt.step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stochastic_round_cost(a):
    """The --stochastic-round mode: on : off ratio of the step time per optimizer, same process, same arena, alternating."""
    from tokensgen_amd import optim
    dev = "cuda"
    model, params = layout_params(dev)
    n_params = sum(v.numel() for v in params.values())
    order = optim.arena_order(list(params), 42)
    a32 = optim.ParamArena(params, order, dev)
    a8 = optim.ParamArena(params, order, dev, moments=False)
    del model, params
    torch.cuda.empty_cache()
    n_clip = a32.prefix_elems(lambda n: not n.startswith("resampler."))
    hyper = dict(lr=2e-4, betas=(0.9, 0.95), eps=1e-8, weight_decay=1e-4, max_grad_norm=1.0, clip_elems=n_clip, sr_seed=3)
    runs = {"adamw_fp32": (a32, optim.AdamW(a32, **hyper), 28), "adamw_8bit": (a8, optim.AdamW8bit(a8, **hyper), 16)}
    gen = torch.Generator(device=dev).manual_seed(3)
    grad = torch.zeros_like(a32.grad)
    for n in a32.names:
        v = a32.grad_view(n)
        grad[a32.offsets[n]:a32.offsets[n] + v.numel()].normal_(generator=gen).mul_(1e-5)
    ms = {k: {False: [], True: []} for k in runs}
    for r in range(a.sr_rounds + 1):                 # round 0: warm-up of both settings (code objects, first touch)
        for name, (arena, opt, _) in runs.items():
            for sr in (False, True):
                opt.stochastic_round = sr
                arena.grad.copy_(grad)
                torch.cuda.synchronize()
                t = _timed_step(opt)
                if r:
                    ms[name][sr].append(t)
    rec = {"what": "optimizer step at the full To2V trainable layout (clip coefficient + update), stochastic bf16 rounding off / on alternating on "
                   "the same optimizer and arena, device events, median per setting",
           "params": n_params, "arena_elems": a32.numel, "rounds": a.sr_rounds, "readme_box_to_box_spread_adamw_fp32_ms": [12.1, 13.2]}
    for name, (arena, opt, bpe) in runs.items():
        off, on = (sorted(ms[name][sr])[len(ms[name][sr]) // 2] for sr in (False, True))
        byt = bpe * arena.numel
        rec[name] = {"off_ms": [round(x, 3) for x in ms[name][False]], "on_ms": [round(x, 3) for x in ms[name][True]], "off_ms_median": round(off, 3),
                     "on_ms_median": round(on, 3), "on_over_off": round(on / off, 4), "algorithmic_bytes": byt,
                     "off_tbs": round(byt / off / 1e9, 3), "on_tbs": round(byt / on / 1e9, 3)}
        assert bool(torch.isfinite(arena.param[:1 << 20].float()).all())
    _emit(rec, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--stochastic-round", action="store_true", help="measure the stochastic bf16 rounding switch (off / on alternating) instead")
    ap.add_argument("--sr-rounds", type=int, default=5, help="timed rounds per setting of --stochastic-round (the median is reported)")
    a = ap.parse_args()
    if a.stochastic_round:
        return stochastic_round_cost(a)
    from tokensgen_amd import optim
    dev = "cuda"
    model, params = layout_params(dev)
    n_params = sum(v.numel() for v in params.values())
    order = optim.arena_order(list(params), 42)
    m0 = torch.cuda.memory_allocated()
    a32 = optim.ParamArena(params, order, dev)
    m1 = torch.cuda.memory_allocated()
    a8 = optim.ParamArena(params, order, dev, moments=False)
    m2 = torch.cuda.memory_allocated()
    ap = optim.ParamArena(params, order, dev)
    del model, params
    torch.cuda.empty_cache()
    n_clip = a32.prefix_elems(lambda n: not n.startswith("resampler."))
    hyper = dict(lr=2e-4, betas=(0.9, 0.95), eps=1e-8, weight_decay=1e-4, max_grad_norm=1.0, clip_elems=n_clip)
    opt32 = optim.AdamW(a32, **hyper)
    m3 = torch.cuda.memory_allocated()
    opt8 = optim.AdamW8bit(a8, **hyper)
    torch.cuda.synchronize()
    m4 = torch.cuda.memory_allocated()
    optp = optim.Prodigy(ap, lr=1.0, betas=(0.9, 0.95), eps=1e-8, weight_decay=1e-4, decouple=True, max_grad_norm=1.0, clip_elems=n_clip)
    torch.cuda.synchronize()
    m5 = torch.cuda.memory_allocated()
    state32 = (m1 - m0) - (m2 - m1)                 # the two fp32 moment arenas: what moments=False leaves out
    state8 = m4 - m3
    gen = torch.Generator(device=dev).manual_seed(3)
    grad = torch.zeros_like(a32.grad)
    for n in a32.names:
        v = a32.grad_view(n)
        grad[a32.offsets[n]:a32.offsets[n] + v.numel()].normal_(generator=gen).mul_(1e-5)
    runs = {"adamw_fp32": (a32, opt32, 28), "adamw_8bit": (a8, opt8, 16), "prodigy": (ap, optp, 56)}
    ms = {k: [] for k in runs}
    for r in range(a.rounds + 1):                    # round 0: warm-up (code objects, first touch)
        for name, (arena, opt, _) in runs.items():
            arena.grad.copy_(grad)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            opt.step()
            e1.record()
            torch.cuda.synchronize()
            if r:
                ms[name].append(e0.elapsed_time(e1))
    rec = {"what": "optimizer step at the full To2V trainable layout (clip coefficient + the optimizer's pass(es)), device events, alternating",
           "params": n_params, "arena_elems": a32.numel, "rounds": a.rounds}
    for name, (arena, opt, bpe) in runs.items():
        best = min(ms[name])
        byt = bpe * arena.numel
        rec[name] = {"ms": [round(x, 3) for x in ms[name]], "ms_min": round(best, 3), "algorithmic_bytes": byt,
                     "gbs": round(byt / best / 1e6, 1), "frac_of_8TBs": round(byt / best / 1e-3 / HBM, 3)}
    rec["state_bytes"] = {"adamw_fp32_moments": state32, "adamw_8bit": state8, "saved": state32 - state8,
                          "adamw_8bit_per_param": round(state8 / n_params, 4)}
    last = ap.names[-1]
    lo = ap.offsets[last]
    moved = int(optp.delta[lo:lo + ap.views[last].numel()].count_nonzero())
    assert moved > 0, f"Prodigy: delta is all zero inside the last tensor {last} at elements {lo}.. of {ap.numel}"
    rec["prodigy"].update({"state_bytes_per_param": round((m5 - m4) / n_params, 4), "arena_moment_bytes_per_param": round(state32 / n_params, 4),
                           "tbs": round(rec["prodigy"]["gbs"] / 1e3, 3), "tbs_vs_adamw_fp32": round(rec["prodigy"]["gbs"] / rec["adamw_fp32"]["gbs"], 3),
                           "ms_vs_adamw_fp32": round(rec["prodigy"]["ms_min"] / rec["adamw_fp32"]["ms_min"], 3),
                           "last_tensor": last, "last_tensor_offset": lo, "last_tensor_delta_nonzero": moved, "stats": optp.stats()})
    rec["speedup_8bit"] = round(rec["adamw_fp32"]["ms_min"] / rec["adamw_8bit"]["ms_min"], 3)
    _emit(rec, a.out)


if __name__ == "__main__":
    main()
