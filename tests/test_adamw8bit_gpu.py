"""GPU: block-wise 8-bit AdamW (optim.AdamW8bit -> tg_adamw8bit_step) against the CPU restatement tests/adamw8bit_ref.py, step by step from the
kernel's own previous state; run-to-run bitwise; inside To2VTrainStep with a checkpoint / resume; and at the full 42-layer + Resampler layout
(allocation per parameter, one step on sampled tensors)."""
import os
import sys

import pytest
import torch

import adamw8bit_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HYPER = dict(lr=3e-2, betas=(0.9, 0.95), eps=1e-8, weight_decay=1e-4)

# the mixed layout: < 4096 (fp32 moments), exactly 2 blocks, 4097 (a 1-element tail block), 5 blocks + 1, an exactly-zero gradient; the
# transformer prefix is clipped, the resampler. rest is not
SHAPES = {"transformer_blocks.0.a.vip_small": (40, 100), "transformer_blocks.0.b.vip_two": (2, 2048), "transformer_blocks.0.c.vip_odd": (4097,),
          "transformer_blocks.0.d.vip_tail": (2048 * 5 + 1,), "transformer_blocks.0.e.vip_zero": (3, 2000), "resampler.proj.weight": (4097,),
          "resampler.proj.bias": (300,)}
ZERO = "transformer_blocks.0.e.vip_zero"


def _mixed(seed):
    from tokensgen_amd import optim
    g = torch.Generator().manual_seed(seed)
    params = {k: (torch.randn(*s, generator=g) * 0.1).to(BF) for k, s in SHAPES.items()}
    arena = optim.ParamArena({k: v.to(DEV) for k, v in params.items()}, optim.arena_order(list(params), 1), DEV, moments=False)
    n_clip = arena.prefix_elems(lambda n: not n.startswith("resampler."))
    opt = optim.AdamW8bit(arena, max_grad_norm=1.0, clip_elems=n_clip, **HYPER)
    return arena, opt, g


def _grads(g, step):
    out = {k: torch.randn(*s, generator=g) * (3.0 if step == 1 else 0.005) for k, s in SHAPES.items()}      # step 1 clips, the others do not
    out[ZERO] = torch.zeros(SHAPES[ZERO])
    return out


def _snapshot(opt, arena, names):
    """{name: (parameter fp32, gradient, TensorState)}: CPU copies of what the kernel holds for each named tensor."""
    out = {}
    for r in opt.rows:
        if r.name not in names:
            continue
        s = R.TensorState(r.numel, opt.block_size, opt.min_8bit_size)
        assert s.eight_bit == (r.kind == 1)
        el, bl = slice(r.offset, r.offset + r.numel), slice(r.state, r.state + r.blocks)
        if s.eight_bit:
            s.codes1, s.codes2, s.absmax1, s.absmax2 = opt.state1[el].cpu(), opt.state2[el].cpu(), opt.absmax1[bl].cpu(), opt.absmax2[bl].cpu()
        else:
            s.m, s.v = opt.small_m[r.state:r.state + r.numel].cpu(), opt.small_v[r.state:r.state + r.numel].cpu()
        out[r.name] = (arena.param[el].float().cpu(), arena.grad[el].cpu(), s)
    return out


def _ulp_f32(x):
    return torch.where(x == 0, torch.zeros_like(x), (x.abs().log2().floor() - 23).exp2())


def _compare_step(opt, arena, before, stats):
    """One kernel step (already taken) against the restatement applied to the state the kernel started from (`before`: _snapshot)."""
    cs = float(opt.coef[1])
    after = _snapshot(opt, arena, set(before))
    for r in opt.rows:
        if r.name not in before:
            continue
        p0, g0, s = before[r.name]
        c = cs if r.clipped else 1.0
        if not s.eight_bit:                                                   # size of the terms of m / v: a fused multiply-add rounds once per sum,
            gc = g0 * c                                                       # so where the two terms cancel the result differs by ulps of the terms
            scale_m = opt.betas[0] * s.m.abs() + (1 - opt.betas[0]) * gc.abs()
            scale_v = opt.betas[1] * s.v + (1 - opt.betas[1]) * gc * gc
        want = R.step_tensor(p0, g0, s, opt.t, opt.lr, opt.betas, opt.eps, opt.wd, c)
        got, _, a = after[r.name]
        ulp = want.abs().clamp_min(1e-30).log2().floor().exp2() * 2.0 ** -7
        assert ((got - want).abs() <= ulp).all(), (r.name, opt.t)                        # at most one bf16 ulp
        stats["param_diff"] = max(stats.get("param_diff", 0.0), float((got != want).float().mean()))
        if s.eight_bit:
            for ga, wa in ((a.absmax1, s.absmax1), (a.absmax2, s.absmax2)):
                err = (ga - wa).abs() / _ulp_f32(wa).clamp_min(1e-45)
                assert bool(torch.isfinite(ga).all()) and bool(((ga == wa) | (err <= 1.0)).all()), (r.name, opt.t)
                stats["absmax_ulps"] = max(stats.get("absmax_ulps", 0.0), float(torch.where(ga == wa, torch.zeros_like(err), err).max()))
            for gc, wc in ((a.codes1, s.codes1), (a.codes2, s.codes2)):
                d = (gc.int() - wc.int()).abs()
                assert int(d.max()) <= 1, (r.name, opt.t)
                stats["codes_off"] = stats.get("codes_off", 0) + int((d != 0).sum())
                stats["codes"] = stats.get("codes", 0) + d.numel()
        else:
            for gm, wm, sc in ((a.m, s.m, scale_m), (a.v, s.v, scale_v)):
                assert bool(((gm - wm).abs() <= 3 * _ulp_f32(sc)).all()), (r.name, opt.t)     # fp32 moments: contraction of the same expression


@pytest.mark.timeout(300)
def test_adamw8bit_kernel_vs_restatement(parity):
    arena, opt, g = _mixed(11)
    inside = torch.zeros(arena.numel, dtype=torch.bool)
    for n in arena.names:
        inside[arena.offsets[n]:arena.offsets[n] + arena.views[n].numel()] = True
    assert (~inside).any()                                                    # there is padding between the tensors
    pad = lambda: (arena.param.cpu()[~inside].clone(), opt.state1.cpu()[~inside].clone(), opt.state2.cpu()[~inside].clone(), arena.grad.cpu()[~inside].clone())
    pad0 = pad()
    stats = {}
    for step in range(5):
        grads = _grads(g, step)
        arena.accumulate({k: v.to(DEV) for k, v in grads.items()}, 1.0)
        before = _snapshot(opt, arena, set(SHAPES))
        norm = float(arena.grad[:opt.clip_elems].double().norm())
        opt.step()
        torch.cuda.synchronize()
        assert abs(float(opt.coef[0]) - norm) < 1e-4 * norm
        assert (float(opt.coef[1]) < 1.0) == (step == 1)
        _compare_step(opt, arena, before, stats)
        assert float(arena.grad.abs().max()) == 0.0                          # zero_grad in the same pass
        for a, b in zip(pad(), pad0):
            assert torch.equal(a, b)                                          # arena padding neither written nor turned into state
        zr = next(r for r in opt.rows if r.name == ZERO)                      # zero gradient: absmax 0, the code of 0.0, decay only, no NaN
        assert float(opt.absmax1[zr.state:zr.state + zr.blocks].abs().max()) == 0 and float(opt.absmax2[zr.state:zr.state + zr.blocks].abs().max()) == 0
        assert bool((R.QMAP1[opt.state1[zr.offset:zr.offset + zr.numel].cpu().long()] == 0).all())
        assert bool(torch.isfinite(arena.param.float()).all())
    parity(stats["param_diff"], 2e-2, "fraction of parameters one bf16 ulp off the restatement, worst tensor and step")
    parity(stats["absmax_ulps"], 1.01, "absmax: worst distance to the restatement in fp32 ulps")
    parity(stats["codes_off"] / stats["codes"], 1e-3, "fraction of 8-bit codes one code off the restatement (FMA contraction)")


@pytest.mark.timeout(300)
def test_adamw8bit_is_run_to_run_bitwise():
    def run():
        arena, opt, g = _mixed(12)
        for step in range(3):
            arena.accumulate({k: v.to(DEV) for k, v in _grads(g, step).items()}, 1.0)
            opt.step()
        torch.cuda.synchronize()
        return [t.clone() for t in (arena.param, opt.state1, opt.state2, opt.absmax1, opt.absmax2, opt.small_m, opt.small_v)]
    a, b = run(), run()
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert int(a[1].count_nonzero()) > 0 and float(a[3].abs().max()) > 0


@pytest.mark.timeout(600)
def test_train_step_with_adamw8bit_checkpoint_resume(tmp_path):
    """train.To2VTrainStep on the 2-layer model of test_training_steps_reduce_the_loss_... with AdamW8bit on a moments=False arena: the loss falls,
    frozen tensors are untouched; a checkpoint after window 2, resumed in a fresh optimizer, gives bitwise the uninterrupted window 3."""
    import numpy as np
    from oracle import dit_ref as O
    from oracle import scheduler_ref as S
    from tokensgen_amd import optim, train
    B, H, Nt, Fr, Hh, Ww = 1, 2, 9, 4, 10, 12
    f32 = np.float32
    cfg = dict(num_attention_heads=H, attention_head_dim=64, num_layers=2, patch_size=2, time_embed_dim=128, text_embed_dim=64, in_channels=16, out_channels=16)
    sd = {k: v.to(BF).to(DEV).contiguous() for k, v in O.make_state_dict(cfg, n_vip_dim=128, seed=95, std=0.08).items()}
    frozen_before = {k: v.clone() for k, v in sd.items() if "vip_" not in k}
    tr = train.To2VTrainer(sd, H, 2, patch_size=2, vip_scale=1.0)
    order = optim.arena_order(tr.trainable, 2)
    fp32_sd = optim.AdamW(optim.ParamArena({k: sd[k] for k in tr.trainable}, order, DEV)).state_dict()
    arena = optim.ParamArena({k: sd[k] for k in tr.trainable}, order, DEV, moments=False)
    tr.use_arena(arena)
    start = arena.param.clone()
    opt = optim.AdamW8bit(arena, lr=2e-3, max_grad_norm=1.0)
    assert {r.kind for r in opt.rows} == {0, 1}                               # both kinds: 128 x 128 weights and 128-element biases
    _, ac = S.alphas_cumprod()
    ac = torch.as_tensor(ac, dtype=torch.float32)
    step = train.To2VTrainStep(tr, arena, opt, ac, accumulation_steps=2)
    g = torch.Generator().manual_seed(96)
    x0, noise = (torch.randn(B, Fr, 16, Hh, Ww, generator=g).to(BF).to(DEV) for _ in range(2))
    text = (torch.randn(B, Nt, 64, generator=g)).to(BF).to(DEV)
    vip = (torch.randn(B, 5, 128, 2, 3, generator=g)).to(BF).to(DEV)
    ts = torch.tensor([[500, 520, 480, 510]])
    rope = O.rope_3d(64, np.arange(4, dtype=f32), np.arange(5, dtype=f32), np.arange(6, dtype=f32))
    vrope = O.rope_3d(64, np.arange(4, dtype=f32) + f32(3), np.arange(5, dtype=f32), np.arange(6, dtype=f32))
    crope = O.rope_3d(64, np.linspace(1000, 1016.25, 5, dtype=f32), np.arange(2, dtype=f32), np.arange(3, dtype=f32))
    window = lambda st: [st.micro_step(x0, noise, ts, text, vip, rope, vrope, crope) for _ in range(2)]
    losses, ck, p2 = [], None, None
    for w in range(3):
        out = window(step)
        assert [d for _, d in out] == [False, True]
        losses += [float(l) for l, _ in out]
        if w == 1:
            torch.save(step.state_dict(), tmp_path / "ck.pt")
            p2 = arena.param.clone()
    assert opt.t == 3 and losses[0] == losses[1]
    assert losses[2] < losses[0] and losses[4] < losses[0], losses
    assert (arena.param != start).float().mean().item() > 0.5
    for k, v in frozen_before.items():
        assert torch.equal(sd[k], v), k
    want = [t.clone() for t in (arena.param, opt.state1, opt.state2, opt.absmax1, opt.absmax2, opt.small_m, opt.small_v)]
    # resume: window-2 parameters + checkpoint into a fresh optimizer and loop state
    arena.param.copy_(p2)
    opt2 = optim.AdamW8bit(arena, lr=2e-3, max_grad_norm=1.0)
    step2 = train.To2VTrainStep(tr, arena, opt2, ac, accumulation_steps=2)
    ck = torch.load(tmp_path / "ck.pt", weights_only=False)
    step2.load_state_dict(ck)
    assert opt2.t == 2 and step2.micro == 4
    out = window(step2)
    assert [d for _, d in out] == [False, True] and [float(l) for l, _ in out] == losses[4:6]
    got = [arena.param, opt2.state1, opt2.state2, opt2.absmax1, opt2.absmax2, opt2.small_m, opt2.small_v]
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    with pytest.raises(ValueError, match="adamw"):
        opt2.load_state_dict(fp32_sd)


@pytest.mark.timeout(1200)
def test_adamw8bit_full_layout_memory_and_step(parity):
    """The 42-layer To2V trainable layout + the Resampler (1.97 B parameters), built as tests/test_full_shape_gpu.py builds it: the 8-bit state
    allocates <= 2.05 B per parameter; a step from a non-trivial state matches the restatement on sampled tensors (independent per tensor)."""
    from tokensgen_amd import optim
    sys.path.insert(0, ROOT)
    import bench
    torch.cuda.empty_cache()
    model = bench.build_model(DEV, 42)
    msd = {k: v.detach() for k, v in model.state_dict().items()}
    params = {k: msd[k] for k in sorted(k for k in msd if "vip_" in k)}
    rsd, _, _ = bench.build_resampler_sd(DEV)
    params.update({"resampler." + k: v for k, v in rsd.items()})
    n_params = sum(v.numel() for v in params.values())
    arena = optim.ParamArena(params, optim.arena_order(list(params), 42), DEV, moments=False)
    del model, msd, params, rsd
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    assert 1.9e9 < n_params < 2.05e9
    n_clip = arena.prefix_elems(lambda n: not n.startswith("resampler."))
    m0 = torch.cuda.memory_allocated()
    opt = optim.AdamW8bit(arena, lr=2e-4, betas=(0.9, 0.95), eps=1e-8, weight_decay=1e-4, max_grad_norm=1.0, clip_elems=n_clip)
    torch.cuda.synchronize()
    state_bytes = torch.cuda.memory_allocated() - m0
    parity(state_bytes / n_params, 2.05, f"AdamW8bit state bytes per parameter ({state_bytes / 2 ** 30:.2f} GiB for {n_params} parameters; "
                                         f"fp32 moments: {8 * arena.numel / 2 ** 30:.2f} GiB)")
    by_name = {r.name: r for r in opt.rows}
    pick = [next(n for n, r in by_name.items() if r.kind == 0 and not n.startswith("resampler.")),              # fp32 moments
            next(n for n, r in by_name.items() if r.kind == 1 and r.numel % opt.block_size == 0 and r.clipped),   # whole blocks
            next(n for n, r in by_name.items() if r.kind == 1 and r.numel % opt.block_size != 0),                # a partial tail block
            next(n for n, r in by_name.items() if r.kind == 1 and not r.clipped)]                                 # the unclipped Resampler
    gen = torch.Generator(device=DEV).manual_seed(5)
    for t in range(2):                                                        # step 2 starts from a non-trivial 8-bit state
        for n in arena.names:                                                 # gradients inside the tensors only: the padding stays zero
            arena.grad_view(n).normal_(generator=gen).mul_(2e-5 if t else 1e-5)
        if t == 1:
            before = _snapshot(opt, arena, set(pick))
        opt.step()
    torch.cuda.synchronize()
    stats = {}
    _compare_step(opt, arena, before, stats)
    assert float(arena.grad.abs().max()) == 0.0
    parity(stats["codes_off"] / stats["codes"], 1e-3, "full layout: fraction of 8-bit codes one code off the restatement")
    parity(stats["param_diff"], 2e-2, "full layout: fraction of parameters one bf16 ulp off the restatement")
