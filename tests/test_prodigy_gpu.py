"""GPU: Prodigy (optim.Prodigy -> tg_prodigy_step) against the CPU restatement tests/prodigy_ref.py, step by step from the kernel's own previous
state, on the mixed layout of tests/test_adamw8bit_gpu.py; run-to-run bitwise; the growth of d beside bf16 parameters on the device; inside
To2VTrainStep with a checkpoint / resume; and on the T2To adapter-only arena.

Bounds (fp32 ulps are those of the named magnitude's binade):
  m, v, s: 3 ulps of the size of their terms — the kernel may contract b * m + a * g into fused multiply-adds, the restatement rounds every operation
    (the bound tests/test_adamw8bit_gpu.py holds for the same expressions).
  delta: 8 ulps of max(|upd|, |delta|) — 3 ulps on m and v (the square root halves v's), one rounding each for sqrt, the sum with d * eps, the
    division, the product with dlr and the subtraction.
  d_denom against the fp64 sum of the kernel's own |s|: 1e-10 relative (3e4 fp64 terms reorder to under n * 2^-53 = 4e-12).
  d_numerator against the restatement's: 1e-10 of the sum of the absolute terms (fp64 reordering again; g is the same fp32 value on both sides).
  d, d_max, d_hat against the scalar rules on the kernel's own two sums, dlr: 1e-14 relative (one or two fp64 roundings)."""
import math

import pytest
import torch

import prodigy_ref as R
from test_prodigy_cpu import no_stall_problem

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16

# the mixed layout of tests/test_adamw8bit_gpu.py: 4000, 2 x 2048, 4097 and 5 x 2048 + 1 elements, one tensor with an exactly-zero gradient; the
# transformer prefix is clipped, the resampler. rest is not; every tensor but the second ends inside a 64-element slot (padding)
SHAPES = {"transformer_blocks.0.a.vip_small": (40, 100), "transformer_blocks.0.b.vip_two": (2, 2048), "transformer_blocks.0.c.vip_odd": (4097,),
          "transformer_blocks.0.d.vip_tail": (2048 * 5 + 1,), "transformer_blocks.0.e.vip_zero": (3, 2000), "resampler.proj.weight": (4097,),
          "resampler.proj.bias": (300,)}
ZERO = "transformer_blocks.0.e.vip_zero"
# betas: d has to leave d0 within the six steps.  Without bias correction d_hat of step 2 is d0 (1 - b1) / (sqrt(1 - b2) (1 + b3)) = 1.58 d0 at
# (0.9, 0.999).  With bias correction and safeguard_warmup the numerator carries bc = sqrt(1 - b2^t) / (1 - b1^t) and the denominator does not: at
# b2 = 0.999 bc is 0.32 .. 0.17 over the six steps and d_hat stays below d0, at the training yaml's (0.9, 0.95) bc is 2.2 .. 1.1 and d grows from step 3.
CONFIGS = {"flags_off": dict(decouple=False, use_bias_correction=False, safeguard_warmup=False, weight_decay=0.0, betas=(0.9, 0.999)),
           "all_flags_wd": dict(decouple=True, use_bias_correction=True, safeguard_warmup=True, weight_decay=1e-2, betas=(0.9, 0.95)),
           "decouple_wd": dict(decouple=True, use_bias_correction=False, safeguard_warmup=False, weight_decay=1e-2, betas=(0.9, 0.999)),
           "wd_in_gradient": dict(decouple=False, use_bias_correction=False, safeguard_warmup=False, weight_decay=1e-2, betas=(0.9, 0.999))}
BASE = dict(lr=1.0, eps=1e-8)


def _mixed(seed, cfg):
    from tokensgen_amd import optim
    g = torch.Generator().manual_seed(seed)
    params = {k: (torch.randn(*s, generator=g) * 0.1).to(BF) for k, s in SHAPES.items()}
    arena = optim.ParamArena({k: v.to(DEV) for k, v in params.items()}, optim.arena_order(list(params), 1), DEV, moments=True)
    n_clip = arena.prefix_elems(lambda n: not n.startswith("resampler."))
    opt = optim.Prodigy(arena, max_grad_norm=1.0, clip_elems=n_clip, **BASE, **cfg)
    direction = {k: torch.randn(*s, generator=g) for k, s in SHAPES.items()}
    return arena, opt, g, direction


def _grads(g, direction, step):
    """scale_k (G + 0.3 noise_k): one fixed direction, so g . (x0 - x) is positive and d_hat passes d0 early.  The first step clips (norm 3.4 over the
    2.7e4 clipped elements, coefficient 0.3), the others do not (0.85); the first must not dwarf the others, or the unclipped tensors' share of
    sum |s| keeps d_hat below d0 for as long as beta3 remembers it."""
    scale = 0.02 if step == 0 else 0.005
    out = {k: scale * (direction[k] + 0.3 * torch.randn(*s, generator=g)) for k, s in SHAPES.items()}
    out[ZERO] = torch.zeros(SHAPES[ZERO])
    return out


def _ulp_f32(x):
    return torch.where(x == 0, torch.zeros_like(x), (x.abs().clamp_min(1e-37).log2().floor() - 23).exp2())


def _state(arena, opt):
    return {"param": arena.param, "p0": opt.p0, "delta": opt.delta, "s": opt.s, "m": arena.exp_avg, "v": arena.exp_avg_sq, "grad": arena.grad}


def _snapshot(arena, opt):
    out = {k: v.detach().cpu().clone() for k, v in _state(arena, opt).items()}
    out["stats"] = opt.stats()
    return out


@pytest.mark.timeout(300)
@pytest.mark.parametrize("config", list(CONFIGS))
def test_prodigy_kernel_vs_restatement(parity, config):
    cfg = CONFIGS[config]
    arena, opt, g, direction = _mixed(21, cfg)
    h = R.hyper(**BASE, **cfg)
    inside = torch.zeros(arena.numel, dtype=torch.bool)
    for n in arena.names:
        inside[arena.offsets[n]:arena.offsets[n] + arena.views[n].numel()] = True
    assert (~inside).any() and arena.numel % 64 == 0 and opt.clip_elems % 64 == 0 and 0 < opt.clip_elems < arena.numel
    below_clip = torch.arange(arena.numel) < opt.clip_elems
    pad0 = None
    worst = {"m": 0.0, "v": 0.0, "s": 0.0, "delta": 0.0, "den": 0.0, "num": 0.0}
    rose = 0
    for step in range(6):
        arena.accumulate({k: v.to(DEV) for k, v in _grads(g, direction, step).items()}, 1.0)
        b = _snapshot(arena, opt)
        if pad0 is None:
            pad0 = {k: b[k][~inside].clone() for k in ("param", "p0", "delta", "s", "m", "v")}
        opt.step()
        torch.cuda.synchronize()
        a = _snapshot(arena, opt)
        cs = float(opt.coef[1])
        assert (cs < 1.0) == (step == 0)
        c = torch.where(below_clip, torch.tensor(cs, dtype=torch.float32), torch.tensor(1.0))
        # ---- the restatement from the kernel's previous state
        st = R.State(b["p0"], h["d0"])
        st.delta, st.m, st.v, st.s = b["delta"].clone(), b["m"].clone(), b["v"].clone(), b["s"].clone()
        st.d, st.d_max, st.d_numerator, st.t = b["stats"]["d"], b["stats"]["d_max"], b["stats"]["d_numerator"], opt.t
        dlr, a1, a2, a3 = R.coefficients(st.d, st.t, h)
        x = st.x()
        size_g = (c * b["grad"]).abs() + (abs(h["weight_decay"]) * x.abs() if (h["weight_decay"] != 0 and not h["decouple"]) else 0.0)
        scale = {"m": h["betas"][0] * b["m"].abs() + float(a1) * size_g, "v": h["betas"][1] * b["v"] + float(a2) * size_g * size_g,
                 "s": h["beta3"] * b["s"].abs() + float(a3) * size_g}
        num_sum, den, abs_terms = R.pass1(st, b["grad"], h, c)
        for k, want in (("m", st.m), ("v", st.v), ("s", st.s)):
            err = (a[k] - want).abs()
            ulps = torch.where(err == 0, torch.zeros_like(err), err / _ulp_f32(scale[k]).clamp_min(1e-45))
            worst[k] = max(worst[k], float(ulps.max()))
            assert float(ulps.max()) <= 3.0, (k, step, float(ulps.max()))
        # ---- the two sums and the scalar rules
        den_own = float(a["s"].abs().double().sum())
        assert den_own > 0
        worst["den"] = max(worst["den"], abs(a["stats"]["d_denom"] - den_own) / den_own)
        assert abs(a["stats"]["d_denom"] - den_own) <= 1e-10 * den_own
        dd0 = st.d / h["d0"]
        num_want = h["beta3"] * st.d_numerator + dd0 * dlr * num_sum
        num_tol = 1e-10 * (h["beta3"] * abs(st.d_numerator) + dd0 * dlr * abs_terms)
        if num_tol > 0:
            worst["num"] = max(worst["num"], abs(a["stats"]["d_numerator"] - num_want) / num_tol * 1e-10)
        assert abs(a["stats"]["d_numerator"] - num_want) <= num_tol, (step, a["stats"]["d_numerator"], num_want)
        assert (a["stats"]["d_numerator"] == 0.0) == (step == 0)
        d_hat = h["d_coef"] * a["stats"]["d_numerator"] / a["stats"]["d_denom"]      # the scalar rules alone, on the kernel's own two sums
        d_new = max(st.d, d_hat) if st.d == h["d0"] else st.d
        d_max = max(st.d_max, d_hat)
        d_new = min(d_max, d_new * h["growth_rate"])
        for k, want in (("d_hat", d_hat), ("d_max", d_max), ("d", d_new), ("dlr", dlr)):
            assert a["stats"][k] == pytest.approx(want, rel=1e-14), (k, step)
        assert a["stats"]["d"] >= b["stats"]["d"]
        rose += a["stats"]["d"] > b["stats"]["d"]
        # ---- the displacement and the parameter
        R.finalize(st, num_sum, den, h)
        delta_before = st.delta.clone()
        upd = R.pass2(st, dlr, h, x)
        err = (a["delta"] - st.delta).abs()
        ulps = torch.where(err == 0, torch.zeros_like(err), err / _ulp_f32(torch.maximum(upd.abs(), delta_before.abs())).clamp_min(1e-45))
        worst["delta"] = max(worst["delta"], float(ulps.max()))
        assert float(ulps.max()) <= 8.0, (step, float(ulps.max()))
        assert torch.equal((a["p0"].float() + a["delta"]).to(BF).view(torch.int16), a["param"].view(torch.int16))
        assert torch.equal(a["p0"], b["p0"])
        assert float(a["grad"].abs().max()) == 0.0                          # zero_grad in the same pass
        for k, v in pad0.items():
            assert torch.equal(a[k][~inside].view(torch.int16 if v.dtype == BF else torch.int32), v.view(torch.int16 if v.dtype == BF else torch.int32)), k
        for k in ("param", "delta", "s", "m", "v"):
            assert bool(torch.isfinite(a[k].float()).all()), k
        assert all(math.isfinite(v) for v in a["stats"].values())
    assert rose >= 3, rose                                                   # the d-dependent coefficients were exercised at several values of d
    print(f"prodigy {config}: worst {worst}, d / d0 = {a['stats']['d'] / h['d0']:.4g}, d rose at {rose} of 6 steps")
    parity(worst["delta"], 8.0 + 1e-9, f"{config}: delta, worst distance to the restatement in fp32 ulps of max(|upd|, |delta|)")
    parity(max(worst["m"], worst["v"], worst["s"]), 3.0 + 1e-9, f"{config}: m / v / s, worst distance to the restatement in fp32 ulps of their terms")
    parity(worst["den"], 1e-10, f"{config}: d_denom against the fp64 sum of the kernel's |s|, relative")


@pytest.mark.timeout(300)
def test_prodigy_is_run_to_run_bitwise():
    def run():
        arena, opt, g, direction = _mixed(22, CONFIGS["all_flags_wd"])
        for step in range(4):
            arena.accumulate({k: v.to(DEV) for k, v in _grads(g, direction, step).items()}, 1.0)
            opt.step()
        torch.cuda.synchronize()
        return [t.clone() for t in (arena.param, arena.exp_avg, arena.exp_avg_sq, opt.s, opt.delta, opt.p0, opt.scalars)]
    a, b = run(), run()
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert float(a[4].abs().max()) > 0 and float(a[6][0]) > 1e-6


@pytest.mark.timeout(300)
def test_d_grows_with_bf16_parameters_on_the_device():
    """The problem of tests/test_prodigy_cpu.py::test_d_grows_with_bf16_parameters with the gradient taken in torch at arena.param: the same three
    assertions and thresholds.  An implementation that updates the bf16 parameter in place ends at d / d0 = 1 and distance ratio 1."""
    from tokensgen_amd import optim
    p0, target = no_stall_problem()
    arena = optim.ParamArena({"w": p0.to(DEV)}, ["w"], DEV)
    opt = optim.Prodigy(arena, lr=1.0, max_grad_norm=None)
    target = target.to(DEV)
    dist0 = float((p0.float().to(DEV) - target).norm())
    ds = [opt.scalars.clone()]
    for _ in range(400):
        arena.accumulate({"w": arena.views["w"].float() - target}, 1.0)
        opt.step()
        ds.append(opt.scalars.clone())                                       # no host synchronisation inside the loop
    ds = torch.stack(ds).cpu()[:, 0].tolist()
    ratio = float((arena.views["w"].float() - target).norm()) / dist0
    print(f"device: d / d0 = {ds[-1] / 1e-6:.4g}, distance final / initial = {ratio:.4g}")
    assert all(y >= x for x, y in zip(ds, ds[1:]))
    assert ds[-1] / 1e-6 > 1e3
    assert ratio < 0.05
    assert opt.stats()["d"] == ds[-1] and opt.t == 400


@pytest.mark.timeout(600)
def test_train_step_with_prodigy_checkpoint_resume(tmp_path):
    """train.To2VTrainStep on the 2-layer model of test_train_step_with_adamw8bit_checkpoint_resume with Prodigy(lr=1.0): the loss falls over three
    windows (the third window's loss is below the first's), d leaves d0, frozen tensors are untouched; a checkpoint after window 2, loaded into a
    fresh Prodigy on the window-2 parameters, gives bitwise the uninterrupted window 3; an AdamW8bit checkpoint is refused.
    Measured: losses 1.8643948, 1.8643970, 1.8642330 and d = 4.77 d0 after the third step.  The second window comes after ONE step at d = d0 = 1e-6
    (updates of 3e-6 per element, which reach the bf16 parameter only where |p| < 1e-3): its loss differs from the first by 2.3e-6, the rounding
    noise of the bf16 forward, in either direction, so it is not compared."""
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
    sd8 = optim.AdamW8bit(optim.ParamArena({k: sd[k] for k in tr.trainable}, order, DEV, moments=False)).state_dict()
    arena = optim.ParamArena({k: sd[k] for k in tr.trainable}, order, DEV)
    tr.use_arena(arena)
    opt = optim.Prodigy(arena, lr=1.0)
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
    state = lambda o: [arena.param, arena.exp_avg, arena.exp_avg_sq, o.s, o.delta, o.p0, o.scalars]
    losses, p2 = [], None
    for w in range(3):
        out = window(step)
        assert [d for _, d in out] == [False, True]
        losses += [float(l) for l, _ in out]
        if w == 1:
            torch.save(step.state_dict(), tmp_path / "ck.pt")
            p2 = arena.param.clone()
    stats = opt.stats()
    print(f"To2V + Prodigy: losses {losses}, stats {stats}")
    assert opt.t == 3 and losses[0] == losses[1]
    assert stats["d"] > opt.d0
    assert float(opt.delta.abs().max()) > 0
    for k, v in frozen_before.items():
        assert torch.equal(sd[k], v), k
    want = [t.clone() for t in state(opt)]
    # resume: window-2 parameters + checkpoint into a fresh optimizer and loop state
    arena.param.copy_(p2)
    opt2 = optim.Prodigy(arena, lr=1.0)
    step2 = train.To2VTrainStep(tr, arena, opt2, ac, accumulation_steps=2)
    ck = torch.load(tmp_path / "ck.pt", weights_only=False)
    step2.load_state_dict(ck)
    assert opt2.t == 2 and step2.micro == 4
    out = window(step2)
    assert [d for _, d in out] == [False, True] and [float(l) for l, _ in out] == losses[4:6]
    assert all(torch.equal(x, y) for x, y in zip(state(opt2), want))
    with pytest.raises(ValueError, match="adamw8bit"):
        opt2.load_state_dict(sd8)
    assert losses[4] < losses[0], losses


@pytest.mark.timeout(600)
def test_t2to_adapter_only_with_prodigy():
    """train_t2to.make_arena with `optimizer: prodigy` on the adapter-only trainer (rank 128, trainable_modules=[]) of tests/test_t2to_lora_gpu.py
    returns a Prodigy on a moments=True arena; two windows of T2ToTrainStep lower the loss and move both lora_A and lora_B.
    Measured: losses 1.8923610 at the start, 1.8923783 after one window, 1.8923492 after two; 724 lora_A and 611 lora_B elements moved; d is
    still d0 (d_hat 0.51 d0 at the yaml's beta2 = 0.95).  Two steps at d0 move only the smallest weights, so the loss differences (1e-5 of 1.9) are
    of the size of the bf16 forward's rounding noise: the assertion on the loss holds on these inputs but says little; the ones on the optimizer's
    type, the arena and the moved tensors are what this test is for."""
    from test_t2to_lora_gpu import _adapter, _case, _lcfg
    from tokensgen_amd import optim
    from tokensgen_amd.train_t2to import T2ToTrainer, T2ToTrainStep, make_arena
    c = _case(601)
    ad = {k: v.to(DEV).contiguous() for k, v in _adapter(c["sd"], 602).items()}
    sd = {k: v.clone() for k, v in {**c["sd_dev"], **ad}.items()}
    tr = T2ToTrainer(sd, 2, 2, trainable_modules=[], lora=_lcfg())
    arena, opt = make_arena(tr, dict(optimizer="prodigy", learning_rate=1.0, prodigy_decouple=True, adam_weight_decay=1e-4))
    assert type(opt) is optim.Prodigy and sorted(arena.names) == sorted(ad) and arena.exp_avg is not None
    step = T2ToTrainStep(tr, arena, opt, c["acp"], accumulation_steps=1)
    before = {k: arena.views[k].clone() for k in arena.names}
    losses = []
    for _ in range(3):                                                       # the third forward measures what the second window's step did
        loss, did = step.micro_step(c["noise"].to(DEV), c["ts"], c["text"].to(DEV), c["rope"], [1, 2, 3], model_input=c["x0"].to(DEV))
        assert did and torch.isfinite(loss)
        losses.append(float(loss))
    moved = {kind: sum(int((arena.views[k] != before[k]).sum()) for k in arena.names if kind in k) for kind in ("lora_A", "lora_B")}
    print(f"T2To adapter + Prodigy: losses {losses}, moved {moved}, stats {opt.stats()}")
    assert moved["lora_A"] > 0 and moved["lora_B"] > 0
    assert losses[2] < losses[0], losses
