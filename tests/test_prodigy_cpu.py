"""Prodigy without a GPU: the restatement (tests/prodigy_ref.py) against values worked out by hand for the first two steps, the property the
exact fp32 displacement exists for (d grows although the first updates lie far below a bf16 ulp of the weights), optim.get_optimizer on the
yaml's prodigy keys and the host side of optim.Prodigy (state, checkpoint checks)."""
import math
import warnings

import numpy as np
import pytest
import torch

import prodigy_ref as R

BF = torch.bfloat16
f32 = np.float32


def test_first_two_steps_closed_form():
    """Step 1 from delta = 0: the numerator is 0, d stays d0 and delta is the Adam-shaped update at d0; step 2's d_hat = num / den by hand."""
    h = R.hyper(betas=(0.9, 0.999))
    b1, b2, b3, d0, eps = 0.9, 0.999, math.sqrt(0.999), 1e-6, 1e-8
    p0 = torch.tensor([0.05, -0.1, 0.15, 0.2]).to(BF)
    g = np.array([0.5, 1.0, 2.0, 3.0], dtype=f32)
    st = R.State(p0, d0)
    R.step(st, torch.from_numpy(g), h)
    dlr = d0 * 1.0 * 1.0
    a1, a2, a3 = f32(d0 * (1 - b1)), f32(d0 * d0 * (1 - b2)), f32((d0 / d0) * dlr)
    m1, v1, s1 = a1 * g, a2 * g * g, a3 * g                                      # numpy fp32, one rounding per operation
    delta1 = -(f32(dlr) * (m1 / (np.sqrt(v1) + f32(d0 * eps))))
    assert st.d == d0 and st.d_max == d0 and st.d_numerator == 0.0 and st.d_hat == 0.0 and not st.skipped
    assert st.d_denom == float(np.abs(s1).astype(np.float64).sum())
    assert np.array_equal(st.delta.numpy(), delta1) and np.array_equal(st.m.numpy(), m1) and np.array_equal(st.v.numpy(), v1)
    assert float(np.abs(delta1).max()) < 1e-5                                    # far below a bf16 ulp of 0.05 .. 0.2 (2^-12 .. 2^-10):
    assert torch.equal(st.param(), p0)                                           # the bf16 parameter has not moved, the displacement has
    R.step(st, torch.from_numpy(g), h)
    s2 = f32(b3) * s1 + a3 * g
    num = b3 * 0.0 + (d0 / d0) * dlr * float((g.astype(np.float64) * (-delta1).astype(np.float64)).sum())
    d_hat = 1.0 * num / float(np.abs(s2).astype(np.float64).sum())
    assert st.d_hat == pytest.approx(d_hat, rel=1e-14) and st.d_numerator == pytest.approx(num, rel=1e-14)
    assert d_hat > d0 and st.d == st.d_max == st.d_hat                           # d == d0 -> max(d, d_hat); growth_rate inf -> d = d_max
    # equal gradients: d_hat = d0 (1 - b1) g / ((g sqrt(1 - b2) + eps) (1 + b3)) in exact arithmetic, 1.58 d0
    st = R.State(p0, d0)
    for _ in range(2):
        R.step(st, torch.full((4,), 0.75), h)
    exact = d0 * (1 - b1) * 0.75 / ((0.75 * math.sqrt(1 - b2) + eps) * (1 + b3))
    assert st.d_hat == pytest.approx(exact, rel=1e-6) and exact / d0 == pytest.approx(1.58, abs=5e-3)


def test_zero_gradients_skip_and_lr_zero_is_a_noop():
    h = R.hyper(use_bias_correction=True)
    st = R.State(torch.tensor([0.1, 0.2]).to(BF))
    R.step(st, torch.zeros(2), h)
    assert st.skipped and st.t == 1 and st.d == 1e-6 and float(st.delta.abs().max()) == 0          # skipped, but counted
    R.step(st, torch.ones(2), R.hyper(lr=0.0))
    assert st.t == 2 and float(st.m.abs().max()) == 0 and float(st.s.abs().max()) == 0
    R.step(st, torch.ones(2), h)
    assert not st.skipped and st.t == 3 and float(st.delta.abs().min()) > 0


def no_stall_problem(seed=7, n=20000):
    """The quadratic of DESIGN §8: |p| uniform in [0.02, 0.2] with a random sign, stored as bf16; target p0 (1 + 0.3 N(0, 1))."""
    g = torch.Generator().manual_seed(seed)
    mag = 0.02 + 0.18 * torch.rand(n, generator=g)
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    p0 = (mag * sign).to(BF)
    target = p0.float() * (1 + 0.3 * torch.randn(n, generator=g))
    return p0, target


def test_d_grows_with_bf16_parameters():
    """Gradients are taken at the bf16 parameter, bf16(p0 + delta); the displacement is exact.  (Updating the bf16 parameter in place instead leaves
    x0 - x = 0, d / d0 = 1 and the distance ratio 1.)"""
    p0, target = no_stall_problem()
    st = R.State(p0)
    h = R.hyper(lr=1.0)
    dist0 = float((p0.float() - target).norm())
    ds = [st.d]
    for _ in range(400):
        R.step(st, st.param().float() - target, h)
        ds.append(st.d)
    ratio = float((st.param().float() - target).norm()) / dist0
    print(f"d / d0 = {st.d / 1e-6:.4g}, distance final / initial = {ratio:.4g}")
    assert all(b >= a for a, b in zip(ds, ds[1:]))
    assert st.d / 1e-6 > 1e3
    assert ratio < 0.05


def _arena(shapes, moments=True, seed=None):
    from tokensgen_amd import optim
    g = torch.Generator().manual_seed(seed or 0)
    params = {k: (torch.randn(*s, generator=g) * 0.1 if seed else torch.zeros(*s)).to(BF) for k, s in shapes.items()}
    return optim.ParamArena(params, optim.arena_order(list(params), 1), "cpu", moments=moments)


SHAPES = {"transformer_blocks.0.d.vip_tail": (2048 * 5 + 1,), "resampler.latents": (1, 3, 1000)}
YAML = {"learning_rate": 1.0, "adam_beta1": 0.9, "adam_beta2": 0.99, "adam_weight_decay": 1e-2, "adam_epsilon": 1e-08, "optimizer": "prodigy",
        "use_8bit_adam": False, "max_grad_norm": 1.0, "prodigy_beta3": 0.98, "prodigy_decouple": True, "prodigy_use_bias_correction": True,
        "prodigy_safeguard_warmup": True}


def test_get_optimizer_builds_prodigy_from_the_yaml_keys():
    from tokensgen_amd import optim
    arena = _arena(SHAPES)
    n_clip = arena.prefix_elems(lambda n: not n.startswith("resampler."))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        opt = optim.get_optimizer(arena, YAML, clip_elems=n_clip)
        assert not w                                                        # learning_rate 1.0, no use_8bit_adam: nothing to warn about
    assert type(opt) is optim.Prodigy and opt.KIND == "prodigy" and opt.t == 0
    assert (opt.lr, opt.betas, opt.beta3, opt.eps, opt.wd, opt.max_norm, opt.clip_elems) == (1.0, (0.9, 0.99), 0.98, 1e-8, 1e-2, 1.0, n_clip)
    assert (opt.decouple, opt.use_bias_correction, opt.safeguard_warmup) == (True, True, True)
    assert (opt.d0, opt.d_coef, opt.growth_rate) == (1e-6, 1.0, float("inf"))
    # argparse defaults: beta3 None -> sqrt(beta2), the three store_true flags off
    opt = optim.get_optimizer(_arena(SHAPES), {"optimizer": "prodigy", "learning_rate": 1.0, "adam_beta2": 0.99, "prodigy_beta3": None})
    assert opt.beta3 == math.sqrt(0.99) and (opt.decouple, opt.use_bias_correction, opt.safeguard_warmup) == (False, False, False)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        opt = optim.get_optimizer(_arena(SHAPES), dict(YAML, learning_rate=1e-4, use_8bit_adam=True))
        assert type(opt) is optim.Prodigy and opt.lr == 1e-4
        msgs = [str(x.message) for x in w]
        assert any("Learning rate is too low" in m and "around 1.0" in m for m in msgs) and any("use_8bit_adam is ignored" in m for m in msgs)
    with pytest.raises(NotImplementedError, match="'prodigy'.*needs the arena's fp32 moments"):
        optim.get_optimizer(_arena(SHAPES, moments=False), YAML)
    with pytest.raises(NotImplementedError, match="adam"):
        optim.get_optimizer(arena, dict(YAML, optimizer="adam"))


def test_prodigy_host_state_and_checkpoint_checks():
    from tokensgen_amd import lib as L, optim
    arena = _arena(SHAPES, seed=5)
    opt = optim.Prodigy(arena, lr=1.0, weight_decay=1e-2, use_bias_correction=True)
    assert opt.p0.dtype == BF and torch.equal(opt.p0, arena.param) and opt.p0.data_ptr() != arena.param.data_ptr()
    assert opt.s.dtype == opt.delta.dtype == torch.float32 and opt.s.numel() == opt.delta.numel() == arena.numel
    assert float(opt.s.abs().max()) == 0 and float(opt.delta.abs().max()) == 0
    assert opt.scalars.dtype == torch.float64 and opt.scalars.tolist() == [1e-6, 1e-6] + [0.0] * (L.PRODIGY_STATE_DOUBLES - 2)
    assert opt.stats() == {"d": 1e-6, "d_max": 1e-6, "d_numerator": 0.0, "d_hat": 0.0, "d_denom": 0.0, "dlr": 0.0}
    assert opt._ws64.numel() == L.load().tg_prodigy_ws_doubles() and opt.beta3 == math.sqrt(0.999)
    sd = opt.state_dict()
    assert {"t", "exp_avg", "exp_avg_sq", "grad", "layout", "hyper", "s", "delta", "p0", "scalars"} == set(sd)
    assert sd["hyper"]["kind"] == "prodigy" and sd["hyper"]["use_bias_correction"] is True and sd["hyper"]["d0"] == 1e-6
    # a checkpoint in the middle of a run: displacement, state and scalars set by hand; the parameters that belong to it are bf16(p0 + delta)
    g = torch.Generator().manual_seed(6)
    sd["t"] = 7
    sd["delta"] = torch.randn(arena.numel, generator=g) * 0.01 * (sd["p0"] != 0)
    sd["s"][5], sd["exp_avg"][9] = 0.25, -0.5
    sd["scalars"][:6] = torch.tensor([3e-4, 4e-4, 1e-9, 4e-4, 2.0, 5e-5], dtype=torch.float64)
    sd["hyper"]["lr"] = 0.5
    params = (sd["p0"].float() + sd["delta"]).to(BF)
    arena2 = _arena(SHAPES, seed=5)
    opt2 = optim.Prodigy(arena2, lr=1.0)
    with pytest.raises(ValueError, match=r"bf16\(p0 \+ delta\)"):
        opt2.load_state_dict(sd)                                            # the arena still holds the start values
    assert opt2.t == 0 and float(opt2.delta.abs().max()) == 0               # refused before anything was copied
    arena2.param.copy_(params)
    opt2.load_state_dict(sd)
    assert opt2.t == 7 and opt2.lr == 0.5 and opt2.wd == 1e-2 and opt2.use_bias_correction is True
    assert torch.equal(opt2.delta, sd["delta"]) and torch.equal(opt2.p0, sd["p0"]) and float(opt2.s[5]) == 0.25 and float(arena2.exp_avg[9]) == -0.5
    assert opt2.stats() == {"d": 3e-4, "d_max": 4e-4, "d_numerator": 1e-9, "d_hat": 4e-4, "d_denom": 2.0, "dlr": 5e-5}
    back = opt2.state_dict()
    assert all(torch.equal(back[k], sd[k]) for k in ("exp_avg", "exp_avg_sq", "grad", "s", "delta", "p0", "scalars")) and back["hyper"] == sd["hyper"]
    # refusals: another kind (both directions), another layout
    with pytest.raises(ValueError, match="'adamw'"):
        opt2.load_state_dict(optim.AdamW(_arena(SHAPES)).state_dict())
    with pytest.raises(ValueError, match="'adamw8bit'"):
        opt2.load_state_dict(optim.AdamW8bit(_arena(SHAPES, moments=False)).state_dict())
    with pytest.raises(ValueError, match="prodigy"):
        optim.AdamW(_arena(SHAPES)).load_state_dict(sd)
    with pytest.raises(ValueError, match="prodigy"):
        optim.AdamW8bit(_arena(SHAPES, moments=False)).load_state_dict(sd)
    other = _arena({"transformer_blocks.0.d.vip_tail": (2048 * 5 + 2,), "resampler.latents": (1, 3, 1000)})
    with pytest.raises(ValueError, match="layout"):
        optim.Prodigy(other).load_state_dict(sd)
    with pytest.raises(NotImplementedError, match="moments=True"):
        optim.Prodigy(_arena(SHAPES, moments=False))
    with pytest.raises(ValueError, match="eps"):
        optim.Prodigy(arena, eps=0.0)


def test_c_abi_validates_prodigy_arguments_before_any_launch():
    """TG_ERR_ARG (-1) for null pointers, TG_ERR_SHAPE (-2) for n <= 0, step < 1, clip_n outside [0, n] or sizes that are no multiple of 64,
    TG_ERR_ALIGN (-3) for misaligned arenas — host checks, no launch."""
    import ctypes
    from tokensgen_amd import lib as L
    lib = L.load()
    assert lib.tg_prodigy_ws_doubles() == 2 * lib.tg_grad_norm_ws_floats()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf) + (16 - ctypes.addressof(buf) % 16)

    def call(ptrs=None, n=64, clip_n=64, step=1, lr=1.0, eps=1e-8):
        ptrs = ptrs or [p] * 9
        return lib.tg_prodigy_step(*ptrs, n, clip_n, step, lr, 0.9, 0.999, 0.9995, eps, 0.0, 1e-6, 1.0, float("inf"), 1, 0, 0, None, 1, None)
    for i in range(9):
        assert call([None if j == i else p for j in range(9)]) == -1 and b"null pointer" in lib.tg_last_error_string()
    for kw in (dict(n=0), dict(n=-64), dict(step=0), dict(clip_n=-64), dict(clip_n=128), dict(n=100, clip_n=0), dict(n=128, clip_n=32), dict(lr=0.0),
               dict(eps=0.0)):
        assert call(**kw) == -2, kw
    for i in range(9):
        assert call([p + 8 if j == i else p for j in range(9)]) == -3 and b"aligned" in lib.tg_last_error_string()
