"""GPU: LoRA on the DiT attention projections — the two kernels (tg_lora_wgrad, tg_lora_merge) against float64 torch on the same bf16 inputs, the training
path (train.To2VBlockTrainer / To2VTrainer / To2VTrainStep with an adapter) against fp32 autograd of tests/lora_ref.py wrapped around the oracle's block, and
fused inference (CogVideoXTransformer3DModel.fuse_lora) against the oracle on weights W + s B A.

Bounds that are measured, not derived, live in profiles/lora_parity.json (figure measured on the MI355X; the test asserts 2x that figure, the convention
of test_train_gpu.py).  Figures recorded there:
  wgrad_real_*: rel-L2 of tg_lora_wgrad at M = 35 552, N = 3072 — ceiling 4e-3 (what the bf16-output weight gradient is held to); this kernel keeps fp32.
  block_* / width_*: the tiny and the full-width block with a NON-zero adapter (class of the un-adapted block: outputs 6e-3, input gradients 7e-3,
  parameter gradients 2e-2 tiny; 1e-2 / 1.3e-2 / 3.5e-2 full width)."""
import json
import os

import numpy as np
import pytest
import torch

import lora_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = dict(rank=128, lora_alpha=64, target_modules=["to_k", "to_q", "to_v", "to_out.0"])


def _tol(name):
    with open(os.path.join(ROOT, "profiles", "lora_parity.json")) as f:
        return 2.0 * float(json.load(f)["figures"][name]["measured"])


def _rel(a, b):
    a, b = a.double(), b.double().to(a.device)
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _rand(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF)


# ------------------------------------------------------------------------------------------------------------------------ kernels
def _wgrad_case(M, N, R, seed, strided, transposed, beta, batch=1):
    from tokensgen_amd import kernels as K
    wide = _rand(batch, M, N + 64, seed=seed).to(DEV) if strided else None
    y = wide[:, :, 32:32 + N] if strided else _rand(batch, M, N, seed=seed).to(DEV)                # a column slice of a wider buffer (16-byte aligned)
    t = _rand(batch, M, R, seed=seed + 1).to(DEV)
    g0 = torch.randn(R, N, generator=torch.Generator().manual_seed(seed + 2)).to(DEV) if transposed else \
        torch.randn(N, R, generator=torch.Generator().manual_seed(seed + 2)).to(DEV)
    out = g0.clone() if beta else torch.full_like(g0, float("nan"))                                # beta = 0 must not read G
    if batch == 1:
        y, t = y[0], t[0]
    K.lora_wgrad(y, t, out, scale=0.37, beta=beta, transposed=transposed)
    want = 0.37 * (y.reshape(-1, N).double().T @ t.reshape(-1, R).double())
    want = (want.T if transposed else want) + beta * g0.double()
    return out, want


@pytest.mark.parametrize("M", [1, 63, 1000])
@pytest.mark.parametrize("R", [64, 128, 384])
def test_lora_wgrad_small_ragged_shapes_vs_float64(M, R, parity):
    for i, (strided, transposed, beta, batch) in enumerate(((False, False, 0.0, 1), (True, True, 1.0, 1), (True, False, 1.0, 2), (False, True, 0.0, 2))):
        out, want = _wgrad_case(M, 192, R, 100 + 10 * i + M, strided, transposed, beta, batch)
        assert torch.isfinite(out).all()
        # fp32 accumulation of exact bf16 x bf16 products over at most 2000 rows: far inside 1e-5 (sqrt(2000) * 2^-24 ~ 3e-6)
        parity(_rel(out, want), 1e-5, f"tg_lora_wgrad M={M} R={R} strided={strided} transposed={transposed} beta={beta} batch={batch}")


@pytest.mark.parametrize("R", [128, 384])
def test_lora_wgrad_real_shape_vs_float64_and_deterministic(R, parity):
    from tokensgen_amd import kernels as K
    M, N = 17776, 3072                                           # batch 2 x 17 776 = 35 552 token rows
    y, t = _rand(2, M, N, seed=7, scale=0.5).to(DEV), _rand(2, M, R, seed=8, scale=0.5).to(DEV)
    out = torch.empty(R, N, dtype=torch.float32, device=DEV)
    K.lora_wgrad(y, t, out, scale=0.5, transposed=True)
    want = torch.empty(R, N, dtype=torch.float64, device=DEV)
    for c0 in range(0, N, 512):                                  # float64 in column panels (the whole Y in float64 would be 1.7 GB)
        want[:, c0:c0 + 512] = 0.5 * (t.reshape(-1, R).double().T @ y.reshape(-1, N)[:, c0:c0 + 512].double())
    tol = _tol(f"wgrad_real_R{R}")
    assert tol < 4e-3, "the fp32 kernel must stay below the bound of the bf16-output weight gradient (test_train_gpu.py)"
    print(f"tg_lora_wgrad real shape R={R}: rel-L2 {_rel(out, want):.3e} (tol {tol:.1e})")
    parity(_rel(out, want), tol, f"tg_lora_wgrad M=35552 N=3072 R={R} vs float64")
    again = torch.full_like(out, -1.0)
    K.lora_wgrad(y, t, again, scale=0.5, transposed=True)
    assert torch.equal(again, out)                               # same inputs, same bits
    flat = torch.empty(N, R, dtype=torch.float32, device=DEV)    # the other output layout, the batch folded into M: the same numbers
    K.lora_wgrad(y.view(2 * M, N), t.view(2 * M, R), flat, scale=0.5)
    assert torch.equal(flat.T, out)


def _ulp_apart(got, want64):
    """True where bf16 `got` is the correctly rounded float64 value or one of its two bf16 neighbours."""
    r = want64.to(torch.float32).to(BF)                          # (float64 -> float32 -> bf16 double rounding moves the result by at most one more neighbour
    gi, ri = got.view(torch.int16).to(torch.int32), r.view(torch.int16).to(torch.int32)      # only on exact ties; covered by the neighbour allowance)
    key = lambda v: torch.where(v < 0, -(v & 0x7fff), v)         # sign-magnitude -> ordered integers
    return (key(gi) - key(ri)).abs() <= 1


@pytest.mark.parametrize("N,K_,R", [(128, 128, 128), (3072, 3072, 128), (200, 136, 16)])
def test_lora_merge_one_rounding_in_place_and_zero_scale(N, K_, R):
    from tokensgen_amd import kernels as K
    store = _rand(3 * N, K_ + 8, seed=21, scale=0.05).to(DEV)    # W is a strided view of a larger storage, like the fused QKV weight
    w = store[N:2 * N, :K_]
    b, a = _rand(N, R, seed=22, scale=0.1).to(DEV), _rand(R, K_, seed=23, scale=0.1).to(DEV)
    before = store.clone()
    out = torch.empty(N, K_, dtype=BF, device=DEV)
    K.lora_merge(w, b, a, 0.5, out=out)
    want = w.double() + 0.5 * (b.double() @ a.double())
    assert _ulp_apart(out, want).all()
    assert (out != want.float().to(BF)).float().mean().item() < 1e-3          # a neighbour only at a tie of the two-step rounding
    assert torch.equal(store, before)                                         # out of place: W untouched
    zero = torch.empty(N, K_, dtype=BF, device=DEV)
    K.lora_merge(w, b, a, 0.0, out=zero)
    assert torch.equal(zero.view(torch.int16), w.view(torch.int16))           # scale 0: W's own bits
    K.lora_merge(w, b, a, 0.5)                                                # in place == out of place, and nothing outside the view moves
    assert torch.equal(w, out)
    after = store.clone()
    after[N:2 * N, :K_] = before[N:2 * N, :K_]
    assert torch.equal(after, before)


# ------------------------------------------------------------------------------------------------------------------------ one block
def _block_case(B, H, Nt, Fr, hw_grid, Np_grid, te, std, seed, vip_scale, ref_dev):
    """The block of test_train_gpu.py's block tests with a NON-zero adapter: fp32 autograd through the oracle block on W + s B A, and the HIP trainer."""
    from oracle import dit_ref as O
    from tokensgen_amd import lora, train
    f32 = np.float32
    gh, gw = hw_grid
    hw, Np = gh * gw, Np_grid[0] * Np_grid[1] * Np_grid[2]
    Nv, D = Fr * hw, H * 64
    cfg = dict(num_attention_heads=H, attention_head_dim=64, num_layers=1, patch_size=2, time_embed_dim=te, text_embed_dim=64, in_channels=16, out_channels=16)
    pre = "transformer_blocks.0"
    lcfg = lora.LoraConfig.from_params(YAML)
    sd = {k: v.to(BF).float().to(ref_dev) for k, v in O.make_state_dict(cfg, n_vip_dim=128, seed=seed, std=std).items() if k.startswith(pre + ".")}
    ad = {k: v.float().to(ref_dev).requires_grad_(True) for k, v in R.random_adapter(sd, lcfg.rank, seed + 1, b_std=std).items()}
    assert len(ad) == 8
    vip_keys = [k for k in sd if "vip_" in k]
    for k in vip_keys:
        sd[k] = sd[k].clone().requires_grad_(True)
    hidden, enc, temb = _rand(B, Nv, D, seed=seed + 2).to(ref_dev), _rand(B, Nt + Np, D, seed=seed + 3).to(ref_dev), _rand(B, Fr, te, seed=seed + 4).to(ref_dev)
    rope = O.rope_3d(64, np.arange(Fr, dtype=f32), np.arange(gh, dtype=f32), np.arange(gw, dtype=f32))
    vrope = O.rope_3d(64, np.arange(Fr, dtype=f32) + f32(3), np.arange(gh, dtype=f32), np.arange(gw, dtype=f32))
    crope = O.rope_3d(64, np.linspace(1000, 1016.25, Np_grid[0], dtype=f32), np.arange(Np_grid[1], dtype=f32), np.arange(Np_grid[2], dtype=f32))
    dev = lambda r: tuple(t.to(ref_dev) for t in r)
    hf, ef = hidden.float().requires_grad_(True), enc.float().requires_grad_(True)
    oh, oe = O.block_forward(R.with_lora(sd, ad, lcfg.scaling), pre, hf, ef, temb.float(), H, Np, [vip_scale], dev(rope), dev(vrope), dev(crope))
    Gh, Ge = _rand(B, Nv, D, seed=seed + 5).to(ref_dev), _rand(B, Nt + Np, D, seed=seed + 6).to(ref_dev)
    ((oh * Gh.float()).sum() + (oe * Ge.float()).sum()).backward()
    sd_dev = {k: v.detach().to(BF).to(DEV).contiguous() for k, v in list(sd.items()) + list(ad.items())}
    blk = train.To2VBlockTrainer(sd_dev, pre, H, Nt, Np, Fr, vip_scale, lora=lcfg)
    gh_, ge_ = blk.forward(hidden.to(DEV), enc.to(DEV), temb.to(DEV), rope, vrope, crope)
    grads, dh, de = blk.backward(Gh.to(DEV), Ge.to(DEV))
    assert set(pre + "." + k for k in grads) == set(vip_keys) | set(ad)
    want = {k: v.grad for k, v in ad.items()}
    want.update({k: sd[k].grad for k in vip_keys})
    fig = dict(out=max(_rel(gh_, oh.detach()), _rel(ge_, oe.detach())), dinput=max(_rel(dh, hf.grad), _rel(de, ef.grad)),
               dlora=max(_rel(grads[k[len(pre) + 1:]], want[k]) for k in ad), dvip=max(_rel(grads[k[len(pre) + 1:]], want[k]) for k in vip_keys))
    worst = {k: _rel(grads[k[len(pre) + 1:]], want[k]) for k in ad}
    print("adapter gradients, rel-L2:", {k[len(pre) + 7:]: f"{v:.2e}" for k, v in worst.items()})
    assert all(float(want[k].abs().max()) > 0 for k in ad)        # B != 0: every adapter gradient carries signal
    return fig


def test_block_with_adapter_vs_fp32_autograd_of_the_oracle_block(parity):
    fig = _block_case(2, 2, 9, 4, (5, 6), (5, 2, 3), 128, 0.08, 181, 0.6, "cpu")
    for name in ("out", "dinput", "dlora", "dvip"):
        print(f"block_{name}: {fig[name]:.3e}")
        parity(fig[name], _tol("block_" + name), f"tiny block with a rank-128 adapter, {name}: HIP vs fp32 autograd (lora_ref around the oracle block)")


def test_full_width_block_with_adapter_vs_fp32_autograd(parity):
    fig = _block_case(1, 48, 16, 2, (12, 16), (4, 4, 4), 512, 0.02, 211, 1.0, DEV)
    for name in ("out", "dinput", "dlora", "dvip"):
        print(f"width_{name}: {fig[name]:.3e}")
        parity(fig[name], _tol("width_" + name), f"full-width block with a rank-128 adapter, {name}: HIP vs fp32 autograd")


# ------------------------------------------------------------------------------------------------------------------------ the trainer
CFG2 = dict(num_attention_heads=2, attention_head_dim=64, num_layers=2, patch_size=2, time_embed_dim=128, text_embed_dim=64, in_channels=16, out_channels=16)


def _model_case(seed, B=1):
    from oracle import dit_ref as O
    from oracle import scheduler_ref as S
    f32 = np.float32
    Nt, Fr, Hh, Ww = 9, 4, 10, 12
    sd = {k: v.to(BF).to(DEV).contiguous() for k, v in O.make_state_dict(CFG2, n_vip_dim=128, seed=seed, std=0.08).items()}
    g = torch.Generator().manual_seed(seed + 1)
    x0, noise = (torch.randn(B, Fr, 16, Hh, Ww, generator=g).to(BF).to(DEV) for _ in range(2))
    text, vip = _rand(B, Nt, 64, seed=seed + 2).to(DEV), _rand(B, 5, 128, 2, 3, seed=seed + 3).to(DEV)
    ts = torch.tensor([[500, 520, 480, 510]] * B)
    rope = O.rope_3d(64, np.arange(4, dtype=f32), np.arange(5, dtype=f32), np.arange(6, dtype=f32))
    vrope = O.rope_3d(64, np.arange(4, dtype=f32) + f32(3), np.arange(5, dtype=f32), np.arange(6, dtype=f32))
    crope = O.rope_3d(64, np.linspace(1000, 1016.25, 5, dtype=f32), np.arange(2, dtype=f32), np.arange(3, dtype=f32))
    ac = torch.as_tensor(S.alphas_cumprod()[1], dtype=torch.float32)
    return sd, dict(x0=x0, noise=noise, text=text, vip=vip, ts=ts, ropes=(rope, vrope, crope), ac=ac)


def _fwd_bwd(tr, c):
    from tokensgen_amd import train
    out = tr.forward(c["noise"], c["text"], c["ts"], c["vip"], *c["ropes"])
    _, _, d_out = train.vpred_loss_and_grad(out, c["noise"], c["x0"], c["ts"], c["ac"])
    grads, d_vip = tr.backward(d_out)
    return out, grads, d_vip


def test_no_adapter_and_zero_b_adapter_equal_the_plain_trainer_and_frozen_adapter_gets_no_gradient():
    from tokensgen_amd import lora, train
    sd, c = _model_case(301, B=2)
    lcfg = lora.LoraConfig.from_params(YAML)
    plain = train.To2VTrainer(dict(sd), 2, 2, vip_scale=0.7)
    out0, g0, dv0 = _fwd_bwd(plain, c)
    fresh = {k: v.to(DEV) for k, v in lora.init_adapter(lcfg, sd, torch.Generator().manual_seed(5)).items()}          # B = 0
    ignored = train.To2VTrainer({**sd, **fresh}, 2, 2, vip_scale=0.7)                  # lora=None: adapter entries of the state dict are not even looked at
    assert ignored.trainable == plain.trainable
    tr = train.To2VTrainer({**sd, **fresh}, 2, 2, vip_scale=0.7, lora=lcfg)
    assert tr.trainable == sorted(plain.trainable + sorted(fresh))
    out1, g1, dv1 = _fwd_bwd(tr, c)
    assert torch.equal(out1, out0) and torch.equal(dv1, dv0)
    assert sorted(g1) == tr.trainable and all(torch.equal(g1[k], g0[k]) for k in plain.trainable)
    assert all(not g1[k].any() for k in fresh if k.endswith("lora_A.weight"))          # dA = s dT^T x with dT = dy B = 0
    assert all(g1[k].abs().max().item() > 0 for k in fresh if k.endswith("lora_B.weight"))
    # a frozen adapter (is_trainable: false): applied in the forward, absent from `trainable`, from the gradients and from the arena
    ad = {k: v.to(DEV) for k, v in R.random_adapter({k: v.cpu() for k, v in sd.items()}, 128, 9, b_std=0.08).items()}
    live = train.To2VTrainer({**sd, **ad}, 2, 2, vip_scale=0.7, lora=lcfg)
    frozen = train.To2VTrainer({**sd, **ad}, 2, 2, vip_scale=0.7, lora=lora.LoraConfig.from_params(dict(YAML, is_trainable=False)))
    assert frozen.trainable == plain.trainable
    out_l, g_l, dv_l = _fwd_bwd(live, c)
    out_f, g_f, dv_f = _fwd_bwd(frozen, c)
    assert not torch.equal(out_l, out0)                                                # the adapter acts ...
    assert torch.equal(out_f, out_l) and torch.equal(dv_f, dv_l)                       # ... the same whether it trains or not
    assert sorted(g_f) == plain.trainable and all(torch.equal(g_f[k], g_l[k]) for k in plain.trainable)


def test_recompute_schedule_equals_kept_schedule_bitwise_with_an_adapter():
    from tokensgen_amd import lora, train
    sd, c = _model_case(311, B=2)
    ad = {k: v.to(DEV) for k, v in R.random_adapter({k: v.cpu() for k, v in sd.items()}, 128, 10, b_std=0.08).items()}
    tr = train.To2VTrainer({**sd, **ad}, 2, 2, vip_scale=0.7, lora=lora.LoraConfig.from_params(YAML))
    out, g, dv = _fwd_bwd(tr, c)
    assert tr.blocks_kept == 2
    tr.activation_budget_bytes = 0
    out0, g0, dv0 = _fwd_bwd(tr, c)
    assert tr.blocks_kept == 0
    assert torch.equal(out0, out) and torch.equal(dv0, dv) and sorted(g0) == sorted(g) and all(torch.equal(g0[k], g[k]) for k in g)


def test_train_step_window_with_adamw8bit_resume_and_save_load(tmp_path):
    from tokensgen_amd import lora, optim, train
    lcfg = lora.LoraConfig.from_params(YAML)
    sd, c = _model_case(321)
    ad = {k: v.to(DEV) for k, v in R.random_adapter({k: v.cpu() for k, v in sd.items()}, 128, 11, b_std=0.08).items()}

    def build(params=None):
        s = {k: v.clone() for k, v in {**sd, **ad}.items()}
        tr = train.To2VTrainer(s, 2, 2, vip_scale=1.0, lora=lcfg)
        arena = optim.ParamArena({k: (s[k] if params is None else params[k]) for k in tr.trainable}, optim.arena_order(tr.trainable, 2), DEV, moments=False)
        tr.use_arena(arena)
        opt = optim.get_optimizer(arena, dict(optimizer="adamw", use_8bit_adam=True, learning_rate=2e-3))
        return s, tr, arena, opt, train.To2VTrainStep(tr, arena, opt, c["ac"], accumulation_steps=2)

    micro = lambda st: st.micro_step(c["x0"], c["noise"], c["ts"], c["text"], c["vip"], *c["ropes"])
    s, tr, arena, opt, step = build()
    assert type(opt).__name__ == "AdamW8bit" and set(arena.names) == set(tr.trainable) and all(k in arena.views for k in ad)
    a3 = [arena.views[f"transformer_blocks.1.attn1.to_{n}.lora_A.weight"] for n in "qkv"]
    assert tr._blocks is None
    before = {k: arena.views[k].clone() for k in tr.trainable}
    # the adapter gradients are added into the arena by tg_lora_wgrad itself: after the first micro-step they are there, scaled by 1 / accumulation steps
    _, did = micro(step)
    assert not did and tr._blocks[1].lA3.data_ptr() == a3[0].data_ptr()                # the [3r, D] projection is a VIEW of the arena
    ref = train.To2VTrainer({k: v.clone() for k, v in {**sd, **ad}.items()}, 2, 2, vip_scale=1.0, lora=lcfg)
    noisy = step.add_noise(c["x0"], c["noise"], c["ts"]).contiguous()
    out = ref.forward(noisy, c["text"], c["ts"], c["vip"], *c["ropes"])
    _, _, d_out = train.vpred_loss_and_grad(out, noisy, c["x0"], c["ts"], c["ac"])
    g_ref, _ = ref.backward(d_out)
    for k in ad:
        want = 0.5 * g_ref[k]
        assert (arena.grad_view(k) - want).abs().max().item() <= 1e-6 * max(1.0, want.abs().max().item()), k
    _, did = micro(step)
    assert did and opt.t == 1
    for k in ad:
        assert not torch.equal(arena.views[k], before[k]), k                           # every adapter tensor moved
    for k, v in sd.items():
        if k not in tr.trainable:
            assert torch.equal(s[k], v), k                                             # the frozen base did not
    # resume in the middle of the next window
    micro(step)
    state, params = step.state_dict(), {k: arena.views[k].clone() for k in tr.trainable}
    micro(step)
    assert opt.t == 2
    s2, tr2, arena2, opt2, step2 = build(params)
    step2.load_state_dict(state)
    micro(step2)
    assert opt2.t == 2 and torch.equal(arena2.param, arena.param)
    # save -> load returns what the arena holds
    tr.save_lora_weights(str(tmp_path))
    back = lora.load_lora_weights(str(tmp_path), lcfg)
    assert sorted(back) == sorted(ad) and all(torch.equal(back[k].to(DEV), arena.views[k]) for k in ad)


# ------------------------------------------------------------------------------------------------------------------------ fused inference
def _fused_oracle_sd(sd, ad, s):
    """Weights W + s B A formed in fp32, then rounded once to bf16 (what fuse_lora on a bf16 model holds)."""
    merged = R.with_lora({k: v.float() for k, v in sd.items()}, {k: v.float() for k, v in ad.items()}, s)
    return {k: v.to(BF) for k, v in merged.items()}


def test_fuse_lora_to2v_model_vs_oracle_and_unfuse_restores_bitwise(tmp_path):
    from oracle import dit_ref as O
    from test_dit_gpu import _build, _tiny_inputs, _tiny_ropes
    from tokensgen_amd import lora
    cfg = dict(num_attention_heads=2, attention_head_dim=64, num_layers=2, patch_size=2, time_embed_dim=128, text_embed_dim=64, in_channels=16, out_channels=16)
    vipcfg = dict(length=30, func_type="1", scale=[0.6], resampler_params=dict(output_dim=128, num_height_queries=2, num_width_queries=3, num_temporal_queries=4))
    sd = {k: v.to(BF) for k, v in O.make_state_dict(cfg, n_vip_dim=128, seed=31).items()}
    m = _build(cfg, vipcfg, sd)
    lcfg = lora.LoraConfig.from_params(YAML)
    ad = R.random_adapter(sd, 128, 32, b_std=0.4)              # strong enough that its effect stands far above the parity error
    inp = _tiny_inputs(33)
    rope, vrope, crope = _tiny_ropes(t0=2.0)
    run = lambda: m(inp["hs"].to(DEV, BF), inp["enc"].to(DEV, BF), inp["ts"].to(DEV), vip_encoder_hidden_states=inp["vip"].to(DEV, BF), image_rotary_emb=rope,
                    vip_image_rotary_emb=vrope, vip_condition_rotary_emb=crope, return_dict=False)[0]
    base_out = run()
    base_w = {k: v.detach().clone() for k, v in m.state_dict().items()}
    lora.save_lora_weights(str(tmp_path), ad)
    assert lora.apply_from_config(m, dict(use_lora=True, lora_path=str(tmp_path), lora_params=YAML))      # the infer yaml's keys
    with pytest.raises(RuntimeError, match="already fused"):
        m.fuse_lora(ad, lcfg)
    y = run()
    want = O.dit_forward(_fused_oracle_sd(sd, ad, lcfg.scaling), cfg, inp["hs"].to(BF), inp["enc"].to(BF), inp["ts"], inp["vip"].to(BF), rope, vrope, crope, vip_scale=[0.6])
    print(f"fused To2V model: rel-L2 to the oracle {_rel(y, want):.3e}, effect of the adapter {_rel(y, base_out):.3e}")
    assert _rel(y, want) < 8.5e-3                                # the bound of test_dit_gpu.py for the un-adapted tiny model
    assert _rel(y, base_out) > 3 * 8.5e-3                        # and the adapter's effect is resolved: a model that ignored it would fail the line above
    changed = [k for k, v in m.state_dict().items() if not torch.equal(v, base_w[k])]
    assert sorted(changed) == sorted(k + ".weight" for k in R.target_modules(sd.keys()))
    m.unfuse_lora()
    assert all(torch.equal(v, base_w[k]) for k, v in m.state_dict().items())
    assert torch.equal(run(), base_out)
    with pytest.raises(RuntimeError, match="no adapter"):
        m.unfuse_lora()
    m.fuse_lora(ad, lcfg, lora_scale=0.0)                        # lora_scale multiplies s: 0 leaves every weight as it was
    assert all(torch.equal(v, base_w[k]) for k, v in m.state_dict().items())


def test_fuse_lora_plain_patch1_model_vs_oracle(golden_dir):
    from oracle import dit_ref as O
    from oracle import t2to_ref as T
    from test_t2to_gpu import _gold, _model
    from tokensgen_amd import lora
    g = _gold(golden_dir)
    m, sd = _model(g)
    sd = {k: v.to(BF) for k, v in sd.items()}
    c = g["cases"]["torch.bfloat16"]
    F_, H, W = g["nfc"] * g["chunks"], g["H"], g["W"]
    x, emb, t = torch.cat([c["init_latents"]] * 2), torch.cat([c["negative"], c["prompt"]]), torch.tensor([999, 999])
    rope = T.rope_tables(64, F_, H, W)
    lcfg = lora.LoraConfig(rank=16, lora_alpha=32)               # a rank the training path does not take: fusing has no granule
    ad = R.random_adapter(sd, 16, 42, b_std=0.4)
    run = lambda: m(x.to(DEV), emb.to(DEV), t.to(DEV), image_rotary_emb=rope, return_dict=False)[0]
    base_out = run()
    m.fuse_lora(ad, lcfg)
    got = run()
    want = O.dit_forward(_fused_oracle_sd(sd, ad, lcfg.scaling), g["cfg"], x, emb, t, image_rotary_emb=rope)
    print(f"fused patch-1 model: rel-L2 to the oracle {_rel(got, want):.3e}, effect of the adapter {_rel(got, base_out):.3e}")
    assert _rel(got, want) < 8.5e-3 and _rel(got, base_out) > 3 * 8.5e-3
    m.unfuse_lora()
    assert torch.equal(run(), base_out)
