"""GPU: stochastic bf16 rounding of the parameter write of optim.AdamW / optim.AdamW8bit (tg_adamw_step_sr / tg_adamw8bit_step_sr) against the numpy
restatement tests/sr_ref.py.  The exact test makes the fp32 value before the rounding known in closed form (zero gradient and moments: x = p * 31/32,
an exact fp32 product), so every parameter must carry the restatement's bits: that pins the counter layout, the index arithmetic across tensors,
segments and tails, and the rounding.  Then the invariances (seed, two-segment launch, checkpoint / resume, the switch off), the edge values, and
the test that shows the point: a parameter at 1.0 under lr 2e-4 never moves with round-to-nearest and follows the fp32 trajectory with the switch on."""
import numpy as np
import pytest
import torch

import sr_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
KINDS = [("AdamW", None), ("AdamW8bit", 2048), ("AdamW8bit", 256)]
IDS = ["adamw", "adamw8bit-2048", "adamw8bit-256"]

# ~2^20 elements: below min_8bit_size (fp32 moments in AdamW8bit) and a multiple of 8; 4097 (no multiple of 8, a 1-element tail block); 70 elements;
# 5 blocks of 2048 + 1; one large tensor of odd sides; the unclipped Resampler rest
SHAPES = {"transformer_blocks.0.a.vip_small": (40, 100), "transformer_blocks.0.b.vip_odd": (4097,), "transformer_blocks.0.c.vip_seventy": (70,),
          "transformer_blocks.0.d.vip_tail": (2048 * 5 + 1,), "transformer_blocks.0.e.vip_large": (1021, 997), "resampler.proj.weight": (4097,),
          "resampler.proj.bias": (300,)}
EXACT = dict(lr=2.0 ** -3, weight_decay=2.0 ** -2, max_grad_norm=None)      # zero gradient: x = p * (1 - 2^-5), nothing else


def _random_bf16(shape, gen):
    """Normal-range bf16 values of both signs, exponents 2^-20 .. 2^20, all 7 mantissa bits random."""
    n = int(np.prod(shape))
    bits = (gen.integers(0, 2, n) << 15) | (gen.integers(127 - 20, 127 + 21, n) << 7) | gen.integers(0, 128, n)
    return torch.from_numpy(bits.astype(np.uint16).view(np.int16)).view(BF).reshape(shape)


def _make(kind, block_size, shapes=SHAPES, params=None, seed=0, **kw):
    from tokensgen_amd import optim
    if params is None:
        gen = np.random.default_rng(seed)
        params = {k: _random_bf16(s, gen) for k, s in shapes.items()}
    arena = optim.ParamArena({k: v.to(DEV) for k, v in params.items()}, optim.arena_order(list(params), 1), DEV, moments=kind == "AdamW")
    if kind == "AdamW8bit":
        kw["block_size"] = block_size
    return arena, getattr(optim, kind)(arena, **kw), params


def _bits(t):
    return t.detach().cpu().view(torch.int16).numpy().view(np.uint16)


def _inside(arena):
    m = torch.zeros(arena.numel, dtype=torch.bool, device=DEV)
    for n in arena.names:
        m[arena.offsets[n]:arena.offsets[n] + arena.views[n].numel()] = True
    return m


def _set_grads(arena, inside, step, scale=1e-3):
    g = torch.Generator(device=DEV).manual_seed(1000 + step)
    arena.grad.normal_(generator=g).mul_(scale).mul_(inside)                # inside the tensors only: the padding stays zero


def _state(arena, opt):
    extra = [arena.exp_avg, arena.exp_avg_sq] if arena.exp_avg is not None else [opt.state1, opt.state2, opt.absmax1, opt.absmax2, opt.small_m, opt.small_v]
    return [t.clone() for t in [arena.param] + extra]


def _same(a, b):
    return all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))


@pytest.mark.parametrize("kind, block_size", KINDS, ids=IDS)
def test_every_parameter_carries_the_restatement_bits(kind, block_size):
    seed, t0 = 0x9E3779B97F4A7C15, 41
    arena, opt, _ = _make(kind, block_size, stochastic_round=True, sr_seed=seed, **EXACT)
    assert arena.numel > 1_000_000 and any(arena.views[n].numel() % 8 for n in arena.names)
    if kind == "AdamW8bit":
        assert {r.kind for r in opt.rows} == {0, 1} and max(r.blocks for r in opt.rows) > 1
    before = _bits(arena.param)
    opt.t = t0                                                               # the step number enters the counter: not step 1
    opt.step()
    torch.cuda.synchronize()
    x = R.bf16_bits_to_f32(before) * np.float32(31.0 / 32.0)                  # exact: an 8-bit by a 5-bit significand
    assert np.array_equal((x.astype(np.float64)), R.bf16_bits_to_f32(before).astype(np.float64) * (31.0 / 32.0))
    want = R.sr_bf16(x, R.r16(seed, t0 + 1, np.arange(arena.numel)))
    got = _bits(arena.param)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad.size, bad[:8], got[bad[:8]], want[bad[:8]])
    inside = _inside(arena).cpu().numpy()
    assert (got[~inside] == 0).all()                                         # arena padding stays zero
    # the test is not vacuous: x lies 2 to 4 bf16 spacings below p, so every value moves; 31 m has 12 or 13 bits, so 15 of 16 values are no bf16 and
    # their fraction f is a multiple of 1/32: the stochastic result differs from round-to-nearest with probability E[min(f, 1 - f)] = 1/4
    assert (got != before)[inside].all()
    assert 0.15 < (got != R.rne_bf16_bits(x))[inside].mean() < 0.35


def test_adamw_sr_segment_with_a_tail_at_an_arena_offset():
    """tg_adamw_step_sr itself on n = 8 * 1000 + 5 elements at arena index 8 * 123: the last group is partial (optim.AdamW never gets there, its
    arenas are padded to 64); nothing past n is written in any of the four buffers."""
    from tokensgen_amd import kernels as K, lib as L
    n, pad, elem0, seed, step = 8 * 1000 + 5, 64, 8 * 123, 77, 3
    gen = np.random.default_rng(5)
    p = _random_bf16((n + pad,), gen).to(DEV)
    g, m, v = (torch.zeros(n + pad, dtype=torch.float32, device=DEV) for _ in range(3))
    g[n:], m[n:], v[n:] = 3.0, 5.0, 7.0                                       # sentinels
    before = _bits(p)
    L.check(L.load().tg_adamw_step_sr(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, step, 2.0 ** -3, 0.9, 0.95, 1e-8, 2.0 ** -2, None, 1,
                                      elem0, seed, K._stream()), "tg_adamw_step_sr")
    torch.cuda.synchronize()
    x = R.bf16_bits_to_f32(before[:n]) * np.float32(31.0 / 32.0)
    assert np.array_equal(_bits(p)[:n], R.sr_bf16(x, R.r16(seed, step, elem0 + np.arange(n))))
    assert np.array_equal(_bits(p)[n:], before[n:])
    assert bool((g[n:] == 3.0).all()) and bool((m[n:] == 5.0).all()) and bool((v[n:] == 7.0).all())
    assert float(g[:n].abs().max()) == 0 and float(m[:n].abs().max()) == 0 and float(v[:n].abs().max()) == 0


def _run(kind, block_size, steps, params=None, resume_at=None, **kw):
    arena, opt, params = _make(kind, block_size, params=params, seed=3, **kw)
    inside = _inside(arena)
    for s in range(steps):
        if s == resume_at:                                                   # checkpoint -> a fresh default-constructed optimizer on a fresh arena
            sd, now = opt.state_dict(), {n: arena.views[n].clone() for n in arena.names}
            kw2 = {k: v for k, v in kw.items() if k not in ("stochastic_round", "sr_seed")}
            arena, opt, _ = _make(kind, block_size, params=now, **kw2)
            assert opt.stochastic_round is False
            opt.load_state_dict(sd)
            assert opt.stochastic_round is True and opt.t == s
        _set_grads(arena, inside, s)
        opt.step()
    torch.cuda.synchronize()
    return _state(arena, opt), params


HYPER = dict(lr=3e-3, weight_decay=1e-2)


@pytest.mark.parametrize("kind, block_size", KINDS[:2], ids=IDS[:2])
def test_same_seed_same_bits_other_seed_other_bits(kind, block_size):
    a, params = _run(kind, block_size, 2, stochastic_round=True, sr_seed=11, **HYPER)
    b, _ = _run(kind, block_size, 2, params=params, stochastic_round=True, sr_seed=11, **HYPER)
    c, _ = _run(kind, block_size, 2, params=params, stochastic_round=True, sr_seed=12, **HYPER)
    d, _ = _run(kind, block_size, 2, params=params, stochastic_round=True, sr_seed=11 + (1 << 32), **HYPER)     # the seed's high half is key word 1
    assert _same(a, b)
    assert (a[0] != c[0]).float().mean().item() > 0.2 and (a[0] != d[0]).float().mean().item() > 0.2


def test_two_segment_launch_does_not_change_the_stream():
    """AdamW steps [0, clip_elems) and [clip_elems, numel) in two launches; without clipping the split must not show, in any bit."""
    kw = dict(stochastic_round=True, sr_seed=5, max_grad_norm=None, **HYPER)
    whole, params = _run("AdamW", None, 2, **kw)
    arena, _, _ = _make("AdamW", None, params=params)
    cut = arena.offsets["transformer_blocks.0.e.vip_large"] + 64 * 1001       # inside a tensor, a multiple of 64
    assert 0 < cut < arena.numel and cut % 64 == 0
    split, _ = _run("AdamW", None, 2, params=params, clip_elems=cut, **kw)
    assert _same(whole, split)


@pytest.mark.parametrize("kind, block_size", KINDS[:2], ids=IDS[:2])
def test_checkpoint_resume_continues_the_same_stream(kind, block_size):
    kw = dict(stochastic_round=True, sr_seed=21, **HYPER)
    straight, params = _run(kind, block_size, 6, **kw)
    resumed, _ = _run(kind, block_size, 6, params=params, resume_at=3, **kw)
    assert _same(straight, resumed)


@pytest.mark.parametrize("kind, block_size", KINDS[:2], ids=IDS[:2])
def test_zero_learning_rate_and_switch_off(kind, block_size):
    arena, opt, params = _make(kind, block_size, seed=4, stochastic_round=True, sr_seed=9, lr=0.0, weight_decay=0.0)
    start = arena.param.clone()
    _set_grads(arena, _inside(arena), 0)
    opt.step()
    torch.cuda.synchronize()
    assert torch.equal(arena.param.view(torch.int16), start.view(torch.int16))         # a bf16-exact value is never changed
    off, _ = _run(kind, block_size, 2, params=params, stochastic_round=False, sr_seed=9, **HYPER)
    default, _ = _run(kind, block_size, 2, params=params, **HYPER)
    on, _ = _run(kind, block_size, 2, params=params, stochastic_round=True, sr_seed=9, **HYPER)
    assert _same(off, default) and not torch.equal(on[0].view(torch.int16), default[0].view(torch.int16))


BIG = float(torch.finfo(BF).max)


@pytest.mark.parametrize("kind, block_size", KINDS[:2], ids=IDS[:2])
def test_edge_values(kind, block_size):
    special = torch.tensor([float("nan"), float("inf"), float("-inf"), 0.0, -0.0, 1.0, -1.0, BIG, -BIG] * 8, dtype=torch.float32)
    params = {"transformer_blocks.0.a.vip_special": special.to(BF),
              "transformer_blocks.0.b.vip_max": torch.cat([torch.full((32768,), BIG), torch.full((32768,), -BIG)]).to(BF),
              "transformer_blocks.0.c.vip_plain": torch.ones(5000).to(BF)}
    # weight decay -2^-7 at lr 2^-3: the factor is 1 + 2^-10, so the largest bf16 grows to a finite fp32 whose upper neighbour would be Inf
    arena, opt, _ = _make(kind, block_size, params=params, stochastic_round=True, sr_seed=1, lr=2.0 ** -3, weight_decay=-(2.0 ** -7), max_grad_norm=None)
    seed, before = 1, _bits(arena.param)
    opt.step()
    torch.cuda.synchronize()
    got = arena.views["transformer_blocks.0.a.vip_special"].float().cpu()
    assert bool(got[0::9].isnan().all()) and bool((got[1::9] == float("inf")).all()) and bool((got[2::9] == float("-inf")).all())
    zeros = _bits(arena.views["transformer_blocks.0.a.vip_special"])
    assert (zeros[3::9] == 0).all() and (zeros[4::9] == 0x8000).all()                      # +0 stays +0, -0 stays -0
    big = arena.views["transformer_blocks.0.b.vip_max"]
    assert big.numel() == 65536 and bool(torch.isfinite(big.float()).all())
    assert (_bits(big)[:32768] == 0x7F7F).all() and (_bits(big)[32768:] == 0xFF7F).all()  # no carry into Inf, for any of the draws
    x = R.bf16_bits_to_f32(before) * np.float32(1.0 + 2.0 ** -10)
    want = R.sr_bf16(x, R.r16(seed, 1, np.arange(arena.numel)))
    finite = np.isfinite(x)
    assert np.array_equal(_bits(arena.param)[finite], want[finite]) and (want != before)[finite].any()
    # a NaN gradient poisons its own element and no other
    name = "transformer_blocks.0.c.vip_plain"
    arena.grad_view(name)[1234] = float("nan")
    opt.step()
    torch.cuda.synchronize()
    plain = arena.views[name].float().cpu()
    assert bool(plain[1234].isnan()) and int(plain.isnan().sum()) == 1
    assert bool(torch.isfinite(arena.views["transformer_blocks.0.b.vip_max"].float()).all())


@pytest.mark.parametrize("kind, block_size", KINDS[:2], ids=IDS[:2])
def test_round_to_nearest_stalls_and_stochastic_rounding_follows_fp32(kind, block_size, parity):
    """4096 parameters at 1.0, gradient 1.0 every step, lr 2e-4, 200 steps: the fp32 trajectory ends at 0.96 (|m^ / sqrt(v^)| = 1).  Next to 1.0 the
    bf16 spacing below is 2^-8 = 19.5 lr: round-to-nearest writes 1.0 back every time.  Stochastically each element steps down 2^-8 with
    probability q = lr / 2^-8 = 0.0512: per-element sd 2^-8 sqrt(200 q (1 - q)) = 0.0122, sd of the mean of 4096 elements 1.9e-4; 1.2e-3 is 6 sigma.
    (With a constant gradient the 8-bit moments of a block all equal its absmax and quantise exactly: the same trajectory.)"""
    means = {}
    for sr in (False, True):
        arena, opt, _ = _make(kind, block_size, params={"transformer_blocks.0.a.vip_w": torch.ones(4096).to(BF)}, stochastic_round=sr, sr_seed=2024,
                              lr=2e-4, weight_decay=0.0, max_grad_norm=None, betas=(0.9, 0.95))
        assert arena.numel == 4096
        for _ in range(200):
            arena.grad.fill_(1.0)
            opt.step()
        torch.cuda.synchronize()
        means[sr] = float(arena.param.double().mean())
        if not sr:
            assert bool((arena.param == 1.0).all())                          # the stall itself
        else:
            spread = float(arena.param.double().std())
            assert 0.5 * 0.0122 < spread < 2 * 0.0122, spread
    print(f"{kind}: mean parameter after 200 steps: round-to-nearest {means[False]:.6f}, stochastic {means[True]:.6f} (fp32: 0.96)")
    parity(abs(means[True] - 0.96), 1.2e-3, f"{kind} stochastic rounding: |mean parameter - 0.96| after 200 steps (mean {means[True]:.6f}; "
                                            f"round-to-nearest: {means[False]:.6f})")
