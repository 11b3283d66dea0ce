"""Stochastic bf16 rounding without a GPU: the Philox known answers and the properties of the rounding rule in the restatement tests/sr_ref.py, and
the host side of the switch (optim.AdamW / AdamW8bit arguments and checkpoints, optim.get_optimizer's bf16_stochastic_round key, the argument checks
of the two exports).  The kernels are held to the restatement in tests/test_sr_gpu.py."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import sr_ref as R

BF = torch.bfloat16


def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


@pytest.mark.parametrize("counter, key, want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    assert _hex(R.philox4x32_10(counter, key)) == want


def test_r16_counter_layout():
    """One Philox call serves 8 consecutive elements: element i takes half j = i & 7 of the words of group i >> 3; the seed's halves are the key, the
    step is counter word 2, the group's high half counter word 1."""
    seed, step = 0x0123456789ABCDEF, 77
    idx = np.array([0, 1, 7, 8, 70, (5 << 35) + 3], dtype=np.uint64)
    got = R.r16(seed, step, idx)
    for i, r in zip(idx.tolist(), got.tolist()):
        g, j = i >> 3, i & 7
        w = R.philox4x32_10((g & 0xFFFFFFFF, g >> 32, step, 0), (seed & 0xFFFFFFFF, seed >> 32))
        assert r == (int(w[j >> 1]) >> (16 * (j & 1))) & 0xFFFF
    assert R.r16(seed, step, idx).tolist() != R.r16(seed, step + 1, idx).tolist() != R.r16(seed + 1, step, idx).tolist()
    many = R.r16(3, 1, np.arange(1 << 16))                              # the draws are uniform 16-bit values: mean 32767.5, sd of the mean 74
    assert many.max() <= 0xFFFF and abs(float(many.mean()) - 32767.5) < 6 * 18918 / 256


ALL_R = np.arange(65536, dtype=np.uint32)


def test_sr_bf16_keeps_exact_values_and_picks_a_neighbour():
    g = np.random.default_rng(1)
    exact = (g.integers(0, 1 << 16, 4096, dtype=np.uint32) << np.uint32(16)).view(np.float32)
    exact = exact[np.isfinite(exact)]
    for r in (0, 1, 0x8000, 0xFFFF):
        assert np.array_equal(R.sr_bf16(exact, np.full(exact.shape, r)), (exact.view(np.uint32) >> 16).astype(np.uint16))
    one = np.array([1.0, -1.0, 0.0, -0.0, 2.0 ** -133], dtype=np.float32)                         # ... for every r16, zeros and a subnormal included
    for x in one:
        assert (R.sr_bf16(np.full(65536, x, dtype=np.float32), ALL_R) == (np.float32(x).view(np.uint32) >> 16)).all()
    u = g.integers(0, 1 << 32, 20000, dtype=np.uint64).astype(np.uint32)
    u = u[(u & 0x7F800000) != 0x7F800000]
    x = u.view(np.float32)
    got = R.sr_bf16(x, g.integers(0, 1 << 16, x.shape)).astype(np.uint32)
    lo = u >> 16                                                           # truncation: the neighbour towards zero; lo + 1: the one away from it
    assert (((got == lo) | (got == lo + 1))).all()
    assert (R.bf16_bits_to_f32(lo) == x)[(u & 0xFFFF) == 0].all()
    away = got == lo + 1
    assert (np.abs(R.bf16_bits_to_f32(got[away])) > np.abs(x[away])).all() and (np.abs(R.bf16_bits_to_f32(got[~away])) <= np.abs(x[~away])).all()


@pytest.mark.parametrize("sign", [0, 0x80000000])
def test_sr_bf16_rounds_away_low16_times_of_65536(sign):
    for bits in (0x3F800001, 0x3F808000, 0x3F80FFFF, 0x3F7F1234, 0x00012345, 0x7F000001, 0x3FFFC000):
        u = np.uint32(bits | sign)
        x = np.full(65536, u, dtype=np.uint32).view(np.float32)
        got = R.sr_bf16(x, ALL_R).astype(np.uint32)
        assert int((got == (u >> 16) + 1).sum()) == int(u & 0xFFFF) and int((got == (u >> 16)).sum()) == 65536 - int(u & 0xFFFF)
        mean = R.bf16_bits_to_f32(got).astype(np.float64).mean()            # hence unbiased, exactly
        assert mean == float(x[0])


def test_sr_bf16_nan_inf_and_the_largest_values():
    nan = np.array([0x7FC00000, 0x7F800001, 0xFFFFFFFF, 0x7F80FFFF], dtype=np.uint32).view(np.float32)
    inf = np.array([np.inf, -np.inf], dtype=np.float32)
    for r in (0, 1, 0x7FFF, 0xFFFF):
        assert np.isnan(R.bf16_bits_to_f32(R.sr_bf16(nan, np.full(4, r)))).all()
        assert np.array_equal(R.bf16_bits_to_f32(R.sr_bf16(inf, np.full(2, r))), inf)
    for bits in (0x7F7F0001, 0x7F7FFFFF, 0xFF7F8000):                       # above the largest bf16 (0x7f7f): never Inf, the carry is dropped
        x = np.full(65536, bits, dtype=np.uint32).view(np.float32)
        got = R.sr_bf16(x, ALL_R)
        assert (got == (bits >> 16)).all() and np.isfinite(R.bf16_bits_to_f32(got)).all()


def test_rne_restatement_is_torch():
    g = np.random.default_rng(2)
    u = g.integers(0, 1 << 32, 50000, dtype=np.uint64).astype(np.uint32)
    x = u.view(np.float32)
    x = x[~np.isnan(x)]
    assert np.array_equal(R.rne_bf16_bits(x).astype(np.int16), torch.from_numpy(x.copy()).to(BF).view(torch.int16).numpy())


# ---- host plumbing
SHAPES = {"transformer_blocks.0.a.vip_small": (40, 100), "transformer_blocks.0.d.vip_tail": (2048 * 5 + 1,), "resampler.latents": (1, 3, 1000)}


def _arena(moments):
    from tokensgen_amd import optim
    params = {k: torch.zeros(*s).to(BF) for k, s in SHAPES.items()}
    return optim.ParamArena(params, optim.arena_order(list(params), 1), "cpu", moments=moments)


@pytest.mark.parametrize("kind", ["AdamW", "AdamW8bit"])
def test_optimizer_arguments_and_checkpoint_keys(kind):
    from tokensgen_amd import optim
    cls, arena = getattr(optim, kind), _arena(kind == "AdamW")
    off = cls(arena)
    assert off.stochastic_round is False and off.sr_seed == 0
    assert off.state_dict()["hyper"]["stochastic_round"] is False and off.state_dict()["hyper"]["sr_seed"] == 0
    on = cls(arena, stochastic_round=True, sr_seed=1234)
    on.t = 9
    sd = on.state_dict()
    assert sd["hyper"]["stochastic_round"] is True and sd["hyper"]["sr_seed"] == 1234 and sd["t"] == 9
    fresh = cls(arena)
    fresh.load_state_dict(sd)
    assert fresh.stochastic_round is True and fresh.sr_seed == 1234 and fresh.t == 9       # the resumed run continues the same stream
    old = off.state_dict()
    del old["hyper"]["stochastic_round"], old["hyper"]["sr_seed"]          # a checkpoint written before the switch existed: off
    fresh.load_state_dict(old)
    assert fresh.stochastic_round is False and fresh.sr_seed == 0
    assert cls(arena, stochastic_round=True, sr_seed=-1).sr_seed == 2 ** 64 - 1 and cls(arena, sr_seed=None).sr_seed == 0


def test_get_optimizer_reads_bf16_stochastic_round_and_seed():
    from tokensgen_amd import optim
    yaml = {"learning_rate": 2e-4, "adam_beta1": 0.9, "adam_beta2": 0.95, "adam_weight_decay": 1e-4, "adam_epsilon": 1e-08, "optimizer": "adamw",
            "use_8bit_adam": True, "max_grad_norm": 1.0, "seed": 42}
    opt = optim.get_optimizer(_arena(False), yaml)
    assert type(opt) is optim.AdamW8bit and opt.stochastic_round is False                     # default off
    opt = optim.get_optimizer(_arena(False), dict(yaml, bf16_stochastic_round=True))
    assert type(opt) is optim.AdamW8bit and opt.stochastic_round is True and opt.sr_seed == 42    # the yaml's seed, no rank mixed in
    opt = optim.get_optimizer(_arena(True), dict(yaml, use_8bit_adam=False, bf16_stochastic_round=True))
    assert type(opt) is optim.AdamW and opt.stochastic_round is True and opt.sr_seed == 42
    no_seed = {k: v for k, v in yaml.items() if k != "seed"}
    assert optim.get_optimizer(_arena(False), dict(no_seed, bf16_stochastic_round=True)).sr_seed == 0

    class Args:
        pass
    args = Args()
    for k, v in dict(yaml, use_8bit_adam=False, bf16_stochastic_round=True, seed=7).items():
        setattr(args, k, v)
    opt = optim.get_optimizer(_arena(True), args)
    assert opt.stochastic_round is True and opt.sr_seed == 7
    for sr, expect in ((True, True), (False, False)):
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            opt = optim.get_optimizer(_arena(True), dict(yaml, optimizer="prodigy", use_8bit_adam=False, learning_rate=1.0, bf16_stochastic_round=sr))
            assert type(opt) is optim.Prodigy
            assert any("bf16_stochastic_round is ignored" in str(x.message) for x in w) == expect


def test_sr_exports_validate_their_arguments_without_a_launch():
    from tokensgen_amd import lib as L
    lib = L.load()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf) + (16 - ctypes.addressof(buf) % 16)
    ok = (p, p, p, p, 64, 1, 1e-3, 0.9, 0.95, 1e-8, 0.0, None, 1)
    assert lib.tg_adamw_step_sr(None, p, p, p, 64, 1, 1e-3, 0.9, 0.95, 1e-8, 0.0, None, 1, 0, 0, None) == -1
    assert lib.tg_adamw_step_sr(*ok[:5], 0, *ok[6:], 0, 0, None) == -2 and b"step must be positive" in lib.tg_last_error_string()
    for elem0 in (4, 63, -8):
        assert lib.tg_adamw_step_sr(*ok, elem0, 0, None) == -2 and b"multiple of 8" in lib.tg_last_error_string()
    assert lib.tg_adamw_step_sr(p + 2, *ok[1:], 0, 0, None) < 0 and b"16-byte aligned" in lib.tg_last_error_string()
    assert lib.tg_adamw8bit_step_sr(*([None] * 11), 1, 1, 2048, 1, 1e-3, 0.9, 0.95, 1e-8, 0.0, None, 1, 0, None) == -1
    assert b"tg_adamw8bit_step_sr: null pointer" in lib.tg_last_error_string()
    assert lib.tg_adamw8bit_step_sr(*([p] * 11), 1, 1, 300, 1, 1e-3, 0.9, 0.95, 1e-8, 0.0, None, 1, 0, None) == -2
    assert b"tg_adamw8bit_step_sr: block_size 300" in lib.tg_last_error_string()
