"""CPU: the per-element bounds of tests/train_bounds.py are satisfiable and sharp, with no measured number involved.
Satisfiable: a plain torch EMULATION of the arithmetic the kernels document — fp32 products and sums, a bf16 rounding where the kernel rounds (P, dS, ln, the bf16 outputs) —
sits at ratio <= 1 for every family, on ordinary inputs and on a peaked softmax (q, k ~ 3 randn, |lse| in the tens).
Sharp: one key's weight counted twice, the ragged last key missing from the normaliser, the scale applied twice to one dQ row, two dK rows swapped, D formed from 63 head
columns, m2 omitted in one adaLN row, the loss mask off by one frame — each FAILS (ratio > 1); and so does the largest-magnitude output moved by 2 bf16 ulps (bf16 outputs)
or by 2^-10 relative (fp32 outputs).  (The fp32 attention gradients are the one place the 2^-10 move cannot fail: their bound starts with the 2^-8 rounding of P / dS to bf16
before the MFMAs, which is 2^-8 of AT LEAST the output's own magnitude; the five structural mutations are what pins those bounds.)"""
import math

import pytest
import torch

import train_bounds as T

F32, BF = torch.float32, torch.bfloat16


def _bf(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF)


def _rb(t):
    return t.to(BF).to(F32)


def _worst(got, pair):
    return T.check(got, *pair)[0]


def _move_largest(best, ref, rel=None):
    """`best` with the largest-|ref| element moved away from the reference by 2 bf16 ulps (rel None) or by `rel` of its magnitude."""
    i = int(ref.abs().argmax())
    bad = T.d(best).clone().flatten()
    r = ref.flatten()[i]
    away = 1.0 if bad[i] >= r else -1.0
    bad[i] += away * (2 * T.ulp_bf16(bad[i]) if rel is None else rel * r.abs())
    return bad.view_as(ref)


# ------------------------------------------------------------ attention backward -----------------------------------------------------------
def _attn_inputs(peaked):
    B, H, nq, nk = 2, 2, 40, 37                              # a ragged last key tile
    s = 3.0 if peaked else 1.0
    q, k, v, g = _bf(B, nq, H * 64, seed=1, scale=s), _bf(B, nk, H * 64, seed=2, scale=s), _bf(B, nk, H * 64, seed=3), _bf(B, nq, H * 64, seed=4)
    qh, kh, vh = (T._heads(t, H) for t in (q, k, v))
    o = T._merge(torch.softmax(qh @ kh.transpose(-1, -2) * 0.125, -1) @ vh).to(BF)
    return q, k, v, o, g, H, 0.125


def _attn_emulate(q, k, v, o, g, H, scale, mutate=None):
    """fp32 emulation of attention_bwd.hip's documented arithmetic: P = exp(s - lse) and dS = P (dP - D) in fp32, each rounded to bf16 ONCE before its MFMA."""
    sp = lambda t: t.float().view(t.shape[0], t.shape[1], H, 64).transpose(1, 2)
    qh, kh, vh, oh, gh = (sp(t) for t in (q, k, v, o, g))
    s = qh @ kh.transpose(-1, -2) * scale
    lse = torch.logsumexp(s[..., :-1] if mutate == "last_key_not_in_normaliser" else s, dim=-1, keepdim=True)
    p = torch.exp(s - lse)
    if mutate == "key_counted_twice":
        p[..., 5] *= 2
    dsum = ((gh * oh)[..., :63] if mutate == "d_one_column_short" else gh * oh).sum(-1, keepdim=True)
    ds = p * (gh @ vh.transpose(-1, -2) - dsum)
    pb, dsb = _rb(p), _rb(ds)
    dv, dq, dk = pb.transpose(-1, -2) @ gh, dsb @ kh * scale, dsb.transpose(-1, -2) @ qh * scale
    if mutate == "scale_twice_on_one_dq_row":
        dq[1, 0, 33] *= scale
    if mutate == "dk_rows_swapped":
        dk[0, 1, [7, 8]] = dk[0, 1, [8, 7]]
    m = lambda t: t.transpose(1, 2).reshape(t.shape[0], t.shape[2], H * 64)
    return {"dq": m(dq), "dk": m(dk), "dv": m(dv)}


@pytest.fixture(scope="module")
def attn_refs():
    out = {}
    for peaked in (False, True):
        args = _attn_inputs(peaked)
        out[peaked] = (args, T.attention_bwd_ref(*args))
    return out


@pytest.mark.parametrize("peaked", [False, True])
def test_attention_bwd_bounds_are_satisfiable(attn_refs, peaked):
    args, ref = attn_refs[peaked]
    if peaked:
        assert float(ref["lse"].abs().max()) > 20.0
    got = _attn_emulate(*args)
    for n in ("dq", "dk", "dv"):
        assert _worst(got[n], ref[n]) <= 1.0, n
    # accumulate and the bf16 copy: one more fp32 / bf16 rounding of the same values
    pre = torch.randn(ref["dk"][0].shape, generator=torch.Generator().manual_seed(9))
    assert _worst((pre + got["dk"]), T.accumulated(*ref["dk"], pre)) <= 1.0
    assert _worst(_rb(got["dv"]), T.as_bf16(*ref["dv"])) <= 1.0


@pytest.mark.parametrize("mutate", ["key_counted_twice", "last_key_not_in_normaliser", "scale_twice_on_one_dq_row", "dk_rows_swapped", "d_one_column_short"])
@pytest.mark.parametrize("peaked", [False, True])
def test_attention_bwd_bounds_are_sharp(attn_refs, peaked, mutate):
    args, ref = attn_refs[peaked]
    got = _attn_emulate(*args, mutate=mutate)
    assert max(_worst(got[n], ref[n]) for n in ("dq", "dk", "dv")) > 1.0


def test_attention_bwd_bf16_dv_two_ulps_fail(attn_refs):
    _, ref = attn_refs[False]
    # the bf16 copy of a dv whose P weights are few (here: the reference itself): its bound is the P rounding + ONE output rounding, a 2-ulp move of the once-rounded
    # reference must lie outside wherever sum P |dO| = |dV| (no cancellation): the element with the largest |dV| / bound
    r, b = T.as_bf16(*ref["dv"])
    i = int((r.abs() / b).argmax())
    best = T.round_bf16(r.clone()).flatten()
    assert T.check(best.view_as(r), r, b)[0] <= 1.0
    best[i] += (1.0 if best[i] >= r.flatten()[i] else -1.0) * 2 * T.ulp_bf16(best[i])
    assert T.check(best.view_as(r), r, b)[0] > 1.0


# ------------------------------------------------------------ tg_adaln_modulate_bwd --------------------------------------------------------
def _adaln_inputs(add, D):
    B, Tk = 2, 9
    x, dy = _bf(B, Tk, D, seed=21, scale=2.0), _bf(B, Tk, D, seed=22)
    w, b = (1 + 0.2 * _bf(D, seed=23).float()).to(BF), _bf(D, seed=24, scale=0.2)
    sc = _bf(B, Tk, D, seed=25, scale=0.5)
    return x, dy, w, b, 1e-5, sc, (_bf(B, Tk, D, seed=26, scale=4.0) if add else None)


def _adaln_emulate(x, dy, w, b, eps, sc, add, drop_m2_row=None):
    x, dy, w, b, sc = (t.float() for t in (x, dy, w, b, sc))
    D = x.shape[-1]
    mean = x.sum(-1, keepdim=True) / D
    rstd = torch.rsqrt(((x - mean) ** 2).sum(-1, keepdim=True) / D + eps)
    xh = (x - mean) * rstd
    dln = dy * (1.0 + sc)
    dxh = dln * w
    m1, m2 = dxh.sum(-1, keepdim=True) / D, (dxh * xh).sum(-1, keepdim=True) / D
    if drop_m2_row is not None:
        m2[drop_m2_row] = 0.0
    v = rstd * (dxh - m1 - xh * m2)
    dx = _rb(v) if add is None else _rb(_rb(v) + add.float())
    return {"dx": dx, "t_dln": dln.reshape(-1, D), "t_dlnx": (dln * xh).reshape(-1, D), "t_dyln": (dy * _rb(xh * w + b)).reshape(-1, D)}


@pytest.mark.parametrize("D", [72, 3072])                  # the row sums are counted by their depth (ceil(D / 64) + 6), so the fp32 products stay sharp at the model's width
@pytest.mark.parametrize("add", [False, True])
def test_adaln_bwd_bounds_are_satisfiable_and_sharp(add, D):
    args = _adaln_inputs(add, D)
    ref = T.adaln_bwd_ref(*args)
    got = _adaln_emulate(*args)
    for n in ref:
        assert _worst(got[n], ref[n]) <= 1.0, n
        assert _worst(_move_largest(got[n], ref[n][0], None if n == "dx" else 2.0 ** -10), ref[n]) > 1.0, n
    assert _worst(_adaln_emulate(*args, drop_m2_row=(1, 4))["dx"], ref["dx"]) > 1.0


# ------------------------------------------------------------ tg_qk_layernorm_rope_bwd -----------------------------------------------------
def _qk_inputs():
    B, Tk, H = 2, 90, 3                                        # 540 rows: a full 512-row block and a 28-row one
    x = _bf(B, Tk, H * 64, seed=31, scale=1.3)
    dy = _bf(B, Tk, H * 64, seed=32).float()
    w = (1 + 0.2 * _bf(64, seed=33).float()).to(BF)
    g = torch.Generator().manual_seed(34)
    tabs = []
    for start, n in ((5, 20), (40, 30)):
        ang = torch.rand(n, 32, generator=g) * 6.28
        tabs.append((start, ang.cos().repeat_interleave(2, 1).contiguous(), ang.sin().repeat_interleave(2, 1).contiguous()))
    return x, dy, H, w, 1e-6, tabs, 0.37


def _qk_emulate(x, dy, H, w, eps, segs, out_scale):
    B, Tk, HD = x.shape
    xr, dl = x.float().view(B, Tk, H, 64), (dy * out_scale).view(B, Tk, H, 64).clone()
    src = dl.clone()
    for start, c, s in segs:
        n = c.shape[0]
        c, s = c[None, :, None, :], s[None, :, None, :]
        ya, yb = src[:, start:start + n, :, 0::2], src[:, start:start + n, :, 1::2]
        dl[:, start:start + n, :, 0::2] = ya * c[..., 0::2] + yb * s[..., 1::2]
        dl[:, start:start + n, :, 1::2] = yb * c[..., 1::2] - ya * s[..., 0::2]
    mean = xr.sum(-1, keepdim=True) / 64
    rstd = torch.rsqrt(((xr - mean) ** 2).sum(-1, keepdim=True) / 64 + eps)
    xh = (xr - mean) * rstd
    dxh = dl * w.float()
    m1, m2 = dxh.sum(-1, keepdim=True) / 64, (dxh * xh).sum(-1, keepdim=True) / 64
    dx = _rb(rstd * (dxh - m1 - xh * m2)).view(B, Tk, HD)
    rows = B * Tk * H
    nblk = (rows + 511) // 512
    blk = lambda t: torch.cat([t.reshape(rows, 64), torch.zeros(nblk * 512 - rows, 64)]).view(nblk, 512, 64).sum(1)
    return {"dx": dx, "partial": torch.stack([blk(dl * xh), blk(dl)], 1)}


def test_qk_rope_bwd_bounds_are_satisfiable_and_sharp():
    args = _qk_inputs()
    ref, got = T.qk_rope_bwd_ref(*args), _qk_emulate(*args)
    assert ref["partial"][0].shape == (2, 2, 64)
    for n in ref:
        assert _worst(got[n], ref[n]) <= 1.0, n
        assert _worst(_move_largest(got[n], ref[n][0], None if n == "dx" else 2.0 ** -10), ref[n]) > 1.0, n
    # one row's db contribution counted in the neighbouring block: the per-block comparison sees what the total cannot
    moved = got["partial"].clone()
    row = (args[1] * 0.37).view(-1, 64)[511]
    moved[0, 1] -= row; moved[1, 1] += row
    assert torch.allclose(moved.sum(0), got["partial"].sum(0), atol=1e-4) and _worst(moved, ref["partial"]) > 1.0


# ------------------------------------------------------- gate, act, colsum, loss -----------------------------------------------------------
def test_gate_residual_bwd_is_exact():
    B, Tk, D, r0 = 2, 7, 24, 3
    dout, y, gate = _bf(B, Tk, D, seed=41), _bf(B, Tk - r0, D, seed=42), _bf(B, Tk, D, seed=43, scale=0.5)
    ref = T.gate_res_bwd_ref(dout, y, gate, r0)
    got = {"dy": _rb(gate.float() * dout.float()), "t_dgate": dout.float()[:, r0:] * y.float()}
    for n in ref:
        assert _worst(got[n], ref[n]) == 0.0, n
        assert _worst(_move_largest(got[n], ref[n][0], None if n == "dy" else 2.0 ** -10), ref[n]) > 1.0, n


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_act_bounds_are_satisfiable_and_sharp(mode):
    x, dy = _bf(4099, seed=51, scale=2.5), _bf(4099, seed=52)
    ref = T.act_ref(x, dy, mode)
    xf, df = x.float(), dy.float()
    if mode == 0:
        got = xf / (1.0 + torch.exp(-xf))
    elif mode == 2:
        got = 0.5 * xf * (1.0 + torch.tanh(T.K0 * (xf + T.K1 * xf ** 3)))
    else:
        th = torch.tanh(T.K0 * (xf + T.K1 * xf ** 3))
        got = df * (0.5 * (1.0 + th) + 0.5 * xf * (1.0 - th * th) * T.K0 * (1.0 + 3.0 * T.K1 * xf * xf))
    got = _rb(got)
    assert _worst(got, ref) <= 1.0
    assert _worst(_move_largest(got, ref[0]), ref) > 1.0


def test_gelu_tanh_grad64_is_the_derivative():
    x = torch.linspace(-6, 6, 241, dtype=torch.float64).requires_grad_(True)
    T.gelu_tanh64(x).sum().backward()
    assert torch.allclose(T.gelu_tanh_grad64(x.detach()), x.grad, rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("f32", [False, True])
def test_colsum_bounds_are_satisfiable_and_sharp(f32):
    g = torch.Generator().manual_seed(61)
    m = torch.randn(300, 30, generator=g)
    m = m if f32 else m.to(BF)
    per = 128
    ref = T.colsum_ref(m, per)
    assert ref[0].shape == (3, 30)
    got = torch.stack([m[i * per:(i + 1) * per].float().sum(0) for i in range(3)])
    assert _worst(got, ref) <= 1.0
    assert _worst(_move_largest(got, ref[0], 2.0 ** -10), ref) > 1.0
    shifted = torch.stack([m[:per + 1].float().sum(0), m[per + 1:2 * per].float().sum(0), m[2 * per:].float().sum(0)])      # a block boundary off by one row
    assert _worst(shifted, ref) > 1.0
    mref = T.colsum_multi_ref([m, m[:5]], 3)                  # every item cut into 3 row blocks: 100 rows each / 2, 2, 1 rows
    cut = lambda t, per: torch.stack([t[i * per:(i + 1) * per].float().sum(0) for i in range(3)])
    assert mref[0].shape == (3, 60) and _worst(torch.cat([cut(m, 100), cut(m[:5], 2)], 1), mref) <= 1.0
    assert T.colsum_block_rows(1000, 3072) == 8 and T.colsum_block_rows(100000, 3072) == 256 and T.colsum_block_rows(1, 8) == 8


def _loss_inputs():
    B, Fr, E = 2, 3, 300
    out, noisy, tgt = (_bf(B * Fr, E, seed=s) for s in (71, 72, 73))
    acp = torch.tensor([0.9, 0.5, 0.1, 0.7, 0.3, 0.02])
    coef = torch.stack([acp.sqrt(), (1 - acp).sqrt(), 1 / (1 - acp)], 1).float()
    return out, noisy, tgt, coef, B, Fr, E


def _loss_emulate(out, noisy, tgt, coef, B, Fr, E, valid):
    sa, sb, w = _rb(coef[:, 0:1]), _rb(coef[:, 1:2]), coef[:, 2:3]
    pred = _rb(_rb(sa * noisy.float()) - _rb(sb * out.float()))
    diff = _rb(pred - tgt.float())
    term = w * _rb(diff * diff)
    vb = torch.tensor(valid).repeat_interleave(Fr).view(-1, 1)
    live = (torch.arange(Fr).repeat(B).view(-1, 1) < vb).float()
    inv = (1.0 / (vb.double() * E * B)).float()
    grad = _rb(-sb * (2.0 * w * diff * inv)) * live
    term = term * live
    return {"grad": grad, "partial": torch.cat([term, torch.zeros(B * Fr, 512 - E)], 1).view(B * Fr, 2, 256).sum(-1)}


@pytest.mark.parametrize("valid", [(3, 3), (1, 3), (3, 2)])
def test_loss_bounds_are_satisfiable_and_sharp(valid):
    out, noisy, tgt, coef, B, Fr, E = _loss_inputs()
    ref = T.vpred_loss_ref(out, noisy, tgt, coef, None, valid_frames=valid, frames=Fr)
    got = _loss_emulate(out, noisy, tgt, coef, B, Fr, E, valid)
    for n in ref:
        assert _worst(got[n], ref[n]) <= 1.0, n
        assert _worst(_move_largest(got[n], ref[n][0], None if n == "grad" else 2.0 ** -10), ref[n]) > 1.0, n
    if valid == (3, 3):        # the unmasked entry point with the matching count: the same reference
        un = T.vpred_loss_ref(out, noisy, tgt, coef, 1.0 / (Fr * E * B))
        assert torch.equal(un["grad"][0], ref["grad"][0]) and torch.equal(un["partial"][0], ref["partial"][0])
    for off in (-1, 1):         # valid_frames off by one, either way: a frame that must be exactly zero is not, or a live frame is missing (and the count differs)
        wrong = (valid[0], valid[1] + off)
        if 1 <= wrong[1] <= Fr:
            bad = _loss_emulate(out, noisy, tgt, coef, B, Fr, E, wrong)
            assert _worst(bad["grad"], ref["grad"]) > 1.0 and _worst(bad["partial"], ref["partial"]) > 1.0
