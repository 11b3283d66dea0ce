"""CPU: the per-element bounds of tests/edge_bounds.py are satisfiable and sharp, with no measured number involved.
For each bound family
  - the fp64 reference rounded ONCE to the output format (the best a correct kernel can do) passes.  The unit roundoff of bf16 (8 significant
    bits) is 2^-8: half an ulp is up to 2^-8 |x| just above a power of two, not 2^-9, so the 2^-8 |ref| term of every bound is exactly ONE
    rounding and the once-rounded reference reaches ratios up to 1 where the other terms are small (GEMM: 0.98), not <= 0.5; the bounds are
    kept as derived (the stricter reading) and the ceiling asserted here is 1;
  - the same tensor with its single largest-magnitude element moved by 2 bf16 ulps (away from the reference) fails;
and for the attention family the same tensor with one key column's weight counted twice fails."""
import pytest
import torch

import edge_bounds as E

F64 = torch.float64


def _bf(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16)


def _gemm_inputs():
    a, w, bias = _bf(2, 37, 192, seed=1), _bf(128, 192, seed=2, scale=0.1), _bf(128, seed=3)
    return a, w, bias, E.gemm_ref(a, w, bias)


def _family_gemm_bias():
    a, w, bias, (lin, mag) = _gemm_inputs()
    return lin, E.gemm_bias_bound(lin, mag, 192)


def _family_gemm_gate_res(rounded):
    a, w, bias, (lin, mag) = _gemm_inputs()
    res, gate = _bf(2, 37, 128, seed=4), _bf(2, 37, 128, seed=5, scale=0.5)
    return E.gemm_gate_res(lin, mag, res, gate, 192, rounded_linear=rounded)


def _family_gemm_act(act):
    a, w, bias, (lin, mag) = _gemm_inputs()
    return E.gemm_act(E.round_bf16(lin), act)


def _attn_inputs():
    """Two segments, B = 2, H = 2, nq = 40, nk = (70, 7), per-item weights.  V > 0 and the values scaled so that the largest output is
    ~1.06: the attention bound legitimately allows ~1.5 x 2^-7 of relative error where sum |w| p |V| = |ref|, and more where the sum
    cancels, so a 2-ulp move (2^-6 / mantissa, relative) is outside it only for a small mantissa and no cancellation."""
    H = 2
    q1, k1, q2, k2 = (_bf(2, n, H * 64, seed=s) for n, s in ((40, 11), (70, 12), (40, 13), (7, 14)))
    v1, v2 = _bf(2, 70, H * 64, seed=15).abs() + 0.25, _bf(2, 7, H * 64, seed=16).abs() + 0.25
    wts = [0.6015625, 0.25]
    ref, _ = E.attention_ref([(q1, k1, v1, 1.0), (q2, k2, v2, wts)], H, 0.125)
    c = 1.06 / float(ref.abs().max())
    v1, v2 = (v1.double() * c).to(torch.bfloat16), (v2.double() * c).to(torch.bfloat16)
    return (q1, k1, v1, 1.0), (q2, k2, v2, wts), H


def _family_attention():
    s1, s2, H = _attn_inputs()
    return E.attention_ref([s1, s2], H, 0.125)


def _family_adaln(modulate):
    x = _bf(2, 9, 72, seed=21, scale=2.0)
    w, b = _bf(72, seed=22, scale=0.1).double() + 1, _bf(72, seed=23, scale=0.1)
    sc, sh = (_bf(2, 9, 72, seed=24, scale=0.5), _bf(2, 9, 72, seed=25, scale=0.5)) if modulate else (None, None)
    return E.adaln_ref(x, w, b, 1e-5, sc, sh)


FAMILIES = {
    "gemm_bias": _family_gemm_bias,
    "gemm_gate_res": lambda: _family_gemm_gate_res(False),
    "gemm_gate_res_rounded_linear": lambda: _family_gemm_gate_res(True),
    "gemm_gelu": lambda: _family_gemm_act("gelu"),
    "gemm_silu": lambda: _family_gemm_act("silu"),
    "attention": _family_attention,
    "adaln_modulate": lambda: _family_adaln(True),
    "adaln_plain": lambda: _family_adaln(False),
}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_bound_is_satisfiable_and_sharp(family):
    ref, bound = FAMILIES[family]()
    best = E.round_bf16(ref)
    worst, _ = E.check(best, ref, bound)
    assert worst <= 1.0, worst
    i = int(ref.abs().argmax())
    bad = best.clone().flatten()
    away = 1.0 if bad[i] >= ref.flatten()[i] else -1.0
    bad[i] += away * 2 * E.ulp_bf16(bad[i])
    worst, where = E.check(bad.view_as(ref), ref, bound)
    assert worst > 1.0, worst
    assert where == tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ref.shape))


def test_lse_bound_is_satisfiable_and_sharp():
    q, k = _bf(2, 40, 128, seed=31), _bf(2, 70, 128, seed=32)
    ref, bound = E.attention_lse_ref(q, k, 2, 0.125)
    best = ref.float().double()                              # the lse output is fp32
    assert E.check(best, ref, bound)[0] <= 0.5
    i = int(ref.abs().argmax())
    bad = best.clone().flatten()
    bad[i] += 2 * E.ulp_bf16(bad[i])
    assert E.check(bad.view_as(ref), ref, bound)[0] > 1.0


def test_attention_key_column_counted_twice_fails():
    """The masked-tail error the whole-tensor norm averages away: key column j of the 7-key second segment enters the numerator twice."""
    (q1, k1, v1, w1), (q2, k2, v2, w2), H = _attn_inputs()
    ref, bound = E.attention_ref([(q1, k1, v1, w1), (q2, k2, v2, w2)], H, 0.125)
    j = 6
    extra, _ = E.attention_ref([(q2, k2[:, j:j + 1], v2[:, j:j + 1], w2)], H, 0.125)       # softmax over one key = 1: w v_j per row ...
    qh, kh = E._heads(q2, H), E._heads(k2, H)
    p = torch.softmax(qh @ kh.transpose(-1, -2) * 0.125, dim=-1)[..., j]                    # ... times the weight key j has in the row
    pj = p.transpose(1, 2).repeat_interleave(64, dim=2)
    bad = E.round_bf16(ref + pj * extra)
    assert E.check(E.round_bf16(ref), ref, bound)[0] <= 1.0
    assert E.check(bad, ref, bound)[0] > 1.0


def test_round_bf16_is_one_rounding_to_nearest_even():
    x = torch.tensor([1.0, 1.00390625, 1.001953125, 1.005859375, -3.1415926, 2.0 ** -20 * 1.7, 255.5, 1.0 + 2.0 ** -8 + 2.0 ** -40], dtype=F64)
    want = torch.tensor([1.0, 1.0, 1.0, 1.0078125, -3.140625, 2.0 ** -20 * 1.703125, 256.0, 1.0078125], dtype=F64)
    assert torch.equal(E.round_bf16(x), want)
    assert torch.equal(E.round_bf16(x[4:5]).float().to(torch.bfloat16).double(), E.round_bf16(x[4:5]))
    assert torch.equal(E.ulp_bf16(torch.tensor([1.0, 1.99, 2.0, 0.75], dtype=F64)), torch.tensor([2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8], dtype=F64))
