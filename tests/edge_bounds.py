"""fp64 CPU references and DERIVED per-element error bounds for the DiT inference kernels (GEMM epilogues, attention, attention lse,
tg_adaln_modulate).  A whole-tensor rel-L2 lets a few dozen elements be 100 % wrong; `check` asserts every element against a bound
that comes from the arithmetic the kernels document (number formats and accumulation lengths), never from a measured figure.
tests/test_edge_bounds_cpu.py pins that each bound is satisfiable (the once-rounded reference sits at <= 0.5) and sharp (a 2-ulp error
fails); tests/test_kernel_edges_gpu.py and tests/test_kernels_gpu.py hold the kernels to them.

All functions take CPU (or GPU) tensors of any float dtype and work in fp64 on the CPU."""
import math

import torch

LOG2E = 1.4426950408889634
F64 = torch.float64


def d(t):
    """fp64 CPU copy."""
    return t.detach().to("cpu", F64)


def round_bf16(x64):
    """fp64 -> nearest bf16 (ties to even) in ONE rounding, returned as fp64 (normal range only: no overflow / denormal handling)."""
    bits = x64.contiguous().view(torch.int64)
    drop = 52 - 7
    bits = bits + ((1 << (drop - 1)) - 1) + ((bits >> drop) & 1)
    bits = bits & ~((1 << drop) - 1)
    return bits.view(F64)


def ulp_bf16(x64):
    """Spacing of the bf16 grid at |x| (fp64)."""
    _, e = torch.frexp(x64.abs().clamp_min(2.0 ** -120))
    return torch.ldexp(torch.ones_like(x64), e - 8)


def check(got, ref64, bound):
    """(worst |got - ref| / bound, index of that element) over ALL elements; a non-finite output or a zero bound under a non-zero error
    gives inf."""
    got, ref64, bound = d(got), d(ref64), d(bound)
    assert got.shape == ref64.shape == bound.shape, (got.shape, ref64.shape, bound.shape)
    err = (got - ref64).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    ratio = torch.where(torch.isfinite(got) & torch.isfinite(ratio), ratio, torch.full_like(ratio, math.inf))
    i = int(ratio.argmax())
    return float(ratio.flatten()[i]), tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape))


# ---------------------------------------------------------------- GEMM --------------------------------------------------------------------
def gemm_ref(a, w, bias=None):
    """(A W^T + bias, |A| |W|^T + |bias|) in fp64: the linear and the magnitude sum its fp32 accumulation error scales with."""
    a, w = d(a), d(w)
    lin, mag = a @ w.T, a.abs() @ w.abs().T
    if bias is not None:
        lin, mag = lin + d(bias), mag + d(bias).abs()
    return lin, mag


def gemm_bias_bound(lin, mag, K):
    """EPI_BIAS: 2^-8 |ref| + K 2^-23 (|A||W|^T + |bias|) — the bf16 rounding of the result and the K-term fp32 accumulation bound K 2^-24 sum |a||w|
    with a factor 2.  (The first term was derived as "half an ulp <= 2^-9, times 2"; the unit roundoff of bf16 is 2^-8 — half an ulp just above a
    power of two — so it is exactly ONE rounding, with no slack: tests/test_edge_bounds_cpu.py.  Kept as derived: the stricter reading.)"""
    return 2.0 ** -8 * lin.abs() + K * 2.0 ** -23 * mag


def gemm_gate_res(lin, mag, res, gate, K, rounded_linear):
    """EPI_BIAS_GATE_RES: (ref, bound) of C = R + gate (A W^T + bias).  The issue's derivation, 2^-8 |ref| + (K + 4) 2^-23 (|R| + |g| (|A||W|^T +
    |bias|)), has one rounding of the result.  rounded_linear: the two 256 x 256 kernels (M >= 1024, N % 256 == 0) pass the linear through
    their bf16 output staging before the gate is applied — `residual + gate * bf16(linear)`, the reference's own nn.Linear output
    rounding (gemm.hip) — which that derivation missed: one more bf16 rounding of the linear, written like the first term: 2^-8 |g| |A W^T + bias|.  The 128 x 128 kernel keeps the linear in fp32 and gets no such term."""
    res, gate = d(res), d(gate)
    ref = res + gate * lin
    bound = 2.0 ** -8 * ref.abs() + (K + 4) * 2.0 ** -23 * (res.abs() + gate.abs() * mag)
    if rounded_linear:
        bound = bound + 2.0 ** -8 * gate.abs() * lin.abs()
    return ref, bound


def gelu_tanh64(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def silu64(x):
    return x / (1.0 + torch.exp(-x))


def gemm_act(pre_bits, act):
    """EPI_BIAS_GELU / _SILU = act(bf16(A W^T + bias)): (ref, bound) from the bits the same call returned with EPI_BIAS (checked per
    element by the caller).  One bf16 rounding, and the 1 + tanh / 1 / (1 + e^-x) cancellation in fp32 taken as 8 ulp of 1, times |x|."""
    x = d(pre_bits)
    ref = {"gelu": gelu_tanh64, "silu": silu64}[act](x)
    return ref, 2.0 ** -8 * ref.abs() + 2.0 ** -20 * x.abs().clamp_min(1.0)


# -------------------------------------------------------------- attention -----------------------------------------------------------------
def _heads(t, H):
    t = d(t)
    return t.reshape(t.shape[0], t.shape[1], H, 64).transpose(1, 2)           # [B, H, n, 64]


def attention_ref(segs, H, scale, k_prescaled=False):
    """segs: [(q, k, v, weight)], q [B, nq, H*64], k / v [B, nk, H*64], weight a float or a list with one entry per batch item.
    out = sum_seg w_seg softmax(scale q k^T) v per head, heads merged; k_prescaled: k already carries scale * log2(e), the scores are in
    the log2 domain as stored.  Returns (ref, bound) [B, nq, H*64]:
        bound = 2^-8 |ref| + 2^-7 sum_seg |w_seg| (p_seg |V_seg|)
    (P rounded to bf16 before the PV MFMA, 2^-9 per weight; the final bf16 rounding; factor 2.  The roundings of the two-segment epilogue —
    bf16(O1), bf16(w O2) before their sum — are each <= 2^-9 of a summand of the second term and live inside its factor 2.)"""
    ref = mag = None
    for q, k, v, w in segs:
        qh, kh, vh = _heads(q, H), _heads(k, H), _heads(v, H)
        s = qh @ kh.transpose(-1, -2) * (math.log(2.0) if k_prescaled else scale)
        p = torch.softmax(s, dim=-1)
        B = qh.shape[0]
        wt = torch.tensor([float(x) for x in w] if isinstance(w, (list, tuple)) else [float(w)] * B, dtype=F64).view(B, 1, 1, 1)
        o, m = wt * (p @ vh), wt.abs() * (p @ vh.abs())
        ref, mag = (o, m) if ref is None else (ref + o, mag + m)
    merge = lambda t: t.transpose(1, 2).reshape(t.shape[0], t.shape[2], H * 64)
    ref, mag = merge(ref), merge(mag)
    return ref, 2.0 ** -8 * ref.abs() + 2.0 ** -7 * mag


def attention_lse_ref(q, k, H, scale):
    """tg_attention_fwd_lse: log2 sum_j exp2(scale log2(e) q.k_j) per row, fp32 [B, H, nq]; bound 2^-17 (1 + max_j sum_d |q_d||k_jd| scale log2 e)."""
    qh, kh = _heads(q, H), _heads(k, H)
    c = scale * LOG2E
    ref = torch.logsumexp(qh @ kh.transpose(-1, -2) * (c * math.log(2.0)), dim=-1) / math.log(2.0)
    mag = (qh.abs() @ kh.abs().transpose(-1, -2)).amax(dim=-1) * c
    return ref, 2.0 ** -17 * (1.0 + mag)


# ------------------------------------------------------------ tg_adaln_modulate ------------------------------------------------------------
def adaln_ref(x, w, b, eps, scale=None, shift=None):
    """The kernel's documented two roundings: ln = bf16(LayerNorm(x) w + b), y = ln (1 + scale) + shift (scale / shift [B, T, D] gathered by
    the caller; None: plain affine LayerNorm).  bound = 2^-8 |ref| + 2^-8 |1 + scale| |ln| + dim 2^-22 |ref|."""
    x = d(x)
    D = x.shape[-1]
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    ln = round_bf16((x - mu) / torch.sqrt(var + eps) * d(w) + d(b))
    one_s = torch.ones_like(ln) if scale is None else 1.0 + d(scale)
    ref = ln * one_s + (0.0 if shift is None else d(shift))
    return ref, 2.0 ** -8 * ref.abs() + 2.0 ** -8 * one_s.abs() * ln.abs() + D * 2.0 ** -22 * ref.abs()
