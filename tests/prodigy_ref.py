"""CPU restatement of the Prodigy step that tokensgen_amd.optim.Prodigy runs on the GPU (tg_prodigy_step): prodigyopt 1.0 `Prodigy.step` in its
published form, with the two stated deviations (fp32 state and an exact fp32 displacement delta = x - x0 beside bf16 parameters; a skipped step
still counts).  Per-element arithmetic in torch fp32 in the order of the description, scalars in Python floats (fp64).  The checker of
tests/test_prodigy_*.py; written from the description, not from the product code."""
import math

import numpy as np
import torch

F32 = torch.float32
DEFAULTS = dict(lr=1.0, betas=(0.9, 0.999), beta3=None, eps=1e-8, weight_decay=0.0, decouple=True, use_bias_correction=False, safeguard_warmup=False,
                d0=1e-6, d_coef=1.0, growth_rate=float("inf"))


def hyper(**kw):
    h = dict(DEFAULTS, **kw)
    if h["beta3"] is None:
        h["beta3"] = math.sqrt(h["betas"][1])
    return h


def _t(x):
    """A Python float as the fp32 scalar the per-element arithmetic uses."""
    return torch.tensor(np.float32(x))


class State:
    """One flat vector: p0 (bf16 start values), fp32 delta / m / v / s, the fp64 scalars and the step count."""

    def __init__(self, p0, d0=1e-6):
        assert p0.dtype == torch.bfloat16
        self.p0 = p0.reshape(-1).clone()
        n = self.p0.numel()
        self.delta, self.m, self.v, self.s = (torch.zeros(n, dtype=F32) for _ in range(4))
        self.d = self.d_max = float(d0)
        self.d_numerator = self.d_hat = self.d_denom = self.dlr = 0.0
        self.skipped = False
        self.t = 0

    def x(self):
        return self.p0.to(F32) + self.delta

    def param(self):
        return self.x().to(torch.bfloat16)


def coefficients(d, t, h):
    """(dlr, a1, a2, a3) of step t (counted from 1) at the d BEFORE the step; dlr a Python float, the a's rounded to fp32."""
    b1, b2 = h["betas"]
    bc = math.sqrt(1 - b2 ** t) / (1 - b1 ** t) if h["use_bias_correction"] else 1.0
    dlr = d * h["lr"] * bc
    a1, a2 = np.float32(d * (1 - b1)), np.float32(d * d * (1 - b2))
    a3 = np.float32((d / h["d0"]) * (d if h["safeguard_warmup"] else dlr))
    return dlr, a1, a2, a3


def pass1(st, g, h, c=1.0):
    """The EMA updates of m, v, s (in place) at step st.t; returns (sum of g * (x0 - x), sum |s|, sum |g * (x0 - x)|) in fp64.
    c: the clip coefficient, a float or an fp32 tensor per element."""
    dlr, a1, a2, a3 = coefficients(st.d, st.t, h)
    b1, b2 = h["betas"]
    wd = h["weight_decay"]
    x = st.x()
    gi = (c if torch.is_tensor(c) else _t(c)) * g.reshape(-1).to(F32)
    if wd != 0 and not h["decouple"]:
        gi = gi + _t(wd) * x
    terms = gi.double() * (-st.delta).double()
    st.m = _t(b1) * st.m + _t(a1) * gi
    st.v = _t(b2) * st.v + _t(a2) * gi * gi
    st.s = _t(h["beta3"]) * st.s + _t(a3) * gi
    return float(terms.sum()), float(st.s.abs().double().sum()), float(terms.abs().sum())


def finalize(st, num_sum, den, h):
    """prodigyopt's scalar rules on the two sums; updates st's scalars unless the step is skipped (den == 0).  Returns the dlr pass 2 uses."""
    dlr = coefficients(st.d, st.t, h)[0]
    st.skipped = den == 0
    if st.skipped:
        return dlr
    d, d0 = st.d, h["d0"]
    num = h["beta3"] * st.d_numerator + (d / d0) * dlr * num_sum
    d_hat = h["d_coef"] * num / den
    if d == d0:
        d = max(d, d_hat)
    d_max = max(st.d_max, d_hat)
    d = min(d_max, d * h["growth_rate"])
    st.d, st.d_max, st.d_numerator, st.d_hat, st.d_denom, st.dlr = d, d_max, num, d_hat, den, dlr
    return dlr


def pass2(st, dlr, h, x_before):
    """delta <- delta - upd with the NEW d in the denominator and the dlr of the old one; returns upd."""
    den_i = torch.sqrt(st.v) + _t(st.d * h["eps"])
    upd = _t(dlr) * (st.m / den_i)
    if h["weight_decay"] != 0 and h["decouple"]:
        upd = upd + _t(h["weight_decay"] * dlr) * x_before
    st.delta = st.delta - upd
    return upd


def step(st, g, h, c=1.0):
    """One whole step; returns the bf16 parameter."""
    st.t += 1
    if not h["lr"] > 0:                      # prodigyopt guards the statistics with group_lr > 0; the denominator is then 0 and it returns
        return st.param()
    x = st.x()
    num_sum, den, _ = pass1(st, g, h, c)
    dlr = finalize(st, num_sum, den, h)
    if not st.skipped:
        pass2(st, dlr, h, x)
    return st.param()
