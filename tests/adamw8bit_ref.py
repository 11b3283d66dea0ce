"""CPU restatement (torch fp32) of the block-wise 8-bit AdamW that tokensgen_amd.optim.AdamW8bit runs on the GPU (tg_adamw8bit_step): the
bitsandbytes 0.44.1 AdamW8bit design (dynamic quantisation maps, one absmax per block of each tensor, fp32 moments for small tensors) with the update
arithmetic of tg_adamw_step.  The checker of tests/test_adamw8bit_*.py; written from the description, not from the product code."""
import numpy as np
import torch

F32 = torch.float32


def create_dynamic_map(signed=True, max_exponent_bits=7, total_bits=8):
    """bitsandbytes.functional.create_dynamic_map for the 8-bit optimizers' layout (7 exponent bits of 8: no extra zero-exponent items)."""
    data = []
    non_sign_bits = total_bits - 1
    for i in range(max_exponent_bits):
        fraction_items = 2 ** (i + non_sign_bits - max_exponent_bits) + 1 if signed else 2 ** (i + non_sign_bits - max_exponent_bits + 1) + 1
        boundaries = torch.linspace(0.1, 1, fraction_items)
        means = (boundaries[:-1] + boundaries[1:]) / 2.0
        data += ((10 ** (-(max_exponent_bits - 1) + i)) * means).tolist()
        if signed:
            data += (-(10 ** (-(max_exponent_bits - 1) + i)) * means).tolist()
    data.append(0)
    data.append(1.0)
    assert len(data) == 2 ** total_bits
    data.sort()
    return torch.tensor(data, dtype=F32)


def _blocks(x, block_size):
    """[n] -> [blocks, block_size] zero-padded view copy and the number of valid elements."""
    n = x.numel()
    nb = (n + block_size - 1) // block_size
    out = torch.zeros(nb * block_size, dtype=x.dtype)
    out[:n] = x.reshape(-1)
    return out.view(nb, block_size), n


def quantize_blockwise(x, qmap, block_size, signed):
    """x fp32 [n] -> (codes uint8 [n], absmax fp32 [blocks]).  absmax = max |x| over the block's elements; code = the map entry nearest to
    x * (1 / absmax) (ties to the lower code); signed: a non-zero x whose code has the other sign moves one code towards its sign; an all-zero block
    stores absmax 0 and the code of 0.0."""
    xb, n = _blocks(x.to(F32), block_size)
    absmax = xb.abs().amax(dim=1)
    inv = torch.where(absmax > 0, torch.ones_like(absmax) / absmax, torch.zeros_like(absmax))
    xn = (xb * inv[:, None]).reshape(-1)[:n]
    j = (torch.searchsorted(qmap, xn, right=True) - 1).clamp(0, 254)
    lo, hi = qmap[j], qmap[j + 1]
    code = torch.where((hi - xn) < (xn - lo), j + 1, j)
    if signed:
        xv = x.reshape(-1).to(F32)
        flip = (xv != 0) & (torch.signbit(qmap[code]) != torch.signbit(xv))
        code = torch.where(flip, code + torch.where(xv > 0, 1, -1), code)
    return code.to(torch.uint8), absmax


def dequantize_blockwise(codes, absmax, qmap, block_size):
    idx = torch.arange(codes.numel()) // block_size
    return qmap[codes.reshape(-1).long()] * absmax[idx]


def _f(x):
    return np.float32(x)


def bias_corrections(beta1, beta2, t):
    """tg_adamw_step's host-side bias corrections in fp32: bc1 = 1 - beta1^t, sqrt(1 - beta2^t)."""
    b1t = np.power(_f(beta1), _f(t), dtype=np.float32)
    b2t = np.power(_f(beta2), _f(t), dtype=np.float32)
    return _f(1) - b1t, np.sqrt(_f(1) - b2t, dtype=np.float32)


def adamw_update(p, g, m, v, t, lr, betas, eps, wd, clip=1.0):
    """The tg_adamw_step arithmetic in fp32, elementwise (torch.optim.AdamW: decoupled decay first, eps outside the corrected sqrt).
    p, g, m, v fp32 tensors; returns the new (p, m, v), p unrounded."""
    b1, b2 = _f(betas[0]), _f(betas[1])
    bc1, bc2s = bias_corrections(betas[0], betas[1], t)
    gi = g.to(F32) * torch.tensor(_f(clip))
    pi = p.to(F32) * torch.tensor(_f(1) - _f(lr) * _f(wd))
    mi = torch.tensor(b1) * m + torch.tensor(_f(1) - b1) * gi
    vi = torch.tensor(b2) * v + torch.tensor(_f(1) - b2) * gi * gi
    denom = torch.sqrt(vi) / torch.tensor(bc2s) + torch.tensor(_f(eps))
    pi = pi - torch.tensor(_f(lr) / bc1) * (mi / denom)
    return pi, mi, vi


class TensorState:
    """Optimizer state of ONE tensor: 8-bit (codes1, codes2, absmax1, absmax2) when numel >= min_8bit_size, else fp32 (m, v)."""

    def __init__(self, numel, block_size=2048, min_8bit_size=4096):
        self.block_size = block_size
        self.eight_bit = numel >= min_8bit_size
        if self.eight_bit:
            nb = (numel + block_size - 1) // block_size
            self.codes1 = torch.zeros(numel, dtype=torch.uint8)
            self.codes2 = torch.zeros(numel, dtype=torch.uint8)
            self.absmax1 = torch.zeros(nb, dtype=F32)
            self.absmax2 = torch.zeros(nb, dtype=F32)
        else:
            self.m = torch.zeros(numel, dtype=F32)
            self.v = torch.zeros(numel, dtype=F32)


QMAP1, QMAP2 = create_dynamic_map(True), create_dynamic_map(False)


def step_tensor(p, g, s, t, lr, betas, eps, wd, clip=1.0, round_bf16=True):
    """One AdamW8bit step of one tensor (flat fp32 p / g, TensorState s updated in place); returns the new parameter (bf16-rounded values in fp32 if
    round_bf16, the parameter arena's storage)."""
    if s.eight_bit:
        m = dequantize_blockwise(s.codes1, s.absmax1, QMAP1, s.block_size)
        v = dequantize_blockwise(s.codes2, s.absmax2, QMAP2, s.block_size)
    else:
        m, v = s.m, s.v
    pn, mn, vn = adamw_update(p.reshape(-1), g.reshape(-1), m, v, t, lr, betas, eps, wd, clip)
    if s.eight_bit:                                            # the parameter took the unquantised moments; now store them
        s.codes1, s.absmax1 = quantize_blockwise(mn, QMAP1, s.block_size, signed=True)
        s.codes2, s.absmax2 = quantize_blockwise(vn, QMAP2, s.block_size, signed=False)
    else:
        s.m, s.v = mn, vn
    if round_bf16:
        pn = pn.to(torch.bfloat16).to(F32)
    return pn.view(p.shape)


def step(params, grads, states, t, lr, betas, eps, wd, clip=None, round_bf16=True):
    """One step over a dict of tensors: params / grads {name: fp32 tensor}, states {name: TensorState}, clip {name: coefficient} (default 1)."""
    clip = clip or {}
    return {k: step_tensor(params[k], grads[k], states[k], t, lr, betas, eps, wd, clip.get(k, 1.0), round_bf16) for k in params}
