"""Plain-torch restatement of the T5 encoder (transformers T5EncoderModel: gated-gelu, no mask, no biases) for the tests; pinned to the library's own float64
run by tests/test_t5_cpu.py (fixture tests/golden/t5_tiny.pt).  Two modes:
  exact                 (rounding=False) every operation in `dtype` (float64 by default), nothing rounded;
  kernel rounding points (rounding=True)  the same arithmetic, rounded to bf16 wherever the kernels store bf16: the normalised value before the gain and the norm's
                        output, every GEMM output, P after the softmax, the attention output, the gated activation, both residual sums.  Scores and the bias stay
                        unrounded (tg_t5_attention keeps them in fp32).
`mutate` injects one semantic error (the mutation check of the GPU bound): "no_bias", "scale" (scores / 8), "swap_ff" (gelu on wi_1), "flip_distance"
(bias of i - j), "mask_pads" (keys of token id 0 masked out)."""
import math
from types import SimpleNamespace

import torch

BF16 = torch.bfloat16


def _r(t, rounding):
    return t.to(BF16).to(t.dtype) if rounding else t


def bucket(rel, num_buckets=32, max_distance=128):
    """bidirectional bucket of rel = j - i (int64 tensor): the sign picks the half, distances < 8 are exact, larger ones logarithmic up to max_distance (float32 log,
    truncation), then saturated"""
    half = num_buckets // 2
    exact = half // 2
    n = rel.abs()
    log_part = exact + (torch.log(n.float() / exact) / math.log(max_distance / exact) * (half - exact)).to(torch.long)
    log_part = torch.clamp(log_part, max=half - 1)
    return (rel > 0).long() * half + torch.where(n < exact, n, log_part)


def dense_bias(weight, S, num_buckets=32, max_distance=128, flip=False):
    """[H, S, S]: weight[bucket(j - i), h]"""
    i = torch.arange(S)[:, None]
    j = torch.arange(S)[None, :]
    rel = (i - j) if flip else (j - i)
    return weight[bucket(rel, num_buckets, max_distance).to(weight.device)].permute(2, 0, 1)


def rmsnorm(x, w, eps=1e-6, rounding=False):
    y = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    return _r(w * _r(y, rounding), rounding)


def gelu_new(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x.pow(3))))


def gated_gelu(h, rounding=False):
    F = h.shape[-1] // 2
    return _r(gelu_new(h[..., :F]) * h[..., F:], rounding)


def attention(q, k, v, bias, rounding=False, scale=1.0, key_mask=None):
    """q, k, v [B, S, H, 64], bias [H, S, S] -> [B, S, H * 64]; softmax(q k^T * scale + bias) v, P rounded in kernel-rounding mode"""
    s = torch.einsum("bihd,bjhd->bhij", q, k) * scale + bias[None]
    if key_mask is not None:
        s = s.masked_fill(~key_mask[:, None, None, :], float("-inf"))
    p = _r(torch.softmax(s, dim=-1), rounding)
    o = torch.einsum("bhij,bjhd->bihd", p, v)
    return _r(o.reshape(q.shape[0], q.shape[1], -1), rounding)


def t5_forward(sd, cfg, input_ids, dtype=torch.float64, rounding=False, mutate=None, device="cpu"):
    """sd: the library's names -> tensors (any float dtype); cfg: dict with d_model, num_heads, d_ff, num_layers, ...; returns [B, S, d_model] in `dtype`"""
    W = lambda n: sd[n].to(device=device, dtype=dtype)
    H, eps = cfg["num_heads"], cfg.get("layer_norm_epsilon", 1e-6)
    nb, md = cfg.get("relative_attention_num_buckets", 32), cfg.get("relative_attention_max_distance", 128)
    input_ids = input_ids.to(device)
    B, S = input_ids.shape
    x = W("shared.weight")[input_ids]
    bias = dense_bias(W("encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"), S, nb, md, flip=mutate == "flip_distance")
    if mutate == "no_bias":
        bias = torch.zeros_like(bias)
    key_mask = (input_ids != 0) if mutate == "mask_pads" else None
    lin = lambda t, n: _r(t @ W(n).t(), rounding)
    for i in range(cfg["num_layers"]):
        a, f = f"encoder.block.{i}.layer.0.", f"encoder.block.{i}.layer.1."
        h = rmsnorm(x, W(a + "layer_norm.weight"), eps, rounding)
        q, k, v = (lin(h, a + f"SelfAttention.{n}.weight").view(B, S, H, 64) for n in "qkv")
        o = attention(q, k, v, bias, rounding, scale=0.125 if mutate == "scale" else 1.0, key_mask=key_mask)
        x = _r(x + lin(o, a + "SelfAttention.o.weight"), rounding)
        h = rmsnorm(x, W(f + "layer_norm.weight"), eps, rounding)
        n0, n1 = ("wi_1", "wi_0") if mutate == "swap_ff" else ("wi_0", "wi_1")
        g = _r(gelu_new(lin(h, f + f"DenseReluDense.{n0}.weight")) * lin(h, f + f"DenseReluDense.{n1}.weight"), rounding)
        x = _r(x + lin(g, f + "DenseReluDense.wo.weight"), rounding)
    return rmsnorm(x, W("encoder.final_layer_norm.weight"), eps, rounding)


def t5_forward_torch_bf16(sd, cfg, input_ids, device="cpu"):
    """The torch route in bf16: the library's arithmetic with torch ops on bf16 tensors (F.linear and matmul in bf16, the norm's variance and the softmax in
    float32, the bias added to bf16 scores, gelu_new op by op in bf16).  Its error against an exact run is the yardstick of the real-width GPU test and the
    route tools/bench_t5.py times beside the kernels."""
    W = lambda n: sd[n].to(device=device, dtype=BF16)
    H, eps = cfg["num_heads"], cfg.get("layer_norm_epsilon", 1e-6)
    input_ids = input_ids.to(device)
    B, S = input_ids.shape
    x = W("shared.weight")[input_ids]
    bias = dense_bias(W("encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"), S, cfg.get("relative_attention_num_buckets", 32),
                      cfg.get("relative_attention_max_distance", 128))[None]
    norm = lambda t, w: w * (t.float() * torch.rsqrt(t.float().pow(2).mean(-1, keepdim=True) + eps)).to(BF16)
    lin = torch.nn.functional.linear
    for i in range(cfg["num_layers"]):
        a, f = f"encoder.block.{i}.layer.0.", f"encoder.block.{i}.layer.1."
        h = norm(x, W(a + "layer_norm.weight"))
        q, k, v = (lin(h, W(a + f"SelfAttention.{n}.weight")).view(B, S, H, 64).transpose(1, 2) for n in "qkv")
        s = torch.matmul(q, k.transpose(3, 2)) + bias
        p = torch.softmax(s.float(), dim=-1).to(BF16)
        o = torch.matmul(p, v).transpose(1, 2).reshape(B, S, H * 64)
        x = x + lin(o, W(a + "SelfAttention.o.weight"))
        h = norm(x, W(f + "layer_norm.weight"))
        x = x + lin(gelu_new(lin(h, W(f + "DenseReluDense.wi_0.weight"))) * lin(h, W(f + "DenseReluDense.wi_1.weight")), W(f + "DenseReluDense.wo.weight"))
    return norm(x, W("encoder.final_layer_norm.weight"))


def rel_l2(a, b):
    """|a - b| / |b| in float64"""
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


class StubTokenizer:
    """The call interface of transformers.T5Tokenizer that encode_prompt uses: a word -> one id in 2..511, EOS = 1 appended, pad = 0."""

    def __call__(self, text, padding=None, max_length=None, truncation=False, add_special_tokens=True, return_tensors=None):
        text = [text] if isinstance(text, str) else list(text)
        rows = [[2 + sum(map(ord, w)) % 510 for w in t.split()] + [1] for t in text]
        if truncation and max_length is not None:
            rows = [r if len(r) <= max_length else r[:max_length - 1] + [1] for r in rows]
        n = max_length if padding == "max_length" else max(len(r) for r in rows)
        return SimpleNamespace(input_ids=torch.tensor([r + [0] * (n - len(r)) for r in rows], dtype=torch.long))

    def batch_decode(self, ids):
        return [" ".join(str(int(i)) for i in row) for row in ids]
