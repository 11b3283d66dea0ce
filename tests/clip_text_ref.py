"""Plain-torch restatement of the CLIP text tower (transformers CLIPTextModelWithProjection) and of the text-video alignment formula, for the tests; pinned to the
library's own float64 run by tests/test_clip_text_cpu.py (fixture tests/golden/clip_text_tiny.pt, tools/make_clip_text_golden.py).  Two modes, as tests/vit_ref.py:
  exact                  (rounding=False) every operation in `dtype` (float64 by default), nothing rounded;
  kernel rounding points (rounding=True)  the same arithmetic, rounded to bf16 wherever the kernels store bf16: the embedding sum (through fp32 first: the kernel
                         adds in fp32), every GEMM output, every LayerNorm output, P after the softmax, the attention output, the activation, both residual sums.
                         Scores stay unrounded (tg_t5_attention keeps them in fp32).
State dicts carry the library's names.  There is NO padding mask anywhere: attention is causal and the pooled row sees only itself and earlier tokens.
`mutate` injects one semantic error (the mutation check of the whole-model bound): "no_causal" (every key visible), "pool_last" (the row at S - 1), "other_pool" (the
other one of the library's two pooling rules), "no_scale" (scores not divided by 8), "pos_shift" (position rows rotated by one), "tanh_gelu" (the tanh form in
place of the quick one), "no_final_ln" (final_layer_norm dropped), "proj_transposed" (text_projection applied transposed)."""
import torch

from vit_ref import BF16, _r, act, layernorm, rel_l2  # noqa: F401  (rel_l2 is re-exported for the tests)

MUTATIONS = ("no_causal", "pool_last", "other_pool", "no_scale", "pos_shift", "tanh_gelu", "no_final_ln", "proj_transposed")


def pooled_positions(ids, eos_token_id):
    """The library's two rules (modeling_clip.py, CLIPTextTransformer.forward): eos_token_id == 2 -> argmax of the ids; else the first position holding eos_token_id"""
    if eos_token_id == 2:
        return ids.int().argmax(dim=-1)
    return (ids.int() == eos_token_id).int().argmax(dim=-1)


def embed(ids, tok, pos, rounding=False):
    """ids [B, S], tok [V, D], pos [P, D] -> [B, S, D].  Rounding goes through fp32 as the kernel's sum does."""
    x = tok[ids] + pos[:ids.shape[1]][None]
    return x.float().to(BF16).to(tok.dtype) if rounding else x


def causal_attention(q, k, v, scale=0.125, rounding=False, causal=True):
    """q, k, v [B, S, H, 64] -> [B, S, H * 64]: softmax(q k^T * scale + causal mask) v, P and the output rounded in kernel-rounding mode"""
    s = torch.einsum("bihd,bjhd->bhij", q, k) * scale
    if causal:
        S = q.shape[1]
        s = s.masked_fill(torch.ones(S, S, dtype=torch.bool, device=q.device).triu(1), float("-inf"))
    p = _r(torch.softmax(s, dim=-1), rounding)
    o = torch.einsum("bhij,bjhd->bihd", p, v)
    return _r(o.reshape(q.shape[0], q.shape[1], -1), rounding)


def clip_text_forward(sd, cfg, ids, dtype=torch.float64, rounding=False, mutate=None, device="cpu"):
    """sd: library names -> tensors; cfg: dict with num_attention_heads, num_hidden_layers, hidden_act, layer_norm_eps, eos_token_id; ids [B, S] integers;
    returns text_embeds [B, projection_dim] in `dtype`"""
    W = lambda n: sd[n].to(device=device, dtype=dtype)
    H, eps, L, eos = cfg["num_attention_heads"], cfg["layer_norm_eps"], cfg["num_hidden_layers"], cfg["eos_token_id"]
    mode = "tanh_gelu" if mutate == "tanh_gelu" else cfg["hidden_act"]
    ids = ids.to(device).long()
    B, S = ids.shape
    lin = lambda t, n, bias=True: _r(t @ W(n + ".weight").t() + (W(n + ".bias") if bias else 0.0), rounding)
    pos = W("text_model.embeddings.position_embedding.weight")
    if mutate == "pos_shift":
        pos = torch.roll(pos, 1, 0)
    x = embed(ids, W("text_model.embeddings.token_embedding.weight"), pos, rounding)
    for i in range(L):
        e = f"text_model.encoder.layers.{i}."
        h = layernorm(x, W(e + "layer_norm1.weight"), W(e + "layer_norm1.bias"), eps, rounding)
        q, k, v = (lin(h, e + f"self_attn.{n}_proj").view(B, S, H, 64) for n in "qkv")
        a = causal_attention(q, k, v, 1.0 if mutate == "no_scale" else 0.125, rounding, causal=mutate != "no_causal")
        x = _r(x + lin(a, e + "self_attn.out_proj"), rounding)
        h = layernorm(x, W(e + "layer_norm2.weight"), W(e + "layer_norm2.bias"), eps, rounding)
        x = _r(x + lin(act(lin(h, e + "mlp.fc1"), mode, rounding), e + "mlp.fc2"), rounding)
    if mutate != "no_final_ln":
        x = layernorm(x, W("text_model.final_layer_norm.weight"), W("text_model.final_layer_norm.bias"), eps, rounding)
    if mutate == "pool_last":
        at = torch.full((B,), S - 1, dtype=torch.long, device=device)
    elif mutate == "other_pool":                                          # eos_token_id 2 selects the argmax rule; cfg["other_eos_token_id"] is the end token's real id
        at = pooled_positions(ids, cfg["other_eos_token_id"] if eos == 2 else 2).long()
    else:
        at = pooled_positions(ids, eos).long()
    c = x[torch.arange(B, device=device), at]
    w = W("text_projection.weight")
    return _r(c @ (w if mutate == "proj_transposed" else w.t()), rounding)


def clip_text_forward_torch_bf16(sd, cfg, ids, device="cpu"):
    """The torch route in bf16: the library's arithmetic with torch ops on bf16 tensors (F.embedding, F.linear, F.layer_norm, matmul in bf16; the masked softmax in
    float32).  Its error against an exact run is the yardstick beside the real-width GPU test."""
    import torch.nn.functional as Fn
    W = lambda n: sd[n].to(device=device, dtype=BF16)
    H, eps, L = cfg["num_attention_heads"], cfg["layer_norm_eps"], cfg["num_hidden_layers"]
    ids = ids.to(device).long()
    B, S = ids.shape
    x = Fn.embedding(ids, W("text_model.embeddings.token_embedding.weight")) + W("text_model.embeddings.position_embedding.weight")[:S][None]
    D = x.shape[-1]
    ln = lambda t, n: Fn.layer_norm(t, (D,), W(n + "weight"), W(n + "bias"), eps)
    mask = torch.zeros(S, S, device=device).masked_fill(torch.ones(S, S, dtype=torch.bool, device=device).triu(1), float("-inf"))
    for i in range(L):
        e = f"text_model.encoder.layers.{i}."
        h = ln(x, e + "layer_norm1.")
        q, k, v = (Fn.linear(h, W(e + f"self_attn.{n}_proj.weight"), W(e + f"self_attn.{n}_proj.bias")).view(B, S, H, 64).transpose(1, 2) for n in "qkv")
        pr = torch.softmax((torch.matmul(q, k.transpose(3, 2)) * 0.125).float() + mask, dim=-1).to(BF16)
        a = torch.matmul(pr, v).transpose(1, 2).reshape(B, S, D)
        x = x + Fn.linear(a, W(e + "self_attn.out_proj.weight"), W(e + "self_attn.out_proj.bias"))
        h = Fn.linear(ln(x, e + "layer_norm2."), W(e + "mlp.fc1.weight"), W(e + "mlp.fc1.bias"))
        h = Fn.gelu(h) if cfg["hidden_act"] == "gelu" else h * torch.sigmoid(1.702 * h)
        x = x + Fn.linear(h, W(e + "mlp.fc2.weight"), W(e + "mlp.fc2.bias"))
    x = ln(x, "text_model.final_layer_norm.")
    c = x[torch.arange(B, device=device), pooled_positions(ids, cfg["eos_token_id"]).long()]
    return Fn.linear(c, W("text_projection.weight"))


class StubTokenizer:
    """stands in for the caller's transformers.CLIPTokenizer (no vocabulary files ship): records how it is called and hands back the ids and mask it was built with"""

    def __init__(self, ids, mask):
        self.ids, self.mask, self.calls = ids, mask, []

    def __call__(self, prompts, **kw):
        self.calls.append((prompts, kw))
        return {"input_ids": self.ids[:len(prompts)], "attention_mask": self.mask[:len(prompts)]}


def alignment(img, txt):
    """img [F, D], txt [K, D] -> (cos [F, K], per_text [K], score) in float64: cos(x, y) = x . y / (max(|x|, 1e-8) max(|y|, 1e-8)), F.cosine_similarity's definition
    (a zero row gives 0); per_text = the mean over frames of max(0, cos); score = mean(per_text)"""
    x, y = img.double(), txt.double()
    cos = (x @ y.t()) / (x.norm(dim=-1).clamp_min(1e-8)[:, None] * y.norm(dim=-1).clamp_min(1e-8)[None])
    per_text = cos.clamp_min(0.0).mean(dim=0)
    return cos, per_text, per_text.mean()
