"""Plain-torch restatement of the two ViT image encoders (transformers ViTModel without pooler, CLIPVisionModelWithProjection) and of the frame-consistency
formula, for the tests; pinned to the library's own float64 run by tests/test_vit_cpu.py (fixture tests/golden/vit_tiny.pt, tools/make_vit_golden.py).  Two modes:
  exact                  (rounding=False) every operation in `dtype` (float64 by default), nothing rounded;
  kernel rounding points (rounding=True)  the same arithmetic, rounded to bf16 wherever the kernels store bf16: the preprocessed pixel (through fp32 first: the kernel
                         forms it with one fp32 fused multiply-add of fp32 constants), every GEMM output, the assembled tokens, every LayerNorm output, P after the
                         softmax, the attention output, the activation, both residual sums.  Scores stay unrounded (tg_t5_attention keeps them in fp32).
State dicts carry the in-memory names of transformers 5.x.  `mutate` injects one semantic error (the mutation check of the whole-model bound): "no_scale" (scores
not divided by 8), "tanh_gelu" (the tanh form in place of the exact or the quick one), "no_pre_ln" (pre_layrnorm dropped; CLIP only), "pos_shift" (position rows
rotated by one), "cls_norm" (the class token taken on the other side of the final norm: not normalised)."""
import math

import torch

BF16 = torch.bfloat16
MEAN_STD = {"vit": ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)),
            "clip": ((0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711))}
MUTATIONS = {"vit": ("no_scale", "tanh_gelu", "pos_shift", "cls_norm"), "clip": ("no_scale", "tanh_gelu", "no_pre_ln", "pos_shift", "cls_norm")}


def _r(t, rounding):
    return t.to(BF16).to(t.dtype) if rounding else t


def rel_l2(a, b):
    """|a - b| / |b| in float64"""
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def fold(mean, std):
    """a, b of `x * a + b == ((x + 1) / 2 - mean) / std`, as the fp32 values the kernel receives (float64 tensors holding them)"""
    a = torch.tensor([0.5 / s for s in std], dtype=torch.float32).double()
    b = torch.tensor([(0.5 - m) / s for m, s in zip(mean, std)], dtype=torch.float32).double()
    return a, b


def preprocess(frames, mean, std, rounding=False):
    """frames [F, 3, H, W] in [-1, 1] -> normalised pixels.  Exact: ((x + 1) / 2 - mean) / std.  Rounding: x * fp32(a) + fp32(b), to fp32 (the kernel's fused
    multiply-add: the float64 expression is exact for bf16 x of ordinary size), then to bf16."""
    x = frames.double()
    if not rounding:
        m, s = torch.tensor(mean, dtype=torch.float64), torch.tensor(std, dtype=torch.float64)
        return ((x + 1.0) / 2.0 - m[:, None, None]) / s[:, None, None]
    a, b = fold(mean, std)
    return (x * a[:, None, None] + b[:, None, None]).float().to(BF16).double()


def patch_rows(pixels, p, pad_to=None):
    """[F, 3, H, W] -> [F * H/p * W/p, 3 p^2 (zero-padded to pad_to)], columns in the order (c, dy, dx) of conv.weight.reshape(D, -1)"""
    F, C, H, W = pixels.shape
    rows = pixels.reshape(F, C, H // p, p, W // p, p).permute(0, 2, 4, 1, 3, 5).reshape(F * (H // p) * (W // p), C * p * p)
    if pad_to is not None and pad_to > rows.shape[1]:
        rows = torch.cat([rows, rows.new_zeros(rows.shape[0], pad_to - rows.shape[1])], dim=1)
    return rows


def assemble(patch, cls, pos, F, rounding=False):
    """patch [F * P, D], cls [D], pos [P + 1, D] -> [F, P + 1, D].  Rounding goes through fp32 as the kernel's sum does."""
    D = patch.shape[-1]
    tok = torch.cat([cls.reshape(1, 1, D).expand(F, 1, D), patch.reshape(F, -1, D)], dim=1) + pos[None]
    return tok.float().to(BF16).to(patch.dtype) if rounding else tok


def layernorm(x, w, b, eps, rounding=False):
    mean = x.mean(-1, keepdim=True)
    var = (x - mean).pow(2).mean(-1, keepdim=True)
    return _r((x - mean) * torch.rsqrt(var + eps) * w + b, rounding)


def gelu_tanh(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x.pow(3))))


def act(x, mode, rounding=False):
    """"gelu": 0.5 x (1 + erf(x / sqrt 2)), written with erfc(-t) == 1 + erf(t) so that float64 keeps the negative tail; "quick_gelu": x sigmoid(1.702 x)"""
    if mode == "gelu":
        y = 0.5 * x * torch.special.erfc(-x / math.sqrt(2.0))
    elif mode == "quick_gelu":
        y = x * torch.sigmoid(1.702 * x)
    elif mode == "tanh_gelu":
        y = gelu_tanh(x)
    else:
        raise ValueError(mode)
    return _r(y, rounding)


def attention(q, k, v, scale=0.125, rounding=False):
    """q, k, v [B, S, H, 64] -> [B, S, H * 64]: softmax(q k^T * scale) v, P and the output rounded in kernel-rounding mode"""
    s = torch.einsum("bihd,bjhd->bhij", q, k) * scale
    p = _r(torch.softmax(s, dim=-1), rounding)
    o = torch.einsum("bhij,bjhd->bihd", p, v)
    return _r(o.reshape(q.shape[0], q.shape[1], -1), rounding)


def _names(kind, i):
    if kind == "vit":
        return (f"layers.{i}.attention.", "o_proj", f"layers.{i}.layernorm_before.", f"layers.{i}.layernorm_after.", f"layers.{i}.mlp.")
    e = f"vision_model.encoder.layers.{i}."
    return (e + "self_attn.", "out_proj", e + "layer_norm1.", e + "layer_norm2.", e + "mlp.")


def vit_forward(sd, cfg, kind, frames, dtype=torch.float64, rounding=False, mutate=None, device="cpu", mean=None, std=None):
    """sd: in-memory names -> tensors; cfg: dict with hidden_size, num_attention_heads, num_hidden_layers, patch_size, hidden_act, layer_norm_eps;
    frames [F, 3, s, s] in [-1, 1]; returns the features [F, D_out] in `dtype`"""
    W = lambda n: sd[n].to(device=device, dtype=dtype)
    H, eps, p, L = cfg["num_attention_heads"], cfg["layer_norm_eps"], cfg["patch_size"], cfg["num_hidden_layers"]
    mode = "tanh_gelu" if mutate == "tanh_gelu" else cfg["hidden_act"]
    m0, s0 = MEAN_STD[kind]
    pixels = preprocess(frames.cpu(), mean or m0, std or s0, rounding).to(device=device, dtype=dtype)
    F = pixels.shape[0]
    lin = lambda t, n, bias=True: _r(t @ W(n + ".weight").t() + (W(n + ".bias") if bias else 0.0), rounding)
    if kind == "vit":
        conv, cls, pos = "embeddings.patch_embeddings.projection", W("embeddings.cls_token").reshape(-1), W("embeddings.position_embeddings")[0]
    else:
        conv, cls, pos = "vision_model.embeddings.patch_embedding", W("vision_model.embeddings.class_embedding"), W("vision_model.embeddings.position_embedding.weight")
    D = cls.numel()
    patch = _r(patch_rows(pixels, p) @ W(conv + ".weight").reshape(D, -1).t() + (W(conv + ".bias") if kind == "vit" else 0.0), rounding)
    if mutate == "pos_shift":
        pos = torch.roll(pos, 1, 0)
    x = assemble(patch, cls, pos, F, rounding)
    S = x.shape[1]
    if kind == "clip" and mutate != "no_pre_ln":
        x = layernorm(x, W("vision_model.pre_layrnorm.weight"), W("vision_model.pre_layrnorm.bias"), eps, rounding)
    for i in range(L):
        attn, o, ln1, ln2, mlp = _names(kind, i)
        h = layernorm(x, W(ln1 + "weight"), W(ln1 + "bias"), eps, rounding)
        q, k, v = (lin(h, attn + f"{n}_proj").view(F, S, H, 64) for n in "qkv")
        a = attention(q, k, v, 1.0 if mutate == "no_scale" else 0.125, rounding)
        x = _r(x + lin(a, attn + o), rounding)
        h = layernorm(x, W(ln2 + "weight"), W(ln2 + "bias"), eps, rounding)
        x = _r(x + lin(act(lin(h, mlp + "fc1"), mode, rounding), mlp + "fc2"), rounding)
    c = x[:, 0]
    fin = "layernorm." if kind == "vit" else "vision_model.post_layernorm."
    if mutate != "cls_norm":
        c = layernorm(c, W(fin + "weight"), W(fin + "bias"), eps, rounding)
    return lin(c, "visual_projection", bias=False) if kind == "clip" else c


def vit_forward_torch_bf16(sd, cfg, kind, frames, device="cpu", mean=None, std=None):
    """The torch route in bf16: the library's arithmetic with torch ops on bf16 tensors (F.linear, F.layer_norm, matmul in bf16; the softmax in float32).  Its error
    against an exact run is the yardstick of the real-width GPU test."""
    import torch.nn.functional as Fn
    W = lambda n: sd[n].to(device=device, dtype=BF16)
    H, eps, p, L = cfg["num_attention_heads"], cfg["layer_norm_eps"], cfg["patch_size"], cfg["num_hidden_layers"]
    m0, s0 = MEAN_STD[kind]
    pixels = preprocess(frames.cpu(), mean or m0, std or s0).to(device=device, dtype=BF16)
    F = pixels.shape[0]
    if kind == "vit":
        conv, cls, pos = "embeddings.patch_embeddings.projection", W("embeddings.cls_token").reshape(-1), W("embeddings.position_embeddings")[0]
    else:
        conv, cls, pos = "vision_model.embeddings.patch_embedding", W("vision_model.embeddings.class_embedding"), W("vision_model.embeddings.position_embedding.weight")
    D = cls.numel()
    patch = Fn.linear(patch_rows(pixels, p), W(conv + ".weight").reshape(D, -1), W(conv + ".bias") if kind == "vit" else None)
    x = torch.cat([cls.reshape(1, 1, D).expand(F, 1, D), patch.reshape(F, -1, D)], dim=1) + pos[None]
    S = x.shape[1]
    ln = lambda t, n: Fn.layer_norm(t, (D,), W(n + "weight"), W(n + "bias"), eps)
    if kind == "clip":
        x = ln(x, "vision_model.pre_layrnorm.")
    for i in range(L):
        attn, o, ln1, ln2, mlp = _names(kind, i)
        h = ln(x, ln1)
        q, k, v = (Fn.linear(h, W(attn + f"{n}_proj.weight"), W(attn + f"{n}_proj.bias")).view(F, S, H, 64).transpose(1, 2) for n in "qkv")
        pr = torch.softmax((torch.matmul(q, k.transpose(3, 2)) * 0.125).float(), dim=-1).to(BF16)
        a = torch.matmul(pr, v).transpose(1, 2).reshape(F, S, D)
        x = x + Fn.linear(a, W(attn + o + ".weight"), W(attn + o + ".bias"))
        h = Fn.linear(ln(x, ln2), W(mlp + "fc1.weight"), W(mlp + "fc1.bias"))
        h = Fn.gelu(h) if cfg["hidden_act"] == "gelu" else h * torch.sigmoid(1.702 * h)
        x = x + Fn.linear(h, W(mlp + "fc2.weight"), W(mlp + "fc2.bias"))
    c = ln(x[:, 0], "layernorm." if kind == "vit" else "vision_model.post_layernorm.")
    return Fn.linear(c, W("visual_projection.weight")) if kind == "clip" else c


def consistency(feat, first=None, prev=None):
    """feat [F, D] -> (prev, first, score) in float64: max(0, cos) of every frame that has a predecessor with the previous frame and with the first, and
    mean((prev + first) / 2).  cos(x, y) = x . y / (max(|x|, 1e-8) max(|y|, 1e-8)), F.cosine_similarity's definition (a zero row gives 0).  With carried rows
    every frame of `feat` has a predecessor."""
    f = feat.double()
    if first is not None:
        f = torch.cat([prev.double()[None], f])
        anchor = first.double()
    else:
        anchor = f[0]
    cos = lambda x, y: (x * y).sum(-1) / (x.norm(dim=-1).clamp_min(1e-8) * y.norm(dim=-1).clamp_min(1e-8))
    pv = cos(f[1:], f[:-1]).clamp_min(0.0)
    fs = cos(f[1:], anchor[None].expand_as(f[1:])).clamp_min(0.0)
    return pv, fs, ((pv + fs) / 2).mean()


def special_features(D=128, seed=0):
    """fp32 [7, D] with the three special rows of the tests: row 2 = -row 1 (cosine -1 with its predecessor: clamped to 0), row 4 = row 3 (a repeated frame:
    cosine 1), row 5 = 0 (a zero row: cosine 0 with both neighbours, not NaN)"""
    f = torch.randn(7, D, generator=torch.Generator().manual_seed(seed))
    f[2] = -f[1]
    f[4] = f[3]
    f[5] = 0
    return f
