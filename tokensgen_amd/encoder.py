"""What the frozen transformer encoders (t5.T5EncoderModel, vit.ViTEncoder, clip_text.CLIPTextEncoder) share on the host: the module plumbing of a frozen model whose
packed bf16 weights are its storage (`FrozenEncoder`), and the pre-LayerNorm tower with heads of 64 that the two CLIP / ViT encoders run (`PreLNTower`).  Two rules
are stated here and nowhere else:

q pre-scaled by 1/8.  tg_t5_attention has no softmax scale (T5 has none).  A tower whose attention is softmax(q k^T / sqrt(64)) multiplies q_proj's weight and bias by
1/8 = 64 ** -0.5 when it loads them (`PreLNTower._layer_views`): a power of two, so the product is exact in bf16, and the kernel serves as it is.  state_dict() hands
q_proj out multiplied by 8 again, which is exact too.

At least 1024 GEMM rows.  `gemm_rows` below: a feature does not depend on how many frames or prompts share its call.

There is no CPU path: construction and loading work on any device, a forward needs the GPU."""
import os
from collections import OrderedDict
from types import SimpleNamespace

import torch

from . import kernels as K

BF16 = torch.bfloat16
GEMM_BIG_ROWS = 1024               # csrc/gemm_plan.h: from this many rows on (and N % 256 == 0) tg_gemm_bf16 launches a 256 x 256 kernel


def config_dict(config=None, **kw):
    """A configuration object (its attributes) or a dict, then the keyword overrides -> a plain dict without the `_`-prefixed keys of a library config."""
    raw = {k: v for k, v in (vars(config) if hasattr(config, "__dict__") else dict(config or {})).items() if not k.startswith("_")}
    raw.update(kw)
    return raw


def check_gemm_shapes(gemms):
    """(what, N, K) of every weight that goes through tg_gemm_bf16: refused at construction, not at the first forward."""
    for what, n, k in gemms:
        if n % 128 or k % 64:
            raise NotImplementedError(f"the {what} projection [{n}, {k}] breaks tg_gemm_bf16's N % 128 == 0 / K % 64 == 0 rule")


def gemm_rows(rows):
    """Rows a GEMM over `rows` real rows is launched with.  tg_gemm_bf16 changes kernels at 1024 rows, and two kernels need not give the same bits; so every GEMM of a
    tower has at least 1024 rows (the extra rows of a short batch are workspace: zeros or stale values, computed and ignored — a GEMM row depends on its own input row
    alone).  Every other kernel works per row, per item or per (item, head), so a feature does not depend on the batch it travels in."""
    return max(rows, GEMM_BIG_ROWS)


def read_checkpoint(path):
    """<path>/model.safetensors, else <path>/pytorch_model.bin (tensors only) -> a state dict on the host"""
    st = os.path.join(path, "model.safetensors")
    if os.path.exists(st):
        from safetensors.torch import load_file
        return load_file(st)
    return torch.load(os.path.join(path, "pytorch_model.bin"), map_location="cpu", weights_only=True)


class FrozenEncoder:
    """A frozen bf16 model whose packed weights `_w` (a dict of tensors, packed once, at load) are the storage.  A subclass supplies `_views()`, may supply
    `_canonical()`, `_tied` and `_frozen`, and keeps whatever it caches on the device in attributes that its `_drop_caches()` sets to empty."""
    _tied = frozenset()            # names of one tensor: any of them in a state dict stands for all of them
    _frozen = "requires_grad: no backward pass here"

    def __init__(self, device):
        self.dtype = BF16
        self.device = torch.device(device)
        self._w = {}
        self._drop_caches()

    def _zeros(self, *shape):
        return torch.zeros(*shape, dtype=BF16, device=self.device)

    def _ones(self, *shape):
        return torch.ones(*shape, dtype=BF16, device=self.device)

    def _views(self):
        """library name -> (view of the packed storage, scale applied at load)"""
        raise NotImplementedError

    def _canonical(self, state_dict):
        """any accepted naming -> the names of `_views()`; a name that fits none is passed on, so that it is reported as unexpected under its own name"""
        return state_dict

    def _drop_caches(self):
        """tables, workspaces and status words on the device: empty at construction and after a move"""

    def state_dict(self):
        """The library's names -> bf16 tensors as they were loaded: a view of the storage where the scale is 1, else a copy with the scale undone."""
        return OrderedDict((k, t if s == 1.0 else t * (1.0 / s)) for k, (t, s) in self._views().items())

    def load_state_dict(self, state_dict, strict=True):
        views, tied = self._views(), self._tied
        sd = self._canonical(state_dict)
        unexpected = [k for k in sd if k not in views]
        missing = [k for k in views if k not in sd and not (k in tied and tied & set(sd))]
        bad = [f"{k}: {tuple(sd[k].shape)} != {tuple(views[k][0].shape)}" for k in sd if k in views and sd[k].shape != views[k][0].shape]
        if bad or (strict and (missing or unexpected)):
            raise RuntimeError(f"{type(self).__name__}.load_state_dict: size mismatch {bad}; missing keys {missing}; unexpected keys {unexpected}")
        with torch.no_grad():
            for k, t in sd.items():
                if k in views:
                    dst, s = views[k]
                    t = t.to(device=self.device, dtype=BF16)
                    dst.copy_(t if s == 1.0 else t * s)              # a power of two: exact in bf16
        return SimpleNamespace(missing_keys=missing, unexpected_keys=unexpected)

    def to(self, device=None, *unused, **kw):
        device = kw.get("device", device)
        if device is not None and not isinstance(device, torch.dtype) and torch.device(device) != self.device:
            self.device = torch.device(device)
            self._w = {k: t.to(self.device) for k, t in self._w.items()}
            self._drop_caches()
        return self

    def eval(self):
        return self

    def requires_grad_(self, flag=False):
        if flag:
            raise NotImplementedError(self._frozen)
        return self


class PreLNTower(FrozenEncoder):
    """L pre-LayerNorm blocks with biases and heads of 64 (ViTModel, both CLIP towers) over a padded workspace.  `config` names the sizes as those libraries' configs
    do: hidden_size, intermediate_size, num_attention_heads, num_hidden_layers, hidden_act, layer_norm_eps.  Per layer i the storage is l{i}.ln1_w, ln1_b, qkv_w, qkv_b
    (q | k | v rows, q pre-scaled), o_w, o_b, ln2_w, ln2_b, fc1_w, fc1_b, fc2_w, fc2_b.  The subclass owns what comes before and after the blocks."""
    _gemm_rows = staticmethod(gemm_rows)

    def __init__(self, config, device):
        c = self.config = config
        if c.hidden_size % c.num_attention_heads or c.hidden_size // c.num_attention_heads != 64:
            raise NotImplementedError(f"hidden_size / num_attention_heads = {c.hidden_size} / {c.num_attention_heads}: tg_t5_attention has head dimension 64 only")
        if c.hidden_act not in K.VIT_ACT:
            raise NotImplementedError(f"hidden_act = {c.hidden_act!r}: tg_vit_act has 'gelu' (exact) and 'quick_gelu' only")
        super().__init__(device)

    def _drop_caches(self):
        self._ws = {}              # call shape -> buffers (`_workspace`)

    def _block_gemms(self):
        D, I = self.config.hidden_size, self.config.intermediate_size
        return [("q | k | v", 3 * D, D), ("o", D, D), ("fc1", I, D), ("fc2", D, I)]

    def _alloc_layers(self):
        """adds the blocks' storage to `_w`: identity LayerNorms, zero projections"""
        z, one, D, I = self._zeros, self._ones, self.config.hidden_size, self.config.intermediate_size
        for i in range(self.config.num_hidden_layers):
            self._w.update({f"l{i}.ln1_w": one(D), f"l{i}.ln1_b": z(D), f"l{i}.qkv_w": z(3 * D, D), f"l{i}.qkv_b": z(3 * D), f"l{i}.o_w": z(D, D), f"l{i}.o_b": z(D),
                            f"l{i}.ln2_w": one(D), f"l{i}.ln2_b": z(D), f"l{i}.fc1_w": z(I, D), f"l{i}.fc1_b": z(I), f"l{i}.fc2_w": z(D, I), f"l{i}.fc2_b": z(D)})

    def _layer_views(self, v, i, attn, o, ln1, ln2, mlp):
        """adds layer i's views to `v` under the library's names: `attn`{q,k,v}_proj and `attn``o` (the output projection's name), the norm prefixes `ln1` and `ln2`,
        `mlp`fc1 and `mlp`fc2.  Row order of the fused weight: q rows, then k, then v; q carries the 1/8."""
        w, D = self._w, self.config.hidden_size
        for j, n in enumerate("qkv"):
            s = 0.125 if n == "q" else 1.0
            v[attn + f"{n}_proj.weight"] = (w[f"l{i}.qkv_w"][j * D:(j + 1) * D], s)
            v[attn + f"{n}_proj.bias"] = (w[f"l{i}.qkv_b"][j * D:(j + 1) * D], s)
        v[attn + o + ".weight"], v[attn + o + ".bias"] = (w[f"l{i}.o_w"], 1.0), (w[f"l{i}.o_b"], 1.0)
        v[ln1 + "weight"], v[ln1 + "bias"] = (w[f"l{i}.ln1_w"], 1.0), (w[f"l{i}.ln1_b"], 1.0)
        v[ln2 + "weight"], v[ln2 + "bias"] = (w[f"l{i}.ln2_w"], 1.0), (w[f"l{i}.ln2_b"], 1.0)
        for n in ("fc1", "fc2"):
            v[mlp + n + ".weight"], v[mlp + n + ".bias"] = (w[f"l{i}.{n}_w"], 1.0), (w[f"l{i}.{n}_b"], 1.0)

    def _workspace(self, key, rows, extra):
        """The buffers of one call shape, kept under `key` (two shapes stay resident): x, h, qkv, a, o, f for `rows` tokens and the subclass's `extra`
        {name: (rows, columns)}, each with gemm_rows(rows) rows.  Zeros: the ignored rows stay finite."""
        ws = self._ws.get(key)
        if ws is None:
            D, rt = self.config.hidden_size, gemm_rows(rows)
            ws = SimpleNamespace(x=self._zeros(rt, D), h=self._zeros(rt, D), qkv=self._zeros(rt, 3 * D), a=self._zeros(rt, D), o=self._zeros(rt, D),
                                 f=self._zeros(rt, self.config.intermediate_size), **{name: self._zeros(gemm_rows(r), k) for name, (r, k) in extra.items()})
            if len(self._ws) >= 2:
                self._ws = {}
            self._ws[key] = ws
        return ws

    def _run_blocks(self, ws, batch, S, bias):
        """ws.x (`batch` items of S tokens in its first rows) through the L blocks, in place; bias: tg_t5_attention's fp32 [heads, 2 S - 1] table"""
        c, w, D = self.config, self._w, self.config.hidden_size
        qkv, att = ws.qkv[:batch * S].view(batch, S, 3 * D), ws.a[:batch * S].view(batch, S, D)
        eps = c.layer_norm_eps
        for i in range(c.num_hidden_layers):
            p = f"l{i}."
            K.layernorm(ws.x, w[p + "ln1_w"], w[p + "ln1_b"], ws.h, eps)
            K.gemm(ws.h, w[p + "qkv_w"], w[p + "qkv_b"], ws.qkv)
            K.t5_attention(qkv, bias, att, c.num_attention_heads)
            K.gemm(ws.a, w[p + "o_w"], w[p + "o_b"], ws.o)
            K.residual_add(ws.x, ws.o, ws.x)
            K.layernorm(ws.x, w[p + "ln2_w"], w[p + "ln2_b"], ws.h, eps)
            K.gemm(ws.h, w[p + "fc1_w"], w[p + "fc1_b"], ws.f)
            K.vit_act(ws.f, ws.f, c.hidden_act)
            K.gemm(ws.f, w[p + "fc2_w"], w[p + "fc2_b"], ws.o)
            K.residual_add(ws.x, ws.o, ws.x)
