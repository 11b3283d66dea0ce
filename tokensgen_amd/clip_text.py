"""The CLIP text tower on the gfx950 kernels: token ids -> one feature per prompt in CLIP's joint space, for the text-video alignment metric
(metrics.video_text_alignment; the image half is vit.ViTEncoder(kind="clip")).

Host mirror of transformers' `CLIPTextModelWithProjection` (modeling_clip.py of transformers 5.x): token embedding + learned position embedding, pre-LayerNorm blocks
with CAUSAL self-attention and heads of 64, `final_layer_norm`, one pooled row per sequence, `text_projection` without bias.
Per call (csrc/clip_text.hip, csrc/vit.hip, csrc/t5.hip): x = tg_text_embed(ids, token table, position table);  per block  h = tg_layernorm(x);
qkv = tg_gemm_bf16(h, q/8 | k | v);  a = tg_t5_attention(qkv, causal table);  x = tg_residual_add(x, tg_gemm_bf16(a, o));  h = tg_layernorm(x);
x = tg_residual_add(x, tg_gemm_bf16(tg_vit_act(tg_gemm_bf16(h, fc1)), fc2));  then tg_layernorm, the pooled rows picked on the device, tg_gemm_bf16 for the projection.
The blocks, the packed storage and the module plumbing are encoder.PreLNTower's; q | k | v carries q pre-scaled by 1/8 (encoder.py says why that is exact).

The causal mask is tg_t5_attention's bias-by-distance table: 0 for key - query <= 0, -inf for key - query > 0 (`causal_table`).  Key 0 is visible to every query, so
every row maximum is finite, a masked term is exp(-inf) = 0 exactly whatever its (finite) score, and a masked key adds an exact 0 to P V.  -inf and not a large finite
value: it absorbs any finite score, where a finite constant would have to be argued against the largest score.

Pooling follows the library's two rules: with `eos_token_id == 2` (the published OpenAI configurations) the row at `input_ids.argmax(-1)`; otherwise the first
position whose id equals `eos_token_id`.  STATED DEVIATION: a sequence without that id is a ValueError here; the library silently pools position 0.
No padding mask is needed: attention is causal, so the pooled row sees itself and earlier tokens only — the library's `text_embeds` with the tokenizer's mask, without
it, and with every later token replaced are equal to the bit (tests/test_clip_text_cpu.py).  `attention_mask` may be None or a right-padded mask that covers the pooled
position; anything else (left padding, holes, a masked pooled position) is refused.

A prompt's feature does not depend on its batch mates: every GEMM is launched with at least 1024 rows (encoder.gemm_rows).  There is no CPU path: construction and
loading work on any device, a forward needs the GPU.  No weights ship, and the tokenizer is the caller's (`encode_prompts` takes a transformers.CLIPTokenizer)."""
import json
import os
from collections import OrderedDict
from types import SimpleNamespace

import torch

from . import kernels as K
from .encoder import PreLNTower, check_gemm_shapes, config_dict, read_checkpoint

MAX_POSITIONS = 512                # tg_t5_attention keeps one head's K and V in LDS

# text_config of openai/clip-vit-base-patch32
_DEFAULTS = dict(vocab_size=49408, hidden_size=512, intermediate_size=2048, num_hidden_layers=12, num_attention_heads=8, max_position_embeddings=77,
                 hidden_act="quick_gelu", layer_norm_eps=1e-5, projection_dim=512, eos_token_id=2)
_OTHER_TOWER = ("vision_model.", "visual_projection.", "logit_scale", "logit_bias")
_BARE = ("embeddings.", "encoder.", "final_layer_norm.")


def canonical_state_dict(state_dict):
    """Any accepted naming -> the names of a transformers CLIPTextModelWithProjection (what CLIPTextEncoder.state_dict() hands out), same tensors: `text_model.*` and
    `text_projection.weight` as that model and a whole CLIPModel name them, or the tower's own names without the `text_model.` prefix (`embeddings.*`, `encoder.*`,
    `final_layer_norm.*`).  From a whole CLIPModel state dict the vision tower, its projection and the logit scale / bias are dropped, and so is the `position_ids`
    buffer of older files.  Any other name is passed on unchanged, so that load_state_dict reports it as unexpected under its own name."""
    out = OrderedDict()
    for k, v in state_dict.items():
        if k.startswith(_OTHER_TOWER) or k.endswith("embeddings.position_ids"):
            continue
        out["text_model." + k if k.startswith(_BARE) else k] = v
    return out


def causal_table(heads, S, device):
    """tg_t5_attention's bias_by_distance for causal attention: fp32 [heads, 2 S - 1], entry j - i + S - 1 is 0 for j <= i and -inf for j > i"""
    t = torch.zeros(heads, 2 * S - 1, dtype=torch.float32)
    t[:, S:] = float("-inf")
    return t.to(device)


def pooled_positions(input_ids, eos_token_id):
    """The library's pooling rule on host ids [B, S] -> int64 [B]: argmax of the ids for eos_token_id == 2, else the first position that holds eos_token_id
    (ValueError if a sequence has none: the library would take position 0)."""
    if eos_token_id == 2:
        return input_ids.argmax(dim=-1)
    hit = input_ids == eos_token_id
    if not bool(hit.any(dim=-1).all()):
        bad = [i for i, h in enumerate(hit.any(dim=-1).tolist()) if not h]
        raise ValueError(f"encode_text: sequence(s) {bad} hold no eos_token_id = {eos_token_id}; the pooled row is the first such position "
                         "(transformers would silently pool position 0)")
    return hit.int().argmax(dim=-1)


class CLIPTextEncoder(PreLNTower):
    _frozen = "requires_grad: the text tower has no backward pass here (it is a frozen feature extractor of a metric)"

    def __init__(self, config=None, device="cuda", **kw):
        cfg = dict(_DEFAULTS)
        cfg.update({k: v for k, v in config_dict(config, **kw).items() if k in cfg and v is not None})
        c = SimpleNamespace(**cfg)
        super().__init__(c, device)
        D = c.hidden_size
        self.out_dim = c.projection_dim
        check_gemm_shapes(self._block_gemms() + [("text_projection", self.out_dim, D)])
        if not 1 <= c.max_position_embeddings <= MAX_POSITIONS:
            raise NotImplementedError(f"max_position_embeddings = {c.max_position_embeddings}: tg_t5_attention keeps a head's keys in LDS, S <= {MAX_POSITIONS}")
        self.prompts_per_launch = 64
        z, one = self._zeros, self._ones
        # the packed weights are the storage (packed once, at load)
        self._w = {"tok": z(c.vocab_size, D), "pos": z(c.max_position_embeddings, D), "ln_w": one(D), "ln_b": z(D), "proj": z(self.out_dim, D)}
        self._alloc_layers()

    def _drop_caches(self):
        super()._drop_caches()
        self._tables, self._status = {}, None

    # ---------------------------------------------------------------------------------------------- weights
    def _views(self):
        """library name -> (view of the packed storage, scale applied at load)"""
        c, w = self.config, self._w
        v = OrderedDict()
        v["text_model.embeddings.token_embedding.weight"] = (w["tok"], 1.0)
        v["text_model.embeddings.position_embedding.weight"] = (w["pos"], 1.0)
        for i in range(c.num_hidden_layers):
            e = f"text_model.encoder.layers.{i}."
            self._layer_views(v, i, e + "self_attn.", "out_proj", e + "layer_norm1.", e + "layer_norm2.", e + "mlp.")
        v["text_model.final_layer_norm.weight"], v["text_model.final_layer_norm.bias"] = (w["ln_w"], 1.0), (w["ln_b"], 1.0)
        v["text_projection.weight"] = (w["proj"], 1.0)
        return v

    def _canonical(self, state_dict):
        return canonical_state_dict(state_dict)

    @classmethod
    def from_pretrained(cls, path, device="cuda", **kw):
        """<path>/config.json + model.safetensors or pytorch_model.bin of a CLIPTextModelWithProjection or a whole CLIPModel (its `text_config` and `projection_dim`
        are taken)."""
        with open(os.path.join(path, "config.json")) as f:
            cfg = json.load(f)
        if "text_config" in cfg:                                      # CLIPModel
            cfg = dict(cfg["text_config"], projection_dim=cfg.get("projection_dim", cfg["text_config"].get("projection_dim", 512)))
        cfg.update(kw)
        m = cls(cfg, device=device)
        m.load_state_dict(read_checkpoint(path), strict=True)
        return m

    # ---------------------------------------------------------------------------------------------- forward
    def _trunk(self, ids, rows, out):
        """ids int32 [B, S] and rows int64 [B] (b * S + pooled position), both on the device -> out fp32 [B, out_dim]"""
        c, w, D, (B, S) = self.config, self._w, self.config.hidden_size, ids.shape
        ws = self._workspace((B, S), B * S, {"pool": (B, D), "proj": (B, self.out_dim)})
        if S not in self._tables:
            self._tables[S] = causal_table(c.num_attention_heads, S, self.device)
        if self._status is None:                                          # tg_text_embed's count of refused ids: encode_text validated them on the host, so it stays 0 and is never read back
            self._status = torch.zeros(1, dtype=torch.int32, device=self.device)
        K.text_embed(ids.view(-1), S, w["tok"], w["pos"], ws.x, self._status)
        ws.x[B * S:].zero_()                                              # the ignored rows restart from zero: they would add up over the calls otherwise
        self._run_blocks(ws, B, S, self._tables[S])
        K.layernorm(ws.x, w["ln_w"], w["ln_b"], ws.h, c.layer_norm_eps)
        torch.index_select(ws.h, 0, rows, out=ws.pool[:B])                # the pooled rows, picked on the device: a copy of B rows, no host synchronisation
        K.gemm(ws.pool, w["proj"], None, ws.proj)
        out.copy_(ws.proj[:B])
        return out

    @torch.no_grad()
    def encode_text(self, input_ids, attention_mask=None):
        """input_ids int32 / int64 [B, S] or [S], S <= max_position_embeddings, as the caller's CLIP tokenizer pads them -> fp32 [B, projection_dim] on the device, not
        normalised (`text_embeds` of the library).  The ids are validated and the pooled positions found on the host (ids on the device are copied back for it).
        attention_mask: None or a right-padded [B, S] mask that covers the pooled position; it changes nothing (causal attention) and is only checked."""
        c = self.config
        if not isinstance(input_ids, torch.Tensor):
            raise TypeError("encode_text: expected a torch tensor of token ids")
        if input_ids.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"encode_text: int32 or int64 token ids, got {input_ids.dtype}")
        ids = input_ids.detach().cpu()
        if ids.dim() == 1:
            ids = ids[None]
        if ids.dim() != 2 or ids.shape[0] < 1 or ids.shape[1] < 1:
            raise ValueError(f"encode_text: input_ids must be [B, S] or [S], got {tuple(input_ids.shape)}")
        B, S = ids.shape
        if S > c.max_position_embeddings:
            raise ValueError(f"encode_text: {S} tokens, the model has max_position_embeddings = {c.max_position_embeddings} (truncate with the tokenizer)")
        if int(ids.min()) < 0 or int(ids.max()) >= c.vocab_size:
            raise ValueError(f"encode_text: token ids must lie in [0, {c.vocab_size}), got [{int(ids.min())}, {int(ids.max())}]")
        pos = pooled_positions(ids.long(), c.eos_token_id)
        if attention_mask is not None:
            m = attention_mask.detach().cpu()
            m = m[None] if m.dim() == 1 else m
            if tuple(m.shape) != (B, S):
                raise ValueError(f"encode_text: attention_mask {tuple(attention_mask.shape)} does not match input_ids {tuple(input_ids.shape)}")
            m = m != 0
            right_padded = bool((m[:, 1:] <= m[:, :-1]).all()) if S > 1 else True
            if not right_padded or not bool(m[torch.arange(B), pos].all()):
                raise NotImplementedError("encode_text: only attention_mask=None or a right-padded mask that covers the pooled position: under causal attention such a "
                                          "mask changes nothing; left padding, holes or a masked pooled position would, and are not built")
        if self.device.type != "cuda":
            raise RuntimeError("CLIPTextEncoder: the forward pass needs the GPU (tokensgen_amd has no CPU fallback); build the model with device='cuda'")
        step = int(self.prompts_per_launch)
        if step < 1:
            raise ValueError("prompts_per_launch must be >= 1")
        out = torch.empty(B, self.out_dim, dtype=torch.float32, device=self.device)
        ids32 = ids.to(torch.int32).contiguous().to(self.device)
        rows = (torch.arange(B) * S + pos).to(self.device)
        for b0 in range(0, B, step):
            n = min(step, B - b0)
            self._trunk(ids32[b0:b0 + n], rows[b0:b0 + n] - b0 * S, out[b0:b0 + n])
        return out

    __call__ = encode_text


def encode_prompts(tokenizer, model, prompts):
    """prompts (a string or a list of strings) -> fp32 [len(prompts), projection_dim]: the caller's transformers.CLIPTokenizer with padding="max_length" and
    truncation to the model's max_position_embeddings, then model.encode_text.  A prompt beyond that length is cut by the tokenizer: encode long prompts sentence by
    sentence (metrics.video_text_alignment takes K text features)."""
    if isinstance(prompts, str):
        prompts = [prompts]
    tok = tokenizer(list(prompts), padding="max_length", truncation=True, max_length=model.config.max_position_embeddings, return_tensors="pt")
    return model.encode_text(tok["input_ids"], tok.get("attention_mask") if hasattr(tok, "get") else None)
