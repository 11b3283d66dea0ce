"""Frozen ViT image encoders on the gfx950 kernels: frames -> one feature per frame, for the frame-consistency metric (metrics.video_consistency).

Host mirror of two transformers models, both pre-LayerNorm ViTs with heads of 64:
  kind "vit"   `ViTModel(add_pooling_layer=False)` (DINO ViT-B/16: "subject"); the feature is the class token after the final LayerNorm;
  kind "clip"  `CLIPVisionModelWithProjection` (CLIP ViT-B/32: "background"): `pre_layrnorm`, a patch convolution without bias, quick GELU; the feature is
               visual_projection(post_layernorm(class token)).
Per call (csrc/vit.hip): rows = tg_vit_patch_rows(frames) with the preprocessing folded in;  tok = tg_vit_assemble(tg_gemm_bf16(rows, conv weight), cls,
pos);  per block  h = tg_layernorm(x);  qkv = tg_gemm_bf16(h, q/8 | k | v);  a = tg_t5_attention(qkv, zero table);  x = tg_residual_add(x, tg_gemm_bf16(a, o));
h = tg_layernorm(x);  x = tg_residual_add(x, tg_gemm_bf16(tg_vit_act(tg_gemm_bf16(h, fc1)), fc2));  then the final LayerNorm on the class-token rows only.
The blocks, the packed storage and the module plumbing are encoder.PreLNTower's; q | k | v carries q pre-scaled by 1/8 (encoder.py says why that is exact).

uint8 frames go through video_io.prepare_video(..., (image_size, image_size), crop_to_fit=True): bicubic antialiased cover, then centre crop — CLIP's own
preprocessing; for the DINO encoder a stated deviation from benchmark scripts that resize without cropping.
A frame's feature does not depend on how many frames a call carries: every GEMM is launched with at least 1024 rows (encoder.gemm_rows).
There is no CPU path: construction and loading work on any device, a forward needs the GPU.  No weights ship."""
import json
import os
import re
from collections import OrderedDict
from types import SimpleNamespace

import torch

from . import kernels as K
from .encoder import BF16, PreLNTower, check_gemm_shapes, config_dict, read_checkpoint

MAX_TOKENS = 512                   # tg_t5_attention keeps one head's K and V in LDS

_DEFAULTS = {
    "vit": dict(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072, hidden_act="gelu", layer_norm_eps=1e-12, image_size=224,
                patch_size=16, num_channels=3, qkv_bias=True, image_mean=(0.485, 0.456, 0.406), image_std=(0.229, 0.224, 0.225)),
    "clip": dict(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072, hidden_act="quick_gelu", layer_norm_eps=1e-5, image_size=224,
                 patch_size=32, num_channels=3, projection_dim=512, image_mean=(0.48145466, 0.4578275, 0.40821073),
                 image_std=(0.26862954, 0.26130258, 0.27577711)),
}
_DINOV2 = ("layerscale_value", "use_swiglu_ffn", "num_register_tokens")


def fold_preprocessing(mean, std):
    """((x + 1) / 2 - mean_c) / std_c == x * a[c] + b[c] for x in [-1, 1]: a = 0.5 / std, b = (0.5 - mean) / std, as Python floats (the kernel takes fp32)."""
    return [0.5 / s for s in std], [(0.5 - m) / s for m, s in zip(mean, std)]


# ------------------------------------------------------------------------------------------------------ names
_VIT_FILE = [(re.compile(p), r) for p, r in (
    (r"^encoder\.layer\.(\d+)\.attention\.attention\.query\.", r"layers.\1.attention.q_proj."),
    (r"^encoder\.layer\.(\d+)\.attention\.attention\.key\.", r"layers.\1.attention.k_proj."),
    (r"^encoder\.layer\.(\d+)\.attention\.attention\.value\.", r"layers.\1.attention.v_proj."),
    (r"^encoder\.layer\.(\d+)\.attention\.output\.dense\.", r"layers.\1.attention.o_proj."),
    (r"^encoder\.layer\.(\d+)\.intermediate\.dense\.", r"layers.\1.mlp.fc1."),
    (r"^encoder\.layer\.(\d+)\.output\.dense\.", r"layers.\1.mlp.fc2."),
    (r"^encoder\.layer\.(\d+)\.layernorm_(before|after)\.", r"layers.\1.layernorm_\2."),
)]
_CLIP_OTHER_TOWER = ("text_model.", "text_projection.", "logit_scale", "logit_bias")


def canonical_state_dict(state_dict, kind):
    """Any accepted naming -> the in-memory names of transformers 5.x for `kind` (what ViTEncoder.state_dict() hands out), same tensors.
    "vit":  the names stored in published checkpoint files (`encoder.layer.N.attention.attention.query.weight`, `...attention.output.dense`, `...intermediate.dense`,
            `...output.dense`, an optional leading `vit.`) or the in-memory ones (`layers.N.attention.q_proj.weight`, `layers.N.mlp.fc1`); `pooler.*` entries are
            dropped (the model is built without pooler).
    "clip": `vision_model.*` and `visual_projection.*` under the names both the files and the library use; from a whole CLIPModel state dict the text tower, its
            projection and the logit scale are dropped, and so is the `position_ids` buffer of older files.
    A name that fits neither family is passed on unchanged, so that load_state_dict reports it as unexpected under its own name."""
    out = OrderedDict()
    for k, v in state_dict.items():
        if kind == "vit":
            k = k[4:] if k.startswith("vit.") else k
            if k.startswith("pooler."):
                continue
            for pat, rep in _VIT_FILE:
                k, n = pat.subn(rep, k)
                if n:
                    break
        else:
            if k.startswith(_CLIP_OTHER_TOWER) or k.endswith("embeddings.position_ids"):
                continue
        out[k] = v
    return out


class ViTEncoder(PreLNTower):
    _frozen = "requires_grad: the image encoders have no backward pass here (they are frozen feature extractors of a metric)"

    def __init__(self, config=None, device="cuda", kind=None, **kw):
        raw = config_dict(config, **kw)
        kind = kind or raw.pop("kind", None) or {"vit": "vit", "clip": "clip", "clip_vision_model": "clip"}.get(raw.get("model_type"), None)
        raw.pop("kind", None)
        if kind not in _DEFAULTS:
            raise ValueError(f"ViTEncoder: kind must be 'vit' or 'clip', got {kind!r}")
        if (raw.get("model_type") or "").startswith("dinov2") or any(raw.get(k) for k in _DINOV2):
            raise NotImplementedError("DINOv2-style configurations (layer scale, SwiGLU feed-forward, register tokens) are not built: a plain ViTModel or "
                                      f"CLIP vision tower only (got {({k: raw[k] for k in ('model_type',) + _DINOV2 if raw.get(k)})})")
        cfg = dict(_DEFAULTS[kind])
        cfg.update({k: v for k, v in raw.items() if k in cfg})
        c = SimpleNamespace(kind=kind, **cfg)
        self.kind = kind
        super().__init__(c, device)
        if c.num_channels != 3 or (kind == "vit" and not c.qkv_bias):
            raise NotImplementedError("three input channels and q / k / v projections with bias only")
        if c.image_size % c.patch_size:
            raise NotImplementedError(f"image_size {c.image_size} is not a multiple of patch_size {c.patch_size}")
        D, p = c.hidden_size, c.patch_size
        self.grid = c.image_size // p
        self.tokens = self.grid * self.grid + 1
        self.patch_k = 3 * p * p
        self.patch_kp = (self.patch_k + 63) // 64 * 64
        self.out_dim = c.projection_dim if kind == "clip" else D
        check_gemm_shapes([("patch", D, self.patch_kp)] + self._block_gemms() + ([("visual_projection", self.out_dim, D)] if kind == "clip" else []))
        if self.tokens > MAX_TOKENS:
            raise NotImplementedError(f"S = {self.tokens} tokens per image: tg_t5_attention keeps a head's keys in LDS, S <= {MAX_TOKENS}")
        self.frames_per_launch = 64
        self.image_mean, self.image_std = tuple(float(v) for v in c.image_mean), tuple(float(v) for v in c.image_std)
        z, one = self._zeros, self._ones
        # the packed weights are the storage (packed once, at load): the patch convolution as [D, Kp] rows with zero pad columns
        w = self._w = {"patch_w": z(D, self.patch_kp), "cls": z(D), "pos": z(self.tokens, D), "ln_w": one(D), "ln_b": z(D)}
        if kind == "vit":
            w["patch_b"] = z(D)
        else:
            w.update({"pre_w": one(D), "pre_b": z(D), "proj": z(self.out_dim, D)})
        self._alloc_layers()

    def _drop_caches(self):
        super()._drop_caches()
        self._zero_bias = None

    # ---------------------------------------------------------------------------------------------- weights
    def _views(self):
        """canonical name -> (view of the packed storage, scale applied at load)"""
        c, w, D, p = self.config, self._w, self.config.hidden_size, self.config.patch_size
        v = OrderedDict()
        conv = w["patch_w"][:, :self.patch_k].view(D, 3, p, p)
        if self.kind == "vit":
            v["embeddings.cls_token"] = (w["cls"].view(1, 1, D), 1.0)
            v["embeddings.position_embeddings"] = (w["pos"].view(1, self.tokens, D), 1.0)
            v["embeddings.patch_embeddings.projection.weight"] = (conv, 1.0)
            v["embeddings.patch_embeddings.projection.bias"] = (w["patch_b"], 1.0)
            layer = lambda i: (f"layers.{i}.attention.", "o_proj", f"layers.{i}.layernorm_before.", f"layers.{i}.layernorm_after.", f"layers.{i}.mlp.")
        else:
            v["vision_model.embeddings.class_embedding"] = (w["cls"], 1.0)
            v["vision_model.embeddings.patch_embedding.weight"] = (conv, 1.0)
            v["vision_model.embeddings.position_embedding.weight"] = (w["pos"], 1.0)
            v["vision_model.pre_layrnorm.weight"], v["vision_model.pre_layrnorm.bias"] = (w["pre_w"], 1.0), (w["pre_b"], 1.0)
            layer = lambda i: (f"vision_model.encoder.layers.{i}.self_attn.", "out_proj", f"vision_model.encoder.layers.{i}.layer_norm1.",
                               f"vision_model.encoder.layers.{i}.layer_norm2.", f"vision_model.encoder.layers.{i}.mlp.")
        for i in range(c.num_hidden_layers):
            self._layer_views(v, i, *layer(i))
        if self.kind == "vit":
            v["layernorm.weight"], v["layernorm.bias"] = (w["ln_w"], 1.0), (w["ln_b"], 1.0)
        else:
            v["vision_model.post_layernorm.weight"], v["vision_model.post_layernorm.bias"] = (w["ln_w"], 1.0), (w["ln_b"], 1.0)
            v["visual_projection.weight"] = (w["proj"], 1.0)
        return v

    def _canonical(self, state_dict):
        return canonical_state_dict(state_dict, self.kind)

    @classmethod
    def from_pretrained(cls, path, device="cuda", kind=None, **kw):
        """<path>/config.json + model.safetensors or pytorch_model.bin of a ViTModel, a CLIPVisionModelWithProjection or a whole CLIPModel (its `vision_config` and
        `projection_dim` are taken); image_mean / image_std of <path>/preprocessor_config.json override the kind's defaults when that file is there."""
        with open(os.path.join(path, "config.json")) as f:
            cfg = json.load(f)
        if "vision_config" in cfg:                                    # CLIPModel
            cfg = dict(cfg["vision_config"], projection_dim=cfg.get("projection_dim", cfg["vision_config"].get("projection_dim", 512)), model_type="clip")
        pre = os.path.join(path, "preprocessor_config.json")
        if os.path.exists(pre):
            with open(pre) as f:
                cfg.update({k: v for k, v in json.load(f).items() if k in ("image_mean", "image_std")})
        cfg.update(kw)
        m = cls(cfg, device=device, kind=kind)
        m.load_state_dict(read_checkpoint(path), strict=True)
        return m

    # ---------------------------------------------------------------------------------------------- forward
    def _trunk(self, frames, out):
        """frames bf16 [n, 3, s, s] in [-1, 1], n <= frames_per_launch -> out fp32 [n, out_dim]"""
        c, w, D, S, n = self.config, self._w, self.config.hidden_size, self.tokens, frames.shape[0]
        ws = self._workspace((n, self.frames_per_launch), n * S,
                             {"rows": (n * (S - 1), self.patch_kp), "patch": (n * (S - 1), D), "cls": (n, D), "proj": (n, self.out_dim)})
        if self._zero_bias is None:
            self._zero_bias = torch.zeros(c.num_attention_heads, 2 * S - 1, dtype=torch.float32, device=self.device)
        a, b = fold_preprocessing(self.image_mean, self.image_std)
        K.vit_patch_rows(frames, c.patch_size, a, b, ws.rows)
        K.gemm(ws.rows, w["patch_w"], w.get("patch_b"), ws.patch)
        tok = ws.x[:n * S].view(n, S, D)
        eps = c.layer_norm_eps
        if self.kind == "clip":
            K.vit_assemble(ws.patch, w["cls"], w["pos"], ws.h[:n * S].view(n, S, D))
            K.layernorm(ws.h, w["pre_w"], w["pre_b"], ws.x, eps)
        else:
            K.vit_assemble(ws.patch, w["cls"], w["pos"], tok)
            ws.x[n * S:].zero_()                                          # the ignored rows restart from zero: they would add up over the calls otherwise
        self._run_blocks(ws, n, S, self._zero_bias)
        K.layernorm(tok[:, 0], w["ln_w"], w["ln_b"], ws.cls[:n], eps)     # the class-token rows only: row stride S * D
        if self.kind == "clip":
            K.gemm(ws.cls, w["proj"], None, ws.proj)
            out.copy_(ws.proj[:n])
        else:
            out.copy_(ws.cls[:n])
        return out

    @torch.no_grad()
    def encode_frames(self, frames):
        """uint8 [F, H, W, 3] / [B, T, H, W, 3] (any size: resized to cover image_size, centre-cropped) or bf16 [F, 3, image_size, image_size] in [-1, 1]
        -> fp32 [F, out_dim] on the device, not normalised.  Long inputs run in batches of frames_per_launch; a frame's feature does not depend on the batching."""
        if not isinstance(frames, torch.Tensor):
            raise TypeError("encode_frames: expected a torch tensor")
        if frames.requires_grad:
            raise NotImplementedError("requires_grad: the image encoders have no backward pass here")
        s = self.config.image_size
        if frames.dtype == torch.uint8:
            if frames.dim() == 5:
                frames = frames.reshape(-1, *frames.shape[2:])
            if frames.dim() != 4 or frames.shape[-1] != 3:
                raise ValueError(f"encode_frames: uint8 frames must be [F, H, W, 3] or [B, T, H, W, 3], got {tuple(frames.shape)}")
        elif frames.dtype == BF16:
            if frames.dim() != 4 or frames.shape[1] != 3:
                raise ValueError(f"encode_frames: bf16 frames must be [F, 3, {s}, {s}], got {tuple(frames.shape)}")
            if tuple(frames.shape[2:]) != (s, s):
                raise NotImplementedError(f"encode_frames: bf16 frames of {tuple(frames.shape[2:])}, the configuration's image_size is {s}: position embeddings are "
                                          "not interpolated; pass uint8 frames (resized here) or resize first")
        else:
            raise TypeError(f"encode_frames: uint8 display frames or bf16 frames in [-1, 1], got {frames.dtype}")
        if frames.shape[0] < 1:
            raise ValueError("encode_frames: no frames")
        if self.device.type != "cuda":
            raise RuntimeError("ViTEncoder: the forward pass needs the GPU (tokensgen_amd has no CPU fallback); build the model with device='cuda'")
        F, step = frames.shape[0], int(self.frames_per_launch)
        if step < 1:
            raise ValueError("frames_per_launch must be >= 1")
        out = torch.empty(F, self.out_dim, dtype=torch.float32, device=self.device)
        for f0 in range(0, F, step):
            part = frames[f0:f0 + step]
            if part.dtype == torch.uint8:
                from .video_io import prepare_video
                part = prepare_video(part, output_res=(s, s), crop_to_fit=True, device=self.device)[0]
            self._trunk(part.to(self.device).contiguous(), out[f0:f0 + step])
        return out

    __call__ = encode_frames
