"""The T5 text encoder on the gfx950 kernels: a sentence -> `prompt_embeds`.

Host mirror of `transformers.T5EncoderModel` in the `CogVideoX-5b/text_encoder` configuration (T5-v1.1-XXL encoder: d_model 4096, d_kv 64, 64 heads, d_ff 10240,
24 layers, gated-gelu, 32 relative-attention buckets, max distance 128, eps 1e-6, no biases) as the reference calls it: `_get_t5_prompt_embeds` / `encode_prompt`
(longvgen/pipeline/pipeline_cogvideox_mp_fifo.py:365-486, pipeline_cogvideox_t2to.py:313-434) and `compute_prompt_embeddings` (train_cogvideo_to2v.py:890-980).
None of those call sites passes an attention mask (:397, :345, :917): padded positions attend and are attended to, and so they do here.

Per block (csrc/t5.hip):  h = tg_rmsnorm(x);  qkv = tg_gemm_bf16(h, q|k|v);  a = tg_t5_attention(qkv, bias_by_distance);  x = tg_residual_add(x,
tg_gemm_bf16(a, o));  h = tg_rmsnorm(x);  g = tg_gated_gelu(tg_gemm_bf16(h, wi_0|wi_1));  x = tg_residual_add(x, tg_gemm_bf16(g, wo));  then the final norm.
The embedding lookup is a torch gather on the device (plumbing).  The relative-position bias is built on the HOST once per sequence length, as an fp32 table
[heads, 2 S - 1] indexed by j - i + S - 1: the library's float32 `log` decides the bucket boundaries, and the same torch ops on the host give the same buckets.
The module plumbing is encoder.FrozenEncoder's; the block is T5's own (RMSNorm, no biases, gated GELU, no softmax scale, an unpadded workspace).
There is no CPU path: construction, loading and weight packing work on any device, a forward needs the GPU.  The tokenizer is the caller's (transformers.T5Tokenizer
or any object with its call interface)."""
import json
import logging
import math
import os
from collections import OrderedDict
from types import SimpleNamespace

import torch

from . import kernels as K
from .encoder import BF16, FrozenEncoder, check_gemm_shapes, config_dict
logger = logging.getLogger(__name__)
MAX_SEQUENCE_LENGTH = 512          # tg_t5_attention keeps one head's K and V in LDS

_NO_MASK = ("attention_mask is not supported: no call site of the reference passes one (pipeline_cogvideox_mp_fifo.py:397, pipeline_cogvideox_t2to.py:345, "
            "train_cogvideo_to2v.py:917), so padded positions attend and are attended to; call without a mask")

_DEFAULTS = dict(vocab_size=32128, d_model=4096, d_kv=64, d_ff=10240, num_layers=24, num_heads=64, relative_attention_num_buckets=32,
                 relative_attention_max_distance=128, layer_norm_epsilon=1e-6, feed_forward_proj="gated-gelu")


def relative_position_bucket(relative_position, num_buckets=32, max_distance=128):
    """T5Attention._relative_position_bucket, bidirectional, op for op (the float32 log and the truncation decide the boundaries); relative_position = j - i, int64."""
    num_buckets //= 2
    buckets = (relative_position > 0).to(torch.long) * num_buckets
    relative_position = torch.abs(relative_position)
    max_exact = num_buckets // 2
    is_small = relative_position < max_exact
    large = max_exact + (torch.log(relative_position.float() / max_exact) / math.log(max_distance / max_exact) * (num_buckets - max_exact)).to(torch.long)
    large = torch.min(large, torch.full_like(large, num_buckets - 1))
    return buckets + torch.where(is_small, relative_position, large)


def bias_by_distance(weight, S, num_buckets=32, max_distance=128):
    """fp32 [heads, 2 S - 1]: entry [h, d + S - 1] = relative_attention_bias.weight[bucket(d), h] for d = j - i in -(S - 1) .. S - 1 — compute_bias(S, S) without its
    S x S repetition.  Built on the host."""
    d = torch.arange(-(S - 1), S, dtype=torch.long)
    table = weight.detach().to("cpu", torch.float32)[relative_position_bucket(d, num_buckets, max_distance)].t()
    return table.reshape(-1).view(table.shape[0], 2 * S - 1)          # canonical strides at S = 1 too (a [H, 1] transpose keeps the source's)


class T5EncoderOutput(tuple):
    """`out[0]` and `out.last_hidden_state`, as BaseModelOutput offers them."""

    def __new__(cls, last_hidden_state):
        return super().__new__(cls, (last_hidden_state,))

    @property
    def last_hidden_state(self):
        return self[0]


class T5EncoderModel(FrozenEncoder):
    _tied = frozenset(("shared.weight", "encoder.embed_tokens.weight"))
    _frozen = "the T5 encoder has no backward pass here: it is frozen in every reference run"

    def __init__(self, config=None, device="cuda", **kw):
        cfg = dict(_DEFAULTS)
        cfg.update(config_dict(config, **kw))
        c = self.config = SimpleNamespace(**cfg)
        if c.d_kv != 64:
            raise NotImplementedError(f"d_kv = {c.d_kv}: tg_t5_attention has head dimension 64 only")
        if c.feed_forward_proj != "gated-gelu":
            raise NotImplementedError(f"feed_forward_proj = {c.feed_forward_proj!r}: only the gated-gelu feed-forward (gelu_new * linear) of T5 v1.1 is built")
        inner = c.num_heads * 64
        check_gemm_shapes((("q | k | v", 3 * inner, c.d_model), ("o", c.d_model, inner), ("wi_0 | wi_1", 2 * c.d_ff, c.d_model), ("wo", c.d_model, c.d_ff)))
        self.inner_dim = inner
        super().__init__(device)
        z, one = self._zeros, self._ones
        # the packed weights ARE the storage: state_dict() hands out views under the library's names, load_state_dict() copies into them (packed once, at load)
        self._w = {"emb": z(c.vocab_size, c.d_model), "rel_bias": z(c.relative_attention_num_buckets, c.num_heads), "final_ln": one(c.d_model)}
        for i in range(c.num_layers):
            self._w.update({f"l{i}.qkv": z(3 * inner, c.d_model), f"l{i}.o": z(c.d_model, inner), f"l{i}.wi": z(2 * c.d_ff, c.d_model), f"l{i}.wo": z(c.d_model, c.d_ff),
                            f"l{i}.ln0": one(c.d_model), f"l{i}.ln1": one(c.d_model)})

    def _drop_caches(self):
        self._bias = {}            # S -> fp32 [heads, 2 S - 1] on the device
        self._ws = {}              # (B, S) -> buffers; one shape resident

    # ---------------------------------------------------------------------------------------------- weights
    def _views(self):
        """library name -> (view of the packed storage, 1.0: nothing is scaled at load).  Row order of the fused weights: q rows, then k, then v; wi_0 rows, then wi_1."""
        c, w, inner = self.config, self._w, self.inner_dim
        v = OrderedDict()
        v["shared.weight"] = w["emb"]
        v["encoder.embed_tokens.weight"] = w["emb"]                # tied
        for i in range(c.num_layers):
            a, f = f"encoder.block.{i}.layer.0.", f"encoder.block.{i}.layer.1."
            for j, n in enumerate("qkv"):
                v[a + f"SelfAttention.{n}.weight"] = w[f"l{i}.qkv"][j * inner:(j + 1) * inner]
            v[a + "SelfAttention.o.weight"] = w[f"l{i}.o"]
            if i == 0:
                v[a + "SelfAttention.relative_attention_bias.weight"] = w["rel_bias"]
            v[a + "layer_norm.weight"] = w[f"l{i}.ln0"]
            v[f + "DenseReluDense.wi_0.weight"] = w[f"l{i}.wi"][:c.d_ff]
            v[f + "DenseReluDense.wi_1.weight"] = w[f"l{i}.wi"][c.d_ff:]
            v[f + "DenseReluDense.wo.weight"] = w[f"l{i}.wo"]
            v[f + "layer_norm.weight"] = w[f"l{i}.ln1"]
        v["encoder.final_layer_norm.weight"] = w["final_ln"]
        return OrderedDict((k, (t, 1.0)) for k, t in v.items())

    def load_state_dict(self, state_dict, strict=True):
        res = super().load_state_dict(state_dict, strict)
        self._bias = {}            # built from relative_attention_bias.weight
        return res

    @classmethod
    def from_pretrained(cls, path, subfolder="text_encoder", device="cuda", **unused):
        """<path>/<subfolder>/config.json + model.safetensors, or the shards of model.safetensors.index.json."""
        from safetensors.torch import load_file
        d = os.path.join(path, subfolder) if subfolder else path
        with open(os.path.join(d, "config.json")) as f:
            cfg = {k: v for k, v in json.load(f).items() if k in _DEFAULTS}
        m = cls(cfg, device=device)
        idx = os.path.join(d, "model.safetensors.index.json")
        if os.path.exists(idx):
            with open(idx) as f:
                files = sorted(set(json.load(f)["weight_map"].values()))
        else:
            files = ["model.safetensors"]
        seen = set()
        for fn in files:
            sd = load_file(os.path.join(d, fn))
            m.load_state_dict(sd, strict=False)
            seen |= set(sd)
        views, tied = m._views(), cls._tied
        missing = [k for k in views if k not in seen and not (k in tied and tied & seen)]
        unexpected = [k for k in seen if k not in views]
        if missing or unexpected:
            raise RuntimeError(f"T5EncoderModel.from_pretrained({d}): missing keys {missing}; unexpected keys {unexpected}")
        return m

    # ---------------------------------------------------------------------------------------------- forward
    def _bias_table(self, S):
        t = self._bias.get(S)
        if t is None:
            c = self.config
            t = self._bias[S] = bias_by_distance(self._w["rel_bias"], S, c.relative_attention_num_buckets, c.relative_attention_max_distance).to(self.device)
        return t

    def _workspace(self, B, S):
        ws = self._ws.get((B, S))
        if ws is None:
            c = self.config
            e = lambda n: torch.empty(B, S, n, dtype=BF16, device=self.device)
            ws = SimpleNamespace(x=e(c.d_model), h=e(c.d_model), qkv=e(3 * self.inner_dim), a=e(self.inner_dim), o=e(c.d_model), ff=e(2 * c.d_ff), g=e(c.d_ff))
            self._ws = {(B, S): ws}
        return ws

    @torch.no_grad()
    def __call__(self, input_ids, attention_mask=None, **unused):
        if attention_mask is not None:
            raise NotImplementedError(_NO_MASK)
        if input_ids.dim() != 2 or not 1 <= input_ids.shape[1] <= MAX_SEQUENCE_LENGTH or input_ids.shape[0] < 1:
            raise ValueError(f"input_ids must be [batch >= 1, 1 <= tokens <= {MAX_SEQUENCE_LENGTH}] (tg_t5_attention keeps a head's keys in LDS), got {tuple(input_ids.shape)}")
        if self.device.type != "cuda" or not input_ids.is_cuda:
            raise RuntimeError("T5EncoderModel: the forward pass needs the GPU (tokensgen_amd has no CPU fallback); build the model with device='cuda' and pass "
                               "input_ids on it")
        c, w = self.config, self._w
        B, S = input_ids.shape
        ws = self._workspace(B, S)
        bias = self._bias_table(S)
        torch.index_select(w["emb"], 0, input_ids.reshape(-1), out=ws.x.view(B * S, c.d_model))
        eps = c.layer_norm_epsilon
        for i in range(c.num_layers):
            p = f"l{i}."
            K.rmsnorm(ws.x, w[p + "ln0"], ws.h, eps)
            K.gemm(ws.h, w[p + "qkv"], None, ws.qkv)
            K.t5_attention(ws.qkv, bias, ws.a, c.num_heads)
            K.gemm(ws.a, w[p + "o"], None, ws.o)
            K.residual_add(ws.x, ws.o, ws.x)
            K.rmsnorm(ws.x, w[p + "ln1"], ws.h, eps)
            K.gemm(ws.h, w[p + "wi"], None, ws.ff)
            K.gated_gelu(ws.ff, ws.g)
            K.gemm(ws.g, w[p + "wo"], None, ws.o)
            K.residual_add(ws.x, ws.o, ws.x)
        out = torch.empty_like(ws.x)
        K.rmsnorm(ws.x, w["final_ln"], out, eps)
        return T5EncoderOutput(out)

    forward = __call__


# -------------------------------------------------------------------------------------------------- prompt encoding
def _get_t5_prompt_embeds(tokenizer, text_encoder, prompt, num_videos_per_prompt=1, max_sequence_length=226, device=None, dtype=None):
    """pipeline_cogvideox_mp_fifo.py:365-405"""
    device = device or text_encoder.device
    dtype = dtype or text_encoder.dtype
    prompt = [prompt] if isinstance(prompt, str) else prompt
    batch_size = len(prompt)
    text_input_ids = tokenizer(prompt, padding="max_length", max_length=max_sequence_length, truncation=True, add_special_tokens=True, return_tensors="pt").input_ids
    untruncated_ids = tokenizer(prompt, padding="longest", return_tensors="pt").input_ids
    if untruncated_ids.shape[-1] >= text_input_ids.shape[-1] and not torch.equal(text_input_ids, untruncated_ids):
        removed_text = tokenizer.batch_decode(untruncated_ids[:, max_sequence_length - 1: -1])
        logger.warning(f"The following part of your input was truncated because `max_sequence_length` is set to  {max_sequence_length} tokens: {removed_text}")
    prompt_embeds = text_encoder(text_input_ids.to(device))[0]
    prompt_embeds = prompt_embeds.to(dtype=dtype, device=device)
    _, seq_len, _ = prompt_embeds.shape
    prompt_embeds = prompt_embeds.repeat(1, num_videos_per_prompt, 1)
    return prompt_embeds.view(batch_size * num_videos_per_prompt, seq_len, -1)


def encode_prompt(tokenizer, text_encoder, prompt, negative_prompt=None, do_classifier_free_guidance=True, num_videos_per_prompt=1, prompt_embeds=None,
                  negative_prompt_embeds=None, max_sequence_length=226, device=None, dtype=None):
    """`encode_prompt` of the two pipelines (pipeline_cogvideox_mp_fifo.py:407-486, pipeline_cogvideox_t2to.py:355-434) as a function: returns (prompt_embeds,
    negative_prompt_embeds); the negative prompt defaults to "" and is encoded only under classifier-free guidance."""
    prompt = [prompt] if isinstance(prompt, str) else prompt
    batch_size = len(prompt) if prompt is not None else prompt_embeds.shape[0]
    if prompt_embeds is None:
        prompt_embeds = _get_t5_prompt_embeds(tokenizer, text_encoder, prompt, num_videos_per_prompt, max_sequence_length, device, dtype)
    if do_classifier_free_guidance and negative_prompt_embeds is None:
        negative_prompt = negative_prompt or ""
        negative_prompt = batch_size * [negative_prompt] if isinstance(negative_prompt, str) else negative_prompt
        if prompt is not None and type(prompt) is not type(negative_prompt):
            raise TypeError(f"`negative_prompt` should be the same type to `prompt`, but got {type(negative_prompt)} != {type(prompt)}.")
        elif batch_size != len(negative_prompt):
            raise ValueError(f"`negative_prompt`: {negative_prompt} has batch size {len(negative_prompt)}, but `prompt`: {prompt} has batch size {batch_size}. "
                             "Please make sure that passed `negative_prompt` matches the batch size of `prompt`.")
        negative_prompt_embeds = _get_t5_prompt_embeds(tokenizer, text_encoder, negative_prompt, num_videos_per_prompt, max_sequence_length, device, dtype)
    return prompt_embeds, negative_prompt_embeds


def compute_prompt_embeddings(tokenizer, text_encoder, prompt, max_sequence_length, device, dtype, requires_grad=False):
    """train_cogvideo_to2v.py:952-976 (the T2To script's is the same): one embedding row per prompt, no guidance rows."""
    if requires_grad:
        raise NotImplementedError("requires_grad=True: the T5 encoder has no backward pass here (the reference trains with a frozen text encoder)")
    return _get_t5_prompt_embeds(tokenizer, text_encoder, prompt, 1, max_sequence_length, device, dtype)
