"""T2To training step on the gfx950 kernels: full fine-tuning of the token-grid DiT (reference loop train_cogvideo_t2to.py:1961-2175 with
config/train/cogvideo_5b_vaevip_4x8x12_t2to.yaml).

`vpred_loss_and_grad_masked` (the masked, per-item normalised v-prediction loss, :2125-2166), `pca_project16` (the PCA normalisation of the
condensed tokens, :1761-1773), `T2ToBlockTrainer` (one plain CogVideoXBlock: forward with the intermediates kept, backward to EVERY block parameter
and to the block inputs), `T2ToTrainer` (the whole patch-1 model: embeddings, 42 blocks, final layers; activations kept while memory allows, the
other blocks recomputed), `t2to_arena_order` and `T2ToTrainStep` (add_noise -> forward -> masked loss -> backward -> gradient arena -> accumulate
/ all-reduce / clip / AdamW8bit through tokensgen_amd.optim).

Trainable set (:1531-1560): `transformer_trainable_modules` (["all"] in the yaml: every transformer parameter whose name does not contain
"patch_embed.proj"; or a list of name fragments) and, with `use_lora`, the LoRA adapter on the attention projections (`lora_params`, :1416-1427).  What
does not train is frozen: it gets no weight gradient (a third of the backward's GEMM work), only the input gradients flow through it.
No attention mask is applied: the loop passes `attention_kwargs={"attention_mask": ...}` (:2122) but the transformer pops "attention_masks"
(cogvideox_transformer_3d.py:653), so padded frames enter attention as ordinary tokens; only the loss is masked.  The forward-only product never
routes through this module."""
import math

import numpy as np
import torch

from . import kernels as K
from . import lib as L
from .lora import is_lora_key
from .optim import ParamArena, get_optimizer
from .train import (BF16, LOG2E, To2VBlockTrainer, To2VTrainStep, _act, _adaln_bwd, _cat_or_view, _dgrad, _fast_attention_ws, _gate_res_bwd, _pad_to,
                    _tok_group, _vpred_coef, _vt_scratch, _weight_t, colsum, colsum_multi, linear_backward, linear_backward_dx,
                    qk_layernorm_rope_backward)

FROZEN = "patch_embed.proj"          # the one frozen name fragment of the recipe (:1547)
_QKV_ORDER = ("attn1.to_q.weight", "attn1.to_k.weight", "attn1.to_v.weight", "attn1.to_q.bias", "attn1.to_k.bias", "attn1.to_v.bias")
_LORA_A_ORDER = ("attn1.to_q.lora_A.weight", "attn1.to_k.lora_A.weight", "attn1.to_v.lora_A.weight")
_LORA_MODULES = ("attn1.to_q", "attn1.to_k", "attn1.to_v", "attn1.to_out.0")
_HEAD = ("norm_final.", "norm_out.", "proj_out.")


def trainable_names(names, modules=("all",), lora=None):
    """train_cogvideo_t2to.py:1531-1557.  A parameter trains if "all" is listed in `modules` (transformer_trainable_modules) and its name lacks
    "patch_embed.proj"; or any listed fragment occurs in its name; or it is a LoRA tensor and `lora.is_trainable` is set.  The rules are the
    reference's, read literally: "all", or a fragment such as "attn1", selects the adapter tensors of those modules too — `is_trainable` adds the
    adapter where nothing else selects it (`modules=[]`: adapter-only training).  lora (a lora.LoraConfig) None: the model carries no adapter, and
    `*.lora_{A,B}.weight` entries among `names` are not parameters of it.  The default call is the yaml's: every name without "patch_embed.proj"."""
    modules = tuple(modules)
    out = []
    for n in names:
        if is_lora_key(n) and (lora is None or not lora.match(n.rsplit(".lora_", 1)[0])):
            continue
        if (("all" in modules and FROZEN not in n) or any(m in n for m in modules)
                or (lora is not None and lora.is_trainable and is_lora_key(n))):
            out.append(n)
    return sorted(out)


def t2to_arena_order(names, num_layers):
    """Arena order of the T2To trainable set = the order gradients become final in the backward: the final layers (norm_final, norm_out,
    proj_out) first, then the blocks from the last to the first, then the embeddings (patch_embed.text_proj, time_embedding).  Inside a block
    attn1.to_{q,k,v} weights and biases lead, adjacent, so that the fused [3D, D] projection weight is a view of the arena; the three lora_A of
    to_q | to_k | to_v follow side by side (one [3r, D] down-projection and one weight-gradient launch).  `names` may be any subset of the
    transformer's parameters (a partial trainable set, or the adapter alone): what is present keeps this order."""
    def block_key(n):
        for j, pat in enumerate(_QKV_ORDER):
            if n.endswith(pat):
                return (0, j, n)
        for j, pat in enumerate(_LORA_A_ORDER):
            if n.endswith(pat):
                return (1, j, n)
        return (2, 0, n)
    out = sorted(n for n in names if n.startswith(_HEAD))
    for i in reversed(range(num_layers)):
        pre = f"transformer_blocks.{i}."
        out += sorted((n for n in names if n.startswith(pre)), key=block_key)
    out += sorted(n for n in names if not n.startswith(_HEAD) and not n.startswith("transformer_blocks."))
    assert sorted(out) == sorted(names)
    return out


def t2to_rope(frames, height=8, width=12, head_dim=64, device=None):
    """RoPE of the token grid (train_cogvideo_t2to.py:2068-2091 with prepare_rotary_positional_embeddings :994-1075): positions 0..F-1, 0..h-1,
    0..w-1 (one chunk, patch 1, no spatial scale), channels split t | h | w = 52 | 6 | 6."""
    from .rope import rope_3d
    f32 = np.float32
    return rope_3d(head_dim, np.arange(frames, dtype=f32), np.arange(height, dtype=f32), np.arange(width, dtype=f32), dim_t=52, dim_h=6, dim_w=6,
                   device=device)


def _silu_grad(x):
    """d silu(x) / dx in fp32 (the time embedding's two [B, 512] activations: a few thousand elements per micro-step)."""
    x = x.float()
    s = torch.sigmoid(x)
    return s * (1 + x * (1 - s))


# ---------------------------------------------------------------------------------------------------------------------------------
# loss and input normalisation
# ---------------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def vpred_loss_and_grad_masked(model_output, noisy_model_input, model_input, timesteps, alphas_cumprod, valid_frames):
    """train_cogvideo_t2to.py:2125-2166: loss_b = sum(w_b (|pred - x0| * mask)^2) / sum(mask), loss = mean_b loss_b, with mask = 1 on the frames
    f < valid_frames[b] (prepare_loss_masks :1098-1108) and w_b = 1 / (1 - acp_t).  model_output / noisy_model_input / model_input bf16
    [B, F, C, H, W]; timesteps [B] (or [B, F]); valid_frames: B ints in 1..F (valid_num_chunks * num_temporal_queries).  Returns (loss fp32
    scalar, per-item losses [B], d loss / d model_output bf16: zero on the masked frames).  tg_vpred_loss_grad_masked; with every frame valid
    the result is bitwise train.vpred_loss_and_grad's."""
    for n, t in (("model_output", model_output), ("noisy_model_input", noisy_model_input), ("model_input", model_input)):
        K._chk(t, n)
        assert t.is_contiguous() and t.shape == model_output.shape
    B, F = model_output.shape[:2]
    E = model_output[0, 0].numel()
    valid = [int(v) for v in (valid_frames.tolist() if torch.is_tensor(valid_frames) else valid_frames)]
    if len(valid) != B or not all(1 <= v <= F for v in valid):
        raise ValueError(f"valid_frames {valid}: need {B} counts in 1..{F}")
    dev = model_output.device
    coef = _vpred_coef(model_output, timesteps, alphas_cumprod)
    vdev = torch.tensor(valid, dtype=torch.int32).to(dev)
    grad = torch.empty_like(model_output)
    lib = L.load()
    partial = torch.empty(lib.tg_vpred_loss_partial_floats(B * F, E), dtype=torch.float32, device=dev)
    L.check(lib.tg_vpred_loss_grad_masked(model_output.data_ptr(), noisy_model_input.data_ptr(), model_input.data_ptr(), coef.data_ptr(),
                                          vdev.data_ptr(), B, F, E, grad.data_ptr(), partial.data_ptr(), K._stream()), "tg_vpred_loss_grad_masked")
    sums = partial.view(B, -1).sum(dim=1)
    # per item by its own mask sum (the same scalar division as the unmasked wrapper's `/ (F * E)`)
    per_item = torch.stack([sums[b] / (valid[b] * E) for b in range(B)])
    return per_item.mean(), per_item, grad


@torch.no_grad()
def pca_project16(tokens, components, pca_mean, mean, std, grid=None):
    """train_cogvideo_t2to.py:1761-1773 `pca_normalization` on tg_pca_project16: condensed tokens -> model_input bf16 [B, F, 16, h, w].
    tokens: bf16 [B, F, C, h, w] (the reference's layout; rearranged to token rows here) or token-major [B, F*h*w, C] with grid = (F, h, w);
    components: the PCA's components_ (fp32, >= 16 rows of C); pca_mean: its mean_ [1, C]; mean / std: the normalisation statistics (their first
    16 entries are used, :1770-1772)."""
    dev = tokens.device
    if tokens.dim() == 5:
        B, F, C, h, w = tokens.shape
        rows = tokens.to(BF16).permute(0, 1, 3, 4, 2).reshape(B * F * h * w, C).contiguous()
    else:
        if grid is None:
            raise ValueError("pca_project16: token-major input needs grid=(frames, h, w)")
        F, h, w = grid
        B, n, C = tokens.shape
        assert n == F * h * w
        rows = tokens.to(BF16).reshape(B * n, C).contiguous()
    f32 = lambda t: torch.as_tensor(t).to(dev, torch.float32).reshape(-1).contiguous()
    comp = torch.as_tensor(components).to(dev, torch.float32)[:16].contiguous()
    pm, m16, s16 = f32(pca_mean), f32(mean)[:16].contiguous(), f32(std)[:16].contiguous()
    assert comp.shape == (16, C) and pm.numel() == C and m16.numel() == 16 and s16.numel() == 16
    out = torch.empty(B, F, 16, h, w, dtype=BF16, device=dev)
    L.check(L.load().tg_pca_project16(rows.data_ptr(), rows.stride(0), rows.shape[0], C, comp.data_ptr(), pm.data_ptr(), m16.data_ptr(),
                                      s16.data_ptr(), h * w, out.data_ptr(), K._stream()), "tg_pca_project16")
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# One plain CogVideoXBlock (cogvideox_transformer_3d.py:221-332 without the vip branch, attention_processor.py:1895-1953)
# ---------------------------------------------------------------------------------------------------------------------------------
class T2ToBlockTrainer:
    """`forward_x` runs the block on the joint stream text | video with the product kernels and keeps what the backward needs; `backward_x`
    returns the gradient of EVERY block parameter (norm1 / norm2: modulation linear + LayerNorm affine; attn1.to_{q,k,v,out.0}; attn1.norm_{q,k};
    ff.net.0.proj, ff.net.2), of the block input stream, and of the modulation input silu(temb) (fp32 [B, te]: the time embedding's share from
    this block).  sd: the state dict under the reference's names (bf16 on the GPU; views of the parameter arena in the training step).

    trainable: None (every block parameter trains: full fine-tuning, the launches of the plain trainer) or the set of FULL parameter names that
    train.  A parameter outside it is frozen: its gradient is ABSENT from the returned dict (not zero), the weight-gradient GEMM and the bias column
    sum of a frozen linear are not launched, and by-products of kernels that run anyway (LayerNorm-affine / modulation sums, the norm_q / norm_k
    sums) are dropped; input gradients always flow.  A weight that trains is transposed by every dgrad that reads it (an optimizer step writes
    the arena through raw pointers without bumping tensor versions); the transpose of a frozen weight is made once and kept (`_wt`).

    lora (lora.LoraConfig): the adapter tensors `attn1.{to_q,to_k,to_v,to_out.0}.lora_{A,B}.weight` of `sd` are applied UNMERGED in every forward,
    y = x W^T + b + s (x A^T) B^T: T = x A^T is one GEMM (to_q | to_k | to_v: one GEMM on the three A stacked, [3r, D]) and is kept for the
    backward; the projection is then the plain GEMM followed by `out += s T B^T` through the gated-residual epilogue (the two-launch form of the
    To2V trainer) — or, with `fused_tail = True` and where the shape has it (kernels.gemm_lora_supported), ONE launch with the low-rank tail
    folded into the K loop (kernels.gemm_lora: no second pass over the output, s applied in fp32); for q | k | v that is THREE calls on the
    thirds of the output, each with its own [D, r] lora_B (one call with a block-diagonal [3D, 3r] B would run three times the tail stages on
    every tile).  Backward: dT = dY B is a plain GEMM, dX = dY W + s dT A is the dgrad + the accumulating tail GEMM, or gemm_lora again (for
    q | k | v ONE call, K = 3D, R = 3r); the adapter gradients come from tg_lora_wgrad (straight into the gradient arena when `grad_sink` is
    set).  `fused_tail` is off by default: the same-box A/B (profiles/t2to_lora_bench.json, profiles/NOTES.md §I) has the tail kernel 2-12 %
    SLOWER than the two launches it replaces.  Restrictions (NotImplementedError otherwise): rank % 128 == 0 (the
    down-projection's N granule; the kernel itself takes R % 64), D % 128 == 0, and the targets are to_q | to_k | to_v as a group and / or
    to_out.0."""

    fused_tail = False         # True: adapted projections run on kernels.gemm_lora where the shape has it (slower today: profiles/NOTES.md §I)

    def __init__(self, sd, pre, heads, n_text, eps=1e-5, trainable=None, lora=None):
        self.sd, self.pre, self.H, self.Nt, self.eps = sd, pre, heads, n_text, eps
        self.keep = True
        self.trainable = trainable
        self._wt = {}             # transposes of this block's FROZEN weights, made on first use (train._weight_t)
        self.grad_sink = None     # (ParamArena, scale): the adapter gradients are ADDED straight into the arena's fp32 gradient instead of being returned
        g = lambda n: sd[f"{pre}.{n}"]
        qkv = [f"attn1.to_{n}.{p_}" for p_ in ("weight", "bias") for n in "qkv"]
        self.qkv_trains = [self._tr(n) for n in qkv]
        self.Wqkv = _cat_or_view([g(n) for n in qkv[:3]])       # views of the arena when q, k, v are adjacent there; else a copy: made once when all six are
        self.bqkv = _cat_or_view([g(n) for n in qkv[3:]])       # frozen (it never goes stale), re-made by every forward when some of them train
        self.fused_is_view = (self.Wqkv.data_ptr() == g("attn1.to_q.weight").data_ptr() and self.bqkv.data_ptr() == g("attn1.to_q.bias").data_ptr())
        self.lora, self.lora_qkv, self.lora_out = lora, False, False
        if lora is not None:
            la = lambda t, h: sd.get(f"{pre}.attn1.{t}.lora_{h}.weight") if lora.match(f"{pre}.attn1.{t}") else None
            have = [la(f"to_{n}", h) is not None for n in "qkv" for h in "AB"]
            if any(have) and not all(have):
                raise NotImplementedError(f"{pre}: LoRA on some of to_q / to_k / to_v only (they are adapted as a group here)")
            self.lora_qkv, self.lora_out = all(have), la("to_out.0", "A") is not None and la("to_out.0", "B") is not None
            if self.lora_qkv or self.lora_out:
                D = g("attn1.to_q.weight").shape[1]
                if lora.rank % 128 or D % 128:
                    raise NotImplementedError(f"LoRA rank {lora.rank} / width {D}: the training path needs multiples of 128 (the GEMM's N granule)")
            if self.lora_qkv:
                self.lA3 = _cat_or_view([la(f"to_{n}", "A") for n in "qkv"])
                self.lA3_is_view = self.lA3.data_ptr() == la("to_q", "A").data_ptr()
                self.lB = [la(f"to_{n}", "B") for n in "qkv"]
            if self.lora_out:
                self.lAo, self.lBo = la("to_out.0", "A"), la("to_out.0", "B")

    _scale_tab = To2VBlockTrainer._scale_tab          # gate table holding s = lora_alpha / r (the two-launch form's `out += s T B^T`)
    _lora_wgrad = To2VBlockTrainer._lora_wgrad        # s y^T t on tg_lora_wgrad, into the arena when a sink is installed

    def lora_names(self):
        """Names (relative to the block) of the adapter tensors this block applies."""
        return ([f"attn1.to_{n}.lora_{h}.weight" for h in "AB" for n in "qkv"] if self.lora_qkv else []) + \
               ([f"attn1.to_out.0.lora_{h}.weight" for h in "AB"] if self.lora_out else [])

    def _w(self, n):
        return self.sd[f"{self.pre}.{n}"]

    def _tr(self, n):
        """Does the block parameter `n` (name relative to the block) train?"""
        return self.trainable is None or f"{self.pre}.{n}" in self.trainable

    def _frozen(self, n, key=None):
        """`frozen` argument of train._dgrad / _weight_t for the weight(s) `n`: the kept-transpose slot when none of them trains, else None."""
        names = [n] if isinstance(n, str) else n
        return None if any(self._tr(m) for m in names) else (self._wt, key or names[0])

    def _refresh_fused(self):
        """The concatenated copies whose parts train (a partial trainable set that splits q | k | v, or an arena that does not hold them side by
        side) are re-made from the tensors an optimizer step has written."""
        if self.trainable is None:
            return
        if not self.fused_is_view and any(self.qkv_trains):
            self.Wqkv = torch.cat([self._w(f"attn1.to_{n}.weight") for n in "qkv"]).contiguous()
            self.bqkv = torch.cat([self._w(f"attn1.to_{n}.bias") for n in "qkv"]).contiguous()
        if self.lora_qkv and not self.lA3_is_view and any(self._tr(f"attn1.to_{n}.lora_A.weight") for n in "qkv"):
            self.lA3 = torch.cat([self._w(f"attn1.to_{n}.lora_A.weight") for n in "qkv"]).contiguous()

    def _lora_linear(self, x, W, b, T, Bm, out):
        """out = x W^T + b + s T Bm^T ([B, N, .] views): one launch with the tail in the K loop, or the plain GEMM + the accumulating tail GEMM."""
        s = self.lora.scaling
        Bn, N, Kd, lda, _ = K._bmk(x)
        if self.fused_tail and K.gemm_lora_supported(N, W.shape[0], Kd, T.shape[-1], lda, W.stride(0), T.stride(-2), Bm.stride(0)):
            return K.gemm_lora(x, W, b, T, Bm, s, out)
        K.gemm(x, W, b, out, L.EPI_BIAS)
        return K.gemm(T, Bm, None, out, L.EPI_BIAS_GATE_RES, residual=out, gate=self._scale_tab(N, W.shape[0], Bn, x.device))

    def _lora_dgrad(self, dy, W, wkey, dT, A, akey):
        """dX = dY W + s dT A for y = x W^T + s (x A^T) B^T: dy [B, N, out], W [out, in], dT [B, N, R], A [R, in] -> [B, N, in].  gemm_lora with
        W := W^T, T := dT, B := A^T, or the dgrad + the accumulating tail GEMM."""
        s = self.lora.scaling
        Bn, N, cout = dy.shape
        cin, R = W.shape[1], A.shape[0]
        if self.fused_tail and cout % 64 == 0 and K.gemm_lora_supported(N, cin, cout, R, dy.stride(1), cout, dT.stride(1), R):
            dx = torch.empty(Bn, N, cin, dtype=BF16, device=dy.device)
            return K.gemm_lora(dy, _weight_t(W, wkey), None, dT, _weight_t(A, akey), s, dx)      # W^T [in, out], A^T [in, R]
        dx = _dgrad(dy.reshape(Bn * N, cout), W, frozen=wkey).view(Bn, N, cin)
        return linear_backward_dx(dT, A, accumulate_into=dx, ones=self._scale_tab(N, cin, Bn, dy.device), frozen=akey)

    def _mod(self, emb, which):
        """[B, 1, 6D] modulation of norm{which} (shift, scale, gate | enc_shift, enc_scale, enc_gate, normalization.py:441-460) and its group
        table: group 0 = the video rows, group 1 = the text rows (one timestep per item: one modulation row)."""
        D = self.D
        mod = torch.empty(emb.shape[0], 1, 6 * D, dtype=BF16, device=emb.device)
        K.gemm(emb, self._w(f"norm{which}.linear.weight"), self._w(f"norm{which}.linear.bias"), mod, L.EPI_BIAS)
        return mod, K.GroupTable(mod, self.tok_group, [0, 0], [0, 3 * D], [D, 4 * D], [2 * D, 5 * D])

    def _gated_add(self, x, mod, y):
        """x + gate * y per row group (hidden = hidden + gate * h, text = text + enc_gate * t: cogvideox_transformer_3d.py:290-293, 321-324)."""
        D, Nt = self.D, self.Nt
        out = torch.empty_like(x)
        torch.addcmul(x[:, Nt:], mod[:, :, 2 * D:3 * D], y[:, Nt:], out=out[:, Nt:])
        torch.addcmul(x[:, :Nt], mod[:, :, 5 * D:6 * D], y[:, :Nt], out=out[:, :Nt])
        return out

    @torch.no_grad()
    def forward(self, hidden, enc, temb, rope):
        """Reference block interface: hidden [B, Nv, D], enc = text [B, Nt, D], temb [B, te] (one timestep per item)."""
        emb = _act(temb.reshape(temb.shape[0], 1, -1).contiguous())
        X2 = self.forward_x(torch.cat([enc, hidden], dim=1).contiguous(), emb, rope)
        return X2[:, self.Nt:], X2[:, :self.Nt]

    @torch.no_grad()
    def forward_x(self, X0, emb, rope):
        """X0 [B, Nt + Nv, D]: the residual stream text | video; emb = silu(temb) [B, 1, te].  Returns the block's output stream."""
        H, Nt = self.H, self.Nt
        B, N, D = X0.shape
        self.D = D
        dev = X0.device
        e = lambda *s: torch.empty(*s, dtype=BF16, device=dev)
        self.tok_group = _tok_group(Nt, N - Nt, 0, 1, dev)
        rope = tuple(t.to(dev, torch.float32).contiguous() for t in rope)
        self._refresh_fused()
        mod1, t1 = self._mod(emb, 1)
        Xn = e(B, N, D)
        K.adaln_modulate(X0, Xn, self._w("norm1.norm.weight"), self._w("norm1.norm.bias"), self.eps, t1)
        qkv_pre = e(B, N, 3 * D)
        T3 = To = None
        if self.lora_qkv:                                     # T = x A^T for the three projections at once, then every third with its own tail
            r = self.lora.rank
            T3 = e(B, N, 3 * r)
            K.gemm(Xn, self.lA3, None, T3, L.EPI_BIAS)
            for j in range(3):
                self._lora_linear(Xn, self.Wqkv[j * D:(j + 1) * D], self.bqkv[j * D:(j + 1) * D], T3[:, :, j * r:(j + 1) * r], self.lB[j],
                                  qkv_pre[:, :, j * D:(j + 1) * D])
        else:
            K.gemm(Xn, self.Wqkv, self.bqkv, qkv_pre, L.EPI_BIAS)
        # post-norm Q / K out of place (the backward reads the pre-norm rows); K carries sm_scale * log2(e) for the constant-shift attention
        qkv = e(B, N, 2 * D)
        sm = 1.0 / 8.0
        retry, km1, kws = _fast_attention_ws(N, H, B, dev)
        K.qk_layernorm_rope_pair(qkv_pre[:, :, :D], qkv_pre[:, :, D:2 * D], H, self._w("attn1.norm_q.weight"), self._w("attn1.norm_q.bias"),
                                 self._w("attn1.norm_k.weight"), self._w("attn1.norm_k.bias"), 1e-6, (Nt, rope), k_scale=sm * LOG2E, kmax=km1,
                                 kmax_ws=kws, out=(qkv[:, :, :D], qkv[:, :, D:2 * D]))
        vt = K.transpose_v(qkv_pre[:, :, 2 * D:], H, 0, N, _vt_scratch(B, H, _pad_to(N, 64), (0, N), dev))
        q, k, v = qkv[:, :, :D], qkv[:, :, D:2 * D], qkv_pre[:, :, 2 * D:]
        o1 = e(B, N, D)
        _, lse = K.attention_lse(q, k, vt, N, o1, H, sm, k_prescaled=True, kmax=km1, retry=retry)
        # the un-gated branch outputs are kept: every gate trains, and d gate = sum over the group's rows of d out * y
        y_attn = e(B, N, D)
        if self.lora_out:
            To = e(B, N, self.lora.rank)
            K.gemm(o1, self.lAo, None, To, L.EPI_BIAS)
            self._lora_linear(o1, self._w("attn1.to_out.0.weight"), self._w("attn1.to_out.0.bias"), To, self.lBo, y_attn)
        else:
            K.gemm(o1, self._w("attn1.to_out.0.weight"), self._w("attn1.to_out.0.bias"), y_attn, L.EPI_BIAS)
        X1 = self._gated_add(X0, mod1, y_attn)
        mod2, t2 = self._mod(emb, 2)
        Xn2 = e(B, N, D)
        K.adaln_modulate(X1, Xn2, self._w("norm2.norm.weight"), self._w("norm2.norm.bias"), self.eps, t2)
        Fw1, Fb1, Fw2, Fb2 = (self._w(f"ff.net.{n}") for n in ("0.proj.weight", "0.proj.bias", "2.weight", "2.bias"))
        ffpre = e(B, N, Fw1.shape[0])
        if K.gemm_act_supported(N, Fw1.shape[0], D):
            ffh = e(B, N, Fw1.shape[0])
            K.gemm(Xn2, Fw1, Fb1, ffpre, L.EPI_BIAS_KEEP_GELU, residual=ffh)
        else:
            K.gemm(Xn2, Fw1, Fb1, ffpre, L.EPI_BIAS)
            ffh = _act(ffpre, gelu=True)
        y_ff = e(B, N, D)
        K.gemm(ffh, Fw2, Fb2, y_ff, L.EPI_BIAS)
        X2 = self._gated_add(X1, mod2, y_ff)
        if not self.keep:
            self.saved = None
            return X2
        self.saved = dict(X0=X0, X1=X1, Xn=Xn, Xn2=Xn2, emb=emb, t1=t1, t2=t2, mod1=mod1, mod2=mod2, qkv_pre=qkv_pre, q=q, k=k, v=v, o1=o1, lse=lse,
                          y_attn=y_attn, y_ff=y_ff, ffpre=ffpre, ffh=ffh, rope=rope, dims=(B, N, D))
        if T3 is not None:
            self.saved["T3"] = T3
        if To is not None:
            self.saved["To"] = To
        return X2

    def _put(self, grads, n, value):
        if self._tr(n):
            grads[n] = value

    def _linear_grads(self, grads, name, x2d, dy2d):
        """dW / db of the linear `name` for whichever of the two trains: the weight-gradient GEMM only for a weight that trains, the column sum alone for a
        bias whose weight is frozen (the same tg_colsum launch linear_backward makes: the same bits)."""
        if self._tr(f"{name}.weight"):
            dW, db, _ = linear_backward(x2d, dy2d)
            grads[f"{name}.weight"] = dW
            self._put(grads, f"{name}.bias", db)
        elif self._tr(f"{name}.bias"):
            grads[f"{name}.bias"] = colsum(dy2d)

    def _adapter_grads(self, names_b, names_a, dy_thirds, T, x, dT, grads):
        """lora_B gradients s dY_j^T T_j (one launch each) and lora_A gradients s dT_j^T x (ONE launch over the [3r, D] stack when all of them train),
        for the adapter tensors that train."""
        r = self.lora.rank
        for j, n in enumerate(names_b):
            if self._tr(n):
                self._lora_wgrad([n], dy_thirds[j], T[:, :, j * r:(j + 1) * r], False, grads)
        want = [self._tr(n) for n in names_a]
        if all(want):
            self._lora_wgrad(list(names_a), x, dT, True, grads)
        else:
            for j, n in enumerate(names_a):
                if want[j]:
                    self._lora_wgrad([n], x, dT[:, :, j * r:(j + 1) * r], True, grads)

    def _norm_grads(self, which, tb, dxn, tdgate, grads):
        """norm{which}: LayerNorm affine from the products over all rows; the modulation linear from d(shift, scale, gate) of the video rows and
        d(enc_shift, enc_scale, enc_gate) of the text rows of every item.  Returns d silu(temb) of this linear (fp32 [B, te])."""
        S = self.saved
        B, N, D = S["dims"]
        Nt = self.Nt
        t_dln, t_dlnx, t_dyln = tb
        dyln = t_dyln.view(B, N, D)
        mats = [t_dlnx, t_dln]
        for b in range(B):
            for lo, hi in ((Nt, N), (0, Nt)):
                mats += [dxn[b, lo:hi], dyln[b, lo:hi], tdgate[b, lo:hi]]
        # (the sums and the modulation linear's backward run whatever trains: d silu(temb) needs all of them, and dropping a matrix from the launch would
        # change the row blocking — the bits — of the others.  The [B, 6D] x [6D, te] products are negligible)
        sums = colsum_multi(mats)
        name = f"norm{which}"
        self._put(grads, f"{name}.norm.weight", sums[0])
        self._put(grads, f"{name}.norm.bias", sums[1])
        dmod = torch.stack([torch.cat(sums[2 + 6 * b:8 + 6 * b]) for b in range(B)])          # [B, 6D] in the chunk order of the linear
        dW, db, d_emb = linear_backward(S["emb"].reshape(B, -1), dmod.to(BF16).contiguous(), self._w(f"{name}.linear.weight"), need_dx=True)
        self._put(grads, f"{name}.linear.weight", dW)
        self._put(grads, f"{name}.linear.bias", db)
        return d_emb.float()

    @torch.no_grad()
    def backward(self, d_hidden, d_enc):
        """Reference block interface: gradients w.r.t. the two outputs -> (grads {name relative to the block}, d_hidden_in, d_enc_in).  The
        modulation input's gradient is left in `self.d_emb`."""
        Nt = self.Nt
        grads, dX0, self.d_emb = self.backward_x(torch.cat([d_enc, d_hidden], dim=1).to(BF16).contiguous())
        return grads, dX0[:, Nt:], dX0[:, :Nt]

    @torch.no_grad()
    def backward_x(self, dX2):
        """dX2 [B, N, D] bf16: gradient w.r.t. the output stream.  Returns (grads, dX0, d_emb fp32 [B, te])."""
        S = self.saved
        B, N, D = S["dims"]
        H, Nt = self.H, self.Nt
        grads = {}
        rows = lambda t, w: t.reshape(B * N, w)
        # ---- feed-forward residual, FeedForward, norm2 ----
        dy_ff, tg2 = _gate_res_bwd(dX2, S["y_ff"], S["t2"])
        Fw1, Fw2 = self._w("ff.net.0.proj.weight"), self._w("ff.net.2.weight")
        F4 = Fw1.shape[0]
        self._linear_grads(grads, "ff.net.2", rows(S["ffh"], F4), rows(dy_ff, D))
        dpre = _dgrad(rows(dy_ff, D), Fw2, frozen=self._frozen("ff.net.2.weight"), gelu_pre=rows(S["ffpre"], F4))      # (dy W2) * gelu'(pre-activation)
        self._linear_grads(grads, "ff.net.0.proj", rows(S["Xn2"], D), dpre)
        dXn2 = _dgrad(dpre, Fw1, frozen=self._frozen("ff.net.0.proj.weight")).view(B, N, D)
        dX1 = torch.empty(B, N, D, dtype=BF16, device=dX2.device)
        tb = _adaln_bwd(S["X1"], dXn2, dX1, self._w("norm2.norm.weight"), self._w("norm2.norm.bias"), self.eps, S["t2"], add=dX2)
        d_emb = self._norm_grads(2, tb, dXn2, tg2, grads)
        del tb, tg2, dXn2, dpre
        # ---- attention residual, to_out ----
        dy_attn, tg1 = _gate_res_bwd(dX1, S["y_attn"], S["t1"])
        self._linear_grads(grads, "attn1.to_out.0", rows(S["o1"], D), rows(dy_attn, D))
        Wo = self._w("attn1.to_out.0.weight")
        if self.lora_out:     # dT = dy B, dAO = dy W + s dT A, the adapter's own gradients (s enters in fp32: the tail's scale, the wgrad's scale)
            nA, nB = "attn1.to_out.0.lora_A.weight", "attn1.to_out.0.lora_B.weight"
            dTo = torch.empty(B, N, self.lora.rank, dtype=BF16, device=dX2.device)
            K.gemm(dy_attn, _weight_t(self.lBo, self._frozen(nB)), None, dTo, L.EPI_BIAS)
            dAO = self._lora_dgrad(dy_attn, Wo, self._frozen("attn1.to_out.0.weight"), dTo, self.lAo, self._frozen(nA))
            self._adapter_grads([nB], [nA], [dy_attn], S["To"], S["o1"], dTo, grads)
        else:
            dAO = _dgrad(rows(dy_attn, D), Wo, frozen=self._frozen("attn1.to_out.0.weight")).view(B, N, D)
        # ---- attention, QK-norm + RoPE, the fused projection: d(QKV pre-norm) written third by third (V by the attention backward's epilogue) ----
        d_pre = torch.empty(B, N, 3 * D, dtype=BF16, device=dX2.device)
        dq, dk, _ = K.attention_bwd(S["q"], S["k"], S["v"], S["o1"], dAO, H, math.log(2.0), lse=S["lse"], dv_bf16=d_pre[:, :, 2 * D:])
        _, dgq, dbq = qk_layernorm_rope_backward(S["qkv_pre"][:, :, :D], dq, H, self._w("attn1.norm_q.weight"), 1e-6, (Nt, S["rope"]), out=d_pre[:, :, :D])
        _, dgk, dbk = qk_layernorm_rope_backward(S["qkv_pre"][:, :, D:2 * D], dk, H, self._w("attn1.norm_k.weight"), 1e-6, (Nt, S["rope"]),
                                                 out_scale=LOG2E / 8.0, out=d_pre[:, :, D:2 * D])
        for n, v in (("attn1.norm_q.weight", dgq), ("attn1.norm_q.bias", dbq), ("attn1.norm_k.weight", dgk), ("attn1.norm_k.bias", dbk)):
            self._put(grads, n, v)        # (the affine sums are by-products of the input-gradient kernel)
        del dq, dk
        # the fused projection's weight gradient is ONE GEMM over the three thirds: launched when any of the three weights trains (its rows are the
        # same bits whichever of them are kept), the bias column sum likewise
        if any(self.qkv_trains[:3]):
            dW, db, _ = linear_backward(rows(S["Xn"], D), rows(d_pre, 3 * D))
        elif any(self.qkv_trains[3:]):
            dW, db = None, colsum(rows(d_pre, 3 * D))
        if any(self.qkv_trains):
            for j, n in enumerate("qkv"):
                if self.qkv_trains[j]:
                    grads[f"attn1.to_{n}.weight"] = dW[j * D:(j + 1) * D]
                if self.qkv_trains[3 + j]:
                    grads[f"attn1.to_{n}.bias"] = db[j * D:(j + 1) * D]
        wq = self._frozen([f"attn1.to_{n}.weight" for n in "qkv"], "qkv")
        if self.lora_qkv:
            r = self.lora.rank
            nA, nB = [f"attn1.to_{n}.lora_A.weight" for n in "qkv"], [f"attn1.to_{n}.lora_B.weight" for n in "qkv"]
            dT3 = torch.empty(B, N, 3 * r, dtype=BF16, device=dX2.device)
            thirds = [d_pre[:, :, j * D:(j + 1) * D] for j in range(3)]
            for j in range(3):
                K.gemm(thirds[j], _weight_t(self.lB[j], self._frozen(nB[j])), None, dT3[:, :, j * r:(j + 1) * r], L.EPI_BIAS)
            dXn = self._lora_dgrad(d_pre, self.Wqkv, wq, dT3, self.lA3, self._frozen(nA, "lA3"))
            self._adapter_grads(nB, nA, thirds, S["T3"], S["Xn"], dT3, grads)
        else:
            dXn = _dgrad(rows(d_pre, 3 * D), self.Wqkv, frozen=wq).view(B, N, D)
        # ---- norm1 ----
        dX0 = torch.empty(B, N, D, dtype=BF16, device=dX2.device)
        tb = _adaln_bwd(S["X0"], dXn, dX0, self._w("norm1.norm.weight"), self._w("norm1.norm.bias"), self.eps, S["t1"], add=dX1)
        d_emb += self._norm_grads(1, tb, dXn, tg1, grads)
        return grads, dX0, d_emb


# ---------------------------------------------------------------------------------------------------------------------------------
# The whole T2To DiT (cogvideox_transformer_3d.py:636-770, patch 1, no vip branch)
# ---------------------------------------------------------------------------------------------------------------------------------
class T2ToTrainer:
    """sd: the transformer's state dict under the reference's key names (bf16 on the GPU).  `forward` keeps each block's input stream and, while
    `activation_budget_bytes` allows, the block's intermediates; `backward` recomputes the other blocks' forward first (the reference's per-block
    gradient checkpointing, :1412-1413) and returns the gradient of every trainable parameter.  No gradient flows into patch_embed.proj or the
    latents.

    trainable_modules: the yaml's `transformer_trainable_modules` (("all",): all but patch_embed.proj — full fine-tuning; a list of name fragments;
    or empty).  lora: a lora.LoraConfig; the adapter tensors are the `*.lora_{A,B}.weight` entries of `sd` (lora.init_adapter /
    load_lora_weights).  They are applied in every forward and train when `trainable_names` selects them (lora.is_trainable, or a listed
    module).  Everything else is frozen (T2ToBlockTrainer): no weight gradient is computed for it.  Restrictions: T2ToBlockTrainer's."""

    activation_budget_bytes = None        # None: automatic (free device memory minus `activation_reserve_bytes`); 0: checkpoint every block
    activation_reserve_bytes = 40 << 30

    def __init__(self, sd, num_attention_heads, num_layers, patch_size=1, eps=1e-5, trainable_modules=("all",), lora=None):
        self.sd, self.H, self.L, self.ps, self.eps = sd, num_attention_heads, num_layers, patch_size, eps
        self.D = sd["norm_final.weight"].shape[0]
        self.lora = lora
        self.grad_sink = None         # (ParamArena, scale), set by T2ToTrainStep: the adapter gradients go straight into the arena (tg_lora_wgrad, beta = 1)
        self.fused_tail = T2ToBlockTrainer.fused_tail
        self.lora_keys = sorted(k for k in sd if is_lora_key(k) and lora.match(k.rsplit(".lora_", 1)[0])) if lora is not None else []
        for k in self.lora_keys:
            mod = k.rsplit(".lora_", 1)[0]
            if not (mod.startswith("transformer_blocks.") and mod.split(".", 2)[2] in _LORA_MODULES):
                raise NotImplementedError(f"LoRA on {mod}: the training path adapts attn1.to_q | to_k | to_v (as a group) and attn1.to_out.0 of the blocks")
        if self.lora_keys and lora.rank % 128:
            raise NotImplementedError(f"LoRA rank {lora.rank}: the training path needs a multiple of 128 (the GEMM's N granule)")
        self.trainable = trainable_names(sd, trainable_modules, lora)
        self._tset = set(self.trainable)
        params = [n for n in sd if n.startswith("transformer_blocks.") and (not is_lora_key(n) or n in self.lora_keys)]
        # every block parameter trains: the blocks run exactly the launches of full fine-tuning (T2ToBlockTrainer trainable=None)
        self._block_trainable = None if all(n in self._tset for n in params) else self._tset
        self._blocks = None
        # the frozen patch embedding, its K padded to the GEMM granule once (zeros)
        w = sd["patch_embed.proj.weight"].reshape(self.D, -1)
        self._patch_w = torch.zeros(self.D, _pad_to(w.shape[1], 64), dtype=BF16, device=w.device)
        self._patch_w[:, :w.shape[1]] = w

    def _activation_budget(self):
        if self.activation_budget_bytes is not None:
            return int(self.activation_budget_bytes)
        free, _ = torch.cuda.mem_get_info()
        free += torch.cuda.memory_reserved() - torch.cuda.memory_allocated()
        # the kept transposes of FROZEN weights (to_out, QKV, FF1, FF2 = 12 D^2 bf16 per block) are allocated in the first backward, after this budget
        # has been handed to kept activations: what is not there yet comes off the budget now
        pending = 0 if self._block_trainable is None else sum(24 * self.D * self.D for blk in (self._blocks or []) if len(blk._wt) < 4)
        return max(0, free - self.activation_reserve_bytes - pending)

    def use_arena(self, arena):
        """Make the trainable entries of the state dict views of a ParamArena (optim.py): the optimizer's writes are what the next forward reads,
        and the fused QKV weights are views (checked)."""
        for n in self.trainable:
            self.sd[n] = arena.views[n]
        self._blocks = None
        for i in range(self.L):
            blk = self._block(i, 0)
            if all(blk.qkv_trains) and not blk.fused_is_view:      # (a frozen q | k | v is a copy made once; a split one is re-made per forward)
                raise ValueError(f"block {i}: attn1.to_q/k/v are not adjacent in the arena (use t2to_arena_order)")

    def _block(self, i, n_text):
        blk = T2ToBlockTrainer(self.sd, f"transformer_blocks.{i}", self.H, n_text, self.eps, trainable=self._block_trainable, lora=self.lora)
        blk.fused_tail = self.fused_tail
        return blk

    def _want(self, n):
        return n in self._tset

    def save_lora_weights(self, lora_dir):
        """`<dir>/pytorch_lora_weights.safetensors` in the diffusers layout the reference writes: the adapter as the state dict (the parameter arena)
        holds it now."""
        from .lora import save_lora_weights
        if not self.lora_keys:
            raise RuntimeError("save_lora_weights: this trainer carries no LoRA adapter")
        return save_lora_weights(lora_dir, {n: self.sd[n] for n in self.lora_keys})

    def state_dict(self):
        """The trained transformer {name: tensor} under the reference's key names (CogVideoXTransformer3DModel.state_dict / save_pretrained)."""
        return {n: t.detach() for n, t in self.sd.items()}

    def save(self, path):
        torch.save({n: t.detach().to("cpu") for n, t in self.sd.items()}, path)

    def _front(self, latents, text, timestep):
        sd, D, ps = self.sd, self.D, self.ps
        dev = latents.device
        B, Fr, C, Hh, Ww = latents.shape
        e = lambda *s: torch.empty(*s, dtype=BF16, device=dev)
        ts = torch.as_tensor(timestep, device=dev).reshape(-1)
        ts = ts.expand(B) if ts.numel() == 1 else ts
        if ts.numel() != B:
            raise ValueError(f"the T2To recipe draws one timestep per item: got {tuple(torch.as_tensor(timestep).shape)} for batch {B}")
        sin = e(B, D)
        K.timestep_sinusoid(ts.to(torch.int64).contiguous(), D, sin)
        te = sd["time_embedding.linear_1.weight"].shape[0]
        h1, temb = e(B, te), e(B, te)
        K.gemm(sin, sd["time_embedding.linear_1.weight"], sd["time_embedding.linear_1.bias"], h1, L.EPI_BIAS)
        t1 = _act(h1)
        K.gemm(t1, sd["time_embedding.linear_2.weight"], sd["time_embedding.linear_2.bias"], temb, L.EPI_BIAS)
        emb = _act(temb).view(B, 1, te)
        hw = (Hh // ps) * (Ww // ps)
        Nt, Nv = text.shape[1], Fr * hw
        X = e(B, Nt + Nv, D)
        patches = torch.zeros(B * Nv, self._patch_w.shape[1], dtype=BF16, device=dev)
        K.patchify(latents.to(BF16).reshape(B * Fr, C, Hh, Ww).contiguous(), patches, ps)
        K.gemm(patches.view(B, Nv, -1), self._patch_w, sd["patch_embed.proj.bias"], X[:, Nt:], L.EPI_BIAS)
        txt = text.to(BF16).contiguous()
        K.gemm(txt, sd["patch_embed.text_proj.weight"], sd["patch_embed.text_proj.bias"], X[:, :Nt], L.EPI_BIAS)
        return X, dict(sin=sin, h1=h1, t1=t1, temb=temb, emb=emb, text=txt), (B, Fr, C, Hh, Ww, Nt, Nv)

    @torch.no_grad()
    def forward(self, latents, text, timestep, rope):
        """latents (the noisy model input) bf16 [B, F, C, H, W], text [B, Nt, text_dim], timestep [B], rope (cos, sin) over the F*H*W grid.
        Returns the model output [B, F, C, H, W]."""
        sd, D = self.sd, self.D
        X, front, dims = self._front(latents, text, timestep)
        B, Fr, C, Hh, Ww, Nt, Nv = dims
        dev = X.device
        if self._blocks is None or self._blocks[0].Nt != Nt:
            self._blocks = [self._block(i, Nt) for i in range(self.L)]
        for blk in self._blocks:
            blk.fused_tail = self.fused_tail
        rope = tuple(t.to(dev, torch.float32).contiguous() for t in rope)
        self._rope = rope
        emb = front["emb"]
        self._ckpt, self._kept = [], {}
        budget, per_block = self._activation_budget(), None
        for i, blk in enumerate(self._blocks):
            self._ckpt.append(X)
            blk.keep = budget > 0 and (per_block is None or budget >= per_block)
            X = blk.forward_x(X, emb, rope)
            if blk.keep:
                self._kept[i], blk.saved = blk.saved, None
                if per_block is None:
                    seen, per_block = {X.untyped_storage().data_ptr(), self._ckpt[i].untyped_storage().data_ptr()}, 0
                    for t in self._kept[i].values():
                        for u in (t if isinstance(t, (tuple, list)) else (t,)):
                            if torch.is_tensor(u) and u.untyped_storage().data_ptr() not in seen:
                                seen.add(u.untyped_storage().data_ptr())
                                per_block += u.untyped_storage().nbytes()
                budget -= per_block
        self.blocks_kept = len(self._kept)
        # final norm (per token: only the video rows reach the output), AdaLayerNorm (shift | scale, normalization.py:70-92), proj_out, unpatchify
        hidden = X[:, Nt:]
        mod = torch.empty(B, 1, 2 * D, dtype=BF16, device=dev)
        K.gemm(emb, sd["norm_out.linear.weight"], sd["norm_out.linear.bias"], mod, L.EPI_BIAS)
        tout = K.GroupTable(mod, torch.zeros(Nv, dtype=torch.uint8, device=dev), [0], [0], [D], [0])
        vidn, vid2 = torch.empty(B, Nv, D, dtype=BF16, device=dev), torch.empty(B, Nv, D, dtype=BF16, device=dev)
        K.adaln_modulate(hidden, vidn, sd["norm_final.weight"], sd["norm_final.bias"], self.eps, None)
        K.adaln_modulate(vidn, vid2, sd["norm_out.norm.weight"], sd["norm_out.norm.bias"], self.eps, tout)
        Wp, bp = sd["proj_out.weight"], sd["proj_out.bias"]
        co = Wp.shape[0]
        cop = _pad_to(co, 128)
        if cop != co:
            Wp, bp = torch.nn.functional.pad(Wp, (0, 0, 0, cop - co)), torch.nn.functional.pad(bp, (0, cop - co))
        po = torch.empty(B, Nv, cop, dtype=BF16, device=dev)
        K.gemm(vid2, Wp.contiguous(), bp.contiguous(), po, L.EPI_BIAS)
        out = torch.empty(B, Fr, co // (self.ps * self.ps), Hh, Ww, dtype=BF16, device=dev)
        K.unpatchify(po.view(B * Nv, -1), out.view(B * Fr, -1, Hh, Ww), self.ps)
        self._saved = dict(front, tout=tout, hidden_L=hidden, vidn=vidn, vid2=vid2, dims=dims)
        return out

    @torch.no_grad()
    def backward(self, d_out, on_grads=None):
        """d_out: dL/d(model output) bf16 [B, F, C, H, W].  Returns {full parameter name: gradient} of every trainable parameter.  on_grads(g):
        called with each group of gradients as soon as it is final — the final layers, then every block (last first), then the embeddings (arena
        order, t2to_arena_order) — instead of collecting them (gradient accumulation / bucketed all-reduce overlap)."""
        sd, D, S = self.sd, self.D, self._saved
        B, Fr, C, Hh, Ww, Nt, Nv = S["dims"]
        dev = d_out.device
        grads = {}
        emit = (lambda g: on_grads(g)) if on_grads is not None else grads.update
        head = {}
        # ---- proj_out, norm_out (AdaLayerNorm), norm_final ----
        co = sd["proj_out.weight"].shape[0]
        d_po = torch.empty(B * Nv, co, dtype=BF16, device=dev)
        K.patchify(d_out.to(BF16).reshape(B * Fr, -1, Hh, Ww).contiguous(), d_po, self.ps)
        want = self._want
        _linear_grads(head, "proj_out", S["vid2"].view(B * Nv, D), d_po, want)
        d_vid2 = _dgrad(d_po, sd["proj_out.weight"]).view(B, Nv, D)
        d_vidn = torch.empty(B, Nv, D, dtype=BF16, device=dev)
        t_dln, t_dlnx, t_dyln = _adaln_bwd(S["vidn"], d_vid2, d_vidn, sd["norm_out.norm.weight"], sd["norm_out.norm.bias"], self.eps, S["tout"])
        mats = [t_dlnx, t_dln]
        for b in range(B):
            mats += [d_vid2[b], t_dyln.view(B, Nv, D)[b]]
        sums = colsum_multi(mats)
        dmod = torch.stack([torch.cat(sums[2 + 2 * b:4 + 2 * b]) for b in range(B)])           # [B, 2D]: shift | scale
        dW, db, d_emb = linear_backward(S["emb"].reshape(B, -1), dmod.to(BF16).contiguous(), sd["norm_out.linear.weight"], need_dx=True)
        for n, v in (("norm_out.norm.weight", sums[0]), ("norm_out.norm.bias", sums[1]), ("norm_out.linear.weight", dW), ("norm_out.linear.bias", db)):
            if want(n):
                head[n] = v
        d_emb = d_emb.float()
        dX = torch.zeros(B, Nt + Nv, D, dtype=BF16, device=dev)                 # only the video rows of the last block's output reach the output
        t_dln, t_dlnx, _ = _adaln_bwd(S["hidden_L"], d_vidn, dX[:, Nt:], sd["norm_final.weight"], sd["norm_final.bias"], self.eps, None)
        if want("norm_final.weight") or want("norm_final.bias"):
            for n, v in zip(("norm_final.weight", "norm_final.bias"), colsum_multi([t_dlnx, t_dln])):
                if want(n):
                    head[n] = v
        del t_dln, t_dlnx, t_dyln, mats, d_vid2, d_vidn
        emit(head)
        # ---- the blocks, last first ----
        for i in reversed(range(self.L)):
            blk = self._blocks[i]
            blk.grad_sink = self.grad_sink
            if i in self._kept:
                blk.saved = self._kept.pop(i)
            else:
                blk.keep = True
                blk.forward_x(self._ckpt[i], S["emb"], self._rope)              # recompute with the intermediates kept
            g, dX, de = blk.backward_x(dX)
            blk.saved = None
            self._ckpt[i] = None
            d_emb += de
            # (adapter gradients that went straight into the arena are not in g: `sunk` names them for the caller's bucket bookkeeping)
            self.sunk = [f"transformer_blocks.{i}.{n}" for n in blk.lora_names() if blk._tr(n)] if self.grad_sink is not None else []
            emit({f"transformer_blocks.{i}.{k}": v for k, v in g.items()})
        self.sunk = []
        self._ckpt = []
        # ---- text projection, time embedding (its gradient: the sum of every AdaLN linear's input gradient, through silu) ----
        front = {}
        dtxt = dX[:, :Nt].reshape(B * Nt, D)
        _linear_grads(front, "patch_embed.text_proj", S["text"].reshape(B * Nt, -1), dtxt, want)
        if any(want(f"time_embedding.linear_{j}.{p_}") for j in (1, 2) for p_ in ("weight", "bias")):
            d_temb = (d_emb * _silu_grad(S["temb"])).to(BF16)
            dW, db, d_t1 = linear_backward(S["t1"], d_temb, sd["time_embedding.linear_2.weight"], need_dx=True)
            for n, v in (("time_embedding.linear_2.weight", dW), ("time_embedding.linear_2.bias", db)):
                if want(n):
                    front[n] = v
            d_h1 = (d_t1.float() * _silu_grad(S["h1"])).to(BF16)
            _linear_grads(front, "time_embedding.linear_1", S["sin"], d_h1, want)
        emit(front)
        self._saved = None
        return grads


def _linear_grads(grads, name, x2d, dy2d, want):
    """dW / db of the linear `name` into `grads` for whichever of the two trains (want(full name)): the weight-gradient GEMM only for a weight that
    trains; a bias alone takes the column sum linear_backward makes (the same launch, the same bits)."""
    if want(f"{name}.weight"):
        dW, db, _ = linear_backward(x2d, dy2d)
        grads[f"{name}.weight"] = dW
        if want(f"{name}.bias"):
            grads[f"{name}.bias"] = db
    elif want(f"{name}.bias"):
        grads[f"{name}.bias"] = colsum(dy2d)


def make_arena(trainer, cfg):
    """ParamArena of the trainer's trainable set in t2to_arena_order (fp32 moments for plain AdamW and for Prodigy; AdamW8bit keeps its own state), the
    trainer moved onto it, and the optimizer of the yaml's keys (optim.get_optimizer).  Returns (arena, optimizer)."""
    get = cfg.get if isinstance(cfg, dict) else (lambda k, d=None: getattr(cfg, k, d))
    eight_bit = bool(get("use_8bit_adam", False)) and str(get("optimizer", "adam")).lower() in ("adam", "adamw")
    names = trainer.trainable
    if not names:
        raise ValueError("make_arena: the trainable set is empty (transformer_trainable_modules selects nothing and no LoRA adapter trains)")
    dev = trainer.sd[names[0]].device
    arena = ParamArena({n: trainer.sd[n] for n in names}, t2to_arena_order(names, trainer.L), dev, moments=not eight_bit)
    trainer.use_arena(arena)
    return arena, get_optimizer(arena, cfg)


class T2ToTrainStep(To2VTrainStep):
    """Host mirror of the T2To loop body (train_cogvideo_t2to.py:1961-2175) for the transformer: [pca_normalization] -> add_noise -> forward
    (checkpointed) -> masked v-prediction loss -> backward -> gradient accumulation over `accumulation_steps` micro-steps (5 in the yaml) -> on
    the window's last micro-step: bucketed all-reduce (GradSync), clip_grad_norm_ over the transformer (1.0), AdamW8bit / AdamW.  Checkpoint
    (state_dict / load_state_dict), the collective failure verdict and discard_window are To2VTrainStep's."""

    def __init__(self, trainer, arena, optimizer, alphas_cumprod, accumulation_steps=5, sync=None, num_temporal_queries=4):
        super().__init__(trainer, arena, optimizer, alphas_cumprod, accumulation_steps=accumulation_steps, sync=sync)
        self.tq = int(num_temporal_queries)

    @torch.no_grad()
    def micro_step(self, noise, timesteps, text, rope, valid_num_chunks, model_input=None, condensed_tokens=None, pca=None, mean=None, std=None,
                   grid=None):
        """One micro-batch.  model_input: the normalised latents bf16 [B, F, 16, h, w]; or condensed_tokens (the frozen Resampler's output,
        [B, F, C, h, w] or token-major with grid) + pca (components_ / mean_) + mean / std, normalised here (pca_project16).  valid_num_chunks [B]:
        frames f < valid_num_chunks[b] * num_temporal_queries carry loss.  Returns (loss tensor on the device, stepped: bool)."""
        if model_input is None:
            model_input = pca_project16(condensed_tokens, pca.components_, pca.mean_, mean, std, grid)
        model_input = model_input.contiguous()
        noisy = self.add_noise(model_input, noise, timesteps).contiguous()
        out = self.tr.forward(noisy, text, timesteps, rope)
        valid = [int(c) * self.tq for c in (valid_num_chunks.tolist() if torch.is_tensor(valid_num_chunks) else valid_num_chunks)]
        loss, _, d_out = vpred_loss_and_grad_masked(out, noisy, model_input, timesteps, self.acp, valid)
        self.micro += 1
        last = self.micro % self.accum == 0
        scale = 1.0 / (self.accum * self.world)

        # adapter tensors that train: tg_lora_wgrad adds their gradients into the arena itself (no separate accumulate pass)
        direct = any(n in self.arena.offsets for n in getattr(self.tr, "lora_keys", ()))
        if direct:
            self.tr.grad_sink = (self.arena, scale)

        def done(g):
            self.arena.accumulate(g, scale)
            names = list(g) + list(getattr(self.tr, "sunk", ()))
            if last and self.sync is not None and names:
                self.sync.ready(max(self.arena.end_of(n) for n in names))
        try:
            self.tr.backward(d_out, on_grads=done)
        finally:
            if direct:
                self.tr.grad_sink = None
        self._apply_or_discard(*K.attention_bwd_status(out.device), last, out.device)
        return loss, last
