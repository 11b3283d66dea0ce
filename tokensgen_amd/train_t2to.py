"""T2To training step on the gfx950 kernels: full fine-tuning of the token-grid DiT (reference loop train_cogvideo_t2to.py:1961-2175 with
config/train/cogvideo_5b_vaevip_4x8x12_t2to.yaml).

`vpred_loss_and_grad_masked` (the masked, per-item normalised v-prediction loss, :2125-2166), `pca_project16` (the PCA normalisation of the
condensed tokens, :1761-1773), `T2ToBlockTrainer` (one plain CogVideoXBlock: forward with the intermediates kept, backward to EVERY block parameter
and to the block inputs), `T2ToTrainer` (the whole patch-1 model: embeddings, 42 blocks, final layers; activations kept while memory allows, the
other blocks recomputed), `t2to_arena_order` and `T2ToTrainStep` (add_noise -> forward -> masked loss -> backward -> gradient arena -> accumulate
/ all-reduce / clip / AdamW8bit through tokensgen_amd.optim).

Trainable set (:1531-1560, `transformer_trainable_modules: ["all"]`): every transformer parameter whose name does not contain "patch_embed.proj".
No attention mask is applied: the loop passes `attention_kwargs={"attention_mask": ...}` (:2122) but the transformer pops "attention_masks"
(cogvideox_transformer_3d.py:653), so padded frames enter attention as ordinary tokens; only the loss is masked.  The forward-only product never
routes through this module."""
import math

import numpy as np
import torch

from . import kernels as K
from . import lib as L
from .optim import ParamArena, get_optimizer
from .train import (BF16, LOG2E, To2VTrainStep, _act, _adaln_bwd, _cat_or_view, _dgrad, _fast_attention_ws, _gate_res_bwd, _pad_to, _tok_group,
                    _vpred_coef, _vt_scratch, colsum_multi, linear_backward, qk_layernorm_rope_backward)

FROZEN = "patch_embed.proj"          # the one frozen name fragment of the recipe (:1547)
_QKV_ORDER = ("attn1.to_q.weight", "attn1.to_k.weight", "attn1.to_v.weight", "attn1.to_q.bias", "attn1.to_k.bias", "attn1.to_v.bias")
_HEAD = ("norm_final.", "norm_out.", "proj_out.")


def trainable_names(names):
    """train_cogvideo_t2to.py:1544-1548 with transformer_trainable_modules ["all"]: every name that does not contain "patch_embed.proj"."""
    return sorted(n for n in names if FROZEN not in n)


def t2to_arena_order(names, num_layers):
    """Arena order of the T2To trainable set = the order gradients become final in the backward: the final layers (norm_final, norm_out,
    proj_out) first, then the blocks from the last to the first, then the embeddings (patch_embed.text_proj, time_embedding).  Inside a block
    attn1.to_{q,k,v} weights and biases lead, adjacent, so that the fused [3D, D] projection weight is a view of the arena."""
    def block_key(n):
        for j, pat in enumerate(_QKV_ORDER):
            if n.endswith(pat):
                return (0, j, n)
        return (1, 0, n)
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
    this block).  sd: the state dict under the reference's names (bf16 on the GPU; views of the parameter arena in the training step).  All
    weights train, so no transpose is cached: every dgrad transposes the weight it reads NOW (an optimizer step writes the arena through raw
    pointers without bumping tensor versions)."""

    def __init__(self, sd, pre, heads, n_text, eps=1e-5):
        self.sd, self.pre, self.H, self.Nt, self.eps = sd, pre, heads, n_text, eps
        self.keep = True
        g = lambda n: sd[f"{pre}.{n}"]
        self.Wqkv = _cat_or_view([g(f"attn1.to_{n}.weight") for n in "qkv"])       # views of the arena when q, k, v are adjacent there
        self.bqkv = _cat_or_view([g(f"attn1.to_{n}.bias") for n in "qkv"])
        self.fused_is_view = (self.Wqkv.data_ptr() == g("attn1.to_q.weight").data_ptr() and self.bqkv.data_ptr() == g("attn1.to_q.bias").data_ptr())

    def _w(self, n):
        return self.sd[f"{self.pre}.{n}"]

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
        mod1, t1 = self._mod(emb, 1)
        Xn = e(B, N, D)
        K.adaln_modulate(X0, Xn, self._w("norm1.norm.weight"), self._w("norm1.norm.bias"), self.eps, t1)
        qkv_pre = e(B, N, 3 * D)
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
        return X2

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
        sums = colsum_multi(mats)
        name = f"norm{which}"
        grads[f"{name}.norm.weight"], grads[f"{name}.norm.bias"] = sums[0], sums[1]
        dmod = torch.stack([torch.cat(sums[2 + 6 * b:8 + 6 * b]) for b in range(B)])          # [B, 6D] in the chunk order of the linear
        dW, db, d_emb = linear_backward(S["emb"].reshape(B, -1), dmod.to(BF16).contiguous(), self._w(f"{name}.linear.weight"), need_dx=True)
        grads[f"{name}.linear.weight"], grads[f"{name}.linear.bias"] = dW, db
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
        grads["ff.net.2.weight"], grads["ff.net.2.bias"], _ = linear_backward(rows(S["ffh"], F4), rows(dy_ff, D))
        dpre = _dgrad(rows(dy_ff, D), Fw2, gelu_pre=rows(S["ffpre"], F4))                 # (dy W2) * gelu'(pre-activation)
        grads["ff.net.0.proj.weight"], grads["ff.net.0.proj.bias"], _ = linear_backward(rows(S["Xn2"], D), dpre)
        dXn2 = _dgrad(dpre, Fw1).view(B, N, D)
        dX1 = torch.empty(B, N, D, dtype=BF16, device=dX2.device)
        tb = _adaln_bwd(S["X1"], dXn2, dX1, self._w("norm2.norm.weight"), self._w("norm2.norm.bias"), self.eps, S["t2"], add=dX2)
        d_emb = self._norm_grads(2, tb, dXn2, tg2, grads)
        del tb, tg2, dXn2, dpre
        # ---- attention residual, to_out ----
        dy_attn, tg1 = _gate_res_bwd(dX1, S["y_attn"], S["t1"])
        grads["attn1.to_out.0.weight"], grads["attn1.to_out.0.bias"], _ = linear_backward(rows(S["o1"], D), rows(dy_attn, D))
        dAO = _dgrad(rows(dy_attn, D), self._w("attn1.to_out.0.weight")).view(B, N, D)
        # ---- attention, QK-norm + RoPE, the fused projection: d(QKV pre-norm) written third by third (V by the attention backward's epilogue) ----
        d_pre = torch.empty(B, N, 3 * D, dtype=BF16, device=dX2.device)
        dq, dk, _ = K.attention_bwd(S["q"], S["k"], S["v"], S["o1"], dAO, H, math.log(2.0), lse=S["lse"], dv_bf16=d_pre[:, :, 2 * D:])
        _, grads["attn1.norm_q.weight"], grads["attn1.norm_q.bias"] = qk_layernorm_rope_backward(
            S["qkv_pre"][:, :, :D], dq, H, self._w("attn1.norm_q.weight"), 1e-6, (Nt, S["rope"]), out=d_pre[:, :, :D])
        _, grads["attn1.norm_k.weight"], grads["attn1.norm_k.bias"] = qk_layernorm_rope_backward(
            S["qkv_pre"][:, :, D:2 * D], dk, H, self._w("attn1.norm_k.weight"), 1e-6, (Nt, S["rope"]), out_scale=LOG2E / 8.0, out=d_pre[:, :, D:2 * D])
        del dq, dk
        dW, db, _ = linear_backward(rows(S["Xn"], D), rows(d_pre, 3 * D))
        for j, n in enumerate("qkv"):
            grads[f"attn1.to_{n}.weight"], grads[f"attn1.to_{n}.bias"] = dW[j * D:(j + 1) * D], db[j * D:(j + 1) * D]
        dXn = _dgrad(rows(d_pre, 3 * D), self.Wqkv).view(B, N, D)
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
    gradient checkpointing, :1412-1413) and returns the gradient of every trainable parameter (all but patch_embed.proj).  No gradient flows into
    patch_embed.proj or the latents."""

    activation_budget_bytes = None        # None: automatic (free device memory minus `activation_reserve_bytes`); 0: checkpoint every block
    activation_reserve_bytes = 40 << 30

    def __init__(self, sd, num_attention_heads, num_layers, patch_size=1, eps=1e-5):
        self.sd, self.H, self.L, self.ps, self.eps = sd, num_attention_heads, num_layers, patch_size, eps
        self.D = sd["norm_final.weight"].shape[0]
        self.trainable = trainable_names(sd)
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
        return max(0, free - self.activation_reserve_bytes)

    def use_arena(self, arena):
        """Make the trainable entries of the state dict views of a ParamArena (optim.py): the optimizer's writes are what the next forward reads,
        and the fused QKV weights are views (checked)."""
        for n in self.trainable:
            self.sd[n] = arena.views[n]
        self._blocks = None
        for i in range(self.L):
            if not T2ToBlockTrainer(self.sd, f"transformer_blocks.{i}", self.H, 0, self.eps).fused_is_view:
                raise ValueError(f"block {i}: attn1.to_q/k/v are not adjacent in the arena (use t2to_arena_order)")

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
            self._blocks = [T2ToBlockTrainer(sd, f"transformer_blocks.{i}", self.H, Nt, self.eps) for i in range(self.L)]
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
        head["proj_out.weight"], head["proj_out.bias"], _ = linear_backward(S["vid2"].view(B * Nv, D), d_po)
        d_vid2 = _dgrad(d_po, sd["proj_out.weight"]).view(B, Nv, D)
        d_vidn = torch.empty(B, Nv, D, dtype=BF16, device=dev)
        t_dln, t_dlnx, t_dyln = _adaln_bwd(S["vidn"], d_vid2, d_vidn, sd["norm_out.norm.weight"], sd["norm_out.norm.bias"], self.eps, S["tout"])
        mats = [t_dlnx, t_dln]
        for b in range(B):
            mats += [d_vid2[b], t_dyln.view(B, Nv, D)[b]]
        sums = colsum_multi(mats)
        head["norm_out.norm.weight"], head["norm_out.norm.bias"] = sums[0], sums[1]
        dmod = torch.stack([torch.cat(sums[2 + 2 * b:4 + 2 * b]) for b in range(B)])           # [B, 2D]: shift | scale
        head["norm_out.linear.weight"], head["norm_out.linear.bias"], d_emb = linear_backward(S["emb"].reshape(B, -1), dmod.to(BF16).contiguous(),
                                                                                              sd["norm_out.linear.weight"], need_dx=True)
        d_emb = d_emb.float()
        dX = torch.zeros(B, Nt + Nv, D, dtype=BF16, device=dev)                 # only the video rows of the last block's output reach the output
        t_dln, t_dlnx, _ = _adaln_bwd(S["hidden_L"], d_vidn, dX[:, Nt:], sd["norm_final.weight"], sd["norm_final.bias"], self.eps, None)
        head["norm_final.weight"], head["norm_final.bias"] = colsum_multi([t_dlnx, t_dln])
        del t_dln, t_dlnx, t_dyln, mats, d_vid2, d_vidn
        emit(head)
        # ---- the blocks, last first ----
        for i in reversed(range(self.L)):
            blk = self._blocks[i]
            if i in self._kept:
                blk.saved = self._kept.pop(i)
            else:
                blk.keep = True
                blk.forward_x(self._ckpt[i], S["emb"], self._rope)              # recompute with the intermediates kept
            g, dX, de = blk.backward_x(dX)
            blk.saved = None
            self._ckpt[i] = None
            d_emb += de
            emit({f"transformer_blocks.{i}.{k}": v for k, v in g.items()})
        self._ckpt = []
        # ---- text projection, time embedding (its gradient: the sum of every AdaLN linear's input gradient, through silu) ----
        front = {}
        dtxt = dX[:, :Nt].reshape(B * Nt, D)
        front["patch_embed.text_proj.weight"], front["patch_embed.text_proj.bias"], _ = linear_backward(S["text"].reshape(B * Nt, -1), dtxt)
        d_temb = (d_emb * _silu_grad(S["temb"])).to(BF16)
        front["time_embedding.linear_2.weight"], front["time_embedding.linear_2.bias"], d_t1 = linear_backward(
            S["t1"], d_temb, sd["time_embedding.linear_2.weight"], need_dx=True)
        d_h1 = (d_t1.float() * _silu_grad(S["h1"])).to(BF16)
        front["time_embedding.linear_1.weight"], front["time_embedding.linear_1.bias"], _ = linear_backward(S["sin"], d_h1)
        emit(front)
        self._saved = None
        return grads


def make_arena(trainer, cfg):
    """ParamArena of the trainer's trainable set in t2to_arena_order (fp32 moments only for plain AdamW; AdamW8bit keeps its own state), the
    trainer moved onto it, and the optimizer of the yaml's keys (optim.get_optimizer).  Returns (arena, optimizer)."""
    get = cfg.get if isinstance(cfg, dict) else (lambda k, d=None: getattr(cfg, k, d))
    eight_bit = bool(get("use_8bit_adam", False)) and str(get("optimizer", "adam")).lower() in ("adam", "adamw")
    names = trainer.trainable
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

        def done(g):
            self.arena.accumulate(g, scale)
            if last and self.sync is not None:
                self.sync.ready(max(self.arena.end_of(n) for n in g))
        self.tr.backward(d_out, on_grads=done)
        self._apply_or_discard(*K.attention_bwd_status(out.device), last, out.device)
        return loss, last
