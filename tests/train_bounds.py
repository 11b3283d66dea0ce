"""fp64 CPU references and DERIVED per-element error bounds for the training backward and loss kernels (tg_attention_bwd*, tg_adaln_modulate_bwd,
tg_qk_layernorm_rope_bwd, tg_gate_residual_bwd, tg_act, tg_colsum*, tg_vpred_loss_grad*), in the conventions of tests/edge_bounds.py: every
reference restates the operation the header documents on the bits the kernel receives, in fp64 on the CPU, and returns (ref, bound); `check`
then holds EVERY element.  No term is a measured figure: each one names the kernel line (csrc/attention_bwd.hip, train.hip, elementwise.hip) whose
rounding it stands for.  tests/test_train_bounds_cpu.py pins that the bounds are satisfiable (an fp32 emulation of the documented arithmetic
passes) and sharp (one wrong key, row, column or mask frame fails); tests/test_train_edges_gpu.py holds the kernels to them.

Unit roundoffs used: bf16 2^-8 (one rounding, as in edge_bounds), fp32 2^-24; an n-term fp32 sum inside an MFMA chain (whose internal summation order is
not documented) is taken as n 2^-23 sum |terms|, a factor 2 over the textbook n 2^-24; sums whose order the source shows (lane loops, wave_sum) are counted by their depth."""
import math

import torch

from edge_bounds import F64, LOG2E, _heads, attention_lse_ref, check, d, gelu_tanh64, round_bf16, silu64, ulp_bf16  # noqa: F401  (re-exported)

LN2 = math.log(2.0)
U8, U22, U23, U24 = 2.0 ** -8, 2.0 ** -22, 2.0 ** -23, 2.0 ** -24
EXP_ULPS = 4 * U23           # v_exp_f32 (fast_exp2): 1 ulp of its result, and the fp32 rounding of its argument's last product / difference


# ------------------------------------------------------------ attention backward -----------------------------------------------------------
def _merge(t):
    return t.transpose(1, 2).reshape(t.shape[0], t.shape[2], t.shape[1] * 64)


def attention_bwd_ref(q, k, v, o, dout, H, scale):
    """q, o, dout [B, nq, H*64], k, v [B, nk, H*64] (the bf16 bits the kernel receives; O AS GIVEN, not recomputed).  Returns a dict:
    "dq" / "dk" / "dv": (ref, bound) merged to [B, n, H*64]; "p": softmax [B, H, nq, nk]; "lse": the row log-sum-exp (log2 domain) [B, H, nq].

    eps_P (relative error of the recomputed P before its bf16 rounding) = ln2 x
        [ 2^-17 (1 + log2e max_j Sm_ij)      the lse the P is normalised by: attention_lse_ref's bound — tg_attention_fwd_lse, or the statistics kernel's own
                                             running-max sum (attn_bwd_stats2_kernel `lse = M + log2f(Lsum)`), the same arithmetic
        + 64 2^-23 log2e Sm_ij               the 64-term fp32 score sum of the S MFMA chain (BWD_CONSUME 5..8 / mfma_pair) and `s * p.scale_log2`
        + 2^-22 |lse_i|                      split_bf16x3(-lse / scale_log2): the division, three truncated bf16 pieces (exact to 2^-24), and their fp32 re-summation
                                             inside the seed k-step (BWD_CONSUME(4)); the dQ kernel subtracts the fp32 lse directly (`sv * scale_log2 - lv`): one rounding
        + 4 2^-23 ]                          fast_exp2 = v_exp_f32
    dV_jd:  sum_i (2^-8 + eps_P) P_ij |dO_id|   P -> bf16 ONCE before the dV MFMA (pack_bf16x2_trans)      + nq 2^-23 sum_i P_ij |dO_id|  fp32 accumulation over the queries
    ddS_ij: (2^-8 + eps_P) |dS_ij|               dS -> bf16 before the dK / dQ MFMAs (pack_bf16x2(ds0, ds1))
            + P_ij (64 2^-23 (dPm_ij + Dm_i) + 2^-22 |D_i|)   the fp32 dP chain and the D sum (stats kernel `d += ...`) where dP - D cancels; split_bf16x3(-dsum)
    dQ_id:  scale sum_j ddS_ij |k_jd| + nk 2^-23 scale sum_j |dS_ij| |k_jd|      (the second term also covers `dq * p.scale`, the key-range join and the ordered key-block adds:
    dK_jd:  the same with q and nq                                                  each is one of at most nk fp32 additions of the same terms)"""
    qh, kh, vh, oh, gh = (_heads(t, H) for t in (q, k, v, o, dout))
    nq, nk = qh.shape[2], kh.shape[2]
    s = qh @ kh.transpose(-1, -2) * scale
    p = torch.softmax(s, dim=-1)
    dsum = (gh * oh).sum(-1, keepdim=True)
    dp = gh @ vh.transpose(-1, -2)
    ds = p * (dp - dsum)
    dv, dq, dk = p.transpose(-1, -2) @ gh, ds @ kh * scale, ds.transpose(-1, -2) @ qh * scale
    sm = qh.abs() @ kh.abs().transpose(-1, -2) * scale
    dpm = gh.abs() @ vh.abs().transpose(-1, -2)
    dm = (gh.abs() * oh.abs()).sum(-1, keepdim=True)
    lse, lse_bound = attention_lse_ref(q, k, H, scale)
    eps_p = LN2 * (lse_bound[..., None] + 64 * U23 * LOG2E * sm + U22 * lse.abs()[..., None] + EXP_ULPS)
    dv_b = ((U8 + eps_p) * p).transpose(-1, -2) @ gh.abs() + nq * U23 * (p.transpose(-1, -2) @ gh.abs())
    dds = (U8 + eps_p) * ds.abs() + p * (64 * U23 * (dpm + dm) + U22 * dsum.abs())
    dq_b = scale * (dds @ kh.abs()) + nk * U23 * scale * (ds.abs() @ kh.abs())
    dk_b = scale * (dds.transpose(-1, -2) @ qh.abs()) + nq * U23 * scale * (ds.abs().transpose(-1, -2) @ qh.abs())
    return {"dq": (_merge(dq), _merge(dq_b)), "dk": (_merge(dk), _merge(dk_b)), "dv": (_merge(dv), _merge(dv_b)), "p": p, "lse": lse}


def accumulated(ref, bound, preload):
    """accumulate modes: the kernel adds its fp32 result to what is there (`*a = add ? *a + vq : vq`, the join's `a + v`): one more fp32 rounding, taken with the
    same factor 2 as the sums: 2^-23 |preload + ref| on top."""
    tot = d(preload) + ref
    return tot, bound + U23 * tot.abs()


def as_bf16(ref, bound):
    """dv_bf16: the epilogue stores bf16 of the value the fp32 dv receives — one more 2^-8 |ref| (and 2^-8 of the error the value already carries: the rounding acts on the
    kernel's value, not on the reference)."""
    return ref, bound * (1 + U8) + U8 * ref.abs()


# ------------------------------------------------------------ LayerNorm backward core -------------------------------------------------------
def _ln_stats(x):
    D = x.shape[-1]
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return mu, var, D


def _ln_bwd(x, dxh, eps, n_sum):
    """x_hat and the LayerNorm input gradient v = rstd (dxh - mean(dxh) - x_hat mean(dxh x_hat)) in fp64 with the magnitudes their fp32 evaluation errs by.
    n_sum: the DEPTH of the kernel's row sums — the additions one value passes through: a lane adds its own terms one after the other, then wave_sum / the shuffles add
    log2(lanes) levels (tg_adaln_modulate_bwd: ceil(D / 64) terms per lane + 6 levels; tg_qk_layernorm_rope_bwd: 8 terms per lane + 3 levels).
    Returns (xh, xh_err, v, v_err):
      xh_err = (n_sum + 16) 2^-23 (1 + mean|x| rstd) (1 + |xh|)      mean and variance are such sums, `(x - mean) * rstd` then cancels against a mean that is off by up to
                                                                     n_sum 2^-24 mean|x|; 16 = the elementwise fp32 roundings of the chain
      v_err  = 2 (n_sum + 16) 2^-23 (1 + mean|x| rstd) rstd (|dxh| + mean|dxh| + (1 + |xh|) mean|dxh xh|)     the two row sums m1, m2 and the final three-term cancellation"""
    mu, var, D = _ln_stats(x)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (x - mu) * rstd
    cond = 1.0 + x.abs().mean(-1, keepdim=True) * rstd
    unit = (n_sum + 16) * U23 * cond
    xh_err = unit * (1.0 + xh.abs())
    m1, m2 = dxh.mean(-1, keepdim=True), (dxh * xh).mean(-1, keepdim=True)
    v = rstd * (dxh - m1 - xh * m2)
    mag = rstd * (dxh.abs() + dxh.abs().mean(-1, keepdim=True) + (1.0 + xh.abs()) * (dxh * xh).abs().mean(-1, keepdim=True))
    return xh, xh_err, v, 2 * unit * mag


def _near_tie(z, z_err):
    """1 where the fp64 value z lies within z_err of a bf16 rounding tie (the kernel's fp32 z may then round to the OTHER neighbour), else 0."""
    r = round_bf16(z)
    half = 0.5 * ulp_bf16(z)
    return ((half - (z - r).abs()).abs() <= z_err).to(F64)


def adaln_bwd_ref(x, dy, w, b, eps, scale=None, add=None):
    """tg_adaln_modulate_bwd (train.hip adaln_bwd_kernel / adaln_bwd_scalar_kernel — the same arithmetic).  x, dy [B, T, D]; w, b [D] or None; scale [B, T, D] gathered by the
    caller (None: modulate = 0); add [B, T, D] or None.  Returns {"dx", "t_dln", "t_dlnx", "t_dyln"}: (ref, bound), the products [B*T, D].
      dx      = bf16(v): 2^-8 |v| + v_err.   With add: bf16(bf16(v) + add) (`round_bf16(v) + a8`): ref = v + add unrounded, the two roundings 2^-8 |v| + 2^-8 |v + add|
                (+ 2^-8 of what the first stage may be off by)
      t_dln   = dy (1 + scale): `1.f + sc` and the product, 2^-23 |ref|
      t_dlnx  = t_dln x_hat: 2^-22 |ref| + |t_dln| xh_err
      t_dyln  = dy ln, ln = bf16(x_hat gamma + beta) rounded AS THE KERNEL ROUNDS IT (round_bf16 of the fp64 value): 2^-23 |ref|, and where the fp64 value lies within its fp32
                evaluation error (|gamma| xh_err + 2^-23 (|x_hat gamma| + |beta|)) of a rounding tie the kernel may hold the other neighbour: + |dy| ulp_bf16(ln) THERE only"""
    x, dy = d(x), d(dy)
    D = x.shape[-1]
    gam = torch.ones(D, dtype=F64) if w is None else d(w)
    bet = torch.zeros(D, dtype=F64) if b is None else d(b)
    one_s = torch.ones_like(x) if scale is None else 1.0 + d(scale)
    dln = dy * one_s
    xh, xh_err, v, v_err = _ln_bwd(x, dln * gam, eps, (D + 63) // 64 + 6)
    z = xh * gam + bet
    z_err = gam.abs() * xh_err + U23 * ((xh * gam).abs() + bet.abs())
    ln = round_bf16(z)
    out = {"t_dln": (dln, U23 * dln.abs()), "t_dlnx": (dln * xh, U22 * (dln * xh).abs() + dln.abs() * xh_err),
           "t_dyln": (dy * ln, U23 * (dy * ln).abs() + dy.abs() * ulp_bf16(ln) * _near_tie(z, z_err))}
    out = {n: (r.reshape(-1, D), bd.reshape(-1, D)) for n, (r, bd) in out.items()}
    if add is None:
        out["dx"] = (v, U8 * v.abs() + v_err)
    else:
        tot = v + d(add)
        out["dx"] = (tot, (U8 * v.abs() + v_err) * (1 + U8) + U8 * tot.abs())
    return out


# ------------------------------------------------------------ tg_qk_layernorm_rope_bwd ------------------------------------------------------
QK_SUM_DEPTH = 8 + 3         # train.hip: 8 elements per lane (`s += v[2 * i] + v[2 * i + 1]`), then three __shfl_xor levels over the row's 8 lanes
QK_BLOCK_ROWS = 512          # train.hip ROWS_PER_BLOCK * PASSES: (token, head) rows per block, row id = (b tokens + t) heads + h


def qk_rope_bwd_ref(x, dy, H, w, eps, segs, out_scale):
    """x [B, T, H*64] (pre-norm, bf16 bits), dy [B, T, H*64] fp32, w [64]; segs: [(start, cos [n, 64], sin [n, 64])] (fp32 tables, interleaved pairs).
    dl = rope^T(dy out_scale): pair (a, b): dl_a = dy_a c_a + dy_b s_b, dl_b = dy_b c_b - dy_a s_a (train.hip `dl[2 * i] = ya * c[2 * i] + yb * sv[2 * i + 1]`).
    Returns {"dx": (ref, bound) [B, T, H*64], "partial": (ref, bound) [blocks, 2, 64]}.
      dx       = bf16(rstd (dxh - m1 - xh m2)), dxh = dl g: 2^-8 |ref| + v_err of _ln_bwd (depth 8 + 3) + the rotation's own two products and sum, 4 2^-24 of its magnitude, through
                 the same three-term expression
      partial[blk][0][c] = sum over the block's rows of dl xh, [1][c] = sum of dl — compared BLOCK BY BLOCK.  Per row |dl|m xh_err + 4 2^-24 |dl|m |xh| (dl's roundings; |dl|m is
                 the rotation evaluated on magnitudes), and the sum's order — 16 passes per lane (`dgs[i] += dl[i] * xh[i]`), then 32 row lanes (`a += red[r][st][c]`) —
                 48 2^-24 sum |terms|."""
    x, dy, g = d(x), d(dy), d(w)
    B, T, HD = x.shape
    xr, dyr = x.reshape(B, T, H, 64), dy.reshape(B, T, H, 64) * float(out_scale)
    dl, dlm = dyr.clone(), dyr.abs()
    for start, cos, sin in segs:
        c, s = d(cos)[None, :, None, :], d(sin)[None, :, None, :]
        n = c.shape[1]
        ya, yb = dyr[:, start:start + n, :, 0::2], dyr[:, start:start + n, :, 1::2]
        dl[:, start:start + n, :, 0::2] = ya * c[..., 0::2] + yb * s[..., 1::2]
        dl[:, start:start + n, :, 1::2] = yb * c[..., 1::2] - ya * s[..., 0::2]
        dlm[:, start:start + n, :, 0::2] = (ya * c[..., 0::2]).abs() + (yb * s[..., 1::2]).abs()
        dlm[:, start:start + n, :, 1::2] = (yb * c[..., 1::2]).abs() + (ya * s[..., 0::2]).abs()
    xh, xh_err, v, v_err = _ln_bwd(xr, dl * g, eps, QK_SUM_DEPTH)
    _, _, _, rot_err = _ln_bwd(xr, dlm * g.abs(), eps, QK_SUM_DEPTH)
    dx_b = U8 * v.abs() + v_err + 4 * U24 / (2 * (QK_SUM_DEPTH + 16) * U23) * rot_err          # rot_err carries 2 (depth + 16) 2^-23: rescaled to 4 2^-24 of the same magnitude
    rows = B * T * H
    nblk = (rows + QK_BLOCK_ROWS - 1) // QK_BLOCK_ROWS
    pad = nblk * QK_BLOCK_ROWS - rows
    blk = lambda t: torch.cat([t.reshape(rows, 64), torch.zeros(pad, 64, dtype=F64)]).reshape(nblk, QK_BLOCK_ROWS, 64).sum(1)
    part = torch.stack([blk(dl * xh), blk(dl)], dim=1)
    part_b = torch.stack([blk(dlm * xh_err + 4 * U24 * dlm * xh.abs()) + 48 * U24 * blk(dlm * xh.abs()), blk(4 * U24 * dlm) + 48 * U24 * blk(dlm)], dim=1)
    return {"dx": (v.reshape(B, T, HD), dx_b.reshape(B, T, HD)), "partial": (part, part_b)}


# ------------------------------------------------------------ tg_gate_residual_bwd ----------------------------------------------------------
def gate_res_bwd_ref(dout, y_kept, gate, t_row0):
    """dy = bf16(gate dout), t_dgate = dout y (fp32) for the rows >= t_row0; y_kept [B, T - t_row0, D] holds only those rows.  The product of two bf16 values has 16
    significant bits: EXACT in fp32 (train.hip `o[k] = ga[k] * d[k]`, `dst[k] = d[k] * yv[k]`), so dy is ONE rounding of the exact product — identical to round_bf16 of the
    fp64 product — and t_dgate is the exact product: both bounds are zero (check() then demands equality)."""
    dout, gate, y = d(dout), d(gate), d(y_kept)
    dy = round_bf16(gate * dout)
    tg = dout[:, t_row0:] * y
    return {"dy": (dy, torch.zeros_like(dy)), "t_dgate": (tg, torch.zeros_like(tg))}


# ------------------------------------------------------------------- tg_act -----------------------------------------------------------------
K0, K1 = 0.7978845608028654, 0.044715


def gelu_tanh_grad64(x):
    """d/dx of 0.5 x (1 + tanh(u)), u = k0 (x + k1 x^3), in fp64."""
    th = torch.tanh(K0 * (x + K1 * x ** 3))
    return 0.5 * (1.0 + th) + 0.5 * x * (1.0 - th * th) * K0 * (1.0 + 3.0 * K1 * x * x)


def act_ref(x, dy, mode):
    """tg_act (train.hip act_one; common.h gelu_tanh / gelu_tanh_bwd).  Modes 0 (silu) and 2 (gelu_tanh): edge_bounds.gemm_act's bound — one bf16 rounding and the
    1 / (1 + e^-x) cancellation as 8 ulp of 1 times max(|x|, 1).  Mode 1, dy gelu'(x) with th = 1 - 2 rcp(1 + exp2(..)): th is off by at most 8 ulp of 1 (v_exp, v_rcp, the
    1 - 2 r cancellation), the expression's sensitivity to th is <= 1/2 + |x| k0 (1 + 3 k1 x^2); its own products add 2^-21 of the same magnitude:
    2^-8 |ref| + 2^-20 |dy| (1 + |x| k0 (1 + 3 k1 x^2))."""
    x = d(x)
    if mode in (0, 2):
        ref = (silu64 if mode == 0 else gelu_tanh64)(x)
        return ref, U8 * ref.abs() + 2.0 ** -20 * x.abs().clamp_min(1.0)
    dy = d(dy)
    ref = dy * gelu_tanh_grad64(x)
    return ref, U8 * ref.abs() + 2.0 ** -20 * dy.abs() * (1.0 + x.abs() * K0 * (1.0 + 3.0 * K1 * x * x))


# ------------------------------------------------------------------ tg_colsum* --------------------------------------------------------------
def colsum_block_rows(rows, cols):
    """train.hip cs_rows: rows per block of tg_colsum / tg_colsum_f32 — "256 rows per block for tall matrices, fewer for short ones, a function of (rows, cols) only"."""
    cb = (cols + 255) // 256
    return int(min(256, max(8, (rows * cb + 2047) // 2048)))


def colsum_ref(src, per):
    """partial[blk][c] = sum of src[r][c] over rows blk*per .. min(rows, (blk+1)*per) - 1, every partial row; bound rows_in_block 2^-24 sum |src| (`a += ...` in row order; a
    block of one row is exact).  Blocks past the last row (tg_colsum_multi with more row blocks than rows) are zero with a zero bound."""
    s = d(src)
    rows, cols = s.shape
    nblk = (rows + per - 1) // per
    sp = torch.cat([s, torch.zeros(nblk * per - rows, cols, dtype=F64)]).view(nblk, per, cols)
    n_in = torch.tensor([min(per, rows - i * per) for i in range(nblk)], dtype=F64).view(nblk, 1)
    return sp.sum(1), torch.where(n_in > 1, n_in, torch.zeros_like(n_in)) * U24 * sp.abs().sum(1)


def colsum_multi_ref(mats, row_blocks):
    """tg_colsum_multi: item i is cut into `row_blocks` blocks of ceil(rows_i / row_blocks) rows (colsum_multi_kernel `per`); partial [row_blocks][sum of cols]."""
    refs, bounds = [], []
    for m in mats:
        per = (m.shape[0] + row_blocks - 1) // row_blocks
        r, bd = colsum_ref(m, per)
        padr = row_blocks - r.shape[0]
        refs.append(torch.cat([r, torch.zeros(padr, r.shape[1], dtype=F64)]))
        bounds.append(torch.cat([bd, torch.zeros(padr, r.shape[1], dtype=F64)]))
    return torch.cat(refs, dim=1), torch.cat(bounds, dim=1)


# --------------------------------------------------------------- loss kernels ---------------------------------------------------------------
LOSS_SUM_DEPTH = 1 + 6 + 2   # elementwise.hip: the term's own product, wave_sum's six levels, `(red[0] + red[1]) + (red[2] + red[3])`
def vpred_loss_ref(out, noisy, target, coef, inv_count, valid_frames=None, frames=None):
    """tg_vpred_loss_grad (valid_frames None; inv_count: the fp32 value handed to the kernel) / tg_vpred_loss_grad_masked (valid_frames: [batch] ints, frames per item;
    inv_count_b = fp32(1 / (valid_b E batch))).  out / noisy / target [F, E] bf16 bits, coef [F, 3] fp32.  The header's chain, every step restated:
        sa, sb = bf16(coef)            pred = bf16(bf16(sa noisy) - bf16(sb out))       diff = bf16(pred - target)        sq = bf16(diff^2)
    Products of two bf16 values and differences of bf16 values this close are exact in fp32, so each round_bf16 of the fp64 value IS the kernel's value: no allowance.
        grad = bf16(-sb (2 w diff inv_count)): ONE bf16 rounding of the last product, 2^-8 |ref|, + 2^-21 |ref| for its three fp32 products
        partial[f][blk] = sum over the block's 256 elements of w sq: 2^-24 per term (`w * round_bf16(diff * diff)`) and the wave_sum / red[] tree: depth 9, 9 2^-24 sum |terms|
    Masked frames: grad and partials EXACTLY zero (zero bound).  Returns {"grad": (ref, bound) [F, E], "partial": (ref, bound) [F, ceil(E / 256)]}."""
    out, noisy, target, coef = d(out), d(noisy), d(target), d(coef.float())
    F, E = out.shape
    sa, sb, w = round_bf16(coef[:, 0:1].clone()), round_bf16(coef[:, 1:2].clone()), coef[:, 2:3]
    pred = round_bf16(round_bf16(sa * noisy) - round_bf16(sb * out))
    diff = round_bf16(pred - target)
    term = w * round_bf16(diff * diff)
    if valid_frames is None:
        inv = torch.full((F, 1), float(torch.tensor(inv_count, dtype=torch.float32)), dtype=F64)
        live = torch.ones(F, 1, dtype=F64)
    else:
        batch = len(valid_frames)
        assert F == batch * frames
        inv = torch.tensor([float(torch.tensor(1.0 / (max(vb, 1) * E * batch), dtype=torch.float32)) for vb in valid_frames for _ in range(frames)], dtype=F64).view(F, 1)
        live = torch.tensor([1.0 if fl < vb else 0.0 for vb in valid_frames for fl in range(frames)], dtype=F64).view(F, 1)
    grad = -sb * (2.0 * w * diff * inv) * live
    term = term * live
    nblk = (E + 255) // 256
    tp = torch.cat([term, torch.zeros(F, nblk * 256 - E, dtype=F64)], dim=1).view(F, nblk, 256)
    return {"grad": (grad, (U8 + 2.0 ** -21) * grad.abs()), "partial": (tp.sum(-1), LOSS_SUM_DEPTH * U24 * tp.abs().sum(-1))}
