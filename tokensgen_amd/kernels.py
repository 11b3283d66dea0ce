"""torch-tensor front end of the C ABI (include/tokensgen_hip.h).  Plumbing only: device memory comes from
torch, launches go on torch's current HIP stream.  Every function requires bf16 CUDA(HIP) tensors; there is
no CPU path."""
import ctypes as C
import os

import torch

from . import lib as L

BF16 = torch.bfloat16


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _chk(t, name, dtype=BF16):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name}: expected a GPU tensor (tokensgen_amd has no CPU fallback)")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if t.stride(-1) != 1:
        raise ValueError(f"{name}: innermost dimension must be contiguous")
    return t


def _p(t):
    return 0 if t is None else t.data_ptr()


# Optional per-launch timing with HIP events recorded on the launch stream (bench.py's roofline leg).
PROFILE_ON = [False]
PROFILE = {}


PROFILE_FILTER = [None]      # None: time every launch; a set of names: only those (fewer event markers in a timed region)


def _launch(name, fn, *args):
    if not PROFILE_ON[0] or (PROFILE_FILTER[0] is not None and name not in PROFILE_FILTER[0]):
        return fn(*args)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    code = fn(*args)
    e.record()
    PROFILE.setdefault(name, []).append((s, e))
    return code


def profile_summary():
    """{kernel name: {"ms": mean launch duration, "n": launches, "total_ms": sum}} from the recorded events."""
    torch.cuda.synchronize()
    out = {}
    for name, evs in PROFILE.items():
        ms = [s.elapsed_time(e) for s, e in evs]
        out[name] = {"ms": sum(ms) / len(ms), "n": len(ms), "total_ms": sum(ms)}
    return out


class GroupTable:
    """Host mirror of tg_group_table: token -> (modulation row, shift/scale/gate column)."""

    def __init__(self, mod, tok_group, rows, shift_cols, scale_cols, gate_cols, tok_offset=0):
        _chk(mod, "mod")
        assert mod.dim() == 3, "mod must be [batch, rows, cols]"
        _chk(tok_group, "tok_group", torch.uint8)
        self.mod, self.tok_group = mod, tok_group
        self.c = L.GroupTable()
        self.c.mod = mod.data_ptr()
        self.c.mod_ld = mod.stride(1)
        self.c.mod_batch_stride = mod.stride(0)
        self.c.tok_group = tok_group.data_ptr() + tok_offset
        n = len(rows)
        assert n <= L.TG_MAX_GROUPS
        for i in range(n):
            self.c.row[i], self.c.shift_col[i], self.c.scale_col[i], self.c.gate_col[i] = (
                int(rows[i]), int(shift_cols[i]), int(scale_cols[i]), int(gate_cols[i]))
        self.rows, self.shift_cols, self.scale_cols, self.gate_cols = list(rows), list(shift_cols), list(scale_cols), list(gate_cols)

    def offset(self, tok_offset):
        """Same table, token indices shifted (for launches that start at a later token)."""
        return GroupTable(self.mod, self.tok_group, self.rows, self.shift_cols, self.scale_cols, self.gate_cols, tok_offset)

    def ref(self):
        return C.byref(self.c)


def _bmk(t):
    """View a [M,K] or [B,M,K] tensor as (batch, M, K, ld, batch_stride)."""
    if t.dim() == 2:
        return 1, t.shape[0], t.shape[1], t.stride(0), 0
    if t.dim() == 3:
        return t.shape[0], t.shape[1], t.shape[2], t.stride(1), t.stride(0)
    raise ValueError("expected a 2-D or 3-D tensor")


def gemm(a, w, bias, out, epilogue=L.EPI_BIAS, residual=None, gate=None):
    """out = epilogue(a @ w.T + bias); a [..,M,K], w [N,K] (nn.Linear layout), out [..,M,N] (views allowed)."""
    _chk(a, "a"); _chk(w, "w"); _chk(out, "out")
    B, M, K, lda, sa = _bmk(a)
    Bo, Mo, N, ldc, sc = _bmk(out)
    if (B, M) != (Bo, Mo) or w.shape != (N, K):
        raise ValueError(f"gemm: shape mismatch a{tuple(a.shape)} w{tuple(w.shape)} out{tuple(out.shape)}")
    if bias is not None:
        _chk(bias, "bias")
    ldr = sr = 0
    if residual is not None:
        _chk(residual, "residual")
        _, _, _, ldr, sr = _bmk(residual)
    L.check(_launch(f"gemm_M{M}_N{N}_K{K}_epi{epilogue}", L.load().tg_gemm_bf16, _p(a), lda, sa, _p(w), w.stride(0), _p(bias), _p(out), ldc, sc, M, N, K, B, epilogue,
                                  _p(residual), ldr, sr, gate.ref() if gate is not None else None, _stream()), "tg_gemm_bf16")
    return out


def gemm_act_supported(M, N, K, lda=0, ldw=0):
    """Shapes that have the training step's activation epilogues (EPI_BIAS_KEEP_GELU: `residual` is the second OUTPUT, gelu of the kept pre-activation;
    EPI_BIAS_MUL_GELU_GRAD: `residual` is the kept pre-activation): the 4-wave GEMM kernel's.  Elsewhere: gemm(EPI_BIAS) + tg_act."""
    return L.gemm_kernel(M, N, K, lda, ldw) == 2


def gemm_lora_supported(M, N, K, R, lda=0, ldw=0, ldt=0, ldb=0):
    """Shapes tg_gemm_bf16_lora takes.  Elsewhere: gemm(EPI_BIAS) + the accumulating gemm(EPI_BIAS_GATE_RES) with a gate table that holds the scale."""
    return L.gemm_kernel(M, N, K, lda, ldw) == 2 and R % 64 == 0 and 64 <= R <= 384 and max(ldt, ldb) < (1 << 21)


def gemm_lora(a, w, bias, t, b, scale, out):
    """out = bf16(a @ w.T + bias + scale * (t @ b.T)) in one launch (tg_gemm_bf16_lora): a [.., M, K], w [N, K], t [.., M, R] (the adapter's down-projection),
    b [N, R] (lora_B), scale a Python float (applied in fp32), out [.., M, N]; views with row / batch strides allowed.  Shapes: gemm_lora_supported."""
    _chk(a, "a"); _chk(w, "w"); _chk(t, "t"); _chk(b, "b"); _chk(out, "out")
    B, M, K, lda, sa = _bmk(a)
    Bt, Mt, R, ldt, st = _bmk(t)
    Bo, Mo, N, ldc, sc = _bmk(out)
    if (B, M) != (Bo, Mo) or (B, M) != (Bt, Mt) or w.shape != (N, K) or b.shape != (N, R):
        raise ValueError(f"gemm_lora: shape mismatch a{tuple(a.shape)} w{tuple(w.shape)} t{tuple(t.shape)} b{tuple(b.shape)} out{tuple(out.shape)}")
    if bias is not None:
        _chk(bias, "bias")
    L.check(_launch(f"gemm_lora_M{M}_N{N}_K{K}_R{R}", L.load().tg_gemm_bf16_lora, _p(a), lda, sa, _p(w), w.stride(0), _p(bias), _p(t), ldt, st, _p(b), b.stride(0),
                    float(scale), _p(out), ldc, sc, M, N, K, R, B, _stream()), "tg_gemm_bf16_lora")
    return out


def gemm_pair_supported(M1, M2, N, K):
    return L.gemm_kernel(M1, N, K) >= 1 and L.gemm_kernel(M2, N, K) >= 1


def gemm_pair(a1, w1, bias1, out1, a2, w2, bias2, out2, epilogue=L.EPI_BIAS):
    """out1 = epi(a1 @ w1^T + bias1) and out2 = epi(a2 @ w2^T + bias2) in one launch (tg_gemm_bf16_pair): same N, K, batch, leading
    dimensions; both problems on a 256x256 kernel (gemm_pair_supported)."""
    for n, t in (("a1", a1), ("w1", w1), ("out1", out1), ("a2", a2), ("w2", w2), ("out2", out2)):
        _chk(t, n)
    B, M1, Kd, lda, sa1 = _bmk(a1)
    B2, M2, Kd2, lda2, sa2 = _bmk(a2)
    _, _, N, ldc, sc1 = _bmk(out1)
    _, _, N2, ldc2, sc2 = _bmk(out2)
    assert (B, Kd, lda, N, ldc) == (B2, Kd2, lda2, N2, ldc2) and w1.shape == w2.shape == (N, Kd) and w1.stride(0) == w2.stride(0)
    L.check(_launch(f"gemm_pair_M{M1}+{M2}_N{N}_K{Kd}_epi{epilogue}", L.load().tg_gemm_bf16_pair, _p(a1), sa1, _p(w1), _p(bias1), _p(out1), sc1, M1,
                    _p(a2), sa2, _p(w2), _p(bias2), _p(out2), sc2, M2, lda, w1.stride(0), ldc, N, Kd, B, epilogue, _stream()), "tg_gemm_bf16_pair")
    return out1, out2


def gemm_qkv_supported(M, N, K, v_col0):
    """Shapes the fused QKV + V^T launch (tg_gemm_bf16_qkv) takes; TG_GEMM_W4=0 (the cross-check tests' switch to the 8-wave GEMM) disables it too."""
    return L.gemm_kernel(M, N, K) == 2 and v_col0 % 256 == 0 and 0 < v_col0 < N


def gemm_qkv(a1, w1, bias1, out1, vt1, a2=None, w2=None, bias2=None, out2=None, vt2=None, v_col0=None):
    """QKV projection(s) with the V third (columns >= v_col0, default 2N/3) written transposed into vt [B, H, 64, ld] instead of out
    (tg_gemm_bf16_qkv): out[:, :, :v_col0] = a @ w[:v_col0]^T + bias, vt[b, h, d, m] = (a @ w^T + bias)[b, m, v_col0 + 64 h + d], zero for
    m >= M.  One or two problems (same N, K, batch, leading dimensions) in one launch."""
    two = a2 is not None
    for n, t in (("a1", a1), ("w1", w1), ("out1", out1), ("vt1", vt1)) + ((("a2", a2), ("w2", w2), ("out2", out2), ("vt2", vt2)) if two else ()):
        _chk(t, n)
    B, M1, Kd, lda, sa1 = _bmk(a1)
    _, _, N, ldc, sc1 = _bmk(out1)
    v_col0 = 2 * N // 3 if v_col0 is None else v_col0
    assert w1.shape == (N, Kd)

    def vt_ld(vt, M):
        assert vt.dim() == 4 and vt.shape[0] == B and vt.shape[1] * vt.shape[2] == N - v_col0 and vt.is_contiguous() and vt.shape[3] >= M
        return vt.shape[3]
    ld1 = vt_ld(vt1, M1)
    M2 = sa2 = sc2 = ld2 = 0
    if two:
        B2, M2, Kd2, lda2, sa2 = _bmk(a2)
        _, _, N2, ldc2, sc2 = _bmk(out2)
        assert (B, Kd, lda, N, ldc) == (B2, Kd2, lda2, N2, ldc2) and w2.shape == (N, Kd) and w1.stride(0) == w2.stride(0)
        ld2 = vt_ld(vt2, M2)
    name = f"gemm_qkv_M{M1}+{M2}_N{N}_K{Kd}" if two else f"gemm_qkv_M{M1}_N{N}_K{Kd}"
    L.check(_launch(name, L.load().tg_gemm_bf16_qkv, _p(a1), sa1, _p(w1), _p(bias1), _p(out1), sc1, M1, _p(vt1), ld1,
                    _p(a2) if two else None, sa2, _p(w2) if two else None, _p(bias2) if two else None, _p(out2) if two else None, sc2, M2,
                    _p(vt2) if two else None, ld2, lda, w1.stride(0), ldc, N, Kd, B, v_col0, _stream()), "tg_gemm_bf16_qkv")
    return out1, vt1


def adaln_modulate(x, out, ln_weight, ln_bias, eps, table=None):
    """out = LN(x)*(1+scale[g])+shift[g] (table given) or plain affine LN (table None). x/out [B,T,D] views."""
    _chk(x, "x"); _chk(out, "out")
    B, T, D, ldx, sx = _bmk(x)
    _, _, _, ldy, sy = _bmk(out)
    L.check(_launch("adaln_modulate", L.load().tg_adaln_modulate, _p(x), ldx, sx, _p(out), ldy, sy, _p(ln_weight), _p(ln_bias), float(eps), T, D, B,
                                       1 if table is not None else 0, table.ref() if table is not None else None,
                                       _stream()), "tg_adaln_modulate")
    return out


def qk_layernorm_rope(x, heads, ln_weight, ln_bias, eps, seg0=None, seg1=None, out_scale=1.0):
    """In place on x [B,T,heads*64] (a column slice of the fused QKV buffer). seg = (start, (cos, sin))."""
    _chk(x, "x")
    B, T, HD, ld, sb = _bmk(x)
    assert HD == heads * 64

    def unpack(seg):
        if seg is None:
            return 0, 0, None, None
        start, (cos, sin) = seg
        _chk(cos, "cos", torch.float32); _chk(sin, "sin", torch.float32)
        assert cos.is_contiguous() and sin.is_contiguous() and cos.shape[-1] == 64
        return int(start), int(cos.shape[0]), cos, sin
    s0, l0, c0, n0 = unpack(seg0)
    s1, l1, c1, n1 = unpack(seg1)
    L.check(_launch("qk_layernorm_rope", L.load().tg_qk_layernorm_rope, _p(x), ld, sb, T, heads, B, _p(ln_weight), _p(ln_bias), float(eps), s0, l0, _p(c0),
                                          _p(n0), s1, l1, _p(c1), _p(n1), float(out_scale), _stream()), "tg_qk_layernorm_rope")
    return x


def kmax_workspace(tokens, heads, batch, device):
    """Scratch for qk_layernorm_rope_pair(kmax=...): fp32 [tg_qk_kmax_ws_floats]."""
    return torch.empty(L.load().tg_qk_kmax_ws_floats(tokens, heads, batch), dtype=torch.float32, device=device)


def qk_layernorm_rope_pair(xq, xk, heads, q_weight, q_bias, k_weight, k_bias, eps, seg0=None, seg1=None, q_scale=1.0, k_scale=1.0,
                           kmax=None, kmax_ws=None, out=None):
    """qk_layernorm_rope on the q and the k column slices of the same fused buffer in one launch (rotary tables read once).
    kmax (fp32 [B, heads], with kmax_ws from kmax_workspace): also receives max_t ||k_t||^2 of the stored K rows — the key-side range
    bound of the constant-shift attention (tg_qk_layernorm_rope_pair_kmax).  out = (yq, yk): OUT OF PLACE (tg_qk_layernorm_rope_pair_out) — xq / xk stay as they are."""
    _chk(xq, "xq"); _chk(xk, "xk")
    B, T, HD, ld, sb = _bmk(xq)
    assert HD == heads * 64 and _bmk(xk) == (B, T, HD, ld, sb)
    if out is not None:
        yq, yk = out
        _chk(yq, "yq"); _chk(yk, "yk")
        _, _, _, yld, ysb = _bmk(yq)
        assert _bmk(yk) == (B, T, HD, yld, ysb)

    def unpack(seg):
        if seg is None:
            return 0, 0, None, None
        start, (cos, sin) = seg
        _chk(cos, "cos", torch.float32); _chk(sin, "sin", torch.float32)
        assert cos.is_contiguous() and sin.is_contiguous() and cos.shape[-1] == 64
        return int(start), int(cos.shape[0]), cos, sin
    s0, l0, c0, n0 = unpack(seg0)
    s1, l1, c1, n1 = unpack(seg1)
    if kmax is not None:
        _chk(kmax, "kmax", torch.float32); _chk(kmax_ws, "kmax_ws", torch.float32)
        assert kmax.is_contiguous() and kmax.shape == (B, heads) and kmax_ws.numel() >= L.load().tg_qk_kmax_ws_floats(T, heads, B)
    if out is not None:
        L.check(_launch("qk_layernorm_rope_pair", L.load().tg_qk_layernorm_rope_pair_out, _p(xq), _p(xk), ld, sb, _p(yq), _p(yk), yld, ysb, T, heads, B, _p(q_weight),
                        _p(q_bias), _p(k_weight), _p(k_bias), float(eps), s0, l0, _p(c0), _p(n0), s1, l1, _p(c1), _p(n1), float(q_scale), float(k_scale),
                        _p(kmax), _p(kmax_ws) if kmax is not None else None, _stream()), "tg_qk_layernorm_rope_pair_out")
        return yq, yk
    if kmax is not None:
        L.check(_launch("qk_layernorm_rope_pair", L.load().tg_qk_layernorm_rope_pair_kmax, _p(xq), _p(xk), ld, sb, T, heads, B, _p(q_weight), _p(q_bias),
                        _p(k_weight), _p(k_bias), float(eps), s0, l0, _p(c0), _p(n0), s1, l1, _p(c1), _p(n1), float(q_scale), float(k_scale),
                        _p(kmax), _p(kmax_ws), _stream()), "tg_qk_layernorm_rope_pair_kmax")
        return xq, xk
    L.check(_launch("qk_layernorm_rope_pair", L.load().tg_qk_layernorm_rope_pair, _p(xq), _p(xk), ld, sb, T, heads, B, _p(q_weight), _p(q_bias),
                    _p(k_weight), _p(k_bias), float(eps), s0, l0, _p(c0), _p(n0), s1, l1, _p(c1), _p(n1), float(q_scale), float(k_scale),
                    _stream()), "tg_qk_layernorm_rope_pair")
    return xq, xk


def transpose_v(v, heads, key_start, n_keys, vt):
    """vt [B,heads,64,ldvt] <- v[:, key_start:key_start+n_keys] (v is a [B,T,heads*64] column slice)."""
    _chk(v, "v"); _chk(vt, "vt")
    B, T, HD, ld, sb = _bmk(v)
    assert vt.is_contiguous() and vt.shape[:3] == (B, heads, 64)
    L.check(_launch("transpose_v", L.load().tg_transpose_v, _p(v), ld, sb, key_start, n_keys, heads, B, _p(vt), vt.shape[3], _stream()), "tg_transpose_v")
    return vt


def attention(q1, k1, vt1, nk1, out, heads, scale, q2=None, k2=None, vt2=None, nk2=0, seg2_scale=0.0, k_prescaled=False):
    """out[B,nq,heads*64] = softmax(q1 k1^T) v1 + seg2_scale*softmax(q2 k2^T) v2 (segment 2 optional)."""
    _chk(q1, "q1"); _chk(k1, "k1"); _chk(vt1, "vt1"); _chk(out, "out")
    B, nq, _, qld, qsb = _bmk(q1)
    _, _, _, kld, ksb = _bmk(k1)
    _, _, _, old, osb = _bmk(out)
    a2 = (0, 0, 0, 0, 0, 0, 0, 0, 0)
    if q2 is not None:
        _chk(q2, "q2"); _chk(k2, "k2"); _chk(vt2, "vt2")
        _, _, _, q2ld, q2sb = _bmk(q2)
        _, _, _, k2ld, k2sb = _bmk(k2)
        a2 = (_p(q2), q2ld, q2sb, _p(k2), k2ld, k2sb, _p(vt2), vt2.stride(2), nk2)
    L.check(_launch("attention_2seg" if q2 is not None else f"attention_1seg_nq{nq}", L.load().tg_attention_fwd, _p(q1), qld, qsb, _p(k1), kld, ksb, _p(vt1), vt1.stride(2), nk1, *a2, float(seg2_scale),
                                      _p(out), old, osb, nq, heads, B, float(scale), 1 if k_prescaled else 0, _stream()), "tg_attention_fwd")
    return out


def attention_lse(q, k, vt, nk, out, heads, scale, k_prescaled=False, kmax=None, retry=None):
    """Training forward of one attention call: out = softmax(scale q k^T) v AND the per-row log-sum-exp (log2 domain, fp32 [B, heads, nq]) that
    attention_bwd takes instead of recomputing it (tg_attention_fwd_lse).  k_prescaled: k already carries scale * log2(e)
    (qk_layernorm_rope_pair k_scale) — attention_bwd then takes the same k with scale = ln 2; kmax (from qk_layernorm_rope_pair) + retry
    (AttnRetry): the verified constant-shift softmax of the inference path (tg_attention_fwd_lse_ex)."""
    _chk(q, "q"); _chk(k, "k"); _chk(vt, "vt"); _chk(out, "out")
    B, nq, _, qld, qsb = _bmk(q)
    _, _, _, kld, ksb = _bmk(k)
    _, _, _, old, osb = _bmk(out)
    lse = torch.empty(B, heads, nq, dtype=torch.float32, device=q.device)
    if k_prescaled or kmax is not None or retry is not None:
        if kmax is not None:
            _chk(kmax, "kmax", torch.float32)
            assert kmax.is_contiguous() and kmax.shape == (B, heads)
        assert retry is None or retry.fits(nq, 0, heads, B)
        L.check(_launch(f"attention_lse_nq{nq}", L.load().tg_attention_fwd_lse_ex, _p(q), qld, qsb, _p(k), kld, ksb, _p(vt), vt.stride(2), nk, _p(out), old, osb,
                        nq, heads, B, float(scale), 1 if k_prescaled else 0, _p(kmax), _p(retry.buf) if retry is not None else None,
                        retry.ints if retry is not None else 0, _p(lse), _stream()), "tg_attention_fwd_lse_ex")
        return out, lse
    L.check(_launch(f"attention_lse_nq{nq}", L.load().tg_attention_fwd_lse, _p(q), qld, qsb, _p(k), kld, ksb, _p(vt), vt.stride(2), nk, _p(out), old, osb, nq, heads, B,
                    float(scale), _p(lse), _stream()), "tg_attention_fwd_lse")
    return out, lse


class BwdDeviceState:
    """What the one-kernel attention backward needs per DEVICE, owned by the caller of the C ABI (nothing process-wide lives in the library):
    `status` = the int32[4] words tg_attention_bwd_ex reports through ([0] sticky count of exchange polls that timed out, [1] poll-limit override),
    `one_kernel` = verdict of the device probe (tg_attention_bwd_probe on a buffer of ours; one synchronisation, here, outside the ABI)."""

    _by_device = {}

    def __init__(self, device):
        lib = L.load()
        self.status = torch.zeros(4, dtype=torch.int32, device=device)
        self.one_kernel = False
        self.probe = None
        if os.environ.get("TG_ATTN_BWD_FUSED", "1") != "0":
            nb = lib.tg_attention_bwd_probe_bytes()
            buf = torch.empty(nb, dtype=torch.uint8, device=device)
            L.check(lib.tg_attention_bwd_probe(_p(buf), nb, _stream()), "tg_attention_bwd_probe")
            host = buf.cpu()                                   # (synchronises this stream, once per device and process)
            self.one_kernel = bool(lib.tg_attention_bwd_probe_verdict(host.data_ptr(), nb))
            # what the probe saw, for the record (bench.py's train sub-record): workgroups off their XCD / polls that gave up, and the chain's sums
            hi = host[:16].view(torch.int32)
            self.probe = {"flagged": int(hi[0]), "workgroups_not_on_xcd_b_mod_8": int(hi[2]),
                          "sums_exact": bool((host[4 * 2052:].view(torch.float32) == 528.0).all())}

    def flags(self):
        return L.TG_BWD_ONE_KERNEL if self.one_kernel else 0

    @classmethod
    def get(cls, device):
        device = torch.device(device)
        idx = device.index if device.index is not None else torch.cuda.current_device()
        st = cls._by_device.get(idx)
        if st is None:
            with torch.cuda.device(idx):
                st = cls._by_device[idx] = cls(torch.device("cuda", idx))
        return st


def attention_bwd_status(device=None, clear=True):
    """(timed-out exchange polls, workgroups off their head's XCD) summed over the devices this process has used since the last call — the sticky status
    words of the one-kernel backward (one synchronisation).  `clear` resets them, so that a discarded step can be attempted again."""
    devs = [torch.device(device).index] if device is not None else list(BwdDeviceState._by_device)
    polls = xcd = 0
    for idx in devs:
        st = BwdDeviceState._by_device.get(idx if idx is not None else torch.cuda.current_device())
        if st is None:
            continue
        n, _, x, _ = st.status.tolist()
        polls, xcd = polls + n, xcd + x
        if clear and (n or x):
            st.status[0].zero_(); st.status[2].zero_()
    return polls, xcd


def attention_bwd_error(polls, xcd, where="this process"):
    return RuntimeError(f"tg_attention_bwd_ex ({where}): {polls} ordered dQ exchange poll(s) timed out, {xcd} workgroup(s) found their head's key blocks on "
                        "more than one XCD — the gradients of this step are invalid; discard the step. TG_ATTN_BWD_FUSED=0 selects the two-launch form.")


def attention_bwd_check(device=None):
    """Read the sticky status word of the one-kernel backward on `device` (synchronises) and raise if any ordered-exchange poll timed out since the
    last check: the dq of that launch is invalid, the step must not be applied.  Single-process callers; the training step uses attention_bwd_status
    and makes the verdict collective before anything is applied (train.To2VTrainStep.micro_step)."""
    polls, xcd = attention_bwd_status(device)
    if polls or xcd:
        raise attention_bwd_error(polls, xcd, f"cuda:{torch.device(device).index}" if device is not None else "this process")


def _bwd_problem(q, k, v, o, dout, heads, scale, dq=None, dk=None, dv=None, accumulate=False, lse=None, dv_bf16=None):
    """One tg_attn_bwd_problem + the tensors that must outlive the launch call: (struct, (dq, dk, dv), keep).  dv_bf16 (bf16 [B, nk, heads*64] view, e.g. the V third of a fused
    projection gradient): receives bf16(dv) from the kernel's epilogue; the fp32 dv is then written only when `dv` is given too (else the tuple's dv is None)."""
    for n, t in (("q", q), ("k", k), ("v", v), ("o", o), ("dout", dout)):
        _chk(t, n)
    if lse is not None:
        _chk(lse, "lse", torch.float32)
        assert lse.is_contiguous() and lse.shape == (q.shape[0], heads, q.shape[1])
    B, nq, HD, qld, qsb = _bmk(q)
    _, nk, _, kld, ksb = _bmk(k)
    _, _, _, vld, vsb = _bmk(v)
    _, _, _, old, osb = _bmk(o)
    _, _, _, gld, gsb = _bmk(dout)
    assert HD == heads * 64 and o.shape == q.shape == dout.shape and v.shape == k.shape
    f32 = torch.float32
    acc = 3 if accumulate is True else int(accumulate)     # True: all three; 2: dk / dv only (dq overwritten); 0 / False: overwrite
    new = torch.zeros if acc else torch.empty              # accumulate adds to the buffer: a fresh one must start at zero
    dq = new(B, nq, HD, dtype=f32, device=q.device) if dq is None else _chk(dq, "dq", f32)
    dk = new(B, nk, HD, dtype=f32, device=q.device) if dk is None else _chk(dk, "dk", f32)
    if dv_bf16 is not None:
        _chk(dv_bf16, "dv_bf16")
        assert dv_bf16.shape == (B, nk, HD) and dv_bf16.stride(2) == 1 and (dv is not None or not (acc & 2)), "accumulate into dv needs the fp32 dv"
    if dv is not None or dv_bf16 is None:
        dv = new(B, nk, HD, dtype=f32, device=q.device) if dv is None else _chk(dv, "dv", f32)
    ws = torch.empty(L.load().tg_attention_bwd_ws_floats(nq, nk, heads, B), dtype=f32, device=q.device)
    pr = L.AttnBwdProblem()
    (pr.q, pr.q_ld, pr.q_sb, pr.k, pr.k_ld, pr.k_sb, pr.v, pr.v_ld, pr.v_sb, pr.o, pr.o_ld, pr.o_sb, pr.dout, pr.do_ld, pr.do_sb) = (
        _p(q), qld, qsb, _p(k), kld, ksb, _p(v), vld, vsb, _p(o), old, osb, _p(dout), gld, gsb)
    (pr.dq, pr.dq_ld, pr.dq_sb, pr.dk, pr.dk_ld, pr.dk_sb, pr.dv, pr.dv_ld, pr.dv_sb) = (
        _p(dq), dq.stride(1), dq.stride(0), _p(dk), dk.stride(1), dk.stride(0), _p(dv) if dv is not None else None, dv.stride(1) if dv is not None else 0,
        dv.stride(0) if dv is not None else 0)
    if dv_bf16 is not None:
        pr.dv_bf16, pr.dv_bf16_ld, pr.dv_bf16_sb = _p(dv_bf16), dv_bf16.stride(1), dv_bf16.stride(0)
    pr.nq, pr.nk, pr.scale, pr.accumulate, pr.lse, pr.ws = nq, nk, float(scale), acc, _p(lse), _p(ws)
    return pr, (dq, dk, dv), (ws, B)


def attention_bwd_multi(problems, heads):
    """One or two attention backward problems in ONE call (tg_attention_bwd_multi): the same as attention_bwd on each in order, except that two problems that both
    take the one-kernel form share a launch (the second rides in the first's last round of CUs).  problems: dicts of attention_bwd's arguments (without `heads`).
    Returns the list of (dq, dk, dv)."""
    assert 1 <= len(problems) <= 2
    built = [_bwd_problem(heads=heads, **pr) for pr in problems]
    arr = (L.AttnBwdProblem * len(built))(*[b[0] for b in built])
    B = built[0][2][1]
    dev = problems[0]["q"].device
    st = BwdDeviceState.get(dev)
    L.check(_launch("attention_bwd", L.load().tg_attention_bwd_multi, arr, len(built), heads, B, st.flags(), _p(st.status), _stream()), "tg_attention_bwd_multi")
    return [b[1] for b in built]


def attention_bwd(q, k, v, o, dout, heads, scale, dq=None, dk=None, dv=None, accumulate=False, lse=None, dv_bf16=None):
    """Gradients of o = softmax(scale q k^T) v per head (tg_attention_bwd_multi with one problem).  q/o/dout [B,nq,heads*64], k/v [B,nk,heads*64] bf16 views;
    returns fp32 (dq, dk, dv) shaped like q, k, v (given tensors are written, or added to with accumulate=True).  lse: the forward's
    log-sum-exp from attention_lse (optional; recomputed when None).  The one-kernel form is offered to the library when the device probe
    passed (BwdDeviceState); a poll time-out inside it is reported by attention_bwd_status() / attention_bwd_check(), never silently."""
    return attention_bwd_multi([dict(q=q, k=k, v=v, o=o, dout=dout, scale=scale, dq=dq, dk=dk, dv=dv, accumulate=accumulate, lse=lse, dv_bf16=dv_bf16)], heads)[0]


def _attn_problem(q1, k1, vt1, nk1, out, q2=None, k2=None, vt2=None, nk2=0, seg2_scale=0.0, kmax1=None, kmax2=None, seg2_scale_batch=None):
    for n, t in (("q1", q1), ("k1", k1), ("vt1", vt1), ("out", out)):
        _chk(t, n)
    pr = L.AttnProblem()
    B, nq, _, qld, qsb = _bmk(q1)
    _, _, _, kld, ksb = _bmk(k1)
    _, _, _, old, osb = _bmk(out)
    for km in (kmax1, kmax2):
        if km is not None:
            _chk(km, "kmax", torch.float32)
            assert km.is_contiguous() and km.shape[0] == B
    pr.seg[0] = L.AttnSegment(_p(q1), qld, qsb, _p(k1), kld, ksb, _p(vt1), vt1.stride(2), nk1, _p(kmax1) or None)
    pr.nseg = 1
    if q2 is not None:
        _chk(q2, "q2"); _chk(k2, "k2"); _chk(vt2, "vt2")
        _, _, _, q2ld, q2sb = _bmk(q2)
        _, _, _, k2ld, k2sb = _bmk(k2)
        pr.seg[1] = L.AttnSegment(_p(q2), q2ld, q2sb, _p(k2), k2ld, k2sb, _p(vt2), vt2.stride(2), nk2, _p(kmax2) or None)
        pr.nseg = 2
    pr.seg2_scale = float(seg2_scale)
    pr.out, pr.out_ld, pr.out_strideB, pr.nq = _p(out), old, osb, nq
    if seg2_scale_batch is not None:            # host list of per-batch-item weights; the ctypes array must outlive the call: kept on the struct
        assert len(seg2_scale_batch) == B
        pr._scales = (C.c_float * B)(*[float(v) for v in seg2_scale_batch])
        pr.seg2_scale_batch = C.cast(pr._scales, C.POINTER(C.c_float))
    return pr, B


class AttnRetry:
    """Retry workspace of the constant-shift attention path (tg_attention_fwd_multi retry_ws): one int32 buffer per model, sized for its
    largest launch, zeroed once.  `count()` = workgroups recomputed with the running maximum so far (a device read: diagnostics / tests);
    `poll()` is the non-blocking form the model uses to notice weights for which the shift estimate keeps failing."""

    def __init__(self, nq0, nq1, heads, batch, device):
        self.ints = int(L.load().tg_attention_retry_ints(nq0, nq1, heads, batch))
        self.buf = torch.zeros(self.ints, dtype=torch.int32, device=device)
        self._host = torch.zeros(1, dtype=torch.int32).pin_memory()
        self._event = None
        # the fast-path launches issued against THIS buffer and (launches, retries) at the last landed poll: the counter lives in this buffer, so
        # the bookkeeping that interprets it does too (a model owns one AttnRetry per workspace shape; mixing their deltas would be meaningless)
        self.launches, self.mark = 0, (0, 0)
        # the key-split scratch of the same launch shape (tg_attn_workspace.split; 0 floats when the shape leaves no half-round tail)
        nsf = int(L.load().tg_attention_split_floats(nq0, nq1, heads, batch))
        self.split = torch.empty(nsf, dtype=torch.float32, device=device) if nsf else None

    def fits(self, nq0, nq1, heads, batch):
        return L.load().tg_attention_retry_ints(nq0, nq1, heads, batch) <= self.ints

    def count(self):
        return int(self.buf[0].item())

    def poll(self, tag):
        """Non-blocking read of the counter: returns (value, tag given when that copy was queued) once a queued copy has landed, else
        None; queues the next copy on the current stream when none is pending."""
        val = None
        if self._event is not None and self._event.query():
            val = (int(self._host[0]), self._tag)
            self._event = None
        if self._event is None:
            self._host.copy_(self.buf[:1], non_blocking=True)
            self._event = torch.cuda.Event()
            self._event.record()
            self._tag = tag
        return val


def attention_multi(main, rider, heads, scale, k_prescaled=False, retry=None, split=None):
    """One launch for one or two attention problems of the same heads/batch (tg_attention_fwd_multi).  main / rider: dicts of the
    keyword arguments of `attention` (q1, k1, vt1, nk1, out [, q2, k2, vt2, nk2, seg2_scale, kmax1, kmax2]); the rider (may be None) has one
    key segment.  kmax1 / kmax2 (fp32 [B, heads], from qk_layernorm_rope_pair(kmax=...)) on every segment + retry (AttnRetry): the
    constant-shift softmax path (tg_attn_segment.k_norm2_max).  split (fp32 scratch tensor, e.g. AttnRetry.split): lets the launch split its
    half-round tail over the key axis (tg_attn_workspace.split)."""
    import ctypes
    pa, B = _attn_problem(**main)
    n = 1
    if rider is not None:
        pb, B2 = _attn_problem(**rider)
        assert B == B2
        arr = (L.AttnProblem * 2)(pa, pb)
        n = 2
    else:
        arr = (L.AttnProblem * 1)(pa)
    if retry is not None:
        assert retry.fits(main["q1"].shape[1], rider["q1"].shape[1] if rider is not None else 0, heads, B)
    ws = L.AttnWorkspace(_p(retry.buf) if retry is not None else None, retry.ints if retry is not None else 0,
                         _p(split) if split is not None else None, split.numel() if split is not None else 0)
    L.check(_launch("attention_2seg+rider" if n == 2 else f"attention_multi1_nq{pa.nq}", L.load().tg_attention_fwd_multi, ctypes.addressof(arr), n, heads, B,
                    float(scale), 1 if k_prescaled else 0, ctypes.addressof(ws), _stream()), "tg_attention_fwd_multi")
    return main["out"], (rider["out"] if rider is not None else None)


_LORA_WS = {}


def lora_wgrad(y, t, out, scale=1.0, beta=0.0, transposed=False):
    """out = beta * out + scale * y^T t, summed over the token axis (tg_lora_wgrad).  y [M, N] or [B, M, N], t likewise [.., R]: bf16, row / batch strides
    allowed (column slices of wider buffers).  out fp32: [N, R], or [R, N] with transposed=True; any strides (a view of a gradient arena).  The partial-sum
    workspace is kept per (rows, N, R, device): every use is ordered on the launch stream."""
    _chk(y, "y"); _chk(t, "t")
    B, M, N, ldy, sy = _bmk(y)
    Bt, Mt, R, ldt, st = _bmk(t)
    if (B, M) != (Bt, Mt):
        raise ValueError(f"lora_wgrad: y{tuple(y.shape)} and t{tuple(t.shape)} differ in their token axes")
    if not out.is_cuda or out.dtype != torch.float32 or tuple(out.shape) != ((R, N) if transposed else (N, R)):
        raise ValueError(f"lora_wgrad: out must be an fp32 GPU tensor of shape {(R, N) if transposed else (N, R)}, got {out.dtype} {tuple(out.shape)}")
    gsn, gsj = (out.stride(1), out.stride(0)) if transposed else (out.stride(0), out.stride(1))
    lib = L.load()
    key = (B * M, N, R, str(y.device))
    if key not in _LORA_WS:
        _LORA_WS[key] = torch.empty(max(1, lib.tg_lora_wgrad_ws_floats(B * M, N, R)), dtype=torch.float32, device=y.device)
    L.check(_launch(f"lora_wgrad_M{B * M}_N{N}_R{R}", lib.tg_lora_wgrad, _p(y), ldy, sy, _p(t), ldt, st, M, B, N, R, _p(out), gsn, gsj, float(beta), float(scale),
                    _p(_LORA_WS[key]), _stream()), "tg_lora_wgrad")
    return out


def lora_merge(w, b, a, scale, out=None):
    """out = bf16(w + scale * b @ a), summed in fp64 and rounded once (tg_lora_merge).  w [N, K], b [N, R], a [R, K] bf16 (row strides allowed);
    out defaults to w (in place)."""
    out = w if out is None else out
    for n_, t_ in (("w", w), ("b", b), ("a", a), ("out", out)):
        _chk(t_, n_)
    N, K_ = w.shape
    R = a.shape[0]
    if b.shape != (N, R) or a.shape != (R, K_) or out.shape != w.shape:
        raise ValueError(f"lora_merge: shape mismatch w{tuple(w.shape)} b{tuple(b.shape)} a{tuple(a.shape)} out{tuple(out.shape)}")
    L.check(L.load().tg_lora_merge(_p(w), w.stride(0), _p(b), b.stride(0), _p(a), a.stride(0), _p(out), out.stride(0), N, K_, R, float(scale), _stream()),
            "tg_lora_merge")
    return out


def timestep_sinusoid(t, dim, out):
    _chk(t, "t", torch.int64); _chk(out, "out")
    L.check(L.load().tg_timestep_sinusoid(_p(t), t.numel(), dim, _p(out), _stream()), "tg_timestep_sinusoid")
    return out


def patchify(lat, out, p=2):
    """lat [BF,C,H,W] contiguous -> out [BF*(H/p)*(W/p), ld >= p*p*C] (pad columns are left untouched)"""
    _chk(lat, "lat"); _chk(out, "out")
    assert lat.is_contiguous() and out.stride(1) == 1
    BF, Cc, H, W = lat.shape
    L.check(L.load().tg_patchify(_p(lat), _p(out), out.stride(0), BF, Cc, H, W, p, _stream()), "tg_patchify")
    return out


def unpatchify(x, lat, p=2):
    """x [BF*(H/p)*(W/p), ld >= p*p*C] rows -> lat [BF,C,H,W] contiguous"""
    _chk(x, "x"); _chk(lat, "lat")
    assert lat.is_contiguous()
    BF, Cc, H, W = lat.shape
    L.check(L.load().tg_unpatchify(_p(x), x.stride(0), _p(lat), BF, Cc, H, W, p, _stream()), "tg_unpatchify")
    return lat


def cfg_dpm_step(model_out, x, old_x0, noise, coef, guidance, x_out, x0_out):
    """model_out [2,F,E]; x/old_x0/x_out/x0_out [F,E]; noise [F,2,E]; coef fp32 [F,8] (device)."""
    for n, t in (("model_out", model_out), ("x", x), ("old_x0", old_x0), ("noise", noise), ("x_out", x_out), ("x0_out", x0_out)):
        _chk(t, n)
        assert t.is_contiguous()
    _chk(coef, "coef", torch.float32)
    F_, E = x.shape[0], x[0].numel()
    L.check(L.load().tg_cfg_dpm_step(_p(model_out), _p(x), _p(old_x0), _p(noise), _p(coef), float(guidance), _p(x_out),
                                     _p(x0_out), F_, E, _stream()), "tg_cfg_dpm_step")
    return x_out, x0_out


def cfg_dpm_step_f32(model_out, x, old_x0, noise, coef, guidance, x_out, x0_out):
    """Pipeline-loop variant: model_out [2,F,E] / x / x_out / noise [F,2,E] bf16; old_x0, x0_out [F,E] fp32."""
    for n, t in (("model_out", model_out), ("x", x), ("x_out", x_out), ("noise", noise)):
        _chk(t, n)
        assert t.is_contiguous()
    for n, t in (("old_x0", old_x0), ("x0_out", x0_out), ("coef", coef)):
        _chk(t, n, torch.float32)
        assert t.is_contiguous()
    F_, E = x.shape[0], x[0].numel()
    L.check(L.load().tg_cfg_dpm_step_f32(_p(model_out), _p(x), _p(old_x0), _p(noise), _p(coef), float(guidance), _p(x_out),
                                         _p(x0_out), F_, E, _stream()), "tg_cfg_dpm_step_f32")
    return x_out, x0_out


PRED_TYPES = {"v_prediction": 0, "epsilon": 1, "sample": 2}


def cfg_dpm_step_ex(model_out, x, old_x0, noise, coef, guidance, x_out, x0_out, guidance_img=0.0, guidance_per_frame=None, f32_math=False,
                    prediction_type="v_prediction"):
    """tg_cfg_dpm_step_ex: model_out [1 (no guidance), 2 or 3, F, E] bf16; x / x_out / noise [F,2,E] bf16; old_x0 / x0_out [F,E] bf16 or fp32 (fp32: the pipelines'
    solver state, implies f32_math); guidance_per_frame: fp32 [F, 2] device tensor {g, g_img} (the worker's dynamic cfg) or None."""
    for n, t in (("model_out", model_out), ("x", x), ("x_out", x_out), ("noise", noise)):
        _chk(t, n)
        assert t.is_contiguous()
    f32_state = old_x0.dtype == torch.float32
    for n, t in (("old_x0", old_x0), ("x0_out", x0_out)):
        _chk(t, n, torch.float32 if f32_state else BF16)
        assert t.is_contiguous()
    _chk(coef, "coef", torch.float32)
    F_, E = x.shape[0], x[0].numel()
    br = model_out.shape[0]
    assert br in (1, 2, 3) and model_out.numel() == br * F_ * E and coef.shape == (F_, 8) and coef.is_contiguous()
    if guidance_per_frame is not None:
        _chk(guidance_per_frame, "guidance_per_frame", torch.float32)
        assert guidance_per_frame.is_contiguous() and guidance_per_frame.shape == (F_, 2)
    L.check(L.load().tg_cfg_dpm_step_ex(_p(model_out), br, _p(x), _p(old_x0), _p(noise), _p(coef), float(guidance), float(guidance_img),
                                        _p(guidance_per_frame) or None, 1 if (f32_math or f32_state) else 0, 1 if f32_state else 0,
                                        PRED_TYPES[prediction_type], _p(x_out), _p(x0_out), F_, E, _stream()), "tg_cfg_dpm_step_ex")
    return x_out, x0_out


def pca_inverse(lat, std, mean, comp, pmean, out):
    """lat bf16 [F,16,h,w]; std/mean fp32 [16]; comp fp32 [16,C]; pmean fp32 [C] -> out bf16 [F,C,h,w]."""
    _chk(lat, "lat"); _chk(out, "out")
    for n, t in (("std", std), ("mean", mean), ("comp", comp), ("pmean", pmean)):
        _chk(t, n, torch.float32)
        assert t.is_contiguous()
    assert lat.is_contiguous() and out.is_contiguous()
    F_, nc, h, w = lat.shape
    Cc = out.shape[1]
    assert comp.shape == (nc, Cc) and pmean.numel() == Cc and std.numel() == nc and mean.numel() == nc and out.shape == (F_, Cc, h, w)
    L.check(L.load().tg_pca_inverse(_p(lat), _p(std), _p(mean), _p(comp), _p(pmean), _p(out), F_, nc, h * w, Cc, _stream()), "tg_pca_inverse")
    return out


def pca_lowrank_filter(x, comp, mean, out=None):
    """x bf16 [rows, D] (rows may be strided) -> bf16 [rows, D]: project onto the first comp.shape[0] (<= 16) PCA components and back, fp32."""
    _chk(x, "x"); _chk(comp, "comp", torch.float32); _chk(mean, "mean", torch.float32)
    assert x.dim() == 2 and comp.is_contiguous() and mean.is_contiguous() and comp.shape[1] == x.shape[1] and mean.numel() == x.shape[1]
    out = torch.empty_like(x) if out is None else _chk(out, "out")
    L.check(_launch("pca_lowrank_filter", L.load().tg_pca_lowrank_filter, _p(x), x.stride(0), _p(comp), _p(mean), _p(out), out.stride(0), x.shape[0],
                    x.shape[1], comp.shape[0], _stream()), "tg_pca_lowrank_filter")
    return out


# ---------------------------------------------------------------------------------------------------------
# VAE (channels-last bf16 activations)
# ---------------------------------------------------------------------------------------------------------
_ZEROS = {}


def zero_page(device):
    z = _ZEROS.get(device)
    if z is None:
        z = _ZEROS[device] = torch.zeros(8192, dtype=BF16, device=device)
    return z


_SPLITK = {}


def _splitk_floats(*key):
    n = _SPLITK.get(key)
    if n is None:
        n = _SPLITK[key] = int(L.load().tg_conv3d_splitk_floats(*key))
    return n


def conv3d_cl(x, w_packed, bias, cout, kt, kh, kw, cache=None, stride=1, pad=1, up=1, t_map=None, residual=None, out_dims=None,
              gn_stats_eps=None):
    """x [T,H,W,Cin] channels-last; w_packed [Cout_pad, kt*kh*kw, Cin]; returns y [To,Ho,Wo,cout].
    gn_stats_eps: also produce the GroupNorm(32) sums of y in the epilogue (cout % 128 == 0): attached as y.gn_sums (GnSums) for the norm that
    consumes y, which finalises them itself — no statistics launch; y.gn_sums.stats() gives the [32, 2] (mean, rstd) tensor on request."""
    _chk(x, "x"); _chk(w_packed, "w")
    assert x.is_contiguous() and w_packed.is_contiguous()
    T, H, W, Cin = x.shape
    To, Ho, Wo = out_dims if out_dims is not None else (T, H, W)
    y = torch.empty(To, Ho, Wo, cout, dtype=BF16, device=x.device)
    if cache is not None:
        _chk(cache, "cache"); assert cache.is_contiguous() and cache.shape == (kt - 1, H, W, Cin)
    if residual is not None:
        _chk(residual, "residual"); assert residual.is_contiguous() and residual.shape == y.shape
    if t_map is not None:
        _chk(t_map, "t_map", torch.int32)
    fuse = gn_stats_eps is not None and cout % 128 == 0 and w_packed.shape[0] == cout and 128 % (cout // 32) == 0      # whole groups per 128-channel tile (conv_plan.h)
    partial = torch.empty(L.load().tg_conv3d_gn_partial_floats(To, Ho, Wo), dtype=torch.float32, device=x.device) if fuse else None
    nws = _splitk_floats(Cin, cout, w_packed.shape[0], kt, kh, kw, To, Ho, Wo)
    ws = torch.empty(nws, dtype=torch.float32, device=x.device) if nws else None
    L.check(_launch(f"conv3d_cl_Cin{Cin}_Cout{cout}_k{kt}{kh}{kw}_s{stride}_u{up}", L.load().tg_conv3d_cl, _p(x), T, H, W, Cin, _p(cache),
                    _p(w_packed), _p(bias), cout, w_packed.shape[0], kt, kh, kw, stride, pad, up, _p(t_map), _p(residual), _p(y), cout, To, Ho,
                    Wo, _p(zero_page(x.device)), _p(partial), _p(ws), _stream()), "tg_conv3d_cl")
    if fuse:
        y.gn_sums = GnSums(partial, To * Ho * Wo, cout, float(gn_stats_eps))
    return y


def conv3d_up2_subpixel_ok(T, H, W, Cin, cout):
    """Does tg_conv3d_up2_subpixel take this shape (the 256 x 256 convolution kernel's range)?"""
    return bool(L.load().tg_conv3d_up2_subpixel_ok(T, H, W, Cin, cout))


def conv3d_up2_subpixel(x, w_phases, bias, cout, gn_stats_eps=None, time_x2=False):
    """Nearest x2 spatial upsampling + Conv2d 3x3 (pad 1) as four 2x2 phase convolutions on the low-resolution input (tg_conv3d_up2_subpixel; the deviation — pre-summed
    bf16 weights — is stated in the header).  x [T, H, W, Cin] channels-last; w_phases [4, cout, 4, Cin] (vae.pack_up2_phases); returns y [To, 2H, 2W, cout], with
    y.gn_sums as conv3d_cl leaves them.  time_x2: the layer's nearest x2 in TIME as well (each frame convolved once, stored twice; To = 2T, or 2T - 1 for odd T > 1)."""
    _chk(x, "x"); _chk(w_phases, "w_phases")
    assert x.is_contiguous() and w_phases.is_contiguous()
    T, H, W, Cin = x.shape
    assert tuple(w_phases.shape) == (4, cout, 4, Cin)
    To = T if not (time_x2 and T > 1) else (2 * T - 1 if T % 2 else 2 * T)        # time_x2: every frame twice, except the first of an odd count (CogVideoXUpsample3D)
    y = torch.empty(To, 2 * H, 2 * W, cout, dtype=BF16, device=x.device)
    fuse = gn_stats_eps is not None and cout % 256 == 0 and 256 % (cout // 32) == 0     # whole groups per 256-channel tile
    partial = torch.empty(L.load().tg_conv3d_up2_subpixel_gn_floats(T, H, W), dtype=torch.float32, device=x.device) if fuse else None
    L.check(_launch(f"conv3d_up2_subpixel_Cin{Cin}_Cout{cout}_t{int(bool(time_x2))}", L.load().tg_conv3d_up2_subpixel, _p(x), T, H, W, Cin, _p(w_phases), _p(bias), cout, _p(y), cout,
                    1 if time_x2 else 0, _p(zero_page(x.device)), _p(partial), _stream()), "tg_conv3d_up2_subpixel")
    if fuse:
        y.gn_sums = GnSums(partial, To * 4 * H * W, cout, float(gn_stats_eps))
    return y


class GnSums:
    """The GroupNorm(32) sums a convolution's epilogue left for the norm that reads its output: rows of [2][32] (sum, sum of squares per group), one per
    128 voxels.  The norm pass turns <= 64 rows into (mean, rstd) in its own prologue (tg_groupnorm_silu_ex / tg_spatialnorm_silu_ex); longer lists are
    cut to <= 64 fp64 rows by one tg_groupnorm_reduce launch first.  `.stats()` gives the classic [32, 2] (mean, rstd) tensor through
    tg_groupnorm_finalize (tests / callers that want the numbers)."""

    def __init__(self, partial, V, C, eps):
        self.partial, self.V, self.C, self.eps = partial, V, C, eps
        self._rows = None

    def rows(self):
        """(tensor, row count, is_f64) as the *_ex norm entry points take them."""
        if self._rows is None:
            n = self.partial.numel() // 64
            r = L.load().tg_groupnorm_reduce_rows(n)
            if r == 0:
                self._rows = (self.partial, n, 0)
            else:
                out = torch.empty(r, 64, dtype=torch.float64, device=self.partial.device)
                L.check(_launch("groupnorm_reduce", L.load().tg_groupnorm_reduce, _p(self.partial), n, _p(out), _stream()), "tg_groupnorm_reduce")
                self._rows = (out, r, 1)
        return self._rows

    def stats(self):
        if self.partial.numel() // 64 != (self.V + 127) // 128:
            # tg_groupnorm_finalize walks ceil(V / 128) rows: the phase launches of conv3d_up2_subpixel leave 4 x ceil(V / 4 / 128) — the norm passes take any row count (rows())
            raise ValueError("GnSums.stats(): this buffer has one row list per phase launch; use rows() (what the norm passes read)")
        stats = torch.empty(32, 2, dtype=torch.float32, device=self.partial.device)
        L.check(_launch("groupnorm_finalize", L.load().tg_groupnorm_finalize, _p(self.partial), self.V, self.C, self.eps, _p(stats), _stream()),
                "tg_groupnorm_finalize")
        return stats


def groupnorm_stats(x2d, eps=1e-6):
    """x2d [V, C] -> stats fp32 [32, 2] (mean, rstd)."""
    _chk(x2d, "x"); assert x2d.is_contiguous()
    V, C = x2d.shape
    n = L.load().tg_groupnorm_partial_floats(V, C)
    partial = torch.empty(n, dtype=torch.float32, device=x2d.device)
    stats = torch.empty(32, 2, dtype=torch.float32, device=x2d.device)
    L.check(_launch("groupnorm_stats", L.load().tg_groupnorm_stats, _p(x2d), V, C, float(eps), _p(partial), _p(stats), _stream()), "tg_groupnorm_stats")
    return stats


def _stats_args(stats):
    """stats: a [32, 2] (mean, rstd) tensor, or a GnSums -> (stats ptr, sums ptr, rows, is_f64, eps) of the *_ex norm entry points."""
    if isinstance(stats, GnSums):
        t, n, f64 = stats.rows()
        return None, _p(t), n, f64, stats.eps
    return _p(stats), None, 0, 0, 0.0


def groupnorm_silu(x, stats, gamma, beta, silu=True):
    """stats: [32, 2] (mean, rstd) from groupnorm_stats, or the GnSums a convolution attached to x (no statistics launch)."""
    _chk(x, "x"); assert x.is_contiguous()
    C = x.shape[-1]
    y = torch.empty_like(x)
    L.check(_launch("groupnorm_silu", L.load().tg_groupnorm_silu_ex, _p(x), x.numel() // C, C, *_stats_args(stats), _p(gamma), _p(beta), _p(y),
                    1 if silu else 0, _stream()), "tg_groupnorm_silu")
    return y


def spatialnorm_silu(f, stats, gamma, beta, yz, bz, zdims, silu=True):
    """f [T,H,W,C]; yz/bz [Tz*Hz*Wz, >=C] = conv_y(z)/conv_b(z) per latent voxel (row stride may exceed C); zdims=(Tz,Hz,Wz)."""
    _chk(f, "f"); _chk(yz, "yz"); _chk(bz, "bz"); assert f.is_contiguous()
    T, H, W, C = f.shape
    Tz, Hz, Wz = zdims
    assert yz.shape[0] == Tz * Hz * Wz and yz.stride(0) == bz.stride(0)
    y = torch.empty_like(f)
    L.check(_launch("spatialnorm_silu", L.load().tg_spatialnorm_silu_ex, _p(f), T, H, W, C, *_stats_args(stats), _p(gamma), _p(beta), _p(yz), _p(bz),
                    yz.stride(0), Tz, Hz, Wz, _p(y), 1 if silu else 0, _stream()), "tg_spatialnorm_silu")
    return y


def avgpool_time(x):
    _chk(x, "x"); assert x.is_contiguous()
    T, H, W, C = x.shape
    To = 1 + (T - 1) // 2 if T % 2 else T // 2
    y = torch.empty(To, H, W, C, dtype=BF16, device=x.device)
    L.check(_launch("avgpool_time", L.load().tg_avgpool_time, _p(x), T, H * W, C, _p(y), _stream()), "tg_avgpool_time")
    return y


def ncdhw_to_cl(src, t0, Tc, h0, Hc, w0, Wc, Cpad, scale=1.0):
    """src [C,T,H,W] (fp32 or bf16, contiguous) window -> [Tc,Hc,Wc,Cpad] bf16."""
    if not src.is_cuda:
        raise RuntimeError("ncdhw_to_cl: expected a GPU tensor (tokensgen_amd has no CPU fallback)")
    assert src.is_contiguous() and src.dtype in (torch.float32, BF16)
    C, Tt, Ht, Wt = src.shape
    dst = torch.empty(Tc, Hc, Wc, Cpad, dtype=BF16, device=src.device)
    L.check(L.load().tg_ncdhw_to_cl(_p(src), 1 if src.dtype == torch.float32 else 0, C, Tt, Ht, Wt, t0, Tc, h0, Hc, w0, Wc, float(scale), _p(dst),
                                    Cpad, _stream()), "tg_ncdhw_to_cl")
    return dst


def cl_to_ncdhw(src, dst, t0=0, h0=0, w0=0):
    """src [T,H,W,C] channels-last bf16 -> window of dst [C,Tt,Ht,Wt] (fp32 or bf16)."""
    _chk(src, "src"); assert src.is_contiguous() and dst.is_contiguous() and dst.is_cuda
    T, H, W, C = src.shape
    Cd, Tt, Ht, Wt = dst.shape
    assert Cd == C
    L.check(L.load().tg_cl_to_ncdhw(_p(src), C, C, T, H, W, _p(dst), 1 if dst.dtype == torch.float32 else 0, Tt, Ht, Wt, t0, h0, w0, _stream()),
            "tg_cl_to_ncdhw")
    return dst


def tile_blend(a, b, axis, extent):
    """In place on b: NCDHW [C,T,H,W] tiles (same dtype, fp32 or bf16); axis 3 = height (blend_v), 4 = width (blend_h)."""
    assert a.is_cuda and b.is_cuda and a.dtype == b.dtype and a.is_contiguous() and b.is_contiguous()
    C, T, Ha, Wa = a.shape
    _, _, Hb, Wb = b.shape
    extent = min(a.shape[axis - 1], b.shape[axis - 1], extent)
    if extent <= 0:
        return b
    L.check(L.load().tg_tile_blend(_p(a), _p(b), 1 if a.dtype == torch.float32 else 0, C, T, Ha, Wa, Hb, Wb, axis, extent, _stream()), "tg_tile_blend")
    return b


def _chk_vec(t, name, dtype, shape):
    """this dtype, exactly this shape, contiguous, on the GPU"""
    _chk(t, name, dtype)
    if tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{name}: expected contiguous {list(shape)}, got {tuple(t.shape)}")


def _chk_rgb(t, name, contiguous=False):
    """uint8 RGB frames on the GPU, [F, H, W, 3] or [B, T, H, W, 3], any view; with `contiguous` only a contiguous [F, H, W, 3] with at least one pixel and frames
    below 2^31 pixels.  -> (n_outer, n_inner, H, W) and the byte strides (outer, inner, row, pixel, channel)"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name}: expected a GPU tensor (tokensgen_amd has no CPU fallback)")
    want = "contiguous uint8 [F, H, W, 3] with at least one pixel" if contiguous else "uint8 [F, H, W, 3] or [B, T, H, W, 3] with non-negative strides"
    if t.dtype != torch.uint8 or t.dim() not in ((4,) if contiguous else (4, 5)) or t.shape[-1] != 3 or min(t.stride()) < 0 or \
            (contiguous and (not t.is_contiguous() or t.numel() < 1)):
        raise ValueError(f"{name}: expected {want}, got {t.dtype} {tuple(t.shape)}")
    if contiguous and t.shape[1] * t.shape[2] >= 1 << 31:
        raise ValueError(f"{name}: a frame of {t.shape[1]} x {t.shape[2]} pixels reaches 2^31")
    s = t.stride()
    if t.dim() == 4:
        return (1, t.shape[0], t.shape[1], t.shape[2]), (0, s[0], s[1], s[2], s[3])
    return (t.shape[0], t.shape[1], t.shape[2], t.shape[3]), (s[0], s[1], s[2], s[3], s[4])


def video_resample(frames_u8, tables, oh, ow):
    """tg_video_resample: uint8 [F, H, W, 3] contiguous -> bf16 [F, 3, oh, ow] in [-1, 1].  tables = (y0, ny, wy, x0, nx, wx) on the same device: int32 [oh], int32
    [oh], fp32 [oh, taps_y] and the same per output column (tokensgen_amd.video_io.resample_plan builds them)."""
    _chk(frames_u8, "frames", torch.uint8)
    (_, F, H, W), _ = _chk_rgb(frames_u8, "frames", contiguous=True)
    y0, ny, wy, x0, nx, wx = tables
    for t, name, dt, n in ((y0, "y0", torch.int32, oh), (ny, "ny", torch.int32, oh), (wy, "wy", torch.float32, oh), (x0, "x0", torch.int32, ow),
                           (nx, "nx", torch.int32, ow), (wx, "wx", torch.float32, ow)):
        _chk(t, name, dt)
        if t.device != frames_u8.device or not t.is_contiguous() or t.shape[0] != n or t.dim() != (2 if dt == torch.float32 else 1):
            raise ValueError(f"{name}: expected a contiguous table of {n} rows on {frames_u8.device}, got {tuple(t.shape)} on {t.device}")
    out = torch.empty(F, 3, oh, ow, dtype=BF16, device=frames_u8.device)
    L.check(_launch("video_resample", L.load().tg_video_resample, _p(frames_u8), F, H, W, _p(out), oh, ow, _p(y0), _p(ny), _p(wy), wy.shape[1], _p(x0), _p(nx),
                    _p(wx), wx.shape[1], _stream()), "tg_video_resample")
    return out


VIDEO_U8, VIDEO_F32, VIDEO_BF16_PLANAR = 0, 1, 2


def video_to_uint8(video, channel_dim, kind=VIDEO_U8, rounding=0):
    """tg_video_to_uint8: bf16 [B, 3, T, H, W] (channel_dim 1) or [B, T, 3, H, W] (channel_dim 2), any batch / channel / frame strides over contiguous H x W planes ->
    uint8 [B, T, H, W, 3] (kind VIDEO_U8; rounding 0 truncates, 1 rounds half to even), fp32 [B, T, H, W, 3] in [0, 1] (VIDEO_F32) or bf16 [B, T, 3, H, W] in [0, 1]
    (VIDEO_BF16_PLANAR)."""
    _chk(video, "video")
    if video.dim() != 5 or channel_dim not in (1, 2) or video.shape[channel_dim] != 3:
        raise ValueError(f"video: expected [B, 3, T, H, W] or [B, T, 3, H, W] with the channel axis named, got {tuple(video.shape)} / channel_dim={channel_dim}")
    B, H, W = video.shape[0], video.shape[3], video.shape[4]
    t_dim = 3 - channel_dim
    T = video.shape[t_dim]
    if H * W > 1 and (video.stride(4) != 1 or (H > 1 and video.stride(3) != W)):
        raise ValueError("video: the H x W planes must be contiguous")
    shape, dt = {VIDEO_U8: ((B, T, H, W, 3), torch.uint8), VIDEO_F32: ((B, T, H, W, 3), torch.float32), VIDEO_BF16_PLANAR: ((B, T, 3, H, W), BF16)}[kind]
    out = torch.empty(shape, dtype=dt, device=video.device)
    L.check(_launch("video_to_uint8", L.load().tg_video_to_uint8, _p(video), video.stride(0), video.stride(channel_dim), video.stride(t_dim), B, T, H, W, _p(out),
                    kind, int(rounding), _stream()), "tg_video_to_uint8")
    return out


IMAGE_LAYOUTS = ("hwc", "chw", "bcthw", "bfchw")
_IMAGE_DTYPES = {torch.uint8: 0, torch.float32: 1, BF16: 2}
IMAGE_WINDOW = 11


def _image_strides(t, layout):
    """(n_outer, n_inner, C, H, W) and the element strides (outer, inner, channel, row, pixel) of an image batch in one of IMAGE_LAYOUTS"""
    s = t.stride()
    if layout == "hwc" and t.dim() == 4:            # [F, H, W, C]
        return (1, t.shape[0], t.shape[3], t.shape[1], t.shape[2]), (0, s[0], s[3], s[1], s[2])
    if layout == "hwc" and t.dim() == 5:            # [B, T, H, W, C]
        return (t.shape[0], t.shape[1], t.shape[4], t.shape[2], t.shape[3]), (s[0], s[1], s[4], s[2], s[3])
    if layout == "chw" and t.dim() == 4:            # [n, C, H, W]
        return (1, t.shape[0], t.shape[1], t.shape[2], t.shape[3]), (0, s[0], s[1], s[2], s[3])
    if layout == "bcthw" and t.dim() == 5:          # [B, C, T, H, W]
        return (t.shape[0], t.shape[2], t.shape[1], t.shape[3], t.shape[4]), (s[0], s[2], s[1], s[3], s[4])
    if layout == "bfchw" and t.dim() == 5:          # [B, F, C, H, W]
        return (t.shape[0], t.shape[1], t.shape[2], t.shape[3], t.shape[4]), (s[0], s[1], s[2], s[3], s[4])
    raise ValueError(f"layout {layout!r} does not describe a tensor of shape {tuple(t.shape)} (hwc: [F, H, W, C] / [B, T, H, W, C]; chw: [n, C, H, W]; bcthw; bfchw)")


def _image_args(tensors, layout, crop_border, channels, min_side, least):
    """What the wrappers that read an image batch share, everything but the device: tensors ((t, name), ..) of one dtype (uint8, fp32, bf16) and one shape in `layout`
    (IMAGE_LAYOUTS), any views; C must be one of `channels`, and the plane without `crop_border` pixels on every side at least min_side x min_side (`least` names that
    in the refusal).  -> (n_outer, n_inner, C, H, W, h, w, the tensors' element strides, their base offsets in elements: where the cropped plane starts)"""
    for t, name in tensors:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: expected a tensor")
        if t.dtype not in _IMAGE_DTYPES:
            raise TypeError(f"{name}: expected uint8, float32 or bfloat16, got {t.dtype}")
    first, rest = tensors[0][0], [t for t, _ in tensors[1:]]
    if any(t.dtype != first.dtype for t in rest):
        raise TypeError(f"a and b must have one dtype, got {first.dtype} and {rest[0].dtype}")
    if layout not in IMAGE_LAYOUTS:
        raise ValueError(f"layout must be one of {sorted(IMAGE_LAYOUTS)}, got {layout!r}")
    if any(t.shape != first.shape for t in rest):
        raise ValueError(f"image shapes are different: {tuple(first.shape)}, {tuple(rest[0].shape)}")
    (n_outer, n_inner, Cn, H, W), _ = _image_strides(first, layout)
    strides = [_image_strides(t, layout)[1] for t, _ in tensors]
    if Cn not in channels:
        raise ValueError(f"expected {' or '.join(map(str, channels))} channels, got {Cn}")
    cb = int(crop_border)
    h, w = H - 2 * cb, W - 2 * cb
    if cb < 0 or h < min_side or w < min_side:
        raise ValueError(f"a {H} x {W} plane with crop_border {cb} is smaller than {least}")
    if n_outer * n_inner < 1:
        raise ValueError("no images")
    if min(min(st) for st in strides) < 0:
        raise ValueError("views with negative strides are not supported")
    return n_outer, n_inner, Cn, H, W, h, w, strides, [cb * (st[3] + st[4]) for st in strides]


def image_metrics(a, b, layout, crop_border=0, y_only=False):
    """tg_image_metrics: per image plane of two equally shaped uint8 (0..255), fp32 or bf16 (in [0, 1]) image batches, float64 [n_outer, n_inner, planes, 2] =
    (sum of squared differences on the 0..255 scale over the plane, sum of the SSIM map over its (h - 10) x (w - 10) window positions), h x w the plane without
    `crop_border` pixels on every side; planes = C, or 1 with y_only (C == 3: BT.601 luma).  layout names the axes (IMAGE_LAYOUTS); a and b may be any views with
    non-negative strides, the crop costs no copy.  One call for all planes; a plane's numbers do not depend on the other planes of the call."""
    n_outer, n_inner, Cn, _, _, h, w, (sa, sb), (oa, ob) = _image_args(((a, "a"), (b, "b")), layout, crop_border, (3,) if y_only else (1, 3), IMAGE_WINDOW,
                                                                       f"the {IMAGE_WINDOW} x {IMAGE_WINDOW} window")
    if not (a.is_cuda and b.is_cuda) or a.device != b.device:
        raise RuntimeError("image_metrics: expected two tensors on one GPU (tokensgen_amd has no CPU fallback)")
    lib = L.load()
    planes = n_outer * n_inner * (1 if y_only else Cn)
    ws = torch.empty(lib.tg_image_metrics_ws_doubles(planes, h, w), dtype=torch.float64, device=a.device)
    out = torch.empty(n_outer, n_inner, planes // (n_outer * n_inner), 2, dtype=torch.float64, device=a.device)
    pa, pb = a.data_ptr() + oa * a.element_size(), b.data_ptr() + ob * b.element_size()
    L.check(_launch("image_metrics", lib.tg_image_metrics, pa, *sa, pb, *sb, _IMAGE_DTYPES[a.dtype], n_outer, n_inner, Cn, h, w, int(bool(y_only)), _p(ws), _p(out),
                    _stream()), "tg_image_metrics")
    return out


LPIPS_MIN_SIDE = 16            # four floor-mode 2 x 2 pools leave at least one pixel at the last tap


def lpips_conv_in(x, layout, weight, bias, out, crop_border=0, normalize=False, outer=None, inner=None):
    """tg_lpips_conv_in: the pixel ends, the LPIPS scaling layer, conv1_1, bias and ReLU of an image batch -> `out`, bf16 channels-last [F, h, w, 64] (h x w the
    plane without `crop_border` pixels on every side).  x: uint8 (0..255), fp32 or bf16 (in [-1, 1], or in [0, 1] with normalize) in one of IMAGE_LAYOUTS with 3
    channels, any view with non-negative strides.  outer: only that outer index; inner = (first, count): only those inner indices (a chunk of a clip: a base offset,
    no copy); F = the images taken.  weight fp32 [64, 27], bias fp32 [64]."""
    n_outer, n_inner, _, _, _, h, w, (st,), (off,) = _image_args(((x, "x"),), layout, crop_border, (3,), LPIPS_MIN_SIDE, f"{LPIPS_MIN_SIDE} x {LPIPS_MIN_SIDE}")
    if normalize and x.dtype == torch.uint8:
        raise ValueError("normalize is for float inputs in [0, 1]; uint8 frames are read as 2 (v / 255) - 1")
    if outer is not None:
        if not 0 <= outer < n_outer:
            raise ValueError(f"outer index {outer} out of range 0..{n_outer - 1}")
        off, n_outer = off + outer * st[0], 1
    if inner is not None:
        first, count = inner
        if not (0 <= first and count >= 1 and first + count <= n_inner):
            raise ValueError(f"inner range {inner} out of range 0..{n_inner}")
        off, n_inner = off + first * st[1], count
    if tuple(weight.shape) != (64, 27) or tuple(bias.shape) != (64,) or not weight.is_contiguous() or not bias.is_contiguous():
        raise ValueError(f"weight / bias: expected contiguous [64, 27] / [64], got {tuple(weight.shape)} / {tuple(bias.shape)}")
    if tuple(out.shape) != (n_outer * n_inner, h, w, 64) or not out.is_contiguous():
        raise ValueError(f"out: expected contiguous {(n_outer * n_inner, h, w, 64)}, got {tuple(out.shape)}")
    if not x.is_cuda:
        raise RuntimeError("lpips_conv_in: expected a GPU tensor (tokensgen_amd has no CPU fallback)")
    _chk(weight, "weight", torch.float32); _chk(bias, "bias", torch.float32); _chk(out, "out")
    L.check(_launch("lpips_conv_in", L.load().tg_lpips_conv_in, x.data_ptr() + off * x.element_size(), *st, _IMAGE_DTYPES[x.dtype], int(bool(normalize)), n_outer,
                    n_inner, h, w, _p(weight), _p(bias), _p(out), _stream()), "tg_lpips_conv_in")
    return out


def relu_cl_(x):
    """tg_relu_cl: F.relu in place on a contiguous bf16 tensor whose element count is a multiple of 8."""
    _chk(x, "x")
    if not x.is_contiguous() or x.numel() % 8 != 0 or x.numel() == 0:
        raise ValueError(f"x: expected a contiguous tensor with a positive multiple of 8 elements, got {tuple(x.shape)}")
    L.check(_launch("relu_cl", L.load().tg_relu_cl, _p(x), x.numel(), _stream()), "tg_relu_cl")
    return x


def relu_maxpool2_cl(x):
    """tg_relu_maxpool2_cl: x bf16 [F, H, W, C] channels-last -> F.max_pool2d(F.relu(x), 2, 2) as [F, H // 2, W // 2, C] (floor)."""
    _chk(x, "x")
    if x.dim() != 4 or not x.is_contiguous() or x.shape[0] < 1 or x.shape[1] < 2 or x.shape[2] < 2 or x.shape[3] % 8 != 0 or x.shape[3] == 0:
        raise ValueError(f"x: expected contiguous [F, H >= 2, W >= 2, C % 8 == 0], got {tuple(x.shape)}")
    F, H, W, Cn = x.shape
    y = torch.empty(F, H // 2, W // 2, Cn, dtype=BF16, device=x.device)
    L.check(_launch("relu_maxpool2_cl", L.load().tg_relu_maxpool2_cl, _p(x), F, H, W, Cn, _p(y), _stream()), "tg_relu_maxpool2_cl")
    return y


def lpips_head(fa, fb, w, relu_on_load=False):
    """tg_lpips_head: fa, fb bf16 [F, H, W, C] channels-last (C in 64 / 128 / 256 / 512), w fp32 [C] -> float64 [F]: per frame the SUM over the pixels of
    sum_c w[c] (a_c / (|a| + 1e-10) - b_c / (|b| + 1e-10))^2, the features after F.relu with relu_on_load.  A frame's value does not depend on the other frames."""
    _chk(fa, "fa"); _chk(fb, "fb"); _chk(w, "w", torch.float32)
    if fa.dim() != 4 or fa.shape != fb.shape or not fa.is_contiguous() or not fb.is_contiguous() or fa.shape[0] < 1:
        raise ValueError(f"fa, fb: expected two contiguous [F, H, W, C] tensors of one shape, got {tuple(fa.shape)} and {tuple(fb.shape)}")
    F, H, W, Cn = fa.shape
    if Cn not in (64, 128, 256, 512) or tuple(w.shape) != (Cn,):
        raise ValueError(f"expected C in (64, 128, 256, 512) and w [C], got C = {Cn} and w {tuple(w.shape)}")
    lib = L.load()
    ws = torch.empty(lib.tg_lpips_head_ws_doubles(F, H, W), dtype=torch.float64, device=fa.device)
    out = torch.empty(F, dtype=torch.float64, device=fa.device)
    L.check(_launch("lpips_head", lib.tg_lpips_head, _p(fa), _p(fb), _p(w), F, H, W, Cn, int(bool(relu_on_load)), _p(ws), _p(out), _stream()), "tg_lpips_head")
    return out


def rmsnorm(x, weight, out, eps=1e-6):
    """tg_rmsnorm (T5LayerNorm): out = weight * bf16(x * rsqrt(mean(x^2) + eps)) over the last dimension; x, out [.., D] views with contiguous rows of one row
    stride (D % 64 == 0), weight [D]."""
    _chk(x, "x"); _chk(weight, "weight"); _chk(out, "out")
    D = x.shape[-1]
    x2, o2 = x.reshape(-1, D) if x.dim() != 2 else x, out.reshape(-1, D) if out.dim() != 2 else out
    if x2.data_ptr() != x.data_ptr() or o2.data_ptr() != out.data_ptr() or x2.shape != o2.shape or tuple(weight.shape) != (D,) or not weight.is_contiguous():
        raise ValueError(f"rmsnorm: x{tuple(x.shape)} and out{tuple(out.shape)} must be views with one row stride over [rows, D], weight [D]")
    L.check(_launch("rmsnorm", L.load().tg_rmsnorm, _p(x2), x2.stride(0), _p(weight), _p(o2), o2.stride(0), x2.shape[0], D, float(eps), _stream()), "tg_rmsnorm")
    return out


def t5_attention(qkv, bias_by_distance, out, heads):
    """tg_t5_attention on the fused projection: qkv [B, S, 3 * heads * 64] (q | k | v along the last dimension, a view with row / batch strides allowed),
    bias_by_distance fp32 [heads, 2 S - 1], out contiguous [B, S, heads * 64]: softmax_fp32(q k^T + bias) v per head, unscaled and unmasked.  1 <= S <= 512."""
    _chk(qkv, "qkv"); _chk(bias_by_distance, "bias_by_distance", torch.float32); _chk(out, "out")
    if qkv.dim() != 3 or qkv.shape[2] != 3 * heads * 64:
        raise ValueError(f"t5_attention: qkv must be [B, S, {3 * heads * 64}], got {tuple(qkv.shape)}")
    B, S, _ = qkv.shape
    inner = heads * 64
    if tuple(out.shape) != (B, S, inner) or not out.is_contiguous() or tuple(bias_by_distance.shape) != (heads, 2 * S - 1) or not bias_by_distance.is_contiguous():
        raise ValueError(f"t5_attention: out must be contiguous {(B, S, inner)} and bias_by_distance contiguous {(heads, 2 * S - 1)}, got {tuple(out.shape)} and "
                         f"{tuple(bias_by_distance.shape)}")
    p = qkv.data_ptr()
    L.check(_launch("t5_attention", L.load().tg_t5_attention, p, p + 2 * inner, p + 4 * inner, qkv.stride(1), qkv.stride(0), _p(bias_by_distance), _p(out), B, S, heads,
                    _stream()), "tg_t5_attention")
    return out


def gated_gelu(h, out):
    """tg_gated_gelu: out [.., F] = bf16(gelu_tanh(h[.., :F]) * h[.., F:]), h [.., 2 F] the output of one GEMM over wi_0 | wi_1; both contiguous."""
    _chk(h, "h"); _chk(out, "out")
    F = out.shape[-1]
    if h.shape[-1] != 2 * F or h.shape[:-1] != out.shape[:-1] or not h.is_contiguous() or not out.is_contiguous():
        raise ValueError(f"gated_gelu: expected contiguous h [.., 2 F] and out [.., F], got {tuple(h.shape)} and {tuple(out.shape)}")
    L.check(_launch("gated_gelu", L.load().tg_gated_gelu, _p(h), 2 * F, _p(out), F, out.numel() // max(F, 1), F, _stream()), "tg_gated_gelu")
    return out


def residual_add(x, y, out):
    """tg_residual_add: out = bf16(x + y), three contiguous tensors of one shape (out may be x)."""
    _chk(x, "x"); _chk(y, "y"); _chk(out, "out")
    if not (x.shape == y.shape == out.shape) or not (x.is_contiguous() and y.is_contiguous() and out.is_contiguous()):
        raise ValueError(f"residual_add: expected three contiguous tensors of one shape, got {tuple(x.shape)}, {tuple(y.shape)}, {tuple(out.shape)}")
    L.check(_launch("residual_add", L.load().tg_residual_add, _p(x), _p(y), _p(out), x.numel(), _stream()), "tg_residual_add")
    return out


def vit_patch_rows(frames, patch, a, b, out):
    """tg_vit_patch_rows: frames bf16 [F, 3, H, W] contiguous -> out[:F * (H / patch) * (W / patch)] (out: contiguous [rows >= that, Kp], Kp = 3 patch^2 rounded up
    to a multiple of 64) = bf16(frames * a[c] + b[c]) in the column order (c, dy, dx), pad columns zero.  a, b: three Python floats each."""
    _chk(frames, "frames"); _chk(out, "out")
    if frames.dim() != 4 or frames.shape[1] != 3 or not frames.is_contiguous() or out.dim() != 2 or not out.is_contiguous():
        raise ValueError(f"vit_patch_rows: expected contiguous frames [F, 3, H, W] and out [rows, Kp], got {tuple(frames.shape)} and {tuple(out.shape)}")
    F, _, H, W = frames.shape
    if H % patch or W % patch or out.shape[0] < F * (H // patch) * (W // patch):
        raise ValueError(f"vit_patch_rows: {H} x {W} frames do not divide into patches of {patch}, or out{tuple(out.shape)} has too few rows")
    fa, fb = (C.c_float * 3)(*a), (C.c_float * 3)(*b)
    L.check(_launch("vit_patch_rows", L.load().tg_vit_patch_rows, _p(frames), F, H, W, int(patch), fa, fb, _p(out), out.shape[1], _stream()), "tg_vit_patch_rows")
    return out


def vit_assemble(patch, cls, pos, tok):
    """tg_vit_assemble: tok [F, S, D] = (cls | patch[f * P + i]) + pos, S = P + 1; patch contiguous [rows >= F * P, D], cls [D], pos [S, D], all bf16."""
    _chk(patch, "patch"); _chk(cls, "cls"); _chk(pos, "pos"); _chk(tok, "tok")
    if tok.dim() != 3 or not (tok.is_contiguous() and patch.is_contiguous() and cls.is_contiguous() and pos.is_contiguous()):
        raise ValueError("vit_assemble: expected contiguous tok [F, S, D], patch [rows, D], cls [D] and pos [S, D]")
    F, S, D = tok.shape
    if patch.dim() != 2 or patch.shape[1] != D or patch.shape[0] < F * (S - 1) or cls.numel() != D or tuple(pos.shape) != (S, D) or S < 2:
        raise ValueError(f"vit_assemble: tok{tuple(tok.shape)} needs patch [>= {F * (S - 1)}, {D}], cls [{D}] and pos [{S}, {D}]; got {tuple(patch.shape)}, "
                         f"{tuple(cls.shape)}, {tuple(pos.shape)}")
    L.check(_launch("vit_assemble", L.load().tg_vit_assemble, _p(patch), _p(cls), _p(pos), _p(tok), F, S - 1, D, _stream()), "tg_vit_assemble")
    return tok


def layernorm(x, weight, bias, out, eps):
    """tg_layernorm (nn.LayerNorm over the last dimension): x, out [rows, D] views with one row stride each (D % 64 == 0, D <= 4096), weight and bias [D]."""
    _chk(x, "x"); _chk(weight, "weight"); _chk(bias, "bias"); _chk(out, "out")
    D = x.shape[-1]
    if x.dim() != 2 or out.shape != x.shape or tuple(weight.shape) != (D,) or tuple(bias.shape) != (D,) or not (weight.is_contiguous() and bias.is_contiguous()):
        raise ValueError(f"layernorm: expected x and out [rows, D] of one shape, weight and bias [D]; got {tuple(x.shape)}, {tuple(out.shape)}, {tuple(weight.shape)}")
    L.check(_launch("layernorm", L.load().tg_layernorm, _p(x), x.stride(0), _p(weight), _p(bias), _p(out), out.stride(0), x.shape[0], D, float(eps), _stream()),
            "tg_layernorm")
    return out


VIT_ACT = {"gelu": 0, "quick_gelu": 1}


def vit_act(x, out, mode):
    """tg_vit_act: out = bf16(act(x)) on two contiguous bf16 tensors of one shape (out may be x); mode "gelu" (the exact, erf form) or "quick_gelu"."""
    _chk(x, "x"); _chk(out, "out")
    if x.shape != out.shape or not (x.is_contiguous() and out.is_contiguous()):
        raise ValueError(f"vit_act: expected two contiguous tensors of one shape, got {tuple(x.shape)} and {tuple(out.shape)}")
    L.check(_launch("vit_act", L.load().tg_vit_act, _p(x), _p(out), x.numel(), VIT_ACT[mode], _stream()), "tg_vit_act")
    return out


def feature_consistency(feat, first=None, prev=None):
    """tg_feature_consistency: feat fp32 [F, D] (a row stride allowed) -> (prev, first), float64 [F - 1]: max(0, cos) of frames 1 .. F - 1 with their predecessor and
    with frame 0.  With the carried rows `first` and `prev` (fp32 [D], both or neither: the first and the last feature of the video so far) -> float64 [F], frame 0
    compared with `prev`, every frame with `first`."""
    _chk(feat, "feat", torch.float32)
    if feat.dim() != 2 or (first is None) != (prev is None):
        raise ValueError("feature_consistency: expected feat [F, D] and both carried rows or neither")
    F, D = feat.shape
    for t, name in ((first, "first"), (prev, "prev")):
        if t is not None and (_chk(t, name, torch.float32).numel() != D or not t.is_contiguous()):
            raise ValueError(f"feature_consistency: {name} must be a contiguous row of {D} elements, got {tuple(t.shape)}")
    n = F if first is not None else F - 1
    if n < 1:
        raise ValueError(f"feature_consistency: no frame with a predecessor among {F}")
    out = torch.empty(2, n, dtype=torch.float64, device=feat.device)
    L.check(_launch("feature_consistency", L.load().tg_feature_consistency, _p(feat), feat.stride(0), F, D, _p(first), _p(prev), _p(out[0]), _p(out[1]), _stream()),
            "tg_feature_consistency")
    return out[0], out[1]


def text_embed(ids, seq, tok_emb, pos_emb, out, status):
    """tg_text_embed: out[r] = bf16(tok_emb[ids[r]] + pos_emb[r % seq]) for the int32 ids [rows] (rows a multiple of seq); tok_emb bf16 [V, D], pos_emb bf16 [>= seq, D],
    out bf16 [>= rows, D] with a row stride, status int32 [1] on the device: incremented once per id outside [0, V), whose row is written as zeros."""
    _chk(ids, "ids", torch.int32); _chk(tok_emb, "tok_emb"); _chk(pos_emb, "pos_emb"); _chk(out, "out"); _chk(status, "status", torch.int32)
    rows = ids.numel()
    if ids.dim() != 1 or rows < 1 or seq < 1 or rows % seq or tok_emb.dim() != 2 or pos_emb.dim() != 2 or out.dim() != 2 or status.numel() != 1:
        raise ValueError(f"text_embed: expected ids [rows] with rows a multiple of seq = {seq}, tok_emb [V, D], pos_emb [P, D], out [>= rows, D] and status [1]; got "
                         f"{tuple(ids.shape)}, {tuple(tok_emb.shape)}, {tuple(pos_emb.shape)}, {tuple(out.shape)}, {tuple(status.shape)}")
    V, D = tok_emb.shape
    if pos_emb.shape[0] < seq or pos_emb.shape[1] != D or out.shape[1] != D or out.shape[0] < rows or not (tok_emb.is_contiguous() and pos_emb.is_contiguous()):
        raise ValueError(f"text_embed: tok_emb{tuple(tok_emb.shape)} needs contiguous pos_emb [>= {seq}, {D}] and out [>= {rows}, {D}]; got {tuple(pos_emb.shape)} and "
                         f"{tuple(out.shape)}")
    L.check(_launch("text_embed", L.load().tg_text_embed, _p(ids), rows, int(seq), _p(tok_emb), V, _p(pos_emb), _p(out), out.stride(0), D, _p(status), _stream()),
            "tg_text_embed")
    return out


def text_alignment(img, txt):
    """tg_text_alignment: img fp32 [F, D], txt fp32 [K, D] (row strides allowed) -> float64 [F, K]: cos(img[f], txt[k]) = x . y / (max(|x|, 1e-8) max(|y|, 1e-8)),
    not clamped.  Bitwise reproducible; an output depends on its two rows alone."""
    _chk(img, "img", torch.float32); _chk(txt, "txt", torch.float32)
    if img.dim() != 2 or txt.dim() != 2 or img.shape[1] != txt.shape[1] or img.shape[0] < 1 or txt.shape[0] < 1:
        raise ValueError(f"text_alignment: expected img [F, D] and txt [K, D] of one width, got {tuple(img.shape)} and {tuple(txt.shape)}")
    (F, D), Kt = img.shape, txt.shape[0]
    out = torch.empty(F, Kt, dtype=torch.float64, device=img.device)
    L.check(_launch("text_alignment", L.load().tg_text_alignment, _p(img), img.stride(0), F, _p(txt), txt.stride(0), Kt, D, _p(out), _stream()), "tg_text_alignment")
    return out


MOTION_BLOCKS, MOTION_MAX_RADIUS = (8, 16), 32


def luma_u8(frames):
    """tg_luma_u8: uint8 RGB frames [F, H, W, 3] / [B, T, H, W, 3] (any view) -> uint8 luma planes [n_outer, n_inner, H, pitch], pitch = W rounded up to a multiple of
    4 (pad bytes 0); Y = (77 R + 150 G + 29 B + 128) >> 8."""
    (no, ni, H, W), st = _chk_rgb(frames, "frames")
    if no * ni < 1 or H < 1 or W < 1:
        raise ValueError(f"luma_u8: no pixels in {tuple(frames.shape)}")
    lib = L.load()
    out = torch.empty(no, ni, H, lib.tg_luma_pitch(W), dtype=torch.uint8, device=frames.device)
    L.check(_launch("luma_u8", lib.tg_luma_u8, _p(frames), *st, no, ni, H, W, _p(out), _stream()), "tg_luma_u8")
    return out


def _chk_planes(prev, nxt, width, block, who):
    for t, name in ((prev, "prev"), (nxt, "next")):
        _chk(t, name, torch.uint8)
    if prev.dim() != 4 or prev.shape != nxt.shape or prev.stride()[2:] != (prev.shape[3], 1) or nxt.stride()[2:] != (nxt.shape[3], 1) or min(prev.stride() + nxt.stride()) < 0:
        raise ValueError(f"{who}: expected two equally shaped stacks of packed planes [n_outer, n_inner, H, pitch], got {tuple(prev.shape)} and {tuple(nxt.shape)}")
    no, ni, H, pitch = prev.shape
    if block not in MOTION_BLOCKS or no * ni < 1 or not block <= int(width) <= pitch or H < block:
        raise ValueError(f"{who}: block {block} (8 or 16), planes {tuple(prev.shape)} of width {width}")
    return no, ni, H, pitch


def block_motion(cur, ref, width, block, radius):
    """tg_block_motion: cur, ref uint8 luma planes [n_outer, n_inner, H, pitch] from luma_u8 (views along the first two axes allowed: a video's planes 0 .. T - 2 and
    1 .. T - 1), width = the planes' true W.  Returns mv int16 [n_outer, n_inner, Hb, Wb, 2] (dy, dx), sad and sad0 int32 [n_outer, n_inner, Hb, Wb]."""
    block, radius, W = int(block), int(radius), int(width)
    no, ni, H, pitch = _chk_planes(cur, ref, W, block, "block_motion")
    if not 1 <= radius <= MOTION_MAX_RADIUS:
        raise ValueError(f"block_motion: radius must be in 1..{MOTION_MAX_RADIUS}, got {radius}")
    Hb, Wb = H // block, W // block
    mv = torch.empty(no, ni, Hb, Wb, 2, dtype=torch.int16, device=cur.device)
    sad = torch.empty(2, no, ni, Hb, Wb, dtype=torch.int32, device=cur.device)
    L.check(_launch("block_motion", L.load().tg_block_motion, _p(cur), cur.stride(0), cur.stride(1), _p(ref), ref.stride(0), ref.stride(1), no, ni, H, W, pitch, block,
                    radius, _p(mv), _p(sad[0]), _p(sad[1]), _stream()), "tg_block_motion")
    return mv, sad[0], sad[1]


def block_warp_sse(cur, ref, mv, block):
    """tg_block_warp_sse: cur, ref uint8 RGB frames of one shape ([F, H, W, 3] / [B, T, H, W, 3], any views), pair i of cur against pair i of ref; mv int16
    [n_outer, n_inner, Hb, Wb, 2] contiguous.  Returns sse, sse0 int32 [n_outer, n_inner, Hb, Wb] and status int32 [1] (vectors that had to be clamped)."""
    (no, ni, H, W), sa = _chk_rgb(cur, "cur")
    _, sb = _chk_rgb(ref, "ref")
    block = int(block)
    if cur.shape != ref.shape or block not in MOTION_BLOCKS or no * ni < 1 or H < block or W < block:
        raise ValueError(f"block_warp_sse: frames {tuple(cur.shape)} and {tuple(ref.shape)} with block {block}")
    Hb, Wb = H // block, W // block
    _chk_vec(mv, "mv", torch.int16, (no, ni, Hb, Wb, 2))
    sse = torch.empty(2, no, ni, Hb, Wb, dtype=torch.int32, device=cur.device)
    status = torch.zeros(1, dtype=torch.int32, device=cur.device)
    L.check(_launch("block_warp_sse", L.load().tg_block_warp_sse, _p(cur), *sa, _p(ref), *sb, _p(mv), no, ni, H, W, block, _p(sse[0]), _p(sse[1]), _p(status),
                    _stream()), "tg_block_warp_sse")
    return sse[0], sse[1], status


MCI_FACTORS = (2, 8)


def mci_select(prev, nxt, fwd, bwd, width, block, factor):
    """tg_mci_select: prev, nxt uint8 luma planes [n_outer, n_inner, H, pitch] from luma_u8 (views along the first two axes allowed); fwd, bwd int16
    [n_outer, n_inner, Hb, Wb, 2] contiguous, the fields of block_motion(prev, nxt) and block_motion(nxt, prev) (bwd may be None).  Returns mvi int16
    [n_outer, n_inner, factor - 1, Hb, Wb, 2] and cost int32 [n_outer, n_inner, factor - 1, Hb, Wb]."""
    block, n, W = int(block), int(factor), int(width)
    no, ni, H, pitch = _chk_planes(prev, nxt, W, block, "mci_select")
    if not MCI_FACTORS[0] <= n <= MCI_FACTORS[1]:
        raise ValueError(f"mci_select: factor must be in {MCI_FACTORS[0]}..{MCI_FACTORS[1]}, got {n}")
    Hb, Wb = H // block, W // block
    for t, name in ((fwd, "fwd"), (bwd, "bwd")):
        if t is None and name == "bwd":
            continue
        _chk_vec(t, name, torch.int16, (no, ni, Hb, Wb, 2))
    mvi = torch.empty(no, ni, n - 1, Hb, Wb, 2, dtype=torch.int16, device=prev.device)
    cost = torch.empty(no, ni, n - 1, Hb, Wb, dtype=torch.int32, device=prev.device)
    L.check(_launch("mci_select", L.load().tg_mci_select, _p(prev), prev.stride(0), prev.stride(1), _p(nxt), nxt.stride(0), nxt.stride(1), _p(fwd),
                    None if bwd is None else _p(bwd), no, ni, H, W, pitch, block, n, _p(mvi), _p(cost), _stream()), "tg_mci_select")
    return mvi, cost


def mci_render(prev, nxt, mvi, block, factor, out):
    """tg_mci_render: prev, nxt uint8 RGB frames of one shape ([B, P, H, W, 3], any views), mvi int16 [B, P, factor - 1, Hb, Wb, 2] contiguous; out uint8
    [B, P * factor + 1, H, W, 3] contiguous: frame i * factor + k of out is written for every pair i and phase k = 1 .. factor - 1, the frames i * factor are left alone."""
    (no, ni, H, W), sa = _chk_rgb(prev, "prev")
    _, sb = _chk_rgb(nxt, "next")
    block, n = int(block), int(factor)
    if prev.dim() != 5 or prev.shape != nxt.shape or block not in MOTION_BLOCKS or not MCI_FACTORS[0] <= n <= MCI_FACTORS[1]:
        raise ValueError(f"mci_render: frames {tuple(prev.shape)} and {tuple(nxt.shape)} ([B, P, H, W, 3]) with block {block}, factor {n}")
    if no * ni < 1 or H < block or W < block:
        raise ValueError(f"mci_render: frames {tuple(prev.shape)} hold no {block} x {block} block")
    Hb, Wb = H // block, W // block
    _chk_vec(mvi, "mvi", torch.int16, (no, ni, n - 1, Hb, Wb, 2))
    _chk_vec(out, "out", torch.uint8, (no, ni * n + 1, H, W, 3))
    L.check(_launch("mci_render", L.load().tg_mci_render, _p(prev), *sa, _p(nxt), *sb, _p(mvi), no, ni, H, W, block, n, _p(out), out.stride(0), out.stride(1),
                    _stream()), "tg_mci_render")
    return out


COLOR_MODES = {"meanstd": 0, "histogram": 1}
COLOR_MAX_WINDOW = 64


def color_hist_u8(frames):
    """tg_color_hist_u8: contiguous uint8 [F, H, W, 3] -> int32 [F, 3, 256], the counts per frame, channel and value (exact; a frame's counts depend on it alone)."""
    (_, F, H, W), _ = _chk_rgb(frames, "color_hist_u8", contiguous=True)
    out = torch.empty(F, 3, 256, dtype=torch.int32, device=frames.device)
    L.check(_launch("color_hist_u8", L.load().tg_color_hist_u8, _p(frames), F, H, W, _p(out), _stream()), "tg_color_hist_u8")
    return out


def color_match_lut(hist, anchor, mode, strength, window, max_gain, history=None, status=None):
    """tg_color_match_lut: hist int32 [F, 3, 256], anchor int64 [3, 256], history None or int32 [n, 3, 256] (the n < window frames before the call's, oldest first)
    -> (lut uint8 [F, 3, 256], status int32 [1]: the number of (frame, channel) histograms the device refused and gave the identity table)."""
    _chk(hist, "hist", torch.int32)
    if hist.dim() != 3 or tuple(hist.shape[1:]) != (3, 256) or hist.shape[0] < 1 or not hist.is_contiguous():
        raise ValueError(f"color_match_lut: hist must be contiguous [F, 3, 256], got {tuple(hist.shape)}")
    _chk_vec(anchor, "anchor", torch.int64, (3, 256))
    n_hist = 0
    if history is not None and history.shape[0] > 0:
        _chk(history, "history", torch.int32)
        if history.dim() != 3 or tuple(history.shape[1:]) != (3, 256) or not history.is_contiguous() or history.shape[0] >= window:
            raise ValueError(f"color_match_lut: history must be contiguous [n, 3, 256] with n < window = {window}, got {tuple(history.shape)}")
        n_hist = history.shape[0]
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=hist.device)
    else:
        _chk(status, "status", torch.int32)
    lut = torch.empty(hist.shape[0], 3, 256, dtype=torch.uint8, device=hist.device)
    L.check(_launch("color_match_lut", L.load().tg_color_match_lut, _p(hist), hist.shape[0], _p(history) if n_hist else None, n_hist, _p(anchor), COLOR_MODES[mode],
                    float(strength), int(window), float(max_gain), _p(lut), _p(status), _stream()), "tg_color_match_lut")
    return lut, status


def color_apply_lut(frames, lut, out=None):
    """tg_color_apply_lut: out[f, y, x, c] = lut[f, c, frames[f, y, x, c]]; frames contiguous uint8 [F, H, W, 3], lut uint8 [F, 3, 256] contiguous; out None (a new
    tensor), `frames` itself (in place) or another contiguous tensor of its shape."""
    (_, F, H, W), _ = _chk_rgb(frames, "color_apply_lut", contiguous=True)
    _chk_vec(lut, "lut", torch.uint8, (F, 3, 256))
    if out is None:
        out = torch.empty_like(frames)
    elif _chk_rgb(out, "color_apply_lut: out", contiguous=True)[0] != (1, F, H, W) or out.device != frames.device:
        raise ValueError(f"color_apply_lut: out must have the frames' shape {tuple(frames.shape)} and device, got {tuple(out.shape)}")
    L.check(_launch("color_apply_lut", L.load().tg_color_apply_lut, _p(frames), _p(lut), F, H, W, _p(out), _stream()), "tg_color_apply_lut")
    return out


def lab_metrics(a, b, layout, crop_border=0):
    """tg_lab_metrics: per frame of one (b None) or two equally shaped uint8 (0..255), fp32 or bf16 (in [0, 1]) RGB image batches the float64 sums over the h x w pixels
    (the plane without `crop_border` pixels on every side) of CIE L*, a*, b*, C*ab of `a` -> [n_outer, n_inner, 4], and with b also those of b and of the CIE76
    dE between them -> [n_outer, n_inner, 9].  layout, views and the crop as image_metrics; a frame's sums do not depend on the other frames of the call."""
    n_outer, n_inner, _, _, _, h, w, st, off = _image_args(((a, "a"),) + (((b, "b"),) if b is not None else ()), layout, crop_border, (3,), 1, "one pixel")
    if not a.is_cuda or (b is not None and (not b.is_cuda or a.device != b.device)):
        raise RuntimeError("lab_metrics: expected tensors on one GPU (tokensgen_amd has no CPU fallback)")
    lib = L.load()
    ns = 4 if b is None else 9
    ws = torch.empty(lib.tg_lab_metrics_ws_doubles(n_outer * n_inner, h, w, int(b is not None)), dtype=torch.float64, device=a.device)
    out = torch.empty(n_outer, n_inner, ns, dtype=torch.float64, device=a.device)
    pa = a.data_ptr() + off[0] * a.element_size()
    pb, sb = (None, (0, 0, 0, 0, 0)) if b is None else (b.data_ptr() + off[1] * b.element_size(), st[1])
    L.check(_launch("lab_metrics", lib.tg_lab_metrics, pa, *st[0], pb, *sb, _IMAGE_DTYPES[a.dtype], n_outer, n_inner, h, w, _p(ws), _p(out), _stream()), "tg_lab_metrics")
    return out


JPEG_SUBSAMPLINGS = {"420": 420, "444": 444}


def jpeg_geometry(H, W, subsampling, restart_interval=1):
    """tg_jpeg_geometry: (MCU rows, MCU columns, blocks per MCU, restart segments per frame) of an H x W frame; refused arguments raise."""
    lib = L.load()
    g = tuple(lib.tg_jpeg_geometry(H, W, JPEG_SUBSAMPLINGS.get(subsampling, 0), restart_interval, what) for what in range(4))
    if not all(g):
        raise ValueError(f"jpeg: a frame of {H} x {W} (1..65535), subsampling {subsampling!r} ({sorted(JPEG_SUBSAMPLINGS)}), restart_interval {restart_interval!r} (1..65535)")
    return g


def jpeg_coeffs(frames, quality, subsampling):
    """tg_jpeg_coeffs: contiguous uint8 [F, H, W, 3] -> int16 [F, MCUs, blocks per MCU, 64], the quantised DCT coefficients in zigzag order (the header's definition)."""
    (_, F, H, W), _ = _chk_rgb(frames, "jpeg_coeffs", contiguous=True)
    rows, cols, bpm, _ = jpeg_geometry(H, W, subsampling)
    coef = torch.empty(F, rows * cols, bpm, 64, dtype=torch.int16, device=frames.device)
    L.check(_launch("jpeg_coeffs", L.load().tg_jpeg_coeffs, _p(frames), F, H, W, JPEG_SUBSAMPLINGS[subsampling], int(quality), _p(coef), _stream()), "tg_jpeg_coeffs")
    return coef


def _chk_jpeg_coef(coef, H, W, subsampling, restart_interval, who):
    _chk(coef, "coef", torch.int16)
    rows, cols, bpm, n_seg = jpeg_geometry(H, W, subsampling, restart_interval)
    if coef.dim() != 4 or tuple(coef.shape[1:]) != (rows * cols, bpm, 64) or coef.shape[0] < 1 or not coef.is_contiguous():
        raise ValueError(f"{who}: coef must be contiguous [F, {rows * cols}, {bpm}, 64], got {tuple(coef.shape)}")
    return coef.shape[0], n_seg


def jpeg_segment_bytes(coef, H, W, subsampling, restart_interval):
    """tg_jpeg_segment_bytes: int32 [F, n_seg], the bytes of every restart segment with stuffing, fill and the marker that ends it (FF D9 for the last)."""
    F, n_seg = _chk_jpeg_coef(coef, H, W, subsampling, restart_interval, "jpeg_segment_bytes")
    out = torch.empty(F, n_seg, dtype=torch.int32, device=coef.device)
    L.check(_launch("jpeg_segment_bytes", L.load().tg_jpeg_segment_bytes, _p(coef), F, H, W, JPEG_SUBSAMPLINGS[subsampling], int(restart_interval), _p(out), _stream()),
            "tg_jpeg_segment_bytes")
    return out


def jpeg_write(coef, H, W, quality, subsampling, restart_interval, seg_offsets, frame_offsets, data):
    """tg_jpeg_write: the header and the segments of every frame into `data` (uint8 [n]) at frame_offsets (int64 [F]) and seg_offsets (int64 [F, n_seg])."""
    F, n_seg = _chk_jpeg_coef(coef, H, W, subsampling, restart_interval, "jpeg_write")
    _chk_vec(seg_offsets, "seg_offsets", torch.int64, (F, n_seg)); _chk_vec(frame_offsets, "frame_offsets", torch.int64, (F,)); _chk(data, "data", torch.uint8)
    if data.dim() != 1:
        raise ValueError(f"jpeg_write: data must be uint8 [n], got {tuple(data.shape)}")
    L.check(_launch("jpeg_write", L.load().tg_jpeg_write, _p(coef), F, H, W, JPEG_SUBSAMPLINGS[subsampling], int(quality), int(restart_interval), _p(seg_offsets),
                    _p(frame_offsets), _p(data), data.numel(), _stream()), "tg_jpeg_write")
    return data


# the bits of the decoder's status (TG_JPEG_ST_* of the header) and what each says
JPEG_STATUS = {1: "an invalid Huffman code", 2: "a coefficient index past 63", 4: "a DC category above 11 or an AC size above 10", 8: "a restart segment runs out of bits",
               16: "the count of restart markers is not that of the restart interval", 32: "a restart marker out of order", 64: "a byte range or table index outside its buffer"}


def jpeg_huff_table(bits, vals):
    """tg_jpeg_huff_table (host only): BITS (16 counts) and HUFFVAL -> the 912 bytes of one decoding table; ValueError for counts that do not add up or an
    over-subscribed code."""
    lib = L.load()
    bits, vals = bytes(bits), bytes(vals)
    if len(bits) != 16:
        raise ValueError(f"jpeg_huff_table: BITS has 16 counts, got {len(bits)}")
    out = (C.c_uint32 * (lib.tg_jpeg_huff_table_bytes() // 4))()
    if lib.tg_jpeg_huff_table(bits, vals, len(vals), C.addressof(out)) != 0:
        raise ValueError(lib.tg_last_error_string().decode())
    return bytes(out)


def jpeg_decode_segments(H, W, subsampling, restart_interval):
    """tg_jpeg_decode_segments: restart segments per frame, 1 for restart_interval 0 (no markers); refused arguments raise."""
    n = L.load().tg_jpeg_decode_segments(H, W, JPEG_SUBSAMPLINGS.get(subsampling, 0), restart_interval)
    if not n:
        raise ValueError(f"jpeg: a frame of {H} x {W} (1..65535), subsampling {subsampling!r} ({sorted(JPEG_SUBSAMPLINGS)}), restart_interval {restart_interval!r} (0..65535)")
    return n


def jpeg_find_segments(data, scan_begin, scan_end, n_seg, status):
    """tg_jpeg_find_segments: data uint8 [n], scan_begin / scan_end int64 [F] -> (seg_begin, seg_end) int64 [F, n_seg], the bytes of every restart segment; stores
    status (int32 [F])."""
    _chk(data, "data", torch.uint8)
    F = scan_begin.numel() if isinstance(scan_begin, torch.Tensor) else 0
    if data.dim() != 1 or data.numel() < 1 or not data.is_contiguous() or F < 1 or int(n_seg) < 1:
        raise ValueError(f"jpeg_find_segments: data uint8 [n >= 1], at least one frame and one segment; got {tuple(data.shape)}, F={F}, n_seg={n_seg}")
    _chk_vec(scan_begin, "scan_begin", torch.int64, (F,)); _chk_vec(scan_end, "scan_end", torch.int64, (F,)); _chk_vec(status, "status", torch.int32, (F,))
    seg_begin = torch.empty(F, int(n_seg), dtype=torch.int64, device=data.device)
    seg_end = torch.empty_like(seg_begin)
    L.check(_launch("jpeg_find_segments", L.load().tg_jpeg_find_segments, _p(data), data.numel(), _p(scan_begin), _p(scan_end), F, int(n_seg), _p(seg_begin), _p(seg_end),
                    _p(status), _stream()), "tg_jpeg_find_segments")
    return seg_begin, seg_end


def _chk_jpeg_decode_args(who, data, seg_begin, seg_end, H, W, subsampling, restart_interval, htabs, htab_index):
    """what tg_jpeg_decode_coeffs and tg_jpeg_decode_coeffs_sync both take -> (F, MCUs, blocks per MCU)"""
    _chk(data, "data", torch.uint8)
    n_seg = jpeg_decode_segments(H, W, subsampling, restart_interval)
    rows, cols, bpm, _ = jpeg_geometry(H, W, subsampling)
    _chk(seg_begin, "seg_begin", torch.int64)
    F = seg_begin.shape[0] if seg_begin.dim() == 2 else 0
    if data.dim() != 1 or data.numel() < 1 or not data.is_contiguous() or F < 1:
        raise ValueError(f"{who}: data uint8 [n >= 1], seg_begin [F, {n_seg}]; got {tuple(data.shape)}, {tuple(seg_begin.shape)}")
    _chk_vec(seg_begin, "seg_begin", torch.int64, (F, n_seg)); _chk_vec(seg_end, "seg_end", torch.int64, (F, n_seg))
    _chk_vec(htab_index, "htab_index", torch.int32, (F,))
    _chk(htabs, "htabs", torch.uint8)
    set_bytes = 6 * L.load().tg_jpeg_huff_table_bytes()
    if htabs.dim() != 2 or htabs.shape[0] < 1 or htabs.shape[1] != set_bytes or not htabs.is_contiguous():
        raise ValueError(f"{who}: htabs must be contiguous uint8 [sets, {set_bytes}], got {tuple(htabs.shape)}")
    return F, rows * cols, bpm


def jpeg_decode_coeffs(data, seg_begin, seg_end, H, W, subsampling, restart_interval, htabs, htab_index, status):
    """tg_jpeg_decode_coeffs: -> int16 [F, MCUs, blocks per MCU, 64], every coefficient written; htabs uint8 [sets, 6 * 912], htab_index int32 [F]; ORs into status."""
    F, n_mcu, bpm = _chk_jpeg_decode_args("jpeg_decode_coeffs", data, seg_begin, seg_end, H, W, subsampling, restart_interval, htabs, htab_index)
    _chk_vec(status, "status", torch.int32, (F,))
    coef = torch.empty(F, n_mcu, bpm, 64, dtype=torch.int16, device=data.device)
    L.check(_launch("jpeg_decode_coeffs", L.load().tg_jpeg_decode_coeffs, _p(data), data.numel(), _p(seg_begin), _p(seg_end), F, H, W, JPEG_SUBSAMPLINGS[subsampling],
                    int(restart_interval), _p(htabs), htabs.shape[0], _p(htab_index), _p(coef), _p(status), _stream()), "tg_jpeg_decode_coeffs")
    return coef


JPEG_SYNC_SUB_BYTES = (16, 32, 64, 128, 256)


def jpeg_decode_coeffs_sync(data, seg_begin, seg_end, H, W, subsampling, restart_interval, htabs, htab_index, sub_bytes, clean, rounds, coef=None):
    """tg_jpeg_decode_coeffs_sync: the coefficients of jpeg_decode_coeffs, decoded in parallel inside every restart segment, sub_bytes raw bytes per lane; stores
    clean (int32 [F]: 1 where the frame's coefficients are vouched for, 0 where the frame is to be decoded by jpeg_decode_coeffs) and rounds (int32 [F]); never
    touches a status.  `coef`: a contiguous int16 [F, MCUs, blocks per MCU, 64] to fill instead of a new one."""
    F, n_mcu, bpm = _chk_jpeg_decode_args("jpeg_decode_coeffs_sync", data, seg_begin, seg_end, H, W, subsampling, restart_interval, htabs, htab_index)
    if isinstance(sub_bytes, bool) or sub_bytes not in JPEG_SYNC_SUB_BYTES:
        raise ValueError(f"jpeg_decode_coeffs_sync: sub_bytes must be one of {JPEG_SYNC_SUB_BYTES}, got {sub_bytes!r}")
    _chk_vec(clean, "clean", torch.int32, (F,)); _chk_vec(rounds, "rounds", torch.int32, (F,))
    lib = L.load()
    if coef is None:
        coef = torch.empty(F, n_mcu, bpm, 64, dtype=torch.int16, device=data.device)
    else:
        _chk_vec(coef, "coef", torch.int16, (F, n_mcu, bpm, 64))
    ws = torch.empty(max(lib.tg_jpeg_sync_ws_bytes(F, H, W, JPEG_SUBSAMPLINGS[subsampling], int(restart_interval)), 4), dtype=torch.uint8, device=data.device)
    L.check(_launch("jpeg_decode_coeffs_sync", lib.tg_jpeg_decode_coeffs_sync, _p(data), data.numel(), _p(seg_begin), _p(seg_end), F, H, W,
                    JPEG_SUBSAMPLINGS[subsampling], int(restart_interval), _p(htabs), htabs.shape[0], _p(htab_index), int(sub_bytes), _p(ws), ws.numel(), _p(coef),
                    _p(clean), _p(rounds), _stream()), "tg_jpeg_decode_coeffs_sync")
    return coef


def jpeg_idct_rgb(coef, H, W, subsampling, qtabs, qtab_index, out=None):
    """tg_jpeg_idct_rgb: coef int16 [F, MCUs, blocks per MCU, 64], qtabs uint16 [sets, 3, 64] (natural order), qtab_index int32 [F] -> uint8 [F, H, W, 3].  `out`: a
    flat uint8 buffer to fill instead (every store is checked against its end)."""
    F, _ = _chk_jpeg_coef(coef, H, W, subsampling, 1, "jpeg_idct_rgb")
    _chk(qtabs, "qtabs", torch.uint16)
    if qtabs.dim() != 3 or qtabs.shape[0] < 1 or tuple(qtabs.shape[1:]) != (3, 64) or not qtabs.is_contiguous():
        raise ValueError(f"jpeg_idct_rgb: qtabs must be contiguous uint16 [sets, 3, 64], got {tuple(qtabs.shape)}")
    _chk_vec(qtab_index, "qtab_index", torch.int32, (F,))
    lib = L.load()
    ws = torch.empty(lib.tg_jpeg_idct_ws_bytes(F, H, W, JPEG_SUBSAMPLINGS[subsampling]), dtype=torch.uint8, device=coef.device)
    if out is None:
        out = torch.empty(F, H, W, 3, dtype=torch.uint8, device=coef.device)
    else:
        _chk(out, "out", torch.uint8)
        if out.dim() != 1 or out.numel() < 1:
            raise ValueError(f"jpeg_idct_rgb: out must be a flat uint8 buffer, got {tuple(out.shape)}")
    L.check(_launch("jpeg_idct_rgb", lib.tg_jpeg_idct_rgb, _p(coef), F, H, W, JPEG_SUBSAMPLINGS[subsampling], _p(qtabs), qtabs.shape[0], _p(qtab_index), _p(ws),
                    ws.numel(), _p(out), out.numel(), _stream()), "tg_jpeg_idct_rgb")
    return out


PNG_FILTERS = {"none": 0, "sub": 1, "up": 2, "average": 3, "paeth": 4, "adaptive": 5}


def png_geometry(H, W, rows_per_block=0):
    """tg_png_geometry: (rows of a band, bands of a frame, bytes of a filtered row, bytes of a frame in the filtered workspace, bytes of a plan record, an upper bound of
    a file's bytes, the bytes in front of the first and behind the last IDAT chunk); rows_per_block 0 is the default; refused arguments raise."""
    lib = L.load()
    g = tuple(lib.tg_png_geometry(H, W, rows_per_block, what) for what in range(8))
    if not all(g):
        raise ValueError(f"png: a frame of {H} (1..65535) x {W} (1..21844) with bands of rows_per_block {rows_per_block!r} rows, each at most 65535 bytes")
    return g


def png_filter(frames, filter, rows_per_block=0):
    """tg_png_filter: contiguous uint8 [F, H, W, 3] -> uint8 [F, workspace bytes of a frame]: every row's filter type and filtered bytes, a band's rows together and
    every band at a multiple of 16 bytes (the header's definition)."""
    (_, F, H, W), _ = _chk_rgb(frames, "png_filter", contiguous=True)
    if filter not in PNG_FILTERS:
        raise ValueError(f"png_filter: filter must be one of {tuple(PNG_FILTERS)}, got {filter!r}")
    ws = png_geometry(H, W, rows_per_block)[3]
    out = torch.empty(F, ws, dtype=torch.uint8, device=frames.device)
    L.check(_launch("png_filter", L.load().tg_png_filter, _p(frames), F, H, W, PNG_FILTERS[filter], int(rows_per_block), _p(out), _stream()), "tg_png_filter")
    return out


def _chk_png_filtered(filtered, H, W, rows_per_block, who):
    _chk(filtered, "filtered", torch.uint8)
    g = png_geometry(H, W, rows_per_block)
    if filtered.dim() != 2 or filtered.shape[1] != g[3] or filtered.shape[0] < 1 or not filtered.is_contiguous():
        raise ValueError(f"{who}: filtered must be contiguous [F, {g[3]}], got {tuple(filtered.shape)}")
    return filtered.shape[0], g


def png_band_plan(filtered, H, W, rows_per_block=0):
    """tg_png_band_plan: -> (plans uint8 [F, bands, record bytes], band_bytes int32 [F, bands]: every band's IDAT chunk with its framing)."""
    F, g = _chk_png_filtered(filtered, H, W, rows_per_block, "png_band_plan")
    plans = torch.empty(F, g[1], g[4], dtype=torch.uint8, device=filtered.device)
    band_bytes = torch.empty(F, g[1], dtype=torch.int32, device=filtered.device)
    L.check(_launch("png_band_plan", L.load().tg_png_band_plan, _p(filtered), F, H, W, int(rows_per_block), _p(plans), _p(band_bytes), _stream()), "tg_png_band_plan")
    return plans, band_bytes


def png_write(filtered, plans, H, W, rows_per_block, band_offsets, data):
    """tg_png_write: every frame's file into `data` (uint8 [n]); band_offsets int64 [F, bands]: where every band's IDAT chunk starts."""
    F, g = _chk_png_filtered(filtered, H, W, rows_per_block, "png_write")
    _chk_vec(plans, "plans", torch.uint8, (F, g[1], g[4])); _chk_vec(band_offsets, "band_offsets", torch.int64, (F, g[1])); _chk(data, "data", torch.uint8)
    if data.dim() != 1:
        raise ValueError(f"png_write: data must be uint8 [n], got {tuple(data.shape)}")
    L.check(_launch("png_write", L.load().tg_png_write, _p(filtered), _p(plans), F, H, W, int(rows_per_block), _p(band_offsets), _p(data), data.numel(), _stream()),
            "tg_png_write")
    return data


# the bits of the PNG decoder's status (the list of include/tokensgen_hip.h) and what each says
PNG_STATUS = {1: "a block of type 3, or a stored block whose LEN is not ~NLEN", 2: "code lengths that are no prefix code", 4: "an invalid symbol",
              8: "a distance that reaches before the start of the output", 16: "the zlib stream ends inside a block",
              32: "the stream does not decode to exactly the frame's bytes, or does not end where the last IDAT ends", 64: "the Adler-32 does not match",
              128: "a filter type above 4", 256: "a piece of the stream is not independent", 512: "a byte range or index outside its buffer"}
PNG_INFLATE_MODES = {"stream": 0, "chunk_size": 1, "chunk_write": 2}


def png_decode_geometry(H, W, bpp):
    """tg_png_decode_geometry: (bytes of a filtered row, of a frame's filtered bytes, lanes per piece, bytes of the output ring); refused arguments raise."""
    lib = L.load()
    g = tuple(lib.tg_png_decode_geometry(H, W, bpp, what) for what in range(4))
    if not all(g):
        raise ValueError(f"png: a frame of {H} x {W} pixels of {bpp} bytes (3 or 4) whose filtered bytes, H (1 + bpp W), and 3 H W stay below 2^31")
    return g


def png_inflate(data, pieces, mode, filtered, H, W, bpp, status, piece_at=None):
    """tg_png_inflate: data uint8 [n]; pieces = (begin int64 [P], end int64 [P], frame int32 [P], last int32 [P]); filtered uint8 [F, frame bytes]; status int32 [F].
    mode "chunk_size" returns piece_bytes int32 [P]; "stream" and "chunk_write" (with piece_at int64 [P]) return adler3 uint32-as-int32 [P, 3]."""
    begin, end, frame, last = pieces
    P, F = begin.numel(), status.numel()
    _chk(data, "data", torch.uint8); _chk_vec(begin, "piece_begin", torch.int64, (P,)); _chk_vec(end, "piece_end", torch.int64, (P,))
    _chk_vec(frame, "piece_frame", torch.int32, (P,)); _chk_vec(last, "piece_last", torch.int32, (P,)); _chk_vec(status, "status", torch.int32, (F,))
    _chk_vec(filtered, "filtered", torch.uint8, (F, png_decode_geometry(H, W, bpp)[1]))
    if mode not in PNG_INFLATE_MODES or data.dim() != 1 or not data.is_contiguous():
        raise ValueError(f"png_inflate: mode is one of {tuple(PNG_INFLATE_MODES)} and data contiguous uint8 [n], got {mode!r}, {tuple(data.shape)}")
    sizes = adler3 = None
    if mode == "chunk_size":
        sizes = torch.empty(P, dtype=torch.int32, device=data.device)
    else:
        adler3 = torch.empty(P, 3, dtype=torch.int32, device=data.device)
    if mode == "chunk_write":
        _chk_vec(piece_at, "piece_at", torch.int64, (P,))
    L.check(_launch("png_inflate", L.load().tg_png_inflate, _p(data), data.numel(), _p(begin), _p(end), _p(frame), _p(last), P, PNG_INFLATE_MODES[mode],
                    _p(piece_at) if mode == "chunk_write" else None, _p(filtered), F, H, W, bpp, _p(sizes) if sizes is not None else None,
                    _p(adler3) if adler3 is not None else None, _p(status), _stream()), "tg_png_inflate")
    return sizes if mode == "chunk_size" else adler3


def png_unfilter(filtered, H, W, bpp, frame_first, adler3, expect, status):
    """tg_png_unfilter: filtered uint8 [F, frame bytes] -> uint8 [F, H, W, 3]; frame_first int32 [F + 1], adler3 int32 [P, 3], expect int32 [F] (the bits of the
    streams' Adler-32), status int32 [F]."""
    F = status.numel()
    _chk_vec(filtered, "filtered", torch.uint8, (F, png_decode_geometry(H, W, bpp)[1])); _chk_vec(frame_first, "frame_first", torch.int32, (F + 1,))
    _chk_vec(expect, "expect", torch.int32, (F,)); _chk_vec(status, "status", torch.int32, (F,)); _chk(adler3, "adler3", torch.int32)
    out = torch.empty(F, H, W, 3, dtype=torch.uint8, device=filtered.device)
    L.check(_launch("png_unfilter", L.load().tg_png_unfilter, _p(filtered), F, H, W, bpp, _p(frame_first), _p(adler3), _p(expect), _p(status), _p(out), _stream()),
            "tg_png_unfilter")
    return out
