"""GPU: tg_gemm_bf16_lora — C = bf16(A W^T + bias + s (T B^T)) in one launch — PER ELEMENT against float64 of
bf16(x) bf16(W)^T + b + s bf16(T) bf16(B)^T computed by torch on the CPU.

Bound (edge_bounds.gemm_bias_bound, the construction of the plain bf16-output GEMM, over all K + R products): one bf16 rounding of the result,
2^-8 |ref|, plus the fp32 accumulation term (K + R) 2^-23 (|A||W|^T + |bias| + |s| |T||B|^T).  The one extra operation of the kernel — the fp32
multiplication of the tail sum by s, 2^-24 |s T B^T| — lives inside the factor 2 that term carries over (K + R) 2^-24.  No fitted constant; every
element is checked; the padding around the strided output is sentinel-filled and checked untouched.

Shapes: the smallest that reach every path of the kernel — one full and one ragged last m-tile (M = 1024, 1100), one and three n-tiles (N = 256, 768),
the fewest k-stages the 4-wave kernel takes and one more (K = 256, 320), one / two / the most tail stages (R = 64, 128, 384), batch 2 with padded row and
batch strides, s = 0.5 (exact in bf16), 0.3 (not) and 0; a tail-only case (A = W = 0); and one launch with more tiles than the device has compute units,
where the stage stream crosses from one tile's main loop into the next tile's tail."""
import ctypes
import os
import re

import pytest
import torch

import edge_bounds as E

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF).to(DEV)


@pytest.fixture(scope="module")
def K():
    from tokensgen_amd import kernels
    return kernels


def _operands(M, N, Kd, R, B, seed, zero_main=False):
    """Strided views: A [B, M, K] inside [B, M + 5, K + 8], T [B, M, R] inside [B, M + 3, R + 16], W / lora_B with padded rows."""
    a = _rand(B, M + 5, Kd + 8, seed=seed)[:, 2:2 + M, :Kd]
    w = _rand(N, Kd + 8, seed=seed + 1, scale=0.1)[:, :Kd]
    if zero_main:
        a, w = torch.zeros_like(a), torch.zeros_like(w)
    bias = _rand(N, seed=seed + 2)
    t = _rand(B, M + 3, R + 16, seed=seed + 3)[:, 1:1 + M, :R]
    b = _rand(N, R + 8, seed=seed + 4, scale=0.1)[:, :R]
    return a, w, bias, t, b


def _run(K, a, w, bias, t, b, s, M, N, B):
    full = torch.full((B, M + 2, N + 16), 9.0, dtype=BF, device=DEV)
    out = full[:, 1:1 + M, 8:8 + N]
    K.gemm_lora(a, w, bias, t, b, s, out)
    assert (full[:, 0] == 9.0).all() and (full[:, M + 1] == 9.0).all() and (full[:, :, :8] == 9.0).all() and (full[:, :, 8 + N:] == 9.0).all()
    return out


def _check(K, parity, M, N, Kd, R, B, scales, seed, zero_main=False, with_bias=True):
    from tokensgen_amd import lib as L
    a, w, bias, t, b = _operands(M, N, Kd, R, B, seed, zero_main)
    if not with_bias:
        bias = None
    lin, mag = E.gemm_ref(a, w, bias)                       # fp64, computed once per shape and shared by every s
    tail, tmag = E.gemm_ref(t, b)
    for s in scales:
        what = f"gemm_lora M={M} N={N} K={Kd} R={R} B={B} s={s}" + (" tail only" if zero_main else "")
        got = _run(K, a, w, bias, t, b, s, M, N, B)
        ref, m = lin + s * tail, mag + abs(s) * tmag
        ratio, where = E.check(got, ref, E.gemm_bias_bound(ref, m, Kd + R))
        print(f"{what}: worst error / bound = {ratio:.4f} at {where}")
        parity(ratio, 1.0, what)
        if s == 0:                                          # the main K loop on top of cleared accumulators IS the plain GEMM
            plain = torch.empty(B, M, N, dtype=BF, device=DEV)
            K.gemm(a, w, bias, plain, L.EPI_BIAS)
            assert torch.equal(got.view(torch.int16), plain.view(torch.int16)), what + ": not bitwise tg_gemm_bf16(TG_EPI_BIAS)"


@pytest.mark.parametrize("R", [64, 128, 384])
@pytest.mark.parametrize("Kd", [256, 320])
@pytest.mark.parametrize("N", [256, 768])
@pytest.mark.parametrize("M", [1024, 1100])
def test_gemm_lora_per_element(K, parity, M, N, Kd, R):
    _check(K, parity, M, N, Kd, R, 2, (0.5, 0.3, 0.0), seed=7000 + M + 3 * N + 5 * Kd + 7 * R)


@pytest.mark.parametrize("R", [64, 128, 384])
def test_gemm_lora_tail_only(K, parity, R):
    """A = W = 0: every output element is bias + s T B^T, so a tail stage that is skipped, fetched from the wrong operand or scaled twice shows."""
    _check(K, parity, 1100, 768, 320, R, 2, (0.5, 0.3), seed=8100 + R, zero_main=True)
    _check(K, parity, 1024, 256, 256, R, 1, (0.3,), seed=8200 + R, zero_main=True, with_bias=False)


def test_gemm_lora_more_tiles_than_cus(K, parity):
    """33 x 4 x 2 = 264 tiles: on a 256-CU device some workgroups walk two tiles, so the fetch of the second tile's tail stages is issued from
    inside the first tile's last main stages and the operand switch happens twice per workgroup."""
    tiles = 33 * 4 * 2
    assert tiles > torch.cuda.get_device_properties(0).multi_processor_count, "grow this case: it must exceed the CU count"
    _check(K, parity, 8300, 1024, 256, 128, 2, (0.3, 0.0), seed=8300)


def test_gemm_lora_position_detecting(K):
    """T = rows of the identity, A = 0, s = 1: C[m][n] must equal lora_B[n][(5 m + 1) % R] EXACTLY (ragged last tile, three n-tiles)."""
    M, N, Kd, R = 1100, 768, 256, 128
    idx = (5 * torch.arange(M) + 1) % R
    t_full = torch.zeros(M, R, dtype=BF)
    t_full[torch.arange(M), idx] = 1.0
    t = t_full.to(DEV)
    b = _rand(N, R, seed=11)
    out = torch.empty(M, N, dtype=BF, device=DEV)
    K.gemm_lora(torch.zeros(M, Kd, dtype=BF, device=DEV), torch.zeros(N, Kd, dtype=BF, device=DEV), None, t, b, 1.0, out)
    assert torch.equal(out, b[:, idx.to(DEV)].T)


def test_gemm_lora_refuses_other_shapes(K):
    """Outside the contract: TG_ERR_SHAPE (-2) before any launch — the caller then runs the two-launch form."""
    from tokensgen_amd import lib as L
    lib = L.load()
    buf = torch.zeros(1 << 16, dtype=BF, device=DEV)
    p = buf.data_ptr()

    def call(M, N, Kd, R, ld=None):
        ld = ld or max(Kd, R, N)
        return lib.tg_gemm_bf16_lora(p, ld, 0, p, ld, None, p, ld, 0, p, ld, 0.5, p, ld, 0, M, N, Kd, R, 1, None)
    for M, N, Kd, R in ((1023, 256, 256, 64), (1024, 128, 256, 64), (1024, 384, 256, 64), (1024, 256, 192, 64), (1024, 256, 288, 64),
                        (1024, 256, 256, 32), (1024, 256, 256, 96), (1024, 256, 256, 448), (1024, 256, 256, 0)):
        assert call(M, N, Kd, R) == -2, (M, N, Kd, R)
        assert b"tg_gemm_bf16_lora" in lib.tg_last_error_string()
        assert not K.gemm_lora_supported(M, N, Kd, R)
    assert call(1024, 256, 256, 64, ld=1 << 21) == -2
    assert K.gemm_lora_supported(1024, 256, 256, 64) and K.gemm_lora_supported(28326, 9216, 3072, 128)
    assert lib.tg_gemm_bf16_lora(None, 0, 0, None, 0, None, None, 0, 0, None, 0, 0.0, None, 0, 0, 0, 0, 0, 0, 0, None) == -1


def test_every_export_still_matches_the_header():
    """The new export is declared, bound and exported; every prototype of the binding has as many arguments as the header's declaration."""
    from tokensgen_amd import lib as L
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tokensgen_hip.h")).read(), flags=re.S)
    so = ctypes.CDLL(L.LIB_PATH)
    assert "tg_gemm_bf16_lora" in L.PROTOTYPES and hasattr(so, "tg_gemm_bf16_lora")
    for name, argtypes in L.PROTOTYPES.items():
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
        assert m is not None, f"{name}: not declared in the header"
        assert len(m.group(1).split(",")) == len(argtypes), f"{name}: the header declares {len(m.group(1).split(','))} arguments, the binding {len(argtypes)}"
    declared = set(re.findall(r"\b(tg_[a-z0-9_]+)\s*\(", hdr))
    assert set(L.PROTOTYPES) | set(L.QUERIES) | set(L.OTHER_EXPORTS) == declared
