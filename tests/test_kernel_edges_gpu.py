"""GPU: the DiT inference kernels PER ELEMENT against fp64 at the dispatch edges the rest of the suite never visits, and the header's
stream contract.

Every numeric check goes through edge_bounds.check (all elements, bound derived from the documented arithmetic: tests/edge_bounds.py)
and is recorded as parity(worst error/bound, 1.0, what).  Inputs come from seeded CPU generators; A, C, x and y are strided views and
the padding around every output is sentinel-filled and checked untouched."""
import numpy as np
import pytest
import torch

import edge_bounds as E

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF).to(DEV)


@pytest.fixture(scope="module")
def K():
    from tokensgen_amd import kernels
    return kernels


def _table(K, B, rows, D, ngroups, tokens, seed):
    """A modulation table with `ngroups` token groups: (GroupTable, [B, tokens, D] shift, scale, gate rows as the kernels must gather them)."""
    mod = _rand(B, rows, 3 * D * ngroups, seed=seed, scale=0.5)
    g = torch.Generator().manual_seed(seed + 1)
    tok_group = torch.randint(0, ngroups, (tokens,), generator=g, dtype=torch.uint8)
    r = [int(x) for x in torch.randint(0, rows, (ngroups,), generator=g)]
    cols = [[3 * D * i + part * D for i in range(ngroups)] for part in range(3)]
    tab = K.GroupTable(mod, tok_group.to(DEV), r, *cols)
    tg = tok_group.long()
    rr = torch.tensor(r)[tg]
    gathered = []
    for c in cols:
        idx = torch.tensor(c)[tg][:, None] + torch.arange(D)[None]
        gathered.append(mod.cpu()[:, rr[:, None], idx])
    return (tab, *gathered)


# ---------------------------------------------------------------- GEMM --------------------------------------------------------------------
_NK = [(128, 64), (384, 128), (256, 128), (256, 192), (256, 256), (512, 320)]


def _gemm_cases():
    """Every kernel x every M edge (gemm.hip `launch`): the 128 x 128 kernel (M < 1024, or N % 256 != 0 at any M) at M = 1, 2 and +-1 around
    its 128- / 256-row edges and at 1023; the 8-wave 256 x 256 kernel (M >= 1024, N % 256 == 0, K < 256) with K = 64, 128, 192 — fewer,
    exactly as many and barely more K stages than its 4 ring slots — and the 4-wave 256 x 256 kernel (K >= 256), each at 1024, 1025 and
    +-1 around the 1280-row tile edge.  (N, K) and the batch size (1 or 3) of a row are drawn from a seeded generator."""
    rng = np.random.RandomState(17)
    cases = []
    for M in (1, 2, 127, 128, 129, 255, 256, 257, 1023):
        for j in rng.choice(len(_NK), 2, replace=False):
            cases.append((M, *_NK[j], int(rng.choice([1, 3]))))
    for M in (1024, 1025, 1279, 1281):
        cases.append((M, *_NK[int(rng.choice([0, 1]))], int(rng.choice([1, 3]))))            # N % 256 != 0: still the 128 x 128 kernel
        for nk in ((256, 64), (256, 128), (256, 192), (256, 256), (512, 320)):               # 8-wave K = 64 / 128 / 192, 4-wave K = 256 / 320
            cases.append((M, *nk, int(rng.choice([1, 3]))))
    return cases


@pytest.mark.parametrize("M,N,Kd,B", _gemm_cases())
def test_gemm_edges_per_element(K, parity, M, N, Kd, B):
    """All four inference epilogues of one shape, per element against fp64.  GELU / SiLU are defined on bf16(A W^T + bias): their reference is
    act64 of the bits the EPI_BIAS launch of the same shape returned, which are themselves checked first."""
    from tokensgen_amd import lib as L
    seed = 1000 + M * 7 + N + Kd + B
    a = _rand(B, M + 5, Kd + 8, seed=seed)[:, 2:2 + M, :Kd]                  # row stride K + 8, batch stride (M + 5)(K + 8)
    w, bias = _rand(N, Kd, seed=seed + 1, scale=0.1), _rand(N, seed=seed + 2)
    res = _rand(B, M + 1, N + 8, seed=seed + 3)[:, 1:, :N]
    tab, _, _, gate = _table(K, B, 7, N, 5, M, seed=seed + 4)
    lin, mag = E.gemm_ref(a, w, bias)
    what = f"gemm M={M} N={N} K={Kd} B={B}"

    def run(epi, **kw):
        full = torch.full((B, M + 2, N + 16), 9.0, dtype=BF, device=DEV)
        out = full[:, 1:1 + M, 8:8 + N]
        K.gemm(a, w, bias, out, epi, **kw)
        assert (full[:, 0] == 9.0).all() and (full[:, M + 1] == 9.0).all() and (full[:, :, :8] == 9.0).all() and (full[:, :, 8 + N:] == 9.0).all(), what
        return out.cpu()

    pre = run(L.EPI_BIAS)
    parity(E.check(pre, lin, E.gemm_bias_bound(lin, mag, Kd))[0], 1.0, what + " bias")
    for act, epi in (("gelu", L.EPI_BIAS_GELU), ("silu", L.EPI_BIAS_SILU)):
        ref, bound = E.gemm_act(pre, act)
        parity(E.check(run(epi), ref, bound)[0], 1.0, f"{what} {act}")
    ref, bound = E.gemm_gate_res(lin, mag, res, gate, Kd, rounded_linear=M >= 1024 and N % 256 == 0)
    parity(E.check(run(L.EPI_BIAS_GATE_RES, residual=res, gate=tab), ref, bound)[0], 1.0, what + " gate_res")


@pytest.mark.parametrize("M,N,Kd", [(129, 128, 128), (1025, 256, 128), (1025, 256, 256)])     # 128 x 128 / 8-wave / 4-wave kernel, ragged last m-tile
def test_gemm_position_detecting_ragged(K, M, N, Kd):
    """A = rows of the identity (row m selects column (7 m + 3) % K of W^T): C[m][n] must equal W[n][(7 m + 3) % K] EXACTLY — a fragment
    written to the wrong lane or row of a ragged tile edge shows as a wrong element, not as noise."""
    from tokensgen_amd import lib as L
    idx = (7 * torch.arange(M) + 3) % Kd
    a_full = torch.zeros(M + 3, Kd + 8, dtype=BF)
    a_full[1 + torch.arange(M), idx] = 1.0
    a = a_full.to(DEV)[1:1 + M, :Kd]
    w = _rand(N, Kd, seed=5)
    full = torch.full((M + 2, N + 8), 9.0, dtype=BF, device=DEV)
    out = full[1:1 + M, :N]
    K.gemm(a, w, None, out, L.EPI_BIAS)
    assert torch.equal(out, w[:, idx.to(DEV)].T)
    assert (full[0] == 9.0).all() and (full[M + 1] == 9.0).all() and (full[:, N:] == 9.0).all()


# ------------------------------------------------------------ tg_adaln_modulate ------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 7])
@pytest.mark.parametrize("D", [8, 72, 512, 520, 8192])     # one masked vector per row / a partly filled first chunk / each side of a CHUNKS template edge / the largest dim
def test_adaln_modulate_edges_per_element(K, parity, D, T):
    B = 2
    x = _rand(B, T + 3, D + 8, seed=D + T, scale=2.0)[:, 1:1 + T, :D]
    w, b = _rand(D, seed=2, scale=0.1) + 1, _rand(D, seed=3, scale=0.1)
    tab, shift, scale, _ = _table(K, B, 13, D, 4, T, seed=5)
    for table, sc, sh in ((tab, scale, shift), (None, None, None)):
        full = torch.full((B, T + 2, D + 16), 9.0, dtype=BF, device=DEV)
        out = full[:, 1:1 + T, 8:8 + D]
        K.adaln_modulate(x, out, w, b, 1e-5, table)
        ref, bound = E.adaln_ref(x, w, b, 1e-5, sc, sh)
        parity(E.check(out, ref, bound)[0], 1.0, f"adaln_modulate D={D} T={T} {'modulated' if table is not None else 'plain'}")
        assert (full[:, 0] == 9.0).all() and (full[:, T + 1] == 9.0).all() and (full[:, :, :8] == 9.0).all() and (full[:, :, 8 + D:] == 9.0).all()


# ------------------------------------------------------------- stream contract -------------------------------------------------------------
def _eager_then_captured(run):
    """run() launches on the CURRENT stream and returns its output tensors.  Once eagerly on the default stream, once captured into a graph on
    a side stream (one linear chain) and replayed once: bitwise the same.  A call that touched the null stream or synchronised would fail the
    capture with a HIP error."""
    eager = [t.clone() for t in run()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
        outs = run()
    graph.replay()
    torch.cuda.synchronize()
    assert len(eager) == len(outs)
    for i, (a, b) in enumerate(zip(eager, outs)):
        assert torch.isfinite(a.float()).all() and torch.equal(a, b), f"output {i}: captured replay differs from the eager launch"


def test_stream_capture_qk_layernorm_rope_pair_kmax(K):
    from oracle import dit_ref as O
    B, T, H = 2, 50, 3
    buf = _rand(B, T, 3 * H * 64, seed=1)
    wq, bq, wk, bk = _rand(64, seed=2, scale=0.1) + 1, _rand(64, seed=3, scale=0.1), _rand(64, seed=4, scale=0.1) + 1, _rand(64, seed=5, scale=0.1)
    f32 = np.float32
    c0 = tuple(t.to(DEV).contiguous() for t in O.rope_3d(64, np.arange(2, dtype=f32), np.arange(3, dtype=f32), np.arange(4, dtype=f32)))
    kws = K.kmax_workspace(T, H, B, DEV)

    def run():
        c = buf.clone()
        km = torch.zeros(B, H, dtype=torch.float32, device=DEV)
        K.qk_layernorm_rope_pair(c[:, :, :H * 64], c[:, :, H * 64:2 * H * 64], H, wq, bq, wk, bk, 1e-6, (8, c0), k_scale=0.18033688, kmax=km, kmax_ws=kws)
        return c, km
    _eager_then_captured(run)


def test_stream_capture_attention_multi_with_rider(K):
    B, H, N1, NP = 2, 2, 200, 70
    D, N = H * 64, N1 + NP
    qkv, qkvv = _rand(B, N1, 3 * D, seed=1, scale=0.5), _rand(B, N, 3 * D, seed=2, scale=0.5)
    pad = lambda n: (n + 63) // 64 * 64
    vt1 = torch.zeros(B, H, 64, pad(N1), dtype=BF, device=DEV); K.transpose_v(qkv[:, :, 2 * D:], H, 0, N1, vt1)
    vt2 = torch.zeros(B, H, 64, pad(NP), dtype=BF, device=DEV); K.transpose_v(qkvv[:, :, 2 * D:], H, N1, NP, vt2)
    vt3 = torch.zeros(B, H, 64, pad(N), dtype=BF, device=DEV); K.transpose_v(qkvv[:, :, 2 * D:], H, 0, N, vt3)

    def run():
        o = torch.zeros(B, N, D, dtype=BF, device=DEV)
        K.attention_multi(dict(q1=qkv[:, :, :D], k1=qkv[:, :, D:2 * D], vt1=vt1, nk1=N1, out=o[:, :N1], q2=qkvv[:, :N1, :D], k2=qkvv[:, N1:, D:2 * D],
                               vt2=vt2, nk2=NP, seg2_scale=0.6, seg2_scale_batch=[0.6015625, 0.25]),
                          dict(q1=qkvv[:, N1:, :D], k1=qkvv[:, :, D:2 * D], vt1=vt3, nk1=N, out=o[:, N1:]), H, 0.125)
        return (o,)
    _eager_then_captured(run)


def test_stream_capture_attention_bwd_two_launches(K):
    B, H, nq, nk = 2, 2, 200, 130                         # fewer than 4 query tiles per key block: the statistics + dK/dV + dQ launches
    q, k, v, dout = (_rand(B, n, H * 64, seed=s, scale=0.5) for n, s in ((nq, 1), (nk, 2), (nk, 3), (nq, 4)))
    vt = torch.zeros(B, H, 64, 192, dtype=BF, device=DEV); K.transpose_v(v, H, 0, nk, vt)
    o = torch.empty(B, nq, H * 64, dtype=BF, device=DEV)
    K.attention(q, k, vt, nk, o, H, 0.125)
    _eager_then_captured(lambda: K.attention_bwd(q, k, v, o, dout, H, 0.125))


def test_stream_capture_lora_wgrad(K):
    B, M, N, R = 2, 300, 128, 64
    y, t = _rand(B, M, N, seed=1), _rand(B, M, R, seed=2)

    def run():
        out = torch.zeros(N, R, dtype=torch.float32, device=DEV)
        K.lora_wgrad(y, t, out, scale=0.5)
        return (out,)
    _eager_then_captured(run)


def test_stream_capture_gemm_4wave(K):
    from tokensgen_amd import lib as L
    a, w, bias = _rand(1024, 256, seed=1), _rand(256, 256, seed=2, scale=0.1), _rand(256, seed=3)

    def run():
        out = torch.zeros(1024, 256, dtype=BF, device=DEV)
        K.gemm(a, w, bias, out, L.EPI_BIAS_GELU)
        return (out,)
    _eager_then_captured(run)
