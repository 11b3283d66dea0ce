"""GPU: the training backward and loss kernels PER ELEMENT against fp64 (tests/train_bounds.py: bounds derived from the documented arithmetic, no measured figure) at the
dispatch edges the norm-based tests of test_train_gpu.py never visit: both forms of tg_attention_bwd* around the one-kernel threshold, both workgroup-to-head mappings,
every key-split count of the dQ launch, the scalar / NC = 6 / 8 / 0 forms of tg_adaln_modulate_bwd, the 512-row blocks of tg_qk_layernorm_rope_bwd, the vector and scalar
forms of the elementwise and column-sum kernels and the 256-element blocks of the loss kernels.

Every numeric check goes through train_bounds.check (ALL elements) and is recorded as parity(worst error / bound, 1.0, "kernel shape output").  Inputs come from seeded CPU
generators; attention inputs are column slices of a fused QKV buffer; outputs are strided views of larger buffers whose frame is sentinel-filled and checked untouched, and
whose inside is NaN-filled wherever the kernel must overwrite (finite outputs prove it never read them)."""
import functools
import os
from types import SimpleNamespace as NS

import pytest
import torch

import train_bounds as T

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
FUSED_OFF = os.environ.get("TG_ATTN_BWD_FUSED") == "0"


def _randn(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _rand(*shape, seed, scale=1.0):
    return _randn(*shape, seed=seed, scale=scale).to(BF)


@pytest.fixture(scope="module")
def K():
    from tokensgen_amd import kernels
    return kernels


@pytest.fixture(scope="module")
def lib():
    from tokensgen_amd import lib as L
    return NS(L=L, so=L.load())


@pytest.fixture(autouse=True)
def _nothing_runs_after_a_gpu_fault():
    """A failed assertion lets the next test run; a GPU fault (the runtime reports it at the next synchronisation) ends the session: nothing more is launched on that device."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU fault, stopping the run: {e}", returncode=3)


def _framed(B, n, D, dtype, inside, sentinel=9.0):
    """([B, n + 2, D + 16] buffer filled with the sentinel, its [B, n, D] view at row 1, column 8 filled with `inside` (a float or a [B, n, D] tensor))."""
    full = torch.full((B, n + 2, D + 16), sentinel, dtype=dtype, device=DEV)
    view = full[:, 1:1 + n, 8:8 + D]
    view.copy_(inside.to(DEV)) if isinstance(inside, torch.Tensor) else view.fill_(inside)
    return full, view


def _frame_untouched(full, n, D, sentinel=9.0):
    return bool((full[:, 0] == sentinel).all() and (full[:, n + 1] == sentinel).all() and (full[:, :, :8] == sentinel).all() and (full[:, :, 8 + D:] == sentinel).all())


def _flat_framed(numel, dtype, inside=NAN, sentinel=9.0, pad=32):
    """A contiguous `numel` view inside a flat sentinel-padded buffer (pad elements each side: the view stays 16-byte aligned)."""
    full = torch.full((numel + 2 * pad,), sentinel, dtype=dtype, device=DEV)
    full[pad:pad + numel] = inside
    return full, full[pad:pad + numel]


def _flat_untouched(full, numel, sentinel=9.0, pad=32):
    return bool((full[:pad] == sentinel).all() and (full[pad + numel:] == sentinel).all())


# ------------------------------------------------------------ attention backward -----------------------------------------------------------
TWO_LAUNCH = [(1, 1, 1, 1), (1, 1, 1, 257), (1, 3, 31, 1), (1, 2, 33, 255), (2, 3, 257, 256), (1, 5, 255, 257), (1, 1, 64, 33),      # (H B) % 8 != 0: smallest and ragged tiles
              (1, 8, 96, 256), (2, 4, 224, 512)]                                                                                      # (H B) % 8 == 0 without the chain: 3 < 4, 7 < 8 tiles
ONE_KERNEL = [(1, 8, 128, 256), (2, 4, 256, 512), (1, 8, 257, 257), (1, 16, 130, 31)]     # at the threshold; 9 tiles, second key block of ONE key; H B = 16
KEY_SPLIT = [(1, 2, 40, 992), (1, 2, 40, 993), (1, 2, 40, 1536), (1, 2, 33, 4065), (1, 2, 33, 4100), (2, 3, 257, 2050)]     # kparts 1, 2, 3, 8, 8 (129 tiles: uneven), batch / head strides
SCALE = 0.125


def _is_one_kernel(B, H, nq, nk):
    """The documented dispatch condition (tg_attention_bwd_ex): >= 4 query tiles per key block and a multiple of 8 (batch, head) pairs."""
    return (nq + 31) // 32 >= 4 * ((nk + 255) // 256) and (H * B) % 8 == 0


def _kparts(B, H, nq, nk, cus=256):
    """The dQ launch's key ranges as the library documents them: min(8, 6 CUs / workgroups, key tiles / 16), below 2 -> 1 (at the shapes used here the CU term never binds
    on a device with more than 16 CUs).  _run reads the split a launch really took back from the workspace and holds it to this."""
    wgs = (nq + 255) // 256 * H * B
    kp = min(8, 6 * cus // wgs, ((nk + 31) // 32) // 16) if wgs <= 256 else 1
    return kp if kp >= 2 else 1


def test_the_shape_lists_sit_where_the_dispatch_changes():
    assert all(not _is_one_kernel(*s) for s in TWO_LAUNCH + KEY_SPLIT) and all(_is_one_kernel(*s) for s in ONE_KERNEL)
    assert [(B * H) % 8 == 0 for B, H, _, _ in TWO_LAUNCH] == [False] * 7 + [True] * 2
    assert [_kparts(*s) for s in KEY_SPLIT] == [1, 2, 3, 8, 8, 4]
    assert (4100 + 31) // 32 == 129 and all(B * H * nq * nk <= 4.1e6 for B, H, nq, nk in TWO_LAUNCH + ONE_KERNEL + KEY_SPLIT)


def _case(q, k, v, o, g, H, scale=SCALE):
    """CPU bf16 tensors -> the device views the kernel gets (q | k | v as column slices of ONE fused buffer) + the fp64 reference."""
    B, nq, D = q.shape
    nk = k.shape[1]
    fused = torch.zeros(B, max(nq, nk), 3 * D, dtype=BF)
    fused[:, :nq, :D], fused[:, :nk, D:2 * D], fused[:, :nk, 2 * D:] = q, k, v
    fd = fused.to(DEV)
    return NS(B=B, H=H, nq=nq, nk=nk, D=D, scale=scale, cpu=(q, k, v, o, g), q=fd[:, :nq, :D], k=fd[:, :nk, D:2 * D], v=fd[:, :nk, 2 * D:], o=o.to(DEV), g=g.to(DEV),
              ref=T.attention_bwd_ref(q, k, v, o, g, H, scale), what=f"attention_bwd B={B} H={H} nq={nq} nk={nk}")


def _forward_o(q, k, v, H, scale=SCALE):
    qh, kh, vh = (T._heads(t, H) for t in (q, k, v))
    return T._merge(torch.softmax(qh @ kh.transpose(-1, -2) * scale, -1) @ vh).to(BF)


@functools.lru_cache(maxsize=None)
def _random_case(B, H, nq, nk, peaked=False):
    """One shared reference per shape: the tests below only read it."""
    D, seed = H * 64, 1000 * nq + nk + 7 * H + B
    s = 3.0 if peaked else 1.2                           # peaked: q, k ~ 3 randn, |lse| in the tens
    q, k, v, g = _rand(B, nq, D, seed=seed, scale=s), _rand(B, nk, D, seed=seed + 1, scale=s), _rand(B, nk, D, seed=seed + 2), _rand(B, nq, D, seed=seed + 3)
    c = _case(q, k, v, _forward_o(q, k, v, H), g, H)
    c.what += " peaked" if peaked else ""
    return c


WS_SENTINEL = 0x7FC12345          # a NaN bit pattern: no kernel computes it


def _expected_form(B, H, nq, nk):
    return ("one_kernel", 0) if _is_one_kernel(B, H, nq, nk) and not FUSED_OFF else ("two_launch", _kparts(B, H, nq, nk))


def _launch_and_read_back_the_form(K, c, **kw):
    """tg_attention_bwd_multi with one problem, as kernels.attention_bwd launches it, on a workspace pre-filled with a sentinel: which words behind the row statistics
    (6 floats per (batch, head, query) + 8) the call changed tells which form ran.  The one-kernel form clears and then uses its exchange counters (32 per (batch, head,
    query tile)) and per-head XCD masks; the two launches leave them alone, and a dQ launch cut into kparts key ranges writes kparts partial dQ tensors behind them."""
    from tokensgen_amd import lib as L
    pr, _, (ws, B) = K._bwd_problem(c.q, c.k, c.v, c.o, c.g, c.H, c.scale, **kw)
    wi = ws.view(torch.int32)
    wi.fill_(WS_SENTINEL)
    st = K.BwdDeviceState.get(DEV)
    L.check(L.load().tg_attention_bwd_multi((L.AttnBwdProblem * 1)(pr), 1, c.H, B, st.flags(), K._p(st.status), K._stream()), "tg_attention_bwd_multi")
    torch.cuda.synchronize()
    changed = int((wi[6 * B * c.H * c.nq + 8:] != WS_SENTINEL).sum())
    counters = B * c.H * ((c.nq + 31) // 32) * 32 + B * c.H
    if changed == counters:
        return ("one_kernel", 0)
    assert changed % (B * c.nq * c.D) == 0, f"{c.what}: {changed} workspace words changed: neither the counters ({counters}) nor whole partial dQ tensors"
    return ("two_launch", max(1, changed // (B * c.nq * c.D)))


def _run(K, c, accumulate=0, pre=None, lse=None, dv="f32"):
    """One launch into framed outputs.  accumulate bit 0: dq, bit 1: dk / dv are preloaded with pre[...] (else NaN inside).  dv: "f32", "bf16" (no fp32 dv) or "both".
    Returns {"dq", "dk", "dv", "dv_bf16"} (CPU copies) after checking every frame — and that the call took the form (and the dQ key split) its shape was chosen for."""
    acc = 3 if accumulate in (1, 3) else accumulate
    fill = lambda name, bit: pre[name] if acc & bit else NAN
    fq, dq = _framed(c.B, c.nq, c.D, F32, fill("dq", 1))
    fk, dk = _framed(c.B, c.nk, c.D, F32, fill("dk", 2))
    fv, dvv = _framed(c.B, c.nk, c.D, F32, fill("dv", 2)) if dv != "bf16" else (None, None)
    fb, dvb = _framed(c.B, c.nk, c.D, BF, NAN, sentinel=7.0) if dv != "f32" else (None, None)
    form = _launch_and_read_back_the_form(K, c, dq=dq, dk=dk, dv=dvv, accumulate=accumulate, lse=lse, dv_bf16=dvb)
    assert form == _expected_form(c.B, c.H, c.nq, c.nk), f"{c.what}: ran as {form}"
    assert _frame_untouched(fq, c.nq, c.D) and _frame_untouched(fk, c.nk, c.D), c.what
    assert fv is None or _frame_untouched(fv, c.nk, c.D), c.what
    assert fb is None or _frame_untouched(fb, c.nk, c.D, 7.0), c.what
    return {"dq": dq.cpu(), "dk": dk.cpu(), "dv": None if dvv is None else dvv.cpu(), "dv_bf16": None if dvb is None else dvb.cpu()}


def _hold(parity, c, got, tag="", names=("dq", "dk", "dv")):
    for n in names:
        assert torch.isfinite(got[n]).all(), f"{c.what} {n}{tag}: non-finite output (an overwritten output was read, or a tile was skipped)"
        parity(T.check(got[n], *c.ref[n])[0], 1.0, f"{c.what} {n}{tag}")


def _assert_only(measured, tol, what=""):
    assert measured < tol, f"{what}: measured {measured:.4e} >= tolerance {tol:.1e}"


def _edges(K, parity, shape):
    if _is_one_kernel(*shape) and not FUSED_OFF:
        assert K.BwdDeviceState.get(DEV).one_kernel, "tg_attention_bwd_probe failed on this device: the one-kernel form would never be selected"
    if FUSED_OFF:                 # the cross-check child process shares the parent's test ids: it asserts, the parent's figures are the recorded ones
        parity = _assert_only
    c = _random_case(*shape)
    got = _run(K, c)
    _hold(parity, c, got)
    again = _run(K, c)
    assert all(torch.equal(got[n], again[n]) for n in ("dq", "dk", "dv")), c.what + ": a rerun differs"
    K.attention_bwd_check(DEV)


@pytest.mark.parametrize("shape", TWO_LAUNCH + KEY_SPLIT, ids=lambda s: "-".join(map(str, s)))
def test_attention_bwd_edges_two_launch_shapes(K, parity, shape):
    _edges(K, parity, shape)


@pytest.mark.parametrize("shape", ONE_KERNEL, ids=lambda s: "-".join(map(str, s)))
def test_attention_bwd_edges_one_kernel_shapes(K, parity, shape):
    """(test_train_gpu.py::test_attention_bwd_two_kernel_form_in_a_child_process runs these with TG_ATTN_BWD_FUSED=0 as well: the same shapes through the two launches)"""
    _edges(K, parity, shape)


MODE_SHAPES = [(2, 3, 257, 256), (1, 5, 255, 257), (1, 8, 96, 256), (2, 4, 224, 512), (1, 8, 257, 257), (1, 16, 130, 31), (1, 2, 40, 993), (2, 3, 257, 2050)]     # two per form


@pytest.mark.parametrize("shape", MODE_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_attention_bwd_lse_accumulate_bf16_dv_and_peaked(K, parity, shape):
    c = _random_case(*shape)
    # the forward's own log-sum-exp instead of the statistics pass
    vt = K.transpose_v(c.v, c.H, 0, c.nk, torch.zeros(c.B, c.H, 64, (c.nk + 63) // 64 * 64, dtype=BF, device=DEV))
    _, lse = K.attention_lse(c.q, c.k, vt, c.nk, torch.empty(c.B, c.nq, c.D, dtype=BF, device=DEV), c.H, c.scale)
    parity(T.check(lse, *T.attention_lse_ref(c.cpu[0], c.cpu[1], c.H, c.scale))[0], 1.0, c.what + " lse (tg_attention_fwd_lse)")
    _hold(parity, c, _run(K, c, lse=lse), " lse given")
    # accumulate modes on non-trivial preloaded tensors, per element against preload + ref
    pre = {n: _randn(c.B, c.nq if n == "dq" else c.nk, c.D, seed=11 + i) for i, n in enumerate(("dq", "dk", "dv"))}
    for mode in (1, 2, 3):
        got = _run(K, c, accumulate=mode, pre=pre)                 # mode 2: the dq inside is NaN and must come back finite
        for n in ("dq", "dk", "dv"):
            ref = T.accumulated(*c.ref[n], pre[n]) if (n != "dq" or mode != 2) else c.ref[n]
            assert torch.isfinite(got[n]).all(), f"{c.what} {n} accumulate={mode}"
            parity(T.check(got[n], *ref)[0], 1.0, f"{c.what} {n} accumulate={mode}")
    # bf16 dv from the epilogue, alone and beside the fp32 tensor
    base = _run(K, c)
    alone, both = _run(K, c, dv="bf16"), _run(K, c, dv="both")
    for tag, got in (("alone", alone), ("beside fp32", both)):
        assert torch.isfinite(got["dv_bf16"].float()).all()
        parity(T.check(got["dv_bf16"], *T.as_bf16(*c.ref["dv"]))[0], 1.0, f"{c.what} dv_bf16 {tag}")
        assert torch.equal(got["dv_bf16"], base["dv"].to(BF)) and torch.equal(got["dq"], base["dq"]) and torch.equal(got["dk"], base["dk"])
    assert alone["dv"] is None and torch.equal(both["dv"], base["dv"])
    # peaked softmax
    cp = _random_case(*shape, peaked=True)
    assert float(cp.ref["lse"].abs().max()) > 20.0
    _hold(parity, cp, _run(K, cp))
    K.attention_bwd_check(DEV)


@pytest.mark.parametrize("pair", [((1, 8, 257, 257), (1, 8, 130, 200)), ((1, 8, 257, 257), (1, 8, 96, 256))], ids=["main_plus_rider", "one_kernel_plus_two_launch"])
def test_attention_bwd_multi_two_problems_per_element(K, parity, pair):
    """tg_attention_bwd_multi: each problem held per element (not only equal to two single calls — which it must be too), the second one accumulating into dk / dv."""
    assert _is_one_kernel(*pair[0]) and _is_one_kernel(*pair[1]) == (pair[1][2] == 130)
    c1, c2 = _random_case(*pair[0]), _random_case(*pair[1])
    pre = {n: _randn(c2.B, c2.nk, c2.D, seed=21 + i) for i, n in enumerate(("dk", "dv"))}
    outs = []
    for c, acc in ((c1, 0), (c2, 2)):
        o = {"dq": _framed(c.B, c.nq, c.D, F32, NAN), "dk": _framed(c.B, c.nk, c.D, F32, pre["dk"] if acc else NAN), "dv": _framed(c.B, c.nk, c.D, F32, pre["dv"] if acc else NAN)}
        outs.append(o)
    prob = lambda c, o, acc: dict(q=c.q, k=c.k, v=c.v, o=c.o, dout=c.g, scale=c.scale, dq=o["dq"][1], dk=o["dk"][1], dv=o["dv"][1], accumulate=acc)
    K.attention_bwd_multi([prob(c1, outs[0], 0), prob(c2, outs[1], 2)], 8)
    torch.cuda.synchronize()
    K.attention_bwd_check(DEV)
    for c, o, acc in ((c1, outs[0], 0), (c2, outs[1], 2)):
        for n in ("dq", "dk", "dv"):
            full, view = o[n]
            assert _frame_untouched(full, c.nq if n == "dq" else c.nk, c.D) and torch.isfinite(view).all(), f"{c.what} {n}"
            ref = T.accumulated(*c.ref[n], pre[n]) if acc and n != "dq" else c.ref[n]
            parity(T.check(view, *ref)[0], 1.0, f"multi[{'+'.join(map(str, pair[1]))}] {c.what} {n}")
    single = _run(K, c2, accumulate=2, pre=pre)
    assert all(torch.equal(single[n], outs[1][n][1].cpu()) for n in ("dq", "dk", "dv"))
    first = _run(K, c1)
    assert all(torch.equal(first[n], outs[0][n][1].cpu()) for n in ("dq", "dk", "dv"))


# ---- known answers ----
@pytest.mark.parametrize("B,H,nq", [(1, 3, 31), (2, 4, 130)])
def test_attention_bwd_single_key_known_answer(K, parity, B, H, nq):
    """nk = 1, O := v: P = 1, dV[0] = sum_i dO_i; dQ and dK are exactly 0 in exact arithmetic (dP = D) — the kernel's values must lie within the cancellation terms alone."""
    D = H * 64
    q, k, v, g = _rand(B, nq, D, seed=1), _rand(B, 1, D, seed=2), _rand(B, 1, D, seed=3), _rand(B, nq, D, seed=4)
    c = _case(q, k, v, v.expand(B, nq, D).contiguous(), g, H)
    assert float(c.ref["dq"][0].abs().max()) < 1e-12 and float(c.ref["dk"][0].abs().max()) < 1e-12
    assert torch.allclose(c.ref["dv"][0], T.d(g).sum(1, keepdim=True))
    _hold(parity, c, _run(K, c), " single key, O = v")


@pytest.mark.parametrize("nk", [256, 257])
def test_attention_bwd_zero_queries_give_uniform_p(K, parity, nk):
    """q = 0: P = 1 / nk, so every dV row is sum_i dO_i / nk — all rows identical up to the bound.  A padded key inside the normaliser (nk = 257: 255 of them) shows here."""
    B, H, nq = 1, 2, 70
    D = H * 64
    q, k, v, g = torch.zeros(B, nq, D, dtype=BF), _rand(B, nk, D, seed=5), _rand(B, nk, D, seed=6), _rand(B, nq, D, seed=7)
    c = _case(q, k, v, _forward_o(q, k, v, H), g, H)
    want = T.d(g).sum(1, keepdim=True) / nk
    assert torch.allclose(c.ref["dv"][0], want.expand(B, nk, D), rtol=1e-12, atol=1e-15)
    got = _run(K, c)
    _hold(parity, c, got, " q = 0")
    parity(T.check(got["dv"], want.expand(B, nk, D), c.ref["dv"][1])[0], 1.0, c.what + " q = 0: dv rows against sum dO / nk")


@pytest.mark.parametrize("shape", [(2, 3, 257, 256), (2, 4, 256, 512)], ids=lambda s: "-".join(map(str, s)))
def test_attention_bwd_one_hot_dout_goes_nowhere_else(K, parity, shape):
    """dO = 1 at one (batch b0, row i0, head h0, column d0), O the forward's output (D = O[i0, d0] in that row and head, 0 everywhere else — a D that leaked into another row
    or head would show): dV is EXACTLY 0 outside head h0 / column d0 / batch b0 and dV[:, d0] = P[i0, :]; dQ is exactly 0 outside row i0 / head h0; dK is exactly 0 outside
    head h0 / batch b0."""
    B, H, nq, nk = shape
    D = H * 64
    b0, i0, h0, d0 = B - 1, nq - 2, H - 2, 37
    q, k, v = _rand(B, nq, D, seed=8, scale=1.2), _rand(B, nk, D, seed=9, scale=1.2), _rand(B, nk, D, seed=10)
    g = torch.zeros(B, nq, D, dtype=BF)
    g[b0, i0, h0 * 64 + d0] = 1.0
    c = _case(q, k, v, _forward_o(q, k, v, H), g, H)
    assert float(c.cpu[3][b0, i0, h0 * 64 + d0].abs()) > 0
    got = _run(K, c)
    _hold(parity, c, got, " one-hot dO")
    col = h0 * 64 + d0
    dv = got["dv"].clone()
    parity(T.check(dv[b0, :, col], c.ref["p"][b0, h0, i0], c.ref["dv"][1][b0, :, col])[0], 1.0, c.what + " one-hot dO: dv[:, d0] against P[i0, :]")
    dv[b0, :, col] = 0
    assert not dv.any(), "dV outside (b0, h0, d0)"
    dq = got["dq"].clone()
    dq[b0, i0, h0 * 64:h0 * 64 + 64] = 0
    assert not dq.any(), "dQ outside (b0, i0, h0)"
    dk = got["dk"].clone()
    dk[b0, :, h0 * 64:h0 * 64 + 64] = 0
    assert not dk.any(), "dK outside (b0, h0)"


# ------------------------------------------------------------ tg_adaln_modulate_bwd --------------------------------------------------------
def _group_table(K, B, D, tokens, ngroups, seed, rows=5):
    """(GroupTable with a different shift / scale / gate column per group, the [B, tokens, D] scale and gate rows the kernels must gather)."""
    mod = _rand(B, rows, 3 * D * ngroups, seed=seed, scale=0.5)
    g = torch.Generator().manual_seed(seed + 1)
    tok = torch.arange(tokens) % ngroups if tokens >= ngroups else torch.randint(0, ngroups, (tokens,), generator=g)
    tok = tok[torch.randperm(tokens, generator=g)].to(torch.uint8)
    r = [int(x) for x in torch.randint(0, rows, (ngroups,), generator=g)]
    cols = [[3 * D * i + part * D for i in range(ngroups)] for part in range(3)]
    tab = K.GroupTable(mod.to(DEV), tok.to(DEV), r, *cols)
    rr = torch.tensor(r)[tok.long()]
    gather = lambda c: mod[:, rr[:, None], torch.tensor(c)[tok.long()][:, None] + torch.arange(D)[None]]
    return tab, gather(cols[1]), gather(cols[2])


def _adaln_bwd_run(lib, K, parity, B, Tk, D, what, ld_extra=16, seed=0):
    """All eight (modulate, products, add) combinations of one shape, per element.  x, dy, dx and add each have their OWN row stride (D + ld_extra + 0 / 8 / 16 / 24) and
    batch stride (tokens + 3 / 2 / 4 / 5 rows): a stride taken from the wrong tensor lands on sentinel values.  ld_extra % 8 == 0 keeps every row 16-byte aligned."""
    x, dy, add = _rand(B, Tk, D, seed=seed + 1, scale=2.0), _rand(B, Tk, D, seed=seed + 2), _rand(B, Tk, D, seed=seed + 3, scale=2.0)
    w, b = (1 + 0.2 * _randn(D, seed=seed + 4)).to(BF), _rand(D, seed=seed + 5, scale=0.2)
    tab, scale, _ = _group_table(K, B, D, Tk, 3, seed + 6)

    def strided(t, rows, ld, fill=None):                  # the view starts one row in
        full = torch.full((B, Tk + rows, D + ld_extra + ld), 9.0, dtype=BF, device=DEV)
        view = full[:, 1:1 + Tk, :D]
        view.copy_(t.to(DEV)) if t is not None else view.fill_(fill)
        return full, view
    (_, xd), (_, dyd), (_, addd) = strided(x, 3, 0), strided(dy, 2, 8), strided(add, 5, 24)
    assert len({t.stride(1) for t in (xd, dyd, addd)}) == 3 and (B == 1 or len({t.stride(0) for t in (xd, dyd, addd)}) == 3)      # (a batch stride is never used with batch 1)
    wd, bd = w.to(DEV), b.to(DEV)
    st = lambda t: (t.data_ptr(), t.stride(1), t.stride(0))
    for modulate in (0, 1):
        for use_add in (False, True):
            ref = T.adaln_bwd_ref(x, dy, w, b, 1e-5, scale if modulate else None, add if use_add else None)
            for products in (False, True):
                full, dx = strided(None, 4, 16, NAN)
                prods = [_flat_framed(B * Tk * D, F32) if products else (None, None) for _ in range(3)]
                lib.L.check(lib.so.tg_adaln_modulate_bwd(*st(xd), *st(dyd), *st(dx), wd.data_ptr(), bd.data_ptr(), 1e-5, Tk, D, B, modulate, tab.ref() if modulate else None,
                                                         *[K._p(p[1]) for p in prods], *(st(addd) if use_add else (None, 0, 0)), K._stream()), "tg_adaln_modulate_bwd")
                torch.cuda.synchronize()
                tag = f"{what} modulate={modulate} add={int(use_add)} products={int(products)}"
                assert bool((full[:, 0] == 9.0).all() and (full[:, Tk + 1:] == 9.0).all() and (full[:, :, D:] == 9.0).all()), tag
                parity(T.check(dx, *ref["dx"])[0], 1.0, f"adaln_modulate_bwd {tag} dx")
                if products:
                    for (pf, pv), n in zip(prods, ("t_dln", "t_dlnx", "t_dyln")):
                        assert _flat_untouched(pf, B * Tk * D), tag
                        parity(T.check(pv.view(B * Tk, D), *ref[n])[0], 1.0, f"adaln_modulate_bwd {tag} {n}")


@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("D", [8, 512, 3064, 3072, 3080, 4096, 4104])      # NC = 6 up to 3072, NC = 8 up to 4096, NC = 0 beyond: each chunk boundary and its neighbours
def test_adaln_bwd_vector_forms_per_element(lib, K, parity, D, rows):
    _adaln_bwd_run(lib, K, parity, 1, rows, D, f"D={D} rows={rows}", seed=D + rows)


def test_adaln_bwd_batch_strides_and_group_table(lib, K, parity):
    _adaln_bwd_run(lib, K, parity, 2, 9, 520, "D=520 tokens=9 batch=2", seed=77)


@pytest.mark.parametrize("D,ld_extra", [(100, 16), (512, 20)], ids=["dim_100", "row_stride_not_a_multiple_of_8"])
def test_adaln_bwd_scalar_form_per_element(lib, K, parity, D, ld_extra):
    """The scalar kernel, reached by dim % 8 != 0 and, separately, by row strides that are no multiples of 8.  For D = 512 the vector form then runs on the SAME values
    (same seed): both forms are held to the same reference and the same bounds."""
    _adaln_bwd_run(lib, K, parity, 2, 5, D, f"D={D} scalar (ld = D + {ld_extra})", ld_extra=ld_extra, seed=5)
    if D == 512:
        _adaln_bwd_run(lib, K, parity, 2, 5, D, f"D={D} vector, the scalar case's values", ld_extra=16, seed=5)


# ------------------------------------------------------------ tg_qk_layernorm_rope_bwd -----------------------------------------------------
@pytest.mark.parametrize("Tk,H", [(85, 3), (64, 4), (257, 1), (73, 7), (171, 3)], ids=["510_rows", "512_rows", "514_rows", "1022_rows", "1026_rows"])
def test_qk_layernorm_rope_bwd_per_element_and_per_block(lib, K, parity, Tk, H):
    """batch 2 x tokens x heads rows around the 512-row blocks (the total is even with batch 2: 510 = one ragged block, 512 = exactly one, 514 = a second block of 2 rows;
    2 x 511 = a ragged second block, 2 x 513 = a third block of 2 rows).  Two rotary segments that neither start at 0 nor touch, un-rotated rows before, between and after; out_scale != 1; distinct batch strides for x, dy and dx."""
    B, HD = 2, H * 64
    n0, n1 = Tk // 4, Tk // 3
    s0, s1 = 3, 3 + n0 + 2
    assert s1 + n1 < Tk - 1
    x, dy = _rand(B, Tk, HD, seed=Tk, scale=1.3), _randn(B, Tk, HD, seed=Tk + 1)
    w = (1 + 0.2 * _randn(64, seed=3)).to(BF)
    tabs = []
    for start, n, seed in ((s0, n0, 5), (s1, n1, 6)):
        ang = torch.rand(n, 32, generator=torch.Generator().manual_seed(seed)) * 6.28
        tabs.append((start, ang.cos().repeat_interleave(2, 1).contiguous(), ang.sin().repeat_interleave(2, 1).contiguous()))
    ref = T.qk_rope_bwd_ref(x, dy, H, w, 1e-6, tabs, 0.37)
    xd = torch.zeros(B, Tk + 1, 3 * HD, dtype=BF, device=DEV)[:, :Tk, HD:2 * HD]
    xd.copy_(x.to(DEV))
    dyd = torch.zeros(B, Tk + 2, HD + 4, dtype=F32, device=DEV)[:, 1:1 + Tk, :HD]
    dyd.copy_(dy.to(DEV))
    full, dx = _framed(B, Tk, HD, BF, NAN)
    nfl = lib.so.tg_qk_layernorm_rope_bwd_partial_floats(Tk, H, B)
    assert nfl == ref["partial"][0].numel()
    pfull, part = _flat_framed(nfl, F32)
    dev = [(s, c.to(DEV), sn.to(DEV)) for s, c, sn in tabs]
    wd = w.to(DEV)
    lib.L.check(lib.so.tg_qk_layernorm_rope_bwd(xd.data_ptr(), xd.stride(1), xd.stride(0), dyd.data_ptr(), dyd.stride(1), dyd.stride(0), dx.data_ptr(), dx.stride(1), dx.stride(0),
                                                Tk, H, B, wd.data_ptr(), 1e-6, dev[0][0], n0, dev[0][1].data_ptr(), dev[0][2].data_ptr(), dev[1][0], n1,
                                                dev[1][1].data_ptr(), dev[1][2].data_ptr(), 0.37, part.data_ptr(), K._stream()), "tg_qk_layernorm_rope_bwd")
    torch.cuda.synchronize()
    assert _frame_untouched(full, Tk, HD) and _flat_untouched(pfull, nfl)
    what = f"qk_layernorm_rope_bwd tokens={Tk} heads={H} batch=2"
    parity(T.check(dx, *ref["dx"])[0], 1.0, what + " dx")
    parity(T.check(part.view(-1, 2, 64), *ref["partial"])[0], 1.0, what + " partial, block by block")


# ------------------------------------------------------------ tg_gate_residual_bwd ---------------------------------------------------------
def _gate_cases():
    """(form, batch, tokens, dim) x t_row0 in {0, 1, tokens - 1}.  Scalar form (one element per thread, 256 per block; reached by dim % 8 != 0 or a pointer offset by 2 bytes):
    batch tokens dim = 1, 7, 8, 2047, 2048, 2049.  Vector form (8 elements per thread): 1, 255, 256 and 257 chunks — a partly filled block, a full one, a second block of one
    thread — and a batch-2 case with a few rows."""
    shapes = [("dim", 1, 1, 1), ("dim", 1, 7, 1), ("offset", 1, 1, 8), ("dim", 1, 23, 89), ("offset", 2, 16, 64), ("dim", 1, 3, 683),
              ("vector", 1, 1, 8), ("vector", 1, 15, 136), ("vector", 2, 16, 64), ("vector", 1, 257, 8), ("vector", 2, 11, 40)]
    return [(f, B, Tk, D, r0) for f, B, Tk, D in shapes for r0 in sorted({0, min(1, Tk - 1), Tk - 1})]


@pytest.mark.parametrize("form,B,Tk,D,row0", _gate_cases())
def test_gate_residual_bwd_is_exact(lib, K, parity, form, B, Tk, D, row0):
    assert (form == "dim") == (D % 8 != 0)
    dout, y = _rand(B, Tk, D, seed=41 + Tk), _rand(B, Tk - row0, D, seed=42 + Tk)          # y holds only the kept rows
    tab, _, gate = _group_table(K, B, D, Tk, 4, seed=43)
    ref = T.gate_res_bwd_ref(dout, y, gate, row0)
    off = 1 if form == "offset" else 0
    dbuf = torch.zeros(B * (Tk + 1) * (D + 8) + 8, dtype=BF, device=DEV)
    dd = dbuf[off:].as_strided((B, Tk, D), ((Tk + 1) * (D + 8), D + 8, 1))
    dd.copy_(dout.to(DEV))
    yd = y.to(DEV).contiguous()
    full, dy = _framed(B, Tk, D, BF, NAN)
    tfull, tg = _flat_framed(B * (Tk - row0) * D, F32)
    y_ptr = yd.data_ptr() - row0 * D * 2                                          # the address row 0 WOULD have
    lib.L.check(lib.so.tg_gate_residual_bwd(dd.data_ptr(), dd.stride(1), dd.stride(0), y_ptr, D, (Tk - row0) * D, dy.data_ptr(), dy.stride(1), dy.stride(0), Tk, D, B, tab.ref(),
                                            tg.data_ptr(), row0, K._stream()), "tg_gate_residual_bwd")
    torch.cuda.synchronize()
    assert _frame_untouched(full, Tk, D) and _flat_untouched(tfull, tg.numel())
    what = f"gate_residual_bwd {form} batch={B} tokens={Tk} dim={D} t_row0={row0}"
    r_dy, r_tg = T.check(dy, *ref["dy"])[0], T.check(tg.view(B, Tk - row0, D), *ref["t_dgate"])[0]
    parity(r_dy, 1.0, what + " dy")                        # zero bounds: the ratio is 0 (equal) or inf
    parity(r_tg, 1.0, what + " t_dgate")
    assert r_dy == 0.0 and r_tg == 0.0, what


# ------------------------------------------------------------------- tg_act ----------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 8, 2047, 2048, 2049])
def test_act_per_element_vector_and_scalar_forms(lib, K, parity, n):
    """n % 8 == 0 takes the 16-byte form, everything else the scalar one; n = 8 / 2048 also run from a pointer offset by 2 bytes (scalar form on the same values: same bits)."""
    x, dy = _rand(n + 1, seed=n, scale=2.5), _rand(n + 1, seed=n + 1)
    for off in ((0, 1) if n % 8 == 0 else (0,)):
        xs, ds = x[:n], dy[:n]
        xd, dd = torch.zeros(n + 8, dtype=BF, device=DEV)[off:off + n], torch.zeros(n + 8, dtype=BF, device=DEV)[off:off + n]
        xd.copy_(xs.to(DEV)); dd.copy_(ds.to(DEV))
        outs = []
        for mode in (0, 1, 2):
            full = torch.full((n + 64,), 9.0, dtype=BF, device=DEV)
            out = full[32 + off:32 + off + n]
            out.fill_(NAN)
            lib.L.check(lib.so.tg_act(xd.data_ptr(), dd.data_ptr() if mode == 1 else None, out.data_ptr(), n, mode, K._stream()), "tg_act")
            torch.cuda.synchronize()
            assert bool((full[:32 + off] == 9.0).all() and (full[32 + off + n:] == 9.0).all())
            parity(T.check(out, *T.act_ref(xs, ds, mode))[0], 1.0, f"act n={n} mode={mode} {'scalar (offset pointer)' if off else 'natural form'}")
            outs.append(out.cpu())
        if off:
            assert all(torch.equal(a, b) for a, b in zip(outs, first))
        first = outs


# ------------------------------------------------------------------ tg_colsum* -------------------------------------------------------------
def _colsum_cases():
    """rows {1, 255, 256, 257, 1000} x cols {8, 30, 72, 3072} (all of them 8-row blocks: the launch wants ~2000 workgroups) + the two other block sizes of cs_rows: (2731, 3072) -> 17 rows per block,
    (524289, 8) -> the 256-row clamp with a last block of ONE row."""
    return [(r, c) for c in (8, 30, 72, 3072) for r in (1, 255, 256, 257, 1000)] + [(2731, 3072), (524289, 8)]


@pytest.mark.parametrize("rows,cols", _colsum_cases())
def test_colsum_every_partial_row(lib, K, parity, rows, cols):
    """tg_colsum (16-byte form: cols % 8 == 0 and an aligned source; scalar form: cols = 30, or the same matrix from a pointer offset by 2 bytes) and tg_colsum_f32: every
    partial row against the fp64 sum of that block's rows."""
    m = _randn(rows, cols, seed=rows + cols)
    per = T.colsum_block_rows(rows, cols)
    nblk = (rows + per - 1) // per
    assert per == {2731: 17, 524289: 256}.get(rows, 8)
    assert lib.so.tg_colsum_partial_floats(rows, cols) == nblk * cols
    ld = cols + 8
    for dtype, offs in ((BF, (0, 1)), (F32, (0,))):
        src_cpu = m.to(dtype)
        ref = T.colsum_ref(src_cpu, per)
        for off in offs:
            buf = torch.zeros(rows * ld + 8, dtype=dtype, device=DEV)
            src = buf[off:off + rows * ld].view(rows, ld)[:, :cols]
            src.copy_(src_cpu.to(DEV))
            pfull, part = _flat_framed(nblk * cols, F32)
            fn = lib.so.tg_colsum if dtype == BF else lib.so.tg_colsum_f32
            lib.L.check(fn(src.data_ptr(), ld, rows, cols, part.data_ptr(), K._stream()), "tg_colsum")
            torch.cuda.synchronize()
            assert _flat_untouched(pfull, nblk * cols)
            parity(T.check(part.view(nblk, cols), *ref)[0], 1.0, f"colsum{'_f32' if dtype == F32 else ''} rows={rows} cols={cols} offset={off}")


@pytest.mark.parametrize("row_blocks", [1, 3])
def test_colsum_multi_mixed_items(lib, K, parity, row_blocks):
    # mixed dtype and row counts; the third item spans three 256-column blocks (the kernel finds a block's item through first_block), the last is shorter than row_blocks
    mats = [_randn(257, 72, seed=1).to(BF), _randn(1000, 30, seed=2), _randn(300, 520, seed=4).to(BF), _randn(1, 8, seed=3).to(BF)]
    dev = [torch.zeros(m.shape[0], m.shape[1] + 4, dtype=m.dtype, device=DEV)[:, :m.shape[1]] for m in mats]
    items = (lib.L.ColsumItem * len(mats))()
    for i, (m, dm) in enumerate(zip(mats, dev)):
        dm.copy_(m.to(DEV))
        items[i].src, items[i].ld, items[i].rows, items[i].cols, items[i].src_is_f32 = dm.data_ptr(), dm.stride(0), m.shape[0], m.shape[1], int(m.dtype == F32)
    total = sum(m.shape[1] for m in mats)
    pfull, part = _flat_framed(row_blocks * total, F32)
    lib.L.check(lib.so.tg_colsum_multi(items, len(mats), row_blocks, part.data_ptr(), K._stream()), "tg_colsum_multi")
    torch.cuda.synchronize()
    assert _flat_untouched(pfull, row_blocks * total)
    parity(T.check(part.view(row_blocks, total), *T.colsum_multi_ref(mats, row_blocks))[0], 1.0, f"colsum_multi row_blocks={row_blocks}")


# --------------------------------------------------------------- loss kernels --------------------------------------------------------------
@pytest.mark.parametrize("valid", [(3, 3), (1, 3), (3, 2)], ids=lambda v: f"valid_{v[0]}_{v[1]}")
@pytest.mark.parametrize("E", [8, 255, 256, 257, 4096 + 8])
def test_vpred_loss_kernels_per_element_and_per_block(lib, K, parity, E, valid):
    B, Fr = 2, 3
    out, noisy, tgt = (_rand(B * Fr, E, seed=E + s) for s in (1, 2, 3))
    acp = torch.tensor([0.9, 0.5, 0.1, 0.7, 0.3, 0.02])                          # coefficient rows that differ per frame
    coef = torch.stack([acp.sqrt(), (1 - acp).sqrt(), 1 / (1 - acp)], 1).float().contiguous()
    od, nd, td, cd = out.to(DEV), noisy.to(DEV), tgt.to(DEV), coef.to(DEV)
    nblk = (E + 255) // 256
    assert lib.so.tg_vpred_loss_partial_floats(B * Fr, E) == B * Fr * nblk

    def launch(masked):
        gfull, grad = _flat_framed(B * Fr * E, BF)
        pfull, part = _flat_framed(B * Fr * nblk, F32)
        if masked:
            vd = torch.tensor(valid, dtype=torch.int32, device=DEV)
            lib.L.check(lib.so.tg_vpred_loss_grad_masked(od.data_ptr(), nd.data_ptr(), td.data_ptr(), cd.data_ptr(), vd.data_ptr(), B, Fr, E, grad.data_ptr(), part.data_ptr(),
                                                         K._stream()), "tg_vpred_loss_grad_masked")
        else:
            lib.L.check(lib.so.tg_vpred_loss_grad(od.data_ptr(), nd.data_ptr(), td.data_ptr(), cd.data_ptr(), B * Fr, E, 1.0 / (Fr * E * B), grad.data_ptr(), part.data_ptr(),
                                                  K._stream()), "tg_vpred_loss_grad")
        torch.cuda.synchronize()
        assert _flat_untouched(gfull, B * Fr * E) and _flat_untouched(pfull, B * Fr * nblk)
        return grad.view(B * Fr, E), part.view(B * Fr, nblk)
    ref = T.vpred_loss_ref(out, noisy, tgt, coef, None, valid_frames=valid, frames=Fr)
    grad, part = launch(True)
    what = f"vpred_loss_grad_masked E={E} valid={valid}"
    parity(T.check(grad, *ref["grad"])[0], 1.0, what + " grad")
    parity(T.check(part, *ref["partial"])[0], 1.0, what + " partial, block by block")
    for b in range(B):                                                            # the masked frames: exactly zero
        assert not grad[b * Fr + valid[b]:(b + 1) * Fr].float().any() and not part[b * Fr + valid[b]:(b + 1) * Fr].any()
    if valid == (3, 3):
        g2, p2 = launch(False)
        un = T.vpred_loss_ref(out, noisy, tgt, coef, 1.0 / (Fr * E * B))
        parity(T.check(g2, *un["grad"])[0], 1.0, f"vpred_loss_grad E={E} grad")
        parity(T.check(p2, *un["partial"])[0], 1.0, f"vpred_loss_grad E={E} partial, block by block")
        assert torch.equal(g2, grad) and torch.equal(p2, part)                    # everything valid: bitwise the unmasked kernel
