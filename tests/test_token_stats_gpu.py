"""GPU: the streaming fit of the T2To token statistics (tokensgen_amd/token_stats.py on tg_gram_accumulate / tg_pca_coef_stats).

Kernels: every element against fp64 torch on the same bf16 inputs, within bounds DERIVED from the arithmetic the header documents (edge_bounds.check), at
row counts around the fp32 fold length, with padded row strides; the padding columns and the rows after `rows` hold bf16 NaN, so any read of them shows
up as a non-finite total.
  gram:    calls * F * 2^-23 * (|X|^T |X|)[i][j] + 2^-50 |ref|: at most F = tg_gram_fold_rows() exact bf16 products are added in fp32 (either rounding
           mode, any order) before the partial joins the fp64 total.  colsum likewise with sum |x|.
  coef:    per row e_r = (D + 2) 2^-23 sum_c |x - mu| |v_c| (D fp32 fused multiply-adds in any order, the fp32 subtraction, the final adds); sum within
           sum_r e_r, sumsq within sum_r (2 |y_r| e_r + e_r^2), each + 2^-50 |ref|; | |extreme| - max |y| | <= 2 max e_r with the fp64 arg-max's sign.

End to end on tests/golden/token_stats_tiny.pt: every fitted quantity stays below 16x the distance of the reference's OWN fp32 run from its fp64 run (the
fixture's yardstick, never derived from the code under test; a CPU emulation of 256-row fp32 folds gave 0.19x .. 4.6x of it for the components).  The figures
measured on the MI355X are in profiles/token_stats_parity.json."""
import os

import pytest
import torch

import edge_bounds as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
F64 = torch.float64
NAN = float("nan")


def _lib():
    from tokensgen_amd import lib as L
    return L, L.load()


def _fold():
    return _lib()[1].tg_gram_fold_rows()


def _padded(x, ldx, extra_rows=3):
    """x bf16 [rows, D] inside a NaN-filled [rows + extra_rows, ldx] buffer on the GPU: (buffer, view of the valid part)."""
    buf = torch.full((x.shape[0] + extra_rows, ldx), NAN, dtype=BF, device=DEV)
    buf[:x.shape[0], :x.shape[1]] = x.to(DEV)
    return buf


def _gram(buf, ldx, rows, D, gram, colsum):
    L, lib = _lib()
    L.check(lib.tg_gram_accumulate(buf.data_ptr(), ldx, rows, D, gram.data_ptr(), colsum.data_ptr(), torch.cuda.current_stream().cuda_stream), "tg_gram_accumulate")


GRAM_CASES = [(lambda F: 1, 128, 128), (lambda F: 37, 128, 136), (lambda F: F - 1, 256, 256), (lambda F: F, 256, 256), (lambda F: F + 1, 256, 264),
              (lambda F: 2 * F + 77, 384, 392),
              (lambda F: 40, 896, 904)]          # 7 x 7 blocks, 28 tiles: the tile numbering beyond a few rows of the triangle, every tile exactly once


@pytest.mark.parametrize("case", range(len(GRAM_CASES)))
def test_gram_accumulate_per_element_vs_fp64(case):
    F = _fold()
    assert 1 <= F <= 512
    rows_of, D, ldx = GRAM_CASES[case]
    rows = rows_of(F)
    g = torch.Generator().manual_seed(100 + case)
    x = (torch.randn(rows, D, generator=g) * (0.5 + torch.rand(D, generator=g)) + 0.3).to(BF)
    buf = _padded(x, ldx)
    gram, colsum = torch.zeros(D, D, dtype=F64, device=DEV), torch.zeros(D, dtype=F64, device=DEV)
    calls = 2
    for _ in range(calls):                                   # the second call must add
        _gram(buf, ldx, rows, D, gram, colsum)
    torch.cuda.synchronize()
    x64 = x.to(F64)
    ref, mag = calls * (x64.T @ x64), x64.abs().T @ x64.abs()
    worst, where = E.check(gram, ref, calls * F * 2.0 ** -23 * mag + 2.0 ** -50 * ref.abs())
    print(f"gram rows={rows} D={D} ldx={ldx}: worst error / bound = {worst:.3e} at {where}")
    assert worst <= 1.0, (worst, where)
    cref, cmag = calls * x64.sum(0), x64.abs().sum(0)
    cworst, cwhere = E.check(colsum, cref, calls * F * 2.0 ** -23 * cmag + 2.0 ** -50 * cref.abs())
    print(f"colsum: worst error / bound = {cworst:.3e} at {cwhere}")
    assert cworst <= 1.0, (cworst, cwhere)
    assert torch.equal(gram, gram.T)                         # the mirror is a copy: bitwise
    gram2, colsum2 = torch.zeros_like(gram), torch.zeros_like(colsum)
    for _ in range(calls):
        _gram(buf, ldx, rows, D, gram2, colsum2)
    assert torch.equal(gram2, gram) and torch.equal(colsum2, colsum)      # same inputs, same bits


def _coef_inputs(rows, D, nc, seed):
    """Inputs whose per-coefficient extreme is not a near tie between opposite signs (margin 1.001 in fp64): the first seed that meets it."""
    for s in range(seed, seed + 50):
        g = torch.Generator().manual_seed(s)
        x = (torch.randn(rows, D, generator=g) + 0.3).to(BF)
        pmean = (0.3 + 0.05 * torch.randn(D, generator=g)).float()
        q, _ = torch.linalg.qr(torch.randn(D, nc, generator=g))
        comp = q.T.contiguous().float()
        y = (x.to(F64) - pmean.to(F64)) @ comp.to(F64).T
        if rows == 1:
            return x, pmean, comp, y
        top = torch.topk(y.abs(), 2, dim=0)
        sg = torch.sign(y)
        cols = torch.arange(nc)
        tie = (sg[top.indices[0], cols] != sg[top.indices[1], cols]) & (top.values[0] < 1.001 * top.values[1])
        if not tie.any():
            return x, pmean, comp, y
    raise AssertionError("no seed with a 1.001 margin")


@pytest.mark.parametrize("rows,D,nc", [(1, 128, 16), (95, 128, 16), (385, 384, 64)])
def test_pca_coef_stats_vs_fp64(rows, D, nc):
    L, lib = _lib()
    ldx = D + 8
    x, pmean, comp, y = _coef_inputs(rows, D, nc, 7 * rows)
    buf = _padded(x, ldx)
    s, s2 = torch.zeros(nc, dtype=F64, device=DEV), torch.zeros(nc, dtype=F64, device=DEV)
    ex = torch.zeros(nc, dtype=torch.float32, device=DEV)
    ws = torch.empty(lib.tg_pca_coef_stats_ws_floats(rows, nc), dtype=torch.float32, device=DEV)
    cd, pd = comp.to(DEV), pmean.to(DEV)
    run = lambda b: L.check(lib.tg_pca_coef_stats(b.data_ptr(), ldx, rows, D, cd.data_ptr(), nc, pd.data_ptr(), s.data_ptr(), s2.data_ptr(), ex.data_ptr(),
                                                  ws.data_ptr(), torch.cuda.current_stream().cuda_stream), "tg_pca_coef_stats")
    run(buf)
    torch.cuda.synchronize()
    e = (D + 2) * 2.0 ** -23 * ((x.to(F64) - pmean.to(F64)).abs() @ comp.to(F64).abs().T)            # [rows, nc]
    ref_s, ref_s2 = y.sum(0), (y * y).sum(0)
    w1, at1 = E.check(s, ref_s, e.sum(0) + 2.0 ** -50 * ref_s.abs())
    w2, at2 = E.check(s2, ref_s2, (2 * y.abs() * e + e * e).sum(0) + 2.0 ** -50 * ref_s2.abs())
    ymax = y.abs().max(0)
    w3, at3 = E.check(ex.abs(), ymax.values, 2 * e.max(0).values)
    print(f"coef stats rows={rows} D={D} ncoef={nc}: error / bound sum {w1:.3e} sumsq {w2:.3e} |extreme| {w3:.3e}")
    assert w1 <= 1.0 and w2 <= 1.0 and w3 <= 1.0, (w1, at1, w2, at2, w3, at3)
    assert torch.equal(torch.sign(ex.cpu()).double(), torch.sign(y[ymax.indices, torch.arange(nc)]))
    # rows of smaller magnitude leave the extreme alone (and the sums go on adding)
    x2 = (pmean + 0.25 * (x.float() - pmean)).to(BF)
    y2 = (x2.to(F64) - pmean.to(F64)) @ comp.to(F64).T
    assert (y2.abs().max(0).values < 0.9 * ymax.values).all()
    before, s_before = ex.clone(), s.clone()
    run(_padded(x2, ldx))
    torch.cuda.synchronize()
    assert torch.equal(ex, before) and not torch.equal(s, s_before)
    e2 = (D + 2) * 2.0 ** -23 * ((x2.to(F64) - pmean.to(F64)).abs() @ comp.to(F64).abs().T)
    w4, at4 = E.check(s, ref_s + y2.sum(0), e.sum(0) + e2.sum(0) + 2.0 ** -50 * (ref_s + y2.sum(0)).abs())
    assert w4 <= 1.0, (w4, at4)


@pytest.fixture(scope="module")
def fitted(golden_dir):
    """The whole fit on the fixture, once: pass 1 in two batches with valid_chunks, fit(16), pass 2, finalize."""
    from tokensgen_amd.token_stats import TokenStats
    g = torch.load(os.path.join(golden_dir, "token_stats_tiny.pt"))
    tok, valid, ntq = g["tokens"].to(DEV), g["valid_chunks"], g["num_temporal_queries"]
    st = TokenStats(128, DEV)
    for lo, hi in ((0, 2), (2, 4)):
        st.update(tok[lo:hi], valid[lo:hi], ntq)
    coef = st.fit(16)
    for lo, hi in ((0, 2), (2, 4)):
        coef.update(tok[lo:hi], valid[lo:hi], ntq)
    return g, st, coef, coef.finalize()


def test_end_to_end_fit_against_the_reference_fp64_run(fitted, parity):
    g, st, coef, norm = fitted
    assert st.n == coef.n == 672
    V = norm.pca.components_.double()
    assert ((V * g["components64"]).sum(1) > 0).all(), "signs differ from the reference's fp64 run"
    factor = 16.0
    parity((V - g["components64"]).abs().max(), factor * g["yard_components"], "components max-abs vs reference fp64")
    parity((norm.pca.mean_.double() - g["mean64"]).abs().max(), factor * g["yard_mean"], "mean_ max-abs vs reference fp64")
    parity((norm.mean.double() - g["coef_mean64"]).abs().max(), factor * g["yard_coef_mean"], "coefficient mean max-abs vs reference fp64")
    parity(((norm.std.double() - g["coef_std64"]).abs() / g["coef_std64"]).max(), factor * g["yard_coef_std"], "coefficient std max-rel vs reference fp64")


def test_merge_of_halves_equals_one_pass(fitted):
    from tokensgen_amd.token_stats import TokenStats
    g, st, _, _ = fitted
    tok, valid, ntq = g["tokens"].to(DEV), g["valid_chunks"], g["num_temporal_queries"]
    a, b = TokenStats(128, DEV).update(tok[:2], valid[:2], ntq), TokenStats(128, DEV).update(tok[2:], valid[2:], ntq)
    whole = TokenStats(128, DEV).update(tok, valid, ntq)
    a.merge(b)
    rows = torch.cat([tok[i, :int(v) * ntq].permute(0, 2, 3, 1).reshape(-1, 128) for i, v in enumerate(valid)]).to("cpu", F64)
    mag = rows.abs().T @ rows.abs()
    assert a.n == whole.n == 672
    # the fp32 folds are the same launches; only the order of the fp64 additions differs
    assert ((a.gram - whole.gram).abs().cpu() <= 2.0 ** -50 * mag).all()
    assert ((a.colsum - whole.colsum).abs().cpu() <= 2.0 ** -50 * rows.abs().sum(0)).all()
    assert torch.equal(whole.gram, st.gram)                  # and the batching of `update` does not change the launches


def test_fitted_statistics_drive_pca_project16_and_the_pipeline_loader(fitted, tmp_path):
    from tokensgen_amd.pipeline_t2to import _load
    from tokensgen_amd.token_stats import TokenNorm
    from tokensgen_amd.train_t2to import pca_project16
    g, _, _, norm = fitted
    tok, valid, ntq = g["tokens"].to(DEV), g["valid_chunks"], g["num_temporal_queries"]
    out = pca_project16(tok, norm.pca.components_, norm.pca.mean_, norm.mean, norm.std)
    assert out.shape == (4, 8, 16, 4, 6) and out.dtype == BF
    rows = torch.cat([out[i, :int(v) * ntq].permute(0, 2, 3, 1).reshape(-1, 16) for i, v in enumerate(valid)]).double().cpu()
    assert rows.shape == (672, 16)
    # pooled statistics through pca.transform make the normalised coefficients zero-mean / unit-variance; the bf16 output rounding is <= 2^-8 relative
    assert rows.mean(0).abs().max().item() < 0.01 and (rows.std(0) - 1).abs().max().item() < 0.01
    norm.save(str(tmp_path))
    mean, std, pca = (_load(str(tmp_path / n)) for n in ("mean.pt", "std.pt", "pca.pt"))
    assert torch.equal(mean, norm.mean) and torch.equal(std, norm.std) and torch.equal(pca.components_, norm.pca.components_)
    back = TokenNorm.load(str(tmp_path))
    assert torch.equal(pca_project16(tok, back.pca.components_, back.pca.mean_, back.mean, back.std), out)
