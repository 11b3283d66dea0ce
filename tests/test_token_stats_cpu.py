"""tokensgen_amd.token_stats without a GPU: the finalisation of the streaming fit (eigh of the scatter matrix from fp64 totals, the u-based sign rule, pooled
mean / unbiased std), merge / state_dict, and the three files it writes.  The totals are built here with plain fp64 torch on the valid rows of
tests/golden/token_stats_tiny.pt and injected through load_state_dict; the expected values are the reference's own pca.PCA run in fp64
(tools/make_token_stats_golden.py).  The kernels that build the totals on the GPU are held to fp64 in tests/test_token_stats_gpu.py."""
import os
import pickletools

import pytest
import torch

F64 = torch.float64


@pytest.fixture(scope="module")
def fx(golden_dir):
    g = torch.load(os.path.join(golden_dir, "token_stats_tiny.pt"))
    tok, ntq = g["tokens"], g["num_temporal_queries"]
    C = tok.shape[2]
    g["rows64"] = torch.cat([tok[b, :int(v) * ntq].permute(0, 2, 3, 1).reshape(-1, C) for b, v in enumerate(g["valid_chunks"])]).to(F64)
    return g


def _stats_from(x64):
    from tokensgen_amd.token_stats import TokenStats
    st = TokenStats(x64.shape[1], "cpu")
    return st.load_state_dict({"n": x64.shape[0], "gram": x64.T @ x64, "colsum": x64.sum(0), "dim": x64.shape[1]})


def _second_pass(coef, x64):
    """What tg_pca_coef_stats accumulates, in fp64, injected through load_state_dict."""
    y = (x64 - coef.mean64) @ coef.components64.T
    ext = y[y.abs().argmax(0), torch.arange(y.shape[1])]
    return coef.load_state_dict({"n": x64.shape[0], "sum": y.sum(0), "sumsq": (y * y).sum(0), "extreme": ext.float(), "dim": x64.shape[1]}), y


def test_fit_from_fp64_totals_matches_the_reference_fp64_run(fx):
    x = fx["rows64"]
    assert x.shape == (672, 128)
    coef = _stats_from(x).fit(16)
    V, ref = coef.components64, fx["components64"]
    sgn = torch.sign((V * ref).sum(1))
    assert (V * sgn[:, None] - ref).abs().max().item() < 1e-10          # fp64 eigh against fp64 SVD measured 3e-15 .. 1.4e-14: a cap, not a measurement
    assert (coef.mean64 - fx["mean64"][0]).abs().max().item() < 1e-12
    # the holder carries the fp32 rounding of exactly these, in the reference's shapes
    assert coef.pca.mean_.shape == (1, 128) and coef.pca.components_.shape == (16, 128)
    assert coef.pca.mean_.dtype == coef.pca.components_.dtype == torch.float32
    assert torch.equal(coef.pca.components_, V.float()) and torch.equal(coef.pca.mean_[0], coef.mean64.float())
    assert torch.equal(_stats_from(x).fit(None).pca.components_[:16], coef.pca.components_) and _stats_from(x).fit(None).d == 128


def test_finalize_signs_mean_and_std_from_injected_sums(fx):
    x = fx["rows64"]
    coef, y = _second_pass(_stats_from(x).fit(16), x)
    before = coef.pca.components_.clone()
    norm = coef.finalize()
    # the reference's signs, not "up to sign"
    assert ((norm.pca.components_.double() * fx["components64"]).sum(1) > 0).all()
    assert (norm.pca.components_.double() - fx["components64"]).abs().max().item() < 1e-7
    flipped = (norm.pca.components_ * before).sum(1) < 0
    assert flipped.any() and not flipped.all(), "the fixture exercises both signs"
    # a flipped component flips its coefficient mean; std is unbiased and sign-free
    want_mean = torch.where(flipped, -1.0, 1.0).double() * y.mean(0)
    assert (norm.mean.double() - want_mean).abs().max().item() < 1e-9 + 2.0 ** -24 * want_mean.abs().max().item()
    assert (norm.mean.double() - fx["coef_mean64"]).abs().max().item() < 1e-7
    assert ((norm.std.double() - fx["coef_std64"]).abs() / fx["coef_std64"]).max().item() < 1e-6
    assert norm.mean.dtype == norm.std.dtype == torch.float32 and norm.mean.shape == norm.std.shape == (16,)
    # flipping the injected extreme of one component flips that component and its mean, nothing else
    sd = coef.state_dict()
    sd["extreme"] = sd["extreme"].clone()
    sd["extreme"][3] = -sd["extreme"][3]
    other = coef.load_state_dict(sd).finalize()
    assert torch.equal(other.pca.components_[3], -norm.pca.components_[3]) and other.mean[3] == -norm.mean[3] and other.std[3] == norm.std[3]
    keep = torch.arange(16) != 3
    assert torch.equal(other.pca.components_[keep], norm.pca.components_[keep]) and torch.equal(other.mean[keep], norm.mean[keep])


def test_save_load_round_trip_and_file_formats(fx, tmp_path):
    import sys
    from tokensgen_amd.pca import PCA
    from tokensgen_amd.token_stats import TokenNorm
    x = fx["rows64"]
    norm = _second_pass(_stats_from(x).fit(16), x)[0].finalize()
    had = "pca" in sys.modules
    norm.save(str(tmp_path / "stats"))
    assert ("pca" in sys.modules) == had and PCA.__module__ == "tokensgen_amd.pca"
    raw = (tmp_path / "stats" / "pca.pt").read_bytes()
    assert b"tokensgen_amd" not in raw
    import zipfile
    with zipfile.ZipFile(tmp_path / "stats" / "pca.pt") as z:
        pkl = z.read([n for n in z.namelist() if n.endswith("data.pkl")][0])
    globs = {(op.name, arg) for op, arg, _ in pickletools.genops(pkl) if op.name in ("GLOBAL", "STACK_GLOBAL")}
    strings = [arg for op, arg, _ in pickletools.genops(pkl) if op.name in ("SHORT_BINUNICODE", "BINUNICODE", "UNICODE")]
    assert ("GLOBAL", "pca PCA") in globs or ("pca" in strings and "PCA" in strings and strings.index("PCA") == strings.index("pca") + 1)
    mean = torch.load(tmp_path / "stats" / "mean.pt", weights_only=True)
    std = torch.load(tmp_path / "stats" / "std.pt", weights_only=True)
    assert torch.equal(mean, norm.mean) and torch.equal(std, norm.std)
    back = TokenNorm.load(str(tmp_path / "stats"))
    assert type(back.pca) is PCA and back.pca.n_components == 16
    assert torch.equal(back.pca.components_, norm.pca.components_) and torch.equal(back.pca.mean_, norm.pca.mean_)
    assert torch.equal(back.mean, norm.mean) and torch.equal(back.std, norm.std)
    # and the way the T2To pipeline reads them
    from tokensgen_amd.pipeline_t2to import _load
    got = _load(str(tmp_path / "stats" / "pca.pt"))
    assert torch.equal(got.components_, norm.pca.components_) and torch.equal(_load(str(tmp_path / "stats" / "std.pt")), norm.std)
    if not had:
        sys.modules.pop("pca", None)                 # compat.ensure_pca_module registered it for the loads above


def test_merge_is_addition_and_dim_mismatch_raises(fx):
    from tokensgen_amd.token_stats import TokenStats
    x = fx["rows64"]
    a, b, whole = _stats_from(x[:300]), _stats_from(x[300:]), _stats_from(x)
    ga, gb = a.gram.clone(), b.gram.clone()
    a.merge(b)
    assert a.n == 672 and torch.equal(a.gram, ga + gb) and torch.equal(b.gram, gb)
    assert torch.allclose(a.gram, whole.gram, rtol=1e-13, atol=0) and torch.allclose(a.colsum, whole.colsum, rtol=1e-13, atol=0)
    with pytest.raises(ValueError):
        a.merge(TokenStats(256, "cpu"))
    with pytest.raises(ValueError):
        TokenStats(256, "cpu").load_state_dict(whole.state_dict())
    sd = whole.state_dict()
    assert set(sd) == {"n", "gram", "colsum", "dim"} and sd["dim"] == 128 and sd["n"] == 672
    # CoefficientStats: sums add, the extreme of larger magnitude wins
    ca, _ = _second_pass(_stats_from(x).fit(16), x[:300])
    cb, _ = _second_pass(_stats_from(x).fit(16), x[300:])
    cw, _ = _second_pass(_stats_from(x).fit(16), x)
    ca.merge(cb)
    assert ca.n == 672 and torch.allclose(ca.sumsq, cw.sumsq, rtol=1e-13, atol=0) and torch.equal(ca.extreme, cw.extreme)
    # statistics of another fit do not add up to anything: refused
    with pytest.raises(ValueError, match="different fits"):
        ca.merge(_second_pass(_stats_from(x[:300]).fit(16), x[:300])[0])
    with pytest.raises(ValueError):
        ca.merge(_second_pass(_stats_from(x).fit(8), x)[0])


def test_all_reduce_sums_totals_and_keeps_the_extreme_of_largest_magnitude(fx, tmp_path):
    """One-rank gloo group on CPU totals: SUM over one rank is the identity, and the MAX / -MIN rule returns each extreme with its sign."""
    import torch.distributed as dist
    x = fx["rows64"]
    own = not dist.is_initialized()
    if own:
        dist.init_process_group("gloo", store=dist.FileStore(str(tmp_path / "store"), 1), rank=0, world_size=1)
    try:
        st = _stats_from(x)
        gram, colsum = st.gram.clone(), st.colsum.clone()
        st.all_reduce()
        assert st.n == 672 and torch.equal(st.gram, gram) and torch.equal(st.colsum, colsum)
        coef, _ = _second_pass(st.fit(16), x)
        want = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in coef.state_dict().items()}
        assert (want["extreme"] > 0).any() and (want["extreme"] < 0).any()
        coef.all_reduce()
        got = coef.state_dict()
        assert got["n"] == 672 and all(torch.equal(got[k], want[k]) for k in ("sum", "sumsq", "extreme"))
    finally:
        if own:
            dist.destroy_process_group()


def test_fit_tool_prints_its_usage():
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "fit_token_stats.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "--out" in out.stdout and "--components" in out.stdout


def test_update_refuses_cpu_tokens(fx):
    from tokensgen_amd.token_stats import TokenStats
    with pytest.raises(RuntimeError, match="GPU"):
        TokenStats(128, "cpu").update(fx["tokens"], fx["valid_chunks"])
    coef = _stats_from(fx["rows64"]).fit(16)
    with pytest.raises(RuntimeError, match="GPU"):
        coef.update(fx["tokens"], fx["valid_chunks"])


def test_new_exports_validate_their_arguments_without_a_launch():
    import ctypes
    from tokensgen_amd import lib as L
    lib = L.load()
    F = lib.tg_gram_fold_rows()
    assert 1 <= F <= 512
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf) + (16 - ctypes.addressof(buf) % 16)
    assert lib.tg_gram_accumulate(None, 128, 1, 128, p, p, None) == -1
    for rows, D, ldx in ((1, 192, 192), (1, 64, 64), (1, 4224, 4224), (0, 128, 128), (1, 128, 120)):
        assert lib.tg_gram_accumulate(p, ldx, rows, D, p, p, None) == -2, (rows, D, ldx)
    assert lib.tg_gram_accumulate(p, 132, 1, 128, p, p, None) == -3 and lib.tg_gram_accumulate(p + 2, 128, 1, 128, p, p, None) == -3
    for nc in (0, 8, 24, 80):
        assert lib.tg_pca_coef_stats(p, 128, 1, 128, p, nc, p, p, p, p, p, None) == -2, nc
    assert lib.tg_pca_coef_stats(p, 128, 1, 128, p, 16, p, p, p, None, p, None) == -1
    assert lib.tg_pca_coef_stats_ws_floats(1, 16) > 0 and lib.tg_pca_coef_stats_ws_floats(385, 64) >= lib.tg_pca_coef_stats_ws_floats(1, 64)
