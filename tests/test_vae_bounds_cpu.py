"""CPU: the references, bounds and shape lists of tests/vae_bounds.py, with no GPU and no measured number involved.
  - each bound is satisfiable: the fp64 reference rounded ONCE to bf16 (twice where the kernels document two roundings: bf16(bf16(conv) + residual)) passes.  As
    tests/test_edge_bounds_cpu.py explains, the 2^-8 |ref| term is exactly one bf16 rounding, so the once-rounded reference reaches ratios up to 1, not 0.5, where the
    accumulation term is small; the ceiling asserted here is 1, and 0.5 for the fused GroupNorm sums (fp32 sums under a bound of many fp32 roundings);
  - each bound is sharp: the same tensor with one element moved by 2 bf16 ulps fails, at that element; sums that miss one stored value fail;
  - the references agree with direct evaluations of the header's formulas written a second way (the position-detecting expectation, exact; torch's conv3d);
  - every listed shape, under the knob setting named for it, is answered by tg_conv3d_kernel with the kernel it was written for (tg_device_cus() answers 256 without
    a device), split-K cases with the intended ksplit and reduce template."""
import pytest
import torch

import edge_bounds as E
import vae_bounds as V
from tokensgen_amd import lib as L

F64 = torch.float64
SMALL = {"plain": V.Case(L.CONV_128, 64, 128, 128, V.K333, (3, 5, 7), cache=True),
         "residual": V.Case(L.CONV_128, 64, 128, 128, V.K333, (3, 5, 7), cache=True, res=True),
         # the split-K FORMULA (K + 8 terms) on the small shape: at the shapes the plan really splits (K >= 2048) the accumulation term alone is about one bf16 ulp of
         # the largest outputs (K 2^-23 sum |x||w| against 2^-8 |sum x w|, the sum of K random signs being ~ sqrt(K) of its terms), so no bound of this form is 2-ulp sharp there
         "splitk": V.Case(L.CONV_128_SPLITK, 64, 128, 128, V.K333, (3, 5, 7), cache=True, res=True),
         "in8": V.Case(L.CONV_IN8, 8, 128, 128, V.K333, (2, 5, 7)),
         "up2": None}


def _family(name):
    """(ref, bound, the best a correct kernel can store)"""
    if name == "up2":
        from tokensgen_amd.vae import pack_up2_phases
        g = torch.Generator().manual_seed(5)
        x, w, b = (torch.randn(2, 5, 7, 64, generator=g)).to(V.BF), (0.05 * torch.randn(128, 64, 3, 3, generator=g)).to(V.BF), torch.randn(128, generator=g).to(V.BF)
        lin, mag = V.up2_ref(x, pack_up2_phases(w), b, time_x2=True)
        assert lin.shape == (4, 10, 14, 128)
        return lin, E.gemm_bias_bound(lin, mag, 4 * 64), E.round_bf16(lin)
    case = SMALL[name]
    ref, bound = V.reference(case)
    if case.res:
        lin, _ = V.reference(case._replace(res=False))
        return ref, bound, E.round_bf16(E.round_bf16(lin) + E.d(V.make_inputs(case)["res"]))
    return ref, bound, E.round_bf16(ref)


@pytest.mark.parametrize("family", sorted(SMALL))
def test_bound_is_satisfiable_and_sharp(family):
    ref, bound, best = _family(family)
    worst, _ = E.check(best, ref, bound)
    print(f"{family}: the once-rounded reference sits at {worst:.3f} of the bound")
    assert worst <= 1.0, worst
    i = int(ref.abs().argmax())
    bad = best.clone().flatten()
    away = 1.0 if bad[i] >= ref.flatten()[i] else -1.0
    bad[i] += away * 2 * E.ulp_bf16(bad[i])
    worst, where = E.check(bad.view_as(ref), ref, bound)
    assert worst > 1.0, worst
    assert where == tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ref.shape))


def test_splitk_bound_is_the_plain_one_with_eight_more_terms():
    case = V.Case(L.CONV_128_SPLITK, 128, 128, 128, V.K333, (2, 6, 8), ksplit=(6, 0))
    lin, bound = V.reference(case)
    _, plain = V.reference(case._replace(kernel=L.CONV_128))
    mag = (plain - 2.0 ** -8 * lin.abs()) / (case.K * 2.0 ** -23)
    assert case.K == 27 * 128 and torch.allclose(bound - plain, 8 * 2.0 ** -23 * mag, rtol=1e-9, atol=0) and (mag >= lin.abs() * (1 - 1e-12)).all()


def test_gn_sums_bound_is_satisfiable_and_sharp():
    """fp32 row sums of the stored values pass at <= 0.5; a row list that misses ONE stored value fails (at this size: 516 values per group — the bound is
    n 2^-23 = 2^-12 of sum |v| for 128 channels, so it sees a missing value among up to a few thousand, and a missing row or patch at any size)."""
    cout, M = 128, 129
    y = torch.randn(M, cout, generator=torch.Generator().manual_seed(3)).to(V.BF)
    g = E.d(y).reshape(-1, 32, cout // 32)
    rows = torch.zeros(2, 2, 32, dtype=torch.float32)
    for r, sl in enumerate((slice(0, 128), slice(128, M))):
        rows[r, 0], rows[r, 1] = g[sl].sum((0, 2)).float(), (g[sl] * g[sl]).sum((0, 2)).float()
    a, b = V.gn_sums_check(rows, y, cout)
    assert a <= 0.5 and b <= 0.5, (a, b)
    v = g[128, 7, 2]
    bad = rows.clone()
    bad[1, 0, 7] -= float(v)
    bad[1, 1, 7] -= float(v * v)
    a, b = V.gn_sums_check(bad, y, cout)
    assert a > 1.0 and b > 1.0, (a, b, float(v))
    bad = rows.clone()
    bad[1] = float("nan")                                 # a row the launch never wrote
    assert V.gn_sums_check(bad, y, cout) == (float("inf"), float("inf"))


def _torch_conv(x, w, bias, k, cache):
    """F.conv3d on cat(cache or frame 0, x) with the spatial zero padding: the header's formula for stride 1, pad 1, up 1, a second way (fp64)"""
    xv = torch.cat([E.d(cache) if cache is not None else E.d(x)[:1].expand(k[0] - 1, -1, -1, -1), E.d(x)], 0)
    y = torch.nn.functional.conv3d(xv.permute(3, 0, 1, 2)[None], E.d(w), E.d(bias), padding=(0, 1, 1))
    return y[0].permute(1, 2, 3, 0)


@pytest.mark.parametrize("cache", [True, False])
def test_conv_ref_equals_torch_conv3d(cache):
    case = SMALL["plain"]._replace(cache=cache)
    i = V.make_inputs(case)
    lin = V.reference(case)[0]
    want = _torch_conv(i["x"], i["w"], i["bias"], case.k, i["cache"] if cache else None)
    assert (lin - want).abs().max() <= 1e-12 * want.abs().max()
    case = SMALL["in8"]._replace(cache=cache)                # the reference ignores channels 3..7 (finite, not zero)
    i = V.make_inputs(case)
    assert (i["x"][..., 3:] != 0).any()
    want = _torch_conv(i["x"][..., :3], i["w"], i["bias"], case.k, i["cache"][..., :3] if cache else None)
    assert (V.reference(case)[0] - want).abs().max() <= 1e-12 * want.abs().max()


FOLDED = [V.Case(0, 64, 128, 128, V.K333, (3, 5, 7), cache=True), V.Case(0, 64, 128, 128, V.K333, (3, 5, 7)), V.Case(0, 64, 32, 32, V.K333, (1, 4, 3)),
          V.Case(0, 64, 128, 128, V.K133, (3, 5, 6), up=2, tmap=V.time_double_idx(3), out_dims=(5, 10, 12)),
          V.Case(0, 64, 128, 128, V.K133, (2, 5, 6), up=2, tmap=V.time_double_idx(2), out_dims=(4, 10, 12)),
          V.Case(0, 64, 128, 128, V.K133, (2, 8, 12), stride=2, pad=0, out_dims=(2, 4, 6)), V.Case(0, 64, 128, 128, V.K133, (2, 7, 11), stride=2, pad=0, out_dims=(2, 3, 5)),
          V.Case(0, 128, 256, 256, V.K111, (2, 3, 5), pad=0)]


@pytest.mark.parametrize("case", FOLDED, ids=lambda c: c.what)
def test_position_expectation_equals_the_fp64_reference(case):
    """Identity weights on one tap: the fp64 reference (pad, slice, matmul) and the index-arithmetic expectation agree exactly, for every tap and every folded form —
    and the expectation moves with the tap (it is not all zeros, and two different taps differ)."""
    T, H, W = case.dims
    kt, kh, kw = case.k
    x = V.position_input(T, H, W, case.cin)
    cache = V.position_input(kt - 1, H, W, case.cin, t0=-(kt - 1)) if case.cache else None
    seen = []
    for dt in range(kt):
        for dh in range(kh):
            for dw in range(kw):
                w = V.identity_weight(case.cout, case.cin, case.k, (dt, dh, dw))
                want = V.shift_expected(x, cache, (dt, dh, dw), case.k, case.cout, case.stride, case.pad, case.up, case.tmap, case.out_dims)
                lin, _ = V.conv_ref(x, w, None, case.k, cache, case.stride, case.pad, case.up, case.tmap, case.out_dims)
                assert torch.equal(lin, want.double()), (dt, dh, dw)
                assert (want[..., min(case.cin, case.cout):] == 0).all() and (want != 0).any()
                seen.append(want)
    same_frame = T == 1 and cache is None                    # one frame and no cache: every temporal tap reads frame 0
    assert all(not torch.equal(seen[i], seen[j]) for i in range(len(seen)) for j in range(i) if not (same_frame and i % (kh * kw) == j % (kh * kw)))


def test_up2_reference_and_position_expectation():
    """The four-phase reference on pack_up2_phases' weights is the 9-tap convolution on the upsampled grid up to the ONE bf16 rounding of the pre-summed weights;
    with exactly representable sums (weights that are small integers) it is that convolution exactly.  The one-tap expectation equals the reference for all 16 taps."""
    from tokensgen_amd.vae import pack_up2_phases
    g = torch.Generator().manual_seed(9)
    x = torch.randn(3, 5, 6, 64, generator=g).to(V.BF)
    w = torch.randint(-3, 4, (128, 64, 3, 3), generator=g).to(V.BF)
    b = torch.randn(128, generator=g).to(V.BF)
    lin4, _ = V.up2_ref(x, pack_up2_phases(w), b, time_x2=True)
    idx = V.time_double_idx(3)
    lin9, _ = V.conv_ref(x, w[:, :, None], b, V.K133, None, 1, 1, 2, idx, (len(idx), 10, 12))
    assert lin4.shape == lin9.shape and (lin4 - lin9).abs().max() <= 1e-12 * lin9.abs().max()
    xi = V.position_input(2, 5, 6, 64)
    seen = []
    for phase in range(4):
        for tap in range(4):
            want = V.up2_shift_expected(xi, phase, tap, 128)
            lin, _ = V.up2_ref(xi, V.up2_identity_phases(128, 64, phase, tap), None)
            assert torch.equal(lin, want.double()), (phase, tap)
            seen.append(want)
    assert all(not torch.equal(seen[i], seen[j]) for i in range(16) for j in range(i))


@pytest.mark.parametrize("name", sorted(V.CASES))
def test_the_shape_lists_sit_where_the_dispatch_changes(name):
    cases = V.CASES[name] + [V.POSITION[name], V.POSITION[name]._replace(cache=True)]
    assert len(set(V.CASES[name])) == len(V.CASES[name])
    for case in cases:
        with V.knob(case.knob):
            assert L.conv3d_kernel(**case.query()) == case.kernel, case.what
            assert L.conv3d_splitk_plan(**case.query()) == case.ksplit, case.what
        if case.knob:                                        # ... and only under the knob: by default these small shapes run another kernel
            assert L.conv3d_kernel(**case.query()) not in (case.kernel, -2), case.what
        # fp64 work of one reference (lin and mag): <= 8 GFLOP, but 26 for the one split-K shape with 171 tiles (no smaller shape reaches ksplit 2)
        assert 4 * case.M * case.K * case.cout <= (8e9 if case.ksplit != (2, 2) else 26e9) and (case.M <= 5600 or case.ksplit == (2, 2)), case.what
    if name == "in8":        # the sums wherever the plan accepts them — and nowhere else
        for case in V.CASES[name]:
            assert case.gn or L.conv3d_kernel(**case._replace(gn=True).query()) == -2, case.what
        assert sum(c.gn for c in V.CASES[name]) >= 20
    if name == "halo2":      # patches <= rows of 128 voxels <= 4 patches, checked with the query: one frame more at 1 x 1 and the plan leaves the kernel
        with V.knob(V.HALO2):
            assert L.conv3d_kernel(**V.Case(0, 64, 128, 128, V.K333, (2, 1, 1)).query()) != L.CONV_HALO2


def test_the_shape_lists_cover_the_edges():
    C = V.CASES
    assert sorted({c.M for c in C["k128"] if c.k == V.K333}) == [1, 127, 128, 129, 255, 257]
    assert {c.ksplit for c in C["splitk"]} == {(8, 8), (6, 0), (4, 4), (2, 2)} and {1, 127} <= {c.M for c in C["splitk"]}
    assert {(c.cin, c.cout, c.cout_pad) for c in C["n16"]} == {(128, 3, 16), (64, 32, 32), (64, 100, 112)} and {c.M for c in C["n16"]} == {1, 127, 128, 129}
    assert {c.dims for c in C["in8"]} == {(T, H, W) for T in (1, 2, 3) for H, W in V.PATCH_HW}
    assert {(c.cin, c.cout) for c in C["halo2"]} == {(64, 128), (128, 128), (256, 128), (64, 256)} and {c.dims[1:] for c in C["halo2"]} == set(V.PATCH_HW)
    assert {c.cout for c in C["halo_narrow"]} == {1, 3, 4} and {c.dims for c in C["halo_narrow"]} == {(T, H, W) for T in (1, 3) for H, W in V.PATCH_HW}
    assert {1024, 1025, 1281} <= {c.M for c in C["w4_256"]} and {c.k[0] * c.k[1] * c.k[2] * c.cin // 64 for c in C["w4_256"] if c.k == V.K111} == {4, 5}
    assert {2048, 2049, 2559, 2561} == {c.M for c in C["w4_128"]} and any(c.k == V.K111 and c.cin == 256 for c in C["w4_128"])
    for name, cases in C.items():                            # every kernel: a residual and fused sums somewhere (the two narrow-output kernels have neither / no sums)
        assert any(c.res for c in cases) or name in ("in8", "halo_narrow"), name
        assert any(c.gn for c in cases) or name in ("n16", "halo_narrow"), name
    for cin, cout, (T, H, W), _ in V.UP2_CASES + [V.UP2_POSITION + (False,)]:
        assert L.load().tg_conv3d_up2_subpixel_ok(T, H, W, cin, cout) == 1
    assert L.load().tg_conv3d_up2_subpixel_ok(1, 43, 41, 128, 256) == 0          # (1, 43, 42) is the smallest M with 32 tile-phases for 256 channels


def test_the_decoders_last_shortcut_is_the_1x1x1_case_of_the_512x128_kernel():
    """The 256 -> 128 conv_shortcut of the decoder's last up block (vae.py _resnet: 1x1x1, pad 0) at a full-size tile, 8 x 240 x 360, default knobs"""
    from tokensgen_amd.vae import AutoencoderKLCogVideoX
    shapes = AutoencoderKLCogVideoX(device="cpu").param_shapes()
    assert shapes["decoder.up_blocks.3.resnets.0.conv_shortcut.weight"] == (128, 256, 1, 1, 1)
    assert L.conv3d_kernel(8, 240, 360, 256, 128, 128, 1, 1, 1, pad=0) == L.CONV_W4_128
