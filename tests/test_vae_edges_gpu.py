"""GPU: the VAE convolution kernels PER ELEMENT against fp64 (tests/vae_bounds.py: references written from the header's formula, bounds derived from the documented
arithmetic, no measured figure) at the dispatch and tile edges the norm-based tests of test_vae_gpu.py average away: one test function per kernel of tg_conv3d_cl
(conv_plan.h: CONV_128, CONV_128_SPLITK and its reduce, CONV_N16, CONV_IN8, CONV_HALO2, CONV_HALO_NARROW, CONV_W4_256, CONV_W4_128) and one for
tg_conv3d_up2_subpixel, then one exact position-detecting test over every tap of every kernel.

Every case asks tg_conv3d_kernel, before its launch, that the shape takes the kernel it was written for (TG_CONV_HALO / TG_CONV_W4 switched through lib.debug_set and
restored; TG_CONV_SPLITK left alone).  Every launch goes through the C ABI directly: the output is a column slice of a wider buffer — row stride ldy = cout + 8, the
slice at column 4, one row before and one after — whose frame is sentinel-filled and checked untouched (for cout = 3 padded to 16 this is where a store of the padding
would land) and whose inside is NaN-filled (an unwritten voxel is a non-finite output); the residual has the same row stride; the GroupNorm partial buffer is NaN-filled
too: every row its consumer reads must have been written.  Every case runs twice and must repeat bitwise.  Every numeric check goes through edge_bounds.check (ALL
elements) and is recorded as parity(worst error / bound, 1.0, what)."""
import pytest
import torch

import edge_bounds as E
import vae_bounds as V
from tokensgen_amd import lib as L

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
NAN, SENTINEL, COL0, FRAME_COLS = float("nan"), 9.0, 4, 8


@pytest.fixture(scope="module")
def K():
    from tokensgen_amd import kernels
    return kernels


@pytest.fixture(autouse=True)
def _nothing_runs_after_a_gpu_fault():
    """A failed assertion lets the next test run; a GPU fault (the runtime reports it at the next synchronisation) ends the session: nothing more is launched on that device."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU fault, stopping the run: {e}", returncode=3)


def _framed(M, cout, inside=NAN):
    """([M + 2, cout + 8] buffer filled with the sentinel, its [M, cout] view at row 1, column 4 filled with `inside`)"""
    full = torch.full((M + 2, cout + FRAME_COLS), SENTINEL, dtype=BF, device=DEV)
    view = full[1:1 + M, COL0:COL0 + cout]
    view.copy_(inside.reshape(M, cout).to(DEV)) if isinstance(inside, torch.Tensor) else view.fill_(inside)
    return full, view


def _frame_untouched(full, M, cout):
    return bool((full[0] == SENTINEL).all() and (full[M + 1] == SENTINEL).all() and (full[:, :COL0] == SENTINEL).all() and (full[:, COL0 + cout:] == SENTINEL).all())


def _ptr(t):
    return None if t is None else t.data_ptr()


def _launch(K, case, x, wp, bias, cache, res):
    """One tg_conv3d_cl call on device tensors -> (the framed buffer, its [M, cout] view, the GroupNorm partial buffer or None)"""
    T, H, W = case.dims
    kt, kh, kw = case.k
    To, Ho, Wo = case.odims
    so = L.load()
    full, y = _framed(case.M, case.cout)
    partial = torch.full((so.tg_conv3d_gn_partial_floats(To, Ho, Wo),), NAN, dtype=F32, device=DEV) if case.gn else None
    nws = so.tg_conv3d_splitk_floats(case.cin, case.cout, case.cout_pad, kt, kh, kw, To, Ho, Wo)
    assert (nws > 0) == (case.kernel == L.CONV_128_SPLITK) or case.knob is not None      # (the workspace size ignores the halo / w4 knobs: conv_plan.h)
    ws = torch.empty(nws, dtype=F32, device=DEV) if nws else None
    tmap = torch.tensor(case.tmap, dtype=torch.int32, device=DEV) if case.tmap is not None else None
    L.check(so.tg_conv3d_cl(_ptr(x), T, H, W, case.cin, _ptr(cache), _ptr(wp), _ptr(bias), case.cout, case.cout_pad, kt, kh, kw, case.stride, case.pad, case.up,
                            _ptr(tmap), _ptr(res), _ptr(y), y.stride(0), To, Ho, Wo, _ptr(K.zero_page(torch.device(DEV, torch.cuda.current_device()))), _ptr(partial),
                            _ptr(ws), torch.cuda.current_stream().cuda_stream), "tg_conv3d_cl")
    return full, y, partial


def _run_twice(K, case, x, w, bias, cache, res):
    """Asks the plan, launches twice -> (y [To, Ho, Wo, cout] on the CPU, partial, what went wrong: a touched frame, a rerun that is not bitwise equal)"""
    with V.knob(case.knob):
        assert L.conv3d_kernel(**case.query()) == case.kernel and L.conv3d_splitk_plan(**case.query()) == case.ksplit, case.what
        xd, wd, bd = x.to(DEV), V.pack(case, w).to(DEV), bias.to(DEV) if bias is not None else None
        cd = cache.to(DEV) if cache is not None else None
        rfull, rd = _framed(case.M, case.cout, res) if res is not None else (None, None)
        runs = [_launch(K, case, xd, wd, bd, cd, rd) for _ in range(2)]
        torch.cuda.synchronize()
    wrong = [f"{case.what}: a store outside the [M, cout] output" for full, _, _ in runs if not _frame_untouched(full, case.M, case.cout)]
    (_, y, partial), (_, y2, partial2) = runs
    if not torch.equal(y.view(torch.int16), y2.view(torch.int16)):
        wrong.append(f"{case.what}: not bitwise repeatable")
    if partial is not None and not torch.equal(partial.view(torch.int32), partial2.view(torch.int32)):
        wrong.append(f"{case.what}: sums not bitwise repeatable")
    return y.cpu().view(*case.odims, case.cout), partial, wrong


def _check_case(K, parity, name, case):
    i = V.make_inputs(case)
    y, partial, wrong = _run_twice(K, case, i["x"], i["w"], i["bias"], i["cache"] if case.cache else None, i["res"] if case.res else None)
    ref, bound = V.reference(case)
    worst, where = E.check(y, ref, bound)
    print(f"{name} {case.what}: {worst:.3f} at {where}, whole-tensor rel-L2 {float((y.double() - ref).norm() / ref.norm()):.2e}")
    assert not wrong, wrong
    parity(worst, 1.0, f"{name} {case.what}")
    if case.gn:
        a, b = V.gn_sums_check(partial, y, case.cout)
        parity(a, 1.0, f"{name} {case.what} GroupNorm sums")
        parity(b, 1.0, f"{name} {case.what} GroupNorm sums of squares")


def _ids(cases):
    return [c.what.replace(" ", "_") for c in cases]


@pytest.mark.parametrize("case", V.CASES["k128"], ids=_ids(V.CASES["k128"]))
def test_conv_128(case, K, parity):
    """conv3d_cl_kernel<2, 4, 4>: M on and beside the 128-voxel tile, two column tiles, the three folded forms (nearest x2 with a frame map in both parities,
    stride 2 with the implied zero pad at odd and even sizes, 1x1x1), cache / replicated first frame / residual / sums"""
    _check_case(K, parity, "conv_128", case)


@pytest.mark.parametrize("case", V.CASES["splitk"], ids=_ids(V.CASES["splitk"]))
def test_conv_128_splitk(case, K, parity):
    """conv3d_cl_kernel over K ranges + conv_splitk_reduce_kernel<8 / generic (6) / 4 / 2>: the reduce launch adds the partial tensors and runs the whole epilogue"""
    _check_case(K, parity, "conv_128_splitk", case)


@pytest.mark.parametrize("case", V.CASES["n16"], ids=_ids(V.CASES["n16"]))
def test_conv_n16(case, K, parity):
    """conv3d_cl_kernel<1, 2, 1>: 128 voxels x 16 channels; cout = 3 (scalar stores, 13 padding columns never stored), 32 and 100 of 112 (8-byte stores)"""
    _check_case(K, parity, "conv_n16", case)


@pytest.mark.parametrize("case", V.CASES["in8"], ids=_ids(V.CASES["in8"]))
def test_conv_in8(case, K, parity):
    """conv3d_in_kernel: 8-channel input (channels 3..7 finite, not zero: the reference ignores them), weights from the product's packer, 16 x 32 patches"""
    _check_case(K, parity, "conv_in8", case)


@pytest.mark.parametrize("case", V.CASES["halo2"], ids=_ids(V.CASES["halo2"]))
def test_conv_halo2(case, K, parity):
    """conv3d_halo2_kernel<8> (TG_CONV_HALO = 2): 1 / 2 / 4 channel chunks, two slabs per patch, 3x3x3 with and without a cache and 1x3x3, patches on and around 16 x 32"""
    _check_case(K, parity, "conv_halo2", case)


@pytest.mark.parametrize("case", V.CASES["halo_narrow"], ids=_ids(V.CASES["halo_narrow"]))
def test_conv_halo_narrow(case, K, parity):
    """conv3d_halo_narrow_kernel<128, 3> (TG_CONV_HALO = 2): cout 1, 3, 4 with LDS-resident weights"""
    _check_case(K, parity, "conv_halo_narrow", case)


@pytest.mark.parametrize("case", V.CASES["w4_256"], ids=_ids(V.CASES["w4_256"]))
def test_conv_w4_256(case, K, parity):
    """conv3d_w4_kernel<256> (TG_CONV_W4 = 2): M on and beside the 256-voxel tile, two column tiles, the shortest reductions (nk = 4, 5), upsampling, stride 2"""
    _check_case(K, parity, "conv_w4_256", case)


@pytest.mark.parametrize("case", V.CASES["w4_128"], ids=_ids(V.CASES["w4_128"]))
def test_conv_w4_128(case, K, parity):
    """conv3d_w4_kernel<128> (TG_CONV_W4 = 2): M on and beside the 512-voxel tile; 3x3x3, 1x3x3 and the 1x1x1, pad 0 form the decoder's last shortcut takes at full size"""
    _check_case(K, parity, "conv_w4_128", case)


@pytest.mark.parametrize("cin,cout,dims,time_x2", V.UP2_CASES, ids=[f"{ci}->{co}_{'x'.join(map(str, d))}{'_t2' if t else ''}" for ci, co, d, t in V.UP2_CASES])
def test_conv_up2_subpixel(cin, cout, dims, time_x2, K, parity):
    """tg_conv3d_up2_subpixel against the four-phase formula in fp64 on the pre-summed bf16 weights of vae.pack_up2_phases (the pre-sum's own rounding does not enter),
    each output phase against its own formula and reported separately (a swapped (py, px) shows), the four image borders too; time doubling with odd and even T; the
    fused sums over the 4 x ceil(M / 128) rows."""
    from tokensgen_amd.vae import pack_up2_phases
    T, H, W = dims
    so = L.load()
    assert so.tg_conv3d_up2_subpixel_ok(T, H, W, cin, cout) == 1
    g = torch.Generator().manual_seed(1000 * cin + cout + 7 * T + 3 * H + W)
    x, w, bias = torch.randn(T, H, W, cin, generator=g).to(BF), (0.05 * torch.randn(cout, cin, 3, 3, generator=g)).to(BF), torch.randn(cout, generator=g).to(BF)
    wp = pack_up2_phases(w)
    To = len(V.up2_out_frames(T, time_x2))
    M = To * 4 * H * W
    xd, wd, bd = x.to(DEV), wp.to(DEV), bias.to(DEV)
    runs = []
    for _ in range(2):
        full, y = _framed(M, cout)
        partial = torch.full((so.tg_conv3d_up2_subpixel_gn_floats(T, H, W),), NAN, dtype=F32, device=DEV)
        assert partial.numel() == 4 * ((T * H * W + 127) // 128) * 64
        L.check(so.tg_conv3d_up2_subpixel(_ptr(xd), T, H, W, cin, _ptr(wd), _ptr(bd), cout, _ptr(y), y.stride(0), int(time_x2),
                                          _ptr(K.zero_page(torch.device(DEV, torch.cuda.current_device()))), _ptr(partial), torch.cuda.current_stream().cuda_stream),
                "tg_conv3d_up2_subpixel")
        runs.append((full, y, partial))
    torch.cuda.synchronize()
    what = f"up2_subpixel {cin}->{cout} {T}x{H}x{W}{' time_x2' if time_x2 else ''}"
    assert all(_frame_untouched(full, M, cout) for full, _, _ in runs), what
    assert torch.equal(runs[0][1].view(torch.int16), runs[1][1].view(torch.int16)) and torch.equal(runs[0][2].view(torch.int32), runs[1][2].view(torch.int32)), what
    y = runs[0][1].cpu().view(To, 2 * H, 2 * W, cout)
    lin, mag = V.up2_ref(x, wp, bias, time_x2)
    bound = E.gemm_bias_bound(lin, mag, 4 * cin)
    for py in range(2):
        for px in range(2):
            parity(E.check(y[:, py::2, px::2], lin[:, py::2, px::2], bound[:, py::2, px::2])[0], 1.0, f"{what} phase ({py}, {px})")
    for nm, sl in (("top", (slice(None), 0)), ("bottom", (slice(None), 2 * H - 1)), ("left", (slice(None), slice(None), 0)), ("right", (slice(None), slice(None), 2 * W - 1))):
        parity(E.check(y[sl], lin[sl], bound[sl])[0], 1.0, f"{what} {nm} border")
    a, b = V.gn_sums_check(runs[0][2], y, cout)
    parity(a, 1.0, f"{what} GroupNorm sums")
    parity(b, 1.0, f"{what} GroupNorm sums of squares")


TAPS = [(dt, dh, dw) for dt in range(3) for dh in range(3) for dw in range(3)]


@pytest.mark.parametrize("tap", TAPS, ids=lambda t: "tap" + "".join(map(str, t)))
@pytest.mark.parametrize("name", sorted(V.POSITION))
def test_every_tap_reads_the_right_voxel(name, tap, K):
    """Position-detecting, exact: weights that are the channel identity on ONE tap, zero bias, an input of small integers that encode (t, h, w, c).  The output must be
    the input shifted by that tap — zero where the tap leaves the image, frame 0 (no cache) or the right cache frame where it leaves the window in time, zero in the
    output channels above Cin — with torch.equal, at each kernel's ragged shape.  A fragment stored to the wrong row of a ragged tile, a halo read off by one, two taps
    swapped or a wrong cache frame is a wrong integer, not noise.  (The 8-channel input convolution: its three real input channels to three output channels.)"""
    base = V.POSITION[name]
    T, H, W = base.dims
    cr = 3 if base.cin == 8 else base.cin
    w = V.identity_weight(base.cout, cr, base.k, tap)
    x = V.position_input(T, H, W, base.cin)
    for cached in (True, False):
        case = base._replace(cache=cached)
        cache = V.position_input(2, H, W, base.cin, t0=-2) if cached else None
        y, _, wrong = _run_twice(K, case, x, w, None, cache, None)
        assert not wrong, wrong
        want = V.shift_expected(x[..., :cr], cache[..., :cr] if cached else None, tap, base.k, base.cout)
        assert torch.equal(y, want), (name, tap, cached, (y != want).nonzero()[:4].tolist())


@pytest.mark.parametrize("tap", range(4), ids=lambda t: f"a{t >> 1}b{t & 1}")
@pytest.mark.parametrize("phase", range(4), ids=lambda p: f"py{p >> 1}px{p & 1}")
def test_every_subpixel_tap_reads_the_right_voxel(phase, tap, K):
    """The same for tg_conv3d_up2_subpixel: a w_phases that selects one of the four taps of one phase — that phase holds the input shifted by the tap's own offset,
    the other three phases are zero."""
    cin, cout, (T, H, W) = V.UP2_POSITION
    so = L.load()
    assert so.tg_conv3d_up2_subpixel_ok(T, H, W, cin, cout) == 1
    x = V.position_input(T, H, W, cin)
    xd, wd = x.to(DEV), V.up2_identity_phases(cout, cin, phase, tap).to(DEV)
    M = T * 4 * H * W
    full, y = _framed(M, cout)
    L.check(so.tg_conv3d_up2_subpixel(_ptr(xd), T, H, W, cin, _ptr(wd), None, cout, _ptr(y), y.stride(0), 0, _ptr(K.zero_page(torch.device(DEV, torch.cuda.current_device()))),
                                      None, torch.cuda.current_stream().cuda_stream), "tg_conv3d_up2_subpixel")
    torch.cuda.synchronize()
    assert _frame_untouched(full, M, cout)
    got, want = y.cpu().view(T, 2 * H, 2 * W, cout), V.up2_shift_expected(x, phase, tap, cout)
    assert torch.equal(got, want), (phase, tap, (got != want).nonzero()[:4].tolist())
