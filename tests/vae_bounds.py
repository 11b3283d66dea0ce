"""fp64 CPU references, DERIVED per-element bounds and the shape lists for the VAE convolution kernels (tg_conv3d_cl's eight kernels and
tg_conv3d_up2_subpixel).  The references are written from the formula in the header comment of tg_conv3d_cl (include/tokensgen_hip.h), independently of
oracle/vae_ref.py:
    tv = to + dt - (kt-1)         tv < 0 reads cache frame kt-1+tv, or frame 0 when there is no cache
    hv = ho*stride + dh - pad     zero outside [0, H*up); wv likewise
    xv(t, h, w) = x[t_map[t]][h/up][w/up]
The arithmetic is the GEMM's — fp32 accumulation over K = kt kh kw Cin products, one bf16 store — so the bounds are edge_bounds' (no measured figure):
    plain      E.gemm_bias_bound(lin, mag, K)
    residual   E.gemm_gate_res(lin, mag, res, gate = 1, K, rounded_linear=True)      every kernel documents bf16(bf16(conv) + residual)
    split-K    the same with K + 8                                                   at most 8 fp32 partial tensors are added
tests/test_vae_bounds_cpu.py pins that each bound is satisfiable and sharp and that every shape below takes the kernel it was written for;
tests/test_vae_edges_gpu.py holds the kernels to them.  All shapes are for 256 CUs (what tg_device_cus() answers without a device, and the MI355X)."""
import functools
import zlib
from typing import NamedTuple, Optional

import torch

import edge_bounds as E
from tokensgen_amd import lib as L

BF, F64 = torch.bfloat16, torch.float64
HALO2, W4_ON = ("TG_CONV_HALO", 2), ("TG_CONV_W4", 2)


class Case(NamedTuple):
    kernel: int                      # lib.CONV_*: the kernel the case was written for
    cin: int
    cout: int
    cout_pad: int
    k: tuple                         # (kt, kh, kw)
    dims: tuple                      # (T, H, W) of x
    stride: int = 1
    pad: int = 1
    up: int = 1
    tmap: Optional[tuple] = None     # frame index map (time doubling), To entries
    out_dims: Optional[tuple] = None
    cache: bool = False
    res: bool = False
    gn: bool = False
    knob: Optional[tuple] = None     # (name, value) set through lib.debug_set for the launch
    ksplit: tuple = (1, 0)           # (ksplit, reduce template) of a CONV_128_SPLITK launch

    @property
    def odims(self):
        return self.out_dims if self.out_dims is not None else self.dims

    @property
    def M(self):
        To, Ho, Wo = self.odims
        return To * Ho * Wo

    @property
    def K(self):
        """terms of one output's sum: 81 real ones for the 8-channel input convolution"""
        kt, kh, kw = self.k
        return kt * kh * kw * (3 if self.cin == 8 else self.cin)

    @property
    def what(self):
        f = "".join(c for c, on in (("c", self.cache), ("r", self.res), ("g", self.gn)) if on)
        return (f"{self.cin}->{self.cout} k{''.join(map(str, self.k))} {'x'.join(map(str, self.dims))} s{self.stride}u{self.up}"
                f"{'t' if self.tmap else ''} M{self.M}{' ' + f if f else ''}")

    def query(self):
        """keyword arguments of lib.conv3d_kernel / lib.conv3d_splitk_plan"""
        T, H, W = self.dims
        kt, kh, kw = self.k
        return dict(T=T, H=H, W=W, Cin=self.cin, cout=self.cout, cout_pad=self.cout_pad, kt=kt, kh=kh, kw=kw, stride=self.stride, pad=self.pad, up=self.up,
                    out_dims=self.out_dims, t_map=self.tmap is not None, residual=self.res, gn_partial=self.gn)


class knob:
    """with knob(case.knob): the TG_CONV_HALO / TG_CONV_W4 override of a case, restored on the way out"""

    def __init__(self, setting):
        self.setting = setting

    def __enter__(self):
        self.old = L.debug_set(*self.setting) if self.setting else None

    def __exit__(self, *exc):
        if self.setting:
            L.debug_set(self.setting[0], self.old)


def time_double_idx(T):
    """CogVideoXUpsample3D's nearest x2 in time: every frame twice, except the first of an odd count > 1"""
    if T == 1:
        return (0,)
    return tuple([0] + [t for t in range(1, T) for _ in (0, 1)]) if T % 2 else tuple(t for t in range(T) for _ in (0, 1))


# ------------------------------------------------------------ the shape lists ------------------------------------------------------------
K333, K133, K111 = (3, 3, 3), (1, 3, 3), (1, 1, 1)
CRG = [dict(cache=True), dict(), dict(cache=True, res=True)]            # with a cache, without a cache, with a residual
PATCH_HW = [(1, 1), (15, 31), (16, 32), (17, 33), (16, 33)]             # inside, exactly on and one past the 16 x 32 patch, in each direction


def _k128():
    out = []
    for dims in [(1, 1, 1), (1, 127, 1), (2, 8, 8), (1, 3, 43), (3, 5, 17)]:                       # M = 1, 127, 128, 129, 255; nk = 27 < 32: no split-K
        out += [Case(L.CONV_128, 64, 128, 128, K333, dims, **v) for v in CRG]
    out += [Case(L.CONV_128, 64, 256, 256, K333, (257, 1, 1), **v) for v in CRG]                   # two column tiles, ragged third row tile
    out += [Case(L.CONV_128, 64, 128, 128, K333, (3, 5, 17), cache=True, res=True, gn=True),
            Case(L.CONV_128, 64, 256, 256, K333, (257, 1, 1), gn=True)]
    for T in (3, 2):                                                                                # kt = 1, up = 2, both parities of the time doubling
        idx = time_double_idx(T)
        out.append(Case(L.CONV_128, 64, 128, 128, K133, (T, 5, 6), up=2, tmap=idx, out_dims=(len(idx), 10, 12), gn=T == 3))
    for H, W in ((8, 12), (7, 11)):                                                                 # stride 2, pad 0 with the (0, 1, 0, 1) zero pad implied: even and odd H, W
        out.append(Case(L.CONV_128, 64, 128, 128, K133, (2, H, W), stride=2, pad=0, out_dims=(2, (H - 2) // 2 + 1, (W - 2) // 2 + 1), res=H == 7))
    out += [Case(L.CONV_128, 128, 256, 256, K111, (1, 9, 15), pad=0), Case(L.CONV_128, 128, 256, 256, K111, (1, 9, 15), pad=0, res=True, gn=True)]
    return out


def _splitk():
    RG = [dict(), dict(res=True, gn=True)]
    out = []
    for cin, cout, k, dims, ks in [(256, 128, K333, (1, 3, 43), (8, 8)),          # M 129, nk 108
                                   (128, 128, K333, (2, 6, 8), (6, 0)),           # M 96, nk 54: the generic reduce loop
                                   (256, 512, K133, (1, 8, 12), (4, 4)),          # M 96, nk 36
                                   # the issue's 256 -> 512 at M 5505 has 44 tiles of 256 x 256 >= 256 / 8 CUs: the plan gives it to the 4-wave kernel, as it does every
                                   # shape with 171 .. 255 tiles and 256 | cout.  Same edge — 171 tiles, 2 * 256 / 171 floors to 2 — at 128 output channels: 171 row tiles
                                   (256, 128, K133, (1, 120, 182), (2, 2)),       # M 21840, nk 36
                                   (256, 128, K333, (1, 1, 1), (8, 8)), (256, 128, K333, (1, 127, 1), (8, 8))]:
        out += [Case(L.CONV_128_SPLITK, cin, cout, cout, k, dims, ksplit=ks, **v) for v in RG]
    out.append(Case(L.CONV_128_SPLITK, 256, 128, 128, K333, (1, 3, 43), ksplit=(8, 8), cache=True))
    return out


def _n16():
    out = []
    for cin, cout, cp in [(128, 3, 16), (64, 32, 32), (64, 100, 112)]:          # cout 3: scalar stores; the other two: 8-byte stores
        for i, dims in enumerate([(1, 1, 1), (1, 127, 1), (2, 8, 8), (1, 3, 43)]):
            out += [Case(L.CONV_N16, cin, cout, cp, K333, dims, cache=i % 2 == 0), Case(L.CONV_N16, cin, cout, cp, K333, dims, cache=i % 2 == 1, res=True)]
    return out


def _in8():
    out = []
    for H, W in PATCH_HW:
        for T in (1, 2, 3):
            patches, rows = T * -(-H // 16) * -(-W // 32), -(-T * H * W // 128)
            out += [Case(L.CONV_IN8, 8, 128, 128, K333, (T, H, W), cache=c, gn=patches <= rows) for c in (True, False)]     # the sums wherever the plan accepts them
    return out


def _halo2():
    out = []
    for cin, cout in [(64, 128), (128, 128), (256, 128), (64, 256)]:            # 1, 2 and 4 channel chunks; two slabs per patch
        for H, W in PATCH_HW:
            T = 1 if (H, W) == (1, 1) else 3                                    # the plan needs patches <= rows of 128 voxels <= 4 patches
            out += [Case(L.CONV_HALO2, cin, cout, cout, K333, (T, H, W), cache=True, res=True, gn=True, knob=HALO2),
                    Case(L.CONV_HALO2, cin, cout, cout, K333, (1, H, W), knob=HALO2),
                    Case(L.CONV_HALO2, cin, cout, cout, K133, (T, H, W), gn=True, knob=HALO2)]
    return out


def _halo_narrow():
    return [Case(L.CONV_HALO_NARROW, 128, cout, 16, K333, (T, H, W), cache=c, knob=HALO2)
            for cout in (1, 3, 4) for H, W in PATCH_HW for T in (1, 3) for c in (True, False)]


def _w4_256():
    W = dict(knob=W4_ON)
    out = []
    for i, dims in enumerate([(2, 16, 32), (1, 25, 41), (3, 7, 61)]):                            # M = 1024, 1025, 1281
        out += [Case(L.CONV_W4_256, 64, 256, 256, K333, dims, **v, **W) for v in (CRG[i % 2], dict(cache=True, res=True, gn=True))]
    out += [Case(L.CONV_W4_256, 64, 512, 512, K333, (1, 25, 41), gn=True, **W),                   # two column tiles
            Case(L.CONV_W4_256, 256, 256, 256, K111, (1, 25, 41), pad=0, **W),                    # nk = 4: the shortest reduction the plan admits
            Case(L.CONV_W4_256, 320, 256, 256, K111, (1, 25, 41), pad=0, res=True, gn=True, **W),  # nk = 5
            Case(L.CONV_W4_256, 64, 256, 256, K133, (2, 13, 20), up=2, out_dims=(2, 26, 40), gn=True, **W),
            Case(L.CONV_W4_256, 64, 256, 256, K133, (1, 65, 65), stride=2, pad=0, out_dims=(1, 32, 32), res=True, **W),
            Case(L.CONV_W4_256, 64, 256, 256, K133, (1, 64, 66), stride=2, pad=0, out_dims=(1, 32, 33), **W)]
    return out


def _w4_128():
    W = dict(knob=W4_ON)
    out = []
    for i, dims in enumerate([(1, 32, 64), (1, 3, 683), (3, 1, 853), (1, 13, 197)]):              # M = 2048, 2049, 2559, 2561: on and beside the 512-row tile edges
        out += [Case(L.CONV_W4_128, 64, 128, 128, K333, dims, cache=True, res=i % 2 == 1, gn=i % 2 == 0, **W),
                Case(L.CONV_W4_128, 64, 128, 128, K133, dims, res=i % 2 == 0, gn=i % 2 == 1, **W)]
    out += [Case(L.CONV_W4_128, 64, 128, 128, K333, (3, 1, 853), **W),                             # three frames without a cache: frame 0 replicated
            Case(L.CONV_W4_128, 256, 128, 128, K111, (1, 3, 683), pad=0, **W),                     # the decoder's last 256 -> 128 shortcut (vae.py: _resnet) at full size
            Case(L.CONV_W4_128, 256, 128, 128, K111, (1, 3, 683), pad=0, res=True, gn=True, **W)]
    return out


CASES = {"k128": _k128(), "splitk": _splitk(), "n16": _n16(), "in8": _in8(), "halo2": _halo2(), "halo_narrow": _halo_narrow(), "w4_256": _w4_256(),
         "w4_128": _w4_128()}

# tg_conv3d_up2_subpixel: (Cin, cout, (T, H, W), time_x2).  (1, 43, 42): the smallest M with 32 tile-phases for 256 channels
UP2_CASES = [(64, 512, (1, 32, 32), False), (64, 512, (1, 25, 41), False), (64, 512, (3, 19, 18), False), (64, 512, (3, 19, 18), True), (64, 512, (2, 23, 23), True),
             (128, 256, (1, 43, 42), False)]

# the position-detecting test: one ragged shape per kernel, every tap of its footprint
POSITION = {"k128": Case(L.CONV_128, 64, 128, 128, K333, (3, 5, 17)),
            "splitk": Case(L.CONV_128_SPLITK, 256, 128, 128, K333, (1, 3, 43), ksplit=(8, 8)),
            "n16": Case(L.CONV_N16, 64, 100, 112, K333, (1, 3, 43)),
            "in8": Case(L.CONV_IN8, 8, 128, 128, K333, (3, 17, 33)),
            "halo2": Case(L.CONV_HALO2, 64, 128, 128, K333, (3, 17, 33), knob=HALO2),
            "halo_narrow": Case(L.CONV_HALO_NARROW, 128, 4, 16, K333, (3, 17, 33), knob=HALO2),
            "w4_256": Case(L.CONV_W4_256, 64, 256, 256, K333, (3, 7, 61), knob=W4_ON),
            "w4_128": Case(L.CONV_W4_128, 64, 128, 128, K333, (3, 1, 853), knob=W4_ON)}
UP2_POSITION = (64, 512, (1, 25, 41))


# ------------------------------------------------------------ inputs ------------------------------------------------------------
def _gen(case, salt):
    return torch.Generator().manual_seed(zlib.crc32(repr((case.cin, case.cout, case.k, case.dims, case.stride, case.up, case.tmap, salt)).encode()))


def make_inputs(case):
    """Seeded CPU bf16 inputs: x ~ randn, w ~ 0.05 randn (torch layout [cout, cin, kt, kh, kw]), bias ~ randn; cache and residual whether or not the case uses them
    (the variants of one shape share inputs and reference).  Cin = 8: w has the 3 real input channels, channels 3..7 of x and cache are finite and NOT zero."""
    T, H, W = case.dims
    kt, kh, kw = case.k
    r = lambda salt, *shape: torch.randn(*shape, generator=_gen(case, salt))
    return dict(x=r("x", T, H, W, case.cin).to(BF), w=(0.05 * r("w", case.cout, 3 if case.cin == 8 else case.cin, kt, kh, kw)).to(BF), bias=r("b", case.cout).to(BF),
                cache=r("c", kt - 1, H, W, case.cin).to(BF) if kt > 1 else None, res=r("r", *case.odims, case.cout).to(BF))


def pack(case, w):
    """[cout, cin, kt, kh, kw] -> tg_conv3d_cl's [cout_pad][kt kh kw][Cin], zero rows above cout; Cin = 8: the product's own [128][96] packing"""
    if case.cin == 8:
        from tokensgen_amd.vae import pack_conv_in_k96
        return pack_conv_in_k96(w)
    co, ci = w.shape[:2]
    p = torch.zeros(case.cout_pad, w[0, 0].numel(), case.cin, dtype=BF)
    p[:co, :, :ci] = w.reshape(co, ci, -1).permute(0, 2, 1)
    return p.contiguous()


# ------------------------------------------------------------ references ------------------------------------------------------------
def conv_ref(x, w, bias, k, cache=None, stride=1, pad=1, up=1, tmap=None, out_dims=None):
    """(lin, mag) fp64 [To, Ho, Wo, cout]: the header's sum, and the same sum over |x|, |w| plus |bias|.  x [T, H, W, C], w [cout, C, kt, kh, kw], cache [kt-1, H, W, C].
    The virtual input (time-mapped, upsampled, cache or frame 0 in front, zeros around) is built once; every tap is then one strided slice and one matmul."""
    x, w = E.d(x), E.d(w)
    kt, kh, kw = k
    T, H, W, C = x.shape
    To, Ho, Wo = out_dims if out_dims is not None else (T, H, W)
    xv = x if tmap is None else x[torch.tensor(tmap)]
    assert xv.shape[0] == To
    front = E.d(cache) if cache is not None else xv[:1].expand(kt - 1, -1, -1, -1)       # frames -(kt-1) .. -1: cache frame kt-1+tv, or frame 0
    xv = torch.cat([front, xv], 0) if kt > 1 else xv
    if up == 2:
        xv = xv.repeat_interleave(2, 1).repeat_interleave(2, 2)                          # xv(h, w) = x[h / 2][w / 2]
    Hv, Wv = H * up, W * up
    hi_h, hi_w = max(0, (Ho - 1) * stride + kh - 1 - pad - (Hv - 1)), max(0, (Wo - 1) * stride + kw - 1 - pad - (Wv - 1))
    P = torch.zeros(xv.shape[0], pad + Hv + hi_h, pad + Wv + hi_w, C, dtype=F64)         # index hv + pad, wv + pad
    P[:, pad:pad + Hv, pad:pad + Wv] = xv
    cout = w.shape[0]
    lin, mag = torch.zeros(To * Ho * Wo, cout, dtype=F64), torch.zeros(To * Ho * Wo, cout, dtype=F64)
    for dt in range(kt):
        for dh in range(kh):
            for dw in range(kw):
                a = P[dt:dt + To, dh:dh + (Ho - 1) * stride + 1:stride, dw:dw + (Wo - 1) * stride + 1:stride].reshape(-1, C)
                wt = w[:, :, dt, dh, dw].T
                lin += a @ wt
                mag += a.abs() @ wt.abs()
    if bias is not None:
        lin, mag = lin + E.d(bias), mag + E.d(bias).abs()
    return lin.view(To, Ho, Wo, cout), mag.view(To, Ho, Wo, cout)


@functools.lru_cache(maxsize=8)
def _lin_mag(case):
    i = make_inputs(case)
    c3 = (lambda t: t[..., :3]) if case.cin == 8 else (lambda t: t)          # the 8-channel input convolution uses channels 0..2
    return conv_ref(c3(i["x"]), i["w"], i["bias"], case.k, c3(i["cache"]) if case.cache else None, case.stride, case.pad, case.up, case.tmap, case.out_dims)


def reference(case):
    """(ref, bound) fp64 [To, Ho, Wo, cout] of a case on make_inputs(case); the variants of one shape that differ in residual / sums / knob share the convolution"""
    lin, mag = _lin_mag(case._replace(res=False, gn=False, knob=None, kernel=0, ksplit=(1, 0), cout_pad=0))
    K = case.K + (8 if case.kernel == L.CONV_128_SPLITK else 0)
    if case.res:
        return E.gemm_gate_res(lin, mag, make_inputs(case)["res"], torch.ones((), dtype=F64), K, rounded_linear=True)
    return lin, E.gemm_bias_bound(lin, mag, K)


def up2_out_frames(T, time_x2):
    return time_double_idx(T) if time_x2 and T > 1 else tuple(range(T))


def up2_ref(x, w_phases, bias, time_x2=False):
    """tg_conv3d_up2_subpixel's four-phase formula in fp64 on the already pre-summed bf16 w_phases [4][cout][4][Cin] (vae.pack_up2_phases):
        y[t][2 yl + py][2 xl + px][n] = bias[n] + sum_{a, b, c} w_phases[py*2+px][n][a*2+b][c] x[t][yl + a - (1 - py)][xl + b - (1 - px)][c]      (zero outside the image)
    -> (lin, mag) [To, 2H, 2W, cout]; time_x2: every frame stored twice, the first of an odd count once."""
    x, wp = E.d(x), E.d(w_phases)
    T, H, W, C = x.shape
    cout = wp.shape[1]
    P = torch.zeros(T, H + 2, W + 2, C, dtype=F64)                        # index y + 1, x + 1
    P[:, 1:H + 1, 1:W + 1] = x
    lin, mag = torch.zeros(T, 2 * H, 2 * W, cout, dtype=F64), torch.zeros(T, 2 * H, 2 * W, cout, dtype=F64)
    for py in range(2):
        for px in range(2):
            l, m = torch.zeros(T * H * W, cout, dtype=F64), torch.zeros(T * H * W, cout, dtype=F64)
            for a in range(2):
                for b in range(2):
                    s = P[:, a + py:a + py + H, b + px:b + px + W].reshape(-1, C)        # row yl + a - (1 - py) sits at index yl + a + py
                    wt = wp[py * 2 + px, :, a * 2 + b].T
                    l += s @ wt
                    m += s.abs() @ wt.abs()
            lin[:, py::2, px::2], mag[:, py::2, px::2] = l.view(T, H, W, cout), m.view(T, H, W, cout)
    if bias is not None:
        lin, mag = lin + E.d(bias), mag + E.d(bias).abs()
    idx = torch.tensor(up2_out_frames(T, time_x2))
    return lin[idx], mag[idx]


# ------------------------------------------------------------ fused GroupNorm sums ------------------------------------------------------------
def gn_sums_check(partial, y, cout):
    """The fused sums against the tensor the same launch stored.  partial: fp32 rows of [2][32] (sum, sum of squares per GroupNorm(32) group); y: the stored bf16
    values [..., cout].  Per group, the sum over ALL rows (formed here in fp64) against the fp64 sums of y:
        bound = n 2^-23 sum |v|      (sum v^2 for the squares),     n = 512 (cout / 32): the most values one row can hold (a 16 x 32 patch of the halo kernels)
    -> (worst ratio of the sums, worst ratio of the sums of squares).  A row the launch left unwritten (the caller pre-fills with NaN) gives inf."""
    rows = E.d(partial).view(-1, 2, 32).sum(0)
    g = E.d(y).reshape(-1, 32, cout // 32)
    n = 512 * (cout // 32)
    s, a, q = g.sum((0, 2)), g.abs().sum((0, 2)), (g * g).sum((0, 2))
    return E.check(rows[0], s, n * 2.0 ** -23 * a)[0], E.check(rows[1], q, n * 2.0 ** -23 * q)[0]


# ------------------------------------------------------------ position-detecting, exact ------------------------------------------------------------
def position_input(frames, H, W, C, t0=0):
    """small integers that encode (t, h, w, c), exact in bf16: (7 t + 3 h + 5 w + c) % 251 - 125; t counts from t0 (cache frames: t0 = -(kt-1))"""
    t, h, w, c = torch.meshgrid(torch.arange(t0, t0 + frames), torch.arange(H), torch.arange(W), torch.arange(C), indexing="ij")
    return ((7 * t + 3 * h + 5 * w + c) % 251 - 125).to(BF)


def identity_weight(cout, cin, k, tap):
    """[cout, cin, kt, kh, kw]: the channel identity on one tap (dt, dh, dw), zero elsewhere"""
    w = torch.zeros(cout, cin, *k, dtype=BF)
    n = torch.arange(min(cout, cin))
    w[n, n, tap[0], tap[1], tap[2]] = 1.0
    return w


def shift_expected(x, cache, tap, k, cout, stride=1, pad=1, up=1, tmap=None, out_dims=None):
    """What identity_weight(tap) with zero bias must give, by index arithmetic alone: the input shifted by the tap — zero where the tap leaves the image, frame 0
    or cache frame kt-1+tv where it leaves the window in time, zero in the channels >= Cin."""
    T, H, W, C = x.shape
    To, Ho, Wo = out_dims if out_dims is not None else (T, H, W)
    dt, dh, dw = tap
    n = min(C, cout)
    out = torch.zeros(To, Ho, Wo, cout, dtype=BF)
    hv, wv = torch.arange(Ho) * stride + dh - pad, torch.arange(Wo) * stride + dw - pad
    hin, win = (hv >= 0) & (hv < H * up), (wv >= 0) & (wv < W * up)
    for to in range(To):
        tv = to + dt - (k[0] - 1)
        if tv < 0 and cache is not None:
            frame = cache[k[0] - 1 + tv]
        else:
            tv = max(tv, 0)
            frame = x[tmap[tv] if tmap is not None else tv]
        sub = frame[(hv[hin] // up)][:, (wv[win] // up)]
        out[to, hin.nonzero()[:, 0, None], win.nonzero()[None, :, 0], :n] = sub[..., :n]
    return out


def up2_identity_phases(cout, cin, phase, tap):
    """w_phases [4][cout][4][cin] that selects tap a*2+b of phase py*2+px with the channel identity"""
    w = torch.zeros(4, cout, 4, cin, dtype=BF)
    n = torch.arange(min(cout, cin))
    w[phase, n, tap, n] = 1.0
    return w


def up2_shift_expected(x, phase, tap, cout):
    """y[t][2 yl + py][2 xl + px][c] = x[t][yl + a - (1 - py)][xl + b - (1 - px)][c] on the selected phase (zero outside the image), zero on the other three"""
    T, H, W, C = x.shape
    py, px, a, b = phase >> 1, phase & 1, tap >> 1, tap & 1
    out = torch.zeros(T, 2 * H, 2 * W, cout, dtype=BF)
    ys, xs = torch.arange(H) + a - (1 - py), torch.arange(W) + b - (1 - px)
    yin, xin = (ys >= 0) & (ys < H), (xs >= 0) & (xs < W)
    n = min(C, cout)
    sub = x[:, ys[yin]][:, :, xs[xin]]
    out[:, (2 * torch.arange(H)[yin] + py)[:, None], (2 * torch.arange(W)[xin] + px)[None, :], :n] = sub[..., :n]
    return out
