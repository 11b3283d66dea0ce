"""CPU: the colour feature's definitions as tests/color_ref.py restates them (known L*a*b* values, both sides of every branch point, the properties of the two table
modes, the streaming bookkeeping), every refusal of tokensgen_amd.color / metrics / video_io that is raised before a device is needed, and the argument validation
of the four C entry points of csrc/color.hip (which happens before any launch)."""
import ctypes

import pytest
import torch

import color_ref as R

F64 = torch.float64


def lab_u8(*rgb):
    return R.rgb_to_lab(torch.tensor([rgb], dtype=torch.uint8))[0]


def test_known_lab_values():
    """white, black, the red and blue primaries (to 1e-4, the figures every sRGB -> Lab table gives) and a grey"""
    assert torch.allclose(lab_u8(255, 255, 255), torch.tensor([100.0, 0.0, 0.0, 0.0], dtype=F64), rtol=0, atol=1e-9)
    assert torch.equal(lab_u8(0, 0, 0), torch.zeros(4, dtype=F64))
    assert torch.allclose(lab_u8(255, 0, 0)[:3], torch.tensor([53.2406, 80.0942, 67.2015], dtype=F64), rtol=0, atol=1e-4)
    assert torch.allclose(lab_u8(0, 0, 255)[:3], torch.tensor([32.2957, 79.1870, -107.8617], dtype=F64), rtol=0, atol=1e-4)
    grey = lab_u8(128, 128, 128)
    assert abs(float(grey[1])) < 1e-9 and abs(float(grey[2])) < 1e-9 and abs(float(grey[3])) < 1e-9 and 53.0 < float(grey[0]) < 54.0
    red = lab_u8(255, 0, 0)
    assert abs(float(red[3]) - (float(red[1]) ** 2 + float(red[2]) ** 2) ** 0.5) < 1e-12


def test_both_sides_of_both_branch_points():
    """sRGB curve: 10 / 255 <= 0.04045 < 11 / 255.  Lab: Y on either side of 0.008856, where the two branches of L meet to 1e-3"""
    c10, c11 = torch.tensor(10 / 255.0, dtype=F64), torch.tensor(11 / 255.0, dtype=F64)
    assert float(R.srgb_linear(c10)) == (10 / 255.0) / 12.92
    assert float(R.srgb_linear(c11)) == ((11 / 255.0 + 0.055) / 1.055) ** 2.4 != (11 / 255.0) / 12.92
    assert float(lab_u8(10, 10, 10)[0]) == pytest.approx(903.3 * (10 / 255.0) / 12.92, abs=1e-12)           # the coefficients of Y add up to 1
    c0 = 1.055 * 0.008856 ** (1 / 2.4) - 0.055                                                               # the grey whose Y is the branch point
    lo, hi = (R.rgb_to_lab(torch.full((1, 3), c0 * s, dtype=torch.float32))[0] for s in (1 - 1e-4, 1 + 1e-4))
    y_lo, y_hi = (float(R.srgb_linear(R.unit(torch.tensor(c0 * s, dtype=torch.float32)))) for s in (1 - 1e-4, 1 + 1e-4))
    assert y_lo < 0.008856 < y_hi
    assert float(lo[0]) == pytest.approx(903.3 * y_lo, abs=1e-12) and float(hi[0]) == pytest.approx(116.0 * y_hi ** (1 / 3) - 16.0, abs=1e-12)
    assert abs(float(lo[0]) - float(hi[0])) < 1e-2 and 7.9 < float(lo[0]) < 8.1
    assert abs(float(lo[1])) < 1e-9 and abs(float(hi[2])) < 1e-9
    # floats outside [0, 1] are clamped
    assert torch.equal(R.rgb_to_lab(torch.tensor([[1.5, -0.25, 0.0]])), R.rgb_to_lab(torch.tensor([[1.0, 0.0, 0.0]])))


def rand_hist(seed, n=1, total=5000, lo=0, hi=256):
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(lo, hi, (n, 3, total), generator=g)
    return torch.stack([torch.stack([torch.bincount(v[f, c], minlength=256) for c in range(3)]) for f in range(n)]).to(torch.int32)


def test_histogram_match_properties():
    src, ref = rand_hist(1, 1, 4000, 40, 200)[0].long(), rand_hist(2, 1, 9000, 0, 256)[0].long()
    for c in range(3):
        m = R.histogram_map(src[c], ref[c])
        assert bool((m[1:] >= m[:-1]).all()) and 0 <= int(m.min()) and int(m.max()) <= 255                  # monotone
        same = R.histogram_map(src[c], src[c])
        occupied = src[c] > 0
        assert torch.equal(same[occupied], torch.arange(256)[occupied])                                     # identity on the occupied bins
        assert torch.equal(R.histogram_lut(src[c], ref[c], 0.0), torch.arange(256, dtype=torch.uint8))      # strength 0
        assert torch.equal(R.meanstd_lut(src[c], ref[c], 0.0, 4.0), torch.arange(256, dtype=torch.uint8))
        # the matched cumulative distribution reaches the source's: cr[m[v]] / nr >= cs[v] / ns, and m[v] is the first such bin
        cs, cr = src[c].cumsum(0), ref[c].cumsum(0)
        assert bool((cr[m] * cs[255] >= cs * cr[255]).all())
        prev = (m - 1).clamp_min(0)
        assert bool(((cr[prev] * cs[255] < cs * cr[255]) | (m == 0)).all())
    # a hand-made case: two equally likely values onto three
    s, r = torch.zeros(256, dtype=torch.int64), torch.zeros(256, dtype=torch.int64)
    s[10], s[20] = 5, 5
    r[100], r[150], r[200] = 4, 4, 4
    m = R.histogram_map(s, r)
    assert int(m[10]) == 150 and int(m[20]) == 200 and int(m[9]) == 0 and int(m[15]) == 150
    assert int(R.histogram_lut(s, r, 0.5)[10]) == 80 and int(R.histogram_lut(s, r, 0.3)[20]) == 74


def test_meanstd_known_answers():
    s, r = torch.zeros(256, dtype=torch.int64), torch.zeros(256, dtype=torch.int64)
    s[100], s[110] = 7, 7                                                                                   # mean 105, std 5
    r[50], r[70] = 3, 3                                                                                     # mean 60, std 10
    lut = R.meanstd_lut(s, r, 1.0, 4.0)
    assert (int(lut[100]), int(lut[110]), int(lut[105])) == (50, 70, 60)
    lut = R.meanstd_lut(s, r, 1.0, 1.5)                                                                     # the gain 2 is cut to 1.5: 52.5 and 67.5, halves to even
    assert (int(lut[100]), int(lut[110])) == (52, 68)
    lut = R.meanstd_lut(r, s, 1.0, 1.25)                                                                    # the gain 0.5 is raised to 0.8
    assert (int(lut[50]), int(lut[70])) == (97, 113)
    lut = R.meanstd_lut(s, r, 0.5, 4.0)                                                                     # half way: gain 1.5, mean 82.5 -> 75 and 90
    assert (int(lut[100]), int(lut[110])) == (75, 90)
    flat = torch.zeros(256, dtype=torch.int64)
    flat[30] = 11                                                                                           # std 0: gain 1, the mean moves
    lut = R.meanstd_lut(flat, r, 1.0, 4.0)
    assert int(lut[30]) == 60 and int(lut[0]) == 30 and int(lut[255]) == 255
    lut = R.meanstd_lut(r, flat, 1.0, 4.0)                                                                  # anchor std 0: the gain 0 is raised to 1 / 4; 27.5 and 32.5, halves to even
    assert (int(lut[50]), int(lut[70])) == (28, 32)


def test_streaming_bookkeeping_of_the_reference():
    hist = rand_hist(5, 14, 600)
    anchor = rand_hist(6, 1, 900)[0].long()
    w3 = R.window_sums(hist, 3)
    assert torch.equal(w3[0], hist[0].long()) and torch.equal(w3[1], hist[:2].long().sum(0)) and torch.equal(w3[5], hist[3:6].long().sum(0))
    assert torch.equal(R.window_sums(hist[5:], 3, hist[3:5]), w3[5:]) and torch.equal(R.window_sums(hist[1:], 3, hist[:1]), w3[1:])
    assert torch.equal(R.window_sums(hist, 1), hist.long())
    for mode in ("meanstd", "histogram"):
        for given in (None, anchor):
            whole = R.match_luts(hist, R.anchor_of(given, hist, 8), mode, 0.7, 3, 2.0)
            s = R.Streamer(mode, 0.7, 3, 2.0, anchor=given, anchor_frames=8)
            pieces = torch.cat([s.update(hist[0:8]), s.update(hist[8:9]), s.update(hist[9:14])])
            assert torch.equal(pieces, whole)
            assert s.history.shape[0] == 2 and torch.equal(s.history, hist[12:14])
            s.new_video()
            assert s.history is None and torch.equal(s.update(hist[0:8]), whole[0:8])
    with pytest.raises(ValueError):
        R.Streamer(anchor_frames=8).update(hist[:7])


def test_refusals_before_any_device():
    from tokensgen_amd import color, metrics, video_io
    u8 = torch.zeros(4, 6, 5, 3, dtype=torch.uint8)
    with pytest.raises(NotImplementedError):
        color.match_colors(u8.float())
    with pytest.raises(NotImplementedError):
        color.color_histograms(u8.to(torch.int16))
    with pytest.raises(NotImplementedError):
        color.ColorMatcher().update(u8.to(torch.bfloat16))
    for bad in (u8[..., :2], u8[0, 0], torch.zeros(0, 6, 5, 3, dtype=torch.uint8), "frames"):
        with pytest.raises(ValueError):
            color.match_colors(bad)
    for kw in (dict(mode="lab"), dict(strength=1.5), dict(strength=-0.1), dict(strength="1"), dict(window=0), dict(window=65), dict(window=2.0), dict(max_gain=0.5),
               dict(max_gain=float("inf")), dict(anchor_frames=0), dict(anchor=torch.zeros(3, 256)), dict(anchor=torch.zeros(3, 255, dtype=torch.int64))):
        with pytest.raises(ValueError):
            color.match_colors(u8, **kw)
        if "anchor_frames" not in kw:
            with pytest.raises(ValueError):
                color.ColorMatcher(**kw)
    with pytest.raises(ValueError, match="2\\^31"):
        color.match_colors(torch.zeros(2, 1, 1, 3, dtype=torch.uint8).expand(2, 40000, 40000, 3), window=2)
    with pytest.raises(ValueError, match="anchor frames"):
        color.ColorMatcher(anchor_frames=8).update(u8)                                                      # 4 frames: no lookahead
    with pytest.raises(ValueError):
        color.ColorMatcher().update(u8[None])                                                               # one video's clip
    hist, anchor = torch.zeros(2, 3, 256, dtype=torch.int32), torch.zeros(3, 256, dtype=torch.int64)
    for h, a, kw in ((hist.long(), anchor, {}), (hist, anchor.int(), {}), (hist[0], anchor, {}), (hist, anchor, dict(history=hist, window=2)),
                     (hist, anchor, dict(history=hist.long(), window=3))):
        with pytest.raises(ValueError):
            color.match_luts(h, a, **kw)
    with pytest.raises(ValueError):
        color.apply_luts(u8, torch.zeros(3, 3, 256, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="GPU"):
        color.color_histograms(u8)                                                                          # no CPU path
    with pytest.raises(RuntimeError, match="GPU"):
        color.match_luts(hist, anchor)
    # metrics
    img = torch.zeros(8, 9, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="test_y_channel"):
        metrics.calculate_delta_Eab(img, img, 0, test_y_channel=True)
    with pytest.raises(ValueError, match="input_order"):
        metrics.calculate_delta_Eab(img, img, 0, input_order="WHC")
    with pytest.raises(ValueError):
        metrics.calculate_delta_Eab(img, img, 0, input_order="CHW")
    with pytest.raises(AssertionError):
        metrics.calculate_delta_Eab(img, img[:4], 0)
    with pytest.raises(ValueError):
        metrics.video_color_drift(u8, anchor_frames=0)
    with pytest.raises(ValueError):
        metrics.video_color_drift(u8, anchor_frames=5)
    with pytest.raises(ValueError):
        metrics.VideoColorDrift(anchor_frames=True)
    with pytest.raises(ValueError):
        metrics.video_delta_eab(u8, u8, crop_border=3)                                                      # nothing left of a 6 x 5 frame
    with pytest.raises(RuntimeError, match="GPU"):
        metrics.video_delta_eab(u8, u8)
    with pytest.raises(RuntimeError):
        metrics.VideoColorDrift().finalize()
    # video_io
    for args, kw in ((("lab",), {}), (("meanstd",), dict(strength=2.0)), (("histogram",), dict(window=0)), (("meanstd",), dict(anchor_frames=0)),
                     (("meanstd",), dict(anchor=torch.zeros(3, 256)))):
        with pytest.raises(ValueError):
            video_io.VideoProcessor().set_color_match(*args, **kw)
    vp = video_io.VideoProcessor().set_color_match("meanstd")
    assert (vp.color_match, vp.color_anchor, vp.color_anchor_frames, vp.color_strength, vp.color_window) == ("meanstd", None, 8, 1.0, 1)
    assert video_io.VideoProcessor().color_match is None and vp.set_color_match(None).color_match is None and vp.set_color_match("meanstd") is vp
    for ot in ("np", "pt"):
        with pytest.raises(ValueError, match="color_match"):
            vp.postprocess_video(torch.zeros(1, 3, 2, 8, 8, dtype=torch.bfloat16), ot)


def test_default_processor_imports_no_colour_code():
    import subprocess
    import sys
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); from tokensgen_amd import video_io, metrics; video_io.VideoProcessor(); metrics.VideoMetrics(); "
            "assert 'tokensgen_amd.color' not in sys.modules; video_io.VideoProcessor().set_color_match('meanstd'); assert 'tokensgen_amd.color' in sys.modules") % root
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]


def test_c_abi_validates_before_any_launch():
    """one argument wrong at a time; the calls never reach a launch"""
    from tokensgen_amd import lib as L
    lib = L.load()
    err = lambda: lib.tg_last_error_string().decode()
    buf = ctypes.create_string_buffer(8192)
    p = ctypes.addressof(buf) + (16 - ctypes.addressof(buf) % 16)
    assert lib.tg_color_hist_u8(p, 0, 4, 4, p, None) == -2 and "bad shape" in err()
    assert lib.tg_color_hist_u8(p, 1, 65536, 32768, p, None) == -2 and "2^31" in err()                    # H W = 2^31
    assert lib.tg_color_hist_u8(p, 1, 4, 4, p + 2, None) == -3
    assert lib.tg_color_hist_u8(None, 1, 4, 4, p, None) == -1 and "null pointer" in err()
    ml = dict(hist=p, F=1, history=None, n_history=0, anchor=p, mode=0, strength=1.0, window=1, max_gain=4.0, lut=p, status=p, stream=None)
    call = lambda **kw: lib.tg_color_match_lut(*{**ml, **kw}.values())
    assert call(mode=2) == -1 and "mode" in err()
    assert call(strength=1.5) == -1 and call(strength=-0.5) == -1 and call(strength=float("nan")) == -1 and call(max_gain=0.99) == -1 and call(max_gain=float("inf")) == -1
    assert call(window=0) == -1 and call(window=65) == -1 and "1..64" in err()
    assert call(F=0) == -2 and call(n_history=1) == -2 and call(n_history=1, window=2) == -2 and "carried" in err()     # as many as the window; no pointer
    assert call(n_history=2, window=2, history=p) == -2 and call(n_history=-1) == -2
    assert call(anchor=p + 4) == -3 and call(hist=p + 2) == -3 and call(status=p + 1) == -3
    assert call(status=None) == -1 and call(lut=None) == -1 and call(anchor=None) == -1
    assert lib.tg_color_apply_lut(p, p, 1, 65536, 32768, p + 4096, None) == -2 and "2^31" in err()
    assert lib.tg_color_apply_lut(p, p + 2, 1, 4, 4, p + 4096, None) == -3
    assert lib.tg_color_apply_lut(p, p + 4096, 2, 4, 4, p + 16, None) == -1 and "overlap" in err()        # 96 bytes, 16 apart
    assert lib.tg_color_apply_lut(p, p + 4096, 0, 4, 4, p, None) == -2
    lab = dict(a=p, a_so=0, a_si=48, a_sc=1, a_sr=12, a_sp=3, b=None, b_so=0, b_si=0, b_sc=0, b_sr=0, b_sp=0, dtype=0, n_outer=1, n_inner=1, h=4, w=4, ws=p + 1024,
               out=p + 2048, stream=None)
    call = lambda **kw: lib.tg_lab_metrics(*{**lab, **kw}.values())
    assert call(dtype=3) == -1 and call(h=0) == -2 and call(n_inner=0) == -2 and call(a_sr=-12) == -2 and "negative stride" in err()
    assert call(dtype=1, a=p + 2) == -3 and call(ws=p + 1028) == -3 and call(out=None) == -1 and call(n_outer=1 << 30, n_inner=4) == -2 and "too many tiles" in err()
    th, tw = lib.tg_lab_metrics_tile(0), lib.tg_lab_metrics_tile(1)
    assert th >= 1 and tw >= 1 and lib.tg_lab_metrics_tile(2) == 0
    assert lib.tg_lab_metrics_ws_doubles(1, 1, 1, 0) == 4 and lib.tg_lab_metrics_ws_doubles(5, th, tw + 1, 1) == 90 and lib.tg_lab_metrics_ws_doubles(0, 4, 4, 0) == 0
    assert lib.tg_color_strip_bytes(0) % 16 == 0 and lib.tg_color_strip_bytes(1) % 16 == 0 and lib.tg_color_strip_bytes(2) == 0
