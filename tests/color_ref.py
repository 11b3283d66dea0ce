"""The definitions of the colour feature (include/tokensgen_hip.h) restated in torch float64 / int64, written from the definitions, not from the
kernels.  Every function runs on whatever device its inputs are on.

Lab: OpenCV's documented floating-point RGB2Lab.  Histograms: bincount.  Tables: the causal window sum in int64, then `meanstd` (each float64 operation is its own
torch call, so each is rounded by itself, in the order of the definition) or `histogram` (integers only up to the final blend).  Streaming: the bookkeeping a
clip-by-clip caller has to do so that the pieces give the tables of one call."""
import torch

F64 = torch.float64


# ---- L*a*b* -------------------------------------------------------------------------------------------------------------------------------------------------------------
def unit(t):
    """pixel values as float64 in [0, 1]: uint8 / 255, floats clamped"""
    if t.dtype == torch.uint8:
        return t.to(F64) / 255.0
    return t.to(F64).clamp(0.0, 1.0)


def srgb_linear(c):
    return torch.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055).pow(2.4))


def _cbrt(t):
    return t.clamp_min(0.0).pow(1.0 / 3.0)


def _f(t):
    return torch.where(t > 0.008856, _cbrt(t), 7.787 * t + 16.0 / 116.0)


def rgb_to_lab(rgb):
    """rgb: [..., 3] pixel values (uint8, or floats in [0, 1]) -> float64 [..., 4] = (L, a, b, C)"""
    lin = srgb_linear(unit(rgb))
    R, G, B = lin[..., 0], lin[..., 1], lin[..., 2]
    X = (0.412453 * R + 0.357580 * G + 0.180423 * B) / 0.950456
    Y = 0.212671 * R + 0.715160 * G + 0.072169 * B
    Z = (0.019334 * R + 0.119193 * G + 0.950227 * B) / 1.088754
    L = torch.where(Y > 0.008856, 116.0 * _cbrt(Y) - 16.0, 903.3 * Y)
    a = 500.0 * (_f(X) - _f(Y))
    b = 200.0 * (_f(Y) - _f(Z))
    return torch.stack([L, a, b, (a * a + b * b).sqrt()], dim=-1)


def lab_means(a, b=None):
    """a, b: [F, H, W, 3] channels-last frames.  Per-frame means over the pixels: float64 [F, 4] (L, a, b, C) of `a`; with b [F, 9]: those, the same of b, and
    the mean CIE76 dE"""
    la = rgb_to_lab(a)
    out = [la.mean(dim=(1, 2))]
    if b is not None:
        lb = rgb_to_lab(b)
        out += [lb.mean(dim=(1, 2)), (la[..., :3] - lb[..., :3]).pow(2).sum(-1).sqrt().mean(dim=(1, 2))[:, None]]
    return torch.cat(out, dim=1)


def channels_last(t, layout):
    """a video in one of the layouts of metrics._layout as [F, H, W, 3]"""
    if layout == "hwc":
        return t.reshape(-1, *t.shape[-3:])
    if layout == "chw":
        return t.permute(0, 2, 3, 1)
    if layout == "bcthw":
        return t.permute(0, 2, 3, 4, 1).reshape(-1, t.shape[3], t.shape[4], 3)
    raise ValueError(layout)


def crop(t, cb):
    return t if cb == 0 else t[:, cb:-cb, cb:-cb]


def color_drift(frames, anchor_frames=1):
    """frames [F, H, W, 3] -> dict of the curves of metrics.video_color_drift"""
    m = lab_means(frames)
    lab, chroma = m[:, :3], m[:, 3]
    drift = (lab - lab[:anchor_frames].mean(0, keepdim=True)).pow(2).sum(-1).sqrt()
    return {"lab_mean": lab, "chroma": chroma, "drift": drift, "drift_mean": drift.mean(), "drift_max": drift.max(), "chroma_ratio": chroma[-1] / chroma[0]}


# ---- histograms and tables ----------------------------------------------------------------------------------------------------------------------------------------------
def histograms(frames):
    """uint8 [F, H, W, 3] -> int64 [F, 3, 256]"""
    F = frames.shape[0]
    flat = frames.reshape(F, -1, 3).to(torch.int64)
    return torch.stack([torch.stack([torch.bincount(flat[f, :, c], minlength=256) for c in range(3)]) for f in range(F)])


def window_sums(hist, window, history=None):
    """S_t = sum of hist_k, k = max(0, t - window + 1) .. t, k counted from the start of the video; history: the frames before hist's, oldest first.  int64 [F, 3, 256]"""
    h = hist.to(torch.int64)
    n0 = 0
    if history is not None and history.shape[0] > 0:
        n0 = history.shape[0]
        h = torch.cat([history.to(torch.int64), h])
    return torch.stack([h[max(0, t - window + 1):t + 1].sum(0) for t in range(n0, h.shape[0])])


def _moments(S):
    """S int64 [256] -> (mean, std) as 0-dim float64, each operation rounded by itself"""
    v = torch.arange(256, dtype=torch.int64, device=S.device)
    n, s1, s2 = S.sum(), (v * S).sum(), (v * v * S).sum()
    mean = s1.to(F64) / n.to(F64)
    ex2 = s2.to(F64) / n.to(F64)
    var = (ex2 - mean * mean).clamp_min(0.0)
    return mean, var.sqrt()


def meanstd_lut(S, R, strength, max_gain):
    """S, R int64 [256] (source, anchor) -> uint8 [256]"""
    ms, ss = _moments(S)
    mr, sr = _moments(R)
    g = sr / ss if float(ss) > 0.0 else torch.ones((), dtype=F64, device=S.device)
    g = g.clamp_min(1.0 / max_gain).clamp_max(max_gain)
    g2 = 1.0 + strength * (g - 1.0)
    m2 = ms + strength * (mr - ms)
    v = torch.arange(256, dtype=F64, device=S.device)
    return ((v - ms) * g2 + m2).round().clamp(0.0, 255.0).to(torch.uint8)           # torch.round: halves to even


def histogram_map(S, R):
    """m[v] = min{u : cr[u] ns >= cs[v] nr}, int64 [256]"""
    cs, cr = S.cumsum(0), R.cumsum(0)
    ns, nr = cs[255], cr[255]
    return ((cr * ns)[None, :] < (cs * nr)[:, None]).sum(1)                          # cr is non-decreasing: the number of u that fail is the first u that holds


def histogram_lut(S, R, strength):
    v = torch.arange(256, dtype=torch.int64, device=S.device)
    m = histogram_map(S, R)
    return (v.to(F64) + strength * (m - v).to(F64)).round().clamp(0.0, 255.0).to(torch.uint8)


def match_luts(hist, anchor, mode="meanstd", strength=1.0, window=1, max_gain=4.0, history=None):
    """hist [F, 3, 256], anchor int64 [3, 256] -> uint8 [F, 3, 256]"""
    S = window_sums(hist, window, history)
    one = (lambda s, r: meanstd_lut(s, r, strength, max_gain)) if mode == "meanstd" else (lambda s, r: histogram_lut(s, r, strength))
    return torch.stack([torch.stack([one(S[f, c], anchor[c]) for c in range(3)]) for f in range(S.shape[0])])


def apply_luts(frames, luts):
    """frames uint8 [F, H, W, 3], luts uint8 [F, 3, 256] -> out[f, y, x, c] = luts[f, c, frames[f, y, x, c]]"""
    F, H, W, _ = frames.shape
    idx = frames.reshape(F, H * W, 3).permute(0, 2, 1).to(torch.int64)                 # [F, 3, HW]
    return torch.gather(luts, 2, idx).permute(0, 2, 1).reshape(F, H, W, 3).contiguous()


def anchor_of(anchor, hist, anchor_frames):
    """the anchor histogram of one video: None -> the first anchor_frames frames' sum; uint8 frames -> their histograms' sum; int64 [3, 256] as it is"""
    if anchor is None:
        return hist[:min(hist.shape[0], anchor_frames)].to(torch.int64).sum(0)
    if anchor.dtype == torch.int64:
        return anchor
    return histograms(anchor.reshape(-1, *anchor.shape[-3:])).sum(0)


def match_colors(frames, anchor=None, anchor_frames=8, mode="meanstd", strength=1.0, window=1, max_gain=4.0):
    """frames uint8 [T, H, W, 3] -> (matched frames, luts)"""
    hist = histograms(frames)
    luts = match_luts(hist, anchor_of(anchor, hist, anchor_frames), mode, strength, window, max_gain)
    return apply_luts(frames, luts), luts


class Streamer:
    """The bookkeeping of a clip-by-clip caller, on histograms: the anchor from the first clip (or given), the last window - 1 histograms carried."""

    def __init__(self, mode="meanstd", strength=1.0, window=1, max_gain=4.0, anchor=None, anchor_frames=8):
        self.mode, self.strength, self.window, self.max_gain, self.given, self.anchor_frames = mode, strength, window, max_gain, anchor, anchor_frames
        self.new_video()

    def new_video(self, anchor=None):
        self.anchor = anchor if anchor is not None else self.given
        self.history = None

    def update(self, hist):
        """hist [F, 3, 256] of the next clip -> its tables"""
        if self.anchor is None:
            if hist.shape[0] < self.anchor_frames:
                raise ValueError("the first clip must carry the anchor frames")
            self.anchor = hist[:self.anchor_frames].to(torch.int64).sum(0)
        luts = match_luts(hist, self.anchor, self.mode, self.strength, self.window, self.max_gain, self.history)
        if self.window > 1:
            seen = hist if self.history is None else torch.cat([self.history, hist])
            self.history = seen[-(self.window - 1):]
        return luts
