"""Colour of the byte output, on the GPU and in exact arithmetic: per-frame histograms (tg_color_hist_u8), per-frame lookup tables that pull a video's colour
towards an anchor (tg_color_match_lut) and their application (tg_color_apply_lut), csrc/color.hip; DESIGN.md §8j.  No reference code: the header's comment is the
definition, tests/color_ref.py restates it.

    from tokensgen_amd.color import match_colors, ColorMatcher

Long FIFO generation lets exposure, white balance and saturation wander away from the first clip.  `match_colors` measures every frame's three channel histograms,
sums them over a causal window, and maps each channel by one 256-entry table per frame towards the anchor (by default the video's own first frames): `meanstd` moves
mean and standard deviation (the per-channel "AdaIN colour fix"), `histogram` matches the cumulative distribution exactly, in integers.  `strength` blends the table
with the identity, `window` smooths it over time, `max_gain` bounds the contrast change.  `ColorMatcher` does the same for a video that arrives clip by clip and
produces the bytes of one call.  `metrics.video_color_drift` measures what this corrects.

uint8 frames only ("uint8" of video_io.VideoProcessor, which runs this step after `set_color_match`).  Every refusal comes before any kernel call.  There is no CPU path."""
import torch

from . import kernels as K
from .frames import check_frames, is_int

MODES = tuple(K.COLOR_MODES)
MAX_WINDOW = K.COLOR_MAX_WINDOW


def check_params(mode, strength, window, max_gain, who):
    if mode not in MODES:
        raise ValueError(f"{who}: mode must be one of {MODES}, got {mode!r}")
    if isinstance(strength, bool) or not isinstance(strength, (int, float)) or not 0.0 <= strength <= 1.0:
        raise ValueError(f"{who}: strength must be a number in [0, 1], got {strength!r}")
    if not is_int(window) or not 1 <= window <= MAX_WINDOW:
        raise ValueError(f"{who}: window must be an integer in 1..{MAX_WINDOW}, got {window!r}")
    if isinstance(max_gain, bool) or not isinstance(max_gain, (int, float)) or not 1.0 <= max_gain < float("inf"):
        raise ValueError(f"{who}: max_gain must be a finite number >= 1, got {max_gain!r}")


def check_anchor_frames(anchor_frames, who):
    if not is_int(anchor_frames) or anchor_frames < 1:
        raise ValueError(f"{who}: anchor_frames must be a positive integer, got {anchor_frames!r}")


def check_color_frames(frames, who, dims=(4, 5)):
    """frames.check_frames and what is colour's own: a frame's histogram counts are int32"""
    check_frames(frames, who, dims)
    if frames.shape[-3] * frames.shape[-2] >= 1 << 31:
        raise ValueError(f"{who}: a frame of {frames.shape[-3]} x {frames.shape[-2]} pixels reaches 2^31")


def _check_hist(h, name, dtype, lead, who):
    shape = "[F, 3, 256]" if lead else "[3, 256]"
    if not isinstance(h, torch.Tensor) or h.dtype != dtype or h.dim() != 2 + lead or tuple(h.shape[-2:]) != (3, 256) or (lead and h.shape[0] < 1):
        raise ValueError(f"{who}: {name} must be {dtype} {shape}, got {getattr(h, 'dtype', type(h))} {tuple(getattr(h, 'shape', ()))}")


def color_histograms(frames):
    """uint8 [F, H, W, 3] (or [B, T, H, W, 3]) -> int32 [F, 3, 256] ([B, T, 3, 256]): per frame and channel the number of pixels of each value.  Exact; a frame's
    counts depend on that frame alone.  A view that is not contiguous is copied first."""
    check_color_frames(frames, "color_histograms")
    h = K.color_hist_u8(frames.contiguous().reshape(-1, *frames.shape[-3:]))
    return h.reshape(*frames.shape[:-3], 3, 256)


def match_luts(hist, anchor_hist, mode="meanstd", strength=1.0, window=1, max_gain=4.0, history=None, status=None):
    """The per-frame tables: hist int32 [F, 3, 256] (color_histograms of one video's consecutive frames), anchor_hist int64 [3, 256] -> uint8 [F, 3, 256].  Frame t's
    source histogram is the sum over frames max(0, t - window + 1) .. t counted from the start of the video; `history` (int32 [n, 3, 256], n < window) carries the
    frames before this call's, oldest first.  A histogram with a negative count or a total outside 1 .. 2^31 - 1 cannot be judged on the host without waiting for
    the device: the device gives it the identity table and counts it in `status` (an int32 [1] device tensor of the caller's, optional)."""
    check_params(mode, strength, window, max_gain, "match_luts")
    _check_hist(hist, "hist", torch.int32, 1, "match_luts")
    _check_hist(anchor_hist, "anchor_hist", torch.int64, 0, "match_luts")
    if history is not None:
        if not isinstance(history, torch.Tensor) or history.dtype != torch.int32 or history.dim() != 3 or tuple(history.shape[1:]) != (3, 256):
            raise ValueError(f"match_luts: history must be int32 [n, 3, 256], got {getattr(history, 'dtype', type(history))} {tuple(getattr(history, 'shape', ()))}")
        if history.shape[0] >= window:
            raise ValueError(f"match_luts: history carries {history.shape[0]} frames; a window of {window} takes at most {window - 1}")
        history = history.contiguous()
    return K.color_match_lut(hist.contiguous(), anchor_hist.contiguous(), mode, strength, window, max_gain, history, status)[0]


def apply_luts(frames, luts, out=None):
    """out[f, y, x, c] = luts[f, c, frames[f, y, x, c]].  frames uint8 [F, H, W, 3] contiguous, luts uint8 [F, 3, 256]; out: None (a new tensor), `frames` (in place)
    or a contiguous tensor of the frames' shape."""
    check_color_frames(frames, "apply_luts", dims=(4,))
    if not isinstance(luts, torch.Tensor) or luts.dtype != torch.uint8 or tuple(luts.shape) != (frames.shape[0], 3, 256):
        raise ValueError(f"apply_luts: luts must be uint8 [{frames.shape[0]}, 3, 256], got {getattr(luts, 'dtype', type(luts))} {tuple(getattr(luts, 'shape', ()))}")
    if not frames.is_contiguous():
        raise ValueError("apply_luts: frames must be contiguous")
    return K.color_apply_lut(frames, luts.contiguous(), out)


def check_anchor(anchor, who):
    """None, uint8 frames of any size, or an int64 [3, 256] histogram"""
    if anchor is None:
        return
    if isinstance(anchor, torch.Tensor) and anchor.dtype == torch.int64 and tuple(anchor.shape) == (3, 256):
        return
    if isinstance(anchor, torch.Tensor) and anchor.dtype == torch.uint8 and anchor.dim() in (3, 4, 5) and anchor.shape[-1] == 3 and anchor.numel() >= 1:
        return
    raise ValueError(f"{who}: anchor must be None, uint8 frames [.., H, W, 3] or an int64 [3, 256] histogram, got "
                     f"{getattr(anchor, 'dtype', type(anchor))} {tuple(getattr(anchor, 'shape', ()))}")


def anchor_histogram(anchor, device):
    """int64 [3, 256] on `device` from a checked anchor (not None): a histogram as it is, frames by the sum of their histograms"""
    if anchor.dtype == torch.int64:
        return anchor.to(device)
    f = anchor.to(device).contiguous().reshape(-1, *anchor.shape[-3:]) if anchor.dim() != 3 else anchor.to(device).contiguous()[None]
    return K.color_hist_u8(f).sum(0, dtype=torch.int64)


def _check_window_total(window, H, W, who):
    if window * H * W >= 1 << 31:
        raise ValueError(f"{who}: a window of {window} frames of {H} x {W} pixels reaches a histogram total of 2^31")


def match_colors(frames, anchor=None, anchor_frames=8, mode="meanstd", strength=1.0, window=1, max_gain=4.0, return_luts=False):
    """Colour-match a video to an anchor.  frames: uint8 [T, H, W, 3] or [B, T, H, W, 3] (each batch item is its own video).  anchor: uint8 frames of any size, whose
    histograms are summed; an int64 [3, 256] histogram; or None: the first min(T, anchor_frames) frames of the video itself.  Returns the matched uint8 video (a new
    tensor), or with return_luts (video, luts uint8 [.., T, 3, 256]).  With strength 0, or with mode "histogram" and an anchor equal to the source, the output is
    the input byte for byte.  Nothing here waits for the device."""
    check_color_frames(frames, "match_colors")
    check_params(mode, strength, window, max_gain, "match_colors")
    check_anchor_frames(anchor_frames, "match_colors")
    check_anchor(anchor, "match_colors")
    T, H, W = frames.shape[-4:-1]
    _check_window_total(window, H, W, "match_colors")
    src = frames.contiguous()
    hist = color_histograms(src)
    ref = None if anchor is None else anchor_histogram(anchor, frames.device)
    h5 = hist if frames.dim() == 5 else hist[None]
    luts = torch.stack([match_luts(h, ref if ref is not None else h[:min(T, anchor_frames)].sum(0, dtype=torch.int64), mode, strength, window, max_gain) for h in h5])
    out = K.color_apply_lut(src.reshape(-1, H, W, 3), luts.reshape(-1, 3, 256)).reshape(frames.shape)
    return (out, luts.reshape(*frames.shape[:-3], 3, 256)) if return_luts else out


class ColorMatcher:
    """match_colors for a long video that arrives clip by clip (the FIFO result).  `update(frames)` continues the current video with a clip, uint8 [F, H, W, 3]
    (F >= 1), and returns it matched; the object keeps the anchor histogram and the last window - 1 frame histograms on the device, so the pieces are the bytes of one
    match_colors call on the whole video.  anchor as in match_colors; with None the anchor is taken from the first anchor_frames frames of the video, which the first
    `update` must carry (ValueError otherwise: no lookahead).  `new_video(anchor=None)` starts the next video (None: the constructor's anchor).  Nothing waits for
    the device."""

    def __init__(self, mode="meanstd", strength=1.0, window=1, max_gain=4.0, anchor=None, anchor_frames=8):
        check_params(mode, strength, window, max_gain, "ColorMatcher")
        check_anchor_frames(anchor_frames, "ColorMatcher")
        check_anchor(anchor, "ColorMatcher")
        self.mode, self.strength, self.window, self.max_gain, self.anchor_frames = mode, strength, window, max_gain, anchor_frames
        self._given = anchor
        self.new_video()

    def new_video(self, anchor=None):
        check_anchor(anchor, "ColorMatcher.new_video")
        self._anchor = anchor if anchor is not None else self._given          # frames, a histogram or None; a histogram on the device after the first update
        self._ready, self._history = False, None

    def update(self, frames):
        check_color_frames(frames, "ColorMatcher.update", dims=(4,))
        _check_window_total(self.window, frames.shape[1], frames.shape[2], "ColorMatcher.update")
        if not self._ready and self._anchor is None and frames.shape[0] < self.anchor_frames:
            raise ValueError(f"ColorMatcher.update: the first clip of a video must carry the {self.anchor_frames} anchor frames, got {frames.shape[0]} (no lookahead)")
        src = frames.contiguous()
        hist = color_histograms(src)
        if not self._ready:
            self._anchor = hist[:self.anchor_frames].sum(0, dtype=torch.int64) if self._anchor is None else anchor_histogram(self._anchor, frames.device)
            self._ready = True
        luts = match_luts(hist, self._anchor, self.mode, self.strength, self.window, self.max_gain, self._history)
        if self.window > 1:
            seen = hist if self._history is None else torch.cat([self._history, hist])
            self._history = seen[-(self.window - 1):].clone()
        return K.color_apply_lut(src, luts)
