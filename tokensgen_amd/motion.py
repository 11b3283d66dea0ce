"""Motion between the frames of a video, on the GPU and in integers: exhaustive block matching on 8-bit luma (tg_luma_u8, tg_block_motion) and the
motion-compensated squared error (tg_block_warp_sse), csrc/motion.hip.  The definitions are the project's own (include/tokensgen_hip.h); every result
of the kernels is an exact integer, so a test is `torch.equal`.

    from tokensgen_amd.motion import block_motion, warp_sse, summarize

Frames are the uint8 output of video_io, [F, H, W, 3] or [B, T, H, W, 3] (views allowed).  Pairs are (t, t + 1) inside each batch item; with `ref` (same shape)
frame t of `frames` is paired with frame t of `ref`.  The vector (dy, dx) of a block says: the block at (y, x) of the first frame of the pair matches
(y + dy, x + dx) of the second.  `summarize` is plain torch arithmetic on the small per-block results and runs on any device; the search has no CPU path.

`interpolate_frames` / `FrameRateUpsampler` use those vectors to make frames: motion-compensated interpolation of the in-between frames of every pair, for an
integer frame-rate factor 2 .. 8 (tg_mci_select, tg_mci_render, csrc/mci.hip), exact integers as well.
Not registered under the `longvgen` alias."""
import math

import torch

from . import kernels as K
from .frames import check_frames, is_int

BLOCKS, MAX_RADIUS, FACTORS = K.MOTION_BLOCKS, K.MOTION_MAX_RADIUS, K.MCI_FACTORS


def check_pairs(frames, who, ref=None, pairs_within=True):
    """frames.check_frames and what is motion's own, the second video and the pairs; checked before any kernel call.  Returns the number of pairs per batch item."""
    check_frames(frames, who)
    if ref is not None:
        if not isinstance(ref, torch.Tensor):
            raise ValueError(f"{who}: expected a tensor as the second video")
        if ref.dtype != torch.uint8:
            raise NotImplementedError(f"{who}: uint8 frames only, got {ref.dtype}")
        if ref.shape != frames.shape:
            raise ValueError(f"{who}: the two videos differ in shape: {tuple(frames.shape)} and {tuple(ref.shape)}")
    n = frames.shape[-4]
    pairs = n - 1 if pairs_within else n
    if pairs < 1 or (frames.dim() == 5 and frames.shape[0] < 1):
        raise ValueError(f"{who}: {n} frame(s) make no pair; pass at least 2")
    return pairs


def check_block(block, radius, H, W, who):
    if not isinstance(block, int) or block not in BLOCKS:
        raise ValueError(f"{who}: block must be one of {BLOCKS}, got {block!r}")
    if radius is not None and (not is_int(radius) or not 1 <= radius <= MAX_RADIUS):
        raise ValueError(f"{who}: radius must be an integer in 1..{MAX_RADIUS}, got {radius!r}")
    if H < block or W < block:
        raise ValueError(f"{who}: a {H} x {W} frame holds no {block} x {block} block")


def block_motion(frames, block=16, radius=16, ref=None):
    """Exhaustive block matching.  Returns {"mv": int16 [.., P, Hb, Wb, 2] as (dy, dx), "sad": int32 [.., P, Hb, Wb] the winner's cost, "sad0": int32 the cost at
    (0, 0)} on the device; P = F - 1 (T - 1 per batch item), or F (T) with `ref`.  The winner is the minimum of (sad, dy^2 + dx^2, dy, dx) over the candidates that
    keep the block inside the frame.  Nothing here waits for the device."""
    P = check_pairs(frames, "block_motion", ref, pairs_within=ref is None)
    H, W = frames.shape[-3], frames.shape[-2]
    check_block(block, radius, H, W, "block_motion")
    ya = K.luma_u8(frames)
    if ref is None:
        cur, oth = ya[:, :-1], ya[:, 1:]
    else:
        cur, oth = ya, K.luma_u8(ref)
    mv, sad, sad0 = K.block_motion(cur, oth, W, block, radius)
    if frames.dim() == 4:
        mv, sad, sad0 = mv[0], sad[0], sad0[0]
    assert mv.shape[-4] == P
    return {"mv": mv, "sad": sad, "sad0": sad0}


def warp_sse(frames, mv, ref=None):
    """Motion-compensated squared error of uint8 RGB frames under given vectors (this video's or another's of the same shape): {"sse": int32 [.., P, Hb, Wb] =
    sum over the block and the channels of (cur - ref displaced by (dy, dx))^2, "sse0": the same at zero displacement, "status": int32 [1], the number of vectors
    that pointed out of the frame and were clamped (0 for vectors of block_motion)}.  The block size is read off mv's shape: H // Hb must be 8 or 16."""
    P = check_pairs(frames, "warp_sse", ref, pairs_within=ref is None)
    H, W = frames.shape[-3], frames.shape[-2]
    if not isinstance(mv, torch.Tensor) or mv.dtype != torch.int16 or mv.dim() != frames.dim() or mv.shape[-1] != 2 or mv.shape[-2] < 1 or mv.shape[-3] < 1:
        raise ValueError(f"warp_sse: mv must be int16 [.., P, Hb, Wb, 2], got {getattr(mv, 'dtype', None)} {tuple(getattr(mv, 'shape', ()))}")
    block = next((b for b in BLOCKS if (H // b, W // b) == tuple(mv.shape[-3:-1])), None)
    if block is None or mv.shape[:-3] != frames.shape[:-4] + (P,):
        raise ValueError(f"warp_sse: mv {tuple(mv.shape)} does not describe the blocks of {P} pair(s) of {H} x {W} frames")
    check_block(block, None, H, W, "warp_sse")
    if ref is None:
        cur, oth = (frames[:-1], frames[1:]) if frames.dim() == 4 else (frames[:, :-1], frames[:, 1:])
    else:
        cur, oth = frames, ref
    m5 = mv.contiguous()
    sse, sse0, status = K.block_warp_sse(cur, oth, m5[None] if frames.dim() == 4 else m5, block)
    if frames.dim() == 4:
        sse, sse0 = sse[0], sse0[0]
    return {"sse": sse, "sse0": sse0, "status": status}


def check_factor(factor, who):
    if not is_int(factor) or not FACTORS[0] <= factor <= FACTORS[1]:
        raise ValueError(f"{who}: factor must be an integer in {FACTORS[0]}..{FACTORS[1]}, got {factor!r}")


def interpolate_frames(frames, factor=2, block=16, radius=16, bidirectional=True, return_vectors=False):
    """Motion-compensated frame-rate upsampling.  frames: uint8 [F, H, W, 3] or [B, T, H, W, 3] (any view), at least 2 frames.  Returns the uint8 video
    [.., (T - 1) * factor + 1, H, W, 3]: original frame t sits at index t * factor byte for byte, frame t * factor + k is the phase-k frame of pair (t, t + 1) and
    depends on that pair's two frames alone.  The vectors of block_motion (prev -> next and, with `bidirectional`, next -> prev) give every block of an in-between
    frame its candidates; tg_mci_select picks one by the bilateral SAD, tg_mci_render blends the overlapping block predictions.  With return_vectors a dict
    {"video", "mvi": int16 [.., P, factor - 1, Hb, Wb, 2], "cost": int32 [.., P, factor - 1, Hb, Wb]}.  Nothing here waits for the device."""
    P = check_pairs(frames, "interpolate_frames")
    H, W = frames.shape[-3], frames.shape[-2]
    check_factor(factor, "interpolate_frames")
    check_block(block, radius, H, W, "interpolate_frames")
    f5 = frames if frames.dim() == 5 else frames[None]
    ya = K.luma_u8(f5)
    prev, nxt = ya[:, :-1], ya[:, 1:]
    fwd = K.block_motion(prev, nxt, W, block, radius)[0]
    bwd = K.block_motion(nxt, prev, W, block, radius)[0] if bidirectional else None
    mvi, cost = K.mci_select(prev, nxt, fwd, bwd, W, block, factor)
    video = torch.empty(f5.shape[0], P * factor + 1, H, W, 3, dtype=torch.uint8, device=frames.device)
    video[:, ::factor] = f5                                               # the originals: one strided copy
    K.mci_render(f5[:, :-1], f5[:, 1:], mvi, block, factor, video)
    if frames.dim() == 4:
        video, mvi, cost = video[0], mvi[0], cost[0]
    return {"video": video, "mvi": mvi, "cost": cost} if return_vectors else video


class FrameRateUpsampler:
    """interpolate_frames for a long video that arrives clip by clip (the FIFO result).  `update(frames)` continues the current video with a clip, uint8 [F, H, W, 3]
    (F >= 1), and returns the frames that became final: the in-between frames that lead from the last frame of the previous clip (carried on the device) to this
    clip, and this clip upsampled; the very first frame of a video comes with its first clip.  `new_video()` forgets the carried frame.  Every pair's frames come
    from its two frames alone: the pieces concatenate to the bits of one interpolate_frames call on the whole video.  Nothing waits for the device."""

    def __init__(self, factor=2, block=16, radius=16, bidirectional=True):
        check_factor(factor, "FrameRateUpsampler")
        check_block(block, radius, block, block, "FrameRateUpsampler")
        self.factor, self.block, self.radius, self.bidirectional = factor, block, radius, bool(bidirectional)
        self._last = None

    def update(self, frames):
        if isinstance(frames, torch.Tensor) and frames.dim() != 4:
            raise ValueError(f"FrameRateUpsampler.update: one video's clip [F, H, W, 3], got {tuple(frames.shape)}")
        check_pairs(frames, "FrameRateUpsampler.update", pairs_within=False)
        check_block(self.block, self.radius, frames.shape[1], frames.shape[2], "FrameRateUpsampler.update")
        if self._last is not None and self._last.shape[1:] != frames.shape[1:]:
            raise ValueError(f"FrameRateUpsampler.update: the video's frames are {tuple(self._last.shape[1:])}, this clip's {tuple(frames.shape[1:])}")
        seq = frames if self._last is None else torch.cat([self._last, frames])
        out = seq.clone() if seq.shape[0] < 2 else interpolate_frames(seq, self.factor, self.block, self.radius, self.bidirectional)
        if self._last is not None:
            out = out[1:]                                                 # the carried frame was returned with its own clip
        self._last = frames[-1:].clone()
        return out

    def new_video(self):
        self._last = None


def top_count(top_fraction, blocks):
    """ceil(top_fraction * blocks), at least 1 and at most `blocks`; a product that lands within 1e-9 above an integer counts as that integer (0.05 * 60)"""
    if not 0.0 < float(top_fraction) <= 1.0:
        raise ValueError(f"top_fraction must be in (0, 1], got {top_fraction!r}")
    return min(blocks, max(1, math.ceil(float(top_fraction) * blocks - 1e-9)))


def summarize(mv, sad, sad0, block, top_fraction=0.05):
    """Per-pair motion statistics from the results of block_motion, float64, on the tensors' device (any device): mv [.., Hb, Wb, 2], sad, sad0 [.., Hb, Wb] ->
    "magnitude": mean over blocks of sqrt(dy^2 + dx^2) in pixels; "magnitude_top": mean of the largest ceil(top_fraction * Hb * Wb) block magnitudes (what the
    common benchmarks threshold for their "dynamic degree"; the threshold is the caller's); "static_fraction": share of blocks with mv == 0; "flicker":
    sum(sad0) / (255 * Hb * Wb * block^2); "residual": the same with sad.  Each shaped like the leading axes."""
    if mv.dim() < 3 or mv.shape[-1] != 2 or sad.shape != mv.shape[:-1] or sad0.shape != sad.shape:
        raise ValueError(f"summarize: expected mv [.., Hb, Wb, 2] and sad, sad0 [.., Hb, Wb], got {tuple(mv.shape)}, {tuple(sad.shape)}, {tuple(sad0.shape)}")
    if block not in BLOCKS:
        raise ValueError(f"summarize: block must be one of {BLOCKS}, got {block!r}")
    n = mv.shape[-3] * mv.shape[-2]
    k = top_count(top_fraction, n)
    v = mv.to(torch.int64)
    mag = (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]).to(torch.float64).sqrt().flatten(-2)
    norm = 255.0 * n * block * block
    return {"magnitude": mag.mean(-1), "magnitude_top": mag.topk(k, dim=-1).values.mean(-1), "static_fraction": (mag == 0).to(torch.float64).mean(-1),
            "flicker": sad0.flatten(-2).sum(-1, dtype=torch.int64).to(torch.float64) / norm,
            "residual": sad.flatten(-2).sum(-1, dtype=torch.int64).to(torch.float64) / norm}
