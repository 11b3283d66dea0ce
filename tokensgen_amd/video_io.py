"""The two pixel ends of a run: decoded uint8 frames -> the [-1, 1] bf16 tensor `vae_encode_image` wants, and decoded bf16 frames -> display bytes.

Front end: the arithmetic of `load_video` (longvgen/data/long_video.py:28-76) after the container is decoded: frame index sampling (:37-51, `sample_frame_indices`),
then `video / 255.` -> resize -> crop / pad -> `* 2 - 1` (:61-76) with `resize_for_rectangle_crop` (longvgen/data/utils.py:112-140, bicubic, centre crop) or
`ResolutionControl.__call__` (utils.py:13-107, optional pad with -1, bilinear to exactly output_res), in one launch of tg_video_resample (csrc/video.hip).
`prepare_video` takes the uint8 [F, H, W, 3] frames a decoder delivers; `load_video` is the whole function for Motion-JPEG .avi files, decoded on the device by
tokensgen_amd.jpeg, and for numbered PNG sequences (tokensgen_amd.png, §8o); there is no decoder library here, so every other container is refused by
name.

STATED ASSUMPTION: torchvision 0.19.1 `resize` defaults to antialias=True and, on a float tensor, is
`F.interpolate(img, size, mode, align_corners=False, antialias=True)` without a clamp; torchvision's source is absent, so that call is taken as the definition and
`aa_weights` restates its filter (tests/test_video_io_cpu.py holds the restatement to F.interpolate on the CPU).

Back end: `VideoProcessor.postprocess_video` (the attribute the reference's pipeline carries; tokensgen_amd.fifo looks for `pipe.video_processor`), restated from
diffusers 0.31, source absent: VaeImageProcessor.denormalize on the bf16 tensor, then "pt" / "np" / "pil" as there, plus "uint8": the bytes `export_to_video` writes
from the "np" output, formed on the device (a quarter of the float32 transfer).  One launch of tg_video_to_uint8 each; no torch elementwise chain.

Not registered under the `longvgen.data` alias (tokensgen_amd.compat): the dataset classes are out of scope."""
import functools
import os
from types import SimpleNamespace

import numpy as np
import torch

from . import kernels as K
from .frames import gpu_device

MAX_TAPS = 64          # tg_video_resample refuses more (about 15x downscaling)


def sample_frame_indices(n_frames, avg_fps, nf_per_chunk, sample_fps=-1, start_t=0, end_t=-1, max_num_chunks=1):
    """long_video.py:37-51 — which decoded frames `load_video` keeps: `sample_fps` frames per second between start_t and end_t (seconds; -1: the clip's own rate / its
    end), cut to whole chunks of nf_per_chunk, at most max_num_chunks.  Returns an int64 numpy array; raises AssertionError where the reference does."""
    if sample_fps == -1:
        sample_fps = avg_fps
    if end_t == -1:
        end_t = n_frames / avg_fps
    else:
        end_t = min(n_frames / avg_fps, end_t)
    assert 0 <= start_t < end_t
    assert sample_fps > 0
    start_f, end_f = int(start_t * avg_fps), int(end_t * avg_fps)
    num_f = int((end_t - start_t) * sample_fps)
    idx = np.linspace(start_f, end_f, num_f, endpoint=False).astype(int)
    num_chunks = min(len(idx) // nf_per_chunk, max_num_chunks)
    idx = idx[:num_chunks * nf_per_chunk]
    assert len(idx) > 0, "sample_idx is empty!"
    return idx.astype(np.int64)


def _cubic(x, a=-0.5):
    x = np.abs(x)
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0, np.where(x < 2.0, ((a * x - 5.0 * a) * x + 8.0 * a) * x - 4.0 * a, 0.0))


def _triangle(x):
    return np.maximum(0.0, 1.0 - np.abs(x))


_FILTERS = {"bicubic": (4.0, _cubic), "bilinear": (2.0, _triangle)}


def aa_weights(n_in, n_out, mode):
    """The separable filter of F.interpolate(mode, align_corners=False, antialias=True) along one axis, n_in -> n_out samples, as tables:
    (first[n_out] int32, count[n_out] int32, weights[n_out, taps] fp32): output i = sum_k weights[i, k] * input[first[i] + k], k < count[i]; weights past count are 0.
    scale = n_in / n_out; support = isz / 2 * max(scale, 1) (isz 4 bicubic / 2 bilinear); centre c = scale (i + 0.5); taps int(c - support + 0.5) .. int(c + support
    + 0.5) clipped to the input; w = f((j - c + 0.5) / max(scale, 1)) normalised to sum 1 in fp64, stored as fp32.  Exact zeros at either end of a row are dropped (at
    scale 1 the bicubic row is the single tap of weight 1)."""
    if mode not in _FILTERS:
        raise ValueError(f"mode must be 'bicubic' or 'bilinear', got {mode!r}")
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError(f"aa_weights: sizes must be positive (n_in={n_in}, n_out={n_out})")
    isz, f = _FILTERS[mode]
    scale = n_in / n_out
    support = isz / 2.0 * scale if scale >= 1.0 else isz / 2.0
    inv = 1.0 / scale if scale >= 1.0 else 1.0
    rows, first = [], np.zeros(n_out, np.int32)
    for i in range(n_out):
        c = scale * (i + 0.5)
        xmin, xmax = max(0, int(c - support + 0.5)), min(n_in, int(c + support + 0.5))
        w = f((np.arange(xmin, xmax, dtype=np.float64) - c + 0.5) * inv)
        w = w / w.sum()
        nz = np.nonzero(w)[0]
        lo, hi = int(nz[0]), int(nz[-1]) + 1
        first[i] = xmin + lo
        rows.append(w[lo:hi])
    count = np.array([len(r) for r in rows], np.int32)
    weights = np.zeros((n_out, int(count.max())), np.float32)
    for i, r in enumerate(rows):
        weights[i, :len(r)] = r
    return first, count, weights


@functools.lru_cache(maxsize=64)
def _plan(in_hw, output_res, crop_to_fit, pad_to_fit):
    H, W = in_hw
    oh, ow = output_res
    if min(H, W, oh, ow) < 1:
        raise ValueError(f"resample_plan: sizes must be positive (in {in_hw}, out {output_res})")
    pad_y = pad_x = top = left = 0
    if crop_to_fit:                                              # resize_for_rectangle_crop(reshape_mode="center"), utils.py:112-140
        mode = "bicubic"
        if W / H > ow / oh:
            rh, rw = oh, int(W * oh / H)                         # :113-118
        else:
            rh, rw = int(H * ow / W), ow                         # :119-124
        if rh < oh or rw < ow:
            raise ValueError(f"resample_plan: {in_hw} -> {output_res} resizes to {(rh, rw)}, smaller than the crop window")
        top, left = (rh - oh) // 2, (rw - ow) // 2               # :129-136
    else:                                                        # ResolutionControl.__call__, utils.py:90-107
        mode = "bilinear"
        rh, rw = oh, ow
        if pad_to_fit:                                           # pad_with_ratio, :22-49: Pad((p, 0)) / Pad((0, p)) pads BOTH sides by p
            if H / W > oh / ow:
                pad_x = (int(H / oh * ow) - W) // 2              # :38-40
            else:
                pad_y = (int(W / ow * oh) - H) // 2              # :42-43
            if pad_x < 0 or pad_y < 0:
                raise ValueError(f"resample_plan: {in_hw} -> {output_res} asks for a negative pad")
    y0, ny, wy = aa_weights(H + 2 * pad_y, rh, mode)
    x0, nx, wx = aa_weights(W + 2 * pad_x, rw, mode)
    y0, ny, wy = y0[top:top + oh] - np.int32(pad_y), ny[top:top + oh], wy[top:top + oh]
    x0, nx, wx = x0[left:left + ow] - np.int32(pad_x), nx[left:left + ow], wx[left:left + ow]
    wy, wx = np.ascontiguousarray(wy[:, :int(ny.max())]), np.ascontiguousarray(wx[:, :int(nx.max())])
    if wy.shape[1] > MAX_TAPS or wx.shape[1] > MAX_TAPS:
        raise ValueError(f"resample_plan: {in_hw} -> {(rh, rw)} needs {wy.shape[1]} x {wx.shape[1]} taps; tg_video_resample takes at most {MAX_TAPS} per axis")
    tables = tuple(np.ascontiguousarray(t) for t in (y0, ny, wy, x0, nx, wx))
    for t in tables:
        t.setflags(write=False)
    return SimpleNamespace(in_hw=(H, W), output_res=(oh, ow), mode=mode, resized_hw=(rh, rw), top=top, left=left, pad_y=pad_y, pad_x=pad_x,
                           padded_hw=(H + 2 * pad_y, W + 2 * pad_x), taps=(wy.shape[1], wx.shape[1]), tables=tables, _device={})


def resample_plan(in_hw, output_res=(480, 720), crop_to_fit=False, pad_to_fit=False):
    """Pure host plan of one prepare_video shape (cached per shape): resized_hw, top / left crop offsets, pad_y / pad_x (each side), padded_hw, mode, taps and
    tables = (y0, ny, wy, x0, nx, wx) of the CROPPED window, first indices relative to the UNPADDED source (negative inside the pad).
    crop_to_fit: utils.py:112-140 — bicubic to cover output_res (`int(...)` truncation of :116 / :122), centre crop (`delta // 2`, :136); pad_to_fit is ignored, as in
    long_video.py:66-74.  Otherwise utils.py:90-107: optional pad (`(nw - iw) // 2` on both sides, :37-43), then bilinear to exactly output_res (the aspect ratio
    changes unless padded)."""
    return _plan((int(in_hw[0]), int(in_hw[1])), (int(output_res[0]), int(output_res[1])), bool(crop_to_fit), bool(pad_to_fit) and not crop_to_fit)


def _device_tables(plan, device):
    key = (device.type, device.index)
    if key not in plan._device:
        plan._device[key] = tuple(torch.tensor(t, device=device) for t in plan.tables)
    return plan._device[key]


def prepare_video(frames_u8, output_res=(480, 720), crop_to_fit=False, pad_to_fit=False, device=None):
    """Decoded frames, uint8 [F, H, W, 3] (torch tensor or numpy array), -> bf16 [1, F, 3, oh, ow] in [-1, 1] on the GPU: what `load_video` returns
    (long_video.py:61-76) and `vae_encode_image` / `pipe(frames=...)` take.  See resample_plan for the two branches.  The result does not depend on how many frames one
    call carries.  Raises RuntimeError without a GPU."""
    if isinstance(frames_u8, np.ndarray):
        frames_u8 = torch.from_numpy(frames_u8)
    if not isinstance(frames_u8, torch.Tensor) or frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[-1] != 3:
        raise TypeError("prepare_video: expected uint8 frames [F, H, W, 3]")
    dev = gpu_device(device if device is not None else (frames_u8.device if frames_u8.is_cuda else None), "tokensgen_amd.video_io")
    plan = resample_plan(frames_u8.shape[1:3], output_res, crop_to_fit, pad_to_fit)
    out = K.video_resample(frames_u8.to(dev).contiguous(), _device_tables(plan, dev), *plan.output_res)
    return out[None]


_LAYOUTS = {"bcthw": 1, "bfchw": 2}


def frames_to_uint8(video, layout="bcthw", rounding=0):
    """bf16 frames in [-1, 1] -> uint8 [B, T, H, W, 3] on the device.  layout "bcthw": [B, 3, T, H, W] (vae.decode); "bfchw": [B, F, 3, H, W] (a source video).
    rounding 0 truncates (`export_to_video` on the "np" output), 1 rounds half to even (`numpy_to_pil`).  NaN gives 0."""
    if layout not in _LAYOUTS:
        raise ValueError(f"layout must be one of {sorted(_LAYOUTS)}, got {layout!r}")
    if rounding not in (0, 1):
        raise ValueError("rounding must be 0 (truncate) or 1 (half to even)")
    return K.video_to_uint8(video, _LAYOUTS[layout], K.VIDEO_U8, rounding)


class VideoProcessor:
    """`pipe.video_processor = VideoProcessor()`: the post-processing the reference pipeline's attribute of that name does (diffusers 0.31 VideoProcessor, restated,
    source absent).  The pipeline carries none by default: the FIFO driver then returns the decoded bf16 [B, 3, T, H, W] as before.

    frame_rate_factor n > 1 (2 .. 8; not in diffusers) raises the frame rate of the byte outputs by motion-compensated interpolation on the device
    (tokensgen_amd.motion.interpolate_frames with `block`, `radius`, `bidirectional`): T frames become (T - 1) n + 1, the originals unchanged at
    every n-th place, and the caller writes them at `fps = output_fps * n`.  With the default, 1, every output is what it was and the motion code is never imported.

    `set_color_match("meanstd" | "histogram", anchor=None, anchor_frames=8, strength=1.0, window=1)` (not in diffusers; the constructor's parameter list stays what it
    was) makes the byte outputs colour-matched to an anchor on the device, before the interpolation, whose motion search assumes constant brightness
    (tokensgen_amd.color.match_colors); it returns the processor, so `VideoProcessor(frame_rate_factor=2).set_color_match("meanstd")` reads in one line.
    Without it (`color_match` is None) every output is what it was and the colour code is never imported."""

    color_match, color_anchor, color_anchor_frames, color_strength, color_window = None, None, 8, 1.0, 1

    def __init__(self, frame_rate_factor=1, block=16, radius=16, bidirectional=True):
        if not isinstance(frame_rate_factor, int) or isinstance(frame_rate_factor, bool) or not 1 <= frame_rate_factor <= 8:
            raise ValueError(f"VideoProcessor: frame_rate_factor must be an integer in 1..8, got {frame_rate_factor!r}")
        self.frame_rate_factor, self.block, self.radius, self.bidirectional = frame_rate_factor, block, radius, bidirectional
        if frame_rate_factor > 1:
            from . import motion
            motion.check_block(block, radius, block, block, "VideoProcessor")

    def set_color_match(self, mode, anchor=None, anchor_frames=8, strength=1.0, window=1):
        """Colour-match the "uint8" and "pil" outputs (mode "meanstd" or "histogram"; None switches it off again).  anchor: None (each video's own first
        anchor_frames frames), uint8 frames of any size, or an int64 [3, 256] histogram.  Every argument is checked here, before any kernel call.  Returns self."""
        if mode is not None:
            from . import color
            color.check_params(mode, strength, window, 4.0, "VideoProcessor.set_color_match")
            color.check_anchor_frames(anchor_frames, "VideoProcessor.set_color_match")
            color.check_anchor(anchor, "VideoProcessor.set_color_match")
        self.color_match, self.color_anchor, self.color_anchor_frames, self.color_strength, self.color_window = mode, anchor, anchor_frames, strength, window
        return self

    def _upsample(self, frames_u8):
        if self.color_match is not None:
            from .color import match_colors
            frames_u8 = match_colors(frames_u8, self.color_anchor, self.color_anchor_frames, self.color_match, self.color_strength, self.color_window)
        if self.frame_rate_factor == 1:
            return frames_u8
        from .motion import interpolate_frames
        return interpolate_frames(frames_u8, self.frame_rate_factor, self.block, self.radius, self.bidirectional)

    def postprocess_video(self, video, output_type="np"):
        """video bf16 [B, 3, T, H, W] in [-1, 1].  "pt": [B, T, 3, H, W] in the input dtype, in [0, 1]; "np": float32 numpy [B, T, H, W, 3] in [0, 1]; "pil": B lists of T
        PIL images (rounded half to even); "uint8": uint8 tensor [B, T, H, W, 3] on the device, truncated: `(np_output * 255).astype(uint8)` byte for byte.
        With frame_rate_factor > 1 "uint8" is interpolated, "pil" is interpolated from its rounded bytes, and the float outputs are refused; with color_match the
        bytes are colour-matched first, and the float outputs are refused as well."""
        if output_type in ("pt", "np") and self.color_match is not None:
            raise ValueError(f"color_match {self.color_match!r} maps bytes: ask for output_type \"uint8\" (or \"pil\"), not {output_type!r}")
        if output_type in ("pt", "np") and self.frame_rate_factor > 1:
            raise ValueError(f"frame_rate_factor {self.frame_rate_factor} interpolates bytes: ask for output_type \"uint8\" (or \"pil\"), not {output_type!r}")
        if output_type == "pt":
            return K.video_to_uint8(video, 1, K.VIDEO_BF16_PLANAR)
        if output_type == "np":
            return K.video_to_uint8(video, 1, K.VIDEO_F32).cpu().numpy()
        if output_type == "uint8":
            return self._upsample(K.video_to_uint8(video, 1, K.VIDEO_U8, 0))
        if output_type == "pil":
            from PIL import Image
            by = self._upsample(K.video_to_uint8(video, 1, K.VIDEO_U8, 1)).cpu().numpy()
            return [[Image.fromarray(frame) for frame in clip] for clip in by]
        raise ValueError(f"output_type must be one of 'pt', 'np', 'pil', 'uint8'; got {output_type!r}")


def load_video(video_path, output_res, nf_per_chunk, pad_to_fit, sample_fps, start_t, end_t, max_num_chunks, crop_to_fit=False, device=None):
    """The first step of the reference's entry script (`load_video`, long_video.py:28-76, same parameter order): a Motion-JPEG .avi file (one that `export_to_video`
    wrote, or any baseline MJPG AVI) -> bf16 [1, F, 3, oh, ow] in [-1, 1] on the device.  The file's index is read on the host, `sample_frame_indices` picks the
    frames, they are decoded on the device (tokensgen_amd.jpeg.MJPEGReader; a file without restart markers in parallel inside each frame, §8m) and go
    through `prepare_video`.  A path with the suffix .png is the pattern of a numbered sequence of PNG frames ("clip/frame_{:05d}.png", what `save_png_sequence` writes
    and any tool can produce from an .mp4), read at 8 frames a second, the rate `export_to_video` writes by default: `load_image_sequence`, DESIGN.md §8o.  Any other
    suffix is refused: there is no H.264 / mp4 decoder here.  The JPEG or PNG code is imported by the first call."""
    if os.path.splitext(str(video_path))[1].lower() == ".png":
        return load_image_sequence(video_path, output_res, nf_per_chunk, pad_to_fit, sample_fps, start_t, end_t, max_num_chunks, crop_to_fit, device)
    from . import jpeg
    return jpeg.load_video(video_path, output_res, nf_per_chunk, pad_to_fit, sample_fps, start_t, end_t, max_num_chunks, crop_to_fit, device)


def load_image_sequence(video_path, output_res, nf_per_chunk, pad_to_fit, sample_fps, start_t, end_t, max_num_chunks, crop_to_fit=False, device=None, fps=8, start=0):
    """`load_video` for a numbered sequence of PNG frames: video_path is the pattern ("clip/frame_{:05d}.png"), `start` the first number; the files that exist in a row
    from there are the clip.  A sequence has no rate of its own: `fps` says what the frames are, and `sample_frame_indices` works with it as with a container's.  The
    frames asked for are decoded on the device (tokensgen_amd.png.PNGSequenceReader) and go through `prepare_video`."""
    from . import png
    with png.PNGSequenceReader(video_path, fps, start, device) as r:
        idx = sample_frame_indices(len(r), r.get_avg_fps(), nf_per_chunk, sample_fps, start_t, end_t, max_num_chunks)
        frames = r.get_batch(idx.tolist())
    return prepare_video(frames, output_res, crop_to_fit, pad_to_fit, device)


def export_to_video(video_frames, output_video_path, fps=8, quality=90):
    """The last step of the reference's entry script (diffusers.utils.export_to_video, same argument order): the "uint8" output of `postprocess_video`, uint8
    [T, H, W, 3] or [1, T, H, W, 3] on the device, as a Motion-JPEG .avi file (tokensgen_amd.jpeg, encoded on the device).  quality is the JPEG
    quality, 1 .. 100.  Any other suffix is refused: there is no H.264 / mp4 encoder here.  Returns the path.  The JPEG code is imported by the first call."""
    from . import jpeg
    return jpeg.export_to_video(video_frames, output_video_path, fps, quality)
