"""fp64 restatements for tokensgen_amd.video_io, written from the reference's arithmetic (no product code is imported here):

  dense_aa / resize_geometry / prepare_ref   `load_video` after decoding (longvgen/data/long_video.py:61-76) with resize_for_rectangle_crop / ResolutionControl
                                             (longvgen/data/utils.py:13-140), the resize taken as F.interpolate(align_corners=False, antialias=True) — the filter as a
                                             dense fp64 matrix per axis — plus the magnitude sum `A` the derived error bound of tests/test_video_io_gpu.py scales with
  display_ref                                diffusers 0.31 VaeImageProcessor.denormalize on the bf16 tensor ((v * 0.5 + 0.5).clamp(0, 1), torch's own two bf16
                                             operations on the CPU), then `export_to_video`'s truncation or `numpy_to_pil`'s rounding (restated, source absent)
"""
import math

import numpy as np
import torch

F64 = torch.float64


def _cubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    if x < 2.0:
        return a * x ** 3 - 5.0 * a * x * x + 8.0 * a * x - 4.0 * a
    return 0.0


def _triangle(x):
    return max(0.0, 1.0 - abs(x))


def dense_aa(n_in, n_out, mode):
    """[n_out, n_in] fp64: row i holds the normalised antialias filter of output sample i."""
    isz, f = {"bicubic": (4, _cubic), "bilinear": (2, _triangle)}[mode]
    scale = n_in / n_out
    support = isz / 2 * scale if scale >= 1 else isz / 2
    inv = 1 / scale if scale >= 1 else 1.0
    M = torch.zeros(n_out, n_in, dtype=F64)
    for i in range(n_out):
        c = scale * (i + 0.5)
        xmin, xmax = max(0, int(c - support + 0.5)), min(n_in, int(c + support + 0.5))
        w = [f((j - c + 0.5) * inv) for j in range(xmin, xmax)]
        tot = math.fsum(w)
        M[i, xmin:xmax] = torch.tensor([v / tot for v in w], dtype=F64)
    return M


def densify(first, count, weights, n_in):
    """The (first, count, weights) tables of tokensgen_amd.video_io.aa_weights as a dense [n_out, n_in] fp64 matrix; first may be negative (a pad): such taps fall away."""
    M = torch.zeros(len(first), n_in, dtype=F64)
    for i, (a, n) in enumerate(zip(first.tolist(), count.tolist())):
        for k in range(n):
            if 0 <= a + k < n_in:
                M[i, a + k] = float(weights[i, k])
    return M


def resize_geometry(in_hw, output_res, crop_to_fit, pad_to_fit):
    """(mode, resized (h, w), (top, left), (pad_y, pad_x)) by the integer arithmetic of utils.py:113-124, :136 and :37-43."""
    (H, W), (oh, ow) = in_hw, output_res
    if crop_to_fit:
        if W / H > ow / oh:
            rh, rw = oh, int(W * oh / H)
        else:
            rh, rw = int(H * ow / W), ow
        return "bicubic", (rh, rw), ((rh - oh) // 2, (rw - ow) // 2), (0, 0)
    py = px = 0
    if pad_to_fit:
        if H / W > oh / ow:
            px = (int(H / oh * ow) - W) // 2
        else:
            py = (int(W / ow * oh) - H) // 2
    return "bilinear", (oh, ow), (0, 0), (py, px)


def operators(in_hw, output_res, crop_to_fit=False, pad_to_fit=False):
    """(Dy [oh, H], Dx [ow, W]) fp64: out = Dy @ img @ Dx^T per channel; the crop is a row slice, the zero pad a column slice."""
    mode, (rh, rw), (top, left), (py, px) = resize_geometry(in_hw, output_res, crop_to_fit, pad_to_fit)
    H, W = in_hw
    oh, ow = output_res
    Dy = dense_aa(H + 2 * py, rh, mode)[top:top + oh, py:py + H]
    Dx = dense_aa(W + 2 * px, rw, mode)[left:left + ow, px:px + W]
    return Dy, Dx


def prepare_ref(frames_u8, output_res, crop_to_fit=False, pad_to_fit=False):
    """frames uint8 [F, H, W, 3] -> (ref, A, taps) fp64 [1, F, 3, oh, ow]: ref = 2 Dy (u8 / 255) Dx^T - 1, A = |Dy| (u8 / 255) |Dx|^T, taps = (max taps per output
    row, per output column)."""
    Dy, Dx = operators(tuple(frames_u8.shape[1:3]), tuple(output_res), crop_to_fit, pad_to_fit)
    img = frames_u8.to("cpu", F64).permute(0, 3, 1, 2) / 255.0
    lin = Dy @ img @ Dx.T
    mag = Dy.abs() @ img @ Dx.abs().T
    taps = (int((Dy != 0).sum(1).max()), int((Dx != 0).sum(1).max()))
    return (2.0 * lin - 1.0)[None], mag[None], taps


def display_unit_ref(v_bf16):
    """VaeImageProcessor.denormalize on the CPU in the tensor's dtype: bf16 in, bf16 out."""
    v = v_bf16.detach().cpu()
    assert v.dtype == torch.bfloat16
    return (v * 0.5 + 0.5).clamp(0, 1)


def display_ref(v_bf16, rounding):
    """bf16 (any shape) -> uint8 of the same shape: rounding 0 truncates float(r) * 255, rounding 1 rounds it half to even; NaN gives 0."""
    x = display_unit_ref(v_bf16).float().numpy() * np.float32(255.0)
    x = np.where(np.isnan(x), np.float32(0.0), x)
    x = np.rint(x) if rounding else np.trunc(x)
    return torch.from_numpy(x.astype(np.uint8))


def all_bf16_patterns():
    """All 65 536 bf16 bit patterns as a bf16 tensor [65536] (NaNs and infinities included)."""
    return torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
