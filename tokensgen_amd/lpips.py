"""LPIPS (VGG16, version 0.1) on the GPU: the third figure of the reconstruction triple next to PSNR and SSIM (tokensgen_amd.metrics).  The reference's call site,
longvgen/metrics/lpips.py:12-47, is `model(img2, img)` on an `lpips.LPIPS(net='vgg')` object; neither that package nor torchvision is needed here.  The definition
is restated in DESIGN.md §8d (a restatement: their sources are absent) and in tests/lpips_ref.py.

    from tokensgen_amd.lpips import LPIPS, video_lpips
    model = LPIPS.from_files("vgg16-397923af.pth", "lpips_vgg.pth")          # torchvision's VGG16 weights and the lpips package's weights/v0.1/vgg.pth
    d = model(in0, in1)                                                       # (N, 3, H, W) in [-1, 1] on the GPU -> (N, 1, 1, 1) float32
    m = video_lpips(frames_a, frames_b, model)                                # uint8 [B, T, H, W, 3] ... -> {"lpips": float64 [B, T], "lpips_pooled": 0-dim}

Launches per chunk of frames: tg_lpips_conv_in per clip (pixel ends, scaling layer, conv1_1, ReLU), 12 x tg_conv3d_cl (bf16, fp32 accumulation; the frame axis is
its T), 4 x tg_relu_maxpool2_cl, 7 x tg_relu_cl (after the convolutions that feed another convolution), 5 x tg_lpips_head (ReLU on load).  Both clips go through
the trunk as ONE batch of 2 n images.

STATED DEVIATION: trunk activations and the weights and biases of the 12 MFMA convolutions are bf16 with fp32 accumulation; conv1_1 and the head are fp32 or better.
The reference runs fp32.  Per-frame values may differ in the last bf16-induced digits between chunkings (the convolution planner picks its kernel by launch size);
two identical calls are bitwise equal.  No weights ship with the project.  There is no CPU path."""
import torch

from . import kernels as K

BF16 = torch.bfloat16
# torchvision vgg16().features: index of every convolution, (Cin, Cout), and the stage (tap) it belongs to; a 2 x 2 max-pool stands before stages 2..5
CONVS = ((0, 3, 64, 1), (2, 64, 64, 1), (5, 64, 128, 2), (7, 128, 128, 2), (10, 128, 256, 3), (12, 256, 256, 3), (14, 256, 256, 3), (17, 256, 512, 4),
         (19, 512, 512, 4), (21, 512, 512, 4), (24, 512, 512, 5), (26, 512, 512, 5), (28, 512, 512, 5))
TAP_CHANNELS = (64, 128, 256, 512, 512)
_LAST_OF_STAGE = {2, 7, 14, 21, 28}


def _pad_to(n, m):
    return (n + m - 1) // m * m


def canonical_state_dict(sd):
    """Any mix of the accepted key layouts -> {"features.N.weight" / ".bias", "lin{k}.weight"}:
    torchvision `features.N.*`; a full lpips.LPIPS state dict `net.slice{s}.N.*`, `lin{k}.model.1.weight` (duplicates under `lins.{k}.model.1.weight`;
    `scaling_layer.*` ignored); the package's vgg.pth: the five `lin{k}.model.1.weight`.  Returns (canonical dict, unexpected keys)."""
    out, unexpected = {}, []
    conv_idx = {str(c[0]) for c in CONVS}
    for k, v in sd.items():
        parts = k.split(".")
        if parts[0] == "scaling_layer":
            continue
        if parts[0] == "features" and len(parts) == 3 and parts[1] in conv_idx and parts[2] in ("weight", "bias"):
            out[k] = v
        elif parts[0] == "net" and len(parts) == 4 and parts[1] in ("slice1", "slice2", "slice3", "slice4", "slice5") and parts[2] in conv_idx and \
                parts[3] in ("weight", "bias"):
            out[f"features.{parts[2]}.{parts[3]}"] = v
        elif len(parts) == 4 and parts[0] in ("lin0", "lin1", "lin2", "lin3", "lin4") and parts[1:] == ["model", "1", "weight"]:
            out[f"{parts[0]}.weight"] = v
        elif len(parts) == 5 and parts[0] == "lins" and parts[1] in "01234" and len(parts[1]) == 1 and parts[2:] == ["model", "1", "weight"]:
            out.setdefault(f"lin{parts[1]}.weight", v)
        else:
            unexpected.append(k)
    return out, unexpected


def expected_shapes():
    want = {}
    for idx, ci, co, _ in CONVS:
        want[f"features.{idx}.weight"], want[f"features.{idx}.bias"] = (co, ci, 3, 3), (co,)
    for k, c in enumerate(TAP_CHANNELS):
        want[f"lin{k}.weight"] = (1, c, 1, 1)
    return want


def pack_conv(weight, bias, device=None):
    """[Cout, Cin, 3, 3] / [Cout] -> tg_conv3d_cl's bf16 [Cout_pad, 9, Cin] (Cout_pad a multiple of 128) and bf16 [Cout_pad]"""
    co, ci = weight.shape[:2]
    cp = _pad_to(co, 128)
    w = torch.zeros(cp, 9, ci, dtype=BF16, device=device or weight.device)
    w[:co] = weight.reshape(co, ci, 9).permute(0, 2, 1).to(w.device, BF16)
    b = torch.zeros(cp, dtype=BF16, device=w.device)
    b[:co] = bias.to(w.device, BF16)
    return w.contiguous(), b


def _load_file(path):
    if str(path).endswith(".safetensors"):
        from safetensors.torch import load_file
        return load_file(str(path))
    sd = torch.load(str(path), map_location="cpu", weights_only=True)
    return sd.get("state_dict", sd) if isinstance(sd, dict) else sd


class LPIPS:
    """lpips.LPIPS(net='vgg', version='0.1', lpips=True, spatial=False) in eval mode, on one GPU."""

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        self.frames_per_launch = 8         # frames of EACH clip per trunk batch (conv1 activations of 2 x 8 frames of 480 x 720: 0.7 GB per buffer)
        self._w = None

    @classmethod
    def from_files(cls, vgg_path, lin_path=None, device="cuda"):
        """vgg_path: torchvision's VGG16 weights or a full lpips.LPIPS state dict; lin_path: the lpips package's weights/v0.1/vgg.pth (.pth / .pt / .safetensors)"""
        sd = dict(_load_file(vgg_path))
        if lin_path is not None:
            sd.update(_load_file(lin_path))
        m = cls(device)
        m.load_state_dict(sd)
        return m

    def load_state_dict(self, sd, strict=True):
        canon, unexpected = canonical_state_dict(sd)
        unexpected = [k for k in unexpected if not k.startswith("classifier.")]            # torchvision's file carries the classifier: not part of the trunk
        want = expected_shapes()
        missing = [k for k in want if k not in canon]
        bad = [k for k in want if k in canon and tuple(canon[k].shape) != want[k]]
        if missing or bad or (strict and unexpected):
            raise RuntimeError(f"LPIPS.load_state_dict: missing {missing[:4]}, unexpected {unexpected[:4]}, shape mismatch {bad[:4]}")
        dev = self.device
        w = {"in.weight": canon["features.0.weight"].detach().to(dev, torch.float32).reshape(64, 27).contiguous(),
             "in.bias": canon["features.0.bias"].detach().to(dev, torch.float32).contiguous()}
        for idx, ci, co, _ in CONVS[1:]:
            w[f"{idx}.weight"], w[f"{idx}.bias"] = pack_conv(canon[f"features.{idx}.weight"].detach(), canon[f"features.{idx}.bias"].detach(), dev)
        for k, c in enumerate(TAP_CHANNELS):
            w[f"lin{k}"] = canon[f"lin{k}.weight"].detach().to(dev, torch.float32).reshape(c).contiguous()
        self._w = w
        return unexpected

    # ---- the trunk and the five heads on one chunk ------------------------------------------------------------------------------------------------------------
    def max_frames(self, h, w):
        """images per trunk batch that tg_conv3d_cl's 32-bit-offset guard allows: (T + 2) h w 64 < 2^31 at the widest layer"""
        return ((1 << 31) - 1) // (h * w * 64) - 2

    def _taps(self, x, n):
        """x: conv1_1's output for 2 n images [2 n, h, w, 64] (a's images, then b's) -> float64 [5, n]: per tap the spatial MEAN of the distance"""
        w = self._w
        out = []
        for idx, ci, co, stage in CONVS[1:]:
            if idx in (5, 10, 17, 24):
                x = K.relu_maxpool2_cl(x)
            x = K.conv3d_cl(x, w[f"{idx}.weight"], w[f"{idx}.bias"], co, 1, 3, 3, pad=1)
            if idx in _LAST_OF_STAGE:
                out.append(K.lpips_head(x[:n], x[n:], w[f"lin{stage - 1}"], relu_on_load=True) / float(x.shape[1] * x.shape[2]))
            else:
                K.relu_cl_(x)
        return torch.stack(out)

    def per_frame(self, a, b, layout, crop_border=0, normalize=False):
        """float64 [5, n_outer, n_inner]: the five per-tap values of every image pair of two equally shaped batches in one of kernels.IMAGE_LAYOUTS"""
        if self._w is None:
            raise RuntimeError("LPIPS: no weights loaded (load_state_dict / from_files)")
        for t in (a, b):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise RuntimeError("LPIPS: expected GPU tensors (tokensgen_amd has no CPU fallback)")
        if a.shape != b.shape or a.dtype != b.dtype:
            raise ValueError(f"the two inputs differ: {tuple(a.shape)} {a.dtype} and {tuple(b.shape)} {b.dtype}")
        (n_outer, n_inner, _, H, W), _ = K._image_strides(a, layout)
        h, wd = H - 2 * int(crop_border), W - 2 * int(crop_border)
        if n_outer * n_inner < 1:
            raise ValueError("no images")
        if h < K.LPIPS_MIN_SIDE or wd < K.LPIPS_MIN_SIDE:
            raise ValueError(f"a {H} x {W} image with crop_border {crop_border} is smaller than {K.LPIPS_MIN_SIDE} x {K.LPIPS_MIN_SIDE}")
        step = min(int(self.frames_per_launch), self.max_frames(h, wd) // 2)
        if step < 1:
            raise ValueError(f"a {h} x {wd} image is too large for tg_conv3d_cl's 32-bit offsets")
        K.zero_page(a.device)
        rows = []
        for o in range(n_outer):
            cols = []
            for i0 in range(0, n_inner, step):
                n = min(step, n_inner - i0)
                x = torch.empty(2 * n, h, wd, 64, dtype=BF16, device=a.device)
                K.lpips_conv_in(a, layout, self._w["in.weight"], self._w["in.bias"], x[:n], crop_border, normalize, outer=o, inner=(i0, n))
                K.lpips_conv_in(b, layout, self._w["in.weight"], self._w["in.bias"], x[n:], crop_border, normalize, outer=o, inner=(i0, n))
                cols.append(self._taps(x, n))
            rows.append(torch.cat(cols, dim=1))
        return torch.stack(rows, dim=1)

    def __call__(self, in0, in1, normalize=False, retPerLayer=False):
        """lpips.LPIPS.forward: in0, in1 GPU fp32 / bf16 (N, 3, H, W) in [-1, 1] ([0, 1] with normalize), views allowed -> (N, 1, 1, 1) float32; with retPerLayer
        also the list of the five per-tap (N, 1, 1, 1) tensors."""
        for t in (in0, in1):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise RuntimeError("LPIPS: expected GPU tensors (tokensgen_amd has no CPU fallback)")
            if t.dim() != 4 or t.shape[1] != 3 or t.dtype not in (torch.float32, BF16):
                raise ValueError(f"expected fp32 / bf16 (N, 3, H, W), got {tuple(t.shape)} {t.dtype}")
        taps = self.per_frame(in0, in1, "chw", 0, normalize)[:, 0]                       # [5, N]
        val = taps.sum(0).to(torch.float32).view(-1, 1, 1, 1)
        if retPerLayer:
            return val, [t.to(torch.float32).view(-1, 1, 1, 1) for t in taps]
        return val

    forward = __call__


def video_lpips(a, b, model, crop_border=0):
    """Per-frame and pooled LPIPS of two equally shaped videos, the input layouts of metrics.video_metrics: uint8 [B, T, H, W, 3] / [F, H, W, 3] (display bytes, read
    as 2 (v / 255) - 1) or fp32 / bf16 in [0, 1] as (n, 3, h, w) / [B, 3, T, H, W] (views allowed).  Returns {"lpips": float64 per frame, shaped [B, T] / [F] / [n],
    "lpips_taps": the five per-tap values [5, ...], "lpips_pooled": their mean over the frames, 0-dim}.  Frames go through the trunk in chunks of
    model.frames_per_launch per clip (a remainder chunk is legal).  Nothing here waits for the device."""
    from .metrics import _layout
    assert isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.shape == b.shape, \
        f"Image shapes are different: {getattr(a, 'shape', None)}, {getattr(b, 'shape', None)}."
    layout = _layout(a)
    taps = model.per_frame(a, b, layout, crop_border, normalize=a.dtype != torch.uint8)
    if a.dim() == 4:
        taps = taps[:, 0]
    val = taps.sum(0)
    return {"lpips": val, "lpips_taps": taps, "lpips_pooled": val.mean()}
