"""LPIPS(net='vgg', version='0.1', lpips=True, spatial=False).forward in eval mode, restated with F.conv2d (the `lpips` package and torchvision are absent: a
restatement of their definition), the yardstick of tokensgen_amd.lpips:

  x = (x - shift) / scale per channel, shift = (-0.030, -0.088, -0.188), scale = (0.458, 0.448, 0.450)              (inputs in [-1, 1]; `normalize`: x = 2 x - 1 first)
  torchvision vgg16().features[0:30]: 3 x 3 convolutions, stride 1, zero padding 1, bias, ReLU; MaxPool2d(2, 2) (floor) before stages 2..5; taps after the last ReLU
  of each stage; per tap f = feat / (sqrt(sum_c feat^2) + 1e-10), d = (f0 - f1)^2, r_k = mean_hw sum_c w_k[c] d[c]; the result is sum_k r_k, shape (N, 1, 1, 1).

`weights` is the canonical dict {"features.N.weight" [Cout, Cin, 3, 3], "features.N.bias" [Cout], "lin{k}.weight" [1, C, 1, 1]} of random_weights()."""
import math

import torch
import torch.nn.functional as F

SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
# (features index, Cin, Cout, stage)
CONVS = ((0, 3, 64, 1), (2, 64, 64, 1), (5, 64, 128, 2), (7, 128, 128, 2), (10, 128, 256, 3), (12, 256, 256, 3), (14, 256, 256, 3), (17, 256, 512, 4),
         (19, 512, 512, 4), (21, 512, 512, 4), (24, 512, 512, 5), (26, 512, 512, 5), (28, 512, 512, 5))
TAP_CHANNELS = (64, 128, 256, 512, 512)
LAST_OF_STAGE = (2, 7, 14, 21, 28)
FIRST_OF_STAGE = (5, 10, 17, 24)                # a pool stands in front of these
DETERMINISTIC = True                            # on a GPU: deterministic convolution algorithms, so that a test's figures repeat from run to run (tools/bench_lpips.py turns it off)


def random_weights(seed):
    """He-normal convolution weights (std = sqrt(2 / (9 Cin))), biases 0.05 N(0, 1), lin weights uniform in [0, 2 / C] (non-negative as the trained ones are); fp32"""
    g = torch.Generator().manual_seed(seed)
    w = {}
    for idx, ci, co, _ in CONVS:
        w[f"features.{idx}.weight"] = torch.randn(co, ci, 3, 3, generator=g) * math.sqrt(2.0 / (9 * ci))
        w[f"features.{idx}.bias"] = 0.05 * torch.randn(co, generator=g)
    for k, c in enumerate(TAP_CHANNELS):
        w[f"lin{k}.weight"] = torch.rand(1, c, 1, 1, generator=g) * (2.0 / c)
    return w


def as_state_dict(w):
    """random_weights' dict under the names a user's files carry: torchvision's `features.N.*` and the lpips package's `lin{k}.model.1.weight`"""
    return {(k if k.startswith("features.") else k.replace(".weight", ".model.1.weight")): v for k, v in w.items()}


def scaling_layer(x, normalize=False):
    if normalize:
        x = 2 * x - 1
    shift = torch.tensor(SHIFT, dtype=x.dtype, device=x.device).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=x.dtype, device=x.device).view(1, 3, 1, 1)
    return (x - shift) / scale


def _bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def trunk(x, weights, dtype, bf16=False, drop_relu_after=None, ceil_mode=False):
    """x (N, 3, H, W) in scaled space -> the five taps.  bf16: weights, biases and every activation above conv1_1 rounded to bf16 where tokensgen_amd.lpips rounds them
    (conv1_1's weights and arithmetic stay unrounded, its output is rounded after the ReLU; a later convolution's output is rounded before the ReLU, which commutes).
    drop_relu_after / ceil_mode: the two wrong trunks of the negative controls."""
    if not DETERMINISTIC or not x.is_cuda:
        return _trunk(x, weights, dtype, bf16, drop_relu_after, ceil_mode)
    with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        return _trunk(x, weights, dtype, bf16, drop_relu_after, ceil_mode)


def _trunk(x, weights, dtype, bf16, drop_relu_after, ceil_mode):
    taps = []
    for idx, ci, co, _ in CONVS:
        if idx in FIRST_OF_STAGE:
            x = F.max_pool2d(x, 2, 2, ceil_mode=ceil_mode)
        w, b = weights[f"features.{idx}.weight"].to(x.device, dtype), weights[f"features.{idx}.bias"].to(x.device, dtype)
        if bf16 and idx != 0:
            w, b = _bf16(w), _bf16(b)
        x = F.conv2d(x, w, b, stride=1, padding=1)
        if bf16:
            x = _bf16(x)
        if idx != drop_relu_after:
            x = F.relu(x)
        if idx in LAST_OF_STAGE:
            taps.append(x)
    return taps


def head(f0, f1, w):
    """one tap: (N, C, H, W) features and the lin weight [1, C, 1, 1] -> (N, 1, 1, 1)"""
    n0 = f0 / (torch.sqrt(torch.sum(f0 ** 2, dim=1, keepdim=True)) + 1e-10)
    n1 = f1 / (torch.sqrt(torch.sum(f1 ** 2, dim=1, keepdim=True)) + 1e-10)
    return ((n0 - n1) ** 2 * w.to(f0.device, f0.dtype)).sum(dim=1, keepdim=True).mean([2, 3], keepdim=True)


def lpips_ref(in0, in1, weights, dtype=torch.float32, normalize=False, ret_per_layer=False, bf16=False, drop_relu_after=None, ceil_mode=False):
    """The definition in `dtype` (fp32 or fp64) on the inputs' device.  Returns (N, 1, 1, 1), with ret_per_layer also the five per-tap tensors."""
    kw = dict(bf16=bf16, drop_relu_after=drop_relu_after, ceil_mode=ceil_mode)
    t0 = trunk(scaling_layer(in0.to(dtype), normalize), weights, dtype, **kw)
    t1 = trunk(scaling_layer(in1.to(dtype), normalize), weights, dtype, **kw)
    res = [head(t0[k], t1[k], weights[f"lin{k}.weight"]) for k in range(5)]
    val = res[0] + res[1] + res[2] + res[3] + res[4]
    return (val, res) if ret_per_layer else val


def lpips_ref_bf16(in0, in1, weights, dtype=torch.float32, normalize=False, ret_per_layer=False, **kw):
    """The same with the stated deviation of tokensgen_amd.lpips built in: separates kernel faults from the deviation."""
    return lpips_ref(in0, in1, weights, dtype, normalize, ret_per_layer, bf16=True, **kw)


def conv_in_ref(x_scaled, weights, padding=1):
    """conv1_1 + ReLU in float64 on a scaled float64 (N, 3, H, W), and sum |w x| over the 27 taps per output element (the fp32 error scale)"""
    w, b = weights["features.0.weight"].double(), weights["features.0.bias"].double()
    return F.relu(F.conv2d(x_scaled, w, b, padding=padding)), F.conv2d(x_scaled.abs(), w.abs(), None, padding=padding)


SIGMAS = (0.02, 0.1, 0.5)
WHOLE_MODEL_SHAPES = ((3, 70, 100), (2, 16, 16), (1, 480, 720))      # pools floor 35 -> 17, 25 -> 12, 17 -> 8; 1 x 1 at the last tap; launch-scale convolution kernels


def make_inputs(shape, seed, sigma):
    """in0: a picture-like batch in [-1, 1] (smooth content plus texture); in1 = in0 + sigma * noise (not clamped).  fp32 (N, 3, H, W) on the CPU."""
    n, h, w = shape
    g = torch.Generator().manual_seed(1000 * seed + h)
    base = F.interpolate(torch.rand(n, 3, max(h // 8, 2), max(w // 8, 2), generator=g), size=(h, w), mode="bilinear", align_corners=False)
    in0 = (0.7 * base + 0.3 * torch.rand(n, 3, h, w, generator=g)) * 2 - 1
    in1 = in0 + sigma * torch.randn(n, 3, h, w, generator=g)
    return in0, in1
