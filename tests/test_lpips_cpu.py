"""tokensgen_amd.lpips without a GPU: the loader (three key layouts and a mix), the restatement of tests/lpips_ref.py against a hand-computed answer and fp32 against
fp64, the argument checks of the new exports (no launch) and of the bindings, and that VideoMetrics without a model is what it was.  The kernels are held to the
restatement in tests/test_lpips_gpu.py."""
import ctypes

import pytest
import torch

import lpips_ref as LR

F64 = torch.float64


def _torchvision(w):
    return {k: v for k, v in w.items() if k.startswith("features.")}


def _lin_file(w):
    return {f"lin{k}.model.1.weight": w[f"lin{k}.weight"] for k in range(5)}


def _full_lpips(w):
    sd = {"scaling_layer.shift": torch.zeros(1, 3, 1, 1), "scaling_layer.scale": torch.ones(1, 3, 1, 1)}
    for idx, _, _, stage in LR.CONVS:
        for leaf in ("weight", "bias"):
            sd[f"net.slice{stage}.{idx}.{leaf}"] = w[f"features.{idx}.{leaf}"]
    for k in range(5):
        sd[f"lin{k}.model.1.weight"] = w[f"lin{k}.weight"]
        sd[f"lins.{k}.model.1.weight"] = w[f"lin{k}.weight"]
    return sd


def test_loader_takes_the_three_key_layouts_and_a_mix():
    from tokensgen_amd.lpips import LPIPS, canonical_state_dict, expected_shapes
    w = LR.random_weights(0)
    layouts = {"torchvision + vgg.pth": {**_torchvision(w), **_lin_file(w)}, "full lpips.LPIPS": _full_lpips(w)}
    mix = {k: v for k, v in _full_lpips(w).items() if ".slice3." not in k and k[:4] not in ("lin0", "lin1", "lin2", "lin3", "lin4")}          # slices 1, 2, 4, 5 and lins.* from the full dict ...
    mix.update({k: v for k, v in _torchvision(w).items() if k.split(".")[1] in ("10", "12", "14")})             # ... stage 3 under torchvision's names
    layouts["mix"] = mix
    packed = None
    for name, sd in layouts.items():
        canon, unexpected = canonical_state_dict(sd)
        assert not unexpected and set(canon) == set(expected_shapes()) == set(w), name
        assert all(torch.equal(canon[k], w[k]) for k in w), name
        m = LPIPS("cpu")
        assert m.load_state_dict(sd) == []
        if packed is not None:
            assert all(torch.equal(m._w[k], packed[k]) for k in packed), name
        packed = m._w
    # packed shapes: conv1_2 is padded to 128 output channels, the rows past 64 are zero; the tap axis is (row, column); conv1_1 and the lin weights stay fp32
    assert packed["2.weight"].shape == (128, 9, 64) and packed["2.bias"].shape == (128,) and packed["28.weight"].shape == (512, 9, 512)
    assert packed["2.weight"].dtype == torch.bfloat16 and not packed["2.weight"][64:].any() and not packed["2.bias"][64:].any()
    assert torch.equal(packed["2.weight"][5, 7, 11], w["features.2.weight"][5, 11, 2, 1].bfloat16())
    assert packed["in.weight"].shape == (64, 27) and packed["in.weight"].dtype == torch.float32 and torch.equal(packed["in.weight"][3, 9 + 3 + 2], w["features.0.weight"][3, 1, 1, 2])
    assert packed["lin4"].shape == (512,) and packed["lin4"].dtype == torch.float32
    # torchvision's file also carries the classifier: ignored, not an error
    assert LPIPS("cpu").load_state_dict({**layouts["mix"], "classifier.0.weight": torch.zeros(2, 2)}) == []


def test_loader_refuses_missing_misshapen_and_unexpected_keys():
    from tokensgen_amd.lpips import LPIPS
    w = LR.random_weights(1)
    good = {**_torchvision(w), **_lin_file(w)}
    with pytest.raises(RuntimeError, match=r"missing \['features.7.bias', 'lin2.weight'\]"):
        LPIPS("cpu").load_state_dict({k: v for k, v in good.items() if k not in ("features.7.bias", "lin2.model.1.weight")})
    with pytest.raises(RuntimeError, match=r"missing \['features.0.weight'"):
        LPIPS("cpu").load_state_dict(_lin_file(w))                                     # vgg.pth alone: the trunk is missing
    with pytest.raises(RuntimeError, match=r"shape mismatch \['features.2.weight'\]"):
        LPIPS("cpu").load_state_dict({**good, "features.2.weight": torch.zeros(64, 64, 1, 1)})
    with pytest.raises(RuntimeError, match=r"shape mismatch \['lin0.weight'\]"):
        LPIPS("cpu").load_state_dict({**good, "lin0.model.1.weight": torch.zeros(64)})
    with pytest.raises(RuntimeError, match=r"unexpected \['features.1.weight', 'lin5.model.1.weight'\]"):
        LPIPS("cpu").load_state_dict({**good, "features.1.weight": torch.zeros(1), "lin5.model.1.weight": torch.zeros(1)})
    assert LPIPS("cpu").load_state_dict({**good, "features.1.weight": torch.zeros(1)}, strict=False) == ["features.1.weight"]
    with pytest.raises(RuntimeError, match="no weights loaded"):
        LPIPS("cpu").per_frame(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 16), "chw")


def _copy_weights():
    """every convolution copies channel 0 (centre tap 1, all else 0, no bias): a tap's feature is relu / pooled relu of the scaled red channel in channel 0, zero elsewhere"""
    w = {}
    for idx, ci, co, _ in LR.CONVS:
        w[f"features.{idx}.weight"] = torch.zeros(co, ci, 3, 3, dtype=F64)
        w[f"features.{idx}.weight"][0, 0, 1, 1] = 1.0
        w[f"features.{idx}.bias"] = torch.zeros(co, dtype=F64)
    for k, c in enumerate(LR.TAP_CHANNELS):
        w[f"lin{k}.weight"] = torch.zeros(1, c, 1, 1, dtype=F64)
        w[f"lin{k}.weight"][0, 0, 0, 0] = (0.3, 0.5, 0.7, 1.1, 1.3)[k]
    return w


def test_restatement_against_a_hand_computed_answer():
    """in0: red = 0.5 everywhere (scaled: positive); in1: red = -0.5 on the left half (scaled: negative, ReLU: 0), 0.25 on the right half.  A unit-normalised
    one-channel feature is 1 where it is positive and 0 where it is 0, so per tap d = 1 on the pixels where only one image is positive: the left half at 16 x 16, 8 x 8,
    4 x 4 and 2 x 2 (the pools keep the halves apart), nothing at 1 x 1 (the last pool sees the right half).  Result: 0.5 (0.3 + 0.5 + 0.7 + 1.1) + 0 = 1.3."""
    w = _copy_weights()
    in0 = torch.full((1, 3, 16, 16), 0.5, dtype=F64)
    in1 = torch.full((1, 3, 16, 16), 0.25, dtype=F64)
    in1[:, :, :, :8] = -0.5
    val, taps = LR.lpips_ref(in0, in1, w, F64, ret_per_layer=True)
    assert val.shape == (1, 1, 1, 1) and [tuple(t.shape) for t in taps] == [(1, 1, 1, 1)] * 5
    want = [0.15, 0.25, 0.35, 0.55, 0.0]
    assert all(abs(taps[k].item() - want[k]) < 1e-9 for k in range(5)), [t.item() for t in taps]
    assert abs(val.item() - 1.3) < 1e-9
    # normalize: the same pictures given in [0, 1]
    assert abs(LR.lpips_ref((in0 + 1) / 2, (in1 + 1) / 2, w, F64, normalize=True).item() - 1.3) < 1e-9
    # in0 == in1 gives 0, with random weights too
    assert LR.lpips_ref(in1, in1.clone(), w, F64).item() == 0.0
    a, _ = LR.make_inputs((2, 16, 16), 0, 0.1)
    assert LR.lpips_ref(a, a.clone(), LR.random_weights(0)).abs().max().item() == 0.0
    # the bf16 restatement of the same case: every value in play is a bf16 number
    assert abs(LR.lpips_ref_bf16(in0, in1, w, F64).item() - LR.lpips_ref_bf16(in0, in1, w, torch.float32).item()) < 1e-6


@pytest.mark.parametrize("shape", LR.WHOLE_MODEL_SHAPES[:2], ids=["3x70x100", "2x16x16"])
def test_fp32_restatement_agrees_with_fp64(shape):
    """The fp32 yardstick of the GPU tests against float64 on the GPU tests' inputs, every seed and sigma of two of the three shapes: the value within 1e-5
    relative.  The third shape, 480 x 720, is held to the same bound on the device: tests/test_lpips_gpu.py::test_fp32_restatement_agrees_with_fp64_at_480x720.  The per-tap gaps are printed, not asserted: a single tap of a single 1 x 1 map (16 x 16 inputs, sigma 0.02) carries the cancellation of f0 - f1 without
    any averaging and comes to 1e-5 by itself."""
    worst, worst_tap = 0.0, 0.0
    for seed in range(3):
        w = LR.random_weights(seed)
        for sigma in LR.SIGMAS:
            in0, in1 = LR.make_inputs(shape, seed, sigma)
            v32, t32 = LR.lpips_ref(in0, in1, w, torch.float32, ret_per_layer=True)
            v64, t64 = LR.lpips_ref(in0, in1, w, F64, ret_per_layer=True)
            assert bool((v64 > 0).all()) and v32.dtype == torch.float32 and v64.dtype == F64
            worst = max(worst, ((v32.double() - v64).abs() / v64).max().item())
            worst_tap = max(worst_tap, max(((a.double() - b).abs() / b).max().item() for a, b in zip(t32, t64)))
    print("fp32 against fp64, worst relative gap of the value", worst, "of a single tap", worst_tap)
    assert worst < 1e-5


def _aligned(nbytes=1 << 12):
    buf = ctypes.create_string_buffer(nbytes + 16)
    return buf, ctypes.addressof(buf) + (16 - ctypes.addressof(buf) % 16)


def test_new_exports_validate_their_arguments_without_a_launch():
    from tokensgen_amd import lib as L
    lib = L.load()
    _keep, p = _aligned()
    err = lambda: lib.tg_last_error_string().decode()
    # tg_lpips_conv_in, in the order of the prototype
    args = dict(x=p, so=0, si=768, sc=256, sr=16, sp=1, dtype=1, normalize=0, n_outer=1, n_inner=1, h=16, w=16, weight=p, bias=p, y=p, stream=None)
    ci = lambda **kw: lib.tg_lpips_conv_in(*{**args, **kw}.values())
    for name in ("x", "weight", "bias", "y"):
        assert ci(**{name: None}) == -1 and "null pointer" in err(), name
    assert ci(dtype=3) == -1 and ci(dtype=-1) == -1 and ci(normalize=2) == -1 and ci(dtype=0, normalize=1) == -1 and "0 with uint8" in err()
    for name in ("n_outer", "n_inner", "h", "w"):
        assert ci(**{name: 0}) == -2 and "bad shape" in err(), name
    for name in ("so", "si", "sc", "sr", "sp"):
        assert ci(**{name: -1}) == -2 and "negative stride" in err(), name
    assert ci(x=p + 2) == -3 and ci(dtype=2, x=p + 1) == -3 and ci(weight=p + 2) == -3 and ci(bias=p + 1) == -3 and ci(y=p + 8) == -3
    assert ci(dtype=0, x=p + 1, y=None) == -1                                         # uint8 needs no alignment: the next fault is reported
    assert ci(n_outer=1 << 15, n_inner=1 << 15, h=32, w=32) == -2 and "too many tiles" in err()
    # tg_relu_cl
    assert lib.tg_relu_cl(None, 64, None) == -1 and "null pointer" in err()
    for n in (0, -8, 12, 7):
        assert lib.tg_relu_cl(p, n, None) == -2 and "multiple of 8" in err(), n
    assert lib.tg_relu_cl(p + 2, 64, None) == -3
    # tg_relu_maxpool2_cl
    mp = lambda x=p, F=1, H=4, W=4, C=64, y=p: lib.tg_relu_maxpool2_cl(x, F, H, W, C, y, None)
    assert mp(x=None) == -1 and mp(y=None) == -1 and "null pointer" in err()
    assert mp(F=0) == -2 and mp(H=1) == -2 and mp(W=1) == -2 and mp(C=0) == -2 and mp(C=60) == -2 and "multiple of 8" in err()
    assert mp(x=p + 8) == -3 and mp(y=p + 2) == -3
    # tg_lpips_head
    hd = dict(fa=p, fb=p, w=p, F=1, H=4, W=4, C=64, relu_on_load=0, ws=p, out=p, stream=None)
    head = lambda **kw: lib.tg_lpips_head(*{**hd, **kw}.values())
    for name in ("fa", "fb", "w", "ws", "out"):
        assert head(**{name: None}) == -1 and "null pointer" in err(), name
    assert head(relu_on_load=2) == -1
    for kw in (dict(F=0), dict(H=0), dict(W=0), dict(C=0), dict(C=8), dict(C=96), dict(C=1024)):
        assert head(**kw) == -2 and "C in {64, 128, 256, 512}" in err(), kw
    assert head(fa=p + 8) == -3 and head(fb=p + 2) == -3 and head(w=p + 2) == -3 and head(ws=p + 4) == -3 and head(out=p + 4) == -3
    # the workspace: one double per tile of 512 pixels of a frame
    q = lib.tg_lpips_head_ws_doubles
    assert q(1, 1, 1) == 1 and q(3, 16, 32) == 3 and q(3, 16, 33) == 6 and q(2, 480, 720) == 2 * 675 and q(0, 4, 4) == 0 and q(1, 0, 4) == 0 and q(1, 4, 0) == 0


def test_bindings_refuse_bad_arguments_and_cpu_tensors():
    from tokensgen_amd import kernels as K
    from tokensgen_amd import metrics as M
    from tokensgen_amd.lpips import LPIPS, video_lpips
    z = torch.zeros
    w27, b64 = z(64, 27), z(64)
    out = lambda n, h, w: z(n, h, w, 64, dtype=torch.bfloat16)
    for shape in ((1, 3, 15, 40), (1, 3, 40, 15)):
        with pytest.raises(ValueError, match="smaller than 16 x 16"):
            K.lpips_conv_in(z(*shape), "chw", w27, b64, out(1, *shape[2:]))
    with pytest.raises(ValueError, match="smaller than 16 x 16"):
        K.lpips_conv_in(z(1, 3, 20, 40), "chw", w27, b64, out(1, 14, 34), crop_border=3)
    with pytest.raises(ValueError, match="out: expected contiguous"):
        K.lpips_conv_in(z(2, 3, 16, 16), "chw", w27, b64, out(2, 16, 32)[:, :, ::2])          # a strided output
    with pytest.raises(ValueError, match="out: expected contiguous"):
        K.lpips_conv_in(z(2, 3, 16, 16), "chw", w27, b64, out(1, 16, 16))
    with pytest.raises(ValueError, match="weight / bias"):
        K.lpips_conv_in(z(2, 3, 16, 16), "chw", z(27, 64).t(), b64, out(2, 16, 16))           # [64, 27], but transposed in memory
    with pytest.raises(ValueError, match="3 channels"):
        K.lpips_conv_in(z(1, 1, 16, 16), "chw", w27, b64, out(1, 16, 16))
    with pytest.raises(TypeError):
        K.lpips_conv_in(z(1, 3, 16, 16, dtype=torch.float16), "chw", w27, b64, out(1, 16, 16))
    with pytest.raises(ValueError, match="normalize"):
        K.lpips_conv_in(z(1, 16, 16, 3, dtype=torch.uint8), "hwc", w27, b64, out(1, 16, 16), normalize=True)
    with pytest.raises(ValueError, match="inner range"):
        K.lpips_conv_in(z(2, 3, 16, 16), "chw", w27, b64, out(2, 16, 16), inner=(1, 2))
    with pytest.raises(RuntimeError, match="GPU"):
        K.lpips_conv_in(z(1, 3, 16, 16), "chw", w27, b64, out(1, 16, 16))
    for fn, arg in ((K.relu_cl_, out(1, 2, 2)), (K.relu_maxpool2_cl, out(1, 2, 2))):
        with pytest.raises(RuntimeError, match="GPU"):
            fn(arg)
    with pytest.raises(RuntimeError, match="GPU"):
        K.lpips_head(out(1, 2, 2), out(1, 2, 2), z(64))
    m = LPIPS("cpu")
    m.load_state_dict(LR.as_state_dict(LR.random_weights(0)))
    with pytest.raises(RuntimeError, match="GPU"):
        m(z(1, 3, 16, 16), z(1, 3, 16, 16))
    with pytest.raises(RuntimeError, match="GPU"):
        video_lpips(z(2, 16, 16, 3, dtype=torch.uint8), z(2, 16, 16, 3, dtype=torch.uint8), m)
    # calculate_lpips: the reference's signature, its unsupported arguments refused
    with pytest.raises(ValueError, match="model"):
        M.calculate_lpips(z(1, 3, 16, 16), z(1, 3, 16, 16), 0)
    with pytest.raises(ValueError, match="test_y_channel"):
        M.calculate_lpips(z(1, 3, 16, 16), z(1, 3, 16, 16), 0, test_y_channel=True, model=m)
    with pytest.raises(ValueError, match="input_order"):
        M.calculate_lpips(z(1, 16, 16, 3), z(1, 16, 16, 3), 0, input_order='HWC', model=m)
    with pytest.raises(AssertionError, match="Image shapes are different"):
        M.calculate_lpips(z(1, 3, 16, 16), z(1, 3, 16, 17), 0, model=m)
    with pytest.raises(RuntimeError, match="GPU"):
        M.calculate_lpips(z(1, 3, 16, 16), z(1, 3, 16, 16), 0, model=m)
    # the chunk rule: frames_per_launch, cut to tg_conv3d_cl's 32-bit-offset guard (T + 2) h w 64 < 2^31
    assert m.frames_per_launch == 8 and m.max_frames(480, 720) == 95 and (95 + 2) * 480 * 720 * 64 < 2 ** 31 <= (96 + 2) * 480 * 720 * 64
    assert m.max_frames(2160, 3840) == 2 and m.max_frames(4320, 7680) < 2


def test_video_metrics_without_a_model_is_unchanged():
    import inspect
    from tokensgen_amd import metrics as M
    sig = inspect.signature(M.VideoMetrics.__init__)
    assert list(sig.parameters) == ["self", "crop_border", "test_y_channel", "lpips_model"] and sig.parameters["lpips_model"].default is None
    vm = M.VideoMetrics()
    assert vm.lpips_model is None
    # finalize without a model: today's keys, from stored per-frame values (no device needed for the pooling arithmetic)
    vm._mse, vm._ssim = [torch.tensor([0.01, 0.02], dtype=F64)], [torch.tensor([0.9, 0.8], dtype=F64)]
    fin = vm.finalize()
    assert set(fin) == {"frames", "mse", "psnr", "ssim", "psnr_pooled", "ssim_pooled"} and fin["frames"] == 2
    assert abs(fin["ssim_pooled"].item() - 0.85) < 1e-15 and abs(fin["psnr_pooled"].item() - 10 * torch.log10(torch.tensor(1 / (0.015 + 1e-8), dtype=F64)).item()) < 1e-12
    assert list(inspect.signature(M.calculate_lpips).parameters)[:6] == ["img", "img2", "crop_border", "input_order", "test_y_channel", "model"]
