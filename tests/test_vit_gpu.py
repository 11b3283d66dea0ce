"""GPU: the ViT encoder kernels (csrc/vit.hip), the encoders built from them (tokensgen_amd/vit.py) and the frame-consistency metric (tokensgen_amd/metrics.py).

The tolerance method is tests/test_t5_gpu.py's.  Per kernel: inputs are bf16 values; the reference is tests/vit_ref.py in exact float64; the bound is 2 x the error
that vit_ref's kernel-rounding mode (bf16 wherever the kernel stores bf16) has against that reference on the same inputs.  Where that emulation is exact — a kernel
with one rounding per element whose fp32 arithmetic before it is exact: tg_vit_patch_rows, tg_vit_assemble — the kernel must be exact too (the bound is then 1e-12,
for the strict `<`).  Whole model: the error against the library's float64 features stored in tests/golden/vit_tiny*.pt must be at most 1.5 x the error of the
library's own bf16 run stored beside them; tests/test_vit_cpu.py shows that the kernels' rounding points emulated on the CPU land at 0.7 .. 1.0 x of it and that
every semantic mutation lands >= 3 x beyond the bound."""
import os

import pytest
import torch

import vit_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
F64 = torch.float64
FILES = {"vit": "vit_tiny.pt", "clip": "vit_tiny_clip.pt"}
KINDS = ["vit", "clip"]


@pytest.fixture(scope="module")
def gold(golden_dir):
    return {k: torch.load(os.path.join(golden_dir, f), weights_only=False) for k, f in FILES.items()}


@pytest.fixture(scope="module")
def tiny(gold):
    from tokensgen_amd.vit import ViTEncoder
    out = {}
    for kind in KINDS:
        m = ViTEncoder(gold[kind]["config"], device=DEV, kind=kind)
        m.load_state_dict(gold[kind]["state_dict"], strict=True)
        out[kind] = m
    return out


@pytest.fixture(scope="module")
def tiny_features(gold, tiny):
    """encode_frames of the fixture's 6 bf16 frames, one call per kind: computed once, shared, left unchanged"""
    return {kind: tiny[kind].encode_frames(gold[kind]["frames"].to(DEV)) for kind in KINDS}


def _bound(emulated, exact):
    return 2.0 * R.rel_l2(emulated, exact) + 1e-12


def _randn(shape, seed, scale=1.0):
    return (scale * torch.randn(shape, generator=torch.Generator().manual_seed(seed))).to(BF)


def _launch_counts(forward):
    """{kernel name: launches} of one call of `forward`, after a warm-up call.  kernels.PROFILE keeps tg_gemm_bf16 under names that carry the shape
    (`gemm_M.._N.._K.._epi..`): they are counted together as "gemm"."""
    from tokensgen_amd import kernels as K
    forward()
    K.PROFILE.clear()
    was = K.PROFILE_ON[0]
    try:
        K.PROFILE_ON[0] = True
        forward()
        counts = {}
        for name, events in K.PROFILE.items():
            name = "gemm" if name.startswith("gemm_M") else name
            counts[name] = counts.get(name, 0) + len(events)
    finally:
        K.PROFILE_ON[0] = was
        K.PROFILE.clear()
    return counts


# ---------------------------------------------------------------------------------------------------- kernels
@pytest.mark.timeout(120)
@pytest.mark.parametrize("H,W,p", [(40, 40, 8), (30, 30, 6), (16, 48, 8)])
def test_patch_rows_exact(H, W, p, parity):
    """one rounding per element: bitwise against the restatement's rounding mode (column order (c, dy, dx), the folded constants as fp32, pad columns zero)"""
    from tokensgen_amd import kernels as K
    from tokensgen_amd.vit import fold_preprocessing
    F = 3
    x = (2 * torch.rand(F, 3, H, W, generator=torch.Generator().manual_seed(H + p)) - 1).to(BF)
    x[0, 0, 0, :4] = torch.tensor([1.0, -1.0, 0.0, -0.0]).to(BF)
    mean, std = R.MEAN_STD["clip"]
    Kp = (3 * p * p + 63) // 64 * 64
    want = R.patch_rows(R.preprocess(x, mean, std, rounding=True), p, pad_to=Kp)
    rows = F * (H // p) * (W // p)
    out = torch.full((rows + 1, Kp), 7.0, dtype=BF, device=DEV)
    a, b = fold_preprocessing(mean, std)
    K.vit_patch_rows(x.to(DEV), p, a, b, out)
    assert Kp == {8: 192, 6: 128}[p] and want.shape == (rows, Kp)
    parity((out[:rows].double().cpu() - want).abs().max(), 1e-12, f"tg_vit_patch_rows {H} x {W} p {p}: max |kernel - restatement with the kernel's rounding|")
    assert (out[:rows, 3 * p * p:] == 0).all() and (out[rows] == 7.0).all()                  # pad columns zero; nothing written past the last row
    exact = R.patch_rows(R.preprocess(x, mean, std), p, pad_to=Kp)
    parity(R.rel_l2(out[:rows], exact), _bound(want, exact), f"tg_vit_patch_rows {H} x {W} p {p}: against the exact preprocessing")


@pytest.mark.timeout(120)
@pytest.mark.parametrize("S", [26, 17])
def test_assemble_exact(S, parity):
    from tokensgen_amd import kernels as K
    F, D, P = 3, 128, S - 1
    patch, cls, pos = _randn((F * P, D), S), _randn((D,), S + 1), _randn((S, D), S + 2, 0.7)
    want = R.assemble(patch.double(), cls.double(), pos.double(), F, rounding=True)
    tok = torch.empty(F, S, D, dtype=BF, device=DEV)
    K.vit_assemble(patch.to(DEV), cls.to(DEV), pos.to(DEV), tok)
    parity((tok.double().cpu() - want).abs().max(), 1e-12, f"tg_vit_assemble S {S}: max |kernel - restatement with the kernel's rounding|")
    assert torch.equal(tok[1, 0], tok[0, 0]) and torch.equal(tok[0, 0].cpu(), (cls.float() + pos[0].float()).to(BF))


@pytest.mark.timeout(120)
@pytest.mark.parametrize("rows,D", [(1, 128), (453, 128), (1, 768), (453, 768)])
def test_layernorm_vs_float64(rows, D, parity):
    from tokensgen_amd import kernels as K
    g = torch.Generator().manual_seed(rows + D)
    x = (1.5 + 3.0 * torch.randn(rows, D, generator=g)).to(BF)
    w, b = (1.0 + 0.25 * torch.randn(D, generator=g)).to(BF), (0.2 * torch.randn(D, generator=g)).to(BF)
    if rows > 1:
        x[7] = 1.5                                    # a constant row whose fp32 sum is exact (D * 1.5): mean = 1.5, variance 0, the result is the bias
        x[8] *= 1e-3                                  # a row scaled by 1e-3
    for eps in (1e-12, 1e-5):
        exact = R.layernorm(x.to(F64), w.to(F64), b.to(F64), eps)
        out = torch.empty(rows, D, dtype=BF, device=DEV)
        K.layernorm(x.to(DEV), w.to(DEV), b.to(DEV), out, eps)
        assert torch.isfinite(out).all()
        parity(R.rel_l2(out, exact), _bound(R.layernorm(x.to(F64), w.to(F64), b.to(F64), eps, rounding=True), exact), f"tg_layernorm rows {rows} D {D} eps {eps}")
        if rows > 1:
            assert torch.equal(out[7].cpu(), b)
            parity(R.rel_l2(out[8], exact[8]), _bound(R.layernorm(x[8].to(F64), w.to(F64), b.to(F64), eps, rounding=True), exact[8]),
                   f"tg_layernorm D {D} eps {eps}: the row scaled by 1e-3")
    if rows > 1:
        # every 26th row through a strided view (ldx = 26 D, as the final norm reads the class tokens): the bits of the contiguous call on those rows
        picked = x[::26].contiguous()
        dense = torch.empty(picked.shape, dtype=BF, device=DEV)
        K.layernorm(picked.to(DEV), w.to(DEV), b.to(DEV), dense, 1e-5)
        xd = x.to(DEV)
        view = xd.view(-1)[:(rows // 26) * 26 * D].view(rows // 26, 26 * D)[:, :D]
        assert view.stride(0) == 26 * D and torch.equal(view.cpu(), picked[:rows // 26])
        strided = torch.empty(rows // 26, D, dtype=BF, device=DEV)
        K.layernorm(view, w.to(DEV), b.to(DEV), strided, 1e-5)
        assert torch.equal(strided, dense[:rows // 26])


@pytest.mark.timeout(120)
@pytest.mark.parametrize("n", [8, 8 * 4099])
@pytest.mark.parametrize("mode", ["gelu", "quick_gelu"])
def test_act_vs_float64(mode, n, parity):
    from tokensgen_amd import kernels as K
    if n == 8:
        x = torch.tensor([-12.0, -3.0, -0.5, 0.0, 0.5, 3.0, 7.0, 12.0]).to(BF)
    else:
        x = torch.linspace(-12, 12, n).to(BF)                                                # 4 099 threads: 16 full workgroups and a tail of 3
        x[:4] = torch.tensor([0.0, -0.0, 1e-3, -1e-3]).to(BF)
    exact = R.act(x.to(F64), mode)
    out = torch.empty(n, dtype=BF, device=DEV)
    K.vit_act(x.to(DEV), out, mode)
    assert torch.isfinite(out).all()
    parity(R.rel_l2(out, exact), _bound(R.act(x.to(F64), mode, rounding=True), exact), f"tg_vit_act {mode} n {n}")
    # the negative tail on its own, where the values are tiny and a 1 + erf form would cancel
    tail = x.double() < -3.0
    parity(R.rel_l2(out.cpu()[tail], exact[tail]), _bound(R.act(x.to(F64), mode, rounding=True)[tail], exact[tail]), f"tg_vit_act {mode} n {n}: x < -3")
    inplace = x.to(DEV)
    K.vit_act(inplace, inplace, mode)
    assert torch.equal(inplace, out)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("S", [17, 26, 197])
def test_attention_as_the_encoder_calls_it(S, parity):
    """q already multiplied by 1/8 (as the loader leaves q_proj) and a zero bias table, against float64 softmax attention with the 1/8 scale"""
    from tokensgen_amd import kernels as K
    B, H = 3, 2
    qkv = _randn((B, S, 3 * H * 64), S)
    qkv[..., :2 * H * 64] *= 1.6                      # scores of a few units after the scale
    q, k, v = (t.to(F64).view(B, S, H, 64) for t in qkv.split(H * 64, dim=-1))
    exact, emulated = R.attention(q, k, v, 0.125), R.attention(q, k, v, 0.125, rounding=True)
    scaled = qkv.clone()
    scaled[..., :H * 64] = (qkv[..., :H * 64].float() * 0.125).to(BF)
    assert torch.equal(scaled[..., :H * 64].double() * 8, qkv[..., :H * 64].double())       # exact in bf16
    out = torch.empty(B, S, H * 64, dtype=BF, device=DEV)
    K.t5_attention(scaled.to(DEV), torch.zeros(H, 2 * S - 1, device=DEV), out, H)
    assert torch.isfinite(out).all()
    parity(R.rel_l2(out, exact), _bound(emulated, exact), f"tg_t5_attention as the ViT calls it, S {S}")


@pytest.mark.timeout(120)
@pytest.mark.parametrize("D", [128, 512, 768])
@pytest.mark.parametrize("F", [2, 3, 50])
def test_feature_consistency_vs_float64(F, D, parity):
    from tokensgen_amd import kernels as K
    g = torch.Generator().manual_seed(F * D)
    base = torch.randn(D, generator=g)
    f = base[None] + 0.6 * torch.randn(F, D, generator=g)                                    # correlated frames: cosines around 0.7
    want_p, want_f, _ = R.consistency(f)
    prev, first = K.feature_consistency(f.to(DEV))
    assert prev.dtype == F64 and prev.shape == first.shape == (F - 1,)
    parity(((prev.cpu() - want_p).abs() / want_p.clamp_min(1e-300)).max(), 1e-12, f"tg_feature_consistency F {F} D {D}: prev, relative")
    parity(((first.cpu() - want_f).abs() / want_f.clamp_min(1e-300)).max(), 1e-12, f"tg_feature_consistency F {F} D {D}: first, relative")
    p2, f2 = K.feature_consistency(f.to(DEV))
    assert torch.equal(p2, prev) and torch.equal(f2, first)                                  # two launches: the same bits
    wide = torch.full((F, D + 40), float("nan"), device=DEV)                                 # a row stride that is not D
    wide[:, :D] = f
    p3, f3 = K.feature_consistency(wide[:, :D])
    assert torch.equal(p3, prev) and torch.equal(f3, first)


@pytest.mark.timeout(120)
def test_feature_consistency_special_rows_and_carried_rows(parity):
    from tokensgen_amd import kernels as K
    f = R.special_features(128, seed=3)
    want_p, want_f, _ = R.consistency(f)
    prev, first = K.feature_consistency(f.to(DEV))
    parity((prev.cpu() - want_p).abs().max(), 1e-12, "tg_feature_consistency special rows: prev")
    parity((first.cpu() - want_f).abs().max(), 1e-12, "tg_feature_consistency special rows: first")
    assert prev[1] == 0 and abs(prev[3].item() - 1.0) < 1e-12 and prev[4] == 0 and prev[5] == 0 and first[4] == 0 and torch.isfinite(prev).all()
    fd = f.to(DEV)
    p2, f2 = K.feature_consistency(fd[3:], fd[0].clone(), fd[2].clone())                      # the video's second part with its carried rows
    assert p2.shape == (4,) and torch.equal(p2, prev[2:]) and torch.equal(f2, first[2:])
    p1, f1 = K.feature_consistency(fd[6:], fd[0].clone(), fd[5].clone())                      # a part of one frame
    assert torch.equal(p1, prev[5:]) and torch.equal(f1, first[5:])


# ---------------------------------------------------------------------------------------------------- the models
@pytest.mark.timeout(120)
@pytest.mark.parametrize("kind", KINDS)
def test_tiny_model_vs_library_float64(kind, gold, tiny_features, parity):
    g, out = gold[kind], tiny_features[kind]
    assert out.dtype == torch.float32 and out.shape == (6, 128) and torch.isfinite(out).all()
    library = R.rel_l2(g["bf16"], g["f64"])
    parity(R.rel_l2(out, g["f64"]), 1.5 * library, f"{kind} tiny: error against float64, bound 1.5 x the library's bf16 run ({library:.3e})")


@pytest.mark.timeout(120)
@pytest.mark.parametrize("kind", KINDS)
def test_a_frame_s_feature_does_not_depend_on_the_call(kind, gold, tiny, tiny_features):
    frames = gold[kind]["frames"].to(DEV)
    m = tiny[kind]
    assert torch.equal(torch.cat([m.encode_frames(frames[:4]), m.encode_frames(frames[4:])]), tiny_features[kind])          # 4 + 2 against 6 in one call
    assert torch.equal(m.encode_frames(frames), tiny_features[kind])                                                        # a second call: the same bits
    m.frames_per_launch = 4                                                                                                 # ... and the trunk cut into batches of 4 + 2
    try:
        assert torch.equal(m.encode_frames(frames), tiny_features[kind])
    finally:
        m.frames_per_launch = 64


@pytest.mark.timeout(120)
@pytest.mark.parametrize("kind", KINDS)
def test_launches_per_forward(kind, gold, tiny):
    """2 bf16 frames through a model of L layers: the patch rows, the patch GEMM, the assembly, ten launches per block, the class-token LayerNorm; CLIP adds
    pre_layrnorm and the projection.  No other kernel."""
    m, frames = tiny[kind], gold[kind]["frames"][:2].to(DEV)
    L, clip = m.config.num_hidden_layers, int(kind == "clip")
    assert _launch_counts(lambda: m.encode_frames(frames)) == {"vit_patch_rows": 1, "vit_assemble": 1, "gemm": 4 * L + 1 + clip, "layernorm": 2 * L + 1 + clip,
                                                               "t5_attention": L, "residual_add": 2 * L, "vit_act": L}


@pytest.mark.timeout(120)
@pytest.mark.parametrize("kind", KINDS)
def test_tiny_model_consistency_vs_float64_features(kind, gold, tiny, tiny_features, parity):
    """prev / first against float64 values from the library's float64 features: |delta| <= 4 eps / (1 - eps), eps the per-frame feature bound of the test above
    (1.5 x the library's bf16 error, taken per frame).  A relative feature error eps moves a unit vector by at most 2 eps (its direction by eps / (1 - eps) at most
    on either side), so it moves the cosine of two such vectors by at most 4 eps / (1 - eps).  Derived, not measured."""
    from tokensgen_amd.metrics import video_consistency
    g = gold[kind]
    res = video_consistency(g["frames"].to(DEV), tiny[kind])
    want_p, want_f, want_s = R.consistency(g["f64"])
    assert res["prev"].dtype == F64 and res["prev"].shape == (5,) and res["score"].dim() == 0 and res["prev"].is_cuda
    per_frame = max(R.rel_l2(g["bf16"][i], g["f64"][i]) for i in range(6))
    eps = 1.5 * per_frame
    worst = max(R.rel_l2(tiny_features[kind][i], g["f64"][i]) for i in range(6))
    parity(worst, eps, f"{kind} tiny: the worst frame's feature error, bound 1.5 x the library's worst frame ({per_frame:.3e})")
    bound = 4 * eps / (1 - eps)
    parity((res["prev"].cpu() - want_p).abs().max(), bound, f"{kind} tiny: prev against float64 features")
    parity((res["first"].cpu() - want_f).abs().max(), bound, f"{kind} tiny: first against float64 features")
    parity(abs(res["score"].item() - want_s.item()), bound, f"{kind} tiny: score against float64 features")
    own_p, own_f, own_s = R.consistency(tiny_features[kind].cpu())                                # on the encoder's own features the kernel is a float64 formula
    assert (res["prev"].cpu() - own_p).abs().max() < 1e-12 and (res["first"].cpu() - own_f).abs().max() < 1e-12 and abs(res["score"].item() - own_s.item()) < 1e-12


@pytest.mark.timeout(120)
@pytest.mark.parametrize("kind", KINDS)
def test_uint8_frames_take_the_prepare_video_route(kind, tiny):
    """6 uint8 frames of 80 x 120 through encode_frames: the bits of prepare_video(..., (s, s), crop_to_fit=True) followed by the bf16 entry; [B, T, H, W, 3] too"""
    from tokensgen_amd.video_io import prepare_video
    m = tiny[kind]
    s = m.config.image_size
    u8 = torch.randint(0, 256, (6, 80, 120, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(9))
    yy = torch.linspace(0, 1, 80)[:, None, None]
    u8 = (u8.float() * 0.3 + 160 * yy).clamp(0, 255).to(torch.uint8)                          # structure that survives the resize
    direct = m.encode_frames(u8.to(DEV))
    prepared = prepare_video(u8, output_res=(s, s), crop_to_fit=True, device=DEV)[0]
    assert prepared.shape == (6, 3, s, s) and prepared.dtype == BF
    assert torch.equal(direct, m.encode_frames(prepared))
    assert torch.equal(m.encode_frames(u8.to(DEV).view(2, 3, 80, 120, 3)), direct)
    assert torch.equal(m.encode_frames(u8), direct)                                           # host frames are moved


@pytest.mark.timeout(120)
def test_streaming_consistency_gives_the_bits_of_one_call(gold, tiny):
    from tokensgen_amd.metrics import VideoConsistency, video_consistency
    u8 = torch.randint(0, 256, (16, 48, 64, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(10)).to(DEV)
    a, b = u8[:10], u8[10:]
    whole = {k: video_consistency(a, tiny[k]) for k in KINDS}
    second = {k: video_consistency(b, tiny[k]) for k in KINDS}
    vc = VideoConsistency(subject_model=tiny["vit"], background_model=tiny["clip"])
    for lo, hi in ((0, 4), (4, 5), (5, 10)):
        vc.update(a[lo:hi])
    vc.new_video()
    vc.update(b[:1])                                  # a first piece of one frame: nothing to compare yet
    vc.update(b[1:])
    res = vc.finalize()
    assert res["videos"] == 2
    for name, k in (("subject", "vit"), ("background", "clip")):
        assert torch.equal(res[f"{name}_first"][0], whole[k]["first"]) and torch.equal(res[f"{name}_prev"][0], whole[k]["prev"])
        assert torch.equal(res[f"{name}_first"][1], second[k]["first"]) and torch.equal(res[f"{name}_prev"][1], second[k]["prev"])
        assert torch.equal(res[f"{name}_scores"], torch.stack([whole[k]["score"], second[k]["score"]]))
        assert torch.equal(res[f"{name}_consistency"], res[f"{name}_scores"].mean()) and res[f"{name}_scores"].dtype == F64
        assert not torch.equal(whole[k]["first"][:5], second[k]["first"][:5])                 # new_video() separated the two
    only = VideoConsistency(background_model=tiny["clip"])
    only.update(a)
    out = only.finalize()
    assert "subject_consistency" not in out and torch.equal(out["background_scores"][0], whole["clip"]["score"])
    with pytest.raises(ValueError, match="at least 2"):
        one = VideoConsistency(subject_model=tiny["vit"])
        one.update(a[:1])
        one.new_video()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("kind", KINDS)
def test_one_real_width_layer_vs_fp32(kind, parity):
    """hidden 768, 12 heads, MLP 3072, one layer, F = 4 ("vit": image 224, patch 16, S = 197; "clip": patch 32, S = 50, projection 512), random weights:
    against vit_ref in fp32 on the GPU (checker only); the bound is 1.5 x the error of the bf16 torch route computed here."""
    from tokensgen_amd.vit import ViTEncoder
    cfg = dict(hidden_size=768, num_attention_heads=12, num_hidden_layers=1, intermediate_size=3072, image_size=224, patch_size=16 if kind == "vit" else 32,
               hidden_act="gelu" if kind == "vit" else "quick_gelu", layer_norm_eps=1e-12 if kind == "vit" else 1e-5, projection_dim=512)
    m = ViTEncoder(cfg, device=DEV, kind=kind)
    assert m.tokens == (197 if kind == "vit" else 50)
    g = torch.Generator(device=DEV).manual_seed(21)
    sd = {}
    for k, v in m.state_dict().items():
        r = torch.randn(v.shape, generator=g, device=DEV)
        if "norm" in k and k.endswith("weight"):
            r = 1.0 + 0.25 * r
        elif "norm" in k or k.endswith("bias"):
            r = 0.1 * r
        elif "cls_token" in k or "class_embedding" in k or "position_embedding" in k:
            r = 0.7 * r
        elif "patch_embedding" in k:
            r = r * (3 * cfg["patch_size"] ** 2) ** -0.5
        elif "q_proj" in k or "k_proj" in k:
            r = r * 768 ** -0.5 * 1.3
        else:
            r = r * v.shape[-1] ** -0.5
        sd[k] = r.to(BF)
    m.load_state_dict(sd, strict=True)
    frames = (2 * torch.rand(4, 3, 224, 224, generator=torch.Generator().manual_seed(22)) - 1).to(BF)
    out = m.encode_frames(frames.to(DEV))
    assert out.shape == (4, m.out_dim) and torch.isfinite(out).all()
    exact = R.vit_forward(sd, cfg, kind, frames, dtype=torch.float32, device=DEV)
    torch_bf16 = R.rel_l2(R.vit_forward_torch_bf16(sd, cfg, kind, frames, device=DEV), exact)
    parity(R.rel_l2(out, exact), 1.5 * torch_bf16, f"{kind} real-width layer: error against fp32, bound 1.5 x the bf16 torch route ({torch_bf16:.3e})")
