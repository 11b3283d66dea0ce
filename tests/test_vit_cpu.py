"""CPU: the ViT encoders' host side (tokensgen_amd/vit.py), the restatement the GPU tests use (tests/vit_ref.py) pinned to the library's own float64 run stored in
tests/golden/vit_tiny.pt and vit_tiny_clip.pt (tools/make_vit_golden.py), the consistency formula against F.cosine_similarity, and every refusal.  No GPU, no
transformers."""
import ctypes
import json
import os

import pytest
import torch
import torch.nn.functional as Fn

import vit_ref as R

BF = torch.bfloat16
GPU_BOUND_FACTOR = 1.5          # tests/test_vit_gpu.py: error against float64 <= 1.5 x the error of the library's own bf16 run
FILES = {"vit": "vit_tiny.pt", "clip": "vit_tiny_clip.pt"}
KINDS = ["vit", "clip"]


@pytest.fixture(scope="module")
def gold(golden_dir):
    return {k: torch.load(os.path.join(golden_dir, f), weights_only=False) for k, f in FILES.items()}


# ---------------------------------------------------------------------------------------------------- the restatement, pinned
@pytest.mark.parametrize("kind", KINDS)
def test_restatement_float64_reproduces_the_library(gold, kind):
    g = gold[kind]
    assert g["kind"] == kind and g["frames"].dtype == BF and g["frames"].shape[0] == 6 and g["f64"].dtype == torch.float64
    S = (g["config"]["image_size"] // g["config"]["patch_size"]) ** 2 + 1
    assert S == {"vit": 26, "clip": 17}[kind] and S % 8
    err = R.rel_l2(R.vit_forward(g["state_dict"], g["config"], kind, g["frames"]), g["f64"])
    print(f"{kind}: float64 restatement against the library's float64 run: rel-L2 {err:.3e}")
    assert err < 1e-10


@pytest.mark.parametrize("kind", KINDS)
def test_kernel_rounding_mode_is_inside_the_gpu_bound(gold, kind):
    """The planned rounding points, emulated on the CPU, must themselves sit inside the GPU bound (otherwise a correct kernel could not meet it)."""
    g = gold[kind]
    lib = R.rel_l2(g["bf16"], g["f64"])
    emu = R.rel_l2(R.vit_forward(g["state_dict"], g["config"], kind, g["frames"], rounding=True), g["f64"])
    print(f"{kind}: library bf16 {lib:.3e}, kernel rounding points {emu:.3e} ({emu / lib:.2f} x)")
    assert emu < GPU_BOUND_FACTOR * lib


@pytest.mark.parametrize("kind", KINDS)
def test_every_semantic_mutation_lands_three_times_beyond_the_gpu_bound(gold, kind):
    g = gold[kind]
    bound = GPU_BOUND_FACTOR * R.rel_l2(g["bf16"], g["f64"])
    assert set(g["mutation_ratios"]) == set(R.MUTATIONS[kind])
    for mut in R.MUTATIONS[kind]:
        err = R.rel_l2(R.vit_forward(g["state_dict"], g["config"], kind, g["frames"], rounding=True, mutate=mut), g["f64"])
        print(f"{kind} {mut}: {err:.3e} = {err / bound:.1f} x the bound (recorded {g['mutation_ratios'][mut]:.1f})")
        assert err >= 3.0 * bound, (mut, err, bound)


@pytest.mark.parametrize("kind", KINDS)
def test_torch_bf16_route_is_a_yardstick_of_the_library_s_size(gold, kind):
    """vit_ref.vit_forward_torch_bf16 (the yardstick of the real-width GPU test, where no library run exists) has the library's size of error."""
    g = gold[kind]
    lib = R.rel_l2(g["bf16"], g["f64"])
    route = R.rel_l2(R.vit_forward_torch_bf16(g["state_dict"], g["config"], kind, g["frames"]), g["f64"])
    print(f"{kind}: library bf16 {lib:.3e}, torch bf16 route {route:.3e} ({route / lib:.2f} x)")
    assert lib / 1.5 < route < 1.5 * lib


# ---------------------------------------------------------------------------------------------------- loading
@pytest.mark.parametrize("kind", KINDS)
def test_both_name_families_load_the_same_tensors(gold, kind):
    from tokensgen_amd.vit import ViTEncoder, canonical_state_dict
    g = gold[kind]
    sd, files = g["state_dict"], g["state_dict_files"]
    assert set(sd) != set(files)
    a, b = canonical_state_dict(sd, kind), canonical_state_dict(files, kind)
    assert set(a) == set(b) == set(sd) and all(torch.equal(a[k], b[k]) for k in a)
    if kind == "vit":
        assert "encoder.layer.1.attention.attention.query.weight" in files and "layers.1.attention.q_proj.weight" in sd
        assert set(canonical_state_dict({"vit." + k: v for k, v in files.items()}, kind)) == set(sd)
        assert set(canonical_state_dict(dict(files, **{"pooler.dense.weight": sd["layernorm.weight"]}), kind)) == set(sd)
    else:
        assert {"logit_scale", "text_projection.weight", "vision_model.embeddings.position_ids"} <= set(files)          # a whole CLIPModel
    m1, m2 = ViTEncoder(g["config"], device="cpu", kind=kind), ViTEncoder(g["config"], device="cpu", kind=kind)
    m1.load_state_dict(sd, strict=True)
    m2.load_state_dict(files, strict=True)
    assert all(torch.equal(m1._w[k], m2._w[k]) for k in m1._w)
    out = m1.state_dict()
    assert set(out) == set(sd) and all(torch.equal(out[k], sd[k]) for k in sd)          # q_proj comes back without its 1/8
    # the packed storage: q | k | v rows with q scaled by 1/8 (exact), the patch convolution as zero-padded rows
    D = g["config"]["hidden_size"]
    attn = "layers.1.attention." if kind == "vit" else "vision_model.encoder.layers.1.self_attn."
    assert torch.equal(m1._w["l1.qkv_w"], torch.cat([sd[attn + "q_proj.weight"] * 0.125, sd[attn + "k_proj.weight"], sd[attn + "v_proj.weight"]]))
    assert torch.equal(m1._w["l1.qkv_b"], torch.cat([sd[attn + "q_proj.bias"] * 0.125, sd[attn + "k_proj.bias"], sd[attn + "v_proj.bias"]]))
    assert torch.equal((m1._w["l1.qkv_w"][:D].double() * 8).to(BF), sd[attn + "q_proj.weight"])
    conv = sd["embeddings.patch_embeddings.projection.weight" if kind == "vit" else "vision_model.embeddings.patch_embedding.weight"]
    assert m1.patch_kp == 192 and torch.equal(m1._w["patch_w"], conv.reshape(D, -1))
    # strict reports a missing and an unexpected key by name
    some = "layernorm.weight" if kind == "vit" else "visual_projection.weight"
    with pytest.raises(RuntimeError, match=f"missing keys \\['{some}'\\]"):
        ViTEncoder(g["config"], device="cpu", kind=kind).load_state_dict({k: v for k, v in sd.items() if k != some}, strict=True)
    with pytest.raises(RuntimeError, match="unexpected keys \\['classifier.weight'\\]"):
        ViTEncoder(g["config"], device="cpu", kind=kind).load_state_dict(dict(files, **{"classifier.weight": sd[some]}), strict=True)
    res = ViTEncoder(g["config"], device="cpu", kind=kind).load_state_dict({k: v for k, v in sd.items() if k != some}, strict=False)
    assert res.missing_keys == [some] and res.unexpected_keys == []


def test_patch_rows_pad_to_a_multiple_of_64():
    from tokensgen_amd.vit import ViTEncoder
    m = ViTEncoder(dict(hidden_size=1024, num_attention_heads=16, num_hidden_layers=1, intermediate_size=4096, image_size=224, patch_size=14, projection_dim=768),
                   device="meta", kind="clip")
    assert (m.patch_k, m.patch_kp, m.tokens, m.out_dim) == (588, 640, 257, 768)          # ViT-L/14
    sd = m.state_dict()
    assert sd["vision_model.embeddings.patch_embedding.weight"].shape == (1024, 3, 14, 14)
    b16 = ViTEncoder(device="meta", kind="vit")
    assert (b16.patch_kp, b16.tokens, b16.out_dim, b16.frames_per_launch) == (768, 197, 768, 64)
    b32 = ViTEncoder(device="meta", kind="clip")
    assert (b32.patch_kp, b32.tokens, b32.out_dim) == (3072, 50, 512)
    # every GEMM is launched with at least the 1024 rows at which tg_gemm_bf16 changes kernels: a short batch takes the kernels a long one takes
    assert b16._gemm_rows(2 * 197) == 1024 and b16._gemm_rows(64 * 197) == 64 * 197 and b16._gemm_rows(1) == 1024


@pytest.mark.parametrize("kind", KINDS)
def test_from_pretrained_reads_a_local_directory(gold, kind, tmp_path):
    from safetensors.torch import save_file
    from tokensgen_amd.vit import ViTEncoder
    g = gold[kind]
    cfg = dict(g["config"], model_type="vit") if kind == "vit" else dict(model_type="clip", projection_dim=128, vision_config=dict(g["config"], model_type="clip_vision_model"),
                                                                         text_config={})
    d = tmp_path / "st"
    d.mkdir()
    (d / "config.json").write_text(json.dumps(cfg))
    save_file({k: v.contiguous() for k, v in g["state_dict_files"].items()}, str(d / "model.safetensors"))
    m = ViTEncoder.from_pretrained(str(d), device="cpu")
    assert m.kind == kind and all(torch.equal(m.state_dict()[k], v) for k, v in g["state_dict"].items())
    assert m.image_mean == R.MEAN_STD[kind][0] and m.image_std == R.MEAN_STD[kind][1]
    b = tmp_path / "bin"
    b.mkdir()
    (b / "config.json").write_text(json.dumps(cfg))
    (b / "preprocessor_config.json").write_text(json.dumps(dict(image_mean=[0.5, 0.5, 0.5], image_std=[0.5, 0.5, 0.5], size=224)))
    torch.save(g["state_dict_files"], str(b / "pytorch_model.bin"))
    m2 = ViTEncoder.from_pretrained(str(b), device="cpu")
    assert all(torch.equal(m2.state_dict()[k], v) for k, v in g["state_dict"].items()) and m2.image_mean == (0.5, 0.5, 0.5)
    os.remove(str(b / "pytorch_model.bin"))
    with pytest.raises(Exception):
        ViTEncoder.from_pretrained(str(b), device="cpu")


# ---------------------------------------------------------------------------------------------------- preprocessing constants
@pytest.mark.parametrize("kind", KINDS)
def test_folded_preprocessing_constants(kind):
    from tokensgen_amd.vit import ViTEncoder, fold_preprocessing
    m = ViTEncoder(device="meta", kind=kind)
    mean, std = R.MEAN_STD[kind]
    assert m.image_mean == mean and m.image_std == std
    a, b = fold_preprocessing(m.image_mean, m.image_std)
    x = torch.linspace(-1, 1, 257, dtype=torch.float64)
    for c in range(3):
        want = ((x + 1) / 2 - mean[c]) / std[c]
        assert (x * a[c] + b[c] - want).abs().max() < 1e-14
        assert a[c] == 0.5 / std[c] and b[c] == (0.5 - mean[c]) / std[c]
    ra, rb = R.fold(mean, std)                                                             # the restatement holds the same constants, as fp32
    assert torch.equal(ra, torch.tensor(a, dtype=torch.float32).double()) and torch.equal(rb, torch.tensor(b, dtype=torch.float32).double())
    assert (0.0 * a[0] + b[0]) == (0.5 - mean[0]) / std[0]                                 # mid-grey
    over = ViTEncoder(dict(image_mean=(0.5, 0.5, 0.5), image_std=(0.5, 0.5, 0.5)), device="meta", kind=kind)
    assert fold_preprocessing(over.image_mean, over.image_std) == ([1.0, 1.0, 1.0], [0.0, 0.0, 0.0])


# ---------------------------------------------------------------------------------------------------- the consistency formula
def test_consistency_formula_equals_a_loop_over_cosine_similarity():
    f = R.special_features(128, seed=3)
    prev, first, score = R.consistency(f)
    d = f.double()
    want_prev = torch.stack([Fn.cosine_similarity(d[i], d[i - 1], dim=0).clamp_min(0) for i in range(1, 7)])
    want_first = torch.stack([Fn.cosine_similarity(d[i], d[0], dim=0).clamp_min(0) for i in range(1, 7)])
    assert prev.dtype == torch.float64 and (prev - want_prev).abs().max() < 1e-12 and (first - want_first).abs().max() < 1e-12
    assert abs(score.item() - ((want_prev + want_first) / 2).mean().item()) < 1e-12
    assert Fn.cosine_similarity(d[2], d[1], dim=0).item() < -0.999 and prev[1] == 0                      # a negative cosine, clamped
    assert abs(prev[3].item() - 1.0) < 1e-12                                                               # a repeated frame
    assert prev[4] == 0 and prev[5] == 0 and first[4] == 0 and torch.isfinite(prev).all()                  # a zero row: 0 on both sides, not NaN
    # carried rows: the second part of a video continues the first
    p2, f2, _ = R.consistency(f[3:], first=f[0], prev=f[2])
    assert torch.equal(p2, prev[2:]) and torch.equal(f2, first[2:])


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals(gold):
    from tokensgen_amd import lib as L
    from tokensgen_amd.metrics import VideoConsistency, video_consistency
    from tokensgen_amd.vit import ViTEncoder
    cfg = gold["vit"]["config"]
    with pytest.raises(NotImplementedError, match="head dimension 64"):
        ViTEncoder(dict(cfg, num_attention_heads=4), device="cpu", kind="vit")
    with pytest.raises(NotImplementedError, match="N % 128"):
        ViTEncoder(dict(cfg, hidden_size=192, num_attention_heads=3), device="cpu", kind="vit")
    with pytest.raises(NotImplementedError, match="N % 128"):
        ViTEncoder(dict(cfg, intermediate_size=480), device="cpu", kind="vit")
    with pytest.raises(NotImplementedError, match="N % 128"):
        ViTEncoder(dict(gold["clip"]["config"], projection_dim=96), device="cpu", kind="clip")
    with pytest.raises(NotImplementedError, match="S = 530"):
        ViTEncoder(dict(cfg, image_size=184), device="meta", kind="vit")                  # 23 x 23 + 1 tokens
    for a in ("relu", "gelu_new", "gelu_pytorch_tanh"):
        with pytest.raises(NotImplementedError, match="hidden_act"):
            ViTEncoder(dict(cfg, hidden_act=a), device="cpu", kind="vit")
    for extra in (dict(layerscale_value=1.0), dict(use_swiglu_ffn=True), dict(num_register_tokens=4), dict(model_type="dinov2")):
        with pytest.raises(NotImplementedError, match="DINOv2"):
            ViTEncoder(dict(cfg, **extra), device="cpu", kind="vit")
    with pytest.raises(ValueError, match="kind"):
        ViTEncoder(cfg, device="cpu")
    m = ViTEncoder(cfg, device="cpu", kind="vit")
    with pytest.raises(NotImplementedError, match="requires_grad"):
        m.requires_grad_(True)
    assert m.requires_grad_(False) is m and m.eval() is m
    with pytest.raises(NotImplementedError, match="requires_grad"):
        m.encode_frames(torch.zeros(2, 3, 40, 40, dtype=BF, requires_grad=True))
    with pytest.raises(NotImplementedError, match="image_size is 40.*not interpolated"):
        m.encode_frames(torch.zeros(2, 3, 48, 48, dtype=BF))
    with pytest.raises(TypeError):
        m.encode_frames(torch.zeros(2, 3, 40, 40))
    with pytest.raises(ValueError):
        m.encode_frames(torch.zeros(2, 40, 40, 4, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="GPU"):
        m.encode_frames(gold["vit"]["frames"])
    # fewer than 2 frames
    with pytest.raises(ValueError, match="at least 2"):
        video_consistency(gold["vit"]["frames"][:1], m)
    with pytest.raises(ValueError, match="at least 2"):
        video_consistency(torch.zeros(1, 1, 8, 8, 3, dtype=torch.uint8), m)
    with pytest.raises(ValueError, match="attach"):
        VideoConsistency()
    # the exports validate before any launch
    lib = L.load()
    f3 = (ctypes.c_float * 3)(1, 1, 1)
    assert lib.tg_vit_patch_rows(None, 0, 0, 0, 0, None, None, None, 0, None) == -1 and b"tg_vit_patch_rows: null pointer" in lib.tg_last_error_string()
    assert lib.tg_vit_assemble(None, None, None, None, 0, 0, 0, None) == -1 and b"tg_vit_assemble: null pointer" in lib.tg_last_error_string()
    assert lib.tg_layernorm(None, 0, None, None, None, 0, 0, 0, 0.0, None) == -1 and b"tg_layernorm: null pointer" in lib.tg_last_error_string()
    assert lib.tg_vit_act(None, None, 0, 0, None) == -1 and b"tg_vit_act: null pointer" in lib.tg_last_error_string()
    assert lib.tg_feature_consistency(None, 0, 0, 0, None, None, None, None, None) == -1 and b"tg_feature_consistency: null pointer" in lib.tg_last_error_string()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf) + (16 - ctypes.addressof(buf) % 16)
    assert lib.tg_vit_patch_rows(p, 1, 40, 42, 8, f3, f3, p, 192, None) == -2 and b"W % p" in lib.tg_last_error_string()
    assert lib.tg_vit_patch_rows(p, 1, 28, 28, 14, f3, f3, p, 588, None) == -2 and b"640" in lib.tg_last_error_string()          # Kp must be the padded width
    assert lib.tg_vit_patch_rows(p + 2, 1, 40, 40, 8, f3, f3, p, 192, None) == -3
    assert lib.tg_vit_assemble(p, p, p, p, 1, 25, 96, None) == -2 and lib.tg_vit_assemble(p, p + 2, p, p, 1, 25, 128, None) == -3
    assert lib.tg_layernorm(p, 96, p, p, p, 96, 1, 96, 1e-6, None) == -2 and b"D % 64" in lib.tg_last_error_string()
    assert lib.tg_layernorm(p, 8192, p, p, p, 8192, 1, 8192, 1e-6, None) == -2 and b"4096" in lib.tg_last_error_string()
    assert lib.tg_layernorm(p, 64, p, p, p, 128, 1, 128, 1e-6, None) == -2 and lib.tg_layernorm(p, 132, p, p, p, 128, 1, 128, 1e-6, None) == -3
    assert lib.tg_vit_act(p, p, 12, 0, None) == -2 and lib.tg_vit_act(p, p, 16, 2, None) == -1 and lib.tg_vit_act(p + 2, p, 16, 0, None) == -3
    assert lib.tg_feature_consistency(p, 128, 1, 128, None, None, p, p, None) == -2 and b"F >= 2" in lib.tg_last_error_string()
    assert lib.tg_feature_consistency(p, 128, 2, 128, p, None, p, p, None) == -1 and b"together" in lib.tg_last_error_string()
    assert lib.tg_feature_consistency(p, 64, 2, 128, None, None, p, p, None) == -2
    assert lib.tg_feature_consistency(p, 128, 2, 128, None, None, p + 4, p, None) == -3
