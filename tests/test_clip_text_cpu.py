"""CPU: the CLIP text tower's host side (tokensgen_amd/clip_text.py), the restatement the GPU tests use (tests/clip_text_ref.py) pinned to the library's own float64
run stored in tests/golden/clip_text_tiny.pt (tools/make_clip_text_golden.py), the alignment formula against F.cosine_similarity, and every refusal.  No GPU, no
transformers."""
import ctypes
import json
import os

import pytest
import torch
import torch.nn.functional as Fn

import clip_text_ref as R

BF = torch.bfloat16
GPU_BOUND_FACTOR = 1.5          # tests/test_clip_text_gpu.py: error against float64 <= 1.5 x the error of the library's own bf16 run
RULES = ["argmax", "first"]


@pytest.fixture(scope="module")
def gold(golden_dir):
    return torch.load(os.path.join(golden_dir, "clip_text_tiny.pt"), weights_only=False)


def _cfg(gold, rule):
    return gold["config"] if rule == "argmax" else gold["config_first"]


# ---------------------------------------------------------------------------------------------------- the restatement, pinned
@pytest.mark.parametrize("rule", RULES)
def test_restatement_float64_reproduces_the_library(gold, rule):
    """... without any padding mask, against the library's run WITH the tokenizer-style mask: under causal attention the mask changes nothing"""
    cfg, ids = _cfg(gold, rule), gold["ids"]
    assert ids.shape == (3, 21) and gold["f64_" + rule].dtype == torch.float64 and sum(v.numel() for v in gold["state_dict"].values()) == 296960
    at = R.pooled_positions(ids, cfg["eos_token_id"])
    assert at.tolist() == {"argmax": [1, 15, 20], "first": [1, 10, 20]}[rule]              # BOS | EOS, the middle, S - 1; the two rules part on sequence 1
    mask = gold["mask_" + rule]
    assert torch.equal(mask, (torch.arange(21)[None] <= at[:, None]).long()) and int(mask.sum()) < mask.numel()          # a real padding mask was in the library's run
    err = R.rel_l2(R.clip_text_forward(gold["state_dict"], cfg, ids), gold["f64_" + rule])
    print(f"{rule}: float64 restatement (no mask) against the library's float64 run (tokenizer-style mask): rel-L2 {err:.3e}")
    assert err < 1e-10


@pytest.mark.parametrize("rule", RULES)
def test_tokens_after_the_pooled_position_do_not_matter(gold, rule):
    cfg, ids = _cfg(gold, rule), gold["ids"].clone()
    want = R.clip_text_forward(gold["state_dict"], cfg, ids)
    at = R.pooled_positions(ids, cfg["eos_token_id"])
    for b in range(3):
        ids[b, int(at[b]) + 1:] = 5
    assert torch.equal(R.pooled_positions(ids, cfg["eos_token_id"]), at) and not torch.equal(ids, gold["ids"])
    assert torch.equal(R.clip_text_forward(gold["state_dict"], cfg, ids), want)          # exactly 0.0


@pytest.mark.parametrize("rule", RULES)
def test_kernel_rounding_mode_is_inside_the_gpu_bound(gold, rule):
    """The planned rounding points, emulated on the CPU, must themselves sit inside the GPU bound (otherwise a correct kernel could not meet it)."""
    f64 = gold["f64_" + rule]
    lib = R.rel_l2(gold["bf16_" + rule], f64)
    emu = R.rel_l2(R.clip_text_forward(gold["state_dict"], _cfg(gold, rule), gold["ids"], rounding=True), f64)
    print(f"{rule}: library bf16 {lib:.3e}, kernel rounding points {emu:.3e} ({emu / lib:.2f} x)")
    assert emu < GPU_BOUND_FACTOR * lib


@pytest.mark.parametrize("rule", RULES)
def test_every_semantic_mutation_lands_three_times_beyond_the_gpu_bound(gold, rule):
    f64 = gold["f64_" + rule]
    bound = GPU_BOUND_FACTOR * R.rel_l2(gold["bf16_" + rule], f64)
    assert set(gold["mutation_ratios"][rule]) == set(R.MUTATIONS) and len(R.MUTATIONS) == 8
    for mut in R.MUTATIONS:
        err = R.rel_l2(R.clip_text_forward(gold["state_dict"], _cfg(gold, rule), gold["ids"], rounding=True, mutate=mut), f64)
        print(f"{rule} {mut}: {err:.3e} = {err / bound:.1f} x the bound (recorded {gold['mutation_ratios'][rule][mut]:.1f})")
        assert err >= 3.0 * bound, (mut, err, bound)


@pytest.mark.parametrize("rule", RULES)
def test_torch_bf16_route_is_a_yardstick_of_the_library_s_size(gold, rule):
    f64 = gold["f64_" + rule]
    lib = R.rel_l2(gold["bf16_" + rule], f64)
    route = R.rel_l2(R.clip_text_forward_torch_bf16(gold["state_dict"], _cfg(gold, rule), gold["ids"]), f64)
    print(f"{rule}: library bf16 {lib:.3e}, torch bf16 route {route:.3e} ({route / lib:.2f} x)")
    assert lib / 1.5 < route < 1.5 * lib


# ---------------------------------------------------------------------------------------------------- loading
def test_every_accepted_naming_loads_the_same_tensors(gold):
    from tokensgen_amd.clip_text import CLIPTextEncoder, canonical_state_dict
    sd, cfg = gold["state_dict"], gold["config"]
    bare = {(k[len("text_model."):] if k.startswith("text_model.") else k): v for k, v in sd.items()}          # the tower's own names + text_projection.weight
    whole = dict(sd, **{"logit_scale": torch.tensor(2.6592), "logit_bias": torch.tensor(0.0), "visual_projection.weight": torch.zeros(4, 4, dtype=BF),
                        "vision_model.embeddings.class_embedding": torch.zeros(4, dtype=BF), "vision_model.embeddings.position_ids": torch.arange(5)[None],
                        "text_model.embeddings.position_ids": torch.arange(24)[None]})                          # a whole CLIPModel, as older files store it
    assert set(bare) != set(sd) and "embeddings.token_embedding.weight" in bare
    for other in (bare, whole):
        c = canonical_state_dict(other)
        assert list(c) == list(sd) and all(torch.equal(c[k], sd[k]) for k in sd)
    models = []
    for src in (sd, bare, whole):
        m = CLIPTextEncoder(cfg, device="cpu")
        res = m.load_state_dict(src, strict=True)
        assert res.missing_keys == [] and res.unexpected_keys == []
        models.append(m)
    assert all(torch.equal(models[0]._w[k], m._w[k]) for m in models[1:] for k in m._w)
    out = models[0].state_dict()
    assert set(out) == set(sd) and all(torch.equal(out[k], sd[k]) for k in sd)          # the library's names; q_proj comes back without its 1/8
    e = "text_model.encoder.layers.1.self_attn."
    assert torch.equal(models[0]._w["l1.qkv_w"], torch.cat([sd[e + "q_proj.weight"] * 0.125, sd[e + "k_proj.weight"], sd[e + "v_proj.weight"]]))
    assert torch.equal(models[0]._w["l1.qkv_b"], torch.cat([sd[e + "q_proj.bias"] * 0.125, sd[e + "k_proj.bias"], sd[e + "v_proj.bias"]]))
    assert torch.equal((models[0]._w["l1.qkv_w"][:128].double() * 8).to(BF), sd[e + "q_proj.weight"])              # exact in bf16
    with pytest.raises(RuntimeError, match="missing keys \\['text_projection.weight'\\]"):
        CLIPTextEncoder(cfg, device="cpu").load_state_dict({k: v for k, v in sd.items() if k != "text_projection.weight"}, strict=True)
    with pytest.raises(RuntimeError, match="unexpected keys \\['classifier.weight'\\]"):
        CLIPTextEncoder(cfg, device="cpu").load_state_dict(dict(whole, **{"classifier.weight": sd["text_projection.weight"]}), strict=True)
    with pytest.raises(RuntimeError, match="size mismatch \\['text_projection.weight"):
        CLIPTextEncoder(cfg, device="cpu").load_state_dict(dict(sd, **{"text_projection.weight": torch.zeros(64, 128)}), strict=True)
    res = CLIPTextEncoder(cfg, device="cpu").load_state_dict({k: v for k, v in sd.items() if k != "text_projection.weight"}, strict=False)
    assert res.missing_keys == ["text_projection.weight"] and res.unexpected_keys == []
    # the vision half of such a dictionary still goes to the image tower, which drops this half
    from tokensgen_amd.vit import canonical_state_dict as vision_names
    assert set(vision_names(whole, "clip")) == {"visual_projection.weight", "vision_model.embeddings.class_embedding"}


def test_from_pretrained_reads_a_local_directory(gold, tmp_path):
    from safetensors.torch import save_file
    from tokensgen_amd.clip_text import CLIPTextEncoder
    sd = gold["state_dict"]
    text_cfg = {k: v for k, v in gold["config_first"].items() if k not in ("projection_dim", "other_eos_token_id")}
    d = tmp_path / "whole"                                                   # a whole CLIPModel: text_config + the top-level projection_dim
    d.mkdir()
    (d / "config.json").write_text(json.dumps(dict(model_type="clip", projection_dim=128, text_config=dict(text_cfg, model_type="clip_text_model"), vision_config={})))
    save_file({k: v.contiguous() for k, v in dict(sd, logit_scale=torch.tensor(2.6592)).items()}, str(d / "model.safetensors"))
    m = CLIPTextEncoder.from_pretrained(str(d), device="cpu")
    assert m.out_dim == 128 and m.config.eos_token_id == 90 and m.config.vocab_size == 96 and all(torch.equal(m.state_dict()[k], v) for k, v in sd.items())
    b = tmp_path / "tower"                                                   # a CLIPTextModelWithProjection directory with a .bin file
    b.mkdir()
    (b / "config.json").write_text(json.dumps(dict(gold["config"], model_type="clip_text_model")))
    torch.save(sd, str(b / "pytorch_model.bin"))
    m2 = CLIPTextEncoder.from_pretrained(str(b), device="cpu")
    assert m2.config.eos_token_id == 2 and all(torch.equal(m2.state_dict()[k], v) for k, v in sd.items())
    os.remove(str(b / "pytorch_model.bin"))
    with pytest.raises(Exception):
        CLIPTextEncoder.from_pretrained(str(b), device="cpu")


def test_defaults_are_the_base_patch32_text_config():
    from tokensgen_amd.clip_text import CLIPTextEncoder, causal_table
    m = CLIPTextEncoder(device="meta")
    c = m.config
    assert (c.vocab_size, c.hidden_size, c.intermediate_size, c.num_hidden_layers, c.num_attention_heads, c.max_position_embeddings, c.hidden_act, c.layer_norm_eps,
            c.projection_dim, c.eos_token_id) == (49408, 512, 2048, 12, 8, 77, "quick_gelu", 1e-5, 512, 2)
    assert m.out_dim == 512 and m.state_dict()["text_model.embeddings.token_embedding.weight"].shape == (49408, 512)
    # every GEMM is launched with at least the 1024 rows at which tg_gemm_bf16 changes kernels: a prompt's feature does not depend on its batch mates
    assert m._gemm_rows(77) == 1024 and m._gemm_rows(16 * 77) == 1232 and m._gemm_rows(1) == 1024
    # a longer-context checkpoint of the same architecture simply loads
    assert CLIPTextEncoder(dict(max_position_embeddings=248), device="meta").state_dict()["text_model.embeddings.position_embedding.weight"].shape == (248, 512)
    t = causal_table(2, 4, "cpu")                                            # index j - i + S - 1: zeros up to the diagonal, -inf for later keys
    assert t.dtype == torch.float32 and torch.equal(t, torch.tensor([[0, 0, 0, 0, float("-inf"), float("-inf"), float("-inf")]] * 2))
    assert torch.equal(causal_table(3, 1, "cpu"), torch.zeros(3, 1))


def test_encode_prompts_calls_the_tokenizer_as_documented(gold):
    from tokensgen_amd.clip_text import CLIPTextEncoder, encode_prompts
    m = CLIPTextEncoder(gold["config"], device="cpu")
    tok = R.StubTokenizer(gold["ids"], gold["mask_argmax"])
    with pytest.raises(RuntimeError, match="GPU"):                               # ids and mask pass every host check and reach the device check
        encode_prompts(tok, m, ["a", "b", "c"])
    with pytest.raises(RuntimeError, match="GPU"):
        encode_prompts(tok, m, "one prompt")
    assert tok.calls[0] == (["a", "b", "c"], dict(padding="max_length", truncation=True, max_length=24, return_tensors="pt")) and tok.calls[1][0] == ["one prompt"]


# ---------------------------------------------------------------------------------------------------- the alignment formula
def test_alignment_formula_against_the_golden_matrix(gold):
    cos, per_text, score = R.alignment(gold["img_f64"], gold["f64_argmax"])
    assert cos.dtype == torch.float64 and cos.shape == (6, 3)
    assert (cos - gold["cos"]).abs().max() < 1e-12 and (per_text - gold["per_text"]).abs().max() < 1e-12 and abs(score.item() - gold["score"].item()) < 1e-12
    want = torch.stack([torch.stack([Fn.cosine_similarity(gold["img_f64"][f], gold["f64_argmax"][k], dim=0) for k in range(3)]) for f in range(6)])
    assert (cos - want).abs().max() < 1e-12
    assert (gold["cos"] < 0).any() and (gold["cos"] > 0).any()                  # the clamp of per_text has something to do
    assert (per_text - want.clamp_min(0).mean(0)).abs().max() < 1e-12 and abs(score.item() - want.clamp_min(0).mean(0).mean().item()) < 1e-12
    z, _, _ = R.alignment(torch.zeros(2, 128), gold["f64_argmax"])              # a zero row: 0, not NaN
    assert torch.equal(z, torch.zeros(2, 3, dtype=torch.float64))


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals(gold):
    from tokensgen_amd import lib as L
    from tokensgen_amd.clip_text import CLIPTextEncoder
    from tokensgen_amd.metrics import VideoConsistency, video_text_alignment
    from tokensgen_amd.vit import ViTEncoder
    cfg, first = gold["config"], gold["config_first"]
    with pytest.raises(NotImplementedError, match="head dimension 64"):
        CLIPTextEncoder(dict(cfg, num_attention_heads=4), device="cpu")
    with pytest.raises(NotImplementedError, match="N % 128"):
        CLIPTextEncoder(dict(cfg, hidden_size=192, num_attention_heads=3), device="cpu")
    with pytest.raises(NotImplementedError, match="N % 128"):
        CLIPTextEncoder(dict(cfg, intermediate_size=224), device="cpu")
    with pytest.raises(NotImplementedError, match="N % 128"):
        CLIPTextEncoder(dict(cfg, projection_dim=96), device="cpu")
    with pytest.raises(NotImplementedError, match="max_position_embeddings = 513"):
        CLIPTextEncoder(dict(cfg, max_position_embeddings=513), device="meta")
    for a in ("relu", "gelu_new", "gelu_pytorch_tanh"):
        with pytest.raises(NotImplementedError, match="hidden_act"):
            CLIPTextEncoder(dict(cfg, hidden_act=a), device="cpu")
    assert CLIPTextEncoder(dict(cfg, hidden_act="gelu"), device="cpu").config.hidden_act == "gelu"
    m, mf = CLIPTextEncoder(cfg, device="cpu"), CLIPTextEncoder(first, device="cpu")
    with pytest.raises(NotImplementedError, match="requires_grad"):
        m.requires_grad_(True)
    assert m.requires_grad_(False) is m and m.eval() is m
    ids = gold["ids"]
    with pytest.raises(ValueError, match="max_position_embeddings = 24"):
        m.encode_text(torch.ones(2, 25, dtype=torch.int64))
    for bad in (96, -1):
        wrong = ids.clone()
        wrong[1, 3] = bad
        with pytest.raises(ValueError, match="\\[0, 96\\)"):
            m.encode_text(wrong)
    with pytest.raises(TypeError):
        m.encode_text(ids.float())
    with pytest.raises(ValueError):
        m.encode_text(torch.zeros(2, 3, 4, dtype=torch.int64))
    with pytest.raises(ValueError, match="no eos_token_id = 90"):
        mf.encode_text(torch.tensor([[1, 5, 90], [1, 5, 6]]))                     # the first-occurrence rule and a sequence without the token
    left = torch.cat([torch.zeros(3, 1, dtype=torch.long), gold["mask_first"][:, 1:]], dim=1)
    hole = gold["mask_first"].clone()
    hole[2, 4] = 0
    short = gold["mask_first"].clone()
    short[1, 10] = 0                                                              # right-padded, but the pooled position is masked
    for mask in (left, hole, short):
        with pytest.raises(NotImplementedError, match="right-padded"):
            mf.encode_text(ids, mask)
    with pytest.raises(ValueError, match="attention_mask"):
        mf.encode_text(ids, gold["mask_first"][:, :5])
    # everything valid reaches the device check: there is no CPU forward
    for model, mask in ((m, None), (m, gold["mask_argmax"]), (mf, gold["mask_first"]), (mf, torch.ones(3, 21, dtype=torch.long)), (m, None)):
        with pytest.raises(RuntimeError, match="GPU"):
            model.encode_text(ids.to(torch.int32) if mask is None else ids, mask)
    with pytest.raises(RuntimeError, match="GPU"):
        m.encode_text(ids[0])                                                     # [S]
    # the metric's argument checks come before any device work
    clip = ViTEncoder(dict(hidden_size=128, num_attention_heads=2, num_hidden_layers=1, intermediate_size=512, patch_size=8, image_size=32, projection_dim=128),
                      device="cpu", kind="clip")
    dino = ViTEncoder(dict(hidden_size=128, num_attention_heads=2, num_hidden_layers=1, intermediate_size=512, patch_size=8, image_size=40), device="cpu", kind="vit")
    frames = torch.zeros(2, 3, 32, 32, dtype=BF)
    with pytest.raises(ValueError, match="width 64"):
        video_text_alignment(frames, clip, torch.zeros(3, 64))
    with pytest.raises(ValueError, match="kind='clip'"):
        video_text_alignment(frames, dino, torch.zeros(3, 128))
    with pytest.raises(TypeError):
        video_text_alignment(frames, clip, torch.zeros(3, 128, dtype=torch.float64))
    with pytest.raises(ValueError, match="background_model"):
        VideoConsistency(subject_model=dino, text_features=torch.zeros(128))
    with pytest.raises(ValueError, match="width 64"):
        VideoConsistency(background_model=clip).new_video(text_features=torch.zeros(64))
    assert VideoConsistency(background_model=clip, text_features=torch.zeros(128))._text.shape == (1, 128)
    # the exports validate before any launch
    lib = L.load()
    assert lib.tg_text_embed(None, 0, 0, None, 0, None, None, 0, 0, None, None) == -1 and b"tg_text_embed: null pointer" in lib.tg_last_error_string()
    assert lib.tg_text_alignment(None, 0, 0, None, 0, 0, 0, None, None) == -1 and b"tg_text_alignment: null pointer" in lib.tg_last_error_string()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf) + (16 - ctypes.addressof(buf) % 16)
    assert lib.tg_text_embed(p, 4, 2, p, 8, p, p, 64, 64, None, None) == -1                                      # the status word is required
    assert lib.tg_text_embed(p, 4, 2, p, 8, p, p, 60, 60, p, None) == -2 and b"D % 8" in lib.tg_last_error_string()
    assert lib.tg_text_embed(p, 0, 2, p, 8, p, p, 64, 64, p, None) == -2 and lib.tg_text_embed(p, 4, 2, p, 0, p, p, 64, 64, p, None) == -2
    assert lib.tg_text_embed(p, 4, 2, p, 8, p, p, 32, 64, p, None) == -2                                          # ldo < D
    assert lib.tg_text_embed(p, 4, 2, p + 2, 8, p, p, 64, 64, p, None) == -3 and lib.tg_text_embed(p, 4, 2, p, 8, p, p, 68, 64, p, None) == -3
    assert lib.tg_text_alignment(p, 128, 0, p, 128, 1, 128, p, None) == -2 and lib.tg_text_alignment(p, 128, 1, p, 128, 0, 128, p, None) == -2
    assert lib.tg_text_alignment(p, 64, 1, p, 128, 1, 128, p, None) == -2 and b"leading dimensions" in lib.tg_last_error_string()
    assert lib.tg_text_alignment(p, 128, 1, p, 128, 1, 128, p + 4, None) == -3 and lib.tg_text_alignment(p + 2, 128, 1, p, 128, 1, 128, p, None) == -3
