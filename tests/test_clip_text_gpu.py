"""GPU: the CLIP text tower's kernels (csrc/clip_text.hip), tg_t5_attention under the causal bias table, the tower built from them (tokensgen_amd/clip_text.py) and
the text-video alignment metric (tokensgen_amd/metrics.py).

The tolerance method is tests/test_vit_gpu.py's.  Per kernel: inputs are bf16 values; the reference is tests/clip_text_ref.py in exact float64; the bound is 2 x the
error that its kernel-rounding mode (bf16 wherever the kernel stores bf16) has against that reference on the same inputs.  Where that emulation is exact — tg_text_embed:
one rounding per element of an exact fp32 sum — the kernel must be exact too (the bound is then 1e-12, for the strict `<`).  tg_text_alignment is a float64 formula:
1e-12, from D * 2^-53 = 6e-14 for a sum of D = 512 products.  Whole model: the error against the library's float64 `text_embeds` stored in
tests/golden/clip_text_tiny.pt must be at most 1.5 x the error of the library's own bf16 run stored beside them; tests/test_clip_text_cpu.py shows that the kernels'
rounding points emulated on the CPU land at 0.7 x of it and that every semantic mutation lands >= 3 x beyond the bound."""
import os

import pytest
import torch

import clip_text_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
F64 = torch.float64
RULES = ["argmax", "first"]
NEG_INF = float("-inf")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return torch.load(os.path.join(golden_dir, "clip_text_tiny.pt"), weights_only=False)


@pytest.fixture(scope="module")
def image_gold(golden_dir):
    return torch.load(os.path.join(golden_dir, "vit_tiny_clip.pt"), weights_only=False)


@pytest.fixture(scope="module")
def tiny(gold):
    from tokensgen_amd.clip_text import CLIPTextEncoder
    out = {}
    for rule in RULES:
        m = CLIPTextEncoder(gold["config" if rule == "argmax" else "config_first"], device=DEV)
        m.load_state_dict(gold["state_dict"], strict=True)
        out[rule] = m
    return out


@pytest.fixture(scope="module")
def tiny_features(gold, tiny):
    """encode_text of the fixture's [3, 21] ids under either pooling rule: computed once, shared, left unchanged"""
    return {rule: tiny[rule].encode_text(gold["ids"]) for rule in RULES}


@pytest.fixture(scope="module")
def image_model(image_gold):
    from tokensgen_amd.vit import ViTEncoder
    m = ViTEncoder(image_gold["config"], device=DEV, kind="clip")
    m.load_state_dict(image_gold["state_dict"], strict=True)
    return m


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


# ---------------------------------------------------------------------------------------------------- tg_text_embed
@pytest.mark.timeout(120)
@pytest.mark.parametrize("B,S,D", [(3, 21, 128), (2, 77, 512), (1, 1, 64)])
def test_text_embed_exact(B, S, D, parity):
    """one rounding per element of an exact fp32 sum: bitwise against the restatement's rounding mode; nothing written past the last row; ids outside [0, V) give
    zero rows and are counted, and no other row changes"""
    from tokensgen_amd import kernels as K
    V, rows = 96, B * S
    g = torch.Generator().manual_seed(rows + D)
    tok, pos = _randn((V, D), rows), _randn((S + 3, D), rows + 1, 0.7)
    ids = torch.randint(0, V, (B, S), generator=g)
    ids.view(-1)[0], ids.view(-1)[-1] = 0, V - 1                                              # both ends of the table
    want = R.embed(ids, tok.double(), pos.double(), rounding=True).reshape(rows, D)
    exact = R.embed(ids, tok.double(), pos.double()).reshape(rows, D)
    out = torch.full((rows + 1, D), 7.0, dtype=BF, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    K.text_embed(ids.to(torch.int32).view(-1).to(DEV), S, tok.to(DEV), pos.to(DEV), out, status)
    parity((out[:rows].double().cpu() - want).abs().max(), 1e-12, f"tg_text_embed rows {rows} D {D}: max |kernel - restatement with the kernel's rounding|")
    assert (out[rows] == 7.0).all() and status.item() == 0                                    # the canary row; nothing refused
    parity(R.rel_l2(out[:rows], exact), _bound(want, exact), f"tg_text_embed rows {rows} D {D}: against the exact sum")
    # a row stride that is not D: the same bits
    wide = torch.full((rows, D + 64), 7.0, dtype=BF, device=DEV)
    K.text_embed(ids.to(torch.int32).view(-1).to(DEV), S, tok.to(DEV), pos.to(DEV), wide[:, :D], status)
    assert torch.equal(wide[:, :D], out[:rows]) and (wide[:, D:] == 7.0).all()
    if rows > 2:
        bad = ids.clone().view(-1)
        bad[1], bad[rows - 2] = V, -1
        out2 = torch.full((rows + 1, D), 7.0, dtype=BF, device=DEV)
        K.text_embed(bad.to(torch.int32).to(DEV), S, tok.to(DEV), pos.to(DEV), out2, status)
        assert status.item() == 2
        assert (out2[1] == 0).all() and (out2[rows - 2] == 0).all() and (out2[rows] == 7.0).all()
        keep = torch.ones(rows + 1, dtype=torch.bool)
        keep[1] = keep[rows - 2] = False
        assert torch.equal(out2[keep.to(DEV)], out[keep.to(DEV)])


# ---------------------------------------------------------------------------------------------------- tg_t5_attention, causal
def _causal_inputs(S, B=2, H=2):
    qkv = _randn((B, S, 3 * H * 64), 100 + S)
    qkv[..., :2 * H * 64] *= 1.6                      # scores of a few units after the scale
    scaled = qkv.clone()
    scaled[..., :H * 64] = (qkv[..., :H * 64].float() * 0.125).to(BF)                         # as the loader leaves q_proj: exact in bf16
    return qkv, scaled


@pytest.mark.timeout(120)
@pytest.mark.parametrize("S", [77, 21, 1])
def test_causal_attention_vs_float64(S, parity):
    """tg_t5_attention with the causal bias table (0 for key <= query, -inf beyond) against float64 causal softmax attention with the 1/8 scale"""
    from tokensgen_amd import kernels as K
    from tokensgen_amd.clip_text import causal_table
    B, H = 2, 2
    qkv, scaled = _causal_inputs(S, B, H)
    q, k, v = (t.to(F64).view(B, S, H, 64) for t in qkv.split(H * 64, dim=-1))
    exact, emulated = R.causal_attention(q, k, v, 0.125), R.causal_attention(q, k, v, 0.125, rounding=True)
    table = causal_table(H, S, DEV)
    assert table.shape == (H, 2 * S - 1) and (table[:, :S] == 0).all() and (table[:, S:] == NEG_INF).all()
    out = torch.empty(B, S, H * 64, dtype=BF, device=DEV)
    K.t5_attention(scaled.to(DEV), table, out, H)
    assert torch.isfinite(out).all()
    parity(R.rel_l2(out, exact), _bound(emulated, exact), f"tg_t5_attention with the causal table, S {S}")
    # query 0 sees key 0 alone: its output is v[0], to the bit
    assert torch.equal(out[:, 0].cpu(), qkv[:, 0, 2 * H * 64:])


@pytest.mark.timeout(120)
@pytest.mark.parametrize("S", [77, 21])
def test_causal_attention_ignores_later_keys_bitwise(S):
    """K and V rows after position i replaced by other finite values, large ones included: output row i keeps its bits, at the 16-key tile edges"""
    from tokensgen_amd import kernels as K
    from tokensgen_amd.clip_text import causal_table
    B, H = 2, 2
    _, scaled = _causal_inputs(S, B, H)
    table = causal_table(H, S, DEV)
    base = torch.empty(B, S, H * 64, dtype=BF, device=DEV)
    K.t5_attention(scaled.to(DEV), table, base, H)
    for i in (0, 15, 16, S - 1):
        other = scaled.clone()
        if i + 1 < S:
            repl = _randn((B, S - i - 1, 2 * H * 64), 7 * S + i, 40.0)
            repl[:, 0::3, :64] = 1e30                                                        # large, finite: scores of +-1e31 under the mask
            repl[:, 1::3, 64:128] = -1e30
            repl[:, 0::2, 2 * H * 64 - 64:] = 3e30                                            # ... and values that an inexact 0 in P would let through
            other[:, i + 1:, H * 64:] = repl
            assert torch.isfinite(other.float()).all() and not torch.equal(other, scaled)
        out = torch.empty(B, S, H * 64, dtype=BF, device=DEV)
        K.t5_attention(other.to(DEV), table, out, H)
        assert torch.equal(out[:, :i + 1], base[:, :i + 1]), f"S {S}: rows up to {i} changed with the keys after {i}"
        assert torch.isfinite(out[:, :i + 1]).all()


# ---------------------------------------------------------------------------------------------------- tg_text_alignment
@pytest.mark.timeout(120)
@pytest.mark.parametrize("D", [128, 512])
@pytest.mark.parametrize("Kt", [1, 3])
@pytest.mark.parametrize("F", [1, 6, 70])
def test_text_alignment_vs_float64(F, Kt, D, parity):
    from tokensgen_amd import kernels as K
    g = torch.Generator().manual_seed(F * D + Kt)
    base = torch.randn(D, generator=g)
    img = 0.5 * base[None] + torch.randn(F, D, generator=g)
    txt = 0.5 * base[None] + torch.randn(Kt, D, generator=g)
    txt[0] = -txt[0]                                                                          # negative cosines: the kernel does not clamp
    if F > 1:
        img[1] = 0                                                                            # a zero row: 0, not NaN
    want, _, _ = R.alignment(img, txt)
    cos = K.text_alignment(img.to(DEV), txt.to(DEV))
    assert cos.dtype == F64 and cos.shape == (F, Kt) and torch.isfinite(cos).all()
    parity((cos.cpu() - want).abs().max(), 1e-12, f"tg_text_alignment F {F} K {Kt} D {D}: max |kernel - float64 torch|")
    assert torch.equal(cos.cpu() < 0, want < 0) and (want[:, 0] < 0).any() and (F == 1 or (cos[1] == 0).all())
    assert torch.equal(K.text_alignment(img.to(DEV), txt.to(DEV)), cos)                       # two launches: the same bits
    wide_i, wide_t = torch.full((F, D + 40), float("nan"), device=DEV), torch.full((Kt, D + 8), float("nan"), device=DEV)
    wide_i[:, :D], wide_t[:, :D] = img, txt                                                   # row strides that are not D
    assert torch.equal(K.text_alignment(wide_i[:, :D], wide_t[:, :D]), cos)
    if F > 1:                                                                                 # an output depends on its two rows alone
        assert torch.equal(K.text_alignment(img[F // 2:].to(DEV), txt[-1:].to(DEV)), cos[F // 2:, -1:])


# ---------------------------------------------------------------------------------------------------- the model
@pytest.mark.timeout(120)
@pytest.mark.parametrize("rule", RULES)
def test_tiny_model_vs_library_float64(rule, gold, tiny_features, parity):
    out, f64 = tiny_features[rule], gold["f64_" + rule]
    assert out.dtype == torch.float32 and out.shape == (3, 128) and out.is_cuda and torch.isfinite(out).all()
    library = R.rel_l2(gold["bf16_" + rule], f64)
    parity(R.rel_l2(out, f64), 1.5 * library, f"clip text tiny, {rule} pooling: error against float64, bound 1.5 x the library's bf16 run ({library:.3e})")


@pytest.mark.timeout(120)
def test_the_two_pooling_rules_part_on_the_second_sequence(tiny_features):
    a, b = tiny_features["argmax"], tiny_features["first"]
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and not torch.equal(a[1], b[1])


@pytest.mark.timeout(120)
@pytest.mark.parametrize("rule", RULES)
def test_a_prompt_s_feature_does_not_depend_on_the_call(rule, gold, tiny, tiny_features):
    m, ids = tiny[rule], gold["ids"]
    for b in range(3):
        assert torch.equal(m.encode_text(ids[b:b + 1])[0], tiny_features[rule][b])            # B = 1 against B = 3
    assert torch.equal(m.encode_text(ids[1]), tiny_features[rule][1:2])                      # [S]
    assert torch.equal(m.encode_text(ids.to(torch.int32).to(DEV), gold["mask_" + rule]), tiny_features[rule])          # int32 on the device, with the tokenizer's mask
    from tokensgen_amd.clip_text import encode_prompts
    assert torch.equal(encode_prompts(R.StubTokenizer(ids, gold["mask_" + rule]), m, ["a", "b", "c"]), tiny_features[rule])          # the tokenizer's ids and mask, passed on
    m.prompts_per_launch = 2                                                                  # ... and the batch cut into 2 + 1
    try:
        assert torch.equal(m.encode_text(ids), tiny_features[rule])
    finally:
        m.prompts_per_launch = 64


@pytest.mark.timeout(120)
def test_launches_per_forward(gold, tiny):
    """2 prompts through a tower of L layers: the embedding, ten launches per block, the final LayerNorm, the projection.  No other kernel."""
    m, ids = tiny["argmax"], gold["ids"][:2]
    L = m.config.num_hidden_layers
    assert _launch_counts(lambda: m.encode_text(ids)) == {"text_embed": 1, "gemm": 4 * L + 1, "layernorm": 2 * L + 1, "t5_attention": L, "residual_add": 2 * L,
                                                          "vit_act": L}


@pytest.mark.timeout(120)
@pytest.mark.parametrize("rule", RULES)
def test_tokens_after_the_pooled_position_do_not_matter(rule, gold, tiny, tiny_features):
    ids = gold["ids"].clone()
    at = R.pooled_positions(ids, tiny[rule].config.eos_token_id)
    for b in range(3):
        ids[b, int(at[b]) + 1:] = torch.randint(3, 90, (21 - int(at[b]) - 1,), generator=torch.Generator().manual_seed(b))
    assert torch.equal(R.pooled_positions(ids, tiny[rule].config.eos_token_id), at) and not torch.equal(ids, gold["ids"])
    assert torch.equal(tiny[rule].encode_text(ids), tiny_features[rule])


@pytest.mark.timeout(300)
def test_one_real_width_layer(parity):
    """hidden 512, 8 heads, MLP 2048, one layer, S = 77, B = 3, projection 512, random weights, the pooled row at three different positions.  Reference: the
    restatement in exact float64.  Bound: the per-kernel method's, 2 x the error of the restatement's kernel-rounding mode against it.  The bf16 torch route (torch
    ops on bf16 tensors, on the GPU) is held beside it: by the triangle inequality the tower is within (that bound + the route's own error) of the route."""
    from tokensgen_amd.clip_text import CLIPTextEncoder
    cfg = dict(vocab_size=1024, hidden_size=512, intermediate_size=2048, num_hidden_layers=1, num_attention_heads=8, max_position_embeddings=77, projection_dim=512,
               hidden_act="quick_gelu", layer_norm_eps=1e-5, eos_token_id=2)
    m = CLIPTextEncoder(cfg, device=DEV)
    g = torch.Generator().manual_seed(51)
    sd = {}
    for k, v in m.state_dict().items():
        r = torch.randn(v.shape, generator=g)
        if "norm" in k and k.endswith("weight"):
            r = 1.0 + 0.25 * r
        elif "norm" in k or k.endswith("bias"):
            r = 0.1 * r
        elif "embedding" in k:
            r = 0.7 * r
        elif "q_proj" in k or "k_proj" in k:
            r = r * 512 ** -0.5 * 1.3
        else:
            r = r * v.shape[-1] ** -0.5
        sd[k] = r.to(BF)
    m.load_state_dict(sd, strict=True)
    ids = torch.randint(3, 1000, (3, 77), generator=g)
    ids[0, 76], ids[1, 40], ids[2, 1] = 1023, 1023, 1023                                      # argmax pooling: rows 76, 40 and 1
    out = m.encode_text(ids)
    assert out.shape == (3, 512) and torch.isfinite(out).all()
    exact = R.clip_text_forward(sd, cfg, ids)
    emulated = R.clip_text_forward(sd, cfg, ids, rounding=True)
    route = R.clip_text_forward_torch_bf16(sd, cfg, ids, device=DEV)
    bound, route_err = _bound(emulated, exact), R.rel_l2(route, exact)
    parity(R.rel_l2(out, exact), bound, f"clip text real-width layer: error against float64, bound 2 x the kernel-rounding emulation; the bf16 torch route has {route_err:.3e}")
    parity(R.rel_l2(out, route), bound + route_err, "clip text real-width layer: against the bf16 torch route, bound = (bound against float64) + (the route's error)")


# ---------------------------------------------------------------------------------------------------- the metric
@pytest.mark.timeout(120)
def test_video_text_alignment_vs_float64_features(gold, image_gold, image_model, tiny_features, parity):
    """cos against the float64 matrix from the library's float64 image and text features.  A feature with relative error eps moves its unit vector by at most
    2 eps / (1 - eps) (tests/test_vit_gpu.py), so the cosine of an image feature (eps_i) and a text feature (eps_t) moves by at most
    2 eps_i / (1 - eps_i) + 2 eps_t / (1 - eps_t); eps_i, eps_t: the per-row feature bounds, 1.5 x the library's bf16 error on its worst row.  Derived, not measured.
    per_text and score are means of max(0, cos), a 1-Lipschitz function: the same bound."""
    from tokensgen_amd.metrics import video_text_alignment
    txt = tiny_features["argmax"]
    res = video_text_alignment(image_gold["frames"].to(DEV), image_model, txt)
    assert res["cos"].dtype == F64 and res["cos"].shape == (6, 3) and res["per_text"].shape == (3,) and res["score"].dim() == 0 and res["cos"].is_cuda
    assert torch.equal(gold["img_f64"], image_gold["f64"].double())
    eps_i = 1.5 * max(R.rel_l2(image_gold["bf16"][i], image_gold["f64"][i]) for i in range(6))
    eps_t = 1.5 * max(R.rel_l2(gold["bf16_argmax"][k], gold["f64_argmax"][k]) for k in range(3))
    feats = image_model.encode_frames(image_gold["frames"].to(DEV))
    parity(max(R.rel_l2(feats[i], image_gold["f64"][i]) for i in range(6)), eps_i, "clip tiny: the worst frame's image-feature error, bound 1.5 x the library's worst frame")
    parity(max(R.rel_l2(txt[k], gold["f64_argmax"][k]) for k in range(3)), eps_t, "clip text tiny: the worst prompt's text-feature error, bound 1.5 x the library's worst prompt")
    bound = 2 * eps_i / (1 - eps_i) + 2 * eps_t / (1 - eps_t)
    parity((res["cos"].cpu() - gold["cos"]).abs().max(), bound, "video_text_alignment tiny: cos against float64 features")
    parity((res["per_text"].cpu() - gold["per_text"]).abs().max(), bound, "video_text_alignment tiny: per_text against float64 features")
    parity(abs(res["score"].item() - gold["score"].item()), bound, "video_text_alignment tiny: score against float64 features")
    own = R.alignment(feats.cpu(), txt.cpu())                                                 # on the towers' own features the kernel is a float64 formula
    assert (res["cos"].cpu() - own[0]).abs().max() < 1e-12 and (res["per_text"].cpu() - own[1]).abs().max() < 1e-12 and abs(res["score"].item() - own[2].item()) < 1e-12
    one = video_text_alignment(image_gold["frames"][:1].to(DEV), image_model, txt[2])          # one frame, one text [D]
    assert one["cos"].shape == (1, 1) and torch.equal(one["cos"][0, 0], res["cos"][0, 2])


class _Counting:
    """a background model that counts its encode_frames calls"""

    def __init__(self, model):
        self._model, self.calls, self.frames = model, 0, 0

    def __getattr__(self, name):
        return getattr(self._model, name)

    def encode_frames(self, frames):
        self.calls += 1
        self.frames += frames.shape[0]
        return self._model.encode_frames(frames)


@pytest.mark.timeout(120)
def test_streaming_alignment_gives_the_bits_of_one_call_and_encodes_once(image_model, tiny_features):
    from tokensgen_amd.metrics import VideoConsistency, video_consistency, video_text_alignment
    u8 = torch.randint(0, 256, (16, 48, 64, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(10)).to(DEV)
    a, b = u8[:10], u8[10:]
    txt_a, txt_b = tiny_features["argmax"], tiny_features["first"][1]
    whole_a, whole_b = video_text_alignment(a, image_model, txt_a), video_text_alignment(b, image_model, txt_b)
    cons_a, cons_b = video_consistency(a, image_model), video_consistency(b, image_model)
    counts = {}
    results = {}
    for with_text in (False, True):
        bg = _Counting(image_model)
        vc = VideoConsistency(background_model=bg, text_features=txt_a if with_text else None)
        for lo, hi in ((0, 4), (4, 5), (5, 10)):
            vc.update(a[lo:hi])
        vc.new_video(text_features=txt_b if with_text else None)
        vc.update(b[:1])
        vc.update(b[1:])
        results[with_text], counts[with_text] = vc.finalize(), (bg.calls, bg.frames)
    assert counts[True] == counts[False] == (5, 16)                                           # the frames go through the CLIP trunk once, alignment or not
    plain, res = results[False], results[True]
    # without text features: exactly the keys and the bits of the consistency-only class
    assert set(plain) == {"background_scores", "background_consistency", "background_prev", "background_first", "videos"} and plain["videos"] == 2
    for r in (plain, res):
        assert torch.equal(r["background_prev"][0], cons_a["prev"]) and torch.equal(r["background_first"][0], cons_a["first"])
        assert torch.equal(r["background_prev"][1], cons_b["prev"]) and torch.equal(r["background_first"][1], cons_b["first"])
        assert torch.equal(r["background_scores"], torch.stack([cons_a["score"], cons_b["score"]])) and torch.equal(r["background_consistency"], r["background_scores"].mean())
    assert set(res) == set(plain) | {"text_cos", "text_alignment", "text_alignment_mean"}
    # with them: 10 frames fed as 4 + 1 + 5 give the bits of one call on the whole video
    assert torch.equal(res["text_cos"][0], whole_a["cos"]) and res["text_cos"][0].shape == (10, 3)
    assert torch.equal(res["text_cos"][1], whole_b["cos"]) and res["text_cos"][1].shape == (6, 1)
    assert torch.equal(res["text_alignment"], torch.stack([whole_a["score"], whole_b["score"]])) and res["text_alignment"].dtype == F64
    assert torch.equal(res["text_alignment_mean"], res["text_alignment"].mean())
    # a video without text features among videos with them: no curve, NaN, left out of the mean
    vc = VideoConsistency(background_model=image_model)
    vc.update(a)
    vc.new_video(text_features=txt_b)
    vc.update(b)
    mixed = vc.finalize()
    assert mixed["text_cos"][0] is None and torch.equal(mixed["text_cos"][1], whole_b["cos"]) and torch.isnan(mixed["text_alignment"][0])
    assert torch.equal(mixed["text_alignment"][1], whole_b["score"]) and torch.equal(mixed["text_alignment_mean"], whole_b["score"])
