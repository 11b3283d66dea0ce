"""Writes tests/golden/clip_text_tiny.pt: a tiny CLIP text tower with bf16-representable weights and what the installed `transformers` computes from it.
Run on the CPU:

    python tools/make_clip_text_golden.py

Needs `transformers` (the tests do not) and tests/golden/vit_tiny_clip.pt (tools/make_vit_golden.py), whose image features share the projection width.  Contents:
  config            hidden 128 = 2 heads x 64, 2 layers, MLP 256, vocabulary 96, 24 positions, projection 128, quick GELU, eps 1e-5 (CLIPTextModelWithProjection);
                    eos_token_id 2: the argmax pooling rule of the published OpenAI configurations.  296 960 parameters.
  config_first      the same with eos_token_id = END (90): the first-occurrence rule
  state_dict        the library's names, bf16
  ids               int64 [3, 21].  END ends every sequence: at position 1 (BOS, END, then END as padding), at 10 — with the larger id 95 (an "added token") at 15,
                    so the argmax rule pools row 15 and the first-occurrence rule row 10 — and at S - 1 = 20
  mask_argmax, mask_first   tokenizer-style right-padded masks [3, 21]: ones up to and including each rule's pooled position
  f64_argmax, f64_first     the library's float64 `text_embeds` [3, 128] under either rule, run WITH that mask
  bf16_argmax, bf16_first   the library's own bfloat16 `text_embeds` (its error is the yardstick)
  img_f64, cos, per_text, score   the library's float64 image features [6, 128] of vit_tiny_clip.pt's frames, their float64 cosine matrix [6, 3] with f64_argmax
                    (F.cosine_similarity), the mean over frames of max(0, cos) and its mean
  mutation_ratios   error of each semantic mutation of tests/clip_text_ref.py (run with the kernels' rounding points) / (1.5 x the library's bf16 error), per rule
Asserted here, in float64 under both rules: the library's `text_embeds` with the mask, without it, and with every token after the pooled position replaced differ by
exactly 0.0 — attention is causal, so no padding mask is needed.  The mutations give the whole-model bound of tests/test_clip_text_gpu.py (1.5 x the library's bf16
error) its meaning: each must land at least 3 x beyond it, asserted here; the weights are scaled for that as in tools/make_vit_golden.py (q and k for scores of a
few units after the 1/8, an fc1 bias near -3 with a large fc2 so that the MLP works where the quick and the tanh GELU differ)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import clip_text_ref as R  # noqa: E402

END, ADDED = 90, 95
CONFIG = dict(vocab_size=96, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, max_position_embeddings=24, projection_dim=128,
              hidden_act="quick_gelu", layer_norm_eps=1e-5, eos_token_id=2, other_eos_token_id=END)
CONFIG_FIRST = dict(CONFIG, eos_token_id=END, other_eos_token_id=2)
BOUND_FACTOR, MUTATION_MARGIN = 1.5, 3.0
SCALES = dict(qk=1.3, fc1=0.3, fc1_bias=-3.0, fc2=100.0)
PATH = os.path.join(ROOT, "tests", "golden", "clip_text_tiny.pt")


def library_model(cfg, dtype):
    from transformers import CLIPTextConfig, CLIPTextModelWithProjection
    c = {k: v for k, v in cfg.items() if k != "other_eos_token_id"}
    return CLIPTextModelWithProjection(CLIPTextConfig(**c, attention_dropout=0.0, bos_token_id=1, pad_token_id=END)).eval().to(dtype)


def make_ids(g):
    S = 21
    ids = torch.randint(3, END, (3, S), generator=g)
    ids[:, 0] = 1
    ids[0, 1:] = END                                       # BOS, END, padding
    ids[1, 10], ids[1, 11:] = END, END
    ids[1, 15] = ADDED                                     # an id above END after it: the two rules part here
    ids[2, S - 1] = END
    return ids


def masks(ids, eos):
    at = R.pooled_positions(ids, eos)
    return (torch.arange(ids.shape[1])[None] <= at[:, None]).long(), at


def main():
    g = torch.Generator().manual_seed(41)
    D, I, sc = CONFIG["hidden_size"], CONFIG["intermediate_size"], SCALES
    sd = {}
    for k, v in library_model(CONFIG, torch.float32).state_dict().items():
        r = torch.randn(v.shape, generator=g)
        if "norm" in k and k.endswith("weight"):
            t = 1.0 + 0.25 * r
        elif "norm" in k:
            t = 0.1 * r
        elif "embedding" in k:
            t = 0.7 * r
        elif ("q_proj" in k or "k_proj" in k) and k.endswith("weight"):
            t = r * D ** -0.5 * sc["qk"]
        elif "fc1.weight" in k:
            t = r * D ** -0.5 * sc["fc1"]
        elif "fc1.bias" in k:
            t = sc["fc1_bias"] + 0.3 * r
        elif "fc2.weight" in k:
            t = r * I ** -0.5 * sc["fc2"]
        elif k.endswith("weight"):
            t = r * v.shape[-1] ** -0.5
        else:
            t = 0.1 * r
        sd[k] = t.to(torch.bfloat16)
    assert sum(v.numel() for v in sd.values()) == 296960
    ids = make_ids(g)
    out = {}
    for rule, cfg in (("argmax", CONFIG), ("first", CONFIG_FIRST)):
        mask, at = masks(ids, cfg["eos_token_id"])
        out["mask_" + rule] = mask
        with torch.no_grad():
            for dtype, key in ((torch.float64, "f64_"), (torch.bfloat16, "bf16_")):
                m = library_model(cfg, dtype)
                m.load_state_dict({k: v.to(dtype) for k, v in sd.items()}, strict=True)
                out[key + rule] = m(input_ids=ids, attention_mask=mask).text_embeds.clone()
                assert out[key + rule].dtype == dtype and out[key + rule].shape == (3, 128)
                if dtype == torch.float64:
                    # no padding mask is needed: without it, and with every later token replaced (by ids the pooling rule does not react to), exactly the same
                    other = ids.clone()
                    for b in range(3):
                        other[b, at[b] + 1:] = torch.randint(3, END, (ids.shape[1] - int(at[b]) - 1,), generator=g)
                    assert torch.equal(R.pooled_positions(other, cfg["eos_token_id"]), at)
                    for variant in (m(input_ids=ids).text_embeds, m(input_ids=other, attention_mask=mask).text_embeds, m(input_ids=other).text_embeds):
                        diff = (variant - out[key + rule]).abs().max().item()
                        print(f"{rule}: with the mask against a variant without it / with later tokens replaced: max |diff| {diff}")
                        assert diff == 0.0
        print(f"{rule}: pooled positions {at.tolist()}")
    assert not torch.equal(masks(ids, 2)[1], masks(ids, END)[1])
    ratios = {}
    for rule, cfg in (("argmax", CONFIG), ("first", CONFIG_FIRST)):
        f64 = out["f64_" + rule]
        lib = R.rel_l2(out["bf16_" + rule], f64)
        exact = R.rel_l2(R.clip_text_forward(sd, cfg, ids), f64)
        emu = R.rel_l2(R.clip_text_forward(sd, cfg, ids, rounding=True), f64)
        print(f"{rule}: library bf16 against its float64 run {lib:.3e}; restatement exact {exact:.1e}, with the kernels' rounding points {emu:.3e} ({emu / lib:.2f} x)")
        assert exact < 1e-10 and emu < BOUND_FACTOR * lib
        ratios[rule] = {}
        for mut in R.MUTATIONS:
            e = R.rel_l2(R.clip_text_forward(sd, cfg, ids, rounding=True, mutate=mut), f64)
            ratios[rule][mut] = e / (BOUND_FACTOR * lib)
            print(f"  {mut}: {e:.3e} = {ratios[rule][mut]:.1f} x the bound")
            assert ratios[rule][mut] >= MUTATION_MARGIN, (rule, mut, ratios[rule][mut])
    img = torch.load(os.path.join(ROOT, "tests", "golden", "vit_tiny_clip.pt"), weights_only=False)["f64"].double()
    cos = torch.nn.functional.cosine_similarity(img[:, None, :], out["f64_argmax"][None, :, :], dim=-1)
    assert cos.shape == (6, 3) and cos.dtype == torch.float64 and (cos < 0).any() and (cos > 0).any()
    per_text = cos.clamp_min(0.0).mean(dim=0)
    import transformers
    torch.save(dict(config=CONFIG, config_first=CONFIG_FIRST, state_dict=sd, ids=ids, img_f64=img, cos=cos, per_text=per_text, score=per_text.mean(),
                    mutation_ratios=ratios, bound_factor=BOUND_FACTOR, transformers_version=transformers.__version__, **out), PATH)
    size = os.path.getsize(PATH)
    print(f"wrote {PATH}: {size} bytes")
    assert size < 1 << 20, "a committed fixture stays under 1 MiB"


if __name__ == "__main__":
    sys.exit(main())
