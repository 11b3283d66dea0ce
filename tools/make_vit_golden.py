"""Writes tests/golden/vit_tiny.pt (kind "vit") and tests/golden/vit_tiny_clip.pt (kind "clip"): a tiny image encoder of each kind with bf16-representable weights and
what the installed `transformers` computes from it.  Run on the CPU:

    python tools/make_vit_golden.py

Needs `transformers` (the tests do not).  One file per kind, because a committed file stays under 1 MiB and each model's weights are 0.85 MB.  Contents of a file:
  kind, config      hidden 128, 2 heads, 2 layers, MLP 512; "vit": image 40, patch 8 (S = 26), exact GELU, eps 1e-12 (ViTModel without pooler);
                    "clip": image 32, patch 8 (S = 17), quick GELU, eps 1e-5, projection 128 (CLIPVisionModelWithProjection).  S is no multiple of 8.
  state_dict        the library's in-memory names, bf16
  state_dict_files  the same tensors under the names stored in published checkpoint files ("vit": encoder.layer.N.attention.attention.query.weight, ...;
                    "clip": a whole CLIPModel: the vision names are the in-memory ones, beside a position_ids buffer, a logit scale and two text-tower entries)
  frames            bf16 [6, 3, s, s] in [-1, 1]
  f64, bf16         the library's features [6, 128] of ((frames + 1) / 2 - mean) / std, the model in float64 / in bfloat16 (its own error is the yardstick)
  mutation_ratios   error of each semantic mutation of tests/vit_ref.py (run with the kernels' rounding points) / (1.5 x the library's bf16 error)
The mutations give the whole-model bound of tests/test_vit_gpu.py (1.5 x the library's bf16 error) its meaning: each must land at least 3 x beyond it, asserted
here.  The weights are scaled for that: q and k large enough for scores of a few units after the 1/8; an fc1 bias near -4 ("vit") / -3 ("clip") with a large fc2, so that
the MLP works in the GELU's negative tail, the only place where the tanh form differs from the exact one by more than bf16 resolution (10 % at -3, 45 % at -4, against 0.02 %
at +2; the quick form differs from it there by more still); position rows and LayerNorm gains of ordinary size.  "cls_norm" is read as: the class token taken on the other side of the final norm (not normalised) —
a LayerNorm works per token, so normalising all tokens and then taking the first is no mutation at all."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vit_ref as R  # noqa: E402

BASE = dict(hidden_size=128, num_attention_heads=2, num_hidden_layers=2, intermediate_size=512, patch_size=8)
CONFIG = {"vit": dict(BASE, image_size=40, hidden_act="gelu", layer_norm_eps=1e-12),
          "clip": dict(BASE, image_size=32, hidden_act="quick_gelu", layer_norm_eps=1e-5, projection_dim=128)}
FILES = {"vit": "vit_tiny.pt", "clip": "vit_tiny_clip.pt"}
BOUND_FACTOR, MUTATION_MARGIN = 1.5, 3.0
# per kind: q / k element scale, fc1 weight gain, fc1 bias mean, fc2 gain
SCALES = {"vit": dict(qk=1.3, fc1=0.3, fc1_bias=-4.0, fc2=2000.0), "clip": dict(qk=1.3, fc1=0.3, fc1_bias=-3.0, fc2=100.0)}

_TO_FILE = (("attention.q_proj.", "attention.attention.query."), ("attention.k_proj.", "attention.attention.key."), ("attention.v_proj.", "attention.attention.value."),
            ("attention.o_proj.", "attention.output.dense."), ("mlp.fc1.", "intermediate.dense."), ("mlp.fc2.", "output.dense."))


def file_names(sd, kind):
    out = {}
    if kind == "vit":
        for k, v in sd.items():
            if k.startswith("layers."):
                k = "encoder.layer." + k[len("layers."):]
                for a, b in _TO_FILE:
                    k = k.replace(a, b)
            out[k] = v
        return out
    out.update(sd)
    S = sd["vision_model.embeddings.position_embedding.weight"].shape[0]
    out["vision_model.embeddings.position_ids"] = torch.arange(S)[None]
    out["logit_scale"] = torch.tensor(2.6592)
    out["text_projection.weight"] = torch.zeros(4, 4, dtype=torch.bfloat16)
    out["text_model.embeddings.token_embedding.weight"] = torch.zeros(4, 4, dtype=torch.bfloat16)
    return out


def library_model(kind, dtype):
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection, ViTConfig, ViTModel
    c = CONFIG[kind]
    if kind == "vit":
        return ViTModel(ViTConfig(**c, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0), add_pooling_layer=False).eval().to(dtype)
    return CLIPVisionModelWithProjection(CLIPVisionConfig(**c, attention_dropout=0.0)).eval().to(dtype)


def make(kind, seed):
    c, sc = CONFIG[kind], SCALES[kind]
    D, I = c["hidden_size"], c["intermediate_size"]
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in library_model(kind, torch.float32).state_dict().items():
        r = torch.randn(v.shape, generator=g)
        if "norm" in k and k.endswith("weight"):
            t = 1.0 + 0.25 * r
        elif "norm" in k:
            t = 0.1 * r
        elif "cls_token" in k or "class_embedding" in k or "position_embedding" in k:
            t = 0.7 * r
        elif "patch_embedding" in k and k.endswith("weight"):
            t = r * (3 * c["patch_size"] ** 2) ** -0.5
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
    s = c["image_size"]
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, s), torch.linspace(-1, 1, s), indexing="ij")
    frames = torch.stack([torch.stack([torch.sin(3.0 * xx * (1 + ch) + 0.4 * f) * torch.cos(2.0 * yy - 0.3 * f * ch) for ch in range(3)]) for f in range(6)])
    frames = (0.8 * frames + 0.15 * torch.randn(frames.shape, generator=g)).clamp(-1, 1).to(torch.bfloat16)
    mean, std = R.MEAN_STD[kind]
    pixels = R.preprocess(frames, mean, std)
    out = {}
    with torch.no_grad():
        for dtype, key in ((torch.float64, "f64"), (torch.bfloat16, "bf16")):
            m = library_model(kind, dtype)
            m.load_state_dict({k: v.to(dtype) for k, v in sd.items()}, strict=True)
            res = m(pixel_values=pixels.to(dtype))
            out[key] = (res.last_hidden_state[:, 0] if kind == "vit" else res.image_embeds).clone()
            assert out[key].dtype == dtype and out[key].shape == (6, 128)
    lib = R.rel_l2(out["bf16"], out["f64"])
    exact = R.rel_l2(R.vit_forward(sd, c, kind, frames), out["f64"])
    emu = R.rel_l2(R.vit_forward(sd, c, kind, frames, rounding=True), out["f64"])
    print(f"{kind}: library bf16 against its float64 run {lib:.3e}; restatement exact {exact:.1e}, with the kernels' rounding points {emu:.3e} ({emu / lib:.2f} x)")
    assert exact < 1e-10 and emu < BOUND_FACTOR * lib
    ratios = {}
    for mut in R.MUTATIONS[kind]:
        e = R.rel_l2(R.vit_forward(sd, c, kind, frames, rounding=True, mutate=mut), out["f64"])
        ratios[mut] = e / (BOUND_FACTOR * lib)
        print(f"  {mut}: {e:.3e} = {ratios[mut]:.1f} x the bound")
        assert ratios[mut] >= MUTATION_MARGIN, (kind, mut, ratios[mut])
    import transformers
    return dict(kind=kind, config=c, state_dict=sd, state_dict_files=file_names(sd, kind), frames=frames, f64=out["f64"], bf16=out["bf16"], mutation_ratios=ratios,
                bound_factor=BOUND_FACTOR, transformers_version=transformers.__version__)


def main():
    for kind, seed in (("vit", 31), ("clip", 32)):
        path = os.path.join(ROOT, "tests", "golden", FILES[kind])
        torch.save(make(kind, seed), path)
        size = os.path.getsize(path)
        print(f"wrote {path}: {size} bytes")
        assert size < 1 << 20, "a committed fixture stays under 1 MiB"


if __name__ == "__main__":
    sys.exit(main())
