"""Writes tests/golden/t5_tiny.pt: a tiny T5 encoder with bf16-representable weights and what `transformers.T5EncoderModel` computes from it.

    python tools/make_t5_golden.py

Needs `transformers` (the tests do not).  Contents:
  config        vocab 512, d_model 128, d_kv 64, 2 heads, d_ff 256, 2 layers, gated-gelu, 32 buckets, max distance 128, eps 1e-6
  state_dict    the library's names, bf16 (non-trivial norm gains and relative-attention bias table)
  cases[name]   input_ids [B, S]; positions [n, 2] (batch row, token) at which outputs are kept; f64 [n, 128]: the library run in float64;
                bf16 [n, 128]: the library run in bfloat16 on the same weights (its own error against f64 is the yardstick of the GPU test)
                  s226  [2, 226]: a prompt ending in EOS then pads, and an all-pad row.  Only 51 of the 452 positions are kept: the file must stay under 1 MB and the
                        weights alone are 0.79 MB.  Kept: the prompt, its EOS and the first pads, then positions through the padded tail up to the last one (queries
                        whose distances to the prompt saturate in the last bucket), and four positions of the all-pad row.
                  s7    [2, 7], s1 [1, 1]: every position
  buckets       int16 [1023]: T5Attention._relative_position_bucket(d, bidirectional) for d = -511 .. 511
No mask is passed (none of the reference's call sites passes one)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = dict(vocab_size=512, d_model=128, d_kv=64, num_heads=2, d_ff=256, num_layers=2, feed_forward_proj="gated-gelu", relative_attention_num_buckets=32,
              relative_attention_max_distance=128, layer_norm_epsilon=1e-6)


def main():
    from transformers import T5Config, T5EncoderModel
    from transformers.models.t5.modeling_t5 import T5Attention
    g = torch.Generator().manual_seed(20)
    cfg = T5Config(**CONFIG, dropout_rate=0.0, is_encoder_decoder=False, use_cache=False, tie_word_embeddings=True)
    model = T5EncoderModel(cfg).eval()
    sd = {}
    for k, v in model.state_dict().items():
        r = torch.randn(v.shape, generator=g)
        if k.endswith("layer_norm.weight"):
            t = 1.0 + 0.25 * r
        elif "relative_attention_bias" in k:
            t = 1.5 * r
        elif "embed_tokens" in k or k == "shared.weight":
            t = sd.get("shared.weight", r)
        elif ".q." in k:
            t = r * (cfg.d_model * cfg.d_kv) ** -0.5 * 2.0          # scores of a few units: a softmax that is neither flat nor one-hot
        elif ".wo." in k:
            t = r * cfg.d_ff ** -0.5
        else:
            t = r * cfg.d_model ** -0.5
        sd[k] = t.to(torch.bfloat16)
    sd["encoder.embed_tokens.weight"] = sd["shared.weight"]

    ids226 = torch.zeros(2, 226, dtype=torch.long)
    ids226[0, :23] = torch.randint(2, 512, (23,), generator=g)
    ids226[0, 23] = 1
    ids7 = torch.randint(2, 512, (2, 7), generator=g)
    ids7[0, 6] = 1
    ids7[1, 4], ids7[1, 5:] = 1, 0
    ids1 = torch.tensor([[5]])
    keep0 = list(range(40)) + [100, 128, 129, 130, 200, 224, 225]
    pos226 = torch.tensor([[0, p] for p in keep0] + [[1, p] for p in (0, 1, 113, 225)])

    def every(ids):
        return torch.tensor([[b, s] for b in range(ids.shape[0]) for s in range(ids.shape[1])])

    cases = {"s226": dict(input_ids=ids226, positions=pos226), "s7": dict(input_ids=ids7, positions=every(ids7)), "s1": dict(input_ids=ids1, positions=every(ids1))}
    with torch.no_grad():
        for dtype, key in ((torch.float64, "f64"), (torch.bfloat16, "bf16")):
            m = T5EncoderModel(cfg).eval().to(dtype)
            m.load_state_dict({k: v.to(dtype) for k, v in sd.items()}, strict=True)
            for c in cases.values():
                out = m(input_ids=c["input_ids"])[0]
                assert out.dtype == dtype
                c[key] = out[c["positions"][:, 0], c["positions"][:, 1]].clone()
    d = torch.arange(-511, 512)
    buckets = T5Attention._relative_position_bucket(d, bidirectional=True, num_buckets=32, max_distance=128).to(torch.int16)
    import transformers
    out = dict(config=CONFIG, state_dict=sd, cases=cases, buckets=buckets, transformers_version=transformers.__version__)
    path = os.path.join(ROOT, "tests", "golden", "t5_tiny.pt")
    torch.save(out, path)
    size = os.path.getsize(path)
    for n, c in cases.items():
        e = ((c["bf16"].double() - c["f64"]).norm() / c["f64"].norm()).item()
        print(f"{n}: the library's bf16 run against its float64 run: rel-L2 {e:.3e}")
    print(f"wrote {path}: {size} bytes")
    assert size < 1000000, "the fixture must stay under 1 MB"


if __name__ == "__main__":
    sys.exit(main())
