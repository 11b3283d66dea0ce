"""The CLIP text tower at full width on the GPU against the bf16 `transformers` route, and what text alignment adds to a streaming consistency update; one
process, alternating.

    python tools/bench_clip_text.py [--frames 49] [--out profiles/clip_text_bench.json]

Random weights (nothing to download).  Text tower: the text_config of CLIP ViT-B/32 (12 layers of width 512, 8 heads, 77 positions, vocabulary 49408, projection
512), prompts padded to 77 tokens, B = 1 and B = 16.  Routes, each from int64 ids on the HOST to the fp32 features on the device:
  hip           clip_text.CLIPTextEncoder.encode_text (host validation and pooling positions, one copy of the ids, the kernels);
  transformers  ids.to(device) -> the library's CLIPTextModelWithProjection in bf16 on the same weights -> text_embeds.float().
Consistency update: metrics.VideoConsistency(background_model=CLIP ViT-B/32).update on 49 uint8 frames of 480 x 720 on the device, with K = 3 text features and
without: the same frames, the same trunk, one more launch (tg_text_alignment) with them.
Every route is warmed up twice, then timed five times in turn (device events around one call, a synchronise after each); the median and the five values are
recorded.  The tool records what it measures; nothing is asserted."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda"
BF = torch.bfloat16


def random_state_dict(model, patch=32):
    g = torch.Generator(device=DEV).manual_seed(0)
    sd = {}
    for k, v in model.state_dict().items():
        r = torch.randn(v.shape, generator=g, device=DEV)
        if "norm" in k and k.endswith("weight"):
            r = 1.0 + 0.1 * r
        elif "norm" in k or k.endswith("bias"):
            r = 0.05 * r
        elif "patch_embedding" in k:
            r = r * (3 * patch * patch) ** -0.5
        elif "embedding" in k:
            r = 0.5 * r
        else:
            r = r * v.shape[-1] ** -0.5
        sd[k] = r.to(BF)
    return sd


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def alternate(routes):
    for fn in routes.values():
        fn(), fn()
    torch.cuda.synchronize()
    ms = {n: [] for n in routes}
    for _ in range(5):
        for n, fn in routes.items():
            ms[n].append(timed(fn))
    return {n: dict(median_ms=statistics.median(v), runs_ms=v) for n, v in ms.items()}


def library_text_route(cfg, sd):
    import transformers
    old = torch.get_default_dtype()
    torch.set_default_dtype(BF)
    try:
        with torch.device(DEV):
            hf = transformers.CLIPTextModelWithProjection(transformers.CLIPTextConfig(**cfg)).eval()
    finally:
        torch.set_default_dtype(old)
    hf.load_state_dict(sd, strict=True)
    return (lambda ids: hf(input_ids=ids.to(DEV)).text_embeds.float()), transformers.__version__


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=49)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_text_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_clip_text.py measures on the GPU; there is none here")
    from tokensgen_amd.clip_text import CLIPTextEncoder
    from tokensgen_amd.metrics import VideoConsistency
    from tokensgen_amd.vit import ViTEncoder
    res = dict(device=torch.cuda.get_device_name(0),
               method="device events around one call, 2 warm-up calls per route, then 5 rounds alternating the routes; median of 5", text_tower={}, consistency_update={})
    with torch.no_grad():
        cfg = dict(vocab_size=49408, hidden_size=512, intermediate_size=2048, num_hidden_layers=12, num_attention_heads=8, max_position_embeddings=77,
                   projection_dim=512, hidden_act="quick_gelu", layer_norm_eps=1e-5, eos_token_id=2)
        model = CLIPTextEncoder(cfg, device=DEV)
        sd = random_state_dict(model)
        model.load_state_dict(sd, strict=True)
        try:
            run, version = library_text_route(cfg, sd)
            note = f"transformers {version}, bf16, on the device"
        except Exception as ex:              # recorded, not hidden
            run, note = None, f"not measured: {type(ex).__name__}: {ex}"
        g = torch.Generator().manual_seed(1)
        for B in (1, 16):
            ids = torch.randint(3, 49000, (B, 77), generator=g)
            ids[:, 0] = 49406
            for b in range(B):
                ids[b, 8 + 4 * b:] = 49407                                # BOS, 7 + 4 b words, EOS, EOS as padding
            routes = {"hip": lambda: model.encode_text(ids)}
            if run is not None:
                routes["transformers"] = lambda: run(ids)
            entry = alternate(routes)
            if run is not None:
                x, y = routes["hip"]().double(), routes["transformers"]().double()
                entry["rel_l2_between_the_routes"] = ((x - y).norm() / y.norm()).item()
                entry["hip_over_transformers"] = round(entry["hip"]["median_ms"] / entry["transformers"]["median_ms"], 3)
            entry.update(transformers_route=note, ids=list(ids.shape))
            res["text_tower"][f"B{B}"] = entry
            print(f"text tower B = {B}: " + ", ".join(f"{n} {entry[n]['median_ms']:.3f} ms" for n in routes), flush=True)
        text = model.encode_text(ids[:3])

        vcfg = dict(hidden_size=768, num_attention_heads=12, num_hidden_layers=12, intermediate_size=3072, image_size=224, patch_size=32, hidden_act="quick_gelu",
                    layer_norm_eps=1e-5, projection_dim=512)
        image = ViTEncoder(vcfg, device=DEV, kind="clip")
        image.load_state_dict(random_state_dict(image), strict=True)
        yy, xx = torch.meshgrid(torch.linspace(0, 1, 480), torch.linspace(0, 1, 720), indexing="ij")
        u8 = torch.stack([(128 + 90 * torch.sin(6 * xx + 0.05 * f)[..., None] * torch.cos(4 * yy - 0.03 * f)[..., None] * torch.tensor([1.0, 0.7, 0.4])
                           + 12 * torch.randn(480, 720, 3, generator=g)).clamp(0, 255).to(torch.uint8) for f in range(a.frames)]).to(DEV)
        routes = {"without_text": lambda: VideoConsistency(background_model=image).update(u8),
                  "with_text": lambda: VideoConsistency(background_model=image, text_features=text).update(u8)}
        entry = alternate(routes)
        entry.update(frames=list(u8.shape), texts=int(text.shape[0]),
                     with_over_without=round(entry["with_text"]["median_ms"] / entry["without_text"]["median_ms"], 4))
        res["consistency_update"] = entry
        print("VideoConsistency.update: " + ", ".join(f"{n} {entry[n]['median_ms']:.3f} ms" for n in routes), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
