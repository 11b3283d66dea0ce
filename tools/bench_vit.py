"""Frame consistency of one decoded clip at full width on the GPU: uint8 frames to score, the kernels of tokensgen_amd/vit.py against the bf16 `transformers` route,
in one process, alternating.

    python tools/bench_vit.py [--frames 49] [--out profiles/vit_bench.json]

Random weights (nothing to download).  Encoders: ViT-B/16 (`ViTModel` without pooler: "subject") and CLIP ViT-B/32 (`CLIPVisionModelWithProjection`: "background"),
12 layers of width 768.  Input: 49 frames of 480 x 720 uint8 on the device.  Routes, each from the uint8 frames to the 0-dim score:
  hip           metrics.video_consistency: prepare_video (bicubic antialiased cover + centre crop) -> ViTEncoder -> tg_feature_consistency;
  transformers  F.interpolate(bicubic, antialias) + centre crop + normalisation in torch on the device -> the library's model in bf16 on the same weights ->
                F.cosine_similarity in float64 -> the same score formula.
Both routes are warmed up twice, then timed five times in turn (device events around one call, a synchronise after each); the median and the five values are
recorded.  A separate, untimed pass with per-launch events gives the time per kernel and the GEMM's share of it.  The tool records what it measures; nothing is
asserted."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as Fn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
DEV = "cuda"
BF = torch.bfloat16


def random_state_dict(model, patch):
    g = torch.Generator(device=DEV).manual_seed(0)
    sd = {}
    for k, v in model.state_dict().items():
        r = torch.randn(v.shape, generator=g, device=DEV)
        if "norm" in k and k.endswith("weight"):
            r = 1.0 + 0.1 * r
        elif "norm" in k or k.endswith("bias"):
            r = 0.05 * r
        elif "cls_token" in k or "class_embedding" in k or "position_embedding" in k:
            r = 0.5 * r
        elif "patch_embedding" in k:
            r = r * (3 * patch * patch) ** -0.5
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


def library_route(kind, cfg, sd, mean, std):
    import transformers
    old = torch.get_default_dtype()
    torch.set_default_dtype(BF)
    try:
        with torch.device(DEV):
            if kind == "vit":
                hf = transformers.ViTModel(transformers.ViTConfig(**cfg), add_pooling_layer=False).eval()
            else:
                hf = transformers.CLIPVisionModelWithProjection(transformers.CLIPVisionConfig(**cfg)).eval()
    finally:
        torch.set_default_dtype(old)
    hf.load_state_dict(sd, strict=True)
    s = cfg["image_size"]
    m, d = torch.tensor(mean, device=DEV).view(1, 3, 1, 1), torch.tensor(std, device=DEV).view(1, 3, 1, 1)

    def run(u8):
        x = u8.permute(0, 3, 1, 2).float() / 255.0
        H, W = x.shape[2:]
        rh, rw = (s, int(W * s / H)) if W / H > 1 else (int(H * s / W), s)
        x = Fn.interpolate(x, size=(rh, rw), mode="bicubic", antialias=True, align_corners=False)
        top, left = (rh - s) // 2, (rw - s) // 2
        x = ((x[:, :, top:top + s, left:left + s] - m) / d).to(BF)
        out = hf(pixel_values=x)
        f = (out.last_hidden_state[:, 0] if kind == "vit" else out.image_embeds).double()
        prev = Fn.cosine_similarity(f[1:], f[:-1], dim=-1).clamp_min(0)
        first = Fn.cosine_similarity(f[1:], f[:1].expand_as(f[1:]), dim=-1).clamp_min(0)
        return ((prev + first) / 2).mean()
    return run, transformers.__version__


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=49)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vit_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_vit.py measures on the GPU; there is none here")
    import vit_ref as R
    from tokensgen_amd import kernels as K
    from tokensgen_amd.metrics import video_consistency
    from tokensgen_amd.vit import ViTEncoder
    g = torch.Generator().manual_seed(1)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, 480), torch.linspace(0, 1, 720), indexing="ij")
    u8 = torch.stack([(128 + 90 * torch.sin(6 * xx + 0.05 * f)[..., None] * torch.cos(4 * yy - 0.03 * f)[..., None] * torch.tensor([1.0, 0.7, 0.4])
                       + 12 * torch.randn(480, 720, 3, generator=g)).clamp(0, 255).to(torch.uint8) for f in range(a.frames)]).to(DEV)
    res = dict(device=torch.cuda.get_device_name(0), frames=list(u8.shape),
               method="device events around one call from uint8 frames to the score, 2 warm-up calls per route, then 5 rounds alternating the routes; median of 5; "
                      "per-launch times from a separate pass with an event pair around every launch", encoders={})
    base = dict(hidden_size=768, num_attention_heads=12, num_hidden_layers=12, intermediate_size=3072, image_size=224)
    with torch.no_grad():
        for name, kind, cfg in (("ViT-B/16", "vit", dict(base, patch_size=16, hidden_act="gelu", layer_norm_eps=1e-12)),
                                ("CLIP ViT-B/32", "clip", dict(base, patch_size=32, hidden_act="quick_gelu", layer_norm_eps=1e-5, projection_dim=512))):
            model = ViTEncoder(cfg, device=DEV, kind=kind)
            sd = random_state_dict(model, cfg["patch_size"])
            model.load_state_dict(sd, strict=True)
            routes = {"hip": lambda: video_consistency(u8, model)["score"]}
            try:
                run, version = library_route(kind, cfg, sd, *R.MEAN_STD[kind])
                routes["transformers"] = lambda: run(u8)
                note = f"transformers {version}, bf16, on the device"
            except Exception as ex:          # recorded, not hidden
                note = f"not measured: {type(ex).__name__}: {ex}"
            for fn in routes.values():
                fn(), fn()
            torch.cuda.synchronize()
            ms = {n: [] for n in routes}
            for _ in range(5):
                for n, fn in routes.items():
                    ms[n].append(timed(fn))
            entry = {n: dict(median_ms=statistics.median(v), runs_ms=v, score=float(routes[n]())) for n, v in ms.items()}
            K.PROFILE.clear()
            K.PROFILE_ON[0] = True
            routes["hip"]()
            K.PROFILE_ON[0] = False
            per = {n: dict(total_ms=round(v["total_ms"], 4), launches=v["n"]) for n, v in sorted(K.profile_summary().items())}
            total = sum(v["total_ms"] for v in per.values())
            gemm = sum(v["total_ms"] for n, v in per.items() if n.startswith("gemm_"))
            entry["hip"].update(per_kernel_ms=per, per_kernel_total_ms=round(total, 4), gemm_share=round(gemm / total, 4))
            S = model.tokens
            flop = a.frames * cfg["num_hidden_layers"] * (2 * S * 768 * (4 * 768 + 2 * 3072) + 4 * S * S * 768) + a.frames * 2 * (S - 1) * model.patch_kp * 768
            entry.update(transformers_route=note, tokens=S, tflop=round(flop / 1e12, 4), hip_tflops=round(flop / 1e9 / entry["hip"]["median_ms"], 1))
            res["encoders"][name] = entry
            print(f"{name}: " + ", ".join(f"{n} {entry[n]['median_ms']:.2f} ms" for n in routes) + f"; GEMM share of the launches {entry['hip']['gemm_share']:.2f}", flush=True)
            del model, routes
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
