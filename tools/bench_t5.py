"""T5-v1.1-XXL encoder at full width on the GPU: the kernels of tokensgen_amd/t5.py against the torch route, in one process, alternating.

    python tools/bench_t5.py [--layers 24] [--out profiles/t5_bench.json]

Random weights (nothing to download), input_ids [1 | 2 | 3, 226].  Per batch size: both routes are warmed up, then timed five times in turn (device events around one
forward, a synchronise after each); the median and the five values are recorded.  Routes: `hip` (T5EncoderModel of this repository), `torch_bf16` (the library's
arithmetic with F.linear / matmul / softmax on bf16 tensors, tests/t5_ref.py) and `transformers` (T5EncoderModel of the library on the same weights) when it can be
imported.  A separate, untimed forward with per-launch events gives the time per kernel; memory is torch's allocator peak during one forward of each route above what was
resident before it (weights excluded: 9.4 GB per model at 24 layers, recorded as resident_weights_gb).  The floor quoted for orientation is the time to read the weights once at 8 TB/s."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CFG = dict(vocab_size=32128, d_model=4096, d_kv=64, num_heads=64, d_ff=10240, num_layers=24, feed_forward_proj="gated-gelu", relative_attention_num_buckets=32,
           relative_attention_max_distance=128, layer_norm_epsilon=1e-6)
DEV = "cuda"


def random_weights(model):
    g = torch.Generator(device=DEV).manual_seed(0)
    c = model.config
    with torch.no_grad():
        for k, v in model.state_dict().items():
            if k == "encoder.embed_tokens.weight":
                continue
            r = torch.randn(v.shape, generator=g, device=DEV)
            if k.endswith("layer_norm.weight"):
                r = 1.0 + 0.1 * r
            elif ".q." in k:
                r = r * (c.d_model * c.d_kv) ** -0.5
            elif ".wo." in k:
                r = r * c.d_ff ** -0.5
            elif v.dim() == 2 and "shared" not in k and "relative_attention_bias" not in k:
                r = r * c.d_model ** -0.5
            v.copy_(r)
    model._bias = {}


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def forward_peak_gb(fn):
    """allocator peak DURING one forward minus what was resident before it (the weights of every route stay resident in this process)"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - before) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "t5_bench.json"))
    ap.add_argument("--no-transformers", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_t5.py measures on the GPU; there is none here")
    import t5_ref as R
    from tokensgen_amd import kernels as K
    from tokensgen_amd.t5 import T5EncoderModel
    cfg = dict(CFG, num_layers=a.layers)
    model = T5EncoderModel(cfg, device=DEV)
    random_weights(model)
    sd = model.state_dict()
    weight_bytes = sum(t.numel() * 2 for n, t in model._w.items() if n != "emb")
    routes = {"hip": lambda ids: model(ids)[0], "torch_bf16": lambda ids: R.t5_forward_torch_bf16(sd, cfg, ids, device=DEV)}
    hf_note = None
    if not a.no_transformers:
        try:
            import transformers
            hf_cfg = transformers.T5Config(**cfg, dropout_rate=0.0, is_encoder_decoder=False, use_cache=False)
            old = torch.get_default_dtype()
            torch.set_default_dtype(torch.bfloat16)
            try:
                with torch.device(DEV):
                    hf = transformers.T5EncoderModel(hf_cfg).eval()
            finally:
                torch.set_default_dtype(old)
            hf.load_state_dict(sd, strict=True)
            routes["transformers"] = lambda ids: hf(input_ids=ids)[0]
            hf_note = f"transformers {transformers.__version__}"
        except Exception as ex:          # recorded, not hidden: the two other routes are still measured
            hf_note = f"not measured: {type(ex).__name__}: {ex}"
    res = dict(device=torch.cuda.get_device_name(0), config=cfg, weight_gb_read_per_forward=weight_bytes / 1e9, floor_ms_at_8TBps=weight_bytes / 8e12 * 1e3,
               transformers=hf_note, resident_weights_gb=sum(t.numel() * 2 for t in model._w.values()) / 1e9, method="device events around one forward, 2 warm-up calls per route, then 5 rounds alternating the routes; median of 5", batches={})
    with torch.no_grad():
        for B in (1, 2, 3):
            ids = torch.randint(2, cfg["vocab_size"], (B, 226), generator=torch.Generator().manual_seed(B)).to(DEV)
            ids[:, 40:] = 0
            for fn in routes.values():
                fn(ids), fn(ids)
            torch.cuda.synchronize()
            ms = {n: [] for n in routes}
            for _ in range(5):
                for n, fn in routes.items():
                    ms[n].append(timed(lambda: fn(ids)))
            entry = {n: dict(median_ms=statistics.median(v), runs_ms=v, forward_peak_memory_gb=forward_peak_gb(lambda: routes[n](ids))) for n, v in ms.items()}
            ref = routes["torch_bf16"](ids).float()
            entry["hip"]["rel_l2_vs_torch_bf16"] = ((routes["hip"](ids).float() - ref).norm() / ref.norm()).item()
            K.PROFILE.clear()
            K.PROFILE_ON[0] = True
            routes["hip"](ids)
            K.PROFILE_ON[0] = False
            entry["hip"]["per_kernel_ms"] = {n: dict(total_ms=round(v["total_ms"], 4), launches=v["n"]) for n, v in sorted(K.profile_summary().items())}
            res["batches"][f"{B}x226"] = entry
            print(f"[{B}, 226]: " + ", ".join(f"{n} {entry[n]['median_ms']:.2f} ms" for n in routes), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
