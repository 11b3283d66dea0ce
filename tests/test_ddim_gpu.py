"""GPU: the DDIM sampler on the HIP path.  The update runs in the fused guidance + solver kernel through the coefficient row of
`ddim_coef_row`; the reference is tests/ddim_ref.py (bitwise the reference class's `step`, tests/test_ddim_cpu.py) and runs of the
reference's own pipelines under its DDIM scheduler stored in tests/golden/*ddim*.pt.

Per-element bounds of the f32-arithmetic variants (`mag` = sum of the absolute values of the terms):
    fp32 x0:      |err| <= 12 * 2^-23 * mag      twelve fp32 operations on the longest path (six for 3-way guidance, two for x0, two for the
                                                 update, and a factor 2 as in edge_bounds.gemm_bias_bound)
    bf16 output:  |err| <= 2^-8 |ref| + 12 * 2^-23 * mag
The static bf16-state variant is the kernel's bf16-chained path: the reference rounds every op to bf16, the kernel once per output — rel-L2
9e-3, the bound and the reason of tests/test_kernels_gpu.py::test_cfg_dpm_step_ex_variants_match_oracle."""
import os

import numpy as np
import pytest
import torch

from ddim_ref import ddim_ref, terms_magnitude
from oracle import dit_ref as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
KW = dict(prediction_type="v_prediction", rescale_betas_zero_snr=True, snr_shift_scale=1.0, timestep_spacing="trailing")
ROWS = [(999, 979, True), (979, 959, True), (499, 479, True), (19, -1, True), (19, -1, False)]      # (t, prev_t, set_alpha_to_one)
U23, STATIC_TOL = 12 * 2.0 ** -23, 9e-3
G, GI = 6.0, 4.0


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _ratio(out, ref, mag, bf16_out):
    """worst |err| / bound over the elements (<= 1 passes)"""
    ref = ref.double()
    bound = U23 * mag + (2.0 ** -8 * ref.abs() if bf16_out else 0.0)
    return ((out.double().cpu() - ref).abs() / bound.clamp_min(1e-300)).max().item()


@pytest.fixture(scope="module")
def tables():
    from tokensgen_amd.scheduler import CogVideoXDDIMScheduler
    out = {}
    for one in (True, False):
        s = CogVideoXDDIMScheduler(set_alpha_to_one=one, **KW)
        out[one] = (s.alphas_cumprod, s.final_alpha_cumprod)
    return out


def _guided(mo, branches, gpf, f32):
    """The guided prediction [F, E] with torch's promotion, and the sum of |terms|.  f32 without gpf: the pipelines' `.float()` first, Python
    float weights; gpf [F, 2] fp32: the worker's guidance tensor on bf16 branches; neither: Python floats on bf16 tensors, every op bf16."""
    m = mo.float() if (f32 and gpf is None) else mo
    g, gi = (G, GI) if gpf is None else (gpf[:, :1], gpf[:, 1:])
    a = m.double().abs()
    gd, gid = (G, GI) if gpf is None else (gpf[:, :1].double(), gpf[:, 1:].double())
    if branches == 1:                                   # no guidance: the weights are unused, an fp32 solver sees the `.float()` of the output
        return (m[0].float() if f32 else m[0]), a[0]
    if branches == 2:
        return m[0] + g * (m[1] - m[0]), a[0] + abs(gd) * (a[1] + a[0])
    return (m[2] + (g - 1) * (m[2] - m[0]) + (gi - 1) * (m[2] - m[1]),
            a[2] + abs(gd - 1) * (a[2] + a[0]) + abs(gid - 1) * (a[2] + a[1]))


@pytest.mark.parametrize("f32_state", [True, False], ids=["f32state", "bf16state"])
@pytest.mark.parametrize("pred", ["v_prediction", "epsilon", "sample"])
@pytest.mark.parametrize("per_frame", [False, True], ids=["static", "perframe"])
@pytest.mark.parametrize("branches", [1, 2, 3])
def test_ddim_rows_through_the_fused_kernel(tables, parity, branches, per_frame, pred, f32_state):
    """Five coefficient rows, one per frame, through tg_cfg_dpm_step_ex against ddim_ref per frame.  Epsilon prediction divides by
    sqrt(alphas_cumprod[999]) = 0 in the reference too: its first row is (959, 939) instead of (999, 979)."""
    from tokensgen_amd import kernels as K
    from tokensgen_amd.scheduler import ddim_coef_row
    rows = list(ROWS)
    if pred == "epsilon":
        rows[0] = (959, 939, True)
    frames, E = len(rows), 16 * 4 * 6
    gen = torch.Generator().manual_seed(21)
    mo = torch.randn(branches, frames, E, generator=gen).to(BF)
    x = torch.randn(frames, E, generator=gen).to(BF)
    coef = torch.tensor([ddim_coef_row(tables[one][0].numpy(), t, p, float(tables[one][1])) for (t, p, one) in rows], dtype=torch.float32, device=DEV)
    gpf = None
    if per_frame:
        tv = torch.tensor([r[0] for r in rows])
        ramp = (1 - torch.cos(np.pi * ((52 - tv) / 52) ** 5.0)) / 2                  # an fp32 tensor over the frames, as the worker builds
        gpf = torch.stack([1 + G * ramp, 1 + GI * ramp], dim=1).to(torch.float32).contiguous()
    f32_math = f32_state or per_frame
    sdt = torch.float32 if f32_state else BF

    def run(old):
        xo, x0o = torch.empty(frames, E, dtype=BF, device=DEV), torch.empty(frames, E, dtype=sdt, device=DEV)
        K.cfg_dpm_step_ex(mo.to(DEV), x.to(DEV), old, torch.zeros(frames, 2, E, dtype=BF, device=DEV), coef, G, xo, x0o, guidance_img=GI,
                          guidance_per_frame=None if gpf is None else gpf.to(DEV), f32_math=f32_math, prediction_type=pred)
        return xo.cpu(), x0o.cpu()
    xo, x0o = run(torch.zeros(frames, E, dtype=sdt, device=DEV))
    # mn = 0 on a zero noise buffer, has_old = 0: the outputs do not depend on what old_x0 holds
    xo2, x0o2 = run(torch.full((frames, E), float("nan"), dtype=sdt, device=DEV))
    assert torch.equal(xo, xo2) and torch.equal(x0o, x0o2)
    assert x0o.dtype == sdt and torch.isfinite(xo.float()).all() and torch.isfinite(x0o.float()).all()

    v, vmag = _guided(mo, branches, gpf, f32_math)
    assert v.dtype == (torch.float32 if f32_math else BF)
    worst = dict(prev=0.0, x0=0.0)
    for f, (t, p, one) in enumerate(rows):
        prev, x0 = ddim_ref(v[f], t, p, x[f], tables[one], pred)
        assert prev.dtype == x0.dtype == v.dtype or pred == "sample"
        if f32_math:
            m0, mp = terms_magnitude(vmag[f], t, p, x[f], tables[one], pred)
            worst["x0"] = max(worst["x0"], _ratio(x0o[f], x0, m0, bf16_out=not f32_state))
            worst["prev"] = max(worst["prev"], _ratio(xo[f], prev, mp, bf16_out=True))
        else:
            worst["x0"] = max(worst["x0"], _rel(x0o[f], x0) / STATIC_TOL)
            worst["prev"] = max(worst["prev"], _rel(xo[f], prev) / STATIC_TOL)
    kind = "|err|/bound" if f32_math else "rel-L2/9e-3"
    for k, w in worst.items():
        print(f"ddim rows br={branches} per_frame={per_frame} {pred} f32_state={f32_state}: worst {kind} {k} = {w:.4f}")
    parity(worst["x0"], 1.0 + 1e-12, f"worst {kind}, x0")
    parity(worst["prev"], 1.0 + 1e-12, f"worst {kind}, prev_sample")


def test_fused_step_and_window_step_are_that_launch(tables):
    """scheduler.fused_step / window_step build the same rows and launch: bitwise the direct kernel call; window_step takes non-tensors
    for the arguments it ignores."""
    from tokensgen_amd import kernels as K
    from tokensgen_amd.scheduler import CogVideoXDDIMScheduler
    s = CogVideoXDDIMScheduler(**KW)
    s.set_timesteps(50)
    gen = torch.Generator().manual_seed(22)
    F_, shp = 4, (16, 4, 6)
    mo, x = torch.randn(2, F_, *shp, generator=gen).to(BF).to(DEV), torch.randn(F_, *shp, generator=gen).to(BF).to(DEV)
    t, p = [999, 979, 499, 19], [979, 959, 479, -1]
    coef = s.coef_table(t, p, DEV)
    for f32_state in (False, True):
        xo, x0o = torch.empty_like(x), torch.empty(x.shape, dtype=torch.float32 if f32_state else BF, device=DEV)
        K.cfg_dpm_step_ex(mo.reshape(2, F_, -1), x.reshape(F_, -1), torch.zeros_like(x0o).reshape(F_, -1), torch.zeros(F_, 2, x[0].numel(), dtype=BF, device=DEV),
                          coef, G, xo.view(F_, -1), x0o.view(F_, -1), f32_math=f32_state)
        if f32_state:
            a, b = s.fused_step(mo, x, t, p, G, f32_math=True, f32_state=True)
        else:
            a, b = s.window_step(mo, x, None, None, t, p, [None] * F_, "ignored", G)
        assert torch.equal(a, xo) and torch.equal(b, x0o) and b.dtype == x0o.dtype
    assert len(s._zeros) == 3 and all(float(z.abs().max()) == 0 for z in s._zeros.values())      # allocated once per shape, never written
    s.window_step(mo, x, None, None, t, p, None, None, G)
    assert len(s._zeros) == 3


def test_step_vs_reference_step_outputs(golden_dir, tables, parity):
    """`step` against the reference class's recorded outputs: an fp32 model output with a bf16 sample (x0 fp32, per-element bounds) and all
    bf16 (x0 bf16, the bf16-chained bound); prev_sample comes back in the sample's dtype."""
    from tokensgen_amd.scheduler import CogVideoXDDIMScheduler, DDIMSchedulerOutput
    g = torch.load(os.path.join(golden_dir, "scheduler_ddim.pt"), weights_only=False)
    worst = dict(f32_x0=0.0, f32_prev=0.0, bf16_x0=0.0, bf16_prev=0.0)
    n = 0
    for c in g["steps"]:
        if c["dtypes"] == "f64":
            continue
        i = g["inputs"][c["row"]]
        s = CogVideoXDDIMScheduler(set_alpha_to_one=c["set_alpha_to_one"], **dict(KW, prediction_type=c["prediction_type"]))
        s.set_timesteps(50)
        f32 = c["dtypes"] == "f32_bf16"
        mo = i["model_output"].bfloat16().float() if f32 else i["model_output"].bfloat16()
        x = i["sample"].bfloat16()
        prev, x0 = s.step(mo.to(DEV), torch.tensor(c["t"]), torch.tensor(c["prev_t"]), x.to(DEV), eta=0.3, generator=object(), return_dict=False)
        assert prev.dtype == BF and x0.dtype == (torch.float32 if f32 else BF) and prev.shape == x0.shape == x.shape
        if f32:
            m0, mp = terms_magnitude(mo, c["t"], c["prev_t"], x, tables[c["set_alpha_to_one"]], c["prediction_type"])
            worst["f32_x0"] = max(worst["f32_x0"], _ratio(x0, c["x0"], m0, bf16_out=False))
            worst["f32_prev"] = max(worst["f32_prev"], _ratio(prev, c["prev_sample"], mp, bf16_out=True))
        else:
            worst["bf16_x0"] = max(worst["bf16_x0"], _rel(x0, c["x0"]) / STATIC_TOL)
            worst["bf16_prev"] = max(worst["bf16_prev"], _rel(prev, c["prev_sample"]) / STATIC_TOL)
        n += 1
    assert n == 28
    out = s.step(mo.to(DEV), c["t"], c["prev_t"], x.to(DEV))
    assert isinstance(out, DDIMSchedulerOutput) and torch.equal(out.prev_sample, prev) and torch.equal(out.pred_original_sample, x0)
    for k, w in worst.items():
        print(f"ddim step vs reference: worst {k} ratio = {w:.4f}")
        parity(w, 1.0 + 1e-12, f"step vs reference class, worst {'|err|/bound' if k.startswith('f32') else 'rel-L2/9e-3'}: {k}")


def _to2v_model(golden_dir, seed):
    from tokensgen_amd.transformer import CogVideoXTransformer3DModel
    gt = torch.load(os.path.join(golden_dir, "dit_tiny.pt"), weights_only=False)
    cfg, vipcfg = gt["cfg"], gt["vip"]
    m = CogVideoXTransformer3DModel(num_attention_heads=2, attention_head_dim=64, num_layers=2, time_embed_dim=cfg["time_embed_dim"],
                                    text_embed_dim=cfg["text_embed_dim"], use_rotary_positional_embeddings=True, device=DEV)
    m.set_vip_layers(None, **vipcfg)
    m.load_state_dict({k: v.to(BF) for k, v in O.make_state_dict(cfg, 128, seed=seed).items()}, strict=True)
    return m


def _never(*a, **k):
    raise AssertionError("the DDIM path must not ask for step noise")


def test_base_stage_vs_reference_pipeline_under_ddim(golden_dir, parity):
    """The base stage under CogVideoXDDIMScheduler against the reference's own pipeline run under its DDIM scheduler
    (tests/golden/base_stage_ddim_tiny.pt, bf16 case, 50 trailing steps, static guidance 6.0): rel-L2 2e-2, the bound of the DPM run of the
    same model in tests/test_fifo_gpu.py (no noise here, so nothing looser is justified).  No step noise is requested and the generator
    only serves the initial latents."""
    from tokensgen_amd.pipeline import MPFIFOVideoIPAdapterCogVideoXPipeline
    from tokensgen_amd.scheduler import CogVideoXDDIMScheduler, CogVideoXDPMScheduler
    g = torch.load(os.path.join(golden_dir, "base_stage_ddim_tiny.pt"), weights_only=False)
    c = g["cases"]["torch.bfloat16"]
    H, W, T, nf = g["H"], g["W"], g["steps"], 13
    assert T == 50 and g["scheduler"] == "CogVideoXDDIMScheduler"
    m = _to2v_model(golden_dir, g["weight_seed"])
    pipe = MPFIFOVideoIPAdapterCogVideoXPipeline(m, CogVideoXDPMScheduler(**KW), resampler_config=dict(num_temporal_queries=4, num_height_queries=2, num_width_queries=3))
    pipe.scheduler = CogVideoXDDIMScheduler.from_config(pipe.scheduler.config, timestep_spacing="trailing")      # the reference's way
    out = pipe(prompt_embeds=c["prompt"], negative_prompt_embeds=c["negative"], image_embeddings=c["emb_in"], height=H * 8, width=W * 8,
               num_chunks=g["chunks"], num_inference_steps=T, latents=c["init_latents"], video_ipadapter_scale=g["vip_scale"], step_noise=_never)
    assert [int(t) for t in out.timesteps] == [int(t) for t in g["timesteps"]] == list(range(999, 0, -20))
    assert [o is None for o in out.fifo_old_pred_original_sample] == [o is None for o in c["fifo_old"]]
    assert out.fifo_old_pred_original_sample[-1] is None and out.fifo_old_pred_original_sample[0] is not None
    assert torch.equal(out.image_embeddings.cpu(), c["image_embeddings"]) and out.fifo_latents.shape == c["fifo_latents"].shape
    parity(_rel(out.fifo_latents, c["fifo_latents"]), 2e-2, "DDIM base stage FIFO seed latents vs reference pipeline run (bf16, 50 steps)")
    parity(_rel(out.orig_latents, c["orig_latents"]), 2e-2, "DDIM base stage final latents vs reference pipeline run")
    x0 = torch.cat([o for o in out.fifo_old_pred_original_sample if o is not None], dim=1)
    x0r = torch.cat([o for o in c["fifo_old"] if o is not None], dim=1)
    parity(_rel(x0, x0r), 2e-2, "DDIM base stage x0 seed list vs reference pipeline run")
    # the generator serves the initial latents and nothing else
    gen, alone = torch.Generator(device=DEV).manual_seed(5), torch.Generator(device=DEV).manual_seed(5)
    a = pipe(prompt_embeds=c["prompt"], negative_prompt_embeds=c["negative"], image_embeddings=c["emb_in"], height=H * 8, width=W * 8,
             num_chunks=g["chunks"], num_inference_steps=3, generator=gen, step_noise=_never)
    first = torch.randn((1, nf, 16, H, W), generator=alone, device=DEV, dtype=torch.float32).to(BF)
    assert torch.equal(gen.get_state(), alone.get_state()) and torch.equal(a.fifo_latents[:, [-1]], first[:, [nf - 1]])


def test_t2to_stage_vs_reference_pipeline_under_ddim(golden_dir, parity, monkeypatch):
    """The T2To stage under DDIM against the reference pipeline run under its DDIM scheduler (tests/golden/t2to_ddim_tiny.pt, bf16 case,
    6 steps, dynamic CFG): the sampled latents and the condensed tokens, rel-L2 1.2e-2 — the bound tests/test_t2to_gpu.py uses for the DPM
    run of the same model and step count (there on the tokens; the tail that makes tokens of latents is linear, and DDIM adds no noise)."""
    from tokensgen_amd import pipeline_t2to as P
    from tokensgen_amd.pca import PCA
    from tokensgen_amd.scheduler import CogVideoXDDIMScheduler
    from tokensgen_amd.transformer import CogVideoXTransformer3DModel
    g = torch.load(os.path.join(golden_dir, "t2to_ddim_tiny.pt"), weights_only=False)
    c, cfg = g["cases"]["torch.bfloat16"], g["cfg"]
    m = CogVideoXTransformer3DModel(num_attention_heads=cfg["num_attention_heads"], attention_head_dim=64, num_layers=cfg["num_layers"],
                                    time_embed_dim=cfg["time_embed_dim"], text_embed_dim=cfg["text_embed_dim"], patch_size=1,
                                    use_rotary_positional_embeddings=True, device=DEV)
    m.load_state_dict({k: v.to(BF) for k, v in O.make_state_dict(cfg, seed=g["weight_seed"]).items()}, strict=True)
    pipe = P.LongVGenCogVideoXPipeline(m, CogVideoXDDIMScheduler(**KW))
    pca = PCA()
    pca.register_buffer("mean_", g["pca_mean"]); pca.register_buffer("components_", g["pca_components16"])
    sampled = []
    real = P.K.pca_inverse
    monkeypatch.setattr(P.K, "pca_inverse", lambda lat, *a: (sampled.append(lat.clone()), real(lat, *a))[1])
    gen = torch.Generator().manual_seed(3)
    before = gen.get_state()
    out = pipe(prompt_embeds=c["prompt"], negative_prompt_embeds=c["negative"], height=g["H"], width=g["W"], num_frames_per_chunk=g["nfc"],
               num_chunks=g["chunks"], num_inference_steps=g["steps"], use_dynamic_cfg=True, guidance_scale=g["guidance_scale"],
               latents=c["init_latents"], generator=gen, longvgen_mean=g["mean"], longvgen_std=g["std"], longvgen_pca=pca, step_noise=_never).frames
    assert torch.equal(gen.get_state(), before)
    assert [int(t) for t in pipe.scheduler.timesteps] == [int(t) for t in c["timesteps"]]
    assert out.shape == c["frames"].shape and out.dtype == BF and len(sampled) == 1
    parity(_rel(sampled[0][None], c["sampled"]), 1.2e-2, "DDIM T2To sampled latents vs reference pipeline run (bf16, 6 steps, dynamic CFG)")
    parity(_rel(out, c["frames"]), 1.2e-2, "DDIM T2To condensed tokens vs reference pipeline run")


def test_fifo_under_ddim_is_deterministic_and_keeps_the_window_schedule(golden_dir, parity, tables):
    """The FIFO driver under DDIM (beyond the reference, whose worker asserts the DPM class): tiny DiT, 2 clips, 13 steps on one partition.
    Different step-noise seeds with the same tail-noise seed give bitwise the same video; the index trace is the DPM run's; one window's
    output is ddim_ref applied frame by frame to that window's own model output (static guidance: the bf16-chained bound)."""
    from tokensgen_amd import fifo
    from tokensgen_amd.pipeline import MPFIFOVideoIPAdapterCogVideoXPipeline
    from tokensgen_amd.scheduler import CogVideoXDDIMScheduler, CogVideoXDPMScheduler
    m = _to2v_model(golden_dir, 400)
    chunks, H, W, T, nf = 2, 4, 6, 13, 13
    gen = torch.Generator().manual_seed(41)
    prompt, negative = torch.randn(1, 8, 64, generator=gen).to(BF), torch.randn(1, 8, 64, generator=gen).to(BF)
    tokens = torch.randn(1, 4 * chunks, 128, 2, 3, generator=gen).to(BF)
    lat0 = torch.randn(1, nf, 16, H, W, generator=gen).to(BF)
    tail = lambda i, shape: torch.randn(shape, generator=torch.Generator().manual_seed(500 + i)).to(BF).to(DEV)

    def run(sched, seed):
        pipe = MPFIFOVideoIPAdapterCogVideoXPipeline(m, sched, resampler_config=dict(num_temporal_queries=4, num_height_queries=2, num_width_queries=3))
        base = pipe(prompt_embeds=prompt, negative_prompt_embeds=negative, image_embeddings=tokens, height=H * 8, width=W * 8, num_chunks=chunks,
                    num_inference_steps=T, latents=lat0, generator=torch.Generator(device=DEV).manual_seed(seed),
                    sampling_params=dict(use_adaptive_padding=True, num_partitions=1))
        trace = []
        video = fifo.cogvideo_fifo_mp_v2([pipe], base, noise_seed=seed, tail_noise_fn=tail, trace=trace)[1]
        assert video.shape == (1, chunks * nf, 16, H, W) and torch.isfinite(video).all()
        return pipe, base, video.cpu(), trace
    pipe, base, v1, tr1 = run(CogVideoXDDIMScheduler(**KW), 7)
    _, _, v2, tr2 = run(CogVideoXDDIMScheduler(**KW), 8)
    _, _, v3, tr3 = run(CogVideoXDPMScheduler(**KW), 7)
    assert torch.equal(v1, v2) and tr1 == tr2
    assert tr1 == tr3 and len(tr1) > 0 and not torch.equal(v1, v3)
    # a step-noise callable handed to the driver is not called either
    assert torch.equal(fifo.cogvideo_fifo_mp_v2([pipe], base, step_noise_fn=_never, tail_noise_fn=tail)[1].cpu(), v1)

    # one window: frames at mixed noise levels, the last ones on their final step (prev_t = -1)
    ts = pipe.scheduler.timesteps.tolist()
    t = ts[::-1]
    prev_t = [-1] + t[:-1]
    g_t, g_h, g_w = base.vip_image_rotary_grid
    c_t, c_h, c_w = base.vip_condition_rotary_grid
    worker = fifo.FifoWorker(m, pipe.scheduler, base.prompt_embeds, base.image_rotary_emb, 6.0, g_h, g_w, c_h, c_w, num_inference_steps=T)
    lat = torch.randn(1, nf, 16, H, W, generator=gen).to(BF).to(DEV)
    kw = dict(latents=lat, t=np.asarray(t), grid_t=np.asarray(g_t[:nf], dtype=np.float32), cond_grid_t=np.asarray(c_t[:5], dtype=np.float32),
              image_embeddings=base.image_embeddings[:, :5].contiguous())
    pred = worker.predict(None, **kw)
    x_out, x0_out = worker.finish(pred, lat, old_x0=torch.full((nf, 16, H, W), float("nan"), dtype=BF, device=DEV), has_old=[False] * nf, t=t,
                                  prev_t=prev_t, next_t=[-1] * nf, noise=None)
    pc = pred.cpu()
    v = pc[0] + 6.0 * (pc[1] - pc[0])                                           # Python-float guidance on bf16 tensors
    ref = [ddim_ref(v[f], t[f], prev_t[f], lat[0, f].cpu(), tables[True], "v_prediction") for f in range(nf)]
    parity(_rel(x_out[0], torch.stack([r[0] for r in ref])), STATIC_TOL, "FIFO window under DDIM vs ddim_ref per frame, prev_sample")
    parity(_rel(x0_out, torch.stack([r[1] for r in ref])), STATIC_TOL, "FIFO window under DDIM vs ddim_ref per frame, x0")
