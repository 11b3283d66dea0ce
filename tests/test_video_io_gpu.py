"""GPU: tokensgen_amd.video_io on the HIP path.  tg_video_resample against the fp64 restatement of tests/video_ref.py, EVERY element by a derived bound (the style of
tests/edge_bounds.py); tg_video_to_uint8 exactly, on all 65 536 bf16 bit patterns; VideoProcessor through the FIFO driver's hook; and `pipe(frames=...)` bitwise
against `pipe(image_embeddings=pipe.vae_encode_image(...))`.

The resample bound, for out = bf16(2 acc - 1), acc = sum_y wy sum_x wx (u8 / 255) in fp32:
    bound = 2^-8 |ref| + (taps_y + taps_x + 8) 2^-23 A,   A = sum_y |wy| sum_x |wx| (u8 / 255) in fp64
The first term is the bf16 rounding of the result (unit roundoff 2^-8).  The second is the fp32 work: each of the taps_x + taps_y fused multiply-adds on the way to an
output, the fp32 rounding of the two weights and the fp32 division each cost at most 2^-24 of the magnitude sum A, and the `2 acc - 1` map doubles it.  No measured
figure enters."""
import os

import numpy as np
import pytest
import torch

import edge_bounds as E
import video_ref as VR

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


def _frames(F, H, W, seed, checker=False):
    if checker:
        yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        plane = (((yy + xx) % 2) * 255).to(torch.uint8)
        return torch.stack([torch.stack([plane if (f + c) % 2 == 0 else 255 - plane for c in range(3)], dim=-1) for f in range(F)])
    return torch.randint(0, 256, (F, H, W, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


CASES = {          # name: (F, H, W, output_res, crop_to_fit, pad_to_fit, checkerboard)
    "wide_source_crop_left": (3, 45, 100, (32, 48), True, False, False),
    "tall_source_crop_top": (3, 100, 45, (32, 48), True, False, False),
    "upscale_checkerboard": (3, 20, 30, (32, 48), True, False, True),
    "ten_taps": (3, 90, 160, (40, 64), True, False, False),
    "downscale_4p5": (3, 216, 324, (48, 72), True, False, False),
    "unaligned_rows_231_bytes": (3, 203, 77, (24, 40), True, False, False),
    "several_tiles": (3, 270, 484, (120, 184), True, False, False),
    "bilinear_no_flag": (3, 50, 70, (32, 48), False, False, False),
    "pad_to_fit": (3, 60, 60, (32, 48), False, True, False),
    "one_frame": (1, 45, 100, (32, 48), True, False, False),
    "five_frames": (5, 45, 100, (32, 48), True, False, False),
}


@pytest.mark.parametrize("name", list(CASES))
def test_prepare_video_every_element_within_the_derived_bound(name, parity):
    from tokensgen_amd.video_io import prepare_video, resample_plan
    F, H, W, res, crop, pad, checker = CASES[name]
    frames = _frames(F, H, W, seed=len(name), checker=checker)
    got = prepare_video(frames, res, crop_to_fit=crop, pad_to_fit=pad, device=DEV)
    assert got.shape == (1, F, 3) + res and got.dtype == BF and got.is_cuda
    ref, A, (ty, tx) = VR.prepare_ref(frames, res, crop, pad)
    bound = 2.0 ** -8 * ref.abs() + (ty + tx + 8) * 2.0 ** -23 * A
    worst, where = E.check(got, ref, bound)
    print(name, "taps", (ty, tx), "worst ratio", worst, "at", where)
    parity(worst, 1.0, f"prepare_video {name}: worst |out - fp64| / derived bound")
    plan = resample_plan((H, W), res, crop, pad)
    assert plan.taps == (ty, tx)
    if name == "ten_taps":
        assert 10 in (ty, tx)
    if name == "downscale_4p5":
        assert 18 <= max(ty, tx) <= 22
    if name == "upscale_checkerboard":
        assert (got.float().abs() > 1).any(), "bicubic overshoot past +-1 is the reference's behaviour: no clamp"
    if name == "pad_to_fit":
        assert plan.pad_x == 15 and plan.tables[3][0] < 0                        # the outermost columns draw on the pad: column 0 on nothing else ...
        assert (got[..., 0] == -1).all() and (got[..., -1] == -1).all() and (ref[..., 0] == -1).all()
        assert (plan.tables[3][8] < 0 <= plan.tables[3][8] + plan.tables[4][8] - 1) and (ref[..., 8] > -1).all()      # ... column 8 on both sides of the edge


def test_prepare_video_identity_is_exact():
    from tokensgen_amd.video_io import prepare_video
    frames = _frames(2, 32, 48, seed=3)
    frames.view(-1)[:256] = torch.arange(256, dtype=torch.uint8)                 # every byte value: the kernel's u8 / 255 against torch's division on all of them
    frames.view(-1)[-256:] = torch.arange(256, dtype=torch.uint8).flip(0)        # ... also through the byte-by-byte reads at the end of the buffer
    got = prepare_video(frames, (32, 48), crop_to_fit=True, device=DEV)
    want = (2.0 * (frames.float() / 255.0) - 1.0).to(BF).permute(0, 3, 1, 2)[None]
    assert torch.equal(got.cpu(), want)
    # a GPU tensor and a numpy array are taken as well
    assert torch.equal(prepare_video(frames.to(DEV), (32, 48), crop_to_fit=True), got) and torch.equal(prepare_video(frames.numpy(), (32, 48), crop_to_fit=True), got)


def test_prepare_video_does_not_depend_on_the_frame_count():
    from tokensgen_amd.video_io import prepare_video
    frames = _frames(5, 90, 160, seed=4).to(DEV)
    whole = prepare_video(frames, (40, 64), crop_to_fit=True)
    assert torch.equal(whole, prepare_video(frames, (40, 64), crop_to_fit=True))
    single = torch.cat([prepare_video(frames[f:f + 1], (40, 64), crop_to_fit=True) for f in range(5)], dim=1)
    assert torch.equal(whole, single)


def _all_patterns_video():
    """[1, 3, 4, 64, 86] bf16: 66 048 elements, every one of the 65 536 bit patterns at least once"""
    allv = VR.all_bf16_patterns()
    return torch.cat([allv, allv[:3 * 4 * 64 * 86 - 65536]]).view(1, 3, 4, 64, 86)


@pytest.mark.parametrize("rounding", [0, 1])
def test_frames_to_uint8_is_exact_on_every_bf16_pattern(rounding):
    from tokensgen_amd.video_io import frames_to_uint8
    v = _all_patterns_video()                                                     # [1, 3, 4, 64, 86]: 66 048 elements, every pattern at least once
    assert v.numel() >= 65536 and torch.isnan(v.float()).any() and torch.isinf(v.float()).any()
    want = VR.display_ref(v, rounding).permute(0, 2, 3, 4, 1)                     # [B, T, H, W, 3]
    got = frames_to_uint8(v.to(DEV), "bcthw", rounding)
    assert got.dtype == torch.uint8 and got.shape == (1, 4, 64, 86, 3) and torch.equal(got.cpu(), want)
    # the same values as a source video [B, F, 3, H, W]
    got2 = frames_to_uint8(v.permute(0, 2, 1, 3, 4).contiguous().to(DEV), "bfchw", rounding)
    assert torch.equal(got2.cpu(), want)
    # ... and as a permuted VIEW of it (strides, not layout, are what the kernel takes)
    assert torch.equal(frames_to_uint8(v.to(DEV).permute(0, 2, 1, 3, 4), "bfchw", rounding).cpu(), want)


@pytest.mark.parametrize("rounding", [0, 1])
def test_frames_to_uint8_odd_plane(rounding):
    from tokensgen_amd.video_io import frames_to_uint8
    v = (torch.randn(2, 3, 3, 7, 13, generator=torch.Generator().manual_seed(6)) * 0.7).to(BF)
    want = VR.display_ref(v, rounding).permute(0, 2, 3, 4, 1)
    assert torch.equal(frames_to_uint8(v.to(DEV), "bcthw", rounding).cpu(), want)
    assert torch.equal(frames_to_uint8(v.permute(0, 2, 1, 3, 4).contiguous().to(DEV), "bfchw", rounding).cpu(), want)
    assert rounding == 0 or not torch.equal(want, VR.display_ref(v, 0).permute(0, 2, 3, 4, 1))


def test_video_processor_output_types():
    from tokensgen_amd.video_io import VideoProcessor
    vp = VideoProcessor()
    v = (torch.randn(2, 3, 5, 16, 24, generator=torch.Generator().manual_seed(7)) * 0.8).to(BF)      # finite: the float outputs are compared as numbers
    unit = VR.display_unit_ref(v).permute(0, 2, 1, 3, 4)                                             # [B, T, 3, H, W] bf16
    pt = vp.postprocess_video(v.to(DEV), "pt")
    assert pt.dtype == BF and pt.shape == (2, 5, 3, 16, 24) and pt.is_cuda and torch.equal(pt.cpu(), unit)
    npo = vp.postprocess_video(v.to(DEV), "np")
    assert isinstance(npo, np.ndarray) and npo.dtype == np.float32 and npo.shape == (2, 5, 16, 24, 3)
    assert np.array_equal(npo, unit.permute(0, 1, 3, 4, 2).float().numpy())
    u8 = vp.postprocess_video(v.to(DEV), "uint8")
    assert u8.dtype == torch.uint8 and u8.is_cuda and u8.shape == (2, 5, 16, 24, 3)
    assert np.array_equal(u8.cpu().numpy(), (npo * 255).astype(np.uint8))                            # what export_to_video writes from "np"
    assert torch.equal(u8.cpu(), VR.display_ref(v, 0).permute(0, 2, 3, 4, 1))
    pil = vp.postprocess_video(v.to(DEV), "pil")
    assert len(pil) == 2 and len(pil[0]) == 5 and pil[0][0].size == (24, 16) and pil[0][0].mode == "RGB"
    want = VR.display_ref(v, 1).permute(0, 2, 3, 4, 1).numpy()
    assert all(np.array_equal(np.asarray(pil[b][t]), want[b, t]) for b in range(2) for t in range(5))
    assert np.array_equal(want, (npo * 255).round().astype(np.uint8))                                # numpy_to_pil
    # a NaN stays a NaN in the float outputs, as torch's clamp leaves it
    bad = v.clone()
    bad[0, 1, 2, 3, 4] = float("nan")
    assert torch.isnan(vp.postprocess_video(bad.to(DEV), "pt")[0, 2, 1, 3, 4]) and np.isnan(vp.postprocess_video(bad.to(DEV), "np")[0, 2, 3, 4, 1])
    with pytest.raises(ValueError):
        vp.postprocess_video(v.to(DEV), "latent")


def _noise(i, tag, shape):
    g = torch.Generator().manual_seed(1000 * i + tag)
    return torch.randn(shape, generator=g).to(BF).to(DEV)


def _fake_decode(z):
    """Stand-in for vae.decode on one chunk: [1, nf, C, h, w] -> bf16 [1, 3, 4 (nf - 1) + 1, 2h, 2w] (the hook behind the decode is under test; the VAE has its own tests)."""
    x = z.float().permute(0, 2, 1, 3, 4)[:, :3]
    x = torch.nn.functional.interpolate(x, size=(4 * (z.shape[1] - 1) + 1, 2 * z.shape[3], 2 * z.shape[4]), mode="nearest")
    return (x * 0.5).to(BF)


@pytest.mark.timeout(600)
def test_video_processor_through_the_fifo_driver():
    """The small pipeline of the FIFO tests (tiny DiT with vip layers, 52 steps, one 13-frame chunk): `pipe.video_processor` + output_type="uint8" gives
    frames_to_uint8 of what the driver returns as "pt" without a processor (the raw decoded [B, 3, T, H, W])."""
    from oracle import dit_ref as O
    from tokensgen_amd import fifo
    from tokensgen_amd.pipeline import MPFIFOVideoIPAdapterCogVideoXPipeline
    from tokensgen_amd.scheduler import CogVideoXDPMScheduler
    from tokensgen_amd.transformer import CogVideoXTransformer3DModel
    from tokensgen_amd.video_io import VideoProcessor, frames_to_uint8
    cfg = dict(num_attention_heads=2, attention_head_dim=64, num_layers=2, patch_size=2, time_embed_dim=128, text_embed_dim=64, in_channels=16, out_channels=16)
    vip = dict(length=30, func_type="1", scale=[0.6], resampler_params=dict(output_dim=128, num_height_queries=2, num_width_queries=3, num_temporal_queries=4))
    m = CogVideoXTransformer3DModel(num_attention_heads=2, attention_head_dim=64, num_layers=2, time_embed_dim=128, text_embed_dim=64,
                                    use_rotary_positional_embeddings=True, device=DEV)
    m.set_vip_layers(None, **vip)
    m.load_state_dict({k: v.to(BF) for k, v in O.make_state_dict(cfg, 128, seed=31).items()}, strict=True)
    sched = CogVideoXDPMScheduler(prediction_type="v_prediction", rescale_betas_zero_snr=True, snr_shift_scale=1.0, timestep_spacing="trailing")
    pipe = MPFIFOVideoIPAdapterCogVideoXPipeline(m, sched, resampler_config=dict(num_temporal_queries=4, num_height_queries=2, num_width_queries=3))
    assert getattr(pipe, "video_processor", None) is None                       # none by default: "pt" stays the raw decode
    g = torch.Generator().manual_seed(5)
    H, W, nf, T = 4, 6, 13, 52
    lat0 = torch.randn(1, nf, 16, H, W, generator=g).to(BF)
    pe, ne = torch.randn(1, 8, 64, generator=g).to(BF), torch.randn(1, 8, 64, generator=g).to(BF)
    emb = torch.randn(1, 4, 128, 2, 3, generator=g).to(BF)

    def run(output_type):
        out = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, image_embeddings=emb, height=H * 8, width=W * 8, num_chunks=1, num_inference_steps=T, latents=lat0,
                   step_noise=lambda i: _noise(i, 5, (nf, 2, 16, H, W)), output_type=output_type)
        return fifo.cogvideo_fifo_mp_v2([pipe], out, step_noise_fn=_noise, tail_noise_fn=lambda i, shape: _noise(i, 97, shape), decode_chunk_fn=_fake_decode)
    orig_pt, video_pt, _ = run("pt")
    assert video_pt.dtype == BF and video_pt.shape == (1, 3, 49, 2 * H, 2 * W)
    pipe.video_processor = VideoProcessor()
    orig_u8, video_u8, _ = run("uint8")
    assert video_u8.dtype == torch.uint8 and video_u8.shape == (1, 49, 2 * H, 2 * W, 3)
    assert torch.equal(video_u8, frames_to_uint8(video_pt, "bcthw", 0)) and torch.equal(orig_u8, frames_to_uint8(orig_pt, "bcthw", 0))
    assert video_u8.float().std() > 1                                            # not a constant picture


@pytest.mark.timeout(600)
def test_pipeline_accepts_frames(golden_dir):
    """pipe(frames=video, vip_generator=g) == pipe(image_embeddings=pipe.vae_encode_image(video, generator=g'), ...) bit for bit with equally seeded generators, on the
    tiny VAE + DiT + Resampler of the condensed-token tests; the video comes from prepare_video.  A raw prompt still raises."""
    from oracle import dit_ref as O
    from oracle import resampler_ref as RR
    from oracle import vae_ref as V
    from tokensgen_amd.pipeline import MPFIFOVideoIPAdapterCogVideoXPipeline
    from tokensgen_amd.resampler import Resampler
    from tokensgen_amd.scheduler import CogVideoXDPMScheduler
    from tokensgen_amd.transformer import CogVideoXTransformer3DModel
    from tokensgen_amd.vae import AutoencoderKLCogVideoX
    from tokensgen_amd.video_io import prepare_video
    gv = torch.load(os.path.join(golden_dir, "vae_tiny.pt"), weights_only=False)
    vcfg = gv["cfg"]
    dcfg = dict(num_attention_heads=2, attention_head_dim=64, num_layers=2, patch_size=2, time_embed_dim=128, text_embed_dim=64, in_channels=16, out_channels=16)
    vip = dict(length=30, func_type="1", scale=[0.6], resampler_params=dict(output_dim=128, num_height_queries=2, num_width_queries=3, num_temporal_queries=4))
    rcfg = dict(dim=128, depth=2, dim_head=64, heads=2, num_height_queries=2, num_width_queries=3, num_temporal_queries=4, embedding_dim=128, output_dim=128, ff_mult=4,
                max_height_seq_len=4, max_width_seq_len=6, max_temporal_seq_len=5)
    vae = AutoencoderKLCogVideoX(block_out_channels=vcfg["block_out_channels"], layers_per_block=1, sample_height=64, sample_width=96, device=DEV)
    vae.load_state_dict(V.make_state_dict(vcfg, seed=gv["weight_seed"]))
    m = CogVideoXTransformer3DModel(num_attention_heads=2, attention_head_dim=64, num_layers=2, time_embed_dim=128, text_embed_dim=64,
                                    use_rotary_positional_embeddings=True, device=DEV)
    m.set_vip_layers(None, **vip)
    m.load_state_dict({k: v.to(BF) for k, v in O.make_state_dict(dcfg, 128, seed=31).items()}, strict=True)
    rs = Resampler(**rcfg, device=DEV)
    rs.load_state_dict(RR.make_state_dict(rcfg, seed=22))
    sched = CogVideoXDPMScheduler(prediction_type="v_prediction", rescale_betas_zero_snr=True, snr_shift_scale=1.0, timestep_spacing="trailing")
    pipe = MPFIFOVideoIPAdapterCogVideoXPipeline(m, sched, vae=vae, resampler=rs)
    video = prepare_video(_frames(17, 80, 150, seed=8), (64, 96), crop_to_fit=True, device=DEV)       # [1, 17, 3, 64, 96]: one 17-frame chunk -> 5 latent frames of 8 x 12
    g = torch.Generator().manual_seed(9)
    H, W, nf, T = 8, 12, 5, 4
    lat0 = torch.randn(1, nf, 16, H, W, generator=g).to(BF)
    pe, ne = torch.randn(1, 8, 64, generator=g).to(BF), torch.randn(1, 8, 64, generator=g).to(BF)
    common = dict(prompt_embeds=pe, negative_prompt_embeds=ne, height=64, width=96, num_frames_per_chunk=17, num_chunks=1, num_inference_steps=T, latents=lat0,
                  step_noise=lambda i: _noise(i, 5, (nf, 2, 16, H, W)), video_ipadapter_start_frame_idx=1000)
    seeded = lambda: torch.Generator(device=DEV).manual_seed(11)
    a = pipe(frames=video, vip_generator=seeded(), **common)
    emb = pipe.vae_encode_image(video, nf_per_chunk=17, compressed_nf_per_chunk=5, generator=seeded())
    assert emb.shape == (2, 8, 128, 2, 3)
    b = pipe(image_embeddings=emb, **common)
    assert torch.equal(a.image_embeddings, emb) and torch.equal(b.image_embeddings, emb)
    assert torch.equal(a.fifo_latents, b.fifo_latents) and torch.equal(a.orig_latents, b.orig_latents) and bool(torch.isfinite(a.fifo_latents).all())
    # another posterior draw gives other tokens: the generator is really used
    c = pipe(frames=video, vip_generator=torch.Generator(device=DEV).manual_seed(12), **common)
    assert not torch.equal(c.image_embeddings, emb)
    # the three-way batch of use_separate_guidance and the no-guidance single row come out of the encode laid out as the base stage wants them
    s = pipe(frames=video, vip_generator=seeded(), use_separate_guidance=True, guidance_scale_img=4.0, **common)
    assert s.image_embeddings.shape == (3, 8, 128, 2, 3) and torch.equal(s.image_embeddings[0], emb[0]) and torch.equal(s.image_embeddings[2], emb[0])
    n = pipe(frames=video, vip_generator=seeded(), guidance_scale=1.0, **{**common, "negative_prompt_embeds": None})
    assert n.image_embeddings.shape == (1, 8, 128, 2, 3) and torch.equal(n.image_embeddings[0], emb[0])
    with pytest.raises(NotImplementedError):
        pipe(prompt="a cat")
