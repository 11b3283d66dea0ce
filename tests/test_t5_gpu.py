"""GPU: the T5 encoder kernels (csrc/t5.hip) and the encoder built from them (tokensgen_amd/t5.py).

Per kernel: inputs are bf16 values; the reference is tests/t5_ref.py in exact float64; the bound is 2 x the error that t5_ref's kernel-rounding mode (bf16 wherever
the kernel stores bf16) has against that reference on the same inputs — the kernel rounds at the same points and differs in summation order only.  Where that
emulation is exact (attention over one key: P = 1, out = v) the kernel must be exact too (the bound is then 1e-12, for the strict `<`).
Whole model: the error against the float64 run of the library stored in tests/golden/t5_tiny.pt must be at most 1.5 x the error of the library's own bf16 run stored
beside it; tests/test_t5_cpu.py shows that the kernels' rounding points emulated on the CPU land at 0.93 .. 0.98 x of it and that every semantic mutation lands
>= 29 x beyond the bound."""
import os

import pytest
import torch

import t5_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
F64 = torch.float64


@pytest.fixture(scope="module")
def gold(golden_dir):
    return torch.load(os.path.join(golden_dir, "t5_tiny.pt"), weights_only=False)


@pytest.fixture(scope="module")
def tiny(gold):
    from tokensgen_amd.t5 import T5EncoderModel
    m = T5EncoderModel(gold["config"], device=DEV)
    m.load_state_dict(gold["state_dict"], strict=True)
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


# ---------------------------------------------------------------------------------------------------- kernels
@pytest.mark.timeout(120)
@pytest.mark.parametrize("rows,D", [(1, 128), (453, 128), (1, 4096), (453, 4096)])
def test_rmsnorm_vs_float64(rows, D, parity):
    from tokensgen_amd import kernels as K
    x, w = _randn((rows, D), 1, 3.0), (1.0 + 0.25 * torch.randn(D, generator=torch.Generator().manual_seed(2))).to(BF)
    if rows > 1:
        x[7] = 0                                      # a row of zeros: rsqrt(eps) * 0
        x[8] *= 1e-3                                  # a row whose mean square is of the order of eps
    exact = R.rmsnorm(x.to(F64), w.to(F64), 1e-6)
    out = torch.empty(rows, D, dtype=BF, device=DEV)
    K.rmsnorm(x.to(DEV), w.to(DEV), out, 1e-6)
    parity(R.rel_l2(out, exact), _bound(R.rmsnorm(x.to(F64), w.to(F64), 1e-6, rounding=True), exact), f"tg_rmsnorm rows {rows} D {D}")
    if rows > 1:
        assert (out[7] == 0).all()
        # a strided view (the leading dimension is not D, a column offset) gives the same bits
        wide = torch.zeros(rows, D + 64, dtype=BF, device=DEV)
        wide[:, 8:D + 8] = x.to(DEV)
        out2 = torch.empty(rows, D + 64, dtype=BF, device=DEV)
        K.rmsnorm(wide[:, 8:D + 8], w.to(DEV), out2[:, :D], 1e-6)
        assert torch.equal(out2[:, :D], out)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("rows", [1, 453])
def test_gated_gelu_vs_float64(rows, parity):
    from tokensgen_amd import kernels as K
    F = 256
    h = _randn((rows, 2 * F), 3, 2.5)
    h[0, :8] = torch.tensor([0.0, -0.0, 30.0, -30.0, 1e-3, -1e-3, 8.0, -8.0]).to(BF)           # both tails of the gelu and its origin
    exact = R.gated_gelu(h.to(F64))
    out = torch.empty(rows, F, dtype=BF, device=DEV)
    K.gated_gelu(h.to(DEV), out)
    parity(R.rel_l2(out, exact), _bound(R.gated_gelu(h.to(F64), rounding=True), exact), f"tg_gated_gelu rows {rows}")
    assert torch.isfinite(out).all()
    if rows > 1:
        x, y = _randn((rows, F), 4), _randn((rows, F), 5)
        s = torch.empty(rows, F, dtype=BF, device=DEV)
        K.residual_add(x.to(DEV), y.to(DEV), s)
        assert torch.equal(s.cpu(), (x.float() + y.float()).to(BF))                            # one rounding of an exact fp32 sum: bitwise


def _attention_case(B, S, H, seed):
    """q | k | v as bf16 [B, S, 3 H 64]; a bias-by-distance table with entries of +-20 among moderate ones"""
    qkv = _randn((B, S, 3 * H * 64), seed)
    qkv[..., :H * 64] *= 0.5                          # scores of a few units
    g = torch.Generator().manual_seed(seed + 1)
    table = 1.5 * torch.randn(H, 2 * S - 1, generator=g)
    table[:, ::5] = 20.0
    table[:, 2::7] = -20.0
    table = table.to(BF).float()
    return qkv, table


def _attention_refs(qkv, table, H):
    B, S, _ = qkv.shape
    q, k, v = (t.to(F64).view(B, S, H, 64) for t in qkv.split(H * 64, dim=-1))
    i, j = torch.arange(S)[:, None], torch.arange(S)[None, :]
    dense = table.to(F64)[:, j - i + S - 1]
    return R.attention(q, k, v, dense), R.attention(q, k, v, dense, rounding=True)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("S", [1, 7, 64, 226, 512])
def test_t5_attention_vs_float64(S, B, parity):
    from tokensgen_amd import kernels as K
    H = 2
    qkv, table = _attention_case(B, S, H, 10 * S + B)
    exact, emulated = _attention_refs(qkv, table, H)
    out = torch.empty(B, S, H * 64, dtype=BF, device=DEV)
    K.t5_attention(qkv.to(DEV), table.to(DEV), out, H)
    assert torch.isfinite(out).all()
    parity(R.rel_l2(out, exact), _bound(emulated, exact), f"tg_t5_attention S {S} B {B}")


@pytest.mark.timeout(120)
def test_t5_attention_reads_a_strided_fused_buffer(parity):
    """q, k, v inside a wider buffer (row stride 512, not 384; a batch stride that is not S * ld; a non-zero column offset), NaN everywhere else"""
    from tokensgen_amd import kernels as K
    B, S, H = 2, 226, 2
    qkv, table = _attention_case(B, S, H, 77)
    exact, emulated = _attention_refs(qkv, table, H)
    buf = torch.full((B, S + 3, 512), float("nan"), dtype=BF, device=DEV)
    view = buf[:, 1:S + 1, 64:64 + 3 * H * 64]
    view.copy_(qkv)
    out = torch.empty(B, S, H * 64, dtype=BF, device=DEV)
    K.t5_attention(view, table.to(DEV), out, H)
    assert torch.isfinite(out).all()
    parity(R.rel_l2(out, exact), _bound(emulated, exact), "tg_t5_attention strided")
    dense = torch.empty_like(out)
    K.t5_attention(qkv.to(DEV), table.to(DEV), dense, H)
    assert torch.equal(dense, out)


# ---------------------------------------------------------------------------------------------------- the model
@pytest.mark.timeout(120)
@pytest.mark.parametrize("case", ["s226", "s7", "s1"])
def test_tiny_model_vs_library_float64(case, gold, tiny, parity):
    c = gold["cases"][case]
    res = tiny(c["input_ids"].to(DEV))
    out = res[0]
    assert res.last_hidden_state is out and out.dtype == BF and out.shape == tuple(c["input_ids"].shape) + (128,) and torch.isfinite(out).all()
    p = c["positions"]
    library = R.rel_l2(c["bf16"], c["f64"])
    parity(R.rel_l2(out.cpu()[p[:, 0], p[:, 1]], c["f64"]), 1.5 * library, f"T5 tiny {case}: error against float64, bound 1.5 x the library's bf16 run ({library:.3e})")


@pytest.mark.timeout(120)
def test_launches_per_forward(gold, tiny):
    """a [2, 7] id batch through an encoder of L layers: ten launches per block and the final norm.  No other kernel."""
    ids = gold["cases"]["s7"]["input_ids"].to(DEV)
    assert ids.shape == (2, 7)
    L = tiny.config.num_layers
    assert _launch_counts(lambda: tiny(ids)) == {"gemm": 4 * L, "rmsnorm": 2 * L + 1, "t5_attention": L, "residual_add": 2 * L, "gated_gelu": L}


@pytest.mark.timeout(300)
def test_one_real_width_layer_vs_fp32(parity):
    """d_model 4096, 64 heads, d_ff 10240, one layer, [3, 226]: against t5_ref in fp32 on the GPU, the bound is 1.5 x the error of the bf16 torch route"""
    from tokensgen_amd.t5 import T5EncoderModel
    cfg = dict(vocab_size=512, d_model=4096, d_kv=64, num_heads=64, d_ff=10240, num_layers=1, feed_forward_proj="gated-gelu", relative_attention_num_buckets=32,
               relative_attention_max_distance=128, layer_norm_epsilon=1e-6)
    m = T5EncoderModel(cfg, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(11)
    sd = {}
    for k, v in m.state_dict().items():
        r = torch.randn(v.shape, generator=g, device=DEV)
        if k.endswith("layer_norm.weight"):
            r = 1.0 + 0.25 * r
        elif "relative_attention_bias" in k:
            r = 1.5 * r
        elif k.endswith(("shared.weight", "embed_tokens.weight")):
            r = sd.get("shared.weight", r)
        elif ".q." in k:
            r = r * (4096 * 64) ** -0.5 * 2.0
        elif ".wo." in k:
            r = r * 10240 ** -0.5
        else:
            r = r * 4096 ** -0.5
        sd[k] = r.to(BF)
    m.load_state_dict(sd, strict=True)
    ids = torch.randint(2, 512, (3, 226), generator=torch.Generator().manual_seed(12))
    ids[0, 30:], ids[1, 1:], ids[1, 0] = 0, 0, 1
    out = m(ids.to(DEV))[0]
    assert torch.isfinite(out).all()
    exact = R.t5_forward(sd, cfg, ids, dtype=torch.float32, device=DEV)
    torch_bf16 = R.rel_l2(R.t5_forward_torch_bf16(sd, cfg, ids, device=DEV), exact)
    parity(R.rel_l2(out, exact), 1.5 * torch_bf16, f"T5 real-width layer: error against fp32, bound 1.5 x the bf16 torch route ({torch_bf16:.3e})")


@pytest.mark.timeout(120)
def test_two_calls_are_bitwise_equal_and_rows_do_not_see_each_other(gold, tiny):
    ids = gold["cases"]["s226"]["input_ids"].to(DEV)
    a = tiny(ids)[0].clone()
    b = tiny(ids)[0]
    assert torch.equal(a, b)
    assert torch.equal(tiny(ids[:1])[0], a[:1]) and torch.equal(tiny(ids[1:])[0], a[1:])
    three = torch.cat([ids[1:], ids, ids[:1]])
    assert torch.equal(tiny(three)[0][1:3], a)


@pytest.mark.timeout(300)
def test_base_stage_with_a_prompt_equals_the_same_call_with_its_embeddings(tiny):
    """The tiny To2V base stage (the configuration of tests/test_fifo_gpu.py: 2 heads, 2 layers, condensed tokens, 13 latent frames of 4 x 6) with `prompt=` and an
    attached encoder + tokenizer, against the same call with the `prompt_embeds` that encode_prompt returns: bitwise."""
    from tokensgen_amd.pipeline import MPFIFOVideoIPAdapterCogVideoXPipeline
    from tokensgen_amd.scheduler import CogVideoXDPMScheduler
    from tokensgen_amd.t5 import encode_prompt
    from tokensgen_amd.transformer import CogVideoXTransformer3DModel
    m = CogVideoXTransformer3DModel(num_attention_heads=2, attention_head_dim=64, num_layers=2, time_embed_dim=128, text_embed_dim=tiny.config.d_model,
                                    use_rotary_positional_embeddings=True, device=DEV)
    m.set_vip_layers(None, length=30, func_type="1", scale=[0.6],
                     resampler_params=dict(output_dim=128, num_height_queries=2, num_width_queries=3, num_temporal_queries=4))
    g = torch.Generator().manual_seed(5)
    m.load_state_dict({k: ((1.0 if (k.endswith("weight") and v.dim() == 1) else 0.0) + 0.05 * torch.randn(v.shape, generator=g)).to(BF)
                       for k, v in m.state_dict().items()}, strict=True)
    sched = CogVideoXDPMScheduler(prediction_type="v_prediction", rescale_betas_zero_snr=True, snr_shift_scale=1.0, timestep_spacing="trailing")
    tok = R.StubTokenizer()
    H, W, nf = 4, 6, 13
    lat0 = torch.randn(1, nf, 16, H, W, generator=g).to(BF)
    emb = torch.randn(1, 8, 128, 2, 3, generator=g).to(BF)
    noise = [torch.randn(nf, 2, 16, H, W, generator=g).to(BF) for _ in range(6)]
    kw = dict(image_embeddings=emb, height=H * 8, width=W * 8, latents=lat0, num_inference_steps=6, step_noise=lambda i: noise[i])
    bare = MPFIFOVideoIPAdapterCogVideoXPipeline(m, sched, resampler_config=dict(num_temporal_queries=4, num_height_queries=2, num_width_queries=3))
    with pytest.raises(NotImplementedError):
        bare(prompt="a cat", **kw)
    pipe = MPFIFOVideoIPAdapterCogVideoXPipeline(m, sched, resampler_config=dict(num_temporal_queries=4, num_height_queries=2, num_width_queries=3),
                                                 text_encoder=tiny, tokenizer=tok)
    a = pipe(prompt="a cat on a mat", negative_prompt="blurry", max_sequence_length=16, **kw)
    pe, ne = encode_prompt(tok, tiny, "a cat on a mat", "blurry", max_sequence_length=16, device=DEV)
    assert pe.shape == ne.shape == (1, 16, 128) and not torch.equal(pe, ne)
    b = bare(prompt_embeds=pe, negative_prompt_embeds=ne, **kw)
    assert torch.isfinite(a.fifo_latents).all() and a.prompt_embeds.shape == (2, 16, 128)
    assert torch.equal(a.prompt_embeds, b.prompt_embeds) and torch.equal(a.fifo_latents, b.fifo_latents) and torch.equal(a.orig_latents, b.orig_latents)
