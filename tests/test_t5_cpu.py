"""CPU: the T5 encoder's host side (tokensgen_amd/t5.py), the oracle the GPU tests use (tests/t5_ref.py) pinned to the library's own float64 run stored in
tests/golden/t5_tiny.pt (tools/make_t5_golden.py), and the mutation check that gives the GPU tolerance its meaning.  No GPU, no transformers."""
import ctypes
import json
import logging
import os

import pytest
import torch

import t5_ref as R

BF = torch.bfloat16
GPU_BOUND_FACTOR = 1.5          # tests/test_t5_gpu.py: error against float64 <= 1.5 x the error of the library's own bf16 run


@pytest.fixture(scope="module")
def gold(golden_dir):
    return torch.load(os.path.join(golden_dir, "t5_tiny.pt"), weights_only=False)


def _at(out, case):
    p = case["positions"]
    return out[p[:, 0], p[:, 1]]


# ---------------------------------------------------------------------------------------------------- the oracle, pinned
def test_oracle_float64_reproduces_the_library(gold):
    """t5_ref in exact float64 mode against the library's float64 run.  The library computes the T5LayerNorm variance in float32 even in a float64 model
    (`hidden_states.to(torch.float32).pow(2).mean`), which leaves a relative residue of about 1e-7 (measured here: 6.4e-8 .. 1.4e-7); asserted with one decade of
    margin, four decades below the bf16 errors the GPU tests deal in."""
    for name, c in gold["cases"].items():
        out = R.t5_forward(gold["state_dict"], gold["config"], c["input_ids"])
        err = R.rel_l2(_at(out, c), c["f64"])
        print(f"{name}: float64 oracle against the library's float64 run: rel-L2 {err:.3e}")
        assert err < 1.4e-6, (name, err)


def test_bucket_rule_and_distance_table_match_the_library(gold):
    from tokensgen_amd import t5
    d = torch.arange(-511, 512)
    assert torch.equal(R.bucket(d), gold["buckets"].long())
    assert torch.equal(t5.relative_position_bucket(d), gold["buckets"].long())
    b = gold["buckets"].long()
    assert (b[511 + 128:] == 31).all() and (b[:511 - 127] == 15).all() and b[511 + 64] < 31 and b[511 - 64] < 15          # distances past 128 saturate
    w = gold["state_dict"]["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"]
    for S in (1, 7, 226, 512):
        table = t5.bias_by_distance(w, S)
        assert table.dtype == torch.float32 and table.shape == (2, 2 * S - 1) and table.stride() == (2 * S - 1, 1)
        i, j = torch.arange(S)[:, None], torch.arange(S)[None, :]
        assert torch.equal(table[:, j - i + S - 1], R.dense_bias(w.float(), S))


def test_kernel_rounding_mode_is_as_close_as_the_library_bf16_run(gold):
    """The planned rounding points, emulated on the CPU, must themselves sit inside the GPU bound (otherwise the bound could not be met by a correct kernel)."""
    for name, c in gold["cases"].items():
        lib = R.rel_l2(c["bf16"], c["f64"])
        emu = R.rel_l2(_at(R.t5_forward(gold["state_dict"], gold["config"], c["input_ids"], rounding=True), c), c["f64"])
        print(f"{name}: library bf16 {lib:.3e}, kernel rounding points {emu:.3e} ({emu / lib:.2f} x)")
        assert emu < GPU_BOUND_FACTOR * lib


def test_torch_bf16_route_is_a_yardstick_of_the_library_s_size(gold):
    """t5_ref.t5_forward_torch_bf16 (the yardstick of the real-width GPU test, where no library run exists) against the library's own bf16 run: not the same bits
    (the library's attention takes another route through torch), but the same size of error against float64 — measured 1.03 x, 1.14 x and 1.00 x of the library's.
    A yardstick 1.5 x off either way would make the real-width bound mean something else than the tiny model's."""
    for name, c in gold["cases"].items():
        lib = R.rel_l2(c["bf16"], c["f64"])
        route = R.rel_l2(_at(R.t5_forward_torch_bf16(gold["state_dict"], gold["config"], c["input_ids"]), c), c["f64"])
        print(f"{name}: library bf16 {lib:.3e}, torch bf16 route {route:.3e} ({route / lib:.2f} x)")
        assert lib / 1.5 < route < 1.5 * lib


@pytest.mark.parametrize("mutation", ["no_bias", "scale", "swap_ff", "flip_distance", "mask_pads"])
def test_every_semantic_mutation_exceeds_the_gpu_bound_tenfold(gold, mutation):
    """What makes `1.5 x the library's bf16 error` a meaningful bound: each wrong reading of the model, run with the kernels' rounding points, lands at least
    10 x beyond it.  On the prompt row of the [2, 226] case (the all-pad row has no key left under mask_pads)."""
    c = gold["cases"]["s226"]
    row0 = c["positions"][:, 0] == 0
    pos = c["positions"][row0]
    bound = GPU_BOUND_FACTOR * max(R.rel_l2(c["bf16"], c["f64"]), R.rel_l2(c["bf16"][row0], c["f64"][row0]))
    out = R.t5_forward(gold["state_dict"], gold["config"], c["input_ids"][:1], rounding=True, mutate=mutation)
    err = R.rel_l2(out[0, pos[:, 1]], c["f64"][row0])
    print(f"{mutation}: {err:.3e} against the bound {bound:.3e} ({err / bound:.1f} x)")
    assert err >= 10 * bound, (mutation, err, bound)


# ---------------------------------------------------------------------------------------------------- loading
def test_state_dict_round_trip_tied_embedding_and_fused_row_order(gold):
    from tokensgen_amd.t5 import T5EncoderModel
    sd, cfg = gold["state_dict"], gold["config"]
    m = T5EncoderModel(cfg, device="cpu")
    assert m.dtype == BF and m.device == torch.device("cpu") and m.config.d_model == 128 and m.to("cpu") is m
    m.load_state_dict(sd, strict=True)
    out = m.state_dict()
    assert set(out) == set(sd) and all(torch.equal(out[k], sd[k]) for k in sd)
    a, f = "encoder.block.1.layer.0.SelfAttention.", "encoder.block.1.layer.1.DenseReluDense."
    assert torch.equal(m._w["l1.qkv"], torch.cat([sd[a + "q.weight"], sd[a + "k.weight"], sd[a + "v.weight"]]))          # q rows, then k, then v
    assert torch.equal(m._w["l1.wi"], torch.cat([sd[f + "wi_0.weight"], sd[f + "wi_1.weight"]]))                         # wi_0, then wi_1
    for name in ("shared.weight", "encoder.embed_tokens.weight"):                                                        # the tied embedding under either name
        other = ({"shared.weight", "encoder.embed_tokens.weight"} - {name}).pop()
        m2 = T5EncoderModel(cfg, device="cpu")
        m2.load_state_dict({k: v for k, v in sd.items() if k != other}, strict=True)
        assert torch.equal(m2.state_dict()[other], sd["shared.weight"])
    with pytest.raises(RuntimeError, match="missing keys"):
        T5EncoderModel(cfg, device="cpu").load_state_dict({k: v for k, v in sd.items() if "final_layer_norm" not in k}, strict=True)
    with pytest.raises(RuntimeError, match="unexpected keys"):
        T5EncoderModel(cfg, device="cpu").load_state_dict(dict(sd, **{"lm_head.weight": sd["shared.weight"]}), strict=True)


def test_from_pretrained_reads_a_two_shard_checkpoint(gold, tmp_path):
    from safetensors.torch import save_file
    from tokensgen_amd.t5 import T5EncoderModel
    sd = {k: v for k, v in gold["state_dict"].items() if k != "encoder.embed_tokens.weight"}
    d = tmp_path / "text_encoder"
    d.mkdir()
    (d / "config.json").write_text(json.dumps(dict(gold["config"], architectures=["T5EncoderModel"], _name_or_path="x", torch_dtype="bfloat16")))
    names = sorted(sd)
    shards = {"model-00001-of-00002.safetensors": names[:len(names) // 2], "model-00002-of-00002.safetensors": names[len(names) // 2:]}
    for fn, ks in shards.items():
        save_file({k: sd[k].contiguous() for k in ks}, str(d / fn))
    (d / "model.safetensors.index.json").write_text(json.dumps({"metadata": {}, "weight_map": {k: fn for fn, ks in shards.items() for k in ks}}))
    m = T5EncoderModel.from_pretrained(str(tmp_path), device="cpu")
    assert all(torch.equal(m.state_dict()[k], v) for k, v in gold["state_dict"].items())
    one = tmp_path / "single"
    one.mkdir()
    (one / "config.json").write_text(json.dumps(gold["config"]))
    save_file({k: v.contiguous() for k, v in sd.items()}, str(one / "model.safetensors"))
    m1 = T5EncoderModel.from_pretrained(str(one), subfolder=None, device="cpu")
    assert all(torch.equal(m1.state_dict()[k], v) for k, v in gold["state_dict"].items())
    os.remove(str(d / "model-00002-of-00002.safetensors"))
    with pytest.raises(Exception):
        T5EncoderModel.from_pretrained(str(tmp_path), device="cpu")


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals(gold):
    from tokensgen_amd import lib as L
    from tokensgen_amd.t5 import T5EncoderModel
    cfg = gold["config"]
    with pytest.raises(NotImplementedError, match="d_kv"):
        T5EncoderModel(dict(cfg, d_kv=32), device="cpu")
    for proj in ("relu", "gelu", "gated-silu"):
        with pytest.raises(NotImplementedError, match="feed_forward_proj"):
            T5EncoderModel(dict(cfg, feed_forward_proj=proj), device="cpu")
    with pytest.raises(NotImplementedError, match="N % 128"):
        T5EncoderModel(dict(cfg, d_model=192), device="cpu")
    with pytest.raises(NotImplementedError, match="N % 128"):
        T5EncoderModel(dict(cfg, d_ff=96), device="cpu")
    m = T5EncoderModel(cfg, device="cpu")
    ids = gold["cases"]["s7"]["input_ids"]
    with pytest.raises(NotImplementedError, match="pipeline_cogvideox_mp_fifo.py:397.*pipeline_cogvideox_t2to.py:345.*train_cogvideo_to2v.py:917"):
        m(ids, attention_mask=torch.ones_like(ids))
    with pytest.raises(RuntimeError, match="GPU"):
        m(ids)
    with pytest.raises(ValueError, match="512"):
        m(torch.zeros(1, 513, dtype=torch.long))
    with pytest.raises(NotImplementedError):
        m.requires_grad_(True)
    # the exports validate before any launch: null arguments, and S = 513 with real pointers
    lib = L.load()
    assert lib.tg_rmsnorm(None, 0, None, None, 0, 0, 0, 0.0, None) == -1 and b"tg_rmsnorm: null pointer" in lib.tg_last_error_string()
    assert lib.tg_t5_attention(None, None, None, 0, 0, None, None, 0, 0, 0, None) == -1 and b"tg_t5_attention: null pointer" in lib.tg_last_error_string()
    assert lib.tg_gated_gelu(None, 0, None, 0, 0, 0, None) == -1 and b"tg_gated_gelu: null pointer" in lib.tg_last_error_string()
    assert lib.tg_residual_add(None, None, None, 0, None) == -1 and b"tg_residual_add: null pointer" in lib.tg_last_error_string()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf) + (16 - ctypes.addressof(buf) % 16)
    for S in (0, 513):
        assert lib.tg_t5_attention(p, p, p, 384, 0, p, p, 1, S, 2, None) == -2 and b"1 <= S <= 512" in lib.tg_last_error_string()
    assert lib.tg_t5_attention(p + 2, p, p, 384, 0, p, p, 1, 7, 2, None) == -3
    assert lib.tg_t5_attention(p, p, p, 64, 0, p, p, 1, 7, 2, None) == -2                       # ld < 64 H
    assert lib.tg_rmsnorm(p, 96, p, p, 96, 1, 96, 1e-6, None) == -2 and b"D % 64" in lib.tg_last_error_string()
    assert lib.tg_rmsnorm(p, 0, p, p, 128, 0, 128, 1e-6, None) == -2 and lib.tg_rmsnorm(p + 2, 128, p, p, 128, 1, 128, 1e-6, None) == -3
    assert lib.tg_gated_gelu(p, 24, p, 12, 1, 12, None) == -2 and lib.tg_gated_gelu(p + 2, 32, p, 16, 1, 16, None) == -3
    assert lib.tg_residual_add(p, p, p, 12, None) == -2 and lib.tg_residual_add(p, p + 2, p, 16, None) == -3


# ---------------------------------------------------------------------------------------------------- encode_prompt
class CountingEncoder:
    """Stands where the encoder does: row b of the output is filled with 1000 b + the first token id, so order and repeats can be read off."""
    device, dtype = torch.device("cpu"), BF

    def __init__(self):
        self.calls = []

    def __call__(self, input_ids, attention_mask=None):
        self.calls.append(input_ids.clone())
        B, S = input_ids.shape
        out = (1000.0 * torch.arange(B)[:, None, None] + input_ids[:, :1, None].float()).expand(B, S, 4).contiguous()
        return (out,)


def test_encode_prompt_follows_the_reference(caplog):
    from tokensgen_amd.t5 import compute_prompt_embeddings, encode_prompt
    tok, enc = R.StubTokenizer(), CountingEncoder()
    pe, ne = encode_prompt(tok, enc, "a cat", max_sequence_length=8)
    assert pe.shape == ne.shape == (1, 8, 4) and pe.dtype == BF
    assert enc.calls[0][0].tolist() == tok("a cat", padding="max_length", max_length=8).input_ids[0].tolist()
    assert enc.calls[1][0].tolist() == [1, 0, 0, 0, 0, 0, 0, 0]                                   # the default negative prompt is "": EOS then pads
    enc.calls.clear()
    pe, ne = encode_prompt(tok, enc, "a cat", do_classifier_free_guidance=False, max_sequence_length=8)
    assert ne is None and len(enc.calls) == 1
    given = torch.zeros(1, 8, 4)
    assert encode_prompt(tok, enc, "a cat", negative_prompt_embeds=given, max_sequence_length=8)[1] is given
    assert encode_prompt(tok, enc, None, prompt_embeds=given, max_sequence_length=8)[0] is given
    with pytest.raises(TypeError, match="`negative_prompt` should be the same type to `prompt`, but got <class 'tuple'> != <class 'list'>"):
        encode_prompt(tok, enc, "a cat", negative_prompt=("bad",), max_sequence_length=8)
    with pytest.raises(ValueError, match="has batch size 2, but `prompt`: .* has batch size 1. Please make sure that passed `negative_prompt` matches"):
        encode_prompt(tok, enc, ["a cat"], negative_prompt=["x", "y"], max_sequence_length=8)
    # num_videos_per_prompt = 2: each prompt's rows stay together (repeat along the sequence axis, then view)
    pe, ne = encode_prompt(tok, enc, ["b", "c"], negative_prompt=["d", "e"], num_videos_per_prompt=2, max_sequence_length=8, dtype=torch.float32)
    first = lambda w: float(tok(w).input_ids[0, 0])
    assert pe.shape == (4, 8, 4) and pe[:, 0, 0].tolist() == [first("b"), first("b"), 1000 + first("c"), 1000 + first("c")]
    assert ne[:, 0, 0].tolist() == [first("d"), first("d"), 1000 + first("e"), 1000 + first("e")]
    # truncation: warned with the removed part, as the reference words it
    caplog.clear()
    with caplog.at_level(logging.WARNING, logger="tokensgen_amd.t5"):
        encode_prompt(tok, enc, "one two three four five six", do_classifier_free_guidance=False, max_sequence_length=4)
    assert "The following part of your input was truncated because `max_sequence_length` is set to  4 tokens" in caplog.text
    assert enc.calls[-1].shape == (1, 4) and enc.calls[-1][0, -1] == 1
    caplog.clear()
    with caplog.at_level(logging.WARNING, logger="tokensgen_amd.t5"):
        encode_prompt(tok, enc, "one two", do_classifier_free_guidance=False, max_sequence_length=4)
    assert "truncated" not in caplog.text
    out = compute_prompt_embeddings(tok, enc, ["a", "b"], 8, "cpu", torch.float32)
    assert out.shape == (2, 8, 4) and out.dtype == torch.float32
    with pytest.raises(NotImplementedError, match="requires_grad"):
        compute_prompt_embeddings(tok, enc, "a", 8, "cpu", torch.float32, requires_grad=True)


# ---------------------------------------------------------------------------------------------------- pipelines
def test_pipelines_take_an_encoder_and_refuse_a_prompt_without_one():
    from tokensgen_amd.pipeline import MPFIFOVideoIPAdapterCogVideoXPipeline
    from tokensgen_amd.pipeline_t2to import LongVGenCogVideoXPipeline
    from tokensgen_amd.scheduler import CogVideoXDPMScheduler
    from tokensgen_amd.transformer import CogVideoXTransformer3DModel
    m = CogVideoXTransformer3DModel(num_attention_heads=2, attention_head_dim=64, num_layers=1, time_embed_dim=128, text_embed_dim=128,
                                    use_rotary_positional_embeddings=True, device="cpu")
    sched = CogVideoXDPMScheduler(prediction_type="v_prediction", rescale_betas_zero_snr=True, snr_shift_scale=1.0, timestep_spacing="trailing")
    tok, enc = R.StubTokenizer(), CountingEncoder()
    for cls in (MPFIFOVideoIPAdapterCogVideoXPipeline, LongVGenCogVideoXPipeline):
        assert cls.text_encoder is None and cls.tokenizer is None
        bare = cls(m, sched)
        assert bare.text_encoder is None and bare.tokenizer is None
        with pytest.raises(NotImplementedError, match="T5 prompt encoding is upstream of the hot path"):
            bare(prompt="a cat")
        half = cls(m, sched, text_encoder=enc)
        with pytest.raises(NotImplementedError, match="T5 prompt encoding is upstream of the hot path"):
            half(prompt="a cat")
        full = cls(m, sched, text_encoder=enc, tokenizer=tok)
        assert full.text_encoder is enc and full.tokenizer is tok
    with pytest.raises(NotImplementedError, match="T5 prompt encoding is upstream"):
        LongVGenCogVideoXPipeline(m, sched)(negative_prompt="x")
    # with both attached the prompt IS encoded (the stand-in encoder is called with max_sequence_length tokens) before the call reaches the GPU-only part
    full = MPFIFOVideoIPAdapterCogVideoXPipeline(m, sched, text_encoder=enc, tokenizer=tok)
    enc.calls.clear()
    with pytest.raises(RuntimeError, match="GPU"):
        full(prompt="a cat", negative_prompt="blurry", max_sequence_length=16, height=32, width=48, num_inference_steps=2)
    assert [c.shape for c in enc.calls] == [(1, 16), (1, 16)] and enc.calls[1][0, 0] == tok("blurry").input_ids[0, 0]
    with pytest.raises(NotImplementedError, match="one prompt per call"):
        full(prompt=["a", "b"])
    # the T2To stage: the prompt and the default negative prompt are encoded, then the call goes on to its own argument checks
    t2to = LongVGenCogVideoXPipeline(m, sched, text_encoder=enc, tokenizer=tok)
    enc.calls.clear()
    with pytest.raises(ValueError, match="longvgen_mean, longvgen_std and longvgen_pca are required"):
        t2to(prompt="a cat", max_sequence_length=12, height=8, width=12, num_frames_per_chunk=4)
    assert [c.shape for c in enc.calls] == [(1, 12), (1, 12)] and enc.calls[1][0].tolist() == [1] + [0] * 11
