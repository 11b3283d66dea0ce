"""Host side of LoRA (tokensgen_amd/lora.py, optim.arena_order with adapter names) against tests/lora_ref.py: no GPU needed."""
import math

import pytest
import torch

import lora_ref as R

BF = torch.bfloat16
CFG = dict(num_attention_heads=2, attention_head_dim=64, num_layers=2, patch_size=2, time_embed_dim=128, text_embed_dim=64, in_channels=16, out_channels=16)
YAML = dict(rank=128, lora_alpha=64, target_modules=["to_k", "to_q", "to_v", "to_out.0"])


def _sd():
    from oracle import dit_ref as O
    return O.make_state_dict(CFG, n_vip_dim=128, seed=5)


def test_target_matching_on_the_real_key_list():
    from tokensgen_amd import lora
    cfg = lora.LoraConfig.from_params(YAML)
    sd = _sd()
    mods = lora.target_modules(cfg, sd.keys())
    assert mods == R.target_modules(sd.keys())
    assert len(mods) == 4 * CFG["num_layers"]
    assert not any("vip_to_" in m for m in mods) and all(".attn1." in m and ".processor." not in m for m in mods)
    assert sorted(m.split(".attn1.")[1] for m in mods if m.startswith("transformer_blocks.0.")) == ["to_k", "to_out.0", "to_q", "to_v"]
    for name in sd:                                        # module by module, the product's rule is the restated peft rule
        mod = name.rsplit(".", 1)[0]
        assert cfg.match(mod) == R.matches(mod), mod
    assert not cfg.match("transformer_blocks.0.attn1.processor.vip_to_q") and not cfg.match("xto_q") and cfg.match("to_q")
    assert cfg.scaling == R.scaling(128, 64) == 0.5
    assert lora.LoraConfig.from_params(dict(YAML, is_trainable=False)).is_trainable is False and cfg.is_trainable is True


def test_init_adapter_is_peft_default_init_and_seeded():
    from tokensgen_amd import lora
    cfg = lora.LoraConfig.from_params(YAML)
    sd = _sd()
    a1 = lora.init_adapter(cfg, sd, torch.Generator().manual_seed(7), dtype=torch.float32)
    a2 = lora.init_adapter(cfg, sd, torch.Generator().manual_seed(7), dtype=torch.float32)
    a3 = lora.init_adapter(cfg, sd, torch.Generator().manual_seed(8), dtype=torch.float32)
    from_cfg = lora.init_adapter(cfg, CFG, torch.Generator().manual_seed(7), dtype=torch.float32)
    assert sorted(a1) == sorted(R.key(m, h, False) for m in R.target_modules(sd.keys()) for h in "AB") == sorted(from_cfg)
    D = 128
    for k, v in a1.items():
        assert torch.equal(v, a2[k]) and torch.equal(v, from_cfg[k])
        if k.endswith("lora_B.weight"):
            assert v.shape == (D, 128) and not v.any()
        else:
            assert v.shape == (128, D) and v.abs().max().item() <= R.init_bound(D) and math.isclose(R.init_bound(D), 1 / math.sqrt(D), rel_tol=1e-12)
            assert v.abs().max().item() > 0.9 * R.init_bound(D) and abs(v.mean().item()) < 0.05 * R.init_bound(D)     # uniform over the whole interval
            assert not torch.equal(v, a3[k])
    assert all(v.dtype == BF for v in lora.init_adapter(cfg, sd, torch.Generator().manual_seed(7)).values())


def test_save_load_round_trip_and_refusals(tmp_path):
    from safetensors.torch import load_file, save_file
    from tokensgen_amd import lora
    cfg = lora.LoraConfig.from_params(YAML)
    ad = R.random_adapter(_sd(), 128, seed=9)
    fn = lora.save_lora_weights(str(tmp_path / "a"), ad)
    assert fn.endswith("pytorch_lora_weights.safetensors")
    raw = load_file(fn)
    assert sorted(raw) == sorted(R.PREFIX + k for k in ad)                       # the diffusers layout: `transformer.` in front of the model's names
    assert "transformer.transformer_blocks.1.attn1.to_out.0.lora_B.weight" in raw
    back = lora.load_lora_weights(str(tmp_path / "a"), cfg)
    assert sorted(back) == sorted(ad) and all(torch.equal(back[k], ad[k]) and back[k].dtype == BF for k in ad)
    save_file({k: v for k, v in ad.items()}, str(tmp_path / "bare.safetensors"))   # without the prefix
    bare = lora.load_lora_weights(str(tmp_path / "bare.safetensors"), cfg)
    assert all(torch.equal(bare[k], ad[k]) for k in ad)
    with_prefix = lora.save_lora_weights(str(tmp_path / "b"), {R.PREFIX + k: v for k, v in ad.items()})
    assert sorted(load_file(with_prefix)) == sorted(raw)
    # wrong rank: named
    bad = dict(ad)
    kb = "transformer_blocks.0.attn1.to_q.lora_B.weight"
    bad[kb] = bad[kb][:, :64].contiguous()
    save_file(bad, str(tmp_path / "rank.safetensors"))
    with pytest.raises(ValueError, match=r"transformer_blocks\.0\.attn1\.to_q\.lora_"):
        lora.load_lora_weights(str(tmp_path / "rank.safetensors"), cfg)
    with pytest.raises(ValueError, match="rank 128.*says 64|rank"):
        lora.load_lora_weights(fn, lora.LoraConfig(rank=64))
    # a missing half: named
    half = {k: v for k, v in ad.items() if k != "transformer_blocks.1.attn1.to_v.lora_A.weight"}
    save_file(half, str(tmp_path / "half.safetensors"))
    with pytest.raises(ValueError, match=r"transformer_blocks\.1\.attn1\.to_v\.lora_A\.weight"):
        lora.load_lora_weights(str(tmp_path / "half.safetensors"), cfg)
    with pytest.raises(ValueError, match="lora_path"):
        lora.apply_from_config(None, dict(use_lora=True, lora_path="", lora_params=YAML))
    assert lora.apply_from_config(None, dict(use_lora=False, lora_path="x")) is False


def test_reference_arithmetic_of_the_restated_lora_linear():
    """lora_ref itself: the adapted linear == the linear on the merged weight (float64), and a fresh adapter (B = 0) changes nothing."""
    g = torch.Generator().manual_seed(3)
    x, W, b = torch.randn(5, 16, generator=g, dtype=torch.float64), torch.randn(8, 16, generator=g, dtype=torch.float64), torch.randn(8, generator=g, dtype=torch.float64)
    A, B = torch.randn(4, 16, generator=g, dtype=torch.float64), torch.randn(8, 4, generator=g, dtype=torch.float64)
    y = R.lora_linear(x, W, b, A, B, 0.5)
    assert torch.allclose(y, torch.nn.functional.linear(x, R.merged_weight(W, A, B, 0.5), b), rtol=1e-12, atol=1e-12)
    assert torch.equal(R.lora_linear(x, W, b, A, torch.zeros_like(B), 0.5), torch.nn.functional.linear(x, W, b))


def test_arena_order_with_lora_names():
    from tokensgen_amd import lora, optim
    cfg = lora.LoraConfig.from_params(YAML)
    sd = _sd()
    names = sorted([k for k in sd if "vip_" in k] + list(lora.init_adapter(cfg, sd, torch.Generator().manual_seed(1))))
    order = optim.arena_order(names, CFG["num_layers"])
    assert sorted(order) == names and len(set(order)) == len(order)
    # block-local: all of block 1, then all of block 0, then the rest
    blk = [int(n.split(".")[1]) if n.startswith("transformer_blocks.") else -1 for n in order]
    assert blk == sorted(blk, reverse=True)
    for i in range(CFG["num_layers"]):
        for group in ([f"transformer_blocks.{i}.attn1.processor.vip_to_{n}.weight" for n in "qkv"],
                      [f"transformer_blocks.{i}.attn1.processor.vip_to_{n}.bias" for n in "qkv"],
                      [f"transformer_blocks.{i}.attn1.to_{n}.lora_A.weight" for n in "qkv"]):
            at = [order.index(n) for n in group]
            assert at == [at[0], at[0] + 1, at[0] + 2], group
    # without adapter names the order is what it was
    vip_only = [k for k in sd if "vip_" in k]
    assert optim.arena_order(vip_only, 2) == [n for n in order if ".lora_" not in n]


def test_param_arena_and_get_optimizer_accept_the_enlarged_name_set():
    from tokensgen_amd import lora, optim
    cfg = lora.LoraConfig.from_params(YAML)
    sd = {k: v.to(BF) for k, v in _sd().items()}
    ad = lora.init_adapter(cfg, sd, torch.Generator().manual_seed(2))
    params = {k: v for k, v in sd.items() if "vip_" in k}
    params.update(ad)
    order = optim.arena_order(sorted(params), CFG["num_layers"])
    arena = optim.ParamArena(params, order, "cpu", moments=False)
    for k, v in params.items():
        assert torch.equal(arena.views[k], v) and arena.grad_view(k).shape == v.shape
    a3 = [arena.views[f"transformer_blocks.0.attn1.to_{n}.lora_A.weight"] for n in "qkv"]
    assert a3[1].data_ptr() == a3[0].data_ptr() + a3[0].numel() * 2 and a3[2].data_ptr() == a3[1].data_ptr() + a3[1].numel() * 2
    rows, n_absmax, n_small = optim.block_table(arena)
    assert [r.name for r in rows] == order and n_absmax > 0
    assert arena.prefix_elems(lambda n: not n.startswith("resampler.")) == arena.numel
    for use8 in (False, True):
        ar = optim.ParamArena(params, order, "cpu", moments=not use8)
        opt = optim.get_optimizer(ar, dict(optimizer="adamw", use_8bit_adam=use8, learning_rate=1e-4))
        assert type(opt).__name__ == ("AdamW8bit" if use8 else "AdamW") and opt.clip_elems == ar.numel
