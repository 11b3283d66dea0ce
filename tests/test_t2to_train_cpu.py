"""CPU: host-side facts of the T2To training step (tokensgen_amd/train_t2to.py; train_cogvideo_t2to.py with cogvideo_5b_vaevip_4x8x12_t2to.yaml):
the attention-mask key mismatch that leaves every block unmasked, the loss masks and their per-item normalisation, the trainable set, and the
arena order (To2V names keep theirs; T2To to_q / to_k / to_v adjacent, the fused QKV weight a view)."""
import os
import re

import pytest
import torch

# the reference's training loop and model sources, when a checkout is named (they are not part of this repository)
REF = os.environ.get("TOKENSGEN_REFERENCE_ROOT", "")

CFG = dict(num_attention_heads=2, attention_head_dim=64, num_layers=3, patch_size=1, time_embed_dim=128, text_embed_dim=64, in_channels=16,
           out_channels=16)


def _read(rel):
    p = os.path.join(REF, rel)
    if not REF or not os.path.exists(p):
        pytest.skip("reference sources not available (set TOKENSGEN_REFERENCE_ROOT)")
    return open(p).read()


def test_reference_passes_attention_mask_but_the_model_pops_attention_masks():
    """T1 (issue item 3): the loop hands its masks over as attention_kwargs={"attention_mask": ...} while the transformer pops "attention_masks"
    (plural): no mask reaches a block, so the T2To trainer runs unmasked attention."""
    loop = _read("train_cogvideo_t2to.py")
    model = _read(os.path.join("longvgen", "models", "cogvideox_transformer_3d.py"))
    passed = set(re.findall(r'attention_kwargs\s*=\s*\{\s*"([a-z_]+)"\s*:', loop))
    popped = set(re.findall(r'attention_kwargs\.pop\(\s*"(attention_masks?)"', model))
    assert passed == {"attention_mask"}, passed
    assert popped == {"attention_masks"}, popped
    assert not passed & popped


def _loss_masks(shape, valid):
    """prepare_loss_masks (train_cogvideo_t2to.py:1098-1108) restated."""
    m = torch.zeros(shape)
    for b, v in enumerate(valid):
        m[b, :v] = 1
    return m


def test_loss_masks_and_per_item_normalisation():
    """:2125-2166: loss_b = sum(w_b (|pred - x0| * mask)^2) / sum(mask) is the mean over item b's VALID frames only (normalised by valid_b * E, not
    F * E), padded frames carry no gradient, and the bf16 mask sums of the yaml's shapes are exact (valid * 4 frames of 16 x 8 x 12 elements)."""
    g = torch.Generator().manual_seed(0)
    B, F, E = 3, 12, 16 * 8 * 12
    valid = [4, 8, 12]
    pred = torch.randn(B, F, 16, 8, 12, generator=g, dtype=torch.float64, requires_grad=True)
    x0 = torch.randn(B, F, 16, 8, 12, generator=g, dtype=torch.float64)
    w = torch.tensor([1.5, 2.0, 7.0], dtype=torch.float64).view(B, 1, 1, 1, 1)
    mask = _loss_masks(pred.shape, valid).double()
    loss_b = torch.sum((w * (torch.abs(pred - x0) * mask) ** 2).reshape(B, -1), dim=1) / torch.sum(mask.reshape(B, -1), dim=1)
    for b in range(B):
        want = (w[b] * (pred[b, :valid[b]] - x0[b, :valid[b]]) ** 2).sum() / (valid[b] * E)
        assert torch.allclose(loss_b[b], want, rtol=1e-12)
    loss_b.mean().backward()
    for b in range(B):
        assert bool((pred.grad[b, valid[b]:] == 0).all())
        want = 2 * w[b] * (pred[b, :valid[b]] - x0[b, :valid[b]]) / (valid[b] * E * B)
        assert torch.allclose(pred.grad[b, :valid[b]], want, rtol=1e-12)
    # the reference sums a bf16 mask: exact for every count the yaml allows (1..24 chunks x 4 frames x 1536 elements = 3 * 2^11 * chunks)
    for chunks in range(1, 25):
        m = torch.ones(chunks * 4 * E, dtype=torch.bfloat16)
        assert float(m.sum()) == chunks * 4 * E


def test_trainable_set_and_arena_order():
    """T1: every name but patch_embed.proj trains (:1531-1560); T2To's arena order puts to_q / to_k / to_v (weights, then biases) adjacent in
    every block and follows the backward (final layers, blocks last first, embeddings); optim.arena_order is untouched for the To2V names."""
    from oracle import dit_ref as O
    from tokensgen_amd import optim
    from tokensgen_amd.train_t2to import T2ToBlockTrainer, T2ToTrainer, t2to_arena_order, trainable_names
    sd = O.make_state_dict(CFG, seed=1)
    names = trainable_names(sd)
    assert "patch_embed.proj.weight" not in names and "patch_embed.proj.bias" not in names
    assert set(sd) - set(names) == {"patch_embed.proj.weight", "patch_embed.proj.bias"}
    assert "patch_embed.text_proj.weight" in names and "time_embedding.linear_1.weight" in names
    order = t2to_arena_order(names, CFG["num_layers"])
    assert sorted(order) == names
    assert [n.split(".")[0] for n in order[:6]] == ["norm_final", "norm_final", "norm_out", "norm_out", "norm_out", "norm_out"]
    assert order[-6:] == sorted(n for n in names if n.startswith(("patch_embed.", "time_embedding.")))
    blocks = [int(n.split(".")[1]) for n in order if n.startswith("transformer_blocks.")]
    assert blocks == sorted(blocks, reverse=True)
    for i in range(CFG["num_layers"]):
        k = order.index(f"transformer_blocks.{i}.attn1.to_q.weight")
        assert order[k:k + 6] == [f"transformer_blocks.{i}.attn1.to_{n}.{p}" for p in ("weight", "bias") for n in "qkv"]
    # the arena: the fused QKV weight and bias of every block are views of it; the frozen patch embedding stays outside
    arena = optim.ParamArena({n: sd[n].to(torch.bfloat16) for n in names}, order, "cpu", moments=False)
    sd2 = {k: v.to(torch.bfloat16) for k, v in sd.items()}
    tr = T2ToTrainer(sd2, CFG["num_attention_heads"], CFG["num_layers"])
    assert tr.trainable == names
    tr.use_arena(arena)
    for i in range(CFG["num_layers"]):
        blk = T2ToBlockTrainer(sd2, f"transformer_blocks.{i}", CFG["num_attention_heads"], 9)
        assert blk.fused_is_view
        assert blk.Wqkv.data_ptr() == arena.views[f"transformer_blocks.{i}.attn1.to_q.weight"].data_ptr() and blk.Wqkv.shape == (3 * 128, 128)
    with pytest.raises(ValueError, match="not adjacent"):
        bad = optim.ParamArena({n: sd[n].to(torch.bfloat16) for n in names}, sorted(names), "cpu", moments=False)
        T2ToTrainer({k: v.to(torch.bfloat16) for k, v in sd.items()}, CFG["num_attention_heads"], CFG["num_layers"]).use_arena(bad)
    # To2V: the vip names keep exactly the order they had (vip_to_{q,k,v} leading each block, embeddings, then the Resampler)
    sdv = O.make_state_dict(dict(CFG, patch_size=2), n_vip_dim=128, seed=2)
    vip = sorted(k for k in sdv if "vip_" in k) + ["resampler.latents", "resampler.proj_in.weight"]
    got = optim.arena_order(vip, CFG["num_layers"])
    want = []
    for i in reversed(range(CFG["num_layers"])):
        pre = f"transformer_blocks.{i}.attn1.processor."
        lead = [pre + f"vip_to_{n}.{p}" for p in ("weight", "bias") for n in "qkv"]
        want += lead + sorted(n for n in vip if n.startswith(f"transformer_blocks.{i}.") and n not in lead)
    want += ["patch_embed.vip_proj.bias", "patch_embed.vip_proj.weight", "resampler.latents", "resampler.proj_in.weight"]
    assert got == want


def test_t2to_rope_split_52_6_6():
    """:2068-2091: the token grid's RoPE has 52 temporal, 6 height and 6 width channels over positions 0..F-1, 0..7, 0..11."""
    import numpy as np
    from oracle import dit_ref as O
    from tokensgen_amd.train_t2to import t2to_rope
    cos, sin = t2to_rope(5)
    assert cos.shape == sin.shape == (5 * 8 * 12, 64)
    f32 = np.float32
    rc, rs = O.rope_3d(64, np.arange(5, dtype=f32), np.arange(8, dtype=f32), np.arange(12, dtype=f32), dim_t=52, dim_h=6, dim_w=6)
    assert torch.equal(cos, rc) and torch.equal(sin, rs)
    # frame f, row h, column w: the temporal channels depend on f only, the last 12 on (h, w) only
    c = cos.view(5, 8, 12, 64)
    assert torch.equal(c[2, 0, 0, :52], c[2, 7, 11, :52]) and torch.equal(c[0, 3, 4, 52:], c[4, 3, 4, 52:])
