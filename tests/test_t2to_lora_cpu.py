"""CPU: the T2To trainer's trainable-set selection (tokensgen_amd/train_t2to.py `trainable_names`; train_cogvideo_t2to.py:1531-1557 with the yaml keys
`transformer_trainable_modules`, `use_lora`, `lora_params`) against a hand-written table, and the arena order of a reduced set.  The names are those of the
tiny T2To model of tests/golden/t2to_tiny.pt (its configuration and weight seed; the oracle's make_state_dict builds the state dict from them)."""
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGETS = ("to_q", "to_k", "to_v", "to_out.0")


@pytest.fixture(scope="module")
def tiny():
    from oracle import dit_ref as O
    from tokensgen_amd import lora
    g = torch.load(os.path.join(ROOT, "tests", "golden", "t2to_tiny.pt"))
    cfg = g["cfg"]
    assert cfg["patch_size"] == 1
    sd = {k: v.to(torch.bfloat16) for k, v in O.make_state_dict(cfg, None, seed=g["weight_seed"]).items()}
    ad = lora.init_adapter(lora.LoraConfig(rank=128, lora_alpha=64), sd, torch.Generator().manual_seed(1))
    return cfg, sd, ad


def _block(i, *names):
    return [f"transformer_blocks.{i}.{n}" for n in names]


# the 24 parameters of a plain CogVideoXBlock, written out by hand (cogvideox_transformer_3d.py:221-332)
ATTN1 = ["attn1.norm_k.bias", "attn1.norm_k.weight", "attn1.norm_q.bias", "attn1.norm_q.weight", "attn1.to_k.bias", "attn1.to_k.weight",
         "attn1.to_out.0.bias", "attn1.to_out.0.weight", "attn1.to_q.bias", "attn1.to_q.weight", "attn1.to_v.bias", "attn1.to_v.weight"]
FF = ["ff.net.0.proj.bias", "ff.net.0.proj.weight", "ff.net.2.bias", "ff.net.2.weight"]
NORMS = ["norm1.linear.bias", "norm1.linear.weight", "norm1.norm.bias", "norm1.norm.weight",
         "norm2.linear.bias", "norm2.linear.weight", "norm2.norm.bias", "norm2.norm.weight"]
QK_NORMS = ["attn1.norm_k.bias", "attn1.norm_k.weight", "attn1.norm_q.bias", "attn1.norm_q.weight"]
OUTSIDE = ["norm_final.bias", "norm_final.weight", "norm_out.linear.bias", "norm_out.linear.weight", "norm_out.norm.bias", "norm_out.norm.weight",
           "patch_embed.text_proj.bias", "patch_embed.text_proj.weight", "proj_out.bias", "proj_out.weight",
           "time_embedding.linear_1.bias", "time_embedding.linear_1.weight", "time_embedding.linear_2.bias", "time_embedding.linear_2.weight"]
FROZEN_ALWAYS = ["patch_embed.proj.bias", "patch_embed.proj.weight"]
ADAPTER = [f"attn1.{t}.lora_{h}.weight" for t in TARGETS for h in "AB"]


def _table(layers, modules, lora_state):
    """The expected set, by the three rules read off :1531-1557.  lora_state: None (no adapter), "trainable" or "frozen"."""
    per_block, outside = [], []
    if modules == ["all"]:
        per_block, outside = ATTN1 + FF + NORMS, list(OUTSIDE)                  # all but patch_embed.proj
        if lora_state is not None:
            per_block = per_block + ADAPTER                                     # "all": a name without patch_embed.proj — the adapter's too
    elif modules == ["attn1"]:
        per_block = list(ATTN1)
        if lora_state is not None:
            per_block = per_block + ADAPTER                                     # "attn1" occurs in attn1.to_q.lora_A.weight
    elif modules == ["ff", "norm"]:
        # "norm" occurs in norm1 / norm2, attn1.norm_q / norm_k, norm_final, norm_out; "ff" in ff.net.*
        per_block, outside = FF + NORMS + QK_NORMS, [n for n in OUTSIDE if n.startswith(("norm_final", "norm_out"))]
        if lora_state == "trainable":
            per_block = per_block + ADAPTER
    else:
        assert modules == []
        if lora_state == "trainable":
            per_block = list(ADAPTER)
    return sorted(outside + [n for i in range(layers) for n in _block(i, *per_block)])


@pytest.mark.parametrize("lora_state", [None, "trainable", "frozen"])
@pytest.mark.parametrize("modules", [["all"], [], ["attn1"], ["ff", "norm"]])
def test_trainable_names_against_the_hand_written_table(tiny, modules, lora_state):
    from tokensgen_amd import lora
    from tokensgen_amd.train_t2to import trainable_names
    cfg, sd, ad = tiny
    L_ = cfg["num_layers"]
    assert sorted(sd) == sorted(OUTSIDE + FROZEN_ALWAYS + [n for i in range(L_) for n in _block(i, *(ATTN1 + FF + NORMS))])      # the table covers the model
    assert sorted(ad) == sorted(n for i in range(L_) for n in _block(i, *ADAPTER))
    lcfg = None if lora_state is None else lora.LoraConfig(rank=128, lora_alpha=64, is_trainable=lora_state == "trainable")
    names = dict(sd, **ad) if lora_state is not None else sd
    got = trainable_names(names, modules, lcfg)
    assert got == _table(L_, modules, lora_state)
    assert not any("patch_embed.proj" in n for n in got)
    # a state dict that carries adapter entries without a LoraConfig: they are not parameters of the model
    assert trainable_names(dict(sd, **ad), modules, None) == _table(L_, modules, None)


def test_default_call_reproduces_the_full_fine_tuning_list(tiny):
    from tokensgen_amd.train_t2to import T2ToTrainer, trainable_names
    cfg, sd, _ = tiny
    want = sorted(n for n in sd if "patch_embed.proj" not in n)              # what trainable_names returned before it took arguments
    assert trainable_names(sd) == want == trainable_names(sd, ("all",), None)
    tr = T2ToTrainer(dict(sd), cfg["num_attention_heads"], cfg["num_layers"])
    assert tr.trainable == want and tr.lora is None and tr.lora_keys == [] and tr._block_trainable is None


def test_a_lora_target_subset_selects_only_its_tensors(tiny):
    from tokensgen_amd import lora
    from tokensgen_amd.train_t2to import trainable_names
    cfg, sd, ad = tiny
    lcfg = lora.LoraConfig(rank=128, lora_alpha=64, target_modules=("to_out.0",))
    got = trainable_names(dict(sd, **ad), [], lcfg)
    assert got == sorted(n for i in range(cfg["num_layers"]) for n in _block(i, "attn1.to_out.0.lora_A.weight", "attn1.to_out.0.lora_B.weight"))


@pytest.mark.parametrize("modules,lora_state", [([], "trainable"), (["attn1"], None), (["attn1"], "trainable"), (["ff", "norm"], "trainable"), (["to_q"], None)])
def test_arena_order_of_a_reduced_set(tiny, modules, lora_state):
    """A permutation of the set, in backward order (final layers, blocks last first, embeddings), with q | k | v (weights, then biases) adjacent when present and
    the three lora_A of q | k | v side by side."""
    from tokensgen_amd import lora
    from tokensgen_amd.train_t2to import t2to_arena_order, trainable_names
    cfg, sd, ad = tiny
    L_ = cfg["num_layers"]
    lcfg = None if lora_state is None else lora.LoraConfig(rank=128, lora_alpha=64)
    names = trainable_names(dict(sd, **ad), modules, lcfg)
    order = t2to_arena_order(names, L_)
    assert sorted(order) == names and len(set(order)) == len(order)
    blocks = [int(n.split(".")[1]) for n in order if n.startswith("transformer_blocks.")]
    assert blocks == sorted(blocks, reverse=True)
    first_block = min(i for i, n in enumerate(order) if n.startswith("transformer_blocks."))
    assert all(n.startswith(("norm_final", "norm_out", "proj_out")) for n in order[:first_block])
    for i in range(L_):
        qkv = [n for n in _block(i, *[f"attn1.to_{c}.{p}" for p in ("weight", "bias") for c in "qkv"]) if n in names]
        if qkv:
            k = order.index(qkv[0])
            assert order[k:k + len(qkv)] == qkv
        la = _block(i, *[f"attn1.to_{c}.lora_A.weight" for c in "qkv"])
        if la[0] in names:
            k = order.index(la[0])
            assert order[k:k + 3] == la


def test_adapter_only_arena_holds_the_adapter_and_the_fused_projections_are_views_or_frozen_copies(tiny):
    """make_arena on `trainable_modules=[]` + a trainable adapter: the arena is the adapter alone, the [3r, D] down-projection of every block is a VIEW of it, the frozen
    fused QKV weight is a copy made once (nothing checks its adjacency), and a full arena still insists on adjacent q | k | v."""
    from tokensgen_amd import lora, optim
    from tokensgen_amd.train_t2to import T2ToTrainer, t2to_arena_order
    cfg, sd, ad = tiny
    H, L_ = cfg["num_attention_heads"], cfg["num_layers"]
    lcfg = lora.LoraConfig(rank=128, lora_alpha=64)
    full = dict(sd, **ad)
    tr = T2ToTrainer(full, H, L_, trainable_modules=[], lora=lcfg)
    assert tr.trainable == sorted(ad) == tr.lora_keys
    arena = optim.ParamArena({n: full[n] for n in tr.trainable}, t2to_arena_order(tr.trainable, L_), "cpu", moments=False)
    tr.use_arena(arena)
    assert arena.numel == sum(v.numel() for v in ad.values())
    for i in range(L_):
        blk = tr._block(i, 9)
        assert not blk.fused_is_view and not any(blk.qkv_trains) and blk.lora_qkv and blk.lora_out
        assert blk.lA3_is_view and blk.lA3.data_ptr() == arena.views[f"transformer_blocks.{i}.attn1.to_q.lora_A.weight"].data_ptr()
        assert blk.lA3.shape == (3 * 128, H * 64)
    # restrictions are refused by name
    with pytest.raises(NotImplementedError, match="multiple of 128"):
        T2ToTrainer(dict(sd, **lora.init_adapter(lora.LoraConfig(rank=64), sd)), H, L_, trainable_modules=[], lora=lora.LoraConfig(rank=64))
    part = {k: v for k, v in ad.items() if ".to_v." not in k}
    with pytest.raises(NotImplementedError, match="as a group"):
        T2ToTrainer(dict(sd, **part), H, L_, trainable_modules=[], lora=lcfg)._block(0, 9)
    ff = lora.LoraConfig(rank=128, target_modules=("ff.net.2",))
    with pytest.raises(NotImplementedError, match="attn1"):
        T2ToTrainer(dict(sd, **lora.init_adapter(ff, sd)), H, L_, trainable_modules=[], lora=ff)
    with pytest.raises(ValueError, match="empty"):
        from tokensgen_amd.train_t2to import make_arena
        make_arena(T2ToTrainer(dict(sd), H, L_, trainable_modules=[]), dict(optimizer="adamw"))
