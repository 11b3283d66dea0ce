"""GPU: the T2To training step (tokensgen_amd/train_t2to.py; train_cogvideo_t2to.py:1961-2175 with cogvideo_5b_vaevip_4x8x12_t2to.yaml): full
fine-tuning of the plain, patch-1 CogVideoX DiT on the gfx950 kernels against torch.autograd through the fp32 oracle (oracle/dit_ref.py with
n_vip = 0), run on the GPU from the same bf16-rounded weights and inputs.  The masked loss is restated here from :2125-2166."""
import math
import subprocess
import sys
import os

import numpy as np
import pytest
import torch
from conftest import measured

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return measured(((a - b).norm() / (b.norm() + 1e-12)).item())


def _rand(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF)


def _cfg(heads, layers):
    return dict(num_attention_heads=heads, attention_head_dim=64, num_layers=layers, patch_size=1, time_embed_dim=128, text_embed_dim=64,
                in_channels=16, out_channels=16)


def _rope(frames, h, w):
    from oracle import dit_ref as O
    return O.rope_3d(64, np.arange(frames, dtype=f32), np.arange(h, dtype=f32), np.arange(w, dtype=f32), dim_t=52, dim_h=6, dim_w=6)


def _acp():
    from oracle import scheduler_ref as S
    _, ac = S.alphas_cumprod()
    return torch.as_tensor(ac, dtype=torch.float32)


def masked_loss_ref(acp, model_output, noisy, x0, timesteps, valid_frames):
    """train_cogvideo_t2to.py:2125-2166 (norm "pca", use_per_timestep_weight) with prepare_loss_masks (:1098-1108), on whatever dtype the inputs
    carry (get_velocity in the sample dtype, the weights in the table's).  Returns (loss, per-item losses)."""
    from oracle import train_ref as T
    B = model_output.shape[0]
    pred = T.get_velocity(acp.to(model_output.device), model_output, noisy, timesteps)
    w = 1 / (1 - acp.to(model_output.device)[timesteps])
    while w.dim() < pred.dim():
        w = w.unsqueeze(-1)
    mask = torch.zeros_like(pred)
    for b, v in enumerate(valid_frames):
        mask[b, :v] = 1
    loss = torch.sum((w * (torch.abs(pred - x0) * mask) ** 2).reshape(B, -1), dim=1) / torch.sum(mask.reshape(B, -1), dim=1)
    return loss.mean(), loss


def _key_padding_sdpa(valid_tokens):
    """F.scaled_dot_product_attention with the prefix-valid key mask of every item (text + the valid frames): what a masked recipe would run."""
    sdpa = torch.nn.functional.scaled_dot_product_attention

    def masked(q, k, v, attn_mask=None, **kw):
        n = k.shape[-2]
        m = torch.zeros(len(valid_tokens), 1, 1, n, dtype=torch.bool, device=q.device)
        for b, t in enumerate(valid_tokens):
            m[b, ..., :t] = True
        return sdpa(q, k, v, attn_mask=m)
    return masked


# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_t2to_block_backward_vs_autograd_of_the_oracle_block(parity):
    """G1: one plain block (4 heads x 64, 2 frames of 8 x 12 + 226 text tokens, B = 2): the gradient of every block parameter, of both block
    inputs and of the modulation input (-> time embedding) against fp32 autograd through oracle.dit_ref.block_forward(n_vip=0)."""
    from oracle import dit_ref as O
    from tokensgen_amd.train_t2to import T2ToBlockTrainer
    B, H, Nt, Fr, h, w = 2, 4, 226, 2, 8, 12
    Nv, D = Fr * h * w, H * 64
    pre = "transformer_blocks.0"
    sd = {k: v.to(BF).float().to(DEV) for k, v in O.make_state_dict(_cfg(H, 1), seed=11, std=0.08).items() if k.startswith(pre + ".")}
    assert len(sd) == 24
    for k in sd:
        sd[k].requires_grad_(True)
    hidden, enc, temb = _rand(B, Nv, D, seed=12), _rand(B, Nt, D, seed=13), _rand(B, 128, seed=14)
    rope = tuple(t.to(DEV) for t in _rope(Fr, h, w))
    hf, ef, tf = (t.float().to(DEV).requires_grad_(True) for t in (hidden, enc, temb))
    with torch.device(DEV):
        oh, oe = O.block_forward(sd, pre, hf, ef, tf[:, None], H, 0, None, rope, None, None)
    Gh, Ge = _rand(B, Nv, D, seed=15), _rand(B, Nt, D, seed=16)
    ((oh * Gh.float().to(DEV)).sum() + (oe * Ge.float().to(DEV)).sum()).backward()
    sd_dev = {k: v.detach().to(BF).contiguous() for k, v in sd.items()}
    blk = T2ToBlockTrainer(sd_dev, pre, H, Nt)
    gh, ge = blk.forward(hidden.to(DEV), enc.to(DEV), temb.to(DEV), rope)
    # tolerances = 2x the values measured on MI355X (3.9e-3 / 3.9e-3 / 4.2e-3 / 4.3e-3 / 5.4e-3 / 1.4e-2, the worst tensor attn1.to_k.bias)
    parity(_rel(gh, oh.detach()), 8e-3, "block output (video rows)")
    parity(_rel(ge, oe.detach()), 8e-3, "block output (text rows)")
    grads, dh, de = blk.backward(Gh.to(DEV), Ge.to(DEV))
    assert set(pre + "." + k for k in grads) == set(sd)
    parity(_rel(dh, hf.grad), 8.5e-3, "d hidden")
    parity(_rel(de, ef.grad), 8.6e-3, "d text")
    from tokensgen_amd.train_t2to import _silu_grad
    parity(_rel(blk.d_emb * _silu_grad(temb.to(DEV)), tf.grad), 1.1e-2, "d temb")
    worst = max((float(_rel(g_, sd[pre + "." + name].grad)), name) for name, g_ in grads.items())
    parity(worst[0], 2.9e-2, f"worst block parameter ({worst[1]})")


def _model_case(seed, B=3, H=2, layers=2, Nt=226, Fr=12, h=8, w=12):
    from oracle import dit_ref as O
    cfg = _cfg(H, layers)
    sd = {k: v.to(BF).float() for k, v in O.make_state_dict(cfg, seed=seed, std=0.08).items()}
    g = torch.Generator().manual_seed(seed + 1)
    x0, noise = (torch.randn(B, Fr, 16, h, w, generator=g).to(BF) for _ in range(2))
    text = _rand(B, Nt, 64, seed=seed + 2)
    ts = torch.tensor([37, 512, 901])[:B]
    return cfg, sd, x0, noise, text, ts


def _oracle_grads(cfg, sd, noisy, x0, text, ts, rope, valid_frames, acp, key_mask_tokens=None, monkeypatch=None):
    """fp32 autograd of the oracle model + the restated masked loss on the GPU; optionally with the prefix-valid key mask in every attention."""
    from oracle import dit_ref as O
    from tokensgen_amd.train_t2to import trainable_names
    p = {k: v.to(DEV).clone().requires_grad_(k in trainable_names(sd)) for k, v in sd.items()}
    if key_mask_tokens is not None:
        monkeypatch.setattr(torch.nn.functional, "scaled_dot_product_attention", _key_padding_sdpa(key_mask_tokens))
    try:
        with torch.device(DEV):         # the oracle's own small tables (timestep frequencies) on the same device
            out = O.dit_forward(p, cfg, noisy.float().to(DEV), text.float().to(DEV), ts.to(DEV), None, tuple(t.to(DEV) for t in rope))
    finally:
        if key_mask_tokens is not None:
            monkeypatch.undo()
    loss, per_item = masked_loss_ref(acp, out, noisy.float().to(DEV), x0.float().to(DEV), ts.to(DEV), valid_frames)
    loss.backward()
    return loss.detach(), {k: v.grad for k, v in p.items() if v.grad is not None}, p


def _flat(gr, names):
    return torch.cat([gr[n].float().reshape(-1).cpu() for n in names])


def test_t2to_model_masked_loss_and_every_trainable_gradient_vs_the_oracle(parity, monkeypatch):
    """G2: 2 layers, B = 3, valid_num_chunks = (1, 2, 3) of 3 (4 frames per chunk): the masked loss and EVERY trainable gradient against the oracle
    run the way the reference runs (unmasked attention); patch_embed.proj receives none.  The gradients are clearly farther from an oracle run WITH
    the prefix-valid attention mask: the padded frames enter attention (issue item 3)."""
    from tokensgen_amd.train_t2to import T2ToTrainer, trainable_names, vpred_loss_and_grad_masked
    from oracle import train_ref as T
    cfg, sd, x0, noise, text, ts = _model_case(21)
    B, Fr, h, w, Nt = 3, 12, 8, 12, 226
    acp = _acp()
    valid = [c * 4 for c in (1, 2, 3)]
    # padded frames hold what padding holds: the same latent in every token (a fixed per-channel vector; the noise stays Gaussian).  They take part
    # in attention like any other token
    pad = (torch.randn(16, generator=torch.Generator().manual_seed(22)) * 2).to(BF)
    for b, v in enumerate(valid):
        x0[b, v:] = pad[:, None, None]
    noisy = T.add_noise(acp, x0, noise, ts)
    rope = _rope(Fr, h, w)
    loss_ref, g_ref, _ = _oracle_grads(cfg, sd, noisy, x0, text, ts, rope, valid, acp)
    names = trainable_names(sd)
    assert set(g_ref) == set(names)
    sd_dev = {k: v.to(BF).to(DEV).contiguous() for k, v in sd.items()}
    tr = T2ToTrainer(sd_dev, 2, 2)
    out = tr.forward(noisy.to(DEV), text.to(DEV), ts, rope)
    loss, per_item, d_out = vpred_loss_and_grad_masked(out, noisy.to(DEV), x0.to(DEV), ts, acp, valid)
    # tolerances = 2x the values measured on MI355X (3.8e-3 / 2.5e-2, the worst tensor transformer_blocks.1.attn1.norm_k.bias / 1.16e-2)
    parity(abs(loss.item() - loss_ref.item()) / abs(loss_ref.item()), 7.6e-3, "masked loss, HIP vs fp32 oracle")
    grads = tr.backward(d_out)
    assert sorted(grads) == names and not any("patch_embed.proj" in n for n in grads)
    worst = max((float(_rel(grads[n], g_ref[n])), n) for n in names)
    parity(worst[0], 5e-2, f"worst trainable tensor, HIP vs fp32 oracle ({worst[1]})")
    agg = _rel(_flat(grads, names), _flat(g_ref, names))
    parity(agg, 2.3e-2, "all trainable gradients, HIP vs fp32 oracle")
    # the same oracle with every item's keys limited to text + its valid frames: a different function of the padded frames (measured 0.147 on
    # MI355X, 13x the HIP run's distance to the unmasked oracle)
    _, g_mask, _ = _oracle_grads(cfg, sd, noisy, x0, text, ts, rope, valid, acp, [Nt + v * h * w for v in valid], monkeypatch)
    far = float(_rel(_flat(grads, names), _flat(g_mask, names)))
    assert far > 4 * 2.3e-2, far
    # the padded frames of the output get no gradient; their contents still change the valid frames' gradients
    for b, v in enumerate(valid):
        assert bool((d_out[b, v:] == 0).all())


def test_masked_loss_kernel_vs_restatement_and_bitwise_unmasked_when_all_valid(parity):
    """G3: tg_vpred_loss_grad_masked against the restated loss (per item and gradient, bf16 autograd like the reference); bitwise
    train.vpred_loss_and_grad when every frame is valid."""
    from tokensgen_amd import train
    from tokensgen_amd.train_t2to import vpred_loss_and_grad_masked
    acp = _acp()
    B, Fr = 3, 12
    g = torch.Generator().manual_seed(31)
    out, noisy, x0 = (torch.randn(B, Fr, 16, 8, 12, generator=g).to(BF).to(DEV) for _ in range(3))
    ts = torch.tensor([5, 400, 990])
    for valid in ([4, 8, 12], [1, 12, 5]):
        loss, per_item, grad = vpred_loss_and_grad_masked(out, noisy, x0, ts, acp, valid)
        o = out.clone().requires_grad_(True)
        ref, ref_items = masked_loss_ref(acp, o, noisy, x0, ts.to(DEV), valid)
        ref.backward()
        # tolerances = 2x the values measured on MI355X (1.6e-7, 3.5e-3)
        parity(_rel(per_item, ref_items.detach()), 3.3e-7, "per-item masked loss")
        parity(_rel(grad, o.grad), 7e-3, "d loss / d model output (bf16 autograd: one bf16 rounding per op)")
        for b, v in enumerate(valid):
            assert bool((grad[b, v:] == 0).all())
        # deterministic
        loss2, _, grad2 = vpred_loss_and_grad_masked(out, noisy, x0, ts, acp, valid)
        assert torch.equal(loss2, loss) and torch.equal(grad2, grad)
    la, pa, ga = vpred_loss_and_grad_masked(out, noisy, x0, ts, acp, [Fr] * B)
    lb, pb, gb = train.vpred_loss_and_grad(out, noisy, x0, ts, acp)
    assert torch.equal(ga, gb) and torch.equal(pa, pb) and torch.equal(la, lb)
    with pytest.raises(ValueError):
        vpred_loss_and_grad_masked(out, noisy, x0, ts, acp, [0, 4, 4])


def test_pca_project16_vs_fp32_pca_normalization(parity):
    """G4: tg_pca_project16 against the fp32 restatement of pca_normalization (:1761-1773): (b f h w) x C rows in fp32, pca.transform, minus
    mean, over std, the first 16 coefficients, bf16, [b f 16 h w]."""
    from tokensgen_amd.pca import PCA
    from tokensgen_amd.train_t2to import pca_project16
    B, Fr, C, h, w = 2, 3, 3072, 8, 12
    g = torch.Generator().manual_seed(41)
    tokens = (torch.randn(B, Fr, C, h, w, generator=g) * 2 + 0.3).to(BF)
    pca = PCA(48).fit(torch.randn(300, C, generator=g))
    mean, std = torch.randn(48, generator=g) * 0.5, torch.rand(48, generator=g) + 0.5
    X = tokens.permute(0, 1, 3, 4, 2).reshape(-1, C).float()
    y = (pca.transform(X) - mean) / std
    ref = y.reshape(B, Fr, h, w, -1).permute(0, 1, 4, 2, 3)[:, :, :16]
    got = pca_project16(tokens.to(DEV), pca.components_.to(DEV), pca.mean_.to(DEV), mean, std)
    assert got.shape == (B, Fr, 16, h, w) and got.dtype == BF
    parity(_rel(got, ref), 3.3e-3, "pca_project16 vs fp32 restatement (bf16 output)")      # 2x the 1.65e-3 measured on MI355X
    assert ((got.float().cpu() - ref).abs() <= ref.abs() * 2.0 ** -7 + 1e-4).all()
    # the token-major input (the Resampler's own order) gives the same bits
    tm = tokens.permute(0, 1, 3, 4, 2).reshape(B, Fr * h * w, C).to(DEV)
    assert torch.equal(pca_project16(tm, pca.components_, pca.mean_, mean, std, grid=(Fr, h, w)), got)


def _run_windows(sd, cfg, batches, acp, budget, accum):
    """Two accumulation windows of T2ToTrainStep with AdamW8bit; the optimizer's step is wrapped to snapshot what it started from."""
    from tokensgen_amd.train_t2to import T2ToTrainer, T2ToTrainStep, make_arena
    sd_dev = {k: v.to(BF).to(DEV).contiguous() for k, v in sd.items()}
    tr = T2ToTrainer(sd_dev, cfg["num_attention_heads"], cfg["num_layers"])
    tr.activation_budget_bytes = budget
    yaml = dict(optimizer="adamw", use_8bit_adam=True, learning_rate=3e-4, adam_beta1=0.9, adam_beta2=0.95, adam_epsilon=1e-8,
                adam_weight_decay=1e-4, max_grad_norm=1.0)
    arena, opt = make_arena(tr, yaml)
    step = T2ToTrainStep(tr, arena, opt, acp, accumulation_steps=accum)
    snaps, real = [], opt.step

    def snap_step(*a, **k):
        snaps.append(dict(param=arena.param.clone(), grad=arena.grad.clone()))
        real(*a, **k)
        snaps[-1].update(coef=opt.coef.clone(), after=arena.param.clone())
    opt.step = snap_step
    losses = []
    for x0, noise, text, ts, chunks in batches:
        loss, _ = step.micro_step(noise.to(DEV), ts, text.to(DEV), _rope(x0.shape[1], 8, 12), chunks, model_input=x0.to(DEV))
        losses.append(loss)
    return tr, arena, opt, snaps, torch.stack(losses)


def test_two_accumulation_windows_with_adamw8bit(parity):
    """G5: two full accumulation windows (AdamW8bit, the yaml's hyper-parameters): window 1's update equals tests/adamw8bit_ref.py applied to the
    arena's gradients; window 2's accumulated gradients equal autograd at the UPDATED weights (a stale weight transpose would fail here); the
    frozen patch_embed.proj stays bitwise unchanged; activation_budget_bytes=0 (the yaml's per-block recompute) is bitwise keep-all."""
    import adamw8bit_ref as R
    from oracle import train_ref as T
    from tokensgen_amd.train_t2to import trainable_names
    cfg, sd, _, _, _, _ = _model_case(51, Fr=8)
    acp, accum = _acp(), 2
    g = torch.Generator().manual_seed(52)
    batches = []
    for i in range(2 * accum):
        x0, noise = (torch.randn(3, 8, 16, 8, 12, generator=g).to(BF) for _ in range(2))
        batches.append((x0, noise, _rand(3, 226, 64, seed=60 + i), torch.randint(0, 1000, (3,), generator=g), [1 + i % 2, 2, 1]))
    tr, arena, opt, snaps, losses = _run_windows(sd, cfg, batches, acp, None, accum)
    assert len(snaps) == 2 and bool(torch.isfinite(losses).all())
    assert tr.blocks_kept == 2
    # frozen: the state dict's own tensor and the trainer's padded copy
    assert torch.equal(tr.sd["patch_embed.proj.weight"].cpu(), sd["patch_embed.proj.weight"].to(BF))
    assert torch.equal(tr.sd["patch_embed.proj.bias"].cpu(), sd["patch_embed.proj.bias"].to(BF))
    # window 1: the optimizer step against the restatement from the snapshot
    s0 = snaps[0]
    cs = float(s0["coef"][1])
    bad = 0
    for r in opt.rows:
        el = slice(r.offset, r.offset + r.numel)
        st = R.TensorState(r.numel, opt.block_size, opt.min_8bit_size)
        want = R.step_tensor(s0["param"][el].float().cpu(), s0["grad"][el].cpu(), st, 1, opt.lr, opt.betas, opt.eps, opt.wd, cs if r.clipped else 1.0)
        got = s0["after"][el].float().cpu()
        ulp = want.abs().clamp_min(1e-30).log2().floor().exp2() * 2.0 ** -7
        bad += int(((got - want).abs() > ulp).sum())
    assert bad == 0
    # window 2: the accumulated gradient = mean over its micro-steps of autograd at the weights window 1 left behind
    names = trainable_names(sd)
    p1 = snaps[1]["param"]                                                # what window 2 ran on: the arena after window 1's step
    upd = {k: (p1[arena.offsets[k]:arena.offsets[k] + v.numel()].view(v.shape).float().cpu() if k in arena.views else v) for k, v in sd.items()}
    want = {n: torch.zeros(sd[n].shape, device=DEV) for n in names}
    for x0, noise, text, ts, chunks in batches[accum:]:
        noisy = T.add_noise(acp, x0, noise, ts)
        _, gr, _ = _oracle_grads(cfg, upd, noisy, x0, text, ts, _rope(8, 8, 12), [c * 4 for c in chunks], acp)
        for n in names:
            want[n] += gr[n] / accum
    got = {n: snaps[1]["grad"][arena.offsets[n]:arena.offsets[n] + arena.views[n].numel()].view(arena.shapes[n]) for n in names}
    # tolerances = 2x the values measured on MI355X (2.3e-3, 6.3e-3)
    parity(_rel(_flat(got, names), _flat(want, names)), 4.6e-3, "window 2 accumulated gradients vs autograd at the updated weights")
    worst = max((float(_rel(got[n], want[n])), n) for n in names)
    parity(worst[0], 1.3e-2, f"window 2, worst tensor ({worst[1]})")
    # the reference's per-block checkpointing: bitwise the same run
    tr0, arena0, _, snaps0, losses0 = _run_windows(sd, cfg, batches, acp, 0, accum)
    assert tr0.blocks_kept == 0
    assert torch.equal(losses0, losses) and torch.equal(arena0.param, arena.param)
    assert all(torch.equal(a["grad"], b["grad"]) for a, b in zip(snaps0, snaps))


_FULL = r"""
import json, sys, time, torch
sys.path.insert(0, %r)
from tokensgen_amd.train_t2to import T2ToTrainer, T2ToTrainStep, make_arena, t2to_rope
from oracle import scheduler_ref as S
torch.manual_seed(0)
D, H, L, te, B, Fr, Nt = 3072, 48, 42, 512, 3, 96, 226
dev = "cuda"
def lin(sd, n, o, i, s=0.02):
    sd[n + ".weight"] = (torch.randn(o, i, device=dev) * s).to(torch.bfloat16)
    sd[n + ".bias"] = (torch.randn(o, device=dev) * s).to(torch.bfloat16)
def ln(sd, n, d):
    sd[n + ".weight"] = (1 + 0.1 * torch.randn(d, device=dev)).to(torch.bfloat16)
    sd[n + ".bias"] = (0.1 * torch.randn(d, device=dev)).to(torch.bfloat16)
sd = {}
sd["patch_embed.proj.weight"] = (torch.randn(D, 16, 1, 1, device=dev) * 0.1).to(torch.bfloat16)
sd["patch_embed.proj.bias"] = (torch.randn(D, device=dev) * 0.02).to(torch.bfloat16)
lin(sd, "patch_embed.text_proj", D, 4096); lin(sd, "time_embedding.linear_1", te, D); lin(sd, "time_embedding.linear_2", te, te)
for i in range(L):
    b = "transformer_blocks.%%d" %% i
    for n in ("norm1", "norm2"):
        lin(sd, b + "." + n + ".linear", 6 * D, te); ln(sd, b + "." + n + ".norm", D)
    for n in ("to_q", "to_k", "to_v", "to_out.0"):
        lin(sd, b + ".attn1." + n, D, D)
    ln(sd, b + ".attn1.norm_q", 64); ln(sd, b + ".attn1.norm_k", 64)
    lin(sd, b + ".ff.net.0.proj", 4 * D, D); lin(sd, b + ".ff.net.2", D, 4 * D)
ln(sd, "norm_final", D); lin(sd, "norm_out.linear", 2 * D, te); ln(sd, "norm_out.norm", D); lin(sd, "proj_out", 16, D)
tr = T2ToTrainer(sd, H, L)
tr.activation_budget_bytes = 0
n_train = sum(sd[n].numel() for n in tr.trainable)
arena, opt = make_arena(tr, dict(optimizer="adamw", use_8bit_adam=True, learning_rate=3e-4, max_grad_norm=1.0))
_, ac = S.alphas_cumprod()
step = T2ToTrainStep(tr, arena, opt, torch.as_tensor(ac, dtype=torch.float32), accumulation_steps=5)
x0 = torch.randn(B, Fr, 16, 8, 12, device=dev).to(torch.bfloat16)
noise = torch.randn_like(x0)
text = torch.randn(B, Nt, 4096, device=dev).to(torch.bfloat16)
torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
t0 = time.time()
loss, stepped = step.micro_step(noise, torch.tensor([10, 500, 990]), text, t2to_rope(Fr, device=dev), [24, 13, 1], model_input=x0)
torch.cuda.synchronize()
g = arena.grad
print(json.dumps(dict(loss=float(loss), stepped=bool(stepped), finite=bool(torch.isfinite(g).all()), grad_norm=float(g.norm()), n_train=n_train,
                      peak_gb=torch.cuda.max_memory_allocated() / 1e9, s=time.time() - t0, kept=tr.blocks_kept)))
"""


@pytest.mark.timeout(900)
def test_full_shape_micro_step_recompute_schedule():
    """G6: the yaml's shape (42 x 3072, B = 3, 96 latent frames = 9 442 tokens per item, per-block recompute): one micro-step gives a finite loss and
    finite, non-zero gradients over the 5.57 B trainable parameters, and the peak device memory stays under 100 GB.  In a child process with a time
    limit."""
    r = subprocess.run([sys.executable, "-c", _FULL % ROOT], capture_output=True, text=True, timeout=840)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    import json
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(res)
    assert 5.55e9 < res["n_train"] < 5.59e9
    assert math.isfinite(res["loss"]) and res["finite"] and res["grad_norm"] > 0 and not res["stepped"] and res["kept"] == 0
    assert res["peak_gb"] < 100, res
