"""fp32 autograd references for the T2To trainer with a LoRA adapter: the oracle's plain block / model (oracle/dit_ref.py, n_vip = 0) on weights W + s B A
built from autograd adapter tensors (tests/lora_ref.py `with_lora`: in fp32, F.linear on the merged weight IS the adapted linear).  Nothing here imports
tokensgen_amd."""
import torch

import lora_ref as R


def block_reference(sd, ad, s, pre, hidden, enc, temb, heads, rope, Gh, Ge, dev):
    """One plain block with the adapter, on `dev`: returns (out_hidden, out_text, {adapter name: grad}, d hidden, d text).  sd / ad: fp32 tensors (bf16-rounded
    values); the adapter tensors get requires_grad here."""
    from oracle import dit_ref as O
    sd = {k: v.float().to(dev) for k, v in sd.items()}
    ad = {k: v.float().to(dev).requires_grad_(True) for k, v in ad.items()}
    hf, ef, tf = (t.float().to(dev).requires_grad_(True) for t in (hidden, enc, temb))
    with torch.device(dev):
        oh, oe = O.block_forward(R.with_lora(sd, ad, s), pre, hf, ef, tf[:, None], heads, 0, None, tuple(t.to(dev) for t in rope), None, None)
    ((oh * Gh.float().to(dev)).sum() + (oe * Ge.float().to(dev)).sum()).backward()
    return oh.detach(), oe.detach(), {k: v.grad for k, v in ad.items()}, hf.grad, ef.grad


def model_reference(cfg, sd, ad, s, noisy, x0, text, ts, rope, valid_frames, acp, loss_fn, dev):
    """The whole plain DiT with the adapter + the masked loss (loss_fn: the restated loss of tests/test_t2to_train_gpu.py): (loss, {adapter name: grad})."""
    from oracle import dit_ref as O
    p = {k: v.float().to(dev) for k, v in sd.items()}
    a = {k: v.float().to(dev).requires_grad_(True) for k, v in ad.items()}
    with torch.device(dev):
        out = O.dit_forward(R.with_lora(p, a, s), cfg, noisy.float().to(dev), text.float().to(dev), ts.to(dev), None, tuple(t.to(dev) for t in rope))
    loss, _ = loss_fn(acp, out, noisy.float().to(dev), x0.float().to(dev), ts.to(dev), valid_frames)
    loss.backward()
    return loss.detach(), {k: v.grad for k, v in a.items()}
