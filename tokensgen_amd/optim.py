"""Optimizer side of the To2V training step (train_cogvideo_to2v.py:1056-1130 optimizer, :1157-1164 DDP, :1726 accumulate,
:2012-2021 clip / step / zero_grad).

MI355X-first layout: every trainable parameter lives in ONE flat bf16 arena (the state-dict entries the kernels read are views of it), with one
flat fp32 arena for the accumulated gradient and the optimizer state beside it.  The optimizer step is then three streaming launches over the arena
(sum of squares -> clip coefficient on the device -> AdamW + zero_grad), and the data-parallel gradient exchange is a handful of large RCCL
all-reduces over slices of the same buffer (xGMI rings are per-link bound: few big buckets, once per `gradient_accumulation_steps` micro-steps —
the reference's `no_sync` for the other eight).  Three optimizers: `AdamW` keeps fp32 moments (torch.optim.AdamW); `AdamW8bit` is the yaml's
`use_8bit_adam: true` (bitsandbytes AdamW8bit): block-wise 8-bit moments, 2 B per parameter instead of 8, on an arena built with `moments=False`;
`Prodigy` is the yaml's `optimizer: prodigy` (prodigyopt), learning-rate free, with two arena-wide reductions per step and its scalars on the device.
`get_optimizer` picks one from the yaml's keys."""
import warnings

import torch

from . import kernels as K
from . import lib as L

BF16 = torch.bfloat16
_ALIGN = 64          # elements: keeps every view 128-byte aligned (the GEMM wants 16 B, the streaming kernels like full lines)


def arena_order(names, num_layers):
    """Arena order = the order gradients become final in the backward (last block first, embeddings last, Resampler after the transformer), so
    that a bucket can be handed to RCCL as soon as the backward has passed its end.  Inside a block vip_to_{q,k,v} weights (and biases) are
    adjacent: the fused [3D, D] projection weight is then a view of the arena, not a copy.  A block's LoRA tensors (`*.lora_{A,B}.weight`) sort with their block."""
    def block_key(n):
        for j, pat in enumerate(("vip_to_q.weight", "vip_to_k.weight", "vip_to_v.weight", "vip_to_q.bias", "vip_to_k.bias", "vip_to_v.bias")):
            if n.endswith(pat):
                return (0, j, n)
        # LoRA: the three lora_A of to_q | to_k | to_v side by side (one [3r, D] projection and ONE weight-gradient launch, train.To2VBlockTrainer), then the rest
        for j, pat in enumerate(("to_q.lora_A.weight", "to_k.lora_A.weight", "to_v.lora_A.weight")):
            if n.endswith(pat):
                return (1, j, n)
        return (2, 0, n)
    out = []
    for i in reversed(range(num_layers)):
        pre = f"transformer_blocks.{i}."
        out += sorted((n for n in names if n.startswith(pre)), key=block_key)
    rest = [n for n in names if not n.startswith("transformer_blocks.")]
    out += sorted(n for n in rest if not n.startswith("resampler."))
    out += sorted(n for n in rest if n.startswith("resampler."))
    assert sorted(out) == sorted(names)
    return out


class ParamArena:
    """Flat storage for the trainable parameters.  `params`: {name: tensor}; `order`: names in arena order.  After construction `views[name]` is a
    bf16 view of the arena holding the parameter (install these in the state dict the kernels use).  moments=False: no fp32 moment arenas
    (exp_avg / exp_avg_sq are None) — the arena of an AdamW8bit, which keeps its own 8-bit state."""

    def __init__(self, params, order, device, moments=True):
        self.names = list(order)
        self.offsets, self.shapes = {}, {}
        off = 0
        for n in self.names:
            self.offsets[n], self.shapes[n] = off, tuple(params[n].shape)
            off += (params[n].numel() + _ALIGN - 1) // _ALIGN * _ALIGN
        self.numel = off
        self.param = torch.zeros(off, dtype=BF16, device=device)
        self.grad = torch.zeros(off, dtype=torch.float32, device=device)
        self.exp_avg = torch.zeros(off, dtype=torch.float32, device=device) if moments else None
        self.exp_avg_sq = torch.zeros(off, dtype=torch.float32, device=device) if moments else None
        self.views = {}
        for n in self.names:
            v = self.param[self.offsets[n]: self.offsets[n] + params[n].numel()].view(self.shapes[n])
            v.copy_(params[n])
            self.views[n] = v

    def end_of(self, name):
        n = self.offsets[name]
        k = 1
        for s in self.shapes[name]:
            k *= s
        return n + (k + _ALIGN - 1) // _ALIGN * _ALIGN

    def prefix_elems(self, pred):
        """Number of leading arena elements whose names satisfy pred (they must form a prefix of the order)."""
        end, seen_other = 0, False
        for n in self.names:
            if pred(n):
                assert not seen_other, "names selected by pred must be a prefix of the arena order"
                end = self.end_of(n)
            else:
                seen_other = True
        return end

    def grad_view(self, name):
        o = self.offsets[name]
        k = self.views[name].numel()
        return self.grad[o:o + k].view(self.shapes[name])

    @torch.no_grad()
    def accumulate(self, grads, scale=1.0):
        """grad arena += scale * grads[name] for every entry (bf16 or fp32 tensors shaped like the parameter) — one launch per L.TG_ACCUM_MAX entries."""
        if not grads:
            return
        lib = L.load()
        items = (L.AccumItem * len(grads))()
        keep = []                                          # the contiguous copies must outlive the launch call
        for i, (n, g) in enumerate(grads.items()):
            if tuple(g.shape) != self.shapes[n]:
                raise ValueError(f"gradient of {n}: shape {tuple(g.shape)} != parameter shape {self.shapes[n]}")
            g = g.contiguous()
            if g.dtype not in (BF16, torch.float32):
                raise TypeError(f"gradient of {n}: dtype {g.dtype}")
            keep.append(g)
            items[i].grad, items[i].acc, items[i].n, items[i].grad_is_bf16 = g.data_ptr(), self.grad.data_ptr() + 4 * self.offsets[n], g.numel(), 1 if g.dtype == BF16 else 0
        L.check(lib.tg_grad_accumulate_multi(items, len(grads), float(scale), K._stream()), "tg_grad_accumulate_multi")

    def state_dict(self):
        return {"exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq}

    def layout(self):
        """(name, offset, shape) of every parameter in the flat arenas — stored with a checkpoint so that a resume can check it is loading
        moments of the same geometry."""
        return [(n, int(self.offsets[n]), tuple(self.shapes[n])) for n in self.names]


def _sr_seed(seed):
    """The 64-bit Philox key of stochastic rounding from a yaml / argparse seed (None -> 0; negative values wrap)."""
    return int(seed or 0) & 0xFFFFFFFFFFFFFFFF


class AdamW:
    """torch.optim.AdamW semantics (decoupled weight decay) on a ParamArena, with the reference's gradient clipping folded in:
    `clip_elems` leading arena elements (the transformer's parameters, train_cogvideo_to2v.py:2014-2015) are clipped to `max_grad_norm` by their
    global L2 norm; the rest (the Resampler) is stepped unclipped, as in the reference.  stochastic_round=True (not in the reference):
    the bf16 parameter write rounds stochastically (tg_adamw_step_sr) with bits that depend on (sr_seed, step t, arena index) only; give every
    data-parallel rank the same sr_seed."""

    def __init__(self, arena, lr=2e-4, betas=(0.9, 0.95), eps=1e-8, weight_decay=1e-4, max_grad_norm=1.0, clip_elems=None, stochastic_round=False,
                 sr_seed=0):
        if arena.exp_avg is None:
            raise ValueError("AdamW needs a ParamArena with fp32 moments (moments=True); an arena built with moments=False is for AdamW8bit")
        self.arena, self.lr, self.betas, self.eps, self.wd, self.max_norm = arena, lr, betas, eps, weight_decay, max_grad_norm
        self.clip_elems = arena.numel if clip_elems is None else int(clip_elems)
        self.stochastic_round, self.sr_seed = bool(stochastic_round), _sr_seed(sr_seed)
        self.t = 0
        dev = arena.param.device
        self._ws = torch.empty(L.load().tg_grad_norm_ws_floats(), dtype=torch.float32, device=dev)
        self.coef = torch.ones(2, dtype=torch.float32, device=dev)        # [total norm, clip coefficient] of the last step (device side)

    @torch.no_grad()
    def step(self, lr=None, zero_grad=True):
        a, lib = self.arena, L.load()
        self.t += 1
        lr = self.lr if lr is None else lr
        st = K._stream()
        clip_ptr = None
        nc = self.clip_elems
        if self.max_norm is not None and self.max_norm > 0 and nc > 0:
            L.check(lib.tg_grad_clip_coef(a.grad.data_ptr(), nc, float(self.max_norm), self._ws.data_ptr(), self.coef.data_ptr(), st), "tg_grad_clip_coef")
            clip_ptr = self.coef.data_ptr() + 4
        for lo, hi, cp in ((0, nc, clip_ptr), (nc, a.numel, None)):
            if hi > lo:
                args = (a.param.data_ptr() + 2 * lo, a.grad.data_ptr() + 4 * lo, a.exp_avg.data_ptr() + 4 * lo, a.exp_avg_sq.data_ptr() + 4 * lo,
                        hi - lo, self.t, float(lr), float(self.betas[0]), float(self.betas[1]), float(self.eps), float(self.wd), cp, 1 if zero_grad else 0)
                if self.stochastic_round:                                  # lo: the segment's absolute arena index (the random bits follow the element)
                    L.check(lib.tg_adamw_step_sr(*args, lo, self.sr_seed, st), "tg_adamw_step_sr")
                else:
                    L.check(lib.tg_adamw_step(*args, st), "tg_adamw_step")


    # ---- checkpoint / resume (the reference: accelerator.save_state / load_state behind --resume_from_checkpoint, train_cogvideo_to2v.py:1690-1716,
    # 2030-2047).  Layout of the dict: {"t": optimizer steps taken (bias correction), "exp_avg" / "exp_avg_sq": the flat fp32 moment arenas,
    # "grad": the flat fp32 gradient arena (non-zero only in the middle of an accumulation window), "layout": ParamArena.layout(),
    # "hyper": lr / betas / eps / weight_decay / max_grad_norm / clip_elems / stochastic_round / sr_seed (with "t": a resume continues the same
    # random stream; a checkpoint without the two keys loads as off)}.  Parameters are saved separately under the reference's names
    # (CogVideoXTransformer3DModel.save_vip_layers -> vip.pt, Resampler.save_pretrained).
    def state_dict(self):
        a = self.arena
        return {"t": int(self.t), "exp_avg": a.exp_avg.detach().cpu().clone(), "exp_avg_sq": a.exp_avg_sq.detach().cpu().clone(),
                "grad": a.grad.detach().cpu().clone(), "layout": a.layout(),
                "hyper": {"lr": self.lr, "betas": tuple(self.betas), "eps": self.eps, "weight_decay": self.wd, "max_grad_norm": self.max_norm,
                          "clip_elems": self.clip_elems, "stochastic_round": self.stochastic_round, "sr_seed": self.sr_seed}}

    @torch.no_grad()
    def load_state_dict(self, sd):
        a = self.arena
        kind = sd.get("hyper", {}).get("kind", "adamw")
        if kind != "adamw":
            raise ValueError(f"AdamW.load_state_dict: the checkpoint holds {kind!r} optimizer state, not fp32 AdamW moments")
        if [(n, int(o), tuple(sh)) for n, o, sh in sd["layout"]] != a.layout():
            raise ValueError("AdamW.load_state_dict: the checkpoint's arena layout (names / offsets / shapes) differs from this arena's")
        for name in ("exp_avg", "exp_avg_sq", "grad"):
            t = sd[name]
            if t.numel() != a.numel or t.dtype != torch.float32:
                raise ValueError(f"AdamW.load_state_dict: {name} has {t.numel()} {t.dtype} elements, arena has {a.numel} fp32")
            getattr(a, name).copy_(t.to(a.param.device))
        self.t = int(sd["t"])
        h = sd.get("hyper", {})
        self.lr, self.betas, self.eps = h.get("lr", self.lr), tuple(h.get("betas", self.betas)), h.get("eps", self.eps)
        self.wd, self.max_norm, self.clip_elems = h.get("weight_decay", self.wd), h.get("max_grad_norm", self.max_norm), int(h.get("clip_elems", self.clip_elems))
        self.stochastic_round, self.sr_seed = bool(h.get("stochastic_round", False)), _sr_seed(h.get("sr_seed", 0))


def dynamic_map(signed=True, max_exponent_bits=7, total_bits=8):
    """bitsandbytes.functional.create_dynamic_map (0.44.1), restated in the same torch fp32 operations: for every decade e = 0 .. max_exponent_bits-1
    the means of linearly spaced fractions in [0.1, 1] scaled by 10^(e - max_exponent_bits + 1) (and their negatives if signed), plus 0 and 1.0; the
    256 codes sorted ascending.  AdamW8bit quantises exp_avg with the signed map and exp_avg_sq with the unsigned one."""
    non_sign_bits = total_bits - 1                         # bitsandbytes: `total_bits - (1 if signed else 1)`
    if 2 ** (non_sign_bits - max_exponent_bits) - 1 != 0:
        raise NotImplementedError("dynamic_map: only the layouts without extra zero-exponent items (AdamW8bit's 7 exponent bits of 8)")
    data = []
    for i in range(max_exponent_bits):
        items = 2 ** (i + non_sign_bits - max_exponent_bits) + 1 if signed else 2 ** (i + non_sign_bits - max_exponent_bits + 1) + 1
        bounds = torch.linspace(0.1, 1, items)
        means = (bounds[:-1] + bounds[1:]) / 2.0
        data += ((10 ** (-(max_exponent_bits - 1) + i)) * means).tolist()
        if signed:
            data += (-(10 ** (-(max_exponent_bits - 1) + i)) * means).tolist()
    data += [0.0, 1.0]
    assert len(data) == 2 ** total_bits
    data.sort()
    return torch.tensor(data, dtype=torch.float32)


class BlockRow:
    """One row of the AdamW8bit tensor table (tg_adamw8bit_row): `kind` L.ADAMW8BIT_BLOCKWISE or L.ADAMW8BIT_FP32, `state` = first absmax index or
    first element in the small fp32 moment arenas, `first_block` = workgroups of the earlier rows, `blocks` = this tensor's."""
    __slots__ = ("name", "offset", "numel", "kind", "state", "first_block", "blocks", "clipped")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


def block_table(arena, block_size=2048, min_8bit_size=4096, clip_elems=None):
    """The static tensor table of AdamW8bit over `arena` (arena order): returns (rows, absmax entries per moment, small fp32 moment elements).
    Tensors with numel >= min_8bit_size get 8-bit moments in blocks of block_size that restart at the tensor's first element (the last may be
    partial); the others keep fp32 moments in a compact side arena (64-element aligned slots).  clipped: the tensor lies below clip_elems."""
    clip_elems = arena.numel if clip_elems is None else int(clip_elems)
    rows, n_absmax, n_small, wg = [], 0, 0, 0
    for n in arena.names:
        off, k = arena.offsets[n], arena.views[n].numel()
        if off < clip_elems < off + k:
            raise ValueError(f"AdamW8bit: clip_elems {clip_elems} splits the tensor {n} [{off}, {off + k}); it must fall on a tensor boundary")
        blocks = (k + block_size - 1) // block_size
        if k >= min_8bit_size:
            rows.append(BlockRow(name=n, offset=off, numel=k, kind=L.ADAMW8BIT_BLOCKWISE, state=n_absmax, first_block=wg, blocks=blocks, clipped=off < clip_elems))
            n_absmax += blocks
        else:
            rows.append(BlockRow(name=n, offset=off, numel=k, kind=L.ADAMW8BIT_FP32, state=n_small, first_block=wg, blocks=blocks, clipped=off < clip_elems))
            n_small += (k + _ALIGN - 1) // _ALIGN * _ALIGN
        wg += blocks
    return rows, n_absmax, n_small


class AdamW8bit:
    """bitsandbytes AdamW8bit (0.44.1, block-wise; the yaml's `use_8bit_adam: true`, train_cogvideo_to2v.py:1083-1098) on a ParamArena, with the
    same surface as AdamW (step / coef / t / state_dict / load_state_dict) and the same clipping split.  Tensors of >= min_8bit_size elements keep
    both moments as uint8 codes of the dynamic maps (exp_avg signed, exp_avg_sq unsigned) in blocks of block_size elements with one fp32 absmax per
    block and moment; the state arenas are byte arenas at the parameter arena's offsets.  Smaller tensors keep fp32 moments.  The update itself is
    tg_adamw_step's fp32 arithmetic on the dequantised moments (where this restates bitsandbytes).  Build the arena with moments=False:
    the fp32 moment arenas are what this optimizer saves.  stochastic_round / sr_seed: as AdamW's (tg_adamw8bit_step_sr)."""

    KIND = "adamw8bit"

    def __init__(self, arena, lr=2e-4, betas=(0.9, 0.95), eps=1e-8, weight_decay=1e-4, max_grad_norm=1.0, clip_elems=None, min_8bit_size=4096,
                 block_size=2048, stochastic_round=False, sr_seed=0):
        if block_size not in (256, 512, 1024, 2048):
            raise ValueError(f"AdamW8bit: block_size {block_size} not in (256, 512, 1024, 2048)")
        self.arena, self.lr, self.betas, self.eps, self.wd, self.max_norm = arena, lr, tuple(betas), eps, weight_decay, max_grad_norm
        self.clip_elems = arena.numel if clip_elems is None else int(clip_elems)
        self.min_8bit_size, self.block_size = int(min_8bit_size), int(block_size)
        self.stochastic_round, self.sr_seed = bool(stochastic_round), _sr_seed(sr_seed)
        self.t = 0
        dev = arena.param.device
        self.rows, n_absmax, n_small = block_table(arena, self.block_size, self.min_8bit_size, self.clip_elems)
        self.nblocks = self.rows[-1].first_block + self.rows[-1].blocks
        self.state1 = torch.zeros(arena.numel, dtype=torch.uint8, device=dev)          # codes start at 0 with absmax 0: the moments dequantise to 0
        self.state2 = torch.zeros(arena.numel, dtype=torch.uint8, device=dev)
        self.absmax1 = torch.zeros(max(n_absmax, 1), dtype=torch.float32, device=dev)
        self.absmax2 = torch.zeros(max(n_absmax, 1), dtype=torch.float32, device=dev)
        self.small_m = torch.zeros(max(n_small, _ALIGN), dtype=torch.float32, device=dev)
        self.small_v = torch.zeros(max(n_small, _ALIGN), dtype=torch.float32, device=dev)
        self.qmap1, self.qmap2 = dynamic_map(True).to(dev), dynamic_map(False).to(dev)
        tab = (L.Adamw8bitRow * len(self.rows))()
        for i, r in enumerate(self.rows):
            tab[i].offset, tab[i].numel, tab[i].state, tab[i].first_block, tab[i].kind, tab[i].clipped = r.offset, r.numel, r.state, r.first_block, r.kind, int(r.clipped)
        self._table = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(dev)   # device-resident, built once: the layout is static
        self._ws = torch.empty(L.load().tg_grad_norm_ws_floats(), dtype=torch.float32, device=dev)
        self.coef = torch.ones(2, dtype=torch.float32, device=dev)        # [total norm, clip coefficient] of the last step (device side)

    @torch.no_grad()
    def step(self, lr=None, zero_grad=True):
        a, lib = self.arena, L.load()
        self.t += 1
        lr = self.lr if lr is None else lr
        st = K._stream()
        clip_ptr = None
        nc = self.clip_elems
        if self.max_norm is not None and self.max_norm > 0 and nc > 0:
            L.check(lib.tg_grad_clip_coef(a.grad.data_ptr(), nc, float(self.max_norm), self._ws.data_ptr(), self.coef.data_ptr(), st), "tg_grad_clip_coef")
            clip_ptr = self.coef.data_ptr() + 4
        args = (a.param.data_ptr(), a.grad.data_ptr(), self.state1.data_ptr(), self.state2.data_ptr(), self.absmax1.data_ptr(), self.absmax2.data_ptr(),
                self.small_m.data_ptr(), self.small_v.data_ptr(), self.qmap1.data_ptr(), self.qmap2.data_ptr(), self._table.data_ptr(), len(self.rows),
                self.nblocks, self.block_size, self.t, float(lr), float(self.betas[0]), float(self.betas[1]), float(self.eps), float(self.wd), clip_ptr,
                1 if zero_grad else 0)
        if self.stochastic_round:
            L.check(lib.tg_adamw8bit_step_sr(*args, self.sr_seed, st), "tg_adamw8bit_step_sr")
        else:
            L.check(lib.tg_adamw8bit_step(*args, st), "tg_adamw8bit_step")

    # ---- checkpoint / resume, as AdamW: {"t", "state1" / "state2": the uint8 code arenas, "absmax1" / "absmax2", "small_m" / "small_v": the fp32
    # moments of the small tensors, "grad", "layout", "hyper": AdamW's keys (stochastic_round / sr_seed among them) + kind / block_size / min_8bit_size}
    _STATE = ("state1", "state2", "absmax1", "absmax2", "small_m", "small_v")

    def state_dict(self):
        a = self.arena
        sd = {"t": int(self.t), "grad": a.grad.detach().cpu().clone(), "layout": a.layout(),
              "hyper": {"lr": self.lr, "betas": tuple(self.betas), "eps": self.eps, "weight_decay": self.wd, "max_grad_norm": self.max_norm,
                        "clip_elems": self.clip_elems, "kind": self.KIND, "block_size": self.block_size, "min_8bit_size": self.min_8bit_size,
                        "stochastic_round": self.stochastic_round, "sr_seed": self.sr_seed}}
        for name in self._STATE:
            sd[name] = getattr(self, name).detach().cpu().clone()
        return sd

    @torch.no_grad()
    def load_state_dict(self, sd):
        a = self.arena
        h = sd.get("hyper", {})
        kind = h.get("kind", "adamw")
        if kind != self.KIND:
            raise ValueError(f"AdamW8bit.load_state_dict: the checkpoint holds {kind!r} optimizer state, not {self.KIND!r}")
        for key, mine in (("block_size", self.block_size), ("min_8bit_size", self.min_8bit_size)):
            if int(h.get(key, -1)) != mine:
                raise ValueError(f"AdamW8bit.load_state_dict: the checkpoint's {key} is {h.get(key)}, this optimizer's is {mine}")
        if [(n, int(o), tuple(sh)) for n, o, sh in sd["layout"]] != a.layout():
            raise ValueError("AdamW8bit.load_state_dict: the checkpoint's arena layout (names / offsets / shapes) differs from this arena's")
        for name in self._STATE + ("grad",):
            dst = a.grad if name == "grad" else getattr(self, name)
            t = sd[name]
            if t.numel() != dst.numel() or t.dtype != dst.dtype:
                raise ValueError(f"AdamW8bit.load_state_dict: {name} has {t.numel()} {t.dtype} elements, this optimizer has {dst.numel()} {dst.dtype}")
            dst.copy_(t.to(dst.device))
        self.t = int(sd["t"])
        self.lr, self.betas, self.eps = h.get("lr", self.lr), tuple(h.get("betas", self.betas)), h.get("eps", self.eps)
        self.wd, self.max_norm = h.get("weight_decay", self.wd), h.get("max_grad_norm", self.max_norm)
        self.stochastic_round, self.sr_seed = bool(h.get("stochastic_round", False)), _sr_seed(h.get("sr_seed", 0))
        if int(h.get("clip_elems", self.clip_elems)) != self.clip_elems:
            raise ValueError(f"AdamW8bit.load_state_dict: the checkpoint's clip_elems is {h.get('clip_elems')}, this optimizer's is {self.clip_elems} "
                             "(the table's clipped flags are fixed at construction)")


class Prodigy:
    """prodigyopt.Prodigy (1.0; the yaml's `optimizer: prodigy`, train_cogvideo_to2v.py:1109-1132) on a ParamArena built with moments=True, with the
    same surface as AdamW (step / coef / t / state_dict / load_state_dict) and the same clipping split.  Learning-rate free: the step size is d * lr
    with d an estimate of the distance to the solution grown from d0 by sum g . (x0 - x) / sum |s|; lr stays near 1.  The arena's exp_avg /
    exp_avg_sq are Prodigy's (scaled by d and d^2); this optimizer adds s (fp32), delta = x - x0 (fp32) and p0 = x0 (bf16), 10 B per parameter, and
    writes param = bf16(p0 + delta) every step: an update applied to the bf16 parameter in place is rounded away while d is still d0, x0 - x stays
    0 and d never grows.  d, d_max, the numerator and the last step's d_hat / denominator / dlr live on the device in fp64
    (`scalars`, layout: include/tokensgen_hip.h); a step is three launches and never synchronises — `stats()` is the one call that does."""

    KIND = "prodigy"
    _STATE = ("s", "delta", "p0", "scalars")
    _SCALARS = ("d", "d_max", "d_numerator", "d_hat", "d_denom", "dlr")

    def __init__(self, arena, lr=1.0, betas=(0.9, 0.999), beta3=None, eps=1e-8, weight_decay=0.0, decouple=True, use_bias_correction=False,
                 safeguard_warmup=False, d0=1e-6, d_coef=1.0, growth_rate=float("inf"), max_grad_norm=1.0, clip_elems=None):
        if arena.exp_avg is None:
            raise NotImplementedError("optimizer 'prodigy' (Prodigy) needs the arena's fp32 moments (exp_avg / exp_avg_sq): build the ParamArena with "
                                      "moments=True; an arena built with moments=False is for AdamW8bit")
        if not (eps > 0 and d0 > 0):
            raise ValueError(f"Prodigy: eps {eps} and d0 {d0} must be positive")
        self.arena, self.lr, self.betas, self.eps, self.wd, self.max_norm = arena, lr, tuple(betas), eps, weight_decay, max_grad_norm
        self.beta3 = float(self.betas[1]) ** 0.5 if beta3 is None else float(beta3)
        self.decouple, self.use_bias_correction, self.safeguard_warmup = bool(decouple), bool(use_bias_correction), bool(safeguard_warmup)
        self.d0, self.d_coef, self.growth_rate = float(d0), float(d_coef), float(growth_rate)
        self.clip_elems = arena.numel if clip_elems is None else int(clip_elems)
        self.t = 0
        dev = arena.param.device
        self.p0 = arena.param.clone()
        self.delta = torch.zeros(arena.numel, dtype=torch.float32, device=dev)
        self.s = torch.zeros(arena.numel, dtype=torch.float32, device=dev)
        self.scalars = torch.tensor([self.d0, self.d0] + [0.0] * (L.PRODIGY_STATE_DOUBLES - 2), dtype=torch.float64, device=dev)
        lib = L.load()
        self._ws = torch.empty(lib.tg_grad_norm_ws_floats(), dtype=torch.float32, device=dev)
        self._ws64 = torch.empty(lib.tg_prodigy_ws_doubles(), dtype=torch.float64, device=dev)
        self.coef = torch.ones(2, dtype=torch.float32, device=dev)        # [total norm, clip coefficient] of the last step (device side)

    @torch.no_grad()
    def step(self, lr=None, zero_grad=True):
        a, lib = self.arena, L.load()
        self.t += 1
        lr = self.lr if lr is None else lr
        if not lr > 0:                                                     # prodigyopt: no statistics at lr 0, the denominator is 0, nothing moves
            if zero_grad:
                a.grad.zero_()
            return
        st = K._stream()
        clip_ptr = None
        nc = self.clip_elems
        if self.max_norm is not None and self.max_norm > 0 and nc > 0:
            L.check(lib.tg_grad_clip_coef(a.grad.data_ptr(), nc, float(self.max_norm), self._ws.data_ptr(), self.coef.data_ptr(), st), "tg_grad_clip_coef")
            clip_ptr = self.coef.data_ptr() + 4
        L.check(lib.tg_prodigy_step(a.param.data_ptr(), a.grad.data_ptr(), a.exp_avg.data_ptr(), a.exp_avg_sq.data_ptr(), self.s.data_ptr(),
                                    self.delta.data_ptr(), self.p0.data_ptr(), self.scalars.data_ptr(), self._ws64.data_ptr(), a.numel,
                                    nc if clip_ptr is not None else 0, self.t, float(lr), float(self.betas[0]), float(self.betas[1]), self.beta3,
                                    float(self.eps), float(self.wd), self.d0, self.d_coef, self.growth_rate, int(self.decouple),
                                    int(self.use_bias_correction), int(self.safeguard_warmup), clip_ptr, 1 if zero_grad else 0, st), "tg_prodigy_step")

    def stats(self):
        """{"d", "d_max", "d_numerator", "d_hat", "d_denom", "dlr"} as Python floats (d_hat, d_denom, dlr: of the last step that was not skipped).
        Synchronises with the device; d * lr is the effective learning rate a Prodigy run logs."""
        return dict(zip(self._SCALARS, self.scalars.cpu().tolist()))

    # ---- checkpoint / resume: AdamW's dict + "s" / "delta" / "p0" (flat arenas), "scalars" (the fp64 state buffer) and, in "hyper", kind and
    # Prodigy's own knobs.  The parameters are saved separately (as for AdamW); a resume must put back exactly bf16(p0 + delta).
    def _hyper(self):
        return {"lr": self.lr, "betas": tuple(self.betas), "beta3": self.beta3, "eps": self.eps, "weight_decay": self.wd, "max_grad_norm": self.max_norm,
                "clip_elems": self.clip_elems, "kind": self.KIND, "decouple": self.decouple, "use_bias_correction": self.use_bias_correction,
                "safeguard_warmup": self.safeguard_warmup, "d0": self.d0, "d_coef": self.d_coef, "growth_rate": self.growth_rate}

    def state_dict(self):
        a = self.arena
        sd = {"t": int(self.t), "exp_avg": a.exp_avg.detach().cpu().clone(), "exp_avg_sq": a.exp_avg_sq.detach().cpu().clone(),
              "grad": a.grad.detach().cpu().clone(), "layout": a.layout(), "hyper": self._hyper()}
        for name in self._STATE:
            sd[name] = getattr(self, name).detach().cpu().clone()
        return sd

    @torch.no_grad()
    def load_state_dict(self, sd, chunk=1 << 26):
        a = self.arena
        h = sd.get("hyper", {})
        kind = h.get("kind", "adamw")
        if kind != self.KIND:
            raise ValueError(f"Prodigy.load_state_dict: the checkpoint holds {kind!r} optimizer state, not {self.KIND!r}")
        if [(n, int(o), tuple(sh)) for n, o, sh in sd["layout"]] != a.layout():
            raise ValueError("Prodigy.load_state_dict: the checkpoint's arena layout (names / offsets / shapes) differs from this arena's")
        dst = {"exp_avg": a.exp_avg, "exp_avg_sq": a.exp_avg_sq, "grad": a.grad, **{name: getattr(self, name) for name in self._STATE}}
        for name, d in dst.items():
            t = sd[name]
            if t.numel() != d.numel() or t.dtype != d.dtype:
                raise ValueError(f"Prodigy.load_state_dict: {name} has {t.numel()} {t.dtype} elements, this optimizer has {d.numel()} {d.dtype}")
        for lo in range(0, a.numel, chunk):                                # the parameters must be the checkpoint's own bf16(p0 + delta), bit for bit
            sl = slice(lo, min(a.numel, lo + chunk))
            want = (sd["p0"][sl].to(a.param.device).float() + sd["delta"][sl].to(a.param.device)).to(BF16)
            if not torch.equal(want.view(torch.int16), a.param[sl].view(torch.int16)):
                raise ValueError("Prodigy.load_state_dict: the arena's param is not bitwise bf16(p0 + delta) of the checkpoint — load the parameters "
                                 "saved with this checkpoint before the optimizer state")
        for name, d in dst.items():
            d.copy_(sd[name].to(d.device))
        self.t = int(sd["t"])
        self.lr, self.betas, self.eps = h.get("lr", self.lr), tuple(h.get("betas", self.betas)), h.get("eps", self.eps)
        self.beta3, self.wd, self.max_norm = float(h.get("beta3", self.beta3)), h.get("weight_decay", self.wd), h.get("max_grad_norm", self.max_norm)
        self.clip_elems = int(h.get("clip_elems", self.clip_elems))
        self.decouple, self.use_bias_correction = bool(h.get("decouple", self.decouple)), bool(h.get("use_bias_correction", self.use_bias_correction))
        self.safeguard_warmup = bool(h.get("safeguard_warmup", self.safeguard_warmup))
        self.d0, self.d_coef, self.growth_rate = float(h.get("d0", self.d0)), float(h.get("d_coef", self.d_coef)), float(h.get("growth_rate", self.growth_rate))


def get_optimizer(arena, cfg, clip_elems=None):
    """The reference's get_optimizer (train_cogvideo_to2v.py:1056-1133) for its yaml keys: optimizer, use_8bit_adam, learning_rate, adam_beta1 /
    adam_beta2, adam_epsilon, adam_weight_decay, max_grad_norm, prodigy_beta3 / prodigy_decouple / prodigy_use_bias_correction /
    prodigy_safeguard_warmup (argparse defaults where a key is missing).  `cfg`: a dict or an object with those attributes.  "adamw" -> AdamW,
    "adamw" + use_8bit_adam -> AdamW8bit (build the arena with moments=False), "prodigy" -> Prodigy (arena with moments=True; warns when
    learning_rate <= 0.1, as the reference does); use_8bit_adam with another optimizer is ignored with a warning, an unknown optimizer falls back to
    "adamw" with a warning; "adam" raises NotImplementedError.  One key of this project's own: bf16_stochastic_round (default False) turns on the
    stochastic bf16 parameter write of AdamW / AdamW8bit, seeded by the yaml's `seed` (default 0) — the SAME seed on every rank, the rank is not
    mixed in, so data-parallel ranks keep bitwise-equal parameters; with "prodigy" it is ignored with a warning (Prodigy writes bf16(p0 + delta)
    from an exact fp32 delta: nothing is lost to the rounding there)."""
    get = cfg.get if isinstance(cfg, dict) else (lambda k, d=None: getattr(cfg, k, d))
    name = str(get("optimizer", "adam")).lower()
    if name not in ("adam", "adamw", "prodigy"):
        warnings.warn(f"Unsupported choice of optimizer: {name}. Supported optimizers include ['adam', 'adamw', 'prodigy']. Defaulting to AdamW")
        name = "adamw"
    use_8bit = bool(get("use_8bit_adam", False))
    if use_8bit and name not in ("adam", "adamw"):
        warnings.warn(f"use_8bit_adam is ignored when optimizer is not set to 'Adam' or 'AdamW'. Optimizer was set to {name}")
        use_8bit = False
    if name == "adam":
        raise NotImplementedError("optimizer 'adam' (torch.optim.Adam / bitsandbytes Adam8bit: weight decay added to the gradient) is not implemented; "
                                  "the training yamls use 'adamw'")
    sr = bool(get("bf16_stochastic_round", False))
    if name == "prodigy":
        if sr:
            warnings.warn("bf16_stochastic_round is ignored when optimizer is 'prodigy': Prodigy keeps the update in an exact fp32 delta and writes "
                          "bf16(p0 + delta), so no update is lost to the rounding")
        lr = float(get("learning_rate", 1e-4))
        if lr <= 0.1:
            warnings.warn("Learning rate is too low. When using prodigy, it's generally better to set learning rate around 1.0")
        beta3 = get("prodigy_beta3", None)
        return Prodigy(arena, lr=lr, betas=(float(get("adam_beta1", 0.9)), float(get("adam_beta2", 0.95))), beta3=None if beta3 is None else float(beta3),
                       weight_decay=float(get("adam_weight_decay", 1e-4)), eps=float(get("adam_epsilon", 1e-8)),
                       decouple=bool(get("prodigy_decouple", False)), use_bias_correction=bool(get("prodigy_use_bias_correction", False)),
                       safeguard_warmup=bool(get("prodigy_safeguard_warmup", False)), max_grad_norm=float(get("max_grad_norm", 1.0)), clip_elems=clip_elems)
    kw = dict(lr=float(get("learning_rate", 1e-4)), betas=(float(get("adam_beta1", 0.9)), float(get("adam_beta2", 0.95))),
              eps=float(get("adam_epsilon", 1e-8)), weight_decay=float(get("adam_weight_decay", 1e-4)), max_grad_norm=float(get("max_grad_norm", 1.0)),
              clip_elems=clip_elems, stochastic_round=sr, sr_seed=get("seed", 0))
    return AdamW8bit(arena, **kw) if use_8bit else AdamW(arena, **kw)


def constant_with_warmup(step, base_lr, warmup_steps):
    """diffusers get_scheduler("constant") ignores warm-up; "constant_with_warmup" ramps linearly (optimization.py).  The yaml uses "constant"."""
    return base_lr if warmup_steps <= 0 else base_lr * min(1.0, step / float(warmup_steps))


class GradSync:
    """Data-parallel gradient exchange (accelerate DDP, train_cogvideo_to2v.py:1157-1164): SUM all-reduce of the flat gradient in a few large
    buckets; averaging is folded into the accumulation scale (1 / (accumulation_steps * world_size)).  `ready(end)` may be called during the
    backward of the LAST micro-step of an accumulation window: every bucket that lies entirely below `end` (arena order = backward order) is
    handed to the collective asynchronously, so the exchange overlaps the remaining blocks' backward; `finish()` launches what is left and waits.
    Works on any flat tensor (gloo on CPU in the tests, RCCL on the GPU)."""

    def __init__(self, flat, group=None, bucket_elems=64 * 1024 * 1024):
        import torch.distributed as dist
        self.dist, self.flat, self.group = dist, flat, group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        n = flat.numel()
        self.bounds = [(lo, min(n, lo + bucket_elems)) for lo in range(0, n, bucket_elems)]
        self._next, self._work = 0, []

    def ready(self, end):
        if not self.dist.is_initialized():
            return                                   # single process without a process group: nothing to exchange
        while self._next < len(self.bounds) and self.bounds[self._next][1] <= end:
            lo, hi = self.bounds[self._next]
            self._work.append(self.dist.all_reduce(self.flat[lo:hi], op=self.dist.ReduceOp.SUM, group=self.group, async_op=True))
            self._next += 1

    def finish(self):
        self.ready(self.flat.numel())
        for w in self._work:
            w.wait()
        self._next, self._work = 0, []
