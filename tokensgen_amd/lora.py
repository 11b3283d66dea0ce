"""LoRA on the DiT attention projections (the yamls' `use_lora` / `lora_path` / `lora_params`; reference: peft adapters added, trained, saved and loaded by
train_cogvideo_to2v.py:1326-1338, 1456-1481, 1345-1416).  peft and diffusers are not dependencies: the semantics restated here are peft's LoraLayer on
nn.Linear with init_lora_weights=True and no dropout,

    y = x W^T + b + s (x A^T) B^T,    A = lora_A.weight [r, in],  B = lora_B.weight [out, r],  s = lora_alpha / r,

with A ~ U(-1/sqrt(in), 1/sqrt(in)) (Kaiming-uniform, a = sqrt(5)) and B = 0, module names matched as peft matches `target_modules` (equal to a target
or ending in "." + target), and the diffusers `save_lora_weights` file layout: `pytorch_lora_weights.safetensors` with keys
`transformer.transformer_blocks.{i}.attn1.{to_q,to_k,to_v,to_out.0}.lora_{A,B}.weight`.

Training applies the adapter UNMERGED (train.To2VBlockTrainer), inference fuses it into the model's weights (CogVideoXTransformer3DModel.fuse_lora, on
tg_lora_merge)."""
import math
import os

import torch

WEIGHT_NAME = "pytorch_lora_weights.safetensors"
PREFIX = "transformer."
DEFAULT_TARGETS = ("to_k", "to_q", "to_v", "to_out.0")


class LoraConfig:
    """rank / lora_alpha / target_modules of the yaml's `lora_params` (+ `is_trainable` of the training yaml: a frozen adapter is applied in the forward and
    gets no gradient, train_cogvideo_to2v.py:1465-1467)."""

    def __init__(self, rank=128, lora_alpha=64, target_modules=DEFAULT_TARGETS, is_trainable=True):
        self.rank, self.lora_alpha = int(rank), float(lora_alpha)
        self.target_modules = tuple(target_modules)
        self.is_trainable = bool(is_trainable)
        if self.rank <= 0:
            raise ValueError(f"LoraConfig: rank {rank} must be positive")

    @classmethod
    def from_params(cls, lora_params):
        """From the yaml's `lora_params` mapping (a dict or an object with those attributes)."""
        get = lora_params.get if isinstance(lora_params, dict) else (lambda k, d=None: getattr(lora_params, k, d))
        return cls(rank=get("rank", 128), lora_alpha=get("lora_alpha", 64), target_modules=tuple(get("target_modules", DEFAULT_TARGETS)),
                   is_trainable=bool(get("is_trainable", True)))

    @property
    def scaling(self):
        return self.lora_alpha / self.rank

    def match(self, module_name):
        """peft's rule for a list of targets: the module name equals a target or ends with "." + target."""
        return any(module_name == t or module_name.endswith("." + t) for t in self.target_modules)


def target_modules(cfg, keys):
    """The linear modules of a model that `cfg` adapts, from its parameter names (sorted; `<module>.weight` with a 2-D meaning is the caller's concern:
    the DiT's targets are all nn.Linear)."""
    return sorted({k[:-len(".weight")] for k in keys if k.endswith(".weight") and ".lora_" not in k and cfg.match(k[:-len(".weight")])})


def is_lora_key(name):
    return name.endswith(".lora_A.weight") or name.endswith(".lora_B.weight")


def _shapes(transformer_config_or_sd, cfg):
    """{module name: (out, in)} of the targets."""
    src = transformer_config_or_sd
    if isinstance(src, dict) and any(torch.is_tensor(v) for v in src.values()):
        return {m: tuple(src[m + ".weight"].shape) for m in target_modules(cfg, src.keys())}
    get = src.get if isinstance(src, dict) else (lambda k, d=None: getattr(src, k, d))
    D = int(get("num_attention_heads")) * int(get("attention_head_dim"))
    names = [f"transformer_blocks.{i}.attn1.{t}" for i in range(int(get("num_layers"))) for t in ("to_q", "to_k", "to_v", "to_out.0")]
    return {m: (D, D) for m in names if cfg.match(m)}


def init_adapter(cfg, transformer_config_or_sd, generator=None, dtype=torch.bfloat16, device="cpu"):
    """A fresh adapter {`<module>.lora_A.weight`: [r, in], `<module>.lora_B.weight`: [out, r]} for every target: A Kaiming-uniform (a = sqrt(5)), drawn in
    fp32 on the CPU from `generator` in sorted module order, B zeros — a fresh adapter changes nothing."""
    out = {}
    for m, (cout, cin) in sorted(_shapes(transformer_config_or_sd, cfg).items()):
        bound = 1.0 / math.sqrt(cin)                       # gain sqrt(2 / (1 + 5)) * sqrt(3 / fan_in)
        a = (torch.rand(cfg.rank, cin, generator=generator, dtype=torch.float32) * 2.0 - 1.0) * bound
        out[m + ".lora_A.weight"] = a.to(dtype).to(device)
        out[m + ".lora_B.weight"] = torch.zeros(cout, cfg.rank, dtype=dtype, device=device)
    return out


def check_adapter(sd, cfg=None):
    """Every module has both halves, of matching rank (and of cfg.rank when given); raises ValueError naming the key."""
    mods = sorted({k.rsplit(".lora_", 1)[0] for k in sd})
    for k in sd:
        if not is_lora_key(k):
            raise ValueError(f"LoRA state dict: unexpected key {k!r}")
    for m in mods:
        ka, kb = m + ".lora_A.weight", m + ".lora_B.weight"
        for k in (ka, kb):
            if k not in sd:
                raise ValueError(f"LoRA state dict: {k!r} is missing (its other half is present)")
        a, b = sd[ka], sd[kb]
        if a.dim() != 2 or b.dim() != 2 or a.shape[0] != b.shape[1]:
            raise ValueError(f"LoRA state dict: {ka!r} {tuple(a.shape)} and {kb!r} {tuple(b.shape)} do not share a rank")
        if cfg is not None and a.shape[0] != cfg.rank:
            raise ValueError(f"LoRA state dict: {ka!r} has rank {a.shape[0]}, the configuration says {cfg.rank}")
        if cfg is not None and not cfg.match(m):
            raise ValueError(f"LoRA state dict: {ka!r} adapts a module that target_modules {cfg.target_modules} does not name")
    return mods


def _path(path):
    return os.path.join(path, WEIGHT_NAME) if os.path.isdir(path) or not path.endswith(".safetensors") else path


def save_lora_weights(path, sd):
    """`<path>/pytorch_lora_weights.safetensors` (or `path` itself when it names a .safetensors file) with the `transformer.` key prefix."""
    from safetensors.torch import save_file
    check_adapter({(k[len(PREFIX):] if k.startswith(PREFIX) else k): v for k, v in sd.items()})
    fn = _path(path)
    os.makedirs(os.path.dirname(fn) or ".", exist_ok=True)
    save_file({(k if k.startswith(PREFIX) else PREFIX + k): v.detach().to("cpu").contiguous() for k, v in sd.items()}, fn)
    return fn


def load_lora_weights(path, cfg=None):
    """The adapter of a file written by save_lora_weights / diffusers: keys with or without the `transformer.` prefix are accepted (the reference strips it,
    train_cogvideo_to2v.py:1392-1396); returned under the model's own names.  cfg given: the rank and the targets are checked."""
    from safetensors.torch import load_file
    raw = load_file(_path(path))
    sd = {(k[len(PREFIX):] if k.startswith(PREFIX) else k): v for k, v in raw.items()}
    check_adapter(sd, cfg)
    return sd


def apply_from_config(model, cfg):
    """Honour `use_lora` + `lora_path` + `lora_params` of an infer yaml (gen.yaml / edit.yaml; a dict or an object with those attributes): load the adapter
    and fuse it into `model` (CogVideoXTransformer3DModel.fuse_lora).  Returns True when an adapter was fused."""
    get = cfg.get if isinstance(cfg, dict) else (lambda k, d=None: getattr(cfg, k, d))
    if not get("use_lora", False):
        return False
    path = get("lora_path", None)
    if not path:
        raise ValueError("use_lora is set but lora_path is empty")
    lcfg = LoraConfig.from_params(get("lora_params", {}) or {})
    model.fuse_lora(load_lora_weights(path, lcfg), lcfg)
    return True
