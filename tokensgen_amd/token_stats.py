"""Fitting the T2To token statistics on the GPU: the stage between the To2V and the T2To training runs.  `train_t2to` and `pipeline_t2to` consume
three files (train_cogvideo_t2to.py:1399-1404, 1761-1773; pipeline_cogvideox_t2to.py:698, 891-904): pca.pt (a pickled `pca.PCA` fitted on the
Resampler's condensed tokens, pca.py:40-51), mean.pt and std.pt (the per-coefficient normalisation).  A real token set is millions of rows x 3072, so
the fit streams twice over the data instead of holding it:

    stats = TokenStats(3072, "cuda")
    for tokens, valid in batches: stats.update(tokens, valid)          # pass 1: G += X^T X, colsum += sum X  (tg_gram_accumulate, fp64 totals)
    coef = stats.fit(n_components=16)                                  # eigh of G - n mu mu^T in fp64, once per dataset
    for tokens, valid in batches: coef.update(tokens, valid)           # pass 2: sum / sum of squares / signed extreme of y = (X - mu) V^T
    coef.finalize().save(out_dir)                                      # signs as pca.py:30-32, pooled mean / unbiased std -> pca.pt, mean.pt, std.pt

The totals are plain fp64 tensors: `merge` / `all_reduce` add them (several loaders or ranks), `state_dict` checkpoints them, and `fit` / `finalize`
run wherever the totals live, the CPU included.  `update` is the hot path and has no CPU fallback.

Stated deviation: the reference ships mean.pt / std.pt without the recipe that made them (calculate_vae_latents.py:1867-1878 survives as comments and
averages per video, for the per-channel mode).  Here they are the statistics pooled over all valid token rows of `pca.transform(X)`, std unbiased:
exactly what makes `pca_normalization`'s output zero-mean and unit-variance per coefficient."""
import os
import pickle
import types

import torch

from . import kernels as K
from . import lib as L
from .pca import PCA

BF16 = torch.bfloat16
F64 = torch.float64


def _row_blocks(tokens, valid_chunks, num_temporal_queries, grid):
    """tokens -> list of bf16 [rows, C] blocks (contiguous rows) holding the valid token rows: all of them, or per item b the rows of its first
    valid_chunks[b] * num_temporal_queries frames (train_cogvideo_t2to.py's `valid_num_chunks` masking)."""
    K._chk(tokens, "tokens")
    if tokens.dim() == 5:
        B, F, C, h, w = tokens.shape
        rows = tokens.permute(0, 1, 3, 4, 2).reshape(B, F * h * w, C).contiguous()
        hw = h * w
    elif tokens.dim() == 3:
        if grid is None:
            raise ValueError("token-major input [B, n, C] needs grid=(frames, h, w)")
        F, h, w = grid
        B, n, C = tokens.shape
        if n != F * h * w:
            raise ValueError(f"tokens have {n} rows per item, grid {tuple(grid)} needs {F * h * w}")
        rows, hw = tokens.contiguous(), h * w
    else:
        raise ValueError(f"tokens: expected [B, F, C, h, w] or [B, n, C], got {tuple(tokens.shape)}")
    if valid_chunks is None:
        return [rows.reshape(-1, C)]
    valid = [int(v) for v in (valid_chunks.tolist() if torch.is_tensor(valid_chunks) else valid_chunks)]
    if len(valid) != B or not all(0 <= v * num_temporal_queries <= F for v in valid):
        raise ValueError(f"valid_chunks {valid}: need {B} counts with count * {num_temporal_queries} frames in 0..{F}")
    return [rows[b, :v * num_temporal_queries * hw] for b, v in enumerate(valid) if v > 0]


class _Totals:
    """fp64 running totals + a row count: SUM-merged, all-reduced and checkpointed as a unit."""
    _tensors = ()

    def merge(self, other):
        if type(other) is not type(self) or other.dim != self.dim:
            raise ValueError(f"merge: {type(other).__name__} of width {getattr(other, 'dim', None)} into {type(self).__name__} of width {self.dim}")
        for name in self._tensors:
            getattr(self, name).add_(getattr(other, name).to(self.device))
        self.n += other.n
        return self

    def all_reduce(self, group=None):
        """SUM over the ranks of `group` (every rank ends with the whole data set's totals)."""
        import torch.distributed as dist
        n = torch.tensor([self.n], dtype=torch.int64, device=self.device)
        for t in [getattr(self, name) for name in self._tensors] + [n]:
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
        self.n = int(n.item())
        return self


class TokenStats(_Totals):
    """Pass 1: n, colsum [D] and the Gram matrix X^T X [D, D] of the valid token rows, fp64."""
    _tensors = ("gram", "colsum")

    def __init__(self, dim, device="cuda"):
        self.dim, self.device = int(dim), torch.device(device)
        self.gram = torch.zeros(self.dim, self.dim, dtype=F64, device=self.device)
        self.colsum = torch.zeros(self.dim, dtype=F64, device=self.device)
        self.n = 0

    @torch.no_grad()
    def update(self, tokens, valid_chunks=None, num_temporal_queries=4, grid=None):
        blocks = _row_blocks(tokens, valid_chunks, num_temporal_queries, grid)
        if self.gram.device != tokens.device:
            raise RuntimeError(f"TokenStats.update: the totals live on {self.gram.device}, the tokens on {tokens.device} (update runs on the GPU)")
        lib = L.load()
        for x in blocks:
            if x.shape[1] != self.dim:
                raise ValueError(f"tokens of width {x.shape[1]} into TokenStats of width {self.dim}")
            L.check(K._launch("gram_accumulate", lib.tg_gram_accumulate, x.data_ptr(), x.stride(0), x.shape[0], self.dim, self.gram.data_ptr(),
                              self.colsum.data_ptr(), K._stream()), "tg_gram_accumulate")
            self.n += x.shape[0]
        return self

    def state_dict(self):
        return {"n": self.n, "gram": self.gram, "colsum": self.colsum, "dim": self.dim}

    def load_state_dict(self, sd):
        if int(sd["dim"]) != self.dim:
            raise ValueError(f"state dict of width {int(sd['dim'])} into TokenStats of width {self.dim}")
        self.gram.copy_(sd["gram"])
        self.colsum.copy_(sd["colsum"])
        self.n = int(sd["n"])
        return self

    @torch.no_grad()
    def fit(self, n_components=None):
        """pca.py:40-51 from the totals: mean_ = colsum / n, components_ = the top eigenvectors of the scatter matrix G - n mu mu^T (the right singular
        vectors of the centred data), fp64 eigh, descending.  The signs are fixed by CoefficientStats.finalize (they need the second pass)."""
        if self.n < 2:
            raise ValueError(f"fit: {self.n} rows seen")
        d = self.dim if n_components is None else min(int(n_components), self.dim)
        mu = self.colsum / self.n
        scatter = self.gram - self.n * torch.outer(mu, mu)
        scatter = (scatter + scatter.T) * 0.5
        _, vec = torch.linalg.eigh(scatter)                              # ascending
        comp = vec[:, -d:].flip(1).T.contiguous()
        pca = PCA(d)
        pca.register_buffer("mean_", mu.to(torch.float32)[None].contiguous())
        pca.register_buffer("components_", comp.to(torch.float32))
        coef = CoefficientStats(pca, self.device)
        coef.mean64, coef.components64 = mu, comp                       # what eigh gave, before the rounding to the holder's fp32
        return coef


class CoefficientStats(_Totals):
    """Pass 2 over the same rows: per component j of `pca`, sum and sum of squares of y_j = (x - mean_) . components_[j] (fp64) and the signed y_j of
    largest magnitude (tg_pca_coef_stats)."""
    _tensors = ("sum", "sumsq")

    def __init__(self, pca, device="cuda"):
        self.pca, self.device = pca, torch.device(device)
        self.dim = pca.components_.shape[1]
        self.d = d = pca.components_.shape[0]
        self.sum = torch.zeros(d, dtype=F64, device=self.device)
        self.sumsq = torch.zeros(d, dtype=F64, device=self.device)
        self.extreme = torch.zeros(d, dtype=torch.float32, device=self.device)
        self.n = 0
        self._dev = None

    def _operands(self):
        """components_ padded with zero rows to the kernel's multiple of 16, mean_, and padded totals, on the device."""
        if self._dev is None:
            if self.d > 64:
                raise ValueError(f"CoefficientStats.update: {self.d} components (tg_pca_coef_stats takes at most 64)")
            nc = -(-self.d // 16) * 16
            comp = torch.zeros(nc, self.dim, dtype=torch.float32, device=self.device)
            comp[:self.d] = self.pca.components_.to(self.device, torch.float32)
            self._dev = (comp, self.pca.mean_.reshape(-1).to(self.device, torch.float32).contiguous(), nc)
        return self._dev

    @torch.no_grad()
    def update(self, tokens, valid_chunks=None, num_temporal_queries=4, grid=None):
        blocks = _row_blocks(tokens, valid_chunks, num_temporal_queries, grid)
        if self.sum.device != tokens.device:
            raise RuntimeError(f"CoefficientStats.update: the totals live on {self.sum.device}, the tokens on {tokens.device} (update runs on the GPU)")
        lib = L.load()
        comp, pmean, nc = self._operands()
        s, s2, ex = (torch.zeros(nc, dtype=t.dtype, device=self.device) for t in (self.sum, self.sumsq, self.extreme))
        s[:self.d], s2[:self.d], ex[:self.d] = self.sum, self.sumsq, self.extreme
        for x in blocks:
            if x.shape[1] != self.dim:
                raise ValueError(f"tokens of width {x.shape[1]} into CoefficientStats of width {self.dim}")
            ws = torch.empty(lib.tg_pca_coef_stats_ws_floats(x.shape[0], nc), dtype=torch.float32, device=self.device)
            L.check(K._launch("pca_coef_stats", lib.tg_pca_coef_stats, x.data_ptr(), x.stride(0), x.shape[0], self.dim, comp.data_ptr(), nc, pmean.data_ptr(),
                              s.data_ptr(), s2.data_ptr(), ex.data_ptr(), ws.data_ptr(), K._stream()), "tg_pca_coef_stats")
            self.n += x.shape[0]
        self.sum, self.sumsq, self.extreme = s[:self.d].clone(), s2[:self.d].clone(), ex[:self.d].clone()
        return self

    def merge(self, other):
        if isinstance(other, CoefficientStats) and (other.d != self.d or not torch.equal(other.pca.components_.cpu(), self.pca.components_.cpu())
                                                    or not torch.equal(other.pca.mean_.cpu(), self.pca.mean_.cpu())):
            raise ValueError("merge: the two CoefficientStats were accumulated against different fits (components_ / mean_ differ)")
        super().merge(other)
        theirs = other.extreme.to(self.device)
        self.extreme = torch.where(theirs.abs() > self.extreme.abs(), theirs, self.extreme)
        return self

    def all_reduce(self, group=None):
        """SUM of the sums; the extreme of largest magnitude over the ranks (ties: the positive one, on every rank alike)."""
        import torch.distributed as dist
        super().all_reduce(group)
        hi, lo = self.extreme.clone(), self.extreme.clone()
        dist.all_reduce(hi, op=dist.ReduceOp.MAX, group=group)
        dist.all_reduce(lo, op=dist.ReduceOp.MIN, group=group)
        self.extreme = torch.where(hi >= -lo, hi, lo)
        return self

    def state_dict(self):
        return {"n": self.n, "sum": self.sum, "sumsq": self.sumsq, "extreme": self.extreme, "dim": self.dim}

    def load_state_dict(self, sd):
        if int(sd["dim"]) != self.dim or sd["sum"].numel() != self.d:
            raise ValueError(f"state dict of width {int(sd['dim'])} x {sd['sum'].numel()} into CoefficientStats of width {self.dim} x {self.d}")
        self.sum.copy_(sd["sum"])
        self.sumsq.copy_(sd["sumsq"])
        self.extreme.copy_(sd["extreme"])
        self.n = int(sd["n"])
        return self

    @torch.no_grad()
    def finalize(self):
        """pca.py:30-38 `_svd_flip(u_based_decision=True)`: component j takes the sign of the entry of largest magnitude of its left singular vector
        u[:, j] = y[:, j] / s_j, i.e. of `extreme[j]`; the coefficient mean flips with it.  mean / std: pooled over the valid rows, std unbiased."""
        if self.n < 2:
            raise ValueError(f"finalize: {self.n} rows seen")
        sign = torch.where(self.extreme < 0, -1.0, 1.0).to(F64).cpu()
        s, s2 = self.sum.cpu(), self.sumsq.cpu()
        mean = sign * s / self.n
        var = ((s2 - s * s / self.n) / (self.n - 1)).clamp_min(0.0)
        pca = PCA(self.d)
        pca.register_buffer("mean_", self.pca.mean_.detach().cpu().clone())
        pca.register_buffer("components_", (self.pca.components_.detach().cpu().to(F64) * sign[:, None]).to(torch.float32))
        return TokenNorm(pca, mean.to(torch.float32), var.sqrt().to(torch.float32))


class _PcaPickler(pickle._Pickler):
    """Writes the class global of tokensgen_amd.pca.PCA as `pca PCA`, the name the reference's pickles carry (compat.ensure_pca_module resolves it here,
    the reference's own pca.py there); everything else is the stock pickler."""

    def save_global(self, obj, name=None):
        if obj is PCA:
            self.write(pickle.GLOBAL + b"pca\nPCA\n")
            self.memoize(obj)
        else:
            super().save_global(obj, name)


_pca_pickle = types.ModuleType("tokensgen_amd._pca_pickle")             # what torch.save(pickle_module=) wants: a module with a Pickler
_pca_pickle.__dict__.update({k: v for k, v in vars(pickle).items() if not k.startswith("__")})
_pca_pickle.Pickler = _PcaPickler


class TokenNorm:
    """The three files of the T2To stage: pca (a fitted pca.PCA: mean_ [1, D], components_ [d, D], fp32), mean / std fp32 [d]."""

    def __init__(self, pca, mean, std):
        self.pca, self.mean, self.std = pca, mean, std

    def save(self, directory):
        """pca.pt is a pickle of the whole module whose class global reads `pca PCA`: what the reference's `torch.load(pca_path)` resolves with its own
        pca.py on the path (and tokensgen_amd.compat here); mean.pt / std.pt are plain tensors (`weights_only=True` loads them).  The class name is
        written by the pickler (_PcaPickler): nothing process-wide (PCA.__module__, sys.modules) is touched, so concurrent saves and imports are safe."""
        os.makedirs(directory, exist_ok=True)
        holder = PCA(self.pca.n_components)
        holder.register_buffer("mean_", self.pca.mean_.detach().cpu().to(torch.float32).clone())
        holder.register_buffer("components_", self.pca.components_.detach().cpu().to(torch.float32).clone())
        torch.save(holder, os.path.join(directory, "pca.pt"), pickle_module=_pca_pickle)
        torch.save(self.mean.detach().cpu().to(torch.float32).clone(), os.path.join(directory, "mean.pt"))
        torch.save(self.std.detach().cpu().to(torch.float32).clone(), os.path.join(directory, "std.pt"))
        return directory

    @classmethod
    def load(cls, directory):
        from . import compat
        compat.ensure_pca_module()
        pca = torch.load(os.path.join(directory, "pca.pt"), map_location="cpu", weights_only=False)
        if not hasattr(pca, "components_") or not hasattr(pca, "mean_"):
            raise ValueError(f"{directory}/pca.pt: expected a fitted pca.PCA (buffers mean_, components_)")
        return cls(pca, torch.load(os.path.join(directory, "mean.pt"), map_location="cpu", weights_only=True),
                   torch.load(os.path.join(directory, "std.pt"), map_location="cpu", weights_only=True))
