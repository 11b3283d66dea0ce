"""The definitions of block-matching motion estimation and of the warp error, restated in int64 torch (CPU or device tensors), and the known-answer inputs the CPU and
GPU tests share.  Vectorised over pairs and blocks, a Python loop over the candidates.  Not a test module.

Luma        Y = (77 R + 150 G + 29 B + 128) >> 8.
Blocks      tile the frame from the top left, Hb = H // block, Wb = W // block.
Candidates  integer (dy, dx), |dy|, |dx| <= R, with the displaced block wholly inside the other frame.
Winner      the minimum of (sad, dy^2 + dx^2, dy, dx) in lexicographic order — compared here field by field, not through a packed key.
Warp error  sse = sum over block and channels of (cur - ref displaced)^2, sse0 at zero displacement; a displaced origin outside the frame is clamped and counted.

`variant` selects a deliberately wrong rule (the mutation tests): "luma_no_round", "l1", "raster", "clamp"."""
import torch
import torch.nn.functional as F


def luma(frames, variant=None):
    f = frames.to(torch.int64)
    return (77 * f[..., 0] + 150 * f[..., 1] + 29 * f[..., 2] + (0 if variant == "luma_no_round" else 128)) >> 8


def block_motion_planes(cur, ref, block, radius, variant=None):
    """cur, ref: int64 luma [P, H, W] -> mv int16 [P, Hb, Wb, 2], sad int32 [P, Hb, Wb], sad0 int32"""
    P, H, W = cur.shape
    Hb, Wb = H // block, W // block
    dev = cur.device
    R = radius
    c = cur[:, :Hb * block, :Wb * block]
    if variant == "clamp":
        pad = F.pad(ref[:, None].to(torch.float64), (R, R, R, R), mode="replicate")[:, 0].to(torch.int64)
    else:
        pad = F.pad(ref, (R, R, R, R))
    ys = torch.arange(Hb, device=dev)[:, None] * block
    xs = torch.arange(Wb, device=dev)[None, :] * block
    big = torch.iinfo(torch.int64).max
    best = [torch.full((P, Hb, Wb), big, dtype=torch.int64, device=dev) for _ in range(4)]
    sad0 = None
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            shifted = pad[:, R + dy:R + dy + Hb * block, R + dx:R + dx + Wb * block]
            sad = (c - shifted).abs().reshape(P, Hb, block, Wb, block).sum((2, 4))
            if dy == 0 and dx == 0:
                sad0 = sad
            legal = ((ys + dy >= 0) & (ys + dy + block <= H) & (xs + dx >= 0) & (xs + dx + block <= W))[None].expand(P, Hb, Wb)
            if variant == "clamp":
                legal = torch.ones_like(legal)
            dist = abs(dy) + abs(dx) if variant == "l1" else dy * dy + dx * dx
            cand = (sad, torch.full_like(sad, 0 if variant == "raster" else dist), torch.full_like(sad, dy), torch.full_like(sad, dx))
            less = torch.zeros_like(legal)
            equal = torch.ones_like(legal)
            for a, b in zip(cand, best):
                less = less | (equal & (a < b))
                equal = equal & (a == b)
            take = legal & less
            best = [torch.where(take, a, b) for a, b in zip(cand, best)]
    mv = torch.stack([best[2], best[3]], -1).to(torch.int16)
    return mv, best[0].to(torch.int32), sad0.to(torch.int32)


def _pairs(frames, ref):
    """[.., n, H, W, ..] -> (cur, other) flattened over the leading axes, pairs (t, t + 1) inside a batch item, or (t, t) with ref"""
    if ref is None:
        cur, oth = (frames[:-1], frames[1:]) if frames.dim() == 4 else (frames[:, :-1], frames[:, 1:])
    else:
        cur, oth = frames, ref
    lead = cur.shape[:-3]
    return cur.reshape(-1, *cur.shape[-3:]), oth.reshape(-1, *oth.shape[-3:]), lead


def block_motion(frames, block=16, radius=16, ref=None, variant=None):
    """uint8 RGB [F, H, W, 3] / [B, T, H, W, 3] -> {"mv", "sad", "sad0"} shaped like tokensgen_amd.motion.block_motion's"""
    cur, oth, lead = _pairs(frames, ref)
    mv, sad, sad0 = block_motion_planes(luma(cur, variant), luma(oth, variant), block, radius, variant)
    return {"mv": mv.reshape(*lead, *mv.shape[1:]), "sad": sad.reshape(*lead, *sad.shape[1:]), "sad0": sad0.reshape(*lead, *sad0.shape[1:])}


def warp_sse(frames, mv, block, ref=None):
    """{"sse", "sse0"} int32 [.., P, Hb, Wb] and "status": the number of vectors whose displaced origin had to be clamped into the frame"""
    cur, oth, lead = _pairs(frames, ref)
    P, H, W, _ = cur.shape
    Hb, Wb = H // block, W // block
    dev = cur.device
    v = mv.reshape(P, Hb, Wb, 2).to(torch.int64)
    ys = (torch.arange(Hb, device=dev) * block)[None, :, None]
    xs = (torch.arange(Wb, device=dev) * block)[None, None, :]
    ty, tx = ys + v[..., 0], xs + v[..., 1]
    ry, rx = ty.clamp(0, H - block), tx.clamp(0, W - block)
    status = ((ry != ty) | (rx != tx)).sum().to(torch.int32).reshape(1)
    i = torch.arange(block, device=dev)
    rows = (ry[..., None] + i)[..., :, None].expand(P, Hb, Wb, block, block)
    cols = (rx[..., None] + i)[..., None, :].expand(P, Hb, Wb, block, block)
    pidx = torch.arange(P, device=dev)[:, None, None, None, None].expand_as(rows)
    c64, o64 = cur.to(torch.int64), oth.to(torch.int64)
    tiles = lambda t: t[:, :Hb * block, :Wb * block].reshape(P, Hb, block, Wb, block, 3).permute(0, 1, 3, 2, 4, 5)
    a = tiles(c64)
    sse0 = ((a - tiles(o64)) ** 2).sum((3, 4, 5))
    sse = ((a - o64[pidx, rows, cols]) ** 2).sum((3, 4, 5))
    return {"sse": sse.to(torch.int32).reshape(*lead, Hb, Wb), "sse0": sse0.to(torch.int32).reshape(*lead, Hb, Wb), "status": status}


# ---- the known-answer inputs: name -> (frames uint8 [2, H, W, 3], block, radius) ----

def gray(y):
    """uint8 [.., H, W] -> RGB with R = G = B, whose luma is the value itself: (256 v + 128) >> 8 = v"""
    return y[..., None].expand(*y.shape, 3).contiguous()


def shifted_texture():
    """two 43 x 61 windows of one random RGB image: cur[y, x] = ref[y + 3, x - 5]; every block with x >= 8 has mv (3, -5), sad 0"""
    g = torch.Generator().manual_seed(11)
    img = torch.randint(0, 256, (64, 80, 3), generator=g, dtype=torch.uint8)
    img[::3, ::5] = 0                                     # plenty of zero bytes in the reference: a masked SAD would skip them
    ref = img[8:8 + 43, 5:5 + 61]
    cur = img[11:11 + 43, 0:0 + 61]                       # ref[y + 3, x - 5] = img[11 + y, x] = cur[y, x]
    return torch.stack([cur, ref]).contiguous(), 8, 7


def constant_frames():
    return torch.full((2, 24, 40, 3), 93, dtype=torch.uint8), 8, 5


def black_white():
    f = torch.zeros(2, 16, 16, 3, dtype=torch.uint8)
    f[1] = 255
    return f, 16, 16


def stripes():
    """period-4 vertical stripes, the second frame shifted right by one pixel: dx = 1, -3, 5 (and every dy) cost nothing"""
    x = torch.arange(48)
    vals = torch.tensor([10, 200, 90, 250], dtype=torch.uint8)
    cur = vals[x % 4][None].expand(32, 48)
    ref = vals[(x - 1) % 4][None].expand(32, 48)
    return gray(torch.stack([cur, ref])), 8, 6


def hand_built():
    """24 x 24, block 8, radius 3.  Centre block: one bright pixel against a plus of four: (-1, 0), (0, -1), (0, 1), (1, 0) tie at 600 (one match, three strays), every
    other candidate costs more or lies farther.  Top-left block: flat 77 against a 5 x 5 corner of 77: only a search that admitted out-of-frame candidates with
    clamped coordinates would find a free match at (-3, -3)."""
    cur = torch.zeros(24, 24, dtype=torch.uint8)
    ref = torch.zeros(24, 24, dtype=torch.uint8)
    cur[12, 12] = 200
    for y, x in ((11, 12), (13, 12), (12, 11), (12, 13)):
        ref[y, x] = 200
    cur[0:8, 0:8] = 77
    ref[0:5, 0:5] = 77
    return gray(torch.stack([cur, ref])), 8, 3


def diagonal_stripes():
    """40 x 40, block 8, radius 4: T[y, x] = v[(x - y) % 8] against itself shifted right by 4: zero cost wherever dx - dy = 4 (mod 8).  The squared distance picks
    (-2, 2) (8; its twin (2, -2) has the larger dy); |dy| + |dx| would tie (-4, 0), (-3, 1), ... at 4 and pick (-4, 0)."""
    y, x = torch.arange(40)[:, None], torch.arange(40)[None, :]
    vals = torch.tensor([0, 31, 250, 77, 140, 9, 201, 110], dtype=torch.uint8)
    cur = vals[(x - y) % 8]
    ref = vals[(x - 4 - y) % 8]
    return gray(torch.stack([cur, ref])), 8, 4


KNOWN = {"shifted_texture": shifted_texture, "constant_frames": constant_frames, "black_white": black_white, "stripes": stripes, "hand_built": hand_built,
         "diagonal_stripes": diagonal_stripes}
