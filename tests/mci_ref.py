"""The definitions of motion-compensated frame interpolation, restated in int64 torch (CPU or device tensors), and the known-answer inputs the CPU and
GPU tests share.  Vectorised over pairs, blocks and pixels, a Python loop over phases and candidates.  The fields come from motion_ref.block_motion.  Not a test module.

Pairs       (t, t + 1) inside a batch item; factor n gives the n - 1 frames at phases k = 1 .. n - 1 between them.
Fields      fwd = block_motion(prev -> next); bwd = block_motion(next -> prev) (bidirectional).
rnd         rnd(k, d, n) = (2 k d + n) // (2 n), floor division: k d / n rounded, halves toward +inf.
Candidates  of block (by, bx): (0, 0), fwd[y][x] and -bwd[y][x] over the 3 x 3 block neighbourhood with clamped indices.  v = (dy, dx) is the motion prev -> next;
            a = (rnd(k, dy, n), rnd(k, dx, n)); the previous-frame block starts at (by block - a_y, bx block - a_x), the next-frame block at that point plus v.
            Admitted only if both blocks lie wholly inside the frame.
Winner      the minimum of (bisad, dy^2 + dx^2, dy, dx), bisad = sum |Y_prev - Y_next| over the two blocks — compared field by field.
Render      pixel row y: c = 2 y + 1 - block, r0 = c // (2 block), f = c - r0 2 block; block rows clamp(r0), clamp(r0 + 1) weigh 2 block - f and f; columns alike.
            Per (row, column) choice with its vector v and a: P = prev[clamp(y - a_y)][clamp(x - a_x)], N = next[clamp(y - a_y + dy)][clamp(x - a_x + dx)];
            out = (sum wy wx ((n - k) P + k N) + D / 2) // D, D = n 4 block^2.

`variant` selects a deliberately wrong rule (the mutation tests): "trunc" (rnd truncates toward 0), "nearest" (no overlap: the pixel's own block alone),
"clamp" (out-of-frame candidates admitted with clamped coordinates)."""
import torch

import motion_ref as MR


def rnd(k, d, n, variant=None):
    """k d / n rounded, halves toward +inf; d an int or an int64 tensor"""
    num = 2 * k * d + n
    if variant == "trunc":
        if isinstance(num, torch.Tensor):
            return torch.div(num, 2 * n, rounding_mode="trunc")
        return int(num / (2 * n))
    return num // (2 * n)


def fields(frames, block, radius, bidirectional=True):
    """frames uint8 [.., T, H, W, 3] -> (fwd, bwd or None), int16 [.., P, Hb, Wb, 2]"""
    prev, nxt = (frames[:-1], frames[1:]) if frames.dim() == 4 else (frames[:, :-1], frames[:, 1:])
    if not bidirectional:
        return MR.block_motion(prev, block, radius, ref=nxt)["mv"], None
    ax = frames.dim() - 4                                     # both directions in one pass over the candidates: pairs (prev, next) then (next, prev)
    mv = MR.block_motion(torch.cat([prev, nxt], ax), block, radius, ref=torch.cat([nxt, prev], ax))["mv"]
    return mv.narrow(ax, 0, prev.shape[ax]), mv.narrow(ax, prev.shape[ax], prev.shape[ax])


def _blocks(plane, ys, xs, block, clamp):
    """plane int64 [P, H, W]; ys, xs int64 [P, Hb, Wb] block origins -> [P, Hb, Wb, block, block]"""
    P, H, W = plane.shape
    i = torch.arange(block, device=plane.device)
    rows = (ys[..., None] + i)[..., :, None].expand(*ys.shape, block, block)
    cols = (xs[..., None] + i)[..., None, :].expand(*ys.shape, block, block)
    if clamp:
        rows, cols = rows.clamp(0, H - 1), cols.clamp(0, W - 1)
    p = torch.arange(P, device=plane.device)[:, None, None, None, None].expand_as(rows)
    return plane[p, rows, cols]


def select_planes(yp, yn, fwd, bwd, n, block, variant=None):
    """yp, yn int64 luma [P, H, W]; fwd, bwd [P, Hb, Wb, 2] -> mvi int16 [P, n - 1, Hb, Wb, 2], cost int32 [P, n - 1, Hb, Wb]"""
    P, H, W = yp.shape
    Hb, Wb = H // block, W // block
    dev = yp.device
    by = torch.arange(Hb, device=dev)[:, None].expand(Hb, Wb)
    bx = torch.arange(Wb, device=dev)[None, :].expand(Hb, Wb)
    cands = [torch.zeros(P, Hb, Wb, 2, dtype=torch.int64, device=dev)]
    for field, sign in ((fwd, 1), (bwd, -1)):
        if field is None:
            continue
        f = sign * field.to(torch.int64)
        for oy in (-1, 0, 1):
            for ox in (-1, 0, 1):
                cands.append(f[:, (by + oy).clamp(0, Hb - 1), (bx + ox).clamp(0, Wb - 1)])
    big = torch.iinfo(torch.int64).max
    mvis, costs = [], []
    for k in range(1, n):
        best = [torch.full((P, Hb, Wb), big, dtype=torch.int64, device=dev) for _ in range(4)]
        for v in cands:
            dy, dx = v[..., 0], v[..., 1]
            py, px = by * block - rnd(k, dy, n, variant), bx * block - rnd(k, dx, n, variant)
            qy, qx = py + dy, px + dx
            legal = (py >= 0) & (py + block <= H) & (px >= 0) & (px + block <= W) & (qy >= 0) & (qy + block <= H) & (qx >= 0) & (qx + block <= W)
            if variant == "clamp":
                legal = torch.ones_like(legal)
            z = torch.zeros_like(py)
            take = lambda t: t if variant == "clamp" else torch.where(legal, t, z)
            sad = (_blocks(yp, take(py), take(px), block, variant == "clamp") - _blocks(yn, take(qy), take(qx), block, variant == "clamp")).abs().sum((3, 4))
            cand = (sad, dy * dy + dx * dx, dy, dx)
            less, equal = torch.zeros_like(legal), torch.ones_like(legal)
            for a, b in zip(cand, best):
                less = less | (equal & (a < b))
                equal = equal & (a == b)
            pick = legal & less
            best = [torch.where(pick, a, b) for a, b in zip(cand, best)]
        mvis.append(torch.stack([best[2], best[3]], -1))
        costs.append(best[0])
    return torch.stack(mvis, 1).to(torch.int16), torch.stack(costs, 1).to(torch.int32)


def _taps(size, nb, block, dev, variant):
    """per pixel row (column): the two block indices [size, 2] and their weights [size, 2]"""
    y = torch.arange(size, device=dev)
    if variant == "nearest":
        own = (y // block).clamp(0, nb - 1)
        return torch.stack([own, own], 1), torch.stack([torch.full_like(y, 2 * block), torch.zeros_like(y)], 1)
    c = 2 * y + 1 - block
    r0 = c // (2 * block)
    f = c - r0 * 2 * block
    return torch.stack([r0.clamp(0, nb - 1), (r0 + 1).clamp(0, nb - 1)], 1), torch.stack([2 * block - f, f], 1)


def render_frames(prev, nxt, mvi, n, block, variant=None):
    """prev, nxt uint8 [P, H, W, 3]; mvi [P, n - 1, Hb, Wb, 2] -> uint8 [P, n - 1, H, W, 3]"""
    P, H, W, _ = prev.shape
    Hb, Wb = H // block, W // block
    dev = prev.device
    p64, n64 = prev.to(torch.int64), nxt.to(torch.int64)
    ry, wy = _taps(H, Hb, block, dev, variant)
    rx, wx = _taps(W, Wb, block, dev, variant)
    y = torch.arange(H, device=dev)[None, :, None]
    x = torch.arange(W, device=dev)[None, None, :]
    pi = torch.arange(P, device=dev)[:, None, None].expand(P, H, W)
    D = n * 4 * block * block
    out = []
    for k in range(1, n):
        acc = torch.zeros(P, H, W, 3, dtype=torch.int64, device=dev)
        for i in range(2):
            for j in range(2):
                v = mvi[:, k - 1].to(torch.int64)[:, ry[:, i]][:, :, rx[:, j]]                 # [P, H, W, 2]
                dy, dx = v[..., 0], v[..., 1]
                sy, sx = y - rnd(k, dy, n, variant), x - rnd(k, dx, n, variant)
                a = p64[pi, sy.clamp(0, H - 1), sx.clamp(0, W - 1)]
                b = n64[pi, (sy + dy).clamp(0, H - 1), (sx + dx).clamp(0, W - 1)]
                w = (wy[:, i][:, None] * wx[:, j][None, :])[None, :, :, None]
                acc += w * ((n - k) * a + k * b)
        out.append((acc + D // 2) // D)
    return torch.stack(out, 1).to(torch.uint8)


def interpolate_frames(frames, factor=2, block=16, radius=16, bidirectional=True, variant=None, field_pair=None):
    """uint8 RGB [F, H, W, 3] / [B, T, H, W, 3] -> {"video" uint8 [.., (T - 1) n + 1, H, W, 3], "mvi" int16 [.., P, n - 1, Hb, Wb, 2], "cost" int32 [.., P, n - 1, Hb, Wb]}
    shaped like tokensgen_amd.motion.interpolate_frames(return_vectors=True)'s.  field_pair: (fwd, bwd) computed before (fields()), to share them between calls."""
    n = factor
    f5 = frames if frames.dim() == 5 else frames[None]
    B, T, H, W, _ = f5.shape
    fwd, bwd = field_pair if field_pair is not None else fields(frames, block, radius, bidirectional)
    flat = lambda t: None if t is None else t.reshape(B * (T - 1), *t.shape[-3:])
    prev, nxt = f5[:, :-1].reshape(-1, H, W, 3), f5[:, 1:].reshape(-1, H, W, 3)
    mvi, cost = select_planes(MR.luma(prev), MR.luma(nxt), flat(fwd), flat(bwd), n, block, variant)
    new = render_frames(prev, nxt, mvi, n, block, variant).reshape(B, T - 1, n - 1, H, W, 3)
    video = torch.empty(B, (T - 1) * n + 1, H, W, 3, dtype=torch.uint8, device=frames.device)
    video[:, ::n] = f5
    for k in range(1, n):
        video[:, k::n] = new[:, :, k - 1]
    mvi, cost = mvi.reshape(B, T - 1, *mvi.shape[1:]), cost.reshape(B, T - 1, *cost.shape[1:])
    if frames.dim() == 4:
        video, mvi, cost = video[0], mvi[0], cost[0]
    return {"video": video, "mvi": mvi, "cost": cost}


def blend(a, b):
    """the plain average (a + b + 1) >> 1 of uint8 frames"""
    return ((a.to(torch.int64) + b.to(torch.int64) + 1) >> 1).to(torch.uint8)


def psnr(a, b):
    """10 log10(1 / (mse + 1e-8)) on the [0, 1] scale, float64, over all of a and b"""
    mse = ((a.to(torch.float64) - b.to(torch.float64)) ** 2).mean() / (255.0 * 255.0)
    return float(10.0 * torch.log10(1.0 / (mse + 1e-8)))


# ---- the known-answer inputs ----

def smooth_canvas(seed, H, W):
    """seeded uint8 noise smoothed by a 5 x 5 box mean (rounded down), RGB [H, W, 3]"""
    g = torch.Generator().manual_seed(seed)
    raw = torch.randint(0, 256, (H + 4, W + 4, 3), generator=g, dtype=torch.uint8).to(torch.int64)
    acc = torch.zeros(H, W, 3, dtype=torch.int64)
    for i in range(5):
        for j in range(5):
            acc += raw[i:i + H, j:j + W]
    return (acc // 25).to(torch.uint8)


def translating_texture(block, step, seed=21):
    """three H x W windows (H = 6 block + 3, W = 8 block + 5) of one smoothed canvas; the content moves by `step` = (sy, sx) per frame: frame t + 1 at
    (y + sy, x + sx) shows what frame t shows at (y, x), and real content enters at the borders.  Returns uint8 [3, H, W, 3]."""
    H, W = 6 * block + 3, 8 * block + 5
    sy, sx = step
    m = 2 * max(abs(sy), abs(sx)) + 1
    canvas = smooth_canvas(seed, H + 2 * m, W + 2 * m)
    return torch.stack([canvas[m - sy * t:m - sy * t + H, m - sx * t:m - sx * t + W] for t in range(3)]).contiguous()


def border_case():
    """24 x 24, block 8, n = 2, and hand-made vectors: block (0, 0) holds (0, 0), its right neighbour (0, 1) holds (-12, -12), so a = (-6, -6) and for the pixels of
    columns 4 .. 11 (which block column 1 weighs in) the next-frame coordinate y + 6 - 12, x + 6 - 12 is negative in the top-left corner: the clamp holds it at 0.
    Returns (frames uint8 [2, 24, 24, 3], mvi int16 [1, 1, 3, 3, 2])."""
    g = torch.Generator().manual_seed(23)
    frames = torch.randint(0, 256, (2, 24, 24, 3), generator=g, dtype=torch.uint8)
    mvi = torch.zeros(1, 1, 3, 3, 2, dtype=torch.int16)
    mvi[0, 0, 0, 1] = torch.tensor([-12, -12], dtype=torch.int16)
    return frames, mvi
