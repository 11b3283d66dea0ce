"""numpy restatement of the stochastic bf16 rounding of optim.AdamW / AdamW8bit (tg_adamw_step_sr, tg_adamw8bit_step_sr): the Philox4x32-10 counter
generator, the 16 random bits of an arena element and the rounding rule.  The checker of tests/test_sr_*.py; written from the description in
include/tokensgen_hip.h (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11 for the generator), not from the kernel."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # the two round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # the key increments (golden ratio, sqrt(3) - 1)
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: 4 words, key: 2 words (scalars or equal-shaped integer arrays, each < 2^32) -> 4 uint32 arrays.  64-bit products, 10 rounds, the key
    bumped between rounds."""
    c = [np.asarray(x, dtype=np.uint64) & _MASK for x in counter]
    k = [np.asarray(x, dtype=np.uint64) & _MASK for x in key]
    for r in range(10):
        if r:
            k = [(k[0] + np.uint64(W0)) & _MASK, (k[1] + np.uint64(W1)) & _MASK]
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]            # < 2^64: no wrap
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & _MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & _MASK]
    return [x.astype(np.uint32) for x in c]


def r16(seed, step, index):
    """The 16 random bits of arena element `index` (array of non-negative ints) at optimizer step `step` under `seed` (64 bits), as uint32."""
    i = np.asarray(index, dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    g = i >> np.uint64(3)
    w = philox4x32_10((g & _MASK, g >> np.uint64(32), np.full(i.shape, int(step), dtype=np.uint64), np.zeros(i.shape, dtype=np.uint64)),
                      (seed & 0xFFFFFFFF, seed >> 32))
    j = (i & np.uint64(7)).astype(np.int64)
    word = np.choose(j >> 1, w)
    return (word >> (16 * (j & 1)).astype(np.uint32)) & np.uint32(0xFFFF)


def rne_bf16_bits(x_f32):
    """Round-to-nearest-even bf16 bits of fp32 values (NaN stays NaN: the quiet bit is forced)."""
    u = np.asarray(x_f32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    rounded = ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)
    nan = ((u & np.uint64(0x7F800000)) == np.uint64(0x7F800000)) & ((u & np.uint64(0x007FFFFF)) != 0)
    return np.where(nan, ((u >> np.uint64(16)) | np.uint64(0x40)).astype(np.uint16), rounded)


def sr_bf16(x_f32, r16):
    """bf16 bits (uint16) of the fp32 values x rounded stochastically with the 16-bit draws r16.  NaN / Inf: round to nearest even; a carry into the
    all-ones exponent is dropped."""
    x = np.asarray(x_f32, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = np.asarray(r16).astype(np.uint64)
    assert int(r.max(initial=0)) <= 0xFFFF
    exp = np.uint64(0x7F800000)
    s = u + r
    s = np.where((s & exp) == exp, u, s)
    return np.where((u & exp) == exp, rne_bf16_bits(x), (s >> np.uint64(16)).astype(np.uint16))


def bf16_bits_to_f32(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)
