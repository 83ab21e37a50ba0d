"""numpy restatement of the R1 / R2 noise generator of `ttv_gp_noise_add` (include/titok_hip.h): Philox4x32-10 on the counter
(element block, draw) under the key (seed), a word -> u = ((x >> 9) + 0.5) 2^-23, words (0, 1) and (2, 3) one Box-Muller pair each,
lanes cos, sin, cos, sin.  The integer part is exact; everything after it is float64 (or `ftype`, for the float32 cross-check).
Not a test module: tests/test_gp_noise_cpu.py and tests/test_hip_gp_noise.py import it."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) of one shape, key: two ints -> four uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in counter]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]                 # 32 x 32 -> 64 bits: no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & MASK, p1 >> np.uint64(32), p1 & MASK
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def unit_open(x, ftype=np.float64):
    """u = ((x >> 9) + 0.5) 2^-23: 24 significant bits, strictly inside (0, 1)."""
    return ((np.asarray(x, dtype=np.uint32) >> np.uint32(9)).astype(ftype) + ftype(0.5)) * ftype(2.0 ** -23)


def clip_offsets(numels):
    """The element offset of every clip with the clips laid end to end, each offset rounded up to a multiple of 4 (no block
    straddles two clips), and the padded total."""
    offs, at = [], 0
    for n in numels:
        at = (at + 3) // 4 * 4
        offs.append(at)
        at += int(n)
    return offs, (at + 3) // 4 * 4


def normals(offset, numel, seed, draw, ftype=np.float64):
    """The standard normals of elements offset .. offset + numel - 1 (offset a multiple of 4) of draw `draw` under `seed`."""
    assert offset % 4 == 0
    blocks = np.arange(offset // 4, (offset + numel + 3) // 4, dtype=np.uint64)
    n_b = len(blocks)
    ctr = [blocks & MASK, blocks >> np.uint64(32), np.full(n_b, draw & 0xFFFFFFFF, np.uint64), np.full(n_b, (draw >> 32) & 0xFFFFFFFF, np.uint64)]
    w = philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    out = np.empty((n_b, 4), dtype=ftype)
    for p in range(2):
        ua, ub = unit_open(w[2 * p], ftype), unit_open(w[2 * p + 1], ftype)
        r = np.sqrt(ftype(-2.0) * np.log(ua))
        ang = ftype(2.0 * np.pi) * ub
        out[:, 2 * p], out[:, 2 * p + 1] = r * np.cos(ang), r * np.sin(ang)
    return out.reshape(-1)[:numel]


def round_bf16(x):
    """float64 -> the nearest bfloat16 (8 significant bits, ties to even), as float64; one rounding."""
    x = np.asarray(x, dtype=np.float64)
    _m, e = np.frexp(x)                                      # x = m 2^e, 0.5 <= |m| < 1
    step = np.ldexp(1.0, np.maximum(e, -125) - 8)            # bf16 normals down to 2^-126
    return np.rint(x / step) * step


def round_f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def noisy(real, offset, seed, draw, gp_noise, dtype):
    """(s, real + s) of one clip in float64: the exact chain, and - for 'bf16' / 'f32' - the reference's rounding steps applied
    to the float64 normals: n to the clip dtype (randn_like), s = n * gp_noise in fp32 then to the clip dtype, the sum likewise."""
    real = np.asarray(real, dtype=np.float64).reshape(-1)
    n = normals(offset, real.size, seed, draw)
    gp = float(np.float32(gp_noise))
    exact_s = n * gp
    rnd = round_bf16 if dtype == "bf16" else round_f32
    s = rnd(round_f32(rnd(n) * gp))
    return exact_s, real + exact_s, s, rnd(round_f32(real + s))
