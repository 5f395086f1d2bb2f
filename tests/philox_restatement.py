"""NumPy restatement of the device generator (csrc/sbtv_internal.h, philox_normal_pair): Philox4x32-10 (Salmon, Moraes, Dror,
Shaw, "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 distribution) and Box-Muller on two 53-bit uniforms,
with the counter layout that include/sbtv.h states: pair q of chain b in step s draws counter (q lo, q hi, s, chain_offset + b)
with key (seed lo, seed hi), and fills doubles 2q, 2q + 1 of the chain's state in device memory.  32-bit words travel in uint64
arrays so that the 32 x 32 -> 64 bit products are exact.  Nothing here imports the library."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)           # the round multipliers
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)           # the key schedule (Weyl constants)
MASK = np.uint64(0xFFFFFFFF)
S32, S11 = np.uint64(32), np.uint64(11)


def _words(v):
    return np.atleast_1d(np.asarray(v, dtype=np.uint64)) & MASK


def philox4x32_10(counter4, key2):
    """Ten rounds on counters (c0, c1, c2, c3) under key (k0, k1); every word a uint64 array (broadcast against each other)
    holding a 32-bit value.  Returns the four output words."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[_words(c) for c in counter4])
    k0, k1 = (_words(k) for k in key2)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK, (p0 >> S32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def _sincos_2pi(u):
    """(sin 2 pi u, cos 2 pi u) for u in [0, 1] with the reduction done exactly (2 u = k / 2 + f, |f| <= 1/4), so that the
    result is within a few ulp like the device's sincospi(2 u), not within an ulp of the ARGUMENT 2 pi u."""
    t = 2.0 * u
    k = np.rint(2.0 * t)
    f = t - 0.5 * k
    s, c = np.sin(np.pi * f), np.cos(np.pi * f)
    k = k.astype(np.int64) & 3
    sin = np.choose(k, [s, c, -s, -c])
    cos = np.choose(k, [c, -s, -c, s])
    return sin, cos


def normal_pairs(q, step, chain, seed):
    """The two standard normals of counter (q, step, chain) under `seed` (a 64-bit integer): arrays (z0, z1) of q's shape."""
    q = np.asarray(q, dtype=np.uint64)
    seed = int(seed)
    c0, c1, c2, c3 = philox4x32_10((q & MASK, q >> S32, np.uint64(step), np.uint64(chain)),
                                   (np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)))
    a, b = (c0 << S32) | c1, (c2 << S32) | c3
    u1 = ((a >> S11).astype(np.float64) + 0.5) * 2.0 ** -53        # (0, 1]: 2^53 - 1 + 0.5 rounds to 2^53, on the device too
    u2 = ((b >> S11).astype(np.float64) + 0.5) * 2.0 ** -53
    r = np.sqrt(-2.0 * np.log(u1))
    s, c = _sincos_2pi(u2)
    return (r * c).reshape(q.shape), (r * s).reshape(q.shape)


def chain_normals(n_doubles, steps, chains, seed, chain_offset=0):
    """The normals of `chains` chains of n_doubles (even) doubles each, in device memory order: (steps, chains, n_doubles).
    steps: a count (steps 0 .. steps-1) or the step numbers themselves."""
    assert n_doubles % 2 == 0
    steps = range(steps) if np.ndim(steps) == 0 else list(steps)
    q = np.arange(n_doubles // 2, dtype=np.uint64)
    out = np.empty((len(steps), chains, n_doubles))
    for i, s in enumerate(steps):
        for b in range(chains):
            z0, z1 = normal_pairs(q, s, chain_offset + b, seed)
            out[i, b, 0::2], out[i, b, 1::2] = z0, z1
    return out


def as_arrays(z, M):
    """Device-order normals (..., M * C) as the (..., M, C) arrays that a binding's `noise=` takes: the library stores an image
    or a coefficient array column by column (include/sbtv.h), so double i of a chain is row i % M of column i // M."""
    z = np.asarray(z)
    return np.swapaxes(z.reshape(z.shape[:-1] + (z.shape[-1] // M, M)), -1, -2)


def device_order(x):
    """The inverse of as_arrays: (..., M, C) arrays as (..., M * C) doubles in device memory order."""
    x = np.asarray(x)
    return np.swapaxes(x, -1, -2).reshape(x.shape[:-2] + (-1,))
