"""TEST INFRASTRUCTURE -- numpy restatement of Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as
easy as 1, 2, 3", SC'11; the Random123 library's philox4x32 with 10 rounds), the generator behind the product's
device-side noise (`ssn_philox_uniform_*`, tc_gan_amd/csrc/ssn_aux.hip).  The reference has no device noise (its z is
`rng.rand` on the host, tc_gan/networks/ssn.py:434-439), so this is pinned by the published known-answer vectors
(tests/test_noise.py), not by the reference.  `uniform` is the scalar statement of the stream; `uniform_vec` the same stream on
uint64 arrays (held to `uniform` by tests/test_philox_inputs.py), and `device_inputs_noise` what the one-launch inputs of a
device-noise forward draw from it (tests/test_device_inputs_gpu.py).  Only tests/ may import this module."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: 4 words, key: 2 words (Python ints) -> 4 output words."""
    c0, c1, c2, c3 = (int(c) & MASK for c in counter)
    k0, k1 = (int(k) & MASK for k in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        hi0, lo0 = p0 >> 32, p0 & MASK
        hi1, lo1 = p1 >> 32, p1 & MASK
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def uniform(seed, offset, n):
    """The stream of ssn_philox_uniform_*: element g = word g % 4 of the block with counter (g // 4, 0, 0, 0) and key
    (seed & 0xffffffff, seed >> 32); value = (word >> 8) / 2^24 as float32."""
    out = np.empty(n, dtype=np.float32)
    key = (seed & MASK, (seed >> 32) & MASK)
    cache = {}
    for i in range(n):
        g = offset + i
        blk = g // 4
        if blk not in cache:
            cache = {blk: philox4x32_10((blk & MASK, blk >> 32, 0, 0), key)}
        out[i] = np.float32(cache[blk][g % 4] >> 8) * np.float32(1.0 / 16777216.0)
    return out


def philox4x32_10_vec(c0, c1, key):
    """`philox4x32_10` of the counters (c0[i], c1[i], 0, 0): uint64 arrays holding 32-bit words in, an (n, 4) uint64 array of
    output words out.  Every product is of two 32-bit words, so it fits the 64 bits it is formed in."""
    m = np.uint64(MASK)
    s32 = np.uint64(32)
    c0, c1 = np.asarray(c0, dtype=np.uint64) & m, np.asarray(c1, dtype=np.uint64) & m
    c2, c3 = np.zeros_like(c0), np.zeros_like(c0)
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & m, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & m
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack([c0, c1, c2, c3], axis=1)


def uniform_vec(seed, offset, n):
    """`uniform`, vectorised: the same counter and key layout, one Philox block per four stream elements (uint64 arrays; the
    stream position is a Python int until it is split into the two counter words)."""
    seed, offset, n = int(seed), int(offset), int(n)
    if n == 0:
        return np.empty(0, dtype=np.float32)
    first, last = offset // 4, (offset + n + 3) // 4                     # Philox blocks touched
    blk = np.uint64(first) + np.arange(last - first, dtype=np.uint64)
    words = philox4x32_10_vec(blk & np.uint64(MASK), blk >> np.uint64(32), (seed & MASK, (seed >> 32) & MASK))
    lo = offset - 4 * first
    bits = (words.reshape(-1)[lo:lo + n] >> np.uint64(8)).astype(np.float32)        # (24 bits: exact in float32)
    return bits * np.float32(1.0 / 16777216.0)


def signs_and_amp(seed, off_zin, v, bernoulli, B, M):
    """zin[B][M] = +1 where u < 0.5 and -1 otherwise (`bernoulli`) or 2 u - 1 (exact in float32: u is a multiple of 2^-24) of
    stream elements off_zin.., and amp = 1 + v zin as the two float32 operations of the torch expression
    `1 + vs[None, :] * zin` (networks/ssn.py): the product is rounded before the sum.  Both float32."""
    u = uniform_vec(seed, off_zin, B * M).reshape(B, M)
    one = np.float32(1)
    zin = np.where(u < np.float32(0.5), one, -one).astype(np.float32) if bernoulli else u * np.float32(2) - one
    v32 = np.asarray(v, dtype=np.float32).reshape(M)
    prod = v32[None, :] * zin
    amp = one + prod
    assert zin.dtype == prod.dtype == amp.dtype == np.float32
    return zin, amp


def device_inputs_noise(seed, off_z, off_zin, v, bernoulli, B, N):
    """The noise outputs of `ssn_gen_inputs_philox_f32` (include/ssnode_mi355x.h): z[B][2N][2N] = stream elements off_z.., and
    with `v` (2N values; None: no heterogeneous input, zin = amp = None) `signs_and_amp` of stream elements off_zin...  float32."""
    M = 2 * int(N)
    z = uniform_vec(seed, off_z, B * M * M).reshape(B, M, M)
    if v is None:
        return z, None, None
    return (z,) + signs_and_amp(seed, off_zin, v, bernoulli, B, M)


def amp_rounded_once(v, zin):
    """1 + v zin rounded ONCE to float32 (what one fused multiply-add gives), for float32 v >= 2^-5 and zin a multiple of 2^-23
    in [-1, 1]: v is then a multiple of 2^-28 below 1, the product a multiple of 2^-51 below 1 in magnitude, and 1 + product a
    multiple of 2^-51 below 2 -- 52 bits, so both float64 operations are exact and the only rounding is the cast."""
    v64 = np.asarray(v, dtype=np.float32).astype(np.float64)
    z64 = np.asarray(zin, dtype=np.float32).astype(np.float64)
    assert v64.min() >= 2.0 ** -5 and v64.max() < 1.0 and np.abs(z64).max() <= 1.0
    assert np.array_equal(z64 * 2.0 ** 23, np.round(z64 * 2.0 ** 23))
    return (1.0 + v64[None, :] * z64).astype(np.float32)
