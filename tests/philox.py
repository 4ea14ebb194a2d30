"""numpy restatement of the library's random numbers (csrc/ccmm_internal.h: philox4x32_10, u01, Rng::raw,
Rng::normal), for tests that run a kernel on its own Philox draws and need the same numbers on the host.

Philox4x32-10 (Salmon et al. 2011): counter (idx >> 1, chain, sweep, block), key = the 64-bit seed (low word,
high word); one call gives two doubles.  A normal is Box-Muller on the call's two uniforms: the even index takes
the cosine, the odd one the sine.  tests/test_launch_plans.py (test_philox_words_bit_for_bit)
pins the integer part bit for bit to the library's own host function and to the published Random123 known answers."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Ten rounds on the counter words (arrays or scalars, broadcast together) with key (k0, k1).  Returns the
    four output words as uint64 arrays holding 32-bit values."""
    c = [np.asarray(x, np.uint64) & MASK for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]  # 32 x 32 -> 64 bits: no overflow
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & MASK, p1 >> np.uint64(32), p1 & MASK
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0 = (k0 + np.uint64(W0)) & MASK
        k1 = (k1 + np.uint64(W1)) & MASK
    return c


def raw(seed, chain, sweep, block, pair):
    """Rng::raw(block, pair) of a generator with this seed, chain and sweep."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return philox4x32_10(pair, chain, sweep, block, seed & 0xFFFFFFFF, seed >> 32)


def u01(lo, hi):
    """Uniform in (0, 1) from two 32-bit words: the top 53 bits of hi:lo, plus a half, times 2^-53."""
    v = ((np.asarray(hi, np.uint64) << np.uint64(32)) | np.asarray(lo, np.uint64)) >> np.uint64(11)
    return (v.astype(np.float64) + 0.5) * 1.1102230246251565404e-16


def normal(seed, chain, sweep, block, idx):
    """Rng::normal(block, idx): Box-Muller on the two uniforms of call idx >> 1."""
    idx = np.asarray(idx, np.uint64) & MASK
    x, y, z, w = raw(seed, chain, sweep, block, idx >> np.uint64(1))
    u1, u2 = u01(x, y), u01(z, w)
    rad = np.sqrt(-2.0 * np.log(u1))
    ang = 2.0 * np.pi * u2
    return np.where(idx & np.uint64(1), rad * np.sin(ang), rad * np.cos(ang))


GIRF_BLOCK_Z, GIRF_BLOCK_SVZ = 9, 10


def girf_normals(seed, M, N, H, nsim):
    """The normals ccmm_girf draws for itself (csrc/ccmm_girf.hip: z == nullptr): block 9 for z, block 10 for the
    SV normals, index (nn H + h) N + i, chain = the kept draw, sweep 0.  Returns z, svz in the drop-in's layout
    N x H x nsim x M."""
    i, h, nn, m = np.meshgrid(np.arange(N), np.arange(H), np.arange(nsim), np.arange(M), indexing="ij")
    idx = (nn * H + h) * N + i
    return (normal(seed, m, 0, GIRF_BLOCK_Z, idx), normal(seed, m, 0, GIRF_BLOCK_SVZ, idx))


PHI_BLOCK = 5  # CCMM_RNG_PHI (include/ccmm.h)


def phi_normals(seed, B, N, T, dPHI, sweep=0):
    """The normals k_phi_gen draws for the inverse-Wishart block (csrc/ccmm_kernels.hip): block CCMM_RNG_PHI, index
    i + N col of the N x (T + dPHI) column-major matrix, the chain as the chain word.  The block-level drop-in
    ccmm_phi_iw with Zdraw == NULL runs seed 0 at sweep 0 (ccmm_dropins.hip: block_cfg, crn_args).  Returns Z in the
    drop-in's layout N x (T + dPHI) x B."""
    i, col, c = np.meshgrid(np.arange(N), np.arange(T + dPHI), np.arange(B), indexing="ij")
    return normal(seed, c, sweep, PHI_BLOCK, i + N * col)
