"""Cases, inputs and cached references of the PHI draw for N <= 32 (k_phi_gen / k_phi, csrc/ccmm_kernels.hip),
shared by tests/test_gpu_phi_edges.py (device), tests/test_refs.py (conditioning of every case, CPU) and
tests/test_launch_plans.py (phi_plan of csrc/ccmm_sweep.h held to the restatement below).

k_phi stages its two sources in LDS when they fit one CU (phi_plan): eta and Z (plan 3), eta only (1), nothing
(0).  A staging loop moves sixteen loads per thread, 16 x 256 = 4096 doubles a round: N TP doubles of eta (row
stride TP + 1 in LDS), then N (T + dPHI) doubles of Z into the region eta has been read from.  Both Gram loops
keep four partial sums with a remainder loop for T mod 4 and (T + dPHI) mod 4.  Each table entry names the edge
it sits on; the plan beside it is computed here and asserted below, and held to the library on the CPU.

The kernel takes any dPHI >= 0 (more Wishart degrees of freedom); the prior scale sPHI is the toy prior's, which
depends on N alone.  Every case keeps T + dPHI >= 2 N, so that Z Z' is well conditioned.
"""
import functools

import numpy as np

import refs
from helpers import toy_setup
from oracle import ccmm_oracle as O

LDS_CU = 160 * 1024
ROUND = 16 * 256  # doubles one staging round moves

# (N, T, dPHI) -> plan
CASES = {
    # N edges and tiny shapes: one thread of 256 works in wg_chol_lds (N = 1); T < N + 1; the last N below 32
    (1, 30, 4): 3, (2, 31, 5): 3, (3, 5, 6): 3, (31, 130, 34): 3,
    # Gram remainders: T mod 4 = 0..3 with (T + dPHI) mod 4 = 0..3 ...
    (5, 40, 8): 3, (5, 41, 8): 3, (5, 42, 8): 3, (5, 43, 8): 3,
    # ... (T + dPHI) mod 4 = 1..3 at T mod 4 = 0 ...
    (5, 40, 9): 3, (5, 40, 10): 3, (5, 40, 11): 3,
    # ... and TP = 64 with 31 padded months, which the eta loop must not read into the sums
    (9, 33, 12): 3,
    # eta staging rounds: N TP = 4096 (one full round) against 4608 and 4352 (a partial second round)
    (16, 256, 19): 3, (16, 257, 19): 3, (8, 512, 11): 3, (8, 513, 11): 3,
    (32, 97, 35): 3,  # one full round at N = 32
    # Z staging rounds: N (T + dPHI) = 4096 and 4112
    (16, 237, 19): 3, (16, 238, 19): 3,
    # plan boundaries at the natural prior dPHI = N + 3: TP = 448 | 480 | 480 | 512
    (32, 448, 35): 3, (32, 449, 35): 1, (32, 480, 35): 1, (32, 481, 35): 0,
    # exact byte boundaries: staged_z = 160 KiB to the byte, then eight bytes per row more
    (32, 97, 380): 3, (32, 97, 381): 1,
    (5, 4064, 8): 3, (5, 4064, 9): 1, (5, 4065, 8): 0,
    # the workload's own shape
    (20, 750, 23): 3,
}
# (N, T, dPHI, B): per-chain offsets of eta (N TP), Z (N (TP + dPHI)) and the outputs over 33 workgroups
MULTI = (12, 61, 15, 33)
MULTI_LD_CHAINS = (0, 32)

# the staging-round cases: (N, T, dPHI) -> ("eta" | "z", doubles staged, rounds)
ROUNDS = {
    (16, 256, 19): ("eta", 4096, 1), (16, 257, 19): ("eta", 4608, 2),
    (8, 512, 11): ("eta", 4096, 1), (8, 513, 11): ("eta", 4352, 2),
    (32, 97, 35): ("eta", 4096, 1),
    (16, 237, 19): ("z", 4096, 1), (16, 238, 19): ("z", 4112, 2),
}
# the cases whose normals k_phi_gen draws itself in test_philox_layout: the smallest with both remainders odd, and
# the eta-only plan at N = 32 (indices up to 32 * 484, 61 workgroups of k_phi_gen per chain)
PHILOX = [(5, 41, 9), (32, 449, 35)]


def round_up(x, m):
    return -(-x // m) * m


# ================================================================================================================
# restatement of phi_plan (csrc/ccmm_sweep.h); tests/test_launch_plans.py holds the library to it
def plan_bytes(N, T, dPHI):
    """(unstaged, eta staged, eta and Z staged) dynamic LDS bytes: Lpost | Rz | Sq | Ph [N x (N + 1)] each, then
    eta [N x (TP + 1)], the region widened to hold Z [N x (TP + dPHI)] after it."""
    TP = round_up(T, 32)
    base = 4 * N * (N + 1) * 8
    return base, base + N * (TP + 1) * 8, base + N * max(TP + 1, TP + dPHI) * 8


def plan(N, T, dPHI, mask=3):
    """(LDS bytes, stage bits) of launch_phi with option phi_stage = mask: bit 1 eta, bit 2 Z behind eta (a mask
    without bit 1 stages nothing)."""
    base, staged, staged_z = plan_bytes(N, T, dPHI)
    if not mask & 1:
        mask = 0
    if staged_z <= LDS_CU and mask & 2:
        return staged_z, 3
    if staged <= LDS_CU and mask & 1:
        return staged, 1
    return base, 0


def rounds(N, T, dPHI):
    """(eta, Z) staging rounds of the default plan (0: not staged)."""
    bits = plan(N, T, dPHI)[1]
    return (-(-N * round_up(T, 32) // ROUND) if bits & 1 else 0, -(-N * (T + dPHI) // ROUND) if bits & 2 else 0)


for _c, _p in CASES.items():
    assert plan(*_c)[1] == _p, (_c, plan(*_c))
    assert _c[1] + _c[2] >= 2 * _c[0], _c
assert plan(*MULTI[:3])[1] == 3
assert plan(5, 4064, 8)[0] == LDS_CU == plan(32, 97, 380)[0]
assert plan(20, 750, 23) == ((4 * 20 * 21 + 20 * (768 + 23)) * 8, 3) and plan(20, 750, 23)[0] == 140_000


# ================================================================================================================
@functools.lru_cache(maxsize=None)
def _sphi(N):
    su = toy_setup(O, N=N, p=1, Tobs=62, seed=6)
    assert su.sPHI.shape == (N, N)
    return su.sPHI


@functools.lru_cache(maxsize=None)
def phi_inputs(N, T, dPHI, B=2):
    """sPHI of the toy prior, B chains' shocks (T x N x B, a scale of their own each) and normals
    (N x (T + dPHI) x B).  Read-only."""
    rng = np.random.default_rng([N, T, dPHI, B, 11])
    eta = np.stack([(0.1 + 0.05 * (c % 7) + 0.001 * c) * rng.standard_normal((T, N)) for c in range(B)], -1)
    Z = np.stack([rng.standard_normal((N, T + dPHI)) for _ in range(B)], -1)
    sPHI = _sphi(N)
    for a in (eta, Z, sPHI):
        a.setflags(write=False)
    return sPHI, eta, Z


@functools.lru_cache(maxsize=None)
def phi_reference(N, T, dPHI):
    """Per chain of the two-chain inputs: ((sqrtPHI, PHI) in longdouble, (sqrtPHI, PHI) of the fp64 oracle)."""
    sPHI, eta, Z = phi_inputs(N, T, dPHI)
    return [(refs.phi_iw_ld(eta[..., c], sPHI, Z[..., c]), O.phi_iw(eta[..., c], sPHI, Z[..., c])) for c in range(2)]


@functools.lru_cache(maxsize=None)
def multi_reference():
    """The B = 33 case: (the fp64 oracle's (sqrtPHI, PHI) per chain, {chain: longdouble (sqrtPHI, PHI)} for
    MULTI_LD_CHAINS)."""
    N, T, dPHI, B = MULTI
    sPHI, eta, Z = phi_inputs(N, T, dPHI, B)
    orc = [O.phi_iw(eta[..., c], sPHI, Z[..., c]) for c in range(B)]
    return orc, {c: refs.phi_iw_ld(eta[..., c], sPHI, Z[..., c]) for c in MULTI_LD_CHAINS}


def phi_err(got_sq, got_PHI, sq, PHI):
    """(PHI, sqrtPHI) errors relative to the largest entry of each: the metric of the PHI block."""
    return (float(np.max(np.abs(got_PHI - PHI)) / np.abs(PHI).max()),
            float(np.max(np.abs(got_sq - sq)) / np.abs(sq).max()))
