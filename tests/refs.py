"""Plain extended-precision references of the Gibbs blocks (np.longdouble, 80-bit on x86-64).

Explicit-loop Cholesky factorisations and substitutions, no LAPACK in a factor or solve step,
and none of the structure the device kernels (or the fp64 oracle's samplers) exploit: the
coefficient block is the weighted-Gram algebra of CTA.m:57-98 / CTAsys.m:57-108 per equation,
the A block one dense regression per row (mcmcVAR.m:236-254), and the SV draw one dense
factorisation of the whole (T+1)N-square precision.  tests/test_refs.py pins the fp64 oracles to
these within 1e-11 on every shape of tests/test_gpu_shape_edges.py."""
import numpy as np

LD = np.longdouble


def chol_ld(P):
    """Lower Cholesky factor of a symmetric positive definite longdouble matrix (row by row)."""
    n = P.shape[0]
    L = np.zeros((n, n), LD)
    for k in range(n):
        d = P[k, k] - L[k, :k] @ L[k, :k]
        assert d > 0, f"pivot {k} not positive"
        L[k, k] = np.sqrt(d)
        if k + 1 < n:
            L[k + 1:, k] = (P[k + 1:, k] - L[k + 1:, :k] @ L[k, :k]) / L[k, k]
    return L


def fwd_ld(L, r):
    """y = L \\ r (forward substitution)."""
    n = r.shape[0]
    y = np.zeros(n, LD)
    for k in range(n):
        y[k] = (r[k] - L[k, :k] @ y[:k]) / L[k, k]
    return y


def bwd_ld(L, y):
    """x = L' \\ y (backward substitution on the transpose of the lower factor)."""
    n = y.shape[0]
    x = np.zeros(n, LD)
    for k in range(n - 1, -1, -1):
        x[k] = (y[k] - L[k + 1:, k] @ x[k + 1:]) / L[k, k]
    return x


def cta_ld(Y, X, A, sqrtht, iVdiag, iVb, PAI, z):
    """CTA.m:57-98 (X: T x K) / CTAsys.m:57-108 (X: T x K x N, one design per equation) in
    longdouble: per equation j, with the columns < j already redrawn, the weighted Gram
    X_j' diag(w) X_j + diag(iV_j), the right-hand side iVb_j + X_j' v, a Cholesky factor and
    x = L' \\ (L \\ rhs + z_j).  Returns PAI (K x N) rounded to float64."""
    Y = np.asarray(Y).astype(LD)
    X = np.asarray(X).astype(LD)
    A = np.asarray(A).astype(LD)
    ih2 = 1 / np.asarray(sqrtht).astype(LD) ** 2
    iVdiag, iVb, z = (np.asarray(a).astype(LD) for a in (iVdiag, iVb, z))
    PAI = np.asarray(PAI).astype(LD).copy()
    K, N = PAI.shape
    Xs = [X[:, :, j] for j in range(N)] if X.ndim == 3 else [X] * N
    XPAI = np.column_stack([Xs[jj] @ PAI[:, jj] for jj in range(N)])
    for j in range(N):
        E = Y - XPAI
        E[:, j] = Y[:, j]
        w = ih2[:, j:] @ (A[j:, j] ** 2)
        v = ((E @ A[j:, :].T) * ih2[:, j:]) @ A[j:, j]
        Xj = Xs[j]
        P = Xj.T @ (Xj * w[:, None])
        P[np.diag_indices(K)] += iVdiag[:, j]
        L = chol_ld(P)
        PAI[:, j] = bwd_ld(L, fwd_ld(L, iVb[:, j] + Xj.T @ v) + z[:, j])
        XPAI[:, j] = Xj @ PAI[:, j]
    return PAI.astype(np.float64)


def astep_ld(RESID, sqrtht, z):
    """The A block (mcmcVAR.m:236-254, flat prior) in longdouble: row ii regresses
    RESID(:, ii) / sqrtht(:, ii) on RESID(:, :ii) / sqrtht(:, ii); alpha = L' \\ (L \\ Zz + z_ii)
    with L L' = ZZ; A(ii, :ii) = -alpha.  invA by forward substitution.  Returns (A, invA)."""
    R = np.asarray(RESID).astype(LD)
    sh = np.asarray(sqrtht).astype(LD)
    z = np.asarray(z).astype(LD)
    N = R.shape[1]
    A = np.eye(N, dtype=LD)
    off = 0
    for ii in range(1, N):
        y = R[:, ii] / sh[:, ii]
        Xa = R[:, :ii] / sh[:, ii:ii + 1]
        L = chol_ld(Xa.T @ Xa)
        A[ii, :ii] = -bwd_ld(L, fwd_ld(L, Xa.T @ y) + z[off:off + ii])
        off += ii
    invA = np.zeros((N, N), LD)
    for c in range(N):
        e = np.zeros(N, LD)
        e[c] = 1
        invA[:, c] = fwd_ld(A, e)
    return A.astype(np.float64), invA.astype(np.float64)


def sv_order(T, seps):
    """Block order of the declared SV factorisation: the interiors of the segments between
    the separators, each in time order, then the separators."""
    bounds = [-1] + list(seps) + [T + 1]
    order = [t for k in range(1, len(bounds)) for t in range(bounds[k - 1] + 1, bounds[k])]
    return order + list(seps)


def sv_dense_ld(D, b, Q, z):
    """x = Pi' L^-T (L^-1 Pi b + Pi z) in longdouble, L the dense Cholesky factor of the whole
    (T+1)N-square block-tridiagonal precision (diagonal blocks D[t], off-diagonal blocks -Q)
    permuted into the order Pi of ``sv_order``; z column t belongs to block t.  Returns x as
    (T+1) x N float64.  Nothing here follows the block recursion of the partitioned sampler."""
    T1, N = b.shape
    n = T1 * N
    P = np.zeros((n, n), LD)
    Qd = np.asarray(Q).astype(LD)
    for t in range(T1):
        P[t * N:(t + 1) * N, t * N:(t + 1) * N] = np.asarray(D[t]).astype(LD)
        if t + 1 < T1:
            P[t * N:(t + 1) * N, (t + 1) * N:(t + 2) * N] = -Qd
            P[(t + 1) * N:(t + 2) * N, t * N:(t + 1) * N] = -Qd.T
    from oracle.ccmm_oracle import sv_separators  # the declared separator positions only
    perm = np.concatenate([np.arange(t * N, (t + 1) * N)
                           for t in sv_order(T1 - 1, sv_separators(T1 - 1))])
    assert np.array_equal(np.sort(perm), np.arange(n))
    L = chol_ld(P[np.ix_(perm, perm)])
    bp = np.asarray(b).astype(LD).reshape(-1)[perm]
    zp = np.asarray(z).astype(LD).T.reshape(-1)[perm]
    xp = bwd_ld(L, fwd_ld(L, bp) + zp)
    x = np.zeros(n, LD)
    x[perm] = xp
    return x.reshape(T1, N).astype(np.float64)
