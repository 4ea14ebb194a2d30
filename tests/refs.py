"""Plain extended-precision references of the Gibbs blocks (np.longdouble, 80-bit on x86-64).

Explicit-loop Cholesky factorisations and substitutions, no LAPACK in a factor or solve step,
and none of the structure the device kernels (or the fp64 oracle's samplers) exploit: the
coefficient block is the weighted-Gram algebra of CTA.m:57-98 / CTAsys.m:57-108 per equation,
the A block one dense regression per row (mcmcVAR.m:236-254), and the SV draw one dense
factorisation of the whole (T+1)N-square precision.  tests/test_refs.py pins the fp64 oracles to
these within 1e-11 on every shape of tests/test_gpu_shape_edges.py.  elb_gibbs_ld is the ELB
shadow-rate step cell by cell from the joint density of the window (tests/elb_cases.py)."""
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


def inv_ld(M):
    """Inverse of a small dense longdouble matrix (Gauss-Jordan, partial pivoting)."""
    n = M.shape[0]
    W = np.hstack([np.asarray(M).astype(LD), np.eye(n, dtype=LD)])
    for col in range(n):
        piv = col + int(np.argmax(np.abs(W[col:, col])))
        assert W[piv, col] != 0, "singular"
        if piv != col:
            W[[col, piv]] = W[[piv, col]]
        W[col] /= W[col, col]
        f = W[:, col].copy()
        f[col] = 0
        W -= f[:, None] * W[col][None, :]
    return W[:, n:]


def elb_gibbs_ld(Y, STATE0, YHAT0, ndxS, sNaN, p, C, Psi, SVol, elb, burnin, u):
    """One chain of gibbsdrawShadowrates.m (burnin passes + 1 draw, uniforms u Ns x T x (burnin + 1)),
    every censored cell drawn from its full conditional read off the joint Gaussian density of the
    window in longdouble: with ytilde = Y - Y0 (Y0 the deterministic path of :157-165, started at STATE0)
    and the structural residuals eps_t = diag(SVol_t)^-1 Psi(2:Ny+1,:)^-1 (ytilde_t - sum_l Phi_l ytilde_{t-l}),
    t = 0..T-1 (ytilde = 0 before month 0), the density is exp(-1/2 sum_t |eps_t|^2).  Cell x = ytilde(a, t)
    enters eps_t .. eps_{min(t+p, T-1)} linearly with slopes g_k; so its conditional precision is
    sum_k |g_k|^2 and its mean x - (sum_k g_k . eps_{t+k}) / precision.  No smoothing weights, no QR, no
    month-level Ns x Ns conditioning: neither the oracle's form nor the device's.  Passes, months and
    series run in the order of :206-218.  The scalar draw is oracle.draw_trunc_normal on the mean and sd
    rounded to fp64 (tests/test_gpu_truncnorm_grid.py pins that transform on its own).

    Returns (S, flags, ub, PHIbar, sig): S Ns x T fp64 (the last pass), the others Ns x T x passes
    (flags uint8; ub, PHIbar, sig fp64, NaN where no draw was made)."""
    from oracle.ccmm_oracle import draw_trunc_normal, erfc
    Yl = np.asarray(Y).astype(LD).copy()
    Ny, T = Yl.shape
    Cl = np.asarray(C).astype(LD)
    ndx = np.nonzero(np.asarray(ndxS, bool))[0]
    sNaN = np.asarray(sNaN, bool)
    Ns, passes = len(ndx), burnin + 1
    Y0 = np.zeros((Ny, T), LD)
    st = np.asarray(STATE0).astype(LD)
    for t in range(T):
        Y0[:, t] = st[1:1 + Ny]
        if YHAT0 is not None:
            Y0[:, t] += np.asarray(YHAT0[:, t]).astype(LD)
        st = Cl @ st
    Phi = Cl[1:1 + Ny, 1:1 + Ny * p]                       # [Phi_1 ... Phi_p]
    Yt = np.hstack([np.zeros((Ny, p), LD), Yl - Y0])       # column p + t is month t
    Pinv = inv_ld(np.asarray(Psi)[1:1 + Ny, :])
    Wm = [Pinv / np.asarray(SVol[:, t]).astype(LD)[:, None] for t in range(T)]
    months = [t for t in range(T) if sNaN[:, t].any()]
    slopes = {}
    for t in months:
        kmax = min(p, T - 1 - t)
        for a in np.nonzero(sNaN[:, t])[0]:
            g = [Wm[t][:, ndx[a]]] + [-(Wm[t + k] @ Phi[:, (k - 1) * Ny + ndx[a]]) for k in range(1, kmax + 1)]
            g = np.stack(g)
            slopes[a, t] = (g, np.sum(g * g))
    flags = np.zeros((Ns, T, passes), np.uint8)
    ub, PHIbar, sig = (np.full((Ns, T, passes), np.nan) for _ in range(3))
    for n in range(passes):
        for t in months:
            kmax = min(p, T - 1 - t)
            eps = np.stack([Wm[tau] @ (Yt[:, p + tau] - Phi @ Yt[:, [p + tau - l for l in range(1, p + 1)]].T.reshape(-1))
                            for tau in range(t, t + kmax + 1)])
            for a in np.nonzero(sNaN[:, t])[0]:
                g, prec = slopes[a, t]
                x = Yt[ndx[a], p + t]
                mu = float(x - np.sum(g * eps) / prec + Y0[ndx[a], t])
                sd = float(1 / np.sqrt(prec))
                draw, fl = draw_trunc_normal(mu, sd, elb, u[a, t, n])
                xn = LD(draw) - Y0[ndx[a], t]
                eps += g * (xn - x)
                Yt[ndx[a], p + t] = xn
                Yl[ndx[a], t] = draw
                flags[a, t, n], sig[a, t, n] = fl, sd
                if sd > 1e-10:
                    ub[a, t, n] = (elb - mu) / sd
                    PHIbar[a, t, n] = 0.5 * erfc(-np.sqrt(0.5) * ub[a, t, n])
    return Yl[ndx, :].astype(np.float64), flags, ub, PHIbar, sig
