"""Plain extended-precision references of the Gibbs blocks (np.longdouble, 80-bit on x86-64).

Explicit-loop Cholesky factorisations and substitutions, no LAPACK in a factor or solve step,
and none of the structure the device kernels (or the fp64 oracle's samplers) exploit: the
coefficient block is the weighted-Gram algebra of CTA.m:57-98 / CTAsys.m:57-108 per equation,
the A block one dense regression per row (mcmcVAR.m:236-254), and the SV draw one dense
factorisation of the whole (T+1)N-square precision.  tests/test_refs.py pins the fp64 oracles to
these within 1e-11 on every shape of tests/test_gpu_shape_edges.py.  elb_gibbs_ld is the ELB
shadow-rate step cell by cell from the joint density of the window (tests/elb_cases.py), ps_draw_ld the joint
draw of all censored cells of the window from the same density (tests/ps_cases.py)."""
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


def chol_band_ld(P, bw):
    """chol_ld for a matrix whose entries with |i - j| > bw are exactly zero: the factor has the same
    band, so every dot product runs over the band only (the terms left out are products with exact
    zeros).  Still one dense factorisation row by row; no block structure is used."""
    n = P.shape[0]
    L = np.zeros((n, n), LD)
    for k in range(n):
        lo, hi = max(0, k - bw), min(n, k + bw + 1)
        d = P[k, k] - L[k, lo:k] @ L[k, lo:k]
        assert d > 0, f"pivot {k} not positive"
        L[k, k] = np.sqrt(d)
        if k + 1 < hi:
            L[k + 1:hi, k] = (P[k + 1:hi, k] - L[k + 1:hi, lo:k] @ L[k, lo:k]) / L[k, k]
    return L


def phi_iw_ld(eta, sPHI, Z):
    """The inverse-Wishart draw of mcmcVAR.m:268-274 in longdouble: Lpost = chol(sPHI + eta' eta, 'lower'),
    R = chol(Z Z') (upper), sqrtPHI_ = Lpost / R, PHI = sqrtPHI_ sqrtPHI_', sqrtPHI = chol(PHI, 'lower').
    eta: T x N, Z: N x (T + dPHI).  Row r of Lpost / R solves R' x = Lpost(r, :)' (forward substitution on
    the lower factor R' of Z Z').  Returns (sqrtPHI, PHI) rounded to float64."""
    e = np.asarray(eta).astype(LD)
    Zl = np.asarray(Z).astype(LD)
    Lpost = chol_ld(np.asarray(sPHI).astype(LD) + e.T @ e)
    Rt = chol_ld(Zl @ Zl.T)
    Sq = np.stack([fwd_ld(Rt, Lpost[r]) for r in range(Lpost.shape[0])])
    PHI = Sq @ Sq.T
    return chol_ld(PHI).astype(np.float64), PHI.astype(np.float64)


def sv_dense_ld(D, b, Q, z, order=None):
    """x = Pi' L^-T (L^-1 Pi b + Pi z) in longdouble, L the dense Cholesky factor of the whole
    (T+1)N-square block-tridiagonal precision (diagonal blocks D[t], off-diagonal blocks -Q)
    permuted into the block order Pi; z column t belongs to block t.  order = None: the order of
    ``sv_order`` (the partitioned sampler's declaration, N <= 32).  order = range(T + 1): time order, what
    oracle.sv_draw_sequential declares for N > 32; the permuted matrix then has half bandwidth 2N - 1 and
    the factorisation's dot products run over that band (chol_band_ld).  Returns x as (T+1) x N float64.
    Nothing here follows the block recursion of either sampler."""
    T1, N = b.shape
    n = T1 * N
    P = np.zeros((n, n), LD)
    Qd = np.asarray(Q).astype(LD)
    for t in range(T1):
        P[t * N:(t + 1) * N, t * N:(t + 1) * N] = np.asarray(D[t]).astype(LD)
        if t + 1 < T1:
            P[t * N:(t + 1) * N, (t + 1) * N:(t + 2) * N] = -Qd
            P[(t + 1) * N:(t + 2) * N, t * N:(t + 1) * N] = -Qd.T
    if order is None:
        from oracle.ccmm_oracle import sv_separators  # the declared separator positions only
        blocks = sv_order(T1 - 1, sv_separators(T1 - 1))
    else:
        blocks = list(order)
    perm = np.concatenate([np.arange(t * N, (t + 1) * N) for t in blocks])
    assert np.array_equal(np.sort(perm), np.arange(n))
    Pp = P[np.ix_(perm, perm)]
    if order is None:
        L = chol_ld(Pp)
    else:
        i, j = np.nonzero(Pp)
        L = chol_band_ld(Pp, int(np.max(np.abs(i - j))))
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


# ------------------------------------------------------------------ predictive density (tests/fcst_cases.py)
def _sv_nu_ld(invA, logSV0, sqrtPHI, svz, z):
    """The shock side of one kept draw: logSV = logSV0 + cumsum(sqrtPHI randn, 2), sv = exp(logSV / 2),
    nu = invA (sv .* z) (mcmcVAR.m:301-314; BlockHybrid.m:553-561, 612).  Returns sv, nu: N x H x Nd."""
    N = invA.shape[0]
    H, Nd = z.shape[1], z.shape[2]
    shocks = (np.asarray(sqrtPHI).astype(LD) @ np.asarray(svz).astype(LD)).reshape(N, H, Nd, order="F")
    logSV = np.asarray(logSV0).astype(LD)[:, None, None] + np.cumsum(shocks, axis=1)
    sv = np.exp(logSV * LD(0.5))
    w = sv * np.asarray(z).astype(LD)
    nu = np.einsum("ij,jhn->ihn", np.asarray(invA).astype(LD), w)
    return sv, nu


def fcst_paths_ld(PAI, invA, logSV0, sqrtPHI, Xjumpoff, ndxYields, elb, svz, z, rec_floor=None):
    """mcmcVAR.m:298-323, 354-379 for one kept draw in longdouble: the companion recursion on the explicit
    state x = [1, y(t), ..., y(t-p+1)] (x <- [1; PAI' x + nu; x(2:K-N)], the rows fcstA has at :108-110, 317),
    once without a floor (:320-323), once with the series of rec_floor (default ndxYields, :360-366; a
    shadow-rate model passes ndxOTHERYIELDS) set to ELBbound inside the state when below it, and once with
    zero shocks (:376-379).

    Returns fY, fYc (N x H x Nd) and yhat (N x H) rounded to fp64, sv1 (N x Nd, longdouble: fcstSVdraws(:,1))
    and the smallest |y - elb| over every floor comparison made."""
    P = np.asarray(PAI).astype(LD)
    K, N = P.shape
    H, Nd = z.shape[1], z.shape[2]
    fl = np.asarray(ndxYields if rec_floor is None else rec_floor, bool)
    x0 = np.asarray(Xjumpoff).astype(LD)
    sv, nu = _sv_nu_ld(invA, logSV0, sqrtPHI, svz, z)
    E = LD(elb)

    def step(x, shock):
        xn = np.empty(K, LD)
        xn[0] = x[0]
        xn[1:1 + N] = P.T @ x + shock
        xn[1 + N:] = x[1:K - N]
        return xn

    fY, fYc, yhat = np.empty((N, H, Nd)), np.empty((N, H, Nd)), np.empty((N, H))
    gap = np.inf
    for nn in range(Nd):
        x = x0.copy()
        for hh in range(H):
            x = step(x, nu[:, hh, nn])
            fY[:, hh, nn] = x[1:1 + N]
        x = x0.copy()
        for hh in range(H):
            x = step(x, nu[:, hh, nn])
            y = x[1:1 + N]  # a view: the floor goes into the state
            gap = min(gap, float(np.min(np.abs(y[fl] - E))))
            y[fl & (y < E)] = E
            fYc[:, hh, nn] = y
    x = x0.copy()
    zero = np.zeros(N, LD)
    for hh in range(H):
        x = step(x, zero)
        yhat[:, hh] = x[1:1 + N]
    return fY, fYc, yhat, sv[:, 0, :], gap


def gauss_logscore_ld(mu, S, y):
    """logscoreGaussian.m:15-20 for N(mu, S S') in longdouble through chol_ld of S S' (any full-row-rank S)."""
    S = np.asarray(S).astype(LD)
    L = chol_ld(S @ S.T)
    zz = fwd_ld(L, np.asarray(y).astype(LD) - np.asarray(mu).astype(LD))
    n = L.shape[0]
    return float(-(n * np.log(2 * LD(np.pi)) + 2 * np.sum(np.log(np.diag(L))) + zz @ zz) / 2)


def fcst_scores_ld(PAI, invA, sv1, Xjumpoff, yrealized, ndxYields):
    """The two uncensored one-step scores of mcmcVAR.m:326-332, 341-344 per draw: the full vector and the macro
    block, N(muY, sqrtOmegaY sqrtOmegaY') with muY = PAI' Xjumpoff and sqrtOmegaY = invA diag(sv1(:, nn)).
    Returns 2 x Nd."""
    mu = np.asarray(PAI).astype(LD).T @ np.asarray(Xjumpoff).astype(LD)
    x = ~np.asarray(ndxYields, bool)
    out = np.empty((2, sv1.shape[1]))
    for nn in range(sv1.shape[1]):
        S = np.asarray(invA).astype(LD) * sv1[:, nn][None, :]
        out[0, nn] = gauss_logscore_ld(mu, S, yrealized)
        out[1, nn] = gauss_logscore_ld(mu[x], S[x, :], np.asarray(yrealized)[x])
    return out


def _shadow_core_ld(Pshadow, Pactual, src, x0, nu, elb, yl):
    """The simulation core of the shadow-rate models for given reduced-form shocks nu (N x H x Nd, longdouble),
    on the explicit state x = [1, y(t) .. y(t-p+1)] and the actual-rate state a = [a(t) .. a(t-p+1)] (blocks of
    len(src) rates; none for the linear model): y <- Pshadow' x + Pactual' a + nu, the shadow state shifted,
    a <- [max(y(src), ELB); a(1:end-block)].  Returns the unfloored paths (N x H x Nd, longdouble) and the
    smallest |y(yl) - ELB| over every path and horizon (inf when yl selects nothing)."""
    K, N = Pshadow.shape
    H, Nd = nu.shape[1], nu.shape[2]
    E = LD(elb)
    nb = len(src)
    fY = np.empty((N, H, Nd), LD)
    gap = np.inf
    for nn in range(Nd):
        x, a = x0[:K].copy(), x0[K:].copy()
        for hh in range(H):
            y = Pshadow.T @ x + Pactual.T @ a + nu[:, hh, nn]
            fY[:, hh, nn] = y
            x = np.concatenate([x[:1], y, x[1:K - N]])
            a = np.concatenate([np.maximum(y[src], E), a[:len(a) - nb]])
            if yl.any():
                gap = min(gap, float(np.min(np.abs(y[yl] - E))))
    return fY, gap


def _shadow_sim_ld(Pshadow, Pactual, src, invA, logSV0, sqrtPHI, Xjumpoff, ndxYields, elb, svz, z):
    """The simulation shared by the two shadow-rate models (_shadow_core_ld) on the shocks of one kept draw
    (_sv_nu_ld).  Returns fY, fY with the yields floored afterwards, sv1 and the smallest |y - ELB| over every
    comparison with the bound."""
    yl = np.asarray(ndxYields, bool)
    x0 = np.asarray(Xjumpoff).astype(LD)
    sv, nu = _sv_nu_ld(invA, logSV0, sqrtPHI, svz, z)
    fYl, gap = _shadow_core_ld(Pshadow, Pactual, src, x0, nu, elb, yl)
    fY = fYl.astype(np.float64)
    fYc = fY.copy()
    fYc[yl] = np.maximum(fYc[yl], float(elb))
    return fY, fYc, sv[:, 0, :], gap


def _bh_split_ld(P, yl, act):
    """PAIshadow / PAIactual of the block-hybrid model (mcmcVARshadowrateBlockHybrid.m:566-574;
    generateGIRF2blockhybrid.m:226-234): the equations of ``act`` read the yields' lags from the actual-rate
    states, every other coefficient multiplies the shadow state."""
    K, N = P.shape
    p = (K - 1) // N
    lag_rows = 1 + np.flatnonzero(np.tile(yl, p))  # ndxYIELDLAGS
    Pact = P[lag_rows, :].copy()
    Pact[:, ~act] = 0
    Psh = P.copy()
    Psh[np.ix_(lag_rows, np.flatnonzero(act))] = 0
    return Psh, Pact


def fcst_paths_bh_ld(PAI, invA, logSV0, sqrtPHI, Xjumpoff, ndxYields, actualrateBlock, elb, svz, z):
    """mcmcVARshadowrateBlockHybrid.m:566-574, 611-625 for one kept draw in longdouble (arguments as
    oracle.ccmm_oracle_fcst.fcst_draw_bh; Xjumpoff has K + Nyields p entries): the equations of
    actualrateBlock read the yields' lags from the actual-rate states (PAIactual; PAIshadow is zero there), every
    other coefficient multiplies the shadow state; the actual-rate state of a yield is max(shadow, ELB) (:623).
    The yields of the returned censored paths are floored afterwards (:696-700)."""
    P = np.asarray(PAI).astype(LD)
    yl, act = np.asarray(ndxYields, bool), np.asarray(actualrateBlock, bool)
    Psh, Pact = _bh_split_ld(P, yl, act)
    return _shadow_sim_ld(Psh, Pact, np.flatnonzero(yl), invA, logSV0, sqrtPHI, Xjumpoff, yl, elb, svz, z)


def fcst_paths_hybrid_ld(PAI, invA, logSV0, sqrtPHI, Xjumpoff, ndxYields, ndxSHADOWRATE, elb, svz, z):
    """mcmcVARhybridGibbs.m:585, 621-635 for one kept draw in longdouble (arguments as
    oracle.ccmm_oracle_fcst.fcst_draw_hybrid): PAI has Kshadow + Ns p rows, the last Ns p multiply the lags of
    the actual rates max(shadow, ELB) of the Ns shadow-rate variables."""
    P = np.asarray(PAI).astype(LD)
    s = np.asarray(ndxSHADOWRATE, int)
    N = P.shape[1]
    p = (P.shape[0] - 1) // (N + s.size)
    K = 1 + N * p
    return _shadow_sim_ld(P[:K], P[K:], s, invA, logSV0, sqrtPHI, Xjumpoff, ndxYields, elb, svz, z)


def fcst_mu_shadow_ld(PAI, Xjumpoff, ndxYields, actualrateBlock=None, ndxSHADOWRATE=None):
    """muY = fcstA(ndxfcstY, :) Xjumpoff of the block-hybrid (:566-584) or hybrid (:585, 591-595) model."""
    P = np.asarray(PAI).astype(LD)
    x = np.asarray(Xjumpoff).astype(LD)
    if ndxSHADOWRATE is not None:
        return P.T @ x
    K, N = P.shape
    p = (K - 1) // N
    yl, act = np.asarray(ndxYields, bool), np.asarray(actualrateBlock, bool)
    lag_rows = 1 + np.flatnonzero(np.tile(yl, p))
    Pact = P[lag_rows, :].copy()
    Pact[:, ~act] = 0
    Psh = P.copy()
    Psh[np.ix_(lag_rows, np.flatnonzero(act))] = 0
    return Psh.T @ x[:K] + Pact.T @ x[K:]


# ------------------------------------------------------------------ generalized impulse responses (tests/girf_cases.py)
def girf_ld(PAI, invA, sqrtPHI, SV0, Xjumpoff, z, svz, shock11, cumcode, np_, model="linear", actual=None,
            yields=None, shadow=None, elb=0.25):
    """generateGIRF2linear.m / generateGIRF2blockhybrid.m:199-259 / generateGIRF2hybrid.m:191-251 for one kept
    draw in longdouble, on the explicit state of _shadow_core_ld (no companion matrix).  z, svz: N x H x nsim.
    antitheticSim: SV = exp(cumsum(sqrtPHI svz, 2) / 2) and the four shock sets z SV SV0, -z SV SV0, z / SV SV0,
    -z / SV SV0, each with the scenario's shock (0, +shock11, -shock11) added to element (1, 1) before invA.
    model "bh": PAIshadow / PAIactual of ``actual`` and ``yields`` (the ring holds the yields); "hybrid": PAI has
    K + Ns p rows, the last Ns p multiply the lags of the actual rates of ``shadow``.  The ring takes max(y, ELB);
    the yields are floored in the output only.  Mean over the 4 nsim paths, then cumsum / np_ for ``cumcode``.

    Returns the three mean paths (3 x N x H, longdouble), the share of yield values (all paths, horizons and
    scenarios) below the ELB (nan for the linear model) and the smallest |y - ELB| over all of them."""
    P = np.asarray(PAI).astype(LD)
    N, H, nsim = z.shape
    if model == "hybrid":
        src = np.flatnonzero(np.asarray(shadow, bool))
        p = (P.shape[0] - 1) // (N + src.size)
        K = 1 + N * p
        Psh, Pact = P[:K], P[K:]
        yl = np.asarray(yields, bool)
    elif model == "bh":
        yl = np.asarray(yields, bool)
        Psh, Pact = _bh_split_ld(P, yl, np.asarray(actual, bool))
        src = np.flatnonzero(yl)
    else:
        assert model == "linear"
        Psh, Pact, src, yl = P, np.zeros((0, N), LD), np.zeros(0, int), np.zeros(N, bool)
    x0 = np.asarray(Xjumpoff).astype(LD)
    assert x0.size == Psh.shape[0] + Pact.shape[0]
    zl = np.asarray(z).astype(LD)
    SV = np.exp(np.cumsum(np.einsum("ij,jhn->ihn", np.asarray(sqrtPHI).astype(LD), np.asarray(svz).astype(LD)),
                          axis=1) / 2)
    s0 = np.asarray(SV0).astype(LD)[:, None, None]
    iA = np.asarray(invA).astype(LD)
    cc = np.zeros(N, bool) if cumcode is None else np.asarray(cumcode, bool)
    E = LD(elb)
    out = np.empty((3, N, H), LD)
    below = total = 0
    gap = np.inf
    for sc, s11 in enumerate((LD(0), LD(shock11), -LD(shock11))):
        sets = []
        for sign, up in ((1, True), (-1, True), (1, False), (-1, False)):
            eps = sign * zl * (SV if up else 1 / SV) * s0
            eps[0, 0, :] += s11
            sets.append(np.einsum("ij,jhn->ihn", iA, eps))
        fY, g = _shadow_core_ld(Psh, Pact, src, x0, np.concatenate(sets, axis=2), elb, yl)
        gap = min(gap, g)
        below += int(np.sum(fY[yl] < E))
        total += fY[yl].size
        fY[yl] = np.maximum(fY[yl], E)
        m = np.sum(fY, axis=2) / (4 * nsim)
        m[cc] = np.cumsum(m[cc], axis=1) / LD(np_)
        out[sc] = m
    return out, (below / total if total else float("nan")), gap


# ------------------------------------------------------------------ precision sampler of the censored cells (tests/ps_cases.py)
def bwd_cols_ld(L, Y):
    """bwd_ld on every column of Y (n x K) at once."""
    n = Y.shape[0]
    X = np.zeros(Y.shape, LD)
    for k in range(n - 1, -1, -1):
        X[k] = (Y[k] - L[k + 1:, k] @ X[k + 1:]) / L[k, k]
    return X


def ps_draw_ld(pai3, invbbb, Y, yNaN, Y0, pai0, z):
    """The joint Gaussian draw of the censored cells of the window (arguments of oracle.ccmm_oracle_bh.ps_inputs /
    precision_sampler_nan; z: n x K, one column per draw) in longdouble, read off the joint density of the
    window as elb_gibbs_ld reads its single-cell conditionals: with the structural residuals
    eps_t = invbbb_t (y_t - pai0_t - sum_l pai3_l y_{t-l}), t = 0..T-1 (y before month 0 from Y0), the density is
    exp(-1/2 sum_t |eps_t|^2).  Cell i = (a, t) enters eps_t .. eps_{min(t+p, T-1)} linearly: column i of G holds
    its slopes invbbb_t(:, a) and -invbbb_{t+k} pai3_k(:, a), so eps = e0 + G x with e0 the residuals at censored
    cells = 0, the precision is P = G' G and the linear term b = -G' e0.  Then one dense lower Cholesky factor
    (chol_ld) of P in month-major cell order (variables in index order within a month), ybar = L^-1 b and
    x_k = L'^-1 (ybar + z_k).  No stacked system matrix, no band, no LAPACK.

    Returns (mean P^-1 b, ybar, L, draws n x K) in longdouble and the cells as (variable, month) pairs."""
    B = np.asarray(invbbb).astype(LD)
    N, T = np.asarray(Y).shape
    p = np.asarray(pai3).shape[2]
    Phi = [np.asarray(pai3)[:, :, l].astype(LD) for l in range(p)]
    m = np.asarray(yNaN, bool)
    Yx = np.hstack([np.asarray(Y0).astype(LD)[:, ::-1], np.where(m, LD(0), np.asarray(Y).astype(LD))])  # column p + t: month t
    c0 = np.asarray(pai0).astype(LD)
    e0 = np.zeros((T, N), LD)
    for t in range(T):
        r = Yx[:, p + t] - c0[:, t]
        for l in range(1, p + 1):
            r = r - Phi[l - 1] @ Yx[:, p + t - l]
        e0[t] = B[:, :, t] @ r
    cells = [(a, t) for t in range(T) for a in np.nonzero(m[:, t])[0]]
    n = len(cells)
    G = np.zeros((T, N, n), LD)
    for i, (a, t) in enumerate(cells):
        G[t, :, i] = B[:, a, t]
        for k in range(1, min(p, T - 1 - t) + 1):
            G[t + k, :, i] = -(B[:, :, t + k] @ Phi[k - 1][:, a])
    G = G.reshape(T * N, n)
    L = chol_ld(G.T @ G)
    ybar = fwd_ld(L, -(G.T @ e0.reshape(-1)))
    zl = np.asarray(z).astype(LD).reshape(n, -1)
    return bwd_ld(L, ybar), ybar, L, bwd_cols_ld(L, ybar[:, None] + zl), cells
