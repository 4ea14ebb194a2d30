"""Toy data of tests/test_gpu_stationarity.py: N = 2, p = 1, 41 observations (T = 40).  The random-walk slots
hold two independent random walks under a Minnesota prior centred on the unit root, so the posterior of the
companion's spectral radius straddles 1; the stable slots hold two AR(1) series with phi = 0.3 under a prior
centred on 0."""
import numpy as np

N, P, TOBS = 2, 1, 41


def random_walk(seed):
    rng = np.random.default_rng([seed, 1])
    return np.cumsum(rng.standard_normal((TOBS, N)), axis=0)


def stable_ar1(seed, phi=0.3):
    rng = np.random.default_rng([seed, 2])
    y = np.zeros((TOBS, N))
    for t in range(1, TOBS):
        y[t] = phi * y[t - 1] + rng.standard_normal(N)
    return y


def rho(PAI):
    """Spectral radius of the p = 1 companion: PAI is K x N with K = 1 + N."""
    return float(np.max(np.abs(np.linalg.eigvals(PAI[1:1 + N].T))))
