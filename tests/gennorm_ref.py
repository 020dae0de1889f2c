"""A numpy float64 restatement of the device fit of include/epilogos_gennorm.h (no GPU): the objective, the start, Nelder-Mead as
scipy.optimize.fmin runs it with its defaults, and the median pick -- and the fixed-seed sample families that
tests/test_gennorm_host.py and the GPU tests fit.  scipy is the reference of those tests; this file shows that the ALGORITHM the
header describes satisfies their condition, before any device arithmetic comes into it."""
import numpy as np
from scipy.special import gammaln

MAXFUN = 600
FTOL = 1e-4                      # fmin's absolute xtol and ftol, and the margin of the tests' fit-quality condition


def objective(p, x):
    """n (log scale - log(beta / 2) + lgamma(1 / beta)) + sum |(x - loc) / scale| ** beta; +inf outside the parameter space."""
    beta, loc, scale = float(p[0]), float(p[1]), float(p[2])
    if not (beta > 0.0) or not (scale > 0.0) or loc != loc:
        return np.inf
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        f = x.size * (np.log(scale) - np.log(0.5 * beta) + gammaln(1.0 / beta)) + np.sum(np.abs((x - loc) / scale) ** beta)
    return float(f) if f == f else np.inf


def start(x):
    """(1, mean, sqrt(var / 2)) in float64, or None for a degenerate sample (variance 0 or a value that is not finite)."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        mean = x.sum() / x.size
        var = ((x - mean) ** 2).sum() / x.size
    if not (var > 0.0) or not np.isfinite(mean) or not np.isfinite(var):
        return None
    return np.array([1.0, mean, np.sqrt(var * 0.5)])


class _Cap(Exception):
    pass


def fit(x):
    """-> (params (beta, loc, scale), fval, evaluations, flag): flag 0 converged, 1 stopped at the cap, 2 degenerate (params NaN)."""
    x0 = start(x)
    if x0 is None:
        return np.full(3, np.nan), np.nan, 0, 2
    x = np.asarray(x, dtype=np.float64)
    evals = [0]

    def f(p):
        if evals[0] >= MAXFUN:
            raise _Cap()
        evals[0] += 1
        return objective(p, x)
    sim = np.tile(x0, (4, 1))
    for k in range(3):
        sim[k + 1, k] = 1.05 * x0[k] if x0[k] != 0 else 0.00025
    fsim = np.array([f(p) for p in sim])
    order = np.argsort(fsim, kind="stable")
    sim, fsim = sim[order], fsim[order]
    iterations, converged = 1, False
    while evals[0] < MAXFUN and iterations < MAXFUN:
        with np.errstate(invalid="ignore"):
            if np.max(np.abs(sim[1:] - sim[0])) <= FTOL and np.max(np.abs(fsim[0] - fsim[1:])) <= FTOL:
                converged = True
                break
        try:
            xbar = ((sim[0] + sim[1]) + sim[2]) / 3.0
            xr = 2.0 * xbar - sim[3]
            fxr = f(xr)
            shrink = False
            if fxr < fsim[0]:
                xe = 3.0 * xbar - 2.0 * sim[3]
                fxe = f(xe)
                sim[3], fsim[3] = (xe, fxe) if fxe < fxr else (xr, fxr)
            elif fxr < fsim[2]:
                sim[3], fsim[3] = xr, fxr
            elif fxr < fsim[3]:
                xc = 1.5 * xbar - 0.5 * sim[3]
                fxc = f(xc)
                if fxc <= fxr:
                    sim[3], fsim[3] = xc, fxc
                else:
                    shrink = True
            else:
                xcc = 0.5 * xbar + 0.5 * sim[3]
                fxcc = f(xcc)
                if fxcc < fsim[3]:
                    sim[3], fsim[3] = xcc, fxcc
                else:
                    shrink = True
            if shrink:
                for j in (1, 2, 3):
                    sim[j] = sim[0] + 0.5 * (sim[j] - sim[0])
                    fsim[j] = f(sim[j])
            iterations += 1
        except _Cap:
            pass
        order = np.argsort(fsim, kind="stable")
        sim, fsim = sim[order], fsim[order]
    return sim[0].copy(), float(fsim[0]), evals[0], 0 if converged else 1


def median_pick(nnlf):
    """The trial with the median negative log-likelihood: the lower median of a stable ascending sort."""
    return int(np.argsort(np.asarray(nnlf, dtype=np.float64), kind="stable")[(len(nnlf) - 1) // 2])


def nnlf_bound(params, x):
    """The tests' bound on |device - scipy| of a negative log-likelihood over x:
    1e-13 * (sum |z| ** beta + M * (|log scale| + |log(beta / 2)| + |lgamma(1 / beta)|))."""
    beta, loc, scale = (float(v) for v in params)
    x = np.asarray(x, dtype=np.float64)
    return 1e-13 * (np.sum(np.abs((x - loc) / scale) ** beta) + x.size * (abs(np.log(scale)) + abs(np.log(0.5 * beta)) + abs(gammaln(1.0 / beta))))


# ---- the samples ---------------------------------------------------------------------------------------------------------------
FAMILIES = ("gennorm06", "gennorm2", "signedsq", "rounded")
# the seed of a (family, n) that needs another one than 0 for the restatement ALONE to satisfy the fit-quality condition against
# scipy's fit (tests/test_gennorm_host.py asserts that it does; with scipy 1.15.3 seed 0 serves every family and size)
SEEDS = {}


def sample(family, n, seed=None):
    """float32 [n] of one of the four families, from a fixed seed."""
    import scipy.stats as st
    rng = np.random.default_rng([FAMILIES.index(family), n, SEEDS.get((family, n), 0) if seed is None else seed])
    if family == "gennorm06":
        v = st.gennorm.rvs(0.6, size=n, random_state=rng)
    elif family == "gennorm2":
        v = st.gennorm.rvs(2.0, loc=-1.0, size=n, random_state=rng)
    elif family == "signedsq":                       # signed squares of normals: beta about 0.34, the shape of real null distances
        z = rng.normal(size=n)
        v = np.sign(z) * z * z
    elif family == "rounded":                        # ties, and data points at loc
        v = np.round(rng.normal(scale=0.2, size=n), 2)
    else:
        raise KeyError(family)
    return v.astype(np.float32)


def sub_samples(M, T, n, seed=0):
    """int32 [T, n]: T sub-samples of n of M indices without replacement, from a fixed seed (the GPU tests' idx)."""
    rng = np.random.default_rng([M, T, n, seed])
    return np.stack([rng.choice(M, size=n, replace=False) for _ in range(T)]).astype(np.int32)
