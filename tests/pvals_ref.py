"""The p-value arithmetic of epilogos_amd/csrc/epg_pvals.hip restated in float64 numpy, operation for operation: the same split
between the series of the lower incomplete gamma function and the continued fraction of the upper one (at x = a + 1), the same
order of operations in the exponent, the same stopping rules and the same cap.  numpy's pow / log / exp and math.lgamma stand
where the kernel calls the device library's; nothing here is contracted into a fused multiply-add, and the kernel is compiled
with contraction off.  Also the test inputs of tests/test_hip_pvals.py, which tests/test_pvals_host.py runs through this
restatement and scipy.

What the restatement differs from roiAndVisualPairwise.calculatePVals (scipy 1.15's gennorm.cdf) by, measured by
tests/test_pvals_host.py over every (size, parameter set) of the GPU test, is RECORDED below; the GPU test's bounds are four
times these figures (the device's pow, log, exp and lgamma are a few ulp from the host's, and the magnitude of the exponent
amplifies that)."""
import math

import numpy as np

EPS = 2.220446049250313e-16
FPMIN = 2.2250738585072014e-308 / EPS
ITMAX = 2000                                                     # GAMMA_ITMAX of the kernel
MAXLOG = 7.09782712893383996843e2                               # scipy's (cephes') underflow cut: a prefactor below exp(-MAXLOG) is 0

# the restatement against calculatePVals, the worst over SIZES x PARAMS (test_pvals_host prints the figures it measures):
# measured 6.171e-14 (beta = 8, |z|**beta = 1.115: 1 - P where scipy sums Q itself) and 24 x 2^-52 = 5.329e-15 (beta = 2), rounded up
# to two digits; 0 of the 427 314 "%.5e" strings differ
REL_BELOW = 6.2e-14    # x <= loc: the smallest r with |p - scipy's| <= r * scipy's + ABS_FLOOR
ABS_ABOVE = 5.4e-15    # x >  loc: |p - scipy's|
FACTOR = 4                                                       # the device's bound is FACTOR times the figures above
ABS_FLOOR = 1e-300                                               # below loc, on top of the relative bound: the denormal p

SIZES = (1, 63, 64, 65, 1025, 70001)
PARAMS = ((0.3478, -6.1e-11, 5.05e-4), (0.6, -0.002, 0.003), (1.0, 0.001, 0.01), (2.0, 0.0, 0.02), (8.0, 0.0, 0.02), (0.05, 0.0, 1e-6))


def gammaincc(a, x):
    """Q(a, x) for a scalar a > 0 and an array x >= 0 (NaN allowed): -> (Q, capped) with capped[i] True where the iteration
    stopped at ITMAX.  x < a + 1: 1 - P by the series; else the continued fraction (modified Lentz)."""
    x = np.asarray(x, dtype=np.float64)
    q = np.full(x.shape, np.nan)
    capped = np.zeros(x.shape, dtype=bool)
    if a == 0.0:                                                 # beta = inf: scipy's answer, 0 for x > 0 and NaN at 0
        q[x > 0] = 0.0
        return q, capped
    gln = math.lgamma(a)
    q[x == 0] = 1.0
    q[x == np.inf] = 0.0
    with np.errstate(all="ignore"):
        ser = np.where((x > 0) & (x < a + 1.0))[0]
        if ser.size:
            xs = x[ser]
            ap = np.full(xs.shape, a)
            dl = np.full(xs.shape, 1.0 / a)
            sm = dl.copy()
            live = np.ones(xs.shape, dtype=bool)
            for _ in range(ITMAX):
                ap = np.where(live, ap + 1.0, ap)
                dl = np.where(live, dl * (xs / ap), dl)
                sm = np.where(live, sm + dl, sm)
                live &= ~(np.abs(dl) < np.abs(sm) * EPS)
                if not live.any():
                    break
            capped[ser] = live
            arg = -xs + a * np.log(xs) - gln
            q[ser] = 1.0 - sm * np.where(arg < -MAXLOG, 0.0, np.exp(arg))
        cf = np.where((x >= a + 1.0) & (x < np.inf))[0]
        if cf.size:
            xs = x[cf]
            b = xs + 1.0 - a
            c = np.full(xs.shape, 1.0 / FPMIN)
            d = 1.0 / b
            h = d.copy()
            live = np.ones(xs.shape, dtype=bool)
            for i in range(1, ITMAX + 1):
                an = -float(i) * (float(i) - a)
                b = b + 2.0
                d2 = an * d + b
                d2 = np.where(np.abs(d2) < FPMIN, FPMIN, d2)
                c2 = b + an / c
                c2 = np.where(np.abs(c2) < FPMIN, FPMIN, c2)
                d2 = 1.0 / d2
                dl = d2 * c2
                d, c, h = np.where(live, d2, d), np.where(live, c2, c), np.where(live, h * dl, h)
                live &= ~(np.abs(dl - 1.0) <= EPS)
                if not live.any():
                    break
            capped[cf] = live
            arg = -xs + a * np.log(xs) - gln
            q[cf] = np.where(arg < -MAXLOG, 0.0, np.exp(arg)) * h
    return q, capped


def pvals(x, beta, loc, scale):
    """The kernel's p-values of the float32 array x: -> (p float64, flags int32 [2] = (NaN p-values, values stopped at the cap))."""
    xd = np.asarray(x, dtype=np.float32).astype(np.float64)
    beta, loc, scale = float(beta), float(loc), float(scale)
    if not (beta > 0.0 and scale > 0.0 and loc == loc):
        return np.full(xd.shape, np.nan), np.array([xd.size, 0], dtype=np.int32)
    with np.errstate(all="ignore"):
        z = (xd - loc) / scale
        q, capped = gammaincc(1.0 / beta, np.abs(z) ** beta)
        c = 0.5 * np.sign(z)
        cdf = (0.5 + c) - c * q
        p = np.where(xd <= loc, 2.0 * cdf, 2.0 * (1.0 - cdf))
    return p, np.array([int(np.isnan(p).sum()), int(capped.sum())], dtype=np.int32)


def _around(v):
    """The float32 at or below v, v itself where it is a float32, and the float32 above."""
    f = np.float32(v)
    if float(f) == v:
        return [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
    lo = f if float(f) < v else np.nextafter(f, np.float32(-np.inf))
    return [lo, np.nextafter(lo, np.float32(np.inf))]


def specials(params):
    """The values every case holds first: loc (where it is a float32) and its float32 neighbours, both zeros, the largest finite
    float32 and infinity of both signs, a denormal of both signs, and the float32 values around the two x at which |z|**beta
    crosses the series / continued-fraction switch a + 1."""
    beta, loc, scale = params
    big = np.finfo(np.float32).max
    v = _around(loc)
    v = [v[len(v) // 2]] + v[:len(v) // 2] + v[len(v) // 2 + 1:]            # (loc itself, or its upper neighbour, first)
    v += [np.float32(0.0), np.float32(-0.0), big, -big, np.float32(np.inf), np.float32(-np.inf), np.float32(1e-45), np.float32(-1e-45)]
    t = (1.0 / beta + 1.0) ** (1.0 / beta) * scale
    for s in (loc + t, loc - t):
        if abs(s) < float(big):
            v += _around(s)
    return np.array(v, dtype=np.float32)


def values(M, params, seed=0):
    """float32 [M]: specials(params), then signed squares of normals times 0.02; M smaller than the specials takes their head."""
    sp = specials(params)
    if M <= sp.size:
        return sp[:M].copy()
    n = np.random.default_rng([seed, M]).normal(size=M - sp.size)
    return np.concatenate([sp, (np.sign(n) * n * n * 0.02).astype(np.float32)])


def differences(p, want, x, loc):
    """(rel, ab): the smallest rel with |p - want| <= rel * want + ABS_FLOOR wherever x <= loc (inf where want is 0 and p is further
    than ABS_FLOOR from it), and the largest |p - want| where x > loc.  NaN positions are excluded; they must be the same in both."""
    xd = np.asarray(x, dtype=np.float64)
    assert np.array_equal(np.isnan(p), np.isnan(want))
    ok = ~np.isnan(want)
    below, above = ok & (xd <= loc), ok & (xd > loc)
    with np.errstate(all="ignore"):
        over = np.maximum(np.abs(p[below] - want[below]) - ABS_FLOOR, 0.0)
        rel = float(np.max(np.where(over > 0, over / want[below], 0.0))) if below.any() else 0.0
    ab = float(np.max(np.abs(p[above] - want[above]))) if above.any() else 0.0
    return rel, ab
