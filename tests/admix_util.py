"""Inputs, tolerances and fixtures shared by tests/test_admix.py and tests/test_gpu_admix.py."""
import itertools

import numpy as np

from locator_amd import admix as A
from tests import neighbors_util as NU

VCF, SAMPLE_DATA = NU.VCF, NU.SAMPLE_DATA
EPS32 = np.float32(A.EPS)


def planted_case(N, K, C, seed, alpha=0.3, fst=0.1, missing=0.05, P=2):
    """(c int8 [N][K], Q [N][C], F [K][C]): Q ~ Dirichlet(alpha), F per site Balding-Nichols Beta(p (1 - fst) / fst,
    (1 - p)(1 - fst) / fst) around an ancestral p ~ U(0.05, 0.95), counts Binomial(P, Q F'), `missing` of the calls missing."""
    rng = np.random.default_rng(seed)
    Q = rng.dirichlet(np.full(C, alpha), N)
    p = rng.uniform(0.05, 0.95, K)
    s = (1.0 - fst) / fst
    F = rng.beta((p * s)[:, None], ((1.0 - p) * s)[:, None], (K, C))
    c = rng.binomial(P, np.clip(Q @ F.T, 0.0, 1.0)).astype(np.int8)
    c[rng.random((N, K)) < missing] = -1
    return c, Q, F


def edge_case(N, K, C, seed, P=2, missing=0.1):
    """(c int8 [N][K], Q float32 [N][C], F float32 [K][C]) at the bounds of the model: 20 % of F at EPS, 20 % at 1 - EPS, the sites
    3, 10, 17, ... with all clusters at one bound; a fifth of the samples with entries of Q at EPS (rows renormalised by the
    model's own projection); sample N // 2 and site K // 2 all missing (where there are three or more).  The counts are drawn
    from the model, so a site at a bound is almost monomorphic, as it is in a fit.
    The all-bound sites start at site 3, not 0: a panel of ONE site that is all-bound has an ll of a few log(1 - 1e-5) and nothing
    else, and no fp32 h = sum Q F within 2^-24 of 1 can give that to a relative bound (step_host(float32) itself misses LL_BOUND
    there by factors of 2 to 76); among other sites such terms are their share of the sum."""
    rng = np.random.default_rng(seed)
    F = rng.uniform(0.05, 0.95, (K, C))
    u = rng.random((K, C))
    F[u < 0.2] = A.EPS
    F[u > 0.8] = 1.0 - A.EPS
    F[3::7] = np.where(rng.random((len(F[3::7]), 1)) < 0.5, A.EPS, 1.0 - A.EPS)
    Q = rng.dirichlet(np.full(C, 0.5), N)
    low = rng.random((N, C)) < 0.2
    low[:, 0] = False                                                            # every row keeps a free entry
    Q[low & (np.arange(N) % 5 == 0)[:, None]] = 0.0
    Q32, F32 = A.project(Q.astype(np.float32), F.astype(np.float32))
    c = rng.binomial(P, np.clip(Q32.astype(np.float64) @ F32.astype(np.float64).T, 0.0, 1.0)).astype(np.int8)
    c[rng.random((N, K)) < missing] = -1
    if N >= 3:
        c[N // 2] = -1
    if K >= 3:
        c[:, K // 2] = -1
    return c, Q32, F32


def best_permutation_rmse(Q, truth):
    """The smallest root-mean-square difference of Q [N][C] from the planted Q over the C! labellings (C <= 6 here)."""
    Q, truth = np.asarray(Q, dtype=np.float64), np.asarray(truth, dtype=np.float64)
    C = Q.shape[1]
    assert C <= 6 and Q.shape == truth.shape
    return min(float(np.sqrt(((Q[:, list(perm)] - truth) ** 2).mean())) for perm in itertools.permutations(range(C)))


def step_tolerance(N, K):
    """The relative bound of an fp32 step against the float64 one: a float32 sum of at most max(N, K) non-negative terms in any
    order stays within max(N, K) 2^-24 of the exact sum, the handful of products, quotients and the reciprocal around it add
    less than 32 more; doubled (both the sums over samples and over sites enter a second step's input): (max(N, K) + 32) 2^-23."""
    return (max(N, K) + 32) * 2.0 ** -23


LL_BOUND = (A.LL_RUN + 8) * 2.0 ** -23           # relative, of ll: fp32 runs of at most LL_RUN terms of one sign, logf, the products


def step_errors(got, want, N, K):
    """(largest error / bound over Q', F', 1 - F' and ll, details) of a step `got` against the float64 step `want`: relative on
    Q' and F'; on 1 - F' relative too, plus an absolute 2^-23 (a float32 F' next to 1 cannot say 1 - F' more finely than its own
    spacing there, 2^-24, whatever the arithmetic); relative LL_BOUND on ll."""
    tol = step_tolerance(N, K)
    Qg, Fg, llg = (np.asarray(got[0], dtype=np.float64), np.asarray(got[1], dtype=np.float64), float(got[2]))
    Qw, Fw, llw = want
    ratios = {"Q": float((np.abs(Qg - Qw) / Qw).max() / tol) if Qw.size else 0.0,
              "F": float((np.abs(Fg - Fw) / Fw).max() / tol) if Fw.size else 0.0,
              "1-F": float((np.abs((1.0 - Fg) - (1.0 - Fw)) / (tol * (1.0 - Fw) + 2.0 ** -23)).max()) if Fw.size else 0.0,
              "ll": abs(llg - llw) / (LL_BOUND * abs(llw)) if llw != 0 else (0.0 if llg == 0 else np.inf)}
    return max(ratios.values()), ratios
