"""Inputs, tolerances and fixtures shared by tests/test_spa.py and tests/test_gpu_spa.py."""
import numpy as np

from locator_amd import spa as S
from tests import neighbors_util as NU
from tests.pca_util import clines, write_sample_data, write_vcf  # noqa: F401  (re-exported to the two test files)

VCF, SAMPLE_DATA = NU.VCF, NU.SAMPLE_DATA


def surface_counts(K, N, seed, P=2, missing=0.1):
    """(ct int8 [K][N], xy float32 [N][2]): counts drawn from random logistic surfaces over standard-normal coordinates, with
    `missing` of the calls missing; every site has its own slope and level."""
    rng = np.random.default_rng(seed)
    xy = rng.normal(size=(N, 2)).astype(np.float32)
    th = rng.normal(size=(K, 3)) * np.array([[1.0, 1.0, 1.5]])
    f = 1.0 / (1.0 + np.exp(-(th[:, :1] * xy[None, :, 0] + th[:, 1:2] * xy[None, :, 1] + th[:, 2:])))
    ct = rng.binomial(P, f).astype(np.int8)
    ct[rng.random((K, N)) < missing] = -1
    return ct, xy


def masks(N, seed):
    """Several w: everybody, a random 70 %, every third sample left out (a fold), nobody."""
    rng = np.random.default_rng(seed)
    return [np.ones(N, dtype=np.uint8), (rng.random(N) < 0.7).astype(np.uint8), (np.arange(N) % 3 != 1).astype(np.uint8),
            np.zeros(N, dtype=np.uint8)]


def fit_tolerance(ct, P, xy, w, ridge, iters):
    """(theta64 float64 [K][4], used, tol float64 [K]): the float64 fit before its rounding to float32 (spa.fit_state) and the
    device's parameter tolerance per site, 8 times the fixture's host figure: the largest |fit_state(float32) -
    fit_state(float64)| over the three parameters of the used sites, both taken BEFORE the rounding to float32 and computed
    from the host definition alone.  On a fixture of one or a few sites that figure can be small by chance (a float32 state that
    happens to lie next to the float64 one; seen on N = 64, K = 1 with the rounded forms: 0.0, the device 2^-24 away), which
    would ask of the device a correctly rounded result; so per site the figure is floored at half the float32 spacing of that
    site's own largest parameter, the error any float32 value of it carries.  Wherever the measured figure is larger - every
    fixture of more than a few sites - it stands as measured."""
    t64, used = S.fit_state(ct, P, xy, w, ridge, iters)
    t32, used32 = S.fit_state(ct, P, xy, w, ridge, iters, dtype=np.float32)
    assert np.array_equal(used, used32)
    on = used.astype(bool)
    if not on.any():
        return t64, used, np.zeros(len(used))
    host = float(np.abs(t32[on, :3].astype(np.float64) - t64[on, :3]).max())
    floor = 0.5 * np.spacing(np.abs(t64[:, :3]).max(axis=1).astype(np.float32)).astype(np.float64)
    return t64, used, 8.0 * np.maximum(host, floor)


def host_figure(tol, used):
    """The largest per-site figure behind a fit_tolerance (tests print it)."""
    on = np.asarray(used).astype(bool)
    return float(tol[on].max()) / 8.0 if on.any() else 0.0


def grid_case(Q, K, G, seed, P=2, missing=0.2):
    """(c int8 [Q][K], theta float32 [K][4], used uint8 [K], gx, gy float32 [G]): counts as neighbors_util.counts with the
    all-missing rows 0 and Q // 2 (where there are three rows or more), random surfaces, 15 % of the sites unused; every other
    unused site keeps finite garbage in theta (the kernel must not multiply it in)."""
    rng = np.random.default_rng(seed)
    c = NU.counts(Q, K, seed + 1, P=P, missing=missing)
    if Q >= 3:
        c[0] = -1
        c[Q // 2] = -1
    theta = (rng.normal(size=(K, 4)) * np.array([[1.0, 1.0, 2.0, 1.0]])).astype(np.float32)
    used = (rng.random(K) < 0.85).astype(np.uint8)
    off = np.flatnonzero(used == 0)
    theta[off[::2]] = 0
    gx, gy = rng.uniform(-2.5, 2.5, G).astype(np.float32), rng.uniform(-2.5, 2.5, G).astype(np.float32)
    return c, theta, used, gx, gy


def top_two_margin(ll):
    """[Q]: the largest ll of a row minus its second largest (0 on a tie)."""
    part = np.partition(np.asarray(ll, dtype=np.float64), -2, axis=1)
    return part[:, -1] - part[:, -2]
