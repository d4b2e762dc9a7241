"""Inputs, window layouts, attributes and allowances shared by tests/test_ancestry.py and tests/test_gpu_ancestry.py.  The cases
are paint_util's."""
import numpy as np

from locator_amd import ancestry as AN
from tests import paint_util as U

SIX = ("h", "donor", "owner", "rec", "rho", "theta")
FULL = 64                              # the channels of `attributes`; fewer are a selection of them (SUBSETS)
SUBSETS = {1: [63], 3: [0, 40, 63], 63: list(range(62)) + [63], 64: list(range(64))}


def attributes(case, seed):
    """v float64 [64][H]: 31 one-hot label channels (a column's label is one of 32, so that one label has no channel), 32 of
    uniform values in [-1, 1] and a channel of ones; NaN at every column that is no donor."""
    H = len(case["donor"])
    rng = np.random.default_rng(seed)
    label = rng.integers(0, 32, H)
    v = np.concatenate([(label[None, :] == np.arange(31)[:, None]).astype(np.float64), rng.uniform(-1.0, 1.0, (32, H)), np.ones((1, H))])
    v[:, np.asarray(case["donor"]) == 0] = np.nan
    return v


def layouts(K):
    """{name: win int32 [W][2]}: all sites in one window; one site a window; windows of 5 with a one-site gap between them and
    a ragged last window; a single interior window.  Those that K admits."""
    out = {"all": [[0, K]], "each": [[j, j + 1] for j in range(K)]}
    if K >= 7:
        out["fives"] = [[s, min(s + 5, K)] for s in range(0, K, 6)]
    if K >= 3:
        out["interior"] = [[K // 3, max(K // 3 + 1, (2 * K) // 3)]]
    return {name: np.array(w, dtype=np.int32) for name, w in out.items()}


def host(case, v, win, dtype=np.float64):
    return AN.local_host(*(case[k] for k in SIX), v, win, dtype=dtype)


def means(out, win):
    """out [R][W][C] / n_sites: what the tests compare, float64."""
    win = np.asarray(win)
    return np.asarray(out, dtype=np.float64) / (win[:, 1] - win[:, 0])[None, :, None]


def distance(got, want, win):
    """The largest absolute difference of the window means."""
    d = np.abs(means(got, win) - means(want, win))
    return float(d.max()) if d.size else 0.0


def allowance(case, v, win, want=None):
    """(allowance, the float64 answer): paint_util.FACTOR times the distance of local_host(float32) from local_host(float64) on
    the case, floored at paint_util.FLOOR: the project's convention."""
    want = host(case, v, win) if want is None else want
    return max(U.FACTOR * distance(host(case, v, win, np.float32)[0], want[0], win), U.FLOOR), want


def spliced(seed, K=320):
    """A recipient that is one donor's alleles below K / 2 and another's, of the other label, above: (case with the recipient as
    the last individual's first haplotype, label [columns] 0 / 1 by x >= 0.5, (label below, label above))."""
    hap, x = U.planted(40, K, seed, missing=0)
    lab = (x >= 0.5).astype(np.int64)
    a, b = int(np.flatnonzero(lab == 0)[0]), int(np.flatnonzero(lab == 1)[0])
    mosaic = np.concatenate([hap[:K // 2, 2 * a], hap[K // 2:, 2 * b]])
    h = np.concatenate([hap, mosaic[:, None], mosaic[:, None]], axis=1)
    donor = np.concatenate([np.ones(80, dtype=np.uint8), np.zeros(2, dtype=np.uint8)])
    owner = np.repeat(np.arange(41, dtype=np.int32), 2)
    case = {"h": h, "donor": donor, "owner": owner, "rec": np.array([80], dtype=np.int32), "rho": np.full(K, 0.05),
            "theta": AN.PT.default_theta(80)}
    return case, np.concatenate([np.repeat(lab, 2), [-1, -1]]), (0, 1)
