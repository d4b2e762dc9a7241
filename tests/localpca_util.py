"""Inputs shared by tests/test_localpca.py and tests/test_gpu_localpca.py (the localpca command), on top of tests/pca_util.py."""
import numpy as np

from tests import pca_util as U

VCF, SAMPLE_DATA, U24 = U.VCF, U.SAMPLE_DATA, U.U24
PLANTED = (4, 5, 6)                                # the windows of `planted` that follow y


def planted(N=130, S=96, W=12, seed=3):
    """(c [N][W S], locs [N][2], win [W][2]): samples uniform in the unit square; the sites of windows 4 .. 6 follow y with
    frequency 0.15 + 0.7 y, the rest x with 0.1 + 0.8 x; binomial(2) counts, 5 % of the calls missing.

    With the float64 definition (npc 2, mds 2) seed 3 gives: distances within either class <= 0.393, between the classes
    >= 1.405; robust scores on axis 1 at most 1.07 in magnitude on the nine plain windows and 216.8 .. 216.9 on the planted
    ones, on axis 2 at most 1.24 against 3.9 .. 11.4 (tests/test_localpca.py asserts the conditions the other tests rely
    on: within < between / 2, plain < 2 and planted > 6 on axis 1)."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0.0, 1.0, (N, 2))
    on_y = np.isin(np.arange(W * S) // S, PLANTED)
    freq = np.where(on_y[None], 0.15 + 0.7 * xy[:, 1:], 0.1 + 0.8 * xy[:, :1])
    c = rng.binomial(2, freq).astype(np.int8)
    c[rng.random((N, W * S)) < 0.05] = -1
    win = np.array([(w * S, (w + 1) * S) for w in range(W)], dtype=np.int64)
    return c, xy * np.array([[40.0, 25.0]]), win


def write_planted(tmp_path, **kw):
    """The planted fixture as files: (vcf path, sample data path, c, locs, win).  Every site passes the default filter."""
    c, locs, win = planted(**kw)
    samples = [f"s{i}" for i in range(len(c))]
    vcf = U.write_vcf(str(tmp_path / "planted.vcf"), c, samples)
    sd = U.write_sample_data(str(tmp_path / "planted.txt"), samples, locs)
    return vcf, sd, c, locs, win


def window_bound(c, mean, scale, win):
    """[W][N][N]: the element bound of an fp32 window matrix, (S_w + 8) 2^-24 sum_{k in w} |z_ik| |z_jk| (pca_util.grm_bound
    over the window's own sites)."""
    from locator_amd import pca as P
    az = np.abs(P.z_host(c, mean, scale))
    return np.stack([(v1 - v0 + 8) * U24 * (az[:, v0:v1] @ az[:, v0:v1].T) for v0, v1 in win])


def definitions32(c, mean, scale, win, used, npc):
    """(lam [W][npc], U [W][N][npc]) of the windows with z and G_w formed in float32 NumPy: the yardstick of what fp32 window
    matrices do to the distances."""
    from locator_amd import pca as P
    z = ((c.astype(np.float32) - mean[None]) * scale[None]).astype(np.float32)
    z[c < 0] = 0.0
    out = [P.components((z[:, v0:v1] @ z[:, v0:v1].T).astype(np.float64), int(k), npc)[:2] for (v0, v1), k in zip(win, used)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def read_windows(out):
    """The windows table as (header, {column: list of strings})."""
    head, rows = U.read_table(out + "_localpca_windows.txt")
    return head, {h: [r[i] for r in rows] for i, h in enumerate(head)}
