"""The spa command without a GPU (locator_amd/spa.py): the binding of include/locator_hip_spa.h, fit_host against the stated
objective, grid_host and peaks by hand, the fold rule, the --host command on the golden VCF with its summary pinned, the
refusals, and the unchanged bytes of the neighbors and pca commands."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from locator_amd import baselines as BL
from locator_amd import neighbors as NB
from locator_amd import pca as PC
from locator_amd import spa as S
from tests import spa_util as U


# ------------------------------------------------------------------ the binding
def test_spa_header_is_bound_as_the_other_headers_are():
    from locator_amd import _abi
    from tests.abi_util import check_extension
    vp, i64, i = C.c_void_p, C.c_int64, C.c_int
    check_extension("spa", {"loc_spa_fit": (i, [vp, i64, i, i64, i, vp, vp, C.c_float, i, vp, vp, vp]),
                            "loc_spa_grid_work_bytes": (i64, [i, i64, i, i]),
                            "loc_spa_grid": (i, [vp, i, i64, i64, i, vp, vp, vp, vp, i, i, vp, vp, i64, vp])},
                    {"LOC_SPA_TILE", "LOC_SPA_BLOCK", "LOC_SPA_MAX_STEP", "LOC_SPA_MAX_ITERS", "LOC_SPA_MAX_NODES",
                     "LOC_SPA_FIT_SITES", "LOC_SPA_FIT_CHUNK", "LOC_SPA_TILE_SAMPLES"})
    assert (_abi.LOC_SPA_TILE, _abi.LOC_SPA_BLOCK, _abi.LOC_SPA_MAX_STEP, _abi.LOC_SPA_MAX_ITERS, _abi.LOC_SPA_MAX_NODES) == (
        S.TILE, S.BLOCK, S.MAX_STEP, S.MAX_ITERS, S.MAX_NODES) == (128, 32, 2, 64, 128 * 128)
    assert _abi.LOC_SPA_TILE_SAMPLES == S.TILE_SAMPLES == 256
    assert S.GRID_RANGE[1] ** 2 == S.MAX_NODES


# ------------------------------------------------------------------ fit_host
def test_the_gradient_of_the_stated_objective_vanishes_at_the_fit():
    for P in (1, 2):
        ct, xy = U.surface_counts(40, 300, 3 + P, P=P)
        for ridge in (1.0, 0.25):
            theta, used = S.fit_host(ct, P, xy, np.ones(300, dtype=np.uint8), ridge, 12)
            assert theta.dtype == np.float32 and theta.shape == (40, 4) and used.dtype == np.uint8 and used.all()
            # the solution in float64, before theta is rounded to float32 (a float32 ulp of a slope moves the gradient by 1e-5)
            state, _ = S.fit_state(ct, P, xy, np.ones(300, dtype=np.uint8), ridge, 12)
            assert state.dtype == np.float64 and np.array_equal(state.astype(np.float32), theta)
            g = S.objective_gradient(ct, P, xy, np.ones(300), ridge, state)
            assert np.abs(g).max() < 1e-9, np.abs(g).max()
            assert np.abs(state[:, :3] - _fit64(ct, P, xy, np.ones(300), ridge, 12)).max() < 1e-12
            assert (theta[:, 3] < 1e-9).all() and np.abs(theta[:, :2]).max() > 0.3      # converged, and there are slopes
    # ... and it is a maximum of the objective, not another stationary point: moving any parameter lowers it
    ct, xy = U.surface_counts(5, 200, 9)
    w = np.ones(200)
    th = _fit64(ct, 2, xy, w, 1.0, 12)
    for j in range(3):
        for d in (-1e-3, 1e-3):
            moved = th.copy()
            moved[:, j] += d
            assert (_objective(ct, 2, xy, w, 1.0, moved) < _objective(ct, 2, xy, w, 1.0, th)).all()


def _fit64(ct, P, xy, w, ridge, iters):
    """fit_host's parameters before they are rounded to float32: the same Newton steps written out independently, float64,
    by numpy.linalg.solve on the 3 x 3 system (no clamp is reached on these fixtures)."""
    on = (ct >= 0) & (np.asarray(w)[None] == 1)
    x = np.asarray(xy, dtype=np.float64)
    X = np.stack([x[:, 0], x[:, 1], np.ones(len(x))], axis=1)
    out = np.zeros((len(ct), 3))
    for k in range(len(ct)):
        A, cv = X[on[k]], ct[k][on[k]].astype(np.float64)
        th = np.array([0.0, 0.0, np.log(cv.sum() / (P * len(cv) - cv.sum()))])
        R = np.diag([ridge, ridge, 0.0])
        for _ in range(iters):
            f = 1.0 / (1.0 + np.exp(-(A @ th)))
            step = np.linalg.solve((A * (P * f * (1 - f))[:, None]).T @ A + R, A.T @ (cv - P * f) - R @ th)
            assert np.abs(step).max() < S.MAX_STEP
            th = th + step
        out[k] = th
    return out


def _objective(ct, P, xy, w, ridge, th):
    on = (ct >= 0) & (np.asarray(w)[None] == 1)
    x = np.asarray(xy, dtype=np.float64)
    t = th[:, :1] * x[None, :, 0] + th[:, 1:2] * x[None, :, 1] + th[:, 2:]
    return np.where(on, ct * t - P * S.softplus64(t), 0.0).sum(axis=1) - 0.5 * ridge * (th[:, 0] ** 2 + th[:, 1] ** 2)


def test_fit_host_is_the_written_out_newton_iteration():
    ct, xy = U.surface_counts(30, 120, 11)
    w = U.masks(120, 1)[1]
    theta, used = S.fit_host(ct, 2, xy, w, 1.0, 12)
    assert used.all() and np.abs(S.fit_state(ct, 2, xy, w, 1.0, 12)[0][:, :3] - _fit64(ct, 2, xy, w, 1.0, 12)).max() < 1e-12
    assert np.abs(theta[:, :3] - _fit64(ct, 2, xy, w, 1.0, 12)).max() < 1e-6
    # one step from the start is clamped where the unclamped step is larger than the limit
    hard = np.array([[0] * 10 + [2] * 10], dtype=np.int8)
    far = np.stack([np.r_[np.full(10, -1.0), np.full(10, 1.0)], np.zeros(20)], axis=1).astype(np.float32)
    one, _ = S.fit_host(hard, 2, far, np.ones(20), 0.0, 1)
    assert one[0, 0] == S.MAX_STEP and one[0, 3] == S.MAX_STEP                     # perfectly separated: the step is cut to 2


def test_unused_sites():
    ct, xy = U.surface_counts(6, 50, 21)
    ct[0] = -1                                               # all missing
    ct[1] = np.where(ct[1] >= 0, 0, -1)                      # monomorphic 0
    ct[2] = np.where(ct[2] >= 0, 2, -1)                      # monomorphic P
    w = np.zeros(50, dtype=np.uint8)
    w[:30] = 1
    ct[3, :30] = -1                                          # called only outside w
    ct[4, :30] = np.where(np.arange(30) == 7, 1, 0)          # one copy of the allele: used
    theta, used = S.fit_host(ct, 2, xy, w, 1.0, 12)
    assert used.tolist() == [0, 0, 0, 0, 1, 1] and not theta[:4].any() and theta[4:, 2].all()
    assert np.isfinite(theta).all()
    none, used0 = S.fit_host(ct, 2, xy, np.zeros(50), 1.0, 12)
    assert not used0.any() and not none.any()
    t32, u32 = S.fit_host(ct, 2, xy, w, 1.0, 12, dtype=np.float32)
    assert np.array_equal(u32, used) and not t32[:4].any() and np.abs(t32 - theta)[:, :3].max() < 1e-4
    # haploid counts: 1 is monomorphic there
    h = np.where(ct >= 1, 1, ct).astype(np.int8)
    assert S.fit_host(h, 1, xy, w, 1.0, 3)[1].tolist() == [0, 0, 0, 0, 1, 1]


def test_all_zero_coordinates_leave_the_slopes_at_zero():
    ct, _ = U.surface_counts(12, 80, 31)
    zero = np.zeros((80, 2), dtype=np.float32)
    for dtype in (np.float64, np.float32):
        theta, used = S.fit_host(ct, 2, zero, np.ones(80), 1.0, 12, dtype=dtype)
        on = ct >= 0
        p = np.where(on, ct, 0).sum(axis=1) / (2.0 * on.sum(axis=1))
        assert used.all() and not theta[:, 0].any() and not theta[:, 1].any()          # exactly 0
        assert np.abs(theta[:, 2] - np.log(p / (1 - p))).max() < (1e-6 if dtype is np.float32 else 2e-7)


def test_the_mask_equals_deleting_the_rows():
    ct, xy = U.surface_counts(25, 90, 41)
    for w in U.masks(90, 2)[:3]:
        keep = w == 1
        a, ua = S.fit_host(ct, 2, xy, w, 1.0, 12)
        b, ub = S.fit_host(ct[:, keep], 2, xy[keep], np.ones(int(keep.sum())), 1.0, 12)
        assert np.array_equal(ua, ub) and np.abs(a[:, :3] - b[:, :3]).max() <= 2.4e-7   # the sums run over other lengths
    # a NaN coordinate outside w is never read
    bad = xy.copy()
    bad[~(U.masks(90, 2)[1] == 1)] = np.nan
    assert np.array_equal(S.fit_host(ct, 2, bad, U.masks(90, 2)[1], 1.0, 12)[0], S.fit_host(ct, 2, xy, U.masks(90, 2)[1], 1.0, 12)[0])


# ------------------------------------------------------------------ grid_host
def test_grid_host_by_hand_on_two_sites():
    theta = np.array([[0.5, -0.25, 0.125, 0.0], [-1.0, 2.0, 0.5, 0.0], [3.0, 3.0, 3.0, 0.0]], dtype=np.float32)
    used = np.array([1, 1, 0], dtype=np.uint8)
    gx, gy = np.array([0.0, 1.0, -2.0], dtype=np.float32), np.array([0.0, 2.0, 1.0], dtype=np.float32)
    t = np.array([[0.125, 0.125, -1.125], [0.5, 3.5, 4.5]])                      # ax gx + ay gy + b: exact in fp32
    assert np.array_equal(S.surface(theta, gx, gy)[:2].astype(np.float64), t)
    sp = np.log1p(np.exp(t))
    c = np.array([[2, 1, 2], [0, -1, 1], [-1, -1, 2], [1, 0, -1]], dtype=np.int8)
    ll = S.grid_host(c, 2, theta, used, gx, gy)
    want = np.stack([2 * t[0] - 2 * sp[0] + 1 * t[1] - 2 * sp[1],                # both sites called
                     0 * t[0] - 2 * sp[0],                                       # the second missing
                     np.zeros(3),                                                # only the unused site called
                     1 * t[0] - 2 * sp[0] + 0 * t[1] - 2 * sp[1]])
    assert ll.shape == (4, 3) and np.abs(ll - want).max() < 1e-14 and not ll[2].any()
    assert np.array_equal(ll, S.grid_host(c, 2, theta, used, gx, gy, chunk=1))
    h = S.grid_host(np.minimum(c, 1), 1, theta, used, gx, gy)                    # haploid: P = 1
    assert np.abs(h[0] - (t[0] - sp[0] + t[1] - sp[1])).max() < 1e-14
    # t is the float32 value: three roundings, not the float64 expression
    th = np.array([[0.1, 0.3, 0.7, 0.0]], dtype=np.float32)
    g = np.array([1.1], dtype=np.float32)
    t32 = np.float32(np.float32(th[0, 0] * g[0]) + np.float32(th[0, 1] * g[0])) + th[0, 2]
    assert S.surface(th, g, g)[0, 0] == t32 and float(t32) != float(th[0, 0]) * float(g[0]) + float(th[0, 1]) * float(g[0]) + float(th[0, 2])
    one = S.grid_host(np.array([[1]], dtype=np.int8), 2, th, [1], g, g)
    assert one[0, 0] == float(t32) - 2 * S.softplus64(float(t32))
    b = S.ll_bound(c, 2, theta, used, gx, gy, 2)
    assert not b[2].any() and (b[[0, 1, 3]] > 0).all() and S.sites_per_group(1000, 3) == 352 and S.sites_per_group(33, 5) == 32


# ------------------------------------------------------------------ peaks
def test_peaks():
    n = 8
    xs, ys = np.linspace(-1, 1, n).astype(np.float32), np.linspace(10, 24, n).astype(np.float32)
    hx, hy = 2.0 / 7, 2.0
    gx, gy = S.flat_nodes(xs, ys)
    assert gx[n + 3] == xs[3] and gy[n + 3] == ys[1]                             # g = iy n + ix

    def quad(cx, cy):
        return -(gx.astype(np.float64) - cx) ** 2 - 0.01 * (gy.astype(np.float64) - cy) ** 2

    plateau = np.full(n * n, -9.0)
    plateau[4 * n + 2] = plateau[4 * n + 3] = plateau[4 * n + 4] = 1.0           # three equal nodes in a row
    ll = np.stack([quad(float(xs[3]) + 0.3 * hx, float(ys[5]) - 0.2 * hy),       # a parabola: the vertex is found
                   quad(-5.0, 17.0),                                             # the peak left of the grid, y between two nodes
                   np.zeros(n * n),                                              # a tie everywhere
                   plateau])
    xy, node, border = S.peaks(ll, xs, ys)
    assert xy.shape == (4, 2) and node.dtype == np.int64
    # ties go to the lowest index: y = 17 lies between the nodes 16 and 18, the all-equal row sits on node 0
    assert node.tolist() == [5 * n + 3, 3 * n + 0, 0, 4 * n + 2] and border.tolist() == [False, True, True, False]
    assert np.allclose(xy[0], [float(xs[3]) + 0.3 * hx, float(ys[5]) - 0.2 * hy], atol=1e-6)
    assert xy[1, 0] == float(xs[0]) and abs(xy[1, 1] - 17.0) < 1e-6              # no refinement on the border axis, the other is
    assert xy[2].tolist() == [float(xs[0]), float(ys[0])]
    # the plateau: on x left -9, mid 1, right 1 -> the vertex half a step to the right; on y -9, 1, -9 -> the node itself
    assert abs(xy[3, 0] - (float(xs[2]) + 0.5 * hx)) < 1e-12 and xy[3, 1] == float(ys[4])
    # by hand: left 1 - 1e-3, mid 1, right 1 - 3e-3 -> offset 0.5 (left - right) / (left - 2 mid + right) = -0.25 steps
    up = np.full((1, n * n), -9.0)
    up[0, 3 * n + 3], up[0, 3 * n + 2], up[0, 3 * n + 4] = 1.0, 1.0 - 1e-3, 1.0 - 3e-3
    at, nd, _ = S.peaks(up, xs, ys)
    assert nd[0] == 3 * n + 3 and abs(at[0, 0] - (float(xs[3]) - 0.25 * hx)) < 1e-9 and at[0, 1] == float(ys[3])
    # a flat second difference: left = mid = right cannot be at the chosen node (the left neighbour has the lower index and
    # would have won), so the flattest reachable case is mid = right with left one ulp below: the offset stays within half a
    # step, and a row whose largest value is NaN-free but constant is placed on node 0
    flat = np.full((1, n * n), -9.0)
    flat[0, 3 * n + 3] = flat[0, 3 * n + 4] = 1.0
    flat[0, 3 * n + 2] = np.nextafter(1.0, 0.0)
    at, nd, _ = S.peaks(flat, xs, ys)
    const = S.peaks(np.full((1, n * n), -3.5), xs, ys)
    assert nd[0] == 3 * n + 3 and abs(at[0, 0] - (float(xs[3]) + 0.5 * hx)) < 1e-12
    assert const[1][0] == 0 and const[0][0].tolist() == [float(xs[0]), float(ys[0])]
    # the all-missing row: NaN, and no border count
    xy, node, border = S.peaks(ll, xs, ys, placed=[True, True, False, True])
    assert np.isnan(xy[2]).all() and border.tolist() == [False, True, False, False] and np.isfinite(xy[[0, 1, 3]]).all()
    assert S.peaks(np.zeros((0, n * n)), xs, ys)[0].shape == (0, 2)


def test_grid_nodes():
    xy = np.array([[-1.0, 2.0], [3.0, 4.0], [100.0, 100.0]], dtype=np.float32)
    xs, ys = S.grid_nodes(xy, np.array([True, True, False]), 9, 0.25)
    assert xs.dtype == ys.dtype == np.float32 and len(xs) == len(ys) == 9
    assert (xs[0], xs[-1], ys[0], ys[-1]) == (-2.0, 4.0, 1.5, 4.5) and np.allclose(np.diff(xs), 0.75) and np.allclose(np.diff(ys), 0.375)
    for n in (7, 129):
        with pytest.raises(ValueError, match="must be 8 .. 128"):
            S.grid_nodes(xy, np.array([True, True, False]), n, 0.1)
    with pytest.raises(ValueError, match="sd 0"):
        S.normalise(np.array([[1.0, 2.0], [1.0, 3.0]]), np.array([True, True]))
    nxy, mean, sd = S.normalise(np.array([[1.0, 2.0], [3.0, 6.0], [np.nan, np.nan]]), np.array([True, True, False]))
    assert nxy.dtype == np.float32 and nxy.tolist() == [[-1.0, -1.0], [1.0, 1.0], [0.0, 0.0]] and mean.tolist() == [2.0, 4.0]
    assert sd.tolist() == [1.0, 2.0]                                             # the population sd


# ------------------------------------------------------------------ folds
def test_the_fold_rule():
    located = np.array([1, 0, 1, 1, 0, 1, 1, 1, 0, 1], dtype=bool)
    assert S.fold_of(located, 3).tolist() == [0, -1, 1, 2, -1, 0, 1, 2, -1, 0]
    assert S.fold_of(located, 7).tolist() == [0, -1, 1, 2, -1, 3, 4, 5, -1, 6]
    assert S.fold_of(np.zeros(3, dtype=bool), 2).tolist() == [-1, -1, -1]


# ------------------------------------------------------------------ the command
GOLDEN_ARGS = ("--max_SNPs", "300", "--seed", "1", "--folds", "3", "--grid", "8")


def run(tmp_path, name, *extra):
    out = str(tmp_path / name)
    assert S.main(["--vcf", U.VCF, "--sample_data", U.SAMPLE_DATA, "--out", out, "--silence", "--host"] + list(extra)) == 0
    return out


def test_the_host_command_on_the_golden_vcf(tmp_path, capsys):
    out = run(tmp_path, "g", "--keep_surfaces", *GOLDEN_ARGS)
    s = json.load(open(out + "_spa_summary.json"))
    assert tuple(s) == S.SUMMARY_KEYS
    assert (s["N"], s["n_located"], s["K"], s["K_used"], s["P"], s["folds"], s["grid"], s["pad"], s["ridge"], s["iters"]) == (
        500, 450, 300, 300, 2, 3, 8, 0.1, 1.0, 12)
    # pinned from the host form (float64; the last digits are left to the platform's exp and matrix product)
    assert s["error_unit"] == "map units" and s["n_border"] == 62 and s["n_unplaced"] == 0 and s["max_last_step"] < 1e-12
    assert s["median_error"] == pytest.approx(8.086970560389581, rel=1e-9) and s["r2_x"] == pytest.approx(0.7972420270831593, rel=1e-9)
    assert s["r2_y"] == pytest.approx(0.808913316383373, rel=1e-9)
    head, *rows = [line.split(",") for line in open(out + "_spa_locs.txt").read().splitlines()]
    assert head == ["x", "y", "sampleID"] and len(rows) == 500 and rows[0][2] == "msp_0"
    placed = np.array([[float(r[0]), float(r[1])] for r in rows])
    assert np.isfinite(placed).all()
    head, *sites = [line.split("\t") for line in open(out + "_spa_sites.txt").read().splitlines()]
    assert head == ["variant", "used", "ax", "ay", "b", "slope"] and len(sites) == 300
    z = np.load(out + "_spa.npz")
    assert z["theta"].shape == (4, 300, 4) and z["theta"].dtype == np.float32 and z["used"].shape == (4, 300) and z["used"][-1].all()
    assert [int(r[0]) for r in sites] == z["sites"].tolist() and len(z["xs"]) == len(z["ys"]) == 8
    th = np.array([[float(v) for v in r[2:]] for r in sites])
    assert np.array_equal(th[:, :3], z["theta"][-1][:, :3].astype(np.float64)) and np.array_equal(th[:, 3], np.hypot(th[:, 0], th[:, 1]))
    # the files are the definitions': the sites of a fit with the same draw, the folds, the fits, the grids, the peaks
    from locator_amd import genotypes as G
    vcf = G.read_vcf(U.VCF)
    np.random.seed(1)
    _, idx = G.filter_snps(vcf["calldata/GT"], min_mac=2, max_snps=300, verbose=False, sites=True)
    assert np.array_equal(z["sites"], idx)
    c, P = BL.count_matrix(vcf["calldata/GT"], idx)
    ct, _ = BL.count_matrix_sites(vcf["calldata/GT"], idx)
    locs = BL.read_locations(U.SAMPLE_DATA, vcf["samples"], S.PROG)
    located = ~np.isnan(locs).any(axis=1)
    xy, mean, sd = S.normalise(locs, located)
    xs, ys = S.grid_nodes(xy, located, 8, 0.1)
    assert np.array_equal(xs, z["xs"]) and np.array_equal(ys, z["ys"])
    fold = S.fold_of(located, 3)
    assert np.array_equal(fold, z["fold"]) and (fold[~located] == -1).all()
    for i, f in enumerate((0, 1, 2, -1)):
        theta, used = S.fit_host(ct, P, xy, (located & (fold != f)).astype(np.uint8), 1.0, 12)
        assert np.array_equal(theta, z["theta"][i]) and np.array_equal(used, z["used"][i])
        rows_f = np.flatnonzero(fold == f)
        ll = S.grid_host(c[rows_f], P, theta, used, *S.flat_nodes(xs, ys))
        assert np.array_equal(ll, z["ll_all" if f < 0 else f"ll_fold{f}"])
        at, node, _ = S.peaks(ll, xs, ys)
        assert np.array_equal(at * sd[None] + mean[None], placed[rows_f]) and np.array_equal(node, z["nodes"][rows_f])
    err = BL.errors(placed[located], locs[located])
    assert s["median_error"] == float(np.median(err)) and s["mean_error"] == float(np.mean(err))
    # a second run writes the same bytes; without --silence the four lines of the other baselines
    again = run(tmp_path, "again", "--keep_surfaces", *GOLDEN_ARGS)
    for name in ("_spa_locs.txt", "_spa_sites.txt", "_spa_summary.json", "_spa.npz"):
        assert open(again + name, "rb").read() == open(out + name, "rb").read(), name
    assert sorted(os.listdir(tmp_path)) == sorted(f"{o}{n}" for o in ("g", "again") for n in (
        "_spa_locs.txt", "_spa_sites.txt", "_spa_summary.json", "_spa.npz"))
    capsys.readouterr()
    assert S.main(["--vcf", U.VCF, "--sample_data", U.SAMPLE_DATA, "--out", str(tmp_path / "loud"), "--host", *GOLDEN_ARGS]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 4 and lines[0].startswith("R2(x)=") and lines[3] == f"median SPA held-out error {s['median_error']} (map units)"
    assert not os.path.exists(str(tmp_path / "loud_spa.npz"))


def test_longlat_and_ld_prune(tmp_path):
    plain = json.load(open(run(tmp_path, "p", *GOLDEN_ARGS) + "_spa_summary.json"))
    km = run(tmp_path, "km", "--longlat", *GOLDEN_ARGS)
    s = json.load(open(km + "_spa_summary.json"))
    assert s["error_unit"] == "km" and s["median_error"] > 50 * plain["median_error"] and s["r2_x"] == plain["r2_x"]
    assert open(km + "_spa_locs.txt").read() == open(str(tmp_path / "p_spa_locs.txt")).read()          # the model stays planar
    pruned = run(tmp_path, "ld", "--ld_prune", "0.2", "--folds", "2", "--grid", "8", "--iters", "3")
    s = json.load(open(pruned + "_spa_summary.json"))
    assert tuple(s) == S.SUMMARY_KEYS + ("ld_prune", "ld_window", "ld_window_bp", "K_before_prune")
    assert (s["K"], s["K_before_prune"], s["ld_prune"], s["iters"]) == (1996, 5830, 0.2, 3)      # the sites of neighbors --ld_prune 0.2


def test_unplaced_samples_and_unlocated_ones(tmp_path):
    c, locs = U.clines(40, 30, 7, unlocated=6)
    c[3] = -1                                                                     # a located sample without a call
    c[38] = -1                                                                    # an unlocated one
    s = S.spa(c, 2, [f"s{i}" for i in range(40)], locs, str(tmp_path / "o"), folds=4, grid=8, host=True, silence=True)
    assert s["n_unplaced"] == 2 and s["n_located"] == 34 and np.isnan(s["_xy"][[3, 38]]).all() and s["_nodes"][3] == -1
    ok = np.setdiff1d(np.arange(40), [3, 38])
    assert np.isfinite(s["_xy"][ok]).all() and (s["_nodes"][ok] >= 0).all()
    rows = open(str(tmp_path / "o_spa_locs.txt")).read().splitlines()
    assert rows[4] == ",,s3" and rows[39] == ",,s38" and len(rows) == 41
    # the unlocated samples come from the fit on all located samples
    located = ~np.isnan(locs).any(axis=1)
    xy, mean, sd = S.normalise(locs, located)
    xs, ys = S.grid_nodes(xy, located, 8, 0.1)
    theta, used = S.fit_host(c.T, 2, xy, located.astype(np.uint8), 1.0, 12)
    assert np.array_equal(theta, s["_theta"][-1])
    at = S.peaks(S.grid_host(c[34:38], 2, theta, used, *S.flat_nodes(xs, ys)), xs, ys)[0]
    assert np.array_equal(at * sd[None] + mean[None], s["_xy"][34:38])
    # the planted clines are found: the error is a fraction of the 40 x 25 map
    assert s["median_error"] < 8 and s["r2_x"] > 0.6


# ------------------------------------------------------------------ stops and errors
def test_without_a_gpu_the_command_stops_unless_host(tmp_path, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match="no GPU visible.*loc_spa_fit.*loc_spa_grid.*--host"):
        S.main(["--vcf", U.VCF, "--sample_data", U.SAMPLE_DATA, "--out", str(tmp_path / "o")])
    assert not os.listdir(tmp_path)


def test_refusals(tmp_path, capsys):
    base = ["--vcf", U.VCF, "--sample_data", U.SAMPLE_DATA, "--out", str(tmp_path / "o"), "--host", "--silence"]
    for extra, text in ((["--folds", "1"], "--folds must be 2 .."), (["--grid", "7"], "--grid must be 8 .. 128"),
                        (["--grid", "129"], "--grid must be 8 .. 128"), (["--pad", "-0.1"], "--pad must be"),
                        (["--pad", "nan"], "--pad must be"), (["--ridge", "-1"], "--ridge must be"),
                        (["--ridge", "inf"], "--ridge must be"), (["--iters", "0"], "--iters must be 1 .. 64"),
                        (["--iters", "65"], "--iters must be 1 .. 64"), (["--zarr", "x"], "exactly one of --vcf / --zarr / --matrix"),
                        (["--npc", "3"], "unrecognized arguments"), (["--ld_prune", "0.2", "--ld_window", "0"], "--ld_window must be")):
        with pytest.raises(SystemExit) as e:
            S.main(base + extra)
        assert e.value.code == 2 and text in capsys.readouterr().err, extra
    with pytest.raises(SystemExit, match="--folds must be 2 .. the number of located samples \\(450\\)"):
        S.main(base + ["--folds", "451", "--max_SNPs", "50", "--seed", "1"])
    assert not os.listdir(tmp_path)
    c, locs = U.clines(20, 10, 1, unlocated=0)
    names = [f"s{i}" for i in range(20)]
    flat = locs.copy()
    flat[:, 1] = 3.0
    with pytest.raises(ValueError, match="sd 0"):
        S.spa(c, 2, names, flat, None, folds=2, grid=8, host=True, silence=True)
    none = np.full_like(locs, np.nan)
    none[0] = 1.0
    with pytest.raises(SystemExit, match="fewer than 2 samples"):
        S.spa(c, 2, names, none, None, folds=2, grid=8, host=True, silence=True)
    ct = np.ascontiguousarray(c.T)
    for kw, text in (({"iters": 0}, "iters = 0"), ({"iters": 65}, "iters = 65"), ({"ridge": -1.0}, "ridge = -1"),
                     ({"ridge": float("nan")}, "ridge = nan")):
        with pytest.raises(ValueError, match=text):
            S.fit_host(ct, 2, locs, np.ones(20), **{"ridge": 1.0, "iters": 12, **kw})
    with pytest.raises(ValueError, match="a count of 3"):
        S.fit_host(np.full((2, 4), 3, dtype=np.int8), 2, np.zeros((4, 2)), np.ones(4), 1.0, 1)
    with pytest.raises(ValueError, match="a count of 2 exceeds the ploidy 1"):
        S.grid_host(np.full((2, 4), 2, dtype=np.int8), 1, np.zeros((4, 4)), np.ones(4), np.zeros(3), np.zeros(3))


# ------------------------------------------------------------------ the other baselines
KNN_LOCS_SHA256 = "466f8d11a219b58ade00fda766a96c45b2d0e07062144ee545a4c1f49450ff4c"
NEIGHBORS_SHA256 = "49481cae9efacce8cddd747bd50f93091fed397e65a4d0dfadc544ce07d69007"


def test_neighbors_and_pca_write_what_they_wrote(tmp_path):
    """The neighbors files that hold only integer sums, their quotients and means in rank order are pinned by digest (written
    by the commit before the spa command existed); the pca files hold the eigenvectors of a platform's eigh and are compared
    with a run of the command's functions called directly, as they were before the spa command existed."""
    from locator_amd import genotypes as G
    common = ["--vcf", U.VCF, "--sample_data", U.SAMPLE_DATA, "--host", "--silence", "--max_SNPs", "400", "--seed", "11"]
    out = str(tmp_path / "nb")
    assert NB.main(common + ["--out", out, "--kmax", "8"]) == 0
    assert hashlib.sha256(open(out + "_knn_locs.txt", "rb").read()).hexdigest() == KNN_LOCS_SHA256
    assert hashlib.sha256(open(out + "_neighbors.txt", "rb").read()).hexdigest() == NEIGHBORS_SHA256
    assert tuple(json.load(open(out + "_knn_summary.json"))) == NB.SUMMARY_KEYS
    cmd, fn = str(tmp_path / "pc"), str(tmp_path / "fn")
    assert PC.main(common + ["--out", cmd, "--npc", "4"]) == 0
    np.random.seed(11)
    data = G.read_vcf(U.VCF)
    gt, samples = data["calldata/GT"], data["samples"]
    _, idx = G.filter_snps(gt, min_mac=2, max_snps=400, verbose=False, sites=True)
    c, P = BL.count_matrix(gt, idx)
    PC.pca(c, P, samples, BL.read_locations(U.SAMPLE_DATA, samples, PC.PROG), fn, npc=4, host=True, silence=True, sites=idx)
    for name in ("_pca.txt", "_pca_eigenvalues.txt", "_pca_locs.txt", "_pca_summary.json"):
        assert open(cmd + name, "rb").read() == open(fn + name, "rb").read(), name
    assert tuple(json.load(open(cmd + "_pca_summary.json"))) == PC.SUMMARY_KEYS
    assert sorted(os.listdir(tmp_path)) == sorted([f"nb{n}" for n in ("_knn_locs.txt", "_neighbors.txt", "_knn_summary.json")]
                                                  + [f"{o}{n}" for o in ("pc", "fn") for n in (
                                                      "_pca.txt", "_pca_eigenvalues.txt", "_pca_locs.txt", "_pca_summary.json")])
