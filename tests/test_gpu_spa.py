"""The spa command on the device (locator_amd/csrc/spa_kernels.hip).

loc_spa_grid against spa.grid_host within the derived bound of the module text of locator_amd/spa.py,
(B + 8) 2^-24 sum_k (|c t| + |P m sp|) + 5 * 2^-24 sum_k P m sp, B = the largest number of sites one group sums: sample counts
around the tile, site counts around the block, node counts around the tile, every k_groups from 1 to one past the number of
site blocks, P = 1 and 2, pad garbage, NaN-filled scratch and ll; all-missing rows and unused sites are exact zeros, two
launches give the same bits, bad arguments launch nothing.

loc_spa_fit against spa.fit_host(float64): `used` and the unused zeros are exact; the parameter tolerance is 8 times the largest
|fit_state(float32) - fit_state(float64)| of the same fixture, a figure of the host definition alone, floored per site at half a
float32 spacing of the site's parameters (spa_util.fit_tolerance says why); sample counts around the kernel's chunk of 1,024 too.

The command's device path against its --host path on the planted clines and on the golden VCF.

Measured on one MI355X: see DESIGN.md section 8 (the spa command)."""
import json

import numpy as np
import pytest

from locator_amd import neighbors as NB
from locator_amd import spa as S
from tests import spa_util as U

pytestmark = pytest.mark.gpu
T, TQ, B = S.TILE, S.TILE_SAMPLES, S.BLOCK
FIT_CHUNK = S.FIT_CHUNK
QNAN = 0x7fc00000


def within(c, P, theta, used, gx, gy, k_groups, want=None, **kw):
    """One launch held to the bound; returns (ll, largest error / bound)."""
    K = c.shape[1]
    want = S.grid_host(c, P, theta, used, gx, gy) if want is None else want
    per = S.sites_per_group(K, k_groups) if k_groups else K
    bound = S.ll_bound(c, P, theta, used, gx, gy, per)
    got = S.grid_device(c, P, theta, used, gx, gy, k_groups=k_groups, **kw)
    assert got.dtype == np.float64 and got.shape == want.shape
    err = np.abs(got - want)
    assert (err <= bound).all(), (k_groups, np.argwhere(err > bound)[:5], err.max())
    assert not got[bound == 0].any()                                             # exact zeros, not small numbers
    live = bound > 0
    return got, float((err[live] / bound[live]).max()) if live.any() else 0.0


# ------------------------------------------------------------------ loc_spa_grid
@pytest.mark.parametrize("K", [1, B - 1, B, B + 1, 1000])
@pytest.mark.parametrize("Q", [1, T - 1, T, T + 1, TQ - 1, TQ, TQ + 1])
def test_grid_rows_and_sites_at_every_split(Q, K):
    G = 144
    nblocks = (K + B - 1) // B
    worst = 0.0
    for P in (1, 2):
        c, theta, used, gx, gy = U.grid_case(Q, K, G, 100 * Q + K + P, P=P)
        want = S.grid_host(c, P, theta, used, gx, gy)
        fills = np.random.default_rng(K)
        for k_groups in list(range(1, nblocks + 2)) + [0]:
            pad = fills if k_groups % 2 else 0x77
            got, ratio = within(c, P, theta, used, gx, gy, k_groups, want, fill=QNAN, pad_fill=pad,
                                pitch=(K + 15) // 16 * 16 + 16 * (k_groups % 3))
            worst = max(worst, ratio)
            assert Q < 3 or (not got[0].any() and not got[Q // 2].any())         # the all-missing rows
    print(f"loc_spa_grid Q={Q} K={K} G={G}: largest error / bound = {worst:.4g}")


@pytest.mark.parametrize("G", [1, 9, T - 1, T, 144])
def test_grid_node_counts_around_the_tile(G):
    Q, K = T + 1, B + 1
    for P in (1, 2):
        c, theta, used, gx, gy = U.grid_case(Q, K, G, 7 * G + P, P=P)
        for k_groups in (1, 2, 3, 0):
            got, ratio = within(c, P, theta, used, gx, gy, k_groups, fill=QNAN, pad_fill=0x77)
    print(f"loc_spa_grid Q={Q} K={K} G={G}: error / bound = {ratio:.4g}")


def test_grid_exact_zeros_and_the_same_bits():
    Q, K, G = T + 1, 3 * B + 5, 130
    c, theta, used, gx, gy = U.grid_case(Q, K, G, 5)
    first, _ = within(c, 2, theta, used, gx, gy, 2)
    assert np.isfinite(first).all() and first[1].any()
    assert np.array_equal(S.grid_device(c, 2, theta, used, gx, gy, k_groups=2), first)
    for pattern in (QNAN, 0xffffffff, 0x7f800001):                               # stale scratch and ll of every kind
        assert np.array_equal(S.grid_device(c, 2, theta, used, gx, gy, k_groups=2, fill=pattern,
                                            pad_fill=np.random.default_rng(pattern)), first)
    # every site unused: exact zeros whatever theta holds; no site at all: zeros too
    assert not S.grid_device(c, 2, theta, np.zeros(K, dtype=np.uint8), gx, gy, fill=QNAN).any()
    assert not S.grid_device(np.zeros((3, 0), dtype=np.int8), 2, np.zeros((0, 4)), np.zeros(0), gx, gy, fill=QNAN).any()
    # one lost site shows: the bound is far below a site's contribution
    lost = S.grid_host(c[:, 1:], 2, theta[1:], used[1:], gx, gy) if used[0] else S.grid_host(c[:, 2:], 2, theta[2:], used[2:], gx, gy)
    bound = S.ll_bound(c, 2, theta, used, gx, gy, S.sites_per_group(K, 2))
    live = bound > 0
    assert np.median(np.abs(lost - S.grid_host(c, 2, theta, used, gx, gy))[live] / bound[live]) > 100


def test_grid_bad_arguments_launch_nothing():
    import torch
    from locator_amd import _lib
    lib = _lib.load()
    Q, K, G = 5, 40, 9
    d_c = torch.zeros((Q, 48), dtype=torch.int8, device="cuda")
    d_t = torch.zeros((K + 1, 4), dtype=torch.float32, device="cuda")
    d_u = torch.ones(K, dtype=torch.uint8, device="cuda")
    d_g = torch.zeros(G + 1, dtype=torch.float32, device="cuda")
    d_ll = torch.full((Q, G), 77.0, dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    need = lib.loc_spa_grid_work_bytes(Q, K, G, 2)                               # two blocks, one tile
    assert need == 2 * TQ * T * 4 == lib.loc_spa_grid_work_bytes(Q, K, G, 5) and lib.loc_spa_grid_work_bytes(Q, K, G, 1) == TQ * T * 4
    assert 0 < lib.loc_spa_grid_work_bytes(Q, K, G, 0) <= need and lib.loc_spa_grid_work_bytes(Q, 0, G, 0) == 0
    assert lib.loc_spa_grid_work_bytes(TQ + 1, K, T + 1, 1) == 2 * 2 * TQ * T * 4
    for args in ((-1, K, G, 0), (Q, -1, G, 0), (Q, K, 0, 0), (Q, K, S.MAX_NODES + 1, 0), (Q, K, G, -1), (1 << 20, K, G, 0), (Q, 1 << 31, G, 0)):
        assert lib.loc_spa_grid_work_bytes(*args) == -1 and b"loc_spa_grid_work_bytes" in lib.loc_last_error(), args
    d_w = torch.full((need // 4 + 4,), 55.0, dtype=torch.float32, device="cuda")
    c, t, u, g, ll, w = d_c.data_ptr(), d_t.data_ptr(), d_u.data_ptr(), d_g.data_ptr(), d_ll.data_ptr(), d_w.data_ptr()
    good = (c, Q, K, 48, 2, t, u, g, g, G, 2, ll, w, need, s)

    def but(**kw):
        names = ("c", "Q", "K", "pitch", "P", "theta", "used", "gx", "gy", "G", "k_groups", "ll", "work", "work_bytes", "stream")
        return tuple(kw.get(n, v) for n, v in zip(names, good))

    bad = [but(c=None), but(theta=None), but(used=None), but(gx=None), but(gy=None), but(ll=None), but(work=None),
           but(pitch=32), but(pitch=40), but(c=c + 1), but(theta=t + 4), but(ll=ll + 4), but(work=w + 4), but(P=0), but(P=3),
           but(K=1 << 31, pitch=1 << 31), but(Q=1 << 20), but(Q=-1), but(K=-1), but(G=0), but(G=S.MAX_NODES + 1), but(k_groups=-1),
           but(work_bytes=need - 1), but(work_bytes=-1)]
    for args in bad:
        assert lib.loc_spa_grid(*args) == -1 and b"loc_spa_grid" in lib.loc_last_error(), args
    torch.cuda.synchronize()
    assert (d_ll == 77.0).all() and (d_w == 55.0).all()
    assert lib.loc_spa_grid(*good) == 0                                          # ... and the good call goes through
    torch.cuda.synchronize()
    assert torch.allclose(d_ll, torch.full_like(d_ll, -2.0 * K * float(np.log(2.0))), rtol=1e-6)     # c = 0, t = 0: -P log 2 a site
    assert lib.loc_spa_grid(*but(Q=0, ll=None, c=None)) == 0                     # zero rows: a valid launch of nothing


# ------------------------------------------------------------------ loc_spa_fit
def fit_case(N, K):
    """One (N, K) fixture in both ploidies under every mask, pad garbage and NaN coordinates outside w."""
    worst = host = 0.0
    for P in (1, 2):
        ct, xy = U.surface_counts(K, N, 1000 * N + K + P, P=P, missing=0.15)
        if K > 4:
            ct[1] = -1                                                           # an all-missing site, a monomorphic one
            ct[3] = np.where(ct[3] >= 0, P, -1)
        for j, w in enumerate(U.masks(N, N + K)):
            want, used, tol = U.fit_tolerance(ct, P, xy, w, 1.0, 12)
            bad_xy = np.where((w == 1)[:, None], xy, np.float32(np.nan))         # coordinates outside w are never interpreted
            pad = np.random.default_rng(j) if j % 2 else 0x77
            got, got_used = S.fit_device(ct, P, bad_xy, w, 1.0, 12, pad_fill=pad, pitch=(N + 15) // 16 * 16 + 16 * (j % 2))
            assert got.dtype == np.float32 and got.shape == (K, 4) and got_used.dtype == np.uint8
            assert np.array_equal(got_used, used) and not got[used == 0].any()
            on = used.astype(bool)
            if on.any():
                dist = np.abs(got[:, :3].astype(np.float64) - want[:, :3]).max(axis=1)
                assert (dist[on] <= tol[on]).all(), (P, j, dist[on].max(), tol[on].min())
                assert (got[on, 3] >= 0).all() and (got[on, 3] <= S.MAX_STEP).all()
                worst, host = max(worst, float(dist[on].max())), max(host, U.host_figure(tol, used))
            again, _ = S.fit_device(ct, P, xy, w, 1.0, 12)
            assert np.array_equal(again, got)                                    # the same bits, whatever pad and NaN hold
    print(f"loc_spa_fit N={N} K={K}: host float32 - float64 {host:.3g}, device - float64 {worst:.3g}")


@pytest.mark.parametrize("K", [1, 3, 4, 5, 300])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 1000])
def test_fit_against_the_float64_definition(N, K):
    fit_case(N, K)


@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("N", [FIT_CHUNK - 1, FIT_CHUNK, FIT_CHUNK + 1, 2 * FIT_CHUNK + 1])
def test_fit_across_sample_chunks(N, K):
    """The kernel walks the samples LOC_SPA_FIT_CHUNK at a time: a full chunk, one sample into the second, a partial third; the
    sums carried from chunk to chunk, the staging barrier and the column offset of a chunk are all in the parameters."""
    fit_case(N, K)
    # ... and the samples of the later chunks do enter: without them the fit is another one
    ct, xy = U.surface_counts(K, N, 5 * N + K, missing=0.1)
    head = np.arange(N) < FIT_CHUNK - 1
    full, _ = S.fit_device(ct, 2, xy, np.ones(N), 1.0, 12)
    cut, _ = S.fit_device(ct, 2, xy, head.astype(np.uint8), 1.0, 12)
    same, _ = S.fit_device(ct[:, head], 2, xy[head], np.ones(int(head.sum())), 1.0, 12)
    assert np.array_equal(cut, same) and (N < FIT_CHUNK or not np.array_equal(cut[:, :3], full[:, :3]))


def test_fit_zero_coordinates_other_settings_and_bad_arguments():
    import torch
    from locator_amd import _lib
    ct, xy = U.surface_counts(37, 200, 77)
    zero = np.zeros_like(xy)
    got, used = S.fit_device(ct, 2, zero, np.ones(200), 1.0, 12)
    want, _, tol = U.fit_tolerance(ct, 2, zero, np.ones(200), 1.0, 12)
    assert used.all() and not got[:, 0].any() and not got[:, 1].any()           # exactly 0
    assert (np.abs(got[:, 2].astype(np.float64) - want[:, 2]) <= tol).all()
    # a sample of w whose call is missing: its coordinates are not interpreted either (the definition zeroes them)
    gap = xy.copy()
    gap[5] = np.nan
    holes = ct.copy()
    holes[:, 5] = -1
    want, used, tol = U.fit_tolerance(holes, 2, gap, np.ones(200), 1.0, 12)
    got, got_used = S.fit_device(holes, 2, gap, np.ones(200), 1.0, 12)
    assert np.isfinite(want).all() and np.array_equal(got_used, used)
    assert (np.abs(got[:, :3].astype(np.float64) - want[:, :3]).max(axis=1) <= tol).all()
    for ridge, iters in ((0.25, 3), (4.0, 64), (0.0, 1)):
        want, used, tol = U.fit_tolerance(ct, 2, xy, np.ones(200), ridge, iters)
        got, got_used = S.fit_device(ct, 2, xy, np.ones(200), ridge, iters)
        assert np.array_equal(got_used, used) and (np.abs(got[:, :3].astype(np.float64) - want[:, :3]).max(axis=1) <= tol).all()
    # no sample at all: every site is unused; no site: nothing to write
    none, used = S.fit_device(np.zeros((5, 0), dtype=np.int8), 2, np.zeros((0, 2)), np.zeros(0), 1.0, 12)
    assert not none.any() and not used.any()
    lib = _lib.load()
    K, N = 6, 40
    d_ct = torch.zeros((K, 48), dtype=torch.int8, device="cuda")
    d_xy = torch.zeros((N + 1, 2), dtype=torch.float32, device="cuda")
    d_w = torch.ones(N, dtype=torch.uint8, device="cuda")
    d_th = torch.full((K + 1, 4), 77.0, dtype=torch.float32, device="cuda")
    d_us = torch.full((K,), 9, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    c, x, w, th, us = d_ct.data_ptr(), d_xy.data_ptr(), d_w.data_ptr(), d_th.data_ptr(), d_us.data_ptr()
    good = (c, K, N, 48, 2, x, w, 1.0, 12, th, us, s)

    def but(**kw):
        names = ("ct", "K", "N", "pitch", "P", "xy", "w", "ridge", "iters", "theta", "used", "stream")
        return tuple(kw.get(n, v) for n, v in zip(names, good))

    for args in (but(ct=None), but(xy=None), but(w=None), but(theta=None), but(used=None), but(pitch=32), but(pitch=40), but(ct=c + 1),
                 but(theta=th + 4), but(xy=x + 4), but(P=0), but(P=3), but(K=1 << 31), but(K=-1), but(N=1 << 20, pitch=1 << 20),
                 but(N=-1), but(iters=0), but(iters=65), but(ridge=-1.0), but(ridge=float("nan")), but(ridge=float("inf"))):
        assert lib.loc_spa_fit(*args) == -1 and b"loc_spa_fit" in lib.loc_last_error(), args
    torch.cuda.synchronize()
    assert (d_th == 77.0).all() and (d_us == 9).all()
    assert lib.loc_spa_fit(*but(K=0, ct=None, theta=None, used=None)) == 0      # no site: a valid launch of nothing
    assert lib.loc_spa_fit(*good) == 0
    torch.cuda.synchronize()
    assert not d_th[:K].any() and not d_us.any() and (d_th[K] == 77.0).all()     # every count 0: monomorphic, unused


# ------------------------------------------------------------------ the command
def run(tmp_path, name, vcf, sample_data, *extra):
    out = str(tmp_path / name)
    assert S.main(["--vcf", vcf, "--sample_data", sample_data, "--out", out, "--silence", "--keep_surfaces"] + list(extra)) == 0
    return out


def against_host(tmp_path, vcf, sd, c, P, locs, folds, grid, *extra):
    """The device run held to the host run of the same command line: theta within the fit's tolerance, ll within the bound
    (against the definition evaluated at the DEVICE's theta), placements and medians as the margin rule allows."""
    args = ("--folds", str(folds), "--grid", str(grid)) + extra
    dev, host = run(tmp_path, "dev", vcf, sd, *args), run(tmp_path, "host", vcf, sd, "--host", *args)
    zd, zh = np.load(dev + "_spa.npz"), np.load(host + "_spa.npz")
    sdev, shost = (json.load(open(o + "_spa_summary.json")) for o in (dev, host))
    N, K = c.shape
    located = ~np.isnan(locs).any(axis=1)
    xy, mean, sd_ = S.normalise(locs, located)
    xs, ys = zh["xs"], zh["ys"]
    gx, gy = S.flat_nodes(xs, ys)
    assert np.array_equal(zd["xs"], xs) and np.array_equal(zd["ys"], ys) and np.array_equal(zd["fold"], zh["fold"])
    assert np.array_equal(zd["sites"], zh["sites"]) and np.array_equal(zd["used"], zh["used"]) and sdev["K"] == K
    ct = np.ascontiguousarray(c.T)
    fold = zh["fold"]
    step = np.array([(float(xs[-1]) - float(xs[0])) / (grid - 1) * sd_[0], (float(ys[-1]) - float(ys[0])) / (grid - 1) * sd_[1]])
    placed_d = np.loadtxt(dev + "_spa_locs.txt", delimiter=",", skiprows=1, usecols=(0, 1))
    placed_h = np.loadtxt(host + "_spa_locs.txt", delimiter=",", skiprows=1, usecols=(0, 1))
    excluded, compared, worst_ll, worst_theta, worst_host, worst_place = 0, 0, 0.0, 0.0, 0.0, 0.0
    for i, f in enumerate(list(range(folds)) + [-1]):
        w = (located & (fold != f)).astype(np.uint8)
        want, used, tol = U.fit_tolerance(ct, P, xy, w, 1.0, 12)
        assert np.array_equal(want.astype(np.float32), zh["theta"][i]) and np.array_equal(used, zd["used"][i])
        on = used.astype(bool)
        dist = np.abs(zd["theta"][i][:, :3].astype(np.float64) - want[:, :3]).max(axis=1)
        assert (dist[on] <= tol[on]).all(), (f, dist[on].max(), tol[on].min())
        assert not zd["theta"][i][~on].any()
        worst_theta, worst_host = max(worst_theta, float(dist[on].max())), max(worst_host, U.host_figure(tol, used))
        rows = np.flatnonzero(fold == f)
        if not len(rows):
            continue
        name = "ll_all" if f < 0 else f"ll_fold{f}"
        ref = S.grid_host(c[rows], P, zd["theta"][i], used, gx, gy)
        bound = S.ll_bound(c[rows], P, zd["theta"][i], used, gx, gy, K)
        err = np.abs(zd[name] - ref)
        assert (err <= bound).all(), (f, err.max())
        worst_ll = max(worst_ll, float((err[bound > 0] / bound[bound > 0]).max()))
        # the margin rule, from the host surfaces alone
        llh = zh[name]
        node = np.argmax(llh, axis=1)
        clear = U.top_two_margin(llh) > 2 * S.ll_bound(c[rows], P, zh["theta"][i], used, gx, gy, K)[np.arange(len(rows)), node]
        excluded += int((~clear).sum())
        compared += int(clear.sum())
        diff = np.abs(placed_d[rows][clear] - placed_h[rows][clear]) / step[None]
        assert (diff <= 0.1).all(), (f, diff.max())
        worst_place = max(worst_place, float(diff.max()) if diff.size else 0.0)
    assert excluded <= 0.1 * N, (excluded, N)
    assert abs(sdev["median_error"] - shost["median_error"]) <= 0.01 * float(step.min())
    print(f"spa command N={N} K={K} grid={grid}: theta device - float64 {worst_theta:.3g} (host float32 - float64 {worst_host:.3g}), "
          f"ll error / bound {worst_ll:.4g}, {excluded} of {N} samples excluded by the margin rule, placements differ by at most "
          f"{worst_place:.3g} grid steps, medians {sdev['median_error']!r} (device) {shost['median_error']!r} (host)")
    return dev, sdev


def test_the_command_against_host_on_planted_clines(tmp_path):
    N, K = T + 2, 150
    c, locs = U.clines(N, K, 5)
    samples = [f"s{i}" for i in range(N)]
    vcf = U.write_vcf(str(tmp_path / "clines.vcf"), c, samples)
    sd = U.write_sample_data(str(tmp_path / "clines.txt"), samples, locs)
    dev, s = against_host(tmp_path, vcf, sd, c, 2, locs, 3, 16)
    assert s["K_used"] == K and s["r2_x"] > 0.9 and s["r2_y"] > 0.9 and s["n_unplaced"] == 0      # both planted axes are found
    again = run(tmp_path, "again", vcf, sd, "--folds", "3", "--grid", "16")
    for name in ("_spa_locs.txt", "_spa_sites.txt", "_spa_summary.json", "_spa.npz"):
        assert open(again + name, "rb").read() == open(dev + name, "rb").read(), name              # the same bits on every run


def test_the_command_against_host_on_the_golden_vcf(tmp_path):
    from locator_amd import baselines as BL
    from locator_amd import genotypes as G
    vcf = G.read_vcf(U.VCF)
    np.random.seed(1)
    _, idx = G.filter_snps(vcf["calldata/GT"], min_mac=2, max_snps=300, verbose=False, sites=True)
    c, P = BL.count_matrix(vcf["calldata/GT"], idx)
    locs = BL.read_locations(U.SAMPLE_DATA, vcf["samples"], S.PROG)
    _, s = against_host(tmp_path, U.VCF, U.SAMPLE_DATA, c, P, locs, 3, 8, "--max_SNPs", "300", "--seed", "1")
    assert (s["N"], s["n_located"], s["K"]) == (500, 450, 300)


def test_ld_prune_runs_on_the_sites_of_neighbors(tmp_path):
    out, nb = str(tmp_path / "spa"), str(tmp_path / "nb")
    common = ["--vcf", U.VCF, "--sample_data", U.SAMPLE_DATA, "--silence", "--ld_prune", "0.2"]
    assert S.main(common + ["--out", out, "--folds", "2", "--grid", "8", "--iters", "4"]) == 0
    assert NB.main(common + ["--out", nb, "--kmax", "4"]) == 0
    s, n = json.load(open(out + "_spa_summary.json")), json.load(open(nb + "_knn_summary.json"))
    keys = ("K", "ld_prune", "ld_window", "ld_window_bp", "K_before_prune")
    assert [s[k] for k in keys] == [n[k] for k in keys] == [1996, 0.2, 100, None, 5830]
    sites = [int(line.split("\t")[0]) for line in open(out + "_spa_sites.txt").read().splitlines()[1:]]
    assert len(sites) == 1996 and sites == sorted(sites)
