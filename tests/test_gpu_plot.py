"""Density grids of the plot command on the device: loc_kde_grid_batch through the C ABI against sklearn's haversine
KernelDensity and a NumPy float64 evaluation, one launch of ~300 mixed panels, bad arguments, and the command end to
end against its --host run."""
import os

import numpy as np
import pytest

from tests.test_plot import write_predlocs

pytestmark = pytest.mark.gpu


def _pairs_numpy(lat, lon, glat, glon, h):
    """Densities at the grid points (glat[k], glon[k]) written out with NumPy, float64, radians."""
    hav = np.sin((glat[:, None] - lat[None, :]) / 2) ** 2 + \
        np.cos(glat[:, None]) * np.cos(lat[None, :]) * np.sin((glon[:, None] - lon[None, :]) / 2) ** 2
    d = 2 * np.arcsin(np.sqrt(hav))
    return np.exp(-d * d / (2 * h * h)).sum(axis=1) / (len(lat) * 2 * np.pi * h * h)


def _panel(rng, n, spread_deg=(6.0, 8.0), grid=None):
    c = rng.uniform([-50, -150], [60, 150])
    pts = np.radians(c + rng.normal(0, 1, (n, 2)) * np.asarray(spread_deg) / 2)
    if grid is None:
        lo, hi = np.degrees(pts.min(0)) - 10, np.degrees(pts.max(0)) + 10
        grid = (int(hi[0] - lo[0]) * 10 or 100, int(hi[1] - lo[1]) * 10 or 100)
    lat_axis = np.radians(np.linspace(np.degrees(pts[:, 0].min()) - 10, np.degrees(pts[:, 0].max()) + 10, grid[0]))
    lon_axis = np.radians(np.linspace(np.degrees(pts[:, 1].min()) - 10, np.degrees(pts[:, 1].max()) + 10, grid[1]))
    return pts[:, 0].copy(), pts[:, 1].copy(), lat_axis, lon_axis


def test_three_panels_equal_sklearn_haversine_kde():
    from sklearn.neighbors import KernelDensity
    from locator_amd import plot as P
    rng = np.random.default_rng(1)
    panels = [_panel(rng, 257, (12, 16)), _panel(rng, 40, (3, 2)), _panel(rng, 120, (0.5, 0.7))]
    zs = P.kde_grids_device(panels, 0.04)
    for (lat, lon, ya, xa), z in zip(panels, zs):
        Y, X = np.meshgrid(ya, xa, indexing="ij")
        kde = KernelDensity(bandwidth=0.04, metric="haversine", kernel="gaussian", algorithm="ball_tree")
        kde.fit(np.column_stack([lat, lon]))
        want = np.exp(kde.score_samples(np.column_stack([Y.ravel(), X.ravel()]))).reshape(z.shape)
        assert z.shape == (len(ya), len(xa))
        assert np.all(np.abs(z - want) <= 1e-9 * want + 1e-14 * want.max()), np.abs(z - want).max()


def test_one_launch_of_mixed_panels_matches_numpy_and_is_bit_stable():
    """~300 panels of 257 replicates with grids of every size, plus a 1-point panel, a 5000-point panel (five LDS stages)
    and a panel with a NaN prediction: a random sample of grid points per panel against NumPy, NaN panels all NaN, and a
    second launch bit-identical."""
    from locator_amd import plot as P
    rng = np.random.default_rng(2)
    panels = []
    for s in range(300):
        if s == 17:
            panels.append(_panel(rng, 1, grid=(100, 100)))
        elif s == 150:
            panels.append(_panel(rng, 5000, (10, 10), grid=(90, 110)))
        elif s == 201:
            p = list(_panel(rng, 257, grid=(40, 30)))
            p[1][100] = np.nan
            panels.append(tuple(p))
        else:
            panels.append(_panel(rng, 257, (rng.uniform(0.3, 14), rng.uniform(0.3, 14)),
                                 grid=(int(rng.integers(3, 240)), int(rng.integers(3, 240)))))
    zs = P.kde_grids_device(panels, 0.04)
    for s, ((lat, lon, ya, xa), z) in enumerate(zip(panels, zs)):
        assert z.shape == (len(ya), len(xa))
        if s == 201:
            assert np.isnan(z).all()
            continue
        k = rng.choice(z.size, min(z.size, 64), replace=False)
        iy, ix = np.divmod(k, len(xa))
        want = _pairs_numpy(lat, lon, ya[iy], xa[ix], 0.04)
        got = z[iy, ix]
        assert np.all(np.abs(got - want) <= 1e-9 * want + 1e-14 * want.max()), (s, np.abs(got - want).max())
        assert np.isfinite(z).all()
    zs2 = P.kde_grids_device(panels, 0.04)
    for a, b in zip(zs, zs2):
        np.testing.assert_array_equal(a.view(np.uint64), b.view(np.uint64))
    # a panel's values do not depend on the other panels of the launch
    alone = P.kde_grids_device(panels[150:152], 0.04)
    np.testing.assert_array_equal(alone[0], zs[150])
    np.testing.assert_array_equal(alone[1], zs[151])


def test_bad_arguments_return_nonzero_with_a_message():
    import torch
    from locator_amd import _lib
    lib = _lib.load()
    dev = "cuda:0"
    pts = torch.zeros((4, 2), dtype=torch.float64, device=dev)
    ax = torch.zeros(6, dtype=torch.float64, device=dev)
    z = torch.full((6,), -1.0, dtype=torch.float64, device=dev)
    off = lambda *v: torch.tensor(v, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def call(pt_off, lat_off, lon_off, z_off, h=0.04, n=1):
        rc = lib.loc_kde_grid_batch(pts.data_ptr(), pt_off.data_ptr(), ax.data_ptr(), lat_off.data_ptr(), ax.data_ptr(),
                                    lon_off.data_ptr(), n, h, z.data_ptr(), z_off.data_ptr(), stream)
        return rc, lib.loc_last_error().decode()

    assert call(off(0, 4), off(0, 2), off(0, 3), off(0, 6))[0] == 0
    torch.cuda.synchronize()
    assert torch.isfinite(z).all()
    z.fill_(-1.0)
    for args, kw in [((off(0, 4), off(0, 2), off(0, 3), off(0, 5)), {}),          # z holds 5 values, grid is 2 x 3
                     ((off(3, 1), off(0, 2), off(0, 3), off(0, 6)), {}),          # points offsets decrease
                     ((off(0, 4), off(0, 2), off(0, 3), off(0, 6)), {"h": 0.0}),
                     ((off(0, 4), off(0, 2), off(0, 3), off(0, 6)), {"h": -1.0}),
                     ((off(0, 4), off(0, 2), off(0, 3), off(0, 6)), {"n": -1})]:
        rc, msg = call(*args, **kw)
        assert rc != 0 and "loc_kde_grid_batch" in msg, (kw, msg)
    torch.cuda.synchronize()
    assert (z == -1.0).all()                                                       # nothing was launched
    rc = lib.loc_kde_grid_batch(None, None, None, None, None, None, 1, 0.04, None, None, stream)
    assert rc != 0 and "null" in lib.loc_last_error().decode()


def test_command_on_the_device_matches_the_host_run(tmp_path):
    from locator_amd import plot as P
    _, sd = write_predlocs(str(tmp_path / "pred"), n_files=20, n_samples=30, spread=3.0)
    common = ["--infile", str(tmp_path / "pred"), "--sample_data", sd, "--error", "--longlat", "--seed", "4",
              "--training_samples", sd, "--silence"]
    dev, bp_dev, pdf = P.run(P.build_parser().parse_args(common + ["--out", str(tmp_path / "dev")]))
    host, bp_host, _ = P.run(P.build_parser().parse_args(common + ["--out", str(tmp_path / "host"), "--host"]))
    assert os.path.exists(pdf) and os.path.getsize(pdf) > 1000
    assert [p["sample"] for p in dev] == [p["sample"] for p in host]
    for d, h in zip(dev, host):
        np.testing.assert_array_equal(d["xgrid"], h["xgrid"])
        zd, zh = d["Z"], h["Z"]
        assert np.all(np.abs(zd - zh) <= 1e-9 * zh + 1e-14 * zh.max())
        assert d["limits"] == h["limits"]
        # levels: equal, or the adjacent evenly spaced value where the mapped values nearly tie
        zed = np.sort(zh.ravel())
        even = np.linspace(zed[0], zed[-1], len(zed))
        step = even[1] - even[0] if len(even) > 1 else 0.0
        assert len(d["levels"]) == len(h["levels"]) and d["labels"] == h["labels"]
        for a, b in zip(d["levels"], h["levels"]):
            assert a == b or abs(a - b) <= step * (1 + 1e-9), (d["sample"], a, b)
    # the summaries come from loc_kde_peak_batch on the device and the NumPy form on the host
    assert list(bp_dev.sampleID) == list(bp_host.sampleID)
    np.testing.assert_allclose(bp_dev[["kd_x", "kd_y", "gc_x", "gc_y"]].to_numpy(),
                               bp_host[["kd_x", "kd_y", "gc_x", "gc_y"]].to_numpy(), rtol=1e-12, atol=1e-12)
