"""The plot command on the host (`python -m locator_amd.plot --host`): the panel-data functions against restatements of
their rules, the sample draw, exact sample IDs, the basemap store, the end-to-end run and the refusal without a GPU.
Nothing here needs a GPU; tests/test_gpu_plot.py runs the density grids on the device."""
import math
import os
import re

import numpy as np
import pandas as pd
import pytest

from locator_amd import _lib
from locator_amd import genotypes as G
from locator_amd import plot as P
from locator_amd import summarize as S


def _levels_restated(Z):
    """The contour-level rule written out with scipy's interp1d, as the reference script evaluates it."""
    from scipy.interpolate import interp1d
    zed = np.sort(np.ravel(Z))
    c = np.cumsum(zed)
    w = interp1d(c, zed)(zed)
    e = np.linspace(zed.min(), zed.max(), len(zed))
    out = []
    for t in np.quantile(w, [0.05, 0.5, 0.9]):
        i = int(np.abs(w - t).argmin())
        if e[i] not in out:
            out.append(e[i])
    return out


@pytest.mark.parametrize("kind", ["random", "peaked", "constant", "two_values"])
def test_contour_levels_follow_the_rule(kind):
    rng = np.random.default_rng(3)
    Z = {"random": rng.random((37, 53)),
         "peaked": np.exp(-np.add.outer(np.linspace(-3, 3, 40) ** 2, np.linspace(-4, 4, 61) ** 2)),
         "constant": np.full((10, 12), 0.25),
         "two_values": np.where(rng.random((20, 30)) < 0.7, 0.5, 2.0)}[kind]
    levels, labels = P.contour_levels(Z)
    assert levels == _levels_restated(Z)
    assert labels == ["0.95", "0.5", "0.1"][:len(levels)]
    assert levels == sorted(levels)
    if kind == "constant":
        assert levels == [0.25] and labels == ["0.95"]


def test_contour_levels_of_a_nan_grid_are_empty():
    assert P.contour_levels(np.full((4, 5), np.nan)) == ([], [])


def test_grid_count_rule_and_the_under_one_degree_floor():
    assert P.axis_count(0.0, 12.7) == 120
    assert P.axis_count(-3.2, 13.1) == 160           # int(16.3) * 10
    assert P.axis_count(5.0, 5.99) == 100            # spread under 1 degree: the reference would ask for 0 points
    assert P.axis_count(2.0, 2.0) == 100
    xg, yg = P.panel_grid([10.0, 22.5, 11.0], [40.0, 40.4, 40.2])
    assert len(xg) == 120 and len(yg) == 100
    assert xg[0] == 0.0 and xg[-1] == 32.5 and yg[0] == 30.0 and yg[-1] == pytest.approx(50.4, abs=1e-12)
    np.testing.assert_array_equal(xg, np.linspace(0.0, 32.5, 120))


def test_panel_limits_both_branches_and_the_equal_case():
    # x span 30 + 20 = 50 > y span 24: x kept, y centred, height = width / aspect
    lim = P.panel_limits([0.0, 30.0], [5.0, 9.0], 2.0)
    assert lim == pytest.approx((-10.0, 40.0, 7.0 - 12.5, 7.0 + 12.5))
    # y span 40 > x span 22: y kept, x centred, width = aspect * height
    lim = P.panel_limits([1.0, 3.0], [-10.0, 10.0], 0.5)
    assert lim == pytest.approx((2.0 - 10.0, 2.0 + 10.0, -20.0, 20.0))
    # equal padded spans take the x branch
    lim = P.panel_limits([0.0, 10.0], [100.0, 110.0], 2.0)
    assert lim == pytest.approx((-10.0, 20.0, 105.0 - 7.5, 105.0 + 7.5))
    rows, aspect = P.layout(7, 3, 10.0, 8.0)
    assert rows == 3 and aspect == pytest.approx((10 / 3) / (8 / 3))


def test_distance_km_is_great_circle_on_radians():
    # one degree of longitude on the equator = R * pi / 180
    assert P.distance_km(1.0, 0.0, 0.0, 0.0) == pytest.approx(6373.0 * math.pi / 180, rel=1e-12)
    # (0, 0) -> (90 E, 0): a quarter of the circle; (0, 0) -> (0, 90 N) likewise
    assert P.distance_km(90.0, 0.0, 0.0, 0.0) == pytest.approx(6373.0 * math.pi / 2, rel=1e-12)
    assert P.distance_km(0.0, 90.0, 0.0, 0.0) == pytest.approx(6373.0 * math.pi / 2, rel=1e-12)
    # a hand-worked pair at 60 N: hav = cos^2(60) sin^2(5 deg) -> d = 2 asin(0.5 sin 5 deg)
    want = 6373.0 * 2 * math.asin(0.5 * math.sin(math.radians(5.0)))
    assert P.distance_km(10.0, 60.0, 0.0, 60.0) == pytest.approx(want, rel=1e-12)
    got = P.distance_km(np.array([1.0, 10.0]), np.array([0.0, 60.0]), np.array([0.0, 0.0]), np.array([0.0, 60.0]))
    assert got == pytest.approx([6373.0 * math.pi / 180, want], rel=1e-12)


def test_sample_ids_match_exactly():
    aeg = pd.DataFrame({"sampleID": ["s1", "s10", "s1", "s11", "s10"], "xpred": [1.0, 2, 3, 4, 5],
                        "ypred": [0.0, 0, 0, 0, 0]})
    assert P.sample_rows(aeg, "s1")["xpred"].tolist() == [1.0, 3.0]
    assert P.sample_rows(aeg, "s10")["xpred"].tolist() == [2.0, 5.0]


def test_seed_makes_the_draw_reproducible_and_nsamples_is_capped():
    ids = [f"s{i}" for i in range(40)]
    a = P.pick_samples(ids, None, 9, seed=5)
    assert a == P.pick_samples(ids, None, 9, seed=5) and len(set(a)) == 9
    assert a != P.pick_samples(ids, None, 9, seed=6)
    assert sorted(P.pick_samples(ids[:4], None, 9, seed=1)) == sorted(ids[:4])
    assert P.pick_samples(ids, ["s3", "s1"], 9, seed=1) == ["s3", "s1"]


def test_host_density_equals_sklearn_haversine_kde():
    from sklearn.neighbors import KernelDensity
    rng = np.random.default_rng(11)
    pts = np.radians(np.column_stack([rng.normal(40, 3, 60), rng.normal(-100, 4, 60)]))
    lat_axis, lon_axis = np.radians(np.linspace(25, 55, 17)), np.radians(np.linspace(-120, -80, 23))
    Z = P.kde_grid_host(pts[:, 0], pts[:, 1], lat_axis, lon_axis, 0.04)
    Y, X = np.meshgrid(lat_axis, lon_axis, indexing="ij")
    kde = KernelDensity(bandwidth=0.04, metric="haversine", kernel="gaussian", algorithm="ball_tree").fit(pts)
    want = np.exp(kde.score_samples(np.column_stack([Y.ravel(), X.ravel()]))).reshape(Z.shape)
    assert np.all(np.abs(Z - want) <= 1e-9 * want + 1e-14 * want.max())
    assert np.isnan(P.kde_grid_host(np.array([0.1, np.nan]), np.array([0.2, 0.3]), lat_axis, lon_axis)).all()
    assert np.isnan(P.kde_grid_host(np.empty(0), np.empty(0), lat_axis, lon_axis)).all()


def test_zarr_group_lists_its_members(tmp_path):
    G.write_zarr_array(str(tmp_path / "m" / "B" / "B"), np.zeros((2, 3)), (2, 3), compressor="blosc")
    G.write_zarr_array(str(tmp_path / "m" / "A" / "A_1"), np.ones((2, 4)), (2, 4), compressor="blosc")
    G.write_zarr_array(str(tmp_path / "m" / "A" / "A_0"), np.ones((2, 2)), (2, 2), compressor="blosc")
    open(tmp_path / "m" / ".zgroup", "w").write('{"zarr_format": 2}')     # metadata files are not members
    g = G.ZarrGroup(str(tmp_path / "m"))
    assert list(g) == ["A", "B"]
    assert list(g["A"]) == ["A_0", "A_1"]
    shapes = P.read_basemap(str(tmp_path / "m"))
    assert [s[0].shape for s in shapes] == [(2,), (4,), (3,)]


def write_predlocs(d, n_files=20, n_samples=30, seed=0, spread=2.0):
    """n_files replicate predlocs files of n_samples samples around random true locations (degrees), and the sample file."""
    rng = np.random.default_rng(seed)
    ids = [f"s{i}" for i in range(n_samples)]
    truth = np.column_stack([rng.uniform(-20, 40, n_samples), rng.uniform(-30, 50, n_samples)])
    os.makedirs(d, exist_ok=True)
    for f in range(n_files):
        xy = truth + rng.normal(0, spread, truth.shape)
        pd.DataFrame({"x": xy[:, 0], "y": xy[:, 1], "sampleID": ids}).to_csv(os.path.join(d, f"boot{f}_predlocs.txt"),
                                                                              index=False)
    sd = pd.DataFrame({"sampleID": ids, "x": truth[:, 0], "y": truth[:, 1]})
    sd.loc[3, ["x", "y"]] = np.nan                       # one sample without a known location
    sd.to_csv(os.path.join(d, "samples.txt"), sep="\t", index=False)
    return ids, os.path.join(d, "samples.txt")


def write_map(path):
    square = np.array([[-10.0, 10.0, 10.0, -10.0, -10.0], [-10.0, -10.0, 10.0, 10.0, -10.0]])
    G.write_zarr_array(os.path.join(path, "Squareland", "Squareland"), square, (2, 5), compressor="blosc")
    G.write_zarr_array(os.path.join(path, "Farland", "Farland_0"), square + 500.0, (2, 5), compressor="blosc")


def test_end_to_end_on_the_host(tmp_path, capsys):
    ids, sd = write_predlocs(str(tmp_path / "pred"))
    write_map(str(tmp_path / "map.zarr"))
    out = str(tmp_path / "plot")
    panels, bp, pdf = P.run(P.build_parser().parse_args(
        ["--infile", str(tmp_path / "pred"), "--sample_data", sd, "--out", out, "--error", "--longlat",
         "--training_samples", sd, "--basemap", "--map", str(tmp_path / "map.zarr"), "--seed", "2", "--host"]))
    assert os.path.exists(out + ".pdf") and os.path.getsize(out + ".pdf") > 1000 and pdf == out + ".pdf"
    assert len(panels) == 9 and len({p["sample"] for p in panels}) == 9
    for p in panels:
        assert p["Z"].shape == (len(p["ygrid"]), len(p["xgrid"])) and np.isfinite(p["Z"]).all()
        assert 1 <= len(p["levels"]) <= 3
    want = S.summarize(str(tmp_path / "pred"), sd, str(tmp_path / "ref"), silence=True, host=True)
    got = pd.read_csv(out + "_centroids.txt", sep="\t")
    assert open(out + "_centroids.txt").read() == open(str(tmp_path / "ref") + "_centroids.txt").read()
    pd.testing.assert_frame_equal(got, pd.read_csv(str(tmp_path / "ref") + "_centroids.txt", sep="\t"))
    text = capsys.readouterr().out
    known = want.dropna(subset=["x", "y"])
    assert len(known) == 29
    kd = P.distance_km(known.kd_x, known.kd_y, known.x, known.y)
    m = re.search(r"^90% CI for kernel peak error = (\S+) (\S+)$", text, flags=re.M)
    assert m and float(m.group(1)) == np.quantile(kd, 0.05) and float(m.group(2)) == np.quantile(kd, 0.95)
    assert re.search(r"^90% CI for centroid error = \S+ \S+$", text, flags=re.M)
    assert re.search(r"^mean kernel peak error = ", text, flags=re.M)
    # the same seed draws the same panels
    panels2, _, _ = P.run(P.build_parser().parse_args(
        ["--infile", str(tmp_path / "pred"), "--out", str(tmp_path / "again"), "--seed", "2", "--host", "--silence"]))
    assert [p["sample"] for p in panels2] == [p["sample"] for p in panels]


def test_a_panel_without_a_density_is_drawn_without_contours(tmp_path, capsys):
    d = str(tmp_path / "pred")
    write_predlocs(d, n_files=3, n_samples=4)
    bad = pd.DataFrame({"x": [np.nan], "y": [1.0], "sampleID": ["s2"]})
    bad.to_csv(os.path.join(d, "zz_predlocs.txt"), index=False)
    panels, _, pdf = P.run(P.build_parser().parse_args(
        ["--infile", d, "--out", str(tmp_path / "p"), "--samples", "s1", "s2", "--ncol", "2", "--host"]))
    assert os.path.exists(pdf)
    assert panels[1]["levels"] == [] and np.isnan(panels[1]["Z"]).all()
    assert "s2: no density map" in capsys.readouterr().err


def test_without_a_gpu_the_command_stops_unless_host(tmp_path, monkeypatch):
    import torch
    write_predlocs(str(tmp_path / "pred"), n_files=2, n_samples=3)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match="no GPU visible.*--host"):
        P.main(["--infile", str(tmp_path / "pred"), "--out", str(tmp_path / "p")])
    assert not os.path.exists(str(tmp_path / "p") + ".pdf")


def test_header_declares_kde_grid_batch_as_the_bindings_do(repo_root):
    src = open(os.path.join(repo_root, "include", "locator_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"int\s+loc_kde_grid_batch\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m, "loc_kde_grid_batch is not declared"
    params = [p.strip() for p in m.group(1).split(",")]
    kinds = []
    for p in params:
        kinds.append("ptr" if "*" in p else "double" if p.startswith("double") else "int" if p.startswith("int ") else p)
    import ctypes as C
    res, args = _lib.SIGNATURES["loc_kde_grid_batch"]
    assert res is C.c_int
    want = {"ptr": C.c_void_p, "double": C.c_double, "int": C.c_int}
    assert [want[k] for k in kinds] == args
    assert kinds == ["ptr"] * 6 + ["int", "double", "ptr", "ptr", "ptr"]
