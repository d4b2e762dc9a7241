"""The localpca command without a GPU (locator_amd/localpca.py): the binding of include/locator_hip_localpca.h, the window
geometry, the distance, the MDS, the robust scores, the regions, and the --host command on a planted fixture: windows 4 .. 6 of
twelve follow y where the others follow x."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from locator_amd import localpca as L
from locator_amd import pca as P
from tests import localpca_util as LU
from tests import pca_util as U


def test_the_binding_comes_from_the_header():
    from tests.abi_util import check_extension
    i, i64, vp = C.c_int, C.c_int64, C.c_void_p
    check_extension("localpca", {"loc_grm_windows": (i, [vp, i, i64, i64, vp, vp, vp, i, vp, vp])}, {"LOC_LOCALPCA_MAX_WINDOWS": 65535})
    assert L.MAX_WINDOWS == 65535


# ------------------------------------------------------------------ windows
def test_site_windows_when_the_size_does_not_divide_the_chromosome():
    idx = np.arange(3, 26, 2)                                                            # 12 filtered sites of one chromosome
    pos = 100 + 10 * idx
    win, tab = L.window_bounds(np.full(12, "7"), pos, idx, snps=5)
    assert win.dtype == np.int64 and win.tolist() == [[0, 5], [5, 10], [10, 12]]
    assert tab["chrom"].tolist() == ["7"] * 3
    assert tab["start"].tolist() == [130, 230, 330] and tab["stop"].tolist() == [211, 311, 351]      # first .. last position + 1
    win, tab = L.window_bounds(None, None, idx, snps=5)                                  # a --matrix: variant indices
    assert win.tolist() == [[0, 5], [5, 10], [10, 12]] and tab["chrom"].tolist() == ["1"] * 3
    assert tab["start"].tolist() == [3, 13, 23] and tab["stop"].tolist() == [12, 22, 26]


def test_windows_never_span_two_chromosomes():
    chrom = np.array(["1"] * 7 + ["2"] * 4)
    pos = np.concatenate([np.arange(7) * 10, np.arange(4) * 10 + 5])
    win, tab = L.window_bounds(chrom, pos, np.arange(11), snps=3)
    assert win.tolist() == [[0, 3], [3, 6], [6, 7], [7, 10], [10, 11]]
    assert tab["chrom"].tolist() == ["1", "1", "1", "2", "2"]
    win, tab = L.window_bounds(chrom, pos, np.arange(11), bp=25)
    assert win.tolist() == [[0, 3], [3, 5], [5, 7], [7, 9], [9, 11]]                    # 0,10,20 | 30,40 | 50,60 || 5,15 | 25,35
    assert tab["start"].tolist() == [0, 25, 50, 0, 25] and tab["stop"].tolist() == [25, 50, 75, 25, 50]
    with pytest.raises(ValueError, match="not contiguous"):
        L.window_bounds(np.array(["1", "2", "1"]), np.arange(3), np.arange(3), snps=2)
    with pytest.raises(ValueError, match="ascending order"):
        L.window_bounds(np.array(["1", "1", "1"]), np.array([5, 4, 6]), np.arange(3), bp=2)


def test_bp_windows_with_an_empty_window_start_and_step():
    pos = np.array([100, 110, 120, 300, 310])
    chrom = np.full(5, "1")
    win, tab = L.window_bounds(chrom, pos, np.arange(5), bp=100)
    assert win.tolist() == [[0, 0], [0, 3], [3, 3], [3, 5]] and tab["start"].tolist() == [0, 100, 200, 300]   # 0-99 and 200-299 empty
    win, tab = L.window_bounds(chrom, pos, np.arange(5), bp=100, start=105)
    assert win.tolist() == [[1, 3], [3, 4], [4, 5]] and tab["start"].tolist() == [105, 205, 305] and tab["stop"][0] == 205
    win, tab = L.window_bounds(chrom, pos, np.arange(5), bp=100, start=100, step=50)     # sliding: overlapping windows
    assert win.tolist() == [[0, 3], [3, 3], [3, 3], [3, 5], [3, 5]] and tab["start"].tolist() == [100, 150, 200, 250, 300]
    win, _ = L.window_bounds(chrom, pos, np.arange(5), snps=2, start=1, step=1)
    assert win.tolist() == [[1, 3], [2, 4], [3, 5], [4, 5]]
    with pytest.raises(ValueError, match="no window"):
        L.window_bounds(chrom, pos, np.arange(5), bp=100, start=311)


def test_a_matrix_refuses_bp_windows(tmp_path, capsys):
    with pytest.raises(ValueError, match="--window_bp needs positions"):
        L.window_bounds(None, None, np.arange(5), bp=100)
    with pytest.raises(ValueError, match="exactly one of"):
        L.window_bounds(None, None, np.arange(5))
    with pytest.raises(ValueError, match="exactly one of"):
        L.window_bounds(None, None, np.arange(5), snps=2, bp=2)
    with pytest.raises(ValueError, match=">= 1"):
        L.window_bounds(None, None, np.arange(5), snps=0)
    with pytest.raises(ValueError, match="ascending variant order"):
        L.window_bounds(None, None, np.array([0, 2, 1]), snps=2)
    for extra, text in ((["--matrix", "m.txt", "--window_bp", "100"], "--window_bp needs positions"),
                        (["--vcf", U.VCF], "exactly one of --window_snps / --window_bp"),
                        (["--vcf", U.VCF, "--window_snps", "5", "--window_bp", "9"], "exactly one of --window_snps / --window_bp"),
                        (["--vcf", U.VCF, "--window_snps", "5", "--npc", "11"], "--npc must be")):
        with pytest.raises(SystemExit) as e:
            L.main(extra + ["--out", str(tmp_path / "o"), "--host"])
        assert e.value.code == 2 and text in capsys.readouterr().err
    assert not os.listdir(tmp_path)


def test_check_windows_refusals():
    assert L.check_windows([(0, 0), (2, 5), (5, 5), (0, 5), (2, 5)], 5).tolist() == [[0, 0], [2, 5], [5, 5], [0, 5], [2, 5]]
    assert L.check_windows(np.array([[1.0, 3.0]]), 5).dtype == np.int64
    for bad in ([(0, 6)], [(-1, 2)], [(3, 2)], [(0, 2), (6, 6)]):
        with pytest.raises(ValueError, match="needs 0 <= v0 <= v1 <= K = 5"):
            L.check_windows(bad, 5)
    for bad in ([], [0, 2], [(0, 1, 2)], np.zeros((0, 2), dtype=np.int64)):
        with pytest.raises(ValueError, match=r"needs \[W\]\[2\]"):
            L.check_windows(bad, 5)
    for bad in ([(0.5, 2)], [(0, np.nan)], [("a", "b")]):
        with pytest.raises(ValueError, match="whole numbers"):
            L.check_windows(bad, 5)


def test_windows_host_is_the_sum_over_the_windows_own_sites():
    c = U.spread_counts(9, 40, 1)
    mean, scale, _ = P.site_constants(c, 2)
    win = [(0, 40), (3, 17), (17, 40), (5, 5), (0, 3)]
    G = L.windows_host(c, mean, scale, win)
    assert G.shape == (5, 9, 9) and not G[3].any()
    assert np.array_equal(G[0], P.grm_host(c, mean, scale)) and np.array_equal(G[1], P.grm_host(c[:, 3:17], mean[3:17], scale[3:17]))
    assert np.allclose(G[4] + G[1] + G[2], G[0], rtol=0, atol=1e-10)
    scale[[4, 20]] = 0
    assert L.used_sites(scale, L.check_windows(win, 40)).tolist() == [int((scale[a:b] > 0).sum()) for a, b in win]
    assert L.used_sites(np.ones(40), L.check_windows(win, 40)).tolist() == [40, 14, 23, 0, 3]


# ------------------------------------------------------------------ the distance
def _random_windows(W, N, npc, seed):
    rng = np.random.default_rng(seed)
    U_ = np.stack([np.linalg.qr(rng.normal(size=(N, npc)))[0] for _ in range(W)])
    lam = np.sort(rng.uniform(0.5, 4.0, (W, npc)), axis=1)[:, ::-1]
    return lam, U_


def test_pc_dist_is_the_frobenius_distance_of_the_weighted_projectors():
    lam, U_ = _random_windows(7, 23, 3, 4)
    lam[2, 2] = -0.3                                                                     # a negative eigenvalue counts as 0
    D = L.pc_dist(lam, U_)
    assert D.shape == (7, 7) and not np.diag(D).any() and np.array_equal(D, D.T) and (D[~np.eye(7, dtype=bool)] > 0).all()
    a = np.maximum(lam, 0)
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    M = np.einsum("wp,wip,wjp->wij", a, U_, U_)
    want = np.array([[np.linalg.norm(M[v] - M[w]) for w in range(7)] for v in range(7)])
    assert np.abs(D - want).max() <= 1e-12
    signs = np.random.default_rng(5).choice([-1.0, 1.0], (7, 1, 3))
    assert np.abs(L.pc_dist(lam, U_ * signs) - D).max() <= 1e-14                         # signs do not matter
    assert np.abs(L.pc_dist(3.0 * lam, U_) - D).max() <= 1e-14                           # ... nor the scale of the eigenvalues
    assert np.abs(L.pc_dist(lam[[0, 0, 3]], U_[[0, 0, 3]])[0, 1]) < 1e-7                 # a repeated window: the root of rounding


def test_pc_dist_of_orthogonal_subspaces_is_root_two():
    Q = np.linalg.qr(np.random.default_rng(6).normal(size=(12, 6)))[0]
    lam = np.array([[3.0, 1.0, 0.5], [2.0, 2.0, 0.1]])
    D = L.pc_dist(lam, np.stack([Q[:, :3], Q[:, 3:]]))
    assert abs(D[0, 1] - np.sqrt(2.0)) <= 1e-14 and D[0, 0] == 0
    assert abs(L.pc_dist(lam[:, :1], np.stack([Q[:, :1], Q[:, 1:2]]))[0, 1] - np.sqrt(2.0)) <= 1e-14


def test_mds_recovers_a_planar_configuration():
    pts = np.random.default_rng(7).normal(size=(15, 2)) * np.array([[3.0, 1.0]])
    D = np.sqrt(((pts[:, None] - pts[None]) ** 2).sum(axis=-1))
    Y, lam = L.mds(D, 2)
    assert Y.shape == (15, 2) and lam[0] > lam[1] > 0
    assert np.abs(np.sqrt(((Y[:, None] - Y[None]) ** 2).sum(axis=-1)) - D).max() <= 1e-10
    assert np.abs(Y.mean(axis=0)).max() <= 1e-12
    big = np.argmax(np.abs(Y), axis=0)
    assert (Y[big, [0, 1]] > 0).all()                                                    # the sign rule of pca.components
    Y3, lam3 = L.mds(D, 3)
    assert abs(lam3[2]) <= 1e-10 * lam3[0] and np.abs(Y3[:, 2]).max() <= 1e-4            # a plane has no third axis
    with pytest.raises(ValueError, match="windows - 1"):
        L.mds(D[:2, :2], 2)


def test_robust_scores_and_an_axis_without_spread():
    Y = np.array([[0.0, 1.0], [1.0, 1.0], [2.0, 1.0], [3.0, 1.0], [100.0, 5.0]])
    s, med, mad = L.robust_scores(Y)
    assert med.tolist() == [2.0, 1.0] and mad.tolist() == [1.0, 0.0]
    assert np.allclose(s[:, 0], (Y[:, 0] - 2.0) / 1.4826) and not s[:, 1].any()          # MAD 0: nothing scores, nothing is flagged


def test_regions_merge_within_a_chromosome_only():
    chrom = np.array(["1", "1", "1", "1", "2", "2", "2", "2"])
    assert L.merge_regions(chrom, [0, 1, 1, 1, 1, 1, 0, 1]) == [(1, 3), (4, 5), (7, 7)]
    assert L.merge_regions(chrom, [0] * 8) == [] and L.merge_regions(chrom, [1] * 8) == [(0, 3), (4, 7)]
    assert L.merge_regions(chrom, [1, 0, 1, 0, 0, 0, 0, 0]) == [(0, 0), (2, 2)]


# ------------------------------------------------------------------ the command
@pytest.fixture(scope="module")
def planted_files(tmp_path_factory):
    return LU.write_planted(tmp_path_factory.mktemp("planted"))


def run(tmp_path, name, vcf, *extra):
    out = str(tmp_path / name)
    assert L.main(["--vcf", vcf, "--out", out, "--silence", "--host"] + list(extra)) == 0
    return out


def test_the_planted_fixture_meets_its_conditions(planted_files):
    """What the host definition alone must give, so that the command tests (here and on the device) say something."""
    _, _, c, _, win = planted_files
    mean, scale, K_used = P.site_constants(c, 2)
    used = L.used_sites(scale, win)
    assert K_used == c.shape[1] and (used == 96).all()
    G = L.windows_host(c, mean, scale, win)
    parts = [P.components(G[w], 96, 2) for w in range(12)]
    D = L.pc_dist(np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts]))
    pl = np.isin(np.arange(12), LU.PLANTED)
    within, between = max(D[np.ix_(pl, pl)].max(), D[np.ix_(~pl, ~pl)].max()), D[np.ix_(pl, ~pl)].min()
    s = L.robust_scores(L.mds(D, 2)[0])[0]
    print(f"planted fixture: within {within:.4g}, between {between:.4g}, axis-1 scores plain <= {np.abs(s[~pl, 0]).max():.4g}, "
          f"planted >= {np.abs(s[pl, 0]).min():.4g}")
    assert within < between / 2
    assert (np.abs(s[~pl, 0]) < 2).all() and (np.abs(s[pl, 0]) > 6).all()


def test_the_host_command_finds_the_planted_windows(planted_files, tmp_path):
    vcf, sd, c, locs, win = planted_files
    out = run(tmp_path, "a", vcf, "--sample_data", sd, "--window_snps", "96", "--keep_matrix", "--keep_components")
    s = json.load(open(out + "_localpca_summary.json"))
    assert list(s) == list(L.SUMMARY_KEYS)
    assert (s["N"], s["n_located"], s["K"], s["K_used"], s["W"], s["W_kept"], s["W_skipped"]) == (130, 130, 1152, 1152, 12, 12, 0)
    assert (s["window_unit"], s["window_size"], s["window_start"], s["window_step"]) == ("sites", 96, 0, 96)
    assert s["flagged"] == [4, 5, 6] and s["n_flagged"] == 3 and s["n_regions"] == 1 and s["mad_zero_axes"] == []
    assert s["mds_eigenvalues"][0] > s["mds_eigenvalues"][1] > 0
    head, t = LU.read_windows(out)
    assert head[:9] == ["window", "chrom", "start", "stop", "first_site", "last_site", "n_sites", "K_used", "kept"]
    assert head[9:] == ["eigenvalue1", "eigenvalue2", "share1", "share2", "mds1", "mds2", "score1", "score2", "flag",
                        "pc1_r2_x", "pc1_r2_y", "pc2_r2_x", "pc2_r2_y"]
    assert [int(v) for v in t["flag"]] == [0, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0] and t["chrom"] == ["1"] * 12
    assert [int(v) for v in t["first_site"]] == win[:, 0].tolist() and [int(v) for v in t["last_site"]] == (win[:, 1] - 1).tolist()
    assert [int(v) for v in t["start"]] == (100 + 10 * win[:, 0]).tolist()               # pca_util.write_vcf: POS = 100 + 10 k
    assert [int(v) for v in t["stop"]] == (100 + 10 * (win[:, 1] - 1) + 1).tolist()
    r2x, r2y = np.array([float(v) for v in t["pc1_r2_x"]]), np.array([float(v) for v in t["pc1_r2_y"]])
    pl = np.isin(np.arange(12), LU.PLANTED)
    assert (r2x[~pl] > r2y[~pl]).all() and (r2y[pl] > r2x[pl]).all() and r2x[~pl].min() > 0.5 and r2y[pl].min() > 0.5
    rhead, rrows = U.read_table(out + "_localpca_regions.txt")
    assert rhead == ["region", "chrom", "start", "stop", "first_window", "last_window", "n_windows", "first_site", "last_site",
                     "peak_score"]
    assert len(rrows) == 1 and rrows[0][:9] == ["0", "1", str(100 + 10 * 384), str(100 + 10 * 671 + 1), "4", "6", "3", "384", "671"]
    assert float(rrows[0][9]) > 6
    # the kept arrays are the definitions
    mean, scale, _ = P.site_constants(c, 2)
    G = L.windows_host(c, mean, scale, win)
    z, comp = np.load(out + "_localpca_dist.npz"), np.load(out + "_localpca_components.npz")
    for w in (0, 5, 11):
        lam, U_, _ = P.components(G[w], 96, 2)
        assert np.array_equal(comp["eigenvalues"][w], lam) and np.array_equal(comp["U"][w], U_)
    assert np.array_equal(z["D"], L.pc_dist(comp["eigenvalues"], comp["U"])) and np.array_equal(z["windows"], np.arange(12))
    assert np.array_equal(z["win"], win) and np.array_equal(comp["K_used"], np.full(12, 96))
    assert np.array_equal(np.array([[float(a), float(b)] for a, b in zip(t["mds1"], t["mds2"])]), z["mds"])
    # two runs write the same bytes
    again = run(tmp_path, "b", vcf, "--sample_data", sd, "--window_snps", "96", "--keep_matrix", "--keep_components")
    for name in ("_localpca_windows.txt", "_localpca_regions.txt", "_localpca_summary.json", "_localpca_dist.npz",
                 "_localpca_components.npz"):
        assert open(again + name, "rb").read() == open(out + name, "rb").read(), name
    assert not [f for f in os.listdir(tmp_path) if ".tmp" in f]
    # without locations: the same windows, no r2 columns
    bare = run(tmp_path, "c", vcf, "--window_snps", "96")
    head2, t2 = LU.read_windows(bare)
    assert head2 == head[:-4] and t2["flag"] == t["flag"] and t2["mds1"] == t["mds1"]
    assert json.load(open(bare + "_localpca_summary.json"))["n_located"] is None


def test_skipped_windows_are_listed_and_excluded(planted_files, tmp_path):
    vcf, _, c, _, _ = planted_files
    # positions 100, 110 .. 11610: bp windows of 960 bp hold 96 sites; from --window_start 40 the first one holds 90 and the
    # thirteenth 6, below --min_sites 10
    out = run(tmp_path, "a", vcf, "--window_bp", "960", "--window_start", "40", "--keep_matrix")
    s = json.load(open(out + "_localpca_summary.json"))
    _, t = LU.read_windows(out)
    n = [int(v) for v in t["n_sites"]]
    assert s["W"] == 13 and n == [90] + [96] * 11 + [6] and (s["window_unit"], s["window_start"]) == ("bp", 40)
    assert s["W_skipped"] == 1 and [int(v) for v in t["kept"]] == [1] * 12 + [0]
    assert t["flag"][12] == "0" and t["mds1"][12] == "nan" and t["eigenvalue1"][12] == "nan" and t["score2"][12] == "nan"
    assert int(t["start"][0]) == 40 and int(t["stop"][0]) == 1000 and int(t["first_site"][12]) == 1146
    z = np.load(out + "_localpca_dist.npz")
    assert z["D"].shape == (12, 12) and z["windows"].tolist() == list(range(12)) and len(z["win"]) == 13
    assert np.isfinite([float(v) for v in t["mds1"][:12]]).all()
    # an empty window is listed with no site
    out = run(tmp_path, "b", vcf, "--window_bp", "90", "--window_step", "1000", "--min_sites", "5")
    _, t = LU.read_windows(out)
    assert [int(v) for v in t["n_sites"]] == [0] + [9] * 11 and t["kept"] == ["0"] + ["1"] * 11      # 0 .. 89 holds no site
    assert (t["first_site"][0], t["last_site"][0], t["start"][0], t["stop"][0]) == ("-1", "-1", "0", "90")
    assert (t["first_site"][1], t["last_site"][1]) == ("90", "98")
    with pytest.raises(SystemExit, match="at least 3 are needed"):
        run(tmp_path, "c", vcf, "--window_snps", "600")
    with pytest.raises(SystemExit, match="--mds 5 with 4 kept windows"):
        run(tmp_path, "d", vcf, "--window_snps", "300", "--mds", "5")


def test_without_a_gpu_the_command_stops_unless_host(planted_files, tmp_path, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    vcf, _, c, _, win = planted_files
    out = tmp_path / "none"
    os.makedirs(str(out))
    with pytest.raises(SystemExit, match="no GPU visible.*loc_grm_windows.*--host"):
        L.main(["--vcf", vcf, "--out", str(out / "o"), "--window_snps", "96"])
    table = {"chrom": np.full(12, "1"), "start": win[:, 0], "stop": win[:, 1]}
    with pytest.raises(SystemExit, match="no GPU visible.*loc_grm_windows.*--host"):
        L.localpca(c, 2, [f"s{i}" for i in range(len(c))], None, win, table, str(out / "o"))
    assert not os.listdir(str(out))
