"""The pca command without a GPU (locator_amd/pca.py): the site constants and the relationship matrix on hand-computed cases,
the components of a constructed matrix, the hat-matrix placement against a real refit, the choice of p, the binding of
include/locator_hip_pca.h, the --host command on the golden VCF, and the refusals."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from locator_amd import baselines as BL
from locator_amd import pca as P
from tests import pca_util as U


# ------------------------------------------------------------------ constants and G
def test_site_constants_by_hand():
    #            site 0      1     2     3     4
    c = np.array([[0,       -1,    2,    1,    0],
                  [1,       -1,    2,   -1,    0],
                  [2,       -1,    2,    1,    0],
                  [-1,      -1,   -1,    2,    0]], dtype=np.int8)
    mean, scale, K_used = P.site_constants(c, 2)
    assert mean.dtype == scale.dtype == np.float32 and K_used == 2
    # site 0: 3 calls, sum 3: p = 1/2, mean 1, scale 1 / sqrt(2 * 1/4); site 3: 3 calls, sum 4: p = 2/3, mean 4/3
    assert mean.tolist() == [1.0, 0.0, 0.0, float(np.float32(4 / 3)), 0.0]
    assert scale.tolist() == [float(np.float32(2 ** 0.5)), 0.0, 0.0, float(np.float32(1.5)), 0.0]   # 1 / sqrt(2 * 2/3 * 1/3)
    # haploid: the same counts of copies among half the alleles
    h = np.array([[0, 1, 1], [1, 1, -1], [1, 1, 0], [1, 1, -1]], dtype=np.int8)
    mean, scale, K_used = P.site_constants(h, 1)
    assert K_used == 2 and mean.tolist() == [0.75, 0.0, 0.5] and scale[1] == 0
    assert scale.tolist() == [float(np.float32(1 / np.sqrt(0.75 * 0.25))), 0.0, 2.0]
    with pytest.raises(ValueError, match="exceeds the ploidy 1"):
        P.site_constants(np.array([[0, 2]], dtype=np.int8), 1)


def test_grm_host_against_three_loops():
    c = U.spread_counts(7, 23, 3, missing=0.2)
    c[2] = -1
    mean, scale, _ = P.site_constants(c, 2)
    G = P.grm_host(c, mean, scale)
    want = np.zeros((7, 7))
    for i in range(7):
        for j in range(7):
            for k in range(23):
                if c[i, k] >= 0 and c[j, k] >= 0:
                    want[i, j] += (float(c[i, k]) - float(mean[k])) * float(scale[k]) * ((float(c[j, k]) - float(mean[k])) * float(scale[k]))
    assert G.dtype == np.float64 and np.allclose(G, want, rtol=1e-13, atol=1e-13) and not G[2].any()
    assert np.array_equal(G, G.T)


# ------------------------------------------------------------------ components
def test_components_of_a_rank_2_matrix():
    a = np.array([1.0, 1.0, 1.0, 1.0, -4.0]) / np.sqrt(20.0)
    b = np.array([1.0, -3.0, 1.0, 1.0, 0.0]) / np.sqrt(12.0)               # orthogonal to a
    K_used = 10
    G = K_used * (6.0 * np.outer(a, a) + 2.0 * np.outer(b, b))
    lam, V, share = P.components(G, K_used, 3)
    assert np.allclose(lam, [6.0, 2.0, 0.0], atol=1e-12) and np.allclose(share, [0.75, 0.25, 0.0], atol=1e-12)
    assert np.allclose(V[:, 0], -a, atol=1e-12) and np.allclose(V[:, 1], -b, atol=1e-12)   # largest components (-4, -3) made positive
    pcs = P.scores(lam, V)
    assert np.allclose(pcs[:, 0], -a * np.sqrt(6.0)) and np.allclose(pcs[:, :2] @ pcs[:, :2].T, G / K_used, atol=1e-12)
    # a tie of the largest magnitude goes to the lowest index
    t = np.array([1.0, -1.0, 0.0]) / np.sqrt(2.0)
    lam, V, _ = P.components(4.0 * np.outer(t, t), 1, 1)
    assert V[0, 0] > 0 and V[1, 0] < 0
    with pytest.raises(ValueError, match="at most N - 1 = 4"):
        P.components(G, K_used, 5)
    with pytest.raises(ValueError, match="must be 1 .. 64"):
        P.components(np.eye(100), 1, 65)
    with pytest.raises(ValueError, match="must be 1 .. 64"):
        P.components(G, K_used, 0)


# ------------------------------------------------------------------ placement
def test_hat_matrix_placement_equals_the_refit():
    rng = np.random.default_rng(4)
    N, npc = 40, 6
    pcs = rng.normal(size=(N, npc)) * np.array([5.0, 4.0, 3.0, 2.0, 1.5, 1.0])
    locs = np.stack([3.0 * pcs[:, 0] - pcs[:, 2], 2.0 * pcs[:, 1] + 0.5 * pcs[:, 3]], axis=1) + rng.normal(size=(N, 2))
    locs[[5, 17, 33]] = np.nan
    located = ~np.isnan(locs).any(axis=1)
    fast, slow = P.placements(pcs, locs, located, npc), P.placements_refit(pcs, locs, located, npc)
    assert fast.shape == slow.shape == (npc, N, 2) and not np.isnan(fast).any()
    assert np.abs(fast - slow).max() <= 1e-9 * np.abs(slow).max()
    assert np.abs(fast[:, located] - fast[:, located].mean()).min() > 0                   # ... and it is no constant
    # leverage 1: a sample alone on a PC cannot be predicted without itself
    lone = np.zeros((5, 1))
    lone[0] = 1.0
    got = P.placements(lone, np.arange(10.0).reshape(5, 2), np.ones(5, dtype=bool), 1)
    assert np.isnan(got[0, 0]).all() and not np.isnan(got[0, 1:]).any()


def test_choose_p_ties_go_to_the_smaller_p():
    locs = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [np.nan, np.nan]])
    located = np.array([True, True, True, False])
    placed = np.zeros((3, 4, 2))
    placed[0] += 5.0                                                                     # p = 1 far off, p = 2 and 3 equal
    p, med = BL.choose_smallest_median(placed, locs, located, False, P.NOTHING_TO_CHOOSE_BY)
    assert p == 2 and med[1] == med[2] == 1.0 and med[0] > med[1]
    with pytest.raises(ValueError, match="nothing to choose p by"):
        BL.choose_smallest_median(np.full((2, 4, 2), np.nan), locs, located, False, P.NOTHING_TO_CHOOSE_BY)


def test_pc_r2_names_the_axis():
    rng = np.random.default_rng(6)
    pcs = rng.normal(size=(50, 3))
    locs = np.stack([2.0 * pcs[:, 1] + 7.0, rng.normal(size=50)], axis=1)
    r2 = P.pc_r2(pcs, locs, np.ones(50, dtype=bool))
    assert r2.shape == (3, 2) and r2[1, 0] == pytest.approx(1.0) and r2[:, 1].max() < 0.3 and r2[0, 0] < 0.3


# ------------------------------------------------------------------ the binding
def test_pca_header_is_bound_as_the_other_headers_are():
    from tests.abi_util import check_extension
    vp, i64 = C.c_void_p, C.c_int64
    check_extension("pca", {"loc_grm_pairs": (C.c_int, [vp, C.c_int, i64, i64, vp, vp, C.c_int, vp, vp, i64, vp]),
                            "loc_grm_work_bytes": (i64, [C.c_int, i64, C.c_int]),
                            "loc_pca_loadings": (C.c_int, [vp, C.c_int, i64, i64, vp, vp, vp, C.c_int, vp, vp])},
                    {"LOC_PCA_TILE": 128, "LOC_PCA_BLOCK": 32, "LOC_PCA_MAX_NPC": 64, "LOC_PCA_SITES": 256})
    assert (P.TILE, P.BLOCK, P.NPC_LIMIT) == (128, 32, 64)


# ------------------------------------------------------------------ the command
NAMES = ("_pca.txt", "_pca_eigenvalues.txt", "_pca_locs.txt", "_pca_summary.json", "_grm.npz", "_pca_loadings.npz")


@pytest.fixture(scope="module")
def golden_run(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pca") / "g")
    assert P.main(["--vcf", U.VCF, "--sample_data", U.SAMPLE_DATA, "--out", out, "--min_mac", "2", "--host", "--npc", "12",
                   "--keep_matrix", "--loadings", "--silence"]) == 0
    return out


def test_the_command_on_the_golden_vcf(golden_run):
    out = golden_run
    s = json.load(open(out + "_pca_summary.json"))
    assert (s["N"], s["n_located"], s["K"], s["K_used"], s["P"], s["npc"], s["pmax"]) == (500, 450, 5830, 5830, 2, 12, 12)
    med = s["median_error_by_p"]
    assert len(med) == 12 and s["p"] == s["p_auto"] == int(np.argmin(med)) + 1 and s["p_chosen_by"] == "auto"
    assert s["median_error"] == med[s["p"] - 1] and 0 < s["median_error"] <= s["mean_error"] and med[1] < med[0]
    assert 0 < s["r2_x"] <= 1 and 0 < s["r2_y"] <= 1 and s["error_unit"] == "map units"
    head, rows = U.read_table(out + "_pca.txt")
    assert head == ["sampleID"] + [f"PC{q}" for q in range(1, 13)] and len(rows) == 500 and rows[0][0] == "msp_0"
    assert all(repr(float(v)) == v for v in rows[0][1:])
    pcs = np.array([[float(v) for v in r[1:]] for r in rows])
    head, ev = U.read_table(out + "_pca_eigenvalues.txt")
    assert head == ["PC", "eigenvalue", "variance_share", "r2_x", "r2_y"] and [int(r[0]) for r in ev] == list(range(1, 13))
    lam, share = np.array([float(r[1]) for r in ev]), np.array([float(r[2]) for r in ev])
    assert (np.diff(lam) < 0).all() and lam[-1] > 0 and (share > 0).all() and share.sum() <= 1
    assert lam.tolist() == s["eigenvalues"] and share.tolist() == s["variance_share"]
    assert all(0 <= float(r[3]) <= 1 and 0 <= float(r[4]) <= 1 for r in ev)
    z = np.load(out + "_grm.npz")
    A = z["G"] / int(z["K_used"])
    assert z["G"].dtype == np.float64 and z["G"].shape == (500, 500) and z["samples"][0] == "msp_0" and int(z["K_used"]) == 5830
    assert np.array_equal(z["G"], z["G"].T)
    # scores times scores-transposed is the top of G / K_used: what is left has the next eigenvalue as its norm
    full = np.linalg.eigvalsh(A)[::-1]
    assert np.allclose(lam, full[:12], rtol=1e-10) and np.allclose((pcs * pcs).sum(axis=0), lam, rtol=1e-10)
    assert np.linalg.norm(A - pcs @ pcs.T, 2) == pytest.approx(full[12], rel=1e-8)
    assert share == pytest.approx(lam / np.trace(A), rel=1e-12)
    locs = open(out + "_pca_locs.txt").read().splitlines()
    assert locs[0] == "x,y,sampleID" and len(locs) == 501
    rows = [line.split(",") for line in locs[1:]]
    assert all(len(r) == 3 and np.isfinite(float(r[0])) and np.isfinite(float(r[1])) for r in rows)
    assert rows[0][2] == "msp_0" and repr(float(rows[0][0])) == rows[0][0]
    ld = np.load(out + "_pca_loadings.npz")
    assert ld["loadings"].shape == (5830, 12) and ld["loadings"].dtype == np.float64 and ld["mean"].dtype == np.float32
    assert len(ld["sites"]) == 5830 and (np.diff(ld["sites"]) > 0).all()
    assert np.allclose((ld["loadings"] ** 2).sum(axis=0), 1.0, rtol=1e-5)               # Z' u / sqrt(K lam) has unit length
    assert not [f for f in os.listdir(os.path.dirname(out)) if "predlocs" in f or ".tmp" in f]


def test_two_runs_write_identical_bytes(golden_run, tmp_path):
    out = str(tmp_path / "again")
    assert P.main(["--vcf", U.VCF, "--sample_data", U.SAMPLE_DATA, "--out", out, "--min_mac", "2", "--host", "--npc", "12",
                   "--keep_matrix", "--loadings", "--silence"]) == 0
    for name in NAMES:
        assert open(out + name, "rb").read() == open(golden_run + name, "rb").read(), name


def test_a_fixed_p_and_max_snps(tmp_path, capsys):
    from tests import neighbors_util as NU
    vcf = NU.write_vcf_cut(str(tmp_path / "cut.vcf"), 80, 400)
    out = str(tmp_path / "o")
    assert P.main(["--vcf", vcf, "--sample_data", U.SAMPLE_DATA, "--out", out, "--host", "--npc", "5", "--p", "3", "--max_SNPs",
                   "50", "--seed", "7"]) == 0
    s = json.load(open(out + "_pca_summary.json"))
    assert s["K"] == 50 and s["p"] == 3 and s["p_chosen_by"] == "--p" and s["median_error"] == s["median_error_by_p"][2]
    text = capsys.readouterr().out
    assert "variance share of PC1..4" in text and "x is carried by PC" in text and "median PC-regression leave-one-out error" in text
    assert not os.path.exists(out + "_grm.npz") and not os.path.exists(out + "_pca_loadings.npz")


# ------------------------------------------------------------------ stops and errors
def test_without_a_gpu_the_command_stops_unless_host(tmp_path, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match="no GPU visible.*loc_grm_pairs.*--host"):
        P.main(["--vcf", U.VCF, "--sample_data", U.SAMPLE_DATA, "--out", str(tmp_path / "o")])
    with pytest.raises(SystemExit, match="no GPU visible.*loc_grm_pairs.*--host"):
        P.pca(np.zeros((4, 3), dtype=np.int8), 2, list("abcd"), np.arange(8.0).reshape(4, 2), str(tmp_path / "o"), npc=2)
    assert not os.listdir(tmp_path)


def test_refusals_from_shared_code_name_this_command(tmp_path):
    ids = [f"msp_{i}" for i in range(48, 54)]
    g = np.random.default_rng(3).integers(0, 3, (6, 30))

    def matrix(path, g, ids):
        with open(path, "w") as fh:
            fh.write("sampleID\t" + "\t".join(f"v{k}" for k in range(g.shape[1])) + "\n")
            for s, row in zip(ids, g):
                fh.write(s + "\t" + "\t".join(str(v) for v in row) + "\n")
        return str(path)

    base = ["--sample_data", U.SAMPLE_DATA, "--out", str(tmp_path / "o"), "--host", "--silence", "--npc", "2"]
    g3 = g.copy()
    g3[2, 5] = 3
    with pytest.raises(SystemExit, match="^locator_amd.pca: .*count of 3.*above 2"):
        P.main(["--matrix", matrix(tmp_path / "three.txt", g3, ids)] + base)
    with pytest.raises(SystemExit, match="^locator_amd.pca: 1 genotype samples are not in .*first: nobody"):
        P.main(["--matrix", matrix(tmp_path / "who.txt", g, ids[:5] + ["nobody"])] + base)
    assert P.main(["--matrix", matrix(tmp_path / "ok.txt", g, ids)] + base) == 0


def test_refusals(tmp_path, capsys):
    base = ["--sample_data", U.SAMPLE_DATA, "--out", str(tmp_path / "o"), "--host", "--silence"]
    for extra, text in (([], "exactly one of --vcf / --zarr / --matrix"),
                        (["--vcf", U.VCF, "--npc", "0"], "--npc must be 1 .. 64"),
                        (["--vcf", U.VCF, "--npc", "65"], "--npc must be 1 .. 64"),
                        (["--vcf", U.VCF, "--p", "some"], "--p must be"),
                        (["--vcf", U.VCF, "--p", "0"], "--p must be"),
                        (["--vcf", U.VCF, "--phased"], "unrecognized arguments"),
                        (["--vcf", U.VCF, "--dosage", "DS"], "unrecognized arguments")):
        with pytest.raises(SystemExit) as e:
            P.main(base + extra)
        assert e.value.code == 2 and text in capsys.readouterr().err
    c = U.spread_counts(8, 30, 2)
    samples = [f"s{i}" for i in range(8)]
    locs = np.random.default_rng(1).uniform(0, 9, (8, 2))
    with pytest.raises(ValueError, match="exceeds the ploidy 1"):                        # a count above P
        P.pca(c, 1, samples, locs, None, npc=2, host=True, silence=True)
    with pytest.raises(SystemExit, match="at most N - 1"):
        P.pca(c, 2, samples, locs, None, npc=8, host=True, silence=True)
    with pytest.raises(SystemExit, match="--p must be `auto` or 1 .. .* = 3"):
        P.pca(c, 2, samples, locs, None, npc=3, p=4, host=True, silence=True)
    few = locs.copy()
    few[2:] = np.nan
    with pytest.raises(SystemExit, match="fewer than 3 samples"):
        P.pca(c, 2, samples, few, None, npc=3, host=True, silence=True)
    five = locs.copy()
    five[5:] = np.nan                                                                    # pmax = min(npc, located - 2) = 3
    assert P.pca(c, 2, samples, five, None, npc=6, host=True, silence=True)["pmax"] == 3
    assert not os.listdir(tmp_path)
