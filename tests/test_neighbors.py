"""The neighbors command without a GPU (locator_amd/neighbors.py): the definition of the pair statistics on hand-written rows,
the plane identity the kernel computes against the brute-force sum, the neighbour order on crafted ties, the choice of k, the
binding of include/locator_hip_neighbors.h, the --host command on the golden VCF, and the refusals.  Every comparison is exact:
integers, and float64 from one division."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from locator_amd import baselines as BL
from locator_amd import neighbors as NB
from tests import neighbors_util as U


def brute(c):
    """d, n by two Python loops over pairs: nothing shared with pairs_host but the definition."""
    c = np.asarray(c, dtype=np.int64)
    N = len(c)
    d, n = np.zeros((N, N), dtype=np.int64), np.zeros((N, N), dtype=np.int64)
    for i in range(N):
        for j in range(N):
            ok = (c[i] >= 0) & (c[j] >= 0)
            n[i, j] = ok.sum()
            d[i, j] = np.abs(c[i] - c[j])[ok].sum()
    return d, n


# ------------------------------------------------------------------ pair statistics
def test_every_pair_of_values_by_hand():
    vals = [-1, 0, 1, 2]
    a = np.repeat(vals, 4)                                   # -1 -1 -1 -1  0 0 0 0  1 1 1 1  2 2 2 2
    b = np.tile(vals, 4)                                     # -1  0  1  2 -1 0 1 2 -1 0 1 2 -1 0 1 2
    c = np.stack([a, b, np.full(16, -1), np.full(16, 2)]).astype(np.int8)
    d, n = NB.pairs_host(c)
    assert d.dtype == n.dtype == np.int32
    # rows 0 and 1 share the 9 sites with both in 0..2: |0-0| |0-1| |0-2| |1-0| |1-1| |1-2| |2-0| |2-1| |2-2| = 8
    assert n.tolist() == [[12, 9, 0, 12], [9, 12, 0, 12], [0, 0, 0, 0], [12, 12, 0, 16]]
    assert d.tolist() == [[0, 8, 0, 12], [8, 0, 0, 12], [0, 0, 0, 0], [12, 12, 0, 0]]
    D = NB.distances(d, n, 2)
    assert D[0, 1] == 8 / 18 and D[0, 3] == 0.5 and D[3, 3] == 0.0
    assert np.isnan(D[2]).all() and np.isnan(D[:, 2]).all()                   # the all-missing row: NaN, its own pair included
    assert np.array_equal(d, brute(c)[0]) and np.array_equal(n, brute(c)[1])


def test_haploid_counts():
    c = np.array([[0, 1, 1, -1, 0], [1, 1, 0, 0, -1], [0, 0, 0, 0, 0]], dtype=np.int8)
    d, n = NB.pairs_host(c)
    assert d.tolist() == [[0, 2, 2], [2, 0, 2], [2, 2, 0]] and n.tolist() == [[4, 3, 4], [3, 4, 4], [4, 4, 5]]
    assert NB.distances(d, n, 1)[0, 1] == 2 / 3 and NB.distances(d, n, 2)[0, 1] == 2 / 6   # one division by P n
    with pytest.raises(ValueError, match="exceeds the ploidy 1"):
        BL.check_counts(np.array([[0, 2]], dtype=np.int8), 1)


@pytest.mark.parametrize("P", [1, 2])
def test_the_plane_identity_equals_the_brute_force_sum(P):
    c = U.counts(37, 211, 5 + P, P=P)
    c[11] = -1
    want = brute(c)
    for got in (NB.pairs_host(c), NB.pairs_planes(c)):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    m, a, t1, t2 = NB.planes(c)
    assert np.array_equal(a, np.where(c < 0, 0, c)) and np.array_equal(m, c >= 0) and not a[11].any()
    lo, hi = np.minimum(a[:, None, :], a[None, :, :]), t1[:, None, :] * t1[None, :, :] + t2[:, None, :] * t2[None, :, :]
    assert np.array_equal(lo, hi)                                             # min(a, b) = [a>=1][b>=1] + [a>=2][b>=2]


def test_host_pairs_in_chunks_of_sites():
    c = U.counts(9, 50, 3)
    assert all(np.array_equal(x, y) for x, y in zip(NB.pairs_host(c, chunk=9 * 7), NB.pairs_host(c)))


def test_count_matrix_missing_stays_missing():
    gt = np.array([[[0, 1], [1, 1], [-1, 1], [0, -1], [-1, -1]],
                   [[0, 0], [1, 0], [1, 1], [0, 0], [1, 0]],
                   [[1, 1], [1, 1], [1, 1], [1, 1], [1, 1]]], dtype=np.int8)
    c, P = BL.count_matrix(gt, [0, 1])
    assert P == 2 and c.dtype == np.int8 and c.shape == (5, 2)
    assert c.T.tolist() == [[1, 2, -1, -1, -1], [0, 1, 2, 0, 1]]              # a partly missing call counts as missing
    c1, P1 = BL.count_matrix(gt.reshape(3, 10, 1), [1])
    assert P1 == 1 and c1[:, 0].tolist() == [0, 0, 1, 0, 1, 1, 0, 0, 1, 0]


# ------------------------------------------------------------------ neighbours
def test_duplicate_rows_resolve_to_the_lower_index():
    base = U.counts(1, 40, 9, missing=0.0)[0]
    far = (2 - base).astype(np.int8)
    c = np.stack([base, far, base, base, far])                                # 0, 2, 3 identical; 1, 4 identical
    d, n = NB.pairs_host(c)
    located = np.array([True, True, True, True, False])
    nbr, dist = NB.knn_host(d, n, 2, located, 4)
    assert nbr[0].tolist()[:2] == [2, 3] and dist[0, 0] == dist[0, 1] == 0.0
    assert nbr[2].tolist()[:2] == [0, 3] and nbr[3].tolist()[:2] == [0, 2]
    assert nbr[0].tolist() == [2, 3, 1, -1] and np.isnan(dist[0, 3])          # 3 candidates: -1 / NaN fill
    assert nbr[4].tolist() == [1, 0, 2, 3]                                    # the unlocated row gets neighbours ...
    assert not (nbr == 4).any()                                               # ... and is nobody's candidate


def test_ties_between_different_fractions_and_nan_pairs():
    d = np.array([[0, 1, 2, 3, 0], [1, 0, 0, 0, 0], [2, 0, 0, 0, 0], [3, 0, 0, 0, 0], [0, 0, 0, 0, 0]], dtype=np.int32)
    n = np.array([[9, 4, 8, 12, 0], [4, 9, 1, 1, 1], [8, 1, 9, 1, 1], [12, 1, 1, 9, 1], [0, 1, 1, 1, 9]], dtype=np.int32)
    nbr, dist = NB.knn_host(d, n, 2, np.ones(5, dtype=bool), 4)
    assert nbr[0].tolist() == [1, 2, 3, -1] and dist[0, :3].tolist() == [0.125, 0.125, 0.125]   # 1/8 = 2/16 = 3/24; 4 is NaN
    want = np.argsort(np.array([np.inf, 0.125, 0.125, 0.125]), kind="stable")[:3]
    assert want.tolist() == [1, 2, 3]


def test_placement_is_the_rank_order_mean():
    locs = np.array([[0.0, 0.0], [1.0, 10.0], [2.0, 20.0], [np.nan, np.nan]])
    nbr = np.array([[1, 2, -1], [0, 2, -1], [1, 0, -1], [2, 1, 0]], dtype=np.int32)
    placed = NB.placements(nbr, locs)
    assert placed.shape == (3, 4, 2)
    assert placed[0, 0].tolist() == [1.0, 10.0] and placed[1, 0].tolist() == [1.5, 15.0]
    assert placed[2, 0].tolist() == [1.5, 15.0]                               # fewer than k neighbours: the mean of those there are
    assert placed[2, 3].tolist() == [(2.0 + 1.0 + 0.0) / 3.0, (20.0 + 10.0 + 0.0) / 3.0]
    none = NB.placements(np.full((1, 2), -1, dtype=np.int32), locs)
    assert np.isnan(none).all()


def test_k_auto_is_the_argmin_of_the_recorded_errors(tmp_path):
    c = U.counts(60, 300, 12)
    rng = np.random.default_rng(13)
    locs = rng.uniform(0, 50, (60, 2))
    locs[50:] = np.nan
    samples = [f"s{i}" for i in range(60)]
    out = str(tmp_path / "o")
    s = NB.neighbors(c, 2, samples, locs, out, kmax=12, host=True, silence=True)
    med = s["median_error_by_k"]
    assert len(med) == 12 and s["k"] == s["k_auto"] == int(np.argmin(med)) + 1 and s["k_chosen_by"] == "auto"
    # ... each recorded error is the leave-one-out median at that k, from the neighbour table alone
    nbr = s["_nbr"]
    for k in (1, 5, 12):
        xy = np.array([locs[nbr[i, :k]].mean(axis=0) for i in range(50)])
        assert med[k - 1] == pytest.approx(np.median(np.sqrt(((xy - locs[:50]) ** 2).sum(axis=1))), rel=1e-12)
    assert (nbr[:, :12] < 50).all() and (nbr >= 0).all()
    fixed = NB.neighbors(c, 2, samples, locs, out, k=7, kmax=12, host=True, silence=True)
    assert fixed["k"] == 7 and fixed["k_auto"] == s["k_auto"] and fixed["median_error"] == med[6]
    assert json.load(open(out + "_knn_summary.json"))["k_chosen_by"] == "--k"
    # the smallest k wins a tie: two located samples, every k gives the same placement
    two = NB.neighbors(c[:3], 2, samples[:3], np.array([[0.0, 0.0], [1.0, 1.0], [np.nan, np.nan]]), None, kmax=3, host=True,
                       silence=True)
    assert two["median_error_by_k"] == [2 ** 0.5] * 3 and two["k"] == 1


def test_longlat_errors_are_the_haversine_of_plot():
    from locator_amd.plot import distance_km
    xy, truth = np.array([[10.0, 50.0], [0.0, 0.0]]), np.array([[11.0, 51.0], [0.0, 1.0]])
    assert np.array_equal(BL.errors(xy, truth, True), distance_km(xy[:, 0], xy[:, 1], truth[:, 0], truth[:, 1]))
    assert BL.errors(xy, truth)[1] == 1.0


# ------------------------------------------------------------------ the binding
def test_neighbor_header_is_bound_as_the_other_headers_are():
    from locator_amd import _abi
    from tests.abi_util import check_extension
    vp, i64 = C.c_void_p, C.c_int64
    check_extension("neighbor", {"loc_ibs_pairs": (C.c_int, [vp, C.c_int, i64, i64, C.c_int, vp, vp, vp, i64, vp]),
                                 "loc_ibs_work_bytes": (i64, [C.c_int, i64, C.c_int]),
                                 "loc_ibs_knn": (C.c_int, [vp, vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp])},
                    {"LOC_IBS_TILE": 128, "LOC_IBS_BLOCK": 64})
    assert (_abi.LOC_IBS_TILE, _abi.LOC_IBS_BLOCK) == (NB.TILE, NB.BLOCK) == (128, 64)


# ------------------------------------------------------------------ the command
@pytest.fixture(scope="module")
def golden_run(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("neighbors") / "g")
    assert NB.main(["--vcf", U.VCF, "--sample_data", U.SAMPLE_DATA, "--out", out, "--min_mac", "2", "--host", "--close", "0",
                    "--keep_matrix", "--silence"]) == 0
    return out


def test_the_command_on_the_golden_vcf(golden_run):
    out = golden_run
    s = json.load(open(out + "_knn_summary.json"))
    assert (s["N"], s["n_located"], s["K"], s["P"]) == (500, 450, 5830, 2)
    assert s["n_close_pairs"] == 14 and s["close"] == 0.0
    assert s["k"] == s["k_auto"] == int(np.argmin(s["median_error_by_k"])) + 1 and len(s["median_error_by_k"]) == 32
    assert s["median_error"] == s["median_error_by_k"][s["k"] - 1] and 0 < s["median_error"] <= s["mean_error"]
    assert 0 < s["r2_x"] <= 1 and 0 < s["r2_y"] <= 1 and 0 < s["pearson_r_ibs_geo"] <= 1
    locs = open(out + "_knn_locs.txt").read().splitlines()
    assert locs[0] == "x,y,sampleID" and len(locs) == 501
    rows = [line.split(",") for line in locs[1:]]
    assert all(len(r) == 3 and np.isfinite(float(r[0])) and np.isfinite(float(r[1])) for r in rows)
    assert rows[0][2] == "msp_0" and repr(float(rows[0][0])) == rows[0][0]     # the number formatting of a predlocs file
    nb = [line.split("\t") for line in open(out + "_neighbors.txt").read().splitlines()]
    assert nb[0] == ["sampleID", "rank", "neighborID", "ibs_dist", "n_sites"] and len(nb) == 1 + 500 * 32
    assert [int(r[1]) for r in nb[1:33]] == list(range(1, 33)) and all(int(r[4]) == 5830 for r in nb[1:])
    dist = np.array([float(r[3]) for r in nb[1:]]).reshape(500, 32)
    assert (np.diff(dist, axis=1) >= 0).all()
    cp = [line.split("\t") for line in open(out + "_close_pairs.txt").read().splitlines()]
    assert cp[0] == ["sampleA", "sampleB", "ibs_dist", "n_sites"] and len(cp) == 15
    assert all(float(r[2]) == 0.0 and int(r[3]) == 5830 and r[0] != r[1] for r in cp[1:])
    z = np.load(out + "_ibs.npz")
    assert z["d"].shape == z["n"].shape == (500, 500) and z["d"].dtype == np.int32 and z["samples"][0] == "msp_0"
    assert int((np.triu(z["d"] == 0, 1)).sum()) == 14 and (z["n"] == 5830).all()
    assert np.array_equal(z["d"], z["d"].T) and not np.diag(z["d"]).any()
    assert not [f for f in os.listdir(os.path.dirname(out)) if "predlocs" in f or ".tmp" in f]
    # the tie rule is not cosmetic here: most located rows have an exact tie inside their first 33 neighbours
    located = ~np.isnan(BL.read_locations(U.SAMPLE_DATA, z["samples"], NB.PROG)).any(axis=1)
    nbr, dd = NB.knn_host(z["d"], z["n"], 2, located, 33)
    assert int(((np.diff(dd, axis=1) == 0).any(axis=1) & located).sum()) == 391
    # ... and the table holds exactly these rows
    ids = z["samples"]
    assert [r[2] for r in nb[1:33]] == ids[nbr[0, :32]].tolist()


def test_max_snps_draws_the_sites_a_fit_would(tmp_path):
    from locator_amd import genotypes as G
    vcf = U.write_vcf_cut(str(tmp_path / "cut.vcf"), 80, 400)
    out = str(tmp_path / "o")
    argv = ["--vcf", vcf, "--sample_data", U.SAMPLE_DATA, "--out", out, "--host", "--silence", "--keep_matrix", "--kmax", "4"]
    assert NB.main(argv + ["--max_SNPs", "50", "--seed", "7"]) == 0
    gt = G.read_vcf(vcf)["calldata/GT"]
    np.random.seed(7)
    _, idx = G.filter_snps(gt, min_mac=2, max_snps=50, verbose=False, sites=True)
    c, P = BL.count_matrix(gt, idx)
    z = np.load(out + "_ibs.npz")
    assert json.load(open(out + "_knn_summary.json"))["K"] == 50
    assert np.array_equal(z["d"], NB.pairs_host(c)[0])


# ------------------------------------------------------------------ stops and errors
def test_without_a_gpu_the_command_stops_unless_host(tmp_path, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match="no GPU visible.*loc_ibs_pairs.*--host"):
        NB.main(["--vcf", U.VCF, "--sample_data", U.SAMPLE_DATA, "--out", str(tmp_path / "o")])
    assert not os.listdir(tmp_path)


def test_refusals(tmp_path, capsys):
    base = ["--sample_data", U.SAMPLE_DATA, "--out", str(tmp_path / "o"), "--host", "--silence"]
    for extra, text in (([], "exactly one of --vcf / --zarr / --matrix"),
                        (["--vcf", U.VCF, "--matrix", "m.txt"], "exactly one of --vcf / --zarr / --matrix"),
                        (["--vcf", U.VCF, "--kmax", "0"], "--kmax must be 1 .. 64"),
                        (["--vcf", U.VCF, "--kmax", "65"], "--kmax must be 1 .. 64"),
                        (["--vcf", U.VCF, "--k", "9", "--kmax", "8"], "--k must be"),
                        (["--vcf", U.VCF, "--k", "many"], "--k must be"),
                        (["--vcf", U.VCF, "--close", "-1"], "--close must be"),
                        (["--vcf", U.VCF, "--phased"], "unrecognized arguments"),
                        (["--vcf", U.VCF, "--dosage", "DS"], "unrecognized arguments")):
        with pytest.raises(SystemExit) as e:
            NB.main(base + extra)
        assert e.value.code == 2 and text in capsys.readouterr().err
    # a count matrix above 2, a sample without a row in --sample_data, and no located sample at all
    ids = [f"msp_{i}" for i in range(48, 54)]                    # two to place, four located
    rng = np.random.default_rng(3)
    g = rng.integers(0, 3, (6, 30))

    def matrix(path, g, ids):
        with open(path, "w") as fh:
            fh.write("sampleID\t" + "\t".join(f"v{k}" for k in range(g.shape[1])) + "\n")
            for s, row in zip(ids, g):
                fh.write(s + "\t" + "\t".join(str(v) for v in row) + "\n")
        return str(path)

    ok = matrix(tmp_path / "ok.txt", g, ids)
    assert NB.main(["--matrix", ok] + base + ["--kmax", "3"]) == 0
    assert json.load(open(str(tmp_path / "o") + "_knn_summary.json"))["N"] == 6
    g3 = g.copy()
    g3[2, 5] = 3
    with pytest.raises(SystemExit, match="count of 3.*above 2"):
        NB.main(["--matrix", matrix(tmp_path / "three.txt", g3, ids)] + base)
    with pytest.raises(SystemExit, match="1 genotype samples are not in .*first: nobody"):
        NB.main(["--matrix", matrix(tmp_path / "who.txt", g, ids[:5] + ["nobody"])] + base)
    sd = str(tmp_path / "nowhere.txt")
    with open(sd, "w") as fh:
        fh.write("sampleID\tx\ty\n" + "".join(f"{s}\tNA\tNA\n" for s in ids))
    with pytest.raises(SystemExit, match="no sample .* has a location"):
        NB.main(["--matrix", ok, "--sample_data", sd, "--out", str(tmp_path / "p"), "--host", "--silence"])
    with pytest.raises(ValueError, match="exceeds the ploidy 2"):
        NB.pairs_host(np.array([[0, 3]], dtype=np.int8))
    with pytest.raises(ValueError, match="could leave int32"):
        BL.check_counts(np.lib.stride_tricks.as_strided(np.zeros(1, dtype=np.int8), (1, 2 ** 30), (0, 0)), 2)
