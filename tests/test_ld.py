"""The ld command without a GPU (locator_amd/ld.py): the six pair sums and r2 by hand, the plane identity the kernel computes
against the brute-force sums, the NaN rules, the window, the greedy walk, the binding of include/locator_hip_ld.h, the --host
command on the golden VCF, --ld_prune of the neighbors command, and the refusals.  Every comparison is exact: integers, bits,
and float64 from two products and one division of exact integers."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from locator_amd import baselines as BL
from locator_amd import ld as LD
from locator_amd import neighbors as NB
from tests import ld_util as U


# ------------------------------------------------------------------ sums and r2
def test_every_pair_of_values_by_hand():
    vals = [-1, 0, 1, 2]
    a = np.repeat(vals, 4)                                   # -1 -1 -1 -1  0 0 0 0  1 1 1 1  2 2 2 2
    b = np.tile(vals, 4)                                     # -1  0  1  2 -1 0 1 2 -1 0 1 2 -1 0 1 2
    ct = np.stack([a, b]).astype(np.int8)
    s = LD.sums_host(ct, 1)
    assert s.dtype == np.int32 and s.shape == (2, 1, 6)
    # the 9 samples with both called: a = 0 0 0 1 1 1 2 2 2, b = 0 1 2 0 1 2 0 1 2
    assert s[0, 0].tolist() == [9, 9, 9, 9, 15, 15] and not s[1].any()
    r2 = LD.r2_host(s)
    assert r2[0, 0] == 0.0 and np.isnan(r2[1, 0])            # cov = 9 * 9 - 9 * 9 = 0; the last site has nobody to meet
    assert np.array_equal(s, U.brute(ct, 1, [1, 0]))
    # three samples by hand: a = 0 1 2, b = 0 2 2 -> n 3, sa 3, sb 4, sab 6, saa 5, sbb 8: cov 6, va 6, vb 8, r2 = 36 / 48
    s3 = LD.sums_host(np.array([[0, 1, 2, -1], [0, 2, 2, 1]], dtype=np.int8), 4)
    assert s3[0, 0].tolist() == [3, 3, 4, 6, 5, 8] and not s3[0, 1:].any()
    assert LD.r2_host(s3)[0, 0] == (6.0 * 6.0) / (6.0 * 8.0) == 0.75
    assert LD.over_host(LD.r2_host(s3), 0.75).tolist() == [[0], [0]] and LD.over_host(LD.r2_host(s3), 0.7).tolist() == [[1], [0]]


@pytest.mark.parametrize("P", [1, 2])
def test_the_plane_identity_equals_the_brute_force_sums(P):
    ct = U.site_counts(41, 67, 3 + P, P=P, missing=0.3)
    ct[11] = -1
    W = 9
    reach = LD.clamp_reach(None, len(ct), W)
    want = U.brute(ct, W, reach)
    assert np.array_equal(LD.sums_host(ct, W), want) and np.array_equal(LD.sums_host(ct, W, rows=7), want)
    m, a, a2 = (p.astype(np.int64) for p in LD.planes(ct))
    assert np.array_equal(a, np.where(ct < 0, 0, ct)) and np.array_equal(m, ct >= 0) and np.array_equal(a2, a * a)
    assert LD.planes(ct)[2].max() == (4 if P == 2 else 1) and not a[11].any()
    prod = [m @ m.T, a @ m.T, m @ a.T, a @ a.T, a2 @ m.T, m @ a2.T]            # the six products of the kernel
    for i in range(len(ct)):
        for lag in range(reach[i]):
            assert [int(p[i, i + 1 + lag]) for p in prod] == want[i, lag].tolist()


def test_nan_rules():
    rng = np.random.default_rng(5)
    ct = rng.integers(0, 3, (6, 30)).astype(np.int8)
    ct[1] = 1                                                # monomorphic
    ct[2] = -1                                               # all missing
    ct[3, 1:] = -1                                           # one call: n < 2 with everybody
    ct[4, :15] = -1
    ct[5, 15:] = -1                                          # 4 and 5 share no sample
    s = LD.sums_host(ct, 5)
    r2 = LD.r2_host(s)
    assert np.isnan(r2[0, 0]) and np.isnan(r2[0, 1]) and np.isnan(r2[0, 2]) and np.isnan(r2[4, 0])
    assert s[0, 0, 0] == 30 and s[0, 1, 0] == 0 and s[0, 2, 0] == 1 and s[4, 0, 0] == 0
    assert np.isfinite(r2[0, 3]) and np.isfinite(r2[0, 4])
    assert np.isnan(r2[5]).all() and not s[5].any()          # past the end of the array
    with np.errstate(invalid="ignore"):
        assert not LD.unpack_bits(LD.over_host(r2, -1.0), 5)[np.isnan(r2)].any()      # NaN is never over, whatever the threshold
    assert LD.unpack_bits(LD.over_host(r2, -1.0), 5)[~np.isnan(r2)].all()


def test_bits_round_trip():
    rng = np.random.default_rng(6)
    for W in (1, 31, 32, 33, 100):
        flags = rng.random((7, W)) < 0.4
        over = LD.pack_bits(flags)
        assert over.dtype == np.uint32 and over.shape == (7, (W + 31) // 32) and np.array_equal(LD.unpack_bits(over, W), flags)
        assert all(bool(over[i, l // 32] >> np.uint32(l % 32) & np.uint32(1)) == flags[i, l] for i in range(7) for l in range(W))


# ------------------------------------------------------------------ the window
def test_reach():
    assert LD.reach_host(6, 3).tolist() == [3, 3, 3, 2, 1, 0]                 # the end of the array
    assert LD.reach_host(0, 3).tolist() == [] and LD.reach_host(1, 3).tolist() == [0]
    chrom = np.array(["1", "1", "1", "2", "2", "1"], dtype=object)
    assert LD.reach_host(6, 4, chrom).tolist() == [2, 1, 0, 1, 0, 0]          # a break ends the window; a name that returns is a new run
    pos = np.array([10, 20, 35, 5, 500, 501])
    assert LD.reach_host(6, 4, chrom, pos, 15).tolist() == [1, 1, 0, 0, 0, 0]
    assert LD.reach_host(6, 4, chrom, pos, 25).tolist() == [2, 1, 0, 0, 0, 0]
    assert LD.reach_host(6, 4, None, pos, 1).tolist() == [0, 0, 1, 0, 1, 0]   # an unsorted position is "at most B after"
    assert LD.reach_host(6, 1, chrom, pos, 10 ** 9).tolist() == [1, 1, 0, 1, 0, 0]
    with pytest.raises(ValueError, match="needs positions"):
        LD.reach_host(6, 4, chrom, None, 15)
    assert LD.clamp_reach([9, -3, 2, 2, 7, 1], 6, 4).tolist() == [4, 0, 2, 2, 1, 0]
    assert LD.clamp_reach(None, 3, 4).tolist() == [2, 1, 0]


# ------------------------------------------------------------------ the greedy walk
def test_greedy_on_a_chain():
    flags = np.zeros((4, 3), dtype=bool)
    flags[0, 0] = True                                       # a ~ b
    flags[1, 0] = True                                       # b ~ c, a !~ c
    kept, removed_by = LD.greedy_host(LD.pack_bits(flags))
    assert kept.tolist() == [True, False, True, True] and removed_by.tolist() == [-1, 0, -1, -1]
    flags[0, 1] = True                                       # a ~ c as well: both go to a
    kept, removed_by = LD.greedy_host(LD.pack_bits(flags))
    assert kept.tolist() == [True, False, False, True] and removed_by.tolist() == [-1, 0, 0, -1]
    assert LD.greedy_host(np.zeros((0, 1), dtype=np.uint32))[0].tolist() == []


@pytest.mark.parametrize("W", [1, 31, 32, 33, 100])
def test_the_word_wise_walk_equals_the_bit_wise_one(W):
    rng = np.random.default_rng(W)
    K = 400
    reach = LD.clamp_reach(rng.integers(0, W + 1, K), K, W)
    flags = (rng.random((K, W)) < 0.05) & (np.arange(W)[None] < reach[:, None])
    want = U.greedy_bitwise(flags, reach)
    got = LD.greedy_host(LD.pack_bits(flags))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert 0 < got[0].sum() < K and (got[1][~got[0]] < np.flatnonzero(~got[0])).all()


def test_lag_buckets():
    flags = np.zeros((3, 11), dtype=bool)
    flags[0, [0, 1, 2, 3, 4, 8, 10]] = True
    flags[1, [0, 7]] = True
    assert LD.lag_buckets(LD.pack_bits(flags), 11) == {"1": 2, "2": 1, "3-4": 2, "5-8": 2, "9-11": 2}
    assert list(LD.lag_buckets(LD.pack_bits(flags[:, :1]), 1)) == ["1"]
    assert list(LD.lag_buckets(np.zeros((0, 4), dtype=np.uint32), 100)) == ["1", "2", "3-4", "5-8", "9-16", "17-32", "33-64", "65-100"]


# ------------------------------------------------------------------ the binding
def test_ld_header_is_bound_as_the_other_headers_are():
    from locator_amd import _abi
    from tests.abi_util import check_extension
    vp, i64 = C.c_void_p, C.c_int64
    check_extension("ld", {"loc_ld_band": (C.c_int, [vp, i64, C.c_int, i64, C.c_int, vp, C.c_double, vp, vp, vp, vp])},
                    {"LOC_LD_TILE", "LOC_LD_BLOCK", "LOC_LD_MAX_WINDOW"})
    assert (_abi.LOC_LD_TILE, _abi.LOC_LD_BLOCK, _abi.LOC_LD_MAX_WINDOW) == (LD.TILE, LD.BLOCK, LD.MAX_WINDOW)
    assert LD.TILE % 32 == 0 and LD.BLOCK % 32 == 0 and LD.MAX_WINDOW >= 512


def test_count_matrix_sites_is_the_count_matrix_not_transposed():
    from locator_amd import genotypes as G
    gt = G.read_vcf(U.VCF)["calldata/GT"][:300]
    gt = gt.copy()
    gt[5, 3, 1] = -1
    idx = [7, 5, 200, 12]
    c, P = BL.count_matrix(gt, idx)
    ct, Pt = BL.count_matrix_sites(gt, idx)
    assert P == Pt == 2 and ct.dtype == np.int8 and ct.flags["C_CONTIGUOUS"] and np.array_equal(ct, c.T) and ct[1, 3] == -1


# ------------------------------------------------------------------ the command
@pytest.fixture(scope="module")
def golden_run(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ld") / "g")
    assert LD.main(["--vcf", U.VCF, "--out", out, "--r2", "0.2", "--ld_window", "100", "--min_mac", "2", "--host", "--keep_matrix",
                    "--silence"]) == 0
    return out


def test_the_command_on_the_golden_vcf(golden_run):
    out = golden_run
    s = json.load(open(out + "_ld_summary.json"))
    assert list(s) == ["K", "n_kept", "P", "N", "r2", "window", "window_bp", "n_pairs_compared", "n_pairs_over", "pairs_over_by_lag"]
    assert (s["K"], s["n_kept"], s["P"], s["N"], s["r2"], s["window"], s["window_bp"]) == (5830, 1996, 2, 500, 0.2, 100, None)
    assert s["n_pairs_over"] == 39958 and s["n_pairs_compared"] == 5830 * 100 - 100 * 101 // 2
    assert sum(s["pairs_over_by_lag"].values()) == 39958 and list(s["pairs_over_by_lag"])[:4] == ["1", "2", "3-4", "5-8"]
    rows = [line.split("\t") for line in open(out + "_ld_sites.txt").read().splitlines()]
    assert rows[0] == ["variant", "chrom", "pos", "kept", "removed_by"] and len(rows) == 5831
    variant = np.array([int(r[0]) for r in rows[1:]])
    kept = np.array([int(r[3]) for r in rows[1:]])
    assert (np.diff(variant) > 0).all() and kept.sum() == 1996 and kept[0] == 1 and {r[1] for r in rows[1:]} == {"1"}
    assert all((r[4] == "NA") == (r[3] == "1") for r in rows[1:])
    by = {int(r[0]): int(r[4]) for r in rows[1:] if r[4] != "NA"}
    kept_variants = set(variant[kept == 1].tolist())
    assert all(b < v and b in kept_variants for v, b in by.items())           # removed by an earlier site that was kept
    z = np.load(out + "_ld.npz")
    assert z["over"].dtype == np.uint32 and z["over"].shape == (5830, 4) and np.array_equal(z["sites"], variant)
    assert z["reach"].tolist() == LD.reach_host(5830, 100).tolist()
    assert int(LD.unpack_bits(z["over"], 100).sum()) == 39958
    # ... and the mask is the definition's: re-derived here from the counts, pair by pair on a stretch of the file
    from locator_amd import genotypes as G
    ct, _ = BL.count_matrix_sites(G.read_vcf(U.VCF)["calldata/GT"], variant[:150])
    r2 = LD.r2_host(U.brute(ct, 100, np.minimum(100, 149 - np.arange(150))))
    assert np.array_equal(LD.unpack_bits(z["over"], 100)[:50], r2[:50] > 0.2)
    assert not [f for f in os.listdir(os.path.dirname(out)) if ".tmp" in f]


@pytest.mark.parametrize("r2,kept", [("0.1", 1684), ("0.5", 2666)])
def test_other_thresholds_on_the_golden_vcf(tmp_path, r2, kept):
    out = str(tmp_path / "o")
    assert LD.main(["--vcf", U.VCF, "--out", out, "--r2", r2, "--host", "--silence"]) == 0      # --ld_window 100, --min_mac 2
    assert json.load(open(out + "_ld_summary.json"))["n_kept"] == kept


def test_two_chromosomes_a_bp_window_and_a_matrix(tmp_path):
    vcf, ct, chrom, pos = U.planted_vcf(tmp_path / "p.vcf", K=300, N=40)
    out = str(tmp_path / "o")
    assert LD.main(["--vcf", vcf, "--out", out, "--r2", "0.3", "--ld_window", "20", "--ld_window_bp", "1500", "--min_mac", "1",
                    "--host", "--silence", "--keep_matrix"]) == 0
    z = np.load(out + "_ld.npz")
    sites = z["sites"]
    assert np.array_equal(z["reach"], LD.reach_host(len(sites), 20, chrom[sites], pos[sites], 1500))
    assert z["reach"].max() <= 20 and len(np.unique(z["reach"])) > 5 and z["reach"][sites < 163][-1] == 0      # the break
    want = LD.band_host(ct[sites], 20, z["reach"], 0.3)[0]
    assert np.array_equal(z["over"], want) and want.any()
    rows = [line.split("\t") for line in open(out + "_ld_sites.txt").read().splitlines()][1:]
    assert {r[1] for r in rows} == {"chr1", "chr2"} and [int(r[2]) for r in rows] == pos[sites].tolist()
    assert all(chrom[int(r[0])] == chrom[int(r[4])] for r in rows if r[4] != "NA")
    # a count matrix: one chromosome, no positions
    with open(tmp_path / "m.txt", "w") as fh:
        fh.write("sampleID\t" + "\t".join(f"v{k}" for k in range(60)) + "\n")
        for s in range(40):
            fh.write(f"msp_{s}\t" + "\t".join(str(max(int(v), 0)) for v in ct[:60, s]) + "\n")
    assert LD.main(["--matrix", str(tmp_path / "m.txt"), "--out", out + "m", "--r2", "0.3", "--host", "--silence"]) == 0
    rows = [line.split("\t") for line in open(out + "m_ld_sites.txt").read().splitlines()][1:]
    assert {(r[1], r[2]) for r in rows} == {(".", "NA")} and json.load(open(out + "m_ld_summary.json"))["window_bp"] is None


def test_max_snps_sites_are_compared_in_input_order(tmp_path):
    from locator_amd import genotypes as G
    out = str(tmp_path / "o")
    assert LD.main(["--vcf", U.VCF, "--out", out, "--r2", "0.2", "--ld_window", "10", "--max_SNPs", "300", "--seed", "7", "--host",
                    "--silence", "--keep_matrix"]) == 0
    gt = G.read_vcf(U.VCF)["calldata/GT"]
    np.random.seed(7)
    _, idx = G.filter_snps(gt, min_mac=2, max_snps=300, verbose=False, sites=True)
    assert (np.diff(idx) < 0).any()                                           # the draw is not in order ...
    assert np.array_equal(np.load(out + "_ld.npz")["sites"], np.sort(idx))    # ... the windows are


# ------------------------------------------------------------------ --ld_prune
def test_neighbors_with_ld_prune(tmp_path):
    out = str(tmp_path / "o")
    assert NB.main(["--vcf", U.VCF, "--sample_data", U.SAMPLE_DATA, "--out", out, "--min_mac", "2", "--host", "--silence",
                    "--ld_prune", "0.2", "--kmax", "8"]) == 0
    s = json.load(open(out + "_knn_summary.json"))
    assert s["K"] == 1996 and s["N"] == 500
    assert list(s)[-4:] == ["ld_prune", "ld_window", "ld_window_bp", "K_before_prune"]
    assert (s["ld_prune"], s["ld_window"], s["ld_window_bp"], s["K_before_prune"]) == (0.2, 100, None, 5830)


def test_pruned_sites_keep_the_order_of_the_draw():
    from locator_amd import genotypes as G
    vcf = G.read_vcf(U.VCF, sites=True)
    gt = vcf["calldata/GT"]
    np.random.seed(3)
    _, idx = G.filter_snps(gt, min_mac=2, max_snps=500, verbose=False, sites=True)
    kept = LD.prune_sites(gt, idx, vcf["variants/CHROM"], vcf["variants/POS"], 0.2, 50, None, True)
    assert (np.diff(kept) > 0).all() and set(kept) < set(idx.tolist()) and 0 < len(kept) < 500
    ct, _ = BL.count_matrix_sites(gt, np.sort(idx))
    want = np.sort(idx)[LD.greedy_host(LD.band_host(ct, 50, LD.reach_host(500, 50), 0.2)[0])[0]]
    assert np.array_equal(kept, want)


def test_neighbors_without_the_flag_writes_what_it_wrote(tmp_path):
    """The files of a run without --ld_prune against a run of the command's functions as they were before the option existed:
    the readers, filter_snps, count_matrix and NB.neighbors called directly, no prelude, no new argument."""
    from locator_amd import genotypes as G
    vcf = U.VCF
    out_cmd, out_fn = str(tmp_path / "cmd"), str(tmp_path / "fn")
    assert NB.main(["--vcf", vcf, "--sample_data", U.SAMPLE_DATA, "--out", out_cmd, "--host", "--silence", "--close", "0",
                    "--keep_matrix", "--max_SNPs", "400", "--seed", "11"]) == 0
    np.random.seed(11)
    data = G.read_vcf(vcf)
    gt, samples = data["calldata/GT"], data["samples"]
    locs = BL.read_locations(U.SAMPLE_DATA, samples, NB.PROG)
    _, idx = G.filter_snps(gt, min_mac=2, max_snps=400, verbose=False, sites=True)
    c, P = BL.count_matrix(gt, idx)
    NB.neighbors(c, P, samples, locs, out_fn, "auto", 32, False, 0.0, True, True, True)
    for name in ("_knn_locs.txt", "_neighbors.txt", "_knn_summary.json", "_close_pairs.txt", "_ibs.npz"):
        assert open(out_cmd + name, "rb").read() == open(out_fn + name, "rb").read(), name
    s = json.load(open(out_cmd + "_knn_summary.json"))
    assert tuple(s) == NB.SUMMARY_KEYS + ("close", "n_close_pairs") and s["K"] == 400


# ------------------------------------------------------------------ stops and errors
def test_without_a_gpu_the_command_stops_unless_host(tmp_path, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match="no GPU visible.*loc_ld_band.*--host"):
        LD.main(["--vcf", U.VCF, "--out", str(tmp_path / "o"), "--r2", "0.2"])
    with pytest.raises(SystemExit, match="no GPU visible"):
        NB.main(["--vcf", U.VCF, "--sample_data", U.SAMPLE_DATA, "--out", str(tmp_path / "o"), "--ld_prune", "0.2"])
    assert not os.listdir(tmp_path)


def test_refusals(tmp_path, capsys):
    base = ["--out", str(tmp_path / "o"), "--host", "--silence"]
    for extra, text in (([], "the following arguments are required: --r2"),
                        (["--vcf", U.VCF], "the following arguments are required: --r2"),
                        (["--r2", "0.2"], "exactly one of --vcf / --zarr / --matrix"),
                        (["--vcf", U.VCF, "--r2", "nan"], "--r2 must be"),
                        (["--vcf", U.VCF, "--r2", "0.2", "--ld_window", "0"], f"--ld_window must be 1 .. {LD.MAX_WINDOW}"),
                        (["--vcf", U.VCF, "--r2", "0.2", "--ld_window", str(LD.MAX_WINDOW + 1)], "--ld_window must be 1 .."),
                        (["--vcf", U.VCF, "--r2", "0.2", "--ld_window_bp", "-1"], "--ld_window_bp must be"),
                        (["--matrix", "m.txt", "--r2", "0.2", "--ld_window_bp", "1000"], "a --matrix has none"),
                        (["--vcf", U.VCF, "--r2", "0.2", "--ld_prune", "0.2"], "unrecognized arguments")):
        with pytest.raises(SystemExit) as e:
            LD.main(base + extra)
        assert e.value.code == 2 and text in capsys.readouterr().err, extra
    nb = ["--vcf", U.VCF, "--sample_data", U.SAMPLE_DATA] + base
    for extra, text in ((["--ld_prune", "0.2", "--ld_window", "0"], "--ld_window must be"),
                        (["--ld_prune", "inf"], "--ld_prune must be"),
                        (["--ld_prune"], "expected one argument")):
        with pytest.raises(SystemExit) as e:
            NB.main(nb + extra)
        assert e.value.code == 2 and text in capsys.readouterr().err, extra
    with pytest.raises(SystemExit) as e:
        NB.main(["--matrix", "m.txt", "--sample_data", U.SAMPLE_DATA] + base + ["--ld_prune", "0.2", "--ld_window_bp", "5"])
    assert e.value.code == 2 and "a --matrix has none" in capsys.readouterr().err
    assert not os.listdir(tmp_path)
    with pytest.raises(ValueError, match="must be 1 .."):
        LD.sums_host(np.zeros((3, 4), dtype=np.int8), 0)
    with pytest.raises(ValueError, match="a count of 3"):
        LD.sums_host(np.full((3, 4), 3, dtype=np.int8), 2)
    with pytest.raises(ValueError, match="fewer than 2\\^20 samples"):
        LD.check_sites(np.lib.stride_tricks.as_strided(np.zeros(1, dtype=np.int8), (1, 2 ** 20), (0, 0)), 2)
