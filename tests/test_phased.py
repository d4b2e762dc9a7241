"""--phased on the host: one matrix row per haplotype (row 2s + h = allele h of individual s), the individual-level split,
haploid imputation and jacknife draws, the refusals, params.json and the replicate summaries of haplotype rows.  Nothing
here needs a GPU; tests/test_gpu_phased.py runs the same path on the device."""
import json
import os

import numpy as np
import pandas as pd
import pytest

from locator_amd import genotypes as G
from locator_amd import locator as L

GOLD = os.path.join(os.path.dirname(__file__), "golden")
VCF = os.path.join(GOLD, "test_genotypes.vcf.gz")
SAMPLES = os.path.join(GOLD, "test_sample_data.txt")


@pytest.fixture(scope="module")
def fixture_vcf():
    return G.read_vcf(VCF)


def _naive_haplotypes(gt, min_mac):
    """The filters written out site by site (biallelic, allele-1 count >= min_mac unless 1), then H[k][2s + h] = 1 where
    allele h of individual s is 1 - missing alleles count 0."""
    V, N, _ = gt.shape
    keep = np.zeros(V, bool)
    for v in range(V):
        called = gt[v][gt[v] >= 0]
        keep[v] = len(np.unique(called)) == 2 and (min_mac == 1 or int((called == 1).sum()) >= min_mac)
    kept = gt[keep]
    H = np.zeros((len(kept), 2 * N), np.int8)
    for s in range(N):
        for h in (0, 1):
            H[:, 2 * s + h] = kept[:, s, h] == 1
    return H, keep


def _setup(tmp_path, name, *extra):
    np.random.seed(None)
    return L._setup(["--vcf", VCF, "--sample_data", SAMPLES, "--out", str(tmp_path / name), "--seed", "12345"]
                    + list(extra))


# ------------------------------------------------------------------ the haplotype matrix
@pytest.mark.parametrize("missing", [0.0, 0.03])
def test_haplotype_matrix_equals_the_naive_rows_with_the_diploid_sites(fixture_vcf, missing):
    gt = np.array(fixture_vcf["calldata/GT"], dtype=np.int8)
    if missing:
        gt[np.random.default_rng(5).random(gt.shape) < missing] = -1
    H, keep = _naive_haplotypes(gt, 2)
    got = G.filter_snps(G.haplotypes(gt), min_mac=2, verbose=False)
    diploid = G.filter_snps(gt, min_mac=2, verbose=False)
    assert got.shape == H.shape == (diploid.shape[0], 2 * gt.shape[1])
    assert np.array_equal(got, H)
    assert np.array_equal(got[:, 0::2] + got[:, 1::2], diploid)           # the two haplotypes add up to the count
    # the NumPy restatement (the --impute_missing path's filters) gives the same rows
    assert np.array_equal(G.filter_snps(G.haplotypes(gt), min_mac=2, verbose=False, native=False), H)
    if not missing:
        assert H.shape[0] == 5830


def test_cli_prologue_builds_the_haplotype_matrix(tmp_path, fixture_vcf):
    _setup(tmp_path, "p", "--phased")
    samples, state = L._prologue()
    H, _ = _naive_haplotypes(fixture_vcf["calldata/GT"], 2)
    assert np.array_equal(state[4], H)
    ids = L.row_ids(samples)
    assert list(ids[:4]) == ["msp_0_h0", "msp_0_h1", "msp_1_h0", "msp_1_h1"] and len(ids) == 1000


# ------------------------------------------------------------------ the split
def test_split_is_by_individual_and_equals_the_diploid_draw(tmp_path):
    _setup(tmp_path, "d")
    _, d = L._prologue()
    _setup(tmp_path, "p", "--phased")
    _, p = L._prologue()
    (mld, sld, mad, sad, _, trd, ted, tgd, vgd, tld, vld, prd, pgd) = d
    (mlp, slp, map_, sap, _, trp, tep, tgp, vgp, tlp, vlp, prp, pgp) = p
    assert (mld, sld, mad, sad) == (mlp, slp, map_, sap)                  # same means and SDs, exactly
    for dip, hap in ((trd, trp), (ted, tep), (prd, prp)):
        assert np.array_equal(hap, L.haplotype_rows(dip))                # each individual -> rows 2s, 2s + 1
        assert np.array_equal(hap[0::2] // 2, hap[1::2] // 2)
    assert list(ted[:10]) == [465, 459, 233, 149, 429, 423, 454, 140, 489, 165]    # the --seed 12345 draw
    assert np.array_equal(prp, np.arange(100))                            # msp_0..msp_49 have NA coordinates
    assert len(set(trp) | set(tep) | set(prp)) == 1000 and (len(trp), len(tep)) == (810, 90)
    assert np.array_equal(tlp, np.repeat(tld, 2, axis=0)) and np.array_equal(vlp, np.repeat(vld, 2, axis=0))
    assert tgp.shape == (810, 5830) and pgp.shape == (100, 5830) and set(np.unique(tgp)) <= {0, 1}
    assert np.array_equal(tgp[0::2] + tgp[1::2], tgd)


def test_window_units_split_by_individual(tmp_path, fixture_vcf):
    store = str(tmp_path / "fix.zarr")
    G.write_callset_zarr(store, fixture_vcf["calldata/GT"], fixture_vcf["variants/POS"], fixture_vcf["samples"],
                         chunk_variants=4096)
    units = {}
    for name, extra in (("d", []), ("p", ["--phased"])):
        np.random.seed(None)
        L._setup(["--zarr", store, "--sample_data", SAMPLES, "--out", str(tmp_path / name), "--seed", "12345", "--windows",
                  "--window_size", "1250000"] + extra)
        samples, state = L._prologue()
        units[name] = L._window_units(samples)
    assert len(units["p"]) == len(units["d"]) == 2
    for ud, up in zip(units["d"], units["p"]):
        assert up["phased"] and "phased" not in ud
        for k in ("train", "test", "pred"):
            assert np.array_equal(up[k], L.haplotype_rows(ud[k]))
        assert np.array_equal(up["locs"], np.repeat(ud["locs"], 2, axis=0), equal_nan=True) and up["samples"][1] == "msp_0_h1"
        # the host half of a lazy window: the window's calls viewed as (V, 2N, 1)
        L._load_window(up)
        L._load_window(ud)
        assert np.array_equal(up["traingen"][0::2] + up["traingen"][1::2], ud["traingen"])
        assert up["predgen"].shape == (100, ud["predgen"].shape[1])


# ------------------------------------------------------------------ imputation and jacknife draws
def _old_replace_md(gt, rng):
    """genotypes.replace_md as it was before --phased (P = 2 written in)."""
    dc = G.count_alleles(gt, max(int(gt.max()), 1))[:, 1]
    ac = G.to_allele_counts_1(gt)
    miss = G.is_missing(gt)
    with np.errstate(divide="ignore", invalid="ignore"):
        af = dc / (2 * (~miss).sum(axis=1))
    for i, j in np.argwhere(miss):
        ac[i, j] = rng.binomial(2, af[i])
    return ac


def test_haploid_imputation_draws_binomial_1_in_site_then_row_order():
    rng = np.random.default_rng(11)
    gt = (rng.random((40, 30, 2)) < rng.uniform(0.1, 0.9, (40, 1, 1))).astype(np.int8)
    gt[rng.random(gt.shape) < 0.1] = -1
    hv = G.haplotypes(gt)
    np.random.seed(7)
    got = G.replace_md(hv)
    tail = np.random.random_sample()
    np.random.seed(7)
    want = (hv[:, :, 0] == 1).astype(np.int8)
    for i in range(hv.shape[0]):
        called = hv[i, :, 0] >= 0
        af = (hv[i, :, 0] == 1).sum() / called.sum()
        for j in range(hv.shape[1]):
            if not called[j]:
                want[i, j] = np.random.binomial(1, af)
    assert np.array_equal(got, want) and set(np.unique(got)) <= {0, 1}
    assert np.random.random_sample() == tail
    assert (got[hv[:, :, 0] < 0] == 1).any() and (got[hv[:, :, 0] < 0] == 0).any()
    # P = 2: the same values and stream as before (few missing alleles: the diploid frequency counts allele-1 copies of
    # half-missing calls over whole calls and can pass 1 where most calls are missing - the reference's arithmetic)
    g2 = (rng.random((40, 30, 2)) < rng.uniform(0.1, 0.8, (40, 1, 1))).astype(np.int8)
    g2[rng.random(g2.shape) < 0.02] = -1
    np.random.seed(3)
    a = G.replace_md(g2.copy())
    ta = np.random.random_sample()
    np.random.seed(3)
    b = _old_replace_md(g2.copy(), np.random)
    assert np.array_equal(a, b) and np.random.random_sample() == ta
    # and through filter_snps --impute_missing on the haplotype view
    np.random.seed(1)
    ac = G.filter_snps(hv, min_mac=1, impute_missing=True, verbose=False)
    assert set(np.unique(ac)) <= {0, 1} and ac.shape[1] == 60


def test_jacknife_draws_at_ploidy_1_and_the_unchanged_default_stream():
    rs = np.random.RandomState(4)
    predgen = rs.randint(0, 2, (12, 500)).astype(np.uint8)
    af = rs.uniform(0.01, 0.99, 500)
    np.random.seed(99)
    hap = L.jacknife_draws(predgen, af, 3, 0.1, ploidy=1)
    t1 = np.random.random_sample()
    np.random.seed(99)
    ref = []
    for _ in range(3):
        sites = np.random.choice(500, 50, replace=False)
        ref.append((sites, np.array([np.random.binomial(1, af[i], 12) for i in sites])))
    assert np.random.random_sample() == t1
    for (s, v), (rs_, rv) in zip(hap, ref):
        assert np.array_equal(s, rs_) and np.array_equal(v, rv) and set(np.unique(v)) <= {0, 1}
    np.random.seed(99)
    dflt = L.jacknife_draws(predgen, af, 3, 0.1)
    t2 = np.random.random_sample()
    np.random.seed(99)
    two = L.jacknife_draws(predgen, af, 3, 0.1, ploidy=2)
    assert np.random.random_sample() == t2
    assert all(np.array_equal(a[1], b[1]) for a, b in zip(dflt, two)) and max(v.max() for _, v in dflt) == 2


# ------------------------------------------------------------------ refusals
@pytest.fixture
def no_device(monkeypatch):
    """Fail the test if anything would start a worker or touch the HIP library."""
    from locator_amd import _lib
    from locator_amd import replicates as R

    def boom(*a, **k):
        raise AssertionError("a device or worker was started")
    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(L, "_fit_unit", boom)
    monkeypatch.setattr(R, "ReplicatePool", boom)


def test_phased_with_a_count_matrix_is_refused(tmp_path, no_device):
    mat = tmp_path / "m.txt"
    pd.DataFrame({"sampleID": ["a", "b"], "s0": [0, 1]}).to_csv(mat, sep="\t", index=False)
    with pytest.raises(SystemExit, match="carries no phase"):
        L.main(["--matrix", str(mat), "--sample_data", SAMPLES, "--out", str(tmp_path / "m"), "--phased"])
    with pytest.raises(SystemExit, match="carries no phase"):
        L.main(["--matrix", str(mat), "--sample_data", SAMPLES, "--out", str(tmp_path / "m"), "--phased", "--bootstrap",
                "--in_process"])


def _write_vcf(path, calls):
    lines = ["##fileformat=VCFv4.2", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(
        f"i{j}" for j in range(len(calls[0])))]
    for v, row in enumerate(calls):
        lines.append(f"1\t{100 * (v + 1)}\t.\tA\tT\t.\tPASS\t.\tGT\t" + "\t".join(row))
    path.write_text("\n".join(lines) + "\n")


def test_unphased_heterozygous_vcf_calls_are_refused_and_counted(tmp_path, no_device):
    sd = tmp_path / "s.txt"
    pd.DataFrame({"sampleID": ["i0", "i1", "i2"], "x": [1.0, 2.0, np.nan], "y": [1.0, 2.0, np.nan]}).to_csv(
        sd, sep="\t", index=False)
    vcf = tmp_path / "u.vcf"
    _write_vcf(vcf, [["0|1", "1|1", "0|0"], ["0/1", "1/1", "0/0"], ["1|0", "0|.", "0/."]])
    r = G.read_vcf(str(vcf), phase=True)
    assert r["unphased_hets"] == 1 and "unphased_hets" not in G.read_vcf(str(vcf))
    with pytest.raises(SystemExit, match=r"has 1 heterozygous call\(s\) without phase"):
        L.main(["--vcf", str(vcf), "--sample_data", str(sd), "--out", str(tmp_path / "u"), "--phased"])
    # the slow parser (FORMAT with more keys) reports the same
    slow = tmp_path / "slow.vcf"
    _write_vcf(slow, [["0/1:3", "1/0:4", "0|1:5"]])
    slow.write_text(slow.read_text().replace("\tGT\t", "\tGT:DP\t"))
    assert G.read_vcf(str(slow), phase=True)["unphased_hets"] == 2
    # phased, homozygous-unphased and haploid calls pass
    ok = tmp_path / "ok.vcf"
    _write_vcf(ok, [["0|1", "1/1", "0"], ["1|0", "0/0", "1"]])
    assert G.read_vcf(str(ok), phase=True)["unphased_hets"] == 0
    assert G.read_vcf(VCF, phase=True)["unphased_hets"] == 0


def test_zarr_gt_phased_flags_are_checked_when_present(tmp_path, no_device):
    gt = np.array([[[0, 1], [1, 1], [0, 0]], [[1, 0], [0, 1], [0, 0]]], np.int8)
    store = str(tmp_path / "z.zarr")
    G.write_callset_zarr(store, gt, [100, 200], ["i0", "i1", "i2"])
    assert G.zarr_unphased_hets(G.open_group(store)) is None                # no flags: taken as it is
    flags = np.ones((2, 3), bool)
    flags[1, 1] = False                                                    # a heterozygote without phase
    flags[0, 2] = False                                                    # a homozygote: no matter
    G.write_zarr_array(os.path.join(store, "calldata", "GT_phased"), flags, (1, 3))
    assert G.zarr_unphased_hets(G.open_group(store)) == 1
    sd = tmp_path / "s.txt"
    pd.DataFrame({"sampleID": ["i0", "i1", "i2"], "x": [1.0, 2.0, np.nan], "y": [1.0, 2.0, np.nan]}).to_csv(
        sd, sep="\t", index=False)
    with pytest.raises(SystemExit, match="GT_phased has 1 heterozygous"):
        L.main(["--zarr", store, "--sample_data", str(sd), "--out", str(tmp_path / "z"), "--phased"])


# ------------------------------------------------------------------ params.json
def test_params_json_has_no_phased_key_without_the_flag(tmp_path):
    out = str(tmp_path / "a")
    a = L._setup(["--vcf", "x.vcf", "--sample_data", "s.txt", "--out", out, "--seed", "1"])
    raw = open(out + "_params.json").read()
    js = json.loads(raw)
    assert "phased" not in js and not L._phased(a)
    assert list(js) == list(vars(L.build_parser().parse_args([])))
    assert raw == json.dumps({k: v for k, v in vars(a).items() if k != "_net_seed"}, indent=2)
    b = L._setup(["--vcf", "x.vcf", "--sample_data", "s.txt", "--out", str(tmp_path / "b"), "--phased"])
    jb = json.load(open(str(tmp_path / "b") + "_params.json"))
    assert jb["phased"] is True and list(jb)[-1] == "phased" and L._phased(b)
    # --load_params: a file without the key (an older run) stays unphased; one with it restores it
    assert not L._phased(L._setup(["--load_params", out + "_params.json"]))
    assert L._phased(L._setup(["--load_params", str(tmp_path / "b") + "_params.json"]))


# ------------------------------------------------------------------ summaries
def test_summaries_of_haplotype_rows_use_the_individuals_truth(tmp_path, capsys):
    from locator_amd import summarize as S
    sd = pd.read_csv(SAMPLES, sep="\t").set_index("sampleID")
    ids = ["msp_60", "msp_61"]
    rng = np.random.default_rng(0)
    d = tmp_path / "runs"
    d.mkdir()
    for b in range(6):
        rows = [(sd.loc[i, "x"] + rng.normal(0, 0.5), sd.loc[i, "y"] + rng.normal(0, 0.5), f"{i}_h{h}")
                for i in ids for h in (0, 1)]
        pd.DataFrame(rows, columns=["x", "y", "sampleID"]).to_csv(d / f"p_boot{b}_predlocs.txt", index=False)
    bp = S.summarize(str(d), SAMPLES, str(tmp_path / "o"), host=True)
    assert list(bp["sampleID"]) == ["msp_60_h0", "msp_60_h1", "msp_61_h0", "msp_61_h1"]
    assert np.allclose(bp["x"], np.repeat(sd.loc[ids, "x"].to_numpy(), 2))
    assert np.allclose(bp["y"], np.repeat(sd.loc[ids, "y"].to_numpy(), 2))
    txt = capsys.readouterr().out
    assert "mean centroid error" in txt and "mean kernel peak error" in txt
