"""Kept models on new genotypes, host side: the site identities the readers return, the model file (--keep_model) and its
round trip without pickle, the matching rules, the refusals, the --impute_missing draws, and query_rows_numpy - the NumPy
restatement of loc_query_rows that tests/test_gpu_query.py holds the kernel to.  Nothing here needs a GPU."""
import json
import os
import struct

import numpy as np
import pytest

from locator_amd import genotypes as G
from locator_amd import locator as L
from locator_amd import query as Q

GOLD = os.path.join(os.path.dirname(__file__), "golden")
VCF = os.path.join(GOLD, "test_genotypes.vcf.gz")


def query_rows_numpy(gt, col_variant, col_allele, sample_order, width=None):
    """loc_query_rows restated: X[r][k] = copies of allele col_allele[k] among the alleles of sample sample_order[r] at
    variant col_variant[k] (missing alleles count nothing); an absent column (-1) is 0; columns K .. width stay 0."""
    gt = np.asarray(gt)
    K = len(col_variant)
    X = np.zeros((len(sample_order), K if width is None else width), np.uint8)
    order = np.asarray(sample_order, dtype=np.int64)
    for k in range(K):
        v = int(col_variant[k])
        if v >= 0:
            X[:, k] = (gt[v][order] == int(col_allele[k])).sum(axis=1)
    return X


def _model(chrom, pos, ref, alt, K=None, ploidy=2, phased=False):
    K = len(chrom) if K is None else K
    return {"path": "m.model.npz", "stem": "m", "chrom": np.array(chrom, str), "pos": np.array(pos, np.int64),
            "ref": np.array(ref, str), "alt": np.array(alt, str), "af": np.full(K, 0.5), "ploidy": ploidy, "phased": phased}


def _query(chrom, pos, alleles, n=3, P=2):
    return {"kind": "vcf", "chrom": np.array(chrom, str), "pos": np.array(pos, np.int64), "alleles": alleles,
            "gt": np.zeros((len(chrom), n, P), np.int8), "samples": np.array([f"s{i}" for i in range(n)]),
            "unphased_hets": 0}


# ------------------------------------------------------------------ readers
def test_read_vcf_sites_and_unchanged_default():
    plain = G.read_vcf(VCF)
    full = G.read_vcf(VCF, sites=True)
    assert set(plain) == {"calldata/GT", "samples", "variants/POS"}
    for k in plain:
        assert np.array_equal(plain[k], full[k])
    V = plain["calldata/GT"].shape[0]
    assert full["variants/CHROM"].shape == (V,) and set(full["variants/CHROM"]) == {"1"}
    assert full["variants/REF"][0] == "A" and full["variants/ALT"].shape == (V, 1) and full["variants/ALT"][0, 0] == "T"


def test_read_vcf_multiallelic_alt_table(tmp_path):
    p = tmp_path / "m.vcf"
    p.write_text("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ta\tb\n"
                 "2\t10\t.\tC\tG,T\t.\t.\t.\tGT\t0|2\t1|1\n3\t11\t.\tA\t.\t.\t.\t.\tGT\t0|0\t0|0\n")
    d = G.read_vcf(str(p), sites=True)
    assert list(d["variants/CHROM"]) == ["2", "3"] and list(d["variants/REF"]) == ["C", "A"]
    assert d["variants/ALT"].tolist() == [["G", "T"], ["", ""]]
    assert d["calldata/GT"][0].tolist() == [[0, 2], [1, 1]]


@pytest.mark.parametrize("compressor", [None, "zlib", "blosc"])
def test_zarr_fixed_width_string_sites(tmp_path, compressor):
    gt = np.zeros((5, 2, 2), np.int8)
    alt = np.array([["T", ""], ["G", "C"], ["A", ""], ["TT", ""], ["C", ""]])
    G.write_callset_zarr(str(tmp_path / "z"), gt, [1, 2, 3, 4, 5], ["a", "b"], chunk_variants=2, compressor=compressor,
                         chrom=["1", "1", "2", "2", "X"], ref=list("ACGTA"), alt=alt)
    d = G.zarr_sites(G.open_group(str(tmp_path / "z")))
    assert d["variants/CHROM"].tolist() == ["1", "1", "2", "2", "X"]
    assert d["variants/POS"].tolist() == [1, 2, 3, 4, 5] and d["variants/REF"].tolist() == list("ACGTA")
    assert d["variants/ALT"].tolist() == alt.tolist()


def test_zarr_vlen_utf8_sites(tmp_path):
    root = tmp_path / "z"
    G.write_callset_zarr(str(root), np.zeros((3, 2, 2), np.int8), [5, 6, 7], ["a", "b"])
    for name, vals in (("CHROM", ["chr1", "chr1", "chr2"]), ("REF", ["A", "C", "G"]), ("ALT", ["T", "G", "C"])):
        d = root / "variants" / name
        d.mkdir()
        (d / ".zarray").write_text(json.dumps({"zarr_format": 2, "shape": [3], "chunks": [3], "dtype": "|O",
                                               "compressor": None, "fill_value": None, "order": "C",
                                               "filters": [{"id": "vlen-utf8"}]}))
        raw = struct.pack("<I", 3) + b"".join(struct.pack("<I", len(v)) + v.encode() for v in vals)
        (d / "0").write_bytes(raw)
    d = G.zarr_sites(G.open_group(str(root)))
    assert d["variants/CHROM"].tolist() == ["chr1", "chr1", "chr2"] and d["variants/ALT"].tolist() == [["T"], ["G"], ["C"]]


def test_zarr_without_sites_names_the_missing_array(tmp_path):
    G.write_callset_zarr(str(tmp_path / "z"), np.zeros((2, 2, 2), np.int8), [1, 2], ["a", "b"])
    with pytest.raises(KeyError, match="variants/CHROM"):
        G.zarr_sites(G.open_group(str(tmp_path / "z")))


def test_filter_snps_sites_draws_nothing_more():
    gt = G.read_vcf(VCF)["calldata/GT"]
    for kw in ({}, {"max_snps": 300}, {"impute_missing": True, "max_snps": 100}, {"native": False}):
        np.random.seed(7)
        ac = G.filter_snps(gt, verbose=False, **kw)
        after = np.random.get_state()[1].copy()
        np.random.seed(7)
        ac2, idx = G.filter_snps(gt, verbose=False, sites=True, **kw)
        assert np.array_equal(np.random.get_state()[1], after) and np.array_equal(ac, ac2)
        if not kw.get("impute_missing"):
            assert np.array_equal(G.to_allele_counts_1(gt[idx]), ac)


def test_site_af():
    gt = np.array([[[0, 1], [1, -1]], [[1, 1], [0, 0]]], np.int8)
    assert np.allclose(G.site_af(gt, [1, 0, 0]), [0.5, 2 / 3, 2 / 3])


# ------------------------------------------------------------------ the model file
def _weights(K=7, H=4, L_=2, rng=None):
    rng = rng or np.random.default_rng(0)
    W = [rng.normal(size=(K, H)).astype(np.float32)] + [rng.normal(size=(H, H)).astype(np.float32) for _ in range(L_ - 1)]
    W += [rng.normal(size=(H, 2)).astype(np.float32), rng.normal(size=(2, 2)).astype(np.float32)]
    b = [rng.normal(size=w.shape[1]).astype(np.float32) for w in W]
    f = lambda: rng.normal(size=K).astype(np.float32)
    return {"W": W, "b": b, "gamma": f(), "beta": f(), "mov_mean": f(), "mov_var": np.abs(f())}


def test_model_file_round_trip_without_pickle(tmp_path):
    w = _weights()
    meta = {"chrom": np.array(["1", "1", "2", "2", "X", "1", "1"], dtype=object), "pos": np.arange(7) * 10,
            "ref": np.array(list("ACGTACG"), dtype=object), "alt": np.array(list("TTTAGGA"), dtype=object),
            "af": np.linspace(0.1, 0.7, 7), "locs_norm": [1.5, 2.5, -3.5, 4.5], "ploidy": 2, "phased": False,
            "params_json": json.dumps({"width": 4, "nlayers": 2, "dropout_prop": 0.25}, indent=2)}
    path = str(tmp_path / "run.model.npz")
    L.save_model(path, w, meta)
    with np.load(path, allow_pickle=False) as z:
        for k in ("site_chrom", "site_ref", "site_alt"):
            assert z[k].dtype.kind == "U"
        assert int(z["format_version"]) == 1
    m = Q.load_model(path)
    assert m["stem"] == "run" and m["K"] == 7 and (m["width"], m["nlayers"]) == (4, 2)
    assert m["chrom"].tolist() == meta["chrom"].tolist() and m["pos"].tolist() == meta["pos"].tolist()
    assert m["alt"].tolist() == list("TTTAGGA") and np.array_equal(m["af"], meta["af"])
    assert m["locs_norm"] == [1.5, 2.5, -3.5, 4.5] and m["ploidy"] == 2 and m["phased"] is False
    assert m["params"]["dropout_prop"] == 0.25
    back = L.read_weights(path)                    # --load_weights takes a model file unchanged
    for k in ("gamma", "beta", "mov_mean", "mov_var"):
        assert np.array_equal(back[k], w[k])
    for a, b in zip(back["W"] + back["b"], w["W"] + w["b"]):
        assert np.array_equal(a, b)
    # the weights file is unchanged by the model file's existence: same arrays, nothing more
    L.save_weights(str(tmp_path / "run.weights.npz"), w)
    with np.load(str(tmp_path / "run.weights.npz"), allow_pickle=False) as zw, np.load(path, allow_pickle=False) as zm:
        assert set(zw.files) < set(zm.files)
        assert all(np.array_equal(zw[k], zm[k]) for k in zw.files)


def test_model_file_rejects_a_site_table_of_the_wrong_length(tmp_path):
    meta = {"chrom": ["1"], "pos": [1], "ref": ["A"], "alt": ["T"], "af": [0.5], "locs_norm": [0, 1, 0, 1], "ploidy": 2,
            "phased": False, "params_json": "{}"}
    with pytest.raises(ValueError, match="site_chrom"):
        L.save_model(str(tmp_path / "x.model.npz"), _weights(), meta)


def test_weights_file_is_refused(tmp_path):
    L.save_weights(str(tmp_path / "a.weights.npz"), _weights())
    with pytest.raises(SystemExit, match="no site table"):
        Q.load_model(str(tmp_path / "a.weights.npz"))


def test_keep_model_flag_absent_unless_given():
    p = L.build_parser()
    assert not hasattr(p.parse_args([]), "keep_model")
    assert p.parse_args(["--keep_model"]).keep_model is True


def test_model_paths_directory(tmp_path):
    for n in ("b_boot1.model.npz", "b_bootFULL.model.npz", "b_boot0.model.npz", "b_boot0.weights.npz", "x.txt"):
        (tmp_path / n).write_bytes(b"")
    got = [os.path.basename(p) for p in Q.model_paths([str(tmp_path)])]
    assert got == ["b_boot0.model.npz", "b_boot1.model.npz", "b_bootFULL.model.npz"]
    assert Q.model_stem("/a/b_boot0.model.npz") == "b_boot0"


# ------------------------------------------------------------------ matching
def test_match_ref_alt_swap_gives_allele_0():
    cv, ca, rep = Q.match_sites(_model(["1"], [100], ["A"], ["T"]), _query(["1"], [100], [["T", "A"]]))
    assert cv.tolist() == [0] and ca.tolist() == [0] and rep["allele_not_1"] == 1 and rep["absent"] == 0


def test_match_model_alt_as_second_query_alt_gives_allele_2():
    cv, ca, _ = Q.match_sites(_model(["1"], [100], ["A"], ["T"]), _query(["1"], [100], [["A", "G", "T"]]))
    assert cv.tolist() == [0] and ca.tolist() == [2]
    # a multi-allelic query record that holds neither of the model's alleles in full does not match
    cv, _, _ = Q.match_sites(_model(["1"], [100], ["A"], ["T"]), _query(["1"], [100], [["C", "G", "T"]]))
    assert cv.tolist() == [-1]


def test_match_duplicate_records_first_wins():
    q = _query(["1", "1", "1"], [50, 100, 100], [["A", "T"], ["A", "T"], ["T", "A"]])
    cv, ca, _ = Q.match_sites(_model(["1"], [100], ["A"], ["T"]), q)
    assert cv.tolist() == [1] and ca.tolist() == [1]
    q = _query(["1", "1", "1"], [100, 100, 100], [["G", "C"], ["T", "A"], ["A", "T"]])     # first record that MATCHES
    cv, ca, _ = Q.match_sites(_model(["1"], [100], ["A"], ["T"]), q)
    assert cv.tolist() == [1] and ca.tolist() == [0]


def test_match_other_chrom_same_pos_is_absent():
    m = _model(["1", "2", "2"], [100, 100, 200], ["A", "A", "C"], ["T", "T", "G"])
    q = _query(["2", "3"], [200, 100], [["C", "G"], ["A", "T"]])
    cv, ca, rep = Q.match_sites(m, q)
    assert cv.tolist() == [-1, -1, 0] and ca.tolist()[2] == 1
    assert rep == {"model": "m", "K": 3, "matched": 1, "allele_not_1": 0, "absent": 2}


def test_match_repeated_model_sites():
    m = _model(["1", "1", "1"], [7, 9, 7], ["A", "C", "A"], ["T", "G", "T"])      # a bootstrap replicate repeats sites
    cv, ca, _ = Q.match_sites(m, _query(["1", "1"], [9, 7], [["C", "G"], ["A", "T"]]))
    assert cv.tolist() == [1, 0, 1] and ca.tolist() == [1, 1, 1]


def test_match_matrix_headers(tmp_path):
    p = tmp_path / "q.txt"
    p.write_text("sampleID\tsnpB\tsnpA\tsnpB\nq1\t0\t1\t2\nq2\t2\t2\t0\n")
    q = Q.read_query(matrix=str(p))
    assert q["names"].tolist() == ["snpB", "snpA", "snpB"]
    m = _model(["snpA", "snpB", "snpC"], [-1] * 3, [""] * 3, [""] * 3)
    cv, ca, rep = Q.match_sites(m, q)
    assert cv.tolist() == [1, 0, -1] and ca.tolist() == [1, 1, 0] and rep["absent"] == 1
    X = query_rows_numpy(q["gt"], cv, ca, [0, 1])
    assert X.tolist() == [[1, 0, 0], [2, 2, 0]]


# ------------------------------------------------------------------ refusals
def test_refuse_low_overlap():
    m = _model(["1"] * 4, [1, 2, 3, 4], ["A"] * 4, ["T"] * 4)
    q = _query(["1", "1"], [1, 2], [["A", "T"], ["A", "T"]])
    _, _, rep = Q.match_sites(m, q)
    Q.check_query(m, q, rep, 0.5)
    with pytest.raises(SystemExit, match="min_site_overlap"):
        Q.check_query(m, q, rep, 0.75)


def test_refuse_other_ploidy():
    m = _model(["1"], [1], ["A"], ["T"])
    q = _query(["1"], [1], [["A", "T"]], P=1)
    _, _, rep = Q.match_sites(m, q)
    with pytest.raises(SystemExit, match="ploidy"):
        Q.check_query(m, q, rep)


def test_refuse_unphased_query_for_phased_model(tmp_path):
    m = _model(["1"], [1], ["A"], ["T"], phased=True)
    p = tmp_path / "u.vcf"
    p.write_text("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ta\tb\n1\t1\t.\tA\tT\t.\t.\t.\tGT\t0/1\t1|1\n")
    q = Q.read_query(vcf=str(p))
    _, _, rep = Q.match_sites(m, q)
    with pytest.raises(SystemExit, match="without phase"):
        Q.check_query(m, q, rep)
    Q.check_query(dict(m, phased=False), q, rep)              # an unphased model takes it
    mq = {"kind": "matrix", "gt": np.zeros((1, 2, 2), np.int8), "unphased_hets": None}
    with pytest.raises(SystemExit, match="no phase"):
        Q.check_query(m, mq, rep)


def test_select_samples():
    q = _query(["1"], [1], [["A", "T"]], n=4)
    assert Q.select_samples(q).tolist() == [0, 1, 2, 3]
    assert Q.select_samples(q, ["s2", "s0"]).tolist() == [2, 0]
    with pytest.raises(SystemExit, match="not in the query"):
        Q.select_samples(q, ["s9"])


# ------------------------------------------------------------------ rows, imputation, absent sites
def test_query_rows_numpy_against_a_naive_loop():
    rng = np.random.default_rng(3)
    gt = rng.integers(-1, 4, (9, 11, 2)).astype(np.int8)
    cv = np.array([3, -1, 0, 8, 3, 5], np.int32)
    ca = np.array([1, 1, 0, 2, 3, 1], np.int8)
    order = np.array([10, 0, 4, 4, 7], np.int32)
    X = query_rows_numpy(gt, cv, ca, order, width=8)
    for r, s in enumerate(order):
        for k in range(8):
            want = 0 if k >= 6 or cv[k] < 0 else sum(int(gt[cv[k], s, p] == ca[k]) for p in range(2))
            assert X[r, k] == want


def test_compact_calls_remaps_in_query_order():
    gt = np.arange(6 * 2 * 2, dtype=np.int8).reshape(6, 2, 2)
    cols = [(np.array([4, -1, 1], np.int32), None), (np.array([1, 5], np.int32), None)]
    calls, remapped, used = Q.compact_calls({"gt": gt}, cols)
    assert used.tolist() == [1, 4, 5] and np.array_equal(calls, gt[[1, 4, 5]])
    assert remapped[0].tolist() == [1, -1, 0] and remapped[1].tolist() == [0, 2]


def test_impute_draw_order_and_values():
    rng = np.random.default_rng(5)
    calls = rng.integers(0, 2, (4, 6, 2)).astype(np.int8)
    calls[rng.random((4, 6, 2)) < 0.3] = -1
    before = calls.copy()
    cv = np.array([2, 0, -1, 2], np.int32)
    ca = np.array([1, 0, 1, 1], np.int8)
    af = np.array([0.3, 0.6, 0.5, 0.9])
    rows = np.array([5, 1, 3], np.int64)
    np.random.seed(11)
    Q.impute_calls(calls, rows, cv, ca, af, phased=False)
    np.random.seed(11)
    for v, k in ((0, 1), (2, 0)):                              # variant order; a variant takes its first column
        for r in rows:                                         # then row order
            if (before[v, r] < 0).any():
                c = np.random.binomial(2, af[k])
                assert (calls[v, r] == ca[k]).sum() == c and (calls[v, r] >= 0).all()
    untouched = np.ones(calls.shape[:2], bool)
    untouched[np.ix_([0, 2], rows)] = False
    assert np.array_equal(calls[untouched], before[untouched])


def test_absent_gamma():
    w = _weights(K=4)
    out = Q.absent_gamma(w, np.array([0, -1, 2, -1], np.int32))
    assert out["gamma"].tolist() == [w["gamma"][0], 0.0, w["gamma"][2], 0.0] and out["gamma"].dtype == np.float32
    assert out["beta"] is w["beta"] and w["gamma"][1] != 0
