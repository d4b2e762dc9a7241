"""Kept models on imputed dosages (`predict` / `explain --dosage`), host side: query_rows_dosage_numpy - the NumPy restatement
of loc_query_rows_dosage that tests/test_gpu_query_dosage.py holds the kernel to -, the readers (DS and GP VCFs, a zarr
store, a float matrix), the matching of two-allele records, compact_dosages, the --impute_missing draws against impute_calls,
and every refusal before any device work.  Nothing here needs a GPU."""
import json
import os

import numpy as np
import pytest

from locator_amd import explain as E
from locator_amd import genotypes as G
from locator_amd import locator as L
from locator_amd import predict as P
from locator_amd import query as Q
from tests.dosage_util import write_dosage_vcf
from tests.test_query import _model, _weights

QMAX = 2 * G.DOSAGE_UNIT


def query_rows_dosage_numpy(ds, col_variant, col_allele, sample_order, width=None):
    """loc_query_rows_dosage restated: with d = ds[col_variant[k]][sample_order[r]] and q = rint(fp32(d) * 63) clamped to
    0..126, X[r][k] = q for col_allele[k] == 1, 126 - q for col_allele[k] == 0, and 0 for an absent (-1) or out-of-range
    column, any other allele, or a NaN; columns K .. width stay 0."""
    ds = np.asarray(ds, dtype=np.float32)
    K = len(col_variant)
    X = np.zeros((len(sample_order), K if width is None else width), np.uint8)
    order = np.asarray(sample_order, dtype=np.int64)
    for k in range(K):
        v, a = int(col_variant[k]), int(col_allele[k])
        if v < 0 or v >= ds.shape[0] or a not in (0, 1):
            continue
        d = ds[v][order]
        with np.errstate(invalid="ignore"):
            q = np.minimum(np.maximum(np.rint(d * np.float32(63.0)), np.float32(0)), np.float32(QMAX))
        x = q if a == 1 else np.float32(QMAX) - q
        X[:, k] = np.where(np.isnan(d), 0, x).astype(np.uint8)
    return X


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


# ------------------------------------------------------------------ the entry point's declaration and binding
def test_extension_header_is_bound_as_the_main_header_is():
    """include/locator_hip_query.h (entry points after version 1 of the ABI, whose list tests/test_abi.py pins): every
    function it declares is exported by the library and bound from its prototype, by the parser that reads locator_hip.h."""
    import ctypes as C

    from locator_amd import _abi
    from tests.abi_util import check_extension
    vp = C.c_void_p
    check_extension("ext", {"loc_query_rows_dosage": (C.c_int, [vp, C.c_int64, C.c_int, vp, vp, C.c_int, vp, C.c_int, vp, C.c_int64, vp])},
                    {})
    with pytest.raises(ValueError):
        _abi.parse("int loc_f(size_t n);")                       # the same refusals as for the main header


# ------------------------------------------------------------------ the restatement on hand-written values
def test_restatement_on_hand_written_values():
    nan = np.nan
    #               0    1    2    3     4    5     6        7       8    9
    ds = np.array([[0.0, 2.0, nan, 0.25, 0.5, 1.5, -0.0005, 2.0005, 2.5, -1.0],      # variant 0
                   [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]], np.float32)   # variant 1
    order = np.arange(10, dtype=np.int32)
    # 0.25 * 63 = 15.75 -> 16; 0.5 * 63 = 31.5 and 1.5 * 63 = 94.5 are exact ties: to the even neighbour, 32 and 94;
    # values outside [0, 2] clamp to 0 and 126
    want = [0, 126, 0, 16, 32, 94, 0, 126, 126, 0]
    cv = np.array([0, 0, -1, 0, 1, 5, 0], np.int32)
    ca = np.array([1, 0, 1, 2, 0, 1, -1], np.int8)
    X = query_rows_dosage_numpy(ds, cv, ca, order, width=9)
    assert X.shape == (10, 9)
    assert X[:, 0].tolist() == want
    flipped = [QMAX - w for w in want]
    flipped[2] = 0                                              # a NaN stays 0 under the flip
    assert X[:, 1].tolist() == flipped
    assert not X[:, 2].any()                                    # absent
    assert not X[:, 3].any()                                    # col_allele 2: no such allele in a two-allele record
    assert X[:, 4].tolist() == [63] * 10                        # 126 - 63
    assert not X[:, 5].any()                                    # variant index past the end: never read
    assert not X[:, 6].any() and not X[:, 7:].any()             # negative allele; padding
    assert X[[3, 0], :][:, 0].tolist() == query_rows_dosage_numpy(ds, cv, ca, [3, 0])[:, 0].tolist() == [16, 0]


def test_restatement_ties_round_to_even_and_flip_sums_to_126():
    """d = fp32((k + 0.5) / 63): the fp32 product d * 63 (the exact double product rounded once) is k + 0.5 for many k - an
    exact tie, which goes to the even neighbour - and just off it for the rest.  Python's round() is the witness."""
    k = np.arange(0, 126)
    d = ((k + 0.5) / 63.0).astype(np.float32)
    prod = [float(np.float32(float(x) * 63.0)) for x in d]      # 24-bit x 6-bit: exact in double, one rounding to fp32
    assert sum(p == i + 0.5 for i, p in zip(k, prod)) >= 20     # real ties are among them
    want = [int(round(p)) for p in prod]                         # half to even
    ds = d[None, :]
    order = np.arange(126, dtype=np.int32)
    X = query_rows_dosage_numpy(ds, np.array([0, 0], np.int32), np.array([1, 0], np.int8), order)
    assert X[:, 0].tolist() == want
    assert (X[:, 0].astype(int) + X[:, 1] == QMAX).all()
    assert np.array_equal(X[:, 0], G.dosage_q(d))                # the host form of the training path agrees


# ------------------------------------------------------------------ readers
def _vary_format(path, field):
    """Every second record of a `GT:DP:field` VCF rewritten as `field:GT:DP`."""
    lines = open(path).read().splitlines()
    n = 0
    for i, ln in enumerate(lines):
        if ln.startswith("#"):
            continue
        n += 1
        if n % 2:
            continue
        f = ln.split("\t")
        assert f[8] == f"GT:DP:{field}"
        f[8] = f"{field}:GT:DP"
        f[9:] = [":".join([c.split(":")[2]] + c.split(":")[:2]) for c in f[9:]]
        lines[i] = "\t".join(f)
    open(path, "w").write("\n".join(lines) + "\n")


def _small_ds(V=7, N=5, seed=3):
    rng = np.random.default_rng(seed)
    ds = rng.uniform(0, 2, (V, N)).round(4).astype(np.float32)
    ds[1, 2] = np.nan
    ds[V - 2, 0] = np.nan
    return ds, np.array([f"s{i}" for i in range(N)]), np.arange(V) * 10 + 100


@pytest.mark.parametrize("field", ["DS", "GP"])
def test_vcf_reader_sites_line_up_after_a_multiallelic_record_is_dropped(tmp_path, field):
    ds, samples, pos = _small_ds()
    alts = ["T", "T", "T,G", "C", "T", "T", "G"]
    path = str(tmp_path / "q.vcf")
    write_dosage_vcf(path, ds, samples, pos, field=field, alts=alts)
    _vary_format(path, field)
    plain = G.read_vcf_dosage(path, field)
    full = G.read_vcf_dosage(path, field, sites=True)
    assert set(plain) == {"calldata/DS", "samples", "variants/POS", "multiallelic_dropped"}          # default unchanged
    for k in plain:
        assert np.array_equal(plain[k], full[k], equal_nan=True) if k == "calldata/DS" else np.array_equal(plain[k], full[k])
    keep = [0, 1, 3, 4, 5, 6]
    assert full["multiallelic_dropped"] == 1 and full["variants/POS"].tolist() == pos[keep].tolist()
    assert full["variants/CHROM"].tolist() == ["1"] * 6 and full["variants/REF"].tolist() == ["A"] * 6
    assert full["variants/ALT"].tolist() == [alts[i] for i in keep]
    np.testing.assert_allclose(full["calldata/DS"], ds[keep], atol=2e-6 if field == "GP" else 0, equal_nan=True)

    q = Q.read_query_dosage(vcf=path, field=field)
    assert q["kind"] == "vcf" and q["ds"].dtype == np.float32 and q["ds"].shape == (6, 5)
    assert q["samples"].tolist() == samples.tolist() and q["pos"].tolist() == pos[keep].tolist()
    assert q["alleles"] == [["A", alts[i]] for i in keep] and q["chrom"].tolist() == ["1"] * 6
    assert q["multiallelic_dropped"] == 1


def _store(path, ds, samples, pos, alt=None, with_ds=True):
    V = ds.shape[0]
    gt = np.zeros((V, ds.shape[1], 2), np.int8)
    G.write_callset_zarr(path, gt, pos, samples, chunk_variants=4, compressor="blosc", chrom=["1"] * V, ref=["A"] * V,
                         alt=["T"] * V if alt is None else alt)
    if with_ds:
        G.write_dosage_zarr(path, ds, chunk_variants=4, compressor="blosc")


def test_zarr_reader_with_and_without_dosages(tmp_path):
    ds, samples, pos = _small_ds()
    alt = np.array([["T", ""], ["T", ""], ["T", "G"], ["C", ""], ["T", ""], ["T", ""], ["G", ""]])
    _store(str(tmp_path / "z"), ds, samples, pos, alt)
    q = Q.read_query_dosage(zarr=str(tmp_path / "z"))
    assert q["kind"] == "zarr" and np.array_equal(q["ds"], ds, equal_nan=True) and q["ds"].dtype == np.float32
    assert q["samples"].tolist() == samples.tolist() and q["pos"].tolist() == pos.tolist()
    assert all(len(a) == 2 for a in q["alleles"]) and q["alleles"][3] == ["A", "C"]
    assert q["alleles"][2] == ["A", ""] and q["multiallelic_dropped"] == 1         # two ALT alleles: never matched
    m = _model(["1"] * 3, [120, 130, 100], ["A"] * 3, ["T", "C", "T"])
    cv, ca, rep = Q.match_sites(m, q)
    assert cv.tolist() == [-1, 3, 0] and rep["absent"] == 1
    _store(str(tmp_path / "gt_only"), ds, samples, pos, with_ds=False)
    with pytest.raises(Q.QueryRefused, match="calldata/DS"):
        Q.read_query_dosage(zarr=str(tmp_path / "gt_only"))
    G.write_callset_zarr(str(tmp_path / "no_sites"), np.zeros((7, 5, 2), np.int8), pos, samples)
    G.write_dosage_zarr(str(tmp_path / "no_sites"), ds)
    with pytest.raises(Q.QueryRefused, match="variants/CHROM"):
        Q.read_query_dosage(zarr=str(tmp_path / "no_sites"))


def test_float_matrix_reader(tmp_path):
    p = tmp_path / "q.txt"
    p.write_text("sampleID\tsnpB\tsnpA\tsnpC\nq1\t0.25\t1\tNA\nq2\t2\t1.5\t0.0\n")
    q = Q.read_query_dosage(matrix=str(p))
    assert q["kind"] == "matrix" and q["names"].tolist() == ["snpB", "snpA", "snpC"] and q["samples"].tolist() == ["q1", "q2"]
    assert q["ds"].dtype == np.float32 and np.array_equal(q["ds"], np.array([[0.25, 2], [1, 1.5], [np.nan, 0]], np.float32),
                                                          equal_nan=True)
    m = _model(["snpA", "snpC", "snpX"], [-1] * 3, [""] * 3, [""] * 3)
    cv, ca, rep = Q.match_sites(m, q)
    assert cv.tolist() == [1, 2, -1] and ca.tolist()[:2] == [1, 1] and rep["absent"] == 1
    X = query_rows_dosage_numpy(q["ds"], cv, ca, [1, 0])
    assert X.tolist() == [[94, 0, 0], [63, 0, 0]]


# ------------------------------------------------------------------ matching, compaction, imputation
def _dquery(chrom, pos, alleles, ds):
    ds = np.asarray(ds, np.float32)
    return {"kind": "vcf", "chrom": np.array(chrom, str), "pos": np.array(pos, np.int64), "alleles": alleles, "ds": ds,
            "samples": np.array([f"s{i}" for i in range(ds.shape[1])])}


def test_matching_swaps_absent_sites_and_repeated_columns():
    # a bootstrap-like model: site (1, 7) twice; (1, 9) swapped in the query; (1, 11) absent; (2, 7) another chromosome
    m = _model(["1", "1", "1", "1", "2"], [7, 9, 7, 11, 7], ["A", "C", "A", "G", "A"], ["T", "G", "T", "C", "T"])
    ds = [[0.1, 1.9], [1.0, np.nan], [0.5, 0.25], [2.0, 0.0]]
    q = _dquery(["3", "1", "1", "2"], [7, 9, 7, 7], [["A", "T"], ["G", "C"], ["A", "T"], ["A", "T"]], ds)
    cv, ca, rep = Q.match_sites(m, q)
    assert cv.tolist() == [2, 1, 2, -1, 3] and ca.tolist() == [1, 0, 1, 0, 1]
    assert rep == {"model": "m", "K": 5, "matched": 4, "allele_not_1": 1, "absent": 1}
    assert set(ca[cv >= 0].tolist()) <= {0, 1}
    Q.check_query_dosage(m, q, rep, 0.8)
    comp, (cvc,), used = Q.compact_dosages(q, [(cv, ca)])
    assert used.tolist() == [1, 2, 3] and comp.flags.c_contiguous and comp.dtype == np.float32
    assert np.array_equal(comp, np.asarray(ds, np.float32)[[1, 2, 3]], equal_nan=True) and cvc.tolist() == [1, 0, 1, -1, 2]
    X = query_rows_dosage_numpy(comp, cvc, ca, [1, 0])
    assert X.tolist() == [[16, 0, 16, 0, 0], [32, 63, 32, 0, 126]]
    assert np.array_equal(X, query_rows_dosage_numpy(q["ds"], cv, ca, [1, 0]))
    # two models share one compaction, as compact_calls
    comp2, remapped, used2 = Q.compact_dosages(q, [(np.array([3, -1], np.int32), None), (np.array([0, 3], np.int32), None)])
    assert used2.tolist() == [0, 3] and remapped[0].tolist() == [1, -1] and remapped[1].tolist() == [0, 1]
    empty, (none,), _ = Q.compact_dosages(q, [(np.full(3, -1, np.int32), None)])
    assert empty.shape == (0, 2) and none.tolist() == [-1] * 3


def test_impute_dosages_draws_as_impute_calls_and_gives_63_draws():
    rng = np.random.default_rng(5)
    U, N = 6, 9
    calls = rng.integers(0, 2, (U, N, 2)).astype(np.int8)
    miss = rng.random((U, N)) < 0.3
    miss[:, 5] = True                                           # every variant misses one of the predicted rows
    calls[miss] = -1
    ds = rng.uniform(0, 2, (U, N)).astype(np.float32)
    ds[miss] = np.nan                                           # the same missing pattern
    before = ds.copy()
    cv = np.array([2, 0, -1, 2, 5, 4], np.int32)                # variant 2 twice: takes its first column (0)
    ca = np.array([1, 0, 1, 0, 0, 1], np.int8)
    af = np.array([0.3, 0.6, 0.5, 0.9, 0.2, 0.7])
    rows = np.array([5, 1, 3, 8], np.int64)
    np.random.seed(11)
    Q.impute_calls(calls, rows, cv, ca, af, phased=False)
    state_calls = np.random.get_state()[1].copy()
    follow_calls = np.random.random_sample()
    np.random.seed(11)
    out = Q.impute_dosages(ds, rows, cv, ca, af)
    assert out is ds
    assert np.array_equal(np.random.get_state()[1], state_calls) and np.random.random_sample() == follow_calls
    np.random.seed(11)
    for v, k in ((0, 1), (2, 0), (4, 5), (5, 4)):               # variant order; a variant takes its first column
        for r in rows:                                          # then row order
            if miss[v, r]:
                c = np.random.binomial(2, af[k])
                assert ds[v, r] == (c if ca[k] == 1 else 2 - c)
                assert (calls[v, r] == ca[k]).sum() == c         # ... the very draw impute_calls stored
    untouched = np.ones((U, N), bool)
    untouched[np.ix_([0, 2, 4, 5], rows)] = False
    assert np.array_equal(ds[untouched], before[untouched], equal_nan=True)
    assert not np.isnan(ds[np.ix_([0, 2, 4, 5], rows)]).any()
    # column values: 63 * draws = 63 * copies of the column's allele in the imputed calls, for every column's own allele
    order = rows.astype(np.int32)
    X = query_rows_dosage_numpy(ds, cv, ca, order)
    for k in (0, 1, 4, 5):
        copies = (calls[cv[k]][rows] == ca[k]).sum(axis=1)
        was = miss[cv[k]][rows]
        assert (X[was, k] == 63 * copies[was]).all() and was.any()
    # an explicit generator draws from itself, not from the global stream
    ds2 = before.copy()
    np.random.seed(1)
    s0 = np.random.get_state()[1].copy()
    Q.impute_dosages(ds2, rows, cv, ca, af, np.random.RandomState(11))
    assert np.array_equal(np.random.get_state()[1], s0) and np.array_equal(ds2, ds, equal_nan=True)
    none = before.copy()
    assert Q.impute_dosages(none, rows, np.full(3, -1, np.int32), np.ones(3, np.int8), af[:3]) is none
    assert np.array_equal(none, before, equal_nan=True)


# ------------------------------------------------------------------ refusals, all before any device work
def _model_file(path, K=6, ploidy=2, phased=False):
    meta = {"chrom": np.array(["1"] * K, dtype=object), "pos": np.arange(K) * 10 + 100, "ref": np.array(["A"] * K, dtype=object),
            "alt": np.array(["T"] * K, dtype=object), "af": np.full(K, 0.4), "locs_norm": [0.0, 1.0, 0.0, 1.0],
            "ploidy": ploidy, "phased": phased, "params_json": json.dumps({"width": 4, "nlayers": 2, "dropout_prop": 0.25})}
    L.save_model(path, _weights(K=K), meta)
    return path


def _ds_vcf(tmp_path, name="q.vcf", V=6, field="DS", ds=None):
    d, samples, pos = _small_ds(V=V)
    path = str(tmp_path / name)
    write_dosage_vcf(path, d if ds is None else ds, samples, pos, field=field)
    return path


@pytest.mark.parametrize("command", [P, E], ids=["predict", "explain"])
def test_commands_refuse_before_any_device_work(tmp_path, no_device, command):
    good = _model_file(str(tmp_path / "ok.model.npz"))
    vcf = _ds_vcf(tmp_path)
    out = str(tmp_path / "o")

    def refused(match, model=good, query=("--vcf", vcf), extra=("--dosage",)):
        with pytest.raises(Q.QueryRefused, match=match):
            command.main(["--model", model, *query, "--out", out, *extra])

    refused("--phased model", model=_model_file(str(tmp_path / "ph.model.npz"), phased=True))
    refused("ploidy 1", model=_model_file(str(tmp_path / "hap.model.npz"), ploidy=1))
    refused("min_site_overlap", query=("--vcf", _ds_vcf(tmp_path, "few.vcf", V=2)))
    refused("min_site_overlap", extra=("--dosage", "--min_site_overlap", "1.01"))
    refused("no FORMAT/GP", extra=("--dosage", "GP"))                                   # a DS-only file asked for GP
    gt_only = tmp_path / "gt.vcf"
    gt_only.write_text("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ta\tb\n1\t100\t.\tA\tT\t.\t.\t.\tGT\t0|1\t1|1\n")
    refused("no FORMAT/DS", query=("--vcf", str(gt_only)))
    ds, samples, pos = _small_ds(V=6)
    _store(str(tmp_path / "z"), ds, samples, pos)
    refused("GP: a zarr store", query=("--zarr", str(tmp_path / "z")), extra=("--dosage", "GP"))
    _store(str(tmp_path / "zgt"), ds, samples, pos, with_ds=False)
    refused("calldata/DS", query=("--zarr", str(tmp_path / "zgt")))
    mat = tmp_path / "m.txt"
    mat.write_text("sampleID\tsnpA\nq1\t0.5\n")
    refused("GP: a --matrix", query=("--matrix", str(mat)), extra=("--dosage", "GP"))
    lines = open(vcf).read().splitlines()
    f = lines[4].split("\t")
    f[10] = "0/1:7:2.25"
    lines[4] = "\t".join(f)
    (tmp_path / "range.vcf").write_text("\n".join(lines) + "\n")
    refused(r"dosage 2\.25 .* outside", query=("--vcf", str(tmp_path / "range.vcf")))
    big = tmp_path / "big.txt"
    big.write_text("sampleID\t" + "\t".join(f"s{i}" for i in range(3)) + "\nq1\t0.5\t-0.5\t1\n")
    refused(r"dosage -0\.5 .* outside", query=("--matrix", str(big)))
    assert not [f for f in os.listdir(tmp_path) if f.startswith("o_")]                   # nothing was written


def test_check_query_dosage_on_dicts(no_device):
    m = _model(["1"] * 4, [1, 2, 3, 4], ["A"] * 4, ["T"] * 4)
    q = _dquery(["1", "1"], [1, 2], [["A", "T"], ["A", "T"]], [[0.5, 2.0005], [np.nan, -0.0005]])
    _, _, rep = Q.match_sites(m, q)
    Q.check_query_dosage(m, q, rep, 0.5)                                         # the edge of the accepted range passes
    with pytest.raises(Q.QueryRefused, match="min_site_overlap"):
        Q.check_query_dosage(m, q, rep, 0.75)
    with pytest.raises(Q.QueryRefused, match="--phased model"):
        Q.check_query_dosage(dict(m, phased=True), q, rep, 0.5)
    with pytest.raises(Q.QueryRefused, match="ploidy 3"):
        Q.check_query_dosage(dict(m, ploidy=3), q, rep, 0.5)
    with pytest.raises(Q.QueryRefused, match="holds no dosages"):
        Q.check_query_dosage(m, {k: v for k, v in q.items() if k != "ds"}, rep, 0.5)
    for bad in (2.002, -0.002):
        q2 = dict(q, ds=np.array([[0.5, bad], [np.nan, 0.0]], np.float32))
        with pytest.raises(Q.QueryRefused, match="outside"):
            Q.check_query_dosage(m, q2, rep, 0.5)


def test_flag_is_absent_unless_given_and_bare_means_ds():
    for cmd in (P, E):
        p = cmd.build_parser()
        base = ["--model", "m", "--out", "o"]
        assert p.parse_args(base).dosage is None
        assert p.parse_args(base + ["--dosage"]).dosage == "DS" and p.parse_args(base + ["--dosage", "GP"]).dosage == "GP"
        with pytest.raises(SystemExit):
            p.parse_args(base + ["--dosage", "PL"])
