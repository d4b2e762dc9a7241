"""--dosage on the host: the DS / GP reader, the fixed-point form q = rint(63 d), the filter and the impute / jacknife
streams on q, the refusals and params.json.  Nothing here needs a GPU; tests/test_gpu_dosage.py runs the device path."""
import json

import numpy as np
import pandas as pd
import pytest

from locator_amd import genotypes as G
from locator_amd import locator as L
from tests.dosage_util import SAMPLES, VCF, golden_counts, noisy_dosage, write_dosage_vcf, write_dosage_zarr


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


def _vcf(path, header_samples, records):
    lines = ["##fileformat=VCFv4.2",
             "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(header_samples)]
    lines += ["\t".join(r) for r in records]
    path.write_text("\n".join(lines) + "\n")
    return str(path)


def _sd(path, ids):
    pd.DataFrame({"sampleID": ids, "x": [1.0, 2.0] + [np.nan] * (len(ids) - 2),
                  "y": [1.0, 3.0] + [np.nan] * (len(ids) - 2)}).to_csv(path, sep="\t", index=False)
    return str(path)


# ------------------------------------------------------------------ reader
def test_ds_and_gp_at_any_format_position_mixed_formats_missing_and_multi_alt(tmp_path, capsys):
    rec = lambda pos, alt, fmt, *cells: ["1", str(pos), ".", "A", alt, ".", "PASS", ".", fmt] + list(cells)
    path = _vcf(tmp_path / "a.vcf", ["s0", "s1", "s2"], [
        rec(10, "T", "GT:DS", "0/1:0.9", "1/1:2", "0/0:."),
        rec(20, "T", "DS:GT:GP", "1.25:0/1:0,1,0", ".:./.:.", "0:0/0:1,0,0"),
        rec(30, "G,C", "GT:DS", "0/1:1,0", "0/0:0,0", "1/1:0,2"),          # multi-ALT: dropped
        rec(40, "T", "GT:DP:GP:DS", "0/1:3:0.1,0.6,0.3:1.2", "0/0:4:.,.,.:0", "1/1:5:0,0,1"),   # s2 has no DS subfield
    ])
    ds = G.read_vcf_dosage(path, "DS")
    want = np.array([[0.9, 2, np.nan], [1.25, np.nan, 0], [1.2, 0, np.nan]], np.float32)
    assert np.array_equal(ds["calldata/DS"], want, equal_nan=True)
    assert ds["multiallelic_dropped"] == 1 and list(ds["variants/POS"]) == [10, 20, 40]
    assert list(ds["samples"]) == ["s0", "s1", "s2"]
    # GP -> GP1 + 2 GP2; the first record has no GP: a clear error naming it
    with pytest.raises(ValueError, match=r"record 1:10 has no FORMAT/GP"):
        G.read_vcf_dosage(path, "GP")
    gp_only = _vcf(tmp_path / "g.vcf", ["s0", "s1", "s2"], [
        rec(20, "T", "GT:GP", "0/1:0,1,0", "./.:.", "0/0:1,0,0"),
        rec(40, "T", "GP:GT", "0.1,0.6,0.3:0/1", ".,.,.:0/0", "0,0,1:1/1"),
    ])
    gp = G.read_vcf_dosage(gp_only, "GP")["calldata/DS"]
    assert np.array_equal(gp, np.array([[1, np.nan, 0], [np.float32(0.6 + 0.6), np.nan, 2]], np.float32), equal_nan=True)


def test_range_errors_name_the_record_and_the_sample_and_in_range_values_are_clamped(tmp_path):
    rec = lambda pos, *cells: ["2", str(pos), ".", "A", "T", ".", "PASS", ".", "DS"] + list(cells)
    ok = _vcf(tmp_path / "ok.vcf", ["a", "b"], [rec(5, "-0.001", "2.001")])
    assert np.array_equal(G.read_vcf_dosage(ok)["calldata/DS"], np.array([[0, 2]], np.float32))
    bad = _vcf(tmp_path / "bad.vcf", ["a", "b"], [rec(5, "0.5", "1"), rec(7, "1", "2.0011")])
    with pytest.raises(ValueError, match=r"record 2:7, sample b: dosage 2.0011"):
        G.read_vcf_dosage(bad)
    neg = _vcf(tmp_path / "neg.vcf", ["a", "b"], [rec(9, "-0.01", "1")])
    with pytest.raises(ValueError, match=r"record 2:9, sample a"):
        G.read_vcf_dosage(neg)
    junk = _vcf(tmp_path / "junk.vcf", ["a", "b"], [rec(9, "x", "1")])
    with pytest.raises(ValueError, match=r"record 2:9, sample a"):
        G.read_vcf_dosage(junk)


def test_golden_derived_vcf_roundtrips_through_ds_and_gp(tmp_path):
    c, samples, pos = golden_counts()
    d = noisy_dosage(c[:300], missing=0.02)
    write_dosage_vcf(tmp_path / "d.vcf.gz", d, samples, pos[:300], "DS")
    write_dosage_vcf(tmp_path / "g.vcf", d, samples, pos[:300], "GP", gt=False)
    a = G.read_vcf_dosage(str(tmp_path / "d.vcf.gz"), "DS")["calldata/DS"]
    b = G.read_vcf_dosage(str(tmp_path / "g.vcf"), "GP")["calldata/DS"]
    assert np.array_equal(a, d, equal_nan=True)
    assert np.array_equal(np.isnan(b), np.isnan(d)) and np.nanmax(np.abs(b - d)) < 2e-6
    assert np.array_equal(G.dosage_q(a), G.dosage_q(b))


# ------------------------------------------------------------------ fixed point and the filter
def test_quantisation_known_answers():
    d = np.array([0, 1 / 63, 0.5, 0.0079, 0.008, 1, 1.99, 2, np.nan, 2.0009], np.float32)
    q = G.dosage_q(d)
    assert list(q) == [0, 1, 32, 0, 1, 63, 125, 126, 255, 126]
    # the largest error is half a step, 1/126 of an allele
    x = np.linspace(0, 2, 100001, dtype=np.float32)
    assert np.abs(G.dosage_q(x) / 63.0 - x).max() <= 1 / 126 + 1e-7


def test_filter_boundaries_on_the_sum_of_q():
    # rows: sum = 63*2 - 1, = 63*2, all 126 (monomorphic), all 0, one missing keeps n_called at 2 of 3
    q = np.array([[63, 62, 0], [63, 63, 0], [126, 126, 126], [0, 0, 0], [126, 126, 255], [126, 125, 255]], np.uint8)
    kept = G.filter_dosage(q, min_mac=2, verbose=False)
    assert kept.tolist() == [[63, 63, 0], [126, 125, 0]]
    assert G.filter_dosage(q, min_mac=1, verbose=False).tolist() == [[63, 62, 0], [63, 63, 0], [126, 125, 0]]
    assert G.filter_dosage(q, min_mac=3, verbose=False).tolist() == [[126, 125, 0]]      # 251 >= 189
    assert G.filter_dosage(q, min_mac=4, verbose=False).shape == (0, 3)                   # 251 < 252


def test_impute_stream_is_63_binomial_2_af_in_replace_md_order():
    rng = np.random.default_rng(3)
    q = rng.integers(0, 127, (40, 25)).astype(np.uint8)
    q[rng.random(q.shape) < 0.1] = 255
    np.random.seed(11)
    got = G.filter_dosage(q, min_mac=2, impute_missing=True, verbose=False)
    # hand-written: the same filter, then one legacy-stream draw per missing value, variant-major
    np.random.seed(11)
    keep = []
    for v in range(q.shape[0]):
        c = q[v][q[v] != 255].astype(np.int64)
        keep.append(c.sum() >= 126 and c.sum() > 0 and c.sum() < 126 * len(c))
    want = q[np.array(keep)].astype(np.int64)
    for i in range(want.shape[0]):
        called = want[i] != 255
        af = want[i][called].sum() / (126 * called.sum())
        for j in range(want.shape[1]):
            if not called[j]:
                want[i, j] = 63 * np.random.binomial(2, af)
    assert np.array_equal(got, want) and got.dtype == np.uint8
    assert set(np.unique(got[q[np.array(keep)] == 255])) <= {0, 63, 126}
    after = np.random.random()                          # the hand-written draws left the stream here ...
    np.random.seed(11)
    G.filter_dosage(q, min_mac=2, impute_missing=True, verbose=False)
    assert np.random.random() == after                  # ... and so does filter_dosage


def test_jacknife_dosage_draws_are_63_binomial_of_the_q_frequency(tmp_path, monkeypatch):
    ac = np.array([[0, 63, 126, 63], [126, 126, 0, 0], [63, 0, 0, 0]], np.uint8)      # (sites, samples)
    base = np.array([[63, 126, 0], [0, 63, 63]], np.uint8)                            # (pred rows, sites)
    seen = {}

    class _Model:
        def predict(self, x):
            seen.setdefault("x", []).append(np.array(x))
            return np.zeros((len(x), 2), np.float32)
    monkeypatch.setattr(L, "train_network", lambda *a, **k: (None, _Model()))
    monkeypatch.setattr(L, "predict_locs", lambda *a, **k: [])
    monkeypatch.setattr(L, "plot_history", lambda *a, **k: None)
    monkeypatch.setattr(L, "load_network", lambda *a, **k: None)
    L._setup(["--vcf", "x.vcf", "--sample_data", SAMPLES, "--out", str(tmp_path / "j"), "--dosage", "--jacknife",
              "--nboots", "3", "--jacknife_prop", "0.67", "--seed", "5"])
    np.random.seed(21)
    L._jacknife(ac, None, None, None, None, base, np.array([0, 1]), np.array(["a", "b"]), 1.0, 0.0, 1.0, 0.0)
    np.random.seed(21)
    af = ac.sum(axis=1) / (4 * 126)
    for b in range(3):
        sites = np.random.choice(3, 2, replace=False)
        vals = 63 * np.random.binomial(2, af[sites][:, None], (2, 2))
        want = base.copy()
        want[:, sites] = vals.T
        assert np.array_equal(seen["x"][0][2 * b:2 * b + 2], want), b


# ------------------------------------------------------------------ CLI prologue, refusals, params.json
def test_cli_prologue_builds_the_q_matrix_from_ds(tmp_path):
    c, samples, pos = golden_counts()
    d = noisy_dosage(c, missing=0.01)
    vcf = str(tmp_path / "d.vcf.gz")
    write_dosage_vcf(vcf, d, samples, pos)
    L._setup(["--vcf", vcf, "--sample_data", SAMPLES, "--out", str(tmp_path / "o"), "--seed", "12345", "--dosage"])
    L._dosage_preflight()
    s, state = L._prologue()
    ac = state[4]
    assert np.array_equal(ac, G.filter_dosage(G.dosage_q(d), 2, verbose=False))
    assert ac.dtype == np.uint8 and ac.max() == 126 and ac.shape[1] == len(samples)
    # the split and the transposed row sets are the GT run's functions on q
    train = state[5]
    assert np.array_equal(state[7], ac[:, train].T)


def test_matrix_values_are_read_as_float_dosages(tmp_path):
    mat = tmp_path / "m.txt"
    pd.DataFrame({"sampleID": ["a", "b", "c"], "s0": [0.93, 1.5, np.nan], "s1": [0, 2, 1]}).to_csv(mat, sep="\t", index=False)
    d, samples = G.read_matrix_dosage(str(mat))
    assert np.array_equal(d, np.array([[0.93, 1.5, np.nan], [0, 2, 1]], np.float32), equal_nan=True)
    L._setup(["--matrix", str(mat), "--sample_data", SAMPLES, "--out", str(tmp_path / "m"), "--dosage"])
    q, _ = L.load_genotypes()
    assert q.tolist() == [[59, 94, 255], [0, 126, 63]]


@pytest.mark.parametrize("extra, msg", [
    (["--phased"], "--dosage cannot be combined with --phased"),
    (["--predict_packed"], "--dosage cannot be combined with --predict_packed"),
    (["--keep_model"], "--dosage cannot be combined with --keep_model"),
])
def test_refusals_before_any_device_work(tmp_path, no_device, extra, msg):
    c, samples, pos = golden_counts()
    vcf = str(tmp_path / "d.vcf")
    write_dosage_vcf(vcf, noisy_dosage(c[:50]), samples, pos[:50])
    with pytest.raises(SystemExit, match=msg):
        L.main(["--vcf", vcf, "--sample_data", SAMPLES, "--out", str(tmp_path / "r"), "--dosage"] + extra)


def test_inputs_without_the_field_are_refused(tmp_path, no_device):
    with pytest.raises(SystemExit, match=r"no FORMAT/DS"):
        L.main(["--vcf", VCF, "--sample_data", SAMPLES, "--out", str(tmp_path / "gt"), "--dosage"])
    with pytest.raises(SystemExit, match=r"no FORMAT/GP"):
        L.main(["--vcf", VCF, "--sample_data", SAMPLES, "--out", str(tmp_path / "gt"), "--dosage", "GP"])
    c, samples, pos = golden_counts()
    store = str(tmp_path / "z.zarr")
    G.write_callset_zarr(store, np.zeros((4, len(samples), 2), np.int8), pos[:4], samples)
    with pytest.raises(SystemExit, match=r"has no calldata/DS"):
        L.main(["--zarr", store, "--sample_data", SAMPLES, "--out", str(tmp_path / "z"), "--dosage", "--windows",
                "--in_process"])
    with pytest.raises(SystemExit, match=r"has no calldata/DS"):
        L.main(["--zarr", store, "--sample_data", SAMPLES, "--out", str(tmp_path / "z"), "--dosage"])
    dz_path = str(tmp_path / "d.zarr")
    write_dosage_zarr(dz_path, noisy_dosage(c[:40]), samples, pos[:40])
    with pytest.raises(SystemExit, match=r"calldata/DS only"):
        L.main(["--zarr", dz_path, "--sample_data", SAMPLES, "--out", str(tmp_path / "z"), "--dosage", "GP"])


def test_params_json_has_the_dosage_keys_only_with_the_flag(tmp_path):
    out = str(tmp_path / "a")
    a = L._setup(["--vcf", "x.vcf", "--sample_data", "s.txt", "--out", out, "--seed", "1"])
    raw = open(out + "_params.json").read()
    js = json.loads(raw)
    assert "dosage" not in js and "dosage_unit" not in js and L._dosage(a) is None
    assert list(js) == list(vars(L.build_parser().parse_args([])))
    assert raw == json.dumps({k: v for k, v in vars(a).items() if k != "_net_seed"}, indent=2)
    b = L._setup(["--vcf", "x.vcf", "--sample_data", "s.txt", "--out", str(tmp_path / "b"), "--dosage"])
    jb = json.load(open(str(tmp_path / "b") + "_params.json"))
    assert jb["dosage"] == "DS" and jb["dosage_unit"] == 63 and list(jb)[-2:] == ["dosage", "dosage_unit"]
    assert L._dosage(b) == "DS"
    c = L._setup(["--vcf", "x.vcf", "--sample_data", "s.txt", "--out", str(tmp_path / "c"), "--dosage", "GP"])
    assert json.load(open(str(tmp_path / "c") + "_params.json"))["dosage"] == "GP" and L._dosage(c) == "GP"
    assert L._dosage(L._setup(["--load_params", str(tmp_path / "b") + "_params.json"])) == "DS"
    assert L._dosage(L._setup(["--load_params", out + "_params.json"])) is None


def test_zarr_windows_host_form_reads_calldata_ds(tmp_path):
    c, samples, pos = golden_counts()
    d = noisy_dosage(c[:2000], missing=0.01)
    store = str(tmp_path / "w.zarr")
    write_dosage_zarr(store, d, samples, pos[:2000], chunk_variants=512, with_gt=False)
    L._setup(["--zarr", store, "--sample_data", SAMPLES, "--out", str(tmp_path / "w"), "--dosage", "--windows",
              "--window_size", "200000", "--seed", "3"])
    L._dosage_preflight()
    samples2, state = L._prologue()
    assert state is None
    units = L._window_units(samples2)
    u = dict(units[0], args=L.args)
    L._load_window(u)
    a, b = u["window"]
    ac = G.filter_dosage(G.dosage_q(d[a:b]), 2, verbose=False)
    assert np.array_equal(u["traingen"], ac[:, u["train"]].T)
