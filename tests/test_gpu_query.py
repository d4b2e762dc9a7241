"""Kept models on new genotypes, on the device: loc_query_rows against its NumPy restatement (tests/test_query.py), the
round trip train --keep_model -> predict on the same file (byte-identical predictions), a perturbed query (shuffled,
partly missing, swapped, multi-allelic, reordered samples) against an independent expectation and the oracle, and model
sets: --bootstrap, --windows on a zarr store, --phased."""
import gzip
import os

import numpy as np
import pandas as pd
import pytest
import torch

from locator_amd import genotypes as G
from locator_amd import locator as L
from locator_amd import predict as P
from locator_amd import query as Q
from locator_amd import summarize as S
from tests.test_query import query_rows_numpy

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
VCF = os.path.join(GOLD, "test_genotypes.vcf.gz")
SAMPLES = os.path.join(GOLD, "test_sample_data.txt")
SHORT = ["--max_epochs", "3", "--patience", "3", "--keras_verbose", "0", "--plot_history", ""]


def _run(argv):
    np.random.seed(None)
    assert L.main(argv) == 0


def _na_ids(tmp_path):
    t = pd.read_csv(SAMPLES, sep="\t")
    ids = t.loc[t["x"].isna(), "sampleID"].astype(str).tolist()
    path = tmp_path / "na_ids.txt"
    path.write_text("\n".join(ids) + "\n")
    return ids, str(path)


def _device_rows(gt, cv, ca, order, K, width=None):
    calls = torch.from_numpy(np.ascontiguousarray(gt)).cuda()
    X = Q.query_rows(calls, cv, ca, order, K)
    torch.cuda.synchronize()
    X = X.cpu().numpy()
    if width is not None:
        assert X.shape[1] == width
    return X


# ------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("N,P,K", [(100, 2, 200), (2000, 2, 300), (1001, 2, 77), (2049, 1, 130), (1536, 1, 64),
                                   (7, 3, 65)])
def test_kernel_matches_the_restatement(N, P, K):
    """Every load width of the kernel (16 / 8 / 4 bytes, and the per-sample form for odd rows and ploidy 3), N > 960 (several
    LDS sample chunks), K not a multiple of the 64-column tile, repeated and absent columns, multi-allelic targets, output
    rows in any order, row pitch Kp."""
    rng = np.random.default_rng(N * 7 + P + K)
    V = 150
    gt = rng.integers(-1, 4, (V, N, P)).astype(np.int8)
    cv = rng.integers(0, V, K).astype(np.int32)
    cv[rng.random(K) < 0.15] = -1
    cv[5:9] = cv[1]                                           # repeated columns
    ca = rng.integers(0, 4, K).astype(np.int8)
    order = rng.permutation(N)[: max(1, N - 13)].astype(np.int32)
    Kp = (K + 31) // 32 * 32
    X = _device_rows(gt, cv, ca, order, K, Kp)
    assert np.array_equal(X, query_rows_numpy(gt, cv, ca, order, width=Kp))


def test_kernel_haplotype_view_and_no_matched_variant():
    rng = np.random.default_rng(9)
    gt = rng.integers(-1, 2, (40, 1200, 2)).astype(np.int8)
    cv = rng.integers(-1, 40, 90).astype(np.int32)
    ca = np.ones(90, np.int8)
    order = rng.permutation(2400).astype(np.int32)
    calls = torch.from_numpy(gt).cuda().view(40, 2400, 1)
    X = Q.query_rows(calls, cv, ca, order, 90).cpu().numpy()
    assert np.array_equal(X, query_rows_numpy(gt.reshape(40, 2400, 1), cv, ca, order, width=96))
    empty = torch.zeros((0, 10, 2), dtype=torch.int8, device="cuda")
    X = Q.query_rows(empty, np.full(5, -1, np.int32), np.ones(5, np.int8), np.arange(10, dtype=np.int32), 5)
    assert X.shape == (10, 32) and not X.cpu().numpy().any()


# ------------------------------------------------------------------ 2. round trip on the example data
@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    d = tmp_path_factory.mktemp("query_train")
    common = ["--vcf", VCF, "--sample_data", SAMPLES, "--seed", "12345"] + SHORT
    _run(common + ["--out", str(d / "plain")])
    _run(common + ["--out", str(d / "kept"), "--keep_model"])
    return d


def test_round_trip_is_byte_identical(tmp_path, trained):
    d = trained
    for suffix in ("_predlocs.txt", "_history.txt"):              # --keep_model changes no other output
        assert (d / ("kept" + suffix)).read_bytes() == (d / ("plain" + suffix)).read_bytes(), suffix
    assert not (d / "plain.model.npz").exists() and (d / "kept.model.npz").exists()
    m = Q.load_model(str(d / "kept.model.npz"))
    assert m["params"]["keep_model"] is True and m["K"] == 5830 and set(m["chrom"]) == {"1"}
    ids, id_file = _na_ids(tmp_path)
    out = str(tmp_path / "q")
    assert P.main(["--model", str(d / "kept.model.npz"), "--vcf", VCF, "--samples", id_file, "--out", out]) == 0
    assert open(out + "_predlocs.txt", "rb").read() == (d / "kept_predlocs.txt").read_bytes()
    rep = pd.read_csv(out + "_sites.txt", sep="\t")
    assert rep.iloc[0].tolist() == ["kept", 5830, 5830, 0, 0]


# ------------------------------------------------------------------ 3. a perturbed query
def _write_vcf(path, samples, recs):
    with open(path, "w") as fh:
        fh.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(samples) + "\n")
        for chrom, pos, ref, alt, g in recs:
            calls = ["|".join("." if a < 0 else str(a) for a in call) for call in g]
            fh.write(f"{chrom}\t{pos}\t.\t{ref}\t{alt}\t.\tPASS\t.\tGT\t" + "\t".join(calls) + "\n")


@pytest.mark.parametrize("mode", ["exact", "auto"])
def test_perturbed_query(tmp_path, trained, mode):
    from oracle import locator_oracle as O
    rng = np.random.default_rng(2024)
    m = Q.load_model(str(trained / "kept.model.npz"))
    src = G.read_vcf(VCF, sites=True)
    gt = np.array(src["calldata/GT"], dtype=np.int8)
    V, N, _ = gt.shape
    pos = src["variants/POS"].astype(np.int64)
    samples = np.asarray(src["samples"]).astype(str)
    blank = rng.random((V, N)) < 0.02
    gt[blank] = -1                                             # 2 % of calls missing
    model_pos = set(m["pos"].tolist())
    model_rows = [v for v in range(V) if pos[v] in model_pos]
    dropped = set(rng.choice(model_rows, len(model_rows) // 5, replace=False).tolist())
    swapped = set(rng.choice(V, V // 10, replace=False).tolist())
    split = next(v for v in model_rows if v not in dropped and v not in swapped)
    perm = np.arange(N)
    perm[:60] = rng.permutation(60)                            # a subset of the samples reordered
    recs = []
    for v in range(V):
        if v in dropped:
            continue
        g = gt[v][perm]
        if v == split:                                         # A,T -> A,G,T: allele 1 becomes 2
            recs.append(("1", pos[v], "A", "G,T", np.where(g == 1, 2, g)))
        elif v in swapped:                                     # REF/ALT swapped, calls recoded
            recs.append(("1", pos[v], "T", "A", np.where(g >= 0, 1 - g, g)))
        else:
            recs.append(("1", pos[v], "A", "T", g))
    for i in range(400):                                       # unrelated sites
        recs.append(("2" if i % 2 else "1", 10_000_000 + i, "C", "G", rng.integers(0, 2, (N, 2))))
    recs = [recs[i] for i in rng.permutation(len(recs))]
    qpath = str(tmp_path / "query.vcf")
    _write_vcf(qpath, samples[perm], recs)
    ids, id_file = _na_ids(tmp_path)

    q = Q.read_query(vcf=qpath)
    cv, ca, rep = Q.match_sites(m, q)
    assert rep["absent"] == len(dropped) and rep["allele_not_1"] >= 1
    calls, (cvc,), _ = Q.compact_calls(q, [(cv, ca)])
    rows = Q.select_samples(q, ids).astype(np.int32)
    X = _device_rows(calls, cvc, ca, rows, m["K"])
    assert np.array_equal(X, query_rows_numpy(calls, cvc, ca, rows, width=X.shape[1]))
    # independent of the matcher: the allele-1 counts of the (blanked) source calls at every kept model site, 0 where dropped
    col_src = np.searchsorted(pos, m["pos"])
    src_rows = np.array([int(np.flatnonzero(samples == s)[0]) for s in ids])
    want = G.to_allele_counts_1(gt[col_src][:, src_rows]).T.astype(np.uint8)
    want[:, [p in {pos[v] for v in dropped} for p in m["pos"]]] = 0
    assert np.array_equal(X[:, :m["K"]], want)

    out = str(tmp_path / f"p_{mode}")
    assert P.main(["--model", str(trained / "kept.model.npz"), "--vcf", qpath, "--samples", id_file, "--out", out,
                   "--predict_mode", mode]) == 0
    got = pd.read_csv(out + "_predlocs.txt")
    assert got["sampleID"].astype(str).tolist() == ids
    meanlong, sdlong, meanlat, sdlat = m["locs_norm"]
    z = np.column_stack([(got["x"] - meanlong) / sdlong, (got["y"] - meanlat) / sdlat])
    ref = O.predict(Q.absent_gamma(m["weights"], cv), want.astype(np.float32))
    err = np.abs(z - ref).max()
    assert err <= (2e-5 if mode == "exact" else 1e-3 * np.abs(ref).max()), err
    assert pd.read_csv(out + "_sites.txt", sep="\t")["absent"].tolist() == [len(dropped)]


# ------------------------------------------------------------------ 4. model sets
def _same_file_as_summarize(pred_dir, out):
    """{out}_centroids.txt is byte for byte what `python -m locator_amd.summarize --infile <pred_dir>` writes."""
    theirs = str(pred_dir.parent / "summarize")
    assert S.main(["--infile", str(pred_dir), "--out", theirs, "--silence"]) == 0
    assert open(out + "_centroids.txt", "rb").read() == open(theirs + "_centroids.txt", "rb").read()


def test_bootstrap_models(tmp_path):
    train = tmp_path / "train"
    train.mkdir()
    _run(["--vcf", VCF, "--sample_data", SAMPLES, "--seed", "77", "--bootstrap", "--nboots", "3", "--keep_model",
          "--in_process", "--out", str(train / "b")] + SHORT)
    files = sorted(f for f in os.listdir(train) if f.endswith(".model.npz"))
    assert files == ["b_boot0.model.npz", "b_boot1.model.npz", "b_boot2.model.npz", "b_bootFULL.model.npz"]
    full = Q.load_model(str(train / "b_bootFULL.model.npz"))
    b1 = Q.load_model(str(train / "b_boot1.model.npz"))
    assert b1["K"] == full["K"] and len(set(b1["pos"].tolist())) < b1["K"]          # resampled sites repeat
    ids, id_file = _na_ids(tmp_path)
    pred = tmp_path / "pred"
    pred.mkdir()
    out = str(pred / "q")
    assert P.main(["--model", str(train), "--vcf", VCF, "--samples", id_file, "--out", out]) == 0
    for f in files:
        stem = f[:-len(".model.npz")]
        assert open(f"{out}_{stem}_predlocs.txt", "rb").read() == (train / f"{stem}_predlocs.txt").read_bytes(), stem
    _same_file_as_summarize(pred, out)
    assert len(pd.read_csv(out + "_sites.txt", sep="\t")) == 4


def test_windows_models_on_zarr(tmp_path):
    src = G.read_vcf(VCF, sites=True)
    store = str(tmp_path / "fix.zarr")
    G.write_callset_zarr(store, src["calldata/GT"], src["variants/POS"], src["samples"], chunk_variants=4096,
                         compressor="blosc", chrom=src["variants/CHROM"], ref=src["variants/REF"], alt=src["variants/ALT"])
    train = tmp_path / "train"
    train.mkdir()
    _run(["--zarr", store, "--sample_data", SAMPLES, "--seed", "4242", "--windows", "--window_size", "1250000",
          "--keep_model", "--in_process", "--out", str(train / "w")] + SHORT)
    files = sorted(f for f in os.listdir(train) if f.endswith(".model.npz"))
    assert len(files) == 2
    m0 = Q.load_model(str(train / files[0]))
    assert m0["pos"].max() < 1250000 and np.all(np.diff(m0["pos"]) > 0)
    ids, id_file = _na_ids(tmp_path)
    pred = tmp_path / "pred"
    pred.mkdir()
    out = str(pred / "q")
    assert P.main(["--model"] + [str(train / f) for f in files] + ["--zarr", store, "--samples", id_file, "--out", out]) == 0
    for f in files:
        stem = f[:-len(".model.npz")]
        trained = [t for t in os.listdir(train) if t.startswith(stem + "_") and t.endswith("_predlocs.txt")]
        assert len(trained) == 1
        assert open(f"{out}_{stem}_predlocs.txt", "rb").read() == (train / trained[0]).read_bytes(), stem
    _same_file_as_summarize(pred, out)


def test_phased_model(tmp_path):
    train = tmp_path / "train"
    train.mkdir()
    _run(["--vcf", VCF, "--sample_data", SAMPLES, "--seed", "12345", "--phased", "--keep_model", "--out",
          str(train / "h")] + SHORT)
    m = Q.load_model(str(train / "h.model.npz"))
    assert m["phased"] is True and m["ploidy"] == 2
    ids, id_file = _na_ids(tmp_path)
    out = str(tmp_path / "q")
    assert P.main(["--model", str(train / "h.model.npz"), "--vcf", VCF, "--samples", id_file, "--out", out]) == 0
    got = pd.read_csv(out + "_predlocs.txt")
    assert got["sampleID"].tolist() == [f"{s}_h{h}" for s in ids for h in (0, 1)]
    assert open(out + "_predlocs.txt", "rb").read() == (train / "h_predlocs.txt").read_bytes()
    # an unphased heterozygote in the query: refused before any device work
    lines = gzip.open(VCF, "rt").read().splitlines()
    k = next(i for i, ln in enumerate(lines) if not ln.startswith("#") and "\t0|1" in ln)
    lines[k] = lines[k].replace("\t0|1", "\t0/1", 1)
    bad = tmp_path / "unphased.vcf"
    bad.write_text("\n".join(lines) + "\n")
    with pytest.raises(SystemExit, match="without phase"):
        P.main(["--model", str(train / "h.model.npz"), "--vcf", str(bad), "--out", str(tmp_path / "bad")])
    assert not os.path.exists(str(tmp_path / "bad_predlocs.txt"))
