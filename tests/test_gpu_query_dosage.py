"""Kept models on imputed dosages, on the device: loc_query_rows_dosage against its NumPy restatement
(tests/test_query_dosage.py) byte for byte - both load forms, several sample chunks, a misaligned base, offsets past 2^31
bytes -, `predict --dosage` on a query whose DS is the GT count (63 x the hard-call rows, and the float64 oracle), a perturbed
noisy query (dropped, swapped, multi-allelic, shuffled records, reordered samples, unrelated sites) against an expectation
built from the source dosages, GP / zarr / matrix queries, a bootstrap model set, and `explain --dosage` against the float64
forms of locator_amd/explain.py."""
import os

import numpy as np
import pandas as pd
import pytest
import torch

from locator_amd import _lib
from locator_amd import explain as E
from locator_amd import genotypes as G
from locator_amd import locator as L
from locator_amd import predict as P
from locator_amd import query as Q
from locator_amd.net import _ptr, _stream
from oracle import locator_oracle as O
from tests.dosage_util import SAMPLES, VCF, noisy_dosage
from tests.test_gpu_query import SHORT, _device_rows, _run, _same_file_as_summarize
from tests.test_query_dosage import QMAX, query_rows_dosage_numpy

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ 1. the kernel
def _kernel_inputs(N, K, V=150):
    rng = np.random.default_rng(N * 7 + K)
    ds = rng.uniform(0, 2, (V, N)).astype(np.float32)
    ties = np.concatenate([[0.5, 1.5, 0.0, 2.0, 1.0], (rng.integers(0, 126, 40) + 0.5) / 63.0]).astype(np.float32)
    at = rng.random((V, N)) < 0.05
    ds[at] = rng.choice(ties, int(at.sum()))                          # exact ties of the rounding, and the end points
    out = rng.random((V, N)) < 0.01
    ds[out] = rng.choice(np.array([-0.0008, 2.0007, -1.0, 2.5, 300.0], np.float32), int(out.sum()))     # pins the clamp
    ds[rng.random((V, N)) < 0.05] = np.nan
    cv = rng.integers(0, V, K).astype(np.int32)
    cv[rng.random(K) < 0.15] = -1
    cv[5:9] = cv[1]                                                   # repeated columns
    cv[11] = V + 3                                                    # out of range: read as absent
    ca = rng.integers(0, 2, K).astype(np.int8)                        # random flips
    ca[13], ca[14] = 2, -1                                            # no such allele in a two-allele record
    order = rng.permutation(N)[: max(1, N - 13)].astype(np.int32)     # a partial permutation
    return ds, cv, ca, order


def _on_device(ds, misaligned=False):
    """The dosages as a contiguous device tensor; misaligned: its base 4 bytes past a 16-byte boundary."""
    if not misaligned:
        t = torch.from_numpy(np.ascontiguousarray(ds)).cuda()
        assert t.data_ptr() % 16 == 0
        return t
    buf = torch.empty(ds.size + 1, dtype=torch.float32, device="cuda")
    t = buf[1:].view(ds.shape)
    t.copy_(torch.from_numpy(ds))
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t


def _raw_rows(ds_dev, cv, ca, order, K, pitch, guard_rows=3):
    """loc_query_rows_dosage into a caller-owned buffer: 0xAB in the padding columns K .. pitch of every row and in guard_rows
    rows behind the last.  -> the whole buffer (n_out + guard_rows, pitch) on the host."""
    lib = _lib.load()
    n = len(order)
    X = torch.full((n + guard_rows, pitch), 0xAB, dtype=torch.uint8, device="cuda")
    X[:n, :K] = 0x77                                                  # every element of the result must be written
    d = lambda a, t: torch.from_numpy(np.ascontiguousarray(a, dtype=t)).cuda()
    so, dcv, dca = d(order, np.int32), d(cv, np.int32), d(ca, np.int8)
    U, N = ds_dev.shape
    _lib.check(lib.loc_query_rows_dosage(_ptr(ds_dev), U, N, _ptr(dcv), _ptr(dca), K, _ptr(so), n, _ptr(X), pitch, _stream()),
               "loc_query_rows_dosage")
    torch.cuda.synchronize()
    return X.cpu().numpy()


@pytest.mark.parametrize("N,K,misaligned", [(100, 200, False), (2000, 300, False), (1001, 77, False), (963, 64, False),
                                            (1536, 130, True)],
                         ids=["float4-one-chunk", "float4-three-chunks", "scalar-odd-row", "scalar-3-sample-tail",
                              "scalar-misaligned-base"])
def test_kernel_matches_the_restatement(N, K, misaligned):
    ds, cv, ca, order = _kernel_inputs(N, K)
    ds_dev = _on_device(ds, misaligned)
    Kp = (K + 31) // 32 * 32
    want = query_rows_dosage_numpy(ds, cv, ca, order, width=Kp)
    assert want[:, :K].max() == QMAX and len(np.unique(want)) > 100 and not want[:, K:].any()
    X = Q.query_rows_dosage(ds_dev, cv, ca, order, K)
    torch.cuda.synchronize()
    assert X.shape == (len(order), Kp) and X.dtype == torch.uint8
    assert np.array_equal(X.cpu().numpy(), want)                      # padding columns K .. Kp stay zero
    pitch = Kp + 32
    raw = _raw_rows(ds_dev, cv, ca, order, K, pitch)
    n = len(order)
    assert np.array_equal(raw[:n, :K], want[:, :K])
    assert (raw[:n, K:] == 0xAB).all() and (raw[n:] == 0xAB).all()    # columns K .. pitch and the rows behind: untouched


def test_kernel_empty_cases_and_bad_arguments():
    lib = _lib.load()
    order = np.arange(10, dtype=np.int32)
    empty = torch.zeros((0, 10), dtype=torch.float32, device="cuda")
    X = Q.query_rows_dosage(empty, np.full(5, -1, np.int32), np.ones(5, np.int8), order, 5)       # no matched variant
    assert X.shape == (10, 32) and not X.cpu().numpy().any()
    ds = torch.ones((3, 10), dtype=torch.float32, device="cuda")
    X = Q.query_rows_dosage(ds, np.zeros(0, np.int32), np.zeros(0, np.int8), order, 0)             # K == 0
    assert X.shape == (10, 32) and not X.cpu().numpy().any()
    X = Q.query_rows_dosage(ds, np.array([1, 2], np.int32), np.ones(2, np.int8), order[:0], 2)     # n_out == 0
    assert X.shape == (0, 32)
    # bad arguments: -1, the reason in loc_last_error, nothing launched (the sentinel stays)
    buf = torch.full((10, 32), 0xAB, dtype=torch.uint8, device="cuda")
    cv = torch.zeros(40, dtype=torch.int32, device="cuda")
    ca = torch.ones(40, dtype=torch.int8, device="cuda")
    so = torch.from_numpy(order).cuda()
    for U, N, K, n_out, pitch, p_ds in ((3, 10, 40, 10, 32, _ptr(ds)),        # x_pitch < K
                                        (3, 0, 2, 10, 32, _ptr(ds)),          # no samples
                                        (-1, 10, 2, 10, 32, _ptr(ds)),
                                        (3, 10, 2, -1, 32, _ptr(ds)),
                                        (3, 10, 2, 10, 32, None)):            # variants without a matrix
        assert lib.loc_query_rows_dosage(p_ds, U, N, _ptr(cv), _ptr(ca), K, _ptr(so), n_out, _ptr(buf), pitch, _stream()) == -1
        assert b"loc_query_rows_dosage" in lib.loc_last_error()
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 0xAB).all()


@pytest.mark.parametrize("N", [1048580, 1048581], ids=["float4", "scalar"])
def test_kernel_past_2_31_bytes_of_dosages(N):
    """ds of 2.26 GB generated on the device; 70 columns into the variants whose rows start past 2^31 bytes (and two in front),
    8 output rows from every part of a row.  The same formula in torch on the gathered rows is the reference."""
    V, K = 540, 70
    assert (V - 27) * N * 4 > 2 ** 31
    g = torch.Generator(device="cuda").manual_seed(N)
    ds = torch.empty((V, N), dtype=torch.float32, device="cuda").uniform_(-0.05, 2.05, generator=g)
    rng = np.random.default_rng(N)
    cv = rng.integers(V - 27, V, K).astype(np.int32)
    cv[:4] = [V - 1, 0, 7, -1]
    ca = rng.integers(0, 2, K).astype(np.int8)
    order = np.array([N - 1, 0, 959, 960, N // 2 + 1, N - 962, 123456, N - 2], np.int32)
    ds[V - 1, N - 1] = float("nan")
    ds[V - 1, 0] = 1.5
    ds[V - 2, N - 2] = 0.5
    X = Q.query_rows_dosage(ds, cv, ca, order, K)
    torch.cuda.synchronize()
    cols = torch.from_numpy(np.where(cv < 0, 0, cv).astype(np.int64)).cuda()
    d = ds[cols][:, torch.from_numpy(order.astype(np.int64)).cuda()]              # (K, 8)
    q = torch.clamp(torch.round(d * 63.0), 0, QMAX)                               # fp32 product; half to even
    flip = torch.from_numpy(ca == 0).cuda()[:, None]
    want = torch.where(flip, QMAX - q, q)
    want = torch.where(torch.isnan(d) | torch.from_numpy(cv < 0).cuda()[:, None], torch.zeros_like(want), want)
    want = want.T.to(torch.uint8).cpu().numpy()
    got = X.cpu().numpy()
    del ds, X
    torch.cuda.empty_cache()
    assert got.shape == (8, 96) and np.array_equal(got[:, :K], want) and not got[:, K:].any()
    assert got[0, 0] == 0 and got[1, 0] == (94 if ca[0] == 1 else 32) and len(np.unique(want)) > 60


# ------------------------------------------------------------------ 2. models trained on the example data
def _na_ids():
    t = pd.read_csv(SAMPLES, sep="\t")
    return t.loc[t["x"].isna(), "sampleID"].astype(str).tolist()


def _fmt_row(row, field):
    if field == "DS":
        return ["." if np.isnan(x) else f"{float(x):.4f}" for x in row]
    out = []
    for x in row:                                # d = p1 + 2 p2 with p2 = max(0, d - 1), as tests/dosage_util.py writes GP
        if np.isnan(x):
            out.append(".")
            continue
        p2 = max(0.0, float(x) - 1.0)
        p1 = float(x) - 2 * p2
        out.append(f"{1 - p1 - p2:.6f},{p1:.6f},{p2:.6f}")
    return out


def _write_vcf(path, samples, recs, field="DS"):
    """recs: (chrom, pos, ref, alt, dosages of every sample) in file order."""
    with open(path, "w") as fh:
        fh.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(samples) + "\n")
        for chrom, pos, ref, alt, row in recs:
            fh.write(f"{chrom}\t{pos}\t.\t{ref}\t{alt}\t.\tPASS\t.\t{field}\t" + "\t".join(_fmt_row(row, field)) + "\n")


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """One model kept from the example data (as tests/test_gpu_query.py trains it), the source calls, and two query files over
    120 of the samples (the 50 without a location among them): DS = the GT allele-1 count, and the perturbed noisy query."""
    d = tmp_path_factory.mktemp("query_dosage_train")
    _run(["--vcf", VCF, "--sample_data", SAMPLES, "--seed", "12345", "--keep_model", "--out", str(d / "kept")] + SHORT)
    m = Q.load_model(str(d / "kept.model.npz"))
    src = G.read_vcf(VCF, sites=True)
    gt = np.array(src["calldata/GT"], dtype=np.int8)
    pos = src["variants/POS"].astype(np.int64)
    samples = np.asarray(src["samples"]).astype(str)
    ids = _na_ids()
    rng = np.random.default_rng(2025)
    na = np.array([int(np.flatnonzero(samples == s)[0]) for s in ids])
    others = rng.choice(np.setdiff1d(np.arange(len(samples)), na), 70, replace=False)
    sub = np.sort(np.concatenate([na, others]))                       # file order of the source
    (d / "ids.txt").write_text("\n".join(ids) + "\n")
    rows_v = np.searchsorted(pos, m["pos"])                           # the source variant of every model site
    assert (pos[rows_v] == m["pos"]).all() and len(set(m["pos"].tolist())) == m["K"]
    counts = (gt[rows_v][:, sub] == 1).sum(axis=2).astype(np.float32)          # (K, 120)
    _write_vcf(str(d / "counts.vcf"), samples[sub], [("1", p, "A", "T", c) for p, c in zip(m["pos"], counts)])
    gq = {"kind": "vcf", "gt": np.ascontiguousarray(gt[rows_v][:, sub]), "chrom": np.array(["1"] * m["K"]), "pos": m["pos"],
          "alleles": [["A", "T"]] * m["K"], "samples": samples[sub], "unphased_hets": 0}

    # ---- the perturbed query: noisy dosages, 2 % missing; values as the file prints them (4 decimals)
    K = m["K"]
    noisy = noisy_dosage(counts, seed=11, missing=0.02)
    dropped = rng.choice(K, K // 5, replace=False)
    state = np.zeros(K, np.int8)                                      # 0 kept, 1 dropped, 2 swapped, 3 multi-allelic
    state[dropped] = 1
    rest = np.flatnonzero(state == 0)
    state[rng.choice(rest, K // 10, replace=False)] = 2
    state[np.flatnonzero(state == 0)[17]] = 3
    perm = np.arange(len(sub))
    perm[:60] = rng.permutation(60)                                   # a subset of the samples reordered
    recs, stored = [], np.array(noisy)
    for k in range(K):
        if state[k] == 1:
            continue
        if state[k] == 2:                                             # REF/ALT swapped, DS written as 2 - DS
            stored[k] = [np.nan if np.isnan(x) else np.float32(round(2.0 - float(x), 4)) for x in noisy[k]]
            recs.append(("1", m["pos"][k], "T", "A", stored[k][perm]))
        elif state[k] == 3:                                           # a second ALT allele: the reader drops the record
            recs.append(("1", m["pos"][k], "A", "T,G", stored[k][perm]))
        else:
            recs.append(("1", m["pos"][k], "A", "T", stored[k][perm]))
    for i in range(400):                                              # unrelated sites
        recs.append(("2" if i % 2 else "1", 10_000_000 + i, "C", "G", rng.uniform(0, 2, len(sub)).astype(np.float32)))
    recs = [recs[i] for i in rng.permutation(len(recs))]
    _write_vcf(str(d / "noisy.vcf"), samples[sub][perm], recs)
    _write_vcf(str(d / "noisy_gp.vcf"), samples[sub][perm], recs[:1500], field="GP")
    # the expectation, from the source dosages alone: q of what the file holds, flipped where the record is swapped
    src_rows = np.array([int(np.flatnonzero(samples[sub] == s)[0]) for s in ids])
    dq = G.dosage_q(stored[:, src_rows])                              # (K, 50); 255 = missing
    want = np.where(dq == G.Q_MISSING, 0, np.where((state == 2)[:, None], QMAX - dq.astype(np.int32), dq)).astype(np.uint8)
    want[(state == 1) | (state == 3)] = 0
    return {"dir": d, "model": str(d / "kept.model.npz"), "m": m, "ids": ids, "id_file": str(d / "ids.txt"),
            "counts": counts, "gt_query": gq, "sub_samples": samples[sub], "state": state, "want": want.T.copy(),
            "recs": recs, "perm_samples": samples[sub][perm]}


def _z_of(path, m, ids):
    got = pd.read_csv(path)
    assert got["sampleID"].astype(str).tolist() == ids
    meanlong, sdlong, meanlat, sdlat = m["locs_norm"]
    return np.column_stack([(got["x"] - meanlong) / sdlong, (got["y"] - meanlat) / sdlat])


def _bar(mode, ref):
    """The project's bars (tests/test_gpu_query.py::test_perturbed_query, test_every_predict_route_at_q_up_to_126)."""
    return 2e-5 if mode == "exact" else 1e-3 * np.abs(ref).max()


def test_dosage_of_the_hard_call_count_gives_63_times_the_call_rows(trained):
    m, ids = trained["m"], trained["ids"]
    q = Q.read_query_dosage(vcf=str(trained["dir"] / "counts.vcf"))
    cv, ca, rep = Q.match_sites(m, q)
    assert rep["matched"] == m["K"] and rep["allele_not_1"] == 0
    Q.check_query_dosage(m, q, rep)
    ds, (cvc,), _ = Q.compact_dosages(q, [(cv, ca)])
    rows = Q.select_samples(q, ids).astype(np.int32)
    X = Q.query_rows_dosage(torch.from_numpy(ds).cuda(), cvc, ca, rows, m["K"]).cpu().numpy()
    gq = trained["gt_query"]
    gcv, gca, _ = Q.match_sites(m, gq)
    calls, (gcvc,), _ = Q.compact_calls(gq, [(gcv, gca)])
    Xg = _device_rows(calls, gcvc, gca, rows, m["K"])
    assert Xg.max() == 2 and np.array_equal(X, 63 * Xg)


@pytest.mark.parametrize("mode", ["exact", "auto"])
def test_predict_on_the_hard_call_count_matches_the_oracle(tmp_path, trained, mode):
    m, ids = trained["m"], trained["ids"]
    out = str(tmp_path / f"c_{mode}")
    assert P.main(["--model", trained["model"], "--vcf", str(trained["dir"] / "counts.vcf"), "--dosage", "--samples",
                   trained["id_file"], "--out", out, "--predict_mode", mode]) == 0
    z = _z_of(out + "_predlocs.txt", m, ids)
    src_rows = [int(np.flatnonzero(trained["sub_samples"] == s)[0]) for s in ids]
    x = trained["counts"][:, src_rows].T.astype(np.float64)
    ref = O.predict(O.cast_params(m["weights"], np.float64), x)
    err = np.abs(z - ref).max()
    print(f"predict --dosage on DS = count, {mode}: max |dz| {err:.3e}, max |ref| {np.abs(ref).max():.3f}")
    assert err <= _bar(mode, ref), err
    assert pd.read_csv(out + "_sites.txt", sep="\t").iloc[0].tolist() == ["kept", m["K"], m["K"], 0, 0]


def test_perturbed_query_rows(trained):
    m, ids, state = trained["m"], trained["ids"], trained["state"]
    q = Q.read_query_dosage(vcf=str(trained["dir"] / "noisy.vcf"))
    assert q["multiallelic_dropped"] == 1
    cv, ca, rep = Q.match_sites(m, q)
    n_absent = int(((state == 1) | (state == 3)).sum())
    assert rep["absent"] == n_absent and rep["allele_not_1"] == int((state == 2).sum()) and rep["matched"] == m["K"] - n_absent
    ds, (cvc,), _ = Q.compact_dosages(q, [(cv, ca)])
    rows = Q.select_samples(q, ids).astype(np.int32)
    X = Q.query_rows_dosage(torch.from_numpy(ds).cuda(), cvc, ca, rows, m["K"]).cpu().numpy()
    assert np.array_equal(X, query_rows_dosage_numpy(ds, cvc, ca, rows, width=X.shape[1]))
    want = trained["want"]
    assert np.array_equal(X[:, :m["K"]], want) and not X[:, m["K"]:].any()
    assert (want[:, state == 2] > 0).any() and len(np.unique(want)) > 50


@pytest.mark.parametrize("mode", ["exact", "auto"])
def test_perturbed_query_predictions(tmp_path, trained, mode):
    m, ids, state = trained["m"], trained["ids"], trained["state"]
    out = str(tmp_path / f"p_{mode}")
    assert P.main(["--model", trained["model"], "--vcf", str(trained["dir"] / "noisy.vcf"), "--dosage", "DS", "--samples",
                   trained["id_file"], "--out", out, "--predict_mode", mode]) == 0
    z = _z_of(out + "_predlocs.txt", m, ids)
    present = np.where((state == 1) | (state == 3), -1, 0).astype(np.int32)
    p = O.cast_params(Q.absent_gamma(m["weights"], present), np.float64)
    ref = O.predict(p, trained["want"].astype(np.float64) / 63.0)
    err = np.abs(z - ref).max()
    print(f"predict --dosage on the perturbed query, {mode}: max |dz| {err:.3e}, max |ref| {np.abs(ref).max():.3f}")
    assert err <= _bar(mode, ref), err
    n_absent = int((present < 0).sum())
    assert pd.read_csv(out + "_sites.txt", sep="\t").iloc[0].tolist() == [
        "kept", m["K"], m["K"] - n_absent, int((state == 2).sum()), n_absent]


def _host_rows(q, cv, ca, rows):
    """The rows from the host's fixed-point form genotypes.dosage_q of the query's dosages."""
    dq = G.dosage_q(q["ds"])
    X = np.zeros((len(rows), len(cv)), np.uint8)
    for k in np.flatnonzero(cv >= 0):
        col = dq[cv[k]][rows]
        X[:, k] = np.where(col == G.Q_MISSING, 0, col if ca[k] == 1 else QMAX - col.astype(np.int32))
    return X


def _rows_of(m, q, ids=None):
    cv, ca, rep = Q.match_sites(m, q)
    ds, (cvc,), _ = Q.compact_dosages(q, [(cv, ca)])
    rows = Q.select_samples(q, ids).astype(np.int32)
    X = Q.query_rows_dosage(torch.from_numpy(ds).cuda(), cvc, ca, rows, m["K"]).cpu().numpy()
    return X[:, :m["K"]], _host_rows(q, cv, ca, rows), rep


def test_gp_zarr_and_matrix_queries_give_the_host_fixed_point_rows(tmp_path, trained):
    m, ids = trained["m"], trained["ids"]
    X, host, rep = _rows_of(m, Q.read_query_dosage(vcf=str(trained["dir"] / "noisy_gp.vcf"), field="GP"), ids)
    assert 500 < rep["matched"] < 1500 and rep["allele_not_1"] > 20 and np.array_equal(X, host) and len(np.unique(X)) > 50
    # the same records as a zarr store (the multi-allelic record keeps both ALT alleles there: unmatched)
    recs = [r for r in trained["recs"][:1500]]
    alt = np.array([(r[3].split(",") + [""])[:2] for r in recs])
    store = str(tmp_path / "q.zarr")
    G.write_callset_zarr(store, np.zeros((len(recs), len(trained["perm_samples"]), 2), np.int8), [r[1] for r in recs],
                         trained["perm_samples"], chunk_variants=512, compressor="blosc", chrom=[r[0] for r in recs],
                         ref=[r[2] for r in recs], alt=alt)
    G.write_dosage_zarr(store, np.stack([r[4] for r in recs]), chunk_variants=512, compressor="blosc")
    Xz, hostz, repz = _rows_of(m, Q.read_query_dosage(zarr=store), ids)
    assert repz["matched"] == rep["matched"] and repz["allele_not_1"] == rep["allele_not_1"] and np.array_equal(Xz, hostz)
    # GP prints six decimals of each probability: the two files agree to a fixed-point step
    assert np.abs(Xz.astype(int) - X).max() <= 1
    # a float matrix: sites matched by name (a VCF model's name is its CHROM: every column takes the first "1")
    mat = tmp_path / "q.txt"
    names = ["x0", "1", "x2", "1"]
    vals = np.stack([r[4] for r in recs[:4]], axis=1)                              # (120, 4)
    with open(mat, "w") as fh:
        fh.write("sampleID\t" + "\t".join(names) + "\n")
        for s, row in zip(trained["perm_samples"], vals):
            fh.write(s + "\t" + "\t".join("NA" if np.isnan(x) else f"{float(x):.4f}" for x in row) + "\n")
    qm = Q.read_query_dosage(matrix=str(mat))
    Xm, hostm, repm = _rows_of(m, qm, ids)
    assert repm["matched"] == m["K"] and np.array_equal(Xm, hostm) and (Xm == Xm[:, :1]).all()
    printed = np.array([np.nan if np.isnan(x) else np.float32(f"{float(x):.4f}") for x in vals[:, 1]], np.float32)
    want = np.where(np.isnan(printed), 0, np.rint(printed * np.float32(63)))
    order = [int(np.flatnonzero(trained["perm_samples"] == s)[0]) for s in ids]
    assert Xm[:, 0].tolist() == want[order].astype(np.uint8).tolist()


def test_bootstrap_model_set(tmp_path, trained):
    train = tmp_path / "train"
    train.mkdir()
    _run(["--vcf", VCF, "--sample_data", SAMPLES, "--seed", "77", "--bootstrap", "--nboots", "2", "--keep_model",
          "--in_process", "--out", str(train / "b")] + SHORT)
    files = sorted(f for f in os.listdir(train) if f.endswith(".model.npz"))
    assert files == ["b_boot0.model.npz", "b_boot1.model.npz", "b_bootFULL.model.npz"]
    b1 = Q.load_model(str(train / "b_boot1.model.npz"))
    assert len(set(b1["pos"].tolist())) < b1["K"]                                  # resampled sites repeat
    pred = tmp_path / "pred"
    pred.mkdir()
    out = str(pred / "q")
    assert P.main(["--model", str(train), "--vcf", str(trained["dir"] / "noisy.vcf"), "--dosage", "--samples",
                   trained["id_file"], "--out", out, "--impute_missing", "--seed", "5"]) == 0
    _same_file_as_summarize(pred, out)
    rep = pd.read_csv(out + "_sites.txt", sep="\t")
    assert len(rep) == 3 and (rep["absent"] > 0).all() and (rep["allele_not_1"] > 0).all()
    for f in files:
        t = pd.read_csv(f"{out}_{f[:-len('.model.npz')]}_predlocs.txt")
        assert t["sampleID"].astype(str).tolist() == trained["ids"] and np.isfinite(t[["x", "y"]].to_numpy()).all()
    # the same seed draws the same imputed values: byte-identical files
    out2 = str(tmp_path / "again")
    assert P.main(["--model", str(train), "--vcf", str(trained["dir"] / "noisy.vcf"), "--dosage", "--samples",
                   trained["id_file"], "--out", out2, "--impute_missing", "--seed", "5"]) == 0
    for f in os.listdir(pred):
        assert open(pred / f, "rb").read() == open(out2 + f[1:], "rb").read(), f


# ------------------------------------------------------------------ 3. explain --dosage
STATS = list(E.STATS)


def _table(path):
    return pd.read_csv(path, sep="\t", dtype={"chrom": str})


def test_explain_on_the_perturbed_query(tmp_path, trained):
    m, state = trained["m"], trained["state"]
    out = str(tmp_path / "e")
    assert E.main(["--model", trained["model"], "--vcf", str(trained["dir"] / "noisy.vcf"), "--dosage", "--samples",
                   trained["id_file"], "--out", out]) == 0
    t = _table(out + "_snp_importance.txt")
    absent = (state == 1) | (state == 3)
    col_site, first = E.site_index(m)
    assert len(first) == m["K"] and (t["pos"].to_numpy() == m["pos"]).all() and (t["present"].to_numpy() == ~absent).all()
    p = O.cast_params(Q.absent_gamma(m["weights"], np.where(absent, -1, 0)), np.float64)
    x = trained["want"].astype(np.float64) / 63.0                                  # the dosage d = q / 63
    d1 = E.reference_delta1(p, x, m["locs_norm"])
    _, ref = E.reference_stats(d1, E.fold_first_layer(p, col_site, len(first)), x[:, first], p["mov_mean"][first])
    got = t[STATS].to_numpy().T
    print("explain --dosage: max relative error per statistic",
          (np.abs(got - ref) / (np.abs(ref) + 1e-7 * np.abs(ref).max())).max(axis=1))
    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-7 * np.abs(ref).max())
    assert (got[:, absent] == 0).all() and (got[3, ~absent] > 0).all()


def test_explain_rms_grad_is_that_of_the_hard_call_run(tmp_path, trained):
    """DS = the GT count puts the same rows through the same network: the Jacobian per allele copy, hence rms_grad, is that of
    the GT run (a missing factor of 63 would show here), and so are the attributions."""
    gt_vcf = str(tmp_path / "gt.vcf")
    gq = trained["gt_query"]
    with open(gt_vcf, "w") as fh:
        fh.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(gq["samples"]) + "\n")
        for p, g in zip(gq["pos"], gq["gt"]):
            fh.write(f"1\t{p}\t.\tA\tT\t.\tPASS\t.\tGT\t" + "\t".join(f"{a}|{b}" for a, b in g) + "\n")
    a, b = str(tmp_path / "gt"), str(tmp_path / "ds")
    common = ["--model", trained["model"], "--samples", trained["id_file"]]
    assert E.main(common + ["--vcf", gt_vcf, "--out", a]) == 0
    assert E.main(common + ["--vcf", str(trained["dir"] / "counts.vcf"), "--dosage", "--out", b]) == 0
    ta, tb = _table(a + "_snp_importance.txt"), _table(b + "_snp_importance.txt")
    assert (ta["present"] == 1).all() and (tb["present"] == 1).all()
    ref, got = ta[STATS].to_numpy().T, tb[STATS].to_numpy().T
    assert ref[3].min() > 0
    np.testing.assert_allclose(got[3], ref[3], rtol=1e-4, atol=1e-7 * np.abs(ref[3]).max())
    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-7 * np.abs(ref).max())
