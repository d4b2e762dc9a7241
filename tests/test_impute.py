"""The impute command without a GPU: the binding through _abi's table, the NumPy definition (the exact posterior by
enumeration, the closed form without linkage, the split at a certain switch, the structural NaNs, ll and n_donors of copy_host),
the quality of the dose against the donors' allele frequency, the --host command in fill and panel mode, the refusals."""
import ctypes as C
import itertools
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from locator_amd import genotypes as G
from locator_amd import impute as IM
from locator_amd import paint as PT
from locator_amd import query as Q
from tests import impute_util as IU
from tests import paint_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the binding
def test_the_table_binds_the_impute_header():
    from tests.abi_util import check_extension
    vp, i64, i, f = C.c_void_p, C.c_int64, C.c_int, C.c_float
    want = {"loc_impute_dose": (i, [vp, i, i64, i64, vp, vp, vp, i, vp, f, i, vp, vp, vp, vp, i64, vp])}
    check_extension("impute", want, {"LOC_IMPUTE_STORE_RUN": 64})


def test_a_later_header_that_declares_what_it_may_not_is_refused_by_name(tmp_path):
    pkg = tmp_path / "locator_amd"
    pkg.mkdir()
    (pkg / "__init__.py").write_text("")
    shutil.copy(os.path.join(ROOT, "locator_amd", "_abi.py"), pkg / "_abi.py")
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "include")
    run = lambda: subprocess.run([sys.executable, "-c", "import locator_amd._abi"], cwd=tmp_path, capture_output=True, text=True)
    assert run().returncode == 0
    path = tmp_path / "include" / "locator_hip_impute.h"
    text = path.read_text()
    for addition, named in (("int loc_paint_copy(int N);", "loc_paint_copy"),       # a function of an earlier header
                            ("int loc_version(void);", "loc_version"),              # a function of the main header
                            ("#define LOC_PAINT_TILE 2", "LOC_PAINT_TILE"),         # a constant outside its prefix
                            ("#define LOC_IMPUTE_TILE 2.5", "LOC_IMPUTE_TILE")):    # no integer
        path.write_text(text + "\n" + addition + "\n")
        r = run()
        assert r.returncode != 0 and "ValueError" in r.stderr and str(path) + " may declare" in r.stderr and named in r.stderr, addition
    path.write_text(text)
    assert run().returncode == 0


# ------------------------------------------------------------------ dose_host
def _exact_dose(h, rho, theta):
    """The dose of recipient column 0 from the donors 1 .. D by enumerating every donor path."""
    K, D = h.shape[0], h.shape[1] - 1
    u = 1.0 / D
    emit = lambda j, d: 1.0 if h[j, 0] < 0 or h[j, d] < 0 else (1 - theta if h[j, 0] == h[j, d] else theta)
    at = np.zeros((K, D))
    for path in itertools.product(range(D), repeat=K):
        p = u * emit(0, path[0] + 1)
        for j in range(1, K):
            p *= ((1 - rho[j]) * (path[j] == path[j - 1]) + rho[j] * u) * emit(j, path[j] + 1)
        for j in range(K):
            at[j, path[j]] += p
    a1 = np.where(h[:, 1:] == 1, at, 0).sum(axis=1)
    a0 = np.where(h[:, 1:] == 0, at, 0).sum(axis=1)
    return a1 / (a0 + a1)


def test_the_dose_is_the_exact_posterior_of_all_donor_paths():
    h = np.array([[1, 1, 0, 1], [-1, 0, 1, 1], [0, 0, -1, 1], [-1, 1, 1, 0], [1, 0, 1, 1]], dtype=np.int8)   # a missing recipient and donor allele
    rho = np.array([0.5, 0.3, 0.0, 1.0, 0.3])                                     # rho[0] counts as 1
    donor, owner = np.ones(4, dtype=np.uint8), np.arange(4, dtype=np.int32)
    for theta in (0.01, 0.2):
        dose, ll, nd = IM.dose_host(h, donor, owner, [0], rho, theta)
        assert nd.tolist() == [3] and np.abs(dose[0] - _exact_dose(h, rho, theta)).max() < 1e-12


def test_without_linkage_the_dose_is_the_closed_form():
    case = U.edge_case(20, 15, 2, 0.05)
    case["rho"] = np.ones(15)
    dose, ll, nd = IU.host(case, np.float64)
    dn = (case["donor"][None, :] != 0) & (case["owner"][None, :] != case["owner"][case["rec"]][:, None])
    for j in range(15):
        e = PT.emissions(case["h"], j, case["rec"], dn, 0.05, np.float64)
        x = case["h"][j][None, :]
        with np.errstate(invalid="ignore"):
            want = np.where(x == 1, e, 0).sum(axis=1) / np.where(x >= 0, e, 0).sum(axis=1)
        assert np.array_equal(np.isnan(want), np.isnan(dose[:, j]))
        assert np.abs(dose[:, j] - want)[~np.isnan(want)].max(initial=0) < 1e-14


def test_a_certain_switch_splits_the_problem_and_the_forward_pass_is_copy_hosts():
    H, K, cut = 24, 30, 13
    case = U.planted_case(H, K, 9)
    case["rho"] = np.full(K, 0.07)
    case["rho"][cut] = 1.0
    whole = IU.host(case, np.float64)
    parts = []
    for a, b in ((0, cut), (cut, K)):
        part = dict(case)
        part["h"], part["rho"] = case["h"][a:b], case["rho"][a:b]
        parts.append(IU.host(part, np.float64))
    assert np.abs(whole[0] - np.concatenate([p[0] for p in parts], axis=1)).max() < 1e-12
    assert whole[0].min() >= 0 and whole[0].max() <= 1 and whole[0].shape == (len(case["rec"]), K)
    for dtype in (np.float64, np.float32):
        for c in (case, U.edge_case(30, 40, 4, 0.01)):
            dose, ll, nd = IU.host(c, dtype)
            share, chunks, ll_copy, nd_copy = IU.copy_host(c, dtype)
            assert dose.dtype == dtype and np.array_equal(ll, ll_copy) and np.array_equal(nd, nd_copy)


def test_nan_is_structural_and_rows_without_a_donor_are_nan():
    for case in (U.edge_case(30, 40, 4, 0.01), U.edge_case(4, 9, 1, 0.5), U.planted_case(30, 40, 4)):
        want = IU.structural_nan(case)
        for dtype in (np.float64, np.float32):
            dose, ll, nd = IU.host(case, dtype)
            assert np.array_equal(np.isnan(dose), want)
            assert want[nd == 0].all() and not ll[nd == 0].any()
            assert np.nanmin(dose) >= 0 and np.nanmax(dose) <= 1
    case = U.edge_case(30, 40, 4, 0.01)
    assert IU.structural_nan(case)[:, 20].all() and (IU.host(case, np.float64)[2] == 0).any()      # the all-missing site, a D = 0 row
    case = U.no_switch_case()
    assert not np.isnan(IU.host(case, np.float64)[0]).any() and not np.isnan(IU.host(case, np.float32)[0]).any()
    empty = IM.dose_host(np.zeros((0, 8), dtype=np.int8), *U.everyone(4), np.zeros(0), 0.01)
    assert empty[0].shape == (8, 0) and not empty[1].any() and not empty[2].any()
    none = IM.dose_host(np.zeros((5, 8), dtype=np.int8), *U.everyone(4)[:2], [], np.zeros(5), 0.01)
    assert none[0].shape == (0, 5) and none[1].shape == none[2].shape == (0,)


# ------------------------------------------------------------------ quality
def test_filled_alleles_beat_the_donors_frequency_by_half():
    """planted 40 x 300, seed 2, 10 % hidden from everyone, rho = 0.05: mean squared error 0.0509 (concordance 0.934) against
    0.2215 of the donors' allele frequency; float32 within 2.5e-7 of float64."""
    truth, seen, hidden = IU.hidden_fill(2, 0.10)
    args = IU.fill_arguments(seen)
    dose = IM.dose_host(*args)[0]
    dose32 = IM.dose_host(*args, dtype=np.float32)[0]
    model, freq = IU.mse_against(dose, IM.donor_frequency(seen, np.arange(seen.shape[1])), truth, hidden)
    print(f"fill, 10 % hidden: mse {model:.4f} against {freq:.4f} of the frequency; float32 within {IU.distance(dose32, dose):.3g}")
    assert not np.isnan(dose).any() and model <= 0.5 * freq and IU.distance(dose32, dose) < 1e-5


def test_untyped_sites_of_a_panel_beat_the_panels_frequency_by_half():
    """30 panel samples, 10 targets typed at every 4th site, seed 2, rho = 0.05: mean squared error at the untyped sites 0.0904
    against 0.2232 of the panel's allele frequency."""
    truth, untyped, args = IU.panel_arguments(2)
    dose = IM.dose_host(*args)[0]
    at = np.broadcast_to(untyped[:, None], truth.shape)
    model, freq = IU.mse_against(dose, IM.donor_frequency(args[0], np.arange(60)), truth, at)
    print(f"panel, every 4th site typed: mse {model:.4f} against {freq:.4f} of the panel's frequency")
    assert not np.isnan(dose).any() and model <= 0.5 * freq


# ------------------------------------------------------------------ the command
FILES = ("_imputed.zarr", "_impute_summary.json", "_impute_history.txt")


def _read_store(path):
    callset = G.open_group(path, mode="r")
    ds = G.check_dosage(np.asarray(G.zarr_dosage(callset, path)[:]), path)
    q = Q.read_query_dosage(zarr=path)
    assert np.array_equal(q["ds"], ds, equal_nan=True)
    return np.asarray(callset["calldata/GT"][:]), np.asarray(callset["calldata/DS"][:]), q


def _tree(path):
    return {os.path.relpath(os.path.join(d, f), path): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(path) for f in fs}


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    return IU.planted_store(str(tmp_path_factory.mktemp("impute") / "planted.zarr"))


@pytest.fixture(scope="module")
def cut(tmp_path_factory):
    return U.write_vcf_cut(str(tmp_path_factory.mktemp("impute") / "cut.vcf"), 40, 60, 300)


def test_the_host_command_fills_a_planted_store(planted, tmp_path):
    store, hap = planted
    outs = [str(tmp_path / n) for n in ("a", "b")]
    for out in outs:
        assert IM.main(["--zarr", store, "--out", out, "--host", "--silence", "--em_rounds", "2"]) == 0
    assert sorted(os.listdir(tmp_path)) == sorted(n + f for n in ("a", "b") for f in FILES)
    assert _tree(outs[0] + FILES[0]) == _tree(outs[1] + FILES[0])
    for f in FILES[1:]:
        assert open(outs[0] + f, "rb").read() == open(outs[1] + f, "rb").read()
    s = json.load(open(outs[0] + "_impute_summary.json"))
    assert tuple(s) == IM.SUMMARY + ("path",)
    miss = int((hap < 0).sum())
    assert (s["mode"], s["N"], s["K"], s["H"], s["n_donor_haps"], s["groups"], s["path"]) == ("fill", 40, 300, 80, 80, 1, "host")
    assert (s["missing_alleles"], s["imputed_alleles"], s["without_dose"], s["typed"], s["untyped"]) == (miss, miss, 0, 300, 0)
    assert s["recipients"] == int((hap < 0).any(axis=0).sum()) and s["ll"] < 0
    head, *hist = [line.split("\t") for line in open(outs[0] + "_impute_history.txt").read().splitlines()]
    assert head == ["round", "switch", "ll"] and [r[0] for r in hist] == ["0", "1"] and s["switch"] in [float(r[1]) for r in hist]
    gt, ds, q = _read_store(outs[0] + FILES[0])
    assert ds.dtype == np.float32 and ds.shape == (300, 40) and np.array_equal(gt.reshape(300, 80), hap)
    both = (gt >= 0).all(axis=2)
    assert np.array_equal(ds[both], gt.sum(axis=2)[both].astype(np.float32))       # exact where both alleles are observed
    assert not np.isnan(ds).any() and ds.min() >= 0 and ds.max() <= 2 and len(q["alleles"]) == 300 and q["alleles"][0] == ["A", "C"]
    assert IM.main(["--zarr", store, "--out", outs[0], "--host", "--silence", "--em_rounds", "0", "--fill_calls"]) == 0
    filled = _read_store(outs[0] + FILES[0])[0].reshape(300, 80)
    assert (filled >= 0).all() and np.array_equal(filled[hap >= 0], hap[hap >= 0])


def test_a_check_run_writes_the_summary_only_and_the_estimated_rate_keeps_the_margin(planted, tmp_path):
    """planted 40 x 300, seed 2 (3 % missing), 10 % of the observed alleles hidden with --seed 7, two rounds from --switch 0.01:
    the estimated rate 0.0315 is used and the mean squared error at the 2,285 hidden alleles is 0.0438 (concordance 0.946, r2 0.825)
    against 0.2252 (0.622, 0.100) of the donors' frequency: the margin of a half holds with the estimated rate."""
    out = str(tmp_path / "c")
    assert IM.main(["--zarr", planted[0], "--out", out, "--host", "--silence", "--em_rounds", "2", "--check_mask", "0.1", "--seed", "7"]) == 0
    assert sorted(os.listdir(tmp_path)) == ["c" + f for f in sorted(FILES[1:])]
    s = json.load(open(out + "_impute_summary.json"))
    assert tuple(s) == IM.SUMMARY + IM.CHECKED + ("path",)
    print(f"check run, estimated switch rate {s['switch']:.4f}: mse {s['mse']:.4f} (frequency {s['mse_frequency']:.4f}), concordance "
          f"{s['concordance']:.3f} ({s['concordance_frequency']:.3f}), r2 {s['r2']:.3f} ({s['r2_frequency']:.3f}), {s['masked']} hidden")
    assert 0.08 * 300 * 80 < s["masked"] < 0.12 * 300 * 80 and s["scored"] == s["masked"]
    assert s["mse"] <= 0.5 * s["mse_frequency"] and s["concordance"] > s["concordance_frequency"] and s["r2"] > s["r2_frequency"]


def test_the_host_command_on_a_cut_of_the_golden_vcf(cut, tmp_path):
    out = str(tmp_path / "g")
    assert IM.main(["--vcf", cut, "--out", out, "--host", "--silence", "--em_rounds", "1"]) == 0
    assert sorted(os.listdir(tmp_path)) == sorted("g" + f for f in FILES)
    s = json.load(open(out + "_impute_summary.json"))
    vcf = G.read_vcf(cut)
    calls = vcf["calldata/GT"]
    keep = ~(calls > 1).any(axis=(1, 2))
    assert (s["N"], s["K"], s["multiallelic_dropped"], s["missing_alleles"]) == (60, int(keep.sum()), int((~keep).sum()), int((calls[keep] < 0).sum()))
    gt, ds, q = _read_store(out + FILES[0])
    assert np.array_equal(gt, calls[keep]) and q["samples"].tolist() == list(vcf["samples"])
    both = (gt >= 0).all(axis=2)
    assert np.array_equal(ds[both], gt.sum(axis=2)[both].astype(np.float32))
    assert int(np.isnan(ds).sum()) <= s["without_dose"] and s["imputed_alleles"] + s["without_dose"] == s["missing_alleles"]


def test_the_host_command_imputes_a_thinned_cut_from_a_panel_cut(tmp_path):
    """Golden VCF: 40 samples the panel, the next 20 typed at every 4th of 300 sites.  DS at the 225 untyped sites against the
    targets' true allele counts: mean squared error 0.0163 against 0.1358 of twice the panel's allele frequency, which the model
    must beat (the margin of a half is asserted on planted data, where the issue measured it)."""
    panel, target = IU.golden_panel(str(tmp_path))
    out = str(tmp_path / "o")
    assert IM.main(["--vcf", target, "--panel", panel, "--out", out, "--host", "--silence", "--em_rounds", "2"]) == 0
    s = json.load(open(out + "_impute_summary.json"))
    assert (s["mode"], s["N"], s["K"], s["H"], s["n_donor_haps"], s["recipients"]) == ("panel", 20, 300, 120, 80, 40)
    assert (s["typed"], s["untyped"], s["swapped"], s["target_unmatched"], s["without_dose"]) == (75, 225, 0, 0, 0)
    gt, ds, q = _read_store(out + FILES[0])
    truth = G.read_vcf(str(tmp_path / "whole.vcf"))["calldata/GT"]
    typed = np.arange(300) % 4 == 0
    assert np.array_equal(gt[typed], truth[typed]) and (gt[~typed] < 0).all()
    assert np.array_equal(ds[typed], truth[typed].sum(axis=2).astype(np.float32)) and not np.isnan(ds).any()
    pan = G.read_vcf(panel)["calldata/GT"].reshape(300, 80)
    twice = 2 * IM.donor_frequency(pan, np.arange(80))[:, None]
    model, freq = (float(((v - truth.sum(axis=2))[~typed] ** 2).mean()) for v in (ds, twice))
    print(f"golden panel 40, 20 targets at every 4th of 300 sites: DS mse {model:.4f} against {freq:.4f} of twice the panel's frequency")
    assert model < freq


def test_panel_matching(tmp_path):
    K, rng = 40, np.random.default_rng(3)
    hap, _ = U.planted(16, K, 5, missing=0.0)
    pos = np.cumsum(rng.integers(10, 500, K))
    ref, alt = np.full(K, "A", dtype=object), np.full(K, "G", dtype=object)
    panel = str(tmp_path / "panel.zarr")
    G.write_callset_zarr(panel, hap[:, :24].reshape(K, 12, 2), pos, [f"p{i}" for i in range(12)], chrom=np.full(K, "1"), ref=ref, alt=alt)
    typed = np.arange(0, K, 3)                                                     # the target's sites, 14 of the panel's
    t_hap = hap[typed][:, 24:].copy()
    t_ref, t_alt, t_pos = ref[typed].copy(), alt[typed].copy(), pos[typed].copy()
    t_ref[2], t_alt[2] = "G", "A"                                                  # exchanged: the target's alleles are flipped
    t_hap[2] = 1 - t_hap[2]
    t_alt[5] = "T"                                                                 # another ALT: no panel site
    t_pos[7] += 1                                                                  # another position: none either
    t_hap[9, 3] = -1
    target = str(tmp_path / "target.zarr")
    G.write_callset_zarr(target, t_hap.reshape(len(typed), 4, 2), t_pos, [f"t{i}" for i in range(4)], chrom=np.full(len(typed), "1"),
                         ref=t_ref, alt=t_alt)
    out = str(tmp_path / "o")
    assert IM.main(["--zarr", target, "--panel", panel, "--out", out, "--host", "--silence", "--em_rounds", "1", "--uniform"]) == 0
    s = json.load(open(out + "_impute_summary.json"))
    assert (s["mode"], s["N"], s["K"], s["H"], s["n_donor_haps"], s["recipients"]) == ("panel", 4, K, 32, 24, 8)
    assert (s["typed"], s["untyped"], s["swapped"], s["target_unmatched"]) == (12, K - 12, 1, 2)
    gt, ds, q = _read_store(out + FILES[0])
    got = gt.reshape(K, 8)
    seen = np.full((K, 8), -1, dtype=np.int8)
    ok = np.setdiff1d(np.arange(len(typed)), [5, 7])
    seen[typed[ok]] = hap[typed[ok]][:, 24:]                                       # in the panel's orientation, the exchanged site too
    seen[typed[9], 3] = -1
    assert np.array_equal(got, seen) and q["pos"].tolist() == pos.tolist() and q["samples"].tolist() == [f"t{i}" for i in range(4)]
    assert s["missing_alleles"] == int((seen < 0).sum()) == s["imputed_alleles"] and not np.isnan(ds).any()
    truth = hap[:, 24:].reshape(K, 4, 2).sum(axis=2)                               # DS against the targets' true allele counts
    untyped = (seen < 0).all(axis=1)
    twice = 2 * IM.donor_frequency(hap[:, :24], np.arange(24))[:, None]
    assert ((ds - truth)[untyped] ** 2).mean() < ((twice - truth)[untyped] ** 2).mean()
    G.write_callset_zarr(str(tmp_path / "shared.zarr"), t_hap.reshape(len(typed), 4, 2), t_pos, ["t0", "p3", "t2", "t3"],
                         chrom=np.full(len(typed), "1"), ref=t_ref, alt=t_alt)
    with pytest.raises(SystemExit, match=r"1 sample\(s\) of the input are in the panel too \(first: p3\)"):
        IM.main(["--zarr", str(tmp_path / "shared.zarr"), "--panel", panel, "--out", out, "--host"])


def test_refusals(cut, tmp_path, capsys, monkeypatch):
    out = str(tmp_path / "o")
    matrix = str(tmp_path / "m.txt")
    with open(matrix, "w") as fh:
        fh.write("sampleID\ts0\ts1\nzz_1\t0\t1\nzz_2\t2\t1\n")
    with pytest.raises(SystemExit, match="--matrix carries no phase"):
        IM.main(["--matrix", matrix, "--out", out, "--host"])
    slashed = U.write_vcf_cut(str(tmp_path / "slashed.vcf"), 40, 60, 50, unphase=((3, 7), (20, 0)))
    with pytest.raises(SystemExit, match=r"slashed.vcf has 2 heterozygous call\(s\) without phase"):
        IM.main(["--vcf", slashed, "--out", out, "--host"])
    haploid = str(tmp_path / "haploid.zarr")
    G.write_callset_zarr(haploid, np.zeros((5, 4, 1), dtype=np.int8), np.arange(1, 6), list("abcd"), chrom=np.full(5, "1"),
                         ref=np.full(5, "A"), alt=np.full(5, "C"))
    with pytest.raises(SystemExit, match="calls of ploidy 1"):
        IM.main(["--zarr", haploid, "--out", out, "--host"])
    with pytest.raises(SystemExit, match=r"120 donor haplotypes and a recipient do not fit 64 columns.*--max_donors M"):
        IM.main(["--vcf", cut, "--out", out, "--host", "--max_haps", "64"])
    for extra, text in ((["--check_mask", "1.5"], "--check_mask must be"), (["--check_mask", "0"], "--check_mask must be"),
                        (["--budget_gb", "0"], "--budget_gb"), (["--zarr", "x"], "exactly one of"), (["--max_haps", "5000"], "--max_haps must be")):
        with pytest.raises(SystemExit) as e:
            IM.main(["--vcf", cut, "--out", out, "--host"] + extra)
        assert e.value.code == 2 and text in capsys.readouterr().err, extra
    for extra, text in ((["--theta", "0.7"], "--theta must be"), (["--switch", "0"], "--switch must be"), (["--em_rounds=-1"], "--em_rounds must be")):
        with pytest.raises(SystemExit, match=text):
            IM.main(["--vcf", cut, "--out", out, "--host"] + extra)
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match="no GPU visible.*loc_impute_dose.*--host"):
        IM.main(["--vcf", cut, "--out", out])
    assert sorted(os.listdir(tmp_path)) == ["haploid.zarr", "m.txt", "slashed.vcf"]
