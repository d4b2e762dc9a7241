"""The paint command without a GPU: the binding, the NumPy definition (rows on the simplex, exact zeros, the closed form without
linkage, the split at a certain switch, the stretch without a switch in float32), the planted placement, the driver's pieces, the
--host command on a cut of the golden VCF, the refusals."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from locator_amd import baselines as BL
from locator_amd import paint as PT
from tests import paint_util as U


# ------------------------------------------------------------------ the binding
def test_paint_header_is_bound_as_the_other_headers_are():
    from locator_amd import _abi
    from tests.abi_util import check_extension
    vp, i64, i, f = C.c_void_p, C.c_int64, C.c_int, C.c_float
    check_extension("paint", {"loc_paint_work_bytes": (i64, [i, i64, i, i]),
                              "loc_paint_copy": (i, [vp, i, i64, i64, vp, vp, vp, i, vp, f, i, vp, vp, vp, vp, vp, i64, vp])},
                    {"LOC_PAINT_MAX_HAPS", "LOC_PAINT_LANE_COLS", "LOC_PAINT_LL_RUN", "LOC_PAINT_C_SLOTS"})
    assert (_abi.LOC_PAINT_MAX_HAPS, _abi.LOC_PAINT_LANE_COLS) == (PT.MAX_HAPS, 4) == (4096, 4)


# ------------------------------------------------------------------ copy_host
def _donor_mask(case):
    return (case["donor"][None, :] != 0) & (case["owner"][None, :] != case["owner"][case["rec"]][:, None])


@pytest.mark.parametrize("kind", ["planted", "edge"])
def test_rows_are_on_the_simplex_and_exact_zeros_stay(kind):
    H, K = 30, 40
    case = U.planted_case(H, K, 4) if kind == "planted" else U.edge_case(H, K, 4, 0.01)
    share, chunks, ll, nd = U.host(case, np.float64)
    dn = _donor_mask(case)
    assert np.array_equal(nd, dn.sum(axis=1)) and share.shape == chunks.shape == dn.shape
    live = nd > 0
    assert (~live).any() == (kind == "edge")                                     # the edge case holds recipients without a donor
    assert np.abs(share[live].sum(axis=1) - 1).max() < 1e-12
    assert not share[~dn].any() and not chunks[~dn].any() and not ll[~live].any() and (ll[live] < 0).all()
    certain = int((np.concatenate([[1.0], case["rho"][1:]]) == 1).sum())
    rows = chunks[live].sum(axis=1)
    assert (rows >= certain - 1e-9).all() and (rows <= K + 1e-9).all() and (share >= 0).all() and (chunks >= 0).all()


def test_without_linkage_the_share_is_the_closed_form():
    case = U.edge_case(20, 15, 2, 0.05)
    case["rho"] = np.ones(15)
    share, chunks, ll, nd = U.host(case, np.float64)
    dn = _donor_mask(case)
    live = np.flatnonzero(nd > 0)
    want = np.zeros_like(share)
    for j in range(15):
        e = PT.emissions(case["h"], j, case["rec"], dn, 0.05, np.float64)
        with np.errstate(invalid="ignore"):
            want += e / e.sum(axis=1, keepdims=True)
    assert np.abs(share[live] - want[live] / 15).max() < 1e-14
    assert np.abs(chunks[live] - want[live]).max() < 1e-12                       # every site starts a chunk


def test_a_certain_switch_splits_the_problem():
    H, K, cut = 24, 30, 13
    case = U.planted_case(H, K, 9)
    case["rho"] = np.full(K, 0.07)
    case["rho"][cut] = 1.0
    whole = U.host(case, np.float64)
    parts = []
    for a, b in ((0, cut), (cut, K)):
        part = dict(case)
        part["h"], part["rho"] = case["h"][a:b], case["rho"][a:b]
        parts.append((b - a, U.host(part, np.float64)))
    assert np.abs(K * whole[0] - sum(n * p[0] for n, p in parts)).max() < 1e-12
    assert np.abs(whole[1] - sum(p[1] for _, p in parts)).max() < 1e-12
    assert np.abs(whole[2] - sum(p[2] for _, p in parts)).max() < 1e-10


def test_a_long_stretch_without_a_switch_stays_finite_in_float32():
    case = U.no_switch_case(K=200, theta=1e-3)
    for dtype in (np.float32, np.float64):
        share, chunks, ll, nd = U.host(case, dtype)
        assert share.dtype == dtype and all(np.isfinite(v).all() for v in (share, chunks, ll))
        # rho = 0 after the first site: every xi is an exact 0 and chunks is gamma_0 alone, a row that sums to 1
        assert np.abs(chunks.sum(axis=1) - 1).max() < 1e-6
        if dtype == np.float32:
            assert share[0, 2] == 0 and chunks[0, 2] == 0                        # the donor that never matches underflowed
    rho = case["rho"].copy()
    rho[1:] = 1e-3                                                               # ... and with switches the same row does not
    assert U.host({**case, "rho": rho}, np.float32)[1].sum(axis=1).min() > 1 + 1e-3
    assert share[0, 2] < 1e-200 and share[0, 4] > 0.99                           # float64: the copy of the recipient takes all


def test_refusals_of_the_definition():
    case = U.planted_case(8, 5, 1)
    for change, text in (({"theta": 0.6}, "theta"), ({"theta": 1e-8}, "theta"), ({"rec": np.array([8])}, "recipient"),
                         ({"rho": np.full(5, 1.5)}, "switch probability"), ({"rho": np.zeros(4)}, "switch probabilities"),
                         ({"h": case["h"].astype(np.int16)}, "int8"), ({"owner": case["owner"][:3]}, "owners")):
        with pytest.raises(ValueError, match=text):
            U.host({**case, **change}, np.float64)
    with pytest.raises(ValueError, match="columns"):
        PT.copy_host(np.zeros((2, PT.MAX_HAPS + 1), dtype=np.int8), np.ones(PT.MAX_HAPS + 1), np.zeros(PT.MAX_HAPS + 1), [0], [1, 0.1], 0.1)


# ------------------------------------------------------------------ the driver's pieces
def test_the_planted_placement_beats_half_the_centroid():
    hap, x = U.planted(20, 300, 1)
    locs = np.stack([x, np.zeros(20)], axis=1)
    s = PT.paint(hap, np.zeros((20, 300), dtype=np.int8), 2, [f"s{i}" for i in range(20)], locs, host=True, k=3, uniform=True,
                 silence=True)
    centroid = float(np.median(np.abs(x - x.mean())))
    print(f"planted 20 x 300, seed 1: top-3 placement median error {s['median_error']:.4f}, centroid {centroid:.4f}")
    assert s["median_error"] < 0.5 * centroid
    lls = [r[2] for r in s["_history"]]
    assert len(lls) == 3 and max(lls) >= lls[0] and s["switch"] == s["_history"][int(np.argmax(lls))][1]
    W = s["_W"]
    assert not np.diag(W).any() and np.abs(W.sum(axis=1) - 2).max() < 1e-9       # nobody copies from themself


def test_switch_rates_theta_and_groups():
    g, first = PT.site_gaps(np.array(["1", "1", "1", "2", "2"]), np.array([10, 20, 40, 5, 35]), 5)
    assert first.tolist() == [True, False, False, True, False] and np.allclose(g, [1, 0.5, 1.0, 1, 1.5])
    rho = PT.switch_rates(0.1, g, first)
    assert rho.dtype == np.float32 and rho[0] == rho[3] == 1 and np.allclose(rho[[1, 2, 4]], 1 - np.exp(-0.1 * g[[1, 2, 4]]))
    assert PT.site_gaps(None, None, 3)[0].tolist() == [1, 1, 1] and PT.site_gaps(["1"] * 3, [1, 5, 9], 3, uniform=True)[0].tolist() == [1, 1, 1]
    with pytest.raises(ValueError, match="ascending"):
        PT.site_gaps(["1"] * 3, [1, 9, 5], 3)
    w = 1 / (1 + 1 / 2 + 1 / 3)
    assert PT.default_theta(4) == 0.5 * w / (4 + w) and PT.default_theta(1) == 0.5
    groups = PT.launch_groups(7, [1, 4], 8)
    assert [c.tolist() for c, _ in groups] == [[1, 4, 0, 2], [1, 4, 3, 5], [1, 4, 6]]
    assert [r.tolist() for _, r in groups] == [[1, 4, 0, 2], [3, 5], [6]]
    # the groups of a small --max_haps give what one launch gives
    hap, _ = U.planted(7, 40, 2)
    rho = PT.switch_rates(0.05, *PT.site_gaps(None, None, 40))
    one = PT.sample_weights(PT.copy_host, hap, [1, 4], rho, 0.01, 14)
    many = PT.sample_weights(PT.copy_host, hap, [1, 4], rho, 0.01, 8)
    assert one[4] == 1 and many[4] == 3
    assert all(np.abs(a - b).max() < 1e-12 for a, b in zip(one[:3], many[:3])) and np.array_equal(one[3], many[3])
    assert PT.em_update(0.1, np.array([1.0, 0.5, 0.5]), np.full((2, 4), 0.3), np.array([3, 3, 0])) == 0.1 * (2.4 - 2) / 2.0


# ------------------------------------------------------------------ the command
ARGS = ("--max_SNPs", "300", "--seed", "3", "--em_rounds", "2", "--kmax", "8", "--keep_matrix")
FILES = ("_paint_summary.json", "_paint_history.txt", "_paint_donors.txt", "_paint_locs.txt", "_paint.npz")


@pytest.fixture(scope="module")
def cut(tmp_path_factory):
    return U.write_vcf_cut(str(tmp_path_factory.mktemp("paint") / "cut.vcf"), 40, 60, 900)


def test_the_host_command_on_a_cut_of_the_golden_vcf(cut, tmp_path):
    outs = []
    for name in ("a", "b"):
        outs.append(str(tmp_path / name))
        assert PT.main(["--vcf", cut, "--sample_data", U.SAMPLE_DATA, "--out", outs[-1], "--host", "--silence", *ARGS]) == 0
    assert sorted(os.listdir(tmp_path)) == sorted(o + n for o in ("a", "b") for n in FILES)
    for n in FILES:
        assert open(outs[0] + n, "rb").read() == open(outs[1] + n, "rb").read(), n
    s = json.load(open(outs[0] + "_paint_summary.json"))
    assert tuple(s) == PT.HEAD + PT.OWN + PT.PLACED + ("path",)
    assert (s["N"], s["n_located"], s["K"], s["H"], s["n_donor_haps"], s["groups"], s["path"]) == (60, 50, 300, 120, 100, 1, "host")
    head, *hist = [line.split("\t") for line in open(outs[0] + "_paint_history.txt").read().splitlines()]
    assert head == ["round", "switch", "ll"] and [r[0] for r in hist] == ["0", "1"]
    lls, lams = [float(r[2]) for r in hist], [float(r[1]) for r in hist]
    chosen = lams.index(s["switch"])
    assert lls[chosen] >= lls[0] and lls[chosen] == max(lls) and s["ll"] == lls[chosen]      # every individual was a recipient of the rounds
    head, *rows = [line.split(",") for line in open(outs[0] + "_paint_locs.txt").read().splitlines()]
    assert head == ["x", "y", "sampleID"] and len(rows) == 60 and np.isfinite([float(r[0]) for r in rows]).all()
    head, *rows = [line.split("\t") for line in open(outs[0] + "_paint_donors.txt").read().splitlines()]
    assert head == ["sampleID", "rank", "donorID", "share"] and len(rows) == 60 * 8 and all(r[0] != r[2] for r in rows)
    z = np.load(outs[0] + "_paint.npz")
    assert sorted(z.files) == ["counts", "lengths", "samples"] and z["lengths"].shape == z["counts"].shape == (60, 60)
    assert np.abs(z["lengths"].sum(axis=1) - 300).max() < 1e-6 and not np.diag(z["counts"]).any()
    locs = BL.read_locations(U.SAMPLE_DATA, z["samples"], PT.PROG)
    located = ~np.isnan(locs).any(axis=1)
    assert not z["lengths"][:, ~located].any()                                   # only located samples give
    centroid = float(np.median(BL.errors(np.broadcast_to(locs[located].mean(axis=0), (50, 2)), locs[located])))
    print(f"golden VCF cut 60 x 300: leave-one-out median error {s['median_error']:.3f} at k = {s['k']}, centroid {centroid:.3f}")
    assert s["median_error"] < centroid


def test_without_locations_everyone_gives(cut, tmp_path):
    out = str(tmp_path / "n")
    assert PT.main(["--vcf", cut, "--out", out, "--host", "--silence", "--max_SNPs", "100", "--seed", "1", "--em_rounds", "0",
                    "--uniform", "--theta", "0.01"]) == 0
    assert sorted(os.listdir(tmp_path)) == ["n" + n for n in sorted(FILES[:3])]
    s = json.load(open(out + "_paint_summary.json"))
    assert tuple(s) == ("N", "K", "P") + PT.OWN + ("path",) and (s["n_donor_haps"], s["theta"], s["switch"], s["uniform"]) == (120, 0.01, 0.01, True)
    assert open(out + "_paint_history.txt").read() == "round\tswitch\tll\n"


def test_refusals(cut, tmp_path, capsys, monkeypatch):
    out = str(tmp_path / "o")
    matrix = str(tmp_path / "m.txt")
    with open(matrix, "w") as fh:
        fh.write("sampleID\ts0\ts1\nzz_1\t0\t1\nzz_2\t2\t1\n")
    with pytest.raises(SystemExit, match="--matrix carries no phase"):
        PT.main(["--matrix", matrix, "--out", out, "--host"])
    slashed = U.write_vcf_cut(str(tmp_path / "slashed.vcf"), 40, 60, 50, unphase=((3, 7), (20, 0)))
    with pytest.raises(SystemExit, match=r"slashed.vcf has 2 heterozygous call\(s\) without phase"):
        PT.main(["--vcf", slashed, "--out", out, "--host"])
    with pytest.raises(SystemExit, match=r"100 donor haplotypes and a recipient do not fit 64 columns.*--max_donors M"):
        PT.main(["--vcf", cut, "--sample_data", U.SAMPLE_DATA, "--out", out, "--host", "--max_haps", "64", "--max_SNPs", "50"])
    # ... and with --max_donors the run goes through in groups
    assert PT.main(["--vcf", cut, "--sample_data", U.SAMPLE_DATA, "--out", out, "--host", "--max_haps", "64", "--max_SNPs", "50",
                    "--seed", "1", "--max_donors", "20", "--em_rounds", "1", "--silence"]) == 0
    s = json.load(open(out + "_paint_summary.json"))
    assert (s["n_donor_haps"], s["groups"]) == (34, 3)
    for n in FILES[:4]:
        os.remove(out + n)
    for extra, text in ((["--k", "9", "--kmax", "8"], "--k must be"), (["--kmax", "0"], "--kmax must be"), (["--budget_gb", "0"], "--budget_gb"),
                        (["--zarr", "x"], "exactly one of")):
        with pytest.raises(SystemExit) as e:
            PT.main(["--vcf", cut, "--out", out, "--host"] + extra)
        assert e.value.code == 2 and text in capsys.readouterr().err, extra
    for extra, text in ((["--theta", "0.7"], "--theta must be"), (["--switch", "0"], "--switch must be"), (["--em_rounds=-1"], "--em_rounds must be"),
                        (["--max_haps", "5000"], "--max_haps must be"), (["--max_donors", "0"], "--max_donors must be")):
        with pytest.raises(SystemExit, match=text):
            PT.main(["--vcf", cut, "--out", out, "--host", "--max_SNPs", "50"] + extra)
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match="no GPU visible.*loc_paint_copy.*--host"):
        PT.main(["--vcf", cut, "--out", out])
    assert sorted(os.listdir(tmp_path)) == ["m.txt", "slashed.vcf"]
