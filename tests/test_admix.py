"""The admix command without a GPU (locator_amd/admix.py): the binding of include/locator_hip_admix.h, step_host by hand and
by its properties, float32 against float64 within admix_util.step_tolerance, the driver (monotone likelihood, the extrapolation,
the stop rule, the labels), the leave-one-out placement against refitting, the --host command on the golden VCF, the refusals."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

from locator_amd import admix as A
from locator_amd import baselines as BL
from tests import admix_util as U


# ------------------------------------------------------------------ the binding
def test_admix_header_is_bound_as_the_other_headers_are():
    from locator_amd import _abi
    from tests.abi_util import check_extension
    vp, i64, i = C.c_void_p, C.c_int64, C.c_int
    check_extension("admix", {"loc_admix_work_bytes": (i64, [i, i64, i, i]),
                              "loc_admix_step": (i, [vp, i, i64, i64, i, i, vp, vp, vp, vp, vp, i, vp, i64, vp])},
                    {"LOC_ADMIX_MAX_POPS", "LOC_ADMIX_LL_RUN", "LOC_ADMIX_TILE", "LOC_ADMIX_BLOCK", "LOC_ADMIX_SPLIT"})
    assert (_abi.LOC_ADMIX_MAX_POPS, _abi.LOC_ADMIX_LL_RUN, _abi.LOC_ADMIX_TILE, _abi.LOC_ADMIX_BLOCK) == (
        A.MAX_POPS, A.LL_RUN, A.TILE, A.BLOCK) == (16, 1024, 64, 64)


# ------------------------------------------------------------------ step_host
def _step_scalar(c, P, Q, F):
    """The step of the module text one number at a time (plain Python floats)."""
    N, K, Cn = len(c), len(c[0]), len(Q[0])
    a, b = [[0.0] * K for _ in range(N)], [[0.0] * K for _ in range(N)]
    ll = 0.0
    for i in range(N):
        for k in range(K):
            if c[i][k] < 0:
                continue
            h = sum(Q[i][x] * F[k][x] for x in range(Cn))
            hb = sum(Q[i][x] * (1 - F[k][x]) for x in range(Cn))
            a[i][k], b[i][k] = c[i][k] / h, (P - c[i][k]) / hb
            ll += c[i][k] * math.log(h) + (P - c[i][k]) * math.log(hb)
    Fn = [[0.0] * Cn for _ in range(K)]
    for k in range(K):
        for x in range(Cn):
            up = F[k][x] * sum(Q[i][x] * a[i][k] for i in range(N))
            down = (1 - F[k][x]) * sum(Q[i][x] * b[i][k] for i in range(N))
            Fn[k][x] = min(max(up / (up + down) if up + down > 0 else F[k][x], A.EPS), 1 - A.EPS)
    Qn = [[0.0] * Cn for _ in range(N)]
    for i in range(N):
        n = sum(1 for k in range(K) if c[i][k] >= 0)
        row = [Q[i][x] * sum(F[k][x] * a[i][k] + (1 - F[k][x]) * b[i][k] for k in range(K)) / (P * n) if n else Q[i][x]
               for x in range(Cn)]
        row = [max(v, A.EPS) for v in row]
        Qn[i] = [v / sum(row) for v in row]
    return np.array(Qn), np.array(Fn), ll


def test_step_host_by_hand_on_two_samples_two_sites_two_clusters():
    c = [[2, 0], [1, -1]]
    Q = [[0.75, 0.25], [0.5, 0.5]]
    F = [[0.5, 0.25], [0.25, 0.75]]
    Qn, Fn, ll = A.step_host(np.array(c, dtype=np.int8), 2, np.array(Q), np.array(F))
    # h = .4375 .375 / .375 -, hb = .5625 .625 / .625 -; a = 2/.4375 0 / 1/.375 0, b = 0 3.2 / 1.6 0
    assert ll == pytest.approx(2 * math.log(0.4375) + 2 * math.log(0.625) + math.log(0.375) + math.log(0.625), rel=1e-15)
    # site 0: A = (.75 * 2/.4375 + .5 / .375, .25 * 2/.4375 + .5 / .375), B = (.5 * 1.6, .5 * 1.6)
    A0 = (0.75 * 2 / 0.4375 + 0.5 / 0.375, 0.25 * 2 / 0.4375 + 0.5 / 0.375)
    want_f0 = [0.5 * A0[0] / (0.5 * A0[0] + 0.5 * 0.8), 0.25 * A0[1] / (0.25 * A0[1] + 0.75 * 0.8)]
    # site 1 (sample 1 missing): A = 0, B = (.75 * 3.2, .25 * 3.2): F' = 0, clipped to EPS
    assert np.allclose(Fn, [want_f0, [A.EPS, A.EPS]], rtol=1e-14, atol=0)
    # sample 0: S_c = F_0c a00 + Fb_1c b01, n = 2; sample 1: S_c = F_0c a10 + Fb_0c b10, n = 1
    s0 = (0.5 * 2 / 0.4375 + 0.75 * 3.2, 0.25 * 2 / 0.4375 + 0.25 * 3.2)
    s1 = (0.25 / 0.375 * 2 + 0.5 * 1.6, 0.25 / 0.375 + 0.75 * 1.6)
    q0, q1 = [0.75 * s0[0] / 4, 0.25 * s0[1] / 4], [0.5 * s1[0] / 2, 0.5 * s1[1] / 2]
    assert sum(q0) == pytest.approx(1, rel=1e-15) and sum(q1) == pytest.approx(1, rel=1e-15)        # the EM map keeps the simplex
    assert np.allclose(Qn, [q0, q1], rtol=1e-14, atol=0)
    for got, want in zip((Qn, Fn, ll), _step_scalar(c, 2, Q, F)):
        assert np.allclose(got, want, rtol=1e-14, atol=0)


def test_step_host_is_the_scalar_form_and_keeps_its_invariants():
    for P, Cn in ((2, 3), (1, 5)):
        c, Q, F = U.edge_case(9, 11, Cn, 3 + P, P=P)
        Qn, Fn, ll = A.step_host(c, P, Q, F)
        assert Qn.dtype == Fn.dtype == np.float64 and Qn.shape == (9, Cn) and Fn.shape == (11, Cn) and ll < 0
        for got, want in zip((Qn, Fn, ll), _step_scalar(c.tolist(), P, Q.astype(np.float64).tolist(), F.astype(np.float64).tolist())):
            assert np.allclose(got, want, rtol=1e-11, atol=0)
        assert np.abs(Qn.sum(axis=1) - 1).max() < 1e-15 and Qn.min() >= A.EPS / (1 + 16 * A.EPS)
        assert Fn.min() >= A.EPS and Fn.max() <= 1 - A.EPS
        # the sample and the site without a call stay (the row of Q up to its projection)
        stay_q, stay_f = A.project(Q.astype(np.float64), F.astype(np.float64))
        assert np.array_equal(Qn[4], stay_q[4]) and np.array_equal(Fn[5], stay_f[5]) and np.abs(stay_f[5] - F[5]).max() < 1e-12
        # a masked call is no call: the values behind a mask do not matter, and a sample without calls adds nothing
        more = np.concatenate([c, np.full((2, 11), -1, dtype=np.int8)])
        Qm, Fm, llm = A.step_host(more, P, np.concatenate([Q, Q[:2]]), F)
        assert np.array_equal(Fm, Fn) and llm == pytest.approx(ll, rel=1e-14) and np.array_equal(Qm[:9], Qn)   # (NumPy's sum pairs anew)
        low = np.where(c < 0, np.int8(-7), c)
        assert all(np.array_equal(x, y) for x, y in zip(A.step_host(low, P, Q, F), (Qn, Fn, ll)))
    # ll is the likelihood of the input: a step does not lower it
    c, _, _ = U.planted_case(40, 120, 3, 2)
    Q, F = A.project(*A.start(40, 120, 3))
    Q1, F1, ll0 = A.step_host(c, 2, Q, F)
    assert A.step_host(c, 2, Q1, F1)[2] > ll0
    none = A.step_host(np.zeros((4, 0), dtype=np.int8), 2, Q[:4], np.zeros((0, 3)))
    assert np.array_equal(none[0], Q[:4]) and none[1].shape == (0, 3) and none[2] == 0.0


@pytest.mark.parametrize("N,K,Cn,P", [(300, 2000, 3, 2), (129, 65, 16, 1), (65, 1000, 8, 2)])
def test_float32_stays_within_the_step_tolerance_of_float64_at_the_bounds(N, K, Cn, P):
    c, Q, F = U.edge_case(N, K, Cn, N + K, P=P)
    assert (F == U.EPS32).mean() > 0.15 and (F == np.float32(1) - U.EPS32).mean() > 0.15 and (Q < 2e-5).any()
    ratio, parts = U.step_errors(A.step_host(c, P, Q, F, np.float32), A.step_host(c, P, Q, F), N, K)
    print(f"step_host float32 against float64 at {N} x {K} x {Cn}: error / bound " + ", ".join(f"{k} {v:.4g}" for k, v in parts.items()))
    assert ratio <= 1.0, parts


def test_refusals_of_the_definitions():
    c = np.zeros((4, 5), dtype=np.int8)
    for Q, F, text in ((np.ones((4, 1)), np.ones((5, 1)), "C = 1"), (np.ones((4, 17)), np.ones((5, 17)), "C = 17"),
                       (np.ones((3, 2)), np.ones((5, 2)), "need"), (np.ones((4, 2)), np.ones((5, 3)), "need")):
        with pytest.raises(ValueError, match=text):
            A.step_host(c, 2, Q, F)
    with pytest.raises(ValueError, match="a count of 2 exceeds the ploidy 1"):
        A.step_host(np.full((4, 5), 2, dtype=np.int8), 1, np.ones((4, 2)), np.ones((5, 2)))
    for kw, text in (({"accel": "qn"}, "accel"), ({"tol": -1.0}, "tol"), ({"tol": float("nan")}, "tol"), ({"max_rounds": 0}, "max_rounds")):
        with pytest.raises(ValueError, match=text):
            A.fit_host(c, 2, 2, **kw)


# ------------------------------------------------------------------ fit_host
@pytest.fixture(scope="module")
def small():
    c, Q, _ = U.planted_case(60, 300, 3, 4)
    return c, Q


def test_the_likelihood_never_decreases_and_the_stop_rule_ends_where_it_says(small):
    c, truth = small
    state = np.random.get_state()[1].copy()
    tol = 1e-5
    res = A.fit_host(c, 2, 3, tol=tol)
    assert np.array_equal(np.random.get_state()[1], state)                        # --seed's stream is not touched
    rounds, lls, acc = zip(*res["history"])
    assert rounds == tuple(range(res["rounds"] + 1)) and acc[-1] is None and set(acc[:-1]) <= {0, 1} and res["converged"]
    assert (np.diff(lls) >= 0).all() and res["ll"] == lls[-1] and res["steps"] == 3 * res["rounds"] + 1
    thr = tol * A.n_alleles(c, 2)
    gains = np.diff(lls)
    assert gains[-1] < thr and (gains[:-1] >= thr).all()
    # the result is the x0 of the round that stopped: the same rounds without a tolerance end on it
    same = A.fit_host(c, 2, 3, tol=0.0, max_rounds=res["rounds"])
    assert not same["converged"] and same["rounds"] == res["rounds"] and same["ll"] == res["ll"]
    assert np.array_equal(same["Q"], res["Q"]) and np.array_equal(same["F"], res["F"]) and same["history"] == res["history"]
    # ... and it is the planted structure: at 60 x 300 less than half the error of giving everybody 1 / C
    assert U.best_permutation_rmse(res["Q"], truth) < 0.5 * U.best_permutation_rmse(np.full((60, 3), 1 / 3), truth)
    # plain EM: one step a round, monotone too, slower
    plain = A.fit_host(c, 2, 3, accel="none", tol=tol, max_rounds=30)
    assert plain["steps"] == plain["rounds"] + 1 and (np.diff([ll for _, ll, _ in plain["history"]]) >= 0).all()
    assert plain["history"][3][1] < res["history"][3][1]
    Q, F = A.start(60, 300, 3)
    for t in range(3):
        assert plain["history"][t][1] == A.step_host(c, 2, Q, F)[2]
        Q, F, _ = A.step_host(c, 2, Q, F)


def test_alpha_minus_one_is_two_plain_steps(small):
    c, _ = small
    ops = A._HostOps(c, 2, np.float64)
    x0 = ops.take(*A.start(60, 300, 3))
    Q1, F1, _ = ops.step(*x0)
    Q2, F2, _ = ops.step(Q1, F1)
    (Qa, Fa), alpha = A.extrapolate(ops, x0, (Q1, F1), (Q2, F2), alpha=-1.0)
    assert alpha == -1.0 and np.abs(Qa - Q2).max() < 1e-14 and np.abs(Fa - F2).max() < 1e-14
    (Qa, Fa), alpha = A.extrapolate(ops, x0, (Q1, F1), (Q2, F2))
    r = np.sqrt(((Q1 - x0[0]) ** 2).sum() + ((F1 - x0[1]) ** 2).sum())
    v = np.sqrt(((Q2 - 2 * Q1 + x0[0]) ** 2).sum() + ((F2 - 2 * F1 + x0[1]) ** 2).sum())
    assert alpha == pytest.approx(-max(1.0, r / v), rel=1e-12) and alpha < -1
    assert np.abs(Qa.sum(axis=1) - 1).max() < 1e-15 and Fa.min() >= A.EPS and Fa.max() <= 1 - A.EPS and Qa.min() > 0
    assert A.extrapolate(ops, x0, x0, x0)[1] == -1.0                              # |v| = 0


def test_the_labels_are_ordered_by_size(small):
    c, _ = small
    res = A.fit_host(c, 2, 3, max_rounds=3)
    sizes = res["Q"].sum(axis=0)
    assert (np.diff(sizes) <= 0).all() and sorted(res["order"]) == [0, 1, 2]
    Q = np.array([[0.2, 0.5, 0.3], [0.2, 0.25, 0.55], [0.1, 0.5, 0.4]])
    Qr, Fr, order = A.relabel(Q, np.arange(6.0).reshape(2, 3))
    assert order.tolist() == [1, 2, 0] and np.array_equal(Qr, Q[:, [1, 2, 0]]) and np.array_equal(Fr, [[1, 2, 0], [4, 5, 3]])
    assert A.relabel(np.full((4, 3), 1 / 3), np.zeros((2, 3)))[2].tolist() == [0, 1, 2]     # ties: the lower index first


# ------------------------------------------------------------------ the placement
def _refit(Q, locs, located):
    li, ui = np.flatnonzero(located), np.flatnonzero(~located)
    X = np.concatenate([np.ones((len(Q), 1)), Q[:, :-1]], axis=1)
    out = np.full((len(Q), 2), np.nan)
    for i in li:
        rest = li[li != i]
        out[i] = X[i] @ np.linalg.lstsq(X[rest], locs[rest], rcond=None)[0]
    out[ui] = X[ui] @ np.linalg.lstsq(X[li], locs[li], rcond=None)[0]
    return out


def test_the_leave_one_out_formula_is_a_refit_without_the_sample():
    rng = np.random.default_rng(8)
    for Cn in (2, 4):
        Q = rng.dirichlet(np.ones(Cn), 40)
        locs = Q[:, :2] @ np.array([[30.0, 5.0], [-10.0, 20.0]]) + rng.normal(0, 1.0, (40, 2))
        locs[[3, 17, 39]] = np.nan
        located = ~np.isnan(locs).any(axis=1)
        got = A.placements(Q, locs, located)
        assert np.isfinite(got).all() and np.abs(got - _refit(Q, locs, located)).max() < 1e-9
    # a sample the fit cannot do without (the only one with a share of cluster 3): no leave-one-out prediction
    Q = np.concatenate([np.stack([np.linspace(0.1, 0.9, 8), 1 - np.linspace(0.1, 0.9, 8), np.zeros(8)], axis=1), [[0.2, 0.3, 0.5]]])
    Q = Q[:, [0, 2, 1]]                                                           # the regressors are the first C - 1 columns
    locs = rng.normal(size=(9, 2))
    got = A.placements(Q, locs, np.ones(9, dtype=bool))
    assert np.isnan(got[8]).all() and np.isfinite(got[:8]).all()
    assert A.placements(Q, locs, np.arange(9) < 3) is None and A.placements(Q, locs, np.arange(9) < 4) is not None


# ------------------------------------------------------------------ the command
GOLDEN_ARGS = ["--max_SNPs", "1000", "--seed", "1", "--max_rounds", "10"]


def run(tmp_path, name, *extra, sample_data=True):
    out = str(tmp_path / name)
    where = ["--sample_data", U.SAMPLE_DATA] if sample_data else []
    assert A.main(["--vcf", U.VCF, "--out", out, "--silence", "--host"] + where + list(extra)) == 0
    return out


def test_the_host_command_on_the_golden_vcf(tmp_path, capsys):
    out = run(tmp_path, "g", *GOLDEN_ARGS)
    s = json.load(open(out + "_admix_summary.json"))
    assert tuple(s) == A.HEAD + A.OWN + ("path",)
    assert (s["N"], s["n_located"], s["K"], s["P"], s["C"], s["rounds"], s["steps"], s["converged"], s["accel"], s["init_seed"],
            s["tol"], s["path"], s["error_unit"]) == (500, 450, 1000, 2, 3, 10, 31, False, "squarem", 1, 1e-7, "host", "map units")
    head, *rows = [line.split("\t") for line in open(out + "_admix_Q.txt").read().splitlines()]
    assert head == ["sampleID", "q1", "q2", "q3"] and len(rows) == 500 and rows[0][0] == "msp_0"
    Q = np.array([[float(v) for v in r[1:]] for r in rows])
    assert np.abs(Q.sum(axis=1) - 1).max() < 1e-12 and Q.min() > 0
    assert s["cluster_sizes"] == [float(v) for v in Q.sum(axis=0)] and (np.diff(s["cluster_sizes"]) <= 0).all()
    head, *hist = [line.split("\t") for line in open(out + "_admix_history.txt").read().splitlines()]
    assert head == ["round", "ll", "accepted"] and [r[0] for r in hist] == [str(t) for t in range(11)] and hist[-1][2] == "NA"
    lls = [float(r[1]) for r in hist]
    assert (np.diff(lls) >= 0).all() and lls[-1] == s["ll"] and {r[2] for r in hist[:-1]} <= {"0", "1"}
    # the files are the definitions': the sites of a fit with the same draw, the fit, the placement
    from locator_amd import genotypes as G
    vcf = G.read_vcf(U.VCF)
    np.random.seed(1)
    _, idx = G.filter_snps(vcf["calldata/GT"], min_mac=2, max_snps=1000, verbose=False, sites=True)
    c, P = BL.count_matrix(vcf["calldata/GT"], idx)
    res = A.fit_host(c, P, 3, max_rounds=10)
    assert np.array_equal(res["Q"], Q) and res["ll"] == s["ll"] and s["ll_per_allele"] == s["ll"] / A.n_alleles(c, P)
    locs = BL.read_locations(U.SAMPLE_DATA, vcf["samples"], A.PROG)
    located = ~np.isnan(locs).any(axis=1)
    head, *rows = [line.split(",") for line in open(out + "_admix_locs.txt").read().splitlines()]
    assert head == ["x", "y", "sampleID"] and len(rows) == 500 and rows[0][2] == "msp_0"
    placed = np.array([[float(r[0]), float(r[1])] for r in rows])
    assert np.isfinite(placed).all() and np.array_equal(placed, A.placements(Q, locs, located))
    err = BL.errors(placed[located], locs[located])
    assert s["median_error"] == float(np.median(err)) and s["mean_error"] == float(np.mean(err))
    # the baseline it is: better than placing everybody at the centroid of the located samples
    centroid = float(np.median(BL.errors(np.broadcast_to(locs[located].mean(axis=0), (450, 2)), locs[located])))
    print(f"golden VCF, 1,000 sites, C = 3, 10 rounds: leave-one-out median error {s['median_error']:.3f}, centroid {centroid:.3f}")
    assert s["median_error"] < centroid
    # a second run writes the same bytes; exactly the listed files
    again = run(tmp_path, "again", *GOLDEN_ARGS)
    names = ("_admix_Q.txt", "_admix_history.txt", "_admix_summary.json", "_admix_locs.txt")
    for name in names:
        assert open(again + name, "rb").read() == open(out + name, "rb").read(), name
    assert sorted(os.listdir(tmp_path)) == sorted(f"{o}{n}" for o in ("g", "again") for n in names)


def test_without_locations_with_frequencies_and_ld_prune(tmp_path, capsys):
    out = run(tmp_path, "q", "--max_SNPs", "200", "--seed", "1", "--max_rounds", "2", "--pops", "4", "--accel", "none",
              "--keep_frequencies", "--init_seed", "5", sample_data=False)
    assert sorted(os.listdir(tmp_path)) == [f"q_admix_{n}" for n in ("Q.txt", "frequencies.npz", "history.txt", "summary.json")]
    s = json.load(open(out + "_admix_summary.json"))
    assert tuple(s) == ("N", "K", "P") + A.OWN + ("path",) and (s["C"], s["accel"], s["steps"], s["init_seed"]) == (4, "none", 3, 5)
    z = np.load(out + "_admix_frequencies.npz")
    assert sorted(z.files) == ["F", "idx", "samples"] and z["F"].shape == (200, 4) and z["F"].dtype == np.float64
    assert len(z["idx"]) == 200 and z["samples"][0] == "msp_0" and z["F"].min() >= A.EPS and z["F"].max() <= 1 - A.EPS
    pruned = run(tmp_path, "ld", "--ld_prune", "0.2", "--max_rounds", "1", "--longlat")
    s = json.load(open(pruned + "_admix_summary.json"))
    assert tuple(s) == A.HEAD + A.OWN + ("ld_prune", "ld_window", "ld_window_bp", "K_before_prune", "path")
    assert (s["K"], s["K_before_prune"], s["ld_prune"], s["error_unit"]) == (1996, 5830, 0.2, "km")
    # too few located samples: no placement, and a line that says so
    c, _, _ = U.planted_case(12, 40, 3, 1)
    locs = np.full((12, 2), np.nan)
    locs[:3] = [[0, 0], [1, 2], [2, 1]]
    capsys.readouterr()
    s = A.admix(c, 2, [f"s{i}" for i in range(12)], locs, str(tmp_path / "few"), max_rounds=1, host=True)
    assert "fewer than C + 1, no placement is made" in capsys.readouterr().out and s["_xy"] is None and "n_located" not in s
    assert not os.path.exists(str(tmp_path / "few_admix_locs.txt")) and os.path.exists(str(tmp_path / "few_admix_Q.txt"))


def test_without_a_gpu_the_command_stops_unless_host(tmp_path, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match="no GPU visible.*loc_admix_step.*--host"):
        A.main(["--vcf", U.VCF, "--out", str(tmp_path / "o")])
    c, _, _ = U.planted_case(12, 40, 3, 1)
    with pytest.raises(SystemExit, match="no GPU visible.*loc_admix_step.*--host"):
        A.admix(c, 2, [f"s{i}" for i in range(12)], None, str(tmp_path / "o"))
    assert not os.listdir(tmp_path)


def test_refusals_leave_nothing_behind(tmp_path, capsys):
    base = ["--vcf", U.VCF, "--out", str(tmp_path / "o"), "--host", "--silence"]
    for extra, text in ((["--pops", "1"], "--pops must be 2 .. 16"), (["--pops", "17"], "--pops must be 2 .. 16"),
                        (["--tol=-1e-3"], "--tol must be"), (["--tol", "nan"], "--tol must be"), (["--tol", "inf"], "--tol must be"),
                        (["--max_rounds", "0"], "--max_rounds must be"), (["--accel", "qn"], "invalid choice"),
                        (["--zarr", "x"], "exactly one of --vcf / --zarr / --matrix"), (["--folds", "3"], "unrecognized arguments"),
                        (["--ld_prune", "0.2", "--ld_window", "0"], "--ld_window must be")):
        with pytest.raises(SystemExit) as e:
            A.main(base + extra)
        assert e.value.code == 2 and text in capsys.readouterr().err, extra
    c, _, _ = U.planted_case(3, 40, 2, 1)
    names = ["a", "b", "c"]
    for kw, text in ((dict(pops=4), "--pops 4 with 3 samples"), (dict(pops=1), "--pops must be"), (dict(pops=17), "--pops must be"),
                     (dict(tol=float("nan")), "--tol must be"), (dict(max_rounds=0), "--max_rounds must be"),
                     (dict(accel="qn"), "--accel must be")):
        with pytest.raises(SystemExit, match=text):
            A.admix(c, 2, names, None, str(tmp_path / "o"), host=True, **kw)
    with pytest.raises(SystemExit, match="no site is left"):
        A.admix(c[:, :0], 2, names, None, str(tmp_path / "o"), host=True)
    with pytest.raises(SystemExit, match="not in"):                               # a sample the table does not know
        A.main(["--matrix", _matrix(tmp_path), "--sample_data", U.SAMPLE_DATA, "--out", str(tmp_path / "m" / "o"), "--host"])
    assert sorted(os.listdir(tmp_path)) == ["in"]


def _matrix(tmp_path):
    os.makedirs(str(tmp_path / "in"))
    path = str(tmp_path / "in" / "m.txt")
    with open(path, "w") as fh:
        fh.write("sampleID\ts0\ts1\ts2\nzz_1\t0\t1\t2\nzz_2\t2\t1\t0\nzz_3\t1\t1\t1\n")
    return path
