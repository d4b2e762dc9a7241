"""The admix command on the device (locator_amd/csrc/admix_kernels.hip).

loc_admix_step against admix.step_host(float64) within admix_util.step_tolerance = (max(N, K) + 32) 2^-23, relative on Q', F'
and (with an absolute 2^-23) on 1 - F', and within (LOC_ADMIX_LL_RUN + 8) 2^-23 relative on ll: sample counts around the tile,
site counts around the block, C = 2, 3, 8, 16, P = 1 and 2, planted and edge inputs, every k_groups from 1 to one past the number
of site blocks and 0, pad garbage, NaN-filled scratch and outputs.  Missing calls are exact zeros, all-missing rows stay, two
launches give the same bits, bad arguments launch nothing.

Twenty plain steps against the host float64 fit element by element; the accelerated fit and the command against --host by their
likelihood and their distance from the planted Q (admix.py says why not element by element).

Measured on one MI355X: see DESIGN.md section 8 (the admix command)."""
import json
import os

import numpy as np
import pytest

from locator_amd import admix as A
from tests import admix_util as U

pytestmark = pytest.mark.gpu
T, BL = A.TILE, A.BLOCK
QNAN = 0x7fc00000


def inputs(kind, N, K, C, seed, P):
    """(c, Q float32, F float32) of a step: the planted counts with the start of a fit, or the edge case."""
    if kind == "edge":
        return U.edge_case(N, K, C, seed, P=P)
    c, _, _ = U.planted_case(N, K, C, seed, P=P)
    Q, F = A.project(*A.start(N, K, C, seed))
    return c, Q, F


# ------------------------------------------------------------------ loc_admix_step
@pytest.mark.parametrize("K", [1, BL - 1, BL, BL + 1, 1000])
@pytest.mark.parametrize("N", [1, T - 1, T, T + 1])
def test_step_rows_and_sites_at_every_split(N, K):
    nblocks = (K + BL - 1) // BL
    worst = {}
    fills = np.random.default_rng(N + K)
    for C in (2, 3, 8, 16):
        for P in (1, 2):
            for kind in ("planted", "edge"):
                c, Q, F = inputs(kind, N, K, C, 1000 * N + K + C + P, P)
                want = A.step_host(c, P, Q, F)
                stay_q, stay_f = A.project(Q, F)
                for k_groups in list(range(1, nblocks + 2)) + [0]:
                    got = A.step_device(c, P, Q, F, k_groups=k_groups, fill=QNAN, pad_fill=fills if k_groups % 2 else 0x77,
                                        pitch=(K + 15) // 16 * 16 + 16 * (k_groups % 3))
                    assert got[0].dtype == got[1].dtype == np.float32 and got[0].shape == (N, C) and got[1].shape == (K, C)
                    ratio, parts = U.step_errors(got, want, N, K)
                    assert ratio <= 1.0, (C, P, kind, k_groups, parts)
                    for name, v in parts.items():
                        worst[name] = max(worst.get(name, 0.0), v)
                    assert abs(got[0].astype(np.float64).sum(axis=1) - 1).max() < 1e-6
                    assert got[1].min() >= U.EPS32 and got[1].max() <= np.float32(1) - U.EPS32
                    if kind == "edge" and N >= 3:                        # the sample without a call: its row, projected
                        assert np.array_equal(got[0][N // 2], stay_q[N // 2])
                    if kind == "edge" and K >= 3:                        # the site without a call: its row
                        assert np.array_equal(got[1][K // 2], stay_f[K // 2]) and np.array_equal(stay_f[K // 2], F[K // 2])
    print(f"loc_admix_step N={N} K={K}: largest error / bound " + ", ".join(f"{k} {v:.4g}" for k, v in worst.items()))


def test_step_exact_zeros_and_the_same_bits():
    N, K, C = T + 9, 3 * BL + 5, 3
    c, Q, F = inputs("planted", N, K, C, 5, 2)
    first = A.step_device(c, 2, Q, F, k_groups=2)
    assert all(np.isfinite(v).all() for v in first)
    U_ratio, _ = U.step_errors(first, A.step_host(c, 2, Q, F), N, K)
    assert U_ratio <= 1.0
    for pattern in (None, QNAN, 0xffffffff, 0x7f800001):                          # stale scratch and outputs of every kind
        again = A.step_device(c, 2, Q, F, k_groups=2, fill=pattern, pad_fill=np.random.default_rng(7))
        assert np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1]) and again[2] == first[2]
    # a missing call contributes exactly 0: samples without a call leave F' and ll as they were, bit for bit ...
    more = np.concatenate([c, np.full((5, K), -1, dtype=np.int8)])
    Qm = np.concatenate([Q, Q[:5]])
    got = A.step_device(more, 2, Qm, F, k_groups=2)
    assert np.array_equal(got[1], first[1]) and got[2] == first[2]
    assert np.array_equal(got[0][:N], first[0]) and np.array_equal(got[0][N:], A.project(Q[:5], F)[0])
    # ... and sites without a call leave Q' and ll as they were (one group: the same order of the sites' sums)
    one = A.step_device(c, 2, Q, F, k_groups=1)
    wide = np.concatenate([c, np.full((N, BL + 6), -1, dtype=np.int8)], axis=1)
    Fw = np.concatenate([F, F[:BL + 6]])
    got = A.step_device(wide, 2, Q, Fw, k_groups=1)
    assert np.array_equal(got[0], one[0]) and got[2] == one[2] and np.array_equal(got[1][:K], one[1])
    assert np.array_equal(got[1][K:], F[:BL + 6])
    # one lost site shows: the tolerance is far below a site's share of Q'
    lost = A.step_host(c[:, 1:], 2, Q, F[1:])
    assert np.abs(lost[0] - A.step_host(c, 2, Q, F)[0]).max() > 10 * U.step_tolerance(N, K)
    # no site: Q is copied, ll = 0; no sample: F is copied
    none = A.step_device(np.zeros((N, 0), dtype=np.int8), 2, Q, np.zeros((0, C), dtype=np.float32), fill=QNAN)
    assert np.array_equal(none[0], Q) and none[1].shape == (0, C) and none[2] == 0.0
    none = A.step_device(np.zeros((0, K), dtype=np.int8), 2, np.zeros((0, C), dtype=np.float32), F, fill=QNAN)
    assert np.array_equal(none[1], F) and none[0].shape == (0, C) and none[2] == 0.0


def test_step_bad_arguments_launch_nothing():
    import torch
    from locator_amd import _lib
    lib = _lib.load()
    N, K, C = 70, 100, 3
    d_c = torch.zeros((N, 128), dtype=torch.int8, device="cuda")
    d_q = torch.full((N + 2, C), 1.0 / C, dtype=torch.float32, device="cuda")
    d_f = torch.full((K + 2, C), 0.5, dtype=torch.float32, device="cuda")
    d_qo = torch.full((N + 2, C), 77.0, dtype=torch.float32, device="cuda")
    d_fo = torch.full((K + 2, C), 77.0, dtype=torch.float32, device="cuda")
    d_ll = torch.full((2,), 77.0, dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    need = lib.loc_admix_work_bytes(N, K, C, 2)                                  # two site blocks, two sample tiles
    up16 = lambda v: (v + 15) // 16 * 16                                         # noqa: E731
    assert need == up16(up16(2 * 8) + 2 * N * 4 * 4 + 2 * N * 4) == lib.loc_admix_work_bytes(N, K, C, 5)
    assert lib.loc_admix_work_bytes(N, K, 5, 1) == up16(up16(2 * 8) + N * 8 * 4 + N * 4)
    assert 0 < lib.loc_admix_work_bytes(N, K, C, 0) <= need
    assert lib.loc_admix_work_bytes(N, 0, C, 0) == 0 == lib.loc_admix_work_bytes(0, K, C, 0)
    for args in ((-1, K, C, 0), (N, -1, C, 0), (N, K, 1, 0), (N, K, 17, 0), (N, K, C, -1), (1 << 20, K, C, 0), (N, 1 << 31, C, 0)):
        assert lib.loc_admix_work_bytes(*args) == -1 and lib.loc_last_error()
    work = torch.zeros(need // 4 + 8, dtype=torch.float32, device="cuda")

    def call(c=None, n=N, k=K, pitch=128, P=2, pops=C, q=None, f=None, qo=None, fo=None, ll=None, groups=2, w=None, wb=need):
        ptr = lambda v, d: d.data_ptr() if v is None else v                       # noqa: E731
        return lib.loc_admix_step(ptr(c, d_c), n, k, pitch, P, pops, ptr(q, d_q), ptr(f, d_f), ptr(qo, d_qo), ptr(fo, d_fo),
                                  ptr(ll, d_ll), groups, ptr(w, work), wb, s)

    bad = (dict(pops=1), dict(pops=17), dict(P=3), dict(P=0), dict(pitch=120), dict(pitch=96), dict(c=d_c.data_ptr() + 1),
           dict(q=d_q.data_ptr() + 4), dict(f=d_f.data_ptr() + 8), dict(qo=d_qo.data_ptr() + 4), dict(fo=d_fo.data_ptr() + 4),
           dict(ll=d_ll.data_ptr() + 4), dict(qo=d_q.data_ptr()), dict(fo=d_f.data_ptr()), dict(qo=d_f.data_ptr()),
           dict(fo=d_q.data_ptr()), dict(qo=d_q.data_ptr() + 16), dict(fo=d_qo.data_ptr()), dict(wb=need - 16),
           dict(w=work.data_ptr() + 4), dict(w=0), dict(n=-1), dict(k=-1), dict(n=1 << 20), dict(groups=-1), dict(q=0), dict(ll=0))
    for kw in bad:
        assert call(**kw) == -1, kw
        assert lib.loc_last_error(), kw
    torch.cuda.synchronize()
    assert (d_qo == 77).all() and (d_fo == 77).all() and (d_ll == 77).all() and not work.any()
    assert call() == 0
    torch.cuda.synchronize()
    assert (d_qo[:N] != 77).all() and (d_fo[:K] != 77).all() and (d_qo[N:] == 77).all() and (d_fo[K:] == 77).all()
    assert d_ll[0] != 77 and d_ll[1] == 77


# ------------------------------------------------------------------ the fit
@pytest.fixture(scope="module")
def planted():
    c, Q, F = U.planted_case(300, 2000, 3, 1)
    return c, Q


def test_twenty_plain_steps_follow_the_host(planted):
    c, _ = planted
    N, K = c.shape
    kw = dict(accel="none", tol=0.0, max_rounds=20)
    h64, h32 = A.fit_host(c, 2, 3, **kw), A.fit_host(c, 2, 3, dtype=np.float32, **kw)
    dev = A.fit_device(c, 2, 3, **kw)
    assert dev["rounds"] == h64["rounds"] == 20 and dev["steps"] == 21 and not dev["converged"]
    assert np.array_equal(dev["order"], h64["order"]) and dev["Q"].dtype == np.float32
    yard = max(float(np.abs(h32[k].astype(np.float64) - h64[k]).max()) for k in ("Q", "F"))
    tol = max(8.0 * yard, U.step_tolerance(N, K))
    err = max(float(np.abs(dev[k].astype(np.float64) - h64[k]).max()) for k in ("Q", "F"))
    print(f"twenty plain steps at {N} x {K} x 3: host float32 - float64 {yard:.3g}, device - float64 {err:.3g}, tolerance {tol:.3g}")
    assert err <= tol
    lls = np.array([ll for _, ll, _ in dev["history"]])
    want = np.array([ll for _, ll, _ in h64["history"]])
    assert len(lls) == 21 and (np.abs(lls - want) <= U.LL_BOUND * np.abs(want)).all()
    assert (np.diff(lls) >= -U.LL_BOUND * np.abs(want[1:])).all()


def test_the_accelerated_fit_against_the_host(planted, tmp_path):
    c, truth = planted
    names = [f"s{i}" for i in range(len(c))]
    kw = dict(pops=3, tol=0.0, max_rounds=20, silence=True)
    dev = A.admix(c, 2, names, None, str(tmp_path / "d"), **kw)
    host = A.admix(c, 2, names, None, str(tmp_path / "h"), host=True, **kw)
    h32 = A.fit_host(c, 2, 3, tol=0.0, max_rounds=20, dtype=np.float32)
    assert dev["rounds"] == host["rounds"] == 20 and dev["steps"] == host["steps"] == 61 and dev["path"] == "device"
    assert sorted(os.listdir(tmp_path)) == sorted(f"{o}_admix_{n}" for o in "dh" for n in ("Q.txt", "history.txt", "summary.json"))
    lls = np.array([ll for _, ll, _ in dev["_history"]])
    assert len(lls) == 21 and (np.diff(lls) >= -U.LL_BOUND * np.abs(lls[1:])).all()
    yard = abs(h32["ll"] - host["ll"])
    tol = max(8.0 * yard, U.LL_BOUND * abs(host["ll"]))
    assert abs(dev["ll"] - host["ll"]) <= tol, (dev["ll"], host["ll"], tol)
    r_dev, r_host = U.best_permutation_rmse(dev["_Q"], truth), U.best_permutation_rmse(host["_Q"], truth)
    print(f"accelerated fit, 20 rounds at 300 x 2000 x 3: ll device {dev['ll']!r} host {host['ll']!r} (host float32 {h32['ll']!r}); "
          f"RMSE from the planted Q device {r_dev:.4f} host {r_host:.4f} (host float32 {U.best_permutation_rmse(h32['Q'], truth):.4f})")
    assert r_dev <= 1.25 * r_host
    # the device path repeats itself bit for bit
    again = A.admix(c, 2, names, None, str(tmp_path / "d2"), **kw)
    for n in ("Q.txt", "history.txt", "summary.json"):
        assert open(str(tmp_path / f"d2_admix_{n}"), "rb").read() == open(str(tmp_path / f"d_admix_{n}"), "rb").read(), n
    assert again["ll"] == dev["ll"]


def test_the_command_on_the_golden_vcf(tmp_path):
    base = ["--vcf", U.VCF, "--sample_data", U.SAMPLE_DATA, "--silence", "--max_SNPs", "1000", "--seed", "1", "--max_rounds", "10",
            "--keep_frequencies"]
    assert A.main(base + ["--out", str(tmp_path / "d")]) == 0
    assert A.main(base + ["--out", str(tmp_path / "h"), "--host"]) == 0
    names = ("Q.txt", "history.txt", "summary.json", "locs.txt", "frequencies.npz")
    assert sorted(os.listdir(tmp_path)) == sorted(f"{o}_admix_{n}" for o in "dh" for n in names)
    d, h = (json.load(open(str(tmp_path / f"{o}_admix_summary.json"))) for o in "dh")
    assert tuple(d) == tuple(h) == A.HEAD + A.OWN + ("path",) and (d["path"], h["path"]) == ("device", "host")
    assert (d["N"], d["K"], d["C"], d["rounds"], d["steps"]) == (h["N"], h["K"], h["C"], h["rounds"], h["steps"]) == (500, 1000, 3, 10, 31)
    assert abs(d["ll"] - h["ll"]) <= U.LL_BOUND * abs(h["ll"]), (d["ll"], h["ll"])
    print(f"golden VCF, 1,000 sites, 10 rounds: ll device {d['ll']!r} host {h['ll']!r}; leave-one-out median error device "
          f"{d['median_error']:.4f} host {h['median_error']:.4f}")
    assert abs(d["median_error"] - h["median_error"]) <= 0.25 * h["median_error"]
    zd, zh = np.load(str(tmp_path / "d_admix_frequencies.npz")), np.load(str(tmp_path / "h_admix_frequencies.npz"))
    assert np.array_equal(zd["idx"], zh["idx"]) and zd["F"].shape == zh["F"].shape == (1000, 3) and zd["F"].dtype == np.float32
