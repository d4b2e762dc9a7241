"""The paint command on the device (locator_amd/csrc/paint_kernels.hip).

loc_paint_copy against paint.copy_host(float64).  The allowance of a case is 8 times the distance of copy_host(float32) from
copy_host(float64) on that case, floored at 2^-21 (paint_util.allowances): absolute on share, |d| / (1 + |x|) on chunks, relative
on ll.  Shapes around the 64 lanes and the 256 columns of a sweep, site counts around the checkpoint blocks, every block size,
planted and edge inputs, pad garbage, NaN-filled scratch and outputs, rec a subset in non-ascending order.  No result depends on
the block size, on what scratch held, on appended non-donor columns or on appended recipients, bit for bit; bad arguments
launch nothing.  The command on the device against --host.

Measured on one MI355X: see DESIGN.md section 8 (the paint command)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from locator_amd import paint as PT
from tests import paint_util as U

pytestmark = pytest.mark.gpu
QNAN = 0x7fc00000
THETAS = (1e-7, None, 0.5)


def device(case, **kw):
    return PT.copy_device(case["h"], case["donor"], case["owner"], case["rec"], case["rho"], case["theta"], **kw)


def same_bits(a, b):
    return all(np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)) for x, y in zip(a, b))


def cases(H, K):
    yield "planted", U.planted_case(H, K, 100 * H + K)
    for theta in THETAS:
        yield f"edge theta={theta}", U.edge_case(H, K, 100 * H + K + 1, PT.default_theta(H) if theta is None else theta)


# ------------------------------------------------------------------ loc_paint_copy
@pytest.mark.parametrize("K", [1, 2, 7, 8, 9, 29])
@pytest.mark.parametrize("H", [4, 62, 64, 66, 130])
def test_copy_against_the_float64_definition_at_every_block(H, K):
    worst = (0.0, None)
    fills = np.random.default_rng(H + K)
    for name, case in cases(H, K):
        want = U.host(case, np.float64)
        allow = U.allowances(case, want)[0]
        first = None
        for n, block in enumerate((1, 4, 8, 0, K + 3)):
            got = device(case, block=block, fill=QNAN, pad_fill=fills if n % 2 else 0x55, pitch=(H + 15) // 16 * 16 + 16 * (n % 3))
            assert got[0].dtype == got[1].dtype == np.float32 and got[0].shape == got[1].shape == (len(case["rec"]), H)
            assert all(np.isfinite(v).all() for v in got[:3])
            ratios = tuple(d / a for d, a in zip(U.distances(got, want), allow))
            assert max(ratios) <= 1.0, (name, block, ratios, allow)
            if max(ratios) > worst[0]:
                worst = (max(ratios), (name, block, ratios))
            assert np.array_equal(got[3], want[3])
            dn = (case["donor"][None, :] != 0) & (case["owner"][None, :] != case["owner"][case["rec"]][:, None])
            assert not got[0][~dn].any() and not got[1][~dn].any()               # exact zeros off the donors
            dead = want[3] == 0
            assert not got[0][dead].any() and not got[1][dead].any() and not got[2][dead].any()
            assert np.abs(got[0][~dead].astype(np.float64).sum(axis=1) - 1).max(initial=0) < 1e-5
            first = got if first is None else first
            assert same_bits(got, first), (name, block)
    print(f"loc_paint_copy H={H} K={K}: largest error / allowance {worst[0]:.4g} at {worst[1]}")


def test_the_same_bits_whatever_scratch_held_and_whatever_is_appended():
    H, K = 130, 37
    case = U.planted_case(H, K, 3)
    case["donor"][5:9] = 0
    first = device(case, block=1)
    assert U.worst_ratio(first, case)[0] <= 1.0
    for block in (1, 5, 0, K):
        for pattern in (None, QNAN, 0xffffffff, 0x7f800001):
            assert same_bits(device(case, block=block, fill=pattern, pad_fill=np.random.default_rng(block)), first), (block, pattern)
    # appended non-donor columns, across the step from one sweep of 256 columns to two
    for extra in (3, 200):
        more = dict(case)
        more["h"] = np.concatenate([case["h"], np.random.default_rng(extra).integers(-1, 2, (K, extra)).astype(np.int8)], axis=1)
        more["donor"] = np.concatenate([case["donor"], np.zeros(extra, dtype=np.uint8)])
        more["owner"] = np.concatenate([case["owner"], np.full(extra, 9999, dtype=np.int32)])
        got = device(more, block=4)
        assert not got[0][:, H:].any() and not got[1][:, H:].any()
        assert same_bits((got[0][:, :H], got[1][:, :H], got[2], got[3]), first), extra
    # appended recipients, and rec split over two launches
    more = dict(case)
    more["rec"] = np.concatenate([case["rec"], np.array([0, H - 1, 0], dtype=np.int32)])
    got = device(more, block=3)
    n = len(case["rec"])
    assert same_bits([v[:n] for v in got], first)
    cut = n // 3
    a, b = dict(case), dict(case)
    a["rec"], b["rec"] = case["rec"][:cut], case["rec"][cut:]
    assert same_bits([np.concatenate(p) for p in zip(device(a, block=2), device(b, block=7))], first)
    # ... and the batches of a small memory budget are such launches
    assert same_bits(device(case, budget=1), first)


def test_a_long_stretch_without_a_switch_underflows_to_zeros_not_to_nan():
    case = U.no_switch_case()
    got = device(case, fill=QNAN)
    assert all(np.isfinite(v).all() for v in got[:3])
    ratio, parts = U.worst_ratio(got, case)
    print(f"no switch over 200 sites: largest error / allowance {ratio:.4g} {parts}")
    assert ratio <= 1.0
    assert got[0][0, 2] <= 1e-30 and got[1][0, 2] <= 1e-30                        # the donor that never matches
    assert same_bits(device(case, block=1), got) and same_bits(device(case, block=200), got)


def _raw(lib, t, H, K, R, pitch, theta, block, rec=None, work_bytes=None, pattern=0x5a5a5a5a, null_share=False, share_off=0, ll_off=0):
    """One direct call on buffers filled with a pattern: (return code, share, chunks, ll, n_donors as int32 views).  share_off,
    ll_off: bytes by which share and ll are passed off the start of their buffers, which hold a word more than they need."""
    dev = "cuda:0"
    h = t.zeros((max(K, 1), max(pitch, 16)), dtype=t.int8, device=dev)
    donor = t.ones(max(H, 1), dtype=t.uint8, device=dev)
    owner = (t.arange(max(H, 1), dtype=t.int32, device=dev) // 2).contiguous()
    d_rec = t.tensor(list(range(R)) if rec is None else rec, dtype=t.int32, device=dev) if R else t.zeros(1, dtype=t.int32, device=dev)
    rho = t.full((max(K, 1),), 0.1, dtype=t.float32, device=dev)
    outs = [t.empty(max(R * max(H, 1), 1) + 1, dtype=t.int32, device=dev) for _ in range(2)]
    outs += [t.empty(2 * max(R, 1) + 1, dtype=t.int32, device=dev), t.empty(max(R, 1), dtype=t.int32, device=dev)]
    for o in outs:
        o.fill_(int(np.array(pattern, dtype=np.uint32).view(np.int32)))
    need = int(lib.loc_paint_work_bytes(min(max(H, 1), PT.MAX_HAPS), max(K, 0), max(R, 0), max(block, 0)))
    work = t.empty(max(need // 4, 4), dtype=t.float32, device=dev)
    rc = lib.loc_paint_copy(h.data_ptr(), H, K, pitch, donor.data_ptr(), owner.data_ptr(), d_rec.data_ptr(), R, rho.data_ptr(),
                            C.c_float(theta), block, None if null_share else outs[0].data_ptr() + share_off, outs[1].data_ptr(),
                            outs[2].data_ptr() + ll_off, outs[3].data_ptr(), work.data_ptr(), need if work_bytes is None else work_bytes, t.cuda.current_stream().cuda_stream)
    t.cuda.synchronize()
    return rc, [o.cpu().numpy() for o in outs]


OK = dict(H=8, K=5, R=3, pitch=16, theta=0.01, block=0)
BAD = [dict(H=PT.MAX_HAPS + 1, pitch=PT.MAX_HAPS + 16), dict(H=0), dict(rec=[0, 8, 1]), dict(rec=[-1, 0, 1]), dict(theta=0.6),
       dict(theta=5e-8), dict(theta=float("nan")), dict(pitch=0), dict(pitch=24), dict(H=20, pitch=16), dict(work_bytes=16),
       dict(block=-1), dict(K=-1), dict(R=-1), dict(null_share=True)]


def test_bad_arguments_launch_nothing_and_empty_inputs_are_as_specified():
    import torch as t
    from locator_amd import _lib
    lib = _lib.load()
    pat = np.array(0x5a5a5a5a, dtype=np.uint32).view(np.int32)
    ok = OK
    rc, outs = _raw(lib, t, **ok)
    assert rc == 0 and not any((o == pat).all() for o in outs)
    for change in BAD:
        rc, outs = _raw(lib, t, **{**ok, **change})
        assert rc == -1 and lib.loc_last_error(), change
        assert all((o == pat).all() for o in outs), change
    assert lib.loc_paint_work_bytes(PT.MAX_HAPS + 1, 5, 1, 0) == -1 and lib.loc_paint_work_bytes(8, 5, 0, 0) == 0
    rc, outs = _raw(lib, t, **{**ok, "R": 0})
    assert rc == 0 and all((o == pat).all() for o in outs)
    rc, outs = _raw(lib, t, **{**ok, "K": 0})
    assert rc == 0 and not outs[0][:24].any() and not outs[1][:24].any() and not outs[2][:6].any()
    share, chunks, ll, nd = PT.copy_host(np.zeros((0, 8), dtype=np.int8), *U.everyone(4), np.zeros(0), 0.01)
    assert share.shape == (8, 8) and not share.any() and not chunks.any() and not ll.any()


def test_a_refusal_speaks_for_its_own_entry_point_and_misaligned_buffers_are_refused():
    """The launcher's refusals are shared with loc_impute_dose: every message begins with this entry point's name, and the null and
    alignment messages are the literal texts of the launcher before the refusals were shared."""
    import torch as t
    from locator_amd import _lib
    lib = _lib.load()
    pat = np.array(0x5a5a5a5a, dtype=np.uint32).view(np.int32)
    said = lambda: lib.loc_last_error().decode()
    for change in BAD:
        rc, outs = _raw(lib, t, **{**OK, **change})
        assert rc == -1 and said().startswith("loc_paint_copy: "), (change, said())
        if "null_share" in change:
            assert said() == "loc_paint_copy: null buffer"
    for change in (dict(ll_off=4), dict(share_off=2)):                            # ll at 4 mod 8, share at 2 mod 4
        rc, outs = _raw(lib, t, **{**OK, **change})
        assert rc == -1 and all((o == pat).all() for o in outs), change
        assert said() == "loc_paint_copy: share, chunks, n_donors, rho, owner and rec must be multiples of 4 bytes, ll of 8", (change, said())


def test_the_register_limit():
    top, K = PT.MAX_HAPS, 5
    rng = np.random.default_rng(11)
    for H in (top, top - 1):
        hap = rng.integers(0, 2, (K, H)).astype(np.int8)
        hap[rng.random((K, H)) < 0.02] = -1
        case = {"h": hap, "donor": (rng.random(H) < 0.9).astype(np.uint8), "owner": (np.arange(H) // 2).astype(np.int32),
                "rec": np.array([H - 1, 0, 255, 256, H // 2], dtype=np.int32), "rho": np.array([1.0, 0.1, 0.0, 1.0, 0.3]),
                "theta": PT.default_theta(H)}
        got = device(case, block=2, fill=QNAN, pad_fill=rng)
        ratio, parts = U.worst_ratio(got, case)
        print(f"H={H} K={K}: largest error / allowance {ratio:.4g} {parts}")
        assert ratio <= 1.0 and np.array_equal(got[3], U.host(case, np.float64)[3])
        assert same_bits(device(case, block=0), got)
    with pytest.raises(ValueError):
        device({**case, "h": np.zeros((K, top + 1), dtype=np.int8), "donor": np.ones(top + 1, dtype=np.uint8),
                "owner": np.zeros(top + 1, dtype=np.int32)})


# ------------------------------------------------------------------ the command
def test_the_command_on_the_device_against_host(tmp_path):
    vcf = U.write_vcf_cut(str(tmp_path / "cut.vcf"), 40, 60, 900)
    runs = {}
    for name, extra in (("device", []), ("host", ["--host"]), ("host32", ["--host", "--host_dtype", "float32"])):
        out = str(tmp_path / name / "o")
        os.makedirs(os.path.dirname(out))
        assert PT.main(["--vcf", vcf, "--sample_data", U.SAMPLE_DATA, "--out", out, "--silence", "--max_SNPs", "300", "--seed", "3",
                        "--em_rounds", "2", "--kmax", "8"] + extra) == 0
        s = json.load(open(out + "_paint_summary.json"))
        xy = np.loadtxt(out + "_paint_locs.txt", delimiter=",", skiprows=1, usecols=(0, 1))
        hist = np.loadtxt(out + "_paint_history.txt", skiprows=1, ndmin=2)
        runs[name] = (s, xy, hist)
    (sd, xyd, hd), (sh, xyh, hh), (s32, xy32, h32) = runs["device"], runs["host"], runs["host32"]
    assert sd["path"] == "device" and sh["path"] == "host" and sd["K"] == sh["K"] == 300 and sd["N"] == 60
    rel = lambda a, b: float(np.max(np.abs(np.asarray(a, dtype=np.float64) - b) / np.abs(b)))
    scalars = lambda s, h: np.concatenate([[s["ll"], s["switch"]], h[:, 1], h[:, 2]])
    allow = max(U.FACTOR * rel(scalars(s32, h32), scalars(sh, hh)), U.FLOOR)
    err = rel(scalars(sd, hd), scalars(sh, hh))
    print(f"command: switch rate and ll, largest relative error {err:.3g}, allowance {allow:.3g}")
    assert err <= allow
    import pandas as pd
    locs = pd.read_csv(U.SAMPLE_DATA, sep="\t")[["x", "y"]].to_numpy(dtype=np.float64)
    extent = float(np.nanmax(np.nanmax(locs, axis=0) - np.nanmin(locs, axis=0)))
    by_k = lambda s: np.array(s["median_error_by_k"], dtype=np.float64)
    near = max(U.FACTOR * float(np.abs(by_k(s32) - by_k(sh)).max()), 1e-6 * extent)
    best = np.sort(by_k(sh))
    if len(best) < 2 or best[1] - best[0] > near:                                 # else the choice of k is a tie within round-off
        assert sd["k"] == sh["k"]
    if sd["k"] == sh["k"] == s32["k"]:
        dist = lambda xy: float(np.nanmax(np.sqrt(((xy - xyh) ** 2).sum(axis=1))))
        bound = max(U.FACTOR * dist(xy32), 1e-6 * extent)
        print(f"command: placements, largest distance from --host {dist(xyd):.3g}, allowance {bound:.3g} (extent {extent:.3g})")
        assert np.array_equal(np.isnan(xyd), np.isnan(xyh)) and dist(xyd) <= bound
