"""The impute command on the device (locator_amd/csrc/impute_kernels.hip).

loc_impute_dose against impute.dose_host(float64).  The allowance of a case is 8 times the largest distance of dose_host(float32)
from dose_host(float64) on that case over the entries finite in both, floored at 2^-21 (impute_util.allowance).  The device's
NaNs are exactly the structural ones (rows of a recipient without a donor, sites at which no donor holds an allele).  Shapes
around the 64 lanes, the 256 columns of a sweep and the 64 sites of a store run, site counts around the checkpoint blocks, every
block size, planted and edge inputs, pad garbage, NaN-filled scratch and outputs.  ll and n_donors are loc_paint_copy's bits.  No
result depends on the block size, on what scratch held, on appended non-donor columns, on appended recipients or on how rec is
split, bit for bit; every element of dose is written and nothing around it; bad arguments launch nothing.  The command on the
device against --host.

Measured on one MI355X: see DESIGN.md section 8 (the impute command)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from locator_amd import genotypes as G
from locator_amd import impute as IM
from locator_amd import paint as PT
from tests import impute_util as IU
from tests import paint_util as U

pytestmark = pytest.mark.gpu
QNAN = 0x7fc00000
THETAS = (1e-7, None, 0.5)
SIX = ("h", "donor", "owner", "rec", "rho", "theta")


def device(case, **kw):
    return IM.dose_device(*(case[k] for k in SIX), **kw)


def same_bits(a, b):
    return all(np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)) for x, y in zip(a, b))


def cases(H, K):
    yield "planted", U.planted_case(H, K, 100 * H + K)
    for theta in THETAS:
        yield f"edge theta={theta}", U.edge_case(H, K, 100 * H + K + 1, PT.default_theta(H) if theta is None else theta)


def held(got, case, want=None):
    """error / allowance of a device answer, after the checks of its NaNs (the structural ones, float64's) and of n_donors."""
    want = IU.host(case, np.float64) if want is None else want
    nan = IU.structural_nan(case)
    assert got[0].dtype == np.float32 and got[0].shape == (len(case["rec"]), case["h"].shape[0])
    assert np.array_equal(np.isnan(want[0]), nan) and np.array_equal(np.isnan(got[0]), nan)
    assert np.array_equal(got[2], want[2]) and np.isfinite(got[1]).all() and not got[1][want[2] == 0].any()
    assert ((got[0][~nan] >= 0) & (got[0][~nan] <= 1)).all()
    return IU.distance(got[0], want[0]) / IU.allowance(want[0], IU.host(case, np.float32)[0])


# ------------------------------------------------------------------ loc_impute_dose
SHAPES = [(H, K) for H in (4, 62, 64, 66, 130) for K in (1, 2, 7, 8, 9, 29)] + [(H, K) for H in (6, 66) for K in (63, 64, 65, 129)]


@pytest.mark.parametrize("H,K", SHAPES)
def test_dose_against_the_float64_definition_at_every_block(H, K):
    worst = (0.0, None)
    fills = np.random.default_rng(H + K)
    for name, case in cases(H, K):
        want = IU.host(case, np.float64)
        first = None
        for n, block in enumerate((1, 4, 8, 0, K + 3)):
            got = device(case, block=block, fill=QNAN, pad_fill=fills if n % 2 else 0x55, pitch=(H + 15) // 16 * 16 + 16 * (n % 3))
            ratio = held(got, case, want)
            assert ratio <= 1.0, (name, block, ratio)
            if ratio > worst[0]:
                worst = (ratio, (name, block))
            first = got if first is None else first
            assert same_bits(got, first), (name, block)
        copied = PT.copy_device(*(case[k] for k in SIX), fill=QNAN)
        assert same_bits(first[1:], copied[2:]), name                            # ll and n_donors: the same forward pass
    print(f"loc_impute_dose H={H} K={K}: largest error / allowance {worst[0]:.4g} at {worst[1]}")


def test_the_same_bits_whatever_scratch_held_and_whatever_is_appended():
    H, K = 130, 37
    case = U.planted_case(H, K, 3)
    case["donor"][5:9] = 0
    first = device(case, block=1)
    assert held(first, case) <= 1.0
    for block in (1, 5, 0, K):
        for pattern in (None, QNAN, 0xffffffff, 0x7f800001):
            assert same_bits(device(case, block=block, fill=pattern, pad_fill=np.random.default_rng(block)), first), (block, pattern)
    # appended non-donor columns, across the step from one sweep of 256 columns to two
    for extra in (3, 200):
        more = dict(case)
        more["h"] = np.concatenate([case["h"], np.random.default_rng(extra).integers(-1, 2, (K, extra)).astype(np.int8)], axis=1)
        more["donor"] = np.concatenate([case["donor"], np.zeros(extra, dtype=np.uint8)])
        more["owner"] = np.concatenate([case["owner"], np.full(extra, 9999, dtype=np.int32)])
        assert same_bits(device(more, block=4), first), extra
    # appended and repeated recipients, and rec split over two launches at different block sizes
    more = dict(case)
    more["rec"] = np.concatenate([case["rec"], np.array([0, H - 1, 0], dtype=np.int32)])
    got = device(more, block=3)
    n = len(case["rec"])
    assert same_bits([v[:n] for v in got], first) and same_bits([v[n:n + 1] for v in got], [v[n + 2:] for v in got])
    cut = n // 3
    a, b = dict(case), dict(case)
    a["rec"], b["rec"] = case["rec"][:cut], case["rec"][cut:]
    assert same_bits([np.concatenate(p) for p in zip(device(a, block=2), device(b, block=7))], first)
    # ... and the batches of a small memory budget are such launches
    assert same_bits(device(case, budget=1), first)


def _raw(lib, t, H, K, R, pitch, theta, block, rec=None, work_bytes=None, pattern=0x5a5a5a5a, null_dose=False, case=None, dose_off=0,
         ll_off=0):
    """One direct call on buffers filled with a pattern, dose 64 floats inside a larger buffer: (return code, [the whole dose
    buffer, ll, n_donors] as int32 views).  case: its haplotypes, flags and rho instead of zeros, ones and 0.1.  dose_off, ll_off:
    bytes by which dose and ll are passed further into their buffers (ll's holds a word more than it needs)."""
    dev = "cuda:0"
    put = lambda v, dt: t.from_numpy(np.ascontiguousarray(v, dtype=dt)).to(dev)
    if case is None:
        h = t.zeros((max(K, 1), max(pitch, 16)), dtype=t.int8, device=dev)
        donor = t.ones(max(H, 1), dtype=t.uint8, device=dev)
        owner = (t.arange(max(H, 1), dtype=t.int32, device=dev) // 2).contiguous()
        rho = t.full((max(K, 1),), 0.1, dtype=t.float32, device=dev)
    else:
        h, donor, owner = put(IM.B.padded(case["h"], pitch), np.int8), put(case["donor"], np.uint8), put(case["owner"], np.int32)
        rho = put(case["rho"], np.float32)
    d_rec = t.tensor(list(range(R)) if rec is None else list(rec), dtype=t.int32, device=dev) if R else t.zeros(1, dtype=t.int32, device=dev)
    outs = [t.empty(128 + max(R, 0) * max(K, 0), dtype=t.int32, device=dev), t.empty(2 * max(R, 1) + 1, dtype=t.int32, device=dev),
            t.empty(max(R, 1), dtype=t.int32, device=dev)]
    for o in outs:
        o.fill_(int(np.array(pattern, dtype=np.uint32).view(np.int32)))
    need = int(lib.loc_paint_work_bytes(min(max(H, 1), PT.MAX_HAPS), max(K, 0), max(R, 0), max(block, 0)))
    work = t.empty(max(need // 4, 4), dtype=t.float32, device=dev)
    rc = lib.loc_impute_dose(h.data_ptr(), H, K, pitch, donor.data_ptr(), owner.data_ptr(), d_rec.data_ptr(), R, rho.data_ptr(),
                             C.c_float(theta), block, None if null_dose else outs[0].data_ptr() + 4 * 64 + dose_off,
                             outs[1].data_ptr() + ll_off,
                             outs[2].data_ptr(), work.data_ptr(), need if work_bytes is None else work_bytes,
                             t.cuda.current_stream().cuda_stream)
    t.cuda.synchronize()
    return rc, [o.cpu().numpy() for o in outs]


@pytest.mark.parametrize("K", [1, 63, 64, 65, 129])
def test_every_dose_is_stored_and_nothing_around_them(K):
    import torch as t
    from locator_amd import _lib
    lib = _lib.load()
    pat = np.array(0x5a5a5a5a, dtype=np.uint32).view(np.int32)
    H, R = 8, 3
    case = U.planted_case(H, K, 40 + K)
    case["rec"] = np.array([5, 2, 0], dtype=np.int32)                             # descending
    for block in (0, 1, 64):
        rc, outs = _raw(lib, t, H, K, R, 16, case["theta"], block, rec=case["rec"], case=case)
        assert rc == 0
        inner = outs[0][64:64 + R * K]
        assert (outs[0][:64] == pat).all() and (outs[0][64 + R * K:] == pat).all() and not (inner == pat).any()
        assert same_bits([inner.view(np.float32).reshape(R, K)], device(case)[:1])


OK = dict(H=8, K=5, R=3, pitch=16, theta=0.01, block=0)
BAD = [dict(H=PT.MAX_HAPS + 1, pitch=PT.MAX_HAPS + 16), dict(H=0), dict(rec=[0, 8, 1]), dict(rec=[-1, 0, 1]), dict(theta=0.6),
       dict(theta=5e-8), dict(theta=float("nan")), dict(pitch=0), dict(pitch=24), dict(H=20, pitch=16), dict(work_bytes=16),
       dict(block=-1), dict(K=-1), dict(R=-1), dict(null_dose=True)]


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
    rc, outs = _raw(lib, t, **{**ok, "R": 0})
    assert rc == 0 and all((o == pat).all() for o in outs)
    rc, outs = _raw(lib, t, **{**ok, "K": 0})
    assert rc == 0 and (outs[0] == pat).all() and not outs[1][:6].any() and not outs[2][:3].any()      # ll, n_donors zeros, no dose
    dose, ll, nd = IM.dose_device(np.zeros((0, 8), dtype=np.int8), *U.everyone(4), np.zeros(0), 0.01)
    assert dose.shape == (8, 0) and not ll.any() and not nd.any()


def test_a_refusal_speaks_for_its_own_entry_point_and_misaligned_buffers_are_refused():
    """The launcher's refusals are shared with loc_paint_copy: every message begins with this entry point's name, and the null and
    alignment messages are the literal texts of the launcher before the refusals were shared."""
    import torch as t
    from locator_amd import _lib
    lib = _lib.load()
    pat = np.array(0x5a5a5a5a, dtype=np.uint32).view(np.int32)
    said = lambda: lib.loc_last_error().decode()
    for change in BAD:
        rc, outs = _raw(lib, t, **{**OK, **change})
        assert rc == -1 and said().startswith("loc_impute_dose: "), (change, said())
        if "null_dose" in change:
            assert said() == "loc_impute_dose: null buffer"
    for change in (dict(ll_off=4), dict(dose_off=2)):                             # ll at 4 mod 8, dose at 2 mod 4
        rc, outs = _raw(lib, t, **{**OK, **change})
        assert rc == -1 and all((o == pat).all() for o in outs), change
        assert said() == "loc_impute_dose: dose, n_donors, rho, owner and rec must be multiples of 4 bytes, ll of 8", (change, said())


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
        ratio = held(got, case)
        print(f"H={H} K={K}: largest error / allowance {ratio:.4g}")
        assert ratio <= 1.0 and same_bits(device(case, block=0), got)
    with pytest.raises(ValueError):
        device({**case, "h": np.zeros((K, top + 1), dtype=np.int8), "donor": np.ones(top + 1, dtype=np.uint8),
                "owner": np.zeros(top + 1, dtype=np.int32)})


def test_a_long_stretch_without_a_switch_gives_no_nan_where_float32_has_none():
    case = U.no_switch_case()
    got = device(case, fill=QNAN)
    want, w32 = IU.host(case, np.float64), IU.host(case, np.float32)
    assert np.isfinite(got[0][np.isfinite(w32[0])]).all() and np.isfinite(got[1]).all() and np.array_equal(got[2], want[2])
    ratio = IU.distance(got[0], want[0]) / IU.allowance(want[0], w32[0])
    print(f"no switch over 200 sites: largest error / allowance {ratio:.4g}")
    assert ratio <= 1.0
    assert same_bits(device(case, block=1), got) and same_bits(device(case, block=200), got)


# ------------------------------------------------------------------ the command
def test_the_command_on_the_device_against_host(tmp_path):
    panel, target = IU.golden_panel(str(tmp_path), 40, 20, 300)
    runs = {}
    for name, extra in (("device", []), ("host", ["--host"]), ("host32", ["--host", "--host_dtype", "float32"])):
        out = str(tmp_path / name / "o")
        os.makedirs(os.path.dirname(out))
        assert IM.main(["--vcf", target, "--panel", panel, "--out", out, "--silence", "--em_rounds", "2"] + extra) == 0
        s = json.load(open(out + "_impute_summary.json"))
        callset = G.open_group(out + "_imputed.zarr", mode="r")
        hist = np.loadtxt(out + "_impute_history.txt", skiprows=1, ndmin=2)
        runs[name] = (s, np.asarray(callset["calldata/DS"][:]), np.asarray(callset["calldata/GT"][:]), hist)
    (sd, dsd, gtd, hd), (sh, dsh, gth, hh), (s32, ds32, gt32, h32) = runs["device"], runs["host"], runs["host32"]
    assert sd["path"] == "device" and sh["path"] == "host" and (sd["K"], sd["N"], sd["recipients"], sd["untyped"]) == (300, 20, 40, 225)
    assert {k: v for k, v in sd.items() if k not in ("ll", "switch", "path")} == {k: v for k, v in sh.items() if k not in ("ll", "switch", "path")}
    assert np.array_equal(gtd, gth) and np.array_equal(np.isnan(dsd), np.isnan(dsh)) and dsd.dtype == np.float32
    allow = 2 * max(U.FACTOR * IU.distance(ds32, dsh), U.FLOOR)                   # two haplotypes add
    print(f"command: DS, largest distance from --host {IU.distance(dsd, dsh):.3g}, allowance {allow:.3g}")
    assert IU.distance(dsd, dsh) <= allow
    rel = lambda a, b: float(np.max(np.abs(np.asarray(a, dtype=np.float64) - b) / np.abs(b)))
    scalars = lambda s, h: np.concatenate([[s["ll"], s["switch"]], h[:, 1], h[:, 2]])
    allow = max(U.FACTOR * rel(scalars(s32, h32), scalars(sh, hh)), U.FLOOR)
    err = rel(scalars(sd, hd), scalars(sh, hh))
    print(f"command: switch rate and ll, largest relative error {err:.3g}, allowance {allow:.3g}")
    assert err <= allow
    # a check run on the cut itself (fill mode): with --host, mse 0.0032 against 0.0570 of the donors' frequency
    cut = U.write_vcf_cut(str(tmp_path / "cut.vcf"), 40, 60, 300)
    out = str(tmp_path / "check")
    assert IM.main(["--vcf", cut, "--out", out, "--silence", "--em_rounds", "2", "--check_mask", "0.1", "--seed", "7"]) == 0
    s = json.load(open(out + "_impute_summary.json"))
    print(f"check run: mse {s['mse']:.4f} against {s['mse_frequency']:.4f} of the donors' frequency, {s['masked']} hidden")
    assert s["path"] == "device" and s["mse"] <= 0.5 * s["mse_frequency"] and not os.path.exists(out + "_imputed.zarr")
