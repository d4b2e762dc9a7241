"""The ancestry command on the device (locator_amd/csrc/local_kernels.hip).

loc_paint_local against ancestry.local_host(float64) on the window means out / n_sites.  The allowance of a case is 8 times the
distance of local_host(float32) from local_host(float64) on that case, floored at 2^-21 (ancestry_util.allowance).  Shapes around
the 64 lanes and the 256 columns of a sweep, site counts around the checkpoint blocks, every block size, every window layout that
fits, 1, 3 and 64 channels, planted and edge inputs, pad garbage in h and v, NaN attributes at every non-donor column, NaN-filled
scratch and outputs.  ll and n_donors are loc_paint_copy's bits, and with one window of all sites and one-hot channels so is
out: share K exactly.  No result depends on the block size, on what scratch held, on appended non-donor columns, on appended
recipients or on how rec is split, on the other windows or the other channels of the call, bit for bit; every element of out is
written and nothing around it; bad arguments launch nothing.  The command on the device against --host.

Measured on one MI355X: see DESIGN.md (the ancestry command)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from locator_amd import ancestry as AN
from locator_amd import genotypes as G
from locator_amd import paint as PT
from tests import ancestry_util as AU
from tests import paint_util as U

pytestmark = pytest.mark.gpu
QNAN = 0x7fc00000
THETAS = (1e-7, None, 0.5)
SIX = AU.SIX
PAT = np.array(0x5a5a5a5a, dtype=np.uint32).view(np.int32)


def device(case, v, win, **kw):
    return AN.local_device(*(case[k] for k in SIX), v, win, **kw)


def same_bits(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) for x, y in zip(a, b))


def thinned(case, H):
    """The case with at most 18 recipients where it has many columns (the definition's cost a recipient grows with them): the
    first 16 of its own order, then the last and the first column."""
    if H < 130:
        return case
    return {**case, "rec": np.concatenate([case["rec"][:16], np.array([H - 1, 0], dtype=np.int32)])}


def cases(H, K):
    yield "planted", thinned(U.planted_case(H, K, 100 * H + K), H)
    for theta in THETAS:
        yield f"edge theta={theta}", thinned(U.edge_case(H, K, 100 * H + K + 1, PT.default_theta(H) if theta is None else theta), H)


# ------------------------------------------------------------------ loc_paint_local
@pytest.mark.parametrize("K", (1, 2, 7, 8, 9, 29, 63, 64, 65, 129))
@pytest.mark.parametrize("H", (4, 62, 64, 66, 130, 258))
def test_window_sums_against_the_float64_definition_at_every_block(H, K):
    """The reference is computed once a case and layout with all 64 channels; a launch with 1 or 3 channels takes a selection of
    them (ancestry_util.SUBSETS) and must give those channels' bits: no channel depends on the others."""
    worst = (0.0, None)
    fills = np.random.default_rng(H + K)
    for name, case in cases(H, K):
        v = AU.attributes(case, H + K)
        copied = PT.copy_device(*(case[k] for k in SIX), fill=QNAN)
        for lname, win in AU.layouts(K).items():
            allow, want = AU.allowance(case, v, win)
            first = None
            for n, (block, Cn) in enumerate(zip((1, 4, 8, 0, K + 3), (64, 1, 3, 64, 3))):
                sel = AU.SUBSETS[Cn]
                got = device(case, v[sel], win, block=block, fill=QNAN, pad_fill=fills if n % 2 else 0x55,
                             pitch=(H + 15) // 16 * 16 + 16 * (n % 3), vpitch=(H + 3) // 4 * 4 + 4 * (n % 4), v_pad=fills if n % 2 else np.nan)
                assert got[0].dtype == np.float32 and got[0].shape == (len(case["rec"]), len(win), Cn)
                assert np.isfinite(got[0]).all() and np.array_equal(got[2], want[2]) and not got[0][want[2] == 0].any()
                ratio = AU.distance(got[0], want[0][:, :, sel], win) / allow
                assert ratio <= 1.0, (name, lname, block, Cn, ratio)
                if ratio > worst[0]:
                    worst = (ratio, (name, lname, block, Cn))
                first = got if first is None else first
                assert same_bits([got[0], *got[1:]], [first[0][:, :, sel], *first[1:]]), (name, lname, block, Cn)
            assert same_bits(first[1:], copied[2:]), (name, lname)                     # ll and n_donors: the same forward pass
    print(f"loc_paint_local H={H} K={K}: largest error / allowance {worst[0]:.4g} at {worst[1]}")


@pytest.mark.parametrize("K", (8, 64))
def test_one_window_of_all_sites_and_one_hot_channels_give_the_bits_of_the_shares(K):
    """out[i][0][c] = S(d_c) exactly (one term 1 S + 0, zeros from every other lane) and share = S / K with K a power of two."""
    for H in (6, 66, 130, 300):
        case = U.planted_case(H, K, 7 * H + K)
        share = PT.copy_device(*(case[k] for k in SIX))[0]
        cols = np.flatnonzero(case["donor"])
        for a in range(0, len(cols), 64):
            part = cols[a:a + 64]
            v = np.full((len(part), H), np.nan)
            v[:, cols] = 0.0
            v[np.arange(len(part)), part] = 1.0
            out = device(case, v, np.array([[0, K]], dtype=np.int32))[0]
            assert same_bits([out[:, 0, :]], [share[:, part] * np.float32(K)]), (H, a)


def test_the_same_bits_whatever_scratch_held_and_whatever_is_appended():
    H, K = 130, 37
    case = U.planted_case(H, K, 3)
    case["donor"][5:9] = 0
    v = AU.attributes(case, 9)[AU.SUBSETS[3]]
    win = AU.layouts(K)["fives"]
    first = device(case, v, win, block=1)
    assert AU.distance(first[0], AU.host(case, v, win)[0], win) <= AU.allowance(case, v, win)[0]
    for block in (1, 5, 0, K):
        for pattern in (None, QNAN, 0xffffffff, 0x7f800001):
            got = device(case, v, win, block=block, fill=pattern, pad_fill=np.random.default_rng(block), v_pad=np.random.default_rng(block))
            assert same_bits(got, first), (block, pattern)
    # appended non-donor columns with NaN attributes, across the step from one sweep of 256 columns to two
    for extra in (3, 200):
        more = dict(case)
        more["h"] = np.concatenate([case["h"], np.random.default_rng(extra).integers(-1, 2, (K, extra)).astype(np.int8)], axis=1)
        more["donor"] = np.concatenate([case["donor"], np.zeros(extra, dtype=np.uint8)])
        more["owner"] = np.concatenate([case["owner"], np.full(extra, 9999, dtype=np.int32)])
        assert same_bits(device(more, np.concatenate([v, np.full((3, extra), np.nan)], axis=1), win, block=4), first), extra
    # appended and repeated recipients, and rec split over two launches at different block sizes
    more = dict(case)
    more["rec"] = np.concatenate([case["rec"], np.array([0, H - 1, 0], dtype=np.int32)])
    got = device(more, v, win, block=3)
    n = len(case["rec"])
    assert same_bits([x[:n] for x in got], first) and same_bits([x[n:n + 1] for x in got], [x[n + 2:] for x in got])
    cut = n // 3
    a, b = dict(case), dict(case)
    a["rec"], b["rec"] = case["rec"][:cut], case["rec"][cut:]
    assert same_bits([np.concatenate(p) for p in zip(device(a, v, win, block=2), device(b, v, win, block=7))], first)
    # ... and the batches of a small memory budget are such launches
    assert same_bits(device(case, v, win, budget=1), first)


def test_the_same_bits_whichever_other_windows_and_channels_are_in_the_call():
    H, K = 66, 65
    case = U.edge_case(H, K, 12, 0.02)
    v = AU.attributes(case, 2)
    for win in AU.layouts(K).values():
        whole = device(case, v, win, block=4)
        for keep in ([len(win) - 1], [0], list(range(0, len(win), 2))):
            part = device(case, v, win[keep], block=0)
            assert same_bits([part[0], *part[1:]], [whole[0][:, keep], *whole[1:]]), keep
        for sel in ([63], [40, 0, 63, 2], list(range(63, -1, -1))):                    # a subset, a reordering
            part = device(case, v[sel], win[:3])
            assert same_bits([part[0]], [whole[0][:, :3][:, :, sel]]), sel


def _raw(lib, t, H, K, R, pitch, theta, block, Cn=3, W=1, vpitch=None, win=None, rec=None, work_bytes=None, null=(), off=None, case=None,
         v=None):
    """One direct call on buffers filled with a pattern, out R W C floats inside a larger buffer: (return code, [the whole out
    buffer, ll, n_donors] as int32 views).  case: its haplotypes, flags and rho instead of zeros, ones and 0.1.  null: arguments
    passed as null pointers; off: (argument, bytes) by which one is passed further into its buffer."""
    dev = "cuda:0"
    put = lambda x, dt: t.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)
    vpitch = (max(H, 1) + 3) // 4 * 4 if vpitch is None else vpitch
    if case is None:
        h = t.zeros((max(K, 1), max(pitch, 16)), dtype=t.int8, device=dev)
        donor = t.ones(max(H, 1), dtype=t.uint8, device=dev)
        owner = (t.arange(max(H, 1), dtype=t.int32, device=dev) // 2).contiguous()
        rho = t.full((max(K, 1),), 0.1, dtype=t.float32, device=dev)
    else:
        h, donor, owner = put(AN.B.padded(case["h"], pitch), np.int8), put(case["donor"], np.uint8), put(case["owner"], np.int32)
        rho = put(case["rho"], np.float32)
    d_v = t.ones((max(Cn, 1) + 1, max(vpitch, 4) + 4), dtype=t.float32, device=dev)
    if v is not None:
        d_v = put(np.concatenate([v, np.ones((1, v.shape[1]))]), np.float32)
    win = [[0, max(K, 1)]] if win is None else win
    d_win = put(np.concatenate([np.asarray(win).reshape(-1), [0, 0]]), np.int32)
    d_rec = t.tensor(list(range(R)) if rec is None else list(rec), dtype=t.int32, device=dev) if R > 0 else t.zeros(1, dtype=t.int32, device=dev)
    cells = max(R, 0) * max(W, 0) * max(Cn, 0)
    outs = [t.empty(128 + cells, dtype=t.int32, device=dev), t.empty(2 * max(R, 1) + 1, dtype=t.int32, device=dev),
            t.empty(max(R, 1), dtype=t.int32, device=dev)]
    for o in outs:
        o.fill_(int(PAT))
    need = int(lib.loc_paint_work_bytes(min(max(H, 1), PT.MAX_HAPS), max(K, 0), max(R, 0), max(block, 0)))
    work = t.empty(max(need // 4, 4), dtype=t.float32, device=dev)
    ptr = {"v": d_v.data_ptr(), "win": d_win.data_ptr(), "out": outs[0].data_ptr() + 4 * 64, "ll": outs[1].data_ptr()}
    for name in null:
        ptr[name] = None
    if off:
        ptr[off[0]] += off[1]
    rc = lib.loc_paint_local(h.data_ptr(), H, K, pitch, donor.data_ptr(), owner.data_ptr(), d_rec.data_ptr(), R, rho.data_ptr(),
                             C.c_float(theta), block, ptr["v"], Cn, vpitch, ptr["win"], W, ptr["out"], ptr["ll"], outs[2].data_ptr(),
                             work.data_ptr(), need if work_bytes is None else work_bytes, t.cuda.current_stream().cuda_stream)
    t.cuda.synchronize()
    return rc, [o.cpu().numpy() for o in outs]


@pytest.mark.parametrize("Cn", [1, 63, 64])
def test_every_element_is_stored_and_nothing_around_them(Cn):
    import torch as t
    from locator_amd import _lib
    lib = _lib.load()
    H, R, K = 8, 3, 9
    case = U.planted_case(H, K, 40 + Cn)
    case["rec"] = np.array([5, 2, 0], dtype=np.int32)                             # descending
    v = AU.attributes(case, 4)[AU.SUBSETS[Cn]]
    v[:, case["donor"] != 0] += 0.25                                              # no sum is the pattern's value by accident, none is 0
    for win in ([[0, K]], [[1, 4], [4, 9]], [[j, j + 1] for j in range(K)]):
        W = len(win)
        for block in (0, 1, 64):
            rc, outs = _raw(lib, t, H, K, R, 16, case["theta"], block, Cn=Cn, W=W, win=win, rec=case["rec"], case=case,
                            v=np.nan_to_num(v, nan=7.0))
            assert rc == 0
            inner = outs[0][64:64 + R * W * Cn]
            assert (outs[0][:64] == PAT).all() and (outs[0][64 + R * W * Cn:] == PAT).all() and not (inner == PAT).any()
            assert same_bits([inner.view(np.float32).reshape(R, W, Cn)], device(case, v, np.array(win, dtype=np.int32))[:1])
    # a recipient without a donor: rows of zeros, written
    lone = U.edge_case(4, 8, 1, 0.01)
    assert (lone["owner"][lone["donor"] != 0] == 0).all()
    rc, outs = _raw(lib, t, 4, 8, 4, 16, 0.01, 0, Cn=Cn, W=2, win=[[0, 3], [5, 8]], rec=lone["rec"], case=lone, v=np.ones((Cn, 4)))
    got = outs[0][64:64 + 4 * 2 * Cn].reshape(4, 2, Cn)
    none = lone["owner"][lone["rec"]] == 0
    assert rc == 0 and none.any() and not got[none].any() and not (got == PAT).any() and (outs[0][64 + 8 * Cn:] == PAT).all()
    assert not outs[2][none].any() and not outs[1][:8].reshape(4, 2)[none].any()


OK = dict(H=8, K=5, R=3, pitch=16, theta=0.01, block=0)
NEW = [dict(Cn=0), dict(Cn=65), dict(W=0), dict(W=6, win=[[j, j + 1] for j in range(6)]), dict(vpitch=4), dict(vpitch=10), dict(K=0),
       dict(null=("v",)), dict(null=("win",)), dict(null=("out",)), dict(null=("ll",)), dict(off=("v", 4)), dict(off=("win", 2)),
       dict(off=("out", 2)), dict(off=("ll", 4)), dict(win=[[2, 2]]), dict(win=[[3, 2]]), dict(win=[[0, 6]]), dict(win=[[-1, 2]]),
       dict(W=2, win=[[0, 3], [2, 5]]), dict(W=2, win=[[3, 5], [0, 2]]), dict(W=3, win=[[0, 1], [1, 2], [2, 7]])]


def _bad():
    from tests.test_gpu_impute import BAD
    shared = [{("null" if k == "null_dose" else k): (("out",) if k == "null_dose" else x) for k, x in change.items()} for change in BAD]
    for change in shared:
        if change.get("H", 0) > PT.MAX_HAPS:
            change["vpitch"] = change["H"] + 3
    return shared + NEW


def test_bad_arguments_launch_nothing_and_every_refusal_names_the_entry_point():
    import torch as t
    from locator_amd import _lib
    lib = _lib.load()
    said = lambda: lib.loc_last_error().decode()
    rc, outs = _raw(lib, t, **OK)
    assert rc == 0 and not any((o == PAT).all() for o in outs)
    for change in _bad():
        rc, outs = _raw(lib, t, **{**OK, **change})
        assert rc == -1 and said().startswith("loc_paint_local: "), (change, said())
        assert all((o == PAT).all() for o in outs), change
    for change, index in ((dict(W=2, win=[[0, 3], [2, 5]]), "win[1]"), (dict(win=[[0, 6]]), "win[0]"), (dict(W=3, win=[[0, 1], [1, 2], [2, 7]]), "win[2]")):
        rc, outs = _raw(lib, t, **{**OK, **change})
        assert rc == -1 and index in said(), (change, said())
    rc, outs = _raw(lib, t, **{**OK, "R": 0})
    assert rc == 0 and all((o == PAT).all() for o in outs)
    rc, outs = _raw(lib, t, **{**OK, "R": 0, "Cn": 65})                              # the sizes are refused before R = 0 returns
    assert rc == -1 and said().startswith("loc_paint_local: C=65")


def test_the_register_limit():
    top, K = PT.MAX_HAPS, 5
    rng = np.random.default_rng(11)
    win = np.array([[0, 2], [3, 5]], dtype=np.int32)
    for H in (top, top - 1):
        hap = rng.integers(0, 2, (K, H)).astype(np.int8)
        hap[rng.random((K, H)) < 0.02] = -1
        case = {"h": hap, "donor": (rng.random(H) < 0.9).astype(np.uint8), "owner": (np.arange(H) // 2).astype(np.int32),
                "rec": np.array([H - 1, 0, 255, 256, H // 2], dtype=np.int32), "rho": np.array([1.0, 0.1, 0.0, 1.0, 0.3]),
                "theta": PT.default_theta(H)}
        v = np.stack([rng.uniform(-1.0, 1.0, H), np.ones(H)])
        v[:, case["donor"] == 0] = np.nan
        got = device(case, v, win, block=2, fill=QNAN, pad_fill=rng, v_pad=rng)
        allow, want = AU.allowance(case, v, win)
        ratio = AU.distance(got[0], want[0], win) / allow
        print(f"H={H} K={K}: largest error / allowance {ratio:.4g}")
        assert ratio <= 1.0 and np.array_equal(got[2], want[2]) and same_bits(device(case, v, win, block=0), got)
        assert same_bits(got[1:], PT.copy_device(*(case[k] for k in SIX))[2:])
    with pytest.raises(ValueError):
        device({**case, "h": np.zeros((K, top + 1), dtype=np.int8), "donor": np.ones(top + 1, dtype=np.uint8),
                "owner": np.zeros(top + 1, dtype=np.int32)}, np.ones((1, top + 1)), win)


def test_a_long_stretch_without_a_switch_gives_finite_sums_wherever_float32_does():
    case = U.no_switch_case()
    v = np.stack([np.arange(6) % 2, np.linspace(-1.0, 1.0, 6), np.ones(6)]).astype(np.float64)
    win = AU.layouts(200)["fives"]
    got = device(case, v, win, fill=QNAN)
    w32 = AU.host(case, v, win, np.float32)
    allow, want = AU.allowance(case, v, win)
    assert np.isfinite(got[0][np.isfinite(w32[0])]).all() and np.isfinite(got[1]).all() and np.array_equal(got[2], want[2])
    ratio = AU.distance(got[0], want[0], win) / allow
    print(f"no switch over 200 sites: largest error / allowance {ratio:.4g}")
    assert ratio <= 1.0
    assert same_bits(device(case, v, win, block=1), got) and same_bits(device(case, v, win, block=200), got)


# ------------------------------------------------------------------ the command
def test_the_command_on_the_device_against_host(tmp_path):
    import pandas as pd
    vcf = U.write_vcf_cut(str(tmp_path / "cut.vcf"), 40, 40, 300)
    with open(vcf) as fh:
        ids = next(line for line in fh if line.startswith("#CHROM")).rstrip("\n").split("\t")[9:]
    truth = pd.read_csv(U.SAMPLE_DATA, sep="\t").set_index("sampleID").reindex(ids)
    labels = str(tmp_path / "labels.txt")
    with open(labels, "w") as fh:
        fh.write("sampleID\tlabel\n" + "".join(f"{s}\t{'NA' if np.isnan(x) else 'east' if x >= np.nanmedian(truth['x']) else 'west'}\n"
                                               for s, x in zip(ids, truth["x"])))
    runs = {}
    for name, extra in (("device", []), ("host", ["--host"]), ("host32", ["--host", "--host_dtype", "float32"])):
        out = str(tmp_path / name / "o")
        os.makedirs(os.path.dirname(out))
        assert AN.main(["--vcf", vcf, "--out", out, "--sample_data", U.SAMPLE_DATA, "--labels", labels, "--window_snps", "40", "--silence",
                        "--em_rounds", "2", "--keep_windows"] + extra) == 0
        s = json.load(open(out + "_ancestry_summary.json"))
        store = G.open_group(out + "_ancestry.zarr", mode="r")
        hist = np.loadtxt(out + "_ancestry_history.txt", skiprows=1, ndmin=2)
        q = pd.read_csv(out + "_ancestry_Q.txt", sep="\t", keep_default_na=False)
        runs[name] = (s, np.asarray(store["mass"][:], dtype=np.float64), np.asarray(store["local"][:], dtype=np.float64), hist, q,
                      pd.read_csv(out + "_ancestry_locs.txt"), open(out + "_ancestry_windows.txt").read(),
                      sorted(os.listdir(out + "_ancestry_windows")), [str(x) for x in store["samples"][:]],
                      np.asarray(store["windows/n_sites"][:]))
    d, h, h32 = runs["device"], runs["host"], runs["host32"]
    floats = ("ll", "switch", "path", "r2_x", "r2_y", "mean_error", "median_error", "min_mass", "label_accuracy")
    assert d[0]["path"] == "device" and h[0]["path"] == "host" and d[0]["W"] == -(-d[0]["K"] // 40) and d[0]["C"] == 5
    assert {k: x for k, x in d[0].items() if k not in floats} == {k: x for k, x in h[0].items() if k not in floats}
    assert d[6] == h[6] and d[7] == h[7] and d[8] == h[8] and np.array_equal(d[9], h[9])     # tables of integers and text
    assert list(d[4]["sampleID"]) == list(h[4]["sampleID"]) and list(d[4]["label"]) == list(h[4]["label"])
    # the channels in units of their range: labels and mass as they are, coordinates over the donors' largest deviation
    xy = truth[["x", "y"]].to_numpy()
    scale = np.nanmax(np.abs(xy - np.nanmean(xy, axis=0)))
    unit = np.array([1.0, 1.0, scale, scale])
    dist = lambda a, b: float(max(np.abs(a[1] - b[1]).max(), (np.abs(a[2] - b[2]) / unit).max()))
    allow = max(U.FACTOR * dist(h32, h), U.FLOOR)
    print(f"command: mass and local, largest distance from --host {dist(d, h):.3g}, allowance {allow:.3g}")
    assert dist(d, h) <= allow
    tables = lambda r: np.concatenate([r[4][["east", "west"]].to_numpy().reshape(-1), r[5][["x", "y"]].to_numpy().reshape(-1) / scale])
    allow = max(U.FACTOR * float(np.abs(tables(h32) - tables(h)).max()), U.FLOOR)
    err = float(np.abs(tables(d) - tables(h)).max())
    print(f"command: Q and locations, largest distance from --host {err:.3g}, allowance {allow:.3g}")
    assert err <= allow
    rel = lambda a, b: float(np.max(np.abs(np.asarray(a, dtype=np.float64) - b) / np.abs(b)))
    scalars = lambda r: np.concatenate([[r[0]["ll"], r[0]["switch"]], r[3][:, 1], r[3][:, 2]])
    allow = max(U.FACTOR * rel(scalars(h32), scalars(h)), U.FLOOR)
    err = rel(scalars(d), scalars(h))
    print(f"command: switch rate and ll, largest relative error {err:.3g}, allowance {allow:.3g}")
    assert err <= allow
