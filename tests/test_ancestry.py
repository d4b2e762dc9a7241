"""The ancestry command without a GPU: the binding through _abi's open table, the refusals of loc_paint_local that need no
device, the NumPy definition (the mass channel, the link to copy_host's shares, a spliced recipient's junction, the recovery of
planted locations and labels), the --host command on a cut of the golden VCF and its refusals."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from locator_amd import ancestry as AN
from locator_amd import genotypes as G
from locator_amd import paint as PT
from tests import ancestry_util as AU
from tests import paint_util as U


# ------------------------------------------------------------------ the binding
def test_the_open_table_binds_the_local_header():
    """What tests.abi_util.check_extension asserts of a line of _abi's first table, here of the line `local` of the open table:
    the table's other keys are not looked at."""
    from locator_amd import _abi, _lib
    from tests import abi_util
    vp, i64, i, f = C.c_void_p, C.c_int64, C.c_int, C.c_float
    prototypes = {"loc_paint_local": (i, [vp, i, i64, i64, vp, vp, vp, i, vp, f, i, vp, i, i64, vp, i, vp, vp, vp, vp, i64, vp])}
    ext = _abi.OPEN["local"]
    assert ext.header == os.path.join(abi_util.INCLUDE, "locator_hip_local.h")
    src = re.sub(r"/\*.*?\*/", "", open(ext.header).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(loc_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(prototypes) == sorted(ext.prototypes) and ext.prototypes == prototypes
    assert ext.constants == {"LOC_LOCAL_MAX_CHANNELS": 64}
    assert all(getattr(_abi, k) == v for k, v in ext.constants.items())
    others = [o for table in (_abi.EXTENSIONS, _abi.LATER, _abi.OPEN) for t, o in table.items() if o is not ext]
    for consts, protos in [(_abi.CONSTANTS, _abi.PROTOTYPES)] + [(o.constants, o.prototypes) for o in others]:
        assert not set(names) & set(protos) and not set(ext.constants) & set(consts)
    lib = _lib.load()
    for name in names:
        fn = getattr(lib, name)
        assert _abi.ALL_PROTOTYPES[name] == prototypes[name]
        assert fn.restype is prototypes[name][0] and list(fn.argtypes) == prototypes[name][1]
    assert AN.MAX_CHANNELS == _abi.LOC_LOCAL_MAX_CHANNELS and AN.MAX_LABELS == 61


def _call(lib, H=12, K=5, R=3, pitch=16, theta=0.01, block=0, Cn=3, vpitch=12, W=2, work_bytes=None, null=(), off=None):
    """loc_paint_local on pointers that are never followed: every refusal here comes before the first use of the device."""
    ptr = {name: 0x100000 * (n + 1) for n, name in enumerate(("h", "donor", "owner", "rec", "rho", "v", "win", "out", "ll", "n_donors",
                                                              "work"))}
    for name in null:
        ptr[name] = None
    if off:
        ptr[off[0]] += off[1]
    need = int(lib.loc_paint_work_bytes(min(max(H, 1), PT.MAX_HAPS), max(K, 0), max(R, 0), max(block, 0)))
    return lib.loc_paint_local(ptr["h"], H, K, pitch, ptr["donor"], ptr["owner"], ptr["rec"], R, ptr["rho"], C.c_float(theta), block,
                               ptr["v"], Cn, vpitch, ptr["win"], W, ptr["out"], ptr["ll"], ptr["n_donors"], ptr["work"],
                               need if work_bytes is None else work_bytes, None)


def test_the_refusals_of_the_entry_point_that_need_no_device():
    from locator_amd import _lib
    lib = _lib.load()
    said = lambda: lib.loc_last_error().decode()
    for change, word in ((dict(H=0), "H="), (dict(H=PT.MAX_HAPS + 1, pitch=PT.MAX_HAPS + 16, vpitch=PT.MAX_HAPS + 4), "H="),
                         (dict(K=-1), "K="), (dict(K=2 ** 31), "K="), (dict(R=-1), "R="), (dict(block=-1), "block="),
                         (dict(H=20), "pitch >= H"), (dict(pitch=24), "multiple of 16"), (dict(work_bytes=-1), "work_bytes"),
                         (dict(theta=0.6), "theta"), (dict(theta=5e-8), "theta"), (dict(theta=float("nan")), "theta"),
                         (dict(K=0), "K=0"), (dict(Cn=0), "C=0"), (dict(Cn=65), "C=65"), (dict(W=0), "W=0"), (dict(W=6), "W=6"),
                         (dict(vpitch=8), "vpitch >= H"), (dict(vpitch=14), "multiple of 4"),
                         (dict(work_bytes=16), "needs"), (dict(null=("work",)), "needs"), (dict(off=("work", 4)), "16-byte aligned"),
                         (dict(off=("h", 4)), "multiples of 16"), (dict(off=("v", 4)), "v must be a multiple of 16"),
                         (dict(off=("win", 2)), "win of 4"),
                         *((dict(null=(name,)), "null buffer") for name in ("h", "donor", "owner", "rec", "rho", "v", "win", "out", "ll",
                                                                            "n_donors")),
                         *((dict(off=(name, 2)), "multiples of 4 bytes") for name in ("owner", "rec", "rho", "out", "n_donors")),
                         (dict(off=("ll", 4)), "ll of 8")):
        assert _call(lib, **change) == -1, change
        assert said().startswith("loc_paint_local: ") and word in said(), (change, said())
    assert _call(lib, R=0, null=("rec", "v", "win", "out", "ll", "work")) == 0    # nothing to do: nothing is looked at
    for change in (dict(theta=0.7), dict(Cn=65), dict(W=0), dict(vpitch=10), dict(K=0)):
        assert _call(lib, R=0, **change) == -1 and said().startswith("loc_paint_local: "), change   # ... but the sizes are


def test_refusals_of_the_definition():
    case = U.planted_case(8, 6, 1)
    v = np.ones((2, 8))
    ok = np.array([[0, 3], [3, 6]])
    assert AU.host(case, v, ok)[0].shape == (len(case["rec"]), 2, 2)
    for vv, win, text in ((v, [[0, 7]], "window 0"), (v, [[2, 2]], "window 0"), (v, [[0, 3], [2, 5]], "window 1"),
                          (v, [[3, 5], [0, 2]], "window 1"), (v, [[-1, 2]], "window 0"), (v, np.zeros((0, 2), dtype=int), "W >= 1"),
                          (v, [[0.0, 2.0]], "whole numbers"), (np.ones((2, 7)), ok, "attributes of shape"),
                          (np.ones((65, 8)), ok, "attributes of shape"), (np.ones((0, 8)), ok, "attributes of shape")):
        with pytest.raises(ValueError, match=text):
            AU.host(case, vv, np.asarray(win))
    with pytest.raises(ValueError, match="window 0"):
        AU.host({**case, "h": case["h"][:0], "rho": case["rho"][:0]}, v, np.array([[0, 1]]))     # K = 0 admits no window


# ------------------------------------------------------------------ local_host
@pytest.mark.parametrize("H,K", [(4, 1), (10, 7), (20, 37), (66, 29)])
def test_the_mass_channel_is_the_number_of_sites_and_the_windows_add_up_to_the_shares(H, K):
    for case in (U.planted_case(H, K, 100 * H + K), U.edge_case(H, K, 100 * H + K + 1, 0.01), U.edge_case(H, K, 7, 0.5)):
        v = AU.attributes(case, 5)
        share, _, ll, nd = U.host(case, np.float64)
        for name, win in AU.layouts(K).items():
            out, l, n = AU.host(case, v, win)
            assert out.shape == (len(case["rec"]), len(win), 64) and np.isfinite(out).all(), name
            assert np.array_equal(l, ll) and np.array_equal(n, nd)                      # the same forward pass
            n_sites = (win[:, 1] - win[:, 0])[None, :]
            assert np.abs(out[nd > 0, :, -1] - n_sites).max(initial=0) <= 1e-9, name    # no G underflows in these cases
            assert not out[nd == 0].any()
        # windows that tile all sites, one-hot channels of the first columns: their sum over the windows is share K
        eye = np.eye(H)[:min(H, 64)]
        for win in (AU.layouts(K)["each"], AU.layouts(K)["all"], np.array([[0, (K + 1) // 2], [(K + 1) // 2, K]][:2 if K > 1 else 1])):
            if K == 1:
                win = np.array([[0, 1]])
            out = AU.host(case, eye, win)[0]
            assert np.abs(out.sum(axis=1) - share[:, :len(eye)] * K).max() <= 1e-12


def test_no_result_depends_on_the_other_windows_or_channels_of_the_call():
    case = U.planted_case(20, 37, 3)
    v = AU.attributes(case, 1)
    win = AU.layouts(37)["fives"]
    whole = AU.host(case, v, win)[0]
    assert np.array_equal(AU.host(case, v, win[[1, 4]])[0], whole[:, [1, 4]])
    part = AU.host(case, v[[63, 2, 40]], win)[0]
    assert np.abs(part - whole[:, :, [63, 2, 40]]).max() <= 1e-12                       # a matrix product: the order of its sums may differ


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_a_spliced_recipient_is_localised_to_the_window(seed):
    """The recipient is one donor's alleles below K / 2 and a donor's of the other label above: in each of the ten 32-site
    windows the posterior of the true label is 0.8 at least (smallest seen: 0.914, the last window of seed 1)."""
    case, lab, (below, above) = AU.spliced(seed)
    v = np.array([np.where(lab == 0, 1.0, 0.0), np.where(lab == 1, 1.0, 0.0), np.ones(len(lab))])
    v[:, lab < 0] = np.nan
    win = np.array([[s, s + 32] for s in range(0, 320, 32)])
    out = AU.host(case, v, win)[0]
    post = out[0, :, :2] / out[0, :, 2:3]
    truth = np.array([below] * 5 + [above] * 5)
    print(f"seed {seed}: posterior of the true label by window {np.round(post[np.arange(10), truth], 3).tolist()}")
    assert (post[np.arange(10), truth] >= 0.8).all()
    d = AU.distance(AU.host(case, v, win, np.float32)[0], out, win)
    print(f"seed {seed}: float32 / float64 distance of the window means {d:.3g}")
    assert d <= 1e-5


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_planted_locations_and_labels_are_recovered(seed):
    """planted(40, 300, seed), everyone a donor: every sample's leave-one-out placement has r2 with x of 0.9 at least (seen 0.973
    .. 0.988) and the call of the two labels x >= 0.5 an accuracy of 0.9 at least (seen 0.95 .. 1.0)."""
    hap, x = U.planted(40, 300, seed)
    locs = np.stack([x, np.zeros(40)], axis=1)
    labels = np.array(["east" if a >= 0.5 else "west" for a in x], dtype=object)
    s = AN.ancestry(hap, [f"s{i}" for i in range(40)], None, None, locs, labels, None, window_snps=30, host=True, silence=True)
    r2 = PT.B.r2(s["_xy"][:, 0], x)
    print(f"seed {seed}: r2 with x {r2:.4f}, accuracy of the call {s['label_accuracy']:.3f}")
    assert r2 >= 0.9 and s["label_accuracy"] >= 0.9 and s["W"] == 10 and s["channels"] == ["label:east", "label:west", "x", "y", "mass"]


# ------------------------------------------------------------------ the command
def _labels_file(path, ids, labels):
    with open(path, "w") as fh:
        fh.write("sampleID\tlabel\n" + "".join(f"{s}\t{lab}\n" for s, lab in zip(ids, labels)))
    return path


def _cut_ids(vcf):
    with open(vcf) as fh:
        for line in fh:
            if line.startswith("#CHROM"):
                return line.rstrip("\n").split("\t")[9:]


def test_the_host_command_on_a_cut_of_the_golden_vcf(tmp_path):
    import pandas as pd
    from locator_amd import plot as PL
    vcf = U.write_vcf_cut(str(tmp_path / "cut.vcf"), 40, 30, 240)                      # 10 samples without a location, 20 with
    ids = _cut_ids(vcf)
    truth = pd.read_csv(U.SAMPLE_DATA, sep="\t").set_index("sampleID").reindex(ids)
    lab = ["NA" if np.isnan(x) else ("east" if x >= np.nanmedian(truth["x"]) else "west") for x in truth["x"]]
    labels = _labels_file(str(tmp_path / "labels.txt"), ids, lab)
    runs = []
    for name in ("a", "b"):
        out = str(tmp_path / name / "o")
        os.makedirs(os.path.dirname(out))
        assert AN.main(["--vcf", vcf, "--out", out, "--sample_data", U.SAMPLE_DATA, "--labels", labels, "--window_snps", "50",
                        "--em_rounds", "1", "--host", "--silence", "--keep_windows"]) == 0
        runs.append(out)
    out = runs[0]
    s = json.load(open(out + "_ancestry_summary.json"))
    N, W = 30, s["W"]
    assert (s["path"], s["N"], s["H"], s["n_donor_haps"], s["C"], s["groups"]) == ("host", N, 2 * N, 40, 5, 1)
    assert s["channels"] == ["label:east", "label:west", "x", "y", "mass"] and s["n_located"] == 20 and s["n_labelled"] == 20
    assert s["K"] <= 240 and W == -(-s["K"] // 50) and 0 <= s["label_accuracy"] <= 1 and s["median_error"] > 0
    table = pd.read_csv(out + "_ancestry_windows.txt", sep="\t")
    assert list(table.columns) == ["chrom", "start", "stop", "first_site", "n_sites"] and len(table) == W
    assert table["n_sites"].sum() == s["K"] and (table["first_site"].to_numpy() == 50 * np.arange(W)).all()
    store = G.open_group(out + "_ancestry.zarr", mode="r")
    mass, local = np.asarray(store["mass"][:]), np.asarray(store["local"][:])
    assert mass.shape == (W, 2 * N) and local.shape == (W, 2 * N, 4) and mass.dtype == local.dtype == np.float32
    assert [str(x) for x in store["samples"][:]] == ids and [str(x) for x in store["channels"][:]] == s["channels"]
    assert np.array_equal(np.asarray(store["windows/n_sites"][:]), table["n_sites"].to_numpy())
    assert np.abs(mass - 1).max() <= 1e-5 and np.isfinite(local).all()
    assert np.abs(local[:, :, :2].sum(axis=2) - 1).max() <= 1e-5                       # the labels' posteriors: every donor has one
    q = pd.read_csv(out + "_ancestry_Q.txt", sep="\t", keep_default_na=False)
    assert list(q.columns) == ["sampleID", "east", "west", "label", "call"] and list(q["sampleID"]) == ids and list(q["label"]) == lab
    assert np.abs(q["east"] + q["west"] - 1).max() <= 1e-6 and set(q["call"]) <= {"east", "west"}
    locs = pd.read_csv(out + "_ancestry_locs.txt")
    assert list(locs.columns) == ["x", "y", "sampleID"] and list(locs["sampleID"]) == ids and np.isfinite(locs[["x", "y"]].to_numpy()).all()
    folder = out + "_ancestry_windows"
    files = sorted(os.listdir(folder))
    assert files == sorted(f"{c}_{a}-{b}_predlocs.txt" for c, a, b in zip(table["chrom"], table["start"], table["stop"]))
    aeg = PL.load_predlocs(folder)
    assert len(aeg) == W * N and set(aeg["sampleID"]) == set(ids) and list(aeg.columns) == ["xpred", "ypred", "sampleID"]
    # a sample's location is the site-weighted mean of its windows' (each the mean of its two haplotypes' posterior means)
    per = aeg.groupby("sampleID")[["xpred", "ypred"]]
    first = aeg[aeg["sampleID"] == ids[0]][["xpred", "ypred"]].to_numpy()
    names = [f"{c}_{a}-{b}_predlocs.txt" for c, a, b in zip(table["chrom"], table["start"], table["stop"])]
    in_file_order = table["n_sites"].to_numpy()[np.argsort(names)]                     # load_predlocs reads in name order
    wanted = (first * in_file_order[:, None]).sum(axis=0) / s["K"]
    assert per.ngroups == N and np.abs(wanted - locs[["x", "y"]].to_numpy()[0]).max() <= 1e-6 * (1 + np.abs(wanted).max())
    hist = np.loadtxt(out + "_ancestry_history.txt", skiprows=1, ndmin=2)
    assert hist.shape == (1, 3)
    # determinism: the two runs wrote the same bytes
    for tail in ("_ancestry_summary.json", "_ancestry_windows.txt", "_ancestry_Q.txt", "_ancestry_locs.txt", "_ancestry_history.txt",
                 "_ancestry.zarr/local/0.0.0", "_ancestry.zarr/mass/0.0", "_ancestry_windows/" + files[-1]):
        assert open(runs[0] + tail, "rb").read() == open(runs[1] + tail, "rb").read(), tail


def test_the_refusals_of_the_command(tmp_path):
    vcf = U.write_vcf_cut(str(tmp_path / "cut.vcf"), 40, 30, 60)
    ids = _cut_ids(vcf)
    base = ["--vcf", vcf, "--out", str(tmp_path / "o"), "--host", "--silence", "--em_rounds", "0"]
    run = lambda *more: AN.main(base + list(more))
    with pytest.raises(SystemExit, match="without phase"):
        AN.main(["--vcf", U.write_vcf_cut(str(tmp_path / "unphased.vcf"), 40, 30, 60, unphase=[(3, 2)]), *base[2:], "--sample_data",
                 U.SAMPLE_DATA, "--window_snps", "20"])
    with pytest.raises(SystemExit, match="would overlap"):
        run("--sample_data", U.SAMPLE_DATA, "--window_snps", "20", "--window_step", "10")
    with pytest.raises(SystemExit, match="62 labels"):
        many = [f"g{n:02d}" for n in range(30)] + [f"h{n:02d}" for n in range(32)]
        big = U.write_vcf_cut(str(tmp_path / "big.vcf"), 40, 62, 20)
        run("--vcf", big, "--labels", _labels_file(str(tmp_path / "many.txt"), _cut_ids(big), many), "--window_snps", "10")
    with pytest.raises(SystemExit):                                                  # no attribute given (argparse's error)
        run("--window_snps", "20")
    with pytest.raises(SystemExit, match="needs --sample_data"):
        hap, _ = U.planted(4, 10, 1)
        AN.ancestry(hap, list("abcd"), None, None, None, None, None, window_snps=5, host=True)
    with pytest.raises(SystemExit, match="there is no donor"):
        run("--labels", _labels_file(str(tmp_path / "none.txt"), ids, ["NA"] * len(ids)), "--window_snps", "20")
    with pytest.raises(SystemExit, match="there is no donor"):                       # located and labelled samples do not meet
        run("--sample_data", U.SAMPLE_DATA, "--labels", _labels_file(str(tmp_path / "first.txt"), ids, ["a"] * 10 + ["NA"] * 20),
            "--window_snps", "20")
    with pytest.raises(SystemExit):
        run("--sample_data", U.SAMPLE_DATA)                                          # no window size
    assert not [f for f in os.listdir(tmp_path) if f.startswith("o_")]
