"""The phase command without a GPU: the binding and the refusals that need no device, the NumPy definition on small exact cases
(copies of two donors, untouched calls, no donor, no linkage, ties), ll against the path's probability, the switch error on
planted data and on a cut of the golden VCF, the --host command."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from locator_amd import impute as IM
from locator_amd import phase as PH
from tests import phase_util as U


# ------------------------------------------------------------------ the binding
def test_phase_header_is_bound_as_the_other_headers_are():
    """What tests.abi_util.check_extension asserts of a line of _abi's first table, here of the line in its second table."""
    import re
    from locator_amd import _abi, _lib
    from tests import abi_util
    vp, i64, i, f = C.c_void_p, C.c_int64, C.c_int, C.c_float
    prototypes = {"loc_phase_work_bytes": (i64, [i, i64, i, i]),
                  "loc_phase_viterbi": (i, [vp, i, i64, i64, vp, i, vp, i, vp, f, i, vp, i64, vp, vp, vp, vp, vp, i64, vp])}
    assert list(_abi.EXTENSIONS) == list(abi_util.HEADERS) and list(_abi.LATER) == ["phase"]
    ext = _abi.LATER["phase"]
    assert ext.header == os.path.join(abi_util.INCLUDE, "locator_hip_phase.h")
    src = re.sub(r"/\*.*?\*/", "", open(ext.header).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(loc_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(prototypes) == sorted(ext.prototypes) and ext.prototypes == prototypes
    assert ext.constants == {"LOC_PHASE_MAX_STATES": 64, "LOC_PHASE_MIN_STATES": 2}
    assert all(getattr(_abi, k) == v for k, v in ext.constants.items())
    for consts, protos in [(_abi.CONSTANTS, _abi.PROTOTYPES)] + [(o.constants, o.prototypes) for o in _abi.EXTENSIONS.values()]:
        assert not set(names) & set(protos) and not set(ext.constants) & set(consts)
    lib = _lib.load()
    for name in names:
        fn = getattr(lib, name)
        assert _abi.ALL_PROTOTYPES[name] == prototypes[name]
        assert fn.restype is prototypes[name][0] and list(fn.argtypes) == prototypes[name][1]
    assert (PH.MAX_STATES, PH.MIN_STATES) == (_abi.LOC_PHASE_MAX_STATES, _abi.LOC_PHASE_MIN_STATES)


def _call(lib, H=12, K=5, R=3, S=4, pitch=16, theta=0.01, block=0, first_pitch=8, work_bytes=None, null=(), off=None):
    """loc_phase_viterbi on pointers that are never followed: every refusal here comes before the first use of the device."""
    ptr = {name: 0x100000 * (n + 1) for n, name in enumerate(("h", "rec", "don", "rho", "first", "ll", "n_switch", "n_tied", "n_donors",
                                                              "work"))}
    for name in null:
        ptr[name] = None
    if off:
        ptr[off[0]] += off[1]
    need = int(lib.loc_phase_work_bytes(min(max(S, 2), 64), max(K, 0), max(R, 0), max(block, 0)))
    return lib.loc_phase_viterbi(ptr["h"], H, K, pitch, ptr["rec"], R, ptr["don"], S, ptr["rho"], C.c_float(theta), block, ptr["first"],
                                 first_pitch, ptr["ll"], ptr["n_switch"], ptr["n_tied"], ptr["n_donors"], ptr["work"],
                                 need if work_bytes is None else work_bytes, None)


def test_the_refusals_of_the_entry_points_that_need_no_device():
    from locator_amd import _lib
    lib = _lib.load()
    said = lambda: lib.loc_last_error().decode()
    for change, word in ((dict(S=1), "S="), (dict(S=65), "S="), (dict(K=-1), "K="), (dict(K=2 ** 31), "K="), (dict(R=-1), "R="),
                         (dict(block=-1), "block="), (dict(H=11), "H even"), (dict(H=0), "H even"), (dict(H=32), "pitch >= H"),
                         (dict(pitch=24), "multiple of 16"), (dict(first_pitch=4), "first_pitch >= K"), (dict(work_bytes=-1), "work_bytes"),
                         (dict(theta=0.6), "theta"), (dict(theta=5e-8), "theta"), (dict(theta=float("nan")), "theta"),
                         (dict(work_bytes=16), "needs"), (dict(null=("work",)), "needs"), (dict(off=("work", 4)), "16-byte aligned"),
                         (dict(off=("h", 4)), "multiples of 16"),
                         *((dict(null=(name,)), "null buffer") for name in ("h", "rec", "don", "rho", "first", "ll", "n_switch", "n_tied",
                                                                            "n_donors")),
                         *((dict(off=(name, 2)), "multiples of 4 bytes") for name in ("rec", "don", "rho", "n_switch", "n_tied", "n_donors")),
                         (dict(off=("ll", 4)), "ll of 8")):
        assert _call(lib, **change) == -1, change
        assert said().startswith("loc_phase_viterbi: ") and word in said(), (change, said())
    assert _call(lib, R=0, null=("rec", "don", "first", "ll", "work")) == 0      # nothing to do: nothing is looked at
    assert _call(lib, R=0, theta=0.7) == -1                                      # ... but the sizes and theta are
    for S, K, R, block in ((1, 5, 1, 0), (65, 5, 1, 0), (8, -1, 1, 0), (8, 5, -1, 0), (8, 5, 1, -1), (8, 2 ** 31, 1, 0)):
        assert lib.loc_phase_work_bytes(S, K, R, block) == -1 and said().startswith("loc_phase_work_bytes: ")
    assert lib.loc_phase_work_bytes(8, 5, 0, 0) == 0 and lib.loc_phase_work_bytes(8, 0, 3, 0) == 0
    assert lib.loc_phase_work_bytes(64, 50, 2, 25) == 2 * (64 * 64 * 4 + 25 * 64 * 5 * 4)


def test_refusals_of_the_definition():
    case = U.planted_case(4, 5, 1)
    s = int(case["rec"][0])
    own = case["don"].copy()
    own[0, 1] = 2 * s + 1
    for change, text in (({"theta": 0.6}, "theta"), ({"theta": 1e-8}, "theta"), ({"rec": np.full(len(case["rec"]), 99)}, "recipient"),
                         ({"rho": np.full(5, 1.5)}, "switch probability"), ({"rho": np.zeros(4)}, "switch probabilities"),
                         ({"h": case["h"].astype(np.int16)}, "int8"), ({"h": case["h"] + np.int8(1)}, "alleles 0 and 1"),
                         ({"don": case["don"][:2]}, "donors of shape"), ({"don": case["don"][:, :1]}, "donors of shape"),
                         ({"don": np.full_like(case["don"], 99)}, "outside the columns"), ({"don": own}, "column of its recipient"),
                         ({"don": np.full_like(case["don"], -2)}, "outside the columns")):
        with pytest.raises(ValueError, match=text):
            U.host({**case, **change})


# ------------------------------------------------------------------ viterbi_host on exact cases
def _copies(K=60, seed=3, theta=0.001):
    """Sample 0 copies the columns 2 and 5 exactly; samples 1 .. 3 are random.  Sample 0 has missing calls, and its heterozygous
    calls are shuffled.  Returns (case, truth of sample 0: [K][2])."""
    rng = np.random.default_rng(seed)
    hap = rng.integers(0, 2, (K, 8)).astype(np.int8)
    hap[:, 0], hap[:, 1] = hap[:, 2], hap[:, 5]
    hap[rng.random(K) < 0.1, 0:2] = -1
    truth = hap[:, :2].copy()
    hap = np.concatenate([U.shuffled(hap[:, :2], seed + 1), hap[:, 2:]], axis=1)
    don = np.array([[2, 3, 4, 5, 6, 7], [-1] * 6], dtype=np.int32)
    return {"h": hap, "rec": np.array([0, 1], dtype=np.int32), "don": don, "rho": np.full(K, 0.01), "theta": theta}, truth


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_copies_of_two_donors_are_phased_as_the_donors_are(dtype):
    case, truth = _copies()
    first, ll, n_switch, n_tied, n_donors = U.host(case, dtype)
    h = case["h"]
    het = (truth[:, 0] >= 0) & (truth[:, 0] != truth[:, 1])
    assert het.sum() > 15
    assert np.array_equal(first[0][het], truth[het, 0]) or np.array_equal(first[0][het], truth[het, 1])      # up to the labels
    assert np.array_equal(first[0][~het], h[~het, 0])                            # homozygous and missing calls stay
    assert n_switch[0] == 0 and n_tied[0] == 0 and ll[0] < 0 and n_donors[0] == 6
    assert np.array_equal(first[1], h[:, 2]) and ll[1] == 0 and n_donors[1] == 0 and n_switch[1] == 0          # nobody to copy from
    assert first.dtype == np.int8 and ll.dtype == np.float64 and n_switch.dtype == n_tied.dtype == n_donors.dtype == np.int32


def test_without_linkage_a_het_call_follows_the_best_pair_of_its_site_or_stays_on_a_tie():
    """rho = 1 everywhere (the module text): the path is a best state of every site on its own.  Donors (1, 0) put allele 1 on
    the first copy whatever the input's order was; where both donors hold the same allele the two products tie and the call stays."""
    K = 12
    hap = np.zeros((K, 6), dtype=np.int8)
    hap[:, 2], hap[:, 3] = 1, 0                                                  # sample 1: the donors
    hap[:, 0], hap[:, 1] = np.arange(K) % 2, 1 - np.arange(K) % 2                # sample 0: het everywhere, alternating order
    hap[:, 4], hap[:, 5] = hap[:, 1], hap[:, 0]                                  # sample 2 likewise
    case = {"h": hap, "rec": np.array([0, 2], dtype=np.int32), "don": np.array([[2, 3], [3, 3]], dtype=np.int32), "rho": np.ones(K),
            "theta": 0.01}
    paths = []
    first, ll, n_switch, n_tied, _ = U.host(case, paths=paths)
    assert (first[0] == 1).all() and n_tied[0] == 0 and n_switch[0] == 0         # the state (0, 1) = donors (1, 0), the lowest of the best
    assert np.array_equal(first[1], hap[:, 4]) and n_tied[1] == K                # donors (0, 0): a tie at every site
    _, d1, d2, _ = paths[0]
    assert (d1[0] == 0).all() and (d2[0] == 1).all()


def test_repeated_donor_columns_tie_exactly_and_the_lowest_index_is_taken():
    K = 30
    rng = np.random.default_rng(8)
    hap = rng.integers(0, 2, (K, 6)).astype(np.int8)
    hap[:, 0], hap[:, 1] = hap[:, 2], hap[:, 4]                                  # sample 0 = (column 2, column 4)
    case = {"h": hap, "rec": np.array([0], dtype=np.int32), "don": np.array([[2, 2, 4, 4, 3, 5]], dtype=np.int32),
            "rho": np.full(K, 0.02), "theta": 0.01}
    paths = []
    first, ll, n_switch, n_tied, _ = U.host(case, paths=paths)
    _, d1, d2, code = paths[0]
    # the pairs (0|1, 2|3) and their mirrors all hold the same value; the end state is the lowest flat index, and staying is preferred
    assert (d1[0] == 0).all() and (d2[0] == 2).all() and not code[0].any() and n_switch[0] == 0
    assert np.array_equal(first[0], hap[:, 2])
    # ... mirrored donors give the mirrored labels
    case["don"] = np.array([[4, 4, 2, 2, 3, 5]], dtype=np.int32)
    assert np.array_equal(U.host(case)[0][0], np.where(hap[:, 0] != hap[:, 1], hap[:, 4], hap[:, 0]))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_ll_is_the_log_probability_of_the_returned_path(dtype):
    K = 60
    case = U.planted_case(8, K, 6)
    case["theta"] = 2.0 ** -7                                                    # the same number in both types
    paths = []
    first, ll, n_switch, n_tied, n_donors = U.host(case, dtype, paths=paths)
    rows, d1, d2, code = paths[0]
    # a site's factor passes through about ten roundings of the type (the table, tt, the products, the normalisation)
    bound = K * 10 * float(np.finfo(dtype).eps)
    worst = 0.0
    for n, i in enumerate(rows):
        want = U.path_log_probability(case, i, d1[n], d2[n], code[n])
        worst = max(worst, abs(ll[i] - want))
        assert n_switch[i] == int((code[n] == 3).sum() * 2 + ((code[n] == 1) | (code[n] == 2)).sum())
    print(f"ll against the path's log probability, {np.dtype(dtype).name}: largest difference {worst:.3g}, bound {bound:.3g}")
    assert worst <= bound and n_switch.sum() > 0


def test_the_emission_table_is_symmetric_bit_for_bit():
    for theta in (1e-7, 0.01, 0.3, 0.5):
        for dtype in (np.float32, np.float64):
            E = PH.emission_table(theta, dtype)
            assert E.dtype == dtype and np.array_equal(E, E.transpose(0, 2, 1)) and (E[3] == 1).all()
    case = U.edge_case(6, 9, 2, 0.3)


def test_switch_error():
    truth = np.array([[0, 1], [1, 0], [0, 1], [1, 1], [0, 1], [-1, 1]], dtype=np.int8)
    assert PH.switch_error(truth, truth) == 0 and PH.switch_error(truth[:, ::-1], truth) == 0        # the labels do not count
    est = truth.copy()
    est[2] = est[2, ::-1]
    assert PH.switch_error(est, truth) == 2 / 3                                  # four het calls, three pairs, the third call turned
    assert np.isnan(PH.switch_error(truth[3:4], truth[3:4]))


# ------------------------------------------------------------------ quality
def _gt(hap):
    return np.ascontiguousarray(hap.reshape(hap.shape[0], -1, 2))


def test_the_switch_error_on_planted_data_falls_below_half_its_start():
    hap, _ = U.planted(40, 300, seed=2, stay=0.99)
    s = PH.phase(_gt(hap), [f"s{i}" for i in range(40)], {"chrom": None, "pos": None}, states=32, rounds=8, switch=0.01, theta=0.01,
                 uniform=True, check=True, host=True, silence=True, init_seed=0)
    print(f"planted 40 x 300, 32 states, 8 rounds: switch error {s['switch_error_start']:.4f} at the start, by round "
          + " ".join(f"{r[4]:.4f}" for r in s["_history"]))
    assert 0.4 < s["switch_error_start"] < 0.6 and s["switch_error"] < 0.5 * s["switch_error_start"]


def test_the_switch_error_on_a_cut_of_the_golden_vcf_falls_below_half_its_start(tmp_path):
    vcf = U.write_vcf_cut(str(tmp_path / "cut.vcf"), 0, 60, 600)
    out = str(tmp_path / "o")
    assert PH.main(["--vcf", vcf, "--out", out, "--host", "--states", "32", "--rounds", "3", "--check", "--silence"]) == 0
    s = json.load(open(out + "_phase_summary.json"))
    lines = open(out + "_phase_history.txt").read().splitlines()
    print(f"golden VCF, 60 samples x {s['K']} sites, 32 states: switch error {s['switch_error_start']:.4f} at the start, by round "
          + " ".join(f"{float(line.split()[4]):.4f}" for line in lines[1:]))
    assert lines[0].split("\t") == ["round", "ll", "switches_per_site", "changed", "switch_error"] and len(lines) == 4
    assert 0.4 < s["switch_error_start"] < 0.6 and s["switch_error"] < 0.5 * s["switch_error_start"]
    assert s["path"] == "host" and s["het_calls"] > s["het_undecided"] >= 0 and s["N"] == 60 and s["states"] == 32


# ------------------------------------------------------------------ the command
def test_the_host_command_twice_writes_the_same_bytes_and_impute_reads_the_store(tmp_path):
    vcf = U.write_vcf_cut(str(tmp_path / "cut.vcf"), 40, 30, 200, unphase=((3, 2), (7, 5)))
    with pytest.raises(SystemExit, match="without phase"):                       # what the phase command is for
        IM.read_phased(vcf, False)
    outs = []
    for name in ("a", "b"):
        out = str(tmp_path / name / "o")
        os.makedirs(os.path.dirname(out))
        assert PH.main(["--vcf", vcf, "--out", out, "--host", "--states", "8", "--rounds", "2", "--silence"]) == 0
        outs.append(out)
    assert U.tree_bytes(os.path.dirname(outs[0])) == U.tree_bytes(os.path.dirname(outs[1]))
    assert sorted(os.listdir(os.path.dirname(outs[0]))) == ["o_phase_history.txt", "o_phase_summary.json", "o_phased.zarr"]
    d = IM.read_phased(outs[0] + "_phased.zarr", True)
    raw = IM.read_phased(vcf, False, refuse=False)
    assert raw.pop("unphased_hets") == 2
    raw, dropped = IM.biallelic(raw)
    assert d["gt"].shape == raw["gt"].shape and np.array_equal(np.sort(d["gt"], axis=2), np.sort(raw["gt"], axis=2))       # the same calls
    assert all(np.array_equal(d[k], raw[k]) for k in ("samples", "chrom", "pos", "ref", "alt"))
    s = json.load(open(outs[0] + "_phase_summary.json"))
    assert s["multiallelic_dropped"] == dropped and s["K"] == len(raw["pos"]) and s["switch_error"] is None and s["rounds_run"] == 2
    with pytest.raises(SystemExit, match="--check needs"):
        PH.main(["--vcf", vcf, "--out", outs[0], "--host", "--check", "--silence"])
    # a store goes in as a VCF does, and --init keep on the phased store changes less than a fresh draw
    again = str(tmp_path / "again")
    assert PH.main(["--zarr", outs[0] + "_phased.zarr", "--out", again, "--host", "--states", "8", "--rounds", "1", "--init", "keep",
                    "--silence"]) == 0
    assert json.load(open(again + "_phase_summary.json"))["init"] == "keep"


def test_refusals_of_the_command(tmp_path, monkeypatch):
    import torch
    out = str(tmp_path / "o")
    vcf = U.write_vcf_cut(str(tmp_path / "cut.vcf"), 40, 6, 30)
    for argv, text in ((["--matrix", "m.txt"], "carries no|has no CHROM"), ):
        with pytest.raises(SystemExit, match=text):
            PH.main(argv + ["--out", out, "--host"])
    for argv in (["--out", out], ["--vcf", vcf, "--zarr", vcf, "--out", out], ["--vcf", vcf, "--out", out, "--states", "7"],
                 ["--vcf", vcf, "--out", out, "--states", "66"], ["--vcf", vcf, "--out", out, "--states", "0"],
                 ["--vcf", vcf, "--out", out, "--rounds", "0"], ["--vcf", vcf, "--out", out, "--budget_gb", "0"],
                 ["--vcf", vcf, "--out", out, "--init", "other"]):
        with pytest.raises(SystemExit) as e:
            PH.main(argv + ["--host"])
        assert e.value.code == 2, argv
    for argv, text in ((["--theta", "0.7"], "--theta"), (["--switch", "0"], "--switch"), (["--switch", "nan"], "--switch")):
        with pytest.raises(SystemExit, match=text):
            PH.main(["--vcf", vcf, "--out", out, "--host", "--silence"] + argv)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match="no GPU visible .*pass --host"):
        PH.main(["--vcf", vcf, "--out", out])
    gt = np.zeros((4, 1, 2), dtype=np.int8)
    sites = {"chrom": None, "pos": None}
    with pytest.raises(SystemExit, match="nobody to copy from"):
        PH.phase(gt, ["a"], sites, host=True)
    with pytest.raises(SystemExit, match="nothing to phase"):
        PH.phase(np.zeros((0, 3, 2), dtype=np.int8), ["a", "b", "c"], sites, host=True)
    with pytest.raises(SystemExit, match="ploidy"):
        PH.phase(np.zeros((4, 3, 1), dtype=np.int8), ["a", "b", "c"], sites, host=True)
    assert not os.path.exists(out + "_phase_summary.json")
