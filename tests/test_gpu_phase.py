"""The phase command on the device (locator_amd/csrc/phase_kernels.hip).

loc_phase_viterbi against phase.viterbi_host(float32): first, n_switch, n_tied and n_donors bit for bit, ll within
1e-9 (1 + |ll|) (the m_j are the same floats; only the float64 logarithms are grouped and summed differently).  State counts around
the three instantiations (16, 32, 64 slots), site counts around the checkpoint blocks, every block size, planted and edge inputs
(missing alleles, an all-missing site, rho of 0, 1 and tiny values, theta at both ends, -1-padded and repeated donors, a recipient
with no donor).  No result depends on the block size, on what scratch and outputs held, on appended or permuted recipients or on the
batches; the pad bytes of `first` and a guard band behind the scratch stay untouched; bad arguments launch nothing.  The command on
the device writes the bytes of --host, and paint accepts the store."""
import ctypes as C
import os

import numpy as np
import pytest

from locator_amd import phase as PH
from tests import phase_util as U

pytestmark = pytest.mark.gpu
QNAN = 0x7fc00000
GUARD = 1024


def same(got, want):
    """first, n_switch, n_tied, n_donors equal; ll within the bound of the module text."""
    assert got[0].dtype == np.int8 and got[0].shape == want[0].shape
    exact = all(np.array_equal(got[i], want[i]) for i in (0, 2, 3, 4))
    return exact and bool((np.abs(got[1] - want[1]) <= 1e-9 * (1 + np.abs(want[1]))).all())


def same_bits(a, b):
    return all(np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)) for x, y in zip(a, b))


def cases(S, K):
    yield "planted", U.planted_case(S, K, 100 * S + K)
    for theta in (1e-7, 0.5):
        yield f"edge theta={theta}", U.edge_case(S, K, 100 * S + K + 1, theta)


# ------------------------------------------------------------------ loc_phase_viterbi
@pytest.mark.parametrize("K", [1, 2, 7, 33, 64, 65, 200])
@pytest.mark.parametrize("S", [2, 4, 30, 62, 64])
def test_viterbi_is_the_float32_definition_at_every_block(S, K):
    fills = np.random.default_rng(S + K)
    for name, case in cases(S, K):
        want = U.host(case)
        if name != "planted":
            assert (want[4] == 0).any() and (want[4] == S).any() and (want[4] == S // 2).any()     # no donor, all slots, half
        first = None
        for n, block in enumerate((0, 1, 2, 7, K)):
            report = {}
            got = U.device(case, block=block, fill=QNAN if n % 2 else 0x5a5a5a5a, pad_fill=fills if n % 2 else 0x55,
                           pitch=(case["h"].shape[1] + 15) // 16 * 16 + 16 * (n % 3), first_pitch=K + 5 * (n % 2), guard=GUARD,
                           report=report)
            assert same(got, want), (name, block, [int((got[i] != want[i]).sum()) for i in (0, 2, 3, 4)], got[1] - want[1])
            assert report == {"pad_untouched": True, "guard_untouched": True}, (name, block, report)
            first = got if first is None else first
            assert same_bits(got, first), (name, block)


def test_the_same_bits_whatever_scratch_held_and_however_the_recipients_are_batched():
    S, K = 30, 37
    case = U.planted_case(S, K, 3)
    first = U.device(case, block=1)
    assert same(first, U.host(case))
    for block in (1, 5, 0, K):
        for pattern in (None, QNAN, 0xffffffff, 0x7f800001):
            assert same_bits(U.device(case, block=block, fill=pattern, pad_fill=np.random.default_rng(block)), first), (block, pattern)
    n = len(case["rec"])
    more = dict(case)                                                             # appended recipients
    more["rec"] = np.concatenate([case["rec"], case["rec"][:2]])
    more["don"] = np.concatenate([case["don"], case["don"][:2]])
    got = U.device(more, block=3)
    assert same_bits([v[:n] for v in got], first) and same_bits([v[n:] for v in got], [v[:2] for v in first])
    order = np.random.default_rng(1).permutation(n)                               # a permuted rec
    mixed = dict(case)
    mixed["rec"], mixed["don"] = case["rec"][order], case["don"][order]
    assert same_bits(U.device(mixed, block=4), [v[order] for v in first])
    cut = n // 3                                                                  # two launches, and the batches of a small budget
    a, b = dict(case), dict(case)
    a["rec"], a["don"], b["rec"], b["don"] = case["rec"][:cut], case["don"][:cut], case["rec"][cut:], case["don"][cut:]
    assert same_bits([np.concatenate(p) for p in zip(U.device(a, block=2), U.device(b, block=7))], first)
    assert same_bits(U.device(case, budget=1), first)
    one = PH.viterbi_device(case["h"], case["rec"], case["don"], case["rho"], case["theta"],
                            budget=2 * (int(K) + _work_bytes(S, K, 1)) + 1)
    assert same_bits(one, first)


def _work_bytes(S, K, R, block=0):
    from locator_amd import _lib
    return int(_lib.load().loc_phase_work_bytes(S, K, R, block))


def test_a_long_stretch_without_a_switch_and_denormal_rates():
    """rho = 0 lets every state but the best underflow to exact zeros; rho = 1e-20 makes ru ru a float32 denormal or zero and
    t ru a small normal number: the device keeps denormals as NumPy does."""
    S, K = 8, 120
    case = U.planted_case(S, K, 5)
    for rho in (0.0, 1e-20, 1e-22):
        case["rho"] = np.full(K, rho)
        got = U.device(case, fill=QNAN)
        assert same(got, U.host(case)), rho
        assert same_bits(U.device(case, block=1), got) and same_bits(U.device(case, block=K), got)


def _raw(lib, t, H=12, K=5, R=3, S=4, pitch=16, theta=0.01, block=0, rec=None, don=None, work_bytes=None, first_pitch=None,
         pattern=0x5a5a5a5a, null=None, off=None):
    """One direct call on buffers filled with a pattern: (return code, the outputs as int32 views).  null: the name of a buffer
    passed as a null pointer; off: (name, bytes) a buffer passed off its start."""
    dev = "cuda:0"
    fp = max(K, 1) if first_pitch is None else first_pitch
    bufs = {"h": t.zeros((max(K, 1), max(pitch, 16)), dtype=t.int8, device=dev),
            "rec": t.tensor(list(range(max(R, 1))) if rec is None else rec, dtype=t.int32, device=dev),
            "don": t.tensor([[(2 * r + 2 + d) % 12 for d in range(max(S, 1))] for r in range(max(R, 1))] if don is None else don,
                            dtype=t.int32, device=dev),
            "rho": t.full((max(K, 1) + 1,), 0.1, dtype=t.float32, device=dev)}
    outs = {"first": t.empty((max(R, 1) * max(fp, 1) + 7) // 4, dtype=t.int32, device=dev),
            "ll": t.empty(2 * max(R, 1) + 1, dtype=t.int32, device=dev)}
    for name in ("n_switch", "n_tied", "n_donors"):
        outs[name] = t.empty(max(R, 1) + 1, dtype=t.int32, device=dev)
    for o in outs.values():
        o.fill_(int(np.array(pattern, dtype=np.uint32).view(np.int32)))
    need = int(lib.loc_phase_work_bytes(min(max(S, 2), 64), max(K, 0), max(R, 0), max(block, 0)))
    bufs["work"] = t.empty(max(need // 4, 4) + 4, dtype=t.float32, device=dev)
    ptr = {**{k: v.data_ptr() for k, v in bufs.items()}, **{k: v.data_ptr() for k, v in outs.items()}}
    if null:
        ptr[null] = None
    if off:
        ptr[off[0]] += off[1]
    rc = lib.loc_phase_viterbi(ptr["h"], H, K, pitch, ptr["rec"], R, ptr["don"], S, ptr["rho"], C.c_float(theta), block, ptr["first"], fp,
                               ptr["ll"], ptr["n_switch"], ptr["n_tied"], ptr["n_donors"], ptr["work"],
                               need if work_bytes is None else work_bytes, t.cuda.current_stream().cuda_stream)
    t.cuda.synchronize()
    return rc, [o.cpu().numpy() for o in outs.values()]


BAD = [dict(S=1), dict(S=65), dict(K=-1), dict(R=-1), dict(block=-1), dict(H=11), dict(H=0), dict(H=32), dict(pitch=24), dict(pitch=0),
       dict(first_pitch=4), dict(theta=0.6), dict(theta=5e-8), dict(theta=float("nan")), dict(work_bytes=16), dict(work_bytes=-1),
       dict(rec=[0, 6, 1]), dict(rec=[-1, 0, 1]), dict(don=[[2, 3, 4, 5], [0, 1, 12, 5], [0, 1, 2, 3]]),
       dict(don=[[2, 3, 4, 5], [0, 1, -2, 5], [0, 1, 2, 3]]), dict(don=[[2, 3, 4, 5], [0, 1, 4, 5], [0, 1, 2, 5]]),
       dict(don=[[2, 3, 4, 0], [0, 1, 4, 5], [0, 1, 2, 3]]),
       *(dict(null=name) for name in ("h", "rec", "don", "rho", "first", "ll", "n_switch", "n_tied", "n_donors", "work")),
       *(dict(off=(name, by)) for name, by in (("h", 4), ("rec", 2), ("don", 2), ("rho", 2), ("ll", 4), ("n_switch", 2), ("n_tied", 2),
                                               ("n_donors", 2), ("work", 4)))]


def test_bad_arguments_launch_nothing_and_empty_inputs_are_as_specified():
    import torch as t
    from locator_amd import _lib
    lib = _lib.load()
    pat = np.array(0x5a5a5a5a, dtype=np.uint32).view(np.int32)
    rc, outs = _raw(lib, t)
    assert rc == 0 and not any((o == pat).all() for o in outs)
    for change in BAD:
        rc, outs = _raw(lib, t, **change)
        assert rc == -1 and lib.loc_last_error().decode().startswith("loc_phase_viterbi: "), (change, lib.loc_last_error())
        assert all((o == pat).all() for o in outs), change
    assert lib.loc_phase_work_bytes(65, 5, 1, 0) == -1 and lib.loc_phase_work_bytes(1, 5, 1, 0) == -1
    assert lib.loc_phase_work_bytes(8, 5, 0, 0) == 0 and lib.loc_phase_work_bytes(8, 0, 3, 0) == 0
    rc, outs = _raw(lib, t, R=0)
    assert rc == 0 and all((o == pat).all() for o in outs)
    rc, outs = _raw(lib, t, K=0)                                                  # as loc_paint_copy: zeros, no recursion ran
    assert rc == 0 and (outs[0] == pat).all() and not outs[1][:6].any() and not any(o[:3].any() for o in outs[2:])
    first, ll, ns, nt, nd = PH.viterbi_host(np.zeros((0, 12), dtype=np.int8), [0, 1], [[2, 3], [4, 5]], np.zeros(0), 0.01)
    assert first.shape == (2, 0) and not ll.any() and not ns.any() and not nd.any()


def test_the_scratch_is_what_the_header_says():
    for S, slots in ((2, 16), (16, 16), (17, 32), (32, 32), (33, 64), (64, 64)):
        ck, bp = slots * 64 * 4, 64 * (slots // 16 + 1) * 4
        for K in (1, 50, 1000):
            for block in (1, 7, K, K + 9):
                B = min(block, K)
                assert _work_bytes(S, K, 3, block) == 3 * ((-(-K // B) - 1) * ck + B * bp)
            assert _work_bytes(S, K, 1) == min(_work_bytes(S, K, 1, B) for B in range(1, K + 1))          # block 0: the least


# ------------------------------------------------------------------ the command
def test_the_command_on_the_device_writes_the_bytes_of_host_and_paint_accepts_them(tmp_path):
    from locator_amd import paint as PT
    vcf = U.write_vcf_cut(str(tmp_path / "cut.vcf"), 40, 40, 400)
    outs = {}
    for name, extra in (("device", ["--budget_gb", "0.01"]), ("host", ["--host"])):
        out = str(tmp_path / name / "o")
        os.makedirs(os.path.dirname(out))
        assert PH.main(["--vcf", vcf, "--out", out, "--silence", "--states", "16", "--rounds", "3", "--check"] + extra) == 0
        outs[name] = out
    assert U.tree_bytes(outs["device"] + "_phased.zarr") == U.tree_bytes(outs["host"] + "_phased.zarr")
    text = {name: [line.split("\t") for line in open(out + "_phase_history.txt").read().splitlines()] for name, out in outs.items()}
    assert [r[:1] + r[2:] for r in text["device"]] == [r[:1] + r[2:] for r in text["host"]] and len(text["host"]) == 4
    for a, b in zip(text["device"][1:], text["host"][1:]):
        assert abs(float(a[1]) - float(b[1])) <= 1e-9 * (1 + abs(float(b[1])))
    import json
    sd, sh = (json.load(open(out + "_phase_summary.json")) for out in (outs["device"], outs["host"]))
    assert sd.pop("path") == "device" and sh.pop("path") == "host"
    assert abs(sd.pop("ll") - sh["ll"]) <= 1e-9 * (1 + abs(sh.pop("ll"))) and sd == sh
    out = str(tmp_path / "painted")
    assert PT.main(["--zarr", outs["device"] + "_phased.zarr", "--out", out, "--silence", "--em_rounds", "1", "--min_mac", "1"]) == 0
    assert os.path.exists(out + "_paint_summary.json")
