"""The ibd command on the device (locator_amd/csrc/ibd_kernels.hip): integer code, so every comparison is np.array_equal.

loc_ibd_pack against ibd.pack_host; loc_ibd_scan and loc_ibd_fill against ibd.segments_host on the planted fixtures of
tests/ibd_util.py (shown not to be vacuous from 130 sites on), over column counts around the 64 lanes of a wave and site counts
around the 64 sites of a word, every parameter set of the CPU test, chromosome starts inside a word and at a word boundary, pad
garbage, patterned planes and outputs.  The same bits under every batching of the rows, with columns appended and with the pads
changed; a capacity below the total only shortens the answer; bad arguments launch nothing.  The command on the device against
--host, file by file.

Measured on one MI355X: see DESIGN.md section 8 (the ibd command)."""
import os

import numpy as np
import pytest

from locator_amd import ibd as IB
from tests import ibd_util as U
from tests import paint_util as PU

pytestmark = pytest.mark.gpu
HS = (1, 2, 63, 64, 65, 130)
KS = (1, 63, 64, 65, 127, 128, 129, 200)
# chromosome starts besides site 0: one inside a word; one at a word boundary and one inside; one at the word boundary where the
# fixtures' one-site gaps lie, which forbids those links (no link is then asked of the fixture)
FIRSTS = ((34,), (128, 100), (64,))
FILLS = (0x5a5a5a5a, 0xffffffff)
PAT = np.array(0x5a5a5a5a, dtype=np.uint32).view(np.int32)


def device(fx, P, **kw):
    return IB.segments_device(fx["h"], fx["owner"], fx["first"], fx["x"], P, **kw)


# ------------------------------------------------------------------ loc_ibd_pack
def _pack(lib, t, h, H, K, pitch, wpitch, pattern=0x5a5a5a5a, rows=None):
    """One direct call: (return code, the planes as the launch left them, uint64 [2][max(W, 1)][wpitch])."""
    W = (K + 63) // 64
    d_h = t.from_numpy(np.ascontiguousarray(h)).cuda()
    bits = t.empty((2, max(W, 1), max(wpitch, 8)), dtype=t.int64, device="cuda:0")
    bits.view(t.int32).fill_(int(np.array(pattern, dtype=np.uint32).view(np.int32)))
    rc = lib.loc_ibd_pack(d_h.data_ptr(), H, K, pitch, bits.data_ptr(), wpitch, t.cuda.current_stream().cuda_stream)
    t.cuda.synchronize()
    return rc, bits.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("H", HS)
def test_pack_against_the_host_form(H):
    import torch as t
    from locator_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(H)
    for K in KS:
        h = rng.integers(-1, 2, (K, H)).astype(np.int8)
        h[rng.random((K, H)) < 0.05] = -128
        for n, (pitch, wpitch) in enumerate((((H + 15) // 16 * 16, (H + 7) // 8 * 8), ((H + 15) // 16 * 16 + 32, (H + 7) // 8 * 8 + 8),
                                             ((H + 15) // 16 * 16 + 16, (H + 7) // 8 * 8 + 24))):
            buf = IB.B.padded(h, pitch, rng if n % 2 else 0x55)
            rc, bits = _pack(lib, t, buf, H, K, pitch, wpitch, FILLS[n % 2])
            assert rc == 0 and np.array_equal(bits, IB.pack_host(h, H, K, wpitch)), (K, pitch, wpitch)


# ------------------------------------------------------------------ loc_ibd_scan + loc_ibd_fill
@pytest.mark.parametrize("H", HS)
def test_segments_against_the_host_form(H):
    rng = np.random.default_rng(H)
    segments = 0
    for K in KS:
        for n, P in enumerate(U.PARAMS):
            starts = FIRSTS[n % 3] if K >= 130 else FIRSTS[2 * (n % 2)]
            fx = U.fixture(H, K, 1000 * H + K + n, P, starts)
            want = U.host(fx, P)
            if K >= 130 and H >= 4 and starts != FIRSTS[2]:
                U.assert_not_vacuous(fx, P, want)
            got = device(fx, P, fill=FILLS[(n // 2) % 2], pad_fill=rng if n % 3 else 0x55, pitch=(H + 15) // 16 * 16 + 16 * (n % 3),
                         wpitch=(H + 7) // 8 * 8 + 8 * (n % 2))
            assert U.same(got, want), (K, P)
            segments += int(want[0].sum())
    print(f"H={H}: {segments} segments compared exactly")
    assert segments > 0 or H < 3


def test_the_same_bits_under_batching_appending_and_pad_garbage():
    H, K = 130, 200
    P = U.PARAMS[2]
    fx = U.fixture(H, K, 5, P, FIRSTS[1])
    want = U.host(fx, P)
    U.assert_not_vacuous(fx, P, want)
    assert U.same(device(fx, P), want)
    # rows in batches: R = 1, 7, all; then a budget of one byte, which is a row a launch
    for step in (1, 7, H):
        parts = [device(fx, P, rows=range(a, min(a + step, H)), fill=FILLS[1]) for a in range(0, H, step)]
        assert U.same([np.concatenate([p[i] for p in parts]) for i in range(5)], want), step
    assert U.same(device(fx, P, rows=range(0)), [v[:0] for v in want[:3]] + [want[3][:0], want[4][:0]])
    assert U.same(device(fx, P, budget=1), want)
    assert device(fx, P, segments=False)[3:] == (None, None) and U.same(device(fx, P, segments=False)[:3], want[:3])
    # the columns of fresh owners appended: what the earlier pairs hold does not change
    rng = np.random.default_rng(9)
    extra = 70
    more = dict(fx)
    more["h"] = np.concatenate([fx["h"], rng.integers(-1, 2, (K, extra)).astype(np.int8)], axis=1)
    more["owner"] = np.concatenate([fx["owner"], 1000 + np.arange(extra, dtype=np.int32) // 2])
    got = device(more, P, segments=False)
    assert U.same([v[:H, :H] for v in got[:3]], want[:3]) and U.same(got[:3], U.host(more, P, segments=False)[:3])
    # pad garbage of every kind
    for pad in (0, 1, -128, np.random.default_rng(1), np.random.default_rng(2)):
        assert U.same(device(fx, P, pad_fill=pad, pitch=160, wpitch=152), want)


def test_a_larger_fixture():
    H, K = 258, 1000
    P = IB.Params(12, 0, 3, 1, U.NO_LIMIT, 0)
    fx = U.fixture(H, K, 77, P, (64, 500, 640))
    want = U.host(fx, P)
    U.assert_not_vacuous(fx, P, want)
    assert U.same(device(fx, P, fill=FILLS[0]), want)
    print(f"H={H} K={K}: {int(want[0].sum())} segments, {int((want[0] > 0).sum())} pairs share")


# ------------------------------------------------------------------ direct calls
class Raw:
    """The device buffers of one fixture for direct calls of loc_ibd_scan and loc_ibd_fill, the outputs filled with PAT."""

    def __init__(self, fx, guard=64):
        import torch as t
        from locator_amd import _lib
        self.t, self.lib = t, _lib.load()
        self.H, self.K = len(fx["owner"]), fx["h"].shape[0]
        self.wp = (self.H + 7) // 8 * 8
        put = lambda v: t.from_numpy(np.ascontiguousarray(v)).cuda()
        self.bits = put(IB.pack_host(fx["h"], self.H, self.K).view(np.int64)) if self.K else t.zeros((2, 1, self.wp), dtype=t.int64, device="cuda:0")
        self.owner, self.first, self.x = put(fx["owner"]), put(IB.pack_first(fx["first"], self.K).view(np.int64)), put(fx["x"] if self.K else np.zeros(1, dtype=np.int64))
        self.guard = guard

    def outputs(self, R):
        t = self.t
        n = max(R, 1) * self.H
        outs = [t.empty(n, dtype=t.int32, device="cuda:0"), t.empty(2 * n, dtype=t.int32, device="cuda:0"), t.empty(2 * n, dtype=t.int32, device="cuda:0")]
        for o in outs:
            o.fill_(int(PAT))
        return outs

    def args(self, P, row0, rows, **change):
        a = dict(bits=self.bits.data_ptr(), wpitch=self.wp, H=self.H, K=self.K, owner=self.owner.data_ptr(), first=self.first.data_ptr(),
                 x=self.x.data_ptr(), p0=row0, R=rows, **P._asdict())
        a.update(change)
        return tuple(a.values())

    def scan(self, P, row0, rows, **change):
        outs = self.outputs(rows)
        rc = self.lib.loc_ibd_scan(*self.args(P, row0, rows, **change), *(o.data_ptr() for o in outs), self.t.cuda.current_stream().cuda_stream)
        self.t.cuda.synchronize()
        return rc, [o.cpu().numpy() for o in outs]

    def fill(self, P, row0, rows, offsets, capacity, room, **change):
        t = self.t
        seg = [t.empty(room + self.guard, dtype=t.int32, device="cuda:0") for _ in range(2)]
        for s in seg:
            s.fill_(int(PAT))
        d_off = t.from_numpy(np.ascontiguousarray(offsets, dtype=np.int64)).cuda()
        rc = self.lib.loc_ibd_fill(*self.args(P, row0, rows, **change), d_off.data_ptr(), capacity, seg[0].data_ptr(), seg[1].data_ptr(),
                                   t.cuda.current_stream().cuda_stream)
        t.cuda.synchronize()
        return rc, [s.cpu().numpy() for s in seg]


def test_a_capacity_below_the_total_only_shortens_the_answer():
    H, K = 66, 200
    P = U.PARAMS[2]
    fx = U.fixture(H, K, 21, P)
    count, length, longest, sa, sb = U.host(fx, P)
    total = int(count.sum())
    assert total > 20
    raw = Raw(fx)
    offsets = (np.cumsum(count.reshape(-1)) - count.reshape(-1)).astype(np.int64)
    for capacity in (total, total - 1, total // 2, 1, 0):
        rc, (a, b) = raw.fill(P, 0, H, offsets, capacity, total)
        assert rc == 0
        assert np.array_equal(a[:capacity], sa[:capacity]) and np.array_equal(b[:capacity], sb[:capacity]), capacity
        assert (a[capacity:] == PAT).all() and (b[capacity:] == PAT).all(), capacity       # the rest of the buffer and the guard behind it
    # offsets that do not belong to the counts stay inside the capacity all the same
    wild = np.where(np.arange(H * H) % 3 == 0, -5, offsets + total - 3)
    rc, (a, b) = raw.fill(P, 0, H, wild, total, total)
    assert rc == 0 and (a[total:] == PAT).all() and (b[total:] == PAT).all()


def test_bad_arguments_launch_nothing_and_empty_inputs_are_as_specified():
    import torch as t
    H, K = 10, 70
    P = U.PARAMS[2]
    fx = U.fixture(H, K, 3, P)
    raw = Raw(fx)
    want = U.host(fx, P)
    rc, outs = raw.scan(P, 2, 5)
    assert rc == 0 and np.array_equal(outs[0], want[0][2:7].reshape(-1)) and np.array_equal(outs[1].view(np.int64), want[1][2:7].reshape(-1))
    assert np.array_equal(outs[2].view(np.int64), want[2][2:7].reshape(-1))
    bad = [dict(H=0), dict(H=IB.MAX_HAPS + 1, wpitch=IB.MAX_HAPS + 8), dict(K=-1), dict(K=2 ** 31), dict(wpitch=8), dict(wpitch=20),
           dict(extend_sites=13), dict(extend_sites=0), dict(seed_sites=0), dict(gap_sites=IB.MAX_GAP + 1), dict(gap_sites=-1),
           dict(seed_len=-1), dict(gap_len=-1), dict(min_len=-1), dict(p0=6), dict(p0=-1), dict(R=-1), dict(p0=H, R=1)]
    offsets = np.zeros(5 * H, dtype=np.int64)
    for change in bad:
        rc, outs = raw.scan(P, 2, 5, **change)
        assert rc == -1 and raw.lib.loc_last_error() and all((o == PAT).all() for o in outs), change
        rc, seg = raw.fill(P, 2, 5, offsets, 8, 8, **change)
        assert rc == -1 and all((s == PAT).all() for s in seg), change
    rc, seg = raw.fill(P, 2, 5, offsets, -1, 8)
    assert rc == -1 and all((s == PAT).all() for s in seg)
    # loc_ibd_pack
    lib, h = raw.lib, IB.B.padded(fx["h"], 16, 0)
    ok = dict(H=H, K=K, pitch=16, wpitch=16)
    assert _pack(lib, t, h, **ok)[0] == 0
    for change in (dict(H=0), dict(H=IB.MAX_HAPS + 1, pitch=IB.MAX_HAPS + 16, wpitch=IB.MAX_HAPS + 8), dict(K=-1), dict(pitch=0), dict(pitch=8),
                   dict(pitch=24), dict(H=20, pitch=16, wpitch=24), dict(wpitch=8), dict(wpitch=12)):
        rc, bits = _pack(lib, t, h, **{**ok, **change})
        assert rc == -1 and lib.loc_last_error() and (bits.view(np.int32) == PAT).all(), change
    rc, bits = _pack(lib, t, h, **{**ok, "K": 0})
    assert rc == 0 and (bits.view(np.int32) == PAT).all()                                  # no site: nothing to write
    # R = 0 launches nothing; K = 0 gives zeros
    rc, outs = raw.scan(P, 2, 0)
    assert rc == 0 and all((o == PAT).all() for o in outs)
    rc, outs = raw.scan(P, 2, 5, K=0)
    assert rc == 0 and not any(o[:n].any() for o, n in zip(outs, (5 * H, 10 * H, 10 * H)))
    rc, seg = raw.fill(P, 2, 5, offsets, 8, 8, K=0)
    assert rc == 0 and all((s == PAT).all() for s in seg)
    empty = {"h": np.zeros((0, H), dtype=np.int8), "owner": fx["owner"], "first": np.zeros(0, dtype=bool), "x": np.zeros(0, dtype=np.int64)}
    assert U.same(device(empty, P, fill=FILLS[0]), U.host(empty, P)) and not device(empty, P)[0].any()
    with pytest.raises(ValueError):
        device({**fx, "owner": np.zeros(IB.MAX_HAPS + 1, dtype=np.int32)}, P)


# ------------------------------------------------------------------ the command
def test_the_command_on_the_device_against_host(tmp_path):
    vcf = PU.write_vcf_cut(str(tmp_path / "cut.vcf"), 40, 60, 900)
    outs = {}
    for name, extra in (("device", []), ("host", ["--host"]), ("batched", ["--budget_gb", "0.00001"])):
        outs[name] = str(tmp_path / name / "o")
        os.makedirs(os.path.dirname(outs[name]))
        assert IB.main(["--vcf", vcf, "--sample_data", U.SAMPLE_DATA, "--out", outs[name], "--silence", "--seed_sites", "40", "--extend_sites", "8",
                        "--kmax", "8", "--keep_matrix", "--keep_segments"] + extra) == 0
    files = sorted(os.listdir(os.path.dirname(outs["host"])))
    assert files == sorted("o" + n for n in ("_ibd_summary.json", "_ibd_pairs.txt", "_ibd_locs.txt", "_ibd_segments.txt", "_ibd.npz"))
    for name in ("device", "batched"):
        assert sorted(os.listdir(os.path.dirname(outs[name]))) == files
        for n in files:
            got = open(os.path.join(os.path.dirname(outs[name]), n), "rb").read()
            want = open(os.path.join(os.path.dirname(outs["host"]), n), "rb").read()
            if n.endswith("_summary.json"):                                          # the one entry that names the path
                assert b'"path": "device"' in got and b'"path": "host"' in want
                got = got.replace(b'"path": "device"', b'"path": "host"')
            assert got == want, (name, n)
    assert len(open(outs["host"] + "_ibd_segments.txt").read().splitlines()) > 100
