"""loc_epoch_callbacks and loc_snapshot_if called directly, epoch by epoch, against tests/keras_callbacks_ref.py.

Every fit's history, stop epoch, learning-rate column and kept weights come from these two entry points; the fits of the
suite reach them with whatever val_loss sequence training happens to produce.  Here the sequence is scripted:

  * the validation distances of an epoch are all the same fp32 value v, so their double sum divided by n_val is exactly
    v and a tie with the best value is a real tie; NaN and +inf are put in the same way;
  * the per-step losses are random fp32; loss_j * n_j is exact in double (24 x 8 bits), so the index-order float64 sum
    divided by n_train is the one value the kernel may write, fused multiply-add or not;
  * for the LDS staging loops the distances are distinct random fp32 and the expected val_loss is their index-order float64
    sum, so a chunk of 1024 that is skipped, read twice or read from the wrong offset shows.

After every epoch the whole state struct, the mirrored learning rate, the whole history buffer and the whole `best`
buffer are compared with the reference - bit for bit, NaN compared as NaN - and save_now is also read between the two
calls.  State, learning rate, history and `best` sit inside guard margins (tests/gpu_util.guarded)."""
import ctypes as C
import struct

import numpy as np
import pytest
import torch

from locator_amd import _lib
from tests import keras_callbacks_ref as KR
from tests.gpu_util import GUARD_BYTES, guarded

pytestmark = pytest.mark.gpu

MARGIN = 4096
INT_FIELDS = ("es_wait", "rl_wait", "epoch", "stopped", "stop_epoch", "best_epoch", "save_now")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset) if t is not None else None


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_f64(got, want, nan_ok=True):
    """Bit-equal doubles; where nan_ok (a mask, or everywhere) a NaN that is expected matches any NaN: the payload of a NaN
    val_loss carries nothing."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool(np.all((_u64(got) == _u64(want)) | (nan_ok & np.isnan(got) & np.isnan(want))))


def _host_bits(t):
    return t.detach().cpu().contiguous().view(-1).view(torch.uint8).numpy().copy()


def expected_loss(losses, batch, n_last):
    """Index-order float64 sum of loss_j * n_j, divided by n_train (np.cumsum adds strictly left to right)."""
    sizes = np.full(len(losses), batch, np.float64)
    sizes[-1] = n_last
    return np.cumsum(losses.astype(np.float64) * sizes)[-1] / np.float64((len(losses) - 1) * batch + n_last)


def expected_val(dists):
    return np.cumsum(dists.astype(np.float64))[-1] / np.float64(len(dists))


class Rig:
    """One callback state on the device, set up as EpochRunner.enable_device_callbacks does, with the buffers the two entry
    points write inside guard margins."""

    def __init__(self, steps, batch, n_last, n_val, patience, lr_patience, factor, hist_cap, n_params=64, lr0=KR.LR0):
        self.lib = _lib.load()
        self.steps, self.batch, self.n_last, self.n_val, self.hist_cap = steps, batch, n_last, n_val, hist_cap
        self.cb = (patience, lr_patience, factor, lr0)
        st = _lib.CbState()
        st.ck_best = st.es_best = st.rl_best = float("inf")
        st.lr = float(np.float32(lr0))
        st.lr_factor = float(factor)
        st.patience, st.lr_patience = int(patience), int(lr_patience)
        st.stop_epoch = st.best_epoch = -1
        self.checks = []
        self.state = self._guarded(C.sizeof(_lib.CbState), torch.uint8, "state")
        self.state.copy_(torch.from_numpy(np.frombuffer(bytes(st), dtype=np.uint8).copy()))
        self.lr = self._guarded(1, torch.float32, "lr")
        self.lr.fill_(st.lr)
        self.hist = self._guarded(4 * hist_cap, torch.float64, "hist")
        self.best = self._guarded(n_params, torch.float32, "best")
        self.stats = torch.zeros(steps + n_val, dtype=torch.float32, device="cuda")
        self.params = torch.zeros(n_params, dtype=torch.float32, device="cuda")
        self.want_hist = _host_bits(self.hist).view(np.float64).copy()       # rows nobody wrote keep the guard pattern
        self.want_best = _host_bits(self.best)
        self.nan_rows = np.zeros(4 * hist_cap, bool)                         # history values written as a NaN val_loss
        self.rng = np.random.default_rng(steps * 1000003 + n_val)

    def _guarded(self, n, dtype, name):
        view, check = guarded(n, dtype, MARGIN)
        self.checks.append(lambda: check(name))
        return view

    def read_state(self):
        return _lib.CbState.from_buffer_copy(self.state.cpu().numpy().tobytes())

    def callbacks(self, **over):
        a = dict(stats=_p(self.stats), steps=self.steps, batch=self.batch, n_last=self.n_last, n_val=self.n_val,
                 state=_p(self.state), lr=_p(self.lr), hist=_p(self.hist), hist_cap=self.hist_cap)
        a.update(over)
        return self.lib.loc_epoch_callbacks(a["stats"], a["steps"], a["batch"], a["n_last"], a["n_val"], a["state"], a["lr"],
                                            a["hist"], a["hist_cap"], _stream())

    def snapshot(self):
        return self.lib.loc_snapshot_if(_p(self.state), _p(self.params), _p(self.best), self.params.numel(), _stream())

    def upload_epoch(self, dists):
        """Fresh random per-step losses and parameters, the given validation distances -> expected loss."""
        losses = self.rng.uniform(0.05, 3.0, self.steps).astype(np.float32)
        self.params_host = self.rng.standard_normal(self.params.numel()).astype(np.float32)
        self.stats.copy_(torch.from_numpy(np.concatenate([losses, np.asarray(dists, np.float32)])))
        self.params.copy_(torch.from_numpy(self.params_host))
        return expected_loss(losses, self.batch, self.n_last)

    def assert_epoch(self, want, loss, mid, where):
        """The device after both calls of one epoch (and `mid`, the state between them) against the trace entry `want`."""
        if want["row"] is not None and want["epoch"] - 1 < self.hist_cap:
            val, lr_logged, flags = want["row"]
            self.want_hist[4 * (want["epoch"] - 1):4 * want["epoch"]] = (loss, val, lr_logged, flags)
            self.nan_rows[4 * (want["epoch"] - 1) + 1] = np.isnan(val)
        if want["save_now"]:
            self.want_best = self.params_host.view(np.uint8).copy()
        st = self.read_state()
        for name, s in (("between the calls", mid), ("after the epoch", st)):
            if s is None:
                continue
            for f in ("ck_best", "es_best", "rl_best"):
                assert struct.pack("d", getattr(s, f)) == struct.pack("d", float(want[f])), (where, name, f, getattr(s, f), want[f])
            for f in INT_FIELDS:
                assert getattr(s, f) == want[f], (where, name, f, getattr(s, f), want[f])
            assert np.float32(s.lr).tobytes() == np.float32(want["lr"]).tobytes(), (where, name, s.lr, want["lr"])
            assert (s.patience, s.lr_patience, np.float32(s.lr_factor)) == (self.cb[0], self.cb[1], np.float32(self.cb[2]))
        assert _host_bits(self.lr).tobytes() == np.float32(want["lr_mirror"]).tobytes(), (where, "*lr", want["lr_mirror"])
        got_hist = _host_bits(self.hist).view(np.float64)
        assert _same_f64(got_hist, self.want_hist, self.nan_rows), (where, "hist", got_hist.reshape(-1, 4), self.want_hist.reshape(-1, 4))
        assert np.array_equal(_host_bits(self.best), self.want_best), (where, "best")
        assert np.array_equal(_host_bits(self.params), self.params_host.view(np.uint8)), (where, "params were written")
        return st

    def run(self, dist_rows, where, launch=None):
        """dist_rows: one array of n_val validation distances per epoch.  launch: what enqueues the two calls (a graph replay);
        None = eager calls with the state read between them.  -> the raw device bytes after every epoch."""
        vals = [expected_val(np.asarray(d, np.float32)) for d in dist_rows]
        trace = KR.device_trace(vals, *self.cb)
        out = []
        for e, (d, want) in enumerate(zip(dist_rows, trace)):
            loss = self.upload_epoch(d)
            mid = None
            if launch is None:
                assert self.callbacks() == 0, self.lib.loc_last_error()
                mid = self.read_state()
                assert self.snapshot() == 0, self.lib.loc_last_error()
            else:
                launch()
            self.assert_epoch(want, loss, mid, f"{where}, epoch {e}")
            out.append(b"".join(_host_bits(t).tobytes() for t in (self.state, self.lr, self.hist, self.best)))
        for c in self.checks:
            c()
        return trace, out


def _constant_rows(vals, n_val):
    return [np.full(n_val, v, np.float32) for v in vals]


@pytest.mark.parametrize("name", sorted(KR.SEQUENCES))
def test_scripted_sequence(name):
    """Ties, plateaus, resets, NaN / +inf, patience 0 and 1, int(patience / 6) == 0, and the epochs enqueued behind the stop
    epoch (only `epoch` advances; save_now 0; *lr, bests, waits, stop_epoch, best_epoch, hist and best frozen)."""
    vals, patience, lr_patience, factor = KR.SEQUENCES[name]
    rig = Rig(steps=5, batch=32, n_last=7, n_val=9, patience=patience, lr_patience=lr_patience, factor=factor,
              hist_cap=len(vals))
    trace, _ = rig.run(_constant_rows(vals, rig.n_val), name)
    assert all(_same_f64(s["row"][0], v) for s, v in zip(trace, vals) if s["row"]), "a constant column's mean is the constant"
    if name.startswith("main"):
        stop = next(e for e, s in enumerate(trace) if s["stopped"])
        assert len(vals) - 1 - stop >= 3 and trace[-1]["epoch"] == len(vals) and trace[-1]["stop_epoch"] == stop
        assert sum(1 for s in trace if s["row"] and s["row"][2] >= 4) >= 2
    if name == "nan-first-never-better":
        assert trace[-1]["best_epoch"] == -1 and not any(s["save_now"] for s in trace)
        assert np.array_equal(rig.want_best, np.tile(np.array(GUARD_BYTES, np.uint8), 64)), "best was never written"
    if name.startswith("patience"):
        assert trace[0]["stopped"] == 0
        if patience == 0 or name == "patience1-nan-first":
            assert trace[0]["es_wait"] >= patience, "wait >= patience at epoch 0 and still no stop"
        assert trace[-1]["stop_epoch"] == (2 if name in ("patience1-improving", "patience1-nan-first") else 1)


def test_more_epochs_than_history_rows():
    """hist_cap 3, 6 epochs: rows 0-2 are written, nothing lands at or beyond row 3 (the guard margin starts there), and
    the state goes on as if the history were long enough."""
    vals = [2.0, 1.5, 1.5, 1.0, 1.25, 0.5]
    rig = Rig(steps=3, batch=16, n_last=16, n_val=4, patience=6, lr_patience=1, factor=0.5, hist_cap=3)
    trace, _ = rig.run(_constant_rows(vals, 4), "hist_cap 3")
    assert [s["best_epoch"] for s in trace] == [0, 1, 1, 3, 3, 5] and trace[-1]["epoch"] == 6
    full = KR.device_trace(vals, 6, 1, 0.5, KR.LR0)
    assert [s["lr"] for s in trace] == [s["lr"] for s in full]


@pytest.mark.parametrize("batch,n_last", [(32, 5), (1, 1)], ids=["batch32-last5", "batch1"])
@pytest.mark.parametrize("steps,n_val", [(1, 1), (4, 1024), (4, 1025), (1025, 7), (2049, 3000)])
def test_staging_loops(steps, n_val, batch, n_last):
    """Both 1024-value LDS staging loops at one value, exactly one chunk, one value into the second chunk, and several
    chunks with a partial last one; distinct random distances, three epochs with fresh numbers."""
    rig = Rig(steps=steps, batch=batch, n_last=n_last, n_val=n_val, patience=6, lr_patience=1, factor=0.5, hist_cap=3)
    rng = np.random.default_rng(steps * 7919 + n_val)
    rows = [rng.uniform(0.01, 4.0, n_val).astype(np.float32) for _ in range(3)]
    rig.run(rows, f"steps {steps}, n_val {n_val}")


def test_bad_arguments_are_refused_and_launch_nothing():
    rig = Rig(steps=4, batch=8, n_last=3, n_val=5, patience=6, lr_patience=1, factor=0.5, hist_cap=2)
    rig.upload_epoch(np.full(5, 1.0, np.float32))
    before = [_host_bits(t) for t in (rig.state, rig.lr, rig.hist, rig.best)]
    for over in ({"steps": 0}, {"n_last": 9}, {"n_last": 0}, {"n_val": 0}, {"batch": 0}, {"state": None}, {"lr": None},
                 {"hist": None}):
        assert rig.callbacks(**over) != 0, over
        assert b"loc_epoch_callbacks" in rig.lib.loc_last_error(), over
    n = rig.params.numel()
    for args in ((_p(rig.state), _p(rig.params), _p(rig.best), n - 1),            # not a multiple of 4 floats
                 (_p(rig.state), _p(rig.params, 4), _p(rig.best), n - 4),          # misaligned source
                 (_p(rig.state), _p(rig.params), _p(rig.best, 8), n - 4)):         # misaligned destination
        assert rig.lib.loc_snapshot_if(*args, _stream()) != 0
        assert b"loc_snapshot_if" in rig.lib.loc_last_error()
    torch.cuda.synchronize()
    for t, b in zip((rig.state, rig.lr, rig.hist, rig.best), before):
        assert np.array_equal(_host_bits(t), b)
    assert rig.read_state().epoch == 0
    for c in rig.checks:
        c()


@pytest.mark.parametrize("save_now", [0, 1])
@pytest.mark.parametrize("n", [4, 1020, 4 * (1024 * 256) + 4])
def test_snapshot_if(n, save_now):
    """One vector, less than one workgroup's worth, and one vector past a full sweep of the 1024 x 256 grid: a bit-equal
    copy or an untouched destination, the source untouched, both inside guard margins."""
    lib = _lib.load()
    st = _lib.CbState()
    st.save_now = save_now
    state = torch.from_numpy(np.frombuffer(bytes(st), dtype=np.uint8).copy()).cuda()
    src, check_src = guarded(n, torch.float32, MARGIN)
    dst, check_dst = guarded(n, torch.float32, MARGIN)
    host = np.random.default_rng(n).integers(0, 1 << 32, n, dtype=np.uint32)      # every bit pattern, NaNs included
    src.view(torch.int32).copy_(torch.from_numpy(host.view(np.int32)))
    before = _host_bits(dst)
    assert lib.loc_snapshot_if(_p(state), _p(src), _p(dst), n, _stream()) == 0, lib.loc_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(_host_bits(dst), host.view(np.uint8) if save_now else before)
    assert np.array_equal(_host_bits(src), host.view(np.uint8))
    assert np.array_equal(_host_bits(state), np.frombuffer(bytes(st), dtype=np.uint8))
    check_src("params")
    check_dst("best")


def test_captured_graph_equals_eager_calls():
    """[loc_epoch_callbacks, loc_snapshot_if] captured once as a linear chain, the way EpochRunner captures an epoch, and
    replayed once per scripted epoch with stats and params rewritten in between: the same bytes as eager calls."""
    vals, patience, lr_patience, factor = KR.SEQUENCES["main-p6-lp1-f0.25"]
    kw = dict(steps=5, batch=32, n_last=7, n_val=1030, patience=patience, lr_patience=lr_patience, factor=factor,
              hist_cap=len(vals), n_params=1020)
    rows = _constant_rows(vals, kw["n_val"])
    _, eager = Rig(**kw).run(rows, "eager")
    rig = Rig(**kw)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        assert rig.callbacks() == 0, rig.lib.loc_last_error()
        assert rig.snapshot() == 0, rig.lib.loc_last_error()
    torch.cuda.synchronize()
    assert rig.read_state().epoch == 0, "capturing runs nothing"
    _, replayed = rig.run(rows, "graph", launch=g.replay)
    assert replayed == eager
