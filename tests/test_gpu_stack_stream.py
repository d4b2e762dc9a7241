"""The weight stream of the fused hidden stack (stack_fused.hip): a register ring of untracked loads with hand-counted waits
that runs through every layer pass of loc_stack_forward_backward and loc_stack_forward_eval_form (locator.py:319-325 layers
2..L, Dense(2) x 2, euclidean_distance_loss and their backward pass), called directly through the C ABI at the smallest
shapes at which a ring can go wrong:

  padded widths 64 / 128 / 256 / 512   k-group of a thread 2 / 8 / 32 / 128 rows: two slots of one row, a whole layer in
                                       eight slots, one trip round the ring per pass, four trips
  L = 2, 3, 10                         one hidden layer (the ring wraps from pass 0 straight into the backward pass and then
                                       into the dummy behind the last pass), two passes of an eval launch, the usual depth
  n_b = 1, 10, 32 (slot 32), 33 (64)   one row, a short block, a full block, a second block with one row
  with / without a dropout mask        the mask is an epilogue operand of one forward and one backward pass
  independent random weights per layer, WhT from loc_transpose_hidden: a slot filled from the wrong layer or copy shows
  output buffers pre-filled with NaN

Checks: (a) acts, adrop, dz, head_out and yhat / dist against the float64 reference of tests/test_gpu_stack_train.py (pinned
to the oracle there) within the 2e-5 absolute that tests/test_gpu_parity.py grants activations, predictions and losses;
(b) the same bits with 1, 2 and 4 rows per workgroup, and with 2, 4 and 8 rows in the eval forms of width 256; (c) the same
bits without and with 12 L2 warm-up helpers and at XCD strides 1 and 8; (d) the same bits from the drained twin library
(`make debug_drain`: every hand count becomes vmcnt(0)).

The 2e-5 of (a) is an absolute bound for O(1) quantities.  For dz and the loss gradient dy2, which scale with 1 / n_b, it is
loose: it is NOT the accuracy of the backward pass.  That is guarded by the relative, per-row bounds of
tests/test_gpu_stack_train.py and by the bitwise checks (b) - (d) here."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from locator_amd import _lib
from oracle import locator_oracle as O
from tests.gpu_util import bits, maxerr
from tests.test_gpu_stack_train import _Stack, _tensors

pytestmark = pytest.mark.gpu

TOL = 2e-5          # tests/test_gpu_parity.py: activations / predictions / losses, absolute on O(1) values

_twin = None


def _drained():
    """The parity-debug twin (part of build()), bound with the product's prototypes.  Both libraries run on the HIP runtime
    that torch loaded; every buffer is passed in, so one process can call both."""
    global _twin
    if _twin is None:
        path = os.path.join(os.path.dirname(_lib.LIB_PATH), "liblocator_hip_drain.so")
        assert os.path.exists(path), f"{path} not built (make -C locator_amd/csrc debug_drain, part of build())"
        _twin = C.CDLL(path)
        for name in ("loc_stack_forward_backward", "loc_stack_forward_eval_form", "loc_last_error"):
            fn = getattr(_twin, name)
            fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return _twin


def _train(s, lib, tune=None):
    """One loc_stack_forward_backward of `lib` on freshly poisoned buffers -> the bits of the four buffers."""
    s.fill("zero")
    net, b = s.net, s.bufs
    lay, P = net.lay, net.params.data_ptr()
    a1_in = b["adrop"] if s.adrop_is_input else b["acts"]
    rc = lib.loc_stack_forward_backward(
        a1_in.data_ptr(), P + 4 * lay.wh, net.wht.data_ptr(), P + 4 * lay.bh, P + 4 * lay.wa, P + 4 * lay.ba, P + 4 * lay.wb,
        P + 4 * lay.bb, s.mask.data_ptr() if s.drop else None, s.ks, s.Hp, s.L, net.d.n_pre, s.n_b, s.slot,
        s.rows.data_ptr(), net.Y.data_ptr(), b["acts"].data_ptr(), b["adrop"].data_ptr(), b["dz"].data_ptr(),
        b["head_out"].data_ptr(), C.byref(tune) if tune is not None else None, None)
    torch.cuda.synchronize()
    assert rc == 0, lib.loc_last_error()
    return {k: bits(t).clone() for k, t in b.items()}


def _eval(s, lib, a1_dev, form):
    net = s.net
    lay, P = net.lay, net.params.data_ptr()
    yhat = torch.full((s.n_b, 2), float("nan"), device="cuda")
    dist = torch.full((s.n_b,), float("nan"), device="cuda")
    rc = lib.loc_stack_forward_eval_form(a1_dev.data_ptr(), P + 4 * lay.wh, P + 4 * lay.bh, P + 4 * lay.wa, P + 4 * lay.ba,
                                         P + 4 * lay.wb, P + 4 * lay.bb, s.Hp, s.L, s.n_b, s.rows.data_ptr(), net.Y.data_ptr(),
                                         yhat.data_ptr(), dist.data_ptr(), form, None)
    torch.cuda.synchronize()
    assert rc == 0, lib.loc_last_error()
    return yhat.cpu().numpy(), dist.cpu().numpy()


def _same(got, ref, what):
    for k in ref:
        assert torch.equal(got[k], ref[k]), (what, k, int((got[k] != ref[k]).sum()))


CASES = [(w, L, n_b, slot, drop) for w in (64, 128, 256, 512) for L in (2, 3, 10)
         for n_b, slot in ((1, 32), (10, 32), (32, 32), (33, 64)) for drop in (True, False)]


@pytest.mark.parametrize("width,L,n_b,slot,drop", CASES,
                         ids=[f"w{w}-L{L}-n{n}-slot{s}-{'drop' if d else 'nodrop'}" for w, L, n, s, d in CASES])
def test_training_stream(width, L, n_b, slot, drop):
    s = _Stack(width, L, n_b, slot, drop, seed=1000 * L + width + n_b, kind="nan")
    lib = s.net.lib
    ref_bits = _train(s, lib)
    out = s.outputs()
    s.check_margins()

    # (a) rows < n_b against the float64 reference
    _, r64 = s.reference(np.float64)
    want, got = _tensors(s, r64, False), _tensors(s, out, True)
    worst = {k: maxerr(got[k], want[k]) for k in want}
    k = max(worst, key=worst.get)
    print(f"stream width {width} L {L} n_b {n_b} drop {drop}: largest absolute error {worst[k]:.2e} ({k})")
    assert np.isfinite(worst[k]) and worst[k] < TOL, worst
    assert not out["dz"][:, n_b:s.used].any()

    # (b), (c) rows per workgroup x helpers x XCD stride: the default's bits
    for rows in (1, 2, 4):
        for helpers in (-1, 12):
            for stride in (1, 8):
                tune = _lib.Tuning(stack_train_rows=rows, stack_xcd_stride=stride, stack_helpers=helpers)
                _same(_train(s, lib, tune), ref_bits, (rows, helpers, stride))

    # (d) the drained twin
    twin = _drained()
    _same(_train(s, twin), ref_bits, "drained twin")
    for rows in (2, 4):
        _same(_train(s, twin, _lib.Tuning(stack_train_rows=rows)), ref_bits, ("drained twin", rows))
    s.check_margins()


EVAL_CASES = [(w, L, n_b) for w in (64, 128, 256, 512) for L in (2, 3, 10) for n_b in (1, 10, 32, 33)]


@pytest.mark.parametrize("width,L,n_b", EVAL_CASES, ids=[f"w{w}-L{L}-n{n}" for w, L, n in EVAL_CASES])
def test_eval_stream(width, L, n_b):
    s = _Stack(width, L, n_b, 64, False, seed=2000 * L + width + n_b, kind="nan")
    lib = s.net.lib
    a1_dev = torch.zeros(((n_b + 7) // 8 * 8, s.Hp), device="cuda")       # whole row groups of every form
    a1_dev[:n_b] = s.a1_dev

    # (a) inference forward in float64: no dropout
    p = s.p
    a = s.a1
    for l in range(2, L + 1):
        a = O.elu(a @ p["W"][l - 1] + p["b"][l - 1])
    y2 = (a @ p["W"][L] + p["b"][L]) @ p["W"][L + 1] + p["b"][L + 1]
    yhat, dist = _eval(s, lib, a1_dev, -1)
    e_y, e_d = maxerr(yhat, y2), maxerr(dist, O.euclid(y2, s.y))
    print(f"stream eval width {width} L {L} n_b {n_b}: yhat {e_y:.2e} dist {e_d:.2e}")
    assert np.isfinite(e_y) and e_y < TOL and np.isfinite(e_d) and e_d < TOL

    # (b) rows per workgroup (the forms other than 2 rows exist at width 256), the default form at this row count
    forms = (0, -2, -3) if s.Hp == 256 else (0,)
    for form in forms:
        y_f, d_f = _eval(s, lib, a1_dev, form)
        assert np.array_equal(y_f.view(np.int32), yhat.view(np.int32)) and np.array_equal(d_f.view(np.int32), dist.view(np.int32)), form

    # (d) the drained twin
    twin = _drained()
    for form in (-1,) + forms[1:]:
        y_t, d_t = _eval(s, twin, a1_dev, form)
        assert np.array_equal(y_t.view(np.int32), yhat.view(np.int32)) and np.array_equal(d_t.view(np.int32), dist.view(np.int32)), form


def test_a_stack_without_a_layer_pass_is_refused():
    """The kernel waits for its labels and its ring inside the layer passes, so L < 2 is an error at the entry points, with a
    message and no byte written."""
    s = _Stack(128, 2, 10, 32, False, seed=5, kind="junk")
    s.fill("zero")
    net, b = s.net, s.bufs
    lay, P = net.lay, net.params.data_ptr()
    rc = net.lib.loc_stack_forward_backward(
        b["acts"].data_ptr(), P + 4 * lay.wh, net.wht.data_ptr(), P + 4 * lay.bh, P + 4 * lay.wa, P + 4 * lay.ba, P + 4 * lay.wb,
        P + 4 * lay.bb, None, 1.0, s.Hp, 1, 0, s.n_b, s.slot, s.rows.data_ptr(), net.Y.data_ptr(), b["acts"].data_ptr(),
        b["adrop"].data_ptr(), b["dz"].data_ptr(), b["head_out"].data_ptr(), None, None)
    assert rc != 0 and net.lib.loc_last_error().decode()
    yhat = torch.full((s.n_b, 2), float("nan"), device="cuda")
    rc = net.lib.loc_stack_forward_eval_form(s.a1_dev.data_ptr(), P + 4 * lay.wh, P + 4 * lay.bh, P + 4 * lay.wa, P + 4 * lay.ba,
                                             P + 4 * lay.wb, P + 4 * lay.bb, s.Hp, 1, s.n_b, None, None, yhat.data_ptr(), None, -1, None)
    torch.cuda.synchronize()
    assert rc != 0 and net.lib.loc_last_error().decode()
    assert torch.isnan(yhat).all()
    for k, t in b.items():
        assert torch.equal(bits(t), s.before[k]), k
