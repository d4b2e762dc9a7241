"""explain_kernels.hip entry point by entry point: loc_explain_stack_grad with layer 1's output given, loc_explain_sites +
loc_explain_reduce with delta1 given, called through _lib.load() on the test's own buffers (tests/explain_util.py).

tests/test_gpu_explain.py runs the same kernels through the package (locator_amd/explain.py): widths that pad to a multiple
of 64, the split count loc_explain_splits picks (one M tile per split on a 256-unit device), buffers of torch.empty, and
constant bounds (1e-5 of a row's maximum, 1e-4 relative).  Here:

  - padded widths 32, 96, 160, where the `c0 + c < Hp` guards of ex_dense_kernel's 64-column tile run, next to 64 and 1024;
    2n = 62 / 64 / 66 and n = 64 / 65 around its 64-row tile; both parities of L - 1 (the ping-pong between g and delta1)
    and L = 1; the forward activations of every layer, not only delta1;
  - every split count the launcher takes - for n = 300 (5 M tiles) 1, 2, 3 and 5, i.e. workgroups that walk 5, 3 + 2 and
    2 + 2 + 1 tiles - each split's partial sums against the float64 form of exactly its samples; n and Ks on both sides of
    the 64-sample and 128-site tiles; 1 to 32 h chunks; genotypes in q units (0..126); three row pitches with two fillings
    of the pad columns;
  - every output and scratch buffer a guarded view of exactly the size include/locator_hip.h documents, poisoned with NaN
    and with finite junk: the two runs agree bit for bit (every element is written by the call, none read before), no
    margin is touched; the operands are guarded too, so a read past an operand's end would meet NaN;
  - the refusals: -1, the function's name in loc_last_error, nothing launched.

Bounds (the floor rule of tests/test_gpu_stack_train.py and tests/test_gpu_moments.py): F = the distance of the float32
NumPy form from the float64 one on the same inputs, per metric - relative L2 per tensor and worst relative L2 per row for
acts and delta1, relative L2 over sites per statistic and worst per-site relative error for partial and out.  The device may
be MARGIN times as far (explain_util.MARGIN_STACK / MARGIN_STATS) and never more than CAP (1e-5 / 1e-4: what
tests/test_gpu_explain.py grants); tests/test_explain.py checks 0 < F and MARGIN F < CAP for every case without a GPU.
Across split counts `out` agrees within 2 n 2^-52 relative: every statistic is an fp64 sum of at most n non-negative fp32
terms that do not depend on the split, each order of summation is within (n - 1) 2^-53 of the exact sum, and the division
and the square root add 2^-53 each.

Every case prints device / F per metric (pytest -s).  Largest ratios measured on an MI355X, (tensor or statistic L2, worst
row or site), with their cases:
  acts     1.60 (65, 1024, 3)      1.56 (33, 1000, 2)
  delta1   1.63 (65, 1024, 3)      1.66 (65, 1024, 3)         -> MARGIN_STACK = 4
  partial  8.77 (65, 129, 1000, 2), splits 2, the split of sample 64 alone; 8.73 there too
  out      8.86 (65, 129, 1000, 2) 8.40 (65, 129, 1000, 2)    -> MARGIN_STATS = 18
The statistics stay between 0.8 and 3.9 at widths <= 160.  At width 1000 the ratio is the order of summation: one MFMA
accumulator adds the Hp products of a J one after the other, BLAS sums them in blocks, and the float32 form with J
accumulated sequentially (np.cumsum over h) is 8.76 F / 8.40 F from float64 on the CPU.  In absolute terms the device is
never further than 1.0e-6 (delta1, worst row, (65, 96, 10)) and 1.7e-6 (partial, worst site).

Mutations of explain_kernels.hip tried on a scratch copy: the column guards of ex_dense_kernel dropped -> the guard margin
of acts, cases (31, 96, 2), (32, 96, 3), (33, 160, 4), (65, 96, 10); jx / jy swapped, and the last 32-wide h chunk skipped
-> the floor rule in every case of test_sites_with_every_accepted_split_count; partial written for s <= Ks -> the guard
margin of partial, every case but Ks = 128.  `mt1` without its clip and `smp > n` for `smp >= n` change no output (the extra
tile's and the extra sample's rows of D are loaded as 0), so nothing here sees them."""
import ctypes as C

import numpy as np
import pytest
import torch

from locator_amd import _lib
from tests import explain_util as XU
from tests.explain_util import CAP_STACK, CAP_STATS, MARGIN_STACK, MARGIN_STATS

pytestmark = pytest.mark.gpu


def _held(case, what, got, F, margin, cap):
    """got and F: (tensor / statistic L2, worst row / site).  Prints the ratios, then asserts the floor rule."""
    assert XU.floor_ok(F, margin, cap), (case, what, F)
    print(f"explain_kernels {case} {what}: " + ", ".join(f"{name} {g:.3e} / F {f:.3e} = {g / f:.2f}"
                                                           for name, g, f in zip(("l2", "worst"), got, F)))
    for name, g, f in zip(("l2", "worst"), got, F):
        assert g <= margin * f, (case, what, name, g, f, g / f)


# ------------------------------------------------------------------ loc_explain_stack_grad
@pytest.mark.parametrize("case", XU.STACK_CASES, ids=str)
def test_stack_grad_per_layer_on_guarded_buffers(case):
    lib = _lib.load()
    n, H, L = case
    prob = XU.stack_problem(*case)
    a64, d64, F = XU.stack_refs(prob)
    acts, d1 = XU.run_stack(lib, prob, "nan")
    acts_j, d1_j = XU.run_stack(lib, prob, "junk", seed=1)
    # every element written, none read before it was: NaN nowhere, and the junk-poisoned run gives the same bits
    assert not np.isnan(d1).any() and not np.isnan(acts).any()
    assert d1.tobytes() == d1_j.tobytes() and acts.tobytes() == acts_j.tobytes()
    assert acts.shape == (L - 1, n, prob["Hp"]) and d1.shape == (n, 2, prob["Hp"])
    assert not d1[:, :, H:].any(), "columns H .. Hp of delta1 have to be exactly 0"
    assert not acts[:, :, H:].any(), "columns H .. Hp of acts have to be exactly 0"
    if L > 1:
        per_layer = [XU.tensor_err(acts[l, :, :H], a64[l]) for l in range(L - 1)]
        _held(case, "acts", tuple(max(e) for e in zip(*per_layer)), F["acts"], MARGIN_STACK, CAP_STACK)
    _held(case, "delta1", XU.tensor_err(d1[:, :, :H], d64), F["delta1"], MARGIN_STACK, CAP_STACK)


# ------------------------------------------------------------------ loc_explain_sites + loc_explain_reduce
@pytest.mark.parametrize("case", XU.SITES_CASES, ids=str)
def test_sites_with_every_accepted_split_count(case):
    lib = _lib.load()
    n, Ks = case[0], case[1]
    prob = XU.sites_problem(*case)
    absent = prob["absent"]
    counts = XU.accepted_splits(n)
    assert counts[0] == 1 and counts[-1] == XU.mt_of(n) and (n != 300 or counts == [1, 2, 3, 5])
    outs = {}
    for splits in counts:
        per_split, (o64, F_out) = XU.sites_refs(prob, splits)
        partial, out = XU.run_sites(lib, prob, splits, "nan")
        partial_j, out_j = XU.run_sites(lib, prob, splits, "junk", seed=1)
        # every element written, none read before it was; two runs with one split count are bit-identical
        assert not np.isnan(partial).any() and not np.isnan(out).any()
        assert partial.tobytes() == partial_j.tobytes() and out.tobytes() == out_j.tobytes()
        assert not partial[:, :, absent].any() and not out[:, absent].any(), "an all-zero row of U gives exactly 0"
        assert (partial[:, :, ~absent] > 0).all() and (out[:, ~absent] > 0).all()
        for sp, (p64, F) in enumerate(per_split):
            _held(case, f"splits {splits} partial[{sp}] samples {XU.split_range(n, splits, sp)}",
                  XU.stats_err(partial[sp], p64), F, MARGIN_STATS, CAP_STATS)
        _held(case, f"splits {splits} out", XU.stats_err(out, o64), F_out, MARGIN_STATS, CAP_STATS)
        outs[splits] = out
    for splits in counts[1:]:
        a, b = outs[1], outs[splits]
        assert (np.abs(a - b) <= 2 * n * 2.0 ** -52 * np.maximum(a, b)).all(), (case, splits, np.abs(a - b).max())


@pytest.mark.parametrize("case", XU.SITES_CASES, ids=str)
def test_sites_row_pitch_and_pad_columns_do_not_matter(case):
    """xs_pitch = Ks, Ks + 1 and Ks rounded up to 64 plus 64; the pad columns seeded random bytes, then the constant 2: the
    same bits as at pitch Ks."""
    lib = _lib.load()
    n, Ks = case[0], case[1]
    prob = XU.sites_problem(*case)
    counts = XU.accepted_splits(n)
    splits = counts[len(counts) // 2]
    want = XU.run_sites(lib, prob, splits, "nan")
    for pitch in (Ks + 1, (Ks + 63) // 64 * 64 + 64):
        for pad in ("random", "two"):
            got = XU.run_sites(lib, prob, splits, "junk", seed=pitch, pitch=pitch, pad=pad)
            assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), (case, pitch, pad)


# ------------------------------------------------------------------ refusals
def test_refusals_return_minus_one_name_themselves_and_launch_nothing():
    lib = _lib.load()
    dev = "cuda"
    n, Ks, Hp = 300, 8, 32                                   # mt = 5
    f32 = lambda count: torch.full((count,), 7.5, dtype=torch.float32, device=dev)
    a1, wh, bh, wa, wb = f32(n * Hp), f32(Hp * Hp), f32(Hp), f32(2 * Hp), f32(4)
    U, mm = f32(Ks * Hp), f32(Ks)
    Xs = torch.ones((n, Ks), dtype=torch.uint8, device=dev)
    acts, g, delta1 = f32(n * Hp), f32(2 * n * Hp), f32(2 * n * Hp)
    partial = torch.full((6 * 4 * Ks,), -3.25, dtype=torch.float64, device=dev)
    out = torch.full((4 * Ks,), -3.25, dtype=torch.float64, device=dev)
    outputs = (acts, g, delta1, partial, out)
    before = [t.clone() for t in outputs]
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    big = 2 ** 29 + 1

    def stack(n_=n, Hp_=Hp, L_=2, acts_=acts, g_=g):
        return lib.loc_explain_stack_grad(p(a1), n_, Hp_, L_, p(wh), p(bh), p(wa), p(wb), 2.5, 1.5, p(acts_), p(g_),
                                          p(delta1), st)

    def sites(n_=n, Ks_=Ks, Hp_=Hp, pitch_=Ks, splits_=1):
        return lib.loc_explain_sites(p(delta1), n_, p(U), Ks_, Hp_, p(Xs), pitch_, p(mm), splits_, p(partial), st)

    def reduce_(splits_=1, Ks_=Ks, n_=n):
        return lib.loc_explain_reduce(p(partial), splits_, Ks_, n_, p(out), st)

    bad_hp = (0, 16, 48, 1056)
    calls = ([("loc_explain_stack_grad", lambda kw=kw: stack(**kw), kw) for kw in
              [{"n_": 0}, {"n_": big}, {"L_": 0}, {"acts_": None}, {"g_": None}] + [{"Hp_": h} for h in bad_hp]]
             + [("loc_explain_sites", lambda kw=kw: sites(**kw), kw) for kw in
                [{"n_": 0}, {"n_": big}, {"Ks_": 0}, {"pitch_": Ks - 1}, {"splits_": 0}, {"splits_": 6}, {"splits_": 4}]
                + [{"Hp_": h} for h in bad_hp]]
             + [("loc_explain_reduce", lambda kw=kw: reduce_(**kw), kw) for kw in
                [{"splits_": 0}, {"Ks_": 0}, {"n_": 0}]])
    assert len(calls) == 9 + 11 + 3
    for name, call, kw in calls:
        assert call() == -1, (name, kw)
        assert name.encode() in lib.loc_last_error(), (name, kw, lib.loc_last_error())
    torch.cuda.synchronize()
    for t, b in zip(outputs, before):
        assert torch.equal(t, b), "a refused call wrote to an output buffer"
    # the same buffers are fine with good arguments: the refusals above were about the arguments
    assert stack() == 0 and sites(splits_=5) == 0 and reduce_(splits_=5) == 0, lib.loc_last_error()
    torch.cuda.synchronize()
