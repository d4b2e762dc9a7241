"""The per-layer hidden kernels at kernel level: loc_dense_forward, loc_dense_backward, loc_head_train and loc_head_eval
(locator_amd/csrc/stack_kernels.hip) called directly through the C ABI, at every unit-tile count NHT = Hp / 32 = 1..32 that
NHT_SWITCH instantiates.  train_step_impl and loc_predict take this route for every --width that does not pad to 64, 128,
256 or 512, for --nlayers 1 and for C callers without wht (locator.py:319-325, :314-315).

The memory contract these tests state (include/locator_hip.h):
  loc_dense_forward   all 32 rows of `in` are read, all 32 rows of `out` written; padded units stay exactly 0; out_drop is
                      written with a mask only and is the single fp32 product out * (mask ? keep_scale : 0)
  loc_dense_backward  a half is given in full or not at all and the skipped half writes nothing; the dW half contracts all
                      32 rows: dz2 rows >= n_b EXACTLY 0, in2 rows >= n_b finite (then their values change nothing); the
                      padded rows and columns of W2 / mW2 / vW2 stay exactly 0
  loc_head_train      `a` rows >= n_b finite (their values change nothing); dz_last rows >= n_b come back exactly 0; of the
                      flat m / v only the four head slices are written; distance 0 -> gradient 0
  loc_head_eval       rows >= n_b of yhat / dist are not written; no dist without targets
  all four            Hp that is no multiple of 32 in 32..1024 (heads: n_b outside 1..32) -> nonzero, a message, nothing
                      written
Every caller buffer is a guarded view of exactly the documented size, poisoned before the call.

The reference is plain NumPy in float64 (_ref_stack / _ref_grads of tests/test_gpu_stack_train.py for the heads, the three
single-layer functions below for the Dense kernels); the same functions in float32 give the floors: F per tensor, F_row per
row, F_tile per 32 x 32 tile of a kernel and per 32 entries of a bias.  The device may be MARGIN (the heads:
HEAD_MARGIN) times as far and never more than CAP; weights after the Adam step within 1e-5 and the loss within 2e-5, the
bars of test_one_training_step_matches_oracle.  The comparison functions (_judge, _judge_step) are the ones
test_the_comparison_flags_what_these_kernels_could_get_wrong feeds perturbed references to, without a GPU."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import locator_oracle as O
from tests.gpu_util import (_rel, bits, build_net, guarded, make_problem, maxerr, moments_err, poison, replay_epoch,
                            tile_norms)
from tests.test_gpu_stack_train import _distances, _elu_grad, _problem, _ref_grads, _ref_stack

# The device over the float32 reference's own distance from float64 (it sums in another order, fuses multiply-adds and uses
# the hardware's exp).  Every case prints device / F for each of its floors (pytest -s) and the largest so far of its group.
# Measured on an MI355X, each margin about twice the largest ratio of its group, rounded up:
#   the Dense kernels, 64 forward and 128 backward cases: forward 0.40..0.74 per tensor, 0.36..0.71 per row; dx 0.38..1.13 /
#   0.37..1.00 (one tile, with the mask); dW + Adam moments 0.66..1.00 per tensor, 0.59..1.03 per tile (NHT 16, v of b2)
#   -> MARGIN 3
#   the heads, 52 cases: moments of the step 0.25..1.86 per tensor, 0.31..2.02 per tile (Hp 96, one row); yhat / dist
#   0.08..2.93 (Hp 512, one row); dz_last 0.68..4.39 (Hp 1024, one row) -> HEAD_MARGIN 9.
#   The dz_last ratios above 1.3 all belong to batches of one or two rows: there dz_last = dy1 Wa^T carries the rounding of
#   the two numbers dy1 of a row after the cancellation e = y2 - y, and the float32 reference happens to be 3.8e-8 to 6e-8
#   from float64 - half an fp32 ulp - where the device is 1.6e-7 to 2.5e-7, 1.4 to 2 ulp.  At 31 and 32 rows
#   loc_head_train stays below 1.3.
MARGIN = 3.0
HEAD_MARGIN = 9.0
STACK_TRAIN_MARGIN = 4.0        # tests/test_gpu_stack_train.py: the perturbations have to be flagged at this margin as well
CAP = 1e-3
DROP_P = 0.25
KS = float(np.float32(1.0) / (np.float32(1.0) - np.float32(DROP_P)))
K = 40
N_Y = 50                        # target rows the heads index through `rows`

_f32 = lambda a: np.asarray(a).astype(np.float32).astype(np.float64)
_WORST = {}


def _note(group, ratio):
    _WORST[group] = max(_WORST.get(group, 0.0), float(ratio))
    return _WORST[group]


# ------------------------------------------------------------------ the single-layer references
def _ref_dense_fwd(x, W, b, dt):
    """ELU(x W + b) in dtype dt."""
    return O.elu(np.asarray(x, dt) @ np.asarray(W, dt) + np.asarray(b, dt))


def _ref_dense_dx(dz, W, a_prev, mask, dt):
    """(dz W^T) * keep * ELU'(a_prev) in dtype dt; mask: keep flags or None."""
    da = np.asarray(dz, dt) @ np.asarray(W, dt).T
    if mask is not None:
        da = da * (mask.astype(dt) * dt(1.0 / (1.0 - DROP_P)))
    return da * _elu_grad(np.asarray(a_prev, dt))


def _ref_dw_step(in2, dz2, W2, b2, dt, grad_hook=None):
    """dW2 = in2^T dz2, db2 = sum_b dz2 and Adam step 1 from zero moments at lr 1e-3, in dtype dt.
    -> (params, m, v) in the oracle's format with one kernel and one bias (gamma / beta: one unused zero)."""
    z = lambda: np.zeros(1, dt)
    p = {"gamma": z(), "beta": z(), "W": [np.array(W2, dt)], "b": [np.array(b2, dt)]}
    g = {"gamma": z(), "beta": z(), "W": [np.asarray(in2, dt).T @ np.asarray(dz2, dt)], "b": [np.asarray(dz2, dt).sum(0)]}
    if grad_hook is not None:
        grad_hook(g)
    m, v = O.zeros_like_trainable(p), O.zeros_like_trainable(p)
    O.adam_apply(p, g, m, v, 1, dt(1e-3))
    return p, m, v


# ------------------------------------------------------------------ the comparison
def _judge(got, ref64, ref32, margin, label, group=None):
    """{name: 2-D array} of the device (or of a perturbed reference) against the float64 reference, the float32 reference's
    distance as the floor, per tensor and per row.  -> the list of violations (empty: passes)."""
    ft, fr = _distances(ref32, ref64)
    F, F_row = max(ft.values()), max(fr.values())
    assert 0 < F and margin * F < CAP and 0 < F_row and margin * F_row < CAP, (label, F, F_row)
    dt, dr = _distances(got, ref64)
    kt, kr = max(dt, key=dt.get), max(dr, key=dr.get)
    if group is not None:
        wt, wr = _note(group + " per tensor", dt[kt] / F), _note(group + " per row", dr[kr] / F_row)
        print(f"{label}: F {F:.2e} device {dt[kt]:.2e} ({kt}) ratio {dt[kt] / F:.2f} | F_row {F_row:.2e} device "
              f"{dr[kr]:.2e} ({kr}) ratio {dr[kr] / F_row:.2f} | largest so far in {group}: {wt:.2f} / {wr:.2f}")
    fails = []
    if not dt[kt] <= margin * F:
        fails.append(f"{label}: {kt} is {dt[kt]:.3e} from float64, {margin} x F = {margin * F:.3e}")
    if not dr[kr] <= margin * F_row:
        fails.append(f"{label}: a row of {kr} is {dr[kr]:.3e} from float64, {margin} x F_row = {margin * F_row:.3e}")
    return fails


def _moment_dists(m, v, m64, v64):
    """-> {moment.tensor: relative L2 distance}, {moment.tensor: the worst over 32 x 32 tiles (kernels) / 32 entries
    (biases)}."""
    per_tensor, per_tile = {}, {}
    for name, g, r in (("m", m, m64), ("v", v, v64)):
        t, tt = moments_err(g, r)
        for l in range(len(r["b"])):          # one workgroup owns 32 entries of a bias: the kt == 0 tile of its column
            gb, rb = np.asarray(g["b"][l], np.float64)[None, :], np.asarray(r["b"][l], np.float64)[None, :]
            tt[f"b{l}"] = float(_rel(tile_norms(gb - rb), tile_norms(rb)).max())
        per_tensor.update({f"{name}.{k}": e for k, e in t.items()})
        per_tile.update({f"{name}.{k}": e for k, e in tt.items()})
    return per_tensor, per_tile


def _judge_step(got, s64, s32, margin, label, layers, group=None):
    """(params, m, v) after one Adam step in the oracle's format: the kernels and biases `layers` within 1e-5 of the float64
    step, the moments within margin x the float32 step's distance per tensor and per tile.  -> the list of violations."""
    ft, ftt = _moment_dists(s32[1], s32[2], s64[1], s64[2])
    F, F_tile = max(ft.values()), max(ftt.values())
    assert 0 < F and margin * F < CAP and 0 < F_tile and margin * F_tile < CAP, (label, F, F_tile)
    dt, dtt = _moment_dists(got[1], got[2], s64[1], s64[2])
    kt, kk = max(dt, key=dt.get), max(dtt, key=dtt.get)
    if group is not None:
        wt, wk = _note(group + " per tensor", dt[kt] / F), _note(group + " per tile", dtt[kk] / F_tile)
        print(f"{label}: F {F:.2e} device {dt[kt]:.2e} ({kt}) ratio {dt[kt] / F:.2f} | F_tile {F_tile:.2e} device "
              f"{dtt[kk]:.2e} ({kk}) ratio {dtt[kk] / F_tile:.2f} | largest so far in {group}: {wt:.2f} / {wk:.2f}")
    fails = []
    for l in layers:
        for name in ("W", "b"):
            e = maxerr(got[0][name][l], s64[0][name][l])
            if not e < 1e-5:
                fails.append(f"{label}: {name}{l} after the step is {e:.3e} from float64")
    if not dt[kt] <= margin * F:
        fails.append(f"{label}: {kt} is {dt[kt]:.3e} from float64, {margin} x F = {margin * F:.3e}")
    if not dtt[kk] <= margin * F_tile:
        fails.append(f"{label}: a tile of {kk} is {dtt[kk]:.3e} from float64, {margin} x F_tile = {margin * F_tile:.3e}")
    return fails


# ------------------------------------------------------------------ one Dense layer pair on the host
def _pad(a, shape):
    out = np.zeros(shape, np.float64)
    out[tuple(slice(0, n) for n in a.shape)] = a
    return out


@functools.lru_cache(maxsize=2)
def _layer_case(nht):
    """Tile count nht: width 32 * nht (odd nht) or 32 * nht - 7 (even: padded units exist), every array padded to Hp with
    zeros and fp32-representable.  Layer `W` (forward, dx) and the layer above it, `W2` (dW + Adam), as api.hip pairs them
    in one backward launch; n_b of the dW half spread over the tile counts."""
    width = 32 * nht if nht % 2 else 32 * nht - 7
    Hp, n_b = 32 * nht, (1, 31, 32)[nht % 3]
    p, a1, _, rng = _problem(width, 3, 32, seed=100 + nht, K=K)
    c = SimpleNamespace(nht=nht, width=width, Hp=Hp, n_b=n_b)
    c.inp = _pad(a1, (32, Hp))                                       # ELU outputs of the layer below: `in` and `a_prev`
    c.W, c.b = _pad(p["W"][1], (Hp, Hp)), _pad(p["b"][1], (Hp,))
    c.W2, c.b2 = _pad(p["W"][2], (Hp, Hp)), _pad(p["b"][2], (Hp,))
    c.mask = (rng.random((32, Hp)) >= DROP_P).astype(np.uint8)
    c.dz = _pad(_f32(rng.normal(0, 1 / 32, (32, width))), (32, Hp))
    c.in2 = _pad(_f32(O.elu(rng.normal(0, 1, (32, width)))), (32, Hp))
    dz2 = _f32(rng.normal(0, 1 / 32, (32, width)))
    dz2[n_b:] = 0
    c.dz2 = _pad(dz2, (32, Hp))
    c.fwd = functools.lru_cache(None)(lambda dt: {"out": _ref_dense_fwd(c.inp, c.W, c.b, dt)})
    c.dx = functools.lru_cache(None)(
        lambda dt, drop: {"dz_prev": _ref_dense_dx(c.dz, c.W, c.inp, c.mask if drop else None, dt)})
    c.dw = functools.lru_cache(None)(lambda dt: _ref_dw_step(c.in2, c.dz2, c.W2, c.b2, dt))
    return c


# ------------------------------------------------------------------ the heads on the host
HEAD_WIDTH = {32: 32, 96: 89, 512: 512, 544: 537, 1024: 1017}      # Hp -> width: two of them with padded units


def _head_case(Hp, n_b, seed, zero_row=None):
    """Dense(2) -> Dense(2) -> loss on n_b rows of `a` (an --nlayers 1 problem: _ref_stack with no hidden layer), the
    targets reached through `rows` into N_Y rows of Y.  zero_row: Wa = 0, ba = 0 and that row's target = bb, so that its
    y2 equals its target exactly.  Both references and their Adam step 1: refs[name] = (_ref_stack's output, params, m,
    v)."""
    width = HEAD_WIDTH[Hp]
    p, a1, y, rng = _problem(width, 1, n_b, seed, K=K)
    Y = _f32(rng.normal(0, 1, (N_Y, 2)))
    rows = rng.permutation(N_Y)[:32].astype(np.int32)
    if zero_row is not None:
        p["W"][1][:] = 0
        p["b"][1][:] = 0
        y[zero_row] = p["b"][2]
    Y[rows[:n_b]] = y
    h = SimpleNamespace(Hp=Hp, width=width, n_b=n_b, p=p, a1=a1, y=y, Y=Y, rows=rows, refs={})
    for name, dt in (("f64", np.float64), ("f32", np.float32)):
        pc = O.cast_params(p, dt)
        r = _ref_stack(pc, a1, None, y, DROP_P)
        pp = O.copy_params(pc)
        m, v = O.zeros_like_trainable(pp), O.zeros_like_trainable(pp)
        O.adam_apply(pp, _ref_grads(pc, r), m, v, 1, dt(1e-3))
        h.refs[name] = (r, pp, m, v)
    return h


def _head_eval_ref(h, dt):
    pc = O.cast_params(h.p, dt)
    y2 = (np.asarray(h.a1, dt) @ pc["W"][1] + pc["b"][1]) @ pc["W"][2] + pc["b"][2]
    return {"yhat": y2, "dist": O.euclid(y2, np.asarray(h.y, dt))[:, None]}


# ------------------------------------------------------------------ no GPU: the floors and the comparison itself
def test_floors_leave_room_below_the_cap():
    """0 < F and MARGIN x F < CAP for the smallest and the largest case of every group: a condition on the inputs."""
    for nht in (1, 32):
        c = _layer_case(nht)
        assert not _judge(c.fwd(np.float32), c.fwd(np.float64), c.fwd(np.float32), MARGIN, f"forward {nht}")
        for drop in (False, True):
            assert not _judge(c.dx(np.float32, drop), c.dx(np.float64, drop), c.dx(np.float32, drop), MARGIN, f"dx {nht}")
        assert not _judge_step(c.dw(np.float32), c.dw(np.float64), c.dw(np.float32), MARGIN, f"dw {nht}", [0])
    for Hp, n_b in ((32, 1), (1024, 32)):
        h = _head_case(Hp, n_b, seed=Hp + n_b)
        (r64, *s64), (r32, *s32) = h.refs["f64"], h.refs["f32"]
        dz32 = {"dz_last": r32["dz"][0]}
        assert not _judge(dz32, {"dz_last": r64["dz"][0]}, dz32, HEAD_MARGIN, "head")
        assert not _judge_step(s32, s64, s32, HEAD_MARGIN, f"head {Hp}", [1, 2])
        assert abs(r32["loss"] - r64["loss"]) < 2e-5
        e32 = _head_eval_ref(h, np.float32)
        assert not _judge(e32, _head_eval_ref(h, np.float64), e32, HEAD_MARGIN, f"head eval {Hp}")


@pytest.mark.parametrize("nht", [1, 6, 32])
def test_the_comparison_flags_what_these_kernels_could_get_wrong(nht):
    """The float64 reference perturbed in the ways these kernels could be wrong is refused by _judge / _judge_step at the
    margin of tests/test_gpu_stack_train.py and at this module's own, on the float32 floors: one 32 x 32 tile of dW x 0.9,
    one group of 8 k dropped from one output tile of the forward sum, two batch rows swapped in dz_prev, the bias gradient
    without one row, the dropout scale applied twice.  The unperturbed float32 reference passes."""
    c = _layer_case(nht)
    f64, f32 = np.float64, np.float32
    kt, nt = (c.width - 1) // 32, nht // 2                           # the last (partial, where the width is padded) k-tile

    def tile_scaled(g):
        g["W"][0][32 * kt:32 * kt + 32, 32 * nt:32 * nt + 32] *= 0.9

    def bias_short_of_a_row(g):
        g["b"][0] -= c.dz2[c.n_b - 1]

    k0, n0 = 8 * (2 * nht), 32 * (nht - 1)                            # a group of 8 real k, the last output tile
    z = c.inp @ c.W + c.b
    z[:, n0:n0 + 32] -= c.inp[:, k0:k0 + 8] @ c.W[k0:k0 + 8, n0:n0 + 32]
    swapped = c.dx(f64, False)["dz_prev"].copy()
    swapped[[3, 4]] = swapped[[4, 3]]
    twice = c.dx(f64, True)["dz_prev"] * np.where(c.mask > 0, 1.0 / (1.0 - DROP_P), 0.0)
    for margin in sorted({STACK_TRAIN_MARGIN, MARGIN, HEAD_MARGIN}):
        step = lambda hook: _judge_step(_ref_dw_step(c.in2, c.dz2, c.W2, c.b2, f64, hook), c.dw(f64), c.dw(f32), margin,
                                        "dw", [0])
        assert any("tile" in f for f in step(tile_scaled))
        assert any(".b0" in f for f in step(bias_short_of_a_row))
        assert not step(None) and not _judge_step(c.dw(f32), c.dw(f64), c.dw(f32), margin, "dw", [0])
        assert len(_judge({"out": O.elu(z)}, c.fwd(f64), c.fwd(f32), margin, "forward")) == 2
        assert _judge({"dz_prev": swapped}, c.dx(f64, False), c.dx(f32, False), margin, "dx")
        assert len(_judge({"dz_prev": twice}, c.dx(f64, True), c.dx(f32, True), margin, "dx")) == 2
        assert not _judge(c.fwd(f32), c.fwd(f64), c.fwd(f32), margin, "forward")
        assert not _judge(c.dx(f32, True), c.dx(f64, True), c.dx(f32, True), margin, "dx")


# ------------------------------------------------------------------ the device side
@functools.lru_cache(maxsize=1)
def _plumbing():
    """A LocatorNet for the library handle, the Adam alpha table, lr and the step counter (t_base = 0: t_off 1 is step 1)."""
    x, y, p, _ = make_problem(8, K, 32, 2, seed=1)
    return build_net(x, y, p, drop_p=0.0)


def _adam_args(net):
    from locator_amd.net import ALPHA_TAB_LEN
    return net.alpha_tab.data_ptr(), ALPHA_TAB_LEN, net.lr_t.data_ptr(), net.t_base_t.data_ptr(), 1


class _Bufs:
    """Caller buffers as guarded views of exactly n elements (float32, or (n, dtype)), margins of 128 * Hp floats."""

    def __init__(self, Hp, **sizes):
        self.t, self.checks = {}, []
        for name, n in sizes.items():
            n, dtype = n if isinstance(n, tuple) else (n, torch.float32)
            self.t[name], chk = guarded(n, dtype, 128 * Hp * (4 if dtype == torch.uint8 else 1))
            self.checks.append((name, chk))

    def poison(self, kind):
        for i, t in enumerate(self.t.values()):
            poison(t, "nan" if t.dtype == torch.int32 else kind, 11 + i)      # row indices: -1 either way

    def put(self, name, a):
        t = self.t[name]
        src = torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(t.dtype)
        assert src.numel() == t.numel(), (name, src.numel(), t.numel())
        t.copy_(src)

    def ptr(self, name):
        return self.t[name].data_ptr()

    def snap(self):
        torch.cuda.synchronize()
        return {k: bits(t) for k, t in self.t.items()}

    def get(self, name, *shape):
        return self.t[name].cpu().numpy().reshape(shape)

    def check_margins(self):
        for name, chk in self.checks:
            chk(name)


def _unchanged(before, after, names):
    for k in names:
        assert torch.equal(after[k], before[k]), f"{k}: {int((after[k] != before[k]).sum())} words written"


# ------------------------------------------------------------------ loc_dense_forward
@pytest.mark.gpu
@pytest.mark.parametrize("nht,drop", [(n, d) for n in range(1, 33) for d in (False, True)],
                         ids=[f"nht{n}-{'mask' if d else 'nomask'}" for n in range(1, 33) for d in (False, True)])
def test_dense_forward_at_every_tile_count(nht, drop):
    """All 32 rows of out against the float64 reference per tensor and per row; padded units exactly 0; in, W, b and the
    mask bit-unchanged; out_drop the fp32 product of the device's own out with the keep scale, or - without a mask - its
    poison."""
    c, lib = _layer_case(nht), _plumbing().lib
    Hp = c.Hp
    kind = ("nan", "junk")[(nht + drop) % 2]
    B = _Bufs(Hp, inp=32 * Hp, W=Hp * Hp, b=Hp, out=32 * Hp, out_drop=32 * Hp, mask=(32 * Hp, torch.uint8))
    B.poison(kind)
    for name in ("inp", "W", "b"):
        B.put(name, getattr(c, name))
    if drop:
        B.put("mask", c.mask)
    before = B.snap()
    rc = lib.loc_dense_forward(B.ptr("inp"), B.ptr("W"), B.ptr("b"), Hp, B.ptr("out"), B.ptr("out_drop"),
                               B.ptr("mask") if drop else None, KS if drop else 1.0, None)
    assert rc == 0, lib.loc_last_error()
    after = B.snap()
    B.check_margins()
    _unchanged(before, after, ("inp", "W", "b", "mask") + (() if drop else ("out_drop",)))
    out = B.get("out", 32, Hp)
    fails = _judge({"out": out}, c.fwd(np.float64), c.fwd(np.float32), MARGIN, f"forward nht {nht} mask {drop}", "forward")
    assert not fails, fails
    assert not out[:, c.width:].any(), "a padded unit is not exactly 0"
    if drop:
        want = out * np.where(c.mask > 0, np.float32(KS), np.float32(0))
        assert want.dtype == np.float32
        assert np.array_equal(B.get("out_drop", 32, Hp).view(np.int32), want.view(np.int32)), "out_drop is not out * keep"


# ------------------------------------------------------------------ loc_dense_backward
BWD_FORMS = ("dx", "dx-mask", "dw", "both")
_DW_BUFS = ("in2", "dz2", "W2", "mW2", "vW2", "b2", "mb2", "vb2")


def _backward(c, form, kind, in2_pad="zero"):
    """One loc_dense_backward launch on fresh guarded buffers.  form: which halves are given; in2_pad: rows >= n_b of in2 as
    zeros or as finite junk.  -> (buffers, bits before, bits after)."""
    net = _plumbing()
    Hp, dx, dw = c.Hp, form != "dw", form in ("dw", "both")
    drop = form == "dx-mask" or (form == "both" and c.nht % 2 == 1)
    B = _Bufs(Hp, dz=32 * Hp, W=Hp * Hp, a_prev=32 * Hp, mask=(32 * Hp, torch.uint8), dz_prev=32 * Hp, in2=32 * Hp,
              dz2=32 * Hp, W2=Hp * Hp, mW2=Hp * Hp, vW2=Hp * Hp, b2=Hp, mb2=Hp, vb2=Hp)
    B.poison(kind)
    if dx:
        for name, a in (("dz", c.dz), ("W", c.W), ("a_prev", c.inp)):
            B.put(name, a)
        if drop:
            B.put("mask", c.mask)
    if dw:
        for name, a in (("in2", c.in2), ("dz2", c.dz2), ("W2", c.W2), ("b2", c.b2)):
            B.put(name, a)
        for name in ("mW2", "vW2", "mb2", "vb2"):
            B.t[name].zero_()
        if c.n_b < 32:
            poison(B.t["in2"].view(32, Hp)[c.n_b:], in2_pad, 77)
    before = B.snap()
    P = lambda name, given: B.ptr(name) if given else None
    rc = net.lib.loc_dense_backward(P("dz", dx), P("W", dx), P("a_prev", dx), P("mask", dx and drop), KS if drop else 1.0,
                                    P("dz_prev", dx), *(P(name, dw) for name in _DW_BUFS), Hp, *_adam_args(net), None)
    assert rc == 0, net.lib.loc_last_error()
    after = B.snap()
    B.check_margins()
    written = (("dz_prev",) if dx else ()) + (("W2", "mW2", "vW2", "b2", "mb2", "vb2") if dw else ())
    _unchanged(before, after, [k for k in B.t if k not in written])
    return B, drop


def _dw_outputs(B, Hp):
    z = np.zeros(1, np.float32)
    return tuple({"gamma": z, "beta": z, "W": [B.get(w, Hp, Hp)], "b": [B.get(b, Hp)]}
                 for w, b in (("W2", "b2"), ("mW2", "mb2"), ("vW2", "vb2")))


@pytest.mark.gpu
@pytest.mark.parametrize("nht,form", [(n, f) for n in range(1, 33) for f in BWD_FORMS],
                         ids=[f"nht{n}-{f}" for n in range(1, 33) for f in BWD_FORMS])
def test_dense_backward_at_every_tile_count(nht, form):
    """dx alone (with and without the mask), dW + Adam alone, and both in one launch on distinct layers: dz_prev against
    (dz W^T) * keep * ELU'(a_prev) per tensor and per row; W2, b2 and their moments after Adam step 1 from zero moments per
    tensor, per 32 x 32 tile and per 32 entries of the bias; padding exactly 0; every input and the skipped half's buffers
    bit-unchanged; junk in rows >= n_b of in2 changes no value."""
    c = _layer_case(nht)
    Hp, width = c.Hp, c.width
    kind = ("nan", "junk")[(nht + BWD_FORMS.index(form)) % 2]
    B, drop = _backward(c, form, kind)
    label = f"backward nht {nht} {form} n_b {c.n_b}"
    if form != "dw":
        dzp = B.get("dz_prev", 32, Hp)
        fails = _judge({"dz_prev": dzp}, c.dx(np.float64, drop), c.dx(np.float32, drop), MARGIN, label, "dx")
        assert not fails, fails
        assert not dzp[:, width:].any(), "dz_prev of a padded unit is not exactly 0"
    if form in ("dw", "both"):
        got = _dw_outputs(B, Hp)
        fails = _judge_step(got, c.dw(np.float64), c.dw(np.float32), MARGIN, label, [0], "dw")
        assert not fails, fails
        for d in got:
            assert not d["W"][0][width:].any() and not d["W"][0][:, width:].any() and not d["b"][0][width:].any(), \
                "padding of W2 / b2 or of their moments is not exactly 0"
        if form == "dw" and c.n_b < 32:
            B2, _ = _backward(c, form, kind, in2_pad="junk")
            for a, b in zip(got, _dw_outputs(B2, Hp)):
                assert np.array_equal(a["W"][0], b["W"][0]) and np.array_equal(a["b"][0], b["b"][0]), \
                    "the dW half depends on rows >= n_b of in2"


# ------------------------------------------------------------------ the heads
class _Head:
    """One head problem on the device: a LocatorNet (--nlayers 1) for the parameter layout and the import, the flat params /
    m / v and every other caller buffer as guarded views.  Of m and v only the four head slices start at 0; the rest holds
    poison."""

    def __init__(self, h, kind):
        self.h, self.kind = h, kind
        self.net = net = build_net(np.zeros((N_Y, K), np.uint8), h.Y, h.p, drop_p=0.0)
        lay, d = net.lay, net.d
        assert d.Hp == h.Hp and d.L == 1
        Hp = h.Hp
        self.slices = [(lay.wa, 2 * Hp), (lay.ba, 2), (lay.wb, 4), (lay.bb, 2)]
        self.B = _Bufs(Hp, a=32 * Hp, params=lay.n_total, m=lay.n_trainable, v=lay.n_trainable, dz_last=32 * Hp, loss=1,
                       rows=(32, torch.int32), yhat=64, dist=32)

    def fill(self, pad="zero", a_pad_kind=None):
        h, B, Hp = self.h, self.B, self.h.Hp
        B.poison(self.kind)
        B.t["params"].copy_(self.net.params)
        for name in ("m", "v"):
            for off, n in self.slices:
                B.t[name][off:off + n] = 0
        a = B.t["a"].view(32, Hp)
        a[:h.n_b] = torch.from_numpy(_pad(h.a1, (h.n_b, Hp)).astype(np.float32)).cuda()
        if h.n_b < 32 and pad is not None:
            poison(a[h.n_b:], pad, 78)
        rows = np.full(32, -1, np.int32)
        rows[:h.n_b] = h.rows[:h.n_b]
        B.put("rows", rows)
        return B.snap()

    def head_ptrs(self):
        P, lay = self.B.ptr("params"), self.net.lay
        return P + 4 * lay.wa, P + 4 * lay.ba, P + 4 * lay.wb, P + 4 * lay.bb

    def train(self, n_b=None, Hp=None):
        B, net, lay = self.B, self.net, self.net.lay
        rc = net.lib.loc_head_train(B.ptr("a"), self.h.Hp if Hp is None else Hp, self.h.n_b if n_b is None else n_b,
                                    B.ptr("rows"), net.Y.data_ptr(), *self.head_ptrs(), B.ptr("m"), B.ptr("v"), lay.wa,
                                    lay.ba, lay.wb, lay.bb, B.ptr("dz_last"), B.ptr("loss"), *_adam_args(net), None)
        torch.cuda.synchronize()
        return rc

    def eval(self, targets, n_b=None, Hp=None):
        B, net = self.B, self.net
        rc = net.lib.loc_head_eval(B.ptr("a"), self.h.Hp if Hp is None else Hp, self.h.n_b if n_b is None else n_b,
                                   *self.head_ptrs(), B.ptr("yhat"), B.ptr("rows") if targets else None,
                                   net.Y.data_ptr() if targets else None, B.ptr("dist") if targets else None, None)
        torch.cuda.synchronize()
        return rc

    def step(self, name):
        """(params, m, v) of the device in the oracle's format, layer 1 and BatchNorm as zeros (the heads do not own
        them)."""
        h, lay, Hp = self.h, self.net.lay, self.h.Hp
        f = self.B.get(name, -1)
        return {"gamma": np.zeros(K, np.float32), "beta": np.zeros(K, np.float32),
                "W": [np.zeros((K, h.width), np.float32), f[lay.wa:lay.wa + 2 * Hp].reshape(Hp, 2)[:h.width],
                      f[lay.wb:lay.wb + 4].reshape(2, 2)],
                "b": [np.zeros(h.width, np.float32), f[lay.ba:lay.ba + 2], f[lay.bb:lay.bb + 2]]}

    def only_the_head_slices_written(self, before, after):
        """params, m, v: no bit outside wa, ba, wb, bb changed; the padded rows of Wa and of its moments still exactly 0."""
        lay, Hp, width = self.net.lay, self.h.Hp, self.h.width
        for name in ("params", "m", "v"):
            rest = torch.ones(before[name].numel(), dtype=torch.bool)
            for off, n in self.slices:
                rest[off:off + n] = False
            assert torch.equal(after[name][rest], before[name][rest]), f"{name} written outside the head slices"
            assert not self.B.get(name, -1)[lay.wa + 2 * width:lay.wa + 2 * Hp].any(), f"{name}: padded rows of Wa"

    def train_outputs(self):
        B, Hp = self.B, self.h.Hp
        return [B.get("loss", 1), B.get("dz_last", 32, Hp)] + \
            [a for name in ("params", "m", "v") for k in ("W", "b") for a in self.step(name)[k][1:]]


def _check_head_train(H, before, label, group="head"):
    """The outputs of one loc_head_train launch against the references of H.h."""
    h, B, Hp = H.h, H.B, H.h.Hp
    after = B.snap()
    B.check_margins()
    _unchanged(before, after, ("a", "rows", "yhat", "dist"))
    H.only_the_head_slices_written(before, after)
    (r64, *s64), (r32, *s32) = h.refs["f64"], h.refs["f32"]
    loss, dzl = float(B.get("loss", 1)[0]), B.get("dz_last", 32, Hp)
    assert abs(loss - r64["loss"]) < 2e-5, (loss, r64["loss"])
    assert not dzl[h.n_b:].any(), "dz_last of a row >= n_b is not exactly 0"
    assert not dzl[:, h.width:].any(), "dz_last of a padded unit is not exactly 0"
    assert all(np.isfinite(a).all() for a in H.train_outputs())
    got = tuple(H.step(n) for n in ("params", "m", "v"))
    fails = _judge_step(got, s64, s32, HEAD_MARGIN, label, [1, 2], group + " step")
    assert not fails, fails
    return dzl[:h.n_b, :h.width], r64, r32


HEAD_HP = (32, 96, 512, 544, 1024)


@pytest.mark.gpu
@pytest.mark.parametrize("Hp,n_b", [(w, n) for w in HEAD_HP for n in (1, 2, 31, 32)])
def test_head_train_against_the_reference(Hp, n_b):
    """One step: the loss, dz_last (rows >= n_b exactly 0), Wa, ba, Wb, bb and their slices of the flat m / v, nothing else
    of m, v or the parameters written; finite junk in rows >= n_b of `a` changes no output value."""
    h = _head_case(Hp, n_b, seed=Hp + n_b)
    H = _Head(h, ("nan", "junk")[(Hp // 32 + n_b) % 2])
    before = H.fill("zero")
    assert H.train() == 0, H.net.lib.loc_last_error()
    label = f"head_train Hp {Hp} n_b {n_b}"
    dzl, r64, r32 = _check_head_train(H, before, label)
    fails = _judge({"dz_last": dzl}, {"dz_last": r64["dz"][0]}, {"dz_last": r32["dz"][0]}, HEAD_MARGIN, label,
                   "head dz_last")
    assert not fails, fails
    if n_b < 32:
        first = H.train_outputs()
        H.fill("junk")
        assert H.train() == 0, H.net.lib.loc_last_error()
        for a, b in zip(first, H.train_outputs()):
            assert np.array_equal(a, b), "an output depends on rows >= n_b of a"
        H.B.check_margins()


@pytest.mark.gpu
@pytest.mark.parametrize("Hp", [32, 544])
def test_head_train_at_distance_zero(Hp):
    """Wa = 0, ba = 0 and one target equal to bb: that row's y2 is its target exactly, d = 0, and its loss gradient is taken
    as 0 (Keras: NaN).  Alone in its batch nothing moves at all; among five rows every output is finite and as the
    reference, which drops that row's gradient, has it."""
    h = _head_case(Hp, 1, seed=Hp, zero_row=0)
    H = _Head(h, "nan")
    before = H.fill("zero")
    assert H.train() == 0, H.net.lib.loc_last_error()
    after = H.B.snap()
    H.B.check_margins()
    assert float(H.B.get("loss", 1)[0]) == 0.0
    assert not H.B.get("dz_last", 32, Hp).any()
    assert torch.equal(after["params"], before["params"]), "a zero gradient moved a weight"
    for name in ("m", "v"):
        assert torch.equal(after[name], before[name]), f"{name}: a zero gradient left a moment"

    h = _head_case(Hp, 5, seed=Hp + 5, zero_row=2)
    r64 = h.refs["f64"][0]
    assert r64["head"][0][2] == 0 and not r64["head"][3][2].any() and (np.delete(r64["head"][0], 2) > 0).all()
    H = _Head(h, "junk")
    before = H.fill("zero")
    assert H.train() == 0, H.net.lib.loc_last_error()
    dzl, _, _ = _check_head_train(H, before, f"head_train Hp {Hp} distance 0", "head at distance 0")
    assert not dzl.any()                                             # Wa = 0: no gradient reaches the layer below


@pytest.mark.gpu
@pytest.mark.parametrize("Hp,n_b,targets", [(w, n, t) for w in HEAD_HP for n in (1, 31, 32) for t in (False, True)])
def test_head_eval_against_the_reference(Hp, n_b, targets):
    """yhat (and dist with targets) of rows < n_b per tensor and per row; rows >= n_b of both keep their poison, as does
    all of dist without targets; nothing else is written.  Rows >= n_b of `a` hold poison."""
    h = _head_case(Hp, n_b, seed=Hp + n_b)
    H = _Head(h, ("nan", "junk")[(Hp // 32 + n_b + targets) % 2])
    before = H.fill(pad=None)
    assert H.eval(targets) == 0, H.net.lib.loc_last_error()
    after = H.B.snap()
    H.B.check_margins()
    _unchanged(before, after, ("a", "params", "m", "v", "dz_last", "loss", "rows") + (() if targets else ("dist",)))
    assert torch.equal(after["yhat"][2 * n_b:], before["yhat"][2 * n_b:]), "yhat of a row >= n_b written"
    assert torch.equal(after["dist"][n_b:], before["dist"][n_b:]), "dist of a row >= n_b written"
    names = ("yhat", "dist") if targets else ("yhat",)
    got = {"yhat": H.B.get("yhat", 32, 2)[:n_b], "dist": H.B.get("dist", 32, 1)[:n_b]}
    ref64, ref32 = _head_eval_ref(h, np.float64), _head_eval_ref(h, np.float32)
    pick = lambda d: {k: d[k] for k in names}
    fails = _judge(pick(got), pick(ref64), pick(ref32), HEAD_MARGIN, f"head_eval Hp {Hp} n_b {n_b} targets {targets}",
                   "head eval")
    assert not fails, fails


# ------------------------------------------------------------------ refusals
BAD_HP = (0, 100, 1056)
REFUSALS = [(f, dict(Hp=w)) for f in ("dense_forward", "dense_backward", "head_train", "head_eval") for w in BAD_HP] + \
           [(f, dict(n_b=n)) for f in ("head_train", "head_eval") for n in (0, 33)] + \
           [("dense_forward", dict(null="W")), ("dense_backward", dict(null="dz_prev")),
            ("dense_backward", dict(null="vb2"))]


@functools.lru_cache(maxsize=1)
def _refusal_buffers():
    """Every buffer of the four entry points at Hp = 1056, so that no launch a missing check lets through can leave them."""
    Hp = 1056
    act = ("inp", "out", "out_drop", "dz", "a_prev", "dz_prev", "in2", "dz2", "a", "dz_last")
    mat = ("W", "W2", "mW2", "vW2")
    vec = ("b", "b2", "mb2", "vb2")
    flat = 2 * Hp + 8                                                # wa | ba | wb | bb
    B = _Bufs(Hp, **{k: 32 * Hp for k in act}, **{k: Hp * Hp for k in mat}, **{k: Hp for k in vec},
              mask=(32 * Hp, torch.uint8), params=flat, m=flat, v=flat, loss=1, yhat=64, dist=32, rows=(32, torch.int32),
              Y=64)
    return B


@pytest.mark.gpu
@pytest.mark.parametrize("entry,bad", REFUSALS, ids=[f"{f}-{k}{v}" for f, b in REFUSALS for k, v in b.items()])
def test_bad_arguments_write_nothing(entry, bad):
    """Hp = 0, 100 (no multiple of 32) and 1056 (above the limit) for all four entry points, n_b = 0 and 33 for the heads, a
    NULL mandatory pointer and a half-given half of the backward: nonzero, a message that names the entry point, and no
    byte of any buffer written."""
    net, B = _plumbing(), _refusal_buffers()
    lib = net.lib
    Hp, n_b = bad.get("Hp", 96), bad.get("n_b", 20)
    B.poison("junk")
    B.put("rows", np.arange(32, dtype=np.int32))
    before = B.snap()
    P = lambda name: None if name == bad.get("null") else B.ptr(name)
    off = 2 * 1056
    heads = (P("params"), P("params") + 4 * off, P("params") + 4 * (off + 2), P("params") + 4 * (off + 6))
    if entry == "dense_forward":
        rc = lib.loc_dense_forward(P("inp"), P("W"), P("b"), Hp, P("out"), P("out_drop"), P("mask"), KS, None)
    elif entry == "dense_backward":
        rc = lib.loc_dense_backward(P("dz"), P("W"), P("a_prev"), P("mask"), KS, P("dz_prev"), *(P(k) for k in _DW_BUFS),
                                    Hp, *_adam_args(net), None)
    elif entry == "head_train":
        rc = lib.loc_head_train(P("a"), Hp, n_b, P("rows"), P("Y"), *heads, P("m"), P("v"), 0, off, off + 2, off + 6,
                                P("dz_last"), P("loss"), *_adam_args(net), None)
    else:
        rc = lib.loc_head_eval(P("a"), Hp, n_b, *heads, P("yhat"), P("rows"), P("Y"), P("dist"), None)
    after = B.snap()
    B.check_margins()
    assert rc != 0, (entry, bad)
    assert ("loc_" + entry).encode() in lib.loc_last_error(), lib.loc_last_error()
    _unchanged(before, after, list(B.t))


# ------------------------------------------------------------------ the routes that use these kernels
@pytest.mark.gpu
@pytest.mark.parametrize("width,nlayers,n_b", [(160, 2, 32), (160, 3, 19), (160, 5, 32), (320, 2, 19), (320, 3, 32),
                                               (320, 5, 7), (992, 2, 32), (992, 3, 32), (992, 5, 19)])
def test_one_train_step_on_the_per_layer_route(width, nlayers, n_b):
    """loc_train_step at NHT 5, 10 and 31, depths 2, 3 and 5, dropout 0.25: the moments after that single step against the
    float64 replay per tensor and per 32 x 32 tile, as tests/test_gpu_moments.py has them after one epoch (its margin: layer
    1 and BatchNorm are part of the step), and the loss within 2e-5."""
    from tests.test_gpu_moments import MARGIN as STEP_MARGIN
    x, y, p, rng = make_problem(64, K, width, nlayers, seed=width + nlayers)
    p = O.cast_params(O.cast_params(p, np.float32), np.float64)
    net = build_net(x, y, p, drop_p=DROP_P, seed=5)
    assert not net.use_fused and net.d.Hp == width
    idx = rng.choice(64, n_b, replace=False)
    mask_np = (rng.random((32, net.d.Hp)) >= DROP_P).astype(np.uint8)
    loss = torch.zeros(1, device="cuda")
    net.train_step(torch.from_numpy(idx.astype(np.int32)).cuda(), n_b, 1, torch.from_numpy(mask_np).cuda(), loss)
    torch.cuda.synchronize()
    gm, gv = net.export_adam()
    kw = dict(x=x, y=y, rows=idx, batch=n_b, masks=[mask_np], drop_p=DROP_P)
    l64, m64, v64 = replay_epoch(p, **kw)
    _, m32, v32 = replay_epoch(p, dtype=np.float32, **kw)
    floors = [moments_err(a, b) for a, b in ((m32, m64), (v32, v64))]
    F, F_tile = max(max(t.values()) for t, _ in floors), max(max(tt.values()) for _, tt in floors)
    assert 0 < F and STEP_MARGIN * F < CAP and 0 < F_tile and STEP_MARGIN * F_tile < CAP, (F, F_tile)
    worst, worst_tile = {}, {}
    for name, got, ref in (("m", gm, m64), ("v", gv, v64)):
        t, tt = moments_err(got, ref)
        worst.update({f"{name}.{k}": e for k, e in t.items()})
        worst_tile.update({f"{name}.{k}": e for k, e in tt.items()})
    kt, kk = max(worst, key=worst.get), max(worst_tile, key=worst_tile.get)
    print(f"train step width {width} L {nlayers} n_b {n_b}: F {F:.2e} device {worst[kt]:.2e} ({kt}) ratio "
          f"{worst[kt] / F:.2f} | F_tile {F_tile:.2e} device {worst_tile[kk]:.2e} ({kk}) ratio "
          f"{worst_tile[kk] / F_tile:.2f} | loss {abs(loss.item() - l64[0]):.1e}")
    assert worst[kt] <= STEP_MARGIN * F, (kt, worst[kt], F)
    assert worst_tile[kk] <= STEP_MARGIN * F_tile, (kk, worst_tile[kk], F_tile)
    assert abs(loss.item() - l64[0]) < 2e-5, (loss.item(), l64[0])


@pytest.mark.gpu
@pytest.mark.parametrize("width,nlayers", [(96, 3), (600, 2)])
def test_predict_on_the_per_layer_route(width, nlayers):
    """loc_predict at NHT 3 and 19 with 1, 33 and 70 rows - one block, a second block of one row, three blocks - against
    the oracle, at the predict bar of tests/test_gpu_edge.py."""
    x, y, p, _ = make_problem(70, K, width, nlayers, seed=width)
    net = build_net(x, y, p)
    assert not net.use_fused
    for n in (1, 33, 70):
        yhat = torch.full((n, 2), float("nan"), device="cuda")
        net.predict_rows(torch.arange(n, dtype=torch.int32, device="cuda"), n, yhat)
        torch.cuda.synchronize()
        assert maxerr(yhat.cpu().numpy(), O.predict(p, x[:n])) < 2e-4, n
