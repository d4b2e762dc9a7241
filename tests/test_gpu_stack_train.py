"""The fused hidden stack of a TRAINING step at kernel level: loc_stack_forward_backward and loc_stack_dw_adam_tail called
directly (locator.py:319-325 layers 2..L with Dropout, Dense(2) x 2, euclidean_distance_loss and their backward pass,
:314-315), every caller buffer a guarded view of exactly the documented size and poisoned before the call.

The memory contract these tests state (include/locator_hip.h, Conventions):
  acts [L][slot_rows][Hp]   slot 0 = layer 1's ELU output is an INPUT (rows of the 32-row blocks in use must be finite);
                            layers 2..L are written for every row of the blocks in use, nothing beyond them
  adrop [slot_rows][Hp]     an input when Dropout follows layer 1 (n_pre == 1), written (blocks in use) when n_pre >= 2,
                            untouched without dropout
  dz [L][slot_rows][Hp]     written for the blocks in use; EXACTLY 0 for rows >= n_b (stack_dw_all_body and the layer-1
                            backward contract whole 32-row blocks)
  head_out [slot_rows][8]   [d, dy1 x 2, y1 x 2, dy2 x 2, 0]; rows >= n_b of the blocks in use: 0 in columns 0, 1, 2, 5, 6
Rows of unused blocks keep whatever they held.

The reference is a plain NumPy MLP (_ref_stack) in float64; the same function in float32 gives the floor: F = the largest
relative L2 distance of the float32 form from the float64 one over all tensors, F_row the same over all rows of all
tensors.  The device may be MARGIN times as far and never more than CAP.  test_reference_stack_matches_the_oracle (no GPU)
pins the float64 form to oracle.loss_and_grads."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import locator_oracle as O
from tests.gpu_util import _rel, bits, guarded, maxerr, moments_err, poison, randomize_params

# The device over the float32 reference's own distance from float64: it sums in another order and uses the hardware's exp.
# Every case prints device / F and device / F_row (pytest -s); measured on an MI355X the largest ratios are 1.75 per tensor
# (one row, width 64), 1.93 per row (129 rows, width 64, 10 layers) and 1.51 / 1.50 for the moments of the tail's Adam step
# per tensor / per 32 x 32 tile, so the margin stands at about twice the largest - not at the 10 that
# tests/test_gpu_moments.py grants over the same kind of floor.
MARGIN = 4.0
CAP = 1e-3
DROP_P = 0.25


# ------------------------------------------------------------------ the reference
def _elu_grad(a):
    return np.where(a > 0, 1, a + 1)


def _ref_stack(p, a1, mask, y, drop_p):
    """Layers 2..L, the heads, the loss and the backward pass down to dz of layer 1, in the dtype of p.
    p: oracle-format parameters; a1 [n_b][H] ELU output of layer 1; mask [n_b][H] keep flags or None; y [n_b][2].
    -> acts (L arrays, acts[0] = a1), adrop (or None), dz (L arrays), head = (d, dy1, y1, g), ins (input of layers 2..L),
    loss."""
    dt = p["gamma"].dtype.type
    L = len(p["W"]) - 2
    n_pre = O.n_pre(L)
    n_b = a1.shape[0]
    a1, y = np.asarray(a1, dt), np.asarray(y, dt)
    keep = None if mask is None else mask.astype(dt) * dt(1.0 / (1.0 - drop_p))
    acts, ins, adrop, a = [a1], [], None, a1
    if keep is not None and n_pre == 1:
        adrop = a = a1 * keep
    for l in range(2, L + 1):
        ins.append(a)
        a = O.elu(a @ p["W"][l - 1] + p["b"][l - 1])
        acts.append(a)
        if keep is not None and l == n_pre:
            adrop = a = a * keep
    y1 = a @ p["W"][L] + p["b"][L]
    y2 = y1 @ p["W"][L + 1] + p["b"][L + 1]
    e = y2 - y
    d = np.sqrt(np.maximum((e * e).sum(-1), 0))
    g = np.where(d[:, None] > 0, e / np.where(d > 0, d, 1)[:, None], 0) / dt(n_b)
    dy1 = g @ p["W"][L + 1].T
    dz = [None] * L
    dz[L - 1] = (dy1 @ p["W"][L].T) * _elu_grad(acts[L - 1])
    for l in range(L, 1, -1):
        da = dz[l - 1] @ p["W"][l - 1].T
        if keep is not None and l - 1 == n_pre:
            da = da * keep
        dz[l - 2] = da * _elu_grad(acts[l - 2])
    return dict(acts=acts, adrop=adrop, dz=dz, head=(d, dy1, y1, g), ins=ins, head_in=a, loss=d.mean())


def _ref_grads(p, r):
    """Gradients of layers 2..L and of the two heads from _ref_stack's output, in oracle format (layer 1, gamma and beta,
    which the hidden stack does not touch, stay 0)."""
    L = len(p["W"]) - 2
    d, dy1, y1, g = r["head"]
    out = O.zeros_like_trainable(p)
    for l in range(2, L + 1):
        out["W"][l - 1] = r["ins"][l - 2].T @ r["dz"][l - 1]
        out["b"][l - 1] = r["dz"][l - 1].sum(0)
    out["W"][L], out["b"][L] = r["head_in"].T @ dy1, dy1.sum(0)
    out["W"][L + 1], out["b"][L + 1] = y1.T @ g, g.sum(0)
    return out


def _problem(width, L, n_b, seed, K=40):
    """fp32-representable parameters, layer-1 activations, targets and keep flags: both references and the device start
    from identical values."""
    rng = np.random.default_rng(seed)
    p = randomize_params(O.init_params(K, width, L, rng), rng, round_fp32=True)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    a1 = f32(O.elu(rng.normal(0, 1, (n_b, width))))
    y = f32(rng.normal(0, 1, (n_b, 2)))
    return p, a1, y, rng


@pytest.mark.parametrize("width,L,n_b,drop", [(33, 2, 5, True), (40, 3, 7, True), (64, 4, 33, True), (24, 10, 9, True),
                                              (40, 2, 1, False), (50, 5, 12, False)])
def test_reference_stack_matches_the_oracle(width, L, n_b, drop):
    """in_l^T dz_l and sum_b dz_l of the float64 reference = the oracle's W / b gradients of layers 2..L and of the heads,
    its loss the oracle's, to 1e-12 relative (n_pre = 1, where the stack's input is the dropped-out a1, among the cases)."""
    K = 40
    p, _, y, rng = _problem(width, L, n_b, seed=width + L, K=K)
    x = rng.integers(0, 3, (n_b, K))
    mask = (rng.random((n_b, width)) >= DROP_P).astype(np.uint8) if drop else None
    loss, g, _ = O.loss_and_grads(p, x, y, mask, DROP_P if drop else 0.0, update_moving=False)
    _, c = O.forward(p, x, True, mask, DROP_P if drop else 0.0, update_moving=False)
    r = _ref_stack(p, c["acts_out"][0], mask, y, DROP_P)
    mine = _ref_grads(p, r)
    assert abs(r["loss"] - loss) <= 1e-12 * abs(loss)
    for l in range(1, L + 2):
        for name in ("W", "b"):
            ref = g[name][l]
            err = np.linalg.norm(mine[name][l] - ref) / np.linalg.norm(ref)
            assert err < 1e-12, (name, l, err)
    assert not np.any(mine["W"][0]) and not np.any(mine["gamma"])


# ------------------------------------------------------------------ the device side
class _Stack:
    """One problem on the device: a LocatorNet for its parameter plumbing, and the four caller buffers of
    loc_stack_forward_backward as guarded views of exactly the documented sizes."""

    def __init__(self, width, L, n_b, slot, drop, seed, kind="nan"):
        from tests.gpu_util import build_net
        self.p, self.a1, self.y, rng = _problem(width, L, n_b, seed)
        x = np.zeros((n_b, 40), np.uint8)
        self.net = net = build_net(x, self.y, self.p, drop_p=DROP_P if drop else 0.0)
        d = net.d
        assert net.use_fused and d.L == L and d.n_pre == L // 2
        self.width, self.L, self.n_b, self.slot, self.drop, self.kind = width, L, n_b, slot, drop, kind
        self.Hp, self.used = d.Hp, (n_b + 31) // 32 * 32
        Hp, used = self.Hp, self.used
        self.mask_np = (rng.random((used, Hp)) >= DROP_P).astype(np.uint8) if drop else None
        self.mask = torch.from_numpy(self.mask_np).cuda() if drop else None
        self.ks = float(np.float32(1.0) / (np.float32(1.0) - np.float32(DROP_P))) if drop else 1.0
        self.rows = torch.arange(used, dtype=torch.int32, device="cuda")
        margin = 128 * Hp
        self.bufs, self.checks = {}, []
        for name, n in (("acts", L * slot * Hp), ("adrop", slot * Hp), ("dz", L * slot * Hp), ("head_out", slot * 8)):
            self.bufs[name], chk = guarded(n, torch.float32, margin)
            self.checks.append((name, chk))
        self.adrop_is_input = drop and d.n_pre == 1
        a1p = np.zeros((n_b, Hp), np.float32)
        a1p[:, :width] = self.a1
        self.a1_dev = torch.from_numpy(a1p).cuda()
        if self.adrop_is_input:
            self.adrop_in = self.a1_dev * (self.mask[:n_b].float() * self.ks)          # one fp32 product, as layer 1 leaves it

    def fill(self, pad="zero"):
        """Poison the four buffers, then write the inputs: rows < n_b of acts[0] (and of adrop when it is an input), and the
        rows from n_b to the end of the last block in use as the layer-1 forward leaves them (pad = "zero") or as finite
        junk (pad = "junk": the contract only asks for finite values there)."""
        n_b, used, Hp = self.n_b, self.used, self.Hp
        for i, t in enumerate(self.bufs.values()):
            poison(t, self.kind, 7 + i)
        a = self.view("acts")[0]
        a[:n_b] = self.a1_dev
        poison(a[n_b:used], pad, 31)
        if self.adrop_is_input:
            ad = self.view("adrop")
            ad[:n_b] = self.adrop_in
            poison(ad[n_b:used], pad, 32)
        torch.cuda.synchronize()
        self.before = {k: bits(t) for k, t in self.bufs.items()}

    def view(self, name):
        t = self.bufs[name]
        return {"acts": lambda: t.view(self.L, self.slot, self.Hp), "dz": lambda: t.view(self.L, self.slot, self.Hp),
                "adrop": lambda: t.view(self.slot, self.Hp), "head_out": lambda: t.view(self.slot, 8)}[name]()

    def launch(self, n_b=None, slot=None, Hp=None, tune=None):
        net, b = self.net, self.bufs
        lay, P = net.lay, net.params.data_ptr()
        a1_in = b["adrop"] if self.adrop_is_input else b["acts"]
        rc = net.lib.loc_stack_forward_backward(
            a1_in.data_ptr(), P + 4 * lay.wh, net.wht.data_ptr(), P + 4 * lay.bh, P + 4 * lay.wa, P + 4 * lay.ba,
            P + 4 * lay.wb, P + 4 * lay.bb, self.mask.data_ptr() if self.drop else None, self.ks,
            self.Hp if Hp is None else Hp, self.L, net.d.n_pre, self.n_b if n_b is None else n_b,
            self.slot if slot is None else slot, self.rows.data_ptr(), net.Y.data_ptr(), b["acts"].data_ptr(),
            b["adrop"].data_ptr(), b["dz"].data_ptr(), b["head_out"].data_ptr(), C.byref(tune) if tune is not None else None,
            None)
        torch.cuda.synchronize()
        return rc

    def tail(self, loss_out):
        from locator_amd.net import ALPHA_TAB_LEN
        net, b = self.net, self.bufs
        lay = net.lay
        rc = net.lib.loc_stack_dw_adam_tail(
            self.Hp, self.L, net.d.n_pre, self.n_b, self.slot, 1 if self.drop else 0, b["acts"].data_ptr(),
            b["adrop"].data_ptr(), b["dz"].data_ptr(), b["head_out"].data_ptr(), net.params.data_ptr(),
            net.adam_m.data_ptr(), net.adam_v.data_ptr(), net.wht.data_ptr(), lay.wh, lay.bh, lay.wa, lay.ba, lay.wb,
            lay.bb, loss_out.data_ptr(), net.alpha_tab.data_ptr(), ALPHA_TAB_LEN, net.lr_t.data_ptr(),
            net.t_base_t.data_ptr(), 1, None, None)
        torch.cuda.synchronize()
        return rc

    def outputs(self):
        """Host copies: acts [L][slot][Hp], adrop, dz, head_out as float32 arrays."""
        return {k: self.view(k).cpu().numpy() for k in self.bufs}

    def check_margins(self):
        for name, chk in self.checks:
            chk(name)

    def reference(self, dtype):
        p = O.cast_params(self.p, dtype)
        mask = self.mask_np[:self.n_b, :self.width] if self.drop else None
        return p, _ref_stack(p, self.a1, mask, self.y, DROP_P)


def _tensors(s, out_or_ref, device):
    """name -> [n_b][...] arrays that loc_stack_forward_backward computes, from the device's buffers or a reference."""
    n_b, H, L = s.n_b, s.width, s.L
    t = {}
    if device:
        o = out_or_ref
        for l in range(2, L + 1):
            t[f"acts{l}"] = o["acts"][l - 1, :n_b, :H]
        for l in range(1, L + 1):
            t[f"dz{l}"] = o["dz"][l - 1, :n_b, :H]
        if s.drop and not s.adrop_is_input:
            t["adrop"] = o["adrop"][:n_b, :H]
        h = o["head_out"][:n_b]
        t["d"], t["dy1"], t["y1"], t["dy2"] = h[:, 0:1], h[:, 1:3], h[:, 3:5], h[:, 5:7]
    else:
        r = out_or_ref
        for l in range(2, L + 1):
            t[f"acts{l}"] = r["acts"][l - 1]
        for l in range(1, L + 1):
            t[f"dz{l}"] = r["dz"][l - 1]
        if s.drop and not s.adrop_is_input:
            t["adrop"] = r["adrop"]
        d, dy1, y1, g = r["head"]
        t["d"], t["dy1"], t["y1"], t["dy2"] = d[:, None], dy1, y1, g
    return t


def _distances(got, ref):
    """-> {tensor: relative L2 distance}, {tensor: the largest relative L2 distance of one row}, in float64."""
    per_tensor, per_row = {}, {}
    for k, r in ref.items():
        g, r = np.asarray(got[k], np.float64), np.asarray(r, np.float64)
        assert g.shape == r.shape, (k, g.shape, r.shape)
        per_tensor[k] = float(_rel(np.linalg.norm(g - r), np.linalg.norm(r)))
        per_row[k] = float(_rel(np.linalg.norm(g - r, axis=1), np.linalg.norm(r, axis=1)).max())
    return per_tensor, per_row


# width, L, n_b, slot_rows, dropout, poison
STACK_CASES = [
    (64, 2, 1, 32, True, "nan"),            # n_pre = 1: the stack's input is adrop
    (61, 3, 2, 32, True, "junk"),           # n_pre = 1, padded width
    (64, 3, 31, 32, False, "nan"),
    (128, 4, 31, 32, True, "junk"),
    (256, 10, 32, 32, True, "nan"),
    (253, 10, 32, 32, False, "junk"),
    (512, 4, 32, 32, True, "nan"),
    (512, 2, 31, 32, True, "junk"),         # n_pre = 1 at the widest form
    (256, 4, 33, 64, True, "nan"),
    (128, 10, 64, 64, False, "junk"),
    (64, 4, 65, 128, True, "nan"),
    (128, 4, 100, 128, True, "junk"),
    (256, 4, 128, 128, True, "nan"),
    (64, 10, 129, 256, True, "junk"),
    (125, 4, 300, 384, True, "nan"),
    (256, 2, 100, 128, False, "junk"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("width,L,n_b,slot,drop,kind", STACK_CASES,
                         ids=[f"w{w}-L{L}-n{n}-slot{s}-{'drop' if dr else 'nodrop'}" for w, L, n, s, dr, _ in STACK_CASES])
def test_stack_forward_backward_and_tail_against_the_reference(width, L, n_b, slot, drop, kind):
    """Per element: rows < n_b of every output within MARGIN x the float32 reference's own error; dz and the loss-gradient
    columns of head_out exactly 0 from n_b to the end of the last block in use; unused blocks and every margin untouched;
    junk instead of the layer-1 forward's values in the padded input rows changes no bit of rows < n_b nor of the Adam
    step the tail takes from them; that step against a float64 Adam step from the reference's gradients."""
    s = _Stack(width, L, n_b, slot, drop, seed=width + 7 * L + n_b, kind=kind)
    Hp, used, net = s.Hp, s.used, s.net
    s.fill("zero")
    assert s.launch() == 0, net.lib.loc_last_error()
    out = s.outputs()
    after = {k: bits(t) for k, t in s.bufs.items()}
    s.check_margins()

    # 1. rows < n_b against the float64 reference, the float32 reference's distance as the floor
    p64, r64 = s.reference(np.float64)
    p32, r32 = s.reference(np.float32)
    ref = _tensors(s, r64, False)
    ft, fr = _distances(_tensors(s, r32, False), ref)
    F, F_row = max(ft.values()), max(fr.values())
    assert 0 < F and MARGIN * F < CAP and 0 < F_row and MARGIN * F_row < CAP, (F, F_row)
    dt, dr = _distances(_tensors(s, out, True), ref)
    kt, kr = max(dt, key=dt.get), max(dr, key=dr.get)
    print(f"stack width {width} L {L} n_b {n_b} slot {slot} drop {drop}: F {F:.2e} device {dt[kt]:.2e} ({kt}) ratio "
          f"{dt[kt] / F:.2f} | F_row {F_row:.2e} device {dr[kr]:.2e} ({kr}) ratio {dr[kr] / F_row:.2f}")
    assert dt[kt] <= MARGIN * F, (kt, dt[kt], F, dt)
    assert dr[kr] <= MARGIN * F_row, (kr, dr[kr], F_row, dr)
    # padded units stay exactly 0 through every layer
    assert not out["acts"][1:, :n_b, width:].any() and not out["dz"][:, :n_b, width:].any()

    # 2. rows n_b .. end of the last block in use
    assert not out["dz"][:, n_b:used].any(), "dz of a padded row is not exactly 0"
    assert not out["head_out"][n_b:used][:, [0, 1, 2, 5, 6]].any()
    assert np.isfinite(out["acts"][:, :used]).all() and np.isfinite(out["head_out"][:used]).all()

    # 3. what the launch may not touch: the inputs, every row of the unused blocks, adrop without dropout
    def same(name, index):
        shape = {"acts": (L, slot, Hp), "dz": (L, slot, Hp), "adrop": (slot, Hp), "head_out": (slot, 8)}[name]
        a, b = after[name].view(shape)[index], s.before[name].view(shape)[index]
        assert torch.equal(a, b), f"{name}{index}: {int((a != b).sum())} words written"
    same("acts", (0,))
    if not drop or s.adrop_is_input:
        same("adrop", slice(None))
    for name in s.bufs:
        same(name, (slice(None), slice(used, slot)) if name in ("acts", "dz") else slice(used, slot))

    # 4a. the tail on this variant
    def tail_state():
        loss = torch.full((1,), float("nan"), device="cuda")
        assert s.tail(loss) == 0, net.lib.loc_last_error()
        return {"params": bits(net.params), "adam_m": bits(net.adam_m), "adam_v": bits(net.adam_v), "wht": bits(net.wht),
                "loss": bits(loss)}
    start = {k: getattr(net, k).clone() for k in ("params", "adam_m", "adam_v", "wht")}
    tail_a = tail_state()
    s.check_margins()
    lay = net.lay
    assert torch.equal(tail_a["params"][:lay.wh], bits(start["params"])[:lay.wh])                 # layer 1 and BatchNorm
    assert torch.equal(tail_a["params"][lay.n_trainable:], bits(start["params"])[lay.n_trainable:])
    for k in ("acts", "adrop", "dz", "head_out"):
        assert torch.equal(bits(s.bufs[k]), after[k]), f"the tail wrote {k}"
    got_p, (got_m, got_v) = net.export_params(), net.export_adam()
    loss_dev = float(tail_a["loss"].view(torch.float32))
    wh = net.params[lay.wh:lay.wh + (L - 1) * Hp * Hp].view(L - 1, Hp, Hp)
    assert torch.equal(net.wht.view(L - 1, Hp, Hp), wh.transpose(1, 2)), "WhT is not the transposed updated kernels"

    # ... against one float64 Adam step from the reference's gradients (float32 step = the moments' floor)
    steps = {}
    for name, p, r in (("f64", p64, r64), ("f32", p32, r32)):
        pp = O.copy_params(p)
        m, v = O.zeros_like_trainable(pp), O.zeros_like_trainable(pp)
        O.adam_apply(pp, _ref_grads(p, r), m, v, 1, pp["gamma"].dtype.type(1e-3))
        steps[name] = (pp, m, v)
    pp, m64, v64 = steps["f64"]
    for l in range(1, L + 2):
        assert maxerr(got_p["W"][l], pp["W"][l]) < 1e-5 and maxerr(got_p["b"][l], pp["b"][l]) < 1e-5, l
    assert abs(loss_dev - r64["loss"]) < 2e-5, (loss_dev, r64["loss"])
    floors = [moments_err(a, b) for a, b in ((steps["f32"][1], m64), (steps["f32"][2], v64))]
    Fm = max(max(t.values()) for t, _ in floors)
    Fm_tile = max(max(tt.values()) for _, tt in floors)
    assert 0 < Fm and MARGIN * Fm < CAP and 0 < Fm_tile and MARGIN * Fm_tile < CAP, (Fm, Fm_tile)
    worst, worst_tile = {}, {}
    for name, got, want in (("m", got_m, m64), ("v", got_v, v64)):
        t, tt = moments_err(got, want)
        worst.update({f"{name}.{k}": e for k, e in t.items()})
        worst_tile.update({f"{name}.{k}": e for k, e in tt.items()})
    km, kk = max(worst, key=worst.get), max(worst_tile, key=worst_tile.get)
    print(f"  tail: F {Fm:.2e} device {worst[km]:.2e} ({km}) ratio {worst[km] / Fm:.2f} | F_tile {Fm_tile:.2e} device "
          f"{worst_tile[kk]:.2e} ({kk}) ratio {worst_tile[kk] / Fm_tile:.2f} | loss {abs(loss_dev - r64['loss']):.1e}")
    assert worst[km] <= MARGIN * Fm, (km, worst[km], Fm)
    assert worst_tile[kk] <= MARGIN * Fm_tile, (kk, worst_tile[kk], Fm_tile)

    # 4b. finite junk in the padded input rows: no bit of rows < n_b changes, nor of the step the tail takes
    if used > n_b:
        for k, t in start.items():
            getattr(net, k).copy_(t)
        s.fill("junk")
        assert s.launch() == 0, net.lib.loc_last_error()
        junk = s.outputs()
        for k in out:
            a, b = junk[k][..., :n_b, :], out[k][..., :n_b, :]
            assert np.array_equal(a.view(np.int32), b.view(np.int32)), f"{k}: rows < n_b depend on the padded input rows"
        assert not junk["dz"][:, n_b:used].any() and not junk["head_out"][n_b:used][:, [0, 1, 2, 5, 6]].any()
        tail_b = tail_state()
        for k in tail_a:
            assert torch.equal(tail_b[k], tail_a[k]), f"tail: {k} depends on the padded input rows"
        s.check_margins()


@pytest.mark.gpu
@pytest.mark.parametrize("width,L,n_b,slot", [(256, 10, 32, 32), (128, 4, 100, 128)])
def test_stack_speed_hints_change_no_bit(width, L, n_b, slot):
    """stack_train_rows x stack_xcd_stride x stack_helpers: every combination leaves the default's bits in acts, adrop, dz
    and head_out - the whole buffers, so also the same rows untouched."""
    from locator_amd import _lib
    s = _Stack(width, L, n_b, slot, True, seed=width + L, kind="junk")
    s.fill("zero")
    assert s.launch() == 0
    ref = {k: bits(t) for k, t in s.bufs.items()}
    assert torch.isfinite(s.view("dz")[:, :n_b]).all() and s.view("dz")[:, :n_b].abs().sum() > 0
    for rows in (1, 2, 4):
        for stride in (1, 2, 4, 8):
            for helpers in (-1, 0, 5):
                tune = _lib.Tuning(stack_train_rows=rows, stack_xcd_stride=stride, stack_helpers=helpers)
                s.fill("zero")
                assert s.launch(tune=tune) == 0, s.net.lib.loc_last_error()
                for k, t in s.bufs.items():
                    assert torch.equal(bits(t), ref[k]), (k, rows, stride, helpers)
    s.check_margins()


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [dict(n_b=0), dict(n_b=33), dict(slot=48), dict(Hp=96)],
                         ids=["n_b-0", "n_b-above-slot", "slot-48", "width-96"])
def test_stack_bad_arguments_write_nothing(bad):
    """n_b = 0, n_b > slot_rows, a slot that is no multiple of 32, a width without a fused form: nonzero, a message, and no
    byte of any buffer written."""
    s = _Stack(128, 4, 20, 32 if "n_b" in bad else 64, True, seed=3, kind="junk")      # buffers hold what width 96 would need
    s.fill("zero")
    rc = s.launch(**bad)
    assert rc != 0 and s.net.lib.loc_last_error().decode(), (rc, bad)
    for k, t in s.bufs.items():
        assert torch.equal(bits(t), s.before[k]), k
    s.check_margins()
