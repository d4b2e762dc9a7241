"""Layer 1 of a TRAINING step at kernel level: the BatchNorm statistics kernels, every form of the fused layer-1 backward +
Adam that its launcher can pick, and the two small forward forms, called through the C ABI on caller buffers that are
guarded views of exactly the documented sizes, poisoned before the call (locator.py:318-320, :367-376).

The memory contract these tests state (include/locator_hip.h):
  gb_scratch (Kp/32)*128 floats for EVERY row count up to LOC_BIG_BATCH_MAX; dz1 32*ceil(n_b/32) rows of Hp floats, rows
  >= n_b exactly 0; bn4 / bn4_out 4*Kp; stats_ep n_steps*2*Kp; W1 / m / v Kp*Hp in the W1S layout; `rows` / `rows_all` are
  read for n_b (batch) entries per step and no further - they are index buffers, so instead of poison they are followed by
  valid row numbers of a sentinel row of X that holds 255 everywhere: a read past the end gives a wrong number, not a fault.

References.  BatchNorm statistics: exact integers (sum x, sum x^2 as int64; the variance numerator n ss - s^2 stays below
2^53).  Backward: _ref_l1, a plain NumPy function evaluated in float64 and in float32, pinned to oracle.loss_and_grads by
test_reference_l1_matches_the_oracle (no GPU).  The float32 form's distance from the float64 one is the floor F - per
tensor, per 32 x 32 tile of W1 and per element of the vectors (relative to the tensor's largest entry); the device may be
MARGIN times as far and never more than CAP.  test_floors_leave_room_below_the_cap (no GPU) holds 0 < F and
MARGIN * F < CAP on every case.

MARGIN: every case prints device / F (pytest -s).  Measured on an MI355X (the table is in DESIGN.md section 2):
  backward, every form, more than one row: at most 3.11 per tensor (--nlayers 1 form, 7 rows, width 256: v of beta), 3.63 per
  tile (4096 rows, width 256: the big-batch form adds 128 row blocks in one fp32 accumulator chain where NumPy sums in
  blocks), 2.97 per element; gb_scratch slot 0 + slot 1 at most 2.72; the Adam run 1.00..1.23; the next step's bn4 at most
  1.81  ->  MARGIN = 8, about twice the largest;
  backward, ONE row: dgamma / dbeta at most 4.26 per tensor and 7.17 per element (width 1024), 5.99 in gb_scratch.  With one
  row nothing is summed over the batch, so dbeta[k] = sum_h dz[h] W1[k][h] is the device's single fp32 chain over all units
  (one MFMA accumulator carried across the unit tiles of a k-tile, l1_bwd_adam_kernel) against NumPy's blocked dot product:
  a chain of 1024 terms is sqrt(1024 / 16) = 8 times as far as 16-lane blocks.  Twice the largest gives
  MARGIN_ONE_ROW = 14 for the gamma / beta sums of one-row calls only; it is above 10 and stays, because shortening the
  chain would change the bits of every 32-row step of the default path for the sake of a batch of one;
  BatchNorm statistics at most 1.58, forward forms at most 0.96  ->  MARGIN_SMALL = 4."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import locator_oracle as O
from tests.gpu_util import _rel, bits, guarded, moments_err, poison, randomize_params, ulp32, w1s_pack, w1s_unpack

MARGIN = 8.0
MARGIN_ONE_ROW = 14.0
MARGIN_SMALL = 4.0
CAP = 1e-3
BIG_BATCH_MAX = 4096
KEEP_SCALE = float(np.float32(1.0) / (np.float32(1.0) - np.float32(0.25)))
# The Adam run: t = 10 and a rate far from the default.  w' - w is read from fp32 weights, so it carries their rounding:
# half an ulp of |w| ~ 0.1..1 over an update of 0.15 lr m / sqrt(v).  At lr = 1e-3 that is 2e-4 of the update and would be
# all the comparison sees; at lr = 1/8 (exact in fp32) the update is 1e-2 and the floor of w' - w comes out at 1e-5.
LR_ADAM, T_BASE, T_OFF = 0.125, 7, 3
ALPHA_LEN = 64


# ------------------------------------------------------------------ the reference
def _ref_l1(x, bn4, dz1, W1, mask=None, keep_scale=1.0, dtype=np.float64):
    """Gradients of layer 1 and of BatchNorm's gamma / beta for one minibatch, everything in `dtype`.
    x [n_b][K] genotypes; bn4 = (scale, shift, mean, rstd), the fp32 values handed to the kernel - they carry gamma and
    beta (scale = gamma rstd, shift = beta - mean scale), which therefore are no inputs of their own here (_adam_step
    takes them); dz1 [n_b][H]; W1 [K][H]; mask [n_b][K] keep flags of a Dropout directly on the BatchNorm output, or None.
    -> {"W": [dW1], "b": [db1], "gamma", "beta"} (oracle format)."""
    dt = dtype
    x = np.asarray(x).astype(dt)
    sc, sh, mu, rs = (np.asarray(a).astype(dt) for a in bn4)
    dz, W = np.asarray(dz1).astype(dt), np.asarray(W1).astype(dt)
    xhat = x * sc + sh
    xn = (x - mu) * rs
    mk = None if mask is None else np.asarray(mask).astype(dt) * dt(keep_scale)
    if mk is not None:
        xhat = xhat * mk
    dxhat = dz @ W.T
    if mk is not None:
        dxhat = dxhat * mk
    return {"W": [xhat.T @ dz], "b": [dz.sum(0)], "gamma": (dxhat * xn).sum(0), "beta": dxhat.sum(0)}


def _bn4_from(mean, var, gamma, beta):
    """(scale, shift, mean, rstd) in the dtype of gamma from batch statistics [mean, biased var]."""
    dt = gamma.dtype.type
    rstd = dt(1.0) / np.sqrt(var.astype(dt) + dt(O.BN_EPS))
    scale = gamma * rstd
    return scale, beta - mean.astype(dt) * scale, mean.astype(dt), rstd


def _adam_step(p, g, m, v, t, lr):
    """One O.adam_apply on copies, in the dtype of p -> (p', m', v')."""
    dt = p["gamma"].dtype.type
    p, m, v = O.copy_params(p), O.copy_params(m), O.copy_params(v)
    O.adam_apply(p, g, m, v, t, dt(lr))
    return p, m, v


@pytest.mark.parametrize("K,width,L,n_b,drop", [(40, 33, 4, 9, True), (37, 24, 1, 7, True)])
def test_reference_l1_matches_the_oracle(K, width, L, n_b, drop):
    """_ref_l1 in float64, fed the oracle's batch statistics and its dz of layer 1, gives the oracle's gradients of W1, b1,
    gamma and beta to 1e-12 relative - with --nlayers 1 the Dropout mask sits on the BatchNorm output."""
    from tests.test_gpu_stack_train import _ref_stack
    rng = np.random.default_rng(K + L)
    p = randomize_params(O.init_params(K, width, L, rng), rng, round_fp32=True)
    x = rng.integers(0, 3, (n_b, K))
    y = rng.normal(0, 1, (n_b, 2))
    mw = K if L == 1 else width
    mask = (rng.random((n_b, mw)) >= 0.25).astype(np.uint8)
    _, g, _ = O.loss_and_grads(p, x, y, mask, 0.25, update_moving=False)
    _, c = O.forward(p, x, True, mask, 0.25, update_moving=False)
    dz1 = _ref_stack(p, c["acts_out"][0], None if L == 1 else mask, y, 0.25)["dz"][0]
    bn4 = _bn4_from(c["mu"], c["var"], p["gamma"], p["beta"])
    mine = _ref_l1(x, bn4, dz1, p["W"][0], mask if L == 1 else None, 1.0 / (1.0 - 0.25))
    for name, a, b in (("W1", mine["W"][0], g["W"][0]), ("b1", mine["b"][0], g["b"][0]), ("gamma", mine["gamma"], g["gamma"]),
                       ("beta", mine["beta"], g["beta"])):
        assert np.linalg.norm(b) > 0 and np.linalg.norm(a - b) / np.linalg.norm(b) < 1e-12, name


# ------------------------------------------------------------------ one backward problem on the host
def _genotypes(rng, n, K, xmax):
    """Binomial(xmax, allele frequency) per SNP; with more than one row the largest value is present."""
    af = rng.beta(0.4, 0.9, K).clip(0.02, 0.98)
    x = rng.binomial(xmax, af, (n, K))
    if n > 1:
        x[rng.integers(0, n), rng.integers(0, K)] = xmax
    return x.astype(np.uint8)


class _Problem:
    """Inputs (all fp32-representable) and both references of one layer-1 backward call."""

    def __init__(self, K, width, n_b, xmax, seed, indrop=False):
        rng = np.random.default_rng(seed)
        f32 = lambda a: np.asarray(a, np.float32)
        self.K, self.width, self.n_b, self.xmax, self.indrop = K, width, n_b, xmax, indrop
        self.Kp, self.Hp = -(-K // 32) * 32, -(-width // 32) * 32
        self.used = -(-n_b // 32) * 32
        self.n_samp = n_b + 3
        self.x_all = _genotypes(rng, self.n_samp, K, xmax)
        self.rows = rng.permutation(self.n_samp)[:n_b].astype(np.int32)
        self.x = self.x_all[self.rows]
        self.p = {"gamma": f32(rng.uniform(0.7, 1.3, K)), "beta": f32(rng.normal(0, 0.05, K)),
                  "W": [f32(rng.normal(0, 0.1, (K, width)))], "b": [f32(rng.normal(0, 0.05, width))]}
        self.dz = f32(rng.normal(0, 1, (n_b, width)) / n_b)
        x64 = self.x.astype(np.float64)
        p64 = O.cast_params(self.p, np.float64)
        self.bn4 = tuple(f32(a) for a in _bn4_from(x64.mean(0), x64.var(0), p64["gamma"], p64["beta"]))
        nxt = self.x_all[rng.permutation(self.n_samp)[:max(2, n_b // 2)]].astype(np.float64)
        self.next_stats = (f32(nxt.mean(0)), f32(nxt.var(0)))
        self.mask = (rng.random((32, self.Kp)) >= 0.25).astype(np.uint8) if indrop else None
        self.rng = rng
        self._grads, self._runs = {}, {}

    def grads(self, dt):
        if dt not in self._grads:
            mask = self.mask[:self.n_b, :self.K] if self.indrop else None
            self._grads[dt] = _ref_l1(self.x, self.bn4, self.dz, self.p["W"][0], mask, KEEP_SCALE, dt)
        return self._grads[dt]

    def moments(self):
        """Random m and v >= 0 of the Adam run, of the size a fit gives them (v ~ m^2 ~ g^2), fp32 values."""
        if not hasattr(self, "_mv"):
            g = self.grads(np.float64)
            rms = lambda a: float(np.sqrt(np.mean(np.square(a)))) or 1e-3
            draw_m = lambda a: np.float32(self.rng.normal(0, 0.3 * rms(a), np.shape(a)))
            draw_v = lambda a: np.float32((0.5 + self.rng.random(np.shape(a))) * rms(a) ** 2)
            self._mv = tuple({"gamma": d(g["gamma"]), "beta": d(g["beta"]), "W": [d(g["W"][0])], "b": [d(g["b"][0])]}
                             for d in (draw_m, draw_v))
        return self._mv

    def run(self, which, dt):
        """(p', m', v') of the gradient run (m = v = 0, t = 1, lr 1e-3) or the Adam run, in dt."""
        if (which, dt) not in self._runs:
            p = O.cast_params(self.p, dt)
            if which == "gradient":
                m, v, t, lr = O.zeros_like_trainable(p), O.zeros_like_trainable(p), 1, float(np.float32(1e-3))
            else:
                m, v = (O.cast_params(a, dt) for a in self.moments())
                t, lr = T_BASE + T_OFF, LR_ADAM
            self._runs[(which, dt)] = _adam_step(p, self.grads(dt), m, v, t, lr)
        return self._runs[(which, dt)]

    def bn4_next(self, dt):
        """[scale|shift|mean|rstd] of the next minibatch from the Adam run's updated gamma / beta, [4][K]."""
        p1 = self.run("adam", dt)[0]
        return np.stack(_bn4_from(self.next_stats[0], self.next_stats[1], p1["gamma"], p1["beta"]))


def _delta(after, before):
    """w' - w per tensor, in float64 from the two parameter dicts."""
    f = lambda a, b: np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return {"gamma": f(after["gamma"], before["gamma"]), "beta": f(after["beta"], before["beta"]),
            "W": [f(after["W"][0], before["W"][0])], "b": [f(after["b"][0], before["b"][0])]}


def _distances(got, ref):
    """got / ref: {group: oracle-format dict}.  -> three {name: distance}: per tensor and per 32 x 32 tile of W1 (relative
    L2, tests/gpu_util.moments_err), and per element of b1 / gamma / beta relative to the tensor's largest entry."""
    per_tensor, per_tile, per_elem = {}, {}, {}
    for grp in ref:
        t, tt = moments_err(got[grp], ref[grp])
        per_tensor.update({f"{grp}.{k}": e for k, e in t.items()})
        per_tile.update({f"{grp}.{k}": e for k, e in tt.items()})
        for name, g, r in (("gamma", got[grp]["gamma"], ref[grp]["gamma"]), ("beta", got[grp]["beta"], ref[grp]["beta"]),
                           ("b0", got[grp]["b"][0], ref[grp]["b"][0])):
            g, r = np.asarray(g, np.float64), np.asarray(r, np.float64)
            per_elem[f"{grp}.{name}"] = float(_rel(np.abs(g - r).max(), np.abs(r).max()))
    return per_tensor, per_tile, per_elem


def _floors(prob, which):
    """-> ref (float64 groups), (F, F_tile, F_elem) of the float32 form for the gradient run or the Adam run."""
    out = {}
    for dt in (np.float64, np.float32):
        p1, m1, v1 = prob.run(which, dt)
        out[dt] = {"m": m1, "v": v1}
        if which == "adam":
            out[dt]["dw"] = _delta(p1, O.cast_params(prob.p, dt))
    F = tuple(max(d.values()) for d in _distances(out[np.float32], out[np.float64]))
    return out[np.float64], F


def _vector_floor(got32, ref64):
    """Relative L2 per row of a [rows][n] pair and per element relative to the row's largest entry -> (F, F_elem)."""
    g, r = np.asarray(got32, np.float64), np.asarray(ref64, np.float64)
    per_row = _rel(np.linalg.norm(g - r, axis=1), np.linalg.norm(r, axis=1))
    per_el = _rel(np.abs(g - r).max(axis=1), np.abs(r).max(axis=1))
    return float(per_row.max()), float(per_el.max())


# ------------------------------------------------------------------ the cases of the backward
KGRID = [(20, 1), (97, 1), (1000, 1), (1000, 8), (1000, 5)]
#   K = 20: less than one k-tile; 97: three tiles and one SNP; 1000 (32 k-tiles): grid 1 = four waves of eight k-tiles,
#   grid 8 = 32 waves of exactly one k-tile, grid 5 = 20 waves whose unit ranges (1.6 k-tiles) cut k-tiles in two, so
#   both gbs slots are used (unless the width is a single unit tile)


def _form(n_b, Hp, in_mask, tune):
    """The kernel l1_backward_main_impl launches for these arguments."""
    nht = Hp // 32
    if n_b > 128:
        return f"big<{nht}>"
    rb = -(-n_b // 32)
    if rb == 1 and tune.get("l1b_rows") == 1 and nht == 8 and not in_mask:
        return "rows<8,13,1>"
    if rb > 1:
        return f"rows<{nht},13,{rb}>"
    if in_mask:
        return f"adam<{nht},13,true>"
    ntm = tune.get("l1b_nt_mask", 0)
    return f"adam<{nht},{13 if ntm == 0 or nht != 8 else (0 if ntm < 0 else ntm)}>"


def _make_cases():
    cases = []

    def add(kind, shapes, indrop=False, tune=None):
        every = len(shapes) <= 6                   # few shapes: each at all five (K, grid); else two of the five per shape
        for i, (width, n_b) in enumerate(shapes):
            for j, (K, grid) in enumerate(KGRID):
                if every or j in (i % 5, (i + 2) % 5):
                    # one row: the batch variance is 0, rstd = 31.6 and xhat = x scale + shift cancels from +-4000 gamma at
                    # x = 126 down to beta - the float32 reference itself is then 1e-3 off, so one-row cases stay at 0..2
                    xmax = 2 if n_b == 1 else (2, 126, 2, 255, 2)[(i + j) % 5]
                    cases.append((kind, width, n_b, K, grid, xmax, indrop, tune or {}, ("nan", "junk")[(i + j) % 2]))
    add("adam", [(w, n) for w in (8, 96, 256, 512, 600, 1024) for n in (1, 31, 32)])
    add("adam-in-dropout", [(w, n) for w in (64, 33, 256) for n in (7, 32)], indrop=True)
    add("rows-one-block", [(256, 17), (256, 32)], tune={"l1b_rows": 1})
    add("rows", [(w, n) for w in (64, 128, 256) for n in (33, 64, 65, 96, 97, 128)])
    add("big", [(w, n) for w in (64, 128, 256) for n in (129, 160, 257, 1000, 4095, 4096)])
    return cases


CASES = _make_cases()
CASE_IDS = [f"{c[0]}-w{c[1]}-n{c[2]}-K{c[3]}-grid{c[4]}-x{c[5]}" for c in CASES]


def _expected_form(kind, width, n_b):
    nht = -(-width // 32)
    return {"adam": f"adam<{nht},13>", "adam-in-dropout": f"adam<{nht},13,true>", "rows-one-block": "rows<8,13,1>",
            "rows": f"rows<{nht},13,{-(-n_b // 32)}>", "big": f"big<{nht}>"}[kind]


def test_cases_cover_every_form_shape_and_value_range():
    """Every form at K = 20, K = 97 and the three grids of K = 1000, and at genotypes 0..2, 0..126 and 0..255."""
    by_kind = {}
    for kind, width, n_b, K, grid, xmax, *_ in CASES:
        by_kind.setdefault(kind, []).append(((K, grid), xmax, (width, n_b)))
    assert set(by_kind) == {"adam", "adam-in-dropout", "rows-one-block", "rows", "big"}
    for kind, got in by_kind.items():
        assert {g[0] for g in got} == set(KGRID), kind
        assert {g[1] for g in got} == {2, 126, 255}, kind
    assert {g[2] for g in by_kind["big"]} == {(w, n) for w in (64, 128, 256) for n in (129, 160, 257, 1000, 4095, 4096)}
    assert {g[2] for g in by_kind["rows"]} == {(w, n) for w in (64, 128, 256) for n in (33, 64, 65, 96, 97, 128)}
    assert {g[2] for g in by_kind["adam"]} == {(w, n) for w in (8, 96, 256, 512, 600, 1024) for n in (1, 31, 32)}


def _case_problem(case):
    kind, width, n_b, K, grid, xmax, indrop, tune, poison_kind = case
    return _Problem(K, width, n_b, xmax, seed=1000 * width + 7 * n_b + K + grid, indrop=indrop)


def test_floors_leave_room_below_the_cap():
    """0 < F and MARGIN * F < CAP for the gradient run, the Adam run and the next step's bn4 of the largest and the
    smallest cases of every form (the device tests assert the same for each of their cases)."""
    picked = {}
    for case in CASES:
        picked.setdefault((case[0], "small"), case)
        picked[(case[0], "large")] = case
    for case in picked.values():
        prob = _case_problem(case)
        for which in ("gradient", "adam"):
            _, F = _floors(prob, which)
            assert all(0 < f and MARGIN_ONE_ROW * f < CAP for f in F), (case[:6], which, F)
        Fb = _vector_floor(prob.bn4_next(np.float32), prob.bn4_next(np.float64))
        assert all(0 < f and MARGIN_ONE_ROW * f < CAP for f in Fb), (case[:6], Fb)


# ------------------------------------------------------------------ the device side of the backward
NAMES_KH = ("w", "m", "v")
NAMES_K = ("gamma", "beta", "m_gamma", "v_gamma", "m_beta", "v_beta")
NAMES_H = ("b1", "m_b1", "v_b1")


class _Device:
    """The buffers of one loc_l1_backward_adam* call for a _Problem: every float buffer a guarded view of exactly the
    documented size."""

    def __init__(self, prob, poison_kind, dz_rows=None, rows_len=None):
        from locator_amd import _lib
        self.lib, self.prob, self.kind = _lib.load(), prob, poison_kind
        self.d = _lib.make_dims(prob.K, prob.width, 1 if prob.indrop else 2)
        K, Kp, Hp = prob.K, prob.Kp, prob.Hp
        assert (self.d.Kp, self.d.Hp) == (Kp, Hp)
        dev = "cuda"
        X = np.zeros((prob.n_samp + 1, Kp), np.uint8)
        X[:prob.n_samp, :K] = prob.x_all
        X[prob.n_samp, :K] = 255                                    # the sentinel row
        self.X = torch.from_numpy(X).to(dev)
        rows = np.full(max(rows_len or 0, prob.used + 64), prob.n_samp, np.int32)
        rows[:prob.n_b] = prob.rows
        self.rows = torch.from_numpy(rows).to(dev)
        self.mask = torch.from_numpy(prob.mask).to(dev) if prob.indrop else None
        tab = np.ones(ALPHA_LEN)
        t = np.arange(1, ALPHA_LEN, dtype=np.float64)
        tab[1:] = np.sqrt(1.0 - O.ADAM_B2 ** t) / (1.0 - O.ADAM_B1 ** t)
        self.alpha_tab = torch.from_numpy(tab.astype(np.float32)).to(dev)
        self.lr = torch.zeros(1, device=dev)
        self.t_base = torch.zeros(1, dtype=torch.int32, device=dev)
        self.dz_rows = dz_rows or prob.used
        sizes = {n: Kp * Hp for n in NAMES_KH}
        sizes.update({n: Kp for n in NAMES_K})
        sizes.update({n: Hp for n in NAMES_H})
        sizes.update(gbs=(Kp // 32) * 128, dz=self.dz_rows * Hp, bn4=4 * Kp, bn4_out=4 * Kp, next_stats=2 * Kp)
        self.g, self.checks = {}, []
        for name, n in sizes.items():
            self.g[name], chk = guarded(n, torch.float32, 128 * Hp)
            self.checks.append((name, chk))
        pad = lambda a, n: np.concatenate([np.asarray(a, np.float32), np.zeros(n - len(a), np.float32)])
        self.const = {"dz": np.zeros((self.dz_rows, Hp), np.float32),
                      "bn4": np.concatenate([pad(a, Kp) for a in prob.bn4]),
                      "next_stats": np.concatenate([pad(a, Kp) for a in prob.next_stats])}
        self.const["dz"][:prob.n_b, :prob.width] = prob.dz           # rows n_b.. and units width.. are exact zeros
        self.x_bits = bits_u8(self.X)

    def load(self, which):
        """Write the inputs of the gradient run or the Adam run; gb_scratch and bn4_out start out poisoned."""
        prob, K, Kp, Hp = self.prob, self.prob.K, self.prob.Kp, self.prob.Hp
        zeros = O.zeros_like_trainable(prob.p)
        m, v = (zeros, zeros) if which == "gradient" else prob.moments()
        put = lambda name, a: self.g[name].copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1)))
        pad = lambda a, n: np.concatenate([np.asarray(a, np.float32), np.zeros(n - len(a), np.float32)])
        for names, src in ((("w", "gamma", "beta", "b1"), prob.p), (("m", "m_gamma", "m_beta", "m_b1"), m),
                           (("v", "v_gamma", "v_beta", "v_b1"), v)):
            put(names[0], w1s_pack(src["W"][0], Kp, Hp))
            put(names[1], pad(src["gamma"], Kp))
            put(names[2], pad(src["beta"], Kp))
            put(names[3], pad(src["b"][0], Hp))
        for name, a in self.const.items():
            put(name, a)
        poison(self.g["gbs"], self.kind, 3)
        poison(self.g["bn4_out"], self.kind, 4)
        self.lr.fill_(1e-3 if which == "gradient" else LR_ADAM)
        self.t_base.fill_(0 if which == "gradient" else T_BASE)
        self.t_off = 1 if which == "gradient" else T_OFF
        torch.cuda.synchronize()
        self.before = self.state()

    def state(self):
        torch.cuda.synchronize()
        return {k: bits(t) for k, t in self.g.items()}

    def call(self, entry, grid, tune=None, n_b=None, with_next=False):
        """entry: "full" = loc_l1_backward_adam (loc_l1_backward_adam_in_dropout for an --nlayers 1 problem), "main" =
        loc_l1_backward_adam_main.  -> the return code."""
        from locator_amd import _lib
        g, lib, prob = self.g, self.lib, self.prob
        ptr = lambda n: g[n].data_ptr()
        n_b = prob.n_b if n_b is None else n_b
        tune_s = _lib.Tuning(**(tune or {}))
        head = [self.X.data_ptr(), self.X.stride(0), self.rows.data_ptr(), n_b, C.byref(self.d), ptr("bn4"), ptr("dz"),
                ptr("w"), ptr("m"), ptr("v")]
        gb = [ptr(n) for n in NAMES_K]
        mid = [ptr("b1"), ptr("m_b1"), ptr("v_b1"), ptr("gbs"), self.alpha_tab.data_ptr(), ALPHA_LEN, self.lr.data_ptr(),
               self.t_base.data_ptr(), self.t_off, grid]
        nxt = [ptr("next_stats") if with_next else None, ptr("bn4_out")]
        if entry == "main":
            assert not prob.indrop
            rc = lib.loc_l1_backward_adam_main(*head, *mid, C.byref(tune_s), None)
        elif prob.indrop:
            rc = lib.loc_l1_backward_adam_in_dropout(*head, *gb, *mid, *nxt, C.byref(tune_s), self.mask.data_ptr(),
                                                     KEEP_SCALE, None)
        else:
            rc = lib.loc_l1_backward_adam(*head, *gb, *mid, *nxt, None, C.byref(tune_s), None)
        torch.cuda.synchronize()
        return rc

    def check_margins(self):
        for name, chk in self.checks:
            chk(name)
        assert torch.equal(bits_u8(self.X), self.x_bits), "X was written"

    def read(self, names):
        """Oracle-format dict from the four buffers `names` = (W1-layout, gamma-like, beta-like, b1-like)."""
        K, H, Kp, Hp = self.prob.K, self.prob.width, self.prob.Kp, self.prob.Hp
        full = w1s_unpack(self.g[names[0]].cpu().numpy(), Kp, Hp)
        vec = lambda n: self.g[n].cpu().numpy()
        out = {"W": [full[:K, :H]], "gamma": vec(names[1])[:K], "beta": vec(names[2])[:K], "b": [vec(names[3])[:H]]}
        padding = np.concatenate([full[K:].ravel(), full[:, H:].ravel(), vec(names[1])[K:], vec(names[2])[K:],
                                  vec(names[3])[H:]])
        return out, padding

    def results(self):
        """-> {"p", "m", "v"} oracle-format dicts; asserts that every padded entry is exactly 0."""
        out = {}
        for grp, names in (("p", ("w", "gamma", "beta", "b1")), ("m", ("m", "m_gamma", "m_beta", "m_b1")),
                           ("v", ("v", "v_gamma", "v_beta", "v_b1"))):
            out[grp], padding = self.read(names)
            assert not padding.any(), f"{grp}: padding (k >= K or h >= width) is not exactly 0"
        return out


def bits_u8(t):
    return t.detach().contiguous().view(-1).cpu()


def _report(label, dist, floors, sums_margin=MARGIN):
    """Print device / F per class, then hold every class to its margin x its floor: MARGIN, and sums_margin for the two
    classes that contain the gamma / beta sums (per tensor and per element)."""
    names = ("tensor", "tile", "element")
    margins = (sums_margin, MARGIN, sums_margin)
    worst = [max(d, key=d.get) for d in dist]
    print(f"{label}: " + " | ".join(f"{n} F {f:.2e} device {d[k]:.2e} ({k}) ratio {d[k] / f:.2f}"
                                    for n, f, d, k in zip(names, floors, dist, worst)))
    for n, f, d, k, mg in zip(names, floors, dist, worst, margins):
        assert 0 < f and mg * f < CAP, (label, n, f)
        assert d[k] <= mg * f, (label, n, k, d[k], f)
    if sums_margin != MARGIN:                                   # ... and W1 / b1 stay at MARGIN there too
        for n, f, d in zip(names, floors, dist):
            rest = {k: e for k, e in d.items() if not k.endswith(("gamma", "beta"))}
            assert max(rest.values()) <= MARGIN * f, (label, n, rest, f)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_l1_backward_adam_against_the_reference(case):
    """One form of the layer-1 backward: gradient run (m' = 0.1 g, v' = 0.001 g^2 per tensor, per tile and per element;
    loc_l1_backward_adam_main leaves the same bits and slot 0 + slot 1 of gb_scratch = dgamma / dbeta), Adam run (w' - w,
    m', v' and the next step's bn4 against a float64 step from the float64 gradient), padding exactly 0, the same call twice
    the same bits, inputs and every guard margin intact."""
    kind, width, n_b, K, grid, xmax, indrop, tune, poison_kind = case
    prob = _case_problem(case)
    assert _form(n_b, prob.Hp, indrop, tune) == _expected_form(kind, width, n_b)
    s = _Device(prob, poison_kind)
    label = f"l1 {CASE_IDS[CASES.index(case)]}"
    inputs = ("dz", "bn4", "next_stats")

    # 1. the gradient run; no bn_next_stats: bn4_out stays as it was
    s.load("gradient")
    assert s.call("full", grid, tune) == 0, s.lib.loc_last_error()
    s.check_margins()
    after = s.state()
    for name in inputs + ("bn4_out",):
        assert torch.equal(after[name], s.before[name]), f"{name} was written"
    got = s.results()
    ref, F = _floors(prob, "gradient")
    sums_margin = MARGIN_ONE_ROW if n_b == 1 else MARGIN
    _report(label + " gradient", _distances({"m": got["m"], "v": got["v"]}, ref), F, sums_margin)

    # ... and through loc_l1_backward_adam_main: the same W1 / m / v / b1, gamma and beta left alone, the two slots
    if not indrop:
        s.load("gradient")
        assert s.call("main", grid, tune) == 0, s.lib.loc_last_error()
        s.check_margins()
        main = s.state()
        for name in NAMES_KH + NAMES_H + ("gbs",):
            assert torch.equal(main[name], after[name]), f"main: {name} differs from loc_l1_backward_adam"
        for name in NAMES_K + inputs + ("bn4_out",):
            assert torch.equal(main[name], s.before[name]), f"main: {name} was written"
        gbs = s.g["gbs"].cpu().numpy().reshape(prob.Kp // 32, 2, 2, 32)                 # [k-tile][slot][dgamma|dbeta][32]
        slots = (gbs[:, 0] + gbs[:, 1]).transpose(1, 0, 2).reshape(2, prob.Kp)[:, :K]
        g64, g32 = prob.grads(np.float64), prob.grads(np.float32)
        want = np.stack([g64["gamma"], g64["beta"]])
        Fg = _vector_floor(np.stack([g32["gamma"], g32["beta"]]), want)
        dg = _vector_floor(slots, want)
        print(f"{label} gbs: F {Fg[0]:.2e} device {dg[0]:.2e} ratio {dg[0] / Fg[0]:.2f} | element F {Fg[1]:.2e} device "
              f"{dg[1]:.2e} ratio {dg[1] / Fg[1]:.2f}")
        assert all(0 < f and sums_margin * f < CAP for f in Fg), Fg
        assert dg[0] <= sums_margin * Fg[0] and dg[1] <= sums_margin * Fg[1], (dg, Fg)

    # 2. the Adam run, with the next minibatch's statistics
    s.load("adam")
    assert s.call("full", grid, tune, with_next=True) == 0, s.lib.loc_last_error()
    s.check_margins()
    after = s.state()
    for name in inputs:
        assert torch.equal(after[name], s.before[name]), f"{name} was written"
    got = s.results()
    ref, F = _floors(prob, "adam")
    start = O.cast_params(prob.p, np.float64)
    _report(label + " adam", _distances({"m": got["m"], "v": got["v"], "dw": _delta(got["p"], start)}, ref), F)
    out = s.g["bn4_out"].cpu().numpy().reshape(4, prob.Kp)
    want = prob.bn4_next(np.float64)
    Fb, db = _vector_floor(prob.bn4_next(np.float32), want), _vector_floor(out[:, :K], want)
    print(f"{label} bn4_out: F {Fb[0]:.2e} device {db[0]:.2e} ratio {db[0] / Fb[0]:.2f} | element F {Fb[1]:.2e} device "
          f"{db[1]:.2e} ratio {db[1] / Fb[1]:.2f}")
    assert all(0 < f and MARGIN * f < CAP for f in Fb), Fb
    assert db[0] <= MARGIN * Fb[0] and db[1] <= MARGIN * Fb[1], (db, Fb)
    assert torch.equal(after["bn4_out"].view(4, prob.Kp)[:, K:], s.before["bn4_out"].view(4, prob.Kp)[:, K:])

    # 3. the same call again: the same bits everywhere
    s.load("adam")
    assert s.call("full", grid, tune, with_next=True) == 0, s.lib.loc_last_error()
    again = s.state()
    for name in after:
        assert torch.equal(again[name], after[name]), f"{name}: two identical calls differ"
    s.check_margins()


@pytest.mark.gpu
def test_l1_backward_cache_policy_hints_change_no_bit():
    """l1b_nt_mask 0 (default), 9, 15 and -1 at width 256 pick four instantiations of l1_bwd_adam_kernel<8, NTM> that
    differ in the cache policy of their streams only: every buffer bit-identical."""
    prob = _Problem(1000, 256, 31, 2, seed=11)
    s = _Device(prob, "junk")
    forms, states = set(), []
    for ntm in (0, 9, 15, -1):
        forms.add(_form(31, 256, False, {"l1b_nt_mask": ntm}))
        s.load("adam")
        assert s.call("full", 5, {"l1b_nt_mask": ntm}, with_next=True) == 0, s.lib.loc_last_error()
        states.append(s.state())
        s.check_margins()
    assert forms == {"adam<8,13>", "adam<8,9>", "adam<8,15>", "adam<8,0>"}
    assert not torch.equal(states[0]["w"], s.before["w"])
    for st in states[1:]:
        for name in st:
            assert torch.equal(st[name], states[0][name]), name


@pytest.mark.gpu
@pytest.mark.parametrize("width,n_b,indrop", [(256, 0, False), (256, 4097, False), (512, 33, False), (96, 33, False),
                                              (64, 33, True), (512, 129, False)],
                         ids=["n_b-0", "n_b-4097", "n_b-33-width-512", "n_b-33-width-96", "n_b-33-in-dropout",
                              "n_b-129-width-512"])
def test_l1_backward_refusals_write_nothing(width, n_b, indrop):
    """Row counts outside 1..LOC_BIG_BATCH_MAX, more than 32 rows at a width without a row-block form or with Dropout on
    the BatchNorm output: nonzero, a message, and no bit of any buffer written (the buffers are sized for the call as
    if it were valid)."""
    prob = _Problem(97, width, 20, 2, seed=5, indrop=indrop)
    rows_alloc = -(-max(n_b, 32) // 32) * 32
    s = _Device(prob, "nan", dz_rows=rows_alloc, rows_len=rows_alloc + 64)
    for entry in ("full",) if indrop else ("full", "main"):
        s.load("adam")
        rc = s.call(entry, 3, n_b=n_b, with_next=True)
        assert rc != 0 and s.lib.loc_last_error().decode(), (rc, entry)
        after = s.state()
        for name in after:
            assert torch.equal(after[name], s.before[name]), (entry, name)
        s.check_margins()


# ------------------------------------------------------------------ the two small forward forms
FWD_CASES = [(w, n, K, grid, form) for form, widths in (("in-dropout", (64, 33)), ("dropout-on-output", (64, 33, 256)))
             for w in widths for n in (7, 32) for K, grid in ((97, 3), (1000, 5))]


def _fwd_ref(prob, mask_out, dt):
    p = O.cast_params(prob.p, dt)
    sc, sh = (np.asarray(a).astype(dt) for a in prob.bn4[:2])
    xhat = prob.x.astype(dt) * sc + sh
    if prob.indrop:
        xhat = xhat * (prob.mask[:prob.n_b, :prob.K].astype(dt) * dt(KEEP_SCALE))
    a1 = O.elu(xhat @ p["W"][0] + p["b"][0])
    return a1, (None if mask_out is None else a1 * (mask_out.astype(dt) * dt(KEEP_SCALE)))


@pytest.mark.gpu
@pytest.mark.parametrize("width,n_b,K,grid,form", FWD_CASES, ids=[f"{c[4]}-w{c[0]}-n{c[1]}-K{c[2]}" for c in FWD_CASES])
def test_l1_forward_small_forms_against_the_reference(width, n_b, K, grid, form):
    """loc_l1_forward_in_dropout (keep flags on the BatchNorm output) and loc_l1_forward with Dropout on its output (a1 and
    a1_drop) against the float64 contraction, the float32 one as the floor (per tensor and per row); partial of exactly
    grid * 32 * Hp floats, a1 / a1_drop of 32 * Hp, all poisoned; rows >= n_b of the block stay finite, padded units 0."""
    from locator_amd import _lib
    indrop = form == "in-dropout"
    prob = _Problem(K, width, n_b, 126 if K == 97 else 2, seed=width + n_b + K, indrop=indrop)
    s = _Device(prob, "nan")
    s.load("gradient")
    Hp, Kp = prob.Hp, prob.Kp
    bufs, checks = {}, []
    for name, n in (("partial", grid * 32 * Hp), ("a1", 32 * Hp), ("a1_drop", 32 * Hp)):
        bufs[name], chk = guarded(n, torch.float32, 128 * Hp)
        checks.append((name, chk))
        poison(bufs[name], "nan" if n_b == 7 else "junk", len(name))
    mask_out = None if indrop else (prob.rng.random((32, Hp)) >= 0.25).astype(np.uint8)
    mask_dev = None if indrop else torch.from_numpy(mask_out).cuda()
    drop_before = bits(bufs["a1_drop"])
    common = [s.X.data_ptr(), s.X.stride(0), s.rows.data_ptr(), n_b, C.byref(s.d), s.g["bn4"].data_ptr(), s.g["w"].data_ptr(),
              s.g["b1"].data_ptr(), bufs["partial"].data_ptr(), grid, bufs["a1"].data_ptr()]
    if indrop:
        rc = s.lib.loc_l1_forward_in_dropout(*common, s.mask.data_ptr(), KEEP_SCALE, None)
    else:
        rc = s.lib.loc_l1_forward(*common, bufs["a1_drop"].data_ptr(), mask_dev.data_ptr(), KEEP_SCALE, None)
    torch.cuda.synchronize()
    assert rc == 0, s.lib.loc_last_error()
    for name, chk in checks:
        chk(name)
    s.check_margins()
    after = s.state()
    for name in after:
        assert torch.equal(after[name], s.before[name]), f"the forward wrote {name}"
    a1 = bufs["a1"].view(32, Hp).cpu().numpy()
    assert np.isfinite(a1).all() and not a1[:n_b, width:].any()
    m_used = None if indrop else mask_out[:n_b, :width]
    r64, r32 = _fwd_ref(prob, m_used, np.float64), _fwd_ref(prob, m_used, np.float32)
    got = [a1[:n_b, :width]]
    if indrop:
        assert torch.equal(bits(bufs["a1_drop"]), drop_before), "a1_drop written without a mask"
    else:
        ad = bufs["a1_drop"].view(32, Hp).cpu().numpy()
        assert np.isfinite(ad).all()
        assert np.array_equal(ad, a1 * (mask_out.astype(np.float32) * np.float32(KEEP_SCALE))), "a1_drop != a1 * mask * keep_scale"
        got.append(ad[:n_b, :width])
    for name, g, a, b in zip(("a1", "a1_drop"), got, r32, r64):
        F = float(_rel(np.linalg.norm(a - b), np.linalg.norm(b))), _vector_floor(a, b)[0]
        dev = float(_rel(np.linalg.norm(g - b), np.linalg.norm(b))), _vector_floor(g, b)[0]
        print(f"l1 forward {form} width {width} n_b {n_b} K {K} {name}: F {F[0]:.2e} device {dev[0]:.2e} ratio "
              f"{dev[0] / F[0]:.2f} | F_row {F[1]:.2e} device {dev[1]:.2e} ratio {dev[1] / F[1]:.2f}")
        assert all(0 < f and MARGIN_SMALL * f < CAP for f in F), F
        assert dev[0] <= MARGIN_SMALL * F[0] and dev[1] <= MARGIN_SMALL * F[1], (name, dev, F)


# ------------------------------------------------------------------ BatchNorm statistics
COLUMN_KINDS = ("0..2", "constant", "all-255", "alternating", "0..126", "0..255")


def _bn_matrix(rng, batch, n_steps, K, shift):
    """[n_steps][batch][K] uint8; column k is of kind COLUMN_KINDS[(k + shift) % 6]: random values of the three ranges,
    one value per minibatch (variance exactly 0), 255 everywhere, 0 / 255 alternating along the rows."""
    x = np.zeros((n_steps, batch, K), np.uint8)
    for k in range(K):
        kind = COLUMN_KINDS[(k + shift) % 6]
        if kind == "constant":
            x[:, :, k] = rng.integers(0, 256, (n_steps, 1))
        elif kind == "all-255":
            x[:, :, k] = 255
        elif kind == "alternating":
            x[:, :, k] = (255 * ((np.arange(batch) + k) % 2))[None, :]
        else:
            hi = {"0..2": 2, "0..126": 126, "0..255": 255}[kind]
            x[:, :, k] = rng.integers(0, hi + 1, (n_steps, batch))
    return x


class _BN:
    """One epoch's minibatches on the device and their exact statistics."""

    def __init__(self, K, batch, n_steps, n_last, shift, seed):
        from locator_amd import _lib
        self.lib = _lib.load()
        rng = np.random.default_rng(seed)
        self.K, self.Kp, self.batch, self.n_steps, self.n_last = K, -(-K // 32) * 32, batch, n_steps, n_last
        Kp, n_rows = self.Kp, n_steps * batch
        x = _bn_matrix(rng, batch, n_steps, K, shift)
        place = rng.permutation(n_rows)                          # minibatch row (step, b) lives in row place[...] of X
        X = np.zeros((n_rows + 1, Kp), np.uint8)
        X[place, :K] = x.reshape(n_rows, K)
        X[n_rows, :K] = 255                                      # the sentinel row
        rows = np.full(n_rows + 64, n_rows, np.int32)
        for j in range(n_steps):
            n = n_last if j == n_steps - 1 else batch
            rows[j * batch:j * batch + n] = place[j * batch:j * batch + n]
        self.X, self.rows = torch.from_numpy(X).cuda(), torch.from_numpy(rows).cuda()
        # exact statistics: integers, then one float64 division (the numerator stays below 2^53)
        self.mean, self.var = np.zeros((n_steps, K)), np.zeros((n_steps, K))
        self.n = [n_last if j == n_steps - 1 else batch for j in range(n_steps)]
        for j, n in enumerate(self.n):
            xi = x[j, :n].astype(np.int64)
            s_, ss = xi.sum(0), (xi * xi).sum(0)
            num = n * ss - s_ * s_
            assert num.max() < 2 ** 53 and num.min() >= 0
            self.mean[j], self.var[j] = s_ / n, num / float(n * n)
            self.largest_numerator = int(num.max())
        kinds = [COLUMN_KINDS[(k + shift) % 6] for k in range(K)]
        self.const_cols = np.array([kind in ("constant", "all-255") for kind in kinds])
        if batch == BIG_BATCH_MAX and n_last == batch and "alternating" in kinds:
            assert self.largest_numerator > 2 ** 31              # 4096 rows of 0 / 255: 2.7e11, the 64-bit path
        f32 = lambda a: np.asarray(a, np.float32)
        pad = lambda a: np.concatenate([f32(a), np.zeros(Kp - K, np.float32)])
        self.gamma, self.beta = pad(rng.uniform(0.7, 1.3, K)), pad(rng.normal(0, 0.05, K))
        self.mov0 = pad(rng.uniform(0, 2, K)), pad(rng.uniform(0.2, 1.2, K))
        self.gamma_t, self.beta_t = torch.from_numpy(self.gamma).cuda(), torch.from_numpy(self.beta).cuda()
        self.g, self.checks = {}, []
        for name, size in (("stats_ep", n_steps * 2 * Kp), ("bn4", 4 * Kp), ("mov_mean", Kp), ("mov_var", Kp)):
            self.g[name], chk = guarded(size, torch.float32, 4096)
            self.checks.append((name, chk))

    def reset(self, kind):
        poison(self.g["stats_ep"], kind, 1)
        poison(self.g["bn4"], kind, 2)
        self.g["mov_mean"].copy_(torch.from_numpy(self.mov0[0]))
        self.g["mov_var"].copy_(torch.from_numpy(self.mov0[1]))
        torch.cuda.synchronize()
        self.before = self.state()

    def state(self):
        torch.cuda.synchronize()
        return {k: bits(t) for k, t in self.g.items()}

    def args(self, batch=None, n_last=None):
        return [self.X.data_ptr(), self.X.stride(0), self.rows.data_ptr(), self.batch if batch is None else batch,
                self.n_last if n_last is None else n_last, self.n_steps, self.K, self.Kp]

    def gb_mov(self):
        return [self.gamma_t.data_ptr(), self.beta_t.data_ptr(), self.g["mov_mean"].data_ptr(), self.g["mov_var"].data_ptr()]

    def epoch_stats(self, unit=None, **kw):
        tail = [self.g["stats_ep"].data_ptr(), self.g["bn4"].data_ptr()]
        if unit is None:
            rc = self.lib.loc_bn_epoch_stats(*self.args(**kw), *self.gb_mov(), *tail, None)
        else:
            rc = self.lib.loc_bn_epoch_stats_unit(*self.args(**kw), *self.gb_mov(), *tail, unit, None)
        return rc, self.state()

    def stats_only(self, unit=None, **kw):
        if unit is None:
            rc = self.lib.loc_bn_epoch_stats_only(*self.args(**kw), self.g["stats_ep"].data_ptr(), None)
        else:
            rc = self.lib.loc_bn_epoch_stats_only_unit(*self.args(**kw), self.g["stats_ep"].data_ptr(), unit, None)
        return rc, self.state()

    def finish(self, with_bn4=True):
        rc = self.lib.loc_bn_epoch_finish(self.n_steps, self.K, self.Kp, *self.gb_mov(), self.g["stats_ep"].data_ptr(),
                                          self.g["bn4"].data_ptr() if with_bn4 else None, None)
        return rc, self.state()

    def check_margins(self):
        for name, chk in self.checks:
            chk(name)


def _moving(mov0, mean, var, dt):
    """The n_steps moving-statistics updates in dt from per-step statistics [n_steps][K] -> (mov_mean, mov_var)."""
    mom = dt(O.BN_MOMENTUM)
    mm, mv = mov0[0].astype(dt), mov0[1].astype(dt)
    for mu, va in zip(mean, var):
        mm = mm * mom + mu.astype(dt) * (dt(1) - mom)
        mv = mv * mom + va.astype(dt) * (dt(1) - mom)
    return mm, mv


BN_SHAPES = [(K, batch) for K in (1, 31, 33, 257) for batch in (1, 7, 32, 33, 300, 4096)]


@pytest.mark.gpu
@pytest.mark.parametrize("K,batch", BN_SHAPES, ids=[f"K{K}-batch{b}" for K, b in BN_SHAPES])
def test_bn_statistics_against_exact_integers(K, batch):
    """n_steps 1 and 3, a last step of 1 row and of `batch` rows, columns of every kind (K = 1: each kind in turn): mean within
    1 ulp of s / n and exact where s / n is an fp32 number; variance within 2 ulp of the exact rational (it rounds twice)
    and exactly 0 for a column that is constant within the minibatch; bn4 of step 0 and the moving statistics against
    float64 (floor: the fp32 NumPy form, and never below the format's half-ulp 2^-24); zeros beyond K; the split, NULL-bn4, unit-1 and unit-63 identities bit for
    bit; loc_bn_batch_stats = step 0 of the epoch form; every margin intact."""
    combos = [(n_steps, n_last, shift) for n_steps in (1, 3) for n_last in sorted({1, batch})
              for shift in (range(6) if K == 1 else (0,))]
    for ci, (n_steps, n_last, shift) in enumerate(combos):
        s = _BN(K, batch, n_steps, n_last, shift, seed=K + batch + 10 * n_steps + n_last)
        Kp, kind = s.Kp, ("nan", "junk")[ci % 2]
        s.reset(kind)
        rc, full = s.epoch_stats()
        assert rc == 0, s.lib.loc_last_error()
        s.check_margins()
        st = s.g["stats_ep"].cpu().numpy().reshape(n_steps, 2, Kp)
        mean, var = st[:, 0, :K].astype(np.float64), st[:, 1, :K].astype(np.float64)
        assert not st[:, :, K:].view(np.int32).any(), "stats_ep is not exactly 0 beyond K"
        assert (np.abs(mean - s.mean) <= ulp32(s.mean)).all(), np.abs(mean - s.mean).max()
        exact = s.mean.astype(np.float32).astype(np.float64) == s.mean
        assert (mean[exact] == s.mean[exact]).all()
        assert (np.abs(var - s.var) <= 2 * ulp32(s.var)).all(), (np.abs(var - s.var) / ulp32(s.var)).max()
        assert not var[:, s.const_cols].any() and (var[s.var == 0] == 0).all()
        if n_last == 1:
            assert not var[-1].any()

        # bn4 of step 0 and the moving statistics after n_steps
        bn4 = s.g["bn4"].cpu().numpy().reshape(4, Kp)
        assert not bn4[:, K:].view(np.int32).any(), "bn4 is not exactly 0 beyond K"
        g64, b64 = s.gamma[:K].astype(np.float64), s.beta[:K].astype(np.float64)
        want = np.stack(_bn4_from(s.mean[0], s.var[0], g64, b64))
        floor = np.stack(_bn4_from(s.mean[0].astype(np.float32), s.var[0].astype(np.float32), s.gamma[:K], s.beta[:K]))
        mov = np.stack([s.g["mov_mean"].cpu().numpy()[:K], s.g["mov_var"].cpu().numpy()[:K]])
        mov0 = (s.mov0[0][:K], s.mov0[1][:K])
        want_mov = np.stack(_moving(mov0, s.mean, s.var, np.float64))
        floor_mov = np.stack(_moving(mov0, s.mean.astype(np.float32), s.var.astype(np.float32), np.float32))
        assert not s.g["mov_mean"].cpu().numpy()[K:].any() and not s.g["mov_var"].cpu().numpy()[K:].any()
        for name, got, w, f in (("bn4", bn4[:, :K], want, floor), ("moving", mov, want_mov, floor_mov)):
            # K = 1 leaves one number per row, and one fp32 rounding can land anywhere from 0 to half an ulp from the truth:
            # no floor counts below 2^-24, the relative half-ulp of the format
            F, dv = tuple(max(x, 2.0 ** -24) for x in _vector_floor(f, w)), _vector_floor(got, w)
            print(f"bn K {K} batch {batch} steps {n_steps} last {n_last} shift {shift} {name}: F {F[0]:.2e} device "
                  f"{dv[0]:.2e} ratio {dv[0] / F[0]:.2f} | element F {F[1]:.2e} device {dv[1]:.2e} ratio {dv[1] / F[1]:.2f}")
            assert all(MARGIN_SMALL * x < CAP for x in F), (name, F)
            assert dv[0] <= MARGIN_SMALL * F[0] and dv[1] <= MARGIN_SMALL * F[1], (name, dv, F)

        # identities, bit for bit
        s.reset(kind)
        rc, half = s.stats_only()
        assert rc == 0 and torch.equal(half["stats_ep"], full["stats_ep"])
        for name in ("bn4", "mov_mean", "mov_var"):
            assert torch.equal(half[name], s.before[name]), f"loc_bn_epoch_stats_only wrote {name}"
        rc, fin = s.finish(with_bn4=False)
        assert rc == 0 and torch.equal(fin["bn4"], s.before["bn4"]), "loc_bn_epoch_finish(bn4 = NULL) wrote bn4"
        assert torch.equal(fin["mov_mean"], full["mov_mean"]) and torch.equal(fin["mov_var"], full["mov_var"])
        s.reset(kind)
        assert s.stats_only()[0] == 0
        rc, both = s.finish()
        assert rc == 0
        for name in full:
            assert torch.equal(both[name], full[name]), f"stats_only + finish != loc_bn_epoch_stats in {name}"
        s.reset(kind)
        rc, u1 = s.epoch_stats(unit=1)
        assert rc == 0
        for name in full:
            assert torch.equal(u1[name], full[name]), f"unit 1 differs from the GT form in {name}"
        s.reset(kind)
        rc, u1 = s.stats_only(unit=1)
        assert rc == 0 and torch.equal(u1["stats_ep"], full["stats_ep"])
        s.reset(kind)
        rc, u63 = s.stats_only(unit=63)
        assert rc == 0
        st63 = s.g["stats_ep"].cpu().numpy().reshape(n_steps, 2, Kp)
        add = np.float32(s.lib.loc_bn_var_add(63))
        assert add == np.float32(63 * 63 - 1) * np.float32(1e-3)
        assert np.array_equal(st63[:, 0], st[:, 0]) and np.array_equal(st63[:, 1, :K], st[:, 1, :K] + add)
        assert not st63[:, :, K:].view(np.int32).any()
        s.reset(kind)
        rc, e63 = s.epoch_stats(unit=63)
        assert rc == 0 and torch.equal(e63["stats_ep"], u63["stats_ep"])
        s.check_margins()

        # loc_bn_batch_stats (<= 32 rows) = step 0 of the epoch form
        if n_steps == 1 and n_last <= 32:
            s.reset(kind)
            rc = s.lib.loc_bn_batch_stats(s.X.data_ptr(), s.X.stride(0), s.rows.data_ptr(), n_last, K, Kp, *s.gb_mov(),
                                          s.g["bn4"].data_ptr(), None)
            one = s.state()
            assert rc == 0, s.lib.loc_last_error()
            s.check_margins()
            assert torch.equal(one["stats_ep"], s.before["stats_ep"])
            b1_, bf = one["bn4"].view(4, Kp), full["bn4"].view(4, Kp)
            for q in (0, 2, 3):                                    # scale, mean, rstd: the same single operations
                assert torch.equal(b1_[q], bf[q]), q
            # shift = beta - mean * scale, mov = mov * 0.99 + stat * 0.01: two operations that a compiler may or may not
            # fuse, each form within one ulp of the largest term of the other
            f = lambda t: t.view(torch.float32).numpy().astype(np.float64)
            term = np.maximum(np.abs(f(bf[2]) * f(bf[0])), np.abs(s.beta))
            assert (np.abs(f(b1_[1]) - f(bf[1])) <= ulp32(term)).all()
            for name, m0 in (("mov_mean", s.mov0[0]), ("mov_var", s.mov0[1])):
                assert (np.abs(f(one[name]) - f(full[name])) <= ulp32(np.maximum(np.abs(m0), np.abs(f(full[name]))))).all(), name


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [dict(batch=4097, n_last=4097), dict(n_last=0), dict(n_last=8)],
                         ids=["batch-4097", "n_last-0", "n_last-above-batch"])
def test_bn_bad_arguments_write_nothing(bad):
    """batch above LOC_BIG_BATCH_MAX, n_last 0, n_last > batch: every epoch entry point returns nonzero with a message
    and writes no bit."""
    s = _BN(33, 7, 2, 7, 0, seed=3)
    calls = (lambda: s.epoch_stats(**bad), lambda: s.stats_only(**bad), lambda: s.epoch_stats(unit=63, **bad),
             lambda: s.stats_only(unit=63, **bad))
    for call in calls:
        s.reset("junk")
        rc, after = call()
        assert rc != 0 and s.lib.loc_last_error().decode()
        for name in after:
            assert torch.equal(after[name], s.before[name]), name
        s.check_margins()
