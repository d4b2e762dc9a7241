"""Shared by tests/test_stack_eval.py (no GPU) and tests/test_gpu_stack_eval.py: the inference hidden stack - layers 2..L,
Dense(2) x 2 and the distance (locator.py:319-325, :314-315) - as plain NumPy in float64 (the reference) and float32 (the
floor), the float32 emulation of the fused input stage's group sum, generators of exact (all-integer) and random cases, the
comparison, and a ctypes caller of loc_stack_forward_eval / _form / _partial on guarded buffers of exactly the documented
sizes.  Importing this module needs no GPU; torch is imported inside the caller only."""
from types import SimpleNamespace

import numpy as np

from oracle import locator_oracle as O

CAP = 1e-3          # margin x floor never above this
ABS_BAR = 2e-5      # absolute distance from float64 on the random cases: the bar of tests/test_gpu_stack_rows.py
# device / floor, measured on an MI355X over the 200 random cases of tests/test_gpu_stack_eval.py (ranges and where the largest
# occur: that file's header and DESIGN.md section 2); each margin is about twice the largest ratio of its group, rounded up
MARGIN_VALU = 4.0   # forms -1, -2, -3: 2 / 4 / 8 rows per workgroup on the vector ALU: largest 1.83 per tensor, 1.03 per row
MARGIN_MFMA = 6.0   # forms 1, 2: 32- and 16-row tiles on the fp32 matrix pipe: largest 2.77 per tensor (one row), 1.30 per row
FORMS = (-1, -2, -3, 1, 2)
ROWS_PER_WG = {-1: 2, -2: 4, -3: 8, 1: 32, 2: 16}
Y_EXTRA = 5         # rows of Y beyond n: `rows` is a permutation into a larger array


def margin_of(form):
    return MARGIN_VALU if form < 0 else MARGIN_MFMA


def _rel(num, den):
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    return np.where(den > 0, num / np.where(den > 0, den, 1.0), np.where(num == 0, 0.0, np.inf))


def row_scale(ref):
    """{tensor: the rms of its rows' L2 norms}: the size of a typical row."""
    return {k: float(np.sqrt(np.mean(np.sum(np.asarray(r, np.float64) ** 2, axis=1)))) for k, r in ref.items()}


def distances(got, ref, scale=None):
    """-> {tensor: relative L2 distance}, {tensor: the largest relative L2 distance of one row}, in float64: the _distances of
    tests/test_gpu_stack_train.py, except that a row is measured against its own norm or the typical row's (scale, default
    row_scale(ref)), whichever is larger.  The rows here hold two numbers (yhat) or one (dist), not a layer's units: a
    prediction near (0, 0) carries the rounding of sums of O(1) terms, and the largest error RELATIVE to such a row is the
    error of whichever row happens to lie closest to the origin - a figure that moves by a factor of ten from one draw to
    the next, in the float32 reference as on the device."""
    per_tensor, per_row = {}, {}
    scale = row_scale(ref) if scale is None else scale
    for k, r in ref.items():
        g, r = np.asarray(got[k], np.float64), np.asarray(r, np.float64)
        assert g.shape == r.shape, (k, g.shape, r.shape)
        per_tensor[k] = float(_rel(np.linalg.norm(g - r), np.linalg.norm(r)))
        per_row[k] = float(_rel(np.linalg.norm(g - r, axis=1), np.maximum(np.linalg.norm(r, axis=1), scale[k])).max())
    return per_tensor, per_row


# ------------------------------------------------------------------ the references
def ref_eval(a1, Wh, bh, wa, ba, wb, bb, Y_rows, dtype, trace=None):
    """Layers 2..L (Wh [L-1][Hp][Hp] input-major, bh [L-1][Hp]), the heads (wa [Hp][2], wb [2][2] input-major) and the distance
    to Y_rows [n][2] (None: no distance), every operand cast to `dtype` first.  -> {"yhat": [n][2], "dist": [n][1]}.
    trace: a list that receives (pre-activations, weights, bias, input) of every product, hidden layers first, then the
    two heads."""
    dt = np.dtype(dtype).type
    c = lambda v: np.asarray(v).astype(dt)
    a = c(a1)
    for W, b in zip(c(Wh), c(bh)):
        z = a @ W + b
        if trace is not None:
            trace.append((z, W, b, a))
        a = O.elu(z).astype(dt)
    y1 = a @ c(wa) + c(ba)
    y2 = y1 @ c(wb) + c(bb)
    if trace is not None:
        trace += [(y1, c(wa), c(ba), a), (y2, c(wb), c(bb), y1)]
    out = {"yhat": y2}
    if Y_rows is not None:
        e = y2 - c(Y_rows)
        out["dist"] = np.sqrt(np.maximum(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1], 0))[:, None]
    return out


def ref_case(case, dtype, a1=None, trace=None):
    """ref_eval on a case (its a1 unless another is given)."""
    return ref_eval(case.a1 if a1 is None else a1, case.Wh, case.bh, case.wa, case.ba, case.wb, case.bb,
                    case.Y[case.rows], dtype, trace)


def ref_partial_a1(partial, G, stride, cvec8, b1, n_b, Hp, assoc="documented", skip_group=None):
    """The fused input stage in float32 with the documented association (l1_gemm_reduce_kernel's): gq = (G + 3) / 4 groups
    per quarter, each quarter's groups added in ascending order into 0, ((q0 + q1) + q2) + q3, then + (c + b1) with
    c = ((cvec8[0] + cvec8[1]) + ...) + cvec8[7], then ELU.  partial: flat float32, group g of row m at g * stride + m * Hp.
    assoc = "right" combines the quarters as q0 + (q1 + (q2 + q3)); skip_group leaves one group out (what a wrong kernel
    might do: tests/test_stack_eval.py).  -> a1 [n_b][Hp] float32."""
    f = np.float32
    partial = np.asarray(partial, f)
    gq = (G + 3) // 4
    sq = []
    for q in range(4):
        z = np.zeros((n_b, Hp), f)
        for g in range(q * gq, min(q * gq + gq, G)):
            if g != skip_group:
                z = (z + partial[g * stride:g * stride + n_b * Hp].reshape(n_b, Hp)).astype(f)
        sq.append(z)
    s = ((sq[0] + sq[1]) + sq[2]) + sq[3] if assoc == "documented" else sq[0] + (sq[1] + (sq[2] + sq[3]))
    cv = np.asarray(cvec8, f).reshape(8, Hp)
    c = cv[0]
    for sl in range(1, 8):
        c = (c + cv[sl]).astype(f)
    z = (s + (c + np.asarray(b1, f))).astype(f)
    with np.errstate(over="ignore"):
        return O.elu(z).astype(f)


def partial_a1_f64(partial, G, stride, cvec8, b1, n_b, Hp):
    """The same stage in float64 (any order): the reference for random partial sums."""
    p = np.asarray(partial, np.float64)
    s = sum(p[g * stride:g * stride + n_b * Hp].reshape(n_b, Hp) for g in range(G))
    return O.elu(s + np.asarray(cvec8, np.float64).reshape(8, Hp).sum(0) + np.asarray(b1, np.float64))


# ------------------------------------------------------------------ the cases
def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _case(n, H, Hp, L, a1, Wh, bh, wa, ba, wb, bb, Y, rows, kind):
    return SimpleNamespace(n=n, H=H, Hp=Hp, L=L, a1=_f32(a1), Wh=_f32(Wh), bh=_f32(bh), wa=_f32(wa), ba=_f32(ba), wb=_f32(wb),
                           bb=_f32(bb), Y=_f32(Y), rows=np.ascontiguousarray(rows, dtype=np.int32), kind=kind)


def exact_nz(L):
    return 2 if L > 4 else 4 if L >= 3 else 8


def _pythagorean(rng, n):
    """n integer error vectors e with |e| < 2896 (e0^2 + e1^2 < 2^24) whose length is an integer."""
    out = np.zeros((n, 2))
    for b in range(n):
        kind = b % 6
        if kind == 1:
            out[b] = (rng.integers(1, 2896), 0)
        elif kind == 2:
            out[b] = (0, rng.integers(1, 2896))
        elif kind >= 3:
            x, y, h = ((3, 4, 5), (5, 12, 13), (8, 15, 17))[kind - 3]
            m = rng.integers(1, (2895 // h) + 1)
            v = (m * x, m * y) if rng.integers(2) else (m * y, m * x)
            out[b] = v * rng.choice([-1, 1], 2)
    return out


def exact_case(n, H, Hp, L, seed):
    """A stack whose every value is an integer below 2^24 in every partial sum of every order, so that fp32 in any
    summation order, fused or not, gives float64's bits.  The conditions are asserted here."""
    rng = np.random.default_rng(seed)
    nz = exact_nz(L)
    a1 = np.zeros((n, Hp))
    a1[:, :H] = rng.integers(0, 4, (n, H))
    Wh, bh = np.zeros((L - 1, Hp, Hp)), np.zeros((L - 1, Hp))
    cols = np.arange(H)
    for l in range(L - 1):
        for q in range(nz):                      # one weight 1 in each of nz equal ranges of the real input units
            lo, hi = q * H // nz, (q + 1) * H // nz
            Wh[l, rng.integers(lo, hi, H), cols] = 1
        bh[l, :H] = rng.integers(0, 3, H)
    wa = np.zeros((Hp, 2))
    wa[:H] = rng.integers(-1, 2, (H, 2))
    ba = rng.integers(-3, 4, 2).astype(float)
    while True:
        wb = rng.integers(-3, 4, (2, 2)).astype(float)
        if wb[0, 1] != wb[1, 0] and abs(np.linalg.det(wb)) > 0.5:
            break
    bb = rng.integers(-3, 4, 2).astype(float)
    rows = rng.permutation(n + Y_EXTRA)[:n]
    Y = rng.integers(-1000, 1000, (n + Y_EXTRA, 2)).astype(float)
    case = _case(n, H, Hp, L, a1, Wh, bh, wa, ba, wb, bb, Y, rows, "exact")
    for _ in range(100):                         # rows whose y2 repeats an earlier row's are drawn again: swapped rows must show
        trace = []
        y2 = ref_case(case, np.float64, trace=trace)["yhat"]
        again = np.setdiff1d(np.arange(n), np.unique(y2, axis=0, return_index=True)[1])
        if again.size == 0:
            break
        case.a1[again, :H] = rng.integers(0, 4, (again.size, H))
    case.Y[case.rows] = y2 - _pythagorean(rng, n)
    check_exact(case, trace, y2)
    return case


def check_exact(case, trace=None, y2=None):
    """The conditions of an exact case: integers everywhere, hidden pre-activations >= 0, the sum of absolute terms of every
    dot product below 2^24, integer distances with e0^2 + e1^2 < 2^24, rows of y2 distinct in at least n - 2 cases."""
    if trace is None:
        trace = []
        y2 = ref_case(case, np.float64, trace=trace)["yhat"]
    n, lim = case.n, 2.0 ** 24
    for i, (z, W, b, a) in enumerate(trace):
        assert np.array_equal(z, np.rint(z)) and np.array_equal(a, np.rint(a)), i
        assert i >= len(trace) - 2 or z.min() >= 0, i
        assert (np.abs(a) @ np.abs(W) + np.abs(b)).max() < lim, i
    assert not case.a1[:, case.H:].any() and not trace[-2][3][:, case.H:].any()
    Yr = case.Y[case.rows].astype(np.float64)
    assert np.array_equal(Yr, np.rint(Yr)) and np.abs(Yr).max() < lim and np.array_equal(Yr.astype(np.float32), Yr)
    e = y2 - Yr
    ss = (e * e).sum(1)
    assert ss.max() < lim and np.array_equal(np.rint(np.sqrt(ss)) ** 2, ss)
    assert len(np.unique(y2, axis=0)) >= n - 2, (len(np.unique(y2, axis=0)), n)
    assert len(np.unique(case.rows)) == n and case.Y.shape[0] > n
    return max(np.abs(t[0]).max() for t in trace)


def random_case(n, H, Hp, L, seed):
    """Weights on the scale of make_problem / randomize_params (glorot_uniform kernels, N(0, 0.05) biases), a1 = float32 ELU
    outputs of N(0, 1), targets N(0, 1).  Asserted: in every hidden layer the share of negative pre-activations of the
    float64 reference lies in 0.2 .. 0.8, so that both branches of the ELU count."""
    rng = np.random.default_rng(seed)
    p = O.init_params(8, H, L, rng)
    a1 = np.zeros((n, Hp))
    a1[:, :H] = O.elu(rng.normal(0, 1, (n, H)))
    Wh, bh = np.zeros((L - 1, Hp, Hp)), np.zeros((L - 1, Hp))
    for l in range(L - 1):
        Wh[l, :H, :H] = p["W"][l + 1]
        bh[l, :H] = rng.normal(0, 0.05, H)
    wa = np.zeros((Hp, 2))
    wa[:H] = p["W"][L]
    ba, wb, bb = rng.normal(0, 0.05, 2), p["W"][L + 1], rng.normal(0, 0.05, 2)
    rows = rng.permutation(n + Y_EXTRA)[:n]
    Y = rng.normal(0, 1, (n + Y_EXTRA, 2))
    case = _case(n, H, Hp, L, a1, Wh, bh, wa, ba, wb, bb, Y, rows, "random")
    check_random(case)
    return case


def check_random(case, a1=None):
    trace = []
    ref_case(case, np.float64, a1=a1, trace=trace)
    for i, (z, _, _, _) in enumerate(trace[:-2]):
        share = float((z[:, :case.H] < 0).mean())
        assert 0.2 <= share <= 0.8, (i, share)


# ---- partial sums of the fused input stage: a case plus partial [G][stride], cvec8 [8][Hp], b1 [Hp]
def pad_stride(n_b, Hp):
    """The production layout (api.hip): groups mp * Hp apart, mp = n_b rounded up to 128 rows."""
    return -(-n_b // 128) * 128 * Hp


def _with_partial(case, G, stride, parts, cvec8, b1):
    """parts [G][n][Hp] -> case.partial flat [G * stride] float32, the rows between n and the stride NaN."""
    n, Hp = case.n, case.Hp
    assert stride >= n * Hp
    flat = np.full(G * stride, np.nan, np.float32)
    for g in range(G):
        flat[g * stride:g * stride + n * Hp] = np.asarray(parts[g], np.float32).reshape(-1)
    case.partial, case.G, case.stride, case.cvec8, case.b1 = flat, G, stride, _f32(cvec8), _f32(b1)
    return case


def integer_partials(case, G, stride, seed):
    """Small-integer partial sums, shift slices and b1 that add up to the (exact) case's a1 in any order; the
    pre-activation is a1 >= 0."""
    rng = np.random.default_rng(seed)
    n, Hp = case.n, case.Hp
    cvec8, b1 = rng.integers(-2, 3, (8, Hp)), rng.integers(-3, 4, Hp)
    parts = rng.integers(-5, 6, (G, n, Hp)).astype(np.float64)
    parts[rng.integers(G)] += case.a1 - parts.sum(0) - cvec8.sum(0) - b1
    _with_partial(case, G, stride, parts, cvec8, b1)
    got = ref_partial_a1(case.partial, G, stride, case.cvec8, case.b1, n, Hp)
    assert np.array_equal(got, case.a1) and np.array_equal(partial_a1_f64(case.partial, G, stride, cvec8, b1, n, Hp), case.a1)
    return case


def association_case(n, Hp, G, stride, seed, picks):
    """Partial sums of magnitude 2^24 and 1, so that the float32 sum depends on the association, with a positive
    pre-activation; L = 2 with a one-nonzero-per-column hidden kernel, zero biases, a one-hot wa on the units `picks` and
    wb = identity: yhat[b] = (a1[b][src[picks[0]]], a1[b][src[picks[1]]]) in any summation order, where src is the input
    unit the hidden kernel routes to each output unit.  -> case with .partial etc. and .a1 = the float32 emulation."""
    rng = np.random.default_rng(seed)
    vals = np.array([2.0 ** 24, -2.0 ** 24, 1.0, -1.0, 1.0, -1.0, 0.0])
    parts = rng.choice(vals, (G, n, Hp))
    cvec8 = rng.integers(-1, 2, (8, Hp)).astype(np.float64)
    b1 = rng.integers(1, 4, Hp) - cvec8.sum(0)               # c + b1 in 1..3
    flat = lambda pp: np.concatenate([np.asarray(x, np.float32).reshape(-1) for x in pp])
    z = ref_partial_a1(flat(parts), G, n * Hp, cvec8, b1, n, Hp)
    parts = np.where((z <= 0)[None], -parts, parts)         # the group sum is odd in its terms; + (c + b1) > 0
    a1 = ref_partial_a1(flat(parts), G, n * Hp, cvec8, b1, n, Hp)
    assert a1.min() > 0
    src = rng.permutation(Hp)
    Wh = np.zeros((1, Hp, Hp))
    Wh[0, src, np.arange(Hp)] = 1
    case = _case(n, Hp, Hp, 2, a1, Wh, np.zeros((1, Hp)), np.zeros((Hp, 2)), np.zeros(2), np.eye(2), np.zeros(2),
                 np.zeros((n + Y_EXTRA, 2)), rng.permutation(n + Y_EXTRA)[:n], "association")
    case.src = src
    set_picks(case, picks)
    return _with_partial(case, G, stride, parts, cvec8, b1)


def set_picks(case, picks):
    case.wa[:] = 0
    case.wa[picks[0], 0] = case.wa[picks[1], 1] = 1
    case.picks = picks


def association_expected(case, a1=None):
    a1 = case.a1 if a1 is None else a1
    return a1[:, case.src[list(case.picks)]]


def random_partials(case, G, stride, seed):
    """Random partial sums whose float64 sum is the (random) case's pre-ELU layer-1 output: N(0, 1), so about half of the
    pre-activations are negative.  -> case with .partial etc., .a1_64 (the float64 stage) and .a1 (its float32 emulation)."""
    rng = np.random.default_rng(seed)
    n, Hp, H = case.n, case.Hp, case.H
    parts = np.zeros((G, n, Hp))
    parts[:, :, :H] = rng.normal(0, 1, (G, n, H)) / np.sqrt(G)
    cvec8, b1 = np.zeros((8, Hp)), np.zeros(Hp)
    cvec8[:, :H], b1[:H] = rng.normal(0, 0.1, (8, H)), rng.normal(0, 0.05, H)
    _with_partial(case, G, stride, parts, cvec8, b1)
    case.a1_64 = partial_a1_f64(case.partial, G, stride, case.cvec8, case.b1, n, Hp)
    case.a1 = ref_partial_a1(case.partial, G, stride, case.cvec8, case.b1, n, Hp)
    assert 0.2 <= float((case.a1_64[:, :H] < 0).mean()) <= 0.8
    check_random(case, case.a1_64)
    return case


# ------------------------------------------------------------------ the comparison
_WORST = {}


def judge(got, ref64, ref32, margin, label, group=None, floor=None):
    """{"yhat": [n][2], "dist": [n][1]} of the device (or of a perturbed reference) against the float64 reference: per
    tensor and per row within margin x the float32 reference's own distance (F, F_row), margin x floor below CAP, and within
    ABS_BAR absolute.  -> the list of violations (empty: passes).  group: print the ratios (pytest -s) and the largest so
    far of the group.  floor = (ref32, ref64) of MORE rows through the same weights: F, F_row and the typical row are then
    taken there.  The worst of one to three rows is no floor (it can be 0); of a few hundred it is a stable figure."""
    f32, f64 = floor if floor is not None else (ref32, ref64)
    scale = row_scale(f64)
    ft, fr = distances(f32, f64, scale)
    F, F_row = max(ft.values()), max(fr.values())
    assert 0 < F and margin * F < CAP and 0 < F_row and margin * F_row < CAP, (label, F, F_row)
    fails = [f"{label}: {k} has shape {np.shape(got[k])}" for k in ref64 if np.shape(got[k]) != np.shape(ref64[k])]
    if fails:
        return fails
    dt, dr = distances(got, ref64, scale)
    kt, kr = max(dt, key=dt.get), max(dr, key=dr.get)
    absd = max(float(np.max(np.abs(np.asarray(got[k], np.float64) - ref64[k]))) for k in ref64)
    if group is not None:
        wt = _WORST[group + " per tensor"] = max(_WORST.get(group + " per tensor", 0.0), dt[kt] / F)
        wr = _WORST[group + " per row"] = max(_WORST.get(group + " per row", 0.0), dr[kr] / F_row)
        print(f"{label}: F {F:.2e} device {dt[kt]:.2e} ({kt}) ratio {dt[kt] / F:.2f} | F_row {F_row:.2e} device {dr[kr]:.2e} "
              f"({kr}) ratio {dr[kr] / F_row:.2f} | abs {absd:.1e} | largest so far in {group}: {wt:.2f} / {wr:.2f}")
    if not dt[kt] <= margin * F:
        fails.append(f"{label}: {kt} is {dt[kt]:.3e} from float64, {margin} x F = {margin * F:.3e}")
    if not dr[kr] <= margin * F_row:
        fails.append(f"{label}: a row of {kr} is {dr[kr]:.3e} from float64, {margin} x F_row = {margin * F_row:.3e}")
    if not absd < ABS_BAR:
        fails.append(f"{label}: {absd:.3e} absolute from float64, the bar is {ABS_BAR}")
    return fails


def exact_equal(got, ref64):
    """Bit for bit: every tensor of got equals the float64 reference cast to float32."""
    return all(np.array_equal(np.asarray(got[k], np.float32), np.asarray(ref64[k]).astype(np.float32)) for k in ref64)


# ------------------------------------------------------------------ the device side
def _guarded_tail(n, tail, margin, seed=0):
    """gpu_util.guarded for n floats, with the choice of what the margin directly ABOVE the view holds: "nan" = the guard
    pattern (a NaN), "junk" = finite values in +-1e4, "zero".  -> (view, check)."""
    import torch
    from tests.gpu_util import GUARD_BYTES, poison
    front = -(-margin * 4 // 256) * 256
    total = front + n * 4 + margin * 4
    raw = torch.tensor(GUARD_BYTES, dtype=torch.uint8, device="cuda").repeat(total // 4)
    view = raw[front:front + n * 4].view(torch.float32)
    assert view.numel() == n and view.data_ptr() % 256 == 0
    if tail != "nan":
        poison(raw[front + n * 4:].view(torch.float32), tail, seed)
    expect = raw.clone()

    def check(what="buffer"):
        torch.cuda.synchronize()
        for side, lo, hi in (("below", 0, front), ("above", front + n * 4, total)):
            bad = (raw[lo:hi] != expect[lo:hi]).nonzero().flatten()
            assert bad.numel() == 0, f"{what}: {bad.numel()} bytes of the guard margin {side} the buffer were overwritten"
    return view, check


class Device:
    """A case's read-only operands on the device (uploaded once per case)."""

    def __init__(self, case):
        import torch
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.case = case
        self.t = {k: up(getattr(case, k)) for k in ("Wh", "bh", "wa", "ba", "wb", "bb", "Y", "rows")}
        for k in ("partial", "cvec8", "b1"):
            if hasattr(case, k):
                self.t[k] = up(getattr(case, k))
        self.a1 = {}

    def update(self, name):
        import torch
        self.t[name] = torch.from_numpy(np.ascontiguousarray(getattr(self.case, name))).cuda()

    def a1_view(self, tail):
        import torch
        if tail not in self.a1:
            c = self.case
            view, check = _guarded_tail(c.n * c.Hp, tail, 128 * c.Hp, seed=11)
            view.copy_(torch.from_numpy(c.a1.reshape(-1)).cuda())
            self.a1[tail] = (view, check)
        return self.a1[tail]


def run(case, form, entry="loc_stack_forward_eval_form", *, with_targets=True, dist_buffer=True, a1_tail="nan", dev=None,
        expect_rc=0, **override):
    """One call of `entry` (loc_stack_forward_eval: the form argument is not passed; loc_stack_forward_eval_partial: the
    case's partial sums instead of a1).  a1 is a guarded view of exactly n * Hp floats with `a1_tail` directly above it;
    yhat (2 n floats) and dist (n floats, when dist_buffer) are guarded views poisoned with NaN words; every margin is
    checked after the call.  override: n_b, L, Hp, groups, group_stride, or rows / Y / partial / cvec8 / b1 = None for a NULL
    pointer.  expect_rc = 0: asserts success -> {"yhat": [n][2], "dist": [n][1] (when written: with targets and a buffer)} plus
    "dist_raw" (the dist buffer's words, whatever happened).  expect_rc = "refused": asserts a nonzero return code, the
    entry point's name in the message and that no word of yhat and dist was written -> the message."""
    import torch
    from locator_amd import _lib
    from tests.gpu_util import bits, guarded, poison
    lib = _lib.load()
    dev = dev or Device(case)
    n, Hp, t = case.n, case.Hp, dev.t
    margin = 128 * Hp
    yhat, chk_y = guarded(2 * n, torch.float32, margin)
    dist, chk_d = guarded(n, torch.float32, margin)
    poison(yhat, "nan"), poison(dist, "nan")
    before = bits(yhat), bits(dist)
    ptr = lambda name, on=True: None if (name in override and override[name] is None) or not on else t[name].data_ptr()
    tail = (ptr("Wh"), ptr("bh"), ptr("wa"), ptr("ba"), ptr("wb"), ptr("bb"), override.get("Hp", Hp), override.get("L", case.L),
            override.get("n_b", n), ptr("rows", with_targets), ptr("Y", with_targets), yhat.data_ptr(),
            dist.data_ptr() if dist_buffer else None)
    checks = [(chk_y, "yhat"), (chk_d, "dist")]
    if entry == "loc_stack_forward_eval_partial":
        rc = lib.loc_stack_forward_eval_partial(ptr("partial"), override.get("groups", case.G),
                                                override.get("group_stride", case.stride), ptr("cvec8"), ptr("b1"), *tail, form, None)
    else:
        a1, chk_a = dev.a1_view(a1_tail)
        checks.append((chk_a, "a1"))
        if entry == "loc_stack_forward_eval":
            rc = lib.loc_stack_forward_eval(a1.data_ptr(), *tail, None)
        else:
            assert entry == "loc_stack_forward_eval_form", entry
            rc = lib.loc_stack_forward_eval_form(a1.data_ptr(), *tail, form, None)
    torch.cuda.synchronize()
    for chk, what in checks:
        chk(f"{entry} form {form}: {what}")
    if expect_rc == "refused":
        msg = lib.loc_last_error().decode()
        assert rc != 0 and entry in msg, (rc, msg)
        assert torch.equal(bits(yhat), before[0]) and torch.equal(bits(dist), before[1]), "a refused call wrote its outputs"
        return msg
    assert rc == 0, lib.loc_last_error()
    out = {"yhat": yhat.cpu().numpy().reshape(n, 2), "dist_raw": bits(dist).numpy()}
    assert torch.equal(bits(dist), before[1]) or (with_targets and dist_buffer), "dist written without targets"
    if with_targets and dist_buffer:
        out["dist"] = dist.cpu().numpy().reshape(n, 1)
    return out


# ------------------------------------------------------------------ the shapes of tests/test_gpu_stack_eval.py
# (tests/test_stack_eval.py checks the generators' conditions at every one of them, without a GPU)
WIDE = [(256, 256), (250, 256)]                    # (H, Hp) that all five forms take
NARROW = [(50, 64), (100, 128), (500, 512)]        # (H, Hp) of the 2-rows-per-workgroup form alone
EXACT_LAYERS = (2, 3, 10)
RANDOM_LAYERS = (2, 10)
PARTIAL_GROUPS = (1, 2, 3, 4, 5, 6, 8, 9, 13)
PARTIAL_ROWS = (1, 37, 70, 163, 235)               # one row, a ragged tile of every form, xcd_stride 4, 2 and 1 at 2 rows per workgroup
PARTIAL_KERNELS = [(-1, 64), (-1, 256), (1, 256), (2, 256)]      # (form, Hp): the three copies of the loop, the first at two widths


def row_counts(form):
    """Exact cases.  Vector-ALU forms (R rows per workgroup): one group and its edges, both sides of the three changes of
    xcd_stride (8 up to 20 row groups, 4 up to 52, 2 up to 116, then 1 without helpers) and one count inside the stride-2
    geometry.  Matrix-pipe forms: one tile and its edges, several tiles with a ragged last one."""
    R = ROWS_PER_WG[form]
    if form < 0:
        return sorted({1, R - 1, R, R + 1, 20 * R, 20 * R + 1, 52 * R, 52 * R + 1, 116 * R, 116 * R + 1, 80 * R + 3} - {0})
    return [1, R - 1, R, R + 1, 3 * 32 + 5 if R == 32 else 5 * 16 + 3]


def two_counts(form):
    """The two row counts at which every L runs."""
    R = ROWS_PER_WG[form]
    return [R + 1, 80 * R + 3] if form < 0 else [R + 1, row_counts(form)[-1]]


def random_counts(form):
    """Random cases: one row count per launch geometry, ragged tiles."""
    R = ROWS_PER_WG[form]
    return [R + 1, 20 * R + 1, 80 * R + 3, 116 * R + 1] if form < 0 else two_counts(form)


def n_max(Hp):
    return max(max(row_counts(f)) for f in FORMS) if Hp == 256 else max(row_counts(-1))


def sub_case(case, n):
    """The first n rows of a case (same weights and targets)."""
    out = SimpleNamespace(**vars(case))
    out.n, out.a1, out.rows = n, np.ascontiguousarray(case.a1[:n]), np.ascontiguousarray(case.rows[:n])
    return out


def sub_ref(ref, n):
    return {k: v[:n] for k, v in ref.items()}


def picks_16_row_tiles(n_b, cu, first_us=12, round16_us=52, round32_us=105):
    """The round model documented in stack_rows.hip (SR16_FIRST_US, SR16_ROUND_US, SR32_ROUND_US)."""
    r16, r32 = -(-(-(-n_b // 16)) // cu), -(-(-(-n_b // 32)) // cu)
    return first_us + r16 * round16_us < r32 * round32_us
