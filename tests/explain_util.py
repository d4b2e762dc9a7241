"""Plain NumPy forms of explain_kernels.hip, problem builders, error metrics and guarded device callers, shared by
tests/test_explain.py (no GPU: the forms against locator_amd/explain.py, the floors of every device case, loc_explain_splits)
and tests/test_gpu_explain_kernels.py (the three entry points called directly).  Importable without a GPU: torch and
tests/gpu_util are imported by the device callers only.

Every form takes a dtype.  float64 is the reference; the same form in float32 is the floor F of a case - how far plain fp32
arithmetic in NumPy's order lands from float64 on exactly these inputs.  The builders draw values that fp32 holds exactly, so
the float64 form, the float32 form and the device start from the same numbers.

The device callers state the memory contract of include/locator_hip.h (per-SNP attribution): every output and scratch
buffer is a gpu_util.guarded view of EXACTLY the documented size, poisoned before the call, and every margin is checked
after it.  The operands sit in guarded views too, so a read past an operand's end meets the guard pattern (a NaN as fp32, the
bytes 225 / 195 / 165 / 127 as genotypes) instead of whatever the allocator left there."""
import ctypes as C

import numpy as np

SD = (2.5, 1.5)                    # sd_x != sd_y: an x / y swap changes the numbers
EX_MT_SAMPLES = 64                 # samples per M tile of ex_sites_kernel (128 rows of D)

# (n, width, L) of loc_explain_stack_grad: 2n = 62 / 64 / 66 and n = 64 / 65 around the 64-row tile of ex_dense_kernel;
# Hp = 32, 96, 160 where its column guard runs, Hp = 64 and 1024; both parities of L - 1; L = 1 (no dense launch)
STACK_CASES = [(1, 32, 1), (1, 33, 2), (31, 96, 2), (32, 96, 3), (33, 160, 4), (64, 64, 2), (65, 96, 10), (33, 1000, 2),
               (65, 1024, 3)]
# (n, Ks, width, xmax) of loc_explain_sites + loc_explain_reduce: the 64-sample M tile, the 128-site tile, 1 to 32 h chunks,
# q-unit genotypes (xmax 126)
SITES_CASES = [(1, 1, 32, 2), (63, 127, 96, 2), (64, 128, 32, 2), (65, 129, 1000, 2), (129, 257, 160, 2), (300, 5, 33, 2),
               (300, 300, 96, 126)]

# The floor rule (tests/test_gpu_stack_train.py, tests/test_gpu_moments.py): the device may be MARGIN times as far from the
# float64 form as the float32 form is, and never more than CAP - what tests/test_gpu_explain.py grants: 1e-5 for acts and
# delta1, 1e-4 for the statistics.  The margins are about twice the largest ratio device / F measured on an MI355X (the
# docstring of tests/test_gpu_explain_kernels.py lists them): 1.66 for acts and delta1, 8.86 for the statistics.  The
# latter is the order of summation at H = 1000: one MFMA accumulator adds the Hp products of a J one after the other, BLAS
# sums them in blocks, so F hardly grows with H and the device's error grows like sqrt(H) (ratios 0.8 to 3.9 at H <= 160).
# The float32 form with J accumulated sequentially (np.cumsum over h) is 8.76 F / 8.40 F from float64 on the CPU.
MARGIN_STACK = 4.0
MARGIN_STATS = 18.0
CAP_STACK = 1e-5
CAP_STATS = 1e-4


def _exact32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def hp_of(width):
    return (width + 31) // 32 * 32


def mt_of(n):
    return (n + EX_MT_SAMPLES - 1) // EX_MT_SAMPLES


def split_accepted(mt, s):
    """The rule by which loc_explain_sites takes a split count: no split is left without an M tile."""
    return 1 <= s <= mt and -(-mt // s) * (s - 1) < mt


def accepted_splits(n):
    mt = mt_of(n)
    return [s for s in range(1, mt + 1) if split_accepted(mt, s)]


def split_range(n, splits, sp):
    """Samples [lo, hi) of split sp."""
    per = -(-mt_of(n) // splits)
    return EX_MT_SAMPLES * per * sp, min(n, EX_MT_SAMPLES * per * (sp + 1))


# ------------------------------------------------------------------ the forms
def _elu(z):
    return np.where(z > 0, z, np.expm1(np.minimum(z, 0)))


def _dact(a):
    """elu'(z) from a = elu(z): 1 where z > 0, else e^z = a + 1"""
    return np.where(a > 0, a.dtype.type(1), a + a.dtype.type(1))


def ref_delta1(a1, Wh, bh, wa, wb, sd, dtype):
    """The hidden-stack part of locator_amd.explain.reference_delta1, from layer 1's ELU output a1 (n, H): Wh / bh the L - 1
    hidden kernels (H, H; in x out) and biases, wa (H, 2) and wb (2, 2) the two linear heads, sd = (sd_x, sd_y).  Entirely in
    `dtype`.  -> acts (L - 1, n, H): the ELU outputs of layers 2 .. L, and delta1 (n, 2, H)."""
    a = np.asarray(a1, dtype)
    W = [np.asarray(w, dtype) for w in Wh]
    b = [np.asarray(v, dtype) for v in bh]
    acts = [a]
    for w, v in zip(W, b):
        a = _elu(a @ w + v)
        acts.append(a)
    c = (np.asarray(wa, dtype) @ np.asarray(wb, dtype)) * np.asarray(sd, dtype)       # (H, 2): the head in map units
    g = c.T[None, :, :] * _dact(acts[-1])[:, None, :]
    for l in range(len(W) - 1, -1, -1):
        g = (g @ W[l].T) * _dact(acts[l])[:, None, :]
    assert g.dtype == dtype
    return np.stack(acts[1:]) if W else np.zeros((0,) + acts[0].shape, dtype), g


def ref_partial(delta1, U, X, mov_mean, samples, dtype):
    """What ex_sites_kernel defines for one split: J = delta1 U^T, dx = x - mov_mean, ax = J_x dx, ay = J_y dx and the four
    terms |ax|, |ay|, sqrt(ax^2 + ay^2), jx^2 + jy^2 in `dtype`, summed over the samples [lo, hi) in float64.
    delta1 (n, 2, H), U (Ks, H), X (n, Ks) uint8, mov_mean (Ks,) -> (4, Ks) float64."""
    lo, hi = samples
    J = np.asarray(delta1[lo:hi], dtype) @ np.asarray(U, dtype).T
    dx = np.asarray(X[lo:hi], dtype) - np.asarray(mov_mean, dtype)
    jx, jy = J[:, 0], J[:, 1]
    ax, ay = jx * dx, jy * dx
    terms = (np.abs(ax), np.abs(ay), np.sqrt(ax * ax + ay * ay), jx * jx + jy * jy)
    assert all(t.dtype == dtype for t in terms)
    return np.stack([t.astype(np.float64).sum(axis=0) for t in terms])


def ref_out(partial_sum, n):
    """loc_explain_reduce: the summed splits (4, Ks) divided by n, the square root of the fourth row."""
    out = np.asarray(partial_sum, np.float64) / float(n)
    out[3] = np.sqrt(out[3])
    return out


# ------------------------------------------------------------------ problems
def stack_problem(n, width, L):
    rng = np.random.default_rng(100003 * n + 101 * width + L)
    H = width
    return {"n": n, "H": H, "Hp": hp_of(H), "L": L,
            "a1": _exact32(_elu(rng.normal(0, 1, (n, H)))),
            "Wh": [_exact32(rng.normal(0, 1, (H, H)) / np.sqrt(H)) for _ in range(L - 1)],     # Glorot: var 2 / (H + H)
            "bh": [_exact32(rng.normal(0, 0.05, H)) for _ in range(L - 1)],
            "wa": _exact32(rng.normal(0, 1, (H, 2)) * np.sqrt(2.0 / (H + 2))),
            "wb": _exact32(rng.normal(0, 1, (2, 2)) * np.sqrt(0.5)),
            "sd": SD}


def sites_problem(n, Ks, width, xmax):
    rng = np.random.default_rng(100003 * n + 1009 * Ks + 101 * width + xmax)
    H = width
    U = (rng.normal(0, 1, (Ks, H)) + 1.0) / np.sqrt(H)
    absent = rng.random(Ks) < 0.1
    absent[0] = False                                  # a one-site problem keeps its site
    if Ks >= 3:
        absent[Ks // 2] = True                         # ... and every other one has an absent site
    U[absent] = 0.0
    delta1 = rng.normal(0, 1, (n, 2, H))
    if n % EX_MT_SAMPLES == 1:
        # With splits = mt the last sample is alone in its split, and one sample's J = delta1 . U[s] cancels to nothing at
        # some of a few hundred sites: the float32 form's per-site error of that split then reaches 1e-4 (3e-5 at n = 129,
        # Ks = 257), no floor to hold a kernel to.  The rows of U share the component 1 / sqrt(H) (above), which leaves
        # every other sample's J a centred normal; this one gets the offset 1.5, so its J is 1.5 sqrt(H) +- 2.1: 4 sigma
        # from zero at H = 32, 9 at H = 160.
        delta1[n - 1] += 1.5
    return {"n": n, "Ks": Ks, "H": H, "Hp": hp_of(H), "xmax": xmax, "absent": absent,
            "delta1": _exact32(delta1), "U": _exact32(U),
            "X": rng.integers(0, xmax + 1, (n, Ks)).astype(np.uint8),
            "mov_mean": _exact32(rng.uniform(0.05, 0.95, Ks) * (xmax / 2.0))}


# ------------------------------------------------------------------ metrics
def _rel(num, den):
    """num / den; where the reference den is 0 the other side has to be exactly 0 as well (-> 0, else inf)"""
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    return np.where(den > 0, num / np.where(den > 0, den, 1.0), np.where(num == 0, 0.0, np.inf))


def tensor_err(got, ref):
    """-> (relative L2 of the whole tensor, worst relative L2 of a row: the last axis)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    d = got - ref
    return (float(_rel(np.linalg.norm(d), np.linalg.norm(ref))),
            float(_rel(np.linalg.norm(d, axis=-1), np.linalg.norm(ref, axis=-1)).max()))


def stats_err(got, ref):
    """(4, Ks) statistics -> (worst relative L2 over sites of one statistic, worst relative error of one site)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and got.shape[0] == 4, (got.shape, ref.shape)
    d = got - ref
    return (float(_rel(np.linalg.norm(d, axis=1), np.linalg.norm(ref, axis=1)).max()),
            float(_rel(np.abs(d), np.abs(ref)).max()))


def stack_refs(prob):
    """-> acts64, delta64 and the floors {"acts": (F, F_row), "delta1": (F, F_row)} ("acts": the worst layer; absent when
    L = 1)"""
    args = [prob[k] for k in ("a1", "Wh", "bh", "wa", "wb", "sd")]
    a64, d64 = ref_delta1(*args, np.float64)
    a32, d32 = ref_delta1(*args, np.float32)
    F = {"delta1": tensor_err(d32, d64)}
    if prob["L"] > 1:
        F["acts"] = tuple(max(e) for e in zip(*(tensor_err(a32[l], a64[l]) for l in range(prob["L"] - 1))))
    return a64, d64, F


def sites_refs(prob, splits):
    """-> per split (ref64 (4, Ks), (F, F_site)), then the same for `out`"""
    n = prob["n"]
    args = [prob[k] for k in ("delta1", "U", "X", "mov_mean")]
    per_split, sum64, sum32 = [], 0.0, 0.0
    for sp in range(splits):
        rng = split_range(n, splits, sp)
        p64, p32 = ref_partial(*args, rng, np.float64), ref_partial(*args, rng, np.float32)
        per_split.append((p64, stats_err(p32, p64)))
        sum64, sum32 = sum64 + p64, sum32 + p32
    o64 = ref_out(sum64, n)
    return per_split, (o64, stats_err(ref_out(sum32, n), o64))


def floor_ok(F, margin, cap):
    return all(0 < f and margin * f < cap for f in F)


# ------------------------------------------------------------------ device callers
def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class Guarded:
    """Guarded device buffers of one call: take() hands out views, check() runs every margin's check."""

    def __init__(self, margin):
        self.margin, self.checks = margin, []

    def take(self, n, dtype, name):
        from tests.gpu_util import guarded
        view, check = guarded(n, dtype, self.margin)
        self.checks.append(lambda: check(name))
        return view

    def put(self, a, name):
        """A host array as a guarded operand of exactly its size."""
        import torch
        a = np.ascontiguousarray(a)
        view = self.take(a.size, getattr(torch, a.dtype.name), name)
        view.copy_(torch.from_numpy(a.reshape(-1)))
        return view

    def check(self):
        for c in self.checks:
            c()


def poison_any(t, kind, seed):
    """gpu_util.poison, with the 64-bit buffers filled through their 32-bit words ("nan": every byte 0xFF, a NaN as fp64)"""
    import torch
    from tests.gpu_util import poison
    poison(t.view(torch.float32) if kind == "nan" and t.element_size() == 8 else t, kind, seed)


def _pad(a, shape):
    out = np.zeros(shape, np.float32)
    out[tuple(slice(0, s) for s in a.shape)] = a
    return out


def stack_operands(prob, G):
    """The operands as include/locator_hip.h lays them out: a1 [n][Hp], wh [L-1][Hp][Hp] input-major, bh [L-1][Hp],
    wa [Hp][2], wb [2][2]; zero in H .. Hp."""
    n, Hp, L = prob["n"], prob["Hp"], prob["L"]
    ops = {"a1": G.put(_pad(prob["a1"], (n, Hp)), "a1"), "wa": G.put(_pad(prob["wa"], (Hp, 2)), "wa"),
           "wb": G.put(np.asarray(prob["wb"], np.float32), "wb"), "wh": None, "bh": None}
    if L > 1:
        ops["wh"] = G.put(np.stack([_pad(w, (Hp, Hp)) for w in prob["Wh"]]), "wh")
        ops["bh"] = G.put(np.stack([_pad(b, (Hp,)) for b in prob["bh"]]), "bh")
    return ops


def run_stack(lib, prob, kind, seed=0):
    """loc_explain_stack_grad on guarded, `kind`-poisoned acts / g / delta1 of exactly (L-1) n Hp, 2 n Hp and 2 n Hp floats
    (acts and g NULL when L = 1).  -> acts (L-1, n, Hp) and delta1 (n, 2, Hp) as float32 host arrays."""
    import torch
    n, Hp, L = prob["n"], prob["Hp"], prob["L"]
    G = Guarded(128 * Hp)
    ops = stack_operands(prob, G)
    acts = G.take((L - 1) * n * Hp, torch.float32, "acts") if L > 1 else None
    g = G.take(2 * n * Hp, torch.float32, "g") if L > 1 else None
    delta1 = G.take(2 * n * Hp, torch.float32, "delta1")
    for i, t in enumerate(t for t in (acts, g, delta1) if t is not None):
        poison_any(t, kind, 16 * seed + i)
    torch.cuda.synchronize()
    rc = lib.loc_explain_stack_grad(_p(ops["a1"]), n, Hp, L, _p(ops["wh"]), _p(ops["bh"]), _p(ops["wa"]), _p(ops["wb"]),
                                    SD[0], SD[1], _p(acts), _p(g), _p(delta1), _stream())
    assert rc == 0, lib.loc_last_error()
    G.check()
    a = acts.cpu().numpy().reshape(L - 1, n, Hp) if L > 1 else np.zeros((0, n, Hp), np.float32)
    return a, delta1.cpu().numpy().reshape(n, 2, Hp)


def xs_rows(prob, pitch, pad):
    """Xs [n][pitch]: the genotypes, the pad columns Ks .. pitch seeded random bytes (pad = "random") or the constant 2"""
    n, Ks = prob["n"], prob["Ks"]
    xs = (np.random.default_rng(pitch).integers(0, 256, (n, pitch)).astype(np.uint8) if pad == "random"
          else np.full((n, pitch), 2, np.uint8))
    xs[:, :Ks] = prob["X"]
    return xs


def run_sites(lib, prob, splits, kind, seed=0, pitch=None, pad="random"):
    """loc_explain_sites + loc_explain_reduce on guarded, `kind`-poisoned partial / out of exactly splits 4 Ks and 4 Ks
    doubles.  -> partial (splits, 4, Ks) and out (4, Ks) as float64 host arrays."""
    import torch
    n, Ks, Hp = prob["n"], prob["Ks"], prob["Hp"]
    pitch = Ks if pitch is None else pitch
    G = Guarded(128 * Hp)
    delta1 = G.put(_pad(prob["delta1"], (n, 2, Hp)), "delta1")
    U = G.put(_pad(prob["U"], (Ks, Hp)), "U")
    Xs = G.put(xs_rows(prob, pitch, pad), "Xs")
    mm = G.put(np.asarray(prob["mov_mean"], np.float32), "mov_mean")
    partial = G.take(splits * 4 * Ks, torch.float64, "partial")
    out = G.take(4 * Ks, torch.float64, "out")
    poison_any(partial, kind, 16 * seed)
    poison_any(out, kind, 16 * seed + 1)
    torch.cuda.synchronize()
    rc = lib.loc_explain_sites(_p(delta1), n, _p(U), Ks, Hp, _p(Xs), pitch, _p(mm), splits, _p(partial), _stream())
    assert rc == 0, lib.loc_last_error()
    rc = lib.loc_explain_reduce(_p(partial), splits, Ks, n, _p(out), _stream())
    assert rc == 0, lib.loc_last_error()
    G.check()
    return partial.cpu().numpy().reshape(splits, 4, Ks), out.cpu().numpy().reshape(4, Ks)
