"""The inference hidden stack at kernel level: loc_stack_forward_eval, loc_stack_forward_eval_form and
loc_stack_forward_eval_partial (stack_fused.hip, stack_rows.hip) called directly through the C ABI, in all five forms -
2 / 4 / 8 rows per workgroup on the vector ALU (forms -1 / -2 / -3), 32- and 16-row tiles on the fp32 matrix pipe (1 / 2) - at
every width, on both sides of every change of launch geometry, and with the fused input stage that sums layer-1 group
partials (locator.py:319-325 layers 2..L, Dense(2) x 2, :314-315 the distance; model.predict, :414, :441).

The contract these tests state (include/locator_hip.h):
  a1 [n_b][Hp]   exactly that is read: a guarded view of n_b * Hp floats with a NaN, junk or zeros directly above it gives
                 the same bits
  yhat, dist     guarded, NaN-poisoned views of exactly 2 n_b and n_b floats; no dist without targets, in any form
  bad arguments  Y without rows or the reverse, n_b < 0, L < 2, a width without a fused form, and the partial entry's own
                 refusals: nonzero, the entry point's name in the message, nothing launched; n_b = 0: 0 and nothing written

References (tests/stack_eval_util.py; tests/test_stack_eval.py checks them and the comparison without a GPU):
  exact cases    every value of the stack is an integer and every sum of absolute terms stays below 2^24, so fp32 in ANY
                 summation order, fused or not, has to give the float64 result bit for bit - yhat and dist
  random cases   float64 is the reference, the same NumPy code in float32 the floor: F per tensor, F_row per row.  The device
                 may be MARGIN times as far, never more than CAP, and never more than 2e-5 absolute
                 (tests/test_gpu_stack_rows.py's bar).  Every case prints device / F (pytest -s).
  partial sums   integers (exact), magnitudes 2^24 and 1 (bit for bit the float32 emulation of the documented association:
                 "the same bits as the dedicated reduction", for each of the three copies of the loop), random (the floor)

Measured on an MI355X over the random cases below, device / floor per tensor | per row; F is
1.5e-7..9.2e-7, F_row 4.3e-7..2.9e-6, the largest absolute distance from float64 1.8e-6:
  vector ALU, a1 given, 72 cases       0.29..1.83 (3 rows, width 50, 10 layers) | 0.14..1.00 (163 rows, width 500, 10 layers)
  vector ALU, partial sums, 56 cases   0.21..1.05 (70 rows, Hp 64, 3 groups)    | 0.06..1.03 (235 rows, Hp 64, 5 groups)
  matrix pipe, a1 given, 16 cases      0.86..1.14 (32-row form, 33 rows, width 250, 2 layers) | 0.49..0.96 (16-row form, 17 rows)
  matrix pipe, partial sums, 56 cases  0.20..2.77 (32-row form, ONE row, 13 groups) | 0.04..1.30 (32-row form, 163 rows, 8 groups)
The ratios above 1.5 all belong to launches of one to three rows measured against the floor of a few hundred: the error of
six numbers or fewer.  The margins stand at about twice the largest ratio of their group, rounded up: 4 for the vector-ALU
forms, 6 for the matrix-pipe forms (stack_eval_util.MARGIN_VALU,
MARGIN_MFMA)."""
import functools

import numpy as np
import pytest
import torch

from tests import stack_eval_util as U

pytestmark = pytest.mark.gpu

EVAL, FORM, PARTIAL = "loc_stack_forward_eval", "loc_stack_forward_eval_form", "loc_stack_forward_eval_partial"


@functools.lru_cache(maxsize=None)
def _exact(H, Hp, L):
    case = U.exact_case(U.n_max(Hp), H, Hp, L, seed=H + L)
    return case, U.ref_case(case, np.float64), {}


@functools.lru_cache(maxsize=None)
def _random(H, Hp, L):
    case = U.random_case(U.n_max(Hp), H, Hp, L, seed=H + L)
    return case, U.ref_case(case, np.float64), U.ref_case(case, np.float32), {}


def _device(case, n, cache):
    """Sub-cases share the weights; a1 and rows are the first n."""
    if n not in cache:
        cache[n] = U.Device(U.sub_case(case, n))
    return cache[n]


def _launch(case, cache, n, form, entry=FORM, **kw):
    dev = _device(case, n, cache)
    return U.run(dev.case, form, entry, dev=dev, **kw)


def _bits_equal(a, b):
    return all(np.array_equal(np.asarray(a[k]).view(np.int32), np.asarray(b[k]).view(np.int32)) for k in ("yhat", "dist"))


# ------------------------------------------------------------------ exact: bit for bit float64
def _exact_params():
    out = []
    for H, Hp in U.WIDE:
        for form in U.FORMS:
            out.append((form, FORM, H, Hp, 10, tuple(U.row_counts(form))))
            out += [(form, FORM, H, Hp, L, tuple(U.two_counts(form))) for L in (2, 3)]
    for H, Hp in U.NARROW:
        out.append((-1, EVAL, H, Hp, 10, tuple(U.row_counts(-1))))
        out += [(-1, EVAL, H, Hp, L, tuple(U.two_counts(-1))) for L in (2, 3)]
    return out


@pytest.mark.parametrize("form,entry,H,Hp,L,counts", _exact_params(),
                         ids=[f"form{f}-H{H}-L{L}-{len(c)}counts" for f, _, H, _, L, c in _exact_params()])
def test_exact_cases_bit_for_bit(form, entry, H, Hp, L, counts):
    """np.array_equal with the float64 reference cast to float32, yhat and dist, at every row count of the form."""
    case, ref, cache = _exact(H, Hp, L)
    for n in counts:
        got = _launch(case, cache, n, form, entry)
        want = U.sub_ref(ref, n)
        for k in ("yhat", "dist"):
            bad = np.argwhere(got[k] != want[k].astype(np.float32))
            assert bad.size == 0, (f"form {form} H {H} L {L} n {n}: {k} differs from float64 in {len(bad)} places, first at "
                                   f"{bad[0]}: {got[k][tuple(bad[0])]} for {want[k][tuple(bad[0])]}")


@pytest.mark.parametrize("H,Hp", U.WIDE)
@pytest.mark.parametrize("L", U.EXACT_LAYERS)
def test_the_five_forms_agree_bit_for_bit_on_exact_cases(H, Hp, L):
    case, ref, cache = _exact(H, Hp, L)
    for n in (33, 101):
        outs = {form: _launch(case, cache, n, form) for form in U.FORMS}
        outs[0] = _launch(case, cache, n, 0, EVAL)
        for form, got in outs.items():
            assert _bits_equal(got, outs[-1]), (form, n)
        assert U.exact_equal(outs[-1], U.sub_ref(ref, n))


# ------------------------------------------------------------------ random: against the floor
def _random_params():
    out = [(form, FORM, H, Hp, L) for H, Hp in U.WIDE for form in U.FORMS for L in U.RANDOM_LAYERS]
    return out + [(-1, EVAL, H, Hp, L) for H, Hp in U.NARROW for L in U.RANDOM_LAYERS]


@pytest.mark.parametrize("form,entry,H,Hp,L", _random_params())
def test_random_cases_against_the_float32_floor(form, entry, H, Hp, L):
    """One row count per launch geometry and the ragged tiles: within MARGIN x the float32 reference's own distance from
    float64 per tensor and per row, and within 2e-5 absolute; the floor is taken over all rows of the case (U.judge says
    why).  The vector-ALU forms give the same bits whatever the rows per workgroup."""
    case, r64, r32, cache = _random(H, Hp, L)
    group = "vector ALU" if form < 0 else "matrix pipe"
    fails = []
    for n in U.random_counts(form):
        got = _launch(case, cache, n, form, entry)
        fails += U.judge(got, U.sub_ref(r64, n), U.sub_ref(r32, n), U.margin_of(form), f"form {form} H {H} L {L} n {n}", group,
                         floor=(r32, r64))
        if form in (-2, -3):
            assert _bits_equal(got, _launch(case, cache, n, -1)), (form, n)
    assert not fails, fails


# ------------------------------------------------------------------ form 0 takes what the header says
def test_form_0_takes_the_documented_form_at_every_threshold():
    """Up to 2 x compute units rows 2 rows per workgroup, up to 4 x 4, up to 8 x 8, above that the matrix-pipe form with the
    smaller modelled time (the three constants of stack_rows.hip); equal bits with that form and, on random data, not with
    the other matrix-pipe form."""
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    case = U.random_case(8 * cu + 1, 256, 256, 3, seed=cu)
    cache = {}
    plan = [(2 * cu, -1), (2 * cu + 1, -2), (4 * cu, -2), (4 * cu + 1, -3), (8 * cu, -3),
            (8 * cu + 1, 2 if U.picks_16_row_tiles(8 * cu + 1, cu) else 1)]
    for n, form in plan:
        for entry in (EVAL, FORM):
            got = _launch(case, cache, n, 0, entry)
            assert _bits_equal(got, _launch(case, cache, n, form)), (n, form, entry)
        if form > 0:
            assert not _bits_equal(got, _launch(case, cache, n, 3 - form)), "the two matrix-pipe forms cannot be told apart"
            assert not _bits_equal(got, _launch(case, cache, n, -3))
        cache.clear()


# ------------------------------------------------------------------ the fused input stage
def _strides(n, Hp):
    return (n * Hp, U.pad_stride(n, Hp))


def _rows_for(i):
    return U.PARTIAL_ROWS[i % len(U.PARTIAL_ROWS)]


_PARTIAL_PARAMS = ([(form, Hp, G, _rows_for(i + j)) for j, (form, Hp) in enumerate(U.PARTIAL_KERNELS)
                    for i, G in enumerate(U.PARTIAL_GROUPS)] +
                   [(form, Hp, 5, n) for form, Hp in U.PARTIAL_KERNELS for n in U.PARTIAL_ROWS])


@pytest.mark.parametrize("form,Hp,G,n", _PARTIAL_PARAMS)
def test_partial_stage_integer_sums_bit_for_bit(form, Hp, G, n):
    """Small-integer partial sums that add up to an exact case's a1 in any order: float64's bits, with the groups n_b * Hp
    apart and in the production layout (n_b rounded up to 128 rows, NaN in between)."""
    H = Hp - 6
    base = U.exact_case(n, H, Hp, 3, seed=G + n)
    ref = U.ref_case(base, np.float64)
    for stride in _strides(n, Hp):
        case = U.integer_partials(base, G, stride, seed=G)
        got = U.run(case, form, PARTIAL)
        assert U.exact_equal(got, ref), (form, Hp, G, n, stride)
    assert _bits_equal(got, U.run(base, form, FORM))


@pytest.mark.parametrize("form,Hp", U.PARTIAL_KERNELS)
@pytest.mark.parametrize("G", U.PARTIAL_GROUPS)
def test_partial_stage_keeps_the_documented_association(form, Hp, G):
    """Partial sums of magnitude 2^24 and 1: the float32 sum depends on the association, and the stack is built so that a1
    reaches yhat unchanged - bit for bit the float32 emulation of ((q0 + q1) + q2) + q3 with ascending groups inside the
    quarters, (c + b1) last.  Six pairs of units per case, three with each layout."""
    n = 37
    rng = np.random.default_rng(G)
    for i in range(6):
        picks = tuple(int(v) for v in rng.choice(Hp, 2, replace=False))
        case = U.association_case(n, Hp, G, _strides(n, Hp)[i % 2], seed=100 * G + i, picks=picks)
        got = U.run(case, form, PARTIAL, with_targets=False)
        want = U.association_expected(case)
        bad = np.argwhere(got["yhat"] != want)
        assert bad.size == 0, (f"form {form} Hp {Hp} G {G} units {picks}: {len(bad)} sums differ from the documented "
                               f"association, first at {bad[0]}: {got['yhat'][tuple(bad[0])]} for {want[tuple(bad[0])]}")


@pytest.mark.parametrize("form,Hp,G,n", _PARTIAL_PARAMS)
def test_partial_stage_random_sums_against_the_floor(form, Hp, G, n):
    """Random partial sums, about half of the pre-activations negative: float64 stage + float64 stack is the reference,
    the float32 emulation + float32 stack the floor."""
    H = Hp - 6
    group = "vector ALU" if form < 0 else "matrix pipe"
    fails = []
    refs = lambda c: (U.ref_case(c, np.float32), U.ref_case(c, np.float64, a1=c.a1_64))
    big = U.random_case(max(U.PARTIAL_ROWS), H, Hp, 3, seed=G + n)
    floor = refs(U.random_partials(U.sub_case(big, big.n), G, big.n * Hp, seed=G + 1))      # the floor: all rows, same weights
    for stride in _strides(n, Hp):
        case = U.random_partials(U.sub_case(big, n), G, stride, seed=G)
        r32, r64 = refs(case)
        got = U.run(case, form, PARTIAL)
        fails += U.judge(got, r64, r32, U.margin_of(form), f"partial form {form} Hp {Hp} G {G} n {n} stride {stride}", group,
                         floor=floor)
    assert not fails, fails


# ------------------------------------------------------------------ the memory contract
@pytest.mark.parametrize("form,entry,H,Hp", [(f, FORM, 250, 256) for f in U.FORMS] + [(0, EVAL, 250, 256)] +
                         [(-1, EVAL, H, Hp) for H, Hp in U.NARROW])
def test_memory_contract_of_every_form(form, entry, H, Hp):
    """A ragged row count (37: no form's tile divides it).  The same bits whether the words directly above a1 are a NaN,
    junk or zeros; the margins of a1, yhat and dist intact (checked by the caller after every launch); without targets and
    with a poisoned dist passed anyway, dist comes back untouched and yhat is the run with targets'."""
    case = U.random_case(37, H, Hp, 3, seed=Hp)
    dev = U.Device(case)
    base = U.run(case, form, entry, dev=dev, a1_tail="nan")
    assert np.isfinite(base["yhat"]).all() and np.isfinite(base["dist"]).all()
    for tail in ("junk", "zero"):
        assert _bits_equal(base, U.run(case, form, entry, dev=dev, a1_tail=tail)), tail
    none = U.run(case, form, entry, dev=dev, with_targets=False)           # asserts that no word of dist was written
    assert "dist" not in none and np.array_equal(none["yhat"].view(np.int32), base["yhat"].view(np.int32))
    nobuf = U.run(case, form, entry, dev=dev, dist_buffer=False)
    assert np.array_equal(nobuf["yhat"].view(np.int32), base["yhat"].view(np.int32))


# ------------------------------------------------------------------ bad arguments launch nothing
def test_bad_arguments_launch_nothing():
    """Each refused call returns nonzero with the entry point's name in the message and leaves the poisoned outputs as they
    were (U.run(expect_rc="refused") asserts all three).  The first two would follow a NULL pointer on the device if they
    were launched: the refusals stand in sf_eval_launch in front of every launch."""
    case = U.random_partials(U.random_case(37, 100, 128, 3, seed=1), 5, U.pad_stride(37, 128), seed=1)
    dev = U.Device(case)
    wide = U.random_partials(U.random_case(37, 250, 256, 3, seed=2), 5, U.pad_stride(37, 256), seed=2)
    wdev = U.Device(wide)
    bad = [dict(Y=None), dict(rows=None), dict(n_b=-1), dict(n_b=-2 ** 31), dict(L=1), dict(L=0), dict(Hp=96), dict(Hp=1024)]
    for c, d, forms in ((case, dev, (0,)), (wide, wdev, (0, 1, 2, -3))):
        for form in forms:
            for entry in (EVAL, FORM, PARTIAL):
                if entry == EVAL and form != 0:
                    continue
                for kw in bad:
                    msg = U.run(c, form, entry, dev=d, expect_rc="refused", **kw)
                    assert msg, (entry, form, kw)
                if entry == PARTIAL:
                    for kw in (dict(groups=0), dict(groups=-3), dict(group_stride=37 * c.Hp - 1), dict(partial=None),
                               dict(cvec8=None), dict(b1=None)):
                        U.run(c, form, entry, dev=d, expect_rc="refused", **kw)
                # no rows: success, and not a word written
                out = U.run(c, form, entry, dev=d, n_b=0)
                assert np.isnan(out["yhat"]).all() and "dist" in out and np.isnan(out["dist"]).all(), (entry, form)
                assert (out["yhat"].view(np.int32) == -1).all() and (out["dist_raw"] == -1).all()
    # and the library still works
    assert np.isfinite(U.run(case, 0, EVAL, dev=dev)["yhat"]).all()
