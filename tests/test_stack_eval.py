"""The references, generators and comparison of tests/stack_eval_util.py, without a GPU: what tests/test_gpu_stack_eval.py
relies on.  The float64 stack against oracle.predict (locator.py:319-325, :414); the float32 emulation of the fused input
stage against a float64 sum; the generators' conditions at every shape the GPU file uses; and the comparison itself, fed
float64 references computed with the mistakes these kernels could make - each has to be refused at the margin the GPU file
grants, and each has to change a bit of an exact case."""
import copy
import functools

import numpy as np
import pytest

from oracle import locator_oracle as O
from tests import stack_eval_util as U
from tests.gpu_util import make_problem

MARGIN = max(U.MARGIN_VALU, U.MARGIN_MFMA)      # refused at the wider margin = refused at both


@pytest.mark.parametrize("width,nlayers,n", [(40, 2, 5), (33, 3, 7), (64, 10, 9)])
def test_reference_stack_matches_the_oracle(width, nlayers, n):
    """ref_eval(float64) from the oracle's layer-1 activations = oracle.predict, and its distance = oracle.euclid."""
    x, y, p, rng = make_problem(n, 60, width, nlayers, seed=width + nlayers)
    s = p["gamma"] / np.sqrt(p["mov_var"] + O.BN_EPS)
    a1 = O.elu(((x.astype(np.float64) - p["mov_mean"]) * s + p["beta"]) @ p["W"][0] + p["b"][0])
    L = nlayers
    got = U.ref_eval(a1, np.stack(p["W"][1:L]), np.stack(p["b"][1:L]), p["W"][L], p["b"][L], p["W"][L + 1], p["b"][L + 1], y,
                     np.float64)
    want = O.predict(p, x)
    assert np.abs(got["yhat"] - want).max() <= 1e-12 * np.abs(want).max()
    d = O.euclid(want, y)
    assert np.abs(got["dist"][:, 0] - d).max() <= 1e-12 * d.max()


@pytest.mark.parametrize("H,Hp", U.WIDE + U.NARROW)
def test_generators_hold_their_conditions_at_every_shape(H, Hp):
    """exact_case and random_case assert their conditions themselves; here at the largest row count of every width and
    every L the GPU file uses, and on the sub-cases it cuts from them."""
    n = U.n_max(Hp)
    for L in U.EXACT_LAYERS:
        case = U.exact_case(n, H, Hp, L, seed=L)
        assert U.check_exact(case) < 2 ** 24
        assert U.check_exact(U.sub_case(case, 37)) < 2 ** 24
        r64, r32 = U.ref_case(case, np.float64), U.ref_case(case, np.float32)
        assert U.exact_equal(r32, r64), "float32 NumPy is not exact on an exact case"
    for L in U.RANDOM_LAYERS:
        case = U.random_case(n, H, Hp, L, seed=L)
        r64, r32 = U.ref_case(case, np.float64), U.ref_case(case, np.float32)
        assert U.judge(r32, r64, r32, 1.0, f"H {H} L {L}") == []            # the floor against itself
        assert np.abs(r64["yhat"]).max() > 0.1                             # 2e-5 absolute is a bar on O(1) values


def test_round_model_of_the_matrix_pipe_forms():
    """picks_16_row_tiles reproduces what stack_rows.hip documents for 256 compute units: 16-row tiles up to 4096 rows and at
    8193..12,288, 32-row tiles at 4097..8192 and 12,289..16,384."""
    for n, want in ((2049, True), (4096, True), (4097, False), (8192, False), (8193, True), (12288, True), (12289, False),
                    (16384, False)):
        assert U.picks_16_row_tiles(n, 256) == want, n


@pytest.mark.parametrize("G", U.PARTIAL_GROUPS)
def test_partial_emulation_against_a_float64_sum(G):
    """ref_partial_a1 (float32, the documented association) within the float32 floor of the float64 sum: 2^-24 relative
    per addition, G + 10 additions, on the sum of absolute terms."""
    n, Hp = 37, 64
    for stride in (n * Hp, U.pad_stride(n, Hp)):
        case = U.random_partials(U.random_case(n, 50, Hp, 2, seed=G), G, stride, seed=G)
        P = np.asarray(case.partial, np.float64)
        mag = sum(np.abs(P[g * stride:g * stride + n * Hp].reshape(n, Hp)) for g in range(G))
        mag = mag + np.abs(case.cvec8.astype(np.float64)).sum(0) + np.abs(case.b1)
        assert (np.abs(case.a1 - case.a1_64) <= (G + 10) * 2.0 ** -24 * mag + 1e-30).all()
        # the rows between n and the stride are NaN in the buffer and never read
        assert np.isfinite(case.a1).all() and (stride == n * Hp or np.isnan(case.partial[n * Hp:stride]).all())
    ints = U.integer_partials(U.exact_case(n, 50, Hp, 2, seed=G), G, U.pad_stride(n, Hp), seed=G)
    assert np.array_equal(U.ref_partial_a1(ints.partial, G, ints.stride, ints.cvec8, ints.b1, n, Hp, assoc="right"), ints.a1)


# ------------------------------------------------------------------ what these kernels could get wrong
def _best_block(W, H):
    """(k0, w): the 16-input range x 32-unit tile of a kernel with the largest sum of absolute weights."""
    best = max(((np.abs(W[k0:k0 + 16, 32 * w:32 * w + 32]).sum(), k0, w) for k0 in range(0, H - 15, 16) for w in range((H + 31) // 32)))
    assert best[0] > 0
    return best[1], best[2]


def _perturbed(case, which):
    """The float64 result of a stack that makes one mistake."""
    c = copy.deepcopy(case)
    l = (case.L - 1) // 2                         # a layer in the middle (the only one at L = 2)
    if which == "k-range missing":                # 16 inputs of one 32-unit output tile of one layer
        k0, w = _best_block(c.Wh[l], c.H)
        c.Wh[l, k0:k0 + 16, 32 * w:32 * w + 32] = 0
    elif which == "rows swapped in a tile":       # rowmap: rows 5 and 9 of the second 32-row tile change places
        c.a1[[37, 41]] = c.a1[[41, 37]]
    elif which == "accumulators swapped":         # units 32 w + i16 and 32 w + 16 + i16 of the 16-row form, w = 1, i16 = 3
        c.Wh[l][:, [35, 51]] = c.Wh[l][:, [51, 35]]
    elif which == "neighbouring bias":
        c.bh[l] = case.bh[l + 1] if l + 1 < case.L - 1 else case.bh[l - 1]
    elif which == "wb transposed":
        c.wb = np.ascontiguousarray(c.wb.T)
    else:
        raise ValueError(which)
    return U.ref_case(c, np.float64)


@functools.lru_cache(maxsize=None)
def _cases(L):
    n, H, Hp = 101, 250, 256
    rnd, ex = U.random_case(n, H, Hp, L, seed=5), U.exact_case(n, H, Hp, L, seed=5)
    return rnd, U.ref_case(rnd, np.float64), U.ref_case(rnd, np.float32), ex, U.ref_case(ex, np.float64)


@pytest.mark.parametrize("L", [3, 10])
@pytest.mark.parametrize("which", ["k-range missing", "rows swapped in a tile", "accumulators swapped", "neighbouring bias",
                                   "wb transposed", "ragged tile stale"])
def test_the_comparison_flags_what_these_kernels_could_get_wrong(which, L):
    rnd, r64, r32, ex, e64 = _cases(L)
    assert U.judge(r64, r64, r32, MARGIN, "unperturbed") == [] and U.exact_equal(U.ref_case(ex, np.float32), e64)
    if which == "ragged tile stale":              # rows 96..100 keep what an earlier launch left there: rows 0..4
        bad, bad_e = ({k: v.copy() for k, v in ref.items()} for ref in (r64, e64))
        for d in (bad, bad_e):
            for v in d.values():
                v[96:] = v[:5]
    else:
        bad, bad_e = _perturbed(rnd, which), _perturbed(ex, which)
    fails = U.judge(bad, r64, r32, MARGIN, which)
    assert fails, which
    assert not U.exact_equal(bad_e, e64), which
    if which not in ("ragged tile stale", "rows swapped in a tile"):       # those two move whole rows, also of dist
        assert not np.array_equal(bad_e["yhat"], e64["yhat"])


@pytest.mark.parametrize("G", [3, 5, 13])
def test_the_comparison_flags_a_skipped_group(G):
    n, H, Hp = 37, 250, 256
    stride = U.pad_stride(n, Hp)
    rnd = U.random_partials(U.random_case(n, H, Hp, 3, seed=G), G, stride, seed=G)
    r64, r32 = U.ref_case(rnd, np.float64, a1=rnd.a1_64), U.ref_case(rnd, np.float32)
    assert U.judge(r32, r64, r32, MARGIN, "unperturbed") == []
    a1 = U.ref_partial_a1(rnd.partial, G, stride, rnd.cvec8, rnd.b1, n, Hp, skip_group=G // 2)
    assert U.judge(U.ref_case(rnd, np.float64, a1=a1), r64, r32, MARGIN, "skipped group")
    ex = U.integer_partials(U.exact_case(n, H, Hp, 3, seed=G), G, stride, seed=G)
    a1 = U.ref_partial_a1(ex.partial, G, stride, ex.cvec8, ex.b1, n, Hp, skip_group=G // 2)
    assert not U.exact_equal(U.ref_case(ex, np.float64, a1=a1), U.ref_case(ex, np.float64))


def test_the_association_cases_tell_the_two_associations_apart():
    """2^24, 1, -2^24, 1 across the quarters: ((q0 + q1) + q2) + q3 = 1 in float32, q0 + (q1 + (q2 + q3)) = 2; and the generated
    association cases differ between the two on the units that reach yhat, for every group count with three quarters or
    more in use."""
    Hp, b1 = 64, np.ones(64)
    part = np.repeat(np.array([2.0 ** 24, 1, -2.0 ** 24, 1], np.float32), Hp)
    doc = U.ref_partial_a1(part, 4, Hp, np.zeros((8, Hp)), b1, 1, Hp)
    alt = U.ref_partial_a1(part, 4, Hp, np.zeros((8, Hp)), b1, 1, Hp, assoc="right")
    assert (doc == 2).all() and (alt == 3).all()                 # + b1 = 1
    for G in U.PARTIAL_GROUPS:
        case = U.association_case(37, Hp, G, U.pad_stride(37, Hp), seed=G, picks=(3, 40))
        doc = U.ref_partial_a1(case.partial, G, case.stride, case.cvec8, case.b1, 37, Hp)
        assert np.array_equal(doc, case.a1) and doc.min() > 0
        got = U.ref_case(case, np.float64)["yhat"]
        assert np.array_equal(got, U.association_expected(case).astype(np.float64))      # a1 reaches yhat unchanged
        if G >= 3:
            alt = U.ref_partial_a1(case.partial, G, case.stride, case.cvec8, case.b1, 37, Hp, assoc="right")
            assert not np.array_equal(U.association_expected(case, alt), U.association_expected(case)), G
            skip = U.ref_partial_a1(case.partial, G, case.stride, case.cvec8, case.b1, 37, Hp, skip_group=1)
            assert not np.array_equal(U.association_expected(case, skip), U.association_expected(case)), G
