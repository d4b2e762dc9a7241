"""The fixtures of tests/l1_infer_util.py prove what tests/test_gpu_l1_infer.py takes from them - checked on the host:
the exact fixtures (A, B, D) give the same bits in any summation order, a lost piece / digit, swapped units or a neighbouring
SNP changes the expected bits, fixture B stays inside its span, fixture C's bound is tighter than one SNP, and the bar on
the expm1 side lies below what a lost lowest bf16 piece changes there."""
import numpy as np
import pytest

from tests import l1_infer_util as U

H = 250


def _exact_fixtures():
    return [U.fixture_a(96, H), U.fixture_a(280, H, 300), U.fixture_b(161, H, 129), U.fixture_b(640, H, 257),
            U.fixture_b(1152, H, 128), U.fixture_d(161, H, 3, {160: 1.0}), U.few_shifts(640, H, 2)]


@pytest.mark.parametrize("mode", U.MODES)
def test_exact_fixtures_give_the_same_bits_in_any_summation_order(mode):
    rng = np.random.default_rng(1)
    for fx in _exact_fixtures():
        z = fx.z(mode)                                           # float64, asserted to be fp32 numbers
        T = fx.terms(mode)                                       # [n][J][H] fp32
        assert np.array_equal(T.astype(np.float64).sum(1), z), fx.name
        assert np.array_equal(T.sum(1, dtype=np.float32).astype(np.float64), z), fx.name
        for _ in range(24):
            acc = np.zeros((fx.n, fx.H), np.float32)
            for j in rng.permutation(T.shape[1]):
                acc = acc + T[:, j]
            assert np.array_equal(acc.astype(np.float64), z), (fx.name, mode)
        # groups of terms summed on their own first (SNP groups), then the group sums
        for _ in range(8):
            perm = rng.permutation(T.shape[1])
            cut = rng.integers(0, T.shape[1] + 1)
            parts = [T[:, perm[:cut]].sum(1, dtype=np.float32), T[:, perm[cut:]].sum(1, dtype=np.float32)]
            assert np.array_equal((parts[1] + parts[0]).astype(np.float64), z), (fx.name, mode)
        # the negated fixture is the mirror image
        assert np.array_equal(fx.negated().z(mode), -z)


def test_the_big_shift_fixture_is_exact():
    K = U.BIG_K
    assert K == 24576 + 3 * 64 + 1 and K % 64 and (K + 63) // 64 > 384
    W = U.full_weights(K, 8, 0)
    for k in U.BIG_SHIFT_SNPS:
        fx = U.fixture_d(K, 8, 1, {k: 1.0}, weights=W)
        assert np.array_equal(fx.z("p3")[0].astype(np.float32), W[k]) and np.array_equal(fx.negated().z("d2")[0], -fx.z("p1")[0])
    blocks = sorted({k // 64 for k in U.BIG_SHIFT_SNPS})
    assert blocks == [0, 127, 128, 255, 256, 383, 384, (K - 1) // 64]


def _bits(z):
    return U.expected_bits(z)[0]


@pytest.mark.parametrize("mode", U.MODES)
def test_a_lost_piece_swapped_units_or_a_neighbouring_snp_change_the_expected_bits(mode):
    for fx in (U.fixture_a(96, H), U.fixture_b(161, H, 129)):
        both = lambda f: np.concatenate([_bits(f.z(mode)), _bits(-f.z(mode))])     # the W run and the -W run
        want = both(fx)
        low = U.lowest_term(fx.wp(), mode)
        used = np.flatnonzero(fx.x.any(0))
        hits = 0
        for k in used[:: max(1, len(used) // 12)]:
            for h in (0, 101, H - 1):
                if low[k, h] == 0:
                    continue
                hits += 1
                z = fx.z(mode)
                z[:, h] -= fx.x[:, k] * low[k, h]                 # this weight without its lowest piece / digit
                assert not np.array_equal(np.concatenate([_bits(z), _bits(-z)]), want), (fx.name, k, h)
        assert hits >= 12
        for h1, h2 in ((0, 1), (31, 32), (7, H - 1)):
            sw = U.Fixture("swap", fx.x, fx.W.copy(), fx.scale, fx.shift, fx.b1, True)
            sw.W[:, [h1, h2]] = sw.W[:, [h2, h1]]
            assert not np.array_equal(both(sw), want)
    a = U.fixture_a(96, H)
    for off in (-1, 1):
        assert not np.array_equal(_bits(U.fixture_a(96, H, snp_offset=off).z(mode)), _bits(a.z(mode)))
    rows = U.Fixture("rows", a.x[::-1], a.W, a.scale, a.shift, a.b1, True)
    assert not np.array_equal(_bits(rows.z(mode)), _bits(a.z(mode)))


@pytest.mark.parametrize("mode", U.MODES)
def test_fixture_b_stays_inside_24_bits_for_every_row_and_unit(mode):
    for K, n in U.B_SHAPES:
        fx = U.fixture_b(K, H, n)
        assert U.b_span_ratio(fx, mode) < 1.0, (K, n)
        if mode == "p3":
            assert all((p != 0).all() for p in U.bf16_pieces(fx.wp(), 3))          # three non-zero pieces everywhere
            nnz = (fx.x != 0).sum(1)
            assert nnz.max() == min(U.NNZ_B, K) and nnz.min() >= 1
    few = U.few_shifts(640, H, 2)
    assert U.b_span_ratio(few, mode) < 1.0 and len({k // 64 for k in np.flatnonzero(few.shift)}) == 4


def test_the_digit_step_is_the_rule_of_the_image_kernel():
    """digit_delta against the kernel's arithmetic (frexp, one comparison) on awkward maxima."""
    rng = np.random.default_rng(5)
    mx = np.concatenate([rng.uniform(1e-4, 3.0, 2000), 2.0 ** np.arange(-12.0, 3.0), 32638.0 * 2.0 ** np.arange(-20.0, -10.0),
                         8355710.0 * 2.0 ** np.arange(-30.0, -20.0)]).astype(np.float32)
    for D in (2, 3):
        f, x = np.frexp(mx)
        e = x - (8 * D - 1) + (np.ldexp(f, 8 * D - 1) > np.float32(U.DIGIT_LIM[D] - 1))
        assert np.array_equal(U.digit_delta(mx, D), np.ldexp(1.0, e))
    assert U.digit_delta(np.zeros(3), 2).tolist() == [1.0, 1.0, 1.0]
    q, delta = U.digit_q(U.fixture_a(96, H).wp(), 3)
    for D, planes in ((3, U.digit_planes(q, 3)),):
        assert all(p.min() >= -128 and p.max() <= 127 for p in planes)
        assert np.array_equal((planes[0] * 256 + planes[1]) * 256 + planes[2], q)


@pytest.mark.parametrize("mode", U.MODES)
def test_fixture_c_bound_is_tighter_than_one_snp(mode):
    for K, n, x_max in U.C_SHAPES:
        if x_max > 2 and mode[0] != "d":
            continue
        fx = U.fixture_c(K, H, n, x_max=x_max)
        bound = U.c_bound(fx, mode)
        k = int(np.argmax((fx.x.astype(np.float64) * np.abs(fx.wp()).max(1)[None, :]).max(0)))
        x = fx.x.copy()
        x[:, k] = 0
        less = U.Fixture("less", x, fx.W, fx.scale, fx.shift, fx.b1, False)
        assert (np.abs(less.ref64() - fx.ref64()) > bound).any(), (K, n, mode)
        # ... and the mode's own definition lies inside it with room for the accumulation
        own = np.abs(U.elu64(fx.z(mode)) - fx.ref64())
        assert (own <= bound).all()


def test_the_elu_bar_lies_below_a_lost_lowest_piece():
    """Fixture A has one term per element, so a lost lowest piece is not hidden by the other terms: the smallest change
    over all elements on the expm1 side must exceed the bar (fixture B fills its 24 bits - there the lowest piece of the
    smallest term can be one unit in the last place of the largest sum - and the digit modes may have a lowest digit of
    +-1: both are caught bit for bit on the positive side, which every element reaches in the W or the -W run)."""
    for K, n in ((96, 129), (280, 385), (128, 128)):
        fx = U.fixture_a(K, 256, n)
        for mode in ("p3", "p2", "p1"):
            assert U.ELU_ULP_BAR < U.lost_piece_ulps(fx, mode), (K, mode, U.lost_piece_ulps(fx, mode))
