"""Fixtures and host forms of the inference layer-1 GEMMs (tests/test_l1_infer.py, tests/test_gpu_l1_infer.py):
loc_l1_forward_rows (l1_rows.hip), loc_l1_image_build + loc_l1_forward_gemm (l1_gemm.hip) and loc_l1_image_i8_build +
loc_l1_forward_gemm_i8 / _packed (l1_gemm_i8.hip).

What every one of them computes (include/locator_hip.h; the headers of the three files), for a MODE of carrying a weight:

    z1[m][h] = sum_k x[m][k] c(w'[k][h]) + sum_k t_k W1[k][h] + b1[h],      w'[k][h] = fl32(s_k W1[k][h]),
    a1 = z1 if z1 > 0 else expm1(z1)

    mode   c(w')                                                    kernels
    p3     w'  (hi = trunc16(w'), mid = trunc16(w' - hi), lo = w' - hi - mid: three bf16 values, their sum is w')
    p2     trunc16(w') + rne16(w' - trunc16(w'))                     rows, gemm: `pieces`
    p1     rne16(w')
    d2/d3  rint(w' / delta_h) delta_h, delta_h the smallest power of two with max_k |w'[k][h]| / delta_h <= lim - 1,
           lim = 127 (256^D - 1) / 255 = 32639 | 8355711 (1 where the unit has no weight)      gemm_i8: `digits`

trunc16 / rne16 keep the top 16 bits of an fp32 pattern (truncated / rounded to nearest even): a bf16 number.  The functions
below restate these definitions in NumPy; none of them follows a kernel's loops, tiles or summation order.

THE FIXTURES.  A, B and D are EXACT: every term of every element is an fp32 number and so is every partial sum of them in
any order (test_l1_infer.py checks that by summing in many random orders), so the expected a1 is known bit for bit whatever
the group split, the unrolling or the tile shapes - wherever z1 > 0.  Each exact case is run with W and with -W (a sign flip
of every piece and digit), so every element is on the positive side once; on the other side it is held to ELU_ULP_BAR units
in the last place against float64 expm1 of the exact z1, and z1 = 0 must give +0.0.

  A  one-hot rows: row m has one non-zero genotype x in {1, 2} at SNP k(m) = m stride mod K (stride coprime to K, 29 or more:
     a 128-row tile meets every 32- and 64-SNP block of K <= 3712 SNPs, hence every group); shift 0, b1 0; weights with all
     24 significand bits in use at Glorot scale, scales ordinary fp32 numbers: z1[m][h] = x c(w'[k(m)][h]).
  B  sparse rows: NNZ_B non-zero genotypes per row, one in each fifth of the SNP range; weights +-(a + b 2^-9 + c 2^-18) 2^-6
     with a, b, c in 1..3 (three non-zero bf16 pieces, 21 bits of span), scales 1/2 or 1: every term is a multiple of
     2^-25 below 2^-3.4, five of them stay below 2^24 units (b_span_ratio).  In the int8 modes the same numbers are integer
     multiples q of delta_h (delta_h divides the grid unit), the i32 sums are exact, and the fp32 fold of the kernel,
     (65536 S0 + 256 S1) delta + S2 delta with S_p = sum_k x digit_p, is exact too: 65536 S0 + 256 S1 = sum x (q - digit_2) is
     a multiple of 256 below 2^32 and the total is sum x q, below 2^24 units by the same condition.  So fixture B is
     bit-exact in all five modes (two digits: q <= 2^15, far inside).
  D  shift term: x = 0, b1 = 0, one-hot shift t_k = 1: z1[m][h] = W1[k][h] for every row, unscaled; and a few
     t_k in {+-1, +-2} on B's weights.
  C  dense rows (make_problem-style genotypes, Glorot weights, real scale, shift and b1) against the float64 forward, held
     to the derived bound below.

THE BOUND OF FIXTURE C (c_bound).  With u = 2^-24 and S[m][h] = sum_k |x| |w'| + sum_k |t_k| |W1| + |b1|:
  - w' = s W1 (1 + e), |e| <= u: the product terms are off by at most u sum |x| |w'| before anything is added        [1]
  - z1 is a sum of N = planes K + K + 1 numbers (the planes K exact products x piece, the K shift terms - each enters by one
    fused multiply-add, so its product is not rounded on its own - and b1) in some order the kernel chooses: SNP groups, the
    matrix pipe's accumulation, the reductions.  For ANY order of recursive summation the error is at most
    (N - 1) u sum |terms| (Jeannerod and Rump 2013, no higher-order term), taking every accumulation of the matrix pipe to
    round no worse than an fp32 addition; the terms are those of [1], (1 + u) larger at most: (N - 1) u (1 + u) S <=
    ((N - 1) + 1) u S while N u <= 1                                                                            [N - 1, + 1]
  - ELU is 1-Lipschitz, and expm1f adds ELU_ULP_BAR units in the last place of a result no larger than |z1| <= (1 + N u) S:
    2 ELU_ULP_BAR u S                                                                                  [2 ELU_ULP_BAR]
  so |a1 - ref64| <= (N + C_CONST) u S with n_terms = N and C_CONST = 2 + 2 ELU_ULP_BAR, plus what the mode gives up:
  2^-9 sum |x| |w'| for one piece (rne16 keeps 8 bits), 2^-17 for two (hi is exact, the rest is rounded to 8 bits 2^-8
  below), max_k |w'| 2^-(8 D) sum |x| for D digits.  The int8 modes add integers exactly and round only in the fold and
  the group sums, so N over-counts there; the bound holds all the same.  (The digit term is the one the kernel's header
  states.  The strict worst case of one weight is delta_h / 2, which lies between max |w'| 2^-(8 D) and twice that,
  depending on where max |w'| falls between two powers of two; over hundreds of SNPs the rounding errors do not line up, and
  the measured ratios in tests/test_gpu_l1_infer.py show how far below the stated term the kernels stay.)
"""
import numpy as np

U24 = 2.0 ** -24
MODES = ("p1", "p2", "p3", "d2", "d3")
NNZ_B = 5
ELU_ULP_BAR = 2          # twice the 0.875 ulp measured on the device, rounded up: tests/test_gpu_l1_infer.py
C_CONST = 2 + 2 * ELU_ULP_BAR
DIGIT_LIM = {2: 32639.0, 3: 8355711.0}


def planes(mode):
    return int(mode[1])


# ---------------------------------------------------------------- number formats
def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def trunc16(a):
    """The top 16 bits of each fp32 pattern (a bf16 number, truncated towards zero)."""
    return (_u32(a) & np.uint32(0xFFFF0000)).view(np.float32)


def rne16(a):
    """Each fp32 number rounded to bf16, nearest even."""
    u = _u32(a).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)


def scaled_weight(W, scale):
    """w' = fl32(s_k W1[k][h])"""
    return np.asarray(W, np.float32) * np.asarray(scale, np.float32)[:, None]


def bf16_pieces(wp, pieces):
    """The `pieces` bf16 numbers (as fp32 arrays) that stand for w'."""
    wp = np.asarray(wp, np.float32)
    if pieces == 1:
        return [rne16(wp)]
    hi = trunc16(wp)
    if pieces == 2:
        return [hi, rne16(wp - hi)]
    mid = trunc16(wp - hi)
    return [hi, mid, wp - hi - mid]


def digit_delta(mx, digits):
    """The per-unit step: the smallest power of two with mx / delta <= lim - 1; 1 where mx = 0."""
    mx = np.asarray(mx, np.float64)
    e = np.ceil(np.log2(np.where(mx > 0, mx, 1.0) / (DIGIT_LIM[digits] - 1.0)))
    delta = np.where(mx > 0, np.exp2(e), 1.0)
    live = mx > 0
    assert np.all(mx[live] / delta[live] <= DIGIT_LIM[digits] - 1) and np.all(2 * mx[live] / delta[live] > DIGIT_LIM[digits] - 1)
    return delta


def digit_q(wp, digits):
    """-> (q [K][H] int64, delta [H] float64): the fixed-point weights of the int8 image."""
    wp = np.asarray(wp, np.float32).astype(np.float64)
    delta = digit_delta(np.abs(wp).max(0) if wp.shape[0] else np.zeros(wp.shape[1]), digits)
    return np.rint(wp / delta).astype(np.int64), delta


def digit_planes(q, digits):
    """Signed base-256 digits of q, most significant first; every digit in -128..127 (the top one takes what is left)."""
    out, q = [], q.copy()
    for _ in range(digits - 1):
        lo = ((q + 128) & 255) - 128
        out.append(lo)
        q = (q - lo) >> 8
    out.append(q)
    return out[::-1]


def mode_terms(wp, mode):
    """The float64 arrays [K][H] whose products with a genotype a kernel adds up in fp32: the bf16 pieces, or q delta (the
    digits of one weight meet in an exact integer sum)."""
    if mode[0] == "p":
        return [p.astype(np.float64) for p in bf16_pieces(wp, planes(mode))]
    q, delta = digit_q(wp, planes(mode))
    return [q * delta]


def lowest_term(wp, mode):
    """What a kernel that loses the lowest piece / digit plane of a weight loses, float64 [K][H]."""
    if mode[0] == "p":
        return bf16_pieces(wp, planes(mode))[-1].astype(np.float64)
    q, delta = digit_q(wp, planes(mode))
    return digit_planes(q, planes(mode))[-1] * delta


def carried_weight(wp, mode):
    """c(w') in float64 (exact: the pieces of one weight span 24 bits at most)."""
    return sum(mode_terms(wp, mode))


def elu64(z):
    return np.where(z > 0, z, np.expm1(np.minimum(z, 0.0)))


def is_fp32(a):
    a = np.asarray(a, np.float64)
    return a.astype(np.float32).astype(np.float64) == a


def ulp32(a):
    from tests.gpu_util import ulp32 as f
    return f(a)


# ---------------------------------------------------------------- fixtures
class Fixture:
    """x [n][K] uint8, W [K][H] fp32 (Keras orientation), scale / shift [K] fp32, b1 [H] fp32; exact: A, B, D."""

    def __init__(self, name, x, W, scale, shift, b1, exact):
        self.name, self.exact = name, exact
        self.x = np.ascontiguousarray(x, np.uint8)
        self.W = np.ascontiguousarray(W, np.float32)
        self.scale, self.shift, self.b1 = (np.ascontiguousarray(a, np.float32) for a in (scale, shift, b1))
        self.n, self.K = self.x.shape
        self.H = self.W.shape[1]
        assert self.W.shape[0] == self.K == self.scale.size == self.shift.size and self.b1.size == self.H

    def negated(self):
        """The same fixture with -W (and -b1): every piece and digit changes its sign only, z1 -> -z1."""
        return Fixture(self.name + "-", self.x, -self.W, self.scale, self.shift, -self.b1, self.exact)

    def wp(self):
        return scaled_weight(self.W, self.scale)

    def z(self, mode):
        """z1 [n][H] in float64: for an exact fixture the exact value, asserted to be an fp32 number."""
        z = self.shift.astype(np.float64) @ self.W.astype(np.float64) + self.b1.astype(np.float64)
        z = z[None, :] + (self.x.astype(np.float64) @ carried_weight(self.wp(), mode) if self.x.any() else np.zeros((self.n, 1)))
        if self.exact:
            assert is_fp32(z).all(), (self.name, mode)
        return z

    def ref64(self):
        """The float64 forward on the fp32 inputs: no fl32(s W), no pieces."""
        xh = self.x.astype(np.float64) * self.scale.astype(np.float64) + self.shift.astype(np.float64)
        return elu64(xh @ self.W.astype(np.float64) + self.b1.astype(np.float64))

    def terms(self, mode):
        """[n][J][H] float32: the non-zero addends of every element, J = the most any row has (zero padded): x piece for
        every non-zero genotype and piece, t_k W1[k][h] for every non-zero shift."""
        T = mode_terms(self.wp(), mode) if self.x.any() else []
        ks = [np.flatnonzero(r) for r in self.x]
        kt = np.flatnonzero(self.shift)
        J = max(len(k) for k in ks) * len(T) + len(kt)
        out = np.zeros((self.n, max(J, 1), self.H), np.float64)
        for m, k in enumerate(ks):
            j = 0
            for t in T:
                out[m, j:j + len(k)] = self.x[m, k, None].astype(np.float64) * t[k]
                j += len(k)
            out[m, j:j + len(kt)] = self.shift[kt, None].astype(np.float64) * self.W[kt].astype(np.float64)
        assert is_fp32(out).all()
        return out.astype(np.float32)


def _stride(K):
    s = 29
    while np.gcd(s, K) != 1:
        s += 1
    return s


def full_weights(K, H, seed, scale=None):
    """fp32 weights of both signs at Glorot scale (|w| uniform in 1/4 .. 1 of sqrt(6 / (K + H))) with unrestricted
    significands, drawn again while the lowest of the three bf16 pieces of w' = fl32(scale w) is below 2^-19 |w'| (bit 15
    of the significand field clear, so that the middle piece reaches into the low byte, or a low byte below 32; 44 % of
    all draws pass): all 24 bits of w' are in use, and losing the lowest piece moves expm1 by several units in the last
    place (lost_piece_ulps)."""
    rng = np.random.default_rng(seed)
    lim = np.sqrt(6.0 / (K + H))
    scale = np.ones(K, np.float32) if scale is None else np.asarray(scale, np.float32)
    w = np.zeros((K, H), np.float32)
    todo = np.ones((K, H), bool)
    while todo.any():
        cnt = int(todo.sum())
        w[todo] = (rng.uniform(0.25 * lim, lim, cnt) * rng.choice([-1.0, 1.0], cnt)).astype(np.float32)
        u = (w * scale[:, None]).view(np.uint32)
        todo = ((u >> 15) & 1 == 0) | ((u & 255) < 32)
    return w


def plain_scales(K, seed):
    """Ordinary non-round fp32 BatchNorm scales gamma / sqrt(var + eps) in 0.6 .. 2.9."""
    rng = np.random.default_rng(seed + 1)
    return (rng.uniform(0.7, 1.3, K) / np.sqrt(rng.uniform(0.2, 1.2, K) + 1e-3)).astype(np.float32)


def a_snp(m, K):
    return (m * _stride(K)) % K


def fixture_a(K, H, n=None, seed=0, snp_offset=0):
    """Row m: x = 1 + (k + m // K) % 2 at SNP k = a_snp(m, K) (+ snp_offset, for the sensitivity tests); n = K by default -
    every SNP once; rows K.. repeat SNPs with the other genotype."""
    n = K if n is None else n
    x = np.zeros((n, K), np.uint8)
    m = np.arange(n)
    k = (a_snp(m, K) + snp_offset) % K
    x[m, k] = 1 + (a_snp(m, K) + m // K) % 2
    scale = plain_scales(K, seed + K)
    return Fixture(f"A{K}x{H}n{n}", x, full_weights(K, H, seed + K, scale), scale, np.zeros(K), np.zeros(H), True)


def grid_weights(K, H, seed):
    """+-(a + b 2^-9 + c 2^-18) 2^-6 with a, b, c in 1..3."""
    rng = np.random.default_rng(seed + 2)
    a, b, c = (rng.integers(1, 4, (K, H)).astype(np.float64) for _ in range(3))
    w = (a + b * 2.0 ** -9 + c * 2.0 ** -18) * 2.0 ** -6 * rng.choice([-1.0, 1.0], (K, H))
    assert is_fp32(w).all()
    return w.astype(np.float32)


def fixture_b(K, H, n, seed=0):
    """Row m: genotypes 1 or 2 at NNZ_B SNPs, one drawn from each fifth of 0..K (fewer when K < NNZ_B)."""
    rng = np.random.default_rng(seed + 3 + 1000 * K + n)
    x = np.zeros((n, K), np.uint8)
    edges = np.unique(np.linspace(0, K, NNZ_B + 1).astype(int))
    for lo, hi in zip(edges[:-1], edges[1:]):
        x[np.arange(n), rng.integers(lo, hi, n)] = rng.integers(1, 3, n)
    scale = rng.choice(np.array([0.5, 1.0], np.float32), K)
    return Fixture(f"B{K}x{H}n{n}", x, grid_weights(K, H, seed + K), scale, np.zeros(K), np.zeros(H), True)


def b_span_ratio(fx, mode):
    """max over (row, unit) of sum |terms| / (2^24 units), the unit being the largest power of two that divides every
    non-zero term of the fixture: below 1, every partial sum in every order is an fp32 number."""
    t = fx.terms(mode).astype(np.float64)
    nz = np.abs(t[t != 0])
    unit = 2.0 ** np.floor(np.log2(nz.min()))
    while not np.all(nz / unit == np.rint(nz / unit)):
        unit /= 2
    return float(np.abs(t).sum(1).max() / (2.0 ** 24 * unit))


def fixture_d(K, H, n, shift_at, seed=0, weights=None):
    """x = 0, b1 = 0, shift = {k: t_k}: z1[m][h] = sum_k t_k W1[k][h] for every row."""
    W = full_weights(K, H, seed + K) if weights is None else weights
    shift = np.zeros(K, np.float32)
    for k, t in shift_at.items():
        shift[k] = t
    return Fixture(f"D{K}x{H}n{n}", np.zeros((n, K), np.uint8), W, plain_scales(K, seed + K), shift, np.zeros(H), True)


def few_shifts(K, H, n, seed=0):
    """Fixture D on B's weights: t = 1, -2, 2, -1 at four SNPs in four different 64-SNP blocks (K >= 448)."""
    at = {5: 1.0, 64 * 3 + 17: -2.0, 64 * 6 + 63: 2.0, K - 1: -1.0}
    return fixture_d(K, H, n, at, seed, weights=grid_weights(K, H, seed + K))


# the one large input: 388 blocks of 64 SNPs, the last one a single SNP - the second turn of l1_image_cvec_kernel's strided
# loop and its tail, more than one stride of l1_scan_kernel's 256 workgroups
BIG_K = 24576 + 3 * 64 + 1
BIG_SHIFT_SNPS = (0, 128 * 64 - 1, 128 * 64, 256 * 64 - 1, 256 * 64, 384 * 64 - 1, 384 * 64, BIG_K - 1)

N_SWEEP = (1, 127, 128, 129, 257)
# (K, n) of every fixture B that tests/test_gpu_l1_infer.py runs
B_SHAPES = tuple(sorted({(K, n) for K in (32, 64, 96, 97, 128, 161, 320) for n in N_SWEEP}
                        | {(128 * c, 129) for c in range(1, 8)}
                        | {(280, n) for n in (129, 256, 257, 385)} | {(640, 257), (1152, 129), (1152, 256)}))
# (K, n, largest genotype) of every fixture C
C_SHAPES = ((1000, 257, 2), (1000, 130, 127))


def fixture_c(K, H, n, seed=0, x_max=2):
    """Dense rows: genotypes binomial(2, beta-distributed frequency) as gpu_util.make_problem (x_max > 2: uniform in
    0..x_max), Glorot-uniform weights, BatchNorm constants and b1 drawn as gpu_util.randomize_params draws them."""
    rng = np.random.default_rng(seed + 4 + K + n)
    if x_max <= 2:
        x = rng.binomial(2, rng.beta(0.4, 0.9, K).clip(0.02, 0.98), (n, K))
    else:
        x = rng.integers(0, x_max + 1, (n, K))
    lim = np.sqrt(6.0 / (K + H))
    W = rng.uniform(-lim, lim, (K, H)).astype(np.float32)
    gamma, beta = rng.uniform(0.7, 1.3, K), rng.normal(0, 0.05, K)
    mean, var = rng.uniform(0, 1, K), rng.uniform(0.2, 1.2, K)
    scale = (gamma / np.sqrt(var + 1e-3)).astype(np.float32)
    shift = (beta - mean * scale).astype(np.float32)
    return Fixture(f"C{K}x{H}n{n}", x, W, scale, shift, rng.normal(0, 0.05, H), False)


def c_bound(fx, mode):
    """The per-element bound of |a1 - fx.ref64()| derived in the module docstring, [n][H] float64."""
    x = fx.x.astype(np.float64)
    awp = np.abs(fx.wp().astype(np.float64))
    sx = x @ awp
    S = sx + np.abs(fx.shift.astype(np.float64)) @ np.abs(fx.W.astype(np.float64)) + np.abs(fx.b1.astype(np.float64))
    n_terms = planes(mode) * fx.K + fx.K + 1
    assert n_terms * U24 <= 1
    bound = (n_terms + C_CONST) * U24 * S
    if mode == "p1":
        bound = bound + 2.0 ** -9 * sx
    elif mode == "p2":
        bound = bound + 2.0 ** -17 * sx
    elif mode[0] == "d":
        bound = bound + awp.max(0)[None, :] * 2.0 ** (-8 * planes(mode)) * x.sum(1)[:, None]
    return bound


# ---------------------------------------------------------------- comparing a device result with an exact fixture
def expected_bits(z):
    """int32 bit patterns of a1 where z1 >= 0 (z1 itself; +0.0 for 0), and the mask of those elements."""
    pos = z >= 0
    return np.where(z > 0, z, 0.0).astype(np.float32).view(np.int32), pos


def compare_exact(a1, z, what=""):
    """a1 [n][H] fp32 from the device against the exact z1 [n][H]: bit for bit where z1 >= 0 (+0.0 for z1 = 0), within
    ELU_ULP_BAR units in the last place of float64 expm1(z1) elsewhere.  -> the largest such ratio (in ulp)."""
    a1 = np.ascontiguousarray(a1, np.float32)
    want, pos = expected_bits(z)
    got = a1.view(np.int32)
    bad = np.argwhere(pos & (got != want))
    assert len(bad) == 0, (f"{what}: {len(bad)} of {int(pos.sum())} elements with z1 >= 0 differ from the exact value, first at "
                           f"(row, unit) {tuple(bad[0])}: got {a1[tuple(bad[0])]!r}, want {np.float32(z[tuple(bad[0])])!r}")
    neg = ~pos
    if not neg.any():
        return 0.0
    ref = np.expm1(z[neg])
    ratio = np.abs(a1[neg].astype(np.float64) - ref) / ulp32(ref)
    worst = float(ratio.max())
    assert worst <= ELU_ULP_BAR, f"{what}: expm1 side off by {worst:.3g} ulp (bar {ELU_ULP_BAR})"
    return worst


def lost_piece_ulps(fx, mode="p3"):
    """The smallest change, in units in the last place of a1, that losing the lowest piece of ONE non-zero term makes on the
    expm1 side of fixture fx (and of its negation): min over elements with z1 < 0 and over their non-zero terms."""
    out = np.inf
    for f in (fx, fx.negated()):
        z = f.z(mode)
        low = lowest_term(f.wp(), mode)
        for m in range(f.n):
            for k in np.flatnonzero(f.x[m]):
                lost = f.x[m, k] * low[k]
                sel = (z[m] < 0) & (lost != 0)
                if sel.any():
                    a = np.expm1(z[m][sel])
                    out = min(out, float((np.abs(np.expm1(z[m][sel] - lost[sel]) - a) / ulp32(a)).min()))
    return out
