"""The three inference layer-1 GEMMs on the device, element for element: loc_l1_forward_rows (l1_rows.hip),
loc_l1_image_build + loc_l1_forward_gemm (l1_gemm.hip), loc_l1_image_i8_build + loc_l1_forward_gemm_i8 / _packed
(l1_gemm_i8.hip), called through the C ABI on the fixtures of tests/l1_infer_util.py (tests/test_l1_infer.py proves the
fixtures on the host).

Exact fixtures (A one-hot rows, B sparse rows, D shift term) are compared with np.array_equal on bit patterns wherever
z1 >= 0, and run with W and with -W so that every element is there once; where z1 < 0 the result is held to ELU_ULP_BAR units
in the last place of float64 expm1(z1).  Fixture C (dense) is held to the derived bound l1_infer_util.c_bound.  Every
output and scratch buffer is a guarded view of exactly the documented size (partial: the SNP groups asked for x Mp x Hp
floats, a1: ceil(n / 128) 128 rows, images: loc_l1_image_bytes / loc_l1_image_i8_bytes), poisoned with NaN patterns and
again with finite junk: both runs must give the same bits in all of a1, pad rows included, the guard margins must hold, and
after the NaN run exactly the group slabs the launcher's rule predicts are written (which also shows that the intended
kernel and group count ran).  `rows` is followed by indices of a sentinel row of 255s, X's pad columns K..pitch hold
genotypes 1..3 (the padding of W1S is zero, so they must not matter), the pads of scale / shift are zero as
loc_bn_infer_scale_shift leaves them.

LOOP PATHS AND THE SHAPES THAT REACH THEM
l1_rows.hip (k-tiles of 32 SNPs, group g walks tiles g, g + G, ...; pairs of tiles in the loop, an odd last tile after it;
tile i + 2 requested while tile i is multiplied, requests past the end clamped and masked):
  one group, 1 / 2 / 3 / 4 / 6 tiles               K = 32 / 64 / 96 / 128 / 161 (Kp = 192: the last tile is partly padding)
  nine tiles (K = 280) over G = 2, 3                5 + 4 and 3 + 3 + 3 tiles
  nine tiles, 9 groups asked -> 8                   group 0 has two tiles, the others one (cnt = 1: both prefetches clamped)
  every padded width 32 .. 512 x pieces             K = 96, n = 129, G = 2: odd unit-tile counts (TH = (NHT + 1) / 2), widths
                                                    whose weight tile is no multiple of the 512 threads; refused: 3 pieces
                                                    from width 384 on (LDS), anything outside 1..3 pieces
  rows_rt = 8 (256-row tiles, 4 waves)              width 256, pieces 1, 2, 3, n = 129, 256, 385, K = 280; n = 300 (three
                                                    128-row tiles) falls back to the default's bits
l1_gemm.hip (pairs of 64-SNP blocks, group g owns pairs g, g + G, ...; unrolled body of 6 blocks for 1 and 2 pieces with a
remainder of 2 or 4, body of 2 for 3 pieces; three weight tiles and two genotype pairs requested ahead, clamped at the end):
  one group, 1..6 pairs                             K = 128, 256, .., 768: remainder 2, remainder 4, body, body + 2, body + 4,
                                                    two bodies
  odd block counts (a zero tile pads the pair)      K = 64, 320;   less than a block / no multiple of 64: K = 32, 97
  five pairs over G = 2, 3                          K = 640: 3 + 2 and 2 + 2 + 1 pairs
  G = 8, nine pairs, more than one row tile         K = 1152, n = 256 and n = K: the (G & 7) == 0 placement
  l1_image_cvec_kernel: second turn of the strided loop and the tail: K = 24769 (388 blocks), fixture D
l1_gemm_i8.hip (group g owns a contiguous run of pairs, balanced to one; grid padded to a multiple of 8, surplus workgroups
leave; ring of 4 pairs; per sweep the unrolled body holds UP pairs - two planes: 3 (eight waves) or 2 (four waves), the
third plane's sweep: 3 or 4 - and up to UP - 1 pairs follow it):
  one group, 1..7 pairs                             K = 128 c: every remainder of every body, digits 2 and 3, unit tiles 1 and
                                                    2, packed genotypes
  odd / short                                       K = 32, 64, 97, 320
  uneven runs, n_mt G no multiple of 8              K = 640 (5 pairs), G = 2, 3, n = 257: runs 3 + 2 and 2 + 2 + 1, 6 and 9
                                                    workgroups in a grid of 8 and 16
  nine pairs over G = 5 (2 + 2 + 2 + 2 + 1) and G = 8 (the strided placement), n = 256
  l1_scan_kernel past its 256 workgroups: K = 24769, fixture D

MEASURED on one MI355X (every case prints its figure before it asserts):
  expm1 side of the exact cases: largest |a1 - expm1(z1)| over all 1,096 exact runs of this file = 0.875 ulp
  -> ELU_ULP_BAR = 2 (twice that, rounded up); the smallest change a lost lowest bf16 piece makes there is 19.9 ulp
  (tests/test_l1_infer.py).
  fixture C, largest error / bound (K = 1000, width 250; the larger of 1 and 4 SNP groups, every wave form):
                        rows p1   p2       p3        gemm p1   p2       p3        i8 d2    d3       (packed: the same)
    n = 257, x <= 2     0.185     0.0036   0.00034   0.185     0.0036   0.00037   0.026    0.00011
    n = 130, x <= 127                      0.00056                      0.00039   0.027    0.00013
  (the bound counts one rounding per addend in the worst direction; the kernels' errors are those of a random walk.)
WHAT THE FIRST RUN FOUND: loc_l1_image_build with 2 pieces, fixture A at K = 128 (and every other K): 43 of 15,785 elements a
unit of the second piece off.  l1_image_kernel's `w * scale[k]` was contracted with the subtraction of the first piece into
fma(w, s, -hi), so the lower pieces split the unrounded product while the first piece, l1_rows.hip and the documented
definition split w' = fl32(s w).  With 3 pieces the same contraction cut the product off at 24 bits where w' rounds it: in a
host restatement of the contracted form the pieces of 17,131 of these 32,000 weights do not add up to w' (one unit in its
last place).
Fixed in l1_gemm.hip (contraction off in that loop); the two bf16 kernels now agree bit for bit on these fixtures.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import l1_infer_util as U
from tests.gpu_util import guarded, poison, w1s_pack

pytestmark = pytest.mark.gpu

H = 250
KINDS = ("nan", "junk")
ELU_SEEN = []            # the ulp ratios on the expm1 side, printed by the last test of the file


@functools.lru_cache(maxsize=None)
def fx_a(K, h=H, n=None):
    return U.fixture_a(K, h, n)


@functools.lru_cache(maxsize=None)
def fx_b(K, n, h=H):
    assert (K, n) in U.B_SHAPES                 # the span condition is checked for these (tests/test_l1_infer.py)
    return U.fixture_b(K, h, n)


def groups(kernel, n, Kp, asked, target_blocks=0, big=False):
    """The SNP groups the launchers take: min(target_blocks / n_mt, scratch slabs, blocks), and in the two bf16 kernels
    rounded down to a multiple of 8 from 8 on."""
    rmt = 256 if big else 128
    n_mt = -(-n // rmt)
    blocks = Kp // 32 if kernel == "rows" else (((Kp + 63) // 64 + 1) & ~1) // 2
    G = min((target_blocks or 256) // n_mt, asked, blocks)
    if kernel != "i8" and G >= 8:
        G &= ~7
    return G, n_mt * rmt


class Dev:
    """One fixture on the device.  X holds the fixture's rows in a shuffled order (rows[] undoes it), junk 1..3 in the pad
    columns K..pitch and a sentinel row of 255s that the indices behind rows[n] point at."""

    def __init__(self, fx):
        from locator_amd import _lib
        self.L, self.lib, self.fx = _lib, _lib.load(), fx
        self.d = d = _lib.make_dims(fx.K, fx.H, 2)
        rng = np.random.default_rng(fx.K * 131 + fx.n)
        self.pitch = d.Kp + 16
        X = rng.integers(1, 4, (fx.n + 1, self.pitch)).astype(np.uint8)
        perm = rng.permutation(fx.n)
        X[perm, :fx.K] = fx.x
        X[fx.n] = 255
        rows = np.full(fx.n + 256, fx.n, np.int32)
        rows[:fx.n] = perm
        ss = np.zeros(2 * d.Kp, np.float32)
        ss[:fx.K], ss[d.Kp:d.Kp + fx.K] = fx.scale, fx.shift
        self.X, self.rows, self.ss = (torch.from_numpy(a).cuda() for a in (X, rows, ss))
        self.w, self.b1, self.buf, self._x2 = {}, {}, {}, None

    def set_shift(self, shift):
        ss = np.zeros(self.d.Kp, np.float32)
        ss[:self.fx.K] = shift
        self.ss[self.d.Kp:] = torch.from_numpy(ss).cuda()

    def weights(self, sign):
        if sign not in self.w:
            fx, d = self.fx, self.d
            self.w[sign] = torch.from_numpy(w1s_pack(sign * fx.W, d.Kp, d.Hp)).cuda()
            b1 = np.zeros(d.Hp, np.float32)
            b1[:fx.H] = sign * fx.b1
            self.b1[sign] = torch.from_numpy(b1).cuda()
        return self.w[sign], self.b1[sign]

    def x2(self):
        if self._x2 is None:
            p2 = self.d.Kp // 4 + 4
            self._x2 = torch.full((self.fx.n + 1, p2), 0xA5, dtype=torch.uint8, device="cuda")
            self.L.check(self.lib.loc_pack_genotypes_2bit(self.X.data_ptr(), self.pitch, self.fx.n + 1, self.d.Kp,
                                                          self._x2.data_ptr(), p2, None), "loc_pack_genotypes_2bit")
        return self._x2

    def take(self, name, n, dtype=torch.float32):
        """A guarded view of exactly n elements, kept for the next run of the same size."""
        key = (name, n, dtype)
        if key not in self.buf:
            self.buf[key] = guarded(n, dtype, 128 * self.d.Hp * (4 if dtype == torch.uint8 else 1))
        return self.buf[key]

    def run(self, kernel, mode, sign, asked, kind, target_blocks=0, tune=None, packed=False, x_max=3):
        """-> a1 [Mp][Hp] fp32 (host).  kernel: rows | gemm | i8; mode: p1..p3 | d2, d3; asked: SNP groups the scratch has
        room for; tune: dict of loc_tuning fields."""
        L, lib, d, fx = self.L, self.lib, self.d, self.fx
        planes = U.planes(mode)
        big = kernel == "rows" and bool(tune) and tune.get("rows_rt") == 8 and (-(-fx.n // 128)) % 2 == 0 and d.Hp == 256
        G, Mp = groups(kernel, fx.n, d.Kp, asked, target_blocks, big)
        w1s, b1 = self.weights(sign)
        partial, chk_p = self.take("partial", asked * Mp * d.Hp)
        a1, chk_a = self.take("a1", -(-fx.n // 128) * 128 * d.Hp)
        poison(partial, kind, 1)
        poison(a1, kind, 2)
        tn = C.byref(L.Tuning(**tune)) if tune else None
        checks = [("partial", chk_p), ("a1", chk_a)]
        if kernel == "rows":
            L.check(lib.loc_l1_forward_rows(self.X.data_ptr(), self.pitch, self.rows.data_ptr(), fx.n, C.byref(d),
                                            self.ss.data_ptr(), w1s.data_ptr(), b1.data_ptr(), partial.data_ptr(),
                                            partial.numel(), a1.data_ptr(), planes, target_blocks, tn, None),
                    "loc_l1_forward_rows")
        else:
            nbytes = int(lib.loc_l1_image_bytes(C.byref(d), planes) if kernel == "gemm" else
                         lib.loc_l1_image_i8_bytes(C.byref(d), planes))
            assert nbytes > 0
            image, chk_i = self.take("image", nbytes, torch.uint8)
            checks.append(("image", chk_i))
            poison(image, kind, 3)
            if kernel == "gemm":
                L.check(lib.loc_l1_image_build(C.byref(d), self.ss.data_ptr(), w1s.data_ptr(), planes, image.data_ptr(), None),
                        "loc_l1_image_build")
                L.check(lib.loc_l1_forward_gemm(self.X.data_ptr(), self.pitch, self.rows.data_ptr(), fx.n, C.byref(d),
                                                image.data_ptr(), planes, b1.data_ptr(), partial.data_ptr(),
                                                partial.numel(), a1.data_ptr(), target_blocks, None), "loc_l1_forward_gemm")
            else:
                L.check(lib.loc_l1_image_i8_build(C.byref(d), self.ss.data_ptr(), w1s.data_ptr(), planes, image.data_ptr(),
                                                  None), "loc_l1_image_i8_build")
                if packed:
                    X2 = self.x2()
                    L.check(lib.loc_l1_forward_gemm_i8_packed(X2.data_ptr(), X2.stride(0), self.rows.data_ptr(), fx.n,
                                                              C.byref(d), image.data_ptr(), planes, b1.data_ptr(),
                                                              partial.data_ptr(), partial.numel(), a1.data_ptr(),
                                                              target_blocks, tn, None), "loc_l1_forward_gemm_i8_packed")
                else:
                    L.check(lib.loc_l1_forward_gemm_i8(self.X.data_ptr(), self.pitch, self.rows.data_ptr(), fx.n, C.byref(d),
                                                       image.data_ptr(), planes, x_max, b1.data_ptr(), partial.data_ptr(),
                                                       partial.numel(), a1.data_ptr(), target_blocks, tn, None),
                            "loc_l1_forward_gemm_i8")
        torch.cuda.synchronize()
        for name, chk in checks:
            chk(f"{kernel} {mode} {fx.name} {name}")
        if kind == "nan":                      # exactly the slabs of the groups in use are written, every word of them
            words = partial.view(torch.int32).view(asked, -1)
            written = (words != -1).all(1).cpu().numpy()
            untouched = (words == -1).all(1).cpu().numpy()
            assert written[:G].all() and untouched[G:].all(), (kernel, mode, fx.name, G, written, untouched)
        return a1.view(-1, d.Hp).cpu().numpy()


def run_exact(dev, kernel, mode, asked, **kw):
    """Both signs x both poisons of one exact case -> the a1 of the W run (all Mp rows)."""
    fx = dev.fx
    z = fx.z(mode)
    out = None
    for sign in (1.0, -1.0):
        a = [dev.run(kernel, mode, sign, asked, kind, **kw) for kind in KINDS]
        assert np.array_equal(a[0].view(np.int32), a[1].view(np.int32)), (kernel, mode, fx.name, "depends on the scratch")
        what = f"{kernel} {mode} {fx.name} sign {sign:+.0f} G {asked} {kw}"
        ELU_SEEN.append(U.compare_exact(a[0][:fx.n, :fx.H], sign * z, what))
        assert not a[0][:fx.n, fx.H:].view(np.int32).any(), what + ": pad units must be +0.0"
        out = a[0] if out is None else out
    return out


ROWS_MODES, I8_FORMS = ("p1", "p2", "p3"), ((1, False), (2, False), (1, True))      # (unit tiles, packed)


def run_i8_forms(dev, asked, target_blocks=0, modes=("d2", "d3")):
    for mode in modes:
        outs = [run_exact(dev, "i8", mode, asked, target_blocks=target_blocks, tune={"gemm_i8_unit_tiles": ut}, packed=pk)
                for ut, pk in I8_FORMS]
        for o in outs[1:]:
            assert np.array_equal(outs[0].view(np.int32), o.view(np.int32)), (mode, dev.fx.name)


# ------------------------------------------------------------------ loc_l1_forward_rows
def rows_lds_fits(Hp, pieces):
    """Two stages of a 128-row genotype tile and `pieces` weight tiles (64 bytes per row / unit), and the shift vector."""
    return 2 * (128 * 64 + pieces * Hp * 64) + 4 * Hp <= 160 * 1024


@pytest.mark.parametrize("width", range(32, 513, 32))
def test_rows_every_width_and_piece_count(width):
    from locator_amd import _lib
    fx = fx_a(96, width, 129)
    dev = Dev(fx)
    for pieces in (1, 2, 3):
        ok = rows_lds_fits(width, pieces)
        assert bool(dev.lib.loc_l1_rows_supported(width, pieces)) == ok
        assert ok == (pieces < 3 or width <= 352)
        if ok:
            run_exact(dev, "rows", f"p{pieces}", 2)
        else:
            with pytest.raises(_lib.LocatorHipError, match="does not fit"):
                dev.run("rows", f"p{pieces}", 1.0, 2, "nan")
    assert not dev.lib.loc_l1_rows_supported(width, 0) and not dev.lib.loc_l1_rows_supported(width, 4)
    assert not dev.lib.loc_l1_rows_supported(width + 16, 1) and not dev.lib.loc_l1_rows_supported(544, 1)


@pytest.mark.parametrize("K", [32, 64, 96, 128, 161])
def test_rows_one_group(K):
    dev = Dev(fx_a(K))
    for mode in ROWS_MODES:
        run_exact(dev, "rows", mode, 1)
    for n in U.N_SWEEP:
        dev = Dev(fx_b(K, n))
        for mode in ROWS_MODES if n == 129 else ("p3",):
            run_exact(dev, "rows", mode, 1)


@pytest.mark.parametrize("asked", [2, 3, 9])
def test_rows_nine_tiles_split_over_groups(asked):
    for fx in (fx_a(280), fx_b(280, 129), fx_b(280, 257)):
        dev = Dev(fx)
        assert groups("rows", fx.n, dev.d.Kp, asked)[0] == {2: 2, 3: 3, 9: 8}[asked]
        for mode in ROWS_MODES:
            run_exact(dev, "rows", mode, asked)


@pytest.mark.parametrize("n", [129, 256, 385])
@pytest.mark.parametrize("mode", ROWS_MODES)
def test_rows_256_row_tiles(mode, n):
    """loc_tuning.rows_rt = 8: l1_rows_partial_kernel<8, P, 8, 256>.  target_blocks = two per 128-row tile gives the default
    kernel 2 groups and the 256-row kernel 4 - the slabs written say which one ran."""
    for fx in (fx_a(280, 256, n), fx_b(280, n, 256)):
        dev = Dev(fx)
        tb = 2 * (-(-n // 128))
        assert groups("rows", n, 288, 4, tb, big=True) == (4, -(-n // 256) * 256) and groups("rows", n, 288, 4, tb)[0] == 2
        big = run_exact(dev, "rows", mode, 4, target_blocks=tb, tune={"rows_rt": 8})
        small = run_exact(dev, "rows", mode, 4, target_blocks=tb)
        assert np.array_equal(big[:n].view(np.int32), small[:n].view(np.int32))


def test_rows_256_row_tiles_fall_back_on_an_odd_tile_count():
    fx = fx_a(280, 256, 300)
    dev = Dev(fx)
    for mode in ROWS_MODES:
        a = run_exact(dev, "rows", mode, 2, target_blocks=6, tune={"rows_rt": 8})       # 2 groups: the 128-row kernel
        b = run_exact(dev, "rows", mode, 2, target_blocks=6)
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


# ------------------------------------------------------------------ loc_l1_image_build + loc_l1_forward_gemm
@pytest.mark.parametrize("c", range(1, 7))
def test_gemm_one_group(c):
    for fx in (fx_a(128 * c), fx_b(128 * c, 129)):
        dev = Dev(fx)
        for mode in ROWS_MODES:
            run_exact(dev, "gemm", mode, 1)


@pytest.mark.parametrize("K", [32, 64, 97, 320])
def test_gemm_short_and_odd_block_counts(K):
    dev = Dev(fx_a(K))
    for mode in ROWS_MODES:
        run_exact(dev, "gemm", mode, 1)
    for n in U.N_SWEEP:
        dev = Dev(fx_b(K, n))
        for mode in ROWS_MODES if n == 129 else ("p3",):
            run_exact(dev, "gemm", mode, 3)                   # K = 320: three pairs, one each; else one group


@pytest.mark.parametrize("asked", [2, 3])
def test_gemm_five_pairs_split_over_groups(asked):
    for fx in (fx_a(640), fx_b(640, 257)):
        dev = Dev(fx)
        for mode in ROWS_MODES:
            run_exact(dev, "gemm", mode, asked)


def test_gemm_eight_groups_and_several_row_tiles():
    for fx in (fx_a(1152), fx_b(1152, 256)):
        dev = Dev(fx)
        assert groups("gemm", fx.n, dev.d.Kp, 9)[0] == 8
        for mode in ROWS_MODES:
            run_exact(dev, "gemm", mode, 9)


# ------------------------------------------------------------------ loc_l1_image_i8_build + loc_l1_forward_gemm_i8 / _packed
@pytest.mark.parametrize("c", range(1, 8))
def test_i8_one_group(c):
    for fx in (fx_a(128 * c), fx_b(128 * c, 129)):
        run_i8_forms(Dev(fx), 1)


@pytest.mark.parametrize("K", [32, 64, 97, 320])
def test_i8_short_and_odd_block_counts(K):
    run_i8_forms(Dev(fx_a(K)), 1)
    for n in U.N_SWEEP:
        run_i8_forms(Dev(fx_b(K, n)), 2, modes=("d2", "d3") if n == 129 else ("d3",))


@pytest.mark.parametrize("K,n,asked", [(640, 257, 2), (640, 257, 3), (1152, 256, 5), (1152, 256, 8)])
def test_i8_uneven_runs_and_both_placements(K, n, asked):
    for fx in (fx_a(K), fx_b(K, n)):
        dev = Dev(fx)
        assert groups("i8", fx.n, dev.d.Kp, asked)[0] == asked
        run_i8_forms(dev, asked)


# ------------------------------------------------------------------ fixture D: the shift term
ALL_KERNEL_MODES = [("rows", m) for m in ROWS_MODES] + [("gemm", m) for m in ROWS_MODES] + [("i8", "d2"), ("i8", "d3")]


def test_shift_term_small():
    """One-hot shifts at the ends and at a block edge of K = 161 (Kp = 192), every kernel and mode; then four shifts in four
    blocks on fixture B's weights."""
    for fx in [U.fixture_d(161, H, 129, {k: 1.0}) for k in (0, 63, 64, 160)] + [U.few_shifts(640, H, 129)]:
        dev = Dev(fx)
        for kernel, mode in ALL_KERNEL_MODES:
            a = run_exact(dev, kernel, mode, 2)
            if len(np.flatnonzero(fx.shift)) == 1:
                k = int(np.flatnonzero(fx.shift)[0])
                assert np.array_equal(np.maximum(a[:fx.n, :H], 0), np.maximum(np.tile(fx.W[k], (fx.n, 1)), 0))


def test_shift_term_at_24769_snps():
    """K = 24576 + 3 * 64 + 1, one row, x = 0: z1 = W1[k] for a one-hot shift at k, swept over the first and last SNP and
    both sides of blocks 127 | 128, 255 | 256 and 383 | 384 (l1_image_cvec_kernel: strided pairs, second turn, tail;
    l1_scan_kernel: blocks b and b + 256 of one workgroup; l1_rows: 775 k-tiles over 8 groups)."""
    K = U.BIG_K
    W = U.full_weights(K, 256, 7)
    fx = U.fixture_d(K, 256, 1, {0: 1.0}, weights=W)
    dev = Dev(fx)
    for k in U.BIG_SHIFT_SNPS:
        fx.shift[:] = 0
        fx.shift[k] = 1.0
        dev.set_shift(fx.shift)
        for kernel, mode in (("rows", "p3"), ("gemm", "p1"), ("i8", "d2")):
            a = run_exact(dev, kernel, mode, 8)
            assert np.array_equal(np.maximum(a[0], 0), np.maximum(W[k], 0)), (kernel, k)


# ------------------------------------------------------------------ fixture C: dense rows against the derived bound
@pytest.mark.parametrize("K,n,x_max", U.C_SHAPES)
def test_dense_rows_within_the_derived_bound(K, n, x_max):
    fx = U.fixture_c(K, H, n, x_max=x_max)
    dev = Dev(fx)
    ref = fx.ref64()
    cases = [("i8", "d2", {"gemm_i8_unit_tiles": 1}, False), ("i8", "d3", {"gemm_i8_unit_tiles": 1}, False),
             ("i8", "d2", {"gemm_i8_unit_tiles": 2}, False), ("i8", "d3", {"gemm_i8_unit_tiles": 2}, False)]
    if x_max <= 3:
        cases += [(k, m, None, False) for k in ("rows", "gemm") for m in ROWS_MODES]
        cases += [("i8", "d2", None, True), ("i8", "d3", None, True)]
    else:
        cases += [("rows", "p3", None, False), ("gemm", "p3", None, False)]       # any uint8 is exact in bf16
    for kernel, mode, tune, packed in cases:
        for asked in (1, 4):
            a = [dev.run(kernel, mode, 1.0, asked, kind, tune=tune, packed=packed, x_max=max(x_max, 3)) for kind in KINDS]
            assert np.array_equal(a[0].view(np.int32), a[1].view(np.int32))
            ratio = np.abs(a[0][:n, :H].astype(np.float64) - ref) / U.c_bound(fx, mode)
            print(f"fixture C K={K} n={n} x<={x_max} {kernel} {mode} {tune or ''}{' packed' if packed else ''} G={asked}: "
                  f"largest error / bound = {ratio.max():.4g}")
            assert ratio.max() <= 1.0, (kernel, mode, asked, float(ratio.max()))
            assert not a[0][:n, H:].any()


def test_zz_report_the_expm1_side():
    """Last in the file: the largest deviation on the expm1 side over every exact case that ran in this process."""
    if ELU_SEEN:
        print(f"expm1 side of {len(ELU_SEEN)} exact runs: largest |a1 - expm1(z1)| = {max(ELU_SEEN):.4g} ulp "
              f"(ELU_ULP_BAR = {U.ELU_ULP_BAR})")
        assert max(ELU_SEEN) <= U.ELU_ULP_BAR
