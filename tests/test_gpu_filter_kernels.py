"""The window filter kernels at kernel level (locator_amd/csrc/filter_kernels.hip): loc_filter_snps_flags, loc_filter_snps_rows,
loc_dosage_flags and loc_dosage_rows called directly through the C ABI at the smallest shapes that can go wrong - calls per
variant around the 64 lanes, variants around the 4 of a workgroup, the 1024 chunks of the prefix sum and the 64-variant tile,
samples around the 960-sample LDS chunk, alleles on both sides of every 32-bit mask word, sums on both sides of every bound
of the filters - with hand-made keep / pos for the rows kernels.

The memory contract these tests state (include/locator_hip.h, the filter section):
  the flags launchers   write keep[0..V), pos[0..V) (kept or not) and n_kept, nothing else
  the rows launchers    write columns [0, K) of the rows whose sample_order[r] is in 0..N-1 and no other byte of the
                        [n_out][x_pitch] block (x_pitch > Kp included); n_out == 0 launches nothing
  all four              bad sizes -> -1, the function's name in loc_last_error(), nothing written
Every output is a guarded view of exactly its documented size, poisoned before the call.  The references are the NumPy
restatements of tests/filter_util.py; everything compared is an integer, so no tolerance appears anywhere."""
import numpy as np
import pytest
import torch

from locator_amd import _lib
from tests import filter_util as FU
from tests.gpu_util import guarded, poison

pytestmark = pytest.mark.gpu

KINDS = ("nan", "junk")
FILLS = ("0x77", "nan", "junk")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t):
    return t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _err(lib):
    return lib.loc_last_error().decode(errors="replace")


# ------------------------------------------------------------------ the four calls
def _flag_outputs(V, kind, seed=0):
    """keep uint8 [V], pos int32 [V], n_kept int32 [1]: guarded, poisoned.  -> the three views and their margin checks."""
    keep, c0 = guarded(V, torch.uint8)
    posf, c1 = guarded(V, torch.float32)
    nkf, c2 = guarded(1, torch.float32)
    for i, t in enumerate((keep, posf, nkf)):
        poison(t, kind, 3 * seed + i)
    return keep, posf.view(torch.int32), nkf.view(torch.int32), (lambda: c0("keep"), lambda: c1("pos"), lambda: c2("n_kept"))


def _flags(data, min_mac, kind="nan", seed=0):
    """loc_filter_snps_flags for int8 calls (V, N, P), loc_dosage_flags for float32 dosages (V, N).
    -> keep, pos, n_kept as the device left them; the margins are checked."""
    lib = _lib.load()
    d = _dev(data)
    V = data.shape[0]
    keep, pos, nk, checks = _flag_outputs(V, kind, seed)
    if data.dtype == np.int8:
        rc = lib.loc_filter_snps_flags(_p(d), V, data.shape[1], data.shape[2], int(min_mac), _p(keep), _p(pos), _p(nk),
                                       _stream())
    else:
        assert data.dtype == np.float32 and data.ndim == 2
        rc = lib.loc_dosage_flags(_p(d), V, data.shape[1], int(min_mac), _p(keep), _p(pos), _p(nk), _stream())
    assert rc == 0, _err(lib)
    for c in checks:
        c()
    return keep.cpu().numpy(), pos.cpu().numpy(), int(nk.cpu().numpy()[0])


def _same_flags(got, want, label):
    keep, pos, nk = got
    assert np.array_equal(keep, want[0]), (label, "keep", np.flatnonzero(keep != want[0])[:8])
    assert np.array_equal(pos, want[1]), (label, "pos", np.flatnonzero(pos != want[1])[:8])
    assert nk == want[2], (label, "n_kept", nk, want[2])


def _rows(data, keep, order, extra=0, fill="0x77", seed=0):
    """loc_filter_snps_rows / loc_dosage_rows with the hand-made flags `keep` (pos = their exclusive prefix sum) into a
    guarded, poisoned [n_out][Kp + extra] block.  The whole block is compared: columns [0, K) of the rows whose sample is
    inside the window hold the reference, every other byte what it held before the call."""
    lib = _lib.load()
    is_gt = data.dtype == np.int8
    V, N = data.shape[:2]
    keep = np.ascontiguousarray(keep, dtype=np.uint8)
    pos = FU.exclusive_cumsum(keep)
    K = int(keep.sum())
    order = np.ascontiguousarray(order, dtype=np.int32)
    n_out = len(order)
    pitch = (max(K, 1) + 31) // 32 * 32 + extra
    X, check = guarded(n_out * pitch, torch.uint8)
    if fill == "0x77":
        X.fill_(0x77)
    else:
        poison(X, fill, seed)
    torch.cuda.synchronize()
    want = X.cpu().numpy().reshape(n_out, pitch).copy()
    inside = (order >= 0) & (order < N)
    ref = (FU.rows_ref if is_gt else FU.dosage_rows_ref)(data, keep, pos, order[inside], K)
    want[inside, :K] = ref
    d, dk, dp, do = _dev(data), _dev(keep), _dev(pos), _dev(order)
    if is_gt:
        rc = lib.loc_filter_snps_rows(_p(d), V, N, data.shape[2], _p(dk), _p(dp), _p(do), n_out, _p(X), pitch, _stream())
    else:
        rc = lib.loc_dosage_rows(_p(d), V, N, _p(dk), _p(dp), _p(do), n_out, _p(X), pitch, _stream())
    assert rc == 0, _err(lib)
    check("X")
    got = X.cpu().numpy().reshape(n_out, pitch)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{len(bad)} bytes of the [{n_out}][{pitch}] block differ (K = {K}); first (row, column, got, "
                             f"want): {[(int(r), int(c), int(got[r, c]), int(want[r, c])) for r, c in bad[:6]]}")
    return ref


# ------------------------------------------------------------------ GT flags
_NP = {1: (1, 1), 63: (21, 3), 64: (32, 2), 65: (65, 1), 129: (43, 3)}            # calls per variant -> (N, P)


@pytest.mark.parametrize("V", [1, 3, 4, 5])
@pytest.mark.parametrize("n_calls", [1, 63, 64, 65, 129])
def test_gt_flags_calls_around_the_lanes_and_variants_around_the_workgroup(n_calls, V):
    """Lanes stride the calls by 64, a workgroup takes 4 variants: sites that are biallelic only through their first or
    only through their last call, in every position of the workgroup."""
    N, P = _NP[n_calls]
    rng = np.random.default_rng(100 * n_calls + V)
    seen = set()
    nk = len(FU.TAIL_KINDS)
    for rot in range(nk):
        kinds = [FU.TAIL_KINDS[(rot + i) % nk] for i in range(V)]
        gt = FU.tail_cases(n_calls, kinds, rng).reshape(V, N, P)
        want = FU.check_flags_ref(gt, 1)
        seen |= set(want[0].tolist())
        _same_flags(_flags(gt, 1, KINDS[rot % 2], rot), want, (n_calls, V, kinds))
    assert seen == ({0, 1} if n_calls > 1 else {0})                          # one call is never biallelic


@pytest.mark.parametrize("min_mac", [1, 2, 3])
def test_gt_flags_alleles_on_both_sides_of_every_mask_word(min_mac):
    gt = FU.as_calls(FU.allele_edge_cases(66), 2)
    want = FU.check_flags_ref(gt, min_mac)
    assert 0 < want[2] < len(gt)
    _same_flags(_flags(gt, min_mac, KINDS[min_mac % 2], min_mac), want, min_mac)
    if min_mac == 1:                                                          # the same sites, one workgroup each way round
        _same_flags(_flags(gt[::-1].copy(), 1, "junk", 7), FU.check_flags_ref(gt[::-1], 1), "reversed")


@pytest.mark.parametrize("n_calls,P", [(66, 2), (129, 3), (5, 1)])
def test_gt_flags_allele_1_counts_on_both_sides_of_min_mac(n_calls, P):
    gt = FU.as_calls(FU.mac_boundary_cases(n_calls, (1, 2, 3)), P)
    kept = []
    for mm in (1, 2, 3):
        want = FU.check_flags_ref(gt, mm)
        assert 0 < want[2] < len(gt)
        kept.append(want[2])
        _same_flags(_flags(gt, mm, KINDS[mm % 2], mm), want, (n_calls, mm))
    assert kept[0] > kept[1] > kept[2], kept


# ------------------------------------------------------------------ the prefix sum
@pytest.mark.parametrize("V", [1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 3077])
def test_scan_around_the_1024_chunks(V):
    """snp_scan_kernel through loc_filter_snps_flags: two haploid calls per variant, `0 1` = kept at min_mac 1.  chunk =
    ceil(V / 1024): one variant per thread up to 1024, two from 1025 (threads from 513 / 1024 / 1025 on start past V),
    four at 3077 (the last thread with work takes one variant).  pos is compared at every index, kept or not."""
    rng = np.random.default_rng(V)
    for i, (name, keep) in enumerate(FU.scan_patterns(V, rng).items()):
        gt = FU.scan_calls(keep)
        want = FU.flags_ref(gt, 1)
        assert np.array_equal(want[0], keep)
        _same_flags(_flags(gt, 1, KINDS[i % 2], i), want, (V, name))
    keep = FU.scan_patterns(V, rng)["random"]                                 # the dosage launcher runs the same kernel
    ds = np.repeat(keep.astype(np.float32)[:, None], 2, axis=1)
    want = FU.dosage_flags_ref(ds, 1)
    assert np.array_equal(want[0], keep)
    _same_flags(_flags(ds, 1, "junk", V), want, (V, "dosage"))


# ------------------------------------------------------------------ rows
# V, N, ploidy, per-tile pattern, n_out ("N": every sample), order, x_pitch - Kp.  Every listed value of every axis occurs,
# N in {960, 961, 1921} each with ploidy 3; the largest input is 129 x 1921 x 3 calls (0.74 MB) / x 4 bytes of dosage (0.99 MB).
ROW_CASES = [
    (1, 1, 1, "full", "N", "reversed", 0),
    (1, 961, 2, "full", 3, "repeated", 48),
    (1, 960, 3, "full", 5, "repeated", 0),
    (63, 959, 2, "random", 3, "subset", 48),
    (63, 1, 3, "last", 5, "repeated", 0),
    (63, 1921, 3, "first", "N", "reversed", 48),
    (64, 960, 3, "full", 4, "subset", 0),
    (64, 1921, 1, "first", 5, "repeated", 48),
    (64, 961, 1, "none", 3, "subset", 48),
    (64, 959, 2, "last", 4, "repeated", 0),
    (65, 961, 3, "last", 5, "subset", 48),
    (65, 959, 1, "first", 1, "subset", 0),
    (65, 960, 3, "random", 1, "subset", 0),
    (65, 1921, 2, "full", 4, "repeated", 0),
    (129, 1921, 3, "empty_between", "N", "reversed", 0),
    (129, 1921, 2, "random", 5, "subset", 48),
    (129, 1, 2, "last", 1, "subset", 48),
    (129, 959, 1, "full", "N", "reversed", 0),
    (129, 961, 2, "first", 5, "subset", 48),
    (193, 960, 1, "first", 4, "repeated", 0),
    (193, 960, 2, "random", "N", "reversed", 48),
    (193, 961, 2, "empty_between", "N", "reversed", 48),
    (193, 959, 3, "full", 3, "repeated", 0),
    (193, 961, 3, "last", 4, "subset", 0),
    (193, 1, 1, "empty_between", 1, "subset", 0),
]


def test_the_row_cases_hit_every_listed_value():
    col = lambda i: {c[i] for c in ROW_CASES}
    assert col(0) == {1, 63, 64, 65, 129, 193} and col(1) == {1, 959, 960, 961, 1921} and col(2) == {1, 2, 3}
    assert col(3) == set(FU.PATTERNS) and col(4) == {1, 3, 4, 5, "N"} and col(5) == {"reversed", "repeated", "subset"}
    assert col(6) == {0, 48}
    assert {c[1] for c in ROW_CASES if c[2] == 3} >= {960, 961, 1921}
    assert max(c[0] * c[1] * max(c[2], 4) for c in ROW_CASES) < 1 << 20


def _row_case(i):
    V, N, P, pattern, n_out, kind, extra = ROW_CASES[i]
    rng = np.random.default_rng(1000 + i)
    keep = FU.tile_pattern(V, pattern, rng)
    order = FU.make_order(N, N if n_out == "N" else n_out, kind, rng)
    return V, N, P, keep, order, extra, rng


@pytest.mark.parametrize("i", range(len(ROW_CASES)), ids=lambda i: "-".join(str(x) for x in ROW_CASES[i]))
def test_gt_rows_with_hand_made_flags(i):
    V, N, P, keep, order, extra, rng = _row_case(i)
    gt = FU.row_calls(V, N, P, rng)
    if V * N >= 64:
        assert set(np.unique((gt == 1).sum(axis=2))) == set(range(P + 1)) and {0, 2, -1, 127} <= set(np.unique(gt))
    ref = _rows(gt, keep, order, extra, FILLS[i % 3], i)
    if keep.any() and V * N >= 64:
        assert len(np.unique(ref)) > 1


@pytest.mark.parametrize("i", range(len(ROW_CASES)), ids=lambda i: "-".join(str(x) for x in ROW_CASES[i]))
def test_dosage_rows_with_hand_made_flags(i):
    V, N, _, keep, order, extra, rng = _row_case(i)
    ds = FU.dosage_matrix(V, N, rng)
    ref = _rows(ds, keep, order, extra, FILLS[(i + 1) % 3], i)
    if keep.all() and V * N >= 135 and len(order) == N:                       # every special value went through the kernel
        assert ref.min() == 0 and ref.max() == 2 * FU.UNIT and len(np.unique(ref)) >= 64


@pytest.mark.parametrize("form", ["gt", "dosage"])
def test_rows_of_every_special_dosage_and_every_allele_count(form):
    """One tile, every sample: all 135 special dosages (NaN, the infinities, -0.0, the range ends, 1e30, a denormal, every
    rounding tie) in kept variants / every count 0..3 of triploid calls."""
    rng = np.random.default_rng(5)
    if form == "gt":
        data = FU.row_calls(7, 50, 3, rng)
    else:
        sp = FU.special_values()
        data = np.ascontiguousarray(np.stack([np.roll(sp, 11 * v) for v in range(7)]))
    keep = np.array([1, 1, 0, 1, 1, 1, 1], np.uint8)
    ref = _rows(data, keep, np.arange(data.shape[1], dtype=np.int32), 48, "0x77")
    if form == "dosage":
        assert ref.min() == 0 and ref.max() == 2 * FU.UNIT and len(np.unique(ref)) >= 64


@pytest.mark.parametrize("form", ["gt", "dosage"])
@pytest.mark.parametrize("N", [5, 960, 961])
def test_rows_skip_a_sample_outside_the_window(form, N):
    """A row whose sample_order is not in 0..N-1 is not written at all (the wrappers refuse such an order)."""
    rng = np.random.default_rng(N)
    V = 70
    data = FU.row_calls(V, N, 2, rng) if form == "gt" else FU.dosage_matrix(V, N, rng)
    order = np.array([-1, N, 0, N + 1, 2 ** 31 - 1, N - 1, -960, 2 * 960, N, 1 % N], np.int32)
    _rows(data, FU.tile_pattern(V, "random", rng), order, 0, "0x77")
    _rows(data, FU.tile_pattern(V, "full", rng), order, 48, "junk", N)


# ------------------------------------------------------------------ dosage flags
@pytest.mark.parametrize("V", [1, 3, 4, 5])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_dosage_flags_samples_around_the_lanes_and_variants_around_the_workgroup(n, V):
    rng = np.random.default_rng(100 * n + V)
    seen = set()
    nk = len(FU.DOSAGE_TAIL_KINDS)
    for rot in range(nk):
        kinds = [FU.DOSAGE_TAIL_KINDS[(rot + i) % nk] for i in range(V)]
        ds = FU.dosage_tail_cases(n, kinds, rng)
        want = FU.check_dosage_flags_ref(ds, 1)
        seen |= set(want[0].tolist())
        _same_flags(_flags(ds, 1, KINDS[rot % 2], rot), want, (n, V, kinds))
    assert seen == {0, 1}


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129])
def test_dosage_flags_sums_on_both_sides_of_every_bound(n):
    """S = 63 m - 1 | 63 m for min_mac m in 1, 2, 5; S = 126 c - 1 | 126 c over c called samples among missing ones; S = 0;
    all missing; a single called sample."""
    ds = FU.dosage_boundary_cases(n, (1, 2, 5))
    for mm in (1, 2, 5):
        want = FU.check_dosage_flags_ref(ds, mm)
        if FU.UNIT * mm < 2 * FU.UNIT * n:                                    # else no site of n samples can pass: 63 m <= S < 126 n
            assert 0 < want[2] < len(ds), (n, mm, want[2])
        _same_flags(_flags(ds, mm, KINDS[mm % 2], mm), want, (n, mm))


@pytest.mark.parametrize("min_mac", [1, 2, 5])
def test_dosage_flags_of_every_special_value(min_mac):
    rng = np.random.default_rng(min_mac)
    sp = FU.special_values()
    ds = np.concatenate([FU.dosage_matrix(5, 65, rng), np.resize(sp, (2, 65)), np.resize(sp[::-1], (2, 65)),
                         np.resize(sp[8:48], (3, 65))]).astype(np.float32)       # the last: only small ties, low sums
    ds[-1, 5:] = np.nan
    want = FU.check_dosage_flags_ref(ds, min_mac)
    _same_flags(_flags(ds, min_mac, KINDS[min_mac % 2], min_mac), want, min_mac)
    wide = np.resize(sp, (3, 135)).astype(np.float32)
    wide[1] = np.roll(sp, 40)
    _same_flags(_flags(wide, min_mac, "junk", 9), FU.check_dosage_flags_ref(wide, min_mac), ("wide", min_mac))


# ------------------------------------------------------------------ refusals
def test_bad_sizes_are_refused_and_nothing_is_written():
    lib = _lib.load()
    big = (1 << 31) - 1023
    src = torch.zeros(64, dtype=torch.uint8, device="cuda")
    s = _stream()
    for kind in KINDS:
        keep, pos, nk, checks = _flag_outputs(8, kind, 1)
        Xf, cx = guarded(64, torch.float32)
        poison(Xf, kind, 5)
        X = Xf.view(torch.uint8)
        outs = (keep, pos, nk, X)
        torch.cuda.synchronize()
        before = [t.cpu().numpy().copy() for t in outs]
        g, k, p, n, x = _p(src), _p(keep), _p(pos), _p(nk), _p(X)
        refused = {
            "loc_filter_snps_flags": (lib.loc_filter_snps_flags, [
                (g, 0, 2, 2, 1, k, p, n, s), (g, 2, 0, 2, 1, k, p, n, s), (g, 2, 2, 0, 1, k, p, n, s), (g, -1, 2, 2, 1, k, p, n, s),
                (g, 2, (1 << 29) + 1, 2, 1, k, p, n, s), (g, 2, 1, (1 << 30) + 1, 1, k, p, n, s), (g, big, 2, 2, 1, k, p, n, s)]),
            "loc_filter_snps_rows": (lib.loc_filter_snps_rows, [
                (g, 0, 2, 2, k, p, p, 2, x, 32, s), (g, 2, 0, 2, k, p, p, 2, x, 32, s), (g, 2, 2, 0, k, p, p, 2, x, 32, s),
                (g, 2, 2, 2, k, p, p, -1, x, 32, s), (g, big, 2, 2, k, p, p, 2, x, 32, s), (g, big, 2, 2, k, p, p, 0, x, 32, s)]),
            "loc_dosage_flags": (lib.loc_dosage_flags, [
                (g, 0, 2, 1, k, p, n, s), (g, 2, 0, 1, k, p, n, s), (g, -1, 2, 1, k, p, n, s), (g, big, 2, 1, k, p, n, s)]),
            "loc_dosage_rows": (lib.loc_dosage_rows, [
                (g, 0, 2, k, p, p, 2, x, 32, s), (g, 2, 0, k, p, p, 2, x, 32, s), (g, 2, 2, k, p, p, -1, x, 32, s),
                (g, big, 2, k, p, p, 2, x, 32, s), (g, big, 2, k, p, p, 0, x, 32, s)]),
        }
        for name, (fn, calls) in refused.items():
            for args in calls:
                assert fn(*args) == -1, (name, args)
                msg = _err(lib)
                assert msg.startswith(name + ":") and f"n_variants={args[1]} " in msg + " ", (name, args, msg)
        # no row wanted: 0, and nothing launched
        assert lib.loc_filter_snps_rows(g, 2, 2, 2, k, p, p, 0, x, 32, s) == 0
        assert lib.loc_dosage_rows(g, 2, 2, k, p, p, 0, x, 32, s) == 0
        torch.cuda.synchronize()
        for c in checks:
            c()
        cx("X")
        for t, b in zip(outs, before):
            assert np.array_equal(t.cpu().numpy(), b)


# ------------------------------------------------------------------ the wrappers
def _windows():
    """(a window where nothing passes, one where every variant passes) as calls (V, N, 2) and as dosages (V, N)."""
    rng = np.random.default_rng(77)
    V, N = 70, 9
    none = np.zeros((V, N, 2), np.int8)
    none[::3] = 1
    none[1::3, 0, 0] = -1
    every = rng.integers(0, 2, (V, N, 2)).astype(np.int8)
    every[:, 0], every[:, 1] = (0, 1), (1, 1)
    every[::5, 2, 1] = -1
    return none, every


@pytest.mark.parametrize("form", ["gt", "dosage"])
def test_wrappers_on_windows_where_nothing_and_where_everything_passes(form):
    from locator_amd.net import filter_dosage_device, filter_snps_device
    order = np.array([8, 0, 3, 3, 5], np.int32)
    for name, gt in zip(("none", "every"), _windows()):
        V = len(gt)
        if form == "gt":
            want = FU.check_flags_ref(gt, 2)
            X, K, keep = filter_snps_device(_dev(gt), order, 2, return_keep=True)
            assert keep.dtype == np.uint8 and np.array_equal(keep, want[0]), name
            ref = FU.rows_ref(gt, want[0], want[1], order, want[2])
        else:
            ds = (gt == 1).sum(axis=2).astype(np.float32)
            ds[(gt < 0).any(axis=2)] = np.nan
            want = FU.check_dosage_flags_ref(ds, 2)
            X, K = filter_dosage_device(_dev(ds), order, 2)
            ref = FU.dosage_rows_ref(ds, want[0], want[1], order, want[2])
        assert K == want[2] == (0 if name == "none" else V), (name, K, want[2])
        Kp = (max(K, 1) + 31) // 32 * 32
        X = X.cpu().numpy()
        assert X.dtype == np.uint8 and X.shape == (len(order), Kp)
        assert np.array_equal(X[:, :K], ref) and not X[:, K:].any()
        if name == "every":
            assert ref.any()


@pytest.mark.parametrize("form", ["gt", "dosage"])
@pytest.mark.parametrize("bad", [[0, 9], [-1, 2], [3, 2 ** 31 - 1]])
def test_wrappers_refuse_a_sample_outside_the_window(form, bad):
    from locator_amd.net import filter_dosage_device, filter_snps_device
    gt = _windows()[1]
    with pytest.raises(ValueError, match="sample_order holds rows outside 0..8"):
        if form == "gt":
            filter_snps_device(_dev(gt), np.array(bad, np.int32), 2)
        else:
            filter_dosage_device(_dev((gt == 1).sum(axis=2).astype(np.float32)), np.array(bad, np.int32), 2)
    torch.cuda.synchronize()
