"""References and case builders of the window filter tests (tests/test_gpu_filter_kernels.py on the device,
tests/test_host.py for the C twin in csrc/codecs.c).  The references are NumPy restatements of the definitions in
include/locator_hip.h (the filter section), spelled with the host forms of locator_amd/genotypes.py; everything is an
integer, so every comparison made with them is np.array_equal.

Calls are built flat, int8 [variants][n_calls]; the caller views them as (variants, n_samples, ploidy) with
n_samples * ploidy = n_calls (as_calls)."""
import numpy as np

from locator_amd import genotypes as G

UNIT = G.DOSAGE_UNIT                                        # 63
ALLELES = (0, 1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 126, 127)      # both sides of every 32-bit (and the 64-bit) mask word
MISSING_CODES = (-1, -2, -128)
FT, FS = 64, 960                                            # filter_kernels.hip: variants per tile, samples per LDS chunk


def exclusive_cumsum(keep):
    keep = np.asarray(keep, np.uint8)
    pos = np.zeros(len(keep), np.int32)
    np.cumsum(keep[:-1], out=pos[1:])
    return pos


def as_calls(flat, ploidy):
    flat = np.ascontiguousarray(flat, dtype=np.int8)
    V, n_calls = flat.shape
    assert n_calls % ploidy == 0, (n_calls, ploidy)
    return flat.reshape(V, n_calls // ploidy, ploidy)


# ------------------------------------------------------------------ references
def flags_ref(gt, min_mac):
    """loc_filter_snps_flags: (keep uint8 [V], pos int32 [V] = exclusive prefix sum of keep over ALL variants, n_kept).
    keep = exactly two distinct called alleles and - unless min_mac == 1 - allele 1 at least min_mac times: count_alleles ->
    is_biallelic -> the allele-1 count, as genotypes.filter_snps(native=False) spells it."""
    gt = np.asarray(gt, np.int8)
    keep = G.is_biallelic(G.count_alleles(gt))
    if not min_mac == 1:
        keep = keep & (G.count_alleles(gt, max(int(gt.max()), 1))[:, 1] >= min_mac)
    keep = keep.astype(np.uint8)
    return keep, exclusive_cumsum(keep), int(keep.sum())


def check_flags_ref(gt, min_mac):
    """flags_ref pinned to genotypes.filter_snps(native=False): the same sites, the same matrix.  -> flags_ref's result."""
    keep, pos, K = flags_ref(gt, min_mac)
    ac, idx = G.filter_snps(np.asarray(gt, np.int8), min_mac, verbose=False, native=False, sites=True)
    assert np.array_equal(np.flatnonzero(keep), idx), (np.flatnonzero(keep)[:8], idx[:8])
    order = np.arange(gt.shape[1])
    assert np.array_equal(rows_ref(gt, keep, pos, order, K), np.asarray(ac).T.astype(np.uint8))
    return keep, pos, K


def rows_ref(gt, keep, pos, order, K):
    """loc_filter_snps_rows: X[r, pos[v]] = (gt[v, order[r], :] == 1).sum() for kept v; uint8 [len(order)][K]."""
    gt = np.asarray(gt, np.int8)
    kv = np.flatnonzero(keep)
    assert len(kv) == K
    X = np.zeros((len(order), K), np.uint8)
    if K:
        X[:, np.asarray(pos)[kv]] = (gt[kv][:, np.asarray(order, np.int64), :] == 1).sum(axis=2).T
    return X


def dosage_flags_ref(ds, min_mac):
    """loc_dosage_flags: over the called samples S = sum(q) >= 63 min_mac, S > 0 and S < 126 n_called."""
    with np.errstate(invalid="ignore", over="ignore"):
        q = G.dosage_q(ds)
    S, called = G.dosage_site_sums(q)
    keep = ((S >= UNIT * int(min_mac)) & (S > 0) & (S < 2 * UNIT * called)).astype(np.uint8)
    return keep, exclusive_cumsum(keep), int(keep.sum())


def check_dosage_flags_ref(ds, min_mac):
    """dosage_flags_ref pinned to genotypes.filter_dosage: its matrix is the kept rows of q, missing -> 0."""
    keep, pos, K = dosage_flags_ref(ds, min_mac)
    with np.errstate(invalid="ignore", over="ignore"):
        ac = G.filter_dosage(G.dosage_q(ds), min_mac, verbose=False)
    assert ac.shape[0] == K
    assert np.array_equal(dosage_rows_ref(ds, keep, pos, np.arange(np.shape(ds)[1]), K), ac.T)
    return keep, pos, K


def dosage_rows_ref(ds, keep, pos, order, K):
    """loc_dosage_rows: X[r, pos[v]] = q of sample order[r] at kept v, missing -> 0."""
    with np.errstate(invalid="ignore", over="ignore"):
        q = G.dosage_q(ds)
    q = np.where(q == G.Q_MISSING, 0, q).astype(np.uint8)
    kv = np.flatnonzero(keep)
    assert len(kv) == K
    X = np.zeros((len(order), K), np.uint8)
    if K:
        X[:, np.asarray(pos)[kv]] = q[kv][:, np.asarray(order, np.int64)].T
    return X


# ------------------------------------------------------------------ calls
def _site(n_calls, base, i, *others):
    """All calls `base`; others = (value, offset): call (7 i + offset) % n_calls becomes value (later ones win)."""
    row = np.full(n_calls, base, np.int16)
    for value, off in others:
        row[(7 * i + off) % n_calls] = value
    return row


def allele_edge_cases(n_calls=66):
    """One variant per ordered pair (a, b) of ALLELES: every call a, one call b, one call missing (coded -1 / -2 / -128 in
    turn; a == b gives a monomorphic site), the odd calls at places that move with the variant.  Then a and a + 32, a and
    a + 64 half and half (one bit position in two mask words), a tri-allelic site over three words (0, 40, 100), an
    all-missing site, a site with a single called allele and three sites of alleles {0, 1} with every missing code."""
    assert n_calls >= 6
    rows = []
    for a in ALLELES:
        for b in ALLELES:
            i = len(rows)
            rows.append(_site(n_calls, a, i, (b, 0), (MISSING_CODES[i % 3], 3)))
    half = np.arange(n_calls) % 2 == 0
    for a in ALLELES:
        for step in (32, 64):
            if a + step <= 127:
                rows.append(np.where(half, a, a + step))
    tri = np.zeros(n_calls, np.int16)
    tri[1::3], tri[2::3] = 40, 100
    rows.append(tri)
    rows.append(np.resize(np.array(MISSING_CODES, np.int16), n_calls))           # all missing
    one = np.full(n_calls, -1, np.int16)
    one[n_calls - 1] = 1
    rows.append(one)                                                              # a single called allele
    for code in MISSING_CODES:
        row = np.where(half, 0, 1).astype(np.int16)
        row[[0, n_calls // 2, n_calls - 1]] = code
        rows.append(row)
    return np.array(rows).astype(np.int8)


def mac_boundary_cases(n_calls, min_macs=(1, 2, 3)):
    """For every min_mac m: allele 1 on m - 1, on m and on n_calls - 1 calls among 0s, once at the END of the row and once
    at its start (a count that misses the row's tail changes the flag); allele 1 m - 1 and m times among 2s (a {1, 2}
    site); then a {0, 2} site (kept only at min_mac 1), a {1, 2} site that is nearly all 1 and the same counts with
    missing calls in between.  Sites whose count does not fit n_calls are left out."""
    rows = []
    counts = sorted({c for m in min_macs for c in (m - 1, m)} | {n_calls - 1})
    for c in counts:
        if not 0 <= c <= n_calls:
            continue
        for other in (0, 2):
            tail = np.full(n_calls, other, np.int16)
            tail[n_calls - c:] = 1
            head = np.full(n_calls, other, np.int16)
            head[:c] = 1
            rows += [tail, head]
            if n_calls - c >= 2:
                gap = tail.copy()
                gap[0] = -1 - (c % 2) * 127                                       # -1 or -128
                rows.append(gap)
    z2 = np.zeros(n_calls, np.int16)
    z2[n_calls - 1] = 2
    rows.append(z2)
    return np.array(rows).astype(np.int8)


TAIL_KINDS = ("last_is_1", "first_is_1", "all_0", "random", "last_is_2_among_1", "first_missing")


def tail_cases(n_calls, kinds, rng):
    """Variants that are biallelic only through one call at an end of the row, and some that are not."""
    rows = []
    for kind in kinds:
        row = np.zeros(n_calls, np.int16)
        if kind == "last_is_1":
            row[-1] = 1
        elif kind == "first_is_1":
            row[0] = 1
        elif kind == "random":
            row = rng.integers(0, 2, n_calls).astype(np.int16)
        elif kind == "last_is_2_among_1":
            row[:] = 1
            row[-1] = 2
        elif kind == "first_missing":
            row[-1] = 1
            row[0] = -1
        rows.append(row)
    return np.array(rows).astype(np.int8).reshape(len(kinds), n_calls)


def scan_calls(keep):
    """N = 2, P = 1 calls whose flags at min_mac 1 are `keep`: `0 1` where kept, `0 0` where not."""
    keep = np.asarray(keep, np.uint8)
    gt = np.zeros((len(keep), 2, 1), np.int8)
    gt[:, 1, 0] = keep
    return gt


def scan_patterns(V, rng):
    first, last = np.zeros(V, np.uint8), np.zeros(V, np.uint8)
    first[0], last[-1] = 1, 1
    return {"all": np.ones(V, np.uint8), "none": np.zeros(V, np.uint8), "first": first, "last": last,
            "alternating": (np.arange(V) % 2).astype(np.uint8), "random": (rng.random(V) < 0.5).astype(np.uint8)}


def row_calls(V, N, P, rng):
    """Calls for the rows kernel: allele 1 in about half the calls (0..P copies per sample), 0, 2, -1 and 127 (all of
    which count 0) in the rest."""
    return rng.choice(np.array([1, 1, 1, 1, 0, 2, -1, 127], np.int8), size=(V, N, P))


PATTERNS = ("full", "empty_between", "first", "last", "random", "none")


def tile_pattern(V, name, rng):
    """keep flags [V] by FT-variant tile: every variant; full and empty tiles in turn; only the first / only the last
    variant of every tile (the last tile's last is V - 1); random; nothing."""
    v = np.arange(V)
    if name == "full":
        keep = np.ones(V, bool)
    elif name == "empty_between":
        keep = (v // FT) % 2 == 0
    elif name == "first":
        keep = v % FT == 0
    elif name == "last":
        keep = (v % FT == FT - 1) | (v == V - 1)
    elif name == "random":
        keep = rng.random(V) < 0.5
    elif name == "none":
        keep = np.zeros(V, bool)
    else:
        raise ValueError(name)
    return keep.astype(np.uint8)


def make_order(N, n_out, kind, rng):
    """n_out sample indices < N as int32: "reversed" (N - 1 downwards), "repeated" (random with the first sample again at
    the end) or "subset" (strictly increasing); the samples on both sides of the FS chunk edges are put in where they
    exist and fit."""
    edges = [s for s in (N - 1, FS, FS - 1, 0, 2 * FS, 2 * FS - 1) if 0 <= s < N]
    edges = list(dict.fromkeys(edges))
    if kind == "reversed":
        order = np.arange(N - 1, -1, -1)[:n_out]
    elif kind == "repeated":
        order = rng.integers(0, N, n_out)
        m = min(len(edges), max(n_out - 1, 0))
        order[:m] = edges[:m]
        order[-1] = order[0]
    elif kind == "subset":
        assert n_out <= N
        rest = np.setdiff1d(np.arange(N), edges)
        take = edges[:n_out]
        order = np.sort(np.concatenate([take, rng.choice(rest, n_out - len(take), replace=False)]).astype(np.int64))
    else:
        raise ValueError(kind)
    assert len(order) == n_out
    return np.ascontiguousarray(order, dtype=np.int32)


# ------------------------------------------------------------------ dosages
def special_values():
    """NaN, the infinities, -0.0, both ends of the accepted range, a huge value, a denormal and the rounding ties
    (k + 0.5) / 63 in fp32 for every k: 135 float32 values."""
    ties = (np.arange(127, dtype=np.float64) + 0.5) / UNIT
    return np.concatenate([np.array([np.nan, np.inf, -np.inf, -0.0, -0.001, 2.001, 1e30, 1e-45]), ties]).astype(np.float32)


def dosage_matrix(V, N, rng, specials=True):
    """Dosages in [0, 2] rounded to 4 decimals, 3 % missing; with specials the 135 special_values() are laid over it from a
    random start as often as they fit (all of them when V * N >= 135)."""
    ds = rng.uniform(0, 2, (V, N)).round(4).astype(np.float32)
    ds[rng.random((V, N)) < 0.03] = np.nan
    if specials:
        sp = special_values()
        flat = ds.reshape(-1)
        at = rng.permutation(flat.size)[:len(sp)]
        flat[at] = sp[:len(at)]
    return ds


def q_to_dosage(q):
    """float32 dosages whose dosage_q is the integer matrix q (-1 -> NaN)."""
    q = np.asarray(q, np.int64)
    ds = np.where(q < 0, np.nan, q / float(UNIT)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        back = G.dosage_q(ds).astype(np.int64)
    assert np.array_equal(np.where(back == G.Q_MISSING, -1, back), q)
    return ds


def _spread(total, n, missing=()):
    """q row of n samples whose called samples (all but `missing`) sum to total, filled from the END of the row (a sum that
    misses the tail changes), or None when total does not fit."""
    row = np.zeros(n, np.int64)
    row[list(missing)] = -1
    left = total
    for s in range(n - 1, -1, -1):
        if row[s] < 0:
            continue
        row[s] = min(2 * UNIT, left)
        left -= row[s]
    return row if left == 0 else None


def dosage_boundary_cases(n, min_macs=(1, 2, 5)):
    """q sites (as dosages) on both sides of every bound of the filter: S = 63 m - 1 and 63 m for every min_mac m;
    S = 126 c - 1 and 126 c over c called samples with missing ones in between; S = 0; all missing; a single called sample
    holding 62, 63, 125 and 126.  Sums that do not fit n samples are left out.  -> float32 [sites][n]"""
    gaps = (0, n // 2) if n > 2 else ()
    rows = []
    for m in min_macs:
        rows += [_spread(UNIT * m - 1, n), _spread(UNIT * m, n), _spread(UNIT * m, n, gaps)]
    for missing in ((), gaps):
        c = n - len(missing)
        rows += [_spread(2 * UNIT * c - 1, n, missing), _spread(2 * UNIT * c, n, missing)]
    rows += [np.zeros(n, np.int64), np.full(n, -1, np.int64)]
    for v in (62, 63, 125, 126):
        one = np.full(n, -1, np.int64)
        one[n - 1] = v
        rows.append(one)
    return q_to_dosage(np.array([r for r in rows if r is not None]))


DOSAGE_TAIL_KINDS = ("last_is_1", "first_is_1", "all_0", "random", "all_2_last_1", "all_missing_last_1", "all_2_last_missing")


def dosage_tail_cases(n, kinds, rng):
    """Sites that pass only through the value at one end of the row, and some that do not pass."""
    rows = []
    for kind in kinds:
        row = np.zeros(n, np.float32)
        if kind == "last_is_1":
            row[-1] = 1.0
        elif kind == "first_is_1":
            row[0] = 1.0
        elif kind == "random":
            row = dosage_matrix(1, n, rng, specials=False)[0]
        elif kind == "all_2_last_1":
            row[:] = 2.0
            row[-1] = 1.0
        elif kind == "all_missing_last_1":
            row[:] = np.nan
            row[-1] = 1.0
        elif kind == "all_2_last_missing":
            row[:] = 2.0
            row[-1] = np.nan
        rows.append(row)
    return np.array(rows, np.float32).reshape(len(kinds), n)
