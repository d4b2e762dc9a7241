"""The literal form of the IBD rule, fixtures with planted stretches and the check that a fixture is not vacuous, shared by
tests/test_ibd.py and tests/test_gpu_ibd.py."""
import numpy as np

from locator_amd import ibd as IB
from tests import paint_util as PU

VCF, SAMPLE_DATA = PU.VCF, PU.SAMPLE_DATA
NO_LIMIT = IB.NO_LIMIT
# gap_sites 0, 1, 2 x extend_sites 1, 3, then two sets whose length thresholds cut some chains (the fixtures' sites are 1 .. 20
# apart, so a seed of 12 sites spans about 115, a gap of one site about 21)
PARAMS = tuple(IB.Params(12, 0, e, g, NO_LIMIT, 0) for g in (0, 1, 2) for e in (1, 3)) + (
    IB.Params(12, 110, 3, 1, 20, 0), IB.Params(10, 0, 2, 2, NO_LIMIT, 120))


# ------------------------------------------------------------------ the rule, word for word
def pair_literal(hp, hq, first, x, P):
    """The segments [(a, b)] of two columns: a loop over the sites that follows the words of the rule."""
    K = len(hp)
    agrees = [bool(hp[j] < 0 or hq[j] < 0 or hp[j] == hq[j]) for j in range(K)]
    runs, j = [], 0
    while j < K:
        if not agrees[j]:
            j += 1
            continue
        a = j
        while j + 1 < K and agrees[j + 1] and not first[j + 1]:
            j += 1
        runs.append((a, j))
        j += 1

    def sites(r):
        return r[1] - r[0] + 1

    def linked(r1, r2):
        g = r2[0] - r1[1] - 1
        return (sites(r1) >= P.extend_sites and sites(r2) >= P.extend_sites and 1 <= g <= P.gap_sites
                and not any(first[s] for s in range(r1[1] + 1, r2[0] + 1)) and int(x[r2[0]]) - int(x[r1[1]]) <= P.gap_len)

    chains = []
    for r in runs:
        if chains and linked(chains[-1][-1], r):
            chains[-1].append(r)
        else:
            chains.append([r])
    out = []
    for chain in chains:
        a, b = chain[0][0], chain[-1][1]
        seeded = any(sites(r) >= P.seed_sites and int(x[r[1]]) - int(x[r[0]]) >= P.seed_len for r in chain)
        if seeded and int(x[b]) - int(x[a]) >= P.min_len:
            out.append((a, b))
    return out


def segments_literal(h, owner, first, x, params, rows=None):
    """segments_host's answer by pair_literal: tiny shapes only."""
    P = IB.check_params(params)
    H, K = len(owner), h.shape[0]
    first = np.array(first, dtype=bool)
    if K:
        first[0] = True
    rows = range(H) if rows is None else rows
    count, length, longest = np.zeros((len(rows), H), dtype=np.int32), np.zeros((len(rows), H), dtype=np.int64), np.zeros((len(rows), H), dtype=np.int64)
    sa, sb = [], []
    for i, p in enumerate(rows):
        for q in range(p + 1, H):
            if owner[q] == owner[p]:
                continue
            for a, b in pair_literal(h[:, p], h[:, q], first, x, P):
                ln = int(x[b]) - int(x[a])
                count[i, q] += 1
                length[i, q] += ln
                longest[i, q] = max(longest[i, q], ln)
                sa.append(a)
                sb.append(b)
    return count, length, longest, np.array(sa, dtype=np.int32), np.array(sb, dtype=np.int32)


# ------------------------------------------------------------------ fixtures
def owners(H):
    """Two columns an individual; an odd H leaves the last column an individual of its own."""
    return np.repeat(np.arange((H + 1) // 2, dtype=np.int32), 2)[:H].copy()


def fixture(H, K, seed, P, first_sites=(34,)):
    """{h, owner, first, x}: random haplotypes (an allele a coin, sites 1 .. 20 apart) with 3 % missing alleles, a site and (from
    six columns on) a column entirely missing, and stretches copied between columns of different owners, as far as K holds them:
      columns 0 -> 2: a stretch from site 0; one cut by the first site 34 in its middle; two runs one discordant site apart at
              bit 0 of a word (site 64); a stretch across the word boundary 127 | 128; two more runs one discordant site apart from
              site 220; a stretch that ends at site K - 1;
      columns 0 -> 3: two runs one site short of seed_sites each, one discordant site apart: a chain without a seed;
      columns 1 -> 3: two runs with exactly one discordant site between them at bit 63 of a word (site 63); two runs
              gap_sites + 1 discordant sites apart, which must not link.
    The copied-from columns hold no missing allele and are written once, so that no stretch undoes another.
    first_sites: the chromosome starts besides site 0."""
    rng = np.random.default_rng(seed)
    owner = owners(H)
    h = rng.integers(0, 2, (K, H)).astype(np.int8)
    h[rng.random((K, H)) < 0.03] = -1
    h[:, :2] = np.abs(h[:, :2])
    x = np.cumsum(rng.integers(1, 21, K)).astype(np.int64)
    first = np.zeros(K, dtype=bool)
    first[[s for s in (0,) + tuple(first_sites) if s < K]] = True
    sd, gap = P.seed_sites, P.gap_sites

    def differ(p, q, j):
        if 0 <= j < K and q < H:
            h[j, q] = 1 - h[j, p]

    def plant(p, q, a, b):
        if q < H and 0 <= a <= b < K:
            h[a:b + 1, q] = h[a:b + 1, p]
            differ(p, q, a - 1)
            differ(p, q, b + 1)

    plant(0, 2, 0, sd + 1)
    plant(0, 2, 20, 47)
    plant(0, 2, 64 - sd, 63)
    plant(0, 2, 65, 64 + sd)
    plant(0, 2, 120, 135)
    plant(0, 2, 220, 219 + sd)
    plant(0, 2, 221 + sd, 220 + 2 * sd)
    plant(0, 2, K - sd - 2, K - 1)
    plant(0, 3, 10, 8 + sd)
    plant(0, 3, 10 + sd, 8 + 2 * sd)
    plant(1, 3, 63 - sd, 62)
    plant(1, 3, 64, 63 + sd)
    plant(1, 3, 88, 87 + sd)
    plant(1, 3, 89 + sd + gap, 88 + 2 * sd + gap)
    for j in range(88 + sd, 89 + sd + gap):
        differ(1, 3, j)
    if K > 40:
        h[40, :] = -1
    elif K:
        h[K // 2, :] = -1
    if H >= 6:
        h[:, H - 1] = -1
    return {"h": h, "owner": owner, "first": first, "x": x}


def host(fx, P, rows=None, segments=True):
    return IB.segments_host(fx["h"], fx["owner"], fx["first"], fx["x"], P, rows, segments)


def assert_not_vacuous(fx, P, answer=None):
    """By segments_host: the fixture has a segment, a pair with two segments at least, a pair whose chains pass every threshold
    but hold no seed and that reports nothing and, where runs may link at all, a segment that is a chain of two runs or more.
    A comparison of two empty answers can then pass for nothing."""
    count, length, longest, sa, sb = host(fx, P) if answer is None else answer
    assert count.sum() > 0 and len(sa) == count.sum(), "no segment"
    assert count.max() >= 2, "no pair with two segments"
    loose = host(fx, P._replace(seed_sites=P.extend_sites, seed_len=0), segments=False)[0]
    assert ((count == 0) & (loose > 0)).any(), "no pair whose seed-less chain reports nothing"
    if P.gap_sites >= 1:
        h, H = fx["h"], len(fx["owner"])
        pair = np.repeat(np.arange(count.size), count.reshape(-1))
        joined = 0
        for at, a, b in zip(pair, sa, sb):
            p, q = h[a:b + 1, at // H], h[a:b + 1, at % H]
            joined += bool(((p >= 0) & (q >= 0) & (p != q)).any())
        assert joined, "no chain of two runs or more"


def same(got, want):
    return all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip(got, want))
