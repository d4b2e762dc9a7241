#!/usr/bin/env python3
"""`python -m locator_amd.ibd`: identity-by-descent (IBD) segments between phased haplotypes (GERMLINE, Gusev et al. 2009;
hap-IBD, Zhou et al. 2020; Ralph & Coop 2013) and a placement baseline from them.  A segment is a long stretch over which two
haplotypes of different individuals are identical, a few discordant sites apart at most; the total shared length of two samples
carries their recent common ancestry.  With --sample_data a sample is placed at the length-weighted mean location of the located
samples it shares most with.

  python -m locator_amd.ibd --vcf phased.vcf.gz --out out/test [--sample_data samples.txt]

  haplotypes  h [K][pitch] int8, site-major, the paint command's matrix: h[j][d] = allele of haplotype column d at site j, 0 or
              1, negative = missing; column 2 s + a is allele a of sample s.  owner [H] the individual of a column, first [K]
              the first sites of the chromosomes (first[0] counts as set), x [K] int64 the coordinate of a site: its base-pair
              position, the site index with --uniform or without positions; non-decreasing inside a chromosome.
  parameters  Params(seed_sites >= 1, seed_len >= 0, extend_sites 1 .. seed_sites, gap_sites 0 .. LOC_IBD_MAX_GAP, gap_len >= 0,
              min_len >= 0), whole numbers; every comparison is exact in int64.
  the rule    for columns p < q of different owners.  Site j agrees when either allele is missing or the two are equal.  A run
              [a, b] is a maximal interval of agreeing sites inside one chromosome (a first site starts a new run); it has
              b - a + 1 sites and length x[b] - x[a].  Consecutive runs [a1, b1], [a2, b2] are linked when both have
              extend_sites sites at least, 1 <= a2 - b1 - 1 <= gap_sites, no site of b1 + 1 .. a2 is a first site and
              x[a2] - x[b1] <= gap_len.  A chain is a maximal sequence of runs whose neighbours are linked; a chain from a to b
              is the segment (a, b) when it holds a seed, a run of seed_sites sites at least and length >= seed_len, and
              x[b] - x[a] >= min_len.  gap_sites = 0: the exact maximal identical runs that pass the thresholds.
  answers     `segments_host(h, owner, first, x, params, rows)` -> (count int32 [R][H], length int64 [R][H], longest int64
              [R][H], seg_a int32 [T], seg_b int32 [T]): row i is column rows[0] + i, the entries with q <= p or the same owner
              are zeros, length the sum and longest the largest of a pair's segment lengths; the segments pair-major in (p, q)
              order, ascending inside a pair, a pair's offset the exclusive prefix sum of count in row-major order.
              `pack_host(h, H, K)` -> uint64 [2][ceil(K / 64)][wpitch]: bit j % 64 of word [j / 64][d] of plane 0 set where
              h[j][d] > 0, of plane 1 where h[j][d] >= 0; what the device scans.
  samples     S[s][t] = the sum of `length` over the four haplotype pairs of two samples, C likewise of `count`, L the largest
              `longest`; symmetric, zero diagonals.
  placement   candidates are the located samples, the weight is S: for k = 1 .. --kmax the S-weighted mean location of the k
              candidates with the largest S[s][t] (ties to the lower index; nobody shares with themself, so it is leave-one-out
              by construction; a sample that shares nothing is NaN); --k auto takes the k with the smallest leave-one-out
              median error, as the paint and neighbors commands do.

Outputs: {out}_ibd_pairs.txt (sampleID1 sampleID2 segments length longest: the sample pairs that share), {out}_ibd_summary.json,
with --sample_data {out}_ibd_locs.txt (x,y,sampleID), with --keep_segments {out}_ibd_segments.txt (sampleID1 hap1 sampleID2 hap2
chrom start end sites length; start and end are positions, site indices without positions; it can run to millions of lines),
with --keep_matrix {out}_ibd.npz (S, C, L, samples).  Without a GPU the run stops and says so; --host asks for the NumPy form.
The device (loc_ibd_pack, loc_ibd_scan, loc_ibd_fill: include/locator_hip_ibd.h) computes in integers what segments_host
computes: the files of the two paths are byte-identical, but for the summary's `path` entry, which names the path.  --budget_gb
bounds the per-pair answers of one batch of rows on the device (20 bytes a pair, 36 with --keep_segments; the bit planes, K H / 4
bytes, and a batch's segments, 8 bytes each, come on top; batching changes no bit).  The NumPy form holds the agreement of one
row with every column as [columns][K] booleans and a few copies of them, about 6 K H bytes a row (20 GB at 32,768 columns x
100,000 sites): --host is meant for checking and for small inputs.

Not built: genetic maps (lengths in cM), genotype-error-tolerant seeds beyond the gap rule, within-individual segments (runs of
homozygosity), unphased input.
"""
from __future__ import annotations

import json
import sys
from typing import NamedTuple

import numpy as np

from . import _abi
from . import baselines as B
from ._files import write_atomic

MAX_HAPS = _abi.LOC_IBD_MAX_HAPS
MAX_GAP = _abi.LOC_IBD_MAX_GAP
NO_LIMIT = 1 << 62                   # --gap_length without a limit: no difference of two int64 coordinates the command reads reaches it
PROG = "locator_amd.ibd"
LAUNCH = "the scans are loc_ibd_scan launches"
NOTHING_TO_CHOOSE_BY = "no located sample shares a segment with another located sample: nothing to choose k by"
HEAD = ("N", "n_located", "K", "P", "error_unit", "r2_x", "r2_y", "mean_error", "median_error")
OWN = ("H", "seed_sites", "seed_length", "extend_sites", "gap_sites", "gap_length", "min_length", "uniform", "segments",
       "pairs_sharing", "mean_length", "median_length")
PLACED = ("kmax", "k", "k_auto", "k_chosen_by", "median_error_by_k")
BATCH_BYTES = 1 << 28                # the [rows][H] answers one batch of rows of the host form may hold
PAIR_BYTES = 20                      # count, length and longest of a pair
PAIR_BYTES_SEGMENTS = 36             # ... and, where segments are wanted, the running sum of count and the offsets


class Params(NamedTuple):
    seed_sites: int
    seed_len: int
    extend_sites: int
    gap_sites: int
    gap_len: int
    min_len: int


# ---------------------------------------------------------------- the definition

def check_params(params):
    """params as a Params of Python ints, after the refusal of a value outside the ranges of the module text."""
    raw = tuple(params)
    if len(raw) != 6 or any(int(v) != v for v in raw):
        raise ValueError(f"parameters {raw}: need six whole numbers (seed_sites, seed_len, extend_sites, gap_sites, gap_len, min_len)")
    P = Params(*(int(v) for v in raw))
    if P.seed_sites < 1 or not 1 <= P.extend_sites <= P.seed_sites:
        raise ValueError(f"seed_sites = {P.seed_sites}, extend_sites = {P.extend_sites}: seed_sites must be >= 1 and extend_sites 1 .. seed_sites")
    if not 0 <= P.gap_sites <= MAX_GAP:
        raise ValueError(f"gap_sites = {P.gap_sites}: must be 0 .. {MAX_GAP}")
    if min(P.seed_len, P.gap_len, P.min_len) < 0 or max(P) >= 1 << 63:
        raise ValueError(f"seed_len = {P.seed_len}, gap_len = {P.gap_len}, min_len = {P.min_len}: no length may be negative")
    return P


def _check(h, owner, first, x, params, rows):
    h = np.asarray(h)
    if h.ndim != 2 or h.dtype != np.int8:
        raise ValueError(f"haplotypes of shape {h.shape} and type {h.dtype}: need int8 [sites][columns]")
    owner = np.ascontiguousarray(owner, dtype=np.int32)
    K, H = h.shape[0], len(owner)
    if not 1 <= H <= MAX_HAPS:
        raise ValueError(f"{H} haplotype columns: must be 1 .. {MAX_HAPS}")
    if h.shape[1] < H or K >= 2 ** 31:
        raise ValueError(f"{H} owners for rows of {h.shape[1]} columns, {K} sites: needs a column an owner and fewer than 2^31 sites")
    first = np.asarray(first).astype(bool).copy()
    x = np.ascontiguousarray(x, dtype=np.int64)
    if first.shape != (K,) or x.shape != (K,):
        raise ValueError(f"{first.shape} chromosome starts and {x.shape} coordinates for {K} sites")
    if K:
        first[0] = True
        if (np.diff(x) < 0)[~first[1:]].any():
            raise ValueError("the coordinates of a chromosome are not in ascending order")
    P = check_params(params)
    if rows is None:
        p0, R = 0, H
    else:
        rows = np.asarray(rows, dtype=np.int64)
        p0, R = (int(rows[0]) if len(rows) else 0), len(rows)
        if R and not np.array_equal(rows, np.arange(p0, p0 + R)) or p0 < 0 or p0 + R > H:
            raise ValueError(f"rows must be consecutive columns of 0 .. {H - 1}")
    return h, owner, first, x, P, p0, R


def _row_host(h, H, owner, first, x, P, p):
    """The answers of row p against all columns: (q of every segment ascending, its a, its b, its length)."""
    K = h.shape[0]
    cols = np.flatnonzero((np.arange(H) > p) & (owner != owner[p]))
    if not len(cols) or not K:
        return (np.zeros(0, dtype=np.int64),) * 4
    mine, theirs = h[:, p:p + 1], h[:, cols]
    agree = ((mine < 0) | (theirs < 0) | (mine == theirs)).T                      # [columns][K]
    blank = np.zeros((len(cols), 1), dtype=bool)
    begins = agree & (first[None, :] | ~np.concatenate([blank, agree[:, :-1]], axis=1))
    ends = agree & (np.append(first[1:], True)[None, :] | ~np.concatenate([agree[:, 1:], blank], axis=1))
    c, a = np.nonzero(begins)                                                     # the runs, column-major, ascending inside a column
    b = np.nonzero(ends)[1]
    if not len(a):
        return (np.zeros(0, dtype=np.int64),) * 4
    n, ln = b - a + 1, x[b] - x[a]
    starts = np.cumsum(first)                                                     # chromosome starts in 0 .. j
    linked = ((c[1:] == c[:-1]) & (n[:-1] >= P.extend_sites) & (n[1:] >= P.extend_sites) & (a[1:] - b[:-1] - 1 >= 1)
              & (a[1:] - b[:-1] - 1 <= P.gap_sites) & (starts[a[1:]] == starts[b[:-1]]) & (x[a[1:]] - x[b[:-1]] <= P.gap_len))
    head = np.flatnonzero(np.concatenate([[True], ~linked]))                      # the first run of every chain
    last = np.append(head[1:], len(a)) - 1
    seeded = np.logical_or.reduceat((n >= P.seed_sites) & (ln >= P.seed_len), head)
    ca, cb = a[head], b[last]
    keep = seeded & (x[cb] - x[ca] >= P.min_len)
    return cols[c[head][keep]], ca[keep], cb[keep], (x[cb] - x[ca])[keep]


def segments_host(h, owner, first, x, params, rows=None, segments=True):
    """(count int32 [R][H], length int64 [R][H], longest int64 [R][H], seg_a int32 [T], seg_b int32 [T]): the definition in the
    module text, a row at a time, all of a row's runs at once.  segments False: seg_a and seg_b are None."""
    h, owner, first, x, P, p0, R = _check(h, owner, first, x, params, rows)
    H = len(owner)
    count, length, longest = np.zeros((R, H), dtype=np.int32), np.zeros((R, H), dtype=np.int64), np.zeros((R, H), dtype=np.int64)
    sa, sb = [], []
    for i in range(R):
        q, a, b, ln = _row_host(h, H, owner, first, x, P, p0 + i)
        np.add.at(count[i], q, 1)
        np.add.at(length[i], q, ln)
        np.maximum.at(longest[i], q, ln)
        sa.append(a)
        sb.append(b)
    if not segments:
        return count, length, longest, None, None
    cat = lambda v: np.concatenate(v).astype(np.int32) if v else np.zeros(0, dtype=np.int32)
    return count, length, longest, cat(sa), cat(sb)


def pack_host(h, H, K, wpitch=None):
    """bits uint64 [2][W][wpitch], W = ceil(K / 64), wpitch the next multiple of 8 from H unless given: the two bit planes of the
    module text; the bits of sites >= K and the words of columns >= H are zero."""
    h = np.asarray(h)
    wpitch = (H + 7) // 8 * 8 if wpitch is None else int(wpitch)
    if wpitch < H or wpitch % 8:
        raise ValueError(f"wpitch = {wpitch}: must be a multiple of 8 and >= H = {H}")
    W = (K + 63) // 64
    bits = np.zeros((2, W, wpitch), dtype=np.uint64)
    if K:
        sites = np.full((W * 64, H), -1, dtype=np.int8)
        sites[:K] = h[:K, :H]
        for plane, flags in enumerate((sites > 0, sites >= 0)):
            octets = np.packbits(flags.reshape(W, 64, H), axis=1, bitorder="little")         # [W][8][H], byte b = sites 8 b .. 8 b + 7
            bits[plane, :, :H] = np.ascontiguousarray(octets.transpose(0, 2, 1)).view("<u8")[:, :, 0]
    return bits


def pack_first(first, K):
    """first_bits uint64 [max(W, 1)]: bit j % 64 of word j / 64 set where site j starts a chromosome."""
    W = (K + 63) // 64
    flags = np.zeros(max(W, 1) * 64, dtype=bool)
    flags[:K] = np.asarray(first, dtype=bool)[:K]
    return np.packbits(flags.reshape(-1, 64), axis=1, bitorder="little").view("<u8")[:, 0].copy()


# ---------------------------------------------------------------- the device form

def _device_batches(h, owner, first, x, P, p0, R, segments, budget, pitch, wpitch, pad_fill, fill, device):
    """(first row, count, length, longest, seg_a, seg_b) of one batch of rows after the other: one loc_ibd_pack launch, then a
    loc_ibd_scan launch a batch and, where segments are wanted, the prefix sum of its count and a loc_ibd_fill launch."""
    import torch as t
    from . import _device as D, _lib
    lib = _lib.load()
    K, H = h.shape[0], len(owner)
    buf = B.padded(np.ascontiguousarray(h[:, :H]), pitch, pad_fill)
    wp = (H + 7) // 8 * 8 if wpitch is None else int(wpitch)
    W = (K + 63) // 64

    def fresh(shape, dtype):
        v = t.empty(shape, dtype=dtype, device=device)
        if v.numel():
            D.prefill((v,), fill)
        return v

    with t.cuda.device(device):
        stream = D.stream
        d_h = D.put(buf, np.int8, device)
        d_bits = fresh((2, max(W, 1), max(wp, 8)), t.int64)
        _lib.check(lib.loc_ibd_pack(d_h.data_ptr(), H, K, int(buf.shape[1]), d_bits.data_ptr(), wp, stream()), "loc_ibd_pack")
        del d_h
        d_owner = D.put(owner, np.int32, device)
        d_first = D.put(pack_first(first, K).view(np.int64), np.int64, device)
        d_x = D.put(x if K else np.zeros(1, dtype=np.int64), np.int64, device)
        step = max(1, int(budget) // ((PAIR_BYTES_SEGMENTS if segments else PAIR_BYTES) * H))
        for a in range(p0, p0 + R, step):
            n = min(step, p0 + R - a)
            d_count, d_length, d_longest = fresh((n, H), t.int32), fresh((n, H), t.int64), fresh((n, H), t.int64)
            args = (d_bits.data_ptr(), wp, H, K, d_owner.data_ptr(), d_first.data_ptr(), d_x.data_ptr(), a, n, *P)
            _lib.check(lib.loc_ibd_scan(*args, d_count.data_ptr(), d_length.data_ptr(), d_longest.data_ptr(), stream()), "loc_ibd_scan")
            seg_a = seg_b = None
            if segments:
                flat = d_count.view(-1)
                ends = t.cumsum(flat, dim=0, dtype=t.int64)
                total = int(ends[-1])
                d_offsets = (ends - flat).contiguous()
                d_a, d_b = fresh(max(total, 1), t.int32), fresh(max(total, 1), t.int32)
                _lib.check(lib.loc_ibd_fill(*args, d_offsets.data_ptr(), total, d_a.data_ptr(), d_b.data_ptr(), stream()), "loc_ibd_fill")
                seg_a, seg_b = d_a[:total].cpu().numpy(), d_b[:total].cpu().numpy()
            yield a, d_count.cpu().numpy(), d_length.cpu().numpy(), d_longest.cpu().numpy(), seg_a, seg_b


def _host_batches(h, owner, first, x, P, p0, R, segments):
    step = max(1, BATCH_BYTES // (PAIR_BYTES * len(owner)))
    for a in range(p0, p0 + R, step):
        yield (a,) + segments_host(h, owner, first, x, P, range(a, min(a + step, p0 + R)), segments)


def segments_device(h, owner, first, x, params, rows=None, segments=True, budget=4 << 30, pitch=None, wpitch=None, pad_fill=-1,
                    fill=None, device="cuda:0"):
    """segments_host's answer from the device: the planes packed once, the rows in batches whose answers stay within `budget`
    bytes, loc_ibd_fill only where segments are wanted.  fill: a 32-bit pattern that the planes and every output hold before a
    launch; pitch, wpitch, pad_fill: the row pitches and the pad bytes of the haplotype matrix (tests)."""
    h, owner, first, x, P, p0, R = _check(h, owner, first, x, params, rows)
    H = len(owner)
    parts = list(_device_batches(h, owner, first, x, P, p0, R, segments, budget, pitch, wpitch, pad_fill, fill, device))
    cat = lambda i, dtype, shape: np.concatenate([p[i] for p in parts]) if parts else np.zeros(shape, dtype=dtype)
    answer = (cat(1, np.int32, (0, H)), cat(2, np.int64, (0, H)), cat(3, np.int64, (0, H)))
    return answer + ((cat(4, np.int32, 0), cat(5, np.int32, 0)) if segments else (None, None))


# ---------------------------------------------------------------- the driver's pieces

def fold_samples(count, length, longest, p0, S, C, L):
    """Adds the rows p0 .. of a batch to the upper triangles of S, C (sums) and L (largest) [N][N]: column 2 s + a is sample s."""
    R, H = count.shape
    N = H // 2
    s = (p0 + np.arange(R)) // 2
    np.add.at(S, s, length.reshape(R, N, 2).sum(axis=2))
    np.add.at(C, s, count.reshape(R, N, 2).sum(axis=2, dtype=np.int64))
    np.maximum.at(L, s, longest.reshape(R, N, 2).max(axis=2))


def sample_sharing(batches, N, keep_segments=False):
    """(S, C, L int64 [N][N], symmetric; the segments as (p, q, a, b) int arrays, or None): `batches` folded to samples."""
    S, C, L = (np.zeros((N, N), dtype=np.int64) for _ in range(3))
    segs = []
    for p0, count, length, longest, seg_a, seg_b in batches:
        fold_samples(count, length, longest, p0, S, C, L)
        if keep_segments:
            pair = np.repeat(np.arange(count.size, dtype=np.int64), count.reshape(-1))
            segs.append((p0 + pair // count.shape[1], pair % count.shape[1], seg_a.astype(np.int64), seg_b.astype(np.int64)))
    segs = tuple(np.concatenate([s[i] for s in segs]) if segs else np.zeros(0, dtype=np.int64) for i in range(4)) if keep_segments else None
    return S + S.T, C + C.T, np.maximum(L, L.T), segs


# ---------------------------------------------------------------- the command's work

def ibd(hap, c, P, samples, locs, chrom=None, pos=None, out=None, params=Params(64, 0, 16, 1, NO_LIMIT, 0), uniform=False, k="auto",
        kmax=16, longlat=False, keep_segments=False, keep_matrix=False, host=False, silence=False, device="cuda:0", budget=4 << 30):
    """The command's work for a site-major haplotype matrix hap [K][2N] (c: the count matrix of the same sites, for the shared
    summary entries): returns the summary dict and writes the output files when `out` is given.  locs None: no locations."""
    from .paint import site_gaps
    hap = np.ascontiguousarray(hap, dtype=np.int8)
    K, H = hap.shape
    N = H // 2
    samples = np.asarray(samples).astype(str)
    if H != 2 * N or len(samples) != N or N < 2:
        raise SystemExit(f"{PROG}: {H} haplotype columns for {len(samples)} samples: needs two a sample and two samples at least")
    if H > MAX_HAPS:
        raise SystemExit(f"{PROG}: {H} haplotype columns: at most {MAX_HAPS}")
    if K == 0:
        raise SystemExit(f"{PROG}: no site is left after the filters: nothing to compare")
    try:
        par = check_params(params)
    except ValueError as e:
        raise SystemExit(f"{PROG}: {e} (--seed_sites, --extend_sites, --gap_sites, --seed_length, --gap_length, --min_length)") from None
    if k != "auto" and not 1 <= int(k) <= kmax or not 1 <= kmax <= B.KMAX_LIMIT:
        raise SystemExit(f"{PROG}: --kmax must be 1 .. {B.KMAX_LIMIT} and --k `auto` or 1 .. --kmax")
    located = None
    if locs is not None:
        locs, located = B.located_mask(locs, N, PROG)
    if not host:
        B.require_gpu(PROG, LAUNCH)
    _, first = site_gaps(chrom, pos, K, uniform)                    # refuses positions that descend inside a chromosome
    flat = uniform or pos is None
    x = np.arange(K, dtype=np.int64) if flat else np.asarray(pos, dtype=np.int64)
    owner = np.repeat(np.arange(N, dtype=np.int32), 2)
    checked = _check(hap, owner, first, x, par, None)
    batches = (_host_batches(*checked, keep_segments) if host else
               _device_batches(*checked, keep_segments, budget, None, None, -1, None, device))
    S, C, L, segs = sample_sharing(batches, N, keep_segments)

    upper = np.triu(C > 0, 1)
    shared = S[upper]
    own = {"H": int(H), "seed_sites": par.seed_sites, "seed_length": par.seed_len, "extend_sites": par.extend_sites,
           "gap_sites": par.gap_sites, "gap_length": None if par.gap_len >= NO_LIMIT else par.gap_len, "min_length": par.min_len,
           "uniform": bool(flat), "segments": int(C[upper].sum()), "pairs_sharing": int(upper.sum()),
           "mean_length": B.num(shared.mean()) if len(shared) else None, "median_length": B.num(np.median(shared)) if len(shared) else None}
    xy, head, placed_own, lines = None, {}, {}, []
    if located is not None:
        xy, head, placed_own, lines, _, _ = B.place_by_weight(PROG, S.astype(np.float64), located, kmax, k, c, P, locs, located, longlat,
                                                              "IBD", NOTHING_TO_CHOOSE_BY)
    summary = B.assemble_summary(head or {"N": int(N), "K": int(K), "P": int(P)}, own, placed_own, HEAD, OWN, PLACED, host)
    lines = [f"{N} samples, {K} sites: {own['segments']} segments between {H} haplotypes, {own['pairs_sharing']} sample pairs share, "
             f"median shared length {own['median_length']!r}", *lines]
    if out is not None:
        s_idx, t_idx = np.nonzero(upper)
        write_atomic(out + "_ibd_pairs.txt", "sampleID1\tsampleID2\tsegments\tlength\tlongest\n" + "".join(
            f"{samples[s]}\t{samples[t]}\t{C[s, t]}\t{S[s, t]}\t{L[s, t]}\n" for s, t in zip(s_idx, t_idx)))
        write_atomic(out + "_ibd_summary.json", json.dumps(summary, indent=1) + "\n")
        if xy is not None:
            B.write_locs(out + "_ibd_locs.txt", xy, samples)
        if keep_segments:
            where = np.arange(K, dtype=np.int64) if pos is None else np.asarray(pos, dtype=np.int64)
            names = np.full(K, ".", dtype=object) if chrom is None else np.asarray(chrom).astype(str)

            def rows(fh):
                fh.write("sampleID1\thap1\tsampleID2\thap2\tchrom\tstart\tend\tsites\tlength\n")
                for p, q, a, b in zip(*segs):
                    fh.write(f"{samples[p // 2]}\t{p % 2}\t{samples[q // 2]}\t{q % 2}\t{names[a]}\t{where[a]}\t{where[b]}\t{b - a + 1}\t"
                             f"{x[b] - x[a]}\n")
            write_atomic(out + "_ibd_segments.txt", rows)
        if keep_matrix:
            write_atomic(out + "_ibd.npz", lambda fh: B.save_npz(fh, S=S, C=C, L=L, samples=samples), mode="wb")
    if not silence:
        for line in lines:
            print(line)
    summary["_S"], summary["_C"], summary["_L"], summary["_xy"], summary["_segments"] = S, C, L, xy, segs
    return summary


# ---------------------------------------------------------------- command

def _own_arguments(p):
    p.add_argument("--seed_sites", default=64, type=int, help="sites of agreement a segment must hold in one run (default 64)")
    p.add_argument("--seed_length", default=0, type=int, help="length such a run must span, base pairs (sites with --uniform; default 0)")
    p.add_argument("--extend_sites", default=16, type=int, help="sites a run needs to be joined to its neighbour, 1 .. --seed_sites (default 16)")
    p.add_argument("--gap_sites", default=1, type=int, help=f"discordant sites between two joined runs at most, 0 .. {MAX_GAP} (default 1; "
                                                            "0: exact identical runs)")
    p.add_argument("--gap_length", default=None, type=int, help="length between two joined runs at most (default: no limit)")
    p.add_argument("--min_length", default=0, type=int, help="length a segment must span (default 0)")
    p.add_argument("--uniform", default=False, action="store_true", help="lengths in sites: the coordinate of a site is its index")
    B.add_k_arguments(p, 16, "sharing samples")
    p.add_argument("--longlat", default=False, action="store_true",
                   help="x / y are longitude / latitude degrees: errors are great-circle km (the mean stays planar)")
    p.add_argument("--keep_segments", default=False, action="store_true", help="write every segment to {out}_ibd_segments.txt")
    p.add_argument("--keep_matrix", default=False, action="store_true",
                   help="keep the sample-level shared lengths, segment counts, longest segments and the sample IDs in {out}_ibd.npz")
    p.add_argument("--budget_gb", default=4.0, type=float, help="per-pair answers of a batch of rows on the device at most, GiB (default 4); the bit planes and "
                                                                    "the segments of a batch come on top")
    p.add_argument("--host", default=False, action="store_true", help="the NumPy form instead of the GPU (the same files)")


def build_parser():
    return B.build_parser(PROG, "Identity-by-descent segments between phased haplotypes and a placement baseline.", _own_arguments,
                          sample_data=False, prune=False, sample_data_help="tab-separated sampleID, x, y; NaN / NA = to be placed.  "
                          "Optional: with it every sample is placed from the located samples it shares most with")


def main(argv=None):
    parser = build_parser()
    a = B.parse_args(parser, argv)
    B.check_k(parser, a)
    B.check_budget(parser, a)
    hap, c, P, samples, locs, chrom, pos = B.haplotype_prelude(parser, a, LAUNCH, "segments are sought between the two haplotypes a sample "
                                                               "of ploidy 2 has")
    try:
        params = Params(a.seed_sites, a.seed_length, a.extend_sites, a.gap_sites, NO_LIMIT if a.gap_length is None else a.gap_length,
                        a.min_length)
        ibd(hap, c, P, samples, locs, chrom, pos, a.out, params, a.uniform, a.k, a.kmax, a.longlat,
            a.keep_segments, a.keep_matrix, a.host, a.silence, budget=int(a.budget_gb * (1 << 30)))
    except ValueError as e:
        raise SystemExit(f"{PROG}: {e}") from None
    return 0


if __name__ == "__main__":
    sys.exit(main())
