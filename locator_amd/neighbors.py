#!/usr/bin/env python3
"""`python -m locator_amd.neighbors`: is there geographic signal in these genotypes at all, and does the network beat the
obvious baseline?  Pairwise identity-by-state (IBS) distances of all samples over the sites a fit would train on, each
sample's genetically nearest located samples, and a k-nearest-neighbour placement to set next to locator's validation error.

  python -m locator_amd.neighbors --vcf genotypes.vcf.gz --sample_data samples.txt --out out/test --close 0

  counts      c[s][v] = copies of allele 1 of sample s at site v (genotypes.to_allele_counts_1, the count a fit trains on),
              -1 where any allele of the call is missing; the sites are those of genotypes.filter_snps with the same
              --min_mac / --max_SNPs / --seed.  P = the ploidy of the calls (1 or 2).
  pairs       over the sites where both samples are called: n[i][j] = their number, d[i][j] = sum |c_i - c_j|, exact int32;
              D = float64(d) / float64(P n), one division (PLINK's 1 - IBS), NaN where n = 0.  `pairs_host` below is the
              definition, loc_ibs_pairs (include/locator_hip_neighbors.h) the same integers from the int8 matrix pipe.
  neighbours  of row i: the located samples j != i with n[i][j] > 0 by ascending D, equal doubles to the lower j
              (`knn_host`; loc_ibs_knn gives the same rows).
  placement   the arithmetic mean of x and of y (planar, float64, summed in rank order) over the first k neighbours: located
              samples leave-one-out, the others from all located samples.  --k auto takes the k in 1 .. --kmax with the
              smallest leave-one-out median error (the smallest such k).

Outputs: {out}_knn_locs.txt (x,y,sampleID as a predlocs file, but NOT named predlocs: it is no replicate),
{out}_neighbors.txt, {out}_knn_summary.json, with --close T {out}_close_pairs.txt, with --keep_matrix {out}_ibs.npz.
--ld_prune R2 (with --ld_window / --ld_window_bp) prunes the sites by linkage disequilibrium first, as locator_amd.ld does; the
summary then also holds ld_prune, ld_window, ld_window_bp and K_before_prune.  There
is no silent fallback: without a GPU the run stops and says so; --host asks for the NumPy form, which writes the same bytes.
"""
from __future__ import annotations

import json
import sys

import numpy as np

from . import _abi
from . import baselines as B
from ._files import write_atomic

TILE = _abi.LOC_IBS_TILE
BLOCK = _abi.LOC_IBS_BLOCK
PROG = "locator_amd.neighbors"
LAUNCH = "the pair statistics are one loc_ibs_pairs launch"
NOTHING_TO_CHOOSE_BY = "no located sample has a located neighbour: nothing to choose k by"
# the key order of {out}_knn_summary.json (with --close: close, n_close_pairs behind them)
SUMMARY_KEYS = ("N", "n_located", "K", "P", "kmax", "k", "k_auto", "k_chosen_by", "error_unit", "median_error_by_k", "r2_x", "r2_y",
                "mean_error", "median_error", "pearson_r_ibs_geo", "n_located_pairs", "n_pairs_no_shared_site")


# ---------------------------------------------------------------- pair statistics

def pairs_host(c, chunk=1 << 24):
    """(d, n) int32 [N][N] of a count matrix c [N][K] with values -1, 0 .. 2: the definition.  For every pair, over the sites
    where both counts are >= 0, the number of such sites and the sum of |c_i - c_j|; row i against rows i .. N - 1, mirrored."""
    c = B.check_counts(c, 2)
    N, K = c.shape
    d, n = np.zeros((N, N), dtype=np.int32), np.zeros((N, N), dtype=np.int32)
    called = c >= 0
    step = max(1, chunk // max(N, 1))
    for i in range(N):
        for k0 in range(0, K, step):
            both = called[i:, k0:k0 + step] & called[i, k0:k0 + step]
            diff = np.abs(c[i:, k0:k0 + step] - c[i, k0:k0 + step])      # int8: at most 3
            d[i, i:] += np.sum(diff, axis=1, dtype=np.int32, where=both)
            n[i, i:] += np.sum(both, axis=1, dtype=np.int32)
        d[i:, i], n[i:, i] = d[i, i:], n[i, i:]
    return d, n


def planes(c):
    """The byte planes the kernel multiplies: m = [c >= 0], t1 = [c >= 1], t2 = [c >= 2], a = t1 + t2 (uint8 [N][K])."""
    c = np.asarray(c, dtype=np.int8)
    m, t1, t2 = (c >= 0).view(np.uint8), (c >= 1).view(np.uint8), (c >= 2).view(np.uint8)
    return m, t1 + t2, t1, t2


def pairs_planes(c):
    """(d, n) by the identity loc_ibs_pairs computes: n = M M', d = A M' + M A' - 2 (T1 T1' + T2 T2').  float64 products of
    small integers are exact below 2^53; the sums are returned as int32."""
    m, a, t1, t2 = (p.astype(np.float64) for p in planes(B.check_counts(c, 2)))
    am = a @ m.T
    d = am + am.T - 2.0 * (t1 @ t1.T + t2 @ t2.T)
    return d.astype(np.int32), (m @ m.T).astype(np.int32)


def pairs_device(c, k_groups=0, pitch=None, pad_fill=-1, device="cuda:0", keep_on_device=False):
    """pairs_host's answers from one loc_ibs_pairs launch.  keep_on_device: the two int32 tensors, not NumPy arrays."""
    import torch
    from . import _device as D, _lib
    lib = _lib.load()
    c = B.check_counts(c, 2)
    N, K = c.shape
    buf = B.padded(c, pitch, pad_fill)
    with torch.cuda.device(device):
        d_c = D.put(buf, np.int8, device)
        d_d = torch.empty((max(N, 1), max(N, 1)), dtype=torch.int32, device=device)
        d_n = torch.empty_like(d_d)
        work_bytes = int(lib.loc_ibs_work_bytes(N, K, int(k_groups)))
        work = torch.empty(max(work_bytes, 1), dtype=torch.uint8, device=device)
        _lib.check(lib.loc_ibs_pairs(d_c.data_ptr(), N, K, buf.shape[1], int(k_groups), d_d.data_ptr(), d_n.data_ptr(),
                                     work.data_ptr(), work_bytes, D.stream()), "loc_ibs_pairs")
        if keep_on_device:
            torch.cuda.synchronize()
            return d_d, d_n
        return d_d.cpu().numpy()[:N, :N], d_n.cpu().numpy()[:N, :N]


def distances(d, n, P):
    """D = float64(d) / float64(P n), NaN where n = 0."""
    d, n = np.asarray(d), np.asarray(n)
    D = np.full(d.shape, np.nan)
    np.divide(d.astype(np.float64), (P * n.astype(np.int64)).astype(np.float64), out=D, where=n > 0)
    return D


# ---------------------------------------------------------------- neighbours

def knn_host(d, n, P, candidate, kmax):
    """(nbr int32 [N][kmax], nbr_dist float64 [N][kmax]): for row i the candidates j != i with n[i][j] > 0, by D ascending,
    equal doubles to the lower j (a stable sort of the candidates in index order); -1 / NaN past the last."""
    D = distances(d, n, P)
    N = len(D)
    candidate = np.asarray(candidate).astype(bool)
    nbr = np.full((N, kmax), -1, dtype=np.int32)
    dist = np.full((N, kmax), np.nan)
    for i in range(N):
        ok = candidate & (np.asarray(n[i]) > 0)
        ok[i] = False
        js = np.flatnonzero(ok)
        js = js[np.argsort(D[i, js], kind="stable")][:kmax]
        nbr[i, :len(js)] = js
        dist[i, :len(js)] = D[i, js]
    return nbr, dist


def knn_device(d_d, d_n, N, P, candidate, kmax, device="cuda:0"):
    """knn_host's answers from one loc_ibs_knn launch; d_d, d_n are NumPy arrays or the device tensors of pairs_device."""
    import torch
    from . import _device as D, _lib
    lib = _lib.load()
    with torch.cuda.device(device):
        if not torch.is_tensor(d_d):
            d_d, d_n = D.put(np.reshape(d_d, (N, N)), np.int32, device), D.put(np.reshape(d_n, (N, N)), np.int32, device)
        d_cand = D.put(np.asarray(candidate).astype(np.uint8), np.uint8, device)
        d_nbr = torch.empty((max(N, 1), kmax), dtype=torch.int32, device=device)
        d_dist = torch.empty((max(N, 1), kmax), dtype=torch.float64, device=device)
        _lib.check(lib.loc_ibs_knn(d_d.data_ptr(), d_n.data_ptr(), N, int(P), d_cand.data_ptr(), int(kmax), d_nbr.data_ptr(),
                                   d_dist.data_ptr(), D.stream()), "loc_ibs_knn")
        return d_nbr.cpu().numpy()[:N], d_dist.cpu().numpy()[:N]


# ---------------------------------------------------------------- placement

def placements(nbr, locs):
    """[kmax][N][2]: for k = 1 .. kmax the mean location of each row's first k neighbours, summed in rank order; a row with
    fewer than k neighbours keeps the mean over those it has, a row with none is NaN."""
    nbr = np.asarray(nbr)
    have = nbr >= 0
    xy = np.where(have[:, :, None], np.asarray(locs, dtype=np.float64)[np.maximum(nbr, 0)], 0.0)
    sums = np.cumsum(xy, axis=1)
    cnt = np.cumsum(have, axis=1).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.transpose(sums / cnt[:, :, None], (1, 0, 2))


def neighbors(c, P, samples, locs, out=None, k="auto", kmax=32, longlat=False, close=None, keep_matrix=False, host=False,
              silence=False, device="cuda:0", extra=None):
    """The command's work for a count matrix: returns the summary dict and writes the output files when `out` is given.
    extra: entries appended to the summary (--ld_prune: what baselines.prelude recorded)."""
    c = B.check_counts(c, P)
    N, K = c.shape
    samples = np.asarray(samples).astype(str)
    locs, located = B.located_mask(locs, N, PROG)
    if not 1 <= kmax <= B.KMAX_LIMIT:
        raise SystemExit(f"locator_amd.neighbors: --kmax must be 1 .. {B.KMAX_LIMIT}")
    if k != "auto" and not 1 <= int(k) <= kmax:
        raise SystemExit(f"locator_amd.neighbors: --k must be `auto` or 1 .. --kmax ({kmax})")
    if host:
        d, n = pairs_host(c)
        nbr, nbr_dist = knn_host(d, n, P, located, kmax)
    else:
        B.require_gpu(PROG, LAUNCH)
        d_d, d_n = pairs_device(c, device=device, keep_on_device=True)
        nbr, nbr_dist = knn_device(d_d, d_n, N, P, located, kmax, device=device)
        d, n = d_d.cpu().numpy()[:N, :N], d_n.cpu().numpy()[:N, :N]     # downloaded once: the diagnostics are host NumPy
    D = distances(d, n, P)

    placed = placements(nbr, locs)
    k_auto, med = B.choose_smallest_median(placed, locs, located, longlat, NOTHING_TO_CHOOSE_BY)
    k_used = k_auto if k == "auto" else int(k)
    xy = placed[k_used - 1]
    shared, shared_lines = B.placement_summary(c, P, located, xy, locs, longlat, "kNN")
    li = np.flatnonzero(located)
    iu = np.triu_indices(len(li), 1)
    pa, pb = li[iu[0]], li[iu[1]]
    geo = B.errors(locs[pa], locs[pb], longlat)
    gen = D[pa, pb]
    both = ~np.isnan(gen)
    with np.errstate(divide="ignore", invalid="ignore"):
        r_geo = float(np.corrcoef(gen[both], geo[both])[0][1]) if both.sum() > 1 else np.nan
    own = {"kmax": int(kmax), "k": int(k_used), "k_auto": int(k_auto), "k_chosen_by": "auto" if k == "auto" else "--k",
           "median_error_by_k": [B.num(v) for v in med], "pearson_r_ibs_geo": B.num(r_geo), "n_located_pairs": int(both.sum()),
           "n_pairs_no_shared_site": int((np.triu(n == 0, 1)).sum())}
    summary = {key: {**shared, **own}[key] for key in SUMMARY_KEYS}
    pairs = None
    if close is not None:
        ia, ib = np.triu_indices(N, 1)
        with np.errstate(invalid="ignore"):
            hit = D[ia, ib] <= close
        ia, ib = ia[hit], ib[hit]
        order = np.lexsort((ib, ia, D[ia, ib]))
        pairs = (ia[order], ib[order])
        summary["close"] = float(close)
        summary["n_close_pairs"] = int(len(order))
    summary.update(extra or {})

    lines = [f"{N} samples ({int(located.sum())} located), {K} sites, ploidy {P}",
             f"k = {k_used} ({summary['k_chosen_by']}; leave-one-out median error by k, k = 1 .. {kmax}, smallest at k = {k_auto})",
             *shared_lines,
             f"Pearson r of IBS distance and geographic distance over {int(both.sum())} located pairs = {r_geo}"]
    if pairs is not None:
        lines.append(f"{len(pairs[0])} pairs with IBS distance <= {close}")
    if out is not None:
        B.write_locs(out + "_knn_locs.txt", xy, samples)
        rows = ["sampleID\trank\tneighborID\tibs_dist\tn_sites\n"]
        for i in range(N):
            for r in range(kmax):
                j = int(nbr[i, r])
                if j < 0:
                    break
                rows.append(f"{samples[i]}\t{r + 1}\t{samples[j]}\t{float(nbr_dist[i, r])!r}\t{int(n[i, j])}\n")
        write_atomic(out + "_neighbors.txt", "".join(rows))
        write_atomic(out + "_knn_summary.json", json.dumps(summary, indent=1) + "\n")
        if pairs is not None:
            write_atomic(out + "_close_pairs.txt", "sampleA\tsampleB\tibs_dist\tn_sites\n" + "".join(
                f"{samples[a]}\t{samples[b]}\t{float(D[a, b])!r}\t{int(n[a, b])}\n" for a, b in zip(*pairs)))
        if keep_matrix:
            write_atomic(out + "_ibs.npz", lambda fh: B.save_npz(fh, d=d, n=n, samples=samples), mode="wb")
    if not silence:
        for line in lines:
            print(line)
    summary["_nbr"], summary["_nbr_dist"], summary["_xy"] = nbr, nbr_dist, xy
    return summary


# ---------------------------------------------------------------- command

def _own_arguments(p):
    B.add_k_arguments(p, 32, "neighbours", "neighbours")
    p.add_argument("--longlat", default=False, action="store_true",
                   help="x / y are longitude / latitude degrees: errors are great-circle km (the mean stays planar)")
    p.add_argument("--close", default=None, type=float, metavar="T",
                   help="also list every sample pair with IBS distance <= T in {out}_close_pairs.txt (no default threshold)")
    p.add_argument("--keep_matrix", default=False, action="store_true", help="keep d, n and the sample IDs in {out}_ibs.npz")
    p.add_argument("--host", default=False, action="store_true", help="the NumPy form instead of the GPU (same files)")


def build_parser():
    return B.build_parser(PROG, "IBS distances of all sample pairs and a k-nearest-neighbour placement baseline.", _own_arguments)


def main(argv=None):
    parser = build_parser()
    a = B.parse_args(parser, argv)
    B.check_k(parser, a)
    if a.close is not None and not a.close >= 0:
        parser.error("--close must be a distance >= 0")
    c, P, samples, locs, _ = B.prelude(parser, a, LAUNCH)
    try:
        neighbors(c, P, samples, locs, a.out, a.k, a.kmax, a.longlat, a.close, a.keep_matrix, a.host, a.silence,
                  extra=getattr(a, "ld_summary", None))
    except ValueError as e:
        raise SystemExit(f"{PROG}: {e}") from None
    return 0


if __name__ == "__main__":
    sys.exit(main())
