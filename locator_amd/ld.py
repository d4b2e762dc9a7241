#!/usr/bin/env python3
"""`python -m locator_amd.ld`: linkage disequilibrium between neighbouring sites, and LD pruning.  neighbors and pca sum over every
site a fit would train on; sites in LD are then counted many times over, and a low-recombination block can own a principal
component.  The usual remedy is to prune before summing (PLINK --indep-pairwise, scikit-allel locate_unlinked, smartpca
r2thresh): this command does it and says how much LD there was; --ld_prune gives the same pruning to neighbors and pca.

  python -m locator_amd.ld --vcf genotypes.vcf.gz --out out/test --r2 0.2 --ld_window 100

  counts   ct [K][N] int8, site-major: the values of baselines.count_matrix, not transposed (count_matrix_sites): -1 = missing,
           0 .. P.  The sites are those of genotypes.filter_snps with the same --min_mac / --max_SNPs / --seed, TAKEN IN
           ASCENDING VARIANT INDEX: a window is a run of neighbouring sites of the input.
  sums     for sites i < j over the samples where both are called (m = [c >= 0], a = max(c, 0)): n = sum m_i m_j,
           sa = sum a_i m_j, sb = sum m_i a_j, sab = sum a_i a_j, saa = sum a_i^2 m_j, sbb = sum m_i a_j^2, six exact int32
           sums (`sums_host`): pairwise-complete, as PLINK and scikit-allel do it.
  r2       in float64 from those integers (`r2_host`): cov = n sab - sa sb, va = n saa - sa^2, vb = n sbb - sb^2, exact below 2^53
           for N < 2^20; r2 = (cov cov) / (va vb), two correctly rounded products and one correctly rounded division; NaN where
           n < 2, va <= 0 or vb <= 0.  A pair is `over` where r2 > --r2; NaN is never over.
  window   reach[i] = the number of following sites i is compared with (`reach_host`): at most --ld_window, at most K - 1 - i,
           only sites of the same CHROM, with --ld_window_bp B only sites with POS_j - POS_i <= B.
  pruning  `greedy_host`: walk i = 0 .. K - 1; a site still kept removes every j in i + 1 .. i + reach[i] that is over with
           it, removed_by[j] = i.  The earlier site always wins; there is no allele-frequency rule (PLINK removes the site
           with the lower minor-allele frequency).  The walk is sequential and runs on the host over the downloaded bit mask.

loc_ld_band (include/locator_hip_ld.h) gives the same integers, the same doubles bit for bit and the same mask from the int8
matrix pipe.  Outputs: {out}_ld_sites.txt (variant chrom pos kept removed_by), {out}_ld_summary.json, with --keep_matrix
{out}_ld.npz (over, reach, sites).  Device and --host runs write the same bytes.  There is no silent fallback: without a GPU
the run stops and says so; --host asks for the NumPy form.

Not built: --ld_prune for the fit itself; --phased / --dosage inputs; a greedy pass on the device; an r2-decay table.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

from . import _abi
from . import baselines as B
from ._files import write_atomic

TILE = _abi.LOC_LD_TILE
BLOCK = _abi.LOC_LD_BLOCK
MAX_WINDOW = _abi.LOC_LD_MAX_WINDOW
MAX_SAMPLES = 1 << 20
PROG = "locator_amd.ld"
LAUNCH = "the pair statistics are one loc_ld_band launch"


# ---------------------------------------------------------------- the definitions

def check_sites(ct, W):
    """ct as an int8 [K][N] array (negative = -1) and W, after the refusals that precede any work."""
    ct = np.asarray(ct)
    if ct.ndim != 2:
        raise ValueError(f"count matrix of shape {ct.shape}: needs [sites][samples]")
    if not 1 <= int(W) <= MAX_WINDOW:
        raise ValueError(f"window of {W} sites: must be 1 .. {MAX_WINDOW}")
    if ct.shape[1] >= MAX_SAMPLES:
        raise ValueError(f"{ct.shape[1]} samples: the products of the pair sums must stay below 2^53 (fewer than 2^20 samples)")
    if ct.size and int(ct.max()) > 2:
        raise ValueError(f"a count of {int(ct.max())}: allele-1 counts are 0 .. 2, missing is -1")
    ct = np.ascontiguousarray(ct, dtype=np.int8)
    return (np.where(ct < 0, np.int8(-1), ct) if ct.size and int(ct.min()) < -1 else ct), int(W)


def planes(ct):
    """The byte planes the kernel multiplies: m = [c >= 0], a = t1 + t2, a2 = t1 + 3 t2 (= a a) with t1 = [c >= 1], t2 = [c >= 2]."""
    ct = np.asarray(ct, dtype=np.int8)
    m, t1, t2 = (ct >= 0).view(np.uint8), (ct >= 1).view(np.uint8), (ct >= 2).view(np.uint8)
    return m, t1 + t2, t1 + 3 * t2


def clamp_reach(reach, K, W):
    """reach (None = W everywhere) clamped to 0 .. min(W, K - 1 - i), int32 [K]: what the kernel does with its argument."""
    i = np.arange(K, dtype=np.int64)
    r = np.full(K, W, dtype=np.int64) if reach is None else np.asarray(reach, dtype=np.int64).reshape(K)
    return np.clip(np.minimum(r, np.minimum(W, K - 1 - i)), 0, None).astype(np.int32)


def sums_host(ct, W, reach=None, rows=256):
    """int32 [K][W][6]: slot l of row i holds n, sa, sb, sab, saa, sbb of the pair (i, i + 1 + l), zeros where l >= reach[i].
    Blocks of `rows` sites against the sites of their windows; the products are float64 matrix products of small integers,
    exact below 2^53 whatever the order of the additions."""
    ct, W = check_sites(ct, W)
    K, N = ct.shape
    reach = clamp_reach(reach, K, W)
    out = np.zeros((K, W, 6), dtype=np.int32)
    m = (ct >= 0).astype(np.float64)
    a = np.maximum(ct, 0).astype(np.float64)
    aa = a * a
    lag = np.arange(W)
    for i0 in range(0, K, rows):
        i1 = min(K, i0 + rows)
        j0, j1 = i0 + 1, min(K, i1 + W)                 # the sites the block's windows cover
        if j1 <= j0:
            continue
        mi, ai, qi, mj, aj, qj = m[i0:i1], a[i0:i1], aa[i0:i1], m[j0:j1].T, a[j0:j1].T, aa[j0:j1].T
        full = np.stack([mi @ mj, ai @ mj, mi @ aj, ai @ aj, qi @ mj, mi @ qj], axis=2)      # [rows][sites j0 .. j1 - 1][6]
        r = np.arange(i1 - i0)
        col = r[:, None] + lag[None, :]                  # site i0 + r + 1 + l is column r + l
        ok = lag[None, :] < reach[i0:i1, None]           # reach <= K - 1 - i: the column exists
        picked = full[r[:, None], np.minimum(col, j1 - j0 - 1)]
        out[i0:i1] = np.where(ok[:, :, None], picked, 0.0).astype(np.int32)
    return out


def r2_host(sums):
    """float64 [...]: r2 of sums [...][6] as defined above; NaN where n < 2, va <= 0 or vb <= 0 (an empty slot has n = 0)."""
    s = np.asarray(sums).astype(np.int64)
    n, sa, sb, sab, saa, sbb = (s[..., q] for q in range(6))
    cov, va, vb = n * sab - sa * sb, n * saa - sa * sa, n * sbb - sb * sb
    ok = (n >= 2) & (va > 0) & (vb > 0)
    c = cov.astype(np.float64)
    num = c * c
    den = va.astype(np.float64) * vb.astype(np.float64)
    out = np.full(n.shape, np.nan)
    np.divide(num, den, out=out, where=ok)
    return out


def pack_bits(flags):
    """bool [K][W] -> uint32 [K][(W + 31) / 32]: bit b of word w of row i = flags[i][32 w + b]."""
    flags = np.asarray(flags, dtype=bool)
    K, W = flags.shape
    words = (W + 31) // 32
    padded = np.zeros((K, 32 * words), dtype=bool)
    padded[:, :W] = flags
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view("<u4").astype(np.uint32).reshape(K, words)


def unpack_bits(over, W):
    """pack_bits backwards: bool [K][W]."""
    over = np.ascontiguousarray(over, dtype="<u4")
    return np.unpackbits(over.view(np.uint8).reshape(len(over), -1), axis=1, bitorder="little")[:, :W].astype(bool)


def over_host(r2, thr):
    """The mask of r2 > thr (NaN is never over) as the kernel lays it out."""
    with np.errstate(invalid="ignore"):
        return pack_bits(np.asarray(r2) > thr)


def band_host(ct, W, reach, thr):
    """(over, sums, r2) by the definitions: what band_device must return."""
    sums = sums_host(ct, W, reach)
    r2 = r2_host(sums)
    return over_host(r2, thr), sums, r2


def reach_host(K, W, chrom=None, pos=None, window_bp=None):
    """int32 [K]: the number of following sites site i is compared with, the largest value with reach <= W, reach <= K - 1 - i,
    every site i + 1 .. i + reach on the CHROM of i and, with window_bp, at most window_bp base pairs after i."""
    if window_bp is not None and pos is None:
        raise ValueError("a window in base pairs needs positions")
    code = np.zeros(K, dtype=np.int64) if chrom is None else np.unique(np.asarray(chrom).astype(str), return_inverse=True)[1]
    pos = None if pos is None else np.asarray(pos, dtype=np.int64)
    reach = np.zeros(K, dtype=np.int32)
    alive = np.ones(K, dtype=bool)
    for lag in range(1, min(W, K - 1) + 1):
        alive[K - lag:] = False
        ok = code[lag:] == code[:K - lag]
        if window_bp is not None:
            ok &= pos[lag:] - pos[:K - lag] <= window_bp
        alive[:K - lag] &= ok
        reach += alive
    return reach


def greedy_host(over, K=None):
    """(kept bool [K], removed_by int64 [K], -1 = kept): the greedy walk over the bit mask.  `window` holds, as one Python
    integer, the removed flags of the sites after the current one, so every step is a few operations on whole words; single
    bits are looked at only to name the sites a step newly removes (each site once)."""
    over = np.ascontiguousarray(over, dtype="<u4")
    K = len(over) if K is None else K
    row_bytes = over.shape[1] * 4 if K else 0
    raw = over.tobytes()
    removed_by = np.full(K, -1, dtype=np.int64)
    window, gone = 0, 0
    for i in range(K):
        if not gone:
            row = int.from_bytes(raw[i * row_bytes:(i + 1) * row_bytes], "little")
            new = row & ~window
            if new:
                window |= new
                while new:
                    low = new & -new
                    removed_by[i + low.bit_length()] = i        # bit l is site i + 1 + l
                    new ^= low
        gone = window & 1
        window >>= 1
    return removed_by < 0, removed_by


def lag_buckets(over, W):
    """{"1": .., "2": .., "3-4": .., "5-8": ..}: set bits per lag j - i, in buckets that double."""
    per_lag = unpack_bits(over, W).sum(axis=0, dtype=np.int64) if len(over) else np.zeros(W, dtype=np.int64)
    out, lo = {}, 1
    while lo <= W:
        hi = min(W, 1 if lo == 1 else 2 * (lo - 1))
        out[str(lo) if lo == hi else f"{lo}-{hi}"] = int(per_lag[lo - 1:hi].sum())
        lo = hi + 1
    return out


# ---------------------------------------------------------------- the device form

def band_device(ct, W, reach=None, thr=0.2, want_sums=True, want_r2=True, pitch=None, pad_fill=-1, device="cuda:0", fill=None):
    """(over, sums, r2) from one loc_ld_band launch; sums / r2 None where not wanted.  pitch / pad_fill as baselines.padded.
    fill: a byte the output buffers hold before the launch (tests: the launch must define every element)."""
    import torch
    from . import _device as D, _lib
    lib = _lib.load()
    ct = np.ascontiguousarray(ct, dtype=np.int8)
    K, N = ct.shape
    W = int(W)
    words = (W + 31) // 32
    buf = B.padded(ct, pitch, pad_fill)
    if not buf.size:
        buf = np.full((1, max(buf.shape[1], 16)), -1, dtype=np.int8)      # no site: the launcher still wants a buffer
    with torch.cuda.device(device):
        d_ct = D.put(buf, np.int8, device)
        d_reach = None if reach is None else D.put(np.reshape(reach, K), np.int32, device)
        if d_reach is not None and K == 0:
            d_reach = torch.zeros(1, dtype=torch.int32, device=device)
        d_over = torch.empty((max(K, 1), words), dtype=torch.int32, device=device)
        d_sums = torch.empty((max(K, 1), W, 6), dtype=torch.int32, device=device) if want_sums else None
        d_r2 = torch.empty((max(K, 1), W), dtype=torch.float64, device=device) if want_r2 else None
        if fill is not None:
            for d in (d_over, d_sums, d_r2):
                if d is not None:
                    d.view(torch.uint8).fill_(int(fill))
        _lib.check(lib.loc_ld_band(d_ct.data_ptr(), K, N, buf.shape[1], W, None if d_reach is None else d_reach.data_ptr(),
                                   float(thr), d_over.data_ptr(), None if d_sums is None else d_sums.data_ptr(),
                                   None if d_r2 is None else d_r2.data_ptr(), D.stream()), "loc_ld_band")
        over = d_over.cpu().numpy()[:K].view(np.uint32)
        return over, None if d_sums is None else d_sums.cpu().numpy()[:K], None if d_r2 is None else d_r2.cpu().numpy()[:K]


# ---------------------------------------------------------------- pruning

def over_mask(ct, W, reach, thr, host, device="cuda:0"):
    """The mask alone: the NumPy form, or one loc_ld_band launch without sums and r2."""
    ct, W = check_sites(ct, W)
    if host:
        return band_host(ct, W, reach, thr)[0]
    B.require_gpu(PROG, LAUNCH)
    return band_device(ct, W, reach, thr, want_sums=False, want_r2=False, device=device)[0]


def prune_sites(gt, idx, chrom, pos, thr, W, window_bp, host):
    """--ld_prune of the baseline commands: the variant indices among idx that survive the pruning, ascending.  The sites are
    compared in ascending variant index whatever the order of idx."""
    order = np.sort(np.asarray(idx, dtype=np.int64))
    ct, _ = B.count_matrix_sites(gt, order)
    reach = reach_host(len(order), W, None if chrom is None else np.asarray(chrom)[order], None if pos is None else np.asarray(pos)[order],
                       window_bp)
    kept, _ = greedy_host(over_mask(ct, W, reach, thr, host))
    return order[kept]


# ---------------------------------------------------------------- the command's work

def ld(ct, P, sites, chrom, pos, out=None, thr=None, W=100, window_bp=None, keep_matrix=False, host=False, silence=False,
       device="cuda:0"):
    """The command's work for site-major counts of the variants `sites` (ascending): returns the summary dict and writes the
    output files when `out` is given.  chrom / pos: per site, or None (one chromosome, no positions)."""
    ct, W = check_sites(ct, W)
    K, N = ct.shape
    sites = np.asarray(sites, dtype=np.int64).reshape(K)
    if thr is None or not np.isfinite(thr):
        raise ValueError("the r2 threshold must be a finite number")
    reach = reach_host(K, W, chrom, pos, window_bp)
    over = over_mask(ct, W, reach, thr, host, device)
    kept, removed_by = greedy_host(over)
    n_over = int(unpack_bits(over, W).sum()) if K else 0
    summary = {"K": int(K), "n_kept": int(kept.sum()), "P": int(P), "N": int(N), "r2": float(thr), "window": int(W),
               "window_bp": None if window_bp is None else int(window_bp), "n_pairs_compared": int(reach.sum(dtype=np.int64)),
               "n_pairs_over": n_over, "pairs_over_by_lag": lag_buckets(over, W)}
    lines = [f"{K} sites, {N} samples, ploidy {P}; window {W} sites" + ("" if window_bp is None else f" and {window_bp} bp"),
             f"{summary['n_pairs_over']} of {summary['n_pairs_compared']} compared pairs have r2 > {thr}",
             f"{summary['n_kept']} sites kept, {K - summary['n_kept']} removed"]
    if out is not None:
        names = np.full(K, ".", dtype=object) if chrom is None else np.asarray(chrom).astype(str)
        where = np.full(K, "NA", dtype=object) if pos is None else np.asarray(pos, dtype=np.int64).astype(str)
        write_atomic(out + "_ld_sites.txt", "variant\tchrom\tpos\tkept\tremoved_by\n" + "".join(
            f"{sites[i]}\t{names[i]}\t{where[i]}\t{int(kept[i])}\t{'NA' if removed_by[i] < 0 else sites[removed_by[i]]}\n"
            for i in range(K)))
        write_atomic(out + "_ld_summary.json", json.dumps(summary, indent=1) + "\n")
        if keep_matrix:
            write_atomic(out + "_ld.npz", lambda fh: B.save_npz(fh, over=over, reach=reach, sites=sites), mode="wb")
    if not silence:
        for line in lines:
            print(line)
    summary["_over"], summary["_reach"], summary["_kept"], summary["_removed_by"] = over, reach, kept, removed_by
    return summary


# ---------------------------------------------------------------- command

def _own_arguments(p):
    p.add_argument("--r2", required=True, type=float, help="the r2 threshold above which a kept site removes a later one (no default)")
    B.add_window_arguments(p)
    p.add_argument("--keep_matrix", default=False, action="store_true", help="keep the mask, reach and the site indices in {out}_ld.npz")
    p.add_argument("--host", default=False, action="store_true", help="the NumPy form instead of the GPU (same files)")


def build_parser():
    return B.build_parser(PROG, "Linkage disequilibrium between neighbouring sites, and greedy LD pruning.", _own_arguments,
                          sample_data=False, prune=False)


def main(argv=None):
    parser = build_parser()
    a = B.parse_args(parser, argv)
    if not np.isfinite(a.r2):
        parser.error("--r2 must be a finite r2 threshold")
    B.check_window(parser, a)
    if a.gpu_number is not None:
        for var in ("HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
            os.environ[var] = a.gpu_number
    if not a.host:
        B.require_gpu(PROG, LAUNCH)
    from . import genotypes as G
    if a.seed is not None:
        np.random.seed(a.seed)
    gt, _, chrom, pos = B.read_inputs_sites(a, PROG)
    _, idx = G.filter_snps(gt, min_mac=a.min_mac, max_snps=a.max_SNPs, verbose=False, sites=True)
    sites = np.sort(np.asarray(idx, dtype=np.int64))
    try:
        ct, P = B.count_matrix_sites(gt, sites)
        ld(ct, P, sites, None if chrom is None else np.asarray(chrom)[sites], None if pos is None else np.asarray(pos)[sites], a.out,
           a.r2, a.ld_window, a.ld_window_bp, a.keep_matrix, a.host, a.silence)
    except ValueError as e:
        raise SystemExit(f"{PROG}: {e}") from None
    return 0


if __name__ == "__main__":
    sys.exit(main())
