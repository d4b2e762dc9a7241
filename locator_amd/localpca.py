#!/usr/bin/env python3
"""`python -m locator_amd.localpca`: a PCA per window of the genome, a distance between every two windows' low-rank structure,
an MDS of the windows and the windows that stand apart (the lostruct method of Li & Ralph 2019).  The pca command reports one
set of axes for the whole genome; this one shows where along the genome the structure differs - an inversion, an introgressed
block, a stretch of low recombination - which is what a fit's --windows predictions respond to.

  python -m locator_amd.localpca --vcf genotypes.vcf.gz --sample_data samples.txt --out out/test --window_snps 500

  counts      c [N][K] int8 as the other baselines take them (baselines.prelude), the K filtered sites IN ASCENDING VARIANT
              ORDER (a --max_SNPs draw is sorted); mean, scale float32 [K] = pca.site_constants over all samples: global,
              not per window.
  windows     win [W][2] int64 = (v0, v1), 0 <= v0 <= v1 <= K: half-open runs of columns of c.  They may overlap, repeat or
              be empty; `check_windows` refuses anything else.  `window_bounds` builds them, never across two chromosomes:
              --window_snps S: runs of S filtered sites per chromosome from site --window_start of the chromosome on, the last
              one shorter; --window_bp B: [start + n B', start + n B' + B) per chromosome for n = 0, 1, .. while the window's
              start does not exceed the chromosome's largest filtered position (the geometry of a fit's --windows, except that
              a fit stops BEFORE a window that starts at the largest position; empty windows are kept and listed).  B' =
              --window_step (default: the window size) slides the windows.  The table names a bp window by start and stop =
              start + B, the `start`-`stop - 1` of a fit's output stem; a site window by the positions of its first and last
              site (stop = last position + 1), with --matrix (one chromosome `1`, no positions: --window_snps only) by their
              variant indices.
  G_w         Z[:, v0:v1] Z[:, v0:v1]' with pca.z_host (`windows_host`: float64, the definition; `windows_device`: one
              loc_grm_windows launch per batch of windows, include/locator_hip_localpca.h, fp32).  K_used_w = the sites of
              the window with scale > 0.
  components  pca.components(G_w, K_used_w, npc) per window on the host in float64: eigenvalues of G_w / K_used_w, sign-fixed
              eigenvectors.  npc 1 .. 10 (default 2).  A window with K_used_w < min_sites (default max(10, 2 npc)) is SKIPPED:
              listed in the table, never part of the distances.
  distance    `pc_dist`: a_w = max(lam_w, 0) / ||max(lam_w, 0)||_2, d^2(v, w) = sum_i a_vi^2 + sum_j a_wj^2 - 2 sum_ij a_vi a_wj
              (u_vi . u_wj)^2 clamped at 0: the Frobenius distance between sum_i a_wi u_wi u_wi' of the two windows.  It does
              not depend on eigenvector signs, is 0 for equal windows (the diagonal is set to 0; two DIFFERENT windows that
              hold the same matrix come out within the root of the rounding of d^2, about 1e-8) and sqrt(2) for orthogonal
              subspaces.  Host float64, one (W npc x N) product.
  MDS         `mds`: classical, eigh of -1/2 J D^2 J, the m leading axes (default 2), coordinates v sqrt(max(lambda, 0)),
              signs as pca.components.
  outliers    `robust_scores`: per axis (y - median) / (1.4826 MAD); a window is flagged when |score| > --outlier (default 3)
              on any axis.  An axis whose MAD is 0 flags nothing and the summary names it.  `merge_regions`: maximal runs of
              consecutive flagged windows of one chromosome (a skipped or unflagged window ends a run).
  locations   with --sample_data, per window pca.pc_r2 of its PCs against x and y over the located samples: which axis carries
              x and which y in that stretch of genome.  --longlat is accepted and recorded; a correlation does not depend on it.

Outputs: {out}_localpca_windows.txt (one row per window, skipped ones included), {out}_localpca_regions.txt,
{out}_localpca_summary.json, with --keep_matrix {out}_localpca_dist.npz, with --keep_components
{out}_localpca_components.npz.  There is no silent fallback: without a GPU the run stops and says so; --host asks for the NumPy
form.  The device forms G_w in fp32, --host in float64, so the files of the two paths differ within fp32 arithmetic: per
element |G_dev - G_host| <= (S_w + 8) 2^-24 sum_k |z_ik| |z_jk| over the window's S_w sites (the derivation of pca.py).  Each
path is deterministic: two runs write the same bytes.

Not built: --phased and --dosage inputs; a plot; an eigensolver on the device (the eigen step is host float64, as in pca.py);
the L1 and covariance variants of lostruct.
"""
from __future__ import annotations

import json
import sys

import numpy as np

from . import _abi
from . import baselines as B
from . import pca as PCA
from ._files import write_atomic

PROG = "locator_amd.localpca"
LAUNCH = "the window matrices are loc_grm_windows launches"
MAX_WINDOWS = _abi.LOC_LOCALPCA_MAX_WINDOWS
NPC_LIMIT = 10
BATCH_BYTES = 1 << 30
# the key order of {out}_localpca_summary.json
SUMMARY_KEYS = ("N", "n_located", "K", "K_used", "P", "window_unit", "window_size", "window_start", "window_step", "W", "W_kept",
                "W_skipped", "npc", "mds", "min_sites", "outlier", "longlat", "mds_eigenvalues", "median", "mad", "mad_zero_axes",
                "n_flagged", "flagged", "n_regions")


# ---------------------------------------------------------------- windows

def check_windows(win, K):
    """win as a contiguous int64 [W][2] array after the refusals that precede any upload: W >= 1, whole numbers,
    0 <= v0 <= v1 <= K."""
    w = np.asarray(win)
    if w.ndim != 2 or w.shape[1] != 2 or len(w) < 1:
        raise ValueError(f"windows of shape {w.shape}: needs [W][2] with W >= 1")
    if not np.issubdtype(w.dtype, np.integer):
        if not (np.issubdtype(w.dtype, np.floating) and np.isfinite(w).all() and (w == np.floor(w)).all()):
            raise ValueError("window bounds must be whole numbers")
    w = np.ascontiguousarray(w, dtype=np.int64)
    bad = np.flatnonzero((w[:, 0] < 0) | (w[:, 0] > w[:, 1]) | (w[:, 1] > K))
    if len(bad):
        raise ValueError(f"window {int(bad[0])} = ({int(w[bad[0], 0])}, {int(w[bad[0], 1])}): needs 0 <= v0 <= v1 <= K = {K}")
    return w


def window_bounds(chrom, pos, idx, snps=None, bp=None, start=0, step=None):
    """(win int64 [W][2], table) for the K filtered sites idx (ascending variant indices) with their CHROM and POS (chrom, pos:
    [K], or None for a --matrix: one chromosome `1`, no positions).  Exactly one of snps / bp; table = {"chrom" [W] str,
    "start" [W], "stop" [W] int64} as the module text names a window."""
    idx = np.asarray(idx, dtype=np.int64)
    K = len(idx)
    if (snps is None) == (bp is None):
        raise ValueError("exactly one of --window_snps / --window_bp must be given")
    size = int(snps if bp is None else bp)
    step = size if step is None else int(step)
    start = int(start)
    if size < 1 or step < 1 or start < 0:
        raise ValueError("the window size and --window_step must be >= 1, --window_start >= 0")
    if K and (np.diff(idx) <= 0).any():
        raise ValueError("the sites must be in ascending variant order")
    if bp is not None and pos is None:
        raise ValueError("--window_bp needs positions: a --matrix has none (use --window_snps)")
    chrom = np.full(K, "1") if chrom is None else np.asarray(chrom).astype(str)
    if pos is not None:
        pos = np.asarray(pos, dtype=np.int64)
    if len(chrom) != K or (pos is not None and len(pos) != K):
        raise ValueError("chrom and pos must hold one entry per filtered site")
    edges = np.flatnonzero(chrom[1:] != chrom[:-1]) + 1 if K else np.zeros(0, dtype=np.int64)
    runs = list(zip(np.concatenate([[0], edges]).tolist(), np.concatenate([edges, [K]]).tolist())) if K else []
    names = [chrom[a] for a, _ in runs]
    if len(set(names)) != len(names):
        raise ValueError("the sites of a chromosome are not contiguous in the input: windows are runs of sites of one chromosome")
    win, tab = [], []
    for (a, b), name in zip(runs, names):
        if pos is not None and (np.diff(pos[a:b]) < 0).any():
            raise ValueError(f"the positions of chromosome {name} are not in ascending order")
        if bp is None:
            for s in range(start, b - a, step):
                v0, v1 = a + s, a + min(s + size, b - a)
                lo, hi = (int(idx[v0]), int(idx[v1 - 1]) + 1) if pos is None else (int(pos[v0]), int(pos[v1 - 1]) + 1)
                win.append((v0, v1))
                tab.append((name, lo, hi))
        else:
            p = pos[a:b]
            for lo in range(start, int(p[-1]) + 1, step):
                win.append((a + int(np.searchsorted(p, lo, "left")), a + int(np.searchsorted(p, lo + size, "left"))))
                tab.append((name, lo, lo + size))
    if not win:
        raise ValueError("no window: no filtered site lies at or after --window_start")
    table = {"chrom": np.array([t[0] for t in tab]), "start": np.array([t[1] for t in tab], dtype=np.int64),
             "stop": np.array([t[2] for t in tab], dtype=np.int64)}
    return check_windows(np.array(win, dtype=np.int64), K), table


def used_sites(scale, win):
    """K_used_w [W]: the sites of every window with scale > 0."""
    cum = np.concatenate([[0], np.cumsum(np.asarray(scale) > 0, dtype=np.int64)])
    return cum[win[:, 1]] - cum[win[:, 0]]


# ---------------------------------------------------------------- the window matrices

def windows_host(c, mean, scale, win):
    """G_w = Z[:, v0:v1] Z[:, v0:v1]' in float64, [W][N][N]: the definition."""
    win = check_windows(win, np.shape(c)[1])
    z = PCA.z_host(c, mean, scale)
    return np.stack([z[:, v0:v1] @ z[:, v0:v1].T for v0, v1 in win])


def batch_windows(N, W, batch_bytes=BATCH_BYTES):
    """Windows of one launch: what fits batch_bytes of g (at least one), LOC_LOCALPCA_MAX_WINDOWS at most."""
    return int(max(1, min(MAX_WINDOWS, W, int(batch_bytes) // max(4 * N * N, 1))))


def windows_batches(c, mean, scale, win, batch_bytes=BATCH_BYTES, pitch=None, pad_fill=-1, device="cuda:0", g_fill=None,
                    on_device=None):
    """Yields (w0, g float32 [n][N][N]) batch by batch: c, mean and scale are uploaded once, every batch is one loc_grm_windows
    launch and one download.  g_fill: a float32 bit pattern g holds before the launch (tests)."""
    import torch
    from . import _device as D, _lib
    lib = _lib.load()
    c = np.ascontiguousarray(c, dtype=np.int8)
    N, K = c.shape
    win = check_windows(win, K)
    d_c, d_mean, d_scale, pitch = on_device or PCA._upload(c, mean, scale, pitch, pad_fill, device)
    per = batch_windows(N, len(win), batch_bytes)
    with torch.cuda.device(device):
        d_g = torch.empty((per, max(N, 1), max(N, 1)), dtype=torch.float32, device=device)
        for w0 in range(0, len(win), per):
            n = min(per, len(win) - w0)
            d_win = D.put(win[w0:w0 + n], np.int64, device)
            D.prefill((d_g,), g_fill)
            _lib.check(lib.loc_grm_windows(d_c.data_ptr(), N, K, pitch, d_mean.data_ptr(), d_scale.data_ptr(), d_win.data_ptr(), n,
                                           d_g.data_ptr(), D.stream()), "loc_grm_windows")
            yield w0, d_g[:n].cpu().numpy()[:, :N, :N]


def windows_device(c, mean, scale, win, **kw):
    """windows_host's matrices from loc_grm_windows, float32 [W][N][N]."""
    return np.concatenate([g for _, g in windows_batches(c, mean, scale, win, **kw)])


# ---------------------------------------------------------------- distances, MDS, outliers

def pc_dist(lam, U):
    """D [W][W] float64 from the kept eigenvalues lam [W][npc] and eigenvectors U [W][N][npc] (the module text)."""
    lam = np.asarray(lam, dtype=np.float64)
    U = np.asarray(U, dtype=np.float64)
    W, N, npc = U.shape
    a = np.maximum(lam, 0.0)
    norm = np.sqrt((a * a).sum(axis=1, keepdims=True))
    a = np.divide(a, norm, out=np.zeros_like(a), where=norm > 0)
    M = U.transpose(0, 2, 1).reshape(W * npc, N)
    C2 = ((M @ M.T) ** 2).reshape(W, npc, W, npc)
    cross = np.einsum("vi,viwj,wj->vw", a, C2, a)
    own = (a * a).sum(axis=1)
    D = np.sqrt(np.maximum(own[:, None] + own[None] - 2.0 * cross, 0.0))
    D = 0.5 * (D + D.T)                                               # the product is symmetric up to rounding
    np.fill_diagonal(D, 0.0)
    return D


def mds(D, m=2):
    """(Y [W][m], lam [m]): classical MDS of the distances D, the m leading axes of -1/2 J D^2 J, Y = v sqrt(max(lam, 0)), each
    axis flipped so that its coordinate of largest magnitude (the lowest index on a tie) is positive."""
    D = np.asarray(D, dtype=np.float64)
    W = len(D)
    if not 1 <= m <= max(W - 1, 1):
        raise ValueError(f"mds = {m} with {W} windows: needs 1 .. windows - 1 axes")
    J = np.eye(W) - 1.0 / W
    Bm = -0.5 * J @ (D * D) @ J
    lam, V = np.linalg.eigh(0.5 * (Bm + Bm.T))
    lam, V = lam[::-1][:m].copy(), V[:, ::-1][:, :m].copy()
    big = np.argmax(np.abs(V), axis=0)
    V *= np.where(V[big, np.arange(m)] < 0, -1.0, 1.0)[None]
    return V * np.sqrt(np.maximum(lam, 0.0))[None], lam


def robust_scores(Y):
    """(scores [W][m], median [m], mad [m]): (y - median) / (1.4826 MAD) per axis; an axis whose MAD is 0 scores 0 everywhere."""
    Y = np.asarray(Y, dtype=np.float64)
    med = np.median(Y, axis=0)
    mad = np.median(np.abs(Y - med[None]), axis=0)
    s = np.zeros_like(Y)
    np.divide(Y - med[None], 1.4826 * mad[None], out=s, where=(mad > 0)[None])
    return s, med, mad


def merge_regions(chrom, flagged):
    """[(first window, last window)]: the maximal runs of consecutive flagged windows of one chromosome."""
    out, run = [], None
    for w, f in enumerate(np.asarray(flagged, dtype=bool)):
        if f and run is not None and chrom[w] == chrom[run[0]] and run[1] == w - 1:
            run[1] = w
        else:
            if run is not None:
                out.append(tuple(run))
            run = [w, w] if f else None
    if run is not None:
        out.append(tuple(run))
    return out


# ---------------------------------------------------------------- the command's work

def _text(v):
    return repr(float(v))


def localpca(c, P, samples, locs, win, table, out=None, npc=2, m=2, min_sites=None, outlier=3.0, keep_matrix=False,
             keep_components=False, longlat=False, host=False, silence=False, device="cuda:0", sites=None, extra=None,
             batch_bytes=BATCH_BYTES, window=None):
    """The command's work for a count matrix and its windows: returns the summary dict and writes the files when `out` is given.
    locs None: no locations.  sites: the variant index of every column (default 0 .. K - 1).  window: the entries window_unit,
    window_size, window_start, window_step of the summary.  extra: entries appended to the summary (--ld_prune)."""
    c = B.check_counts(c, P)
    N, K = c.shape
    samples = np.asarray(samples).astype(str)
    win = check_windows(win, K)
    W = len(win)
    if not 1 <= npc <= NPC_LIMIT:
        raise ValueError(f"--npc must be 1 .. {NPC_LIMIT}")
    if npc > N - 1:
        raise ValueError(f"--npc {npc} with {N} samples: at most N - 1 components")
    min_sites = max(10, 2 * npc) if min_sites is None else int(min_sites)
    if min_sites < 1 or m < 1 or not (np.isfinite(outlier) and outlier > 0):
        raise ValueError("--min_sites and --mds must be >= 1, --outlier a positive number")
    idx = np.arange(K, dtype=np.int64) if sites is None else np.asarray(sites, dtype=np.int64)
    located = None
    if locs is not None:
        locs = np.asarray(locs, dtype=np.float64).reshape(N, 2)
        located = ~np.isnan(locs).any(axis=1)
    mean, scale, K_used = PCA.site_constants(c, P)
    used = used_sites(scale, win)
    kept = np.flatnonzero(used >= min_sites)
    if len(kept) < 3:
        raise ValueError(f"{len(kept)} of {W} windows hold --min_sites = {min_sites} polymorphic sites: at least 3 are needed")
    if m > len(kept) - 1:
        raise ValueError(f"--mds {m} with {len(kept)} kept windows: at most windows - 1 axes")

    lam, U, share = np.full((W, npc), np.nan), np.zeros((W, N, npc)), np.full((W, npc), np.nan)
    r2 = np.full((W, npc, 2), np.nan)

    def decompose(w, G):
        lam[w], U[w], share[w] = PCA.components(G, int(used[w]), npc)
        if located is not None:
            r2[w] = PCA.pc_r2(PCA.scores(lam[w], U[w]), locs, located)

    if host:
        z = PCA.z_host(c, mean, scale)
        for w in kept:
            v0, v1 = win[w]
            decompose(w, z[:, v0:v1] @ z[:, v0:v1].T)
    else:
        B.require_gpu(PROG, LAUNCH)
        for w0, g in windows_batches(c, mean, scale, win[kept], batch_bytes=batch_bytes, device=device):
            for q in range(len(g)):
                decompose(kept[w0 + q], g[q])

    D = pc_dist(lam[kept], U[kept])
    Y, mds_lam = mds(D, m)
    sc, med, mad = robust_scores(Y)
    flag_kept = (np.abs(sc) > outlier).any(axis=1)
    flagged = np.zeros(W, dtype=bool)
    flagged[kept] = flag_kept
    regions = merge_regions(table["chrom"], flagged)
    coords, score = np.full((W, m), np.nan), np.full((W, m), np.nan)
    coords[kept], score[kept] = Y, sc
    zero_axes = [int(q) + 1 for q in np.flatnonzero(mad == 0)]

    own = {"N": int(N), "n_located": None if located is None else int(located.sum()), "K": int(K), "K_used": int(K_used),
           "P": int(P), "W": int(W), "W_kept": int(len(kept)), "W_skipped": int(W - len(kept)), "npc": int(npc), "mds": int(m),
           "min_sites": int(min_sites), "outlier": float(outlier), "longlat": bool(longlat),
           "mds_eigenvalues": [B.num(v) for v in mds_lam], "median": [B.num(v) for v in med], "mad": [B.num(v) for v in mad],
           "mad_zero_axes": zero_axes, "n_flagged": int(flagged.sum()), "flagged": [int(w) for w in np.flatnonzero(flagged)],
           "n_regions": len(regions),
           **{k: (window or {}).get(k) for k in ("window_unit", "window_size", "window_start", "window_step")}}
    summary = {key: own[key] for key in SUMMARY_KEYS}
    summary.update(extra or {})

    nonempty = win[:, 1] > win[:, 0]
    first_site, last_site = np.full(W, -1, dtype=np.int64), np.full(W, -1, dtype=np.int64)      # -1: an empty window
    first_site[nonempty], last_site[nonempty] = idx[win[nonempty, 0]], idx[win[nonempty, 1] - 1]
    if out is not None:
        head = (["window", "chrom", "start", "stop", "first_site", "last_site", "n_sites", "K_used", "kept"]
                + [f"eigenvalue{q + 1}" for q in range(npc)] + [f"share{q + 1}" for q in range(npc)]
                + [f"mds{q + 1}" for q in range(m)] + [f"score{q + 1}" for q in range(m)] + ["flag"])
        if located is not None:
            head += [f"pc{q + 1}_r2_{ax}" for q in range(npc) for ax in ("x", "y")]
        rows = []
        for w in range(W):
            row = [str(w), str(table["chrom"][w]), str(int(table["start"][w])), str(int(table["stop"][w])), str(int(first_site[w])),
                   str(int(last_site[w])), str(int(win[w, 1] - win[w, 0])), str(int(used[w])), str(int(used[w] >= min_sites))]
            row += [_text(v) for v in lam[w]] + [_text(v) for v in share[w]] + [_text(v) for v in coords[w]]
            row += [_text(v) for v in score[w]] + [str(int(flagged[w]))]
            if located is not None:
                row += [_text(v) for v in r2[w].reshape(-1)]
            rows.append("\t".join(row))
        write_atomic(out + "_localpca_windows.txt", "\t".join(head) + "\n" + "".join(r + "\n" for r in rows))
        rhead = ["region", "chrom", "start", "stop", "first_window", "last_window", "n_windows", "first_site", "last_site",
                 "peak_score"]
        rrows = ["\t".join([str(n), str(table["chrom"][a]), str(int(table["start"][a])), str(int(table["stop"][b])), str(a), str(b),
                            str(b - a + 1), str(int(first_site[a])), str(int(last_site[b])),
                            _text(np.abs(score[a:b + 1]).max())]) for n, (a, b) in enumerate(regions)]
        write_atomic(out + "_localpca_regions.txt", "\t".join(rhead) + "\n" + "".join(r + "\n" for r in rrows))
        write_atomic(out + "_localpca_summary.json", json.dumps(summary, indent=1) + "\n")
        if keep_matrix:
            write_atomic(out + "_localpca_dist.npz", lambda fh: B.save_npz(fh, D=D, windows=kept.astype(np.int64), win=win,
                                                                             mds=Y, mds_eigenvalues=mds_lam), mode="wb")
        if keep_components:
            write_atomic(out + "_localpca_components.npz",
                         lambda fh: B.save_npz(fh, windows=kept.astype(np.int64), win=win, eigenvalues=lam[kept], U=U[kept],
                                               K_used=used[kept].astype(np.int64), samples=samples), mode="wb")
    if not silence:
        print(f"{N} samples, {K} sites ({K_used} polymorphic), ploidy {P}; {W} windows, {len(kept)} kept "
              f"(at least {min_sites} polymorphic sites), {npc} PCs each")
        print("MDS eigenvalues: " + ", ".join(f"{v:.4g}" for v in mds_lam))
        for q in zero_axes:
            print(f"MDS axis {q}: the MAD is 0, nothing is flagged on it")
        print(f"{int(flagged.sum())} windows flagged (|robust score| > {outlier:g}) in {len(regions)} regions")
        for a, b in regions:
            print(f"  {table['chrom'][a]}:{int(table['start'][a])}-{int(table['stop'][b]) - 1} (windows {a}..{b})")
    summary["_D"], summary["_kept"], summary["_mds"], summary["_scores"], summary["_regions"] = D, kept, Y, sc, regions
    summary["_lam"], summary["_U"], summary["_r2"] = lam, U, r2
    return summary


# ---------------------------------------------------------------- command

def _own_arguments(p):
    p.add_argument("--window_snps", default=None, type=int, metavar="S", help="windows of S consecutive filtered sites per chromosome")
    p.add_argument("--window_bp", default=None, type=int, metavar="B",
                   help="windows of B base pairs per chromosome, as a fit's --windows (needs positions: not with --matrix)")
    p.add_argument("--window_start", default=0, type=int, help="first window start: a position, or with --window_snps the number "
                                                               "of leading sites of every chromosome to skip (default 0)")
    p.add_argument("--window_step", default=None, type=int, help="stride of the windows in the unit of their size (default: the "
                                                                 "size; smaller slides them)")
    p.add_argument("--npc", default=2, type=int, help=f"components per window (default 2, at most {NPC_LIMIT} and samples - 1)")
    p.add_argument("--mds", default=2, type=int, help="MDS axes kept and scored (default 2)")
    p.add_argument("--min_sites", default=None, type=int,
                   help="windows with fewer polymorphic sites are skipped (default max(10, 2 npc))")
    p.add_argument("--outlier", default=3.0, type=float, help="a window is flagged when a robust score exceeds this (default 3)")
    p.add_argument("--keep_matrix", default=False, action="store_true", help="keep the window distances in {out}_localpca_dist.npz")
    p.add_argument("--keep_components", default=False, action="store_true",
                   help="keep every window's eigenvalues and eigenvectors in {out}_localpca_components.npz")
    p.add_argument("--longlat", default=False, action="store_true",
                   help="x / y are longitude / latitude degrees (recorded; the per-window correlations do not depend on it)")
    p.add_argument("--batch_bytes", default=BATCH_BYTES, type=int,
                   help="device memory for the window matrices of one launch (default 1 GiB)")
    p.add_argument("--host", default=False, action="store_true",
                   help="the NumPy form in float64 instead of the GPU (the files differ within fp32 arithmetic)")


def build_parser():
    return B.build_parser(PROG, "PCA per window of the genome, window distances, MDS and outlying windows.", _own_arguments,
                          sample_data=False, sample_data_help="tab-separated sampleID, x, y; NaN / NA = not located.  Optional: "
                                                              "with it every window's PCs are correlated with x and y")


def main(argv=None):
    parser = build_parser()
    a = B.parse_args(parser, argv)
    if (a.window_snps is None) == (a.window_bp is None):
        parser.error("exactly one of --window_snps / --window_bp must be given")
    if a.window_bp is not None and a.matrix is not None:
        parser.error("--window_bp needs positions: a --matrix has none (use --window_snps)")
    if not 1 <= a.npc <= NPC_LIMIT:
        parser.error(f"--npc must be 1 .. {NPC_LIMIT}")
    if a.batch_bytes < 1:
        parser.error("--batch_bytes must be >= 1")
    c, P, samples, locs, idx, chrom, pos = B.prelude(parser, a, LAUNCH, sites=True)
    try:
        order = np.argsort(idx, kind="stable")                         # a --max_SNPs draw comes in drawn order
        c, idx = np.ascontiguousarray(c[:, order]), np.asarray(idx)[order]
        chrom, pos = (None if t is None else np.asarray(t)[order] for t in (chrom, pos))
        win, table = window_bounds(chrom, pos, idx, a.window_snps, a.window_bp, a.window_start, a.window_step)
        size = a.window_snps if a.window_bp is None else a.window_bp
        window = {"window_unit": "sites" if a.window_bp is None else "bp", "window_size": int(size),
                  "window_start": int(a.window_start), "window_step": int(size if a.window_step is None else a.window_step)}
        localpca(c, P, samples, locs, win, table, a.out, a.npc, a.mds, a.min_sites, a.outlier, a.keep_matrix, a.keep_components,
                 a.longlat, a.host, a.silence, sites=idx, extra=getattr(a, "ld_summary", None), batch_bytes=a.batch_bytes,
                 window=window)
    except ValueError as e:
        raise SystemExit(f"{PROG}: {e}") from None
    return 0


if __name__ == "__main__":
    sys.exit(main())
