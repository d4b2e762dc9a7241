#!/usr/bin/env python3
"""`python -m locator_amd.pca`: the principal components of the genotypes a fit would train on, and a PC-regression placement
baseline.  The reference README names two ways a fit goes wrong: too little signal (neighbors answers that) and a population
"strongly structured in only one direction", where one coordinate collapses to the mean.  This command shows the second: how
much variance the leading axes hold, which axis carries x and which y, and whether any axis carries one of them at all.

  python -m locator_amd.pca --vcf genotypes.vcf.gz --sample_data samples.txt --out out/test --npc 10

  counts      c [N][K] int8 exactly as the neighbors command takes them (baselines.count_matrix over the sites of
              genotypes.filter_snps with the same --min_mac / --max_SNPs / --seed): -1 = missing, 0 .. P, P = 1 or 2.
  constants   per site over its called entries: p = sum c / (P n_called), mean = P p, scale = 1 / sqrt(P p (1 - p))
              (Patterson's scaling, as smartpca and scikit-allel do), computed in float64 and ROUNDED ONCE TO FLOAT32: the
              two float32 arrays are the kernel's inputs and the host definition uses the same rounded values.  A site with
              no call, p = 0 or p = 1 gets mean = scale = 0, contributes nothing and is not counted in K_used.
  G           z[i][k] = (c[i][k] - mean[k]) scale[k], 0 where the call is missing (MEAN IMPUTATION: a missing call sits at the
              site's mean); G = Z Z'.  `grm_host` is the definition in float64; loc_grm_pairs (include/locator_hip_pca.h)
              forms z in fp32 and sums in fp32 on the matrix pipe.
  components  numpy.linalg.eigh of G / K_used on the host in float64 (N^3 is small next to the N^2 K of G): the npc largest
              eigenvalues, eigenvectors flipped so that the component of largest magnitude is positive, scores
              PC_p = U[:, p] sqrt(max(lambda_p, 0)), variance share lambda_p / trace(G / K_used).
  loadings    with --loadings, T = Z' U32 (U32 = the eigenvectors rounded to float32; loc_pca_loadings or `loadings_host`),
              reported as T[k][p] / sqrt(K_used lambda_p).
  placement   for p = 1 .. pmax = min(npc, n_located - 2): x and y (planar, float64) regressed on an intercept and the first
              p PCs over the located samples by ordinary least squares; located samples are predicted LEAVE-ONE-OUT by the
              hat-matrix identity y_i - r_i / (1 - h_i) (NaN where 1 - h_i < 1e-12), the others from the fit on all located
              samples.  --p auto takes the p with the smallest leave-one-out median error (the smallest such p); errors as
              baselines.errors, --longlat included.
  diagnostics per PC the squared Pearson correlation with x and with y over the located samples.

Outputs: {out}_pca.txt, {out}_pca_eigenvalues.txt, {out}_pca_locs.txt (x,y,sampleID as a predlocs file, but NOT named
predlocs: it is no replicate), {out}_pca_summary.json, with --keep_matrix {out}_grm.npz, with --loadings
{out}_pca_loadings.npz.  --ld_prune R2 (with --ld_window / --ld_window_bp) prunes the sites by linkage disequilibrium first,
as locator_amd.ld does; the summary then also holds ld_prune, ld_window, ld_window_bp and K_before_prune.  There is no silent fallback: without a GPU the run stops and says so; --host asks for the NumPy form.

Unlike neighbors, the device and --host files are NOT byte-identical: the device forms z and sums in fp32, --host in float64.
They differ by at most what fp32 arithmetic allows: with u = 2^-24, every element |G_dev - G_host| <= (K + 8) u sum_k |z_ik|
|z_jk| (z carries 2 u from its subtraction and product, a K-term fp32 sum adds gamma_K; the float64 sum over site groups is
negligible); with E the matrix of those bounds every eigenvalue moves by at most ||E||_F / K_used (Weyl) and the sine of the
angle of eigenvector p by at most 2 ||E||_F / (K_used gap_p) (Davis-Kahan).  Each path is deterministic: two runs of it write
the same bytes.

Not built: --phased and --dosage inputs; projecting the samples of another file onto kept components; a plot;
pairwise-complete normalisation instead of mean imputation; an eigen-solver on the device.  The components of single
windows of the genome and how they differ along it: locator_amd.localpca.
"""
from __future__ import annotations

import json
import sys

import numpy as np

from . import _abi
from . import baselines as B
from ._files import write_atomic

TILE = _abi.LOC_PCA_TILE
BLOCK = _abi.LOC_PCA_BLOCK
NPC_LIMIT = _abi.LOC_PCA_MAX_NPC
PROG = "locator_amd.pca"
LAUNCH = "the relationship matrix is one loc_grm_pairs launch"
NOTHING_TO_CHOOSE_BY = "no located sample has a leave-one-out prediction: nothing to choose p by"
# the key order of {out}_pca_summary.json
SUMMARY_KEYS = ("N", "n_located", "K", "K_used", "P", "npc", "pmax", "p", "p_auto", "p_chosen_by", "error_unit", "median_error_by_p",
                "r2_x", "r2_y", "mean_error", "median_error", "eigenvalues", "variance_share", "pc_r2_x", "pc_r2_y")


# ---------------------------------------------------------------- the definitions

def site_constants(c, P):
    """(mean float32 [K], scale float32 [K], K_used): per site over its called entries p = sum c / (P n_called), mean = P p,
    scale = 1 / sqrt(P p (1 - p)), float64 rounded once to float32; mean = scale = 0 for a site with no call, p = 0 or p = 1,
    which K_used does not count."""
    c = B.check_counts(c, P)
    called = c >= 0
    n = called.sum(axis=0, dtype=np.int64)
    s = np.where(called, c, 0).sum(axis=0, dtype=np.int64)
    used = (n > 0) & (s > 0) & (s < P * n)
    p = np.zeros(c.shape[1], dtype=np.float64)
    np.divide(s.astype(np.float64), (P * n).astype(np.float64), out=p, where=used)
    mean = np.where(used, P * p, 0.0)
    scale = np.zeros_like(p)
    np.divide(1.0, np.sqrt(P * p * (1.0 - p)), out=scale, where=used)
    return mean.astype(np.float32), scale.astype(np.float32), int(used.sum())


def z_host(c, mean, scale):
    """z [N][K] float64 = (c - mean) scale with the given (float32) constants, 0 where c < 0: mean imputation."""
    c = np.asarray(c)
    z = (c.astype(np.float64) - np.asarray(mean, dtype=np.float64)[None]) * np.asarray(scale, dtype=np.float64)[None]
    z[c < 0] = 0.0
    return z


def grm_host(c, mean, scale):
    """G = Z Z' in float64, [N][N]: the definition.  A missing call contributes 0, i.e. it is imputed as the site's mean."""
    z = z_host(c, mean, scale)
    return z @ z.T


def components(G, K_used, npc):
    """(lam [npc], U [N][npc], share [npc]): the npc largest eigenvalues of G / K_used in descending order, their eigenvectors,
    each flipped so that its component of largest magnitude (the lowest index on a tie) is positive, and lam / trace."""
    G = np.asarray(G, dtype=np.float64)
    N = len(G)
    if npc < 1 or npc > NPC_LIMIT:
        raise ValueError(f"npc = {npc}: must be 1 .. {NPC_LIMIT}")
    if npc > N - 1:
        raise ValueError(f"npc = {npc} with {N} samples: at most N - 1 = {N - 1} components")
    if K_used < 1:
        raise ValueError("no polymorphic site: nothing to decompose")
    A = G / float(K_used)
    lam, U = np.linalg.eigh(A)
    lam, U = lam[::-1][:npc].copy(), U[:, ::-1][:, :npc].copy()
    big = np.argmax(np.abs(U), axis=0)
    U *= np.where(U[big, np.arange(npc)] < 0, -1.0, 1.0)[None]
    return lam, U, lam / np.trace(A)


def scores(lam, U):
    """PC_p = U[:, p] sqrt(max(lam_p, 0))."""
    return U * np.sqrt(np.maximum(lam, 0.0))[None]


def loadings_host(c, mean, scale, U32):
    """T [K][npc] float64 = Z' U32 with U32 the eigenvectors as float32."""
    return z_host(c, mean, scale).T @ np.asarray(U32, dtype=np.float32).astype(np.float64)


def report_loadings(T, K_used, lam):
    """T[k][p] / sqrt(K_used lam_p) in float64; NaN for an eigenvalue that is not positive."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.asarray(T, dtype=np.float64) / np.sqrt(K_used * np.where(lam > 0, lam, np.nan))[None]


# ---------------------------------------------------------------- the device forms

def _upload(c, mean, scale, pitch=None, pad_fill=-1, device="cuda:0"):
    import torch
    from . import _device as D
    buf = B.padded(c, pitch, pad_fill)
    with torch.cuda.device(device):
        return D.put(buf, np.int8, device), D.put(mean, np.float32, device), D.put(scale, np.float32, device), int(buf.shape[1])


def grm_device(c, mean, scale, k_groups=0, pitch=None, pad_fill=-1, device="cuda:0", work_fill=None, on_device=None):
    """grm_host's matrix from one loc_grm_pairs launch, float64 [N][N].  work_fill: a float32 bit pattern the scratch holds
    before the launch (tests); on_device: the tensors of _upload, to share them with loadings_device."""
    import torch
    from . import _device as D, _lib
    lib = _lib.load()
    c = np.ascontiguousarray(c, dtype=np.int8)
    N, K = c.shape
    d_c, d_mean, d_scale, pitch = on_device or _upload(c, mean, scale, pitch, pad_fill, device)
    with torch.cuda.device(device):
        d_g = torch.empty((max(N, 1), max(N, 1)), dtype=torch.float64, device=device)
        work, work_bytes = D.work_buffer(lib, "loc_grm_work_bytes", N, K, int(k_groups), device=device, fill=work_fill)
        _lib.check(lib.loc_grm_pairs(d_c.data_ptr(), N, K, pitch, d_mean.data_ptr(), d_scale.data_ptr(), int(k_groups),
                                     d_g.data_ptr(), work.data_ptr(), work_bytes, D.stream()), "loc_grm_pairs")
        return d_g.cpu().numpy()[:N, :N]


def loadings_device(c, mean, scale, U32, pitch=None, pad_fill=-1, device="cuda:0", on_device=None):
    """loadings_host's matrix from one loc_pca_loadings launch, float32 [K][npc]."""
    import torch
    from . import _device as D, _lib
    lib = _lib.load()
    c = np.ascontiguousarray(c, dtype=np.int8)
    N, K = c.shape
    U32 = np.ascontiguousarray(U32, dtype=np.float32).reshape(N, -1)
    npc = U32.shape[1]
    d_c, d_mean, d_scale, pitch = on_device or _upload(c, mean, scale, pitch, pad_fill, device)
    with torch.cuda.device(device):
        d_u = D.put(U32, np.float32, device)
        d_t = torch.empty((max(K, 1), npc), dtype=torch.float32, device=device)
        _lib.check(lib.loc_pca_loadings(d_c.data_ptr(), N, K, pitch, d_mean.data_ptr(), d_scale.data_ptr(), d_u.data_ptr(), npc,
                                        d_t.data_ptr(), D.stream()), "loc_pca_loadings")
        return d_t.cpu().numpy()[:K]


# ---------------------------------------------------------------- placement

def _design(pcs, rows, p):
    return np.concatenate([np.ones((len(rows), 1)), pcs[rows][:, :p]], axis=1)


def placements(pcs, locs, located, pmax):
    """[pmax][N][2]: for p = 1 .. pmax, x and y regressed on an intercept and the first p PCs over the located samples
    (ordinary least squares, float64).  A located sample gets its leave-one-out prediction by the hat-matrix identity
    y_i - r_i / (1 - h_i), NaN where 1 - h_i < 1e-12; an unlocated one the prediction of the fit on all located samples."""
    pcs = np.asarray(pcs, dtype=np.float64)
    locs = np.asarray(locs, dtype=np.float64)
    li, ui = np.flatnonzero(located), np.flatnonzero(~np.asarray(located))
    y = locs[li]
    out = np.full((pmax, len(pcs), 2), np.nan)
    for p in range(1, pmax + 1):
        X = _design(pcs, li, p)
        Q, s, Vt = np.linalg.svd(X, full_matrices=False)
        keep = s > s[0] * max(X.shape) * np.finfo(np.float64).eps
        Q = Q[:, keep]
        coef = Q.T @ y                                               # the fit in the basis of X's column space
        r = y - Q @ coef
        one_h = 1.0 - (Q * Q).sum(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            loo = y - r / one_h[:, None]
        loo[one_h < 1e-12] = np.nan
        out[p - 1, li] = loo
        if len(ui):
            beta = (Vt[keep].T / s[keep][None]) @ coef
            out[p - 1, ui] = _design(pcs, ui, p) @ beta
    return out


def placements_refit(pcs, locs, located, pmax):
    """placements() the slow way, for the tests: every located sample really is left out and the regression refitted."""
    pcs = np.asarray(pcs, dtype=np.float64)
    locs = np.asarray(locs, dtype=np.float64)
    li, ui = np.flatnonzero(located), np.flatnonzero(~np.asarray(located))
    out = np.full((pmax, len(pcs), 2), np.nan)
    for p in range(1, pmax + 1):
        for i in li:
            rest = li[li != i]
            beta = np.linalg.lstsq(_design(pcs, rest, p), locs[rest], rcond=None)[0]
            out[p - 1, i] = _design(pcs, np.array([i]), p)[0] @ beta
        if len(ui):
            beta = np.linalg.lstsq(_design(pcs, li, p), locs[li], rcond=None)[0]
            out[p - 1, ui] = _design(pcs, ui, p) @ beta
    return out


def pc_r2(pcs, locs, located):
    """[npc][2]: the squared Pearson correlation of every PC with x and with y over the located samples."""
    return np.array([[B.r2(pcs[located, q], locs[located, a]) for a in (0, 1)] for q in range(pcs.shape[1])])


# ---------------------------------------------------------------- the command's work

def pca(c, P, samples, locs, out=None, npc=10, p="auto", longlat=False, loadings=False, keep_matrix=False, host=False,
        silence=False, device="cuda:0", sites=None, extra=None):
    """The command's work for a count matrix: returns the summary dict and writes the output files when `out` is given.
    extra: entries appended to the summary (--ld_prune: what baselines.prelude recorded)."""
    import pandas as pd
    c = B.check_counts(c, P)
    N, K = c.shape
    samples = np.asarray(samples).astype(str)
    locs = np.asarray(locs, dtype=np.float64).reshape(N, 2)
    located = ~np.isnan(locs).any(axis=1)
    if not 1 <= npc <= NPC_LIMIT:
        raise SystemExit(f"locator_amd.pca: --npc must be 1 .. {NPC_LIMIT}")
    if npc > N - 1:
        raise SystemExit(f"locator_amd.pca: --npc {npc} with {N} samples: at most N - 1 components")
    pmax = min(npc, int(located.sum()) - 2)
    if pmax < 1:
        raise SystemExit("locator_amd.pca: fewer than 3 samples of --sample_data have a location: nothing to regress on")
    if p != "auto" and not 1 <= int(p) <= pmax:
        raise SystemExit(f"locator_amd.pca: --p must be `auto` or 1 .. min(--npc, located samples - 2) = {pmax}")
    mean, scale, K_used = site_constants(c, P)
    on_device = None
    if host:
        G = grm_host(c, mean, scale)
    else:
        B.require_gpu(PROG, LAUNCH)
        on_device = _upload(c, mean, scale, device=device)
        G = grm_device(c, mean, scale, device=device, on_device=on_device)      # downloaded once: the rest is host float64
    lam, U, share = components(G, K_used, npc)
    pcs = scores(lam, U)
    r2pc = pc_r2(pcs, locs, located)

    placed = placements(pcs, locs, located, pmax)
    p_auto, med = B.choose_smallest_median(placed, locs, located, longlat, NOTHING_TO_CHOOSE_BY)
    p_used = p_auto if p == "auto" else int(p)
    xy = placed[p_used - 1]
    shared, shared_lines = B.placement_summary(c, P, located, xy, locs, longlat, "PC-regression")
    own = {"K_used": int(K_used), "npc": int(npc), "pmax": int(pmax), "p": int(p_used), "p_auto": int(p_auto),
           "p_chosen_by": "auto" if p == "auto" else "--p", "median_error_by_p": [B.num(v) for v in med],
           "eigenvalues": [B.num(v) for v in lam], "variance_share": [B.num(v) for v in share],
           "pc_r2_x": [B.num(v) for v in r2pc[:, 0]], "pc_r2_y": [B.num(v) for v in r2pc[:, 1]]}
    summary = {key: {**shared, **own}[key] for key in SUMMARY_KEYS}
    summary.update(extra or {})

    T = None
    if loadings:
        U32 = U.astype(np.float32)
        T = loadings_host(c, mean, scale, U32) if host else loadings_device(c, mean, scale, U32, device=device, on_device=on_device)
        T = report_loadings(T, K_used, lam)

    lead = min(npc, 4)
    best = [int(np.nanargmax(r2pc[:, a])) if not np.isnan(r2pc[:, a]).all() else 0 for a in (0, 1)]
    lines = [f"{N} samples ({int(located.sum())} located), {K} sites ({K_used} polymorphic), ploidy {P}",
             "variance share of PC1.." + str(lead) + ": " + ", ".join(f"{v:.4f}" for v in share[:lead])
             + " (eigenvalues " + ", ".join(f"{v:.4g}" for v in lam[:lead]) + ")",
             f"x is carried by PC{best[0] + 1} (R2 {r2pc[best[0], 0]:.3f}), y by PC{best[1] + 1} (R2 {r2pc[best[1], 1]:.3f}) "
             f"among the first {npc} PCs",
             f"p = {p_used} ({summary['p_chosen_by']}; leave-one-out median error by p, p = 1 .. {pmax}, smallest at p = {p_auto})",
             *shared_lines]
    if out is not None:
        write_atomic(out + "_pca.txt", "sampleID\t" + "\t".join(f"PC{q + 1}" for q in range(npc)) + "\n" + "".join(
            f"{samples[i]}\t" + "\t".join(repr(float(v)) for v in pcs[i]) + "\n" for i in range(N)))
        write_atomic(out + "_pca_eigenvalues.txt", "PC\teigenvalue\tvariance_share\tr2_x\tr2_y\n" + "".join(
            f"{q + 1}\t{float(lam[q])!r}\t{float(share[q])!r}\t{float(r2pc[q, 0])!r}\t{float(r2pc[q, 1])!r}\n" for q in range(npc)))
        frame = pd.DataFrame({"x": xy[:, 0], "y": xy[:, 1], "sampleID": samples.astype(object)})
        write_atomic(out + "_pca_locs.txt", lambda fh: frame.to_csv(fh, index=False))
        write_atomic(out + "_pca_summary.json", json.dumps(summary, indent=1) + "\n")
        if keep_matrix:
            write_atomic(out + "_grm.npz", lambda fh: B.save_npz(fh, G=G, K_used=np.int64(K_used), samples=samples), mode="wb")
        if T is not None:
            idx = np.arange(K, dtype=np.int64) if sites is None else np.asarray(sites, dtype=np.int64)
            write_atomic(out + "_pca_loadings.npz", lambda fh: B.save_npz(fh, sites=idx, mean=mean, scale=scale, loadings=T),
                      mode="wb")
    if not silence:
        for line in lines:
            print(line)
    summary["_G"], summary["_pcs"], summary["_xy"], summary["_loadings"] = G, pcs, xy, T
    return summary


# ---------------------------------------------------------------- command

def _own_arguments(p):
    p.add_argument("--npc", default=10, type=int, help=f"components kept (default 10, at most {NPC_LIMIT} and samples - 1)")
    p.add_argument("--p", default="auto", help="PCs regressed on: a number, or `auto` (default): the p in 1 .. min(--npc, "
                                               "located samples - 2) with the smallest leave-one-out median error")
    p.add_argument("--longlat", default=False, action="store_true",
                   help="x / y are longitude / latitude degrees: errors are great-circle km (the regression stays planar)")
    p.add_argument("--loadings", default=False, action="store_true", help="also write the site loadings to {out}_pca_loadings.npz")
    p.add_argument("--keep_matrix", default=False, action="store_true", help="keep G, K_used and the sample IDs in {out}_grm.npz")
    p.add_argument("--host", default=False, action="store_true",
                   help="the NumPy form in float64 instead of the GPU (the files differ within the fp32 bounds of the module text)")


def build_parser():
    return B.build_parser(PROG, "Principal components of the genotypes and a PC-regression placement baseline.", _own_arguments)


def main(argv=None):
    parser = build_parser()
    a = B.parse_args(parser, argv)
    if a.p != "auto":
        try:
            a.p = int(a.p)
        except ValueError:
            parser.error("--p must be `auto` or a whole number")
        if a.p < 1:
            parser.error("--p must be `auto` or a whole number >= 1")
    if not 1 <= a.npc <= NPC_LIMIT:
        parser.error(f"--npc must be 1 .. {NPC_LIMIT}")
    c, P, samples, locs, idx = B.prelude(parser, a, LAUNCH)
    try:
        pca(c, P, samples, locs, a.out, a.npc, a.p, a.longlat, a.loadings, a.keep_matrix, a.host, a.silence, sites=idx,
            extra=getattr(a, "ld_summary", None))
    except ValueError as e:
        raise SystemExit(f"{PROG}: {e}") from None
    return 0


if __name__ == "__main__":
    sys.exit(main())
