#!/usr/bin/env python3
"""`python -m locator_amd.spa`: the model-based placement baseline.  Every site gets a logistic allele-frequency surface over the
map (a spatial allele-frequency model of the SPA kind, Yang et al. 2012), fitted to the located samples; a sample is placed at
the maximum of its genotype likelihood over a grid.  Unlike kNN (neighbors) and PC regression (pca) it also says which sites
carry the gradient: {out}_spa_sites.txt lists every site's slope.

  python -m locator_amd.spa --vcf genotypes.vcf.gz --sample_data samples.txt --out out/test

  counts      c [N][K] int8 exactly as the neighbors and pca commands take them (baselines.prelude): -1 = missing, 0 .. P; the
              site-major copy ct [K][N] holds the same values (what baselines.count_matrix_sites builds).
  coordinates normalised over the located samples per axis, (loc - mean) / sd with the population sd, an axis with sd 0 is
              refused; ROUNDED ONCE TO FLOAT32, both paths use the rounded values.  The model is planar, also with --longlat:
              only the error is then great-circle km (baselines.errors).
  fit         `fit_host`: per site k over the samples with w[i] = 1 and c >= 0, c_i ~ Binomial(P, f_i), f_i = sigmoid(t_i),
              t_i = ax x_i + ay y_i + b; maximise sum_i [c_i t_i - P softplus(t_i)] - ridge (ax^2 + ay^2) / 2 (no penalty on b)
              from ax = ay = 0, b = logit(sum c / (P n)) by exactly --iters Newton steps on the 3 x 3 system, every component
              of a step clamped to +- 2 (LOC_SPA_MAX_STEP); no data-dependent branch or exit.  A site with no called sample
              in w, sum c = 0 or sum c = P n is UNUSED: parameters 0, used = 0, it contributes nothing anywhere.
              theta [K][4] float32 = ax, ay, b, last_step (the largest absolute component of the final step); used [K] uint8.
  grid        n x n nodes (--grid) over the bounding box of the located samples in normalised units, padded by --pad of the
              span on each side; node coordinates float32, node g = iy n + ix.
  likelihood  `grid_host`: t[k][g] = fl(fl(fl(ax gx) + fl(ay gy)) + b), three correctly rounded fp32 operations;
              ll[q][g] = sum_k used_k [c_qk >= 0] (c_qk t - P softplus(t)), softplus and the sum in float64 from the fp32 t.
  placement   `peaks`: the node of largest ll (the lowest index on a tie), refined per axis by the vertex of the parabola
              through the node and its two neighbours on that axis (not on a border node, not where the second difference is
              not negative), transformed back to map units; NaN for a sample with no called used site.
  folds       the r-th located sample in index order belongs to fold r mod F (--folds; no draw); each located sample is placed
              by the fit that excludes its fold, unlocated samples by one more fit on all located samples, which also
              produces the site table.

Outputs: {out}_spa_locs.txt (x,y,sampleID as {out}_knn_locs.txt), {out}_spa_sites.txt (variant used ax ay b slope, slope =
hypot(ax, ay), from the all-located fit), {out}_spa_summary.json, with --keep_surfaces {out}_spa.npz (theta per fold, used, the
grid).  --ld_prune as in the other baselines.  Without a GPU the run stops and says so; --host asks for the NumPy form.

The device fits in fp32 (loc_spa_fit) and sums the likelihood in fp32 on the matrix pipe (loc_spa_grid), --host in float64:
as with pca the files of the two paths are not byte-identical.  With u = 2^-24, B the sites one group sums and eps = 5 (expf and
log1pf are documented at 1 ulp = 2 u each, and the sum max(t, 0) + log1pf(.) adds one rounding; the argument error of log1pf
is not amplified, since e / ((1 + e) log1p(e)) <= 1): every element |ll_dev - ll_host| <= (B + 8) u sum_k (|c t| + |P m sp|)
+ eps u sum_k P m sp (`ll_bound`).  Each path is deterministic: two runs of it write the same bytes.

Deviations chosen here: allele 1 rather than the minor allele; a partly missing call counts as missing; the
ridge; the fixed step count; the grid with parabola refinement instead of a continuous optimiser.  Not built: --phased and
--dosage inputs, leave-one-out, a selection scan.
"""
from __future__ import annotations

import json
import sys

import numpy as np

from . import _abi
from . import baselines as B
from ._files import write_atomic

TILE = _abi.LOC_SPA_TILE
TILE_SAMPLES = _abi.LOC_SPA_TILE_SAMPLES
BLOCK = _abi.LOC_SPA_BLOCK
MAX_STEP = _abi.LOC_SPA_MAX_STEP
MAX_ITERS = _abi.LOC_SPA_MAX_ITERS
MAX_NODES = _abi.LOC_SPA_MAX_NODES
FIT_CHUNK = _abi.LOC_SPA_FIT_CHUNK
GRID_RANGE = (8, 128)
TINY = 1e-30                                     # floor of a pivot of the 3 x 3 elimination
U24 = 2.0 ** -24                                 # the unit roundoff of fp32
SOFTPLUS_EPS = 5.0                               # error of the device softplus in units of u: 2 (expf) + 2 (log1pf) + 1 (the sum)
PROG = "locator_amd.spa"
LAUNCH = "the surfaces are loc_spa_fit launches, the likelihood grids loc_spa_grid launches"
# the key order of {out}_spa_summary.json
SUMMARY_KEYS = ("N", "n_located", "K", "K_used", "P", "folds", "grid", "pad", "ridge", "iters", "error_unit", "r2_x", "r2_y",
                "mean_error", "median_error", "max_last_step", "n_border", "n_unplaced")


# ---------------------------------------------------------------- the definitions

def normalise(locs, located):
    """(xy float32 [N][2], mean [2], sd [2]): (loc - mean) / sd over the located samples per axis (population sd), rounded once
    to float32; 0 for a sample without a location (never read: w is 0 there).  An axis with sd 0 is refused."""
    locs = np.asarray(locs, dtype=np.float64)
    mean, sd = locs[located].mean(axis=0), locs[located].std(axis=0)
    if not (sd > 0).all():
        raise ValueError("the located samples do not spread over both axes (sd 0): no surface to fit")
    xy = np.zeros(locs.shape, dtype=np.float32)
    xy[located] = ((locs[located] - mean[None]) / sd[None]).astype(np.float32)
    return xy, mean, sd


def check_sites(ct, P):
    """ct as an int8 [K][N] array of counts -1 (any negative), 0 .. P."""
    ct = np.asarray(ct)
    if ct.ndim != 2:
        raise ValueError(f"count matrix of shape {ct.shape}: needs [sites][samples]")
    return np.ascontiguousarray(B.check_counts(ct.T, P).T)


def fit_host(ct, P, xy, w, ridge, iters, dtype=np.float64):
    """(theta float32 [K][4], used uint8 [K]) of the site-major counts ct [K][N]: the definition in the module text.  dtype
    float32 runs the same algorithm with every operation in float32 (what the device's tolerance is measured from)."""
    theta, used = fit_state(ct, P, xy, w, ridge, iters, dtype)
    return np.ascontiguousarray(theta, dtype=np.float32), used


def fit_state(ct, P, xy, w, ridge, iters, dtype=np.float64):
    """fit_host before theta is rounded to float32: (theta `dtype` [K][4], used uint8 [K])."""
    ct = check_sites(ct, P)
    K, N = ct.shape
    f = np.dtype(dtype).type
    if not 1 <= iters <= MAX_ITERS:
        raise ValueError(f"iters = {iters}: must be 1 .. {MAX_ITERS}")
    if not (np.isfinite(ridge) and ridge >= 0):
        raise ValueError(f"ridge = {ridge}: must be finite and >= 0")
    on = (ct >= 0) & (np.asarray(w).reshape(1, N) == 1)
    xy = np.asarray(xy, dtype=np.float32).reshape(N, 2)
    x = np.where(on, xy[None, :, 0], np.float32(0)).astype(dtype)
    y = np.where(on, xy[None, :, 1], np.float32(0)).astype(dtype)
    cv = np.where(on, ct, 0)
    n, s = on.sum(axis=1, dtype=np.int64), cv.sum(axis=1, dtype=np.int64)
    used = (n > 0) & (s > 0) & (s < P * n)
    cf, fP, rdg = cv.astype(dtype), f(P), f(ridge)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ax, ay = np.zeros(K, dtype=dtype), np.zeros(K, dtype=dtype)
        b = np.where(used, np.log(s.astype(dtype)) - np.log((P * n - s).astype(dtype)), f(0)).astype(dtype)
        last = np.zeros(K, dtype=dtype)
        tiny, lim = f(TINY), f(MAX_STEP)
        for _ in range(iters):
            t = (ax[:, None] * x + ay[:, None] * y) + b[:, None]
            p = f(1) / (f(1) + np.exp(-t))
            r = np.where(on, cf - fP * p, f(0))
            v = np.where(on, (fP * p) * (f(1) - p), f(0))
            vx, vy = v * x, v * y
            g1 = (r * x).sum(axis=1, dtype=dtype) - rdg * ax
            g2 = (r * y).sum(axis=1, dtype=dtype) - rdg * ay
            g3 = r.sum(axis=1, dtype=dtype)
            h11 = (vx * x).sum(axis=1, dtype=dtype) + rdg
            h12 = (vx * y).sum(axis=1, dtype=dtype)
            h13 = vx.sum(axis=1, dtype=dtype)
            h22 = (vy * y).sum(axis=1, dtype=dtype) + rdg
            h23 = vy.sum(axis=1, dtype=dtype)
            h33 = v.sum(axis=1, dtype=dtype)
            d1 = np.maximum(h11, tiny)                                   # L D L' without pivoting, pivots floored
            l21, l31 = h12 / d1, h13 / d1
            d2 = np.maximum(h22 - l21 * h12, tiny)
            l32 = (h23 - l31 * h12) / d2
            d3 = np.maximum((h33 - l31 * h13) - l32 * (l32 * d2), tiny)
            z1 = g1
            z2 = g2 - l21 * z1
            z3 = (g3 - l31 * z1) - l32 * z2
            s3 = z3 / d3
            s2 = z2 / d2 - l32 * s3
            s1 = (z1 / d1 - l21 * s2) - l31 * s3
            s1, s2, s3 = (np.minimum(np.maximum(q, -lim), lim) for q in (s1, s2, s3))
            ax, ay, b = ax + s1, ay + s2, b + s3
            last = np.maximum(np.maximum(np.abs(s1), np.abs(s2)), np.abs(s3))
    theta = np.stack([ax, ay, b, last], axis=1)
    theta[~used] = 0
    return theta, used.astype(np.uint8)


def objective_gradient(ct, P, xy, w, ridge, theta):
    """The float64 gradient [K][3] of the stated objective at theta[:, :3] (tests: it vanishes at the solution)."""
    ct = check_sites(ct, P)
    on = (ct >= 0) & (np.asarray(w).reshape(1, -1) == 1)
    xy = np.asarray(xy, dtype=np.float32).astype(np.float64)
    th = np.asarray(theta, dtype=np.float64)
    t = th[:, :1] * xy[None, :, 0] + th[:, 1:2] * xy[None, :, 1] + th[:, 2:3]
    r = np.where(on, ct - P / (1.0 + np.exp(-t)), 0.0)
    return np.stack([(r * np.where(on, xy[None, :, 0], 0.0)).sum(axis=1) - ridge * th[:, 0],
                     (r * np.where(on, xy[None, :, 1], 0.0)).sum(axis=1) - ridge * th[:, 1], r.sum(axis=1)], axis=1)


def grid_nodes(xy, located, n, pad):
    """(xs float32 [n], ys float32 [n]): n nodes per axis over the bounding box of the located samples' normalised coordinates,
    padded by `pad` of the span on each side."""
    if not GRID_RANGE[0] <= n <= GRID_RANGE[1]:
        raise ValueError(f"grid = {n}: must be {GRID_RANGE[0]} .. {GRID_RANGE[1]}")
    if not (np.isfinite(pad) and pad >= 0):
        raise ValueError(f"pad = {pad}: must be finite and >= 0")
    at = np.asarray(xy, dtype=np.float64)[located]
    lo, hi = at.min(axis=0), at.max(axis=0)
    lo, hi = lo - pad * (hi - lo), hi + pad * (hi - lo)
    steps = np.arange(n, dtype=np.float64) / (n - 1)
    return ((lo[0] + (hi[0] - lo[0]) * steps).astype(np.float32), (lo[1] + (hi[1] - lo[1]) * steps).astype(np.float32))


def flat_nodes(xs, ys):
    """(gx, gy) float32 [n n] of node g = iy n + ix."""
    n = len(xs)
    return np.tile(np.asarray(xs, dtype=np.float32), n), np.repeat(np.asarray(ys, dtype=np.float32), n)


def surface(theta, gx, gy):
    """t float32 [K][G] = fl(fl(fl(ax gx) + fl(ay gy)) + b): NumPy float32 rounds each operation as the device does."""
    th = np.asarray(theta, dtype=np.float32)
    gx, gy = np.asarray(gx, dtype=np.float32), np.asarray(gy, dtype=np.float32)
    return (th[:, 0:1] * gx[None] + th[:, 1:2] * gy[None]) + th[:, 2:3]


def softplus64(t):
    t = np.asarray(t, dtype=np.float64)
    return np.maximum(t, 0.0) + np.log1p(np.exp(-np.abs(t)))


def _grid_sums(c, P, theta, used, gx, gy, chunk):
    """(sum_k a t - P m sp, sum_k |a t| + |P m sp|, sum_k P m sp) in float64 [Q][G], `chunk` sites at a time."""
    c = B.check_counts(c, P)
    Q, K = c.shape
    G = len(gx)
    ll, mag, sps = np.zeros((Q, G)), np.zeros((Q, G)), np.zeros((Q, G))
    on = np.asarray(used).astype(bool)
    for k0 in range(0, K, chunk):
        k1 = min(K, k0 + chunk)
        t = surface(theta[k0:k1], gx, gy).astype(np.float64)
        sp = softplus64(t)
        live = on[k0:k1][None]
        a = np.where(live, np.maximum(c[:, k0:k1], 0), 0).astype(np.float64)
        m = (P * (live & (c[:, k0:k1] >= 0))).astype(np.float64)
        lin, pen = a @ t, m @ sp
        ll += lin - pen
        mag += a @ np.abs(t) + pen
        sps += pen
    return ll, mag, sps


def grid_host(c, P, theta, used, gx, gy, chunk=512):
    """ll float64 [Q][G]: the definition in the module text.  Missing calls and unused sites contribute exactly 0."""
    return _grid_sums(c, P, theta, used, gx, gy, chunk)[0]


def ll_bound(c, P, theta, used, gx, gy, sites_per_group, chunk=512):
    """The element bound of a device ll whose groups sum at most `sites_per_group` sites each (module text)."""
    _, mag, sps = _grid_sums(c, P, theta, used, gx, gy, chunk)
    return (sites_per_group + 8) * U24 * mag + SOFTPLUS_EPS * U24 * sps


def sites_per_group(K, k_groups):
    """The largest number of sites one group of a loc_spa_grid launch sums when it is asked for k_groups >= 1 groups."""
    nblocks = (K + BLOCK - 1) // BLOCK
    want = max(1, min(int(k_groups), nblocks))
    return min(K, BLOCK * ((nblocks + want - 1) // want)) if nblocks else 0


def peaks(ll, xs, ys, placed=None):
    """(xy float64 [Q][2] in the grid's units, node int64 [Q], border bool [Q]) of ll [Q][n n]: the node of largest ll (lowest
    index on a tie), refined per axis by the vertex of the parabola through the node and its two neighbours on that axis: no
    refinement on a border node of that axis or where the second difference is not negative.  placed False: NaN."""
    ll = np.asarray(ll, dtype=np.float64)
    xs, ys = np.asarray(xs, dtype=np.float32).astype(np.float64), np.asarray(ys, dtype=np.float32).astype(np.float64)
    n, Q = len(xs), len(ll)
    surf = ll.reshape(Q, n, n)
    node = np.argmax(ll, axis=1) if Q else np.zeros(0, dtype=np.int64)
    iy, ix = node // n, node % n
    out = np.stack([xs[ix], ys[iy]], axis=1) if Q else np.zeros((0, 2))
    rows = np.arange(Q)
    for axis, (i, coords) in enumerate(((ix, xs), (iy, ys))):
        inner = (i > 0) & (i < n - 1)
        lo, hi = np.clip(i - 1, 0, n - 1), np.clip(i + 1, 0, n - 1)
        mid = surf[rows, iy, ix]
        left = surf[rows, iy, lo] if axis == 0 else surf[rows, lo, ix]
        right = surf[rows, iy, hi] if axis == 0 else surf[rows, hi, ix]
        d2 = (left - mid) + (right - mid)
        ok = inner & (d2 < 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            off = np.where(ok, 0.5 * (left - right) / d2, 0.0)
        step = (coords[-1] - coords[0]) / (n - 1)
        out[:, axis] += off * step
    border = (ix == 0) | (ix == n - 1) | (iy == 0) | (iy == n - 1)
    if placed is not None:
        placed = np.asarray(placed, dtype=bool)
        out[~placed] = np.nan
        border = border & placed
    return out, node.astype(np.int64), border


def fold_of(located, folds):
    """int64 [N]: fold r mod F of the r-th located sample in index order, -1 for a sample without a location."""
    located = np.asarray(located, dtype=bool)
    fold = np.full(len(located), -1, dtype=np.int64)
    fold[located] = np.arange(int(located.sum())) % folds
    return fold


# ---------------------------------------------------------------- the device forms

def fit_device(ct, P, xy, w, ridge, iters, pitch=None, pad_fill=-1, device="cuda:0", on_device=None):
    """fit_host's answer from one loc_spa_fit launch.  on_device: (tensor of the padded ct, pitch), to share an upload."""
    import torch
    from . import _device as D, _lib
    lib = _lib.load()
    ct = np.ascontiguousarray(ct, dtype=np.int8)
    K, N = ct.shape
    with torch.cuda.device(device):
        if on_device is None:
            buf = B.padded(ct, pitch, pad_fill)
            on_device = (D.put(buf, np.int8, device), int(buf.shape[1]))
        d_ct, pitch = on_device
        d_xy, d_w = D.put(np.reshape(xy, (N, 2)), np.float32, device), D.put(np.reshape(w, N), np.uint8, device)
        d_theta = torch.full((max(K, 1), 4), float("nan"), dtype=torch.float32, device=device)
        d_used = torch.full((max(K, 1),), 255, dtype=torch.uint8, device=device)
        _lib.check(lib.loc_spa_fit(d_ct.data_ptr(), K, N, pitch, int(P), d_xy.data_ptr(), d_w.data_ptr(), float(ridge), int(iters),
                                   d_theta.data_ptr(), d_used.data_ptr(), D.stream()), "loc_spa_fit")
        return d_theta.cpu().numpy()[:K], d_used.cpu().numpy()[:K]


def grid_device(c, P, theta, used, gx, gy, k_groups=0, pitch=None, pad_fill=-1, device="cuda:0", fill=None, on_device=None):
    """grid_host's matrix from one loc_spa_grid launch, float64 [Q][G].  fill: a float32 bit pattern that scratch and (twice,
    as a float64) ll hold before the launch (tests); on_device: (tensor of the padded c, pitch)."""
    import torch
    from . import _device as D, _lib
    lib = _lib.load()
    c = np.ascontiguousarray(c, dtype=np.int8)
    Q, K = c.shape
    G = len(gx)
    with torch.cuda.device(device):
        if on_device is None:
            buf = B.padded(c, pitch, pad_fill)
            on_device = (D.put(buf, np.int8, device), int(buf.shape[1]))
        d_c, pitch = on_device
        d_theta, d_used = D.put(np.reshape(theta, (K, 4)), np.float32, device), D.put(np.reshape(used, K), np.uint8, device)
        if K == 0:
            d_theta, d_used = torch.zeros(4, dtype=torch.float32, device=device), torch.zeros(1, dtype=torch.uint8, device=device)
        d_gx, d_gy = D.put(gx, np.float32, device), D.put(gy, np.float32, device)
        d_ll = torch.empty((max(Q, 1), G), dtype=torch.float64, device=device)
        work, work_bytes = D.work_buffer(lib, "loc_spa_grid_work_bytes", Q, K, G, int(k_groups), device=device, fill=fill)
        D.prefill((d_ll,), fill)
        _lib.check(lib.loc_spa_grid(d_c.data_ptr(), Q, K, pitch, int(P), d_theta.data_ptr(), d_used.data_ptr(), d_gx.data_ptr(),
                                    d_gy.data_ptr(), G, int(k_groups), d_ll.data_ptr(), work.data_ptr(), work_bytes, D.stream()),
                   "loc_spa_grid")
        return d_ll.cpu().numpy()[:Q]


# ---------------------------------------------------------------- the command's work

def spa(c, P, samples, locs, out=None, folds=10, grid=64, pad=0.1, ridge=1.0, iters=12, longlat=False, keep_surfaces=False,
        host=False, silence=False, device="cuda:0", sites=None, extra=None):
    """The command's work for a count matrix: returns the summary dict and writes the output files when `out` is given.
    extra: entries appended to the summary (--ld_prune: what baselines.prelude recorded)."""
    import pandas as pd
    c = B.check_counts(c, P)
    N, K = c.shape
    samples = np.asarray(samples).astype(str)
    locs = np.asarray(locs, dtype=np.float64).reshape(N, 2)
    located = ~np.isnan(locs).any(axis=1)
    n_located = int(located.sum())
    if n_located < 2:
        raise SystemExit(f"{PROG}: fewer than 2 samples of --sample_data have a location: nothing to fit")
    if not 2 <= folds <= n_located:
        raise SystemExit(f"{PROG}: --folds must be 2 .. the number of located samples ({n_located})")
    if not 1 <= iters <= MAX_ITERS:
        raise SystemExit(f"{PROG}: --iters must be 1 .. {MAX_ITERS}")
    if not (np.isfinite(ridge) and ridge >= 0):
        raise SystemExit(f"{PROG}: --ridge must be finite and >= 0")
    xy, mean, sd = normalise(locs, located)
    xs, ys = grid_nodes(xy, located, grid, pad)
    gx, gy = flat_nodes(xs, ys)
    ct = np.ascontiguousarray(c.T)
    fold = fold_of(located, folds)

    if host:
        def fit(w):
            return fit_host(ct, P, xy, w, ridge, iters)

        def likelihood(rows, theta, used):
            return grid_host(c[rows], P, theta, used, gx, gy)
    else:
        B.require_gpu(PROG, LAUNCH)
        import torch
        from . import _device as D
        with torch.cuda.device(device):
            buf = B.padded(ct)
            d_ct = (D.put(buf, np.int8, device), int(buf.shape[1]))

        def fit(w):
            return fit_device(ct, P, xy, w, ridge, iters, device=device, on_device=d_ct)

        def likelihood(rows, theta, used):
            return grid_device(c[rows], P, theta, used, gx, gy, device=device)

    placed_xy = np.full((N, 2), np.nan)
    nodes = np.full(N, -1, dtype=np.int64)
    border = np.zeros(N, dtype=bool)
    thetas, useds, lls = [], [], {}
    for f in list(range(folds)) + [-1]:                                  # -1: the fit on all located samples
        w = (located & (fold != f)).astype(np.uint8)
        theta, used = fit(w)
        thetas.append(theta)
        useds.append(used)
        rows = np.flatnonzero(fold == f)
        if not len(rows):
            continue
        ll = likelihood(rows, theta, used)
        have = ((c[rows] >= 0) & used.astype(bool)[None]).any(axis=1)
        at, node, edge = peaks(ll, xs, ys, have)
        placed_xy[rows] = at * sd[None] + mean[None]
        nodes[rows], border[rows] = np.where(have, node, -1), edge
        if keep_surfaces:
            lls[f] = ll
    theta_all, used_all = thetas[-1], useds[-1]
    K_used = int(used_all.sum())
    max_last = max((float(t[u.astype(bool), 3].max()) for t, u in zip(thetas, useds) if u.any()), default=0.0)

    shared, shared_lines = B.placement_summary(c, P, located, placed_xy, locs, longlat, "SPA", how="held-out")
    own = {"K_used": K_used, "folds": int(folds), "grid": int(grid), "pad": float(pad), "ridge": float(ridge), "iters": int(iters),
           "max_last_step": B.num(max_last), "n_border": int(border.sum()), "n_unplaced": int(np.isnan(placed_xy).any(axis=1).sum())}
    summary = {key: {**shared, **own}[key] for key in SUMMARY_KEYS}
    summary.update(extra or {})

    if out is not None:
        idx = np.arange(K, dtype=np.int64) if sites is None else np.asarray(sites, dtype=np.int64)
        frame = pd.DataFrame({"x": placed_xy[:, 0], "y": placed_xy[:, 1], "sampleID": samples.astype(object)})
        write_atomic(out + "_spa_locs.txt", lambda fh: frame.to_csv(fh, index=False))
        th = theta_all.astype(np.float64)
        write_atomic(out + "_spa_sites.txt", "variant\tused\tax\tay\tb\tslope\n" + "".join(
            f"{int(idx[k])}\t{int(used_all[k])}\t{float(th[k, 0])!r}\t{float(th[k, 1])!r}\t{float(th[k, 2])!r}\t"
            f"{float(np.hypot(th[k, 0], th[k, 1]))!r}\n"
            for k in range(K)))
        write_atomic(out + "_spa_summary.json", json.dumps(summary, indent=1) + "\n")
        if keep_surfaces:
            write_atomic(out + "_spa.npz", lambda fh: B.save_npz(
                fh, sites=idx, theta=np.stack(thetas), used=np.stack(useds), xs=xs, ys=ys, mean=mean, sd=sd, fold=fold,
                nodes=nodes, **{("ll_all" if f < 0 else f"ll_fold{f}"): v for f, v in lls.items()}), mode="wb")
    if not silence:
        for line in shared_lines:
            print(line)
    summary["_xy"], summary["_theta"], summary["_used"], summary["_nodes"] = placed_xy, np.stack(thetas), np.stack(useds), nodes
    return summary


# ---------------------------------------------------------------- command

def _own_arguments(p):
    p.add_argument("--folds", default=10, type=int, help="cross-validation folds: the r-th located sample belongs to fold r mod "
                                                         "FOLDS (default 10; 2 .. the number of located samples)")
    p.add_argument("--grid", default=64, type=int, help=f"nodes per axis of the likelihood grid (default 64, {GRID_RANGE[0]} .. "
                                                        f"{GRID_RANGE[1]})")
    p.add_argument("--pad", default=0.1, type=float, help="share of the located samples' span the grid adds on each side (default 0.1)")
    p.add_argument("--ridge", default=1.0, type=float, help="penalty on the two slopes of a surface (default 1.0)")
    p.add_argument("--iters", default=12, type=int, help=f"Newton steps of a fit (default 12, 1 .. {MAX_ITERS})")
    p.add_argument("--longlat", default=False, action="store_true",
                   help="x / y are longitude / latitude degrees: errors are great-circle km (the model stays planar)")
    p.add_argument("--host", default=False, action="store_true",
                   help="the NumPy form in float64 instead of the GPU (the files differ within the fp32 bounds of the module text)")
    p.add_argument("--keep_surfaces", default=False, action="store_true",
                   help="keep theta per fold, used, the grid and the likelihood surfaces in {out}_spa.npz")


def build_parser():
    return B.build_parser(PROG, "Logistic allele-frequency surfaces per site and a maximum-likelihood placement baseline.",
                          _own_arguments)


def main(argv=None):
    parser = build_parser()
    a = B.parse_args(parser, argv)
    if a.folds < 2:
        parser.error("--folds must be 2 .. the number of located samples")
    if not GRID_RANGE[0] <= a.grid <= GRID_RANGE[1]:
        parser.error(f"--grid must be {GRID_RANGE[0]} .. {GRID_RANGE[1]}")
    if not (np.isfinite(a.pad) and a.pad >= 0):
        parser.error("--pad must be finite and >= 0")
    if not (np.isfinite(a.ridge) and a.ridge >= 0):
        parser.error("--ridge must be finite and >= 0")
    if not 1 <= a.iters <= MAX_ITERS:
        parser.error(f"--iters must be 1 .. {MAX_ITERS}")
    c, P, samples, locs, idx = B.prelude(parser, a, LAUNCH)
    try:
        spa(c, P, samples, locs, a.out, a.folds, a.grid, a.pad, a.ridge, a.iters, a.longlat, a.keep_surfaces, a.host, a.silence,
            sites=idx, extra=getattr(a, "ld_summary", None))
    except ValueError as e:
        raise SystemExit(f"{PROG}: {e}") from None
    return 0


if __name__ == "__main__":
    sys.exit(main())
