#!/usr/bin/env python3
"""`python -m locator_amd.explain`: which sites a kept model uses to place samples (the explain command).

  python -m locator_amd.explain --model out/run.model.npz --vcf new.vcf.gz --out out/new --window_size 100000

For every selected row n (a sample, or a haplotype row of a --phased model) and distinct site k the Jacobian of the map-unit
prediction, J_x[n,k] = d x^ / d x_k and J_y[n,k] = d y^ / d x_k, and the gradient x input against the training mean,
A = J (x_nk - mov_mean_k).  Per site, means over the rows: mean_abs_x = |A_x|, mean_abs_y = |A_y|, mean_dist =
sqrt(A_x^2 + A_y^2), rms_grad = sqrt(mean(J_x^2 + J_y^2)).  Sites are matched, refused and imputed exactly as predict does
(locator_amd/query.py); the columns of a site listed more than once (a bootstrap model) are summed into one first-layer row
before the contraction; a site absent from the query has gamma = 0, hence all four statistics 0 (present = 0).
With --dosage the query is read as expected alt-allele dosages (FORMAT/DS, or GP; as predict --dosage) and the input is the
dosage d = q / 63 of the fixed-point rows: J = d(x^, y^) / d d per allele copy, A = J (d - mov_mean).
Outputs, each written atomically:
  {out}_snp_importance.txt   (several models: {out}_{model stem}_snp_importance.txt each)
  {out}_window_importance.txt with --window_size (several models: {out}_{model stem}_window_importance.txt each)
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

BN_EPS = 1e-3
STATS = ("mean_abs_x", "mean_abs_y", "mean_dist", "rms_grad")


def build_parser():
    p = argparse.ArgumentParser(prog="locator_amd.explain",
                                description="Per-SNP attribution maps of models kept by --keep_model.")
    p.add_argument("--model", nargs="+", required=True,
                   help="one or more .model.npz files, or directories holding them")
    p.add_argument("--vcf", help="query genotypes: VCF (optionally gzipped)")
    p.add_argument("--zarr", help="query genotypes: zarr-v2 store with calldata/GT, samples and variants/CHROM, POS, REF, ALT")
    p.add_argument("--matrix", help="query genotypes: tab-delimited sampleID + one 0/1/2 column per site (matched by name)")
    p.add_argument("--samples", default=None,
                   help="file of query sample IDs to explain, one per line (default: every query sample)")
    p.add_argument("--out", required=True, help="stem of every output file")
    p.add_argument("--min_site_overlap", default=0.5, type=float,
                   help="refuse a model of which fewer than this fraction of sites are in the query (default 0.5)")
    p.add_argument("--impute_missing", default=False, action="store_true",
                   help="missing calls at matched sites: Binomial(ploidy, training allele frequency) instead of 0")
    p.add_argument("--seed", default=None, type=int, help="NumPy seed of the --impute_missing draws")
    p.add_argument("--gpu_number", default=None, type=str, help="run on this GPU index")
    p.add_argument("--dosage", default=None, nargs="?", const="DS", choices=("DS", "GP"),
                   help="read the query as expected alt-allele dosages instead of GT calls: FORMAT/DS (bare --dosage; "
                        "calldata/DS of a zarr store, float values of a --matrix) or FORMAT/GP as GP1 + 2 GP2 (VCF only)")
    p.add_argument("--window_size", default=0, type=int,
                   help="also write per-window sums of the site statistics, windows of this many bp (default 0: none)")
    p.add_argument("--top", default=10, type=int, help="sites printed to the terminal, by mean_dist (default 10)")
    return p


# ------------------------------------------------------------------ host: site table, fold, reference
def site_index(model):
    """-> (col_site int64 [K]: distinct site of every model column, first int64 [Ks]: first column of every site, in order of
    first appearance).  Sites are (CHROM, POS, REF, ALT); a --matrix model's (POS -1) are its column names."""
    keys = (zip(model["chrom"].tolist()) if is_matrix_model(model)
            else zip(model["chrom"].tolist(), model["pos"].tolist(), model["ref"].tolist(), model["alt"].tolist()))
    seen, col_site, first = {}, [], []
    for c, key in enumerate(keys):
        s = seen.get(key)
        if s is None:
            s = seen[key] = len(first)
            first.append(c)
        col_site.append(s)
    return np.asarray(col_site, np.int64), np.asarray(first, np.int64)


def is_matrix_model(model):
    return bool(len(model["pos"])) and bool((np.asarray(model["pos"]) < 0).all())


def bn_scale(p):
    """Inference BatchNorm scale s_k = gamma_k / sqrt(mov_var_k + eps), float64."""
    return np.asarray(p["gamma"], np.float64) / np.sqrt(np.asarray(p["mov_var"], np.float64) + BN_EPS)


def fold_first_layer(p, col_site, Ks):
    """U[s] = sum over the columns c of site s of s_c W1[c]: float64 (Ks, H)."""
    u = bn_scale(p)[:, None] * np.asarray(p["W"][0], np.float64)
    U = np.zeros((Ks, u.shape[1]))
    np.add.at(U, col_site, u)
    return U


def reference_delta1(p, x, locs_norm):
    """float64 NumPy form of loc_explain_stack_grad: delta1 (n, 2, H) = d(x^, y^) / d(layer-1 pre-activation), for model
    columns x (n, K)."""
    _, sdlong, _, sdlat = locs_norm
    x = np.asarray(x, np.float64)
    W = [np.asarray(w, np.float64) for w in p["W"]]
    b = [np.asarray(v, np.float64) for v in p["b"]]
    s = bn_scale(p)
    a = x * s + (np.asarray(p["beta"], np.float64) - np.asarray(p["mov_mean"], np.float64) * s)
    nl = len(W) - 2
    acts = []
    for l in range(nl):
        z = a @ W[l] + b[l]
        a = np.where(z > 0, z, np.expm1(np.minimum(z, 0)))
        acts.append(a)
    dact = lambda a: np.where(a > 0, 1.0, a + 1.0)
    c = (W[nl] @ W[nl + 1]) * np.array([sdlong, sdlat])           # (H, 2): the linear head in map units
    g = c.T[None, :, :] * dact(acts[-1])[:, None, :]               # (n, 2, H)
    for l in range(nl - 1, 0, -1):
        g = (g @ W[l].T) * dact(acts[l - 1])[:, None, :]
    return g


def reference_stats(delta1, U, x_sites, mov_mean_sites):
    """float64 NumPy form of loc_explain_sites + loc_explain_reduce: J (n, 2, Ks) and the four statistics (4, Ks)."""
    J = delta1 @ np.asarray(U, np.float64).T
    A = J * (np.asarray(x_sites, np.float64) - np.asarray(mov_mean_sites, np.float64))[:, None, :]
    stats = np.stack([np.abs(A[:, 0]).mean(0), np.abs(A[:, 1]).mean(0), np.sqrt(A[:, 0] ** 2 + A[:, 1] ** 2).mean(0),
                      np.sqrt((J[:, 0] ** 2 + J[:, 1] ** 2).mean(0))])
    return J, stats


def window_table(chrom, pos, present, stats, size):
    """Per chromosome (order of first appearance), windows [start, start + size) from 0 up to the last site: the number of
    present sites and the sums of mean_abs_x, mean_abs_y, mean_dist over them.  Windows without a site are listed with 0."""
    chrom, pos = np.asarray(chrom).astype(str), np.asarray(pos, np.int64)
    present, stats = np.asarray(present, bool), np.asarray(stats, np.float64)
    rows = []
    for ch in dict.fromkeys(chrom.tolist()):
        on = chrom == ch
        w = pos[on] // size
        keep = present[on]
        nwin = int(w.max()) + 1
        cnt = np.bincount(w[keep], minlength=nwin)
        sums = [np.bincount(w[keep], weights=stats[i][on][keep], minlength=nwin) for i in range(3)]
        for i in range(nwin):
            rows.append((ch, i * size, (i + 1) * size, int(cnt[i]), sums[0][i], sums[1][i], sums[2][i]))
    return rows


# ------------------------------------------------------------------ device
def _l1_forward(model, X, device, unit=1):
    """Layer 1's ELU output for every row of X (uint8 [n][Kp]) in the exact fp32 forms: loc_l1_forward_rows with 3 bf16
    pieces where the LDS allows it, else the 32-row loc_l1_forward.  unit: the fixed-point unit of X (63 for the q rows of a
    --dosage query: import_params then holds the moving statistics in q units, and scale / shift of q give BN(d)).
    -> (net, a1 [ceil(n/128)*128][Hp])."""
    import ctypes as C

    import torch

    from . import _abi, _lib
    from .net import LocatorNet, _ptr, _stream
    lib = _lib.load()
    n = int(X.shape[0])
    Y = torch.zeros((n, 2), dtype=torch.float32, device=device)
    net = LocatorNet(X, Y, model["K"], model["width"], model["nlayers"], 0.0, seed=0, device=device,
                     **({"unit": int(unit)} if unit != 1 else {}))
    net.import_params(model["weights_used"])
    d, lay, P = net.d, net.lay, net.params.data_ptr()
    Hp, Kp = d.Hp, d.Kp
    bn4 = torch.empty(4 * Kp, dtype=torch.float32, device=device)
    _lib.check(lib.loc_bn_infer_scale_shift(d.K, Kp, P + 4 * lay.gamma, P + 4 * lay.beta, P + 4 * lay.mov_mean,
                                            P + 4 * lay.mov_var, _ptr(bn4), _stream()), "loc_bn_infer_scale_shift")
    rows = torch.arange(n, dtype=torch.int32, device=device)
    a1 = torch.zeros(((n + 127) // 128 * 128, Hp), dtype=torch.float32, device=device)
    chunk = _abi.LOC_PREDICT_CHUNK
    if lib.loc_l1_rows_supported(Hp, 3):
        pf = lib.loc_l1_partial_floats(C.byref(d))                    # the workspace's layer-1 partial sums
        partial = torch.empty(pf, dtype=torch.float32, device=device)
        tune = _lib.Tuning()
        for c0 in range(0, n, chunk):
            nc = min(chunk, n - c0)
            _lib.check(lib.loc_l1_forward_rows(_ptr(X), X.stride(0), C.c_void_p(rows.data_ptr() + 4 * c0), nc,
                                               C.byref(d), _ptr(bn4), P + 4 * lay.w1, P + 4 * lay.b1, _ptr(partial),
                                               pf, C.c_void_p(a1.data_ptr() + 4 * c0 * Hp), 3, 0, C.byref(tune),
                                               _stream()), "loc_l1_forward_rows")
    else:
        grid = net.l1_fwd_grid
        partial = torch.empty(grid * 32 * Hp, dtype=torch.float32, device=device)
        for i in range(0, n, 32):
            _lib.check(lib.loc_l1_forward(_ptr(X), X.stride(0), C.c_void_p(rows.data_ptr() + 4 * i), min(32, n - i),
                                          C.byref(d), _ptr(bn4), P + 4 * lay.w1, P + 4 * lay.b1, _ptr(partial), grid,
                                          C.c_void_p(a1.data_ptr() + 4 * i * Hp), None, None, C.c_float(1.0), _stream()),
                       "loc_l1_forward")
    return net, a1


def device_delta1(model, X, device="cuda:0", unit=1):
    """loc_explain_stack_grad on the query rows X (uint8 [n][Kp], model columns; in units of 1 / unit) -> (net, delta1 device
    [2n][Hp])."""
    import torch

    from . import _lib
    from .net import _ptr, _stream
    lib = _lib.load()
    n = int(X.shape[0])
    net, a1 = _l1_forward(model, X, device, unit)
    d, lay, P = net.d, net.lay, net.params.data_ptr()
    Hp, L = d.Hp, d.L
    _, sdlong, _, sdlat = model["locs_norm"]
    acts = torch.empty((L - 1) * n * Hp, dtype=torch.float32, device=device) if L > 1 else None
    g = torch.empty(2 * n * Hp, dtype=torch.float32, device=device) if L > 1 else None
    delta1 = torch.empty((2 * n, Hp), dtype=torch.float32, device=device)
    _lib.check(lib.loc_explain_stack_grad(_ptr(a1), n, Hp, L, P + 4 * lay.wh, P + 4 * lay.bh, P + 4 * lay.wa,
                                          P + 4 * lay.wb, float(sdlong), float(sdlat), _ptr(acts), _ptr(g), _ptr(delta1),
                                          _stream()), "loc_explain_stack_grad")
    del a1, acts, g
    return net, delta1


def device_sites(delta1, n, U, Xs, mov_mean_sites, device="cuda:0"):
    """loc_explain_sites + loc_explain_reduce: delta1 device [2n][Hp], U (Ks, H) host, Xs device uint8 [n][>= Ks] in site
    order, mov_mean_sites (Ks,) -> float64 (4, Ks)."""
    import torch

    from . import _lib
    from .net import _compute_units, _ptr, _stream
    lib = _lib.load()
    Hp = int(delta1.shape[1])
    Ks, H = U.shape
    Ud = np.zeros((Ks, Hp), np.float32)
    Ud[:, :H] = U
    Ud = torch.from_numpy(Ud).to(device)
    mm = torch.from_numpy(np.ascontiguousarray(mov_mean_sites, dtype=np.float32)).to(device)
    splits = lib.loc_explain_splits(int(n), int(Ks), _compute_units(torch.device(device)))
    partial = torch.empty(splits * 4 * Ks, dtype=torch.float64, device=device)
    out = torch.empty((4, Ks), dtype=torch.float64, device=device)
    _lib.check(lib.loc_explain_sites(_ptr(delta1), int(n), _ptr(Ud), int(Ks), Hp, _ptr(Xs), Xs.stride(0), _ptr(mm), splits,
                                     _ptr(partial), _stream()), "loc_explain_sites")
    _lib.check(lib.loc_explain_reduce(_ptr(partial), splits, int(Ks), int(n), _ptr(out), _stream()), "loc_explain_reduce")
    return out.cpu().numpy()


def explain_model(model, calls_dev, cv, ca, rows, device="cuda:0", dosage=False):
    """The four statistics (4, Ks) of one model on the query rows, plus its site index (col_site, first).  dosage: calls_dev
    holds float dosages (U, N) and the rows are q = rint(63 d).  loc_explain_sites then gets everything in q units - U / 63
    (the Jacobian per q), Xs and the moving means times 63 - so that A = (J / 63) (q - 63 mov_mean) = J (d - mov_mean) comes
    out as it is, and rms_grad, which it returns per q, is multiplied by 63 here."""
    from . import genotypes as G
    from . import query as Q
    col_site, first = site_index(model)
    Ks = len(first)
    unit = G.DOSAGE_UNIT if dosage else 1
    build = Q.query_rows_dosage if dosage else Q.query_rows
    X = build(calls_dev, cv, ca, rows, model["K"])
    net, delta1 = device_delta1(model, X, device, unit)
    del net
    Xs = X if Ks == model["K"] and (first == np.arange(Ks)).all() else build(calls_dev, cv[first], ca[first], rows, Ks)
    p = model["weights_used"]
    U = (fold_first_layer(p, col_site, Ks) / unit).astype(np.float32)
    stats = device_sites(delta1, len(rows), U, Xs, np.asarray(p["mov_mean"], np.float64)[first] * unit, device)
    if dosage:
        stats[3] *= unit
    return stats, col_site, first


# ------------------------------------------------------------------ command
def _read_ids(path):
    with open(path) as fh:
        return [line.strip() for line in fh if line.strip()]


def _write_sites(path, model, first, counts, present, stats, write):
    def body(fh):
        fh.write("chrom\tpos\tref\talt\tcolumns\tpresent\t" + "\t".join(STATS) + "\n")
        for i, c in enumerate(first.tolist()):
            fh.write(f"{model['chrom'][c]}\t{model['pos'][c]}\t{model['ref'][c]}\t{model['alt'][c]}\t{counts[i]}\t"
                     f"{int(present[i])}\t" + "\t".join(repr(float(stats[k, i])) for k in range(4)) + "\n")
    write(path, body)


def _write_windows(path, rows, write):
    def body(fh):
        fh.write("chrom\tstart\tstop\tsites\tmean_abs_x\tmean_abs_y\tmean_dist\n")
        for ch, a, b, n, sx, sy, sd in rows:
            fh.write(f"{ch}\t{a}\t{b}\t{n}\t{float(sx)!r}\t{float(sy)!r}\t{float(sd)!r}\n")
    write(path, body)


def main(argv=None):
    t0 = time.time()
    a = build_parser().parse_args(argv)
    if a.gpu_number is not None:
        for var in ("HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
            os.environ[var] = a.gpu_number
    if a.seed is not None:
        np.random.seed(a.seed)
    from . import query as Q
    from ._files import write_atomic

    # ---- host: read, match, refuse (nothing on the device yet) - as predict
    if a.window_size < 0:
        raise Q.QueryRefused("--window_size must be >= 0")
    if a.top < 0:
        raise Q.QueryRefused("--top must be >= 0")
    models = [Q.load_model(p) for p in Q.model_paths(a.model)]
    if len({(m["phased"], m["ploidy"]) for m in models}) > 1:
        raise Q.QueryRefused("--model: phased and unphased models (or models of different ploidy) cannot share one query")
    stems = [m["stem"] for m in models]
    if len(set(stems)) != len(stems):
        raise Q.QueryRefused("--model: two model files share the name stem " + repr(sorted(s for s in stems if stems.count(s) > 1)[0]))
    if a.window_size:
        for m in models:
            if is_matrix_model(m):
                raise Q.QueryRefused(f"--window_size: {m['path']} is a --matrix model; its sites have no positions")
    dosage = a.dosage is not None
    query = Q.read_query_dosage(a.vcf, a.zarr, a.matrix, a.dosage) if dosage else Q.read_query(a.vcf, a.zarr, a.matrix)
    columns = []
    for m in models:
        cv, ca, rep = Q.match_sites(m, query)
        (Q.check_query_dosage if dosage else Q.check_query)(m, query, rep, a.min_site_overlap)
        columns.append((cv, ca))
    phased = models[0]["phased"]
    idx = Q.select_samples(query, _read_ids(a.samples) if a.samples else None)
    rows = ((2 * idx[:, None] + np.arange(2)).reshape(-1) if phased else idx).astype(np.int32)
    if not len(rows):
        raise Q.QueryRefused("no samples to explain")
    calls, remapped, _ = (Q.compact_dosages if dosage else Q.compact_calls)(query, columns)
    if a.impute_missing:
        every = (np.concatenate(remapped), np.concatenate([ca for _, ca in columns]), np.concatenate([m["af"] for m in models]))
        if dosage:
            Q.impute_dosages(calls, rows, *every)
        else:
            Q.impute_calls(calls, rows, *every, phased)
    for m, (cv, _) in zip(models, columns):
        m["weights_used"] = Q.absent_gamma(m["weights"], cv)

    # ---- device: one upload of the matched calls, then rows + attribution per model
    import torch

    from .net import require_gpu
    require_gpu()
    dev = "cuda:0"
    calls_dev = torch.from_numpy(calls).to(dev)
    if phased:
        U_, N_, P_ = calls.shape
        calls_dev = calls_dev.view(U_, N_ * P_, 1)
    for m, cv, (cv_q, ca) in zip(models, remapped, columns):
        stats, col_site, first = explain_model(m, calls_dev, cv, ca, rows, dev, dosage)
        present = cv_q[first] >= 0
        counts = np.bincount(col_site, minlength=len(first))
        one = len(models) == 1
        path = a.out + "_snp_importance.txt" if one else f"{a.out}_{m['stem']}_snp_importance.txt"
        _write_sites(path, m, first, counts, present, stats, write_atomic)
        if a.window_size:
            wpath = a.out + "_window_importance.txt" if one else f"{a.out}_{m['stem']}_window_importance.txt"
            _write_windows(wpath, window_table(m["chrom"][first], m["pos"][first], present, stats, a.window_size),
                           write_atomic)
        print(f"{m['stem']}: {len(rows)} {'haplotype rows' if phased else 'samples'}, {len(first)} sites "
              f"({int(present.sum())} present, {len(first) - int(present.sum())} absent) -> {path}")
        order = np.argsort(-stats[2], kind="stable")[:a.top]
        for i in order:
            c = first[i]
            print(f"  {m['chrom'][c]}:{m['pos'][c]} {m['ref'][c]}>{m['alt'][c]}  mean_dist {stats[2, i]:.6g}  "
                  f"mean_abs_x {stats[0, i]:.6g}  mean_abs_y {stats[1, i]:.6g}  rms_grad {stats[3, i]:.6g}")
    print(f"explained {len(rows)} rows with {len(models)} model(s) in {time.time() - t0:.2f} s")
    return 0


if __name__ == "__main__":
    sys.exit(main())
