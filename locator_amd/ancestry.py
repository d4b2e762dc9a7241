#!/usr/bin/env python3
"""`python -m locator_amd.ancestry`: where along the chromosome a haplotype copies from whom.  The posterior of the haplotype
copying model of the paint command (locator_amd/paint.py: Li & Stephens 2003) is summed per window of the genome and contracted
with attributes of the donors: one-hot labels give local ancestry, coordinates give a location a window, the copying-model
counterpart of `locator --windows`.

  python -m locator_amd.ancestry --vcf phased.vcf.gz --out out/test --window_snps 500 --sample_data samples.txt [--labels labels.txt]

  model       `local_host(h, donor, owner, rec, rho, theta, v, win, dtype)` -> (out [R][W][C], ll [R] float64, n_donors [R]
              int32), every operation in `dtype`.  The inputs, their checks, the donors of a recipient, u, e_j, the forward
              pass, ll, t, T, g, G, gamma = g (1 / G) (1 / G read as 0 where G is below the smallest normal number) and b_(j-1)
              are paint.copy_host's (its module text).  v [C][>= H] holds C <= 64 attributes of the columns, finite at every
              donor column; win [W][2] the windows [v0, v1) of sites, 0 <= v0 < v1 <= K, ascending and disjoint, gaps allowed.
                S_w(d) = the sum of gamma_j(d) over j = v1 - 1 down to v0; out[i][w][c] = sum over the donors d of recipient i
                of S_w(d) v[c][d].
              out is the plain sum: a channel of ones gives the window's number of sites (its posterior mass), any other channel
              over it the posterior mean of the attribute.  A value of v at a column that is no donor of the recipient is never
              interpreted.  A recipient with D = 0 gets zeros, ll = 0, n_donors = 0.  K = 0 admits no window and is refused.
  input       phased calls of ploidy 2 with CHROM / POS, as the impute command reads them (--vcf or --zarr; a heterozygous call
              without phase is refused).  Sites with an allele above 1 are dropped (multiallelic_dropped).
  attributes  at least one of --sample_data (tab-separated sampleID, x, y; NaN / NA = none) and --labels (tab-separated sampleID,
              label; NA = none).  The channels, in this order: one a label in sorted order, one-hot, at most 61; x and y where
              located, centred on the donors' mean and divided by the largest absolute deviation, so that |v| <= 1 (undone on
              the host in float64); a channel of ones, the mass.
  windows     exactly one of --window_snps / --window_bp, with --window_start and --window_step, as the localpca command forms
              them (localpca.window_bounds); windows without a site are dropped, a --window_step below the size is refused
              (the windows would overlap).
  donors      the samples that have every requested attribute (--max_donors M: every ceil(n / M)-th of them).  Recipients are
              all haplotypes; nobody copies from their own individual, so a donor's own result is leave-one-out by
              construction.  The donor columns and a batch of the other samples share the --max_haps columns of a launch, as
              impute's panel mode lays them out; more donors than fit are refused with their number.
  switching   rho, --switch, --em_rounds, --em_sample, --uniform and --theta as in paint (paint.estimate_switch: rounds of
              loc_paint_copy).

Outputs: {out}_ancestry_windows.txt (chrom start stop first_site n_sites), {out}_ancestry.zarr (samples, channels, windows/chrom,
start, stop, first_site, n_sites; mass [W][2N] = ones / n_sites; local [W][2N][C-1] = channel / ones, coordinates in map units,
NaN where the mass is 0; haplotype 2 s + a is allele a of sample s), with --labels {out}_ancestry_Q.txt (sampleID, a column a
label: the site-weighted mean over windows and both haplotypes of the label's posterior; label, call), with --sample_data
{out}_ancestry_locs.txt (x,y,sampleID: every sample at the site-weighted mean of its windows' posterior-mean locations), with
--keep_windows {out}_ancestry_windows/{chrom}_{start}-{stop}_predlocs.txt a window (x,y,sampleID, the mean of the two haplotypes):
a directory that `plot --infile`, `regions --infile` and `summarize` read as they read a `locator --windows` run,
{out}_ancestry_history.txt (round switch ll) and {out}_ancestry_summary.json.  Without a GPU the run stops and says so; --host
asks for the NumPy form in float64 (--host_dtype float32: the yardstick of the device's round-off).  The device computes in fp32
(loc_paint_local, include/locator_hip_local.h): the files of the two paths agree within round-off; each path is deterministic.
--budget_gb bounds the scratch and the output rows of one launch (the recipients go in batches, which changes no bit).

Not built: a model with ancestry-level states and their own switch rates (FLARE, RFMix), recombination maps, combining donor
groups beyond 4,096 columns, a plot of the windows, per-window donor shares as an output, ploidy other than 2.  Unphased calls
are phased by `python -m locator_amd.phase` first.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

from . import _abi
from . import baselines as B
from . import paint as PT
from ._files import write_atomic

PROG = "locator_amd.ancestry"
LAUNCH = "the recursions are loc_paint_local and loc_paint_copy launches"
MAX_HAPS = PT.MAX_HAPS
MAX_CHANNELS = _abi.LOC_LOCAL_MAX_CHANNELS
MAX_LABELS = MAX_CHANNELS - 3           # beside them x, y and the mass
HEAD = ("N", "n_located", "K", "P", "error_unit", "r2_x", "r2_y", "mean_error", "median_error")
SUMMARY = ("N", "K", "H", "n_donor_haps", "groups", "multiallelic_dropped", "W", "C", "channels", "theta", "switch", "uniform",
           "em_rounds", "ll", "min_mass")


# ---------------------------------------------------------------- the definition

def _check_local(v, win, H, K):
    """(v float64 [C][>= H], win int64 [W][2]) after the refusals of the module text."""
    v = np.asarray(v, dtype=np.float64)
    if v.ndim != 2 or not 1 <= v.shape[0] <= MAX_CHANNELS or v.shape[1] < H:
        raise ValueError(f"attributes of shape {v.shape}: need [C][columns] with C 1 .. {MAX_CHANNELS} and {H} columns at least")
    w = np.asarray(win)
    if w.ndim != 2 or w.shape[1] != 2 or len(w) < 1 or not np.issubdtype(w.dtype, np.integer):
        raise ValueError(f"windows of shape {w.shape} and type {w.dtype}: need whole numbers [W][2] with W >= 1")
    w = np.ascontiguousarray(w, dtype=np.int64)
    bad = (w[:, 0] < 0) | (w[:, 0] >= w[:, 1]) | (w[:, 1] > K)
    bad[1:] |= w[1:, 0] < w[:-1, 1]
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise ValueError(f"window {i} = [{int(w[i, 0])}, {int(w[i, 1])}): needs 0 <= v0 < v1 <= K = {K}, ascending and disjoint")
    return v, w


def _local_batch(h, dn, rcols, rho, theta, dtype, v, win):
    f = np.dtype(dtype).type
    K, (R, H) = h.shape[0], dn.shape
    W, C = len(win), len(v)
    u, rj, ah_all, _, ll = PT.forward_batch(h, dn, rcols, rho, theta, dtype)
    b = np.broadcast_to(u, (R, H)).astype(dtype)
    # a column that is a donor of none of these recipients has S = 0 throughout: its attribute is not looked at
    vt = np.where(dn.any(axis=0)[:, None], v[:, :H].T, 0.0).astype(dtype)
    out = np.zeros((R, W * C), dtype=dtype)
    S = np.zeros((R, H), dtype=dtype)
    tiny = np.finfo(dtype).tiny
    w = W - 1
    for j in range(K - 1, -1, -1):
        t = PT.emissions(h, j, rcols, dn, theta, dtype) * b
        g = ah_all[j] * b
        T, G = t.sum(axis=1, dtype=dtype), g.sum(axis=1, dtype=dtype)
        if w >= 0 and win[w, 0] <= j < win[w, 1]:
            with np.errstate(divide="ignore"):
                invG = np.where(G >= tiny, f(1) / G, f(0)).astype(dtype)
            S += g * invG[:, None]
            if j == win[w, 0]:
                out[:, w * C:(w + 1) * C] = S @ vt
                S[:] = 0
                w -= 1
        b = ((f(1) - rj[j]) * (f(1) / T))[:, None] * t + rj[j] * u
    return out, ll


def local_host(h, donor, owner, rec, rho, theta, v, win, dtype=np.float64):
    """(out [R][W][C] dtype, ll [R] float64, n_donors [R] int32): the definition in the module text."""
    hh = np.asarray(h)
    v, win = _check_local(v, win, len(np.asarray(donor)), hh.shape[0] if hh.ndim == 2 else 0)
    W, C = len(win), len(v)
    out, ll, nd = PT._host_model(_local_batch, ((W * C, dtype, 0),), h, donor, owner, rec, rho, theta, dtype, extra=(v, win))
    return out.reshape(len(out), W, C), ll, nd


# ---------------------------------------------------------------- the device form

def local_device(h, donor, owner, rec, rho, theta, v, win, block=0, pitch=None, pad_fill=-1, fill=None, budget=4 << 30, device="cuda:0",
                 vpitch=None, v_pad=np.nan):
    """local_host's answer from loc_paint_local launches (out float32), the recipients in batches whose scratch and output rows
    stay within `budget` bytes.  fill: a 32-bit pattern that scratch and the outputs hold before a launch (tests); vpitch: the
    floats of a row of v on the device (default: H rounded up to 4), the pad holding v_pad (a value, or a np.random.Generator)."""
    hh = np.asarray(h)
    H = len(np.asarray(donor))
    v, win = _check_local(v, win, H, hh.shape[0] if hh.ndim == 2 else 0)
    W, C = len(win), len(v)
    vpitch = (H + 3) // 4 * 4 if vpitch is None else int(vpitch)
    if isinstance(v_pad, np.random.Generator):
        buf = v_pad.normal(0.0, 1e30, (C, max(vpitch, 4))).astype(np.float32)
    else:
        buf = np.full((C, max(vpitch, 4)), v_pad, dtype=np.float32)
    buf[:, :H] = v[:, :H]
    extra = (buf, C, vpitch, np.ascontiguousarray(win, dtype=np.int32), W)
    out, ll, nd = PT._device_model("loc_paint_local", ((W * C, np.float32, 0),), 0, h, donor, owner, rec, rho, theta, block, pitch,
                                   pad_fill, fill, budget, device, extra=extra)
    return out.reshape(len(out), W, C), ll, nd


# ---------------------------------------------------------------- the command's pieces

def read_labels(path, samples, prog=PROG):
    """[N] object: the label of every genotype sample in their order, None where the table has none (NA) or lacks the sample."""
    import pandas as pd
    table = pd.read_csv(path, sep="\t", dtype=str, keep_default_na=False)
    if "sampleID" not in table.columns or "label" not in table.columns:
        raise SystemExit(f"{prog}: {path} needs the tab-separated columns sampleID and label")
    given = dict(zip(table["sampleID"], table["label"]))
    out = np.array([given.get(s) for s in np.asarray(samples).astype(str)], dtype=object)
    out[[x in ("NA", "NaN", "nan", "") for x in out]] = None
    return out


def channels(labels, locs, donors):
    """(names, V float64 [C][N] the attributes of the samples (NaN where a sample has none), centre [2], scale): the module
    text's channels from the donors' attributes.  labels, locs: None where not requested."""
    N = len(labels) if labels is not None else len(locs)
    names, rows = [], []
    if labels is not None:
        for name in sorted(set(labels[donors])):
            names.append(f"label:{name}")
            rows.append(np.where(labels == None, np.nan, (labels == name).astype(np.float64)))   # noqa: E711 (elementwise)
    centre, scale = np.zeros(2), 1.0
    if locs is not None:
        centre = locs[donors].mean(axis=0)
        scale = float(np.abs(locs[donors] - centre).max())
        scale = scale if scale > 0 else 1.0
        names += ["x", "y"]
        rows += [(locs[:, 0] - centre[0]) / scale, (locs[:, 1] - centre[1]) / scale]
    names.append("mass")
    rows.append(np.ones(N))
    return names, np.array(rows), centre, scale


def run_model(local, hap, donors, V, win, rho, theta, max_haps=MAX_HAPS):
    """The model over paint's launch groups for every haplotype: (out float64 [2N][W][C], ll [2N], n_donors [2N], number of
    groups).  V [C][N]: the samples' attributes; a launch gets them at its donor columns and NaN elsewhere.  local: local_host or
    local_device with the leading eight arguments."""
    N = hap.shape[1] // 2
    out = np.zeros((2 * N, len(win), len(V)))
    ll, nd = np.zeros(2 * N), np.zeros(2 * N, dtype=np.int32)
    n_groups = 0
    for n_groups, (cols, at, hcols, donor, owner, rec) in enumerate(PT.group_columns(N, donors, max_haps), 1):
        v = np.where(donor[None, :] != 0, np.repeat(V[:, cols], 2, axis=1), np.nan)
        o, l, n = local(np.ascontiguousarray(hap[:, hcols]), donor, owner, rec.astype(np.int32), rho, theta, v, win)
        out[hcols[rec]], ll[hcols[rec]], nd[hcols[rec]] = o, l, n
    return out, ll, nd, n_groups


def site_weighted(values, n_sites):
    """The mean of values [W][...] over the windows with weight n_sites, over the windows at which a value is finite (NaN where
    none is)."""
    shape = (len(n_sites),) + (1,) * (values.ndim - 1)
    wt = np.where(np.isfinite(values), np.asarray(n_sites, dtype=np.float64).reshape(shape), 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (np.where(wt > 0, values, 0.0) * wt).sum(axis=0) / wt.sum(axis=0)


# ---------------------------------------------------------------- the command's work

def ancestry(hap, samples, chrom, pos, locs=None, labels=None, out=None, window_snps=None, window_bp=None, window_start=0,
             window_step=None, switch=0.01, em_rounds=3, em_sample=256, theta=None, uniform=False, max_donors=None, max_haps=MAX_HAPS,
             longlat=False, keep_windows=False, dropped=0, host=False, silence=False, device="cuda:0", budget=4 << 30, dtype=np.float64):
    """The command's work for a site-major haplotype matrix hap [K][2N] with the sites' chrom and pos: returns the summary dict
    and writes the output files when `out` is given.  locs [N][2] (NaN: none) and labels [N] (None: none), either may be None."""
    from . import genotypes as G
    from . import localpca as LP
    hap = np.ascontiguousarray(hap, dtype=np.int8)
    K, H = hap.shape
    N = H // 2
    samples = np.asarray(samples).astype(str)
    if H != 2 * N or len(samples) != N or N < 2:
        raise SystemExit(f"{PROG}: {H} haplotype columns for {len(samples)} samples: needs two a sample and two samples at least")
    if K == 0:
        raise SystemExit(f"{PROG}: no site is left: no window to form")
    if locs is None and labels is None:
        raise SystemExit(f"{PROG}: needs --sample_data (locations) or --labels: the posterior is contracted with the donors' attributes")
    if not 2 <= max_haps <= MAX_HAPS:
        raise SystemExit(f"{PROG}: --max_haps must be 2 .. {MAX_HAPS}")
    if max_donors is not None and max_donors < 1:
        raise SystemExit(f"{PROG}: --max_donors must be >= 1")
    has = np.ones(N, dtype=bool)
    located = None
    if locs is not None:
        locs = np.asarray(locs, dtype=np.float64).reshape(N, 2)
        located = ~np.isnan(locs).any(axis=1)
        has &= located
    if labels is not None:
        labels = np.asarray(labels, dtype=object)
        has &= np.array([x is not None for x in labels])
    pool = np.flatnonzero(has)
    if not len(pool):
        raise SystemExit(f"{PROG}: no sample has every requested attribute: there is no donor")
    donors = pool if max_donors is None else pool[::-(-len(pool) // max_donors)]
    PT.check_room(PROG, 2 * len(donors) + (2 if len(donors) < N else 0), len(donors), max_haps, f"of the {len(pool)} candidate samples")
    names, V, centre, scale = channels(labels, locs, donors)
    n_labels = len(names) - 1 - (2 if locs is not None else 0)
    if n_labels > MAX_LABELS:
        raise SystemExit(f"{PROG}: {n_labels} labels among the donors: at most {MAX_LABELS} (a launch holds {MAX_CHANNELS} channels)")
    size = window_snps if window_bp is None else window_bp
    if window_step is not None and size is not None and window_step < size:
        raise SystemExit(f"{PROG}: --window_step {window_step} below the window size {size}: the windows would overlap")
    win, table = LP.window_bounds(chrom, pos, np.arange(K), window_snps, window_bp, window_start, window_step)
    keep = win[:, 1] > win[:, 0]
    win, table = win[keep], {key: val[keep] for key, val in table.items()}
    if not len(win):
        raise SystemExit(f"{PROG}: no window holds a site")
    n_sites = win[:, 1] - win[:, 0]
    W, C = len(win), len(names)
    theta = PT.checked_options(PROG, switch, em_rounds, em_sample, theta, 2 * len(donors))
    if not host:
        B.require_gpu(PROG, LAUNCH)
    copy = PT.model_form(PT.copy_host, PT.copy_device, host, dtype, budget, device)
    if host:
        local = lambda *eight: local_host(*eight, dtype=dtype)
    else:
        local = lambda *eight: local_device(*eight, budget=budget, device=device)
    g, first = PT.site_gaps(chrom, pos, K, uniform)

    lam, history, _ = PT.estimate_switch(copy, hap, donors, g, first, switch, em_rounds, em_sample, theta, max_haps)
    rho = PT.switch_rates(lam, g, first)
    res, ll, nd, n_groups = run_model(local, hap, donors, V, win, rho, theta, max_haps)

    ones = res[:, :, -1].T                                             # [W][2N]
    mass = ones / n_sites[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        local_mean = np.where(ones[:, :, None] > 0, np.transpose(res[:, :, :-1], (1, 0, 2)) / ones[:, :, None], np.nan)
    if locs is not None:
        local_mean[:, :, n_labels:n_labels + 2] = local_mean[:, :, n_labels:n_labels + 2] * scale + centre
    ran = nd > 0
    summary = {"N": int(N), "K": int(K), "H": int(H), "n_donor_haps": int(2 * len(donors)), "groups": int(n_groups),
               "multiallelic_dropped": int(dropped), "W": int(W), "C": int(C), "channels": list(names), "theta": float(theta),
               "switch": float(lam), "uniform": bool(uniform), "em_rounds": int(em_rounds), "ll": B.num(ll.sum()),
               "min_mass": B.num(mass[:, ran].min()) if ran.any() else None}
    summary = {key: summary[key] for key in SUMMARY}
    lines = [f"{N} samples, {K} sites in {W} windows: {H} haplotypes copy from {2 * len(donors)} donor haplotypes in {n_groups} launch "
             f"group(s), {C} channels", f"theta {theta!r}, switch rate {lam!r} after {em_rounds} rounds, ll {summary['ll']!r}"]
    Q = call = xy = None
    if labels is not None:
        per_hap = site_weighted(local_mean[:, :, :n_labels], n_sites)                      # [2N][L]
        with np.errstate(invalid="ignore"):
            Q = np.nanmean(per_hap.reshape(N, 2, n_labels), axis=1) if n_labels else np.zeros((N, 0))
        label_names = [n[len("label:"):] for n in names[:n_labels]]
        call = np.array([label_names[int(np.argmax(q))] if np.isfinite(q).all() and len(q) else None for q in Q], dtype=object)
        known = np.array([x is not None for x in labels]) & np.array([x is not None for x in call])
        acc = float(np.mean(labels[known] == call[known])) if known.any() else None
        summary.update({"labels": label_names, "n_labelled": int(sum(x is not None for x in labels)), "label_accuracy": B.num(acc)})
        lines.append(f"{len(label_names)} labels: leave-one-out accuracy of the call {acc!r} over {int(known.sum())} labelled samples")
    if locs is not None:
        per_hap = site_weighted(local_mean[:, :, n_labels:n_labels + 2], n_sites)          # [2N][2]
        with np.errstate(invalid="ignore"):
            xy = np.nanmean(per_hap.reshape(N, 2, 2), axis=1)
        head, more = B.placement_summary(np.broadcast_to(np.int8(0), (N, K)), 2, located, xy, locs, longlat, "copying")
        summary = {**{key: head[key] for key in HEAD}, **{k: v for k, v in summary.items() if k not in HEAD}}
        lines += more
    summary["path"] = "host" if host else "device"
    if out is not None:
        rows = ["chrom\tstart\tstop\tfirst_site\tn_sites\n"]
        rows += [f"{table['chrom'][w]}\t{int(table['start'][w])}\t{int(table['stop'][w])}\t{int(win[w, 0])}\t{int(n_sites[w])}\n"
                 for w in range(W)]
        write_atomic(out + "_ancestry_windows.txt", "".join(rows))
        store = out + "_ancestry.zarr"
        for grp in ("", "windows"):
            os.makedirs(os.path.join(store, grp), exist_ok=True)
            write_atomic(os.path.join(store, grp, ".zgroup"), json.dumps({"zarr_format": 2}))
        arrays = {"samples": samples.astype("U"), "channels": np.array(names).astype("U"), "windows/chrom": table["chrom"].astype("U"),
                  "windows/start": table["start"], "windows/stop": table["stop"], "windows/first_site": win[:, 0].copy(),
                  "windows/n_sites": n_sites, "mass": mass.astype(np.float32), "local": local_mean.astype(np.float32)}
        for name, arr in arrays.items():
            G.write_zarr_array(os.path.join(store, *name.split("/")), arr, arr.shape)
        PT.write_history(out + "_ancestry_history.txt", history)
        if Q is not None:
            head_q = "sampleID\t" + "".join(f"{n}\t" for n in summary["labels"]) + "label\tcall\n"
            write_atomic(out + "_ancestry_Q.txt", head_q + "".join(
                f"{samples[s]}\t" + "".join(f"{float(q)!r}\t" for q in Q[s]) + f"{'NA' if labels[s] is None else labels[s]}\t"
                f"{'NA' if call[s] is None else call[s]}\n" for s in range(N)))
        if xy is not None:
            B.write_locs(out + "_ancestry_locs.txt", xy, samples)
            if keep_windows:
                from .locator import write_predlocs
                folder = out + "_ancestry_windows"
                os.makedirs(folder, exist_ok=True)
                with np.errstate(invalid="ignore"):
                    per_win = np.nanmean(local_mean[:, :, n_labels:n_labels + 2].reshape(W, N, 2, 2), axis=2)
                for w in range(W):
                    write_predlocs(os.path.join(folder, f"{table['chrom'][w]}_{int(table['start'][w])}-{int(table['stop'][w])}_predlocs.txt"),
                                   per_win[w], samples)
        write_atomic(out + "_ancestry_summary.json", json.dumps(summary, indent=1) + "\n")
    if not silence:
        for line in lines:
            print(line)
    summary["_out"], summary["_mass"], summary["_local"], summary["_Q"], summary["_call"], summary["_xy"] = res, mass, local_mean, Q, call, xy
    summary["_history"], summary["_ll"], summary["_win"] = history, ll, win
    return summary


# ---------------------------------------------------------------- command

def build_parser():
    p = argparse.ArgumentParser(prog=PROG, description="Copying posteriors per window of the genome: local ancestry for labelled "
                                                       "donors, a location a window for located donors.")
    p.add_argument("--vcf", default=None, help="phased VCF (optionally gzipped)")
    p.add_argument("--zarr", default=None, help="phased zarr-v2 callset with calldata/GT, samples and variants/CHROM, POS, REF, ALT")
    p.add_argument("--matrix", default=None, help="refused: an allele-count matrix carries no phase")
    p.add_argument("--sample_data", default=None, help="tab-separated sampleID, x, y; NaN / NA = none: the located samples are donors")
    p.add_argument("--labels", default=None, help="tab-separated sampleID, label; NA = none: the labelled samples are donors")
    p.add_argument("--out", required=True, help="output stem")
    p.add_argument("--window_snps", default=None, type=int, help="sites a window")
    p.add_argument("--window_bp", default=None, type=int, help="base pairs a window")
    p.add_argument("--window_start", default=0, type=int, help="first site (--window_snps) or position (--window_bp) of the first window")
    p.add_argument("--window_step", default=None, type=int, help="distance of two windows' starts (default and least: the size)")
    PT.add_model_arguments(p)
    p.add_argument("--longlat", default=False, action="store_true",
                   help="x / y are longitude / latitude degrees: errors are great-circle km (the means stay planar)")
    p.add_argument("--keep_windows", default=False, action="store_true",
                   help="one {out}_ancestry_windows/{chrom}_{start}-{stop}_predlocs.txt a window (needs --sample_data)")
    PT.add_path_arguments(p, "device scratch and output rows of a launch at most, GiB (default 4)",
                          "the NumPy form in float64 instead of the GPU")
    p.add_argument("--gpu_number", default=None, type=str, help="the GPU to use (sets HIP_VISIBLE_DEVICES)")
    p.add_argument("--silence", default=False, action="store_true", help="no terminal output")
    return p


def main(argv=None):
    from . import impute as IM
    parser = build_parser()
    a = parser.parse_args(argv)
    if a.matrix is not None:
        raise SystemExit(f"{PROG} needs --vcf or --zarr: an allele-count --matrix carries no phase")
    if (a.vcf is None) == (a.zarr is None):
        parser.error("exactly one of --vcf / --zarr must be given")
    if (a.window_snps is None) == (a.window_bp is None):
        parser.error("exactly one of --window_snps / --window_bp must be given")
    if a.sample_data is None and a.labels is None:
        parser.error("at least one of --sample_data / --labels must be given")
    if a.keep_windows and a.sample_data is None:
        parser.error("--keep_windows needs --sample_data: a window's file holds locations")
    B.check_budget(parser, a)
    if a.gpu_number is not None:
        for var in ("HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
            os.environ[var] = a.gpu_number
    if not a.host:
        B.require_gpu(PROG, LAUNCH)
    try:
        d, dropped = IM.biallelic(IM.read_phased(a.vcf if a.zarr is None else a.zarr, a.zarr is not None, prog=PROG))
        N = len(d["samples"])
        locs = None if a.sample_data is None else B.read_locations(a.sample_data, d["samples"], PROG)
        labels = None if a.labels is None else read_labels(a.labels, d["samples"])
        ancestry(d["gt"].reshape(len(d["pos"]), 2 * N), d["samples"], d["chrom"], d["pos"], locs, labels, a.out, a.window_snps, a.window_bp,
                 a.window_start, a.window_step, a.switch, a.em_rounds, a.em_sample, a.theta, a.uniform, a.max_donors, a.max_haps,
                 a.longlat, a.keep_windows, dropped, a.host, a.silence, budget=int(a.budget_gb * (1 << 30)),
                 dtype=np.dtype(a.host_dtype).type)
    except ValueError as e:
        raise SystemExit(f"{PROG}: {e}") from None
    return 0


if __name__ == "__main__":
    sys.exit(main())
