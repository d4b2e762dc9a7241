#!/usr/bin/env python3
"""`python -m locator_amd.plot`: per-sample density maps of replicate predictions, and their error summary.

  python -m locator_amd.plot --infile out/boot --sample_data samples.txt --out out/boot_plot --error --longlat

The post-processing step after --windows / --bootstrap / --jacknife or several kept models.  For each plotted sample:

  grid     per axis from (min - 10) to (max + 10) degrees of its predictions, int(max - min) * 10 points (np.linspace);
           y is latitude, x longitude
  Z        haversine Gaussian kernel density of the predictions (bandwidth 0.04 rad) at every grid point: every panel in
           ONE loc_kde_grid_batch launch (float64, include/locator_hip.h); `--host` evaluates the same sum with NumPy
  levels   three contour levels, labelled 0.95 / 0.5 / 0.1 (contour_levels)
  panel    the padded span of the wider axis, the other axis centred to the panel's aspect ratio (panel_limits)

drawn over the predictions, the sample's known location, the training locations (--training_samples) and a basemap
(--basemap; a zarr-v2 store of [2][n] lon / lat outlines per country and part, --map).  Written to {out}.pdf.

`--error` adds the kernel-peak / centroid summaries of every sample (what `python -m locator_amd.summarize` computes,
{out}_centroids.txt) and prints the mean, median and 5th / 95th percentiles of both errors over the samples with a
known location; `--longlat` gives them in great-circle km.

Deviations from the reference script: sample IDs match exactly, every predlocs file is read once,
--longlat converts degrees to radians, an axis spread under 1 degree gets 100 grid points, the panel grid has
ceil(n / ncol) rows, and equal padded spans take the x branch.
"""
from __future__ import annotations

import argparse
import math
import os
import sys

import numpy as np

BANDWIDTH = 0.04              # radians, the density maps' kernel
PAD = 10.0                    # degrees around the predictions
EARTH_KM = 6373.0
LEVEL_QUANTILES = (0.05, 0.5, 0.9)
LEVEL_LABELS = ("0.95", "0.5", "0.1")


# ---------------------------------------------------------------- panel data (pure functions)

def axis_count(lo, hi):
    """Grid points along one axis: int(spread) * 10, or 100 when the spread is under 1 degree (the reference gets 0)."""
    n = int(hi - lo) * 10
    return n if n > 0 else 100


def panel_grid(xpred, ypred):
    """(x axis, y axis) in degrees for one sample's predictions: the padded range of each, np.linspace."""
    xpred, ypred = np.asarray(xpred, dtype=np.float64), np.asarray(ypred, dtype=np.float64)
    xpred, ypred = xpred[np.isfinite(xpred)], ypred[np.isfinite(ypred)]
    if len(xpred) == 0 or len(ypred) == 0:
        return np.empty(0), np.empty(0)
    x0, x1, y0, y1 = xpred.min(), xpred.max(), ypred.min(), ypred.max()
    return (np.linspace(x0 - PAD, x1 + PAD, axis_count(x0, x1)),
            np.linspace(y0 - PAD, y1 + PAD, axis_count(y0, y1)))


def kde_grid_host(lat, lon, lat_axis, lon_axis, bandwidth=BANDWIDTH, chunk=1 << 22):
    """NumPy form of loc_kde_grid_batch for one panel (all radians): Z[iy, ix] = haversine Gaussian density at
    (lat_axis[iy], lon_axis[ix]); NaN everywhere when there are no points or a point is not finite."""
    lat, lon = np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64)
    ny, nx, n = len(lat_axis), len(lon_axis), len(lat)
    if n == 0 or not (np.isfinite(lat).all() and np.isfinite(lon).all()):
        return np.full((ny, nx), np.nan)
    glat, glon = np.meshgrid(lat_axis, lon_axis, indexing="ij")
    glat, glon = glat.ravel(), glon.ravel()
    z = np.empty(ny * nx)
    step = max(1, chunk // n)
    coslat = np.cos(lat)
    for a in range(0, ny * nx, step):
        b = min(a + step, ny * nx)
        hav = (np.sin((glat[a:b, None] - lat[None, :]) / 2) ** 2
               + np.cos(glat[a:b, None]) * coslat[None, :] * np.sin((glon[a:b, None] - lon[None, :]) / 2) ** 2)
        d = 2.0 * np.arcsin(np.sqrt(np.minimum(hav, 1.0)))
        z[a:b] = np.exp(-(d * d) / (2.0 * bandwidth * bandwidth)).sum(axis=1)
    return (z / (n * 2.0 * np.pi * bandwidth * bandwidth)).reshape(ny, nx)


def kde_grids_device(panels, bandwidth=BANDWIDTH, device="cuda:0"):
    """[(lat, lon, lat_axis, lon_axis) radians, ...] -> [Z (ny, nx), ...] from one loc_kde_grid_batch launch."""
    import torch
    from . import _lib
    lib = _lib.load()

    def offsets(sizes):
        o = np.zeros(len(sizes) + 1, dtype=np.int64)
        np.cumsum(sizes, out=o[1:])
        return o

    n = len(panels)
    if n == 0:
        return []
    pt_off = offsets([len(p[0]) for p in panels])
    lat_off = offsets([len(p[2]) for p in panels])
    lon_off = offsets([len(p[3]) for p in panels])
    z_off = offsets([len(p[2]) * len(p[3]) for p in panels])
    pts = np.empty((int(pt_off[-1]), 2), dtype=np.float64)
    for (lat, lon, _, _), a, b in zip(panels, pt_off[:-1], pt_off[1:]):
        pts[a:b, 0], pts[a:b, 1] = lat, lon
    lat_axis = np.concatenate([np.asarray(p[2], dtype=np.float64) for p in panels])
    lon_axis = np.concatenate([np.asarray(p[3], dtype=np.float64) for p in panels])
    with torch.cuda.device(device):
        d = [torch.from_numpy(a).to(device) for a in (pts, pt_off, lat_axis, lat_off, lon_axis, lon_off, z_off)]
        dz = torch.empty(max(int(z_off[-1]), 1), dtype=torch.float64, device=device)
        _lib.check(lib.loc_kde_grid_batch(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                          d[4].data_ptr(), d[5].data_ptr(), n, float(bandwidth), dz.data_ptr(),
                                          d[6].data_ptr(), torch.cuda.current_stream().cuda_stream), "loc_kde_grid_batch")
        z = dz.cpu().numpy()
    return [z[a:b].reshape(len(p[2]), len(p[3])) for p, a, b in zip(panels, z_off[:-1], z_off[1:])]


def contour_levels(Z):
    """Contour levels of one density grid, and their labels.

    The values are sorted and their running sums taken; each sorted value is then mapped through the piecewise-linear
    curve (running sum -> value).  For each of the quantiles 5 %, 50 % and 90 % of those mapped values, the first entry
    nearest to the quantile picks a level from n evenly spaced values between the smallest and largest density, kept
    unless it is already a level."""
    zed = np.sort(np.asarray(Z, dtype=np.float64).ravel())
    if len(zed) == 0 or not np.isfinite(zed).all():
        return [], []
    csum = np.cumsum(zed)
    w = np.interp(zed, csum, zed)
    even = np.linspace(zed[0], zed[-1], len(zed))
    levels = []
    for t in np.quantile(w, LEVEL_QUANTILES):
        v = even[int(np.argmin(np.abs(w - t)))]
        if v not in levels:
            levels.append(v)
    return levels, list(LEVEL_LABELS[:len(levels)])


def panel_limits(xpred, ypred, aspect):
    """(xmin, xmax, ymin, ymax) of a panel of width / height `aspect`: the larger padded span is kept, the other axis is
    centred on its padded range and sized to the aspect.  Equal spans take the x branch."""
    xpred, ypred = np.asarray(xpred, dtype=np.float64), np.asarray(ypred, dtype=np.float64)
    x0, x1 = np.nanmin(xpred) - PAD, np.nanmax(xpred) + PAD
    y0, y1 = np.nanmin(ypred) - PAD, np.nanmax(ypred) + PAD
    if x1 - x0 >= y1 - y0:
        h = (x1 - x0) / aspect
        c = (y0 + y1) / 2
        return float(x0), float(x1), float(c - h / 2), float(c + h / 2)
    w = aspect * (y1 - y0)
    c = (x0 + x1) / 2
    return float(c - w / 2), float(c + w / 2), float(y0), float(y1)


def distance_km(xpred, ypred, x, y):
    """Great-circle distance in km between (xpred, ypred) and (x, y), longitude / latitude in degrees."""
    xp, yp, x, y = (np.radians(np.asarray(v, dtype=np.float64)) for v in (xpred, ypred, x, y))
    a = np.sin((yp - y) / 2) ** 2 + np.cos(y) * np.cos(yp) * np.sin((xp - x) / 2) ** 2
    return EARTH_KM * 2 * np.arctan2(np.sqrt(a), np.sqrt(1 - a))


def layout(n, ncol, width, height):
    """(rows, panel aspect) of an n-panel figure with ncol columns."""
    rows = max(1, math.ceil(n / ncol))
    return rows, (width / ncol) / (height / rows)


# ---------------------------------------------------------------- data

def load_predlocs(indir):
    """Every *predlocs* file of a directory, read once in name order (as summarize reads them); x / y -> xpred / ypred."""
    import pandas as pd
    files = sorted(f for f in os.listdir(indir) if "predlocs" in f)
    if not files:
        raise SystemExit(f"no *predlocs* files in {indir}")
    aeg = pd.concat([pd.read_csv(os.path.join(indir, f)) for f in files], ignore_index=True)
    return aeg.rename(columns={"x": "xpred", "y": "ypred"})


def read_truth(sample_data):
    import pandas as pd
    return None if sample_data is None else pd.read_csv(sample_data, sep="\t").set_index("sampleID")


def true_location(truth, sid):
    """(x, y) of a sample from the sample file, NaN when unknown; a --phased row `<id>_h0` / `<id>_h1` takes <id>'s."""
    if truth is None:
        return np.nan, np.nan
    key = sid
    if sid not in truth.index and str(sid)[-3:] in ("_h0", "_h1"):
        key = str(sid)[:-3]
    if key not in truth.index:
        return np.nan, np.nan
    return float(truth.loc[key, "x"]), float(truth.loc[key, "y"])


def pick_samples(ids, samples=None, nsamples=9, seed=None):
    """The samples to plot: --samples as given, else --nsamples (at most all of them) drawn without replacement;
    `seed` makes the draw reproducible, None leaves it unseeded."""
    if samples:
        return [str(s) for s in samples]
    ids = [str(s) for s in ids]
    k = min(int(nsamples), len(ids))
    return [str(s) for s in np.random.RandomState(seed).choice(ids, k, replace=False)]


def sample_rows(aeg, sample):
    """The prediction rows of exactly this sample ID (the reference's substring match also picks up `s10` for `s1`)."""
    return aeg[aeg["sampleID"].astype(str) == str(sample)]


def panel_data(aeg, samples, aspect, host=False, bandwidth=BANDWIDTH):
    """Every panel's grid, density, levels and limits, before any drawing: a list of dicts with keys sample, xpred, ypred,
    xgrid, ygrid (degrees), Z (ny, nx), levels, labels, limits.  The densities come from one loc_kde_grid_batch launch,
    or from kde_grid_host under `host`."""
    panels = []
    for s in samples:
        rows = sample_rows(aeg, s)
        if len(rows) == 0:
            raise SystemExit(f"sample {s} has no predictions")
        xp, yp = rows["xpred"].to_numpy(np.float64), rows["ypred"].to_numpy(np.float64)
        xg, yg = panel_grid(xp, yp)
        panels.append({"sample": s, "xpred": xp, "ypred": yp, "xgrid": xg, "ygrid": yg})
    args = [(np.radians(p["ypred"]), np.radians(p["xpred"]), np.radians(p["ygrid"]), np.radians(p["xgrid"])) for p in panels]
    if host:
        zs = [kde_grid_host(*a, bandwidth=bandwidth) for a in args]
    else:
        zs = kde_grids_device(args, bandwidth)
    for p, z in zip(panels, zs):
        p["Z"] = z
        p["levels"], p["labels"] = contour_levels(z)
        p["limits"] = panel_limits(p["xpred"], p["ypred"], aspect) if len(p["xgrid"]) else (-180.0, 180.0, -90.0, 90.0)
    return panels


def error_table(aeg, truth, host=False, bandwidth=0.2):
    """kd / gc summaries of every sample, the DataFrame `summarize.summarize` builds from the same predictions."""
    import pandas as pd
    from . import summarize as S
    groups = [(sid, g["xpred"].to_numpy(), g["ypred"].to_numpy()) for sid, g in aeg.groupby("sampleID", sort=False)]
    dev = None if host else S.device_summaries([(x, y) for _, x, y in groups], bandwidth)[1]
    rows = []
    for i, (sid, xs, ys) in enumerate(groups):
        if dev is not None:
            kx, ky, gx, gy = (float(v) for v in dev[i])
        else:
            (kx, ky), (gx, gy) = S.kde_peak(xs, ys, bandwidth), S.centroid(xs, ys)
        tx, ty = true_location(truth, sid)
        rows.append({"sampleID": sid, "x": tx, "y": ty, "kd_x": kx, "kd_y": ky, "gc_x": gx, "gc_y": gy})
    return pd.DataFrame(rows, columns=["sampleID", "x", "y", "kd_x", "kd_y", "gc_x", "gc_y"])


def error_lines(bp, longlat=False):
    """The printed summary: mean, median and 90 % interval (5th, 95th percentiles) of the kernel-peak and centroid
    errors over the samples with a known location."""
    known = bp.dropna(subset=["x", "y"])
    if len(known) == 0:
        return ["no sample has a known location: no error summary"]
    dist = distance_km if longlat else (lambda xp, yp, x, y: np.hypot(xp - x, yp - y))
    out = []
    for name, cx, cy in (("kernel peak", "kd_x", "kd_y"), ("centroid", "gc_x", "gc_y")):
        e = np.asarray(dist(known[cx].to_numpy(), known[cy].to_numpy(), known["x"].to_numpy(), known["y"].to_numpy()))
        out += [f"mean {name} error = {np.mean(e)}", f"median {name} error = {np.median(e)}",
                f"90% CI for {name} error = {np.quantile(e, 0.05)} {np.quantile(e, 0.95)}"]
    return out


def read_basemap(path):
    """[(lon array, lat array), ...]: every [2][n] outline of a zarr-v2 store grouped by country, then part."""
    from .genotypes import walk_outlines
    return [(lon, lat) for _, _, lon, lat in walk_outlines(path)]


# ---------------------------------------------------------------- drawing

def draw(panels, out, ncol, width, height, truth=None, training=None, basemap=None):
    import matplotlib
    matplotlib.use("Agg")
    from matplotlib import pyplot as plt
    rows, _ = layout(len(panels), ncol, width, height)
    fig, axes = plt.subplots(nrows=rows, ncols=ncol, squeeze=False)
    flat = axes.ravel()
    handles, labels = [], []
    for ax, p in zip(flat, panels):
        xmin, xmax, ymin, ymax = p["limits"]
        ax.set_xlim(xmin, xmax)
        ax.set_ylim(ymin, ymax)
        ax.set_aspect("equal")
        ax.patch.set_facecolor("#ffffff")
        for s in ax.spines.values():
            s.set_visible(False)
        ax.get_xaxis().set_visible(False)
        ax.get_yaxis().set_visible(False)
        for bx, by in basemap or ():
            if ((bx > xmin) & (bx < xmax)).any() or ((by > ymin) & (by < ymax)).any():
                ax.plot(bx, by, "#ffffff", lw=0.15, zorder=0)
                ax.fill(bx, by, "#b0b0b0", zorder=0)
        if p["levels"]:
            cs = ax.contour(p["xgrid"], p["ygrid"], p["Z"], levels=p["levels"], colors="k", zorder=2)
            ax.clabel(cs, cs.levels, inline=True, fmt=dict(zip(cs.levels, p["labels"])), fontsize="small")
        else:
            print(f"locator_amd.plot: {p['sample']}: no density map (a prediction is not finite); "
                  "drawing the predictions only", file=sys.stderr)
        ax.scatter(p["xpred"], p["ypred"], s=1, color="#000000", label="Predicted Locations", zorder=3)
        tx, ty = true_location(truth, p["sample"]) if truth is not None else (np.nan, np.nan)
        if np.isfinite(tx) and np.isfinite(ty):
            ax.scatter([tx], [ty], s=40, color="#FF0000", label="Sample Location", zorder=4)
        if training is not None:
            ax.scatter(training[0], training[1], s=10, color="#1e90ff", label="Training Locations", zorder=3)
        ax.set_title(p["sample"], fontsize="small")
        h, lab = ax.get_legend_handles_labels()
        if len(h) > len(handles):
            handles, labels = h, lab
    for ax in flat[len(panels):]:
        ax.set_visible(False)
    if handles:
        fig.legend(handles, labels, loc="lower center", ncol=len(handles), fontsize="small")
    fig.set_size_inches(width, height)
    fig.savefig(out + ".pdf", format="pdf", bbox_inches="tight")
    plt.close(fig)
    return out + ".pdf"


# ---------------------------------------------------------------- command

def build_parser():
    p = argparse.ArgumentParser(prog="locator_amd.plot", description="Plot a summary of a set of locator predictions.")
    p.add_argument("--infile", required=True, help="directory holding the *predlocs* files")
    p.add_argument("--sample_data", default=None, help="sample file with known x / y (WGS1984 degrees for --basemap)")
    p.add_argument("--out", required=True, help="output stem: {out}.pdf, and {out}_centroids.txt with --error")
    p.add_argument("--width", default=10, type=float, help="figure width in inches (default 10)")
    p.add_argument("--height", default=8, type=float, help="figure height in inches (default 8)")
    p.add_argument("--samples", default=None, nargs="+", help="sample IDs to plot (default: --nsamples drawn at random)")
    p.add_argument("--nsamples", default=9, type=int, help="samples drawn when --samples is not given (default 9)")
    p.add_argument("--ncol", default=3, type=int, help="panels per row (default 3)")
    p.add_argument("--error", default=False, action="store_true",
                   help="summarise every sample, write {out}_centroids.txt and print the error statistics")
    p.add_argument("--basemap", default=False, action="store_true", help="draw country outlines from --map")
    p.add_argument("--map", default="map.zarr", help="basemap store (zarr v2; default map.zarr in the working directory)")
    p.add_argument("--longlat", default=False, action="store_true",
                   help="coordinates are longitude / latitude degrees: errors in great-circle km")
    p.add_argument("--silence", default=False, action="store_true", help="no terminal output")
    p.add_argument("--training_samples", default=None, help="sample file whose x / y are drawn as training locations")
    p.add_argument("--seed", default=None, type=int, help="seed of the --nsamples draw (default: unseeded)")
    p.add_argument("--host", default=False, action="store_true",
                   help="evaluate densities and summaries with NumPy instead of on the GPU")
    return p


def run(a):
    import pandas as pd
    if not a.host:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("locator_amd.plot: no GPU visible (the density maps are one loc_kde_grid_batch launch); "
                             "pass --host for the NumPy form")
    say = (lambda *m: None) if a.silence else print
    say("loading data")
    aeg = load_predlocs(a.infile)
    truth = read_truth(a.sample_data)
    basemap = read_basemap(a.map) if a.basemap else None
    bp = None
    if a.error:
        say("calculating error")
        bp = error_table(aeg, truth, host=a.host)
        bp.to_csv(a.out + "_centroids.txt", index=False, sep="\t")
        for line in error_lines(bp, a.longlat):
            say(line)
    training = None
    if a.training_samples:
        ts = pd.read_csv(a.training_samples, sep="\t")
        ok = np.isfinite(ts["x"].to_numpy(np.float64)) & np.isfinite(ts["y"].to_numpy(np.float64))
        training = (ts["x"].to_numpy(np.float64)[ok], ts["y"].to_numpy(np.float64)[ok])
    samples = pick_samples(aeg["sampleID"].unique(), a.samples, a.nsamples, a.seed)
    _, aspect = layout(len(samples), a.ncol, a.width, a.height)
    say("plotting")
    panels = panel_data(aeg, samples, aspect, host=a.host)
    pdf = draw(panels, a.out, a.ncol, a.width, a.height, truth, training, basemap)
    return panels, bp, pdf


def main(argv=None):
    run(build_parser().parse_args(argv))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
