#!/usr/bin/env python3
"""`python -m locator_amd.regions`: which map region (country, park, population range) holds a sample's replicate
predictions, and with what support.

  python -m locator_amd.regions --infile out/boot --map map.zarr --out out/boot --sample_data samples.txt --longlat

The step after --windows / --bootstrap / --jacknife or several kept models, beside `summarize` and `plot`.  Every
`*predlocs*` file of --infile is read as they read it; each sample's kernel-density peak and centroid (summarize's), and
with --sample_data its true location, are assigned along with its replicates.

  regions     --map: a zarr-v2 store of [2][n] lon / lat outlines (the basemap of `plot`); each top-level group is a region
              and its arrays are the region's rings (a flat store: each array a region of one ring).  --regions: a
              tab-separated file `region part lon lat`, one vertex per line.
  membership  planar even-odd crossing number in float64, edges straight in the coordinates as given, the toggles counted
              over ALL rings of a region together (holes and enclave cuts given as rings of the region are outside);
              `assign_host` below is the definition, loc_region_assign (include/locator_hip_regions.h) the same bit for bit
  nearest     for a point in no region: the region of the nearest outline VERTEX (not edge) - Euclidean in map units, or
              with --longlat the great-circle distance in km; --snap D counts a replicate within D of it for that region

Outputs: {out}_region_support.txt (sampleID, region, n, support: one line per sample and region, `NA` = no region) and
{out}_regions.txt (one line per sample: the two best-supported regions, the regions of the kernel-density peak, the centroid
and the true location).  There is no silent fallback: without a GPU the run stops and says so; --host asks for the NumPy
form, which writes the same bytes.
"""
from __future__ import annotations

import argparse
import os
import sys
from collections import namedtuple

import numpy as np

from . import _abi
from ._files import write_atomic

TILE = _abi.LOC_REGION_TILE
STAGE = _abi.LOC_REGION_STAGE
NONE, NOT_FINITE = -1, -2           # region codes: in no region / a coordinate is not finite
X_PAD = 2.0 ** -40                  # relative padding of a ring box's x bounds (ring_boxes)

# names [n_regions]; parts [n_rings] = (region name, part name); verts [nv][2]; ring_off [n_rings + 1]; ring_region [n_rings]
# (never decreases); ring_bbox [n_rings][4]
RegionSet = namedtuple("RegionSet", "names parts verts ring_off ring_region ring_bbox")


# ---------------------------------------------------------------- readers

def ring_boxes(verts, ring_off):
    """[n_rings][4] = xmin, xmax, ymin, ymax of each ring, the boxes that assign_host and loc_region_assign cull by.

    The y bounds are the exact extremes: an edge is crossed only when ymin <= py < ymax, a comparison without rounding.
    The x bounds are padded.  A point right of every vertex must toggle nothing and a point left of every vertex must
    toggle every crossed edge (an even number around a ring), but t = (xj - xi) * (py - yi) / (yj - yi) + xi is rounded
    four times and can leave [min(xi, xj), max(xi, xj)] by a few units in the last place of X = max |x|: |py - yi| <=
    |yj - yi| survives rounding, so the quotient is at most |xj - xi| (1 + 2^-53)^3 and the sum adds one rounding more,
    under 2^-50 X in all.  The padding is 2^-40 X.  An empty ring gets (+inf, -inf, +inf, -inf): it misses everything."""
    verts, ring_off = np.asarray(verts, dtype=np.float64).reshape(-1, 2), np.asarray(ring_off, dtype=np.int64)
    box = np.empty((len(ring_off) - 1, 4), dtype=np.float64)
    for r, (a, b) in enumerate(zip(ring_off[:-1], ring_off[1:])):
        if b <= a:
            box[r] = (np.inf, -np.inf, np.inf, -np.inf)
            continue
        x, y = verts[a:b, 0], verts[a:b, 1]
        pad = max(abs(x.min()), abs(x.max())) * X_PAD
        box[r] = (x.min() - pad, x.max() + pad, y.min(), y.max())
    return box


def build_regions(rings):
    """(region, part, lon, lat) in any order -> RegionSet: regions in order of first appearance, a region's rings
    adjacent and in the order given.  A vertex that is not finite is an error that names the region and part."""
    by_region = {}
    for region, part, lon, lat in rings:
        lon, lat = np.asarray(lon, dtype=np.float64).ravel(), np.asarray(lat, dtype=np.float64).ravel()
        if len(lon) != len(lat):
            raise ValueError(f"region {region!r} part {part!r}: {len(lon)} longitudes and {len(lat)} latitudes")
        if not (np.isfinite(lon).all() and np.isfinite(lat).all()):
            raise ValueError(f"region {region!r} part {part!r}: a vertex is not finite")
        by_region.setdefault(str(region), []).append((str(part), lon, lat))
    names = list(by_region)
    parts, chunks, sizes, ring_region = [], [], [], []
    for k, name in enumerate(names):
        for part, lon, lat in by_region[name]:
            parts.append((name, part))
            chunks.append(np.stack([lon, lat], axis=1))
            sizes.append(len(lon))
            ring_region.append(k)
    verts = np.concatenate(chunks) if chunks else np.empty((0, 2))
    ring_off = np.zeros(len(sizes) + 1, dtype=np.int64)
    np.cumsum(sizes, out=ring_off[1:])
    verts = np.ascontiguousarray(verts, dtype=np.float64)
    return RegionSet(names, parts, verts, ring_off, np.asarray(ring_region, dtype=np.int32), ring_boxes(verts, ring_off))


def read_map(path):
    """The regions of a zarr-v2 map store (genotypes.walk_outlines: the walk plot.read_basemap draws from)."""
    from .genotypes import walk_outlines
    return build_regions(walk_outlines(path))


def read_regions_tsv(path):
    """The regions of a tab-separated file with header `region part lon lat`, one vertex per line in order.  Regions and
    parts are taken in order of first appearance; a part's lines must be adjacent."""
    with open(path) as fh:
        lines = fh.read().splitlines()
    if not lines:
        raise ValueError(f"{path}: empty file (needs the header `region part lon lat`)")
    header = lines[0].split("\t")
    missing = [c for c in ("region", "part", "lon", "lat") if c not in header]
    if missing:
        raise ValueError(f"{path}: missing column {', '.join(missing)} (header must be `region part lon lat`)")
    col = {c: header.index(c) for c in ("region", "part", "lon", "lat")}
    order, coords, last = [], {}, None
    for no, line in enumerate(lines[1:], start=2):
        if not line.strip():
            continue
        f = line.split("\t")
        if len(f) < len(header):
            raise ValueError(f"{path}: line {no} has {len(f)} fields, the header has {len(header)}")
        key = (f[col["region"]], f[col["part"]])
        try:
            xy = (float(f[col["lon"]]), float(f[col["lat"]]))
        except ValueError:
            raise ValueError(f"{path}: line {no}: lon / lat of region {key[0]!r} part {key[1]!r} is not a number") from None
        if key != last:
            if key in coords:
                raise ValueError(f"{path}: line {no}: part {key[1]!r} of region {key[0]!r} reappears after other parts "
                                 "(a part's vertices must be adjacent lines)")
            order.append(key)
            coords[key] = []
            last = key
        coords[key].append(xy)
    rings = []
    for key in order:
        xy = np.asarray(coords[key], dtype=np.float64)
        rings.append((key[0], key[1], xy[:, 0], xy[:, 1]))
    return build_regions(rings)


# ---------------------------------------------------------------- membership

def _ring_parity(px, py, x, y, chunk=1 << 22):
    """Odd number of toggles of the points against one ring (closed by last -> first): bool [len(px)].  The definition:
    for each edge i -> j with (y_i > py) != (y_j > py), t = (x_j - x_i) * (py - y_i) / (y_j - y_i) + x_i - NumPy rounds
    each operation once - and px < t toggles."""
    xj, yj = np.roll(x, -1), np.roll(y, -1)
    odd = np.zeros(len(px), dtype=bool)
    step = max(1, chunk // len(x))
    for a in range(0, len(px), step):
        qx, qy = px[a:a + step], py[a:a + step]
        above = y[None, :] > qy[:, None]
        pi, ei = np.nonzero(above != np.roll(above, -1, axis=1))
        t = (xj[ei] - x[ei]) * (qy[pi] - y[ei]) / (yj[ei] - y[ei]) + x[ei]
        odd[a:a + step] = (np.bincount(pi[qx[pi] < t], minlength=len(qx)) & 1).astype(bool)
    return odd


def assign_host(pts, verts, ring_off, ring_region, ring_bbox=None, n_regions=None):
    """(region, n_inside) int32 per point of pts [n][2]: the NumPy form of loc_region_assign and its definition.  region =
    the lowest region whose rings the point crosses an odd number of times (even-odd over all rings of the region), NONE
    when there is none, NOT_FINITE for a point with a coordinate that is not finite; n_inside = how many regions hold the
    point.  ring_bbox (ring_boxes) culls rings per point; None visits every ring for every point, with the same answers."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    verts = np.asarray(verts, dtype=np.float64).reshape(-1, 2)
    ring_off, ring_region = np.asarray(ring_off, dtype=np.int64), np.asarray(ring_region, dtype=np.int32)
    if len(ring_region) and (np.diff(ring_region) < 0).any():
        raise ValueError("assign_host: ring_region decreases (a region's rings must be adjacent)")
    if n_regions is not None and len(ring_region) and not (0 <= ring_region.min() and ring_region.max() < n_regions):
        raise ValueError(f"assign_host: a ring names a region outside 0..{n_regions - 1}")
    px, py = np.ascontiguousarray(pts[:, 0]), np.ascontiguousarray(pts[:, 1])
    finite = np.isfinite(px) & np.isfinite(py)
    region = np.full(len(pts), NONE, dtype=np.int32)
    n_inside = np.zeros(len(pts), dtype=np.int32)
    odd = np.zeros(len(pts), dtype=bool)
    cur = -1

    def flush():
        n_inside[odd] += 1
        region[odd & (region == NONE)] = cur
        odd[:] = False

    for r in range(len(ring_region)):
        if ring_region[r] != cur:
            flush()
            cur = int(ring_region[r])
        a, b = int(ring_off[r]), int(ring_off[r + 1])
        if b - a < 3:
            continue
        cand = finite
        if ring_bbox is not None:
            x0, x1, y0, y1 = ring_bbox[r]
            cand = finite & ~((px < x0) | (px > x1) | (py < y0) | (py > y1))
        idx = np.nonzero(cand)[0]
        if len(idx):
            odd[idx] ^= _ring_parity(px[idx], py[idx], verts[a:b, 0], verts[a:b, 1])
    flush()
    region[~finite] = NOT_FINITE
    return region, n_inside


def nearest_host(pts3, verts3, chunk=1 << 21):
    """(nearest int64, dist2 float64) per point of pts3 [m][3]: the first vertex of verts3 [nv][3] with the smallest
    ((dx * dx + dy * dy) + dz * dz), each operation rounded once - the NumPy form of loc_region_nearest."""
    pts3 = np.asarray(pts3, dtype=np.float64).reshape(-1, 3)
    verts3 = np.asarray(verts3, dtype=np.float64).reshape(-1, 3)
    if len(pts3) and not len(verts3):
        raise ValueError("nearest_host: points and no vertex")
    nearest = np.empty(len(pts3), dtype=np.int64)
    dist2 = np.empty(len(pts3), dtype=np.float64)
    step = max(1, chunk // max(len(verts3), 1))
    for a in range(0, len(pts3), step):
        d = verts3[None, :, :] - pts3[a:a + step, None, :]
        d2 = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
        k = np.argmin(d2, axis=1)                     # the first minimum, as strict < in index order keeps
        nearest[a:a + step] = k
        dist2[a:a + step] = d2[np.arange(len(k)), k]
    return nearest, dist2


def assign_device(pts, rs_or_verts, ring_off=None, ring_region=None, ring_bbox=None, n_regions=None, device="cuda:0"):
    """assign_host's answers from one loc_region_assign launch; takes a RegionSet or its arrays."""
    import torch
    from . import _device as D, _lib
    if isinstance(rs_or_verts, RegionSet):
        rs = rs_or_verts
        verts, ring_off, ring_region, ring_bbox, n_regions = rs.verts, rs.ring_off, rs.ring_region, rs.ring_bbox, len(rs.names)
    else:
        verts = rs_or_verts
    lib = _lib.load()
    pts = np.require(pts, dtype=np.float64, requirements=["C", "W"]).reshape(-1, 2)     # torch wants writable memory
    verts = np.ascontiguousarray(verts, dtype=np.float64).reshape(-1, 2)
    ring_off = np.ascontiguousarray(ring_off, dtype=np.int64)
    ring_region = np.ascontiguousarray(ring_region, dtype=np.int32)
    ring_bbox = np.ascontiguousarray(ring_boxes(verts, ring_off) if ring_bbox is None else ring_bbox, dtype=np.float64)
    n_rings = len(ring_region)
    if len(ring_off) != n_rings + 1 or ring_bbox.shape != (n_rings, 4) or (n_rings and int(ring_off[-1]) > len(verts)):
        raise ValueError("assign_device: ring_off needs n_rings + 1 entries that end within verts, ring_bbox n_rings x 4")
    if n_regions is None:
        n_regions = int(ring_region.max()) + 1 if n_rings else 0
    with torch.cuda.device(device):
        d = [D.put(a, None, device) for a in (pts, verts, ring_off, ring_region, ring_bbox)]
        d_reg = torch.empty(max(len(pts), 1), dtype=torch.int32, device=device)
        d_cnt = torch.empty(max(len(pts), 1), dtype=torch.int32, device=device)
        _lib.check(lib.loc_region_assign(d[0].data_ptr(), len(pts), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                         d[4].data_ptr(), n_rings, int(n_regions), d_reg.data_ptr(), d_cnt.data_ptr(),
                                         D.stream()), "loc_region_assign")
        return d_reg.cpu().numpy()[:len(pts)], d_cnt.cpu().numpy()[:len(pts)]


def nearest_device(pts3, verts3, device="cuda:0"):
    """nearest_host's answers from one loc_region_nearest launch."""
    import torch
    from . import _device as D, _lib
    lib = _lib.load()
    pts3 = np.ascontiguousarray(pts3, dtype=np.float64).reshape(-1, 3)
    verts3 = np.ascontiguousarray(verts3, dtype=np.float64).reshape(-1, 3)
    with torch.cuda.device(device):
        d_p, d_v = D.put(pts3, np.float64, device), D.put(verts3, np.float64, device)
        d_k = torch.empty(max(len(pts3), 1), dtype=torch.int64, device=device)
        d_d = torch.empty(max(len(pts3), 1), dtype=torch.float64, device=device)
        _lib.check(lib.loc_region_nearest(d_p.data_ptr(), len(pts3), d_v.data_ptr(), len(verts3), d_k.data_ptr(),
                                          d_d.data_ptr(), D.stream()), "loc_region_nearest")
        return d_k.cpu().numpy()[:len(pts3)], d_d.cpu().numpy()[:len(pts3)]


# ---------------------------------------------------------------- nearest region

def wrap_longitude(lon):
    """Longitudes in degrees wrapped to [-180, 180)."""
    return np.mod(np.asarray(lon, dtype=np.float64) + 180.0, 360.0) - 180.0


def unit_vectors(lon, lat):
    """[n][3] unit vectors (cos lat cos lon, cos lat sin lon, sin lat) of longitude / latitude in degrees."""
    lon, lat = np.radians(np.asarray(lon, dtype=np.float64)), np.radians(np.asarray(lat, dtype=np.float64))
    return np.stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)], axis=1)


def nearest_inputs(xy, longlat):
    """[n][3] coordinates that the nearest-vertex search runs in: (x, y, 0), or unit vectors with longlat."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    if longlat:
        return unit_vectors(xy[:, 0], xy[:, 1])
    return np.concatenate([xy, np.zeros((len(xy), 1))], axis=1)


def nearest_distance(dist2, longlat):
    """The nearest vertex's distance from its squared distance: map units, or with longlat the great-circle km of the
    chord between the two unit vectors."""
    from .plot import EARTH_KM
    d = np.sqrt(np.asarray(dist2, dtype=np.float64))
    return 2.0 * EARTH_KM * np.arcsin(np.minimum(d / 2.0, 1.0)) if longlat else d


def nearest_regions(xy, rs, longlat=False, host=False):
    """(region index, distance) of the nearest outline vertex of each point of xy [n][2]."""
    if len(xy) == 0:
        return np.empty(0, dtype=np.int64), np.empty(0)
    find = nearest_host if host else nearest_device
    k, d2 = find(nearest_inputs(xy, longlat), nearest_inputs(rs.verts, longlat))
    ring = np.searchsorted(rs.ring_off, k, side="right") - 1        # past empty rings: the ring that holds vertex k
    return rs.ring_region[ring].astype(np.int64), nearest_distance(d2, longlat)


# ---------------------------------------------------------------- tables

def _fmt(v):
    return "NA" if v is None else (repr(float(v)) if isinstance(v, (float, np.floating)) else str(v))


def _write_table(path, header, rows):
    write_atomic(path, "".join("\t".join(_fmt(v) for v in row) + "\n" for row in [header] + rows))


def regions(indir, rs, out=None, sample_data=None, longlat=False, snap=0.0, bandwidth=0.2, host=False, silence=False):
    """The command's work for a RegionSet `rs`: returns (support rows, sample rows, printed lines) and writes
    {out}_region_support.txt / {out}_regions.txt when `out` is given."""
    from . import plot as P
    from . import summarize as S
    if not host:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("locator_amd.regions: no GPU visible (membership is one loc_region_assign launch); "
                             "pass --host for the NumPy form")
    aeg = P.load_predlocs(indir)
    truth = P.read_truth(sample_data)
    groups = [(sid, g["xpred"].to_numpy(np.float64), g["ypred"].to_numpy(np.float64))
              for sid, g in aeg.groupby("sampleID", sort=False)]
    ns = len(groups)
    if host:
        summ = np.array([S.kde_peak(x, y, bandwidth) + S.centroid(x, y) for _, x, y in groups]).reshape(ns, 4)
    else:
        summ = S.device_summaries([(x, y) for _, x, y in groups], bandwidth)[1]
    counts = np.array([len(x) for _, x, _ in groups], dtype=np.int64)
    off = np.zeros(ns + 1, dtype=np.int64)
    np.cumsum(counts, out=off[1:])
    nrep = int(off[-1])
    # one array of points, sample-major: every sample's replicates, then the peaks, the centroids and the true locations
    pts = np.empty((nrep + ns * (3 if truth is not None else 2), 2), dtype=np.float64)
    for (_, x, y), a, b in zip(groups, off[:-1], off[1:]):
        pts[a:b, 0], pts[a:b, 1] = x, y
    pts[nrep:nrep + ns] = summ[:, 0:2]
    pts[nrep + ns:nrep + 2 * ns] = summ[:, 2:4]
    if truth is not None:
        pts[nrep + 2 * ns:] = [P.true_location(truth, sid) for sid, _, _ in groups]
    if longlat:
        pts[:, 0] = wrap_longitude(pts[:, 0])
    if host:
        reg, n_in = assign_host(pts, rs.verts, rs.ring_off, rs.ring_region, rs.ring_bbox, len(rs.names))
    else:
        reg, n_in = assign_device(pts, rs)
    near_reg = np.full(len(pts), NONE, dtype=np.int64)
    near_dist = np.full(len(pts), np.nan)
    lost = np.nonzero(reg == NONE)[0]
    if len(lost) and len(rs.verts):
        near_reg[lost], near_dist[lost] = nearest_regions(pts[lost], rs, longlat, host)
    eff = reg.astype(np.int64)
    if snap > 0:
        take = (reg == NONE) & (near_reg >= 0) & (near_dist <= snap)
        take[nrep:] = False                          # the support tables only: a summary point keeps its own answer
        eff[take] = near_reg[take]

    def name(k):
        return rs.names[int(k)] if k >= 0 else None

    support, samples = [], []
    for s, (sid, _, _) in enumerate(groups):
        e = eff[off[s]:off[s + 1]]
        n_finite = int((e != NOT_FINITE).sum())
        ks, ns_k = np.unique(e[e >= 0], return_counts=True)
        ranked = sorted(((int(c), rs.names[int(k)]) for k, c in zip(ks, ns_k)), key=lambda t: (-t[0], t[1]))
        for c, nm in ranked:
            support.append([sid, nm, c, c / n_finite])
        n_na = int((e == NONE).sum())
        if n_na:
            support.append([sid, None, n_na, n_na / n_finite])
        top = ranked[0] if ranked else (None, None)
        second = ranked[1] if len(ranked) > 1 else (None, None)
        kd, gc = nrep + s, nrep + ns + s
        row = [sid, int(counts[s]), n_finite, top[1], None if top[0] is None else top[0] / n_finite, second[1],
               None if second[0] is None else second[0] / n_finite, name(reg[kd]), name(reg[gc]),
               name(near_reg[kd]) if reg[kd] == NONE else None,
               float(near_dist[kd]) if reg[kd] == NONE and near_reg[kd] >= 0 else None]
        if truth is not None:
            row.append(name(reg[nrep + 2 * ns + s]))
        samples.append(row)

    lines = [f"{ns} samples, {nrep} replicate predictions; {len(rs.names)} regions, {len(rs.ring_region)} rings, "
             f"{len(rs.verts)} vertices"]
    rep_fin = reg[:nrep] != NOT_FINITE
    n_fin = int(rep_fin.sum())
    lines.append("share of replicates in no region = " + (str(float((eff[:nrep] == NONE).sum() / n_fin)) if n_fin else "NA"))
    lines.append(f"points in more than one region (counted for the lowest) = {int((n_in > 1).sum())}")
    tops = [r[4] for r in samples if r[4] is not None]
    lines.append("mean top_support = " + (str(float(np.mean(tops))) if tops else "NA"))
    if truth is not None:
        known = [r for r in samples if r[11] is not None]
        lines.append(f"samples whose true location lies in a region = {len(known)}")
        for label, c in (("top_region", 3), ("kd_region", 7), ("gc_region", 8)):
            share = str(float(np.mean([r[c] == r[11] for r in known]))) if known else "NA"
            lines.append(f"share with {label} = true_region: {share}")
    if out is not None:
        _write_table(out + "_region_support.txt", ["sampleID", "region", "n", "support"], support)
        header = ["sampleID", "n_reps", "n_finite", "top_region", "top_support", "second_region", "second_support",
                  "kd_region", "gc_region", "kd_nearest_region", "kd_nearest_dist"]
        _write_table(out + "_regions.txt", header + (["true_region"] if truth is not None else []), samples)
    if not silence:
        for line in lines:
            print(line)
    return support, samples, lines


# ---------------------------------------------------------------- command

def build_parser():
    p = argparse.ArgumentParser(prog="locator_amd.regions",
                                description="Assign replicate predictions to map regions and report each region's support.")
    p.add_argument("--infile", required=True, help="directory holding the *predlocs* files")
    p.add_argument("--out", required=True, help="output stem: {out}_region_support.txt and {out}_regions.txt")
    p.add_argument("--map", default=None, help="zarr-v2 store of [2][n] lon / lat outlines: each top-level group a region, "
                                               "its arrays the region's rings (the basemap store of the plot command)")
    p.add_argument("--regions", default=None, help="tab-separated polygons `region part lon lat`, one vertex per line; "
                                                   "a region's parts are its rings")
    p.add_argument("--sample_data", default=None, help="sample file with known x / y: adds true_region and the accuracy lines")
    p.add_argument("--longlat", default=False, action="store_true",
                   help="coordinates are longitude / latitude degrees: longitudes are wrapped to [-180, 180) and nearest "
                        "distances are great-circle km (membership stays planar, edges straight in degrees)")
    p.add_argument("--snap", default=0.0, type=float, metavar="D",
                   help="count a replicate in no region for the region of its nearest outline vertex when that vertex is "
                        "within D (km with --longlat, else map units; default 0 = off).  The distance is to the nearest "
                        "VERTEX of an outline, not to its nearest edge")
    p.add_argument("--bandwidth", default=0.2, type=float, help="bandwidth of the kernel-density peak (default 0.2)")
    p.add_argument("--host", default=False, action="store_true", help="the NumPy form instead of the GPU (same files)")
    p.add_argument("--gpu_number", default=None, type=str, help="the GPU to use (sets HIP_VISIBLE_DEVICES)")
    p.add_argument("--silence", default=False, action="store_true", help="no terminal output")
    return p


def main(argv=None):
    parser = build_parser()
    a = parser.parse_args(argv)
    if (a.map is None) == (a.regions is None):
        parser.error("exactly one of --map / --regions must be given")
    if a.snap < 0 or not np.isfinite(a.snap):
        parser.error("--snap must be a finite distance >= 0")
    if a.gpu_number is not None:
        for var in ("HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
            os.environ[var] = a.gpu_number
    try:
        rs = read_map(a.map) if a.map is not None else read_regions_tsv(a.regions)
    except (ValueError, FileNotFoundError) as e:
        raise SystemExit(f"locator_amd.regions: {e}") from None
    regions(a.infile, rs, a.out, a.sample_data, a.longlat, a.snap, a.bandwidth, a.host, a.silence)
    return 0


if __name__ == "__main__":
    sys.exit(main())
