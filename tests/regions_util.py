"""Shared inputs of tests/test_regions.py (host) and tests/test_gpu_regions.py (device): the fixture map, its seeded probe
points, star-shaped rings, hand-written ring sets and a hand-made directory of predlocs files."""
import functools
import os

import numpy as np

from locator_amd import regions as R

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE_MAP = os.path.join(HERE, "golden", "regions_map_zarr")
FLAT_MAP = os.path.join(HERE, "golden", "blosc_map_zarr")
SEED = 20240611


@functools.lru_cache(maxsize=None)
def fixture_regions():
    return R.read_map(FIXTURE_MAP)


@functools.lru_cache(maxsize=None)
def fixture_points(n=20000):
    """n seeded uniform points in the fixture map's bounding box, then the vertex mean of every ring, then 200 uniform
    points in each ring's own box (the map's box spans Fiji to Italy and is mostly sea: these are the points near outlines)."""
    rs = fixture_regions()
    rng = np.random.default_rng(SEED)
    lo, hi = rs.verts.min(axis=0), rs.verts.max(axis=0)
    pts = rng.uniform(lo, hi, (n, 2))
    rings = [rs.verts[a:b] for a, b in zip(rs.ring_off[:-1], rs.ring_off[1:])]
    centres = [v.mean(axis=0) for v in rings]
    near = [rng.uniform(v.min(axis=0), v.max(axis=0), (200, 2)) for v in rings]
    pts = np.concatenate([pts, np.asarray(centres)] + near)
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def fixture_answers():
    """assign_host on fixture_points, computed once."""
    rs = fixture_regions()
    reg, cnt = R.assign_host(fixture_points(), rs.verts, rs.ring_off, rs.ring_region, rs.ring_bbox, len(rs.names))
    reg.setflags(write=False)
    cnt.setflags(write=False)
    return reg, cnt


def star(m, cx=0.0, cy=0.0, r0=1.0, r1=2.0, closed=False, phase=0.1):
    """A star-shaped ring of m vertices (radius alternating r0 / r1) around (cx, cy); closed repeats vertex 0, so that
    the ring still has m vertices it turns through m - 1 of them."""
    k = m - 1 if closed else m
    a = phase + 2 * np.pi * np.arange(k) / k
    r = np.where(np.arange(k) % 2 == 0, r1, r0)
    xy = np.stack([cx + r * np.cos(a), cy + r * np.sin(a)], axis=1)
    return np.concatenate([xy, xy[:1]]) if closed else xy


def ring_set(rings, ring_region):
    """(verts, ring_off, ring_region, ring_bbox) of a list of [m][2] rings."""
    rings = [np.asarray(r, dtype=np.float64).reshape(-1, 2) for r in rings]
    verts = np.concatenate(rings) if rings else np.empty((0, 2))
    off = np.zeros(len(rings) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rings], out=off[1:])
    return verts, off, np.asarray(ring_region, dtype=np.int32), R.ring_boxes(verts, off)


def square(x0, y0, x1, y1, closed=False):
    xy = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
    return np.asarray(xy + xy[:1] if closed else xy, dtype=np.float64)


QUADRANTS = {"NE": (0, 0, 10, 10), "NW": (-10, 0, 0, 10), "SW": (-10, -10, 0, 0), "SE": (0, -10, 10, 0)}


def write_quadrants_tsv(path):
    """Four quadrant regions of the square -10..10, as a --regions file."""
    with open(path, "w") as fh:
        fh.write("region\tpart\tlon\tlat\n")
        for name, box in QUADRANTS.items():
            for x, y in square(*box):
                fh.write(f"{name}\t{name}_0\t{float(x)!r}\t{float(y)!r}\n")
    return path


def write_predlocs(d, with_truth=True):
    """A hand-made run: 4 replicate files of 5 samples.  a: all four in NE.  b: 3 in NW, 1 in SW.  c: 2 in SE, 1 in NE, 1
    outside at (10.5, -5).  d: 1 in SW, 2 far outside, 1 with a NaN coordinate.  e_h0: a haplotype row of sample e, 2 in NE
    and 2 in SE (a tie that the name breaks).  Returns the sample file's path."""
    import pandas as pd
    reps = {
        "a": [(5.0, 5.0), (5.2, 5.1), (4.9, 5.3), (5.1, 4.8)],
        "b": [(-5.0, 5.0), (-5.5, 4.0), (-4.0, 6.0), (-5.0, -1.0)],
        "c": [(5.0, -5.0), (6.0, -5.5), (5.0, 1.0), (10.5, -5.0)],
        "d": [(-3.0, -3.0), (40.0, 40.0), (41.0, 40.0), (np.nan, 1.0)],
        "e_h0": [(2.0, 2.0), (3.0, 3.0), (2.0, -2.0), (3.0, -3.0)],
    }
    os.makedirs(d, exist_ok=True)
    for f in range(4):
        ids = list(reps)
        pd.DataFrame({"x": [reps[s][f][0] for s in ids], "y": [reps[s][f][1] for s in ids], "sampleID": ids}).to_csv(
            os.path.join(d, f"boot{f}_predlocs.txt"), index=False)
    sd = os.path.join(d, "samples.txt")
    if with_truth:
        # a: in NE (right).  b: in SW (top is NW: wrong).  c: unknown.  d: outside every region.  e: in SE
        pd.DataFrame({"sampleID": ["a", "b", "c", "d", "e"], "x": [5.0, -5.0, np.nan, 50.0, 2.0],
                      "y": [5.0, -5.0, np.nan, 50.0, -2.0]}).to_csv(sd, sep="\t", index=False, na_rep="NA")
    return sd


def write_predlocs_fixture(d, n_files=12):
    """Replicates around places on the fixture map (degrees): inside Lesotho, in South Africa near Lesotho's border, in
    San Marino, in Italy, on Fiji across the date line (longitudes past 180 that --longlat wraps), and off shore."""
    import pandas as pd
    rng = np.random.default_rng(SEED + 1)
    centres = {"les": (28.3, -29.5), "zaf": (27.0, -29.2), "smr": (12.46, 43.94), "ita": (12.0, 43.0),
               "fji": (179.9, -16.6), "sea": (15.0, -38.0)}
    spread = {"les": 0.4, "zaf": 0.6, "smr": 0.03, "ita": 0.8, "fji": 0.6, "sea": 1.5}
    os.makedirs(d, exist_ok=True)
    ids = list(centres)
    for f in range(n_files):
        xy = np.array([rng.normal(centres[s], spread[s]) for s in ids])
        pd.DataFrame({"x": xy[:, 0], "y": xy[:, 1], "sampleID": ids}).to_csv(os.path.join(d, f"w{f:02d}_predlocs.txt"),
                                                                              index=False)
    sd = os.path.join(d, "samples.txt")
    pd.DataFrame({"sampleID": ids, "x": [centres[s][0] for s in ids], "y": [centres[s][1] for s in ids]}).to_csv(
        sd, sep="\t", index=False)
    return sd
