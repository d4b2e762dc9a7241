#!/usr/bin/env python3
"""Time loc_region_assign (csrc/region_kernels.hip) on a synthetic map of a world basemap's shape: --rings star-shaped rings
(default 2,128) in --regions regions (251), --vertices vertices in all (237,488), ring sizes from 4 to --longest (12,905), and
--samples x --reps points (1,000 x 256) clustered per sample around places on the outlines.  Everything is generated here
from --seed.  Writes one JSON object (and prints it): the median of --launches event-timed launches, the device path end to
end with its transfers (regions.assign_device, median of 5), the NumPy host form on every --sub-th point scaled to the full
count, and the edge tests that survive the per-point culling, per second of each.  The device answers are checked against the
host form on that subsample."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from locator_amd import _lib  # noqa: E402
from locator_amd import regions as R  # noqa: E402


def ring_sizes(rng, n_rings, total, longest):
    """n_rings sizes >= 4 with the given sum, one of them `longest`, one 4: skewed as coastlines are (most rings are islets)."""
    w = rng.lognormal(0.0, 1.6, n_rings - 2)
    rest = total - longest - 4
    sizes = np.maximum(4, np.floor(w / w.sum() * rest).astype(np.int64))
    sizes = np.minimum(sizes, longest)
    k = 0
    while sizes.sum() != rest:                         # hand the rounding remainder out one vertex at a time
        step = 1 if sizes.sum() < rest else -1
        if 4 <= sizes[k % len(sizes)] + step <= longest:
            sizes[k % len(sizes)] += step
        k += 1
    return np.concatenate([[longest], sizes, [4]])


def synthetic_map(rng, n_rings, n_regions, total, longest):
    sizes = ring_sizes(rng, n_rings, total, longest)
    owner = np.sort(np.concatenate([np.arange(n_regions), rng.integers(0, n_regions, n_rings - n_regions)]))
    centre = np.stack([rng.uniform(-170, 170, n_regions), rng.uniform(-60, 75, n_regions)], axis=1)
    rings = []
    for m, k in zip(sizes, owner):
        radius = 0.03 * np.sqrt(m)                     # degrees: 12,905 vertices -> 3.4, 4 vertices -> 0.06
        c = centre[k] + rng.normal(0, 2.5, 2)
        a = rng.uniform(0, 2 * np.pi) + 2 * np.pi * np.arange(m) / m
        r = radius * np.where(np.arange(m) % 2 == 0, 1.0, rng.uniform(0.6, 0.95))
        rings.append((f"r{k}", f"r{k}_{len(rings)}", c[0] + r * np.cos(a), c[1] + r * np.sin(a)))
    return R.build_regions(rings)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rings", type=int, default=2128)
    ap.add_argument("--regions", type=int, default=251)
    ap.add_argument("--vertices", type=int, default=237_488)
    ap.add_argument("--longest", type=int, default=12_905)
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=256)
    ap.add_argument("--spread", type=float, default=1.0, help="standard deviation of a sample's replicates, degrees")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--sub", type=int, default=64, help="the host form runs on every sub-th point")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "regions_bench.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    rs = synthetic_map(rng, a.rings, a.regions, a.vertices, a.longest)
    sizes = np.diff(rs.ring_off)
    assert len(rs.names) == a.regions and len(sizes) == a.rings and len(rs.verts) == a.vertices
    assert sizes.min() == 4 and sizes.max() == a.longest
    home = rs.verts[rng.integers(0, len(rs.verts), a.samples)]             # each sample lives on some outline
    pts = (home[:, None, :] + rng.normal(0, a.spread, (a.samples, a.reps, 2))).reshape(-1, 2)
    n = len(pts)

    # edge tests: every pair, and those left by the per-point culling (a point meets a ring only inside the ring's box)
    survive = 0
    for m, (x0, x1, y0, y1) in zip(sizes, rs.ring_bbox):
        survive += int(m) * int(((pts[:, 0] >= x0) & (pts[:, 0] <= x1) & (pts[:, 1] >= y0) & (pts[:, 1] <= y1)).sum())

    lib = _lib.load()
    d = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (pts, rs.verts, rs.ring_off, rs.ring_region, rs.ring_bbox)]
    d_reg = torch.empty(n, dtype=torch.int32, device="cuda")
    d_cnt = torch.empty(n, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def launch():
        _lib.check(lib.loc_region_assign(d[0].data_ptr(), n, d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(),
                                         a.rings, a.regions, d_reg.data_ptr(), d_cnt.data_ptr(), stream), "loc_region_assign")
    for _ in range(3):                                                     # warm-up (code object load)
        launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    ms = float(np.median(times))
    reg = d_reg.cpu().numpy()
    cnt = d_cnt.cpu().numpy()

    walls = []
    for _ in range(5):                                                     # uploads, the offsets' read-back, launch, downloads
        t0 = time.perf_counter()
        got = R.assign_device(pts, rs)
        walls.append(time.perf_counter() - t0)
    assert np.array_equal(got[0], reg) and np.array_equal(got[1], cnt)

    sub = pts[::a.sub]
    t0 = time.perf_counter()
    want = R.assign_host(sub, rs.verts, rs.ring_off, rs.ring_region, rs.ring_bbox, a.regions)
    host_s = time.perf_counter() - t0
    assert np.array_equal(reg[::a.sub], want[0]) and np.array_equal(cnt[::a.sub], want[1]), "device != host form"

    host_full = host_s * n / len(sub)
    e2e = float(np.median(walls))
    out = {"kernel": "loc_region_assign", "regions": a.regions, "rings": a.rings, "vertices": a.vertices,
           "longest_ring": a.longest, "points": n, "points_in_a_region": int((reg >= 0).sum()),
           "points_in_several": int((cnt > 1).sum()), "edge_tests_all_pairs": int(n) * int(a.vertices),
           "edge_tests_after_culling": survive, "kernel_median_ms": round(ms, 4), "kernel_min_ms": round(float(min(times)), 4),
           "kernel_edge_tests_per_s": round(survive / (ms * 1e-3), 1), "device_end_to_end_ms": round(e2e * 1e3, 3),
           "host_points": len(sub), "host_s_on_those": round(host_s, 4), "host_s_scaled_to_all": round(host_full, 3),
           "host_edge_tests_per_s": round(survive / host_full, 1), "device_end_to_end_speedup": round(host_full / e2e, 1),
           "device_matches_host_on_subsample": True}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
