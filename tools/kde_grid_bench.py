#!/usr/bin/env python3
"""Times one loc_kde_grid_batch launch (the plot command's density grids) at 9 panels (the command's default) and at 256
panels, each of 257 replicate predictions on a 370 x 530 grid (a bootstrap panel spread over tens of degrees: 50 M
haversine pairs), and the --host NumPy form on the same data.  One JSON line per size.

  python tools/kde_grid_bench.py [--panels 9,256] [--iters 5] [--host_panels 1]

Device time: events around the whole call (offset read-back + launch + kernel), median of --iters after a warm-up
launch.  Host time: kde_grid_host over the first --host_panels panels, scaled to pairs per second.  Both report
pair-evaluations per second; the host form's result is also compared with the device's."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from locator_amd import plot as P  # noqa: E402

NY, NX, NREP = 370, 530, 257


def make_panels(n, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        c = rng.uniform([-40, -120], [40, 120])
        pts = c + rng.normal(0, 1, (NREP, 2)) * [6.0, 8.0]
        lo, hi = pts.min(0) - 10, pts.max(0) + 10
        out.append((np.radians(pts[:, 0]), np.radians(pts[:, 1]), np.radians(np.linspace(lo[0], hi[0], NY)),
                    np.radians(np.linspace(lo[1], hi[1], NX))))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--panels", default="9,256")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--host_panels", type=int, default=1, help="panels the host form is timed on (0: skip)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kde_grid_bench needs a GPU"
    for n in (int(v) for v in a.panels.split(",")):
        panels = make_panels(n)
        pairs = n * NY * NX * NREP
        zs = P.kde_grids_device(panels)                     # warm-up: code object load, allocator
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            zs = P.kde_grids_device(panels)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        dev_ms = float(np.median(ms))
        rec = {"panels": n, "replicates": NREP, "grid": [NY, NX], "pairs": pairs, "device_ms_median": dev_ms,
               "device_ms_all": [round(v, 3) for v in ms], "device_pairs_per_s": pairs / (dev_ms * 1e-3)}
        if a.host_panels > 0:
            k = min(a.host_panels, n)
            t0 = time.perf_counter()
            zh = [P.kde_grid_host(*p) for p in panels[:k]]
            host_s = time.perf_counter() - t0
            err = max(float(np.max(np.abs(d - h) / h.max())) for d, h in zip(zs[:k], zh))
            rec.update({"host_panels_timed": k, "host_s": host_s, "host_pairs_per_s": k * NY * NX * NREP / host_s,
                        "host_s_extrapolated_all_panels": host_s * n / k, "max_abs_diff_over_max_z": err})
            rec["speedup_vs_host"] = rec["device_pairs_per_s"] / rec["host_pairs_per_s"]
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
