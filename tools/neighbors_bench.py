#!/usr/bin/env python3
"""Time loc_ibs_pairs (csrc/ibs_kernels.hip) on synthetic allele counts: --rows samples (default 1,000 and 4,096) x --sites
sites (100,000), --missing of the calls missing (2 %), a site's allele frequency uniform in 0.05 .. 0.5.  Everything is
generated here from --seed.  Writes one JSON object (and prints it) with one entry per row count: the median of --launches
event-timed launches, the int8 multiply-adds the launch executes (tile pairs x 128 x 128 x padded sites x 5 products) per
second, that rate as a fraction of the i8 rate this project measured as sustainable (3,557 TOP/s,
profiles/r03_mfma_clock_probe.jsonl; one multiply-add = 2 operations), the device path end to end with its transfers
(neighbors.pairs_device, median of 3), and the NumPy definition on --sub rows against all rows scaled to all pairs.  The device
answers are checked against the definition on those rows."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from locator_amd import _lib  # noqa: E402
from locator_amd import baselines as BL  # noqa: E402
from locator_amd import neighbors as NB  # noqa: E402

I8_SUSTAINED_TOPS = 3557.0


def host_rows(c, rows):
    """The definition for the pairs (i, every j), i in rows: the row step of neighbors.pairs_host."""
    called = c >= 0
    d, n = np.zeros((len(rows), len(c)), dtype=np.int32), np.zeros((len(rows), len(c)), dtype=np.int32)
    for r, i in enumerate(rows):
        both = called & called[i]
        d[r] = np.sum(np.abs(c - c[i]), axis=1, dtype=np.int32, where=both)
        n[r] = np.sum(both, axis=1, dtype=np.int32)
    return d, n


def one(N, K, missing, launches, sub, k_groups, rng):
    freq = rng.uniform(0.05, 0.5, (1, K))
    c = rng.binomial(2, np.broadcast_to(freq, (N, K))).astype(np.int8)
    c[rng.random((N, K)) < missing] = -1
    lib = _lib.load()
    buf = BL.padded(c)
    d_c = torch.from_numpy(buf).cuda()
    d_d = torch.empty((N, N), dtype=torch.int32, device="cuda")
    d_n = torch.empty_like(d_d)
    stream = torch.cuda.current_stream().cuda_stream

    def launch():
        _lib.check(lib.loc_ibs_pairs(d_c.data_ptr(), N, K, buf.shape[1], k_groups, d_d.data_ptr(), d_n.data_ptr(), None, 0,
                                     stream), "loc_ibs_pairs")
    for _ in range(3):                                                     # warm-up (code object load, clocks)
        launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    ms = float(np.median(times))
    d, n = d_d.cpu().numpy(), d_n.cpu().numpy()

    walls = []
    for _ in range(3):                                                     # upload, launch, two downloads
        t0 = time.perf_counter()
        got = NB.pairs_device(c, k_groups=k_groups)
        walls.append(time.perf_counter() - t0)
    assert np.array_equal(got[0], d) and np.array_equal(got[1], n)

    rows = np.linspace(0, N - 1, sub).astype(np.int64)
    t0 = time.perf_counter()
    want = host_rows(c, rows)
    host_s = time.perf_counter() - t0
    assert np.array_equal(d[rows], want[0]) and np.array_equal(n[rows], want[1]), "device != definition"

    tiles = (N + NB.TILE - 1) // NB.TILE
    pairs = tiles * (tiles + 1) // 2
    macs = pairs * NB.TILE * NB.TILE * ((K + NB.BLOCK - 1) // NB.BLOCK * NB.BLOCK) * 5
    tops = 2 * macs / (ms * 1e-3) / 1e12
    host_full = host_s * N / len(rows)
    e2e = float(np.median(walls))
    return {"rows": N, "sites": K, "missing": missing, "tile_pairs": pairs, "k_groups": k_groups,
            "kernel_median_ms": round(ms, 4), "kernel_min_ms": round(float(min(times)), 4), "int8_multiply_adds": macs,
            "kernel_tera_multiply_adds_per_s": round(macs / (ms * 1e-3) / 1e12, 2), "kernel_tops": round(tops, 1),
            "fraction_of_sustained_i8": round(tops / I8_SUSTAINED_TOPS, 4),
            "useful_pair_sites_per_s": round(N * (N - 1) / 2 * K / (ms * 1e-3), 1),
            "device_end_to_end_ms": round(e2e * 1e3, 2), "host_rows": len(rows), "host_s_on_those": round(host_s, 3),
            "host_s_scaled_to_all_rows": round(host_full, 1), "device_end_to_end_speedup": round(host_full / e2e, 1),
            "device_matches_definition_on_those_rows": True}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1000, 4096])
    ap.add_argument("--sites", type=int, default=100_000)
    ap.add_argument("--missing", type=float, default=0.02)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--sub", type=int, default=4, help="the definition runs on this many rows against all rows")
    ap.add_argument("--k_groups", type=int, default=0, help="0 = the launcher's choice")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "neighbors_bench.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    out = {"kernel": "loc_ibs_pairs", "device": torch.cuda.get_device_name(0), "i8_sustained_tops": I8_SUSTAINED_TOPS,
           "runs": [one(N, a.sites, a.missing, a.launches, a.sub, a.k_groups, rng) for N in a.rows]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
