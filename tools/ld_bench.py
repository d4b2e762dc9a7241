#!/usr/bin/env python3
"""Time loc_ld_band (csrc/ld_kernels.hip) on synthetic site-major allele counts: --sites sites (100,000) x --samples samples
(1,000 and 4,096), --missing of the calls missing (2 %), windows --windows (100 and 512), the mask alone (no sums, no r2).  Every
second site is a copy of the site before it with 5 % of its entries redrawn, so that the mask is not empty and the greedy
walk removes sites.  Everything is generated here from --seed.  Writes one JSON object (and prints it) with one entry per
(samples, window): twice the median of --launches event-timed launches; the int8 multiply-adds the launch executes (the
32 x 32 quadrants of the band's tile pairs that hold a pair of the band x 32 x 32 x padded samples x 6 products) per second and
as a fraction of the i8 rate this project measured as sustainable (3,557 TOP/s, profiles/r03_mfma_clock_probe.jsonl; one
multiply-add = 2 operations); interleaved with it (a) what one would write without a kernel: the three planes materialised
as fp32 tensors and per block of --torch_rows sites six torch.matmul products against the sites of the block's windows, r2 in
float64 and the comparison (exact while the sums stay below 2^24; no band extraction and no bit packing, which would only add
to it); (b) the NumPy definition on --sub rows, scaled to all rows, which the device mask is checked against; the ld command's
work end to end on that input (upload, launch, download, greedy walk, files) and the host greedy walk alone."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from locator_amd import _lib  # noqa: E402
from locator_amd import baselines as BL  # noqa: E402
from locator_amd import ld as LD  # noqa: E402

I8_SUSTAINED_TOPS = 3557.0


def synth(K, N, missing, rng):
    freq = rng.uniform(0.05, 0.5, ((K + 1) // 2, 1))
    base = rng.binomial(2, np.broadcast_to(freq, ((K + 1) // 2, N))).astype(np.int8)
    ct = np.repeat(base, 2, axis=0)[:K]
    redraw = rng.random((K, N)) < 0.05
    redraw[0::2] = False
    ct[redraw] = rng.integers(0, 3, int(redraw.sum()), dtype=np.int8)
    ct[rng.random((K, N)) < missing] = -1
    return ct


def quadrants(K, W):
    """The 32 x 32 quadrants whose MFMAs a launch issues: those of tile pairs inside the array that hold a pair with
    1 <= j - i <= W (ld_band_kernel's `live`)."""
    T = LD.TILE
    tiles = (K + T - 1) // T
    total = 0
    for d in range((T - 1 + W) // T + 1):
        live = sum(1 for qi in (0, 32) for qj in (0, 32) if T * d + qj + 31 - qi >= 1 and T * d + qj - qi - 31 <= W)
        total += live * max(tiles - d, 0)
    return total


def torch_band(planes, W, thr, rows):
    """(a): the mask's ingredients without a kernel; returns the number of over pairs it saw (band and not)."""
    m, a, a2 = planes
    K = len(m)
    seen = 0
    for i0 in range(0, K, rows):
        i1, j1 = min(K, i0 + rows), min(K, i0 + rows + W)
        mi, ai, qi, mj, aj, qj = m[i0:i1], a[i0:i1], a2[i0:i1], m[i0 + 1:j1].T, a[i0 + 1:j1].T, a2[i0 + 1:j1].T
        n, sa, sb, sab, saa, sbb = (x.double() for x in (mi @ mj, ai @ mj, mi @ aj, ai @ aj, qi @ mj, mi @ qj))
        cov, va, vb = n * sab - sa * sb, n * saa - sa * sa, n * sbb - sb * sb
        r2 = (cov * cov) / (va * vb)
        seen += int(((r2 > thr) & (n >= 2) & (va > 0) & (vb > 0)).sum())
    return seen


def one(ct, W, thr, launches, sub, torch_rows):
    K, N = ct.shape
    lib = _lib.load()
    buf = BL.padded(ct)
    d_ct = torch.from_numpy(buf).cuda()
    words = (W + 31) // 32
    d_over = torch.empty((K, words), dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def launch():
        _lib.check(lib.loc_ld_band(d_ct.data_ptr(), K, N, buf.shape[1], W, None, thr, d_over.data_ptr(), None, None, stream),
                   "loc_ld_band")

    planes = tuple(torch.from_numpy(p).cuda().float() for p in LD.planes(ct))
    for _ in range(3):                                                     # warm-up (code object load, clocks)
        launch()
    torch_band(planes, W, thr, torch_rows)
    torch.cuda.synchronize()
    kernel_ms, kernel_min, torch_ms = [], [], []
    for _ in range(2):                                                     # the two ways interleaved, twice
        times = []
        for _ in range(launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        kernel_ms.append(float(np.median(times)))
        kernel_min.append(float(min(times)))
        walls = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            torch_band(planes, W, thr, torch_rows)
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - t0)
        torch_ms.append(float(np.median(walls)) * 1e3)
    del planes
    over = d_over.cpu().numpy().view(np.uint32)

    reach = np.where(np.arange(min(K, sub + W)) < sub, W, 0)
    t0 = time.perf_counter()
    want = LD.band_host(ct[:sub + W], W, reach, thr)[0]
    host_s = time.perf_counter() - t0
    assert np.array_equal(over[:sub], want[:sub]), "device != definition"

    t0 = time.perf_counter()
    kept, _ = LD.greedy_host(over)
    greedy_s = time.perf_counter() - t0
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        s = LD.ld(ct, 2, np.arange(K), None, None, os.path.join(tmp, "b"), thr, W, silence=True)
        e2e = time.perf_counter() - t0
    assert s["n_kept"] == int(kept.sum())

    ms = min(kernel_ms)
    macs = quadrants(K, W) * 32 * 32 * ((N + LD.BLOCK - 1) // LD.BLOCK * LD.BLOCK) * 6
    tops = 2 * macs / (ms * 1e-3) / 1e12
    host_full = host_s * K / sub
    return {"sites": K, "samples": N, "window": W, "r2": thr, "tile_pairs": (K + LD.TILE - 1) // LD.TILE * ((LD.TILE - 1 + W) // LD.TILE + 1),
            "kernel_median_ms_twice": [round(v, 4) for v in kernel_ms], "kernel_min_ms_twice": [round(v, 4) for v in kernel_min],
            "int8_multiply_adds": macs, "kernel_tops": round(tops, 1), "fraction_of_sustained_i8": round(tops / I8_SUSTAINED_TOPS, 4),
            "useful_pair_samples_per_s": round(float(s["n_pairs_compared"]) * N / (ms * 1e-3), 1),
            "torch_fp32_matmul_ms_twice": [round(v, 2) for v in torch_ms], "torch_rows_per_block": torch_rows,
            "kernel_speedup_over_torch": round(min(torch_ms) / ms, 2),
            "host_rows": sub, "host_s_on_those": round(host_s, 3), "host_s_scaled_to_all_rows": round(host_full, 1),
            "command_end_to_end_s": round(e2e, 3), "host_greedy_s": round(greedy_s, 4), "n_kept": s["n_kept"],
            "n_pairs_over": s["n_pairs_over"], "device_matches_definition_on_those_rows": True}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=100_000)
    ap.add_argument("--samples", type=int, nargs="+", default=[1000, 4096])
    ap.add_argument("--windows", type=int, nargs="+", default=[100, 512])
    ap.add_argument("--missing", type=float, default=0.02)
    ap.add_argument("--r2", type=float, default=0.2)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--sub", type=int, default=512, help="the definition runs on this many rows")
    ap.add_argument("--torch_rows", type=int, default=1024, help="sites per block of the torch.matmul comparison")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "ld_bench.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    runs = []
    for N in a.samples:
        ct = synth(a.sites, N, a.missing, rng)
        for W in a.windows:
            runs.append(one(ct, W, a.r2, a.launches, a.sub, a.torch_rows))
            print(json.dumps(runs[-1]), flush=True)
    out = {"kernel": "loc_ld_band", "device": torch.cuda.get_device_name(0), "i8_sustained_tops": I8_SUSTAINED_TOPS, "runs": runs}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
