#!/usr/bin/env python3
"""Time loc_grm_pairs (csrc/grm_kernels.hip) on synthetic allele counts: --rows samples (default 1,000 and 4,096) x --sites
sites (100,000), --missing of the calls missing (2 %), a site's allele frequency uniform in 0.05 .. 0.5; the site constants
are pca.site_constants of those counts.  Everything is generated here from --seed.  Next to it, in the same run and
interleaved launch by launch, the obvious alternative: materialise Z as fp32 on the device (torch elementwise kernels) and
call torch.matmul(Z, Z.T), both parts timed.  Writes one JSON object (and prints it) with one entry per row count: the medians
of --launches event-timed launches of each, the fused multiply-adds loc_grm_pairs executes (tile pairs x 128 x 128 x padded
sites) per second and that rate, two operations a multiply-add, as a fraction of the 157.3 TF fp32 matrix peak
(MI355X: 256 compute units x 4 SIMDs x 64 FLOP per clock x 2.4 GHz), the device path end to end with its transfers
(pca.grm_device, median of 3), and the largest error of --sub device rows against the float64 definition in units of the
derived element bound (K + 8) 2^-24 sum |z_ik| |z_jk|, for loc_grm_pairs and for the alternative."""
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
from locator_amd import pca as P  # noqa: E402

FP32_MATRIX_PEAK_TF = 157.3


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def one(N, K, missing, launches, sub, k_groups, rng):
    print(f"{N} rows x {K} sites: generating", file=sys.stderr, flush=True)
    freq = rng.uniform(0.05, 0.5, (1, K))
    c = rng.binomial(2, np.broadcast_to(freq, (N, K))).astype(np.int8)
    c[rng.random((N, K)) < missing] = -1
    mean, scale, K_used = P.site_constants(c, 2)
    lib = _lib.load()
    buf = BL.padded(c)
    d_c = torch.from_numpy(buf).cuda()
    d_mean, d_scale = torch.from_numpy(mean).cuda(), torch.from_numpy(scale).cuda()
    d_g = torch.empty((N, N), dtype=torch.float64, device="cuda")
    work_bytes = int(lib.loc_grm_work_bytes(N, K, k_groups))
    work = torch.empty(max(work_bytes // 4, 4), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def fused():
        _lib.check(lib.loc_grm_pairs(d_c.data_ptr(), N, K, buf.shape[1], d_mean.data_ptr(), d_scale.data_ptr(), k_groups,
                                     d_g.data_ptr(), work.data_ptr(), work_bytes, stream), "loc_grm_pairs")

    def materialise():
        cc = d_c[:, :K]
        return torch.where(cc < 0, torch.zeros((), device="cuda"), (cc.to(torch.float32) - d_mean[None]) * d_scale[None])

    print(f"{N} rows x {K} sites: timing", file=sys.stderr, flush=True)
    for _ in range(3):                                                     # warm-up (code object load, clocks, the BLAS choice)
        fused()
        z = materialise()
        g_alt = torch.matmul(z, z.T)
    torch.cuda.synchronize()
    t_fused, t_mat, t_mm = [], [], []
    for _ in range(launches):                                              # interleaved: every round times all three
        t_fused.append(timed(fused)[0])
        ms, z = timed(materialise)
        t_mat.append(ms)
        ms, g_alt = timed(lambda: torch.matmul(z, z.T))
        t_mm.append(ms)
    ms = float(np.median(t_fused))
    g = d_g.cpu().numpy()
    g_alt = g_alt.cpu().numpy().astype(np.float64)
    del z

    walls = []
    for _ in range(3):                                                     # upload, launch, download
        t0 = time.perf_counter()
        got = P.grm_device(c, mean, scale, k_groups=k_groups)
        walls.append(time.perf_counter() - t0)
    assert np.array_equal(got, g) and np.array_equal(g, g.T)

    print(f"{N} rows x {K} sites: the definition on {sub} rows", file=sys.stderr, flush=True)
    rows = np.linspace(0, N - 1, sub).astype(np.int64)
    t0 = time.perf_counter()
    want, bound = np.zeros((len(rows), N)), np.zeros((len(rows), N))
    for k0 in range(0, K, 8192):                                           # the float64 z of all rows, a chunk of sites at a time
        zz = P.z_host(c[:, k0:k0 + 8192], mean[k0:k0 + 8192], scale[k0:k0 + 8192])
        want += zz[rows] @ zz.T
        bound += np.abs(zz[rows]) @ np.abs(zz).T
    bound *= (K + 8) * 2.0 ** -24
    host_s = time.perf_counter() - t0
    ratio = float((np.abs(g[rows] - want) / bound).max())
    ratio_alt = float((np.abs(g_alt[rows] - want) / bound).max())
    assert ratio <= 1.0, "device outside the fp32 bound of the definition"

    tiles = (N + P.TILE - 1) // P.TILE
    pairs = tiles * (tiles + 1) // 2
    fmas = pairs * P.TILE * P.TILE * ((K + P.BLOCK - 1) // P.BLOCK * P.BLOCK)
    tf = 2 * fmas / (ms * 1e-3) / 1e12
    mat, mm = float(np.median(t_mat)), float(np.median(t_mm))
    e2e = float(np.median(walls))
    return {"rows": N, "sites": K, "sites_used": K_used, "missing": missing, "tile_pairs": pairs, "k_groups": k_groups,
            "work_bytes": work_bytes, "kernel_median_ms": round(ms, 4), "kernel_min_ms": round(float(min(t_fused)), 4),
            "fused_multiply_adds": fmas, "kernel_tera_fma_per_s": round(fmas / (ms * 1e-3) / 1e12, 2), "kernel_tflops": round(tf, 1),
            "fraction_of_fp32_matrix_peak": round(tf / FP32_MATRIX_PEAK_TF, 4),
            "alt_materialise_z_median_ms": round(mat, 4), "alt_matmul_median_ms": round(mm, 4),
            "alt_total_median_ms": round(mat + mm, 4), "alt_over_fused": round((mat + mm) / ms, 3),
            "alt_matmul_tflops_full_square": round(2.0 * N * N * K / (mm * 1e-3) / 1e12, 1),
            "device_end_to_end_ms": round(e2e * 1e3, 2), "host_rows": len(rows), "host_s_on_those": round(host_s, 3),
            "error_over_bound_on_those_rows": round(ratio, 5), "alt_error_over_bound_on_those_rows": round(ratio_alt, 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1000, 4096])
    ap.add_argument("--sites", type=int, default=100_000)
    ap.add_argument("--missing", type=float, default=0.02)
    ap.add_argument("--launches", type=int, default=15)
    ap.add_argument("--sub", type=int, default=4, help="the definition runs on this many rows against all rows")
    ap.add_argument("--k_groups", type=int, default=0, help="0 = the launcher's choice")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "pca_bench.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    out = {"kernel": "loc_grm_pairs", "device": torch.cuda.get_device_name(0), "fp32_matrix_peak_tf": FP32_MATRIX_PEAK_TF,
           "runs": [one(N, a.sites, a.missing, a.launches, a.sub, a.k_groups, rng) for N in a.rows]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
