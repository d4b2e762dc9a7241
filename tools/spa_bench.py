#!/usr/bin/env python3
"""Time loc_spa_grid (csrc/spa_kernels.hip) on synthetic allele counts and surfaces: --rows samples (default 1,000 and 4,096) x
--sites sites (100,000) x --nodes grid nodes (4,096 = 64 x 64), --missing of the calls missing (2 %), every site used, slopes
N(0, 0.5) and levels N(0, 1.5), nodes uniform in +- 2.  Everything is generated here from --seed.  Next to it, in the same run
and interleaved launch by launch, what one would write without a kernel: the t and softplus(t) surfaces [K][G] materialised
as fp32 on the device with torch elementwise kernels, then two torch.matmul, all parts timed.  Every series of --launches
event-timed launches is taken twice, both medians are kept, and the rates and ratios use the smaller of the two.  Writes one JSON object (and prints it) with one entry per row
count: the medians, the fused multiply-adds loc_spa_grid executes (tiles x 256 x 128 x padded sites x 2 products) per second
and that rate, two operations a multiply-add, as a fraction of the 157.3 TF fp32 matrix peak (MI355X: 256 compute units x 4
SIMDs x 64 FLOP per clock x 2.4 GHz), and the largest error of --sub rows x --sub_nodes nodes against the float64 definition
in units of the derived element bound (spa.ll_bound), for loc_spa_grid and for the alternative."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from locator_amd import _lib  # noqa: E402
from locator_amd import baselines as BL  # noqa: E402
from locator_amd import spa as S  # noqa: E402

FP32_MATRIX_PEAK_TF = 157.3


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def one(Q, K, G, missing, launches, sub, sub_nodes, k_groups, rng):
    print(f"{Q} rows x {K} sites x {G} nodes: generating", file=sys.stderr, flush=True)
    freq = rng.uniform(0.05, 0.5, (1, K))
    c = rng.binomial(2, np.broadcast_to(freq, (Q, K))).astype(np.int8)
    c[rng.random((Q, K)) < missing] = -1
    theta = (rng.normal(size=(K, 4)) * np.array([[0.5, 0.5, 1.5, 0.0]])).astype(np.float32)
    used = np.ones(K, dtype=np.uint8)
    gx, gy = rng.uniform(-2, 2, G).astype(np.float32), rng.uniform(-2, 2, G).astype(np.float32)
    lib = _lib.load()
    buf = BL.padded(c)
    d_c = torch.from_numpy(buf).cuda()
    d_theta, d_used = torch.from_numpy(theta).cuda(), torch.from_numpy(used).cuda()
    d_gx, d_gy = torch.from_numpy(gx).cuda(), torch.from_numpy(gy).cuda()
    d_ll = torch.empty((Q, G), dtype=torch.float64, device="cuda")
    work_bytes = int(lib.loc_spa_grid_work_bytes(Q, K, G, k_groups))
    work = torch.empty(max(work_bytes // 4, 4), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    tiles = ((Q + S.TILE_SAMPLES - 1) // S.TILE_SAMPLES) * ((G + S.TILE - 1) // S.TILE)
    groups = work_bytes // (tiles * S.TILE_SAMPLES * S.TILE * 4)
    nblocks = (K + S.BLOCK - 1) // S.BLOCK
    per_group = (nblocks + groups - 1) // groups * S.BLOCK

    def fused():
        _lib.check(lib.loc_spa_grid(d_c.data_ptr(), Q, K, buf.shape[1], 2, d_theta.data_ptr(), d_used.data_ptr(), d_gx.data_ptr(),
                                    d_gy.data_ptr(), G, k_groups, d_ll.data_ptr(), work.data_ptr(), work_bytes, stream), "loc_spa_grid")

    cc = d_c[:, :K]
    a_op = torch.clamp(cc, min=0).to(torch.float32)                        # the sample operands: made once, not timed
    m_op = (cc >= 0).to(torch.float32) * -2.0

    def surfaces():
        t = (d_theta[:, 0:1] * d_gx[None] + d_theta[:, 1:2] * d_gy[None]) + d_theta[:, 2:3]
        return t, torch.clamp(t, min=0) + torch.log1p(torch.exp(-torch.abs(t)))

    def products(t, sp):
        return torch.matmul(a_op, t) + torch.matmul(m_op, sp)

    print(f"{Q} rows x {K} sites x {G} nodes: timing", file=sys.stderr, flush=True)
    for _ in range(3):                                                     # warm-up (code object load, clocks, the BLAS choice)
        fused()
        t, sp = surfaces()
        alt = products(t, sp)
    torch.cuda.synchronize()
    series = []
    for _ in range(2):                                                     # every series twice
        t_fused, t_surf, t_mm = [], [], []
        for _ in range(launches):                                          # interleaved: every round times all three
            t_fused.append(timed(fused)[0])
            ms, (t, sp) = timed(surfaces)
            t_surf.append(ms)
            ms, alt = timed(lambda: products(t, sp))
            t_mm.append(ms)
        series.append((float(np.median(t_fused)), float(min(t_fused)), float(np.median(t_surf)), float(np.median(t_mm))))
    ll = d_ll.cpu().numpy()
    alt = alt.cpu().numpy().astype(np.float64)
    del t, sp

    print(f"{Q} rows x {K} sites: the definition on {sub} rows x {sub_nodes} nodes", file=sys.stderr, flush=True)
    rows = np.linspace(0, Q - 1, sub).astype(np.int64)
    nodes = np.linspace(0, G - 1, sub_nodes).astype(np.int64)
    want = S.grid_host(c[rows], 2, theta, used, gx[nodes], gy[nodes], chunk=8192)
    bound = S.ll_bound(c[rows], 2, theta, used, gx[nodes], gy[nodes], per_group, chunk=8192)
    ratio = float((np.abs(ll[np.ix_(rows, nodes)] - want) / bound).max())
    ratio_alt = float((np.abs(alt[np.ix_(rows, nodes)] - want) / bound).max())
    assert ratio <= 1.0, "device outside the fp32 bound of the definition"

    fmas = 2 * tiles * S.TILE_SAMPLES * S.TILE * nblocks * S.BLOCK
    ms = min(s[0] for s in series)
    tf = 2 * fmas / (ms * 1e-3) / 1e12
    surf, mm = min(s[2] for s in series), min(s[3] for s in series)
    return {"rows": Q, "sites": K, "nodes": G, "missing": missing, "tiles": tiles, "k_groups": k_groups, "groups_launched": groups,
            "sites_per_group": per_group, "work_bytes": work_bytes,
            "kernel_median_ms_both_series": [round(s[0], 4) for s in series], "kernel_min_ms": round(min(s[1] for s in series), 4),
            "fused_multiply_adds": fmas, "kernel_tera_fma_per_s": round(fmas / (ms * 1e-3) / 1e12, 2), "kernel_tflops": round(tf, 1),
            "fraction_of_fp32_matrix_peak": round(tf / FP32_MATRIX_PEAK_TF, 4),
            "alt_surfaces_median_ms_both_series": [round(s[2], 4) for s in series],
            "alt_two_matmul_median_ms_both_series": [round(s[3], 4) for s in series],
            "alt_total_median_ms": round(surf + mm, 4), "alt_over_fused": round((surf + mm) / ms, 3),
            "alt_matmul_tflops": round(4.0 * Q * K * G / (mm * 1e-3) / 1e12, 1), "alt_surface_bytes": 2 * 4 * K * G,
            "host_rows": len(rows), "host_nodes": len(nodes), "error_over_bound_on_those": round(ratio, 5),
            "alt_error_over_bound_on_those": round(ratio_alt, 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1000, 4096])
    ap.add_argument("--sites", type=int, default=100_000)
    ap.add_argument("--nodes", type=int, default=4096)
    ap.add_argument("--missing", type=float, default=0.02)
    ap.add_argument("--launches", type=int, default=9)
    ap.add_argument("--sub", type=int, default=4, help="the definition runs on this many rows ...")
    ap.add_argument("--sub_nodes", type=int, default=32, help="... and this many nodes")
    ap.add_argument("--k_groups", type=int, default=0, help="0 = the launcher's choice")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "spa_bench.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    out = {"kernel": "loc_spa_grid", "device": torch.cuda.get_device_name(0), "fp32_matrix_peak_tf": FP32_MATRIX_PEAK_TF,
           "runs": [one(Q, a.sites, a.nodes, a.missing, a.launches, a.sub, a.sub_nodes, a.k_groups, rng) for Q in a.rows]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
