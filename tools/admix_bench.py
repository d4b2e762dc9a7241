#!/usr/bin/env python3
"""Time loc_admix_step (csrc/admix_kernels.hip) on planted genotypes (--alpha, --fst and --missing as tests/admix_util.py plants
them, generated here from --seed) at --shapes N x K x C, default 1,000 x 100,000 x 8 (the project's scale) and 500 x 5,830 x 6
(the size of the golden VCF), from the start of a fit.  Every series of --launches event-timed launches is taken twice, both
medians are kept and the rates use the smaller.  Next to it the NumPy float64 step (admix.step_host) on the same inputs: on all
sites where N x K <= --host_pairs, else on the first --host_pairs / N sites, its time scaled by the share of sites and said so;
F' of those sites and (on all sites) Q' and ll are held to the tolerance of the tests.  Writes one JSON object (and prints it):
the medians, the bytes of counts a step reads (twice N x pitch: one pass per reduction), the useful operations
N K (8 C + 30) it is credited with (both passes form h and hb: 4 C each, uncontracted multiplies and adds) and their rate."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from locator_amd import _lib  # noqa: E402
from locator_amd import admix as A  # noqa: E402
from locator_amd import baselines as BL  # noqa: E402


def planted(N, K, C, rng, alpha, fst, missing):
    Q = rng.dirichlet(np.full(C, alpha), N)
    p = rng.uniform(0.05, 0.95, K)
    s = (1.0 - fst) / fst
    F = rng.beta((p * s)[:, None], ((1.0 - p) * s)[:, None], (K, C))
    c = np.empty((N, K), dtype=np.int8)
    for i0 in range(0, N, 128):                                             # by rows: the probabilities are N x K doubles
        c[i0:i0 + 128] = rng.binomial(2, np.clip(Q[i0:i0 + 128] @ F.T, 0.0, 1.0))
        c[i0:i0 + 128][rng.random(c[i0:i0 + 128].shape) < missing] = -1
    return c


def errors(got, want, N, K):
    tol = (max(N, K) + 32) * 2.0 ** -23
    return float((np.abs(got.astype(np.float64) - want) / want).max() / tol)


def one(N, K, C, a, rng):
    print(f"{N} x {K} x {C}: generating", file=sys.stderr, flush=True)
    c = planted(N, K, C, rng, a.alpha, a.fst, a.missing)
    Q, F = A.project(*A.start(N, K, C, a.seed))
    lib = _lib.load()
    buf = BL.padded(c)
    d_c, d_q, d_f = torch.from_numpy(buf).cuda(), torch.from_numpy(Q).cuda(), torch.from_numpy(F).cuda()
    d_qo, d_fo = torch.empty_like(d_q), torch.empty_like(d_f)
    d_ll = torch.empty(1, dtype=torch.float64, device="cuda")
    work_bytes = int(lib.loc_admix_work_bytes(N, K, C, a.k_groups))
    work = torch.empty(max(work_bytes // 4, 4), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def step():
        _lib.check(lib.loc_admix_step(d_c.data_ptr(), N, K, buf.shape[1], 2, C, d_q.data_ptr(), d_f.data_ptr(), d_qo.data_ptr(),
                                      d_fo.data_ptr(), d_ll.data_ptr(), a.k_groups, work.data_ptr(), work_bytes, stream), "loc_admix_step")

    print(f"{N} x {K} x {C}: timing", file=sys.stderr, flush=True)
    for _ in range(3):                                                      # warm-up (code object load, clocks)
        step()
    torch.cuda.synchronize()
    series = []
    for _ in range(2):
        ms = []
        for _ in range(a.launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            step()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        series.append((float(np.median(ms)), float(min(ms))))
    Qd, Fd, lld = d_qo.cpu().numpy(), d_fo.cpu().numpy(), float(d_ll.item())

    Ks = K if N * K <= a.host_pairs else max(1, a.host_pairs // N)
    print(f"{N} x {K} x {C}: the definition on {Ks} sites", file=sys.stderr, flush=True)
    t0 = time.perf_counter()
    Qh, Fh, llh = A.step_host(c[:, :Ks], 2, Q, F[:Ks])
    host_ms = (time.perf_counter() - t0) * 1e3
    out = {"samples": N, "sites": K, "clusters": C, "missing": a.missing, "k_groups": a.k_groups, "work_bytes": work_bytes,
           "step_median_ms_both_series": [round(s[0], 4) for s in series], "step_min_ms": round(min(s[1] for s in series), 4)}
    ms = min(s[0] for s in series)
    ops = N * K * (8 * C + 30)
    out.update({"count_bytes_read": 2 * N * int(buf.shape[1]), "count_gb_per_s": round(2 * N * buf.shape[1] / (ms * 1e-3) / 1e9, 1),
                "operations_credited": ops, "tera_operations_per_s": round(ops / (ms * 1e-3) / 1e12, 2),
                "host_sites": Ks, "host_float64_step_ms_on_those": round(host_ms, 1),
                "host_float64_step_ms_scaled_to_all_sites": round(host_ms * K / Ks, 1),
                "host_over_device": round(host_ms * K / Ks / ms, 1),
                "F_error_over_tolerance_on_those": round(errors(Fd[:Ks], Fh, N, K), 5)})
    if Ks == K:
        out.update({"Q_error_over_tolerance": round(errors(Qd, Qh, N, K), 5),
                    "ll_error_over_bound": round(abs(lld - llh) / ((A.LL_RUN + 8) * 2.0 ** -23 * abs(llh)), 6)})
        assert out["Q_error_over_tolerance"] <= 1.0 and out["ll_error_over_bound"] <= 1.0
    assert out["F_error_over_tolerance_on_those"] <= 1.0, "device outside the fp32 tolerance of the definition"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["1000x100000x8", "500x5830x6"])
    ap.add_argument("--alpha", type=float, default=0.3)
    ap.add_argument("--fst", type=float, default=0.1)
    ap.add_argument("--missing", type=float, default=0.05)
    ap.add_argument("--launches", type=int, default=15)
    ap.add_argument("--host_pairs", type=int, default=10_000_000, help="the float64 step runs on at most this many (sample, site) pairs")
    ap.add_argument("--k_groups", type=int, default=0, help="0 = the launcher's choice")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "admix_bench.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    out = {"kernel": "loc_admix_step", "device": torch.cuda.get_device_name(0),
           "runs": [one(*(int(v) for v in shape.split("x")), a, rng) for shape in a.shapes]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
