#!/usr/bin/env python3
"""Time the hot path of `python -m locator_amd.explain` - loc_explain_sites + loc_explain_reduce - at K = 100,000 sites and
width 256, n = 1,000 and 10,000 samples, and the same contraction + epilogue on the host (torch CPU, fp32) for comparison.

  rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/explain_bench.py --json OUT/explain_bench.json

The device time per configuration is the median of --reps launches measured with stream events; rocprofv3's kernel stats
give the per-kernel split.  TF/s counts 2 * (2n) * K * Hp FLOP (the contraction; the epilogue is not counted) against the
155 TF fp32 matrix peak.  The host time is measured on --cpu_sites sites and scaled linearly to K (the full (2n x K) result
would not fit a host's memory at n = 10,000).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from locator_amd import _lib  # noqa: E402
from locator_amd.net import _compute_units, _ptr, _stream  # noqa: E402

PEAK_TF = 155.0


def device_case(n, K, Hp, reps):
    lib = _lib.load()
    g = torch.Generator(device="cuda").manual_seed(n + K)
    delta1 = torch.randn((2 * n, Hp), generator=g, device="cuda") * 1e-2
    U = torch.randn((K, Hp), generator=g, device="cuda") * 1e-2
    Xs = torch.randint(0, 3, (n, (K + 31) // 32 * 32), dtype=torch.uint8, device="cuda", generator=g)
    mm = torch.rand(K, generator=g, device="cuda")
    splits = lib.loc_explain_splits(n, K, _compute_units(torch.device("cuda")))
    partial = torch.empty(splits * 4 * K, dtype=torch.float64, device="cuda")
    out = torch.empty((4, K), dtype=torch.float64, device="cuda")

    def run():
        _lib.check(lib.loc_explain_sites(_ptr(delta1), n, _ptr(U), K, Hp, _ptr(Xs), Xs.stride(0), _ptr(mm), splits,
                                         _ptr(partial), _stream()), "loc_explain_sites")
        _lib.check(lib.loc_explain_reduce(_ptr(partial), splits, K, n, _ptr(out), _stream()), "loc_explain_reduce")

    run()
    torch.cuda.synchronize()
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    _lib.check(lib.loc_event_create(C.byref(ev0)))
    _lib.check(lib.loc_event_create(C.byref(ev1)))
    times = []
    for _ in range(reps):
        lib.loc_event_record(ev0, _stream())
        run()
        lib.loc_event_record(ev1, _stream())
        ms = C.c_float()
        _lib.check(lib.loc_event_elapsed_ms(ev0, ev1, C.byref(ms)))
        times.append(ms.value)
    lib.loc_event_destroy(ev0)
    lib.loc_event_destroy(ev1)
    ms = float(np.median(times))
    return {"n": n, "K": K, "Hp": Hp, "splits": splits, "device_ms_median": ms, "device_ms_min": float(min(times)),
            "tflops": 2.0 * 2 * n * K * Hp / (ms * 1e-3) / 1e12,
            "fraction_of_peak": 2.0 * 2 * n * K * Hp / (ms * 1e-3) / 1e12 / PEAK_TF}


def host_case(n, K, Hp, cpu_sites):
    rng = np.random.default_rng(0)
    d1 = torch.from_numpy(rng.normal(0, 1e-2, (n, 2, Hp)).astype(np.float32))
    U = torch.from_numpy(rng.normal(0, 1e-2, (cpu_sites, Hp)).astype(np.float32))
    x = torch.from_numpy(rng.integers(0, 3, (n, cpu_sites)).astype(np.float32))
    mm = torch.from_numpy(rng.random(cpu_sites).astype(np.float32))
    t0 = time.perf_counter()
    J = torch.einsum("njh,kh->njk", d1, U)
    A = J * (x - mm)[:, None, :]
    _ = torch.stack([A[:, 0].abs().mean(0), A[:, 1].abs().mean(0), torch.sqrt(A[:, 0] ** 2 + A[:, 1] ** 2).mean(0),
                     torch.sqrt((J ** 2).sum(1).mean(0))])
    dt = time.perf_counter() - t0
    return {"host_sites_measured": cpu_sites, "host_threads": torch.get_num_threads(),
            "host_ms_measured": dt * 1e3, "host_ms_scaled_to_K": dt * 1e3 * K / cpu_sites}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default="1000,10000")
    ap.add_argument("--K", default=100000, type=int)
    ap.add_argument("--Hp", default=256, type=int)
    ap.add_argument("--reps", default=20, type=int)
    ap.add_argument("--cpu_sites", default=2000, type=int)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    rows = []
    for n in (int(v) for v in a.ns.split(",")):
        r = device_case(n, a.K, a.Hp, a.reps)
        r.update(host_case(n, a.K, a.Hp, a.cpu_sites))
        print(json.dumps(r), flush=True)
        rows.append(r)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "peak_tf": PEAK_TF, "cases": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
