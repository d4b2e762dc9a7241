#!/usr/bin/env python3
"""Time loc_query_rows (csrc/query_kernels.hip) on a synthetic query: --samples x --sites diploid calls (random, 1 % missing)
generated on the device, every model column mapped to a distinct variant in shuffled order, every sample an output row in
shuffled order.  Prints one JSON line: the median of --reps event-timed launches, and the bytes the kernel must move (calls
read once, the rows written once) over that time.  For kernel time from the trace, run it under
`rocprofv3 --kernel-trace --stats -d <dir> -o run -- python tools/query_rows_bench.py`.
--dosage times loc_query_rows_dosage instead: --samples x --sites float32 dosages (uniform over [0, 2], 1 % NaN), half of the
columns flipped; 4 bytes read and 1 written per element."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from locator_amd import _lib  # noqa: E402
from locator_amd import query as Q  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10_000)
    ap.add_argument("--sites", type=int, default=100_000)
    ap.add_argument("--ploidy", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--dosage", action="store_true", help="time loc_query_rows_dosage on float32 dosages")
    a = ap.parse_args()
    if a.dosage:
        return dosage(a)
    N, V, P = a.samples, a.sites, a.ploidy
    g = torch.Generator(device="cuda").manual_seed(1)
    calls = torch.randint(0, 2, (V, N, P), dtype=torch.int8, device="cuda", generator=g)
    calls[torch.rand((V, N, P), device="cuda", generator=g) < 0.01] = -1
    rng = np.random.default_rng(2)
    cv = rng.permutation(V).astype(np.int32)
    ca = np.ones(V, np.int8)
    order = rng.permutation(N).astype(np.int32)
    for _ in range(3):                                                     # warm-up (code object load)
        X = Q.query_rows(calls, cv, ca, order, V)
    torch.cuda.synchronize()
    # check one launch against the restatement on a slice of rows / columns
    cols = rng.choice(V, 256, replace=False)
    rows = rng.choice(N, 64, replace=False)
    host = calls[torch.as_tensor(cv[cols].astype(np.int64), device="cuda")].cpu().numpy()      # (256, N, P)
    want = (host[:, order[rows], :] == 1).sum(axis=2).T.astype(np.uint8)
    assert np.array_equal(X[torch.as_tensor(rows, device="cuda")][:, torch.as_tensor(cols, device="cuda")].cpu().numpy(), want)
    lib = _lib.load()
    from locator_amd.net import _ptr, _stream
    d_cv = torch.as_tensor(cv).cuda()
    d_ca = torch.as_tensor(ca).cuda()
    d_so = torch.as_tensor(order).cuda()
    times = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(lib.loc_query_rows(_ptr(calls), V, N, P, _ptr(d_cv), _ptr(d_ca), V, _ptr(d_so), N, _ptr(X), X.stride(0),
                                      _stream()), "loc_query_rows")
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    ms = float(np.median(times))
    nbytes = V * N * P + N * V                                              # calls read + rows written
    print(json.dumps({"kernel": "loc_query_rows", "samples": N, "sites": V, "ploidy": P, "median_ms": round(ms, 4),
                      "min_ms": round(float(min(times)), 4), "bytes": nbytes, "TB_per_s": round(nbytes / ms / 1e9, 3),
                      "of_6.29_TBps_copy": round(nbytes / ms / 1e9 / 6.29, 3)}))


def dosage(a):
    N, V = a.samples, a.sites
    g = torch.Generator(device="cuda").manual_seed(1)
    ds = torch.empty((V, N), dtype=torch.float32, device="cuda").uniform_(0, 2, generator=g)
    for v0 in range(0, V, 8192):                                           # 1 % missing, a slab at a time
        blk = ds[v0:v0 + 8192]
        blk[torch.rand(blk.shape, device="cuda", generator=g) < 0.01] = float("nan")
    rng = np.random.default_rng(2)
    cv = rng.permutation(V).astype(np.int32)
    ca = rng.integers(0, 2, V).astype(np.int8)
    order = rng.permutation(N).astype(np.int32)
    for _ in range(3):                                                     # warm-up (code object load)
        X = Q.query_rows_dosage(ds, cv, ca, order, V)
    torch.cuda.synchronize()
    # check one launch against the host's fixed-point form on a slice of rows / columns
    from locator_amd import genotypes as G
    cols = rng.choice(V, 256, replace=False)
    rows = rng.choice(N, 64, replace=False)
    host = ds[torch.as_tensor(cv[cols].astype(np.int64), device="cuda")].cpu().numpy()[:, order[rows]]      # (256, 64)
    q = G.dosage_q(host).astype(np.int32)
    want = np.where(q == G.Q_MISSING, 0, np.where(ca[cols][:, None] == 0, 2 * G.DOSAGE_UNIT - q, q)).T.astype(np.uint8)
    assert np.array_equal(X[torch.as_tensor(rows, device="cuda")][:, torch.as_tensor(cols, device="cuda")].cpu().numpy(), want)
    lib = _lib.load()
    from locator_amd.net import _ptr, _stream
    d_cv = torch.as_tensor(cv).cuda()
    d_ca = torch.as_tensor(ca).cuda()
    d_so = torch.as_tensor(order).cuda()
    times = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(lib.loc_query_rows_dosage(_ptr(ds), V, N, _ptr(d_cv), _ptr(d_ca), V, _ptr(d_so), N, _ptr(X), X.stride(0),
                                             _stream()), "loc_query_rows_dosage")
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    ms = float(np.median(times))
    nbytes = 4 * V * N + N * V                                              # dosages read + rows written
    print(json.dumps({"kernel": "loc_query_rows_dosage", "samples": N, "sites": V, "median_ms": round(ms, 4),
                      "min_ms": round(float(min(times)), 4), "bytes": nbytes, "TB_per_s": round(nbytes / ms / 1e9, 3),
                      "of_6.29_TBps_copy": round(nbytes / ms / 1e9 / 6.29, 3)}))


if __name__ == "__main__":
    main()
