#!/usr/bin/env python3
"""Time loc_phase_viterbi (csrc/phase_kernels.hip) on planted haplotypes (mosaics of founder haplotypes, generated here from
--seed, the order of every call shuffled) at --shapes samples x sites, default 150 x 600, 500 x 5,830 (the golden VCF) and
1,000 x 100,000 (the project's scale), --states donor slots a sample (the columns of states / 2 other samples, drawn): every
sample a recipient, one launch, event-timed, --launches times (the median and the smallest).  Next to it, on the first shape only:
  phase.viterbi_host in float32 on --host_recipients recipients, its time scaled to all recipients and to the other shapes by
  recipients x sites x states^2 and LABELLED as extrapolated;
  the device result held to that answer bit for bit.
With --ablate, the timing-ablation builds of the kernel (`make -C locator_amd/csrc variant F=phase_kernels XDEF=-DPH_ABLATE=<bits>
TAG=ph<bits>` for bits 1, 2, 4: no traceback, the forward pass alone, no logarithm) are timed on every shape; their results are
wrong by construction.  Writes one JSON object (and prints it)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from locator_amd import _abi, _lib  # noqa: E402
from locator_amd import baselines as BL  # noqa: E402
from locator_amd import phase as PH  # noqa: E402

ABLATIONS = {1: "no traceback", 2: "the forward pass alone", 4: "no logarithm"}


def planted(N, K, rng, founders=8, stay=0.98, flips=0.01, missing=0.03, cols=64):
    found = rng.integers(0, 2, (founders, K)).astype(np.int8)
    hap = np.empty((K, 2 * N), dtype=np.int8)
    sites = np.arange(K)
    for c0 in range(0, 2 * N, cols):
        n = min(cols, 2 * N - c0)
        new = rng.random((K, n)) >= stay
        new[0] = True
        start = np.maximum.accumulate(np.where(new, sites[:, None], 0), axis=0)
        pick = rng.integers(0, founders, (K, n))
        part = found[pick[start, np.arange(n)[None, :]], sites[:, None]]
        part ^= (rng.random(part.shape) < flips).astype(np.int8)
        part[rng.random(part.shape) < missing] = -1
        hap[:, c0:c0 + n] = part
    swap = rng.random((K, N)) < 0.5
    a0, a1 = hap[:, 0::2].copy(), hap[:, 1::2].copy()
    hap[:, 0::2], hap[:, 1::2] = np.where(swap, a1, a0), np.where(swap, a0, a1)
    return hap


def bind(path):
    lib = C.CDLL(path)
    for name, (res, args) in _abi.LATER["phase"].prototypes.items():
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    return lib


def one(N, K, a, rng, libs, first):
    print(f"{N} x {K}: generating", file=sys.stderr, flush=True)
    hap = planted(N, K, rng)
    S, H = a.states, 2 * N
    rec = np.arange(N, dtype=np.int32)
    others = (rec[:, None] + 1 + np.stack([rng.permutation(N - 1)[:S // 2] for _ in range(N)])) % N
    don = np.stack([2 * others, 2 * others + 1], axis=2).reshape(N, S).astype(np.int32)
    rho = np.full(K, 1 - np.exp(-a.switch), dtype=np.float32)
    rho[0] = 1
    theta = PH.PT.default_theta(S)
    buf = BL.padded(hap)
    put = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
    d_h, d_rec, d_don, d_rho = put(buf), put(rec), put(don), put(rho)
    d_first = torch.empty((N, K), dtype=torch.int8, device="cuda")
    d_ll = torch.empty(N, dtype=torch.float64, device="cuda")
    d_ns, d_nt, d_nd = (torch.empty(N, dtype=torch.int32, device="cuda") for _ in range(3))
    lib = libs[0]
    work_bytes = int(lib.loc_phase_work_bytes(S, K, N, a.block))
    work = torch.empty(max(work_bytes // 4, 4), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def timed(which, launches):
        ms = []
        for _ in range(launches + 1):                                       # the first is the warm-up
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = which.loc_phase_viterbi(d_h.data_ptr(), H, K, buf.shape[1], d_rec.data_ptr(), N, d_don.data_ptr(), S, d_rho.data_ptr(),
                                         theta, a.block, d_first.data_ptr(), K, d_ll.data_ptr(), d_ns.data_ptr(), d_nt.data_ptr(),
                                         d_nd.data_ptr(), work.data_ptr(), work_bytes, stream)
            assert rc == 0, rc
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms[1:])), float(min(ms[1:]))

    print(f"{N} x {K}: timing", file=sys.stderr, flush=True)
    med, low = timed(lib, a.launches)
    got_first, got_ns = d_first.cpu().numpy(), d_ns.cpu().numpy()
    cells = N * K * S * S
    out = {"samples": N, "sites": K, "states": S, "recipients": N, "block": a.block, "work_bytes": work_bytes,
           "work_bytes_a_recipient": work_bytes // N, "viterbi_median_ms": round(med, 3), "viterbi_min_ms": round(low, 3),
           "us_per_site_and_wave": round(med * 1e3 / K / max(1.0, N / (4.0 * torch.cuda.get_device_properties(0).multi_processor_count)), 3),
           "recipient_site_state_cells": cells, "giga_cells_per_s": round(cells / (med * 1e-3) / 1e9, 2),
           "switches_per_site": round(float(got_ns.sum()) / (N * K), 5)}
    for bits, lab in sorted(libs.items()):
        if bits:
            m, _ = timed(lab, max(1, a.launches // 2))
            out[f"ablation_{bits}_median_ms ({ABLATIONS[bits]}; results wrong)"] = round(m, 3)
    if first:
        sub = rec[:: max(1, N // min(a.host_recipients, N))][:a.host_recipients]
        print(f"{N} x {K}: the definition on {len(sub)} recipients", file=sys.stderr, flush=True)
        t0 = time.perf_counter()
        want = PH.viterbi_host(hap, sub, don[sub], rho, theta)
        host_s = time.perf_counter() - t0
        assert np.array_equal(got_first[sub], want[0]) and np.array_equal(got_ns[sub], want[2]), "device differs from the definition"
        out.update({"device_equals_the_definition_on": int(len(sub)), "host_float32_s_on_those": round(host_s, 2),
                    "host_float32_s_all_recipients_EXTRAPOLATED": round(host_s * N / len(sub), 1),
                    "host_ns_per_cell": round(host_s * 1e9 / (len(sub) * K * S * S), 2)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["150x600", "500x5830", "1000x100000"])
    ap.add_argument("--states", type=int, default=64)
    ap.add_argument("--switch", type=float, default=0.01)
    ap.add_argument("--block", type=int, default=0)
    ap.add_argument("--launches", type=int, default=4)
    ap.add_argument("--host_recipients", type=int, default=8)
    ap.add_argument("--ablate", action="store_true", help="also time build/liblocator_hip_ph{1,2,4}.so")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "phase_bench.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    libs = {0: _lib.load()}
    if a.ablate:
        for bits in ABLATIONS:
            libs[bits] = bind(os.path.join(ROOT, "build", f"liblocator_hip_ph{bits}.so"))
    runs = []
    for n, shape in enumerate(a.shapes):
        N, K = (int(v) for v in shape.split("x"))
        runs.append(one(N, K, a, rng, libs, n == 0))
    per_cell = runs[0]["host_ns_per_cell"]
    for r in runs[1:]:
        r["host_float32_s_EXTRAPOLATED from the first shape by cells"] = round(per_cell * 1e-9 * r["recipient_site_state_cells"], 0)
    out = {"kernel": "loc_phase_viterbi", "device": torch.cuda.get_device_name(0), "switch": a.switch, "runs": runs}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
