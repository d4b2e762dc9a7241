#!/usr/bin/env python3
"""Time loc_impute_dose (csrc/impute_kernels.hip) next to loc_paint_copy (csrc/paint_kernels.hip) on the inputs of
tools/paint_bench.py: planted haplotypes at --shapes samples x sites, default 150 x 600, 500 x 5,830 and 1,000 x 100,000, every
haplotype a donor and a recipient, one launch each.  The two entry points are timed in the same run, interleaved (one launch of
each, --launches times after --warmup launches of each), event-timed; the medians, the smallest times and the ratio of the
medians are reported with the dose bytes written.  On the first shape the device's doses of --host_recipients recipients are held
to the allowance of the tests against impute.dose_host(float64), and ll and n_donors to loc_paint_copy's bits.
With --ablate, the timing-ablation builds of the kernel (`make -C locator_amd/csrc variant F=impute_kernels XDEF=-DPK_ABLATE=<bits>
TAG=ik<bits>` for bits 1, 4, 8, 16, 24: no cross-lane sums, no scratch rows, no dose stored, no compare and select of a column's
allele, the last two) are timed on every shape: what a build saves is what that part costs while the others run (their results
are wrong by construction).  Writes one JSON object (and prints it)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from locator_amd import _abi, _lib  # noqa: E402
from locator_amd import baselines as BL  # noqa: E402
from locator_amd import impute as IM  # noqa: E402
from locator_amd import paint as PT  # noqa: E402
from tools.paint_bench import planted  # noqa: E402

ABLATIONS = {1: "no cross-lane sums", 4: "no scratch rows", 8: "no dose stored", 16: "no allele compare and select", 24: "both"}


def bind(path):
    lib = C.CDLL(path)
    for name, (res, args) in _abi.EXTENSIONS["impute"].prototypes.items():
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    return lib


def one(N, K, a, rng, libs, first):
    print(f"{N} x {K}: generating", file=sys.stderr, flush=True)
    hap = planted(N, K, rng)
    H = 2 * N
    donor, owner = np.ones(H, dtype=np.uint8), np.repeat(np.arange(N, dtype=np.int32), 2)
    rec = np.arange(H, dtype=np.int32)
    rho = np.full(K, 1 - np.exp(-a.switch), dtype=np.float32)
    rho[0] = 1
    theta = PT.default_theta(H)
    buf = BL.padded(hap)
    put = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
    d_h, d_donor, d_owner, d_rec, d_rho = put(buf), put(donor), put(owner), put(rec), put(rho)
    d_share, d_chunks = (torch.empty((H, H), dtype=torch.float32, device="cuda") for _ in range(2))
    d_dose = torch.empty((H, K), dtype=torch.float32, device="cuda")
    d_ll, d_nd = (torch.empty((2, H), dtype=dt, device="cuda") for dt in (torch.float64, torch.int32))
    lib = libs[0]
    work_bytes = int(lib.loc_paint_work_bytes(H, K, H, a.block))
    work = torch.empty(max(work_bytes // 4, 4), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    head = (d_h.data_ptr(), H, K, buf.shape[1], d_donor.data_ptr(), d_owner.data_ptr(), d_rec.data_ptr(), H, d_rho.data_ptr(), theta, a.block)
    tail = (work.data_ptr(), work_bytes, stream)
    calls = {"dose": lambda which: which.loc_impute_dose(*head, d_dose.data_ptr(), d_ll[0].data_ptr(), d_nd[0].data_ptr(), *tail),
             "copy": lambda which: lib.loc_paint_copy(*head, d_share.data_ptr(), d_chunks.data_ptr(), d_ll[1].data_ptr(),
                                                      d_nd[1].data_ptr(), *tail)}

    def launch(name, which):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = calls[name](which)
        e1.record()
        torch.cuda.synchronize()
        assert rc == 0, (name, rc)
        return e0.elapsed_time(e1)

    def interleaved(which, launches):
        ms = {"dose": [], "copy": []}
        for n in range(a.warmup + launches):
            for name in ("dose", "copy") if n % 2 == 0 else ("copy", "dose"):
                v = launch(name, which)
                if n >= a.warmup:
                    ms[name].append(v)
        return ms

    print(f"{N} x {K}: timing", file=sys.stderr, flush=True)
    ms = interleaved(lib, a.launches)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    got = (d_dose.cpu().numpy(), d_ll.cpu().numpy(), d_nd.cpu().numpy())
    assert np.array_equal(got[1][0].view(np.uint64), got[1][1].view(np.uint64)) and np.array_equal(got[2][0], got[2][1]), "ll / n_donors differ"
    cells = H * K * H
    out = {"samples": N, "sites": K, "columns": H, "recipients": H, "block": a.block, "work_bytes": work_bytes,
           "launches_each": a.launches, "warmup_each": a.warmup,
           "dose_median_ms": round(med["dose"], 3), "dose_min_ms": round(min(ms["dose"]), 3),
           "copy_median_ms": round(med["copy"], 3), "copy_min_ms": round(min(ms["copy"]), 3),
           "dose_over_copy": round(med["dose"] / med["copy"], 4), "dose_bytes_written": 4 * H * K,
           "recipient_site_column_cells": cells, "giga_cells_per_s": round(cells / (med["dose"] * 1e-3) / 1e9, 2),
           "ll_and_n_donors_equal_loc_paint_copy": True, "doses_nan": int(np.isnan(got[0]).sum())}
    for bits, lab in sorted(libs.items()):
        if bits:
            m = interleaved(lab, max(3, a.launches // 2))
            out[f"ablation_{bits}_dose_median_ms ({ABLATIONS[bits]}; results wrong)"] = round(float(np.median(m["dose"])), 3)
            out[f"ablation_{bits}_copy_median_ms_beside_it (the product kernel)"] = round(float(np.median(m["copy"])), 3)
    if first:
        n = min(a.host_recipients, H)
        sub = rec[:: max(1, H // n)][:n]
        print(f"{N} x {K}: the definition on {len(sub)} recipients", file=sys.stderr, flush=True)
        want = IM.dose_host(hap, donor, owner, sub, rho, theta)[0]
        w32 = IM.dose_host(hap, donor, owner, sub, rho, theta, np.float32)[0]
        dist = lambda g: float(np.nanmax(np.abs(g.astype(np.float64) - want)))
        allow = max(8 * dist(w32), 2.0 ** -21)
        ratio = dist(got[0][sub]) / allow
        assert ratio <= 1.0 and np.array_equal(np.isnan(got[0][sub]), np.isnan(want)), ("device outside the allowance of the definition", ratio)
        out.update({"error_over_allowance": round(ratio, 4), "allowance": allow, "host_float64_recipients": int(len(sub))})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["150x600", "500x5830", "1000x100000"])
    ap.add_argument("--switch", type=float, default=0.01)
    ap.add_argument("--block", type=int, default=0)
    ap.add_argument("--launches", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host_recipients", type=int, default=16)
    ap.add_argument("--ablate", action="store_true", help="also time build/liblocator_hip_ik{1,4,8,16,24}.so")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "impute_bench.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    libs = {0: _lib.load()}
    if a.ablate:
        for bits in ABLATIONS:
            libs[bits] = bind(os.path.join(ROOT, "build", f"liblocator_hip_ik{bits}.so"))
    runs = []
    for n, shape in enumerate(a.shapes):
        N, K = (int(v) for v in shape.split("x"))
        runs.append(one(N, K, a, rng, libs, n == 0))
    out = {"kernel": "loc_impute_dose beside loc_paint_copy", "device": torch.cuda.get_device_name(0), "switch": a.switch, "runs": runs}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
