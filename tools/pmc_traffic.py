#!/usr/bin/env python3
"""Summarise rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes into per-launch HBM traffic.

Units and corrections per /opt/skills/guides/MI355X_MICROARCH.md (HBM section):
  FETCH_SIZE, WRITE_SIZE are in KiB (hbm_bytes = counter * 1024);
  on gfx950 FETCH_SIZE reports exactly 1/2 of the bytes of a wide (16 B/lane) coalesced streaming
  read -> doubled for kernels whose reads are such streams (flagged per kernel below);
  WRITE_SIZE is uncalibrated by the guide -> calibrated here on a known byte count in the same run:
  the ModelCheckpoint snapshot, a device-to-device copy of n_total floats (`snapshot_if_kernel` since round 4; a torch
  tensor copy, `__amd_rocclr_copyBuffer`, before).

usage: pmc_traffic.py <fetch_dir>/f_counter_collection.csv <write_dir>/w_counter_collection.csv out.json [K H n]
(tools/pmc_traffic.sh runs the two passes and this summary)
"""
import csv
import hashlib
import json
import os
import sys
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_sources_sha():
    """Same hash bench.py computes: `traffic` is only reported while the kernel sources still match the profile."""
    h = hashlib.sha256()
    for rel in ("locator_amd/csrc/l1_kernels.hip", "locator_amd/csrc/l1_chain.hip", "locator_amd/csrc/common.h"):
        h.update(open(os.path.join(ROOT, rel), "rb").read())
    return h.hexdigest()[:16]

WIDE_STREAM_READ = ("l1_bwd_adam_kernel", "l1_bwd_adam_chain_kernel", "l1_fwd_partial_kernel", "__amd_rocclr_copyBuffer",
                    "snapshot_if_kernel")


def per_kernel(path, counter):
    acc = defaultdict(list)
    for r in csv.DictReader(open(path)):
        if r["Counter_Name"] == counter:
            name = r["Kernel_Name"].split("(")[0].replace("void ", "")
            acc[name].append(float(r["Counter_Value"]))
    return acc


def main():
    fetch = per_kernel(sys.argv[1], "FETCH_SIZE")
    write = per_kernel(sys.argv[2], "WRITE_SIZE")
    out = {}
    for k in sorted(set(fetch) | set(write)):
        f = fetch.get(k, [0.0])
        w = write.get(k, [0.0])
        f_mean, w_mean = sum(f) / len(f), sum(w) / len(w)
        wide = any(k.startswith(p) for p in WIDE_STREAM_READ)
        rd = f_mean * 1024 * (2 if wide else 1)
        out[k] = {"launches": len(f), "FETCH_SIZE_KiB_mean": f_mean, "WRITE_SIZE_KiB_mean": w_mean,
                  "fetch_doubled_for_wide_stream": wide, "read_bytes": rd, "write_bytes": w_mean * 1024,
                  "traffic_bytes": rd + w_mean * 1024, "FETCH_max": max(f), "WRITE_max": max(w)}
    K, H, n = (int(v) for v in sys.argv[4:7]) if len(sys.argv) >= 7 else (100000, 256, 1000)
    n_total = None
    # round 4: the ModelCheckpoint snapshot is the predicated device copy snapshot_if_kernel (the epochs that improve val_loss
    # copy all n_total parameters: its largest launch); before, a torch tensor copy (__amd_rocclr_copyBuffer)
    cal_name = next((k for k in out if k.startswith("snapshot_if_kernel")), "__amd_rocclr_copyBuffer")
    cal = out.get(cal_name)
    doc = {"source": "rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE (separate passes) --kernel-trace -- python3 "
                     "bench.py --full --steps 2 --warmup 2 --no-cpu-baseline --no-l1-gemm --no-graph; tools/pmc_traffic.sh",
           "workload": {"K": K, "H": H, "n": n},
           "kernel_sources_sha256_16": kernel_sources_sha(),
           "units": "FETCH_SIZE/WRITE_SIZE in KiB; FETCH_SIZE doubled for wide (16 B/lane) streaming reads per "
                    "MI355X_MICROARCH.md (HBM section)",
           "calibration": None if cal is None else {
               "kernel": cal_name + ": its largest launch is the ModelCheckpoint snapshot, a device-to-device copy of all "
                                    "n_total parameters",
               "WRITE_SIZE_KiB_max": cal["WRITE_max"], "FETCH_SIZE_KiB_max": cal["FETCH_max"],
               "fetch_over_write": cal["FETCH_max"] / cal["WRITE_max"] if cal["WRITE_max"] else None,
               "note": "a copy reads what it writes: WRITE_SIZE equals the buffer size and FETCH_SIZE reports 1/2 of it "
                       "-> the x2 correction holds on this access pattern"},
           "kernels": out}
    json.dump(doc, open(sys.argv[3], "w"), indent=1)
    for k, v in out.items():
        if v["traffic_bytes"] > 1e6:
            print(f"{k[:44]:44s} n={v['launches']:5d} read={v['read_bytes']/1e6:9.2f} MB write={v['write_bytes']/1e6:9.2f} MB")


if __name__ == "__main__":
    main()
