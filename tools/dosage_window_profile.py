"""--dosage window kernels at the size of a real window (150,000 variants x 765 samples, float32 calldata/DS): runs
net.filter_dosage_device a few times on device-resident dosages and prints the per-pass times and the bytes-based HBM
estimate.  Profile it with
    rocprofv3 --kernel-trace --stats -d OUT -o dosage -- python tools/dosage_window_profile.py
(profiles/dosage_window_kernels.md holds one such run)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from locator_amd.net import filter_dosage_device  # noqa: E402

V, N, REPS = 150_000, 765, 5
HBM_PEAK = 8.0e12          # MI355X spec, bytes/s


def main():
    g = torch.Generator(device="cuda").manual_seed(1)
    d = torch.rand((V, N), generator=g, device="cuda") * 2.0
    d[torch.rand((V, N), generator=g, device="cuda") < 0.01] = float("nan")
    order = np.random.default_rng(0).permutation(N).astype(np.int32)
    filter_dosage_device(d, order)                      # warm-up
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(REPS):
        e0.record()
        X, K = filter_dosage_device(d, order)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    flags_bytes = 4 * V * N + V
    rows_bytes = 4 * K * N + N * K           # kept variants read once, rows written once
    print(f"window {V} x {N}: K = {K}; filter_dosage_device (both passes, scan, one host sync) median {np.median(ms):.3f} ms")
    print(f"bytes: flags pass {flags_bytes / 1e6:.1f} MB, rows pass {rows_bytes / 1e6:.1f} MB; at 8 TB/s that is "
          f"{flags_bytes / HBM_PEAK * 1e3:.3f} + {rows_bytes / HBM_PEAK * 1e3:.3f} ms")


if __name__ == "__main__":
    main()
