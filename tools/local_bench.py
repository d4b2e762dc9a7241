#!/usr/bin/env python3
"""Time loc_paint_local (csrc/local_kernels.hip) next to loc_paint_copy (csrc/paint_kernels.hip, which this kernel's addition
left as it was) on the inputs of tools/paint_bench.py: planted haplotypes at --shapes samples x sites, default 128 x 2048,
512 x 2048 and 2048 x 2048 (H = 256, 1,024 and 4,096 columns), every haplotype a donor and a recipient, the same h, rec, rho and
block for both, one launch each.  loc_paint_local runs in two configurations: 8 channels with windows of 64 sites, and 3 channels
with one site a window.  The three are timed in the same run, interleaved (one launch of each in a rotating order, --launches
times after --warmup launches of each), event-timed; the medians, the smallest times, the ratios of the medians to
loc_paint_copy's and the spread of loc_paint_copy's own repeats ((largest - smallest) / median) are reported.  On the first
shape the device's window means of --host_recipients recipients are held to the allowance of the tests against
ancestry.local_host(float64), and ll and n_donors to loc_paint_copy's bits.
With --ablate, the timing-ablation build without the contraction at a window's end (`make -C locator_amd/csrc variant
F=local_kernels XDEF=-DPK_ABLATE=32 TAG=lk32`; it stores zeros) is timed on every shape: what it saves is what the window ends
cost.  Writes one JSON object (and prints it)."""
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
from locator_amd import ancestry as AN  # noqa: E402
from locator_amd import baselines as BL  # noqa: E402
from locator_amd import paint as PT  # noqa: E402
from tools.paint_bench import planted  # noqa: E402

CONFIGS = {"c8_w64": (8, 64), "c3_w1": (3, 1)}            # name: (channels, sites a window)


def bind(path):
    lib = C.CDLL(path)
    for table in (_abi.EXTENSIONS["paint"], _abi.OPEN["local"]):
        for name, (res, args) in table.prototypes.items():
            getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    return lib


def one(N, K, a, rng, lib, ablated, first):
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
    d_ll, d_nd = (torch.empty((1 + len(CONFIGS), H), dtype=dt, device="cuda") for dt in (torch.float64, torch.int32))
    work_bytes = int(lib.loc_paint_work_bytes(H, K, H, a.block))
    work = torch.empty(max(work_bytes // 4, 4), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    head = (d_h.data_ptr(), H, K, buf.shape[1], d_donor.data_ptr(), d_owner.data_ptr(), d_rec.data_ptr(), H, d_rho.data_ptr(), theta, a.block)
    tail = (work.data_ptr(), work_bytes, stream)
    v_all = np.concatenate([rng.uniform(-1.0, 1.0, (7, H)), np.ones((1, H))]).astype(np.float32)
    held = {}
    for n, (name, (Cn, size)) in enumerate(CONFIGS.items(), 1):
        win = np.array([[s, min(s + size, K)] for s in range(0, K, size)], dtype=np.int32)
        v = np.ascontiguousarray(v_all[-Cn:])
        d_v, d_win = put(v), put(win)
        d_out = torch.empty((H, len(win), Cn), dtype=torch.float32, device="cuda")
        held[name] = (v, win, d_v, d_win, d_out, n)
    calls = {"copy": lambda which: lib.loc_paint_copy(*head, d_share.data_ptr(), d_chunks.data_ptr(), d_ll[0].data_ptr(), d_nd[0].data_ptr(),
                                                      *tail)}
    for name, (v, win, d_v, d_win, d_out, n) in held.items():
        calls[name] = (lambda which, v=v, win=win, d_v=d_v, d_win=d_win, d_out=d_out, n=n:
                       which.loc_paint_local(*head, d_v.data_ptr(), len(v), H, d_win.data_ptr(), len(win), d_out.data_ptr(),
                                             d_ll[n].data_ptr(), d_nd[n].data_ptr(), *tail))
    names = list(calls)

    def launch(name, which):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = calls[name](which)
        e1.record()
        torch.cuda.synchronize()
        assert rc == 0, (name, rc)
        return e0.elapsed_time(e1)

    def interleaved(which, launches):
        ms = {name: [] for name in names}
        for n in range(a.warmup + launches):
            for name in names[n % len(names):] + names[:n % len(names)]:
                t = launch(name, which)
                if n >= a.warmup:
                    ms[name].append(t)
        return ms

    print(f"{N} x {K}: timing", file=sys.stderr, flush=True)
    ms = interleaved(lib, a.launches)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    ll, nd = d_ll.cpu().numpy(), d_nd.cpu().numpy()
    assert all(np.array_equal(ll[n].view(np.uint64), ll[0].view(np.uint64)) and np.array_equal(nd[n], nd[0]) for n in range(1, len(ll))), \
        "ll / n_donors differ"
    out = {"samples": N, "sites": K, "columns": H, "recipients": H, "block": a.block, "work_bytes": work_bytes,
           "launches_each": a.launches, "warmup_each": a.warmup,
           "copy_median_ms": round(med["copy"], 3), "copy_min_ms": round(min(ms["copy"]), 3),
           "copy_spread ((max - min) / median of its own repeats)": round((max(ms["copy"]) - min(ms["copy"])) / med["copy"], 4),
           "ll_and_n_donors_equal_loc_paint_copy": True}
    for name, (Cn, size) in CONFIGS.items():
        out.update({f"{name}_channels": Cn, f"{name}_window_sites": size, f"{name}_windows": int(len(held[name][1])),
                    f"{name}_median_ms": round(med[name], 3), f"{name}_min_ms": round(min(ms[name]), 3),
                    f"{name}_over_copy": round(med[name] / med["copy"], 4)})
    if ablated is not None:
        m = interleaved(ablated, max(3, a.launches // 2))
        for name in CONFIGS:
            out[f"ablation_32_{name}_median_ms (no contraction at a window's end; results wrong)"] = round(float(np.median(m[name])), 3)
        out["ablation_32_copy_median_ms_beside_it (the product kernel)"] = round(float(np.median(m["copy"])), 3)
    if first:
        n = min(a.host_recipients, H)
        sub = rec[:: max(1, H // n)][:n]
        print(f"{N} x {K}: the definition on {len(sub)} recipients", file=sys.stderr, flush=True)
        interleaved(lib, 1)                                   # the product library's results, whichever library ran last
        for name, (v, win, _, _, d_out, _) in held.items():
            got = d_out.cpu().numpy()[sub]
            want = AN.local_host(hap, donor, owner, sub, rho, theta, v, win)[0]
            w32 = AN.local_host(hap, donor, owner, sub, rho, theta, v, win, np.float32)[0]
            sites = (win[:, 1] - win[:, 0])[None, :, None]
            dist = lambda g: float(np.abs(g.astype(np.float64) / sites - want / sites).max())
            allow = max(8 * dist(w32), 2.0 ** -21)
            ratio = dist(got) / allow
            assert ratio <= 1.0, ("device outside the allowance of the definition", name, ratio)
            out.update({f"{name}_error_over_allowance": round(ratio, 4), f"{name}_allowance": allow})
        out["host_float64_recipients"] = int(len(sub))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["128x2048", "512x2048", "2048x2048"])
    ap.add_argument("--switch", type=float, default=0.01)
    ap.add_argument("--block", type=int, default=0)
    ap.add_argument("--launches", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host_recipients", type=int, default=8)
    ap.add_argument("--ablate", action="store_true", help="also time build/liblocator_hip_lk32.so")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_bench.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    lib = _lib.load()
    ablated = bind(os.path.join(ROOT, "build", "liblocator_hip_lk32.so")) if a.ablate else None
    runs = []
    for n, shape in enumerate(a.shapes):
        N, K = (int(v) for v in shape.split("x"))
        runs.append(one(N, K, a, rng, lib, ablated, n == 0))
    out = {"kernel": "loc_paint_local beside loc_paint_copy", "device": torch.cuda.get_device_name(0), "switch": a.switch, "runs": runs}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
