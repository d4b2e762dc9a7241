#!/usr/bin/env python3
"""Time loc_paint_copy (csrc/paint_kernels.hip) on planted haplotypes (mosaics of founder haplotypes as tests/paint_util.py
plants them, generated here from --seed) at --shapes samples x sites, default 150 x 600 (the size of the prototype), 500 x 5,830
(the golden VCF) and 1,000 x 100,000 (the project's scale): every haplotype a donor and a recipient, one launch, event-timed,
--launches times (the median and the smallest).  Next to it, on the first shape only:
  the same recursion as torch tensor operations, one batch of all recipients a site (torch_copy);
  paint.copy_host in float64 on --host_recipients recipients, its time scaled to all recipients and to the other shapes by
  recipients x sites x columns and LABELLED as extrapolated;
  the device result held to the allowance of the tests against that float64 answer.
With --ablate, the timing-ablation builds of the kernel (`make -C locator_amd/csrc variant F=paint_kernels XDEF=-DPK_ABLATE=<bits>
TAG=pk<bits>` for bits 1, 2, 4, 7: no cross-lane sums, no alleles and constant emissions, no scratch rows, all three) are timed
on every shape: what a build saves is what that part of a wave's site step costs while the others run (their results are wrong by
construction).  Writes one JSON object (and prints it)."""
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
from locator_amd import paint as PT  # noqa: E402

ABLATIONS = {1: "no cross-lane sums", 2: "no alleles read, constant emissions", 4: "no scratch rows", 7: "all three"}


def planted(N, K, rng, founders=8, stay=0.98, width=0.12, flips=0.01, missing=0.03):
    found = rng.integers(0, 2, (founders, K)).astype(np.int8)
    place = np.linspace(0.0, 1.0, founders)
    hap = np.empty((K, 2 * N), dtype=np.int8)
    for s in range(N):
        w = np.exp(-(rng.uniform() - place) ** 2 / (2 * width ** 2))
        for a in range(2):
            new = rng.random(K) >= stay
            new[0] = True
            pick = rng.choice(founders, K, p=w / w.sum())
            hap[:, 2 * s + a] = found[pick[np.maximum.accumulate(np.where(new, np.arange(K), 0))], np.arange(K)]
    for j0 in range(0, K, 4096):
        part = hap[j0:j0 + 4096]
        part ^= (rng.random(part.shape) < flips).astype(np.int8)
        part[rng.random(part.shape) < missing] = -1
    return hap


def bind(path):
    lib = C.CDLL(path)
    for name, (res, args) in _abi.EXTENSIONS["paint"].prototypes.items():
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    return lib


def torch_copy(h, dn, rec, rho, theta):
    """The recursion of paint.copy_host in float32 torch operations on the device, all recipients a site: (share, chunks, ll)."""
    K, (R, H) = h.shape[0], dn.shape
    f = torch.float32
    u = (1.0 / dn.sum(dim=1, keepdim=True).to(f))
    one, th = torch.tensor(1.0, dtype=f, device=h.device), torch.tensor(theta, dtype=f, device=h.device)

    def emit(j):
        a, x = h[j, rec][:, None], h[j, :H][None, :]
        e = torch.where((a < 0) | (x < 0), one, torch.where(a == x, one - th, th))
        return torch.where(dn, e, torch.zeros((), dtype=f, device=h.device))

    ah_all = torch.empty((K, R, H), dtype=f, device=h.device)
    c_all = torch.empty((K, R), dtype=f, device=h.device)
    ah = torch.zeros((R, H), dtype=f, device=h.device)
    ll = torch.zeros(R, dtype=torch.float64, device=h.device)
    for j in range(K):
        a = emit(j) * ((1 - rho[j]) * ah + rho[j] * u)
        c = a.sum(dim=1)
        ah = a * (1 / c)[:, None]
        ah_all[j], c_all[j] = ah, c
        ll += torch.log(c.double())
    b = u.expand(R, H).clone()
    sa, ca = torch.zeros_like(ah), torch.zeros_like(ah)
    for j in range(K - 1, -1, -1):
        t = emit(j) * b
        g = ah_all[j] * b
        T, G = t.sum(dim=1), g.sum(dim=1)
        invG = torch.where(G >= 1.1754944e-38, 1 / G, torch.zeros_like(G))
        gam = g * invG[:, None]
        sa += gam
        ru = rho[j] * u
        ca += gam if j == 0 else t * ((ru[:, 0] * invG) * (1 / c_all[j]))[:, None]
        b = ((1 - rho[j]) * (1 / T))[:, None] * t + ru
    return sa / K, ca, ll


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
    d_ll, d_nd = torch.empty(H, dtype=torch.float64, device="cuda"), torch.empty(H, dtype=torch.int32, device="cuda")
    lib = libs[0]
    work_bytes = int(lib.loc_paint_work_bytes(H, K, H, a.block))
    work = torch.empty(max(work_bytes // 4, 4), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def timed(which, launches):
        ms = []
        for _ in range(launches + 1):                                       # the first is the warm-up
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = which.loc_paint_copy(d_h.data_ptr(), H, K, buf.shape[1], d_donor.data_ptr(), d_owner.data_ptr(), d_rec.data_ptr(), H,
                                      d_rho.data_ptr(), theta, a.block, d_share.data_ptr(), d_chunks.data_ptr(), d_ll.data_ptr(),
                                      d_nd.data_ptr(), work.data_ptr(), work_bytes, stream)
            assert rc == 0, rc
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms[1:])), float(min(ms[1:]))

    print(f"{N} x {K}: timing", file=sys.stderr, flush=True)
    med, low = timed(lib, a.launches)
    got = (d_share.cpu().numpy(), d_chunks.cpu().numpy(), d_ll.cpu().numpy())
    cells = H * K * H
    out = {"samples": N, "sites": K, "columns": H, "recipients": H, "block": a.block, "work_bytes": work_bytes,
           "copy_median_ms": round(med, 3), "copy_min_ms": round(low, 3), "recipient_site_column_cells": cells,
           "giga_cells_per_s": round(cells / (med * 1e-3) / 1e9, 2),
           "scratch_bytes_written_and_read": 2 * 4 * cells,
           "scratch_tb_per_s": round(2 * 4 * cells / (med * 1e-3) / 1e12, 3),
           "share_rows_sum_to_one_within": float(np.abs(got[0].astype(np.float64).sum(axis=1) - 1).max())}
    for bits, lab in sorted(libs.items()):
        if bits:
            m, _ = timed(lab, max(1, a.launches // 2))
            out[f"ablation_{bits}_median_ms ({ABLATIONS[bits]}; results wrong)"] = round(m, 3)
    if first:
        n = min(a.host_recipients, H)
        sub = rec[:: max(1, H // n)][:n]
        print(f"{N} x {K}: the definition on {len(sub)} recipients", file=sys.stderr, flush=True)
        t0 = time.perf_counter()
        want = PT.copy_host(hap, donor, owner, sub, rho, theta)
        host_s = time.perf_counter() - t0
        w32 = PT.copy_host(hap, donor, owner, sub, rho, theta, np.float32)
        pick = lambda r: (r[0][sub], r[1][sub], r[2][sub])
        dist = lambda g: (float(np.abs(g[0] - want[0]).max()), float((np.abs(g[1] - want[1]) / (1 + np.abs(want[1]))).max()),
                          float((np.abs(g[2] - want[2]) / np.abs(want[2])).max()))
        allow = [max(8 * v, 2.0 ** -21) for v in dist(w32)]
        ratios = [d / al for d, al in zip(dist(pick(got)), allow)]
        assert max(ratios) <= 1.0, ("device outside the allowance of the definition", ratios)
        dn = torch.from_numpy(owner[None, :] != owner[rec][:, None]).cuda()
        h64 = d_h.to(torch.int32)
        torch_copy(h64, dn, d_rec.long(), d_rho, theta)                     # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ts = torch_copy(h64, dn, d_rec.long(), d_rho, theta)
        torch.cuda.synchronize()
        torch_ms = (time.perf_counter() - t0) * 1e3
        tg = (ts[0].cpu().numpy(), ts[1].cpu().numpy(), ts[2].cpu().numpy())
        out.update({"error_over_allowance (share, chunks, ll)": [round(r, 4) for r in ratios],
                    "torch_per_site_ms": round(torch_ms, 1), "torch_over_kernel": round(torch_ms / med, 1),
                    "torch_error_over_allowance": [round(d / al, 4) for d, al in zip(dist(pick(tg)), allow)],
                    "host_float64_recipients": int(len(sub)), "host_float64_s_on_those": round(host_s, 2),
                    "host_float64_s_all_recipients_EXTRAPOLATED": round(host_s * H / len(sub), 1),
                    "host_ns_per_cell": round(host_s * 1e9 / (len(sub) * K * H), 2)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["150x600", "500x5830", "1000x100000"])
    ap.add_argument("--switch", type=float, default=0.01)
    ap.add_argument("--block", type=int, default=0)
    ap.add_argument("--launches", type=int, default=4)
    ap.add_argument("--host_recipients", type=int, default=16)
    ap.add_argument("--ablate", action="store_true", help="also time build/liblocator_hip_pk{1,2,4,7}.so")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "paint_bench.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    libs = {0: _lib.load()}
    if a.ablate:
        for bits in ABLATIONS:
            libs[bits] = bind(os.path.join(ROOT, "build", f"liblocator_hip_pk{bits}.so"))
    runs = []
    for n, shape in enumerate(a.shapes):
        N, K = (int(v) for v in shape.split("x"))
        runs.append(one(N, K, a, rng, libs, n == 0))
    per_cell = runs[0]["host_ns_per_cell"]
    for r in runs[1:]:
        r["host_float64_s_EXTRAPOLATED from the first shape by cells"] = round(per_cell * 1e-9 * r["recipient_site_column_cells"], 0)
    out = {"kernel": "loc_paint_copy", "device": torch.cuda.get_device_name(0), "switch": a.switch, "runs": runs}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
