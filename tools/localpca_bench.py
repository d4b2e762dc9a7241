#!/usr/bin/env python3
"""Time loc_grm_windows (grm_windows_kernel, csrc/grm_kernels.hip) against the forms it replaces, on seeded counts with allele
frequencies spread over 0.05 .. 0.95 and 5 % missing calls:

  windows       one loc_grm_windows launch for all windows (float32 [W][N][N]);
  windows_alt   the same launch from another build of the library (--alt_lib: `make -C locator_amd/csrc variant F=grm_kernels
                XDEF=-DGW_MIRROR_STRIDED TAG=gwstrided` stores the mirrored half from the registers, without the LDS
                transposition); its output must have the same bits;
  pairs_loop    loc_grm_pairs once per window (two launches and a double [N][N] each).  That entry point reads rows 16 bytes at
                a time, so every window start is moved down to a multiple of 16 sites: a few more sites, the timing of the loop
                a caller without loc_grm_windows would write;
  torch         Z formed in fp32 by torch (timed on its own: z_ms), then torch.bmm over equal windows, or one torch.mm per
                window where they are uneven;
  host          localpca.windows_host (float64 BLAS) on the first --host_windows windows, scaled to all by their sites;
  eigen         pca.components (numpy.linalg.eigh, float64) on the first --host_windows windows, scaled by their number: the
                host step that follows the launch in the command, and its share of launch + download + eigen.

Shapes: the golden VCF's 500 x 5,830 in windows of 100 sites, 1,000 x 100,000 in windows of 500, and 1,000 x 100,000 in uneven
windows of 20 .. 2,000 sites (what base-pair windows give).  Every device form is warmed once, then the forms are timed in turn,
--repeats times round (device events around each), and the medians are kept.  Writes one JSON object (and prints it)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from locator_amd import _abi, _lib  # noqa: E402
from locator_amd import localpca as L  # noqa: E402
from locator_amd import pca as P  # noqa: E402


def counts(N, K, rng):
    c = np.empty((N, K), dtype=np.int8)
    freq = rng.uniform(0.05, 0.95, K)
    for i0 in range(0, N, 64):
        c[i0:i0 + 64] = rng.binomial(2, np.broadcast_to(freq[None], (min(64, N - i0), K)))
        c[i0:i0 + 64][rng.random((min(64, N - i0), K)) < 0.05] = -1
    return c


def windows_of(K, spec, rng):
    if spec != "uneven":
        S = int(spec)
        return np.array([(v, min(v + S, K)) for v in range(0, K, S)], dtype=np.int64)
    cuts = [0]
    while cuts[-1] < K:
        cuts.append(min(K, cuts[-1] + int(rng.integers(20, 2001))))
    return np.array(list(zip(cuts[:-1], cuts[1:])), dtype=np.int64)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def one(N, K, spec, a, rng, alt):
    print(f"{N} x {K} windows {spec}: generating", file=sys.stderr, flush=True)
    c = counts(N, K, rng)
    mean, scale, _ = P.site_constants(c, 2)
    win = windows_of(K, spec, rng)
    W, sites = len(win), int((win[:, 1] - win[:, 0]).sum())
    lib = _lib.load()
    d_c, d_mean, d_scale, pitch = P._upload(c, mean, scale)
    d_win = torch.from_numpy(win).cuda()
    d_g = torch.empty((W, N, N), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def windows(which=lib):
        rc = which.loc_grm_windows(d_c.data_ptr(), N, K, pitch, d_mean.data_ptr(), d_scale.data_ptr(), d_win.data_ptr(), W,
                                   d_g.data_ptr(), stream)
        assert rc == 0, lib.loc_last_error()

    lo = win[:, 0] // 16 * 16
    d_g64 = torch.empty((N, N), dtype=torch.float64, device="cuda")
    work_bytes = max(int(lib.loc_grm_work_bytes(N, int(v1 - v0), 0)) for v0, v1 in zip(lo, win[:, 1]))
    work = torch.empty(max(work_bytes // 4, 4), dtype=torch.float32, device="cuda")

    def pairs_loop():
        for v0, v1 in zip(lo.tolist(), win[:, 1].tolist()):
            _lib.check(lib.loc_grm_pairs(d_c.data_ptr() + v0, N, v1 - v0, pitch, d_mean.data_ptr() + 4 * v0, d_scale.data_ptr() + 4 * v0,
                                         0, d_g64.data_ptr(), work.data_ptr(), work_bytes, stream), "loc_grm_pairs")

    equal = spec != "uneven" and K % int(spec) == 0
    d_z = [None]

    def form_z():
        z = (d_c[:, :K].to(torch.float32) - d_mean[None, :K]) * d_scale[None, :K]
        d_z[0] = torch.where(d_c[:, :K] < 0, torch.zeros_like(z), z)

    d_t = torch.empty((W, N, N), dtype=torch.float32, device="cuda")

    def torch_form():
        z = d_z[0]
        if equal:
            zw = z.view(N, W, K // W).permute(1, 0, 2)
            torch.bmm(zw, zw.transpose(1, 2), out=d_t)
        else:
            for w, (v0, v1) in enumerate(win.tolist()):
                torch.mm(z[:, v0:v1], z[:, v0:v1].T, out=d_t[w])

    forms = {"windows": windows, "pairs_loop": pairs_loop, "z": form_z, "torch": torch_form}
    if alt is not None:
        forms["windows_alt"] = lambda: windows(alt)
    print(f"{N} x {K} windows {spec}: timing {W} windows", file=sys.stderr, flush=True)
    torch.backends.cuda.matmul.allow_tf32 = False
    for fn in forms.values():                                               # warm-up: code objects, algorithm choice, clocks
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in forms}
    for _ in range(a.repeats):
        for k, fn in forms.items():
            ms[k].append(timed(fn))
    med = {k: float(np.median(v)) for k, v in ms.items()}

    windows()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    g = d_g.cpu().numpy()
    download_ms = (time.perf_counter() - t0) * 1e3
    same = None
    if alt is not None:
        windows(alt)
        torch.cuda.synchronize()
        same = bool(torch.equal(d_g, torch.from_numpy(g).cuda()))
        assert same, "the two builds disagree"
    t = d_t.cpu().numpy()
    # results must agree: both are fp32 sums of the same products in different orders
    tol = (int((win[:, 1] - win[:, 0]).max()) + 8) * 2.0 ** -23 * np.abs(g).max()
    assert np.abs(g - t).max() <= tol, (np.abs(g - t).max(), tol)

    nh = min(a.host_windows, W)
    t0 = time.perf_counter()
    Gh = L.windows_host(c, mean, scale, win[:nh])
    host_ms = (time.perf_counter() - t0) * 1e3 * sites / max(int((win[:nh, 1] - win[:nh, 0]).sum()), 1)
    bound = np.stack([(v1 - v0 + 8) * 2.0 ** -24 for v0, v1 in win[:nh]])
    az = np.abs(P.z_host(c[:, :int(win[nh - 1, 1])], mean[:int(win[nh - 1, 1])], scale[:int(win[nh - 1, 1])]))
    worst = max(float((np.abs(g[w] - Gh[w]) / np.maximum(bound[w] * (az[:, v0:v1] @ az[:, v0:v1].T), 1e-300)).max())
                for w, (v0, v1) in enumerate(win[:nh]))
    assert worst <= 1.0, "device outside the fp32 bound of the definition"
    used = L.used_sites(scale, win)
    t0 = time.perf_counter()
    for w in range(nh):
        P.components(g[w], int(used[w]), 2)
    eigen_ms = (time.perf_counter() - t0) * 1e3 * W / nh

    out_bytes = 4 * W * N * N
    tiles = (N + 127) // 128
    flops = 2 * (tiles * (tiles + 1) // 2) * 128 * 128 * int((((win[:, 1] - 1) // 32 - win[:, 0] // 32 + 1) * 32).sum())
    out = {"samples": N, "sites": K, "windows": spec, "n_windows": W, "window_sites": sites, "output_bytes": out_bytes,
           "median_ms": {k: round(v, 4) for k, v in med.items()}, "min_ms": {k: round(min(v), 4) for k, v in ms.items()},
           "torch_with_z_ms": round(med["z"] + med["torch"], 4),
           "windows_output_gb_per_s": round(out_bytes / (med["windows"] * 1e-3) / 1e9, 1),
           "windows_mfma_flops_issued": flops, "windows_tflops_issued": round(flops / (med["windows"] * 1e-3) / 1e12, 2),
           "pairs_loop_over_windows": round(med["pairs_loop"] / med["windows"], 2),
           "torch_with_z_over_windows": round((med["z"] + med["torch"]) / med["windows"], 2),
           "host_windows_timed": nh, "host_float64_ms_scaled": round(host_ms, 1), "host_over_windows": round(host_ms / med["windows"], 1),
           "error_over_bound_on_those": round(worst, 4), "download_ms": round(download_ms, 2),
           "host_eigen_ms_scaled": round(eigen_ms, 1),
           "eigen_share_of_launch_download_eigen": round(eigen_ms / (eigen_ms + download_ms + med["windows"]), 4)}
    if same is not None:
        out["alt_same_bits"] = same
        out["alt_over_windows"] = round(med["windows_alt"] / med["windows"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["500x5830x100", "1000x100000x500", "1000x100000xuneven"])
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--host_windows", type=int, default=4, help="windows the float64 forms and the eigen step are timed on")
    ap.add_argument("--alt_lib", default=None, help="another build of liblocator_hip.so to time loc_grm_windows from as well")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "localpca_bench.json"))
    a = ap.parse_args()
    alt = None
    if a.alt_lib is not None:
        alt = C.CDLL(os.path.abspath(a.alt_lib))
        alt.loc_grm_windows.restype, alt.loc_grm_windows.argtypes = _abi.ALL_PROTOTYPES["loc_grm_windows"]
    rng = np.random.default_rng(a.seed)
    runs = []
    for shape in a.shapes:
        N, K, spec = shape.split("x")
        runs.append(one(int(N), int(K), spec, a, rng, alt))
    out = {"kernel": "loc_grm_windows", "device": torch.cuda.get_device_name(0), "repeats": a.repeats,
           "alt_lib": None if a.alt_lib is None else "grm_kernels.hip with -DGW_MIRROR_STRIDED", "runs": runs}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
