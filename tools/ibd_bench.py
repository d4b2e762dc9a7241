#!/usr/bin/env python3
"""Time loc_ibd_pack, loc_ibd_scan and loc_ibd_fill (csrc/ibd_kernels.hip) on planted haplotypes (mosaics of founder haplotypes as
tools/paint_bench.py plants them, generated here from --seed) at --shapes samples x sites, default 1,000 x 100,000 (the shape
every baseline reports) and 8,000 x 20,000 (a cohort the paint command would have to thin): all rows against all columns in
batches of --budget_gb / (28 H) rows, event-timed, --launches times after a warm-up (the median and the smallest).
Next to it, per shape:
  the scan of an all-zero matrix of the same shape: no discordant site, so what is left is the stream of the words
  (`scan_stream_only_ms`); the scan is bound by the walk over the events where it takes much longer than that, else by the stream;
  the discordant-site events, estimated from --sample_pairs random column pairs, over the scan time;
  the bytes the lanes ask for (16 a pair and word; a row's own words are wave-uniform scalar loads and not counted);
  a torch form of the exact-run case (gap_sites = 0): one row at a time, the agreement of the row with every column as a
  [H][K] tensor, the start of every site's run by a running maximum (cummax) of the last break, then masked sums and maxima;
  timed on --torch_rows rows, held equal to the kernel's answer on them and scaled to all rows, LABELLED as extrapolated;
  ibd.segments_host on --host_rows rows, scaled by pairs, LABELLED as extrapolated.
With --golden the command runs on the golden VCF on the device and its placement error is recorded.
Writes one JSON object (and prints it)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from locator_amd import _lib  # noqa: E402
from locator_amd import baselines as BL  # noqa: E402
from locator_amd import ibd as IB  # noqa: E402
from tools.paint_bench import planted  # noqa: E402


def torch_exact_rows(h, owner, first, x, P, rows):
    """count, length, longest of `rows` for gap_sites = 0 in torch operations: [len(rows)][H] each."""
    K, H = h.shape[0], len(owner)
    site = torch.arange(K, device=h.device)
    next_first = torch.cat([first[1:], torch.ones(1, dtype=torch.bool, device=h.device)])
    outs = [torch.zeros((len(rows), H), dtype=torch.int64, device=h.device) for _ in range(3)]
    for i, p in enumerate(rows):
        mine = h[:, p:p + 1]
        agree = ((mine < 0) | (h < 0) | (mine == h)).T                                   # [H][K]
        # the site a run began at: one past the last discordant site, or the last chromosome start, whichever is later
        brk = torch.where(agree, torch.where(first, site, torch.full_like(site, -1))[None, :], (site + 1)[None, :])
        start = torch.cummax(brk, dim=1).values
        nxt = torch.cat([agree[:, 1:], torch.zeros((H, 1), dtype=torch.bool, device=h.device)], dim=1)
        end = agree & (next_first[None, :] | ~nxt)
        n = site[None, :] - start + 1
        ln = x[None, :] - x[start.clamp(min=0, max=K - 1)]
        keep = end & (n >= P.seed_sites) & (ln >= P.seed_len) & (ln >= P.min_len)
        live = (torch.arange(H, device=h.device) > p) & (owner != owner[p])
        keep &= live[:, None]
        lk = torch.where(keep, ln, torch.zeros_like(ln))
        outs[0][i], outs[1][i], outs[2][i] = keep.sum(dim=1), lk.sum(dim=1), lk.max(dim=1).values
    return outs


def one(N, K, a, rng, P):
    print(f"{N} x {K}: generating", file=sys.stderr, flush=True)
    hap = planted(N, K, rng)
    H = 2 * N
    owner = np.repeat(np.arange(N, dtype=np.int32), 2)
    first = np.zeros(K, dtype=bool)
    first[0] = True
    x = np.arange(K, dtype=np.int64) * 100
    lib = _lib.load()
    buf = BL.padded(hap)
    put = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
    d_h, d_owner, d_first, d_x = put(buf), put(owner), put(IB.pack_first(first, K).view(np.int64)), put(x)
    W, wp = (K + 63) // 64, (H + 7) // 8 * 8
    d_bits = torch.empty((2, W, wp), dtype=torch.int64, device="cuda")
    d_zero = torch.zeros((2, W, wp), dtype=torch.int64, device="cuda")
    d_zero[1] = -1                                                                   # every allele 0 and valid: no discordant site
    stream = torch.cuda.current_stream().cuda_stream
    step = max(1, int(a.budget_gb * (1 << 30)) // (28 * H))
    n = min(step, H)
    d_count = torch.empty((n, H), dtype=torch.int32, device="cuda")
    d_length, d_longest = (torch.empty((n, H), dtype=torch.int64, device="cuda") for _ in range(2))

    def timed(fn, launches):
        ms = []
        for _ in range(launches + 1):                                                # the first is the warm-up
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return round(float(np.median(ms[1:])), 3), round(float(min(ms[1:])), 3)

    def pack():
        assert lib.loc_ibd_pack(d_h.data_ptr(), H, K, buf.shape[1], d_bits.data_ptr(), wp, stream) == 0

    def scan_args(bits, p0, R, par):
        return (bits.data_ptr(), wp, H, K, d_owner.data_ptr(), d_first.data_ptr(), d_x.data_ptr(), p0, R, *par)

    def scan(bits=d_bits, par=P):
        for p0 in range(0, H, step):
            R = min(step, H - p0)
            assert lib.loc_ibd_scan(*scan_args(bits, p0, R, par), d_count.data_ptr(), d_length.data_ptr(), d_longest.data_ptr(), stream) == 0

    totals = {}

    def scan_and_fill():
        segs = 0
        for p0 in range(0, H, step):
            R = min(step, H - p0)
            assert lib.loc_ibd_scan(*scan_args(d_bits, p0, R, P), d_count.data_ptr(), d_length.data_ptr(), d_longest.data_ptr(), stream) == 0
            flat = d_count[:R].view(-1)
            ends = torch.cumsum(flat, dim=0, dtype=torch.int64)
            total = int(ends[-1])
            off = (ends - flat).contiguous()
            sa, sb = (torch.empty(max(total, 1), dtype=torch.int32, device="cuda") for _ in range(2))
            assert lib.loc_ibd_fill(*scan_args(d_bits, p0, R, P), off.data_ptr(), total, sa.data_ptr(), sb.data_ptr(), stream) == 0
            segs += total
        totals["segments"] = segs

    print(f"{N} x {K}: timing", file=sys.stderr, flush=True)
    pack_ms = timed(pack, a.launches)
    scan_ms = timed(scan, a.launches)
    both_ms = timed(scan_and_fill, max(1, a.launches // 2))
    zero_ms = timed(lambda: scan(d_zero), a.launches)
    pairs = int((owner[:, None] != owner[None, :]).sum()) // 2 if H <= 4096 else H * (H - 2) // 2
    ps, qs = rng.integers(0, H, a.sample_pairs), rng.integers(0, H, a.sample_pairs)
    ok = owner[ps] != owner[qs]
    hp, hq = hap[:, ps[ok]], hap[:, qs[ok]]
    frac = float(((hp >= 0) & (hq >= 0) & (hp != hq)).mean())
    events = frac * K * pairs
    lane_bytes = pairs * W * 16
    out = {"samples": N, "sites": K, "columns": H, "pairs": pairs, "words": W, "rows_a_launch": n, "launches_a_scan": -(-H // step),
           "pack_median_ms": pack_ms[0], "pack_min_ms": pack_ms[1], "pack_bytes_read": int(K) * int(buf.shape[1]),
           "pack_gb_per_s": round(K * buf.shape[1] / (pack_ms[0] * 1e-3) / 1e9, 1),
           "scan_median_ms": scan_ms[0], "scan_min_ms": scan_ms[1], "scan_and_fill_median_ms (with the prefix sums and allocations)": both_ms[0],
           "fill_median_ms (the difference)": round(both_ms[0] - scan_ms[0], 3), "segments": totals["segments"],
           "scan_stream_only_ms (all-zero matrix, no event)": zero_ms[0],
           "discordant_fraction (sampled pairs)": round(frac, 4), "events_ESTIMATED": int(events),
           "giga_events_per_s": round(events / (scan_ms[0] * 1e-3) / 1e9, 2),
           "lane_bytes_read": lane_bytes, "lane_tb_per_s": round(lane_bytes / (scan_ms[0] * 1e-3) / 1e12, 3),
           "lane_tb_per_s_stream_only": round(lane_bytes / (zero_ms[0] * 1e-3) / 1e12, 3),
           "bound_by": "the walk over the events" if scan_ms[0] > 2 * zero_ms[0] else "the stream of the words"}
    # the torch form of the exact-run case against the kernel on the same rows
    exact = P._replace(gap_sites=0)
    rows = list(range(0, H, max(1, H // a.torch_rows)))[:a.torch_rows]
    th, tf = d_h[:, :H].to(torch.int8), put(first)
    torch_exact_rows(th, d_owner, tf, d_x, exact, rows[:1])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tc = torch_exact_rows(th, d_owner, tf, d_x, exact, rows)
    torch.cuda.synchronize()
    torch_ms = (time.perf_counter() - t0) * 1e3
    exact_ms = timed(lambda: scan(par=exact), a.launches)
    for i, p in enumerate(rows):
        assert lib.loc_ibd_scan(*scan_args(d_bits, p, 1, exact), d_count.data_ptr(), d_length.data_ptr(), d_longest.data_ptr(), stream) == 0
        torch.cuda.synchronize()
        assert torch.equal(tc[0][i], d_count[0].long()) and torch.equal(tc[1][i], d_length[0]) and torch.equal(tc[2][i], d_longest[0]), p
    out.update({"exact_scan_median_ms (gap_sites 0)": exact_ms[0], "torch_exact_rows": len(rows), "torch_exact_ms_on_those": round(torch_ms, 1),
                "torch_exact_ms_all_rows_EXTRAPOLATED (rows do equal work in this form)": round(torch_ms * H / len(rows), 0),
                "torch_over_kernel_EXTRAPOLATED": round(torch_ms * H / len(rows) / exact_ms[0], 1)})
    del th, tc
    hrows = range(0, a.host_rows)
    t0 = time.perf_counter()
    want = IB.segments_host(hap, owner, first, x, P, hrows, segments=False)
    host_s = time.perf_counter() - t0
    assert lib.loc_ibd_scan(*scan_args(d_bits, 0, a.host_rows, P), d_count.data_ptr(), d_length.data_ptr(), d_longest.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    assert np.array_equal(d_count[:a.host_rows].cpu().numpy(), want[0]) and np.array_equal(d_length[:a.host_rows].cpu().numpy(), want[1])
    host_pairs = int(sum((owner[p + 1:] != owner[p]).sum() for p in hrows))
    out.update({"host_rows": a.host_rows, "host_s_on_those": round(host_s, 2),
                "host_s_all_pairs_EXTRAPOLATED by pairs": round(host_s * pairs / host_pairs, 0)})
    return out


def golden():
    from tests import paint_util as PU
    with tempfile.TemporaryDirectory() as tmp:
        stem = os.path.join(tmp, "g")
        t0 = time.perf_counter()
        IB.main(["--vcf", PU.VCF, "--sample_data", PU.SAMPLE_DATA, "--out", stem, "--silence"])
        wall = time.perf_counter() - t0
        s = json.load(open(stem + "_ibd_summary.json"))
    s["command_wall_s"] = round(wall, 2)
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["1000x100000", "8000x20000"])
    ap.add_argument("--params", nargs=6, type=int, default=[64, 0, 16, 1, IB.NO_LIMIT, 0], help="seed_sites seed_len extend_sites gap_sites gap_len min_len")
    ap.add_argument("--launches", type=int, default=4)
    ap.add_argument("--budget_gb", type=float, default=4.0)
    ap.add_argument("--sample_pairs", type=int, default=2000)
    ap.add_argument("--torch_rows", type=int, default=4)
    ap.add_argument("--host_rows", type=int, default=1)
    ap.add_argument("--golden", action="store_true")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ibd_bench.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    P = IB.check_params(a.params)
    runs = [one(*(int(v) for v in shape.split("x")), a, rng, P) for shape in a.shapes]
    out = {"kernels": "loc_ibd_pack, loc_ibd_scan, loc_ibd_fill", "device": torch.cuda.get_device_name(0), "params": P._asdict(), "runs": runs,
           "paint_recorded_s_at_1000x100000 (context only: another computation)": 0.85}
    if a.golden:
        out["golden"] = golden()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
