#!/usr/bin/env python3
"""`python -m locator_amd.phase`: haplotypes of unphased calls from the diploid form of the haplotype copying model of the paint
command (locator_amd/paint.py: Li & Stephens 2003).  A sample's two haplotypes copy from two donor haplotypes at once; the most
likely pair of copying paths (Viterbi) says, at every heterozygous call, which copy carries allele 1.  Every sample is re-phased
against the previous round's haplotypes of its nearest samples, for a few rounds.  The output is a callset store that `paint`,
`ibd`, `impute` and `locator --zarr ... --phased` accept as it stands.

  python -m locator_amd.phase --vcf calls.vcf.gz --out out/test [--states 64] [--rounds 10] [--check]

  model       `viterbi_host(h, rec, don, rho, theta, dtype)` -> (first [R][K] int8, ll [R] float64, n_switch [R], n_tied [R],
              n_donors [R] int32), every operation in `dtype`, rounded on its own.
                h [K][pitch] int8, site-major as in paint: column 2 s + a is allele a of sample s, 0 or 1, negative = missing:
                  the current estimate.  rec [R]: the samples to phase.  don [R][S] int32, 2 <= S <= 64: the donor columns of each
                  recipient, -1 = none, never one of the recipient's own two columns, repeats allowed.  rho [K] in [0, 1] as in
                  paint (rho[0] counts as 1; 1 at a chromosome's first site), theta in [1e-7, 0.5].
                A slot d is valid where don[d] >= 0, D of them, u = 1 / D.  A state is an ordered pair (d1, d2) of slots.
                q(x, a) = 1 - theta where the donor allele x == a, theta where not, 1/2 where x is missing.  The recipient's
                  genotype g = h[2s] + h[2s+1], missing where either is.  e(g; x, y) = q(x,0) q(y,0) for g = 0, q(x,1) q(y,1)
                  for g = 2, q(x,1) q(y,0) + q(x,0) q(y,1) for g = 1, 1 for g missing: `emission_table`, 4 x 3 x 3, formed once;
                  e = 0 where d1 or d2 is no valid slot.
                v_(-1) = 1 at the pairs of valid slots, else 0.  R(d) = max_d' v(d, d') and arg(d) the lowest such d'; G = max R
                  at the lowest flat index d S + arg(d).  Step j with r = rho_j, om = 1 - r, ru = r u, t = om + ru, tt = t t,
                  tr = t ru, rr = ru ru:
                    a = tt v(d1, d2)                  stay
                    b = tr max(R(d1), R(d2))          row where R(d1) >= R(d2): from (d1, arg(d1)); else column: from (arg(d2), d2)
                    c = rr G                          both: from G's pair
                    best = a, then b if b > best, then c if c > best: stay before row, row before column, column before both
                    v'(d1, d2) = e best;  m = max v';  v = v' (1 / m);  ll += log m in float64.
                e is a commutative sum of products, so e and with it v are symmetric in (d1, d2) bit for bit: the column maximum
                  max_d' v(d', d2) IS the row maximum R(d2), and the column step's predecessor (arg(d2), d2) is read off row d2.
                  The definition relies on this; it holds for repeated donor columns and in every float type.
                The end state is the lowest flat index of max v_(K-1); the traceback follows the predecessors.  n_switch adds 1
                  for a row or column step and 2 for both (sites j >= 1).  At a site of the path (d1, d2) with donor alleles
                  (x, y) where g = 1: the first copy gets allele 1 if q(x,1) q(y,0) > q(x,0) q(y,1), 0 if that product is
                  smaller, and keeps the recipient's current first allele on equality (n_tied adds 1).  Homozygous and missing
                  calls stay as they are.  A recipient with D = 0 keeps its calls: ll = 0, zeros.
                rho_j = 1 makes a = b = c scale the same, so the path is free to restart there; where rho = 1 at every site the
                  path is the best state of each site on its own, and a het call follows it or, on equality, stays.
  sites       every biallelic site of the input is phased; a site with an allele above 1 is dropped (multiallelic_dropped), as
              impute does.  A call with one allele missing counts as missing; the store keeps it as it was read.
  start       --init random (default): the order of every heterozygous call is drawn by np.random.default_rng(--init_seed);
              --init keep starts from the input's order.
  donors      --states S (default 64, even): the two columns of each sample's S / 2 nearest samples by IBS distance over the
              same sites (neighbors.pairs_device / knn_device; with --host pairs_host / knn_host: the same rows), ties to the
              lower index; a sample with fewer neighbours has -1 in the slots left.
  switching   rho from the base-pair gaps as paint forms it (paint.site_gaps, paint.switch_rates) with --switch lambda (default
              0.01) and --uniform; --theta (default paint.default_theta(S)).
  rounds      --rounds (default 10) Jacobi rounds: every sample is re-phased against the matrix of the round before, so no result
              depends on how the recipients are batched (--budget_gb).  A round that changes no allele ends the run.
  checking    --check: where every heterozygous call of the input carries phase, `switch_error` against the input's own phase is
              reported per round (the input's phase is used for nothing else, except by --init keep): over the heterozygous
              calls of a sample in site order, the share of adjacent pairs whose orientation against the truth differs, summed
              over the samples (chromosome ends are not treated apart).

Outputs: {out}_phased.zarr (genotypes.write_callset_zarr: calldata/GT, samples, variants/CHROM, POS, REF, ALT),
{out}_phase_history.txt (round ll switches_per_site changed [switch_error]), {out}_phase_summary.json.  Without a GPU the run
stops and says so; --host asks for the NumPy form in float32.  The device (loc_phase_viterbi, include/locator_hip_phase.h) takes
the same decisions bit for bit: the store is byte-identical to --host's, and the text files agree apart from the ll fields, whose
logarithms are summed differently.

Not built: sampling instead of Viterbi, donors chosen per window or by PBWT, re-estimating lambda from n_switch, recombination
maps, keeping already-phased calls fixed, writing a VCF, ploidy other than 2.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

from . import _abi
from . import baselines as B
from . import paint as PT
from ._files import write_atomic

PROG = "locator_amd.phase"
LAUNCH = "the paths are loc_phase_viterbi launches"
MAX_STATES, MIN_STATES = _abi.LOC_PHASE_MAX_STATES, _abi.LOC_PHASE_MIN_STATES
THETA_MIN, THETA_MAX = PT.THETA_MIN, PT.THETA_MAX
HEAD = ("N", "K", "P")
OWN = ("states", "rounds", "rounds_run", "init", "init_seed", "theta", "switch", "uniform", "multiallelic_dropped", "het_calls",
       "het_undecided", "singleton_hets", "changed_last_round", "switches_per_site", "ll", "switch_error_start", "switch_error")
HOST_BATCH_BYTES = 1 << 28          # back-pointers of all sites that viterbi_host keeps for one batch of recipients


# ---------------------------------------------------------------- the definition

def emission_table(theta, dtype=np.float32):
    """E [4][3][3] of the module text: genotype 0, 1, 2, missing by the donor alleles x, y = 0, 1, missing."""
    f = np.dtype(dtype).type
    th, omt, half = f(theta), f(1) - f(theta), f(0.5)
    q = np.array([[omt, th], [th, omt], [half, half]], dtype=dtype)          # q[x][a]
    E = np.ones((4, 3, 3), dtype=dtype)
    E[0] = q[:, None, 0] * q[None, :, 0]
    E[2] = q[:, None, 1] * q[None, :, 1]
    E[1] = q[:, None, 1] * q[None, :, 0] + q[:, None, 0] * q[None, :, 1]
    return E


def _check(h, rec, don, rho, theta):
    h = np.asarray(h)
    if h.ndim != 2 or h.dtype != np.int8:
        raise ValueError(f"haplotypes of shape {h.shape} and type {h.dtype}: need int8 [sites][columns]")
    if h.size and int(h.max()) > 1:
        raise ValueError(f"an allele of {int(h.max())}: the model is built for the alleles 0 and 1, negative = missing")
    H = h.shape[1] // 2 * 2
    rec, don = np.asarray(rec, dtype=np.int64), np.asarray(don, dtype=np.int64)
    if don.ndim != 2 or don.shape[0] != len(rec) or not MIN_STATES <= don.shape[1] <= MAX_STATES:
        raise ValueError(f"donors of shape {don.shape} for {len(rec)} recipients: need [recipients][{MIN_STATES} .. {MAX_STATES}]")
    if H < 2:
        raise ValueError(f"{h.shape[1]} haplotype columns: two a sample, one sample at least")
    if len(rec) and (rec.min() < 0 or rec.max() >= H // 2):
        raise ValueError(f"a recipient outside the samples 0 .. {H // 2 - 1}")
    if don.size and (don.min() < -1 or don.max() >= H):
        raise ValueError(f"a donor outside the columns 0 .. {H - 1} (-1 = none)")
    if don.size and ((don == 2 * rec[:, None]) | (don == 2 * rec[:, None] + 1)).any():
        raise ValueError("a donor that is a column of its recipient")
    rho = np.asarray(rho, dtype=np.float64)
    if rho.shape != (h.shape[0],):
        raise ValueError(f"{rho.shape} switch probabilities for {h.shape[0]} sites")
    if len(rho) > 1 and not (np.isfinite(rho[1:]).all() and rho[1:].min() >= 0 and rho[1:].max() <= 1):
        raise ValueError("a switch probability outside [0, 1]")
    if not THETA_MIN <= float(np.float32(theta)) <= THETA_MAX:
        raise ValueError(f"theta = {theta}: must be {THETA_MIN} .. {THETA_MAX}")
    return h, H, rec, don, rho


def _summary(v):
    """(R [n][S], arg [n][S], G [n], gflat [n]) of v [n][S][S]: np.argmax takes the lowest index."""
    n, S, _ = v.shape
    R, arg = v.max(axis=2), v.argmax(axis=2)
    flat = v.reshape(n, S * S).argmax(axis=1)
    return R, arg, v.reshape(n, S * S)[np.arange(n), flat], flat


def _viterbi_batch(h, rec, don, rho, theta, dtype, paths=None):
    """The module text for recipients that all have a donor.  paths: a list that receives (d1 [n][K], d2 [n][K], code [n][K])."""
    f = np.dtype(dtype).type
    K, (n, S) = h.shape[0], don.shape
    ok = don >= 0
    u = f(1) / ok.sum(axis=1).astype(dtype)
    pair = ok[:, :, None] & ok[:, None, :]
    E = emission_table(theta, dtype)
    rj = np.concatenate([[1.0], rho[1:]]).astype(dtype)
    a0, a1 = h[:, 2 * rec].astype(np.int64), h[:, 2 * rec + 1].astype(np.int64)                     # [K][n]
    g = np.where((a0 < 0) | (a1 < 0), 3, a0 + a1)
    x = np.where(ok[None], h[:, np.maximum(don, 0).reshape(-1)].reshape(K, n, S), -1).astype(np.int64)
    x = np.where(x < 0, 2, x)                                                                    # 0, 1, 2 = missing: E's index
    rows = np.arange(n)
    v = pair.astype(dtype)
    R, arg, G, gflat = _summary(v)
    code = np.empty((K, n, S, S), dtype=np.uint8)
    args, gflats = np.empty((K, n, S), dtype=np.int64), np.empty((K, n), dtype=np.int64)
    ll = np.zeros(n)
    for j in range(K):
        om = f(1) - rj[j]
        ru = rj[j] * u
        t = om + ru
        tt, tr, rr = t * t, t * ru, ru * ru
        e = np.where(pair, E[g[j][:, None, None], x[j][:, :, None], x[j][:, None, :]], f(0))
        best = tt[:, None, None] * v
        row = R[:, :, None] >= R[:, None, :]
        b = tr[:, None, None] * np.where(row, R[:, :, None], R[:, None, :])
        take = b > best
        cj = np.where(take, np.where(row, 1, 2), 0).astype(np.uint8)
        best = np.where(take, b, best)
        c = (rr * G)[:, None, None]
        take = c > best
        cj = np.where(take, np.uint8(3), cj)
        best = np.where(take, c, best)
        v = e * best
        m = v.max(axis=(1, 2))
        v = (v * (f(1) / m)[:, None, None]).astype(dtype)
        code[j], args[j], gflats[j] = cj, arg, gflat
        R, arg, G, gflat = _summary(v)
        ll += np.log(m.astype(np.float64))
    first = a0.T.astype(np.int8).copy()
    d1, d2 = gflat // S, gflat % S
    n_switch, n_tied = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    trace = (np.empty((n, K), dtype=np.int64), np.empty((n, K), dtype=np.int64), np.zeros((n, K), dtype=np.uint8))
    q = np.array([[f(1) - f(theta), f(theta)], [f(theta), f(1) - f(theta)], [f(0.5), f(0.5)]], dtype=dtype)
    for j in range(K - 1, -1, -1):
        trace[0][:, j], trace[1][:, j] = d1, d2
        xs, ys = x[j][rows, d1], x[j][rows, d2]
        p10, p01 = q[xs, 1] * q[ys, 0], q[xs, 0] * q[ys, 1]
        het = g[j] == 1
        first[:, j] = np.where(het & (p10 > p01), 1, np.where(het & (p10 < p01), 0, first[:, j]))
        n_tied += het & (p10 == p01)
        if j > 0:
            cj = code[j][rows, d1, d2]
            trace[2][:, j] = cj
            n_switch += np.where(cj == 3, 2, (cj > 0).astype(np.int64)).astype(np.int32)
            n1 = np.where(cj == 2, args[j][rows, d2], np.where(cj == 3, gflats[j] // S, d1))
            n2 = np.where(cj == 1, args[j][rows, d1], np.where(cj == 3, gflats[j] % S, d2))
            d1, d2 = n1, n2
    if paths is not None:
        paths.append(trace)
    return first, ll, n_switch, n_tied


def viterbi_host(h, rec, don, rho, theta, dtype=np.float32, paths=None):
    """(first [R][K] int8, ll [R] float64, n_switch, n_tied, n_donors [R] int32): the definition in the module text.  paths: a
    list that receives, a batch of recipients with a donor, (their rows, d1 [n][K], d2 [n][K], code [n][K]) of the traceback."""
    h, H, rec, don, rho = _check(h, rec, don, rho, theta)
    K, (R, S) = h.shape[0], don.shape
    first = np.ascontiguousarray(h[:, 2 * rec].T) if R else np.zeros((0, K), dtype=np.int8)
    ll = np.zeros(R)
    n_switch, n_tied, n_donors = (np.zeros(R, dtype=np.int32) for _ in range(3))
    if K == 0 or R == 0:
        return first, ll, n_switch, n_tied, n_donors
    n_donors[:] = (don >= 0).sum(axis=1)
    live = np.flatnonzero(n_donors > 0)
    step = max(1, HOST_BATCH_BYTES // (K * S * (S + 16)))
    for a in range(0, len(live), step):
        at = live[a:a + step]
        got = [] if paths is not None else None
        first[at], ll[at], n_switch[at], n_tied[at] = _viterbi_batch(h, rec[at], don[at], rho, theta, dtype, got)
        if paths is not None:
            paths.append((at, *got[0]))
    return first, ll, n_switch, n_tied, n_donors


# ---------------------------------------------------------------- the device form

def viterbi_device(h, rec, don, rho, theta, block=0, pitch=None, pad_fill=-1, fill=None, budget=4 << 30, device="cuda:0",
                   first_pitch=None, guard=0, report=None):
    """viterbi_host(float32)'s answer from loc_phase_viterbi launches, the recipients in batches whose scratch stays within
    `budget` bytes.  first_pitch: the row pitch of `first` on the device (default K).  Tests: fill, a 32-bit pattern that scratch
    and the outputs hold before a launch; guard, floats allocated behind the stated scratch; report, a dict that learns whether
    the pad bytes of `first` (pad_untouched) and the guard (guard_untouched) still held the pattern after every launch."""
    import torch as t
    from . import _device as D, _lib
    lib = _lib.load()
    h, H, rec, don, rho = _check(h, rec, don, rho, theta)
    K, (R, S) = h.shape[0], don.shape
    buf = B.padded(np.ascontiguousarray(h[:, :H]), pitch, pad_fill)
    fp = K if first_pitch is None else int(first_pitch)
    first = np.zeros((R, K), dtype=np.int8)
    ll = np.zeros(R)
    n_switch, n_tied, n_donors = (np.zeros(R, dtype=np.int32) for _ in range(3))
    with t.cuda.device(device):
        d_h = D.put(buf, np.int8, device)
        d_rho = D.put(rho if K else np.zeros(1), np.float32, device)
        one = int(lib.loc_phase_work_bytes(S, K, 1, int(block)))
        if one < 0:
            _lib.check(-1, "loc_phase_work_bytes")
        step = max(1, int(budget) // max(one + K, 1))
        for a in range(0, R, step):
            n = min(step, R - a)
            d_rec, d_don = D.put(rec[a:a + n], np.int32, device), D.put(don[a:a + n], np.int32, device)
            d_first = t.empty((n * max(fp, 1) + 3) // 4 * 4, dtype=t.int8, device=device)
            d_ll = t.empty(n, dtype=t.float64, device=device)
            d_ns, d_nt, d_nd = (t.empty(n, dtype=t.int32, device=device) for _ in range(3))
            work_bytes = int(lib.loc_phase_work_bytes(S, K, n, int(block)))
            d_work = t.empty(max(work_bytes // 4, 4) + int(guard), dtype=t.float32, device=device)
            D.prefill((d_work, d_first, d_ll, d_ns, d_nt, d_nd), fill)
            _lib.check(lib.loc_phase_viterbi(d_h.data_ptr(), H, K, int(buf.shape[1]), d_rec.data_ptr(), n, d_don.data_ptr(), S,
                                             d_rho.data_ptr(), float(theta), int(block), d_first.data_ptr(), max(fp, 1),
                                             d_ll.data_ptr(), d_ns.data_ptr(), d_nt.data_ptr(), d_nd.data_ptr(), d_work.data_ptr(),
                                             work_bytes, D.stream()), "loc_phase_viterbi")
            flat = d_first.cpu().numpy()
            rows = flat[:n * max(fp, 1)].reshape(n, max(fp, 1))
            first[a:a + n] = rows[:, :K]
            if fill is not None and report is not None:
                pat = np.frombuffer(np.array(fill, dtype=np.uint32).tobytes(), dtype=np.int8)
                held = pat[np.arange(len(flat)) % 4]
                report["pad_untouched"] = report.get("pad_untouched", True) and bool(
                    np.array_equal(rows[:, K:], held[:n * max(fp, 1)].reshape(n, -1)[:, K:]) and np.array_equal(flat[n * max(fp, 1):],
                                                                                                             held[n * max(fp, 1):]))
                tail = d_work[max(work_bytes // 4, 4):].cpu().numpy().view(np.uint32)
                report["guard_untouched"] = report.get("guard_untouched", True) and bool((tail == np.uint32(fill)).all())
            ll[a:a + n], n_switch[a:a + n], n_tied[a:a + n] = d_ll.cpu().numpy(), d_ns.cpu().numpy(), d_nt.cpu().numpy()
            n_donors[a:a + n] = d_nd.cpu().numpy()
            del d_work
    return first, ll, n_switch, n_tied, n_donors


# ---------------------------------------------------------------- the command's pieces

def switch_error(est, truth):
    """The switch error of the haplotype matrix est [K][2N] against truth [K][2N] (the same calls in the true order): over the
    heterozygous calls of a sample in site order, adjacent pairs whose orientation against the truth differs, over all adjacent
    pairs, summed over the samples.  NaN where no sample has two heterozygous calls."""
    est, truth = np.asarray(est), np.asarray(truth)
    t0, t1 = truth[:, 0::2], truth[:, 1::2]
    het = (t0 >= 0) & (t1 >= 0) & (t0 != t1)
    same = est[:, 0::2] == t0
    wrong = pairs = 0
    for s in range(het.shape[1]):
        o = same[het[:, s], s]
        if len(o) > 1:
            wrong += int((o[1:] != o[:-1]).sum())
            pairs += len(o) - 1
    return wrong / pairs if pairs else float("nan")


def nearest_donors(c, states, host, device="cuda:0"):
    """don int32 [N][states]: the two columns of each sample's states / 2 nearest samples by IBS distance over the counts c
    [N][K] (-1 = missing), nearest first, -1 where a sample has fewer neighbours."""
    from . import neighbors as NB
    N, k = c.shape[0], states // 2
    everyone = np.ones(N, dtype=np.uint8)
    if host:
        d, n = NB.pairs_host(c)
        nbr, _ = NB.knn_host(d, n, 2, everyone, k)
    else:
        d_d, d_n = NB.pairs_device(c, device=device, keep_on_device=True)
        nbr, _ = NB.knn_device(d_d, d_n, N, 2, everyone, k, device=device)
    nbr = np.asarray(nbr, dtype=np.int64)
    don = np.stack([2 * nbr, 2 * nbr + 1], axis=2).reshape(N, 2 * k)
    return np.where(np.repeat(nbr, 2, axis=1) < 0, -1, don).astype(np.int32)


def apply_first(hap, first):
    """hap [K][2N] with every heterozygous call ordered as first [N][K] says (allele `first` on the first copy)."""
    new = hap.copy()
    a0, a1 = hap[:, 0::2], hap[:, 1::2]
    het = (a0 >= 0) & (a1 >= 0) & (a0 != a1)
    f = np.asarray(first).T
    new[:, 0::2] = np.where(het, f, a0)
    new[:, 1::2] = np.where(het, 1 - f, a1)
    return new


def write_history(path, history, check):
    head = "round\tll\tswitches_per_site\tchanged" + ("\tswitch_error" if check else "") + "\n"
    write_atomic(path, head + "".join(f"{r}\t{l!r}\t{s!r}\t{c}" + (f"\t{e!r}" if check else "") + "\n" for r, l, s, c, e in history))


# ---------------------------------------------------------------- the command's work

def phase(gt, samples, sites, out=None, states=64, rounds=10, init="random", init_seed=0, switch=0.01, theta=None, uniform=False,
          check=False, truth_known=True, dropped=0, host=False, silence=False, device="cuda:0", budget=4 << 30, block=0):
    """The command's work for the calls gt [K][N][2] int8 of biallelic sites (sites = {chrom, pos, ref, alt}): returns the
    summary dict and writes the output files when `out` is given.  truth_known: every heterozygous call of gt carries phase."""
    from . import genotypes as G
    gt = np.ascontiguousarray(gt, dtype=np.int8)
    samples = np.asarray(samples).astype(str)
    K, N = gt.shape[0], len(samples)
    if gt.ndim != 3 or gt.shape[1] != N or gt.shape[2] != 2:
        raise SystemExit(f"{PROG}: calls of ploidy {gt.shape[2] if gt.ndim == 3 else '?'}: the copying model is built for two haplotypes "
                         "a sample")
    if K == 0:
        raise SystemExit(f"{PROG}: no site is left: nothing to phase")
    if N < 2:
        raise SystemExit(f"{PROG}: {N} sample(s): nobody to copy from")
    if states % 2 != 0 or not MIN_STATES <= states <= MAX_STATES:
        raise SystemExit(f"{PROG}: --states must be even, {MIN_STATES} .. {MAX_STATES}")
    if rounds < 1:
        raise SystemExit(f"{PROG}: --rounds must be >= 1")
    if init not in ("random", "keep"):
        raise SystemExit(f"{PROG}: --init must be `random` or `keep`")
    if not (np.isfinite(switch) and switch > 0):
        raise SystemExit(f"{PROG}: --switch must be a positive number")
    if theta is None:
        theta = PT.default_theta(states)
    if not THETA_MIN <= theta <= THETA_MAX:
        raise SystemExit(f"{PROG}: --theta must be {THETA_MIN} .. {THETA_MAX}")
    if check and not truth_known:
        raise SystemExit(f"{PROG}: --check needs an input whose heterozygous calls all carry phase (written 'a|b')")
    if not host:
        B.require_gpu(PROG, LAUNCH)
    try:
        g, first_site = PT.site_gaps(sites["chrom"], sites["pos"], K, uniform)
    except ValueError as e:
        raise SystemExit(f"{PROG}: {e}") from None
    rho = PT.switch_rates(switch, g, first_site)

    calls = gt.reshape(K, 2 * N)
    work = np.where(np.repeat((gt < 0).any(axis=2), 2, axis=1), np.int8(-1), calls)         # a half-missing call is missing
    het = (work[:, 0::2] >= 0) & (work[:, 0::2] != work[:, 1::2])
    truth = work.copy()
    if init == "random":
        swap = np.random.default_rng(init_seed).random((K, N)) < 0.5
        a0, a1 = work[:, 0::2].copy(), work[:, 1::2].copy()
        work[:, 0::2], work[:, 1::2] = np.where(het & swap, a1, a0), np.where(het & swap, a0, a1)
    c = np.ascontiguousarray(np.where(work[:, 0::2] < 0, np.int8(-1), work[:, 0::2] + work[:, 1::2]).T, dtype=np.int8)
    don = nearest_donors(c, states, host, device)
    rec = np.arange(N, dtype=np.int32)
    run = (lambda h: viterbi_host(h, rec, don, rho, theta, np.float32)) if host else \
        (lambda h: viterbi_device(h, rec, don, rho, theta, block=block, budget=budget, device=device))

    err0 = switch_error(work, truth) if check else None
    history, changed, n_tied = [], 0, np.zeros(N, dtype=np.int32)
    ll = n_switch = None
    for r in range(rounds):
        first, ll, n_switch, n_tied, _ = run(work)
        new = apply_first(work, first)
        changed = int((new != work).sum())
        work = new
        history.append((r, B.num(ll.sum()), B.num(n_switch.sum() / (N * K)), changed, switch_error(work, truth) if check else None))
        if changed == 0:
            break
    minor = np.minimum((c == 1).sum(axis=0) + 2 * (c == 2).sum(axis=0), (c == 1).sum(axis=0) + 2 * (c == 0).sum(axis=0))
    own = {"states": int(states), "rounds": int(rounds), "rounds_run": len(history), "init": init, "init_seed": int(init_seed),
           "theta": float(theta), "switch": float(switch), "uniform": bool(uniform), "multiallelic_dropped": int(dropped),
           "het_calls": int(het.sum()), "het_undecided": int(n_tied.sum()), "singleton_hets": int(het[minor == 1].sum()),
           "changed_last_round": changed, "switches_per_site": history[-1][2], "ll": history[-1][1],
           "switch_error_start": B.num(err0), "switch_error": history[-1][4] if check else None}
    summary = B.assemble_summary({"N": int(N), "K": int(K), "P": 2}, own, {}, HEAD, OWN, (), host)
    lines = [f"{N} samples, {K} sites, {own['het_calls']} heterozygous calls: {states} states, {len(history)} round(s)",
             f"theta {theta!r}, switch rate {switch!r}, {own['switches_per_site']!r} switches a site, {changed} alleles changed in the "
             f"last round, {own['het_undecided']} heterozygous calls left as they were by a tie"]
    if check:
        lines.append(f"switch error against the input's phase: {err0!r} at the start, {own['switch_error']!r} at the end")
    if out is not None:
        keep = (gt < 0).any(axis=2)                                                     # half-missing calls stay as read
        final = np.where(np.repeat(keep, 2, axis=1), calls, work).reshape(K, N, 2)
        G.write_callset_zarr(out + "_phased.zarr", final, np.asarray(sites["pos"], dtype=np.int32), samples, chrom=sites["chrom"],
                             ref=sites["ref"], alt=sites["alt"])
        write_history(out + "_phase_history.txt", history, check)
        write_atomic(out + "_phase_summary.json", json.dumps(summary, indent=1) + "\n")
    if not silence:
        for line in lines:
            print(line)
    summary["_hap"], summary["_history"], summary["_don"] = work, history, don
    return summary


# ---------------------------------------------------------------- command

def build_parser():
    p = argparse.ArgumentParser(prog=PROG, description="Haplotypes of unphased calls by diploid haplotype copying.")
    p.add_argument("--vcf", default=None, help="VCF (optionally gzipped) of the samples to phase")
    p.add_argument("--zarr", default=None, help="zarr-v2 callset with calldata/GT, samples and variants/CHROM, POS, REF, ALT")
    p.add_argument("--matrix", default=None, help="refused: the output needs the variants' CHROM, POS, REF and ALT")
    p.add_argument("--out", required=True, help="output stem")
    p.add_argument("--states", default=64, type=int, help=f"donor haplotypes of a sample: the two of each of its states / 2 nearest "
                                                          f"samples (default 64; even, {MIN_STATES} .. {MAX_STATES})")
    p.add_argument("--rounds", default=10, type=int, help="rounds at most; a round that changes nothing ends the run (default 10)")
    p.add_argument("--init", default="random", choices=("random", "keep"),
                   help="the first order of a heterozygous call: drawn (default), or the input's")
    p.add_argument("--init_seed", default=0, type=int, help="seed of the --init random draw (default 0)")
    p.add_argument("--switch", default=0.01, type=float, help="switch rate lambda a mean gap (default 0.01)")
    p.add_argument("--theta", default=None, type=float, help=f"mismatch probability, {THETA_MIN} .. {THETA_MAX} (default: Li & "
                                                             "Stephens' from --states)")
    p.add_argument("--uniform", default=False, action="store_true", help="every site one mean gap from the one before it")
    p.add_argument("--check", default=False, action="store_true",
                   help="report the switch error against the input's own phase (every heterozygous call must carry it)")
    p.add_argument("--budget_gb", default=4.0, type=float, help="device scratch of a launch at most, GiB (default 4)")
    p.add_argument("--host", default=False, action="store_true", help="the NumPy form in float32 instead of the GPU: the same store")
    p.add_argument("--gpu_number", default=None, type=str, help="the GPU to use (sets HIP_VISIBLE_DEVICES)")
    p.add_argument("--silence", default=False, action="store_true", help="no terminal output")
    return p


def main(argv=None):
    from . import impute as IM
    parser = build_parser()
    a = parser.parse_args(argv)
    if a.matrix is not None:
        raise SystemExit(f"{PROG} needs --vcf or --zarr: an allele-count --matrix has no CHROM, POS, REF and ALT to write")
    if (a.vcf is None) == (a.zarr is None):
        parser.error("exactly one of --vcf / --zarr must be given")
    B.check_budget(parser, a)
    if a.states % 2 != 0 or not MIN_STATES <= a.states <= MAX_STATES:
        parser.error(f"--states must be even, {MIN_STATES} .. {MAX_STATES}")
    if a.rounds < 1:
        parser.error("--rounds must be >= 1")
    if a.gpu_number is not None:
        for var in ("HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
            os.environ[var] = a.gpu_number
    if not a.host:
        B.require_gpu(PROG, LAUNCH)
    try:
        d = IM.read_phased(a.vcf if a.zarr is None else a.zarr, a.zarr is not None, prog=PROG, refuse=False)
        unphased = d.pop("unphased_hets")
        d, dropped = IM.biallelic(d)
        phase(d["gt"], d["samples"], d, a.out, a.states, a.rounds, a.init, a.init_seed, a.switch, a.theta, a.uniform, a.check,
              not unphased, dropped, a.host, a.silence, budget=int(a.budget_gb * (1 << 30)))
    except ValueError as e:
        raise SystemExit(f"{PROG}: {e}") from None
    return 0


if __name__ == "__main__":
    sys.exit(main())
