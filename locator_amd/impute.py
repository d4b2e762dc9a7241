#!/usr/bin/env python3
"""`python -m locator_amd.impute`: allele dosages of missing and untyped calls from the haplotype copying model of the paint
command (locator_amd/paint.py: Li & Stephens 2003).  A recipient's missing allele has emission 1, so the posterior over its
donors at that site is the imputation: the dose is the posterior weight of the donors that hold allele 1 over that of the donors
that hold any allele.  The output is a callset store with calldata/DS that `locator --zarr ... --dosage` and `predict --zarr ...
--dosage` read.

  python -m locator_amd.impute --vcf phased.vcf.gz --out out/test                        fill: every missing allele from everyone else
  python -m locator_amd.impute --vcf array.vcf.gz --panel panel.vcf.gz --out out/test    panel: the panel's sites for the targets

  model       `dose_host(h, donor, owner, rec, rho, theta, dtype)` -> (dose [R][K], ll [R] float64, n_donors [R] int32), every
              operation in `dtype`.  The inputs, their checks, the donors of a recipient, u, e_j, the forward pass, ll, t, T, g
              and b_(j-1) are paint.copy_host's (its module text).  In the backward walk at site j, in place of share / chunks:
                A1 = sum_d of g where h[j][d] == 1, A0 = sum_d of g where h[j][d] == 0 (a negative allele adds +0 to both),
                S = A0 + A1, dose[i][j] = min(A1 (1 / S), 1) where S is a normal number at least, else NaN.
              The normalisation 1 / G of gamma cancels.  NaN: no donor of the recipient holds an allele at the site (or, over a
              long stretch without a switch in float32, the sums underflowed).  A recipient with D = 0 gets a row of NaN, ll = 0,
              n_donors = 0.  K = 0 or R = 0: empty doses, zeros.
  input       phased calls of ploidy 2 with CHROM / POS / REF / ALT: --vcf or --zarr (a --matrix carries no phase; a heterozygous
              call without phase is refused as paint refuses it).  Sites with an allele above 1 are dropped
              (multiallelic_dropped).  There is no --min_mac filter: the fit applies its own.
  fill        without --panel.  The donors are all haplotypes (--max_donors M: those of every ceil(n / M)-th sample), nobody
              copies from their own individual, the recipients are the haplotypes with a missing allele.
  panel       --panel (a VCF, or a zarr store when the path is a directory).  The donors are the panel's haplotypes (--max_donors
              thins them), the recipients all target haplotypes; a target sample whose ID is in the panel is refused.  A target
              site is a panel site with the same CHROM, POS, REF and first ALT; with REF and ALT exchanged it matches with its
              alleles flipped (swapped); a target site without a panel site is dropped (target_unmatched; a second target site of
              a panel site too).  The output sites are the panel's in panel order, typed (matched) or untyped (all missing).
  switching   rho, --switch, --em_rounds, --em_sample, --uniform and --theta as in paint (paint.estimate_switch: rounds of
              loc_paint_copy with evenly spaced recipient samples); in panel mode the rounds' recipients are target samples.
  output      {out}_imputed.zarr: samples, variants/CHROM, POS, REF, ALT, calldata/GT and calldata/DS float32 (variants, samples).
              DS = v0 + v1 summed in float32, v_a the observed allele where there is one, else the haplotype's dose; NaN stays
              NaN, which --dosage reads as missing.  calldata/GT holds the input calls; with --fill_calls a missing allele that has
              a dose becomes dose >= 0.5.  {out}_impute_summary.json, {out}_impute_history.txt (round switch ll).
  checking    --check_mask F (with --seed): every observed allele of a candidate recipient (fill: every haplotype; panel: every
              target haplotype, at the typed sites) is hidden with probability F by np.random.default_rng(seed) and imputed; only
              the summary is written, and it gains masked and, over the hidden alleles that have a dose and a frequency, mse,
              concordance (dose >= 0.5 against the allele), r2 and the same three of the donors' allele-1 frequency at the site
              over the donors with an allele (*_frequency).  The counts of missing alleles are then those of the masked input.

Without a GPU the run stops and says so; --host asks for the NumPy form in float64 (--host_dtype float32: the yardstick of the
device's round-off).  The device computes in fp32 (loc_impute_dose, include/locator_hip_impute.h): the stores of the two paths
agree within round-off; each path is deterministic.  --budget_gb bounds the scratch and the dose rows of one launch (the
recipients go in batches, which changes no bit).

Not built: recombination maps, per-population donor pools (the posterior per window and label: `python -m
locator_amd.ancestry`), ploidy other than 2, writing a VCF.  Unphased calls are phased by
`python -m locator_amd.phase` first.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

from . import baselines as B
from . import paint as PT
from ._files import write_atomic

PROG = "locator_amd.impute"
LAUNCH = "the recursions are loc_impute_dose and loc_paint_copy launches"
MAX_HAPS = PT.MAX_HAPS
SUMMARY = ("mode", "N", "K", "H", "n_donor_haps", "groups", "recipients", "multiallelic_dropped", "typed", "untyped", "swapped",
           "target_unmatched", "missing_alleles", "imputed_alleles", "without_dose", "theta", "switch", "uniform", "em_rounds", "ll")
CHECKED = ("masked", "scored", "mse", "concordance", "r2", "mse_frequency", "concordance_frequency", "r2_frequency")


# ---------------------------------------------------------------- the definition

def _dose_batch(h, dn, rcols, rho, theta, dtype):
    f = np.dtype(dtype).type
    K, (R, H) = h.shape[0], dn.shape
    u, rj, ah_all, _, ll = PT.forward_batch(h, dn, rcols, rho, theta, dtype)
    b = np.broadcast_to(u, (R, H)).astype(dtype)
    dose = np.empty((R, K), dtype=dtype)
    tiny = np.finfo(dtype).tiny
    for j in range(K - 1, -1, -1):
        t = PT.emissions(h, j, rcols, dn, theta, dtype) * b
        g = ah_all[j] * b
        x = h[j, :H][None, :]
        A1 = np.where(x == 1, g, f(0)).sum(axis=1, dtype=dtype)
        A0 = np.where(x == 0, g, f(0)).sum(axis=1, dtype=dtype)
        S, T = A0 + A1, t.sum(axis=1, dtype=dtype)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            dose[:, j] = np.where(S >= tiny, np.minimum(A1 * (f(1) / S), f(1)), f(np.nan))
        b = ((f(1) - rj[j]) * (f(1) / T))[:, None] * t + rj[j] * u
    return dose, ll


def dose_host(h, donor, owner, rec, rho, theta, dtype=np.float64):
    """(dose [R][K] dtype, ll [R] float64, n_donors [R] int32): the definition in the module text."""
    return PT._host_model(_dose_batch, (("K", dtype, np.nan),), h, donor, owner, rec, rho, theta, dtype)


# ---------------------------------------------------------------- the device form

def dose_device(h, donor, owner, rec, rho, theta, block=0, pitch=None, pad_fill=-1, fill=None, budget=4 << 30, device="cuda:0"):
    """dose_host's answer from loc_impute_dose launches (dose float32), the recipients in batches whose scratch and dose rows
    stay within `budget` bytes.  fill: a 32-bit pattern that scratch and the outputs hold before a launch (tests)."""
    return PT._device_model("loc_impute_dose", (("K", np.float32, np.nan),), 4, h, donor, owner, rec, rho, theta, block, pitch, pad_fill,
                            fill, budget, device)


# ---------------------------------------------------------------- the command's pieces

def read_phased(path, zarr, prog=PROG, refuse=True):
    """{gt (V, N, P) int8, samples, chrom, pos, ref, alt (the first ALT)} of a phased VCF (zarr False) or zarr store, after the
    refusal of heterozygous calls without phase and of a store without the variants' tables.  refuse False (the phase command,
    under its own name `prog`): such calls are counted into the entry unphased_hets instead (0: none is known of)."""
    from . import genotypes as G
    if zarr:
        callset = G.open_group(path, mode="r")
        unphased = G.zarr_unphased_hets(callset)
        if refuse:
            B.refuse_unphased(unphased, f"{path}: calldata/GT_phased", prog)
        try:
            d = G.zarr_sites(callset)
        except KeyError as e:
            raise SystemExit(f"{prog}: {path} lacks {e.args[0]}: sites are identified by CHROM, POS, REF and ALT") from None
        d["calldata/GT"], d["samples"] = np.asarray(callset["calldata/GT"][:], dtype=np.int8), np.asarray(callset["samples"][:])
    else:
        d = G.read_vcf(path, phase=True, sites=True)
        unphased = d["unphased_hets"]
        if refuse:
            B.refuse_unphased(unphased, path, prog)
    gt = np.asarray(d["calldata/GT"], dtype=np.int8)
    if gt.ndim != 3 or gt.shape[2] != 2:
        raise SystemExit(f"{prog}: {path}: calls of ploidy {gt.shape[2] if gt.ndim == 3 else '?'}: the copying model is built for two "
                         "haplotypes a sample")
    tables = {"gt": gt, "samples": np.asarray(d["samples"]).astype(str), **G.site_columns(d)}
    return tables if refuse else {**tables, "unphased_hets": int(unphased or 0)}


def biallelic(d):
    """(d with the sites that hold an allele above 1 dropped, their number)."""
    multi = (d["gt"] > 1).any(axis=(1, 2))
    keep = ~multi
    return {k: (v if k == "samples" else v[keep]) for k, v in d.items()}, int(multi.sum())


def match_panel(panel, target):
    """The target's alleles at the panel's sites: (hap int8 [K][2 Nt] with -1 where the panel site is untyped, counts).  A target
    site matches the panel site of its (CHROM, POS, REF, ALT); with REF and ALT exchanged it matches flipped."""
    index = {}
    for i, key in enumerate(zip(panel["chrom"], panel["pos"].tolist(), panel["ref"], panel["alt"])):
        index.setdefault(key, i)
    K, Nt = len(panel["pos"]), len(target["samples"])
    hap = np.full((K, 2 * Nt), -1, dtype=np.int8)
    taken = np.zeros(K, dtype=bool)
    swapped = unmatched = 0
    calls = np.where(target["gt"] < 0, np.int8(-1), target["gt"]).reshape(len(target["pos"]), 2 * Nt)
    for v, (c, p, r, a) in enumerate(zip(target["chrom"], target["pos"].tolist(), target["ref"], target["alt"])):
        i, flip = index.get((c, p, r, a)), False
        if i is None:
            i, flip = index.get((c, p, a, r)), True
        if i is None or taken[i]:
            unmatched += 1
            continue
        taken[i] = True
        swapped += int(flip)
        hap[i] = np.where(calls[v] < 0, np.int8(-1), 1 - calls[v]) if flip else calls[v]
    return hap, {"typed": int(taken.sum()), "untyped": int(K - taken.sum()), "swapped": swapped, "target_unmatched": unmatched}


def run_model(dose, hap, donor_samples, want, rho, theta, max_haps=MAX_HAPS):
    """The model over paint's launch groups for the haplotype columns flagged in want [2 M]: (their columns ascending, dose
    [R][K], ll [R], n_donors [R], number of groups).  dose: dose_host or dose_device with the leading six arguments."""
    M = hap.shape[1] // 2
    n_groups, cols_of, parts = 0, [], []
    for n_groups, (_, _, hcols, donor, owner, rec) in enumerate(PT.group_columns(M, donor_samples, max_haps), 1):
        rec = rec[want[hcols[rec]]]
        if not len(rec):
            continue
        parts.append(dose(np.ascontiguousarray(hap[:, hcols]), donor, owner, rec.astype(np.int32), rho, theta))
        cols_of.append(hcols[rec])
    if not parts:
        return np.zeros(0, dtype=np.int64), np.zeros((0, hap.shape[0]), dtype=np.float32), np.zeros(0), np.zeros(0, dtype=np.int32), n_groups
    cols = np.concatenate(cols_of)
    order = np.argsort(cols, kind="stable")
    d, ll, nd = (np.concatenate([p[i] for p in parts])[order] for i in range(3))
    return cols[order], d, ll, nd, n_groups


def donor_frequency(hap, donor_cols):
    """The donors' allele-1 frequency of every site over the donors that hold an allele (NaN where none does)."""
    x = hap[:, donor_cols]
    with np.errstate(invalid="ignore", divide="ignore"):
        return (x == 1).sum(axis=1) / (x >= 0).sum(axis=1)


def scores(value, truth):
    """(mse, concordance of value >= 0.5, r2) of values against the 0 / 1 alleles they stand for."""
    value, truth = np.asarray(value, dtype=np.float64), np.asarray(truth, dtype=np.float64)
    if not len(truth):
        return None, None, None
    return B.num(((value - truth) ** 2).mean()), B.num(((value >= 0.5) == (truth == 1)).mean()), B.num(B.r2(value, truth))


# ---------------------------------------------------------------- the command's work

def impute(hap, donors, candidates, samples, sites, out=None, counts=None, mode="fill", switch=0.01, em_rounds=3, em_sample=256,
           theta=None, uniform=False, max_haps=MAX_HAPS, fill_calls=False, check_mask=None, seed=None, host=False, silence=False,
           device="cuda:0", budget=4 << 30, dtype=np.float64):
    """The command's work for a site-major haplotype matrix hap [K][2 M] (column 2 s + a: allele a of sample s): the donor
    samples `donors`, the samples whose haplotypes may be recipients `candidates` (the output's samples, IDs `samples`), sites =
    {chrom, pos, ref, alt} of the K sites.  Returns the summary dict and writes the output files when `out` is given."""
    from . import genotypes as G
    hap = np.ascontiguousarray(hap, dtype=np.int8)
    hap[hap < 0] = -1
    K, M = hap.shape[0], hap.shape[1] // 2
    donors, candidates = np.asarray(donors, dtype=np.int64), np.asarray(candidates, dtype=np.int64)
    if K == 0:
        raise SystemExit(f"{PROG}: no site is left: nothing to impute")
    theta = PT.checked_options(PROG, switch, em_rounds, em_sample, theta, 2 * len(donors))
    if not host:
        B.require_gpu(PROG, LAUNCH)
    copy = PT.model_form(PT.copy_host, PT.copy_device, host, dtype, budget, device)
    dose = PT.model_form(dose_host, dose_device, host, dtype, budget, device)
    try:
        g, first = PT.site_gaps(sites["chrom"], sites["pos"], K, uniform)
    except ValueError as e:
        raise SystemExit(f"{PROG}: {e}") from None

    ccols = PT.hap_cols(candidates)
    truth = None
    if check_mask is not None:
        hidden = (np.random.default_rng(seed).random((K, len(ccols))) < check_mask) & (hap[:, ccols] >= 0)
        truth = hap[:, ccols].copy()
        seen = hap[:, ccols]
        seen[hidden] = -1
        hap[:, ccols] = seen
    want = np.zeros(2 * M, dtype=bool)
    want[ccols] = (hap[:, ccols] < 0).any(axis=0)

    lam, history, _ = PT.estimate_switch(copy, hap, donors, g, first, switch, em_rounds, em_sample, theta, max_haps, pool=candidates)
    rho = PT.switch_rates(lam, g, first)
    cols, d, ll, nd, n_groups = run_model(dose, hap, donors, want, rho, theta, max_haps)
    doses = np.full((len(ccols), K), np.nan, dtype=np.float32)          # a row a candidate haplotype, in the output's order
    doses[np.searchsorted(ccols, cols)] = d
    calls = hap[:, ccols]
    missing = calls < 0
    has = missing & np.isfinite(doses.T)
    summary = {"mode": mode, "N": int(len(candidates)), "K": int(K), "H": int(2 * M), "n_donor_haps": int(2 * len(donors)),
               "groups": int(n_groups), "recipients": int(len(cols)), "multiallelic_dropped": 0, "typed": int(K), "untyped": 0,
               "swapped": 0, "target_unmatched": 0, **(counts or {}), "missing_alleles": int(missing.sum()),
               "imputed_alleles": int(has.sum()), "without_dose": int(missing.sum() - has.sum()), "theta": float(theta),
               "switch": float(lam), "uniform": bool(uniform), "em_rounds": int(em_rounds), "ll": B.num(ll.sum())}
    summary = {key: summary[key] for key in SUMMARY}
    lines = [f"{len(candidates)} samples, {K} sites: {len(cols)} haplotypes copy from {2 * len(donors)} donor haplotypes in {n_groups} "
             f"launch group(s)", f"theta {theta!r}, switch rate {lam!r} after {em_rounds} rounds, ll {summary['ll']!r}",
             f"{summary['imputed_alleles']} of {summary['missing_alleles']} missing alleles have a dose"]
    if truth is not None:
        freq = np.broadcast_to(donor_frequency(hap, PT.hap_cols(donors))[:, None], truth.shape)
        at = hidden & np.isfinite(doses.T) & np.isfinite(freq)
        model, base = scores(doses.T[at], truth[at]), scores(freq[at], truth[at])
        summary.update(dict(zip(CHECKED, (int(hidden.sum()), int(at.sum()), *model, *base))))
        lines.append(f"{int(hidden.sum())} alleles hidden: mse {model[0]!r} (the donors' frequency {base[0]!r}), concordance {model[1]!r} "
                     f"({base[1]!r})")
    summary["path"] = "host" if host else "device"
    if out is not None:
        if truth is None:
            v = np.where(missing, doses.T, calls.astype(np.float32)).astype(np.float32)
            ds = v[:, 0::2] + v[:, 1::2]
            gt = np.where(has & (doses.T >= 0.5), np.int8(1), np.where(has, np.int8(0), calls)) if fill_calls else calls
            store = out + "_imputed.zarr"
            G.write_callset_zarr(store, gt.reshape(K, len(candidates), 2), np.asarray(sites["pos"], dtype=np.int32), samples,
                                 chrom=sites["chrom"], ref=sites["ref"], alt=sites["alt"])
            G.write_dosage_zarr(store, ds)
        PT.write_history(out + "_impute_history.txt", history)
        write_atomic(out + "_impute_summary.json", json.dumps(summary, indent=1) + "\n")
    if not silence:
        for line in lines:
            print(line)
    summary["_doses"], summary["_history"], summary["_ll"] = doses, history, ll
    return summary


# ---------------------------------------------------------------- command

def build_parser():
    p = argparse.ArgumentParser(prog=PROG, description="Allele dosages of missing and untyped calls by haplotype copying.")
    p.add_argument("--vcf", default=None, help="phased VCF (optionally gzipped) of the samples to impute")
    p.add_argument("--zarr", default=None, help="phased zarr-v2 callset with calldata/GT, samples and variants/CHROM, POS, REF, ALT")
    p.add_argument("--matrix", default=None, help="refused: an allele-count matrix carries no phase")
    p.add_argument("--panel", default=None, help="phased reference panel, a VCF or a zarr store (a directory): impute its sites "
                                                 "for the samples of --vcf / --zarr.  Without it the missing alleles are filled")
    p.add_argument("--out", required=True, help="output stem")
    PT.add_model_arguments(p)
    p.add_argument("--fill_calls", default=False, action="store_true",
                   help="calldata/GT: every missing allele that has a dose becomes dose >= 0.5 (default: the input calls)")
    p.add_argument("--check_mask", default=None, type=float, metavar="F",
                   help="check run: hide every observed allele with probability F, impute it and report the errors; writes the summary only")
    p.add_argument("--seed", default=None, type=int, help="seed of the --check_mask draw")
    PT.add_path_arguments(p, "device scratch and dose rows of a launch at most, GiB (default 4)",
                          "the NumPy form in float64 instead of the GPU")
    p.add_argument("--gpu_number", default=None, type=str, help="the GPU to use (sets HIP_VISIBLE_DEVICES)")
    p.add_argument("--silence", default=False, action="store_true", help="no terminal output")
    return p


def main(argv=None):
    parser = build_parser()
    a = parser.parse_args(argv)
    if a.matrix is not None:
        raise SystemExit(f"{PROG} needs --vcf or --zarr: an allele-count --matrix carries no phase")
    if (a.vcf is None) == (a.zarr is None):
        parser.error("exactly one of --vcf / --zarr must be given")
    B.check_budget(parser, a)
    if a.check_mask is not None and not 0 < a.check_mask < 1:
        parser.error("--check_mask must be above 0 and below 1")
    if not 2 <= a.max_haps <= MAX_HAPS:
        parser.error(f"--max_haps must be 2 .. {MAX_HAPS}")
    if a.max_donors is not None and a.max_donors < 1:
        parser.error("--max_donors must be >= 1")
    if a.gpu_number is not None:
        for var in ("HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
            os.environ[var] = a.gpu_number
    if not a.host:
        B.require_gpu(PROG, LAUNCH)
    try:
        target, dropped = biallelic(read_phased(a.vcf if a.zarr is None else a.zarr, a.zarr is not None))
    except ValueError as e:
        raise SystemExit(f"{PROG}: {e}") from None
    Nt = len(target["samples"])
    thin = lambda n: np.arange(n) if a.max_donors is None else np.arange(n)[::-(-n // a.max_donors)]
    if a.panel is None:
        mode, sites, counts = "fill", target, {"multiallelic_dropped": dropped}
        hap = target["gt"].reshape(len(target["pos"]), 2 * Nt)
        donors, candidates = thin(Nt), np.arange(Nt)
        room = 2 * len(donors) + (2 if len(donors) < Nt else 0)
    else:
        try:
            panel, more = biallelic(read_phased(a.panel, os.path.isdir(a.panel)))
        except ValueError as e:
            raise SystemExit(f"{PROG}: {e}") from None
        shared = sorted(set(target["samples"]) & set(panel["samples"]))
        if shared:
            raise SystemExit(f"{PROG}: {len(shared)} sample(s) of the input are in the panel too (first: {shared[0]}): a sample would "
                             "copy from itself")
        mode, sites = "panel", panel
        theirs, counts = match_panel(panel, target)
        counts["multiallelic_dropped"] = dropped + more
        donors = thin(len(panel["samples"]))
        pcols = PT.hap_cols(donors)
        hap = np.concatenate([panel["gt"].reshape(len(panel["pos"]), -1)[:, pcols], theirs], axis=1)
        donors, candidates = np.arange(len(donors)), len(donors) + np.arange(Nt)
        room = 2 * len(donors) + 2
    if Nt < 1 or len(donors) < 1 or (a.panel is None and Nt < 2):
        raise SystemExit(f"{PROG}: {Nt} samples and {len(donors)} donor samples: nobody to copy from")
    PT.check_room(PROG, room, len(donors), a.max_haps, "sample")
    try:
        impute(hap, donors, candidates, target["samples"], sites, a.out, counts, mode, a.switch, a.em_rounds, a.em_sample, a.theta,
               a.uniform, a.max_haps, a.fill_calls, a.check_mask, a.seed, a.host, a.silence, budget=int(a.budget_gb * (1 << 30)),
               dtype=np.dtype(a.host_dtype).type)
    except ValueError as e:
        raise SystemExit(f"{PROG}: {e}") from None
    return 0


if __name__ == "__main__":
    sys.exit(main())
