"""Fixtures of the --dosage tests, built at test time from tests/golden/test_genotypes.vcf.gz: DS = the GT count plus seeded
noise, clipped to [0, 2], written as a VCF (DS and GP at chosen FORMAT positions) or a zarr store with calldata/DS."""
import gzip
import os

import numpy as np

from locator_amd import genotypes as G

GOLD = os.path.join(os.path.dirname(__file__), "golden")
VCF = os.path.join(GOLD, "test_genotypes.vcf.gz")
SAMPLES = os.path.join(GOLD, "test_sample_data.txt")


def golden_counts():
    """(GT allele-1 counts float32 (variants, samples) with NaN where a call is missing, samples, POS)."""
    v = G.read_vcf(VCF)
    gt = v["calldata/GT"]
    c = (gt == 1).sum(axis=2).astype(np.float32)
    c[(gt < 0).any(axis=2)] = np.nan
    return c, v["samples"], v["variants/POS"]


def clean_biallelic(gt):
    """Sites whose calls are all 0 / 1 alleles with none missing: there the GT filter and the dosage filter on the GT count
    see the same thing (a third allele or a half-missing call makes the two differ by design)."""
    return np.flatnonzero(((gt == 0) | (gt == 1)).all(axis=(1, 2)))


def write_gt_vcf(path, gt, samples, pos):
    """Phased GT-only VCF of int8 calls (variants, samples, 2) with alleles 0 / 1."""
    opener = gzip.open if str(path).endswith(".gz") else open
    with opener(path, "wt") as fh:
        fh.write("##fileformat=VCFv4.2\n")
        fh.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(map(str, samples)) + "\n")
        for v in range(gt.shape[0]):
            fh.write(f"1\t{pos[v]}\t.\tA\tT\t.\tPASS\t.\tGT\t" + "\t".join(f"{a}|{b}" for a, b in gt[v]) + "\n")


def noisy_dosage(counts, sd=0.08, seed=7, missing=0.0):
    """counts + N(0, sd) clipped to [0, 2] (NaN stays NaN), rounded to 4 decimals as a VCF writer prints them; a fraction
    `missing` of the values set to NaN."""
    rng = np.random.default_rng(seed)
    d = np.clip(counts + rng.normal(0, sd, counts.shape), 0, 2).round(4).astype(np.float32)
    if missing:
        d[rng.random(d.shape) < missing] = np.nan
    return d


def _fmt(x):
    return "." if np.isnan(x) else f"{float(x):.4f}".rstrip("0").rstrip(".")


def write_dosage_vcf(path, ds, samples, pos, field="DS", gt=True, alts=None):
    """A VCF whose records hold `field` (DS, or GP from the dosage d as (max(0, 1 - d), ..)) after GT:DP when gt=True, or
    alone.  GP is written as P(0) = 1 - p1 - p2, P(1) = p1, P(2) = p2 with d = p1 + 2 p2: p2 = max(0, d - 1), p1 = d - 2 p2."""
    opener = gzip.open if str(path).endswith(".gz") else open
    with opener(path, "wt") as fh:
        fh.write("##fileformat=VCFv4.2\n")
        fh.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(map(str, samples)) + "\n")
        for v in range(ds.shape[0]):
            if field == "DS":
                vals = [_fmt(x) for x in ds[v]]
            else:
                vals = []
                for x in ds[v]:
                    if np.isnan(x):
                        vals.append(".")
                        continue
                    p2 = max(0.0, float(x) - 1.0)
                    p1 = float(x) - 2 * p2
                    vals.append(f"{1 - p1 - p2:.6f},{p1:.6f},{p2:.6f}")
            fmt = f"GT:DP:{field}" if gt else field
            cells = [f"0/1:7:{x}" if gt else x for x in vals]
            alt = "T" if alts is None else alts[v]
            fh.write(f"1\t{pos[v]}\t.\tA\t{alt}\t.\tPASS\t.\t{fmt}\t" + "\t".join(cells) + "\n")


def write_dosage_zarr(path, ds, samples, pos, chunk_variants=4096, with_gt=True):
    """A callset store (calldata/GT from the rounded dosages, variants/POS, samples) plus calldata/DS float32."""
    q = np.nan_to_num(np.rint(ds), nan=-1).astype(np.int8)
    gt = np.stack([np.where(q < 0, -1, (q >= 1).astype(np.int8)), np.where(q < 0, -1, (q >= 2).astype(np.int8))], axis=2)
    G.write_callset_zarr(path, gt.astype(np.int8), pos, samples, chunk_variants=chunk_variants)
    if not with_gt:
        import shutil
        shutil.rmtree(os.path.join(path, "calldata", "GT"))
    G.write_dosage_zarr(path, ds, chunk_variants=chunk_variants)
