"""Inputs shared by tests/test_ld.py and tests/test_gpu_ld.py: site-major counts with missing calls and planted LD (the golden
VCF has no missing call and cannot exercise the mask plane), and a VCF of them on two chromosomes."""
import numpy as np

from tests.neighbors_util import GOLDEN, SAMPLE_DATA, VCF  # noqa: F401  (re-exported)


def site_counts(K, N, seed, P=2, missing=0.15, linked=0.6, flips=0.04):
    """int8 [K][N] counts 0 .. P, -1 = missing.  Every site has its own allele frequency and its own missing rate; a `linked`
    share of the sites is a copy of the site 1 .. 5 places before it with a `flips` share of its entries redrawn, so that runs
    of sites are in LD of every strength, over more than one lag and across tile edges."""
    rng = np.random.default_rng(seed)
    freq = rng.uniform(0.05, 0.95, (K, 1))
    ct = rng.binomial(P, np.broadcast_to(freq, (K, N))).astype(np.int8)
    for v in range(1, K):
        if rng.random() < linked:
            src = v - int(rng.integers(1, min(v, 5) + 1))
            redraw = rng.random(N) < flips
            ct[v] = np.where(redraw, ct[v], ct[src])
    rate = rng.uniform(0.0, missing, (K, 1))
    ct[rng.random((K, N)) < rate] = -1
    return ct


def brute(ct, W, reach):
    """sums [K][W][6] by Python loops over pairs and NumPy sums over the shared samples: nothing shared with ld.sums_host but
    the definition.  reach as the kernel clamps it."""
    ct = np.asarray(ct, dtype=np.int64)
    K = len(ct)
    out = np.zeros((K, W, 6), dtype=np.int64)
    for i in range(K):
        for lag in range(int(reach[i])):
            a, b = ct[i], ct[i + 1 + lag]
            ok = (a >= 0) & (b >= 0)
            a, b = a[ok], b[ok]
            out[i, lag] = [ok.sum(), a.sum(), b.sum(), (a * b).sum(), (a * a).sum(), (b * b).sum()]
    return out


def greedy_bitwise(flags, reach):
    """The greedy walk bit by bit on bool flags [K][W]: the plain restatement of ld.greedy_host."""
    K = len(flags)
    kept = np.ones(K, dtype=bool)
    removed_by = np.full(K, -1, dtype=np.int64)
    for i in range(K):
        if not kept[i]:
            continue
        for lag in range(int(reach[i])):
            j = i + 1 + lag
            if flags[i, lag] and kept[j]:
                kept[j] = False
                removed_by[j] = i
    return kept, removed_by


def write_vcf(path, ct, chrom, pos, samples, P=2):
    """A plain-text VCF of site-major counts: count 1 -> 0/1, 2 -> 1/1, missing -> ./. (haploid: 0, 1, .)."""
    call = {2: {-1: "./.", 0: "0/0", 1: "0/1", 2: "1/1"}, 1: {-1: ".", 0: "0", 1: "1"}}[P]
    with open(path, "w") as fh:
        fh.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(samples) + "\n")
        for v in range(len(ct)):
            fh.write(f"{chrom[v]}\t{pos[v]}\t.\tA\tT\t.\tPASS\t.\tGT\t" + "\t".join(call[int(c)] for c in ct[v]) + "\n")
    return str(path)


def planted_vcf(path, K=700, N=90, seed=5):
    """A two-chromosome VCF with missing calls and planted LD for the samples msp_0 .. of the golden sample table; returns
    (path, ct, chrom, pos)."""
    ct = site_counts(K, N, seed)
    rng = np.random.default_rng(seed + 1)
    cut = K // 2 + 13                                      # the chromosome break: inside a tile
    chrom = np.array(["chr1"] * cut + ["chr2"] * (K - cut), dtype=object)
    pos = np.concatenate([np.cumsum(rng.integers(1, 400, cut)), np.cumsum(rng.integers(1, 400, K - cut))])
    return write_vcf(path, ct, chrom, pos, [f"msp_{i}" for i in range(N)]), ct, chrom, pos
