"""Inputs shared by tests/test_neighbors.py and tests/test_gpu_neighbors.py."""
import gzip
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VCF = os.path.join(GOLDEN, "test_genotypes.vcf.gz")
SAMPLE_DATA = os.path.join(GOLDEN, "test_sample_data.txt")


def counts(N, K, seed, P=2, missing=0.3):
    """int8 [N][K] counts 0 .. P with -1 = missing.  Every row has its own allele frequency and its own missing rate, so
    d and n differ from row to row and from their transposes' neighbours: a transposed or mis-tiled write cannot pass."""
    rng = np.random.default_rng(seed)
    freq = rng.uniform(0.05, 0.95, (N, 1))
    rate = rng.uniform(0.0, missing, (N, 1))
    c = rng.binomial(P, np.broadcast_to(freq, (N, K))).astype(np.int8)
    c[rng.random((N, K)) < rate] = -1
    return c


def pair_tables(N, seed, empty=0.15):
    """Symmetric int32 d, n [N][N] with few distinct values: many exact ties of D = d / (P n) between different (d, n)
    (1 / 4 = 2 / 8), and n = 0 (D is NaN) for a share of the pairs."""
    rng = np.random.default_rng(seed)
    n = rng.choice(np.array([4, 8, 12], dtype=np.int32), (N, N))
    n[rng.random((N, N)) < empty] = 0
    d = rng.integers(0, 7, (N, N), dtype=np.int32)
    iu = np.triu_indices(N, 1)
    d.T[iu], n.T[iu] = d[iu], n[iu]
    d = np.minimum(d, 2 * n)
    np.fill_diagonal(d, 0)
    return np.ascontiguousarray(d), np.ascontiguousarray(n)


def write_vcf_cut(path, n_samples, n_variants):
    """The first n_variants records and n_samples samples of the golden VCF, as a plain-text VCF."""
    kept = 0
    with gzip.open(VCF, "rt") as src, open(path, "w") as dst:
        for line in src:
            if line.startswith("##"):
                dst.write(line)
                continue
            if not line.startswith("#"):
                if kept == n_variants:
                    break
                kept += 1
            dst.write("\t".join(line.rstrip("\n").split("\t")[:9 + n_samples]) + "\n")
    return path
