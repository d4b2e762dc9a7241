"""Inputs and bounds shared by tests/test_pca.py and tests/test_gpu_pca.py."""
import numpy as np

from tests import neighbors_util as NU

VCF, SAMPLE_DATA = NU.VCF, NU.SAMPLE_DATA
U24 = 2.0 ** -24                                   # the unit roundoff of fp32


def exact_case(N, K, seed, P=2, missing=0.3):
    """(c, mean, scale) on which fp32 arithmetic is exact: counts as neighbors_util.counts (every row its own frequency and
    missing rate: a transposed or mis-tiled write cannot pass), mean in {0, 1}, scale in {0, 0.5, 1, 2} per site.  Then
    c - mean is in {-1 .. 2}, z a multiple of 1/2 in -2 .. 4, every product a multiple of 1/4 of magnitude <= 16, and every
    partial sum over K <= 1000 sites a multiple of 1/4 below 2^14: all exactly representable, whatever the order."""
    c = NU.counts(N, K, seed, P=P, missing=missing)
    rng = np.random.default_rng(seed + 1000)
    mean = rng.integers(0, 2, K).astype(np.float32)
    scale = rng.choice(np.array([0.0, 0.5, 1.0, 2.0], dtype=np.float32), K)
    return c, mean, scale


def spread_counts(N, K, seed, missing=0.05, P=2):
    """Counts with the sites' allele frequencies spread over 0.05 .. 0.95 and `missing` of the calls missing."""
    rng = np.random.default_rng(seed)
    freq = rng.uniform(0.05, 0.95, (1, K))
    c = rng.binomial(P, np.broadcast_to(freq, (N, K))).astype(np.int8)
    c[rng.random((N, K)) < missing] = -1
    return c


def abs_products(c, mean, scale, other=None):
    """sum_k |z_ik| |z_jk| in float64 [N][N]; with `other` [N][npc]: sum_i |z_ik| |other_ip|, [K][npc]."""
    from locator_amd import pca as P
    az = np.abs(P.z_host(c, mean, scale))
    return az @ az.T if other is None else az.T @ np.abs(np.asarray(other, dtype=np.float64))


def grm_bound(c, mean, scale):
    """The element bound of an fp32 G: z carries 2 u (a correctly rounded subtraction and product), a K-term fp32 sum in
    any order adds gamma_K: (K + 8) u sum_k |z_ik| |z_jk|."""
    return (c.shape[1] + 8) * U24 * abs_products(c, mean, scale)


def loadings_bound(c, mean, scale, U32):
    """(N + 8) u sum_i |z_ik| |u_ip|, from the same derivation over the N rows."""
    return (c.shape[0] + 8) * U24 * abs_products(c, mean, scale, U32)


def clines(N, K, seed, missing=0.05, unlocated=10):
    """(c, locs): two planted clines.  Samples sit at uniform (x, y) in the unit square; 60 % of the sites follow x with
    frequency 0.1 + 0.8 x, the rest y with 0.15 + 0.7 y: two leading axes with well separated eigenvalues.  The last
    `unlocated` samples have no location."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0.0, 1.0, (N, 2))
    on_x = np.arange(K) < (6 * K) // 10
    freq = np.where(on_x[None], 0.1 + 0.8 * xy[:, :1], 0.15 + 0.7 * xy[:, 1:])
    c = rng.binomial(2, freq).astype(np.int8)
    c[rng.random((N, K)) < missing] = -1
    locs = xy * np.array([[40.0, 25.0]])
    if unlocated:
        locs[-unlocated:] = np.nan
    return c, locs


def write_vcf(path, c, samples):
    """A plain-text diploid VCF whose allele-1 counts are c [N][K]: 0 -> 0/0, 1 -> 0/1, 2 -> 1/1, -1 -> ./. ."""
    gt = {0: "0/0", 1: "0/1", 2: "1/1", -1: "./."}
    with open(path, "w") as fh:
        fh.write("##fileformat=VCFv4.2\n##contig=<ID=1>\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n")
        fh.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(samples) + "\n")
        for k in range(c.shape[1]):
            fh.write(f"1\t{100 + 10 * k}\t.\tA\tT\t.\tPASS\t.\tGT\t" + "\t".join(gt[int(v)] for v in c[:, k]) + "\n")
    return path


def write_sample_data(path, samples, locs):
    with open(path, "w") as fh:
        fh.write("sampleID\tx\ty\n")
        for s, (x, y) in zip(samples, locs):
            fh.write(f"{s}\t{'NA' if np.isnan(x) else repr(float(x))}\t{'NA' if np.isnan(y) else repr(float(y))}\n")
    return path


def read_table(path, sep="\t"):
    rows = [line.split(sep) for line in open(path).read().splitlines()]
    return rows[0], rows[1:]
