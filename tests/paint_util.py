"""Inputs, allowances and fixtures shared by tests/test_paint.py and tests/test_gpu_paint.py."""
import numpy as np

from locator_amd import paint as PT
from tests import neighbors_util as NU

VCF, SAMPLE_DATA = NU.VCF, NU.SAMPLE_DATA
FLOOR = 2.0 ** -21
FACTOR = 8.0


def planted(N, K, seed, founders=8, flips=0.01, missing=0.03, stay=0.95, width=0.12):
    """(hap int8 [K][2N], x [N]): every haplotype is a mosaic of `founders` random founder haplotypes that sit at evenly
    spaced points of [0, 1]; a sample at location x ~ U(0, 1) starts a new piece with probability 1 - stay a site and draws the
    piece's founder with weight exp(-(x - place)^2 / (2 width^2)).  Then `flips` of the alleles flipped, `missing` missing."""
    rng = np.random.default_rng(seed)
    found = rng.integers(0, 2, (founders, K)).astype(np.int8)
    place = np.linspace(0.0, 1.0, founders)
    x = rng.uniform(0.0, 1.0, N)
    hap = np.empty((K, 2 * N), dtype=np.int8)
    for s in range(N):
        w = np.exp(-(x[s] - place) ** 2 / (2 * width ** 2))
        w /= w.sum()
        for a in range(2):
            new = rng.random(K) >= stay
            new[0] = True
            pick = rng.choice(founders, K, p=w)
            which = pick[np.maximum.accumulate(np.where(new, np.arange(K), 0))]
            hap[:, 2 * s + a] = found[which, np.arange(K)]
    hap ^= (rng.random(hap.shape) < flips).astype(np.int8)
    hap[rng.random(hap.shape) < missing] = -1
    return hap, x


def everyone(N):
    """(donor, owner, rec) of N samples that all give and all receive."""
    return np.ones(2 * N, dtype=np.uint8), np.repeat(np.arange(N, dtype=np.int32), 2), np.arange(2 * N, dtype=np.int32)


def planted_case(H, K, seed):
    """A loc_paint_copy case of H columns (H even): planted haplotypes, everyone a donor, rho from a rate of 0.05 with a second
    chromosome starting at two thirds; rec a strict subset in non-ascending order."""
    rng = np.random.default_rng(seed)
    hap, _ = planted(H // 2, K, seed)
    donor, owner, _ = everyone(H // 2)
    rho = np.full(K, 0.05)
    if K > 2:
        rho[2 * K // 3] = 1.0
    rec = rng.permutation(H)[:max(1, (2 * H) // 3)].astype(np.int32)
    if len(rec) > 1 and (np.diff(rec) > 0).all():
        rec = rec[::-1].copy()
    return {"h": hap, "donor": donor, "owner": owner, "rec": rec, "rho": rho, "theta": PT.default_theta(H)}


def edge_case(H, K, seed, theta):
    """A case at the model's edges: 10 % missing alleles and site K // 2 all missing; every third individual gives and the
    individual 1 never does; with H == 4 or K even all donor columns belong to the individual 0, whose own columns then have
    D = 0; rho holds 0, 1 and tiny values; rec every column, descending."""
    rng = np.random.default_rng(seed)
    hap = rng.integers(0, 2, (K, H)).astype(np.int8)
    hap[rng.random((K, H)) < 0.1] = -1
    hap[K // 2] = -1
    owner = np.repeat(np.arange((H + 1) // 2, dtype=np.int32), 2)[:H]
    donor = (owner % 3 == 0).astype(np.uint8)
    donor[owner == 1] = 0
    if H == 4 or K % 2 == 0:
        owner[donor != 0] = 0
    rho = rng.choice(np.array([0.0, 1.0, 1e-20, 1e-6, 0.02, 0.5]), K)
    return {"h": hap, "donor": donor, "owner": owner, "rec": np.arange(H - 1, -1, -1, dtype=np.int32), "rho": rho, "theta": theta}


def no_switch_case(H=6, K=200, theta=1e-3):
    """K sites without a switch after the first (rho = 0) and one donor (column 2) that mismatches the recipient column 0
    everywhere: its a-hat and b underflow to 0 on the way."""
    rng = np.random.default_rng(5)
    hap = rng.integers(0, 2, (K, H)).astype(np.int8)
    hap[:, 2] = 1 - hap[:, 0]
    hap[:, 4] = hap[:, 0]
    rho = np.zeros(K)
    donor, owner, _ = everyone(H // 2)
    return {"h": hap, "donor": donor, "owner": owner, "rec": np.array([0, 3], dtype=np.int32), "rho": rho, "theta": theta}


def host(case, dtype):
    return PT.copy_host(case["h"], case["donor"], case["owner"], case["rec"], case["rho"], case["theta"], dtype)


def distances(got, want):
    """(share, chunks, ll): the largest absolute difference of share, |d| / (1 + |x|) of chunks, relative of ll (absolute where
    the wanted ll is 0: a recipient without a donor)."""
    sg, cg, lg = (np.asarray(v, dtype=np.float64) for v in got[:3])
    sw, cw, lw = (np.asarray(v, dtype=np.float64) for v in want[:3])
    rel = np.abs(lg - lw) / np.where(lw != 0, np.abs(lw), 1.0)
    return (float(np.abs(sg - sw).max()) if sw.size else 0.0, float((np.abs(cg - cw) / (1.0 + np.abs(cw))).max()) if cw.size else 0.0,
            float(rel.max()) if rel.size else 0.0)


def allowances(case, want=None):
    """(allowance of share, chunks, ll), float64 answer: FACTOR times the distance of copy_host(float32) from copy_host(float64)
    in each norm, floored at FLOOR."""
    want = host(case, np.float64) if want is None else want
    y = distances(host(case, np.float32), want)
    return tuple(max(FACTOR * v, FLOOR) for v in y), want


def worst_ratio(got, case, want=None):
    """(largest error / allowance over the three norms, the three ratios)."""
    allow, want = allowances(case, want)
    ratios = tuple(d / a for d, a in zip(distances(got, want), allow))
    return max(ratios), ratios


def write_vcf_cut(path, first_sample, n_samples, n_variants, unphase=()):
    """The first n_variants records and the samples first_sample .. first_sample + n_samples - 1 of the golden VCF (its first
    50 samples have no location) as a plain-text VCF; unphase: (record, sample of the cut) pairs whose call is rewritten as the
    heterozygote `0/1`."""
    import gzip
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
            f = line.rstrip("\n").split("\t")
            calls = f[9 + first_sample:9 + first_sample + n_samples]
            if not line.startswith("#"):
                for rec, s in unphase:
                    if rec == kept - 1:
                        calls[s] = "0/1"
            dst.write("\t".join(f[:9] + calls) + "\n")
    return path
