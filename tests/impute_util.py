"""Inputs, allowances and fixtures shared by tests/test_impute.py and tests/test_gpu_impute.py.  The cases are paint_util's."""
import numpy as np

from locator_amd import impute as IM
from locator_amd import paint as PT
from tests import paint_util as U

FLOOR, FACTOR = U.FLOOR, U.FACTOR


def host(case, dtype):
    return IM.dose_host(case["h"], case["donor"], case["owner"], case["rec"], case["rho"], case["theta"], dtype)


def copy_host(case, dtype=np.float64):
    return PT.copy_host(case["h"], case["donor"], case["owner"], case["rec"], case["rho"], case["theta"], dtype)


def distance(got, want):
    """The largest absolute difference of two dose arrays over the entries finite in both."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    both = np.isfinite(got) & np.isfinite(want)
    return float(np.abs(got - want)[both].max()) if both.any() else 0.0


def allowance(want64, got32):
    """FACTOR times the distance of dose_host(float32) from dose_host(float64) on the case, floored at FLOOR."""
    return max(FACTOR * distance(got32, want64), FLOOR)


def structural_nan(case):
    """bool [R][K]: where the definition has no dose whatever the precision: the rows of a recipient without a donor, and the
    sites at which no donor of the recipient holds an allele."""
    h, rec = case["h"], np.asarray(case["rec"])
    H = len(case["donor"])
    dn = (np.asarray(case["donor"])[None, :] != 0) & (np.asarray(case["owner"])[None, :] != np.asarray(case["owner"])[rec][:, None])
    held = (h[:, :H] >= 0).astype(np.int64) @ dn.T.astype(np.int64)                # [K][R]: donors that hold an allele
    return (held.T == 0) | (dn.sum(axis=1) == 0)[:, None]


def hidden_fill(seed, share, N=40, K=300):
    """(truth int8 [K][2N], seen with `share` of the alleles hidden from everyone, hidden bool): planted haplotypes without
    missing alleles."""
    truth, _ = U.planted(N, K, seed, missing=0.0)
    hidden = np.random.default_rng(seed).random(truth.shape) < share
    seen = truth.copy()
    seen[hidden] = -1
    return truth, seen, hidden


def fill_arguments(seen, rate=0.05):
    N = seen.shape[1] // 2
    donor, owner, rec = U.everyone(N)
    return seen, donor, owner, rec, np.full(seen.shape[0], rate), PT.default_theta(2 * N)


def panel_arguments(seed, n_panel=30, n_target=10, K=300, every=4, rate=0.05):
    """(truth of the target haplotypes [K][2 n_target], untyped bool [K], dose_host's six arguments): planted haplotypes, the
    first n_panel samples the panel, the others targets typed at every `every`-th site."""
    truth, _ = U.planted(n_panel + n_target, K, seed, missing=0.0)
    untyped = np.arange(K) % every != 0
    seen = truth.copy()
    seen[np.ix_(untyped, np.arange(2 * n_panel, truth.shape[1]))] = -1
    H = truth.shape[1]
    donor = (np.arange(H) < 2 * n_panel).astype(np.uint8)
    owner = np.repeat(np.arange(H // 2, dtype=np.int32), 2)
    rec = np.arange(2 * n_panel, H, dtype=np.int32)
    return truth[:, 2 * n_panel:], untyped, (seen, donor, owner, rec, np.full(K, rate), PT.default_theta(2 * n_panel))


def mse_against(dose, freq, truth, at):
    """(mse of the dose, mse of the frequency) at the alleles `at` ([K][columns]); dose [columns][K], freq [K]."""
    t = truth[at].astype(np.float64)
    return float(((dose.T[at] - t) ** 2).mean()), float(((np.broadcast_to(freq[:, None], truth.shape)[at] - t) ** 2).mean())


def golden_panel(folder, n_panel=40, n_target=20, n_variants=300, every=4):
    """(panel VCF, target VCF) cut from the golden VCF: its samples 40 .. 40 + n_panel - 1 at the first n_variants records, and
    the next n_target samples at every `every`-th of them (an array typed at a quarter of the panel's sites)."""
    panel = U.write_vcf_cut(f"{folder}/panel.vcf", 40, n_panel, n_variants)
    whole = U.write_vcf_cut(f"{folder}/whole.vcf", 40 + n_panel, n_target, n_variants)
    target, record = f"{folder}/target.vcf", 0
    with open(whole) as src, open(target, "w") as dst:
        for line in src:
            if line.startswith("#"):
                dst.write(line)
                continue
            if record % every == 0:
                dst.write(line)
            record += 1
    return panel, target


def planted_store(path, N=40, K=300, seed=2, missing=0.03):
    """A phased callset store of planted haplotypes on two chromosomes with its site tables: (path, hap [K][2N])."""
    from locator_amd import genotypes as G
    hap, _ = U.planted(N, K, seed, missing=missing)
    rng = np.random.default_rng(seed + 100)
    chrom = np.where(np.arange(K) < 2 * K // 3, "1", "2")
    pos = np.concatenate([np.cumsum(rng.integers(50, 2000, 2 * K // 3)), np.cumsum(rng.integers(50, 2000, K - 2 * K // 3))])
    G.write_callset_zarr(path, hap.reshape(K, N, 2), pos, [f"p{i}" for i in range(N)], chrom=chrom, ref=np.full(K, "A"),
                         alt=np.full(K, "C"))
    return path, hap
