"""Inputs and helpers shared by tests/test_phase.py and tests/test_gpu_phase.py."""
import os

import numpy as np

from locator_amd import phase as PH
from tests import paint_util as PU

VCF, SAMPLE_DATA = PU.VCF, PU.SAMPLE_DATA
planted, write_vcf_cut = PU.planted, PU.write_vcf_cut


def shuffled(hap, seed):
    """hap [K][2N] with the two alleles of every call exchanged with probability 1/2: only heterozygous calls change."""
    swap = np.random.default_rng(seed).random((hap.shape[0], hap.shape[1] // 2)) < 0.5
    out = hap.copy()
    out[:, 0::2], out[:, 1::2] = np.where(swap, hap[:, 1::2], hap[:, 0::2]), np.where(swap, hap[:, 0::2], hap[:, 1::2])
    return out


def random_donors(rng, N, rec, S):
    """don [R][S]: S columns of other samples for every recipient, drawn without regard to repeats."""
    don = np.empty((len(rec), S), dtype=np.int32)
    for i, s in enumerate(rec):
        others = np.setdiff1d(np.arange(2 * N), [2 * s, 2 * s + 1])
        don[i] = rng.choice(others, S, replace=len(others) < S)
    return don


def planted_case(S, K, seed):
    """A loc_phase_viterbi case of S slots: planted haplotypes of S / 2 + 3 samples (at least 4), the order of the calls
    shuffled, rho from a rate of 0.05 with a second chromosome starting at two thirds; rec a strict subset in non-ascending
    order, its donors drawn among the other samples' columns."""
    rng = np.random.default_rng(seed)
    N = max(S // 2 + 3, 4)
    hap = shuffled(planted(N, K, seed, missing=0.02)[0], seed + 1)
    rho = np.full(K, 0.05)
    if K > 2:
        rho[2 * K // 3] = 1.0
    rec = rng.permutation(N)[:min(N - 1, 6)].astype(np.int32)
    if len(rec) > 1 and (np.diff(rec) > 0).all():
        rec = rec[::-1].copy()
    return {"h": hap, "rec": rec, "don": random_donors(rng, N, rec, S), "rho": rho, "theta": 0.01}


def edge_case(S, K, seed, theta):
    """A case at the model's edges: 10 % missing alleles and site K // 2 all missing; rho holds 0, 1 and tiny values; the donor
    rows hold -1 at the end, in the middle or everywhere (a recipient with no donor), and repeated columns."""
    rng = np.random.default_rng(seed)
    N = max(S // 2 + 3, 6)
    hap = rng.integers(0, 2, (K, 2 * N)).astype(np.int8)
    hap[rng.random(hap.shape) < 0.1] = -1
    hap[K // 2] = -1
    rho = rng.choice(np.array([0.0, 1.0, 1e-20, 1e-6, 0.02, 0.5]), K)
    rec = np.arange(5, -1, -1, dtype=np.int32)
    don = random_donors(rng, N, rec, S)
    don[0, S // 2:] = -1                                    # padded at the end
    don[1, ::2] = -1                                        # ... and in between
    don[2] = -1                                             # nobody to copy from
    don[3, :] = don[3, 0]                                   # one donor in every slot: every state ties
    if S >= 4:
        don[4, 1], don[4, 3] = don[4, 0], don[4, 2]         # repeated columns among others
    return {"h": hap, "rec": rec, "don": don, "rho": rho, "theta": theta}


def host(case, dtype=np.float32, **kw):
    return PH.viterbi_host(case["h"], case["rec"], case["don"], case["rho"], case["theta"], dtype, **kw)


def device(case, **kw):
    return PH.viterbi_device(case["h"], case["rec"], case["don"], case["rho"], case["theta"], **kw)


def path_log_probability(case, i, d1, d2, code):
    """The log probability of the path (d1 [K], d2 [K], code [K]) of recipient i, from the module text in float64: the emission
    of every site times tt, tr or rr by the step that led there."""
    h, don, rho, theta = case["h"], np.asarray(case["don"])[i], np.asarray(case["rho"], dtype=np.float64), float(np.float32(case["theta"]))
    s = int(case["rec"][i])
    u = 1.0 / (don >= 0).sum()
    q = lambda x, a: 0.5 if x < 0 else (1 - theta if x == a else theta)
    total = 0.0
    for j in range(h.shape[0]):
        a0, a1 = int(h[j, 2 * s]), int(h[j, 2 * s + 1])
        x, y = int(h[j, don[d1[j]]]), int(h[j, don[d2[j]]])
        if a0 < 0 or a1 < 0:
            e = 1.0
        elif a0 + a1 == 0:
            e = q(x, 0) * q(y, 0)
        elif a0 + a1 == 2:
            e = q(x, 1) * q(y, 1)
        else:
            e = q(x, 1) * q(y, 0) + q(x, 0) * q(y, 1)
        r = 1.0 if j == 0 else rho[j]
        ru = r * u
        t = (1 - r) + ru
        step = code[j] if j else 3
        if j:
            moved = (d1[j] != d1[j - 1]) + (d2[j] != d2[j - 1])
            assert moved <= (0, 1, 1, 2)[step]
        total += np.log(e) + np.log((t * t, t * ru, t * ru, ru * ru)[step])
    return total


def tree_bytes(root):
    """{relative path: bytes} of every file under a directory."""
    out = {}
    for folder, _, files in os.walk(root):
        for name in files:
            path = os.path.join(folder, name)
            out[os.path.relpath(path, root)] = open(path, "rb").read()
    return out
