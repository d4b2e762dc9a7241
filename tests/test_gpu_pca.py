"""The pca command on the device (locator_amd/csrc/grm_kernels.hip).  loc_grm_pairs against pca.grm_host: element for element,
no tolerance, on inputs whose every product and partial sum is exactly representable in fp32 (mean in {0, 1}, scale in {0, 0.5,
1, 2}) - everything about indexing is tested there: row counts around the tile, site counts around the block, every split of
the sites over groups, pad garbage, degenerate data, stale scratch - and within the derived fp32 bound (K + 8) 2^-24 sum |z_ik|
|z_jk| on real site constants.  loc_pca_loadings likewise.  The command's device path against its --host path within the
perturbation bounds that follow from the element bound (Weyl for eigenvalues, Davis-Kahan for eigenvectors).

Largest measured error / bound, one MI355X: G 0.071 (N = 130, K = 70), 0.033 (K = 150), 0.021 (N = 257, K = 1000), over every
k_groups tried; loadings 0.006 - 0.03 at N = 129 and 0.12 - 0.31 at N = 1 (a single product, whose bound is 9 u)."""
import json
import os

import numpy as np
import pytest

from locator_amd import baselines as BL
from locator_amd import pca as P
from tests import pca_util as U

pytestmark = pytest.mark.gpu
T, B = P.TILE, P.BLOCK


def exact(c, mean, scale, **kw):
    """Device G of an exact case; asserts it equal to the definition, symmetric, and returns it."""
    want = P.grm_host(c, mean, scale)
    got = P.grm_device(c, mean, scale, **kw)
    N = len(c)
    assert got.dtype == np.float64 and got.shape == (N, N)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert np.array_equal(got, got.T)
    return got


# ------------------------------------------------------------------ loc_grm_pairs, exact cases
@pytest.mark.parametrize("N", [1, 2, T - 1, T, T + 1, 2 * T + 3])
def test_row_counts_around_the_tile(N):
    c, mean, scale = U.exact_case(N, 3 * B + 1, 10 + N)
    G = exact(c, mean, scale)
    if N > 2:
        assert not np.array_equal(G, G[::-1, ::-1]) and len(np.unique(np.diag(G))) > 1     # rows differ: a swap would show


@pytest.mark.parametrize("K", [1, B - 1, B, B + 1, 2 * B + 1])
def test_site_counts_around_the_block(K):
    exact(*U.exact_case(T + 1, K, 20 + K))


@pytest.mark.parametrize("K", [3 * B + 1, 5 * B + 7, 7 * B])
@pytest.mark.parametrize("k_groups", [1, 2, 3, 0])
def test_site_groups(K, k_groups):
    """3 B + 1: 4 blocks in groups of 4 / 2, 2 / 2, 2 (the third group not launched); 5 B + 7: 6 blocks, the last partial, as
    6 / 3, 3 / 2, 2, 2; 7 B: 7 blocks as 7 / 4, 3 / 3, 3, 1."""
    exact(*U.exact_case(T + 1, K, 30 + K), k_groups=k_groups)


def test_more_groups_than_blocks():
    exact(*U.exact_case(T + 1, B + 1, 41), k_groups=5)
    exact(*U.exact_case(2 * T + 3, 7 * B, 42), k_groups=7)                               # one block a group, six tile pairs


def test_pad_columns_are_never_interpreted():
    c, mean, scale = U.exact_case(T + 1, 3 * B + 1, 70)
    want = exact(c, mean, scale)
    K = c.shape[1]
    for pitch in ((K + 15) // 16 * 16, (K + 15) // 16 * 16 + 16, 5 * B + 16):
        assert np.array_equal(P.grm_device(c, mean, scale, pitch=pitch, pad_fill=np.random.default_rng(pitch)), want)
        assert np.array_equal(P.grm_device(c, mean, scale, pitch=pitch, pad_fill=2, k_groups=2), want)


def test_degenerate_data():
    c, mean, scale = U.exact_case(T + 5, 2 * B + 9, 60)
    c[3] = -1                                                                            # all-missing rows
    c[T + 1] = -1
    c[:, 5] = -1                                                                         # an all-missing site
    c[:, B + 2] = -1
    scale[[0, B, 2 * B + 8]] = 0.0                                                       # sites that must contribute nothing
    G = exact(c, mean, scale)
    assert not G[3].any() and not G[:, T + 1].any()
    keep = np.ones(c.shape[1], dtype=bool)
    keep[[0, 5, B, B + 2, 2 * B + 8]] = False
    assert np.array_equal(G, P.grm_host(c[:, keep], mean[keep], scale[keep]))
    h, mean, scale = U.exact_case(T + 5, 2 * B + 9, 61, P=1)                             # haploid counts
    assert h.max() == 1
    exact(h, mean, scale)
    exact(np.full((5, B), -1, dtype=np.int8), np.ones(B, dtype=np.float32), np.ones(B, dtype=np.float32))
    assert not P.grm_device(np.zeros((3, 0), dtype=np.int8), np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.float32)).any()


def test_every_pair_of_values_in_one_block():
    vals = np.array([-1, 0, 1, 2], dtype=np.int8)
    c = np.stack([np.repeat(vals, 4), np.tile(vals, 4)])
    G = exact(c, np.ones(16, dtype=np.float32), np.full(16, 2.0, dtype=np.float32))
    # z = 2 (c - 1): -2, 0, 2 over the called values; the 9 called pairs sum (-2, 0, 2) x (-2, 0, 2) = 0, the squares 4 * 8
    assert G[0, 1] == 0 and G[0, 0] == G[1, 1] == 32
    G = exact(c, np.zeros(16, dtype=np.float32), np.ones(16, dtype=np.float32))
    assert G[0, 1] == 9 and G[0, 0] == 20


def test_the_same_bits_on_every_launch_and_from_stale_scratch():
    c = U.spread_counts(2 * T + 3, 5 * B + 7, 80)
    mean, scale, _ = P.site_constants(c, 2)
    for k_groups in (1, 3):
        first = P.grm_device(c, mean, scale, k_groups=k_groups)
        assert np.array_equal(first, first.T) and np.isfinite(first).all()
        assert np.array_equal(P.grm_device(c, mean, scale, k_groups=k_groups), first)
        for pattern in (0x7fc00000, 0xffffffff, 0x7f800001):                             # quiet NaN, all ones, signalling NaN
            assert np.array_equal(P.grm_device(c, mean, scale, k_groups=k_groups, work_fill=pattern), first)


def test_a_row_permutation_permutes_the_result():
    c, mean, scale = U.exact_case(2 * T + 3, 3 * B + 1, 81)
    G = exact(c, mean, scale)
    perm = np.random.default_rng(82).permutation(len(c))
    assert np.array_equal(P.grm_device(c[perm], mean, scale, k_groups=2), G[np.ix_(perm, perm)])


def test_bad_arguments_launch_nothing():
    import torch
    from locator_amd import _lib
    lib = _lib.load()
    N, K = 5, 40
    d_c = torch.zeros((N, 48), dtype=torch.int8, device="cuda")
    d_m = torch.zeros(K + 4, dtype=torch.float32, device="cuda")
    d_s = torch.ones(K + 4, dtype=torch.float32, device="cuda")
    d_g = torch.full((N, N), 77.0, dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    need = lib.loc_grm_work_bytes(N, K, 2)                                               # two blocks, one tile pair
    assert need == 2 * T * T * 4 == lib.loc_grm_work_bytes(N, K, 5) and lib.loc_grm_work_bytes(N, K, 1) == T * T * 4
    assert 0 < lib.loc_grm_work_bytes(N, K, 0) <= need
    assert lib.loc_grm_work_bytes(N, 0, 0) == 0 and lib.loc_grm_work_bytes(-1, K, 0) == -1
    d_w = torch.zeros(need // 4 + 4, dtype=torch.float32, device="cuda")
    c, m, sc, g, w = d_c.data_ptr(), d_m.data_ptr(), d_s.data_ptr(), d_g.data_ptr(), d_w.data_ptr()
    bad = [(c, -1, K, 48, m, sc, 0, g, w, need, s), (c, N, -1, 48, m, sc, 0, g, w, need, s), (c, N, K, 32, m, sc, 0, g, w, need, s),
           (c, N, K, 40, m, sc, 0, g, w, need, s), (c + 1, N, K, 48, m, sc, 0, g, w, need, s), (c, N, K, 48, m + 4, sc, 0, g, w, need, s),
           (c, N, K, 48, m, sc + 4, 0, g, w, need, s), (c, N, K, 48, m, sc, -1, g, w, need, s),
           (c, N, 1 << 31, 1 << 31, m, sc, 0, g, w, need, s), (c, 1 << 20, K, 48, m, sc, 0, g, w, need, s),
           (None, N, K, 48, m, sc, 0, g, w, need, s), (c, N, K, 48, None, sc, 0, g, w, need, s),
           (c, N, K, 48, m, None, 0, g, w, need, s), (c, N, K, 48, m, sc, 0, None, w, need, s),
           (c, N, K, 48, m, sc, 0, g, None, need, s), (c, N, K, 48, m, sc, 2, g, w, need - 1, s),
           (c, N, K, 48, m, sc, 0, g, w + 4, need, s), (c, N, K, 48, m, sc, 0, g, w, -1, s)]
    for args in bad:
        assert lib.loc_grm_pairs(*args) == -1 and b"loc_grm" in lib.loc_last_error(), args
    t = torch.full((K, 3), 77.0, dtype=torch.float32, device="cuda")
    u = torch.zeros((N, 3), dtype=torch.float32, device="cuda")
    for args in ((c, N, K, 48, m, sc, u.data_ptr(), 0, t.data_ptr(), s), (c, N, K, 48, m, sc, u.data_ptr(), 65, t.data_ptr(), s),
                 (c, N, K, 32, m, sc, u.data_ptr(), 3, t.data_ptr(), s), (c, N, K, 48, m, sc, None, 3, t.data_ptr(), s),
                 (c, N, K, 48, m, sc, u.data_ptr(), 3, None, s), (c + 4, N, K, 48, m, sc, u.data_ptr(), 3, t.data_ptr(), s),
                 (c, -1, K, 48, m, sc, u.data_ptr(), 3, t.data_ptr(), s)):
        assert lib.loc_pca_loadings(*args) == -1 and b"loc_pca_loadings" in lib.loc_last_error(), args
    torch.cuda.synchronize()
    assert (d_g == 77.0).all() and (t == 77.0).all()
    assert lib.loc_grm_pairs(c, N, K, 48, m, sc, 0, g, w, need, s) == 0                   # ... and the good call goes through
    torch.cuda.synchronize()
    assert not d_g.any()                                                                 # mean 0, counts 0: z = 0


# ------------------------------------------------------------------ loc_grm_pairs, real constants
@pytest.mark.parametrize("N,K", [(T + 2, 70), (T + 2, 150), (2 * T + 1, 1000)])
def test_real_constants_within_the_fp32_bound(N, K):
    c = U.spread_counts(N, K, 90 + K)
    mean, scale, K_used = P.site_constants(c, 2)
    assert K_used == K and (K + 8) * U.U24 < 1e-4
    want, bound = P.grm_host(c, mean, scale), U.grm_bound(c, mean, scale)
    got = {g: P.grm_device(c, mean, scale, k_groups=g) for g in (0, 1, 2, 3, 5)}
    worst = 0.0
    for g, G in got.items():
        assert np.array_equal(G, G.T)
        assert (np.abs(G - want) <= bound).all(), (g, np.argwhere(np.abs(G - want) > bound)[:5])
        assert not G[bound == 0].any()
        worst = max(worst, float((np.abs(G - want)[bound > 0] / bound[bound > 0]).max()))
        assert (np.abs(G - got[1]) <= 2 * bound).all()
    print(f"loc_grm_pairs N={N} K={K}: largest error / bound = {worst:.4g}")
    # the bar is tight enough to see one lost site
    lost = P.grm_host(c[:, 1:], mean[1:], scale[1:])
    assert np.median(np.abs(lost - want) / bound) > (100 if K == 70 else 20 if K == 150 else 4)


def test_real_constants_with_an_all_missing_row():
    c = U.spread_counts(T + 2, 150, 97)
    c[7] = -1
    mean, scale, _ = P.site_constants(c, 2)
    G, bound = P.grm_device(c, mean, scale), U.grm_bound(c, mean, scale)
    assert not bound[7].any() and not G[7].any() and not G[:, 7].any()
    assert (np.abs(G - P.grm_host(c, mean, scale)) <= bound).all()


# ------------------------------------------------------------------ loc_pca_loadings
@pytest.mark.parametrize("npc", [1, 3, 64])
@pytest.mark.parametrize("K", [1, B + 1, 1000])
@pytest.mark.parametrize("N", [1, T + 1])
def test_loadings_within_the_fp32_bound(N, K, npc):
    c = U.spread_counts(N, K, 100 + N + K)
    if N > 1:
        mean, scale, _ = P.site_constants(c, 2)
    else:                                                                                # one row has no polymorphic site
        rng = np.random.default_rng(K)
        mean, scale = rng.uniform(0.1, 1.9, K).astype(np.float32), rng.uniform(0.7, 3.0, K).astype(np.float32)
    scale[::7] = 0.0
    u = np.random.default_rng(npc).normal(size=(N, npc)).astype(np.float32)
    want, bound = P.loadings_host(c, mean, scale, u), U.loadings_bound(c, mean, scale, u)
    pitch = (K + 15) // 16 * 16 + 16
    got = P.loadings_device(c, mean, scale, u, pitch=pitch, pad_fill=np.random.default_rng(7))
    assert got.dtype == np.float32 and got.shape == (K, npc)
    assert (np.abs(got - want) <= bound).all(), np.argwhere(np.abs(got - want) > bound)[:5]
    assert not got[::7].any() and not got[bound == 0].any()
    assert np.array_equal(P.loadings_device(c, mean, scale, u), got)                     # no pad, same bits
    if (bound > 0).any():
        print(f"loc_pca_loadings N={N} K={K} npc={npc}: largest error / bound = "
              f"{float((np.abs(got - want)[bound > 0] / bound[bound > 0]).max()):.4g}")


@pytest.mark.parametrize("N,K,npc", [(T + 1, 2 * 256 + 5, 17), (67, 300, 64), (3, B + 1, 1)])
def test_loadings_exact_on_integers(N, K, npc):
    c, mean, scale = U.exact_case(N, K, 120 + N)
    u = np.random.default_rng(N).integers(-1, 2, (N, npc)).astype(np.float32)
    want = P.loadings_host(c, mean, scale, u)
    got = P.loadings_device(c, mean, scale, u, pad_fill=np.random.default_rng(3))
    assert np.array_equal(got.astype(np.float64), want), np.argwhere(got != want)[:5]
    assert len(np.unique(want)) > 3


# ------------------------------------------------------------------ the command
def run(tmp_path, name, vcf, sample_data, *extra):
    out = str(tmp_path / name)
    assert P.main(["--vcf", vcf, "--sample_data", sample_data, "--out", out, "--silence"] + list(extra)) == 0
    return out


def scores_of(out):
    return np.array([[float(v) for v in r[1:]] for r in U.read_table(out + "_pca.txt")[1]])


def test_the_command_against_host_on_planted_clines(tmp_path):
    N, K, npc = T + 2, 150, 4
    c, locs = U.clines(N, K, 5)
    samples = [f"s{i}" for i in range(N)]
    vcf = U.write_vcf(str(tmp_path / "clines.vcf"), c, samples)
    sd = U.write_sample_data(str(tmp_path / "clines.txt"), samples, locs)
    located = ~np.isnan(locs).any(axis=1)
    dev = run(tmp_path, "dev", vcf, sd, "--npc", str(npc), "--keep_matrix", "--loadings")
    host = run(tmp_path, "host", vcf, sd, "--npc", str(npc), "--keep_matrix", "--loadings", "--host")
    sdev, shost = (json.load(open(o + "_pca_summary.json")) for o in (dev, host))
    ld = np.load(dev + "_pca_loadings.npz")
    assert sdev["K"] == sdev["K_used"] == K and np.array_equal(ld["sites"], np.arange(K))   # every site passed the filter
    mean, scale, K_used = P.site_constants(c, 2)
    assert np.array_equal(ld["mean"], mean) and np.array_equal(ld["scale"], scale)
    E = U.grm_bound(c, mean, scale)
    Gd, Gh = np.load(dev + "_grm.npz")["G"], np.load(host + "_grm.npz")["G"]
    assert np.array_equal(Gh, P.grm_host(c, mean, scale)) and (np.abs(Gd - Gh) <= E).all() and np.array_equal(Gd, Gd.T)
    normE = np.linalg.norm(E)
    # eigenvalues: Weyl
    lam_d, lam_h = np.array(sdev["eigenvalues"]), np.array(shost["eigenvalues"])
    assert (np.abs(lam_d - lam_h) <= normE / K_used).all()
    # eigenvectors: Davis-Kahan, with the gaps of the host spectrum
    full = np.linalg.eigvalsh(Gh / K_used)[::-1]
    gap = np.array([min(abs(full[q] - full[q - 1]) if q else np.inf, abs(full[q] - full[q + 1])) for q in range(npc)])
    dk = np.minimum(1.0, 2.0 * normE / (K_used * gap))
    print("Davis-Kahan bounds of the planted fixture:", dk)
    assert (dk[:2] < 0.01).all(), "the fixture is too weak to say anything about the first two eigenvectors"
    pd_, ph = scores_of(dev), scores_of(host)
    for q in range(npc):
        ud, uh = pd_[:, q] / np.linalg.norm(pd_[:, q]), ph[:, q] / np.linalg.norm(ph[:, q])
        cos = abs(float(ud @ uh))
        assert np.sqrt(max(0.0, 1.0 - cos * cos)) <= dk[q] + 1e-12, q
        # scores after aligning signs: |u_d - u_h| <= sqrt(2) sin, and the two lengths are the roots of the eigenvalues
        sign = 1.0 if ud @ uh >= 0 else -1.0
        limit = np.sqrt(lam_h[q]) * np.sqrt(2.0) * dk[q] + abs(np.sqrt(lam_d[q]) - np.sqrt(lam_h[q])) + 1e-12
        assert np.linalg.norm(pd_[:, q] - sign * ph[:, q]) <= limit, q
    # loadings: the device's are Z' u / sqrt(K lam) of the DEVICE eigenvectors
    lam, V, _ = P.components(Gd, K_used, npc)
    want = P.report_loadings(P.loadings_host(c, mean, scale, V.astype(np.float32)), K_used, lam)
    lim = U.loadings_bound(c, mean, scale, V.astype(np.float32)) / np.sqrt(K_used * lam)[None]
    assert (np.abs(ld["loadings"] - want) <= lim * (1 + 1e-12)).all()
    # --p auto: what choose_smallest_median returns on the host from the device's own G
    pcs = P.scores(lam, V)
    assert np.array_equal(pcs, pd_)
    placed = P.placements(pcs, locs, located, sdev["pmax"])
    assert sdev["p"] == sdev["p_auto"] == BL.choose_smallest_median(placed, locs, located, False, P.NOTHING_TO_CHOOSE_BY)[0]
    assert sdev["pmax"] == npc
    # a fixed --p 2: the placements are the refit from the device scores
    two = run(tmp_path, "two", vcf, sd, "--npc", str(npc), "--p", "2")
    assert np.array_equal(scores_of(two), pd_)                                           # the same bits on every launch
    head, rows = U.read_table(two + "_pca_locs.txt", ",")
    got = np.array([[float(r[0]), float(r[1])] for r in rows])
    want = P.placements_refit(pd_, locs, located, 2)[1]
    assert head == ["x", "y", "sampleID"] and [r[2] for r in rows] == samples and np.isfinite(got).all()
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()
    # ... and PC-regression finds both planted axes
    assert json.load(open(two + "_pca_summary.json"))["r2_x"] > 0.8 and json.load(open(two + "_pca_summary.json"))["r2_y"] > 0.8


def test_the_command_on_the_golden_vcf(tmp_path):
    from locator_amd import genotypes as G
    names = ("_pca.txt", "_pca_eigenvalues.txt", "_pca_locs.txt", "_pca_summary.json", "_grm.npz", "_pca_loadings.npz")
    extra = ("--npc", "8", "--keep_matrix", "--loadings")
    dev = run(tmp_path, "dev", U.VCF, U.SAMPLE_DATA, *extra)
    s = json.load(open(dev + "_pca_summary.json"))
    assert (s["N"], s["n_located"], s["K"], s["K_used"], s["npc"]) == (500, 450, 5830, 5830, 8)
    assert len(U.read_table(dev + "_pca.txt")[1]) == len(U.read_table(dev + "_pca_locs.txt", ",")[1]) == 500
    assert len(U.read_table(dev + "_pca_eigenvalues.txt")[1]) == 8
    z, ld = np.load(dev + "_grm.npz"), np.load(dev + "_pca_loadings.npz")
    assert z["G"].shape == (500, 500) and np.array_equal(z["G"], z["G"].T) and ld["loadings"].shape == (5830, 8)
    assert np.isfinite(ld["loadings"]).all() and np.allclose((ld["loadings"] ** 2).sum(axis=0), 1.0, rtol=1e-4)
    assert not [f for f in os.listdir(tmp_path) if "predlocs" in f or ".tmp" in f]
    # the same counts through the function: a second device run writes the same bytes, the host run is within Weyl's bound
    vcf = G.read_vcf(U.VCF)
    gt, samples = vcf["calldata/GT"], vcf["samples"]
    _, idx = G.filter_snps(gt, min_mac=2, max_snps=None, verbose=False, sites=True)
    c, ploidy = BL.count_matrix(gt, idx)
    locs = BL.read_locations(U.SAMPLE_DATA, samples, P.PROG)
    again = str(tmp_path / "again")
    P.pca(c, ploidy, samples, locs, again, npc=8, loadings=True, keep_matrix=True, silence=True, sites=idx)
    for name in names:
        assert open(again + name, "rb").read() == open(dev + name, "rb").read(), name
    host = P.pca(c, ploidy, samples, locs, None, npc=8, host=True, silence=True)
    mean, scale, K_used = P.site_constants(c, ploidy)
    E = U.grm_bound(c, mean, scale)
    assert (np.abs(z["G"] - host["_G"]) <= E).all()
    diff = np.abs(np.array(s["eigenvalues"][:4]) - np.array(host["eigenvalues"][:4]))
    print("golden VCF: eigenvalues", s["eigenvalues"][:4], "device - host", diff, "Weyl bound", np.linalg.norm(E) / K_used)
    assert (diff <= np.linalg.norm(E) / K_used).all()
