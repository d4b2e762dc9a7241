"""The ld command on the device (locator_amd/csrc/ld_kernels.hip): loc_ld_band against the host forms of locator_amd/ld.py - the
six sums equal element for element, r2 bit for bit, the mask word for word - at the smallest shapes that can go wrong: site
counts around the tile, sample counts around the staged block, windows around a mask word and around the tile, every kind of
reach; then the command's device path and --ld_prune against their --host paths.  No tolerance appears: everything compared
is an integer, a bit, or a float64 from three correctly rounded operations on exact integers (pca --ld_prune excepted, whose
fp32 matrix is held to the bounds of tests/test_gpu_pca.py)."""
import json
import os

import numpy as np
import pytest

from locator_amd import ld as LD
from locator_amd import neighbors as NB
from tests import ld_util as U

pytestmark = pytest.mark.gpu
T, B = LD.TILE, LD.BLOCK


def same(got, want):
    """(over, sums, r2) of the device against the host's: r2 by its bits, NaNs by mask."""
    over, sums, r2 = got
    assert over.dtype == np.uint32 and over.shape == want[0].shape
    if sums is not None:
        assert sums.dtype == np.int32 and sums.shape == want[1].shape
        assert np.array_equal(sums, want[1]), np.argwhere(sums != want[1])[:5]
    if r2 is not None:
        assert r2.dtype == np.float64 and r2.shape == want[2].shape
        nan = np.isnan(want[2])
        assert np.array_equal(np.isnan(r2), nan), np.argwhere(np.isnan(r2) != nan)[:5]
        assert np.array_equal(r2[~nan].view(np.int64), want[2][~nan].view(np.int64))
    assert np.array_equal(over, want[0]), np.argwhere(over != want[0])[:5]


def both(ct, W, reach=None, thr=0.2, **kw):
    """Device and host answers of the same counts; asserts them equal and returns the host's.  The device outputs hold 0x77
    bytes before the launch: an element the launch left alone shows."""
    want = LD.band_host(ct, W, reach, thr)
    same(LD.band_device(ct, W, reach, thr, fill=0x77, **kw), want)
    return want


# ------------------------------------------------------------------ shapes
@pytest.mark.parametrize("K", [1, 2, T - 1, T, T + 1, 2 * T + 3])
def test_site_counts_around_the_tile(K):
    over, sums, r2 = both(U.site_counts(K, 3 * B + 1, 10 + K), T + 5)
    assert not sums[-1].any() and np.isnan(r2[-1]).all()                      # the last site meets nobody
    if K > T:
        assert over.any() and (~np.isnan(r2)).sum() > K and len(np.unique(sums[:, 0, 0])) > 3


@pytest.mark.parametrize("N", [1, B - 1, B, B + 1, 2 * B + 1])
def test_sample_counts_around_the_block(N):
    over, sums, r2 = both(U.site_counts(T + 1, N, 20 + N), T + 5)
    assert sums[..., 0].max() <= N and (N > 1) == bool((~np.isnan(r2)).any())


@pytest.mark.parametrize("W", [1, 31, 32, 33, T - 1, T, T + 1, 2 * T + 5, 3 * T + 8])
def test_windows_around_a_word_and_the_tile(W):
    K = 3 * T + 7                                                             # the last window is one above K
    over, sums, r2 = both(U.site_counts(K, B + 1, 30 + W), W)
    assert over.shape == (K, (W + 31) // 32) and over.any()
    assert sums[0, min(W, K - 1) - 1].any() and (W < K or not sums[:, K - 1:].any())


def test_no_site_and_no_sample():
    over, sums, r2 = both(np.zeros((0, 5), dtype=np.int8), 7)
    assert over.shape == (0, 1) and sums.shape == (0, 7, 6) and r2.shape == (0, 7)
    over, sums, r2 = both(np.zeros((T + 1, 0), dtype=np.int8), 7)
    assert not over.any() and not sums.any() and np.isnan(r2).all()


# ------------------------------------------------------------------ reach
_COUNTS = {}


def counts():
    """One fixture for the reach and data cases: 3 tiles and a bit, 2 blocks and a bit."""
    if not _COUNTS:
        _COUNTS["ct"] = U.site_counts(3 * T + 7, 2 * B + 9, 40)
        _COUNTS["ct"].setflags(write=False)
    return _COUNTS["ct"]


@pytest.mark.parametrize("kind", ["null", "zero", "random", "break_inside_a_tile", "break_on_a_tile_edge", "unclamped"])
def test_reach(kind):
    ct = counts()
    K, W = len(ct), T + 9
    rng = np.random.default_rng(41)
    reach = {"null": lambda: None, "zero": lambda: np.zeros(K, dtype=np.int32),
             "random": lambda: rng.integers(0, W + 1, K).astype(np.int32),
             "break_inside_a_tile": lambda: LD.reach_host(K, W, np.where(np.arange(K) < T + 13, "a", "b")),
             "break_on_a_tile_edge": lambda: LD.reach_host(K, W, np.where(np.arange(K) < 2 * T, "a", "b")),
             "unclamped": lambda: rng.integers(-5, 3 * W, K).astype(np.int32)}[kind]()
    over, sums, r2 = both(ct, W, reach)
    if kind == "zero":
        assert not over.any() and not sums.any() and np.isnan(r2).all()
    if kind == "break_inside_a_tile":
        assert reach[T + 12] == 0 and reach[T + 11] == 1 and not sums[T + 12].any() and sums[T + 13, W - 1].any()
    if kind == "break_on_a_tile_edge":
        assert reach[2 * T - 1] == 0 and not sums[2 * T - 1].any() and not sums[2 * T - 2, 1:].any() and sums[2 * T - 2, 0].any()
    if kind == "unclamped":
        assert reach.max() > W and reach.min() < 0 and not sums[reach <= 0].any()


# ------------------------------------------------------------------ data
def test_pad_bytes_are_never_interpreted():
    ct = counts()
    K, N = ct.shape
    want = both(ct, 40)
    for pitch in ((N + 15) // 16 * 16, (N + 15) // 16 * 16 + 16, 5 * B + 16):
        same(LD.band_device(ct, 40, None, 0.2, pitch=pitch, pad_fill=np.random.default_rng(pitch), fill=0x77), want)
        same(LD.band_device(ct, 40, None, 0.2, pitch=pitch, pad_fill=2, fill=0x77), want)


def test_haploid_counts_an_all_missing_and_a_monomorphic_site():
    h = U.site_counts(T + 5, 2 * B + 9, 61, P=1)
    assert h.max() == 1
    both(h, 33)
    ct = counts().copy()
    ct[3] = -1
    ct[T + 1] = 2
    ct[T + 2] = np.where(ct[T + 2] >= 0, 1, -1)                               # monomorphic where called
    over, sums, r2 = both(ct, 12)
    assert not sums[3].any() and np.isnan(r2[3]).all() and np.isnan(r2[2, 0]) and not sums[2, 0].any()
    assert sums[T, 0, 0] > 0 and np.isnan(r2[T, 0]) and np.isnan(r2[T + 2]).all() and np.isnan(r2[T + 1, 0])
    assert np.isfinite(r2[4, 0])


def test_sums_that_leave_16_bits():
    N = 20001
    rng = np.random.default_rng(50)
    ct = U.site_counts(5, N, 51, missing=0.02, linked=0.0)
    ct[1] = ct[3] = 2
    ct[1, rng.choice(N, 40, replace=False)] = 0
    ct[3, rng.choice(N, 30, replace=False)] = 1
    over, sums, r2 = both(ct, 4)
    assert sums[1, 1].tolist() == [N, 2 * (N - 40), 2 * N - 30, sums[1, 1, 3], 4 * (N - 40), 4 * N - 90]
    assert sums[1, 1, 4] > 65535 and sums[1, 1, 3] > 65535 and np.isfinite(r2[1, 1])


def test_a_permutation_of_the_samples_changes_nothing():
    ct = counts()
    want = both(ct, 70, thr=0.1)
    perm = np.random.default_rng(81).permutation(ct.shape[1])
    same(LD.band_device(ct[:, perm], 70, None, 0.1, fill=0x77), want)


@pytest.mark.parametrize("thr", [-1.0, 0.0, 0.5, 1.0, 2.0])
def test_thresholds(thr):
    over = both(counts(), 35, thr=thr)[0]
    assert (thr >= 1.0) == (not over.any())


# ------------------------------------------------------------------ outputs
@pytest.mark.parametrize("fill", [0x77, 0xff])
def test_every_element_of_every_output_is_defined(fill):
    ct = counts()
    K = len(ct)
    reach = np.random.default_rng(90).integers(0, 50, K).astype(np.int32)
    want = LD.band_host(ct, 45, reach, 0.2)
    for want_sums, want_r2 in ((True, True), (False, True), (True, False), (False, False)):
        got = LD.band_device(ct, 45, reach, 0.2, want_sums=want_sums, want_r2=want_r2, fill=fill)
        assert (got[1] is None) == (not want_sums) and (got[2] is None) == (not want_r2)
        same(got, want)


def test_bad_arguments_launch_nothing():
    import torch
    from locator_amd import _lib
    lib = _lib.load()
    K, N, W = 5, 40, 8
    d_ct = torch.zeros((K, 48), dtype=torch.int8, device="cuda")
    d_over = torch.full((K, 1), 0x77, dtype=torch.int32, device="cuda")
    d_sums = torch.full((K, W, 6), 0x77, dtype=torch.int32, device="cuda")
    d_r2 = torch.full((K, W), 77.0, dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    c, o, q, r = d_ct.data_ptr(), d_over.data_ptr(), d_sums.data_ptr(), d_r2.data_ptr()
    bad = [(None, K, N, 48, W, None, 0.2, o, q, r, s), (c, K, N, 48, W, None, 0.2, None, q, r, s),
           (c, -1, N, 48, W, None, 0.2, o, q, r, s), (c, K, -1, 48, W, None, 0.2, o, q, r, s),
           (c, K, N, 32, W, None, 0.2, o, q, r, s), (c, K, N, 40, W, None, 0.2, o, q, r, s),
           (c, K, N, -16, W, None, 0.2, o, q, r, s), (c + 1, K, N, 48, W, None, 0.2, o, q, r, s),
           (c, K, N, 48, 0, None, 0.2, o, q, r, s), (c, K, N, 48, -3, None, 0.2, o, q, r, s),
           (c, K, N, 48, LD.MAX_WINDOW + 1, None, 0.2, o, q, r, s), (c, K, 1 << 20, 1 << 20, W, None, 0.2, o, q, r, s),
           (c, K, N, 48, W, None, float("nan"), o, q, r, s), (c, K, N, 48, W, None, float("inf"), o, q, r, s),
           (c, K, N, 48, W, None, float("-inf"), o, q, r, s)]
    for args in bad:
        assert lib.loc_ld_band(*args) == -1 and b"loc_ld_band" in lib.loc_last_error(), args
    torch.cuda.synchronize()
    assert (d_over == 0x77).all() and (d_sums == 0x77).all() and (d_r2 == 77.0).all()


# ------------------------------------------------------------------ the commands
def test_the_command_writes_the_host_bytes_on_planted_ld(tmp_path, capsys):
    vcf, ct, chrom, pos = U.planted_vcf(tmp_path / "p.vcf")
    outs = {}
    names = ("_ld_sites.txt", "_ld_summary.json", "_ld.npz")
    for mode in ("dev", "host"):
        out = str(tmp_path / mode)
        argv = ["--vcf", vcf, "--out", out, "--r2", "0.3", "--ld_window", "70", "--ld_window_bp", "14500", "--keep_matrix"]
        assert LD.main(argv + (["--host"] if mode == "host" else [])) == 0
        outs[mode] = [open(out + name, "rb").read() for name in names] + [capsys.readouterr().out]
    assert outs["dev"] == outs["host"]
    s = json.loads(outs["dev"][1])
    z = np.load(str(tmp_path / "dev") + "_ld.npz")
    assert 0 < s["n_kept"] < s["K"] and s["n_pairs_over"] > 0 and (ct[z["sites"]] < 0).any()
    by_sites = LD.reach_host(s["K"], 70, chrom[z["sites"]])
    assert len(set(chrom[z["sites"]])) == 2 and (z["reach"] == 70).any() and (z["reach"] < by_sites).any()     # each limit binds


def test_the_command_writes_the_host_bytes_on_the_golden_vcf(tmp_path):
    outs = {}
    for mode in ("dev", "host"):
        out = str(tmp_path / mode)
        argv = ["--vcf", U.VCF, "--out", out, "--r2", "0.2", "--keep_matrix", "--silence"]
        assert LD.main(argv + (["--host"] if mode == "host" else [])) == 0
        outs[mode] = [open(out + name, "rb").read() for name in ("_ld_sites.txt", "_ld_summary.json", "_ld.npz")]
    assert outs["dev"] == outs["host"]
    assert json.loads(outs["dev"][1])["n_kept"] == 1996


def test_neighbors_with_ld_prune_writes_the_host_bytes(tmp_path):
    from tests import neighbors_util as NU
    vcf = NU.write_vcf_cut(str(tmp_path / "cut.vcf"), 120, 2000)
    outs = {}
    names = ("_knn_locs.txt", "_neighbors.txt", "_knn_summary.json", "_ibs.npz")
    for mode in ("dev", "host"):
        out = str(tmp_path / mode)
        argv = ["--vcf", vcf, "--sample_data", U.SAMPLE_DATA, "--out", out, "--keep_matrix", "--kmax", "20", "--silence",
                "--ld_prune", "0.2", "--ld_window", "50"]
        assert NB.main(argv + (["--host"] if mode == "host" else [])) == 0
        outs[mode] = [open(out + name, "rb").read() for name in names]
    assert outs["dev"] == outs["host"]
    s = json.loads(outs["dev"][2])
    assert 0 < s["K"] < s["K_before_prune"] and s["ld_window"] == 50


def test_pca_with_ld_prune_takes_the_host_sites(tmp_path):
    from locator_amd import pca as P
    from tests import neighbors_util as NU
    from tests import pca_util as PU
    vcf = NU.write_vcf_cut(str(tmp_path / "cut.vcf"), 120, 2000)
    res = {}
    for mode in ("dev", "host"):
        out = str(tmp_path / mode)
        argv = ["--vcf", vcf, "--sample_data", U.SAMPLE_DATA, "--out", out, "--keep_matrix", "--loadings", "--npc", "4", "--silence",
                "--ld_prune", "0.2", "--ld_window", "50", "--max_SNPs", "500", "--seed", "4"]
        assert P.main(argv + (["--host"] if mode == "host" else [])) == 0
        res[mode] = (json.load(open(out + "_pca_summary.json")), np.load(out + "_pca_loadings.npz"), np.load(out + "_grm.npz")["G"])
    (sd, ld_d, Gd), (sh, ld_h, Gh) = res["dev"], res["host"]
    assert sd["K"] == sh["K"] == len(ld_d["sites"]) < sd["K_before_prune"] == 500 and np.array_equal(ld_d["sites"], ld_h["sites"])
    assert (np.diff(ld_d["sites"]) < 0).any()                                # the survivors keep the order of the draw
    assert np.array_equal(ld_d["mean"], ld_h["mean"]) and np.array_equal(ld_d["scale"], ld_h["scale"])
    # the numbers: the bounds tests/test_gpu_pca.py holds the unpruned command to, on the pruned counts
    from locator_amd import baselines as BL
    from locator_amd import genotypes as G
    c, ploidy = BL.count_matrix(G.read_vcf(vcf)["calldata/GT"], ld_d["sites"])
    E = PU.grm_bound(c, ld_d["mean"], ld_d["scale"])
    assert (np.abs(Gd - Gh) <= E).all()
    diff = np.abs(np.array(sd["eigenvalues"]) - np.array(sh["eigenvalues"]))
    assert (diff <= np.linalg.norm(E) / sd["K_used"]).all()
    assert not [f for f in os.listdir(tmp_path) if ".tmp" in f]
