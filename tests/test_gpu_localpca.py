"""The localpca command on the device (grm_windows_kernel in locator_amd/csrc/grm_kernels.hip).  loc_grm_windows against
localpca.windows_host: bit for bit on inputs whose every product and partial sum is exactly representable in fp32
(pca_util.exact_case) - row counts around the tile, windows that start and end at every alignment, empty, repeated and
overlapping ones; bit for bit against loc_grm_pairs(k_groups = 1) with scale zeroed outside the window on real site constants;
within the derived fp32 bound (S_w + 8) 2^-24 sum_{k in w} |z_ik| |z_jk|; pad bytes, stale output, bad arguments; and the
command's device path against its --host path.

Largest measured error / bound, one MI355X: 0.1468 (N = 130, K = 150), 0.2364 (N = 257, K = 1000; the one-site windows, whose
bound is 9 u for a product that carries two roundings)."""
import json
import os

import numpy as np
import pytest

from locator_amd import localpca as L
from locator_amd import pca as P
from tests import localpca_util as LU
from tests import pca_util as U

pytestmark = pytest.mark.gpu
T, B = P.TILE, P.BLOCK
NAN = 0x7fc00000


def exact_windows(K):
    return np.array([(0, K), (0, 1), (K - 1, K), (5, 6), (3, 13), (15, 17), (31, 33), (16, 48), (B, 2 * B), (17, K), (7, 7), (0, 0),
                     (K, K), (0, 70), (35, 100), (3, 13)], dtype=np.int64)


# ------------------------------------------------------------------ exact cases
@pytest.mark.parametrize("N", [1, 2, T - 1, T, T + 1, 2 * T + 3])
def test_exact_windows_at_every_alignment(N):
    K = 5 * B + 7
    c, mean, scale = U.exact_case(N, K, 200 + N)
    win = exact_windows(K)
    want = L.windows_host(c, mean, scale, win)
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)             # the case is exact in fp32
    on_device = P._upload(c, mean, scale)
    got = L.windows_device(c, mean, scale, win, on_device=on_device, g_fill=NAN)
    assert got.dtype == np.float32 and got.shape == (len(win), N, N)
    for w in range(len(win)):
        assert np.array_equal(got[w], want[w].astype(np.float32)), (w, win[w], np.argwhere(got[w] != want[w])[:5])
        assert np.array_equal(got[w], got[w].T), w
        one = L.windows_device(c, mean, scale, win[w:w + 1], on_device=on_device, g_fill=NAN)      # n_windows = 1
        assert one.shape == (1, N, N) and np.array_equal(one[0], got[w]), w
    assert not got[10].any() and not got[11].any() and not got[12].any()
    if N > 2:
        assert len(np.unique(np.diag(got[0]))) > 1 and not np.array_equal(got[4], got[5])         # rows and windows differ


def test_batches_give_the_bits_of_one_launch():
    N, K = T + 1, 5 * B + 7
    c, mean, scale = U.exact_case(N, K, 260)
    win = exact_windows(K)
    whole = L.windows_device(c, mean, scale, win)
    assert L.batch_windows(N, len(win), 5 * 4 * N * N + 7) == 5 and L.batch_windows(N, len(win), 1) == 1
    assert L.batch_windows(N, 10 ** 6, 1 << 50) == L.MAX_WINDOWS
    assert np.array_equal(L.windows_device(c, mean, scale, win, batch_bytes=5 * 4 * N * N + 7, g_fill=NAN), whole)


# ------------------------------------------------------------------ real constants
def test_a_window_has_the_bits_of_the_pairs_kernel_with_scale_zeroed_outside():
    N, K = T + 2, 150
    c = U.spread_counts(N, K, 301)
    mean, scale, _ = P.site_constants(c, 2)
    win = np.array([(3, 77), (17, 150), (33, 34), (50, 129)], dtype=np.int64)
    got = L.windows_device(c, mean, scale, win)
    for w, (v0, v1) in enumerate(win):
        only = np.zeros_like(scale)
        only[v0:v1] = scale[v0:v1]
        pairs = P.grm_device(c, mean, only, k_groups=1)
        assert np.array_equal(pairs.astype(np.float32).astype(np.float64), pairs)       # one group: the fp32 chain itself
        assert np.array_equal(got[w], pairs.astype(np.float32)), (w, np.argwhere(got[w] != pairs)[:5])
        assert np.array_equal(got[w], got[w].T) and got[w].any()


@pytest.mark.parametrize("N,K", [(T + 2, 150), (2 * T + 1, 1000)])
def test_real_constants_within_the_fp32_bound(N, K):
    c = U.spread_counts(N, K, 310 + K)
    mean, scale, _ = P.site_constants(c, 2)
    scale[::11] = 0.0                                                                    # sites that contribute nothing
    cuts = [0, 1, 38, 39, 103, 150] if K == 150 else [0, 7, 130, 131, 450, 451, 997, 1000]
    win = np.array(list(zip(cuts[:-1], cuts[1:])) + [(0, K), (cuts[1], cuts[-2])], dtype=np.int64)
    want, bound = L.windows_host(c, mean, scale, win), LU.window_bound(c, mean, scale, win)
    got = L.windows_device(c, mean, scale, win).astype(np.float64)
    worst = 0.0
    for w in range(len(win)):
        err = np.abs(got[w] - want[w])
        assert np.array_equal(got[w], got[w].T), w
        assert (err <= bound[w]).all(), (w, win[w], np.argwhere(err > bound[w])[:5])
        assert not got[w][bound[w] == 0].any(), w                                        # an element whose bound is 0 is 0
        if (bound[w] > 0).any():
            worst = max(worst, float((err[bound[w] > 0] / bound[w][bound[w] > 0]).max()))
    print(f"loc_grm_windows N={N} K={K}: largest error / bound = {worst:.4g}")
    # the bar is tight enough to see one lost site of the longest window
    assert scale[1] > 0
    lost = L.windows_host(np.delete(c, 1, axis=1), np.delete(mean, 1), np.delete(scale, 1), [(0, K - 1)])[0]
    assert np.median(np.abs(lost - want[-2]) / bound[-2]) > (20 if K == 150 else 4)


# ------------------------------------------------------------------ pad bytes and stale output
def test_pad_bytes_stale_output_and_permutations():
    import torch
    N, K = T + 5, 5 * B + 16
    pitch = K + 48
    assert pitch % 16 == 0
    c, mean, scale = U.exact_case(N, K, 320)
    win = np.array([(0, K), (K - 3, K), (K - 20, K), (9, 9), (1, 100), (K, K)], dtype=np.int64)
    want = L.windows_host(c, mean, scale, win).astype(np.float32)
    plain = L.windows_device(c, mean, scale, win)
    assert np.array_equal(plain, want)
    rng = np.random.default_rng(321)
    padded = L.windows_device(c, mean, scale, win, pitch=pitch, pad_fill=rng, g_fill=NAN)
    assert np.array_equal(padded, want) and not padded[3].any() and not padded[5].any()   # empty windows: zeros, not the fill
    # rows past n_rows: seven more rows of arbitrary bytes behind the N the launch is told of
    buf = rng.integers(-128, 128, (N + 7, pitch), dtype=np.int8)
    buf[:N, :K] = c
    on_device = (torch.from_numpy(buf).cuda(), torch.from_numpy(mean).cuda(), torch.from_numpy(scale).cuda(), pitch)
    for pattern in (NAN, 0xffffffff, 0x7f800001):
        assert np.array_equal(L.windows_device(c, mean, scale, win, on_device=on_device, g_fill=pattern), want)
    # real constants: the same bits on every launch, whatever g held
    r = U.spread_counts(2 * T + 3, K, 322)
    rmean, rscale, _ = P.site_constants(r, 2)
    first = L.windows_device(r, rmean, rscale, win, g_fill=NAN)
    assert np.isfinite(first).all() and np.array_equal(first, L.windows_device(r, rmean, rscale, win, g_fill=0xffffffff))
    # a row permutation permutes every window's matrix
    perm = rng.permutation(len(r))
    moved = L.windows_device(r[perm], rmean, rscale, win)
    for w in range(len(win)):
        assert np.array_equal(moved[w], first[w][np.ix_(perm, perm)]), w


# ------------------------------------------------------------------ bad arguments
def test_bad_arguments_launch_nothing():
    import torch
    from locator_amd import _lib
    lib = _lib.load()
    N, K, W = 5, 40, 3
    d_c = torch.zeros((N, 48), dtype=torch.int8, device="cuda")
    d_m = torch.zeros(K + 4, dtype=torch.float32, device="cuda")
    d_s = torch.ones(K + 4, dtype=torch.float32, device="cuda")
    d_w = torch.tensor([[0, K], [3, 9], [0, 0], [1, 2]], dtype=torch.int64, device="cuda")
    d_g = torch.full((W, N, N), 77.0, dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    c, m, sc, wn, g = d_c.data_ptr(), d_m.data_ptr(), d_s.data_ptr(), d_w.data_ptr(), d_g.data_ptr()
    bad = [(c, -1, K, 48, m, sc, wn, W, g, s), (c, N, -1, 48, m, sc, wn, W, g, s), (c, N, K, 32, m, sc, wn, W, g, s),
           (c, N, K, 40, m, sc, wn, W, g, s), (c, N, K, -48, m, sc, wn, W, g, s), (c + 1, N, K, 48, m, sc, wn, W, g, s),
           (c, N, K, 48, m + 4, sc, wn, W, g, s), (c, N, K, 48, m, sc + 4, wn, W, g, s), (c, N, K, 48, m, sc, wn + 8, W, g, s),
           (c, N, K, 48, m, sc, wn, W, g + 2, s), (c, N, K, 48, m, sc, wn, 0, g, s), (c, N, K, 48, m, sc, wn, -1, g, s),
           (c, N, K, 48, m, sc, wn, L.MAX_WINDOWS + 1, g, s), (c, N, 1 << 31, 1 << 31, m, sc, wn, W, g, s),
           (c, 1 << 20, K, 48, m, sc, wn, W, g, s), (None, N, K, 48, m, sc, wn, W, g, s), (c, N, K, 48, None, sc, wn, W, g, s),
           (c, N, K, 48, m, None, wn, W, g, s), (c, N, K, 48, m, sc, None, W, g, s), (c, N, K, 48, m, sc, wn, W, None, s)]
    for args in bad:
        assert lib.loc_grm_windows(*args) == -1 and b"loc_grm_windows" in lib.loc_last_error(), args
    torch.cuda.synchronize()
    assert (d_g == 77.0).all()
    assert lib.loc_grm_windows(c, N, K, 48, m, sc, wn, W, g, s) == 0                     # ... and the good call goes through
    torch.cuda.synchronize()
    assert not d_g.any()                                                                 # mean 0, counts 0: z = 0
    for win in ([(0, 41)], [(-1, 3)], [(5, 4)], np.zeros((0, 2))):                      # the driver refuses before any upload
        with pytest.raises(ValueError):
            L.windows_device(np.zeros((N, K), dtype=np.int8), np.zeros(K, dtype=np.float32), np.ones(K, dtype=np.float32), win)


# ------------------------------------------------------------------ the command
def run(tmp_path, name, vcf, *extra):
    out = str(tmp_path / name)
    assert L.main(["--vcf", vcf, "--out", out, "--silence"] + list(extra)) == 0
    return out


def test_the_command_against_host_on_the_planted_windows(tmp_path):
    """The allowance for |D_dev - D_host| is 8 x the yardstick, floored at 8 x 2^-24: the yardstick is what the same
    definitions give with z and G_w formed in float32 NumPy.  Measured on one MI355X: yardstick max |D_host32 - D_host64| =
    1.143e-08, so the allowance is the floor 4.768e-07; measured max |D_dev - D_host| = 1.046e-08."""
    vcf, sd, c, locs, win = LU.write_planted(tmp_path)
    extra = ("--sample_data", sd, "--window_snps", "96", "--keep_matrix", "--keep_components")
    dev, host = run(tmp_path, "dev", vcf, *extra), run(tmp_path, "host", vcf, *extra, "--host")
    sdev, shost = (json.load(open(o + "_localpca_summary.json")) for o in (dev, host))
    assert sdev["flagged"] == shost["flagged"] == [4, 5, 6] and sdev["n_regions"] == shost["n_regions"] == 1
    (_, td), (_, th) = LU.read_windows(dev), LU.read_windows(host)
    for col in ("window", "chrom", "start", "stop", "first_site", "last_site", "n_sites", "K_used", "kept", "flag"):
        assert td[col] == th[col], col
    (hd, rd), (hh, rh) = U.read_table(dev + "_localpca_regions.txt"), U.read_table(host + "_localpca_regions.txt")
    assert hd == hh and [r[:-1] for r in rd] == [r[:-1] for r in rh] and len(rd) == 1   # all but peak_score, a float
    # the yardstick: the same definitions with z and G_w formed in float32 NumPy
    mean, scale, _ = P.site_constants(c, 2)
    used = L.used_sites(scale, win)
    Dh = np.load(host + "_localpca_dist.npz")["D"]
    D32 = L.pc_dist(*LU.definitions32(c, mean, scale, win, used, 2))
    yard = float(np.abs(D32 - Dh).max())
    allow = max(8.0 * yard, 8.0 * LU.U24)
    Dd = np.load(dev + "_localpca_dist.npz")["D"]
    diff = float(np.abs(Dd - Dh).max())
    print(f"planted windows: yardstick max |D_host32 - D_host64| = {yard:.4g}, allowance {allow:.4g}, "
          f"measured max |D_dev - D_host| = {diff:.4g}")
    assert diff <= allow
    # the device's components are the decomposition of the device's own matrices
    G = L.windows_device(c, mean, scale, win)
    comp = np.load(dev + "_localpca_components.npz")
    for w in (0, 5, 11):
        lam, U_, _ = P.components(G[w], int(used[w]), 2)
        assert np.array_equal(comp["eigenvalues"][w], lam) and np.array_equal(comp["U"][w], U_)
    r2x, r2y = np.array([float(v) for v in td["pc1_r2_x"]]), np.array([float(v) for v in td["pc1_r2_y"]])
    pl = np.isin(np.arange(12), LU.PLANTED)
    assert (r2x[~pl] > r2y[~pl]).all() and (r2y[pl] > r2x[pl]).all()


def test_the_command_on_the_golden_vcf(tmp_path):
    names = ("_localpca_windows.txt", "_localpca_regions.txt", "_localpca_summary.json", "_localpca_dist.npz",
             "_localpca_components.npz")
    extra = ("--sample_data", U.SAMPLE_DATA, "--window_snps", "200", "--keep_matrix", "--keep_components")
    dev = run(tmp_path, "dev", U.VCF, *extra)
    assert all(os.path.exists(dev + n) for n in names)
    s = json.load(open(dev + "_localpca_summary.json"))
    assert (s["N"], s["n_located"], s["K"], s["W"], s["W_kept"]) == (500, 450, 5830, 30, 30)
    assert all(np.isfinite(v) for v in s["mds_eigenvalues"] + s["median"] + s["mad"])
    assert s["mds_eigenvalues"][0] >= s["mds_eigenvalues"][1] > 0
    head, t = LU.read_windows(dev)
    assert len(t["window"]) == 30 and [int(v) for v in t["n_sites"]] == [200] * 29 + [30]
    for col in head[9:]:
        assert np.isfinite([float(v) for v in t[col]]).all(), col
    z = np.load(dev + "_localpca_dist.npz")
    assert z["D"].shape == (30, 30) and np.isfinite(z["D"]).all() and np.array_equal(z["D"], z["D"].T)
    assert len(U.read_table(dev + "_localpca_regions.txt")[1]) == s["n_regions"]
    again = run(tmp_path, "again", U.VCF, *extra, "--batch_bytes", str(7 * 4 * 500 * 500))       # five launches, not one
    for name in names:
        assert open(again + name, "rb").read() == open(dev + name, "rb").read(), name
    assert not [f for f in os.listdir(tmp_path) if ".tmp" in f]
