"""The neighbors command on the device (locator_amd/csrc/ibs_kernels.hip): loc_ibs_pairs against neighbors.pairs_host, d and n
equal element for element, at the smallest shapes that can go wrong - row counts around the tile, site counts around the
staged block, every split of the sites over groups - loc_ibs_knn against neighbors.knn_host, and the command's device path
against its --host path, byte for byte.  Everything is an integer or a float64 from one division: no tolerance anywhere."""
import ctypes as C
import os

import numpy as np
import pytest

from locator_amd import neighbors as NB
from tests import neighbors_util as U

pytestmark = pytest.mark.gpu
T, B = NB.TILE, NB.BLOCK


def both(c, **kw):
    """Device and host (d, n) of the same counts; asserts them equal and returns them."""
    want = NB.pairs_host(c)
    got = NB.pairs_device(c, **kw)
    N = len(c)
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[0].shape == got[1].shape == (N, N)
    assert np.array_equal(got[1], want[1]), np.argwhere(got[1] != want[1])[:5]
    assert np.array_equal(got[0], want[0]), np.argwhere(got[0] != want[0])[:5]
    return got


@pytest.mark.parametrize("N", [1, 2, T - 1, T, T + 1, 2 * T + 3])
def test_row_counts_around_the_tile(N):
    c = U.counts(N, 3 * B + 1, 10 + N)
    d, n = both(c)
    assert (np.diag(d) == 0).all() and np.array_equal(np.diag(n), (c >= 0).sum(axis=1))
    if N > 2:
        assert not np.array_equal(n, n[::-1, ::-1]) and len(np.unique(np.diag(n))) > 1      # rows differ: a swap would show


@pytest.mark.parametrize("K", [1, B - 1, B, B + 1, 2 * B + 1])
def test_site_counts_around_the_block(K):
    both(U.counts(T + 1, K, 20 + K))


@pytest.mark.parametrize("K", [3 * B + 1, 5 * B + 7, 7 * B])
@pytest.mark.parametrize("k_groups", [1, 2, 3, 0])
def test_site_groups(K, k_groups):
    """3 B + 1: 4 blocks in groups of 4 / 2, 2 / 2, 2 (the third group not launched); 5 B + 7: 6 blocks, the last partial, in
    groups of 6 / 3, 3 / 2, 2, 2; 7 B: 7 blocks as 7 / 4, 3 / 3, 3, 1."""
    both(U.counts(T + 1, K, 30 + K), k_groups=k_groups)


def test_more_groups_than_blocks():
    both(U.counts(T + 1, B + 1, 41), k_groups=5)


def test_sums_that_leave_16_bits():
    c = U.counts(T + 1, 20001, 50, missing=0.05)
    c[0], c[T] = 0, 2                                                        # d = 40,002: past a signed and an unsigned 16-bit sum
    d, n = both(c)
    assert d[0, T] == d[T, 0] == d.max() == 40002 and n.max() == 20001
    d3, n3 = NB.pairs_device(c, k_groups=3)
    assert np.array_equal(d3, d) and np.array_equal(n3, n)


def test_an_all_missing_row_and_haploid_counts():
    c = U.counts(T + 5, 2 * B + 9, 60)
    c[3] = -1
    c[T + 1] = -1
    d, n = both(c)
    assert not n[3].any() and not d[3].any() and not n[:, T + 1].any()
    h = U.counts(T + 5, 2 * B + 9, 61, P=1)
    assert h.max() == 1
    both(h)
    z = np.full((5, B), -1, dtype=np.int8)
    assert not both(z)[1].any()


def test_every_pair_of_values_in_one_block():
    vals = np.array([-1, 0, 1, 2], dtype=np.int8)
    c = np.stack([np.repeat(vals, 4), np.tile(vals, 4)])
    d, n = both(c)
    assert n[0, 1] == 9 and d[0, 1] == 8


def test_pad_columns_are_never_interpreted():
    c = U.counts(T + 1, 3 * B + 1, 70)
    want = both(c)
    K = c.shape[1]
    for pitch in ((K + 15) // 16 * 16, (K + 15) // 16 * 16 + 16, 5 * B + 16):
        got = NB.pairs_device(c, pitch=pitch, pad_fill=np.random.default_rng(pitch))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        got = NB.pairs_device(c, pitch=pitch, pad_fill=2, k_groups=2)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_a_row_permutation_permutes_the_result():
    c = U.counts(2 * T + 3, 3 * B + 1, 80)
    d, n = both(c)
    perm = np.random.default_rng(81).permutation(len(c))
    dp, npm = NB.pairs_device(c[perm], k_groups=2)
    assert np.array_equal(dp, d[np.ix_(perm, perm)]) and np.array_equal(npm, n[np.ix_(perm, perm)])


def test_bad_arguments_launch_nothing():
    import torch
    from locator_amd import _lib
    lib = _lib.load()
    N, K = 5, 40
    d_c = torch.zeros((N, 48), dtype=torch.int8, device="cuda")
    d_d = torch.full((N, N), 77, dtype=torch.int32, device="cuda")
    d_n = torch.full((N, N), 77, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    c, d, n = d_c.data_ptr(), d_d.data_ptr(), d_n.data_ptr()
    bad = [(c, -1, K, 48, 0, d, n, None, 0, s), (c, N, -1, 48, 0, d, n, None, 0, s), (c, N, K, 32, 0, d, n, None, 0, s),
           (c, N, K, 40, 0, d, n, None, 0, s), (c + 1, N, K, 48, 0, d, n, None, 0, s), (c, N, K, 48, -1, d, n, None, 0, s),
           (c, N, 1 << 30, 1 << 30, 0, d, n, None, 0, s), (None, N, K, 48, 0, d, n, None, 0, s),
           (c, N, K, 48, 0, None, n, None, 0, s), (c, N, K, 48, 0, d, None, None, 0, s), (c, N, K, 48, 0, d, n, None, -1, s)]
    for args in bad:
        assert lib.loc_ibs_pairs(*args) == -1 and b"loc_ibs_pairs" in lib.loc_last_error(), args
    torch.cuda.synchronize()
    assert (d_d == 77).all() and (d_n == 77).all()
    assert lib.loc_ibs_work_bytes(N, K, 0) >= 0
    cand = torch.ones(N, dtype=torch.uint8, device="cuda")
    nbr = torch.full((N, 64), 77, dtype=torch.int32, device="cuda")
    dist = torch.zeros((N, 64), dtype=torch.float64, device="cuda")
    for P, kmax, dd in ((2, 0, d), (2, 65, d), (3, 4, d), (0, 4, d), (2, 4, None)):
        rc = lib.loc_ibs_knn(dd, n, N, P, cand.data_ptr(), kmax, nbr.data_ptr(), dist.data_ptr(), s)
        assert rc == -1 and b"loc_ibs_knn" in lib.loc_last_error()
    assert lib.loc_ibs_knn(d, n, -1, 2, cand.data_ptr(), 4, nbr.data_ptr(), dist.data_ptr(), s) == -1
    torch.cuda.synchronize()
    assert (nbr == 77).all()


# ------------------------------------------------------------------ neighbours
_TABLES = {}


def tables(N):
    if N not in _TABLES:
        d, n = U.pair_tables(N, 90 + N)
        cand = np.random.default_rng(N).random(N) < 0.7
        cand[:2] = True
        _TABLES[N] = (d, n, cand)
    return _TABLES[N]


@pytest.mark.parametrize("kmax", [1, 5, 64])
@pytest.mark.parametrize("N", [2, 3, 64, 65, 257])
def test_knn_equals_the_definition(N, kmax):
    d, n, cand = tables(N)
    for P in (1, 2):
        want = NB.knn_host(d, n, P, cand, kmax)
        got = NB.knn_device(d, n, N, P, cand, kmax)
        assert got[0].dtype == np.int32 and got[1].dtype == np.float64 and got[0].shape == (N, kmax)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1], equal_nan=True)
    nbr, dist = got
    if N >= 64 and kmax >= 5:
        assert (np.diff(dist[:, :5], axis=1) == 0).any()                     # exact ties inside the first five ...
        tie = np.diff(dist, axis=1) == 0
        assert (np.diff(nbr, axis=1)[tie] > 0).all()                         # ... go to the lower index
        assert cand[nbr[nbr >= 0]].all() and not (nbr == np.arange(N)[:, None]).any()
    if kmax == 64 and N <= 64:
        assert (nbr[:, -1] == -1).all() and np.isnan(dist[:, -1]).all()      # fewer candidates than kmax


def test_knn_with_few_candidates_and_rows_without_any():
    N = 65
    d, n, _ = tables(N)
    n = n.copy()
    n[7] = 0
    n[:, 7] = 0                                                              # row 7 shares no site with anyone
    cand = np.zeros(N, dtype=bool)
    cand[[4, 7, 30, 64]] = True
    want = NB.knn_host(d, n, 2, cand, 5)
    got = NB.knn_device(d, n, N, 2, cand, 5)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1], equal_nan=True)
    assert (got[0][7] == -1).all() and (got[0][:, 3:] == -1).all() and (got[0][4] != 4).all()


# ------------------------------------------------------------------ the command
def test_device_and_host_write_the_same_bytes(tmp_path, capsys):
    vcf = U.write_vcf_cut(str(tmp_path / "cut.vcf"), 120, 2000)
    outs = {}
    names = ("_knn_locs.txt", "_neighbors.txt", "_knn_summary.json", "_close_pairs.txt", "_ibs.npz")
    for mode in ("dev", "host"):
        out = str(tmp_path / mode)
        argv = ["--vcf", vcf, "--sample_data", U.SAMPLE_DATA, "--out", out, "--close", "0.05", "--keep_matrix", "--kmax", "40"]
        assert NB.main(argv + (["--host"] if mode == "host" else [])) == 0
        outs[mode] = [open(out + name, "rb").read() for name in names] + [capsys.readouterr().out]
    assert outs["dev"] == outs["host"]
    assert len(outs["dev"][0].splitlines()) == 121
    assert not [f for f in os.listdir(tmp_path) if "predlocs" in f]
