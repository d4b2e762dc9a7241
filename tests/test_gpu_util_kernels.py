"""The utility kernels of util_kernels.hip / stack_fused.hip against NumPy, where no other test takes them.

gather_columns_kernel, genotype_max_kernel and pack_genotypes_2bit_kernel stride rows over a capped grid.y
(LOC_GRID_Y_MAX = 32768): a batched --jacknife or --windows predict has more rows than that, no other test has.  MANY =
32768 + 37 rows reaches the striding with matrices of a few MB.  loc_genotype_max decides whether a predict may use the
int8 pipe, so its scalar tail (K % 16), its 8-block form (K >= 65536) and "columns >= K do not count" are each aimed at
with a single 127 in a matrix of ones.  The W1 layout conversions and the hidden-kernel transpose are compared element by
element on guarded destinations.  Everything here is integer or copy work: the bar is equality."""
import ctypes as C

import numpy as np
import pytest
import torch

from locator_amd import _lib
from tests.gpu_util import guarded

pytestmark = pytest.mark.gpu

GRID_Y_MAX = 32768
MANY = GRID_Y_MAX + 37
MARGIN = 4096


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset)


# ------------------------------------------------------------------ loc_gather_columns
def test_gather_columns_beyond_the_grid_cap():
    lib = _lib.load()
    K, sp, dp = 257, 288, 320                               # two column blocks of 256 (the second with one live thread)
    rng = np.random.default_rng(11)
    x = rng.integers(0, 256, (MANY, sp), dtype=np.uint8)
    order = rng.integers(0, sp, K).astype(np.int32)         # with repeats, as a bootstrap draws them
    order[:3] = (sp - 1, 0, sp - 1)
    src = torch.from_numpy(x).cuda()
    so = torch.from_numpy(order).cuda()
    dst = torch.full((MANY, dp), 0xEE, dtype=torch.uint8, device="cuda")
    assert lib.loc_gather_columns(_p(src), sp, _p(so), K, _p(dst), dp, MANY, _stream()) == 0, lib.loc_last_error()
    got = dst.cpu().numpy()
    bad = np.flatnonzero((got[:, :K] != x[:, order]).any(axis=1))
    assert bad.size == 0, (bad.size, bad[:4], "first row beyond the cap is", GRID_Y_MAX)
    assert (got[:, K:] == 0xEE).all(), "columns >= K of the destination were written"
    assert np.array_equal(src.cpu().numpy(), x)
    # nothing to do: no launch, return 0
    dst.fill_(0xEE)
    assert lib.loc_gather_columns(_p(src), sp, _p(so), K, _p(dst), dp, 0, _stream()) == 0
    assert lib.loc_gather_columns(_p(src), sp, _p(so), 0, _p(dst), dp, MANY, _stream()) == 0
    torch.cuda.synchronize()
    assert bool((dst == 0xEE).all())


# ------------------------------------------------------------------ loc_pack_genotypes_2bit
def _pack_ref(x, Kp):
    """include/locator_hip.h: X2[r][j] = sum_i (X[r][4 j + i] & 3) << 2 i"""
    out = np.zeros((x.shape[0], Kp // 4), np.uint8)
    for i in range(4):
        out |= (x[:, i:Kp:4] & 3) << np.uint8(2 * i)
    return out


@pytest.mark.parametrize("Kp", [64, 4112])
def test_pack_genotypes_beyond_the_grid_cap(Kp):
    """Kp 4112 = 257 sixteen-SNP groups: a second x-block with one live thread.  Pitches wider than the rows on both sides;
    the bytes beyond Kp / 4 of a packed row stay as they were."""
    lib = _lib.load()
    xp, x2p = Kp + 16, Kp // 4 + 8
    rng = np.random.default_rng(Kp)
    x = rng.integers(0, 256, (MANY, xp), dtype=np.uint8)    # the formula masks with 3: any byte is a legal input
    X = torch.from_numpy(x).cuda()
    X2 = torch.full((MANY, x2p), 0xEE, dtype=torch.uint8, device="cuda")
    assert lib.loc_pack_genotypes_2bit(_p(X), xp, MANY, Kp, _p(X2), x2p, _stream()) == 0, lib.loc_last_error()
    got = X2.cpu().numpy()
    bad = np.flatnonzero((got[:, :Kp // 4] != _pack_ref(x, Kp)).any(axis=1))
    assert bad.size == 0, (bad.size, bad[:4], "first row beyond the cap is", GRID_Y_MAX)
    assert (got[:, Kp // 4:] == 0xEE).all(), "bytes beyond Kp / 4 of a packed row were written"


def test_pack_genotypes_refusals():
    lib = _lib.load()
    X = torch.zeros((4, 64), dtype=torch.uint8, device="cuda")
    X2 = torch.full((4, 32), 0xEE, dtype=torch.uint8, device="cuda")
    for args in ((_p(X, 1), 64, 4, 32, _p(X2), 32), (_p(X), 40, 4, 32, _p(X2), 32), (_p(X), 64, 4, 40, _p(X2), 32),
                 (_p(X), 64, 4, 32, _p(X2, 2), 32), (_p(X), 64, 4, 32, _p(X2), 10), (_p(X), 64, 4, 64, _p(X2), 12)):
        assert lib.loc_pack_genotypes_2bit(*args, _stream()) != 0, args
        assert b"loc_pack_genotypes_2bit" in lib.loc_last_error()
    assert lib.loc_pack_genotypes_2bit(_p(X), 64, 0, 64, _p(X2), 32, _stream()) == 0
    torch.cuda.synchronize()
    assert bool((X2 == 0xEE).all())


# ------------------------------------------------------------------ loc_genotype_max
def _gmax(lib, X, pitch, n_rows, K, preset=0):
    out = torch.full((1,), preset, dtype=torch.int32, device="cuda")
    assert lib.loc_genotype_max(_p(X), pitch, n_rows, K, _p(out), _stream()) == 0, lib.loc_last_error()
    return int(out.item())


def _gmax_cases():
    for K in (15, 16, 47, 65536 + 87):
        K16 = K & ~15
        rows = (0, MANY - 1, GRID_Y_MAX) if K < 65536 else (0, 2)
        n_rows = MANY if K < 65536 else 3
        cols = {0, K16 - 1, K16, K - 1}
        if K >= 65536:
            # 8 column blocks, each thread 16 bytes, block b takes bytes [4096 b, 4096 b + 4096) + 32768 i: the first and
            # the last block's share in their first and later passes
            cols |= {100, 4095, 4096, 28672, 32767, 32768 + 4100, 65535, 65536 + 10}
        yield K, n_rows, rows, sorted(c for c in cols if 0 <= c < K)


@pytest.mark.parametrize("K,n_rows,rows,cols", list(_gmax_cases()), ids=lambda v: str(v) if isinstance(v, int) else None)
def test_genotype_max_finds_a_single_large_value(K, n_rows, rows, cols):
    """A matrix of ones with one 127, one launch per place; the pitch is one vector wider than the rows need and the columns
    K .. pitch hold 255 throughout, which must never count."""
    lib = _lib.load()
    pitch = (K + 15) // 16 * 16 + 16
    X = torch.ones((n_rows, pitch), dtype=torch.uint8, device="cuda")
    X[:, K:] = 255
    assert _gmax(lib, X, pitch, n_rows, K) == 1, "255 in the columns K .. pitch counted"
    for r in rows:
        for c in cols:
            X[r, c] = 127
            got = _gmax(lib, X, pitch, n_rows, K)
            X[r, c] = 1
            assert got == 127, (K, r, c, got)
    # rows beyond n_rows and columns beyond K do not count either
    X[n_rows - 1, K - 1] = 99
    assert _gmax(lib, X, pitch, n_rows - 1, K) == 1 and _gmax(lib, X, pitch, n_rows, K - 1) == 1
    assert _gmax(lib, X, pitch, n_rows, K) == 99


def test_genotype_max_keeps_a_larger_preset_and_refuses_misalignment():
    lib = _lib.load()
    K, pitch = 47, 64
    x = np.random.default_rng(3).integers(0, 3, (300, pitch)).astype(np.uint8)
    x[17, 40] = 2
    X = torch.from_numpy(x).cuda()
    assert _gmax(lib, X, pitch, 300, K) == 2
    assert _gmax(lib, X, pitch, 300, K, preset=5) == 5, "out[0] = max(out[0], ...)"
    assert _gmax(lib, X, pitch, 0, K, preset=5) == 5 and _gmax(lib, X, pitch, 300, 0, preset=5) == 5
    out = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    assert lib.loc_genotype_max(_p(X, 1), pitch, 299, K, _p(out), _stream()) != 0
    assert b"loc_genotype_max" in lib.loc_last_error()
    assert lib.loc_genotype_max(_p(X), 47, 300, K, _p(out), _stream()) != 0
    assert int(out.item()) == 7


# ------------------------------------------------------------------ loc_w1_swizzle / loc_w1_unswizzle
@pytest.mark.parametrize("K,H", [(1, 1), (33, 31), (70, 1000)])
def test_w1_swizzle_places_every_element_and_round_trips(K, H):
    lib = _lib.load()
    d = _lib.make_dims(K, H, 2)
    Kp, Hp = d.Kp, d.Hp
    rng = np.random.default_rng(K * 1009 + H)
    w = rng.integers(1, 1 << 32, (K, H), dtype=np.uint32)           # any word, never +0.0: padding is told from payload
    src = torch.from_numpy(w.view(np.int32)).cuda().view(torch.float32)
    w1s, check_s = guarded(Kp * Hp, torch.float32, MARGIN)
    assert lib.loc_w1_swizzle(_p(src), K, H, _p(w1s), Kp, Hp, _stream()) == 0, lib.loc_last_error()
    got = w1s.cpu().view(torch.int32).numpy().view(np.uint32)
    k, h = np.meshgrid(np.arange(K), np.arange(H), indexing="ij")
    pos = np.array([lib.loc_w1s_index(int(b), int(a), Hp) for a, b in zip(k.ravel(), h.ravel())], np.int64).reshape(K, H)
    assert len(np.unique(pos)) == K * H and pos.min() >= 0 and pos.max() < Kp * Hp
    assert np.array_equal(got[pos], w), np.argwhere(got[pos] != w)[:8]
    pad = np.ones(Kp * Hp, bool)
    pad[pos.ravel()] = False
    assert not got[pad].any(), "padding has to be exactly +0.0"
    check_s("w1s")
    back, check_b = guarded(K * H, torch.float32, MARGIN)
    assert lib.loc_w1_unswizzle(_p(w1s), Kp, Hp, _p(back), K, H, _stream()) == 0, lib.loc_last_error()
    assert np.array_equal(back.cpu().view(torch.int32).numpy().view(np.uint32).reshape(K, H), w)
    assert np.array_equal(src.cpu().view(torch.int32).numpy().view(np.uint32), w)
    check_b("w_kh")
    check_s("w1s")


# ------------------------------------------------------------------ loc_transpose_hidden
@pytest.mark.parametrize("n_hidden", [1, 3])
@pytest.mark.parametrize("Hp", [32, 96, 1024])
def test_transpose_hidden(Hp, n_hidden):
    lib = _lib.load()
    w = np.random.default_rng(Hp + n_hidden).integers(0, 1 << 32, (n_hidden, Hp, Hp), dtype=np.uint32)
    src = torch.from_numpy(w.view(np.int32)).cuda().view(torch.float32)
    dst, check = guarded(n_hidden * Hp * Hp, torch.float32, MARGIN)
    assert lib.loc_transpose_hidden(_p(src), _p(dst), Hp, n_hidden, _stream()) == 0, lib.loc_last_error()
    got = dst.cpu().view(torch.int32).numpy().view(np.uint32).reshape(n_hidden, Hp, Hp)
    assert np.array_equal(got, w.transpose(0, 2, 1))
    assert np.array_equal(src.cpu().view(torch.int32).numpy().view(np.uint32), w)
    check("WhT")
    before = got.copy()
    assert lib.loc_transpose_hidden(_p(src), _p(dst), Hp, 0, _stream()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(dst.cpu().view(torch.int32).numpy().view(np.uint32).reshape(n_hidden, Hp, Hp), before)
