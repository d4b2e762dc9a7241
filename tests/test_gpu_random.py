"""The device's random streams against tests/philox_ref.py, bit for bit.

The Glorot init, loc_init_uniform and the Dropout keep masks are Philox4x32-10 keyed by (seed, stream, counter)
(include/locator_hip.h).  Mean, spread, bounds and run-to-run determinism - what the other tests look at - survive a wrong
round constant, a dropped key or counter word and a layout-dependent value; equality with an independent Philox does not.
Seeds and stream ids have bits above 2^32 and mask offsets above 2^34, so all four counter words and both key words are
live.  Every step of the fp32 value maps is one correctly rounded operation (tests/philox_ref.py), so values are compared as
raw words."""
import ctypes as C

import numpy as np
import pytest
import torch

from locator_amd import _lib
from tests import philox_ref as PR
from tests.gpu_util import GUARD_BYTES, guarded

pytestmark = pytest.mark.gpu

MARGIN = 4096
SEED = 0x9E3779B97F4A7C15           # both key words live
STREAM = (0x5 << 32) | 0x0003_0007  # counter word c3 live
GUARD_F32 = np.frombuffer(bytes(GUARD_BYTES), np.uint32)[0]


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _words(t):
    """Host copy of a device buffer as raw 32-bit words."""
    return t.detach().cpu().contiguous().view(-1).view(torch.int32).numpy().view(np.uint32).copy()


def _w32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------ loc_init_uniform
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023])
def test_init_uniform_is_the_reference_stream(n):
    lib = _lib.load()
    room = n + 9                                            # what follows element n - 1 has to keep the guard pattern
    dst, check = guarded(room, torch.float32, MARGIN)
    limit = 0.3
    assert lib.loc_init_uniform(_p(dst), n, limit, SEED, STREAM, _stream()) == 0, lib.loc_last_error()
    got = _words(dst)
    want = _w32(PR.init_uniform_ref(n, np.float32(limit), SEED, STREAM))
    assert np.array_equal(got[:n], want), (n, np.flatnonzero(got[:n] != want)[:8])
    assert np.all(got[n:] == GUARD_F32), "stored past n"
    check("loc_init_uniform destination")
    # another seed half or stream half is another stream
    for seed, stream in ((SEED ^ (1 << 40), STREAM), (SEED, STREAM ^ (1 << 33)), (SEED ^ 1, STREAM), (SEED, STREAM ^ 1)):
        other = _w32(PR.init_uniform_ref(n, np.float32(limit), seed, stream))
        assert not np.array_equal(other, want)
        assert lib.loc_init_uniform(_p(dst), n, limit, seed, stream, _stream()) == 0
        assert np.array_equal(_words(dst)[:n], other), (hex(seed), hex(stream))


# ------------------------------------------------------------------ loc_init_glorot
@pytest.mark.parametrize("R,C_,Rp,Cp", [(2, 2, 2, 2), (40, 2, 64, 2), (70, 70, 96, 96)])
def test_init_glorot_row_major(R, C_, Rp, Cp):
    lib = _lib.load()
    dst, check = guarded(Rp * Cp, torch.float32, MARGIN)
    assert lib.loc_init_glorot(_p(dst), R, C_, Rp, Cp, 0, SEED, STREAM, _stream()) == 0, lib.loc_last_error()
    want = np.zeros((Rp, Cp), np.float32)
    want[:R, :C_] = PR.glorot_ref(R, C_, SEED, STREAM)
    got = _words(dst).reshape(Rp, Cp)
    assert np.array_equal(got, _w32(want)), np.argwhere(got != _w32(want))[:8]        # padding is +0.0, word 0
    assert np.abs(want).max() <= PR.glorot_limit(R, C_)
    check("loc_init_glorot destination")


def _w1s_positions(lib, K, H, Hp):
    k, h = np.meshgrid(np.arange(K), np.arange(H), indexing="ij")
    pos = np.array([lib.loc_w1s_index(int(hh), int(kk), Hp) for kk, hh in zip(k.ravel(), h.ravel())], np.int64)
    return pos.reshape(K, H)


@pytest.mark.parametrize("K,H", [(70, 40), (33, 1000)])
def test_init_glorot_swizzled_is_the_same_logical_matrix(K, H):
    lib = _lib.load()
    d = _lib.make_dims(K, H, 3)
    Kp, Hp = d.Kp, d.Hp
    dst, check = guarded(Kp * Hp, torch.float32, MARGIN)
    assert lib.loc_init_glorot(_p(dst), K, H, Kp, Hp, 1, SEED, STREAM, _stream()) == 0, lib.loc_last_error()
    rm, check_rm = guarded(Kp * Hp, torch.float32, MARGIN)
    assert lib.loc_init_glorot(_p(rm), K, H, Kp, Hp, 0, SEED, STREAM, _stream()) == 0, lib.loc_last_error()
    want = _w32(PR.glorot_ref(K, H, SEED, STREAM))
    pos = _w1s_positions(lib, K, H, Hp)
    assert len(np.unique(pos)) == K * H and pos.min() >= 0 and pos.max() < Kp * Hp
    got = _words(dst)
    assert np.array_equal(got[pos], want), np.argwhere(got[pos] != want)[:8]
    pad = np.ones(Kp * Hp, bool)
    pad[pos.ravel()] = False
    assert pad.sum() == Kp * Hp - K * H and not got[pad].any(), "padding has to be exactly +0.0"
    assert np.array_equal(_words(rm).reshape(Kp, Hp)[:K, :H], want), "row-major and swizzled hold one logical matrix"
    check("swizzled destination")
    check_rm("row-major destination")


# ------------------------------------------------------------------ loc_dropout_mask_fill
P_ODD = 0.1      # its fp32 value times 2^32 is no multiple of 2^8: a threshold kept in fewer than 32 bits would move it
MASK_SEED = ((SEED & 0xFFFFFFFF) ^ 0x64726F70) + (5 << 40)         # as net.py builds it: the replicate above bit 40


@pytest.mark.parametrize("offset", [0, 4 * 999, (1 << 34) + 8])
@pytest.mark.parametrize("n", [1, 5, 4096 + 3])
@pytest.mark.parametrize("p", [0.0, 0.25, 0.5, P_ODD])
def test_dropout_mask_is_a_slice_of_the_one_stream(p, n, offset):
    lib = _lib.load()
    assert PR.dropout_threshold(P_ODD) % 256 != 0 and MASK_SEED >> 40 == 5
    dst, check = guarded(n + 13, torch.uint8, MARGIN)
    before = dst.cpu().numpy().copy()
    assert lib.loc_dropout_mask_fill(_p(dst), n, p, MASK_SEED, offset, _stream()) == 0, lib.loc_last_error()
    got = dst.cpu().numpy()
    want = PR.dropout_mask_ref(n, p, MASK_SEED, offset)
    assert np.array_equal(got[:n], want), (p, n, offset, np.flatnonzero(got[:n] != want)[:8])
    assert np.array_equal(got[n:], before[n:]), "stored past n"
    check("mask")
    if p == 0.0:
        assert want.all()
    elif n > 4096:
        assert abs(float(want.mean()) - (1 - p)) < 0.03
        # the same numbers under another replicate or offset are another part of the stream
        assert not np.array_equal(want, PR.dropout_mask_ref(n, p, MASK_SEED - (5 << 40), offset))
        assert not np.array_equal(want, PR.dropout_mask_ref(n, p, MASK_SEED, offset + (1 << 34)))


def test_dropout_mask_refusals():
    lib = _lib.load()
    dst, check = guarded(64, torch.uint8, MARGIN)
    before = dst.cpu().numpy().copy()
    assert lib.loc_dropout_mask_fill(_p(dst), 8, 0.25, 1, 6, _stream()) != 0 and b"offset" in lib.loc_last_error()
    assert lib.loc_dropout_mask_fill(_p(dst), 8, 1.0, 1, 0, _stream()) != 0 and b"out of [0,1)" in lib.loc_last_error()
    assert lib.loc_dropout_mask_fill(_p(dst), 8, float("nan"), 1, 0, _stream()) != 0
    assert lib.loc_dropout_mask_fill(_p(dst), 0, 0.25, 1, 0, _stream()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(dst.cpu().numpy(), before)
    check("mask")


# ------------------------------------------------------------------ the net layer on top
@pytest.mark.parametrize("replicate", [0, 3])
def test_locator_net_draws_the_documented_streams(replicate):
    """LocatorNet(seed, replicate): every kernel of the initial weights is the reference Glorot stream of the stream id
    net.py derives - (replicate << 16) | layer - and fill_dropout_masks is the mask stream keyed by
    (seed ^ 0x64726F70) + (replicate << 40)."""
    from locator_amd.net import LocatorNet, upload_genotypes
    K, width, nlayers, seed = 70, 40, 3, 0x0123_4567_89AB_CDEF
    rng = np.random.default_rng(1)
    X = upload_genotypes(rng.integers(0, 3, (8, K)).astype(np.uint8))
    Y = torch.zeros((8, 2), dtype=torch.float32, device="cuda")
    net = LocatorNet(X, Y, K, width, nlayers, 0.25, seed=seed, replicate=replicate)
    d, lay, lib = net.d, net.lay, net.lib
    assert (d.K, d.H, d.L, d.Kp, d.Hp) == (K, width, nlayers, 96, 64)
    sid = lambda layer: (replicate << 16) | layer
    flat = _words(net.params)
    want = np.zeros(flat.size, np.uint32)
    want[lay.w1 + _w1s_positions(lib, K, width, d.Hp)] = _w32(PR.glorot_ref(K, width, seed, sid(0)))
    for i in range(d.L - 1):
        wh = np.zeros((d.Hp, d.Hp), np.float32)
        wh[:width, :width] = PR.glorot_ref(width, width, seed, sid(1 + i))
        want[lay.wh + i * d.Hp * d.Hp:lay.wh + (i + 1) * d.Hp * d.Hp] = _w32(wh).ravel()
    wa = np.zeros((d.Hp, 2), np.float32)
    wa[:width] = PR.glorot_ref(width, 2, seed, sid(d.L))
    want[lay.wa:lay.wa + 2 * d.Hp] = _w32(wa).ravel()
    want[lay.wb:lay.wb + 4] = _w32(PR.glorot_ref(2, 2, seed, sid(d.L + 1))).ravel()
    one = _w32(np.float32(1.0))
    want[lay.gamma:lay.gamma + K] = one
    want[lay.mov_var:lay.mov_var + K] = one
    assert np.array_equal(flat, want), np.flatnonzero(flat != want)[:8]
    if net.wht is not None:
        wht = _words(net.wht).reshape(d.L - 1, d.Hp, d.Hp)
        whs = want[lay.wh:lay.wh + (d.L - 1) * d.Hp * d.Hp].reshape(d.L - 1, d.Hp, d.Hp)
        assert np.array_equal(wht, whs.transpose(0, 2, 1))
    # the keep masks of an epoch: n flags from `offset` of the stream keyed by seed, replicate
    n, offset = 3 * 32 * d.Hp + 1, 4 * 1234
    masks, check = guarded(n, torch.uint8, MARGIN)
    net.fill_dropout_masks(masks, n, offset)
    key = ((seed ^ 0x64726F70) + (replicate << 40)) & PR.MASK64
    assert np.array_equal(masks.cpu().numpy(), PR.dropout_mask_ref(n, 0.25, key, offset))
    check("masks")
