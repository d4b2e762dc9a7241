"""--dosage (X holds q = rint(63 d), values 0..126) on every training schedule and every predict route the library can
take, against the oracle on the float64 matrix q / 63.  test_gpu_dosage.py covers one unchained step, one chained fit and
the predict modes at one shape; here each schedule of train_step_impl (two-block chain, row-block kernels, Dropout on the
BatchNorm output, Dropout after layer 1, width 512, the per-layer kernels, padding in both dimensions, cross-epoch chaining
with an int8 validation sweep) and each predict route (per-block, per-layer, head loop, rows forward, bf16 pieces, int8
with 3 / 2 planes, more rows than one chunk) sees values up to 126, every case asserting that its route actually ran.
Then the int8 GEMM's overflow bound at q <= 126 / 127 with the worst-case digit image, the BatchNorm numerators at their
limits, and --dosage --jacknife against the oracle.

Tolerances are the GT ones: loss / val_loss 5e-4 along a trajectory, 2e-5 for one step, 2e-5 absolute for exact predict
routes and 1e-3 of the output scale for the 2-plane and 2-piece ones."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest
import torch

from locator_amd import genotypes as G
from locator_amd import locator as L
from oracle import locator_oracle as O
from tests.dosage_util import SAMPLES, golden_counts, noisy_dosage, write_dosage_vcf
from tests.gpu_util import build_net, make_problem, maxerr, params_err, randomize_params
from tests.test_gpu_chain import _assert_same_fit

pytestmark = pytest.mark.gpu
U = G.DOSAGE_UNIT


def _sync():
    torch.cuda.synchronize()


def _dosage_problem(n, K, width, nlayers, seed):
    """make_problem's genotypes as noisy dosages over the whole range 0..126: q = rint(63 (x + noise)), every seventh
    column uniform over 0..126, columns 0-1 pinned at 126 and 2-3 at 0."""
    x, y, p, rng = make_problem(n, K, width, nlayers, seed=seed)
    q = np.clip(np.rint((x + rng.normal(0, 0.3, x.shape)) * U), 0, 2 * U)
    q[:, 6::7] = rng.integers(0, 2 * U + 1, q[:, 6::7].shape)
    q[:, :2] = 2 * U
    q[:, 2:4] = 0
    q = q.astype(np.uint8)
    assert q.max() == 2 * U
    return q, q.astype(np.float64) / U, y, p


def _bn4_of(net):
    """Inference scale / shift [scale | shift | mean | rstd] of the net's current parameters (q units)."""
    from locator_amd import _lib
    d, lay, lib = net.d, net.lay, net.lib
    P = net.params.data_ptr()
    bn4 = torch.zeros(4 * d.Kp, device="cuda")
    _lib.check(lib.loc_bn_infer_scale_shift(d.K, d.Kp, P + 4 * lay.gamma, P + 4 * lay.beta, P + 4 * lay.mov_mean,
                                            P + 4 * lay.mov_var, bn4.data_ptr(), None))
    _sync()
    return bn4.cpu().numpy()


# ------------------------------------------------------------------ 1. every training schedule against oracle.fit on q / 63
def _route_two_block_chain(net, r):
    return r.chain and r.slot_rows == 64 and net.d.Hp == 256


def _route_row_blocks(slot):
    return lambda net, r: not r.chain and net.use_fused and r.slot_rows == slot


def _route_in_dropout(net, r):
    return net.d.n_pre == 0 and net.mask_width == net.d.Kp and not net.use_fused and not r.chain


def _route_dr(chained):
    return lambda net, r: net.d.n_pre == 1 and net.use_fused and r.chain == chained and r.slot_rows == 32


def _route_chain(Hp, Kp=None):
    return lambda net, r: r.chain and net.d.Hp == Hp and (Kp is None or net.d.Kp == Kp)


def _route_per_layer(Hp):
    return lambda net, r: not net.use_fused and not r.chain and net.d.Hp == Hp


@pytest.mark.parametrize("K,width,nlayers,batch,n_train,chain,route", [
    (600, 256, 4, 48, 130, None, _route_two_block_chain),     # chained steps of two 32-row blocks; last batch of 34
    (500, 128, 4, 128, 300, None, _route_row_blocks(128)),    # row-block kernels, four blocks; last batch of 44
    (400, 64, 4, 200, 450, None, _route_row_blocks(256)),     # > 128 rows: row blocks streamed from L2; last batch of 50
    (500, 256, 6, 256, 600, None, _route_row_blocks(256)),    # eight row blocks at width 256; last batch of 88
    (300, 64, 1, 32, 70, None, _route_in_dropout),            # --nlayers 1: Dropout on the BatchNorm output (*_in_dropout)
    (400, 128, 2, 32, 80, None, _route_dr(True)),             # --nlayers 2: Dropout after layer 1, applied by the chained reduction
    (400, 256, 3, 32, 80, False, _route_dr(False)),           # --nlayers 3: Dropout after layer 1 in the unchained forward
    (500, 512, 4, 32, 70, None, _route_chain(512)),           # width 512, chained
    (300, 96, 4, 32, 70, None, _route_per_layer(96)),         # width 96: per-layer kernels
    (300, 600, 3, 32, 70, None, _route_per_layer(608)),       # width 600 -> 608: per-layer, single-buffered forward
    (97, 1024, 2, 16, 40, None, _route_per_layer(1024)),      # width 1024, the limit; K = 3 tiles + 1 SNP
    (257, 33, 5, 16, 33, None, _route_chain(64, 288)),        # width 33 -> 64, K 257 -> 288: padding in both dimensions
], ids=["batch48-two-block-chain", "batch128-row-blocks", "batch200-row-blocks", "batch256-row-blocks",
        "nlayers1-in-dropout", "nlayers2-dropout-after-l1-chained", "nlayers3-dropout-after-l1-unchained",
        "width512-chained", "width96-per-layer", "width600-per-layer", "width1024-per-layer", "width33-K257-padded"])
def test_every_schedule_matches_oracle_fit_on_q_over_63(K, width, nlayers, batch, n_train, chain, route):
    """3 epochs (eager epoch 0, captured graph after it) against oracle.fit on q / 63 with the same init, permutations
    and the device's dropout masks: loss / val_loss within 5e-4, every weight within 1e-4, the moving statistics (in
    dosage units) within 2e-5."""
    from locator_amd.train import EpochRunner
    n_val = 9
    q, xd, y, p = _dosage_problem(n_train + n_val, K, width, nlayers, seed=K + width + batch)
    tr, va = np.arange(n_train), np.arange(n_train, n_train + n_val)
    net = build_net(q, y, p, drop_p=0.25, seed=5, unit=U)
    runner = EpochRunner(net, tr, va, batch, use_graph=True, chain=chain)
    assert route(net, runner), (net.d.Hp, net.d.Kp, net.use_fused, runner.chain, runner.slot_rows)
    perms = [np.random.default_rng(e).permutation(n_train) for e in range(3)]
    masks, hist = [], {"loss": [], "val_loss": []}
    for e in range(3):
        l, vl = runner.run_epoch(perms[e])
        masks.append(runner.masks.cpu().numpy().reshape(runner.steps, runner.slot_rows, net.mask_width).copy())
        hist["loss"].append(l)
        hist["val_loss"].append(vl)
    mw = K if nlayers == 1 else width
    fit_kw = dict(batch_size=batch, max_epochs=3, patience=100, drop_p=0.25, perm_fn=lambda e: perms[e],
                  mask_fn=lambda e, s, nb: masks[e][s, :nb, :mw])
    pref = O.copy_params(p)
    href, _ = O.fit(pref, xd[tr], y[tr], xd[va], y[va], **fit_kw)
    dl, dv = maxerr(hist["loss"], href["loss"]), maxerr(hist["val_loss"], href["val_loss"])
    got = net.export_params()
    errs = params_err(got, pref)
    if max(dl, dv) >= 5e-4 or max(errs.values()) >= 1e-4:
        # the wide, freshly initialised nets overshoot (test_gpu_edge): there the bar is the fp32 oracle's own distance
        p32 = O.cast_params(p, np.float32)
        h32, _ = O.fit(p32, xd[tr].astype(np.float32), y[tr].astype(np.float32), xd[va].astype(np.float32),
                       y[va].astype(np.float32), **fit_kw)
        floor = max(maxerr(h32["loss"], href["loss"]), maxerr(h32["val_loss"], href["val_loss"]))
        wfloor = max(params_err(p32, pref).values())
        assert width > 512 and floor > 1e-4, (dl, dv, floor, errs)
        assert max(dl, dv) < 3 * floor + 5e-4, (dl, dv, floor)
        assert max(errs.values()) < 3 * wfloor + 1e-4, (errs, wfloor)
    assert maxerr(got["mov_mean"], pref["mov_mean"]) < 2e-5 and maxerr(got["mov_var"], pref["mov_var"]) < 2e-5, errs
    flat = net.params.cpu().numpy()
    assert not flat[net.lay.b1 + net.d.H:net.lay.b1 + net.d.Hp].any()
    assert not flat[net.lay.gamma + K:net.lay.gamma + net.d.Kp].any()


def test_fitloop_cross_epoch_chain_with_an_int8_validation_sweep():
    """FitLoop's default schedule: chained steps, the hand-over across the epoch boundary, and the validation sweep in
    the second workspace (ws_predict) between its two halves.  520 validation rows take the int8 pipe (three planes,
    x_max = 126) inside the captured epochs.  History and best weights against oracle.fit on q / 63."""
    from locator_amd.train import FitLoop
    K, width, nlayers, n_train, n_val = 600, 256, 4, 100, 520
    q, xd, y, p = _dosage_problem(n_train + n_val, K, width, nlayers, seed=77)
    tr, va = np.arange(n_train), np.arange(n_train, n_train + n_val)
    net = build_net(q, y, p, drop_p=0.25, seed=11, unit=U)
    perms = [np.random.default_rng(300 + e).permutation(n_train) for e in range(3)]
    loop = FitLoop(net, tr, va, batch_size=32, max_epochs=3, patience=100, perm_fn=lambda e: perms[e], xchain=True)
    r = loop.runner
    assert r.chain and r.xchain and net.ws_predict is not None and net.ws_predict.data_ptr() != net.ws.data_ptr()
    hist = loop.run().history
    # the dropout masks the device drew for epoch e (start_epoch fills them from the net's seed at offset e * size)
    buf = torch.zeros_like(r.masks)
    masks = []
    for e in range(3):
        net.fill_dropout_masks(buf, buf.numel(), e * buf.numel())
        masks.append(buf.cpu().numpy().reshape(r.steps, r.slot_rows, net.d.Hp).copy())
    # the route of the validation sweep: the int8 image at three planes with genotypes up to 126
    assert net.genotype_max() == 2 * U
    assert net.lib.loc_predict_image_mode(C.byref(net.cnet()), n_val) == 13
    pref = O.copy_params(p)
    href, best = O.fit(pref, xd[tr], y[tr], xd[va], y[va], batch_size=32, max_epochs=3, patience=100, drop_p=0.25,
                       perm_fn=lambda e: perms[e], mask_fn=lambda e, s, nb: masks[e][s, :nb, :width])
    assert maxerr(hist["loss"], href["loss"]) < 5e-4, (hist["loss"], href["loss"])
    assert maxerr(hist["val_loss"], href["val_loss"]) < 5e-4, (hist["val_loss"], href["val_loss"])
    got = net.export_params()                            # the best epoch's weights, restored by finish()
    errs = params_err(got, best)
    assert max(errs.values()) < 1e-4, errs
    assert maxerr(got["mov_mean"], best["mov_mean"]) < 2e-5 and maxerr(got["mov_var"], best["mov_var"]) < 2e-5


# ------------------------------------------------------------------ 2. same bits under dosage; the row-block backward at the one-step bar
def _epochs(q, y, p, tr, va, perms, chain, use_graph, batch):
    from locator_amd.train import EpochRunner
    net = build_net(q, y, p, drop_p=0.25, seed=5, unit=U)
    runner = EpochRunner(net, tr, va, batch, use_graph=use_graph, chain=chain)
    assert runner.chain == chain and runner.slot_rows == (64 if batch > 32 else 32)
    hist = [runner.run_epoch(perm) for perm in perms]
    _sync()
    m, v = net.export_adam()
    return hist, net.export_params(), m, v, net.params.cpu().numpy()


@pytest.mark.parametrize("width,batch", [(512, 32), (256, 32), (128, 32), (64, 32), (256, 48)])
def test_chained_unchained_and_graph_replay_agree_under_dosage(width, batch):
    """test_gpu_chain's chained = unchained (up to the summation order of two reductions: _assert_same_fit, the GT bar)
    and graph replay = eager enqueue (bit for bit), with q up to 126."""
    K, nlayers, n_train = 2000, 4, 70
    q, _, y, p = _dosage_problem(n_train + 20, K, width, nlayers, seed=width + batch)
    tr, va = np.arange(n_train), np.arange(n_train, n_train + 20)
    perms = [np.random.default_rng(7 + e).permutation(n_train) for e in range(3)]
    h0, p0, m0, v0, _ = _epochs(q, y, p, tr, va, perms, False, True, batch)
    h1, p1, m1, v1, f1 = _epochs(q, y, p, tr, va, perms, True, True, batch)
    h2, _, _, _, f2 = _epochs(q, y, p, tr, va, perms, True, False, batch)
    assert maxerr(h0, h1) < 2e-5, (h0, h1)
    _assert_same_fit(p0, p1, m0, m1, v0, v1)
    assert h1 == h2 and np.array_equal(f1, f2)
    assert np.abs(p1["W"][0] - p["W"][0]).max() > 1e-4


def _two_epochs(q, y, p, tuning):
    from locator_amd.train import EpochRunner
    net = build_net(q, y, p, drop_p=0.25, seed=7, tuning=tuning, unit=U)
    runner = EpochRunner(net, np.arange(60), np.arange(60, 70), 32, use_graph=False)
    out = [runner.run_epoch(np.random.default_rng(e).permutation(60)) for e in range(2)]
    _sync()
    return net.params.cpu().numpy().copy(), out


def test_speed_hints_do_not_change_a_single_bit_under_dosage():
    q, _, y, p = _dosage_problem(70, 4096, 256, 4, seed=3)
    ref_w, ref_out = _two_epochs(q, y, p, None)
    for tuning in ({"l1b_nt_mask": -1}, {"l1b_nt_mask": 15}, {"l1b_nt_mask": 9},
                   {"stack_xcd_stride": 1, "stack_helpers": -1}, {"stack_helpers": 3}, {"stack_xcd_stride": 2}):
        w, out = _two_epochs(q, y, p, tuning)
        assert np.array_equal(w, ref_w) and out == ref_out, tuning


def test_row_block_backward_meets_the_single_step_bar_on_q_over_63():
    """tuning l1b_rows = 1 sends <= 32-row steps of width 256 through the bf16x3 row-block backward: three steps (Adam t =
    1..3, one of 21 rows), each within test_gpu_edge's one-step bar of the fp64 oracle on q / 63."""
    K, width, nlayers = 5830, 256, 10
    q, xd, y, p = _dosage_problem(64, K, width, nlayers, seed=K)
    rng = np.random.default_rng(K)
    net = build_net(q, y, p, drop_p=0.25, tuning={"l1b_rows": 1}, unit=U)
    assert net.use_fused and net.d.Hp == 256
    pr = O.copy_params(p)
    m, v = O.zeros_like_trainable(pr), O.zeros_like_trainable(pr)
    stats = torch.zeros(2 * net.d.Kp, device="cuda")
    for t, n_b in enumerate((32, 21, 32), start=1):
        idx = rng.choice(64, n_b, replace=False)
        mask_np = (rng.random((32, width)) >= 0.25).astype(np.uint8)
        rows = np.zeros(32, np.int32)
        rows[:n_b] = idx
        rows_d = torch.from_numpy(rows).cuda()
        loss = torch.zeros(1, device="cuda")
        net.epoch_bn_stats(rows_d, 32, n_b, 1, stats)         # a dosage net takes its statistics per epoch (here: one step)
        net.train_step(rows_d, n_b, t, torch.from_numpy(mask_np).cuda(), loss, bn_ready=True)
        _sync()
        ref = O.train_step(pr, m, v, t, 1e-3, xd[idx], y[idx], mask_np[:n_b, :width], 0.25)
        assert abs(loss.item() - ref) < 2e-5 * max(1, abs(ref)), (t, loss.item(), ref)
        errs = params_err(net.export_params(), pr)
        assert max(errs.values()) < (1e-5 if t == 1 else 2e-5), (t, errs)


# ------------------------------------------------------------------ 3. every predict route at q <= 126
def _predict_case(K, width, nlayers, n, seed, **kw):
    from locator_amd.net import LocatorNet, upload_genotypes
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 2 * U + 1, (n, K), dtype=np.uint8)
    q[:, :5] = 2 * U
    q[:, 5:8] = 0
    xd = q.astype(np.float64) / U
    p = randomize_params(O.init_params(K, width, nlayers, rng), rng)
    p["mov_mean"] = xd.mean(0)
    p["mov_var"] = xd.var(0) + 0.05
    X = upload_genotypes(q)
    Y = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
    net = LocatorNet(X, Y, K, width, nlayers, 0.25, seed=1, unit=U, **kw)
    net.import_params(O.cast_params(p, np.float32))
    yhat = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
    net.predict_rows(torch.arange(n, dtype=torch.int32, device="cuda"), n, yhat)
    _sync()
    ref = O.predict(O.cast_params(O.cast_params(p, np.float32), np.float64), xd, batch=2048)
    return net, yhat.cpu().numpy(), ref


def _rows_forward(net):
    """More than 32 rows below the image thresholds: loc_l1_forward_rows (no image) at a width / piece count it supports."""
    return net._image_mode == 0 and bool(net.lib.loc_l1_rows_supported(net.d.Hp, net.predict_pieces)) and \
        bool(net.lib.loc_stack_fused_supported(net.d.Hp))


@pytest.mark.parametrize("K,width,nlayers,n,kw,route,exact", [
    (2000, 256, 4, 20, {}, lambda net: net.use_fused and net._image_mode == 0, True),        # <= 32 rows, fused width
    (2000, 96, 4, 20, {}, lambda net: not net.use_fused and net.d.Hp == 96, True),          # <= 32 rows, per-layer path
    (2000, 256, 1, 100, {}, lambda net: net.d.L == 1 and _rows_forward(net), True),          # rows forward + loc_head_eval loop
    (2000, 128, 4, 100, {}, lambda net: net.d.Hp == 128 and _rows_forward(net), True),      # rows forward, width 128
    (2000, 512, 4, 100, {"predict_pieces": 2}, lambda net: net.d.Hp == 512 and _rows_forward(net), False),  # rows forward,
    #                                                                     width 512: two bf16 pieces (three do not fit the LDS)
    (2000, 256, 4, 1200, {"predict_digits": -1}, lambda net: net._image_mode == 3, True),   # bf16 x 3 pieces image + GEMM
    (2000, 256, 4, 640, {"predict_digits": 3}, lambda net: net._image_mode == 13, True),    # int8, three planes
    (2000, 256, 4, 640, {"predict_digits": 2}, lambda net: net._image_mode == 12, False),   # int8, two planes
    (300, 256, 2, 16385, {"predict_digits": 3}, lambda net: net._image_mode == 13, True),   # LOC_PREDICT_CHUNK + 1 rows, one call
], ids=["fused-le32", "per-layer-le32", "nlayers1-head-loop", "rows-width128", "rows-width512", "bf16-3-pieces",
        "int8-3-planes", "int8-2-planes", "chunk-plus-1"])
def test_every_predict_route_at_q_up_to_126(K, width, nlayers, n, kw, route, exact):
    net, got, ref = _predict_case(K, width, nlayers, n, seed=n + width, **kw)
    assert route(net), (net._image_mode, net.d.Hp, net.use_fused)
    err = np.abs(got - ref).max()
    if exact:
        assert err < 2e-5, err
    assert err / np.abs(ref).max() < 1e-3, (err, np.abs(ref).max())
    assert np.isfinite(got).all()


# ------------------------------------------------------------------ 4. the int8 overflow bound, worst case
G8_HP, G8_TILE = 256, 16384
LIM3 = 8355711                   # 127 (256^3 - 1) / 255: the largest |q| three signed base-256 digits carry


def _worst_case(x_max, Kp, n, seed):
    """n rows over K = Kp SNPs: rows 32.. all at x_max, rows 0..15 uniform over 0..x_max, rows 16..31 at x_max with 10 %
    zeros.  BatchNorm: gamma 1, beta 0, mov_mean 0 and the q-unit variance 3.999f, so that var + BN_EPS = 4 in fp32 and
    the scale is exactly 0.5; W1[k][h] = 2 T_h for every SNP, T_h = +-(LIM3 - 1) 2^e_h: w' = s_k W1[k][h] = T_h exactly,
    every digit of every SNP of unit h +-(127, 127, 126), the largest the image allows (|q| = LIM3 would move delta_h up
    a binade).  e_h puts |z| of an all-x_max row between 0.25 and 4."""
    from locator_amd.net import LocatorNet, upload_genotypes
    rng = np.random.default_rng(seed)
    K = Kp
    q = np.full((n, K), x_max, np.uint8)
    q[:16] = rng.integers(0, x_max + 1, (16, K), dtype=np.uint8)
    q[16:32][rng.random((16, K)) < 0.1] = 0
    width, nlayers = 256, 2
    p = O.init_params(32, width, nlayers, rng)
    sign = np.where(np.arange(width) % 2 == 0, 1.0, -1.0)
    e = np.floor(np.log2(2.0 / (x_max * K * (LIM3 - 1.0)))).astype(int) + 1 - (np.arange(width) % 3)
    T = sign * (LIM3 - 1.0) * np.exp2(e)
    p["W"][0] = np.broadcast_to((2.0 * T).astype(np.float32), (K, width))
    p["b"][0] = rng.normal(0, 0.1, width)
    p["gamma"], p["beta"], p["mov_mean"] = np.ones(K), np.zeros(K), np.zeros(K)
    X = upload_genotypes(q)
    Y = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
    net = LocatorNet(X, Y, K, width, nlayers, 0.25, seed=1, unit=U)
    var_q = np.float32(3.999)
    assert np.float32(var_q + np.float32(O.BN_EPS)) == np.float32(4.0)
    p["mov_var"] = np.full(K, (np.float64(var_q) - np.float64(np.float32(net.var_add))) / U ** 2)
    net.import_params(O.cast_params(p, np.float32))
    net.params[net.lay.mov_var:net.lay.mov_var + K] = float(var_q)       # the q-unit variance, exactly
    net.params_changed()
    bn4 = _bn4_of(net)
    assert (bn4[:K] == np.float32(0.5)).all() and not bn4[Kp:Kp + K].any()     # scale exactly 0.5, shift 0
    return net, q, p, T


def _digit_planes(net, digits=3):
    """[plane][SNP][unit] int8 digits and delta[unit] of the kept int8 image (l1_gemm_i8.hip's layout, as
    test_gpu_gemm_i8.decode_image reads it)."""
    d, lib = net.d, net.lib
    nkt = ((d.Kp + 63) // 64 + 1) & ~1
    off = int(lib.loc_l1_image_i8_tiles_offset(C.byref(d)))
    raw = net.l1_image[off:off + nkt * digits * G8_TILE].cpu().numpy().view(np.int8)
    delta = net.l1_image[8 * G8_HP * 4:9 * G8_HP * 4].cpu().numpy().view(np.float32)
    t = raw.reshape(nkt, digits, 4, G8_HP, 16).transpose(1, 0, 2, 4, 3)       # [plane][block][chunk][SNP][unit]
    return t.reshape(digits, nkt * 64, G8_HP), delta


@pytest.mark.parametrize("x_max,Kp,i8", [(126, 132_896, True), (126, 132_928, False),
                                         (127, 131_840, True), (127, 131_872, False)],
                         ids=["q126-Kp132896-int8", "q126-Kp132928-bf16", "q127-Kp131840-int8", "q127-Kp131872-bf16"])
def test_int8_overflow_bound_with_the_worst_case_digits(x_max, Kp, i8):
    """loc_predict takes the int8 pipe only while x_max 128 (Kp + 256) < 2^31 (one SNP group may span the whole K range):
    the last Kp inside takes it (mode 13), the first one outside takes bf16 pieces (mode 3).  The data drive every digit
    plane to the end of its range for every SNP, with one sign per unit.  Predictions on both sides within 10x the fp32
    oracle's own distance from float64; on the int8 side also the GEMM forced into ONE SNP group, whose top-plane i32
    sums then reach x_max * 127 * K = 99 % of 2^31, against float64."""
    n = 640 if i8 else 1152                  # bf16 pieces x 3 start at LOC_GEMM_MIN_ROWS(3) = 1152 rows
    net, q, p, T = _worst_case(x_max, Kp, n, seed=Kp)
    K = Kp
    assert net.d.Kp == Kp and net.genotype_max() == x_max
    yhat = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
    net.predict_rows(torch.arange(n, dtype=torch.int32, device="cuda"), n, yhat)
    _sync()
    got = yhat.cpu().numpy()
    if i8:
        assert net._image_mode == 13, net._image_mode
        planes, delta = _digit_planes(net)
        assert np.array_equal(delta, np.abs(T / (LIM3 - 1)).astype(np.float32))
        for pl, want in enumerate((127, 127, 126)):
            assert np.array_equal(planes[pl, :K], np.broadcast_to((np.sign(T) * want).astype(np.int8), (K, G8_HP))), pl
            assert not planes[pl, K:].any()
    else:
        assert 1 <= net._image_mode <= 3, net._image_mode
    # the oracle on the distinct rows only: rows 32.. are all x_max
    uniq = np.arange(33)
    assert np.array_equal(got[33:], np.broadcast_to(got[32], got[33:].shape))
    xd = q[uniq].astype(np.float64) / U
    p64 = O.cast_params(O.cast_params(p, np.float32), np.float64)
    ref = O.predict(p64, xd)
    floor = np.abs(O.predict(O.cast_params(p, np.float32), xd.astype(np.float32)).astype(np.float64) - ref).max()
    err = np.abs(got[uniq] - ref).max()
    print(f"x_max {x_max} Kp {Kp}: mode {net._image_mode}, max |err| {err:.3e}, fp32 oracle {floor:.3e}, "
          f"|yhat| <= {np.abs(ref).max():.3f}")
    assert err <= 10 * floor + 1e-5, (err, floor)
    if i8:
        # ONE SNP group (target_blocks = row tiles): the kernel's own bound, x_max 128 SNPs per group < 2^31, holds here
        from tests.test_gpu_gemm_i8 import run_gemm_i8
        rows = torch.arange(n, dtype=torch.int32, device="cuda")
        a1 = run_gemm_i8(net, rows, n, 3, x_max=x_max, target_blocks=(n + 127) // 128, image=net.l1_image)
        z = q[uniq].astype(np.float64).sum(1)[:, None] * T[None, :] + p64["b"][0]
        want = np.where(z > 0, z, np.expm1(np.minimum(z, 0)))
        assert maxerr(a1[uniq], want) < 2e-5 * max(1.0, np.abs(z).max()), maxerr(a1[uniq], want)
        assert np.array_equal(a1[33:n], np.broadcast_to(a1[32], a1[33:n].shape))


# ------------------------------------------------------------------ 5. BatchNorm numerators at their limits
@pytest.mark.parametrize("unit,batch", [(1, 200), (1, 4096), (63, 32), (63, 4096)])
def test_bn_numerators_at_their_limits(unit, batch):
    """unit 1 with bytes up to 255 from 182 rows on, where n sum(x^2) passes 2^31 (l1_kernels.hip: the 64-bit numerator),
    and a 0 / top column whose exact numerator n^2 var passes 2^32 at 4096 rows; a column one below the top in a single
    row, the smallest non-zero variance there is: var' keeps it above the compensation term, and the rstd every reader
    derives from var' (bn4 of step 0) is rstd_d / unit."""
    from locator_amd.net import LocatorNet, upload_genotypes
    rng = np.random.default_rng(batch + unit)
    top = 255 if unit == 1 else 2 * unit
    n, K = 4100, 96
    perm = rng.permutation(n).astype(np.int32)
    q = rng.integers(0, top + 1, (n, K)).astype(np.uint8)
    q[:, 3] = top
    q[:, 5] = np.where(np.arange(n) % 2 == 0, 0, top)
    q[:, 7] = top
    q[perm[0], 7] = top - 1                             # in step 0
    X = upload_genotypes(q)
    Y = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
    net = LocatorNet(X, Y, K, 64, 4, 0.0, seed=1, unit=unit)
    steps = -(-n // batch)
    rows = np.zeros(steps * batch, np.int32)
    rows[:n] = perm
    stats = torch.zeros(steps * 2 * net.d.Kp, dtype=torch.float32, device="cuda")
    net.epoch_bn_stats(torch.from_numpy(rows).cuda(), batch, n - (steps - 1) * batch, steps, stats)
    _sync()
    Kp = net.d.Kp
    st = stats.cpu().numpy().reshape(steps, 2, Kp)[:, :, :K]
    c = np.float32(net.var_add)
    assert c == (0 if unit == 1 else np.float32(np.float32(unit * unit - 1) * np.float32(O.BN_EPS)))
    mm, mv = np.zeros(K), np.ones(K)
    for s in range(steps):
        xq = q[perm[s * batch:(s + 1) * batch]].astype(np.int64)
        nb = xq.shape[0]
        mean, var = (xq / unit).mean(0), (xq / unit).var(0)
        num = nb * (xq * xq).sum(0) - xq.sum(0) ** 2    # the exact integer numerator of var_q
        assert np.abs(st[s, 0] / unit - mean).max() < 1e-6 * max(1.0, np.abs(mean).max())
        assert np.abs((st[s, 1].astype(np.float64) - c) / unit ** 2 - var).max() < 2e-6 * max(1.0, var.max()), s
        want = num / float(nb) ** 2 + float(c)          # var' = var_q + var_add: every entry within 2 fp32 ulps
        assert (np.abs(st[s, 1] - want) <= 2 * np.spacing(st[s, 1])).all(), s
        if s == 0:
            assert num[7] == nb - 1 and st[s, 1, 7] > c, st[s, 1, 7]
            assert nb < 182 or nb * (xq[:, 3] ** 2).sum() >= 2 ** 31
            assert nb < 4096 or num[5] >= 2 ** 32
        mm = mm * O.BN_MOMENTUM + mean * (1 - O.BN_MOMENTUM)
        mv = mv * O.BN_MOMENTUM + var * (1 - O.BN_MOMENTUM)
    # what the readers take from var': step 0's bn4 (it leads the workspace) - rstd in q units = rstd_d / unit
    bn4 = net.ws[:4 * Kp].cpu().numpy().reshape(4, Kp)[:, :K]
    rstd_d = 1.0 / np.sqrt((q[perm[:batch]].astype(np.float64) / unit).var(0) + O.BN_EPS)
    assert np.abs(bn4[3].astype(np.float64) * unit / rstd_d - 1).max() < 2e-6
    assert np.abs(bn4[3] * np.sqrt(st[0, 1].astype(np.float64) + np.float32(O.BN_EPS)) - 1).max() < 3e-7
    assert np.array_equal(bn4[2], st[0, 0])
    p = net.export_params()                             # back in dosage units
    assert np.abs(p["mov_mean"] - mm).max() < 2e-6 * max(1.0, np.abs(mm).max())
    assert np.abs(p["mov_var"] - mv).max() < 2e-5 * max(1.0, np.abs(mv).max())


# ------------------------------------------------------------------ 6. --dosage --jacknife against the oracle
def test_dosage_jacknife_is_one_int8_predict_that_matches_the_oracle(tmp_path, monkeypatch):
    """The nboots perturbed copies of the prediction rows (12 x 50 = 600 rows: the int8 pipe, q <= 126) go through one
    many-row predict.  The redrawn sites hold 63 Binomial(2, af) - only 0, 63, 126 - every other site the sample's own
    q; every {out}_boot{b}_predlocs.txt equals oracle.predict on stacked / 63 with the weights the run kept (2e-5 on
    z-scored outputs, scaled to map units: test_gpu_cli's bar in exact mode)."""
    c, samples, pos = golden_counts()
    vcf = str(tmp_path / "d.vcf.gz")
    write_dosage_vcf(vcf, noisy_dosage(c[:3000], missing=0.01), samples, pos[:3000])
    recorded = {}
    real_draws, real_predict = L.jacknife_draws, L.Model.predict

    def spy_draws(predgen, af, nboots, prop, ploidy=2):
        recorded["predgen"] = np.array(predgen)
        recorded["draws"] = real_draws(predgen, af, nboots, prop, ploidy)
        return recorded["draws"]

    def spy_predict(self, gen):
        out = real_predict(self, gen)
        recorded.setdefault("calls", []).append((np.array(gen), self.net._image_mode, self.net.genotype_max()))
        return out
    monkeypatch.setattr(L, "jacknife_draws", spy_draws)
    monkeypatch.setattr(L.Model, "predict", spy_predict)
    out = str(tmp_path / "j")
    nboots = 12
    np.random.seed(None)
    assert L.main(["--vcf", vcf, "--dosage", "--sample_data", SAMPLES, "--out", out, "--seed", "7", "--jacknife",
                   "--nboots", str(nboots), "--max_epochs", "3", "--patience", "3", "--keras_verbose", "0",
                   "--keep_weights", "--plot_history", "", "--predict_mode", "exact"]) == 0
    stacked, mode, xmax = recorded["calls"][-1]
    base = recorded["predgen"]
    n_pred = base.shape[0]
    assert n_pred == 50 and stacked.shape == (nboots * n_pred, base.shape[1])
    assert mode == 13 and xmax <= 2 * U                      # ONE predict, on the int8 pipe (three planes)
    for b in range(nboots):
        sites, vals = recorded["draws"][b]
        blk = stacked[b * n_pred:(b + 1) * n_pred]
        assert set(np.unique(blk[:, sites])) <= {0, U, 2 * U}
        assert np.array_equal(blk[:, sites], (vals * U).T)
        rest = np.setdiff1d(np.arange(base.shape[1]), sites)
        assert np.array_equal(blk[:, rest], base[:, rest])
    p = O.cast_params(L.read_weights(out + "_bootFULL.weights.npz"), np.float64)
    z = O.predict(p, stacked.astype(np.float64) / U)
    sd = pd.read_csv(SAMPLES, sep="\t")
    mx, sx, my, sy = sd["x"].mean(), sd["x"].std(ddof=0), sd["y"].mean(), sd["y"].std(ddof=0)
    for b in range(nboots):
        got = pd.read_csv(f"{out}_boot{b}_predlocs.txt")
        zb = z[b * n_pred:(b + 1) * n_pred]
        assert np.abs(got["x"].to_numpy() - (zb[:, 0] * sx + mx)).max() < 2e-5 * sx + 1e-9, b
        assert np.abs(got["y"].to_numpy() - (zb[:, 1] * sy + my)).max() < 2e-5 * sy + 1e-9, b
