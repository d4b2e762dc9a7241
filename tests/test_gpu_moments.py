"""Adam's moments after one epoch on every training schedule, against the oracle.

The other schedule tests look at the weights after Adam (5e-4 on epoch losses, 1e-4 on weights, three epochs).  Adam
divides the gradient by its own running magnitude, so a gradient that is too large or too small by a constant factor
moves the weights almost exactly as the right one does: every gradient x 0.9 changes them by 3e-5 to 5e-5 in those
tests, gamma and beta x 2 by 7e-5.  The moments hold the magnitude itself - m = 0.1 g and
v = 0.001 g^2 after the first step - and the same errors put them off by a relative 0.1 to 1.0
(tests/test_oracle.py::test_moments_see_a_ten_percent_gradient_error).

Each case runs ONE epoch on one route of train_step_impl (asserted), reads the device's dropout masks back and replays the
same minibatches through the oracle in float64 and in float32.  The fp32 replay's distance from the float64 one is the
floor: F = its largest per-tensor relative L2 error over both moments, F_tile the same over the 32 x 32 tiles of the
kernels (tests/gpu_util.moments_err).  The device may be MARGIN times as far, and never more than 1e-3."""
import numpy as np
import pytest
import torch

from tests.gpu_util import (build_net, make_problem, moments_err, moments_padding, replay_epoch, tile_norms)
from tests.test_gpu_dosage_paths import (_route_chain, _route_dr, _route_in_dropout, _route_per_layer, _route_row_blocks,
                                         _route_two_block_chain)

pytestmark = pytest.mark.gpu

# The device over the fp32 oracle's own distance from float64: it sums in another order and uses the hardware's exp.  10
# is the factor test_gpu_parity.py::test_one_training_step_matches_oracle gives the device over the same floor; every
# case prints its ratios device / F and device / F_tile (pytest -s), from which the margin is to be set at about twice
# the largest one measured.
MARGIN = 10.0
CAP = 1e-3                      # no bar above this, whatever the margin: 100 x below the 10 % the suite let through


def _both(*preds):
    return lambda net, r: all(p(net, r) for p in preds)


def _tuned(**kw):
    return lambda net, r: all(getattr(net.tuning, k) == v for k, v in kw.items())


def _width_256(net, r):
    return net.d.Hp == 256


CASES = [
    # K, width, nlayers, batch, n_train, chain, tuning, route                                          steps of
    (300, 64, 4, 32, 70, False, None, _route_row_blocks(32)),                                        # 32, 32, 6
    (5830, 256, 10, 32, 58, False, None, _both(_route_row_blocks(32), _width_256)),                  # 32, 26
    (5830, 256, 10, 32, 58, False, {"l1b_rows": 1},
     _both(_route_row_blocks(32), _width_256, _tuned(l1b_rows=1))),                                  # 32, 26
    (600, 256, 4, 32, 70, True, None, _both(_route_chain(256), _tuned(chain_tail=0))),               # 32, 32, 6
    (600, 256, 4, 32, 70, True, {"chain_tail": -1}, _both(_route_chain(256), _tuned(chain_tail=-1))),
    (400, 128, 4, 32, 70, True, None, _route_chain(128)),                                            # 32, 32, 6
    (500, 512, 4, 32, 70, True, None, _route_chain(512)),                                            # 32, 32, 6
    (257, 33, 5, 16, 33, True, None, _route_chain(64, 288)),                                         # 16, 16, 1
    (600, 256, 4, 48, 130, None, None, _route_two_block_chain),                                      # 48, 48, 34
    (1000, 128, 6, 33, 100, None, None, _route_row_blocks(64)),                                      # 33, 33, 33, 1
    (400, 64, 6, 96, 200, None, None, _route_row_blocks(128)),                                       # 96, 96, 8
    (2048, 128, 4, 100, 230, None, None, _route_row_blocks(128)),                                    # 100, 100, 30
    (900, 256, 4, 128, 300, None, None, _both(_route_row_blocks(128), _width_256)),                  # 128, 128, 44
    (700, 256, 10, 129, 400, None, None, _route_row_blocks(256)),                                    # 129 x 3, 13
    (300, 64, 4, 200, 450, None, None, _route_row_blocks(256)),                                      # 200, 200, 50
    (500, 128, 4, 300, 700, None, None, _route_row_blocks(384)),                                     # 300, 300, 100
    (400, 128, 4, 1000, 2300, None, None, _route_row_blocks(1024)),                                  # 1000, 1000, 300
    (300, 64, 4, 1024, 2100, None, None, _route_row_blocks(1024)),                                   # 1024, 1024, 52
    (500, 256, 4, 4096, 4200, None, None, _route_row_blocks(4096)),                                  # 4096 (the limit), 104
    (300, 64, 1, 32, 70, None, None, _route_in_dropout),                                             # 32, 32, 6
    (97, 33, 1, 7, 30, None, None, _route_in_dropout),                                               # 7 x 4, 2
    (400, 128, 2, 32, 80, None, None, _route_dr(True)),                                              # 32, 32, 16
    (400, 256, 3, 32, 80, False, None, _route_dr(False)),                                            # 32, 32, 16
    (300, 96, 4, 32, 70, None, None, _route_per_layer(96)),                                          # 32, 32, 6
    (20, 8, 2, 32, 50, None, None, _route_per_layer(32)),                                            # 32, 18
    (300, 600, 3, 32, 70, None, None, _route_per_layer(608)),                                        # 32, 32, 6
    (97, 1024, 2, 16, 40, None, None, _route_per_layer(1024)),                                       # 16, 16, 8
]
IDS = ["unchained-32", "width256-nt-streams", "width256-l1b-rows", "chain-tail-merged", "chain-tail-own-launch",
       "chain-width128", "chain-width512", "chain-padded-K257-w33", "two-block-chain", "batch33-row-blocks",
       "batch96-row-blocks", "batch100-row-blocks", "batch128-width256", "batch129-big-batch", "batch200-big-batch",
       "batch300-big-batch", "batch1000-big-batch", "batch1024-big-batch", "batch4096-the-limit", "nlayers1-in-dropout", "nlayers1-K97-batch7", "nlayers2-dropout-after-l1-chained",
       "nlayers3-dropout-after-l1-unchained", "width96-per-layer", "width8-K20-per-layer", "width600-per-layer",
       "width1024-per-layer"]


@pytest.mark.parametrize("K,width,nlayers,batch,n_train,chain,tuning,route", CASES, ids=IDS)
def test_moments_after_one_epoch_match_the_oracle(K, width, nlayers, batch, n_train, chain, tuning, route):
    """One epoch; m and v of every tensor and of every 32 x 32 tile of every kernel within MARGIN x the fp32 oracle's own
    error (and within 1e-3), the padding of the flat moment buffers exactly zero, every step's loss within 2e-5."""
    from locator_amd.train import EpochRunner
    n_val = 9
    x, y, p, _ = make_problem(n_train + n_val, K, width, nlayers, seed=K + width)
    tr, va = np.arange(n_train), np.arange(n_train, n_train + n_val)
    net = build_net(x, y, p, drop_p=0.25, seed=5, tuning=tuning)
    runner = EpochRunner(net, tr, va, batch, use_graph=True, chain=chain)
    assert route(net, runner), (net.d.Hp, net.d.Kp, net.use_fused, runner.chain, runner.slot_rows)
    perm = np.random.default_rng(0).permutation(n_train)
    runner.run_epoch(perm)
    steps = runner.steps
    assert steps == -(-n_train // batch)
    masks = runner.masks.cpu().numpy().reshape(steps, runner.slot_rows, net.mask_width)
    losses = runner.stats_host.numpy()[:steps].astype(np.float64)
    gm, gv = net.export_adam()

    kw = dict(x=x, y=y, rows=tr[perm], batch=batch, masks=masks, drop_p=0.25)
    l64, m64, v64 = replay_epoch(p, **kw)
    _, m32, v32 = replay_epoch(p, dtype=np.float32, **kw)

    # no tile inside K x H without a gradient: x_hat = gamma xn + beta is never all zero
    for ref in (m64, v64):
        for l, w in enumerate(ref["W"]):
            assert (tile_norms(w) > 0).all(), l
    floors = [moments_err(a, b) for a, b in ((m32, m64), (v32, v64))]
    F = max(max(t.values()) for t, _ in floors)
    F_tile = max(max(tt.values()) for _, tt in floors)
    assert 0 < F and MARGIN * F < CAP, F
    assert 0 < F_tile and MARGIN * F_tile < CAP, F_tile

    worst, worst_tile = {}, {}
    for name, got, ref in (("m", gm, m64), ("v", gv, v64)):
        t, tt = moments_err(got, ref)
        worst.update({f"{name}.{k}": e for k, e in t.items()})
        worst_tile.update({f"{name}.{k}": e for k, e in tt.items()})
    kt, kk = max(worst, key=worst.get), max(worst_tile, key=worst_tile.get)
    dl = np.abs(losses - l64).max()
    print(f"moments K {K} width {width} L {nlayers} batch {batch} chain {runner.chain} tuning {tuning}: "
          f"F {F:.2e} device {worst[kt]:.2e} ({kt}) ratio {worst[kt] / F:.2f} | "
          f"F_tile {F_tile:.2e} device {worst_tile[kk]:.2e} ({kk}) ratio {worst_tile[kk] / F_tile:.2f} | "
          f"loss {dl:.1e}")
    assert worst[kt] <= MARGIN * F, (kt, worst[kt], F, worst)
    assert worst_tile[kk] <= MARGIN * F_tile, (kk, worst_tile[kk], F_tile, worst_tile)
    assert dl < 2e-5, (losses, l64)
    for flat in (net.adam_m, net.adam_v):
        assert not moments_padding(net, flat).any()
