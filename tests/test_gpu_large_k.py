"""Layer-1 kernels at their 32-bit offset limits: training and predict at 2.1 to 4.2 million SNPs against the fp64 oracle.

The rest of the suite stops at 500,000 SNPs, where byte offsets into W1 / m / v reach about 2^29.  A whole-chromosome VCF
without --max_SNPs gives millions.  Here the problems have sparse support (tests/gpu_util.py, sparse_problem): a handful
of 32-SNP k-tiles hold real genotypes and keep the device's glorot W1 rows, every other SNP column is constant with a
zero W1 row.  Such a problem trains exactly like the reduced problem made of its active columns
(tests/test_oracle.py::test_sparse_support_problem_trains_like_its_reduced_problem), so the oracle runs on a few hundred
SNPs while the device streams the full W1 / m / v.  The active tiles sit at tile 0, tile 1, both sides of every byte
offset 2^31 / 2^32 / 2^33 that W1 crosses, the tiles a 31- or 32-bit offset would alias them to, and the last tile; each
draws its own allele frequencies, so reading or writing the wrong tile changes the numbers.

Per case: one step (tolerances of tests/test_gpu_parity.py::test_one_training_step_matches_oracle), three epochs of three
minibatches, the last one short, from the captured graph (those of
tests/test_gpu_chain.py::test_chained_epochs_match_the_oracle_fit), everything outside the active tiles exactly where it
started over the whole Kp range, and predict in every many-row mode the width has (PREDICT_MODES of
tests/test_gpu_baseline_sizes.py).  Each case asserts which schedule ran: the chained kernel addresses W1 / m / v through
32-bit byte offsets and takes Kp * max(Hp, 256) * 4 < 2^32 only.  Peak device memory 9 to 35 GB per case.
"""
import gc
import time

import numpy as np
import pytest
import torch

from oracle import locator_oracle as O
from tests.gpu_util import (export_reduced, keep_w1_tiles, maxerr, params_err, read_w1_tiles, sparse_problem,
                            untouched)

pytestmark = pytest.mark.gpu

NLAYERS, DROP, N_VAL, N_PRED = 4, 0.25, 20, 10

CASES = {   # width, SNPs, --batch_size, chained schedule
    "A": (512, 2_098_000, 32, False),      # the chain's 2^32-byte offset at width 512 (last tile half full)
    "B32": (256, 4_194_240, 32, True),     # the last Kp the chain accepts at width 256
    "B48": (256, 4_194_240, 48, True),     # ... with two 32-row blocks per step
    "C": (256, 4_194_321, 32, False),      # the first Kp the chain refuses; int8 / bf16 predict images past 2^32 bytes
    "D": (512, 4_194_321, 32, False),      # Kp * Hp >= 2^31 elements
    "E128": (128, 4_194_240, 32, True),    # narrow widths at their largest K
    "E64": (64, 4_194_321, 32, False),
}


def active_tiles(K, Hp):
    """Tiles 0 and 1, the last tile, both sides of each byte offset 2^31 / 2^32 / 2^33 of W1S that the net crosses, and the
    tiles every one of them aliases to modulo 2^31 and 2^32 bytes."""
    nkt, tb = (K + 31) // 32, 32 * Hp * 4
    tiles = {0, 1, nkt - 1}
    for b in (1 << 31, 1 << 32, 1 << 33):
        if b // tb < nkt:
            tiles |= {b // tb - 1, b // tb}
    for kt in list(tiles):
        tiles |= {kt * tb % (1 << 31) // tb, kt * tb % (1 << 32) // tb}
    return sorted(tiles)


def _masks(runner, width):
    return runner.masks.cpu().numpy().reshape(runner.steps, runner.slot_rows, runner.net.d.Hp)[:, :, :width].copy()


def _check_outside(net, tiles, cols, const, steps):
    """Everything outside the active tiles is exactly where it started (zero W1 / m / v, gamma 1, beta 0, their moments 0),
    the padded SNPs K..Kp are zero, and the moving statistics of the constant columns follow c (1 - 0.99^s), 0.99^s."""
    d, lay = net.d, net.lay
    P, M, V = net.params, net.adam_m, net.adam_v
    n_w1 = d.Kp * d.Hp
    for name, flat in (("W1", P), ("m", M), ("v", V)):
        assert untouched(flat[lay.w1:lay.w1 + n_w1], tiles, 0.0, 32 * d.Hp) == 0, name
    sec = lambda flat, off: flat[off:off + d.Kp]
    assert untouched(sec(P, lay.gamma), tiles, 1.0, 32) == 0
    for flat in (P, M, V):
        assert untouched(sec(flat, lay.beta), tiles, 0.0, 32) == 0
    for flat in (M, V):
        assert untouched(sec(flat, lay.gamma), tiles, 0.0, 32) == 0
    # padded SNPs of the (active) last tile
    last, pad = d.Kp // 32 - 1, d.K - 32 * (d.Kp // 32 - 1)
    for flat in (P, M, V):
        assert not read_w1_tiles(flat, lay, [last], d.Hp)[pad:].any()
        assert not flat[lay.gamma + d.K:lay.gamma + d.Kp].any() and not flat[lay.beta + d.K:lay.beta + d.Kp].any()
    mm = sec(P, lay.mov_mean)
    assert untouched(mm, sorted(set(tiles) | set(const)), 0.0, 32) == 0
    worst = 0.0
    for kt, c in const.items():
        got = mm[32 * kt:32 * kt + 32].cpu().numpy().astype(np.float64)
        worst = max(worst, float(np.abs(got - c * (1 - 0.99 ** steps)).max()))
    assert worst < 1e-6, worst
    assert untouched(sec(P, lay.mov_var), tiles, 0.99 ** steps, 32, atol=1e-6) == 0
    return worst


def _predict_checks(net, xr, y, pw, width, report):
    """Many-row predicts in every mode the width has, against oracle.predict on the reduced problem with the device's
    weights; a few distinct rows repeated up to the mode's row threshold."""
    from tests.test_gpu_baseline_sizes import NORTH_STAR_REL, PREDICT_MODES
    n = xr.shape[0]
    modes = {k: v for k, v in PREDICT_MODES.items() if net.lib.loc_l1_gemm_supported(net.d.Hp, 3)}
    modes["rows"] = ({"predict_digits": 3, "predict_pieces": 3}, 2e-5, 200)   # below every image threshold at 256
    for mode, (kw, tol_abs, min_rows) in modes.items():
        net.predict_digits, net.predict_pieces = kw["predict_digits"], kw.get("predict_pieces", 3)
        net.params_changed()
        net._net = None
        rows = np.resize(np.arange(n), min_rows)
        yhat, dist = torch.zeros((min_rows, 2), device="cuda"), torch.zeros(min_rows, device="cuda")
        # three digit planes are refused by the dynamic-range guard on these weights (a unit's largest weight over the
        # mean magnitude of millions of zeros): the validation sweep's unguarded form (in_fit) takes them as asked
        net.predict_rows(torch.from_numpy(rows.astype(np.int32)).cuda(), min_rows, yhat, dist, in_fit=(mode == "int8x3"))
        torch.cuda.synchronize()
        want = {"int8x3": 13, "int8x2": 12, "bf16x3": 3, "bf16x2": 2, "bf16x1": 1, "rows": 0}[mode]
        assert net._image_mode == want, (mode, net._image_mode)
        ref = O.predict(pw, xr[rows])
        err = maxerr(yhat.cpu().numpy(), ref)
        rel = err / float(np.abs(ref).max())
        report[f"predict {mode} (mode {want})"] = (err, rel)
        if mode == "bf16x1":
            assert err < 2e-2, err
        else:
            assert rel <= NORTH_STAR_REL, (mode, err, rel)
        if tol_abs is not None:
            assert err < tol_abs, (mode, err)
            assert maxerr(dist.cpu().numpy(), O.euclid(ref, y[rows])) < tol_abs, mode
    net.predict_digits, net.predict_pieces = 3, 3
    net._net = None


def run_case(width, K, batch, chained, seed=1):
    """One large-K case; returns a dict of what ran and the worst errors."""
    from locator_amd.net import LocatorNet, upload_genotypes
    from locator_amd.train import EpochRunner
    t0 = time.time()
    torch.cuda.reset_peak_memory_stats()
    Hp = (width + 31) // 32 * 32
    tiles = active_tiles(K, Hp)
    n_train = 2 * batch + 16
    n = n_train + N_VAL + N_PRED
    x, y, cols, const = sparse_problem(K, width, NLAYERS, tiles, n, seed=seed + K % 1009)
    X = upload_genotypes(x)
    xr = np.ascontiguousarray(x[:, cols])
    del x
    Y = torch.from_numpy(y.astype(np.float32)).cuda()
    net = LocatorNet(X, Y, K, width, NLAYERS, DROP, seed=seed)
    tr, va, pr_rows = np.arange(n_train), np.arange(n_train, n_train + N_VAL), np.arange(n_train + N_VAL, n)
    report = {"case": (width, K, batch), "active tiles": tiles}

    # one step: an epoch of one minibatch
    keep_w1_tiles(net, tiles)
    p0 = O.cast_params(export_reduced(net, net.params, tiles, cols), np.float64)
    perm = np.random.default_rng(seed).permutation(batch)
    runner = EpochRunner(net, tr[:batch], va, batch, use_graph=True)
    assert runner.chain == chained, (runner.chain, chained)
    runner.run_epoch(perm)
    mask = _masks(runner, width)
    pr = O.copy_params(p0)
    m, v = O.zeros_like_trainable(pr), O.zeros_like_trainable(pr)
    O.train_step(pr, m, v, 1, 1e-3, xr[perm], y[perm], mask[0, :batch], DROP)
    errs = params_err(export_reduced(net, net.params, tiles, cols), pr)
    gm = export_reduced(net, net.adam_m, tiles, cols, with_moving=False)
    gv = export_reduced(net, net.adam_v, tiles, cols, with_moving=False)
    report["one step: weights"], report["one step: m"] = max(errs.values()), max(params_err(gm, m).values())
    assert max(errs.values()) < 1e-5, errs
    assert max(params_err(gm, m).values()) < 1e-6
    for l in range(len(v["W"])):
        np.testing.assert_allclose(gv["W"][l], v["W"][l], rtol=2e-3, atol=1e-12)
    np.testing.assert_allclose(gv["gamma"], v["gamma"], rtol=2e-3, atol=1e-12)
    np.testing.assert_allclose(gv["beta"], v["beta"], rtol=2e-3, atol=1e-12)
    _check_outside(net, tiles, cols, const, 1)
    del runner

    # three epochs from the same start, epochs 1 and 2 replayed from the captured graph
    net.init_weights()
    keep_w1_tiles(net, tiles)
    assert params_err(O.cast_params(export_reduced(net, net.params, tiles, cols), np.float64), p0)["W0"] == 0.0
    runner = EpochRunner(net, tr, va, batch, use_graph=True)
    assert runner.chain == chained and runner.steps == 3 and runner.step_sizes[-1] == 16
    perms = [np.random.default_rng(100 * seed + e).permutation(n_train) for e in range(3)]
    hist, masks = [], []
    for e in range(3):
        hist.append(runner.run_epoch(perms[e]))
        masks.append(_masks(runner, width))
    assert runner.graph is not None
    report["schedule"] = "chained" if runner.chain else "unchained"
    pref = O.copy_params(p0)
    href, _ = O.fit(pref, xr[tr], y[tr], xr[va], y[va], batch_size=batch, max_epochs=3, patience=100, drop_p=DROP,
                    perm_fn=lambda e: perms[e], mask_fn=lambda e, s, nb: masks[e][s, :nb])
    report["fit: loss"] = maxerr([h[0] for h in hist], href["loss"])
    report["fit: val_loss"] = maxerr([h[1] for h in hist], href["val_loss"])
    pw = O.cast_params(export_reduced(net, net.params, tiles, cols), np.float64)
    err = params_err(pw, pref)
    report["fit: weights"] = max(err.values())
    assert report["fit: loss"] < 5e-4, (hist, href["loss"])
    assert report["fit: val_loss"] < 5e-4, (hist, href["val_loss"])
    assert max(err.values()) < 2e-4, err
    assert np.abs(pw["W"][0] - p0["W"][0]).max() > 1e-4       # the active tiles trained, the last one included
    assert np.abs(pw["W"][0][-16:] - p0["W"][0][-16:]).max() > 1e-5
    report["moving mean of the constant tiles"] = _check_outside(net, tiles, cols, const, 3 * runner.steps)
    del runner

    # predict: the fit's result on rows it never saw, then every many-row mode on the device's weights
    yhat = torch.zeros((N_PRED, 2), device="cuda")
    net.predict_rows(torch.from_numpy(pr_rows.astype(np.int32)).cuda(), N_PRED, yhat)
    torch.cuda.synchronize()
    ref = O.predict(pref, xr[pr_rows])
    report["predict after the fit (rel)"] = float((np.abs(yhat.cpu().numpy() - ref) / np.maximum(np.abs(ref), 1.0)).max())
    assert report["predict after the fit (rel)"] < 1e-3
    _predict_checks(net, xr, y, pw, width, report)
    torch.cuda.synchronize()
    report["peak device memory GB"] = torch.cuda.max_memory_allocated() / 1e9
    report["seconds"] = time.time() - t0
    return report


@pytest.fixture(autouse=True)
def _free_device_memory():
    yield
    gc.collect()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("case", list(CASES))
def test_large_k_sparse_support_matches_the_reduced_oracle(case):
    width, K, batch, chained = CASES[case]
    report = run_case(width, K, batch, chained)
    print(f"\nlarge-K case {case}: " + "; ".join(f"{k} {v:.3g}" if isinstance(v, float) else f"{k} {v}"
                                               for k, v in report.items()))
