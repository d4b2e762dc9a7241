"""Pins the CPU oracle (oracle/locator_oracle.py) with everything that can be
pinned without TensorFlow: NumPy known answers, an independent
torch-autograd float64 derivation of every gradient, hand-computed Adam / BN
values, and scripted callback traces."""
import hashlib

import numpy as np
import pytest
import torch

from oracle import locator_oracle as O


# ---------------------------------------------------------------- NumPy KATs
@pytest.mark.parametrize("seed,first10,sha,reseed,so8", [
    (12345, [465, 459, 233, 149, 429, 423, 454, 140, 489, 165], "144d3567059195b1", 812135,
     [1092, 5266, 5679, 4778, 3551, 2418, 1321, 5729]),
    (54321, [334, 260, 165, 112, 292, 283, 364, 87, 65, 82], "94c04ad6e4a776db", 429793,
     [367, 2699, 4649, 5250, 3196, 5447, 143, 2576]),
])
def test_numpy_rng_chain_known_answers(seed, first10, sha, reseed, so8):
    # fixture shape: 500 samples, first 50 NA, K=5830 after filters
    locs = np.random.default_rng(1).uniform(0, 50, (500, 2))
    locs[:50] = np.nan
    ac = np.zeros((5830, 500), np.int8)
    np.random.seed(seed)
    train, test, tg, vg, tl, vl, pred, pg = O.split_train_test(ac, locs, 0.9)
    assert list(test[:10]) == first10
    assert hashlib.sha1(test.astype("int64").tobytes()).hexdigest()[:16] == sha
    assert len(train) == 405 and len(test) == 45 and len(pred) == 50
    assert tg.shape == (405, 5830) and vg.shape == (45, 5830) and pg.shape == (50, 5830)
    assert np.all(np.diff(train) > 0)
    chain = O.bootstrap_chain(2, 5830)
    assert chain[0][0] == reseed
    assert list(chain[0][1][:8]) == so8


def test_normalize_locs():
    locs = np.array([[np.nan, np.nan], [1.0, 10.0], [3.0, 30.0], [5.0, 20.0]])
    ml, sl, ma, sa, out = O.normalize_locs(locs)
    assert ml == 3.0 and ma == 20.0
    assert np.isclose(sl, np.std([1, 3, 5])) and np.isclose(sa, np.std([10, 30, 20]))
    assert np.isnan(out[0]).all()
    assert np.allclose(out[1:, 0], (np.array([1, 3, 5]) - 3) / sl)


# ---------------------------------------------------------------- torch cross-check
def _torch_loss(p, x, y, mask, drop_p):
    """Independent derivation: torch ops + autograd, float64, Keras semantics by hand
    (nn.BatchNorm1d / torch Adam are NOT equivalent, so not used)."""
    tp = {k: ([torch.tensor(a, requires_grad=True) for a in v] if isinstance(v, list)
              else torch.tensor(v, requires_grad=k in ("gamma", "beta"))) for k, v in p.items()}
    xt = torch.tensor(x.astype(np.float64))
    mu = xt.mean(0)
    var = ((xt - mu) ** 2).mean(0)
    a = (xt - mu) / torch.sqrt(var + O.BN_EPS) * tp["gamma"] + tp["beta"]
    nl = len(p["W"]) - 2
    if O.n_pre(nl) == 0 and drop_p > 0:           # --nlayers 1: Dropout directly after the BatchNormalization
        a = a * torch.tensor(mask.astype(np.float64)) / (1 - drop_p)
    for l in range(nl):
        a = torch.nn.functional.elu(a @ tp["W"][l] + tp["b"][l])
        if l == O.n_pre(nl) - 1 and drop_p > 0:
            a = a * torch.tensor(mask.astype(np.float64)) / (1 - drop_p)
    y1 = a @ tp["W"][nl] + tp["b"][nl]
    y2 = y1 @ tp["W"][nl + 1] + tp["b"][nl + 1]
    loss = torch.sqrt(((y2 - torch.tensor(y)) ** 2).sum(-1)).mean()
    loss.backward()
    return loss.item(), tp, y2.detach().numpy()


@pytest.mark.parametrize("n,K,width,nlayers,drop_p", [
    (16, 64, 32, 10, 0.25), (7, 40, 16, 4, 0.5), (32, 128, 64, 3, 0.0), (5, 33, 8, 2, 0.25), (9, 48, 16, 1, 0.25),
    (6, 20, 8, 1, 0.0)])
def test_gradients_match_torch_autograd(n, K, width, nlayers, drop_p):
    rng = np.random.default_rng(7)
    p = O.init_params(K, width, nlayers, rng)
    p["gamma"] = rng.uniform(0.5, 1.5, K)
    p["beta"] = rng.normal(0, 0.1, K)
    for l in range(len(p["b"])):
        p["b"][l] = rng.normal(0, 0.1, p["b"][l].shape)
    x = rng.integers(0, 3, (n, K)).astype(np.uint8)
    y = rng.normal(0, 1, (n, 2))
    mask = (rng.random((n, width if O.n_pre(nlayers) > 0 else K)) >= drop_p).astype(np.uint8)
    loss, g, yhat = O.loss_and_grads(O.copy_params(p), x, y, mask, drop_p)
    tl, tp, ty = _torch_loss(p, x, y, mask, drop_p)
    assert abs(loss - tl) < 1e-12
    assert np.allclose(yhat, ty, atol=1e-12)
    assert np.allclose(g["gamma"], tp["gamma"].grad.numpy(), atol=1e-12)
    assert np.allclose(g["beta"], tp["beta"].grad.numpy(), atol=1e-12)
    for l in range(len(p["W"])):
        assert np.allclose(g["W"][l], tp["W"][l].grad.numpy(), atol=1e-12), l
        assert np.allclose(g["b"][l], tp["b"][l].grad.numpy(), atol=1e-12), l


def test_bn_training_uses_biased_variance_and_updates_moving_stats():
    p = O.init_params(3, 4, 2, np.random.default_rng(0))
    x = np.array([[0, 1, 2], [2, 1, 0], [2, 2, 0], [0, 0, 0]], np.uint8)
    _, c = O.forward(p, x, True, np.ones((4, 4)), 0.25)
    mu = x.astype(float).mean(0)
    var = x.astype(float).var(0)      # ddof=0
    assert np.allclose(c["mu"], mu) and np.allclose(c["var"], var)
    assert np.allclose(p["mov_mean"], 0.01 * mu)
    assert np.allclose(p["mov_var"], 0.99 + 0.01 * var)
    # inference uses moving stats and ignores dropout
    y_inf, _ = O.forward(p, x, False)
    xh = (x - p["mov_mean"]) / np.sqrt(p["mov_var"] + 1e-3)
    a = xh
    for l in range(2):
        a = O.elu(a @ p["W"][l] + p["b"][l])
    ref = (a @ p["W"][2] + p["b"][2]) @ p["W"][3] + p["b"][3]
    assert np.allclose(y_inf, ref)


def test_adam_keras_form_known_value():
    # one step, g=3e-6, eps=1e-7 -> w = 0.9995132 (Keras form), not torch's 0.9990323
    p = {"gamma": np.array([1.0]), "beta": np.array([0.0]), "W": [], "b": []}
    g = {"gamma": np.array([3e-6]), "beta": np.array([0.0]), "W": [], "b": []}
    m = {"gamma": np.zeros(1), "beta": np.zeros(1), "W": [], "b": []}
    v = {"gamma": np.zeros(1), "beta": np.zeros(1), "W": [], "b": []}
    O.adam_apply(p, g, m, v, 1, 1e-3)
    assert abs(p["gamma"][0] - 0.9995132) < 1e-6
    assert np.isclose(m["gamma"][0], 3e-7) and np.isclose(v["gamma"][0], 9e-15)
    assert p["beta"][0] == 0.0


def test_loss_zero_distance_has_zero_gradient():
    rng = np.random.default_rng(3)
    p = O.init_params(8, 4, 2, rng)
    x = rng.integers(0, 3, (4, 8))
    yhat, _ = O.forward(O.copy_params(p), x, True, np.ones((4, 4)), 0.0)
    y = yhat.copy()
    y[1:] += 1.0                       # sample 0 sits exactly on its target
    loss, g, _ = O.loss_and_grads(p, x, y, np.ones((4, 4)), 0.0)
    assert np.isfinite(loss) and all(np.isfinite(a).all() for a in g["W"])


# ---------------------------------------------------------------- callbacks
def test_callbacks_state_machines():
    cb = O.Callbacks(patience=12)        # lr patience int(12/6)=2
    vals = [1.0, 0.9, 0.95, 0.96, 0.97, 0.9, 0.8] + [0.85] * 12
    saves, stops, lrs = [], [], []
    for e, v in enumerate(vals):
        s, st, lr = cb.on_epoch_end(e, v)
        saves.append(s); stops.append(st); lrs.append(lr)
    assert saves[:7] == [True, True, False, False, False, False, True]   # tie at 0.9 does not save
    assert not any(saves[7:])
    # LR: epochs 2,3 non-improving -> halve after epoch 3; epoch 4,5 (0.9 is a tie => not improving) -> halve after 5
    assert np.allclose(lrs[:7], [1e-3, 1e-3, 1e-3, 1e-3, 5e-4, 5e-4, 2.5e-4], rtol=1e-6)
    assert lrs[0] == float(np.float32(1e-3))
    # early stop: best at epoch 6, 12 non-improving epochs -> stop at epoch 18
    assert stops.index(True) == 18 and len(vals) == 19


def test_fit_history_and_best_weights():
    rng = np.random.default_rng(11)
    K, n = 48, 40
    x = rng.integers(0, 3, (n, K)).astype(np.uint8)
    w = rng.normal(0, 1, (K, 2))
    y = (x - x.mean(0)) @ w
    y = (y - y.mean(0)) / y.std(0)
    p = O.init_params(K, 16, 4, rng)
    hist, best = O.fit(p, x[:32], y[:32], x[32:], y[32:], batch_size=10, max_epochs=30, patience=6)
    ne = len(hist["loss"])
    assert ne == len(hist["val_loss"]) == len(hist["learning_rate"]) and 2 <= ne <= 30
    assert hist["loss"][-1] < hist["loss"][0]
    # best weights reproduce the minimum val_loss
    val = O.euclid(O.predict(best, x[32:]), y[32:]).mean()
    assert np.isclose(val, min(hist["val_loss"]))
    # partial last batch kept: 32 rows / 10 -> 4 steps/epoch (checked through Adam's t via determinism)
    p2 = O.init_params(K, 16, 4, np.random.default_rng(11))


def test_fp32_oracle_tracks_fp64():
    rng = np.random.default_rng(5)
    K, n, width = 256, 32, 32
    p = O.init_params(K, width, 4, rng)
    x = rng.integers(0, 3, (n, K)).astype(np.uint8)
    y = rng.normal(0, 1, (n, 2))
    mask = (rng.random((n, width)) >= 0.25)
    l64, g64, _ = O.loss_and_grads(O.copy_params(p), x, y, mask)
    l32, g32, _ = O.loss_and_grads(O.cast_params(p, np.float32), x, y, mask)
    assert abs(l64 - l32) < 1e-5
    assert np.allclose(g64["W"][0], g32["W"][0], atol=2e-6)


def test_torch_cpu_restatement_matches_the_numpy_oracle():
    """oracle/torch_cpu.py (the multi-threaded torch-CPU fp32 restatement timed as bench.py's cpu_baseline) against
    the fp64 NumPy oracle: 2 epochs with the same permutations and dropout masks, a partial last batch, and the
    validation sweep.  fp32 vs fp64: losses 1e-4, weights 5e-5."""
    import torch
    from oracle.torch_cpu import TorchCpuLocator
    rng = np.random.default_rng(5)
    n, K, H, L = 75, 300, 32, 4
    x = rng.integers(0, 3, (n, K)).astype(np.uint8)
    y = rng.normal(0, 1, (n, 2))
    p = O.init_params(K, H, L, rng)
    p["gamma"] = rng.uniform(0.7, 1.3, K)
    p["mov_mean"] = rng.uniform(0, 1, K)
    tr, va = np.arange(60), np.arange(60, 75)
    perms = [rng.permutation(60) for _ in range(2)]
    masks = [[(rng.random((32, H)) >= 0.25) for _ in range(2)] for _ in range(2)]
    pref = O.copy_params(p)
    href, _ = O.fit(pref, x[tr], y[tr], x[va], y[va], batch_size=32, max_epochs=2, patience=100, drop_p=0.25,
                    perm_fn=lambda e: perms[e], mask_fn=lambda e, s, nb: masks[e][s][:nb])
    torch.set_num_threads(2)
    xt, xv = torch.from_numpy(x[tr]), torch.from_numpy(x[va])
    yt, yv = torch.from_numpy(y[tr].astype(np.float32)), torch.from_numpy(y[va].astype(np.float32))
    for fused in (True, False):           # single-pass torch._fused_adam_ with the Keras-equivalent eps, and the foreach form
        net = TorchCpuLocator(O.cast_params(p, np.float32), 0.25, fused=fused)
        for e in range(2):
            loss, val = net.fit_epoch(xt, yt, xv, yv, perms[e],
                                      [torch.from_numpy(m.astype(np.float32)) for m in masks[e]], 1e-3)
            assert abs(loss - href["loss"][e]) < 1e-4 and abs(val - href["val_loss"][e]) < 1e-4
        got = net.export()
        for k in ("gamma", "beta", "mov_mean", "mov_var"):
            assert np.abs(got[k] - pref[k]).max() < 5e-5, (fused, k)
        for l in range(len(pref["W"])):
            assert np.abs(got["W"][l] - pref["W"][l]).max() < 5e-5, (fused, l)
            assert np.abs(got["b"][l] - pref["b"][l]).max() < 5e-5, (fused, l)


def test_sparse_support_problem_trains_like_its_reduced_problem():
    """The premise of tests/test_gpu_large_k.py: SNP columns that are constant over the samples (0s, one tile of 1s, one
    of 2s) and start with zero first-layer weights change nothing.  x - mean = 0 exactly there, so they add nothing to z1,
    their W1 / gamma / beta gradients are exactly 0 and Adam leaves them where they were: a fit of the full problem equals
    the fit of the problem made of the active columns alone, to fp64 round-off, with the same permutations and masks."""
    from tests.gpu_util import sparse_problem
    K, width, nlayers, n_train = 2000, 64, 4, 80
    tiles = [0, 1, 30, 31, 62]                                     # tile 62 is the last one, 16 SNPs (K = 62 * 32 + 16)
    x, y, cols, const = sparse_problem(K, width, nlayers, tiles, n_train + 20, seed=3)
    assert sorted(const.values()) == [1, 2] and len(cols) == 4 * 32 + 16
    rng = np.random.default_rng(4)
    p = O.init_params(K, width, nlayers, rng)
    inactive = np.setdiff1d(np.arange(K), cols)
    p["W"][0][inactive] = 0.0
    pr = O.copy_params(p)
    pr["W"][0] = p["W"][0][cols]
    for k in ("gamma", "beta", "mov_mean", "mov_var"):
        pr[k] = p[k][cols]
    perms = [np.random.default_rng(10 + e).permutation(n_train) for e in range(3)]
    masks = [[rng.random((32, width)) >= 0.25 for _ in range(3)] for _ in range(3)]
    tr, va = slice(0, n_train), slice(n_train, n_train + 20)
    kw = dict(batch_size=32, max_epochs=3, patience=100, drop_p=0.25, perm_fn=lambda e: perms[e],
              mask_fn=lambda e, s, nb: masks[e][s][:nb])
    hf, _ = O.fit(p, x[tr], y[tr], x[va], y[va], **kw)
    hr, _ = O.fit(pr, x[tr][:, cols], y[tr], x[va][:, cols], y[va], **kw)
    assert len(hf["loss"]) == 3
    assert np.abs(np.subtract(hf["loss"], hr["loss"])).max() < 1e-12
    assert np.abs(np.subtract(hf["val_loss"], hr["val_loss"])).max() < 1e-12
    assert np.abs(p["W"][0][cols] - pr["W"][0]).max() < 1e-12
    w0 = O.init_params(K, width, nlayers, np.random.default_rng(4))["W"][0][cols]
    assert np.abs(pr["W"][0] - w0).max() > 1e-4                    # the active rows did train
    for l in range(1, nlayers + 2):
        assert np.abs(p["W"][l] - pr["W"][l]).max() < 1e-12 and np.abs(p["b"][l] - pr["b"][l]).max() < 1e-12
    for k in ("gamma", "beta", "mov_mean", "mov_var"):
        assert np.abs(p[k][cols] - pr[k]).max() < 1e-12, k
    assert not p["W"][0][inactive].any()
    assert (p["gamma"][inactive] == 1.0).all() and (p["beta"][inactive] == 0.0).all()
    # moving statistics of a constant column c after s = 9 steps: mean c (1 - 0.99^s), variance 0.99^s
    c = np.zeros(K)
    for kt, v in const.items():
        c[32 * kt:32 * kt + 32] = v
    assert np.abs(p["mov_mean"][inactive] - c[inactive] * (1 - 0.99 ** 9)).max() < 1e-12
    assert np.abs(p["mov_var"][inactive] - 0.99 ** 9).max() < 1e-12
    assert np.abs(O.predict(p, x) - O.predict(pr, x[:, cols])).max() < 1e-12


# ---------------------------------------------------------------- Adam moments as an observer of gradient magnitude
# tests/test_gpu_moments.py compares the device's Adam moments with the oracle's after one epoch.  Here, without a GPU:
# the metric it uses (tests/gpu_util.moments_err) sees a 10 % error in one gradient tensor at full size, and the fp32
# oracle's own distance from the float64 one (the floor the GPU bars are multiples of) is four orders of magnitude lower.
_MOMENT_CASES = [(300, 64, 4, 200, 450), (900, 256, 4, 128, 300)]     # K, width, nlayers, batch, n_train
_moment_runs = {}


def _moment_case(case):
    """One epoch on `case`, three times: float64, float64 with the layer-1 kernel gradient scaled by 0.9, float32.
    Computed once per case."""
    if case not in _moment_runs:
        from tests.gpu_util import make_problem, replay_epoch
        K, width, nlayers, batch, n_train = case
        x, y, p, rng = make_problem(n_train, K, width, nlayers, seed=K + width)
        perm = rng.permutation(n_train)
        steps = -(-n_train // batch)
        masks = (rng.random((steps, batch, width)) >= 0.25).astype(np.uint8)

        def scale_w1(g):
            g["W"][0] *= 0.9
        kw = dict(x=x, y=y, rows=perm, batch=batch, masks=masks, drop_p=0.25)
        _moment_runs[case] = (replay_epoch(p, **kw), replay_epoch(p, grad_hook=scale_w1, **kw),
                              replay_epoch(p, dtype=np.float32, **kw))
    return _moment_runs[case]


def test_moments_err_on_known_arrays():
    from tests.gpu_util import moments_err, tile_norms
    rng = np.random.default_rng(0)
    ref = {"gamma": rng.normal(size=70), "beta": rng.normal(size=70),
           "W": [rng.normal(size=(70, 40)), rng.normal(size=(40, 2))], "b": [rng.normal(size=40), np.zeros(2)]}
    assert tile_norms(ref["W"][0]).shape == (3, 2) and tile_norms(ref["W"][1]).shape == (2, 1)
    assert np.isclose(tile_norms(ref["W"][0])[2, 1], np.linalg.norm(ref["W"][0][64:, 32:]))
    assert np.isclose(np.linalg.norm(tile_norms(ref["W"][0])), np.linalg.norm(ref["W"][0]))
    got = O.copy_params(ref)
    t, tt = moments_err(got, ref)
    assert set(t) == {"gamma", "beta", "W0", "b0", "W1", "b1"} and set(tt) == {"W0", "W1"}
    assert not any(t.values()) and not any(tt.values())          # b1: reference norm 0 and exactly 0 on the other side
    got["W"][0][64:, 32:] *= 1.5                                  # the last, partial tile (6 x 8 of 70 x 40) alone
    got["gamma"] *= 0.8
    got["b"][1][1] = 1e-30
    t, tt = moments_err(got, ref)
    assert np.isclose(tt["W0"], 0.5) and 0 < t["W0"] < 0.1 and tt["W1"] == 0
    assert np.isclose(t["gamma"], 0.2) and t["beta"] == 0 and t["b1"] == np.inf


@pytest.mark.parametrize("case", _MOMENT_CASES)
def test_moments_see_a_ten_percent_gradient_error(case):
    """g["W"][0] *= 0.9 in every step of one epoch: after it m["W"][0] is off by a relative 0.1 and v["W"][0] by 0.19
    (the weights move as well, so not to the last digit), where three epochs of weights after Adam move by 3e-5."""
    from tests.gpu_util import moments_err
    (_, m, v), (_, mb, vb), _ = _moment_case(case)
    em, _ = moments_err(mb, m)
    ev, tv = moments_err(vb, v)
    assert 0.09 <= em["W0"] < 0.11, em
    assert 0.17 <= ev["W0"] < 0.21, ev
    assert tv["W0"] >= 0.17, tv


@pytest.mark.parametrize("case", _MOMENT_CASES)
def test_fp32_oracle_moments_floor(case):
    """The fp32 NumPy oracle against the float64 one after one epoch: below 1e-4 per tensor and per 32 x 32 tile, on
    both moments and every step's loss within 2e-5."""
    from tests.gpu_util import moments_err
    (l64, m, v), _, (l32, m32, v32) = _moment_case(case)
    assert np.abs(l64 - l32).max() < 2e-5
    for got, ref in ((m32, m), (v32, v)):
        t, tt = moments_err(got, ref)
        assert max(t.values()) < 1e-4, t
        assert max(tt.values()) < 1e-4, tt
