"""No result may depend on stale scratch memory, and no kernel may store outside the documented extents.

LocatorNet.ws, ws_predict and l1_image come from torch.empty.  In a test process that memory is almost always zero; in a
replicate run the caching allocator hands a fit the bytes of the previous one, and a buffer that last held int32 -1 reads
as NaN.  api.hip::carve lays nine regions end to end in the workspace, so a store one tile too far lands in a neighbour or
in the allocator's slack, where nothing faults and nothing is compared.  GPU sanitizers are not available to this suite:
poisoned scratch and guard bands are (tests/gpu_util.py: poison, guarded, swap_scratch).

Every route below runs three times from the same parameters, seed, permutations and tuning - scratch zero-filled, filled
with 0xFFFFFFFF words (NaN), filled with seeded finite junk in +-1e4 - on workspaces and an image buffer of EXACTLY the
sizes the library asks for, each inside guard margins of 128 rows.  The three runs have to agree bit for bit and every
margin has to survive.  The contract this pins is stated in include/locator_hip.h (Conventions).

What is poisoned: the workspaces, the image buffer, the runner's per-step losses / validation distances, the epoch's
batch statistics and the validation predictions, yhat / dist of a predict.  Never rows, permutations, offsets or masks.
No kernel derives an address or a loop bound from a value in those buffers: the one integer kept in scratch is the tail
ticket of the int8 image header (l1_gemm_i8.hip), which selects the workgroup that finishes the guard and is zeroed by the
scan of the same call - it is never waited on.  So the whole of every buffer is poisoned."""
import numpy as np
import pytest
import torch

from tests.gpu_util import bits, build_net, guarded, make_problem, poison, poison_scratch, swap_scratch
from tests.test_gpu_dosage_paths import _dosage_problem
from tests.test_gpu_moments import CASES, IDS

pytestmark = pytest.mark.gpu

KINDS = ("zero", "nan", "junk")


def _state(net):
    out = {"params": bits(net.params), "adam_m": bits(net.adam_m), "adam_v": bits(net.adam_v), "lr_t": bits(net.lr_t)}
    if net.wht is not None:
        out["wht"] = bits(net.wht)
    return out


def _assert_same(got, ref, what):
    assert got.keys() == ref.keys(), (what, sorted(got), sorted(ref))
    for k in ref:
        a, b = got[k], ref[k]
        same = torch.equal(a, b) if torch.is_tensor(b) else np.array_equal(a, b)
        if not same:
            a, b = np.asarray(a), np.asarray(b)
            n = int((a != b).sum()) if a.shape == b.shape else -1
            raise AssertionError(f"{what}: {k} differs from the run on zero-filled scratch in {n} of {b.size} words")


# ------------------------------------------------------------------ 1. training routes
def _train_run(x, y, p, K, batch, n_train, n_val, chain, tuning, route, perms, kind):
    from locator_amd.train import EpochRunner
    tr, va = np.arange(n_train), np.arange(n_train, n_train + n_val)
    net = build_net(x, y, p, drop_p=0.25, seed=5, tuning=tuning)
    runner = EpochRunner(net, tr, va, batch, use_graph=True, chain=chain)
    assert route(net, runner), (net.d.Hp, net.d.Kp, net.use_fused, runner.chain, runner.slot_rows)
    assert not runner.xchain
    checks = swap_scratch(net, runner, kind=kind)
    out = {}
    for e, perm in enumerate(perms):                 # epoch 0 eager, epoch 1 captured and replayed
        if e:
            poison_scratch(net, runner, kind, seed=e)        # nothing is handed over across the epoch boundary
        runner.run_epoch(perm)
        torch.cuda.synchronize()
        out[f"stats{e}"] = bits(runner.stats_host[:runner.steps + n_val].clone())
    assert runner.graph is not None
    out.update(_state(net))
    for check in checks:
        check()
    return out


@pytest.mark.parametrize("K,width,nlayers,batch,n_train,chain,tuning,route", CASES, ids=IDS)
def test_training_route_ignores_stale_scratch(K, width, nlayers, batch, n_train, chain, tuning, route):
    """Two epochs (eager, then the captured graph) on every training route of tests/test_gpu_moments.py: parameters with the
    moving statistics, both Adam moments, the transposed hidden kernels, the learning rate and both epochs' per-step
    losses and validation distances are the same bits whether the scratch started as zeros, NaN or finite junk - poisoned
    again before the second epoch - and every guard margin is untouched."""
    n_val = 9
    x, y, p, _ = make_problem(n_train + n_val, K, width, nlayers, seed=K + width)
    perms = [np.random.default_rng(e).permutation(n_train) for e in range(2)]
    args = (x, y, p, K, batch, n_train, n_val, chain, tuning, route, perms)
    ref = _train_run(*args, "zero")
    assert torch.isfinite(ref["params"].view(torch.float32)).all() and torch.isfinite(ref["stats1"].view(torch.float32)).all()
    for kind in KINDS[1:]:
        _assert_same(_train_run(*args, kind), ref, kind)


def _fit_run(x, y, p, n_train, n_val, perms, kind):
    from locator_amd.train import FitLoop
    tr, va = np.arange(n_train), np.arange(n_train, n_train + n_val)
    net = build_net(x, y, p, drop_p=0.25, seed=11)
    loop = FitLoop(net, tr, va, batch_size=32, max_epochs=len(perms), patience=100, perm_fn=lambda e: perms[e], xchain=True)
    r = loop.runner
    assert r.chain and r.xchain and net.ws_predict is not None
    checks = swap_scratch(net, r, kind=kind)        # before epoch 0 only: the hand-over lives in ws and in stats_ep2
    assert net.ws_predict.data_ptr() != net.ws.data_ptr()
    hist = loop.run().history
    torch.cuda.synchronize()
    assert r.graphs[0] is not None
    out = _state(net)
    out["best"] = bits(net.best)
    out["stats"] = bits(r.stats_host[:r.steps + n_val].clone())
    for k in ("loss", "val_loss", "learning_rate"):
        out[k] = np.asarray(hist[k], np.float64).view(np.int64)
    for check in checks:
        check()
    return out


@pytest.mark.parametrize("K,width,n_val", [(600, 256, 520), (400, 128, 9)], ids=["width256-int8-validation", "width128"])
def test_cross_epoch_chained_fit_ignores_stale_scratch(K, width, n_val):
    """FitLoop(xchain=True), three epochs (two eager, the third captured): the layer-1 hand-over crosses the epoch boundary
    in ws while the validation sweep works in ws_predict (at width 256 its 520 rows build the int8 image inside the
    epoch), so the scratch is poisoned before epoch 0 only.  History, best weights and the final state are the same bits."""
    n_train = 100
    x, y, p, _ = make_problem(n_train + n_val, K, width, 4, seed=K)
    perms = [np.random.default_rng(300 + e).permutation(n_train) for e in range(3)]
    ref = _fit_run(x, y, p, n_train, n_val, perms, "zero")
    assert np.isfinite(ref["val_loss"].view(np.float64)).all()
    for kind in KINDS[1:]:
        _assert_same(_fit_run(x, y, p, n_train, n_val, perms, kind), ref, kind)


# ------------------------------------------------------------------ 2. predict routes
def _predict_run(x, y, p, rows, kind, net_kw, prep, twice):
    net = build_net(x, y, p, **net_kw)
    if prep is not None:
        prep(net)
    n = len(rows)
    rows_dev = torch.from_numpy(rows.astype(np.int32)).cuda()
    checks = swap_scratch(net, None, kind=kind)
    yhat, check_y = guarded(2 * n, torch.float32, 128 * net.d.Hp)
    dist, check_d = guarded(n, torch.float32, 128 * net.d.Hp)
    out = {}
    for call in range(2 if twice else 1):
        if call:                                    # the second predict finds the image of the first: all but l1_image
            poison_scratch(net, None, kind, seed=call, with_image=False)
        poison(yhat, kind, 100 + call)
        poison(dist, kind, 200 + call)
        torch.cuda.synchronize()
        net.predict_rows(rows_dev, n, yhat.view(n, 2), dist)
        torch.cuda.synchronize()
        out[f"yhat{call}"], out[f"dist{call}"] = bits(yhat), bits(dist)
        out[f"mode{call}"] = np.array([net._image_mode, net._net.l1_image_ready])
        out[f"guard{call}"] = np.array(net._guard if net._guard is not None else (), np.float64).view(np.int64)
    for check in checks + [lambda: check_y("yhat"), lambda: check_d("dist")]:
        check()
    return net, out


def _pack(net):
    net.auto_pack = True


# id: (n_samples, K, width, nlayers, rows, net_kw, prep, twice, dosage, image mode expected - None = from the guard)
_CHUNK = 16384                                       # LOC_PREDICT_CHUNK
ROUTES = {
    "rows-20": (40, 300, 256, 4, 20, {}, None, False, False, 0),
    "rows-100-l1-forward-rows": (120, 300, 256, 4, 100, {}, None, False, False, 0),
    "bf16-3-pieces": (200, 700, 256, 4, 1152, dict(predict_digits=-1, predict_pieces=3), None, False, False, 3),
    "bf16-2-pieces": (200, 700, 256, 4, 768, dict(predict_digits=-1, predict_pieces=2), None, False, False, 2),
    "bf16-1-piece": (200, 700, 256, 4, 640, dict(predict_digits=-1, predict_pieces=1), None, False, False, 1),
    "int8-3-digits-guarded": (200, 700, 256, 4, 512, dict(predict_digits=3), None, False, False, None),
    "int8-2-digits": (200, 700, 256, 4, 512, dict(predict_digits=2), None, False, False, 12),
    "int8-auto-guarded": (200, 700, 256, 4, 512, dict(predict_digits=0), None, False, False, None),
    "int8-auto-pack": (200, 300, 256, 4, 3072, dict(predict_digits=2), _pack, False, False, 12),
    "int8-gemm-reduce": (200, 700, 256, 4, 600, dict(predict_digits=2, tuning={"gemm_reduce": 1}), None, False, False, 12),
    "stack-rows-1": (200, 700, 256, 4, 600, dict(predict_digits=2, tuning={"stack_rows": 1}), None, False, False, 12),
    "stack-rows-2": (200, 700, 256, 4, 600, dict(predict_digits=2, tuning={"stack_rows": 2}), None, False, False, 12),
    "stack-rows-vector-alu": (200, 700, 256, 4, 600, dict(predict_digits=2, tuning={"stack_rows": -1}), None, False, False, 12),
    "one-tile-tail-chunk": (200, 300, 256, 3, _CHUNK + 5, dict(predict_digits=2), None, False, False, 12),
    "nlayers1-rows-40": (60, 300, 64, 1, 40, {}, None, False, False, 0),
    "width96-per-layer": (60, 300, 96, 4, 40, {}, None, False, False, 0),
    "width600-per-layer": (60, 300, 600, 3, 40, {}, None, False, False, 0),
    "width128-rows-1500": (200, 400, 128, 4, 1500, {}, None, False, False, 0),
    "dosage-int8": (200, 700, 256, 4, 512, dict(predict_digits=3, unit=63), None, False, True, None),
    "second-predict-int8": (200, 700, 256, 4, 512, dict(predict_digits=3), None, True, False, None),
    "second-predict-bf16": (200, 700, 256, 4, 1152, dict(predict_digits=-1), None, True, False, 3),
}


@pytest.mark.parametrize("route", list(ROUTES), ids=list(ROUTES))
def test_predict_route_ignores_stale_scratch(route):
    """Every route of loc_predict (asserted through the image mode it ran in, the packed matrix, the kept image) gives the
    same bits in yhat, dist and the dynamic-range guard on zero-filled, NaN and junk scratch - workspace, image buffer
    and the outputs themselves - with every margin untouched.  A second predict with unchanged weights reuses the image:
    everything but l1_image is poisoned again between the two calls."""
    n_samples, K, width, nlayers, n, net_kw, prep, twice, dosage, mode = ROUTES[route]
    if dosage:
        x, _, y, p = _dosage_problem(n_samples, K, width, nlayers, seed=K + n)
        assert x.max() == 126
    else:
        x, y, p, _ = make_problem(n_samples, K, width, nlayers, seed=K + n)
    rows = np.random.default_rng(n).permutation(n) % n_samples
    net_kw = dict(net_kw, drop_p=0.25)
    outs = {}
    for kind in KINDS:
        net, outs[kind] = _predict_run(x, y, p, rows, kind, net_kw, prep, twice)
        o = outs[kind]
        guard = net._guard
        want = mode
        if want is None:                             # the guard decided the digit planes (2, 3 or -1: bf16 x 3)
            assert guard is not None
            allowed = int(guard[2] if net.predict_digits == 0 else guard[3])
            want = 10 + allowed if allowed > 0 else 3
        else:
            assert guard is None
        assert int(o["mode0"][0]) == want, (kind, o["mode0"], want)
        if want >= 12:
            assert 1 <= net.genotype_max() <= 127
        if prep is _pack:
            assert getattr(net.X, "loc_x2", None) is not None and net._net.X2
        if twice:
            assert tuple(o["mode1"]) == (want, want), o["mode1"]       # the second call skipped the conversion
            assert tuple(o["mode0"]) == (want, 0), o["mode0"]
        assert torch.isfinite(o["yhat0"].view(torch.float32)).all() and torch.isfinite(o["dist0"].view(torch.float32)).all()
    if twice:
        _assert_same({k[:-1]: v for k, v in outs["zero"].items() if k[-1] == "1" and k[:4] != "mode"},
                     {k[:-1]: v for k, v in outs["zero"].items() if k[-1] == "0" and k[:4] != "mode"}, "second call")
    for kind in KINDS[1:]:
        _assert_same(outs[kind], outs["zero"], kind)
