"""Replicate runs of the command line (--windows, --bootstrap) against an independent rebuild and the fp64 oracle, and the
same runs under every worker layout.

The kernels are pinned one at a time elsewhere (test_gpu_parity.py, test_gpu_filter.py); here the question is what each
replicate UNIT trains on and writes: the composition of the parent's draws (split per window, reseed + site_order chain),
the window slice (gt[a:b] excludes SNP b), the filters (device or host), the row order, the column gather and
the hand-off to the fit thread / worker process.

  A. one run of each job in-process with one fit thread, `train.fit` spied on: the matrix every unit trains on equals the
     rebuild in reference order (NumPy global stream, oracle.split_train_test / bootstrap_chain, the host NumPy filter)
     byte for byte; oracle.fit from the unit's own initial weights, permutations and dropout masks reproduces its history;
     oracle.predict on the best weights reproduces its *_predlocs.txt; {out}_history.txt is the last replicate's.
  B. the same jobs under every worker layout write the same files byte for byte.
  C. early stopping and the LR plateau firing inside FitLoop, against oracle.fit.

Fixture: the reference's example data (500 samples x 11,527 variants, 50 without coordinates) as a zarr store with 2 % of
the allele calls set missing, so the filters' missing-call handling is on the path.
"""
import json
import os
import threading

import numpy as np
import pandas as pd
import pytest
import torch

from locator_amd import genotypes as G
from locator_amd import locator as L
from oracle import locator_oracle as O

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
SEED = 4242
EPOCHS = ["--max_epochs", "6", "--patience", "6"]          # LR patience int(6 / 6) = 1: the plateau can fire
WINDOW = 400_000
NBOOTS = 4
# SNPs per window after the host filters, with the missing calls below (none a multiple of 32, the last window short)
WINDOW_SNPS = [1021, 923, 921, 928, 927, 883, 208]
BOOT_SNPS = 5817
LAYOUT_KEYS = {"in_process", "fits_per_gpu", "procs_per_gpu", "worker_start", "host_filter", "gpus", "out"}


# ------------------------------------------------------------------ fixture data
@pytest.fixture(scope="module")
def data(tmp_path_factory):
    v = G.read_vcf(os.path.join(GOLD, "test_genotypes.vcf.gz"))
    gt = np.array(v["calldata/GT"], dtype=np.int8)
    gt[np.random.default_rng(3).random(gt.shape) < 0.02] = -1           # 2 % of the allele calls missing
    root = tmp_path_factory.mktemp("replicates")
    store = str(root / "fix.zarr")
    G.write_callset_zarr(store, gt, v["variants/POS"], v["samples"], chunk_variants=4096, compressor="blosc")
    return {"gt": gt, "pos": np.asarray(v["variants/POS"]), "samples": np.asarray(v["samples"]).astype(str),
            "store": store, "root": root}


def _argv(data, job, out, extra=()):
    common = ["--zarr", data["store"], "--sample_data", os.path.join(GOLD, "test_sample_data.txt"), "--out", out,
              "--seed", str(SEED), "--keras_verbose", "0", "--predict_mode", "exact"] + EPOCHS
    job_flags = {"W": ["--windows", "--window_size", str(WINDOW)], "B": ["--bootstrap", "--nboots", str(NBOOTS)]}[job]
    return common + job_flags + list(extra)


def _main(argv):
    np.random.seed(None)
    assert L.main(argv) == 0


# ------------------------------------------------------------------ independent rebuild, reference order
def _locs(samples):
    """sort_samples + normalize_locs (locator.py:231-247, :284-292) written out with pandas / the oracle."""
    table = pd.read_csv(os.path.join(GOLD, "test_sample_data.txt"), sep="\t").set_index("sampleID")
    locs = table.loc[list(samples), ["x", "y"]].to_numpy(dtype=np.float64)
    return O.normalize_locs(locs)


def _unit(ac, locs_norm, norm):
    """oracle.split_train_test (one draw from the global stream) + everything a unit's fit and predictions depend on."""
    train, test, traingen, testgen, trainlocs, testlocs, pred, predgen = O.split_train_test(ac, locs_norm)
    meanlong, sdlong, meanlat, sdlat = norm
    return dict(train=train, test=test, pred=pred, traingen=traingen, testgen=testgen, predgen=predgen,
                trainlocs=trainlocs, testlocs=testlocs, norm=(meanlong, sdlong, meanlat, sdlat))


def _host_filter(gt):
    return G.filter_snps(gt, min_mac=2, verbose=False, native=False)


def rebuild_windows(data):
    """The reference's --windows main (locator.py:506-545): whole-store prologue (filter, split: one draw), then per window
    the slice gt[a:b], sort, normalise, filter and split (one draw each).  -> [unit dict] in window order."""
    gt, pos, samples = data["gt"], data["pos"], data["samples"]
    np.random.seed(SEED)
    meanlong, sdlong, meanlat, sdlat, locs = _locs(samples)
    _unit(_host_filter(gt), locs, (meanlong, sdlong, meanlat, sdlat))
    units = []
    for i in np.arange(0, pos.max(), WINDOW):
        inside = np.argwhere((pos >= i) & (pos < i + WINDOW))
        a, b = int(np.min(inside)), int(np.max(inside))
        meanlong, sdlong, meanlat, sdlat, locs = _locs(samples)
        u = _unit(_host_filter(gt[a:b]), locs, (meanlong, sdlong, meanlat, sdlat))
        u["stem"] = f"_{i}-{i + WINDOW - 1}"
        units.append(u)
    return units


def rebuild_bootstrap(data):
    """The reference's --bootstrap main (locator.py:506-516, :612-653): prologue split, the FULL unit, then per replicate
    reseed + site_order (oracle.bootstrap_chain) and the three column resamples.  -> [FULL, boot 0, ...]."""
    np.random.seed(SEED)
    meanlong, sdlong, meanlat, sdlat, locs = _locs(data["samples"])
    full = _unit(_host_filter(data["gt"]), locs, (meanlong, sdlong, meanlat, sdlat))
    full["boot"] = "FULL"
    units = [full]
    for b, (_, so) in enumerate(O.bootstrap_chain(NBOOTS, full["traingen"].shape[1])):
        u = dict(full, boot=str(b), site_order=so)
        for k in ("traingen", "testgen", "predgen"):
            u[k] = full[k][:, so]
        units.append(u)
    return units


# ------------------------------------------------------------------ part A: one spied run per job
class FitSpy:
    """Stands in for locator_amd.train.fit (train_network imports it at call time).  Per unit (keyed by the net's replicate
    index) it records the device matrix, the initial parameters, the permutations - drawn from the very generator FitLoop
    would build, so the run's files do not change - and, after the fit, the dropout masks of every epoch regenerated
    with the runner's size and offsets, in the [steps][slot rows][Hp] layout."""

    def __init__(self):
        from locator_amd import train
        self.real = train.fit
        self.units = {}
        self.lock = threading.Lock()

    def __call__(self, net, train_rows, val_rows, **kw):
        assert "perm_fn" not in kw
        rec = {"X": net.X.cpu().numpy().copy(), "K": net.d.K, "Kp": net.d.Kp, "Hp": net.d.Hp, "width": net.d.H,
               "train_rows": np.asarray(train_rows).copy(), "val_rows": np.asarray(val_rows).copy(),
               "p0": net.export_params(), "perms": {}, "batch": kw["batch_size"]}
        rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence([net.seed, net.replicate, 0x7065726D])))

        def perm_fn(e):
            rec["perms"][e] = rng.permutation(len(train_rows))
            return rec["perms"][e]
        hist = self.real(net, train_rows, val_rows, perm_fn=perm_fn, **kw)
        steps = -(-len(train_rows) // rec["batch"])
        n = steps * net.slot_rows * net.mask_width
        buf = torch.empty(n, dtype=torch.uint8, device=net.device)
        rec["masks"] = []
        for e in range(len(hist.history["loss"])):
            net.fill_dropout_masks(buf, n, e * n)
            rec["masks"].append(buf.cpu().numpy().reshape(steps, net.slot_rows, net.mask_width).copy())
        rec["history"] = {k: list(v) for k, v in hist.history.items()}
        with self.lock:
            assert net.replicate not in self.units, "two units share a replicate index"
            self.units[net.replicate] = rec
        return hist


@pytest.fixture(scope="module")
def runs_a(data):
    out = {}
    for job in ("W", "B"):
        spy = FitSpy()
        d = data["root"] / f"A_{job}"
        d.mkdir()
        with pytest.MonkeyPatch.context() as mp:
            from locator_amd import train
            mp.setattr(train, "fit", spy)
            _main(_argv(data, job, str(d / "r"), ["--in_process", "--fits_per_gpu", "1"]))
        out[job] = {"dir": d, "stem": str(d / "r"), "units": spy.units}
    return out


def _read_history(path):
    h = pd.read_csv(path, sep="\t", float_precision="round_trip")
    assert list(h.columns) == ["loss", "val_loss", "learning_rate"], list(h.columns)
    return {k: h[k].tolist() for k in h.columns}


def maxdiff(a, b):
    return float(np.abs(np.subtract(a, b)).max())


def _check_unit(rec, ref, history, predlocs_path, samples, what):
    K = ref["traingen"].shape[1]
    # 1. the device matrix: [traingen; testgen; predgen] byte for byte in columns 0..K, zero padding up to Kp
    want = np.concatenate([ref["traingen"], ref["testgen"], ref["predgen"]], axis=0).astype(np.uint8)
    X = rec["X"]
    assert rec["K"] == K, (what, rec["K"], K)
    assert X.shape == (want.shape[0], (K + 31) // 32 * 32), (what, X.shape)
    assert np.array_equal(X[:, :K], want), (what, "device matrix differs from the rebuild", np.argwhere(X[:, :K] != want)[:5])
    assert not X[:, K:].any(), (what, "nonzero padding")
    ntr, nva = len(ref["train"]), len(ref["test"])
    assert np.array_equal(rec["train_rows"], np.arange(ntr)) and np.array_equal(rec["val_rows"], np.arange(ntr, ntr + nva))
    # 2. oracle.fit from the unit's initial weights, permutations and masks reproduces its history
    width = rec["width"]

    def oracle(dt):
        p = O.cast_params(rec["p0"], dt)
        h, best = O.fit(p, ref["traingen"], ref["trainlocs"].astype(dt), ref["testgen"], ref["testlocs"].astype(dt),
                        batch_size=rec["batch"], max_epochs=6, patience=6, drop_p=0.25, perm_fn=lambda e: rec["perms"][e],
                        mask_fn=lambda e, s, nb: rec["masks"][e][s, :nb, :width])
        return h, O.predict(O.cast_params(best, np.float64), ref["predgen"])
    href, z = oracle(np.float64)
    meanlong, sdlong, meanlat, sdlat = ref["norm"]
    got = pd.read_csv(predlocs_path)
    assert list(got.columns) == ["x", "y", "sampleID"]
    assert list(got["sampleID"]) == list(samples[ref["pred"]]), what
    zgot = np.stack([(got["x"].to_numpy() - meanlong) / sdlong, (got["y"].to_numpy() - meanlat) / sdlat], axis=1)
    assert history == rec["history"], (what, "history file is not the unit's fit")
    assert len(history["loss"]) == len(href["loss"]), (what, history, href)
    assert [float(np.float32(v)) for v in href["learning_rate"]] == history["learning_rate"], (what, href, history)
    rel = lambda a, b: float((np.abs(np.asarray(a) - b) / np.maximum(np.abs(b), 1.0)).max())
    errs = {"loss": maxdiff(history["loss"], href["loss"]), "val_loss": maxdiff(history["val_loss"], href["val_loss"]),
            "predictions": rel(zgot, z)}                     # 3. 1e-3 relative on z-scored outputs
    bars = {"loss": 5e-4, "val_loss": 5e-4, "predictions": 1e-3}
    if any(errs[k] >= bars[k] for k in bars):
        # Six epochs (78 Adam steps) through the default 10 x 256 stack amplify fp32 round-off: on some units the fp32
        # NumPy oracle itself lands 1.2e-3 from the fp64 one on the predictions (measured: window 1 of this fixture).  There
        # the device must be no further from fp64 than fp32 arithmetic is, within a factor 3.
        h32, z32 = oracle(np.float32)
        floor = {"loss": maxdiff(h32["loss"], href["loss"]), "val_loss": maxdiff(h32["val_loss"], href["val_loss"]),
                 "predictions": rel(z32, z)}
        for k in bars:
            assert errs[k] < max(bars[k], 3 * floor[k]), (what, k, errs[k], "fp32 oracle", floor[k])
    return href


def test_window_units_train_on_the_rebuilt_windows_and_match_the_oracle(data, runs_a):
    """--windows --window_size 400000: 7 windows; each unit's device matrix is its window's rebuild (slice gt[a:b], host
    filter, the split drawn for that window), and its history / predictions are oracle.fit's on that rebuild."""
    ref = rebuild_windows(data)
    assert [u["traingen"].shape[1] for u in ref] == WINDOW_SNPS
    run = runs_a["W"]
    assert sorted(run["units"]) == list(range(len(ref)))
    for n, u in enumerate(ref):
        stem = run["stem"] + u["stem"]
        _check_unit(run["units"][n], u, _read_history(stem + "_history.txt"), f"{stem}_0-{WINDOW - 1}_predlocs.txt",
                    data["samples"], f"window {n}")


def test_bootstrap_units_train_on_the_rebuilt_resamples_and_match_the_oracle(data, runs_a):
    """--bootstrap --nboots 4: the FULL unit and 4 resamples of its 5,817 SNP columns (site_order from the reseed chain);
    every unit against the rebuild and oracle.fit, and {out}_history.txt holds the LAST replicate's history, as the
    reference leaves it (every replicate overwrites it there)."""
    ref = rebuild_bootstrap(data)
    assert ref[0]["traingen"].shape[1] == BOOT_SNPS
    run = runs_a["B"]
    assert sorted(run["units"]) == list(range(NBOOTS + 1))
    hists = []
    for r, u in enumerate(ref):
        rec = run["units"][r]
        _check_unit(rec, u, rec["history"], f"{run['stem']}_boot{u['boot']}_predlocs.txt", data["samples"], f"boot {u['boot']}")
        hists.append(rec["history"])
    assert _read_history(run["stem"] + "_history.txt") == hists[-1]
    assert hists[-1] != hists[0]           # the last replicate's history is told apart from the FULL fit's


# ------------------------------------------------------------------ part B: the same files under every layout
LAYOUTS = [
    ("in_process_3_threads", ["--in_process"]),
    ("forkserver_3_threads", []),
    ("two_procs_one_fit_each", ["--procs_per_gpu", "2", "--fits_per_gpu", "1"]),
    ("spawn_2_threads", ["--worker_start", "spawn", "--fits_per_gpu", "2"]),
    ("host_filter", ["--host_filter"]),             # --windows only
    ("two_gpus", ["--gpus", "2"]),                  # skips on single-GPU hosts
]
CASES = [(job, name, flags) for job in ("W", "B") for name, flags in LAYOUTS if not (job == "B" and name == "host_filter")]


def _files(d):
    return sorted(os.listdir(d))


@pytest.mark.parametrize("job,name,flags", CASES, ids=[f"{j}-{n}" for j, n, _ in CASES])
def test_layout_writes_the_same_files(data, runs_a, job, name, flags):
    """identical files for any GPU / process / thread layout.  Every *_predlocs.txt and *_history.txt byte for
    byte against the part-A run (whose units are pinned to the oracle), the same file set, and _params.json equal but for
    the layout keys and `out`; _fitplot.pdf is not compared (matplotlib output)."""
    if name == "two_gpus" and torch.cuda.device_count() < 2:
        pytest.skip("layout --gpus 2 needs two GPUs (single-GPU host)")
    a = runs_a[job]
    d = data["root"] / f"B_{job}_{name}"
    d.mkdir()
    _main(_argv(data, job, str(d / "r"), flags))
    assert _files(d) == _files(a["dir"])
    n_pred = 0
    for f in _files(a["dir"]):
        if f.endswith("_fitplot.pdf"):
            continue
        got, want = (d / f).read_bytes(), (a["dir"] / f).read_bytes()
        if f.endswith("_params.json"):
            pg, pw = json.loads(got), json.loads(want)
            assert {k: v for k, v in pg.items() if k not in LAYOUT_KEYS} == {k: v for k, v in pw.items() if k not in LAYOUT_KEYS}
            continue
        assert got == want, f"{name}: {f} differs from the in-process single-thread run"
        n_pred += f.endswith("_predlocs.txt")
    assert n_pred == (len(WINDOW_SNPS) if job == "W" else NBOOTS + 1)


# ------------------------------------------------------------------ part C: early stopping that fires
PART_C_SEED = 4          # 14 epochs, stop at 13, 5 LR cuts; smallest decision margin 4e-3, device gap 2e-7


def _overfit_fit(seed):
    """FitLoop (synchronous, device callbacks) and oracle.fit on one overfitting problem: 40 training rows, 30 validation
    rows, patience 6, LR patience 1, at most 60 epochs; the same permutations and the device's dropout masks."""
    from locator_amd.train import FitLoop
    from tests.gpu_util import build_net, make_problem
    K, width, nlayers, max_epochs = 400, 64, 4, 60
    x, y, p, rng = make_problem(82, K, width, nlayers, seed=seed)
    p = O.cast_params(O.cast_params(p, np.float32), np.float64)        # both sides start from the same fp32 values
    tr, va, pr_rows = np.arange(0, 40), np.arange(40, 70), np.arange(70, 82)
    net = build_net(x, y, p, drop_p=0.25, seed=11)
    perms = [np.random.default_rng(500 + e).permutation(40) for e in range(max_epochs)]
    loop = FitLoop(net, tr, va, batch_size=32, max_epochs=max_epochs, patience=6, lr_patience=1,
                   perm_fn=lambda e: perms[e], depth=0)
    masks = []
    while not loop.done:
        loop.submit()
        loop.collect(0)
        masks.append(loop.runner.masks.cpu().numpy().reshape(loop.runner.steps, 32, net.d.Hp).copy())
    hist = loop.finish().history
    href, best = O.fit(O.copy_params(p), x[tr], y[tr], x[va], y[va], batch_size=32, max_epochs=max_epochs, patience=6,
                       drop_p=0.25, perm_fn=lambda e: perms[e], mask_fn=lambda e, s, nb: masks[e][s, :nb, :width])
    yhat = torch.zeros((len(pr_rows), 2), device="cuda")
    net.predict_rows(torch.from_numpy(pr_rows.astype(np.int32)).cuda(), len(pr_rows), yhat)
    torch.cuda.synchronize()
    n = min(len(hist["loss"]), len(href["loss"]))
    gap = max(np.abs(np.subtract(hist["val_loss"][:n], href["val_loss"][:n])).max(),
              np.abs(np.subtract(hist["loss"][:n], href["loss"][:n])).max())
    v = np.asarray(href["val_loss"])
    margin = min(abs(v[e] - v[:e].min()) for e in range(1, len(v)))
    ref = O.predict(best, x[pr_rows])
    rel = float((np.abs(yhat.cpu().numpy() - ref) / np.maximum(np.abs(ref), 1.0)).max())
    return dict(hist=hist, href=href, stop_epoch=loop.stop_epoch, gap=gap, margin=margin, rel=rel, max_epochs=max_epochs)


def test_early_stopping_and_lr_plateau_firing_match_oracle_fit():
    """FitLoop on a problem that overfits: early stopping (patience 6) and the LR plateau (patience 1) both fire well
    before max_epochs.  Same per-epoch losses (5e-4), the same stop epoch and LR column as oracle.fit, and predictions from
    the restored best weights within 1e-3 relative of the oracle's best.  Each strict-'<' decision on the oracle's val_loss
    sequence must clear the measured device-oracle gap ten times over: a seed where it does not is reported as ambiguous,
    not as a parity failure."""
    r = _overfit_fit(PART_C_SEED)
    hist, href, gap, margin = r["hist"], r["href"], r["gap"], r["margin"]
    assert gap < 5e-4, (gap, hist, href)
    assert margin > 10 * gap, f"ambiguous seed: a callback decision is within {margin:.2e} of a tie, gap {gap:.2e}"
    assert len(hist["loss"]) == len(href["loss"]) < r["max_epochs"], (len(hist["loss"]), len(href["loss"]))
    assert r["stop_epoch"] == len(href["loss"]) - 1
    assert [float(np.float32(lr)) for lr in href["learning_rate"]] == hist["learning_rate"]
    assert len(set(hist["learning_rate"])) >= 2                      # at least one LR cut
    assert r["rel"] < 1e-3, r["rel"]
