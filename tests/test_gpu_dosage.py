"""--dosage on the GPU, through the C ABI and the command line: the window filter kernels against the host form (bit for
bit, also past 2^31 bytes of dosages), the BatchNorm statistics in q units against float64 on q / 63, one step and an
8-epoch fit against oracle.fit on q / 63, every predict mode at K = 100,000 with values up to 126, and the CLI end to end.

Tolerances are the existing ones: loss 2e-5 for one step, loss / val_loss 5e-4 along the trajectory, predictions 1e-3
relative; predict modes 2e-5 absolute (exact) and 1e-3 of the largest prediction (auto, fast)."""
import os

import numpy as np
import pandas as pd
import pytest
import torch

from locator_amd import genotypes as G
from locator_amd import locator as L
from oracle import locator_oracle as O
from tests.dosage_util import (SAMPLES, VCF, clean_biallelic, golden_counts, noisy_dosage, write_dosage_vcf, write_dosage_zarr,
                               write_gt_vcf)
from tests.gpu_util import build_net, make_problem, maxerr, params_err

pytestmark = pytest.mark.gpu
U = G.DOSAGE_UNIT


def _host_rows(d, order, min_mac):
    ac = G.filter_dosage(G.dosage_q(d), min_mac, verbose=False)
    return G.rows_transposed(ac, np.asarray(order, np.int64)), ac.shape[0]


def _device_rows(d, order, min_mac):
    from locator_amd.net import filter_dosage_device
    X, K = filter_dosage_device(torch.from_numpy(d).cuda(), order, min_mac)
    torch.cuda.synchronize()
    return X.cpu().numpy(), K


# ------------------------------------------------------------------ window filter kernels
@pytest.mark.parametrize("min_mac", [1, 2, 5])
def test_device_flags_and_rows_equal_the_host_form(min_mac):
    rng = np.random.default_rng(min_mac)
    V, N = 3001, 1100                          # N > one 960-sample LDS chunk; V not a multiple of the 64-variant tile
    af = rng.beta(0.3, 0.8, V)[:, None]
    d = (rng.binomial(2, af, (V, N)) + rng.normal(0, 0.1, (V, N))).clip(0, 2).astype(np.float32)
    d[rng.random(d.shape) < 0.03] = np.nan
    d[5, :] = (np.arange(N) % 127 + 0.5) / 63          # exact half steps: ties round to even on both sides
    d[7, :] = 0                                        # monomorphic
    d[9, :] = np.nan                                   # nothing called
    order = rng.permutation(N)[:900].astype(np.int32)
    want, K = _host_rows(d, order, min_mac)
    got, Kd = _device_rows(d, order, min_mac)
    assert Kd == K and K > 100
    assert np.array_equal(got[:, :K], want) and not got[:, K:].any()


def test_device_rows_past_2_31_bytes_of_dosages():
    """720,000 variants x 765 samples = 2.2 GB of float32: every offset of the slice is 64-bit."""
    V, N = 720_000, 765
    rng = np.random.default_rng(31)
    q0 = rng.integers(0, 127, (V, N), dtype=np.uint8)
    d = q0.astype(np.float32) / np.float32(U)
    del q0
    d[rng.integers(0, V, 20000), rng.integers(0, N, 20000)] = np.nan
    d[V - 3:, :] = np.float32(2.0)                   # the last variants: monomorphic, dropped
    d[V - 5, :N - 1] = 0.0                           # sum(q) = 62, one step short of 63 * min_mac: dropped
    d[V - 5, N - 1] = np.float32(62 / 63)
    assert d.nbytes > 2 ** 31
    order = np.concatenate([np.arange(N - 1, -1, -2), np.arange(0, N, 2)])[:N].astype(np.int32)
    want, K = _host_rows(d, order, 1)
    got, Kd = _device_rows(d, order, 1)
    assert Kd == K and K > V - 10
    assert np.array_equal(got[:, :K], want)


# ------------------------------------------------------------------ BatchNorm statistics in q units
@pytest.mark.parametrize("batch", [32, 4096])
def test_bn_statistics_with_the_unit_against_float64(batch):
    from locator_amd.net import LocatorNet, upload_genotypes
    rng = np.random.default_rng(batch)
    n, K = 4100, 96
    q = rng.integers(0, 127, (n, K)).astype(np.uint8)
    q[:, 3] = 126                                      # the largest sums: sum(x^2) of 4096 rows of 126 needs 64 bits
    X = upload_genotypes(q)
    Y = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
    net = LocatorNet(X, Y, K, 64, 4, 0.0, seed=1, unit=U)
    steps = -(-n // batch)
    perm = rng.permutation(n).astype(np.int32)
    rows = np.zeros(steps * batch, np.int32)
    rows[:n] = perm
    stats = torch.zeros(steps * 2 * net.d.Kp, dtype=torch.float32, device="cuda")
    net.epoch_bn_stats(torch.from_numpy(rows).cuda(), batch, n - (steps - 1) * batch, steps, stats)
    torch.cuda.synchronize()
    st = stats.cpu().numpy().reshape(steps, 2, net.d.Kp)[:, :, :K]
    c = np.float32(net.var_add)
    assert c == np.float32(np.float32(U * U - 1) * np.float32(O.BN_EPS))
    mm, mv = np.zeros(K), np.ones(K)
    for s in range(steps):
        xd = q[perm[s * batch:(s + 1) * batch]].astype(np.float64) / U
        mean, var = xd.mean(0), xd.var(0)
        assert np.abs(st[s, 0] / U - mean).max() < 1e-6 * max(1.0, np.abs(mean).max())
        assert np.abs((st[s, 1].astype(np.float64) - c) / U ** 2 - var).max() < 2e-6, s
        # what every reader computes from the compensated variance: rstd of q = rstd of d / 63
        rq = 1.0 / np.sqrt(st[s, 1] + np.float32(O.BN_EPS), dtype=np.float32)
        assert np.abs(rq.astype(np.float64) * U / (1.0 / np.sqrt(var + O.BN_EPS)) - 1).max() < 2e-6
        mm = mm * O.BN_MOMENTUM + mean * (1 - O.BN_MOMENTUM)
        mv = mv * O.BN_MOMENTUM + var * (1 - O.BN_MOMENTUM)
    p = net.export_params()                            # back in dosage units
    assert np.abs(p["mov_mean"] - mm).max() < 2e-6 and np.abs(p["mov_var"] - mv).max() < 2e-5


# ------------------------------------------------------------------ training against the oracle on q / 63
def _dosage_problem(n, K, width, nlayers, seed):
    x, y, p, rng = make_problem(n, K, width, nlayers, seed=seed)
    q = np.clip(np.rint((x + rng.normal(0, 0.15, x.shape)) * U), 0, 2 * U).astype(np.uint8)
    return q, q.astype(np.float64) / U, y, p, rng


def test_one_step_matches_the_oracle_on_q_over_63():
    from locator_amd.train import EpochRunner
    q, xd, y, p, rng = _dosage_problem(64, 500, 256, 10, 1)
    net = build_net(q, y, p, drop_p=0.25, seed=2, unit=U)
    assert np.abs(net.export_params()["mov_var"] - p["mov_var"]).max() < 1e-6       # the import / export round trip
    tr, va = np.arange(0, 32), np.arange(32, 64)
    runner = EpochRunner(net, tr, va, 32, use_graph=False)
    perm = rng.permutation(32)
    loss, _ = runner.run_epoch(perm)
    mask = runner.masks.cpu().numpy().reshape(32, net.d.Hp)[:, :256]
    pr = O.copy_params(p)
    m, v = O.zeros_like_trainable(pr), O.zeros_like_trainable(pr)
    ref = O.train_step(pr, m, v, 1, 1e-3, xd[tr][perm], y[tr][perm], mask, 0.25)
    assert abs(loss - ref) < 2e-5, (loss, ref)
    err = params_err(net.export_params(), pr)
    assert max(err.values()) < 2e-5, err


def test_eight_epoch_fit_matches_oracle_fit_on_q_over_63():
    from locator_amd.train import EpochRunner
    K, width, nlayers = 600, 64, 4
    q, xd, y, p, rng = _dosage_problem(130, K, width, nlayers, 21)
    tr, va, pr_rows = np.arange(0, 100), np.arange(100, 120), np.arange(120, 130)
    net = build_net(q, y, p, drop_p=0.25, seed=11, unit=U)
    runner = EpochRunner(net, tr, va, 32, use_graph=True)
    assert runner.chain                                 # the chained kernel reads the compensated variance as it stands
    perms = [np.random.default_rng(100 + e).permutation(100) for e in range(8)]
    masks, hist = [], {"loss": [], "val_loss": []}
    for e in range(8):
        l, vl = runner.run_epoch(perms[e])
        masks.append(runner.masks.cpu().numpy().reshape(runner.steps, 32, net.d.Hp).copy())
        hist["loss"].append(l)
        hist["val_loss"].append(vl)
    pref = O.copy_params(p)
    href, _ = O.fit(pref, xd[tr], y[tr], xd[va], y[va], batch_size=32, max_epochs=8, patience=100, drop_p=0.25,
                    perm_fn=lambda e: perms[e], mask_fn=lambda e, s, nb: masks[e][s, :nb, :width])
    assert maxerr(hist["loss"], href["loss"]) < 5e-4, (hist["loss"], href["loss"])
    assert maxerr(hist["val_loss"], href["val_loss"]) < 5e-4
    yhat = torch.zeros((10, 2), device="cuda")
    net.predict_rows(torch.from_numpy(pr_rows.astype(np.int32)).cuda(), 10, yhat)
    torch.cuda.synchronize()
    ref = O.predict(pref, xd[pr_rows])
    rel = np.abs(yhat.cpu().numpy() - ref) / np.maximum(np.abs(ref), 1.0)
    assert rel.max() < 1e-3, rel.max()
    pd_ = net.export_params()
    assert np.abs(pd_["mov_mean"] - pref["mov_mean"]).max() < 1e-4 and np.abs(pd_["mov_var"] - pref["mov_var"]).max() < 1e-4


@pytest.mark.parametrize("mode, digits", [("exact", 3), ("fast", 2), ("auto", 0)])
def test_every_predict_mode_at_100k_snps_with_values_up_to_126(mode, digits):
    from locator_amd.net import LocatorNet, upload_genotypes
    from tests.gpu_util import randomize_params
    n, K = 640, 100_000
    rng = np.random.default_rng(5)
    q = rng.integers(0, 127, (n, K), dtype=np.uint8)
    q[:, :50] = 126
    xd = q.astype(np.float64) / U
    p = randomize_params(O.init_params(K, 256, 4, rng), rng)
    p["mov_mean"] = xd.mean(0)
    p["mov_var"] = xd.var(0) + 0.05
    X = upload_genotypes(q)
    Y = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
    net = LocatorNet(X, Y, K, 256, 4, 0.25, seed=1, predict_digits=digits, unit=U)
    net.import_params(O.cast_params(p, np.float32))
    assert net.genotype_max() == 126
    yhat = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
    net.predict_rows(torch.arange(n, dtype=torch.int32, device="cuda"), n, yhat)
    torch.cuda.synchronize()
    assert net._image_mode != 0                         # the many-row image path (int8 planes or bf16 pieces) ran
    ref = O.predict(O.cast_params(O.cast_params(p, np.float32), np.float64), xd, batch=128)
    err = np.abs(yhat.cpu().numpy() - ref).max()
    if mode == "exact":
        assert err < 2e-5, err
    assert err / np.abs(ref).max() < 1e-3, (err, np.abs(ref).max())


# ------------------------------------------------------------------ command line
def _run(argv):
    np.random.seed(None)
    assert L.main(argv) == 0


def _pred(path):
    return pd.read_csv(path)[["x", "y"]].to_numpy()


def test_ds_equal_to_the_gt_count_matches_the_gt_run(tmp_path):
    v = G.read_vcf(VCF)
    keep = clean_biallelic(v["calldata/GT"])
    gt, pos, samples = v["calldata/GT"][keep], v["variants/POS"][keep], v["samples"]
    gvcf, vcf = str(tmp_path / "gt.vcf.gz"), str(tmp_path / "ds.vcf.gz")
    write_gt_vcf(gvcf, gt, samples, pos)
    write_dosage_vcf(vcf, (gt == 1).sum(axis=2).astype(np.float32), samples, pos)
    common = ["--sample_data", SAMPLES, "--seed", "12345", "--net_seed", "7", "--max_epochs", "5", "--keras_verbose", "0",
              "--plot_history", ""]
    _run(["--vcf", gvcf, "--out", str(tmp_path / "gt")] + common)
    _run(["--vcf", vcf, "--out", str(tmp_path / "ds"), "--dosage"] + common)
    a, b = _pred(str(tmp_path / "ds_predlocs.txt")), _pred(str(tmp_path / "gt_predlocs.txt"))
    # The two fits differ by fp32 round-off only (q * scale / 63 against x * scale), amplified by five epochs of a ten-layer
    # net: the bar is test_gpu_cli's for such runs (--no_chain), 1e-3 of the coordinate span (0..50)
    dev = np.abs(a - b).max()
    print(f"DS = GT count against GT: predlocs max |dev| {dev:.4f}, "
          f"relative {(np.abs(a - b) / np.maximum(np.abs(b), 1.0)).max():.2e}")
    assert a.shape == b.shape and dev < 0.05, dev
    ha, hb = (pd.read_csv(str(tmp_path / f"{t}_history.txt"), sep="\t") for t in ("ds", "gt"))
    assert len(ha) == len(hb) == 5 and np.abs(ha["loss"] - hb["loss"]).max() < 1e-3


def test_cli_single_bootstrap_and_jacknife_on_noisy_dosages(tmp_path, capsys):
    c, samples, pos = golden_counts()
    vcf = str(tmp_path / "n.vcf.gz")
    write_dosage_vcf(vcf, noisy_dosage(c, missing=0.01), samples, pos, "GP")
    common = ["--vcf", vcf, "--dosage", "GP", "--sample_data", SAMPLES, "--seed", "3", "--keras_verbose", "0"]
    _run(common + ["--out", str(tmp_path / "s"), "--max_epochs", "150", "--patience", "20", "--keep_weights"])
    s = _pred(str(tmp_path / "s_predlocs.txt"))
    assert np.isfinite(s).all() and len(s) > 0
    out = capsys.readouterr().out
    err = float(out.split("mean validation error ")[1].split()[0])
    assert err < 15, err                                 # it learns (a 0-50 map; the GT run's README band is ~4)
    w = np.load(str(tmp_path / "s.weights.npz"))         # moving statistics written in dosage units
    assert 0 <= w["moving_mean"].min() and w["moving_mean"].max() <= 2 and w["moving_variance"].max() < 1.5
    _run(common + ["--out", str(tmp_path / "lw"), "--load_weights", str(tmp_path / "s.weights.npz")])
    assert np.abs(_pred(str(tmp_path / "lw_predlocs.txt")) - s).max() < 1e-3 * max(1.0, np.abs(s).max())
    _run(common + ["--out", str(tmp_path / "b"), "--bootstrap", "--nboots", "2", "--max_epochs", "3", "--in_process"])
    for tag in ("FULL", "0", "1"):
        assert np.isfinite(_pred(str(tmp_path / f"b_boot{tag}_predlocs.txt"))).all()
    _run(common + ["--out", str(tmp_path / "j"), "--jacknife", "--nboots", "3", "--max_epochs", "3"])
    for tag in ("FULL", "0", "1", "2"):
        assert np.isfinite(_pred(str(tmp_path / f"j_boot{tag}_predlocs.txt"))).all()


def test_cli_windows_on_calldata_ds_device_and_host_filter_agree(tmp_path):
    c, samples, pos = golden_counts()
    store = str(tmp_path / "w.zarr")
    write_dosage_zarr(store, noisy_dosage(c, missing=0.01), samples, pos, chunk_variants=4096, with_gt=False)
    common = ["--zarr", store, "--dosage", "--sample_data", SAMPLES, "--seed", "12345", "--net_seed", "4", "--windows",
              "--window_size", "1250000", "--max_epochs", "3", "--patience", "3", "--keras_verbose", "0", "--gpus", "1",
              "--in_process"]
    _run(common + ["--out", str(tmp_path / "dev")])
    _run(common + ["--out", str(tmp_path / "host"), "--host_filter"])
    size = 1250000
    n = 0
    for i in (0, size):
        a = _pred(f"{tmp_path}/dev_{i}-{i + size - 1}_0-{size - 1}_predlocs.txt")
        b = _pred(f"{tmp_path}/host_{i}-{i + size - 1}_0-{size - 1}_predlocs.txt")
        assert np.array_equal(a, b) and np.isfinite(a).all()
        n += 1
    assert n == 2 and os.path.exists(str(tmp_path / "dev_params.json"))
