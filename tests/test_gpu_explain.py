"""`python -m locator_amd.explain` on the device: loc_explain_stack_grad / loc_explain_sites / loc_explain_reduce against the
float64 NumPy forms of tests/test_explain.py (locator_amd/explain.py), absent sites, run-to-run identity, a case past 2^31
genotype bytes, and the command end to end on models trained from the example data."""
import os

import numpy as np
import pandas as pd
import pytest
import torch

from locator_amd import explain as E
from locator_amd import locator as L
from locator_amd import query as Q
from locator_amd.net import upload_genotypes
from oracle import locator_oracle as O
from tests.gpu_util import make_problem

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
VCF = os.path.join(GOLD, "test_genotypes.vcf.gz")
SAMPLES = os.path.join(GOLD, "test_sample_data.txt")
SHORT = ["--max_epochs", "3", "--patience", "3", "--keras_verbose", "0", "--plot_history", ""]
LOCS = [3.0, 2.5, -1.0, 1.5]


def _model(p, K, width, nlayers):
    return {"K": K, "width": width, "nlayers": nlayers, "weights_used": O.cast_params(p, np.float32), "locs_norm": LOCS}


def _device(model, X, n):
    K = model["K"]
    col_site = np.arange(K)
    net, d1 = E.device_delta1(model, X)
    del net
    p = model["weights_used"]
    U = E.fold_first_layer(p, col_site, K).astype(np.float32)
    stats = E.device_sites(d1, n, U, X, np.asarray(p["mov_mean"], np.float64))
    Hp = d1.shape[1]
    return d1.cpu().numpy().astype(np.float64).reshape(n, 2, Hp), stats


@pytest.mark.parametrize("n,K,width,nlayers", [(1, 1, 64, 1), (33, 31, 64, 2), (1, 33, 256, 10), (33, 5830, 256, 10),
                                               (1000, 33, 512, 2), (1000, 5830, 256, 1), (33, 31, 1024, 2),
                                               (1000, 5830, 1024, 10), (200, 100, 48, 3)])
def test_kernels_match_the_float64_form(n, K, width, nlayers):
    x, _, p, rng = make_problem(n, K, width, nlayers, seed=n + K + width + nlayers)
    absent = rng.random(K) < 0.1
    p["gamma"][absent] = 0.0                              # absent sites (predict's gamma = 0): exact zeros
    m = _model(p, K, width, nlayers)
    p64 = O.cast_params(m["weights_used"], np.float64)
    d1, stats = _device(m, upload_genotypes(x), n)
    ref_d1 = E.reference_delta1(p64, x, LOCS)
    H = ref_d1.shape[2]
    assert not d1[:, :, H:].any()
    scale = np.abs(ref_d1).max(axis=2, keepdims=True) + 1e-30
    assert (np.abs(d1[:, :, :H] - ref_d1) / scale).max() <= 1e-5
    _, ref = E.reference_stats(ref_d1, E.fold_first_layer(p64, np.arange(K), K), x, p64["mov_mean"])
    tol = 1e-4 * np.abs(ref) + 1e-7 * np.abs(ref).max(axis=1, keepdims=True)
    assert (np.abs(stats - ref) <= tol).all(), np.abs(stats - ref).max(axis=1)
    assert (stats[:, absent] == 0).all()
    assert (stats[:, ~absent] > 0).any()


def test_two_runs_are_bit_identical():
    x, _, p, _ = make_problem(300, 1000, 256, 3, seed=5)
    m = _model(p, 1000, 256, 3)
    X = upload_genotypes(x)
    a = _device(m, X, 300)
    b = _device(m, X, 300)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_past_2_31_genotype_bytes():
    """n * Kp > 2^31: the epilogue's genotype reads and the layer-1 rows use 64-bit offsets.  A fixed random subset of sites
    (the last one included) against the float64 form computed from the device's own delta1."""
    n, K, width = 4200, 512000, 64
    assert n * ((K + 31) // 32 * 32) > 2 ** 31
    rng = np.random.default_rng(11)
    p = O.init_params(K, width, 2, rng)
    p["gamma"] = rng.uniform(0.7, 1.3, K)
    p["mov_mean"] = rng.uniform(0, 1, K)
    p["mov_var"] = rng.uniform(0.2, 1.2, K)
    m = _model(p, K, width, 2)
    g = torch.Generator(device="cuda").manual_seed(3)
    X = torch.randint(0, 3, (n, (K + 31) // 32 * 32), dtype=torch.uint8, device="cuda", generator=g)
    X[:, K:] = 0
    d1, stats = _device(m, X, n)
    del X
    torch.cuda.empty_cache()
    cols = np.unique(np.concatenate([rng.choice(K, 40, replace=False), [0, K - 1]]))
    X = torch.randint(0, 3, (n, (K + 31) // 32 * 32), dtype=torch.uint8, device="cuda",
                      generator=torch.Generator(device="cuda").manual_seed(3))
    xs = X[:, torch.from_numpy(cols).cuda()].cpu().numpy()
    del X
    p64 = O.cast_params(m["weights_used"], np.float64)
    U = E.fold_first_layer(p64, np.arange(K), K)[cols]
    _, ref = E.reference_stats(d1[:, :, :width], U, xs, p64["mov_mean"][cols])
    np.testing.assert_allclose(stats[:, cols], ref, rtol=1e-4, atol=1e-7 * np.abs(ref).max())


# ------------------------------------------------------------------ the command on trained models
def _run(argv):
    np.random.seed(None)
    assert L.main(argv) == 0


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    d = tmp_path_factory.mktemp("explain_train")
    common = ["--vcf", VCF, "--sample_data", SAMPLES, "--keep_model"] + SHORT
    _run(common + ["--seed", "12345", "--out", str(d / "a")])
    _run(common + ["--seed", "777", "--out", str(d / "b")])
    _run(common + ["--seed", "99", "--phased", "--out", str(d / "ph")])
    return d


def _expected(model_path, rows_of):
    """float64 statistics from the .model.npz weights and the query rows (model columns), as predict builds them."""
    m = Q.load_model(model_path)
    q = Q.read_query(vcf=VCF)
    cv, ca, _ = Q.match_sites(m, q)
    p = O.cast_params(Q.absent_gamma(m["weights"], cv), np.float64)
    col_site, first = E.site_index(m)
    gt = q["gt"]
    if m["phased"]:
        gt = gt.reshape(gt.shape[0], -1, 1)
    x = np.stack([(gt[cv[k]][rows_of(gt.shape[1])] == ca[k]).sum(axis=1) for k in range(m["K"])], axis=1)
    d1 = E.reference_delta1(p, x, m["locs_norm"])
    _, ref = E.reference_stats(d1, E.fold_first_layer(p, col_site, len(first)), x[:, first], p["mov_mean"][first])
    return m, ref


def test_command_end_to_end(tmp_path, trained):
    out = str(tmp_path / "e")
    assert E.main(["--model", str(trained / "a.model.npz"), "--vcf", VCF, "--out", out, "--window_size", "100000"]) == 0
    t = pd.read_csv(out + "_snp_importance.txt", sep="\t", dtype={"chrom": str})
    assert list(t.columns) == ["chrom", "pos", "ref", "alt", "columns", "present"] + list(E.STATS)
    m, ref = _expected(str(trained / "a.model.npz"), lambda N: np.arange(N))
    assert len(t) == len(E.site_index(m)[1]) and (t["present"] == 1).all() and (t["columns"] >= 1).all()
    np.testing.assert_allclose(t[list(E.STATS)].to_numpy().T, ref, rtol=1e-4, atol=1e-7 * np.abs(ref).max())
    w = pd.read_csv(out + "_window_importance.txt", sep="\t", dtype={"chrom": str})
    assert list(w.columns) == ["chrom", "start", "stop", "sites", "mean_abs_x", "mean_abs_y", "mean_dist"]
    assert w["sites"].sum() == len(t) and ((w["stop"] - w["start"]) == 100000).all()
    np.testing.assert_allclose(w["mean_dist"].sum(), t["mean_dist"].sum(), rtol=1e-9)
    # a second run writes byte-identical files
    out2 = str(tmp_path / "e2")
    assert E.main(["--model", str(trained / "a.model.npz"), "--vcf", VCF, "--out", out2, "--window_size", "100000"]) == 0
    for suffix in ("_snp_importance.txt", "_window_importance.txt"):
        assert open(out + suffix, "rb").read() == open(out2 + suffix, "rb").read()


def test_command_phased_model(tmp_path, trained):
    out = str(tmp_path / "p")
    assert E.main(["--model", str(trained / "ph.model.npz"), "--vcf", VCF, "--out", out]) == 0
    t = pd.read_csv(out + "_snp_importance.txt", sep="\t", dtype={"chrom": str})
    _, ref = _expected(str(trained / "ph.model.npz"), lambda N: np.arange(N))
    assert (t["present"] == 1).all()
    np.testing.assert_allclose(t[list(E.STATS)].to_numpy().T, ref, rtol=1e-4, atol=1e-7 * np.abs(ref).max())


def test_command_two_models(tmp_path, trained):
    out = str(tmp_path / "two")
    assert E.main(["--model", str(trained / "a.model.npz"), str(trained / "b.model.npz"), "--vcf", VCF, "--out", out]) == 0
    assert not os.path.exists(out + "_snp_importance.txt")
    for stem in ("a", "b"):
        t = pd.read_csv(f"{out}_{stem}_snp_importance.txt", sep="\t", dtype={"chrom": str})
        _, ref = _expected(str(trained / f"{stem}.model.npz"), lambda N: np.arange(N))
        np.testing.assert_allclose(t[list(E.STATS)].to_numpy().T, ref, rtol=1e-4, atol=1e-7 * np.abs(ref).max())
