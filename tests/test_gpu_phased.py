"""--phased on the device: the window filter kernels at ploidy 1 (the calls viewed as [variants][2N haplotypes][1]) against
the host haplotype rows, and the command line with --phased in every mode - single run against the oracle, --load_weights,
accuracy on the reference's example data, --windows (device and host filters, eager --impute_missing), --bootstrap in and
out of process, and --jacknife as one batched predict."""
import os
import time

import numpy as np
import pandas as pd
import pytest
import torch

from locator_amd import genotypes as G
from locator_amd import locator as L

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
VCF = os.path.join(GOLD, "test_genotypes.vcf.gz")
SAMPLES = os.path.join(GOLD, "test_sample_data.txt")
SHORT = ["--max_epochs", "3", "--patience", "3", "--keras_verbose", "0", "--plot_history", ""]
HAP_IDS = [f"msp_{i}_h{h}" for i in range(50) for h in (0, 1)]


def _run(argv):
    np.random.seed(None)
    assert L.main(argv) == 0


@pytest.fixture(scope="module")
def fixture_vcf():
    return G.read_vcf(VCF)


# ------------------------------------------------------------------ device filter at ploidy 1
def _host_rows(gt, order, min_mac):
    ac = G.filter_snps(G.haplotypes(gt), min_mac=min_mac, verbose=False)            # (K, 2N)
    return np.ascontiguousarray(ac[:, order].T).astype(np.uint8), ac.shape[0]


def _device_rows(gt, order, min_mac):
    from locator_amd.net import filter_snps_device
    V, N, P = gt.shape
    d = torch.from_numpy(np.ascontiguousarray(gt)).cuda().view(V, N * P, 1)
    X, K = filter_snps_device(d, order, min_mac)
    torch.cuda.synchronize()
    return X.cpu().numpy(), K


def test_device_filter_at_ploidy_1_on_the_fixture(fixture_vcf):
    gt = np.array(fixture_vcf["calldata/GT"], dtype=np.int8)
    order = np.random.default_rng(1).permutation(2 * gt.shape[1]).astype(np.int32)
    ref, K = _host_rows(gt, order, 2)
    X, Kd = _device_rows(gt, order, 2)
    assert K == Kd == 5830 and np.array_equal(X[:, :K], ref) and not X[:, K:].any()


@pytest.mark.parametrize("min_mac", [1, 2])
def test_device_filter_at_ploidy_1_window_sized(min_mac):
    """BASELINE configs[3] window: 150,000 variants x 765 individuals = 1,530 haplotype rows (two 960-row chunks of the
    rows kernel), some missing alleles, rare sites that only min_mac 1 keeps."""
    rng = np.random.default_rng(30 + min_mac)
    V, N = 150_000, 765
    af = rng.beta(0.3, 0.9, V).astype(np.float32)
    af[rng.random(V) < 0.05] = 0.5 / (2 * N)                                       # singleton-ish sites
    gt = (rng.random((V, N, 2), dtype=np.float32) < af[:, None, None]).astype(np.int8)
    gt[rng.random((V, N, 2), dtype=np.float32) < 0.01] = -1
    order = rng.permutation(2 * N).astype(np.int32)
    ref, K = _host_rows(gt, order, min_mac)
    X, Kd = _device_rows(gt, order, min_mac)
    assert Kd == K and np.array_equal(X[:, :K], ref)


# ------------------------------------------------------------------ single run, --load_weights, accuracy
def test_phased_run_matches_the_oracle_and_load_weights_reproduces_it(tmp_path, fixture_vcf):
    from oracle import locator_oracle as O
    a = str(tmp_path / "a")
    common = ["--vcf", VCF, "--sample_data", SAMPLES, "--seed", "12345", "--phased", "--predict_mode", "exact"] + SHORT
    _run(common + ["--out", a, "--keep_weights"])
    got = pd.read_csv(a + "_predlocs.txt")
    assert list(got["sampleID"]) == HAP_IDS
    # the host-built haplotype rows of the 50 individuals without coordinates (msp_0..msp_49 -> rows 0..99)
    H = G.filter_snps(G.haplotypes(fixture_vcf["calldata/GT"]), min_mac=2, verbose=False)
    predgen = np.ascontiguousarray(H[:, :100].T)
    p = O.cast_params(L.read_weights(a + ".weights.npz"), np.float64)
    z = O.predict(p, predgen)
    sd = pd.read_csv(SAMPLES, sep="\t")
    mx, sx, my, sy = sd["x"].mean(), sd["x"].std(ddof=0), sd["y"].mean(), sd["y"].std(ddof=0)
    assert np.abs(got["x"].to_numpy() - (z[:, 0] * sx + mx)).max() < 2e-5 * sx + 1e-9
    assert np.abs(got["y"].to_numpy() - (z[:, 1] * sy + my)).max() < 2e-5 * sy + 1e-9
    assert not np.allclose(got["x"][0::2], got["x"][1::2])                 # the two haplotypes are predicted apart
    b = str(tmp_path / "b")
    _run(common + ["--out", b, "--load_weights", a + ".weights.npz"])
    assert open(a + "_predlocs.txt").read() == open(b + "_predlocs.txt").read()


def _metrics(txt):
    g = lambda key: float(txt.split(key)[1].split("\n")[0])
    return g("R2(x)="), g("R2(y)="), g("mean validation error "), g("median validation error ")


def test_full_default_phased_run_lands_in_a_band(tmp_path, capsys):
    """Every default, --seed 12345, one row per haplotype: 810 training and 90 validation haplotypes (45 individuals).
    Measured on an MI355X: R2 0.920 / 0.929, mean validation error 4.53 (median 3.21) after 158 epochs - below the
    unphased run's 0.961 / 0.971 and 3.27 (a haplotype carries half an individual's alleles); the band keeps a margin."""
    out = str(tmp_path / "d")
    t0 = time.time()
    _run(["--vcf", VCF, "--sample_data", SAMPLES, "--out", out, "--seed", "12345", "--phased", "--keras_verbose", "0",
          "--plot_history", ""])
    wall = time.time() - t0
    txt = capsys.readouterr().out
    r2x, r2y, mean_err, med_err = _metrics(txt)
    h = pd.read_csv(out + "_history.txt", sep="\t")
    print(f"phased default run: R2 {r2x:.4f} / {r2y:.4f}, mean error {mean_err:.3f}, median {med_err:.3f}, "
          f"{len(h)} epochs, {wall:.2f} s")
    assert "validation on 90 haplotypes (45 individuals)" in txt
    assert r2x > 0.87 and r2y > 0.87 and mean_err < 6.0, (r2x, r2y, mean_err)
    assert 50 <= len(h) <= 600 and h["learning_rate"].iloc[-1] < 1e-3         # early stopping and the LR plateau acted
    assert len(pd.read_csv(out + "_predlocs.txt")) == 100


# ------------------------------------------------------------------ replicate modes
@pytest.fixture(scope="module")
def store(tmp_path_factory, fixture_vcf):
    gt = np.array(fixture_vcf["calldata/GT"], dtype=np.int8)
    gt[np.random.default_rng(3).random(gt.shape) < 0.02] = -1            # missing alleles on the filters' path
    path = str(tmp_path_factory.mktemp("phased") / "fix.zarr")
    G.write_callset_zarr(path, gt, fixture_vcf["variants/POS"], fixture_vcf["samples"], chunk_variants=4096,
                         compressor="blosc")
    return path


def _window_files(d):
    return sorted(f for f in os.listdir(d) if f.endswith("_predlocs.txt") or f.endswith("_history.txt"))


def test_phased_windows_device_filter_equals_host_filter(tmp_path, store, monkeypatch):
    from locator_amd import net
    seen = []
    real = net.filter_snps_device

    def spy(gt, order, min_mac=2):
        seen.append((tuple(gt.shape), len(order)))
        return real(gt, order, min_mac)
    monkeypatch.setattr(net, "filter_snps_device", spy)
    common = ["--zarr", store, "--sample_data", SAMPLES, "--seed", "4242", "--phased", "--windows", "--window_size",
              "1250000", "--predict_mode", "exact"] + SHORT
    (tmp_path / "dev").mkdir()
    (tmp_path / "host").mkdir()
    _run(common + ["--out", str(tmp_path / "dev" / "r"), "--in_process"])           # the device filter, spied on
    _run(common + ["--out", str(tmp_path / "host" / "r"), "--host_filter"])         # host filter, in a worker process
    assert len(seen) == 2 and all(shape[1:] == (1000, 1) and n_rows == 1000 for shape, n_rows in seen)    # 2N rows, ploidy 1
    files = _window_files(tmp_path / "dev")
    assert files == _window_files(tmp_path / "host") and len(files) == 4
    for f in files:
        assert (tmp_path / "dev" / f).read_bytes() == (tmp_path / "host" / f).read_bytes(), f
        if f.endswith("_predlocs.txt"):
            assert list(pd.read_csv(tmp_path / "dev" / f)["sampleID"]) == HAP_IDS


def test_phased_windows_impute_missing_runs_the_eager_host_path(tmp_path, store, monkeypatch):
    from locator_amd import net
    monkeypatch.setattr(net, "filter_snps_device", lambda *a, **k: (_ for _ in ()).throw(AssertionError("device filter")))
    out = str(tmp_path / "i")
    _run(["--zarr", store, "--sample_data", SAMPLES, "--out", out, "--seed", "4242", "--phased", "--windows",
          "--window_size", "1250000", "--impute_missing", "--in_process"] + SHORT)
    files = [f for f in _window_files(tmp_path) if f.endswith("_predlocs.txt")]
    assert len(files) == 2
    for f in files:
        assert list(pd.read_csv(tmp_path / f)["sampleID"]) == HAP_IDS


def test_phased_bootstrap_in_process_equals_worker_process(tmp_path):
    common = ["--vcf", VCF, "--sample_data", SAMPLES, "--seed", "54321", "--phased", "--bootstrap", "--nboots", "2",
              "--predict_mode", "exact"] + SHORT
    for name, extra in (("inp", ["--in_process"]), ("wrk", [])):
        (tmp_path / name).mkdir()
        _run(common + ["--out", str(tmp_path / name / "b")] + extra)
    for b in ("FULL", "0", "1"):
        f = f"b_boot{b}_predlocs.txt"
        x, y = (tmp_path / "inp" / f).read_bytes(), (tmp_path / "wrk" / f).read_bytes()
        assert x == y, f
        assert list(pd.read_csv(tmp_path / "inp" / f)["sampleID"]) == HAP_IDS
    assert (tmp_path / "inp" / "b_history.txt").read_bytes() == (tmp_path / "wrk" / "b_history.txt").read_bytes()


def test_phased_jacknife_is_one_batched_predict_of_0_1_rows(tmp_path, monkeypatch):
    recorded = {}
    real_draws, real_predict = L.jacknife_draws, L.Model.predict

    def spy_draws(predgen, af, nboots, prop, ploidy=2):
        recorded["ploidy"] = ploidy
        recorded["draws"] = real_draws(predgen, af, nboots, prop, ploidy=ploidy)
        return recorded["draws"]

    def spy_predict(self, gen):
        recorded.setdefault("rows", []).append(gen.shape[0])
        if not isinstance(gen, L.DeviceRows):
            recorded.setdefault("values", set()).update(np.unique(np.asarray(gen)).tolist())
        return real_predict(self, gen)
    monkeypatch.setattr(L, "jacknife_draws", spy_draws)
    monkeypatch.setattr(L.Model, "predict", spy_predict)
    out = str(tmp_path / "j")
    _run(["--vcf", VCF, "--sample_data", SAMPLES, "--out", out, "--seed", "7", "--phased", "--jacknife", "--nboots", "3"]
         + SHORT)
    assert recorded["ploidy"] == 1 and recorded["rows"][-1] == 3 * 100
    assert recorded["values"] <= {0, 1}
    assert all(set(np.unique(v).tolist()) <= {0, 1} for _, v in recorded["draws"])
    for b in ("FULL", "0", "1", "2"):
        assert list(pd.read_csv(f"{out}_boot{b}_predlocs.txt")["sampleID"]) == HAP_IDS
