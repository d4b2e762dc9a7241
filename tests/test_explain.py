"""`python -m locator_amd.explain`, host side: the float64 NumPy form of the per-site Jacobian / attribution against central
finite differences of the oracle's inference forward, the fold of repeated columns, the window table, and the refusals
(all before any device work); the kernel-level forms of tests/explain_util.py against these, the float32 floor of every case
of tests/test_gpu_explain_kernels.py, and loc_explain_splits against the launcher's rule.  Nothing here needs a GPU;
tests/test_gpu_explain.py and tests/test_gpu_explain_kernels.py hold the kernels to these forms."""
import json
import os

import numpy as np
import pytest

from locator_amd import _lib
from locator_amd import explain as E
from locator_amd import locator as L
from locator_amd import query as Q
from oracle import locator_oracle as O
from tests import explain_util as XU

GOLD = os.path.join(os.path.dirname(__file__), "golden")
VCF = os.path.join(GOLD, "test_genotypes.vcf.gz")
LOCS = [3.0, 2.5, -1.0, 1.5]          # meanlong, sdlong, meanlat, sdlat


def _toy(K=37, width=16, nlayers=2, n=5, seed=0):
    rng = np.random.default_rng(seed)
    p = O.init_params(K, width, nlayers, rng)
    p["gamma"] = rng.uniform(0.7, 1.3, K)
    p["beta"] = rng.normal(0, 0.05, K)
    p["mov_mean"] = rng.uniform(0, 1, K)
    p["mov_var"] = rng.uniform(0.2, 1.2, K)
    for l in range(len(p["b"])):
        p["b"][l] = rng.normal(0, 0.05, p["b"][l].shape)
    x = rng.integers(0, 3, (n, K)).astype(np.float64)
    return p, x


def _map_units(p, x):
    z, _ = O.forward(p, x, training=False)
    return z * np.array([LOCS[1], LOCS[3]]) + np.array([LOCS[0], LOCS[2]])


def _fd_jacobian(p, x, col_site, Ks, eps=1e-5):
    """Central differences of the map-unit prediction: site s moves every one of its columns together."""
    n = x.shape[0]
    J = np.zeros((n, 2, Ks))
    for s in range(Ks):
        on = col_site == s
        xp, xm = x.copy(), x.copy()
        xp[:, on] += eps
        xm[:, on] -= eps
        J[:, :, s] = (_map_units(p, xp) - _map_units(p, xm)) / (2 * eps)
    return J


@pytest.mark.parametrize("nlayers", [1, 2, 3, 10])
def test_reference_jacobian_matches_finite_differences(nlayers):
    p, x = _toy(nlayers=nlayers, seed=nlayers)
    K = x.shape[1]
    col_site = np.arange(K)
    d1 = E.reference_delta1(p, x, LOCS)
    J, stats = E.reference_stats(d1, E.fold_first_layer(p, col_site, K), x, p["mov_mean"])
    fd = _fd_jacobian(p, x, col_site, K)
    assert np.abs(J - fd).max() <= 1e-6 * max(1.0, np.abs(fd).max())
    # the four statistics restated from the finite-difference Jacobian
    A = fd * (x - p["mov_mean"])[:, None, :]
    want = [np.abs(A[:, 0]).mean(0), np.abs(A[:, 1]).mean(0), np.hypot(A[:, 0], A[:, 1]).mean(0),
            np.sqrt((fd ** 2).sum(1).mean(0))]
    np.testing.assert_allclose(stats, np.array(want), rtol=1e-5, atol=1e-9)


def test_repeated_columns_fold_into_one_site():
    """A bootstrap-style model (columns 0 and 5 are one site, 3 and 9 and 11 another): J per site is the derivative with
    respect to moving all of the site's columns together, and the statistics are taken after the fold."""
    p, x = _toy(K=13, width=16, nlayers=3, seed=7)
    dup = {5: 0, 9: 3, 11: 3}
    for c, c0 in dup.items():
        x[:, c] = x[:, c0]
        p["mov_mean"][c] = p["mov_mean"][c0]
    chrom = np.array(["1"] * 13)
    pos = np.arange(13) * 100
    for c, c0 in dup.items():
        pos[c] = pos[c0]
    model = {"chrom": chrom, "pos": pos, "ref": np.array(["A"] * 13), "alt": np.array(["T"] * 13)}
    col_site, first = E.site_index(model)
    assert len(first) == 10 and first.tolist() == [0, 1, 2, 3, 4, 6, 7, 8, 10, 12]
    assert col_site[5] == col_site[0] and col_site[9] == col_site[3] == col_site[11]
    U = E.fold_first_layer(p, col_site, len(first))
    J, stats = E.reference_stats(E.reference_delta1(p, x, LOCS), U, x[:, first], p["mov_mean"][first])
    np.testing.assert_allclose(J, _fd_jacobian(p, x, col_site, len(first)), rtol=1e-6, atol=1e-8)
    # summing the statistics of the unfolded columns would be wrong: |.| does not distribute over the sum
    Ju, stats_u = E.reference_stats(E.reference_delta1(p, x, LOCS), E.fold_first_layer(p, np.arange(13), 13), x,
                                    p["mov_mean"])
    np.testing.assert_allclose(J[:, :, col_site[0]], Ju[:, :, 0] + Ju[:, :, 5], rtol=1e-12)
    unfolded = stats_u[0, 0] + stats_u[0, 5]
    assert stats[0, col_site[0]] <= unfolded * (1 + 1e-12)


def test_fold_equals_merged_columns_exactly():
    """Same network, same activations: a model whose repeated columns are merged into one (summed s_c W1[c], the shift
    terms moved into the first bias) gives the same J per site."""
    p, x = _toy(K=9, width=16, nlayers=2, seed=3)
    x[:, 4] = x[:, 1]
    p["mov_mean"][4] = p["mov_mean"][1]
    col_site = np.array([0, 1, 2, 3, 1, 4, 5, 6, 7])
    first = np.array([0, 1, 2, 3, 5, 6, 7, 8])
    U = E.fold_first_layer(p, col_site, 8)
    J, _ = E.reference_stats(E.reference_delta1(p, x, LOCS), U, x[:, first], p["mov_mean"][first])
    q = {"W": [w.copy() for w in p["W"]], "b": [b.copy() for b in p["b"]]}
    s = E.bn_scale(p)
    t = p["beta"] - p["mov_mean"] * s
    q["mov_mean"], q["mov_var"] = p["mov_mean"][first], np.full(8, 1.0 - O.BN_EPS)   # scale = gamma
    q["gamma"] = np.ones(8)
    q["W"][0] = U
    q["beta"] = q["mov_mean"].copy()                                                # shift 0 ...
    q["b"][0] = p["b"][0] + t @ p["W"][0]                                           # ... moved into the bias
    assert np.allclose(_map_units(q, x[:, first]), _map_units(p, x))
    Jm, _ = E.reference_stats(E.reference_delta1(q, x[:, first], LOCS), U, x[:, first], q["mov_mean"])
    np.testing.assert_allclose(J, Jm, rtol=1e-10, atol=1e-12)


def test_site_index_matrix_model_by_name():
    m = {"chrom": np.array(["a", "b", "a", "c"]), "pos": np.full(4, -1), "ref": np.array([""] * 4),
         "alt": np.array([""] * 4)}
    assert E.is_matrix_model(m)
    col_site, first = E.site_index(m)
    assert col_site.tolist() == [0, 1, 0, 2] and first.tolist() == [0, 1, 3]


def test_window_table():
    chrom = ["2", "2", "1", "2", "1", "1"]
    pos = [5, 250, 120, 260, 10, 330]
    present = [1, 1, 1, 0, 1, 1]
    stats = np.array([[1, 2, 3, 4, 5, 6], [10, 20, 30, 40, 50, 60], [100, 200, 300, 400, 500, 600], [0] * 6], float)
    rows = E.window_table(chrom, pos, present, stats, 100)
    assert rows == [("2", 0, 100, 1, 1.0, 10.0, 100.0), ("2", 100, 200, 0, 0.0, 0.0, 0.0), ("2", 200, 300, 1, 2.0, 20.0, 200.0),
                    ("1", 0, 100, 1, 5.0, 50.0, 500.0), ("1", 100, 200, 1, 3.0, 30.0, 300.0), ("1", 200, 300, 0, 0.0, 0.0, 0.0),
                    ("1", 300, 400, 1, 6.0, 60.0, 600.0)]


# ------------------------------------------------------------------ refusals (before any device work)
def _weights(K, width=4, nlayers=2, seed=0):
    p = O.init_params(K, width, nlayers, np.random.default_rng(seed))
    return O.cast_params(p, np.float32)


def _save(path, chrom, pos, ref, alt, phased=False):
    K = len(chrom)
    meta = {"chrom": np.array(chrom, dtype=object), "pos": np.array(pos), "ref": np.array(ref, dtype=object),
            "alt": np.array(alt, dtype=object), "af": np.full(K, 0.5), "locs_norm": LOCS, "ploidy": 2, "phased": phased,
            "params_json": json.dumps({"width": 4, "nlayers": 2, "dropout_prop": 0.25})}
    L.save_model(str(path), _weights(K), meta)
    return str(path)


def _vcf_model(tmp_path, name="run", n_sites=20, phased=False):
    q = Q.read_query(vcf=VCF)
    return _save(tmp_path / f"{name}.model.npz", q["chrom"][:n_sites], q["pos"][:n_sites],
                 [a[0] for a in q["alleles"][:n_sites]], [a[1] for a in q["alleles"][:n_sites]], phased)


def test_refuse_window_size_on_a_matrix_model(tmp_path):
    m = _save(tmp_path / "mat.model.npz", ["s1", "s2", "s3"], [-1, -1, -1], ["", "", ""], ["", "", ""])
    mat = tmp_path / "q.txt"
    mat.write_text("sampleID\ts1\ts2\ts3\nA\t0\t1\t2\nB\t2\t1\t0\n")
    with pytest.raises(Q.QueryRefused, match="--matrix model"):
        E.main(["--model", m, "--matrix", str(mat), "--out", str(tmp_path / "o"), "--window_size", "1000"])


def test_refuse_low_overlap(tmp_path):
    m = _save(tmp_path / "far.model.npz", ["9"] * 4, [1, 2, 3, 4], ["A"] * 4, ["T"] * 4)
    with pytest.raises(Q.QueryRefused, match="min_site_overlap"):
        E.main(["--model", m, "--vcf", VCF, "--out", str(tmp_path / "o")])


def test_refuse_mixed_phased_models_and_shared_stems(tmp_path):
    a = _vcf_model(tmp_path, "a")
    b = _vcf_model(tmp_path, "b", phased=True)
    with pytest.raises(Q.QueryRefused, match="phased and unphased"):
        E.main(["--model", a, b, "--vcf", VCF, "--out", str(tmp_path / "o")])
    os.makedirs(tmp_path / "d")
    c = _save(tmp_path / "d" / "a.model.npz", ["1"], [197], ["A"], ["T"])
    with pytest.raises(Q.QueryRefused, match="share the name stem"):
        E.main(["--model", a, c, "--vcf", VCF, "--out", str(tmp_path / "o")])


def test_refuse_unknown_samples_and_weights_file(tmp_path):
    a = _vcf_model(tmp_path, "a")
    ids = tmp_path / "ids.txt"
    ids.write_text("msp_0\nnobody\n")
    with pytest.raises(Q.QueryRefused, match="not in the query"):
        E.main(["--model", a, "--vcf", VCF, "--samples", str(ids), "--out", str(tmp_path / "o")])
    L.save_weights(str(tmp_path / "w.weights.npz"), _weights(3))
    with pytest.raises(Q.QueryRefused, match="no site table"):
        E.main(["--model", str(tmp_path / "w.weights.npz"), "--vcf", VCF, "--out", str(tmp_path / "o")])


# ------------------------------------------------------------------ the kernel-level forms (tests/explain_util.py)
def _layer1(p, x):
    """BatchNorm (inference) and layer 1 exactly as E.reference_delta1 forms them: a1 (n, H), float64."""
    s = E.bn_scale(p)
    a = x * s + (p["beta"] - p["mov_mean"] * s)
    z = a @ p["W"][0] + p["b"][0]
    return np.where(z > 0, z, np.expm1(np.minimum(z, 0)))


@pytest.mark.parametrize("nlayers", [1, 2, 3, 10])
def test_util_forms_equal_the_package_forms_in_float64(nlayers):
    """The forms the kernel tests use (from layer 1's output; sums per split, then the reduction) against the forms the
    command's tests use (from the genotypes; means).  Same operations in the same order: equal bit for bit.  Splitting the
    samples changes the order of the float64 sums only: 1e-12."""
    p, x = _toy(K=37, width=16, nlayers=nlayers, n=150, seed=40 + nlayers)
    K, n = x.shape[1], x.shape[0]
    want = E.reference_delta1(p, x, LOCS)
    acts, got = XU.ref_delta1(_layer1(p, x), p["W"][1:nlayers], p["b"][1:nlayers], p["W"][nlayers], p["W"][nlayers + 1],
                              (LOCS[1], LOCS[3]), np.float64)
    assert acts.shape == (nlayers - 1, n, 16) and got.dtype == np.float64
    assert np.array_equal(got, want)
    U = E.fold_first_layer(p, np.arange(K), K)
    _, stats = E.reference_stats(want, U, x, p["mov_mean"])
    xs = x.astype(np.uint8)
    assert np.array_equal(XU.ref_out(XU.ref_partial(got, U, xs, p["mov_mean"], (0, n), np.float64), n), stats)
    for splits in XU.accepted_splits(n):                                  # mt = 3: 1, 2, 3
        parts = [XU.ref_partial(got, U, xs, p["mov_mean"], XU.split_range(n, splits, sp), np.float64)
                 for sp in range(splits)]
        np.testing.assert_allclose(XU.ref_out(sum(parts), n), stats, rtol=1e-12, atol=0)
    assert XU.accepted_splits(n) == [1, 2, 3] and XU.accepted_splits(300) == [1, 2, 3, 5]
    assert [XU.split_range(300, 3, sp) for sp in range(3)] == [(0, 128), (128, 256), (256, 300)]


def test_float32_forms_stay_in_float32():
    prob = XU.stack_problem(5, 33, 3)
    acts, d1 = XU.ref_delta1(*[prob[k] for k in ("a1", "Wh", "bh", "wa", "wb", "sd")], np.float32)
    assert acts.dtype == np.float32 and d1.dtype == np.float32 and acts.shape == (2, 5, 33) and d1.shape == (5, 2, 33)
    for k in ("a1", "wa", "wb"):
        assert np.array_equal(prob[k], prob[k].astype(np.float32).astype(np.float64)), k


def test_explain_splits_never_returns_a_count_the_launcher_refuses():
    """loc_explain_splits over n = 1..700, Ks on both sides of the 128-site tile and large, compute units 0 (-> 256), 1, 64,
    256, 304: 1 <= s <= mt and ceil(mt / s) (s - 1) < mt, the rule by which loc_explain_sites takes a split count."""
    lib = _lib.load()
    for cu in (0, 1, 64, 256, 304):
        for Ks in (1, 127, 128, 129, 5000, 200000):
            for n in range(1, 701):
                s = lib.loc_explain_splits(n, Ks, cu)
                mt = -(-2 * n // 128)
                assert 1 <= s <= mt and -(-mt // s) * (s - 1) < mt, (n, Ks, cu, s, mt)
                assert XU.split_accepted(XU.mt_of(n), s) and XU.mt_of(n) == mt
    # few sites and many tiles: the splits fill the device; many sites: one split
    assert lib.loc_explain_splits(700, 1, 256) == 11 and lib.loc_explain_splits(700, 200000, 256) == 1
    assert lib.loc_explain_splits(0, 5, 256) == 1 and lib.loc_explain_splits(-3, 5, 256) == 1
    assert lib.loc_explain_splits(5, 0, 256) == 1 and lib.loc_explain_splits(5, -1, 256) == 1
    assert lib.loc_explain_splits(0, 0, 0) == 1


@pytest.mark.parametrize("case", XU.STACK_CASES, ids=str)
def test_floor_of_every_stack_case(case):
    """The float32 form's distance from the float64 form, per metric: 0 < F and MARGIN F < CAP, so that every case of
    tests/test_gpu_explain_kernels.py has a bar below what tests/test_gpu_explain.py grants."""
    _, _, F = XU.stack_refs(XU.stack_problem(*case))
    assert set(F) == ({"delta1", "acts"} if case[2] > 1 else {"delta1"})
    for name, f in F.items():
        assert XU.floor_ok(f, XU.MARGIN_STACK, XU.CAP_STACK), (case, name, f)


@pytest.mark.parametrize("case", XU.SITES_CASES, ids=str)
def test_floor_of_every_sites_case(case):
    """... for every split count the launcher takes, every split's partial sums and the reduced statistics."""
    prob = XU.sites_problem(*case)
    assert prob["X"].max() <= case[3] and (prob["X"].size < 100 or prob["X"].max() == case[3])
    assert not prob["absent"][0] and (case[1] < 3 or prob["absent"].any())
    assert not prob["U"][prob["absent"]].any() and prob["U"][~prob["absent"]].any(axis=1).all()
    for splits in XU.accepted_splits(case[0]):
        per_split, (_, F_out) = XU.sites_refs(prob, splits)
        assert len(per_split) == splits
        assert XU.floor_ok(F_out, XU.MARGIN_STATS, XU.CAP_STATS), (case, splits, F_out)
        for sp, (_, F) in enumerate(per_split):
            assert XU.floor_ok(F, XU.MARGIN_STATS, XU.CAP_STATS), (case, splits, sp, F)
