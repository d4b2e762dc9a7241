"""The ibd command without a GPU: the worked example of the rule, segments_host against the literal per-site form on planted
fixtures that are shown not to be vacuous, pack_host against a per-bit loop, the rows argument, the binding, the folding to
samples, the --host command on a cut of the golden VCF with its refusals, the host placement against the centroid."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from locator_amd import baselines as BL
from locator_amd import ibd as IB
from tests import ibd_util as U
from tests import paint_util as PU


# ------------------------------------------------------------------ the rule
@pytest.mark.parametrize("seed_sites, extend_sites, gap_sites, first_at, want",
                         [(4, 2, 1, (), [(0, 15)]), (4, 3, 1, (), [(0, 12)]), (4, 2, 0, (), [(4, 8)]), (3, 2, 1, (6,), [(0, 5), (6, 15)])])
def test_the_worked_example(seed_sites, extend_sites, gap_sites, first_at, want):
    K = 16
    h = np.zeros((K, 2), dtype=np.int8)
    h[[3, 9, 13], 1] = 1
    first = np.zeros(K, dtype=bool)
    first[list(first_at)] = True
    x = 10 * np.arange(K, dtype=np.int64)
    P = IB.Params(seed_sites, 0, extend_sites, gap_sites, 10 ** 9, 0)
    owner = np.array([0, 1], dtype=np.int32)
    assert U.pair_literal(h[:, 0], h[:, 1], np.concatenate([[True], first[1:]]), x, P) == want
    for form in (IB.segments_host, U.segments_literal):
        count, length, longest, sa, sb = form(h, owner, first, x, P)
        assert list(zip(sa.tolist(), sb.tolist())) == want
        assert count.tolist() == [[0, len(want)], [0, 0]] and length[0, 1] == sum(10 * (b - a) for a, b in want)
        assert longest[0, 1] == max(10 * (b - a) for a, b in want) and not length[1].any() and not longest[1].any()


@pytest.mark.parametrize("K", [1, 2, 63, 64, 65, 130])
@pytest.mark.parametrize("H", [4, 6, 10])
def test_host_is_the_literal_form(H, K):
    for n, P in enumerate(U.PARAMS):
        fx = U.fixture(H, K, 1000 * H + K, P)
        got = U.host(fx, P)
        assert U.same(got, U.segments_literal(fx["h"], fx["owner"], fx["first"], fx["x"], P)), P
        assert got[0].dtype == np.int32 and got[1].dtype == got[2].dtype == np.int64 and got[3].dtype == got[4].dtype == np.int32
        assert not np.tril(got[0]).any() and not got[0][fx["owner"][:, None] == fx["owner"][None, :]].any()
        if K >= 130:
            U.assert_not_vacuous(fx, P, got)


def test_the_rows_argument_slices_the_full_answer():
    P = U.PARAMS[2]
    fx = U.fixture(10, 130, 7, P)
    count, length, longest, sa, sb = U.host(fx, P)
    ends = np.cumsum(count.reshape(-1))
    for a, b in ((0, 1), (3, 10), (9, 10), (2, 2)):
        part = U.host(fx, P, range(a, b))
        lo, hi = (ends[a * 10 - 1] if a else 0), (ends[b * 10 - 1] if b else 0)
        assert U.same(part, (count[a:b], length[a:b], longest[a:b], sa[lo:hi], sb[lo:hi]))
    assert U.host(fx, P, segments=False)[3:] == (None, None)
    with pytest.raises(ValueError, match="consecutive"):
        U.host(fx, P, [1, 3])


def test_refusals_of_the_definition():
    P = U.PARAMS[0]
    fx = U.fixture(4, 20, 1, P)
    for change, text in (({"x": fx["x"][::-1].copy()}, "ascending"), ({"h": fx["h"].astype(np.int16)}, "int8"),
                         ({"first": fx["first"][:5]}, "chromosome starts"), ({"owner": np.zeros(9, dtype=np.int32)}, "owners")):
        with pytest.raises(ValueError, match=text):
            U.host({**fx, **change}, P)
    for bad in (P._replace(seed_sites=0), P._replace(extend_sites=13), P._replace(extend_sites=0), P._replace(gap_sites=IB.MAX_GAP + 1),
                P._replace(gap_sites=-1), P._replace(seed_len=-1), P._replace(gap_len=-1), P._replace(min_len=-1), (1, 2, 3)):
        with pytest.raises(ValueError):
            U.host(fx, bad)
    # a descent across a chromosome start is no descent
    first = fx["first"].copy()
    first[10] = True
    x = np.concatenate([fx["x"][10:], fx["x"][:10]])
    U.host({**fx, "first": first, "x": x}, P)


def test_pack_host_bit_by_bit():
    rng = np.random.default_rng(2)
    for H, K, wpitch in ((1, 1, None), (5, 63, 8), (9, 64, 16), (3, 65, 24), (7, 130, None)):
        h = rng.integers(-1, 2, (K, H + 3)).astype(np.int8)
        bits = IB.pack_host(h, H, K, wpitch)
        W = (K + 63) // 64
        assert bits.dtype == np.uint64 and bits.shape == (2, W, (H + 7) // 8 * 8 if wpitch is None else wpitch)
        want = np.zeros(bits.shape, dtype=object)
        for j in range(K):
            for d in range(H):
                want[0, j // 64, d] |= int(h[j, d] > 0) << (j % 64)
                want[1, j // 64, d] |= int(h[j, d] >= 0) << (j % 64)
        assert all(int(bits[i]) == want[i] for i in np.ndindex(*bits.shape))
    assert IB.pack_host(np.zeros((0, 4), dtype=np.int8), 4, 0).shape == (2, 0, 8)
    first = np.zeros(70, dtype=bool)
    first[[0, 63, 64]] = True
    assert [int(v) for v in IB.pack_first(first, 70)] == [1 | 1 << 63, 1]
    with pytest.raises(ValueError, match="wpitch"):
        IB.pack_host(np.zeros((2, 9), dtype=np.int8), 9, 2, 12)


# ------------------------------------------------------------------ the binding
def test_ibd_header_is_bound_as_the_other_headers_are():
    from locator_amd import _abi
    from tests.abi_util import check_extension
    vp, i64, i = C.c_void_p, C.c_int64, C.c_int
    scan = [vp, i64, i, i64, vp, vp, vp, i, i, i64, i64, i64, i64, i64, i64]
    check_extension("ibd", {"loc_ibd_pack": (i, [vp, i, i64, i64, vp, i64, vp]), "loc_ibd_scan": (i, scan + [vp, vp, vp, vp]),
                            "loc_ibd_fill": (i, scan + [vp, i64, vp, vp, vp])},
                    {"LOC_IBD_MAX_HAPS", "LOC_IBD_MAX_GAP", "LOC_IBD_PACK_COLS", "LOC_IBD_BLOCK"})
    assert (_abi.LOC_IBD_MAX_HAPS, _abi.LOC_IBD_MAX_GAP) == (IB.MAX_HAPS, IB.MAX_GAP) and IB.MAX_HAPS >= 32768 and IB.MAX_GAP == 8


def test_paint_keeps_its_names_for_what_moved():
    from locator_amd import paint as PT
    assert PT.top_donors is BL.top_donors and PT.placements is BL.placements


# ------------------------------------------------------------------ the driver's pieces
def test_the_folding_to_samples():
    P = U.PARAMS[3]
    fx = U.fixture(10, 130, 11, P)
    count, length, longest, sa, sb = U.host(fx, P)
    N = 5
    want = [np.zeros((N, N), dtype=np.int64) for _ in range(3)]
    for p in range(10):
        for q in range(10):
            for s, t in ((p // 2, q // 2), (q // 2, p // 2)):
                want[0][s, t] += length[p, q]
                want[1][s, t] += count[p, q]
                want[2][s, t] = max(want[2][s, t], longest[p, q])
    batches = [(a, *U.host(fx, P, range(a, b))) for a, b in ((0, 3), (3, 4), (4, 10))]             # odd cuts: a sample over two batches
    S, Cn, L, segs = IB.sample_sharing(batches, N, keep_segments=True)
    assert all(np.array_equal(g, w) for g, w in zip((S, Cn, L), want)) and S.any()
    assert all(np.array_equal(m, m.T) and not np.diag(m).any() for m in (S, Cn, L))
    p, q, a, b = segs
    assert np.array_equal(a, sa) and np.array_equal(b, sb) and len(p) == count.sum()
    assert np.array_equal(np.bincount(p * 10 + q, minlength=100).reshape(10, 10), count)
    assert IB.sample_sharing(iter(batches), N)[3] is None


# ------------------------------------------------------------------ the command
ARGS = ("--seed_sites", "40", "--extend_sites", "8", "--gap_sites", "1", "--kmax", "8", "--keep_matrix", "--keep_segments")
FILES = ("_ibd_summary.json", "_ibd_pairs.txt", "_ibd_locs.txt", "_ibd_segments.txt", "_ibd.npz")


@pytest.fixture(scope="module")
def cut(tmp_path_factory):
    return PU.write_vcf_cut(str(tmp_path_factory.mktemp("ibd") / "cut.vcf"), 40, 60, 900)


def _inputs(cut):
    """What the command hands to segments_host for the cut: (hap, owner, first, x, chrom, pos, samples)."""
    from locator_amd import genotypes as G
    from locator_amd.paint import site_gaps
    parser = IB.build_parser()
    a = BL.parse_args(parser, ["--vcf", cut, "--out", "unused", "--host"])
    c, P, samples, locs, idx, chrom, pos, gt = BL.prelude(parser, a, IB.LAUNCH, sites=True, phase=True)
    assert (np.diff(idx) > 0).all()
    hap, _ = BL.count_matrix_sites(G.haplotypes(np.asarray(gt)), idx)
    first = site_gaps(chrom, pos, hap.shape[0])[1]
    return hap, np.repeat(np.arange(60, dtype=np.int32), 2), first, np.asarray(pos, dtype=np.int64), chrom, pos, np.asarray(samples).astype(str)


def test_the_host_command_on_a_cut_of_the_golden_vcf(cut, tmp_path):
    outs = []
    for name in ("a", "b"):
        outs.append(str(tmp_path / name))
        assert IB.main(["--vcf", cut, "--sample_data", U.SAMPLE_DATA, "--out", outs[-1], "--host", "--silence", *ARGS]) == 0
    assert sorted(os.listdir(tmp_path)) == sorted(o + n for o in ("a", "b") for n in FILES)
    for n in FILES:
        assert open(outs[0] + n, "rb").read() == open(outs[1] + n, "rb").read(), n
    s = json.load(open(outs[0] + "_ibd_summary.json"))
    assert tuple(s) == IB.HEAD + IB.OWN + IB.PLACED + ("path",)
    assert (s["N"], s["n_located"], s["H"], s["seed_sites"], s["extend_sites"], s["gap_sites"], s["gap_length"], s["path"]) == (
        60, 50, 120, 40, 8, 1, None, "host")
    z = np.load(outs[0] + "_ibd.npz")
    assert sorted(z.files) == ["C", "L", "S", "samples"] and z["S"].shape == z["C"].shape == z["L"].shape == (60, 60)
    S, Cn, L = z["S"], z["C"], z["L"]
    assert all(np.array_equal(m, m.T) and not np.diag(m).any() for m in (S, Cn, L)) and S.any()
    # the segments file against segments_host called directly
    hap, owner, first, x, chrom, pos, samples = _inputs(cut)
    assert s["K"] == hap.shape[0] and np.array_equal(samples, z["samples"])
    P = IB.Params(40, 0, 8, 1, IB.NO_LIMIT, 0)
    count, length, longest, sa, sb = IB.segments_host(hap, owner, first, x, P)
    assert s["segments"] == count.sum() == Cn.sum() // 2 > 0 and s["pairs_sharing"] == (np.triu(Cn, 1) > 0).sum()
    head, *rows = [line.split("\t") for line in open(outs[0] + "_ibd_segments.txt").read().splitlines()]
    assert head == ["sampleID1", "hap1", "sampleID2", "hap2", "chrom", "start", "end", "sites", "length"]
    pair = np.repeat(np.arange(count.size), count.reshape(-1))
    want = [[samples[at // 120 // 2], str(at // 120 % 2), samples[at % 120 // 2], str(at % 120 % 2), str(chrom[a]), str(pos[a]), str(pos[b]),
             str(b - a + 1), str(x[b] - x[a])] for at, a, b in zip(pair, sa, sb)]
    assert rows == want
    head, *rows = [line.split("\t") for line in open(outs[0] + "_ibd_pairs.txt").read().splitlines()]
    assert head == ["sampleID1", "sampleID2", "segments", "length", "longest"] and len(rows) == s["pairs_sharing"]
    at = {n: i for i, n in enumerate(samples)}
    assert all((Cn[at[r[0]], at[r[1]]], S[at[r[0]], at[r[1]]], L[at[r[0]], at[r[1]]]) == tuple(int(v) for v in r[2:]) and at[r[0]] < at[r[1]]
               for r in rows)
    head, *rows = [line.split(",") for line in open(outs[0] + "_ibd_locs.txt").read().splitlines()]
    assert head == ["x", "y", "sampleID"] and len(rows) == 60
    # the placement against the centroid of the others
    locs = BL.read_locations(U.SAMPLE_DATA, samples, IB.PROG)
    located = ~np.isnan(locs).any(axis=1)
    n = int(located.sum())
    others = (locs[located].sum(axis=0)[None, :] - locs[located]) / (n - 1)
    centroid = float(np.median(BL.errors(others, locs[located])))
    print(f"golden VCF cut 60 x {s['K']}: leave-one-out median error {s['median_error']:.3f} at k = {s['k']}, centroid of the others {centroid:.3f}")
    assert s["median_error"] < centroid


def test_without_locations_and_in_sites(cut, tmp_path):
    out = str(tmp_path / "n")
    assert IB.main(["--vcf", cut, "--out", out, "--host", "--silence", "--uniform", "--max_SNPs", "200", "--seed", "1", "--seed_sites", "30",
                    "--extend_sites", "30", "--gap_sites", "0", "--min_length", "35"]) == 0
    assert sorted(os.listdir(tmp_path)) == ["n_ibd_pairs.txt", "n_ibd_summary.json"]
    s = json.load(open(out + "_ibd_summary.json"))
    assert tuple(s) == ("N", "K", "P") + IB.OWN + ("path",) and (s["K"], s["uniform"], s["min_length"]) == (200, True, 35)
    rows = [line.split("\t") for line in open(out + "_ibd_pairs.txt").read().splitlines()][1:]
    assert rows and all(int(r[4]) >= 35 and int(r[3]) >= int(r[4]) for r in rows)                 # exact runs of 36 sites at least


def test_refusals(cut, tmp_path, capsys, monkeypatch):
    out = str(tmp_path / "o")
    matrix = str(tmp_path / "m.txt")
    with open(matrix, "w") as fh:
        fh.write("sampleID\ts0\ts1\nzz_1\t0\t1\nzz_2\t2\t1\n")
    with pytest.raises(SystemExit, match="--matrix carries no phase"):
        IB.main(["--matrix", matrix, "--out", out, "--host"])
    slashed = PU.write_vcf_cut(str(tmp_path / "slashed.vcf"), 40, 60, 50, unphase=((3, 7), (20, 0)))
    with pytest.raises(SystemExit, match=r"slashed.vcf has 2 heterozygous call\(s\) without phase"):
        IB.main(["--vcf", slashed, "--out", out, "--host"])
    with pytest.raises(SystemExit, match="no site is left after the filters"):
        IB.main(["--vcf", cut, "--out", out, "--host", "--min_mac", "1000"])
    one = PU.write_vcf_cut(str(tmp_path / "one.vcf"), 40, 1, 200)
    with pytest.raises(SystemExit, match="two samples at least"):
        IB.main(["--vcf", one, "--out", out, "--host", "--min_mac", "1"])
    for extra, text in ((["--k", "9", "--kmax", "8"], "--k must be"), (["--kmax", "0"], "--kmax must be"), (["--budget_gb", "0"], "--budget_gb"),
                        (["--zarr", "x"], "exactly one of")):
        with pytest.raises(SystemExit) as e:
            IB.main(["--vcf", cut, "--out", out, "--host"] + extra)
        assert e.value.code == 2 and text in capsys.readouterr().err, extra
    for extra, text in ((["--seed_sites", "0"], "seed_sites must be >= 1"), (["--extend_sites", "65"], "extend_sites 1 .. seed_sites"),
                        (["--gap_sites", "9"], "gap_sites = 9: must be 0 .. 8"), (["--min_length=-1"], "no length may be negative"),
                        (["--gap_length=-5"], "no length may be negative"), (["--seed_length=-1"], "no length may be negative")):
        with pytest.raises(SystemExit, match=text):
            IB.main(["--vcf", cut, "--out", out, "--host", "--max_SNPs", "50"] + extra)
    with pytest.raises(SystemExit, match="nothing to choose k by"):
        IB.main(["--vcf", cut, "--sample_data", U.SAMPLE_DATA, "--out", out, "--host", "--max_SNPs", "50", "--seed_sites", "50", "--gap_sites", "0",
                 "--min_length", "1000000000"])
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match="no GPU visible.*loc_ibd_scan.*--host"):
        IB.main(["--vcf", cut, "--out", out])
    assert sorted(os.listdir(tmp_path)) == ["m.txt", "one.vcf", "slashed.vcf"]


def test_the_ploidy_refusal(cut, tmp_path, monkeypatch):
    """Haploid calls reach the command only through a zarr store or a VCF of haploid calls; the refusal is the prelude's answer."""
    real = BL.prelude
    monkeypatch.setattr(BL, "prelude", lambda *a, **k: (lambda r: (r[0], 1) + r[2:])(real(*a, **k)))
    with pytest.raises(SystemExit, match="calls of ploidy 1"):
        IB.main(["--vcf", cut, "--out", str(tmp_path / "p"), "--host", "--max_SNPs", "50"])
    assert os.listdir(tmp_path) == []
