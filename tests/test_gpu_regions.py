"""The regions command on the device (locator_amd/csrc/region_kernels.hip): loc_region_assign bit for bit (region and n_inside)
against regions.assign_host, loc_region_nearest index- and bit-exact (nearest, dist2) against NumPy, at the smallest shapes
that can go wrong - point counts around the tile, rings around the LDS stage, every culling path - and the command's device
path against its --host path, byte for byte."""
import numpy as np
import pytest

from locator_amd import regions as R
from tests import regions_util as U

pytestmark = pytest.mark.gpu
TILE, STAGE = R.TILE, R.STAGE


def both(pts, rings, ring_region, n_regions=None):
    """Device and host answers for the same inputs; asserts them equal and returns (region, n_inside)."""
    verts, off, reg, box = U.ring_set(rings, ring_region)
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    want = R.assign_host(pts, verts, off, reg, box, n_regions)
    got = R.assign_device(pts, verts, off, reg, box, n_regions)
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[0].shape == (len(pts),)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    return got


def cloud(n, seed, lo=-2.5, hi=2.5):
    return np.random.default_rng(seed).uniform(lo, hi, (n, 2))


# ------------------------------------------------------------------ point counts
@pytest.mark.parametrize("n", [0, 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5])
def test_point_counts_around_the_tile_and_shuffled(n):
    rings = [U.star(9), U.star(12, cx=1.0, cy=0.5, r0=0.2, r1=0.6)]
    pts = cloud(n, 100 + n)
    reg, cnt = both(pts, rings, [0, 1])
    if n > TILE:
        assert (reg == 0).any() and (reg == 1).any() and (reg == -1).any() and (cnt == 2).any()
        perm = np.random.default_rng(5).permutation(n)
        r2, c2 = both(pts[perm], rings, [0, 1])
        assert np.array_equal(r2, reg[perm]) and np.array_equal(c2, cnt[perm])          # no dependence on the order or the tile


# ------------------------------------------------------------------ ring sizes around the LDS stage
@pytest.mark.parametrize("closed", [False, True])
@pytest.mark.parametrize("m", [3, STAGE - 1, STAGE, STAGE + 1, 2 * STAGE + 1])
def test_one_star_ring_around_the_stage(m, closed):
    ring = U.star(m, closed=closed)
    # probes level with the first vertex of every stage, with the vertex before it and with the ring's last vertex: the
    # edges that span two stages and the closing edge decide them
    ks = sorted({0, 1, m - 1, m - 2} | {k for s in range(STAGE, m, STAGE) for k in (s - 1, s)})
    xs = np.array([-2.5, -1.5, -0.5, 0.0, 0.3, 0.9, 1.4, 2.5])
    level = np.array([(x, ring[k, 1]) for k in ks for x in xs])
    at = ring[ks] + 0.0                                                                  # the vertices themselves
    pts = np.concatenate([cloud(TILE + 40, m), level, at])
    reg, cnt = both(pts, [ring], [0])
    if not (closed and m == 3):                                                          # (that one is a segment run twice)
        assert (reg == 0).any() and (reg == -1).any()


def test_closed_and_unclosed_forms_of_the_same_ring_agree():
    for m in (STAGE, STAGE + 1):                                                         # the repeat is the stage's extra vertex
        ring = U.star(m)
        pts = np.concatenate([cloud(TILE + 3, m), [(x, ring[k, 1]) for k in (0, m - 1, STAGE - 1) for x in (-2.5, 0.0, 1.0)]])
        a = both(pts, [ring], [0])
        b = both(pts, [np.concatenate([ring, ring[:1]])], [0])
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ------------------------------------------------------------------ culling
def test_a_tile_that_misses_every_ring_box():
    rings = [U.star(7, cx=10.0 * k, cy=50.0) for k in range(40)]
    reg, cnt = both(cloud(2 * TILE, 3), rings, list(range(40)))                          # far below every ring
    assert (reg == -1).all() and (cnt == 0).all()


def test_one_point_inside_one_small_ring_among_many():
    rings = [U.star(11, cx=4.0 * (k % 8), cy=4.0 * (k // 8), r0=0.2, r1=0.5) for k in range(64)]
    pts = cloud(TILE, 9, lo=100.0, hi=101.0)
    pts[77] = (4.0 * 5 + 0.05, 4.0 * 3 - 0.02)                                           # inside ring 29 only
    reg, cnt = both(pts, rings, list(range(64)))
    assert reg[77] == 29 and cnt[77] == 1 and (np.delete(reg, 77) == -1).all()
    # the same with every tile straddling many rings
    both(cloud(2 * TILE + 1, 10, lo=-1.0, hi=30.0), rings, list(range(64)))


def test_points_on_the_four_sides_of_a_ring_box():
    st = U.star(37, cx=3.0, cy=-2.0)
    box = R.ring_boxes(st, [0, len(st)])[0]
    x0, x1, y0, y1 = st[:, 0].min(), st[:, 0].max(), st[:, 1].min(), st[:, 1].max()
    xs = np.concatenate([[x0, x1, box[0], box[1], np.nextafter(x1, 9), np.nextafter(x0, -9)], np.linspace(x0 - 1, x1 + 1, 23)])
    ys = np.concatenate([[y0, y1, np.nextafter(y0, -9), np.nextafter(y1, 9)], st[:5, 1], np.linspace(y0 - 1, y1 + 1, 23)])
    pts = np.stack(np.meshgrid(xs, ys), axis=-1).reshape(-1, 2)
    low = int(np.argmin(st[:, 1]))
    pts = np.concatenate([pts, [(st[low, 0] - 10, y0), (st[low, 0], y0), (st[low, 0] - 1e-3, y0)]])   # py == ymin, rising edges
    reg, cnt = both(pts, [st], [0])
    verts, off, rr, _ = U.ring_set([st], [0])
    nocull = R.assign_host(pts, verts, off, rr, None)
    assert np.array_equal(reg, nocull[0]) and np.array_equal(cnt, nocull[1])
    # a square, whose sides ARE its box: points on each of the four sides and at the corners
    sq = U.square(0, 0, 1, 1)
    side = [(0.0, 0.5), (1.0, 0.5), (0.5, 0.0), (0.5, 1.0), (0.0, 0.0), (1.0, 1.0), (0.0, 1.0), (1.0, 0.0)]
    assert both(side, [sq], [0])[0].tolist() == [0, -1, 0, -1, 0, -1, -1, -1]


# ------------------------------------------------------------------ regions
def test_annulus_nested_regions_and_the_flush_on_a_region_change():
    outer, hole = U.square(0, 0, 10, 10), U.square(4, 4, 6, 6, closed=True)
    pts = np.concatenate([[(5, 5), (1, 1), (11, 1), (4.5, 5.5), (9, 5)], cloud(TILE + 9, 4, lo=-1.0, hi=11.0)])
    reg, cnt = both(pts, [outer, hole], [0, 0])
    assert reg[:5].tolist() == [-1, 0, -1, -1, 0] and cnt[:5].tolist() == [0, 1, 0, 0, 1]
    reg, cnt = both(pts, [outer, hole], [0, 1])
    assert reg[:5].tolist() == [0, 0, -1, 0, 0] and cnt[:5].tolist() == [2, 1, 0, 2, 1]
    nested = [U.square(0, 0, 10, 10), U.square(2, 2, 8, 8), U.square(4, 4, 6, 6)]
    reg, cnt = both(pts, nested, [0, 1, 2])
    assert reg[0] == 0 and cnt[0] == 3 and cnt[1] == 1 and cnt[4] == 1 and set(cnt.tolist()) == {0, 1, 2, 3}
    # rings of region 0 around rings of region 5: an odd parity of region 0 must not leak into region 5, and back
    rings = [U.square(0, 0, 10, 10), U.square(20, 0, 30, 10), U.square(4, 4, 6, 6), U.square(24, 4, 26, 6), U.square(0, 0, 3, 3)]
    pts2 = np.concatenate([[(5, 5), (25, 5), (1, 1), (21, 1), (15, 5)], cloud(TILE + 9, 6, lo=-1.0, hi=31.0)])
    reg, cnt = both(pts2, rings, [0, 0, 5, 5, 5], n_regions=7)                           # regions 1-4 and 6 have no rings
    assert reg[:5].tolist() == [0, 0, 0, 0, -1] and cnt[:5].tolist() == [2, 2, 2, 1, 0]
    reg, cnt = both(pts2, rings[:2] + [np.empty((0, 2)), [(0, 0), (1, 1)]] + rings[2:], [0, 0, 1, 2, 5, 5, 5], n_regions=6)
    assert reg[:5].tolist() == [0, 0, 0, 0, -1]                                          # a ring without vertices, and one of 2


def test_points_that_are_not_finite_leave_the_tile_box_alone():
    rings = [U.star(9), U.star(12, cx=1.0, cy=0.5, r0=0.2, r1=0.6)]
    pts = cloud(2 * TILE + 7, 21)
    clean = both(pts, rings, [0, 1])
    bad = pts.copy()
    where = [0, 5, 63, 64, TILE - 1, TILE, 2 * TILE + 6]
    bad[where] = [(np.nan, 0.0), (0.0, np.nan), (np.inf, 0.0), (0.0, -np.inf), (np.nan, np.nan), (-np.inf, np.inf), (np.inf, 1.0)]
    reg, cnt = both(bad, rings, [0, 1])
    assert (reg[where] == -2).all() and (cnt[where] == 0).all()
    keep = np.setdiff1d(np.arange(len(pts)), where)
    assert np.array_equal(reg[keep], clean[0][keep]) and np.array_equal(cnt[keep], clean[1][keep])
    reg, cnt = both(np.full((TILE + 1, 2), np.nan), rings, [0, 1])                       # a tile without a finite point
    assert (reg == -2).all()
    reg, cnt = both(bad, [], [])                                                         # no rings: -1 or -2
    assert (reg[where] == -2).all() and (reg[keep] == -1).all() and (cnt == 0).all()


def test_fixture_map_equals_the_host_form():
    rs, pts = U.fixture_regions(), U.fixture_points()
    want = U.fixture_answers()
    got = R.assign_device(pts, rs)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert (got[0] >= 0).sum() > 1000 and len(pts) >= 20000


# ------------------------------------------------------------------ bad arguments
def test_bad_arguments_launch_nothing():
    import torch
    from locator_amd import _lib
    lib = _lib.load()
    verts, off, reg, box = U.ring_set([U.square(0, 0, 1, 1), U.square(2, 2, 3, 3)], [0, 1])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()                     # noqa: E731
    d_pts, d_verts, d_box = dev(np.array([[0.5, 0.5], [2.5, 2.5]])), dev(verts), dev(box)
    d_reg = torch.full((2,), 77, dtype=torch.int32, device="cuda")
    d_cnt = torch.full((2,), 77, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def call(pts=d_pts, n=2, off=off, reg=reg, n_rings=2, n_regions=2):
        d_off, d_rr = dev(np.asarray(off, dtype=np.int64)), dev(np.asarray(reg, dtype=np.int32))
        rc = lib.loc_region_assign(pts.data_ptr() if pts is not None else None, n, d_verts.data_ptr(), d_off.data_ptr(),
                                   d_rr.data_ptr(), d_box.data_ptr(), n_rings, n_regions, d_reg.data_ptr(), d_cnt.data_ptr(),
                                   stream)
        torch.cuda.synchronize()
        return rc, lib.loc_last_error().decode()

    for kw, word in (({"reg": [1, 0]}, "ring_region decreases"), ({"off": [0, 8, 4]}, "ring_off decreases"),
                     ({"reg": [0, 2]}, "outside 0..1"), ({"reg": [-1, 0]}, "outside 0..1"), ({"pts": None}, "null"),
                     ({"n": -1}, "negative"), ({"n_rings": -1}, "negative")):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
        assert d_reg.tolist() == [77, 77] and d_cnt.tolist() == [77, 77]                # nothing ran
    assert call(n=0)[0] == 0 and d_reg.tolist() == [77, 77]
    assert call()[0] == 0 and d_reg.tolist() == [0, 1] and d_cnt.tolist() == [1, 1]
    d_k = torch.full((2,), 77, dtype=torch.int64, device="cuda")
    d_d = torch.zeros(2, dtype=torch.float64, device="cuda")
    p3 = dev(np.zeros((2, 3)))
    assert lib.loc_region_nearest(p3.data_ptr(), 2, p3.data_ptr(), 0, d_k.data_ptr(), d_d.data_ptr(), stream) == -1
    assert "no vertex" in lib.loc_last_error().decode()
    assert lib.loc_region_nearest(None, 2, p3.data_ptr(), 2, d_k.data_ptr(), d_d.data_ptr(), stream) == -1
    assert lib.loc_region_nearest(p3.data_ptr(), 0, p3.data_ptr(), 0, d_k.data_ptr(), d_d.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    assert d_k.tolist() == [77, 77]


# ------------------------------------------------------------------ nearest
@pytest.mark.parametrize("unit", [False, True])
@pytest.mark.parametrize("nv", [1, STAGE - 1, STAGE + 1])
@pytest.mark.parametrize("m", [1, TILE + 1])
def test_nearest_equals_numpy(m, nv, unit):
    rng = np.random.default_rng(1000 * m + nv)
    lo, hi = (-179.0, -89.0), (179.0, 89.0)
    v = rng.uniform(lo, hi, (nv, 2))
    if nv > 4:
        v[nv // 2] = v[3]                                                                # duplicated vertices: ties
        v[-1] = v[0]                                                                     # ... across the stages
    p = rng.uniform(lo, hi, (m, 2))
    if nv > 4:
        p[0] = v[3] + 1e-3                                                               # nearest to the duplicated pair
        p[-1] = v[0]                                                                     # on a duplicated vertex: d2 == 0
    p3, v3 = R.nearest_inputs(p, unit), R.nearest_inputs(v, unit)
    want_k, want_d = R.nearest_host(p3, v3)
    k, d2 = R.nearest_device(p3, v3)
    assert k.dtype == np.int64 and d2.dtype == np.float64
    assert np.array_equal(k, want_k) and np.array_equal(d2, want_d)
    for i in (0, m - 1):                                                                 # ... and a direct argmin
        d = v3 - p3[i]
        direct = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        assert k[i] == int(np.argmin(direct)) and d2[i] == direct[k[i]]
    if nv > 4:
        assert k[-1] == 0 and d2[-1] == 0.0 and (m == 1 or k[0] == 3)


# ------------------------------------------------------------------ the command
def test_device_and_host_write_the_same_bytes(tmp_path, capsys):
    d = str(tmp_path / "pred")
    sd = U.write_predlocs_fixture(d)
    outs = {}
    for mode in ("dev", "host"):
        out = str(tmp_path / mode)
        argv = ["--infile", d, "--map", U.FIXTURE_MAP, "--out", out, "--sample_data", sd, "--longlat", "--snap", "50"]
        assert R.main(argv + (["--host"] if mode == "host" else [])) == 0
        outs[mode] = (open(out + "_region_support.txt", "rb").read(), open(out + "_regions.txt", "rb").read(),
                      capsys.readouterr().out)
    assert outs["dev"] == outs["host"]
    support = [line.split("\t") for line in outs["dev"][0].decode().splitlines()[1:]]
    tops = {line.split("\t")[0]: line.split("\t") for line in outs["dev"][1].decode().splitlines()[1:]}
    assert tops["les"][3] == "Lesotho" and tops["smr"][-1] == "San Marino" and tops["fji"][3] == "Fiji"
    assert tops["sea"][3] == "NA" and tops["sea"][9] == "South Africa" and float(tops["sea"][10]) > 50
    assert {r[1] for r in support} >= {"Lesotho", "South Africa", "Italy", "Fiji", "NA"}
    # ... and the hand-made quadrant run
    d2 = str(tmp_path / "quad")
    sd2 = U.write_predlocs(d2)
    tsv = U.write_quadrants_tsv(str(tmp_path / "quad.tsv"))
    for mode in ("dev", "host"):
        out = str(tmp_path / ("q" + mode))
        assert R.main(["--infile", d2, "--regions", tsv, "--out", out, "--sample_data", sd2, "--snap", "6", "--silence"]
                      + (["--host"] if mode == "host" else [])) == 0
        outs[mode] = (open(out + "_region_support.txt", "rb").read(), open(out + "_regions.txt", "rb").read())
    assert outs["dev"] == outs["host"]
