"""The regions command on the host (locator_amd/regions.py): assign_host - the definition that loc_region_assign is held to in
tests/test_gpu_regions.py - on hand-written cases and against matplotlib's point-in-path, the readers, the nearest-vertex
search, the tables, the stops, and the binding of include/locator_hip_regions.h.  Nothing here needs a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from locator_amd import plot as P
from locator_amd import regions as R
from tests import regions_util as U


def assign(pts, rings, ring_region, cull=True):
    verts, off, reg, box = U.ring_set(rings, ring_region)
    return R.assign_host(np.asarray(pts, dtype=np.float64), verts, off, reg, box if cull else None)


# ------------------------------------------------------------------ the definition on hand-written cases
def test_closed_and_unclosed_squares_agree():
    pts = [(0.5, 0.5), (1.5, 0.5), (-0.5, 0.5), (0.5, 1.5), (0.5, -0.5), (0.25, 0.75)]
    a = assign(pts, [U.square(0, 0, 1, 1)], [0])
    b = assign(pts, [U.square(0, 0, 1, 1, closed=True)], [0])
    assert a[0].tolist() == b[0].tolist() == [0, -1, -1, -1, -1, 0]
    assert a[1].tolist() == b[1].tolist() == [1, 0, 0, 0, 0, 1]
    assert a[0].dtype == np.int32 and a[1].dtype == np.int32


def test_py_equal_to_a_vertex_counts_the_vertex_once():
    # a diamond: the ray from (0, 0) to the right passes exactly through the vertex (1, 0); from (-2, 0) it passes through
    # both (-1, 0) and (1, 0); y == the top vertex's touches the ring without crossing
    diamond = [(1, 0), (0, 1), (-1, 0), (0, -1)]
    reg, cnt = assign([(0, 0), (-2, 0), (2, 0), (-1, 1), (0.5, 0), (-0.5, 0)], [diamond], [0])
    assert reg.tolist() == [0, -1, -1, -1, 0, 0]
    assert cnt.tolist() == [1, 0, 0, 0, 1, 1]


def test_px_on_a_vertical_edge_and_a_horizontal_edge():
    sq = U.square(0, 0, 1, 1)
    # on the left edge px < t is 0 < 1 only for the right edge: inside; on the right edge nothing toggles: outside
    # on the bottom edge (y = 0: no vertex above... the two upper are) the vertical edges are crossed: inside; the top is not
    reg, _ = assign([(0.0, 0.5), (1.0, 0.5), (0.5, 0.0), (0.5, 1.0), (0.0, 0.0), (1.0, 1.0)], [sq], [0])
    assert reg.tolist() == [0, -1, 0, -1, 0, -1]
    # a horizontal edge never satisfies (yi > py) != (yj > py): a point level with it is decided by the other edges
    step = [(0, 0), (2, 0), (2, 1), (1, 1), (1, 2), (0, 2)]
    reg, _ = assign([(0.5, 1.0), (1.5, 1.0), (2.5, 1.0), (-0.5, 1.0)], [step], [0])
    assert reg.tolist() == [0, -1, -1, -1]


def test_a_two_vertex_ring_is_ignored_and_a_nan_point_is_minus_two():
    pts = [(0.5, 0.5), (np.nan, 0.5), (0.5, np.inf), (5, 5)]
    reg, cnt = assign(pts, [[(0, 0), (1, 1)], U.square(0, 0, 1, 1), [(0, 0), (9, 9)]], [0, 1, 1])
    assert reg.tolist() == [1, -2, -2, -1] and cnt.tolist() == [1, 0, 0, 0]
    reg, cnt = assign(pts, [], [])
    assert reg.tolist() == [-1, -2, -2, -1] and cnt.tolist() == [0, 0, 0, 0]


def test_annulus_as_one_region_and_as_two():
    outer, hole = U.square(0, 0, 10, 10), U.square(4, 4, 6, 6, closed=True)
    pts = [(5, 5), (1, 1), (11, 1), (4.5, 5.5), (9, 5)]
    reg, cnt = assign(pts, [outer, hole], [0, 0])
    assert reg.tolist() == [-1, 0, -1, -1, 0] and cnt.tolist() == [0, 1, 0, 0, 1]          # the hole is outside
    reg, cnt = assign(pts, [outer, hole], [0, 1])
    assert reg.tolist() == [0, 0, -1, 0, 0] and cnt.tolist() == [2, 1, 0, 2, 1]            # overlap: the lower index
    reg, cnt = assign(pts, [outer, hole], [2, 5])                                        # regions without rings between
    assert reg.tolist() == [2, 2, -1, 2, 2] and cnt.tolist() == [2, 1, 0, 2, 1]


def test_culling_does_not_change_an_answer_on_the_box_sides():
    st = U.star(37, cx=3.0, cy=-2.0)
    verts, off, reg, box = U.ring_set([st], [0])
    x0, x1, y0, y1 = st[:, 0].min(), st[:, 0].max(), st[:, 1].min(), st[:, 1].max()
    xs = np.concatenate([[x0, x1, box[0, 0], box[0, 1], np.nextafter(x1, 9), np.nextafter(x0, -9)], np.linspace(x0 - 1, x1 + 1, 41)])
    ys = np.concatenate([[y0, y1, np.nextafter(y0, -9), np.nextafter(y1, 9)], st[:5, 1], np.linspace(y0 - 1, y1 + 1, 41)])
    pts = np.stack(np.meshgrid(xs, ys), axis=-1).reshape(-1, 2)
    a = R.assign_host(pts, verts, off, reg, box)
    b = R.assign_host(pts, verts, off, reg, None)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and (a[0] == 0).any() and (a[0] == -1).any()
    # py == ymin below a rising edge: the lowest vertex's two edges rise from it, and a point left of it crosses both or none
    low = int(np.argmin(st[:, 1]))
    p = [(st[low, 0] - 10, y0), (st[low, 0], y0)]
    assert R.assign_host(p, verts, off, reg, box)[0].tolist() == R.assign_host(p, verts, off, reg, None)[0].tolist()


def test_assign_host_refuses_a_decreasing_ring_region():
    with pytest.raises(ValueError, match="decreases"):
        assign([(0, 0)], [U.square(0, 0, 1, 1), U.square(2, 2, 3, 3)], [1, 0])


# ------------------------------------------------------------------ against matplotlib, and the fixture's facts
def test_fixture_map_agrees_with_matplotlib_on_every_point():
    from matplotlib.path import Path
    rs, pts = U.fixture_regions(), U.fixture_points()
    assert len(rs.names) == 5 and len(rs.ring_region) == 16 and len(rs.verts) == 2335 and len(pts) == 20016 + 3200
    reg, cnt = U.fixture_answers()
    inside = np.zeros((len(rs.names), len(pts)), dtype=bool)
    for r, (a, b) in enumerate(zip(rs.ring_off[:-1], rs.ring_off[1:])):
        ring = np.concatenate([rs.verts[a:b], rs.verts[a:a + 1]])                         # closed by last -> first
        inside[rs.ring_region[r]] ^= Path(ring).contains_points(pts)                      # parity over a region's rings
    want_cnt = inside.sum(axis=0)
    want_reg = np.where(want_cnt > 0, np.argmax(inside, axis=0), -1)
    assert int((reg != want_reg).sum()) == 0 and int((cnt != want_cnt).sum()) == 0
    assert (reg >= 0).sum() > 1000 and (reg == -1).sum() > 1000
    nocull = R.assign_host(pts, rs.verts, rs.ring_off, rs.ring_region, None)
    assert np.array_equal(nocull[0], reg) and np.array_equal(nocull[1], cnt)


def test_enclaves_are_outside_the_state_around_them():
    rs = U.fixture_regions()
    assert sorted(rs.names) == ["Fiji", "Italy", "Lesotho", "San Marino", "South Africa"]
    assert [sum(1 for p in rs.parts if p[0] == n) for n in ("South Africa", "Lesotho", "Italy", "San Marino", "Fiji")] == [3, 1, 4, 1, 7]
    for inner, outer in (("Lesotho", "South Africa"), ("San Marino", "Italy")):
        k = rs.names.index(inner)
        r = int(np.nonzero(rs.ring_region == k)[0][0])
        centre = rs.verts[rs.ring_off[r]:rs.ring_off[r + 1]].mean(axis=0)
        reg, cnt = R.assign_host(centre[None, :], rs.verts, rs.ring_off, rs.ring_region, rs.ring_bbox)
        assert rs.names[reg[0]] == inner and cnt[0] == 1                                  # not in `outer` as well
        only = rs.ring_region == rs.names.index(outer)
        rings = [rs.verts[a:b] for a, b, o in zip(rs.ring_off[:-1], rs.ring_off[1:], only) if o]
        assert assign(centre[None, :], rings, [0] * len(rings))[0].tolist() == [-1]


# ------------------------------------------------------------------ readers
def test_nested_store_flat_store_and_tsv_give_the_same_structure(tmp_path):
    from locator_amd.genotypes import write_zarr_array
    flat = R.read_map(U.FLAT_MAP)
    assert flat.names == ["Afghanistan", "American_Samoa", "Armenia_0"] and flat.ring_region.tolist() == [0, 1, 2]
    assert flat.parts == [(n, n) for n in flat.names]
    nested = str(tmp_path / "nested.zarr")
    tsv = str(tmp_path / "polys.tsv")
    with open(tsv, "w") as fh:
        fh.write("part\tlat\tregion\tlon\n")                                              # columns in any order
        for (name, part), a, b in zip(flat.parts, flat.ring_off[:-1], flat.ring_off[1:]):
            xy = flat.verts[a:b]
            write_zarr_array(os.path.join(nested, name, part), np.ascontiguousarray(xy.T), (2, len(xy)))
            for x, y in xy:
                fh.write(f"{part}\t{float(y)!r}\t{name}\t{float(x)!r}\n")
    for rs in (R.read_map(nested), R.read_regions_tsv(tsv)):
        assert rs.names == flat.names and rs.parts == flat.parts
        for f in ("verts", "ring_off", "ring_region", "ring_bbox"):
            assert np.array_equal(getattr(rs, f), getattr(flat, f)), f
    assert flat.ring_off.dtype == np.int64 and flat.ring_region.dtype == np.int32 and flat.verts.flags.c_contiguous


def test_tsv_parts_are_rings_in_order_of_first_appearance(tmp_path):
    p = str(tmp_path / "r.tsv")
    rows = [("B", "b0", 0, 0), ("B", "b0", 1, 0), ("B", "b0", 1, 1), ("A", "a0", 5, 5), ("A", "a0", 6, 5), ("A", "a0", 6, 6),
            ("B", "b1", 2, 2), ("B", "b1", 3, 2), ("B", "b1", 3, 3)]
    with open(p, "w") as fh:
        fh.write("region\tpart\tlon\tlat\n" + "".join(f"{r}\t{q}\t{x}\t{y}\n" for r, q, x, y in rows))
    rs = R.read_regions_tsv(p)
    assert rs.names == ["B", "A"] and rs.parts == [("B", "b0"), ("B", "b1"), ("A", "a0")]
    assert rs.ring_region.tolist() == [0, 0, 1] and rs.ring_off.tolist() == [0, 3, 6, 9]
    assert rs.verts[3:6].tolist() == [[2, 2], [3, 2], [3, 3]]


def test_tsv_errors(tmp_path):
    p = str(tmp_path / "r.tsv")

    def write(text):
        with open(p, "w") as fh:
            fh.write(text)
    write("region\tpart\tlon\nA\ta\t1\n")
    with pytest.raises(ValueError, match="missing column lat"):
        R.read_regions_tsv(p)
    write("region\tpart\tlon\tlat\nA\ta\t0\t0\nA\ta\tnan\t0\nA\ta\t1\t1\n")
    with pytest.raises(ValueError, match="region 'A' part 'a'.*not finite"):
        R.read_regions_tsv(p)
    write("region\tpart\tlon\tlat\nA\ta\t0\t0\nA\tb\t1\t0\nA\ta\t1\t1\n")
    with pytest.raises(ValueError, match="line 4.*'a'.*reappears"):
        R.read_regions_tsv(p)
    with pytest.raises(SystemExit, match="reappears"):
        R.main(["--infile", str(tmp_path), "--out", str(tmp_path / "o"), "--regions", p, "--host"])
    with pytest.raises(ValueError, match="region 'Z' part 'z'.*not finite"):
        R.build_regions([("Z", "z", [0.0, 1.0, np.inf], [0.0, 1.0, 2.0])])


def test_read_basemap_returns_what_it_returned(tmp_path):
    """The walk restated as plot.read_basemap spelled it before it shared genotypes.walk_outlines."""
    from locator_amd.genotypes import ZarrArray, ZarrGroup

    def before(path):
        store, shapes = ZarrGroup(path), []
        for country in store:
            node = store[country]
            members = [node] if isinstance(node, ZarrArray) else [node[m] for m in node]
            for arr in members:
                if isinstance(arr, ZarrArray):
                    xy = np.asarray(arr[:], dtype=np.float64)
                    shapes.append((xy[0], xy[1]))
        return shapes
    for path, n in ((U.FLAT_MAP, 3), (U.FIXTURE_MAP, 16)):
        got, want = P.read_basemap(path), before(path)
        assert len(got) == len(want) == n and isinstance(got, list)
        for g, w in zip(got, want):
            assert isinstance(g, tuple) and len(g) == 2
            assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]) and g[0].dtype == np.float64


# ------------------------------------------------------------------ nearest
def test_nearest_takes_the_first_index_on_a_tie():
    ring = U.square(0, 0, 1, 1, closed=True)                                              # vertex 4 repeats vertex 0
    v3 = R.nearest_inputs(ring, False)
    k, d2 = R.nearest_host(R.nearest_inputs([(-1, -1), (0.5, 0.5), (2, 2), (0.5, -3)], False), v3)
    assert k.tolist() == [0, 0, 2, 0] and d2.tolist() == [2.0, 0.5, 2.0, 9.25]
    assert k.dtype == np.int64 and d2.dtype == np.float64


@pytest.mark.parametrize("longlat", [False, True])
def test_nearest_against_a_direct_argmin(longlat):
    rs = U.fixture_regions()
    pts = U.fixture_points()[:300]
    p3, v3 = R.nearest_inputs(pts, longlat), R.nearest_inputs(rs.verts, longlat)
    k, d2 = R.nearest_host(p3, v3, chunk=10000)                                           # several chunks
    for i in range(len(pts)):
        d = v3 - p3[i]
        want = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        assert k[i] == int(np.argmin(want)) and d2[i] == want[k[i]]
    reg, dist = R.nearest_regions(pts, rs, longlat, host=True)
    ring = np.searchsorted(rs.ring_off, k, side="right") - 1
    assert np.array_equal(reg, rs.ring_region[ring]) and (rs.ring_off[ring] <= k).all() and (k < rs.ring_off[ring + 1]).all()
    if longlat:
        assert np.allclose(np.linalg.norm(v3, axis=1), 1.0, atol=1e-15)
        want = P.distance_km(pts[:, 0], pts[:, 1], rs.verts[k, 0], rs.verts[k, 1])
        assert np.max(np.abs(dist - want) / want) < 1e-9
    else:
        assert np.array_equal(dist, np.sqrt(d2)) and (v3[:, 2] == 0).all()


def test_nearest_skips_empty_rings_and_wraps_longitude():
    verts, off, reg, box = U.ring_set([np.empty((0, 2)), U.square(0, 0, 1, 1), np.empty((0, 2)), U.square(5, 5, 6, 6)], [0, 1, 2, 3])
    rs = R.RegionSet(list("abcd"), None, verts, off, reg, box)
    assert R.nearest_regions(np.array([(-1.0, -1.0), (9.0, 9.0)]), rs, host=True)[0].tolist() == [1, 3]
    assert R.wrap_longitude([180.0, 181.5, -180.0, -190.0, 540.0, 0.0]).tolist() == [-180.0, -178.5, -180.0, 170.0, -180.0, 0.0]


# ------------------------------------------------------------------ tables, on a hand-made directory
def _run(tmp_path, *extra, truth=True, capsys=None):
    d = str(tmp_path / "pred")
    sd = U.write_predlocs(d)
    tsv = U.write_quadrants_tsv(str(tmp_path / "quad.tsv"))
    out = str(tmp_path / "o")
    argv = ["--infile", d, "--regions", tsv, "--out", out, "--host"] + (["--sample_data", sd] if truth else []) + list(extra)
    assert R.main(argv) == 0
    read = lambda p: [line.split("\t") for line in open(p).read().splitlines()]           # noqa: E731
    return read(out + "_region_support.txt"), read(out + "_regions.txt")


def test_host_cli_end_to_end(tmp_path, capsys):
    support, samples = _run(tmp_path)
    assert support[0] == ["sampleID", "region", "n", "support"]
    assert support[1:] == [["a", "NE", "4", "1.0"],
                           ["b", "NW", "3", "0.75"], ["b", "SW", "1", "0.25"],
                           ["c", "SE", "2", "0.5"], ["c", "NE", "1", "0.25"], ["c", "NA", "1", "0.25"],
                           ["d", "SW", "1", repr(1 / 3)], ["d", "NA", "2", repr(2 / 3)],
                           ["e_h0", "NE", "2", "0.5"], ["e_h0", "SE", "2", "0.5"]]       # n descending, then the name
    by = {}
    for sid, _, n, s in support[1:]:
        by.setdefault(sid, []).append(float(s))
    assert all(abs(sum(v) - 1.0) < 1e-15 for v in by.values())                            # the supports of a sample sum to 1
    assert samples[0] == ["sampleID", "n_reps", "n_finite", "top_region", "top_support", "second_region", "second_support",
                          "kd_region", "gc_region", "kd_nearest_region", "kd_nearest_dist", "true_region"]
    assert samples[1] == ["a", "4", "4", "NE", "1.0", "NA", "NA", "NE", "NE", "NA", "NA", "NE"]
    assert samples[2] == ["b", "4", "4", "NW", "0.75", "SW", "0.25", "NW", "NW", "NA", "NA", "SW"]
    assert samples[3] == ["c", "4", "4", "SE", "0.5", "NE", "0.25", "SE", "SE", "NA", "NA", "NA"]
    assert samples[4] == ["d", "4", "3", "SW", repr(1 / 3), "NA", "NA", "NA", "NA", "NA", "NA", "NA"]
    assert samples[5] == ["e_h0", "4", "4", "NE", "0.5", "SE", "0.5", "NE", "NE", "NA", "NA", "SE"]   # e's truth
    lines = capsys.readouterr().out.splitlines()
    assert lines[0] == "5 samples, 20 replicate predictions; 4 regions, 4 rings, 16 vertices"
    assert lines[1] == "share of replicates in no region = " + str(3 / 19)
    assert lines[2] == "points in more than one region (counted for the lowest) = 0"
    assert lines[3] == "mean top_support = " + str(float(np.mean([1.0, 0.75, 0.5, 1 / 3, 0.5])))
    assert lines[4] == "samples whose true location lies in a region = 3"
    assert lines[5:] == [f"share with {c} = true_region: {1 / 3}" for c in ("top_region", "kd_region", "gc_region")]
    assert not [f for f in os.listdir(tmp_path) if ".tmp" in f]


def test_snap_moves_only_replicates_in_no_region(tmp_path, capsys):
    base, _ = _run(tmp_path, "--silence")
    assert capsys.readouterr().out == ""
    # (10.5, -5) is 5.02 from (10, 0) - NE's vertex 1, first in upload order - and from SE's (10, -10): NE takes it
    support, samples = _run(tmp_path, "--snap", "6", "--silence")
    assert [r for r in support if r[0] == "c"] == [["c", "NE", "2", "0.5"], ["c", "SE", "2", "0.5"]]
    assert [r for r in support if r[0] != "c"] == [r for r in base if r[0] != "c"]        # d's are 40 away
    assert samples[3][3:7] == ["NE", "0.5", "SE", "0.5"]
    support, _ = _run(tmp_path, "--snap", "5", "--silence")
    assert support == base


def test_without_truth_and_kd_nearest(tmp_path):
    d = str(tmp_path / "far")
    os.makedirs(d)
    with open(os.path.join(d, "x_predlocs.txt"), "w") as fh:
        fh.write("x,y,sampleID\n13.0,14.0,s\n13.0,14.0,s\n")
    tsv = U.write_quadrants_tsv(str(tmp_path / "quad.tsv"))
    support, samples, lines = R.regions(d, R.read_regions_tsv(tsv), str(tmp_path / "o"), host=True, silence=True)
    assert support == [["s", None, 2, 1.0]]
    assert samples == [["s", 2, 2, None, None, None, None, None, None, "NE", 5.0]]       # (10, 10) is 3-4-5 away
    text = open(str(tmp_path / "o") + "_regions.txt").read().splitlines()
    assert text[0].split("\t")[-1] == "kd_nearest_dist" and text[1].split("\t")[-2:] == ["NE", "5.0"]
    assert lines[3] == "mean top_support = NA" and len(lines) == 4


# ------------------------------------------------------------------ stops and errors
def test_without_a_gpu_the_command_stops_unless_host(tmp_path, monkeypatch):
    import torch
    d = str(tmp_path / "pred")
    U.write_predlocs(d)
    tsv = U.write_quadrants_tsv(str(tmp_path / "quad.tsv"))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match="no GPU visible.*loc_region_assign.*--host"):
        R.main(["--infile", d, "--regions", tsv, "--out", str(tmp_path / "o")])
    assert not os.path.exists(str(tmp_path / "o") + "_regions.txt")


def test_exactly_one_of_map_and_regions(tmp_path, capsys):
    for extra in ([], ["--map", U.FIXTURE_MAP, "--regions", "x.tsv"]):
        with pytest.raises(SystemExit) as e:
            R.main(["--infile", str(tmp_path), "--out", str(tmp_path / "o"), "--host"] + extra)
        assert e.value.code == 2 and "exactly one of --map / --regions" in capsys.readouterr().err
    assert "VERTEX" in R.build_parser().format_help()                                     # nearest vertex, not edge


# ------------------------------------------------------------------ the binding
def test_region_header_is_bound_as_the_other_headers_are():
    from locator_amd import _abi
    from tests.abi_util import check_extension
    vp = C.c_void_p
    check_extension("region", {"loc_region_assign": (C.c_int, [vp, C.c_int64, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp]),
                               "loc_region_nearest": (C.c_int, [vp, C.c_int64, vp, C.c_int64, vp, vp, vp])},
                    {"LOC_REGION_TILE": 256, "LOC_REGION_STAGE": 2048})
    assert (_abi.LOC_REGION_TILE, _abi.LOC_REGION_STAGE) == (R.TILE, R.STAGE) == (256, 2048)
