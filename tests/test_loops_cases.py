"""No-GPU checks of the 2-D geometry index's model (loops_cases.py): the reference's own items
(test/segment_quadtree.jl:4-179) hold on it, so the contract of include/wtp.h is consistent with them; the header
declares the entry points, the library exports them and the package exports its mirror."""
import os
import re

import numpy as np
import pytest

import loops_cases as LC

F32, F64 = LC.F32, LC.F64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["wtp_loops_set", "wtp_loops_clear", "wtp_loops_bounds", "wtp_loops_query", "wtp_loops_fill",
                "wtp_loops_fill_get", "wtp_loops_fill_get_dev", "wtp_loops_fill_darts"]


def _inside(idx, *pts):
    return list(LC.inside(idx, np.array(pts, dtype=idx["a"].dtype)))


@pytest.mark.parametrize("dtype", LC.DTYPES)
def test_unit_square_in_either_orientation(dtype):
    for loop, rev in ((LC.square(), False), (LC.square()[[0, 3, 2, 1]], True)):
        idx = LC.build([loop], dtype)
        assert len(idx["a"]) == 4 and idx["reversed"] == [rev]
        assert _inside(idx, (0.5, 0.5), (1.5, 0.5), (-0.1, -0.1), (2.0, 0.5)) == [True, False, False, False]
        q = LC.query(idx, np.array([(0.5, 1.0e-12), (0.5, 0.25)], dtype=dtype))
        assert abs(q["sd"][0]) <= 1.0e-6 and q["sd"][1] == dtype(-0.25)  # (the reference classifies the first as boundary)
        assert (idx["lo"] == 0).all() and (idx["hi"] == 1).all()


@pytest.mark.parametrize("dtype", LC.DTYPES)
def test_annulus_with_the_hole_in_either_orientation(dtype):
    outer, hole = LC.polygon(64, 2.0), LC.polygon(32, 0.5)
    a, b = LC.build([outer, hole], dtype), LC.build([outer, hole[::-1]], dtype)
    assert a["reversed"] == [False, True] and b["reversed"] == [False, False]
    # the reversed hole starts its walk at another vertex: the same segments as a set
    assert {tuple(r) for r in np.concatenate([a["a"], a["b"]], axis=1)} == {tuple(r) for r in np.concatenate([b["a"], b["b"]], axis=1)}
    for idx in (a, b):
        assert _inside(idx, (0.0, 0.0), (1.2, 0.0), (2.5, 0.0)) == [False, True, False]
        assert len(idx["a"]) == 96


def test_degenerate_input_errors():
    with pytest.raises(LC.LoopError, match="has 2 vertices"):
        LC.build([np.array([(0.0, 0.0), (1.0, 0.0)])], F64)
    collinear = np.array([(0.0, 0.0), (1.0, 0.0), (2.0, 0.0)])
    for dt in LC.DTYPES:  # Float32: the threshold must clear the shoelace sum's own round-off
        with pytest.raises(LC.LoopError, match="zero signed area"):
            LC.build([collinear], dt)
    with pytest.raises(LC.LoopError, match="2 distinct vertices"):
        LC.build([np.array([(0.0, 0.0), (1.0, 0.0), (1.0, 0.0), (0.0, 0.0)])], F64)
    with pytest.raises(LC.LoopError):
        LC.build([], F64)
    with pytest.raises(LC.LoopError, match="not finite"):
        LC.build([np.array([(0.0, 0.0), (1.0, np.inf), (1.0, 1.0)])], F64)


@pytest.mark.parametrize("off", [0.0, 1.0e3, 1.0e5])
def test_orientation_is_origin_independent_in_float32(off):
    for loop in (LC.square(off), LC.square(off)[[0, 3, 2, 1]]):
        idx = LC.build([loop.astype(F32)], F32)
        o = F32(off)
        assert _inside(idx, (o + F32(0.5), o + F32(0.5)), (o + F32(1.5), o + F32(0.5)), (o - F32(0.5), o + F32(0.5))) == \
            [True, False, False]


@pytest.mark.parametrize("dtype", LC.DTYPES)
def test_explicitly_closed_loops(dtype):
    closed = np.concatenate([LC.square(), LC.square()[:1]])
    idx = LC.build([closed], dtype)
    assert len(idx["a"]) == 4 and (np.abs(idx["nf"]).sum(axis=1) > 0).all()
    assert np.array_equal(idx["nf"], np.array([(0, -1), (1, 0), (0, 1), (-1, 0)], dtype=dtype))
    assert np.array_equal(idx["na"][0], np.array([-1, -1], dtype=dtype))          # both neighbours: a whole pseudonormal
    # the sharp corner at the seam against the independent even-odd test
    wedge = LC.build([np.concatenate([LC.WEDGE, LC.WEDGE[:1]])], dtype)
    probes = LC.wedge_probes().astype(dtype)
    assert len(wedge["a"]) == 3 and len(probes) == 216
    want = np.array([LC.point_in_loop(p, LC.WEDGE.astype(dtype)) for p in probes])
    assert np.array_equal(LC.inside(wedge, probes), want) and 3 <= want.sum() <= 12


def test_thresholds_scale_with_the_boundary():
    s = F32(1.0e-5)
    idx = LC.build([LC.square(side=1.0).astype(F32) * s], F32)
    assert np.allclose(np.hypot(idx["nf"][:, 0], idx["nf"][:, 1]), 1.0, rtol=1e-6)
    assert _inside(idx, (s / 2, s / 2), (3 * s, s / 2)) == [True, False]
    qc = LC.circle32_index()
    assert len(qc["a"]) == 20_000                                                # no segment was dropped as a duplicate
    t = np.linspace(0, 2 * np.pi, 64)
    ring = np.stack([np.cos(t), np.sin(t)], axis=1)
    assert LC.inside(qc, (0.5 * ring).astype(F32)).all() and not LC.inside(qc, (1.5 * ring).astype(F32)).any()


@pytest.mark.parametrize("r", [0.1, 0.02])
def test_tolerances_are_per_loop(r):
    outer = LC.square(side=10000.0).astype(F32)
    idx = LC.build([outer, LC.small_hole(r)], F32)
    assert len(idx["a"]) == 104 and idx["reversed"] == [False, True]
    assert _inside(idx, (5000.0, 5000.0), (5000.0 + 10 * r, 5000.0), (10001.0, 5000.0)) == [False, True, False]


def test_ties_take_the_smallest_index_and_the_boundary_is_not_inside():
    idx = LC.build([LC.square()], F64)
    q = LC.query(idx, np.array([(0.5, 0.5), (1.0, 1.0), (0.5, 0.0), (1.0, 0.5), (2.0, 2.0)]))
    assert q["seg"][0] == 0 and q["sd"][0] == -0.5                                # four segments tie at the centre
    assert list(q["sd"][1:4]) == [0, 0, 0] and not q["inside"][1:4].any()         # a vertex, a midpoint, the box's edge
    assert q["seg"][1] == 1 and np.array_equal(q["closest"][1], (1.0, 1.0))      # segments 1 and 2 share the vertex
    assert q["sd"][4] == np.sqrt(2.0) and np.array_equal(q["closest"][4], (1.0, 1.0))
    two = LC.build([LC.square(side=4.0), LC.square(off=1.0, side=2.0)], F64)      # midway between parallel edges
    m = LC.query(two, np.array([(2.0, 0.5)]))
    assert m["seg"][0] == 0 and m["sd"][0] == -0.5 and m["inside"][0]


# ---- the header, the library and the package ---------------------------------------------------------------------------
def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "wtp.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"^int %s\(wtp_ctx\* ctx" % name, text, re.M), name
    assert "no 2-D" not in text


def test_library_and_package_export_them(wtp):
    lib = wtp.load_library()
    for name in ENTRY_POINTS:
        assert getattr(lib, name).argtypes is not None
    assert wtp.SegmentQuadtree.from_boundary and callable(wtp.fill_area)
    for m in ("loops_set", "loops_clear", "loops_bounds", "loops_query", "loops_fill", "loops_fill_get",
              "loops_fill_get_dev", "loops_fill_darts"):
        assert callable(getattr(wtp.Context, m))
