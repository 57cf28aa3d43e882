"""The 2-D geometry index on the device (include/wtp.h: wtp_loops_set, wtp_loops_clear, wtp_loops_bounds,
wtp_loops_query; host mirror SegmentQuadtree) against the numpy model of loops_cases.py: segment, closest point, signed
distance and inside flag bit for bit in both types, at the tree's and the wave's edges; every error row; the reference's
own items (test/segment_quadtree.jl:4-179) through SegmentQuadtree."""
import numpy as np
import pytest

import loops_cases as LC

pytestmark = pytest.mark.gpu

F32, F64 = LC.F32, LC.F64


def _check(ctx, loops, dtype, pts, idx=None):
    """The library's answers for pts against the loops equal the model's, bit for bit; returns the model's."""
    loops = [np.ascontiguousarray(l, dtype=dtype) for l in loops]
    ctx.loops_set(loops)
    idx = idx or LC.build(loops, dtype)
    lo, hi, ns = ctx.loops_bounds()
    assert ns == len(idx["a"]) and np.array_equal(lo, idx["lo"].astype(F64)) and np.array_equal(hi, idx["hi"].astype(F64))
    pts = np.ascontiguousarray(pts)
    got, want = ctx.loops_query(pts), LC.query(idx, pts)
    assert got["sd"].dtype == pts.dtype and got["closest"].shape == (len(pts), 2)
    for k in ("seg", "closest", "sd", "inside"):
        assert np.array_equal(got[k], want[k]), k
    return want


def _probes(idx, n, rng):
    """n points about the index's box: uniform over the box widened by a quarter, and some exactly on features."""
    lo, hi = idx["lo"].astype(F64), idx["hi"].astype(F64)
    ext = hi - lo
    p = lo - ext / 4 + rng.random((n, 2)) * ext * 1.5
    k = min(n, len(idx["a"]))
    p[:k:3] = idx["a"][:k:3]                                              # on a vertex
    p[1:k:3] = (idx["a"][1:k:3].astype(F64) + idx["b"][1:k:3].astype(F64)) / 2   # on (or within rounding of) a segment
    return p


@pytest.mark.parametrize("dtype", LC.DTYPES)
@pytest.mark.parametrize("ns", [3, 4, 63, 64, 65])
def test_regular_polygons_at_tree_and_wave_edges(ctx, ns, dtype):
    loop = LC.polygon(ns, 1.0, (0.25, -0.5), 0.1)
    idx = LC.build([loop.astype(dtype)], dtype)
    rng = np.random.default_rng(ns)
    for n in (1, 63, 64, 65, 257, 1000):
        _check(ctx, [loop], dtype, _probes(idx, n, rng).astype(dtype), idx)


def test_circle_of_20000_segments_in_float32(ctx):
    idx = LC.circle32_index()
    rng = np.random.default_rng(7)
    pts = _probes(idx, 257, rng).astype(F32)
    t = np.linspace(0, 2 * np.pi, 64)
    ring = np.stack([np.cos(t), np.sin(t)], axis=1)
    pts = np.concatenate([pts, (0.5 * ring).astype(F32), (1.5 * ring).astype(F32), (0.99999 * ring).astype(F32)])
    want = _check(ctx, [LC.circle32()], F32, pts, idx)
    assert want["inside"][257:321].all() and not want["inside"][321:385].any()


@pytest.mark.parametrize("dtype", LC.DTYPES)
def test_points_on_features_ties_and_the_box(ctx, dtype):
    sq = LC.square()
    pts = np.array([(0.5, 0.5), (1.0, 1.0), (0.0, 0.0), (0.5, 0.0), (1.0, 0.5), (0.0, 0.25), (2.0, 2.0), (-1.0, 0.5),
                    (0.5, 1.0 + 1e-6), (1.0, 0.0)], dtype=dtype)
    want = _check(ctx, [sq], dtype, pts)
    assert want["seg"][0] == 0 and want["sd"][0] == dtype(-0.5) and want["inside"][0]   # four segments tie: index 0 wins
    assert (want["sd"][1:6] == 0).all() and not want["inside"][1:].any()                # on a vertex, a segment, the box's edge
    two = _check(ctx, [LC.square(side=4.0), LC.square(off=1.0, side=2.0)], dtype, np.array([(2.0, 0.5), (2.0, 2.0)], dtype=dtype))
    assert two["seg"][0] == 0 and two["inside"][0] and not two["inside"][1]             # two loops tie; the hole's centre
    # a query of the other type is converted once and the results converted back
    other = F64 if dtype == F32 else F32
    _check(ctx, [sq], dtype, np.array([(0.3, 0.7), (1.5, 0.1), (0.1, 0.1)], dtype=other))


@pytest.mark.parametrize("dtype", LC.DTYPES)
def test_wedge_probes_equal_the_crossing_rule(ctx, dtype):
    probes = LC.wedge_probes().astype(dtype)
    want = _check(ctx, [np.concatenate([LC.WEDGE, LC.WEDGE[:1]])], dtype, probes)
    assert np.array_equal(want["inside"], [LC.point_in_loop(p, LC.WEDGE.astype(dtype)) for p in probes])


@pytest.mark.parametrize("dtype", LC.DTYPES)
def test_a_wave_of_mixed_queries(ctx, dtype):
    """Lanes of one wave alternate between deep inside, far outside and within 1e-6 of the boundary: every lane's walk
    prunes differently."""
    star = LC.star()
    mid = (star + np.roll(star, -1, axis=0)) / 2
    k = np.arange(64)
    pts = np.where((k % 3 == 0)[:, None], 0.05 * star[k], np.where((k % 3 == 1)[:, None], 40.0 * star[k], mid[k] * (1 - 1e-6)))
    want = _check(ctx, [star], dtype, pts.astype(dtype))
    assert want["inside"][0::3].all() and not want["inside"][1::3].any()


def test_float32_offsets_and_the_small_square(ctx):
    for off in (0.0, 1.0e3, 1.0e5):
        o = F32(off)
        pts = np.array([(o + F32(0.5), o + F32(0.5)), (o + F32(1.5), o + F32(0.5)), (o - F32(0.5), o + F32(0.5)),
                        (o + F32(0.25), o + F32(1.0))], dtype=F32)
        want = _check(ctx, [LC.square(off)], F32, pts)
        assert list(want["inside"]) == [True, False, False, False]
    s = F32(1.0e-5)
    small = LC.square().astype(F32) * s
    want = _check(ctx, [small], F32, np.array([(s / 2, s / 2), (3 * s, s / 2), (s / 4, s / 8)], dtype=F32))
    assert list(want["inside"]) == [True, False, True]


def test_error_rows_replace_and_clear(wtp, ctx):
    from whatsthepoint_jl_amd import _lib as L
    import ctypes as C

    ctx.loops_clear()
    for call in (ctx.loops_bounds, lambda: ctx.loops_query(np.zeros((1, 2)))):
        with pytest.raises(wtp.WtpError) as e:
            call()
        assert e.value.code == L.WTP_ERR_STATE
    with pytest.raises(wtp.WtpArgumentError, match="loop 0 has 2 vertices"):
        ctx.loops_set([np.array([(0.0, 0.0), (1.0, 0.0)])])
    collinear = np.array([(0.0, 0.0), (1.0, 0.0), (2.0, 0.0)])
    for dt in LC.DTYPES:
        with pytest.raises(wtp.WtpArgumentError, match="loop 0 has .*zero signed area"):
            ctx.loops_set([collinear.astype(dt)])
    with pytest.raises(wtp.WtpArgumentError, match="loop 1 has 2 distinct vertices"):
        ctx.loops_set([LC.square(), np.array([(0.2, 0.2), (0.4, 0.2), (0.4, 0.2), (0.2, 0.2)])])
    with pytest.raises(wtp.WtpArgumentError, match="not finite"):
        ctx.loops_set([np.array([(0.0, 0.0), (1.0, np.nan), (1.0, 1.0)])])
    with pytest.raises(wtp.WtpArgumentError):
        ctx.loops_set([])
    # the rows of the raw entry that the mirror cannot reach: n_loops < 1, offsets that do not increase, a bad dtype
    xy = np.ascontiguousarray(np.concatenate([LC.square(), LC.square(off=0.25, side=0.5)]))
    for start, nl, dt in (([0, 8], 0, L.WTP_F64), ([0, 5, 3, 8], 3, L.WTP_F64), ([0, 4, 7], 2, L.WTP_F64), ([0, 4, 8], 2, 7)):
        st = np.array(start, dtype=np.int64)
        rc = ctx._lib.wtp_loops_set(ctx._h, xy.ctypes.data_as(C.c_void_p), len(xy), st.ctypes.data_as(C.c_void_p), nl, dt)
        assert rc == L.WTP_ERR_ARG
    with pytest.raises(wtp.WtpError) as e:
        ctx.loops_bounds()                                                 # a failed set leaves no index
    assert e.value.code == L.WTP_ERR_STATE
    ctx.loops_set([LC.square()])
    for v in (np.nan, np.inf):
        with pytest.raises(wtp.WtpArgumentError, match="query point 1 "):
            ctx.loops_query(np.array([(0.5, 0.5), (v, 0.5)]))
    assert ctx.loops_query(np.zeros((0, 2)))["sd"].shape == (0,)
    assert ctx.loops_query(np.array([(0.5, 0.5)]), want=("inside",))["inside"][0]      # every output may be absent
    # replace: the next call's loops answer; clear: none do
    assert ctx.loops_bounds()[2] == 4
    ctx.loops_set([LC.square(off=10.0), LC.polygon(5, 0.2, (10.5, 10.5))])
    assert ctx.loops_bounds()[2] == 9 and not ctx.loops_query(np.array([(0.5, 0.5)]))["inside"][0]
    assert list(ctx.loops_query(np.array([(10.1, 10.1), (10.5, 10.5)]))["inside"]) == [True, False]
    ctx.loops_clear()
    with pytest.raises(wtp.WtpError) as e:
        ctx.loops_query(np.array([(0.5, 0.5)]))
    assert e.value.code == L.WTP_ERR_STATE


# ---- the reference's own items (test/segment_quadtree.jl:4-179), through SegmentQuadtree -------------------------------------
def test_reference_square_annulus_and_boundary(wtp, ctx):
    for loop in (LC.square(), LC.square()[[0, 3, 2, 1]]):
        sq = wtp.SegmentQuadtree(loop, ctx=ctx)
        assert len(sq) == sq.num_segments == 4 and sq.dtype == F64
        assert sq.isinside(np.array([0.5, 0.5])) and not sq.isinside(np.array([1.5, 0.5]))
        assert list(sq.isinside(np.array([(-0.1, -0.1), (2.0, 0.5)]))) == [False, False]
        assert abs(sq.signed_distance(np.array([0.5, 1.0e-12]))) <= 1.0e-6
        lo, hi = sq.bounds()
        assert (lo == 0).all() and (hi == 1).all()
        seg, cp = sq.nearest_segment(np.array([(0.5, -1.0)]))
        assert np.array_equal(cp, [(0.5, 0.0)]) and np.array_equal(sq.query(np.array([0.5, -1.0]))["closest"], (0.5, 0.0))
    outer, hole = LC.polygon(64, 2.0), LC.polygon(32, 0.5)
    for h in (hole, hole[::-1]):
        sq = wtp.SegmentQuadtree([outer, h], ctx=ctx)
        assert list(sq.isinside(np.array([(0.0, 0.0), (1.2, 0.0), (2.5, 0.0)]))) == [False, True, False]
        assert list(wtp.isinside(np.array([(0.0, 0.0), (1.2, 0.0)]), sq)) == [False, True]   # inside.py dispatches to it
    bnd = wtp.PointBoundary(LC.square())
    sq = wtp.SegmentQuadtree.from_boundary(bnd, ctx=ctx)
    assert len(sq) == 4 and sq.isinside(np.array([0.5, 0.5])) and not sq.isinside(np.array([1.5, 0.5]))
    two = wtp.PointBoundary(surfaces=dict(outer=outer, hole=hole))
    assert len(wtp.SegmentQuadtree.from_boundary(two, ctx=ctx)) == 96


def test_reference_errors_closed_loops_and_scales(wtp, ctx):
    for bad in ([(0.0, 0.0), (1.0, 0.0)], [(0.0, 0.0), (1.0, 0.0), (2.0, 0.0)],
                [(0.0, 0.0), (1.0, 0.0), (1.0, 0.0), (0.0, 0.0)]):
        with pytest.raises(wtp.WtpArgumentError):
            wtp.SegmentQuadtree(np.array(bad), ctx=ctx)
    with pytest.raises(wtp.WtpArgumentError):
        wtp.SegmentQuadtree(np.array([(0.0, 0.0), (1.0, 0.0), (2.0, 0.0)], dtype=F32), ctx=ctx)
    closed = np.concatenate([LC.square(), LC.square()[:1]])
    assert len(wtp.SegmentQuadtree(closed, ctx=ctx)) == 4
    for r in (0.1, 0.02):
        sq = wtp.SegmentQuadtree([LC.square(side=10000.0).astype(F32), LC.small_hole(r)], ctx=ctx)
        q = np.array([(5000.0, 5000.0), (5000.0 + 10 * r, 5000.0), (10001.0, 5000.0)], dtype=F32)
        assert len(sq) == 104 and list(sq.isinside(q)) == [False, True, False]
    # two quadtrees in one context: each re-uploads when the other was resident
    a, b = wtp.SegmentQuadtree(LC.square(), ctx=ctx), wtp.SegmentQuadtree(LC.square(off=5.0), ctx=ctx)
    assert a.isinside(np.array([0.5, 0.5])) and b.isinside(np.array([5.5, 5.5])) and not a.isinside(np.array([5.5, 5.5]))


def test_inside_agrees_with_the_winding_number_on_the_star(wtp, ctx):
    star = LC.star()
    sq = wtp.SegmentQuadtree(star, ctx=ctx)
    rng = np.random.default_rng(3)
    p = (rng.random((4000, 2)) - 0.5) * 2.8
    q = sq.query(p, want=("sd", "inside"))
    far = np.abs(q["sd"]) > 1e-6
    assert far.sum() > 3900 and 0.3 < q["inside"].mean() < 0.6
    assert np.array_equal(q["inside"][far], wtp.isinside(p, star, ctx=ctx)[far])
