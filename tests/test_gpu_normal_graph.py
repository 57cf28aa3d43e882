"""wtp_orient_normals / wtp_normal_components against the numpy model of normal_graph_cases.py, bit for bit, in fp32
and fp64: the oriented normals, the sorted minimum spanning forest, the labels and the counts of the info struct.
test_normal_graph_cases.py shows (without a GPU) that every case has the property it is there for.

The forest is compared first: a wrong tree and a wrong parity are told apart by which assertion fails."""
import ctypes as C
import math

import numpy as np
import pytest

import normal_graph_cases as G
from normal_graph_cases import DTYPES, ORIENT_CASES, SPLIT_CASES

pytestmark = pytest.mark.gpu

IDS = ["f32", "f64"]


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _check_orient(got, ref, n):
    out, info, mst = got
    assert mst.dtype == np.int32 and np.array_equal(mst, ref["mst"]), "the forest differs"
    assert _same_bits(out, ref["normals"]), "the tree is right, the signs differ"
    for name, want in ref["info"].items():
        assert info[name] == want, name
    assert 0 <= info["rounds"] <= max(1, math.ceil(math.log2(n)) + 1)
    # one read-back per batch of 4 rounds (the last round only finds nothing left to merge), one for the result
    assert info["host_syncs"] == ((info["rounds"] + 1 + 3) // 4 + 1 if ref["rows"].shape[1] > 1 else 2)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", list(ORIENT_CASES))
def test_orient_equals_the_model(ctx, name, dtype):
    p, nrm, k, ref = G.orient_case(name, dtype)
    _check_orient(ctx.orient_normals(p, nrm, k, return_tree=True), ref, len(p))
    if ORIENT_CASES[name][1].get("left_edges"):
        assert ctx.orient_normals(p, nrm, k)[1]["rounds"] == 1  # one hook chain of length n, flattened in one round


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", list(SPLIT_CASES))
def test_components_equal_the_model(ctx, wtp, name, dtype):
    p, nrm, k, angle, ref = G.split_case(name, dtype)
    labels, info = ctx.normal_components(p, nrm, k, angle)
    assert labels.dtype == np.int32 and np.array_equal(labels, ref["labels"])
    assert info["n_components"] == ref["info"]["n_components"] and info["n_edges"] == ref["info"]["n_edges"]
    assert info["start"] == -1 and info["n_reached"] == 0 and info["n_flipped"] == 0
    # split_surface through both graph parts: the same surfaces under the same names
    made = {}
    for graph in ("device", "host"):
        bnd = wtp.PointBoundary(p.copy(), nrm.copy(), np.arange(len(p), dtype=np.float64))
        wtp.split_surface(bnd, angle, k=k, ctx=ctx, graph=graph)
        made[graph] = {name_: (s.points(), s.normals, s.areas) for name_, s in bnd.surfaces.items()}
    assert list(made["device"]) == list(made["host"]) == [f"surface{i + 1}" for i in range(ref["info"]["n_components"])]
    for key, parts in made["device"].items():
        assert all(_same_bits(x, y) for x, y in zip(parts, made["host"][key]))
    # numbered by first vertex: the areas carry the original indices
    firsts = [int(parts[2][0]) for parts in made["device"].values()]
    assert firsts == sorted(np.unique(ref["labels"]).tolist())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_python_orient_normals_through_both_graph_parts(ctx, wtp, dtype):
    p, nrm, k, ref = G.orient_case("fib_random", dtype)
    for graph in ("device", "host"):
        out = nrm.copy()
        assert wtp.orient_normals(out, p, k=k, ctx=ctx, graph=graph) is None
        assert _same_bits(out, ref["normals"]), graph


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_two_calls_return_the_same_bytes(ctx, dtype):
    p, nrm, k, _ = G.orient_case("quantised", dtype)
    first = ctx.orient_normals(p, nrm, k, return_tree=True)
    again = ctx.orient_normals(p, nrm, k, return_tree=True)
    assert _same_bits(first[0], again[0]) and _same_bits(first[2], again[2])
    assert {k_: v for k_, v in first[1].items()} == {k_: v for k_, v in again[1].items()}
    p, nrm, k, angle, _ = G.split_case("cube", dtype)
    assert _same_bits(ctx.normal_components(p, nrm, k, angle)[0], ctx.normal_components(p, nrm, k, angle)[0])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_device_entry_point_equals_the_host_call(ctx, dtype):
    import torch

    p, nrm, k, ref = G.orient_case("n257", dtype)
    n = len(p)
    dev = torch.device("cuda", 0)
    pd, nd = torch.from_numpy(p.copy()).to(dev), torch.from_numpy(nrm.copy()).to(dev)
    md = torch.full((n - 1, 2), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    info = ctx.orient_normals_dev(pd.data_ptr(), n, 3, dtype, k, nd.data_ptr(), md.data_ptr())
    mst = md.cpu().numpy()[: n - info["n_components"]]
    mst = mst[np.lexsort((mst[:, 1], mst[:, 0]))]
    _check_orient((nd.cpu().numpy(), info, mst), ref, n)
    # without the read-out
    nd2 = torch.from_numpy(nrm.copy()).to(dev)
    torch.cuda.synchronize(dev)
    info2 = ctx.orient_normals_dev(pd.data_ptr(), n, 3, dtype, k, nd2.data_ptr())
    assert _same_bits(nd2.cpu().numpy(), ref["normals"]) and info2["n_flipped"] == info["n_flipped"]


def test_argument_errors(ctx, wtp):
    from whatsthepoint_jl_amd import _lib as L

    p, nrm, k, ref = G.orient_case("n65", np.float32)
    for bad_k in (0, -1, 66):
        with pytest.raises(wtp.WtpArgumentError):
            ctx.orient_normals(p, nrm, bad_k)
        with pytest.raises(wtp.WtpArgumentError):
            ctx.normal_components(p, nrm, bad_k, 1.0)
    # a NaN or an infinite component: the first offending index is named, nothing is written
    for entries, first in (({17: math.nan}, 17), ({40: math.inf, 3: math.nan}, 3), ({64: -math.inf}, 64)):
        bad = nrm.copy()
        for at, value in entries.items():
            bad[at, at % 3] = value
        with pytest.raises(wtp.WtpArgumentError, match=rf"normals\[{first}\]"):
            ctx.orient_normals(p, bad, k)
        with pytest.raises(wtp.WtpArgumentError, match=rf"normals\[{first}\]"):
            ctx.normal_components(p, bad, k, 1.0)
        keep = bad.copy()
        info = L.NormalGraphInfo()
        vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        assert ctx._lib.wtp_orient_normals(ctx._h, vp(p), 65, 3, L.WTP_F32, k, vp(bad), None, C.byref(info)) == L.WTP_ERR_ARG
        assert bad.tobytes() == keep.tobytes()
    with pytest.raises(wtp.WtpArgumentError):
        ctx.normal_components(p, nrm, k, math.nan)
    with pytest.raises(wtp.WtpArgumentError):
        ctx.orient_normals(p, nrm[:10], k)
    # the context still works
    _check_orient(ctx.orient_normals(p, nrm, k, return_tree=True), ref, 65)


def test_refused_during_a_relax_session(wtp):
    p, nrm, k, ref = G.orient_case("n257", np.float32)
    x = np.ascontiguousarray(np.random.default_rng(3).random((2000, 3)).astype(np.float32))
    s = 2000.0 ** (-1.0 / 3.0)
    with wtp.Context(0) as c:
        with c.relax(x, 0, s, dict(kind=2, beta=0.2, u0=1.0, gamma=3.0), 21, s / 2000, s / 20):
            for call in (lambda: c.orient_normals(p, nrm, k), lambda: c.normal_components(p, nrm, k, 1.0)):
                with pytest.raises(wtp.WtpError) as ei:
                    call()
                assert ei.value.code == 4  # WTP_ERR_STATE
        assert _same_bits(c.orient_normals(p, nrm, k)[0], ref["normals"])


def test_ends_a_pending_radius_pair(ctx):
    p, nrm, k, _ = G.orient_case("n257", np.float32)
    counts = np.empty(len(p), dtype=np.int32)
    for call in (lambda: ctx.orient_normals(p, nrm, k), lambda: ctx.normal_components(p, nrm, k, 1.0)):
        assert ctx._lib.wtp_radius_count(ctx._h, p.ctypes.data_as(C.c_void_p), len(p), 3, 0, 0.1,
                                         counts.ctypes.data_as(C.c_void_p)) == 0
        call()
        assert ctx._lib.wtp_radius_fill(ctx._h, None, None) == 4  # WTP_ERR_STATE: the pair is over
