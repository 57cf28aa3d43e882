"""No GPU: every case of normal_graph_cases.py has the property it is there for (a case without its property proves
nothing on the device), and the algorithm the kernels implement, Boruvka rounds that carry a parity bit per vertex,
gives the tree and the normals of Kruskal + walk on every case, in both types."""
import numpy as np
import pytest

import normal_graph_cases as G
from normal_graph_cases import DTYPES, ORIENT_CASES, SPLIT_CASES


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("name", list(ORIENT_CASES))
def test_orient_case_has_its_property(name, dtype):
    p, nrm, k, ref = G.orient_case(name, dtype)
    claims = ORIENT_CASES[name][1]
    n, info = len(p), ref["info"]
    a, b, w, tree = ref["a"], ref["b"], ref["w"], ref["tree"]
    assert p.dtype == dtype and nrm.dtype == dtype and w.dtype == dtype
    if "n_components" in claims:
        assert info["n_components"] == claims["n_components"]
    if "n_unreached" in claims:
        assert n - info["n_reached"] == claims["n_unreached"]
        untouched = ~ref["seen"]
        assert np.array_equal(ref["normals"][untouched].view(np.uint8), nrm[untouched].view(np.uint8))
    if claims.get("ties"):
        assert len(w) - len(np.unique(w)) >= 100, "exact weight ties are what this case is for"
    if claims.get("ties") is False:
        assert len(np.unique(w)) == len(w)
    if claims.get("zero_dots"):
        d = G.dots(nrm, a, b)
        assert (d == 0).any()
    if claims.get("wide_weights"):
        assert (w > 1).any() and (w < 0).any()
    if claims.get("tree_dependent"):
        # a non-tree edge of the start's component that joins two output normals with a negative dot: had it been
        # in the tree, one of its ends would have come out with the other sign
        rest = np.setdiff1d(np.arange(len(a)), tree)
        rest = rest[ref["seen"][a[rest]]]
        assert (G.dots(ref["normals"], a[rest], b[rest]) < 0).any()
    if "start" in claims:
        assert info["start"] == claims["start"] and (p[:, -1] == p[:, -1].max()).sum() == 2
    if "start_below" in claims:
        assert info["start"] < claims["start_below"]
    if "start_from" in claims:
        assert info["start"] >= claims["start_from"]
    if "twin_slot0" in claims:
        assert (ref["rows"][:, 0] != np.arange(n)).sum() == claims["twin_slot0"]
    if claims.get("many_components"):
        assert info["n_components"] >= 4
    if claims.get("left_edges"):
        # the weights grow strictly along the line, so every vertex's lightest edge is the one to its left: one hook
        # chain of length n in the first round
        chain = {(int(x), int(y)): float(ww) for x, y, ww in zip(a, b, w)}
        along = np.array([chain[(i, i + 1)] for i in range(n - 1)], dtype=dtype)
        assert (np.diff(along) > 0).all()
        assert all(chain[(i, i + 2)] > along[i + 1] for i in (0, n - 3))
        assert np.array_equal(ref["mst"], np.stack([np.arange(n - 1), np.arange(1, n)], axis=1))
        assert 0 < info["n_flipped"] < n


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("name", list(ORIENT_CASES))
def test_boruvka_with_parity_equals_kruskal_and_walk(name, dtype):
    p, nrm, k, ref = G.orient_case(name, dtype)
    start = ref["info"]["start"]
    tree, flip, rounds = G.boruvka_parity(len(p), nrm, ref["a"], ref["b"], ref["w"], start, nrm[start, -1] < 0)
    assert np.array_equal(tree, ref["tree"])
    out = np.where(flip[:, None], -nrm, nrm)
    assert np.array_equal(out.view(np.uint8), ref["normals"].view(np.uint8))
    assert int(flip.sum()) == ref["info"]["n_flipped"]
    assert rounds <= max(1, int(np.ceil(np.log2(len(p)))) + 1)
    if ORIENT_CASES[name][1].get("left_edges"):
        assert rounds == 1


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("name", list(SPLIT_CASES))
def test_split_case_has_its_property(name, dtype):
    p, nrm, k, angle, ref = G.split_case(name, dtype)
    claims = SPLIT_CASES[name][1]
    assert ref["info"]["n_components"] == claims["n_components"]
    assert np.abs(np.abs(ref["theta"]) - angle).min() > 1.0e-9, "an edge sits on the threshold"
    labels = ref["labels"]
    assert all(labels[i] == np.nonzero(labels == labels[i])[0][0] for i in range(len(p)))  # smallest id of the component
    if claims.get("signed"):
        assert (ref["theta"] > 1).any() and (ref["theta"] < -1).any()
    if name == "cube":
        assert all(np.array_equal(nrm[labels == c], np.tile(nrm[c], ((labels == c).sum(), 1))) for c in np.unique(labels))


def test_host_path_of_normals_py_equals_the_model_on_given_rows(monkeypatch, wtp):
    """graph="host" of normals.py, the executable description, gives the model's normals when it is handed the model's
    rows (no device): einsum's weight and the explicit one pick the same tree on these cases."""
    N = wtp.normals
    for name in ("fib_random", "two_spheres", "circle2d"):
        p, nrm, k, ref = G.orient_case(name, np.float64)
        monkeypatch.setattr(N, "_rows", lambda pts, kk, ctx, rows=ref["rows"]: rows[:, :kk])
        out = nrm.copy()
        N.orient_normals(out, p, k=k, graph="host")
        assert np.array_equal(out, ref["normals"])
    with pytest.raises(ValueError):
        N.orient_normals(nrm.copy(), p, k=k, graph="numpy")
