"""Case table and numpy model of the graph part of orient_normals! / split_surface! (include/wtp.h:
wtp_orient_normals, wtp_normal_components).  Shared by test_normal_graph_cases.py (no GPU: every case has the
property it is there for; Boruvka with parities equals Kruskal + walk) and test_gpu_normal_graph.py (the device
equals the model bit for bit).

The model, all in the cloud's type T:
  rows     brute force, ((dx dx + dy dy) + dz dz), canonical (d2, index) order, self slot included
  edges    src = slot 0, dst = slots 1..k-1 of every row; undirected, simple
  weight   (1 - |((nx nx' + ny ny') + nz nz')|) + 100 eps(T), written with explicit products and sums
  forest   Kruskal under the total order (w, a, b)
  walk     from the first index with the largest last coordinate, flipped if its last component is < 0; a vertex
           is flipped if its normal has a negative dot with its parent's current one
  split    union-find over the edges with |_angle| < angle; label = smallest id of the component"""
from __future__ import annotations

import functools

import numpy as np

F32, F64 = np.float32, np.float64
DTYPES = [F32, F64]


# ---- the model ------------------------------------------------------------------------------------------------------
def rows_of(p, k):
    p = np.ascontiguousarray(p)
    n, dim = p.shape
    d2 = np.zeros((n, n), dtype=p.dtype)
    for c in range(dim):  # ((dx dx + dy dy) + dz dz): the sum order of the library's canonical d2
        d = p[:, None, c] - p[None, :, c]
        d2 = d2 + d * d if c else d * d
    return np.argsort(d2, axis=1, kind="stable")[:, :k].astype(np.int64)  # stable: ties by index


def dots(nrm, a, b):
    d = nrm[a, 0] * nrm[b, 0] + nrm[a, 1] * nrm[b, 1]
    if nrm.shape[1] == 3:
        d = d + nrm[a, 2] * nrm[b, 2]
    return d


def weights(nrm, a, b):
    T = nrm.dtype.type
    return (T(1) - np.abs(dots(nrm, a, b))) + T(np.finfo(T).eps) * T(100)


def edges_of(rows):
    """distinct undirected edges (a < b) of the row graph, in (a, b) order"""
    n, k = rows.shape
    src = np.repeat(rows[:, 0], k - 1)
    dst = rows[:, 1:].reshape(-1)
    a, b = np.minimum(src, dst), np.maximum(src, dst)
    key = np.unique(a * n + b)
    return key // n, key % n


class _Dsu:
    def __init__(self, n):
        self.p = list(range(n))

    def find(self, a):
        p = self.p
        r = a
        while p[r] != r:
            r = p[r]
        while p[a] != r:
            p[a], a = r, p[a]
        return r


def kruskal(n, a, b, w):
    """edge ids of the minimum spanning forest under (w, a, b)"""
    order = np.lexsort((b, a, w))
    dsu = _Dsu(n)
    tree = []
    for e in order.tolist():
        ra, rb = dsu.find(int(a[e])), dsu.find(int(b[e]))
        if ra != rb:
            dsu.p[ra] = rb
            tree.append(e)
    return np.array(sorted(tree), dtype=np.int64)


def start_of(p):
    return int(np.argmax(p[:, -1]))


def orient_model(p, nrm, k):
    """dict: normals (new array), mst (sorted (m, 2) int32), info counts, plus rows / a / b / w / tree for the checks"""
    p = np.ascontiguousarray(p)
    n = len(p)
    rows = rows_of(p, k)
    a, b = edges_of(rows) if k > 1 else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    w = weights(nrm, a, b)
    tree = kruskal(n, a, b, w)
    adj = [[] for _ in range(n)]
    for e in tree.tolist():
        adj[int(a[e])].append(int(b[e]))
        adj[int(b[e])].append(int(a[e]))
    out = nrm.copy()
    start = start_of(p)
    flipped = 0
    if out[start, -1] < 0:
        out[start] = -out[start]
        flipped += 1
    seen = np.zeros(n, dtype=bool)
    seen[start] = True
    stack = [start]
    while stack:
        v = stack.pop()
        for u in adj[v]:
            if not seen[u]:
                seen[u] = True
                if dots(out, u, v) < 0:
                    out[u] = -out[u]
                    flipped += 1
                stack.append(u)
    mst = np.stack([a[tree], b[tree]], axis=1).astype(np.int32).reshape(-1, 2)
    info = dict(n_edges=len(a), n_components=n - len(tree), n_reached=int(seen.sum()), n_flipped=flipped, start=start)
    return dict(normals=out, mst=mst, info=info, rows=rows, a=a, b=b, w=w, tree=tree, seen=seen)


def angles(nrm, a, b):
    """_angle (src/utils.jl:18-23) of the pairs, in double"""
    u, v = nrm[a].astype(np.float64), nrm[b].astype(np.float64)
    if nrm.shape[1] == 2:
        return np.arctan2(u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0], u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1])
    cx = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1]
    cy = u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2]
    cz = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
    return np.arctan2(np.sqrt((cx * cx + cy * cy) + cz * cz), (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2])


def components_model(p, nrm, k, angle):
    """dict: labels (int32), info counts, the directed entries' angles"""
    p = np.ascontiguousarray(p)
    n = len(p)
    rows = rows_of(p, k)
    src = np.repeat(rows[:, 0], k - 1)
    dst = rows[:, 1:].reshape(-1)
    th = angles(nrm, src, dst)
    keep = np.abs(th) < angle
    dsu = _Dsu(n)
    for x, y in zip(src[keep].tolist(), dst[keep].tolist()):
        rx, ry = dsu.find(x), dsu.find(y)
        if rx != ry:
            dsu.p[max(rx, ry)] = min(rx, ry)
    labels = np.array([dsu.find(i) for i in range(n)], dtype=np.int32)
    a, _ = edges_of(rows) if k > 1 else (np.zeros(0), None)
    return dict(labels=labels, info=dict(n_edges=len(a), n_components=len(np.unique(labels))), theta=th)


def boruvka_parity(n, nrm, a, b, w, start, start_flip):
    """The algorithm of the kernels in plain Python: rounds in which every component takes its smallest outgoing edge
    under (w, a, b) (offered from both endpoints), two components that chose the same edge keep the smaller
    representative, and a parity bit per vertex, relative to its representative, is carried through the hooks
    (par(rep c -> rep p) = par(u) ^ sigma(u, v) ^ par(v)) and the pointer jumps.  Returns (sorted tree edge ids,
    flip decision per vertex, rounds)."""
    rep = list(range(n))
    par = [0] * n
    sigma = (dots(nrm, a, b) < 0).astype(np.int64).tolist()
    al, bl = a.tolist(), b.tolist()
    keys = list(zip(w.tolist(), al, bl))
    tree, rounds = [], 0
    while True:
        best = {}
        for e in range(len(al)):
            cu, cv = rep[al[e]], rep[bl[e]]
            if cu != cv:
                for c in (cu, cv):
                    if c not in best or keys[e] < keys[best[c]]:
                        best[c] = e
        if not best:
            break
        rounds += 1
        link = {}
        for c, e in best.items():
            u, v = (al[e], bl[e]) if rep[al[e]] == c else (bl[e], al[e])
            p = rep[v]
            if best.get(p) == e and c < p:
                continue
            link[c] = (p, par[u] ^ sigma[e] ^ par[v])
            tree.append(e)
        state = [(rep[v], par[v]) for v in range(n)]
        for c, (p, q) in link.items():
            state[c] = (p, q)
        changed = True
        while changed:  # pointer jumping, synchronous
            changed = False
            new = list(state)
            for v in range(n):
                p, q = state[v]
                pp, qq = state[p]
                if p != v and pp != p:
                    new[v] = (pp, q ^ qq)
                    changed = True
            state = new
        rep = [s[0] for s in state]
        par = [s[1] for s in state]
    flip = [rep[v] == rep[start] and bool(par[v] ^ par[start] ^ int(start_flip)) for v in range(n)]
    return np.array(sorted(tree), dtype=np.int64), np.array(flip), rounds


# ---- clouds ---------------------------------------------------------------------------------------------------------
def fib_sphere(n):
    i = np.arange(n) + 0.5
    phi = np.arccos(1 - 2 * i / n)
    th = np.pi * (1 + np.sqrt(5)) * i
    return np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], axis=1)


def unit(x):
    return x / np.linalg.norm(x, axis=1)[:, None]


def _random(n, dim, seed):
    rng = np.random.default_rng(seed)
    return rng.random((n, dim)), unit(rng.standard_normal((n, dim)))


def _tiny(n, k):
    p, nrm = _random(n, 3, 100 + n)
    nrm[:, -1] = -np.abs(nrm[:, -1])  # the start's flip is exercised
    return p, nrm, k


def _fib_random(n=300, k=6):
    return fib_sphere(n), unit(np.random.default_rng(5).standard_normal((n, 3))), k


def _quantised(n=257, k=5):
    rng = np.random.default_rng(6)
    q = rng.integers(-2, 3, size=(n, 3))
    q[(q == 0).all(axis=1)] = (1, 0, -2)
    return rng.random((n, 3)), q / 2.0, k


def _two_spheres(offset_axis, k=5):
    a, b = fib_sphere(100), 0.8 * fib_sphere(80)
    nrm = np.concatenate([a, b / 0.8]) * np.random.default_rng(7).choice([-1.0, 1.0], size=(180, 1))
    b[:, offset_axis] += 5.0
    return np.concatenate([a, b]), nrm, k


def _shared_top(n=65, k=4):
    p, nrm = _random(n, 3, 8)
    p[40, -1] = p[7, -1] = 2.0
    return p, nrm, k


def _coincident(m=40, k=4):
    rng = np.random.default_rng(9)
    q = rng.random((m, 3))
    return np.concatenate([q, q]), unit(rng.standard_normal((2 * m, 3))), k


def chain_points(n=4097):
    p = np.zeros((n, 3))
    p[:, 0] = np.arange(n)
    return p


def _chain(n=4097, k=3):
    """Collinear, unit spacing (exact distance ties, the left neighbour first).  The normals turn by sqrt(2 g (i + 1))
    between i and i + 1, so 1 - cos grows by g = 2e-6 per edge, well above the rounding of a float32 dot (1.2e-7):
    the weights increase strictly along the line and every vertex's lightest edge is its left one.  Random signs make
    the parities non-trivial without changing a weight."""
    step = np.sqrt(2 * 2.0e-6 * (np.arange(n - 1) + 1))
    th = np.concatenate([[0.0], np.cumsum(step)])
    nrm = np.stack([np.zeros(n), np.sin(th), np.cos(th)], axis=1)
    nrm *= np.random.default_rng(10).choice([-1.0, 1.0], size=(n, 1))
    return chain_points(n), nrm, k


def _circle2d(n=65, k=3):
    th = 2 * np.pi * np.arange(n) / n
    p = np.stack([np.cos(th), np.sin(th)], axis=1)
    return p, p * np.random.default_rng(11).choice([-1.0, 1.0], size=(n, 1)), k


# name -> (builder, claims).  Claims: ties (exact weight ties exist), tree_dependent (a non-tree edge of the start's
# component joins two output normals with a negative dot), n_components, n_unreached; None = not claimed.
ORIENT_CASES = {
    "n1": (lambda: _tiny(1, 1), dict(n_components=1, n_unreached=0)),
    "n2": (lambda: _tiny(2, 2), dict(n_components=1, n_unreached=0)),
    "n3": (lambda: _tiny(3, 3), dict(n_components=1, n_unreached=0)),
    "n3_k1": (lambda: _tiny(3, 1), dict(n_components=3, n_unreached=2)),
    "n63": (lambda: _random(63, 3, 63) + (4,), dict(tree_dependent=True)),
    "n64": (lambda: _random(64, 3, 64) + (4,), dict(tree_dependent=True)),
    "n65": (lambda: _random(65, 3, 65) + (4,), dict(tree_dependent=True)),
    "n257": (lambda: _random(257, 3, 257) + (4,), dict(tree_dependent=True)),
    "fib_random": (_fib_random, dict(tree_dependent=True, n_components=1, n_unreached=0)),
    "quantised": (_quantised, dict(ties=True, tree_dependent=True, zero_dots=True, wide_weights=True)),
    "two_spheres": (lambda: _two_spheres(0), dict(n_components=2, n_unreached=80, start_below=100)),
    "start_in_smaller": (lambda: _two_spheres(2), dict(n_components=2, n_unreached=100, start_from=100)),
    "shared_top": (_shared_top, dict(start=7)),
    "coincident": (_coincident, dict(ties=False, twin_slot0=40, many_components=True)),
    "chain": (_chain, dict(n_components=1, n_unreached=0, left_edges=True)),
    "circle2d": (_circle2d, dict(n_components=1, n_unreached=0)),
}


def _cube(m=4):
    g = (np.arange(m) + 0.5) / m
    u, v = np.meshgrid(g, g, indexing="ij")
    pts, nrm = [], []
    for axis in range(3):
        for side in (0.0, 1.0):
            c = np.zeros((m * m, 3))
            c[:, axis], c[:, (axis + 1) % 3], c[:, (axis + 2) % 3] = side, u.ravel(), v.ravel()
            nn = np.zeros_like(c)
            nn[:, axis] = 1.0 if side else -1.0
            pts.append(c)
            nrm.append(nn)
    pts, nrm = np.concatenate(pts), np.concatenate(nrm)
    perm = np.random.default_rng(2).permutation(len(pts))
    return pts[perm], nrm[perm], 10, np.radians(80.0)


def _split_chain(n=4097):
    th = 0.01 * np.arange(n)  # 0.01 rad between neighbours, 41 rad in all: one component through a long chain
    return chain_points(n), np.stack([np.zeros(n), np.sin(th), np.cos(th)], axis=1), 3, 0.015


def _isolated(n=100):
    p, nrm = _random(n, 3, 12)
    return p, nrm, 6, 1.0e-6


def _polygon2d(m=16):
    """a square's boundary walked counter-clockwise, m points per side, outward normals: the signed angle between the
    two sides of a corner is +pi/2 one way round and -pi/2 the other"""
    t = (np.arange(m) + 0.5) / m
    sides = [(np.stack([t, 0 * t], 1), (0, -1)), (np.stack([1 + 0 * t, t], 1), (1, 0)),
             (np.stack([1 - t, 1 + 0 * t], 1), (0, 1)), (np.stack([0 * t, 1 - t], 1), (-1, 0))]
    p = np.concatenate([s for s, _ in sides])
    nrm = np.concatenate([np.tile(np.array(d, dtype=float), (m, 1)) for _, d in sides])
    return p, nrm, 3, np.radians(80.0)


SPLIT_CASES = {
    "cube": (_cube, dict(n_components=6)),
    "chain": (_split_chain, dict(n_components=1)),
    "isolated": (_isolated, dict(n_components=100)),
    "polygon2d": (_polygon2d, dict(n_components=4, signed=True)),
}


@functools.lru_cache(maxsize=None)
def orient_case(name, dtype):
    """(points, normals, k) in dtype and the model's answer; computed once, shared, never written to"""
    p, nrm, k = ORIENT_CASES[name][0]()
    p, nrm = np.ascontiguousarray(p.astype(dtype)), np.ascontiguousarray(nrm.astype(dtype))
    ref = orient_model(p, nrm, k)
    for arr in (p, nrm, ref["normals"], ref["mst"]):
        arr.setflags(write=False)
    return p, nrm, k, ref


@functools.lru_cache(maxsize=None)
def split_case(name, dtype):
    p, nrm, k, angle = SPLIT_CASES[name][0]()
    p, nrm = np.ascontiguousarray(p.astype(dtype)), np.ascontiguousarray(nrm.astype(dtype))
    ref = components_model(p, nrm, k, float(angle))
    for arr in (p, nrm, ref["labels"]):
        arr.setflags(write=False)
    return p, nrm, k, float(angle), ref
