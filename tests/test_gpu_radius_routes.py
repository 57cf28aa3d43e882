"""Every RadiusTopology kernel against the CPU oracle at its row-length and density edges, with a per-query witness.

One ctx.radius() runs up to five kernels and the data decide which of them writes a row: the lane-per-query brick
kernel (fp32, rows <= 32, brick halo <= 1600), the brick-staged dense kernel (rows <= 128; fp32 halos in (1600, hcap],
fp64 and rad_wave_only grids every halo <= hcap), the wave kernel's count phase with ranking (nothing in front of it:
fp64 with WTP_RADIUS_DENSE=0, WTP_FORCE_GENERIC=1; rows up to the wave's share of the arena), the wave kernel's fill
phase (rows <= 512) and the serial kernel.  Context.radius_marks() (wtp_radius_marks) returns the count phase's mark of
every query and the grid it ran on; `radius_stage` and `predict_marks` restate the dispatch from them, each rule naming
the C++ line it mirrors.  test_radius_cases.py checks on the host that the cells below hold what they claim.

Bars for every cell: offsets and ids bit-exact against the oracle (kd-tree above 2000 points, brute force below),
against the same call under WTP_RADIUS_DENSE=0 and under WTP_FORCE_GENERIC=1, and radius_two_phase equal to radius.
Witness: every probe centre carries the stage its cell names; every query's mark equals the mark the restated dispatch
predicts wherever that is determined (see predict_marks); the sparse fp32 cells have >= 90 % of their queries at mark 1
and the fp64 and dense cells whose rows all fit (stars on an empty-row background, islands) >= 90 % at mark 2.

Probe rows ("stars"): a centre and m satellites at integer offsets (units of H = 2^-11) inside the centre's ball of
r = RI * H, in a hole of the background of radius 3 r — the centre's row has exactly m entries, mirror images tie in d2
exactly in fp32 and fp64, a coincident pair ties at equal d2 by index, and with `ties` some satellites sit at exactly
d2 == r * r.  The backgrounds of the star cells are jittered lattices whose points are further than r apart: their rows
are empty, so they neither fill the arena nor outgrow any kernel, and the marks of a star cell are fully predictable.

The dense kernel's arena at these sizes.  The arena holds 48 n ids and the dense kernel takes it in pieces of 2048 per
wave (kRdChunk).  A wave with a non-empty row takes a piece, so the arena is used up once 48 n / 2048 waves hold one:
with 512 x 16 waves that takes n >= 350 k points; below that a uniform cloud exhausts the arena long before 48 n ids
are parked, and which wave finds it empty is a race (measured, fp64 uniform, 40 000 points, rows of about 40: pieces
for 64.5 M ids asked of an arena of 1.92 M, 9 460 rows parked and 30 540 handed back to the wave kernel; the `islands`
cells are built so that whole pieces suffice, and park every row).  That costs time on small clouds, never a row (the
RadiusTopology row of the buffer table); no cell asserts that it happens, so a better use of the arena passes.  The
marks of rows <= 128 are predicted only while info["arena_taken"] shows the arena was not used up; empty rows ask for
no piece and are always parked.

The wave kernel's own arena (WTP_RADIUS_DENSE=0 in fp64, WTP_FORCE_GENERIC=1) is shared out evenly among the waves.  Up
to 65 536 points a wave takes one query, so a row is parked iff it fits the share; the `shares` cell has 72 176 points,
its waves take two, and predict_share_marks restates the accumulation: a second row of 30 finds the share of 52 used
by the first, a second row of 10 is parked behind it.
"""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64

# ---- the dispatch, restated ---------------------------------------------------------------------------------------

BRICK_ROW = 32        # wtp_brick.hip:713 (cnt > 32: handed back) and the 32 ids per query of rad_tmp
RAD_DENSE_MIN = 1600  # wtp_internal.hpp kRadDenseMin; wtp_brick.hip:299-301
RD_CAP = 128          # wtp_radb.hip kRdCap (:365 park = m <= kRdCap)
RD_CHUNK = 2048       # wtp_radb.hip kRdChunk (:366-374)
WTP_ERR_STATE = 4     # include/wtp.h
RAD_CAP = 512         # wtp_wave.hip kRadCap (:533 longer rows: the fb2 list, the serial kernel)
ARENA_PER_POINT = 48  # wtp_internal.hpp kRadArenaPerPoint (wtp_topology.hip radius_count_t: arena_cap)
WAVE_ONLY = 30.0      # wtp_hash.hip:178
SHELL_MIN = 16        # wtp_radb.hip:112 (rows beyond 16 are grouped into shells)
TWO_PER_LANE = 64     # wtp_radb.hip:65 (rows beyond 64: two entries per lane)
STAGES = {"brick", "dense", "wave-arena", "wave-fill", "serial"}


def rd_hcap(dtype):
    """rd_hcap<T>() of wtp_radb.hip:443-446: LDS points of the dense kernel (80 KiB less its tables and 16 lists)."""
    f64 = np.dtype(dtype) == np.float64
    hcells = 6 * 4 * 4 if f64 else 6 * 6 * 6                 # RdTables<T>: (bx + 2)(by + 2)(bz + 2)
    own_rows = 2 * 2 if f64 else 4 * 4
    tables = 4 * ((hcells + 1) + hcells + (own_rows + 1) + 17 + 1)
    lst = (RD_CAP + 2) * (12 if f64 else 8)                  # RdList<T>
    return (80 * 1024 - tables - 32 - lst * 16) // (32 if f64 else 16) // 64 * 64


def radius_stage(mark, length, dense_used):
    """The kernel that wrote a row, from its mark and length (include/wtp.h, wtp_radius_marks)."""
    if mark == 1:
        return "brick"                                       # wtp_brick.hip:728-732
    if mark == 2:
        return "dense" if dense_used else "wave-arena"       # wtp_radb.hip:385-388 / wtp_wave.hip:551-554
    return "wave-fill" if length <= RAD_CAP else "serial"    # wtp_wave.hip:533-538, wtp_generic.hip:311


def wave_share(n):
    """Ids of the arena one wave of the count phase with ranking owns (wtp_wave.hip:545, grid of :596-597)."""
    return (ARENA_PER_POINT * n) // wave_stride(n)


def expected_row(x, r):
    """Expected row length at the box-average density, as grid_setup_kernel computes it (wtp_hash.hip:174-178)."""
    x = np.asarray(x, np.float64)
    dim = x.shape[1]
    ext = x.max(axis=0) - x.min(axis=0)
    emax = ext.max()
    if not (r > 0 and emax > 0):
        return 0.0
    vol = float(np.prod(np.maximum(ext, emax * 1e-6)))
    ball = 4.18879 * r ** 3 if dim == 3 else 3.14159265 * r * r
    return len(x) / vol * ball


def cells_of(x, info):
    """Cell (cx, cy, cz) of every point on the grid the library reports, in the cloud's own arithmetic (cell_coord,
    wtp_device.hpp:46-50)."""
    T = x.dtype.type
    n3 = np.array(info["cells"], np.int64)
    inv_c = T(1) / T(info["cell_edge"])
    xyz = np.zeros((len(x), 3), x.dtype)
    xyz[:, : x.shape[1]] = x
    org = np.array(info["origin"], np.float64).astype(x.dtype)
    f = np.floor((xyz - org) * inv_c)
    return np.clip(f, 0, (n3 - 1).astype(x.dtype)).astype(np.int64)


def wave_stride(n):
    """Waves of the ranking count (wtp_wave.hip:596-597, four waves per block): query qi belongs to wave qi % stride."""
    return 4 * min(16384, max(64, (n + 3) // 4))


def predict_share_marks(x, lengths, info, with_turn=False):
    """Marks of the count phase with ranking (wtp_wave.hip:530-554).  A wave takes the sorted slots w, w + stride, ... in
    turn and parks a row while its share lasts.  Slots are the points in cell order (z slowest); the order inside a cell
    is not fixed, so a query's turn and its predecessor's row are known as a range: -1 where the range leaves it open."""
    n = len(x)
    stride, share = wave_stride(n), wave_share(n)
    lengths = np.asarray(lengths, np.int64)
    first = np.where(lengths <= share, 2, 0)                            # arena_used == 0: wtp_wave.hip:546
    if n <= stride or n > 2 * stride:
        out = first if n <= stride else np.full(n, -1)
        return (out, np.zeros(n, bool)) if with_turn else out
    n3 = np.array(info["cells"], np.int64)
    c = cells_of(x, info)
    lin = (c[:, 2] * n3[1] + c[:, 1]) * n3[0] + c[:, 0]                  # row-major, z slowest (wtp_internal.hpp: cell_start)
    cnt = np.bincount(lin, minlength=int(n3.prod()))
    start = np.concatenate([[0], np.cumsum(cnt)])
    used = np.where(lengths <= share, lengths, 0)                       # ids a first row takes from its wave's share
    big = np.iinfo(np.int64).max
    cmin = np.full(len(cnt), big)
    cmax = np.zeros(len(cnt), np.int64)
    np.minimum.at(cmin, lin, used)
    np.maximum.at(cmax, lin, used)
    slot_cell = np.repeat(np.arange(len(cnt)), cnt)                      # cell of every slot
    lo_slot, hi_slot = cmin[slot_cell], cmax[slot_cell]
    s0, s1 = start[lin], start[lin + 1]
    out = np.full(n, -1)
    out[s1 <= stride] = first[s1 <= stride]
    for i in np.flatnonzero(s0 >= stride):                              # second in its wave: arena_used = its predecessor's row
        a, b = s0[i] - stride, s1[i] - stride
        if lengths[i] > share or lengths[i] + lo_slot[a:b].min() > share:
            out[i] = 0
        elif lengths[i] + hi_slot[a:b].max() <= share:
            out[i] = 2
    return (out, s0 >= stride) if with_turn else out


def brick_halos(x, info, bricks):
    """Per query, the points in the halo of its brick (wtp_brick.hip:257-295, wtp_radb.hip:188-224)."""
    n3 = np.array(info["cells"], np.int64)
    cell = cells_of(x, info)
    cnt = np.zeros(tuple(n3 + 2), np.int64)                  # one empty cell around the grid
    np.add.at(cnt, tuple((cell + 1).T), 1)
    b = np.array(bricks, np.int64)
    lo = cell // b * b                                       # first own cell of the query's brick
    S = cnt.cumsum(0).cumsum(1).cumsum(2)
    S = np.pad(S, ((1, 0), (1, 0), (1, 0)))
    a0 = np.clip(lo - 1 + 1, 0, n3 + 2)                      # halo [lo - 1, lo + b], shifted by the padding cell
    a1 = np.clip(lo + b + 1 + 1, 0, n3 + 2)
    x0, y0, z0 = a0.T
    x1, y1, z1 = a1.T
    return (S[x1, y1, z1] - S[x0, y1, z1] - S[x1, y0, z1] - S[x1, y1, z0] + S[x0, y0, z1] + S[x0, y1, z0]
            + S[x1, y0, z0] - S[x0, y0, z0])


def predict_marks(x, lengths, info, env):
    """The mark of every query as the dispatch decides it: 0 / 1 / 2, -1 where a race decides (a row <= 128 of the
    dense kernel once the arena is used up), -2 where the brick kernel may serve or hand back (mark 0 or 1, never 2)."""
    n = len(x)
    f64 = x.dtype == np.float64
    generic = env.get("WTP_FORCE_GENERIC") == "1"
    dense = env.get("WTP_RADIUS_DENSE", "1") != "0" and not generic     # wtp_generic.hip:274
    lengths = np.asarray(lengths)
    if generic or (f64 and not dense):                                  # wtp_generic.hip:291, wtp_wave.hip:598: ranking count
        return predict_share_marks(x, lengths, info)
    wave_only = bool(info["rad_wave_only"])
    hcap = rd_hcap(x.dtype)
    out = np.zeros(n, np.int64)
    if dense:
        halo = brick_halos(x, info, (4, 2, 2) if f64 else (4, 4, 4))    # RdGeom<T>
        lo = -1 if (f64 or wave_only) else RAD_DENSE_MIN                # wtp_radb.hip:172
        served = (halo > lo) & (halo <= hcap)                           # wtp_radb.hip:225, :240
        used_up = info["arena_taken"] + RD_CHUNK > info["arena_cap"]    # wtp_radb.hip:371
        out[served & (lengths <= RD_CAP)] = -1 if used_up else 2
        out[served & (lengths == 0)] = 2                                # an empty row asks for no piece (m > chunk_left is false, wtp_radb.hip:366)
    if not f64 and not wave_only:                                       # wtp_brick.hip:229
        halo = brick_halos(x, info, (4, 4, 4))
        mine = halo <= RAD_DENSE_MIN                                    # wtp_brick.hip:299 (its LDS area of 2560 lies above)
        out[mine & (lengths <= BRICK_ROW)] = -2                         # wtp_brick.hip:713
    return out


# ---- constructions --------------------------------------------------------------------------------------------------

H = 2.0 ** -11
RI = 10                      # r = RI * H: r * r and every d2 of a star are exact in fp32 and fp64
STAR_M = (16, 17, 32, 33, 64, 65, 128, 129, 512, 513)


def _ball_points():
    g = np.arange(-RI, RI + 1)
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    d2 = (p * p).sum(1)
    return p[(d2 > 0) & (d2 < RI * RI)], p[d2 == RI * RI]


def star_offsets(m, ties, seed):
    """Integer offsets (units of H) of the m satellites of a star: two satellites ON the centre (d2 = 0 ties ranked by
    index), mirror pairs (exact d2 ties), coincident copies of one satellite, and with `ties` six points at exactly
    d2 == r * r ((6, 8, 0) and (10, 0, 0) kin)."""
    inner, rim = _ball_points()
    rng = np.random.default_rng(seed)
    sel = []
    if ties:
        sel += [rim[i] for i in rng.choice(len(rim), 6, replace=False)]
    sel += [np.zeros(3, np.int64)] * 2
    half = inner[(inner[:, 0] > 0)]
    pick = half[rng.choice(len(half), (m - len(sel) - 1) // 2, replace=False)]
    sel += list(pick) + list(-pick)
    while len(sel) < m:                                      # a coincident copy of the first inner satellite (odd rest: two)
        sel.append(pick[0])
    return np.array(sel[:m], np.int64)


def jittered_lattice(per_axis, lo, hi, seed, dim=3):
    """A lattice of spacing s = (hi - lo) / per_axis moved by at most 0.3 s per axis: points at least 0.4 s apart."""
    s = (hi - lo) / per_axis
    g = np.stack(np.meshgrid(*[np.arange(per_axis)] * dim, indexing="ij"), -1).reshape(-1, dim)
    j = np.random.default_rng(seed).uniform(-0.3, 0.3, g.shape)
    return lo + (g + 0.5 + j) * s


def with_stars(bg, sites, ms, ties, seed):
    """Background with a hole of radius 3 r around every site and a star there; returns x (fp64) and the probes
    {m: id of the centre}.  Sites are rounded to multiples of H."""
    r = RI * H
    sites = np.round(np.asarray(sites, np.float64) / H) * H
    keep = np.ones(len(bg), bool)
    for s in sites[: len(ms)]:
        keep &= ((bg - s) ** 2).sum(1) > (3.001 * r) ** 2
    parts, probes, at = [bg[keep]], {}, int(keep.sum())
    for i, (s, m) in enumerate(zip(sites, ms)):
        probes[m] = at
        parts.append(np.concatenate([s[None], s + star_offsets(m, ties, seed + i) * H]))
        at += m + 1
    return np.concatenate(parts), probes


def _sites(nx, ny, nz, lo, hi):
    ax = [np.linspace(lo, hi, k) if k > 1 else np.array([(lo + hi) / 2]) for k in (nx, ny, nz)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)


def lattice(m, dim):
    return np.stack(np.meshgrid(*[np.arange(m, dtype=np.float64)] * dim, indexing="ij"), -1).reshape(-1, dim)


def uniform(n, dim, seed):
    return np.random.default_rng(seed).random((n, dim))


SQRT5_UP = float(np.nextafter(np.float32(np.sqrt(5.0)), np.float32(3)))  # fp32-representable, its square >= 5 in both types


def build(data, dtype):
    """(x in the cell's dtype, r, probes {m: centre id}) of a construction."""
    r = RI * H
    probes = {}
    if data in ("stars", "stars-ties"):                      # sparse background: every brick the brick kernel's (fp32)
        bg = jittered_lattice(27, 0.0, 1.0, 11)
        x, probes = with_stars(bg, _sites(3, 2, 2, 0.2, 0.8), STAR_M, data == "stars-ties", 100)
    elif data in ("zone-stars", "zone-stars-ties"):          # stars up to 129 inside a zone whose brick halos hold ~2900
        bg = jittered_lattice(12, 0.0, 1.0, 12)
        bg = bg[(np.abs(bg - 0.5) > 0.26).any(1)]
        zone = jittered_lattice(36, 0.24, 0.76, 13)
        x, probes = with_stars(np.concatenate([bg, zone]), _sites(2, 2, 2, 0.425, 0.575), STAR_M[:8],
                               data == "zone-stars-ties", 200)
    elif data == "two-zones":                                # halos under 1600, in (1600, 3904] and beyond; fp64: under and over 1728
        bg = jittered_lattice(12, 0.0, 1.0, 14)
        bg = bg[(np.abs(bg - 0.3) > 0.21).any(1) & (np.abs(bg - 0.78) > 0.19).any(1)]
        za = jittered_lattice(28, 0.1, 0.5, 15)              # 343 k per unit volume; each zone is wider than a brick and
        zb = jittered_lattice(29, 0.6, 0.96, 16)             # 523 k per unit volume  its halo, so one halo lies inside it
        x = np.concatenate([bg, za, zb])
    elif data == "wave-only-stars":                          # uniform, 34 expected neighbours: rad_wave_only; stars 512 | 513
        bg = uniform(30000, 3, 17)
        r_u = (34.0 / 30000 / 4.18879) ** (1.0 / 3.0)
        s = H * RI / r_u                                     # scale the cloud so that r = RI * H gives 34 per ball
        x, probes = with_stars(bg * s, _sites(2, 1, 1, 0.3, 0.7) * s, (512, 513), True, 300)
    elif data in ("expect28", "expect32", "rows12", "rows40", "rows60"):
        want = float(data[-2:])
        n = 30000 if data.startswith("expect") else 40000
        x = uniform(n, 3, 18)
        ext = x.max(0) - x.min(0)
        r = float((want * np.prod(ext) / n / 4.18879) ** (1.0 / 3.0))
    elif data == "shares":                                   # 72 176 points: the waves of the ranking count take two queries
        # z slowest in the cell order: the first slots are a slab of groups of 31 (rows of 30), the last slots a slab of
        # groups of 31 and of 11 (rows of 30 and 10); between them a jittered lattice with empty rows.  A wave's share
        # is 52 ids: a second row of 30 finds 30 + 30 > 52 (share full, arena far from it), one of 10 is parked at 30.
        rng = np.random.default_rng(23)

        def groups(sites, sizes):
            return np.concatenate([s + rng.uniform(-0.1 * r, 0.1 * r, (k, 3)) for s, k in zip(sites, sizes)])

        g = np.stack(np.meshgrid(np.arange(20), np.arange(20), indexing="ij"), -1).reshape(-1, 2)
        low = np.concatenate([(g[:300] + 0.5) / 20, np.full((300, 1), 0.05)], 1)
        high = np.concatenate([(g[:364] + 0.5) / 20, np.full((364, 1), 0.95)], 1)
        sizes = rng.permutation([31] * 200 + [11] * 164)
        mid = jittered_lattice(38, 0.0, 1.0, 24)
        mid[:, 2] = 0.15 + 0.7 * mid[:, 2]
        x = np.concatenate([groups(low, [31] * 300), mid, groups(high, sizes)])
    elif data == "islands":                                  # one cluster of 44 points per cell of one brick: rows of 43, all parked
        nxyz = (4, 4, 4) if np.dtype(dtype) == np.float32 else (4, 2, 2)
        s = np.stack(np.meshgrid(*[np.arange(k, dtype=np.float64) for k in nxyz], indexing="ij"), -1).reshape(-1, 3)
        j = np.random.default_rng(19).uniform(-0.02, 0.02, (len(s), 44, 3))
        x = (s[:, None, :] + j).reshape(-1, 3)
        r = 0.9
    elif data.startswith("lattice24"):
        x = lattice(24, 3)
        r = {"lattice24 r=2": 2.0, "lattice24 r=3": 3.0, "lattice24 r=sqrt5": SQRT5_UP, "lattice24 r=2.5": 2.5}[data]
    elif data == "lattice70 r=5":
        x = lattice(70, 2)
        r = 5.0
    elif data in ("coincident", "cluster", "outlier", "coincident r=0"):
        x = uniform(20000, 3, 20)
        r = float((12.0 / 20000 / 4.18879) ** (1.0 / 3.0))
        if data.startswith("coincident"):
            x[100:148] = x[100]
            r = 0.0 if data.endswith("r=0") else r
        elif data == "cluster":
            x[2000:5000] = x[2000] + 1e-4 * (x[2000:5000] - 0.5)
        else:
            x[777] = 1e7 if np.dtype(dtype) == np.float32 else 1e9
    elif data == "whole cloud n=600":
        x, r = uniform(600, 3, 21), 2.0
    elif data in ("n=1", "n=2", "n=33"):
        x, r = uniform(int(data[2:]), 3, 22), 0.4
    else:
        raise ValueError(data)
    return np.ascontiguousarray(x.astype(dtype)), float(r), probes


def _stage_sparse32(m, n=0):   # fp32, brick halo <= 1600
    return "brick" if m <= BRICK_ROW else "wave-fill" if m <= RAD_CAP else "serial"


def _stage_dense(m, n=0):      # a brick of the dense kernel
    return "dense" if m <= RD_CAP else "wave-fill" if m <= RAD_CAP else "serial"


def _stage_fill(m, n=0):       # nothing parks: fp32 wave-only grid with the dense kernel off
    return "wave-fill" if m <= RAD_CAP else "serial"


def _stage_arena(m, n):        # the ranking count, one query per wave: rows up to the wave's share are parked
    return "wave-arena" if m <= wave_share(n) else "wave-fill" if m <= RAD_CAP else "serial"


def probe_ms(data):
    """Row lengths of the stars a construction holds."""
    return STAR_M[:8] if data.startswith("zone-stars") else (512, 513) if data == "wave-only-stars" else \
        STAR_M if data.startswith("stars") else ()


# (label, dtype, data, env, scale exponent, stage of the probe rows, witness class)
#   witness: "mark1" / "mark2": >= 90 % of the queries carry that mark; "flag0" / "flag1": the grid's rad_wave_only;
#   "zones": every kind of brick is present and both marks 1 and 2 (fp64: 2 and 0); "shells" / "rim": the dense kernel
#   parked rows it groups into shells / such rows with hits at d2 == r * r; "share(s)": the wave kernel's own arena
CELLS = [
    # row length 32 | 33 (and every other star) behind the brick kernel
    ("f32 stars", F32, "stars", {}, 0, _stage_sparse32, "mark1"),
    ("f32 stars ties", F32, "stars-ties", {}, 0, _stage_sparse32, "mark1"),
    # row length 16 | 17, 64 | 65, 128 | 129 inside the dense kernel: fp32 bricks with a halo in (1600, hcap], fp64 every brick
    ("f32 zone stars", F32, "zone-stars", {}, 0, _stage_dense, "zones"),
    ("f32 zone stars ties", F32, "zone-stars-ties", {}, 0, _stage_dense, "zones"),
    ("f64 stars", F64, "stars", {}, 0, _stage_dense, "mark2"),
    ("f64 stars ties", F64, "stars-ties", {}, 0, _stage_dense, "mark2"),
    # the wave kernel's own arena (nothing in front of it): rows up to the wave's share of 47 ids, 32 | 33 inside it
    ("f64 stars ties dense off", F64, "stars-ties", {"WTP_RADIUS_DENSE": "0"}, 0, _stage_arena, "share"),
    ("f32 stars ties generic", F32, "stars-ties", {"WTP_FORCE_GENERIC": "1"}, 0, _stage_arena, "share"),
    # row length 512 | 513: fp64 above, and fp32 on a wave-only grid with the dense kernel off
    ("f32 wave-only stars dense off", F32, "wave-only-stars", {"WTP_RADIUS_DENSE": "0"}, 0, _stage_fill, "flag1"),
    # halo edges 1600, rd_hcap<float>() and rd_hcap<double>(): two zones, the bricks classified from the reported grid
    ("f32 two zones", F32, "two-zones", {}, 0, None, "zones"),
    ("f64 two zones", F64, "two-zones", {}, 0, None, "zones"),
    # rad_wave_only at 30 expected neighbours (the variants run both with the dense kernel off)
    ("f32 expect 28", F32, "expect28", {}, 0, None, "flag0"),
    ("f32 expect 32", F32, "expect32", {}, 0, None, "flag1"),
    ("f32 rows 12", F32, "rows12", {}, 0, None, "mark1"),
    # the arena: rows all parked (islands), and used up (uniform fp64 clouds; the variants fill the per-wave shares)
    ("f32 islands", F32, "islands", {}, 0, None, "mark2"),
    ("f64 islands", F64, "islands", {}, 0, None, "mark2"),
    ("f64 arena rows 40", F64, "rows40", {}, 0, None, "arena-under"),
    ("f64 arena rows 60", F64, "rows60", {}, 0, None, "arena-over"),
    # the per-wave shares: two queries per wave, the second finds its wave's share used (n > 65 536)
    ("f64 shares dense off", F64, "shares", {"WTP_RADIUS_DENSE": "0"}, 0, None, "shares"),
    # exact ties at the cut inside the dense kernel
    ("f32 lattice24 r=2", F32, "lattice24 r=2", {}, 0, None, "rim"),
    ("f64 lattice24 r=2", F64, "lattice24 r=2", {}, 0, None, "rim"),
    ("f32 lattice24 r=3", F32, "lattice24 r=3", {}, 0, None, "rim"),
    ("f64 lattice24 r=3", F64, "lattice24 r=3", {}, 0, None, "rim"),
    ("f32 lattice24 r=sqrt5", F32, "lattice24 r=sqrt5", {}, 0, None, "shells"),
    ("f64 lattice24 r=sqrt5", F64, "lattice24 r=sqrt5", {}, 0, None, "shells"),
    ("f32 lattice24 r=2.5", F32, "lattice24 r=2.5", {}, 0, None, "shells"),
    ("f64 lattice24 r=2.5", F64, "lattice24 r=2.5", {}, 0, None, "shells"),
    ("f32 2d lattice70 r=5", F32, "lattice70 r=5", {}, 0, None, "rim"),
    ("f64 2d lattice70 r=5", F64, "lattice70 r=5", {}, 0, None, "rim"),
    # power-of-two scale invariance: one sparse and one dense cell per type
    ("f32 stars ties x2^20", F32, "stars-ties", {}, 20, _stage_sparse32, "mark1"),
    ("f32 stars ties x2^-20", F32, "stars-ties", {}, -20, _stage_sparse32, "mark1"),
    ("f32 zone stars ties x2^20", F32, "zone-stars-ties", {}, 20, _stage_dense, "zones"),
    ("f32 zone stars ties x2^-20", F32, "zone-stars-ties", {}, -20, _stage_dense, "zones"),
    ("f64 stars ties x2^40", F64, "stars-ties", {}, 40, _stage_dense, "mark2"),
    ("f64 stars ties x2^-40", F64, "stars-ties", {}, -40, _stage_dense, "mark2"),
    # stress data in every stage
    ("f32 coincident", F32, "coincident", {}, 0, None, None),
    ("f64 coincident", F64, "coincident", {}, 0, None, None),
    ("f32 coincident r=0", F32, "coincident r=0", {}, 0, None, None),
    ("f64 coincident r=0", F64, "coincident r=0", {}, 0, None, None),
    ("f32 cluster", F32, "cluster", {}, 0, None, None),
    ("f64 cluster", F64, "cluster", {}, 0, None, None),
    ("f32 outlier", F32, "outlier", {}, 0, None, None),
    ("f64 outlier", F64, "outlier", {}, 0, None, None),
    ("f32 whole cloud n=600", F32, "whole cloud n=600", {}, 0, None, None),
    ("f64 whole cloud n=600", F64, "whole cloud n=600", {}, 0, None, None),
    ("f32 n=1", F32, "n=1", {}, 0, None, None),
    ("f64 n=2", F64, "n=2", {}, 0, None, None),
    ("f32 n=33", F32, "n=33", {}, 0, None, None),
    ("f64 n=33", F64, "n=33", {}, 0, None, None),
]


def cases():
    return [pytest.param(*c[1:], id=c[0]) for c in CELLS]


def make_cell(dtype, data, scale):
    x, r, probes = build(data, dtype)
    f = dtype(2.0) ** scale
    return x * f, float(dtype(r) * f), probes


def oracle_method(n):
    return "kdtree" if n > 2000 else "brute"


# ---- the parametrized test --------------------------------------------------------------------------------------------

def _run(wtp, monkeypatch, env, x, r, two_phase=False):
    for key in ("WTP_RADIUS_DENSE", "WTP_FORCE_GENERIC"):
        monkeypatch.delenv(key, raising=False)
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    try:
        with wtp.Context(0) as c:
            off, idx = (c.radius_two_phase if two_phase else c.radius)(x, r)
            marks, info = c.radius_marks()
            return off, idx.copy(), marks.copy(), info
    finally:
        for key in env:
            monkeypatch.delenv(key)


def _check_marks(label, x, lengths, marks, info, env):
    want = predict_marks(x, lengths, info, env)
    fixed = want >= 0
    bad = np.flatnonzero(fixed & (marks != want))
    assert len(bad) == 0, f"{label} {env}: {len(bad)} marks differ from the dispatch, first id {bad[:5]}: " \
                          f"{marks[bad[:5]]} for {want[bad[:5]]}, lengths {np.asarray(lengths)[bad[:5]]}"
    assert not (marks[want == -2] == 2).any(), f"{label} {env}: arena marks in the brick kernel's bricks"
    return want


@pytest.mark.parametrize("dtype,data,env,scale,stage_of,witness", cases())
def test_radius_route_matches_oracle(O, wtp, monkeypatch, dtype, data, env, scale, stage_of, witness):
    label = f"{np.dtype(dtype).name} {data} 2^{scale}"
    x, r, probes = make_cell(dtype, data, scale)
    n = len(x)
    ooff, oidx = O.radius(x, r, oracle_method(n))
    lengths = np.diff(ooff)
    off, idx, marks, info = _run(wtp, monkeypatch, env, x, r)
    bad = np.flatnonzero(np.diff(off) != lengths)
    assert np.array_equal(off, ooff), f"{label}: {len(bad)} row lengths differ from the oracle, first ids {bad[:5]}"
    rows = np.flatnonzero(np.add.reduceat(np.append(idx != oidx, False), ooff[:-1]) * (lengths > 0)) if len(oidx) else []
    assert np.array_equal(idx, oidx), f"{label}: rows differ from the oracle, first ids {rows[:5]} marks {marks[rows[:5]]}"
    if scale:                                                 # the unscaled cell's rows, bit for bit
        x0, r0, _ = make_cell(dtype, data, 0)
        o0, i0 = O.radius(x0, r0, oracle_method(n))
        assert np.array_equal(off, o0) and np.array_equal(idx, i0), f"{label}: rows differ from the unscaled cell's"
    # the witness of the cell's own run
    want = _check_marks(label, x, lengths, marks, info, env)
    stages = {m: radius_stage(int(marks[i]), int(lengths[i]), info["dense_used"]) for m, i in probes.items()}
    cnt = np.bincount(marks, minlength=3)
    seen = {radius_stage(int(k), int(L), info["dense_used"]) for k, L in
            {(int(k), int(min(L, RAD_CAP + 1))) for k, L in zip(marks, lengths)}}
    print(f"[route] {label} n={n} marks0/1/2={cnt[0]}/{cnt[1]}/{cnt[2]} dense_used={int(info['dense_used'])} "
          f"rad_wave_only={info['rad_wave_only']} arena={info['arena_taken']}/{info['arena_cap']} "
          f"cells={info['cells']} stages={sorted(seen)} probes={stages}")
    for m, i in probes.items():
        assert lengths[i] == m, f"{label}: the star of {m} has a row of {lengths[i]}"
        assert stages[m] == stage_of(m, n), f"{label}: the row of {m} entries came from {stages[m]}, not {stage_of(m, n)}"
    if witness == "mark1":
        assert cnt[1] >= 0.9 * n, f"{label}: {cnt[1]} of {n} queries served by the brick kernel"
    elif witness == "mark2":
        assert info["dense_used"] and cnt[2] >= 0.9 * n, f"{label}: {cnt[2]} of {n} queries parked by the dense kernel"
    elif witness in ("flag0", "flag1"):
        assert info["rad_wave_only"] == int(witness[-1]), f"{label}: expected row {expected_row(x, r):.2f}"
        assert (cnt[1] > 0) == (witness == "flag0"), f"{label}: the brick kernel stands aside exactly on a wave-only grid"
    elif witness == "zones":
        if dtype == F32:
            halo = brick_halos(x, info, (4, 4, 4))
            assert (halo <= RAD_DENSE_MIN).any() and ((halo > RAD_DENSE_MIN) & (halo <= rd_hcap(F32))).any(), label
            if data == "two-zones":
                assert (halo > rd_hcap(F32)).any(), f"{label}: no brick beyond the dense kernel's LDS area"
            assert cnt[1] > 0 and cnt[2] > 0, f"{label}: both the brick and the dense kernel serve bricks"
            for m, i in probes.items():
                assert RAD_DENSE_MIN < halo[i] <= rd_hcap(F32), f"{label}: the star of {m} sits in a halo of {halo[i]}"
        else:
            halo = brick_halos(x, info, (4, 2, 2))
            assert (halo <= rd_hcap(F64)).any() and (halo > rd_hcap(F64)).any(), label
            assert cnt[2] > 0 and cnt[0] > 0, f"{label}: bricks inside and beyond the dense kernel's LDS area"
    elif witness in ("arena-under", "arena-over"):
        # rows of 40 n ids fit the arena of 48 n, rows of 60 n do not.  What is determined either way: nothing beyond
        # 128 is parked (predict_marks above), the parked ids fit the arena, and every row is exact (compared above).
        # How many rows <= 128 of the first cell are handed back is the piece granularity's doing (module docstring)
        # and is not asserted, so that a better use of the arena passes
        assert info["dense_used"] and cnt[2] > 0 and int(lengths[marks == 2].sum()) <= info["arena_cap"], label
        if witness == "arena-over":
            assert ((marks == 0) & (lengths <= RD_CAP)).any(), f"{label}: rows within the list handed back by a full arena"
    elif witness in ("shells", "rim"):
        parked = (marks == 2) & (lengths > SHELL_MIN)
        assert info["dense_used"] and parked.any(), f"{label}: no row grouped into shells was parked by the dense kernel"
        if witness == "rim":  # interior rows (the longest) hold a whole shell at d2 == r * r: test_radius_cases.py
            assert (parked & (lengths == lengths.max())).any(), f"{label}: no row with rim hits ranked by the dense kernel"
    elif witness == "share":
        assert not info["dense_used"] and n <= wave_stride(n) and cnt[2] >= 0.9 * n, label
    elif witness == "shares":
        stride, share = wave_stride(n), wave_share(n)
        assert n > stride and (want >= 0).sum() >= 0.99 * n, f"{label}: {(want < 0).sum()} marks left open"
        second = predict_share_marks(x, lengths, info, with_turn=True)[1]  # queries that come second in their wave
        refused = (want == 0) & (lengths <= share) & (lengths > 0)
        after = (want == 2) & second & (lengths > 0)
        assert refused.sum() > 1000 and (marks[refused] == 0).all(), f"{label}: rows <= {share} that found the share used"
        assert after.sum() > 300 and (marks[after] == 2).all(), f"{label}: rows parked second in their wave's share"
        assert int(lengths[marks == 2].sum()) < ARENA_PER_POINT * n // 2, f"{label}: the arena as a whole is far from full"
    assert info["dense_hcap"] == rd_hcap(dtype) and info["arena_cap"] == ARENA_PER_POINT * n
    # the same call on the other routes, and the caller-side scan
    for other in ({}, {"WTP_RADIUS_DENSE": "0"}, {"WTP_FORCE_GENERIC": "1"}):
        if other == env:
            continue
        voff, vidx, vmarks, vinfo = _run(wtp, monkeypatch, other, x, r)
        assert np.array_equal(voff, off) and np.array_equal(vidx, idx), f"{label}: differs under {other}"
        _check_marks(label, x, lengths, vmarks, vinfo, other)
        assert vinfo["dense_used"] == (not other)
        assert vinfo["rad_wave_only"] == info["rad_wave_only"], f"{label}: the grid's flag differs under {other}"
        vc = np.bincount(vmarks, minlength=3)
        print(f"[route] {label} {other}: marks0/1/2={vc[0]}/{vc[1]}/{vc[2]} share={wave_share(n)}")
        if witness in ("arena-under", "arena-over") and "WTP_RADIUS_DENSE" in other:
            # one query per wave here: a row beyond the share of 48 ids is left to the fill phase, the others are parked
            assert vc[0] > 0 and vc[2] > 0, label
    toff, tidx, _, _ = _run(wtp, monkeypatch, env, x, r, two_phase=True)
    assert np.array_equal(toff, off) and np.array_equal(tidx, idx), f"{label}: radius_two_phase differs from radius"


# ---- context reuse ------------------------------------------------------------------------------------------------------

def test_context_reuse_large_small_large(O, wtp):
    """A dense cell, a small sparse one and the dense one again on ONE context: rows and marks as from fresh contexts
    (stale rad_done, rad_arena_off or rad_tmp of the earlier call would show)."""
    for dtype in (F32, F64):
        big, rb, _ = make_cell(dtype, "zone-stars-ties", 0)
        small, rs, _ = make_cell(dtype, "n=33", 0)
        fresh = []
        for x, r in ((big, rb), (small, rs)):
            with wtp.Context(0) as c:
                off, idx = c.radius(x, r)
                fresh.append((off, idx.copy(), c.radius_marks()[0].copy()))
        with wtp.Context(0) as c:
            for which in (0, 1, 0, 1):
                x, r = ((big, rb), (small, rs))[which]
                off, idx = c.radius(x, r)
                marks = c.radius_marks()[0]
                assert np.array_equal(off, fresh[which][0]) and np.array_equal(idx, fresh[which][1])
                assert np.array_equal(marks, fresh[which][2]), "marks of a reused context differ from a fresh one's"
        ooff, oidx = O.radius(big, rb, "kdtree")
        assert np.array_equal(fresh[0][0], ooff) and np.array_equal(fresh[0][1], oidx)


# ---- a call between the two phases ----------------------------------------------------------------------------------------

def _cube():
    v = np.array([(x, y, z) for z in (0, 1) for y in (0, 1) for x in (0, 1)], np.float64)
    t = np.array([(0, 2, 1), (1, 2, 3), (4, 5, 6), (5, 7, 6), (0, 1, 4), (1, 5, 4), (2, 6, 3), (3, 6, 7), (0, 4, 2),
                  (2, 4, 6), (1, 3, 5), (3, 7, 5)], np.int32)
    return v, t


def _between(name, c, wtp, dtype):
    """One other call on the context; large enough to overwrite what a smaller radius count left in shared buffers."""
    y = uniform(30000, 3, 31).astype(dtype)
    if name == "spacing_eval":
        c.spacing_eval(dict(kind=3, p0=0.02, p1=0.09, p2=0.2, boundary=y[:500]), y)
    elif name == "isinside_greens":
        nrm = y[:300] - dtype(0.5)
        c.isinside_greens(y, y[:300], nrm, np.full(300, 0.01, dtype))
    elif name == "mesh":
        c.mesh_set(*_cube())
        c.mesh_query(y, 1e-6)
        c.mesh_clear()
    elif name == "pca_normals":
        c.pca_normals(y, 8)
    elif name == "gradient_limit":
        c.gradient_limit(y, np.full(len(y), 0.1, dtype), 0.2, k=12, max_sweeps=4)
    elif name == "knn":
        c.knn(y, 21)
    elif name == "relax":
        s = float(len(y)) ** (-1.0 / 3.0)
        with c.relax(y, 0, s, dict(kind=2, beta=0.2, u0=1.0, gamma=3.0), 21, s / 2000, s / 20) as sess:
            sess.step(True)
    else:
        raise ValueError(name)


BETWEEN = ("spacing_eval", "isinside_greens", "mesh", "pca_normals", "gradient_limit", "knn", "relax")


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", BETWEEN)
def test_fill_after_an_intervening_call(O, wtp, name, dtype):
    """wtp_radius_offsets, one other call, wtp_radius_fill: the state error of wtp.h or the correct rows — never wrong
    rows with rc = 0."""
    import ctypes as C

    x, r, _ = make_cell(dtype, "stars-ties", 0)
    ooff, oidx = O.radius(x, r, "kdtree")
    with wtp.Context(0) as c:
        n = len(x)
        off = np.empty(n + 1, np.int64)
        lib, h = c._lib, c._h
        rc = lib.wtp_radius_offsets(h, x.ctypes.data_as(C.c_void_p), n, 3, 0 if dtype == F32 else 1, r,
                                    off.ctypes.data_as(C.c_void_p))
        assert rc == 0 and np.array_equal(off, ooff)
        _between(name, c, wtp, dtype)
        idx = np.full(max(int(off[-1]), 1), -1, np.int32)
        rc = lib.wtp_radius_fill(h, None, idx.ctypes.data_as(C.c_void_p))
        print(f"[route] fill after {name} ({np.dtype(dtype).name}): rc={rc}")
        if rc == 0:
            assert np.array_equal(idx[: int(off[-1])], oidx), f"fill after {name} wrote wrong rows with rc = 0"
            # the witness is valid wherever the fill is; a buffer shorter than the cloud is refused, not overrun
            assert len(c.radius_marks()[0]) == n
            short = np.empty(n - 1, np.uint8)
            info = (C.c_double * 13)()
            assert lib.wtp_radius_marks(h, short.ctypes.data_as(C.c_void_p), n - 1, info) == 1  # WTP_ERR_ARG
        else:
            assert rc == WTP_ERR_STATE, f"fill after {name}: rc={rc}"
            marks = np.empty(n, np.uint8)
            info = (C.c_double * 13)()
            assert lib.wtp_radius_marks(h, marks.ctypes.data_as(C.c_void_p), n, info) == WTP_ERR_STATE
        off2, idx2 = c.radius(x, r)                           # and the context still serves the pair afterwards
        assert np.array_equal(off2, ooff) and np.array_equal(idx2, oidx)
