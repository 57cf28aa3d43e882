"""The batch core the three generators share (csrc/wtp_sample.hip: cell tables, cull, rounds in groups of 8, the
three-kernel stop scan in tiles of 2048 positions, append, finish, insert) at the edges the case tables of
test_gpu_surface_sampling.py, test_gpu_volume_fill.py and test_gpu_front.py do not reach:

  1. the second level of the stop scan: a batch of more than 256 tiles (the needle, in one batch of 2^20 darts and
     through the clamp of batch = 0 at 2^20);
  2. a run that ends exactly on a batch or tile seam (position B, the slot behind the batch), and a miss run carried
     through whole batches that accept nothing;
  3. more than one group of rounds: rounds_max and n_batches equal the numpy model's, which decides whole batches as the
     library does;
  4. degenerate cell maps: a box without height, the same far from the origin, and a box so long that its 1e-6 floor sets
     the cell edge.

What a wrong core would do here.  A count carry lost between chunks of the scan leaves the needle's stall run with 15
points instead of 571 (tried on a scratch build); its max_points run would not end at all, position B of a 2^20 batch
being alone in the third chunk, so n never grows.  rounds_max taken within the group reports 2 for cube_r005 instead of
10 (tried).  Not tried on a device, because they can index out of bounds or keep a run from ending: `i >= B` for
`i > B` in sample_scan_c_kernel leaves pos[B] and lastb[B] unwritten, which sample_finish_kernel reads whenever a batch
ends at B or does not end the run (the seam cases and every multi-batch run); scan_tiles(B) without the + 1 drops the
tile that holds B alone (cube_fine at 1686 / 2048 and 2849 / 4096, the needle at 2^20); `(s >> 1) >= round` or `> round
+ 1` in sample_round_kernel changes which round decides a dart and with it rounds_max (all of section 3); a second
group that does not reset `und` never sees its batch decided (cube_r005, grid12_bl); `miss0 + i` without miss0
restarts the miss run at every batch that accepts nothing (one_triangle at batch 1, 7, 10, 25 ends late or never).

The expected values come from the serial loops and the batch models of surface_sampling_cases.py, volume_fill_cases.py
and front_cases.py, which know nothing of cells, tables, tiles or groups; every comparison is exact."""
import numpy as np
import pytest

import front_cases as Fc
import surface_sampling_cases as S
import volume_fill_cases as V

pytestmark = pytest.mark.gpu

F32, F64 = S.F32, S.F64
_DARTS, _SERIAL = {}, {}  # the library's darts per case and the serial runs over them: computed once, never written to


def _ids(rows):
    return ["-".join(np.dtype(x).name if isinstance(x, type) else str(x) for x in row) for row in rows]


def _frozen(arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- the surface sampler ------------------------------------------------------------------------------------------------
def _sampler_darts(ctx, name, dtype, sp, n):
    """At least n of the library's own darts of the case, whose mesh is resident."""
    case = S.case_of(name)
    key = ("sample", name, np.dtype(dtype).name)
    if key not in _DARTS or len(_DARTS[key][0]) < n:
        _DARTS[key] = _frozen(ctx.mesh_sample_darts(sp, case["factor"], S.seed_of(case), 0, n))
    return _DARTS[key]


def _check_sampler(wtp, ctx, name, dtype, batch, max_points=None, rounds=True):
    """One run of the case at `batch` against serial() over the library's darts and, for rounds_max and n_batches,
    batched_run() over the darts of the whole batches the library decides.  Returns (info, n_darts of the model)."""
    case = S.case_of(name)
    v, t = S.mesh_of(name, dtype)
    ctx.mesh_set(v, t)
    sp = wtp.sampling._sampler_spacing(S.library_spacing(wtp, name, dtype))
    max_points = S.max_points_of(case) if max_points is None else max_points
    stall, seed = case["stall_limit"], S.seed_of(case)
    xyz, tri, r = _sampler_darts(ctx, name, dtype, sp, case["horizon"])
    key = ("sample", name, np.dtype(dtype).name, max_points)
    if key not in _SERIAL:
        _SERIAL[key] = S.serial(xyz, r, max_points, stall)
    acc, n_darts, reason = _SERIAL[key]
    nb, whole = S.whole_batches(n_darts, batch)
    info = ctx.mesh_sample(sp, case["factor"], max_points, stall, seed, batch)
    got = ctx.mesh_sample_get(info["n_points"])
    print(f"{name} {np.dtype(dtype).name} batch={batch} max_points={max_points}: n_points={info['n_points']} "
          f"n_darts={info['n_darts']} batches={info['n_batches']} rounds_max={info['rounds_max']} (model: {len(acc)} / {n_darts}, "
          f"{nb} batches)")
    assert info["n_points"] == len(acc) and info["n_darts"] == n_darts and info["stop_reason"] == reason
    assert np.array_equal(got["dart"], acc)
    assert np.array_equal(got["xyz"], xyz[acc]) and np.array_equal(got["tri"], tri[acc]) and np.array_equal(got["r"], r[acc])
    assert info["n_batches"] == nb
    if batch:
        assert info["batch"] == batch and nb == -(-n_darts // batch)
    if rounds:
        xyz, tri, r = _sampler_darts(ctx, name, dtype, sp, whole)
        b = S.batched_run(xyz[:whole], r[:whole], max_points, stall, batch)
        assert np.array_equal(b["acc"], acc) and (b["n_darts"], b["stop_reason"]) == (n_darts, reason)
        assert (info["rounds_max"], info["n_batches"]) == (b["rounds_max"], b["n_batches"])
    return info, n_darts


# ---- the volume fill ----------------------------------------------------------------------------------------------------
def _fill_setup(wtp, ctx, name, dtype):
    case = V.case_of(name)
    v, t = V.mesh_of(name, dtype)
    ctx.mesh_set(v, t)
    sp = wtp.sampling._sampler_spacing(V.library_spacing(wtp, name, dtype))
    seeds = V.seeds_of(name, dtype)[0]
    if not len(seeds):
        sr = np.zeros(0, dtype=dtype)
    elif case["spacing"][0] == "const":
        sr = np.full(len(seeds), dtype(case["factor"]) * dtype(case["spacing"][1]), dtype=dtype)
    else:  # r of the seeds as the library evaluates the law (the device's exp differs from numpy's by an ulp)
        sr = dtype(case["factor"]) * ctx.spacing_eval(sp, seeds)
    return case, sp, seeds, sr


def _fill_darts(ctx, name, dtype, sp, n):
    case = V.case_of(name)
    key = ("fill", name, np.dtype(dtype).name)
    if key not in _DARTS or len(_DARTS[key][0]) < n:
        _DARTS[key] = _frozen(ctx.mesh_fill_darts(sp, case["factor"], V.SEED, 0, n))
    return _DARTS[key]


def _fill_equals(info, got, xyz, r, acc, n_darts, reason, n_in):
    assert info["n_points"] == len(acc) and info["n_darts"] == n_darts and info["stop_reason"] == reason
    assert info["n_inside"] == n_in
    assert np.array_equal(got["dart"], acc) and np.array_equal(got["xyz"], xyz[acc]) and np.array_equal(got["r"], r[acc])


def _check_fill(wtp, ctx, name, dtype, batch, rounds=True):
    """As _check_sampler, over the library's darts and inside flags; n_inside included."""
    case, sp, seeds, sr = _fill_setup(wtp, ctx, name, dtype)
    max_points, stall = V.max_points_of(case), case["stall_limit"]
    xyz, inside, r = _fill_darts(ctx, name, dtype, sp, case["horizon"])
    key = ("fill", name, np.dtype(dtype).name)
    if key not in _SERIAL:
        _SERIAL[key] = V.serial(xyz, inside, r, seeds, sr, max_points, stall)
    acc, n_darts, reason, n_in = _SERIAL[key]
    nb, whole = V.whole_batches(n_darts, batch)
    info = ctx.mesh_fill(sp, case["factor"], seeds, max_points, stall, V.SEED, batch)
    got = ctx.mesh_fill_get(info["n_points"])
    print(f"{name} {np.dtype(dtype).name} batch={batch}: n_points={info['n_points']} n_darts={info['n_darts']} "
          f"n_inside={info['n_inside']} batches={info['n_batches']} rounds_max={info['rounds_max']} (model: {len(acc)} / "
          f"{n_darts}, inside {n_in}, {nb} batches)")
    _fill_equals(info, got, xyz, r, acc, n_darts, reason, n_in)
    assert info["n_batches"] == nb
    if batch:
        assert info["batch"] == batch and nb == -(-n_darts // batch)
    if rounds:
        xyz, inside, r = _fill_darts(ctx, name, dtype, sp, whole)
        b = V.batched_run(xyz[:whole], inside[:whole], r[:whole], seeds, sr, max_points, stall, batch)
        assert np.array_equal(b["acc"], acc) and (b["n_darts"], b["stop_reason"], b["n_inside"]) == (n_darts, reason, n_in)
        assert (info["rounds_max"], info["n_batches"]) == (b["rounds_max"], b["n_batches"])
    return info, n_darts


# ---- 1. the stop scan beyond 256 tiles ------------------------------------------------------------------------------------
def _needle(wtp, ctx, name, dtype, batch):
    """The needle case at `batch` against serial() over the model's own darts, with the oracle's inside flags."""
    case, sp, seeds, sr = _fill_setup(wtp, ctx, name, dtype)
    xyz, inside, r, acc, n_darts, reason, n_in = V.model_run(name, dtype)
    info = ctx.mesh_fill(sp, case["factor"], None, V.max_points_of(case), case["stall_limit"], V.SEED, batch)
    got = ctx.mesh_fill_get(info["n_points"])
    print(f"{name} {np.dtype(dtype).name} batch={batch}: n_points={info['n_points']} n_darts={info['n_darts']} "
          f"n_inside={info['n_inside']} stop_reason={info['stop_reason']} batches={info['n_batches']} batch={info['batch']} "
          f"(model: {len(acc)} / {n_darts}, inside {n_in}, reason {reason})")
    _fill_equals(info, got, xyz, r, acc, n_darts, reason, n_in)
    return case, sp, info, (xyz, inside, r)


@pytest.mark.parametrize("dtype", V.DTYPES)
@pytest.mark.parametrize("name", ["needle", "needle_stall"])
def test_needle_run_ends_in_the_second_chunk_of_the_scan(wtp, ctx, name, dtype):
    """One batch of 2^20 darts is 513 tiles; the run ends in tile 340 (max_points = 618) or 273 (stall_limit = 8929), where
    the counts and the last accepted index come through sample_scan_b_kernel's carry from the first 256 tiles."""
    case, sp, info, _ = _needle(wtp, ctx, name, dtype, 1 << 20)
    assert info["n_batches"] == 1 and info["batch"] == 1 << 20
    assert info["n_darts"] >= V.SCAN_CARRY_FROM
    assert info["stop_reason"] == (2 if name == "needle" else 1)


@pytest.mark.parametrize("dtype", V.DTYPES)
def test_needle_through_the_clamp_of_batch_0(wtp, ctx, dtype):
    """batch = 0 doubles from 4096, reaches 2^20 with the ninth batch and is held there by the clamp from dart 4096 * 511
    on; the run ends in the tenth batch.  The class grid is built on the way, on a mesh that is almost all boundary
    cells: the darts' inside flags and n_inside against the oracle check it."""
    case, sp, info, (xyz, inside, r) = _needle(wtp, ctx, "needle_clamp", dtype, 0)
    assert info["batch"] == 1 << 20 and info["n_darts"] > V.CLAMPED_FROM
    assert info["n_batches"] == V.whole_batches(info["n_darts"], 0)[0] == 10
    # the library's own darts, after the run (with whatever grid it built): positions, flags and r are the model's
    lx, li, lr = ctx.mesh_fill_darts(sp, case["factor"], V.SEED, 0, len(xyz))
    assert np.array_equal(lx, xyz) and np.array_equal(lr, r)
    assert np.array_equal(li, inside), f"inside flags differ at darts {np.nonzero(li != inside)[0][:8]}"


# ---- 2. a stop exactly on a seam ------------------------------------------------------------------------------------------
SEAMS = [(1686, 2048), (1686, 2047), (1686, 4096), (2849, 4096)]


@pytest.mark.parametrize("dtype", S.DTYPES)
@pytest.mark.parametrize("max_points,batch", SEAMS)
def test_run_ends_on_a_tile_or_batch_seam(wtp, ctx, max_points, batch, dtype):
    info, n_darts = _check_sampler(wtp, ctx, "cube_fine", dtype, batch, max_points=max_points)
    assert n_darts == (2048 if max_points == 1686 else 4096)          # the last sample is the dart in front of the seam
    if (max_points, batch) == (1686, 2048):    # the run ends at B, alone in the second tile
        assert info["n_darts"] == batch and info["n_darts"] % batch == 0 and info["n_batches"] == 1
    if (max_points, batch) == (1686, 2047):    # ... at position 1 of the second batch
        assert info["n_darts"] == batch + 1 and info["n_batches"] == 2
    if (max_points, batch) == (1686, 4096):    # ... at the first position of tile 1
        assert info["n_darts"] == 2048 and info["n_batches"] == 1
    if (max_points, batch) == (2849, 4096):    # ... at B behind two full tiles
        assert info["n_darts"] == batch and info["n_darts"] % batch == 0 and info["n_batches"] == 1


@pytest.mark.parametrize("dtype", S.DTYPES)
@pytest.mark.parametrize("name", ["cube_max37", "cube_stall3", "one_triangle"])
def test_sampler_batch_ends_with_the_run(wtp, ctx, name, dtype):
    """batch in {N - 1, N, N + 1} around the run's N darts; on one_triangle also batches that the 50-miss run crosses
    whole, with nothing accepted in them."""
    n = S.model_run(name, dtype)[4]
    for batch in [n - 1, n, n + 1] + ([1, 7, 10, 25] if name == "one_triangle" else []):
        info, n_darts = _check_sampler(wtp, ctx, name, dtype, batch)
        assert n_darts == n
    if name == "one_triangle":
        assert info["n_points"] == 1 and info["n_batches"] == 3 and n == 51   # batch 25: batch 2 accepts nothing, batch 3 ends at 1


@pytest.mark.parametrize("dtype", V.DTYPES)
@pytest.mark.parametrize("name", ["cube_stall200", "cube_const10"])
def test_fill_batch_ends_with_the_run(wtp, ctx, name, dtype):
    n = V.model_run(name, dtype)[4]
    for batch in (n - 1, n, n + 1):
        info, n_darts = _check_fill(wtp, ctx, name, dtype, batch)
        assert n_darts == n


# ---- 3. round groups ----------------------------------------------------------------------------------------------------------
def test_sampler_batch_of_more_than_one_group_of_rounds(wtp, ctx):
    case = S.case_of("cube_r005")
    info, n_darts = _check_sampler(wtp, ctx, "cube_r005", F32, case["batch"])
    assert info["rounds_max"] > 8 and info["n_batches"] == 2 and case["batch"] < n_darts < 2 * case["batch"]
    assert info["rounds_max"] == 10                                       # the model's, as test_surface_sampling_cases.py records it


@pytest.mark.parametrize("batch", [64, 1000, 4096])
@pytest.mark.parametrize("name,dtype", [("cube_f075", F32), ("graded_bl", F64)], ids=_ids([("cube_f075", F32), ("graded_bl", F64)]))
def test_sampler_rounds_and_batches_equal_the_models(wtp, ctx, name, dtype, batch):
    _check_sampler(wtp, ctx, name, dtype, batch)


FILL_ROUNDS = [("cube_stall200", F32), ("cube_seeds", F64), ("cube_bl", F32), ("cavity", F32)]


@pytest.mark.parametrize("batch", [64, 1000, 4096])
@pytest.mark.parametrize("name,dtype", FILL_ROUNDS, ids=_ids(FILL_ROUNDS))
def test_fill_rounds_and_batches_equal_the_models(wtp, ctx, name, dtype, batch):
    _check_fill(wtp, ctx, name, dtype, batch)


FRONT_ROUNDS = [("grid8", F32), ("grid12_bl", F32), ("grid12_bl", F64), ("centre", F64)]


@pytest.mark.parametrize("name,dtype", FRONT_ROUNDS, ids=_ids(FRONT_ROUNDS))
def test_front_rounds_and_batches_equal_the_models(wtp, ctx, name, dtype):
    """Fc.batched over the library's own candidates; grid12_bl with every parent available needs 9 rounds, two groups."""
    case = Fc.CASES[name]
    v, t = Fc.mesh_of(name, dtype)
    ctx.mesh_set(v, t)
    sp = wtp.sampling._sampler_spacing(Fc.library_spacing(wtp, name, dtype))
    seeds, n = Fc.seeds_of(name, dtype), case["n"]
    src = ref = None
    for batch in (0, 1, 7):
        info = ctx.mesh_front(sp, n, seeds, Fc.max_points_of(case), Fc.SEED, batch)
        got = ctx.mesh_front_get(info["n_points"])
        if src is None:   # the candidates of every parent the run expands, read out once
            queue = np.concatenate([seeds, got["xyz"]])
            xyz, inside, r = ctx.mesh_front_candidates(sp, Fc.SEED, queue[:info["n_parents"]], 0, n)
            src = Fc.array_source(xyz, inside, r, n)
            ref = Fc.serial(seeds, n, Fc.max_points_of(case), src)
        b = Fc.batched(seeds, n, Fc.max_points_of(case), src, batch)
        print(f"{name} {np.dtype(dtype).name} batch={batch}: n_points={info['n_points']} batches={info['n_batches']} "
              f"rounds_max={info['rounds_max']} (model: {b['n_batches']} batches, {b['rounds_max']} rounds)")
        assert np.array_equal(b["cand"], ref["cand"]) and np.array_equal(got["cand"], ref["cand"])
        assert all(info[k] == ref[k] for k in ("n_parents", "n_candidates", "n_inside", "stop_reason"))
        assert (info["rounds_max"], info["n_batches"]) == (b["rounds_max"], b["n_batches"])
        if name == "grid12_bl" and batch == 0:
            assert info["rounds_max"] > 8


# ---- 4. degenerate cell maps ------------------------------------------------------------------------------------------------
CELL_MAPS = [(name, dt) for name in ("plate", "plate_far", "cube_stretched") for dt in S.case_dtypes(name)]


@pytest.mark.parametrize("batch", [0, 65])
@pytest.mark.parametrize("name,dtype", CELL_MAPS, ids=_ids(CELL_MAPS))
def test_sampler_on_degenerate_cell_maps(wtp, ctx, name, dtype, batch):
    """plate, plate_far: one layer of cells (nc[2] = 1), and far from the origin darts that round out of the box.
    cube_stretched: the box's 1e-6 floor, 0.3, is the cell edge, above r = 0.1125.  At batch = 65 a ball can touch more
    cells than the table has points, which makes for_near scan the points instead."""
    info, n_darts = _check_sampler(wtp, ctx, name, dtype, batch)
    assert info["stop_reason"] == 1 and info["n_points"] == (299 if name == "cube_stretched" else 469)
