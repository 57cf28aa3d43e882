"""Host check of the cell table of test_gpu_radius_routes.py, with the oracle alone: the probe rows have their designed
lengths, the tie cells hold hits at exactly d2 == r * r, the stars are isolated, the 28 / 32 cells fall on their side of
the rad_wave_only flag, the witness cells keep inside their caps, and every threshold and stage of the dispatch is named
by a cell on each side."""
import numpy as np
import pytest

import test_gpu_radius_routes as R
from test_gpu_radius_routes import CELLS, F32, F64, H, RI, STAGES, STAR_M, make_cell


def _cells(pred):
    return [c for c in CELLS if pred(c)]


def _star_cells():
    seen, out = set(), []
    for label, dt, data, env, scale, stage_of, witness in CELLS:
        if stage_of is not None and (dt, data, scale) not in seen:
            seen.add((dt, data, scale))
            out.append(pytest.param(dt, data, scale, id=label))
    return out


@pytest.mark.parametrize("dtype,data,scale", _star_cells())
def test_probe_rows_have_their_designed_length_and_are_isolated(O, dtype, data, scale):
    x, r, probes = make_cell(dtype, data, scale)
    off, idx = O.radius(x, r, "kdtree")
    lengths = np.diff(off)
    off3, _ = O.radius(x, 3.0 * r, "kdtree")
    rT = dtype(r)
    for m, i in probes.items():
        assert lengths[i] == m, f"star of {m}: row of {lengths[i]}"
        row = idx[off[i]:off[i + 1]]
        assert set(row) == set(range(i + 1, i + 1 + m)), "the row is the star's own satellites"
        # nothing but the star within 3 r of its centre: every member is more than 2 r from the background
        assert off3[i + 1] - off3[i] == m, f"star of {m}: {off3[i + 1] - off3[i] - m} background points within 3 r"
        on_rim_designed = "ties" in data or data == "wave-only-stars"
        d2 = ((x[row] - x[i]) ** 2).sum(1, dtype=dtype)
        assert d2.dtype == dtype and (d2 <= rT * rT).all()
        assert (np.diff(d2) >= 0).all() and (np.diff(d2) == 0).any(), "ascending d2 with exact ties (mirror images)"
        assert (d2 == 0).sum() == 2 and list(row[:2]) == [i + 1 + (6 if on_rim_designed else 0), i + 2 + (6 if on_rim_designed else 0)], \
            "two satellites on the centre lead the row, ranked by index"
        assert len(np.unique(x[row], axis=0)) < m - 1, "and coincident copies at d2 > 0"
        on_rim = int((d2 == rT * rT).sum())
        assert on_rim == (6 if "ties" in data or data == "wave-only-stars" else 0), f"{on_rim} hits at d2 == r * r"
    # the background of a star cell has empty rows (jittered lattices), except the uniform wave-only cell
    if data != "wave-only-stars":
        inside = np.zeros(len(x), bool)
        for m, i in probes.items():
            inside[i:i + 1 + m] = True
        assert lengths[~inside].max() == 0


def test_star_sets_cover_every_row_length_edge():
    assert STAR_M == (16, 17, 32, 33, 64, 65, 128, 129, 512, 513)
    assert (R.SHELL_MIN, R.BRICK_ROW, R.TWO_PER_LANE, R.RD_CAP, R.RAD_CAP) == (16, 32, 64, 128, 512)
    for m in STAR_M:                                          # with and without rim ties, a coincident pair in both
        for ties in (False, True):
            o = R.star_offsets(m, ties, 5)
            d2 = (o * o).sum(1)
            assert len(o) == m and (d2 <= RI * RI).all() and int((d2 == 0).sum()) == 2
            assert int((d2 == RI * RI).sum()) == (6 if ties else 0)
            assert len(np.unique(o, axis=0)) < m - 1
    assert np.float32(RI * H) * np.float32(RI * H) == (RI * H) ** 2  # r * r exact in both types


@pytest.mark.parametrize("data", ["lattice24 r=2", "lattice24 r=3", "lattice24 r=sqrt5", "lattice24 r=2.5", "lattice70 r=5"])
@pytest.mark.parametrize("dtype", [F32, F64])
def test_lattice_cells_hold_rim_hits_in_long_rows(O, dtype, data):
    x, r, _ = make_cell(dtype, data, 0)
    off, idx = O.radius(x, r, "kdtree")
    i = int(np.argmax(np.diff(off)))
    row = idx[off[i]:off[i + 1]]
    d2 = ((x[row] - x[i]) ** 2).sum(1, dtype=dtype)
    rim = int((d2 == dtype(r) * dtype(r)).sum())
    assert R.SHELL_MIN < len(row) <= R.RD_CAP, "a row the dense kernel groups into shells"
    if data in ("lattice24 r=2", "lattice24 r=3", "lattice70 r=5"):
        assert rim > 0, "a whole shell at d2 == r * r"
    else:
        assert rim == 0 and dtype(r) * dtype(r) >= (5 if "sqrt5" in data else 6.25)
    if "sqrt5" in data:
        assert (d2 == 5).any(), "the (2, 1, 0) shell lies inside the ball"


def test_wave_only_cells_fall_on_their_side_of_the_flag():
    for data, side in (("expect28", 0), ("expect32", 1), ("rows12", 0), ("wave-only-stars", 1), ("stars", 0),
                       ("zone-stars", 0), ("two-zones", 0)):
        x, r, _ = make_cell(F32, data, 0)
        e = R.expected_row(x, r)
        assert (e > R.WAVE_ONLY) == bool(side), f"{data}: expected row {e}"
    assert 27 < R.expected_row(*make_cell(F32, "expect28", 0)[:2]) < 29
    assert 31 < R.expected_row(*make_cell(F32, "expect32", 0)[:2]) < 33


def test_witness_cells_keep_inside_their_caps(O):
    done = set()
    for label, dt, data, env, scale, stage_of, witness in CELLS:
        if witness not in ("mark1", "mark2") or (dt, data) in done:
            continue
        done.add((dt, data))
        x, r, _ = make_cell(dt, data, 0)
        lengths = np.diff(O.radius(x, r, "kdtree")[0])
        cap = R.BRICK_ROW if witness == "mark1" else R.RD_CAP
        assert (lengths > cap).sum() < 0.1 * len(x), f"{label}: {(lengths > cap).sum()} rows beyond {cap}"
        if witness == "mark2":                                # and the arena holds them: whole pieces per wave (islands)
            assert lengths.sum() <= R.ARENA_PER_POINT * len(x)


def test_every_threshold_has_both_sides_and_every_stage_a_cell():
    def has(**want):
        return any(all(c[k] == v for k, v in want.items()) for c in
                   [dict(dtype=dt, data=data.replace("-ties", ""), env=tuple(env), witness=w, probes=so is not None)
                    for _, dt, data, env, _, so, w in CELLS])

    # row lengths 32 | 33 (brick kernel), 16 | 17, 64 | 65, 128 | 129 (dense kernel, fp32 and fp64), 512 | 513 (wave | serial)
    assert has(dtype=F32, data="stars", probes=True) and has(dtype=F32, data="zone-stars", probes=True)
    assert has(dtype=F64, data="stars", probes=True)
    assert has(dtype=F32, data="wave-only-stars", env=("WTP_RADIUS_DENSE",), probes=True)
    # every stage is the expected stage of some cell's probe, and every row-length edge has both sides in one cell:
    # the stage changes at 32 | 33 (brick kernel), 128 | 129 (dense kernel) and 512 | 513
    # (wave | serial), and stays the dense kernel's at its shell switches 16 | 17 and 64 | 65
    stages, changes, dense_pairs = set(), set(), set()
    for _, dt, data, env, _, stage_of, _ in CELLS:
        if stage_of is None:
            continue
        ms, n = R.probe_ms(data), len(make_cell(dt, data, 0)[0])
        stages |= {stage_of(m, n) for m in ms}
        for lo, hi in ((16, 17), (32, 33), (64, 65), (128, 129), (512, 513)):
            if lo in ms and hi in ms:
                a, b = stage_of(lo, n), stage_of(hi, n)
                if a != b:
                    changes.add((lo, hi, a, b))
                elif a == "dense":
                    dense_pairs.add((lo, hi, np.dtype(dt).name))
    assert stages == STAGES
    assert {(32, 33, "brick", "wave-fill"), (128, 129, "dense", "wave-fill"),
            (512, 513, "wave-fill", "serial")} <= changes
    assert {(lo, hi, t) for lo, hi in ((16, 17), (64, 65)) for t in ("float32", "float64")} <= dense_pairs
    assert has(dtype=F64, witness="share") and has(dtype=F32, witness="share") and has(dtype=F64, witness="shares")
    n_sh = len(make_cell(F64, "shares", 0)[0])
    assert R.wave_stride(n_sh) < n_sh <= 80000 and R.wave_share(n_sh) == 52
    # halo edges 1600 / rd_hcap, the flag at 30, the arena
    assert has(dtype=F32, data="two-zones") and has(dtype=F64, data="two-zones")
    assert has(witness="flag0") and has(witness="flag1")
    assert has(dtype=F64, witness="arena-under") and has(dtype=F64, witness="arena-over") and has(dtype=F32, witness="mark2") and has(dtype=F64, witness="mark2")
    assert (R.rd_hcap(F32), R.rd_hcap(F64)) == (3904, 1728)
    for dt in (F32, F64):                                     # stress data and degenerate sizes in both types
        for data in ("coincident", "coincident r=0", "cluster", "outlier", "whole cloud n=600", "n=33"):
            assert has(dtype=dt, data=data), (dt, data)
    assert has(data="n=1") and has(data="n=2")
    ids = [c[0] for c in CELLS]
    assert len(ids) == len(set(ids))
    assert max(len(make_cell(dt, data, 0)[0]) for _, dt, data, *_ in CELLS if data != "shares") <= 60000


def test_stage_and_share_rules():
    assert R.radius_stage(1, 5, True) == "brick" and R.radius_stage(2, 5, True) == "dense"
    assert R.radius_stage(2, 5, False) == "wave-arena"
    assert R.radius_stage(0, 512, True) == "wave-fill" and R.radius_stage(0, 513, False) == "serial"
    assert R.wave_share(40000) == 48 and R.wave_share(600) == 48 * 600 // 600 and R.wave_share(1) == 0
    assert R.wave_stride(60000) == 60000 and R.wave_stride(72176) == 65536 and R.wave_share(21193) == 47
