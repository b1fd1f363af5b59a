"""Per-node sums, counts and cells of the history planes on a regular coarse
grid reduced on the device (k_coarse_series, k_coarse_fold, k_coarse_cells;
tfg_coarse_series), through GlacierEngine.coarse_series and coarse.coarse_run:
integer planes that add exactly in any order, real planes within the bound of
m fp64 additions, the key against the engine's own nearest-neighbour forcing
(the adjoint), slot independence and the ring, repeatability, host and device
outputs, NaN containment, the threshold, shards that share a node row, split
launches, the errors of the interface, and the per-node series of a run
against the numpy oracle.

Layouts (source grid over model grid; every figure is asserted on the CPU with
tests/coarse_ref.py in check_coarse_preconditions before any GPU value is read):

  layout  model grid    gny x gnx  y0, x0      sy, sx              cells/node    empty   rows/node  cols/node
  A       37 x 100      5 x 7      0, 0        4/36, 6/99          45-153        0       5-9        9-17
  B       37 x 100      19 x 51    18, 0       -0.5, 0.5           1-4           0       1-2        1-2
  C       37 x 100      3 x 4      -2.3, -1.7  0.2, 0.05           80-792        0       5-18       16-44
  D       37 x 100      80 x 210   0, 0        2.1, 2.1            0-1           13100   0-1        0-1
  E       37 x 100      1 x 1      0.3, -5     0.01, 3             3700          0       37         100
  L       1152 x 2048   9 x 17     0, 0        8/1151, 16/2047     4608-18432    0       72-144     64-128
  M       1152 x 2048   300 x 500  0, 0        299/1151, 499/2047  6-20          0       2-4        3-5

37 x 100 is tests/test_gpu_diagnostics.py's grid: nx is no multiple of a
wave's 256 (fp32) or 128 (fp64) columns, so the only tile is ragged.  A is a
source coarser than the model; B a reversed row axis with a tie at every odd
column; C a source smaller than the model, with many cells clamped onto its
edge nodes; D a source finer than the model; E one node; L long row runs that
are cut into segments (and, 2048 columns, two tiles in fp32 and four in fp64);
M many nodes.  Beyond the table, the exact test also runs the paths the table
does not reach: S1 (37 x 101: an odd nx, scalar loads in both engines), S2
(37 x 102: scalar loads in fp32, 16-byte loads in fp64), W (5 x 1300: a full
tile and a ragged one whose second wave is ragged), W1 (5 x 1301, the same with
scalar loads) and E1 (one node over 1152 x 2048: 576 partials per entry, the
fold with 256 threads per entry; L folds with 16, the others with one).

References.  tests/coarse_ref.py: the key rule from tests/regrid_ref.axis and
math.fsum binning, so the summation error is the kernels' alone.
  integer planes  |v| <= 1024 and at most 2 359 296 cells per node: every
                  partial sum is an integer below 2^53, so any order of fp64
                  additions is exact: sums, counts and cells are asserted equal.
  real planes     per entry |got - fsum| <= m 2^-52 sum |v| over the node's m
                  cells: the textbook bound (m - 1) u sum |v| (1 + O(m u)), u =
                  2^-53, for any order of m fp64 additions, with a factor 2 to
                  spare.  Nothing is fitted; the largest observed ratio to the
                  bound is recorded (MEASURED).
  coarse_run      the numpy oracle's per-cell outputs binned the same way:
                  fp32 forms within 1e-5, the fp64 engine within 1e-12, of the
                  array's largest entry (floored form).
"""

import contextlib
import ctypes
import functools

import numpy as np
import pytest

from tests.coarse_ref import coarse_abs_sum, coarse_cells, coarse_count, coarse_fsum, coarse_key, coarse_keys
from tests.harness import BASE_CFG, make_engine
from tests.test_gpu_catchment_series import check_series_preconditions, history_engine
from tests.test_gpu_diagnostics import FUSE, NSTEPS, NX, NY, SEED, _oracle, _report, floored_err

pytestmark = pytest.mark.gpu

# Measured on an MI355X: the largest ratio of a sum's error to its bound
# m 2^-52 sum |v| (real planes, shards), and the largest floored error of
# coarse_run's sums against the oracle (bounds: 1e-5 fp32 forms, 1e-12 fp64).
MEASURED = {
    "planes_ratio": {"fp32": 1.5e-3, "fp64": 2.3e-2},  # fp32 values mostly add exactly in fp64
    "shards_ratio": {"A": 0.0, "L": 1.1e-4},
    "run_floored": {"fp32": {"SM": 3.7e-8, "IM": 6.6e-8, "M_total": 4.2e-8, "h_snow": 5.5e-9},
                    "fp32_flux64": {"SM": 2.0e-8, "IM": 3.6e-8, "M_total": 3.0e-8, "h_snow": 4.2e-9},
                    "fp64": {"SM": 2.4e-16, "IM": 1.7e-16, "M_total": 3.2e-16, "h_snow": 1.3e-16}},
}

FIELDS = ("h_snow", "SM", "h_ice", "IM", "M_total", "RH")
DEPTH = 24
REPORT: dict = {}

# name: (ny, nx, gny, gnx, y0, x0, sy, sx)
LAYOUTS = {
    "A": (NY, NX, 5, 7, 0.0, 0.0, 4 / 36, 6 / 99),
    "B": (NY, NX, 19, 51, 18.0, 0.0, -0.5, 0.5),
    "C": (NY, NX, 3, 4, -2.3, -1.7, 0.2, 0.05),
    "D": (NY, NX, 80, 210, 0.0, 0.0, 2.1, 2.1),
    "E": (NY, NX, 1, 1, 0.3, -5.0, 0.01, 3.0),
    "L": (1152, 2048, 9, 17, 0.0, 0.0, 8 / 1151, 16 / 2047),
    "M": (1152, 2048, 300, 500, 0.0, 0.0, 299 / 1151, 499 / 2047),
    # the kernel's other paths (module docstring)
    "S1": (NY, 101, 5, 7, 0.0, 0.0, 4 / 36, 6 / 100),
    "S2": (NY, 102, 5, 7, 0.0, 0.0, 4 / 36, 6 / 101),
    "W": (5, 1300, 2, 9, 0.0, 0.0, 1 / 4, 8 / 1299),
    "W1": (5, 1301, 2, 9, 0.0, 0.0, 1 / 4, 8 / 1300),
    "E1": (1152, 2048, 1, 1, 0.0, 0.0, 0.0, 0.0),
}
# cells per node (min, max), empty nodes, rows per node (min, max), columns per node (min, max)
PROMISED = {
    "A": ((45, 153), 0, (5, 9), (9, 17)),
    "B": ((1, 4), 0, (1, 2), (1, 2)),
    "C": ((80, 792), 0, (5, 18), (16, 44)),
    "D": ((0, 1), 13100, (0, 1), (0, 1)),
    "E": ((3700, 3700), 0, (37, 37), (100, 100)),
    "L": ((4608, 18432), 0, (72, 144), (64, 128)),
    "M": ((6, 20), 0, (2, 4), (3, 5)),
}


def _note(kind, key, value):
    REPORT.setdefault(kind, {})[key] = value
    _report("coarse_series", REPORT)


def shape_of(lay):
    return LAYOUTS[lay][:2]


def grid_of(lay, method="nearest"):
    from topoflow_glacier.forcing import ForcingGrid

    _, _, gny, gnx, y0, x0, sy, sx = LAYOUTS[lay]
    return ForcingGrid(gny=gny, gnx=gnx, y0=y0, x0=x0, sy=sy, sx=sx, method=method)


@functools.lru_cache(maxsize=None)
def check_coarse_preconditions():
    """What the layouts promise (module docstring), on the CPU alone."""
    for lay, (cells_mm, empty, rows_mm, cols_mm) in PROMISED.items():
        ny, nx = shape_of(lay)
        g = grid_of(lay)
        J, I = coarse_keys(g, ny, nx)
        rows, cols = np.bincount(J, minlength=g.gny), np.bincount(I, minlength=g.gnx)
        cells = coarse_cells(g, ny, nx)
        assert np.array_equal(cells, np.outer(rows, cols)) and int(cells.sum()) == ny * nx, lay
        assert (int(cells.min()), int(cells.max())) == cells_mm, (lay, cells.min(), cells.max())
        assert int((cells == 0).sum()) == empty, (lay, int((cells == 0).sum()))
        assert (int(rows.min()), int(rows.max())) == rows_mm and (int(cols.min()), int(cols.max())) == cols_mm, lay
        assert (np.diff(J) * np.sign(g.sy) >= 0).all() and (np.diff(I) >= 0).all(), lay  # monotone: a node owns a rectangle
    J, I = coarse_keys(grid_of("B"), NY, NX)
    assert I[:6].tolist() == [0, 1, 1, 2, 2, 3] and J[:6].tolist() == [18, 18, 17, 17, 16, 16]  # ties go up, rows reversed
    assert grid_of("D").gny * grid_of("D").gnx == 16800
    J, _ = coarse_keys(grid_of("L"), 1152, 2048)
    assert J[499] == J[500] == 3  # node row 3 straddles a cut at row 500
    J, _ = coarse_keys(grid_of("A"), NY, NX)
    assert J[12] == J[13] == 1    # node row 1 straddles a cut at row 13
    assert 18432 * 1024 < 2 ** 53 and 1152 * 2048 * 1024 < 2 ** 53  # integer planes add exactly in any order
    return True


@contextlib.contextmanager
def ring_engine(ny, nx, engine, depth, row0=0):
    """An engine whose history the test writes itself (set_field(name, plane, index=slot))."""
    e = make_engine(BASE_CFG, ny, nx, engine, n_frames=1, hist_depth=depth, row0=row0, split="off")
    try:
        yield e
    finally:
        e.close()


@functools.lru_cache(maxsize=8)
def int_planes(n, depth, seed):
    """[depth][n] float32 integer-valued planes, |v| <= 1024, drawn per slot from a seeded generator."""
    p = np.stack([np.random.default_rng([seed, s]).integers(-1024, 1025, size=n) for s in range(depth)]).astype(np.float32)
    p.setflags(write=False)
    return p


def plant(e, name, planes, rows=None):
    """Write planes [slots][cells] (the rows `rows` of them, for a shard) into the field's history slots."""
    for s, p in enumerate(planes):
        e.set_field(name, p if rows is None else p.reshape(-1, e.nx)[rows[0]:rows[1]].reshape(-1), index=s)


def bin_exact(g, ny, nx, planes, row0=0):
    """[slots][gny][gnx] sums of integer-valued planes by np.bincount (exact below 2^53)."""
    key = coarse_key(g, ny, nx, row0)
    nodes = g.gny * g.gnx
    return np.stack([np.bincount(key, weights=np.asarray(p, dtype=np.float64), minlength=nodes) for p in planes]).reshape(
        len(planes), g.gny, g.gnx)


def counts_of(g, ny, nx, planes, thr, row0=0):
    return np.stack([coarse_count(g, ny, nx, p, thr, row0) for p in planes])


def read_planes(e, name, slots):
    return [e.get_field(name, index=int(s), dtype=e.np_dtype) for s in slots]


def bound_ratio(got, planes, g, ny, nx, row0=0):
    """The largest |got - fsum| / (m 2^-52 sum |v|) over the entries of got
    [slots][gny][gnx] against the planes it read; an entry whose bound is 0
    (no cells, or all zeros) must be met exactly."""
    m = coarse_cells(g, ny, nx, row0).astype(np.float64)
    worst = 0.0
    for s, p in enumerate(planes):
        want = coarse_fsum(g, ny, nx, p, row0)
        bound = m * 2.0 ** -52 * coarse_abs_sum(g, ny, nx, p, row0)
        err = np.abs(got[s] - want)
        assert np.all(err[bound == 0] == 0.0)
        if (bound > 0).any():
            worst = max(worst, float(np.max(err[bound > 0] / bound[bound > 0])))
    return worst


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ 1. integer planes: exact
@pytest.mark.parametrize("lay", list(LAYOUTS))
@pytest.mark.parametrize("engine", ["float32", "float64"])
def test_integer_planes_sum_exactly(engine, lay):
    """Integer-valued planes written into the history ("SM", "M_total", "RH",
    three slots each, drawn per slot): sum equals the numpy binning, count
    (threshold 100: the value itself is present and not counted) and cells are
    equal, in every layout and both engines."""
    check_coarse_preconditions()
    ny, nx = shape_of(lay)
    g = grid_of(lay)
    depth = 3
    with ring_engine(ny, nx, engine, depth) as e:
        for i, name in enumerate(("SM", "M_total", "RH")):
            planes = int_planes(ny * nx, depth, 100 + i)
            assert (planes == 100.0).any() and (planes > 100.0).any()
            plant(e, name, planes)
            got = e.coarse_series(name, g, first=0, count=depth, threshold=100.0)
            assert got["sum"].shape == (depth, g.gny, g.gnx) and got["sum"].dtype == np.float64
            assert got["count"].dtype == np.int64 and got["cells"].dtype == np.int64
            want = bin_exact(g, ny, nx, planes)
            assert (want != 0).any()
            np.testing.assert_array_equal(got["sum"], want, err_msg=f"{lay} {name}")
            np.testing.assert_array_equal(got["count"], counts_of(g, ny, nx, planes, 100.0), err_msg=f"{lay} {name}")
            np.testing.assert_array_equal(got["cells"], coarse_cells(g, ny, nx), err_msg=f"{lay} {name}")
            assert np.all(got["sum"][:, got["cells"] == 0] == 0.0) and np.all(got["count"][:, got["cells"] == 0] == 0)


# ------------------------------------------------------------------ 2. real planes
@pytest.mark.parametrize("form", ["fp32", "fp64"])
def test_real_planes_within_the_bound_of_m_additions(form):
    """test_gpu_diagnostics' 20-step workload: the six fields over all 20
    slots under A, C and E against coarse_ref on the planes read back, per
    entry within m 2^-52 sum |v|; counts (threshold 0) and cells equal."""
    check_coarse_preconditions()
    check_series_preconditions()
    ratio = {}
    with history_engine(_oracle(NY, NX, SEED, NSTEPS), form, None, 1, DEPTH) as e:
        e.run(NSTEPS)
        planes = {name: read_planes(e, name, range(NSTEPS)) for name in FIELDS}
        for lay in ("A", "C", "E"):
            g = grid_of(lay)
            for name in FIELDS:
                got = e.coarse_series(name, g, first=0, count=NSTEPS)
                assert (got["sum"] > 0).any(), (lay, name)  # not a comparison of zeros
                ratio[f"{lay}/{name}"] = bound_ratio(got["sum"], planes[name], g, NY, NX)
                np.testing.assert_array_equal(got["count"], counts_of(g, NY, NX, planes[name], 0.0))
                np.testing.assert_array_equal(got["cells"], coarse_cells(g, NY, NX))
    _note("planes_ratio", form, max(ratio.values()))
    print(f"coarse series vs planes {form}: largest error / bound {max(ratio.values()):.3g}")
    assert max(ratio.values()) <= 1.0, ratio


# ------------------------------------------------------------------ 3. the adjoint of nearest-neighbour forcing
@pytest.mark.parametrize("lay", ["A", "B", "C", "D"])
@pytest.mark.parametrize("engine", ["float32", "float64"])
def test_cells_are_the_cells_that_receive_the_nodes_forcing(engine, lay):
    """set_gridded_forcing("nearest") of a source whose T_air holds the node
    index j gnx + i (at most 16 799: exact in fp32): the histogram of the frame
    read back is coarse_series's cells under the same grid -- the key is the
    engine's own forcing key, not only the restatement's."""
    check_coarse_preconditions()
    g = grid_of(lay, "nearest")
    nodes = g.gny * g.gnx
    src = np.zeros((1, 5, g.gny, g.gnx))
    src[0, 3] = np.arange(nodes, dtype=np.float64).reshape(g.gny, g.gnx)  # tfg_set_inputs order: P_air, Hum_sp, P, T_air, uz
    with ring_engine(NY, NX, engine, 1) as e:
        e.set_gridded_forcing(src, g)
        frame = e.get_field("T_air", index=0)
        assert np.array_equal(frame, np.round(frame)) and frame.min() >= 0 and frame.max() < nodes
        received = np.bincount(frame.astype(np.int64), minlength=nodes).reshape(g.gny, g.gnx)
        cells = e.coarse_series("M_total", grid_of(lay, "bilinear"), first=0, count=1, want=("cells",))["cells"]  # the method is not read
    np.testing.assert_array_equal(cells, received)
    np.testing.assert_array_equal(cells, coarse_cells(g, NY, NX))
    assert int(cells.sum()) == NY * NX


# ------------------------------------------------------------------ 4. slot independence, the ring, repeatability, outputs
@pytest.mark.parametrize("form", ["fp32", "fp64"])
def test_a_slots_entries_do_not_depend_on_their_company(form):
    """hist_depth 8, 20 steps: a call over the 7 slots 5 .. 5+6 (it wraps to
    slots 0..3) equals the single-slot calls bit for bit, under A, C and E;
    the defaults are the last 8 steps in order; leaving outputs out changes
    nothing."""
    check_coarse_preconditions()
    with history_engine(_oracle(NY, NX, SEED, NSTEPS), form, None, 1, 8) as e:
        e.run(NSTEPS)
        for lay in ("A", "C", "E"):
            g = grid_of(lay)
            whole = e.coarse_series("M_total", g, first=5, count=7, threshold=1e-9)
            assert (whole["sum"] > 0).any() and 0 < whole["count"].sum() and not same_bits(whole["sum"][0], whole["sum"][6])
            for j in range(7):
                one = e.coarse_series("M_total", g, first=(5 + j) % 8, count=1, threshold=1e-9)
                assert one["sum"].shape == (1, g.gny, g.gnx)
                assert same_bits(one["sum"][0], whole["sum"][j]) and same_bits(one["count"][0], whole["count"][j]), (lay, j)
                assert same_bits(one["cells"], whole["cells"])
            other = e.coarse_series("M_total", g, first=7, count=5, threshold=1e-9)  # rows 2..6 of `whole`, batched otherwise
            assert same_bits(other["sum"], whole["sum"][2:7]) and same_bits(other["count"], whole["count"][2:7])
            only = e.coarse_series("M_total", g, first=5, count=7, want="sum")
            assert list(only) == ["sum"] and same_bits(only["sum"], whole["sum"])
            planes = read_planes(e, "M_total", [(5 + j) % 8 for j in range(7)])
            assert bound_ratio(whole["sum"], planes, g, NY, NX) <= 1.0
        dflt = e.coarse_series("M_total", grid_of("A"))
        last8 = e.coarse_series("M_total", grid_of("A"), first=NSTEPS % 8, count=8)
        assert all(same_bits(dflt[k], last8[k]) for k in dflt)


@pytest.mark.parametrize("form", ["fp32", "fp64"])
def test_a_short_last_batch_repeats_and_device_outputs(form):
    """hist_depth 24, 11 slots from slot 3: a batch of 8 and a short one of 3.
    The rows equal the single-slot calls bit for bit; two identical calls give
    equal bits; device outputs hold the host result bit for bit."""
    import torch

    check_coarse_preconditions()
    with history_engine(_oracle(NY, NX, SEED, NSTEPS), form, None, 1, DEPTH) as e:
        e.run(NSTEPS)
        for lay in ("A", "B"):
            g = grid_of(lay)
            a = e.coarse_series("SM", g, first=3, count=11, threshold=1e-9)
            b = e.coarse_series("SM", g, first=3, count=11, threshold=1e-9)
            assert (a["sum"] > 0).any() and 0 < a["count"].sum()
            assert all(same_bits(a[k], b[k]) for k in ("sum", "count", "cells")), lay
            for j in (0, 7, 8, 10):  # both batches, first and last position
                one = e.coarse_series("SM", g, first=3 + j, count=1, threshold=1e-9)
                assert same_bits(one["sum"][0], a["sum"][j]) and same_bits(one["count"][0], a["count"][j]), (lay, j)
            dev = "cuda:0"
            out = {"sum": torch.full((11, g.gny, g.gnx), -1.0, dtype=torch.float64, device=dev),
                   "count": torch.full((11, g.gny, g.gnx), -1, dtype=torch.int64, device=dev),
                   "cells": torch.full((g.gny, g.gnx), -1, dtype=torch.int64, device=dev)}
            assert e.coarse_series("SM", g, first=3, count=11, threshold=1e-9, out=out) is out
            e.sync()
            for k in out:
                assert out[k].cpu().numpy().tobytes() == a[k].tobytes(), (lay, k)
            part = {"count": torch.full((11, g.gny, g.gnx), -1, dtype=torch.int64, device=dev)}
            e.coarse_series("SM", g, first=3, count=11, threshold=1e-9, out=part)
            e.sync()
            assert np.array_equal(part["count"].cpu().numpy(), a["count"])
        g = grid_of("A")
        for bad in ({"sum": out["sum"].float()}, {"sum": out["sum"]}, {"count": out["sum"]}, {"sum": out["sum"].cpu()},
                    {"mean": out["sum"]}, {}):  # out belongs to B: the wrong size for A
            with pytest.raises(ValueError):
                e.coarse_series("SM", g, first=3, count=11, out=bad)


# ------------------------------------------------------------------ 5. NaN containment
@pytest.mark.parametrize("lay", ["A", "M"])
@pytest.mark.parametrize("engine", ["float32", "float64"])
def test_nan_stays_in_its_slot_and_node(engine, lay):
    """One NaN cell in slot 2: exactly one sum entry is NaN, in slot 2 at the
    cell's node; count there (threshold -inf) excludes the cell; every other
    entry of every slot has the bits of the run without the NaN."""
    check_coarse_preconditions()
    ny, nx = shape_of(lay)
    g = grid_of(lay)
    depth = 4
    cell = (ny // 3) * nx + (2 * nx) // 3 + 1
    node = np.unravel_index(int(coarse_key(g, ny, nx)[cell]), (g.gny, g.gnx))
    planes = int_planes(ny * nx, depth, 7).copy()
    with ring_engine(ny, nx, engine, depth) as e:
        plant(e, "M_total", planes)
        clean = e.coarse_series("M_total", g, first=0, count=depth, threshold=-np.inf)
        planes[2, cell] = np.nan
        e.set_field("M_total", planes[2], index=2)
        got = e.coarse_series("M_total", g, first=0, count=depth, threshold=-np.inf)
    want_nan = np.zeros(got["sum"].shape, dtype=bool)
    want_nan[(2, *node)] = True
    np.testing.assert_array_equal(np.isnan(got["sum"]), want_nan)
    assert not np.isnan(clean["sum"]).any()
    assert got["sum"][~want_nan].tobytes() == clean["sum"][~want_nan].tobytes()
    np.testing.assert_array_equal(clean["count"], np.broadcast_to(clean["cells"], clean["count"].shape))
    np.testing.assert_array_equal(got["count"], clean["count"] - want_nan)
    assert same_bits(got["cells"], clean["cells"])


# ------------------------------------------------------------------ 6. threshold
@pytest.mark.parametrize("engine", ["float32", "float64"])
def test_the_threshold_is_strict(engine):
    """A value equal to the threshold is not counted, the next double below
    the threshold counts it; -inf counts every cell, +inf none."""
    check_coarse_preconditions()
    g = grid_of("A")
    planes = int_planes(NY * NX, 2, 9)
    v = 37.0
    same = counts_of(g, NY, NX, planes, v - 0.5) - counts_of(g, NY, NX, planes, v)  # the cells holding exactly v
    assert same.sum() >= 1
    with ring_engine(NY, NX, engine, 2) as e:
        plant(e, "h_ice", planes)
        at = e.coarse_series("h_ice", g, first=0, count=2, threshold=v, want=("count", "cells"))
        below = e.coarse_series("h_ice", g, first=0, count=2, threshold=float(np.nextafter(v, -np.inf)), want="count")
        every = e.coarse_series("h_ice", g, first=0, count=2, threshold=-np.inf, want="count")
        none = e.coarse_series("h_ice", g, first=0, count=2, threshold=np.inf, want="count")
    np.testing.assert_array_equal(at["count"], counts_of(g, NY, NX, planes, v))
    np.testing.assert_array_equal(below["count"] - at["count"], same)
    assert 0 < at["count"].sum() < 2 * at["cells"].sum()
    np.testing.assert_array_equal(every["count"], np.broadcast_to(at["cells"], (2, g.gny, g.gnx)))
    assert not none["count"].any()


# ------------------------------------------------------------------ 7. shards that share a node row
def _real_planes(lay):
    """Two real M_total planes of the layout's grid, in fp32 (the fp32 engine's own)."""
    ny, nx = shape_of(lay)
    if lay == "A":
        with history_engine(_oracle(NY, NX, SEED, NSTEPS), "fp32", None, 1, DEPTH) as e:
            e.run(NSTEPS)
            return np.stack(read_planes(e, "M_total", (9, 19)))
    from topoflow_glacier.synthetic import diurnal_table

    e = make_engine(BASE_CFG, ny, nx, "float32", n_frames=4, hist_depth=4, fuse_steps=FUSE, split="off")
    try:
        e.fill_synthetic(5, diurnal_table(4), nx_global=nx)
        e.run(4)
        return np.stack(read_planes(e, "M_total", (0, 3)))
    finally:
        e.close()


@pytest.mark.parametrize("lay,cut", [("L", 500), ("A", 13)])
def test_shards_that_share_a_node_row_add_to_the_whole(lay, cut):
    """Two handles on one GPU, cut inside a node row (L at row 500: J = 3 on
    both sides; A at row 13: J = 1).  Integer planes: whole == part0 + part1
    exactly in sum, count and cells.  Real planes (M_total of a run, planted
    into the shards): the sums agree within m 2^-52 sum |v|, counts and cells
    exactly.  A node row outside a shard reads 0 there."""
    check_coarse_preconditions()
    ny, nx = shape_of(lay)
    g = grid_of(lay)
    real = _real_planes(lay)
    assert (real > 0).any() and np.isfinite(real).all()
    ints = int_planes(ny * nx, 2, 21)
    res = {}
    for key, (r0, r1) in (("whole", (0, ny)), ("p0", (0, cut)), ("p1", (cut, ny))):
        with ring_engine(r1 - r0, nx, "float32", 2, row0=r0) as e:
            plant(e, "M_total", ints, rows=(r0, r1))
            plant(e, "SM", real, rows=(r0, r1))
            res[key] = (e.coarse_series("M_total", g, first=0, count=2, threshold=100.0),
                        e.coarse_series("SM", g, first=0, count=2, threshold=1e-9))
    whole, p0, p1 = res["whole"], res["p0"], res["p1"]
    J, _ = coarse_keys(g, ny, nx)
    assert (p0[0]["cells"][J[cut]] > 0).all() and (p1[0]["cells"][J[cut]] > 0).all()  # both hold a partial of the cut's node row
    assert (p0[0]["cells"][J[cut] + 1:] == 0).all() and (p1[0]["cells"][:J[cut]] == 0).all()
    np.testing.assert_array_equal(whole[0]["sum"], bin_exact(g, ny, nx, ints))
    for k in ("sum", "count", "cells"):
        np.testing.assert_array_equal(whole[0][k], p0[0][k] + p1[0][k], err_msg=k)
    for k in ("count", "cells"):
        np.testing.assert_array_equal(whole[1][k], p0[1][k] + p1[1][k], err_msg=k)
    m = coarse_cells(g, ny, nx).astype(np.float64)
    bound = np.stack([m * 2.0 ** -52 * coarse_abs_sum(g, ny, nx, p) for p in real])
    err = np.abs(whole[1]["sum"] - (p0[1]["sum"] + p1[1]["sum"]))
    assert (bound > 0).any() and np.all(err[bound == 0] == 0.0)
    ratio = float(np.max(err[bound > 0] / bound[bound > 0]))
    ratio = max(ratio, bound_ratio(whole[1]["sum"], real, g, ny, nx))
    _note("shards_ratio", lay, ratio)
    print(f"coarse series, shards of {lay}: largest error / bound {ratio:.3g}")
    assert ratio <= 1.0


# ------------------------------------------------------------------ 8. split launches
def test_a_split_handle_gives_the_bits_of_an_unsplit_one():
    """TFG_SPLIT_ON: coarse_series straight after run(), without join(),
    equals a TFG_SPLIT_OFF handle's after the same steps, bit for bit."""
    check_coarse_preconditions()
    orc = _oracle(NY, NX, SEED, NSTEPS)
    got = {}
    for split in ("on", "off"):
        with history_engine(orc, "fp32", None, 1, DEPTH, split=split) as e:
            assert e.is_split() == (split == "on")
            e.run(NSTEPS)
            got[split] = [e.coarse_series(name, grid_of(lay), first=0, count=NSTEPS)  # no sync(), no join()
                          for name in ("M_total", "h_snow") for lay in ("A", "C")]
    for a, b in zip(got["on"], got["off"]):
        assert (a["sum"] > 0).any()
        assert all(same_bits(a[k], b[k]) for k in ("sum", "count", "cells"))


# ------------------------------------------------------------------ 9. errors
def test_bad_arguments_write_nothing_and_leave_the_handle_usable():
    """Every TFG_ERR_ARG case of include/tfg.h, through ctypes: the outputs,
    prefilled with a sentinel, come back unchanged, and the call that follows
    gives the bits of the call before them."""
    from topoflow_glacier import _native as nat

    check_coarse_preconditions()
    L = nat.load()
    fid = nat.FIELD["M_total"]
    g = grid_of("A")
    good = dict(gny=g.gny, gnx=g.gnx, method=0, pad=0, y0=g.y0, x0=g.x0, sy=g.sy, sx=g.sx, row0=0)

    def grid(**kw):
        return ctypes.byref(nat.TfgForcingGrid(**dict(good, **kw)))

    with ring_engine(NY, NX, "float32", 8) as e:
        plant(e, "M_total", int_planes(NY * NX, 8, 3))
        before = e.coarse_series("M_total", g, first=0, count=8, threshold=100.0)
        s = np.full((8, g.gny, g.gnx), -7.0)
        c = np.full((8, g.gny, g.gnx), -7, dtype=np.int64)
        n = np.full((g.gny, g.gnx), -7, dtype=np.int64)
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        out = (ptr(s), ptr(c), ptr(n))
        cases = {
            "null grid": (fid, 0, 1, None, 0.0, *out),
            "no output": (fid, 0, 1, grid(), 0.0, None, None, None),
            "gny = 0": (fid, 0, 1, grid(gny=0), 0.0, *out),
            "gnx = 0": (fid, 0, 1, grid(gnx=0), 0.0, *out),
            "gny < 0": (fid, 0, 1, grid(gny=-3), 0.0, *out),
            "2^29 nodes": (fid, 0, 1, grid(gny=1 << 15, gnx=1 << 14), 0.0, *out),
            "nan y0": (fid, 0, 1, grid(y0=np.nan), 0.0, *out),
            "inf x0": (fid, 0, 1, grid(x0=np.inf), 0.0, *out),
            "inf sy": (fid, 0, 1, grid(sy=-np.inf), 0.0, *out),
            "nan sx": (fid, 0, 1, grid(sx=np.nan), 0.0, *out),
            "row0 < 0": (fid, 0, 1, grid(row0=-1), 0.0, *out),
            "nan threshold": (fid, 0, 1, grid(), np.nan, *out),
            "nan threshold, count alone": (fid, 0, 1, grid(), np.nan, None, ptr(c), None),
            "state field": (nat.FIELD["h_swe"], 0, 1, grid(), 0.0, *out),
            "input field": (nat.FIELD["P"], 0, 1, grid(), 0.0, *out),
            "hist0 < 0": (fid, -1, 1, grid(), 0.0, *out),
            "hist0 = depth": (fid, 8, 1, grid(), 0.0, *out),
            "no slots": (fid, 0, 0, grid(), 0.0, *out),
            "9 slots": (fid, 0, 9, grid(), 0.0, *out),
            "cells only, bad field": (nat.FIELD["P"], 0, 1, grid(), 0.0, None, None, ptr(n)),
            "cells only, 9 slots": (fid, 0, 9, grid(), 0.0, None, None, ptr(n)),
        }
        for what, (f, h0, ns, gp, thr, ps, pc, pn) in cases.items():
            assert L.tfg_coarse_series(e.h, f, h0, ns, gp, thr, ps, pc, pn, 0) == nat.ERR_ARG, what
            assert b"coarse series" in L.tfg_last_error(e.h), what
            assert (s == -7.0).all() and (c == -7).all() and (n == -7).all(), what
        assert L.tfg_coarse_series(None, fid, 0, 1, grid(), 0.0, *out, 0) == nat.ERR_ARG
        assert b"null handle" in L.tfg_last_error(None) and (s == -7.0).all()
        with pytest.raises(nat.NativeError, match="coarse series") as ei:
            e.coarse_series("M_total", g, threshold=np.nan)
        assert ei.value.code == nat.ERR_ARG
        with pytest.raises(ValueError):
            e.coarse_series("M_total", g, want=("mean",))
        # what is allowed: a NaN threshold without count; cells alone; a method of any value (it is not read)
        ok = e.coarse_series("M_total", g, first=0, count=8, threshold=np.nan, want=("sum", "cells"))
        assert same_bits(ok["sum"], before["sum"]) and same_bits(ok["cells"], before["cells"])
        assert L.tfg_coarse_series(e.h, fid, 0, 8, grid(method=77), 100.0, *out, 0) == nat.OK
        assert same_bits(s, before["sum"]) and same_bits(c, before["count"]) and same_bits(n, before["cells"])


# ------------------------------------------------------------------ 10. coarse_run against the oracle
@pytest.mark.parametrize("form", ["fp32", "fp32_flux64", "fp64"])
def test_coarse_run_against_the_oracle(form):
    """coarse_run over 20 steps on a ring of 8 (blocks of 8, 8 and 4), periods
    of 7 steps (7, 7, 6: the last is short, and the periods straddle the
    blocks), layout A: the per-node SM, IM, M_total and h_snow sums against the
    numpy oracle's per-cell outputs binned by coarse_ref; melt_depth, mean,
    fraction and cells follow from them."""
    from topoflow_glacier.coarse import coarse_run

    check_coarse_preconditions()
    out = check_series_preconditions()
    g = grid_of("A")
    blocks = []
    with history_engine(_oracle(NY, NX, SEED, NSTEPS), form, None, 1, 8) as e:
        res = coarse_run(e, NSTEPS, 7, g, ("SM", "IM", "M_total", "h_snow"), threshold={"h_snow": 0.0},
                         on_block=lambda k0, k1, block: blocks.append((k0, k1, block["M_total"]["sum"].shape)))
        assert e.step_index == NSTEPS
    assert res["periods"].tolist() == [7, 7, 6]
    assert blocks == [(0, 8, (8, g.gny, g.gnx)), (8, 16, (8, g.gny, g.gnx)), (16, 20, (4, g.gny, g.gnx))]
    cells = coarse_cells(g, NY, NX)
    np.testing.assert_array_equal(res["cells"], cells)
    err = {}
    for name in ("SM", "IM", "M_total", "h_snow"):
        want = np.stack([coarse_fsum(g, NY, NX, out[name][a:b]) for a, b in ((0, 7), (7, 14), (14, 20))])
        assert (want > 0).any(), name
        assert res["fields"][name]["sum"].shape == (3, g.gny, g.gnx)
        err[name] = floored_err(res["fields"][name]["sum"], want)
        np.testing.assert_array_equal(res["fields"][name]["mean"], res["fields"][name]["sum"] / cells)
    _note("run_floored", form, err)
    print(f"coarse run vs oracle {form}: {err}")
    assert max(err.values()) <= (1e-12 if form == "fp64" else 1e-5), err
    melt = res["fields"]["SM"]["sum"] + res["fields"]["IM"]["sum"]
    assert np.array_equal(res["melt_depth"], melt * (BASE_CFG["dt"] * 3600.0) / cells)
    frac = res["fields"]["h_snow"]["fraction"]
    assert ((frac >= 0) & (frac <= 1)).all() and (frac > 0).any()
    np.testing.assert_array_equal(frac, res["fields"]["h_snow"]["count"] / res["periods"][:, None, None] / cells)
