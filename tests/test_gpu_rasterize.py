"""tfg_rasterize_polygons / GlacierEngine.rasterize_divides on the device.

Every comparison is exact equality of the whole int32 raster with
hydrofabric.rasterize_divides' (-1 -> outside_id): the fixture's 43 divides at
200 m and 50 m, synthetic shapes (tests/raster_ref.py), row-block shards, what
reads the raster downstream, and rejected input."""

from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

from tests import raster_ref as R
from tests.harness import BASE_CFG, GOLDEN, make_engine, synthetic_inputs

pytestmark = pytest.mark.gpu

FIX = GOLDEN / "hydrofabric_12082500.npz"


@functools.lru_cache(maxsize=None)
def _fixture(cell):
    """(divides, x0, y0, ny, nx, host ids [ny][nx]) of the fixture at `cell` metres, computed once."""
    from topoflow_glacier.hydrofabric import grid_covering, load_divides_npz

    _, dv = load_divides_npz(FIX)
    x0, y0, ny, nx = grid_covering(dv, cell)
    want = R.host_ids(dv, x0, y0, cell, ny, nx, len(dv))
    want.setflags(write=False)
    return dv, x0, y0, ny, nx, want


def _device_raster(dv, x0, y0, cell, ny, nx, engine="float32", n_catch=None, **kw):
    """(raster [ny][nx], counts) from a fresh handle."""
    e = make_engine(BASE_CFG, ny, nx, engine, n_frames=1, hist_depth=1, n_catch=n_catch or len(dv) + 1)
    try:
        cells = e.rasterize_divides(dv, x0, y0, cell, **kw)
        return e.get_field("catch_id").reshape(ny, nx), cells
    finally:
        e.close()


@pytest.mark.parametrize("cell,engine", [(200.0, "float32"), (50.0, "float32"), (200.0, "float64")])
def test_fixture_raster_equals_the_host(cell, engine):
    dv, x0, y0, ny, nx, want = _fixture(cell)
    assert (ny, nx) == {200.0: (102, 159), 50.0: (396, 626)}[cell]
    got, cells = _device_raster(dv, x0, y0, cell, ny, nx, engine)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(cells, np.bincount(want.reshape(-1), minlength=len(dv) + 1))


@pytest.mark.parametrize("name", sorted(R.synthetic_cases()))
def test_synthetic_shapes_equal_the_host(name):
    """Holes, multipolygons, overlaps in both orders, vertices and edges on
    cell centres, shapes off the grid, 600 crossings in a row (more than a
    fill of the list holds), 5000 edges in a ring, and grids with n < 256,
    nx % 4 != 0 and tile and wave edges inside a row."""
    dv, ny, nx = R.synthetic_cases()[name]
    want = R.host_ids(dv, R.X0, R.Y0, 1.0, ny, nx, len(dv))
    got, cells = _device_raster(dv, R.X0, R.Y0, 1.0, ny, nx)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(cells, np.bincount(want.reshape(-1), minlength=len(dv) + 1))


@pytest.mark.parametrize("cuts", [(0, 51, 102), (0, 40, 41, 102)])
def test_row_shards_equal_the_whole_raster(cuts):
    """2 and 3 row blocks cut inside polygons, each on a handle of its own."""
    dv, x0, y0, ny, nx, want = _fixture(200.0)
    total = np.zeros(len(dv) + 1, dtype=np.int64)
    for r0, r1 in zip(cuts[:-1], cuts[1:]):
        got, cells = _device_raster(dv, x0, y0, 200.0, r1 - r0, nx, row0=r0, ny_global=ny)
        np.testing.assert_array_equal(got, want[r0:r1])
        total += cells
    np.testing.assert_array_equal(total, np.bincount(want.reshape(-1), minlength=len(dv) + 1))


def test_counts_fill_the_cache_and_a_second_call_replaces_the_raster():
    dv, x0, y0, ny, nx, want = _fixture(200.0)
    nc = len(dv) + 1
    e = make_engine(BASE_CFG, ny, nx, "float32", n_frames=1, hist_depth=1, n_catch=nc)
    try:
        cells = e.rasterize_divides(dv, x0, y0, 200.0)
        np.testing.assert_array_equal(cells, np.bincount(want.reshape(-1), minlength=nc))
        e.get_field = None  # catchment_cells() must not read the raster back
        assert e.catchment_cells() is cells
        del e.get_field
        np.testing.assert_array_equal(e.get_field("catch_id").reshape(ny, nx), want)
        # other divides (the first ten, reversed), another outside id, no counts: nothing of the first raster stays
        other = dv[9::-1]
        assert e.rasterize_divides(other, x0, y0, 200.0, outside_id=nc - 1, counts=False) is None
        want2 = R.host_ids(other, x0, y0, 200.0, ny, nx, nc - 1)
        assert (want2 != want).any()
        np.testing.assert_array_equal(e.get_field("catch_id").reshape(ny, nx), want2)
        np.testing.assert_array_equal(e.catchment_cells(), np.bincount(want2.reshape(-1), minlength=nc))
        with pytest.raises(ValueError, match="n_catch"):
            e.rasterize_divides(dv, x0, y0, 200.0, outside_id=nc)
    finally:
        e.close()


def test_a_run_is_the_same_from_either_raster():
    """n_catch = 44: diagnostics() and catchment_series rows bit for bit,
    whether the raster came from the device call or from set_field with the
    host raster."""
    dv, x0, y0, ny, nx, want = _fixture(200.0)
    nc, nsteps, seed = len(dv) + 1, 8, 5
    assert nc == 44
    _, d = synthetic_inputs(seed, ny, nx, 24)
    res = []
    for device in (True, False):
        e = make_engine(dict(BASE_CFG, da=0.04), ny, nx, "float32", n_frames=24, hist_depth=nsteps, n_catch=nc)
        try:
            e.fill_synthetic(seed, d)
            if device:
                e.rasterize_divides(dv, x0, y0, 200.0, counts=False)
            else:
                e.set_field("catch_id", want.reshape(-1))
            e.run(nsteps)
            e.sync()
            res.append((e.diagnostics(), e.catchment_series("M_total"), e.catchment_series("SM", reduce="mean")))
        finally:
            e.close()
    for a, b in zip(*res):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()
    assert (res[0][0][:, 0] > 0).any() and res[0][1].shape == (nsteps, nc)  # the run did something


def test_rejected_input_leaves_the_previous_raster():
    from topoflow_glacier import _native as nat
    from topoflow_glacier.hydrofabric import polygon_tables

    dv, ny, nx = R.synthetic_cases()["c-later-wins"]
    want = R.host_ids(dv, R.X0, R.Y0, 1.0, ny, nx, 2)
    e = make_engine(BASE_CFG, ny, nx, "float32", n_frames=1, hist_depth=1, n_catch=3)
    try:
        cells = e.rasterize_divides(dv, R.X0, R.Y0, 1.0)
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731

        def call(outside_id=2, **change):
            t = polygon_tables(dv[::-1], R.X0, R.Y0, 1.0, ny, nx)  # accepted, it would change the raster
            for k, v in change.items():
                v(getattr(t, k))
            p = nat.TfgPolygons(len(t.poly_id), ptr(t.poly_id), ptr(t.poly_ring0), ptr(t.poly_box),
                                len(t.ring_edge0) - 1, ptr(t.ring_edge0), ptr(t.edges), ptr(t.px), ptr(t.py))
            return e.lib.tfg_rasterize_polygons(e.h, ctypes.byref(p), outside_id, None)

        def at(index, value):
            def change(a):
                a[index] = value
            return change

        for kw, msg in ((dict(poly_id=at(1, 3)), b"id out of"), (dict(poly_id=at(0, -1)), b"id out of"),
                        (dict(outside_id=3), b"outside_id"), (dict(poly_box=at((0, 3), nx + 1)), b"box outside"),
                        (dict(poly_box=at((1, 0), -1)), b"box outside"), (dict(poly_box=at((1, 1), ny + 1)), b"box outside"),
                        (dict(ring_edge0=at(1, 9)), b"decreases"), (dict(poly_ring0=at(2, 4)), b"past n_rings"),
                        (dict(edges=at((2, 0), np.nan)), b"non-finite"), (dict(px=at(4, np.inf)), b"non-finite"),
                        (dict(py=at(0, np.nan)), b"non-finite"),
                        (dict(edges=lambda a: a.__setitem__((1, 3), a[1, 1])), b"horizontal")):
            assert call(**kw) == nat.ERR_ARG, kw
            assert msg in e.lib.tfg_last_error(e.h), (kw, e.lib.tfg_last_error(e.h))
            np.testing.assert_array_equal(e.get_field("catch_id").reshape(ny, nx), want)
        assert e.lib.tfg_rasterize_polygons(e.h, None, 2, None) == nat.ERR_ARG
        assert e.catchment_cells() is cells
        assert call() == nat.OK  # the unchanged tables are accepted
        assert (e.get_field("catch_id").reshape(ny, nx) != want).any()
    finally:
        e.close()
