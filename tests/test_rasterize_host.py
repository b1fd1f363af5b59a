"""The device rasteriser above the kernel, without a GPU: the C ABI's null
handle and struct layout, hydrofabric.polygon_tables, and the kernel's
algorithm restated in numpy (tests/raster_ref.py) against
hydrofabric.rasterize_divides, cell for cell."""

from __future__ import annotations

import ctypes
import subprocess

import numpy as np
import pytest

from tests import raster_ref as R
from tests.harness import GOLDEN, ROOT

FIX = GOLDEN / "hydrofabric_12082500.npz"


def _fixture(cell):
    from topoflow_glacier.hydrofabric import grid_covering, load_divides_npz

    _, dv = load_divides_npz(FIX)
    return (dv, *grid_covering(dv, cell))


def test_null_handle_is_rejected_without_a_device():
    """tfg_rasterize_polygons fails cleanly on a null handle (no HIP call is
    made), the binding lists the symbol, and the ABI is still 8."""
    from topoflow_glacier import _native as nat

    L = nat.load()
    p = nat.TfgPolygons()
    assert L.tfg_rasterize_polygons(None, ctypes.byref(p), 0, None) == nat.ERR_ARG
    assert b"null handle" in L.tfg_last_error(None)
    assert L.tfg_rasterize_polygons(None, None, 0, None) == nat.ERR_ARG
    assert "tfg_rasterize_polygons" in nat.exported_symbols()
    assert L.tfg_abi_version() == 8  # the entry point is an addition to ABI 8


def test_polygons_layout_matches_header(tmp_path):
    """tfg_polygons' size and offsets from a gcc probe against include/tfg.h,
    compared with the ctypes mirror."""
    from topoflow_glacier import _native as nat

    names = [n for n, _ in nat.TfgPolygons._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tfg.h"\nint main(void){printf("%zu", sizeof(tfg_polygons));'
                   + "".join(f'printf(" %zu", offsetof(tfg_polygons, {n}));' for n in names) + "return 0;}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(nat.TfgPolygons)] + [getattr(nat.TfgPolygons, n).offset for n in names]


@pytest.mark.parametrize("cell", [200.0, 50.0])
def test_restatement_equals_rasterize_divides_on_the_fixture(cell):
    """43 divides at 200 m (102 x 159) and 50 m (396 x 626): 0 differing cells,
    and the same with a list of 7 edges per fill (the capacity does not matter)."""
    from topoflow_glacier.hydrofabric import polygon_tables

    dv, x0, y0, ny, nx = _fixture(cell)
    assert (ny, nx) == {200.0: (102, 159), 50.0: (396, 626)}[cell]
    want = R.host_ids(dv, x0, y0, cell, ny, nx, len(dv))
    t = polygon_tables(dv, x0, y0, cell, ny, nx)
    assert t.edges.shape[1] == 4 and not (t.edges[:, 1] == t.edges[:, 3]).any()
    np.testing.assert_array_equal(R.rasterize(t, len(dv)), want)
    if cell == 200.0:
        np.testing.assert_array_equal(R.rasterize(t, len(dv), cap=7), want)


@pytest.mark.parametrize("name", sorted(R.synthetic_cases()))
def test_restatement_equals_rasterize_divides_on_synthetic_shapes(name):
    from topoflow_glacier.hydrofabric import polygon_tables

    dv, ny, nx = R.synthetic_cases()[name]
    want = R.host_ids(dv, R.X0, R.Y0, 1.0, ny, nx, len(dv))
    t = polygon_tables(dv, R.X0, R.Y0, 1.0, ny, nx)
    np.testing.assert_array_equal(R.rasterize(t, len(dv)), want)
    assert name.startswith("h-") or (want != len(dv)).any()  # the shapes do reach the grid


def test_synthetic_shapes_show_what_they_are_for():
    """The overlap rules and the comb's crossings, on the host raster itself."""
    cases = R.synthetic_cases()
    dv, ny, nx = cases["c-later-wins"]
    fwd = R.host_ids(dv, R.X0, R.Y0, 1.0, ny, nx, 2)
    assert fwd[5, 8] == 0 and fwd[5, 13] == 1 and fwd[11, 8] == 1  # in the later hole: the earlier id stays
    dv, ny, nx = cases["c-reversed"]
    rev = R.host_ids(dv, R.X0, R.Y0, 1.0, ny, nx, 2)
    assert rev[5, 8] == 1 and rev[11, 8] == 1 and rev[5, 16] == 0  # the other order: the whole of `a` wins
    dv, ny, nx = cases["f-comb"]
    from topoflow_glacier.hydrofabric import polygon_tables

    t = polygon_tables(dv, R.X0, R.Y0, 1.0, ny, nx)
    py = t.py[2]
    assert np.count_nonzero((t.edges[:, 1] > py) != (t.edges[:, 3] > py)) == 600 > 2 * R.CAP
    dv, ny, nx = cases["g-circle"]
    assert polygon_tables(dv, R.X0, R.Y0, 1.0, ny, nx).ring_edge0[-1] > 10 * R.CAP


@pytest.mark.parametrize("cuts", [(0, 51, 102), (0, 40, 41, 102)])
def test_row_shards_equal_the_whole_grid(cuts):
    """Row blocks cut inside polygons (row0): each shard's tables give the
    whole raster's rows; px does not depend on the shard and py is the whole
    grid's, bit for bit."""
    from topoflow_glacier.hydrofabric import polygon_tables

    dv, x0, y0, ny, nx = _fixture(200.0)
    want = R.host_ids(dv, x0, y0, 200.0, ny, nx, len(dv))
    whole = polygon_tables(dv, x0, y0, 200.0, ny, nx)
    for r0, r1 in zip(cuts[:-1], cuts[1:]):
        t = polygon_tables(dv, x0, y0, 200.0, ny, nx, row0=r0, rows=r1 - r0)
        assert t.px.tobytes() == whole.px.tobytes() and t.py.tobytes() == whole.py[r0:r1].tobytes()
        assert (t.poly_box[:, 0] >= 0).all() and (t.poly_box[:, 1] <= r1 - r0).all()
        assert (t.poly_box[:, 0] < t.poly_box[:, 1]).all() and len(t.poly_id) <= len(whole.poly_id)
        np.testing.assert_array_equal(R.rasterize(t, len(dv)), want[r0:r1])


def test_polygon_tables_shapes_and_rejections():
    from topoflow_glacier.hydrofabric import Divide, polygon_tables

    dv, ny, nx = R.synthetic_cases()["b-multi-and-empty"]
    t = polygon_tables(dv, R.X0, R.Y0, 1.0, ny, nx)
    assert t.poly_id.tolist() == [0, 0, 2] and t.poly_ring0.tolist() == [0, 1, 2, 3]  # divide 1 has no polygon
    assert t.ring_edge0.tolist() == [0, 2, 4, 6]  # a rectangle keeps its two vertical edges
    assert (t.poly_id.dtype, t.poly_ring0.dtype, t.poly_box.dtype, t.ring_edge0.dtype) == (np.int32, np.int32, np.int32, np.int64)
    assert t.edges.flags.c_contiguous and t.edges.dtype == np.float64 and t.px.shape == (nx,) and t.py.shape == (ny,)
    none = polygon_tables([], R.X0, R.Y0, 1.0, 3, 5)
    assert none.poly_box.shape == (0, 4) and none.edges.shape == (0, 4) and none.poly_ring0.tolist() == [0]
    np.testing.assert_array_equal(R.rasterize(none, 0), np.zeros((3, 5), dtype=np.int32))
    bad = np.array([[1.0, 1.0], [4.0, np.nan], [2.0, 5.0]])
    with pytest.raises(ValueError, match="non-finite"):
        polygon_tables([Divide("x", 0.0, [[bad]])], R.X0, R.Y0, 1.0, 8, 8)
    with pytest.raises(ValueError, match="outside the grid"):
        polygon_tables(dv, R.X0, R.Y0, 1.0, ny, nx, row0=5, rows=ny)
