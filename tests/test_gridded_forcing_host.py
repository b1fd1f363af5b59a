"""The gridded forcing above the kernel, without a GPU: the C ABI's null
handle and struct layout, ForcingGrid.from_axes, the hydrograph driver's frame
ring over a stub engine, and the properties of the restatement the kernel is
pinned to (tests/regrid_ref.py): shards, a constant field, the source's range
and the reach of a NaN node."""

from __future__ import annotations

import ctypes
import subprocess

import numpy as np
import pytest

from tests import downscale_ref as D
from tests import regrid_ref as G
from tests.harness import ROOT
from tests.test_catchment_forcing_host import ForcedStub
from tests.test_catchment_series_host import StubEngine

NY, NX = 37, 100  # geometry A of tests/test_gpu_gridded_forcing.py


def _grid(method, gny=4, gnx=9, y0=-0.31, x0=-0.27, sy=1 / 9, sx=1 / 11):
    from topoflow_glacier.forcing import ForcingGrid

    return ForcingGrid(gny=gny, gnx=gnx, y0=y0, x0=x0, sy=sy, sx=sx, method=method)


def test_null_handle_is_rejected_without_a_device():
    """tfg_set_gridded_forcing fails cleanly on a null handle (no HIP call is
    made), the binding lists the symbol, and the ABI is still 8."""
    from topoflow_glacier import _native as nat

    L = nat.load()
    src = (ctypes.c_double * 5)()
    g = nat.TfgForcingGrid(1, 1, nat.REGRID_BILINEAR, 0, 0.0, 0.0, 1.0, 1.0, 0)
    ds = nat.TfgDownscale(-0.0065, 2e-4, 1.0, 1, 0)
    assert L.tfg_set_gridded_forcing(None, 0, 1, src, 0, None, ctypes.byref(g), ctypes.byref(ds)) == nat.ERR_ARG
    assert b"null handle" in L.tfg_last_error(None)
    assert L.tfg_set_gridded_forcing(None, 0, 1, src, 0, None, None, None) == nat.ERR_ARG
    assert "tfg_set_gridded_forcing" in nat.exported_symbols()
    assert L.tfg_abi_version() == 8  # the entry point is an addition to ABI 8
    assert (nat.REGRID_NEAREST, nat.REGRID_BILINEAR) == (0, 1)


def test_forcing_grid_layout_matches_header(tmp_path):
    """tfg_forcing_grid's size, offsets and method codes from a gcc probe
    against include/tfg.h, compared with the ctypes mirror."""
    from topoflow_glacier import _native as nat
    from topoflow_glacier.forcing import ForcingGrid

    names = [n for n, _ in nat.TfgForcingGrid._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tfg.h"\nint main(void){printf("%zu %d %d", '
                   "sizeof(tfg_forcing_grid), TFG_REGRID_NEAREST, TFG_REGRID_BILINEAR);"
                   + "".join(f'printf(" %zu", offsetof(tfg_forcing_grid, {n}));' for n in names) + "return 0;}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(nat.TfgForcingGrid) == 56
    assert got[1:3] == [ForcingGrid.METHODS.index("nearest"), ForcingGrid.METHODS.index("bilinear")]
    assert got[3:] == [getattr(nat.TfgForcingGrid, n).offset for n in names]


def test_from_axes_on_ascending_and_descending_axes():
    """A model grid of 30 m cells, rows running north to south, under source
    nodes 1 km apart: the same physical map whichever way the source axes
    are stored (a flipped axis flips the sign of the scale), cell centres on
    source nodes land on them exactly, and a non-uniform axis is refused."""
    from topoflow_glacier.forcing import ForcingGrid

    src_x = 500000.0 + 1000.0 * np.arange(9)
    src_y = 4200000.0 + 1000.0 * np.arange(6)           # ascending: south to north
    y_first, x_first, dy, dx = 4203985.0, 501015.0, -30.0, 30.0
    g = ForcingGrid.from_axes(src_y, src_x, y_first, x_first, dy, dx)
    assert (g.gny, g.gnx, g.method) == (6, 9, "bilinear")
    assert g.sy == pytest.approx(-0.03, rel=1e-15) and g.sx == pytest.approx(0.03, rel=1e-15)
    assert g.y0 == pytest.approx(3.985, rel=1e-12) and g.x0 == pytest.approx(1.015, rel=1e-12)
    f = ForcingGrid.from_axes(src_y[::-1], src_x[::-1], y_first, x_first, dy, dx, method="nearest")  # descending
    assert f.method == "nearest" and f.sy == pytest.approx(0.03, rel=1e-15) and f.sx == pytest.approx(-0.03, rel=1e-15)
    assert f.y0 == pytest.approx(5 - 3.985, rel=1e-12) and f.x0 == pytest.approx(8 - 1.015, rel=1e-12)
    # the two describe one map: a field and its flipped copy interpolate alike (to rounding of the coordinates)
    a = np.random.default_rng(2).uniform(-1, 1, (6, 9))
    f.method = "bilinear"
    va, vf = G.interpolate(a, g, 140, 260), G.interpolate(a[::-1, ::-1], f, 140, 260)
    assert np.abs(va - vf).max() <= 1e-11 and np.ptp(va) > 1.0
    # a cell centred on a node takes the node's value: model cells on every node of a 3 x 4 source
    on = ForcingGrid.from_axes([10.0, 20.0, 30.0], [5.0, 3.0, 1.0, -1.0], 10.0, 5.0, 10.0, -2.0)
    b = np.arange(12.0).reshape(3, 4)
    assert np.array_equal(G.interpolate(b, on, 3, 4), b.reshape(-1))
    one = ForcingGrid.from_axes([7.0], [1.0, 2.0], 0.0, 0.0, 1.0, 1.0)  # a one-node axis: every row clamps to it
    assert (one.gny, one.y0, one.sy) == (1, 0.0, 0.0)
    for bad in ([0.0, 1.0, 2.5], [0.0, 0.0, 0.0], [0.0, np.nan, 2.0], []):
        with pytest.raises(ValueError):
            ForcingGrid.from_axes(bad, src_x, 0.0, 0.0, 1.0, 1.0)
        with pytest.raises(ValueError):
            ForcingGrid.from_axes(src_y, bad, 0.0, 0.0, 1.0, 1.0)


class GriddedStub(ForcedStub):
    """ForcedStub whose frames come from set_gridded_forcing: src[j] holds the
    step number in every node."""

    def set_gridded_forcing(self, src, grid, frame0=0, z_src=None, downscale=None):
        src = np.asarray(src)
        assert src.ndim == 4 and src.shape[1:] == (5, grid.gny, grid.gnx)
        self.grids = getattr(self, "grids", []) + [grid]
        self.set_catchment_forcing(np.broadcast_to(src[:, :, :1, 0], (src.shape[0], 5, self.n_catch)), frame0, z_src, downscale)


def test_gridded_hydrograph_driver_frame_ring_over_a_stub_engine():
    """hist_depth 8, n_frames 12, 20 steps: the second block wraps the frame
    ring and takes two calls; every step reads the frame written for it; grid,
    z_src and the downscaling reach every call."""
    from topoflow_glacier.forcing import Downscale
    from topoflow_glacier.hydrograph import gridded_forced_hydrographs
    from topoflow_glacier.routing import boxcar_route

    depth, nf, nsteps, nc, da = 8, 12, 20, 3, 2.5e5
    grid = _grid("bilinear", gny=2, gnx=3)
    src = np.broadcast_to(np.arange(nsteps, dtype=np.float64)[:, None, None, None], (nsteps, 5, 2, 3)).copy()
    eng = GriddedStub(depth, nf, nc, da)
    z_src, ds = np.ones((2, 3)), Downscale(lapse_T=-0.0065)
    res = gridded_forced_hydrographs(eng, src, grid, z_src=z_src, downscale=ds, taps=4)
    assert [(w[0], w[1]) for w in eng.writes] == [(0, 8), (8, 4), (0, 4), (4, 4)]
    assert all(w[2] is z_src and w[3] is ds for w in eng.writes) and all(g is grid for g in eng.grids)
    assert [c[2] for c in eng.calls if c[0] == "run"] == [list(range(0, 8)), [8, 9, 10, 11, 0, 1, 2, 3], [4, 5, 6, 7]]
    assert not any(eng.unread) and eng.step_index == nsteps
    want = np.stack([StubEngine.plane_sum(k, nc) for k in range(nsteps)]) * da
    np.testing.assert_array_equal(res["runoff"], want)
    np.testing.assert_array_equal(res["routed"], boxcar_route(want, 4))
    with pytest.raises(ValueError, match="n_frames"):
        gridded_forced_hydrographs(GriddedStub(8, 7, nc, da), src, grid)


@pytest.mark.parametrize("method", ["nearest", "bilinear"])
def test_the_restatement_on_shards_constants_range_and_nan(method):
    """Geometry A (37 x 100 cells under 4 x 9 nodes; 3 rows clamp north, 7
    south, 3 columns west, 9 east).  A shard's rows equal the same rows of the
    whole grid bit for bit; a constant field comes back exactly; values stay
    within their field's range; a NaN node reaches exactly the cells whose
    stencil holds it (99 nearest, 550 bilinear for node (2, 5)), a weight of 0
    included, in its own frame and variable."""
    g = _grid(method)
    y, x = g.y0 + g.sy * np.arange(NY), g.x0 + g.sx * np.arange(NX)
    assert [(y < 0).sum(), (y > g.gny - 1).sum(), (x < 0).sum(), (x > g.gnx - 1).sum()] == [3, 7, 3, 9]
    rng = np.random.default_rng(11)
    src = rng.uniform(-3.0, 5.0, (3, 5, g.gny, g.gnx))
    whole = G.interpolate(src, g, NY, NX)
    assert whole.shape == (3, 5, NY * NX)
    for r0, r1 in ((0, 18), (18, 37), (3, 4), (30, 37)):
        assert np.array_equal(G.interpolate(src, g, r1 - r0, NX, row0=r0), whole[..., r0 * NX:r1 * NX]), (r0, r1)
    assert np.all(G.interpolate(np.full((g.gny, g.gnx), 0.1), g, NY, NX) == 0.1)
    lo, hi = src.min(axis=(2, 3))[..., None], src.max(axis=(2, 3))[..., None]
    tol = 3 * 2.0 ** -52 * np.abs(src).max()  # three lerps, each within an ulp of the segment between its ends
    assert np.all(whole >= lo - tol) and np.all(whole <= hi + tol)
    # the clamped corner cells hold the corner nodes
    assert np.array_equal(whole[..., 0], src[..., 0, 0]) and np.array_equal(whole[..., -1], src[..., -1, -1])
    node, f, v = (2, 5), 1, D.I_T
    dirty = src.copy()
    dirty[f, v, node[0], node[1]] = np.nan
    got = G.interpolate(dirty, g, NY, NX)
    want = np.zeros(got.shape, dtype=bool)
    want[f, v] = G.reach(g, NY, NX, node)
    assert int(want.sum()) == {"nearest": 99, "bilinear": 550}[method]
    assert np.array_equal(np.isnan(got), want)
    assert np.array_equal(got[~want], whole[~want])
    if method == "bilinear":  # a weight of 0 does not stop it: node (1, 0) is the upper node, at weight 0, of the clamped rows 0-2
        (j0, j1, wy), _ = G.stencil(g, NY, NX)
        assert np.all(j1[:3] == 1) and np.all(wy[:3] == 0.0)
        dirty = src.copy()
        dirty[f, v, 1, 0] = np.nan
        assert np.isnan(G.interpolate(dirty, g, NY, NX)[f, v, :3 * NX].reshape(3, NX)[:, :3]).all()


def test_the_restatement_downscales_through_the_catchment_rule():
    """With a term on, the interpolated fields and z_src go through
    downscale_ref.downscale with one catchment per cell; with every term off
    the frames are the interpolated fields."""
    g = _grid("bilinear")
    rng = np.random.default_rng(5)
    src = np.empty((2, 5, g.gny, g.gnx))
    for k, (lo, hi) in enumerate(((70000.0, 80000.0), (0.002, 0.006), (0.0, 2e-7), (-12.0, 6.0), (0.5, 9.0))):
        src[:, k] = rng.uniform(lo, hi, (2, g.gny, g.gnx))
    z_src, elev = rng.uniform(1800.0, 2700.0, (g.gny, g.gnx)), rng.uniform(1500.0, 3000.0, NY * NX)
    plain = G.gridded(src, g, NY, NX)
    assert np.array_equal(plain, G.interpolate(src, g, NY, NX))
    assert np.array_equal(G.gridded(src, g, NY, NX, z_src=z_src, elev=elev, **D.OFF), plain)
    out, info = G.gridded(src, g, NY, NX, z_src=z_src, elev=elev, parts=True, lapse_T=-0.0065)
    z = G.interpolate(z_src, g, NY, NX)
    assert np.array_equal(info["dz"], elev - z)
    assert np.array_equal(out[:, D.I_T], plain[:, D.I_T] + np.float64(-0.0065) * (elev - z))
    for v in (D.I_PA, D.I_Q, D.I_P, D.I_UZ):
        assert np.array_equal(out[:, v], plain[:, v])
