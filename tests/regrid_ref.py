"""numpy fp64 restatement of the gridded-forcing rule
(tfg_set_gridded_forcing, csrc/tfg_forcing.hpp k_forcing_regrid): what the
kernel is pinned to.  Test infrastructure; the reference has no such term (one
cell per catchment).

Source node (j, i) sits at source-grid coordinate (j, i).  For local cell
(r, c) of a shard whose first row is global row row0, R = row0 + r:
  y = y0 + sy R,  yc = min(max(y, 0), gny - 1)             (x alike, from c)
  bilinear  j0 = min(floor(yc), max(gny - 2, 0)), j1 = min(j0 + 1, gny - 1),
            wy = yc - j0 (i0, i1, wx alike), vertically first:
              west = a[j0][i0] + wy (a[j1][i0] - a[j0][i0])
              east = a[j0][i1] + wy (a[j1][i1] - a[j0][i1])
              v    = west + wx (east - west)
  nearest   v = a[floor(yc + 0.5)][floor(xc + 0.5)]          (ties go up)
Every operation is one numpy fp64 operation (no contraction).  With a
downscaling term on, the interpolated five take the place of a catchment's
table values and the interpolated z_src that of z_ref, one "catchment" per
cell, in tests/downscale_ref.downscale.
"""

from __future__ import annotations

import numpy as np

from tests import downscale_ref as D


def axis(m: int, origin: float, scale: float, k, method: str):
    """(lo, hi, w) per model index k (global, integer) on a source axis of m
    nodes: the stencil's two nodes and the weight of the upper one (nearest:
    lo == hi, the nearest node, w = 0)."""
    t = np.float64(origin) + np.float64(scale) * np.asarray(k, dtype=np.int64).astype(np.float64)
    tc = np.minimum(np.maximum(t, np.float64(0.0)), np.float64(m - 1))
    if method == "nearest":
        lo = np.floor(tc + np.float64(0.5)).astype(np.int64)
        return lo, lo, np.zeros(lo.shape)
    if method != "bilinear":
        raise ValueError(method)
    lo = np.minimum(np.floor(tc).astype(np.int64), max(m - 2, 0))
    hi = np.minimum(lo + 1, m - 1)
    return lo, hi, tc - lo.astype(np.float64)


def stencil(grid, ny: int, nx: int, row0: int = 0):
    """((j0, j1, wy) [ny], (i0, i1, wx) [nx]) of a ny x nx shard at row0."""
    ya = axis(grid.gny, grid.y0, grid.sy, row0 + np.arange(ny, dtype=np.int64), grid.method)
    xa = axis(grid.gnx, grid.x0, grid.sx, np.arange(nx, dtype=np.int64), grid.method)
    return ya, xa


def interpolate(a, grid, ny: int, nx: int, row0: int = 0):
    """[..., ny * nx] fp64 from fields a [..., gny][gnx]."""
    a = np.asarray(a, dtype=np.float64)
    assert a.shape[-2:] == (grid.gny, grid.gnx), a.shape
    (j0, j1, wy), (i0, i1, wx) = stencil(grid, ny, nx, row0)
    if grid.method == "nearest":
        v = a[..., j0[:, None], i0[None, :]]
    else:
        with np.errstate(invalid="ignore"):  # inf - inf at a non-finite node
            a00, a10 = a[..., j0[:, None], i0[None, :]], a[..., j1[:, None], i0[None, :]]
            a01, a11 = a[..., j0[:, None], i1[None, :]], a[..., j1[:, None], i1[None, :]]
            west = a00 + wy[:, None] * (a10 - a00)
            east = a01 + wy[:, None] * (a11 - a01)
            v = west + wx[None, :] * (east - west)
    return v.reshape(a.shape[:-2] + (ny * nx,))


def reach(grid, ny: int, nx: int, node, row0: int = 0):
    """[ny * nx] bool: the cells whose stencil holds source node (j, i)."""
    (j0, j1, _), (i0, i1, _) = stencil(grid, ny, nx, row0)
    rows = (j0 == node[0]) | (j1 == node[0])
    cols = (i0 == node[1]) | (i1 == node[1])
    return (rows[:, None] & cols[None, :]).reshape(-1)


def gridded(src, grid, ny: int, nx: int, row0: int = 0, z_src=None, elev=None, parts: bool = False, **ds):
    """[nframes][5][ny * nx] fp64 frames in tfg_set_inputs order from src
    [nframes][5][gny][gnx]; ds: downscale_ref.downscale's terms, applied to
    the cell's elevation `elev` (as the engine holds it) minus the
    interpolated z_src.  parts=True also returns downscale's dict."""
    v = interpolate(src, grid, ny, nx, row0)
    ds = dict(D.OFF, **ds)
    on = ds["lapse_T"] != 0.0 or ds["grad_P"] != 0.0 or ds["pressure"] == 1 or ds["rh_max"] > 0.0
    if not on:
        return (v, {}) if parts else v
    z = interpolate(z_src, grid, ny, nx, row0)
    return D.downscale(v, np.arange(ny * nx), elev, z, parts=parts, **ds)
