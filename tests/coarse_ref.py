"""The key rule of tfg_coarse_series restated in numpy, and exactly rounded
binning by it (math.fsum, after tests/band_ref.py).  Test infrastructure.

A cell belongs to its nearest source node, by the rule of nearest-neighbour
gridded forcing (tests/regrid_ref.axis(..., "nearest")): for local cell (r, c)
of a shard whose first row is global row row0,
  J = floor(min(max(y0 + sy (row0 + r), 0), gny - 1) + 0.5)   (I alike, from c)
in fp64, one numpy operation each (no contraction), ties going up.  J depends
on the row alone and I on the column alone.  `grid` is anything with gny, gnx,
y0, x0, sy and sx (a forcing.ForcingGrid); its method is not read.
"""

from __future__ import annotations

import math

import numpy as np

from tests import regrid_ref as G


def coarse_keys(grid, ny: int, nx: int, row0: int = 0):
    """(J [ny], I [nx]): the node row of each model row, the node column of each model column."""
    J = G.axis(grid.gny, grid.y0, grid.sy, row0 + np.arange(ny, dtype=np.int64), "nearest")[0]
    I = G.axis(grid.gnx, grid.x0, grid.sx, np.arange(nx, dtype=np.int64), "nearest")[0]
    return J, I


def coarse_key(grid, ny: int, nx: int, row0: int = 0) -> np.ndarray:
    """[ny * nx] the node index J * gnx + I of each cell."""
    J, I = coarse_keys(grid, ny, nx, row0)
    return (J[:, None] * grid.gnx + I[None, :]).reshape(-1)


def coarse_cells(grid, ny: int, nx: int, row0: int = 0) -> np.ndarray:
    """[gny][gnx] int64 cells of each node: rows(J) x cols(I)."""
    key = coarse_key(grid, ny, nx, row0)
    return np.bincount(key, minlength=grid.gny * grid.gnx).astype(np.int64).reshape(grid.gny, grid.gnx)


def coarse_fsum(grid, ny: int, nx: int, per_cell, row0: int = 0) -> np.ndarray:
    """[gny][gnx] exactly rounded sums (math.fsum) of per_cell [..., ny * nx]
    over the cells of each node and every leading axis; 0 for a node without
    cells.  A NaN value makes exactly its node's entry NaN."""
    key = coarse_key(grid, ny, nx, row0)
    nodes = grid.gny * grid.gnx
    v = np.asarray(per_cell, dtype=np.float64).reshape(-1, key.size)
    order = np.argsort(key, kind="stable")
    bounds = np.searchsorted(key[order], np.arange(nodes + 1))
    v = np.ascontiguousarray(v[:, order].T)  # [cells sorted by node][leading]
    out = np.zeros(nodes, dtype=np.float64)
    for k in np.nonzero(bounds[1:] > bounds[:-1])[0]:
        out[k] = math.fsum(v[bounds[k]:bounds[k + 1]].ravel().tolist())
    return out.reshape(grid.gny, grid.gnx)


def coarse_abs_sum(grid, ny: int, nx: int, per_cell, row0: int = 0) -> np.ndarray:
    """[gny][gnx] the sum of |value| over each node's cells (the scale of the
    summation error bound m 2^-52 sum |v|)."""
    with np.errstate(invalid="ignore"):
        return coarse_fsum(grid, ny, nx, np.abs(np.asarray(per_cell, dtype=np.float64)), row0)


def coarse_count(grid, ny: int, nx: int, per_cell, threshold, row0: int = 0) -> np.ndarray:
    """[gny][gnx] int64 cells of each node with float64(value) > threshold
    (strict; a NaN value is never counted)."""
    key = coarse_key(grid, ny, nx, row0)
    with np.errstate(invalid="ignore"):
        above = np.asarray(per_cell, dtype=np.float64).reshape(-1) > threshold
    return np.bincount(key[above], minlength=grid.gny * grid.gnx).astype(np.int64).reshape(grid.gny, grid.gnx)
