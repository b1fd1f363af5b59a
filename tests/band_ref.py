"""The key rule of tfg_band_series restated in numpy, and exactly rounded
binning by it (math.fsum, after harness.catchment_fsum).  Test infrastructure.

A cell of elevation z is in band k iff edges[k] <= z < edges[k+1]:
np.searchsorted(edges, z, side="right") - 1, kept when in 0 .. n_bands-1.  A
cell below the first edge, at or above the last, or of NaN elevation is in no
band (-1).  The key of a cell in a band is catch_id * n_bands + band.
"""

from __future__ import annotations

import math

import numpy as np


def band_of(elev, edges) -> np.ndarray:
    """[ncell] band of each cell, -1 for a cell in no band."""
    z = np.asarray(elev, dtype=np.float64).reshape(-1)
    edges = np.asarray(edges, dtype=np.float64).reshape(-1)
    k = np.searchsorted(edges, z, side="right") - 1  # NaN sorts past every edge: k = n_bands
    return np.where((k >= 0) & (k < edges.size - 1) & ~np.isnan(z), k, -1).astype(np.int64)


def band_keys(cid, elev, edges):
    """([ncell] key or -1, n_bands)."""
    nb = np.asarray(edges).size - 1
    band = band_of(elev, edges)
    cid = np.zeros(band.size, dtype=np.int64) if cid is None else np.asarray(cid, dtype=np.int64).reshape(-1)
    return np.where(band >= 0, cid * nb + band, -1), nb


def band_cells(cid, elev, edges, n_catch) -> np.ndarray:
    """[n_catch][n_bands] int64 cells of each (catchment, band)."""
    key, nb = band_keys(cid, elev, edges)
    return np.bincount(key[key >= 0], minlength=n_catch * nb).astype(np.int64).reshape(n_catch, nb)


def band_fsum(cid, elev, edges, per_cell, n_catch) -> np.ndarray:
    """[n_catch][n_bands] exactly rounded sums (math.fsum) of per_cell
    [..., ncell] over the cells of each (catchment, band) and every leading
    axis; 0 for an empty one.  Cells in no band are left out before anything
    is added, so their values (NaN included) reach nothing."""
    key, nb = band_keys(cid, elev, edges)
    v = np.asarray(per_cell, dtype=np.float64).reshape(-1, key.size)
    keep = np.nonzero(key >= 0)[0]
    order = keep[np.argsort(key[keep], kind="stable")]
    bounds = np.searchsorted(key[order], np.arange(n_catch * nb + 1))
    v = np.ascontiguousarray(v[:, order].T)  # [kept cells sorted by key][leading]
    out = [math.fsum(v[bounds[k]:bounds[k + 1]].ravel().tolist()) for k in range(n_catch * nb)]
    return np.array(out, dtype=np.float64).reshape(n_catch, nb)


def band_count(cid, elev, edges, per_cell, threshold, n_catch) -> np.ndarray:
    """[n_catch][n_bands] int64 cells of each (catchment, band) with
    float64(value) > threshold (a NaN value is never counted)."""
    key, nb = band_keys(cid, elev, edges)
    with np.errstate(invalid="ignore"):
        above = (np.asarray(per_cell, dtype=np.float64).reshape(-1) > threshold) & (key >= 0)
    return np.bincount(key[above], minlength=n_catch * nb).astype(np.int64).reshape(n_catch, nb)
