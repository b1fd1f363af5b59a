"""Elevation-band profiles of a gridded run: melt and runoff per band (the
mass-balance profile), the snow-covered fraction per band, the band
hypsometry and the snow line, per catchment and per period of steps.

A glacier model is read mostly as a function of elevation.  The planes of the
last ``hist_depth`` steps are resident in the engine's history, so the model
advances in blocks of at most ``hist_depth`` steps (blocks.run_blocks) and
each block's planes are reduced on the device per catchment and elevation band
(GlacierEngine.band_series, tfg_band_series).  What comes back per block is
[steps][n_catch][n_bands]: small, so the periods are accumulated on the host
in step order, and row-block shards are combined in one all-reduce at the end
(blocks.period_run).
"""

from __future__ import annotations

import functools

import numpy as np

from .blocks import period_run

__all__ = ["band_edges", "banded_run", "snow_line"]


def band_edges(z_min: float, z_max: float, width: float) -> np.ndarray:
    """Edges of bands `width` metres wide from z_min up, the last edge the
    first at or above z_max: z_min + width * arange(n + 1) (each edge one
    product, so no error accumulates along the profile).  At most 64 bands."""
    z_min, z_max, width = float(z_min), float(z_max), float(width)
    if not (np.isfinite([z_min, z_max, width]).all() and width > 0 and z_max > z_min):
        raise ValueError("band_edges: need finite z_min < z_max and width > 0")
    n = int(np.ceil((z_max - z_min) / width))
    if z_min + width * n < z_max:  # the quotient rounded down
        n += 1
    if n > 64:
        raise ValueError(f"band_edges: {n} bands; tfg_band_series takes at most 64")
    return z_min + width * np.arange(n + 1, dtype=np.float64)


def banded_run(eng, nsteps: int, every: int, edges, fields, frames=None, threshold=0.0, group=None) -> dict:
    """Advance `eng` (a GlacierEngine) by nsteps steps and return, per period
    of `every` steps (the last may be short), per catchment and per elevation
    band, the profiles of the output fields in `fields`.

    edges      [n_bands + 1] band edges [m] (band_edges), tfg_band_series's rule
    fields     names of history fields, e.g. ("SM", "IM", "M_total", "h_snow")
    frames     forcing frame index per step (default: run()'s step % n_frames)
    threshold  a value counts as covered when > threshold: one number, or
               {field: number} (fields not named: 0)
    group      torch.distributed group of the row-block shards; when a process
               group is up the shards' sums, counts and cells are summed (two
               all-reduces) and every rank returns the whole grid's profiles

    Returns ``{"periods": [nperiods] steps of each period, "edges", "cells":
    [n_catch][n_bands] int64 (the hypsometry), "fields": {name: {"sum",
    "count", "mean", "fraction"}}}``, each [nperiods][n_catch][n_bands]: the
    period's sum over steps and cells; the (step, cell) pairs above the
    threshold; mean = sum / cells (per cell of the band, over the period);
    fraction = count / (steps * cells).  A band without cells reads 0 in all
    four.  When both "SM" and "IM" are among the fields, also ``"melt_depth"``
    = (sum SM + sum IM) * dt * 3600 / cells [m per period]."""
    def reader():  # after period_run's checks, where the edges were always parsed
        from .sharding import allreduce_band_series

        res["edges"] = e = np.asarray(edges, dtype=np.float64).reshape(-1)
        return functools.partial(eng.band_series, edges=e), (int(eng.n_catch), e.size - 1), allreduce_band_series

    res = {}
    res.update(period_run(eng, "banded_run", nsteps, every, fields, reader, frames=frames, threshold=threshold, group=group))
    return res


def snow_line(fraction, edges, level: float = 0.5) -> np.ndarray:
    """Per catchment, the lowest elevation [m] at which the covered fraction
    reaches `level`: fraction [..., n_bands] (banded_run's "fraction" of a
    snow field, any leading axes) is read as a profile at the band centres and
    interpolated linearly between the last centre below `level` and the first
    at or above it; the lowest band's centre when that band already reaches
    it.  NaN where no band reaches it.  Bands whose fraction is NaN (no data)
    are skipped."""
    f = np.asarray(fraction, dtype=np.float64)
    e = np.asarray(edges, dtype=np.float64).reshape(-1)
    if f.shape[-1] != e.size - 1:
        raise ValueError("snow_line: fraction's last axis must be the bands of `edges`")
    centres = 0.5 * (e[:-1] + e[1:])
    out = np.full(f.shape[:-1], np.nan)
    for idx in np.ndindex(*f.shape[:-1]):
        p = f[idx]
        ok = ~np.isnan(p)
        z, p = centres[ok], p[ok]
        hit = np.nonzero(p >= level)[0]
        if hit.size == 0:
            continue
        k = int(hit[0])
        out[idx] = z[0] if k == 0 else z[k - 1] + (level - p[k - 1]) / (p[k] - p[k - 1]) * (z[k] - z[k - 1])
    return out
