"""Elevation-band profiles of a gridded run: melt and runoff per band (the
mass-balance profile), the snow-covered fraction per band, the band
hypsometry and the snow line, per catchment and per period of steps.

A glacier model is read mostly as a function of elevation.  The planes of the
last ``hist_depth`` steps are resident in the engine's history, so the model
advances in blocks of at most ``hist_depth`` steps (the blocking of
hydrograph.catchment_hydrographs and aggregate.aggregated_run) and each
block's planes are reduced on the device per catchment and elevation band
(GlacierEngine.band_series, tfg_band_series).  What comes back per block is
[steps][n_catch][n_bands]: small, so the periods are accumulated on the host
in step order, and row-block shards are combined in one all-reduce at the end.
"""

from __future__ import annotations

import numpy as np

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


def _per_cell(x, cells):
    """x / cells over the last two axes, 0 where a band has no cells."""
    return np.where(cells > 0, x / np.maximum(cells, 1), 0.0)


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
    nsteps, every = int(nsteps), int(every)
    if nsteps < 1 or every < 1:
        raise ValueError("nsteps and every must be >= 1")
    if frames is not None and len(frames) != nsteps:
        raise ValueError("one forcing frame index per step")
    fields = (fields,) if isinstance(fields, str) else tuple(fields)
    if not fields:
        raise ValueError("banded_run: no field requested")
    thr = {f: float(threshold.get(f, 0.0)) if isinstance(threshold, dict) else float(threshold) for f in fields}
    edges = np.asarray(edges, dtype=np.float64).reshape(-1)
    nper = -(-nsteps // every)
    lengths = np.minimum(every, nsteps - every * np.arange(nper)).astype(np.int64)
    shape = (nper, int(eng.n_catch), edges.size - 1)
    sums = {f: np.zeros(shape, dtype=np.float64) for f in fields}
    counts = {f: np.zeros(shape, dtype=np.int64) for f in fields}
    cells = None
    depth = int(eng.hist_depth)
    for k0 in range(0, nsteps, depth):
        k1 = min(k0 + depth, nsteps)
        first = eng.step_index % depth  # the slot the block's first step writes
        eng.run(k1 - k0, frames=None if frames is None else frames[k0:k1])
        for f in fields:
            want = ("sum", "count", "cells") if cells is None else ("sum", "count")
            r = eng.band_series(f, edges, first=first, count=k1 - k0, threshold=thr[f], want=want)
            if cells is None:
                cells = r["cells"]
            for j in range(k1 - k0):  # step order: a period's sum is a left fold over its steps
                sums[f][(k0 + j) // every] += r["sum"][j]
                counts[f][(k0 + j) // every] += r["count"][j]
    from .sharding import allreduce_band_series

    s_all, c_all, cells = allreduce_band_series(np.stack([sums[f] for f in fields]), np.stack([counts[f] for f in fields]),
                                                cells, group=group)
    res = {"periods": lengths, "edges": edges, "cells": cells, "fields": {}}
    slots = lengths[:, None, None]
    for i, f in enumerate(fields):
        res["fields"][f] = {"sum": s_all[i], "count": c_all[i], "mean": _per_cell(s_all[i], cells),
                            "fraction": _per_cell(c_all[i] / slots, cells)}
    if "SM" in fields and "IM" in fields:
        melt = res["fields"]["SM"]["sum"] + res["fields"]["IM"]["sum"]
        res["melt_depth"] = _per_cell(melt * (float(eng.params.dt) * 3600.0), cells)
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
