"""The model's outputs on the coarse grid its forcing came from: runoff, melt,
snow depth and snow-covered fraction per source node and per period of steps.

What a coupled run hands back to the atmospheric model (AORC, WRF), and the
way to write step-wise maps of a large run without a plane leaving the device.
The planes of the last ``hist_depth`` steps are resident in the engine's
history, so the model advances in blocks of at most ``hist_depth`` steps (the
blocking of bands.banded_run) and each block's planes are reduced on the
device per node (GlacierEngine.coarse_series, tfg_coarse_series).  What comes
back per block is [steps][gny][gnx]: small, so the periods are accumulated on
the host in step order, and row-block shards are combined in one all-reduce
at the end.
"""

from __future__ import annotations

import numpy as np

__all__ = ["coarse_run"]


def _per_cell(x, cells):
    """x / cells over the last two axes, 0 where a node has no cells."""
    return np.where(cells > 0, x / np.maximum(cells, 1), 0.0)


def coarse_run(eng, nsteps: int, every: int, grid, fields, frames=None, threshold=0.0, group=None, on_block=None) -> dict:
    """Advance `eng` (a GlacierEngine) by nsteps steps and return, per period
    of `every` steps (the last may be short) and per node of `grid`, the
    output fields in `fields`.

    grid       a forcing.ForcingGrid, the one set_gridded_forcing takes; a cell
               belongs to its nearest node whatever the grid's method
    fields     names of history fields, e.g. ("SM", "IM", "M_total", "h_snow")
    frames     forcing frame index per step (default: run()'s step % n_frames)
    threshold  a value counts as covered when > threshold: one number, or
               {field: number} (fields not named: 0)
    group      torch.distributed group of the row-block shards; when a process
               group is up the shards' sums, counts and cells are summed (two
               all-reduces) and every rank returns the whole grid's arrays
    on_block   called as on_block(k0, k1, {field: coarse_series's dict}) after
               each block of steps k0 .. k1-1, with this shard's per-step
               arrays [k1 - k0][gny][gnx] (the step-wise maps, or what goes
               back to the atmospheric model before the next block)

    Returns ``{"periods": [nperiods] steps of each period, "cells": [gny][gnx]
    int64, "fields": {name: {"sum", "count", "mean", "fraction"}}}``, each
    [nperiods][gny][gnx]: the period's sum over steps and cells; the (step,
    cell) pairs above the threshold; mean = sum / cells (per cell of the node,
    over the period); fraction = count / (steps * cells).  A node without
    cells reads 0 in all four.  When both "SM" and "IM" are among the fields,
    also ``"melt_depth"`` = (sum SM + sum IM) * dt * 3600 / cells [m per
    period]."""
    nsteps, every = int(nsteps), int(every)
    if nsteps < 1 or every < 1:
        raise ValueError("nsteps and every must be >= 1")
    if frames is not None and len(frames) != nsteps:
        raise ValueError("one forcing frame index per step")
    fields = (fields,) if isinstance(fields, str) else tuple(fields)
    if not fields:
        raise ValueError("coarse_run: no field requested")
    thr = {f: float(threshold.get(f, 0.0)) if isinstance(threshold, dict) else float(threshold) for f in fields}
    nper = -(-nsteps // every)
    lengths = np.minimum(every, nsteps - every * np.arange(nper)).astype(np.int64)
    shape = (nper, int(grid.gny), int(grid.gnx))
    sums = {f: np.zeros(shape, dtype=np.float64) for f in fields}
    counts = {f: np.zeros(shape, dtype=np.int64) for f in fields}
    cells = None
    depth = int(eng.hist_depth)
    for k0 in range(0, nsteps, depth):
        k1 = min(k0 + depth, nsteps)
        first = eng.step_index % depth  # the slot the block's first step writes
        eng.run(k1 - k0, frames=None if frames is None else frames[k0:k1])
        block = {}
        for f in fields:
            want = ("sum", "count", "cells") if cells is None else ("sum", "count")
            r = block[f] = eng.coarse_series(f, grid, first=first, count=k1 - k0, threshold=thr[f], want=want)
            if cells is None:
                cells = r["cells"]
            for j in range(k1 - k0):  # step order: a period's sum is a left fold over its steps
                sums[f][(k0 + j) // every] += r["sum"][j]
                counts[f][(k0 + j) // every] += r["count"][j]
        if on_block is not None:
            on_block(k0, k1, block)
    from .sharding import allreduce_coarse_series

    s_all, c_all, cells = allreduce_coarse_series(np.stack([sums[f] for f in fields]), np.stack([counts[f] for f in fields]),
                                                  cells, group=group)
    res = {"periods": lengths, "cells": cells, "fields": {}}
    slots = lengths[:, None, None]
    for i, f in enumerate(fields):
        res["fields"][f] = {"sum": s_all[i], "count": c_all[i], "mean": _per_cell(s_all[i], cells),
                            "fraction": _per_cell(c_all[i] / slots, cells)}
    if "SM" in fields and "IM" in fields:
        melt = res["fields"]["SM"]["sum"] + res["fields"]["IM"]["sum"]
        res["melt_depth"] = _per_cell(melt * (float(eng.params.dt) * 3600.0), cells)
    return res
