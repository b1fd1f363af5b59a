"""The model's outputs on the coarse grid its forcing came from: runoff, melt,
snow depth and snow-covered fraction per source node and per period of steps.

What a coupled run hands back to the atmospheric model (AORC, WRF), and the
way to write step-wise maps of a large run without a plane leaving the device.
The planes of the last ``hist_depth`` steps are resident in the engine's
history, so the model advances in blocks of at most ``hist_depth`` steps
(blocks.run_blocks) and each block's planes are reduced on the device per node
(GlacierEngine.coarse_series, tfg_coarse_series).  What comes back per block
is [steps][gny][gnx]: small, so the periods are accumulated on the host in
step order, and row-block shards are combined in one all-reduce at the end
(blocks.period_run, the driver of bands.banded_run).
"""

from __future__ import annotations

import functools

from .blocks import period_run

__all__ = ["coarse_run"]


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
    def reader():  # after period_run's checks, where the grid was always read first
        from .sharding import allreduce_coarse_series

        return functools.partial(eng.coarse_series, grid=grid), (int(grid.gny), int(grid.gnx)), allreduce_coarse_series

    return period_run(eng, "coarse_run", nsteps, every, fields, reader, frames=frames, threshold=threshold, group=group,
                      on_block=on_block)
