"""A gridded run in blocks of the output history, and its periods.

The planes of the last ``hist_depth`` steps are resident in the engine's
history, so a driver that reduces them on the device advances the model in
blocks of at most ``hist_depth`` steps: run_blocks, the loop of the four run
drivers (hydrograph, aggregate, bands, coarse).  period_run is what
bands.banded_run and coarse.coarse_run share beyond it.
"""

from __future__ import annotations

import numpy as np

__all__ = ["check_steps", "period_run", "run_blocks"]


def check_steps(nsteps, frames=None, every=None) -> int:
    """int(nsteps), or ValueError unless nsteps (and `every`, of a driver with
    periods) is >= 1 and `frames` names one forcing frame per step."""
    nsteps = int(nsteps)
    if nsteps < 1 or (every is not None and int(every) < 1):
        raise ValueError("nsteps must be >= 1" if every is None else "nsteps and every must be >= 1")
    if frames is not None and len(frames) != nsteps:
        raise ValueError("one forcing frame index per step")
    return nsteps


def run_blocks(eng, nsteps: int, frames=None, on_block=None):
    """Advance `eng` by nsteps steps in blocks of at most hist_depth steps and
    yield (k0, k1, first) after each block of steps k0 .. k1-1 (relative to
    this call) has been queued, `first` the history slot step k0 wrote: the
    block's planes are slots first, first + 1, ... following the ring until
    the next block is run.  on_block(k0, k1) is called before the block is
    queued.  Of the engine only hist_depth, step_index and run() are used."""
    depth = int(eng.hist_depth)
    for k0 in range(0, nsteps, depth):
        k1 = min(k0 + depth, nsteps)
        if on_block is not None:
            on_block(k0, k1)
        first = eng.step_index % depth  # the slot the block's first step writes
        eng.run(k1 - k0, frames=None if frames is None else frames[k0:k1])
        yield k0, k1, first


def _per_cell(x, cells):
    """x / cells over the last two axes, 0 where there are no cells."""
    return np.where(cells > 0, x / np.maximum(cells, 1), 0.0)


def period_run(eng, who: str, nsteps, every, fields, reader, frames=None, threshold=0.0, group=None, on_block=None) -> dict:
    """banded_run and coarse_run behind their arguments (their docstrings say
    what comes back).  reader(), called once the arguments here have passed
    their checks, gives (series, tail, allreduce): per field and block,
    series(field, first=, count=, threshold=, want=) gives {"sum", "count"
    [count][*tail], "cells" [*tail] when wanted}; the steps are added into
    periods of `every` steps on the host in step order, and the shards combined
    at the end by `allreduce` (sharding.allreduce_band_series's signature).
    on_block(k0, k1, {field: series's dict}) is called after each block's series."""
    nsteps, every = check_steps(nsteps, frames, every), int(every)
    fields = (fields,) if isinstance(fields, str) else tuple(fields)
    if not fields:
        raise ValueError(f"{who}: no field requested")
    thr = {f: float(threshold.get(f, 0.0)) if isinstance(threshold, dict) else float(threshold) for f in fields}
    series, tail, allreduce = reader()
    nper = -(-nsteps // every)
    lengths = np.minimum(every, nsteps - every * np.arange(nper)).astype(np.int64)
    shape = (nper, *tail)
    sums = {f: np.zeros(shape, dtype=np.float64) for f in fields}
    counts = {f: np.zeros(shape, dtype=np.int64) for f in fields}
    cells = None
    for k0, k1, first in run_blocks(eng, nsteps, frames):
        block = {}
        for f in fields:
            want = ("sum", "count", "cells") if cells is None else ("sum", "count")  # the cells once
            r = block[f] = series(f, first=first, count=k1 - k0, threshold=thr[f], want=want)
            if cells is None:
                cells = r["cells"]
            for j in range(k1 - k0):  # step order: a period's sum is a left fold over its steps
                sums[f][(k0 + j) // every] += r["sum"][j]
                counts[f][(k0 + j) // every] += r["count"][j]
        if on_block is not None:
            on_block(k0, k1, block)
    s_all, c_all, cells = allreduce(np.stack([sums[f] for f in fields]), np.stack([counts[f] for f in fields]), cells,
                                    group=group)
    res = {"periods": lengths, "cells": cells, "fields": {}}
    slots = lengths[:, None, None]
    for i, f in enumerate(fields):
        res["fields"][f] = {"sum": s_all[i], "count": c_all[i], "mean": _per_cell(s_all[i], cells),
                            "fraction": _per_cell(c_all[i] / slots, cells)}
    if "SM" in fields and "IM" in fields:
        melt = res["fields"]["SM"]["sum"] + res["fields"]["IM"]["sum"]
        res["melt_depth"] = _per_cell(melt * (float(eng.params.dt) * 3600.0), cells)
    return res
