"""Per-cell maps of a gridded run at a coarser cadence than the step: daily,
monthly or seasonal melt and runoff depth, mean and peak snow depth, hours
with melt, snow-cover duration.

The planes of the last ``hist_depth`` steps are resident in the engine's
history, so the model advances in blocks of at most ``hist_depth`` steps
(blocks.run_blocks) and each block's slots are
folded on the device into per-cell accumulators
(GlacierEngine.cell_aggregate, tfg_cell_aggregate), cut where a period of
``every`` steps ends.  No plane crosses to the host and no host wait separates
the blocks; a period's maps are handed on, or copied out, when it is
complete.  The fold is per cell, so row-block shards need no collective: each
shard's maps are its rows of the whole grid's.
"""

from __future__ import annotations

import numpy as np

from .blocks import check_steps, run_blocks

__all__ = ["STATS", "PeriodFolder", "aggregated_run"]

STATS = ("sum", "mean", "max", "min", "above")


def _parse_fields(fields) -> dict:
    """{"M_total": ("sum",), "SM": ("sum", ("above", 1e-9))} ->
    {name: (stat names in STATS order, threshold)}; a bare "above" counts
    values > 0."""
    out = {}
    for name, spec in fields.items():
        stats, thr = [], 0.0
        for s in ((spec,) if isinstance(spec, str) else spec):
            if not isinstance(s, str):
                s, thr = s[0], float(s[1])
                if s != "above":
                    raise ValueError(f"{name}: only 'above' takes a threshold, not {s!r}")
            if s not in STATS:
                raise ValueError(f"{name}: statistic {s!r} is not one of {STATS}")
            stats.append(s)
        if not stats:
            raise ValueError(f"{name}: no statistic requested")
        out[name] = (tuple(s for s in STATS if s in stats), thr)
    return out


class PeriodFolder:
    """The accumulators of one aggregated run and the cutting of blocks of
    history slots into periods of `every` steps.  fold(first, count) takes the
    slots of `count` consecutive steps, the first of them in slot `first`;
    finish() closes a short last period.  As an after_block hook of
    catchment_hydrographs: ``after_block=lambda k0, k1, first: f.fold(first, k1 - k0)``.

    Two sets of buffers alternate between periods, so what on_period was handed
    stays untouched until the period after next begins."""

    def __init__(self, eng, every: int, fields, on_period=None):
        import torch

        self.eng, self.every = eng, int(every)
        if self.every < 1:
            raise ValueError("every must be >= 1")
        self.fields = _parse_fields(fields)
        self.on_period = on_period
        self.pos = 0      # steps folded into the open period
        self.lengths = []  # steps of each finished period
        self.host = {name: {s: [] for s in stats} for name, (stats, _) in self.fields.items()}
        eng_dtype = {"float32": torch.float32, "float64": torch.float64}[eng.engine]
        kinds = {"sum": torch.float64, "max": eng_dtype, "min": eng_dtype, "above": torch.int32}
        self.sets = []
        for _ in range(2):
            bufs = {}
            for name, (stats, _) in self.fields.items():
                need = {"sum" if s == "mean" else s for s in stats}
                bufs[name] = {k: torch.empty((eng.ny, eng.nx), dtype=kinds[k], device=eng.torch_device)
                              for k in kinds if k in need}
            self.sets.append(bufs)

    def fold(self, first: int, count: int) -> None:
        depth = int(self.eng.hist_depth)
        done = 0
        while done < count:
            m = min(count - done, self.every - self.pos)
            bufs = self.sets[len(self.lengths) % 2]
            for name, (_, thr) in self.fields.items():
                b = bufs[name]
                self.eng.cell_aggregate(name, first=(first + done) % depth, count=m, sum=b.get("sum"), max=b.get("max"),
                                        min=b.get("min"), above=b.get("above"), threshold=thr, init=self.pos == 0)
            done += m
            self.pos += m
            if self.pos == self.every:
                self._close()

    def finish(self) -> None:
        if self.pos:
            self._close()

    def _close(self) -> None:
        p, steps = len(self.lengths), self.pos
        bufs = self.sets[p % 2]
        self.eng.sync()  # the period's folds are done: torch's stream and the host may read
        stats = {}
        for name, (names, _) in self.fields.items():
            b = bufs[name]
            # a device divisor: a true division, where a host scalar would become a multiplication by 1 / steps
            stats[name] = {s: (b["sum"] / b["sum"].new_full((), steps) if s == "mean" else b[s]) for s in names}
        self.lengths.append(steps)
        self.pos = 0
        if self.on_period is not None:
            self.on_period(p, steps, stats)
            return
        for name, st in stats.items():
            for s, t in st.items():
                self.host[name][s].append(t.to("cpu", copy=True).numpy())  # the buffers are reused

    def result(self) -> dict:
        res = {"periods": np.asarray(self.lengths, dtype=np.int64)}
        if self.on_period is None:
            res["stats"] = {name: {s: np.stack(v) for s, v in st.items()} for name, st in self.host.items()}
        return res


def aggregated_run(eng, nsteps: int, every: int, fields, frames=None, on_block=None, on_period=None) -> dict:
    """Advance `eng` (a GlacierEngine) by nsteps steps and aggregate output
    fields per cell over periods of `every` steps.

    fields     {field: statistics}, e.g. ``{"M_total": ("sum",), "h_snow":
               ("mean", "max"), "SM": ("sum", "above")}``: "sum" (float64),
               "mean" (the sum over the period's own step count), "max" and
               "min" (the engine's dtype, NaN-propagating) and "above" (int32:
               the steps with a value > 0, or > thr when given as ("above", thr))
    frames     forcing frame index per step (default: run()'s step % n_frames)
    on_block   on_block(k0, k1) is called before the block of steps k0..k1-1
               (relative to this call) is queued, as in catchment_hydrographs
    on_period  on_period(p, nsteps_in_period, stats) is called when period p is
               complete and its folds have finished, with
               ``stats[field][statistic]`` the [ny][nx] device tensors; they
               are reused from the period after next on, and nothing is kept
               here: a year of daily maps needs two sets of buffers, not 365

    Returns ``{"periods": [nperiods] steps of each period (the last may be
    short)}`` and, without on_period, ``"stats": {field: {statistic:
    [nperiods][ny][nx] host array}}``."""
    nsteps = check_steps(nsteps, frames)
    folder = PeriodFolder(eng, every, fields, on_period=on_period)
    for k0, k1, first in run_blocks(eng, nsteps, frames, on_block):
        folder.fold(first, k1 - k0)
    folder.finish()
    eng.sync()
    return folder.result()
