"""Per-catchment runoff hydrographs of a gridded run (the
per-catchment reduction handed to routing).

The reference's driver emits, per catchment and step, the runoff
``M_total * da_m2`` [m3 s-1] (examples/run_topoflow_glacier.py:112) and
routes it through a boxcar (:129-131).  On a grid with a catchment-id raster
the same series is the per-catchment sum of every step's M_total plane.  The
planes of the last ``hist_depth`` steps are resident in the engine's history,
so the model advances in blocks of at most ``hist_depth`` steps
(blocks.run_blocks) and each block's planes are reduced on the device (GlacierEngine.catchment_series,
tfg_catchment_series) into the block's rows of one device buffer: no plane
crosses to the host, no host wait separates the blocks, and the buffer is
copied out once at the end.
"""

from __future__ import annotations

import numpy as np

from .blocks import check_steps, run_blocks
from .routing import boxcar_route

__all__ = ["catchment_hydrographs", "forced_catchment_hydrographs"]


def catchment_hydrographs(eng, nsteps: int, frames=None, group=None, taps: int = 20, on_block=None,
                          after_block=None) -> dict:
    """Advance `eng` (a GlacierEngine) by nsteps steps and return
    ``{"runoff": [nsteps][n_catch] m3 s-1, "routed": boxcar_route(runoff, taps)}``.

    frames     forcing frame index per step (default: run()'s step % n_frames)
    group      torch.distributed group of the row-block shards; when a process
               group is up the shards' series are summed (one all-reduce) and
               every rank returns the whole grid's hydrographs
    on_block   on_block(k0, k1) is called before the block of steps k0..k1-1
               (relative to this call) is queued: the place to load the forcing
               frames those steps read
    after_block  after_block(k0, k1, first) is called once the block's steps and
               its series are queued, with the history slot `first` that step k0
               wrote: the place to fold the same planes into per-cell aggregates
               (aggregate.PeriodFolder.fold), so that hydrographs and cell maps
               come out of one pass over the ring
    """
    import torch

    nsteps = check_steps(nsteps, frames)
    buf = torch.empty((nsteps, int(eng.n_catch)), dtype=torch.float64, device=eng.torch_device)
    for k0, k1, first in run_blocks(eng, nsteps, frames, on_block):
        eng.catchment_series("M_total", first=first, count=k1 - k0, out=buf[k0:k1])
        if after_block is not None:
            after_block(k0, k1, first)
    eng.sync()
    runoff = buf.cpu().numpy() * float(eng.params.da_m2)
    from .sharding import allreduce_catchment_series

    runoff = allreduce_catchment_series(runoff, group=group)
    return {"runoff": runoff, "routed": boxcar_route(runoff, taps)}


def forced_catchment_hydrographs(eng, table, z_ref=None, downscale=None, group=None, taps: int = 20) -> dict:
    """catchment_hydrographs driven by a per-catchment forcing table
    [nsteps][5][n_catch] (forcing.catchment_table; a host array or a float64
    CUDA tensor): before each block of steps is queued, the block's frames are
    produced on the device from its table rows
    (GlacierEngine.set_catchment_forcing), step k of this call into frame
    k % n_frames, which the step is then told to read.  A block that wraps
    the frame ring takes two calls.  The block before it has been queued by
    then, and the engine's stream keeps the order, so no frame is overwritten
    before the step that reads it; that needs n_frames >= hist_depth (a block
    is at most hist_depth steps).

    downscale  a forcing.Downscale; None or all-off spreads the values as they are
    z_ref      [n_catch] reference elevations; by default, when a term is on,
               the catchments' mean elevations over all shards
               (GlacierEngine.catchment_mean_elevation,
               sharding.allreduce_catchment_elevation)
    """
    nsteps, nf = int(table.shape[0]), int(eng.n_frames)
    if nf < int(eng.hist_depth):
        raise ValueError(f"n_frames ({nf}) must be >= hist_depth ({eng.hist_depth}): a block's frames are resident together")
    if z_ref is None and downscale is not None and downscale.on:
        from .sharding import allreduce_catchment_elevation

        z_ref = allreduce_catchment_elevation(*eng.catchment_mean_elevation(), group=group)
        if getattr(table, "is_cuda", False):
            import torch

            z_ref = torch.from_numpy(z_ref).to(table.device)

    def write(k0, k1, frame0):
        eng.set_catchment_forcing(table[k0:k1], frame0=frame0, z_ref=z_ref, downscale=downscale)

    return _frame_ring_hydrographs(eng, nsteps, write, group, taps)


def _frame_ring_hydrographs(eng, nsteps: int, write, group, taps: int) -> dict:
    """catchment_hydrographs with step k reading frame k % n_frames:
    write(k0, k1, frame0) produces the frames of steps k0..k1-1 from frame0 on,
    before the block that reads them is queued; a block that wraps the frame
    ring takes two calls."""
    nf = int(eng.n_frames)

    def write_frames(k0, k1):
        f0 = k0 % nf
        head = min(k1 - k0, nf - f0)
        write(k0, k0 + head, f0)
        if k0 + head < k1:  # the block wraps the frame ring
            write(k0 + head, k1, 0)

    frames = (np.arange(nsteps) % nf).astype(np.int32)
    return catchment_hydrographs(eng, nsteps, frames=frames, group=group, taps=taps, on_block=write_frames)


def gridded_forced_hydrographs(eng, src, grid, z_src=None, downscale=None, group=None, taps: int = 20) -> dict:
    """catchment_hydrographs driven by forcing on a regular source grid, src
    [nsteps][5][gny][gnx] (a host array or a float64 CUDA tensor) with its
    forcing.ForcingGrid: before each block of steps is queued, the block's
    frames are interpolated onto the model grid on the device
    (GlacierEngine.set_gridded_forcing), step k of this call into frame
    k % n_frames, under forced_catchment_hydrographs' frame-ring rules
    (n_frames >= hist_depth).  The forcing needs no collective: every rank of
    `group` holds the same source grid and z_src [gny][gnx], and its engine
    its own row0.

    downscale  a forcing.Downscale; None or all-off leaves the interpolated values
    z_src      the source grid's elevation, needed when a term is on
    """
    nsteps = int(src.shape[0])
    if int(eng.n_frames) < int(eng.hist_depth):
        raise ValueError(f"n_frames ({eng.n_frames}) must be >= hist_depth ({eng.hist_depth}): a block's frames are resident together")

    def write(k0, k1, frame0):
        eng.set_gridded_forcing(src[k0:k1], grid, frame0=frame0, z_src=z_src, downscale=downscale)

    return _frame_ring_hydrographs(eng, nsteps, write, group, taps)
