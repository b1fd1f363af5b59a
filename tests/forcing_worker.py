"""One rank of the sharded catchment reference elevation (launched by torchrun
from tests/test_catchment_forcing_host.py).  Test infrastructure.

The rank bins its row block of a synthetic DEM (harness.terrain_dem) over its
rows of a catchment raster into per-catchment elevation sums and cell counts
(what GlacierEngine.catchment_mean_elevation returns for a shard) and combines
them with sharding.allreduce_catchment_elevation.  It writes its own and the
reduced arrays to <out>/rank<r>.npz.
"""

from __future__ import annotations

import argparse
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "topoflow-glacier_amd")]


def raster(ny, nx, n_catch):
    """(dem [ny][nx], ids [ny][nx]): catchment c < n_catch - 2 in bands of
    rows over the whole grid, n_catch - 2 only in the last row (one rank of
    two), n_catch - 1 nowhere."""
    from tests.harness import terrain_dem

    cid = (np.arange(ny)[:, None] * (n_catch - 2) // ny + np.zeros((1, nx), dtype=np.int64)).astype(np.int32)
    cid[-1, : nx // 2] = n_catch - 2
    return terrain_dem(ny, nx), cid


def shard_sums(dem, cid, n_catch):
    return (np.bincount(cid.reshape(-1), weights=dem.reshape(-1), minlength=n_catch),
            np.bincount(cid.reshape(-1), minlength=n_catch).astype(np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ny", type=int, required=True)
    ap.add_argument("--nx", type=int, required=True)
    ap.add_argument("--catchments", type=int, required=True)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()

    import torch.distributed as dist

    from topoflow_glacier.sharding import allreduce_catchment_elevation, row_block

    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    row0, rows = row_block(a.ny, rank, world)
    dem, cid = raster(a.ny, a.nx, a.catchments)
    s, cells = shard_sums(dem[row0:row0 + rows], cid[row0:row0 + rows], a.catchments)
    kept = (s.copy(), cells.copy())
    z_ref = allreduce_catchment_elevation(s, cells)
    assert np.array_equal(s, kept[0]) and np.array_equal(cells, kept[1])  # the arguments are left as they were
    np.savez(Path(a.out) / f"rank{rank}.npz", row0=row0, rows=rows, sum=s, cells=cells, z_ref=z_ref)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
