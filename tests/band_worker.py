"""One rank of the sharded band series (launched by torchrun from
tests/test_band_series_host.py).  Test infrastructure.

The rank bins a seeded per-cell field of its row block by catchment and
elevation band on the host (tests/band_ref.py), combines sums, counts and
cells with sharding.allreduce_band_series (CPU, gloo) and writes its own and
the reduced arrays to <out>/rank<r>.npz.
"""

from __future__ import annotations

import argparse
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "topoflow-glacier_amd")]

EDGES = np.linspace(1600.0, 2900.0, 8)
BIG = 2 ** 53 + 1  # a count no float64 holds: the integers must travel as int64


def shard_bands(seed, row0, rows, nx, steps, n_catch):
    """(sums [steps][n_catch][7], counts alike, cells [n_catch][7]) of rows row0..row0+rows-1."""
    from tests.band_ref import band_cells, band_count, band_fsum

    cell = (np.arange(rows)[:, None] + row0) * nx + np.arange(nx)[None, :]
    rng = np.random.default_rng(seed)
    whole = rng.random((steps, 4096))  # indexed by global cell: a shard's values are the whole grid's
    cell = cell.reshape(-1)
    elev = 1500.0 + (cell * 7919 % 1500).astype(np.float64)
    cid = (cell * 37 % n_catch).astype(np.int32)
    v = whole[:, cell]
    sums = np.stack([band_fsum(cid, elev, EDGES, v[s], n_catch) for s in range(steps)])
    counts = np.stack([band_count(cid, elev, EDGES, v[s], 0.5, n_catch) for s in range(steps)])
    return sums, counts, band_cells(cid, elev, EDGES, n_catch)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ny", type=int, required=True)
    ap.add_argument("--nx", type=int, required=True)
    ap.add_argument("--steps", type=int, required=True)
    ap.add_argument("--catchments", type=int, default=3)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()

    import torch.distributed as dist

    from topoflow_glacier.sharding import allreduce_band_series, row_block

    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    row0, rows = row_block(a.ny, rank, world)
    sums, counts, cells = shard_bands(a.seed, row0, rows, a.nx, a.steps, a.catchments)
    counts[0, 0, 0] += BIG * rank  # rank 1 alone adds 2^53 + 1
    kept = (sums.copy(), counts.copy(), cells.copy())
    rs, rc, rl = allreduce_band_series(sums, counts, cells)
    assert all(np.array_equal(x, y) for x, y in zip((sums, counts, cells), kept))  # the arguments are left as they were
    only = allreduce_band_series(None, None, cells)
    assert only[0] is None and only[1] is None and np.array_equal(only[2], rl)
    np.savez(Path(a.out) / f"rank{rank}.npz", row0=row0, rows=rows, sums=sums, counts=counts, cells=cells, rsums=rs,
             rcounts=rc, rcells=rl)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
