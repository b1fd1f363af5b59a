"""One rank of the sharded coarse series (launched by torchrun from
tests/test_coarse_series_host.py).  Test infrastructure.

The rank bins a seeded per-cell field of its row block onto the nodes of a
coarse grid on the host (tests/coarse_ref.py), combines sums, counts and cells
with sharding.allreduce_coarse_series (CPU, gloo) and writes its own and the
reduced arrays to <out>/rank<r>.npz.
"""

from __future__ import annotations

import argparse
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "topoflow-glacier_amd"), str(ROOT / "oracle")]  # oracle: regrid_ref's imports

BIG = 2 ** 53 + 1  # a count no float64 holds: the integers must travel as int64


def grid_of(ny, nx):
    """3 x 5 nodes over ny x nx cells: node row 1 straddles the cut at ny / 2."""
    return SimpleNamespace(gny=3, gnx=5, y0=0.0, x0=0.0, sy=2.0 / (ny - 1), sx=4.0 / (nx - 1))


def shard_nodes(seed, row0, rows, ny, nx, steps):
    """(sums [steps][3][5], counts alike, cells [3][5]) of rows row0..row0+rows-1."""
    from tests.coarse_ref import coarse_cells, coarse_count, coarse_fsum

    g = grid_of(ny, nx)
    cell = ((np.arange(rows)[:, None] + row0) * nx + np.arange(nx)[None, :]).reshape(-1)
    whole = np.random.default_rng(seed).random((steps, ny * nx))  # indexed by global cell: a shard's values are the whole grid's
    v = whole[:, cell]
    sums = np.stack([coarse_fsum(g, rows, nx, v[s], row0) for s in range(steps)])
    counts = np.stack([coarse_count(g, rows, nx, v[s], 0.5, row0) for s in range(steps)])
    return sums, counts, coarse_cells(g, rows, nx, row0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ny", type=int, required=True)
    ap.add_argument("--nx", type=int, required=True)
    ap.add_argument("--steps", type=int, required=True)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()

    import torch.distributed as dist

    from topoflow_glacier.sharding import allreduce_coarse_series, row_block

    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    row0, rows = row_block(a.ny, rank, world)
    sums, counts, cells = shard_nodes(a.seed, row0, rows, a.ny, a.nx, a.steps)
    counts[0, 0, 0] += BIG * rank  # rank 1 alone adds 2^53 + 1
    kept = (sums.copy(), counts.copy(), cells.copy())
    rs, rc, rl = allreduce_coarse_series(sums, counts, cells)
    assert all(np.array_equal(x, y) for x, y in zip((sums, counts, cells), kept))  # the arguments are left as they were
    only = allreduce_coarse_series(None, None, cells)
    assert only[0] is None and only[1] is None and np.array_equal(only[2], rl)
    np.savez(Path(a.out) / f"rank{rank}.npz", row0=row0, rows=rows, sums=sums, counts=counts, cells=cells, rsums=rs,
             rcounts=rc, rcells=rl)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
