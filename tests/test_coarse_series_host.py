"""The coarse series above the kernel, without a GPU: the C ABI's null handle,
the key rule's edge cases in its numpy restatement (tests/coarse_ref.py), the
coarse-run driver's blocking and period cutting over a stub engine, and the
shards' all-reduce (gloo, world size 2)."""

from __future__ import annotations

import os
import socket
import subprocess
import sys
import warnings
from types import SimpleNamespace

import numpy as np
import pytest

from tests.coarse_ref import coarse_abs_sum, coarse_cells, coarse_count, coarse_fsum, coarse_keys
from tests.harness import ROOT


def grid(gny, gnx, y0=0.0, x0=0.0, sy=1.0, sx=1.0):
    return SimpleNamespace(gny=gny, gnx=gnx, y0=y0, x0=x0, sy=sy, sx=sx, method="bilinear")  # the method is not read


def test_null_handle_is_rejected_without_a_device():
    """tfg_coarse_series fails cleanly on a null handle (no HIP call is made),
    and the binding lists the symbol; the entry point is an addition to ABI 8."""
    import ctypes

    from topoflow_glacier import _native as nat

    L = nat.load()
    g = nat.TfgForcingGrid(2, 2, nat.REGRID_NEAREST, 0, 0.0, 0.0, 1.0, 1.0, 0)
    out = (ctypes.c_double * 4)(-7.0, -7.0, -7.0, -7.0)
    assert L.tfg_coarse_series(None, nat.FIELD["M_total"], 0, 1, ctypes.byref(g), 0.0, out, None, None, 0) == nat.ERR_ARG
    assert b"null handle" in L.tfg_last_error(None)
    assert list(out) == [-7.0] * 4
    assert "tfg_coarse_series" in nat.exported_symbols()
    assert L.tfg_abi_version() == 8
    assert ctypes.sizeof(nat.TfgForcingGrid) == 56  # the struct tfg_set_gridded_forcing takes (include/tfg.h)


def test_coarse_ref_key_rule():
    """A tie goes up; a reversed axis; cells outside the source are clamped
    onto its edge nodes; a node nobody is nearest to has no cells."""
    # 5 columns at source coordinates 0, 0.5, 1, 1.5, 2: the halves are ties
    _, I = coarse_keys(grid(1, 3, sx=0.5), 1, 5)
    assert I.tolist() == [0, 1, 1, 2, 2]
    # rows at 2, 1.5, 1, 0.5, 0: the source runs against the model, ties still go up
    J, _ = coarse_keys(grid(3, 1, y0=2.0, sy=-0.5), 5, 1)
    assert J.tolist() == [2, 2, 1, 1, 0]
    # a shard's rows are the global rows from row0 on
    J, _ = coarse_keys(grid(3, 1, y0=2.0, sy=-0.5), 3, 1, row0=2)
    assert J.tolist() == [1, 1, 0]
    # columns at -1.2, -0.2, 0.8, 1.8, 2.8 of 2 nodes: clamped to 0, 0, 0.8, 1, 1
    g = grid(1, 2, x0=-1.2)
    _, I = coarse_keys(g, 1, 5)
    assert I.tolist() == [0, 0, 1, 1, 1]
    assert coarse_cells(g, 3, 5).tolist() == [[6, 9]]  # every cell is some node's: rows(J) x cols(I)
    # columns at 0 and 2 of 4 nodes: nodes 1 and 3 are nobody's
    g = grid(2, 4, sy=0.4, sx=2.0)
    assert coarse_cells(g, 3, 2).tolist() == [[2, 0, 2, 0], [1, 0, 1, 0]]  # rows at 0, 0.4, 0.8
    v = np.arange(6.0) + 1.0  # [[1, 2], [3, 4], [5, 6]]
    assert coarse_fsum(g, 3, 2, v).tolist() == [[4.0, 0.0, 6.0, 0.0], [5.0, 0.0, 6.0, 0.0]]
    assert coarse_count(g, 3, 2, v, 2.5).tolist() == [[1, 0, 1, 0], [1, 0, 1, 0]]


def test_coarse_ref_nan_and_threshold():
    """A NaN value reaches exactly its node's sum and is never counted; the
    threshold is strict; leading axes are summed."""
    g = grid(2, 2, sy=1.0 / 3.0, sx=0.5)  # 4 x 3 cells: rows 0,1 -> J 0; rows 2,3 -> J 1 (row 1 at 1/3; row 2 at 2/3)
    J, I = coarse_keys(g, 4, 3)
    assert J.tolist() == [0, 0, 1, 1] and I.tolist() == [0, 1, 1]
    v = np.array([1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 128.0, 256.0, 512.0, 1024.0, 2048.0])
    assert coarse_cells(g, 4, 3).tolist() == [[2, 4], [2, 4]]
    assert coarse_fsum(g, 4, 3, v).tolist() == [[9.0, 54.0], [576.0, 3456.0]]
    assert coarse_abs_sum(g, 4, 3, -v).tolist() == [[9.0, 54.0], [576.0, 3456.0]]
    assert coarse_count(g, 4, 3, v, 16.0).tolist() == [[0, 1], [2, 4]]  # strict: 16.0 is not above 16.0
    assert coarse_count(g, 4, 3, v, np.nextafter(16.0, -np.inf)).tolist() == [[0, 2], [2, 4]]
    assert coarse_count(g, 4, 3, v, -np.inf).tolist() == [[2, 4], [2, 4]]
    assert coarse_count(g, 4, 3, v, np.inf).tolist() == [[0, 0], [0, 0]]
    v2 = v.copy()
    v2[4] = np.nan  # cell (1, 1): node (0, 1)
    got = coarse_fsum(g, 4, 3, v2)
    assert np.isnan(got[0, 1]) and np.isnan(got).sum() == 1 and got[1].tolist() == [576.0, 3456.0]
    assert coarse_count(g, 4, 3, v2, -np.inf).tolist() == [[2, 3], [2, 4]]
    assert coarse_fsum(g, 4, 3, np.stack([v, v])).tolist() == [[18.0, 108.0], [1152.0, 6912.0]]


class StubCoarseEngine:
    """What coarse_run uses of a GlacierEngine, on the host (after
    test_band_series_host.StubBandEngine): step k (absolute) writes `plane(k)`
    ([gny][gnx] sums and counts of its plane) to history slot k % hist_depth;
    coarse_series reads the ring back."""

    def __init__(self, hist_depth, cells, dt=1.0, step_index=0):
        self.hist_depth, self.step_index = hist_depth, step_index
        self.cells = np.asarray(cells, dtype=np.int64)
        self.gny, self.gnx = self.cells.shape
        self.params = SimpleNamespace(dt=dt)
        self.ring = {}
        self.calls = []

    def plane(self, name, k):
        w = {"SM": 1.0, "IM": 0.5, "h_snow": 2.0}[name]
        sums = w * (k + 1) * (1.0 + np.arange(self.gny * self.gnx).reshape(self.gny, self.gnx))
        counts = np.minimum(self.cells, (k + np.arange(self.gnx)[None, :]) % 4)
        return np.where(self.cells > 0, sums, 0.0), counts

    def run(self, nsteps, frames=None):
        self.calls.append(("run", nsteps, None if frames is None else list(frames)))
        for k in range(self.step_index, self.step_index + nsteps):
            self.ring[k % self.hist_depth] = k
        self.step_index += nsteps

    def coarse_series(self, name, grid, first=None, count=None, threshold=0.0, want=("sum", "count", "cells"), out=None):
        self.calls.append(("coarse", name, first, count, threshold, tuple(want)))
        assert (grid.gny, grid.gnx) == (self.gny, self.gnx) and out is None
        steps = [self.ring[(first + j) % self.hist_depth] for j in range(count)]
        res = {"sum": np.stack([self.plane(name, k)[0] for k in steps]),
               "count": np.stack([self.plane(name, k)[1] for k in steps])}
        if "cells" in want:
            res["cells"] = self.cells.copy()
        return res


def test_coarse_run_blocks_and_periods_over_a_stub_engine():
    """20 steps on a ring of 8 slots from step 5 (the first block starts at
    slot 5 and wraps), periods of 6 steps (6, 6, 6, 2: the last is short, and
    the periods straddle the blocks of 8, 8 and 4 steps): one coarse_series
    call per block and field on the slot the block's first step wrote; sums
    and counts per period in step order; a node without cells reads 0 in sum,
    mean, fraction and melt_depth, with no warning; on_block sees each block."""
    from topoflow_glacier.coarse import coarse_run

    cells = np.array([[4, 0, 7], [1, 5, 0]])
    depth, start, nsteps, every, dt = 8, 5, 20, 6, 0.5
    eng = StubCoarseEngine(depth, cells, dt=dt, step_index=start)
    g = grid(2, 3)
    frames = (np.arange(nsteps) * 7) % 24
    seen = []
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        res = coarse_run(eng, nsteps, every, g, ("SM", "IM", "h_snow"), frames=frames, threshold={"h_snow": 0.05},
                         on_block=lambda k0, k1, block: seen.append((k0, k1, sorted(block), block["SM"]["sum"].shape)))
    runs = [c for c in eng.calls if c[0] == "run"]
    assert [c[1] for c in runs] == [8, 8, 4]
    assert [c[2] for c in runs] == [list(frames[0:8]), list(frames[8:16]), list(frames[16:20])]
    assert [c[0] for c in eng.calls] == ["run", "coarse", "coarse", "coarse"] * 3
    calls = [c for c in eng.calls if c[0] == "coarse"]
    assert [(c[1], c[2], c[3]) for c in calls] == [(f, s, n) for s, n in ((5, 8), (13 % depth, 8), (21 % depth, 4))
                                                    for f in ("SM", "IM", "h_snow")]
    assert [c[4] for c in calls[:3]] == [0.0, 0.0, 0.05]
    assert "cells" in calls[0][5] and all("cells" not in c[5] for c in calls[1:])  # the cells are read once
    assert seen == [(0, 8, ["IM", "SM", "h_snow"], (8, 2, 3)), (8, 16, ["IM", "SM", "h_snow"], (8, 2, 3)),
                    (16, 20, ["IM", "SM", "h_snow"], (4, 2, 3))]
    assert eng.step_index == start + nsteps
    assert res["periods"].tolist() == [6, 6, 6, 2]
    assert np.array_equal(res["cells"], cells) and res["cells"].dtype == np.int64
    bounds = [(0, 6), (6, 12), (12, 18), (18, 20)]
    for name in ("SM", "IM", "h_snow"):
        got = res["fields"][name]
        for p, (a, b) in enumerate(bounds):
            want_sum = np.zeros(cells.shape)
            want_count = np.zeros(cells.shape, dtype=np.int64)
            for k in range(start + a, start + b):  # the same left fold
                want_sum += eng.plane(name, k)[0]
                want_count += eng.plane(name, k)[1]
            assert np.array_equal(got["sum"][p], want_sum), (name, p)
            assert np.array_equal(got["count"][p], want_count) and got["count"].dtype == np.int64
            assert np.array_equal(got["mean"][p], np.where(cells > 0, want_sum / np.maximum(cells, 1), 0.0))
            assert np.array_equal(got["fraction"][p], np.where(cells > 0, want_count / (b - a) / np.maximum(cells, 1), 0.0))
        for key in ("sum", "mean", "fraction"):
            assert got[key].shape == (4, 2, 3)
            assert np.isfinite(got[key]).all() and np.all(got[key][:, cells == 0] == 0.0), (name, key)
        assert (got["fraction"] <= 1.0).all() and (got["fraction"] > 0).any()
    melt = res["fields"]["SM"]["sum"] + res["fields"]["IM"]["sum"]
    assert np.array_equal(res["melt_depth"], np.where(cells > 0, melt * (dt * 3600.0) / np.maximum(cells, 1), 0.0))
    assert (res["melt_depth"][:, cells > 0] > 0).all() and np.all(res["melt_depth"][:, cells == 0] == 0.0)
    # one field as a string, no frames, a period longer than the run: no melt_depth
    eng2 = StubCoarseEngine(24, cells)
    res2 = coarse_run(eng2, 5, 10, g, "SM")
    assert res2["periods"].tolist() == [5] and "melt_depth" not in res2
    assert [c[:4] for c in eng2.calls] == [("run", 5, None), ("coarse", "SM", 0, 5)]
    with pytest.raises(ValueError):
        coarse_run(eng2, 0, 1, g, "SM")
    with pytest.raises(ValueError):
        coarse_run(eng2, 4, 2, g, "SM", frames=[0, 1])
    with pytest.raises(ValueError):
        coarse_run(eng2, 4, 2, g, ())


def test_allreduce_without_a_group_returns_equal_copies():
    from topoflow_glacier.sharding import allreduce_coarse_series

    s = np.arange(12, dtype=np.float64).reshape(2, 2, 3)
    c = np.arange(12, dtype=np.int64).reshape(2, 2, 3)
    cells = np.arange(6, dtype=np.int32).reshape(2, 3)
    rs, rc, rl = allreduce_coarse_series(s, c, cells)
    for r, a in ((rs, s), (rc, c), (rl, cells)):
        assert r is not a and not np.shares_memory(r, a)
        np.testing.assert_array_equal(r, a)
    assert rs.dtype == np.float64 and rc.dtype == np.int64 and rl.dtype == np.int64
    assert allreduce_coarse_series(None, None, cells)[:2] == (None, None)


def _port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_allreduce_coarse_series_gloo_world2(tmp_path):
    """16 x 32 cells, 5 steps, 3 x 5 nodes over two row blocks cut inside node
    row 1: each rank's exactly rounded node sums, counts and cells, reduced,
    are the whole grid's (sums within 1e-13, integers equal) and identical on
    both ranks; a count of 2^53 + 1 survives, so the integers travel as int64."""
    from tests.coarse_worker import BIG, grid_of, shard_nodes

    ny, nx, steps = 16, 32, 5
    J, _ = coarse_keys(grid_of(ny, nx), ny, nx)
    assert J[7] == J[8] == 1  # node row 1 has rows in both blocks: each rank holds a partial of it
    env = dict(os.environ, OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={_port()}", str(ROOT / "tests" / "coarse_worker.py"),
           "--ny", str(ny), "--nx", str(nx), "--steps", str(steps), "--out", str(tmp_path)]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    ranks = [dict(np.load(tmp_path / f"rank{i}.npz")) for i in range(2)]
    sums, counts, cells = shard_nodes(11, 0, ny, ny, nx, steps)
    assert [int(x["rows"]) for x in ranks] == [8, 8]
    assert (cells > 0).all() and int(cells.sum()) == ny * nx  # every cell is some node's
    assert (ranks[0]["cells"][1] > 0).all() and (ranks[1]["cells"][1] > 0).all()  # the shared node row
    assert (ranks[0]["cells"][2] == 0).all() and (ranks[1]["cells"][0] == 0).all()  # a node row outside a shard reads 0
    assert not np.array_equal(ranks[0]["sums"], ranks[1]["sums"])
    counts[0, 0, 0] += BIG
    for x in ranks:
        assert x["rsums"].shape == (steps, 3, 5) and x["rcounts"].dtype == np.int64 and x["rcells"].dtype == np.int64
        np.testing.assert_array_equal(x["rsums"], ranks[0]["sums"] + ranks[1]["sums"])
        np.testing.assert_array_equal(x["rcounts"], counts)
        np.testing.assert_array_equal(x["rcells"], cells)
        assert (np.abs(x["rsums"] - sums) <= 1e-13 * np.abs(sums)).all()
    assert int(ranks[0]["rcounts"][0, 0, 0]) == int(ranks[0]["counts"][0, 0, 0]) + int(ranks[1]["counts"][0, 0, 0]) > 2 ** 53
