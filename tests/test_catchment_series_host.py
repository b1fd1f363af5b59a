"""The catchment series above the kernel, without a GPU: the C ABI's null
handle, the hydrograph driver's blocking over a stub engine, and the shards'
all-reduce (gloo, world size 2)."""

from __future__ import annotations

import os
import socket
import subprocess
import sys
from types import SimpleNamespace

import numpy as np

from tests.harness import ROOT, catchment_fsum


def test_null_handle_is_rejected_without_a_device():
    """tfg_catchment_series fails cleanly on a null handle (no HIP call is
    made), and the binding lists the symbol."""
    import ctypes

    from topoflow_glacier import _native as nat

    L = nat.load()
    out = (ctypes.c_double * 4)()
    assert L.tfg_catchment_series(None, nat.FIELD["M_total"], 0, 1, out, 0) == nat.ERR_ARG
    assert b"null handle" in L.tfg_last_error(None)
    assert "tfg_catchment_series" in nat.exported_symbols()
    assert L.tfg_abi_version() == 8  # the entry point is an addition to ABI 8


class StubEngine:
    """What catchment_hydrographs uses of a GlacierEngine, on the host: step k
    (absolute) writes `plane_sums[k]` ([n_catch] sums of its M_total plane)
    to history slot k % hist_depth; catchment_series reads the ring back."""

    torch_device = "cpu"

    def __init__(self, hist_depth, n_catch, da_m2, step_index=0):
        self.hist_depth, self.n_catch, self.step_index = hist_depth, n_catch, step_index
        self.params = SimpleNamespace(da_m2=da_m2)
        self.ring = np.full((hist_depth, n_catch), np.nan)
        self.calls = []

    @staticmethod
    def plane_sum(k, n_catch):
        return (k + 1) * 100.0 + np.arange(n_catch)

    def run(self, nsteps, frames=None):
        self.calls.append(("run", nsteps, None if frames is None else list(frames)))
        for k in range(self.step_index, self.step_index + nsteps):
            self.ring[k % self.hist_depth] = self.plane_sum(k, self.n_catch)
        self.step_index += nsteps

    def catchment_series(self, name="M_total", first=None, count=None, reduce="sum", out=None):
        self.calls.append(("series", name, first, count, reduce))
        assert out.shape == (count, self.n_catch) and out.is_contiguous()
        import torch

        rows = [(first + j) % self.hist_depth for j in range(count)]
        out.copy_(torch.from_numpy(self.ring[rows]))
        return out

    def sync(self):
        self.calls.append(("sync",))


def test_hydrograph_driver_blocks_over_a_stub_engine():
    """20 steps on a ring of 8 slots, from step 5 (so the first block starts at
    slot 5 and wraps): blocks of 8, 8 and 4 steps, each followed by one series
    call on the slot its first step wrote; rows in step order, scaled by
    da_m2; `routed` is the boxcar of the runoff; on_block sees every block
    before it is queued; the frames are handed on block by block."""
    from topoflow_glacier.hydrograph import catchment_hydrographs
    from topoflow_glacier.routing import boxcar_route

    depth, nc, da, start, nsteps = 8, 3, 2.5e5, 5, 20
    eng = StubEngine(depth, nc, da, step_index=start)
    seen = []
    frames = (np.arange(nsteps) * 7) % 24
    res = catchment_hydrographs(eng, nsteps, frames=frames, taps=4,
                                on_block=lambda k0, k1: seen.append((k0, k1, eng.step_index, len(eng.calls))))
    assert [c[1] for c in eng.calls if c[0] == "run"] == [8, 8, 4]
    assert [c[2] for c in eng.calls if c[0] == "run"] == [list(frames[0:8]), list(frames[8:16]), list(frames[16:20])]
    series = [c for c in eng.calls if c[0] == "series"]
    assert [(c[2], c[3]) for c in series] == [(5 % depth, 8), ((5 + 8) % depth, 8), ((5 + 16) % depth, 4)]
    assert all(c[1] == "M_total" and c[4] == "sum" for c in series)
    assert [c[0] for c in eng.calls] == ["run", "series"] * 3 + ["sync"]  # one host wait, at the end
    assert seen == [(0, 8, 5, 0), (8, 16, 13, 2), (16, 20, 21, 4)]  # before each block's run
    want = np.stack([StubEngine.plane_sum(start + k, nc) for k in range(nsteps)]) * da
    assert res["runoff"].shape == (nsteps, nc) and res["runoff"].dtype == np.float64
    np.testing.assert_array_equal(res["runoff"], want)
    np.testing.assert_array_equal(res["routed"], boxcar_route(want, 4))
    assert eng.step_index == start + nsteps
    # the defaults: no frames, no callback, the reference's 20 taps
    eng2 = StubEngine(24, 2, 1.0)
    res2 = catchment_hydrographs(eng2, 5)
    assert [c for c in eng2.calls if c[0] != "sync"] == [("run", 5, None), ("series", "M_total", 0, 5, "sum")]
    np.testing.assert_array_equal(res2["routed"], boxcar_route(res2["runoff"], 20))


def test_allreduce_without_a_group_returns_an_equal_copy():
    from topoflow_glacier.sharding import allreduce_catchment_series

    s = np.arange(12, dtype=np.float64).reshape(4, 3)
    r = allreduce_catchment_series(s)
    assert r is not s and not np.shares_memory(r, s)
    np.testing.assert_array_equal(r, s)
    r[0, 0] = -1.0
    assert s[0, 0] == 0.0


def _port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_allreduce_catchment_series_gloo_world2(tmp_path):
    """16 x 32 cells, 24 steps, bench.py's 43 block catchments (+1 spare row)
    over two row blocks: each rank's numpy sums of the oracle's M_total,
    reduced, equal the whole grid's exactly rounded sums within 1e-13 and are
    identical on both ranks; the reduced cell counts are the whole grid's, so
    the mean taken after the reduction is the whole grid's mean."""
    from tests.series_worker import shard_series

    ny, nx, steps, k = 16, 32, 24, 43
    env = dict(os.environ, OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={_port()}", str(ROOT / "tests" / "series_worker.py"),
           "--ny", str(ny), "--nx", str(nx), "--steps", str(steps), "--catchments", str(k), "--out", str(tmp_path)]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    ranks = [dict(np.load(tmp_path / f"rank{i}.npz")) for i in range(2)]
    whole, cells, cid = shard_series(11, 0, ny, ny, nx, steps, 24, k)
    from tests.harness import oracle_synthetic

    ref, _ = oracle_synthetic(11, ny, nx, steps, 24)
    want = np.stack([catchment_fsum(cid, ref["M_total"][s], k + 1) for s in range(steps)])
    assert (want[:, :k] > 0).any(axis=0).all() and np.all(want[:, k] == 0)  # every catchment runs off at some step
    np.testing.assert_array_equal(np.concatenate([x["cid"] for x in ranks]), cid)
    assert [int(x["rows"]) for x in ranks] == [8, 8]
    assert not np.array_equal(ranks[0]["sums"], ranks[1]["sums"])
    for x in ranks:
        assert x["reduced"].shape == (steps, k + 1)
        np.testing.assert_array_equal(x["reduced"], ranks[0]["reduced"])
        np.testing.assert_array_equal(x["reduced"], ranks[0]["sums"] + ranks[1]["sums"])
        err = np.abs(x["reduced"] - want) / np.where(want != 0, np.abs(want), 1.0)
        assert err.max() <= 1e-13, err.max()
        np.testing.assert_array_equal(x["reduced_cells"], cells)
    mean = np.where(cells > 0, ranks[0]["reduced"] / np.maximum(cells, 1), 0.0)
    assert np.abs(mean - np.where(cells > 0, whole / np.maximum(cells, 1), 0.0)).max() <= 1e-13 * np.abs(mean).max()
