"""The band series above the kernel, without a GPU: the C ABI's null handle,
the key rule's edge cases in its numpy restatement (tests/band_ref.py), the
banded-run driver's blocking and period cutting over a stub engine, the snow
line, band_edges, and the shards' all-reduce (gloo, world size 2)."""

from __future__ import annotations

import os
import socket
import subprocess
import sys
import warnings
from types import SimpleNamespace

import numpy as np
import pytest

from tests.band_ref import band_cells, band_count, band_fsum, band_of
from tests.harness import ROOT


def test_null_handle_is_rejected_without_a_device():
    """tfg_band_series fails cleanly on a null handle (no HIP call is made),
    and the binding lists the symbol; the entry point is an addition to ABI 8."""
    import ctypes

    from topoflow_glacier import _native as nat

    L = nat.load()
    edges = (ctypes.c_double * 3)(0.0, 1.0, 2.0)
    b = nat.TfgBands(2, 0, edges, 0.0)
    out = (ctypes.c_double * 4)()
    assert L.tfg_band_series(None, nat.FIELD["M_total"], 0, 1, ctypes.byref(b), out, None, None, 0) == nat.ERR_ARG
    assert b"null handle" in L.tfg_last_error(None)
    assert "tfg_band_series" in nat.exported_symbols()
    assert L.tfg_abi_version() == 8
    assert ctypes.sizeof(nat.TfgBands) == 24  # int32, int32, pointer, double (include/tfg.h tfg_bands)


def test_band_ref_edge_semantics():
    """A value on an edge goes up; on the last edge, below the first, NaN and
    +inf are out; the out cells' values (NaN included) reach nothing."""
    edges = np.array([1000.0, 2000.0, 2000.2, 3000.0])
    z = np.array([1000.0, 1999.9, 2000.0, np.float32(2000.2), 2000.2, 2999.9, 3000.0, 999.9, np.nan, np.inf, -np.inf])
    assert float(np.float32(2000.2)) == 2000.199951171875
    want = [0, 0, 1, 1, 2, 2, -1, -1, -1, -1, -1]
    assert band_of(z, edges).tolist() == want
    cid = np.array([0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0], dtype=np.int32)
    v = np.array([1.0, 2.0, 4.0, 8.0, 16.0, 32.0, np.nan, np.nan, np.nan, 7.0, 9.0])
    assert band_cells(cid, z, edges, 2).tolist() == [[1, 1, 1], [1, 1, 1]]
    assert band_fsum(cid, z, edges, v, 2).tolist() == [[1.0, 4.0, 16.0], [2.0, 8.0, 32.0]]
    assert band_count(cid, z, edges, v, 4.0, 2).tolist() == [[0, 0, 1], [0, 1, 1]]  # strict: 4.0 is not above 4.0
    assert band_count(cid, z, edges, v, -np.inf, 2).tolist() == [[1, 1, 1], [1, 1, 1]]
    # a NaN value in a band: exactly its entry, and never counted
    v2 = v.copy()
    v2[2] = np.nan
    got = band_fsum(cid, z, edges, v2, 2)
    assert np.isnan(got[0, 1]) and np.isnan(got).sum() == 1
    assert band_count(cid, z, edges, v2, -np.inf, 2).tolist() == [[1, 0, 1], [1, 1, 1]]
    # without a raster every cell is in catchment 0; leading axes are summed
    assert band_fsum(None, z[:6], edges, np.stack([v[:6], v[:6]]), 1).tolist() == [[6.0, 24.0, 96.0]]


class StubBandEngine:
    """What banded_run uses of a GlacierEngine, on the host: step k (absolute)
    writes `plane(k)` ([n_catch][n_bands] sums and counts of its plane) to
    history slot k % hist_depth; band_series reads the ring back."""

    def __init__(self, hist_depth, cells, dt=1.0, step_index=0):
        self.hist_depth, self.step_index = hist_depth, step_index
        self.cells = np.asarray(cells, dtype=np.int64)
        self.n_catch, self.n_bands = self.cells.shape
        self.params = SimpleNamespace(dt=dt)
        self.ring = {}
        self.calls = []

    def plane(self, name, k):
        w = {"SM": 1.0, "IM": 0.5, "h_snow": 2.0}[name]
        sums = w * (k + 1) * (1.0 + np.arange(self.n_catch * self.n_bands).reshape(self.n_catch, self.n_bands))
        counts = np.minimum(self.cells, (k + np.arange(self.n_bands)[None, :]) % 4)
        return np.where(self.cells > 0, sums, 0.0), counts

    def run(self, nsteps, frames=None):
        self.calls.append(("run", nsteps, None if frames is None else list(frames)))
        for k in range(self.step_index, self.step_index + nsteps):
            self.ring[k % self.hist_depth] = k
        self.step_index += nsteps

    def band_series(self, name, edges, first=None, count=None, threshold=0.0, want=("sum", "count", "cells"), out=None):
        self.calls.append(("bands", name, first, count, threshold, tuple(want)))
        assert len(edges) == self.n_bands + 1 and out is None
        steps = [self.ring[(first + j) % self.hist_depth] for j in range(count)]
        res = {"sum": np.stack([self.plane(name, k)[0] for k in steps]),
               "count": np.stack([self.plane(name, k)[1] for k in steps])}
        if "cells" in want:
            res["cells"] = self.cells.copy()
        return res


def test_banded_run_blocks_and_periods_over_a_stub_engine():
    """20 steps on a ring of 8 slots from step 5 (the first block starts at
    slot 5 and wraps), periods of 6 steps (6, 6, 6, 2: no period boundary but
    the start falls on a block boundary): blocks of 8, 8 and 4 steps, one
    band_series call per block and field on the slot the block's first step
    wrote; sums and counts per period in step order; an empty band reads 0 in
    sum, mean, fraction and melt_depth, with no warning."""
    from topoflow_glacier.bands import banded_run

    cells = np.array([[4, 0, 7], [1, 5, 0]])
    depth, start, nsteps, every, dt = 8, 5, 20, 6, 0.5
    eng = StubBandEngine(depth, cells, dt=dt, step_index=start)
    edges = np.array([1000.0, 2000.0, 2500.0, 3000.0])
    frames = (np.arange(nsteps) * 7) % 24
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        res = banded_run(eng, nsteps, every, edges, ("SM", "IM", "h_snow"), frames=frames, threshold={"h_snow": 0.05})
    runs = [c for c in eng.calls if c[0] == "run"]
    assert [c[1] for c in runs] == [8, 8, 4]
    assert [c[2] for c in runs] == [list(frames[0:8]), list(frames[8:16]), list(frames[16:20])]
    assert [c[0] for c in eng.calls] == ["run", "bands", "bands", "bands"] * 3
    calls = [c for c in eng.calls if c[0] == "bands"]
    assert [(c[1], c[2], c[3]) for c in calls] == [(f, s, n) for s, n in ((5, 8), (13 % depth, 8), (21 % depth, 4))
                                                    for f in ("SM", "IM", "h_snow")]
    assert [c[4] for c in calls[:3]] == [0.0, 0.0, 0.05]
    assert "cells" in calls[0][5] and all("cells" not in c[5] for c in calls[1:])  # the hypsometry is read once
    assert eng.step_index == start + nsteps
    assert res["periods"].tolist() == [6, 6, 6, 2]
    assert np.array_equal(res["cells"], cells) and np.array_equal(res["edges"], edges)
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
            assert np.isfinite(got[key]).all() and np.all(got[key][:, cells == 0] == 0.0), (name, key)
        assert (got["fraction"] <= 1.0).all() and (got["fraction"] > 0).any()
    melt = res["fields"]["SM"]["sum"] + res["fields"]["IM"]["sum"]
    assert np.array_equal(res["melt_depth"], np.where(cells > 0, melt * (dt * 3600.0) / np.maximum(cells, 1), 0.0))
    assert (res["melt_depth"][:, cells > 0] > 0).all() and np.all(res["melt_depth"][:, cells == 0] == 0.0)
    # one field as a string, no frames, a period longer than the run: no melt_depth
    eng2 = StubBandEngine(24, cells)
    res2 = banded_run(eng2, 5, 10, edges, "SM")
    assert res2["periods"].tolist() == [5] and "melt_depth" not in res2
    assert [c[:4] for c in eng2.calls] == [("run", 5, None), ("bands", "SM", 0, 5)]
    with pytest.raises(ValueError):
        banded_run(eng2, 0, 1, edges, "SM")
    with pytest.raises(ValueError):
        banded_run(eng2, 4, 2, edges, "SM", frames=[0, 1])


def test_snow_line_on_hand_made_profiles():
    from topoflow_glacier.bands import snow_line

    edges = np.array([1000.0, 1200.0, 1400.0, 1600.0, 1800.0])  # centres 1100, 1300, 1500, 1700
    frac = np.array([[0.0, 0.25, 0.75, 1.0],     # crosses 0.5 half way between 1300 and 1500
                     [0.6, 0.7, 0.9, 1.0],       # the lowest band already reaches it
                     [0.0, 0.1, 0.2, 0.3],       # never
                     [0.0, 0.5, 0.4, 1.0],       # reaches it exactly at a centre: the lowest crossing
                     [0.0, np.nan, 1.0, 1.0]])   # a band without data is skipped: 1100 .. 1500
    got = snow_line(frac, edges)
    assert got.shape == (5,)
    assert got[0] == 1400.0 and got[1] == 1100.0 and np.isnan(got[2]) and got[3] == 1300.0 and got[4] == 1300.0
    assert snow_line(frac[0], edges, level=0.25) == 1300.0
    assert snow_line(frac[0], edges, level=0.125) == 1200.0
    per = snow_line(np.stack([frac[:2], frac[2:4]]), edges)  # leading axes: [period][catchment]
    assert per.shape == (2, 2) and per[0, 0] == 1400.0 and np.isnan(per[1, 0])
    with pytest.raises(ValueError):
        snow_line(frac[:, :3], edges)


def test_band_edges():
    from topoflow_glacier.bands import band_edges

    e = band_edges(1500.0, 3000.0, 100.0)
    assert e.dtype == np.float64 and e.size == 16 and e[0] == 1500.0 and e[-1] == 3000.0
    assert np.array_equal(e, 1500.0 + 100.0 * np.arange(16))
    e = band_edges(1503.0, 2999.8, 250.0)  # the last edge is the first at or above z_max
    assert e.tolist() == [1503.0, 1753.0, 2003.0, 2253.0, 2503.0, 2753.0, 3003.0]
    assert band_edges(0.0, 64.0, 1.0).size == 65
    for bad in ((0.0, 65.0, 1.0), (1.0, 1.0, 1.0), (0.0, 1.0, 0.0), (0.0, np.inf, 1.0)):
        with pytest.raises(ValueError):
            band_edges(*bad)


def test_allreduce_without_a_group_returns_equal_copies():
    from topoflow_glacier.sharding import allreduce_band_series

    s = np.arange(12, dtype=np.float64).reshape(2, 2, 3)
    c = np.arange(12, dtype=np.int64).reshape(2, 2, 3)
    cells = np.arange(6, dtype=np.int32).reshape(2, 3)
    rs, rc, rl = allreduce_band_series(s, c, cells)
    for r, a in ((rs, s), (rc, c), (rl, cells)):
        assert r is not a and not np.shares_memory(r, a)
        np.testing.assert_array_equal(r, a)
    assert rs.dtype == np.float64 and rc.dtype == np.int64 and rl.dtype == np.int64
    assert allreduce_band_series(None, None, cells)[:2] == (None, None)


def _port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_allreduce_band_series_gloo_world2(tmp_path):
    """16 x 32 cells, 5 steps, 3 catchments x 7 bands over two row blocks:
    each rank's exactly rounded band sums, counts and cells, reduced, are the
    whole grid's (sums within 1e-13, integers equal) and identical on both
    ranks; a count of 2^53 + 1 survives, so the integers travel as int64."""
    from tests.band_worker import BIG, shard_bands

    ny, nx, steps, nc = 16, 32, 5, 3
    env = dict(os.environ, OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={_port()}", str(ROOT / "tests" / "band_worker.py"),
           "--ny", str(ny), "--nx", str(nx), "--steps", str(steps), "--catchments", str(nc), "--out", str(tmp_path)]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    ranks = [dict(np.load(tmp_path / f"rank{i}.npz")) for i in range(2)]
    sums, counts, cells = shard_bands(11, 0, ny, nx, steps, nc)
    assert [int(x["rows"]) for x in ranks] == [8, 8]
    assert (cells > 0).all() and int(cells.sum()) < ny * nx  # every band is used; some cells are in none
    assert not np.array_equal(ranks[0]["sums"], ranks[1]["sums"])
    counts[0, 0, 0] += BIG
    for x in ranks:
        assert x["rsums"].shape == (steps, nc, 7) and x["rcounts"].dtype == np.int64 and x["rcells"].dtype == np.int64
        np.testing.assert_array_equal(x["rsums"], ranks[0]["sums"] + ranks[1]["sums"])
        np.testing.assert_array_equal(x["rcounts"], counts)
        np.testing.assert_array_equal(x["rcells"], cells)
        assert (np.abs(x["rsums"] - sums) <= 1e-13 * np.abs(sums)).all()
    assert int(ranks[0]["rcounts"][0, 0, 0]) == int(ranks[0]["counts"][0, 0, 0]) + int(ranks[1]["counts"][0, 0, 0]) > 2 ** 53
