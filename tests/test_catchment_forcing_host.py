"""The catchment forcing above the kernel, without a GPU: the C ABI's null
handle, the table assembly, the forced hydrograph driver's frame ring over a
stub engine, the shards' reference elevation (gloo, world size 2), and the
invariants of the restatement the kernel is pinned to (tests/downscale_ref.py)."""

from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest

from tests import downscale_ref as D
from tests.harness import ROOT, bare_ice_inputs
from tests.test_catchment_series_host import StubEngine, _port


def test_null_handle_is_rejected_without_a_device():
    """tfg_set_catchment_forcing fails cleanly on a null handle (no HIP call is
    made), and the binding lists the symbol."""
    import ctypes

    from topoflow_glacier import _native as nat

    L = nat.load()
    table = (ctypes.c_double * 5)()
    ds = nat.TfgDownscale(-0.0065, 2e-4, 1.0, 1, 0)
    assert ctypes.sizeof(nat.TfgDownscale) == 32
    assert L.tfg_set_catchment_forcing(None, 0, 1, table, 0, None, ctypes.byref(ds)) == nat.ERR_ARG
    assert b"null handle" in L.tfg_last_error(None)
    assert L.tfg_set_catchment_forcing(None, 0, 1, table, 0, None, None) == nat.ERR_ARG
    assert "tfg_set_catchment_forcing" in nat.exported_symbols()
    assert L.tfg_abi_version() == 8  # the entry point is an addition to ABI 8


def _table(nsteps, seed, t0="2013-03-20T00"):
    from topoflow_glacier.forcing import ForcingTable

    rng = np.random.default_rng(seed)
    times = np.datetime64(t0, "ns") + np.arange(nsteps) * np.timedelta64(1, "h")
    names = ("P", "T_air", "LW_in", "SW_in", "P_air", "Hum_sp", "uz")
    return ForcingTable(times=times, inputs={k: rng.random(nsteps) + i for i, k in enumerate(names)})


def test_catchment_table_assembly_and_errors():
    """[nsteps][5][n_catch] in tfg_set_inputs order, column c from table c;
    unequal lengths and unequal times raise; the Downscale defaults are off."""
    from topoflow_glacier.forcing import INPUT_ORDER, Downscale, catchment_table

    tabs = [_table(7, s) for s in range(3)]
    t = catchment_table(tabs)
    assert t.shape == (7, 5, 3) and t.dtype == np.float64 and t.flags["C_CONTIGUOUS"]
    assert INPUT_ORDER == ("P_air", "Hum_sp", "P", "T_air", "uz") == D.ORDER
    for c, tab in enumerate(tabs):
        for v, name in enumerate(INPUT_ORDER):
            np.testing.assert_array_equal(t[:, v, c], tab.inputs[name])
    assert catchment_table(iter(tabs[:1])).shape == (7, 5, 1)
    with pytest.raises(ValueError, match="steps"):
        catchment_table([tabs[0], _table(6, 5)])
    with pytest.raises(ValueError, match="times"):
        catchment_table([tabs[0], _table(7, 5, t0="2013-03-20T01")])
    with pytest.raises(ValueError):
        catchment_table([])
    d = Downscale()
    assert (d.lapse_T, d.grad_P, d.pressure, d.rh_max) == (0.0, 0.0, 0, 0.0) and not d.on
    assert Downscale(rh_max=1.0).on and Downscale(pressure=1).on and Downscale(lapse_T=-0.0065).on and Downscale(grad_P=1e-4).on


class ForcedStub(StubEngine):
    """StubEngine with a frame ring: set_catchment_forcing notes which step's
    table row each frame holds, run() checks that every step reads its own row
    and a write checks that the row it replaces has been read by a queued step."""

    def __init__(self, hist_depth, n_frames, n_catch, da_m2):
        super().__init__(hist_depth, n_catch, da_m2)
        self.n_frames = n_frames
        self.holds = [None] * n_frames   # the step whose row a frame holds
        self.unread = [False] * n_frames  # written, and its step not queued yet
        self.writes = []

    def set_catchment_forcing(self, table, frame0=0, z_ref=None, downscale=None):
        table = np.asarray(table)
        assert table.ndim == 3 and table.shape[1:] == (5, self.n_catch) and table.shape[0] >= 1
        assert 0 <= frame0 and frame0 + table.shape[0] <= self.n_frames  # a call never wraps the ring
        self.writes.append((frame0, table.shape[0], z_ref, downscale))
        for j in range(table.shape[0]):
            f = frame0 + j
            assert not self.unread[f], f"frame {f} overwritten before step {self.holds[f]} was queued"
            assert np.all(table[j] == table[j, 0, 0])
            self.holds[f], self.unread[f] = int(table[j, 0, 0]), True

    def run(self, nsteps, frames=None):
        assert frames is not None and len(frames) == nsteps
        for j, f in enumerate(frames):
            assert self.holds[int(f)] == self.step_index + j, (self.step_index + j, int(f), self.holds[int(f)])
            self.unread[int(f)] = False
        super().run(nsteps, frames)


def test_forced_hydrograph_driver_frame_ring_over_a_stub_engine():
    """hist_depth 8, n_frames 12, 20 steps: blocks of 8, 8 and 4; the second
    block (steps 8..15 -> frames 8..11, 0..3) wraps the ring and takes two
    calls.  Every step reads the frame written for it, no frame is overwritten
    before its step was queued, z_ref and the downscaling reach every call."""
    from topoflow_glacier.forcing import Downscale
    from topoflow_glacier.hydrograph import forced_catchment_hydrographs
    from topoflow_glacier.routing import boxcar_route

    depth, nf, nsteps, nc, da = 8, 12, 20, 3, 2.5e5
    table = np.broadcast_to(np.arange(nsteps, dtype=np.float64)[:, None, None], (nsteps, 5, nc)).copy()
    eng = ForcedStub(depth, nf, nc, da)
    z_ref, ds = np.array([1.0, 2.0, 3.0]), Downscale(lapse_T=-0.0065)
    res = forced_catchment_hydrographs(eng, table, z_ref=z_ref, downscale=ds, taps=4)
    assert [(w[0], w[1]) for w in eng.writes] == [(0, 8), (8, 4), (0, 4), (4, 4)]
    assert all(w[2] is z_ref and w[3] is ds for w in eng.writes)
    runs = [c for c in eng.calls if c[0] == "run"]
    assert [c[1] for c in runs] == [8, 8, 4]
    assert [c[2] for c in runs] == [list(range(0, 8)), [8, 9, 10, 11, 0, 1, 2, 3], [4, 5, 6, 7]]
    assert not any(eng.unread) and eng.step_index == nsteps
    want = np.stack([StubEngine.plane_sum(k, nc) for k in range(nsteps)]) * da
    np.testing.assert_array_equal(res["runoff"], want)
    np.testing.assert_array_equal(res["routed"], boxcar_route(want, 4))
    # a plain gather needs no z_ref; fewer frames than history slots is refused
    eng2 = ForcedStub(8, 8, nc, da)
    forced_catchment_hydrographs(eng2, table)
    assert [(w[0], w[1]) for w in eng2.writes] == [(0, 8), (0, 8), (0, 4)] and all(w[2] is None for w in eng2.writes)
    with pytest.raises(ValueError, match="n_frames"):
        forced_catchment_hydrographs(ForcedStub(8, 7, nc, da), table)


def test_allreduce_catchment_elevation_without_a_group():
    from topoflow_glacier.sharding import allreduce_catchment_elevation

    z = allreduce_catchment_elevation(np.array([10.0, 0.0, 9.0]), np.array([4, 0, 3]))
    np.testing.assert_array_equal(z, [2.5, 0.0, 3.0])


def test_allreduce_catchment_elevation_gloo_world2(tmp_path):
    """16 x 32 cells of a DEM, 7 catchments over two row blocks: five in bands
    over both ranks, one present on the second rank only, one nowhere.  The
    reduced z_ref is identical on both ranks, the whole grid's mean elevation
    per catchment within 1e-13, and 0 for the catchment without cells."""
    from tests.forcing_worker import raster, shard_sums

    ny, nx, nc = 16, 32, 7
    env = dict(os.environ, OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={_port()}", str(ROOT / "tests" / "forcing_worker.py"),
           "--ny", str(ny), "--nx", str(nx), "--catchments", str(nc), "--out", str(tmp_path)]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    ranks = [dict(np.load(tmp_path / f"rank{i}.npz")) for i in range(2)]
    dem, cid = raster(ny, nx, nc)
    s, cells = shard_sums(dem, cid, nc)
    assert cells[nc - 1] == 0 and (cells[:nc - 1] > 0).all()
    assert ranks[0]["cells"][nc - 2] == 0 and ranks[1]["cells"][nc - 2] > 0  # present on one rank only
    assert [int(x["rows"]) for x in ranks] == [8, 8]
    want = D.catchment_means(cid, dem.reshape(-1), nc)
    assert want[nc - 1] == 0.0 and (want[:nc - 1] > 1000.0).all()
    for x in ranks:
        np.testing.assert_array_equal(x["z_ref"], ranks[0]["z_ref"])
        assert x["z_ref"][nc - 1] == 0.0
        assert np.abs(x["z_ref"] - want).max() <= 1e-13 * np.abs(want).max()
    np.testing.assert_array_equal(ranks[0]["cells"] + ranks[1]["cells"], cells)


def test_the_restatement_gathers_and_keeps_the_catchment_means():
    """A plain gather is table[:, :, cid].  With z_ref the catchment's mean
    elevation and no clamp, the catchment means of T_air and P are the table's
    (the corrections are linear in dz, whose catchment mean is 0), to 1e-12."""
    static, frames = bare_ice_inputs(4, 37, 100, 24)
    n = 3700
    cell = np.arange(n)
    cid = (3 * np.minimum(cell // 925, 3) + cell % 3).astype(np.int32)
    table = np.stack([D.catchment_means(cid, frames[k], 12) for k in D.ORDER], axis=1)
    assert table.shape == (24, 5, 12)
    np.testing.assert_array_equal(D.downscale(table, cid), table[:, :, cid])
    np.testing.assert_array_equal(D.downscale(table, None, elev=static["elev"]), table[:, :, np.zeros(n, dtype=int)])
    z_ref = D.catchment_means(cid, static["elev"], 12)
    out, info = D.downscale(table, cid, static["elev"], z_ref, lapse_T=-0.0065, grad_P=2e-4, parts=True)
    assert not info["clamped"].any() and 700.0 < info["dz"].max() < 800.0 and -800.0 < info["dz"].min() < -700.0
    assert np.abs(D.catchment_means(cid, info["dz"], 12)).max() <= 1e-9
    for v in (D.I_T, D.I_P):
        got, want = D.catchment_means(cid, out[:, v, :], 12), table[:, v, :]
        assert np.abs(want).max() > 0
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), v
    for v in (D.I_PA, D.I_Q, D.I_UZ):  # the terms that are off leave their planes a gather
        np.testing.assert_array_equal(out[:, v, :], table[:, v, cid])
    # a clamped cell breaks the mean (what "no clamp" is for), and P is exactly 0 there
    out2, info2 = D.downscale(table, cid, static["elev"], z_ref, grad_P=2e-3, parts=True)
    assert 0.01 < info2["clamped"].mean() < 0.5
    assert np.all(out2[:, D.I_P, :][:, info2["clamped"]] == 0.0)
