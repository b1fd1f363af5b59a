"""The four readers of the output history on one handle, interleaved: what
the modules of the single readers cannot see.  tfg_catchment_series,
tfg_band_series and tfg_coarse_series share one scratch on the handle (fp64
and int32 partials, fp64 and int64 staging of a host call's results), and each
call reserves what it needs of it; a buffer that must grow is released while
the calls queued before it may still be running, so the call waits for the
handle's stream first.  Here every buffer grows at least once behind queued
device-output calls and then serves a host-output call, and every result must
be what the reader gives alone.

Planes: tests/test_gpu_coarse_series.py's integer-valued planes (|v| <= 1024),
planted into the history of a 37 x 100 engine with 8 slots, so every sum is an
integer far below 2^53 and exact in any order: all comparisons are equalities
with a numpy binning of the planted planes.
"""

import contextlib

import numpy as np
import pytest

from tests.band_ref import band_cells, band_count, band_fsum
from tests.coarse_ref import coarse_cells
from tests.harness import BASE_CFG, bare_ice_inputs, make_engine
from tests.test_gpu_band_series import B7, B64
from tests.test_gpu_coarse_series import bin_exact, counts_of, grid_of, int_planes, plant
from tests.test_gpu_diagnostics import NX, NY, SEED, catch_map

pytestmark = pytest.mark.gpu

DEPTH, THR = 8, 100.0


@contextlib.contextmanager
def reader_engine(engine, cid, n_catch, elev):
    """test_gpu_coarse_series.ring_engine with a catchment map and an elevation raster."""
    e = make_engine(BASE_CFG, NY, NX, engine, n_frames=1, hist_depth=DEPTH, n_catch=n_catch, split="off")
    try:
        e.set_field("elev", elev)
        e.set_field("catch_id", cid)
        yield e
    finally:
        e.close()


def ring(planes, first, count):
    """The planes of `count` slots from slot `first`, following the ring."""
    return [planes[(first + j) % DEPTH] for j in range(count)]


@pytest.mark.parametrize("engine", ["float32", "float64"])
def test_interleaved_readers_share_the_scratch(engine):
    """Eight calls on one engine and one sync() after the last (a host call
    waits for its own result, a device call for nothing); 3700 cells are 15
    chunks, so every launch has 15 workgroups.  Bytes each call reserves
    (csrc/tfg_series.hpp, tfg_bands.hpp, tfg_coarse.hpp), "+" where the
    buffer grows:

                                        fp64 part  int32 part  fp64 staging  int64 staging  tables
      0 coarse A (35 nodes), host       2 240 +    1 120 +     2 240 +       2 520 +        568 +
      1 catchment series (32), device   30 720 +
      2 bands B7 (224 keys), device     215 040 +  120 960 +
      3 coarse A, device                2 240      1 120                                    cached
      4 bands B64 (2048 keys), device   491 520 +  368 640 +
      5 coarse D (16 800 nodes), host   236 800    118 400     1 075 200 +   1 209 600 +    4 032 +
      6 cell aggregate, device          (no scratch)
      7 catchment series again, device  30 720

    (catchment: blocks * 8 * n_catch * 8; bands: blocks * NB * K * 8 and
    blocks * (NB * K + K) * 4 with NB = 8 slots per launch at 224 keys and 2
    at 2048, staging hist_depth * K * 8 and (hist_depth * K + K) * 8; coarse:
    nseg * 8 * P * 8 and * 4 with nseg x P = 5 x 7 under A and 37 x 100 under
    D, staging 8 * nodes * 8 and (8 * nodes + nodes) * 8.)  Call 0 is a host
    call, so that the staging exists before it grows.  Calls 2 and 4 grow the
    partials behind the queued calls 1 and 1-3; call 5 grows the tables and
    both staging buffers behind 1-4 and runs on the partials call 4 left.  The
    second catchment series must equal the first byte for byte."""
    import torch

    ny, nx, cid, nc = catch_map("scatter32")
    assert (ny, nx, nc) == (NY, NX, 32)
    n = ny * nx
    z = bare_ice_inputs(SEED, ny, nx)[0]["elev"]
    assert np.array_equal(z, z.astype(np.float32).astype(np.float64))  # both engines hold this raster
    gA, gD = grid_of("A"), grid_of("D")
    assert (gA.gny * gA.gnx, gD.gny * gD.gnx) == (35, 16800)
    runoff, melt, snow = (int_planes(n, DEPTH, 300 + i) for i in range(3))  # M_total, SM, h_snow
    # the windows: every one wraps the ring, the B64 one ends in a short batch of its two slots per launch
    w_series, w_b7, w_b64, w_coarse, w_agg = (5, 8), (3, 8), (6, 5), (2, 8), (7, 6)

    def bands(planes, edges, first, count):
        got = ring(planes, first, count)
        return {"sum": np.stack([band_fsum(cid, z, edges, p, nc) for p in got]),
                "count": np.stack([band_count(cid, z, edges, p, THR, nc) for p in got]),
                "cells": band_cells(cid, z, edges, nc)}

    def nodes(g, planes, first, count):
        got = ring(planes, first, count)
        return {"sum": bin_exact(g, ny, nx, got), "count": counts_of(g, ny, nx, got, THR), "cells": coarse_cells(g, ny, nx)}

    folded = np.stack(ring(runoff, *w_agg)).astype(np.float32 if engine == "float32" else np.float64)  # max, min: the engine's
    want = {
        "series": np.stack([np.bincount(cid, weights=p.astype(np.float64), minlength=nc) for p in ring(runoff, *w_series)]),
        "b7": bands(melt, B7, *w_b7), "b64": bands(melt, B64, *w_b64),
        "A": nodes(gA, snow, *w_coarse), "D": nodes(gD, snow, *w_coarse),
        "agg": {"sum": folded.astype(np.float64).sum(axis=0), "max": folded.max(axis=0), "min": folded.min(axis=0),
                "above": (folded.astype(np.float64) > THR).sum(axis=0).astype(np.int32)},
    }
    assert want["series"].any()
    for key in ("b7", "b64", "A", "D", "agg"):
        for k, a in want[key].items():
            assert a.any(), (key, k)  # nothing below compares zeros with zeros

    def outs(count, *tail):
        return {"sum": torch.full((count, *tail), -1.0, dtype=torch.float64, device="cuda:0"),
                "count": torch.full((count, *tail), -1, dtype=torch.int64, device="cuda:0"),
                "cells": torch.full(tail, -1, dtype=torch.int64, device="cuda:0")}

    with reader_engine(engine, cid, nc, z) as e:
        for name, planes in (("M_total", runoff), ("SM", melt), ("h_snow", snow)):
            plant(e, name, planes)
        eng_dtype = {"float32": torch.float32, "float64": torch.float64}[engine]
        series = [torch.full((w_series[1], nc), -1.0, dtype=torch.float64, device="cuda:0") for _ in range(2)]
        b7, b64, devA = outs(w_b7[1], nc, 7), outs(w_b64[1], nc, 64), outs(w_coarse[1], gA.gny, gA.gnx)
        agg = {"sum": torch.full((n,), -1.0, dtype=torch.float64, device="cuda:0"),
               "max": torch.full((n,), -1.0, dtype=eng_dtype, device="cuda:0"),
               "min": torch.full((n,), -1.0, dtype=eng_dtype, device="cuda:0"),
               "above": torch.full((n,), -1, dtype=torch.int32, device="cuda:0")}
        hostA = e.coarse_series("h_snow", gA, first=w_coarse[0], count=w_coarse[1], threshold=THR)               # 0
        e.catchment_series("M_total", first=w_series[0], count=w_series[1], out=series[0])                        # 1
        e.band_series("SM", B7, first=w_b7[0], count=w_b7[1], threshold=THR, out=b7)                              # 2
        e.coarse_series("h_snow", gA, first=w_coarse[0], count=w_coarse[1], threshold=THR, out=devA)             # 3
        e.band_series("SM", B64, first=w_b64[0], count=w_b64[1], threshold=THR, out=b64)                          # 4
        hostD = e.coarse_series("h_snow", gD, first=w_coarse[0], count=w_coarse[1], threshold=THR)               # 5
        e.cell_aggregate("M_total", first=w_agg[0], count=w_agg[1], sum=agg["sum"], max=agg["max"], min=agg["min"],
                         above=agg["above"], threshold=THR, init=True)                                           # 6
        e.catchment_series("M_total", first=w_series[0], count=w_series[1], out=series[1])                        # 7
        e.sync()
        got = {"series": series[0].cpu().numpy(), "b7": {k: t.cpu().numpy() for k, t in b7.items()},
               "b64": {k: t.cpu().numpy() for k, t in b64.items()}, "A": {k: t.cpu().numpy() for k, t in devA.items()},
               "agg": {k: t.cpu().numpy() for k, t in agg.items()}}
        again = series[1].cpu().numpy()
    np.testing.assert_array_equal(got["series"], want["series"])
    assert again.tobytes() == got["series"].tobytes()
    for key, res in (("b7", got["b7"]), ("b64", got["b64"]), ("A", got["A"]), ("A", hostA), ("D", hostD), ("agg", got["agg"])):
        assert sorted(res) == sorted(want[key]), key
        for k, a in res.items():
            assert a.dtype == want[key][k].dtype and a.shape == want[key][k].shape, (key, k, a.dtype, a.shape)
            np.testing.assert_array_equal(a, want[key][k], err_msg=f"{key} {k}")
