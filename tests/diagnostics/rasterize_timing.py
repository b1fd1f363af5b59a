"""Time GlacierEngine.rasterize_divides (tfg_rasterize_polygons, k_rasterize)
over the 43 divides of tests/golden/hydrofabric_12082500.npz on grids of 4096^2
and 8192^2 cells, the cell size chosen so that the divides span the grid's
width, beside
  * the host route it replaces: hydrofabric.rasterize_divides + catchment_ids
    + set_field("catch_id"), once, by the host clock;
  * a hipMemsetAsync of the same 4-byte-per-cell plane: the write stream alone.
The device call and the memset are timed with device events on the engine's
stream (median of --reps after a warm-up); the call's host side (building the
tables, staging them) is given by the host clock around a call that waits for
the counts.  The device raster is compared with the host route's.  Diagnostic only.
  python tests/diagnostics/rasterize_timing.py [--sizes 4096,8192] [--reps 10] [--out profiles/rasterize.json]"""
import argparse
import ctypes
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "topoflow-glacier_amd"), str(ROOT / "oracle")]
import torch  # noqa: E402  (one HIP runtime: torch's)

from tests.harness import BASE_CFG, GOLDEN, make_engine  # noqa: E402
from topoflow_glacier import _native as nat  # noqa: E402
from topoflow_glacier import hydrofabric as hf  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="4096,8192")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--no-host", action="store_true", help="skip the host route (minutes of CPU time at 8192^2)")
ap.add_argument("--out", default=None)
a = ap.parse_args()

hip = ctypes.CDLL("libamdhip64.so")  # the runtime torch has loaded
hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
_, dv = hf.load_divides_npz(GOLDEN / "hydrofabric_12082500.npz")
xs = np.concatenate([r[:, 0] for d in dv for p in d.polygons for r in p])


def covering(size):
    """(cell, x0, y0, ny, nx): the largest grid_covering of the divides with nx, ny <= size."""
    cell = (xs.max() - xs.min()) / (size - 2)
    while True:
        x0, y0, ny, nx = hf.grid_covering(dv, cell)
        if max(ny, nx) <= size:
            return cell, x0, y0, ny, nx
        cell *= 1.0005


def event_ms(fn, stream, reps):
    """Median device milliseconds of what fn queues on `stream`, after one warm-up."""
    fn()
    stream.synchronize()
    ms = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        fn()
        t1.record(stream)
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    return float(np.median(ms)), float(np.min(ms))


rows = []
for size in (int(s) for s in a.sizes.split(",")):
    n = size * size
    cell, x0, y0, gny, gnx = covering(size)
    nc = len(dv) + 1
    e = make_engine(dict(BASE_CFG), size, size, "float32", n_frames=1, hist_depth=1, n_catch=nc, split="off")
    stream = torch.cuda.ExternalStream(e.stream(), device=torch.device("cuda", e.device))
    t = hf.polygon_tables(dv, x0, y0, cell, size, size)
    # the library call on tables built once: between the events the host only validates and stages them
    ptr = lambda v: v.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    p = nat.TfgPolygons(len(t.poly_id), ptr(t.poly_id), ptr(t.poly_ring0), ptr(t.poly_box), len(t.ring_edge0) - 1,
                        ptr(t.ring_edge0), ptr(t.edges), ptr(t.px), ptr(t.py))
    dev_ms, dev_min = event_ms(lambda: nat.check(e.lib.tfg_rasterize_polygons(e.h, ctypes.byref(p), nc - 1, None), e.h),
                               stream, a.reps)
    t0 = time.perf_counter()
    cells = e.rasterize_divides(dv, x0, y0, cell)
    call_host_ms = (time.perf_counter() - t0) * 1e3
    plane = torch.empty(n, dtype=torch.int32, device=f"cuda:{e.device}")
    set_ms, set_min = event_ms(lambda: hip.hipMemsetAsync(plane.data_ptr(), 0, n * 4, e.stream()), stream, a.reps)
    row = {"grid": [size, size], "cell_m": cell, "covering": [gny, gnx], "polygons": int(len(t.poly_id)),
           "edges": int(t.ring_edge0[-1]), "outside_share": float(cells[-1] / n), "device_ms_median": dev_ms,
           "device_ms_min": dev_min, "call_with_counts_host_clock_ms": call_host_ms, "memset_ms_median": set_ms,
           "memset_ms_min": set_min, "device_over_memset": dev_ms / set_ms, "plane_GBps": n * 4 / dev_ms / 1e6}
    if not a.no_host:
        got = e.get_field("catch_id")
        t0 = time.perf_counter()
        ids, nc_host = hf.catchment_ids(hf.rasterize_divides(dv, x0, y0, cell, size, size))
        t_raster = time.perf_counter() - t0
        e.set_field("catch_id", ids.reshape(-1))
        e.sync()
        host_s = time.perf_counter() - t0
        row.update(host_route_ms=host_s * 1e3, host_rasterize_ms=t_raster * 1e3, host_over_device=host_s * 1e3 / dev_ms,
                   host_over_call_with_counts=host_s * 1e3 / call_host_ms,
                   differing_cells=int(np.count_nonzero(got != ids.reshape(-1))) if nc_host == nc else -1)
    rows.append(row)
    print(json.dumps(row), flush=True)
    e.close()
    del e, plane
res = {"what": "GlacierEngine.rasterize_divides over the fixture's 43 divides, fp32 engine; device_ms: device events on the "
               "engine's stream around a queued tfg_rasterize_polygons call on tables built once (no counts), median and "
               "min of reps after a warm-up; "
               "call_with_counts: host clock around one call that builds the tables and waits for the counts; memset: "
               "hipMemsetAsync of 4 bytes per cell, same events; host route: rasterize_divides + catchment_ids + "
               "set_field('catch_id'), once, host clock",
       "device": torch.cuda.get_device_name(0), "reps": a.reps, "rows": rows}
if a.out:
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
