"""Time one 24-slot M_total coarse series (tfg_coarse_series: k_coarse_series +
k_coarse_fold, k_coarse_cells) on the fp32 engine at 8192^2 and 4096^2 cells
after a 24-step fused launch, in one process:
  (a) under 257 x 257 nodes (the gridded-forcing profile's grid), in three
      forms: sums only, sums with counts, cells only;
  (b) the same under 33 x 33 nodes and under one node: row runs of 256 rows
      and of the whole grid, cut into segments;
  (c) alternating with (a): the 24-slot tfg_catchment_series call over the
      same slots on the same handle (bench.py's 43 + 1 block catchments);
  (d) the host route to the same numbers: get_field of a slot plus np.add.at,
      timed on --host-planes slots and scaled to 24.
Device times are between two events on the engine's stream, after warm-up, the
outputs on the device.  The yardstick is the sums-only call of (a) against
(c): it reads 8/9 of (c)'s bytes (no id raster) and adds a pass over partials.
Diagnostic only.
  python tests/diagnostics/coarse_series_timing.py [--sizes 8192,4096] [--nodes 257,33,1] [--reps 10] [--host-planes 4]
                                                   [--out profiles/coarse_series.json]
With TFG_LIB naming a library built with -DTFG_COARSE_SEG_ROWS=N the same script times another segment length."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "topoflow-glacier_amd"), str(ROOT / "oracle")]
import torch  # noqa: E402  (one HIP runtime: torch's)

import bench  # noqa: E402
from tests.coarse_ref import coarse_key  # noqa: E402
from tests.harness import BASE_CFG, make_engine  # noqa: E402
from topoflow_glacier.forcing import ForcingGrid  # noqa: E402
from topoflow_glacier.synthetic import diurnal_table  # noqa: E402

SLOTS, NC = 24, 44
NODES = (257, 33, 1)

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="8192,4096")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--host-planes", type=int, default=4)
ap.add_argument("--nodes", default=",".join(map(str, NODES)))
ap.add_argument("--out", default=None)
a = ap.parse_args()


def device_timed(fn, e, stream, reps, warmup=2):
    """Milliseconds of each of `reps` calls between two events on the engine's stream."""
    for _ in range(warmup):
        fn()
    e.sync()
    out = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        fn()
        t1.record(stream)
        e.sync()
        out.append(t0.elapsed_time(t1))
    return out


def stats(ms):
    return {"ms": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}


rows = []
for size in (int(s) for s in a.sizes.split(",")):
    n = size * size
    cid = bench.catchment_blocks(0, size, size, size, NC - 1)
    e = make_engine(dict(BASE_CFG), size, size, "float32", n_frames=SLOTS, hist_depth=SLOTS, n_catch=NC, fuse_steps=SLOTS,
                    split="off")
    e.fill_synthetic(7, diurnal_table(SLOTS), nx_global=size)
    e.set_field("catch_id", cid)
    dev = e.torch_device
    stream = torch.cuda.ExternalStream(e.stream(), device=dev)
    fused = statistics.median(device_timed(lambda: e.run(SLOTS), e, stream, 3, warmup=1))  # the slots are then full
    series_out = torch.empty((SLOTS, NC), dtype=torch.float64, device=dev)

    def series():
        e.catchment_series("M_total", first=0, count=SLOTS, out=series_out)

    plane_bytes = n * 4 * SLOTS            # what the coarse series reads: each plane element once
    series_bytes = n * (4 * SLOTS + 4 * 3)  # the catchment series: the planes, plus the id raster once per batch of 8
    for nodes in (int(s) for s in a.nodes.split(",")):
        g = ForcingGrid(gny=nodes, gnx=nodes, y0=0.0, x0=0.0, sy=(nodes - 1) / (size - 1), sx=(nodes - 1) / (size - 1),
                        method="nearest")
        out = {"sum": torch.empty((SLOTS, nodes, nodes), dtype=torch.float64, device=dev),
               "count": torch.empty((SLOTS, nodes, nodes), dtype=torch.int64, device=dev),
               "cells": torch.empty((nodes, nodes), dtype=torch.int64, device=dev)}
        forms = {"sum": {"sum": out["sum"]}, "sum_count": {"sum": out["sum"], "count": out["count"]},
                 "cells": {"cells": out["cells"]}}
        row = {"grid": [size, size], "nodes": [nodes, nodes], "fused_24_steps_ms": fused}
        t_series = []
        for form, o in forms.items():
            def coarse():
                e.coarse_series("M_total", g, first=0, count=SLOTS, threshold=0.0, out=o)

            t = []
            for _ in range(2):  # the two calls alternate
                t += device_timed(coarse, e, stream, a.reps // 2)
                if nodes == 257:
                    t_series += device_timed(series, e, stream, a.reps // 2)
            row[form] = stats(t)
            if form != "cells":
                row[form]["TBps_algorithmic"] = plane_bytes / row[form]["ms"] / 1e9
        row["algorithmic_bytes"] = plane_bytes
        if t_series:
            row["catchment_series"] = dict(stats(t_series), algorithmic_bytes=series_bytes,
                                           TBps_algorithmic=series_bytes / statistics.median(t_series) / 1e9)
            row["sum_over_catchment_series"] = row["sum"]["ms"] / row["catchment_series"]["ms"]
        if t_series and a.host_planes > 0:  # (d) the host route, and the device result against it
            key = coarse_key(g, size, size)
            t0 = time.perf_counter()
            host = np.zeros((a.host_planes, nodes * nodes))
            for s in range(a.host_planes):
                np.add.at(host[s], key, e.get_field("M_total", index=s, dtype=np.float32))
            host_ms = (time.perf_counter() - t0) * 1e3
            e.coarse_series("M_total", g, first=0, count=SLOTS, threshold=0.0, out=forms["sum_count"])
            e.sync()
            got = out["sum"][:a.host_planes].cpu().numpy().reshape(a.host_planes, -1)
            row["host_route"] = {"planes_timed": a.host_planes, "ms": host_ms, "ms_scaled_to_24": host_ms * SLOTS / a.host_planes,
                                 "scaled_over_sum": host_ms * SLOTS / a.host_planes / row["sum"]["ms"],
                                 "max_rel_diff_vs_add_at": float(np.max(np.abs(got - host) / np.maximum(np.abs(host), 1e-300)))}
            del key, host
        rows.append(row)
        print(json.dumps(row), flush=True)
        del out, forms
    e.close()
    del e, series_out, cid
res = {"what": "one 24-slot M_total tfg_coarse_series call (device outputs), fp32 engine, split off; medians of device-event "
               "times on the engine's stream after warm-up; under 257 x 257 nodes alternating with tfg_catchment_series "
               "(44 catchments) over the same slots on the same handle",
       "device": torch.cuda.get_device_name(0), "reps": a.reps, "rows": rows}
if a.out:
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
