"""Time one 24-slot M_total catchment series (tfg_catchment_series:
k_catch_series + k_series_reduce, three batches of eight slots) on the fp32
engine at 4096^2 and 8192^2 cells, with bench.py's 43 + 1 block catchments
and with 512 scattered ids, beside the same run's 24-step fused launch and
the only other route to the same numbers: get_field of each slot to the host
plus np.bincount.  Diagnostic only.
  python tests/diagnostics/catchment_series_timing.py [--sizes 4096,8192] [--reps 10] [--out result.json]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "topoflow-glacier_amd"), str(ROOT / "oracle")]
import torch  # noqa: E402  (one HIP runtime: torch's)

import bench  # noqa: E402
from tests.harness import BASE_CFG, make_engine  # noqa: E402
from topoflow_glacier.synthetic import diurnal_table  # noqa: E402

SLOTS, BATCH = 24, 8  # one call's slots; kSeriesBatch of csrc/tfg_series.hpp

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="4096,8192")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--out", default=None)
a = ap.parse_args()


def clocked(fn, e, reps):
    """Seconds per call: host clock around a sync, after one warm-up call."""
    fn()
    e.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    e.sync()
    return (time.perf_counter() - t0) / reps


rows = []
for size in (int(s) for s in a.sizes.split(",")):
    n = size * size
    rasters = {"blocks44": (bench.catchment_blocks(0, size, size, size, 43), 44),
               "scatter512": (((np.arange(n, dtype=np.int64) * 37) % 512).astype(np.int32), 512)}
    host_s = None
    for raster, (cid, nc) in rasters.items():
        e = make_engine(dict(BASE_CFG), size, size, "float32", n_frames=SLOTS, hist_depth=SLOTS, n_catch=nc,
                        fuse_steps=SLOTS, split="off")
        e.fill_synthetic(7, diurnal_table(SLOTS), nx_global=size)
        e.set_field("catch_id", cid)
        t_fused = clocked(lambda: e.run(SLOTS), e, 3)  # one 24-step fused launch (the slots it writes are then full)
        out = torch.empty((SLOTS, nc), dtype=torch.float64, device=e.torch_device)
        t_series = clocked(lambda: e.catchment_series("M_total", first=0, count=SLOTS, out=out), e, a.reps)
        got = out.cpu().numpy()
        agree = None
        if host_s is None:  # the host route costs the same for either raster: timed once per grid
            t0 = time.perf_counter()
            host = np.stack([np.bincount(cid, weights=e.get_field("M_total", index=s, dtype=np.float32), minlength=nc)
                             for s in range(SLOTS)])
            host_s = time.perf_counter() - t0
            agree = float(np.max(np.abs(got - host) / np.maximum(np.abs(host), 1e-300)))
        nbytes = SLOTS * n * 4 + (SLOTS // BATCH) * n * 4  # the planes, plus the ids once per slot batch
        rows.append({"grid": [size, size], "raster": raster, "n_catch": nc, "series_ms": t_series * 1e3,
                     "series_GBps": nbytes / t_series / 1e9, "algorithmic_bytes": nbytes,
                     "host_route_ms": host_s * 1e3, "host_route_over_series": host_s / t_series,
                     "fused_24_steps_ms": t_fused * 1e3, "series_share_of_fused": t_series / t_fused,
                     "max_rel_diff_vs_host_bincount": agree})
        print(json.dumps(rows[-1]), flush=True)
        e.close()
        del out, e
    del rasters
res = {"what": "one 24-slot M_total tfg_catchment_series call, fp32 engine, split off; host clock around a sync after warm-up",
       "device": torch.cuda.get_device_name(0), "reps": a.reps, "rows": rows}
if a.out:
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
