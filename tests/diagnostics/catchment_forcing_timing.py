"""Time one 24-frame tfg_set_catchment_forcing call (k_forcing_expand, three
batches of eight frames) on the fp32 engine at 4096^2 and 8192^2 cells with
bench.py's 43 + 1 block catchments: the plain gather and the full downscaling,
each with 16-byte stores (four cells per lane) and with one cell per lane
(TFG_FORCING_CELLS=1), interleaved in one process; beside the same run's
24-step fused launch and the host route the call replaces: building [5][n] on
the host plus set_inputs, per frame.  Diagnostic only.
  python tests/diagnostics/catchment_forcing_timing.py [--sizes 4096,8192] [--reps 10] [--rounds 5] [--out result.json]"""
import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "topoflow-glacier_amd"), str(ROOT / "oracle")]
import torch  # noqa: E402  (one HIP runtime: torch's)

import bench  # noqa: E402
from tests.harness import BASE_CFG, make_engine  # noqa: E402
from topoflow_glacier.forcing import Downscale  # noqa: E402
from topoflow_glacier.sharding import allreduce_catchment_elevation  # noqa: E402
from topoflow_glacier.synthetic import diurnal_table  # noqa: E402

FRAMES, BATCH = 24, 8  # one call's frames; kForcingBatch of csrc/tfg_forcing.hpp
HOST_FRAMES = 3        # frames of the host route that are timed (scaled to 24)

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="4096,8192")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
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
    cid, nc = bench.catchment_blocks(0, size, size, size, 43), 44
    e = make_engine(dict(BASE_CFG), size, size, "float32", n_frames=FRAMES, hist_depth=FRAMES, n_catch=nc,
                    fuse_steps=FRAMES, split="off")
    e.fill_synthetic(7, diurnal_table(FRAMES), nx_global=size)
    e.set_field("catch_id", cid)
    t_fused = clocked(lambda: e.run(FRAMES), e, 3)  # one 24-step fused launch
    z_ref = allreduce_catchment_elevation(*e.catchment_mean_elevation())
    rng = np.random.default_rng(3)
    table = np.empty((FRAMES, 5, nc))  # P_air, Hum_sp, P, T_air, uz
    for v, (lo, hi) in enumerate(((70000.0, 80000.0), (0.002, 0.006), (0.0, 2e-7), (-12.0, 6.0), (0.5, 9.0))):
        table[:, v] = rng.uniform(lo, hi, (FRAMES, nc))
    modes = {"gather": None, "downscaled": Downscale(lapse_T=-0.0065, grad_P=2e-4, pressure=1, rh_max=1.0)}
    times = {(m, w): [] for m in modes for w in ("16B", "1cell")}
    for _ in range(a.rounds):  # variants interleaved, one process
        for (m, w), ts in times.items():
            os.environ["TFG_FORCING_CELLS"] = "1" if w == "1cell" else "0"
            ts.append(clocked(lambda: e.set_catchment_forcing(table, z_ref=z_ref, downscale=modes[m]), e, a.reps))
    os.environ.pop("TFG_FORCING_CELLS", None)
    # the host route: [5][n] built on the host and uploaded, frame by frame
    t0 = time.perf_counter()
    for f in range(HOST_FRAMES):
        e.set_inputs(table[f][:, cid], index=f)
    e.sync()
    host_s = (time.perf_counter() - t0) / HOST_FRAMES * FRAMES
    nbytes = FRAMES * n * 20 + (FRAMES // BATCH) * n * 8  # the planes written, the id and elevation once per batch
    for (m, w), ts in times.items():
        med, best = float(np.median(ts)), float(np.min(ts))
        rows.append({"grid": [size, size], "n_catch": nc, "mode": m, "stores": w, "ms_median": med * 1e3, "ms_min": best * 1e3,
                     "GBps": nbytes / med / 1e9, "algorithmic_bytes": nbytes, "fused_24_steps_ms": t_fused * 1e3,
                     "share_of_fused": med / t_fused, "host_route_ms": host_s * 1e3, "host_route_over_call": host_s / med})
        print(json.dumps(rows[-1]), flush=True)
    e.close()
    del e
res = {"what": "one 24-frame tfg_set_catchment_forcing call (host table), fp32 engine, split off; host clock around a sync "
               "after warm-up; variants interleaved over rounds in one process, median and min of the rounds; host route: "
               f"{HOST_FRAMES} frames timed, scaled to 24",
       "device": torch.cuda.get_device_name(0), "reps": a.reps, "rounds": a.rounds, "rows": rows}
if a.out:
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
