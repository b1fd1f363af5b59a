"""Time one 24-frame tfg_set_gridded_forcing call (k_forcing_regrid, three
batches of eight frames) on the fp32 engine at 8192^2 cells under a 257 x 257
source grid (one node per 32 cells): plain bilinear, plain nearest and bilinear
with every downscaling term on, from a device source; interleaved in one
process with tfg_set_catchment_forcing on the same engine (bench.py's 43 + 1
block catchments), plain and with every term on, which writes the same planes.
Beside them the host route the call replaces, at 4096^2: the numpy
restatement (tests/regrid_ref.py) of a frame plus set_inputs, per frame.
Diagnostic only.
  python tests/diagnostics/gridded_forcing_timing.py [--size 8192] [--host-size 4096] [--reps 10] [--rounds 5] [--out result.json]"""
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
from tests import regrid_ref as G  # noqa: E402
from tests.harness import BASE_CFG, make_engine  # noqa: E402
from topoflow_glacier.forcing import Downscale, ForcingGrid  # noqa: E402
from topoflow_glacier.sharding import allreduce_catchment_elevation  # noqa: E402
from topoflow_glacier.synthetic import diurnal_table  # noqa: E402

FRAMES, BATCH, CELLS_PER_NODE = 24, 8, 32
HOST_FRAMES = 2  # frames of the host route that are timed (scaled to 24)
RANGES = ((70000.0, 80000.0), (0.002, 0.006), (0.0, 2e-7), (-12.0, 6.0), (0.5, 9.0))  # P_air, Hum_sp, P, T_air, uz

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=8192)
ap.add_argument("--host-size", type=int, default=4096)
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


def source(size, rng):
    g = size // CELLS_PER_NODE + 1
    src = np.empty((FRAMES, 5, g, g))
    for v, (lo, hi) in enumerate(RANGES):
        src[:, v] = rng.uniform(lo, hi, (FRAMES, g, g))
    return g, src


ALL_ON = Downscale(lapse_T=-0.0065, grad_P=2e-4, pressure=1, rh_max=1.0)
rng = np.random.default_rng(3)
size = a.size
n = size * size
cid, nc = bench.catchment_blocks(0, size, size, size, 43), 44
e = make_engine(dict(BASE_CFG), size, size, "float32", n_frames=FRAMES, hist_depth=1, n_catch=nc, fuse_steps=FRAMES, split="off")
e.fill_synthetic(7, diurnal_table(FRAMES), nx_global=size)
e.set_field("catch_id", cid)
elev = e.get_field("elev", dtype=np.float32)
z_ref = allreduce_catchment_elevation(*e.catchment_mean_elevation())
g, src = source(size, rng)
z_src = rng.uniform(float(elev.min()), float(elev.max()), (g, g))
table = np.empty((FRAMES, 5, nc))
for v, (lo, hi) in enumerate(RANGES):
    table[:, v] = rng.uniform(lo, hi, (FRAMES, nc))
dev = e.torch_device
src_d, z_src_d = torch.from_numpy(src).to(dev), torch.from_numpy(z_src).to(dev)
table_d, z_ref_d = torch.from_numpy(table).to(dev), torch.from_numpy(np.asarray(z_ref, dtype=np.float64)).to(dev)
grids = {m: ForcingGrid(gny=g, gnx=g, y0=0.0, x0=0.0, sy=1 / CELLS_PER_NODE, sx=1 / CELLS_PER_NODE, method=m)
         for m in ("bilinear", "nearest")}
cases = {
    "gridded_bilinear": lambda: e.set_gridded_forcing(src_d, grids["bilinear"]),
    "gridded_nearest": lambda: e.set_gridded_forcing(src_d, grids["nearest"]),
    "gridded_bilinear_downscaled": lambda: e.set_gridded_forcing(src_d, grids["bilinear"], z_src=z_src_d, downscale=ALL_ON),
    "catchment_gather": lambda: e.set_catchment_forcing(table_d),
    "catchment_downscaled": lambda: e.set_catchment_forcing(table_d, z_ref=z_ref_d, downscale=ALL_ON),
}
times = {k: [] for k in cases}
for _ in range(a.rounds):  # cases interleaved, one process
    for k, fn in cases.items():
        times[k].append(clocked(fn, e, a.reps))
e.sync()
# the tensors the engine read carry its stream (Tensor.record_stream): free them while that stream exists
del src_d, z_src_d, table_d, z_ref_d
torch.cuda.empty_cache()
e.close()
del e
nbytes = FRAMES * n * 20  # the planes written
rows = {}
for k, ts in times.items():
    med = float(np.median(ts))
    rows[k] = {"ms_median": med * 1e3, "ms_min": float(np.min(ts)) * 1e3, "GBps_written": nbytes / med / 1e9}
for k, base in (("gridded_bilinear", "catchment_gather"), ("gridded_nearest", "catchment_gather"),
                ("gridded_bilinear_downscaled", "catchment_downscaled")):
    rows[k]["over_" + base] = rows[k]["ms_median"] / rows[base]["ms_median"]
for k, r in rows.items():
    print(json.dumps({k: r}), flush=True)

# the host route at --host-size: a frame interpolated by numpy (the restatement) and uploaded, frame by frame
hs = a.host_size
gh, src_h = source(hs, rng)
e = make_engine(dict(BASE_CFG), hs, hs, "float32", n_frames=FRAMES, hist_depth=1, fuse_steps=FRAMES, split="off")
gr = ForcingGrid(gny=gh, gnx=gh, y0=0.0, x0=0.0, sy=1 / CELLS_PER_NODE, sx=1 / CELLS_PER_NODE, method="bilinear")
src_hd = torch.from_numpy(src_h).to(dev)
t_call = clocked(lambda: e.set_gridded_forcing(src_hd, gr), e, a.reps)
t0 = time.perf_counter()
for f in range(HOST_FRAMES):
    e.set_inputs(G.interpolate(src_h[f], gr, hs, hs), index=f)
e.sync()
host_s = (time.perf_counter() - t0) / HOST_FRAMES * FRAMES
del src_hd
torch.cuda.empty_cache()
e.close()
host = {"grid": [hs, hs], "source": [gh, gh], "host_route_ms": host_s * 1e3, "gridded_bilinear_ms": t_call * 1e3,
        "host_route_over_call": host_s / t_call}
print(json.dumps({"host_route": host}), flush=True)
res = {"what": "one 24-frame call per case (device sources), fp32 engine, split off; host clock around a sync after warm-up; "
               "cases interleaved over rounds in one process, median and min of the rounds; GBps_written counts the planes "
               f"written (24 x n x 20 B) alone; host route: numpy restatement + set_inputs, {HOST_FRAMES} frames timed, scaled to 24",
       "device": torch.cuda.get_device_name(0), "grid": [size, size], "source": [g, g], "n_catch": nc, "frames": FRAMES,
       "reps": a.reps, "rounds": a.rounds, "algorithmic_bytes": nbytes, "cases": rows, "host_route": host}
if a.out:
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
