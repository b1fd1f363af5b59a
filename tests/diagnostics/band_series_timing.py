"""Time one 24-slot M_total band series (tfg_band_series: k_band_series +
k_series_reduce + k_band_reduce_int; sums, counts and cells) on the fp32
engine at 4096^2 and 8192^2 cells with bench.py's 43 + 1 block catchments,
with 8, 20 and 46 elevation bands (352, 880 and 2024 keys: 8, 4 and 2 slots
per launch), on two elevation rasters: the synthetic workload's uniform-random
one (tens of keys in every wave) and a smooth one, three long-wavelength
sinusoids (one key in most waves).  Beside it, in the same process: the
24-slot tfg_catchment_series call over the same planes, the 24-step fused
launch that wrote them, and the only other route to the same numbers:
get_field of each slot to the host plus np.bincount.  Device times are between
two events on the engine's stream, after warm-up, the band call and the series
call alternating.  Diagnostic only.
  python tests/diagnostics/band_series_timing.py [--sizes 4096,8192] [--reps 10] [--out profiles/band_series.json]"""
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
from tests.harness import BASE_CFG, make_engine  # noqa: E402
from topoflow_glacier.synthetic import diurnal_table  # noqa: E402

SLOTS, NC = 24, 44
BANDS = (8, 20, 46)

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="4096,8192")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--out", default=None)
a = ap.parse_args()


def batch(keys):
    """Slots per launch (band_batch of csrc/tfg_bands.hpp)."""
    return 8 if keys <= 512 else 4 if keys <= 1024 else 2


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


def smooth_raster(size, dev):
    """1500 .. 3000 m: three sinusoids, the shortest wavelength a third of the grid."""
    r = torch.arange(size, dtype=torch.float32, device=dev)[:, None] / size
    c = torch.arange(size, dtype=torch.float32, device=dev)[None, :] / size
    tau = 2.0 * np.pi
    z = 2250.0 + 400.0 * torch.sin(tau * r + 0.3) + 250.0 * torch.sin(tau * 1.5 * c) + 100.0 * torch.sin(tau * 3.0 * (r + c))
    return z.reshape(-1).contiguous()


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

    host_ms = None
    for raster in ("random", "smooth"):
        if raster == "smooth":
            e.set_field("elev", smooth_raster(size, dev))  # the keys follow; the planes stay as the steps wrote them
        for nb in BANDS:
            edges = np.linspace(1500.0, 3000.0, nb + 1)
            keys = NC * nb
            out = {"sum": torch.empty((SLOTS, NC, nb), dtype=torch.float64, device=dev),
                   "count": torch.empty((SLOTS, NC, nb), dtype=torch.int64, device=dev),
                   "cells": torch.empty((NC, nb), dtype=torch.int64, device=dev)}

            def bands():
                e.band_series("M_total", edges, first=0, count=SLOTS, threshold=0.0, out=out)

            t_band, t_series = [], []
            for _ in range(2):  # the two calls alternate
                t_band += device_timed(bands, e, stream, a.reps // 2)
                t_series += device_timed(series, e, stream, a.reps // 2)
            band_ms, series_ms = statistics.median(t_band), statistics.median(t_series)
            agree = None
            if host_ms is None:  # the host route costs the same for every layout: timed once per grid
                t0 = time.perf_counter()
                z = e.get_field("elev", dtype=np.float32).astype(np.float64)
                k = np.searchsorted(edges, z, side="right") - 1
                ok = (k >= 0) & (k < nb)
                key = (cid.astype(np.int64) * nb + k)[ok]
                host = np.stack([np.bincount(key, weights=e.get_field("M_total", index=s, dtype=np.float32)[ok],
                                             minlength=keys) for s in range(SLOTS)]).reshape(SLOTS, NC, nb)
                host_ms = (time.perf_counter() - t0) * 1e3
                got = out["sum"].cpu().numpy()
                agree = float(np.max(np.abs(got - host) / np.maximum(np.abs(host), 1e-300)))
                assert np.array_equal(out["cells"].cpu().numpy().reshape(-1), np.bincount(key, minlength=keys))
                del z, k, ok, key, host
            nbytes = n * (4 * SLOTS + 8 * -(-SLOTS // batch(keys)))  # the planes, plus id and elevation once per batch
            rows.append({"grid": [size, size], "raster": raster, "n_catch": NC, "n_bands": nb, "keys": keys,
                         "slots_per_launch": batch(keys), "band_ms": band_ms, "band_ms_min": min(t_band),
                         "band_ms_max": max(t_band), "band_TBps": nbytes / band_ms / 1e9, "algorithmic_bytes": nbytes,
                         "catchment_series_ms": series_ms, "band_over_catchment_series": band_ms / series_ms,
                         "fused_24_steps_ms": fused, "band_share_of_fused": band_ms / fused,
                         "host_route_ms": host_ms, "host_route_over_band": host_ms / band_ms,
                         "max_rel_diff_vs_host_bincount": agree})
            print(json.dumps(rows[-1]), flush=True)
            del out
    e.close()
    del e, series_out, cid
res = {"what": "one 24-slot M_total tfg_band_series call (sum, count, cells; device outputs), fp32 engine, split off; "
               "medians of device-event times on the engine's stream after warm-up, alternating with tfg_catchment_series",
       "device": torch.cuda.get_device_name(0), "reps": a.reps, "rows": rows}
if a.out:
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
