"""Time one 24-slot M_total cell aggregate (tfg_cell_aggregate: k_cell_aggregate,
three batches of eight slots) on the fp32 engine at 4096^2 and 8192^2 cells:
  (a) the sum alone with init, and all four statistics continuing, as device
      events on the engine's stream, with the achieved rate on the algorithmic
      bytes (csrc/tfg_aggregate.hpp);
  (b) the same calls as a share of the 24-step fused launch they follow;
  (c) the route a caller had before: get_field_device of each slot into a
      torch tensor, then torch's add (and maximum, minimum, gt), in the same
      process; both routes must agree exactly on the sum.
Diagnostic only.
  python tests/diagnostics/cell_aggregate_timing.py [--sizes 4096,8192] [--reps 20] [--out result.json]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "topoflow-glacier_amd"), str(ROOT / "oracle")]
import torch  # noqa: E402  (one HIP runtime: torch's)

from tests.harness import BASE_CFG, make_engine  # noqa: E402
from topoflow_glacier.synthetic import diurnal_table  # noqa: E402

SLOTS = 24

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="4096,8192")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=None)
a = ap.parse_args()


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def device_timed(fn, e, stream, reps, warmup=3):
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


def host_timed(fn, e, reps, warmup=1):
    """Milliseconds of each call by the host clock; fn ends in a device synchronise."""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        e.sync()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


rows = []
for size in (int(s) for s in a.sizes.split(",")):
    n = size * size
    e = make_engine(dict(BASE_CFG), size, size, "float32", n_frames=SLOTS, hist_depth=SLOTS, fuse_steps=SLOTS, split="off")
    e.fill_synthetic(7, diurnal_table(SLOTS), nx_global=size)
    stream = torch.cuda.ExternalStream(e.stream(), device=e.torch_device)
    fused = device_timed(lambda: e.run(SLOTS), e, stream, 5, warmup=1)  # the slots are then full
    dev = e.torch_device
    s = torch.zeros(n, dtype=torch.float64, device=dev)
    mx, mn = torch.zeros(n, dtype=torch.float32, device=dev), torch.zeros(n, dtype=torch.float32, device=dev)
    c = torch.zeros(n, dtype=torch.int32, device=dev)

    def sum_init():
        e.cell_aggregate("M_total", first=0, count=SLOTS, sum=s, init=True)

    def all_continue():
        e.cell_aggregate("M_total", first=0, count=SLOTS, sum=s, max=mx, min=mn, above=c, init=False)

    t_sum, t_all = [], []
    for _ in range(2):  # the two forms alternate
        t_sum += device_timed(sum_init, e, stream, a.reps // 2)
        t_all += device_timed(all_continue, e, stream, a.reps // 2)
    sum_init()
    e.sync()
    kernel_sum = s.clone()

    # the route without the kernel: a device copy of each slot, then torch
    tmp = torch.empty(n, dtype=torch.float32, device=dev)
    ts = torch.zeros(n, dtype=torch.float64, device=dev)
    tmx, tmn = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
    tc = torch.zeros(n, dtype=torch.int32, device=dev)

    def torch_sum():
        ts.zero_()
        for j in range(SLOTS):
            e.get_field_device("M_total", tmp, index=j)
            ts.add_(tmp)

    def torch_all():
        for j in range(SLOTS):
            e.get_field_device("M_total", tmp, index=j)
            ts.add_(tmp)
            torch.maximum(tmx, tmp, out=tmx)
            torch.minimum(tmn, tmp, out=tmn)
            tc.add_(tmp.gt(0.0))

    r_sum = host_timed(torch_sum, e, max(a.reps // 4, 3))
    torch_sum()
    torch.cuda.synchronize()
    agree = bool(torch.equal(ts, kernel_sum))
    e.get_field_device("M_total", tmx, index=0)
    tmn.copy_(tmx)
    r_all = host_timed(torch_all, e, max(a.reps // 4, 3))

    b_sum = n * (SLOTS * 4 + 8)                   # the planes; the sum written, not read (init)
    b_all = n * (SLOTS * 4 + 16 + 8 + 8 + 8)      # the planes; sum, vmax, vmin, count read and written
    ms_sum, ms_all, ms_fused = statistics.median(t_sum), statistics.median(t_all), statistics.median(fused)
    rows.append({
        "grid": [size, size], "slots": SLOTS,
        "sum_init": {**spread(t_sum), "algorithmic_bytes": b_sum, "TBps": b_sum / (ms_sum * 1e-3) / 1e12,
                     "share_of_fused": ms_sum / ms_fused},
        "all_four_continue": {**spread(t_all), "algorithmic_bytes": b_all, "TBps": b_all / (ms_all * 1e-3) / 1e12,
                              "share_of_fused": ms_all / ms_fused},
        "fused_24_steps": spread(fused),
        "torch_route_sum": {**spread(r_sum), "over_kernel": statistics.median(r_sum) / ms_sum},
        "torch_route_all_four": {**spread(r_all), "over_kernel": statistics.median(r_all) / ms_all},
        "sum_equal_bit_for_bit": agree,
    })
    print(json.dumps(rows[-1]), flush=True)
    assert agree, "the two routes differ on the sum"
    e.close()
    del e, s, mx, mn, c, tmp, ts, tmx, tmn, tc, kernel_sum
    torch.cuda.empty_cache()
res = {"what": "one 24-slot M_total tfg_cell_aggregate call, fp32 engine, split off; device events on the engine's stream "
               "after warm-up; the torch route by the host clock around device synchronises",
       "device": torch.cuda.get_device_name(0), "rows": rows}
if a.out:
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
