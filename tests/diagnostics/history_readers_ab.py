"""A/B of the history readers' host path (catchment_series, band_series,
coarse_series, cell_aggregate) between two builds of this project, for a change
that leaves the kernels alone (scripts/kernel_diff.py: 0 differ).

  host     the host-clock time of --calls queued device-output calls of each
           reader plus one final sync, per call [us], on the 37 x 100 fp32
           engine with 32 catchments, 7 bands and 5 x 9 nodes; median of
           --reps.  It times the checkout it lies in (a copy of this file in
           the parent commit's checkout times the parent):
             python tests/diagnostics/history_readers_ab.py host --out run/host.json
  verdict  reads three run directories (parent, this tree, parent again, taken
           in that order in one session on one device; a fourth, the parent
           once more, is judged in the tree's place by the same rule: what an
           identical build misses), each holding host.json
           and the --out files of catchment_series_timing.py (catchment.json),
           band_series_timing.py (band.json), coarse_series_timing.py
           (coarse.json) and cell_aggregate_timing.py (aggregate.json) at
           --sizes 4096, and writes every figure of the three runs with
             pass = tree <= max(parent1, parent2) + |parent1 - parent2|
           (the parent's own run-to-run difference is the margin):
             python tests/diagnostics/history_readers_ab.py verdict P1 TREE P2 [P3] --out profiles/history_readers_ab.json
Diagnostic only."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=("host", "verdict"))
ap.add_argument("runs", nargs="*")
ap.add_argument("--calls", type=int, default=300)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--kernel-diff", default=None, help="scripts/kernel_diff.py's summary line, recorded with the verdict")
ap.add_argument("--out", default=None)
a = ap.parse_args()


def host_figures() -> dict:
    sys.path[:0] = [str(ROOT), str(ROOT / "topoflow-glacier_amd"), str(ROOT / "oracle")]
    import numpy as np
    import torch  # (one HIP runtime: torch's)

    from tests.harness import BASE_CFG, make_engine
    from topoflow_glacier.forcing import ForcingGrid
    from topoflow_glacier.synthetic import diurnal_table

    ny, nx, depth, nc, nb = 37, 100, 8, 32, 7
    e = make_engine(dict(BASE_CFG), ny, nx, "float32", n_frames=depth, hist_depth=depth, n_catch=nc, fuse_steps=depth,
                    split="off")
    e.fill_synthetic(7, diurnal_table(depth), nx_global=nx)
    e.set_field("catch_id", ((np.arange(ny * nx, dtype=np.int64) * 7) % nc).astype(np.int32))
    e.run(depth)
    dev = e.torch_device
    z = e.get_field("elev")
    edges = np.linspace(z.min(), z.max() + 1.0, nb + 1)
    g = ForcingGrid(gny=5, gnx=9, y0=0.0, x0=0.0, sy=4 / (ny - 1), sx=8 / (nx - 1), method="nearest")
    series = torch.empty((depth, nc), dtype=torch.float64, device=dev)
    keyed = lambda *tail: {"sum": torch.empty((depth, *tail), dtype=torch.float64, device=dev),  # noqa: E731
                           "count": torch.empty((depth, *tail), dtype=torch.int64, device=dev),
                           "cells": torch.empty(tail, dtype=torch.int64, device=dev)}
    band, coarse = keyed(nc, nb), keyed(5, 9)
    acc = torch.zeros(ny * nx, dtype=torch.float64, device=dev)
    readers = {"catchment_series": lambda: e.catchment_series("M_total", first=0, count=depth, out=series),
               "band_series": lambda: e.band_series("M_total", edges, first=0, count=depth, out=band),
               "coarse_series": lambda: e.coarse_series("M_total", g, first=0, count=depth, out=coarse),
               "cell_aggregate": lambda: e.cell_aggregate("M_total", first=0, count=depth, sum=acc, init=True)}
    out = {}
    for name, fn in readers.items():
        fn()
        e.sync()
        t = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            for _ in range(a.calls):
                fn()
            e.sync()
            t.append((time.perf_counter() - t0) / a.calls * 1e6)
        out[name] = {"us": statistics.median(t), "us_min": min(t), "us_max": max(t)}
        print(name, json.dumps(out[name]), flush=True)
    e.close()
    return {"what": f"host clock of {a.calls} queued device-output calls plus one sync, per call [us], median of {a.reps}; "
                    f"{ny} x {nx} fp32 engine, {nc} catchments, {nb} bands, 5 x 9 nodes",
            "device": torch.cuda.get_device_name(0), "host_us_per_call": out}


def figures(run: Path) -> dict:
    """{figure: value} of one run directory; control/ holds the fused launch no reader touches (not judged)."""
    load = lambda name: json.loads((run / name).read_text())  # noqa: E731
    f = {f"a/host_us_per_call/{k}": v["us"] for k, v in load("host.json")["host_us_per_call"].items()}
    for r in load("catchment.json")["rows"]:
        f[f"b/catchment_series/{r['raster']}/series_ms"] = r["series_ms"]
        f[f"control/catchment_series/{r['raster']}/fused_24_steps_ms"] = r["fused_24_steps_ms"]
    for r in load("band.json")["rows"]:
        f[f"b/band_series/{r['raster']}/{r['n_bands']}/band_ms"] = r["band_ms"]
        f[f"b/band_series/{r['raster']}/{r['n_bands']}/catchment_series_ms"] = r["catchment_series_ms"]
        f["control/band_series/fused_24_steps_ms"] = r["fused_24_steps_ms"]
    for r in load("coarse.json")["rows"]:
        for form in ("sum", "sum_count", "cells", "catchment_series"):
            if form in r:
                f[f"b/coarse_series/{r['nodes'][0]}/{form}_ms"] = r[form]["ms"]
        f["control/coarse_series/fused_24_steps_ms"] = r["fused_24_steps_ms"]
    for r in load("aggregate.json")["rows"]:
        f["b/cell_aggregate/sum_init_ms"] = r["sum_init"]["median_ms"]
        f["b/cell_aggregate/all_four_continue_ms"] = r["all_four_continue"]["median_ms"]
        f["control/cell_aggregate/fused_24_steps_ms"] = r["fused_24_steps"]["median_ms"]
    return f


def judge(p1: dict, tree: dict, p2: dict, name: str = "tree") -> tuple:
    rows, failed = {}, []
    for k in sorted(tree):
        margin = abs(p1[k] - p2[k])
        rows[k] = {"parent1": p1[k], name: tree[k], "parent2": p2[k], "margin": margin}
        if not k.startswith("control/"):
            rows[k]["pass"] = tree[k] <= max(p1[k], p2[k]) + margin
            if not rows[k]["pass"]:
                failed.append(k)
    return rows, failed


def verdict() -> dict:
    p1, tree, p2, *p3 = (figures(Path(r)) for r in a.runs)
    rows, failed = judge(p1, tree, p2)
    if p3:  # the rule's own rate of misses: a third parent run judged in the tree's place
        null_rows, null_failed = judge(p1, p3[0], p2, "parent3")
        for k, r in null_rows.items():
            rows[k]["parent3"] = r["parent3"]
    host = json.loads((Path(a.runs[1]) / "host.json").read_text())
    return {"what": "the history readers' host path against the parent commit, one session on one device, run order parent, "
                    "tree, parent (tests/diagnostics/history_readers_ab.py).  a/: " + host["what"] + ".  b/: the four "
                    "tests/diagnostics/*_timing.py at --sizes 4096 [ms].  A figure passes when tree <= max(parent1, parent2) "
                    "+ |parent1 - parent2|.  control/: the same runs' 24-step fused launch, which the change does not "
                    "touch (not judged).",
            "kernel_diff": a.kernel_diff, "device": host["device"], "figures": rows, "failed": failed,
            **({"parent3_in_the_trees_place_failed": null_failed} if p3 else {})}


res = host_figures() if a.mode == "host" else verdict()
if a.mode == "verdict":
    print(json.dumps({"judged": sum("pass" in r for r in res["figures"].values()),
                      **{k: v for k, v in res.items() if k.endswith("failed")}}))
if a.out:
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
