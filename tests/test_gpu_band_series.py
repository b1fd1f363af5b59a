"""Per-catchment, per-elevation-band sums, counts and cells of the history
planes reduced on the device (k_band_series, k_series_reduce,
k_band_reduce_int; tfg_band_series), through GlacierEngine.band_series,
GlacierEngine.hypsometry and bands.banded_run: the kernel against the planes
it read in all three batch classes, the one-key and the many-key path, the
edge semantics of the key, slot independence and the ring, repeatability, the
threshold, NaN containment, several chunks per workgroup and shards, split
launches, device outputs, the errors of the interface, and the band profiles
against the numpy oracle.

Inputs.  tests/test_gpu_diagnostics.py's workload (bare_ice_inputs on 37 x 100
cells: 15 chunks with a ragged tail, seed 4, 24 frames, 20 steps) and its
catchment maps.  Its elevation raster is fp32-exact and spans 1502.99 to
2999.84 m.  Band layouts: B7 = linspace(1600, 2900, 8) (248 cells below the
first edge, 248 at or above the last, every band at least 433 cells), B64 =
linspace(1600, 2900, 65) (every band at least 36 cells; every full wave of 64
cells holds 31 to 43 distinct bands, counted with tests/band_ref.py) and the
single band [1000, 4000].  These, and
test_gpu_catchment_series.check_series_preconditions, are asserted on the CPU
before any GPU value is looked at.

References.  tests/band_ref.py: the key rule in numpy and math.fsum binning,
so the summation error is the kernels' alone.
  the kernel    the planes it read (get_field of each slot, of elev and of
                catch_id): sums within 1e-13 relative, absolute where the
                reference is 0 (the project's bound for this fp64
                reassociation: a chain under 900 dependent additions; here it
                is 6 + 4 * chunks per workgroup + workgroups / 16 + 4);
                counts and cells exactly equal.
  profiles      the numpy oracle's per-cell outputs binned the same way: fp32
                forms within 1e-5, the fp64 engine within 1e-12, of the
                array's largest entry (floored form).

Keys per launch (batch classes of csrc/tfg_bands.hpp): tail x B64 = 128 and
scatter64 x B7 = 448 keys run 8 slots per launch, runs x B64 = 576 and
scatter16 x B64 = 1024 keys 4, scatter32 x B64 = 2048 keys (the cap) 2.

Measured on an MI355X (TFG_REPORT_DIR/band_series.json; MEASURED below holds
the same figures), the largest error of each kind:
  the kernel against its planes, all maps, layouts and fields   fp32 2.1e-16
      (its fp32 values mostly add exactly in fp64), fp32_flux64 0, fp64 3.2e-16
  one key per wave (ramp) and many (random)        fp32 0, fp64 3.2e-16
  placed edge cells 2.1e-16 / 2.0e-16; the ring (hist_depth 8) 0 / 2.3e-16;
      NaN run, the other entries 1.6e-16 / 2.5e-16 (fp32 / fp64); split 0
  1152 x 2048, 2048 keys: slots 0 / 11 against the planes 2.2e-16 / 2.2e-16; the
      whole against its two halves 2.1e-16
  profiles against the oracle (floored)   fp32 5.6e-8, fp32_flux64 3.2e-8,
      fp64 2.8e-16
Counts and cells were equal everywhere.  No figure is within a factor of 150
of its bound.
"""

import contextlib
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from tests.band_ref import band_cells, band_count, band_fsum, band_keys, band_of
from tests.harness import BASE_CFG, make_engine
from tests.test_gpu_catchment_series import _oracle_outputs, check_series_preconditions
from tests.test_gpu_diagnostics import (FORMS, FUSE, NFRAMES, NSTEPS, NX, NY, SEED, _oracle, _report, _scatter, catch_map,
                                        floored_err, rel_err)

pytestmark = pytest.mark.gpu

# Measured on an MI355X: the largest error of each kind (bounds: 1e-13 for the
# kernel against its planes, 1e-5 / 1e-12 for the profiles against the oracle).
MEASURED = {
    "planes": {"fp32": 2.1e-16, "fp32_flux64": 0.0, "fp64": 3.2e-16},
    "one_key": {"fp32": 0.0, "fp64": 3.2e-16},
    "edges": {"fp32": 2.1e-16, "fp64": 2.0e-16},
    "ring": {"fp32": 0.0, "fp64": 2.3e-16},
    "nan": {"fp32": 1.6e-16, "fp64": 2.5e-16},
    "split": {"fp32": 0.0},
    "many_chunks": {"slot0_vs_plane": 2.2e-16, "slot11_vs_plane": 2.2e-16, "whole_vs_halves": 2.1e-16},
    "profiles_floored": {"fp32": 5.6e-8, "fp32_flux64": 3.2e-8, "fp64": 2.8e-16},
}

FIELDS = ("h_snow", "SM", "h_ice", "IM", "M_total", "RH")
DEPTH = 24
B7 = np.linspace(1600.0, 2900.0, 8)
B64 = np.linspace(1600.0, 2900.0, 65)
B1 = np.array([1000.0, 4000.0])
LAYOUTS = {"B7": B7, "B64": B64, "B1": B1}
REPORT: dict = {}


def _note(kind, key, value):
    REPORT.setdefault(kind, {})[key] = value
    _report("band_series", REPORT)


def wave_keys(key):
    """Distinct keys (cells in no band left out) of each wave of 64 cells."""
    return [len(set(w[w >= 0].tolist())) for w in (key[i:i + 64] for i in range(0, key.size, 64))]


@functools.lru_cache(maxsize=None)
def check_band_preconditions():
    """What the layouts promise, on the CPU alone."""
    check_series_preconditions()
    z = _oracle(NY, NX, SEED, NSTEPS).static["elev"]
    assert np.array_equal(z, z.astype(np.float32).astype(np.float64))  # fp32-exact: both engines hold the same raster
    assert 1502.9 < z.min() < 1503.1 and 2999.7 < z.max() < 2999.9
    assert int((z < B7[0]).sum()) == 248 and int((z >= B7[-1]).sum()) == 248
    assert band_cells(None, z, B7, 1).min() >= 433
    assert band_cells(None, z, B64, 1).min() >= 36
    per_wave = wave_keys(band_keys(None, z, B64)[0])[:NY * NX // 64]  # the full waves
    assert min(per_wave) >= 31 and max(per_wave) <= 43, (min(per_wave), max(per_wave))
    assert int(band_cells(None, z, B1, 1)[0, 0]) == NY * NX
    return z


def named_map(name):
    """catch_map, plus "none": no raster, one catchment."""
    if name == "none":
        return NY, NX, None, 1
    return catch_map(name)


@contextlib.contextmanager
def band_engine(orc, form, cid, n_catch, hist_depth, elev=None, split=None):
    """test_gpu_catchment_series.history_engine with an elevation raster of the test's own."""
    opt = FORMS[form]
    e = make_engine(BASE_CFG, orc.ny, orc.nx, opt.get("engine", "float32"), n_frames=NFRAMES, hist_depth=hist_depth,
                    n_catch=n_catch, fuse_steps=FUSE, flux=opt.get("flux", "fp32"), split=split)
    try:
        e.set_field("elev", orc.static["elev"] if elev is None else elev)
        for k in ("slope", "aspect"):
            e.set_field(k, orc.static[k])
        for k in ("h_snow", "h_ice", "h_swe", "h_iwe"):
            e.set_field(k, orc.static["h0_" + k[2:]])
        if cid is not None:
            e.set_field("catch_id", cid)
        e.init_state()
        for f in range(NFRAMES):
            for name in ("P", "T_air", "Hum_sp", "P_air", "uz"):
                e.set_field(name, orc.frames[name][f], index=f)
        yield e
    finally:
        e.close()


def rasters(e, has_raster=True):
    """(catch_id or None, elev) as the engine holds them."""
    cid = e.get_field("catch_id") if has_raster else None
    return cid, e.get_field("elev", dtype=e.np_dtype).astype(np.float64)


def read_planes(e, name, slots):
    return [e.get_field(name, index=int(s), dtype=e.np_dtype) for s in slots]


def check_against_planes(got, planes, cid, elev, edges, nc, thr=0.0):
    """The largest sum error of a band_series result against band_ref on the
    planes it read; counts and cells are asserted equal."""
    nb = len(edges) - 1
    want_sum = np.stack([band_fsum(cid, elev, edges, p, nc) for p in planes])
    if "sum" in got:
        assert got["sum"].shape == (len(planes), nc, nb) and got["sum"].dtype == np.float64
    if "count" in got:
        assert got["count"].dtype == np.int64
        np.testing.assert_array_equal(got["count"], np.stack([band_count(cid, elev, edges, p, thr, nc) for p in planes]))
    if "cells" in got:
        assert got["cells"].dtype == np.int64
        np.testing.assert_array_equal(got["cells"], band_cells(cid, elev, edges, nc))
    return rel_err(got["sum"], want_sum) if "sum" in got else 0.0, want_sum


# ------------------------------------------------------------------ 1. the kernel against the planes it read
MAP_LAYOUTS = {"scatter64": ("B7", "B1"), "runs": ("B7", "B64", "B1"), "tail": ("B7", "B64", "B1"),
               "none": ("B7", "B64", "B1"), "scatter16": ("B64",), "scatter32": ("B64",)}
PLANE_CASES = [(f, m) for f in ("fp32", "fp64") for m in MAP_LAYOUTS] + [("fp32_flux64", "scatter64")]


@pytest.mark.parametrize("form,map_name", PLANE_CASES)
def test_bands_equal_the_planes_they_read(form, map_name):
    """All six fields over all 20 slots, in every layout the map allows (keys
    per launch: module docstring), against band_ref on each slot's plane: sums
    1e-13, counts (threshold 0) and cells equal.  With the single band the
    sums also meet catchment_series at 1e-13; cells.sum(axis=1) plus the cells
    in no band is catchment_cells()."""
    check_band_preconditions()
    ny, nx, cid, nc = named_map(map_name)
    err = {}
    with band_engine(_oracle(ny, nx, SEED, NSTEPS), form, cid, nc, DEPTH) as e:
        e.run(NSTEPS)
        rcid, elev = rasters(e, cid is not None)
        planes = {name: read_planes(e, name, range(NSTEPS)) for name in FIELDS}
        for lay in MAP_LAYOUTS[map_name]:
            edges = LAYOUTS[lay]
            assert nc * (len(edges) - 1) <= 2048
            for name in FIELDS:
                got = e.band_series(name, edges, first=0, count=NSTEPS)
                err[f"{lay}/{name}"], want = check_against_planes(got, planes[name], rcid, elev, edges, nc)
                assert (want > 0).any(), (lay, name)  # not a comparison of zeros
                assert np.all(got["sum"][:, got["cells"] == 0] == 0.0)
                if lay == "B1":
                    series = e.catchment_series(name, first=0, count=NSTEPS)
                    err[f"{lay}/{name}/series"] = rel_err(got["sum"][:, :, 0], series)
            cells = e.hypsometry(edges)
            out = np.bincount(np.zeros(ny * nx, int) if rcid is None else rcid, weights=(band_of(elev, edges) < 0).astype(np.float64), minlength=nc)
            np.testing.assert_array_equal(cells.sum(axis=1) + out.astype(np.int64), e.catchment_cells())
            assert e.hypsometry(edges) is cells  # cached
    _note("planes", f"{form}/{map_name}", max(err.values()))
    print(f"band series vs planes {form} {map_name}: {max(err.values()):.2e}")
    assert max(err.values()) <= 1e-13, err


# ------------------------------------------------------------------ 2. one key per wave
@pytest.mark.parametrize("form", ["fp32", "fp64"])
def test_one_key_waves_and_many_key_waves(form):
    """A ramp by row, 1500 to 3000 m, set before init_state, without an id
    raster: with B7, 45 of the 58 waves hold one key (the fast path: the sums
    are formed before the wave's turn), 5 hold two (a wave spans two rows, and
    an edge falls between them) and 8 none (below 1600 m or at or above 2900
    m: no pass at all).  The random raster with B64 holds 31 to 43 keys in
    every full wave: the pass per key.  Both against the planes."""
    z = check_band_preconditions()
    orc = _oracle(NY, NX, SEED, NSTEPS)
    ramp = np.repeat(np.linspace(1500.0, 3000.0, NY).astype(np.float32).astype(np.float64), NX)
    hist = np.bincount(wave_keys(band_keys(None, ramp, B7)[0]), minlength=3)
    assert hist.tolist() == [8, 45, 5]
    assert min(wave_keys(band_keys(None, z, B64)[0])[:NY * NX // 64]) >= 31
    err = {}
    for label, elev, edges in (("ramp/B7", ramp, B7), ("ramp/B64", ramp, B64), ("random/B64", None, B64)):
        with band_engine(orc, form, None, 1, DEPTH, elev=elev) as e:
            e.run(NSTEPS)
            _, held = rasters(e, False)
            assert np.array_equal(held, z if elev is None else elev)
            for name in ("M_total", "h_snow", "RH"):
                got = e.band_series(name, edges, first=0, count=NSTEPS)
                err[f"{label}/{name}"], want = check_against_planes(got, read_planes(e, name, range(NSTEPS)), None, held,
                                                                    edges, 1)
                assert (want > 0).any()
    _note("one_key", form, err)
    assert max(err.values()) <= 1e-13, err


# ------------------------------------------------------------------ 3. edge semantics on the device
E3 = np.array([1600.0, 2000.2, 2250.0, 2900.0])
AT_EDGE, AT_LAST, AT_2000_2, AT_NAN = 70, 71, 200, 333  # cells (none of them bare: cell % 3 != 0)


@pytest.mark.parametrize("form", ["fp32", "fp64"])
def test_edges_on_the_device(form):
    """Cells placed at 2250.0 (an fp32-exact interior edge: the upper band in
    both engines), at edges[n_bands] = 2900.0 (excluded), at 2000.2 with an
    edge at 2000.2 (the fp32 engine holds 2000.199951171875: the lower band;
    the fp64 engine 2000.2: the upper) and, in the fp32 engine, at NaN (its
    outputs are NaN; no sum is NaN; cells and count do not see it)."""
    z = check_band_preconditions().copy()
    z[AT_EDGE], z[AT_LAST], z[AT_2000_2] = 2250.0, 2900.0, 2000.2
    if form == "fp32":
        z[AT_NAN] = np.nan
    orc = _oracle(NY, NX, SEED, NSTEPS)
    with band_engine(orc, form, None, 1, DEPTH, elev=z) as e:
        e.run(NSTEPS)
        _, held = rasters(e, False)
        b = band_of(held, E3)
        assert b[AT_EDGE] == 2 and b[AT_LAST] == -1
        assert held[AT_2000_2] == (2000.199951171875 if form == "fp32" else 2000.2)
        assert b[AT_2000_2] == (0 if form == "fp32" else 1)
        planes = read_planes(e, "M_total", range(NSTEPS))
        got = e.band_series("M_total", E3, first=0, count=NSTEPS, threshold=-np.inf)
        if form == "fp32":
            assert np.isnan(held[AT_NAN]) and b[AT_NAN] == -1
            assert all(np.isnan(p[AT_NAN]) for p in planes)  # the cell's outputs are NaN
            assert np.isnan(np.stack(planes)).sum() == NSTEPS  # and no other cell's
            assert np.isfinite(got["sum"]).all()
        err, want = check_against_planes(got, planes, None, held, E3, 1, thr=-np.inf)
        assert (want > 0).any()
        # the placed cells, one by one: moving one to the other side of its edge moves one cell between bands
        moved = held.copy()
        moved[AT_2000_2] = 2000.2 if form == "fp32" else 2000.199951171875
        d = band_cells(None, moved, E3, 1) - got["cells"]
        assert d.tolist() == [[-1, 1, 0]] if form == "fp32" else d.tolist() == [[1, -1, 0]]
        assert int(got["cells"].sum()) == int((b >= 0).sum())
        np.testing.assert_array_equal(got["count"], np.broadcast_to(got["cells"], got["count"].shape))
    _note("edges", form, err)
    assert err <= 1e-13


# ------------------------------------------------------------------ 4. slot independence and the ring
@pytest.mark.parametrize("form", ["fp32", "fp64"])
def test_a_slots_entries_do_not_depend_on_their_company(form):
    """hist_depth 8, 20 steps: slot 4 holds step 12.  One call over the ring
    from slot 4 (wrapping) equals, bit for bit in sum and exactly in count,
    eight one-slot calls and the rows of a call that starts elsewhere -- with
    8 slots (scatter64 x B7), 4 (scatter16 x B64) and 2 (scatter32 x B64) per
    launch -- and meets the planes."""
    check_band_preconditions()
    orc = _oracle(NY, NX, SEED, NSTEPS)
    err = {}
    for map_name, edges in (("scatter64", B7), ("scatter16", B64), ("scatter32", B64)):
        _, _, cid, nc = catch_map(map_name)
        with band_engine(orc, form, cid, nc, 8) as e:
            e.run(NSTEPS)
            whole = e.band_series("M_total", edges, first=4, count=8)
            dflt = e.band_series("M_total", edges)
            assert all(np.array_equal(whole[k], dflt[k]) for k in whole)  # the defaults: the last 8 steps in order
            for j in range(8):
                one = e.band_series("M_total", edges, first=(4 + j) % 8, count=1)
                assert one["sum"].shape == (1, nc, len(edges) - 1)
                assert np.array_equal(one["sum"][0], whole["sum"][j]), (map_name, j)
                assert np.array_equal(one["count"][0], whole["count"][j]) and np.array_equal(one["cells"], whole["cells"])
            other = e.band_series("M_total", edges, first=7, count=5)  # rows 3..7 of `whole`, batched otherwise
            assert np.array_equal(other["sum"], whole["sum"][3:8]) and np.array_equal(other["count"], whole["count"][3:8])
            only = e.band_series("M_total", edges, first=4, count=8, want=("sum",))  # the other outputs left out
            assert list(only) == ["sum"] and np.array_equal(only["sum"], whole["sum"])
            rcid, elev = rasters(e)
            err[map_name], want = check_against_planes(whole, read_planes(e, "M_total", [(4 + j) % 8 for j in range(8)]),
                                                       rcid, elev, edges, nc)
            assert (want > 0).any() and not np.array_equal(whole["sum"][0], whole["sum"][7])
    _note("ring", form, err)
    assert max(err.values()) <= 1e-13, err


# ------------------------------------------------------------------ 5. repeatability
def test_two_identical_calls_give_identical_bytes():
    check_band_preconditions()
    _, _, cid, nc = catch_map("scatter32")
    with band_engine(_oracle(NY, NX, SEED, NSTEPS), "fp32", cid, nc, DEPTH) as e:
        e.run(NSTEPS)
        for name in FIELDS:
            a = e.band_series(name, B64, first=0, count=NSTEPS)
            b = e.band_series(name, B64, first=0, count=NSTEPS)
            assert (a["sum"] > 0).any()
            for k in ("sum", "count", "cells"):
                assert a[k].tobytes() == b[k].tobytes(), (name, k)


# ------------------------------------------------------------------ 6. threshold
def test_the_threshold_is_strict_and_minus_infinity_counts_every_cell():
    """A threshold equal to a value present in the plane does not count that
    value (>), the next double below it does; -inf counts every cell."""
    check_band_preconditions()
    _, _, cid, nc = catch_map("runs")
    with band_engine(_oracle(NY, NX, SEED, NSTEPS), "fp32", cid, nc, DEPTH) as e:
        e.run(NSTEPS)
        rcid, elev = rasters(e)
        plane = read_planes(e, "h_snow", [10])[0]
        inside = band_of(elev, B7) >= 0
        v = float(np.median(plane[inside & (plane > 0)]))
        v = float(plane[inside][np.argmin(np.abs(plane[inside] - v))])  # a value of a cell in a band
        same = int(((plane == v) & inside).sum())
        assert same >= 1
        at = e.band_series("h_snow", B7, first=10, count=1, threshold=v, want=("count", "cells"))
        below = e.band_series("h_snow", B7, first=10, count=1, threshold=float(np.nextafter(v, -np.inf)), want=("count",))
        check_against_planes(at, [plane], rcid, elev, B7, nc, thr=v)
        assert int(below["count"].sum() - at["count"].sum()) == same
        assert 0 < at["count"].sum() < at["cells"].sum()
        every = e.band_series("h_snow", B7, first=0, count=NSTEPS, threshold=-np.inf, want=("count",))
        np.testing.assert_array_equal(every["count"], np.broadcast_to(at["cells"], every["count"].shape))


# ------------------------------------------------------------------ 7. NaN containment
@pytest.mark.parametrize("form", ["fp32", "fp64"])
def test_nan_stays_in_its_slot_catchment_and_band(form):
    """P = NaN at (step 5, cell 100): the M_total sums are NaN exactly in that
    cell's (catchment, band) from step 5 on; every other entry meets the
    bound; the count at threshold -inf is the cells minus the NaN-valued
    ones."""
    z = check_band_preconditions()
    _, _, cid, nc = catch_map("runs")
    step, cell = 5, 100
    hit = (int(cid[cell]), int(band_of(z, B7)[cell]))
    assert hit[1] >= 0
    with band_engine(_oracle(NY, NX, SEED, NSTEPS, nan=(step, cell)), form, cid, nc, DEPTH) as e:
        e.run(NSTEPS)
        rcid, elev = rasters(e)
        planes = read_planes(e, "M_total", range(NSTEPS))
        got = e.band_series("M_total", B7, first=0, count=NSTEPS, threshold=-np.inf)
    nan_cells = np.stack([band_count(rcid, elev, B7, np.isnan(p).astype(np.float64), 0.5, nc) for p in planes])
    want_nan = nan_cells > 0
    assert want_nan[step:, hit[0], hit[1]].all() and want_nan.sum() == NSTEPS - step  # the planes: that key alone, from that step on
    np.testing.assert_array_equal(np.isnan(got["sum"]), want_nan)
    np.testing.assert_array_equal(got["count"], got["cells"][None] - nan_cells)
    want = np.stack([band_fsum(rcid, elev, B7, p, nc) for p in planes])
    err = rel_err(got["sum"][~want_nan], want[~want_nan])
    _note("nan", form, err)
    assert (want[~want_nan] > 0).any() and err <= 1e-13


# ------------------------------------------------------------------ 8. several chunks per workgroup, shards
BIG_NY, BIG_NX, BIG_STEPS, BIG_SEED, BIG_NC = 1152, 2048, 12, 5, 32


def _big_bands(ny, row0, planes=()):
    from topoflow_glacier.synthetic import diurnal_table

    e = make_engine(BASE_CFG, ny, BIG_NX, "float32", n_frames=BIG_STEPS, hist_depth=BIG_STEPS, n_catch=BIG_NC,
                    fuse_steps=FUSE, row0=row0, split="off")
    try:
        cid = _scatter(np.arange(ny * BIG_NX) + row0 * BIG_NX, BIG_NC)
        e.fill_synthetic(BIG_SEED, diurnal_table(BIG_STEPS), nx_global=BIG_NX)
        e.set_field("catch_id", cid)
        e.run(BIG_STEPS)
        got = e.band_series("M_total", B64, first=0, count=BIG_STEPS, threshold=1e-9)
        rcid, elev = rasters(e)
        ref = {s: SimpleNamespace(sum=band_fsum(rcid, elev, B64, p, BIG_NC), count=band_count(rcid, elev, B64, p, 1e-9, BIG_NC))
               for s in planes for p in read_planes(e, "M_total", [s])}
        return SimpleNamespace(got=got, ref=ref, cells=band_cells(rcid, elev, B64, BIG_NC) if planes else None)
    finally:
        e.close()


def test_many_chunks_per_workgroup_and_shards():
    """1152 x 2048 cells, 32 scattered ids x B64 = 2048 keys: 9216 chunks over
    the 1170 workgroups that the scratch cap leaves (7.9 chunks each), 12 slots
    two per launch.  Slots 0 and 11 meet the planes; the two 576-row halves,
    run as shards, add to the whole: sums within 1e-13, integers equal."""
    whole = _big_bands(BIG_NY, 0, planes=(0, 11))
    err = {}
    for s in (0, 11):
        assert (whole.ref[s].sum > 0).any() and 0 < whole.ref[s].count.sum() < whole.cells.sum()
        err[f"slot{s}_vs_plane"] = rel_err(whole.got["sum"][s], whole.ref[s].sum)
        np.testing.assert_array_equal(whole.got["count"][s], whole.ref[s].count)
    np.testing.assert_array_equal(whole.got["cells"], whole.cells)
    assert whole.cells.min() > 0 and whole.cells.sum() < BIG_NY * BIG_NX  # every key used, some cells in no band
    halves = [_big_bands(BIG_NY // 2, 0), _big_bands(BIG_NY // 2, BIG_NY // 2)]
    err["whole_vs_halves"] = rel_err(whole.got["sum"], halves[0].got["sum"] + halves[1].got["sum"])
    for k in ("count", "cells"):
        np.testing.assert_array_equal(whole.got[k], halves[0].got[k] + halves[1].got[k])
    _note("many_chunks", "fp32", err)
    print(f"band series, many chunks per workgroup: {err}")
    assert max(err.values()) <= 1e-13, err


# ------------------------------------------------------------------ 9. split launches
def test_right_after_a_split_launch():
    """split ON: band_series straight after run(), without join(), equals the planes."""
    check_band_preconditions()
    _, _, cid, nc = catch_map("scatter64")
    with band_engine(_oracle(NY, NX, SEED, NSTEPS), "fp32", cid, nc, DEPTH, split="on") as e:
        assert e.is_split()
        e.run(NSTEPS)
        got = e.band_series("M_total", B7, first=0, count=NSTEPS)  # no sync(), no join()
        rcid, elev = rasters(e)
        err, want = check_against_planes(got, read_planes(e, "M_total", range(NSTEPS)), rcid, elev, B7, nc)
    _note("split", "fp32", err)
    assert (want > 0).any() and err <= 1e-13


# ------------------------------------------------------------------ 10. device outputs
def test_device_outputs_hold_the_host_result():
    import torch

    check_band_preconditions()
    _, _, cid, nc = catch_map("runs")
    with band_engine(_oracle(NY, NX, SEED, NSTEPS), "fp32", cid, nc, DEPTH) as e:
        e.run(NSTEPS)
        host = e.band_series("SM", B64, first=3, count=13, threshold=1e-9)
        assert (host["sum"] > 0).any() and 0 < host["count"].sum()
        dev = "cuda:0"
        out = {"sum": torch.full((13, nc, 64), -1.0, dtype=torch.float64, device=dev),
               "count": torch.full((13, nc, 64), -1, dtype=torch.int64, device=dev),
               "cells": torch.full((nc, 64), -1, dtype=torch.int64, device=dev)}
        assert e.band_series("SM", B64, first=3, count=13, threshold=1e-9, out=out) is out
        e.sync()
        for k in out:
            assert out[k].cpu().numpy().tobytes() == host[k].tobytes(), k
        part = {"count": torch.full((13, nc, 64), -1, dtype=torch.int64, device=dev)}
        e.band_series("SM", B64, first=3, count=13, threshold=1e-9, out=part)
        e.sync()
        assert np.array_equal(part["count"].cpu().numpy(), host["count"])
        for bad in ({"sum": out["sum"].float()}, {"sum": out["sum"][:, :, :-1]}, {"count": out["sum"]},
                    {"cells": out["count"]}, {"sum": out["sum"].cpu()}, {"mean": out["sum"]}, {}):
            with pytest.raises(ValueError):
                e.band_series("SM", B64, first=3, count=13, out=bad)


# ------------------------------------------------------------------ 11. errors
def test_bad_arguments_write_nothing_and_leave_the_handle_usable():
    """Every TFG_ERR_ARG case of include/tfg.h, through ctypes: the outputs,
    prefilled with a sentinel, come back unchanged, and the run that follows
    equals that of a handle that saw none of them."""
    from topoflow_glacier import _native as nat

    ny, nx, nc = 5, NX, 40
    orc = _oracle(ny, nx, SEED, NSTEPS)
    cid = _scatter(np.arange(ny * nx), nc)
    L = nat.load()
    fid = nat.FIELD["M_total"]
    good = np.ascontiguousarray(B7)

    def ten_more(e):
        e.run(10)
        r = e.band_series("M_total", B7)
        return r["sum"], r["count"], r["cells"], e.get_field("M_total", dtype=np.float32), e.get_field("h_swe")

    def bands(edges, n_bands=None, thr=0.0):
        a = np.ascontiguousarray(edges, dtype=np.float64)
        b = nat.TfgBands(len(a) - 1 if n_bands is None else n_bands, 0, a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), thr)
        b._keep = a
        return b

    with band_engine(orc, "fp32", cid, nc, 8) as e:
        e.run(10)
        s = np.full((8, nc, 64), -7.0)
        c = np.full((8, nc, 64), -7, dtype=np.int64)
        n = np.full((nc, 64), -7, dtype=np.int64)
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        inf_edge, nan_edge, flat, down = good.copy(), good.copy(), good.copy(), good.copy()
        inf_edge[-1], nan_edge[2], flat[3], down[4] = np.inf, np.nan, good[2], good[3] - 1.0
        null_edges = nat.TfgBands(7, 0, None, 0.0)
        cases = {
            "null bands": (fid, 0, 1, None, ptr(s), ptr(c), ptr(n)),
            "null edges": (fid, 0, 1, ctypes.byref(null_edges), ptr(s), ptr(c), ptr(n)),
            "no output": (fid, 0, 1, ctypes.byref(bands(good)), None, None, None),
            "no bands": (fid, 0, 1, ctypes.byref(bands(good, n_bands=0)), ptr(s), ptr(c), ptr(n)),
            "65 bands": (fid, 0, 1, ctypes.byref(bands(np.arange(66.0), n_bands=65)), ptr(s), ptr(c), ptr(n)),
            "2080 keys": (fid, 0, 1, ctypes.byref(bands(np.arange(53.0))), ptr(s), ptr(c), ptr(n)),  # 40 x 52
            "inf edge": (fid, 0, 1, ctypes.byref(bands(inf_edge)), ptr(s), ptr(c), ptr(n)),
            "nan edge": (fid, 0, 1, ctypes.byref(bands(nan_edge)), ptr(s), ptr(c), ptr(n)),
            "equal edges": (fid, 0, 1, ctypes.byref(bands(flat)), ptr(s), ptr(c), ptr(n)),
            "descending": (fid, 0, 1, ctypes.byref(bands(down)), ptr(s), ptr(c), ptr(n)),
            "nan threshold": (fid, 0, 1, ctypes.byref(bands(good, thr=np.nan)), ptr(s), ptr(c), ptr(n)),
            "state field": (nat.FIELD["h_swe"], 0, 1, ctypes.byref(bands(good)), ptr(s), ptr(c), ptr(n)),
            "input field": (nat.FIELD["P"], 0, 1, ctypes.byref(bands(good)), ptr(s), ptr(c), ptr(n)),
            "hist0 < 0": (fid, -1, 1, ctypes.byref(bands(good)), ptr(s), ptr(c), ptr(n)),
            "hist0 = depth": (fid, 8, 1, ctypes.byref(bands(good)), ptr(s), ptr(c), ptr(n)),
            "no slots": (fid, 0, 0, ctypes.byref(bands(good)), ptr(s), ptr(c), ptr(n)),
            "9 slots": (fid, 0, 9, ctypes.byref(bands(good)), ptr(s), ptr(c), ptr(n)),
            "cells only, bad field": (nat.FIELD["P"], 0, 1, ctypes.byref(bands(good)), None, None, ptr(n)),
            "cells only, 9 slots": (fid, 0, 9, ctypes.byref(bands(good)), None, None, ptr(n)),
        }
        for what, (f, h0, ns, b, ps, pc, pn) in cases.items():
            assert L.tfg_band_series(e.h, f, h0, ns, b, ps, pc, pn, 0) == nat.ERR_ARG, what
            assert (s == -7.0).all() and (c == -7).all() and (n == -7).all(), what
        with pytest.raises(nat.NativeError, match="band series") as ei:
            e.band_series("M_total", B7, threshold=np.nan)
        assert ei.value.code == nat.ERR_ARG
        # what is allowed: 40 x 51 = 2040 keys; a NaN threshold without count; cells alone
        ok = e.band_series("M_total", np.linspace(1600.0, 2900.0, 52), threshold=np.nan, want=("sum", "cells"))
        assert ok["sum"].shape == (8, nc, 51) and (ok["sum"] > 0).any()
        got = ten_more(e)
    with band_engine(orc, "fp32", cid, nc, 8) as e:
        e.run(10)
        want = ten_more(e)
    assert (want[0] > 0).any()
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------ 12. the profiles against the oracle
@pytest.mark.parametrize("form", ["fp32", "fp32_flux64", "fp64"])
def test_band_profiles_against_the_oracle(form):
    """banded_run over 20 steps on a ring of 8 (blocks of 8, 8 and 4), periods
    of 7 steps (7, 7, 6), map `runs` x B7: the per-band SM, IM and M_total sums
    against the numpy oracle's per-cell outputs binned by band_ref; melt_depth,
    mean and cells follow from them."""
    from topoflow_glacier.bands import banded_run, snow_line

    z = check_band_preconditions()
    _, _, cid, nc = catch_map("runs")
    out = _oracle_outputs(NY, NX)
    orc = _oracle(NY, NX, SEED, NSTEPS)
    with band_engine(orc, form, cid, nc, 8) as e:
        res = banded_run(e, NSTEPS, 7, B7, ("SM", "IM", "M_total", "h_snow"), threshold={"h_snow": 0.0})
        assert e.step_index == NSTEPS
    assert res["periods"].tolist() == [7, 7, 6]
    cells = band_cells(cid, z, B7, nc)
    np.testing.assert_array_equal(res["cells"], cells)
    err = {}
    for name in ("SM", "IM", "M_total"):
        want = np.stack([band_fsum(cid, z, B7, out[name][a:b], nc) for a, b in ((0, 7), (7, 14), (14, 20))])
        assert (want > 0).any(), name
        err[name] = floored_err(res["fields"][name]["sum"], want)
    _note("profiles_floored", form, err)
    print(f"band profiles vs oracle {form}: {err}")
    assert max(err.values()) <= (1e-12 if form == "fp64" else 1e-5), err
    melt = res["fields"]["SM"]["sum"] + res["fields"]["IM"]["sum"]
    assert np.array_equal(res["melt_depth"], np.where(cells > 0, melt * (BASE_CFG["dt"] * 3600.0) / np.maximum(cells, 1), 0.0))
    frac = res["fields"]["h_snow"]["fraction"]
    assert ((frac >= 0) & (frac <= 1)).all() and (frac > 0).any()
    assert snow_line(frac, B7).shape == (3, nc)
