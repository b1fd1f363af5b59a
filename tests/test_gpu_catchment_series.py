"""Per-catchment, per-step sums of the history planes reduced on the device
(k_catch_series, k_series_reduce; tfg_catchment_series), through
GlacierEngine.catchment_series and hydrograph.catchment_hydrographs: the
kernel against the planes it read, slot independence and the ring, the
hydrograph against the numpy oracle, several chunks per workgroup with split
launches and shards, NaN containment and the edges of the interface.

Inputs.  tests/harness.py:bare_ice_inputs on 37 x 100 cells (15 chunks, a
ragged tail), seed 4, 24 frames, 20 steps (tests/test_gpu_diagnostics.py's
workload, whose catchment maps and helpers are used here).  Asserted on the
numpy oracle before any GPU value is looked at: no cell's h_swe crosses zero
in the 20 steps; each of the six history fields has a positive domain sum at
every step; with scatter64, 1278 of the 1280 (step, catchment) runoff entries
are positive; the `tail` catchment's runoff is positive in 18 steps.

References.  Every reference sum over a catchment is math.fsum
(harness.catchment_fsum), so the summation error is the kernels' alone.
  the kernel    the planes it read (get_field of each slot): relative error
                <= 1e-13, absolute where the reference is 0 -- the bound the
                diagnostics tests hold the same fp64 reassociation of
                non-negative terms to; it covers any order whose longest chain
                of dependent additions stays under 900 terms (900 * 2^-53 =
                1e-13), and these kernels' chain is 6 + 4 * chunks per
                workgroup + workgroups / 16 + 4.
  hydrograph    the numpy oracle's per-cell M_total per step, times da_m2:
                fp32 forms within 1e-5, the fp64 engine within 1e-12, of the
                array's largest entry (floored form).

Measured on an MI355X (TFG_REPORT_DIR/catchment_series.json; MEASURED below
holds the same figures), the largest error of each kind:
  the kernel against its planes, all maps and fields   fp32 2.1e-16 (its fp32
      values mostly add exactly in fp64), fp32_flux64 0, fp64 3.1e-16
  the ring (hist_depth 8) against its planes            fp32 2.1e-16, fp64 2.2e-16
  hydrograph against the oracle (floored)               fp32 4.4e-8, fp32_flux64
      3.4e-8, fp64 2.9e-16 (elementwise relative: 2.5e-7, 6.4e-8, 1.5e-15)
  1152 x 2048, 512 ids: slots 0 / 11 against the planes 2.2e-16 / 1.8e-16; the
      whole against its two halves 2.4e-16
No figure is within a factor of 200 of its bound.
"""

import contextlib
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from tests.harness import BASE_CFG, catchment_fsum, make_engine, oracle_run
from tests.test_gpu_diagnostics import (FORMS, FUSE, NFRAMES, NSTEPS, NX, NY, SEED, _oracle, _report, _scatter, catch_map,
                                        check_preconditions, floored_err, rel_err)

pytestmark = pytest.mark.gpu

# Measured on an MI355X: the largest error of each kind (bounds: 1e-13 for the
# kernel against its planes, 1e-5 / 1e-12 for the hydrograph against the oracle).
MEASURED = {
    "planes": {"fp32": 2.1e-16, "fp32_flux64": 0.0, "fp64": 3.1e-16},
    "ring": {"fp32": 2.1e-16, "fp64": 2.2e-16},
    "hydrograph_floored": {"fp32": 4.4e-8, "fp32_flux64": 3.4e-8, "fp64": 2.9e-16},
    "many_chunks": {"slot0_vs_plane": 2.2e-16, "slot11_vs_plane": 1.8e-16, "whole_vs_halves": 2.4e-16},
}

FIELDS = ("h_snow", "SM", "h_ice", "IM", "M_total", "RH")
DA_M2 = BASE_CFG["da"] * 1e6
DEPTH = 24
REPORT: dict = {}


@functools.lru_cache(maxsize=None)
def _oracle_outputs(ny, nx):
    """The numpy oracle's six history fields per step, [20][ncell] each
    (read-only), on the inputs of test_gpu_diagnostics._oracle."""
    orc = _oracle(ny, nx, SEED, NSTEPS)
    idx = np.arange(NSTEPS) % NFRAMES
    out, _ = oracle_run(BASE_CFG, orc.static, {k: v[idx] for k, v in orc.frames.items()}, NSTEPS)
    res = {k: np.asarray(out[k], dtype=np.float64) for k in FIELDS}
    for v in res.values():
        v.setflags(write=False)
    return res


def check_series_preconditions(ny=NY, nx=NX):
    """What the comparisons below stand on, on the CPU oracle alone."""
    orc = _oracle(ny, nx, SEED, NSTEPS)
    check_preconditions(orc)
    out = _oracle_outputs(ny, nx)
    for name in FIELDS:
        assert out[name].shape == (NSTEPS, ny * nx) and np.isfinite(out[name]).all()
        assert (out[name].sum(axis=1) > 0).all(), name  # a positive domain sum at every step
    return out


def oracle_runoff(cid, n_catch, ny=NY, nx=NX):
    """[20][n_catch] the oracle's runoff per step and catchment [m3 s-1]."""
    m = _oracle_outputs(ny, nx)["M_total"]
    return np.stack([catchment_fsum(cid, m[k], n_catch) for k in range(NSTEPS)]) * DA_M2


@contextlib.contextmanager
def history_engine(orc, form, cid, n_catch, hist_depth, fuse=FUSE, split=None):
    """An initialised engine with a history ring, holding an oracle run's
    inputs, in a kernel form (test_gpu_diagnostics.engine_on with a depth)."""
    opt = FORMS[form]
    e = make_engine(BASE_CFG, orc.ny, orc.nx, opt.get("engine", "float32"), n_frames=NFRAMES, hist_depth=hist_depth,
                    n_catch=n_catch, fuse_steps=fuse, flux=opt.get("flux", "fp32"), split=split)
    try:
        for k in ("elev", "slope", "aspect"):
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


def plane_sums(e, name, slots, cid, n_catch):
    """[len(slots)][n_catch] exactly rounded sums of the planes in `slots`, read back."""
    dt = np.float32 if e.engine == "float32" else np.float64
    return np.stack([catchment_fsum(cid, e.get_field(name, index=int(s), dtype=dt), n_catch) for s in slots])


def _note(kind, key, value):
    REPORT.setdefault(kind, {})[key] = value
    _report("catchment_series", REPORT)


# ------------------------------------------------------------------ 1. the kernel against the planes it read
PLANE_CASES = [(f, m) for f in ("fp32", "fp64") for m in ("scatter64", "scatter512", "runs", "holes", "tail")] \
    + [("fp32_flux64", "scatter64")]


@pytest.mark.parametrize("form,map_name", PLANE_CASES)
def test_series_equals_the_planes_it_read(form, map_name):
    """All six fields over all 20 slots (three batches: 8, 8 and 4 slots)
    against catchment_fsum of each slot's plane as get_field returns it:
    1e-13 relative, absolute where the reference is 0; a catchment without
    cells reads exactly 0."""
    ny, nx, cid, nc = catch_map(map_name)
    check_series_preconditions(ny, nx)
    if map_name == "scatter64":
        assert int((oracle_runoff(cid, nc) > 0).sum()) == 1278 and nc * NSTEPS == 1280
    if map_name == "tail":
        assert int((oracle_runoff(cid, nc)[:, 1] > 0).sum()) == 18
    empty = np.bincount(cid, minlength=nc) == 0
    err = {}
    with history_engine(_oracle(ny, nx, SEED, NSTEPS), form, cid, nc, DEPTH) as e:
        e.run(NSTEPS)
        for name in FIELDS:
            got = e.catchment_series(name, first=0, count=NSTEPS)
            want = plane_sums(e, name, range(NSTEPS), cid, nc)
            assert got.shape == (NSTEPS, nc) and got.dtype == np.float64
            assert (want > 0).any(), name  # not a comparison of zeros
            err[name] = rel_err(got, want)
            assert np.all(got[:, empty] == 0.0), name
    _note("planes", f"{form}/{map_name}", err)
    print(f"catchment series vs planes {form} {map_name}: {err}")
    assert max(err.values()) <= 1e-13, err
    if map_name == "holes":
        assert empty.sum() >= 12


# ------------------------------------------------------------------ 2. slot independence, the ring
@pytest.mark.parametrize("form", ["fp32", "fp64"])
def test_a_slots_row_does_not_depend_on_its_company(form):
    """series(f, s, 1) is row s of the 20-slot call bit for bit (s = 0: first
    of a batch; 7: last of a full batch; 19: last of a short batch), and so is
    a call that starts a batch elsewhere."""
    _, _, cid, nc = catch_map("scatter64")
    with history_engine(_oracle(NY, NX, SEED, NSTEPS), form, cid, nc, DEPTH) as e:
        e.run(NSTEPS)
        for name in FIELDS:
            whole = e.catchment_series(name, first=0, count=NSTEPS)
            assert (whole > 0).any()
            for s in (0, 7, 19):
                one = e.catchment_series(name, first=s, count=1)
                assert one.shape == (1, nc)
                assert np.array_equal(one[0], whole[s]), (name, s)
            assert np.array_equal(e.catchment_series(name, first=5, count=11), whole[5:16]), name
        assert np.array_equal(e.catchment_series(), e.catchment_series("M_total", first=0, count=NSTEPS))


@pytest.mark.parametrize("form", ["fp32", "fp64"])
def test_the_ring_reads_back_in_step_order(form):
    """hist_depth = 8: after 20 steps slot 4 holds step 12, and
    catchment_series(first=4, count=8) is steps 12..19 in order -- against the
    planes as in test 1, and bit for bit rows 12..19 of an engine that kept all
    20 steps; the default arguments give the same rows."""
    _, _, cid, nc = catch_map("runs")
    orc = _oracle(NY, NX, SEED, NSTEPS)
    with history_engine(orc, form, cid, nc, DEPTH) as e:
        e.run(NSTEPS)
        full = {name: e.catchment_series(name, first=0, count=NSTEPS) for name in FIELDS}
    err = {}
    with history_engine(orc, form, cid, nc, 8) as e:
        e.run(NSTEPS)
        assert np.array_equal(e.catchment_series(), e.catchment_series("M_total", first=4, count=8))
        for name in FIELDS:
            got = e.catchment_series(name, first=4, count=8)
            want = plane_sums(e, name, [(4 + j) % 8 for j in range(8)], cid, nc)
            assert (want > 0).any(), name
            err[name] = rel_err(got, want)
            assert np.array_equal(got, full[name][12:20]), name
    _note("ring", form, err)
    assert max(err.values()) <= 1e-13, err
    assert not np.array_equal(full["M_total"][12], full["M_total"][19])  # the order is visible


# ------------------------------------------------------------------ 3. hydrograph end to end
@pytest.mark.parametrize("form", ["fp32", "fp32_flux64", "fp64"])
def test_hydrograph_against_the_oracle(form):
    """catchment_hydrographs over 20 steps on a ring of 8 (blocks of 8, 8 and
    4), map `runs`: runoff against the oracle's per-cell M_total summed per
    catchment and step, times da_m2; routed = boxcar_route(runoff); bit-equal
    to one engine with hist_depth = 20 run in a single block."""
    from topoflow_glacier.hydrograph import catchment_hydrographs
    from topoflow_glacier.routing import boxcar_route

    _, _, cid, nc = catch_map("runs")
    check_series_preconditions()
    want = oracle_runoff(cid, nc)
    assert (want > 0).any(axis=1).all()  # some catchment runs off at every step
    orc = _oracle(NY, NX, SEED, NSTEPS)
    blocks = []
    with history_engine(orc, form, cid, nc, 8) as e:
        res = catchment_hydrographs(e, NSTEPS, on_block=lambda k0, k1: blocks.append((k0, k1)))
        assert e.step_index == NSTEPS
    with history_engine(orc, form, cid, nc, NSTEPS) as e:
        one = catchment_hydrographs(e, NSTEPS)
    assert blocks == [(0, 8), (8, 16), (16, 20)]
    assert res["runoff"].shape == (NSTEPS, nc) and res["runoff"].dtype == np.float64
    err = {"floored": floored_err(res["runoff"], want), "relative": rel_err(res["runoff"], want)}
    _note("hydrograph", form, err)
    print(f"catchment hydrograph vs oracle {form}: {err}")
    assert err["floored"] <= (1e-12 if form == "fp64" else 1e-5), err
    assert np.array_equal(res["routed"], boxcar_route(res["runoff"], 20))
    assert np.array_equal(res["runoff"], one["runoff"]) and np.array_equal(res["routed"], one["routed"])


# ------------------------------------------------------------------ 4. several chunks per workgroup, split launches, shards
BIG_NY, BIG_NX, BIG_STEPS, BIG_SEED, BIG_NC = 1152, 2048, 12, 5, 512


def _big_series(ny, row0, split, planes=()):
    from topoflow_glacier.synthetic import diurnal_table

    e = make_engine(BASE_CFG, ny, BIG_NX, "float32", n_frames=BIG_STEPS, hist_depth=BIG_STEPS, n_catch=BIG_NC,
                    fuse_steps=FUSE, row0=row0, split=split)
    try:
        cid = _scatter(np.arange(ny * BIG_NX) + row0 * BIG_NX, BIG_NC)
        e.fill_synthetic(BIG_SEED, diurnal_table(BIG_STEPS), nx_global=BIG_NX)
        e.set_field("catch_id", cid)
        was_split = e.is_split()
        e.run(BIG_STEPS)
        series = e.catchment_series("M_total", first=0, count=BIG_STEPS)  # right after run(): no sync()
        want = {s: catchment_fsum(cid, e.get_field("M_total", index=s, dtype=np.float32), BIG_NC) for s in planes}
        return SimpleNamespace(split=was_split, series=series, want=want)
    finally:
        e.close()


def test_many_chunks_per_workgroup_split_launches_and_shards():
    """1152 x 2048 cells with 512 scattered ids: 9216 chunks over the 2048
    workgroups 512 catchments leave (4.5 chunks each), 12 slots in batches of
    8 and 4.  The series is taken right after run(), without sync(): split
    off, on and auto are bit-equal (the call is ordered after a split launch's
    second part); slots 0 and 11 meet the planes at 1e-13; the two 576-row
    halves, run as shards, add to the whole within 1e-12."""
    wholes = {s: _big_series(BIG_NY, 0, s, planes=(0, 11) if s == "off" else ()) for s in ("off", "on", "auto")}
    assert not wholes["off"].split and wholes["on"].split and wholes["auto"].split
    off = wholes["off"]
    assert (off.want[0] > 0).any() and (off.want[11] > 0).any()  # not a comparison of zeros
    assert np.array_equal(wholes["on"].series, off.series) and np.array_equal(wholes["auto"].series, off.series)
    err = {f"slot{s}_vs_plane": rel_err(off.series[s], off.want[s]) for s in (0, 11)}
    halves = [_big_series(BIG_NY // 2, 0, "off"), _big_series(BIG_NY // 2, BIG_NY // 2, "off")]
    err["whole_vs_halves"] = rel_err(off.series, halves[0].series + halves[1].series)
    _note("many_chunks", "fp32", err)
    print(f"catchment series, many chunks per workgroup: {err}")
    assert err["slot0_vs_plane"] <= 1e-13 and err["slot11_vs_plane"] <= 1e-13, err
    assert err["whole_vs_halves"] <= 1e-12, err


# ------------------------------------------------------------------ 5. NaN stays put
@pytest.mark.parametrize("form", ["fp32", "fp64"])
def test_nan_stays_in_its_slot_and_catchment(form):
    """P = NaN at (step 5, cell 100): the M_total series is NaN exactly where
    the per-slot plane sums are; every other entry equals the clean run's bit
    for bit."""
    _, _, cid, nc = catch_map("runs")
    step, cell = 5, 100
    hit = int(cid[cell])
    runs = {}
    for key, nan in (("clean", None), ("dirty", (step, cell))):
        with history_engine(_oracle(NY, NX, SEED, NSTEPS, nan=nan), form, cid, nc, DEPTH) as e:
            e.run(NSTEPS)
            series = e.catchment_series("M_total", first=0, count=NSTEPS)
            planes = np.stack([e.get_field("M_total", index=k) for k in range(NSTEPS)])
        nan_cells = np.isnan(planes)
        want_nan = np.stack([np.bincount(cid, weights=nan_cells[k], minlength=nc) > 0 for k in range(NSTEPS)])
        runs[key] = SimpleNamespace(series=series, want_nan=want_nan)
    assert not runs["clean"].want_nan.any() and np.isfinite(runs["clean"].series).all()
    want_nan = runs["dirty"].want_nan
    assert want_nan[step, hit] and not want_nan[:step].any() and not np.delete(want_nan, hit, axis=1).any()
    np.testing.assert_array_equal(np.isnan(runs["dirty"].series), want_nan)
    assert np.array_equal(runs["dirty"].series[~want_nan], runs["clean"].series[~want_nan])


# ------------------------------------------------------------------ 6. edges of the interface
def test_bad_arguments_raise_and_leave_the_handle_usable():
    """A state field, an input, a first slot out of range, a count of 0 and a
    count beyond the ring each raise NativeError (TFG_ERR_ARG); the run that
    follows equals that of a handle that saw none of them."""
    from topoflow_glacier._native import ERR_ARG, NativeError

    ny, nx, nc = 5, NX, 4
    orc = _oracle(ny, nx, SEED, NSTEPS)
    cid = _scatter(np.arange(ny * nx), nc)

    def ten_more(e):
        e.run(10)
        return e.catchment_series(), e.get_field("M_total", dtype=np.float32), e.get_field("h_swe")

    with history_engine(orc, "fp32", cid, nc, 8) as e:
        e.run(10)
        for kw in ({"name": "h_swe"}, {"name": "P"}, {"first": -1, "count": 1}, {"first": 8, "count": 1},
                   {"first": 0, "count": 0}, {"first": 0, "count": 9}):
            with pytest.raises(NativeError, match="catchment series") as ei:
                e.catchment_series(**kw)
            assert ei.value.code == ERR_ARG, kw
        got = ten_more(e)
    with history_engine(orc, "fp32", cid, nc, 8) as e:
        e.run(10)
        want = ten_more(e)
    assert (want[0] > 0).any()
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


def test_no_raster_one_cell_mean_and_device_out():
    """n_catch = 3 without a raster: row 0 is the domain sum, rows 1-2 are 0.
    A 1 x 1 fp64 engine's series is its get_field values.  reduce="mean" is
    sum / bincount, 0 for a catchment without cells, and follows a raster set
    again.  A CUDA-tensor `out` holds the host result."""
    import torch

    ny, nx = 5, NX
    orc = _oracle(ny, nx, SEED, NSTEPS)
    with history_engine(orc, "fp32", None, 3, 8) as e:
        e.run(8)
        got = e.catchment_series("M_total")
        want = plane_sums(e, "M_total", range(8), np.zeros(ny * nx, dtype=np.int32), 1)
        assert (want > 0).any() and rel_err(got[:, 0], want[:, 0]) <= 1e-13
        assert np.all(got[:, 1:] == 0.0)
        mean = e.catchment_series("M_total", reduce="mean")
        assert np.array_equal(mean[:, 0], got[:, 0] / (ny * nx)) and np.all(mean[:, 1:] == 0.0)

    one = _oracle(1, 1, SEED, NSTEPS)
    with history_engine(one, "fp64", None, 1, 4) as e:
        e.run(4)
        for name in FIELDS:
            vals = np.array([e.get_field(name, index=s)[0] for s in range(4)])
            assert np.array_equal(e.catchment_series(name)[:, 0], vals), name
        assert any(e.catchment_series(name).any() for name in FIELDS)

    _, _, cid, nc = catch_map("holes")
    cells = np.bincount(cid, minlength=nc)
    with history_engine(orc, "fp32", cid, nc, 8) as e:
        e.run(8)
        sums = e.catchment_series("RH")
        mean = e.catchment_series("RH", reduce="mean")
        assert (cells == 0).any() and (sums > 0).any()
        assert np.array_equal(mean, np.where(cells > 0, sums / np.maximum(cells, 1), 0.0))
        t = torch.full((8, nc), -1.0, dtype=torch.float64, device="cuda:0")
        assert e.catchment_series("RH", out=t) is t
        e.sync()
        assert np.array_equal(t.cpu().numpy(), sums)
        with pytest.raises(ValueError):
            e.catchment_series("RH", out=t, reduce="mean")
        with pytest.raises(ValueError):
            e.catchment_series("RH", out=t[:, :-1])
        # a new raster: every cell in catchment 1
        e.set_field("catch_id", np.ones(ny * nx, dtype=np.int32))
        mean1 = e.catchment_series("RH", reduce="mean")
        assert np.array_equal(mean1[:, 1], e.catchment_series("RH")[:, 1] / (ny * nx))
        assert np.all(np.delete(mean1, 1, axis=1) == 0.0)
