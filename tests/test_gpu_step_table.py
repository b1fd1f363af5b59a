"""The addresses the fused step loop reads and writes, step by step.

Every step of a launch reads one forcing frame and one snowfall-window slot and
writes that slot and one history slot; which ones is the host's choice per step
(tfg_uniforms: frame, slot, hist).  A launch of K steps must touch exactly the
planes K launches of one step touch, whatever K is, wherever a launch is cut
out of the steps of one tfg_step call, and for each of the kernel's forms.  A
wrong plane shows as soon as two steps of one launch differ in it, so the
shapes are the smallest with that property:

  * 5 x 77 cells (385): a ragged last wave, two workgroup chunks, n no multiple
    of 64;
  * n_frames = 5, hist_depth = 7, dt = 1 (a 72-slot window) and 80 steps: the
    frame index, the history slot and the window slot each wrap, at different
    steps.

The update is pointwise and the step arithmetic the same in every launch
length, so the comparisons are bit for bit (np.array_equal); against the numpy
oracle the tolerance is the suite's floored 1e-5 (tests/harness.py).

tfg_update's path: a grid handle fed per step (set_inputs + run(1), and
update_io) against the same steps queued into frames is held below.  The BMI
update() of a one-cell model against the same steps queued into frames is
tests/test_callers.py::test_bulk_mode_equals_per_step_bmi, and update_io
against set_inputs + run(1) + get_outputs on (3, 2) frames and history slots is
tests/test_gpu_parity.py::test_update_io_equals_set_step_get."""

import functools

import numpy as np
import pytest

from tests.harness import (BASE_CFG, FLUX_F64_ENGINE, assert_oracle_rule, gpu_run_fields, make_engine, oracle_run,
                           run_gpu_vs_oracle, synthetic_inputs)

pytestmark = pytest.mark.gpu

NY, NX, SEED = 5, 77, 13
N_FRAMES, HIST_DEPTH, NSTEPS = 5, 7, 80
HIST = ("h_snow", "SM", "h_ice", "IM", "M_total", "RH")
STATE = ("h_swe", "h_iwe", "Eccs", "Ecci", "n", "albedo")


@functools.lru_cache(maxsize=None)
def _run(fuse, chunks=(NSTEPS,), engine="float32", n_catch=1, split=None, ny=NY, nx=NX):
    """The synthetic grid stepped by run(c) for c in chunks.  Returns (history
    [7][6 outputs][n], state planes, all window slots, diagnostics, whether
    the handle split its launches).  Cached: the results are compared, never
    changed."""
    from topoflow_glacier.synthetic import diurnal_table

    e = make_engine(BASE_CFG, ny, nx, engine, n_frames=N_FRAMES, hist_depth=HIST_DEPTH, n_catch=n_catch,
                    fuse_steps=fuse, split=split)
    try:
        e.fill_synthetic(SEED, diurnal_table(N_FRAMES))
        if n_catch > 1:
            e.set_field("catch_id", (np.arange(ny * nx) * 5 // (ny * nx) % n_catch).astype(np.int32))
        was_split = e.is_split()
        for c in chunks:
            e.run(c)
        e.sync()
        hist = {v: np.stack([e.get_field(v, index=j) for j in range(HIST_DEPTH)]) for v in HIST}
        state = {v: e.get_field(v) for v in STATE}
        window = np.stack([e.get_field("window", index=j) for j in range(e.ring_len)])
        return hist, state, window, e.diagnostics(), was_split
    finally:
        e.close()


def _assert_same(a, b, diag=False):
    for v in HIST:
        assert np.array_equal(a[0][v], b[0][v], equal_nan=True), v
    for v in STATE:
        assert np.array_equal(a[1][v], b[1][v], equal_nan=True), v
    assert np.array_equal(a[2], b[2]), "window slots"
    if diag:
        assert np.array_equal(a[3], b[3], equal_nan=True), "diagnostics"


def test_every_index_wraps_inside_fused_launches():
    """80 steps as launches of 24, 24, 24 and 8 against one step per launch:
    the six outputs in all 7 history slots, every state plane and all 72 window
    slots, with the frame (mod 5), the history slot (mod 7) and the window slot
    (mod 72) wrapping inside launches."""
    fused, single = _run(24), _run(1)
    assert fused[2].shape[0] == 72
    assert np.isfinite(fused[0]["M_total"]).all() and fused[0]["M_total"].any()
    _assert_same(fused, single)


def test_wrapping_fused_run_holds_the_oracle_tolerance():
    """The same grid, frames and launches against the numpy oracle (floored 1e-5)."""
    rep = run_gpu_vs_oracle(NY, NX, NSTEPS, "float32", seed=SEED, n_frames=N_FRAMES, fuse_steps=24)
    assert rep["ok"], rep["summary"]


def test_every_tail_of_the_unrolled_loop_and_launches_cut_from_one_call():
    """Calls of 1, 2, 3, 4, 5 and 7 steps (K mod 3 = 1, 2, 0, 1, 2, 1; K = 1 and
    2 have a read-ahead that re-requests the launch's own last frame), and one
    call of 11 steps cut into launches of 4, 4 and 3: both equal one step per
    launch."""
    chunks = (1, 2, 3, 4, 5, 7)
    _assert_same(_run(24, chunks), _run(1, (sum(chunks),)))
    _assert_same(_run(4, (11,)), _run(1, (11,)))


@pytest.mark.parametrize("ny,nx", [(NY, NX), (7, NX)])
def test_split_parts_equal_one_launch(ny, nx):
    """split="on" against split="off": outputs, state, window and (one
    workgroup per chunk either way, as tests/test_gpu_split.py) diagnostics bit
    for bit.  A handle splits from 512 cells of plane stride: 5 x 77 (448) stays
    one launch whatever the mode; 7 x 77 (576: three chunks) runs its second
    part from chunk 1 with its own copy of the steps."""
    on, off = _run(24, split="on", ny=ny, nx=nx), _run(24, split="off", ny=ny, nx=nx)
    stride = -(-ny * nx // 64) * 64
    assert on[4] == (stride >= 512) and not off[4]
    _assert_same(on, off, diag=True)


@pytest.mark.parametrize("engine", ["float32", FLUX_F64_ENGINE])
def test_satterlund_form_vs_oracle(engine):
    """SATTERLUND: true against the oracle at the suite's tolerance, the clean form of the step."""
    rep = run_gpu_vs_oracle(NY, NX, 48, engine, seed=SEED, cfg_over={"SATTERLUND": True})
    assert rep["ok"], rep["summary"]


@pytest.mark.parametrize("engine", ["float32", FLUX_F64_ENGINE])
def test_satterlund_form_with_missing_forcing_vs_oracle(engine):
    """One NaN forcing value: the launch runs the NaN-safe instance of the
    Satterlund form.  NaN where the oracle has NaN, in outputs and state; the
    finite values at the floored 1e-5."""
    nsteps = 24
    cfg = dict(BASE_CFG, SATTERLUND=True)
    syn, _ = synthetic_inputs(SEED, NY, NX, nsteps)
    static = {k: np.asarray(syn[s], np.float64) for k, s in (
        ("elev", "elev"), ("slope", "slope"), ("aspect", "aspect"), ("h0_snow", "h_snow"), ("h0_ice", "h_ice"),
        ("h0_swe", "h_swe"), ("h0_iwe", "h_iwe"))}
    forcing = {k: np.array(syn[k], dtype=np.float64) for k in ("P", "T_air", "Hum_sp", "P_air", "uz")}
    forcing["Hum_sp"][2, 70] = np.nan
    outs, state, _ = gpu_run_fields(cfg, static, forcing, NY, NX, engine, nsteps)
    ref, m = oracle_run(cfg, static, forcing)
    assert np.isnan(ref["M_total"][2:, 70]).all() and np.isnan(ref["M_total"]).sum() == nsteps - 2
    assert_oracle_rule(outs, state, ref, m, 1e-5)


def test_fp64_engine_fused_equals_unfused():
    _assert_same(_run(24, engine="float64"), _run(1, engine="float64"))


def test_catchment_variant_fused_equals_unfused():
    _assert_same(_run(24, n_catch=3), _run(1, n_catch=3))


@pytest.mark.parametrize("engine", ["float32", "float64"])
def test_a_grid_fed_per_step_equals_the_steps_queued_into_frames(engine):
    """tfg_update reads the step's forcing at its host block, not at a frame:
    a grid handle fed per step through set_inputs + run(1), and through
    update_io (tfg_update), against the same steps read from queued frames in
    one fused call.  Outputs of every step and the final state, bit for bit."""
    from topoflow_glacier.synthetic import diurnal_table

    nsteps, n = 12, NY * NX
    syn, _ = synthetic_inputs(SEED, NY, NX, N_FRAMES)  # the host mirror of fill_synthetic's frames
    order = ("P_air", "Hum_sp", "P", "T_air", "uz")
    bmi = ("h_snow", "h_swe", "SM", "h_ice", "h_iwe", "IM", "M_total", "RH")
    runs = []
    for mode in ("queued", "set_inputs", "update_io"):
        queued = mode == "queued"
        e = make_engine(BASE_CFG, NY, NX, engine, n_frames=N_FRAMES if queued else 3,
                        hist_depth=nsteps if queued else 2, fuse_steps=24)
        try:
            e.fill_synthetic(SEED, np.resize(diurnal_table(N_FRAMES), N_FRAMES if queued else 3))
            if queued:
                e.run(nsteps)
                outs = {v: np.stack([e.get_field(v, index=k) for k in range(nsteps)]) for v in HIST}
            else:
                buf, rows = np.empty((8, n)), []
                for k in range(nsteps):
                    vals = np.ascontiguousarray(np.stack([syn[v][k % N_FRAMES].astype(np.float64) for v in order]))
                    if mode == "update_io":
                        rows.append(e.update_io(vals, buf).copy())
                    else:
                        e.set_inputs(vals, k % 3)
                        e.run(1)
                        rows.append(e.get_outputs())
                outs = {v: np.stack([r[bmi.index(v)] for r in rows]) for v in HIST}
            runs.append((outs, {v: e.get_field(v) for v in STATE}))
        finally:
            e.close()
    for outs, state in runs[1:]:
        for v in HIST:
            assert np.array_equal(outs[v], runs[0][0][v]), v
        for v in STATE:
            assert np.array_equal(state[v], runs[0][1][v]), v
