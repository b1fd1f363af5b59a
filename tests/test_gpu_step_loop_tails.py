"""Every way through k_fused's peeled step loops, against one step per launch.

The step loop of a launch is a peeled first round, a steady loop of whole
rounds and a tail (tfg_fused.hpp): three steps per round for the forms that
request two steps ahead, two for those that request one, one for the fp64
engine.  A launch of K steps must compute what K launches of one step compute,
whichever of the three parts its steps fall into:

  * calls of 3, 6, 8, 9 and 13 steps at fuse_steps = 24 are launches of K = 3
    (the peeled round alone), 6 (one round of the loop, no tail), 8 (tail of
    two), 9 (tail of none) and 13 (tail of one); for the two-step rounds they
    are tails of 1, 0, 0, 1, 1 behind 0, 2, 3, 3 and 5 rounds of the loop;
  * one call of 11 steps at fuse_steps = 6 is cut into launches of 6 and 5;
  * dt = 24 gives a window of three slots, the shortest a launch still fuses
    over: at K = 7 the slot a step reads was written two steps earlier in the
    same launch and must not have been overtaken by a request issued ahead.

The grid is 5 x 77 cells (two workgroup chunks, the second ragged) with 5
frames and 7 history slots, as tests/test_gpu_step_table.py; the split handle
runs 7 x 77, the smallest of these grids a handle splits (a plane stride of at
least 512 cells).  After every call the six outputs in all history slots, every
state plane and all window slots are compared bit for bit (the update is
pointwise and its arithmetic the same at every launch length).

The mass-balance integrals are sums of non-negative terms whose grouping
follows the launches, so launches of K steps and of one step round differently
by design (before the loops were peeled as after); P_max, a maximum, is exact.
The fp32 engine adds a launch's steps in fp32 per cell before it folds that sum
into fp64: each fp32 addition is off by at most 2^-24 of the running sum, so
the integrals agree within K 2^-24 <= 24 * 2^-24 of their value.  The fp64
engine adds a launch's steps per lane in fp64, scales the sum by the constant
factors once per launch, folds lanes (6 levels), waves (3) and workgroup rows
(1) and adds the launch to the running totals (39 launches at most here):
fewer than 128 roundings of at most 2^-53 on any path, so within 2^-46."""

import functools

import numpy as np
import pytest

from tests.harness import BASE_CFG, FLUX_F64_ENGINE, make_engine

pytestmark = pytest.mark.gpu

NY, NX, SEED = 5, 77, 13
N_FRAMES, HIST_DEPTH = 5, 7
HIST = ("h_snow", "SM", "h_ice", "IM", "M_total", "RH")
STATE = ("h_swe", "h_iwe", "Eccs", "Ecci", "n", "albedo")
CALLS = (3, 6, 8, 9, 13)
FUSE_MAX = 24

# name: (engine, cfg overrides, n_catch, NaN-safe form, conduction, split, ny)
FORMS = {
    "fp32": ("float32", {}, 1, False, False, None, NY),
    "nan_safe": ("float32", {}, 1, True, False, None, NY),
    "flux_f64": (FLUX_F64_ENGINE, {}, 1, False, False, None, NY),
    "satterlund": ("float32", {"SATTERLUND": True}, 1, False, False, None, NY),
    "catchments": ("float32", {}, 3, False, False, None, NY),
    "conduction": ("float32", {}, 1, False, True, None, NY),
    "fp64": ("float64", {}, 1, False, False, None, NY),
    "split": ("float32", {}, 1, False, False, "on", 7),
    "window_of_3": ("float32", {"dt": 24}, 1, False, False, None, NY),
}


@functools.lru_cache(maxsize=None)
def _run(form, fuse, calls):
    """One snapshot (history, state, window, diagnostics) after each run(c) for
    c in calls.  Cached: the snapshots are compared, never changed."""
    from topoflow_glacier.synthetic import diurnal_table

    engine, over, n_catch, nan_safe, conduction, split, ny = FORMS[form]
    e = make_engine(dict(BASE_CFG, **over), ny, NX, engine, n_frames=N_FRAMES, hist_depth=HIST_DEPTH, n_catch=n_catch,
                    fuse_steps=fuse, split=split)
    try:
        e.fill_synthetic(SEED, diurnal_table(N_FRAMES))
        if n_catch > 1:
            e.set_field("catch_id", (np.arange(ny * NX) * 5 // (ny * NX) % n_catch).astype(np.int32))
        if nan_safe:
            e.set_step_form(True)
        if conduction:
            e.conduction_update(0.3, 2.1, 30.0, 30.0, q_ground=0.5)
        if split:
            assert e.is_split()
        snaps = []
        for c in calls:
            e.run(c)
            e.sync()
            hist = {v: np.stack([e.get_field(v, index=j) for j in range(HIST_DEPTH)]) for v in HIST}
            state = {v: e.get_field(v) for v in STATE}
            window = np.stack([e.get_field("window", index=j) for j in range(e.ring_len)])
            snaps.append((hist, state, window, e.diagnostics()))
        if nan_safe:
            assert e.nan_safe_launches() > 0
        return snaps
    finally:
        e.close()


def _assert_same(form, fused, single):
    fp64_sums = FORMS[form][0] == "float64"
    assert len(fused) == len(single)
    for i, (a, b) in enumerate(zip(fused, single)):
        for v in HIST:
            assert np.array_equal(a[0][v], b[0][v], equal_nan=True), (i, v)
        for v in STATE:
            assert np.array_equal(a[1][v], b[1][v], equal_nan=True), (i, v)
        assert np.array_equal(a[2], b[2]), (i, "window slots")
        da, db = a[3], b[3]
        print(f"{form} call {i}: integrals max rel diff "
              f"{np.max(np.abs(da[:, :5] - db[:, :5]) / np.maximum(np.abs(db[:, :5]), 1e-300)):.3e}")
        assert np.array_equal(da[:, 5], db[:, 5], equal_nan=True), (i, "P_max")
        bound = 2.0**-46 if fp64_sums else FUSE_MAX * 2.0**-24
        assert (np.abs(da[:, :5] - db[:, :5]) <= bound * np.abs(db[:, :5])).all(), (i, "integrals")


@pytest.mark.parametrize("form", [f for f in FORMS if f != "window_of_3"])
def test_peel_loop_and_every_tail(form):
    """Launches of 3, 6, 8, 9 and 13 steps, compared after each."""
    fused = _run(form, FUSE_MAX, CALLS)
    assert np.isfinite(fused[-1][0]["M_total"]).all() and fused[-1][0]["M_total"].any()
    _assert_same(form, fused, _run(form, 1, CALLS))


@pytest.mark.parametrize("form", [f for f in FORMS if f != "window_of_3"])
def test_a_call_cut_into_launches_of_6_and_5(form):
    _assert_same(form, _run(form, 6, (11,)), _run(form, 1, (11,)))


def test_shortest_fused_window():
    """ring_len = 3 at K = 7: two rounds of the two-ahead loop's read-ahead
    inside a window that holds only the slots of steps k, k + 1 and k + 2."""
    fused = _run("window_of_3", FUSE_MAX, (7,))
    assert fused[0][2].shape[0] == 3
    assert fused[0][2].any()
    _assert_same("window_of_3", fused, _run("window_of_3", 1, (7,)))
