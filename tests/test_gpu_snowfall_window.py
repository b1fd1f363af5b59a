"""The snowfall window's fixed-point total at its edges, against the numpy oracle.

The engines replace the reference's float64 ring and per-step np.sum
(:1027-1041) by int32 slots in quanta of 2^-36 m and an int64 running total
(csrc/tfg_physics.hpp window_q / window_tot / window_days, k_window_set / get /
total; DESIGN.md "Snowfall window").  Only the predicate tot >= 0.03 m is used:
it resets or advances n, the days since major snowfall.  The reference here is
the oracle's m.n recorded after EVERY step, and n is compared with ==: in both
it is a sum of identical days_per_dt additions from 0.  No melt-onset or
melt-out allowance and no step mask apply in this file; the only slack is the
stated distance from 0.03 m inside which fixed point and float64 may differ
(part B), derived in tests/window_cases.py.  The inputs are built there and
held to the oracle on the CPU by tests/test_snowfall_window_host.py.

  A  window totals of exact quanta at thr_q - 1, thr_q, thr_q + 1 and at the
     multiples of 20 quanta on each side, by a slot entering and by one expiring
  B  inexact slots at +-1e-6 .. +-2e-10 m from 0.03 m: exact agreement outside
     ring_len 2^-37 (fp64) / 0.03 2^-23 + ring_len 2^-37 (fp32)
  C  slots at and over the saturation value 2^-5 m, in 72-, 3- and 1-slot windows
  D  NaN slots next to NaN, saturated and negative ones; NaN injected as a slot
  E  k_window_set / k_window_get value by value; the total rebuilt after a set
  F  no drift over four ring wraps in every launch shape
"""

import functools

import numpy as np
import pytest

from tests import window_cases as W
from tests.harness import (FLUX_F64_ENGINE, gpu_days_one_cell, gpu_days_per_launch, make_engine, oracle_days_per_step,
                           read_window, setup_engine, split_engine)

pytestmark = pytest.mark.gpu
ENGINES = ["float64", "float32", FLUX_F64_ENGINE]


def _is_fp32(engine):
    return split_engine(engine)[0] == "float32"


def _assert_days(r, ref, what=""):
    """n after every launch equals the oracle's after the same step, exactly."""
    want = ref.n[r.done - 1]
    bad = np.argwhere(r.n != want)
    assert bad.size == 0, (what, "first (launch, cell):", bad[:5].tolist(), r.n[tuple(bad[0])], want[tuple(bad[0])])


# ---------------------------------------------------------------- A
A_NY, A_NX = 3, 65  # one wave plus one cell per row: the ragged tail runs


@functools.lru_cache(maxsize=None)
def _threshold_ref(ws):
    unit, cfg = (1, W.CFG_WS16) if ws == "ws16" else (20, W.CFG_WS20)
    names, q, _ = W.threshold_cases(unit)
    P = W.precipitation(W.tile_cases(q, A_NY * A_NX), cfg)
    static, forcing = W.statics(A_NY * A_NX), W.forcing_of(P)
    return cfg, static, forcing, oracle_days_per_step(cfg, static, forcing, W.A_STEPS)


@pytest.mark.parametrize("ws", ["ws16", "ws20"])
@pytest.mark.parametrize("engine", ENGINES)
def test_exact_threshold(engine, ws):
    """Part A.  Every slot is an exact number of quanta in float64 and in the
    fp32 engine's arithmetic, so the float64 sum and the fixed-point total are
    the same number and n must equal the oracle's after every step: one launch
    per step, fused at 24, and launches cut at the steps next to the threshold."""
    cfg, static, forcing, ref = _threshold_ref(ws)
    cuts = [21, 1, 1, 2, 1, 51, 1, 1, 21]  # ends after steps 20, 21, 22, 24, 25, 76, 77, 78, 99
    for launches in ([1] * W.A_STEPS, [24, 24, 24, 24, 4], cuts):
        r = gpu_days_per_launch(cfg, static, forcing, A_NY, A_NX, engine, launches)
        _assert_days(r, ref, f"launches of {launches[0]}")
        assert not r.ns.any()  # finite data: the fp32 engine's fast step form, with its own predicate line
    if _is_fp32(engine):  # and its NaN-safe form (window_tot / window_days) on the same inputs
        r = gpu_days_per_launch(cfg, static, forcing, A_NY, A_NX, engine, cuts, nan_safe=True)
        _assert_days(r, ref, "NaN-safe form")
        assert r.ns[-1] == len(cuts)


# ---------------------------------------------------------------- B
@functools.lru_cache(maxsize=None)
def _near_ref(dt, fp32):
    cfg = dict(W.CFG_WS20, dt=dt)
    P, _ = W.near_threshold_P(cfg, 65, seed=5, fp32=fp32)
    static, forcing = W.statics(65), W.forcing_of(P)
    return cfg, static, forcing, oracle_days_per_step(cfg, static, forcing, P.shape[0])


@pytest.mark.parametrize("dt", [1, 0.25], ids=["72_slots", "288_slots"])
@pytest.mark.parametrize("engine", ENGINES)
def test_near_threshold_margin(engine, dt):
    """Part B.  Where the oracle's float64 window sum is further from 0.03 m
    than the engine's bound (window_cases.fp64_bound / fp32_bound), the engine
    takes the oracle's decision, and n equals the oracle's exactly for as long
    as no step inside the band has parted them (and again from the next common
    reset).  Inside the band n is 0 or the previous n + days_per_dt.  A fused
    run gives the per-step run's n at its launch ends, bit for bit."""
    fp32 = _is_fp32(engine)
    cfg, static, forcing, ref = _near_ref(dt, fp32)
    L = W.ring_len_of(cfg)
    nsteps = ref.n.shape[0]
    bound = W.fp32_bound(L) if fp32 else W.fp64_bound(L)
    r = gpu_days_per_launch(cfg, static, forcing, 1, 65, engine, [1] * nsteps)
    margin = np.abs(ref.tot - 0.03)
    prev = np.zeros(65)
    agree = np.ones(65, dtype=bool)
    compared = 0
    for k in range(nsteps):
        g = r.n[k]
        reset_g, reset_o = g == 0.0, ref.n[k] == 0.0
        assert (reset_g | (g == prev + ref.dpd)).all(), (k, g, prev)
        outside = margin[k] > bound
        assert (reset_g == reset_o)[outside].all(), (k, np.nonzero(outside & (reset_g != reset_o))[0], margin[k])
        agree = (agree & (reset_g == reset_o)) | (reset_g & reset_o)
        assert (g == ref.n[k])[agree].all(), (k, np.nonzero(agree & (g != ref.n[k]))[0])
        compared += int((outside & (margin[k] <= W.B_NEAR)).sum())
        prev = g
    near = int((margin <= W.B_NEAR).sum())
    assert compared >= 0.5 * near > 0, (compared, near)
    fused = gpu_days_per_launch(cfg, static, forcing, 1, 65, engine, [24] * (nsteps // 24) + [nsteps % 24])
    assert np.array_equal(fused.n, r.n[fused.done - 1])


# ---------------------------------------------------------------- C
@functools.lru_cache(maxsize=None)
def _saturation_ref(shape, fp32):
    cfg, P, k = W.saturation_P(shape, fp32)
    static, forcing = W.statics(P.shape[1]), W.forcing_of(P)
    ref = oracle_days_per_step(cfg, static, forcing, P.shape[0], ring_at=(k + 1, P.shape[0]))
    return cfg, static, forcing, k, ref


@pytest.mark.parametrize("shape", list(W.C_SHAPES))
@pytest.mark.parametrize("engine", ENGINES)
def test_saturated_slots(engine, shape):
    """Part C.  One snowfall of 0.031 m .. +inf of depth in a step, alone or
    among light snowfall, followed until its slot has expired: n equals the
    oracle's after every step (saturation at 2^-5 m > 0.03 m cannot change the
    predicate for non-negative snowfall), launched per step and fused.  Two
    more cells hold one slot of -1 m and of -inf, which saturates at the other
    end and must not read as the NaN sentinel (n keeps advancing).  The
    slots read back: never NaN; a saturated one (2^31 - 1) 2^-36 m -- from the
    fp32 step (2^31 - 128) 2^-36 m, the largest fp32 below 2^31 that its
    quantiser clamps to, 127 quanta inside its bound; an unsaturated one the
    oracle's ring value within half a quantum (fp64) or within one fp32
    rounding of the product plus half a quantum (fp32, part B's bound per slot)."""
    fp32 = _is_fp32(engine)
    cfg, static, forcing, k, ref = _saturation_ref(shape, fp32)
    nsteps, ncell = forcing["P"].shape
    L = W.ring_len_of(cfg)
    r = gpu_days_per_launch(cfg, static, forcing, 1, ncell, engine, [1] * nsteps, window_at=(k + 1, nsteps))
    _assert_days(r, ref, "per step")
    fused = {"72_slots": [24, 24, 24, 18], "3_slots": [5, 7], "1_slot": [8]}[shape]
    rf = gpu_days_per_launch(cfg, static, forcing, 1, ncell, engine, fused, window_at=(nsteps,))
    _assert_days(rf, ref, "fused")
    assert np.array_equal(rf.windows[nsteps], r.windows[nsteps])
    for done in (k + 1, nsteps):
        w, ring = r.windows[done], ref.rings[done]
        assert w.shape == (L, ncell) and not np.isnan(w).any()
        rq = ring * W.QSCALE
        if not fp32:
            sat = np.abs(rq) > float(W.SAT_Q)
            assert np.array_equal(w[sat], np.sign(rq[sat]) * (W.SAT_Q * W.QUANTUM))
            assert (np.abs(w[~sat] - ring[~sat]) <= 0.5 * W.QUANTUM).all()
        else:
            sat = np.abs(rq) >= float(W.SAT_Q_F32) + 64  # the fp32 product, rounded to 128 quanta here, is at the clamp or over
            assert (np.abs(rq[~sat]) <= float(W.SAT_Q_F32) - 64).all()  # no case in between
            assert np.array_equal(w[sat], np.sign(rq[sat]) * (W.SAT_Q_F32 * W.QUANTUM))
            assert (np.abs(w[~sat] - ring[~sat]) <= np.abs(ring[~sat]) * 2.0 ** -23 + 0.5 * W.QUANTUM).all()
            assert (W.SAT_Q - W.SAT_Q_F32) * W.QUANTUM <= 0.03125 * 2.0 ** -23 + 0.5 * W.QUANTUM
    heavy = r.windows[k + 1][k % L]
    npos = 2 * len(W.C_VALUES)
    assert (heavy[2 * 2:npos] >= W.SAT_Q_F32 * W.QUANTUM).all()  # 0.03125 m and more: saturated
    assert (heavy[:2] < 0.0311).all() and (heavy[npos:] <= -W.SAT_Q_F32 * W.QUANTUM).all()


# ---------------------------------------------------------------- D
@functools.lru_cache(maxsize=None)
def _nan_ref():
    cfg, forcing, names = W.nan_cases()
    idx = np.arange(8) % len(names)
    forcing = {k: v[:, idx] for k, v in forcing.items()}
    static = W.statics(8)
    return cfg, static, forcing, oracle_days_per_step(cfg, static, forcing, W.D_STEPS, ring_at=(30, W.D_STEPS))


@pytest.mark.parametrize("engine", ENGINES)
def test_nan_slots(engine):
    """Part D.  Two NaN snowfalls ten steps apart, a NaN next to a saturated
    slot and next to negative ones, and a NaN T_air with positive P (a zero
    slot, no freeze): n equals the oracle's after every step -- frozen from the
    first NaN until the last has expired -- and the slots are NaN exactly where
    the oracle's ring is.  In the fp32 engine the launch that reads the NaN
    and every one after it (the NaN snowfall stays in h_swe) runs the NaN-safe
    step form."""
    cfg, static, forcing, ref = _nan_ref()
    r = gpu_days_per_launch(cfg, static, forcing, 1, 8, engine, [1] * W.D_STEPS, window_at=(30, W.D_STEPS))
    _assert_days(r, ref, "per step")
    for done in (30, W.D_STEPS):
        assert np.array_equal(np.isnan(r.windows[done]), np.isnan(ref.rings[done])), done
    assert np.isnan(r.windows[30]).sum() == 8 and not np.isnan(r.windows[W.D_STEPS]).any()  # 2 1 1 0 0 1 | 2 1
    zero = r.windows[30][10, 3]
    assert zero == 0.0  # NaN T_air: neither rain nor snow
    rf = gpu_days_per_launch(cfg, static, forcing, 1, 8, engine, [10] * 10, window_at=(30, W.D_STEPS))
    _assert_days(rf, ref, "fused at 10")
    assert np.array_equal(rf.windows[30], r.windows[30], equal_nan=True)
    assert np.array_equal(rf.windows[W.D_STEPS], r.windows[W.D_STEPS])
    assert rf.ns.tolist() == ([0] + list(range(1, 10)) if _is_fp32(engine) else [0] * 10)


def _injected(device):
    """Light snowfall in 8 cells over 22 launches of 8 steps; before the third
    launch slot 9 (written by step 9, due to expire at step 81) is set from a
    host array or a device tensor: NaN in cell 3, 0.05 m (saturating) in cell 5."""
    cfg = dict(W.CFG_WS16)
    P = np.full((176, 8), W.C_LIGHT / 16.0)
    values = np.full(8, W.C_LIGHT)
    values[3], values[5] = np.nan, 0.05
    static, forcing = W.statics(8), W.forcing_of(P)
    ref = oracle_days_per_step(cfg, static, forcing, 176, ring_at=(24, 176), inject={16: [(9, values)]})
    if device:
        import torch

        values = torch.as_tensor(values, device="cuda:0")
    return cfg, static, forcing, ref, {16: [(9, values)]}


@pytest.mark.parametrize("source", ["host", "device"])
@pytest.mark.parametrize("engine", ENGINES)
def test_nan_injected_as_a_window_slot(engine, source):
    """Part D, through TFG_ST_WINDOW.  n equals the oracle's (its ring set
    likewise) after every launch: frozen in the NaN's cell until step 81
    overwrites the slot, reset in the saturated one.  The fp32 engine runs the
    NaN-safe form in every launch while the NaN slot is in the window -- found
    at once in a host array, by the lazy state check ahead of the next launch
    for a device tensor -- and the fast form again once a later state check
    (every 8 launches while the state is dirty) finds the window clean."""
    cfg, static, forcing, ref, inject = _injected(source == "device")
    r = gpu_days_per_launch(cfg, static, forcing, 1, 8, engine, [8] * 22, window_at=(24, 176), inject=inject)
    _assert_days(r, ref, source)
    assert np.array_equal(np.isnan(r.windows[24]), np.isnan(ref.rings[24])) and np.isnan(r.windows[24][9, 3])
    assert r.windows[24][9, 5] == W.SAT_Q * W.QUANTUM
    assert not np.isnan(r.windows[176]).any()
    frozen = r.n[1, 3]
    assert (r.n[1:10, 3] == frozen).all() and r.n[10, 3] > frozen  # launches 2 .. 9 end inside steps 16 .. 80
    if _is_fp32(engine):
        assert r.ns[1] == 0, r.ns
        assert np.array_equal(np.diff(r.ns[1:11]), np.ones(9, dtype=r.ns.dtype)), r.ns  # launches 2 .. 10 (steps 16 .. 87)
        assert r.ns[-1] <= r.ns[10] + 8 and r.ns[-1] == r.ns[-2] == r.ns[-3], r.ns  # the fast form is back
    else:
        assert not r.ns.any()


@functools.lru_cache(maxsize=None)
def _full_ring_mix():
    """A 288-slot window (dt = 0.25) filled through TFG_ST_WINDOW after 8 dry
    steps, every slot at a clamp: cell 0 one NaN and 287 slots of -1 m, cell 1
    288 slots of +1 m (the largest finite total, 288 (2^31 - 1) < 2^43), cell 2
    two NaN among -1 m, cell 3 one NaN among +1 m, cell 4 all -1 m, cells 5-7
    left empty; then 17 more dry steps."""
    cfg = dict(W.CFG_WS16, dt=0.25)
    fill = np.zeros((288, 8))
    fill[:, [0, 2, 4]], fill[:, [1, 3]] = -1.0, 1.0
    fill[100, [0, 2, 3]] = np.nan
    fill[200, 2] = np.nan
    inject = {8: [(s, fill[s]) for s in range(288)]}
    static, forcing = W.statics(8), W.forcing_of(np.zeros((25, 8)))
    return cfg, static, forcing, inject, oracle_days_per_step(cfg, static, forcing, 25, inject=inject)


@pytest.mark.parametrize("engine", ENGINES)
def test_nan_slot_outweighs_a_window_of_clamped_slots(engine):
    """Part D, the total's headroom: a NaN slot counts 2^44 and the finite
    slots of the longest window at most 288 (2^31 - 1) < 2^40 either way, so
    the total is >= 2^43 exactly while a NaN slot is in the window.  With
    every other slot at the negative clamp n still freezes (as the oracle's,
    whose sum is NaN), and a window of 288 slots at the positive clamp without
    a NaN resets n instead of freezing it."""
    cfg, static, forcing, inject, ref = _full_ring_mix()
    dpd = ref.dpd
    assert (ref.n[8:, [0, 2, 3]] == 8 * dpd).all() and (ref.n[8:, 1] == 0.0).all()  # frozen; reset
    assert np.array_equal(ref.n[8:, 4], ref.n[8:, 5]) and ref.n[24, 5] == ref.n[23, 5] + dpd  # advancing
    r = gpu_days_per_launch(cfg, static, forcing, 1, 8, engine, [8, 1, 8, 8], inject=inject, window_at=(9,))
    _assert_days(r, ref)
    tot = W.slots_to_quanta(r.windows[9]).sum(axis=0)
    assert (tot[[0, 2, 3]] >= W.NAN_MIN).all() and (tot[[1, 4, 5]] < W.NAN_MIN).all()
    assert tot[0] == W.NAN_TOT - 286 * W.SAT_Q and tot[1] == 287 * W.SAT_Q  # step 8 has overwritten slot 8 with 0


# ---------------------------------------------------------------- E
@pytest.mark.parametrize("engine", ["float64", "float32"])
def test_window_slot_io_value_by_value(engine):
    """Part E.  Values written through TFG_ST_WINDOW (k_window_set) read back
    (k_window_get) as clip(rint(v 2^36), -(2^31-1), 2^31-1) 2^-36 in float64
    numpy -- ties to even, the clamp on both sides, +-inf clamped, NaN as NaN --
    from a float64 and a float32 source; slot -1 and slot ring_len are argument
    errors that change nothing."""
    from topoflow_glacier import _native as nat

    v = W.slot_values()
    e = make_engine(W.CFG_WS16, 1, 65, engine, n_frames=1, hist_depth=1)
    try:
        setup_engine(e, W.statics(65))
        assert e.ring_len == 72
        for slot in (0, 5, 71):
            e.set_field("window", v, index=slot)
            np.testing.assert_array_equal(e.get_field("window", index=slot), W.slot_expected(v))
        v32 = v.astype(np.float32)
        e.set_field("window", v32, index=6)
        np.testing.assert_array_equal(e.get_field("window", index=6), W.slot_expected(v32.astype(np.float64)))
        before = read_window(e)
        assert not before[1:5].any() and not before[7:71].any()
        for bad in (-1, 72):
            with pytest.raises(nat.NativeError) as err:
                e.set_field("window", np.ones(65), index=bad)
            assert err.value.code == nat.ERR_ARG
            with pytest.raises(nat.NativeError) as err:
                e.get_field("window", index=bad)
            assert err.value.code == nat.ERR_ARG
        np.testing.assert_array_equal(read_window(e), before)
    finally:
        e.close()


@pytest.mark.parametrize("form", ["chosen", "nan_safe"])
@pytest.mark.parametrize("engine", ENGINES)
def test_step_quantisers_round_to_nearest_even(engine, form):
    """The step's own quantisers (window_q in the fp64 engine, the fp32
    product's conversion in the fp32 engine, in both of its step forms) on
    slot values with fractions of a quantum that reach them unrounded: the slot
    stores rint(value), ties to even, exactly."""
    qf = np.array(W.STEP_FRACTIONS)
    n = qf.size
    P = np.vstack([W.precipitation(qf, W.CFG_WS16)[None, :], np.zeros((1, n))])
    r = gpu_days_per_launch(W.CFG_WS16, W.statics(n), W.forcing_of(P), 1, n, engine, [1, 1], window_at=(1, 2),
                            nan_safe=form == "nan_safe")
    for done in (1, 2):
        np.testing.assert_array_equal(r.windows[done][0] * W.QSCALE, np.rint(qf))
    assert not r.windows[2][1:].any()
    assert r.ns[-1] == (2 if form == "nan_safe" and _is_fp32(engine) else 0)


@pytest.mark.parametrize("pre", [0, 10], ids=["fresh", "after_10_steps"])
@pytest.mark.parametrize("engine", ["float64", "float32"])
def test_total_is_rebuilt_after_slots_are_set(engine, pre):
    """Part E.  After slots are set the running total is rebuilt from the ring
    (k_window_total), not adjusted: a slot written twice with different values
    counts once, with its last value, and the slot the next step overwrites
    does not count.  The injected totals are thr_q - 1, thr_q, thr_q + 1,
    2061584300, 2061584320 and one with a NaN slot; one step of zero snowfall
    then resets n (set to 5 days first) to 0, advances it or leaves it, as the
    host's int64 sum of the slots read back says."""
    n = 65
    cfg = dict(W.CFG_WS16)
    e = make_engine(cfg, 1, n, engine, n_frames=2, hist_depth=1, fuse_steps=1)
    try:
        setup_engine(e, W.statics(n))
        light, none = W.forcing_of(np.full((1, n), W.C_LIGHT / 16.0)), W.forcing_of(np.zeros((1, n)))
        for frame, f in ((0, light), (1, none)):
            for name in ("P", "T_air", "Hum_sp", "P_air", "uz"):
                e.set_field(name, f[name][0], index=frame)
        if pre:
            e.run(pre, frames=np.zeros(pre, dtype=np.int32))
        b = (W.THR_Q // 3) // 1024 * 1024
        targets = np.array([W.THR_Q - 1, W.THR_Q, W.THR_Q + 1, W.BELOW_20, W.ABOVE_20, 0])[np.arange(n) % 6]
        is_nan = np.arange(n) % 6 == 5
        for j in range(pre):  # clear what the light steps wrote
            e.set_field("window", np.zeros(n), index=j)
        e.set_field("window", np.full(n, 12345 * W.QUANTUM), index=pre)  # overwritten by the step: must not count
        for slot in (20, 21, 22):
            e.set_field("window", np.full(n, b * W.QUANTUM), index=slot)
        rest = (targets - 3 * b) * W.QUANTUM
        e.set_field("window", rest + 1000 * W.QUANTUM, index=23)                  # first a wrong value,
        e.set_field("window", np.where(is_nan, np.nan, rest), index=23)          # then the one that counts
        e.set_field("n", np.full(n, 5.0))
        e.run(1, frames=np.ones(1, dtype=np.int32))
        e.sync()
        got = e.get_field("n")
        w = read_window(e)
    finally:
        e.close()
    assert not w[pre].any()  # the step's own slot: zero snowfall
    tot = W.slots_to_quanta(w).sum(axis=0)
    assert np.array_equal(tot[~is_nan], targets[~is_nan]) and (tot[is_nan] >= W.NAN_MIN).all()
    dpd = cfg["dt"] / 86400
    want = np.where(tot >= W.NAN_MIN, 5.0, np.where(tot >= W.THR_Q, 0.0, 5.0 + dpd))
    assert np.array_equal(got, want), (got[:6], want[:6])


# ---------------------------------------------------------------- F
F_CUTS = (289, 1, 288, 300)  # ends on the below steps 288 and 577 of cell 0; 300 steps: past the window


@functools.lru_cache(maxsize=None)
def _wrap_ref(dt, ncell):
    cfg = dict(W.CFG_WS20, dt=dt)
    q = W.wrap_sequence(cfg, ncell)
    static, forcing = W.statics(ncell), W.forcing_of(W.precipitation(q, cfg))
    return cfg, static, forcing, q, oracle_days_per_step(cfg, static, forcing, q.shape[0], ring_at=(q.shape[0],))


def _wrap_shapes(engine, dt, ncell, shapes):
    cfg, static, forcing, q, ref = _wrap_ref(dt, ncell)
    nsteps = q.shape[0]
    L = W.ring_len_of(cfg)
    final = ref.rings[nsteps]
    assert np.array_equal(final * W.QSCALE, q[nsteps - L:][(np.arange(L) - nsteps) % L].astype(np.float64))
    for name, launches in shapes.items():
        launches = list(launches) + ([nsteps - sum(launches)] if sum(launches) < nsteps else [])
        r = gpu_days_per_launch(cfg, static, forcing, 1, ncell, engine, launches, window_at=(nsteps,))
        _assert_days(r, ref, name)
        assert np.array_equal(r.windows[nsteps], final), name  # bit-equal between launch shapes, and the oracle's ring
    return ref


@pytest.mark.parametrize("engine", ENGINES)
def test_no_drift_over_four_wraps(engine):
    """Part F.  dt = 0.25 (288 slots), 1225 steps of exact-quanta slots whose
    full-window total is 2061584320 (above thr_q) except on one step in 289
    (2061584300, below), at a different ring position on each wrap and a
    different step in each of the 65 cells: n after every launch equals the
    oracle's, launched per step, fused at 24, and fused past the window with
    odd cuts; the final slots are the oracle's ring in every shape."""
    nsteps = _wrap_ref(0.25, 65)[3].shape[0]
    _wrap_shapes(engine, 0.25, 65, {"per step": [1] * nsteps, "fused at 24": [24] * (nsteps // 24), "odd cuts": F_CUTS})


@pytest.mark.parametrize("engine", ["float32", FLUX_F64_ENGINE])
def test_no_drift_72_slots_fused_past_the_window(engine):
    """Part F's 72-slot analogue (dt = 1, 304 steps) in the fp32 engine with
    launches of 96 and of 150 steps, which re-read slots they wrote."""
    _wrap_shapes(engine, 1, 8, {"per step": [1] * 304, "fused at 96": [96, 96, 96], "fused at 150": [150, 150]})


def test_one_cell_kernels_follow_the_grid_over_the_wraps():
    """Part F.  Cell 7 of the same sequence through the one-cell fp64 kernels
    (k_cell: update_io; k_cell_many: update_many; k_cell_run: run() with the odd
    cuts): n after every step / launch is the grid's (fused at 24) wherever
    both were read and the oracle's throughout, the final slots the grid's."""
    cell = 7
    cfg, static, forcing, q, ref = _wrap_ref(0.25, 65)
    nsteps = q.shape[0]
    grid = gpu_days_per_launch(cfg, static, forcing, 1, 65, "float64", [24] * (nsteps // 24) + [nsteps % 24],
                               window_at=(nsteps,))
    _assert_days(grid, ref, "grid")
    cuts = list(F_CUTS) + [nsteps - sum(F_CUTS)]
    for kernel in ("k_cell", "k_cell_many", "k_cell_run"):
        n, done, slots = gpu_days_one_cell(cfg, static, forcing, cell, nsteps, kernel, launches=cuts)
        assert np.array_equal(n, ref.n[done - 1, cell]), kernel
        both = np.isin(grid.done, done)
        assert np.array_equal(grid.n[both, cell], n[np.isin(done, grid.done)]), kernel
        assert np.array_equal(slots, grid.windows[nsteps][:, cell]), kernel
