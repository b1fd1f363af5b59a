"""The constructed snowfall-window inputs (tests/window_cases.py) against the
numpy oracle alone, on the CPU: that every slot meant to be exact is exact in
float64 and in float32, that the window totals sit where the cases say, that
the near-threshold cells sit at their intended distance from 0.03 m, and that
enough of them lie outside the engines' stated bounds for the GPU test
(tests/test_gpu_snowfall_window.py) to assert something.
"""

import importlib.util
import sys

import numpy as np
import pytest

from tests import window_cases as W
from tests.harness import ROOT, oracle_days_per_step, ring_as_slots


def _oracle(cfg, P, T_air=None, **kw):
    P = np.asarray(P, np.float64)
    return oracle_days_per_step(cfg, W.statics(P.shape[1]), W.forcing_of(P, T_air), P.shape[0], **kw)


def test_threshold_constant():
    """thr_q = ceil(0.03 2^36) = 2061584303; against the float64 0.03 the totals
    thr_q - 1 and 2061584300 compare below, thr_q and 2061584320 at or above."""
    assert int(np.ceil(0.03 * 2.0 ** 36)) == W.THR_Q
    for q, above in ((W.THR_Q - 1, False), (W.THR_Q, True), (W.THR_Q + 1, True), (W.BELOW_20, False), (W.ABOVE_20, True)):
        assert (q * W.QUANTUM >= 0.03) == above, q
    assert W.BELOW_20 % 20 == 0 and W.ABOVE_20 - W.BELOW_20 == 20 and W.BELOW_20 < W.THR_Q <= W.ABOVE_20


@pytest.mark.parametrize("unit,cfg", [(1, W.CFG_WS16), (20, W.CFG_WS20)], ids=["ws16", "ws20"])
def test_exact_threshold_cases(unit, cfg):
    """Part A: every slot is an exact number of quanta in float64 and in the fp32
    engine's arithmetic, the window totals are the intended ones, the oracle's
    float64 sum is that integer times 2^-36 at every step, and its n is the
    integer predicate's."""
    names, q, checks = W.threshold_cases(unit)
    assert W.ws_of(cfg) == (16.0 if unit == 1 else 20.0) and W.ring_len_of(cfg) == 72
    assert (q % unit == 0).all()
    P = W.precipitation(q, cfg)
    assert np.array_equal(W.slots_float64(P, cfg) * W.QSCALE, q.astype(np.float64))
    assert W.fp32_exact(q, cfg).all()
    assert (np.abs(q) < 2 ** 31 - 1).all()  # no slot saturates
    tot = W.window_totals(q, 72)
    for j, name in enumerate(names):
        for k, want in checks[name].items():
            assert tot[k, j] == want, (name, k)
    want_totals = {W.THR_Q - 1, W.THR_Q, W.THR_Q + 1, W.BELOW_20, W.ABOVE_20} if unit == 1 else {W.BELOW_20, W.ABOVE_20}
    assert want_totals <= set(tot.ravel().tolist())
    r = _oracle(cfg, P)
    assert np.array_equal(r.tot * W.QSCALE, tot.astype(np.float64))
    assert np.array_equal(r.n, W.days_from_totals(tot, cfg["dt"]))
    # both outcomes at a step next to the threshold, in every case
    reset = r.n == 0.0
    for j, name in enumerate(names):
        ks = sorted(checks[name])
        assert reset[ks, j].any() and not reset[ks, j].all(), name
    # the negative slot takes the sum from above the threshold to below it
    j = names.index("negative_20")
    assert tot[24, j] >= W.THR_Q > tot[25, j] and q[25, j] < 0 and reset[24, j] and not reset[25, j]


def test_exact_cases_through_the_fp32_emulation():
    """The numpy float32 emulation of the fp32 step
    (tests/diagnostics/fp32_emulation.py; its window lines: np.float32
    product, clamp, rint, int64 total) on part A's inputs stores the intended
    quanta in every slot and gives the oracle's n after every step."""
    from topoflow_glacier.physics.clock import StepClock

    spec = importlib.util.spec_from_file_location("fp32_emulation", ROOT / "tests" / "diagnostics" / "fp32_emulation.py")
    emu = importlib.util.module_from_spec(spec)
    path = list(sys.path)
    try:
        spec.loader.exec_module(emu)
    finally:
        sys.path[:] = path
    for unit, cfg in ((1, W.CFG_WS16), (20, W.CFG_WS20)):
        names, q, _ = W.threshold_cases(unit)
        e = emu.Fp32Engine(cfg, W.statics(q.shape[1]))
        assert e.thr_q == W.THR_Q
        P32 = W.precipitation(q, cfg).astype(np.float32)
        f = W.forcing_of(P32.astype(np.float64))
        U = StepClock(cfg["start_time"], cfg["dt"], cfg["lat"], cfg["lon"], None, ring_len=72).uniforms(0, q.shape[0])
        ns = []
        with np.errstate(all="ignore"):
            for k in range(q.shape[0]):
                e.step(U[k], *(f[v][k] for v in ("P", "T_air", "Hum_sp", "P_air", "uz")))
                assert np.array_equal(e.ring[k % 72], q[k]), (unit, k)  # the slot it stored: the intended quanta
                ns.append(e.n.copy())
        assert np.array_equal(e.tot, W.window_totals(q, 72)[-1])
        assert np.array_equal(np.stack(ns), _oracle(cfg, P32.astype(np.float64)).n)


@pytest.mark.parametrize("dt", [1, 0.25])
@pytest.mark.parametrize("fp32", [False, True], ids=["fp64", "fp32"])
def test_near_threshold_cells_sit_at_their_distance(dt, fp32):
    """Part B: from the tuned step until the first slot expires the oracle's
    float64 window sum is 0.03 + delta to within 2 % of |delta| (plus 1e-12), so
    the sign of the decision is the intended one; slots are not whole quanta;
    and at least half of the cell-steps near the threshold lie outside the
    engine's bound, so the GPU test's exact comparison covers them."""
    cfg = dict(W.CFG_WS20, dt=dt)
    L = W.ring_len_of(cfg)
    assert L == (72 if dt == 1 else 288)
    P, delta = W.near_threshold_P(cfg, 65, seed=5, fp32=fp32)
    if fp32:
        assert np.array_equal(P.astype(np.float32).astype(np.float64), P)
    r = _oracle(cfg, P)
    held = r.tot[W.B_FILL:L] - 0.03  # steps at which the sum is held at its distance
    assert (np.abs(held - delta) <= 0.02 * np.abs(delta) + 1e-12).all(), np.abs(held - delta).max()
    assert ((r.n[W.B_FILL:L] == 0.0) == (delta > 0)).all()
    sl = W.slots_float64(P[:W.B_FILL + 1], cfg) * W.QSCALE
    if not fp32:
        assert (sl != np.rint(sl)).mean() > 0.9  # slots that are no whole number of quanta
    else:  # 24-bit P: the engine's fp32 product P f_qfac (a factor 5) rounds instead
        prod = P[:W.B_FILL + 1].astype(np.float32) * np.float32(dt * 20.0 * W.QSCALE)
        assert (prod.astype(np.float64) != sl).mean() > 0.5
    bound = W.fp32_bound(L) if fp32 else W.fp64_bound(L)
    near = np.abs(r.tot - 0.03) <= W.B_NEAR
    assert near.sum() >= 65 * (L - W.B_FILL)
    outside = np.abs(r.tot - 0.03) > bound
    assert (near & outside).sum() >= 0.5 * near.sum(), ((near & outside).sum(), near.sum())
    assert (near & ~outside).sum() >= 0.1 * near.sum()  # and the band itself is visited
    for d in (1e-6, 1e-7, 1e-8):  # the distances that must be outside every bound
        assert d > W.fp32_bound(288)
    assert 2e-10 < W.fp64_bound(72) and 1e-9 < W.fp64_bound(288) and 3e-9 < W.fp32_bound(72)


@pytest.mark.parametrize("shape", list(W.C_SHAPES))
def test_saturation_inputs(shape):
    """Part C: in float64 the heavy slots are the listed values (0.03125 - 2^-36
    and 0.03125 exactly: 2^31 - 1 and 2^31 quanta, the last value that fits
    and the first that saturates); the oracle resets n at the heavy step in
    every cell and, without light snowfall, counts again once the slot has
    expired; light snowfall alone never reaches 0.03 m."""
    cfg, P, k = W.saturation_P(shape, fp32=False)
    L = W.ring_len_of(cfg)
    assert L == {"72_slots": 72, "3_slots": 3, "1_slot": 1}[shape] and W.ws_of(cfg) == 16.0
    sl = W.slots_float64(P[k], cfg)
    assert sl[2] == sl[3] == 0.03125 - W.QUANTUM and sl[2] * W.QSCALE == 2.0 ** 31 - 1
    assert sl[4] == sl[5] == 0.03125 and sl[4] * W.QSCALE == 2.0 ** 31
    assert np.allclose(sl[0::2][:6], W.C_VALUES[:6], rtol=1e-15) and np.isinf(sl[-1])
    assert L * W.C_LIGHT < 0.03
    r = _oracle(cfg, P)
    assert P.shape[0] >= k + L + 3
    pos = np.arange(P.shape[1]) < 2 * len(W.C_VALUES)
    assert (r.n[k:k + L, pos] == 0.0).all()
    assert (r.n[k + L, pos] == r.dpd).all() and (r.n[k - 1] == k * r.dpd).all()
    # the negative slots (-1 m, -inf) saturate too and never reset n
    assert (sl[~pos] * W.QSCALE < -(2.0 ** 31)).all() and (np.diff(r.n[:, ~pos], axis=0) > 0).all()
    cfg32, P32, _ = W.saturation_P(shape, fp32=True)
    assert np.array_equal(P32.astype(np.float32).astype(np.float64), P32)
    assert np.array_equal(_oracle(cfg32, P32).n, r.n)  # fp32-rounded P: the same decisions


def test_nan_cases():
    """Part D: n freezes while a NaN slot is in the oracle's ring (from the
    first NaN until the last has expired) whatever else the window holds; a NaN
    T_air with positive P leaves a zero slot and n running."""
    cfg, forcing, names = W.nan_cases()
    r = oracle_days_per_step(cfg, W.statics(len(names)), forcing, W.D_STEPS, ring_at=(30, W.D_STEPS))
    dpd = r.dpd
    j = names.index("two_nan")
    assert (r.n[9:92, j] == r.n[9, j]).all() and r.n[92, j] == r.n[9, j] + dpd  # frozen over steps 10 .. 91
    assert np.isnan(r.rings[30][:, j]).sum() == 2 and not np.isnan(r.rings[W.D_STEPS][:, j]).any()
    for name in ("nan_and_saturated", "nan_and_negative", "nan_only"):
        j = names.index(name)
        assert (r.n[9:82, j] == r.n[9, j]).all(), name  # frozen over steps 10 .. 81
        assert np.isnan(r.rings[30][:, j]).sum() == 1
    j = names.index("nan_and_saturated")
    assert r.n[82, j] == 0.0 and r.n[83, j] == dpd  # the 0.05 m slot outlives the NaN by one step
    j = names.index("nan_T_air")
    assert np.array_equal(r.n[:, j], r.n[:, names.index("light_only")]) and r.rings[30][10, j] == 0.0
    assert (np.diff(r.n[:, names.index("light_only")]) > 0).all()  # never 0.03 m: n only grows


def test_slot_values_expected():
    """Part E: the expected read-back of every written value, spelled out for
    the ties and the clamp."""
    v = W.slot_values()
    x = W.slot_expected(v)
    q = W.QUANTUM
    want = {0.0: 0.0, q: q, -q: -q, 2.0 ** -37: 0.0, -2.0 ** -37: 0.0, 3 * 2.0 ** -37: 2 * q, -3 * 2.0 ** -37: -2 * q,
            5 * 2.0 ** -37: 2 * q, 0.03125 - q: 0.03125 - q, 0.03125 - 0.5 * q: 0.03125 - q, 0.03125: 0.03125 - q,
            0.05: 0.03125 - q, np.inf: 0.03125 - q, -np.inf: -(0.03125 - q), -0.03125: -(0.03125 - q),
            W.THR_Q * q: W.THR_Q * q, 1e-300: 0.0}
    for a, b in want.items():
        assert x[np.nonzero(v == a)[0][0]] == b, a
    assert np.isnan(x[np.isnan(v)]).all() and np.isnan(v).sum() == 1
    assert (np.abs(x[~np.isnan(x)]) <= W.SAT_Q * q).all()
    tot = W.slots_to_quanta(x)
    assert tot[np.isnan(v)][0] == W.NAN_TOT and tot[np.nonzero(v == 0.05)[0][0]] == W.SAT_Q


def test_step_fractions_are_exact():
    """The fractional slot values of the rounding-mode test reach both step
    quantisers unrounded: P, P dt ws 2^36 and the fp32 product P f_qfac are exact."""
    qf = np.array(W.STEP_FRACTIONS)
    assert W.fp32_exact(qf, W.CFG_WS16).all()
    assert np.array_equal(W.slots_float64(W.precipitation(qf, W.CFG_WS16), W.CFG_WS16) * W.QSCALE, qf)
    assert (np.abs(qf - np.rint(qf)) == 0.5).sum() >= 8  # ties, of both signs and both parities
    assert {0.25, 0.75} <= set(np.abs(qf - np.floor(qf)).tolist())


@pytest.mark.parametrize("dt", [0.25, 1])
def test_wrap_sequence(dt):
    """Part F: exact slots in float64 and float32, period sums of 2061584300
    quanta, a full window above thr_q on ring_len of every ring_len + 1 steps
    and below on the remaining one, which moves one ring position per wrap."""
    cfg = dict(W.CFG_WS20, dt=dt)
    L = W.ring_len_of(cfg)
    q = W.wrap_sequence(cfg, 65 if dt == 0.25 else 8)
    nsteps, ncell = q.shape
    assert nsteps >= 4 * L
    assert (q > 0).all() and (q < 2 ** 31 - 1).all() and (q % (5 if dt == 0.25 else 20) == 0).all()
    P = W.precipitation(q, cfg)
    assert np.array_equal(W.slots_float64(P, cfg) * W.QSCALE, q.astype(np.float64))
    assert W.fp32_exact(q, cfg).all()
    tot = W.window_totals(q, L)
    k = np.arange(nsteps)[:, None]
    below = ((k - np.arange(ncell)[None, :]) % (L + 1)) == L  # the window k-L+1 .. k holds no raised step
    full = k >= L - 1
    assert np.array_equal(tot[full[:, 0]], np.where(below, W.BELOW_20, W.ABOVE_20)[full[:, 0]])
    assert (below & full).sum(axis=0).min() >= 4
    pos = [np.nonzero(below[:, c] & full[:, 0])[0] % L for c in range(ncell)]
    assert all(len(set(p.tolist())) == len(p) for p in pos)  # a different ring position on each wrap
    r = _oracle(cfg, P)
    assert np.array_equal(r.tot * W.QSCALE, tot.astype(np.float64))
    assert np.array_equal(r.n, W.days_from_totals(tot, dt))
    assert np.array_equal(ring_as_slots(np.asarray(q[-L:].T, np.float64), nsteps)[(nsteps - 1) % L], q[-1].astype(np.float64))
