"""Constructed inputs for the snowfall-window tests (test infrastructure).

The engines keep the reference's float64 ring (:296, :1027-1041) as int32 slots
in quanta of 2^-36 m with an int64 running total (csrc/tfg_physics.hpp,
window_q / window_tot / window_days; DESIGN.md "Snowfall window").  The cases
here put the window total where that fixed point could part from the float64
sum: on and around thr_q = ceil(0.03 2^36) in exact quanta, within a stated
distance of 0.03 m with inexact slots, at and over the slot's saturation, with
NaN slots, and over many ring wraps.  tests/test_snowfall_window_host.py holds
every construction to the numpy oracle on the CPU; tests/test_gpu_snowfall_window.py
runs them through the engines.

A slot is P_snow dt ws metres of snow depth (:1031); every step here is cold
(T_air <= T_rain_snow), so P_snow = P.  A case is a row of per-step slot values
in quanta, q[nsteps][ncell]; precipitation(q, cfg) turns it into the P that
gives exactly those slots wherever q / (dt ws) is exact.
"""

from __future__ import annotations

import numpy as np

from tests.harness import BASE_CFG, O

QUANTUM = 2.0 ** -36
QSCALE = 2.0 ** 36
THR_Q = 2061584303            # ceil(0.03 * 2^36): 0.03 * 2^36 = 2061584302.08
BELOW_20, ABOVE_20 = 2061584300, 2061584320  # the multiples of 20 quanta on each side of it
SAT_Q = 2 ** 31 - 1           # window_q's clamp, and k_window_set's
SAT_Q_F32 = 2147483520        # the fp32 step's clamp: the largest float below 2^31 (cell_step_fast)
NAN_TOT = 1 << 44             # a NaN slot's weight in the running total (kWindowNanTot)
NAN_MIN = 1 << 43             # totals at or above it hold a NaN slot (kWindowNanMin)

CFG_WS20 = dict(BASE_CFG)                  # rho_snow = 50 (the default): ws = 20
CFG_WS16 = dict(BASE_CFG, rho_snow=62.5)   # ws = 16: with dt = 1 a slot is P 2^4, exact


def ws_of(cfg: dict) -> float:
    c = dict(O.CFG_DEFAULTS)
    c.update(cfg)
    return float(np.float64(c["rho_H2O"]) / np.float64(c["rho_snow"]))


def ring_len_of(cfg: dict) -> int:
    return int(3 * 24 / cfg["dt"])  # :296


def fp64_bound(ring_len: int) -> float:
    """Distance from 0.03 m beyond which the fp64 engine decides like the
    float64 sum: half a quantum per slot (the float64 sum's own error, ~1e-17,
    does not matter)."""
    return ring_len * 2.0 ** -37


def fp32_bound(ring_len: int) -> float:
    """The same for the fp32 engine on fp32-rounded P: one fp32 rounding of
    f_qfac and one of the product P f_qfac (2^-24 each, of a total of 0.03 m),
    and half a quantum per slot."""
    return 0.03 * 2.0 ** -23 + ring_len * 2.0 ** -37


def statics(ncell: int) -> dict:
    """Snow- and ice-covered cells on a slope (the window does not read them)."""
    c = np.arange(ncell, dtype=np.float64)
    return {"elev": 2000.0 + c, "slope": np.full(ncell, 0.25), "aspect": np.full(ncell, 1.0),
            "h0_snow": np.full(ncell, 1.0), "h0_ice": np.full(ncell, 2.0), "h0_swe": np.full(ncell, 0.0625),
            "h0_iwe": np.full(ncell, 1.75)}


def forcing_of(P: np.ndarray, T_air=None) -> dict:
    """Cold, calm forcing around the given P [nsteps][ncell]; every value but P fp32-exact."""
    P = np.asarray(P, dtype=np.float64)
    one = np.ones_like(P)
    return {"P": P, "T_air": -5.0 * one if T_air is None else np.asarray(T_air, np.float64),
            "Hum_sp": 0.001953125 * one, "P_air": 75000.0 * one, "uz": 3.0 * one}


def precipitation(q: np.ndarray, cfg: dict) -> np.ndarray:
    """P [m/h] whose slot P dt ws is q quanta: (q / (dt ws)) 2^-36.  Exact where
    dt ws is a power of two, or divides q (the multiples of 20 with ws = 20)."""
    u = float(cfg["dt"]) * ws_of(cfg)
    return (np.asarray(q, dtype=np.float64) / u) * QUANTUM


def slots_float64(P: np.ndarray, cfg: dict) -> np.ndarray:
    """The oracle's slot values, P dt ws in its operation order (:1031)."""
    return np.asarray(P, np.float64) * cfg["dt"] * np.float64(ws_of(cfg))


def fp32_exact(q: np.ndarray, cfg: dict) -> np.ndarray:
    """Where the fp32 engine's slot is q quanta with no rounding at all: P is an
    fp32 number, f_qfac = dt ws 2^36 is, and so is their fp32 product."""
    P = precipitation(q, cfg)
    P32 = P.astype(np.float32)
    qfac = float(cfg["dt"]) * ws_of(cfg) * QSCALE
    f_qfac = np.float32(qfac)
    prod = P32 * f_qfac  # np.float32 arithmetic, as the kernel's P_snow * f_qfac
    return (P32.astype(np.float64) == P) & (float(f_qfac) == qfac) & (prod.astype(np.float64) == np.asarray(q, np.float64))


def window_totals(q: np.ndarray, ring_len: int) -> np.ndarray:
    """int64 window totals [nsteps][ncell] of slot rows q: the last ring_len steps' sum."""
    q = np.asarray(q, dtype=np.int64)
    c = np.vstack([np.zeros((1,) + q.shape[1:], np.int64), np.cumsum(q, axis=0)])
    lo = np.maximum(np.arange(q.shape[0]) + 1 - ring_len, 0)
    return c[1:] - c[lo]


def days_from_totals(tot: np.ndarray, dt: float) -> np.ndarray:
    """n after every step from integer totals: the predicate tot >= thr_q on
    exact quanta, in the reference's arithmetic (n + dt/86400 from 0, :1040-1041)."""
    n = np.zeros(tot.shape[1])
    out = np.empty(tot.shape)
    for k in range(tot.shape[0]):
        n = np.where(tot[k] >= THR_Q, 0.0, n + dt / 86400)
        out[k] = n
    return out


def tile_cases(q: np.ndarray, ncell: int) -> np.ndarray:
    """Case columns repeated cyclically over ncell cells."""
    return q[:, np.arange(ncell) % q.shape[1]]


# ---------------------------------------------------------------- A. the exact threshold
A_STEPS = 100  # the 72-slot window (dt = 1): past the expiry of every slot set below


def threshold_cases(unit: int):
    """Part A: (names, q [A_STEPS][ncase], checks) for slots that are multiples
    of `unit` quanta (1 with ws = 16; 20 with ws = 20, where the exact sums need
    them).  Three big slots (steps 10-12, multiples of 1024 unit: 24 significant
    bits or fewer) carry the bulk, one small slot the rest, so that every slot
    is exact in fp32 too.  checks[name] = {step: window total in quanta}."""
    b = (THR_Q // 3) // (unit * 1024) * (unit * 1024)
    base = 3 * b
    cases = {}
    if unit == 1:
        # one slot entering takes the total to thr_q - 1, thr_q, thr_q + 1
        cases["enter_thr"] = ({20: THR_Q - 1 - base, 21: 1, 22: 1}, {20: THR_Q - 1, 21: THR_Q, 22: THR_Q + 1})
        # one slot expiring (steps 5 and 6 leave at steps 77 and 78) takes it back down
        cases["expire_thr"] = ({5: 1, 6: 1, 20: THR_Q + 1 - base - 2}, {76: THR_Q + 1, 77: THR_Q, 78: THR_Q - 1})
        # exactly thr_q on entry, and exactly thr_q - 1 after an expiry, with nothing else near
        cases["enter_at"] = ({20: THR_Q - base}, {19: base, 20: THR_Q, 81: THR_Q})
        cases["negative"] = ({20: THR_Q + 1 - base, 25: -2}, {24: THR_Q + 1, 25: THR_Q - 1, 81: THR_Q - 1})
    s = 20
    cases["enter_20"] = ({20: BELOW_20 - base, 21: s}, {20: BELOW_20, 21: ABOVE_20, 81: ABOVE_20})
    cases["expire_20"] = ({5: s, 20: ABOVE_20 - base - s}, {76: ABOVE_20, 77: BELOW_20, 81: BELOW_20})
    cases["negative_20"] = ({20: ABOVE_20 - base, 25: -s}, {24: ABOVE_20, 25: BELOW_20, 81: BELOW_20})
    names = list(cases)
    q = np.zeros((A_STEPS, len(names)), dtype=np.int64)
    for j, name in enumerate(names):
        q[10:13, j] = b
        for k, v in cases[name][0].items():
            q[k, j] = v
    return names, q, {name: cases[name][1] for name in names}


# ---------------------------------------------------------------- B. near the threshold, inexact slots
B_DELTAS = tuple(s * d for d in (1e-6, 1e-7, 3e-8, 1e-8, 3e-9, 1e-9, 2e-10) for s in (1.0, -1.0))
B_FILL = 30   # random snowfalls ahead of the tuned one
B_NEAR = 2e-6  # |tot - 0.03| of a cell-step counted as a crossing


def near_threshold_P(cfg: dict, ncell: int, seed: int, fp32: bool):
    """Part B: P [nsteps][ncell] and the intended delta per cell.  Cell c has
    B_FILL random snowfalls (steps 0 .. B_FILL-1, slots not representable in
    quanta), then one tuned so that the oracle's float64 window sum is
    0.03 + delta_c; no snow after it.  The sum stays there until the first
    slot expires ring_len steps after step 0, so every step from B_FILL to
    ring_len - 1 decides at distance delta_c, and the sum then falls away as
    the fills leave.  With `fp32`, every P is an fp32 number (what the fp32
    engine holds), the tuned one included: its slot is ~1e-4 m, so rounding it
    moves the sum by < 1e-11."""
    L = ring_len_of(cfg)
    u = cfg["dt"] * np.float64(ws_of(cfg))
    rng = np.random.default_rng(seed)
    nsteps = L + B_FILL + 4
    delta = np.array([B_DELTAS[c % len(B_DELTAS)] for c in range(ncell)])
    w = rng.uniform(0.5, 1.5, (B_FILL, ncell))
    P = np.zeros((nsteps, ncell))
    P[:B_FILL] = w / w.sum(axis=0) * (0.03 - 1e-4) / u
    if fp32:
        P = P.astype(np.float32).astype(np.float64)
    for _ in range(4):  # the last slot takes what is missing; re-tuned against the sum as the oracle forms it
        ring = np.zeros((ncell, L))
        ring[:, L - 1 - B_FILL:] = slots_float64(P[:B_FILL + 1], cfg).T
        miss = (0.03 + delta) - np.sum(ring, axis=1)
        P[B_FILL] = P[B_FILL] + miss / u
        if fp32:
            P[B_FILL] = P[B_FILL].astype(np.float32).astype(np.float64)
    return P, delta


# ---------------------------------------------------------------- C. saturation
C_VALUES = (0.031, 0.03125 - QUANTUM, 0.03125, 0.05, 1.0, 1.0e6, np.inf)  # slot values [m]; 0.03125 = 2^31 quanta
# A negative slot that saturates, alone in an otherwise empty or light window (the sum stays below 0.03 m in
# the oracle and in fixed point alike): -2^31 quanta would be the NaN sentinel's bit pattern.
C_NEGATIVE = (-1.0, -np.inf)
C_SHAPES = {  # name: (dt, step of the heavy snowfall, steps)
    "72_slots": (1, 10, 90),
    "3_slots": (24, 4, 12),
    "1_slot": (72, 3, 8),
}
C_LIGHT = 2.0 ** -12  # light snowfall [m of depth per step] around the heavy one, in every other cell: 72 stay below 0.03 m


def exact_P_for_slot(v: float, cfg: dict) -> float:
    """A P whose oracle slot (P dt ws, rounded twice) is exactly v: v / (dt ws)
    or a neighbour (dt ws = 384 or 1152 is no power of two); v / (dt ws) itself
    where none is (the CPU test holds the two values that must be exact)."""
    u = cfg["dt"] * np.float64(ws_of(cfg))
    p = np.float64(v) / u
    for cand in (p, np.nextafter(p, np.inf), np.nextafter(p, -np.inf), np.nextafter(np.nextafter(p, np.inf), np.inf),
                 np.nextafter(np.nextafter(p, -np.inf), -np.inf)):
        if slots_float64(cand, cfg) == v:
            return float(cand)
    return float(p)


def saturation_P(shape: str, fp32: bool):
    """Part C: (cfg, P [nsteps][2 (len(C_VALUES) + len(C_NEGATIVE))], heavy
    step).  Cell 2j has the heavy snowfall C_VALUES[j] alone, cell 2j+1 the
    same among light snowfall (C_LIGHT per step); the last cells hold
    C_NEGATIVE likewise."""
    dt, k_heavy, nsteps = C_SHAPES[shape]
    cfg = dict(CFG_WS16, dt=dt)
    u = dt * np.float64(ws_of(cfg))
    P = np.zeros((nsteps, 2 * (len(C_VALUES) + len(C_NEGATIVE))))
    P[:, 1::2] = C_LIGHT / u
    for j, v in enumerate(C_VALUES + C_NEGATIVE):
        P[k_heavy, 2 * j:2 * j + 2] = exact_P_for_slot(v, cfg) if np.isfinite(v) else v
    if fp32:
        with np.errstate(over="ignore"):
            P = P.astype(np.float32).astype(np.float64)
    return cfg, P, k_heavy


# ---------------------------------------------------------------- D. NaN slots
D_STEPS = 100
D_CASES = ("two_nan", "nan_and_saturated", "nan_and_negative", "nan_T_air", "light_only", "nan_only")


def nan_cases():
    """Part D: (cfg, forcing [D_STEPS][6], names) on the 72-slot window.  Light
    snowfall everywhere (a slot of 2^-12 m: 72 of them stay below 0.03 m), and
      two_nan            NaN P at steps 10 and 20: n frozen from 10 until 20 + 72
      nan_and_saturated  NaN P at step 10, a slot of 0.05 m (saturated) at step 11
      nan_and_negative   NaN P at step 10, slots of -0.01 m at steps 9 and 11
      nan_T_air          NaN T_air at step 10 with a P worth 0.05 m: neither rain
                         nor snow (:585, :604), a zero slot, no freeze, no reset
      light_only         the control
      nan_only           NaN P at step 10 alone"""
    cfg = dict(CFG_WS16)
    u = 16.0
    P = np.full((D_STEPS, len(D_CASES)), 2.0 ** -12 / u)
    T = np.full(P.shape, -5.0)
    P[[10, 20], 0] = np.nan
    P[10, 1], P[11, 1] = np.nan, 0.05 / u
    P[10, 2], P[[9, 11], 2] = np.nan, -0.01 / u
    T[10, 3], P[10, 3] = np.nan, 0.05 / u
    P[10, 5] = np.nan
    return cfg, forcing_of(P, T), D_CASES


# ---------------------------------------------------------------- E. slot I/O value by value
def slot_values() -> np.ndarray:
    """Part E: the values written into one slot, one per cell (65 cells; the
    tail repeats the first value)."""
    big = 0.03125
    b = (THR_Q // 3) // 1024 * 1024
    v = [0.0, QUANTUM, -QUANTUM, 2.0 ** -37, -2.0 ** -37, 3 * 2.0 ** -37, -3 * 2.0 ** -37, 5 * 2.0 ** -37,
         0.75 * QUANTUM, 0.25 * QUANTUM, 1.5 * QUANTUM + 2.0 ** -60,
         big - 2 * QUANTUM, big - QUANTUM, big - 0.5 * QUANTUM, big - 0.25 * QUANTUM, big, big + QUANTUM, 0.05, 1e6,
         -(big - 2 * QUANTUM), -(big - QUANTUM), -(big - 0.5 * QUANTUM), -big, -(big + QUANTUM), -0.05, -1e6,
         np.inf, -np.inf, np.nan,
         (THR_Q - 1) * QUANTUM, THR_Q * QUANTUM, (THR_Q + 1) * QUANTUM, BELOW_20 * QUANTUM, ABOVE_20 * QUANTUM,
         b * QUANTUM, (THR_Q - 1 - 3 * b) * QUANTUM, 0.03, 0.001, -0.001, 1e-300, -1e-300]
    out = np.zeros(65)
    out[:len(v)] = v
    return out


STEP_FRACTIONS = (0.5, 1.5, 2.5, 0.75, 0.25, 1000.25, 4097.5, -0.5, -1.5, -2.5, -2.75, -1000.5, 3.0, 0.0, 2.0 ** 20 + 0.5, 7.5)
"""Slot values in quanta, with fractions, that the STEP's quantisers see exactly
(fp64: P dt ws 2^36; fp32: the fp32 product P f_qfac) with dt = 1, ws = 16: what
they store shows their rounding mode alone (nearest, ties to even)."""


def slot_expected(v: np.ndarray) -> np.ndarray:
    """What a slot written with v reads back as: clip(rint(v 2^36), -(2^31-1), 2^31-1) 2^-36, NaN as NaN."""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.clip(np.rint(v * QSCALE), -float(SAT_Q), float(SAT_Q)) * QUANTUM


def slots_to_quanta(w: np.ndarray) -> np.ndarray:
    """int64 contribution of slots read back in metres to the running total (a NaN slot: 2^44)."""
    w = np.asarray(w, dtype=np.float64)
    q = np.rint(np.where(np.isnan(w), 0.0, w) * QSCALE).astype(np.int64)
    return np.where(np.isnan(w), np.int64(NAN_TOT), q)


# ---------------------------------------------------------------- F. many wraps
def wrap_sequence(cfg: dict, ncell: int, wraps: int = 4, seed: int = 11, unit: int | None = None):
    """Part F: q [nsteps][ncell].  A sequence of period ring_len that sums to
    2061584300 quanta per period (just below thr_q), every slot a multiple of
    `unit` quanta and, like q / (dt ws), an fp32 number; plus 20 quanta at every
    step k with (k - c) mod (ring_len + 1) == 0 in cell c.  A full window then
    holds one raised step (2061584320, above thr_q) on ring_len of every
    ring_len + 1 steps and none (below) on the remaining one, which falls one
    ring position later on each wrap and on a different step in each cell.
    nsteps covers `wraps` ring lengths and the below step after each."""
    L = ring_len_of(cfg)
    u = int(cfg["dt"] * ws_of(cfg))
    unit = unit or (u if L > 100 else 4 * u)
    rng = np.random.default_rng(seed)
    mean = BELOW_20 // L // unit
    m = rng.integers(mean // 2, mean + mean // 2, size=(L, ncell), dtype=np.int64)
    base = m * unit
    d = BELOW_20 - base.sum(axis=0)  # spread over the period; what does not divide goes to the last slot
    per = d // (unit * L) * unit
    base += per
    base[L - 1] += d - per * L
    nsteps = wraps * (L + 1) + ncell + 4
    k = np.arange(nsteps)
    q = base[k % L].copy()
    q += 20 * (((k[:, None] - np.arange(ncell)[None, :]) % (L + 1)) == 0)
    return q
