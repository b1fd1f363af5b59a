"""One-step probe of the energy terms through the engine's own fp64 cold contents.

melt_core keeps the cold contents Eccs and Ecci in fp64, and both can be set
and read (set_field / get_field, as checkpoint() does).  With a large cold
content injected (ECC0 = 2^20) one step melts nothing and

    Ecci1 = Ecci0 - E_in                    where there is ice      (:1418-1434)
    Eccs1 = Eccs0 - E_in                    without snowfall        (:1556-1558)
    Eccs1 = Eccs0 + cold - E_in             with snowfall           (:1507-1537)

with E_in = Q_sum dt exactly as the step formed it, so

    E_in = Ecci0 - Ecci1      (cells with ice; else Eccs0 - Eccs1)
    cold = (Eccs1 - Eccs0) + E_in           (cells with ice and snowfall)

to the 2^-32 of the fp64 subtractions.  The oracle performs the same
subtractions from the same injected state (oracle_probe), so the two are
compared like for like.  A cell without ice and without snow (the unclamped
surface) keeps its cold content only where new snow falls: such cells get a
snowfall of P_TINY and their probe is E_in - cold, cold being ~1e-5 of it.

The sweeps (sweep_a, sweep_b, sweep_c) are per-point arrays, every forcing and
static value rounded to fp32 first, so the fp32 engine and the fp64 oracle read
the same numbers; steps are (julian day, hours from solar noon) pairs fed to
both directly (probe_clock), so a step can be put within 1e-7 h of a slope's own
sunrise.

Cut rule (parity_cut): a point is left out of the parity assertion only if
moving ONE of the oracle's fp32 inputs P, T_air, Hum_sp, P_air, uz or elev by one ulp (slope and aspect
enter through the fp64 geometry and the depths are fp64 state: they stay) changes the oracle's own probe
by more than half the tolerance at that point (0.5 tol max(|ref|, s_v), s_v the
stratum's floor); at most CUT_CAP of any stratum may be cut.  Points whose
oracle E_in is not finite (a zero or negative humidity: log of it) are outside
the probe's linear range and carry no parity assertion; they stay in the sweep
for the layout-identity assertion.

The one-catchment kernels (k_cell, k_cell_many) run their own restatement of
the fp64 step; gpu_probe_one_cell steps a deterministic sample of each sweep's
(point, step) pairs (one_cell_sample) through them, one launch per pair, from
the same injected state and with the same uniform records as gpu_probe.

The other half of the step, from E_in and the state to the melt rates, depths and cold contents, has its
own cases at the end of this file ("melt states": melt_case, meltout_case, melt_tail), stepped from
injected cold contents of the cell's own size instead of ECC0 (gpu_probe's and gpu_probe_one_cell's `ecc`).

CPU-importable: the engine is imported only inside the gpu_* and update_* functions.
"""

from __future__ import annotations

from functools import lru_cache
from types import SimpleNamespace

import numpy as np

from tests.harness import BASE_CFG, FLUX_F64_ENGINE, make_engine, scale_floor
import tfg_oracle as O

ECC0 = 2.0 ** 20       # injected cold contents
P_TINY = 2.0 ** -40    # snowfall that keeps an unclamped cell's cold content alive
CUT_CAP = 0.01         # largest share of a stratum the cut rule may remove
WAVE = 64
INJ_SNOW = 0.04        # [m] snowfall already in the window of the "fresh snowfall" cells (>= 0.03, :1040)

FORCING = ("P", "T_air", "Hum_sp", "P_air", "uz")
STATE = ("h_swe", "h_iwe", "Eccs", "Ecci", "n", "albedo", "h_snow", "h_ice")
READ = ("Eccs", "Ecci", "h_swe", "n", "albedo")
OUTS = ("h_snow", "SM", "h_ice", "IM", "M_total", "RH")

# engine forms of the GPU test: (name, engine, SATTERLUND, nan_safe or None)
FORMS = [(f"{n}{'-sat' if sat else ''}-{'nansafe' if ns else 'plain'}", eng, sat, ns)
         for n, eng in (("f32", "float32"), ("fluxf64", FLUX_F64_ENGINE)) for sat in (False, True) for ns in (True, False)]
FORMS.append(("f64", "float64", False, None))
FORMS.append(("f64-sat", "float64", True, None))

ONE_CELL_KERNELS = ("k_cell", "k_cell_many")  # tfg_update, tfg_update_many: the drop-in path's single steps
IN_ORDER = ("P_air", "Hum_sp", "P", "T_air", "uz")  # tfg_update / tfg_update_many input order
OUT_ROW = {"h_snow": 0, "SM": 2, "h_ice": 3, "IM": 5, "M_total": 6, "RH": 7}  # rows of their [8][1] output block
SAMPLE_SEED = 20260101  # one_cell_sample's; the same as layouts'
MANY_POOL = 96          # handles of a k_cell_many probe: each batch steps them all in one launch


def f32(x):
    """Rounded to fp32, held as fp64: what the fp32 engine stores of an input."""
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def f32_step(x, direction):
    """The fp32 neighbour of each (fp32-representable) value, as fp64.  A zero stays: it is exact in
    fp32, and the reference branches on it (calm air's bot == 0, :642; T_air > 0, :1041)."""
    a = np.asarray(x, dtype=np.float64).astype(np.float32)
    b = np.nextafter(a, np.float32(np.inf if direction > 0 else -np.inf))
    return np.where(a == 0, a, b).astype(np.float64)


def e_sat_mbar(T, satterlund=False):
    """Saturation vapour pressure [mbar] (:788-802; Brutsaert's or Satterlund's), for building humidities."""
    T = np.asarray(T, np.float64)
    return 10.0 ** (11.4 - 2353.0 / (T + 273.15)) / 100.0 if satterlund else 6.11 * np.exp(17.3 * T / (T + 237.3))


def hum_sp_for(RH, T, P_air, eps=0.622, satterlund=False):
    """Specific humidity that gives e_air = RH e_sat(T) at P_air [Pa] (:817-826 inverted)."""
    e = 100.0 * RH * e_sat_mbar(T, satterlund)
    return eps * e / (P_air - (1.0 - eps) * e)


def _product(**axes):
    names = list(axes)
    grids = np.meshgrid(*[np.asarray(axes[k], dtype=np.float64) for k in names], indexing="ij")
    return {k: g.reshape(-1) for k, g in zip(names, grids)}


def _finish(name, cfg, pts, jd, th, night, strat_uz, meta=None):
    """Common tail of the builders: fp32 rounding, state defaults, classes, layouts."""
    n = len(pts["T_air"])
    for k in FORCING + ("elev", "slope", "aspect", "h_snow", "h_ice"):
        pts[k] = f32(np.broadcast_to(pts[k], (n,)))
    c = dict(O.CFG_DEFAULTS)
    c.update(cfg)
    ws, wi = c["rho_H2O"] / c["rho_snow"], c["rho_H2O"] / c["rho_ice"]
    pts["h_swe"] = pts["h_snow"] / ws
    pts["h_iwe"] = pts["h_ice"] / wi
    for k, v in (("n", 0.0), ("albedo", 0.3), ("ring", 0.0)):
        pts[k] = np.array(np.broadcast_to(np.asarray(pts.get(k, v), np.float64), (n,)))
    uz_vals = np.unique(pts["uz"])
    s = SimpleNamespace(name=name, cfg=cfg, pts=pts, n=n, jd=np.asarray(jd, np.float64), th=np.asarray(th, np.float64),
                        night=np.asarray(night, bool), uz_id=np.searchsorted(uz_vals, pts["uz"]) if strat_uz else
                        np.zeros(n, np.int64), uz_vals=uz_vals if strat_uz else uz_vals[:1], meta=meta or {})
    s.snowing = (pts["P"] > 0) & (pts["T_air"] <= c["T_rain_snow"])
    s.from_ecci = pts["h_ice"] > 0
    # the cold content reads where Eccs survives the step (snow before it, or new snow) beside an Ecci;
    # where it rains instead it must come out as exactly zero
    s.cold_ok = s.from_ecci & (pts["P"] > P_TINY) & (s.snowing | (pts["h_snow"] > 0))
    return s


# ------------------------------------------------------------------------------------------- sweep A
A_T = np.linspace(-45.0, 45.0, 19)                       # includes 0: T_air = T_surf exactly where T_dew > 0 on snow
A_RH = (0.02, 0.1, 0.3, 0.6, 0.9, 1.0, 1.3)
A_PZ = ((104000.0, 0.0), (96000.0, 400.0), (94000.0, 600.0), (75000.0, 2500.0), (60000.0, 4200.0), (45000.0, 6000.0))
A_UZ = (0.0, 0.05, 0.28, 3.0, 15.8, 40.0)
# (h_snow, h_ice): bare ice; snow below, at and beyond z - z0 l2min = 9.9999 m (z = 10 m, z0 = 0.01 m; the
# clamp of :670); no snow and no ice (the unclamped surface).  Depths with (z - h)/z0 near 1 (h ~ 9.99) are
# left out: the roughness log passes through zero there and Dn through infinity (in the reference too).
A_SURF = ((0.0, 2.0), (0.5, 2.0), (5.0, 2.0), (9.9, 2.0), (9.99995, 2.0), (10.5, 2.0), (0.0, 0.0))


@lru_cache(maxsize=None)
def sweep_a():
    """Thermodynamic sweep: the full product T_air x RH x (P_air, elev) x uz x surface, one night and one
    day step.  The flux form's lhc / p0 exponent y = M g elev / (R T_K) leaves exp_near's range
    (|y + 0.345| <= 0.41, i.e. y <= 0.065) between 400 m and 600 m, so both sides of it are present.
    Unclamped cells exist only where it can snow (T_air <= T_rain_snow): without snow, ice or snowfall
    the step resets both cold contents and nothing can be read."""
    g = _product(T_air=A_T, RH=A_RH, pz=np.arange(len(A_PZ)), uz=A_UZ, surf=np.arange(len(A_SURF)))
    pz, sf = g.pop("pz").astype(int), g.pop("surf").astype(int)
    _, g["gid"] = np.unique(np.stack([g["T_air"], g["RH"], pz, sf]), axis=1, return_inverse=True)  # the point but for uz
    g["P_air"], g["elev"] = np.array(A_PZ)[pz, 0], np.array(A_PZ)[pz, 1]
    g["h_snow"], g["h_ice"] = np.array(A_SURF)[sf, 0], np.array(A_SURF)[sf, 1]
    bare = (g["h_snow"] == 0) & (g["h_ice"] == 0)
    keep = ~bare | (g["T_air"] <= BASE_CFG["T_rain_snow"])
    g = {k: v[keep] for k, v in g.items()}
    bare = bare[keep]
    g["Hum_sp"] = hum_sp_for(g.pop("RH"), g["T_air"], g["P_air"])
    g["P"] = np.where(bare, P_TINY, 0.0)
    g["slope"], g["aspect"] = 0.3, 200.0
    g["n"] = 2.0
    gid = g.pop("gid").reshape(-1)
    cfg = dict(BASE_CFG, time_zone="America/Los_Angeles")
    return _finish("A", cfg, g, jd=[100.0, 100.5], th=[-11.0, 0.6], night=[True, False], strat_uz=True,
                   meta={"gid": gid})


# ------------------------------------------------------------------------------------------- sweep B
B_RH = (-0.01, 0.0, 1e-3, 0.05, 0.3, 0.7, 1.0, 1.5, 1.676331, 1.7, 2.5, 4.9, 5.0, 5.1, 8.0, 12.0)
B_P = (1e-9, 1e-7, 1e-6, 1e-5)   # P dt ws <= 2e-4 m: far below the window's 0.03 m, so n is not reset


@lru_cache(maxsize=None)
def sweep_b(T_rs: float, satterlund: bool = False):
    """Wet-bulb sweep, every point with P > 0, one night step.  T_air: a grid up to T_rain_snow, then
    float32(T_rs) and its two fp32 neighbours (the engine compares with the largest float <= T_rs).
    RH as the kernel forms it, from -0.01 (a slightly negative humidity) through the fits' [0, 5] to 12,
    plus, per T_air, the RH at which den = 1 + (T + RH)(RH - 1.676331) is +-1e-3 and +-1e-4.  den < 0
    occurs with T + RH > 0 (RH < 1.676331, warm air: T_rs = 50.2 only) and with T + RH < 0 (RH large, cold
    air).  Humidities whose vapour pressure would exceed 0.8 P_air are left out.  The humidities are built
    with the saturation pressure of the form under test, so RH is what the list says in both."""
    t_thr = np.float32(T_rs)
    near = [np.nextafter(t_thr, np.float32(-np.inf)), t_thr, np.nextafter(t_thr, np.float32(np.inf))]
    grid = [t for t in (-40.0, -25.0, -15.0, -8.0, -3.755, -2.0, -1.0, -0.3, 0.35, 1.0, 2.0, 5.0, 10.0, 20.0, 35.0, 45.0)
            if t < T_rs - 0.01]
    T = np.array(grid + [float(x) for x in near])
    rows = []
    for t in T:
        rh = list(B_RH)
        for target in (1e-3, 1e-4, -1e-4, -1e-3):  # den = target: (t + r)(r - c) = target - 1, both roots
            c0 = 1.676331
            disc = (t - c0) ** 2 + 4.0 * (t * c0 + target - 1.0)
            if disc >= 0:
                rh += [r for r in ((c0 - t + np.sqrt(disc)) / 2, (c0 - t - np.sqrt(disc)) / 2) if 0.0 < r < 12.0]
        for r in rh:
            if 100.0 * r * e_sat_mbar(t, satterlund) < 0.8 * 88000.0:
                rows += [(t, r, p) for p in B_P]
    rows = np.array(rows)
    g = {"T_air": rows[:, 0], "P": rows[:, 2], "P_air": 88000.0, "elev": 2000.0, "uz": 3.0, "h_snow": 1.0, "h_ice": 2.0,
         "slope": 0.3, "aspect": 200.0, "n": 2.0}
    g["Hum_sp"] = hum_sp_for(rows[:, 1], rows[:, 0], 88000.0, satterlund=satterlund)
    cfg = dict(BASE_CFG, time_zone="America/Los_Angeles", T_rain_snow=T_rs)
    return _finish(f"B-Trs{T_rs:g}", cfg, g, jd=[100.0], th=[-11.0], night=[True], strat_uz=False,
                   meta={"RH_built": rows[:, 1]})


# ------------------------------------------------------------------------------------------- sweep C
C_SLOPES = (0.0, 0.5, 5.0, 100.0)
C_ASPECTS = np.arange(0.0, 360.0, 15.0)                  # includes the four cardinal values exactly
C_DAYS = (78.0, 171.0, 264.0, 354.0)                     # 20 March, 21 June, 22 September, 21 December
# albedo states: (n [days], T_air, h_snow, ring, P): aged snow at both signs of T_air, bare ice, snowfall
# already in the window (resets n), snowfall of this step that resets n
C_ALB = [(n, t, 1.0, 0.0, 0.0) for n in (0.0, 0.5, 10.0, 60.0) for t in (-3.0, 3.0)] + \
        [(10.0, 3.0, 0.0, 0.0, 0.0), (10.0, -3.0, 1.0, INJ_SNOW, 0.0), (10.0, -3.0, 1.0, 0.0, 0.002)]
C_NIGHT = (354.0, -11.9)   # the dark reference step: the other three terms do not read the clock
C_MIN_GAP = 1e-9           # [h] no step may be closer than this to any cell's sunrise or sunset
C_BRACKET_ALB = (5, 8)     # albedo states of the bracket sweep: aged snow in warm air, bare ice
C_NEAR = 3e-3              # [h] a bracketing step is within this of the time it brackets


def _sun_offsets(lat, jd, alpha, beta):
    return O.sunrise_offset_slope(lat, jd, alpha, beta), O.sunset_offset_slope(lat, jd, alpha, beta)


def bracket_jd(day):
    """The julian day every bracketing step of a day carries, so that a cell's sunrise and sunset of
    that day are one number each."""
    return day + 0.5


@lru_cache(maxsize=None)
def sweep_c(lat: float, brackets: bool = False):
    """Sun sweep at one latitude (a config value), all cells with ice so that E_in reads from Ecci, in two
    parts with the same slopes x aspects.  Step 0 of both is the dark reference.

    brackets=False ("C-lat*"): x every albedo state; every hour of the four solstice and equinox days.

    brackets=True ("Cb-lat*"): x two albedo states (the dark decision does not read the albedo); for EVERY
    (slope, aspect, day), the steps that bracket that cell's own sunrise and its own sunset as the oracle
    computes them, one set of steps per distinct time (times equal to 1e-6 h share one): +-1e-7 h and
    +-2e-4 h where the slope itself sets the time (the short wave then jumps there, the diffuse part
    being already up: decidable at any distance; 1e-7 h is inside the fp32 dark test's margin, 2e-4 h
    outside), +-2e-3 h where the flat horizon sets it (the short wave starts from zero there, and must
    exceed the rounding of the fp32 sum to be seen).  A step closer than C_MIN_GAP to any cell's sunrise
    or sunset is moved away from the time it brackets."""
    states = C_BRACKET_ALB if brackets else range(len(C_ALB))
    g = _product(slope=C_SLOPES, aspect=C_ASPECTS, alb=np.array(states))
    alb = np.array(C_ALB)[g.pop("alb").astype(int)]
    g["n"], g["T_air"], g["h_snow"], g["ring"], g["P"] = alb.T
    g["h_ice"], g["P_air"], g["elev"], g["uz"] = 2.0, 88000.0, 2000.0, 3.0
    g["Hum_sp"] = hum_sp_for(0.6, g["T_air"], 88000.0)
    cfg = dict(BASE_CFG, time_zone="America/Los_Angeles", lat=lat)
    probe = O.OracleGrid(cfg, elev=2000.0, slope=f32(g["slope"]), aspect=f32(g["aspect"]), h0_snow=0.0, h0_ice=0.0,
                         h0_swe=0.0, h0_iwe=0.0)
    jd, th, away = [C_NIGHT[0]], [C_NIGHT[1]], [1.0]
    for day in C_DAYS:
        if not brackets:
            for h in range(24):
                jd.append(day + h / 24.0)
                th.append(h - 12.0 + 0.37)
                away.append(1.0)
            continue
        jn = bracket_jd(day)
        delta = O.declination(O.day_angle(jn))
        for t_all, flat in zip(_sun_offsets(lat, jn, probe.alpha, probe.beta),
                               (O.sunrise_offset(lat, delta), O.sunset_offset(lat, delta))):
            t_sorted = np.unique(t_all)
            for t in t_sorted[np.concatenate([[True], np.diff(t_sorted) > 1e-6])]:
                for d in ((1e-7, 2e-4) if abs(t - flat) > 0.02 else (2e-3,)):
                    jd += [jn, jn]
                    th += [t - d, t + d]
                    away += [-1.0, 1.0]
    jd, th = np.array(jd), np.array(th)
    for k in range(len(th)):  # decidable by construction
        sr, ss = _sun_offsets(lat, jd[k], probe.alpha, probe.beta)
        for _ in range(64):
            if min(np.abs(th[k] - sr).min(), np.abs(th[k] - ss).min()) >= C_MIN_GAP:
                break
            th[k] += away[k] * 4.0 * C_MIN_GAP
    night = np.zeros(len(th), bool)
    night[0] = True
    return _finish(f"C{'b' if brackets else ''}-lat{lat:g}", cfg, g, jd=jd, th=th, night=night, strat_uz=False)


SWEEPS = {"A": lambda sat: sweep_a(), "B-Trs0": lambda sat: sweep_b(0.0, sat), "B-Trs50.2": lambda sat: sweep_b(50.2, sat),
          "C-lat0": lambda sat: sweep_c(0.0), "C-lat46.8": lambda sat: sweep_c(46.8), "C-lat70": lambda sat: sweep_c(70.0),
          "Cb-lat0": lambda sat: sweep_c(0.0, True), "Cb-lat46.8": lambda sat: sweep_c(46.8, True),
          "Cb-lat70": lambda sat: sweep_c(70.0, True)}


def get_sweep(name: str, satterlund: bool = False):
    return SWEEPS[name](bool(satterlund))


# ------------------------------------------------------------------------------------------- the oracle's probe
def recover(s, Eccs1, Ecci1):
    """(E_in, cold) from the cold contents after a step from the injected ECC0 (module docstring); cold is
    NaN where the sweep has no snowfall to read it from."""
    e_in = np.where(s.from_ecci, ECC0 - Ecci1, ECC0 - Eccs1)  # the masks broadcast over a leading step axis
    cold = np.where(s.cold_ok, (Eccs1 - ECC0) + e_in, np.nan)
    return e_in, cold


def oracle_probe(s, satterlund: bool = False, bump: tuple | None = None):
    """The oracle on every (step, point) of a sweep from the injected state: the probe's E_in and cold
    [steps][points], and the oracle's own terms.  bump = (input name, +-1) moves that fp32 input one ulp.
    Steps are laid side by side as cells of one oracle grid (its clock arguments broadcast per cell)."""
    cfg = dict(s.cfg, SATTERLUND=satterlund)
    p = dict(s.pts)
    if bump is not None:
        p[bump[0]] = f32_step(p[bump[0]], bump[1])
    keys = ("Q_sum", "Qn_SW", "Qn_LW", "Qh", "Qe", "RH", "h_swe", "h_ice", "n", "albedo", "Eccs", "Ecci")
    S, n = len(s.th), s.n
    out = {k: np.empty((S, n)) for k in keys + ("E_in", "cold")}
    per = max(1, 40000 // n)
    with np.errstate(all="ignore"):
        for k0 in range(0, S, per):
            rep = min(per, S - k0)
            t = {k: np.tile(v, rep) for k, v in p.items()}
            m = O.OracleGrid(cfg, elev=t["elev"], slope=t["slope"], aspect=t["aspect"], h0_snow=t["h_snow"],
                             h0_ice=t["h_ice"], h0_swe=t["h_swe"], h0_iwe=t["h_iwe"])
            m.n, m.albedo = t["n"].copy(), t["albedo"].copy()
            m.Eccs, m.Ecci = np.full(rep * n, ECC0), np.full(rep * n, ECC0)
            m.ring[:, -1] = t["ring"]
            r = m.step(*(t[v] for v in FORCING), np.repeat(s.jd[k0:k0 + rep], n), np.repeat(s.th[k0:k0 + rep], n))
            for key in keys:
                out[key][k0:k0 + rep] = np.asarray(r[key]).reshape(rep, n)
    out["E_in"], out["cold"] = recover(s, out["Eccs"], out["Ecci"])
    return out


@lru_cache(maxsize=None)
def reference(sweep: str, satterlund: bool):
    return oracle_probe(get_sweep(sweep, satterlund), satterlund)


def cold_formula(s, RH, satterlund: bool = False):
    """The snowfall's cold content by the reference's formula (:1507-1537), from the oracle's RH."""
    c = dict(O.CFG_DEFAULTS)
    c.update(s.cfg)
    Ta, P = s.pts["T_air"], s.pts["P"]
    with np.errstate(all="ignore"):
        T_wb = (Ta * np.arctan(0.151977 * ((RH + 8.313659) ** 0.5)) + np.arctan(Ta + RH) - np.arctan(RH - 1.676331)
                + ((0.00391838 * (RH ** 1.5)) * np.arctan(0.023101 * RH)) - 4.86035)
        ws = np.float64(c["rho_H2O"]) / np.float64(c["rho_snow"])
        return np.where(s.snowing, (np.float64(c["rho_snow"]) * np.float64(c["Cp_snow"])) * ((P * c["dt"]) * ws)
                        * (np.float64(c["T0"]) - T_wb), 0.0)


def wet_bulb_of(s, cold):
    """T_wb [degC] that a recovered cold content stands for (the formula inverted)."""
    c = dict(O.CFG_DEFAULTS)
    c.update(s.cfg)
    ws = c["rho_H2O"] / c["rho_snow"]
    with np.errstate(all="ignore"):
        return c["T0"] - cold / (c["rho_snow"] * c["Cp_snow"] * s.pts["P"] * c["dt"] * ws)


def strata(s):
    """[(label, step mask [steps], point mask [points])]: one uz value and one of day or night each."""
    out = []
    for j, uz in enumerate(s.uz_vals):
        for night in (True, False):
            steps = s.night == night
            if steps.any():
                out.append((f"uz={uz:g},{'night' if night else 'day'}", steps, s.uz_id == j))
    return out


def stratum_block(a, steps, pts):
    return a[np.ix_(steps, pts)]


@lru_cache(maxsize=None)
def parity_cut(sweep: str, satterlund: bool, tol: float):
    """The cut rule of the module docstring: (cut [steps][points] for E_in, cut for cold, the largest
    share cut of any stratum).  Non-finite reference points are not `cut`; see linear()."""
    s, ref = get_sweep(sweep, satterlund), reference(sweep, satterlund)
    worst = {k: np.zeros_like(ref[k]) for k in ("E_in", "cold")}
    T_rs = dict(O.CFG_DEFAULTS, **s.cfg)["T_rain_snow"]
    for name in FORCING + ("elev",):
        for d in (-1, 1):
            b = oracle_probe(s, satterlund, (name, d))
            # a move that takes T_air across the rain/snow threshold is no rounding error: the engine
            # decides T_air > T_rs exactly (the largest float <= T_rs), and the test holds it to that
            same = np.ones(s.n, bool) if name != "T_air" else \
                (f32_step(s.pts["T_air"], d) <= T_rs) == (s.pts["T_air"] <= T_rs)
            for k in worst:
                with np.errstate(invalid="ignore"):
                    worst[k] = np.fmax(worst[k], np.where(same[None, :], np.abs(b[k] - ref[k]), 0.0))
    cut = {k: np.zeros(ref[k].shape, bool) for k in worst}
    share = 0.0
    for _, steps, pts in strata(s):
        for k in worst:
            r = stratum_block(ref[k], steps, pts)
            ok = np.isfinite(r)
            if not ok.any():
                continue
            s_v = scale_floor(r[ok])
            with np.errstate(invalid="ignore"):
                c = ok & (stratum_block(worst[k], steps, pts) > 0.5 * tol * np.maximum(np.abs(r), s_v))
            cut[k][np.ix_(steps, pts)] = c
            share = max(share, c.sum() / ok.sum())
    return cut["E_in"], cut["cold"], share


def linear(s, ref):
    """[steps][points] True where the probe is in its linear range: the oracle's E_in finite and below
    ECC0 (with the cold content: ECC0 + cold - E_in > 0), and snow or ice left after the step."""
    with np.errstate(invalid="ignore"):
        ice = (ref["Ecci"] > 0) & (ref["h_ice"] > 0)
        snow = (ref["Eccs"] > 0) & (ref["h_swe"] > 0)
    ok = np.where(s.from_ecci[None, :], ice & (snow | ~s.cold_ok[None, :]), snow)
    return np.isfinite(ref["E_in"]) & ok


# ------------------------------------------------------------------------------------------- layouts
def classes(s, ref):
    """Per point, the wave-uniform branches it takes: snowing | RH off the wet bulb's fits | the flux
    form's rare exp_p path | dark at the sweep's middle step (only there: over the other steps of
    sweep C the sorted layout's waves are not uniform in dark)."""
    c = dict(O.CFG_DEFAULTS)
    c.update(s.cfg)
    RH = ref["RH"][0]
    with np.errstate(invalid="ignore"):
        off = ~((RH >= 0) & (RH <= 5))
        y = c["M_mass_air"] * c["g"] * s.pts["elev"] / (c["uni_gas_const"] * (s.pts["T_air"] + 273.15))
        rare = ~(np.abs(y + 0.345) <= 0.41)
    k = len(s.th) // 2
    dark = ref["Qn_SW"][k] == 0
    return s.snowing.astype(int) + 2 * off.astype(int) + 4 * rare.astype(int) + 8 * dark.astype(int)


def layouts(s, ref, seed: int = 20260101):
    """(sorted, interleaved): arrays of point indices, a multiple of 64 long; lane i of the grid holds
    point layout[i].  sorted: each class padded to whole waves (with repeats of its last point), so every
    wave is uniform.  interleaved: a random permutation (padded), then, per class, up to four waves of 63
    points of other classes with ONE lane of that class at a random position."""
    return layouts_of(classes(s, ref), seed)


def layouts_of(cls, seed: int = 20260101):
    """layouts() for any per-point class array."""
    cls = np.asarray(cls)
    s = SimpleNamespace(n=len(cls))
    rng = np.random.default_rng(seed)

    def pad(a):
        a = np.asarray(a, np.int64)
        return np.concatenate([a, np.full((-len(a)) % WAVE, a[-1])])

    srt = np.concatenate([pad(np.nonzero(cls == c)[0]) for c in np.unique(cls)])
    parts = [pad(rng.permutation(s.n))]
    if len(np.unique(cls)) > 1:
        for c in np.unique(cls):
            own, others = np.nonzero(cls == c)[0], np.nonzero(cls != c)[0]
            for _ in range(4):
                w = rng.choice(others, WAVE, replace=len(others) < WAVE)
                w[rng.integers(WAVE)] = rng.choice(own)
                parts.append(w)
    return srt, np.concatenate(parts)


# ------------------------------------------------------------------------------------------- the engine's probe
def probe_clock(s):
    """A StepClock whose calendar is given: step k is (jd[k], th[k])."""
    from topoflow_glacier.physics.clock import StepClock

    class _Clock(StepClock):
        def calendar(self, k0, n):
            z = np.zeros(n)
            return s.jd[k0:k0 + n], z.astype(np.int64), z, s.th[k0:k0 + n]

    c = s.cfg
    return _Clock(c["start_time"], c["dt"], c["lat"], c["lon"], c["time_zone"])


def gpu_probe(s, engine: str, satterlund: bool, nan_safe, layout, ecc=None, extra=(), follow: int = 0, catch=None):
    """One engine step per sweep step on the grid `layout` (1 x len(layout)), state re-injected before
    each; returns, per name in READ + OUTS, [steps][len(layout)] as read back, and E_in, cold by recover().
    The step writes window slot 0 each time and slot 1 holds the snowfall already in the window, so the
    window's total is the same at every step.

    ecc = (Eccs, Ecci), per point: the injected cold contents instead of ECC0 (E_in and cold are then not
    returned).  extra: further fields to read back.  follow: that many further steps after each, from
    the state the step left (same clock, forcing and window slot), read back as "<name>@<j>".  catch =
    (ids per point, n_catch): a catchment raster; the diagnostics are reset before every injected step
    and returned as "diag" [steps][n_catch][6] after it and as "diag@<j>"."""
    lay = np.asarray(layout)
    n = len(lay)
    p = {k: np.ascontiguousarray(v[lay]) for k, v in s.pts.items()}
    cfg = dict(s.cfg, SATTERLUND=satterlund)
    clock = probe_clock(s)
    names = READ + OUTS + tuple(extra)
    e = make_engine(cfg, 1, n, engine, n_frames=1, hist_depth=1, fuse_steps=1, n_catch=1 if catch is None else catch[1])
    out = {k: np.empty((len(s.th), n)) for k in names + tuple(f"{v}@{j}" for v in names for j in range(1, follow + 1))}
    if catch is not None:
        out.update({k: np.empty((len(s.th), catch[1], 6)) for k in ["diag"] + [f"diag@{j}" for j in range(1, follow + 1)]})
    try:
        for k in ("elev", "slope", "aspect", "h_snow", "h_ice", "h_swe", "h_iwe"):
            e.set_field(k, p[k])
        if catch is not None:
            e.set_field("catch_id", np.ascontiguousarray(np.asarray(catch[0])[lay], dtype=np.int32))
        e.init_state()
        if nan_safe is not None:
            e.set_step_form(bool(nan_safe))
        e.set_inputs(np.stack([p[v] for v in ("P_air", "Hum_sp", "P", "T_air", "uz")]), 0)
        e.set_field("window", p["ring"], index=1)
        inj = {"Eccs": np.full(n, ECC0), "Ecci": np.full(n, ECC0)} if ecc is None else \
            {"Eccs": np.ascontiguousarray(ecc[0][lay]), "Ecci": np.ascontiguousarray(ecc[1][lay])}
        for k in range(len(s.th)):
            for name in STATE:
                e.set_field(name, inj[name] if name in inj else p[name])
            if catch is not None:
                e.reset_diagnostics()
            u = clock.uniforms(k, 1)
            u["frame"], u["hist"], u["slot"] = 0, 0, 0
            for j in range(follow + 1):
                e.run(1, uniforms=u)
                e.sync()
                tag = f"@{j}" if j else ""
                for name in names:
                    out[name + tag][k] = e.get_field(name)
                if catch is not None:
                    out["diag" + tag][k] = e.diagnostics()
    finally:
        e.close()
    if ecc is None:
        sl = SimpleNamespace(from_ecci=s.from_ecci[lay], cold_ok=s.cold_ok[lay])
        out["E_in"], out["cold"] = recover(sl, out["Eccs"], out["Ecci"])
    return out


def first_lane(layout, n_points):
    """For each point, the first lane of `layout` that holds it."""
    first = np.full(n_points, -1)
    lay = np.asarray(layout)
    first[lay[::-1]] = np.arange(len(lay))[::-1]
    assert (first >= 0).all()
    return first


# ------------------------------------------------------------------------------------------- the one-cell kernels' probe
def with_steps(s, steps):
    """The sweep with only the steps `steps` (indices, in that order)."""
    sub = SimpleNamespace(**vars(s))
    sub.jd, sub.th, sub.night = s.jd[steps], s.th[steps], s.night[steps]
    return sub


def pad_to_waves(points):
    """Point indices padded to whole waves with repeats of the last, as layouts() pads."""
    a = np.asarray(points, np.int64)
    return np.concatenate([a, np.full((-len(a)) % WAVE, a[-1])])


def cb_near(s):
    """[steps][points] of a bracket sweep (Cb-lat*): True where the step is within C_NEAR of the point's own
    sunrise or sunset for the step's jd, computed with _sun_offsets as sweep_c places the steps."""
    lat = dict(O.CFG_DEFAULTS, **s.cfg)["lat"]
    m = O.OracleGrid(s.cfg, elev=s.pts["elev"], slope=s.pts["slope"], aspect=s.pts["aspect"], h0_snow=0.0, h0_ice=0.0,
                     h0_swe=0.0, h0_iwe=0.0)
    near = np.zeros((len(s.th), s.n), bool)
    for jd in np.unique(s.jd[1:]):
        ks = np.nonzero(s.jd == jd)[0]
        ks = ks[ks > 0]
        sr, ss = _sun_offsets(lat, jd, m.alpha, m.beta)
        th = s.th[ks][:, None]
        with np.errstate(invalid="ignore"):
            near[ks] = (np.abs(th - sr[None, :]) <= C_NEAR) | (np.abs(th - ss[None, :]) <= C_NEAR)
    return near


@lru_cache(maxsize=None)
def one_cell_sample(sweep: str, satterlund: bool = False):
    """The (point, step) pairs [N][2] of a sweep that the one-cell kernels step one launch each, sorted by
    point, then step; deterministic (default_rng(SAMPLE_SEED)).

      A         both steps of one point, drawn at random, of every combination present of classes() value x
                surface (A_SURF) x wind (A_UZ) x (T_air > 0), and of every point with T_air == 0 at uz = 3
      B-Trs*    every point (one step)
      C-lat*    the dark step and the 48 hourly steps of days 171 and 354, for every albedo state at slope
                0.5 and aspects 0, 90, 180 and 270
      Cb-lat*   every (slope, aspect) cell at albedo state 5 (aged snow in warm air): the dark step and the
                steps within C_NEAR of that cell's own sunrise or sunset (cb_near)"""
    s = get_sweep(sweep, satterlund)
    rng = np.random.default_rng(SAMPLE_SEED)
    S = len(s.th)
    if sweep == "A":
        ref = reference(sweep, satterlund)
        _, surf = np.unique(np.stack([s.pts["h_snow"], s.pts["h_ice"]]), axis=1, return_inverse=True)
        key = np.stack([classes(s, ref), surf.reshape(-1), s.uz_id, (s.pts["T_air"] > 0).astype(np.int64)])
        _, combo = np.unique(key, axis=1, return_inverse=True)
        combo = combo.reshape(-1)
        pts = [int(rng.choice(np.nonzero(combo == c)[0])) for c in range(combo.max() + 1)]
        pts += list(np.nonzero((s.pts["T_air"] == 0) & (s.pts["uz"] == 3.0))[0])
        pairs = [(p, k) for p in np.unique(pts) for k in range(S)]
    elif sweep.startswith("B"):
        pairs = [(p, 0) for p in range(s.n)]
    elif sweep.startswith("Cb"):
        near = cb_near(s)
        state5 = np.nonzero(s.pts["h_snow"] > 0)[0]  # C_BRACKET_ALB = (5, 8): state 8 is bare ice
        pairs = [(p, k) for p in state5 for k in [0] + list(np.nonzero(near[:, p])[0])]
    else:
        days = [1 + 24 * C_DAYS.index(d) for d in (171.0, 354.0)]
        steps = [0] + [d0 + h for d0 in days for h in range(24)]
        sel = np.nonzero((s.pts["slope"] == 0.5) & np.isin(s.pts["aspect"], (0.0, 90.0, 180.0, 270.0)))[0]
        pairs = [(p, k) for p in sel for k in steps]
    out = np.array(sorted(set((int(p), int(k)) for p, k in pairs)), dtype=np.int64).reshape(-1, 2)
    out.setflags(write=False)
    return out


def one_cell_engine(cfg, n_catch: int = 1, cell_catchment: int | None = None, shared_stream: bool = False):
    """A 1 x 1 float64 handle with one frame and one history slot, initialised with no snow and no ice
    (inject_point sets the point).  cell_catchment: the catchment (of n_catch) the cell sits in.
    init_state() runs before any static is set and is not repeated when inject_point changes them: set_field
    of elev, slope or aspect marks the handle's static planes stale, and the next launch derives them again
    (the C sweeps' bits against the grid kernel depend on it)."""
    e = make_engine(cfg, 1, 1, "float64", n_frames=1, hist_depth=1, n_catch=n_catch)
    try:
        if cell_catchment is not None:
            e.set_field("catch_id", np.array([cell_catchment], dtype=np.int32))
        e.init_state()
        if shared_stream:
            from topoflow_glacier.bmi import bmi_topoflow_glacier as B

            e.set_stream(B._shared_stream(0))
    except Exception:
        e.close()
        raise
    return e


def inject_point(e, s, i: int, statics: bool = True, ecc=None) -> None:
    """Point i of the sweep into a one-cell handle: its statics (unless the handle holds them), the injected
    state (ECC0 in both cold contents, or ecc = (Eccs, Ecci) per point) and window slot 1."""
    one = lambda a: np.ascontiguousarray(a[i:i + 1], dtype=np.float64)  # noqa: E731
    if statics:
        for k in ("elev", "slope", "aspect"):
            e.set_field(k, one(s.pts[k]))
    inj = {"Eccs": np.full(1, ECC0), "Ecci": np.full(1, ECC0)} if ecc is None else {"Eccs": one(ecc[0]), "Ecci": one(ecc[1])}
    for name in STATE:
        e.set_field(name, inj[name] if name in inj else one(s.pts[name]))
    e.set_field("window", one(s.pts["ring"]), index=1)


def point_inputs(s, i: int) -> np.ndarray:
    return np.array([[s.pts[v][i]] for v in IN_ORDER], dtype=np.float64)


def probe_uniform(clock, k: int):
    """Step k's uniform record with frame = hist = slot = 0, as gpu_probe makes it."""
    u = clock.uniforms(k, 1)
    u["frame"], u["hist"], u["slot"] = 0, 0, 0
    return np.ascontiguousarray(u)


def update_one(e, values, u, out) -> None:
    """tfg_update (k_cell) with the caller's uniform record."""
    from topoflow_glacier import _native as nat

    e._chk(e.lib.tfg_update(e.h, 0, values.ctypes.data, nat.F64, u.ctypes.data, out.ctypes.data, nat.F64, 1))


def update_batch(engines, values, us, outs) -> None:
    """tfg_update_many (k_cell_many, one launch) with the caller's uniform records, as UpdateBatch.run calls it."""
    import ctypes

    from topoflow_glacier import _native as nat

    m = len(engines)
    arr = ctypes.c_void_p * m
    nat.check(engines[0].lib.tfg_update_many(arr(*[e.h.value for e in engines]), m, arr(*[v.ctypes.data for v in values]),
                                             arr(*[u.ctypes.data for u in us]), arr(*[o.ctypes.data for o in outs])))


def gpu_probe_one_cell(s, kernel: str, satterlund: bool, point_steps, handles: list | None = None, ecc=None, extra=(),
                       follow: int = 0):
    """The (point, step) pairs `point_steps` [N][2], each one launch of a one-cell kernel from the injected
    state (the read_depths = 1 entry: the depths are set before every step): per name in READ + OUTS + E_in +
    cold, [N] as gpu_probe returns them per (step, lane); READ from the handle's state, OUTS from the
    call's output block.  "k_cell": one handle, reused over the points; "k_cell_many": up to MANY_POOL
    handles on the BMI's shared stream, each holding a run of consecutive pairs, all stepped once per
    launch.  `handles` (a list) receives, per handle, (diagnostics [1][6], the P it was fed, in order, and
    T_air).  ecc, extra: as gpu_probe's (extra: further state fields).  follow: that many further steps of
    each pair on the same handle, from the state its own step left (no injection; same inputs and uniform
    record), read back as "<name>@<j>"."""
    assert kernel in ONE_CELL_KERNELS, kernel
    ps = np.asarray(point_steps, np.int64).reshape(-1, 2)
    N = len(ps)
    cfg = dict(s.cfg, SATTERLUND=satterlund)
    clock = probe_clock(s)
    urec = {int(k): probe_uniform(clock, int(k)) for k in np.unique(ps[:, 1])}
    res = {k + (f"@{f}" if f else ""): np.empty(N) for k in READ + OUTS + tuple(extra) for f in range(follow + 1)}
    m = 1 if kernel == "k_cell" else min(N, MANY_POOL)
    per = -(-N // m)  # handle j steps pairs j per ... (j + 1) per - 1, one per launch
    engines, fed = [], [[] for _ in range(m)]
    try:
        for _ in range(m):
            engines.append(one_cell_engine(cfg, shared_stream=kernel == "k_cell_many"))
        holds = [-1] * m
        outs = [np.empty((8, 1)) for _ in range(m)]
        for b in range(per):
            js = [j for j in range(m) if j * per + b < min(N, (j + 1) * per)]
            vals = []
            for j in js:
                i, k = ps[j * per + b]
                inject_point(engines[j], s, i, statics=holds[j] != i, ecc=ecc)
                holds[j] = i
                vals.append(point_inputs(s, i))
                fed[j].append((s.pts["P"][i], s.pts["T_air"][i]))
            us = [urec[int(ps[j * per + b, 1])] for j in js]
            for f in range(follow + 1):
                tag = f"@{f}" if f else ""
                if kernel == "k_cell":
                    update_one(engines[0], vals[0], us[0], outs[0])
                else:
                    update_batch([engines[j] for j in js], vals, us, [outs[j] for j in js])
                for j in js:
                    q = j * per + b
                    for name in READ + tuple(extra):
                        res[name + tag][q] = engines[j].get_field(name)[0]
                    for name in OUTS:
                        res[name + tag][q] = outs[j][OUT_ROW[name], 0]
                    if f:
                        fed[j].append((s.pts["P"][ps[q, 0]], s.pts["T_air"][ps[q, 0]]))
        if handles is not None:
            handles += [(e.diagnostics(), np.array([f[0] for f in fd]), np.array([f[1] for f in fd]))
                        for e, fd in zip(engines, fed)]
    finally:
        for e in engines:
            e.close()
    if ecc is None:
        sl = SimpleNamespace(from_ecci=s.from_ecci[ps[:, 0]], cold_ok=s.cold_ok[ps[:, 0]])
        res["E_in"], res["cold"] = recover(sl, res["Eccs"], res["Ecci"])
    return res


def fed_diagnostics(cfg, P, T_air):
    """vol_P, vol_PR, vol_PS, P_max of a handle fed the steps (P, T_air) in order: the fp64 sums, in that
    order, of P da dt (:558-624; da in m2, dt in the config's hours, as harness.catchment_diag has them)."""
    c = dict(O.CFG_DEFAULTS)
    c.update(cfg)
    da_m2, dt = np.float64(c["da"]) * 1e6, np.float64(c["dt"])
    tot = np.zeros(3)
    for p, t in zip(P, T_air):
        rain = 1.0 if t > c["T_rain_snow"] else 0.0
        tot += np.array([p, p * rain, p * (1.0 - rain)]) * da_m2 * dt
    return np.array([tot[0], tot[1], tot[2], np.max(P) if len(P) else 0.0])


# ------------------------------------------------------------------------------------------- melt states
# The other half of the step: from E_in and the state to SM, IM, M_total, the new depths and cold contents
# (:1321-1731; tfg_oracle.py:511-571).  Forcing points of sweep A crossed with a state grid built from the
# oracle's own E_in and snowfall cold content, so that every gate of the tail is taken on both sides and
# none is decided by rounding (melt_margins); a one-point sweep of residual depths for the melt-out bits.
#
# Notation.  E: the oracle's E_in = Q_sum dt at the cell's own state; cold: its snowfall cold content;
# G = E - cold where it snows, else E; c = 3600 / (dt rho_H2O Lf) [m of water per J m-2: a depth is
# "energy-equivalent" when divided by c]; m_s = max(E - Eccs0, 0) c and m_i = max(E - Ecci0, 0) c: the
# depths one step could melt; S = max(|E|, |cold|, s_v dt): the scale of the parity tolerance at the cell,
# s_v being the floor of the point's stratum in sweep A (whose dt is 1).
#
# Placement of the "just below / just above" values.  The parity tolerance admits an E_in error of
# tol S in every fp32 form, and E - Eccs0 cancels: a threshold placed at m_s (1 +- 1e-3) is 1e-3 m_s away
# from the gate, which is less than the admitted error wherever m_s < 1e-2 S c (Eccs0 itself within 1e-3
# of G, or a point whose E at this state is below its stratum's floor).  So every +- value is placed
# MELT_OFF max(|q|, S) from its threshold q, in energy-equivalent units (the depths': max(|q|, 0.6 S)): equal
# to q (1 +- 1e-3) wherever |q| >= S, never closer than 0.6 MELT_OFF S, and every gate then clears MELT_MARGIN S
# = 10 x the fp32 tolerance by construction.  A value that would be negative is 0.
MELT_DTS = (1.0, 2.0, 0.25)
MELT_MARGIN = 1e-4            # no gate quantity closer than this (x S) to its threshold
MELT_OFF = 1e-3               # the +- values' distance from their threshold
MELT_P = float(np.float32(2e-5))  # precipitation of the snowing and raining points: P dt ws << 0.03 m, so n is not reset
DRY, SNOW, RAIN = 0, 1, 2
# (uz of the stratum, night, sign of the sweep's E_in, T_air > 0, precipitation).  A stratum's points at or
# above its floor are what its wind allows: warm nights and days in calm air and at 3 m/s, cold nights
# (E_in < 0) from 0.05 m/s on; E_in > 0 in air at or below 0 degC (snowfall on a melting surface) only in
# the calm day; no stratum has E_in < 0 in warm air at its floor, so "negative and raining" has no point.
# The cold points are night steps: by day a cold point's E_in can be negative under snow and positive on bare
# ground (the albedo), and a grid placed from the cell's own E_in then has no fixed point (melt_case).
MELT_WANTS = ((0.0, True, 1, True, RAIN), (0.0, True, 1, True, DRY), (0.0, False, 1, False, SNOW), (0.0, False, 1, False, DRY),
              (0.0, False, 1, True, RAIN), (0.05, True, -1, False, SNOW), (0.28, False, -1, False, DRY),
              (3.0, True, -1, False, SNOW), (15.8, False, 1, True, RAIN), (40.0, True, 1, True, DRY),
              (3.0, False, 1, True, DRY), (0.28, True, -1, False, SNOW))
MELT_AXES = (5, 5, 6, 6)      # Eccs0, Ecci0, h_swe0, h_iwe0 values per point
MELT_TAIL_OUT = ("SM", "IM", "M_total", "h_swe", "h_iwe", "Eccs", "Ecci", "h_snow", "h_ice", "vol_SM", "vol_IM")
SWEEP_N = 4096                # residual depths of the melt-out sweep
SWEEP_RANGE = (1e-9, 1e-3)    # [m], log-uniform


def _cfgc(cfg):
    c = dict(O.CFG_DEFAULTS)
    c.update(cfg)
    return c


def melt_c(cfg):
    """c = 3600 / (dt rho_H2O Lf), rounded as the fp32 engine's c_sm3600."""
    c = _cfgc(cfg)
    return 3600.0 / (np.float64(c["dt"]) * (np.float64(c["rho_H2O"]) * np.float64(c["Lf"])))


@lru_cache(maxsize=None)
def melt_points(satterlund: bool = False):
    """The forcing points: per entry of MELT_WANTS one point of sweep A, drawn (default_rng(SAMPLE_SEED)) from
    those of its stratum whose oracle |E_in| (the sweep's own state) is at least the stratum's scale_floor
    and has the wanted sign, in air of the wanted side of 0 degC.  idx, step, kind, floor: [points]."""
    s, ref = get_sweep("A", satterlund), reference("A", satterlund)
    rng = np.random.default_rng(SAMPLE_SEED)
    idx, step, kind, floor, e_ref = [], [], [], [], []
    for uz, night, sign, warm, k in MELT_WANTS:
        pts = s.uz_id == int(np.nonzero(s.uz_vals == f32(uz))[0][0])
        steps = s.night == night
        ks = int(np.nonzero(steps)[0][0])
        blk = stratum_block(ref["E_in"], steps, pts)
        sv = scale_floor(blk[np.isfinite(blk)])
        e = ref["E_in"][ks]
        with np.errstate(invalid="ignore"):
            cand = np.nonzero(pts & np.isfinite(e) & (np.abs(e) >= sv) & (np.sign(e) == sign) & ((s.pts["T_air"] > 0) == warm))[0]
        assert len(cand), (uz, night, sign, warm)
        i = int(rng.choice(cand))
        idx.append(i), step.append(ks), kind.append(k), floor.append(sv), e_ref.append(e[i])
    return SimpleNamespace(idx=np.array(idx), step=np.array(step), kind=np.array(kind), floor=np.array(floor),
                           e_ref=np.array(e_ref))


def snowfall_cold(cfg, P_snow, T_air, RH):
    """The snowfall's cold content as tfg_oracle.py:531-543 forms it (same operations, same order)."""
    c = _cfgc(cfg)
    with np.errstate(all="ignore"):
        new_h_snow = (P_snow * c["dt"]) * (np.float64(c["rho_H2O"]) / np.float64(c["rho_snow"]))
        T_wb = (T_air * np.arctan(0.151977 * ((RH + 8.313659) ** 0.5)) + np.arctan(T_air + RH) - np.arctan(RH - 1.676331)
                + ((0.00391838 * (RH**1.5)) * np.arctan(0.023101 * RH)) - 4.86035)
        del_T = np.float64(c["T0"]) - T_wb
        return np.where(P_snow > 0, (np.float64(c["rho_snow"]) * np.float64(c["Cp_snow"])) * new_h_snow * del_T, 0.0)


def melt_oracle(case, st):
    """One OracleGrid.step of every cell of a melt case from the state `st` (h_swe, h_iwe, Eccs, Ecci; the
    depths follow): the step's result, with E_in, cold, P_snow, P_rain, vol_SM and vol_IM (the cell's terms
    of the two integrals) added."""
    c, p = _cfgc(case.cfg), case.pts
    ws, wi = np.float64(c["rho_H2O"]) / np.float64(c["rho_snow"]), np.float64(c["rho_H2O"]) / np.float64(c["rho_ice"])
    m = O.OracleGrid(dict(case.cfg, SATTERLUND=case.sat), elev=p["elev"], slope=p["slope"], aspect=p["aspect"],
                     h0_snow=st["h_swe"] * ws, h0_ice=st["h_iwe"] * wi, h0_swe=st["h_swe"], h0_iwe=st["h_iwe"])
    m.n, m.albedo = p["n"].copy(), p["albedo"].copy()
    m.Eccs, m.Ecci = np.array(st["Eccs"], np.float64), np.array(st["Ecci"], np.float64)
    return m, _oracle_step(case, m)


def _oracle_step(case, m):
    p = case.pts
    with np.errstate(all="ignore"):
        m.cell_vol_SM = m.cell_vol_IM = np.float64(0.0)  # this step's terms alone (the sums are the test's)
        r = dict(m.step(*(p[v] for v in FORCING), case.jd_cell, case.th_cell))
    r["E_in"] = r["Q_sum"] * m.dt
    T_rs = np.float64(m.c["T_rain_snow"])
    r["P_snow"], r["P_rain"] = p["P"] * (p["T_air"] <= T_rs), p["P"] * (p["T_air"] > T_rs)
    r["cold"] = snowfall_cold(case.cfg, r["P_snow"], p["T_air"], r["RH"])
    r["vol_SM"], r["vol_IM"] = m.cell_vol_SM, m.cell_vol_IM
    return {k: np.array(v, copy=True) for k, v in r.items() if np.ndim(v) == 1}  # the per-cell results


def melt_tail(cfg, E_in, cold, P_snow, P_rain, st, variant: str):
    """The step's tail alone, fp64 numpy: from E_in, the snowfall's cold content and the state (h_swe, h_iwe,
    Eccs, Ecci, h_ice: the depth before the step) to MELT_TAIL_OUT, plus the gate quantities ("gates").

    "reference"  tfg_oracle.py:511-571 line by line.
    "fast"       melt_core / melt_fast of the fp32 engine (tfg_physics.hpp): SM 3600 = E_rem c_sm3600 with
                 c_sm3600 = 3600 / (dt rho_H2O Lf); IM = E_rem inv_dt_rhoLf; the cap h_iwe inv_dt; t (1/3600.)
                 for t / 3600; dt3600 = dt 3600 folded into one factor; the SM integral from the fp32 E_rem
                 with the folded factor, the IM integral from the fp32 IM; SM, IM rounded to fp32 and M_total
                 summed in fp32, as the history holds them (h_snow, h_ice stay fp64: the state's)."""
    c = _cfgc(cfg)
    dt = np.float64(c["dt"])
    rho_H2O, Lf = np.float64(c["rho_H2O"]), np.float64(c["Lf"])
    ws, wi = rho_H2O / np.float64(c["rho_snow"]), rho_H2O / np.float64(c["rho_ice"])
    da_m2 = c["da"] * 1e6
    zero = np.float64(0)
    h_swe0, h_iwe0, Eccs0, Ecci0, h_ice0 = (np.asarray(st[k], np.float64) for k in ("h_swe", "h_iwe", "Eccs", "Ecci", "h_ice"))
    E_in, cold, P_snow, P_rain = (np.asarray(a, np.float64) for a in (E_in, cold, P_snow, P_rain))
    previous_swe = h_swe0
    E_rem_s = np.maximum(E_in - Eccs0, zero)
    E_rem_i = np.maximum(E_in - Ecci0, zero)
    avail = h_swe0 + P_snow * dt
    if variant == "reference":
        SM = (E_rem_s / dt) / (rho_H2O * Lf)
        SM = np.maximum(SM, zero)
        vol_SM = SM * da_m2 * dt * 3600
        sm3600 = SM * 3600
        t = np.minimum(sm3600, avail)
        SM = t / 3600
        h_swe = np.maximum(avail - SM * dt * 3600, zero)
        IM = np.maximum((E_rem_i / dt) / (rho_H2O * Lf), zero)
        IM = np.where((h_swe == 0) & (previous_swe == 0), IM, zero)
        im_gated = IM
        IM = np.maximum(np.minimum(IM, h_iwe0 / dt), zero)
        vol_IM = IM * da_m2 * dt * 3600
        im3600 = IM * 3600
        t = np.minimum(im3600, h_iwe0)
        IM = t / 3600
        h_iwe = np.maximum(h_iwe0 - IM * dt * 3600, zero)
        M_total = IM + SM + P_rain / 3600
    elif variant == "fast":
        c_sm3600, inv_dt_rhoLf = 3600.0 / (dt * (rho_H2O * Lf)), 1.0 / (dt * (rho_H2O * Lf))
        inv_dt, dt3600, inv3600 = 1.0 / dt, dt * 3600.0, 1.0 / 3600.0
        vol_SM = E_rem_s.astype(np.float32).astype(np.float64) * (inv_dt_rhoLf * da_m2 * dt * 3600.0)
        sm3600 = E_rem_s * c_sm3600
        SM = np.minimum(sm3600, avail) * inv3600
        h_swe = np.maximum(avail - SM * dt3600, zero)
        IM = np.where((h_swe == 0) & (previous_swe == 0), E_rem_i * inv_dt_rhoLf, zero)
        im_gated = IM
        IM = np.minimum(IM, h_iwe0 * inv_dt)
        vol_IM = IM.astype(np.float32).astype(np.float64) * (da_m2 * dt * 3600.0)
        im3600 = IM * 3600.0
        IM = np.minimum(im3600, h_iwe0) * inv3600
        h_iwe = np.maximum(h_iwe0 - IM * dt3600, zero)
        SM, IM = SM.astype(np.float32), IM.astype(np.float32)
        M_total = (IM + SM + P_rain.astype(np.float32) * (np.float32(1.0) / np.float32(3600.0))).astype(np.float64)
        SM, IM = SM.astype(np.float64), IM.astype(np.float64)
    else:
        raise ValueError(variant)
    Eccs = np.where(P_snow > 0, np.maximum((Eccs0 + cold) - E_in, zero), Eccs0)
    Ecci = np.where(h_ice0 == 0, zero, np.maximum(Ecci0 - E_in, zero))
    h_snow, h_ice = h_swe * ws, h_iwe * wi
    Eccs = np.where(P_snow <= 0, np.maximum(Eccs - E_in, zero), Eccs)
    Eccs = np.where(h_snow == 0, zero, Eccs)
    out = dict(SM=SM, IM=IM, M_total=M_total, h_swe=h_swe, h_iwe=h_iwe, Eccs=Eccs, Ecci=Ecci, h_snow=h_snow, h_ice=h_ice,
               vol_SM=vol_SM, vol_IM=vol_IM)
    out["gates"] = dict(E_rem_s=E_rem_s, E_rem_i=E_rem_i, avail=avail, sm3600=sm3600, im_gated=im_gated, im3600=im3600,
                        capped=(sm3600 >= avail) & (avail > 0))
    return out


def melt_decisions(o, capped=None):
    """The tail's decisions as they show in its results: which of SM, IM, Eccs, Ecci, h_swe, h_iwe are zero,
    and `capped` (SM 3600 == the snow available, avail > 0: given, or from the restatement's gates)."""
    d = {f"{k}==0": np.asarray(o[k]) == 0 for k in ("SM", "IM", "Eccs", "Ecci", "h_swe", "h_iwe")}
    d["capped"] = np.asarray(o["gates"]["capped"] if capped is None else capped)
    return d


def melt_margins(case, ref, st):
    """Per gate of the tail, [cells]: the oracle's distance from the threshold in energy-equivalent units,
    divided by S; inf where the gate is not reached (its outcome is fixed by gates before it) or where both
    sides are exactly zero (both outcomes give the same result).  A cell is decidable when all are >=
    MELT_MARGIN.  Gates: E - Eccs0 and E - Ecci0 (the melt gates; without snowfall also Eccs's survival);
    G - Eccs0 (Eccs's survival under snowfall); SM 3600 against the snow available (the cap) and SM 3600 dt
    against it (melt-out when not capped); IM against h_iwe / dt, IM 3600 against h_iwe, IM 3600 dt against
    h_iwe, where the ice gate is open."""
    c = melt_c(case.cfg)
    dt = np.float64(case.cfg["dt"])
    t = melt_tail(case.cfg, ref["E_in"], ref["cold"], ref["P_snow"], ref["P_rain"], dict(st, h_ice=st["h_iwe"]), "reference")
    g = t["gates"]
    S = case.S(ref)
    inf = np.full(case.n, np.inf)

    def dist(a, b, live):
        d = np.abs(np.asarray(a) - np.asarray(b))
        return np.where(live & ~((np.asarray(a) == 0) & (np.asarray(b) == 0)), d / S, inf)

    on = np.ones(case.n, bool)
    snowing = ref["P_snow"] > 0
    m_s, m_i = g["sm3600"], g["im_gated"] * 3600
    ice_open = g["im_gated"] > 0
    return {"E-Eccs0": dist(ref["E_in"], st["Eccs"], on),
            "E-Ecci0": dist(ref["E_in"], st["Ecci"], on),
            "G-Eccs0": dist(ref["E_in"] - ref["cold"], st["Eccs"], snowing),
            "cap": dist(m_s / c, g["avail"] / c, m_s > 0),
            "melt-out": dist(m_s * dt / c, g["avail"] / c, (m_s > 0) & (m_s < g["avail"])),
            "ice rate cap": dist(m_i / c, st["h_iwe"] * 3600 / dt / c, ice_open),  # IM = m_i / 3600 against h_iwe / dt
            "ice cap": dist(m_i / c, st["h_iwe"] / c, ice_open),
            "ice melt-out": dist(m_i * dt / c, st["h_iwe"] / c, ice_open & (m_i < st["h_iwe"]))}


def _melt_states(case, E, cold):
    """The state grid from (E, cold) per cell: the comment at the head of this section."""
    a, b, sw, iw = case.ax
    dt, c = np.float64(case.cfg["dt"]), melt_c(case.cfg)
    S = np.maximum(np.maximum(np.abs(E), np.abs(cold)), case.floor)
    G = np.abs(np.where(case.snowing, E - cold, E))
    Ea = np.abs(E)

    def five(q, k):
        off = MELT_OFF * np.maximum(q, S)
        return np.maximum(np.choose(k, [0.0 * q, q / 2, q - off, q + off, 2 * q]), 0.0)

    Eccs0, Ecci0 = five(G, a), five(Ea, b)
    m_s, m_i = np.maximum(E - Eccs0, 0.0) * c, np.maximum(E - Ecci0, 0.0) * c
    # 0.6 S for the depths: where Eccs0 = G - MELT_OFF S (m = MELT_OFF S c), m +- MELT_OFF S c would be 0 and 2 m, the
    # melt-out threshold at dt = 2; m (1 +- 0.6) is MELT_MARGIN S c or more from m, 2 m and m / 4
    off_s, off_i = MELT_OFF * np.maximum(m_s, 0.6 * S * c), MELT_OFF * np.maximum(m_i, 0.6 * S * c) * dt
    fall = np.where(case.snowing, case.pts["P"] * dt, 0.0)
    # what is available after the snowfall: h_swe0 = target - P_snow dt (0 where the snowfall alone exceeds it)
    target = np.choose(sw, [0.0 * m_s, 0.0 * m_s, m_s / 2, m_s - off_s, m_s + off_s, 10 * m_s + 1])
    h_swe0 = np.where(sw == 0, 0.0, np.where(sw == 1, 1e-12, np.maximum(target - fall, 0.0)))
    # h_iwe0: none; half of what the rate cap IM <= h_iwe / dt admits (IM = m_i / 3600: the cap binds); the
    # melt-out threshold m_i dt: 0.4 of it (half of it is the cap min(IM 3600, h_iwe)'s own threshold at dt = 2:
    # a tie), just below and just above it; plenty
    h_iwe0 = np.maximum(np.choose(iw, [0.0 * m_i, m_i * dt / 7200, 0.4 * m_i * dt, m_i * dt - off_i, m_i * dt + off_i, 10 * m_i + 1]), 0.0)
    return dict(h_swe=h_swe0, h_iwe=h_iwe0, Eccs=Eccs0, Ecci=Ecci0)


@lru_cache(maxsize=None)
def melt_case(satterlund: bool, dt: float):
    """The melt-state case of one (vapour-pressure form, dt): every point of melt_points() crossed with the
    state grid.  pts: per cell, as a sweep's (the state's depths, n, albedo and window included, so that
    gpu_probe and gpu_probe_one_cell inject them); st: the injected h_swe, h_iwe, Eccs, Ecci; ref: the
    oracle's step from that state (melt_oracle); jd, th: the sweep's two clock steps, step_cell the one each
    cell is compared at.  The grid is placed from the oracle's E_in and cold at the cell's OWN state (both
    read the depths and the albedo), found by iterating state -> oracle -> state until E_in moves by no more
    than 1e-13 S (`residual`: the last round's largest move; the host test asserts it); `ref` is the oracle
    at the final state, and melt_margins() of it is what the host test asserts."""
    s, mp = get_sweep("A", satterlund), melt_points(satterlund)
    NP = len(mp.idx)
    ix = np.indices((NP,) + MELT_AXES).reshape(5, -1)
    pnt, ax = ix[0], tuple(ix[1:])
    src = mp.idx[pnt]
    pts = {k: np.ascontiguousarray(s.pts[k][src]) for k in FORCING + ("elev", "slope", "aspect", "n", "albedo", "ring")}
    pts["P"] = np.where(mp.kind[pnt] == DRY, 0.0, MELT_P)
    cfg = dict(s.cfg, dt=dt)
    case = SimpleNamespace(name=f"melt-dt{dt:g}", cfg=cfg, sat=bool(satterlund), pts=pts, n=len(pnt), point=pnt, ax=ax,
                           jd=s.jd, th=s.th, night=s.night, step_cell=mp.step[pnt], jd_cell=s.jd[mp.step[pnt]],
                           th_cell=s.th[mp.step[pnt]], kind=mp.kind[pnt], floor=mp.floor[pnt] * dt, n_points=NP)
    case.snowing = (pts["P"] > 0) & (pts["T_air"] <= _cfgc(cfg)["T_rain_snow"])
    case.S = lambda ref: np.maximum(np.maximum(np.abs(ref["E_in"]), np.abs(ref["cold"])), case.floor)
    # first guess: the oracle's E_in over 1 m of snow on ice (the sweep's own depths reach the mast's top)
    z = np.zeros(case.n)
    _, ref = melt_oracle(case, dict(h_swe=z + 0.3, h_iwe=z + 2.0, Eccs=z, Ecci=z))
    E, cold = ref["E_in"], ref["cold"]
    for _ in range(24):  # the windy points' E_in reads the snow depth through the roughness: a dozen rounds
        st = _melt_states(case, E, cold)
        _, ref = melt_oracle(case, st)
        case.residual = float(np.max(np.abs(ref["E_in"] - E) / case.S(ref)))  # of the last round, over S
        E, cold = ref["E_in"], ref["cold"]
        if case.residual <= 1e-13:
            break
    # A capped reservoir leaves h - fl(h / 3600) dt 3600: at dt = 1 zero or a last-place residual, decided by
    # h's last bits, and not alike by h / 3600 and h (1/3600.) (the melt-out sweep measures how often).  Such
    # cells are the sweep's business: a depth whose residual the two arithmetics decide differently is moved
    # to the next fp64 number until they agree (both are functions of the depth alone there).
    case.moved = 0
    for _ in range(16):
        t = [melt_tail(cfg, ref["E_in"], ref["cold"], ref["P_snow"], ref["P_rain"], dict(st, h_ice=st["h_iwe"]), v)
             for v in ("reference", "fast")]
        bad = [(t[0][k] == 0) != (t[1][k] == 0) for k in ("h_swe", "h_iwe")]
        if not (bad[0].any() or bad[1].any()):
            break
        case.moved += int(bad[0].sum() + bad[1].sum())
        for k, b in zip(("h_swe", "h_iwe"), bad):
            st[k] = np.where(b, np.nextafter(st[k], np.inf), st[k])
        _, ref = melt_oracle(case, st)
    return _melt_finish(case, st, ref)


def _melt_finish(case, st, ref):
    c = _cfgc(case.cfg)
    ws, wi = np.float64(c["rho_H2O"]) / np.float64(c["rho_snow"]), np.float64(c["rho_H2O"]) / np.float64(c["rho_ice"])
    case.pts.update(h_swe=st["h_swe"], h_iwe=st["h_iwe"], h_snow=st["h_swe"] * ws, h_ice=st["h_iwe"] * wi)
    case.st = dict(st, h_ice=case.pts["h_ice"])
    case.ref = ref
    for a in list(case.pts.values()) + list(case.st.values()) + list(ref.values()):
        a.setflags(write=False)
    return case


@lru_cache(maxsize=None)
def meltout_case(satterlund: bool, dt: float, ice: bool):
    """The melt-out residual sweep of one dt: SWEEP_N seeded depths, log-uniform in SWEEP_RANGE, at the
    strongly melting dry point (the day point of 3 m/s in warm air), no cold content.  ice = False: h_swe0
    swept over h_iwe0 = 2 m; ice = True: h_iwe0 swept on bare ice.  ref, ref2: the oracle's first and second
    step (the second shows the ice gate: IM > 0 exactly where the snow of the first left exactly zero)."""
    s, mp = get_sweep("A", satterlund), melt_points(satterlund)
    j = MELT_WANTS.index((3.0, False, 1, True, DRY))
    src = np.full(SWEEP_N, mp.idx[j])
    pts = {k: np.ascontiguousarray(s.pts[k][src]) for k in FORCING + ("elev", "slope", "aspect", "n", "albedo", "ring")}
    pts["P"] = np.zeros(SWEEP_N)
    rng = np.random.default_rng(SAMPLE_SEED + (1 if ice else 0))
    h = np.exp(rng.uniform(np.log(SWEEP_RANGE[0]), np.log(SWEEP_RANGE[1]), SWEEP_N))
    step = np.full(SWEEP_N, mp.step[j])
    case = SimpleNamespace(name=f"meltout-{'ice' if ice else 'snow'}-dt{dt:g}", cfg=dict(s.cfg, dt=dt), sat=bool(satterlund),
                           pts=pts, n=SWEEP_N, point=np.zeros(SWEEP_N, np.int64), jd=s.jd, th=s.th, night=s.night,
                           step_cell=step, jd_cell=s.jd[step], th_cell=s.th[step], kind=np.full(SWEEP_N, DRY),
                           floor=np.full(SWEEP_N, mp.floor[j] * dt), n_points=1)
    case.snowing = np.zeros(SWEEP_N, bool)
    case.S = lambda ref: np.maximum(np.abs(ref["E_in"]), case.floor)
    z = np.zeros(SWEEP_N)
    st = dict(h_swe=z if ice else h, h_iwe=h if ice else np.full(SWEEP_N, 2.0), Eccs=z.copy(), Ecci=z.copy())
    m, ref = melt_oracle(case, st)
    case.ref2 = _oracle_step(case, m)
    return _melt_finish(case, st, ref)


def meltout_steps(case, variant: str):
    """Both steps of a melt-out case through melt_tail, each fed the oracle's E_in of that step."""
    outs, st = [], case.st
    for r in (case.ref, case.ref2):
        t = melt_tail(case.cfg, r["E_in"], r["cold"], r["P_snow"], r["P_rain"], st, variant)
        st = {k: t[k] for k in ("h_swe", "h_iwe", "Eccs", "Ecci", "h_ice")}
        outs.append(t)
    return outs


@lru_cache(maxsize=None)
def meltout_share(satterlund: bool, dt: float, ice: bool):
    """Of the swept depths: the share left at exactly zero by the first step in each arithmetic, and the
    share where the two disagree on it (a property of the two arithmetics, not of a kernel)."""
    case, k = meltout_case(satterlund, dt, ice), "h_iwe" if ice else "h_swe"
    a, b = meltout_steps(case, "reference")[0][k], meltout_steps(case, "fast")[0][k]
    return {"zero_reference": float(np.mean(a == 0)), "zero_fast": float(np.mean(b == 0)),
            "disagree": float(np.mean((a == 0) != (b == 0)))}


def melt_classes(case):
    """Per cell, the wave-uniform branches of the tail it takes: snowing | snow melts | ice melts | capped."""
    r = case.ref
    t = melt_tail(case.cfg, r["E_in"], r["cold"], r["P_snow"], r["P_rain"], case.st, "reference")
    return (case.snowing.astype(int) + 2 * (r["SM"] > 0).astype(int) + 4 * (r["IM"] > 0).astype(int)
            + 8 * t["gates"]["capped"].astype(int))


def probe_ecc(E):
    """The cold content K injected to read a cell's E_in back: the power of two with 4 |E| <= K < 8 |E|
    (2^-20 where E is zero or not finite), so that nothing melts and K - E_in lies in (K / 2, 2 K).
    Exactness for the fp32-flux forms: there E_in is an fp32 number, a multiple of 2^-24 |E_in| >= 2^-27 K
    (|E_in| > K / 8), and fp64 numbers below 2 K are spaced 2^-52 K or finer, so K - E_in is
    representable: the subtraction does not round."""
    a = np.abs(np.asarray(E, np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(np.isfinite(a) & (a > 0), 2.0 ** np.ceil(np.log2(np.where(a > 0, 4 * a, 1.0))), 2.0 ** -20)


def melt_probe_case(case):
    """The case as the probe run steps it: the same cells, but every cell with snow and no ice stands on 2 m
    of ice, so that its E_in reads from Ecci and, under snowfall, its cold content from Eccs beside it.
    Under snow the step's energy terms read neither h_ice nor h_iwe (the surface clamp and the albedo ask
    h_snow > 0 first), so such a cell forms the E_in and cold of the cell it stands for from the same
    numbers.  readable: [cells] False for the cells with neither snow nor ice, whose cold contents the step
    resets (under snowfall only E_in - cold survives, in Eccs): nothing can be read there."""
    c = _cfgc(case.cfg)
    wi = np.float64(c["rho_H2O"]) / np.float64(c["rho_ice"])
    on_ice = (case.pts["h_ice"] == 0) & (case.pts["h_snow"] > 0)
    sub = SimpleNamespace(**vars(case))
    sub.pts = dict(case.pts, h_iwe=np.where(on_ice, 2.0, case.pts["h_iwe"]), h_ice=np.where(on_ice, 2.0 * wi, case.pts["h_ice"]))
    sub.readable = sub.pts["h_ice"] > 0
    return sub
