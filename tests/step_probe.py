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
    cls = classes(s, ref)
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


def gpu_probe(s, engine: str, satterlund: bool, nan_safe, layout):
    """One engine step per sweep step on the grid `layout` (1 x len(layout)), state re-injected before
    each; returns, per name in READ + OUTS, [steps][len(layout)] as read back, and E_in, cold by recover().
    The step writes window slot 0 each time and slot 1 holds the snowfall already in the window, so the
    window's total is the same at every step."""
    lay = np.asarray(layout)
    n = len(lay)
    p = {k: np.ascontiguousarray(v[lay]) for k, v in s.pts.items()}
    sl = SimpleNamespace(from_ecci=s.from_ecci[lay], cold_ok=s.cold_ok[lay])
    cfg = dict(s.cfg, SATTERLUND=satterlund)
    clock = probe_clock(s)
    e = make_engine(cfg, 1, n, engine, n_frames=1, hist_depth=1, fuse_steps=1)
    out = {k: np.empty((len(s.th), n)) for k in READ + OUTS + ("E_in", "cold")}
    try:
        for k in ("elev", "slope", "aspect", "h_snow", "h_ice", "h_swe", "h_iwe"):
            e.set_field(k, p[k])
        e.init_state()
        if nan_safe is not None:
            e.set_step_form(bool(nan_safe))
        e.set_inputs(np.stack([p[v] for v in ("P_air", "Hum_sp", "P", "T_air", "uz")]), 0)
        e.set_field("window", p["ring"], index=1)
        ecc = np.full(n, ECC0)
        for k in range(len(s.th)):
            for name in STATE:
                e.set_field(name, ecc if name in ("Eccs", "Ecci") else p[name])
            u = clock.uniforms(k, 1)
            u["frame"], u["hist"], u["slot"] = 0, 0, 0
            e.run(1, uniforms=u)
            e.sync()
            for name in READ + OUTS:
                out[name][k] = e.get_field(name)
            out["E_in"][k], out["cold"][k] = recover(sl, out["Eccs"][k], out["Ecci"][k])
    finally:
        e.close()
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


def inject_point(e, s, i: int, statics: bool = True) -> None:
    """Point i of the sweep into a one-cell handle: its statics (unless the handle holds them), the injected
    state (ECC0 in both cold contents) and window slot 1."""
    one = lambda a: np.ascontiguousarray(a[i:i + 1], dtype=np.float64)  # noqa: E731
    if statics:
        for k in ("elev", "slope", "aspect"):
            e.set_field(k, one(s.pts[k]))
    ecc = np.full(1, ECC0)
    for name in STATE:
        e.set_field(name, ecc if name in ("Eccs", "Ecci") else one(s.pts[name]))
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


def gpu_probe_one_cell(s, kernel: str, satterlund: bool, point_steps, handles: list | None = None):
    """The (point, step) pairs `point_steps` [N][2], each one launch of a one-cell kernel from the injected
    state (the read_depths = 1 entry: the depths are set before every step): per name in READ + OUTS + E_in +
    cold, [N] as gpu_probe returns them per (step, lane); READ from the handle's state, OUTS from the
    call's output block.  "k_cell": one handle, reused over the points; "k_cell_many": up to MANY_POOL
    handles on the BMI's shared stream, each holding a run of consecutive pairs, all stepped once per
    launch.  `handles` (a list) receives, per handle, (diagnostics [1][6], the P it was fed, in order, and
    T_air)."""
    assert kernel in ONE_CELL_KERNELS, kernel
    ps = np.asarray(point_steps, np.int64).reshape(-1, 2)
    N = len(ps)
    cfg = dict(s.cfg, SATTERLUND=satterlund)
    clock = probe_clock(s)
    urec = {int(k): probe_uniform(clock, int(k)) for k in np.unique(ps[:, 1])}
    res = {k: np.empty(N) for k in READ + OUTS}
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
                inject_point(engines[j], s, i, statics=holds[j] != i)
                holds[j] = i
                vals.append(point_inputs(s, i))
                fed[j].append((s.pts["P"][i], s.pts["T_air"][i]))
            us = [urec[int(ps[j * per + b, 1])] for j in js]
            if kernel == "k_cell":
                update_one(engines[0], vals[0], us[0], outs[0])
            else:
                update_batch([engines[j] for j in js], vals, us, [outs[j] for j in js])
            for j in js:
                q = j * per + b
                for name in READ:
                    res[name][q] = engines[j].get_field(name)[0]
                for name in OUTS:
                    res[name][q] = outs[j][OUT_ROW[name], 0]
        if handles is not None:
            handles += [(e.diagnostics(), np.array([f[0] for f in fd]), np.array([f[1] for f in fd]))
                        for e, fd in zip(engines, fed)]
    finally:
        for e in engines:
            e.close()
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
