"""The one-step energy probe (tests/step_probe.py) on the oracle alone: the method returns the oracle's
own terms, and every sweep meets the conditions the GPU test (test_gpu_step_terms.py) relies on; the sample
the one-cell kernels step (one_cell_sample, test_gpu_one_cell_terms.py) is deterministic and holds every
set it is meant to.  CPU only."""

from __future__ import annotations

import numpy as np
import pytest

from tests import step_probe as SP
from tests.harness import parity
import tfg_oracle as O

CASES = [(name, sat) for name in SP.SWEEPS for sat in (False, True)]
IDS = [f"{n}{'-sat' if s else ''}" for n, s in CASES]


@pytest.mark.parametrize("name,sat", CASES, ids=IDS)
def test_the_probe_returns_the_oracles_own_energy_and_cold_content(name, sat):
    """E_in read from the cold contents equals the oracle's Q_sum dt, and the cold content read from
    them equals the reference's formula (:1507-1537) evaluated on the oracle's RH, to 1e-9 (floored
    relative error of the project, the floor per sweep) at every point of the probe's linear range.  An
    unclamped cell reads E_in - cold (its only cold content is the one its P_TINY of snowfall keeps)."""
    s, ref = SP.get_sweep(name, sat), SP.reference(name, sat)
    lin = SP.linear(s, ref)
    assert lin.any()
    cf = np.broadcast_to(SP.cold_formula(s, ref["RH"][0], sat), ref["cold"].shape)
    truth = ref["Q_sum"] * s.cfg["dt"] - np.where(~s.from_ecci[None, :], cf, 0.0)
    err, _ = parity(ref["E_in"][lin], truth[lin], rtol=1e-9)
    assert err <= 1e-9, err
    ck = lin & s.cold_ok[None, :]
    if name.startswith("B"):
        assert ck.any()
    if ck.any():
        err, _ = parity(ref["cold"][ck], cf[ck], rtol=1e-9)
        assert err <= 1e-9, err
        rain = ck & ~s.snowing[None, :]
        assert np.all(ref["cold"][rain] == 0.0)  # rain brings no cold content: exactly zero


@pytest.mark.parametrize("name,sat", CASES, ids=IDS)
def test_the_probe_stays_linear_and_the_floor_is_attainable(name, sat):
    """Linear: at every point with a finite oracle E_in, E_in < ECC0 (with the snowfall's cold content,
    ECC0 + cold - E_in > 0) and snow or ice is left, so neither max(., 0) nor the zero-depth reset fires;
    the points with a non-finite E_in are exactly those of a zero or negative humidity (sweep B).
    Attainable: moving one fp32 input by one ulp changes the oracle's probe by more than half of 1e-5
    max(|ref|, s_v) at no more than CUT_CAP of any stratum (step_probe.parity_cut)."""
    s, ref = SP.get_sweep(name, sat), SP.reference(name, sat)
    lin, fin = SP.linear(s, ref), np.isfinite(ref["E_in"])
    assert np.array_equal(lin, fin)
    assert np.array_equal(~fin, np.broadcast_to(s.pts["Hum_sp"] <= 0, fin.shape))
    assert np.nanmax(np.abs(ref["E_in"])) < SP.ECC0 / 1.5
    for label, steps, pts in SP.strata(s):
        assert np.isfinite(SP.stratum_block(ref["E_in"], steps, pts)).mean() > 0.85, label
    cut_e, cut_c, share = SP.parity_cut(name, sat, 1e-5)
    assert share <= SP.CUT_CAP, share


@pytest.mark.parametrize("lat", [0.0, 46.8, 70.0])
@pytest.mark.parametrize("part", ["C", "Cb"])
def test_sweep_c_dark_decisions_are_decidable(part, lat):
    """No step of either part of sweep C is within 1e-9 h of any cell's sunrise or sunset as the oracle
    computes them, and the oracle's own dark mask is the one those times give.  Where the oracle's sun
    is up its net short wave is at least 1e-3 W m-2: |Q_sum| < 1000 W m-2 there, whose fp32 spacing is
    6.1e-5, so the term cannot vanish in the fp32 sum.  Step 0 is dark for every cell."""
    name = f"{part}-lat{lat:g}"
    s, ref = SP.get_sweep(name), SP.reference(name, False)
    m = O.OracleGrid(s.cfg, elev=s.pts["elev"], slope=s.pts["slope"], aspect=s.pts["aspect"], h0_snow=0.0, h0_ice=0.0,
                     h0_swe=0.0, h0_iwe=0.0)
    gap = np.inf
    for jd in np.unique(s.jd):
        ks = np.nonzero(s.jd == jd)[0]
        sr = O.sunrise_offset_slope(lat, jd, m.alpha, m.beta)[None, :]
        ss = O.sunset_offset_slope(lat, jd, m.alpha, m.beta)[None, :]
        th = s.th[ks][:, None]
        gap = min(gap, np.abs(th - sr).min(), np.abs(th - ss).min())
        assert np.array_equal((th <= sr) | (th >= ss), ref["Qn_SW"][ks] == 0), jd
    assert gap >= SP.C_MIN_GAP, gap
    up = ref["Qn_SW"] != 0
    assert up.any() and (~up).any() and ref["Qn_SW"][up].min() >= 1e-3
    assert np.abs(ref["Q_sum"]).max() < 1000.0
    assert np.all(ref["Qn_SW"][0] == 0)  # the dark reference step


@pytest.mark.parametrize("lat", [0.0, 46.8, 70.0])
def test_sweep_c_brackets_every_cells_own_sunrise_and_sunset(lat):
    """For every (slope, aspect, day) the bracket part has a step within C_NEAR before and one within
    C_NEAR after the cell's own sunrise, and the same for its sunset; where the slope itself sets the
    time (not the flat horizon), also within 2e-7 h on each side, inside the fp32 dark test's margin.
    Every slope, every aspect (the four cardinal ones included) and every day takes part."""
    s = SP.get_sweep(f"Cb-lat{lat:g}")
    m = O.OracleGrid(s.cfg, elev=s.pts["elev"], slope=s.pts["slope"], aspect=s.pts["aspect"], h0_snow=0.0, h0_ice=0.0,
                     h0_swe=0.0, h0_iwe=0.0)
    assert {(a, b) for a, b in zip(s.pts["slope"], s.pts["aspect"])} == \
        {(float(np.float32(a)), float(b)) for a in SP.C_SLOPES for b in SP.C_ASPECTS}
    assert {0.0, 90.0, 180.0, 270.0} <= set(SP.C_ASPECTS)
    slope_set = 0
    for day in SP.C_DAYS:
        jn = SP.bracket_jd(day)
        th = s.th[s.jd == jn][:, None]
        assert th.size
        delta = O.declination(O.day_angle(jn))
        for t, flat in ((O.sunrise_offset_slope(lat, jn, m.alpha, m.beta), O.sunrise_offset(lat, delta)),
                        (O.sunset_offset_slope(lat, jn, m.alpha, m.beta), O.sunset_offset(lat, delta))):
            d = th - t[None, :]
            assert np.all(np.any((d > 0) & (d <= SP.C_NEAR), axis=0)), (day, "no step just after")
            assert np.all(np.any((d < 0) & (d >= -SP.C_NEAR), axis=0)), (day, "no step just before")
            own = np.abs(t - flat) > 0.02
            slope_set += int(own.sum())
            assert np.all(np.any((d > 0) & (d <= 2e-7), axis=0)[own]) and np.all(np.any((d < 0) & (d >= -2e-7), axis=0)[own])
    assert slope_set > 100


def test_the_sweeps_reach_the_edges_they_are_built_for():
    a, ra = SP.get_sweep("A"), SP.reference("A", False)
    c = dict(O.CFG_DEFAULTS, **a.cfg)
    y = c["M_mass_air"] * c["g"] * a.pts["elev"] / (c["uni_gas_const"] * (a.pts["T_air"] + 273.15))
    s0 = np.abs(y + 0.345)
    assert (s0 <= 0.41).sum() > 1000 and (s0 > 0.41).sum() > 1000          # both sides of the flux form's exp_near
    assert np.any((s0 > 0.41) & (a.pts["elev"] == 600.0)) and np.any((s0 <= 0.41) & (a.pts["elev"] == 600.0))
    assert set(np.unique(a.pts["uz"])) == {float(np.float32(u)) for u in SP.A_UZ}
    arg = (10.0 - a.pts["h_snow"]) / c["z0_air"]
    assert np.any(arg < 0.01) and np.any(arg < 0) and np.any(arg > 100)    # the l2min clamp, from both sides
    clamped = (a.pts["h_snow"] > 0) | (a.pts["h_ice"] > 0)
    assert clamped.any() and (~clamped).any()
    # T_air == T_surf exactly: on snow or ice at 0 degC with a dew point above it; Ri of both signs
    eq = (a.pts["T_air"] == 0) & clamped & (a.pts["Hum_sp"] > SP.hum_sp_for(1.0, 0.0, a.pts["P_air"]))
    assert eq.sum() > 100
    assert a.n <= 2 ** 17 and a.pts["T_air"].min() == -45 and a.pts["T_air"].max() == 45
    for T_rs in (0.0, 50.2):
        for sat in (False, True):
            b, rb = SP.get_sweep(f"B-Trs{T_rs:g}", sat), SP.reference(f"B-Trs{T_rs:g}", sat)
            T, RH = b.pts["T_air"], rb["RH"][0]
            thr = np.float32(T_rs)
            for t, snow in ((np.nextafter(thr, np.float32(-np.inf)), True), (thr, float(thr) <= T_rs),
                            (np.nextafter(thr, np.float32(np.inf)), False)):
                sel = T == float(t)
                assert sel.any() and np.all(b.snowing[sel] == snow), (T_rs, t)
            assert np.all(b.pts["P"] > 0) and b.pts["P"].max() == float(np.float32(1e-5))
            with np.errstate(invalid="ignore"):
                den = 1.0 + (T + RH) * (RH - 1.676331)
                assert np.any((den > 0) & (den < 1.2e-3)) and np.any((den < 0) & (den > -1.2e-3)), (T_rs, sat)
                assert np.any((den < 0) & (T + RH < 0) & b.snowing)
                if T_rs > 1:
                    assert np.any((den < 0) & (T + RH > 0) & b.snowing)
                assert np.any(RH < 0) and np.any(RH > 5) and np.any(RH > 11) and np.any((RH > 0) & (RH < 5))
    assert float(np.float32(50.2)) > 50.2  # so the engine's threshold is the float below: the rounded-down case


# ------------------------------------------------------------------------------------------- the one-cell sample
def test_one_cell_sample_is_deterministic():
    for name, sat in CASES:
        a = SP.one_cell_sample(name, sat).copy()
        SP.one_cell_sample.cache_clear()
        b = SP.one_cell_sample(name, sat)
        assert a.shape[1] == 2 and np.array_equal(a, b), name
        assert len(np.unique(a, axis=0)) == len(a) and np.array_equal(a, a[np.lexsort((a[:, 1], a[:, 0]))])
        s = SP.get_sweep(name, sat)
        assert a[:, 0].min() >= 0 and a[:, 0].max() < s.n and a[:, 1].min() >= 0 and a[:, 1].max() < len(s.th)


def _pairs(name, sat):
    return {(int(p), int(k)) for p, k in SP.one_cell_sample(name, sat)}


@pytest.mark.parametrize("sat", [False, True])
def test_one_cell_sample_of_sweep_a_holds_every_combination(sat):
    """Both steps of at least one point of every combination, present in the sweep, of classes() value x
    surface x wind x (T_air > 0), and of every point with T_air == 0 at uz = 3."""
    s, ref, have = SP.get_sweep("A", sat), SP.reference("A", sat), _pairs("A", sat)
    both = np.array([(p, 0) in have and (p, 1) in have for p in range(s.n)])
    surf = np.full(s.n, -1)
    for j, (hs, hi) in enumerate(SP.A_SURF):
        surf[(s.pts["h_snow"] == SP.f32(hs)) & (s.pts["h_ice"] == SP.f32(hi))] = j
    wind = np.full(s.n, -1)
    for j, u in enumerate(SP.A_UZ):
        wind[s.pts["uz"] == SP.f32(u)] = j
    assert surf.min() == 0 and wind.min() == 0
    assert set(surf) == set(range(7)) and set(wind) == set(range(6))
    key = np.stack([SP.classes(s, ref), surf, wind, (s.pts["T_air"] > 0).astype(int)])
    combos = {tuple(c) for c in key.T}
    assert {tuple(c) for c in key[:, both].T} == combos and len(combos) > 7 * 6 * 2
    assert np.all(both[(s.pts["T_air"] == 0) & (s.pts["uz"] == 3.0)]) and np.any((s.pts["T_air"] == 0) & (s.pts["uz"] == 3.0))


@pytest.mark.parametrize("sat", [False, True])
@pytest.mark.parametrize("name,n,n_nan", [("B-Trs0", 816, 88), ("B-Trs50.2", 1488, 152)])
def test_one_cell_sample_of_sweep_b_is_the_whole_sweep(name, n, n_nan, sat):
    s, ref = SP.get_sweep(name, sat), SP.reference(name, sat)
    assert s.n == n and len(s.th) == 1 and _pairs(name, sat) == {(p, 0) for p in range(n)}
    assert int(np.isnan(ref["E_in"]).sum()) == n_nan


@pytest.mark.parametrize("lat", [0.0, 46.8, 70.0])
def test_one_cell_sample_of_sweep_c_holds_the_two_solstice_days(lat):
    """The dark step plus the 48 hourly steps of days 171 and 354, for all eleven albedo states, at slope 0.5
    and aspects 0, 90, 180 and 270."""
    name = f"C-lat{lat:g}"
    s, have = SP.get_sweep(name), _pairs(name, False)
    assert _pairs(name, True) == have
    steps = [0] + [k for k in range(1, len(s.th)) if np.floor(s.jd[k]) in (171.0, 354.0)]
    assert len(steps) == 49 and s.night[0] and not s.night[steps[1:]].any()
    assert {(s.jd[k], s.th[k]) for k in steps[1:]} == {(d + h / 24.0, h - 12.0 + 0.37) for d in (171.0, 354.0) for h in range(24)}
    state = np.array(list(zip(s.pts["n"], s.pts["T_air"], s.pts["h_snow"], s.pts["ring"], s.pts["P"])))
    for aspect in (0.0, 90.0, 180.0, 270.0):
        for alb in SP.C_ALB:
            want = np.array([alb[0], SP.f32(alb[1]), SP.f32(alb[2]), alb[3], SP.f32(alb[4])])  # n and the window stay fp64
            p = np.nonzero((s.pts["slope"] == 0.5) & (s.pts["aspect"] == aspect) & np.all(state == want, axis=1))[0]
            assert len(p) == 1, (aspect, alb)
            assert all((int(p[0]), k) in have for k in steps), (aspect, alb)


@pytest.mark.parametrize("lat", [0.0, 46.8, 70.0])
def test_one_cell_sample_of_sweep_cb_brackets_each_cells_own_times(lat):
    """All 96 (slope, aspect) cells at albedo state 5, each with the dark step and every step within C_NEAR
    of its own sunrise or sunset, and steps on both sides of both times on every day the oracle gives it
    one (a finite offset)."""
    name = f"Cb-lat{lat:g}"
    s, have = SP.get_sweep(name), _pairs(name, False)
    assert _pairs(name, True) == have
    m = O.OracleGrid(s.cfg, elev=s.pts["elev"], slope=s.pts["slope"], aspect=s.pts["aspect"], h0_snow=0.0, h0_ice=0.0,
                     h0_swe=0.0, h0_iwe=0.0)
    n5, T5, h5 = SP.C_ALB[5][:3]
    cells = np.nonzero((s.pts["n"] == n5) & (s.pts["T_air"] == T5) & (s.pts["h_snow"] == h5))[0]
    assert {(s.pts["slope"][p], s.pts["aspect"][p]) for p in cells} == \
        {(float(np.float32(a)), float(b)) for a in SP.C_SLOPES for b in SP.C_ASPECTS} and len(cells) == 96
    assert {p for p, _ in have} == set(cells)
    sides = 0
    for p in cells:
        ks = np.array(sorted(k for q, k in have if q == p))
        assert ks[0] == 0 and len(ks) < 60
        for day in SP.C_DAYS:
            jn = SP.bracket_jd(day)
            th = s.th[ks][s.jd[ks] == jn]
            for t in (O.sunrise_offset_slope(lat, jn, m.alpha[p:p + 1], m.beta[p:p + 1])[0],
                      O.sunset_offset_slope(lat, jn, m.alpha[p:p + 1], m.beta[p:p + 1])[0]):
                if not np.isfinite(t):
                    continue
                d = th - t
                assert np.any((d > 0) & (d <= SP.C_NEAR)) and np.any((d < 0) & (d >= -SP.C_NEAR)), (p, day, t)
                # every step of the sweep that near is in the sample
                near = np.nonzero((s.jd == jn) & (np.abs(s.th - t) <= SP.C_NEAR))[0]
                assert set(near) <= set(ks)
                sides += 1
    assert sides == 96 * 4 * 2


@pytest.mark.parametrize("name,sat", CASES, ids=IDS)
def test_one_cell_sample_keeps_linear_points_in_every_stratum(name, sat):
    """Every stratum of the sweep keeps at least one sampled pair in the probe's linear range for E_in, and,
    where the sweep has snowfall to read a cold content from, at least one for the cold content."""
    s, ref, ps = SP.get_sweep(name, sat), SP.reference(name, sat), SP.one_cell_sample(name, sat)
    lin = SP.linear(s, ref)
    P, K = ps[:, 0], ps[:, 1]
    for label, steps, pts in SP.strata(s):
        mine = steps[K] & pts[P] & lin[K, P]
        assert mine.any(), label
        if SP.stratum_block(lin & s.cold_ok[None, :], steps, pts).any():
            assert (mine & s.cold_ok[P]).any(), label
    if name.startswith("B"):
        assert s.cold_ok.any()


@pytest.mark.parametrize("name", list(SP.SWEEPS))
def test_layouts_hold_every_point_in_uniform_and_in_mixed_waves(name):
    s, ref = SP.get_sweep(name), SP.reference(name, False)
    cls = SP.classes(s, ref)
    srt, mix = SP.layouts(s, ref)
    for lay in (srt, mix):
        assert len(lay) % SP.WAVE == 0 and len(lay) <= 2 ** 17
        assert np.array_equal(np.unique(lay), np.arange(s.n))
        assert np.array_equal(lay[SP.first_lane(lay, s.n)], np.arange(s.n))
    w = cls[srt].reshape(-1, SP.WAVE)
    assert np.all(w == w[:, :1])                                         # sorted: every wave uniform
    w = cls[mix].reshape(-1, SP.WAVE)
    if len(np.unique(cls)) > 1:
        odd = sum(int(np.any(np.bincount(row) == 1)) for row in w)
        assert odd >= 4 and np.mean(np.any(w != w[:, :1], axis=1)) > 0.5  # interleaved: mixed, some with one odd lane
