"""The melt-state cases (tests/step_probe.py, "melt states") on the oracle alone: the restatement of the
step's tail reproduces OracleGrid.step bit for bit, every gate of the grid is decidable (melt_margins) and
taken on both sides, and the fp32 engine's documented arithmetic ("fast") decides every cell as the
reference's does and stays within a bound counted from its differing roundings.  The melt-out residual
sweep is where the two arithmetics do part: its share is measured here (and recorded by the GPU test), not
capped.  CPU only."""

from __future__ import annotations

import numpy as np
import pytest

from tests import step_probe as SP

CASES = [(sat, dt) for sat in (False, True) for dt in SP.MELT_DTS]
IDS = [f"{'sat' if s else 'bru'}-dt{d:g}" for s, d in CASES]
SWEEPS = [(dt, ice) for dt in SP.MELT_DTS for ice in (False, True)]
U = 2.0 ** -53    # half an ulp, relative: one fp64 rounding
F = 2.0 ** -24    # one fp32 rounding


def _bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.view(np.int64) == b.view(np.int64)


def _tail(case, variant, ref=None, st=None):
    r = case.ref if ref is None else ref
    return SP.melt_tail(case.cfg, r["E_in"], r["cold"], r["P_snow"], r["P_rain"], case.st if st is None else st, variant)


def test_the_forcing_points_are_seeded_and_at_their_strata_floors():
    for sat in (False, True):
        a = SP.melt_points(sat)
        SP.melt_points.cache_clear()
        b = SP.melt_points(sat)
        assert np.array_equal(a.idx, b.idx) and len(a.idx) == len(SP.MELT_WANTS) == 12
        assert np.all(np.abs(a.e_ref) >= a.floor) and np.all(a.floor > 0)
        s = SP.get_sweep("A", sat)
        T = s.pts["T_air"][a.idx]
        assert np.all(T[a.kind == SP.SNOW] <= 0) and np.all(T[a.kind == SP.RAIN] > 0)
        for sign in (1, -1):                      # positive and negative E_in, each dry and snowing; rain on positive
            for kind in (SP.DRY, SP.SNOW):
                assert np.any((np.sign(a.e_ref) == sign) & (a.kind == kind)), (sign, kind)
        assert np.any((a.e_ref > 0) & (a.kind == SP.RAIN))
        assert a.e_ref[a.e_ref > 0].max() > 4 * a.e_ref[a.e_ref > 0].min()   # strong and weak


@pytest.mark.parametrize("sat,dt", CASES, ids=IDS)
def test_the_reference_tail_is_the_oracles_bit_for_bit(sat, dt):
    """Fed the oracle's own E_in and snowfall cold content, the "reference" restatement returns every
    output of OracleGrid.step, and the cell's terms of the two integrals, with the same bits, on the whole
    grid; and on both steps of the melt-out sweeps."""
    case = SP.melt_case(sat, dt)
    assert case.n == 12 * int(np.prod(SP.MELT_AXES))
    t = _tail(case, "reference")
    for k in SP.MELT_TAIL_OUT:
        assert _bits(t[k], case.ref[k]).all(), (k, int((~_bits(t[k], case.ref[k])).sum()))
    for ice in (False, True):
        mo = SP.meltout_case(sat, dt, ice)
        t1 = _tail(mo, "reference")
        st1 = {k: t1[k] for k in ("h_swe", "h_iwe", "Eccs", "Ecci", "h_ice")}
        t2 = _tail(mo, "reference", mo.ref2, st1)
        for k in SP.MELT_TAIL_OUT:
            assert _bits(t1[k], mo.ref[k]).all() and _bits(t2[k], mo.ref2[k]).all(), (ice, k)


@pytest.mark.parametrize("sat,dt", CASES, ids=IDS)
def test_every_gate_is_decidable_and_taken_on_both_sides(sat, dt):
    """No gate quantity of the oracle is within MELT_MARGIN S of its threshold (S = max(|E|, |cold|, the
    stratum's floor): the scale of the parity tolerance, so the margin is 10 x what any fp32 form may be off),
    and the grid reaches what it is built for."""
    case = SP.melt_case(sat, dt)
    r, st = case.ref, case.st
    m = SP.melt_margins(case, r, st)
    for k, v in m.items():
        assert np.all(v >= SP.MELT_MARGIN), (k, float(v.min()), int(np.argmin(v)))
        assert np.isfinite(v).any(), k                                   # every gate is reached somewhere
        if not (k == "ice melt-out" and dt == 0.25):                     # (there the cap binds first: no ice runs dry)
            assert np.nanmin(np.where(np.isfinite(v), v, np.nan)) < 0.01  # ... and closely: the +- values
    # no depth near z - z0 = 9.99 m, where the roughness log passes through zero (sweep A leaves it out too)
    assert np.isfinite(r["E_in"]).all() and np.all(np.abs(case.pts["h_snow"] - 9.99) > 0.05)
    d = SP.melt_decisions(_tail(case, "reference"))
    for k, v in d.items():
        assert v.any() and (~v).any(), k
    # per kind of point: the gates that kind can reach are taken on both sides
    warm = r["E_in"] > 0
    for kind in (SP.DRY, SP.SNOW, SP.RAIN):
        sel = (case.kind == kind) & warm
        assert sel.any(), kind
        for k in ("SM==0", "IM==0", "capped", "h_swe==0", "h_iwe==0", "Eccs==0", "Ecci==0"):
            if kind == SP.SNOW and dt == 0.25 and k in ("IM==0", "h_swe==0", "h_iwe==0", "Eccs==0"):
                continue  # a quarter-hour step cannot melt all of its own snowfall: the ice below stays shut
            assert d[k][sel].any() and (~d[k][sel]).any(), (kind, k)
    cold = ~warm
    assert cold.any() and np.all(d["SM==0"][cold]) and np.all(d["IM==0"][cold])
    assert np.any(~d["Eccs==0"][cold]) and np.any(~d["Ecci==0"][cold])
    # snow falls on bare ice: previous_swe == 0 but h_swe > 0 after the step, so the ice does not melt
    on_ice = case.snowing & (st["h_swe"] == 0) & (st["h_iwe"] > 0) & (r["h_swe"] > 0) & (r["E_in"] > st["Ecci"])
    assert on_ice.any() and np.all(r["IM"][on_ice] == 0)
    # ... and where the step melts all of the snowfall, it does
    assert dt == 0.25 or np.any(case.snowing & (st["h_swe"] == 0) & (r["h_swe"] == 0) & (r["IM"] > 0))
    assert case.moved <= 0.002 * case.n   # depths moved off a last-place melt-out residual (melt_case)
    assert case.residual <= 1e-12         # the grid is placed from each cell's own E_in: the iteration settled
    # the reset of the cold contents: h_ice_prev == 0 with energy to spare and without; h_snow_new == 0
    assert np.any((st["h_iwe"] == 0) & (st["Ecci"] > r["E_in"])) and np.all(r["Ecci"][st["h_iwe"] == 0] == 0)
    assert np.any((r["h_swe"] == 0) & (st["Eccs"] > r["E_in"] + np.abs(r["cold"])))
    # the rate cap IM <= h_iwe / dt binds somewhere (the integral then holds less than IM's potential)
    t = _tail(case, "reference")["gates"]
    assert np.any((t["im_gated"] > st["h_iwe"] / dt) & (st["h_iwe"] > 0))
    ice = r["IM"] > 0
    if dt == 0.25:   # the dt 3600 quirk: a capped reservoir keeps three quarters, and nothing ever runs dry
        assert np.any(d["capped"] & (r["h_swe"] > 0)) and np.any(ice & (r["IM"] * 3600 == st["h_iwe"]) & (r["h_iwe"] > 0))
    if dt == 2.0:    # ... and at 2 h an uncapped melt of more than half of it takes it all
        assert np.any(~d["capped"] & (r["SM"] > 0) & (r["h_swe"] == 0) & (r["SM"] * 3600 < 0.999 * t["avail"]))
        assert np.any(ice & (r["IM"] * 3600 < 0.999 * st["h_iwe"]) & (r["h_iwe"] == 0))


@pytest.mark.parametrize("sat,dt", CASES, ids=IDS)
def test_the_fast_arithmetic_decides_as_the_reference_and_stays_within_its_roundings(sat, dt):
    """"fast" against "reference" from the oracle's E_in, whole grid.  Decisions: all equal.  Values, with u
    = 2^-53 per fp64 rounding and f = 2^-24 per fp32 rounding, counted from melt_tail's two branches (the
    dts are powers of two, so E_rem / dt, h_iwe / dt, dt 3600 and SM dt are exact in both):
      Eccs, Ecci     the same operations: the same bits.
      SM 3600        E_rem / rhoLf x 3600 (2 roundings) against E_rem x (3600 / (dt rhoLf)) (2): 4 u.
      h_swe          the subtrahend SM dt 3600 adds /3600 and x 3600 (2; 4 in all) against x (1/3600.), whose
                     constant is rounded too, and x dt3600 (3; 5 in all): 9 u of what melts; the subtraction
                     rounds once in each: 2 u of what was available.  Bound: u (10 melt + 2 available).
      h_iwe          IM = E_rem / rhoLf (1) against E_rem x (1 / (dt rhoLf)) (2), then x 3600, / 3600, x 3600 (3; 4 in
                     all) against x 3600, x (1/3600.), x dt3600 (4; 6 in all): 10 u of what melts, 2 u of h_iwe0.
      h_snow, h_ice  one product more in each: w x the depth's bound + 2 u of the depth.
      SM, IM         at most 3 (4) roundings against 4 (5), then the history's fp32: (f + 9 u) of the rate.
      M_total        three fp32 terms, the rain's with a rounded constant and a product, two fp32 additions
                     of non-negative terms: 5 f of M_total beside the terms' own differences (9 u).
      integrals      SM's: E_rem / rhoLf x da x dt x 3600 (3) against fp32(E_rem) x a constant of 3 roundings
                     (1 more): (f + 8 u); IM's: IM (<= 2) x da dt 3600 (2) against fp32(IM) (f, <= 3) x
                     constant (1) x (1): (f + 9 u)."""
    case = SP.melt_case(sat, dt)
    a, b = _tail(case, "reference"), _tail(case, "fast")
    da, db = SP.melt_decisions(a), SP.melt_decisions(b)
    for k in da:
        assert np.array_equal(da[k], db[k]), (k, int((da[k] != db[k]).sum()))
    c = SP._cfgc(case.cfg)
    ws, wi = c["rho_H2O"] / c["rho_snow"], c["rho_H2O"] / c["rho_ice"]
    g = a["gates"]
    melt_s = np.minimum(g["sm3600"], g["avail"]) * dt
    melt_i = np.minimum(g["im_gated"] * 3600, case.st["h_iwe"]) * dt
    b_swe, b_iwe = U * (10 * melt_s + 2 * g["avail"]), U * (10 * melt_i + 2 * case.st["h_iwe"])
    bound = {"Eccs": 0.0, "Ecci": 0.0, "h_swe": b_swe, "h_iwe": b_iwe,
             "h_snow": ws * b_swe + 2 * U * a["h_snow"], "h_ice": wi * b_iwe + 2 * U * a["h_ice"],
             "SM": (F + 9 * U) * a["SM"], "IM": (F + 9 * U) * a["IM"], "M_total": (5 * F + 9 * U) * a["M_total"],
             "vol_SM": (F + 8 * U) * a["vol_SM"], "vol_IM": (F + 9 * U) * a["vol_IM"]}
    for k in SP.MELT_TAIL_OUT:
        over = np.abs(b[k] - a[k]) > bound[k]
        assert not over.any(), (k, int(over.sum()), float(np.max(np.abs(b[k] - a[k])[over])))
    assert _bits(a["Eccs"], b["Eccs"]).all() and _bits(a["Ecci"], b["Ecci"]).all()


@pytest.mark.parametrize("sat,dt", CASES, ids=IDS)
def test_the_probe_case_forms_the_same_energy_and_reads_every_cell_with_snow_or_ice(sat, dt):
    """The probe run's depths (melt_probe_case: 2 m of ice under every cell with snow and none) give the
    oracle the same E_in and snowfall cold content, bit for bit, as the cell they stand for; K - Ecci and
    (Eccs - K) + E_in after a step from K in both cold contents return them to K's last place; the cells
    that cannot be read are exactly those with neither snow nor ice."""
    case = SP.melt_case(sat, dt)
    pc = SP.melt_probe_case(case)
    bare = (case.pts["h_snow"] == 0) & (case.pts["h_ice"] == 0)
    assert np.array_equal(~pc.readable, bare) and 0 < bare.sum() < 0.25 * case.n
    K = SP.probe_ecc(case.ref["E_in"])
    assert np.all(K >= 4 * np.abs(case.ref["E_in"])) and np.all(K < 8 * np.abs(case.ref["E_in"]))
    _, r = SP.melt_oracle(pc, dict(h_swe=pc.pts["h_swe"], h_iwe=pc.pts["h_iwe"], Eccs=K, Ecci=K))
    ok = pc.readable
    assert _bits(r["E_in"], case.ref["E_in"])[ok].all() and _bits(r["cold"], case.ref["cold"])[ok].all()
    assert np.all(r["SM"] == 0) and np.all(r["IM"] == 0)       # nothing melts
    E = K - r["Ecci"]
    cold = np.where(case.snowing, (r["Eccs"] - K) + E, 0.0)
    assert np.all(np.abs(E - case.ref["E_in"])[ok] <= 2.0 ** -53 * K[ok])
    assert np.all(np.abs(cold - case.ref["cold"])[ok] <= 3 * 2.0 ** -53 * K[ok])


@pytest.mark.parametrize("dt,ice", SWEEPS, ids=[f"{'ice' if i else 'snow'}-dt{d:g}" for d, i in SWEEPS])
def test_the_melt_out_sweep_is_capped_everywhere_and_its_share_is_measured(dt, ice):
    """The sweep's point melts at least twice every swept depth in a step, so the first step is capped and
    the depth it leaves is a function of the depth alone.  Measured, not bounded: the share of depths whose
    residual is exactly zero in one arithmetic and not in the other."""
    for sat in (False,):
        mo = SP.meltout_case(sat, dt, ice)
        h = mo.st["h_iwe" if ice else "h_swe"]
        assert mo.n == SP.SWEEP_N and h.min() >= SP.SWEEP_RANGE[0] and h.max() <= SP.SWEEP_RANGE[1]
        pot = np.maximum(mo.ref["E_in"], 0.0) * SP.melt_c(mo.cfg)
        assert np.all(pot >= 2 * h), float((pot / h).min())
        assert np.all(mo.ref2["E_in"] * SP.melt_c(mo.cfg) >= 2e-3)
        sh = SP.meltout_share(sat, dt, ice)
        print(f"{mo.name}: residual == 0 in {sh['zero_reference']:.4f} (reference) and "
              f"{sh['zero_fast']:.4f} (fast) of {mo.n}; they disagree in {sh['disagree']:.2e}")
        assert 0.0 <= sh["disagree"] <= 1.0
        if dt == 0.25:   # three quarters stay: never zero in either
            assert sh["zero_reference"] == sh["zero_fast"] == sh["disagree"] == 0.0
        if dt == 2.0:    # all of it goes, in both
            assert sh["zero_reference"] == sh["zero_fast"] == 1.0
