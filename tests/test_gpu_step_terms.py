"""The shipped step kernels' energy terms over the whole forcing domain, one step at a time, read out of
the engine's own fp64 cold contents (tests/step_probe.py; the method and the conditions on the sweeps
are checked on the oracle alone in tests/test_step_probe_host.py).

Per engine form and sweep:

  parity    E_in = Q_sum dt and the snowfall's cold content against the oracle's, by the project's floored
            relative error (tests.harness.parity), 1e-5 for every fp32 form and 1e-10 for float64; the
            floor is taken per stratum (one uz value, day or night), so a windy stratum's large fluxes
            cannot hide a calm one's error.  Points outside the probe's linear range (the oracle's E_in
            not finite: a zero or negative humidity) and points the +-1 ulp cut rule removes
            (step_probe.parity_cut; none in the committed sweeps) are not compared.
  dark      sweep C, both parts: the short-wave term (a step's E_in minus the dark reference step's) is zero exactly
            where the oracle's is, at every point; no allowance.
  layout    a cell's result does not depend on its wave neighbours: Eccs, Ecci, h_swe, n, albedo and the
            six outputs are the same bits in a layout whose waves are uniform in {snowing, RH off the wet
            bulb's fits, the flux form's rare exp path, dark at the sweep's middle step} and in one that
            mixes them in every wave.
  nan       where the oracle's E_in is NaN (a zero or negative humidity), the fp64 engine's and the NaN-safe
            fp32 forms' is NaN too.

The measured maxima go to $TFG_REPORT_DIR/step_terms.json (profiles/step_terms.json is a GPU run's
copy); no assertion reads them.
"""

from __future__ import annotations

import json
import os

import numpy as np
import pytest

from tests import step_probe as SP
from tests.harness import parity, scale_floor

CASES = [(form, sweep) for sweep in SP.SWEEPS for form in SP.FORMS]
_REPORT: dict = {}


def _write_report():
    d = os.environ.get("TFG_REPORT_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "step_terms.json"), "w") as f:
            json.dump(_REPORT, f, indent=1, sort_keys=True)


def _same_bits(a, b):
    """Elementwise: equal as numbers (so +0 and -0 differ by their bits below), or both NaN."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))


def _max_abs(x):
    x = np.asarray(x)
    x = x[np.isfinite(x)]
    return float(np.abs(x).max()) if x.size else 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("form,sweep", CASES, ids=[f"{s}-{f[0]}" for f, s in CASES])
def test_one_step_energy_terms_against_the_oracle(form, sweep):
    fname, engine, sat, nan_safe = form
    tol = 1e-10 if engine == "float64" else 1e-5
    s, ref = SP.get_sweep(sweep, sat), SP.reference(sweep, sat)
    dt = s.cfg["dt"]
    srt, mix = SP.layouts(s, ref)
    g_srt = SP.gpu_probe(s, engine, sat, nan_safe, srt)
    g_mix = SP.gpu_probe(s, engine, sat, nan_safe, mix)
    first = SP.first_lane(srt, s.n)
    G = {k: v[:, first] for k, v in g_srt.items()}  # [steps][points]
    failures = []
    rep = _REPORT.setdefault(fname, {}).setdefault(sweep, {})

    # ---- layout: every lane of both layouts against the point's first lane in the sorted one
    for lay, g, what in ((srt, g_srt, "sorted"), (mix, g_mix, "interleaved")):
        for name in SP.READ + SP.OUTS:
            bad = ~_same_bits(G[name][:, lay], g[name])
            if bad.any():
                k, lane = np.argwhere(bad)[0]
                failures.append(f"layout: {name} of point {lay[lane]} differs in the {what} layout at lane {lane}, "
                                f"step {k} ({int(bad.sum())} entries): {G[name][k, lay[lane]]!r} vs {g[name][k, lane]!r}")
    rep["layout_entries_differing"] = int(sum((~_same_bits(G[n][:, mix], g_mix[n])).sum() for n in SP.READ + SP.OUTS))

    # ---- parity, per stratum
    lin = SP.linear(s, ref)
    if engine == "float64":
        cut_e = cut_c = np.zeros(lin.shape, bool)  # fp64 inputs: nothing is rounded
    else:
        cut_e, cut_c, share = SP.parity_cut(sweep, sat, tol)
        assert share <= SP.CUT_CAP
    rep["strata"] = {}
    for label, steps, pts in SP.strata(s):
        blk = lambda a: SP.stratum_block(a, steps, pts)  # noqa: E731
        out = rep["strata"].setdefault(label, {})
        for key, ok_pts, cut in (("E_in", np.ones(s.n, bool), cut_e), ("cold", s.cold_ok, cut_c)):
            ok = blk(lin & ok_pts[None, :])
            if not ok.any():
                continue
            g, r, keep = blk(G[key])[ok], blk(ref[key])[ok], ~blk(cut)[ok]
            with np.errstate(invalid="ignore"):
                err, _ = parity(np.where(np.isfinite(g), g, np.inf), r, rtol=tol, mask=keep)
            out[f"{key}_max_floored_error"] = err
            out[f"{key}_floor"] = scale_floor(r)
            out[f"{key}_points"], out[f"{key}_cut"] = int(ok.sum()), int((~keep).sum())
            print(f"{fname} {sweep} {label}: {key} floored error {err:.3e} (floor {scale_floor(r):.4g}, {int(ok.sum())} points)")
            if not err <= tol:
                d = np.abs(g - r) / np.maximum(np.abs(r), scale_floor(r))
                d = np.where(keep, d, 0.0)
                j = int(np.nanargmax(np.where(np.isfinite(d), d, np.inf)))
                kk, pp = (a[ok][j] for a in np.meshgrid(np.nonzero(steps)[0], np.nonzero(pts)[0], indexing="ij"))
                failures.append(f"parity: {key} in {label}: floored error {err:.3e} > {tol:g}; worst at step {kk}, point {pp}: "
                                f"engine {g[j]!r}, oracle {r[j]!r}, inputs "
                                + ", ".join(f"{n}={s.pts[n][pp]!r}" for n in SP.FORCING))
        rain = blk((lin & (s.cold_ok & ~s.snowing)[None, :]))
        if rain.any() and np.any(blk(G["cold"])[rain] != 0.0):
            failures.append(f"parity: {label}: rain brought a cold content")

    # ---- the separated terms [W m-2] and the wet bulb [K] per stratum, for the report
    err = np.where(lin, G["E_in"] - ref["E_in"], np.nan) / dt
    night = np.nonzero(s.night)[0]
    calm = np.nonzero(s.pts["uz"] == 0)[0]
    wb = lin & (s.cold_ok & s.snowing)[None, :]
    d_wb = np.where(wb, SP.wet_bulb_of(s, G["cold"]) - SP.wet_bulb_of(s, ref["cold"]), np.nan)
    for label, steps, pts in SP.strata(s):
        terms = rep["strata"][label].setdefault("max_abs_error", {})
        sel = np.nonzero(pts)[0]
        if steps[night[0]]:
            if sweep == "A" and s.pts["uz"][sel[0]] == 0:
                terms["Qn_LW_Wm2"] = _max_abs(err[night][:, sel])                # a calm night: long wave alone
            elif sweep == "A":                                                   # a windy night minus the calm one
                terms["Qh_plus_Qe_Wm2"] = _max_abs(err[night][:, sel[np.argsort(s.meta["gid"][sel])]]
                                                   - err[night][:, calm[np.argsort(s.meta["gid"][calm])]])
        else:
            terms["Qn_SW_Wm2"] = _max_abs(err[steps][:, sel] - err[night[:1]][:, sel])  # a day step minus the night step
        if wb[np.ix_(steps, pts)].any():
            terms["T_wb_K"] = _max_abs(d_wb[np.ix_(steps, pts)])
    with np.errstate(invalid="ignore"):
        lost = np.isfinite(G["E_in"]) & ~np.isfinite(ref["E_in"])
    rep["points_finite_where_the_oracle_is_not"] = int(lost.sum())
    # missing data: where the reference's E_in is NaN (the log of a zero or negative humidity) the fp64
    # engine and the fp32 step's NaN-safe form return NaN too; the plain form is not held to it
    if nan_safe is not False and lost.any():
        k, p = np.argwhere(lost)[0]
        failures.append(f"nan: {int(lost.sum())} points are finite where the oracle's E_in is not; first at step {k}, "
                        f"point {p} (Hum_sp {s.pts['Hum_sp'][p]!r}): engine {G['E_in'][k, p]!r}")

    # ---- the dark decision
    if sweep.startswith("C"):
        sw_engine = G["E_in"][1:] - G["E_in"][:1]
        wrong = (sw_engine == 0) != (ref["Qn_SW"][1:] == 0)
        rep["dark_decisions"], rep["dark_decisions_wrong"] = int(wrong.size), int(wrong.sum())
        if wrong.any():
            k, p = np.argwhere(wrong)[0]
            failures.append(f"dark: {int(wrong.sum())} of {wrong.size} decisions differ from the oracle's; first at step "
                            f"{k + 1} (jd {s.jd[k + 1]!r}, th {s.th[k + 1]!r}), point {p} (slope {s.pts['slope'][p]}, aspect "
                            f"{s.pts['aspect'][p]}): engine short wave {sw_engine[k, p] / dt!r}, oracle {ref['Qn_SW'][k + 1, p]!r}")
    _write_report()
    assert not failures, "\n".join(failures)
