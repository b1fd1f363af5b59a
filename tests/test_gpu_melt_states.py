"""The step's melt and state update (melt_core / melt_fast, the tail of cell_step_exact, the one-catchment
kernels' restatement) from injected state, one step at a time, against the oracle: tests/step_probe.py's
melt-state cases (their conditions are checked on the oracle alone in tests/test_melt_states_host.py).

Per engine form and dt in {1, 2, 0.25} h, on twelve forcing points x 900 states:

  layout     a cell gives the same bits whether its wave is uniform in {snowing, snow melts, ice melts,
             capped} or mixes them, at both clock steps.
  decisions  SM, IM, Eccs, Ecci, h_swe, h_iwe are zero exactly where the oracle's are, and SM 3600 is the snow
             that was available (capped; read as SM > 0 and |SM 3600 - available| < MELT_MARGIN S c / 2, which the grid's
             margin separates from every uncapped cell within tolerance) exactly where the oracle caps.  Every
             cell; no cut, no allowance.
  parity     in energy-equivalent units (a depth / c, a rate x 3600 / c, cold contents as they are) every
             output is within tol max(|E|, s_v) of the oracle's, tol = 1e-5 (fp32 forms) or 1e-10, s_v the floor
             of the point's stratum; an fp32 history output adds one fp32 rounding (2^-24 of it).
  isolation  the engine's own E_in and snowfall cold content are read back from a second run from the same
             depths with K = the power of two in [4 |E|, 8 |E|) in both cold contents (E_in from Ecci, cold from
             Eccs beside it; a cell with snow and no ice is stepped on 2 m of ice there, which under snow no
             energy term reads: step_probe.melt_probe_case) and fed to the tail's restatement ("fast" for the
             fp32 engine, "reference" for float64 and the one-cell kernels).
               fp32 flux: E_in and cold are fp32 numbers of at least K / 8 and K 2^-28, so K - E_in and K + cold -
               E_in are exact in fp64: the probe is exact and h_swe, h_iwe, Eccs, Ecci, SM, IM, h_snow, h_ice must
               be the restatement's bits.  M_total = (IM + SM) + P_rain (1/3600.f) in fp32, terms >= 0: three
               roundings as written, two where the compiler fuses the product into the sum (it does in some
               forms and not in others): the two evaluations are within 5 x 2^-24 of each other.
               fp64 flux and float64: each read-back rounds to K's last place, 2^-53 K: E_in is off by at most
               that, cold (two more roundings) by 3 x that, and the tail passes each on with slope <= 1; the
               tail's own <= 8 roundings per output act on operands of at most M = max(|E|, Eccs0, Ecci0, the
               depths / c).  Bound: 2^-52 (4 K + 16 M) [J m-2] (+ 2^-24 of an fp32 output, M_total's 5 x 2^-24).
             Cells with neither snow nor ice before the step cannot be read (both cold contents are reset);
             their number is reported.  They stay in every other assertion.
  integrals  the per-catchment SM and IM sums (one catchment per forcing point) match the sums of the
             oracle's per-cell terms (the unclamped SM; the IM after its first cap only) within the sum of the
             cells' tol max(|E|, s_v), in volume units.
  melt-out   the residual sweeps (4096 depths, snow and ice, two steps): float64 leaves the oracle's bits in
             h_swe and h_iwe after the first step, the fp32 forms the "fast" restatement's; the second step's IM
             is zero exactly where theirs is (its value, which reads the engine's own E_in, within tol); M_total
             = SM + IM + P_rain / 3600 to the outputs' rounding at every cell of grid and sweep.

The one-cell kernels step a seeded sample of 320 states (each handle's two integrals against the sums over
the states it stepped) and 128 depths of each sweep, two steps on the same handle: the oracle's bits in h_swe
and h_iwe after the first, the second step's IM zero exactly where the oracle's is and within tol in value
(it reads the kernel's own E_in, which is the oracle's to 1e-13, not to the bit), h_swe after it bit for bit.

Measured maxima and counts go to $TFG_REPORT_DIR/melt_states.json (profiles/melt_states.json is a GPU
run's copy); no assertion reads them.
"""

from __future__ import annotations

import json
import os

import numpy as np
import pytest

from tests import step_probe as SP

CASES = [(form, dt) for dt in SP.MELT_DTS for form in SP.FORMS]
ONE_CELL = [(k, sat, dt) for k in SP.ONE_CELL_KERNELS for sat, dt in ((False, 1.0), (False, 2.0), (False, 0.25), (True, 1.0))]
N_ONE, N_ONE_SWEEP = 320, 128
STATE = ("h_swe", "h_iwe", "Eccs", "Ecci")
RATES = ("SM", "IM", "M_total")
F32 = 2.0 ** -24
_REPORT: dict = {}


def _write_report():
    d = os.environ.get("TFG_REPORT_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        _REPORT["melt_out_share_fast_vs_reference"] = {
            f"{'ice' if ice else 'snow'}-dt{dt:g}": SP.meltout_share(False, dt, ice) for dt in SP.MELT_DTS for ice in (False, True)}
        with open(os.path.join(d, "melt_states.json"), "w") as f:
            json.dump(_REPORT, f, indent=1, sort_keys=True)


def _bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))


def _units(case):
    """Per output: the factor that takes it to energy-equivalent units [J m-2]."""
    c = SP._cfgc(case.cfg)
    k = SP.melt_c(case.cfg)
    ws, wi = c["rho_H2O"] / c["rho_snow"], c["rho_H2O"] / c["rho_ice"]
    return {"h_swe": 1 / k, "h_iwe": 1 / k, "h_snow": 1 / (k * ws), "h_ice": 1 / (k * wi), "SM": 3600 / k, "IM": 3600 / k,
            "M_total": 3600 / k, "Eccs": 1.0, "Ecci": 1.0}


def _check_cells(case, G, P, fp32, tol, one_cell, failures, rep):
    """Decisions, parity and isolation of the cells `G` holds ([cells] per name, in case order or the
    sample `P.cells` of it); P: the probe run's read-back, same cells."""
    sel = P["cells"]
    ref = {k: v[sel] for k, v in case.ref.items()}
    st = {k: v[sel] for k, v in case.st.items()}
    unit = _units(case)
    c = SP.melt_c(case.cfg)
    floor = case.floor[sel]
    scale = np.maximum(np.abs(ref["E_in"]), floor)
    S = np.maximum(scale, np.abs(ref["cold"]))
    hist32 = fp32 and not one_cell
    t_ref = SP.melt_tail(case.cfg, ref["E_in"], ref["cold"], ref["P_snow"], ref["P_rain"], st, "reference")
    avail = t_ref["gates"]["avail"]

    # ---- decisions
    dR = SP.melt_decisions(t_ref)
    dG = SP.melt_decisions(G, capped=(G["SM"] > 0) & (np.abs(G["SM"] * 3600 - avail) < 0.5 * SP.MELT_MARGIN * S * c))
    rep["decisions"] = {k: {"true": int(dR[k].sum()), "false": int((~dR[k]).sum()), "differing": int((dG[k] != dR[k]).sum())}
                        for k in dR}
    for k in dR:
        bad = dG[k] != dR[k]
        if bad.any():
            i = int(np.nonzero(bad)[0][0])
            failures.append(f"decisions: {k} differs from the oracle's in {int(bad.sum())} of {bad.size} cells; first cell {sel[i]} "
                            f"(point {case.point[sel[i]]}, axes {[int(a[sel[i]]) for a in getattr(case, 'ax', ())]}): engine "
                            + ", ".join(f"{n}={G[n][i]!r}" for n in ("SM", "IM", "h_swe", "h_iwe", "Eccs", "Ecci"))
                            + "; oracle " + ", ".join(f"{n}={ref[n][i]!r}" for n in ("SM", "IM", "h_swe", "h_iwe", "Eccs", "Ecci", "E_in")))

    # ---- parity against the oracle
    rep["parity_max_error_over_tolerance"] = {}
    for name, f in unit.items():
        if name not in G:
            continue
        lim = tol * scale + (F32 * np.abs(ref[name]) * f if hist32 and name in SP.OUTS else 0.0)
        err = np.abs(G[name] - ref[name]) * f
        worst = float(np.max(np.where(lim > 0, err / np.where(lim > 0, lim, 1.0), np.where(err > 0, np.inf, 0.0))))
        rep["parity_max_error_over_tolerance"][name] = worst
        print(f"{case.name} parity {name}: worst error / tolerance {worst:.3e}")
        if not worst <= 1.0:
            i = int(np.argmax(err - lim))
            failures.append(f"parity: {name} at cell {sel[i]}: engine {G[name][i]!r}, oracle {ref[name][i]!r}; error {err[i]:.3e} J m-2 "
                            f"equivalent against {lim[i]:.3e} (E_in {ref['E_in'][i]!r}, floor {floor[i]:.4g})")
    out_eps = F32 if hist32 else 2.0 ** -52
    mt = np.abs(G["M_total"] - (G["SM"] + G["IM"] + ref["P_rain"] / 3600))
    if np.any(mt > 3 * out_eps * np.abs(G["M_total"])):
        failures.append(f"M_total is not SM + IM + P_rain / 3600 to rounding in {int((mt > 3 * out_eps * np.abs(G['M_total'])).sum())} cells")

    # ---- isolation: the engine's own E_in and cold through the restatement
    K, has = P["K"], P["readable"]
    E_eng = np.where(has, K - P["Ecci"], 0.0)
    cold_eng = np.where(has & (ref["P_snow"] > 0), (P["Eccs"] - K) + E_eng, 0.0)
    t = SP.melt_tail(case.cfg, E_eng, cold_eng, ref["P_snow"], ref["P_rain"], st, "fast" if fp32 else "reference")
    exact = has & bool(P["fp32_flux"]) & ((cold_eng == 0) | (np.abs(cold_eng) >= K * 2.0 ** -28))
    M = np.maximum.reduce([np.abs(E_eng), st["Eccs"], st["Ecci"], avail / c, st["h_iwe"] / c])
    bound = np.where(exact, 0.0, 2.0 ** -52 * (4 * K + 16 * M))
    rep["isolation"] = {"cells": int(has.sum()), "cells_not_readable": int((~has).sum()), "probe_exact": int(exact.sum()),
                        "max_error_J_m2": {}, "entries_not_bit_equal_where_exact": {}}
    for name, f in unit.items():
        if name not in G:
            continue
        want = t[name]
        lim = bound.copy()
        if hist32 and name in SP.OUTS:
            if name in ("h_snow", "h_ice"):
                want = want.astype(np.float32).astype(np.float64)
            lim = lim + np.where(exact & (name != "M_total"), 0.0, (5 if name == "M_total" else 1) * F32 * np.abs(want) * f)
        err = np.where(has, np.abs(G[name] - want) * f, 0.0)
        rep["isolation"]["max_error_J_m2"][name] = float(err.max())
        nb = has & exact & ~_bits(G[name], want)
        rep["isolation"]["entries_not_bit_equal_where_exact"][name] = int(nb.sum())
        bad = err > lim
        if bad.any():
            i = int(np.nonzero(bad)[0][0])
            failures.append(f"isolation: {name} differs from the restatement fed the engine's own E_in in {int(bad.sum())} cells; first "
                            f"cell {sel[i]}: engine {G[name][i]!r}, restated {want[i]!r} (E_in {E_eng[i]!r}, cold {cold_eng[i]!r}, probe "
                            f"{'exact' if exact[i] else 'rounded'}, bound {lim[i]:.3e} J m-2)")


def _probe(case, cells, run):
    """The read-back of the probe run on `cells`: run(probe case, ecc) -> {Eccs, Ecci} per cell of `cells`,
    stepped from step_probe.melt_probe_case's depths with K in both cold contents."""
    pc = SP.melt_probe_case(case)
    K_all = SP.probe_ecc(case.ref["E_in"])
    P = run(pc, (K_all, K_all))
    P.update(cells=cells, K=K_all[cells], readable=pc.readable[cells])
    return P


@pytest.mark.gpu
@pytest.mark.parametrize("form,dt", CASES, ids=[f"dt{d:g}-{f[0]}" for f, d in CASES])
def test_melt_and_state_update_against_the_oracle_state_by_state(form, dt):
    fname, engine, sat, nan_safe = form
    fp32 = engine != "float64"
    tol = 1e-5 if fp32 else 1e-10
    case = SP.melt_case(sat, dt)
    srt, mix = SP.layouts_of(SP.melt_classes(case))
    first = SP.first_lane(srt, case.n)
    catch = (case.point, case.n_points)
    ecc = (case.st["Eccs"], case.st["Ecci"])
    kw = dict(extra=("h_iwe",), catch=catch)
    g_srt = SP.gpu_probe(case, engine, sat, nan_safe, srt, ecc=ecc, **kw)
    g_mix = SP.gpu_probe(case, engine, sat, nan_safe, mix, ecc=ecc, **kw)
    names = SP.READ + SP.OUTS + ("h_iwe",)
    failures = []
    rep = _REPORT.setdefault(fname, {}).setdefault(f"dt{dt:g}", {})
    rep["cells"], rep["depths_moved_off_a_last_place_residual"] = case.n, case.moved

    # ---- layout
    rep["layout_entries_differing"] = 0
    for lay, g, what in ((srt, g_srt, "sorted"), (mix, g_mix, "interleaved")):
        for name in names:
            bad = ~_bits(g_srt[name][:, first[lay]], g[name])
            rep["layout_entries_differing"] += int(bad.sum())
            if bad.any():
                k, lane = np.argwhere(bad)[0]
                failures.append(f"layout: {name} of cell {lay[lane]} differs in the {what} layout at lane {lane}, step {k} "
                                f"({int(bad.sum())} entries)")

    all_cells = np.arange(case.n)
    G = {name: g_srt[name][case.step_cell, first] for name in names}
    P = _probe(case, all_cells, lambda pc, e: {k: v[case.step_cell, all_cells] for k, v in
                                               SP.gpu_probe(pc, engine, sat, nan_safe, SP.pad_to_waves(all_cells), ecc=e).items()
                                               if k in ("Eccs", "Ecci")})
    P["fp32_flux"] = engine == "float32"
    _check_cells(case, G, P, fp32, tol, False, failures, rep)

    # ---- integrals, per forcing point (catchment), over the lanes of each layout
    c = SP._cfgc(case.cfg)
    to_vol = SP.melt_c(case.cfg) * c["da"] * 1e6 * dt
    step_pt = np.array([case.step_cell[case.point == p][0] for p in range(case.n_points)])
    rep["integrals_max_error_over_tolerance"] = {}
    for lay, g in ((srt, g_srt), (mix, g_mix)):
        lim = np.bincount(case.point[lay], weights=tol * np.maximum(np.abs(case.ref["E_in"]), case.floor)[lay] * to_vol)
        for col, name in ((3, "vol_SM"), (4, "vol_IM")):
            want = np.bincount(case.point[lay], weights=case.ref[name][lay])
            got = g["diag"][step_pt, np.arange(case.n_points), col]
            worst = float(np.max(np.abs(got - want) / lim))
            rep["integrals_max_error_over_tolerance"][name] = max(worst, rep["integrals_max_error_over_tolerance"].get(name, 0.0))
            if not worst <= 1.0:
                p = int(np.argmax(np.abs(got - want) / lim))
                failures.append(f"integrals: {name} of point {p}: engine {got[p]!r}, oracle {want[p]!r} (allowed {lim[p]:.3e})")

    # ---- the melt-out residual sweeps, two steps
    for ice in (False, True):
        mo = SP.meltout_case(sat, dt, ice)
        sub = SP.with_steps(mo, [int(mo.step_cell[0])])
        z = np.zeros(mo.n)
        g = SP.gpu_probe(sub, engine, sat, nan_safe, np.arange(mo.n), ecc=(z, z), extra=("h_iwe",), follow=1)
        want = SP.meltout_steps(mo, "fast" if fp32 else "reference")
        r = rep.setdefault("melt_out", {}).setdefault("ice" if ice else "snow", {})
        for name in ("h_swe", "h_iwe"):
            bad = ~_bits(g[name][0], want[0][name])
            r[f"{name}_after_step_1_not_bit_equal"] = int(bad.sum())
            if bad.any():
                i = int(np.nonzero(bad)[0][0])
                failures.append(f"melt-out ({mo.name}): {name} after the first step differs in {int(bad.sum())} of {mo.n} depths; first "
                                f"from {mo.st[name][i]!r}: engine {g[name][0][i]!r}, restated {want[0][name][i]!r}")
        gate = (g["IM@1"][0] == 0) != (want[1]["IM"] == 0)
        r["IM_of_step_2_gate_differing"] = int(gate.sum())
        r["residual_zero_share"] = float(np.mean(g["h_iwe" if ice else "h_swe"][0] == 0))
        if gate.any():
            failures.append(f"melt-out ({mo.name}): the second step's IM is zero in the one and not in the other at {int(gate.sum())} depths")
        k = SP.melt_c(mo.cfg)
        same = (want[1]["IM"] == 0) == (mo.ref2["IM"] == 0)  # where this arithmetic's gate is the oracle's, so is IM, within tol
        err = np.abs(g["IM@1"][0] - mo.ref2["IM"]) * 3600 / k
        lim = tol * np.maximum(np.abs(mo.ref2["E_in"]), mo.floor) + (F32 * mo.ref2["IM"] * 3600 / k if fp32 else 0.0)
        if np.any((err > lim) & same & ~gate):
            failures.append(f"melt-out ({mo.name}): the second step's IM is off by up to {float(err[same & ~gate].max()):.3e} J m-2 equivalent")
        for tag in ("", "@1"):
            mt = np.abs(g["M_total" + tag][0] - (g["SM" + tag][0] + g["IM" + tag][0]))
            if np.any(mt > 3 * (F32 if fp32 else 2.0 ** -52) * g["M_total" + tag][0]):
                failures.append(f"melt-out ({mo.name}): M_total is not SM + IM at a capped step")
    _write_report()
    assert not failures, "\n".join(failures)


@pytest.mark.gpu
@pytest.mark.parametrize("kernel,sat,dt", ONE_CELL, ids=[f"{k}-{'sat-' if s else ''}dt{d:g}" for k, s, d in ONE_CELL])
def test_the_one_cell_kernels_melt_and_state_update(kernel, sat, dt):
    case = SP.melt_case(sat, dt)
    rng = np.random.default_rng(SP.SAMPLE_SEED)
    cells = np.sort(rng.choice(case.n, N_ONE, replace=False))
    ps = np.stack([cells, case.step_cell[cells]], axis=1)
    names = SP.READ + SP.OUTS + ("h_iwe",)
    handles = []
    G = SP.gpu_probe_one_cell(case, kernel, sat, ps, handles=handles, ecc=(case.st["Eccs"], case.st["Ecci"]), extra=("h_iwe",))
    G = {k: G[k] for k in names}
    P = _probe(case, cells, lambda pc, e: {k: v for k, v in SP.gpu_probe_one_cell(pc, kernel, sat, ps, ecc=e).items() if k in ("Eccs", "Ecci")})
    P["fp32_flux"] = False
    failures = []
    rep = _REPORT.setdefault(kernel + ("-sat" if sat else ""), {}).setdefault(f"dt{dt:g}", {})
    rep["cells"] = len(cells)
    _check_cells(case, G, P, False, 1e-10, True, failures, rep)
    # ---- integrals: each handle's SM and IM sums over the run of consecutive states it stepped
    per = -(-len(cells) // len(handles))
    to_vol = SP.melt_c(case.cfg) * SP._cfgc(case.cfg)["da"] * 1e6 * dt
    rep["integrals_max_error_over_tolerance"] = {"vol_SM": 0.0, "vol_IM": 0.0}
    for j, (diag, _, _) in enumerate(handles):
        mine = cells[j * per:(j + 1) * per]
        if not len(mine):  # k_cell_many's pool has more handles than the sample needs
            assert not diag[0, 3] and not diag[0, 4]
            continue
        lim = float(np.sum(1e-10 * np.maximum(np.abs(case.ref["E_in"]), case.floor)[mine] * to_vol))
        for col, name in ((3, "vol_SM"), (4, "vol_IM")):
            want = float(np.sum(case.ref[name][mine]))
            worst = abs(diag[0, col] - want) / lim
            rep["integrals_max_error_over_tolerance"][name] = max(worst, rep["integrals_max_error_over_tolerance"][name])
            if not worst <= 1.0:
                failures.append(f"integrals: {name} of handle {j}: engine {diag[0, col]!r}, oracle {want!r} (allowed {lim:.3e})")
    for ice in (False, True):
        mo = SP.meltout_case(sat, dt, ice)
        pick = np.sort(rng.choice(mo.n, N_ONE_SWEEP, replace=False))
        z = np.zeros(mo.n)
        g = SP.gpu_probe_one_cell(mo, kernel, sat, np.stack([pick, mo.step_cell[pick]], axis=1), ecc=(z, z), extra=("h_iwe",),
                                  follow=1)  # the second step on the same handle, from the state its first step left
        r = rep.setdefault("melt_out", {})
        tag = "ice" if ice else "snow"
        for name in ("h_swe", "h_iwe"):
            bad = ~_bits(g[name], mo.ref[name][pick])
            r[f"{tag}_{name}_not_bit_equal"] = int(bad.sum())
            if bad.any():
                failures.append(f"melt-out ({mo.name}): {name} after the step differs from the oracle's bits at {int(bad.sum())} depths")
        gate = (g["IM@1"] == 0) != (mo.ref2["IM"][pick] == 0)
        r[f"{tag}_IM_of_step_2_gate_differing"] = int(gate.sum())
        r[f"{tag}_IM_of_step_2_zero"] = int((g["IM@1"] == 0).sum())
        if gate.any():
            failures.append(f"melt-out ({mo.name}): the second step's IM is zero in the one and not in the other at {int(gate.sum())} depths")
        k = SP.melt_c(mo.cfg)
        err = np.abs(g["IM@1"] - mo.ref2["IM"][pick]) * 3600 / k
        lim = 1e-10 * np.maximum(np.abs(mo.ref2["E_in"]), mo.floor)[pick]
        r[f"{tag}_IM_of_step_2_max_error_over_tolerance"] = float(np.max(err / lim))
        if np.any(err > lim):
            failures.append(f"melt-out ({mo.name}): the second step's IM is off by up to {float(err.max()):.3e} J m-2 equivalent")
        for name in ("h_swe", "h_iwe"):   # the state the second step leaves, from the oracle's own second step
            bad = ~_bits(g[name + "@1"], mo.ref2[name][pick]) & (name == "h_swe" or ice)
            if np.any(bad):
                failures.append(f"melt-out ({mo.name}): {name} after the second step differs from the oracle's bits at {int(bad.sum())} depths")
    _write_report()
    assert not failures, "\n".join(failures)
