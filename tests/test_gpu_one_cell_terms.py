"""The one-catchment kernels' step (k_cell: tfg_update; k_cell_many: tfg_update_many), one launch per sampled
(point, step) of the energy probe's sweeps (tests/step_probe.py; the samples' conditions are checked on the
oracle alone in tests/test_step_probe_host.py).  These kernels run cell_step_exact_wave, their own
restatement of the fp64 step with the transcendentals exchanged between lanes and waves through LDS; the
grid probe (test_gpu_step_terms.py) never runs it.

Per kernel, vapour formulas (default, Satterlund) and sweep:

  parity    E_in = Q_sum dt and the snowfall's cold content against the oracle's at 1e-10 (the probe's fp64
            tolerance) by the project's floored relative error; the floor is scale_floor of the FULL sweep's
            stratum, so sampling cannot move it.  Only points of the probe's linear range; no cut rule
            (fp64 inputs are not rounded).  Rain brings a cold content of exactly 0.
  dark      sweeps C and Cb: the short-wave term (a step's E_in minus the dark step's of the same point) is
            zero exactly where the oracle's is, at every sampled pair; no allowance.
  nan       where the oracle's E_in is NaN, the kernel's is NaN.
  bits      Eccs, Ecci, h_swe, n, albedo and the six outputs have the bits of the grid kernel
            (gpu_probe, float64) stepping the sampled points as a 1 x n grid over the sampled steps: the
            kernels' "same arithmetic as k_fused<double>, so the same bits".
  diag      every handle's vol_P, vol_PR, vol_PS and P_max equal the fp64 sums, in order, of the P da dt it
            was fed (1e-12 relative, the bar of test_one_cell_kernels_against_the_grid_and_the_reference;
            P_max exactly).

test_mixed_launch_equals_single_launches: one tfg_update_many call over more workgroups than the chip has
CUs, mixing configurations, against the same points stepped alone through k_cell, bit for bit.

The sample is one_cell_sample's as it stands: sweep A has no per-combination extras beyond the one point
per combination, and the C-lat hours are the mandatory 48; nothing was thinned further.

The measured maxima and each case's wall time go to $TFG_REPORT_DIR/one_cell_terms.json
(profiles/one_cell_terms.json is a GPU run's copy); no assertion reads them.
"""

from __future__ import annotations

import json
import os
import time

import numpy as np
import pytest

from tests import step_probe as SP
from tests.harness import scale_floor

TOL = 1e-10
DIAG_TOL = 1e-12
CASES = [(kernel, sat, sweep) for sweep in SP.SWEEPS for sat in (False, True) for kernel in SP.ONE_CELL_KERNELS]
_REPORT: dict = {}
_GRID: dict = {}


def _write_report():
    d = os.environ.get("TFG_REPORT_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "one_cell_terms.json"), "w") as f:
            json.dump(_REPORT, f, indent=1, sort_keys=True)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))


def _grid_probe(sweep, sat):
    """The grid kernel on the sample's points (padded to whole waves) over the sample's steps, once per
    (sweep, formulas): (result of gpu_probe, points, steps)."""
    key = (sweep, sat)
    if key not in _GRID:
        s, ps = SP.get_sweep(sweep, sat), SP.one_cell_sample(sweep, sat)
        pts, steps = np.unique(ps[:, 0]), np.unique(ps[:, 1])
        g = SP.gpu_probe(SP.with_steps(s, steps), "float64", sat, None, SP.pad_to_waves(pts))
        for v in g.values():
            v.setflags(write=False)
        _GRID[key] = (g, pts, steps)
    return _GRID[key]


def _diag_failures(cfg, handles, what):
    """The fed precipitation sums of each handle; returns (failures, largest relative error)."""
    failures, worst = [], 0.0
    for j, (rows, P, T) in enumerate(handles):
        want = SP.fed_diagnostics(cfg, P, T)
        if rows.shape != (1, 6):
            failures.append(f"diag: {what} handle {j}: diagnostics of shape {rows.shape}")
            continue
        got = rows[0, [0, 1, 2, 5]]
        err = np.abs(got[:3] - want[:3])
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.where(want[:3] != 0, err / np.abs(want[:3]), np.where(err > 0, np.inf, 0.0))
        worst = max(worst, float(rel.max()))
        if not (rel <= DIAG_TOL).all() or got[3] != want[3]:
            failures.append(f"diag: {what} handle {j}: vol_P, vol_PR, vol_PS, P_max {got!r}, fed {want!r}")
    return failures, worst


@pytest.mark.gpu
@pytest.mark.parametrize("kernel,sat,sweep", CASES, ids=[f"{s}-{k}{'-sat' if t else ''}" for k, t, s in CASES])
def test_one_cell_step_terms_against_the_oracle_and_the_grid_kernel(kernel, sat, sweep):
    t0 = time.perf_counter()
    s, ref, ps = SP.get_sweep(sweep, sat), SP.reference(sweep, sat), SP.one_cell_sample(sweep, sat)
    P, K = ps[:, 0], ps[:, 1]
    cfg = dict(s.cfg, SATTERLUND=sat)
    t1 = time.perf_counter()
    handles = []
    G = SP.gpu_probe_one_cell(s, kernel, sat, ps, handles)
    t_probe = time.perf_counter() - t1
    failures = []
    rep = _REPORT.setdefault(f"{kernel}{'-sat' if sat else ''}", {}).setdefault(sweep, {})
    rep["pairs"], rep["probe_ms_per_pair"] = int(len(ps)), 1e3 * t_probe / len(ps)

    # ---- parity, per stratum of the full sweep
    lin = SP.linear(s, ref)
    rep["strata"] = {}
    for label, steps, pts in SP.strata(s):
        out = rep["strata"].setdefault(label, {})
        mine = steps[K] & pts[P]
        for key, ok_pts in (("E_in", np.ones(s.n, bool)), ("cold", s.cold_ok)):
            full = SP.stratum_block(ref[key], steps, pts)[SP.stratum_block(lin & ok_pts[None, :], steps, pts)]
            sel = mine & lin[K, P] & ok_pts[P]
            if not full.size or not sel.any():
                continue
            s_v = scale_floor(full)
            g, r = G[key][sel], ref[key][K[sel], P[sel]]
            d = np.abs(np.where(np.isfinite(g), g, np.inf) - r) / np.maximum(np.abs(r), s_v)
            err = float(d.max())
            out[f"{key}_max_floored_error"], out[f"{key}_floor"], out[f"{key}_pairs"] = err, s_v, int(sel.sum())
            print(f"{kernel} sat={sat} {sweep} {label}: {key} floored error {err:.3e} (floor {s_v:.4g}, {int(sel.sum())} pairs)")
            if not err <= TOL:
                j = int(np.argmax(d))
                pp, kk = P[sel][j], K[sel][j]
                failures.append(f"parity: {key} in {label}: floored error {err:.3e} > {TOL:g}; worst at step {kk}, point {pp}: "
                                f"kernel {g[j]!r}, oracle {r[j]!r}, inputs "
                                + ", ".join(f"{n}={s.pts[n][pp]!r}" for n in SP.FORCING))
        rain = mine & lin[K, P] & (s.cold_ok & ~s.snowing)[P]
        if rain.any() and np.any(G["cold"][rain] != 0.0):
            failures.append(f"parity: {label}: rain brought a cold content")

    # ---- nan
    with np.errstate(invalid="ignore"):
        lost = ~np.isnan(G["E_in"]) & np.isnan(ref["E_in"][K, P])
    rep["oracle_nan_pairs"], rep["pairs_not_nan_where_the_oracle_is_nan"] = int(np.isnan(ref["E_in"][K, P]).sum()), int(lost.sum())
    if lost.any():
        j = int(np.argmax(lost))
        failures.append(f"nan: {int(lost.sum())} pairs are not NaN where the oracle's E_in is NaN; first at step {K[j]}, "
                        f"point {P[j]} (Hum_sp {s.pts['Hum_sp'][P[j]]!r}): kernel {G['E_in'][j]!r}")

    # ---- the dark decision
    if sweep.startswith("C"):
        first = {int(p): j for j, (p, k) in enumerate(ps) if k == 0}
        dark0 = G["E_in"][[first[int(p)] for p in P]]
        sel = K > 0
        wrong = ((G["E_in"] - dark0 == 0) != (ref["Qn_SW"][K, P] == 0)) & sel
        rep["dark_decisions"], rep["dark_decisions_wrong"] = int(sel.sum()), int(wrong.sum())
        if wrong.any():
            j = int(np.argmax(wrong))
            failures.append(f"dark: {int(wrong.sum())} of {int(sel.sum())} decisions differ from the oracle's; first at step "
                            f"{K[j]} (jd {s.jd[K[j]]!r}, th {s.th[K[j]]!r}), point {P[j]} (slope {s.pts['slope'][P[j]]}, aspect "
                            f"{s.pts['aspect'][P[j]]}): kernel short wave {(G['E_in'][j] - dark0[j]) / s.cfg['dt']!r}, "
                            f"oracle {ref['Qn_SW'][K[j], P[j]]!r}")

    # ---- bits: the grid kernel on the same points and steps
    grid, gp, gk = _grid_probe(sweep, sat)
    lane, row = np.searchsorted(gp, P), np.searchsorted(gk, K)
    differing = 0
    for name in SP.READ + SP.OUTS:
        bad = ~_same_bits(G[name], grid[name][row, lane])
        differing += int(bad.sum())
        if bad.any():
            j = int(np.argmax(bad))
            failures.append(f"bits: {name} at step {K[j]}, point {P[j]} ({int(bad.sum())} pairs): kernel {G[name][j]!r}, "
                            f"grid kernel {grid[name][row[j], lane[j]]!r}, inputs "
                            + ", ".join(f"{n}={s.pts[n][P[j]]!r}" for n in SP.FORCING))
    rep["bits_entries_differing"] = differing

    # ---- the handles' precipitation integrals
    dfail, rep["diag_max_rel_error"] = _diag_failures(cfg, handles, kernel)
    failures += dfail
    assert sum(len(h[1]) for h in handles) == len(ps)
    rep["wall_s"] = time.perf_counter() - t0
    _write_report()
    assert not failures, "\n".join(failures)


# ----------------------------------------------------------------------------------------------- the mixed launch
MIXED_PER_CONFIG = 30


def _mixed_jobs():
    """[(sweep, satterlund, point, step, extra)]: MIXED_PER_CONFIG pairs of each of sweep B's two T_rain_snow
    and sweep C's three latitudes under both vapour formulas, evenly spaced through the one-cell sample,
    then one handle of three catchments with its cell in catchment 2 and one with the fixed ground heat
    flux on."""
    jobs = []
    for sweep in ("B-Trs0", "B-Trs50.2", "C-lat0", "C-lat46.8", "C-lat70"):
        for sat in (False, True):
            ps = SP.one_cell_sample(sweep, sat)
            for j in np.linspace(0, len(ps) - 1, MIXED_PER_CONFIG).astype(int):
                jobs.append((sweep, sat, int(ps[j, 0]), int(ps[j, 1]), None))
    # the three-catchment handle is fed snowfall (sweep C's albedo state with P = 0.002 at T_air = -3) at a
    # day step, so its own row of the diagnostics is not zero
    s, ps = SP.get_sweep("C-lat46.8", True), SP.one_cell_sample("C-lat46.8", True)
    j = int(np.nonzero((s.pts["P"][ps[:, 0]] > 0) & ~s.night[ps[:, 1]])[0][10])
    jobs.append(("C-lat46.8", True, int(ps[j, 0]), int(ps[j, 1]), "catchment"))
    ps = SP.one_cell_sample("B-Trs0", True)
    jobs.append(("B-Trs0", True, int(ps[400, 0]), int(ps[400, 1]), "ground"))
    return jobs


Q_GROUND = 0.07  # [W m-2] the fixed ground heat flux of the one handle that has it


def _mixed_engine(s, sat, extra, shared):
    cfg = dict(s.cfg, SATTERLUND=sat)
    if extra == "catchment":
        return SP.one_cell_engine(cfg, n_catch=3, cell_catchment=2, shared_stream=shared)
    e = SP.one_cell_engine(cfg, shared_stream=shared)
    if extra == "ground":
        e.set_field("Qc", np.float64(Q_GROUND))
    return e


def _read_all(e, out):
    return ({"out": out.copy(), "diag": e.diagnostics()}
            | {name: e.get_field(name) for name in ("h_swe", "h_iwe", "Eccs", "Ecci", "n", "albedo")})


@pytest.mark.gpu
def test_mixed_launch_equals_single_launches():
    """ONE tfg_update_many call over 302 handles (more workgroups than the chip has CUs) that mix Satterlund
    on and off, sweep B's two T_rain_snow, sweep C's three latitudes, a handle of three catchments whose cell
    sits in catchment 2 and a handle with the fixed ground heat flux on, each stepping its own sampled
    point: every handle's eight outputs, state and diagnostics equal, bit for bit, the same point stepped
    alone through k_cell; the row of the handle's own catchment holds the fed P da dt (vol_P, vol_PR, vol_PS
    to 1e-12, P_max exactly) and the rows of the other catchments stay 0.  The three-catchment handle is
    fed snowfall, so its row 2 is not zero."""
    t0 = time.perf_counter()
    jobs = _mixed_jobs()
    assert len(jobs) >= 300
    sweeps = {(sw, sat): SP.get_sweep(sw, sat) for sw, sat, *_ in jobs}
    clocks = {key: SP.probe_clock(s) for key, s in sweeps.items()}
    us = [SP.probe_uniform(clocks[sw, sat], k) for sw, sat, _, k, _ in jobs]
    vals = [SP.point_inputs(sweeps[sw, sat], p) for sw, sat, p, _, _ in jobs]
    engines, many = [], []
    try:
        for sw, sat, p, _, extra in jobs:
            engines.append(_mixed_engine(sweeps[sw, sat], sat, extra, True))
            SP.inject_point(engines[-1], sweeps[sw, sat], p)
        outs = [np.full((8, 1), np.nan) for _ in jobs]
        SP.update_batch(engines, vals, us, outs)
        many = [_read_all(e, o) for e, o in zip(engines, outs)]
    finally:
        for e in engines:
            e.close()
    alone, singles = [], {}
    try:
        out = np.empty((8, 1))
        for j, (sw, sat, p, _, extra) in enumerate(jobs):
            e = singles.get((sw, sat, extra))
            if e is None:
                e = singles[sw, sat, extra] = _mixed_engine(sweeps[sw, sat], sat, extra, False)
            else:
                e.init_state()  # the diagnostics row starts from zero again
            SP.inject_point(e, sweeps[sw, sat], p)
            out[:] = np.nan
            SP.update_one(e, vals[j], us[j], out)
            alone.append(_read_all(e, out))
        # the ground-flux handle's point once more without the flux
        g = next(j for j, job in enumerate(jobs) if job[4] == "ground")
        sw, sat, p, _, _ = jobs[g]
        e = singles[sw, sat, None]
        e.init_state()
        SP.inject_point(e, sweeps[sw, sat], p)
        SP.update_one(e, vals[g], us[g], out)
        no_flux = e.get_field("Ecci")[0]
    finally:
        for e in singles.values():
            e.close()
    differing = 0
    for j, (a, b) in enumerate(zip(many, alone)):
        for name in a:
            same = a[name].shape == b[name].shape and bool(_same_bits(a[name], b[name]).all())
            differing += not same
            assert same, (jobs[j], name, a[name], b[name])
        row = 2 if jobs[j][4] == "catchment" else 0
        assert a["diag"].shape == ((3, 6) if jobs[j][4] == "catchment" else (1, 6))
        assert np.all(np.delete(a["diag"], row, axis=0) == 0.0), (jobs[j], a["diag"])
        P_fed, T_fed = vals[j][2, 0], vals[j][3, 0]
        want = SP.fed_diagnostics(sweeps[jobs[j][0], jobs[j][1]].cfg, [P_fed], [T_fed])
        got = a["diag"][row, [0, 1, 2, 5]]
        assert np.all(np.abs(got[:3] - want[:3]) <= DIAG_TOL * np.abs(want[:3])) and got[3] == want[3], (jobs[j], got, want)
        if jobs[j][4] == "catchment":
            assert P_fed > 0 and got[0] > 0 and got[2] > 0 and got[3] == P_fed, (jobs[j], got)
            assert np.all(a["diag"][:2] == 0.0), (jobs[j], a["diag"])
    # the ground heat flux reached the step: E_in = Q_sum dt is larger by Q_GROUND dt than without it
    # (to the 2^-32 of the subtractions from ECC0)
    d_e = no_flux - many[g]["Ecci"][0]
    assert abs(d_e - Q_GROUND * sweeps[jobs[g][0], jobs[g][1]].cfg["dt"]) <= 1e-8, d_e
    _REPORT["mixed_launch"] = {"handles": len(jobs), "entries_differing": int(differing), "wall_s": time.perf_counter() - t0}
    _write_report()
