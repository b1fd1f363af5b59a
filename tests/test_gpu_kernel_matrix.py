"""Every instantiation of k_fused at a fused depth, against the numpy oracle
and against its siblings.

k_fused<R, EXACT, READ_DEPTHS, CATCH, QC, C, NS, PREC, SAT> is compiled 72
times: the fp32 engine's four forms (default, fp64 flux PREC, Satterlund SAT,
both), each for READ_DEPTHS x CATCH x QC x NS (launch_fused_fast), and the fp64
engine's READ_DEPTHS x CATCH x QC (launch_fused_exact).  Each is machine code of
its own: the read-ahead drops from two steps to one under QC, NS or PREC,
PREC with CATCH keeps a third, unpeeled step loop, the launch sums sit in LDS
without CATCH and in registers with it.  The rest of the suite moves one flag
at a time off the default; here every combination runs.

Inputs.  tests/harness.py:bare_ice_inputs(4, 5, 77, 24): 385 cells, two
256-cell chunks, the second ragged.  n_frames 24, hist_depth 21, fuse_steps 24;
step k reads frame k.  21 steps as run(13) then run(8): both launches have
K >= 8 (kVerifySteps), so the engine verifies the data and picks the clean form
itself; 13 and 8 cover the peel, the steady rounds and the tail of the 3-step
and the 2-step loops; the first launch reads the depths from the state
(READ_DEPTHS), the second derives them.

A corner is (form, CATCH, QC, NS):
  form   "fp32", "fp32_flux64", each with and without SATTERLUND: true, "fp64"
  CATCH  n_catch = 5 and catch_id = (cell * 37) % 5: five ids in every wave
  QC     Qc = ((cell % 7) - 3) * 10 W m-2, fp32-exact
  NS     set_step_form(True) on finite data (fp32 forms); nan_safe_launches()
         is 2 there and 0 in the clean corners, the one observable of which
         instance ran
and each corner runs in two variants: A as above; B reads the previous-step
depths (TFG_PREV_DEPTH) after the first launch and writes them back, as
checkpoint() / restore() do, so its second launch is the READ_DEPTHS instance
at K = 8.  (Setting a depth also writes the visible output of history slot 0,
so variant B's outputs of steps 0-12 are read before the write-back.)  36
corners x 2 variants launch all 72 kernels; KERNELS below lists their template
arguments, and tests/test_kernel_matrix_host.py holds it to the built library.

Asserted on the oracle alone, before any GPU value is read (check_oracle), for
both vapour formulas, with and without Qc: no cell's h_swe moves between zero
and non-zero and every non-zero depth stays above 1 m (no melt-out gate is in
play, so no cell may be classified as a flip); >= 60 % of the cells have a
snow-melt integral > 0 (68.6 % measured) and >= 20 % an ice-melt integral > 0
(22.3 %); Qc moves M_total by more than 1e-4 of its largest value in >= 150
cells (183 Brutsaert, 186 Satterlund).

Anchors.  Per form, the corners (CATCH 0, NS 0, variant A) with QC 0 and QC 1
against the oracle (m.Qc for QC 1): the outputs of all 21 steps and the six
state planes under harness.assert_oracle_rule, floored 1e-5 for the fp32 forms
and 1e-10 for the fp64 engine.
Siblings.  Every other corner and every variant B equals the anchor of its
(form, QC) bit for bit: six outputs x 21 steps, the six state planes, both
previous-step depths, all 72 window slots.  Neither the catchment bins, nor
the NaN-safe max / min on finite data, nor the source of the depths enters a
cell's arithmetic.
Diagnostics.  Corners that differ only in NS or the variant: bit-equal (the
launch partition is the same).  A CATCH corner's columns summed over its five
catchments against the anchor's row: all terms are non-negative, so two
summation orders differ by at most 2 m 2^-53 relative, m = 385 for the fp32
forms (the per-cell launch sums are identical) and 385 * 21 for fp64; P_max
exact.
Missing data.  T_air[3, 70] = P[5, 200] = Hum_sp[2, 301] = NaN, per (form, QC,
CATCH).  On the oracle the NaN cells of the last step are exactly those three.
The CATCH 0 corner against the oracle (equal NaN masks in outputs and state,
the finite values under the rule above); the CATCH 1 corner equals it with
equal_nan; its diagnostics have a NaN in the catchments of those cells (0 and
2) only and equal the clean run's rows elsewhere; the fp32 forms count NaN-safe
launches without set_step_form.

Measured on an MI355X (TFG_REPORT_DIR/kernel_matrix.json; MEASURED below holds
the same figures): the anchors' largest floored error, QC 0 / QC 1,
  form             outputs of 21 steps     state planes
  fp32             7.3e-7 / 7.7e-7 (SM)    1.1e-7 / 1.2e-7 (Ecci)
  fp32_flux64      3.3e-7 / 3.3e-7 (RH)    2.0e-8 / 2.0e-8 (albedo)
  fp32_sat         3.5e-6 / 3.5e-6 (RH)    1.2e-7 / 1.2e-7 (Ecci)
  fp32_flux64_sat  3.5e-6 / 3.5e-6 (RH)    2.2e-8 / 2.2e-8 (Ecci)
  fp64             2.8e-15 / 2.4e-15       6.2e-16 / 6.3e-16
The nearest to its bound is the Satterlund forms' RH, 2.9 times inside 1e-5
(the same figure with the fp64 flux: the RH output is formed in fp32 in both);
every other figure is 13 times or more inside.
Every sibling identity and every diagnostics identity held bit for bit, with
and without missing data.
"""

import functools
from types import SimpleNamespace

import numpy as np
import pytest

import tfg_oracle as O
from tests.harness import (BASE_CFG, FLUX_F64_ENGINE, HIST_OUTPUTS, STATE_PLANES, STATIC_KEYS, assert_oracle_rule,
                           bare_ice_inputs, make_engine, read_run)
from tests.test_gpu_diagnostics import _report

pytestmark = pytest.mark.gpu

# Measured on an MI355X: per form and anchor (QC 0, QC 1), the largest floored error over
# the six outputs of 21 steps and over the six state planes (bounds: 1e-5 fp32 forms, 1e-10 fp64)
MEASURED = {
    "fp32": {"qc0": {"outputs": 7.3e-7, "state": 1.1e-7}, "qc1": {"outputs": 7.7e-7, "state": 1.2e-7}},
    "fp32_flux64": {"qc0": {"outputs": 3.3e-7, "state": 2.0e-8}, "qc1": {"outputs": 3.3e-7, "state": 2.0e-8}},
    "fp32_sat": {"qc0": {"outputs": 3.5e-6, "state": 1.2e-7}, "qc1": {"outputs": 3.5e-6, "state": 1.2e-7}},
    "fp32_flux64_sat": {"qc0": {"outputs": 3.5e-6, "state": 2.2e-8}, "qc1": {"outputs": 3.5e-6, "state": 2.2e-8}},
    "fp64": {"qc0": {"outputs": 2.8e-15, "state": 6.2e-16}, "qc1": {"outputs": 2.4e-15, "state": 6.3e-16}},
}

NY, NX, SEED, NFRAMES = 5, 77, 4, 24
N = NY * NX
LAUNCHES = (13, 8)
NSTEPS = sum(LAUNCHES)
NC = 5
NAN_AT = (("T_air", 3, 70), ("P", 5, 200), ("Hum_sp", 2, 301))
NAN_CELLS = (70, 200, 301)

# form -> engine name of the tests, SATTERLUND, and the kernel's (R, EXACT, PREC, SAT)
FORMS = {
    "fp32": SimpleNamespace(engine="float32", sat=False, R="f", exact=False, prec=False),
    "fp32_flux64": SimpleNamespace(engine=FLUX_F64_ENGINE, sat=False, R="f", exact=False, prec=True),
    "fp32_sat": SimpleNamespace(engine="float32", sat=True, R="f", exact=False, prec=False),
    "fp32_flux64_sat": SimpleNamespace(engine=FLUX_F64_ENGINE, sat=True, R="f", exact=False, prec=True),
    "fp64": SimpleNamespace(engine="float64", sat=False, R="d", exact=True, prec=False),
}
VARIANTS = ("A", "B")
REPORT: dict = {}


def corners_of(form):
    """The (form, CATCH, QC, NS) corners of a form; the anchors (CATCH 0, NS 0) first."""
    ns = (False, True) if FORMS[form].R == "f" else (False,)
    return [(form, catch, qc, n) for catch in (False, True) for n in ns for qc in (False, True)]


def launched_kernels(corner, variant):
    """The k_fused template arguments (R, EXACT, READ_DEPTHS, CATCH, QC, C, NS,
    PREC, SAT) of a run's two launches: the first reads the depths from the
    state, the second only after variant B's write-back."""
    form, catch, qc, ns = corner
    f = FORMS[form]
    return {(f.R, f.exact, rd, catch, qc, 1, ns, f.prec, f.sat and f.R == "f")
            for rd in ((True, False) if variant == "A" else (True, True))}


# what test_every_corner_equals_its_anchor launches
KERNELS = frozenset().union(*(launched_kernels(c, v) for f in FORMS for c in corners_of(f) for v in VARIANTS))


def _frozen(a):
    a = np.asarray(a)
    a.setflags(write=False)
    return a


def _qc_field():
    """A fixed, fp32-exact lateral conduction flux [W m-2], -30 .. 30."""
    return ((np.arange(N) % 7) - 3) * 10.0


def _catch_ids():
    return ((np.arange(N, dtype=np.int64) * 37) % NC).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _inputs(nan=False):
    static, frames = bare_ice_inputs(SEED, NY, NX, NFRAMES)
    if nan:
        for name, step, cell in NAN_AT:
            frames[name][step, cell] = np.nan
    return {k: _frozen(v) for k, v in static.items()}, {k: _frozen(v) for k, v in frames.items()}


@functools.lru_cache(maxsize=None)
def _oracle(sat, qc, nan=False):
    """One numpy-oracle run of the 21 steps, shared read-only: the outputs
    [21][n], the final state planes, h_swe at every step boundary and the
    per-cell melt integrals."""
    static, frames = _inputs(nan)
    cfg = dict(BASE_CFG, SATTERLUND=sat)
    m = O.OracleGrid(cfg, **{k: static[k] for k in STATIC_KEYS})
    if qc:
        m.Qc = _qc_field()
    jd, _, _, tsn = O.oracle_clock(cfg["start_time"], cfg["dt"], NSTEPS, cfg["lon"])
    h_swe, outs = [m.h_swe.copy()], {v: [] for v in HIST_OUTPUTS}
    with np.errstate(invalid="ignore"):
        for k in range(NSTEPS):
            r = m.step(*(frames[v][k] for v in ("P", "T_air", "Hum_sp", "P_air", "uz")), jd[k], tsn[k])
            h_swe.append(np.array(m.h_swe, copy=True))
            for v in HIST_OUTPUTS:
                outs[v].append(np.array(r[v], copy=True))
    return SimpleNamespace(outs={v: _frozen(np.stack(a)) for v, a in outs.items()},
                           state={v: _frozen(np.array(getattr(m, v), dtype=np.float64)) for v in STATE_PLANES},
                           h_swe=_frozen(np.stack(h_swe)), cell_SM=_frozen(np.broadcast_to(m.cell_vol_SM, (N,)).copy()),
                           cell_IM=_frozen(np.broadcast_to(m.cell_vol_IM, (N,)).copy()))


@functools.lru_cache(maxsize=None)
def check_oracle(sat):
    """The preconditions of the module docstring for one vapour formula, on the oracle alone."""
    runs = {qc: _oracle(sat, qc) for qc in (False, True)}
    for qc, o in runs.items():
        zero = o.h_swe == 0
        assert (zero == zero[0]).all(), "a cell's h_swe moved between zero and non-zero: the ice-melt gate is in play"
        for v in ("h_snow", "h_ice"):
            assert o.outs[v][o.outs[v] != 0].min() > 1.0, (v, "a depth near melt-out")
        assert all(np.isfinite(a).all() for a in o.outs.values())
        assert float((o.cell_SM > 0).mean()) >= 0.6, (qc, float((o.cell_SM > 0).mean()))
        assert float((o.cell_IM > 0).mean()) >= 0.2, (qc, float((o.cell_IM > 0).mean()))
    a, b = runs[False].outs["M_total"], runs[True].outs["M_total"]
    moved = int((np.abs(b - a).max(axis=0) > 1e-4 * np.abs(a).max()).sum())
    assert moved >= 150, moved
    for qc in (False, True):  # the missing values stay in their three cells, to the last step
        o = _oracle(sat, qc, nan=True)
        bad = np.zeros(N, dtype=bool)
        for a in (*(x[-1] for x in o.outs.values()), *o.state.values()):
            bad |= np.isnan(a)
        assert np.array_equal(np.nonzero(bad)[0], NAN_CELLS), np.nonzero(bad)[0]
        assert np.array_equal(np.nonzero(np.isnan(o.outs["M_total"][-1]))[0], NAN_CELLS)
    return True


@functools.lru_cache(maxsize=None)
def _run(corner, variant="A", nan=False):
    """One corner's 21 steps on the GPU (harness.read_run's fields), cached read-only."""
    from topoflow_glacier import _native as nat

    form, catch, qc, ns = corner
    f = FORMS[form]
    static, frames = _inputs(nan)
    e = make_engine(dict(BASE_CFG, SATTERLUND=f.sat), NY, NX, f.engine, n_frames=NFRAMES, hist_depth=NSTEPS,
                    n_catch=NC if catch else 1, fuse_steps=24)
    try:
        for k in ("elev", "slope", "aspect"):
            e.set_field(k, static[k])
        for k in ("h_snow", "h_ice", "h_swe", "h_iwe"):
            e.set_field(k, static["h0_" + k[2:]])
        if catch:
            e.set_field("catch_id", _catch_ids())
        e.init_state()
        for k in range(NFRAMES):
            for name in ("P", "T_air", "Hum_sp", "P_air", "uz"):
                e.set_field(name, frames[name][k], index=k)
        if ns:
            e.set_step_form(True)
        if qc:
            e.set_field("Qc", _qc_field())
        e.run(LAUNCHES[0])  # step k reads frame k
        early = None
        if variant == "B":
            e.sync()
            early = {v: np.stack([e.get_field(v, index=k) for k in range(LAUNCHES[0])]) for v in ("h_snow", "h_ice")}
            prev = {v: e.get_field(v, index=nat.PREV_DEPTH) for v in ("h_snow", "h_ice")}
            for v in ("h_snow", "h_ice"):
                e.set_field(v, prev[v], index=nat.PREV_DEPTH)
        e.run(LAUNCHES[1])
        r = read_run(e, NSTEPS)
    finally:
        e.close()
    if early is not None:  # the write-back also wrote the two depths' visible output in history slot 0
        for v, a in early.items():
            r.outs[v][:LAUNCHES[0]] = a
    for a in (*r.outs.values(), *r.state.values(), *r.prev.values(), r.window, r.diag):
        a.setflags(write=False)
    return r


def _assert_same_cells(a, b, what, equal_nan=False):
    for v in HIST_OUTPUTS:
        assert np.array_equal(a.outs[v], b.outs[v], equal_nan=equal_nan), (what, v)
    for v in STATE_PLANES:
        assert np.array_equal(a.state[v], b.state[v], equal_nan=equal_nan), (what, v)
    for v in ("h_snow", "h_ice"):
        assert np.array_equal(a.prev[v], b.prev[v], equal_nan=equal_nan), (what, "previous", v)
    assert a.window.shape == (72, N)
    assert np.array_equal(a.window, b.window, equal_nan=equal_nan), (what, "window slots")


def _anchor_errors(r, o, tol):
    """The anchor against the oracle (asserted); its largest errors over the outputs and over the state."""
    res = assert_oracle_rule(r.outs, r.state, o.outs, o.state, tol)
    assert res.flips == 0, res.flip  # check_oracle: no depth comes near a melt-out gate
    return {"outputs": max(res.err[v] for v in HIST_OUTPUTS), "state": max(res.err[v] for v in STATE_PLANES),
            "per_plane": res.err}


@pytest.mark.parametrize("form", list(FORMS))
def test_every_corner_equals_its_anchor(form):
    """The form's corners x variants (16 runs, 8 for fp64): the two anchors
    against the oracle, every other run against its anchor bit for bit, the
    diagnostics across NS and the variants bit for bit and across CATCH to the
    summation order (module docstring)."""
    f = FORMS[form]
    fp32 = f.R == "f"
    assert check_oracle(f.sat)
    tol = 1e-5 if fp32 else 1e-10
    measured = {}
    for qc in (False, True):
        anchor = _run((form, False, qc, False))
        assert np.isfinite(anchor.diag).all() and anchor.outs["M_total"].any()
        measured[f"qc{int(qc)}"] = _anchor_errors(anchor, _oracle(f.sat, qc), tol)
        print(f"kernel matrix {form} anchor qc={int(qc)}: {measured[f'qc{int(qc)}']}")
    REPORT[form] = measured
    _report("kernel_matrix", REPORT)
    assert not np.array_equal(_run((form, False, False, False)).outs["M_total"],
                              _run((form, False, True, False)).outs["M_total"])  # Qc is in the step
    launched = set()
    for corner in corners_of(form):
        _, catch, qc, ns = corner
        anchor = _run((form, False, qc, False))
        first = _run(corner, "A")
        for variant in VARIANTS:
            r = _run(corner, variant)
            launched |= launched_kernels(corner, variant)
            assert r.ns_launches == (2 if ns else 0), (corner, variant, r.ns_launches)
            _assert_same_cells(r, anchor, (corner, variant))
            assert np.array_equal(r.diag, first.diag), (corner, variant, "diagnostics across the variants")
        assert np.array_equal(first.diag, _run((form, catch, qc, False)).diag), (corner, "diagnostics across NS")
        if catch:
            row = anchor.diag[0]
            assert first.diag.shape == (NC, 6) and np.all(row[:5] > 0)
            m = N if fp32 else N * NSTEPS
            rel = np.abs(first.diag[:, :5].sum(axis=0) - row[:5]) / row[:5]
            assert np.all(rel <= 2 * m * 2.0 ** -53), (corner, rel)
            assert first.diag[:, 5].max() == row[5], (corner, "P_max")
    assert launched == {k for k in KERNELS if (k[0], k[7], k[8]) == (f.R, f.prec, f.sat and fp32)}
    assert len(launched) == (16 if fp32 else 8)


@pytest.mark.parametrize("form", list(FORMS))
def test_missing_data_in_every_corner(form):
    """Three NaN forcing values, per (QC, CATCH) of the form: the CATCH 0 run
    against the oracle, the CATCH 1 run against it with equal_nan, the
    diagnostics NaN in the catchments of the three cells only, and the fp32
    forms in their NaN-safe instances by the engine's own choice."""
    f = FORMS[form]
    fp32 = f.R == "f"
    assert check_oracle(f.sat)
    hit = sorted({int(c) for c in _catch_ids()[list(NAN_CELLS)]})
    assert hit == [0, 2]
    for qc in (False, True):
        o = _oracle(f.sat, qc, nan=True)
        plain = _run((form, False, qc, False), nan=True)
        res = assert_oracle_rule(plain.outs, plain.state, o.outs, o.state, 1e-5 if fp32 else 1e-10)
        assert res.flips == 0, res.flip
        binned = _run((form, True, qc, False), nan=True)
        _assert_same_cells(binned, plain, (form, qc, "CATCH"), equal_nan=True)
        clean = _run((form, True, qc, False))
        assert np.array_equal(np.nonzero(np.isnan(binned.diag).any(axis=1))[0], hit), binned.diag
        others = [c for c in range(NC) if c not in hit]
        assert np.array_equal(binned.diag[others], clean.diag[others])
        assert np.isnan(plain.diag).any()
        for r in (plain, binned):
            assert (r.ns_launches > 0) if fp32 else (r.ns_launches == 0), (form, qc, r.ns_launches)
