"""The per-catchment mass-balance reduction (vol_P, vol_PR, vol_PS, vol_SM,
vol_IM, P_max; tfg_get_diag) at its edges: every layer of it -- the per-cell
sums of a launch, wave_flush's pass per distinct id of a wave, the slab row per
workgroup (several chunks per workgroup, the second part of a split launch),
k_diag_reduce, and the one-cell kernels that write their slab row directly --
against a plain high-precision reference.

Inputs.  tests/harness.py:bare_ice_inputs: the synthetic workload with every
third cell bare, dry ice (no snow, no precipitation), so that the exact-zero
snow gate of the ice melt (:1424) moves in no cell and the ice-melt integral is
non-zero and well conditioned.  Each test asserts on the numpy oracle, before
it looks at a GPU value, that no cell's h_swe changes between zero and
non-zero, that at least 20 % of the cells have an ice-melt integral > 0 and at
least 25 % a snow-melt integral > 0.  (The ice share is 20-21 % on these
grids -- 60 % of the bare third -- so the bound is 20 %, not a quarter.)

References.  Every oracle-side sum over a catchment is math.fsum
(harness.catchment_fsum), so the summation error is the engine's alone.
  vol_SM, vol_IM   the numpy oracle's per-cell integrals; fp32 forms within
                   1e-5, the fp64 engine within 1e-12, of the column's largest
                   catchment (SURVEY 8(d) floored form).
  vol_P, PR, PS    fp32 forms: the exact emulation of the engine's own order
                   (harness.fp32_forcing_sums: per cell and launch the steps
                   added in np.float32, then fp64 times da dt), 1e-13 relative:
                   what remains is the fp64 reassociation of a few dozen
                   additions of non-negative terms.  fp64 engine: the oracle's
                   fp64 per-cell sums, 1e-12 relative.
  P_max            exact; 0 for a catchment without cells.

Catchment maps, on 37 x 100 cells (15 chunks, a padded tail) unless noted:
scatter[n] = (cell * 37) % n (64 distinct ids in every wave; 341 / 342 straddle
64 KiB of LDS bins per workgroup, 512 is tfg_create's limit), runs (edges off
the 64- and 256-cell boundaries), holes (scatter[512] on 5 x 100 cells: most
ids own no cell), tail (one id for the last 3 cells: a bin fed only from the
ragged last wave).

Measured on an MI355X (TFG_REPORT_DIR/diagnostics_*.json), the largest error
over every map a form runs (MEASURED below holds the same figures):
  form          vol_P / PR / PS vs emulation    vol_SM     vol_IM    (vs oracle)
  fp32          2.2e-16 / 3.3e-16 / 2.3e-16     1.0e-7     1.2e-7
  fp32_flux64   2.2e-16 / 2.2e-16 / 2.2e-16     3.6e-8     6.1e-8
  fp32_nansafe  2.2e-16 / 2.2e-16 / 2.2e-16     5.3e-8     8.2e-8
  fp32_qc       2.2e-16 / 2.2e-16 / 2.2e-16     5.0e-8     6.9e-8
  fp64          4.1e-16 / 3.2e-16 / 3.2e-16     4.4e-16    3.3e-16   (all vs the oracle)
P_max matched exactly everywhere.  No figure is within a factor of two of its
bound (1e-13 and 1e-5 for the fp32 forms, 1e-12 for fp64): the nearest is the
fp32 ice-melt integral, 80 times below.  The fp64 launch partitions agree to
3.7e-16; whole grid against its halves (test 4) 4.3e-16, and its forcing sums
against the host mirror 2.6e-16 (fp32) and 1.9e-16 (fp64).  The one-cell
kernels against the grid's rows: k_cell and k_cell_many 4.9e-16, k_cell_run
3.7e-16 (not bit for bit, and within 1e-12 as found); the grid's rows against
the reference fixture 5.4e-15 (vol_SM), P_max exact.  Launches with
n_catch >= 342 (more than 64 KiB of dynamic LDS) run as they are.
"""

import contextlib
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import tfg_oracle as O
from tests.harness import (BASE_CFG, bare_ice_inputs, catchment_fsum, fp32_forcing_sums, gpu_run_fields, load_golden,
                           make_engine, melt_out_flips)

pytestmark = pytest.mark.gpu

# Measured on an MI355X, the largest error of each kind over every map a form
# runs (test_oracle_parity; bounds: 1e-5 / 1e-13 for the fp32 forms, 1e-12 for fp64):
MEASURED = {
    "fp32": {"vol_P": 2.2e-16, "vol_PR": 3.3e-16, "vol_PS": 2.3e-16, "vol_SM": 1.0e-7, "vol_IM": 1.2e-7},
    "fp32_flux64": {"vol_P": 2.2e-16, "vol_PR": 2.2e-16, "vol_PS": 2.2e-16, "vol_SM": 3.6e-8, "vol_IM": 6.1e-8},
    "fp32_nansafe": {"vol_P": 2.2e-16, "vol_PR": 2.2e-16, "vol_PS": 2.2e-16, "vol_SM": 5.3e-8, "vol_IM": 8.2e-8},
    "fp32_qc": {"vol_P": 2.2e-16, "vol_PR": 2.2e-16, "vol_PS": 2.2e-16, "vol_SM": 5.0e-8, "vol_IM": 6.9e-8},
    "fp64": {"vol_P": 4.1e-16, "vol_PR": 3.2e-16, "vol_PS": 3.2e-16, "vol_SM": 4.4e-16, "vol_IM": 3.3e-16},
}

NY, NX, SEED = 37, 100, 4
NSTEPS, FUSE, NFRAMES = 20, 8, 24
DA_DT = BASE_CFG["da"] * 1e6 * BASE_CFG["dt"]
COLS = ("vol_P", "vol_PR", "vol_PS", "vol_SM", "vol_IM", "P_max")

FORMS = {
    "fp32": {},
    "fp32_flux64": {"flux": "fp64"},
    "fp32_nansafe": {"nan_safe": True},
    "fp32_qc": {"qc": True},
    "fp64": {"engine": "float64"},
}
RUN_LENGTHS = (1, 63, 65, 257, 255, 1, 511, 64)
REPORT: dict = {}


def _report(name, obj):
    """Measurements a test makes, written as JSON to $TFG_REPORT_DIR when set."""
    import json
    import os

    d = os.environ.get("TFG_REPORT_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, f"{name}.json"), "w") as f:
            json.dump(obj, f, indent=1, sort_keys=True)


def _scatter(cells, n_catch):
    return ((np.asarray(cells, dtype=np.int64) * 37) % n_catch).astype(np.int32)


def _runs(n):
    lengths = list(RUN_LENGTHS) + [n - sum(RUN_LENGTHS)]
    return np.repeat(np.arange(len(lengths)), lengths).astype(np.int32)


def catch_map(name):
    """(ny, nx, catchment id per cell, n_catch) of a named map."""
    ny, nx = (5, NX) if name == "holes" else (NY, NX)
    n = ny * nx
    if name.startswith("scatter"):
        nc = int(name[len("scatter"):])
        return ny, nx, _scatter(np.arange(n), nc), nc
    if name == "holes":
        return ny, nx, _scatter(np.arange(n), 512), 512
    if name == "runs":
        cid = _runs(n)
        return ny, nx, cid, int(cid.max()) + 1
    if name == "tail":
        cid = np.zeros(n, dtype=np.int32)
        cid[-3:] = 1
        return ny, nx, cid, 2
    raise KeyError(name)


def _qc_field(n):
    """A fixed, fp32-exact lateral conduction flux [W m-2], -4.5 .. 4.5."""
    return (((np.arange(n) % 7) - 3) * 1.5).astype(np.float32).astype(np.float64)


def _frozen(a):
    a = np.asarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _oracle(ny, nx, seed, nsteps, qc=False, nan=None):
    """One numpy-oracle run on the bare-ice inputs, shared (read-only) by the
    tests: the inputs, the per-step forcing, h_swe at every step boundary and
    the per-cell integrals.  nan = (step, cell): P is NaN there."""
    static, frames = bare_ice_inputs(seed, ny, nx, NFRAMES)
    n = ny * nx
    if nan is not None:
        assert nsteps <= NFRAMES  # one frame per step: the NaN is read once
        frames["P"][nan[0], nan[1]] = np.nan
    idx = np.arange(nsteps) % NFRAMES
    m = O.OracleGrid(BASE_CFG, **static)
    if qc:
        m.Qc = _qc_field(n)
    jd, _, _, tsn = O.oracle_clock(BASE_CFG["start_time"], BASE_CFG["dt"], nsteps, BASE_CFG["lon"])
    h_swe = [m.h_swe.copy()]
    cell_p = np.zeros((3, n))
    t_rs = np.float64(BASE_CFG["T_rain_snow"])
    with np.errstate(invalid="ignore"):
        for k in range(nsteps):
            P, T = frames["P"][idx[k]], frames["T_air"][idx[k]]
            m.step(P, T, frames["Hum_sp"][idx[k]], frames["P_air"][idx[k]], frames["uz"][idx[k]], jd[k], tsn[k])
            h_swe.append(np.array(m.h_swe, copy=True))
            cell_p[0] += P * m.da_m2 * m.dt  # the oracle's own terms (:567, :585-623), per cell
            cell_p[1] += (P * (T > t_rs)) * m.da_m2 * m.dt
            cell_p[2] += (P * (T <= t_rs)) * m.da_m2 * m.dt
    return SimpleNamespace(
        ny=ny, nx=nx, n=n, nsteps=nsteps, static={k: _frozen(v) for k, v in static.items()},
        frames={k: _frozen(v) for k, v in frames.items()}, P=_frozen(frames["P"][idx]), T=_frozen(frames["T_air"][idx]),
        h_swe=_frozen(np.stack(h_swe)), cell_P=_frozen(cell_p),
        cell_SM=_frozen(np.broadcast_to(m.cell_vol_SM, (n,)).copy()),
        cell_IM=_frozen(np.broadcast_to(m.cell_vol_IM, (n,)).copy()), qc=_frozen(_qc_field(n)) if qc else None)


def check_preconditions(orc):
    """What makes the melt integrals well conditioned, on the oracle alone."""
    zero = orc.h_swe == 0
    assert (zero == zero[0]).all(), "a cell's h_swe moved between zero and non-zero: the ice-melt gate is in play"
    share_im, share_sm = float((orc.cell_IM > 0).mean()), float((orc.cell_SM > 0).mean())
    assert share_im >= 0.20, share_im
    assert share_sm >= 0.25, share_sm
    return share_im, share_sm


def launches_of(chunks, fuse):
    """Steps per launch of run() calls of `chunks` steps each."""
    out = []
    for c in chunks:
        out += [fuse] * (c // fuse) + ([c % fuse] if c % fuse else [])
    return out


def catchment_pmax(cid, P, n_catch):
    """[n_catch] largest P [nsteps][ncell] of each catchment; 0 without cells (NaN propagates)."""
    out = np.zeros(n_catch)
    np.maximum.at(out, cid, np.max(P, axis=0))
    return out


def expected_diag(orc, cid, n_catch, fp32, launches):
    """[n_catch][6] reference diagnostics of an oracle run (module docstring)."""
    want = np.zeros((n_catch, 6))
    if fp32:
        assert sum(launches) == orc.nsteps
        s = fp32_forcing_sums(orc.P, orc.T, BASE_CFG["T_rain_snow"], launches) * DA_DT
        for col in range(3):
            want[:, col] = catchment_fsum(cid, s[:, col, :], n_catch)
    else:
        for col in range(3):
            want[:, col] = catchment_fsum(cid, orc.cell_P[col], n_catch)
    want[:, 3] = catchment_fsum(cid, orc.cell_SM, n_catch)
    want[:, 4] = catchment_fsum(cid, orc.cell_IM, n_catch)
    want[:, 5] = catchment_pmax(cid, orc.P, n_catch)
    return want


def rel_err(got, want):
    """Largest elementwise relative error (absolute where want == 0)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(want != 0, np.abs(got - want) / np.abs(want), np.abs(got - want))
    return float(np.max(r)) if r.size else 0.0


def floored_err(got, want):
    """Largest |got - want| over the column's largest |want| (floored)."""
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))


@contextlib.contextmanager
def engine_on(orc, form, cid, n_catch, fuse, split=None):
    """An initialised engine holding an oracle run's inputs, in a kernel form."""
    opt = FORMS[form]
    e = make_engine(BASE_CFG, orc.ny, orc.nx, opt.get("engine", "float32"), n_frames=NFRAMES, hist_depth=1,
                    n_catch=n_catch, fuse_steps=fuse, flux=opt.get("flux", "fp32"), split=split)
    try:
        for k in ("elev", "slope", "aspect"):
            e.set_field(k, orc.static[k])
        for k in ("h_snow", "h_ice", "h_swe", "h_iwe"):
            e.set_field(k, orc.static["h0_" + k[2:]])
        if cid is not None:
            e.set_field("catch_id", cid)
        e.init_state()
        for f in range(NFRAMES):
            for name in ("P", "T_air", "Hum_sp", "P_air", "uz"):
                e.set_field(name, orc.frames[name][f], index=f)
        if opt.get("nan_safe"):
            e.set_step_form(True)
        if opt.get("qc"):
            e.set_field("Qc", orc.qc)
        yield e
    finally:
        e.close()


def run_diag(orc, form, cid, n_catch, fuse, chunks):
    with engine_on(orc, form, cid, n_catch, fuse) as e:
        for c in chunks:
            e.run(c)  # step k reads frame k % 24
        e.sync()
        return e.diagnostics()


# ------------------------------------------------------------------ 1. oracle parity, per catchment and form
ALL_FORM_MAPS = ("scatter64", "scatter512", "runs")
OTHER_MAPS = ("scatter341", "scatter342", "holes", "tail")
PARITY_CASES = [(f, m) for f in FORMS for m in ALL_FORM_MAPS] + [(f, m) for f in ("fp32", "fp64") for m in OTHER_MAPS]


@pytest.mark.parametrize("form,map_name", PARITY_CASES)
def test_oracle_parity(form, map_name):
    """All six columns of every catchment against the references of the module
    docstring: 20 steps in launches of 8, 8 and 4."""
    ny, nx, cid, nc = catch_map(map_name)
    fp32 = form != "fp64"
    orc = _oracle(ny, nx, SEED, NSTEPS, qc=form == "fp32_qc")
    shares = check_preconditions(orc)
    want = expected_diag(orc, cid, nc, fp32, launches_of([NSTEPS], FUSE))
    assert want[:, 3].max() > 0 and want[:, 4].max() > 0
    got = run_diag(orc, form, cid, nc, FUSE, [NSTEPS])
    err = {COLS[c]: rel_err(got[:, c], want[:, c]) for c in (0, 1, 2)}
    err.update({COLS[c]: floored_err(got[:, c], want[:, c]) for c in (3, 4)})
    err["P_max_mismatches"] = int((got[:, 5] != want[:, 5]).sum())
    err["share_IM"], err["share_SM"] = shares
    REPORT.setdefault(form, {})[map_name] = err
    _report("diagnostics_parity", REPORT)
    print(f"diagnostics parity {form} {map_name}: {err}")
    tol_p, tol_m = (1e-13, 1e-5) if fp32 else (1e-12, 1e-12)
    for c in (0, 1, 2):
        assert err[COLS[c]] <= tol_p, (COLS[c], err)
    for c in (3, 4):
        assert err[COLS[c]] <= tol_m, (COLS[c], err)
    assert np.array_equal(got[:, 5], want[:, 5]), "P_max"
    empty = np.bincount(cid, minlength=nc) == 0
    assert np.all(got[empty] == 0.0)  # a catchment without cells reads 0 in every column
    if map_name == "holes":
        assert empty.sum() >= 12


# ------------------------------------------------------------------ 2. the launch partition
def test_fp64_launch_partition_moves_only_the_last_bits():
    """The fp64 engine sums a cell's terms unscaled over a launch and scales
    once per launch, so its diagnostics move with the launch partition -- by
    fp64 rounding only: 100 steps as one launch per step, as launches of 24,
    and as calls of 1, 30 and 69 steps in launches of 7, agree to 1e-12."""
    _, _, cid, nc = catch_map("scatter64")
    orc = _oracle(NY, NX, SEED, NSTEPS)
    a = run_diag(orc, "fp64", cid, nc, 1, [100])
    b = run_diag(orc, "fp64", cid, nc, 24, [100])
    c = run_diag(orc, "fp64", cid, nc, 7, [1, 30, 69])
    assert np.all(a[:, :5] > 0)
    err = {"fuse24_vs_fuse1": rel_err(b[:, :5], a[:, :5]), "fuse7_chunks_vs_fuse1": rel_err(c[:, :5], a[:, :5])}
    _report("diagnostics_partition_fp64", err)
    print(f"diagnostics fp64 launch partition: {err}")
    assert max(err.values()) <= 1e-12, err
    assert np.array_equal(a[:, 5], b[:, 5]) and np.array_equal(a[:, 5], c[:, 5])


@pytest.mark.parametrize("fuse", [1, 24])
def test_fp32_launch_partition_is_pinned_to_its_own_value(fuse):
    """The fp32 engine sums each cell's precipitation in fp32 over one launch,
    so each partition has its own exact expected value: 40 steps as one launch
    per step and as launches of 24 and 16, each against its own emulation."""
    _, _, cid, nc = catch_map("scatter64")
    nsteps = 40
    orc = _oracle(NY, NX, SEED, nsteps)
    want = expected_diag(orc, cid, nc, True, launches_of([nsteps], fuse))
    other = expected_diag(orc, cid, nc, True, launches_of([nsteps], 25 - fuse))
    assert not np.array_equal(want[:, :3], other[:, :3])  # the partitions' expected values do differ
    got = run_diag(orc, "fp32", cid, nc, fuse, [nsteps])
    err = {COLS[c]: rel_err(got[:, c], want[:, c]) for c in (0, 1, 2)}
    REPORT.setdefault("partition_fp32", {})[f"fuse{fuse}"] = err
    _report("diagnostics_parity", REPORT)
    print(f"diagnostics fp32 launch partition fuse={fuse}: {err}")
    assert max(err.values()) <= 1e-13, err
    assert np.array_equal(got[:, 5], want[:, 5])


# ------------------------------------------------------------------ 3. the one-cell kernels
def test_one_cell_kernels_against_the_grid_and_the_reference():
    """grid64 fixture, fp64, 100 steps.  The 8 x 8 grid with one catchment per
    cell: every row is one cell's integrals, held to the reference fixture's
    per-cell vol_* at 1e-10 (cells without a melt-out flip).  For cells 0, 17,
    42 and 63 a one-cell handle stepped by run() (k_cell_run), by update_io()
    (k_cell) and by update_many over the four handles (k_cell_many) gives the
    grid's row to 1e-12: those kernels scale every step's terms, the grid
    kernel once per launch.  Cell 42's handles have three catchments and the
    cell in the last: the other two rows stay 0."""
    from topoflow_glacier.bmi import bmi_topoflow_glacier as B
    from topoflow_glacier.engine import update_many

    g = load_golden("grid64")
    nsteps = 100
    assert g["nsteps"] >= nsteps
    outs, _, grid = gpu_run_fields(g["cfg"], g["static"], g["forcing"], 8, 8, "float64", nsteps, fuse_steps=24,
                                   catch_id=np.arange(64, dtype=np.int32), n_catch=64)
    ref = np.stack([g["internal"][v][nsteps - 1] for v in COLS], axis=1)  # [64][6]
    flip, genuine = melt_out_flips(outs, {v: g["outputs"][v][:nsteps] for v in outs}, 1e-10)
    assert not genuine, genuine[:5]
    keep = flip < 0
    assert keep.sum() >= 32
    assert all((ref[keep, c] > 0).any() for c in range(6))  # no column is compared on zeros alone
    err = {"grid_vs_fixture": {COLS[c]: rel_err(grid[keep, c], ref[keep, c]) for c in range(6)}}

    cells = (0, 17, 42, 63)
    order = ("P_air", "Hum_sp", "P", "T_air", "uz")  # update_io / update_many input order

    def layout(c):  # (n_catch, catchment id, row of the cell's integrals)
        return (3, np.array([2], dtype=np.int32), 2) if c == 42 else (1, None, 0)

    def one_cell_engine(c):
        nc, cid, _ = layout(c)
        e = make_engine(g["cfg"], 1, 1, "float64", n_frames=1, hist_depth=1, n_catch=nc)
        for k in ("elev", "slope", "aspect"):
            e.set_field(k, g["static"][k][c:c + 1])
        for k in ("h_snow", "h_ice", "h_swe", "h_iwe"):
            e.set_field(k, g["static"]["h0_" + k[2:]][c:c + 1])
        if cid is not None:
            e.set_field("catch_id", cid)
        e.init_state()
        return e

    def inputs(c, k):
        return np.array([[g["forcing"][v][k, c]] for v in order], dtype=np.float64)

    got = {}
    for c in cells:
        nc, cid, _ = layout(c)
        static = {k: v[c:c + 1] for k, v in g["static"].items()}
        forcing = {k: v[:, c:c + 1] for k, v in g["forcing"].items()}
        got["k_cell_run", c] = gpu_run_fields(g["cfg"], static, forcing, 1, 1, "float64", nsteps, fuse_steps=24,
                                              catch_id=cid, n_catch=nc)[2]
        e = one_cell_engine(c)
        try:
            out = np.empty((8, 1))
            for k in range(nsteps):
                e.update_io(inputs(c, k), out)
            got["k_cell", c] = e.diagnostics()
        finally:
            e.close()
    engines = [one_cell_engine(c) for c in cells]
    try:
        for e in engines:
            e.set_stream(B._shared_stream(0))
        outs_many = [np.empty((8, 1)) for _ in cells]
        for k in range(nsteps):
            update_many(engines, [inputs(c, k) for c in cells], outs_many)
        for c, e in zip(cells, engines):
            got["k_cell_many", c] = e.diagnostics()
    finally:
        for e in engines:
            e.close()
    for (kernel, c), d in got.items():
        nc, _, row = layout(c)
        assert d.shape == (nc, 6)
        err.setdefault(kernel, {})[str(c)] = rel_err(d[row, :5], grid[c, :5])
    _report("diagnostics_one_cell", err)
    print(f"diagnostics one-cell kernels: {err}")
    for c in range(6):
        assert err["grid_vs_fixture"][COLS[c]] <= 1e-10, err["grid_vs_fixture"]
    for (kernel, c), d in got.items():
        nc, _, row = layout(c)
        assert err[kernel][str(c)] <= 1e-12, (kernel, c, d[row], grid[c])
        assert d[row, 5] == grid[c, 5], (kernel, c)
        assert np.all(np.delete(d, row, axis=0) == 0.0), (kernel, c, d)


# ------------------------------------------------------------------ 4. several chunks per workgroup, split launches
BIG_NY, BIG_NX, BIG_STEPS, BIG_SEED, BIG_NC = 1152, 2048, 12, 5, 512


@functools.lru_cache(maxsize=None)
def _big_mirror():
    """P and T_air [12][ncell] fp32 of the large grid from the host mirror of
    the device generator (synthetic_cells), in 16 blocks of cells on 8 threads
    (numpy releases the GIL): 1.4 s where the whole grid at once takes 11 s."""
    from concurrent.futures import ThreadPoolExecutor

    from topoflow_glacier.synthetic import diurnal_table, synthetic_cells

    d = diurnal_table(BIG_STEPS)
    blocks = np.array_split(np.arange(BIG_NY * BIG_NX), 16)
    with ThreadPoolExecutor(8) as pool:
        parts = list(pool.map(lambda c: {k: v for k, v in synthetic_cells(BIG_SEED, c, d).items() if k in ("P", "T_air")},
                              blocks))
    return tuple(_frozen(np.concatenate([p[k] for p in parts], axis=1)) for k in ("P", "T_air"))


@functools.lru_cache(maxsize=None)
def _big_expected(fp32):
    """[512][6] per-catchment references of the large grid (columns 0-2 and 5):
    the fp32 engine's exact forcing sums (launches of 8 and 4) or the fp64
    per-cell sums, and P_max."""
    P, T = _big_mirror()
    cid = _scatter(np.arange(BIG_NY * BIG_NX), BIG_NC)
    if fp32:
        s = fp32_forcing_sums(P, T, BASE_CFG["T_rain_snow"], launches_of([BIG_STEPS], FUSE)) * DA_DT
    else:
        rain = T.astype(np.float64) > float(BASE_CFG["T_rain_snow"])
        s = np.zeros((1, 3, cid.size))
        for k in range(BIG_STEPS):
            p = P[k].astype(np.float64) * DA_DT  # the oracle's per-step term P da dt, added in step order
            s[0, 0] += p
            s[0, 1] += np.where(rain[k], p, 0.0)
            s[0, 2] += np.where(rain[k], 0.0, p)
    want = np.zeros((BIG_NC, 6))
    for col in range(3):
        want[:, col] = catchment_fsum(cid, s[:, col, :], BIG_NC)
    want[:, 5] = catchment_pmax(cid, P, BIG_NC)
    return _frozen(want)


def _big_run(engine, ny, row0, split):
    from topoflow_glacier.synthetic import diurnal_table

    e = make_engine(BASE_CFG, ny, BIG_NX, engine, n_frames=BIG_STEPS, hist_depth=1, n_catch=BIG_NC, fuse_steps=FUSE,
                    row0=row0, split=split)
    try:
        e.fill_synthetic(BIG_SEED, diurnal_table(BIG_STEPS), nx_global=BIG_NX)
        e.set_field("catch_id", _scatter(np.arange(ny * BIG_NX) + row0 * BIG_NX, BIG_NC))
        was_split = e.is_split()
        e.run(BIG_STEPS)
        e.sync()
        dt = np.float32 if engine == "float32" else np.float64
        return SimpleNamespace(split=was_split, M_total=e.get_field("M_total", dtype=dt), h_swe=e.get_field("h_swe"),
                               diag=e.diagnostics())
    finally:
        e.close()


@pytest.mark.parametrize("engine", ["float32", "float64"])
def test_many_chunks_per_workgroup_and_the_split_launch(engine):
    """1152 x 2048 cells with 512 scattered catchments have more 256-cell
    chunks than the 8192 slab rows 512 catchments leave, so workgroups run two
    trips, and a split launch (fp32 engine) takes the branch where its parts
    share the rows, half each.  Its two 576-row halves, run as shards, have one
    chunk per workgroup.  Unsplit, split and auto give the same outputs bit
    for bit; each run's sums equal the halves' sum to 1e-12 per catchment (the
    per-cell contributions are bit-identical, only the fp64 order differs) and
    its P_max their maximum; the forcing sums meet the references of the
    module docstring, from the host mirror of the device generator.  12 steps
    in launches of 8 and 4."""
    fp32 = engine == "float32"
    halves = [_big_run(engine, BIG_NY // 2, 0, "off"), _big_run(engine, BIG_NY // 2, BIG_NY // 2, "off")]
    assert not halves[0].split and not halves[1].split
    hsum = halves[0].diag[:, :5] + halves[1].diag[:, :5]
    hmax = np.maximum(halves[0].diag[:, 5], halves[1].diag[:, 5])
    assert np.all(hsum[:, :4] > 0)
    want = _big_expected(fp32)
    tol = 1e-13 if fp32 else 1e-12
    err = {}
    wholes = {s: _big_run(engine, BIG_NY, 0, s) for s in (("off", "on", "auto") if fp32 else ("off",))}
    for s, w in wholes.items():
        err[s] = {"vs_halves": rel_err(w.diag[:, :5], hsum), "vs_forcing_reference": rel_err(w.diag[:, :3], want[:, :3])}
    err["halves"] = {"vs_forcing_reference": rel_err(hsum[:, :3], want[:, :3])}
    _report(f"diagnostics_many_chunks_{engine}", err)
    print(f"diagnostics many chunks per workgroup {engine}: {err}")
    if fp32:
        assert not wholes["off"].split and wholes["on"].split and wholes["auto"].split
    for s, w in wholes.items():
        for v in ("M_total", "h_swe"):
            assert np.array_equal(getattr(w, v), np.concatenate([getattr(h, v) for h in halves])), (s, v)
        assert err[s]["vs_halves"] <= 1e-12, (s, err)
        assert np.array_equal(w.diag[:, 5], hmax), s
        assert err[s]["vs_forcing_reference"] <= tol, (s, err)
        assert np.array_equal(w.diag[:, 5], want[:, 5]), s
    assert err["halves"]["vs_forcing_reference"] <= tol, err


# ------------------------------------------------------------------ 5. reset
@pytest.mark.parametrize("form", ["fp32", "fp64"])
def test_reset_diagnostics(form):
    """tfg_reset_diag: after 24 steps every entry reads 0; 16 more steps then
    give what an identical handle that ran all 40 steps accumulated after its
    reading at 24 (sums within 1e-12 of the 40-step value), and P_max is the
    maximum of steps 24-39 alone -- smaller, in some catchment, than that of
    the first 24 steps, so a maximum that survived the reset shows."""
    nc = 5
    cid = _scatter(np.arange(NY * NX), nc)
    # the inputs (engine is compared with engine here); seed 10: the largest P of three of
    # the five catchments falls in frames 16-23, which steps 24-39 (frames 0-15) do not read
    orc = _oracle(NY, NX, 10, 40)
    first, later = catchment_pmax(cid, orc.P[:24], nc), catchment_pmax(cid, orc.P[24:], nc)
    assert (first > later).any() and (later > 0).all()
    with engine_on(orc, form, cid, nc, 24) as e:
        e.run(24)
        d24 = e.diagnostics()
        e.reset_diagnostics()
        zero = e.diagnostics()
        e.run(16)
        after = e.diagnostics()
    with engine_on(orc, form, cid, nc, 24) as e:
        e.run(24)
        r24 = e.diagnostics()
        e.run(16)
        r40 = e.diagnostics()
    assert np.array_equal(d24, r24) and np.all(d24[:, :4] > 0) and np.array_equal(d24[:, 5], first)
    assert np.all(zero == 0.0), zero
    assert np.all(np.abs(after[:, :5] - (r40[:, :5] - r24[:, :5])) <= 1e-12 * np.abs(r40[:, :5])), (after, r40 - r24)
    assert np.all(after[:, :3] > 0)
    assert np.array_equal(after[:, 5], later), (after[:, 5], later, first)


# ------------------------------------------------------------------ 6. NaN forcing stays in its catchment
@pytest.mark.parametrize("form", ["fp32", "fp64"])
def test_nan_forcing_stays_in_its_catchment(form):
    """P = NaN in one cell at one step: that catchment's vol_P and P_max are
    NaN and its other columns are NaN exactly where the oracle's per-cell
    values, summed over the catchment, are; every other catchment's row equals
    the row of a run without the NaN, bit for bit."""
    _, _, cid, nc = catch_map("runs")
    step, cell = 5, 100
    hit = int(cid[cell])
    clean, dirty = _oracle(NY, NX, SEED, NSTEPS), _oracle(NY, NX, SEED, NSTEPS, nan=(step, cell))
    assert cell % 3 != 0 and 0 < hit < nc - 1  # a snow-covered cell, in a catchment with neighbours on both sides
    per_cell = np.stack([dirty.cell_P[0], dirty.cell_P[1], dirty.cell_P[2], dirty.cell_SM, dirty.cell_IM,
                         np.max(dirty.P, axis=0)])
    want_nan = np.array([[np.isnan(per_cell[c][cid == k]).any() for c in range(6)] for k in range(nc)])
    assert want_nan[hit, 0] and want_nan[hit, 5] and not np.delete(want_nan, hit, axis=0).any()
    d_clean = run_diag(clean, form, cid, nc, FUSE, [NSTEPS])
    d_dirty = run_diag(dirty, form, cid, nc, FUSE, [NSTEPS])
    assert np.isfinite(d_clean).all()
    np.testing.assert_array_equal(np.isnan(d_dirty), want_nan)
    others = np.arange(nc) != hit
    assert np.array_equal(d_dirty[others], d_clean[others])


# ------------------------------------------------------------------ 7. a rejected catchment map
def test_a_rejected_catchment_map_changes_nothing():
    """tfg_set_field validates a catchment map before any of it reaches the
    handle (the ids index the kernels' LDS bins): a map with an id of n_catch
    or -1, from the host or from a device tensor, raises and leaves the map
    set before in place; a run afterwards equals that of a handle that never
    saw the bad maps."""
    import torch

    from topoflow_glacier._native import NativeError

    ny, nx, nc = 5, NX, 4
    orc = _oracle(ny, nx, SEED, NSTEPS)
    good = _scatter(np.arange(ny * nx), nc)

    def ten_steps(e):
        e.run(10)
        e.sync()
        return e.diagnostics(), e.get_field("h_swe"), e.get_field("M_total", dtype=np.float32)

    with engine_on(orc, "fp32", good, nc, FUSE) as e:
        for bad_id in (nc, -1):
            bad = good.copy()
            bad[ny * nx // 2] = bad_id
            for src in (bad, torch.tensor(bad, dtype=torch.int32, device="cuda:0")):
                with pytest.raises(NativeError, match="catchment id out of"):
                    e.set_field("catch_id", src)
                assert np.array_equal(e.get_field("catch_id"), good)
        got = ten_steps(e)
    with engine_on(orc, "fp32", good, nc, FUSE) as e:
        want = ten_steps(e)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    # and a handle that has no map yet gets none from a rejected one
    with engine_on(orc, "fp32", None, nc, FUSE) as e:
        with pytest.raises(NativeError, match="catchment id out of"):
            e.set_field("catch_id", np.full(ny * nx, nc, dtype=np.int32))
        with pytest.raises(NativeError, match="no catchment-id raster set"):
            e.get_field("catch_id")
