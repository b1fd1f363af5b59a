"""Forcing frames produced on the device from a per-catchment table
(k_forcing_expand; tfg_set_catchment_forcing), through
GlacierEngine.set_catchment_forcing and
hydrograph.forced_catchment_hydrographs: the frames against the numpy
restatement of the rule (tests/downscale_ref.py) under both vapour-pressure
formulas (the humidity cap's e_sat is the model's configured one), the
precipitation clamp,
batches and the frame range, several tiles per workgroup, split launches,
missing data, the humidity cap end to end, the hydrograph against the numpy
oracle, the rejected arguments, and the pinned staging ring it shares with
tfg_set_inputs.

Inputs.  tests/harness.py:bare_ice_inputs(4, 37, 100, 24): 3700 cells, 14 whole
chunks and a ragged one.  Catchment map `divide`: id = 3 min(cell // 925, 3) +
cell % 3, 12 catchments, the dry bare-ice cells (cell % 3 == 0) in catchments of
their own; `scatter64`: 64 ids in every wave; and no raster.  The table is the
per-catchment mean of the frames, z_ref the per-catchment mean elevation,
Downscale(lapse_T=-0.0065, grad_P=2e-4, pressure=1, rh_max=1.0).

Asserted on the restatement and the numpy oracle alone, before any GPU value
is read (check_forcing_preconditions): dz spans +-790 m and no precipitation
factor is clamped; 42 % of the cell-frames exceed RH 1 before the cap; over 20
steps no cell's h_swe moves between zero and non-zero; cell_vol_IM > 0 in 33 %
of the cells and cell_vol_SM > 0 in 99 %; 196 of the 240 (step, catchment)
runoff entries are positive; the oracle's RH peaks at 1 + 4e-16.

Bounds.  Plain gather: bit-equal to R(table[f][v][cid]).  Downscaled, with s_v
the variable's largest |ref|: fp64 engine |gpu - ref| <= 1e-13 max(|ref|, s_v),
the bar the fp64 engine's functions are sized for; fp32
engine <= 2^-23 max(|ref|, s_v), one rounding to fp32 (2^-24) doubled, the fp64
arithmetic's own error being far below it.  Hydrograph: 1e-5 of the largest
entry for the fp32 forms, 1e-12 for fp64 (the catchment series' bounds).

Measured on an MI355X (TFG_REPORT_DIR/catchment_forcing.json; MEASURED below
holds the same figures), the largest error of each kind:
  frames against the restatement, three maps, host and device tables
      fp32 5.8e-8 (uz, a pure conversion: one rounding to fp32 is 6.0e-8),
      fp64 9.4e-16 (Hum_sp; P_air 4.5e-16; T_air, P and uz exact)
  the same with SATTERLUND: true (`divide`; the cap binds in 42.6 % of the
      cell-frames and parts from Brutsaert's by up to 6.8e-3 relative there)
      fp32 5.7e-8, fp64 8.4e-16 (both Hum_sp)
  with the clamp (grad_P = 2e-3)                       fp32 5.6e-8, fp64 9.4e-16
  1152 x 2048, 512 ids, against the restatement         fp32 5.7e-8
  hydrograph against the oracle (floored)               fp32 1.6e-7, fp32_flux64
      1.1e-7, fp64 5.4e-16
  the fp64 engine's RH after one step: at most 1.0 with rh_max = 1, 1.66 with 0
The fp32 frames sit at their rounding (half the bound); every other figure is
a factor of 60 or more inside its bound.
"""

import contextlib
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from tests import downscale_ref as D
from tests.harness import BASE_CFG, bare_ice_inputs, catchment_fsum, make_engine, oracle_run
from tests.test_gpu_diagnostics import FORMS, _report, _scatter, check_preconditions, floored_err

pytestmark = pytest.mark.gpu

# Measured on an MI355X: the largest error of each kind, as a fraction of the
# variable's largest |ref| (bounds: 1e-13 fp64, 2^-23 = 1.19e-7 fp32; hydrograph
# 1e-5 / 1e-12 of the largest entry).
MEASURED = {
    "frames": {"float32": 5.8e-8, "float64": 9.4e-16},
    "frames_satterlund": {"float32": 5.7e-8, "float64": 8.4e-16},  # Hum_sp, the capped plane; no plane is above it
    "clamp": {"float32": 5.6e-8, "float64": 9.4e-16},
    "many_tiles": {"float32": 5.7e-8},
    "hydrograph_floored": {"fp32": 1.6e-7, "fp32_flux64": 1.1e-7, "fp64": 5.4e-16},
    "rh_peak": {"rh_max=1": 1.0, "rh_max=0": 1.66},
}

NY, NX, SEED, NFRAMES, NSTEPS = 37, 100, 4, 24, 20
N = NY * NX
DS = dict(lapse_T=-0.0065, grad_P=2e-4, pressure=1, rh_max=1.0)
DA_M2 = BASE_CFG["da"] * 1e6
BOUND = {"float32": 2.0 ** -23, "float64": 1e-13}
NP = {"float32": np.float32, "float64": np.float64}
REPORT: dict = {}


def _note(kind, key, value):
    REPORT.setdefault(kind, {})[key] = value
    _report("catchment_forcing", REPORT)


def _frozen(a):
    a = np.asarray(a)
    a.setflags(write=False)
    return a


def _downscale(**kw):
    from topoflow_glacier.forcing import Downscale

    return Downscale(**kw)


@functools.lru_cache(maxsize=None)
def _inputs(map_name="divide"):
    """The bare-ice inputs with a catchment map, the table of per-catchment
    means of the frames and the mean elevations (read-only, shared)."""
    static, frames = bare_ice_inputs(SEED, NY, NX, NFRAMES)
    cell = np.arange(N)
    if map_name == "divide":
        cid, nc = (3 * np.minimum(cell // 925, 3) + cell % 3).astype(np.int32), 12
    elif map_name == "scatter64":
        cid, nc = _scatter(cell, 64), 64
    else:  # no raster: every cell in catchment 0 of three
        cid, nc = None, 3
    eff = np.zeros(N, dtype=np.int32) if cid is None else cid
    table = np.stack([D.catchment_means(eff, frames[k], nc) for k in D.ORDER], axis=1)
    z_ref = D.catchment_means(eff, static["elev"], nc)
    return SimpleNamespace(static={k: _frozen(v) for k, v in static.items()}, cid=None if cid is None else _frozen(cid),
                           eff=_frozen(eff), nc=nc, table=_frozen(table), z_ref=_frozen(z_ref))


@functools.lru_cache(maxsize=None)
def check_forcing_preconditions():
    """What the comparisons stand on, on the restatement and the numpy oracle
    alone (module docstring).  Returns the restated frames [24][5][n] and the
    oracle's M_total [20][n] on them."""
    inp = _inputs()
    fr, info = D.downscale(inp.table, inp.cid, inp.static["elev"], inp.z_ref, parts=True, **DS)
    assert 780.0 < info["dz"].max() < 800.0 and -800.0 < info["dz"].min() < -780.0
    assert not info["clamped"].any()
    assert 0.41 <= float((info["rh_before"] > 1.0).mean()) <= 0.44
    assert float(D.relative_humidity(fr, D.constants()).max()) <= 1.0 + 1e-12
    idx = np.arange(NSTEPS) % NFRAMES
    import tfg_oracle as O

    m = O.OracleGrid(BASE_CFG, **inp.static)
    jd, _, _, tsn = O.oracle_clock(BASE_CFG["start_time"], BASE_CFG["dt"], NSTEPS, BASE_CFG["lon"])
    h_swe, mtot, rh = [m.h_swe.copy()], [], []
    for k in range(NSTEPS):
        f = fr[idx[k]]
        r = m.step(f[D.I_P], f[D.I_T], f[D.I_Q], f[D.I_PA], f[D.I_UZ], jd[k], tsn[k])
        h_swe.append(np.array(m.h_swe, copy=True))
        mtot.append(np.array(r["M_total"], copy=True))
        rh.append(np.array(r["RH"], copy=True))
    orc = SimpleNamespace(h_swe=np.stack(h_swe), cell_IM=np.broadcast_to(m.cell_vol_IM, (N,)),
                          cell_SM=np.broadcast_to(m.cell_vol_SM, (N,)))
    share_im, share_sm = check_preconditions(orc)
    assert 0.30 <= share_im <= 0.36 and share_sm >= 0.98
    mtot = np.stack(mtot)
    runoff = np.stack([catchment_fsum(inp.cid, mtot[k], inp.nc) for k in range(NSTEPS)]) * DA_M2
    assert int((runoff > 0).sum()) == 196 and runoff.size == 240
    assert 1.0 - 1e-12 <= float(np.max(rh)) <= 1.0 + 1e-12  # the cap binds, and holds in the model's own RH
    # the same M_total through the harness's runner (the hydrograph's reference)
    out, _ = oracle_run(BASE_CFG, inp.static, {k: fr[idx, i, :] for i, k in enumerate(D.ORDER)}, NSTEPS)
    assert np.array_equal(out["M_total"], mtot)
    return _frozen(fr), _frozen(runoff)


@contextlib.contextmanager
def forcing_engine(inp, engine, n_frames=NFRAMES, hist_depth=8, fuse=8, flux="fp32", split=None, fill=None, cfg=BASE_CFG):
    """An initialised engine on the bare-ice rasters with the map's ids; the
    frames zero, or `fill` in every value."""
    e = make_engine(cfg, NY, NX, engine, n_frames=n_frames, hist_depth=hist_depth, n_catch=inp.nc, fuse_steps=fuse,
                    flux=flux, split=split)
    try:
        for k in ("elev", "slope", "aspect"):
            e.set_field(k, inp.static[k])
        for k in ("h_snow", "h_ice", "h_swe", "h_iwe"):
            e.set_field(k, inp.static["h0_" + k[2:]])
        if inp.cid is not None:
            e.set_field("catch_id", inp.cid)
        e.init_state()
        if fill is not None:
            for f in range(n_frames):
                e.set_inputs(np.full((5, N), fill + f), index=f)
        yield e
    finally:
        e.close()


def read_frames(e, frames):
    """[len(frames)][5][n] the frames' planes in tfg_set_inputs order, in the engine's type."""
    dt = NP[e.engine]
    return np.stack([np.stack([e.get_field(name, index=int(f), dtype=dt) for name in D.ORDER]) for f in frames])


def frame_err(got, ref):
    """Per variable, max |gpu - ref| / max(|ref|, s_v) with s_v the variable's largest |ref|."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = {}
    for v, name in enumerate(D.ORDER):
        s_v = np.abs(ref[:, v, :]).max()
        assert s_v > 0, name
        err[name] = float((np.abs(got[:, v, :] - ref[:, v, :]) / np.maximum(np.abs(ref[:, v, :]), s_v)).max())
    return err


def put(e, inp, table, frame0=0, ds=None, device=False, z_ref=None):
    """set_catchment_forcing of a host or device table (z_ref on the same side)."""
    z = (inp.z_ref if z_ref is None else z_ref) if ds is not None and ds.on else None
    if device:
        import torch

        table = torch.from_numpy(np.array(table, dtype=np.float64)).to(e.torch_device)
        z = None if z is None else torch.from_numpy(np.array(z, dtype=np.float64)).to(e.torch_device)
    e.set_catchment_forcing(table, frame0=frame0, z_ref=z, downscale=ds)


# ------------------------------------------------------------------ 1. frames against the restatement
@pytest.mark.parametrize("map_name", ["divide", "scatter64", "none"])
@pytest.mark.parametrize("engine", ["float32", "float64"])
def test_frames_equal_the_restatement(engine, map_name):
    """All 24 frames (three batches of eight) from host and device tables: the
    plain gather bit-equal to R(table[f][v][cid]), with a Downscale of zeros as
    with none; the downscaled frames within the engine's bound of the
    restatement on the elevation the engine holds."""
    check_forcing_preconditions()
    inp = _inputs(map_name)
    R = NP[engine]
    worst = {}
    with forcing_engine(inp, engine, fill=-777.0) as e:
        elev = e.get_field("elev", dtype=R).astype(np.float64)
        want_plain = inp.table[:, :, inp.eff].astype(R)
        want_ds, info = D.downscale(inp.table, inp.eff, elev, inp.z_ref, parts=True, **DS)
        assert float((info["rh_before"] > 1).mean()) > 0.3 and not info["clamped"].any()
        for device in (False, True):
            for ds in (None, _downscale(), _downscale(**DS)):
                put(e, inp, inp.table, ds=ds, device=device)
                got = read_frames(e, range(NFRAMES))
                assert got.dtype == R
                if ds is None or not ds.on:
                    assert np.array_equal(got, want_plain), (device, ds)
                else:
                    err = frame_err(got, want_ds)
                    print(f"catchment forcing vs restatement {engine} {map_name} device={device}: {err}")
                    for k, v in err.items():
                        worst[k] = max(worst.get(k, 0.0), v)
                    assert max(err.values()) <= BOUND[engine], err
                    assert not np.array_equal(got, want_plain)
        e.run(8)  # the frames as the last call left them feed a launch
        assert np.isfinite(e.get_field("M_total")).all()
    _note("frames", f"{engine}/{map_name}", worst)


SAT_CFG = dict(BASE_CFG, SATTERLUND=True)


@functools.lru_cache(maxsize=None)
def check_satterlund_cap_preconditions():
    """On the restatement alone: with SATTERLUND: true the humidity cap binds
    in 42.6 % of the `divide` map's cell-frames, and the capped Hum_sp differs
    from what Brutsaert's e_sat gives there by up to 6.8e-3 relative, by more
    than 1e-4 (800 times the fp32 bound) in 93 % of them: a kernel that capped
    with the other formula cannot pass.  Every other plane is the same."""
    inp = _inputs()
    sat, info = D.downscale(inp.table, inp.cid, inp.static["elev"], inp.z_ref, parts=True, cfg=SAT_CFG, **DS)
    bru = D.downscale(inp.table, inp.cid, inp.static["elev"], inp.z_ref, **DS)
    capped = info["rh_before"] > 1.0
    assert 0.41 <= float(capped.mean()) <= 0.44, float(capped.mean())
    assert not info["clamped"].any()
    rel = np.abs(sat[:, D.I_Q, :] - bru[:, D.I_Q, :]) / np.abs(bru[:, D.I_Q, :])
    assert float(rel[capped].max()) >= 5e-3, float(rel[capped].max())
    assert float((rel[capped] > 1e-4).mean()) >= 0.9
    assert all(np.array_equal(sat[:, v, :], bru[:, v, :]) for v in range(5) if v != D.I_Q)
    assert float(D.relative_humidity(sat, D.constants(SAT_CFG)).max()) <= 1.0 + 1e-12
    return True


@pytest.mark.parametrize("engine", ["float32", "float64"])
def test_satterlund_frames_equal_the_restatement(engine):
    """SATTERLUND: true, the `divide` map, host and device tables: the humidity
    cap of both device forcing paths takes forcing_e_sat's Satterlund branch.
    All 24 frames within the engine's bound of the restatement under the same
    configuration, and outside it of the Brutsaert restatement."""
    assert check_satterlund_cap_preconditions()
    inp = _inputs()
    R = NP[engine]
    worst = {}
    with forcing_engine(inp, engine, fill=-777.0, cfg=SAT_CFG) as e:
        elev = e.get_field("elev", dtype=R).astype(np.float64)
        want, info = D.downscale(inp.table, inp.eff, elev, inp.z_ref, parts=True, cfg=SAT_CFG, **DS)
        other = D.downscale(inp.table, inp.eff, elev, inp.z_ref, **DS)
        assert 0.41 <= float((info["rh_before"] > 1).mean()) <= 0.44 and not info["clamped"].any()
        assert frame_err(other, want)["Hum_sp"] > 1e-3  # the two restatements part by far more than the bound
        for device in (False, True):
            put(e, inp, inp.table, ds=_downscale(**DS), device=device)
            got = read_frames(e, range(NFRAMES))
            assert got.dtype == R
            err = frame_err(got, want)
            print(f"catchment forcing vs restatement, Satterlund, {engine} device={device}: {err}")
            for k, v in err.items():
                worst[k] = max(worst.get(k, 0.0), v)
            assert max(err.values()) <= BOUND[engine], err
            assert frame_err(got, other)["Hum_sp"] > 1e-3
            for f in range(NFRAMES):  # the next table lands on frames it must rewrite
                e.set_inputs(np.full((5, N), -777.0 + f), index=f)
        put(e, inp, inp.table, ds=_downscale(**DS))
        e.run(8)  # the frames feed a launch of the Satterlund step
        assert np.isfinite(e.get_field("M_total")).all()
    _note("frames_satterlund", engine, worst)


# ------------------------------------------------------------------ 2. the precipitation clamp
@pytest.mark.parametrize("engine", ["float32", "float64"])
def test_precipitation_clamps_to_zero_where_the_restatement_does(engine):
    """grad_P = 2e-3: between 1 % and 50 % of the cells clamp; P is exactly 0
    there and nowhere else but where the catchment is dry."""
    inp = _inputs()
    kw = dict(DS, grad_P=2e-3)
    R = NP[engine]
    with forcing_engine(inp, engine) as e:
        elev = e.get_field("elev", dtype=R).astype(np.float64)
        ref, info = D.downscale(inp.table, inp.eff, elev, inp.z_ref, parts=True, **kw)
        assert 0.01 < float(info["clamped"].mean()) < 0.5
        wet = inp.table[:, D.I_P, :][:, inp.eff] > 0
        assert (wet & ~info["clamped"]).any() and (wet & info["clamped"]).any()
        put(e, inp, inp.table, ds=_downscale(**kw))
        got = read_frames(e, range(NFRAMES))
    err = frame_err(got, ref)
    _note("clamp", engine, err)
    assert max(err.values()) <= BOUND[engine], err
    assert np.array_equal(got[:, D.I_P, :] == 0, ref[:, D.I_P, :] == 0)
    assert np.all(got[:, D.I_P, :][:, info["clamped"]] == 0)
    assert np.all(got[:, D.I_P, :][wet & ~info["clamped"]] > 0)


# ------------------------------------------------------------------ 3. batches and the frame range
@pytest.mark.parametrize("engine", ["float32", "float64"])
def test_batches_and_the_frame_range(engine):
    """nframes 1, 8 and 11 at frame0 = 5 of 24 over sentinel frames: frames
    outside the range keep the sentinel bit for bit, and a frame's planes are
    the same whichever call and batch position produced them (the 19-frame
    call: positions 0-7, 0-7, 0-2; 3 frames at 9: positions 0-2 for what was
    4-6)."""
    inp = _inputs()
    ds = _downscale(**DS)
    R = NP[engine]
    sentinel = np.stack([np.full((5, N), -777.0 + f, dtype=R) for f in range(NFRAMES)])

    def call(frame0, nframes):
        with forcing_engine(inp, engine, fill=-777.0) as e:
            assert np.array_equal(read_frames(e, range(NFRAMES)), sentinel)
            put(e, inp, inp.table[frame0:frame0 + nframes], frame0=frame0, ds=ds)
            return read_frames(e, range(NFRAMES))

    whole = call(5, 19)
    assert np.array_equal(whole[:5], sentinel[:5]) and not (whole[5:] == sentinel[5:]).any()
    for frame0, nframes in ((5, 1), (5, 8), (5, 11), (9, 3)):
        got = call(frame0, nframes)
        inside = np.zeros(NFRAMES, dtype=bool)
        inside[frame0:frame0 + nframes] = True
        assert np.array_equal(got[~inside], sentinel[~inside]), (frame0, nframes)
        assert np.array_equal(got[inside], whole[inside]), (frame0, nframes)


# ------------------------------------------------------------------ 4. several tiles per workgroup
BIG_NY, BIG_NX, BIG_NC, BIG_SEED = 1152, 2048, 512, 5


def _big_frames(ny, row0, table, z_ref):
    from topoflow_glacier.synthetic import diurnal_table

    e = make_engine(BASE_CFG, ny, BIG_NX, "float32", n_frames=2, hist_depth=1, n_catch=BIG_NC, fuse_steps=1, row0=row0,
                    split="off")
    try:
        cid = _scatter(np.arange(ny * BIG_NX) + row0 * BIG_NX, BIG_NC)
        e.fill_synthetic(BIG_SEED, diurnal_table(2), nx_global=BIG_NX)
        e.set_field("catch_id", cid)
        elev = e.get_field("elev", dtype=np.float32)
        if table is None:
            return elev, cid
        e.set_catchment_forcing(table, z_ref=z_ref, downscale=_downscale(**DS))
        return np.stack([np.stack([e.get_field(name, index=f, dtype=np.float32) for name in D.ORDER]) for f in range(2)])
    finally:
        e.close()


def test_several_tiles_per_workgroup_and_row_halves():
    """1152 x 2048 cells, 512 scattered ids, two frames, fp32: 9216 chunks, more
    tiles than k_forcing_expand's workgroup cap at either width (2304 tiles of
    four chunks over 2048 workgroups; 9216 over 4096 with one cell per lane).
    Against the restatement, and bit for bit the two 576-row halves run as
    separate handles."""
    elev, cid = _big_frames(BIG_NY, 0, None, None)
    z_ref = D.catchment_means(cid, elev, BIG_NC)
    rng = np.random.default_rng(9)
    table = np.empty((2, 5, BIG_NC))
    table[:, D.I_PA] = rng.uniform(70000.0, 80000.0, (2, BIG_NC))
    table[:, D.I_Q] = rng.uniform(0.002, 0.006, (2, BIG_NC))
    table[:, D.I_P] = rng.uniform(0.0, 2e-7, (2, BIG_NC))
    table[:, D.I_T] = rng.uniform(-12.0, 6.0, (2, BIG_NC))
    table[:, D.I_UZ] = rng.uniform(0.5, 9.0, (2, BIG_NC))
    ref, info = D.downscale(table, cid, elev.astype(np.float64), z_ref, parts=True, **DS)
    assert not info["clamped"].any() and (info["rh_before"] > 1).any() and (info["rh_before"] < 1).any()
    whole = _big_frames(BIG_NY, 0, table, z_ref)
    err = frame_err(whole, ref)
    _note("many_tiles", "float32", err)
    print(f"catchment forcing, several tiles per workgroup: {err}")
    assert max(err.values()) <= BOUND["float32"], err
    half = BIG_NY // 2 * BIG_NX
    assert np.array_equal(whole[:, :, :half], _big_frames(BIG_NY // 2, 0, table, z_ref))
    assert np.array_equal(whole[:, :, half:], _big_frames(BIG_NY // 2, BIG_NY // 2, table, z_ref))


# ------------------------------------------------------------------ 5. split launches
def test_frames_written_between_split_launches():
    """split="on": 16 steps, then the next 16 steps' frames written over the
    ones the launch read, with no join in between, then 16 more steps.  Frames,
    outputs and state equal an unsplit engine's bit for bit."""
    inp = _inputs()
    ds = _downscale(**DS)
    rows = [np.arange(16) % NFRAMES, (np.arange(16) + 5) % NFRAMES]
    assert not np.array_equal(inp.table[rows[0]], inp.table[rows[1]])

    def run(split):
        with forcing_engine(inp, "float32", n_frames=16, hist_depth=16, fuse=8, split=split) as e:
            was_split = e.is_split()
            put(e, inp, inp.table[rows[0]], ds=ds)
            e.run(16)
            put(e, inp, inp.table[rows[1]], ds=ds)  # right after run(): no sync(), no join()
            e.run(16)
            frames = read_frames(e, range(16))
            outs = np.stack([[e.get_field(name, index=s, dtype=np.float32) for s in range(16)]
                             for name in ("h_snow", "SM", "h_ice", "IM", "M_total", "RH")])
            state = np.stack([e.get_field(name) for name in ("h_swe", "h_iwe", "Eccs", "Ecci", "albedo", "n")])
            return was_split, frames, outs, state

    on, off = run("on"), run("off")
    assert on[0] and not off[0]
    assert (off[2][4] > 0).any()  # M_total: not a comparison of zeros
    for a, b in zip(on[1:], off[1:]):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------ 6. missing data
@pytest.mark.parametrize("engine", ["float32", "float64"])
def test_a_nan_table_entry_stays_in_its_catchment_and_frame(engine):
    """T_air = NaN at (frame 3, catchment 4): on a plain gather only that plane
    is non-finite, exactly in the catchment's cells; downscaled, only cells of
    the catchment in that frame are, and T_air in every one of them.  Every
    other value equals the clean call's bit for bit.  The fp32 engine's next
    8-step launch runs the NaN-safe form; after a finite host table with a
    plain gather it does not."""
    inp = _inputs()
    f, c = 3, 4
    dirty = inp.table.copy()
    dirty[f, D.I_T, c] = np.nan
    cells = inp.eff == c
    assert cells.any() and not cells.all()
    for ds in (None, _downscale(**DS)):
        with forcing_engine(inp, engine) as e:
            put(e, inp, inp.table, ds=ds)
            clean = read_frames(e, range(NFRAMES))
            assert np.isfinite(clean).all()
            base = e.nan_safe_launches()
            e.run(8, frames=np.arange(8, dtype=np.int32))
            assert e.nan_safe_launches() == base  # finite: the clean form (lazily checked when downscaled)
            put(e, inp, dirty, ds=ds)
            got = read_frames(e, range(NFRAMES))
            bad = ~np.isfinite(got)
            want = np.zeros_like(bad)
            want[f, D.I_T, cells] = True
            touched = want
            if ds is None:
                assert np.array_equal(bad, want)
            else:  # the catchment's cells in that frame: T_air NaN in each, the other planes whatever follows from it
                assert np.array_equal(bad[:, D.I_T], want[:, D.I_T])
                touched = np.zeros_like(bad)
                touched[f, :, cells] = True
                assert not (bad & ~touched).any()
            assert np.array_equal(got[~touched], clean[~touched])
            e.run(8, frames=np.arange(8, dtype=np.int32))
            assert e.nan_safe_launches() == base + (1 if engine == "float32" else 0)
    with forcing_engine(inp, engine) as e:  # a finite device table is checked lazily and runs the clean form
        put(e, inp, inp.table, device=True)
        base = e.nan_safe_launches()
        e.run(8, frames=np.arange(8, dtype=np.int32))
        assert e.nan_safe_launches() == base


# ------------------------------------------------------------------ 7. the humidity cap end to end
def test_the_models_rh_stays_under_the_cap():
    """fp64 engine, one step: RH <= 1 + 1e-12 everywhere with rh_max = 1, and
    above 1 somewhere with rh_max = 0."""
    check_forcing_preconditions()
    inp = _inputs()
    peak = {}
    for rh_max in (1.0, 0.0):
        with forcing_engine(inp, "float64", hist_depth=1) as e:
            put(e, inp, inp.table, ds=_downscale(**dict(DS, rh_max=rh_max)))
            e.run(1)
            peak[rh_max] = float(e.get_field("RH").max())
    _note("rh_peak", "float64", peak)
    assert 0.99 <= peak[1.0] <= 1.0 + 1e-12, peak
    assert peak[0.0] > 1.0, peak


# ------------------------------------------------------------------ 8. hydrograph end to end
@pytest.mark.parametrize("form", ["fp32", "fp32_flux64", "fp64"])
def test_forced_hydrograph_against_the_oracle(form):
    """forced_catchment_hydrographs, hist_depth 8, n_frames 8, 20 steps (every
    block rewrites the whole frame ring): runoff against the numpy oracle on
    the restated per-cell forcing, summed per catchment (math.fsum), times
    da_m2; z_ref left to the driver (the engine's own catchment means)."""
    from topoflow_glacier.hydrograph import forced_catchment_hydrographs
    from topoflow_glacier.routing import boxcar_route

    _, want = check_forcing_preconditions()
    inp = _inputs()
    opt = FORMS[form]
    with forcing_engine(inp, opt.get("engine", "float32"), n_frames=8, hist_depth=8, flux=opt.get("flux", "fp32")) as e:
        s, cells = e.catchment_mean_elevation()
        assert np.array_equal(cells, np.bincount(inp.cid, minlength=inp.nc))
        assert np.abs(s / cells - inp.z_ref).max() <= 1e-12 * inp.z_ref.max()
        res = forced_catchment_hydrographs(e, inp.table[:NSTEPS], downscale=_downscale(**DS))
        assert e.step_index == NSTEPS
    assert res["runoff"].shape == (NSTEPS, inp.nc) and res["runoff"].dtype == np.float64
    err = floored_err(res["runoff"], want)
    _note("hydrograph_floored", form, err)
    print(f"forced catchment hydrograph vs oracle {form}: {err}")
    assert err <= (1e-12 if form == "fp64" else 1e-5), err
    assert np.array_equal(res["routed"], boxcar_route(res["runoff"], 20))


# ------------------------------------------------------------------ 9. rejected arguments
def test_rejected_arguments_leave_the_frames_as_they_were():
    """Every argument check returns TFG_ERR_ARG and no frame changes."""
    from topoflow_glacier import _native as nat

    inp = _inputs()
    nan, inf = float("nan"), float("inf")
    with forcing_engine(inp, "float32", n_frames=8, fill=-777.0) as e:
        before = read_frames(e, range(8))
        t = np.ascontiguousarray(inp.table[:8])
        zero = np.zeros((0, 5, inp.nc))
        cases = [dict(table=t, frame0=-1), dict(table=zero, frame0=0), dict(table=t, frame0=1), dict(table=t[:1], frame0=8)]
        cases += [dict(table=t, z_ref=inp.z_ref, downscale=_downscale(**dict(DS, **kw)))
                  for kw in (dict(rh_max=nan), dict(rh_max=inf), dict(rh_max=-1.0), dict(lapse_T=nan), dict(lapse_T=inf),
                             dict(grad_P=nan), dict(grad_P=-inf), dict(pressure=2), dict(pressure=-1))]
        cases += [dict(table=t, downscale=_downscale(**{k: v})) for k, v in DS.items()]  # z_ref == NULL with a term on
        for kw in cases:
            with pytest.raises(nat.NativeError, match="catchment forcing") as ei:
                e.set_catchment_forcing(**kw)
            assert ei.value.code == nat.ERR_ARG, kw
        tp = t.ctypes.data_as(ctypes.c_void_p)
        assert e.lib.tfg_set_catchment_forcing(e.h, 0, 8, None, 0, None, None) == nat.ERR_ARG  # null table
        assert e.lib.tfg_set_catchment_forcing(None, 0, 8, tp, 0, None, None) == nat.ERR_ARG  # null handle
        assert np.array_equal(read_frames(e, range(8)), before)
        # and the handle still takes a good call: an all-off Downscale needs no z_ref
        e.set_catchment_forcing(t, downscale=_downscale())
        assert np.array_equal(read_frames(e, range(8)), t[:, :, inp.eff].astype(np.float32))


# ------------------------------------------------------------------ 10. the staging ring of the two entry points
@pytest.mark.parametrize("engine", ["float32", "float64"])
def test_set_inputs_and_catchment_forcing_share_one_staging_ring(engine):
    """tfg_set_inputs and tfg_set_catchment_forcing stage a host source through
    one two-slot pinned ring.  Four calls with no sync in between, on 7 x 77 =
    539 cells (plane stride 576, no multiple of 256): the largest request
    (5 n doubles) into slot 0, the smallest (a table of 2 frames x 5 x 3
    catchments) into slot 1, then 5 n floats into slot 0 again (kept: smaller)
    and 5 n doubles into slot 1 (grown).  Each source is overwritten as soon as
    its call returns: it was borrowed for the call only.  Every plane read back
    equals what was sent, converted once to the engine's type, bit for bit."""
    from topoflow_glacier import _native as nat

    ny, nx, nc = 7, 77, 3
    n = ny * nx
    R = NP[engine]
    rng = np.random.default_rng(539)
    cid = (np.arange(n) % nc).astype(np.int32)
    a0, a4 = rng.uniform(-3.0, 3.0, (2, 5, n))  # fp64 values that fp32 rounds
    a3 = rng.uniform(-3.0, 3.0, (5, n)).astype(np.float32)
    table = rng.uniform(-3.0, 3.0, (2, 5, nc))
    want = np.stack([a0.astype(R), table[0][:, cid].astype(R), table[1][:, cid].astype(R), a3.astype(R), a4.astype(R)])
    assert engine == "float64" or not np.array_equal(want[0].astype(np.float64), a0)  # the conversion is a real one
    e = make_engine(BASE_CFG, ny, nx, engine, n_frames=5, hist_depth=1, n_catch=nc, fuse_steps=1)
    try:
        e.set_field("catch_id", cid)

        def send_inputs(frame, src, code):
            src = np.array(src)  # the call's own copy
            e._chk(e.lib.tfg_set_inputs(e.h, frame, src.ctypes.data_as(ctypes.c_void_p), code, n, 0))
            src.fill(np.nan)

        send_inputs(0, a0, nat.F64)
        t = np.array(table)
        e._chk(e.lib.tfg_set_catchment_forcing(e.h, 1, 2, t.ctypes.data_as(ctypes.c_void_p), 0, None, None))
        t.fill(np.nan)
        send_inputs(3, a3, nat.F32)
        send_inputs(4, a4, nat.F64)
        got = read_frames(e, range(5))
    finally:
        e.close()
    assert got.dtype == want.dtype and np.array_equal(got, want)
