"""Forcing frames interpolated on the device from fields on a regular source
grid (k_forcing_regrid; tfg_set_gridded_forcing), through
GlacierEngine.set_gridded_forcing and hydrograph.gridded_forced_hydrographs:
the frames against the numpy restatement of the rule (tests/regrid_ref.py),
the precipitation clamp, batches and the frame range, several tiles per
workgroup and row-block shards, a NaN node, the model end to end, split
launches, the rejected arguments and the pinned staging ring.

Geometries (a wave of the fp32 engine holds 256 consecutive cells).
  A   37 x 100 cells on bare_ice_inputs(4, 37, 100, 24) under 4 x 9 nodes,
      y0 = -0.31, x0 = -0.27, sy = 1/9, sx = 1/11: 14 whole chunks and a ragged
      one, every wave straddles row ends, and all four edges clamp (3 rows
      north, 7 south, 3 columns west, 9 east).  24 frames, three batches.
  B1  5 x 600 cells under 3 x 20 nodes, sy = 0.37, sx = 1/31: waves inside one
      row and waves that straddle.  B2: 1 x 700 nodes, sx = 1.13 (one source
      row, a source finer than the model).  B3: B1 with the source rows
      flipped and sy < 0.  Two frames each.
Nodes are uniform random over the ranges of the bare-ice frames, z_src over
1800 .. 2700 m, Downscale(lapse_T=-0.0065, grad_P=2e-4, pressure=1, rh_max=1.0).

Asserted on the restatement alone, before any GPU value is read
(check_preconditions): geometry A's dz spans -1.2 .. 1.2 km; no precipitation
factor clamps at grad_P = 2e-4 and 15-17 % of the cells clamp at 2e-3; 43-45 %
of the cell-frames exceed RH 1 before the cap; the capped RH peaks at or under
1 + 1e-12.

Bounds.  Plain: bit-equal to the restatement rounded once to the engine's
type.  Downscaled: the catchment forcing's bounds (the arithmetic after the
interpolation is the same forcing_cell on bit-equal inputs), with s_v the
variable's largest |ref|: fp64 |gpu - ref| <= 1e-13 max(|ref|, s_v), fp32
<= 2^-23 max(|ref|, s_v).

B3 against B1.  Flipping an axis turns a0 + w (a1 - a0) into
a1 + (1 - w)(a0 - a1) with 1 - w rounded: the same number, not the same
roundings.  Nearest has no arithmetic and B3 equals B1 bit for bit, on the
restatement and on the device.  Bilinear B3 is bit-equal to ITS restatement
like every other geometry; against B1 the restatement itself differs in 43 %
of the values by at most 4.4e-16 (nodes in -1 .. 1), so the device's B3 is held
to B1 within 8 2^-53 max|node|: three lerps, each with the rounding of 1 - w
(2^-53) times a difference of at most 2 max|node| and two more roundings.

Measured on an MI355X (TFG_REPORT_DIR/gridded_forcing.json; MEASURED below
holds the same figures), the largest error of each kind:
  plain frames, every geometry, method, engine and source side   bit-equal
  downscaled frames against the restatement     fp32 5.3e-8 (one rounding to
      fp32 is 6.0e-8), fp64 1.0e-15 (Hum_sp; P_air 4.3e-16; T_air, P, uz exact)
  with the clamp (grad_P = 2e-3)                fp32 4.6e-8, fp64 7.1e-16
  1152 x 2048 under 37 x 65 nodes               fp32 5.5e-8
  bilinear B3 against B1, fp64                  5.3e-16 of the largest |node|
"""

import contextlib
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from tests import downscale_ref as D
from tests import regrid_ref as G
from tests.harness import BASE_CFG, bare_ice_inputs, make_engine
from tests.test_gpu_diagnostics import _report

pytestmark = pytest.mark.gpu

# Measured on an MI355X: the largest error of each kind as a fraction of the
# variable's largest |ref| (bounds: 1e-13 fp64, 2^-23 = 1.19e-7 fp32).
MEASURED = {
    "frames": {"float32": 5.3e-8, "float64": 1.0e-15},  # fp32: T_air, geometry B; fp64: Hum_sp, geometry A (P, T_air, uz exact)
    "clamp": {"float32": 4.6e-8, "float64": 7.1e-16},
    "many_tiles": {"float32": 5.5e-8},
    "b3_vs_b1_bilinear": {"float64": 5.3e-16},  # of the variable's largest |node|; bound 8 2^-53 = 8.9e-16
}

SEED, NFRAMES = 4, 24
DS = dict(lapse_T=-0.0065, grad_P=2e-4, pressure=1, rh_max=1.0)
BOUND = {"float32": 2.0 ** -23, "float64": 1e-13}
NP = {"float32": np.float32, "float64": np.float64}
HIST = ("h_snow", "SM", "h_ice", "IM", "M_total", "RH")
STATE = ("h_swe", "h_iwe", "Eccs", "Ecci", "albedo", "n")
GEOM = {  # ny, nx, gny, gnx, y0, x0, sy, sx, frames
    "A": (37, 100, 4, 9, -0.31, -0.27, 1 / 9, 1 / 11, NFRAMES),
    "B1": (5, 600, 3, 20, 0.4, -0.6, 0.37, 1 / 31, 2),
    "B2": (5, 600, 1, 700, 0.0, 3.25, 1.0, 1.13, 2),
    "B3": (5, 600, 3, 20, 2 - 0.4, -0.6, -0.37, 1 / 31, 2),
}
REPORT: dict = {}


def _note(kind, key, value):
    REPORT.setdefault(kind, {})[key] = value
    _report("gridded_forcing", REPORT)


def _frozen(a):
    a = np.asarray(a)
    a.setflags(write=False)
    return a


def _downscale(**kw):
    from topoflow_glacier.forcing import Downscale

    return Downscale(**kw)


def grid_of(name, method):
    from topoflow_glacier.forcing import ForcingGrid

    _, _, gny, gnx, y0, x0, sy, sx, _ = GEOM[name]
    return ForcingGrid(gny=gny, gnx=gnx, y0=y0, x0=x0, sy=sy, sx=sx, method=method)


@functools.lru_cache(maxsize=None)
def _ranges():
    """(lo, hi) of each input over the bare-ice frames of geometry A, in tfg_set_inputs order."""
    _, frames = bare_ice_inputs(SEED, 37, 100, NFRAMES)
    return tuple((float(frames[k].min()), float(frames[k].max())) for k in D.ORDER)


def random_source(rng, nframes, gny, gnx):
    src = np.empty((nframes, 5, gny, gnx))
    for v, (lo, hi) in enumerate(_ranges()):
        src[:, v] = rng.uniform(lo, hi, (nframes, gny, gnx))
    return src


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """The geometry's rasters, source fields and source elevation (read-only, shared)."""
    ny, nx, gny, gnx, *_, nframes = GEOM[name]
    static, _ = bare_ice_inputs(SEED, ny, nx, nframes)
    if name == "B3":  # B1's fields with the rows flipped
        b1 = _inputs("B1")
        src, z_src = b1.src[:, :, ::-1], b1.z_src[::-1]
    else:
        rng = np.random.default_rng(11)
        src = random_source(rng, nframes, gny, gnx)
        z_src = rng.uniform(1800.0, 2700.0, (gny, gnx))
    return SimpleNamespace(name=name, ny=ny, nx=nx, n=ny * nx, nframes=nframes, static={k: _frozen(v) for k, v in static.items()},
                           src=_frozen(np.ascontiguousarray(src)), z_src=_frozen(np.ascontiguousarray(z_src)))


@functools.lru_cache(maxsize=None)
def check_preconditions():
    """What the comparisons stand on, on the restatement alone (module docstring)."""
    inp = _inputs("A")
    for method in ("nearest", "bilinear"):
        g = grid_of("A", method)
        y, x = g.y0 + g.sy * np.arange(inp.ny), g.x0 + g.sx * np.arange(inp.nx)
        assert [(y < 0).sum(), (y > g.gny - 1).sum(), (x < 0).sum(), (x > g.gnx - 1).sum()] == [3, 7, 3, 9]
        fr, info = G.gridded(inp.src, g, inp.ny, inp.nx, z_src=inp.z_src, elev=inp.static["elev"], parts=True, **DS)
        assert -1200.0 < info["dz"].min() < -1000.0 and 1000.0 < info["dz"].max() < 1200.0
        assert not info["clamped"].any()
        assert 0.43 <= float((info["rh_before"] > 1.0).mean()) <= 0.45
        assert float(D.relative_humidity(fr, D.constants()).max()) <= 1.0 + 1e-12
        _, info2 = G.gridded(inp.src, g, inp.ny, inp.nx, z_src=inp.z_src, elev=inp.static["elev"], parts=True, **dict(DS, grad_P=2e-3))
        assert 0.15 <= float(info2["clamped"].mean()) <= 0.17
    # B3 is B1 seen from the other side: the same stencils, mirrored
    b1, b3 = _inputs("B1"), _inputs("B3")
    r1 = G.interpolate(b1.src, grid_of("B1", "nearest"), 5, 600)
    assert np.array_equal(r1, G.interpolate(b3.src, grid_of("B3", "nearest"), 5, 600))
    r1, r3 = (G.interpolate(i.src, grid_of(i.name, "bilinear"), 5, 600) for i in (b1, b3))
    assert not np.array_equal(r1, r3)
    for v in range(5):
        assert np.abs(r1[:, v] - r3[:, v]).max() <= 8 * 2.0 ** -53 * np.abs(b1.src[:, v]).max(), v
    # B2: one source row, more source columns under a wave than it has lanes' worth of cells
    (_, _, _), (i0, _, _) = G.stencil(grid_of("B2", "bilinear"), 5, 600)
    assert i0[255] - i0[0] > 256 and grid_of("B2", "bilinear").gny == 1
    return True


@contextlib.contextmanager
def grid_engine(inp, engine, n_frames=None, hist_depth=8, fuse=8, flux="fp32", split=None, fill=None, n_catch=1, cid=None,
                row0=0):
    """An initialised engine on the geometry's bare-ice rasters; the frames zero, or `fill` + frame in every value."""
    n_frames = n_frames or inp.nframes
    e = make_engine(BASE_CFG, inp.ny, inp.nx, engine, n_frames=n_frames, hist_depth=hist_depth, n_catch=n_catch, fuse_steps=fuse,
                    flux=flux, split=split, row0=row0)
    try:
        for k in ("elev", "slope", "aspect"):
            e.set_field(k, inp.static[k])
        for k in ("h_snow", "h_ice", "h_swe", "h_iwe"):
            e.set_field(k, inp.static["h0_" + k[2:]])
        if cid is not None:
            e.set_field("catch_id", cid)
        e.init_state()
        if fill is not None:
            for f in range(n_frames):
                e.set_inputs(np.full((5, inp.n), fill + f), index=f)
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


def put(e, src, grid, frame0=0, ds=None, device=False, z_src=None):
    """set_gridded_forcing of a host or device source (z_src on the same side)."""
    z = z_src if ds is not None and ds.on else None
    if device:
        import torch

        src = torch.from_numpy(np.array(src, dtype=np.float64)).to(e.torch_device)
        z = None if z is None else torch.from_numpy(np.array(z, dtype=np.float64)).to(e.torch_device)
    e.set_gridded_forcing(src, grid, frame0=frame0, z_src=z, downscale=ds)


# ------------------------------------------------------------------ 1. frames against the restatement
@pytest.mark.parametrize("geom", ["A", "B1", "B2", "B3"])
@pytest.mark.parametrize("engine", ["float32", "float64"])
def test_frames_equal_the_restatement(engine, geom):
    """Both methods, host and device sources: the plain frames bit-equal to
    the restatement rounded once (a Downscale of zeros as none), the
    downscaled frames within the engine's bound of the restatement on the
    elevation the engine holds.  B3 against B1 as the module docstring says."""
    check_preconditions()
    inp = _inputs(geom)
    R = NP[engine]
    frames = range(inp.nframes)
    worst, plain_got = {}, {}
    with grid_engine(inp, engine, fill=-777.0) as e:
        elev = e.get_field("elev", dtype=R).astype(np.float64)
        for method in ("nearest", "bilinear"):
            g = grid_of(geom, method)
            want_plain = G.gridded(inp.src, g, inp.ny, inp.nx).astype(R)
            want_ds, info = G.gridded(inp.src, g, inp.ny, inp.nx, z_src=inp.z_src, elev=elev, parts=True, **DS)
            assert (info["rh_before"] > 1).any() and (info["rh_before"] < 1).any() and not info["clamped"].any()
            for device in (False, True):
                for ds in (None, _downscale(), _downscale(**DS)):
                    if device and ds is not None and not ds.on:
                        continue
                    put(e, inp.src, g, ds=ds, device=device, z_src=inp.z_src)
                    got = read_frames(e, frames)
                    assert got.dtype == R
                    if ds is None or not ds.on:
                        assert np.array_equal(got, want_plain), (method, device, ds)
                        plain_got[method] = got
                    else:
                        err = frame_err(got, want_ds)
                        print(f"gridded forcing vs restatement {engine} {geom} {method} device={device}: {err}")
                        for k, v in err.items():
                            worst[k] = max(worst.get(k, 0.0), v)
                        assert max(err.values()) <= BOUND[engine], err
                        assert not np.array_equal(got, want_plain)
        if geom == "A":
            e.run(8)  # the frames as the last call left them feed a launch
            assert np.isfinite(e.get_field("M_total")).all()
    if geom == "B3":  # against B1 on the same engine type
        b1 = _inputs("B1")
        with grid_engine(b1, engine) as e:
            for method in ("nearest", "bilinear"):
                put(e, b1.src, grid_of("B1", method))
                got1 = read_frames(e, frames)
                if method == "nearest":
                    assert np.array_equal(plain_got[method], got1)
                elif engine == "float64":
                    d = np.abs(plain_got[method] - got1).max(axis=(0, 2)) / np.abs(b1.src).max(axis=(0, 2, 3))
                    _note("b3_vs_b1_bilinear", engine, float(d.max()))
                    assert d.max() <= 8 * 2.0 ** -53, d
                else:  # one fp32 rounding of two values 4.4e-16 apart: equal, or neighbours
                    a, b = plain_got[method], got1
                    assert np.all(np.abs(a - b) <= np.spacing(np.maximum(np.abs(a), np.abs(b))))
    _note("frames", f"{engine}/{geom}", worst)


# ------------------------------------------------------------------ 1b. the precipitation clamp
@pytest.mark.parametrize("engine", ["float32", "float64"])
def test_precipitation_clamps_to_zero_where_the_restatement_does(engine):
    """grad_P = 2e-3 on geometry A, bilinear: about 16 % of the cells clamp; P
    is exactly 0 there and the zero masks are equal."""
    check_preconditions()
    inp = _inputs("A")
    g = grid_of("A", "bilinear")
    kw = dict(DS, grad_P=2e-3)
    R = NP[engine]
    with grid_engine(inp, engine) as e:
        elev = e.get_field("elev", dtype=R).astype(np.float64)
        ref, info = G.gridded(inp.src, g, inp.ny, inp.nx, z_src=inp.z_src, elev=elev, parts=True, **kw)
        assert 0.15 <= float(info["clamped"].mean()) <= 0.17
        put(e, inp.src, g, ds=_downscale(**kw), z_src=inp.z_src)
        got = read_frames(e, range(NFRAMES))
    err = frame_err(got, ref)
    _note("clamp", engine, err)
    assert max(err.values()) <= BOUND[engine], err
    assert np.array_equal(got[:, D.I_P, :] == 0, ref[:, D.I_P, :] == 0)
    assert np.all(got[:, D.I_P, :][:, info["clamped"]] == 0) and (got[:, D.I_P, :][:, ~info["clamped"]] > 0).any()


# ------------------------------------------------------------------ 2. batches and the frame range
@pytest.mark.parametrize("engine", ["float32", "float64"])
def test_batches_and_the_frame_range(engine):
    """Ranges that cut a batch, at frame0 = 5 of 24 over sentinel frames:
    frames outside the range keep the sentinel bit for bit, and a frame's
    planes are the same whichever call and batch position produced them;
    nine frames written in one call equal the same frames written one call
    each."""
    inp = _inputs("A")
    g = grid_of("A", "bilinear")
    ds = _downscale(**DS)
    R = NP[engine]
    sentinel = np.stack([np.full((5, inp.n), -777.0 + f, dtype=R) for f in range(NFRAMES)])

    def call(ranges):
        with grid_engine(inp, engine, fill=-777.0) as e:
            assert np.array_equal(read_frames(e, range(NFRAMES)), sentinel)
            for frame0, nframes in ranges:
                put(e, inp.src[frame0:frame0 + nframes], g, frame0=frame0, ds=ds, z_src=inp.z_src)
            return read_frames(e, range(NFRAMES))

    whole = call([(5, 19)])
    assert np.array_equal(whole[:5], sentinel[:5]) and not (whole[5:] == sentinel[5:]).any()
    for ranges in ([(5, 1)], [(5, 8)], [(5, 11)], [(9, 3)], [(5, 9)], [(f, 1) for f in range(5, 14)]):
        got = call(ranges)
        inside = np.zeros(NFRAMES, dtype=bool)
        for frame0, nframes in ranges:
            inside[frame0:frame0 + nframes] = True
        assert np.array_equal(got[~inside], sentinel[~inside]), ranges
        assert np.array_equal(got[inside], whole[inside]), ranges


# ------------------------------------------------------------------ 3. several tiles per workgroup
BIG_NY, BIG_NX, BIG_SEED = 1152, 2048, 5


def _big_frames(ny, row0, src, z_src, grid):
    from topoflow_glacier.synthetic import diurnal_table

    e = make_engine(BASE_CFG, ny, BIG_NX, "float32", n_frames=2, hist_depth=1, fuse_steps=1, row0=row0, split="off")
    try:
        e.fill_synthetic(BIG_SEED, diurnal_table(2), nx_global=BIG_NX)
        if src is None:
            return e.get_field("elev", dtype=np.float32)
        e.set_gridded_forcing(src, grid, z_src=z_src, downscale=_downscale(**DS))
        return np.stack([np.stack([e.get_field(name, index=f, dtype=np.float32) for name in D.ORDER]) for f in range(2)])
    finally:
        e.close()


def test_several_tiles_per_workgroup_and_row_halves():
    """1152 x 2048 cells under 37 x 65 nodes (sy = sx = 1/32), two frames, fp32,
    every term on: 2304 tiles over k_forcing_regrid's 2048 workgroups.
    Against the restatement, and bit for bit the two 576-row halves run as
    separate handles with row0 0 and 576."""
    from topoflow_glacier.forcing import ForcingGrid

    g = ForcingGrid(gny=37, gnx=65, y0=0.0, x0=0.0, sy=1 / 32, sx=1 / 32, method="bilinear")
    elev = _big_frames(BIG_NY, 0, None, None, g).astype(np.float64)
    rng = np.random.default_rng(9)
    src = np.empty((2, 5, 37, 65))
    for v, (lo, hi) in enumerate(((70000.0, 80000.0), (0.002, 0.006), (0.0, 2e-7), (-12.0, 6.0), (0.5, 9.0))):
        src[:, v] = rng.uniform(lo, hi, (2, 37, 65))
    z_src = rng.uniform(elev.min(), elev.max(), (37, 65))
    ref, info = G.gridded(src, g, BIG_NY, BIG_NX, z_src=z_src, elev=elev, parts=True, **DS)
    assert not info["clamped"].any() and (info["rh_before"] > 1).any() and (info["rh_before"] < 1).any()
    assert info["dz"].max() > 300.0 and info["dz"].min() < -300.0
    whole = _big_frames(BIG_NY, 0, src, z_src, g)
    err = frame_err(whole, ref)
    _note("many_tiles", "float32", err)
    print(f"gridded forcing, several tiles per workgroup: {err}")
    assert max(err.values()) <= BOUND["float32"], err
    half = BIG_NY // 2 * BIG_NX
    assert np.array_equal(whole[:, :, :half], _big_frames(BIG_NY // 2, 0, src, z_src, g))
    assert np.array_equal(whole[:, :, half:], _big_frames(BIG_NY // 2, BIG_NY // 2, src, z_src, g))


# ------------------------------------------------------------------ 4. a NaN node
NAN_NODE, NAN_FRAME = (2, 5), 3


def _dirty(inp):
    src = inp.src.copy()
    src[NAN_FRAME, D.I_T, NAN_NODE[0], NAN_NODE[1]] = np.nan
    return src


@pytest.mark.parametrize("method", ["nearest", "bilinear"])
@pytest.mark.parametrize("engine", ["float32", "float64"])
def test_a_nan_node_reaches_exactly_its_stencils(engine, method):
    """T_air = NaN at node (2, 5) of frame 3, geometry A: plain, the NaN mask
    is the reach rule's (99 cells nearest, 550 bilinear, a weight of 0
    included) in that frame's T_air alone; downscaled, T_air is NaN in exactly
    those cells and nothing outside them changes.  Everything outside the
    mask equals the clean call bit for bit."""
    inp = _inputs("A")
    g = grid_of("A", method)
    reach = G.reach(g, inp.ny, inp.nx, NAN_NODE)
    assert int(reach.sum()) == {"nearest": 99, "bilinear": 550}[method]
    ref_bad = np.isnan(G.gridded(_dirty(inp), g, inp.ny, inp.nx))
    want = np.zeros_like(ref_bad)
    want[NAN_FRAME, D.I_T] = reach
    assert np.array_equal(ref_bad, want)
    for ds in (None, _downscale(**DS)):
        with grid_engine(inp, engine) as e:
            put(e, inp.src, g, ds=ds, z_src=inp.z_src)
            clean = read_frames(e, range(NFRAMES))
            assert np.isfinite(clean).all()
            put(e, _dirty(inp), g, ds=ds, z_src=inp.z_src)
            got = read_frames(e, range(NFRAMES))
        bad = ~np.isfinite(got)
        touched = want
        if ds is None:
            assert np.array_equal(bad, want)
        else:
            assert np.array_equal(bad[:, D.I_T], want[:, D.I_T])
            touched = np.zeros_like(bad)
            touched[NAN_FRAME, :, reach] = True
            assert not (bad & ~touched).any()
        assert np.array_equal(got[~touched], clean[~touched])


# ------------------------------------------------------------------ 5. end to end, without an oracle
def _divide(n):
    cell = np.arange(n)
    return (3 * np.minimum(cell // 925, 3) + cell % 3).astype(np.int32), 12


def _run16(inp, engine, split, load):
    """16 steps on frames that load(e) writes; (frames, histories, state, NaN-safe launches)."""
    cid, nc = _divide(inp.n)
    with grid_engine(inp, engine, n_frames=16, hist_depth=16, fuse=8, split=split, n_catch=nc, cid=cid) as e:
        load(e)
        base = e.nan_safe_launches()
        e.run(16)
        frames = read_frames(e, range(16))
        outs = np.stack([[e.get_field(name, index=s, dtype=NP[engine]) for s in range(16)] for name in HIST])
        state = np.stack([e.get_field(name) for name in STATE])
        return frames, outs, state, e.nan_safe_launches() - base


@pytest.mark.parametrize("engine,split", [("float32", "on"), ("float32", "off"), ("float64", None)])
def test_end_to_end_against_the_same_frames_through_set_inputs(engine, split):
    """Engine 1 takes its frames from set_gridded_forcing, downscaled, and runs
    16 steps; engine 2 is fed engine 1's read-back frames through set_inputs.
    The six histories and the state are bit-equal.  fp32 again with the NaN
    node: the launches run NaN-safe, the NaN masks and the outputs are equal."""
    check_preconditions()
    inp = _inputs("A")
    g, ds = grid_of("A", "bilinear"), _downscale(**DS)
    for src in ([inp.src] if engine == "float64" else [inp.src, _dirty(inp)]):
        one = _run16(inp, engine, split, lambda e: put(e, src[:16], g, ds=ds, z_src=inp.z_src))

        def feed(e):
            for f in range(16):
                e.set_inputs(one[0][f].astype(np.float64), index=f)

        two = _run16(inp, engine, split, feed)
        dirty = src is not inp.src
        assert np.isnan(one[0]).any() == dirty
        assert (one[1][4] > 0).any()  # M_total: not a comparison of zeros
        for a, b in zip(one[:3], two[:3]):
            assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a, b, equal_nan=True)
        if dirty:
            assert np.isnan(one[1]).any() and one[3] > 0 and two[3] > 0
        else:
            assert one[3] == 0 and two[3] == 0 and np.isfinite(one[1]).all()


@pytest.mark.parametrize("engine", ["float32", "float64"])
def test_gridded_hydrograph_equals_the_hydrograph_of_the_same_frames(engine):
    """gridded_forced_hydrographs (hist_depth 8, n_frames 12, 20 steps: the
    second block wraps the frame ring) equals catchment_hydrographs on an
    engine that holds the same 20 frames, bit for bit, and is not all zero."""
    from topoflow_glacier.hydrograph import catchment_hydrographs, gridded_forced_hydrographs

    inp = _inputs("A")
    g, ds = grid_of("A", "bilinear"), _downscale(**DS)
    cid, nc = _divide(inp.n)
    nsteps = 20
    with grid_engine(inp, engine, n_frames=12, hist_depth=8, n_catch=nc, cid=cid) as e:
        res = gridded_forced_hydrographs(e, inp.src[:nsteps], g, z_src=inp.z_src, downscale=ds)
        assert e.step_index == nsteps
    with grid_engine(inp, engine, n_frames=NFRAMES, hist_depth=8, n_catch=nc, cid=cid) as e:
        put(e, inp.src, g, ds=ds, z_src=inp.z_src)
        want = catchment_hydrographs(e, nsteps, frames=np.arange(nsteps, dtype=np.int32))
    assert res["runoff"].shape == (nsteps, nc) and (res["runoff"] > 0).any()
    assert np.array_equal(res["runoff"], want["runoff"]) and np.array_equal(res["routed"], want["routed"])


# ------------------------------------------------------------------ 6. split launches
def test_frames_written_between_split_launches():
    """split="on": 16 steps, then the next 16 steps' frames written over the
    ones the launch read, with no join in between, then 16 more steps.  Frames,
    outputs and state equal an unsplit engine's bit for bit."""
    inp = _inputs("A")
    g, ds = grid_of("A", "bilinear"), _downscale(**DS)
    rows = [np.arange(16) % NFRAMES, (np.arange(16) + 5) % NFRAMES]
    assert not np.array_equal(inp.src[rows[0]], inp.src[rows[1]])

    def run(split):
        with grid_engine(inp, "float32", n_frames=16, hist_depth=16, fuse=8, split=split) as e:
            was_split = e.is_split()
            put(e, inp.src[rows[0]], g, ds=ds, z_src=inp.z_src)
            e.run(16)
            put(e, inp.src[rows[1]], g, ds=ds, z_src=inp.z_src)  # right after run(): no sync(), no join()
            e.run(16)
            frames = read_frames(e, range(16))
            outs = np.stack([[e.get_field(name, index=s, dtype=np.float32) for s in range(16)] for name in HIST])
            state = np.stack([e.get_field(name) for name in STATE])
            return was_split, frames, outs, state

    on, off = run("on"), run("off")
    assert on[0] and not off[0]
    assert (off[2][4] > 0).any()  # M_total: not a comparison of zeros
    for a, b in zip(on[1:], off[1:]):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------ 7. rejected arguments
def test_rejected_arguments_leave_the_frames_as_they_were():
    """Every argument check returns TFG_ERR_ARG, through ctypes, and no frame changes."""
    from topoflow_glacier import _native as nat

    inp = _inputs("A")
    nan, inf = float("nan"), float("inf")
    src = np.ascontiguousarray(inp.src[:8])
    z = np.ascontiguousarray(inp.z_src)
    sp, zp = src.ctypes.data_as(ctypes.c_void_p), z.ctypes.data_as(ctypes.c_void_p)
    good = dict(gny=4, gnx=9, method=nat.REGRID_BILINEAR, pad=0, y0=-0.31, x0=-0.27, sy=1 / 9, sx=1 / 11, row0=0)

    def grid(**kw):
        return ctypes.byref(nat.TfgForcingGrid(**dict(good, **kw)))

    def dsc(**kw):
        d = dict(DS, **kw)
        return ctypes.byref(nat.TfgDownscale(d["lapse_T"], d["grad_P"], d["rh_max"], d["pressure"], 0))

    with grid_engine(inp, "float32", n_frames=8, fill=-777.0) as e:
        before = read_frames(e, range(8))
        call = e.lib.tfg_set_gridded_forcing
        cases = [(None, 0, 8, sp, zp, grid(), None),                     # null handle
                 (e.h, 0, 8, None, zp, grid(), None),                    # null src
                 (e.h, 0, 8, sp, zp, None, None)]                        # null grid
        cases += [(e.h, f0, nf, sp, zp, grid(), None) for f0, nf in ((-1, 8), (0, 0), (1, 8), (8, 1), (0, 9))]
        cases += [(e.h, 0, 8, sp, zp, grid(**kw), None) for kw in (
            dict(gny=0), dict(gnx=0), dict(gny=-4), dict(method=2), dict(method=-1), dict(row0=-1),
            dict(y0=nan), dict(y0=inf), dict(x0=nan), dict(x0=-inf), dict(sy=nan), dict(sy=inf), dict(sx=nan), dict(sx=-inf))]
        cases += [(e.h, 0, 8, sp, zp, grid(), dsc(**kw)) for kw in (
            dict(rh_max=nan), dict(rh_max=inf), dict(rh_max=-1.0), dict(lapse_T=nan), dict(lapse_T=inf), dict(grad_P=nan),
            dict(grad_P=-inf), dict(pressure=2), dict(pressure=-1))]
        cases += [(e.h, 0, 8, sp, None, grid(), dsc(**dict(D.OFF, **{k: v}))) for k, v in DS.items()]  # z_src == NULL, a term on
        for h, f0, nf, s_, z_, g_, d_ in cases:
            assert call(h, f0, nf, s_, 0, z_, g_, d_) == nat.ERR_ARG
        assert np.array_equal(read_frames(e, range(8)), before)
        with pytest.raises(nat.NativeError, match="gridded forcing") as ei:
            e.set_gridded_forcing(src, grid_of("A", "bilinear"), downscale=_downscale(**DS))
        assert ei.value.code == nat.ERR_ARG
        # and the handle still takes a good call: an all-off Downscale needs no z_src
        assert call(e.h, 0, 8, sp, 0, None, grid(), dsc(**D.OFF)) == nat.OK
        assert np.array_equal(read_frames(e, range(8)), G.gridded(src, grid_of("A", "bilinear"), inp.ny, inp.nx).astype(np.float32))


# ------------------------------------------------------------------ 8. the staging ring of the entry points
@pytest.mark.parametrize("engine", ["float32", "float64"])
def test_set_inputs_and_gridded_forcing_share_one_staging_ring(engine):
    """tfg_set_inputs and tfg_set_gridded_forcing stage a host source through
    one two-slot pinned ring.  Four calls with no sync in between, on 7 x 77 =
    539 cells: 5 n doubles into slot 0, a source of 2 frames x 5 x 2 x 3 nodes
    with its z_src into slot 1, then 5 n floats into slot 0 again and 5 n
    doubles into slot 1 (grown).  Each source is overwritten as soon as its
    call returns: it was borrowed for the call only.  Every plane read back
    equals what was sent, bit for bit."""
    from topoflow_glacier import _native as nat
    from topoflow_glacier.forcing import ForcingGrid

    ny, nx = 7, 77
    n = ny * nx
    R = NP[engine]
    rng = np.random.default_rng(539)
    g = ForcingGrid(gny=2, gnx=3, y0=0.1, x0=-0.2, sy=0.13, sx=0.03, method="bilinear")
    a0, a4 = rng.uniform(-3.0, 3.0, (2, 5, n))  # fp64 values that fp32 rounds
    a3 = rng.uniform(-3.0, 3.0, (5, n)).astype(np.float32)
    src, z_src = rng.uniform(-3.0, 3.0, (2, 5, 2, 3)), rng.uniform(0.0, 10.0, (2, 3))
    e = make_engine(BASE_CFG, ny, nx, engine, n_frames=5, hist_depth=1, fuse_steps=1)
    try:
        e.set_field("elev", rng.uniform(0.0, 10.0, n))
        elev = e.get_field("elev", dtype=R).astype(np.float64)
        mid = G.gridded(src, g, ny, nx, z_src=z_src, elev=elev, lapse_T=-0.5)  # T_air alone moves: exact to one rounding
        want = np.stack([a0.astype(R), mid[0].astype(R), mid[1].astype(R), a3.astype(R), a4.astype(R)])

        def send_inputs(frame, s, code):
            s = np.array(s)  # the call's own copy
            e._chk(e.lib.tfg_set_inputs(e.h, frame, s.ctypes.data_as(ctypes.c_void_p), code, n, 0))
            s.fill(np.nan)

        send_inputs(0, a0, nat.F64)
        s, z = np.array(src), np.array(z_src)
        gs = nat.TfgForcingGrid(2, 3, nat.REGRID_BILINEAR, 0, g.y0, g.x0, g.sy, g.sx, 0)
        ds = nat.TfgDownscale(-0.5, 0.0, 0.0, 0, 0)
        e._chk(e.lib.tfg_set_gridded_forcing(e.h, 1, 2, s.ctypes.data_as(ctypes.c_void_p), 0, z.ctypes.data_as(ctypes.c_void_p),
                                             ctypes.byref(gs), ctypes.byref(ds)))
        s.fill(np.nan)
        z.fill(np.nan)
        send_inputs(3, a3, nat.F32)
        send_inputs(4, a4, nat.F64)
        got = read_frames(e, range(5))
    finally:
        e.close()
    assert got.dtype == want.dtype
    plain = np.ones(5, dtype=bool)
    plain[D.I_T] = False
    assert np.array_equal(got[:, plain], want[:, plain])
    assert np.array_equal(got[[0, 3, 4]], want[[0, 3, 4]])
    err = np.abs(got[1:3, D.I_T].astype(np.float64) - mid[:, D.I_T]).max() / np.abs(mid[:, D.I_T]).max()
    assert err <= BOUND[engine], err
