"""Per-cell time aggregates of the history planes folded on the device
(k_cell_aggregate; tfg_cell_aggregate), through GlacierEngine.cell_aggregate
and aggregate.aggregated_run: the kernel against a numpy left fold of the
planes it read, continuation across calls, unaligned and guarded buffers,
special values, several tiles per workgroup, split launches, the numpy oracle
and the edges of the interface.

References.  For the plane tests the history slots are written directly
(set_field(name, values, index=slot)) and the expected result is np_fold below
over the planes as get_field returns them (for h_snow and h_ice, which
get_field serves from the state after a host set, the planes as written), in
slot order: float64 `+`,
np.maximum, np.minimum and `>`, the operations the kernel performs in the
order it performs them, so every comparison is exact (`==` on the values,
identical NaN positions, the sum bit for bit) and the observed error is 0 by
construction.  The oracle comparison holds the per-cell sum of M_total over
20 steps to the project's bounds (floored form): 1e-5 for the
fp32 forms and 1e-12 for the fp64 engine, relative to the array's largest
entry.  On the oracle alone, before any GPU value is read: the summed M_total
is positive in 2644 of the 3700 cells.

Measured on an MI355X (TFG_REPORT_DIR/cell_aggregate.json): see MEASURED.
"""

import contextlib
import ctypes

import numpy as np
import pytest

from tests.harness import BASE_CFG, make_engine
from tests.test_gpu_catchment_series import _oracle_outputs, history_engine
from tests.test_gpu_diagnostics import FORMS, NSTEPS, NX, NY, SEED, _oracle, _report, floored_err

pytestmark = pytest.mark.gpu

# Measured on an MI355X: every plane comparison is exact (0); the per-cell sum
# of M_total against the oracle, floored (bounds 1e-5 / 1e-5 / 1e-12).
MEASURED = {
    "planes": 0.0,
    "oracle_sum_floored": {"fp32": 1.1e-7, "fp32_flux64": 4.3e-8, "fp64": 4.8e-16},
}

FIELDS = ("h_snow", "SM", "h_ice", "IM", "M_total", "RH")
DEPTH = 11
SHAPES = [(1, 1), (3, 5), (37, 101)]
# (first slot, slots): the 9- and 11-slot calls wrap the ring of 11
CALLS = [(10, 1), (2, 7), (3, 8), (5, 9), (4, 11)]
GUARD = 64  # elements: a multiple of 16 bytes for every accumulator type
# k_cell_aggregate's launch arithmetic (csrc/tfg_aggregate.hpp): tiles of 256 lanes x
# 16 bytes, at most 2048 workgroups; above 2048 tiles a workgroup takes two trips
K_BLOCK, K_MAX_BLOCKS = 256, 2048
REPORT: dict = {}


def _note(kind, key, value):
    REPORT.setdefault(kind, {})[key] = value
    _report("cell_aggregate", REPORT)


def np_dtype(engine):
    return np.float32 if engine == "float32" else np.float64


@contextlib.contextmanager
def ring_engine(ny, nx, engine, depth=DEPTH, split=None):
    e = make_engine(BASE_CFG, ny, nx, engine, n_frames=1, hist_depth=depth, split=split)
    try:
        yield e
    finally:
        e.close()


def plant(e, name, planes):
    """Write planes [depth][n] into the field's history slots and return them
    as get_field reads them back, in the engine's dtype.  A depth set from the
    host (h_snow, h_ice) also becomes the fp64 state, which is what get_field
    returns for it until the next step, whatever the slot: for those two the
    planes are returned as they were written (the engine's dtype, copied
    without a conversion)."""
    dt = np_dtype(e.engine)
    planes = np.asarray(planes, dtype=dt)
    for s, p in enumerate(planes):
        e.set_field(name, p, index=s)
    if name in ("h_snow", "h_ice"):
        assert np.array_equal(e.get_field(name, index=0, dtype=dt), planes[-1])  # the state: the last plane set
        return planes
    back = np.stack([e.get_field(name, index=s, dtype=dt) for s in range(len(planes))])
    assert np.array_equal(back, planes, equal_nan=True)
    return back


def random_planes(seed, depth, n, dt):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((depth, n)) * 10.0).astype(dt)


def np_fold(planes, threshold, start=None):
    """The left fold of planes [m][n] in slot order: (sum, max, min, count),
    from +0.0, planes[0], planes[0] and 0, or continuing `start`."""
    if start is None:
        s = np.zeros(planes.shape[1], dtype=np.float64)
        mx, mn = planes[0].copy(), planes[0].copy()
        c = np.zeros(planes.shape[1], dtype=np.int32)
    else:
        s, mx, mn, c = (a.copy() for a in start)
    with np.errstate(invalid="ignore"):
        for v in planes:
            s = s + v.astype(np.float64)
            mx = np.maximum(mx, v)
            mn = np.minimum(mn, v)
            c = c + (v.astype(np.float64) > threshold).astype(np.int32)
    return s, mx, mn, c


SENTINEL = {"sum": -12345.5, "max": -777.25, "min": 555.75, "above": -99}


class Guarded:
    """The four accumulators as views of n elements, `offset` elements past a
    16-byte boundary, inside larger tensors filled with sentinels."""

    def __init__(self, e, offset=0):
        import torch

        self.n, self.lo = e.n, GUARD + offset
        eng = torch.float32 if e.engine == "float32" else torch.float64
        kinds = {"sum": torch.float64, "max": eng, "min": eng, "above": torch.int32}
        self.whole = {k: torch.full((self.lo + e.n + GUARD,), SENTINEL[k], dtype=dt, device=e.torch_device)
                      for k, dt in kinds.items()}
        self.view = {k: t[self.lo:self.lo + e.n] for k, t in self.whole.items()}
        for k, v in self.view.items():
            assert v.is_contiguous() and v.data_ptr() % 16 == (offset * v.element_size()) % 16, k

    def guards_intact(self):
        for k, t in self.whole.items():
            a = t.cpu().numpy()
            assert np.all(a[:self.lo] == SENTINEL[k]) and np.all(a[self.lo + self.n:] == SENTINEL[k]), k

    def untouched(self, k):
        return bool((self.whole[k] == SENTINEL[k]).all().item())

    def host(self):
        return tuple(self.view[k].cpu().numpy() for k in ("sum", "max", "min", "above"))


def assert_same(got, want, what=""):
    """Exact: equal values, identical NaN positions, and the sum bit for bit."""
    for g, w, k in zip(got, want, ("sum", "max", "min", "above")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k)
        assert np.array_equal(np.isnan(g), np.isnan(w)), (what, k)
        assert np.all((g == w) | np.isnan(w)), (what, k)
    ok = ~np.isnan(want[0])  # a NaN's payload is not part of the contract
    assert np.array_equal(got[0].view(np.int64)[ok], want[0].view(np.int64)[ok]), what


def aggregate_all(e, g, name, first, count, threshold, init=True):
    e.cell_aggregate(name, first=first, count=count, sum=g.view["sum"], max=g.view["max"], min=g.view["min"],
                     above=g.view["above"], threshold=threshold, init=init)
    e.sync()
    g.guards_intact()
    return g.host()


def slots_of(first, count, depth=DEPTH):
    return [(first + j) % depth for j in range(count)]


# ------------------------------------------------------------------ 1. the kernel against the planes it read
@pytest.mark.parametrize("engine", ["float32", "float64"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fold_equals_numpy_on_every_shape_and_slot_count(engine, shape):
    """1, 7, 8, 9 and 11 slots (the 9- and 11-slot calls wrap the ring of 11)
    of planted M_total planes, all four statistics into guarded views, 16-byte
    aligned and one element past (sum then 8-byte, the fp32 buffers 4-byte
    aligned): equal to the numpy fold exactly; the guards keep their
    sentinels; a call that asks for the sum alone leaves the other three
    buffers as they were."""
    ny, nx = shape
    with ring_engine(ny, nx, engine) as e:
        planes = plant(e, "M_total", random_planes(ny * 1000 + nx, DEPTH, ny * nx, np_dtype(engine)))
        for offset in (0, 1):
            for first, count in CALLS:
                g = Guarded(e, offset)
                got = aggregate_all(e, g, "M_total", first, count, 0.25)
                want = np_fold(planes[slots_of(first, count)], 0.25)
                assert_same(got, want, (offset, first, count))
                assert 0 < want[3].sum() < count * e.n or e.n == 1  # the threshold divides the values
                only = Guarded(e, offset)
                e.cell_aggregate("M_total", first=first, count=count, sum=only.view["sum"], init=True)
                e.sync()
                only.guards_intact()
                assert np.array_equal(only.host()[0].view(np.int64), want[0].view(np.int64))
                assert only.untouched("max") and only.untouched("min") and only.untouched("above")
    _note("planes", f"{engine}/{ny}x{nx}", 0.0)


@pytest.mark.parametrize("engine", ["float32", "float64"])
def test_every_history_field(engine):
    """Each of the six history fields on 37 x 101, 11 slots from slot 4."""
    ny, nx = SHAPES[-1]
    with ring_engine(ny, nx, engine) as e:
        planted = {name: plant(e, name, random_planes(50 + i, DEPTH, e.n, np_dtype(engine))) for i, name in enumerate(FIELDS)}
        g = Guarded(e)
        for name in FIELDS:
            got = aggregate_all(e, g, name, 4, DEPTH, -1.5)
            assert_same(got, np_fold(planted[name][slots_of(4, DEPTH)], -1.5), name)
        assert not np.array_equal(planted["SM"], planted["IM"])
    _note("fields", engine, 0.0)


@pytest.mark.parametrize("engine", ["float32", "float64"])
@pytest.mark.parametrize("offset", [0, 1])
def test_three_calls_equal_one(engine, offset):
    """4 + 5 + 2 slots (init, then two continuations) equal one call over the
    same 11 slots bit for bit, and the numpy fold continued the same way."""
    ny, nx = SHAPES[-1]
    with ring_engine(ny, nx, engine) as e:
        planes = plant(e, "SM", random_planes(9, DEPTH, e.n, np_dtype(engine)))
        one = aggregate_all(e, Guarded(e, offset), "SM", 4, 11, 0.0)
        g = Guarded(e, offset)
        aggregate_all(e, g, "SM", 4, 4, 0.0, init=True)
        aggregate_all(e, g, "SM", 8, 5, 0.0, init=False)
        three = aggregate_all(e, g, "SM", (8 + 5) % DEPTH, 2, 0.0, init=False)
        for a, b in zip(three, one):
            assert a.tobytes() == b.tobytes()
        order = slots_of(4, 11)
        want = np_fold(planes[order[:4]], 0.0)
        want = np_fold(planes[order[4:9]], 0.0, start=want)
        want = np_fold(planes[order[9:]], 0.0, start=want)
        assert_same(three, want)
        assert_same(one, np_fold(planes[order], 0.0))
    _note("continuation", f"{engine}/offset{offset}", 0.0)


# ------------------------------------------------------------------ 2. special values
@pytest.mark.parametrize("engine", ["float32", "float64"])
def test_special_values(engine):
    """Negative values, +-inf, -0.0 and one NaN (cell 40 of the fourth slot
    read): max, min and sum of that cell are NaN from that slot on and finite
    before it, its count skips that slot, every other cell equals the fold of
    the planes without the NaN, and a value equal to the threshold is not
    counted; a continuation from buffers that hold NaN keeps it."""
    ny, nx = SHAPES[-1]
    dt = np_dtype(engine)
    first, nan_cell, nan_j = 6, 40, 3
    with ring_engine(ny, nx, engine) as e:
        clean = random_planes(21, DEPTH, e.n, dt)
        clean[:, 7] = 2.5          # equal to the threshold in every slot
        clean[:, 8] = -0.0
        clean[2, 9], clean[1, 10] = np.inf, -np.inf  # slots the 9-slot call reads
        clean[:, 11] = -np.abs(clean[:, 11]) - 3.0  # always below the threshold
        dirty = clean.copy()
        dirty[(first + nan_j) % DEPTH, nan_cell] = np.nan
        planes = plant(e, "RH", dirty)
        g = Guarded(e)
        for count in (nan_j, nan_j + 1, 9):
            got = aggregate_all(e, g, "RH", first, count, 2.5)
            order = slots_of(first, count)
            want = np_fold(planes[order], 2.5)
            assert_same(got, want, count)
            ref = np_fold(clean[order], 2.5)
            others = np.arange(e.n) != nan_cell
            for a, b in zip(got, ref):
                assert np.array_equal(a[others], b[others], equal_nan=True)
            hit = count > nan_j
            assert all(bool(np.isnan(a[nan_cell])) == hit for a in got[:3]), count
            want_count = int((clean[order, nan_cell].astype(np.float64) > 2.5).sum())
            want_count -= int(hit and clean[(first + nan_j) % DEPTH, nan_cell] > 2.5)
            assert got[3][nan_cell] == want_count
            assert got[3][7] == 0 and got[3][11] == 0 and got[3][8] == 0
            assert got[0][8] == 0.0 and not np.signbit(got[0][8])  # +0.0 + -0.0 + ... = +0.0
            assert got[1][8] == 0.0 and got[2][8] == 0.0
        assert np.isposinf(got[0][9]) and np.isposinf(got[1][9]) and np.isneginf(got[0][10]) and np.isneginf(got[2][10])
        # continue from accumulators that hold the NaN
        more = aggregate_all(e, g, "RH", 0, 2, 2.5, init=False)
        assert_same(more, np_fold(planes[[0, 1]], 2.5, start=got))
        assert all(np.isnan(a[nan_cell]) for a in more[:3])
    _note("special", engine, 0.0)


# ------------------------------------------------------------------ 3. more than one tile per workgroup
@pytest.mark.parametrize("engine,ny,nx", [("float32", 1449, 1448), ("float64", 1025, 1024)])
def test_a_workgroup_with_two_tiles(engine, ny, nx):
    """The smallest grids at which a workgroup takes a second trip of its tile
    loop: tiles of 256 lanes x 4 (fp32) or 2 (fp64) cells over at most 2048
    workgroups, so 2049 tiles (1449 x 1448) and 2050 (1025 x 1024); one row
    less gives 2048 or fewer.  Three synthetic steps, all four statistics of
    M_total and h_snow, against the planes: the leading rows and the last rows
    (the last workgroup is the one with two tiles)."""
    from topoflow_glacier.synthetic import diurnal_table

    cells = K_BLOCK * (16 // np.dtype(np_dtype(engine)).itemsize)
    assert -(-ny * nx // cells) > K_MAX_BLOCKS >= -(-(ny - 1) * nx // cells)
    steps = 3
    e = make_engine(BASE_CFG, ny, nx, engine, n_frames=steps, hist_depth=steps)
    try:
        e.fill_synthetic(5, diurnal_table(steps))
        e.run(steps)
        g = Guarded(e, 1)
        lead, tail = 64 * nx, 8 * nx
        for name in ("M_total", "h_snow"):
            got = aggregate_all(e, g, name, 0, steps, 0.0)
            planes = np.stack([e.get_field(name, index=s, dtype=np_dtype(engine)) for s in range(steps)])
            assert (planes != 0).any() and not np.array_equal(planes[0], planes[steps - 1]), name
            want = np_fold(planes, 0.0)
            assert_same([a[:lead] for a in got], [a[:lead] for a in want], name)
            assert_same([a[-tail:] for a in got], [a[-tail:] for a in want], name)
    finally:
        e.close()
    _note("two_tiles", engine, 0.0)


# ------------------------------------------------------------------ 4. real steps, split launches
def test_aggregated_run_after_split_launches():
    """The bare-ice workload on 37 x 100 cells (3700 >= 512), 20 steps on a
    ring of 8 with TFG_SPLIT_ON and no join: aggregated_run(every=7) gives
    M_total sum, h_snow max and SM above-0 per period (7, 7, 6 steps), equal to
    the same statistics folded on the host from the planes of an identically
    prepared second engine, captured block by block."""
    from topoflow_glacier.aggregate import aggregated_run

    orc = _oracle(NY, NX, SEED, NSTEPS)
    fields = {"M_total": ("sum",), "h_snow": ("max",), "SM": ("above",)}
    with history_engine(orc, "fp32", None, 1, 8, split="on") as e:
        assert e.n >= 512 and e.is_split()
        res = aggregated_run(e, NSTEPS, 7, fields)
    planes = {name: [] for name in fields}
    with history_engine(orc, "fp32", None, 1, 8, split="on") as e:
        assert e.is_split()
        for k0 in range(0, NSTEPS, 8):
            k1 = min(k0 + 8, NSTEPS)
            e.run(k1 - k0)
            for k in range(k0, k1):
                for name in fields:
                    planes[name].append(e.get_field(name, index=k % 8, dtype=np.float32))
    planes = {name: np.stack(v) for name, v in planes.items()}
    assert res["periods"].tolist() == [7, 7, 6]
    assert (planes["M_total"] > 0).any() and (planes["SM"] > 0).any() and (planes["h_snow"] > 0).any()
    for p, (a, b) in enumerate([(0, 7), (7, 14), (14, 20)]):
        s, _, _, _ = np_fold(planes["M_total"][a:b], 0.0)
        _, mx, _, _ = np_fold(planes["h_snow"][a:b], 0.0)
        _, _, _, c = np_fold(planes["SM"][a:b], 0.0)
        st = res["stats"]
        assert st["M_total"]["sum"][p].shape == (NY, NX)
        assert np.array_equal(st["M_total"]["sum"][p].reshape(-1).view(np.int64), s.view(np.int64)), p
        assert np.array_equal(st["h_snow"]["max"][p].reshape(-1), mx), p
        assert np.array_equal(st["SM"]["above"][p].reshape(-1), c), p
    assert 0 < res["stats"]["SM"]["above"].sum() < NSTEPS * NY * NX
    _note("split", "fp32", 0.0)


# ------------------------------------------------------------------ 5. against the numpy oracle
@pytest.mark.parametrize("form", ["fp32", "fp32_flux64", "fp64"])
def test_summed_runoff_against_the_oracle(form):
    """aggregated_run over the 20 steps as one period on a ring of 8 (pieces
    of 8, 8 and 4 slots): the per-cell sum of M_total against the numpy
    oracle's per-step M_total summed per cell, floored: 1e-5 for the fp32
    forms, 1e-12 for the fp64 engine.  On the oracle the sum is positive in
    2644 of the 3700 cells, so the floor hides nothing; mean is sum / 20."""
    from topoflow_glacier.aggregate import aggregated_run

    want = _oracle_outputs(NY, NX)["M_total"].sum(axis=0)
    assert int((want > 0).sum()) == 2644 and want.size == 3700  # before any GPU value is read
    with history_engine(_oracle(NY, NX, SEED, NSTEPS), form, None, 1, 8) as e:
        res = aggregated_run(e, NSTEPS, NSTEPS, {"M_total": ("sum", "mean")})
    assert res["periods"].tolist() == [NSTEPS]
    got = res["stats"]["M_total"]["sum"][0].reshape(-1)
    err = floored_err(got, want)
    _note("oracle_sum_floored", form, err)
    print(f"per-cell summed M_total vs oracle {form}: floored error {err:.3e}, largest entry {want.max():.3e}")
    assert err <= (1e-12 if form == "fp64" else 1e-5), err
    assert np.array_equal(res["stats"]["M_total"]["mean"][0].reshape(-1), got / NSTEPS)
    assert FORMS[form].get("engine", "float32") == ("float64" if form == "fp64" else "float32")


# ------------------------------------------------------------------ 6. edges of the interface
def test_bad_arguments_raise_and_leave_the_engine_usable():
    """A non-history field, a first slot out of range, 0 and hist_depth + 1
    slots, no statistic, a wrong dtype, device and length and a NaN threshold
    with `above` each raise; the engine aggregates correctly afterwards."""
    import torch

    from topoflow_glacier import _native as nat

    ny, nx = 3, 5
    with ring_engine(ny, nx, "float32") as e:
        planes = plant(e, "RH", random_planes(3, DEPTH, e.n, np.float32))
        dev = e.torch_device
        s = torch.zeros(e.n, dtype=torch.float64, device=dev)
        m = torch.zeros(e.n, dtype=torch.float32, device=dev)
        c = torch.zeros(e.n, dtype=torch.int32, device=dev)
        for kw in ({"name": "h_swe"}, {"name": "P"}, {"first": -1, "count": 1}, {"first": DEPTH, "count": 1},
                   {"first": 0, "count": 0}, {"first": 0, "count": DEPTH + 1}):
            with pytest.raises(nat.NativeError, match="cell aggregate") as ei:
                e.cell_aggregate(**{"name": "RH", "first": 0, "count": 1, **kw}, sum=s, init=True)
            assert ei.value.code == nat.ERR_ARG, kw
        bad = [
            {},                                                                  # no statistic
            {"sum": torch.zeros(e.n, dtype=torch.float32, device=dev)},          # dtypes
            {"max": torch.zeros(e.n, dtype=torch.float64, device=dev)},
            {"min": torch.zeros(e.n, dtype=torch.int32, device=dev)},
            {"above": torch.zeros(e.n, dtype=torch.int64, device=dev)},
            {"sum": torch.zeros(e.n, dtype=torch.float64)},                      # on the host
            {"sum": torch.zeros(e.n + 1, dtype=torch.float64, device=dev)},      # lengths
            {"max": torch.zeros(e.n - 1, dtype=torch.float32, device=dev)},
            {"sum": torch.zeros(2 * e.n, dtype=torch.float64, device=dev)[::2]},  # not contiguous
            {"above": c, "threshold": float("nan")},
        ]
        for kw in bad:
            with pytest.raises(ValueError):
                e.cell_aggregate("RH", first=0, count=1, init=True, **kw)
        # the C entry point's own checks: no statistic, a NaN threshold with count, a null acc
        none = nat.TfgCellStats(None, None, None, None, 0.0)
        nan_thr = nat.TfgCellStats(None, None, None, c.data_ptr(), float("nan"))
        assert e.lib.tfg_cell_aggregate(e.h, nat.FIELD["RH"], 0, 1, ctypes.byref(none), 1) == nat.ERR_ARG
        assert e.lib.tfg_cell_aggregate(e.h, nat.FIELD["RH"], 0, 1, ctypes.byref(nan_thr), 1) == nat.ERR_ARG
        assert e.lib.tfg_cell_aggregate(e.h, nat.FIELD["RH"], 0, 1, None, 1) == nat.ERR_ARG
        # a NaN threshold is ignored when no count is asked for
        e.cell_aggregate("RH", first=0, count=1, sum=s, threshold=float("nan"), init=True)
        e.cell_aggregate("RH", first=2, count=DEPTH, sum=s, max=m, above=c, threshold=1.0, init=True)
        e.sync()
        want = np_fold(planes[slots_of(2, DEPTH)], 1.0)
        assert np.array_equal(s.cpu().numpy().view(np.int64), want[0].view(np.int64))
        assert np.array_equal(m.cpu().numpy(), want[1]) and np.array_equal(c.cpu().numpy(), want[3])


def test_default_slots_are_the_last_steps_in_order():
    """Without first and count the call folds the slots of the last
    min(step_index, hist_depth) steps, as catchment_series does."""
    import torch

    orc = _oracle(NY, NX, SEED, NSTEPS)
    with history_engine(orc, "fp32", None, 1, 8) as e:
        e.run(13)
        a = torch.zeros(e.n, dtype=torch.float64, device=e.torch_device)
        b = torch.zeros_like(a)
        e.cell_aggregate("RH", sum=a, init=True)
        e.cell_aggregate("RH", first=5, count=8, sum=b, init=True)
        e.sync()
        assert torch.equal(a, b) and bool((a > 0).any().item())
        planes = np.stack([e.get_field("RH", index=(5 + j) % 8, dtype=np.float32) for j in range(8)])
        assert np.array_equal(a.cpu().numpy().view(np.int64), np_fold(planes, 0.0)[0].view(np.int64))
