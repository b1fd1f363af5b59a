"""The cell aggregates above the kernel, without a GPU: the C ABI's null
handle, aggregated_run's cutting of blocks into periods over a stub engine,
and the after_block hook of catchment_hydrographs."""

from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import pytest


def test_null_handle_is_rejected_without_a_device():
    """tfg_cell_aggregate fails cleanly on a null handle (no HIP call is made),
    and the binding lists the symbol."""
    import ctypes

    from topoflow_glacier import _native as nat

    L = nat.load()
    acc = nat.TfgCellStats(None, None, None, None, 0.0)
    assert L.tfg_cell_aggregate(None, nat.FIELD["M_total"], 0, 1, ctypes.byref(acc), 1) == nat.ERR_ARG
    assert b"null handle" in L.tfg_last_error(None)
    assert "tfg_cell_aggregate" in nat.exported_symbols()
    assert L.tfg_abi_version() == 8  # the entry point is an addition to ABI 8


class StubEngine:
    """What aggregated_run and catchment_hydrographs use of a GlacierEngine, on
    the host: step k (absolute) writes plane(name, k) to history slot
    k % hist_depth; cell_aggregate and catchment_series read the ring back."""

    torch_device = "cpu"
    engine = "float32"
    ny, nx, n = 2, 3, 6
    FIELDS = ("M_total", "h_snow", "SM")

    def __init__(self, hist_depth, step_index=0, n_catch=2, da_m2=2.0):
        self.hist_depth, self.step_index, self.n_catch = hist_depth, step_index, n_catch
        self.params = SimpleNamespace(da_m2=da_m2)
        self.held = [None] * hist_depth  # the step whose planes a slot holds
        self.calls = []

    @classmethod
    def plane(cls, name, k):
        """Values exact in float32, different per field, step and cell; SM is 0 on odd steps."""
        v = (cls.FIELDS.index(name) + 1) * 1000.0 + k * 8.0 + np.arange(cls.n, dtype=np.float64)
        if name == "SM" and k % 2:
            v = np.zeros(cls.n)
        return v.reshape(cls.ny, cls.nx)

    def run(self, nsteps, frames=None):
        self.calls.append(("run", nsteps, None if frames is None else list(frames)))
        for k in range(self.step_index, self.step_index + nsteps):
            self.held[k % self.hist_depth] = k
        self.step_index += nsteps

    def cell_aggregate(self, name, first=None, count=None, *, sum=None, max=None, min=None, above=None,
                       threshold=0.0, init=False):
        import torch

        steps = [self.held[(first + j) % self.hist_depth] for j in range(count)]
        self.calls.append(("aggregate", name, first, count, bool(init), steps,
                           tuple(k for k, t in (("sum", sum), ("max", max), ("min", min), ("above", above)) if t is not None),
                           threshold))
        for j, k in enumerate(steps):
            v = torch.from_numpy(self.plane(name, k))
            start = init and j == 0
            if sum is not None:
                sum.copy_(v if start else sum + v)
            if max is not None:
                max.copy_(v if start else torch.maximum(max, v.to(max.dtype)))
            if min is not None:
                min.copy_(v if start else torch.minimum(min, v.to(min.dtype)))
            if above is not None:
                hit = (v > threshold).to(torch.int32)
                above.copy_(hit if start else above + hit)

    def catchment_series(self, name="M_total", first=None, count=None, reduce="sum", out=None):
        self.calls.append(("series", name, first, count, reduce))
        out.zero_()
        return out

    def sync(self):
        self.calls.append(("sync",))


FIELDS = {"M_total": ("sum",), "h_snow": ("mean", "max"), "SM": ("sum", ("above", 0.0), "min")}


@pytest.mark.parametrize("start", [0, 7])
def test_aggregated_run_cuts_blocks_at_period_boundaries(start):
    """50 steps on a ring of 10 slots in periods of 24: every field's calls
    cover every step once and in order, none crosses a period boundary or is
    longer than the ring, init is set exactly on a period's first piece, the
    last period reports 2 steps, and mean divides by the period's own length."""
    from topoflow_glacier.aggregate import aggregated_run

    every, depth, nsteps = 24, 10, 50
    eng = StubEngine(depth, step_index=start)
    blocks = []
    res = aggregated_run(eng, nsteps, every, FIELDS, on_block=lambda k0, k1: blocks.append((k0, k1)))
    assert blocks == [(0, 10), (10, 20), (20, 30), (30, 40), (40, 50)]
    assert [c[1] for c in eng.calls if c[0] == "run"] == [10] * 5
    assert eng.step_index == start + nsteps
    assert res["periods"].tolist() == [24, 24, 2]
    for name in FIELDS:
        calls = [c for c in eng.calls if c[0] == "aggregate" and c[1] == name]
        assert [k for c in calls for k in c[5]] == list(range(start, start + nsteps))
        for _, _, first, count, init, steps, _, _ in calls:
            rel = [k - start for k in steps]
            assert 1 <= count <= depth and 0 <= first < depth
            assert first == steps[0] % depth
            assert len({r // every for r in rel}) == 1  # one period per call
            assert init == (rel[0] % every == 0)
    # the statistics asked of the engine: mean is carried as a sum
    asked = {c[1]: c[6] for c in eng.calls if c[0] == "aggregate"}
    assert asked == {"M_total": ("sum",), "h_snow": ("sum", "max"), "SM": ("sum", "min", "above")}
    bounds = [(0, 24), (24, 48), (48, 50)]
    planes = {name: np.stack([StubEngine.plane(name, start + k) for k in range(nsteps)]) for name in FIELDS}
    st = res["stats"]
    assert set(st) == set(FIELDS) and set(st["h_snow"]) == {"mean", "max"} and set(st["SM"]) == {"sum", "above", "min"}
    for p, (a, b) in enumerate(bounds):
        np.testing.assert_array_equal(st["M_total"]["sum"][p], planes["M_total"][a:b].sum(axis=0))
        np.testing.assert_array_equal(st["h_snow"]["mean"][p], planes["h_snow"][a:b].sum(axis=0) / (b - a))
        np.testing.assert_array_equal(st["h_snow"]["max"][p], planes["h_snow"][a:b].max(axis=0))
        np.testing.assert_array_equal(st["SM"]["sum"][p], planes["SM"][a:b].sum(axis=0))
        np.testing.assert_array_equal(st["SM"]["min"][p], planes["SM"][a:b].min(axis=0))
        np.testing.assert_array_equal(st["SM"]["above"][p], (planes["SM"][a:b] > 0).sum(axis=0))
    assert st["M_total"]["sum"].shape == (3, StubEngine.ny, StubEngine.nx)
    assert st["M_total"]["sum"].dtype == np.float64 and st["h_snow"]["mean"].dtype == np.float64
    assert st["h_snow"]["max"].dtype == np.float32 and st["SM"]["above"].dtype == np.int32


def test_on_period_gets_each_period_once_and_nothing_is_kept():
    """With on_period the finished periods are handed over in order, after a
    sync, with their own lengths, and no host arrays are returned."""
    from topoflow_glacier.aggregate import aggregated_run

    eng = StubEngine(10, step_index=7)
    seen = []

    def on_period(p, steps, stats):
        assert eng.calls[-1] == ("sync",)
        seen.append((p, steps, stats["h_snow"]["mean"].numpy().copy(), stats["M_total"]["sum"].numpy().copy()))

    res = aggregated_run(eng, 50, 24, FIELDS, on_period=on_period)
    assert "stats" not in res and res["periods"].tolist() == [24, 24, 2]
    assert [(p, s) for p, s, _, _ in seen] == [(0, 24), (1, 24), (2, 2)]
    for (p, steps, mean, total), a in zip(seen, (0, 24, 48)):
        want = np.stack([StubEngine.plane("h_snow", 7 + k) for k in range(a, a + steps)]).sum(axis=0) / steps
        np.testing.assert_array_equal(mean, want)
        np.testing.assert_array_equal(total, np.stack([StubEngine.plane("M_total", 7 + k) for k in range(a, a + steps)]).sum(axis=0))


def test_bad_field_specifications_raise():
    from topoflow_glacier.aggregate import aggregated_run

    eng = StubEngine(4)
    for bad in ({"M_total": ("median",)}, {"M_total": ()}, {"M_total": (("sum", 1.0),)}):
        with pytest.raises(ValueError):
            aggregated_run(eng, 4, 2, bad)
    with pytest.raises(ValueError):
        aggregated_run(eng, 0, 2, {"M_total": ("sum",)})
    with pytest.raises(ValueError):
        aggregated_run(eng, 4, 0, {"M_total": ("sum",)})
    assert eng.calls == [] and eng.step_index == 0


def test_hydrograph_after_block_hook():
    """after_block is called once per block, after the block's run and series
    call, with the block's k0, k1 and first slot; without it the recorded
    call sequence is what it was before the hook existed; hydrographs and cell
    aggregates come out of one pass."""
    from topoflow_glacier.aggregate import PeriodFolder
    from topoflow_glacier.hydrograph import catchment_hydrographs

    depth, start, nsteps = 8, 5, 20
    today = [("run", 8, None), ("series", "M_total", 5, 8, "sum"), ("run", 8, None), ("series", "M_total", 5, 8, "sum"),
             ("run", 4, None), ("series", "M_total", 5, 4, "sum"), ("sync",)]
    eng = StubEngine(depth, step_index=start)
    catchment_hydrographs(eng, nsteps, taps=4)
    assert eng.calls == today

    eng = StubEngine(depth, step_index=start)
    seen = []
    catchment_hydrographs(eng, nsteps, taps=4, after_block=lambda k0, k1, first: seen.append((k0, k1, first, len(eng.calls))))
    assert seen == [(0, 8, 5, 2), (8, 16, 5, 4), (16, 20, 5, 6)]  # after each block's run and series
    assert eng.calls == today

    eng = StubEngine(depth, step_index=start)
    folder = PeriodFolder(eng, 7, {"M_total": ("sum",)})
    catchment_hydrographs(eng, nsteps, taps=4, after_block=lambda k0, k1, first: folder.fold(first, k1 - k0))
    folder.finish()
    res = folder.result()
    assert res["periods"].tolist() == [7, 7, 6]
    assert [c for c in eng.calls if c[0] in ("run", "series")] == today[:-1]
    planes = np.stack([StubEngine.plane("M_total", start + k) for k in range(nsteps)])
    for p, (a, b) in enumerate([(0, 7), (7, 14), (14, 20)]):
        np.testing.assert_array_equal(res["stats"]["M_total"]["sum"][p], planes[a:b].sum(axis=0))
