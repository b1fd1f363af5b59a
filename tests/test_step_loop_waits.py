"""The memory waits of k_fused's steady-state step loop, counted in the gfx950
assembly (scripts/step_loop_waits.py; no GPU, one compile of tfg_engine.hip).

A wave's loads and stores retire in issue order, and `s_waitcnt vmcnt(N)` waits
for all but the N youngest.  A step of the loop issues one request (6 loads)
and ends in 7 stores.  The headline instance requests two steps ahead: between
a frame's last load and the wait that needs the whole frame stand 7 + 6 + 7 + 6
= 26 operations, and at the top of the loop, before the round's first request
is issued, 7 + 6 + 7 = 20.  So

  * no wait in the loop may be below 20: a smaller count retires something
    requested after the frame the step is about to use;
  * every step's whole-frame wait must be exactly 26.  The compiler also waits
    for single loads of the frame (its first load has 31 operations behind it
    once the step's request is out), and may place such a wait ahead of the
    step's request, where the same wait counts 6 fewer; so the waits of a step
    are compared after adding the loads of the step's request still to be
    issued: the smallest must be 26, none may exceed 26 + 5.

The forms that request one step ahead (here the NaN-safe instance) have 7 + 6 =
13 behind a frame and 7 at the top of the loop.  The conditional steps of the
loop before it was peeled gave 8, 11 and 12 / 19 / 19 for the headline."""

import importlib.util
import os
import shutil
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

pytestmark = pytest.mark.skipif(shutil.which(HIPCC) is None, reason="no hipcc")

NAN_SAFE = "_ZN8tfg_kern7k_fusedIfLb0ELb0ELb0ELb0ELi1ELb1ELb0ELb0E"  # k_fused<float, ..., NS = true>
LOADS, STORES = 6, 7  # of one step


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("step_loop_waits", ROOT / "scripts" / "step_loop_waits.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.asm = mod.unit_assembly("tfg_engine.hip")
    return mod


def steps_of(ev):
    """The loop's events cut into steps, each ending with its 7th store; what
    follows the last store belongs to the first step of the next round."""
    steps, cur, stores = [], [], 0
    for kind, n in ev:
        cur.append((kind, n))
        if kind == "store":
            stores += n
            assert stores <= STORES, "a store group spans two steps"
            if stores == STORES:
                steps.append(cur)
                cur, stores = [], 0
    assert stores == 0
    steps[0] = cur + steps[0]
    return steps


def adjusted(step):
    """Each wait of a step plus the loads the step issues after it."""
    out = []
    for i, (kind, n) in enumerate(step):
        if kind == "wait":
            out.append(n + sum(m for k, m in step[i + 1:] if k == "load"))
    return out


@pytest.mark.parametrize("symbol,ahead", [(None, 2), (NAN_SAFE, 1)], ids=["headline", "nan_safe"])
def test_steady_loop_waits_are_exact(tool, symbol, ahead):
    from topoflow_glacier import _native

    body = tool.kernel_lines(tool.asm, symbol or _native.BENCH_KERNEL)
    ev = tool.events(body, *tool.steady_loop(body))
    tool.show(ev)
    rounds = ahead + 1
    assert sum(n for k, n in ev if k == "load") == rounds * LOADS
    assert sum(n for k, n in ev if k == "store") == rounds * STORES
    whole = ahead * (STORES + LOADS)        # 26 | 13
    floor = whole - LOADS                   # 20 | 7
    waits = [n for k, n in ev if k == "wait"]
    assert min(waits) >= floor, waits
    steps = steps_of(ev)
    assert len(steps) == rounds
    for step in steps:
        adj = adjusted(step)
        assert sum(n for k, n in step if k == "load") == LOADS
        assert min(adj) == whole, (adj, step)
        assert max(adj) <= whole + LOADS - 1, (adj, step)
