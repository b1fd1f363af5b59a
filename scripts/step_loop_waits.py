"""The memory waits of k_fused's step loop, read from the gfx950 assembly.

Compiles one unit of the engine library to assembly on the CPU, with the
unit's own flags (__graft_entry__.UNITS), takes one kernel (default: the
headline instance, _native.BENCH_KERNEL), finds its innermost step loop and
prints, in order, the groups of global_load and global_store and every
`s_waitcnt vmcnt(N)` between them, then the smallest and largest N of the loop.

vmcnt counts a wave's loads and stores together, in issue order: a wait for N
retires all but the N youngest.  A frame of the two-steps-ahead loop is
followed by 7 + 6 + 7 + 6 = 26 operations before it is used, so 26 is the exact
count there; the one-step-ahead loops have 7 + 6 = 13.

  python scripts/step_loop_waits.py [--unit tfg_engine.hip] [--all-loops] [symbol prefix]

Only loads, stores and waits are read and counted.  A loop is a label that a
later line of the kernel refers to (a back edge), whatever that line is.
"""
from __future__ import annotations

import argparse
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "topoflow-glacier_amd"))

import __graft_entry__ as entry  # noqa: E402

LABEL = re.compile(r"^(\.LBB\d+_\d+):")
LABEL_REF = re.compile(r"(\.LBB\d+_\d+)\b")
LOAD = re.compile(r"^\s+global_load_\w+")
STORE = re.compile(r"^\s+global_store_\w+")
WAIT = re.compile(r"^\s+s_waitcnt\b[^;\n]*\bvmcnt\((\d+)\)")


def unit_assembly(unit: str = "tfg_engine.hip") -> str:
    """The gfx950 assembly of one unit, compiled with the flags of a build."""
    with tempfile.TemporaryDirectory() as td:
        out = Path(td) / "unit.s"
        cmd = [entry.HIPCC, *entry.build_flags(), *entry.UNITS[unit], f"-I{ROOT / 'include'}", "-S",
               "--cuda-device-only", str(entry.CSRC / unit), "-o", str(out)]
        subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
        return out.read_text()


def kernel_lines(asm: str, symbol: str) -> list[str]:
    """The lines of the one kernel whose symbol starts with `symbol`."""
    lines = asm.splitlines()
    starts = [i for i, ln in enumerate(lines) if ln.startswith(symbol) and ln.split(";")[0].rstrip().endswith(":")]
    if len(starts) != 1:
        raise SystemExit(f"{len(starts)} kernels start with {symbol}")
    for j in range(starts[0], len(lines)):
        if lines[j].lstrip().startswith(".size"):
            return lines[starts[0]:j]
    raise SystemExit(f"no end of {symbol}")


def loops(body: list[str]) -> list[tuple[int, int]]:
    """(first, last) line of every loop: a label and the last later line that
    refers to it."""
    at = {m.group(1): i for i, ln in enumerate(body) if (m := LABEL.match(ln))}
    last: dict[int, int] = {}
    for i, ln in enumerate(body):
        if LABEL.match(ln):
            continue
        for ref in LABEL_REF.findall(ln.split(";")[0]):
            if ref in at and at[ref] < i:
                last[at[ref]] = max(last.get(at[ref], 0), i)
    return sorted(last.items())


def events(body: list[str], lo: int, hi: int) -> list[tuple[str, int]]:
    """('load', n) / ('store', n) groups and ('wait', N), in program order."""
    ev: list[tuple[str, int]] = []
    for ln in body[lo:hi + 1]:
        kind = "load" if LOAD.match(ln) else "store" if STORE.match(ln) else None
        if kind:
            if ev and ev[-1][0] == kind:
                ev[-1] = (kind, ev[-1][1] + 1)
            else:
                ev.append((kind, 1))
        elif (m := WAIT.match(ln)):
            ev.append(("wait", int(m.group(1))))
    return ev


def step_loops(body: list[str]) -> list[tuple[int, int]]:
    """The innermost loops that both load and store: the step loops."""
    streams = [(lo, hi) for lo, hi in loops(body)
               if {"load", "store"} <= {k for k, _ in events(body, lo, hi)}]
    return [(lo, hi) for lo, hi in streams
            if not any((a, b) != (lo, hi) and lo <= a and b <= hi for a, b in streams)]


def steady_loop(body: list[str]) -> tuple[int, int]:
    """The step loop a long launch spends its time in: the innermost one, and
    of several (a peeled loop keeps a short tail) the one with most accesses."""
    inner = step_loops(body)
    if not inner:
        raise SystemExit("no loop with loads and stores")
    return max(inner, key=lambda r: sum(n for k, n in events(body, *r) if k != "wait"))


def loop_waits(symbol: str, unit: str = "tfg_engine.hip") -> dict:
    body = kernel_lines(unit_assembly(unit), symbol)
    lo, hi = steady_loop(body)
    ev = events(body, lo, hi)
    waits = [n for k, n in ev if k == "wait"]
    return {"events": ev, "waits": waits, "min": min(waits), "max": max(waits),
            "loads": sum(n for k, n in ev if k == "load"), "stores": sum(n for k, n in ev if k == "store")}


def show(ev: list[tuple[str, int]]) -> None:
    for kind, n in ev:
        print(f"    s_waitcnt vmcnt({n})" if kind == "wait" else f"  {n} global_{kind}")


def main() -> None:
    from topoflow_glacier import _native

    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("symbol", nargs="?", default=_native.BENCH_KERNEL)
    ap.add_argument("--unit", default="tfg_engine.hip", choices=sorted(entry.UNITS))
    ap.add_argument("--all-loops", action="store_true", help="every step loop of the kernel, not only the steady one")
    ap.add_argument("--asm", type=Path, help="read this assembly file instead of compiling the unit")
    args = ap.parse_args()
    body = kernel_lines(args.asm.read_text() if args.asm else unit_assembly(args.unit), args.symbol)
    steady = steady_loop(body)
    for lo, hi in (step_loops(body) if args.all_loops else [steady]):
        ev = events(body, lo, hi)
        waits = [n for k, n in ev if k == "wait"]
        print(f"{args.symbol}: {'steady-state ' if (lo, hi) == steady else ''}step loop, lines {lo}-{hi} of the kernel")
        show(ev)
        print(f"  vmcnt in the loop: smallest {min(waits)}, largest {max(waits)}")


if __name__ == "__main__":
    main()
