#!/usr/bin/env python3
"""kernel_diff.py OLD.so NEW.so -- which gfx950 kernels differ between two
builds of the engine library.

Every kernel of every gfx950 code object (every function symbol that has a
``.kd`` kernel descriptor) is compared by ``_native.kernel_code_sha256``: the
kernel's instructions, its descriptor and what it reaches, with the position
in the code object masked out.  A kernel that only one library has differs
too.  Prints the differing kernels and a one-line count; exit status 1 if there
are any, 0 if every kernel is the same.  Needs no GPU.

A host-side refactor runs this against the parent commit's build: equal hashes
mean the device code, and so every result and every device time, cannot have
moved.
"""

from __future__ import annotations

import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "topoflow-glacier_amd"))

from topoflow_glacier import _native  # noqa: E402


def kernel_hashes(lib: Path) -> dict[str, str]:
    """{kernel symbol: kernel_code_sha256} over the library's gfx950 code objects."""
    out = {}
    for elf in _native.gfx950_code_objects(lib):
        syms = _native._elf_symbols(elf)
        descriptors = {s[0][:-3] for s in syms if s[0].endswith(".kd")}
        for name in sorted(s[0] for s in syms if s[3] == 2 and s[0] in descriptors):  # STT_FUNC
            out[name] = _native.kernel_code_sha256(name, lib)
    return out


def main(argv: list[str]) -> int:
    if len(argv) != 3:
        print(__doc__.strip().splitlines()[0], file=sys.stderr)
        return 2
    old, new = (kernel_hashes(Path(p)) for p in argv[1:])
    if not old or not new:
        print("kernel_diff: no gfx950 kernels found in " + (argv[1] if not old else argv[2]), file=sys.stderr)
        return 2
    differing = 0
    for name in sorted(old.keys() | new.keys()):
        a, b = old.get(name), new.get(name)
        if a != b:
            differing += 1
            print(f"{name}: {(a or 'absent')[:16]} -> {(b or 'absent')[:16]}")
    print(f"kernel_diff: {len(old)} kernels in {argv[1]}, {len(new)} in {argv[2]}, {differing} differ")
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
