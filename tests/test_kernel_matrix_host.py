"""The kernel matrix of tests/test_gpu_kernel_matrix.py is complete: the
k_fused instantiations its runs reach are exactly those in the built library.

The gfx950 code objects' function symbols _ZN8tfg_kern7k_fusedI... carry the
template arguments (Itanium mangling: `f` / `d` for the engine type, Lb0E /
Lb1E per flag, Li1E for the cells per thread).  A new template flag, a new
form's translation unit or a dropped instantiation changes that set, and this
test then fails until the matrix reaches it.  No GPU is needed.
"""

import re

import pytest

from tests import test_gpu_kernel_matrix as M

SYMBOL = re.compile(r"^_ZN8tfg_kern7k_fusedI([fd])((?:L[bi]\d+E)+)E")
# k_fused<R, EXACT, READ_DEPTHS, CATCH, QC, C, NS, PREC, SAT>: the kinds of the arguments after R
KINDS = "bbbbibbb"


def built_kernels():
    """The template-argument tuples of the k_fused function symbols in the
    library's gfx950 code objects, in test_gpu_kernel_matrix.KERNELS' form."""
    from topoflow_glacier import _native

    if not _native.LIB_PATH.exists():
        pytest.skip("the engine library is not built")
    found = []
    for elf in _native.gfx950_code_objects():
        for name, _value, _size, typ, _sec_addr, _sec_off in _native._elf_symbols(elf):
            if typ != 2 or "k_fused" not in name:  # STT_FUNC: the kernels, not their descriptors
                continue
            m = SYMBOL.match(name)
            assert m, f"a k_fused symbol this test cannot parse: {name}"
            args = re.findall(r"L([bi])(\d+)E", m.group(2))
            assert "".join(k for k, _ in args) == KINDS, f"k_fused's template arguments changed: {name}"
            found.append((m.group(1), *(bool(int(v)) if k == "b" else int(v) for k, v in args)))
    return found


def test_the_matrix_reaches_every_built_k_fused():
    found = built_kernels()
    assert len(found) == len(set(found)) == 72, len(found)
    missing, extra = set(found) - M.KERNELS, M.KERNELS - set(found)
    assert not missing, f"built but launched by no corner of the matrix: {sorted(missing)}"
    assert not extra, f"claimed by the matrix but not in the library: {sorted(extra)}"


def test_the_matrix_is_36_corners_in_two_variants():
    corners = [c for f in M.FORMS for c in M.corners_of(f)]
    assert len(corners) == len(set(corners)) == 36
    assert len(M.KERNELS) == 72
    # READ_DEPTHS = false comes from the second launch of variant A alone, NS from the fp32 forms alone
    assert all(len(M.launched_kernels(c, "A")) == 2 and len(M.launched_kernels(c, "B")) == 1 for c in corners)
    assert not any(k[6] for k in M.KERNELS if k[0] == "d")
