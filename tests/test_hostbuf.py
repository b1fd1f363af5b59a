"""The host layer's owning buffer (csrc/tfg_hostbuf.hpp) on the CPU.

tests/native/hostbuf_main.cpp instantiates Buf<Mem> with an allocator that
counts live allocations and can fail the n-th one, and checks: reserve() grows
and keeps a smaller request; a failed grow leaves {nullptr, 0} and the next,
smaller reserve() allocates again (the earlier hand-written grow kept the old
capacity over a null pointer); moves empty their source and release the
target's old buffer; nothing is live at exit.  Any failed check is a non-zero
exit status.  The header includes no HIP header, so a plain g++ builds it.
"""

import subprocess

from tests.harness import ROOT

SRC = ROOT / "tests" / "native" / "hostbuf_main.cpp"


def test_buf_grows_fails_and_moves_cleanly(tmp_path):
    exe = tmp_path / "hostbuf_main"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", str(SRC), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 live at exit, 0 failed checks" in r.stdout, r.stdout


def test_header_is_host_only():
    text = (ROOT / "topoflow-glacier_amd" / "csrc" / "tfg_hostbuf.hpp").read_text()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes and not [i for i in includes if "hip" in i.lower()], includes
