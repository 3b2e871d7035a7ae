"""CPU tier: the C ABI of libskw_engine.so as the dynamic linker sees it.  The library is several translation units behind one private header; a function that loses its
`extern "C"` in a move, or an internal helper that stops being `static` without being hidden, changes the exported set — which a plugin linked against the library would
otherwise meet at its own link or load time.  tests/golden/engine_exports.txt is the sorted list of `skw_*` names the library defines in its dynamic symbol table; a new entry
point is added there in the pull request that adds it."""
import os
import shutil
import subprocess

import pytest

from streamkit_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _nm():
    for tool in ("nm", "llvm-nm", "/opt/rocm/llvm/bin/llvm-nm"):
        path = shutil.which(tool)
        if path:
            return path
    return None


def test_exported_skw_names_are_the_committed_list():
    if not os.path.exists(engine.LIB_PATH):
        pytest.skip("libskw_engine.so is not built (run `python -c 'import __graft_entry__ as g; g.build()'`)")
    nm = _nm()
    if nm is None:
        pytest.skip("neither nm nor llvm-nm is installed")
    out = subprocess.run([nm, "-D", "--defined-only", engine.LIB_PATH], check=True, capture_output=True, text=True).stdout
    have = sorted({line.split()[-1] for line in out.splitlines() if line.split() and line.split()[-1].startswith("skw_")})
    want = open(os.path.join(ROOT, "tests", "golden", "engine_exports.txt"), encoding="utf-8").read().split()
    assert want == sorted(want) and len(want) > 100
    assert have == want, {"missing": sorted(set(want) - set(have)), "unexpected": sorted(set(have) - set(want))}
