"""The symbols of include/vcfdist_matchkind.h in the built library: every name of api.MATCHKIND_EXPORTED is a defined dynamic symbol,
and so is the kernel."""
import subprocess

from vcfdist_amd import api


def test_matchkind_symbols_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True, check=True).stdout
    have = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert len(api.MATCHKIND_EXPORTED) == 6 and len(set(api.MATCHKIND_EXPORTED)) == 6
    for name in api.MATCHKIND_EXPORTED + ["k_matchkind"]:
        assert name in have, name
    L = api.lib()
    for name in api.MATCHKIND_EXPORTED:
        assert hasattr(L, name), name
