"""The label cuts' C ABI (include/vcfdist_labelcut.h) and both label kernels of pr_cut.hip are defined dynamic symbols of the library."""
import subprocess

from vcfdist_amd import api


def test_labelcut_symbols_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True, check=True).stdout
    have = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert len(api.LABELCUT_EXPORTED) == 16 and len(set(api.LABELCUT_EXPORTED)) == 16
    for name in api.LABELCUT_EXPORTED + ["k_label_hist_strata", "k_label_boot"]:
        assert name in have, name
    L = api.lib()
    for name in api.LABELCUT_EXPORTED:
        assert hasattr(L, name), name
