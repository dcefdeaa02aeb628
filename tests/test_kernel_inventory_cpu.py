"""Guard of the per-instantiation coverage (no GPU needed): every gfx950 kernel compiled into libwsmgmap.so is listed in
profiles/kernel_coverage.txt with at least one launch by the GPU suite.  Adding a template instantiation without running it under a
GPU test and refreshing the table (profiles/README.md has the command) fails here, before any GPU time is spent."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COVERAGE = os.path.join(ROOT, "profiles", "kernel_coverage.txt")


def _tool():
    spec = importlib.util.spec_from_file_location("kernel_inventory", os.path.join(ROOT, "tools", "kernel_inventory.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_compiled_kernel_is_listed_and_launched_by_the_gpu_suite():
    ki = _tool()
    if not os.path.exists(ki.DEFAULT_LIB):
        pytest.skip("libwsmgmap.so has not been built (make -C ws-mgmap_amd/csrc)")
    built = sorted(d for _, d in ki.inventory())
    rows = ki.read_coverage(COVERAGE)
    listed = sorted(r[0] for r in rows)
    assert len(set(listed)) == len(listed), "profiles/kernel_coverage.txt lists a kernel twice"
    missing = sorted(set(built) - set(listed))
    stale = sorted(set(listed) - set(built))
    assert not missing and not stale, (
        "profiles/kernel_coverage.txt is not the inventory of the built library: compiled but not listed (run it under a GPU test and "
        f"refresh the table) {missing}; listed but no longer compiled {stale}")
    never = [r[0] for r in rows if r[1] <= 0]
    assert not never, f"kernels the GPU suite never launches: {never}"
