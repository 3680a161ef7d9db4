"""The Python copies of the moments kernel's constants equal the header's (include/xvector_hip.h), and the slab-edge cases of
tests/test_gpu_moments.py are built from the same number."""
import os
import re

from conftest import ROOT


def _header_define(name):
    text = open(os.path.join(ROOT, "include", "xvector_hip.h")).read()
    m = re.search(r"^#define\s+%s\s+(\d+)\s*$" % name, text, flags=re.M)
    assert m, name
    return int(m.group(1))


def test_moment_slab_matches_the_header():
    from xvector_amd import hiplib
    assert hiplib.MOMENT_SLAB == _header_define("XV_MOMENT_SLAB")


def test_slab_edge_cases_follow_the_constant():
    import test_gpu_moments
    from xvector_amd import hiplib
    S = hiplib.MOMENT_SLAB
    ns = {n for _, n in test_gpu_moments._cases()}
    assert {1, 3, 4, 5, S - 1, S, S + 1, 3 * S + 7} <= ns
    dims = {d for d, _ in test_gpu_moments._cases()}
    assert {1, 5, 16, 17, 100, 200, 256} <= dims
