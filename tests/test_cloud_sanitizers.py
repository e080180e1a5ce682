"""AddressSanitizer + UndefinedBehaviorSanitizer run of the host side of the sets on arbitrary directions
(jefferson-2.0_amd/csrc/jf_cloud.cpp and jf_cloud_rule.h: the convex hull on generic, coplanar and thin-triangle sets, the
records and seed cells, the host twin of the kernels' rule, every refusal), built the way tests/test_sanitizers.py builds the
rest of the host side."""
import os
import shutil

import pytest

from conftest import ROOT
from test_sanitizers import ENV, SAN, _have_sanitizers, _run


@pytest.mark.skipif(not (shutil.which("g++") and _have_sanitizers("gcc")), reason="gcc with libasan/libubsan not available")
def test_cloud_host_side_under_asan_and_ubsan():
    build = os.path.join(ROOT, "tests", "build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "cloud_san")
    csrc = os.path.join(ROOT, "jefferson-2.0_amd", "csrc")
    _run(["g++", "-std=c++17", *SAN, "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
          os.path.join(ROOT, "tests", "san", "cloud_san_driver.cpp"), os.path.join(csrc, "jf_cloud.cpp"), "-o", exe])
    out = _run([exe], env=ENV)
    assert "0 failed checks" in out
