"""The weight gradient's launch plan (nerf_pl_amd/csrc/wgrad_plan.h) on the CPU:
tests/wgrad_plan_check.cpp is compiled with the host compiler under the address
and undefined-behaviour sanitizers and run directly.  For every arithmetic,
graph, list / non-list path and use_w4 value an object really has, and 8 block
counts from 1 to 3,125,000, it checks the plan's invariants (wg_start, the
slabs' extents, 1 <= G <= nb, the fused pairs, the dispatch order, the slab
workspace derived from the plan: 289,467,648 bytes, attained by the f16x3 full
graph over a sample list with the LDS-DMA kernel) and the recorded totals.

The recorded totals are (slab floats / workgroups) of wgrad_launch as it was
before the plan was split out.  A row's W4 is NR_WGRAD_W4 in the environment;
whether a launch uses wgrad4 is wgrad_launch's rule (n < 2^21, asserted below
to sit there), so the rows' large-nb column, launches of nb >= 65536 full
blocks, is the W4=0 plan for the f16x3 full graph too -- except the wgrad4 row
(over a sample list) at nb = 65536, which is n = 2^21 - 1.
"""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "nerf_pl_amd", "csrc")


@pytest.fixture(scope="module")
def check_run(tmp_path_factory):
    """(exit status, output) of the check program, built and run once"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("wgrad_plan") / "wgrad_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(HERE, "wgrad_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout + r.stderr)
    return r.returncode, r.stdout + r.stderr


def test_plan_properties(check_run):
    rc, out = check_run
    assert rc in (0, 2), out       # 1 (or a sanitizer's abort): a property failed
    assert re.search(r"^properties: 128 plans hold; workspace 289467648 bytes$", out, re.M), out


def test_plan_totals(check_run):
    rc, out = check_run
    assert rc == 0 and re.search(r"^totals: 0 of 16 rows differ$", out, re.M), out


def test_plan_header_is_host_only():
    src = open(os.path.join(CSRC, "wgrad_plan.h")).read()
    assert "hip" not in re.sub(r"//.*", "", src).lower()
    assert "__device__" not in src and "__global__" not in src


def test_launch_keeps_the_w4_rule_and_the_workspace_guard():
    """use_w4 is the caller's: the environment switch and n < 2^21 sit in
    wgrad_launch, which also refuses a plan larger than the workspace"""
    src = open(os.path.join(CSRC, "wgrad.hip")).read()
    launch = src[src.index("int wgrad_launch("):]
    assert re.search(r"use_w4 = A\.w4 && !sigma_only && n < \(\(int64_t\)1 << 21\) &&\s*"
                     r"!\(w4_env && atoi\(w4_env\) == 0\);", launch)
    assert 'getenv("NR_WGRAD_W4")' in launch and "TASKMASK" not in src
    assert "NR_REQUIRE(plan.slab_floats <= kWorkspaceFloats" in launch
    assert "return kWorkspaceFloats * (int64_t)sizeof(float);" in src
    assert "kWorkspaceFloats = wgrad_plan_max_floats()" in src
