"""The conv planner against the stated forms, on the CPU: tools/conv_plan_check.hip (host code only, its own main) plans a sweep of 44.8 million
convs with the library's plan_conv (csrc/conv_plan.hip) and checks that every pipeline plan names an instantiation csrc/conv_forms.h states and
keeps the launcher's contracts; build.S2_UNITS must be the unit list of that header.  A plan without a form was a launch-time error on the GPU.
"""
import os
import re
import subprocess

import pytest

from conftest import ROOT
from drmnet_amd import build


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("conv_plan") / "conv_plan_check")
    cmd = [build.hipcc(), "-O2", "-std=c++17", "--offload-host-only", os.path.join(ROOT, "tools", "conv_plan_check.hip"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_every_plan_has_its_form(check):
    r = subprocess.run([check], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"(\d+) pipeline plans checked .*, (\d+) violations", r.stdout)
    assert m and int(m.group(1)) > 20_000_000 and int(m.group(2)) == 0, r.stdout
    assert re.search(r"^digest [0-9a-f]{16}$", r.stdout, re.M), r.stdout


def test_build_units_are_the_stated_units(check):
    r = subprocess.run([check, "--units"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    stated = sorted(int(u) for u in r.stdout.split())
    assert len(stated) == len(set(stated)) and sorted(build.S2_UNITS) == stated
