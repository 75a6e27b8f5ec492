"""The split planes of the inner BLAS nodes (pbrs_amd/csrc/device/split_planes.h, host/scene_prepare.cpp) and the cull the closest-hit
walk makes with them, on the CPU: a stand-alone program (tests/split_planes_check.cpp), compiled once with AddressSanitizer and
UndefinedBehaviorSanitizer, checks the planes of six scenes node by node and runs a restatement of the walk with and without the cull
over a few thousand rays each.  Nothing is loaded into python."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "pbrs_amd", "csrc", "host")
SOURCES = [os.path.join(ROOT, "tests", "split_planes_check.cpp"), os.path.join(HOST, "scene_prepare.cpp"), os.path.join(HOST, "kernel_choice.cpp"),
           os.path.join(HOST, "flatten.cpp")]
SCENES = ("five", "overlap", "flat", "tiny", "huge", "terrain")


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("split_planes") / "split_planes_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Wextra", "-o", exe] + SOURCES)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr  # a failed check, or a sanitizer report
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    print(run.stdout)
    return run.stdout


def _row(output, scene):
    m = re.search(r"^%s: inner nodes (\d+) \(with planes (\d+)\), rays (\d+) \(guarded range (\d+), hits (\d+)\), pops per ray ([\d.]+) -> ([\d.]+), "
                  r"failed pops per ray ([\d.]+) -> ([\d.]+), culled at push ([\d.]+)$" % scene, output, re.M)
    assert m, output
    return [float(x) for x in m.groups()]


def test_planes_hold_and_the_cull_changes_no_hit_in_every_scene(check_output):
    # (the program stops at the first plane on the wrong side, differing (t, prim) or culled child that passes its box test)
    for scene in SCENES:
        _row(check_output, scene)
    assert check_output.rstrip().endswith("ok"), check_output


def test_every_scene_has_planes_rays_in_the_guarded_range_and_hits(check_output):
    for scene in SCENES:
        inner, with_planes, rays, guarded, hits = _row(check_output, scene)[:5]
        assert inner >= 1 and with_planes >= 1 and rays >= 2000 and guarded >= rays // 2 and hits >= rays // 20, (scene, check_output)
    assert _row(check_output, "five")[0] == 1


def test_the_cull_removes_failed_pops_on_the_terrain(check_output):
    _, _, _, _, _, pops, pops_cull, failed, failed_cull, culled = _row(check_output, "terrain")
    assert culled > 0 and pops_cull < pops and failed_cull < failed, check_output
