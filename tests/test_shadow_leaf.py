"""Leaf references that carry their triangles (pbrs_amd/csrc/device/scene.h, PBRS_WREF_PACKED; host/scene_prepare.cpp, pack_wide_leaves),
the tri_leaf table, and the order of the four-wide any-hit walk's leaf step (device/traverse.h, AnyWalkW: triangles first, the leaf's own
box once one of them has passed), on the CPU: a stand-alone program (tests/shadow_leaf_check.cpp), compiled once with AddressSanitizer and
UndefinedBehaviorSanitizer, checks the references and the table of six scenes and runs a restatement of the walk both ways over 120 000
rays.  Nothing is loaded into python."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "pbrs_amd", "csrc", "host")
SOURCES = [os.path.join(ROOT, "tests", "shadow_leaf_check.cpp"), os.path.join(HOST, "scene_prepare.cpp"), os.path.join(HOST, "kernel_choice.cpp"),
           os.path.join(HOST, "flatten.cpp")]
SCENES = ("terrain", "flat", "overlap", "nested", "tiny", "huge")


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("shadow_leaf") / "shadow_leaf_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Wextra", "-o", exe] + SOURCES)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr  # a failed check, or a sanitizer report
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    print(run.stdout)
    return run.stdout


def _scene(output, scene):
    m = re.search(r"^%s: triangles (\d+), wide nodes (\d+), leaves (\d+), packed (\d+), many-triangle leaves (\d+)$" % scene, output, re.M)
    assert m, output
    return [int(x) for x in m.groups()]


def test_references_and_table_hold_in_every_scene(check_output):
    # (the program stops at the first reference that decodes to another range than its leaf's, table entry that names the wrong leaf,
    # leaf that should have kept the node form, or ray on which two walks disagree)
    for scene in SCENES:
        tris, wide, leaves, packed, many = _scene(check_output, scene)
        assert tris >= 512 and wide >= 1 and packed >= 1 and packed + many == leaves, (scene, check_output)
    assert check_output.rstrip().endswith("ok"), check_output


def test_the_leaf_of_thirteen_keeps_the_node_form(check_output):
    assert _scene(check_output, "nested")[4] == 1
    assert all(_scene(check_output, s)[4] == 0 for s in SCENES if s != "nested")


def test_both_orders_of_the_leaf_step_agree_and_both_branches_are_taken(check_output):
    m = re.search(r"^terrain walks, natural boxes: rays (\d+), occluded (\d+), leaves per ray ([\d.]+), leaf box tests per ray ([\d.]+) -> ([\d.]+), "
                  r"triangle tests per ray ([\d.]+) -> ([\d.]+), triangle passed and box failed (\d+)$", check_output, re.M)
    assert m, check_output
    rays, occluded, _, boxes_before, boxes_after, tris_before, tris_after, _ = [float(x) for x in m.groups()]
    assert rays >= 100000 and occluded >= 0.1 * rays and rays - occluded >= 0.3 * rays, check_output
    assert boxes_after < boxes_before and tris_after >= tris_before, check_output
    m = re.search(r"^terrain walks, shrunk boxes: rays (\d+), occluded (\d+), triangle passed and box failed (\d+)$", check_output, re.M)
    assert m, check_output
    assert int(m.group(1)) == rays and 0 < int(m.group(2)) < occluded and int(m.group(3)) > 0, check_output
