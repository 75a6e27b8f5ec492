"""The entry nodes of the camera rays (pbrs_amd/csrc/device/entry_nodes.h, host/scene_prepare.cpp) on the CPU: a stand-alone program
(tests/entry_nodes_check.cpp), compiled once with AddressSanitizer and UndefinedBehaviorSanitizer, builds the terrain under five cameras
(and, in a second run, at full size), and checks every pixel's list (DFS order, disjoint, within the stack bound), that the lists cover
every leaf a ray of the pixel can pass, and that a restatement of the closest-hit walk with the split-plane cull gives the same (t, prim)
and the same sequence of leaves and extents from the root and from the entries — while forged lists do not.  Nothing is loaded into python."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "pbrs_amd", "csrc", "host")
SOURCES = [os.path.join(ROOT, "tests", "entry_nodes_check.cpp"), os.path.join(HOST, "scene_prepare.cpp"), os.path.join(HOST, "kernel_choice.cpp"),
           os.path.join(HOST, "flatten.cpp")]
SCENES = ("translated", "identity", "above", "inside", "straddle")


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("entry_nodes") / "entry_nodes_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Wextra", "-o", exe] + SOURCES)
    return exe


def _run(exe, *args):
    run = subprocess.run([exe, *args], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr  # a failed check, or a sanitizer report
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    print(run.stdout)
    assert run.stdout.rstrip().endswith("ok"), run.stdout
    return run.stdout


@pytest.fixture(scope="module")
def check_output(check_exe):
    return _run(check_exe)


def _counts(output, scene):
    m = re.search(r"^%s: BLAS height (\d+), stack rows (\d+), pixels (\d+) \(with entries (\d+), empty (\d+), from the root (\d+)\), entries per pixel with some ([\d.]+) "
                  r"at mean depth ([\d.]+), rays (\d+) \(hits (\d+), outside the guarded range (\d+)\), forged lists caught: removed (\d+), swapped (\d+)$" % scene,
                  output, re.M)
    assert m, output
    return [float(x) for x in m.groups()]


def _pops(output, scene):
    m = re.search(r"^%s: pops per camera ray \(passing, failed\): from the root ([\d.]+) \(([\d.]+), ([\d.]+)\)" % scene +
                  "".join(r"; fork budget %d ([\d.]+) \(([\d.]+), ([\d.]+)\)" % f for f in range(4)) + "$", output, re.M)
    assert m, output
    v = [float(x) for x in m.groups()]
    return [v[3 * i:3 * i + 3] for i in range(5)]  # from the root, then budgets 0 .. 3: (all, passing, failed)


def test_lists_cover_and_the_walk_keeps_its_bits_in_every_scene(check_output):
    # (the program stops at the first list out of order or over the stack bound, uncovered leaf, differing walk or forged list that passes)
    for scene in SCENES:
        height, rows, pixels, with_entries, empty, from_root, per_pixel, depth, rays, hits, slow, removed, swapped = _counts(check_output, scene)
        assert height >= 12 and rows >= height
        assert with_entries + empty + from_root == pixels and with_entries > pixels // 4
        assert rays == 3 * pixels and hits > rays // 4
        assert 1.0 <= per_pixel <= 8.0 and depth > 1.0
        assert removed > 0 and swapped > 0


def test_the_cameras_reach_the_cases_they_are_there_for(check_output):
    assert _counts(check_output, "translated")[1:] == _counts(check_output, "identity")[1:]  # the same view of the same terrain
    for scene in ("translated", "above", "straddle"):
        assert _counts(check_output, scene)[4] > 0, scene  # pixels that see no terrain: empty lists
    assert _counts(check_output, "inside")[4] == 0
    # whole columns (and, for the level camera, rows) of pixels straddle a zero direction component: no table there
    assert _counts(check_output, "translated")[5] >= 2 * 64
    assert _counts(check_output, "straddle")[5] >= 2 * 48 + 2 * 64 - 4


def test_entries_take_pops_off_the_walk(check_output):
    for scene in SCENES:
        root, b0, b1, b2, b3 = _pops(check_output, scene)
        assert b0[1] <= root[1] and b3[1] < b1[1] < root[1], (scene, root, b0, b1, b2, b3)  # passing pops fall with the budget
    root, _, _, _, b3 = _pops(check_output, "translated")
    assert b3[0] < 0.7 * root[0]


def test_full_size_terrain(check_exe):
    """C4's terrain at 1 048 576 triangles and 1920 x 1080, 300 sampled pixels: the table DESIGN.md quotes."""
    out = _run(check_exe, "full")
    height, rows, pixels, with_entries, empty, from_root = _counts(out, "full")[:6]
    assert height >= 20 and rows >= height and pixels == 300 and with_entries > 60 and empty > 60
    root, _, _, _, b3 = _pops(out, "full")
    assert b3[1] < 0.7 * root[1], (root, b3)
