"""The light a shadow ray was aimed at (pbrs_amd/csrc/device/scene.h, PBRS_SKIP_*; host/scene_prepare.cpp, prepare_scene and
write_light_links; device/shade.h, light_skip_tag; device/traverse.h, AnyWalk::skip), on the CPU: a stand-alone program
(tests/light_skip_check.cpp), compiled once with AddressSanitizer and UndefinedBehaviorSanitizer, checks the links of four host-prepared
scenes against the matching rule and runs a restatement of the any-hit walk with and without the skip over 110 000 rays per scene, with
the host's links and with forged ones.  Nothing is loaded into python."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "pbrs_amd", "csrc", "host")
SOURCES = [os.path.join(ROOT, "tests", "light_skip_check.cpp"), os.path.join(HOST, "scene_prepare.cpp"), os.path.join(HOST, "kernel_choice.cpp"),
           os.path.join(HOST, "flatten.cpp")]
# scene: (lights, lights that have an instance that is the light, the TLAS is scanned)
SCENES = {"c1": (1, 1, True), "cornell": (2, 0, True), "terrain": (4, 4, True), "lights": (24, 14, False)}


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("light_skip") / "light_skip_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Wextra", "-o", exe] + SOURCES)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr  # a failed check, or a sanitizer report
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    print(run.stdout)
    return run.stdout


def _scene(output, scene):
    m = re.search(r"^%s: instances (\d+), lights (\d+), linked (\d+), scanned leaves (\d+); rays (\d+), scanned (\d+), occluded (\d+), tagged (\d+), "
                  r"own test passes (\d+), instance visits per ray ([\d.]+) -> ([\d.]+)$" % scene, output, re.M)
    assert m, output
    return [float(x) for x in m.groups()]


def test_every_link_satisfies_the_rule_and_the_walks_agree(check_output):
    # (the program stops at the first link that breaks the rule, padding word that differs from its link, ray that is tagged although its
    # linked instance's own test passes, or ray on which the walk with the skip and the walk without it disagree)
    for scene, (lights, linked, scanned) in SCENES.items():
        _, n_lights, n_linked, leaves, rays, _, _, _, _, _, _ = _scene(check_output, scene)
        assert (n_lights, n_linked) == (lights, linked) and (leaves > 0) == scanned and rays >= 100000, (scene, check_output)
    assert check_output.rstrip().endswith("ok"), check_output


def test_both_outcomes_of_the_own_test_and_both_kinds_of_walk_are_taken(check_output):
    for scene, (_, linked, scanned) in SCENES.items():
        _, _, _, _, rays, on_scan, occluded, tagged, own_passes, before, after = _scene(check_output, scene)
        assert 0 < occluded < rays, (scene, check_output)
        # rays outside the guarded range of the division-free box test walk the tree even where the TLAS is scanned
        assert (0 < on_scan < rays) if scanned else on_scan == 0, (scene, check_output)
        if linked:
            assert tagged > 0.5 * rays and own_passes > 0 and after < before, (scene, check_output)
        else:
            assert tagged == 0 and after == before, (scene, check_output)


def test_forged_links_tag_rays_and_change_no_answer(check_output):
    for scene in SCENES:
        m = re.search(r"^%s forged: analytic instances (\d+), tagged (\d+), own test passes (\d+)$" % scene, check_output, re.M)
        assert m, check_output
        assert int(m.group(1)) >= 1 and int(m.group(2)) > 0 and int(m.group(3)) > 0, (scene, check_output)
