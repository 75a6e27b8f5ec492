"""The host-only steps of pbrs_upload_scene — check_scene, prepare_scene, choose_kernels (pbrs_amd/csrc/host/) — run on the CPU: a
stand-alone program (tests/scene_prepare_check.cpp), compiled once with AddressSanitizer and UndefinedBehaviorSanitizer, checks every
refusal, the prepared layout and the kernel choice.  Nothing is loaded into python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "pbrs_amd", "csrc", "host")
SOURCES = [os.path.join(ROOT, "tests", "scene_prepare_check.cpp"), os.path.join(HOST, "scene_prepare.cpp"), os.path.join(HOST, "kernel_choice.cpp"),
           os.path.join(HOST, "flatten.cpp")]


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("scene_prepare") / "scene_prepare_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Wextra", "-o", exe] + SOURCES)
    run = subprocess.run([exe, os.path.join(HOST, "scene_prepare.cpp")], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr  # a failed check, or a sanitizer report
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    return run.stdout


def test_every_refusal_of_check_scene_has_a_row_and_refuses_as_stated(check_output):
    assert "refusals: 28 rows, 3 left out, 31 sites" in check_output, check_output


def test_prepared_layout_of_the_five_scenes(check_output):
    for name in ("first scene:", "with a quad:", "40 spheres:", "large mesh:", "large mesh, one height 1e-30:"):
        assert name in check_output, check_output


def test_every_kernel_choice_names_an_instantiated_kernel(check_output):
    assert "every key instantiated" in check_output and check_output.rstrip().endswith("ok"), check_output
