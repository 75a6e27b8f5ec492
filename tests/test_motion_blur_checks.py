"""check_motion_blur and pbrsm_motion_blur_params_default (pbrs_amd/csrc/host/arg_checks_motion_blur.cpp), the argument check and the
filler of pbrsm_motion_blur[_device], on the CPU: a stand-alone program (tests/motion_blur_check.cpp), compiled once with
AddressSanitizer and UndefinedBehaviorSanitizer, holds one row against every refusal site of the source and every boundary value's
refusing side, the accepted calls with every boundary value's accepting side, the filler's bytes and the order of the refusals.  Nothing
is loaded into python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "pbrs_amd", "csrc", "host")
SOURCES = [os.path.join(ROOT, "tests", "motion_blur_check.cpp"), os.path.join(HOST, "arg_checks_motion_blur.cpp")]


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("motion_blur") / "motion_blur_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Wextra", "-o", exe] + SOURCES)
    run = subprocess.run([exe, os.path.join(HOST, "arg_checks_motion_blur.cpp")], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr  # a failed check, or a sanitizer report
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    return run.stdout


def test_every_refusal_site_has_a_row_and_refuses_as_stated(check_output):
    assert "refusals: 37 rows, 10 sites" in check_output, check_output


def test_the_accepted_calls_the_defaults_and_the_fillers_bytes_pass(check_output):
    assert "accepted calls pass" in check_output, check_output


def test_the_refusals_come_in_the_stated_order(check_output):
    assert "precedence holds" in check_output and check_output.rstrip().endswith("ok"), check_output
