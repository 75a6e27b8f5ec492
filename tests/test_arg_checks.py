"""The argument checks of the render and image-space entry points (pbrs_amd/csrc/host/arg_checks.cpp) run on the CPU: a stand-alone
program (tests/arg_checks_check.cpp), compiled once with AddressSanitizer and UndefinedBehaviorSanitizer, holds one row against every
refusal site of the source, the valid baselines and the order of the refusals.  Nothing is loaded into python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "pbrs_amd", "csrc", "host")
SOURCES = [os.path.join(ROOT, "tests", "arg_checks_check.cpp"), os.path.join(HOST, "arg_checks.cpp")]


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("arg_checks") / "arg_checks_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Wextra", "-o", exe] + SOURCES)
    run = subprocess.run([exe, os.path.join(HOST, "arg_checks.cpp")], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr  # a failed check, or a sanitizer report
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    return run.stdout


def test_every_refusal_site_has_a_row_and_refuses_as_stated(check_output):
    assert "refusals: 80 rows, 80 sites, 12 checks" in check_output, check_output


def test_the_valid_baselines_pass_with_and_without_the_optional_arguments(check_output):
    assert "baselines accepted" in check_output, check_output


def test_the_earlier_refusal_wins(check_output):
    assert "precedence holds" in check_output and check_output.rstrip().endswith("ok"), check_output
