"""check_temporal_clip (pbrs_amd/csrc/host/arg_checks_clip.cpp), the argument check of pbrs_temporal_accumulate_clip[_device], on the
CPU: a stand-alone program (tests/history_clip_check.cpp), compiled once with AddressSanitizer and UndefinedBehaviorSanitizer, holds
one row against every refusal site of the source, the accepted calls and the order of the refusals.  Nothing is loaded into python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "pbrs_amd", "csrc", "host")
SOURCES = [os.path.join(ROOT, "tests", "history_clip_check.cpp"), os.path.join(HOST, "arg_checks_clip.cpp"), os.path.join(HOST, "arg_checks.cpp")]


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("history_clip") / "history_clip_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Wextra", "-o", exe] + SOURCES)
    run = subprocess.run([exe, os.path.join(HOST, "arg_checks_clip.cpp")], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr  # a failed check, or a sanitizer report
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    return run.stdout


def test_every_refusal_site_has_a_row_and_refuses_as_stated(check_output):
    assert "refusals: 9 rows, 5 sites" in check_output, check_output


def test_the_accepted_calls_pass(check_output):
    assert "accepted calls pass" in check_output, check_output


def test_the_motion_calls_refusal_wins_and_a_null_clip_is_the_motion_call(check_output):
    assert "precedence holds" in check_output and check_output.rstrip().endswith("ok"), check_output
