"""The pass driver's decisions (pbrs_amd/csrc/host/pass_plan.cpp) run on the CPU: a stand-alone program (tests/pass_plan_check.cpp),
compiled once with AddressSanitizer and UndefinedBehaviorSanitizer, checks the path-state layout, the counter block, the pass size, the
bounce plan and the grids of a pass.  Nothing is loaded into python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "pbrs_amd", "csrc", "host")
SOURCES = [os.path.join(ROOT, "tests", "pass_plan_check.cpp"), os.path.join(HOST, "pass_plan.cpp")]


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pass_plan") / "pass_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Wextra", "-o", exe] + SOURCES)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr  # a failed check, or a sanitizer report
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    return run.stdout


def test_path_layout_is_aligned_ordered_and_the_size_it_always_was(check_output):
    assert "layout: 12 sizes, 22 columns, 295 bytes per path" in check_output, check_output


def test_counter_regions_tile_the_block_and_hold_every_bounce(check_output):
    assert "counters: 6 regions tile 50952 words, 64 bounces inside" in check_output, check_output


def test_pass_size_properties_and_the_rows_the_driver_answered_before(check_output):
    assert "pass size: 98010 grid points, 42 literal rows" in check_output, check_output


def test_bounce_plan_of_every_integrator_split_order_and_bounce(check_output):
    assert "bounce plan: 216 combinations, two choices each" in check_output, check_output


def test_pass_shape_is_what_the_driver_computed_inline(check_output):
    assert "shape: 5 sizes" in check_output and check_output.rstrip().endswith("ok"), check_output
