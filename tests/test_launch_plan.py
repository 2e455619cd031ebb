"""The routing both backends share (digiham_amd/csrc/launch_plan.hpp).

One chained launch and two separate launches give the same bytes, so no output test can tell which route a push took: a
backend that loses a route still passes them all.  tests/host_cpp/plan_test.cpp asks the plan itself, for every
configuration an engine can hand to a backend, and compares with a table written out by hand; it also checks the grammar
of DH_TAIL_SPLIT, the parameters of a split launch and the tail split's locator, part bounds and flag word
(digiham_amd/csrc/chain_core.hpp), which the device backend and the wave emulation take from the same headers.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_routes_match_the_literal_table(tmp_path):
    exe = str(tmp_path / "plan_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host_cpp", "plan_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    routes, failures = int(r.stdout.split()[0]), int(r.stdout.split()[3])
    assert failures == 0 and routes > 2000, r.stdout
