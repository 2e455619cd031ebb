"""Pass B of the DMR decoder in the both-slots mode, lane-parallel against burst-serial: builds tests/host_cpp/dmr_both_slots_test.cpp
(host code only, its own main) with the address and undefined-behaviour sanitizers and runs it.  What it checks is written at its head."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_both_passes_leave_the_same_in_the_mode(tmp_path):
    exe = str(tmp_path / "dmr_both_slots_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wno-unknown-pragmas",
                    "-Wno-unused-function", os.path.join(ROOT, "tests", "host_cpp", "dmr_both_slots_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(r.stdout)
    assert r.returncode == 0 and "dmr both slots: identical" in r.stdout, r.stdout
