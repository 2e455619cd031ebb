"""The host back ends of steps A and C of the band monitor (the `opened` word, naming on close) under AddressSanitizer
and UndefinedBehaviorSanitizer: tests/host_cpp/monitor_close_seams.cpp, a stand-alone program over one channel and 257
channels, closing channels at the first and the last index, a front end that is not configured, every array an
exact-size heap block.  CPU tier only; nothing is loaded into this process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_close_bodies_are_clean_under_sanitizers(tmp_path):
    exe = str(tmp_path / "monitor_close_seams")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                    "-Wno-unknown-pragmas", "-Wno-unused-function", os.path.join(ROOT, "tests", "host_cpp", "monitor_close_seams.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and "monitor close seams: clean" in r.stdout, r.stdout
