"""The host back ends of the band monitor's kernel bodies (step A, step B, the masked reset) under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/host_cpp/monitor_seams.cpp, a stand-alone program over one channel, 257 channels and
flags at the first and the last channel, every array an exact-size heap block.  CPU tier only; nothing is loaded into
this process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_monitor_bodies_are_clean_under_sanitizers(tmp_path):
    exe = str(tmp_path / "monitor_seams")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                    "-Wno-unknown-pragmas", "-Wno-unused-function", os.path.join(ROOT, "tests", "host_cpp", "monitor_seams.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and "monitor seams: clean" in r.stdout, r.stdout
