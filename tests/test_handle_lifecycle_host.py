"""The five handles behind the C ABI under AddressSanitizer, UndefinedBehaviorSanitizer and leak detection:
tests/host_cpp/handle_lifecycle.cpp, a stand-alone program over the CPU backend -- create and destroy, every class of
invalid configuration, a null handle into every entry point, and create with the k-th backend allocation failing for
every k, which is where a partly built handle (the monitor's engines and ring above all) has to let go of everything.
CPU tier only; nothing is loaded into this process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_handle_lifecycle_is_clean_under_sanitizers(tmp_path):
    exe = str(tmp_path / "handle_lifecycle")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                    "-Wno-unknown-pragmas", "-Wno-unused-function", "-Wno-subobject-linkage",
                    os.path.join(ROOT, "tests", "host_cpp", "handle_lifecycle.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "handle lifecycle: clean" in r.stdout, r.stdout
