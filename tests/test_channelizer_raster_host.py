"""The channelizer's host handle under AddressSanitizer, UndefinedBehaviorSanitizer and leak detection:
tests/host_cpp/raster_lifecycle.cpp, a stand-alone program over the CPU backend -- the raster's invalid configurations with
nothing allocated, a configuration of the older struct size whose heap block ends where that struct ends, and for each of
the three kinds of bank (fixed offsets, rational rate, raster) create with the k-th backend allocation failing for every k
and ragged pushes with a retune and a reset in both output modes, where every window, fold-buffer and output index is the
sanitizer's to check; then the one slot of dh_cz_plan_rat at L = 1 against a fixed bank's position formulas, past 2^32
included.  CPU tier only; nothing is loaded into this process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_raster_lifecycle_is_clean_under_sanitizers(tmp_path):
    exe = str(tmp_path / "raster_lifecycle")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                    "-Wno-unknown-pragmas", "-Wno-unused-function", "-Wno-subobject-linkage",
                    os.path.join(ROOT, "tests", "host_cpp", "raster_lifecycle.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "raster lifecycle: clean" in r.stdout, r.stdout
