"""The device / CPU seam of the kernel bodies (dh_portable.hpp, "THE SEAM") as a text scan, no compiler:

* the token __HIP_DEVICE_COMPILE__ occurs in digiham_amd/csrc only in the layer (dh_portable.hpp, wave_ops.hpp) and in engine.hip;
* in the core headers every #if / #ifdef / #elif that mentions DH_ON_GPU or DH_DEVICE_BUILD stands at namespace scope: the
  algorithm bodies carry no build conditional, only whole pairs of a hand-scheduled piece and its restatement do.
"""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "digiham_amd", "csrc")
LAYER = ("dh_portable.hpp", "wave_ops.hpp")
CORE = tuple(sorted(f for f in os.listdir(CSRC) if f.endswith("_core.hpp")))      # all eleven; what is left of DH_DEVICE_BUILD in them stands at namespace scope, around a CPU restatement


def _code_lines(text):
    """(line number, line with comments, string and character literals blanked) for every line"""
    text = re.sub(r"/\*.*?\*/", lambda m: re.sub(r"[^\n]", " ", m.group(0)), text, flags=re.S)
    out = []
    for no, line in enumerate(text.split("\n"), 1):
        line = re.sub(r'"(\\.|[^"\\])*"', '""', line)
        line = re.sub(r"'(\\.|[^'\\])'", "' '", line)
        out.append((no, line.split("//")[0]))
    return out


def test_device_compile_token_only_in_the_layer():
    for name in sorted(os.listdir(CSRC)):
        if name in LAYER or name == "engine.hip":
            continue
        assert "__HIP_DEVICE_COMPILE__" not in open(os.path.join(CSRC, name)).read(), name
    assert "__HIP_DEVICE_COMPILE__" in open(os.path.join(CSRC, "dh_portable.hpp")).read()     # (the scan looks at the right place)


def test_build_conditionals_of_the_core_headers_stand_at_namespace_scope():
    seen = 0
    for name in CORE:
        depth, else_depths, continued = 0, [], False
        for no, line in _code_lines(open(os.path.join(CSRC, name)).read()):
            if continued:                                  # the rest of a multi-line macro definition
                continued = line.rstrip().endswith("\\")
                continue
            continued = bool(re.match(r"\s*#", line)) and line.rstrip().endswith("\\")
            d = re.match(r"\s*#\s*(if|ifdef|ifndef|elif|else|endif)\b(.*)", line)
            if d:
                kind, cond = d.group(1), d.group(2)
                if kind in ("if", "ifdef", "ifndef", "elif") and re.search(r"\bDH_ON_GPU\b|\bDH_DEVICE_BUILD\b", cond):
                    assert depth == 0, "%s:%d: a build conditional inside a body (brace depth %d): add a primitive to the layer instead" % (name, no, depth)
                    seen += 1
                # both branches of a conditional start from the same depth
                if kind in ("if", "ifdef", "ifndef"):
                    else_depths.append(depth)
                elif kind in ("elif", "else"):
                    depth = else_depths[-1]
                else:
                    else_depths.pop()
                continue
            if re.match(r"\s*#", line):
                continue                                   # (macro bodies: their braces balance on their own lines or not at all)
            depth += line.count("{") - line.count("}")
            assert depth >= 0, "%s:%d: unbalanced braces" % (name, no)
        assert depth == 0 and not else_depths, name
    assert seen >= 5          # dh_fir_lane, dh_fir_mfma, dh_fir_f16, dh_agc_scan, the Viterbi pass, the D-Star ACS
