"""Generate tests/golden/bptc_patterns_ref.npz (run in the development container only).

The REFERENCE's own bptc_196_96.c (compiled where it lies into oracle/_ref/libdigiham_ref_fec.so, oracle/Makefile target `ref`) on
the designed error patterns of tests/common.py: bptc_patterns -- every single bit, every pair, column and row triples, rectangles,
parity-row patterns, R(3), random weights 3..12.  Stored: the ok flags bit-packed, the twelve output bytes of every block the reference
accepts, and the generator's seed, N and a SHA-256 of the payloads it produced, so that a drifted generator fails loudly.

    python tests/golden/make_golden_bptc_patterns.py
    python tests/golden/make_golden_ref_compare.py      # takes the new file's digest into ref_compare_hashes.json
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import oracle as O          # noqa: E402
import common                           # noqa: E402


def main():
    O.build()
    assert O.ref() is not None, "build oracle/_ref first (make -C oracle)"
    payload, sent, cls = common.bptc_patterns(O)
    out, ok = O.bptc_196_96(payload, "ref")
    path = os.path.join(HERE, "bptc_patterns_ref.npz")
    np.savez_compressed(path, seed=np.int64(common.BPTC_PATTERN_SEED), n=np.int64(len(payload)),
                        payload_sha256=np.frombuffer(hashlib.sha256(payload.tobytes()).digest(), np.uint8),
                        class_counts=np.bincount(cls, minlength=len(common.BPTC_CLASSES)).astype(np.int64),
                        ok_bits=np.packbits(ok), out_ok=out[ok == 1])
    wrong = (ok == 1) & (out != sent).any(axis=1)
    print("%-18s %7s %7s %9s %9s" % ("class", "n", "ok", "ok wrong", "rejected"))
    for i, name in enumerate(common.BPTC_CLASSES):
        m = cls == i
        print("%-18s %7d %7d %9d %9d" % (name, m.sum(), (ok[m] == 1).sum(), wrong[m].sum(), (ok[m] == 0).sum()))
    o2, k2 = O.bptc_196_96(payload)
    print("oracle restatement agrees:", bool((k2 == ok).all() and (o2[ok == 1] == out[ok == 1]).all()))
    print("npz bytes:", os.path.getsize(path))


if __name__ == "__main__":
    main()
