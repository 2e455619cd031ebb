"""Generate tests/golden/nxdn_elements_ref.npz (run in the development container only).

SACCH, FACCH1 and filler vectors for tests/test_nxdn_elements.py, which shows every one of them to the product inside
frames.  Every expected value comes from the REFERENCE's own classes (oracle/_ref/libdigiham_ref_nxdn.so =
src/nxdn_decoder/{scrambler,lich,sacch,facch1,trellis}.cpp compiled where they lie, called through oracle/ref_nxdn.cpp),
never from the oracle or from digiham_amd/synth.py; synth only builds inputs.  Inputs are descrambled dibits, as in
nxdn_ref.npz.

The reference's channel decoder counts punctured bits as received zeros, starts every state at metric 0 with a
start-state rule for the first four steps, and takes the lowest best end state: it rejects two clean FACCH1 blocks in
three and miscorrects often (NXDN).  The vectors are chosen so that its tie rules decide:

* one wrong dibit at every position x the three wrong values, and pairs of wrong dibits at distances 1..12, on clean
  codewords the reference accepts;
* k random bit flips (SACCH k = 0..8, FACCH1 k = 0..7 weighted to 0..4) from pools, classified by the reference into
  accepted with the clean payload / accepted with ANOTHER payload (a miscorrection that passes the CRC) / rejected,
  and drawn by quota so both outcomes and the miscorrections are plentiful;
* random SACCH blocks, pre-filtered: the ones whose CRC-6 the reference passes and as many it rejects;
* no accepted FACCH1 with message type TX_RELEASE (it would end the frame grid of an element stream);
* filler blocks (random, rejected by the reference) for the positions a test does not look at.

`*_src` names the class of a vector (SRC below); `*_clean` holds the encoder's own bits for vectors made from a
codeword (`*_has_clean`), so the miscorrections can be counted.

    python tests/golden/make_golden_nxdn_elements.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import oracle as O          # noqa: E402
from digiham_amd import synth           # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
SRC = {"clean": 0, "single": 1, "pair": 2, "flips": 3, "random": 4}
TX_RELEASE = 0x08


def pack_bits(bits, nbytes):
    b = list(bits) + [0] * (8 * nbytes - len(bits))
    return np.packbits(np.array(b, np.uint8))


def sacch_codeword(rng):
    info = synth._bits_of(int(rng.integers(0, 4)), 2) + synth._bits_of(int(rng.integers(0, 64)), 6) + [int(x) for x in rng.integers(0, 2, 18)]
    crc = synth._nxdn_crc(info, 6, 0x3F, 0x13)
    d = synth._nxdn_channel_encode(info, crc, lambda i: (i + 1) % 6 == 0, 12, 5)
    return np.array(d, np.uint8), pack_bits(info + crc, 5)


def facch1_codeword(rng):
    info = [int(x) for x in rng.integers(0, 2, 80)]
    crc = synth._nxdn_crc(info, 12, 0xFFF, 0x407)
    d = synth._nxdn_channel_encode(info, crc, lambda i: (i - 1) % 4 == 0, 16, 9)
    return np.array(d, np.uint8), pack_bits(info + crc, 12)


def accepted_clean(make, parse, rng, not_release=False):
    """a codeword whose unflipped block the reference accepts with the encoder's payload (search over the random bits)"""
    while True:
        d, clean = make(rng)
        ok, out = parse(d, "ref")
        if ok and (out == clean).all() and not (not_release and (out[0] & 0x3F) == TX_RELEASE):
            return d, clean


def flip(d, rng, k):
    d = d.copy()
    for bp in rng.choice(2 * len(d), k, replace=False):
        d[bp // 2] ^= 2 >> (bp % 2)
    return d


class Vectors:
    def __init__(self, n, nbytes, parse):
        self.n, self.nbytes, self.parse = n, nbytes, parse
        self.rows = []

    def classify(self, d, clean):
        ok, out = self.parse(d, "ref")
        if ok and self.n == 72 and (out[0] & 0x3F) == TX_RELEASE:
            return None
        return "rej" if not ok else "same" if clean is not None and (out == clean).all() else "other"

    def add(self, d, clean, src):
        c = self.classify(d, clean)
        if c is not None:
            self.rows.append((d, clean, SRC[src]))
        return c

    def errors(self, codewords, rng, pair_starts):
        for d, clean in codewords:
            self.add(d, clean, "clean")
            for p in range(self.n):
                for w in (1, 2, 3):
                    e = d.copy(); e[p] ^= w
                    self.add(e, clean, "single")
            for dist in range(1, 13):
                for p in rng.choice(self.n - dist, pair_starts, replace=False):
                    e = d.copy(); e[p] ^= rng.integers(1, 4); e[p + dist] ^= rng.integers(1, 4)
                    self.add(e, clean, "pair")

    def flips(self, make, rng, pool_per_k, quota, not_release=False):
        """quota = {class: n}: pools of flipped codewords per k, classified by the reference, drawn round-robin over k"""
        pools = {c: [] for c in quota}
        for k, npool in enumerate(pool_per_k):
            per = {c: [] for c in quota}
            for _ in range(npool):
                d, clean = accepted_clean(make, self.parse, rng, not_release)
                e = flip(d, rng, k)
                c = self.classify(e, clean)
                if c is not None:
                    per[c].append((e, clean))
            for c in quota:
                pools[c].append(per[c])
        for c, want in quota.items():
            got, i = 0, 0
            while got < want and any(pools[c]):
                lst = pools[c][i % len(pools[c])]
                i += 1
                if lst:
                    self.rows.append(lst.pop() + (SRC["flips"],))
                    got += 1
            assert got == want, (c, got, want)

    def arrays(self, name):
        d = np.stack([r[0] for r in self.rows]).astype(np.uint8)
        res = [self.parse(x, "ref") for x in d]
        has = np.array([r[1] is not None for r in self.rows], np.uint8)
        clean = np.stack([r[1] if r[1] is not None else np.zeros(self.nbytes, np.uint8) for r in self.rows])
        return {name + "_in": d, name + "_ok": np.array([ok for ok, _ in res], np.uint8),
                name + "_out": np.stack([o if ok else np.zeros(self.nbytes, np.uint8) for ok, o in res]),
                name + "_src": np.array([r[2] for r in self.rows], np.uint8), name + "_has_clean": has, name + "_clean": clean}


def check(v):
    """the conditions tests/test_nxdn_elements.py asserts again"""
    for name, n_each, n_mis in (("sacch", 500, 100), ("facch1", 300, 30)):
        ok = v[name + "_ok"] == 1
        mis = ok & (v[name + "_has_clean"] == 1) & (v[name + "_out"] != v[name + "_clean"]).any(axis=1)
        print("%s: %d vectors, %d accepted, %d rejected, %d accepted with another payload" % (name, len(ok), ok.sum(), (~ok).sum(), mis.sum()))
        assert ok.sum() >= n_each and (~ok).sum() >= n_each and mis.sum() >= n_mis
    assert not ((v["facch1_ok"] == 1) & ((v["facch1_out"][:, 0] & 0x3F) == TX_RELEASE)).any()
    assert not v["filler_facch1_ok"].any() and not v["filler_sacch_ok"].any()


def main():
    assert O.ref_nxdn() is not None, "build oracle/_ref first (make -C oracle)"
    rng = np.random.default_rng(20261018)
    S = Vectors(30, 5, O.nxdn_sacch)
    S.errors([accepted_clean(sacch_codeword, O.nxdn_sacch, rng) for _ in range(2)], rng, 2)
    S.flips(sacch_codeword, rng, [30, 150, 250, 300, 400, 500, 500, 400, 300], {"same": 150, "other": 110, "rej": 230})
    rnd = rng.integers(0, 4, (20000, 30), dtype=np.uint8)
    ok = np.array([O.nxdn_sacch(x, "ref")[0] for x in rnd])
    n_rnd = min(int(ok.sum()), 280)
    for x in list(rnd[ok][:n_rnd]) + list(rnd[~ok][:n_rnd]):
        S.add(x, None, "random")
    F = Vectors(72, 12, O.nxdn_facch1)
    F.errors([accepted_clean(facch1_codeword, O.nxdn_facch1, rng, True) for _ in range(2)], rng, 2)
    F.flips(facch1_codeword, rng, [60, 1200, 1500, 1500, 1500, 900, 900, 900], {"same": 170, "other": 40, "rej": 170}, True)
    v = {}
    v.update(S.arrays("sacch")); v.update(F.arrays("facch1"))
    for name, n, parse in (("filler_sacch", 30, O.nxdn_sacch), ("filler_facch1", 72, O.nxdn_facch1)):
        blocks = [x for x in rng.integers(0, 4, (64, n), dtype=np.uint8) if not parse(x, "ref")[0]][:8]
        v[name + "_in"] = np.stack(blocks)
        v[name + "_ok"] = np.array([parse(x, "ref")[0] for x in blocks], np.uint8)
    check(v)
    path = os.path.join(OUT, "nxdn_elements_ref.npz")
    np.savez_compressed(path, **v)
    assert os.path.getsize(path) < 300 * 1024
    from common import npz_digest
    print("%d bytes; ref_compare_hashes.json \"nxdn_elements_ref_npz\": \"%s\"" % (os.path.getsize(path), npz_digest(path)))
    clean_acceptance(rng)


def clean_acceptance(rng, n=400):
    """The figures of DESIGN.md (NXDN, "the reference's channel decoder on clean input"): of n random blocks with k flipped
    bits, how many pass the reference's CRC / how many of those carry the encoder's payload; and, for clean FACCH1 blocks,
    the reference's path metric against the number of ones among the punctured bits (= the metric of the encoder's path)."""
    for name, make, parse in (("FACCH1", facch1_codeword, O.nxdn_facch1), ("SACCH", sacch_codeword, O.nxdn_sacch)):
        cells = []
        for k in range(9):
            acc = same = 0
            for _ in range(n):
                d, clean = make(rng)
                ok, out = parse(flip(d, rng, k), "ref")
                acc += ok; same += bool(ok and (out == clean).all())
            cells.append("%d/%d" % (acc, same))
        print("| %s | %s |" % (name, " | ".join(cells)))
    below = 0
    for _ in range(n):
        info = [int(x) for x in rng.integers(0, 2, 80)]
        bits = info + synth._nxdn_crc(info, 12, 0xFFF, 0x407) + [0, 0, 0, 0]
        coded = [b for d in synth.trellis_encode_bits(bits) for b in ((d >> 1) & 1, d & 1)]
        own = sum(b for i, b in enumerate(coded) if (i - 1) % 4 == 0)          # the encoder's path: only the punctured ones differ
        received = [0 if (i - 1) % 4 == 0 else b for i, b in enumerate(coded)]
        _, metric = O.nxdn_trellis(np.packbits(np.array(received, np.uint8)), 192, "ref")
        below += metric < own
    print("clean FACCH1: the reference's best path has a smaller metric than the encoder's own in %d of %d blocks" % (below, n))


if __name__ == "__main__":
    main()
