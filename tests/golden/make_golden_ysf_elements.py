"""Generate tests/golden/ysf_elements_ref.npz (run in the development container only).

V/D2 data-channel (DCH), header CSD and FICH codewords for tests/test_ysf_elements.py, which shows every one of them to
the product inside frames.  Every expected value comes from the REFERENCE's own functions: decode_trellis,
crc16_checksum and decode_whitening of oracle/_ref/libdigiham_ref_fec.so (src/ysf_decoder/{trellis,crc16,whitening}.c
compiled where they lie) called in the order of ysf_phase.cpp:258-267 (DCH) and :323-346 (CSD), and Fich::parse of
oracle/_ref/libdigiham_ref_ysf.so -- never from the oracle or from digiham_amd/synth.py; synth only builds inputs.

`*_in` are dibits in CODEWORD order, one per byte; the test applies the frame's interleave when it places them.
`*_src` names the class of a vector (SRC below):

* clean codewords (32 DCH payloads, 8 CSD payloads, 48 FICH words, all distinct; the singles and pairs are made from them, so a
  result that lands in the wrong frame shows);
* one wrong dibit in each of the three patterns (bit 1, bit 0, both) -- DCH and FICH: at every position 0..99, both sides
  of the product's lane-local repair window 16..88 (decoder_core.hpp, dh_ysf_clean100); CSD: at every third position plus
  the first and last eight;
* two wrong dibits 1..8 apart whose syndrome is none of the three single patterns (the product must hand them to its
  Viterbi decoder), some straddling positions 16 and 88;
* k flipped bits (DCH k = 2..24, CSD k = 2..40);
* random dibits.

`*_sent` holds the encoder's payload (zeros for random vectors), `*_metric` the reference's path metric.

    python tests/golden/make_golden_ysf_elements.py
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
PATTERNS = (2, 1, 3)                    # wrong bit 1, wrong bit 0, both


def pack_dibits(d):
    """[n][len] dibits -> bytes, four to a byte, first on top (ysf_phase.cpp:103-106 / :323-333)"""
    d = np.asarray(d, np.uint8)
    bits = np.stack([d >> 1, d & 1], axis=-1).reshape(len(d), -1)
    return np.packbits(bits, axis=1)


def syndrome(d):
    """parity checks t = 4 .. len-1 of the rate-1/2 code G1 = 1 + D^3 + D^4 (bit 0), G2 = 1 + D + D^2 + D^4 (bit 1) as a set of t"""
    h, l = [int(x) >> 1 for x in d], [int(x) & 1 for x in d]
    return {t for t in range(4, len(d)) if h[t] ^ h[t - 1] ^ h[t - 2] ^ h[t - 4] ^ l[t] ^ l[t - 3] ^ l[t - 4]}


def is_single_pattern(syn):
    """the syndrome of exactly one wrong dibit well inside the block: bit 1 -> t0 + {0, 1, 2, 4}, bit 0 -> t0 + {0, 3, 4},
    both -> t0 + {0, 1, 2}"""
    if not syn:
        return False
    t0 = min(syn)
    return {t - t0 for t in syn} in ({0, 1, 2, 4}, {0, 3, 4}, {0, 1, 2})


def flip(d, rng, k):
    d = d.copy()
    for bp in rng.choice(2 * len(d), k, replace=False):
        d[bp // 2] ^= 2 >> (bp % 2)
    return d


def reference_dch(d, nbytes):
    """ysf_phase.cpp:258-267 (nbytes = 10) / :335-346 (20) with the reference's functions -> ok, payload, metric"""
    n = d.shape[1]
    w, metric = O.trellis(pack_dibits(d), n, "ref")
    check = O.crc16(w, nbytes, "ref")
    ok = (check == (w[:, nbytes].astype(np.uint16) << 8 | w[:, nbytes + 1])).astype(np.uint8)
    out = O.whitening(w, 100 if nbytes == 10 else 160, "ref")[:, :nbytes].copy()
    out[ok == 0] = 0
    return ok, out, metric


def singles(codewords, positions):
    rows = []
    for j, p in enumerate(positions):
        for w in PATTERNS:
            d, sent = codewords[j % len(codewords)]
            e = d.copy(); e[p] ^= w
            rows.append((e, sent, SRC["single"], p, w))
    return rows


def single_columns(rows):
    """position and pattern of the wrong dibit of a single (-1, 0 for the other classes)"""
    return {"pos": np.array([r[3] if len(r) > 3 else -1 for r in rows], np.int16),
            "pat": np.array([r[4] if len(r) > 3 else 0 for r in rows], np.uint8)}


def pairs(codewords, rng, per_dist, edges):
    """two wrong dibits 1..8 apart, none with the syndrome of a single; `edges`: for each, one pair per distance has a wrong
    dibit below it and one at or above it"""
    rows, k = [], 0
    n = len(codewords[0][0])
    for dist in range(1, 9):
        starts = [e - 1 - (dist - 1) // 2 for e in edges] + list(rng.choice(n - dist, per_dist, replace=False))
        for p in starts:
            d, sent = codewords[k % len(codewords)]; k += 1
            for _ in range(20):
                e = d.copy(); e[p] ^= rng.integers(1, 4); e[p + dist] ^= rng.integers(1, 4)
                syn = syndrome(e)
                if syn and not is_single_pattern(syn):
                    rows.append((e, sent, SRC["pair"]))
                    break
    return rows


def dch_vectors(rng, nbytes, n_clean, single_positions, ks, per_k, n_random):
    n = 100 if nbytes == 10 else 180

    def codeword():
        sent = rng.integers(0, 256, nbytes).astype(np.uint8)
        return np.array(synth._ysf_dch_code(bytes(sent.tolist()), nbytes), np.uint8), sent

    cws = [codeword() for _ in range(n_clean)]
    rows = [(d, sent, SRC["clean"]) for d, sent in cws]
    rows += singles(cws, single_positions)
    rows += pairs(cws, rng, 10, (16, 89) if n == 100 else (16, 169))
    for k in ks:
        for _ in range(per_k):
            d, sent = codeword()
            rows.append((flip(d, rng, k), sent, SRC["flips"]))
    rows += [(x, np.zeros(nbytes, np.uint8), SRC["random"]) for x in rng.integers(0, 4, (n_random, n), dtype=np.uint8)]
    d = np.stack([r[0] for r in rows]).astype(np.uint8)
    assert d.shape[1] == n
    ok, out, metric = reference_dch(d, nbytes)
    return {"in": d, "ok": ok, "out": out, "metric": metric, "src": np.array([r[2] for r in rows], np.uint8),
            "sent": np.stack([r[1] for r in rows]).astype(np.uint8), **single_columns(rows)}


def fich_vectors(rng):
    """communication-channel V/D2 FICHs, all words distinct (the frame number cycles 0..7, frame total and the spare bits vary): clean, every
    single, pairs; what Fich::parse gives for them on the air (fich.cpp:12-52)"""
    words = []
    while len(words) < 48:
        w = (1 << 30) | (int(rng.integers(0, 64)) << 22) | ((len(words) & 7) << 19) | (int(rng.integers(0, 8)) << 16) | \
            (int(rng.integers(0, 64)) << 10) | (2 << 8) | int(rng.integers(0, 256))
        if w not in words:
            words.append(w)
    cws = [(np.array(synth._ysf_fich_code(w), np.uint8), w) for w in words]
    rows = [(d, w, SRC["clean"]) for d, w in cws]
    rows += singles(cws, range(100))
    rows += pairs(cws, rng, 6, (16, 89))
    d = np.stack([r[0] for r in rows]).astype(np.uint8)
    air = np.stack([synth.ysf_fich_interleave(list(x)) for x in d]).astype(np.uint8)
    out, data = O.Elements("ref").ysf_fich(air)
    return {"in": d, "ok": out[:, 0].copy(), "data": data, "src": np.array([r[2] for r in rows], np.uint8),
            "sent": np.array([r[1] for r in rows], np.uint32), **single_columns(rows)}


def hard_single(v, name):
    """The singles the reference's decoder does NOT repair (measured on 40 codewords of each length: always these, never
    another): both bits of dibit n - 5 wrong -- rejected for every codeword --, and both bits of dibit 4 or 5 wrong --
    rejected for about half of the codewords.  trellis.c starts every state at metric 0 and takes the best end state, so a
    wrong dibit that close to either end ties with a path from another start state / into another end state."""
    n = len(v[name + "_in"][0])
    return (v[name + "_pat"] == 3) & np.isin(v[name + "_pos"], (4, 5, n - 5))


def check(v):
    """the conditions tests/test_ysf_elements.py asserts again; prints the counts of DESIGN.md"""
    for name in ("dch", "csd"):
        ok, src = v[name + "_ok"] == 1, v[name + "_src"]
        same = (v[name + "_out"] == v[name + "_sent"]).all(axis=1)
        late = src >= 2
        print("%s: %d vectors; per class %s; accepted per class %s; classes 2-4: %d accepted, %d rejected; accepted with another payload %d" % (
            name, len(ok), [int((src == c).sum()) for c in range(5)], [int((ok & (src == c)).sum()) for c in range(5)],
            (ok & late).sum(), (~ok & late).sum(), (ok & ~same & (src < 4)).sum()))
        assert (ok & late).sum() >= 100 and (~ok & late).sum() >= 100
        assert (ok & same)[(src <= 1) & ~hard_single(v, name)].all() and not ok[(v[name + "_pos"] == len(v[name + "_in"][0]) - 5) & (v[name + "_pat"] == 3)].any()
        assert sorted(set(src)) == [0, 1, 2, 3, 4]
        for d in v[name + "_in"][src == 2]:
            assert syndrome(d) and not is_single_pattern(syndrome(d))
    ok, src = v["fichx_ok"] == 1, v["fichx_src"]
    print("fich: %d vectors; per class %s; accepted per class %s" % (len(ok), [int((src == c).sum()) for c in range(3)], [int((ok & (src == c)).sum()) for c in range(3)]))
    assert (ok & (v["fichx_data"] == v["fichx_sent"]))[src <= 1].all() and sorted(set(src)) == [0, 1, 2]


def main():
    O.build()
    assert O.ref() is not None and O.ref_lib("ysf") is not None, "build oracle/_ref first (make -C oracle)"
    rng = np.random.default_rng(20261019)
    v = {}
    for k, a in dch_vectors(rng, 10, 32, range(100), range(2, 25), 12, 60).items():
        v["dch_" + k] = a
    csd_pos = sorted(set(range(0, 180, 3)) | set(range(8)) | set(range(172, 180)))
    for k, a in dch_vectors(rng, 20, 8, csd_pos, range(2, 41), 8, 60).items():
        v["csd_" + k] = a
    for k, a in fich_vectors(rng).items():
        v["fichx_" + k] = a
    check(v)
    path = os.path.join(OUT, "ysf_elements_ref.npz")
    np.savez_compressed(path, **v)
    assert os.path.getsize(path) < 300 * 1024
    from common import npz_digest
    print("%d bytes; ref_compare_hashes.json \"ysf_elements_ref_npz\": \"%s\"" % (os.path.getsize(path), npz_digest(path)))


if __name__ == "__main__":
    main()
