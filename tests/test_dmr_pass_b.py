"""Pass B of the frame-parallel DMR decoder, lane-parallel (dh_dmr_pass_b_lanes) against burst-serial (dh_dmr_pass_b).

* tests/host_cpp/dmr_pass_b_test.cpp feeds identical chunks to both passes and compares all they leave, bit for bit (CPU tier).
* Engines on both tiers -- a decoder-only engine fed dibits in pushes of 63, 64, 65, 128, 129 bursts and ragged pushes, and the
  rrc -> gfsk -> dmr chain in pushes of 63 bursts -- on one-slot and two-slot streams of 4 channels, noise-free and with three wrong
  dibits in every burst: dibits, frames and events equal the oracle's AND the same engine's with DH_DMR_SCALAR_PASS_B=1.
* So that the serial fallback cannot hide a failure: on the noise-free streams the only chunk of a channel that takes the serial pass is
  the one entered from the sync search (slot still unknown); every other chunk, full or not, is counted as lane-parallel.  That the
  streams of the seeds below hold no irregular burst behind that chunk is checked on the serial machine's own events first: every burst
  on the grid carries a SYNC or an EMB event and no reset event follows the first burst.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

from common import assert_matches_oracle, run_engine
from dec_harness import assert_rows, run_dmr_pass_b
from digiham_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (611, 612, 613, 614)             # regular behind their first chunk (test_seeds_are_regular_for_the_serial_machine)
NB = 400                                 # bursts per stream: three pushes of 129
EV_SYNC, EV_SLOT_RESET, EV_META_RESET, EV_EMB = 1, 2, 3, 8


def test_both_passes_leave_the_same(tmp_path):
    exe = str(tmp_path / "dmr_pass_b_test")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wno-unknown-pragmas", "-Wno-unused-function",
                    os.path.join(ROOT, "tests", "host_cpp", "dmr_pass_b_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and "dmr pass b: identical" in r.stdout, r.stdout


@functools.lru_cache(maxsize=None)
def dibits(two_slots, noisy, nb=NB):
    rows = []
    for seed in SEEDS:
        s = synth.dmr_stream(seed, nb, two_slots=two_slots).copy()
        if noisy:                        # three wrong dibits in every burst, whatever it carries (voice, LC header, terminator, idle)
            rng = np.random.default_rng(seed + 1000)
            lead = len(s) - 144 * nb
            for i in range(nb):
                at = lead + 144 * i + rng.choice(144, 3, replace=False)
                s[at] ^= rng.integers(1, 4, 3).astype(np.uint8)
        rows.append(s)
    n = min(len(r) for r in rows)
    return np.stack([r[:n] for r in rows])


@functools.lru_cache(maxsize=None)
def decoded(two_slots, noisy):
    from oracle import oracle as O
    O.build()
    return [O.Decoder("dmr").process(row) for row in dibits(two_slots, noisy)]


def push_plan(kind, n):
    if kind == "ragged":
        rng = np.random.default_rng(5)
        cuts = []
        while sum(cuts) < n:
            cuts.append(int(rng.choice([145, 1000, 144 * 64 - 7, 144 * 64 + 1, 144 * 70, 144 * 130 + 77, 9])))
        return cuts
    return [144 * kind] * (n // (144 * kind) + 1)


@pytest.mark.parametrize("two_slots", [False, True])
def test_seeds_are_regular_for_the_serial_machine(emu_ctx, two_slots):
    """The noise-free streams as the burst-serial pass sees them: one SYNC or EMB event for every burst on the grid, the only reset
    events at the very first burst (the TACT that tells the slot).  Seeds that fail here cannot carry the counter conditions below."""
    syms = dibits(two_slots, False)
    run, counts = run_dmr_pass_b(emu_ctx, syms, [syms.shape[1]], True)
    assert counts[:, 0].sum() == 0                            # the switch holds: no chunk went lane-parallel
    for b, ev in enumerate(run.events):
        first = int(ev["sym_index"][0])
        burst = (ev["sym_index"].astype(np.int64) - first) // 144
        assert ((ev["sym_index"] - first) % 144 == 0).all()
        carrying = np.unique(burst[(ev["type"] == EV_SYNC) | (ev["type"] == EV_EMB)])
        assert len(carrying) == burst.max() + 1 >= NB - 2, (SEEDS[b], "a burst without sync and EMB")
        resets = burst[(ev["type"] == EV_SLOT_RESET) | (ev["type"] == EV_META_RESET)]
        assert (resets == 0).all(), (SEEDS[b], "reset behind the first burst")


@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("two_slots", [False, True])
def test_decoder_only_engine(ctx, two_slots, noisy):
    syms = dibits(two_slots, noisy)
    want = decoded(two_slots, noisy)
    fell_back = 0
    for kind in (63, 64, 65, 128, 129, "ragged"):
        cuts = push_plan(kind, syms.shape[1])
        got, counts = run_dmr_pass_b(ctx, syms, cuts, False)
        forced, forced_counts = run_dmr_pass_b(ctx, syms, cuts, True)
        assert_rows(got, want, ["pushes of %s, seed %d, against the oracle" % (kind, s) for s in SEEDS])
        assert_rows(forced, got.results, ["pushes of %s, seed %d, the serial pass against the lane-parallel" % (kind, s) for s in SEEDS])
        assert forced_counts[:, 0].sum() == 0
        lanes, scalar = counts.sum(axis=0)
        assert (lanes + scalar == forced_counts[:, 1].sum(axis=0)).all()       # the same chunks either way
        if noisy:
            assert (lanes > 0).all()
            fell_back += int(scalar.sum()) - len(SEEDS)
        else:
            assert (scalar == 1).all(), (kind, scalar)         # the chunk behind the sync search; every other chunk lane-parallel
            assert (counts[0, 1] == 1).all()                   # ... which is the first chunk of the first push
            assert (lanes >= syms.shape[1] // (144 * 64)).all()
    if noisy:
        assert fell_back > 0                                   # the wrong dibits did make irregular chunks, and those agree as well


@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("two_slots", [False, True])
def test_chain(ctx, oracle, two_slots, noisy, monkeypatch):
    """rrc -> gfsk -> dmr in pushes of 63 bursts (the shortest of the list: the slicer's share of the test's time)."""
    syms = dibits(two_slots, noisy, 130)
    x = np.stack([synth.shape(row) for row in syms]).astype(np.float32)
    ref = oracle.chain(x, proto=1)
    monkeypatch.delenv("DH_DMR_SCALAR_PASS_B", raising=False)
    res = run_engine(ctx, x, "dmr", [63 * 1440])
    assert_matches_oracle(res, ref, len(SEEDS), "lane-parallel")
    monkeypatch.setenv("DH_DMR_SCALAR_PASS_B", "1")
    forced = run_engine(ctx, x, "dmr", [63 * 1440])
    assert_matches_oracle(forced, ref, len(SEEDS), "serial")
    for b in range(len(SEEDS)):
        assert res["frames"][b].tobytes() == forced["frames"][b].tobytes() and res["events"][b].tobytes() == forced["events"][b].tobytes()
    assert sum(len(f) for f in res["frames"]) > 0
