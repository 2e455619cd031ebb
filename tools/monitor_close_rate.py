"""What naming on close costs api.DeviceMonitor on one MI355X, on workload (b) of tools/monitor_rate.py:
4 096 channels x 4 800 samples, 256 channels assigned and open, the rest closed.

  steady rounds   the same rows pushed alternately, in one process, into a DeviceMonitor of a BASELINE library (--baseline:
                  a libdigiham_amd.so built from the commit before the mode existed), one of this tree with the mode off
                  and one with on_close="default".  No channel closes.  Wall time of push() with its blocks returned,
                  3 warm-up rounds, median of 20, min - max.  The condition, for both of this tree's: median <= the
                  baseline's median + the min - max spread of the baseline's own 20 calls.  Without --baseline the mode-off
                  monitor of this tree is the baseline of the other.
  closing round   256 channels carry a POCSAG preamble and one batch, which the scanner cannot confirm; the round in which
                  their gates close runs step C, the masked resets and the replay of 256 channels from the ring.  Reported
                  without a condition: that round's time, the rounds before it, and what was decoded.

Prints one JSON line; --out appends it to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from digiham_amd import _capi, api, synth      # noqa: E402
from monitor_rate import dmr_rows              # noqa: E402

B, N, BUSY = 4096, 4800, list(range(0, 4096, 16))


def summary(t):
    return {"median_ms": round(float(np.median(t)), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)}


def steady(ctx, base_ctx, rounds, warm):
    import torch
    x = np.zeros((B, N * 10), np.float32)
    x[BUSY] = dmr_rows(len(BUSY), N * 10)
    windows = [ctx.mem.from_numpy(np.ascontiguousarray(x[:, k * N:(k + 1) * N])) for k in range(10)]
    counts = np.zeros(B, np.uint32)
    counts[BUSY] = N
    counts = ctx.mem.from_numpy(counts)
    mons = {}
    if base_ctx is not None:
        mons["baseline"] = api.DeviceMonitor(B, N, depth=24000, ctx=base_ctx)
    mons["off"] = api.DeviceMonitor(B, N, depth=24000, ctx=ctx)
    mons["on_close"] = api.DeviceMonitor(B, N, depth=24000, ctx=ctx, on_close="default")
    times = {k: [] for k in mons}
    for k in range(40):                                   # warm-up: until every busy channel is assigned, `warm` rounds at least
        for m in mons.values():
            m.push(windows[k % 10], counts=counts)
        if k + 1 >= warm and all(sum(a is not None for a in m.assigned) == len(BUSY) for m in mons.values()):
            break
    else:
        raise AssertionError("not every busy channel was named in 40 rounds")
    key_of = lambda blks: [(u["channel"], u["first_sample"], u["frames"].tobytes(), u["events"].tobytes()) for u in blks]
    for r in range(rounds):
        w = windows[(k + 1 + r) % 10]
        got = {}
        for name, m in mons.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got[name] = m.push(w, counts=counts)
            times[name].append((time.perf_counter() - t0) * 1e3)
        assert all(key_of(g) == key_of(got["off"]) for g in got.values()), "the monitors disagree"
    for m in mons.values():
        m.close()
    rec = {name: summary(t) for name, t in times.items()}
    ref = rec["baseline" if base_ctx is not None else "off"]
    rec["condition_median_le_ms"] = round(ref["median_ms"] + ref["max_ms"] - ref["min_ms"], 4)
    rec["off_condition_met"] = rec["off"]["median_ms"] <= rec["condition_median_le_ms"]
    rec["on_close_condition_met"] = rec["on_close"]["median_ms"] <= rec["condition_median_le_ms"]
    return rec


def pocsag_row():
    rng = np.random.default_rng(7)
    text = "".join(chr(int(c)) for c in rng.integers(32, 127, 39))
    bits = [1, 0] * 288
    for w in [synth.POCSAG_SYNC] + synth.pocsag_batches([(int(rng.integers(8, 1 << 21)) & ~7, 3, text)])[:16]:
        bits += synth._bits_of(w, 32)
    return synth.impair(synth.fsk_shape(np.array(bits, np.uint8), sps=40, invert=True), 5, snr_db=22, dc=0.02, delay=11)


def closing(ctx, trials):
    import torch
    row = pocsag_row()
    open_rounds = -(-len(row) // N) + 1                   # the pushes that overlap the row, and one push of hang
    x = np.zeros((B, (open_rounds + 2) * N), np.float32)
    x[BUSY, N:N + len(row)] = row
    x[BUSY, N + len(row):] = np.random.default_rng(8).normal(0, 0.3, x.shape[1] - N - len(row)).astype(np.float32)
    windows = [ctx.mem.from_numpy(np.ascontiguousarray(x[:, k * N:(k + 1) * N])) for k in range(open_rounds + 2)]
    opened, closed = np.zeros(B, np.uint32), ctx.mem.from_numpy(np.zeros(B, np.uint32))
    opened[BUSY] = N
    opened = ctx.mem.from_numpy(opened)
    mon = api.DeviceMonitor(B, N, depth=96000, ctx=ctx, on_close="default")
    out = {"open_rounds": open_rounds, "close_round_ms": [], "scanned_round_ms": [], "named": [], "blocks": [], "frame_bytes": []}
    for _ in range(trials):
        mon.reset()
        scanned = []
        for k in range(open_rounds + 2):
            cnt = opened if 1 <= k <= open_rounds else closed
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            blocks = mon.push(windows[k], counts=cnt)
            ms = (time.perf_counter() - t0) * 1e3
            if 1 <= k <= open_rounds:
                assert not blocks and not any(mon.assigned)
                scanned.append(ms)
        out["close_round_ms"].append(round(ms, 4))        # (the last round: the gates closed in it)
        out["scanned_round_ms"].append(round(float(np.median(scanned)), 4))
        out["named"].append(sum(a == "pocsag" for a in mon.assigned))
        out["blocks"].append(len(blocks))
        out["frame_bytes"].append(int(sum(len(u["frames"]) for u in blocks)))
    mon.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline", help="a libdigiham_amd.so of the commit before naming on close")
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trials", type=int, default=3)
    args = ap.parse_args()
    ctx = api.Context(device=0)
    base_ctx = api.Context(lib=_capi.load(args.baseline), device=0) if args.baseline else None
    rec = {"workload": "b", "channels": B, "samples": N, "assigned": len(BUSY), "rounds": args.rounds,
           "steady": steady(ctx, base_ctx, args.rounds, args.warmup), "closing": closing(ctx, args.trials)}
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
