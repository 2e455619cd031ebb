"""api.Monitor against api.DeviceMonitor on one MI355X: the same rows pushed into the two alternately in one process,
wall time of push() with its blocks returned (3 warm-up rounds, median of 20, min - max).

  (a) 192 channels x 48 000 samples of synth DMR, every channel assigned;
  (b) 4 096 channels x 4 800 samples, 256 channels assigned and open, the rest closed.

A third monitor takes the same pushes through dh_monitor_push with no sink, followed by a synchronisation: what a round
costs a C caller that leaves the outputs on the device ("dh_monitor_push").

A fourth, api.DeviceMonitor(packed=True), reads a round back through one dh_outpack ("DeviceMonitor(packed)"); a fifth
takes the same pushes through dh_outpack_clear, dh_monitor_push_packed and dh_outpack_read from C-level calls, with no
Python blocks built ("dh_monitor_push_packed+read").  The record also holds the packed size of a round beside the dense
size of one DMR engine's outputs, and the time of one dh_outpack_append (its two kernels) by stream events.

Prints one JSON line per workload; --out appends them to a file.  The condition on (a): DeviceMonitor's median <=
Monitor's median + the min - max spread of Monitor's own 20 calls.  The condition on the packed monitor, both workloads:
its median <= DeviceMonitor's median + the min - max spread of DeviceMonitor's own 20 calls."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from digiham_amd import _capi, api, synth      # noqa: E402


def dmr_rows(n_rows, n):
    base = []
    for seed in range(41, 49):
        s = synth.impair(synth.shape(synth.dmr_stream(seed, n // 1440 + 8)), seed, snr_db=24, dc=0.01 * (seed - 44), delay=seed % 7)
        base.append(np.asarray(s[:n + 1440], np.float32))
    return np.stack([np.roll(base[b % len(base)], -1440 * (b // len(base)))[:n] for b in range(n_rows)])


def measure(name, B, n, busy, depth, rounds, warm, ctx):
    import torch
    x = np.zeros((B, n * 10), np.float32)
    x[busy] = dmr_rows(len(busy), n * 10)
    windows = [ctx.mem.from_numpy(np.ascontiguousarray(x[:, k * n:(k + 1) * n])) for k in range(10)]
    counts = np.zeros(B, np.uint32)
    counts[busy] = n
    counts = ctx.mem.from_numpy(counts)
    mons = {"Monitor": api.Monitor(B, n, depth=depth, ctx=ctx), "DeviceMonitor": api.DeviceMonitor(B, n, depth=depth, ctx=ctx),
            "DeviceMonitor(packed)": api.DeviceMonitor(B, n, depth=depth, ctx=ctx, packed=True)}
    raw, no_sink = api.DeviceMonitor(B, n, depth=depth, ctx=ctx), _capi.MONITOR_SINK(0)
    cp = api.DeviceMonitor(B, n, depth=depth, ctx=ctx, packed=True)        # driven through the C entries below
    hdr, host = _capi.OutpackHeader(), [a.ctypes.data_as(C.c_void_p) for a in (cp.pack._entries, cp.pack._events, cp.pack._frames)]
    times, blocks = {k: [] for k in list(mons) + ["dh_monitor_push", "dh_monitor_push_packed+read"]}, {k: 0 for k in mons}
    packed_bytes = []
    k = 0
    while True:                                           # warm-up: until every busy channel is assigned, `warm` rounds at least
        for m in list(mons.values()) + [raw, cp]:
            m.push(windows[k % 10], counts=counts)
        k += 1
        done = all(sum(a is not None for a in m.assigned) == len(busy) for m in mons.values())
        if (k >= warm and done) or k >= 40:
            break
    assert done, "not every busy channel was named in 40 rounds"
    for r in range(rounds):
        w = windows[(k + r) % 10]
        got = {}
        for key, m in mons.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got[key] = m.push(w, counts=counts)
            times[key].append((time.perf_counter() - t0) * 1e3)
            blocks[key] += len(got[key])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = ctx.lib.dh_monitor_push(raw._h, ctx.mem.ptr(w), w.stride(0), n, ctx.mem.ptr(counts), no_sink, None)
        torch.cuda.synchronize()
        times["dh_monitor_push"].append((time.perf_counter() - t0) * 1e3)
        assert rc == 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = ctx.lib.dh_outpack_clear(cp.pack._h)
        rc |= ctx.lib.dh_monitor_push_packed(cp._h, ctx.mem.ptr(w), w.stride(0), n, ctx.mem.ptr(counts), cp.pack._h)
        rc |= ctx.lib.dh_outpack_read(cp.pack._h, C.byref(hdr), *host)
        times["dh_monitor_push_packed+read"].append((time.perf_counter() - t0) * 1e3)
        assert rc == 0 and hdr.n_entries == len(got["DeviceMonitor(packed)"])
        packed_bytes.append(32 + 32 * hdr.n_entries + 32 * hdr.n_events + hdr.frame_bytes)
        key_of = lambda blks: [(u["channel"], u["first_sample"], u["frames"].tobytes(), u["events"].tobytes()) for u in blks]
        assert key_of(got["Monitor"]) == key_of(got["DeviceMonitor"]) == key_of(got["DeviceMonitor(packed)"]), "the monitors disagree"
    rec = {"workload": name, "channels": B, "samples": n, "assigned": len(busy), "warm_up_rounds": k, "rounds": rounds}
    for key, t in times.items():
        rec[key] = {"median_ms": round(float(np.median(t)), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4), "blocks": blocks.get(key)}
    ref = rec["Monitor"]
    rec["condition_median_le_ms"] = round(ref["median_ms"] + ref["max_ms"] - ref["min_ms"], 4)
    rec["condition_met"] = rec["DeviceMonitor"]["median_ms"] <= rec["condition_median_le_ms"]
    base = rec["DeviceMonitor"]
    rec["packed_condition_median_le_ms"] = round(base["median_ms"] + base["max_ms"] - base["min_ms"], 4)
    rec["packed_condition_met"] = rec["DeviceMonitor(packed)"]["median_ms"] <= rec["packed_condition_median_le_ms"]
    # bytes: a round's pack (header + entries + events + padded frame bytes) beside the dense outputs of ONE push of the DMR
    # engine (frames, events and the two count arrays)
    eng = cp.engines["dmr"]
    stride = {}
    for what, getter in (("frames", ctx.lib.dh_engine_frames), ("events", ctx.lib.dh_engine_events)):
        p, st, cnt = C.c_void_p(), C.c_size_t(), C.c_void_p()
        assert getter(eng._h, C.byref(p), C.byref(st), C.byref(cnt)) == 0
        stride[what] = st.value
    rec["packed_bytes_per_round"] = int(np.median(packed_bytes))
    rec["dense_bytes_per_push"] = B * (stride["frames"] + 32 * stride["events"] + 8)
    # one dh_outpack_append of the DMR engine's current rows by stream events: its two kernels, and with an all-zero mask
    # (the scan walks the channels and keeps nothing; the copy's workgroups find no entry)
    zero_mask = ctx.mem.zeros((B,), np.uint32)
    for label, mask in (("append_ms", counts), ("append_nothing_kept_ms", zero_mask)):
        t = []
        for _ in range(20):
            cp.pack.clear()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            assert ctx.lib.dh_outpack_append(cp.pack._h, eng._h, ctx.mem.ptr(mask), None, 0, 0) == 0
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1))
        rec[label] = {"median_ms": round(float(np.median(t)), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)}
    assert raw.assigned == mons["DeviceMonitor"].assigned == cp.assigned
    for m in list(mons.values()) + [raw, cp]:
        m.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["a", "b"])
    args = ap.parse_args()
    ctx = api.Context(device=0)
    work = [("a", 192, 48000, list(range(192)), 96000), ("b", 4096, 4800, list(range(0, 4096, 16)), 24000)]
    for name, B, n, busy, depth in work:
        if args.only and args.only != name:
            continue
        rec = measure(name, B, n, busy, depth, args.rounds, args.warmup, ctx)
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
