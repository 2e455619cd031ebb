#!/usr/bin/env python3
"""tools/channelizer_rate.py [--out FILE] [--pushes K] [--config a|b|all]: throughput of dh_channelizer on cuda:0.

Configurations, taps = api.channel_taps(rate, D, 6.5 kHz, 12 kHz, 60 dB):
  (a) 2.4 MS/s CS16, D = 50, 192 channels on a 12.5 kHz raster, 10 s of input per push;
  (b) 9.6 MS/s CS16, D = 200, 768 channels, 1 s of input per push.
Each push is timed with HIP events (torch.cuda.Event on the channelizer's stream) in "iq" mode (window + GEMM / rotation)
and in "fm" + DC-blocker mode (+ the discriminator and the recurrence).  Reported per push: ms, ms per second of input,
the real-time factor, and the GEMM's TFLOP/s counted as 8 B T' n_out over the whole push, with its fraction of the
157.3 TF f32 matrix peak.  One JSON line per (config, mode)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"a": dict(rate=2.4e6, D=50, B=192, seconds=10.0), "b": dict(rate=9.6e6, D=200, B=768, seconds=1.0)}
PEAK_TF = 157.3


def run(name, c, mode, pushes, warmup=2):
    import torch
    from digiham_amd import api
    rate, D, B = c["rate"], c["D"], c["B"]
    n = int(c["seconds"] * rate)
    h = api.channel_taps(rate, D, 6500.0, 12000.0, 60.0)
    tpad = 16 * ((len(h) + 15) // 16)
    freqs = [(b - B // 2) * 12500.0 for b in range(B)]
    cz = api.Channelizer(rate, D, freqs, h, input="cs16", output=mode, dcblock=(mode == "fm"), max_input=n)
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randint(-2000, 2000, (n, 2), generator=g, device="cuda", dtype=torch.int32).to(torch.int16)
    times = []
    for i in range(warmup + pushes):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        _, n_out = cz.push(x)
        e.record()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(s.elapsed_time(e))
    cz.close()
    ms = sorted(times)[len(times) // 2]
    flop = 8.0 * B * tpad * n_out
    tf = flop / (ms * 1e-3) / 1e12
    return {"config": name, "mode": mode, "rate": rate, "D": D, "B": B, "taps": len(h), "tpad": tpad, "n_in": n, "n_out": n_out,
            "ms_per_push": round(ms, 3), "ms_min": round(min(times), 3), "ms_per_s_input": round(ms / c["seconds"], 3),
            "realtime_factor": round(c["seconds"] * 1e3 / ms, 1), "gemm_tflops": round(tf, 2), "fraction_of_peak": round(tf / PEAK_TF, 3),
            "pushes": pushes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--pushes", type=int, default=5)
    ap.add_argument("--config", default="all")
    ap.add_argument("--modes", default="iq,fm")
    a = ap.parse_args()
    rows = []
    for name in (["a", "b"] if a.config == "all" else [a.config]):
        for mode in a.modes.split(","):
            r = run(name, CONFIGS[name], mode, a.pushes)
            print(json.dumps(r), flush=True)
            rows.append(r)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
