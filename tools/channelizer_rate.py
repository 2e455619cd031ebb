#!/usr/bin/env python3
"""tools/channelizer_rate.py [--out FILE] [--pushes K] [--config a|b|c|c-short|all] [--interpolation L] [--power L]
[--ferr] [--lib PATH --tag NAME] [--raster]: throughput of dh_channelizer on cuda:0.

Configurations, taps = api.channel_taps(rate, D, 6.5 kHz, 12 kHz, 60 dB):
  (a) 2.4 MS/s CS16, D = 50, 192 channels on a 12.5 kHz raster, 10 s of input per push;
  (b) 9.6 MS/s CS16, D = 200, 768 channels, 1 s of input per push;
  (c) 2.048 MS/s CS16, L / M = 3 / 128 (a rational rate: taps designed with interpolation = 3), 160 channels, 10 s of input
      per push; (c-short) the same in 20 ms pushes: 960 outputs, 320 per phase, so every phase's last 128-row tile is half
      empty.  "all" is (a) and (b).
--interpolation L replaces the configuration's L (1 for a and b, 3 for c and c-short); it must share no factor with D.
The lines of profiles/channelizer_rational_rate.jsonl ("Rational rates measured"), in this order in
one run on one device, variants/lib_parent.so being the parent commit built by tools/build_variant.sh:
  --config a --out F --lib variants/lib_parent.so --tag parent_1          --config a --out F --lib digiham_amd/libdigiham_amd.so --tag new_1
  --config a --out F --lib variants/lib_parent.so --tag parent_2          --config a --out F --lib digiham_amd/libdigiham_amd.so --tag new_2
  --config c --out F --tag rational                                       --config c-short --pushes 50 --out F --tag rational
and the kernel trace: rocprofv3 --kernel-trace --stats -- python tools/channelizer_rate.py --config c, in a run of its own.
Each push is timed with HIP events (torch.cuda.Event on the channelizer's stream) in "iq" mode (window + GEMM / rotation)
and in "fm" + DC-blocker mode (+ the discriminator and the recurrence).  Reported per push: ms, ms per second of input,
the real-time factor, and the GEMM's TFLOP/s counted as 8 B T' n_out over the whole push, with its fraction of the
157.3 TF f32 matrix peak.  One JSON line per (config, mode).  --power L adds the modes "iq+power" and "fm+power": the same
with block power over L outputs and the gate enabled (k_cz_power reads 8 bytes per output and channel once more; k_cz_gate).
--ferr (with --power L) adds "iq+ferr" and "fm+ferr": power and the frequency-error blocks (k_cz_ferr reads the same bytes
again).  The lines of profiles/channelizer_ferr_rate.jsonl ("Frequency-error blocks measured"): the
feature off against the parent in ONE process, run(...) of this file called in turn with the parent's and the new library
(tags parent_1, new_1, parent_2, new_2; configuration a, iq and fm), then --config all --power 480 --ferr --modes "" --tag on;
the kernel times: rocprofv3 --kernel-trace --stats -- python tools/channelizer_rate.py --config all --power 480 --ferr
--modes "", in a run of its own.
--lib PATH times another build of the library (tools/build_variant.sh) instead of the package's, --tag labels its lines.
--raster (configurations a and b: their channels sit on 12.5 kHz steps, K = rate / 12.5 kHz) times every (config, mode) four
times in this process, alternating: fixed offsets, raster, fixed offsets, raster (tags fixed_1, raster_1, fixed_2,
raster_2).  A raster line has "raster": K, "fold_p": P, counts the DFT stage as 8 B K' n_out ("gemm_tflops") and adds the
fold's 4 P K n_out ("fold_gflop").  The lines of profiles/channelizer_raster_rate.jsonl ("Raster
measured"), in one run on one device:
  --raster --out F                                                        (no --tag: this one starts F anew)
  --config a --out F --lib variants/lib_parent.so --tag parent_1          --config a --out F --lib digiham_amd/libdigiham_amd.so --tag new_1
  --config a --out F --lib variants/lib_parent.so --tag parent_2          --config a --out F --lib digiham_amd/libdigiham_amd.so --tag new_2
and the split between k_cz_fold and k_cz_gemm_raster: rocprofv3 --kernel-trace --stats -- python tools/channelizer_rate.py
--raster --modes iq, in a run of its own.
The lines of profiles/channelizer_one_gemm_rate.jsonl ("One GEMM entry measured, and not taken"; the
lines tagged new_* are of a build, not kept, in which a fixed bank launched k_cz_gemm_rat with one slot), in one run on one
device, for each of --config a, --config b and --config c-short --pushes 50 the four commands
  --out F --lib variants/lib_parent.so --tag parent_1                     --out F --lib <that build> --tag new_1
  --out F --lib variants/lib_parent.so --tag parent_2                     --out F --lib <that build> --tag new_2"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"a": dict(rate=2.4e6, D=50, B=192, seconds=10.0), "b": dict(rate=9.6e6, D=200, B=768, seconds=1.0),
           "c": dict(rate=2.048e6, D=128, L=3, B=160, seconds=10.0), "c-short": dict(rate=2.048e6, D=128, L=3, B=160, seconds=0.02)}
PEAK_TF = 157.3


def run(name, c, mode, pushes, warmup=2, power=0, ctx=None, tag=None, raster_hz=None):
    import torch
    from digiham_amd import api
    label, mode = mode, mode.split("+")[0]
    rate, D, B, L = c["rate"], c["D"], c["B"], c.get("L", 1)
    n = int(c["seconds"] * rate)
    rational = dict(interpolation=L) if L > 1 else {}          # (an older build given with --lib has no such argument)
    h = api.channel_taps(rate, D, 6500.0, 12000.0, 60.0, **rational)
    tpad = 16 * ((-(-len(h) // L) + 15) // 16)
    freqs = [(b - B // 2) * 12500.0 for b in range(B)]
    if raster_hz:
        rational = dict(raster_hz=raster_hz)
        K = api.raster_steps(rate, raster_hz)
        tpad = 16 * ((K + 15) // 16)                            # the DFT stage's K extent
    cz = api.Channelizer(rate, D, freqs, h, input="cs16", output=mode, dcblock=(mode == "fm"), max_input=n, ctx=ctx, **rational)
    if label.endswith("+power"):
        cz.enable_power(block=power, open_db=-40.0, close_db=-43.0, hang_blocks=2)
    if label.endswith("+ferr"):
        cz.enable_power(block=power, open_db=-40.0, close_db=-43.0, hang_blocks=2, ferr=True)
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
    extra = {"tag": tag} if tag else {}
    if label.endswith("+power") or label.endswith("+ferr"):
        extra.update(block=power, power_read_mb=round(8.0 * B * n_out / 1e6, 1))
    if L > 1:
        extra.update(L=L)
    if raster_hz:
        P = -(-len(h) // K)
        extra.update(raster=K, fold_p=P, fold_gflop=round(4.0 * P * K * n_out / 1e9, 2))
    return {**extra, "config": name, "mode": label, "rate": rate, "D": D, "B": B, "taps": len(h), "tpad": tpad, "n_in": n, "n_out": n_out,
            "ms_per_push": round(ms, 3), "ms_min": round(min(times), 3), "ms_per_s_input": round(ms / c["seconds"], 3),
            "realtime_factor": round(c["seconds"] * 1e3 / ms, 1 if c["seconds"] >= 1 else 2), "gemm_tflops": round(tf, 2), "fraction_of_peak": round(tf / PEAK_TF, 3),
            "pushes": pushes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--pushes", type=int, default=5)
    ap.add_argument("--config", default="all")
    ap.add_argument("--modes", default="iq,fm")
    ap.add_argument("--power", type=int, default=0)
    ap.add_argument("--interpolation", type=int, default=0)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--tag", default=None)
    ap.add_argument("--raster", action="store_true")
    ap.add_argument("--ferr", action="store_true")
    a = ap.parse_args()
    if a.ferr and not a.power:
        ap.error("--ferr needs --power L: the frequency-error blocks are the power blocks")
    names = ["a", "b"] if a.config == "all" else [a.config]
    if a.raster and (a.interpolation > 1 or any(CONFIGS[n].get("L", 1) > 1 for n in names)):
        ap.error("--raster needs interpolation = 1: configurations a and b, no --interpolation")
    rows = []
    ctx = None
    if a.lib:
        from digiham_amd import _capi, api
        ctx = api.Context(lib=_capi.load(a.lib))
    modes = [m for m in a.modes.split(",") if m] + (["iq+power", "fm+power"] if a.power else []) + (["iq+ferr", "fm+ferr"] if a.ferr else [])
    for name in names:
        for mode in modes:
            cfg = dict(CONFIGS[name], L=a.interpolation) if a.interpolation else CONFIGS[name]
            rounds = [(a.tag, None)] if not a.raster else [("fixed_1", None), ("raster_1", 12500.0), ("fixed_2", None), ("raster_2", 12500.0)]
            for tag, raster_hz in rounds:
                r = run(name, cfg, mode, a.pushes, power=a.power, ctx=ctx, tag=tag, raster_hz=raster_hz)
                print(json.dumps(r), flush=True)
                rows.append(r)
    if a.out:
        with open(a.out, "a" if a.tag else "w") as f:       # a tagged run adds its lines to those of the recipe's first command
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
