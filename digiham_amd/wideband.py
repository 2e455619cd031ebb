"""Wideband test signals for the channelizer: the synthesizer's 48 kS/s 4FSK audio (synth.py) FM-modulated onto carriers
of one complex stream at 48 kS/s x D, summed, with noise, quantised to interleaved int16 I / Q (CS16).  torch does the
arithmetic, on the CPU or on a device (`device="cuda"` for the large cases)."""
import numpy as np

from . import synth

AUDIO_RATE = 48000.0
DEVIATION_HZ = 24000.0 * 0.162     # discriminator audio 1.0 <-> 24 kHz; the synth's outer symbols (0.5) -> ~1.94 kHz (DMR)


def dmr_audio(seed, n_calls=2, src=None, dst=None, cc=1, lead_in=37):
    """48 kS/s audio of a DMR carrier whose slot 0 carries `n_calls` voice calls from `src` to `dst` (slot 1 idle bursts).
    Returns (audio float32, dict(src, dst, superframes))."""
    rng = np.random.default_rng(seed)
    src = int(rng.integers(1, 1 << 24)) if src is None else src
    dst = int(rng.integers(1, 1 << 24)) if dst is None else dst
    q0, sf = [synth.dmr_idle_burst(0, cc, rng) for _ in range(4)], 0       # (the receiver syncs before the first LC header)
    for _ in range(n_calls):
        k = int(rng.integers(2, 4))
        q0 += synth.dmr_call(rng, 0, cc, dst=dst, src=src, n_superframes=k)
        sf += k
    q1 = [synth.dmr_idle_burst(1, cc, rng) for _ in range(len(q0))]
    out = list(rng.integers(0, 4, lead_in))
    for i in range(2 * len(q0)):
        out += (q0 if i % 2 == 0 else q1)[i >> 1]
    return synth.shape(np.array(out, np.uint8)), {"src": src, "dst": dst, "superframes": sf}


def ysf_audio(seed, n_frames=30):
    return synth.shape(synth.ysf_stream(seed, n_frames))


def composite(decimation, carriers, n, noise_lsb=2.0, seed=0, device="cpu", peak=0.9, keying=None, noise_device=None):
    """carriers: list of (offset_hz, level_db, audio48) -- each FM-modulated at 48 kS/s x decimation (audio linearly
    interpolated), level relative to the strongest; the sum is scaled so that it never clips, complex Gaussian noise of
    `noise_lsb` rms per component is added, and the result rounded to int16.  `keying`: per carrier None (always on) or
    (start_s, stop_s) -- the carrier's amplitude is 0 outside [start, stop) and its audio begins at start.
    `noise_device`: where the noise generator runs (default: on `device`; a generator's stream depends on its device, so
    "cpu" makes a seed name the same noise whatever `device` is).  Returns
    int16 [n][2] (a numpy array, or a torch tensor on `device` when that is not the CPU)."""
    import torch
    rate = AUDIO_RATE * decimation
    dev = torch.device(device)
    t_out = torch.arange(n, dtype=torch.float64, device=dev) / decimation
    acc = torch.zeros(n, dtype=torch.complex128, device=dev)
    amps = [10.0 ** (lv / 20.0) for _, lv, _ in carriers]
    scale = peak * 32767.0 / max(sum(amps), 1e-9)
    for c, ((off, lv, audio), a) in enumerate(zip(carriers, amps)):
        key = keying[c] if keying is not None else None
        au = torch.from_numpy(np.asarray(audio, np.float64)).to(dev)
        idx = t_out.clamp(max=len(audio) - 1.0) if key is None else (t_out - key[0] * AUDIO_RATE).clamp(min=0.0, max=len(audio) - 1.0)
        i0 = idx.floor().long()
        i1 = (i0 + 1).clamp(max=len(audio) - 1)
        fr = idx - i0.double()
        a_t = au[i0] * (1.0 - fr) + au[i1] * fr
        f = off + DEVIATION_HZ * a_t
        ph = torch.cumsum(f, 0) * (2.0 * np.pi / rate)
        if key is None:
            acc += scale * a * torch.polar(torch.ones_like(ph), ph)
        else:
            t_s = t_out / AUDIO_RATE
            on = ((t_s >= key[0]) & (t_s < key[1])).double()
            acc += scale * a * torch.polar(on, ph)
    ndev = dev if noise_device is None else torch.device(noise_device)
    g = torch.Generator(device=ndev).manual_seed(seed)
    noise = torch.randn((n, 2), generator=g, dtype=torch.float64, device=ndev).to(dev) * noise_lsb
    iq = torch.stack((acc.real, acc.imag), 1) + noise
    q = iq.round().clamp(-32768, 32767).to(torch.int16)
    return q.cpu().numpy() if dev.type == "cpu" else q
