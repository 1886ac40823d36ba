"""Golden vectors produced BY THE REFERENCE'S OWN CODE for the bandwidth estimate (run in the build container only, where
/root/reference exists): ``utils/estimate_audio_bandwidth.py::estimate_bandwidth`` on seeded synthetic files.

The reference module imports soundfile and tqdm, which this image lacks.  They are registered as stand-in modules so that
the file imports; the only behaviour supplied is ``soundfile.read`` serving the seeded in-memory arrays by "path".
Only data is stored (inputs, rates, results), never reference source.

Files: coloured noise low-passed at a random cutoff, over a white noise floor between -120 and -30 dB; a third quantised to 16
bits; a quarter two-channel; 0.3-1.5 s long; at all seven challenge rates; plus one segment-dict case, one all-zero case and
one repeated uid.

A condition, not a tolerance: a case is kept only if the decisive bin and every bin above it lie at least 0.01 dB away from
``min_energy``; at least 6 per rate must remain.  With that gate a float32 transform must reproduce EVERY bin.

Stored:
  ref_bandwidth.npz         per case k: uid, fs, channels, is_int16, segment (start, end | nan), the frequency the reference
                            returned (nan: None), its bin, the float64 mean power of the same torch.stft call (`mp_k`), the
                            margin in dB; the rfftfreq vectors of the seven rates; `f32_cpu_rel_err`: the largest relative
                            error of a float32 torch.stft on the CPU against the float64 mean power over bins within 80 dB of
                            each case's peak - the yardstick of the device tolerance.
  ref_bandwidth_wav<fs>.npz the inputs of the cases at rate fs (`wav_k`: int16 or float32 [C, L]); one file per rate so that
                            no committed file passes 1 MiB.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000)
PER_RATE = 6
MARGIN_DB = 0.01

AUDIO = {}      # "path" -> (float64 [L] or [L, C] array, fs): what the stand-in soundfile serves


def install_stand_ins():
    def mod(name, **attrs):
        m = sys.modules.get(name) or types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m

    def sf_read(path, **kw):
        x, fs = AUDIO[str(path)]
        return np.array(x, dtype=np.float64), fs

    def unavailable(*a, **k):
        raise RuntimeError("not used by the fixture")
    mod("soundfile", read=sf_read, write=unavailable)
    mod("tqdm"); mod("tqdm.contrib"); mod("tqdm.contrib.concurrent", process_map=unavailable)
    sys.path.insert(0, os.path.join(REF, "utils"))


def synth(rng, fs, n, channels, int16):
    from scipy.signal import firwin, lfilter
    cutoff = rng.uniform(0.15, 0.95)                 # of the Nyquist frequency
    floor_db = rng.uniform(-120.0, -30.0)
    taps = firwin(255, cutoff, window=("kaiser", 12.0))
    out = []
    for _ in range(channels):
        x = rng.standard_normal(n + 512)
        acc = lfilter([1.0], [1.0, -rng.uniform(0.0, 0.9)], x)        # colour: one pole
        y = lfilter(taps, 1.0, acc)[512:]
        y = y / np.sqrt(np.mean(y ** 2))
        y = y + 10.0 ** (floor_db / 20.0) * rng.standard_normal(n)
        out.append(y)
    x = np.stack(out)
    x = 0.5 * x / np.abs(x).max()
    if int16:
        return np.round(x * 32768.0).astype(np.int16)
    return x.astype(np.float32)


def as_served(wav):
    """what soundfile.read returns for the stored samples: float64 [L] (mono) or [L, C]"""
    x = wav.astype(np.float64) / 32768.0 if wav.dtype == np.int16 else wav.astype(np.float64)
    return x[0] if x.shape[0] == 1 else np.ascontiguousarray(x.T)


def mean_power(x, fs, dtype):
    n_fft, hop = int(512 / 16000 * fs), int(256 / 16000 * fs)
    spec = torch.stft(torch.from_numpy(x).to(dtype), n_fft=n_fft, hop_length=hop, window=torch.hann_window(n_fft, dtype=dtype),
                      onesided=True, return_complex=True)
    return (spec.real.pow(2) + spec.imag.pow(2)).mean(2)


def main():
    install_stand_ins()
    ref = importlib.import_module("estimate_audio_bandwidth")
    rng = np.random.default_rng(20260)
    meta, wavs = [], {fs: {} for fs in RATES}
    out = {}
    worst32 = 0.0

    def run_case(uid, fs, wav, seg=None):
        """-> record or None (gate)"""
        nonlocal worst32
        path = "/fixture/%s_%d.wav" % (uid, len(AUDIO))
        AUDIO[path] = (as_served(wav), fs)
        entry = path if seg is None else {"audio_path": path, "start": seg[0], "end": seg[1]}
        got = ref.estimate_bandwidth((uid, entry))
        x = wav.astype(np.float64) / 32768.0 if wav.dtype == np.int16 else wav.astype(np.float64)
        if seg is not None:
            x = x[:, int(seg[0] * 16000):int(seg[1] * 16000)]
        mp = mean_power(x, fs, torch.float64)
        n_fft = int(512 / 16000 * fs)
        freq = torch.fft.rfftfreq(n_fft, d=1 / fs)
        # lines 45-49 on the recomputed mean power must give the reference's answer
        min_energy = mp.max(1).values.min() * 10 ** (-50.0 / 10)
        col = mp.min(0).values
        mine = None
        for i in range(len(freq) - 1, -1, -1):
            if col[i] > min_energy:
                mine = i
                break
        if got is None:
            assert mine is None
            return dict(uid=uid, fs=fs, wav=wav, seg=seg, freq=np.nan, bin=-1, mp=mp.numpy(), margin=np.inf)
        assert got[0] == uid and got[1][0] == path and got[1][1] == freq[mine].item(), (got, mine)
        margin = float(np.abs(10.0 * np.log10(col[mine:].numpy() / float(min_energy))).min())
        if margin < MARGIN_DB:
            return None
        mp32 = mean_power(x.astype(np.float32), fs, torch.float32).double()
        for c in range(mp.shape[0]):
            keep = mp[c] >= mp[c].max() * 1e-8
            worst32 = max(worst32, float(((mp32[c] - mp[c]).abs() / mp[c])[keep].max()))
        return dict(uid=uid, fs=fs, wav=wav, seg=seg, freq=got[1][1], bin=mine, mp=mp.numpy(), margin=margin)

    cases = []
    for fs in RATES:
        kept = tries = 0
        while kept < PER_RATE:
            tries += 1
            assert tries <= 4 * PER_RATE, "too many cases fall inside the 0.01 dB gate at %d Hz" % fs
            j = kept
            dur = (1.5, 0.3)[j] if j < 2 else rng.uniform(0.3, 0.7)       # the range's ends, the rest short (file size)
            channels = 2 if j in (1, 4) and fs != 44100 or (fs == 44100 and j == 1) else 1
            rec = run_case("utt%d_%d" % (fs, j), fs, synth(rng, fs, int(dur * fs), channels, int16=(j % 3 == 2)))
            if rec is not None:
                cases.append(rec)
                kept += 1
    # specials: a segment entry at a rate other than 16 kHz (the slice is in 16 kHz samples all the same), an all-zero file,
    # a repeated uid
    rec = None
    while rec is None:
        rec = run_case("segment", 32000, synth(rng, 32000, 16000, 1, False), seg=(0.1, 0.45))
    cases.append(rec)
    cases.append(run_case("zeros", 16000, np.zeros((1, 4800), dtype=np.int16)))
    rec = None
    while rec is None:
        rec = run_case("utt16000_0", 16000, synth(rng, 16000, 5000, 1, True))
    cases.append(rec)

    per_rate = {fs: sum(1 for c in cases if c["fs"] == fs and c["bin"] >= 0) for fs in RATES}
    assert all(v >= 6 for v in per_rate.values()), per_rate
    for k, c in enumerate(cases):
        out["mp_%d" % k] = c["mp"]
        wavs[c["fs"]]["wav_%d" % k] = c["wav"]
    out["uid"] = np.array([c["uid"] for c in cases])
    out["fs"] = np.array([c["fs"] for c in cases], dtype=np.int64)
    out["channels"] = np.array([c["wav"].shape[0] for c in cases], dtype=np.int64)
    out["is_int16"] = np.array([c["wav"].dtype == np.int16 for c in cases])
    out["segment"] = np.array([c["seg"] if c["seg"] else (np.nan, np.nan) for c in cases], dtype=np.float64)
    out["freq"] = np.array([c["freq"] for c in cases], dtype=np.float64)
    out["bin"] = np.array([c["bin"] for c in cases], dtype=np.int64)
    out["margin_db"] = np.array([c["margin"] for c in cases], dtype=np.float64)
    out["threshold_db"] = np.float64(-50.0)
    out["f32_cpu_rel_err"] = np.float64(worst32)
    for fs in RATES:
        out["rfftfreq_%d" % fs] = torch.fft.rfftfreq(int(512 / 16000 * fs), d=1 / fs).numpy()
    path = os.path.join(HERE, "ref_bandwidth.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(cases), "cases; smallest margin %.4f dB; f32 cpu rel err %.3e"
          % (min(c["margin"] for c in cases), worst32))
    for fs in RATES:
        p = os.path.join(HERE, "ref_bandwidth_wav%d.npz" % fs)
        np.savez_compressed(p, **wavs[fs])
        size = os.path.getsize(p)
        print("wrote", p, size, "bytes")
        assert size < (1 << 20), "a committed file may not pass 1 MiB"


if __name__ == "__main__":
    main()
