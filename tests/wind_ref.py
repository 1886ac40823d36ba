"""Float64 numpy restatement of the reference's ``wind_noise()`` (simulation/simulate_data_from_param.py:129-217) from the point where the
aligned, SNR-scaled noise exists: the 16-bit temporary files, ffmpeg's ``sidechaincompress`` + ``amix`` (the filter graph of
``buildFFmpegCommand`` :60-89), the 16-bit output file, the clipper, and the rescaled clean target of a row without an RIR.

TEST INFRASTRUCTURE - never imported by the product path.  No ffmpeg binary or source exists where this suite runs: the two filters are
restated from their published definition (af_sidechaincompress: envelope follower on the squared side chain, soft knee by cubic Hermite
interpolation in the log domain; amix: equal weights 1 / n), every option the command line leaves out at ffmpeg's default (level_in 1,
mode downward, makeup 1, knee 2.82843, link average, detection rms, mix 1).  PARITY UNPINNED against the binary.
"""
import numpy as np

KNEE = 2.82843


def q16(y):
    """a 16-bit WAV round trip (audio_io.write_audio / read_audio, flac.quantise_pcm16): round half to even, saturate"""
    return np.clip(np.rint(32768.0 * np.asarray(y, dtype=np.float64)), -32768, 32767) / 32768.0


def hermite(x, x0, x1, p0, p1, m0, m1):
    w = x1 - x0
    t = (x - x0) / w
    m0 = m0 * w
    m1 = m1 * w
    t2 = t * t
    t3 = t2 * t
    ct2 = -3.0 * p0 - 2.0 * m0 + 3.0 * p1 - m1
    ct3 = 2.0 * p0 + m0 - 2.0 * p1 + m1
    return ct3 * t3 + ct2 * t2 + m0 * t + p0


def setup(threshold, ratio, attack, release, fs, knee=KNEE):
    threshold, ratio = np.float64(threshold), np.float64(ratio)
    s = dict(threshold=threshold, ratio=ratio, knee=np.float64(knee))
    s["thres"] = np.log(threshold)
    s["lin_knee_start"] = threshold / np.sqrt(s["knee"])
    s["lin_knee_stop"] = threshold * np.sqrt(s["knee"])
    s["adj_knee_start"] = s["lin_knee_start"] * s["lin_knee_start"]
    s["knee_start"] = np.log(s["lin_knee_start"])
    s["knee_stop"] = np.log(s["lin_knee_stop"])
    s["compressed_knee_stop"] = (s["knee_stop"] - s["thres"]) / ratio + s["thres"]
    s["ka"] = min(1.0, 1.0 / (np.float64(attack) * fs / 4000.0))
    s["kr"] = min(1.0, 1.0 / (np.float64(release) * fs / 4000.0))
    return s


def envelope(a, ka, kr):
    """S[t] of the follower started at 0: S += (a - S) * (ka if a > S else kr)"""
    out = np.empty(len(a), dtype=np.float64)
    S = 0.0
    ka, kr = float(ka), float(kr)
    for t, at in enumerate(np.asarray(a, dtype=np.float64).tolist()):
        S = S + (at - S) * (ka if at > S else kr)
        out[t] = S
    return out


def log_gain(slope, s):
    """the compressor's output level for the detector level ``slope`` (both natural logs): the ratio's line, the Hermite inside the knee"""
    slope = np.asarray(slope, dtype=np.float64)
    gain = (slope - s["thres"]) / s["ratio"] + s["thres"]
    if s["knee"] > 1.0:
        knee = hermite(slope, s["knee_start"], s["knee_stop"], s["knee_start"], s["compressed_knee_stop"], 1.0, 1.0 / s["ratio"])
        gain = np.where(slope < s["knee_stop"], knee, gain)
    return gain


def gain(S, s):
    """linear gain per sample from the follower's state"""
    S = np.asarray(S, dtype=np.float64)
    on = (S > 0.0) & (S > s["adj_knee_start"])
    slope = 0.5 * np.log(np.where(on, S, 1.0))
    return np.where(on, np.exp(log_gain(slope, s) - slope), 1.0)


def wind_mix(x, v, speech, fs, threshold, ratio, attack, release, sc_gain, clipping_threshold, has_rir):
    """x: the row's speech after high-pass / RIR; v: its aligned, SNR-scaled noise; speech: the clean target (valid samples only).
    -> dict(noisy, noise, speech, c, and the intermediates xq, vq, S, g, mq)"""
    x, v, speech = (np.asarray(t, dtype=np.float64) for t in (x, v, speech))
    peak = max(np.max(np.abs(x)), np.max(np.abs(v)))
    c = 0.9 / peak if peak > 0 else 1.0                      # (the reference divides by zero on two silent inputs)
    xq, vq = q16(c * x), q16(c * v)
    s = setup(threshold, ratio, attack, release, fs)
    a = (vq * np.float64(sc_gain)) ** 2
    S = envelope(a, s["ka"], s["kr"])
    g = gain(S, s)
    y = xq * g
    m = 0.5 * y + 0.5 * vq
    mq = q16(m)
    mix = mq / c
    noise = vq / c
    lo = clipping_threshold * np.min(mix)
    mix = np.maximum(mix, lo)
    hi = clipping_threshold * np.max(mix)
    mix = np.minimum(mix, hi)
    return dict(noisy=mix, noise=noise, speech=speech if has_rir else c * speech, c=c, xq=xq, vq=vq, S=S, g=g, mq=mq, setup=s)


def near_tie(m, eps=1e-9):
    """samples whose 16-bit rounding is decided by less than ``eps`` of a step: there a gain that is 1 up to its last bits may round the
    other way than the closed form with g = 1 exactly"""
    f = 32768.0 * np.asarray(m, dtype=np.float64)
    return np.abs(np.abs(f - np.floor(f)) - 0.5) < eps


# ---- the batch tests/test_wind_gpu.py and the sensitivity check of tests/test_wind_cpu.py share -------------------------------------------------
def kernel_cases(chunk):
    """rows of one [B, ld] batch: lengths 1, chunk - 1, chunk, chunk + 1, 3 chunk + 17 on wind rows, with plain rows between them; fs 8000
    with attack 0.01 ms (ka at its cap of 1) and fs 48000; ratios 1, 7.9, 20; with and without an RIR.  The threshold 0.05 sits inside the
    range the side chain's level sweeps (the noise swells from silence to full scale), so a long row spends time below the knee, in it and above."""
    lens = [1, 700, chunk - 1, 333, chunk, chunk + 1, 3 * chunk + 17, 3 * chunk + 17, 2 * chunk + 5]
    wind = [0, 2, 4, 5, 6, 7]
    par = {0: dict(ratio=7.9, attack=57.5, release=23.6, fs=48000, has_rir=False),
           2: dict(ratio=20.0, attack=0.01, release=5.0, fs=8000, has_rir=True),
           4: dict(ratio=1.0, attack=12.0, release=80.0, fs=48000, has_rir=False),
           5: dict(ratio=7.9, attack=0.01, release=40.0, fs=8000, has_rir=False),
           6: dict(ratio=20.0, attack=5.0, release=23.6, fs=48000, has_rir=True),
           7: dict(ratio=7.9, attack=2.0, release=10.0, fs=8000, has_rir=False)}
    for p in par.values():
        p.update(threshold=0.05, sc_gain=0.87, clipping_threshold=0.9)
    rng = np.random.default_rng(20260)
    B, ld = len(lens), 3 * chunk + 24
    speech = (0.2 * rng.standard_normal((B, ld))).astype(np.float32)
    x = (0.25 * rng.standard_normal((B, ld))).astype(np.float32)
    t = np.arange(ld) / float(ld)
    swell = (0.002 + np.sin(np.pi * t) ** 4)[None, :]                      # the gusts: quiet at both ends, full scale in the middle
    noise = (0.3 * swell * rng.standard_normal((B, ld))).astype(np.float32)
    noisy = (x + noise).astype(np.float32)
    return dict(lens=lens, wind=wind, par=par, speech=speech, x=x, noise=noise, noisy=noisy, B=B, ld=ld)


def run_cases(cs, x=None, noise=None):
    """the oracle on every wind row of ``kernel_cases`` (optionally on perturbed inputs) -> {row: wind_mix result}"""
    x = cs["x"] if x is None else x
    noise = cs["noise"] if noise is None else noise
    out = {}
    for b in cs["wind"]:
        n, p = cs["lens"][b], cs["par"][b]
        out[b] = wind_mix(x[b, :n], noise[b, :n], cs["speech"][b, :n], p["fs"], p["threshold"], p["ratio"], p["attack"], p["release"],
                          p["sc_gain"], p["clipping_threshold"], p["has_rir"])
    return out


def f32_step(want):
    """one float32 unit in the last place at ``want``: what the cast of the float64 result and the device's own last rounding may differ by"""
    return np.spacing(np.abs(np.asarray(want)).astype(np.float32)).astype(np.float64)
