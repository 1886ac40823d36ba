"""Edge fixtures of the ESTOI / SDR tests, shared by tests/test_metrics_cpu.py (oracle against pystoi's dither, Levinson against the
dense solve) and tests/test_metrics_gpu.py (kernels against the oracle).  Plain numpy: no GPU, no package under test."""
from math import gcd

import numpy as np

from oracle import metrics_ref


def _pairs(P, L, fs, seed):
    from tests.test_metrics_gpu import _pairs as f        # the suite's speech-like pairs (imported late: that module imports this one)
    return f(P, L, fs, seed)


# ---- an estimate that is exactly zero for longer than one 30-frame segment (a gated / muted model output) -----------------------
# 10 kHz: 6000 zeros = 0.6 s; a segment is 29 * 128 + 256 = 3968 samples, so at least 2032 / 128 = 15 segments see a whole band row
# of zeros (ss == 0 in every band).  16 kHz: the same 0.6 s in front of the 16 -> 10 kHz resampler, whose FIR has finite support.
DEGENERATE = [(10000, 12000), (10000, 30000), (16000, 19200), (16000, 32000)]


def degenerate_pairs(fs, L):
    ref, inf = _pairs(3, L, fs, 5)
    z0 = int(0.4 * L)
    inf[:, z0:z0 + int(0.6 * fs)] = 0
    return ref, inf


def zero_interior_after_resampling(fs, L):
    """[a, b): the samples of resample_to_10k's output that depend on zeroed input samples only (one sample of margin each side)."""
    z0 = int(0.4 * L)
    z1 = z0 + int(0.6 * fs)
    if fs == metrics_ref.FS:
        return z0, z1
    h, up, down = metrics_ref.resample_window_oct(metrics_ref.FS, fs)
    half = (len(h) - 1) // 2                                  # output n reads inputs j with |j * up - n * down| <= half
    a = -((-(z0 * up + half)) // down) + 1
    b = ((z1 - 1) * up - half) // down - 1
    return a, b


# ---- stationary coloured noise at 10 kHz: no frame is dropped, so L fixes the number of STFT frames M -----------------------------
# frames kept = len(range(0, L - 256, 128)) = K, M = K - 1:  L = 4095 / 4096 -> M = 29 (1e-5);  4097, 4224 -> M = 30 (J = 1);
# 4225 -> M = 31 (J = 2);  4353 -> M = 32 (J = 3)
FRAME_EDGE_SHORT = (4095, 4096)
FRAME_EDGE = (4097, 4224, 4225, 4353)


def stationary_pair(L, seed):
    rng = np.random.default_rng(seed)
    c = np.convolve(rng.standard_normal(L), [1, 0.9, 0.5, 0.2], "same")
    return c.astype(np.float32), (c + 0.5 * rng.standard_normal(L)).astype(np.float32)


def mixed_batch(L=20000):
    """four pairs of one length that keep different numbers of frames: stationary (all kept) | silent head and tail | reference loud in
    its first 20 frames only (fewer than 30 kept -> 1e-5) | estimate zero for 0.6 s"""
    r0, e0 = stationary_pair(L, 71)
    r1, e1 = _pairs(1, L, 10000, 72)
    r2, e2 = stationary_pair(L, 73)
    e2 = e2 - r2
    r2[19 * 128 + 256:] *= 1e-4                               # 80 dB down: dropped by the 40 dB rule
    e2 = (r2 + e2).astype(np.float32)
    r3, e3 = _pairs(1, L, 10000, 74)
    e3[:, int(0.4 * L):int(0.4 * L) + 6000] = 0
    return np.stack([r0, r1[0], r2, r3[0]]), np.stack([e0, e1[0], e2, e3[0]])


# ---- SDR --------------------------------------------------------------------------------------------------------------------
# xcorr_kernel tiles the signal by 2048 samples (+ 512 lags of halo): one tile | exactly one | two | three; below 512 the signal is
# shorter than the distortion filter
SDR_LENGTHS = (300, 511, 512, 513, 2047, 2048, 2049, 4097)
LEVINSON_LENGTHS = (300, 511, 512, 513, 1000, 2047, 2048, 2049, 4096, 4097)


def sdr_pairs(L):
    return _pairs(3, L, 16000, L)


def sdr_levinson(ref, est, clamp_db=50.0, nl=512):
    """float64 transcription of csrc/metrics.hip's SDR: time-domain correlations for `nl` lags (xcorr_kernel), then
    sdr_solve_kernel's Levinson recursion, statement for statement (f = forward vector, x = solution, both grown by one per step)."""
    r = np.asarray(ref, dtype=np.float64)
    e = np.asarray(est, dtype=np.float64)
    L = len(r)
    rp, ep = np.concatenate([r, np.zeros(nl)]), np.concatenate([e, np.zeros(nl)])
    acf = np.array([np.dot(r, rp[k:k + L]) for k in range(nl)])
    xc = np.array([np.dot(r, ep[k:k + L]) for k in range(nl)])
    nr, ne = max(np.sqrt(np.dot(r, r)), 1e-6), max(np.sqrt(np.dot(e, e)), 1e-6)
    t, b = acf / (nr * nr), xc / (nr * ne)
    f, x = np.zeros(nl), np.zeros(nl)
    f[0] = 1.0 / t[0]
    x[0] = b[0] / t[0]
    for k in range(1, nl):
        ef = np.dot(t[k:0:-1], f[:k])
        ex = np.dot(t[k:0:-1], x[:k])
        den = 1.0 / (1.0 - ef * ef)
        fi = np.concatenate([f[:k], [0.0]])
        bi = np.concatenate([[0.0], f[:k][::-1]])
        fnew = den * fi - ef * den * bi
        f[:k + 1] = fnew
        x[:k + 1] = np.concatenate([x[:k], [0.0]]) + (b[k] - ex) * fnew[::-1]
    coh = float(np.dot(b, x))
    eps = 10.0 ** (-clamp_db / 10.0)
    eps = eps / (1.0 + eps)
    coh = min(max(coh, eps), 1.0 - eps)
    return 10.0 * np.log10(coh / (1.0 - coh))


def resample_ratio(fs_in, fs_out):
    g = gcd(fs_in, fs_out)
    return fs_out // g, fs_in // g
