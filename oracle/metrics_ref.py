"""Oracle: intrusive metrics of ``evaluation_metrics/calculate_intrusive_se_metrics.py`` on CPU.

TEST INFRASTRUCTURE - never imported by the product path.

``estoi_metric`` (:37-48) -> ``pystoi.stoi(ref, inf, fs_sig=fs, extended=True)`` (pystoi==0.4.1, requirements.txt:2);
``sdr_metric`` (:90-109) -> ``fast_bss_eval.bss_eval_sources(ref, inf, compute_permutation=False, clamp_db=50)``.
Neither package is on disk: both are restated here from their published algorithms on numpy +
``scipy.signal.resample_poly`` (the routine pystoi itself calls).  Parity with the real packages: unpinned by the
reference (no vectors); self-consistency checks live in tests/test_oracle.py (filter specification, scipy cross-checks)
and tests/test_metrics_cpu.py (pystoi's dither against the zero rule, the Levinson recursion against the dense solve).
"""
import numpy as np
from scipy.signal import resample_poly

FS = 10000
N_FRAME = 256
NFFT = 512
NUMBAND = 15
MINFREQ = 150
N = 30
DYN_RANGE = 40
EPS = np.finfo("float").eps


def resample_window_oct(p, q):
    """pystoi.utils._resample_window_oct: Kaiser-windowed sinc, Octave compatible."""
    g = np.gcd(p, q)
    p, q = p // g, q // g
    stopband_cutoff_f = 1.0 / (2 * max(p, q))
    roll_off_width = stopband_cutoff_f / 10
    rejection_db = 60.0
    L = int(np.ceil((rejection_db - 8) / (28.714 * roll_off_width)))
    t = np.arange(-L, L + 1)
    ideal = 2 * p * stopband_cutoff_f * np.sinc(2 * stopband_cutoff_f * t)
    beta = 0.1102 * (rejection_db - 8.7)
    return np.kaiser(2 * L + 1, beta) * ideal, p, q


def resample_oct(x, p, q):
    h, pr, qr = resample_window_oct(p, q)
    return resample_poly(x, pr, qr, window=h / np.sum(h))


def thirdoct(fs, nfft, num_bands, min_freq):
    f = np.linspace(0, fs, nfft + 1)[: nfft // 2 + 1]
    k = np.arange(num_bands).astype(float)
    cf = np.power(2.0 ** (1.0 / 3), k) * min_freq
    freq_low = min_freq * np.power(2.0, (2 * k - 1) / 6)
    freq_high = min_freq * np.power(2.0, (2 * k + 1) / 6)
    obm = np.zeros((num_bands, len(f)))
    lo, hi = [], []
    for i in range(len(cf)):
        fl = int(np.argmin(np.square(f - freq_low[i])))
        fh = int(np.argmin(np.square(f - freq_high[i])))
        obm[i, fl:fh] = 1
        lo.append(fl)
        hi.append(fh)
    return obm, cf, lo, hi


# pystoi's frame loops are ``range(0, len(x) - framelen, hop)`` (which records the package's code: "last full frame
# excluded - keep the off-by-one"): a signal of exactly framelen + k * hop samples has k frames, not k + 1.  That is the reading this
# oracle and the kernels implement.  LAST_FRAME_INCLUSIVE = True switches the oracle to the other reading (``len - framelen + 1``)
# so that tests/test_metrics_gpu.py::test_estoi_frame_range_at_the_boundary_length can show, on a length = 256 mod 128 fixture,
# which one the kernels follow and what the difference is worth (one frame; a few 1e-4 of ESTOI on a 2.6 s signal).
LAST_FRAME_INCLUSIVE = False


def _frames(x, framelen, hop):
    w = np.hanning(framelen + 2)[1:-1]
    idx = list(range(0, len(x) - framelen + (1 if LAST_FRAME_INCLUSIVE else 0), hop))
    return np.array([w * x[i:i + framelen] for i in idx]).reshape(len(idx), framelen)


def _overlap_and_add(frames, hop):
    n, fl = frames.shape
    out = np.zeros((n - 1) * hop + fl if n > 0 else 0)
    for i in range(n):
        out[i * hop:i * hop + fl] += frames[i]
    return out


def remove_silent_frames(x, y, dyn_range, framelen, hop):
    xf, yf = _frames(x, framelen, hop), _frames(y, framelen, hop)
    energies = 20 * np.log10(np.linalg.norm(xf, axis=1) + EPS)
    mask = (np.max(energies) - dyn_range - energies) < 0
    return _overlap_and_add(xf[mask], hop), _overlap_and_add(yf[mask], hop), mask


def stft_tob(x, obm):
    fr = _frames(x, N_FRAME, N_FRAME // 2)
    spec = np.fft.rfft(fr, n=NFFT).T            # [257, M]
    return np.sqrt(np.matmul(obm, np.square(np.abs(spec))))


# A column of a segment is degenerate where its 15 normalised rows agree: in exact arithmetic its centred sum of squares is 0, in
# float64 it is what rounding leaves, <= 1.2e-30 on every fixture of tests/test_metrics_cpu.py (entries of unit-norm rows are <= 1, their
# rounding ~1e-16, 15 of them squared).  That happens beside every silent stretch of the estimate: a segment with ONE audible frame and
# 29 silent ones has the same row [-a ... -a, 29 a] in every band.  Every other column of the same fixtures has a sum of squares of
# 2.5e-5 or more (1.4e-3 on the regular ones), so any threshold between the two does; it is absolute because the rows are normalised.  (The rows themselves are not: there the rule
# is the exact zero, which is what a silent band gives.)
COL_SS_MIN = 1e-24


def _unit_norm(xn, axis, ss_min):
    ss = np.sum(np.square(xn), axis=axis, keepdims=True)
    if ss_min is None:                           # the bare formula
        with np.errstate(divide="ignore", invalid="ignore"):
            return xn / np.sqrt(ss)
    ok = ss > ss_min
    if np.all(ok):
        return xn / np.sqrt(ss)
    return np.where(ok, xn / np.sqrt(np.where(ok, ss, 1.0)), 0.0)


def row_col_normalize(x, degenerate="zero", dither_rng=None):
    """pystoi.utils.row_col_normalize on x [J, 15, 30]: each row (last axis) to zero mean and unit norm, then each column (axis 1).

    pystoi adds ``EPS * randn`` (EPS = 2.2e-16) to x before the row step and again before the column step; that is why the
    reference script seeds numpy.  ``dither_rng`` (anything with ``standard_normal(shape)``: a ``numpy.random.Generator`` or
    ``RandomState``) restates those two additions, and then the formula is pystoi's, with no rule on top.  Without it there is no
    dither, and a row or column whose centred sum of squares is 0 - an estimate that is exactly silent in a band for 30 frames,
    or for 29 of them (COL_SS_MIN) - would be 0 / 0 or normalised rounding noise.  ``degenerate="zero"`` (the rule the kernels
    follow) makes such a row or column all zeros; ``degenerate="nan"`` is the bare formula.  Where nothing is degenerate the two
    are the same arithmetic, bit for bit.  What the dither is worth against the rule, on both kinds of input, is measured in
    tests/test_metrics_cpu.py."""
    assert degenerate in ("zero", "nan")
    rule = degenerate == "zero" and dither_rng is None
    if dither_rng is not None:
        x = x + EPS * dither_rng.standard_normal(x.shape)
    xn = x - np.mean(x, axis=-1, keepdims=True)
    xn = _unit_norm(xn, -1, 0.0 if rule else None)
    if dither_rng is not None:
        xn = xn + EPS * dither_rng.standard_normal(xn.shape)
    xn = xn - np.mean(xn, axis=1, keepdims=True)
    xn = _unit_norm(xn, 1, COL_SS_MIN if rule else None)
    return xn


def estoi(x, y, fs_sig, degenerate="zero", dither_rng=None):
    """pystoi.stoi(x, y, fs_sig, extended=True); x = clean, y = processed.  degenerate / dither_rng: see row_col_normalize
    (x is normalised before y, so with a dither the draws go to x's rows, x's columns, y's rows, y's columns, as in pystoi)."""
    seg = estoi_segments(x, y, fs_sig)
    if seg is None:
        return 1e-5            # pystoi warns "Not enough STFT frames" and returns 1e-5
    xs, ys = seg
    xn, yn = row_col_normalize(xs, degenerate, dither_rng), row_col_normalize(ys, degenerate, dither_rng)
    return float(np.sum(xn * yn / N) / xn.shape[0])


def estoi_segments(x, y, fs_sig):
    """Everything of ``estoi`` in front of the normalisation: the third-octave segments (xs, ys), each [J, 15, 30], or None
    where fewer than 30 frames are left."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    assert x.shape == y.shape
    if fs_sig != FS:
        x = resample_oct(x, FS, fs_sig)
        y = resample_oct(y, FS, fs_sig)
    x, y, _ = remove_silent_frames(x, y, DYN_RANGE, N_FRAME, N_FRAME // 2)
    obm = thirdoct(FS, NFFT, NUMBAND, MINFREQ)[0]
    x_tob, y_tob = stft_tob(x, obm), stft_tob(y, obm)
    M = x_tob.shape[1]
    if M < N:
        return None
    xs = np.array([x_tob[:, m - N:m] for m in range(N, M + 1)])
    ys = np.array([y_tob[:, m - N:m] for m in range(N, M + 1)])
    return xs, ys


def sdr(ref, est, filter_length=512, clamp_db=50.0):
    """fast_bss_eval.bss_eval_sources for one source: SDR in dB (SIR = inf, SAR = SDR)."""
    ref = np.asarray(ref, dtype=np.float64).reshape(-1)
    est = np.asarray(est, dtype=np.float64).reshape(-1)
    ref = ref / max(np.linalg.norm(ref), 1e-6)
    est = est / max(np.linalg.norm(est), 1e-6)
    n = 2 ** int(np.ceil(np.log2(len(ref) + filter_length - 1)))
    R, E = np.fft.rfft(ref, n), np.fft.rfft(est, n)
    acf = np.fft.irfft(R.conj() * R, n)[:filter_length]
    xcorr = np.fft.irfft(R.conj() * E, n)[:filter_length]
    idx = np.abs(np.arange(filter_length)[:, None] - np.arange(filter_length)[None, :])
    sol = np.linalg.solve(acf[idx], xcorr)
    coh = float(np.dot(xcorr, sol))
    e = 10.0 ** (-clamp_db / 10.0)
    eps = e / (1.0 + e)
    coh = min(max(coh, eps), 1.0 - eps)
    return 10.0 * np.log10(coh / (1.0 - coh))


# ---- soxr HQ specification resampler (stand-in for soxr.resample / librosa res_type="soxr_hq") -----------------------------------
def soxr_hq_design(fs_in, fs_out):
    """One Kaiser-windowed sinc built to the specification of libsoxr's HQ recipe (soxr.c soxr_quality_spec, quality 4: 20-bit =
    120.4 dB rejection from the lower Nyquist frequency, pass band to 1 - 0.05 / TO_3dB(rej) = 0.9136 of it, linear phase,
    cutoff mid-transition as lsx_design_lpf places it).  -> (h with unity DC gain, up, down).  soxr's own cascade is not reproducible
    bit-wise; what is pinned here is the specification, checked in tests/test_oracle.py."""
    from math import gcd
    from scipy.signal import firwin
    g = gcd(int(fs_in), int(fs_out))
    up, down = int(fs_out) // g, int(fs_in) // g
    rej = 20 * 20.0 * np.log10(2.0)
    to3db = (1.6e-6 * rej - 7.5e-4) * rej + 0.646
    nyq = 0.5 * min(fs_in, fs_out)
    f_pass, f_stop = (1.0 - 0.05 / to3db) * nyq, nyq
    fs_work = float(fs_in) * up
    dw = 2.0 * np.pi * (f_stop - f_pass) / fs_work
    att = rej + 2.0          # design margin: Kaiser's length estimate lands 1.3 dB short at the very band edges for the 80 k-tap filters
    half = int(np.ceil((att - 7.95) / (2.285 * dw) / 2.0))
    h = firwin(2 * half + 1, (f_pass + f_stop) / fs_work, window=("kaiser", 0.1102 * (att - 8.7)))
    return h, up, down


def resample_soxr_hq_spec(x, fs_in, fs_out):
    h, up, down = soxr_hq_design(fs_in, fs_out)
    return resample_poly(np.asarray(x, dtype=np.float64), up, down, window=h)     # (scipy scales the taps by `up` itself)
