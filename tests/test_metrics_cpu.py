"""CPU checks of the metrics oracle (oracle/metrics_ref.py) at the inputs where pystoi's ``EPS * randn`` dither decides the value, and
of the SDR kernel's Levinson recursion (restated in float64 numpy) against the oracle's dense solve.  No GPU, no kernel: what is pinned
here is the reference the GPU tests of tests/test_metrics_gpu.py compare against."""
import numpy as np
import pytest

from oracle import metrics_ref
from tests import metrics_cases as mc
from tests.test_metrics_gpu import _pairs

SEEDS = range(32)


def _old_row_col_normalize(x):
    """the oracle's formula before the degenerate rule (no dither, no guard)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        xn = x - np.mean(x, axis=-1, keepdims=True)
        xn = xn / np.sqrt(np.sum(np.square(xn), axis=-1, keepdims=True))
        xn = xn - np.mean(xn, axis=1, keepdims=True)
        xn = xn / np.sqrt(np.sum(np.square(xn), axis=1, keepdims=True))
    return xn


def _old_estoi(seg):
    if seg is None:
        return 1e-5
    xn, yn = _old_row_col_normalize(seg[0]), _old_row_col_normalize(seg[1])
    return float(np.sum(xn * yn / metrics_ref.N) / xn.shape[0])


def _dithered(seg, seed=None):
    """the score of estoi_segments' output under pystoi's dither with numpy's global stream seeded `seed` (the reference script seeds
    it); None: no dither, the zero rule (== metrics_ref.estoi, asserted in the first test)"""
    rng = None if seed is None else np.random.RandomState(seed)
    xn, yn = metrics_ref.row_col_normalize(seg[0], dither_rng=rng), metrics_ref.row_col_normalize(seg[1], dither_rng=rng)
    return float(np.sum(xn * yn / metrics_ref.N) / xn.shape[0])


def _boundary_pairs():
    L = 256 + 128 * 200
    ref, inf = _pairs(3, L, 10000, 31)
    ref[:, -int(0.08 * L):] = ref[:, int(0.3 * L):int(0.3 * L) + int(0.08 * L)]
    inf[:, -int(0.08 * L):] = inf[:, int(0.3 * L):int(0.3 * L) + int(0.08 * L)]
    return ref, inf


def _regular_fixtures():
    """every ESTOI fixture of tests/test_metrics_gpu.py built from _pairs: (name, fs, ref, inf)"""
    out = []
    for fs, L in [(16000, 32000), (48000, 60000), (10000, 20000), (8000, 12345)]:
        out.append(("oracle %d/%d" % (fs, L), fs) + _pairs(4, L, fs, fs + L))
    out.append(("too short", 16000) + _pairs(2, 3000, 16000, 1))
    ref, _ = _pairs(2, 32000, 16000, 2)
    out.append(("identical", 16000, ref, ref.copy()))
    out.append(("driver", 16000) + _pairs(3, 20000, 16000, 9))
    out.append(("boundary", 10000) + _boundary_pairs())
    out.append(("two streams", 16000) + _pairs(37, 24000, 16000, 41))
    return out


@pytest.fixture(scope="module")
def regular_segments():
    return [(name, [metrics_ref.estoi_segments(ref[p], inf[p], fs) for p in range(len(ref))], fs, ref, inf)
            for name, fs, ref, inf in _regular_fixtures()]


@pytest.fixture(scope="module")
def degenerate_segments():
    out = []
    for fs, L in mc.DEGENERATE:
        ref, inf = mc.degenerate_pairs(fs, L)
        out.append((fs, L, [metrics_ref.estoi_segments(ref[p], inf[p], fs) for p in range(3)], ref, inf))
    return out


def test_zero_rule_is_bit_equal_to_the_old_formula_on_the_regular_fixtures(regular_segments):
    n = 0
    for name, segs, fs, ref, inf in regular_segments:
        for p, seg in enumerate(segs):
            new, old = metrics_ref.estoi(ref[p], inf[p], fs), _old_estoi(seg)
            assert np.isfinite(old) and new == old, (name, p, new, old)
            assert seg is None or _dithered(seg) == new
            if seg is not None:
                for s in seg:
                    assert np.array_equal(metrics_ref.row_col_normalize(s), _old_row_col_normalize(s)), (name, p)
                    assert np.array_equal(metrics_ref.row_col_normalize(s, degenerate="nan"), _old_row_col_normalize(s)), (name, p)
            n += 1
    assert n == 16 + 2 + 2 + 3 + 3 + 37


def test_degenerate_fixtures_are_nan_under_the_old_formula(degenerate_segments):
    """guards the fixtures: each must hold a 30-frame band row of exact zeros, after the 16 -> 10 kHz resampler too"""
    for fs, L, segs, ref, inf in degenerate_segments:
        a, b = mc.zero_interior_after_resampling(fs, L)
        assert b - a >= 29 * 128 + 256 + 128                     # room for a whole segment wherever the frame grid falls
        if fs != metrics_ref.FS:
            y = metrics_ref.resample_oct(inf[0].astype(np.float64), metrics_ref.FS, fs)
            assert not np.any(y[a:b]) and np.any(y[a - 40:a]) and np.any(y[b:b + 40])
        for p, seg in enumerate(segs):
            assert np.isnan(_old_estoi(seg)), (fs, L, p)
            assert np.isnan(metrics_ref.estoi(ref[p], inf[p], fs, degenerate="nan"))
            assert np.isfinite(metrics_ref.estoi(ref[p], inf[p], fs))


def test_column_threshold_sits_in_a_wide_gap(regular_segments, degenerate_segments):
    """metrics_ref.COL_SS_MIN (1e-24, the kernel's constant too) separates columns that are 0 in exact arithmetic from all others: on
    every fixture the centred sums of squares of the row-normalised columns are either rounding (measured <= 1.3e-30: the two
    segments beside each silent stretch that hold ONE audible frame) or >= 2.5e-5 (>= 1.4e-3 on the regular fixtures); nothing may
    come within four decades of the threshold from either side."""
    lo, hi, n_deg = 0.0, np.inf, 0
    segs = [s for _, ss, _, _, _ in regular_segments for s in ss] + [s for _, _, ss, _, _ in degenerate_segments for s in ss]
    for seg in segs:
        for s in seg or ():
            xn = metrics_ref._unit_norm(s - np.mean(s, axis=-1, keepdims=True), -1, 0.0)
            c = np.sum(np.square(xn - np.mean(xn, axis=1, keepdims=True)), axis=1).ravel()
            c = c[c > 0]
            small = c[c <= metrics_ref.COL_SS_MIN]
            n_deg += len(small)
            lo, hi = max(lo, small.max(initial=0.0)), min(hi, c[c > metrics_ref.COL_SS_MIN].min())
    print("column sums of squares: %d of rounding size, largest %.1e; smallest of all others %.1e" % (n_deg, lo, hi))
    assert n_deg > 0 and lo <= 1e-28 and hi >= 1e-20


def test_zero_rule_lies_inside_the_spread_of_pystois_dither(degenerate_segments):
    """pystoi's answer on a degenerate input is a random variable (the normalised dither of the silent rows); the deterministic zero
    rule must be one of the values it could have returned: inside the min - max of seeds 0..31.
    Measured: sd of the 32 draws 1.2e-3 .. 5.1e-3 over the twelve pairs (smaller on the longer signals, where fewer of the segments
    are degenerate); the rule sits 0.00 .. 0.18 sd from their mean, e.g. 0.46826 inside 0.46521 .. 0.47104 (10 kHz, L = 30000, pair 0)."""
    worst = 0.0
    for fs, L, segs, ref, inf in degenerate_segments:
        for p, seg in enumerate(segs):
            rule = metrics_ref.estoi(ref[p], inf[p], fs)
            d = np.array([_dithered(seg, s) for s in SEEDS])
            z = abs(rule - d.mean()) / d.std()
            worst = max(worst, z)
            print("fs %5d L %5d pair %d: zero rule %.5f, dither min %.5f max %.5f mean %.5f sd %.1e (rule at %.2f sd)"
                  % (fs, L, p, rule, d.min(), d.max(), d.mean(), d.std(), z))
            assert d.min() <= rule <= d.max(), (fs, L, p, rule, d.min(), d.max())
    print("zero rule: at most %.2f sd from the mean of pystoi's dither" % worst)


def test_all_zero_estimate_scores_zero(degenerate_segments):
    """every row of the estimate degenerate: the rule gives exactly 0.0, the dither a correlation of pure noise (measured: within +-0.02, sd 3.3e-3 .. 8.2e-3)"""
    for fs, L, segs, ref, inf in degenerate_segments:
        z = np.zeros_like(ref[0])
        assert metrics_ref.estoi(ref[0], z, fs) == 0.0
        seg = metrics_ref.estoi_segments(ref[0], z, fs)
        d = np.array([_dithered(seg, s) for s in SEEDS])
        print("fs %5d L %5d all-zero estimate: zero rule 0.0, dither min %.4f max %.4f sd %.1e" % (fs, L, d.min(), d.max(), d.std()))
        assert d.min() < 0.0 < d.max() and np.abs(d).max() < 0.1


def test_dither_is_irrelevant_off_the_degenerate_case(regular_segments):
    """SURVEY A.7's "EPS = 2.2e-16, irrelevant at 1e-4", measured: on every regular fixture the dither moves the score by far less than
    the 1e-4 parity tolerance of the GPU tests.  Measured maximum over the 64 scored pairs x seeds 0..7: 3.3e-16."""
    worst = 0.0
    for name, segs, fs, ref, inf in regular_segments:
        for p, seg in enumerate(segs):
            if seg is None:
                continue
            base = _dithered(seg)
            worst = max(worst, max(abs(_dithered(seg, s) - base) for s in range(8)))
    print("dither shift on the regular fixtures: max %.1e" % worst)
    assert worst < 1e-4             # measured 3.3e-16: float64 rounding


@pytest.mark.parametrize("L", mc.LEVINSON_LENGTHS)
def test_levinson_transcription_matches_the_dense_solve(L):
    """the recursion sdr_solve_kernel runs, in float64 numpy, against metrics_ref.sdr (FFT correlations + numpy.linalg.solve):
    1e-9 dB; measured maximum 1.9e-12 dB (L = 4097).  A zero estimate clamps to exactly -50 dB in both."""
    ref, inf = mc.sdr_pairs(L)
    for p in range(3):
        a, b = mc.sdr_levinson(ref[p], inf[p]), metrics_ref.sdr(ref[p], inf[p])
        print("L %4d pair %d: levinson %.12f dB, solve %.12f dB, diff %.1e" % (L, p, a, b, abs(a - b)))
        assert abs(a - b) <= 1e-9
    z = np.zeros_like(ref[0])
    assert abs(mc.sdr_levinson(ref[0], z) + 50.0) <= 1e-9 and abs(metrics_ref.sdr(ref[0], z) + 50.0) <= 1e-9
