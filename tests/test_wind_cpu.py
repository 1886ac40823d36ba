"""CPU: the float64 restatement of the wind-noise side-chain compressor (tests/wind_ref.py) against closed forms that hold whether or not
the restatement of ffmpeg's filter is right, the sensitivity of its 16-bit rounding decisions to the last bit of its float32 inputs (the cap
tests/test_wind_gpu.py relies on), and the opt-in parsing of a wind row of meta.tsv."""
import numpy as np
import pytest

from tests import wind_ref as wr


def _signals(n, seed, noise_scale=0.3):
    rng = np.random.default_rng(seed)
    x = (0.25 * rng.standard_normal(n)).astype(np.float32)
    v = (noise_scale * rng.standard_normal(n)).astype(np.float32)
    return x, v


def test_ratio_one_is_a_plain_average():
    """(a) ratio 1: the line above the knee is gain = slope and the Hermite joins (knee_start, knee_start) to (knee_stop, knee_stop) with slope 1
    at both ends, so g = 1.  In floating point (slope - thres) / 1 + thres and the cubic's four terms return slope up to a few units in its
    last place (|slope| < 8: 2^-50 absolute), so g = exp(that) = 1 up to 1e-14 - and mq = Q(0.5 xq + 0.5 vq) wherever that rounding is not
    decided by less than 1e-9 of a step (elsewhere: within one step)."""
    x, v = _signals(5000, 1)
    r = wr.wind_mix(x, v, x, 16000, 0.1, 1.0, 20.0, 50.0, 1.0, 0.9, True)
    assert r["S"].max() > r["setup"]["lin_knee_stop"] ** 2 and r["S"].min() < r["setup"]["adj_knee_start"]        # all three regions
    assert np.abs(r["g"] - 1.0).max() <= 1e-14
    plain = 0.5 * r["xq"] + 0.5 * r["vq"]
    tie = wr.near_tie(plain)
    assert np.array_equal(r["mq"][~tie], wr.q16(plain)[~tie])
    assert np.abs(r["mq"] - wr.q16(plain)).max() <= 2.0 ** -15
    assert (~tie).mean() > 0.4


def test_silent_side_chain_leaves_the_speech_alone():
    """(b) an all-zero noise: S stays 0, g is exactly 1, the mixture is the halved, re-quantised speech"""
    x, _ = _signals(3000, 2)
    r = wr.wind_mix(x, np.zeros_like(x), x, 16000, 0.1, 7.9, 20.0, 50.0, 1.2, 0.95, False)
    assert np.all(r["S"] == 0.0) and np.all(r["g"] == 1.0)
    assert np.array_equal(r["mq"], wr.q16(0.5 * r["xq"]))
    c = 0.9 / np.abs(x.astype(np.float64)).max()
    assert r["c"] == c and np.array_equal(r["speech"], c * x.astype(np.float64)) and np.all(r["noise"] == 0.0)
    mix = r["mq"] / c
    lo = 0.95 * mix.min()
    want = np.minimum(np.maximum(mix, lo), 0.95 * max(mix.max(), lo))
    assert np.array_equal(r["noisy"], want) and (r["noisy"] != mix).sum() >= 2          # both clipper bounds bite


def test_constant_side_chain_follows_the_geometric_attack():
    """(c) vq = k: S_t = (k sc_gain)^2 (1 - (1 - ka)^(t + 1)); past lin_knee_stop^2 the gain is the ratio's line,
    g_t = exp((0.5 ln S_t - thres) (1 / ratio - 1))"""
    n, fs, threshold, ratio, attack, sc_gain = 4000, 16000, 0.05, 7.9, 100.0, 1.1
    x, _ = _signals(n, 3)
    v = np.full(n, 0.12, dtype=np.float32)
    r = wr.wind_mix(x, v, x, fs, threshold, ratio, attack, 50.0, sc_gain, 0.9, True)
    k = r["vq"][0]
    assert np.all(r["vq"] == k)
    ka = 1.0 / (attack * fs / 4000.0)
    t = np.arange(n, dtype=np.float64)
    S = (k * sc_gain) ** 2 * (1.0 - (1.0 - ka) ** (t + 1.0))
    assert np.allclose(r["S"], S, rtol=1e-11, atol=0.0)
    above = S > r["setup"]["lin_knee_stop"] ** 2
    assert 100 < above.sum() < n - 20
    g = np.exp((0.5 * np.log(S[above]) - np.log(threshold)) * (1.0 / ratio - 1.0))
    assert np.allclose(r["g"][above], g, rtol=1e-11, atol=0.0)
    assert np.all(r["g"][S <= r["setup"]["adj_knee_start"]] == 1.0)


@pytest.mark.parametrize("ratio", [1.0, 7.9, 20.0])
def test_knee_meets_both_straight_segments(ratio):
    """(d) at knee_start the Hermite has the value and the slope of the identity below the knee, at knee_stop those of the ratio's line"""
    s = wr.setup(0.2, ratio, 10.0, 10.0, 16000)
    line = lambda z: (z - s["thres"]) / s["ratio"] + s["thres"]
    assert abs(float(wr.log_gain(s["knee_start"], s)) - s["knee_start"]) < 1e-13
    inside = np.nextafter(s["knee_stop"], -np.inf)
    assert abs(float(wr.log_gain(inside, s)) - line(s["knee_stop"])) < 1e-13
    assert float(wr.log_gain(s["knee_stop"], s)) == line(s["knee_stop"])
    h = 1e-5
    d0 = (wr.log_gain(s["knee_start"] + h, s) - wr.log_gain(s["knee_start"], s)) / h
    d1 = (wr.log_gain(inside, s) - wr.log_gain(inside - h, s)) / h
    assert abs(d0 - 1.0) < 1e-4 and abs(d1 - 1.0 / ratio) < 1e-4         # (one-sided differences of a cubic: O(h) off)
    assert np.all(np.diff(wr.log_gain(np.linspace(s["knee_start"], inside, 200), s)) > 0)
    assert wr.gain(np.array([s["adj_knee_start"]]), s)[0] == 1.0          # the knee starts strictly above adj_knee_start


def test_last_bit_of_the_inputs_moves_few_rounding_decisions(lib):
    """What tests/test_wind_gpu.py's cap of 1 differing sample in 1,000 has to absorb is far smaller than this: the kernel gets the SAME float32
    inputs as the oracle, and differs from it by the last bits of ln / exp only.  Here every input sample but the one that carries the row's peak
    moves by one float32 unit in the last place (the peak fixes c, which scales every sample of the row at once - a different input, not a
    rounding decision).  Measured on the batch of wind_ref.kernel_cases (chunk 1024): 0.00098 of the samples on the 1023-sample row (one
    sample), 0.00032 on the 3089-sample rows (one sample), none on the others; the assertion is the cap itself, on rows of 1,000 samples and more
    (a shorter row cannot hold "1 in 1,000"); every moved sample moves by exactly one 16-bit step."""
    from urgent2026_challenge_track1_amd import mixing
    cs = wr.kernel_cases(mixing.wind_chunk())
    base = wr.run_cases(cs)
    rng = np.random.default_rng(7)

    def nudge(a, keep):
        up = rng.integers(0, 2, size=a.shape).astype(bool)
        out = np.where(up, np.nextafter(a, np.float32(np.inf)), np.nextafter(a, np.float32(-np.inf))).astype(np.float32)
        out[keep] = a[keep]
        return out
    keep = np.zeros(cs["x"].shape, dtype=bool)
    for b in cs["wind"]:
        n = cs["lens"][b]
        row = np.maximum(np.abs(cs["x"][b, :n]), np.abs(cs["noise"][b, :n]))
        keep[b, int(np.argmax(row))] = True
    moved = wr.run_cases(cs, nudge(cs["x"], keep), nudge(cs["noise"], keep))
    for b in cs["wind"]:
        assert moved[b]["c"] == base[b]["c"]
        for kind in ("noisy", "noise"):
            d = np.abs(moved[b][kind] - base[b][kind])
            share = float((d > wr.f32_step(base[b][kind])).mean())
            print("row %d (%d samples) %s: %.5f of the samples move by a 16-bit step" % (b, cs["lens"][b], kind, share))
            assert d.max() <= 2.0 ** -15 / base[b]["c"] * (1 + 1e-9)
            if cs["lens"][b] >= 1000:
                assert share <= 1e-3, (b, kind, share)


WIND_ROW = dict(id="fileid_3", noise_uid="wind_noise48000_1", snr_dB="2.5", fs="16000", length="5000", rir_uid="none",
                augmentation="wind_noise(threshold=0.2,ratio=7.9,attack=57.5,release=23.6,sc_gain=0.87,clipping=False,clipping_threshold=0.9)/"
                             "bandwidth_limitation-polyphase->8000")


def test_default_parse_of_a_wind_row_is_unchanged():
    from urgent2026_challenge_track1_amd import simulate_data_from_param as sdp
    recipe, lacking = sdp.parse_row(WIND_ROW, False)
    assert lacking == ["wind_noise"] and recipe["wind"] and recipe["order"] == ["bandwidth_limitation"] and recipe["highpass"] is False
    assert recipe == dict(id="fileid_3", snr=2.5, params=dict(bandwidth_limitation=dict(res_type="polyphase", fs_new=8000)),
                          order=["bandwidth_limitation"], wind=True, highpass=False, fs=16000, length=5000)


def test_opt_in_parse_of_a_wind_row_reads_the_seven_fields():
    from urgent2026_challenge_track1_amd import simulate_data_from_param as sdp
    recipe, lacking = sdp.parse_row(WIND_ROW, False, wind_compressor=True)
    assert lacking == [] and recipe["wind"] and recipe["order"] == ["bandwidth_limitation"]
    assert recipe["params"]["wind_noise"] == dict(threshold=0.2, ratio=7.9, attack=57.5, release=23.6, sc_gain=0.87, clipping=True,
                                                  clipping_threshold=0.9)          # (clipping: bool("False") is true, as in the reference)
    assert recipe["params"]["bandwidth_limitation"] == dict(res_type="polyphase", fs_new=8000)
    plain = dict(WIND_ROW, noise_uid="nz", augmentation="clipping(min=0.1,max=0.9)")
    assert sdp.parse_row(plain, True, wind_compressor=True) == sdp.parse_row(plain, True)
    assert sdp.get_parser().parse_args(["--meta_tsv", "m"]).wind_noise_compressor == "skip"
    assert sdp.get_parser().parse_args(["--meta_tsv", "m", "--wind_noise_compressor", "device"]).wind_noise_compressor == "device"


def test_config_switch_defaults_to_skip():
    from urgent2026_challenge_track1_amd import train_se
    from urgent2026_challenge_track1_amd.config import Config
    assert Config().wind_noise_compressor == "skip" and train_se.wind_compressor_on(Config()) is False
    assert train_se.wind_compressor_on(Config(wind_noise_compressor="device")) is True
    with pytest.raises(ValueError):
        train_se.wind_compressor_on(Config(wind_noise_compressor="ffmpeg"))


def test_wind_entry_refuses_bad_arguments_without_touching_the_gpu(lib):
    import ctypes
    p = ctypes.c_void_p
    assert lib.urse_wind_chunk() >= 64
    assert lib.urse_wind_mix(None, None, None, None, None, 1, 8, None, 0, None, None, None) == -1 and b"urse_wind_mix" in lib.urse_last_error()
    assert lib.urse_wind_mix(p(64), p(128), p(192), p(256), p(320), 2, 8, None, 1, None, None, None) == -1          # rows listed, no list
    assert lib.urse_wind_mix(p(64), p(128), p(192), p(256), p(320), 2, 8, p(384), 3, p(448), None, None) == -1      # more rows than the batch has
    assert lib.urse_wind_mix(p(64), p(128), p(192), p(128), p(320), 2, 8, p(384), 1, p(448), None, None) == -1      # noisy is x
    assert b"buffers of their own" in lib.urse_last_error()
    assert lib.urse_wind_mix(p(64), p(64), p(192), p(256), p(320), 2, 8, None, 0, None, None, None) == 0            # no rows: nothing to launch
