"""GPU: the bandwidth estimate on the device against the reference's own results (tests/golden/ref_bandwidth*.npz, written by
tests/golden/make_golden_bandwidth.py from utils/estimate_audio_bandwidth.py::estimate_bandwidth): the mean power spectrum, the
chosen bin of EVERY fixture case, run-to-run bit identity, both entry points end to end, and the unsupported frame sizes.

Mean-power tolerance.  The yardstick is the fixture's ``f32_cpu_rel_err`` = 4.79e-4: the largest relative error of a float32
``torch.stft`` on the CPU against the float64 mean power, over bins within 80 dB of each case's peak.  The device transform is a
different float32 algorithm with another summation order, so a small multiple (at most 8) is allowed.  First GPU run (MI355X):
4.54e-4 = 0.95 x the yardstick (per rate 2.5e-5 / 5.7e-5 / 2.1e-4 / 5.3e-5 / 2.0e-4 / 4.5e-4 / 2.4e-4 from 8 to 48 kHz; 44.1 kHz, the
Bluestein transform through 2880 points, is the largest) -> POWER_TOL_MULT = 2."""
import json
import os
import struct

import numpy as np
import pytest
import torch

from tests import parity_log

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000)
POWER_TOL_MULT = 2.0


@pytest.fixture(scope="module")
def cases():
    z = np.load(os.path.join(GOLD, "ref_bandwidth.npz"))
    wav = {}
    for fs in RATES:
        with np.load(os.path.join(GOLD, "ref_bandwidth_wav%d.npz" % fs)) as w:
            wav.update({k: w[k] for k in w.files})
    out = []
    for k in range(len(z["uid"])):
        x = wav["wav_%d" % k]
        seg = z["segment"][k]
        out.append(dict(k=k, uid=str(z["uid"][k]), fs=int(z["fs"][k]), raw=x,
                        x=(x.astype(np.float32) / 32768.0 if x.dtype == np.int16 else x.astype(np.float32)),
                        seg=None if np.isnan(seg[0]) else (float(seg[0]), float(seg[1])),
                        freq=None if np.isnan(z["freq"][k]) else float(z["freq"][k]), bin=int(z["bin"][k]), mp=z["mp_%d" % k]))
    return out, float(z["f32_cpu_rel_err"])


def _analysed(c):
    """the samples the reference analysed: the whole file, or the segment slice in 16 kHz samples"""
    if c["seg"] is None:
        return c["x"]
    return c["x"][:, int(c["seg"][0] * 16000):int(c["seg"][1] * 16000)]


def _pack(group):
    xs = [_analysed(c) for c in group]
    rows, ld = sum(x.shape[0] for x in xs), max(x.shape[1] for x in xs)
    # the padding behind a row's own length is filled with noise: nothing behind `len` may reach the result
    wav = np.random.default_rng(1).standard_normal((rows, ld)).astype(np.float32)
    lens, row_start = [], [0]
    for x in xs:
        r = row_start[-1]
        wav[r:r + x.shape[0], :x.shape[1]] = x
        lens += [x.shape[1]] * x.shape[0]
        row_start.append(r + x.shape[0])
    return torch.from_numpy(wav).cuda(), lens, row_start


def test_mean_power_matches_the_float64_reference(lib, cases):
    """All seven rates, mono and two-channel files, rows of different lengths in one launch per rate.  Measured on an MI355X:
    4.54e-4 against the yardstick's 4.79e-4 (module docstring); recorded through tests/parity_log.py as `bandwidth_mean_power`."""
    from urgent2026_challenge_track1_amd.bandwidth import mean_power_spectrum
    cs, yard = cases
    worst, per_rate = 0.0, {}
    for fs in RATES:
        group = [c for c in cs if c["fs"] == fs and c["bin"] >= 0]
        assert len({_analysed(c).shape[1] for c in group}) > 1 and {c["x"].shape[0] for c in group} == {1, 2}
        wav, lens, row_start = _pack(group)
        mp = mean_power_spectrum(wav, lens, fs).cpu().numpy().astype(np.float64)
        w = 0.0
        for c, r in zip(group, row_start):
            for ch in range(c["mp"].shape[0]):
                ref = c["mp"][ch]
                keep = ref >= ref.max() * 1e-8                       # bins within 80 dB of the peak, as the yardstick
                w = max(w, float((np.abs(mp[r + ch] - ref) / ref)[keep].max()))
        per_rate[str(fs)] = w
        worst = max(worst, w)
    print("mean power: largest relative error %.3e (f32 torch.stft on the CPU: %.3e), per rate %s" % (worst, yard, per_rate))
    parity_log.record("bandwidth_mean_power", rel_err=worst, f32_cpu_rel_err=yard, per_rate=per_rate, bound_multiple=POWER_TOL_MULT)
    assert POWER_TOL_MULT <= 8.0
    assert worst <= POWER_TOL_MULT * yard, (worst, yard, per_rate)


def test_every_fixture_bin_is_reproduced(lib, cases):
    from urgent2026_challenge_track1_amd.bandwidth import estimate_bandwidth_batch
    cs, _ = cases
    seen = 0
    for fs in RATES:
        group = [c for c in cs if c["fs"] == fs]
        wav, lens, row_start = _pack(group)
        bins, bws = estimate_bandwidth_batch(wav, lens, row_start, fs)
        for c, b, bw in zip(group, bins, bws):
            print("case %d %s fs %d: bin %d (reference %d)" % (c["k"], c["uid"], fs, b, c["bin"]))
            assert b == c["bin"] and bw == c["freq"], (c["k"], c["uid"], fs, b, c["bin"], bw, c["freq"])
            seen += 1
    assert seen == len(cs)
    zero = [c for c in cs if c["bin"] < 0]
    assert len(zero) == 1 and not zero[0]["raw"].any()              # the all-zero file gave no bin above


def test_threshold_moves_the_bin(lib, cases):
    """the threshold reaches the kernel: the chosen bin never falls when the threshold is lowered, and the rule of
    estimate_audio_bandwidth.py:45-49 applied on the host to the device's own mean power gives the device's bins"""
    from urgent2026_challenge_track1_amd.bandwidth import mean_power_spectrum, pick_bins
    cs, _ = cases
    group = [c for c in cs if c["fs"] == 22050 and c["bin"] >= 0]
    wav, lens, row_start = _pack(group)
    mp = mean_power_spectrum(wav, lens, 22050)
    prev = None
    for thr in (-20.0, -50.0, -90.0):
        bins = pick_bins(mp, row_start, thr).cpu().tolist()
        h = mp.cpu().numpy().astype(np.float64)
        for p, b in enumerate(bins):
            rows = h[row_start[p]:row_start[p + 1]]
            min_energy = rows.max(1).min() * 10 ** (thr / 10)
            ok = np.nonzero(rows.min(0) > min_energy)[0]
            assert b == (int(ok[-1]) if len(ok) else -1), (thr, p)
        assert prev is None or all(b >= a for a, b in zip(prev, bins))
        prev = bins


def test_two_runs_give_identical_bytes(lib, cases):
    from urgent2026_challenge_track1_amd.bandwidth import mean_power_spectrum
    cs, _ = cases
    for fs in (22050, 44100, 48000):
        wav, lens, _ = _pack([c for c in cs if c["fs"] == fs and c["bin"] >= 0])
        a = mean_power_spectrum(wav, lens, fs).cpu().numpy().tobytes()
        junk = torch.randn(1 << 22, device="cuda")                  # other work between the runs
        junk.mul_(2.0)
        b = mean_power_spectrum(wav, lens, fs).cpu().numpy().tobytes()
        assert a == b, fs


def test_many_short_and_long_rows_in_one_launch(lib):
    """chunking: rows far shorter than the longest one, lengths around the frame size and one sample past a whole number of hops,
    against the float64 definition (reflect padding, periodic Hann, numpy's rfft).  White noise: every bin is near the peak, and
    1e-4 of the peak is three orders above float32 rounding of a 512-point transform, three below any indexing mistake."""
    from urgent2026_challenge_track1_amd.bandwidth import mean_power_spectrum, stft_params
    fs = 16000
    n_fft, hop = stft_params(fs)
    rng = np.random.default_rng(5)
    lens = [257, 300, 511, 512, 513, 4000, 16000, 48001]
    wav = rng.standard_normal((len(lens), max(lens))).astype(np.float32)
    got = mean_power_spectrum(torch.from_numpy(wav).cuda(), lens, fs).cpu().numpy().astype(np.float64)
    win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n_fft) / n_fft)
    for r, n in enumerate(lens):
        x = np.pad(wav[r, :n].astype(np.float64), n_fft // 2, mode="reflect")
        T = 1 + n // hop
        frames = np.stack([x[t * hop:t * hop + n_fft] * win for t in range(T)])
        ref = (np.abs(np.fft.rfft(frames, axis=1)) ** 2).mean(0)
        assert np.abs(got[r] - ref).max() <= 1e-4 * ref.max(), (n, np.abs(got[r] - ref).max() / ref.max())


def _write_wav(path, raw, fs):
    """int16 [C, L] -> PCM_16, float32 [C, L] -> IEEE float WAV, channels interleaved"""
    ch = raw.shape[0]
    if raw.dtype == np.int16:
        pcm, tag, bits = raw.T.astype("<i2").tobytes(), 1, 16
    else:
        pcm, tag, bits = raw.T.astype("<f4").tobytes(), 3, 32
    hdr = struct.pack("<4sI4s4sIHHIIHH4sI", b"RIFF", 36 + len(pcm), b"WAVE", b"fmt ", 16, tag, ch, fs, fs * ch * bits // 8,
                      ch * bits // 8, bits, b"data", len(pcm))
    with open(path, "wb") as f:
        f.write(hdr + pcm)


def test_entry_points_end_to_end(lib, cases, tmp_path):
    """estimate: WAV files written from the fixture -> the reference's JSON values exactly (repeated uid renamed, the all-zero
    file and an unreadable one left out).  resample: the files and the scp it should write; every resampled signal against
    scipy.signal.resample_poly with the same designed taps (oracle/metrics_ref.resample_soxr_hq_spec) to the bound of
    tests/test_metrics_gpu.py (2e-6 of the peak) on the float result, and to that bound plus half a 16-bit step in the file."""
    from oracle import metrics_ref
    from urgent2026_challenge_track1_amd import audio_io
    from urgent2026_challenge_track1_amd import estimate_audio_bandwidth as est
    from urgent2026_challenge_track1_amd import resample_to_estimated_bandwidth as rs
    from urgent2026_challenge_track1_amd.bandwidth import pick_rate
    cs, _ = cases
    src = tmp_path / "src"
    src.mkdir()
    listing, scp_lines, expect = {}, [], []
    for c in cs:
        path = str(src / ("%s_%d.wav" % (c["uid"], c["k"])))
        _write_wav(path, c["raw"], c["fs"])
        entry = path if c["seg"] is None else {"audio_path": path, "start": c["seg"][0], "end": c["seg"][1]}
        if c["k"] % 2 == 0 and c["seg"] is None:                   # (both files of the repeated uid have even numbers)
            scp_lines.append((c["uid"], path))
        else:
            assert c["uid"] not in listing
            listing[c["uid"]] = entry
        expect.append((c["uid"], path, c["freq"], c))
    # two inputs (an scp and a json), processed both; order of results = order of inputs
    (tmp_path / "in.scp").write_text("".join("%s %s\n" % (u, p) for u, p in scp_lines) + "broken %s\n" % (src / "missing.wav"))
    _write_wav(str(src / "tiny.wav"), np.zeros((1, 100), dtype=np.int16), 16000)
    listing["tiny"] = str(src / "tiny.wav")
    (tmp_path / "in.json").write_text(json.dumps(listing))
    out_json = tmp_path / "out" / "bw.json"
    est.main(["--audio_dir", str(tmp_path / "in.scp"), str(tmp_path / "in.json"), "--outfile", str(out_json), "--nj", "4",
              "--chunksize", "3"])
    got = json.load(open(out_json))
    want, by_path = {}, {p: (f, c) for _, p, f, c in expect}
    # rebuild the expectation in input order with the reference's renaming rule
    seq = [(u, p) for u, p in scp_lines] + [(u, e["audio_path"] if isinstance(e, dict) else e) for u, e in listing.items()]
    for u, p in seq:
        if p not in by_path or by_path[p][0] is None:
            continue                                               # tiny.wav (skipped) and the all-zero file (no bin)
        i, u2 = 1, u
        while u2 in want:
            i += 1
            u2 = "%s(%d)" % (u, i)
        want[u2] = [p, by_path[p][0]]
    assert got == want and list(got) == list(want)
    assert any(k.endswith("(2)") for k in got) and "zeros" not in got and "tiny" not in got and "broken" not in got
    # the text form carries the same values
    est.main(["--audio_dir", str(tmp_path / "in.scp"), str(tmp_path / "in.json"), "--outfile", str(tmp_path / "out" / "bw.txt")])
    assert est.read_bandwidth_file(tmp_path / "out" / "bw.txt") == [(u, p, f) for u, (p, f) in want.items()]

    # ---- resample ----
    outdir, out_scp = tmp_path / "res", tmp_path / "out" / "res.scp"
    ret = rs.main(["--bandwidth_data", str(out_json), "--out_scpfile", str(out_scp), "--outdir", str(outdir), "--nj", "3", "-m", "16"])
    lines = [ln.split(maxsplit=2) for ln in open(out_scp).read().splitlines()]
    assert [ln[0] for ln in lines] == list(want) and len(ret) == len(want)
    nd = rs.num_digits_for(len(want), 16)
    pairs = set()
    for idx, ((uid, (p, f)), ln) in enumerate(zip(want.items(), lines)):
        c = by_path[p][1]
        est_fs = pick_rate(f)
        assert int(ln[1]) == est_fs <= c["fs"]
        if est_fs == c["fs"]:
            assert ln[2] == p                                      # no-op: the original path, nothing written
            continue
        outfile = outdir / rs.subdir_name(idx, 16, nd) / (uid + ".wav")
        assert ln[2] == str(outfile) and outfile.exists()
        y, fs_y = audio_io.read_audio_all(str(outfile))
        assert fs_y == est_fs and y.shape[0] == c["x"].shape[0]
        pairs.add((c["fs"], est_fs))
        for ch in range(y.shape[0]):
            exp = metrics_ref.resample_soxr_hq_spec(c["x"][ch].astype(np.float64), c["fs"], est_fs)
            assert y[ch].shape == exp.shape
            err = np.abs(y[ch] - np.clip(exp, -1.0, 32767.0 / 32768.0)).max()
            assert err <= 2e-6 * np.abs(exp).max() + 0.5 / 32768.0, (uid, c["fs"], est_fs, err)
    assert len(pairs) >= 5, pairs
    # the float result, every downward pair the fixture produced plus one upward pair, to the resampler tests' own bound
    up = next(c for c in cs if c["fs"] == 8000 and c["x"].shape[0] == 2)
    for fs_in, fs_out, x in [(a, b, next(c for c in cs if c["fs"] == a and c["bin"] >= 0)["x"]) for a, b in sorted(pairs)] \
            + [(8000, 16000, up["x"])]:
        got_f = rs.resample_channels(x, fs_in, fs_out)
        for ch in range(x.shape[0]):
            exp = metrics_ref.resample_soxr_hq_spec(x[ch].astype(np.float64), fs_in, fs_out)
            assert got_f[ch].shape == exp.shape and np.abs(got_f[ch] - exp).max() <= 2e-6 * np.abs(exp).max(), (fs_in, fs_out)
    # a second run finds the files and makes none again; an upward target (a bandwidth above the file's Nyquist) is honoured
    before = {p: os.path.getmtime(p) for p in map(str, outdir.rglob("*.wav"))}
    rs.main(["--bandwidth_data", str(out_json), "--out_scpfile", str(tmp_path / "out" / "res2.scp"), "--outdir", str(outdir), "-m", "16"])
    assert {p: os.path.getmtime(p) for p in map(str, outdir.rglob("*.wav"))} == before
    assert open(tmp_path / "out" / "res2.scp").read() == open(out_scp).read()
    up_path = next(p for _, p, _, c in expect if c is up)
    ret = rs.resample_files([("up", up_path, 7000.0)], str(tmp_path / "res_up"))
    assert ret == [("up", tmp_path / "res_up" / "0" / "up.wav", 16000)]
    y, fs_y = audio_io.read_audio_all(str(ret[0][1]))
    assert fs_y == 16000 and y.shape == (2, 2 * up["x"].shape[1])


def test_unsupported_frame_size_raises(lib):
    from urgent2026_challenge_track1_amd._lib import UrseError
    from urgent2026_challenge_track1_amd.bandwidth import mean_power_spectrum, stft_params
    assert stft_params(64438)[0] == 2 * 1031                        # above the Bluestein limit, a prime above the generic butterfly's
    x = torch.randn(2, 9000, device="cuda")
    with pytest.raises(UrseError, match="2062"):
        mean_power_spectrum(x, [9000, 8000], 64438)
    with pytest.raises(UrseError, match="limit"):
        mean_power_spectrum(torch.randn(1, 20000, device="cuda"), [20000], 192000)       # n_fft 6144
    with pytest.raises(UrseError, match="reflect"):
        mean_power_spectrum(x, [9000, 128], 8000)                   # what torch.stft refuses
    with pytest.raises(UrseError):
        mean_power_spectrum(x.cpu(), [9000, 9000], 8000)            # no host path
    # 96 kHz (n_fft 3072) runs
    mp = mean_power_spectrum(torch.randn(1, 20000, device="cuda"), [20000], 96000)
    assert mp.shape == (1, 1537) and bool(torch.isfinite(mp).all()) and float(mp.min()) > 0


@pytest.mark.parametrize("fs", [8219, 13782, 22050, 30500, 44100, 63719, 96000])
def test_other_frame_sizes_against_the_definition(lib, fs):
    """frame sizes beyond the seven rates - 263 (prime), 441 = 3^2 7^2, 976 = 2^4 61, 2039 (prime, the largest Bluestein takes),
    3072 - and the two odd ones among them (705, 1411) against the float64 definition, with a row whose length is a whole number
    of hops: torch.stft pads n_fft // 2 on both sides, so an odd n_fft has 1 + (len - 1) // hop frames, not 1 + len // hop.
    White noise, bound as test_many_short_and_long_rows_in_one_launch"""
    from urgent2026_challenge_track1_amd.bandwidth import mean_power_spectrum, stft_params
    n_fft, hop = stft_params(fs)
    assert n_fft in (263, 441, 705, 976, 1411, 2039, 3072)
    rng = np.random.default_rng(fs)
    lens = [n_fft // 2 + 1, 3 * n_fft + 7, 20 * hop]
    wav = rng.standard_normal((len(lens), max(lens))).astype(np.float32)
    got = mean_power_spectrum(torch.from_numpy(wav).cuda(), lens, fs).cpu().numpy().astype(np.float64)
    win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n_fft) / n_fft)
    for r, n in enumerate(lens):
        x = np.pad(wav[r, :n].astype(np.float64), n_fft // 2, mode="reflect")
        frames = np.stack([x[t * hop:t * hop + n_fft] * win for t in range(1 + (len(x) - n_fft) // hop)])
        ref = (np.abs(np.fft.rfft(frames, axis=1)) ** 2).mean(0)
        assert np.abs(got[r] - ref).max() <= 1e-4 * ref.max(), (n_fft, n, np.abs(got[r] - ref).max() / ref.max())
