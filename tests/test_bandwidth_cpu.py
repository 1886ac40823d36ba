"""CPU: the host side of the bandwidth estimate (utils/estimate_audio_bandwidth.py, utils/resample_to_estimated_bandwidth.py of the
reference): frame sizes, the float32 bin-frequency rule against the stored ``torch.fft.rfftfreq`` vectors, the rate rule on its
boundaries, the file formats, sub-directory names, the segment slice, the C ABI entries and the kernels' register accounting."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "ref_bandwidth.npz")
RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000)


def test_stft_params_at_the_seven_rates():
    from urgent2026_challenge_track1_amd.bandwidth import stft_params
    got = [stft_params(fs) for fs in RATES]
    assert got == [(256, 128), (512, 256), (705, 352), (768, 384), (1024, 512), (1411, 705), (1536, 768)]


def test_bin_frequency_is_rfftfreq_bit_for_bit():
    from urgent2026_challenge_track1_amd.bandwidth import bin_frequency, stft_params
    z = np.load(GOLD)
    for fs in RATES:
        n_fft, _ = stft_params(fs)
        ref = z["rfftfreq_%d" % fs]
        assert ref.dtype == np.float32 and ref.shape == (n_fft // 2 + 1,)
        got = np.array([bin_frequency(i, n_fft, fs) for i in range(n_fft // 2 + 1)], dtype=np.float64)
        assert np.array_equal(got, ref.astype(np.float64)), fs
    # the value is the float32 one, not i * fs / n_fft in double
    assert bin_frequency(345, 705, 22050) != 345 * 22050 / 705


def test_fixture_holds_what_the_issue_asks():
    z = np.load(GOLD)
    fs, bins = z["fs"], z["bin"]
    for r in RATES:
        assert int(((fs == r) & (bins >= 0)).sum()) >= 6, r
    assert z["margin_db"][bins >= 0].min() >= 0.01
    assert (bins < 0).sum() == 1 and np.isnan(z["freq"][bins < 0]).all()                  # the all-zero file
    assert np.isfinite(z["segment"]).all(axis=1).sum() == 1                               # one segment entry
    uids = list(z["uid"])
    assert len(uids) - len(set(uids)) == 1                                                # one repeated uid
    assert set(z["channels"]) == {1, 2} and z["is_int16"].any() and not z["is_int16"].all()
    assert 0 < float(z["f32_cpu_rel_err"]) < 1e-2
    for name in os.listdir(os.path.dirname(GOLD)):
        if name.startswith("ref_bandwidth"):
            assert os.path.getsize(os.path.join(os.path.dirname(GOLD), name)) < (1 << 20), name


def test_pick_rate_on_the_boundaries():
    from urgent2026_challenge_track1_amd.bandwidth import pick_rate
    for sr in RATES:
        assert pick_rate(sr / 2) == sr                       # exactly sr / 2 still fits sr
    for lo, hi in zip(RATES[:-1], RATES[1:]):
        assert pick_rate(np.nextafter(lo / 2, np.inf)) == hi
    assert pick_rate(0.0) == 8000
    assert pick_rate(24000.0) == 48000 and pick_rate(24000.1) == 48000 and pick_rate(1e6) == 48000
    assert pick_rate(10782.7783203125) == 22050


def test_bandwidth_files_round_trip_with_repeated_uids(tmp_path):
    from urgent2026_challenge_track1_amd.estimate_audio_bandwidth import dedup_uids, read_bandwidth_file, write_bandwidth_file
    results = [("a", ["/x/a.wav", 10782.7783203125]), None, ("b", ["/x/b.wav", 4000.0]), ("a", ["/y/a.wav", 8000.0]),
               ("a", ["/z/a a.wav", 0.1 + 0.2])]
    ret = dedup_uids(results)
    assert list(ret) == ["a", "b", "a(2)", "a(3)"] and ret["a(2)"] == ["/y/a.wav", 8000.0]
    want = [("a", "/x/a.wav", 10782.7783203125), ("b", "/x/b.wav", 4000.0), ("a(2)", "/y/a.wav", 8000.0),
            ("a(3)", "/z/a a.wav", 0.1 + 0.2)]
    for name in ("bw.json", "bw.scp"):
        write_bandwidth_file(tmp_path / "sub" / name, ret)
        assert read_bandwidth_file(tmp_path / "sub" / name) == want, name
    assert json.load(open(tmp_path / "sub" / "bw.json"))["a"] == ["/x/a.wav", 10782.7783203125]
    assert open(tmp_path / "sub" / "bw.scp").readline() == "a 10782.7783203125 /x/a.wav\n"


def test_inputs_from_directory_scp_and_json(tmp_path):
    from urgent2026_challenge_track1_amd.estimate_audio_bandwidth import collect_inputs
    (tmp_path / "d" / "e").mkdir(parents=True)
    for p in ("d/one.wav", "d/e/two.wav", "d/skip.flac"):
        (tmp_path / p).write_bytes(b"")
    (tmp_path / "l.scp").write_text("u1 /p/with space.wav\nu2 /q.wav\n")
    (tmp_path / "l.json").write_text(json.dumps({"s": {"audio_path": "/r.wav", "start": 0.5, "end": 1.0}, "t": "/t.wav"}))
    got = collect_inputs([str(tmp_path / "d"), str(tmp_path / "l.scp"), str(tmp_path / "l.json")])
    assert sorted(u for u, _ in got[:2]) == ["one", "two"]
    assert got[2:] == [("u1", "/p/with space.wav"), ("u2", "/q.wav"), ("s", {"audio_path": "/r.wav", "start": 0.5, "end": 1.0}),
                       ("t", "/t.wav")]
    with pytest.raises(ValueError):
        collect_inputs([str(tmp_path / "missing.txt")])


def test_subdirectory_names():
    from urgent2026_challenge_track1_amd.resample_to_estimated_bandwidth import num_digits_for, subdir_name
    assert subdir_name(0, 10000, num_digits_for(1, 10000)) == "0"
    nd = num_digits_for(10000, 10000)
    assert {subdir_name(i, 10000, nd) for i in (0, 9999)} == {"0"}
    nd = num_digits_for(10001, 10000)
    assert nd == 1 and subdir_name(9999, 10000, nd) == "0" and subdir_name(10000, 10000, nd) == "1"
    nd = num_digits_for(300, 1)                      # ceil(log16(300)) = 3 digits
    assert nd == 3 and subdir_name(0, 1, nd) == "000" and subdir_name(299, 1, nd) == "12b"


def test_segment_slice_is_in_16k_samples_whatever_the_rate():
    from urgent2026_challenge_track1_amd.estimate_audio_bandwidth import segment_slice
    path, idx = segment_slice({"audio_path": "/a.wav", "start": 0.1, "end": 0.45})
    assert path == "/a.wav" and idx == slice(1600, 7200)
    assert segment_slice("/b.wav") == ("/b.wav", slice(None))
    assert segment_slice({"audio_path": "/a.wav", "start": 0.29, "end": 1.0001})[1] == slice(int(0.29 * 16000), int(1.0001 * 16000))


def test_all_channel_reader_and_multichannel_writer(tmp_path):
    from urgent2026_challenge_track1_amd import audio_io
    rng = np.random.default_rng(3)
    q = rng.integers(-32768, 32768, size=(2, 777)).astype(np.int16)
    audio_io.write_audio_channels(str(tmp_path / "st.wav"), q.astype(np.float32) / 32768.0, 22050)
    x, fs = audio_io.read_audio_all(str(tmp_path / "st.wav"))
    assert fs == 22050 and x.dtype == np.float32 and np.array_equal(x * 32768.0, q.astype(np.float32))
    first, _ = audio_io.read_audio(str(tmp_path / "st.wav"))            # the existing reader still takes channel 0
    assert np.array_equal(first, x[:1]) and audio_io.audio_frames(str(tmp_path / "st.wav")) == 777
    audio_io.write_audio_channels(str(tmp_path / "mono.wav"), x[1], 8000)
    y, fs = audio_io.read_audio_all(str(tmp_path / "mono.wav"))
    assert fs == 8000 and np.array_equal(y, x[1:2])


def test_entries_are_in_the_header_and_the_library(lib):
    import ctypes
    from urgent2026_challenge_track1_amd import _lib
    names = ("urse_power_spectrum_workspace_bytes", "urse_power_spectrum_mean", "urse_bandwidth_pick")
    protos = _lib.prototypes()
    for n in names:
        assert n in _lib.declared_symbols() and n in protos and hasattr(lib, n), n
    assert len(protos["urse_power_spectrum_mean"]) == 11 and len(protos["urse_bandwidth_pick"]) == 7
    nbytes = ctypes.c_int64()
    assert lib.urse_power_spectrum_workspace_bytes(256, 192000, 1536, 768, ctypes.byref(nbytes)) == 0
    assert nbytes.value % (769 * 4) == 0 and 256 * 769 * 4 <= nbytes.value <= 256 * 251 * 769 * 8 // 16
    # bad arguments and unsupported frame sizes are refused on the host, with a message
    assert lib.urse_power_spectrum_mean(None, 0, None, None, 1, 100, 64, 32, None, 0, None) == -1
    assert b"urse_power_spectrum_mean" in lib.urse_last_error()
    assert lib.urse_bandwidth_pick(None, None, None, 1, 33, -50.0, None) == -1
    for n_fft in (2 * 1031, 4098, 8192):               # above 2048 with a prime factor above 127, or above the limit of 4096
        assert lib.urse_power_spectrum_workspace_bytes(4, 48000, n_fft, n_fft // 2, ctypes.byref(nbytes)) == -3, n_fft
        assert str(n_fft).encode() in lib.urse_last_error()
    for n_fft in (256, 512, 705, 768, 1024, 1411, 1536, 3072, 4096, 960, 441, 263, 2 * 131, 2039):
        assert lib.urse_power_spectrum_workspace_bytes(4, 48000, n_fft, n_fft // 2, ctypes.byref(nbytes)) == 0, n_fft

def test_new_kernels_spill_nothing(lib):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_regs
    table = kernel_regs.collect()
    for k in ("urse::bw_power_kernel<false>", "urse::bw_power_kernel<true>", "urse::bw_mean_kernel", "urse::bw_pick_kernel"):
        assert k in table, k
        t = table[k]
        assert t["vgpr_spill_count"] == 0 and t["sgpr_spill_count"] == 0 and t["private_segment_fixed_size"] == 0 \
            and t["scratch_ops"] == 0, (k, t)
        assert t["object"] == "bandwidth.o"

