"""GPU: the offline simulator (simulate_data_from_param) on the rows of tests/golden/ref_simulate.npz - what the reference's own
``process_one_sample(on_the_fly=False)`` handed to ``soundfile.write`` for them (make_golden_simulate.py): noise shorter than the speech,
shorter than half of it, longer, equal; RIR rows (clean = early-RIR convolution); clipping; packet loss; packet loss then clipping;
high-pass on and off; stored noise.  The sources are float32 WAV files holding exactly what the reference was served."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FLOAT_BOUND = 2e-5          # test_simulate_recipes_matches_the_reference_simulator's bound for this code path (0.9-peak signals, f32 arithmetic)


def _rows(g):
    fields = g["sim_row_fields"].tolist()
    return [dict(zip(fields, r), index=i) for i, r in enumerate(g["sim_rows"].tolist())]


def _write_corpus(g, root):
    from urgent2026_challenge_track1_amd import audio_io
    os.makedirs(os.path.join(root, "src"), exist_ok=True)
    lines = []
    for name, fs in zip(g["sim_audio_names"].tolist(), g["sim_audio_fs"].tolist()):
        path = os.path.join(root, "src", name + ".wav")
        audio_io.write_audio(path, g["sim_audio_" + name], int(fs), subtype="FLOAT")
        lines.append("%s %d %s" % (name, fs, path))
    scp = os.path.join(root, "all.scp")
    with open(scp, "w") as f:
        f.write("\n".join(lines) + "\n")
    return scp


def _write_meta(rows, root, tag, ext, prefix="fileid"):
    log = os.path.join(root, "log_" + tag)
    os.makedirs(log, exist_ok=True)
    head = ["id", "noisy_path", "speech_uid", "speech_sid", "clean_path", "noise_uid", "noise_path", "snr_dB", "rir_uid", "augmentation",
            "fs", "length", "text"]
    with open(os.path.join(log, "meta.tsv"), "w") as f:
        f.write("\t".join(head) + "\n")
        for r in rows:
            uid = "%s_%s" % (prefix, r["id"].split("_")[-1])           # the numeric suffix seeds the noise offset
            name = "%s.%s" % (uid, ext)
            out = os.path.join(root, "out_" + tag)
            f.write("\t".join([uid, os.path.join(out, "noisy", "0", name), r["speech_uid"], "spk", os.path.join(out, "clean", "0", name),
                               r["noise_uid"], os.path.join(out, "noise", "0", name), r["snr_dB"], r["rir_uid"], r["augmentation"], r["fs"],
                               r["length"], "<not-available>"]) + "\n")
    return log


def _run(scp, log, highpass, extra=()):
    from urgent2026_challenge_track1_amd import simulate_data_from_param as sdp
    argv = ["--speech_scps", scp, "--noise_scps", scp, "--wind_noise_scps", scp, "--rir_scps", scp, "--log_dir", log, "--output_dir",
            "unused", "--meta_tsv", os.path.join(log, "meta.tsv"), "--store_noise", "true", "--nj", "4"] + list(extra)
    if highpass:
        argv += ["--highpass", "True"]
    return sdp.main(argv)


def _pcm(path):
    from urgent2026_challenge_track1_amd import audio_io
    x, fs = audio_io.read_audio(path)
    return np.round(x[0].astype(np.float64) * 32768.0).astype(np.int64), fs


@pytest.fixture(scope="module")
def world(lib, tmp_path_factory):
    """the fixture rows simulated once per (high-pass, format): ragged batches of mixed lengths, as the command line runs them"""
    g = np.load(os.path.join(GOLDEN, "ref_simulate.npz"))
    root = str(tmp_path_factory.mktemp("sim"))
    scp = _write_corpus(g, root)
    rows = _rows(g)
    logs = {}
    for hp in (True, False):
        mine = [r for r in rows if bool(r["highpass"]) == hp]
        for ext in ("flac", "wav"):
            tag = "%s_%s" % ("hp" if hp else "nohp", ext)
            logs[tag] = _write_meta(mine, root, tag, ext)
            _run(scp, logs[tag], hp)
    return dict(g=g, root=root, scp=scp, rows=rows, logs=logs)


def _paths(world, r, ext, kind, prefix="fileid"):
    tag = "%s_%s" % ("hp" if r["highpass"] else "nohp", ext)
    return os.path.join(world["root"], "out_" + tag, kind, "0", "%s_%s.%s" % (prefix, r["id"].split("_")[-1], ext))


def test_float_results_meet_the_bound_of_the_on_the_fly_path(world):
    import torch
    from urgent2026_challenge_track1_amd import simulate_data_from_param as sdp
    g, rows = world["g"], world["rows"]
    table = sdp.read_flat_scps([world["scp"]])
    worst = 0.0
    for hp in (True, False):
        for fs in ("8000", "16000"):
            mine = [r for r in rows if bool(r["highpass"]) == hp and r["fs"] == fs]
            if not mine:
                continue
            infos = [dict(r, rir_uid=r["rir_uid"]) for r in mine]
            items = [sdp.load_item(i, sdp.parse_row(i, hp)[0], table, table, table) for i in infos]
            for it, r in zip(items, mine):
                ls, ln = len(g["sim_audio_" + r["speech_uid"]]), len(g["sim_audio_" + r["noise_uid"]])
                if ln > ls:                                                  # a longer noise arrives cropped at its offset
                    assert it["recipe"]["noise_offset"] == 0 and it["noise"].shape[1] == ls
                    assert np.array_equal(it["noise"][0], g["sim_audio_" + r["noise_uid"]][int(r["noise_offset"]):int(r["noise_offset"]) + ls])
                else:
                    assert it["recipe"]["noise_offset"] == int(r["noise_offset"])
            clean, noisy, noise, lens = sdp.simulate_items(items, "cuda")
            torch.cuda.synchronize()
            for b, r in enumerate(mine):
                n = lens[b]
                for kind, got in (("clean", clean), ("noisy", noisy), ("noise", noise)):
                    key = "sim_%s_%d" % (kind, r["index"])
                    if key in g:
                        err = float(np.abs(got[b, :n].cpu().numpy().astype(np.float64) - g[key]).max())
                        print("float parity %s %s: %.3e" % (r["id"], kind, err))
                        worst = max(worst, err)
                        assert err <= FLOAT_BOUND, (r["id"], kind, err)
    print("float parity, worst: %.3e" % worst)


def test_written_pcm_is_within_one_lsb_and_flac_equals_wav(world):
    g = world["g"]
    differ = total = 0
    for r in world["rows"]:
        for kind in ("clean", "noisy", "noise"):
            key = "sim_%s_%d" % (kind, r["index"])
            fl, fs = _pcm(_paths(world, r, "flac", kind))
            wv, fs2 = _pcm(_paths(world, r, "wav", kind))
            assert fs == fs2 == int(r["fs"]) and len(fl) == int(r["length"])
            assert np.array_equal(fl, wv), (r["id"], kind)                   # both containers hold the same samples
            if key in g:
                want = np.clip(np.round(g[key] * 32768.0), -32768, 32767).astype(np.int64)
                d = np.abs(fl - want)
                assert d.max() <= 1, (r["id"], kind, int(d.max()))
                differ += int((d > 0).sum())
                total += d.size
    print("PCM parity: %d of %d samples differ by one LSB (%.4f %%)" % (differ, total, 100.0 * differ / total))


def test_a_row_alone_equals_the_row_in_its_batch_within_one_lsb(world):
    rows = [r for r in world["rows"] if r["highpass"]]
    log = _write_meta(rows, world["root"], "alone", "flac")
    _run(world["scp"], log, True, ["--chunksize", "1"])
    for r in rows:
        for kind in ("clean", "noisy", "noise"):
            a, _ = _pcm(os.path.join(world["root"], "out_alone", kind, "0", "fileid_%s.flac" % r["id"].split("_")[-1]))
            b, _ = _pcm(_paths(world, r, "flac", kind))
            assert np.abs(a - b).max() <= 1, (r["id"], kind)


def test_the_same_command_twice_writes_identical_files(world):
    rows = [r for r in world["rows"] if r["highpass"]]
    log = _write_meta(rows, world["root"], "again", "flac")
    _run(world["scp"], log, True)
    for r in rows:
        for kind in ("clean", "noisy", "noise"):
            name = "fileid_%s.flac" % r["id"].split("_")[-1]
            a = open(os.path.join(world["root"], "out_again", kind, "0", name), "rb").read()
            assert a == open(_paths(world, r, "flac", kind), "rb").read(), (r["id"], kind)


def test_rows_the_device_cannot_fully_simulate_are_refused_or_listed(world):
    from urgent2026_challenge_track1_amd import audio_io
    base = world["rows"][0]
    wind_src = os.path.join(world["root"], "src", "nz16000_short.wav")
    scp = os.path.join(world["root"], "with_wind.scp")
    with open(scp, "w") as f:
        f.write(open(world["scp"]).read() + "wind_noise16000_0 16000 %s\n" % wind_src)
    rows = [dict(base, id="fileid_5", augmentation="codec(format=mp3,encoder=None,qscale=4)/clipping(min=0.05,max=0.95)"),
            dict(base, id="fileid_6", noise_uid="wind_noise16000_0",
                 augmentation="wind_noise(threshold=0.2,ratio=7.9,attack=57.5,release=23.6,sc_gain=0.87,clipping=False,clipping_threshold=0.9)/")]
    log = _write_meta(rows, world["root"], "lacking", "wav")
    with pytest.raises(NotImplementedError, match="codec"):
        _run(scp, log, True, ["--unsupported_augmentation", "raise"])
    assert not os.path.exists(os.path.join(world["root"], "out_lacking"))
    n, lacking = _run(scp, log, True)
    assert n == 2 and lacking == [("fileid_5", "codec"), ("fileid_6", "wind_noise")]
    assert open(os.path.join(log, "unsupported.tsv")).read() == "id\taugmentation\nfileid_5\tcodec\nfileid_6\twind_noise\n"
    for uid in ("fileid_5", "fileid_6"):
        x, fs = audio_io.read_audio(os.path.join(world["root"], "out_lacking", "noisy", "0", uid + ".wav"))
        assert fs == 16000 and x.shape[1] == int(base["length"]) and 0.3 < np.abs(x).max() <= 0.9001


def test_a_length_that_contradicts_the_row_names_the_row(world):
    rows = [dict(world["rows"][0], length="1234")]
    log = _write_meta(rows, world["root"], "badlen", "wav")
    with pytest.raises(AssertionError, match="fileid_17"):
        _run(world["scp"], log, True)


def test_generator_simulator_lengths_and_the_presimulated_loader(world, tmp_path, monkeypatch):
    """the recipe's three programs in a row, then AudioDataModule's pre-simulated loader reads a batch of the result"""
    from urgent2026_challenge_track1_amd import generate_data_param as gdp, simulate_data_from_param as sdp, utt2numsamples
    from urgent2026_challenge_track1_amd.config import Config
    from urgent2026_challenge_track1_amd.dataset import AudioDataModule
    g = world["g"]
    names = dict(zip(g["sim_audio_names"].tolist(), g["sim_audio_fs"].tolist()))
    src = os.path.join(world["root"], "src")

    def scp(path, keep, fmt="%s %d %s\n"):
        with open(path, "w") as f:
            for n, fs in names.items():
                if keep(n):
                    f.write(fmt % (n, fs, os.path.join(src, n + ".wav")))
        return str(path)
    speech = scp(tmp_path / "speech.scp", lambda n: n.startswith("sp"))
    noise = scp(tmp_path / "noise.scp", lambda n: n.startswith("nz"))
    rir = scp(tmp_path / "rir.scp", lambda n: n.startswith("rir"))
    with open(tmp_path / "utt2spk", "w") as f:
        f.write("".join("%s spk\n" % n for n in names if n.startswith("sp")))
    conf = tmp_path / "conf.yaml"
    conf.write_text("repeat_per_utt: 2\nseed: 1\nreuse_noise: true\nreuse_rir: true\nprob_reverberation: 0.5\nprob_wind_noise: 0.0\n"
                    "num_augmentations: {0: 0.4, 1: 0.4, 2: 0.2}\n"
                    "augmentations:\n  clipping: {weight: 1.0, clipping_min_quantile: [0.0, 0.1], clipping_max_quantile: [0.9, 1.0]}\n"
                    "  packet_loss: {weight: 1.0, packet_duration_ms: 20, max_continuous_packet_loss: 10, packet_loss_rate: [0.05, 0.25]}\n")
    common = ["--config", str(conf), "--speech_scps", speech, "--speech_utt2spk", str(tmp_path / "utt2spk"), "--noise_scps", noise,
              "--rir_scps", rir, "--log_dir", str(tmp_path / "log"), "--output_dir", str(tmp_path / "data")]
    assert gdp.main(common) == 8
    n, lacking = sdp.main(common + ["--meta_tsv", str(tmp_path / "log" / "meta.tsv"), "--highpass", "1"])
    assert n == 8 and lacking == []
    rows = sdp.read_meta(str(tmp_path / "log"))
    d = tmp_path / "set"
    d.mkdir()
    (d / "wav.scp").write_text("".join("%s %s\n" % (r["id"], r["noisy_path"]) for r in rows))
    (d / "spk1.scp").write_text("".join("%s %s\n" % (r["id"], r["clean_path"]) for r in rows))
    (d / "utt2fs").write_text("".join("%s %s\n" % (r["id"], r["fs"]) for r in rows))
    utt2numsamples.main(["--input_scp", str(d / "wav.scp"), "--outfile", str(d / "speech_length.scp")])
    assert (d / "speech_length.scp").read_text() == "".join("%s %s\n" % (r["id"], r["length"]) for r in rows)
    assert all(r["noisy_path"].endswith(".flac") for r in rows)
    cfg = Config(train_set_path=str(d), valid_set_path=str(d), train_set_dynamic_mixing=False, batch_size=2, num_worker=0, max_duration=3000)
    dm = AudioDataModule(cfg)
    clean, noisy, fs, lens = next(iter(dm.val_dataloader()))
    assert clean.shape == noisy.shape and clean.shape[0] == 2 and int(fs) in (8000, 16000) and int(lens.max()) == clean.shape[2]
    assert float(noisy.abs().max()) <= 0.9001 and float((clean - noisy).abs().max()) > 1e-3
    clean, noisy, fs, lens = next(iter(dm.train_dataloader()))
    assert clean.shape == (2, 1, 3000)
