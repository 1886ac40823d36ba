"""CPU: the host side of the offline corpus simulation - the recipe generator against the meta.tsv the reference's own ``main`` wrote
(tests/golden/ref_meta.npz, make_golden_simulate.py), the command-line contract of the two entry points, the id-seeded noise offset,
STREAMINFO assembly, and utt2numsamples."""
import hashlib
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def meta():
    return np.load(os.path.join(GOLDEN, "ref_meta.npz"))


def _corpus(meta, tmp_path):
    paths = {}
    for key, text in zip(meta["meta_scp_keys"].tolist(), meta["meta_scp_text"].tolist()):
        paths[key] = str(tmp_path / key)
        with open(paths[key], "w") as f:
            f.write(text)
    lengths = dict(zip(meta["meta_speech_uids"].tolist(), meta["meta_speech_lengths"].tolist()))
    by_path = {ln.split()[2]: lengths[ln.split()[0]] for ln in open(paths["speech"]).read().splitlines()}
    return paths, by_path


@pytest.mark.parametrize("tag", ["a", "b"])
def test_generator_writes_the_reference_meta_tsv_byte_for_byte(meta, tmp_path, monkeypatch, tag):
    """two rates (descending), repeat_per_utt 3, RIR pools that run dry (fall-through to the higher rate, then none / the used pool),
    wind rows and their 'wind meets clipping' re-draws, store_noise on ('a') and off ('b')"""
    from urgent2026_challenge_track1_amd import generate_data_param as gdp
    paths, by_path = _corpus(meta, tmp_path)
    conf = tmp_path / "conf.yaml"
    conf.write_text(str(meta["meta_%s_yaml" % tag]))
    monkeypatch.chdir(tmp_path)
    n = gdp.main(["--config", str(conf), "--speech_scps", paths["speech"], "--speech_utt2spk", paths["utt2spk"], "--speech_text",
                  paths["text"], "--noise_scps", paths["noise"], "--wind_noise_scps", paths["wind"], "--rir_scps", paths["rir"],
                  "--log_dir", str(tmp_path / "log"), "--output_dir", "out/%s" % tag], frames=by_path.__getitem__)
    want = str(meta["meta_%s_tsv" % tag])
    got = (tmp_path / "log" / "meta.tsv").read_text()
    assert n == 24 and got == want
    header = want.splitlines()[0].split("\t")
    assert ("noise_path" in header) == (tag == "a")
    assert (tmp_path / "out" / tag / "noisy" / "0").is_dir() and (tmp_path / "out" / tag / "noise" / "0").is_dir() == (tag == "a")


def test_select_sample_pools(monkeypatch):
    from urgent2026_challenge_track1_amd.generate_data_param import select_sample
    rs = np.random.RandomState(0)
    pool = {16000: {"a": 1}, 48000: {"b": 2, "c": 3}}
    used = {16000: {}, 48000: {}}
    assert select_sample(16000, pool, used, False, rs) == "a" and used[16000] == {"a": 1} and pool[16000] == {}
    assert select_sample(16000, pool, used, False, rs) in ("b", "c") and len(pool[48000]) == 1            # the higher rate
    assert select_sample(48000, pool, used, False, rs) in ("b", "c") and pool[48000] == {}
    assert select_sample(16000, pool, used, False, rs) is None                                             # dry, no reuse
    assert select_sample(16000, pool, used, True, rs) == "a" and used[16000] == {"a": 1}                   # the used pool, nothing moves
    assert select_sample(22050, pool, used, True, rs) in ("b", "c")
    assert select_sample(48000, {8000: {"z": 0}}, {8000: {}}, True, rs) is None                            # nothing at or above the rate


def test_config_file_gives_defaults_and_the_command_line_wins(tmp_path):
    from urgent2026_challenge_track1_amd import generate_data_param as gdp
    conf = tmp_path / "c.yaml"
    conf.write_text("seed: 7\nrepeat_per_utt: 3\nlog_dir: from_yaml\nnum_augmentations: {0: 0.5, 2: 0.5}\nstore_noise: true\n")
    parser = gdp.get_parser()
    args = parser.parse_args(["--config", str(conf), "--seed", "9", "--output_dir", "o", "--speech_scps", "s", "--noise_scps", "n"])
    assert args.seed == 9 and args.repeat_per_utt == 3 and args.log_dir == "from_yaml" and args.store_noise is True
    assert args.num_augmentations == {0: 0.5, 2: 0.5} and args.out_format == "flac"
    gdp.check_required(parser, args)
    with pytest.raises(SystemExit):          # required, as the YAML / command line left it unset
        a = gdp.get_parser().parse_args(["--config", str(conf), "--speech_scps", "s", "--noise_scps", "n"])
        gdp.check_required(gdp.get_parser(), a)
    bad = tmp_path / "bad.yaml"
    bad.write_text("no_such_flag: 1\n")
    with pytest.raises(SystemExit):
        gdp.get_parser().parse_args(["--config", str(bad)])
    assert gdp.get_parser().parse_args(["--reuse_noise", "yes"]).reuse_noise is True


def test_highpass_flag_keeps_the_reference_quirk():
    """type=bool: any non-empty string is true, 'False' included"""
    from urgent2026_challenge_track1_amd import simulate_data_from_param as sdp
    base = ["--meta_tsv", "m"]
    assert sdp.get_parser().parse_args(base).highpass is False
    assert sdp.get_parser().parse_args(base + ["--highpass", "False"]).highpass is True
    assert sdp.get_parser().parse_args(base + ["--highpass", "1"]).highpass is True
    assert sdp.get_parser().parse_args(base + ["--highpass", ""]).highpass is False
    args = sdp.get_parser().parse_args(base)
    assert args.nj == 8 and args.chunksize == 1000 and args.unsupported_augmentation == "warn"
    with pytest.raises(SystemExit):
        sdp.get_parser().parse_args([])       # --meta_tsv is required


def test_meta_tsv_must_be_the_file_that_is_read(tmp_path):
    from urgent2026_challenge_track1_amd import simulate_data_from_param as sdp
    (tmp_path / "log").mkdir()
    (tmp_path / "log" / "meta.tsv").write_text("id\n")
    (tmp_path / "other.tsv").write_text("id\n")
    sdp.check_meta_path(str(tmp_path / "log" / "meta.tsv"), str(tmp_path / "log"))
    sdp.check_meta_path(str(tmp_path / "log" / ".." / "log" / "meta.tsv"), str(tmp_path / "log"))
    with pytest.raises(ValueError, match="log_dir/meta.tsv"):
        sdp.check_meta_path(str(tmp_path / "other.tsv"), str(tmp_path / "log"))


def test_noise_offset_is_the_reference_draw():
    from urgent2026_challenge_track1_amd import simulate_data_from_param as sdp
    g = np.load(os.path.join(GOLDEN, "ref_simulate.npz"))
    fields = g["sim_row_fields"].tolist()
    lens = {k: len(g["sim_audio_" + k]) for k in g["sim_audio_names"].tolist()}
    kinds = set()
    for row in g["sim_rows"].tolist():
        r = dict(zip(fields, row))
        ls, ln = lens[r["speech_uid"]], lens[r["noise_uid"]]
        assert sdp.noise_offset(r["id"], ls, ln) == int(r["noise_offset"]), r["id"]
        kinds.add("equal" if ls == ln else "long" if ln > ls else "tiny" if 2 * ln < ls else "short")
    assert kinds == {"equal", "long", "tiny", "short"}
    assert sdp.noise_offset("fileid_17", 100, 100) == 0


def test_rows_parse_into_recipes_and_name_what_is_not_applied():
    from urgent2026_challenge_track1_amd import simulate_data_from_param as sdp
    row = dict(id="fileid_3", noise_uid="nz", snr_dB="2.5", fs="16000", length="5000", rir_uid="none",
               augmentation="packet_loss(packet_loss_indices=[3, 4],packet_duration_ms=20)/codec(format=mp3,encoder=None,qscale=4)/"
                            "clipping(min=0.1,max=0.9)")
    recipe, lacking = sdp.parse_row(row, True)
    assert recipe["order"] == ["packet_loss", "codec", "clipping"] and lacking == ["codec"] and recipe["snr"] == 2.5
    assert recipe["params"]["packet_loss"]["packet_loss_indices"] == [3, 4] and recipe["params"]["clipping"] == dict(min_quantile=0.1, max_quantile=0.9)
    wind = dict(row, noise_uid="wind_noise48000_1", augmentation="wind_noise(threshold=0.2,ratio=7.9,attack=57.5,release=23.6,sc_gain=0.87,"
                "clipping=False,clipping_threshold=0.9)/bandwidth_limitation-polyphase->8000")
    recipe, lacking = sdp.parse_row(wind, False)
    assert recipe["wind"] and lacking == ["wind_noise"] and recipe["order"] == ["bandwidth_limitation"] and recipe["highpass"] is False
    assert sdp.parse_row(dict(row, augmentation="none"), True)[0]["order"] == []
    with pytest.raises(NotImplementedError):
        sdp.parse_row(dict(row, augmentation="echo(3)"), True)


def test_batches_are_per_rate_sorted_and_under_the_budget():
    from urgent2026_challenge_track1_amd import simulate_data_from_param as sdp
    rows = [dict(fs="16000", length=str(n)) for n in (900, 100, 500, 300)] + [dict(fs="8000", length="50")]
    assert sdp.plan_batches(rows, 1000, budget=1000) == [[4], [1, 3], [2], [0]]
    assert sdp.plan_batches(rows, 2, budget=1 << 30) == [[4], [1, 3], [2, 0]]


def test_streaminfo_assembly_on_a_hand_made_frame_list():
    from urgent2026_challenge_track1_amd import flac
    frames = [bytes([0xFF, 0xF8]) + bytes(range(20)), bytes([0xFF, 0xF8]) + bytes(9), bytes([0xFF, 0xF8]) + bytes(31)]
    pcm = np.arange(-300, 9000 - 300, dtype="<i2")
    md5 = hashlib.md5(pcm.tobytes()).digest()
    data = flac.flac_file(b"".join(frames), [len(f) for f in frames], 44100, len(pcm), 4096, md5)
    assert data[:4] == b"fLaC" and data[4:8] == bytes([0x80, 0, 0, 34]) and data[42:] == b"".join(frames)
    si = data[8:42]
    assert si[0:2] == si[2:4] == (4096).to_bytes(2, "big")
    assert int.from_bytes(si[4:7], "big") == 11 and int.from_bytes(si[7:10], "big") == 33
    bits = int.from_bytes(si[10:18], "big")
    assert bits >> 44 == 44100 and (bits >> 41) & 7 == 0 and (bits >> 36) & 31 == 15 and bits & ((1 << 36) - 1) == 9000
    assert si[18:] == md5
    info = flac.flac_streaminfo(data)          # the library's own reader agrees
    assert (info["fs"], info["channels"], info["bits"], info["total_samples"], info["min_block"], info["max_block"]) == (44100, 1, 16, 9000, 4096, 4096)
    with pytest.raises(ValueError):
        flac.flac_file(b"".join(frames), [1, 2, 3], 44100, 9000, 4096, md5)
    with pytest.raises(ValueError):
        flac.flac_file(b"", [], 44100, 0, 4096, b"short")


def test_utt2numsamples_on_wav_and_flac(lib, tmp_path):
    from tests import flac_writer as fw
    from urgent2026_challenge_track1_amd import audio_io, utt2numsamples
    rng = np.random.default_rng(3)
    audio_io.write_audio(str(tmp_path / "a.wav"), 0.1 * rng.standard_normal(4321).astype(np.float32), 16000)
    x = rng.integers(-2000, 2000, size=(3000, 1))
    frames = [(1024, "indep", [("fixed2", {})]), (1024, "indep", [("verbatim", {})]), (952, "indep", [("fixed1", {})])]
    (tmp_path / "b.flac").write_bytes(fw.encode(x, 8000, 16, frames))
    (tmp_path / "in.scp").write_text("utt_a 16000 %s\nutt_b %s\n" % (tmp_path / "a.wav", tmp_path / "b.flac"))
    utt2numsamples.main(["--input_scp", str(tmp_path / "in.scp"), "--outfile", str(tmp_path / "speech_length.scp")])
    assert (tmp_path / "speech_length.scp").read_text() == "utt_a 4321\nutt_b 3000\n"
