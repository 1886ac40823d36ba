"""Golden vectors produced BY THE REFERENCE'S OWN CODE for the offline corpus simulation (run in the build container only, where
the reference tree exists): ``simulation/generate_data_param.py::main`` (-> ref_meta.npz) and
``simulation/simulate_data_from_param.py::process_one_sample(on_the_fly=False)`` (-> ref_simulate.npz).

The stand-in modules are make_golden_mix.py's (soundfile serves seeded in-memory arrays by "path"; espnet's detect_non_silence is
oracle/mix_ref.py's restatement); here ``soundfile.write`` is a capture, so the float64 arrays the reference hands to its writer are
what is stored.  Only data is stored: inputs, YAML values, the meta.tsv text, rows and arrays - never reference source.
"""
import importlib
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.golden import make_golden_mix as gm  # noqa: E402

WRITTEN = {}


def capture_write(path, audio, samplerate=None, **kw):
    WRITTEN[str(path)] = (np.array(audio, dtype=np.float64), int(samplerate))


AUGMENTATIONS = dict(
    bandwidth_limitation=dict(weight=1.0, resample_methods="random"),
    clipping=dict(weight=2.0, clipping_min_quantile=[0.0, 0.1], clipping_max_quantile=[0.9, 1.0]),
    codec=dict(weight=1.0, config=[dict(format="mp3", encoder=None, qscale=[1, 10]), dict(format="ogg", encoder=["vorbis"], qscale=[-1, 10])]),
    packet_loss=dict(weight=1.0, packet_duration_ms=20, max_continuous_packet_loss=10, packet_loss_rate=[0.05, 0.25]),
)
WIND = dict(threshold=[0.1, 0.3], ratio=[1, 20], attack=[5, 100], release=[5, 100], sc_gain=[0.8, 1.2], clipping_threshold=[0.85, 1.0],
            clipping_chance=0.75)
CONFIGS = {
    "a": dict(repeat_per_utt=3, seed=3, store_noise=True, reuse_noise=True, reuse_rir=False, prob_reverberation=0.5, prob_wind_noise=0.3,
              snr_low_bound=-5.0, snr_high_bound=20.0, wind_noise_snr_low_bound=-10.0, wind_noise_snr_high_bound=15.0,
              wind_noise_config=WIND, augmentations=AUGMENTATIONS, num_augmentations={0: 0.2, 1: 0.4, 2: 0.25, 3: 0.15},
              out_format="flac"),
    "b": dict(repeat_per_utt=3, seed=11, store_noise=False, reuse_noise=False, reuse_rir=True, prob_reverberation=0.25, prob_wind_noise=0.3,
              snr_low_bound=0.0, snr_high_bound=10.0, wind_noise_snr_low_bound=-10.0, wind_noise_snr_high_bound=15.0,
              wind_noise_config=WIND, augmentations=AUGMENTATIONS, num_augmentations={0: 0.2, 1: 0.4, 2: 0.25, 3: 0.15},
              out_format="wav"),
}


def meta_fixture(gen):
    """two rates, pools small enough that reuse_rir: false exhausts 16 kHz, falls through to 48 kHz and then to the used pool"""
    rng = np.random.default_rng(5)
    scp = {"speech": [], "utt2spk": [], "text": [], "noise": [], "wind": [], "rir": []}
    for fs in (16000, 48000):
        for i in range(4):
            uid = "sp%d_%d" % (fs, i)
            ext = "wav" if i % 2 == 0 else "flac"                 # header count / full decode: both serve len(AUDIO[path])
            path = "/corpus/%s.%s" % (uid, ext)
            gm.AUDIO[path] = (np.zeros(int(rng.integers(fs, 2 * fs))), fs)
            scp["speech"].append("%s %d %s" % (uid, fs, path))
            scp["utt2spk"].append("%s spk%d" % (uid, i % 3))
            if i != 3:                                            # one utterance without a transcript
                scp["text"].append("%s the transcript of %s, with  two spaces" % (uid, uid))
        for i in range(14 if fs == 16000 else 30):
            scp["noise"].append("nz%d_%d %d /corpus/nz%d_%d.wav" % (fs, i, fs, fs, i))
        for i in range(2 if fs == 16000 else 9):
            scp["rir"].append("rir%d_%d %d /corpus/rir%d_%d.wav" % (fs, i, fs, fs, i))
    scp["wind"].append("wind_noise48000_0 48000 /corpus/wn0.wav")           # 16 kHz wind rows fall through to the higher rate
    scp["wind"].append("wind_noise48000_1 48000 /corpus/wn1.wav")
    lengths = {ln.split()[0]: len(gm.AUDIO[ln.split()[2]][0]) for ln in scp["speech"]}
    out = {"meta_speech_uids": np.array(list(lengths)), "meta_speech_lengths": np.array(list(lengths.values())),
           "meta_scp_keys": np.array(list(scp)), "meta_scp_text": np.array(["\n".join(v) + "\n" for v in scp.values()])}
    import yaml
    redraws = 0
    for tag, conf in CONFIGS.items():
        tmp = tempfile.mkdtemp()
        paths = {}
        for k, v in scp.items():
            paths[k] = os.path.join(tmp, k)
            with open(paths[k], "w") as f:
                f.write("\n".join(v) + "\n")
        args = types.SimpleNamespace(speech_scps=[paths["speech"]], speech_utt2spk=[paths["utt2spk"]], speech_text=[paths["text"]],
                                     noise_scps=[paths["noise"]], wind_noise_scps=[paths["wind"]], rir_scps=[paths["rir"]],
                                     log_dir=os.path.join(tmp, "log"), output_dir="out/%s" % tag, reuse_wind_noise=False, **conf)
        os.makedirs(args.log_dir)
        cwd = os.getcwd()
        os.chdir(tmp)                                             # main creates the output directories (relative: the text stays portable)
        try:
            import random
            random.seed(args.seed)
            np.random.seed(args.seed)
            sized, plain = [0], np.random.choice

            def counting(*a, **kw):                            # same stream: it only counts the augmentation draws (size=, replace=False)
                sized[0] += "size" in kw and kw.get("replace") is False
                return plain(*a, **kw)
            np.random.choice = counting
            gen.main(args)
        finally:
            np.random.choice = plain
            os.chdir(cwd)
        text = open(os.path.join(args.log_dir, "meta.tsv")).read()
        rows = [dict(zip(text.splitlines()[0].split("\t"), ln.split("\t"))) for ln in text.splitlines()[1:]]
        assert len(rows) == 24
        drawn = sum(1 for r in rows if [a for a in r["augmentation"].split("/") if a and a != "none" and not a.startswith("wind_noise")])
        redraws += sized[0] - drawn                              # 'wind meets clipping' draws again
        wind = [r for r in rows if r["noise_uid"].startswith("wind_noise")]
        assert wind and any("packet_loss" in r["augmentation"] for r in rows) and any("codec" in r["augmentation"] for r in rows)
        assert any(r["rir_uid"].startswith("rir48000") and r["fs"] == "16000" for r in rows) or tag == "b", "no fall-through to a higher rate"
        out["meta_%s_yaml" % tag] = np.array(yaml.safe_dump(conf))
        out["meta_%s_tsv" % tag] = np.array(text)
    assert redraws >= 1, "no re-draw of wind meets clipping: choose other seeds"
    print("re-draws of 'wind meets clipping':", redraws)
    return out


def simulate_fixture(sim):
    rng = np.random.default_rng(77)
    out, rows, audio = {}, [], {}

    def add(name, n, fs, kind):
        # rounded to f32 once: the files the device path reads hold exactly what the reference was served
        audio[name] = (gm.synth(rng, n, fs, kind).astype(np.float32).astype(np.float64), fs)
        gm.AUDIO[name] = audio[name]
    for fs, la, lb, short, tiny, long_, rir in ((16000, 4000, 4400, 3000, 1300, 7000, 1100), (8000, 4000, 4003, 2500, 900, 6000, 700)):
        add("sp%d_a" % fs, la, fs, "speech")
        add("sp%d_b" % fs, lb, fs, "speech")
        add("nz%d_short" % fs, short, fs, "noise")
        add("nz%d_tiny" % fs, tiny, fs, "noise")
        add("nz%d_long" % fs, long_, fs, "noise")
        add("rir%d" % fs, rir, fs, "rir")
    add("nz16000_equal", 4000, 16000, "noise")
    add("nz8000_equal", 4003, 8000, "noise")
    cases = [  # (speech, noise, rir, augmentation, snr, highpass, store the noise)
        ("sp16000_a", "nz16000_short", "none", "none", 5.5, True, True),
        ("sp16000_a", "nz16000_tiny", "none", "none", 0.25, True, False),                # speech > 2 x noise: several wraps
        ("sp16000_a", "nz16000_long", "none", "none", 12.0, False, False),
        ("sp16000_a", "nz16000_equal", "none", "none", -3.0, True, False),
        ("sp16000_b", "nz16000_short", "rir16000", "none", 8.0, True, False),
        ("sp16000_b", "nz16000_tiny", "none", "packet_loss(packet_loss_indices=[1, 2, 9, 11],packet_duration_ms=20)", 10.0, False, False),
        ("sp16000_b", "nz16000_short", "rir16000",
         "packet_loss(packet_loss_indices=[3, 4, 12],packet_duration_ms=20)/clipping(min=0.03,max=0.95)", 4.0, True, True),
        ("sp8000_a", "nz8000_long", "none", "clipping(min=0.06,max=0.93)", 15.0, True, False),
        ("sp8000_a", "nz8000_tiny", "rir8000", "clipping(min=0.1,max=0.9)", 2.0, False, True),
        ("sp8000_b", "nz8000_equal", "none", "packet_loss(packet_loss_indices=[0, 7],packet_duration_ms=20)", 9.0, True, False),
    ]
    ident = {k: k for k in audio}
    for i, (sp, nz, rir, aug, snr, hp, keep_noise) in enumerate(cases):
        uid = "fileid_%d" % (17 + 3 * i)
        fs = audio[sp][1]
        info = {"id": uid, "fs": str(fs), "snr_dB": repr(snr), "speech_uid": sp, "noise_uid": nz, "rir_uid": rir, "augmentation": aug,
                "length": str(len(audio[sp][0])), "clean_path": "clean/%s" % uid, "noisy_path": "noisy/%s" % uid,
                "noise_path": "noise/%s" % uid}
        sim.process_one_sample(dict(info), store_noise=True, speech_dic=ident, noise_dic=ident, rir_dic=ident, highpass=hp, on_the_fly=False)
        for kind in ("clean", "noisy", "noise"):
            x, wfs = WRITTEN["%s/%s" % (kind, uid)]
            assert wfs == fs and x.shape == (len(audio[sp][0]),)
            if kind != "noise" or keep_noise:
                out["sim_%s_%d" % (kind, i)] = x
        ls, ln = len(audio[sp][0]), len(audio[nz][0])
        off = 0 if ls == ln else int(np.random.default_rng(int(uid.split("_")[-1])).integers(0, abs(ls - ln)))
        rows.append([uid, str(fs), repr(snr), sp, nz, rir, aug, str(ls), "1" if hp else "", str(off)])
    out["sim_rows"] = np.array(rows)
    out["sim_row_fields"] = np.array(["id", "fs", "snr_dB", "speech_uid", "noise_uid", "rir_uid", "augmentation", "length", "highpass",
                                      "noise_offset"])
    out["sim_audio_names"] = np.array(list(audio))
    out["sim_audio_fs"] = np.array([audio[k][1] for k in audio])
    for k in audio:
        out["sim_audio_" + k] = audio[k][0].astype(np.float32)
    return out


def main():
    gm.install_stand_ins()
    sys.modules["soundfile"].write = capture_write
    sys.modules["tqdm"] = types.ModuleType("tqdm")
    sys.modules["tqdm"].tqdm = lambda it, **kw: it
    sys.modules["tqdm.contrib"] = types.ModuleType("tqdm.contrib")
    sys.modules["tqdm.contrib.concurrent"] = types.ModuleType("tqdm.contrib.concurrent")
    sys.modules["tqdm.contrib.concurrent"].process_map = None
    gen = importlib.import_module("simulation.generate_data_param")
    sim = importlib.import_module("simulation.simulate_data_from_param")
    meta = meta_fixture(gen)
    p = os.path.join(HERE, "ref_meta.npz")
    np.savez_compressed(p, **meta)
    print("wrote", p, os.path.getsize(p), "bytes")
    simu = simulate_fixture(sim)
    p = os.path.join(HERE, "ref_simulate.npz")
    np.savez_compressed(p, **simu)
    print("wrote", p, os.path.getsize(p), "bytes")


if __name__ == "__main__":
    main()
