"""``python -m urgent2026_challenge_track1_amd.generate_data_param``: one degradation recipe per utterance into ``log_dir/meta.tsv``
(``simulation/generate_data_param.py``; the first step of utils/prepare_train_data.sh / prepare_validation_data.sh).  Host only.

Same flags (:458-622), same ``np.random`` call sequence, same text: for the same scp files, YAML and seed the file equals the
reference's byte for byte (tests/golden/ref_meta.npz).  The per-sample draw is ``dataset.draw_recipe``; what this module adds is the
offline bookkeeping around it: ``select_sample`` with its used pools and ``reuse_*`` flags (:421-452), the rate-descending outer loop
with ``repeat_per_utt``, the 5000-files-per-directory rule and the column order.

``--config file.yaml`` follows espnet2.utils.config_argparse: the YAML's values become the parser's defaults (no type check; a key that
is no flag is an error), the command line overrides them, and every name in ``required`` must end up set.
"""
import argparse
import random
import sys
from collections import defaultdict
from pathlib import Path

import numpy as np

from .audio_io import audio_frames, read_audio_all
from .dataset import draw_recipe


def str2bool(value):
    """espnet2.utils.types.str2bool (distutils' strtobool)."""
    v = str(value).lower()
    if v in ("y", "yes", "t", "true", "on", "1"):
        return True
    if v in ("n", "no", "f", "false", "off", "0"):
        return False
    raise ValueError("invalid truth value %r" % (value,))


class ConfigArgumentParser(argparse.ArgumentParser):
    """argparse + ``--config``: a first parse finds the file, its mapping is installed with ``set_defaults``, a second parse lets the
    command line win."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.add_argument("--config", help="Give config file in yaml format")

    def parse_known_args(self, args=None, namespace=None):
        import yaml
        first, _ = super().parse_known_args(args, namespace)
        if first.config is not None:
            if not Path(first.config).exists():
                self.error("No such file: %s" % first.config)
            with open(first.config, "r", encoding="utf-8") as f:
                values = yaml.safe_load(f)
            if not isinstance(values, dict):
                self.error("Config file has non dict value: %s" % first.config)
            known = {a.dest for a in self._actions}
            for key in values:
                if key not in known:
                    self.error("unrecognized arguments: %s (from %s)" % (key, first.config))
            self.set_defaults(**values)
        return super().parse_known_args(args, namespace)


def check_required(parser, args):
    missing = ["--" + name for name in (getattr(args, "required", None) or []) if getattr(args, name, None) is None]
    if missing:
        parser.error("The following arguments are required: %s" % ", ".join(missing))


def get_parser(parser=None):
    if parser is None:
        class Formatter(argparse.RawTextHelpFormatter, argparse.ArgumentDefaultsHelpFormatter):
            pass
        parser = ConfigArgumentParser(description="base parser", formatter_class=Formatter)
    g = parser.add_argument_group(description="General arguments")
    g.add_argument("--speech_scps", type=str, nargs="+", help="Path to the scp file containing speech samples")
    g.add_argument("--speech_utt2spk", type=str, nargs="+", help="Path to the utt2spk file containing speaker mappings")
    g.add_argument("--speech_text", type=str, nargs="+", help="Path to the text file containing transcripts")
    g.add_argument("--log_dir", type=str, help="Log directory for storing log and scp files")
    g.add_argument("--output_dir", type=str, help="Output directory for storing processed audio files")
    g.add_argument("--out_format", type=str, default="flac", help="Output audio format")
    g.add_argument("--repeat_per_utt", type=int, default=1,
                   help="Number of times to use each utterance\n(The final amount of simulated samples will be "
                        "`repeat_per_utt` * size(speech_scp))")
    g.add_argument("--seed", type=int, default=0, help="Random seed")
    g = parser.add_argument_group(description="Additive noise related")
    g.add_argument("--noise_scps", type=str, nargs="+", help="Path to the scp file containing noise samples")
    g.add_argument("--snr_low_bound", type=float, default=-5.0, help="Lower bound of signal-to-noise ratio (SNR) in dB")
    g.add_argument("--snr_high_bound", type=float, default=20.0, help="Higher bound of signal-to-noise ratio (SNR) in dB")
    g.add_argument("--reuse_noise", type=str2bool, default=False, help="Whether or not to allow reusing noise samples")
    g.add_argument("--store_noise", type=str2bool, default=False, help="Whether or not to store parallel noise samples")
    g = parser.add_argument_group(description="Wind-noise related")
    g.add_argument("--wind_noise_scps", type=str, nargs="+",
                   help="Path to the scp file containing wind noise samples\n(If not provided, wind noise will not be applied)")
    g.add_argument("--prob_wind_noise", type=float, default=0.05,
                   help="Probability of using wind noise instead of other environmental noise to input speech samples")
    g.add_argument("--wind_noise_config", type=dict, default={}, help="Ranges of the wind-noise simulation (from the YAML)")
    g.add_argument("--reuse_wind_noise", type=str2bool, default=False, help="Whether or not to allow reusing wind noise samples")
    g.add_argument("--wind_noise_snr_low_bound", type=float, default=-5.0, help="Lower bound of signal-to-noise ratio (SNR) in dB")
    g.add_argument("--wind_noise_snr_high_bound", type=float, default=20.0, help="Higher bound of signal-to-noise ratio (SNR) in dB")
    g = parser.add_argument_group(description="Reverberation related")
    g.add_argument("--rir_scps", type=str, nargs="+",
                   help="Path to the scp file containing RIR samples\n(If not provided, reverberation will not be applied)")
    g.add_argument("--prob_reverberation", type=float, default=0.5,
                   help="Probability of randomly adding reverberation to input speech samples")
    g.add_argument("--reuse_rir", type=str2bool, default=False, help="Whether or not to allow reusing RIR samples")
    g = parser.add_argument_group(description="Additional augmentation related")
    g.add_argument("--augmentations", default=dict(none=dict(weight=1.0)),
                   help="Dict of mutually-exclusive augmentations to apply to input speech samples")
    g.add_argument("--num_augmentations", default=dict(), help="Dict {number of augmentations: probability}")
    parser.set_defaults(required=["speech_scps", "log_dir", "output_dir", "noise_scps"])
    return parser


def read_rate_scp(paths):
    """``uid fs path`` lines of several scp files -> {fs: {uid: path}} (a uid may not repeat within a rate)."""
    table = defaultdict(dict)
    for scp in paths or []:
        with open(scp, "r") as f:
            for line in f:
                uid, fs, path = line.strip().split()
                assert uid not in table[int(fs)], (uid, fs)
                table[int(fs)][uid] = path
    return table


def read_kv(paths, maxsplit=-1):
    table = {}
    for scp in paths or []:
        with open(scp, "r") as f:
            for line in f:
                uid, value = line.strip().split(maxsplit=maxsplit)
                assert uid not in table, (uid, value)
                table[uid] = value
    return table


def select_sample(fs, pool, used=None, reuse=False, rs=np.random):
    """``select_sample`` (:421-452): an unused sample at ``fs``; else one at a higher rate, found by walking a SHUFFLED list of the rates;
    a picked sample moves to ``used``.  When neither exists and ``reuse`` holds, the same search over the used pool (nothing moves)."""
    if fs not in pool.keys() or len(pool[fs]) == 0:
        rates = list(pool.keys())
        rs.shuffle(rates)
        for other in rates:
            if other > fs and len(pool[other]) > 0:
                uid = rs.choice(list(pool[other].keys()))
                if used is not None:
                    used[other][uid] = pool[other].pop(uid)
                return uid
        if reuse:
            return select_sample(fs, used, None, False, rs)
        return None
    uid = rs.choice(list(pool[fs].keys()))
    if used is not None:
        used[fs][uid] = pool[fs].pop(uid)
    return uid


def speech_frames(path):
    """the header's frame count for .wav, a full decode otherwise (:213-218: 'sometimes the loaded length differs from af.frames')."""
    if path.endswith(".wav"):
        return audio_frames(path)
    return read_audio_all(path)[0].shape[1]


class _DrawConfig:
    """the attribute bag ``draw_recipe`` reads, filled from the command line / YAML"""

    def __init__(self, args):
        self.snr_low_bound, self.snr_high_bound = args.snr_low_bound, args.snr_high_bound
        self.prob_wind_noise, self.prob_reverberation = args.prob_wind_noise, args.prob_reverberation
        self.wind_noise_config = dict(args.wind_noise_config, wind_noise_snr_low_bound=args.wind_noise_snr_low_bound,
                                      wind_noise_snr_high_bound=args.wind_noise_snr_high_bound)
        self.num_augmentations, self.augmentations = args.num_augmentations, args.augmentations


def run(args, frames=speech_frames):
    """``main`` (:122-291)."""
    speech = read_rate_scp(args.speech_scps)
    utt2spk = read_kv(args.speech_utt2spk)
    text = read_kv(args.speech_text, maxsplit=1)
    pools = {"noise": read_rate_scp(args.noise_scps), "wind": read_rate_scp(args.wind_noise_scps)}
    reuse = {"noise": args.reuse_noise, "wind": True, "rir": args.reuse_rir}       # (wind noise is always reused, :313-315)
    rir_table = None
    if args.rir_scps is not None and args.prob_reverberation > 0.0:
        rir_table = pools["rir"] = read_rate_scp(args.rir_scps)
    used = {k: {fs: {} for fs in pool.keys()} for k, pool in pools.items()}
    kind_of = {id(pool): k for k, pool in pools.items()}

    def pick(fs, pool):
        k = kind_of[id(pool)]
        return select_sample(fs, pool, used[k], reuse[k])
    cfg = _DrawConfig(args)
    outdir = Path(args.output_dir)
    headers = ["id", "noisy_path", "speech_uid", "speech_sid", "clean_path", "noise_uid"]
    if args.store_noise:
        headers.append("noise_path")
    headers += ["snr_dB", "rir_uid", "augmentation", "fs", "length", "text"]
    count = 0
    with open(Path(args.log_dir) / "meta.tsv", "w") as f:
        f.write("\t".join(headers) + "\n")
        for fs in sorted(speech.keys(), reverse=True):
            for uid, path in speech[fs].items():
                sid = utt2spk[uid]
                transcript = text.get(uid, "<not-available>")
                length = frames(path)
                for _ in range(args.repeat_per_utt):
                    info = draw_recipe(length, fs, pools["noise"], rir_table, pools["wind"], cfg, np.random, pick)
                    count += 1
                    filedir = str(count // 5000)                      # at most 5000 files per directory
                    (outdir / "noisy" / filedir).mkdir(parents=True, exist_ok=True)
                    (outdir / "clean" / filedir).mkdir(parents=True, exist_ok=True)
                    filename = "fileid_%d.%s" % (count, args.out_format)
                    row = ["fileid_%d" % count, str(outdir / "noisy" / filedir / filename), uid, sid,
                           str(outdir / "clean" / filedir / filename), str(info["noise_uid"])]
                    if args.store_noise:
                        (outdir / "noise" / filedir).mkdir(parents=True, exist_ok=True)
                        row.append(str(outdir / "noise" / filedir / filename))
                    row += [str(info["snr"]), str(info["rir_uid"]), info["augmentation"], str(info["fs"]), str(info["length"]), transcript]
                    f.write("\t".join(row) + "\n")
    return count


def main(argv=None, frames=speech_frames):
    parser = get_parser()
    args = parser.parse_args(argv)
    check_required(parser, args)
    print(args)
    assert len(args.speech_utt2spk) == len(args.speech_scps)
    if args.speech_text:
        assert len(args.speech_text) == len(args.speech_scps)
    if args.prob_reverberation > 0:
        assert args.rir_scps
    outdir = Path(args.output_dir)
    (outdir / "clean").mkdir(parents=True, exist_ok=True)
    (outdir / "noisy").mkdir(parents=True, exist_ok=True)
    if args.store_noise:
        (outdir / "noise").mkdir(parents=True, exist_ok=True)
    Path(args.log_dir).mkdir(parents=True, exist_ok=True)
    random.seed(args.seed)
    np.random.seed(args.seed)
    return run(args, frames)


if __name__ == "__main__":
    main(sys.argv[1:])
