"""``python -m urgent2026_challenge_track1_amd.utt2numsamples --input_scp wav.scp --outfile speech_length.scp``
(``utils/utt2numsamples.py``): ``uid samples`` per line of an scp with two (``uid path``) or three (``uid fs path``) columns.  The
recipes run it on the simulated ``wav.scp``; ``PreSimulatedDataset`` reads the result.  A .wav answers from its header, anything else
is decoded in full (:77-82), as the generator does."""
import argparse
import sys

from .generate_data_param import ConfigArgumentParser, speech_frames


def get_parser():
    class Formatter(argparse.RawTextHelpFormatter, argparse.ArgumentDefaultsHelpFormatter):
        pass
    parser = ConfigArgumentParser(description="base parser", formatter_class=Formatter)
    parser.add_argument("--input_scp", type=str, required=True, help="Path to the scp file containing speech samples")
    parser.add_argument("--outfile", type=str, required=True, help="Path to the output file")
    return parser


def read_flat_scp(scp):
    """{uid: path}; a uid may not repeat within a rate (two-column lines count as rate 0)"""
    seen, flat = set(), {}
    with open(scp, "r") as f:
        for line in f:
            parts = line.strip().split()
            uid, fs, path = parts if len(parts) == 3 else (parts[0], 0, parts[1])
            assert (int(fs), uid) not in seen, (uid, fs)
            seen.add((int(fs), uid))
            flat[uid] = path
    return flat


def main(argv=None):
    args = get_parser().parse_args(argv)
    print(args)
    with open(args.outfile, "w") as out:
        for uid, path in read_flat_scp(args.input_scp).items():
            print("%s %d" % (uid, speech_frames(path)), file=out)


if __name__ == "__main__":
    main(sys.argv[1:])
