"""``python -m urgent2026_challenge_track1_amd.resample_to_estimated_bandwidth --bandwidth_data BW --out_scpfile SCP --outdir DIR``

The reference's ``utils/resample_to_estimated_bandwidth.py:44-76`` with its flags: every file is resampled to the lowest of
the seven challenge rates that holds its estimated bandwidth (``bandwidth.pick_rate``) and written as 16-bit WAV to
``outdir/<idx // max_files as hex, num_digits wide>/<uid>.wav``; an existing output file is not made again (and is listed);
a file already at its target rate keeps its original path.  Out scp: lines ``uid fs path``.

``soxr.resample`` (HQ) is ``metrics.resample_soxr_hq``: the polyphase kernel with a filter built to soxr HQ's specification,
every channel a row.  It is not pinned to libsoxr bit for bit, as everywhere else in this package.

Deviations from the reference's ``__main__`` (see also ``estimate_audio_bandwidth``): the non-JSON bandwidth file is read as
lines ``uid bandwidth path`` (the reference's branch reads an argument that does not exist); an unreadable file is skipped
with the reference's message instead of failing the final unpacking; ``num_digits`` is at least 1 (the reference's
``ceil(log16(n / max_files))`` is negative below ``max_files`` files and its format then raises; from ``max_files`` files
on the names are the same).  ``--nj`` is the number of reader THREADS (at most 16).
"""
import argparse
import math
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import torch

from . import audio_io, bandwidth
from .estimate_audio_bandwidth import read_bandwidth_file
from .metrics import resample_soxr_hq


def num_digits_for(n_files, max_files):
    return max(1, math.ceil(math.log(n_files / max_files, 16))) if n_files > 0 else 1


def subdir_name(idx, max_files, num_digits):
    return f"{idx // max_files:0{num_digits}x}"


def resample_channels(audio, fs, est_fs, device="cuda"):
    """float32 [C, L] at ``fs`` -> float32 [C, ceil(L est_fs / fs)] at ``est_fs`` (numpy), every channel through the device resampler."""
    y = resample_soxr_hq(torch.from_numpy(audio).to(device), fs, est_fs)
    return y.cpu().numpy()


def _read(job):
    uid, audio_path, est_fs, outfile = job
    if outfile.exists():
        return None
    try:
        return audio_io.read_audio_all(str(audio_path))
    except Exception:
        print(f"Error: cannot open audio file '{audio_path}'. Skipping it", flush=True)
        return "error"


def resample_files(audios, outdir, max_files=10000, nj=1, chunksize=1, device="cuda"):
    """[(uid, path, bandwidth)] -> [(uid, path, fs)] of the files that could be read, in input order."""
    num_digits = num_digits_for(len(audios), max_files)
    Path(outdir).mkdir(parents=True, exist_ok=True)
    jobs = []
    for idx, (uid, audio_path, bw) in enumerate(audios):
        est_fs = bandwidth.pick_rate(float(bw))
        jobs.append((uid, audio_path, est_fs, Path(outdir) / subdir_name(idx, max_files, num_digits) / (uid + ".wav")))
    ret = []
    nthreads = max(1, min(int(nj), 16))
    block = nthreads * max(1, int(chunksize))
    with ThreadPoolExecutor(max_workers=nthreads) as pool:
        for b0 in range(0, len(jobs), block):
            part = jobs[b0:b0 + block]
            for (uid, audio_path, est_fs, outfile), got in zip(part, pool.map(_read, part)):
                if got is None:                       # already resampled
                    ret.append((uid, outfile, est_fs))
                    continue
                if isinstance(got, str):
                    continue
                audio, fs = got
                if est_fs == fs:
                    ret.append((uid, audio_path, fs))
                    continue
                outfile.parent.mkdir(parents=True, exist_ok=True)
                audio_io.write_audio_channels(str(outfile), resample_channels(audio, fs, est_fs, device), est_fs)
                ret.append((uid, outfile, est_fs))
    return ret


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--bandwidth_data", type=str, required=True,
                        help="Path to the json (or `uid bandwidth path` text) file written by estimate_audio_bandwidth")
    parser.add_argument("--out_scpfile", type=str, required=True, help="Path to the output scp file")
    parser.add_argument("--outdir", type=str, required=True, help="Output directory for storing resampled audios")
    parser.add_argument("--nj", type=int, default=1, help="Number of reader threads (at most 16)")
    parser.add_argument("--chunksize", type=int, default=1, help="Files decoded per reader thread at a time")
    parser.add_argument("-m", "--max_files", type=int, default=10000, help="The maximum number of files per sub-directory")
    args = parser.parse_args(argv)
    audios = read_bandwidth_file(args.bandwidth_data)
    ret = resample_files(audios, args.outdir, max_files=args.max_files, nj=args.nj, chunksize=args.chunksize)
    Path(args.out_scpfile).parent.mkdir(parents=True, exist_ok=True)
    with open(args.out_scpfile, "w") as f:
        for uid, audio_path, fs in ret:
            f.write(f"{uid} {fs} {audio_path}\n")
    return ret


if __name__ == "__main__":
    main()
