"""``python -m urgent2026_challenge_track1_amd.simulate_data_from_param``: ``log_dir/meta.tsv`` -> the clean / noisy / noise files
``PreSimulatedDataset`` trains and validates on (``simulation/simulate_data_from_param.py``; the second step of
utils/prepare_train_data.sh / prepare_validation_data.sh).

Per row this is ``process_one_sample(on_the_fly=False)`` (:441-589).  The host reads the sources and draws the row's noise offset from
its id-seeded generator (:481, :110 / :118); everything else runs batched on the device: rows of one ``fs`` are sorted by length, cut into
ragged batches under a sample budget and go through ``mixing.simulate_recipes`` (resampling of sources at another rate, high-pass,
RIR / early-RIR convolution, noise tiling or cropping, SNR scaling, the augmentation chain, joint peak normalisation), are quantised to
16 bit there, and ``.flac`` outputs are encoded there too (csrc/flac_enc.hip).  ``.wav`` outputs go through ``write_audio``.

Flags: the generator's, plus ``--meta_tsv``, ``--nj``, ``--chunksize``, ``--highpass`` (:592-622), ``--unsupported_augmentation`` and
``--wind_noise_compressor``.
  * ``--highpass`` keeps the reference's ``type=bool``: ANY non-empty string is true, ``--highpass False`` included; only leaving the
    flag out (or ``--highpass ""``) switches the filter off.
  * The reference reads ``log_dir/meta.tsv`` and never opens ``--meta_tsv``; so does this module, and it refuses a ``--meta_tsv`` that
    names another file instead of silently ignoring it.
  * ``--nj``: host reader / writer threads (at most 16).  ``--chunksize``: upper bound of rows per device batch.
  * ``codec`` and the wind-noise side-chain compressor (ffmpeg) are not applied, exactly as in the on-the-fly path: a wind row is mixed
    additively at its drawn SNR.  ``--unsupported_augmentation warn|raise|count`` (default warn; the trainer's semantics): ``raise``
    stops before anything is simulated, ``warn`` warns once, and every affected row is listed in ``log_dir/unsupported.tsv``
    (id, augmentation) under all three - a dataset on disk must say what it lacks.
  * ``--wind_noise_compressor skip|device`` (default skip: the line above).  ``device``: a wind row is mixed by ``wind_noise()`` (:129-217) on
    the device - 16-bit round trips, ffmpeg's ``sidechaincompress`` + ``amix`` restated from their published definition (not pinned against
    the binary), the clipper - and is no longer listed as lacking.
"""
import ast
import os
import re
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

from .audio_io import read_audio, write_audio
from .generate_data_param import check_required, get_parser as base_parser

SAMPLE_BUDGET = 1 << 23          # samples (rows x longest row) per device batch: 32 MB per f32 signal


def get_parser():
    parser = base_parser()
    g = parser.add_argument_group(description="New arguments")
    g.add_argument("--meta_tsv", type=str, required=True, help="Path to the tsv file containing meta information for simulation\n"
                   "(read from log_dir/meta.tsv, as the reference does; another path is refused)")
    g.add_argument("--nj", type=int, default=8, help="Number of host reader / writer threads (at most 16)")
    g.add_argument("--chunksize", type=int, default=1000, help="Upper bound of rows per device batch")
    g.add_argument("--highpass", type=bool, default=False,
                   help="Apply highpass filter to source speech (type=bool as in the reference: any non-empty string is true)")
    g.add_argument("--unsupported_augmentation", choices=("warn", "raise", "count"), default="warn",
                   help="what to do with rows whose codec / wind-noise compressor the device simulator does not apply")
    g.add_argument("--wind_noise_compressor", choices=("skip", "device"), default="skip",
                   help="skip: wind noise is mixed additively and the row listed as lacking; device: the side-chain compressor recipe "
                        "runs on the device (ffmpeg's filter restated, not pinned against the binary)")
    return parser


def read_flat_scps(paths):
    table = {}
    for scp in paths or []:
        with open(scp, "r") as f:
            for line in f:
                uid, fs, path = line.strip().split()
                assert uid not in table, (uid, fs)
                table[uid] = path
    return table


def read_meta(log_dir):
    rows = []
    with open(Path(log_dir) / "meta.tsv", "r") as f:
        headers = next(f).strip().split("\t")
        for line in f:
            rows.append(dict(zip(headers, line.strip().split("\t"))))
    return rows


def check_meta_path(meta_tsv, log_dir):
    want = Path(log_dir) / "meta.tsv"
    same = os.path.samefile(meta_tsv, want) if os.path.exists(meta_tsv) and os.path.exists(want) else \
        os.path.abspath(meta_tsv) == os.path.abspath(want)
    if not same:
        raise ValueError("--meta_tsv %s is not %s: the rows are read from log_dir/meta.tsv (as the reference does, which never opens "
                         "--meta_tsv); pass that file or move it" % (meta_tsv, want))


def noise_offset(uid, len_speech, len_noise):
    """the draw of mix_noise (:110 / :118) from the row's generator ``default_rng(int(uid.split("_")[-1]))`` (:481)"""
    if len_speech == len_noise:
        return 0
    return int(np.random.default_rng(int(uid.split("_")[-1])).integers(0, abs(len_speech - len_noise)))


WIND_FIELDS = ("threshold", "ratio", "attack", "release", "sc_gain", "clipping", "clipping_threshold")


def parse_row(info, highpass, wind_compressor=False):
    """a meta.tsv row -> the recipe ``mixing.simulate_recipes`` takes, and the augmentations it will not apply.  ``wind_compressor``: the
    seven fields of a wind row's ``wind_noise(...)`` text go to ``params["wind_noise"]`` (:494-518; ``clipping`` as the reference evaluates it,
    ``bool(text)``: true for "False" too) and the row is not listed as lacking."""
    params, order, unsupported = {}, [], []
    wind = info["noise_uid"].startswith("wind_noise")
    parts = info["augmentation"].split("/")
    if wind:
        mine = [a for a in parts if a.startswith("wind_noise")]
        assert len(mine) == 1, "Configuration for the wind-noise simulation is necessary: %s %s" % (parts, info["noise_uid"])
        if wind_compressor:
            vals = re.fullmatch(r"wind_noise\(threshold=(.*),ratio=(.*),attack=(.*),release=(.*),sc_gain=(.*),clipping=(.*),"
                                r"clipping_threshold=(.*)\)", mine[0]).groups()
            params["wind_noise"] = {k: bool(v) if k == "clipping" else float(v) for k, v in zip(WIND_FIELDS, vals)}
        else:
            unsupported.append("wind_noise")
    for a in parts:
        if a in ("none", "") or a.startswith("wind_noise"):
            continue
        if a.startswith("bandwidth_limitation"):
            res_type, fs_new = re.fullmatch(r"bandwidth_limitation-(.*)->(\d+)", a).groups()
            params["bandwidth_limitation"] = dict(res_type=res_type, fs_new=int(fs_new))
            order.append("bandwidth_limitation")
        elif a.startswith("clipping"):
            lo, hi = map(float, re.fullmatch(r"clipping\(min=(.*),max=(.*)\)", a).groups())
            params["clipping"] = dict(min_quantile=lo, max_quantile=hi)
            order.append("clipping")
        elif a.startswith("codec"):
            fmt, enc, q = re.fullmatch(r"codec\(format=(.*),encoder=(.*),qscale=(.*)\)", a).groups()
            params["codec"] = dict(format=fmt, encoder=enc, qscale=int(q))
            order.append("codec")
            unsupported.append("codec")
        elif a.startswith("packet_loss"):
            idx, ms = re.fullmatch(r"packet_loss\(packet_loss_indices=(.*),packet_duration_ms=(.*)\)", a).groups()
            if int(ms) != 20:
                raise NotImplementedError("%s: packets of %s ms (the device kernel zeroes 20 ms packets)" % (info["id"], ms))
            params["packet_loss"] = dict(packet_loss_indices=ast.literal_eval(idx), packet_duration_ms=int(ms))
            order.append("packet_loss")
        else:
            raise NotImplementedError(a)
    fs = int(info["fs"])
    recipe = dict(id=info["id"], snr=float(info["snr_dB"]), params=params, order=order, wind=wind, highpass=bool(highpass), fs=fs,
                  length=int(info["length"]))
    if "bandwidth_limitation" in params:
        from . import mixing
        bw = params["bandwidth_limitation"]
        if bw["res_type"] not in ("polyphase", "scipy", "kaiser_best", "kaiser_fast", "none") or (
                bw["res_type"] == "scipy" and mixing._fft_resample_span(recipe["length"], fs, bw["fs_new"]) > mixing.FFT_RESAMPLE_MAX):
            unsupported.append("bandwidth_limitation")
    return recipe, unsupported


def plan_batches(rows, chunksize, budget=SAMPLE_BUDGET):
    """indices of ``rows`` grouped by fs, sorted by length, cut so that rows x longest row stays under ``budget``"""
    by_fs = {}
    for i, r in enumerate(rows):
        by_fs.setdefault(int(r["fs"]), []).append(i)
    batches = []
    for fs in sorted(by_fs):
        cur = []
        for i in sorted(by_fs[fs], key=lambda i: (int(rows[i]["length"]), i)):
            if cur and (len(cur) >= chunksize or (len(cur) + 1) * int(rows[i]["length"]) > budget):
                batches.append(cur)
                cur = []
            cur.append(i)
        if cur:
            batches.append(cur)
    return batches


def load_item(info, recipe, speech_dic, noise_dic, rir_dic):
    """the host side of one row: the sources as read, and the noise offset.  A source at another rate than the row's travels raw with
    its rate (it is resampled on the device, soxr-HQ specification) - a long noise only as far as its window needs."""
    from .dataset import DynamicMixingDataset as D
    fs = recipe["fs"]
    speech, speech_fs = read_audio(speech_dic[info["speech_uid"]])
    noise, noise_fs = read_audio(noise_dic[info["noise_uid"]])
    rir, rir_fs = (None, fs)
    if info["rir_uid"] != "none":
        rir, rir_fs = read_audio(rir_dic[info["rir_uid"]])
    ls = D.resampled_length(speech.shape[1], speech_fs, fs)
    ln = D.resampled_length(noise.shape[1], noise_fs, fs)
    recipe = dict(recipe, noise_offset=noise_offset(info["id"], ls, ln))
    if ln > ls:                  # only the window [offset, offset + ls) is used: do not upload the rest
        if noise_fs == fs:
            noise, recipe["noise_offset"] = noise[:, recipe["noise_offset"]:recipe["noise_offset"] + ls], 0
        else:
            noise, recipe["noise_offset"] = D.crop_for_resampling(noise, noise_fs, fs, recipe["noise_offset"], ls)
    return dict(speech=speech, speech_fs=int(speech_fs), noise=noise, rir=rir, recipe=recipe, fs=fs, length=ls, noise_fs=int(noise_fs),
                rir_fs=int(rir_fs))


def simulate_items(items, device, skipped=None, wind_compressor=False):
    """items of one fs -> (clean, noisy, noise) f32 [B, T] on the device, lengths"""
    import torch
    from .dataset import RawMixBatch
    from .metrics import resample_soxr_hq
    fs = items[0]["fs"]
    for it in items:             # speech listed at another rate than its file's: resampled on its own (rare: the scp states the file's rate)
        if it["speech_fs"] != fs:
            x = torch.as_tensor(it["speech"], dtype=torch.float32).to(device)
            it["speech"] = resample_soxr_hq(x, it["speech_fs"], fs)[:, :it["length"]].cpu().numpy()
    batch = RawMixBatch(items)
    clean, noisy, noise = batch.simulate(device, skipped, return_noise=True, wind_compressor=wind_compressor)
    return clean, noisy, noise, batch.lengths


def write_batch(signals, lens, fs, paths, pool):
    """signals: f32 [R, T] device rows, one file each.  Quantised on the device; .flac rows are encoded there in one call, .wav rows
    leave through ``write_audio`` (whose rounding the quantiser shares: both formats hold the same samples)."""
    import torch
    from . import flac
    lens_d = torch.as_tensor(lens, dtype=torch.int32).to(signals.device)
    as_flac = [i for i, p in enumerate(paths) if p.endswith(".flac")]
    as_wav = [i for i, p in enumerate(paths) if p.endswith(".wav")]
    other = [p for p in paths if not p.endswith((".flac", ".wav"))]
    if other:
        raise NotImplementedError("output format of %s: only .flac and .wav are written" % other[0])
    jobs = []
    if as_flac:
        pcm = flac.quantise_pcm16(signals[as_flac].contiguous(), lens_d[as_flac])
        files = flac.encode_flac(pcm, [lens[i] for i in as_flac], fs)
        jobs += [(paths[i], data) for i, data in zip(as_flac, files)]
    if as_wav:
        host = signals[as_wav].cpu().numpy()
        jobs += [(paths[i], (host[k, :lens[i]], fs)) for k, i in enumerate(as_wav)]

    def put(job):
        path, data = job
        Path(path).parent.mkdir(parents=True, exist_ok=True)
        if isinstance(data, bytes):
            with open(path, "wb") as f:
                f.write(data)
        else:
            write_audio(path, data[0], data[1])
    list(pool.map(put, jobs))


def run(args, device="cuda"):
    check_meta_path(args.meta_tsv, args.log_dir)
    speech_dic = read_flat_scps(args.speech_scps)
    noise_dic = read_flat_scps(args.noise_scps)
    noise_dic.update(read_flat_scps(args.wind_noise_scps))
    rir_dic = read_flat_scps(args.rir_scps)
    rows = read_meta(args.log_dir)
    wind_compressor = getattr(args, "wind_noise_compressor", "skip") == "device"
    parsed = [parse_row(r, args.highpass, wind_compressor) for r in rows]
    lacking = [(r["id"], a) for r, (_, un) in zip(rows, parsed) for a in un]
    policy = args.unsupported_augmentation
    if lacking:
        msg = ("%d row(s) of meta.tsv carry an augmentation the device simulator does not apply (%s): it is skipped for that row%s; "
               "the rows are listed in %s (--unsupported_augmentation warn | raise | count)"
               % (len({i for i, _ in lacking}), sorted({a for _, a in lacking}),
                  "" if wind_compressor else " (wind noise is mixed additively at its drawn SNR)", Path(args.log_dir) / "unsupported.tsv"))
        if policy == "raise":
            raise NotImplementedError(msg)
        if policy == "warn":
            print("WARNING: " + msg, flush=True)
    with open(Path(args.log_dir) / "unsupported.tsv", "w") as f:
        f.write("id\taugmentation\n")
        for i, a in lacking:
            f.write("%s\t%s\n" % (i, a))
    nj = max(1, min(16, int(args.nj)))
    skipped = {}
    with ThreadPoolExecutor(max_workers=nj) as pool:
        for members in plan_batches(rows, max(1, int(args.chunksize))):
            items = list(pool.map(lambda i: load_item(rows[i], parsed[i][0], speech_dic, noise_dic, rir_dic), members))
            for i, it in zip(members, items):                     # the reference's assertion (:572-573), before any device work
                if it["length"] != int(rows[i]["length"]):
                    raise AssertionError("%s: the speech has %d samples at %d Hz, meta.tsv says length %s"
                                         % (rows[i]["id"], it["length"], it["fs"], rows[i]["length"]))
            clean, noisy, noise, lens = simulate_items(items, device, skipped, wind_compressor)
            fs = items[0]["fs"]
            write_batch(clean, lens, fs, [rows[i]["clean_path"] for i in members], pool)
            write_batch(noisy, lens, fs, [rows[i]["noisy_path"] for i in members], pool)
            if args.store_noise:
                write_batch(noise, lens, fs, [rows[i]["noise_path"] for i in members], pool)
    if skipped and policy != "raise":
        print("not applied: %s" % dict(sorted(skipped.items())), flush=True)
    return len(rows), lacking


def main(argv=None):
    parser = get_parser()
    args = parser.parse_args(argv)
    check_required(parser, args)
    print(args)
    return run(args)


if __name__ == "__main__":
    main(sys.argv[1:])
