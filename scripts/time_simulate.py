"""Where the time of the offline simulator goes: a synthetic corpus (bench.py's speech-like generator; --rows
utterances of 4-10 s, half at 16 kHz and half at 48 kHz, white / coloured noise files, a few RIRs) goes through generate_data_param
and then, stage by stage with a device synchronisation after each, through what simulate_data_from_param runs per batch:

  read + decode | upload + DSP (simulate_recipes) | quantise | FLAC encode (frames to the host) | PCM download | MD5 + STREAMINFO | write

and, on the same batches, the WAV path (quantise, PCM download, write .wav).  Prints one line per stage, rows / s end to end for both
formats and the compressed size as a fraction of the PCM.

  python scripts/time_simulate.py [--rows 200] [--nj 8]
  rocprofv3 --kernel-trace --stats -d DIR -- python scripts/time_simulate.py --encoder-only      (kernel time of the encoder, a run of its own)
"""
import argparse
import hashlib
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_corpus(root, rows, seed=0):
    from urgent2026_challenge_track1_amd import audio_io
    from urgent2026_challenge_track1_amd.dataset import SyntheticPairDataset
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "src"), exist_ok=True)
    lines = {"speech": [], "noise": [], "rir": [], "utt2spk": []}
    for i in range(rows):
        fs = (16000, 48000)[i % 2]
        n = int(rng.uniform(4.0, 10.0) * fs)
        path = os.path.join(root, "src", "sp%d.wav" % i)
        audio_io.write_audio(path, SyntheticPairDataset.speech_like(rng, n, fs).astype(np.float32), fs)
        lines["speech"].append("sp%d %d %s" % (i, fs, path))
        lines["utt2spk"].append("sp%d spk%d" % (i, i % 7))
    for fs in (16000, 48000):
        for i in range(12):
            n = int(rng.uniform(3.0, 20.0) * fs)
            path = os.path.join(root, "src", "nz%d_%d.wav" % (fs, i))
            audio_io.write_audio(path, (0.1 * SyntheticPairDataset.speech_like(rng, n, fs) + 0.02 * rng.standard_normal(n)).astype(np.float32), fs)
            lines["noise"].append("nz%d_%d %d %s" % (fs, i, fs, path))
        for i in range(4):
            n = int(0.4 * fs)
            h = rng.standard_normal(n) * np.exp(-np.arange(n) / (0.05 * fs))
            path = os.path.join(root, "src", "rir%d_%d.wav" % (fs, i))
            audio_io.write_audio(path, (0.9 * h / np.abs(h).max()).astype(np.float32), fs, subtype="FLOAT")
            lines["rir"].append("rir%d_%d %d %s" % (fs, i, fs, path))
    paths = {}
    for k, v in lines.items():
        paths[k] = os.path.join(root, k)
        with open(paths[k], "w") as f:
            f.write("\n".join(v) + "\n")
    conf = os.path.join(root, "conf.yaml")
    with open(conf, "w") as f:
        f.write("seed: 0\nreuse_noise: true\nreuse_rir: true\nprob_reverberation: 0.5\nprob_wind_noise: 0.0\n"
                "num_augmentations: {0: 0.4, 1: 0.4, 2: 0.2}\naugmentations:\n"
                "  clipping: {weight: 1.0, clipping_min_quantile: [0.0, 0.1], clipping_max_quantile: [0.9, 1.0]}\n"
                "  packet_loss: {weight: 1.0, packet_duration_ms: 20, max_continuous_packet_loss: 10, packet_loss_rate: [0.05, 0.25]}\n")
    return ["--config", conf, "--speech_scps", paths["speech"], "--speech_utt2spk", paths["utt2spk"], "--noise_scps", paths["noise"],
            "--rir_scps", paths["rir"], "--log_dir", os.path.join(root, "log"), "--output_dir", os.path.join(root, "data")]


def encoder_only(rows):
    """a batch of speech-like PCM through the encoder three times: what `rocprofv3 --kernel-trace --stats` should see"""
    import torch
    from urgent2026_challenge_track1_amd import flac
    from urgent2026_challenge_track1_amd.dataset import SyntheticPairDataset
    rng = np.random.default_rng(1)
    n = 7 * 48000
    x = np.stack([SyntheticPairDataset.speech_like(rng, n, 48000) for _ in range(rows)]).astype(np.float32)
    pcm = flac.quantise_pcm16(torch.as_tensor(x).cuda())
    for _ in range(3):
        t0 = time.perf_counter()
        streams, sizes = flac.encode_flac_frames(pcm, [n] * rows, 48000)
        dt = time.perf_counter() - t0
    frames = sum(len(s) for s in sizes)
    print("encoder only: %d rows x %d samples, %d frames, %.2f ms per call (kernels + size and stream copies), %.3f of the PCM bytes"
          % (rows, n, frames, 1e3 * dt, sum(len(s) for s in streams) / (2.0 * n * rows)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200)
    ap.add_argument("--nj", type=int, default=8)
    ap.add_argument("--encoder-only", action="store_true")
    opt = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    if opt.encoder_only:
        return encoder_only(min(opt.rows, 64))
    from urgent2026_challenge_track1_amd import audio_io, flac, generate_data_param as gdp, simulate_data_from_param as sdp
    root = tempfile.mkdtemp(prefix="time_simulate_")
    argv = make_corpus(root, opt.rows)
    gdp.main(argv)
    args = sdp.get_parser().parse_args(argv + ["--meta_tsv", os.path.join(root, "log", "meta.tsv"), "--highpass", "1"])
    speech_dic, noise_dic, rir_dic = (sdp.read_flat_scps(p) for p in (args.speech_scps, args.noise_scps, args.rir_scps))
    rows = sdp.read_meta(args.log_dir)
    parsed = [sdp.parse_row(r, True) for r in rows]
    stages = ("read + decode", "upload + DSP", "quantise", "encode (frames to host)", "PCM download", "MD5 + STREAMINFO", "write .flac",
              "write .wav")
    spent = dict.fromkeys(stages, 0.0)
    samples = flac_bytes = 0

    def tick(name, t0):
        torch.cuda.synchronize()
        spent[name] += time.perf_counter() - t0
        return time.perf_counter()
    for rep in range(2):             # the first pass warms up (filter designs, allocator, code objects); the second is reported
        for k in spent:
            spent[k] = 0.0
        samples = flac_bytes = 0
        with ThreadPoolExecutor(max_workers=min(16, opt.nj)) as pool:
            for members in sdp.plan_batches(rows, args.chunksize):
                t = time.perf_counter()
                items = list(pool.map(lambda i: sdp.load_item(rows[i], parsed[i][0], speech_dic, noise_dic, rir_dic), members))
                t = tick("read + decode", t)
                clean, noisy, noise, lens = sdp.simulate_items(items, "cuda")
                t = tick("upload + DSP", t)
                fs = items[0]["fs"]
                for kind, sig in (("clean", clean), ("noisy", noisy)):
                    lens_d = torch.as_tensor(lens, dtype=torch.int32).cuda()
                    t = tick("upload + DSP", t)
                    pcm = flac.quantise_pcm16(sig, lens_d)
                    t = tick("quantise", t)
                    streams, sizes = flac.encode_flac_frames(pcm, lens, fs)
                    t = tick("encode (frames to host)", t)
                    host = pcm.cpu().numpy()
                    t = tick("PCM download", t)
                    files = [flac.flac_file(streams[b], sizes[b], fs, lens[b], 4096, hashlib.md5(host[b, :lens[b]].tobytes()).digest())
                             for b in range(len(lens))]
                    t = tick("MD5 + STREAMINFO", t)

                    def put(job):
                        with open(job[0], "wb") as f:
                            f.write(job[1])
                    list(pool.map(put, [(os.path.join(root, "%s_%s.flac" % (kind, rows[i]["id"])), files[b]) for b, i in enumerate(members)]))
                    t = tick("write .flac", t)
                    flt = host.astype(np.float32) / 32768.0
                    list(pool.map(lambda bi: audio_io.write_audio(os.path.join(root, "%s_%s.wav" % (kind, rows[bi[1]]["id"])),
                                                                  flt[bi[0], :lens[bi[0]]], fs), list(enumerate(members))))
                    t = tick("write .wav", t)
                    samples += sum(lens)
                    flac_bytes += sum(len(f) for f in files)
    n = len(rows)
    print("%d rows, %d files, %.1f M samples (second pass)" % (n, 2 * n, samples / 1e6))
    for k in stages:
        print("  %-26s %8.1f ms" % (k, 1e3 * spent[k]))
    common = spent["read + decode"] + spent["upload + DSP"] + spent["quantise"] + spent["PCM download"]
    t_flac = common + spent["encode (frames to host)"] + spent["MD5 + STREAMINFO"] + spent["write .flac"]
    t_wav = common + spent["write .wav"]
    print("FLAC path: %.1f rows / s end to end; WAV path: %.1f rows / s" % (n / t_flac, n / t_wav))
    print("after the shared stages: FLAC %.1f ms (encode + MD5 + write), WAV %.1f ms (write; includes the host's re-quantisation in write_audio)"
          % (1e3 * (t_flac - common), 1e3 * (t_wav - common)))
    print("compressed size: %.3f of the 16-bit PCM" % (flac_bytes / (2.0 * samples)))


if __name__ == "__main__":
    main()
