"""Time of the wind-noise stage (csrc/wind.hip, ``mixing.wind_noise``): rows of 10 s at 48 kHz, one row and 32 rows in one launch (one workgroup
per row: the launch takes as long as its longest row while rows <= CUs).  HIP events around single launches on restored inputs, median of the
repetitions after two warm-up launches; one JSON line at the end.

    timeout 300 python scripts/time_wind.py
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from urgent2026_challenge_track1_amd import mixing  # noqa: E402

FS, SECONDS, REPS = 48000, 10, 7
PAR = dict(threshold=0.2, ratio=7.9, attack=57.5, release=23.6, sc_gain=0.87, clipping_threshold=0.9)


def measure(rows):
    n = FS * SECONDS
    g = torch.Generator(device="cuda").manual_seed(rows)
    x0 = 0.2 * torch.randn(rows, n, device="cuda", generator=g)
    swell = (0.05 + torch.sin(torch.arange(n, device="cuda") * (3.14159 / FS)) ** 2)[None]
    v0 = 0.3 * swell * torch.randn(rows, n, device="cuda", generator=g)
    speech, noise, noisy = x0.clone(), v0.clone(), x0 + v0
    lens = torch.full((rows,), n, dtype=torch.int32, device="cuda")
    times = []
    for i in range(REPS + 2):
        speech.copy_(x0)
        noise.copy_(v0)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        mixing.wind_noise(speech, x0, noise, noisy, lens, list(range(rows)), [PAR] * rows, [i % 2 == 0] * rows, FS)
        b.record()
        torch.cuda.synchronize()
        if i >= 2:
            times.append(a.elapsed_time(b))
    return dict(rows=rows, samples_per_row=n, ms_median=statistics.median(times), ms_min=min(times), ms_max=max(times))


def main():
    out = [measure(r) for r in (1, 32)]
    for o in out:
        print("%2d row(s) x %d samples: %.3f ms (min %.3f, max %.3f), %.1f ns per sample of a row"
              % (o["rows"], o["samples_per_row"], o["ms_median"], o["ms_min"], o["ms_max"], 1e6 * o["ms_median"] / o["samples_per_row"]))
    print(json.dumps({"wind_stage": out}))


if __name__ == "__main__":
    main()
