"""Timing of the mean-power kernel (csrc/bandwidth.hip) at the reference's seven frame sizes: rows = 256 x 4 s per rate, HIP
events around back-to-back launches on preallocated buffers, bytes read / time against the 8 TB/s of HBM.

One comparison is a REQUIREMENT (exit status 1 when it fails): at n_fft 1536 / hop 768 the kernel reads the samples
urse_stft_fwd reads and writes F floats per row where urse_stft_fwd writes T x F complex values, so it must take no longer
than urse_stft_fwd on the same input in the same process - interleaved after warm-up, medians, +10 % for run-to-run spread.

    timeout 300 python scripts/time_bandwidth.py                      # the table + the comparison, one JSON line at the end
    timeout 300 rocprofv3 --kernel-trace --stats -- python scripts/time_bandwidth.py --profile     # one short pass per rate
    URSE_BW_BLUESTEIN_MIN_PRIME=0 timeout 300 python scripts/time_bandwidth.py --no-compare --rates 22050 44100
                                                                      # the odd sizes on the generic butterfly (0 = no Bluestein)
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from urgent2026_challenge_track1_amd import _lib, bandwidth  # noqa: E402
from urgent2026_challenge_track1_amd._lib import call, stream_ptr  # noqa: E402

RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000)
ROWS, SECONDS, HBM_BW = 256, 4, 8e12


class Power:
    """urse_power_spectrum_mean on preallocated buffers"""

    def __init__(self, x, fs):
        self.x, (self.n_fft, self.hop) = x, bandwidth.stft_params(fs)
        self.rows, self.L = x.shape
        nbytes = ctypes.c_int64()
        rc = _lib.load().urse_power_spectrum_workspace_bytes(self.rows, self.L, self.n_fft, self.hop, ctypes.byref(nbytes))
        assert rc == 0, _lib.load().urse_last_error()
        self.nbytes = nbytes.value
        self.ws = torch.empty(self.nbytes // 4, device=x.device)
        self.lens = torch.full((self.rows,), self.L, device=x.device, dtype=torch.int32)
        self.out = torch.empty(self.rows, self.n_fft // 2 + 1, device=x.device)

    def __call__(self):
        call("power_spectrum_mean", self.x, self.L, self.lens, self.out, self.rows, self.L, self.n_fft, self.hop, self.ws,
             self.nbytes, stream_ptr())


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3          # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile", action="store_true", help="three launches per rate and no comparison (for rocprofv3)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rates", type=int, nargs="+", default=list(RATES), help="sampling rates to time (n_fft = int(0.032 fs))")
    ap.add_argument("--no-compare", action="store_true", help="skip the comparison with urse_stft_fwd")
    args = ap.parse_args()
    result = {"device": torch.cuda.get_device_name(0), "rows": ROWS, "seconds": SECONDS, "rates": {},
              "URSE_BW_BLUESTEIN_MIN_PRIME": os.environ.get("URSE_BW_BLUESTEIN_MIN_PRIME")}
    for fs in args.rates:
        x = torch.randn(ROWS, SECONDS * fs, device="cuda")
        p = Power(x, fs)
        for _ in range(3):
            p()
        torch.cuda.synchronize()
        if args.profile:
            continue
        us = statistics.median(timed(p, args.reps) for _ in range(5))
        read = x.numel() * 4
        result["rates"][str(fs)] = {"n_fft": p.n_fft, "hop": p.hop, "us": round(us, 1), "read_GBps": round(read / us / 1e3, 1),
                                    "hbm_fraction": round(read / (us * 1e-6) / HBM_BW, 4), "workspace_MB": round(p.nbytes / 1e6, 1)}
        print("fs %6d  n_fft %4d  hop %3d  %9.1f us  %7.1f GB/s read = %5.2f %% of 8 TB/s" %
              (fs, p.n_fft, p.hop, us, read / us / 1e3, 100 * read / (us * 1e-6) / HBM_BW), flush=True)
        del x, p
    if args.profile:
        return 0
    if args.no_compare:
        print(json.dumps(result))
        return 0
    # the required comparison: same input, same process, interleaved
    fs = 48000
    x = torch.randn(ROWS, SECONDS * fs, device="cuda")
    p = Power(x, fs)
    T, F = x.shape[1] // p.hop + 1, p.n_fft // 2 + 1
    spec = torch.empty(ROWS, T, F, 2, device="cuda")

    def stft():
        call("stft_fwd", x, None, spec, ROWS, x.shape[1], p.n_fft, p.hop, 1, stream_ptr())
    for _ in range(3):
        p()
        stft()
    torch.cuda.synchronize()
    tp, ts = [], []
    for _ in range(10):
        tp.append(timed(p, 5))
        ts.append(timed(stft, 5))
    mp, ms = statistics.median(tp), statistics.median(ts)
    ok = mp <= 1.10 * ms
    result["vs_stft_fwd_1536_768"] = {"power_us": round(mp, 1), "stft_fwd_us": round(ms, 1), "ratio": round(mp / ms, 3),
                                      "power_us_all": [round(v, 1) for v in tp], "stft_fwd_us_all": [round(v, 1) for v in ts],
                                      "allowance": 1.10, "ok": ok}
    print("n_fft 1536 / hop 768, %d x %d: mean power %.1f us, urse_stft_fwd %.1f us (ratio %.3f, must be <= 1.10): %s" %
          (ROWS, x.shape[1], mp, ms, mp / ms, "ok" if ok else "FAILED"))
    print(json.dumps(result))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
