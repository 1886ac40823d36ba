"""Audio bandwidth estimation on the device: what ``utils/estimate_audio_bandwidth.py:11-49`` of the reference computes
per file with ``torch.stft`` on the CPU, for a batch of rows at one sampling rate in two launches
(``urse_power_spectrum_mean`` + ``urse_bandwidth_pick``, csrc/bandwidth.hip), and the rate rule of
``utils/resample_to_estimated_bandwidth.py:49-54``.
"""
import numpy as np
import torch

from ._lib import UrseError, call, load, require_cuda, stream_ptr

SAMPLING_RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000)   # resample_to_estimated_bandwidth.py:12


def stft_params(fs, nfft=512, hop=256, sample_rate=16000):
    """(n_fft, hop) of estimate_audio_bandwidth.py:34-35: ``int(nfft / sample_rate * fs)``, the same float expression (it
    truncates: 705 at 22.05 kHz, 1411 at 44.1 kHz)."""
    return int(nfft / sample_rate * fs), int(hop / sample_rate * fs)


def bin_frequency(i, n_fft, fs):
    """``torch.fft.rfftfreq(n_fft, d=1 / fs)[i].item()`` (:40, :49) without the transform library: a float32 ramp times the
    float32 rounding of the double ``1 / (n_fft * (1 / fs))``, widened to double.  At 22.05 / 44.1 kHz this is not
    ``i * fs / n_fft`` in double (for example 10782.7783203125), and the reference stores the float32 value as it is."""
    scale = np.float32(1.0 / (n_fft * (1 / fs)))
    return float(np.float32(i) * scale)


def pick_rate(bandwidth):
    """resample_to_estimated_bandwidth.py:49-54: the first challenge rate with ``2 * bandwidth <= sr``, else 48000."""
    for sr in SAMPLING_RATES:
        if bandwidth * 2 <= sr:
            return sr
    return SAMPLING_RATES[-1]


def _host_lens(lens):
    if isinstance(lens, torch.Tensor):
        lens = lens.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(lens, dtype=np.int64).reshape(-1))


def mean_power_spectrum(wav, lens, fs):
    """wav f32 [rows, ld] (cuda; every channel of every file is a row), lens [rows] (host sequence or tensor) -> f32
    [rows, n_fft // 2 + 1]: the mean over each row's frames (``1 + len // hop`` of them for an even n_fft, ``1 + (len - 1) // hop``
    for an odd one: torch.stft pads ``n_fft // 2`` on both sides) of ``|torch.stft|^2`` at the reference's frame
    sizes for ``fs`` (centred, reflect padding at the row's own length, periodic Hann).  Raises UrseError for a frame size
    the kernel does not run and for a row that torch.stft refuses (``len <= n_fft // 2``)."""
    require_cuda(wav)
    assert wav.dim() == 2
    wav = wav.contiguous().float()
    rows, ld = wav.shape
    n_fft, hop = stft_params(fs)
    hl = _host_lens(lens)
    if hl.size != rows:
        raise UrseError("mean_power_spectrum: %d lengths for %d rows" % (hl.size, rows))
    if n_fft < 2 or hop < 1:
        raise UrseError("mean_power_spectrum: fs=%s gives n_fft=%d, hop=%d" % (fs, n_fft, hop))
    if hl.max() > ld:
        raise UrseError("mean_power_spectrum: a length (%d) exceeds the row pitch %d" % (hl.max(), ld))
    if hl.min() <= n_fft // 2:
        raise UrseError("mean_power_spectrum: a row of %d samples cannot be reflect-padded by n_fft // 2 = %d"
                        % (hl.min(), n_fft // 2))
    max_len = int(hl.max())
    lib = load()
    import ctypes
    nbytes = ctypes.c_int64()
    rc = lib.urse_power_spectrum_workspace_bytes(rows, max_len, n_fft, hop, ctypes.byref(nbytes))
    if rc != 0:
        raise UrseError("urse_power_spectrum_workspace_bytes failed (%d): %s" % (rc, lib.urse_last_error().decode()))
    ws = torch.empty(nbytes.value // 4, device=wav.device, dtype=torch.float32)
    lens_d = torch.from_numpy(hl.astype(np.int32)).to(wav.device)
    out = torch.empty(rows, n_fft // 2 + 1, device=wav.device, dtype=torch.float32)
    call("power_spectrum_mean", wav, ld, lens_d, out, rows, max_len, n_fft, hop, ws, nbytes.value, stream_ptr())
    return out


def pick_bins(mean_power, row_start, threshold=-50.0):
    """estimate_audio_bandwidth.py:45-49 on the device: mean_power f32 [rows, F], row_start [P + 1] -> int32 [P] (cuda), -1
    where no bin lies above ``min_c peak[c] * 10 ** (threshold / 10)``."""
    require_cuda(mean_power)
    rs = np.ascontiguousarray(np.asarray(row_start, dtype=np.int32).reshape(-1))
    P = rs.size - 1
    if P < 1 or rs[0] != 0 or rs[-1] != mean_power.shape[0] or np.any(np.diff(rs) < 0):
        raise UrseError("pick_bins: row_start must rise from 0 to the number of rows")
    rs_d = torch.from_numpy(rs).to(mean_power.device)
    bins = torch.empty(P, device=mean_power.device, dtype=torch.int32)
    call("bandwidth_pick", mean_power.contiguous(), rs_d, bins, P, mean_power.shape[1], float(threshold), stream_ptr())
    return bins


def estimate_bandwidth_batch(wav, lens, row_start, fs, threshold=-50.0):
    """The reference's estimate for P files at one rate: file p owns rows ``row_start[p]:row_start[p + 1]`` (its channels).
    -> (bins int list [P], bandwidths list [P]: ``bin_frequency`` of the bin, None where the reference returns nothing)."""
    mp = mean_power_spectrum(wav, lens, fs)
    bins = pick_bins(mp, row_start, threshold).cpu().tolist()
    n_fft, _ = stft_params(fs)
    return bins, [bin_frequency(b, n_fft, fs) if b >= 0 else None for b in bins]
