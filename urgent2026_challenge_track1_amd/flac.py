"""FLAC reading through the library's host-side decoder (csrc/flac.hip): ``decode_flac(bytes) -> (float32 [T, ch], fs)`` with
the scaling of ``soundfile.read`` (integers / 2**(bits-1)); and FLAC writing through the device encoder (csrc/flac_enc.hip): ``encode_flac(int16 rows,
lens, fs) -> list[bytes]`` (mono, 16 bit; frames from the device, 'fLaC' + STREAMINFO + MD5 from the host)."""
import ctypes

import numpy as np

from . import _lib


def flac_streaminfo(data, path="<bytes>"):
    lib = _lib.load()
    info = (ctypes.c_int64 * 6)()
    buf = ctypes.create_string_buffer(bytes(data[:1 << 16]), min(len(data), 1 << 16))
    if lib.urse_flac_info(ctypes.addressof(buf), len(buf), ctypes.addressof(info)) != 0:
        raise ValueError("%s: %s" % (path, lib.urse_last_error().decode()))
    return dict(fs=int(info[0]), channels=int(info[1]), bits=int(info[2]), total_samples=int(info[3]), min_block=int(info[4]),
                max_block=int(info[5]))


def decode_flac(data, path="<bytes>"):
    lib = _lib.load()
    si = flac_streaminfo(data, path)
    raw = np.frombuffer(data, dtype=np.uint8)
    cap = si["total_samples"] if si["total_samples"] > 0 else max(1, len(data) * 16 // max(1, si["channels"]))
    out = np.empty((cap, si["channels"]), dtype=np.int32)
    n = ctypes.c_int64()
    rc = lib.urse_flac_decode(raw.ctypes.data, len(raw), out.ctypes.data, cap, ctypes.addressof(n))
    if rc != 0:
        raise ValueError("%s: %s" % (path, lib.urse_last_error().decode()))
    x = out[:n.value].astype(np.float32) / np.float32(1 << (si["bits"] - 1))
    return x, si["fs"]


# ---- encoding: the frames come from the device (csrc/flac_enc.hip), 'fLaC' + STREAMINFO from here -------------------------------
FLAC_RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000)
FLAC_BLOCKSIZES = (256, 512, 1024, 2048, 4096)


def flac_file(frames, frame_sizes, fs, total_samples, blocksize, pcm_md5):
    """A complete mono 16-bit FLAC file: 'fLaC', one STREAMINFO block (min = max block size = the stream's fixed block size, min / max
    frame size from ``frame_sizes``, the rate, total samples and the 16-byte MD5 of the little-endian PCM), then ``frames``."""
    frames = bytes(frames)
    sizes = [int(s) for s in frame_sizes]
    if sum(sizes) != len(frames):
        raise ValueError("frame sizes add up to %d bytes, the stream has %d" % (sum(sizes), len(frames)))
    if len(pcm_md5) != 16:
        raise ValueError("the MD5 signature has 16 bytes")
    if not (0 < fs < 1 << 20 and 0 <= total_samples < 1 << 36 and 16 <= blocksize <= 65535):
        raise ValueError("STREAMINFO cannot hold fs=%d, total=%d, blocksize=%d" % (fs, total_samples, blocksize))
    lo, hi = (min(sizes), max(sizes)) if sizes else (0, 0)
    packed = (fs << 44) | (0 << 41) | (15 << 36) | total_samples          # rate (20), channels - 1 (3), bits - 1 (5), samples (36)
    info = (blocksize.to_bytes(2, "big") * 2 + lo.to_bytes(3, "big") + hi.to_bytes(3, "big") + packed.to_bytes(8, "big")
            + bytes(pcm_md5))
    return b"fLaC" + bytes([0x80, 0, 0, len(info)]) + info + frames


def quantise_pcm16(x, lens=None, scale=32768.0):
    """f32 device rows [P, T] -> int16 device rows [P, T] by the 16-bit WAV writer's rule (``clip(round(x * 32768))``), zeros behind
    ``lens`` (int32 device tensor [P])."""
    import torch
    _lib.require_cuda(x, lens)
    if x.dim() != 2 or x.dtype != torch.float32 or x.shape[1] == 0:
        raise _lib.UrseError("quantise_pcm16 takes non-empty f32 rows [P, T]")
    x = x.contiguous()
    if lens is not None:
        lens = lens.to(torch.int32).contiguous()
    pcm = torch.empty(x.shape, dtype=torch.int16, device=x.device)
    _lib.call("pcm16_from_f32", x, x.shape[1], lens, pcm, x.shape[1], x.shape[0], x.shape[1], float(scale), _lib.stream_ptr())
    return pcm


def encode_flac_frames(pcm_rows, lens, fs, blocksize=4096, channels=1, bits=16, out_capacity=None):
    """The device encoder on int16 device rows [P, T] -> (list of P frame streams (bytes), list of P int32 arrays of frame sizes)."""
    import torch
    _lib.require_cuda(pcm_rows)
    if pcm_rows.dim() != 2 or pcm_rows.dtype != torch.int16:
        raise _lib.UrseError("encode_flac takes int16 rows [P, T]")
    pcm_rows = pcm_rows.contiguous()
    P, ld = pcm_rows.shape
    lens_h = np.ascontiguousarray(np.asarray(lens, dtype=np.int64).reshape(-1))
    if lens_h.shape[0] != P or (lens_h < 0).any() or (lens_h > ld).any():
        raise _lib.UrseError("encode_flac: %d lengths for %d rows of %d samples" % (lens_h.shape[0], P, ld))
    rates_h = np.ascontiguousarray(np.broadcast_to(np.asarray(fs, dtype=np.int32).reshape(-1), (P,)))
    lens_h = lens_h.astype(np.int32)
    starts_h = np.arange(P, dtype=np.int64) * ld
    lib = _lib.load()

    def check(rc, name):
        if rc != 0:
            raise _lib.UrseError("urse_%s failed (%d): %s" % (name, rc, lib.urse_last_error().decode()))

    info = np.zeros(3, dtype=np.int64)
    check(lib.urse_flac_encode_workspace_bytes(lens_h.ctypes.data, P, blocksize, info.ctypes.data), "flac_encode_workspace_bytes")
    workspace = torch.empty(int(info[0]), dtype=torch.uint8, device=pcm_rows.device)
    out = np.zeros(max(1, int(info[2]) if out_capacity is None else int(out_capacity)), dtype=np.uint8)
    file_bytes = np.zeros(P, dtype=np.int64)
    frame_bytes = np.zeros(max(1, int(info[1])), dtype=np.int32)
    check(lib.urse_flac_encode(pcm_rows.data_ptr(), P * ld, starts_h.ctypes.data, lens_h.ctypes.data, rates_h.ctypes.data, P,
                               channels, bits, blocksize, workspace.data_ptr(), workspace.numel(), out.ctypes.data,
                               out.size if out_capacity is None else int(out_capacity), file_bytes.ctypes.data,
                               frame_bytes.ctypes.data, _lib.stream_ptr()), "flac_encode")
    streams, sizes, pos, f = [], [], 0, 0
    for p in range(P):
        nf = -(-int(lens_h[p]) // blocksize)
        streams.append(out[pos:pos + int(file_bytes[p])].tobytes())
        sizes.append(frame_bytes[f:f + nf].copy())
        pos += int(file_bytes[p])
        f += nf
    return streams, sizes


def encode_flac(pcm_rows, lens, fs, blocksize=4096):
    """int16 rows [P, T] (device tensor; a host array is uploaded), ``lens`` [P], ``fs`` (one rate or one per row) -> list of P complete
    FLAC files (bytes).  The frames are encoded on the device in one call; the PCM also comes to the host, for STREAMINFO's MD5."""
    import hashlib
    import torch
    if not isinstance(pcm_rows, torch.Tensor):
        pcm_rows = torch.as_tensor(np.ascontiguousarray(np.asarray(pcm_rows, dtype=np.int16))).cuda()
    if pcm_rows.dim() == 1:
        pcm_rows = pcm_rows[None]
    streams, sizes = encode_flac_frames(pcm_rows, lens, fs, blocksize)
    host = pcm_rows.cpu().numpy()
    rates = np.broadcast_to(np.asarray(fs, dtype=np.int64).reshape(-1), (len(streams),))
    lens = np.asarray(lens, dtype=np.int64).reshape(-1)
    return [flac_file(streams[p], sizes[p], int(rates[p]), int(lens[p]), blocksize,
                      hashlib.md5(host[p, :lens[p]].astype("<i2").tobytes()).digest()) for p in range(len(streams))]
