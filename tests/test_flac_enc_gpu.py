"""GPU: the device FLAC encoder (csrc/flac_enc.hip) and the 16-bit quantiser in front of it.

a. lossless: the library's own decoder returns the input samples, rate and length;
b. framing, checked here in Python without the decoder: sync, block-size / rate codes, frame number, CRC-8, CRC-16, STREAMINFO;
c. size, as conditions derived from the format: no frame above its VERBATIM size; speech-like and zero frames no larger than header +
   footer + the cost of the best FIXED order with ONE Rice parameter, which a numpy model computes here; zero / constant frames are
   CONSTANT subframes;
d. a file's bytes do not depend on the batch or the run;
e. what the encoder does not do is refused before anything is written;
f. the quantiser equals numpy."""
import ctypes
import hashlib

import numpy as np
import pytest

from tests.flac_writer import crc8, crc16, utf8_number

pytestmark = pytest.mark.gpu

RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000)
RATE_CODE = {8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10}
BS_CODE = {256: 8, 512: 9, 1024: 10, 2048: 11, 4096: 12}

_T16 = []
for _b in range(256):
    _c = _b << 8
    for _ in range(8):
        _c = ((_c << 1) ^ 0x8005) & 0xFFFF if _c & 0x8000 else (_c << 1) & 0xFFFF
    _T16.append(_c)


def fast_crc16(data):
    c = 0
    for b in data:
        c = ((c << 8) & 0xFFFF) ^ _T16[(c >> 8) ^ b]
    return c


def speech_like(n, seed, gap=None):
    """a few harmonics under a slow envelope plus a little noise, int16; ``gap`` = (start, stop) of a run of zeros (a lost packet)"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    env = 0.5 * (1.0 + np.sin(2 * np.pi * 3.1 * t + rng.uniform(0, 6)))
    x = sum(a * np.sin(2 * np.pi * f0 * t + rng.uniform(0, 6)) for a, f0 in ((0.2, 140.0), (0.12, 280.0), (0.07, 425.0), (0.03, 1210.0)))
    x = env * x + 0.002 * rng.standard_normal(n)
    if gap:
        x[gap[0]:gap[1]] = 0.0
    return np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)


def encode(files, rates, blocksize):
    """list of int16 arrays -> (FLAC files, frame streams, frame sizes) from ONE encoder call"""
    import torch
    from urgent2026_challenge_track1_amd import flac
    ld = max(len(f) for f in files)
    rows = np.zeros((len(files), ld), dtype=np.int16)
    for i, f in enumerate(files):
        rows[i, :len(f)] = f
    lens = [len(f) for f in files]
    dev = torch.as_tensor(rows).cuda()
    streams, sizes = flac.encode_flac_frames(dev, lens, rates, blocksize)
    whole = flac.encode_flac(dev, lens, rates, blocksize)
    return whole, streams, sizes


def model_fixed_bits(x):
    """bits of the cheapest FIXED subframe with partition order 0 (subframe header included), by the format's own arithmetic"""
    x = x.astype(np.int64)
    n, best = len(x), None
    for o in range(0, min(4, n - 1) + 1):
        r = np.diff(x, o)[0:] if o else x
        assert len(r) == n - o
        u = np.where(r >= 0, 2 * r, -2 * r - 1)
        cost = min((n - o) * (k + 1) + int((u >> k).sum()) for k in range(15))
        bits = 8 + 16 * o + 2 + 4 + 4 + cost
        best = bits if best is None else min(best, bits)
    return best


def walk(whole, stream, sizes, x, fs, blocksize, model=False, expect_type=None):
    """assertion b and c on one file"""
    n_total = len(x)
    assert whole[:4] == b"fLaC" and whole[4] == 0x80 and whole[5:8] == bytes([0, 0, 34]) and whole[42:] == stream
    si = whole[8:42]
    assert int.from_bytes(si[0:2], "big") == blocksize and int.from_bytes(si[2:4], "big") == blocksize
    assert int.from_bytes(si[4:7], "big") == min(sizes) and int.from_bytes(si[7:10], "big") == max(sizes)
    packed = int.from_bytes(si[10:18], "big")
    assert packed >> 44 == fs and (packed >> 41) & 7 == 0 and (packed >> 36) & 31 == 15 and packed & ((1 << 36) - 1) == n_total
    assert si[18:34] == hashlib.md5(x.astype("<i2").tobytes()).digest()
    assert len(sizes) == -(-n_total // blocksize) and int(sizes.sum()) == len(stream)
    pos = 0
    for fno, size in enumerate(sizes):
        fr = stream[pos:pos + size]
        pos += size
        n = min(blocksize, n_total - fno * blocksize)
        assert fr[0] == 0xFF and fr[1] == 0xF8, fno
        bs_code = BS_CODE[blocksize] if n == blocksize else 6 if n <= 256 else 7
        assert fr[2] == (bs_code << 4 | RATE_CODE[fs]), (fno, hex(fr[2]))
        assert fr[3] == 0x08
        num = utf8_number(fno)
        assert fr[4:4 + len(num)] == num, fno
        h = 4 + len(num)
        if bs_code == 6:
            assert fr[h] == n - 1
            h += 1
        elif bs_code == 7:
            assert int.from_bytes(fr[h:h + 2], "big") == n - 1
            h += 2
        assert fr[h] == crc8(fr[:h]), fno
        h += 1
        assert int.from_bytes(fr[-2:], "big") == fast_crc16(fr[:-2]), fno
        assert size <= h + 1 + 2 * n + 2, (fno, size)                       # never above VERBATIM
        if expect_type is not None:
            assert fr[h] == expect_type, (fno, fr[h])
        if model:
            bound = h + -(-model_fixed_bits(x[fno * blocksize:fno * blocksize + n]) // 8) + 2
            assert size <= bound, (fno, size, bound)


def check_lossless(whole, x, fs):
    from urgent2026_challenge_track1_amd import flac
    y, rate = flac.decode_flac(whole)
    assert rate == fs and y.shape == (len(x), 1)
    assert np.array_equal(np.round(y[:, 0] * 32768.0).astype(np.int64), x.astype(np.int64))


def test_table_crc_is_the_format_crc():
    data = bytes(np.random.default_rng(0).integers(0, 256, 300, dtype=np.uint8))
    assert fast_crc16(data) == crc16(data)


@pytest.mark.parametrize("blocksize", [4096, 256])
def test_every_length_round_trips_and_frames_are_well_formed(lib, blocksize):
    lengths = [1, 5, 255, 256, 257, 4095, 4096, 4097, 10000]
    files = [speech_like(n, 100 + n) for n in lengths]
    rates = [RATES[i % 7] for i in range(len(files))]
    whole, streams, sizes = encode(files, rates, blocksize)
    for w, s, z, x, fs in zip(whole, streams, sizes, files, rates):
        check_lossless(w, x, fs)
        walk(w, s, z, x, fs, blocksize, model=True)


@pytest.mark.parametrize("blocksize", [4096, 256])
def test_signals_at_the_edges_of_the_format(lib, blocksize):
    n = 10000
    rng = np.random.default_rng(7)
    zeros = np.zeros(n, dtype=np.int16)
    floor = np.full(n, -32768, dtype=np.int16)
    alt = np.where(np.arange(n) % 2 == 0, 32767, -32768).astype(np.int16)
    white = rng.integers(-32768, 32768, n).astype(np.int16)
    lost = speech_like(n, 3, gap=(4000, 4700))
    files = [zeros, floor, alt, white, lost]
    whole, streams, sizes = encode(files, [16000] * 5, blocksize)
    for w, x in zip(whole, files):
        check_lossless(w, x, 16000)
    walk(whole[0], streams[0], sizes[0], zeros, 16000, blocksize, model=True, expect_type=0x00)      # CONSTANT
    walk(whole[1], streams[1], sizes[1], floor, 16000, blocksize, expect_type=0x00)
    walk(whole[2], streams[2], sizes[2], alt, 16000, blocksize)
    walk(whole[3], streams[3], sizes[3], white, 16000, blocksize)
    walk(whole[4], streams[4], sizes[4], lost, 16000, blocksize, model=True)
    # the lost packet costs (almost) nothing: at block size 256 its inner frames are CONSTANT
    if blocksize == 256:
        small = [int(s) for i, s in enumerate(sizes[4]) if 4000 <= i * 256 and (i + 1) * 256 <= 4700]
        assert small and max(small) <= 4 + 1 + 1 + 1 + 2 + 2
    # full-scale noise does not compress, and must not grow: VERBATIM is the ceiling
    assert len(streams[3]) <= 2 * n + len(sizes[3]) * 12


def test_frame_numbers_beyond_one_and_two_utf8_bytes(lib):
    x = speech_like(600000, 11, gap=(300000, 301000))
    (whole,), (stream,), (sizes,) = encode([x], [48000], 256)
    assert len(sizes) == 2344
    check_lossless(whole, x, 48000)
    walk(whole, stream, sizes, x, 48000, 256)


def test_a_file_does_not_depend_on_its_batch_or_the_run(lib):
    lengths = [1, 300, 4096, 5000, 10000, 777, 12345]
    files = [speech_like(n, 40 + i, gap=(100, 180) if n > 200 else None) for i, n in enumerate(lengths)]
    rates = list(RATES)
    for blocksize in (4096, 1024):
        whole, streams, sizes = encode(files, rates, blocksize)
        again, _, _ = encode(files, rates, blocksize)
        assert whole == again
        for w, s, z, x, fs in zip(whole, streams, sizes, files, rates):
            check_lossless(w, x, fs)
            walk(w, s, z, x, fs, blocksize)
        for i in (0, 3, 6):
            (alone,), _, _ = encode([files[i]], [rates[i]], blocksize)
            assert alone == whole[i], i


def _raw_encode(lib, pcm, lens, rates, channels, bits, blocksize, capacity):
    import torch
    from urgent2026_challenge_track1_amd import _lib
    P = len(lens)
    lens_h, rates_h = np.asarray(lens, dtype=np.int32), np.asarray(rates, dtype=np.int32)
    starts_h = np.arange(P, dtype=np.int64) * pcm.shape[1]
    info = np.zeros(3, dtype=np.int64)
    rc = lib.urse_flac_encode_workspace_bytes(lens_h.ctypes.data, P, blocksize, info.ctypes.data)
    ws = torch.empty(max(1, int(info[0])) if rc == 0 else 1 << 20, dtype=torch.uint8, device="cuda")
    out = np.full(max(1, capacity), 0xAB, dtype=np.uint8)
    file_bytes = np.full(P, -7, dtype=np.int64)
    frame_bytes = np.zeros(1024, dtype=np.int32)
    rc2 = lib.urse_flac_encode(pcm.data_ptr(), pcm.numel(), starts_h.ctypes.data, lens_h.ctypes.data, rates_h.ctypes.data, P, channels,
                               bits, blocksize, ws.data_ptr(), ws.numel(), out.ctypes.data, capacity, file_bytes.ctypes.data,
                               frame_bytes.ctypes.data, _lib.stream_ptr())
    return rc, rc2, out, file_bytes


def test_what_the_encoder_does_not_do_is_refused(lib):
    import torch
    x = speech_like(5000, 5)
    pcm = torch.as_tensor(x[None].copy()).cuda()
    ok = _raw_encode(lib, pcm, [5000], [16000], 1, 16, 4096, 1 << 16)
    assert ok[0] == 0 and ok[1] == 0 and ok[3][0] > 0 and ok[2][0] == 0xFF
    for channels, bits, blocksize, rate in ((2, 16, 4096, 16000), (1, 24, 4096, 16000), (1, 16, 1000, 16000), (1, 16, 4096, 11025)):
        rc, rc2, out, file_bytes = _raw_encode(lib, pcm, [5000], [rate], channels, bits, blocksize, 1 << 16)
        assert rc2 == -3, (channels, bits, blocksize, rate, rc2)                       # URSE_ERR_UNSUPPORTED
        assert rc == (-3 if blocksize == 1000 else 0)
        assert (out == 0xAB).all() and file_bytes[0] == -7
    rc, rc2, out, file_bytes = _raw_encode(lib, pcm, [5000], [16000], 1, 16, 4096, int(ok[3][0]) - 1)      # one byte short
    assert rc2 == -1 and b"output buffer" in lib.urse_last_error()
    assert (out == 0xAB).all() and file_bytes[0] == 0
    rc, rc2, out, file_bytes = _raw_encode(lib, pcm, [5001], [16000], 1, 16, 4096, 1 << 16)                # reads past the samples given
    assert rc2 == -1 and (out == 0xAB).all()


def test_quantiser_equals_numpy(lib):
    import torch
    from urgent2026_challenge_track1_amd import flac
    rng = np.random.default_rng(2)
    x = (0.5 * rng.standard_normal((5, 1237))).astype(np.float32)
    x[0, :8] = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 3.5, -2.5, 0.0], dtype=np.float32) / 32768.0      # ties go to even
    x[1, :6] = [1.0, -1.0, 1.5, -1.5, 32767.4 / 32768.0, -32768.6 / 32768.0]
    lens = np.array([1237, 1000, 1, 640, 1236], dtype=np.int32)
    want = np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)
    for i, n in enumerate(lens):
        want[i, n:] = 0
    got = flac.quantise_pcm16(torch.as_tensor(x).cuda(), torch.as_tensor(lens).cuda()).cpu().numpy()
    assert got.dtype == np.int16 and np.array_equal(got, want)
    full = flac.quantise_pcm16(torch.as_tensor(x).cuda()).cpu().numpy()
    assert np.array_equal(full, np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16))


def test_write_flac_and_write_audio_hold_the_same_samples(lib, tmp_path):
    from urgent2026_challenge_track1_amd import audio_io
    x = (speech_like(9001, 9).astype(np.float32) / 32768.0) * 1.7 + 1e-5          # clips at both ends, off the integer grid
    audio_io.write_audio(str(tmp_path / "a.wav"), x, 24000)
    audio_io.write_flac(str(tmp_path / "a.flac"), x, 24000)
    w, fw = audio_io.read_audio(str(tmp_path / "a.wav"))
    f, ff = audio_io.read_audio(str(tmp_path / "a.flac"))
    assert fw == ff == 24000 and np.array_equal(w, f)
    assert audio_io.audio_frames(str(tmp_path / "a.flac")) == 9001
