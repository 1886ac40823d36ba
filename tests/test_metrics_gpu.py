"""GPU parity: batched ESTOI / SDR vs the CPU oracle (oracle/metrics_ref.py); tolerance 1e-4 (north_star)."""
import numpy as np
import pytest
import torch

from oracle import metrics_ref
from tests import metrics_cases as mc

pytestmark = pytest.mark.gpu


def _pairs(P, L, fs, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(L) / fs
    refs, infs = [], []
    for p in range(P):
        c = np.convolve(rng.standard_normal(L), [1, 0.9, 0.5, 0.2], "same") * (0.55 + 0.45 * np.sin(2 * np.pi * 4 * t + p))
        c[: int(0.1 * L)] *= 1e-3
        c[-int(0.08 * L):] *= 1e-3
        c *= 0.9 / np.abs(c).max()
        snr = rng.uniform(0, 25)
        n = rng.standard_normal(L)
        n *= np.sqrt((c ** 2).mean() / ((n ** 2).mean() * 10 ** (snr / 10)))
        refs.append(c.astype(np.float32))
        infs.append((c + n).astype(np.float32))
    return np.stack(refs), np.stack(infs)


@pytest.mark.parametrize("fs,L", [(16000, 32000), (48000, 60000), (10000, 20000), (8000, 12345),
                                  (22050, 33092), (24000, 36017), (32000, 48017), (44100, 66167)])
def test_estoi_matches_oracle(lib, fs, L):
    from urgent2026_challenge_track1_amd import metrics
    ref, inf = _pairs(4, L, fs, fs + L)
    got = metrics.estoi_batch(torch.from_numpy(ref).cuda(), torch.from_numpy(inf).cuda(), fs).cpu().numpy()
    exp = np.array([metrics_ref.estoi(ref[p], inf[p], fs) for p in range(4)])
    assert np.abs(got - exp).max() <= 1e-4, (got, exp)
    assert abs(metrics.estoi_metric(ref[0], inf[0], fs) - exp[0]) <= 1e-4


def test_estoi_edge_cases(lib):
    from urgent2026_challenge_track1_amd import metrics
    ref, inf = _pairs(2, 3000, 16000, 1)              # too short: < 30 frames -> 1e-5 (pystoi warning branch)
    got = metrics.estoi_batch(torch.from_numpy(ref).cuda(), torch.from_numpy(inf).cuda(), 16000).cpu().numpy()
    assert np.allclose(got, 1e-5)
    ref, _ = _pairs(2, 32000, 16000, 2)               # identical signals -> 1
    r = torch.from_numpy(ref).cuda()
    assert np.abs(metrics.estoi_batch(r, r.clone(), 16000).cpu().numpy() - 1.0).max() <= 1e-5


def test_resampler_matches_scipy(lib):
    from urgent2026_challenge_track1_amd import metrics
    ref, _ = _pairs(2, 48000, 48000, 3)
    got = metrics.resample_to_10k(torch.from_numpy(ref).cuda(), 48000).cpu().numpy()
    exp = np.stack([metrics_ref.resample_oct(ref[p].astype(np.float64), 10000, 48000) for p in range(2)])
    assert got.shape == exp.shape and np.abs(got - exp).max() <= 2e-6


@pytest.mark.parametrize("L", [16000, 64000, 5000])
def test_sdr_matches_oracle(lib, L):
    from urgent2026_challenge_track1_amd import metrics
    ref, inf = _pairs(3, L, 16000, L)
    got = metrics.sdr_batch(torch.from_numpy(ref).cuda(), torch.from_numpy(inf).cuda()).cpu().numpy()
    exp = np.array([metrics_ref.sdr(ref[p], inf[p]) for p in range(3)])
    assert np.abs(got - exp).max() <= 1e-4, (got, exp)
    # a filtered + delayed copy is (almost) perfectly explained by the 512-tap filter -> clamp at 50 dB
    d = np.zeros_like(ref)
    d[:, 7:] = 0.5 * ref[:, :-7]
    got = metrics.sdr_batch(torch.from_numpy(ref).cuda(), torch.from_numpy(d).cuda()).cpu().numpy()
    exp = np.array([metrics_ref.sdr(ref[p], d[p]) for p in range(3)])
    assert np.abs(got - exp).max() <= 1e-3 and np.all(got > 45)


def test_metrics_driver_files(lib, tmp_path):
    """scp in -> PESQ.scp + ESTOI.scp + RESULTS.txt out, same formats and METRICS = ("PESQ", "ESTOI") as the reference script;
    two ranks splitting the pairs i % world write the same files as one."""
    from oracle import pesq_ref
    from urgent2026_challenge_track1_amd import calculate_intrusive_se_metrics as drv
    from urgent2026_challenge_track1_amd.dataset import write_audio
    ref, inf = _pairs(3, 20000, 16000, 9)
    with open(tmp_path / "ref.scp", "w") as fr, open(tmp_path / "inf.scp", "w") as fi:
        for p in range(3):
            write_audio(str(tmp_path / ("r%d.wav" % p)), ref[p], 16000, "FLOAT")
            write_audio(str(tmp_path / ("i%d.wav" % p)), inf[p], 16000, "FLOAT")
            fr.write("utt%d %s\n" % (p, tmp_path / ("r%d.wav" % p)))
            fi.write("utt%d %s\n" % (p, tmp_path / ("i%d.wav" % p)))
    base = ["--ref_scp", str(tmp_path / "ref.scp"), "--inf_scp", str(tmp_path / "inf.scp")]
    drv.main(drv.parser().parse_args(base + ["--output_dir", str(tmp_path / "out")]))
    lines = (tmp_path / "out" / "ESTOI.scp").read_text().strip().split("\n")
    assert [l.split()[0] for l in lines] == ["utt0", "utt1", "utt2"]
    exp = [metrics_ref.estoi(ref[p], inf[p], 16000) for p in range(3)]
    assert max(abs(float(l.split()[1]) - e) for l, e in zip(lines, exp)) <= 1e-4
    plines = (tmp_path / "out" / "PESQ.scp").read_text().strip().split("\n")
    pexp = [pesq_ref.pesq(16000, ref[p], inf[p], "wb") for p in range(3)]
    assert max(abs(float(l.split()[1]) - e) for l, e in zip(plines, pexp)) <= 2e-3
    res = (tmp_path / "out" / "RESULTS.txt").read_text().split("\n")
    assert res[0].startswith("PESQ: ") and abs(float(res[0].split()[1]) - np.mean(pexp)) <= 2e-3
    assert res[1] == "ESTOI: %.4f" % np.mean(exp)
    # the same pairs split over two processes (rank 1 first, rank 0 merges)
    for rank in (1, 0):
        drv.main(drv.parser().parse_args(base + ["--output_dir", str(tmp_path / "out2"), "--rank", str(rank), "--world", "2",
                                                 "--metrics", "PESQ", "ESTOI", "SDR"]))
    for m in ("PESQ", "ESTOI"):
        assert (tmp_path / "out2" / ("%s.scp" % m)).read_text() == (tmp_path / "out" / ("%s.scp" % m)).read_text()
    assert "SDR: " in (tmp_path / "out2" / "RESULTS.txt").read_text()


@pytest.mark.parametrize("fs_in,fs_out", [(48000, 16000), (44100, 16000), (32000, 16000), (22050, 16000)])
def test_soxr_hq_spec_resampler_matches_oracle(lib, fs_in, fs_out):
    """the stand-in for soxr.resample(x, fs, 16000) in pesq_metric (calculate_intrusive_se_metrics.py:69-70): a filter built to
    libsoxr's HQ specification (oracle/metrics_ref.soxr_hq_design, its specification asserted in tests/test_oracle.py), evaluated
    by the polyphase kernel with f64 accumulation -> equal to the f64 oracle to f32 rounding."""
    from urgent2026_challenge_track1_amd import metrics
    rng = np.random.default_rng(4)
    x = rng.standard_normal((2, 30011)).astype(np.float32)
    got = metrics.resample_soxr_hq(torch.from_numpy(x).cuda(), fs_in, fs_out).cpu().numpy()
    for p in range(2):
        exp = metrics_ref.resample_soxr_hq_spec(x[p], fs_in, fs_out)
        assert got[p].shape == exp.shape and np.abs(got[p] - exp).max() <= 2e-6 * np.abs(exp).max()


def test_estoi_frame_range_at_the_boundary_length(lib):
    """pystoi frames with ``range(0, len - 256, 128)``: at len = 256 + 128 k exactly the last full frame is NOT taken.
    Fixture: 10 kHz signals (no resampling in front) of 256 + 128 * 200 samples whose last frame is loud speech.  The kernels
    follow the pystoi reading to 1e-4 and differ from the inclusive reading by what that one frame is worth."""
    from urgent2026_challenge_track1_amd import metrics
    L = 256 + 128 * 200
    ref, inf = _pairs(3, L, 10000, 31)
    ref[:, -int(0.08 * L):] = ref[:, int(0.3 * L):int(0.3 * L) + int(0.08 * L)]       # loud to the very end: the last frame counts
    inf[:, -int(0.08 * L):] = inf[:, int(0.3 * L):int(0.3 * L) + int(0.08 * L)]
    got = metrics.estoi_batch(torch.from_numpy(ref).cuda(), torch.from_numpy(inf).cuda(), 10000).cpu().numpy()
    a = np.array([metrics_ref.estoi(ref[p], inf[p], 10000) for p in range(3)])
    metrics_ref.LAST_FRAME_INCLUSIVE = True
    try:
        b = np.array([metrics_ref.estoi(ref[p], inf[p], 10000) for p in range(3)])
    finally:
        metrics_ref.LAST_FRAME_INCLUSIVE = False
    assert np.abs(got - a).max() <= 1e-4, (got, a)
    assert np.abs(a - b).max() > 1e-6                      # the two readings are distinguishable on this fixture
    assert np.abs(got - a).max() < 0.2 * np.abs(a - b).max()
    print("ESTOI at len = 256 mod 128: kernels vs pystoi reading %.1e; pystoi vs inclusive reading %.1e" % (np.abs(got - a).max(), np.abs(a - b).max()))


def test_score_batch_on_two_streams_equals_the_separate_calls(lib):
    """metrics.score_batch runs PESQ on the caller's stream and ESTOI / SDR beside it on a second one: same numbers as the three
    entry points called one after the other, whatever the slicing."""
    from urgent2026_challenge_track1_amd import metrics
    ref, inf = _pairs(37, 24000, 16000, 41)
    r, e = torch.from_numpy(ref).cuda(), torch.from_numpy(inf).cuda()
    a = metrics.score_batch(r, e, 16000, ("PESQ", "ESTOI", "SDR"), slice_pairs=16, pesq_pairs_per_launch=20)
    torch.cuda.synchronize()
    assert torch.equal(a["ESTOI"], metrics.estoi_batch(r, e, 16000)) and torch.equal(a["SDR"], metrics.sdr_batch(r, e))
    p = metrics.pesq_batch(r, e, 16000)
    assert torch.equal(torch.nan_to_num(a["PESQ"], nan=-1.0), torch.nan_to_num(p, nan=-1.0))
    b = metrics.score_batch(r, e, 16000, ("ESTOI",))
    assert set(b) == {"ESTOI"} and torch.equal(b["ESTOI"], a["ESTOI"])


# ---- edges: degenerate estimate, frame counts, length limit, every corpus rate, SDR tiles (fixtures: tests/metrics_cases.py) -----
@pytest.mark.parametrize("fs,L", mc.DEGENERATE)
def test_estoi_of_an_estimate_that_is_exactly_zero_for_a_whole_segment(lib, fs, L):
    """a gated / muted estimate: 0.6 s of exact zeros -> band rows whose centred sum of squares is 0.  pystoi dithers them (a finite
    score, random at the 1e-3 level); the kernel and the oracle make them zero rows (tests/test_metrics_cpu.py shows the
    rule inside the dither's spread).  Without the rule an exactly zero row is 0 * inf = NaN; with the reference and the estimate
    sharing one complex FFT (tob_kernel before) the silent rows held the reference's rounding residue instead and the kernels scored
    0.03 - 0.14 too high here (0.204 / 0.330 / 0.283 against 0.086 / 0.186 / 0.168 at 10 kHz, L = 12000)."""
    from urgent2026_challenge_track1_amd import metrics
    ref, inf = mc.degenerate_pairs(fs, L)
    r, e = torch.from_numpy(ref).cuda(), torch.from_numpy(inf).cuda()
    a, b = mc.zero_interior_after_resampling(fs, L)
    y = metrics.resample_to_10k(e, fs).cpu().numpy()
    assert b - a >= 29 * 128 + 256 + 128 and not y[:, a:b].any()        # the FIR's support is finite: the interior stays exactly 0
    assert y[:, a - 40:a].any(axis=1).all() and y[:, b:b + 40].any(axis=1).all()
    got = metrics.estoi_batch(r, e, fs).cpu().numpy()
    exp = np.array([metrics_ref.estoi(ref[p], inf[p], fs) for p in range(3)])
    print("degenerate estimate fs %d L %d: kernel %s oracle %s" % (fs, L, got, exp))
    assert np.isfinite(got).all(), got
    assert np.abs(got - exp).max() <= 1e-4, (got, exp)
    zero = metrics.estoi_batch(r, torch.zeros_like(e), fs).cpu().numpy()
    assert np.abs(zero).max() <= 1e-6, zero
    one = metrics.estoi_metric(ref[0], inf[0], fs)
    assert isinstance(one, float) and np.isfinite(one) and abs(one - exp[0]) <= 1e-4
    assert metrics.estoi_metric(ref[0], np.zeros_like(inf[0]), fs) == pytest.approx(0.0, abs=1e-6)


@pytest.mark.parametrize("fs,L", [(10000, 20000), (16000, 32000)])
def test_estoi_of_an_estimate_120_db_down(lib, fs, L):
    """ESTOI does not depend on the estimate's level (rows are normalised, frames are dropped by the reference's energy alone): the
    estimate scaled by 2^-20 (exact in float32) scores what the unscaled one scores, in the oracle to 1e-12 and in the kernels to the
    1e-4 of every other case.  Holds only if nothing of the reference reaches the estimate's spectrum: a transform shared by the two
    signals leaves 1e-7 of the louder one in the other, 10 % of this estimate."""
    from urgent2026_challenge_track1_amd import metrics
    ref, inf = _pairs(3, L, fs, 6)
    quiet = inf * np.float32(2.0 ** -20)
    exp = np.array([metrics_ref.estoi(ref[p], inf[p], fs) for p in range(3)])
    assert np.abs(np.array([metrics_ref.estoi(ref[p], quiet[p], fs) for p in range(3)]) - exp).max() <= 1e-12
    got = metrics.estoi_batch(torch.from_numpy(ref).cuda(), torch.from_numpy(quiet).cuda(), fs).cpu().numpy()
    print("estimate at -120 dB, fs %d: kernel %s oracle %s" % (fs, got, exp))
    assert np.abs(got - exp).max() <= 1e-4, (got, exp)


@pytest.mark.parametrize("L", mc.FRAME_EDGE_SHORT + mc.FRAME_EDGE)
def test_estoi_at_29_to_32_frames(lib, L):
    """stationary noise at 10 kHz keeps every frame, so L sets M: 29 frames -> pystoi's 1e-5 branch, 30 -> one segment, 31 / 32 -> the
    first turns of the segment loop."""
    from urgent2026_challenge_track1_amd import metrics
    ref, inf = (np.stack(v) for v in zip(mc.stationary_pair(L, L), mc.stationary_pair(L, L + 1)))
    got = metrics.estoi_batch(torch.from_numpy(ref).cuda(), torch.from_numpy(inf).cuda(), 10000).cpu().numpy()
    exp = np.array([metrics_ref.estoi(ref[p], inf[p], 10000) for p in range(2)])
    print("ESTOI at L = %d: kernel %s oracle %s" % (L, got, exp))
    if L in mc.FRAME_EDGE_SHORT:
        assert np.all(exp == 1e-5) and np.all(got == np.float32(1e-5)), (got, exp)
    else:
        assert np.all(exp > 0.1) and np.abs(got - exp).max() <= 1e-4, (got, exp)


def test_estoi_batch_whose_pairs_keep_different_numbers_of_frames(lib):
    """the workspaces are uninitialised and as long as the longest pair: a pair that keeps fewer frames must not see its neighbour's (or an
    earlier call's) data.  One call, four pairs of one length; each equals its own single-pair oracle value and its own single-pair call."""
    from urgent2026_challenge_track1_amd import metrics
    ref, inf = mc.mixed_batch()
    r, e = torch.from_numpy(ref).cuda(), torch.from_numpy(inf).cuda()
    loud = torch.from_numpy(np.stack([mc.stationary_pair(ref.shape[1], 80 + p)[0] for p in range(4)])).cuda()
    metrics.estoi_batch(loud, loud.clone(), 10000)             # leaves full-length workspaces behind in the allocator's cache
    del loud
    got = metrics.estoi_batch(r, e, 10000)
    alone = torch.cat([metrics.estoi_batch(r[p:p + 1], e[p:p + 1], 10000) for p in range(4)])
    exp = np.array([metrics_ref.estoi(ref[p], inf[p], 10000) for p in range(4)])
    print("mixed batch: kernel %s oracle %s" % (got.cpu().numpy(), exp))
    assert exp[2] == 1e-5 and float(got[2]) == float(np.float32(1e-5))
    assert np.isfinite(exp).all() and np.all(exp[[0, 1, 3]] > 0.1)
    assert np.abs(got.cpu().numpy() - exp).max() <= 1e-4, (got, exp)
    assert torch.equal(got, alone)


def test_estoi_length_limit(lib):
    """the longest signal urse_estoi_batch admits (silent_frames_kernel's frame table must fit 60 KiB of LDS: 5119 frames, 655,488 samples
    at 10 kHz) matches the oracle; one sample more is refused by name, and the refusal leaves the next call intact."""
    from urgent2026_challenge_track1_amd import metrics
    from urgent2026_challenge_track1_amd._lib import UrseError
    L = 655488
    ref, inf = _pairs(1, L + 1, 10000, 77)
    r, e = torch.from_numpy(ref).cuda(), torch.from_numpy(inf).cuda()
    got = metrics.estoi_batch(r[:, :L], e[:, :L], 10000).cpu().numpy()
    exp = metrics_ref.estoi(ref[0, :L], inf[0, :L], 10000)
    print("ESTOI at the length limit: kernel %.6f oracle %.6f" % (got[0], exp))
    assert abs(got[0] - exp) <= 1e-4, (got, exp)
    with pytest.raises(UrseError, match=str(L + 1)):
        metrics.estoi_batch(r, e, 10000)
    ref, inf = _pairs(2, 20000, 10000, 78)
    got = metrics.estoi_batch(torch.from_numpy(ref).cuda(), torch.from_numpy(inf).cuda(), 10000).cpu().numpy()
    exp = np.array([metrics_ref.estoi(ref[p], inf[p], 10000) for p in range(2)])
    assert np.abs(got - exp).max() <= 1e-4, (got, exp)


@pytest.mark.parametrize("fs", [8000, 16000, 22050, 24000, 32000, 44100])
def test_resample_to_10k_at_every_corpus_rate_and_short_lengths(lib, fs):
    """the polyphase kernel at up / down = 5/4, 5/8, 200/441, 5/12, 5/16, 100/441; lengths of one sample, less than one output sample's
    worth of input, and far less than the filter's span (down * 2 * 5.8 * 10 taps ... 32 k at 441)"""
    from urgent2026_challenge_track1_amd import metrics
    up, down = mc.resample_ratio(fs, 10000)
    rng = np.random.default_rng(fs)
    for L in (1, 7, down, down + 1, 20011):
        x = rng.standard_normal((2, L)).astype(np.float32)
        got = metrics.resample_to_10k(torch.from_numpy(x).cuda(), fs).cpu().numpy()
        exp = np.stack([metrics_ref.resample_oct(x[p].astype(np.float64), 10000, fs) for p in range(2)])
        assert got.shape == exp.shape, (L, got.shape, exp.shape)
        assert np.abs(got - exp).max() <= 2e-6, (L, np.abs(got - exp).max())


@pytest.mark.parametrize("fs_in,fs_out", [(24000, 16000), (8000, 16000), (16000, 48000), (44100, 48000), (22050, 48000)])
def test_soxr_hq_spec_resampler_upwards_and_short(lib, fs_in, fs_out):
    """towards a higher rate (dataset.RawMixBatch, simulate_data_from_param: up / down = 2, 3, 160/147, 320/147), the one corpus rate the
    downward test leaves out, and an input far shorter than the filter"""
    from urgent2026_challenge_track1_amd import metrics
    rng = np.random.default_rng(fs_in + fs_out)
    for L in (5, 30011):
        x = rng.standard_normal((2, L)).astype(np.float32)
        got = metrics.resample_soxr_hq(torch.from_numpy(x).cuda(), fs_in, fs_out).cpu().numpy()
        for p in range(2):
            exp = metrics_ref.resample_soxr_hq_spec(x[p], fs_in, fs_out)
            scale = np.abs(exp).max() if L > 5 else max(np.abs(exp).max(), 1e-3)      # (a floor against an all-tiny output, no loosening)
            assert got[p].shape == exp.shape and np.abs(got[p] - exp).max() <= 2e-6 * scale, (L, p, np.abs(got[p] - exp).max(), scale)


@pytest.mark.parametrize("L", mc.SDR_LENGTHS)
def test_sdr_at_the_tile_edges_and_below_the_filter_length(lib, L):
    """xcorr_kernel's 2048-sample tiles (one short of a tile, exactly one, one sample into the second, into the third) and signals shorter
    than the 512 lags; a silent estimate clamps at -50 dB."""
    from urgent2026_challenge_track1_amd import metrics
    ref, inf = mc.sdr_pairs(L)
    got = metrics.sdr_batch(torch.from_numpy(ref).cuda(), torch.from_numpy(inf).cuda()).cpu().numpy()
    exp = np.array([metrics_ref.sdr(ref[p], inf[p]) for p in range(3)])
    assert np.abs(got - exp).max() <= 1e-4, (got, exp)
    got = metrics.sdr_batch(torch.from_numpy(ref).cuda(), torch.zeros(3, L, device="cuda")).cpu().numpy()
    assert np.abs(got + 50.0).max() <= 1e-4, got


def test_sdr_silent_estimate_leaves_its_neighbours_alone(lib):
    """one pair of the batch has a zero estimate: -50 dB for it, and the others bit-equal to themselves scored alone.  (L = 2049: two
    tiles per pair, so each f64 atomic sum has two commuting terms and the value does not depend on the order of the workgroups.)"""
    from urgent2026_challenge_track1_amd import metrics
    ref, inf = mc.sdr_pairs(2049)
    inf[1] = 0
    r, e = torch.from_numpy(ref).cuda(), torch.from_numpy(inf).cuda()
    got = metrics.sdr_batch(r, e)
    alone = torch.cat([metrics.sdr_batch(r[p:p + 1], e[p:p + 1]) for p in range(3)])
    assert abs(float(got[1]) + 50.0) <= 1e-4
    assert torch.equal(got, alone), (got, alone)
    exp = np.array([metrics_ref.sdr(ref[p], inf[p]) for p in range(3)])
    assert np.abs(got.cpu().numpy() - exp).max() <= 1e-4, (got, exp)
