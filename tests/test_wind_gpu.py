"""GPU: the wind-noise stage (csrc/wind.hip, ``mixing.wind_noise``) against its float64 restatement tests/wind_ref.py on identical float32
inputs and against closed forms that do not depend on the restatement; ``simulate_recipes(..., wind_compressor=True)`` against the stages of
oracle/mix_ref.py composed with it; ``simulate_data_from_param --wind_noise_compressor device``.

The restatement itself (ffmpeg's sidechaincompress + amix from their published definition) is NOT pinned against an ffmpeg binary: none
exists where this suite runs (DESIGN.md sections 4 and 10)."""
import os

import numpy as np
import pytest

from tests import wind_ref as wr

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FLOAT_BOUND = 2e-5          # tests/test_simulate_gpu.py::test_float_results_meet_the_bound_of_the_on_the_fly_path


def _dev(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a)).cuda()


def _run_kernel(cs):
    """``urse_wind_mix`` with a per-row fs (the wrapper serves batches of one fs)"""
    import torch
    from urgent2026_challenge_track1_amd import _lib, mixing
    t = {k: _dev(cs[k]) for k in ("speech", "x", "noise", "noisy")}
    rows = cs["wind"]
    table = [[float(cs["par"][b][k]) for k in mixing.WIND_PARAMS] + [float(cs["par"][b]["fs"]), 1.0 if cs["par"][b]["has_rir"] else 0.0]
             for b in rows]
    c = torch.empty(len(rows), dtype=torch.float64, device="cuda")
    _lib.call("wind_mix", t["speech"], t["x"], t["noise"], t["noisy"], _dev(np.asarray(cs["lens"], dtype=np.int32)), cs["B"], cs["ld"],
              _dev(np.asarray(rows, dtype=np.int32)), len(rows), _dev(np.asarray(table, dtype=np.float64)), c, _lib.stream_ptr())
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in t.items()}, c.cpu().numpy()


@pytest.fixture(scope="module")
def kernel_run(lib):
    from urgent2026_challenge_track1_amd import mixing
    cs = wr.kernel_cases(mixing.wind_chunk())
    got, c = _run_kernel(cs)
    return cs, got, c, wr.run_cases(cs)


def test_kernel_matches_the_float64_restatement(kernel_run):
    """Row lengths 1, chunk - 1, chunk, chunk + 1, 3 chunk + 17; fs 8000 with ka at its cap and fs 48000; ratios 1, 7.9, 20; rows below, inside and
    above the knee.  Every sample within one 16-bit step 2^-15 / c of the oracle; at most 1 sample in 1,000 of a row off by more than one float32
    unit in the last place of the stored result (the oracle's float64 value cast to float32 against the kernel's own cast).  What that cap has to
    absorb: tests/test_wind_cpu.py::test_last_bit_of_the_inputs_moves_few_rounding_decisions moves every input by one float32 ulp and measures
    at most 0.00098 (one sample of a 1023-sample row; 0.00032 on the 3089-sample rows); here the inputs are identical and only the last bits of
    ln / exp differ."""
    cs, got, c, want = kernel_run
    s6, s7 = want[6]["S"], want[7]["S"]
    for S, st in ((s6, want[6]["setup"]), (s7, want[7]["setup"])):
        below, above = S <= st["adj_knee_start"], S >= st["lin_knee_stop"] ** 2
        assert below.sum() > 20 and above.sum() > 20 and (~below & ~above).sum() > 20, (below.sum(), above.sum())
    assert wr.setup(0.05, 20.0, 0.01, 5.0, 8000)["ka"] == 1.0
    for j, b in enumerate(cs["wind"]):
        n = cs["lens"][b]
        assert c[j] == want[b]["c"], (b, c[j], want[b]["c"])
        for kind in ("noisy", "noise"):
            d = np.abs(got[kind][b, :n].astype(np.float64) - want[b][kind])
            off = d > wr.f32_step(want[b][kind])
            print("row %d (%d samples) %s: worst %.3e (step %.3e), %d samples off" % (b, n, kind, d.max(), 2.0 ** -15 / c[j], off.sum()))
            assert d.max() <= 2.0 ** -15 / want[b]["c"], (b, kind, d.max())
            assert off.sum() <= n / 1000.0, (b, kind, int(off.sum()), n)


def test_kernel_writes_the_listed_rows_up_to_their_lengths_only(kernel_run):
    cs, got, c, want = kernel_run
    for b in range(cs["B"]):
        n = cs["lens"][b] if b in cs["wind"] else 0
        for kind in ("noisy", "noise", "speech"):
            assert np.array_equal(got[kind][b, n:], cs[kind][b, n:]), (b, kind)
        assert np.array_equal(got["x"][b], cs["x"][b])
        if b in cs["wind"]:
            assert not np.array_equal(got["noisy"][b, :n], cs["noisy"][b, :n])


def test_clean_target_is_rescaled_only_without_an_rir(kernel_run):
    cs, got, c, want = kernel_run
    seen = set()
    for j, b in enumerate(cs["wind"]):
        n = cs["lens"][b]
        if cs["par"][b]["has_rir"]:
            assert np.array_equal(got["speech"][b, :n], cs["speech"][b, :n])
        else:
            assert np.array_equal(got["speech"][b, :n], (c[j] * cs["speech"][b, :n].astype(np.float64)).astype(np.float32))
            assert c[j] != 1.0
        seen.add(cs["par"][b]["has_rir"])
    assert seen == {True, False}


def test_wrapper_takes_x_as_the_clean_target_and_lists_of_recipe_values(lib):
    """``mixing.wind_noise`` on a batch of one fs, with the clean target aliasing x (a batch without any RIR)"""
    import torch
    from urgent2026_challenge_track1_amd import mixing
    n = 2 * mixing.wind_chunk() + 3
    rng = np.random.default_rng(5)
    x = (0.2 * rng.standard_normal((2, n))).astype(np.float32)
    v = (0.1 * rng.standard_normal((2, n))).astype(np.float32)
    par = dict(threshold=0.1, ratio=4.0, attack=10.0, release=60.0, sc_gain=1.1, clipping_threshold=0.9)
    xs, vs, ns = _dev(x), _dev(v), _dev(x + v)
    c = mixing.wind_noise(xs, xs, vs, ns, [n, n - 7], [1], [par], [False], 16000)
    torch.cuda.synchronize()
    want = wr.wind_mix(x[1, :n - 7], v[1, :n - 7], x[1, :n - 7], 16000, has_rir=False, **par)
    assert float(c[0]) == want["c"]
    assert np.array_equal(xs.cpu().numpy()[1, :n - 7], want["speech"].astype(np.float32)) and np.array_equal(xs.cpu().numpy()[0], x[0])
    assert np.abs(ns.cpu().numpy()[1, :n - 7] - want["noisy"]).max() <= 2.0 ** -15 / want["c"]
    with pytest.raises(ValueError):
        mixing.wind_noise(xs, xs, vs, ns, [n, n], [1, 1], [par, par], [False, False], 16000)


def test_closed_forms_hold_on_the_device(lib):
    """(a) ratio 1: the mixture is Q(0.5 xq + 0.5 vq) wherever that rounding is not decided by less than 1e-9 of a step (g is 1 up to the last
    bits of ln / exp; within one step elsewhere); (b) a silent side chain: exactly Q(0.5 xq); (c) a constant side chain: the geometric attack
    S_t = (k sc_gain)^2 (1 - (1 - ka)^(t + 1)) and, above the knee, g_t = exp((0.5 ln S_t - thres)(1 / ratio - 1)) - the closed form carries
    1e-11 of relative rounding of its own, so decisions closer than 1e-6 of a step are left out.  clipping_threshold 1 switches the clipper off."""
    import torch
    from urgent2026_challenge_track1_amd import mixing
    n, fs = 2 * mixing.wind_chunk() + 451, 16000
    rng = np.random.default_rng(11)
    x = (0.25 * rng.standard_normal((3, n))).astype(np.float32)
    v = np.stack([(0.3 * rng.standard_normal(n)), np.zeros(n), np.full(n, 0.12)]).astype(np.float32)
    par = [dict(threshold=0.1, ratio=1.0, attack=20.0, release=50.0, sc_gain=1.0, clipping_threshold=1.0),
           dict(threshold=0.1, ratio=7.9, attack=20.0, release=50.0, sc_gain=1.2, clipping_threshold=1.0),
           dict(threshold=0.05, ratio=7.9, attack=100.0, release=50.0, sc_gain=1.1, clipping_threshold=1.0)]
    sp, ns, vs = _dev(x.copy()), _dev(x + v), _dev(v)
    c = mixing.wind_noise(sp, _dev(x), vs, ns, [n] * 3, [0, 1, 2], par, [True] * 3, fs).cpu().numpy()
    torch.cuda.synchronize()
    got = ns.cpu().numpy().astype(np.float64)
    for b in range(3):
        peak = max(np.abs(x[b]).max(), np.abs(v[b]).max())
        assert c[b] == 0.9 / np.float64(peak)
    mq = np.rint(got * c[:, None] * 32768.0) / 32768.0                      # the 16-bit value behind the stored float32
    assert np.abs(mq * 32768.0 - got * c[:, None] * 32768.0).max() < 1e-2
    xq, vq = wr.q16(c[:, None] * x.astype(np.float64)), wr.q16(c[:, None] * v.astype(np.float64))
    assert np.array_equal(vs.cpu().numpy(), (vq / c[:, None]).astype(np.float32))
    # (a)
    plain = 0.5 * xq[0] + 0.5 * vq[0]
    tie = wr.near_tie(plain)
    assert np.array_equal(mq[0][~tie], wr.q16(plain)[~tie]) and np.abs(mq[0] - wr.q16(plain)).max() <= 2.0 ** -15 and (~tie).mean() > 0.4
    # (b)
    assert np.array_equal(mq[1], wr.q16(0.5 * xq[1]))
    # (c)
    k = vq[2][0]
    assert np.all(vq[2] == k)
    ka = 1.0 / (par[2]["attack"] * fs / 4000.0)
    S = (k * par[2]["sc_gain"]) ** 2 * (1.0 - (1.0 - ka) ** (np.arange(n) + 1.0))
    st = wr.setup(par[2]["threshold"], par[2]["ratio"], par[2]["attack"], par[2]["release"], fs)
    above, below = S > st["lin_knee_stop"] ** 2 * (1 + 1e-9), S < st["adj_knee_start"] * (1 - 1e-9)
    assert above.sum() > 1000 and below.sum() > 10
    g = np.ones(n)
    g[above] = np.exp((0.5 * np.log(S[above]) - np.log(par[2]["threshold"])) * (1.0 / par[2]["ratio"] - 1.0))
    m = 0.5 * (xq[2] * g) + 0.5 * vq[2]
    sure = (above | below) & ~wr.near_tie(m, 1e-6)
    assert np.array_equal(mq[2][sure], wr.q16(m)[sure]) and sure.sum() > 1000
    assert g[above].max() < 0.9                                             # the speech is ducked, not copied


def _e2e_inputs():
    rng = np.random.default_rng(2026)
    fs, lens = 16000, [6000, 5000, 4100]
    L = max(lens)
    sp = np.zeros((3, L), dtype=np.float32)
    for b, n in enumerate(lens):
        sp[b, :n] = (0.1 * rng.standard_normal(n) * (1.0 + np.sin(np.arange(n) / 300.0))).astype(np.float32)
    nlens = [2500, 5000, 7000]
    nz = np.zeros((3, max(nlens)), dtype=np.float32)
    for b, n in enumerate(nlens):
        nz[b, :n] = (0.05 * rng.standard_normal(n) * (0.05 + np.sin(np.pi * np.arange(n) / n) ** 2)).astype(np.float32)
    R = 900
    rir = np.zeros((3, R), dtype=np.float32)
    h = rng.standard_normal(R) * np.exp(-np.arange(R) / 120.0)
    h[:20] = 0.0
    h[20] = 1.0
    rir[1] = h.astype(np.float32)
    wind = dict(threshold=0.2, ratio=7.9, attack=57.5, release=23.6, sc_gain=0.87, clipping=True, clipping_threshold=0.9)
    recipes = [dict(snr=3.0, params=dict(wind_noise=wind), order=[], noise_offset=1234, highpass=True, wind=True, length=lens[0]),
               dict(snr=-2.0, params=dict(wind_noise=dict(wind, ratio=20.0, threshold=0.1)), order=[], noise_offset=0, highpass=True, wind=True,
                    length=lens[1]),
               dict(snr=5.0, params={}, order=[], noise_offset=777, highpass=True, wind=False, length=lens[2])]
    return fs, lens, sp, nlens, nz, rir, [0, R, 0], recipes


def _e2e_oracle(fs, n, sp, nz, rir, recipe, stop):
    from oracle import mix_ref
    hp = mix_ref.high_pass(sp[None, :n].astype(np.float64), fs)
    x = clean = hp
    if rir is not None:
        x = mix_ref.add_reverberation(hp, rir[None].astype(np.float64))
        clean = mix_ref.add_reverberation(hp, rir[None, :stop].astype(np.float64))
    noisy, v = mix_ref.mix_noise(x, nz[None].astype(np.float64), recipe["snr"], recipe["noise_offset"])
    c = None
    if recipe["wind"]:
        w = recipe["params"]["wind_noise"]
        r = wr.wind_mix(x[0], v[0], clean[0], fs, w["threshold"], w["ratio"], w["attack"], w["release"], w["sc_gain"], w["clipping_threshold"],
                        rir is not None)
        clean, noisy, v, c = r["speech"][None], r["noisy"][None], r["noise"][None], r["c"]
    scale = 0.9 / max(np.abs(noisy).max(), np.abs(clean).max(), np.abs(v).max(), 1e-6)
    return clean[0] * scale, noisy[0] * scale, v[0] * scale, scale, c


def test_simulate_recipes_with_the_compressor_matches_the_composed_oracle(lib):
    """16 kHz, three rows: wind without an RIR, wind with one, plain noise.  Bound: the on-the-fly bound 2e-5 (float32 arithmetic upstream, 0.9-peak
    signals) + 2 * 2^-15 * (normalisation factor / c): xq and vq may each move one 16-bit step under the upstream error, the mixture m then
    moves by at most one step, and its own rounding adds one more."""
    import torch
    from urgent2026_challenge_track1_amd import mixing
    fs, lens, sp, nlens, nz, rir, rir_lens, recipes = _e2e_inputs()
    stop = mixing.early_rir_stop(rir[1], fs)
    stops = [0, stop, 0]
    out = {}
    for on in (True, False):
        skipped = {}
        res = mixing.simulate_recipes(_dev(sp), lens, _dev(nz), nlens, _dev(rir), rir_lens, stops, fs, [dict(r) for r in recipes], skipped,
                                      return_noise=True, wind_compressor=on)
        torch.cuda.synchronize()
        out[on] = [t.cpu().numpy() for t in res], skipped
    (clean, noisy, noise), skipped = out[True]
    assert "wind_noise" not in skipped and skipped == {}
    assert out[False][1] == {"wind_noise": 2}
    for kind in range(3):                                                  # the plain row does not notice the switch
        assert np.array_equal(out[True][0][kind][2], out[False][0][kind][2])
    assert not np.array_equal(noisy[0], out[False][0][1][0]) and not np.array_equal(noisy[1], out[False][0][1][1])
    for b in range(3):
        n = lens[b]
        wc, wn, wv, scale, c = _e2e_oracle(fs, n, sp[b], nz[b, :nlens[b]], rir[b, :rir_lens[b]] if rir_lens[b] else None, recipes[b], stops[b])
        bound = FLOAT_BOUND + (2.0 * 2.0 ** -15 * scale / c if c is not None else 0.0)
        for name, got, want in (("clean", clean, wc), ("noisy", noisy, wn), ("noise", noise, wv)):
            err = float(np.abs(got[b, :n].astype(np.float64) - want).max())
            print("row %d %s: %.3e (bound %.3e)" % (b, name, err, bound))
            assert err <= bound, (b, name, err, bound)
            assert np.all(got[b, n:] == 0.0)
        assert abs(max(np.abs(clean[b]).max(), np.abs(noisy[b]).max(), np.abs(noise[b]).max()) - 0.9) < 1e-4


def test_batches_and_the_prefetcher_pass_the_switch_on(lib):
    """``RawMixBatch.simulate / materialise`` and ``train_se.DevicePrefetcher`` (what ``train_se.fit`` builds from ``cfg.wind_noise_compressor``) hand
    the switch to ``simulate_recipes``: the same tensors as the direct call, and no wind row counted as not applied"""
    import copy
    import torch
    from urgent2026_challenge_track1_amd import mixing, train_se
    from urgent2026_challenge_track1_amd.dataset import RawMixBatch
    fs, lens, sp, nlens, nz, rir, rir_lens, recipes = _e2e_inputs()
    items = [dict(speech=sp[b:b + 1, :lens[b]], noise=nz[b:b + 1, :nlens[b]], rir=rir[b:b + 1, :rir_lens[b]] if rir_lens[b] else None,
                  recipe=dict(recipes[b]), fs=fs, length=lens[b]) for b in range(3)]
    raw = RawMixBatch(items)
    stops = [0, mixing.early_rir_stop(rir[1:2], fs), 0]
    want = mixing.simulate_recipes(_dev(sp), lens, _dev(nz), nlens, _dev(rir), rir_lens, stops, fs, [dict(r) for r in recipes], {}, wind_compressor=True)
    off = mixing.simulate_recipes(_dev(sp), lens, _dev(nz), nlens, _dev(rir), rir_lens, stops, fs, [dict(r) for r in recipes], {})
    skipped = {}
    got = copy.deepcopy(raw).simulate("cuda", skipped, wind_compressor=True)
    assert skipped == {} and all(torch.equal(a, b) for a, b in zip(got, want))
    clean, noisy, fs_t, lengths = copy.deepcopy(raw).materialise("cuda", skipped, True)
    assert skipped == {} and torch.equal(clean[:, 0], want[0]) and torch.equal(noisy[:, 0], want[1]) and int(fs_t) == fs
    for on, ref in ((True, want), (False, off)):
        skipped = {}
        (clean, noisy, _, _), = list(train_se.DevicePrefetcher([copy.deepcopy(raw)], "cuda", skipped, wind_compressor=on))
        torch.cuda.synchronize()
        assert torch.equal(noisy[:, 0], ref[1]) and torch.equal(clean[:, 0], ref[0])
        assert skipped == ({} if on else {"wind_noise": 2})
    assert not torch.equal(want[1], off[1])
    skipped = {}
    (clean, noisy, _, _), = list(train_se.DevicePrefetcher([copy.deepcopy(raw)], "cuda", skipped))          # nothing passed: the configuration's default
    assert torch.equal(noisy[:, 0], off[1]) and skipped == {"wind_noise": 2}


def test_offline_simulator_with_the_flag(lib, tmp_path):
    """a plain row and a wind row of one meta.tsv: with ``--wind_noise_compressor device`` nothing is listed as lacking and the wind row's noisy
    file is the compressor's mixture (the bound of the test above, within one LSB of the file); without the flag the wind row is byte for byte
    the additive mixture (the same sources listed as a plain noise), listed in unsupported.tsv, and the plain row is the same file both ways."""
    from oracle import mix_ref
    from tests import test_simulate_gpu as tsg
    from urgent2026_challenge_track1_amd import mixing, simulate_data_from_param as sdp
    g = np.load(os.path.join(GOLDEN, "ref_simulate.npz"))
    root = str(tmp_path)
    scp0 = tsg._write_corpus(g, root)
    scp = os.path.join(root, "with_wind.scp")
    with open(scp, "w") as f:
        f.write(open(scp0).read() + "wind_noise16000_0 16000 %s\n" % os.path.join(root, "src", "nz16000_short.wav"))
    base = next(r for r in tsg._rows(g) if r["fs"] == "16000" and r["highpass"])
    text = "wind_noise(threshold=0.2,ratio=7.9,attack=57.5,release=23.6,sc_gain=0.87,clipping=False,clipping_threshold=0.9)/"
    plain = dict(base, id="fileid_5", augmentation="none")
    wind = dict(base, id="fileid_6", noise_uid="wind_noise16000_0", augmentation=text)
    as_plain = dict(base, id="fileid_6", noise_uid="nz16000_short", augmentation="none")
    logs = {tag: tsg._write_meta(rows, root, tag, "wav") for tag, rows in (("dev", [plain, wind]), ("off", [plain, wind]), ("add", [as_plain]))}
    n, lacking = tsg._run(scp, logs["dev"], True, ["--wind_noise_compressor", "device", "--unsupported_augmentation", "raise"])
    assert n == 2 and lacking == [] and open(os.path.join(logs["dev"], "unsupported.tsv")).read() == "id\taugmentation\n"
    n, lacking = tsg._run(scp, logs["off"], True)
    assert lacking == [("fileid_6", "wind_noise")]
    assert open(os.path.join(logs["off"], "unsupported.tsv")).read() == "id\taugmentation\nfileid_6\twind_noise\n"
    tsg._run(scp, logs["add"], True)

    def data(tag, kind, uid):
        return open(os.path.join(root, "out_" + tag, kind, "0", uid + ".wav"), "rb").read()
    for kind in ("clean", "noisy", "noise"):
        assert data("off", kind, "fileid_6") == data("add", kind, "fileid_6"), kind        # the default is the additive mixture
        assert data("off", kind, "fileid_5") == data("dev", kind, "fileid_5"), kind        # a plain row does not notice the flag
    assert data("dev", "noisy", "fileid_6") != data("off", "noisy", "fileid_6")
    # the wind row against the composed oracle
    fs, length = 16000, int(base["length"])
    sp, nz = g["sim_audio_" + base["speech_uid"]], g["sim_audio_nz16000_short"]
    rir = None if base["rir_uid"] == "none" else g["sim_audio_" + base["rir_uid"]]
    stop = 0 if rir is None else mixing.early_rir_stop(rir, fs)
    recipe = dict(sdp.parse_row(dict(wind, length=str(length)), True, wind_compressor=True)[0], noise_offset=sdp.noise_offset("fileid_6", len(sp), len(nz)))
    wc, wn, wv, scale, c = _e2e_oracle(fs, len(sp), sp, nz, rir, recipe, stop)
    bound = FLOAT_BOUND + 2.0 * 2.0 ** -15 * scale / c
    for kind, want in (("clean", wc), ("noisy", wn), ("noise", wv)):
        pcm, rate = tsg._pcm(os.path.join(root, "out_dev", kind, "0", "fileid_6.wav"))
        err = float(np.abs(pcm / 32768.0 - want).max())
        print("%s: %.3e (bound %.3e + one LSB)" % (kind, err, bound))
        assert rate == fs and len(pcm) == length and err <= bound + 2.0 ** -15, (kind, err)
