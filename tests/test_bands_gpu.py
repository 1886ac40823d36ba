"""GPU parity, kernel by kernel: csrc/bands.hip (band split + per-band GroupNorm forward / affine backward, GLU mask apply and
its adjoint, peak normalisation, nan_to_num, axpby, scale by a device scalar) against float64 references on the CPU
(tests/kernel_ref.py).  The band tables are the shipped `_band_tables` of a small core; the references are built from the
subband tuples alone."""
import pytest
import torch

from tests import kernel_ref as kr

pytestmark = pytest.mark.gpu
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
EPS = 1e-5
_cores, _f32_out = {}, {}


def _call(name, *args):
    from urgent2026_challenge_track1_amd._lib import call, stream_ptr
    call(name, *args, stream_ptr())
    torch.cuda.synchronize()


def _tables(dim, F, dtype):
    from urgent2026_challenge_track1_amd.bsrnn import BSRNNCore
    if dim not in _cores:
        _cores[dim] = BSRNNCore(dim, 16, 1, compute_dtype=torch.float32)
    core = _cores[dim]
    tb = core._band_tables(F, dtype, torch.device("cuda", torch.cuda.current_device()))
    rows, ldx, P = kr.band_layout(core.subbands, F, dtype)
    assert (tb["K"], tb["ldx"], tb["P"]) == (len(rows), ldx, P)
    return core.subbands, tb, rows


def _used_cols(rows, ldx):
    used = torch.zeros(ldx, dtype=torch.bool)
    for _, _, sb, xoff, _, _ in rows:
        used[xoff:xoff + 2 * sb] = True
    return used


def _bandsplit_fwd(dim, F, dtype, spec, gamma, beta, copy=False):
    sub, tb, rows = _tables(dim, F, dtype)
    B, T = spec.shape[:2]
    xnb = torch.full((B * T, tb["ldx"]), float("nan"), dtype=dtype, device="cuda")
    xnb2 = torch.full((B * T, tb["ldx"]), float("nan"), dtype=BF16, device="cuda") if copy else None
    stats = torch.full((B * tb["K"] * 2,), float("nan"), dtype=torch.float64, device="cuda")
    from urgent2026_challenge_track1_amd import ops
    _call("bandsplit_norm_fwd", spec.cuda(), tb["bands"], gamma.cuda(), beta.cuda(), xnb, stats, B, T, F, tb["K"], tb["ldx"],
          EPS, ops._dt(xnb), xnb2)
    return xnb.cpu(), stats.cpu(), (xnb2.cpu() if copy else None), sub, tb, rows


@pytest.mark.parametrize("dtype", [F32, BF16, F16])
@pytest.mark.parametrize("dim,F", [(481, 81), (481, 161), (481, 481), (769, 257)])
def test_bandsplit_norm_fwd(lib, dim, F, dtype):
    B, T = 2, 7
    n_gb = 2 * dim
    spec, gamma, beta, _ = kr.draw_spec(B, T, F, n_gb)
    xnb, stats, xnb2, sub, tb, rows = _bandsplit_fwd(dim, F, dtype, spec, gamma, beta, copy=dtype == F16)
    ref, rstats = kr.bandsplit_norm(spec, sub, gamma, beta, EPS, dtype)
    bound = kr.out16(ref, dtype, kr.bandsplit_norm_bound(spec, sub, gamma, beta, EPS, dtype))
    used = _used_cols(rows, tb["ldx"])
    assert torch.all(xnb[:, ~used] == 0)                     # pad columns exactly zero
    assert torch.all(bound[:, ~used] == 0)
    kr.hold("bandsplit_norm_fwd_%s" % str(dtype)[6:], (dim, F, B, T), xnb, ref, bound)
    _, astats = kr.bandsplit_norm(spec.abs(), sub, gamma, beta, EPS, dtype)
    kr.hold("bandsplit_norm_stats", (dim, F, B, T), stats.reshape(B, -1, 2), rstats, 1e-12 * astats)
    if dtype == F32:
        _f32_out[dim, F] = xnb[:, used]
    if dtype == F16:
        # the bf16 copy for the weight-gradient GEMMs: the f32 result rounded once, not the f16 one rounded again
        if (dim, F) not in _f32_out:
            y32, _, _, _, tb32, rows32 = _bandsplit_fwd(dim, F, F32, spec, gamma, beta)
            _f32_out[dim, F] = y32[:, _used_cols(rows32, tb32["ldx"])]
        assert torch.all(xnb2[:, ~used] == 0)
        assert torch.equal(xnb2[:, used].view(torch.int16), _f32_out[dim, F].to(BF16).view(torch.int16))


def test_bandsplit_norm_fwd_constant_spectrum_gives_beta(lib):
    """every value of a band equal: E[x^2] - mean^2 is 0 (clamped if it rounds below), x - mean is 0, the result is beta."""
    B, T, F, dim = 2, 7, 81, 481
    _, gamma, beta, _ = kr.draw_spec(B, T, F, 2 * dim)
    spec = torch.full((B, T, F, 2), 0.3)
    xnb, stats, _, sub, tb, rows = _bandsplit_fwd(dim, F, F32, spec, gamma, beta)
    assert not torch.isnan(xnb).any()
    for _, _, sb, xoff, _, goff in rows:
        assert torch.equal(xnb[:, xoff:xoff + 2 * sb], beta[goff:goff + 2 * sb].expand(B * T, 2 * sb))


def test_bandsplit_norm_bwd(lib):
    B, T, F, dim = 2, 70, 161, 481               # 70 rows: one chunk of 64 and one of 6
    n_gb = 2 * dim
    spec, gamma, beta, g = kr.draw_spec(B, T, F, n_gb)
    _, stats, _, sub, tb, rows = _bandsplit_fwd(dim, F, F32, spec, gamma, beta)
    dxnb = torch.randn(B * T, tb["ldx"], generator=g)
    dg0, db0 = torch.randn(n_gb, generator=g), torch.randn(n_gb, generator=g)
    dg, db = dg0.cuda(), db0.cuda()
    _call("bandsplit_norm_bwd", spec.cuda(), dxnb.cuda(), tb["bands"], stats.cuda(), dg, db, B, T, F, tb["K"], tb["ldx"], EPS)
    rg, rb, ag, ab, n = kr.bandsplit_affine_bwd(spec, sub, gamma, beta, dxnb, EPS, F32)
    end = 2 * (rows[-1][1] + rows[-1][2])        # gamma / beta entries of the bands in use
    assert end == 2 * 181 and torch.all(rg[end:] == 0)
    assert torch.equal(dg.cpu()[end:], dg0[end:]) and torch.equal(db.cpu()[end:], db0[end:])      # bands beyond K: untouched
    kr.hold("bandsplit_norm_bwd_dgamma", (B, T, F), dg, rg + dg0.double(), kr.dot_bound(n, ag + dg0.double().abs()))
    kr.hold("bandsplit_norm_bwd_dbeta", (B, T, F), db, rb + db0.double(), kr.dot_bound(n, ab + db0.double().abs()))


def _glu_mask_case(dim, F, dtype, keep_bands=None):
    sub, tb, rows = _tables(dim, F, dtype)
    bins, vc, gc, P = kr.band_gather_index(sub if keep_bands is None else sub[:keep_bands], F if keep_bands is None else
                                           min(F, sum(sub[:keep_bands])), dtype)
    f2k = tb["f2k"]
    if keep_bands is not None:
        f2k = f2k.clone()
        f2k[f2k >= keep_bands] = -1
        assert int((f2k >= 0).sum()) == len(bins) < F
    return tb, f2k, bins, vc, gc


@pytest.mark.parametrize("keep_bands", [None, 5])
@pytest.mark.parametrize("F", [161, 481])
def test_glu_mask_apply_fwd(lib, F, keep_bands):
    rows_n = 9
    tb, f2k, bins, vc, gc = _glu_mask_case(481, F, F32, keep_bands)
    P = tb["P"]
    pm, pr, x, _ = kr.draw_band_pre(rows_n, F, P)
    out = torch.full((rows_n, F, 2), float("nan"), device="cuda")
    _call("glu_mask_apply_fwd", pm.cuda(), pr.cuda(), x.cuda(), out, tb["bands"], f2k, rows_n, F, P)
    a = kr.band_split_pre(pm, vc, gc) + kr.band_split_pre(pr, vc, gc)
    out = out.cpu()
    mapped = torch.zeros(F, dtype=torch.bool)
    mapped[bins] = True
    assert torch.all(out[:, ~mapped] == 0)                    # bins beyond the used bands: exactly zero
    kr.hold("glu_mask_apply_fwd", (rows_n, F, keep_bands), out[:, mapped], kr.glu_apply(*a, x[:, bins]),
            kr.glu_apply_bound(*a, x[:, bins]))


@pytest.mark.parametrize("keep_bands", [None, 5])
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("F", [161, 481])
def test_glu_mask_apply_bwd(lib, F, dtype, keep_bands):
    from urgent2026_challenge_track1_amd import ops
    rows_n = 9
    tb, f2k, bins, vc, gc = _glu_mask_case(481, F, dtype, keep_bands)
    P = tb["P"]
    pm, pr, x, dout = kr.draw_band_pre(rows_n, F, P)
    fill = 0.0 if keep_bands is None else 7.0      # pre-zeroed as maskdec_bwd does; a sentinel shows what the kernel leaves alone
    dpm = torch.full((rows_n, P), fill, dtype=dtype, device="cuda")
    dpr = torch.full((rows_n, P), fill, dtype=dtype, device="cuda")
    _call("glu_mask_apply_bwd", pm.cuda(), pr.cuda(), x.cuda(), dout.cuda(), dpm, dpr, tb["bands"], f2k, rows_n, F, P,
          ops._dt(dpm))
    a = kr.band_split_pre(pm, vc, gc) + kr.band_split_pre(pr, vc, gc)
    refs = kr.glu_apply_bwd(*a, x[:, bins], dout[:, bins])
    bounds = kr.glu_apply_bwd_bounds(*a, x[:, bins], dout[:, bins])
    written = kr.band_scatter_pre(torch.ones_like(refs[0]), torch.ones_like(refs[1]), vc, gc, P) != 0
    for got, (rv, rg), (bv, bg) in ((dpm, refs[:2], bounds[:2]), (dpr, refs[2:], bounds[2:])):
        got = got.cpu()
        ref = kr.band_scatter_pre(rv, rg, vc, gc, P)
        bound = kr.out16(ref, dtype, kr.band_scatter_pre(bv, bg, vc, gc, P))
        assert torch.all(got[~written] == fill)               # pads and unmapped bands: as they were
        kr.hold("glu_mask_apply_bwd_%s" % str(dtype)[6:], (rows_n, F, keep_bands), got[written], ref[written], bound[written])


@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("n", [1, 255, 100003, 2 ** 20 + 257])
def test_peak_normalize(lib, n, where):
    g = kr.gen(31 + n)
    x = torch.randn(n, generator=g).clamp_(-3, 3)
    x[0 if where == "first" else n - 1] = -4.25          # the peak is negative
    xc = x.cuda()
    scratch = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    _call("peak_normalize", xc, n, 0.9, scratch)
    ref = kr.peak_normalize(x, float(torch.tensor(0.9, dtype=F32)))
    kr.hold("peak_normalize", (n, where), xc, ref, 3 * kr.U24 * ref.abs())


def test_nan_to_num_bits(lib):
    tiny = torch.tensor([1, 0x007FFFFF, 1 - 2 ** 31], dtype=torch.int32).view(F32)       # denormals
    x = torch.cat([torch.tensor([float("nan"), -float("nan"), float("inf"), -float("inf"), 0.0, -0.0, 1.5, -3.4e38]), tiny])
    x = x.repeat(300)[:2051]
    y = torch.full_like(x, 9.0).cuda()
    _call("nan_to_num", x.cuda(), y, x.numel())
    assert torch.equal(y.cpu().view(torch.int32), torch.nan_to_num(x, nan=0.0).view(torch.int32))


def test_axpby_overwrites_nan_when_b_is_zero(lib):
    n = 1031
    x = torch.randn(n, generator=kr.gen(33))
    y = torch.full((n,), float("nan"), device="cuda")
    _call("axpby", x.cuda(), y, 0.75, 0.0, n)
    assert torch.equal(y.cpu(), 0.75 * x)                   # one f32 product, no NaN carried over
    y0 = torch.randn(n, generator=kr.gen(34))
    y = y0.cuda()
    _call("axpby", x.cuda(), y, 0.75, -0.5, n)
    ref = 0.75 * x.double() - 0.5 * y0.double()
    kr.hold("axpby", (n,), y, ref, 2 * kr.U24 * (0.75 * x.double().abs() + 0.5 * y0.double().abs()))


def test_scale_by_device_scalar_bits(lib):
    n = 256 * 16 * 256 + 257
    x = torch.randn(n, generator=kr.gen(35))
    s = torch.tensor([0.3337], dtype=F32)
    xc = x.cuda()
    _call("scale_by_device_scalar", xc, s.cuda(), n)
    assert torch.equal(xc.cpu(), x * s)
