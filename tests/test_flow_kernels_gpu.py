"""GPU parity, kernel by kernel: csrc/flow.hip (5x5 convolution, GLU + complex mask apply, tanh backward pack, spectral
exponent transform, flow-matching state / loss, Euler axpy, EMA, time embedding) against float64 references on the CPU
(tests/kernel_ref.py: formulas, bounds and the reasoning behind each), at shapes where the spectrum is narrower than the band
table (Fs > F) and tiles are ragged.  One model-level test runs the flow DNN at F = 257 and F = 385."""
import pytest
import torch

from tests import kernel_ref as kr

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16


def _call(name, *args):
    from urgent2026_challenge_track1_amd._lib import call, stream_ptr
    call(name, *args, stream_ptr())
    torch.cuda.synchronize()


CONV_SHAPES = [(1, 8, 32), (2, 9, 37), (1, 3, 5), (2, 17, 259)]


@pytest.mark.parametrize("B,T,Fs", CONV_SHAPES)
def test_conv5x5_fwd(lib, B, T, Fs):
    U, W, b, _ = kr.draw_conv(B, T, Fs)
    pre = torch.full((B, T, Fs, 4), float("nan"), device="cuda")
    _call("conv5x5_fwd", U.cuda(), W.cuda(), b.cuda(), pre, B, T, Fs)
    kr.hold("conv5x5_fwd", (B, T, Fs), pre, kr.conv5x5(U, W, b), kr.conv5x5_bound(U, W, b))


@pytest.mark.parametrize("B,T,Fs", CONV_SHAPES)
def test_conv5x5_bwd_accumulates_weight_gradients(lib, B, T, Fs):
    U, W, b, dpre = kr.draw_conv(B, T, Fs)
    g = kr.gen(B + T + Fs)
    dW0, db0 = torch.randn(W.shape, generator=g), torch.randn(b.shape, generator=g)
    dU = torch.full((B, T, Fs, 16), float("nan"), device="cuda")
    dW, db = dW0.cuda(), db0.cuda()
    _call("conv5x5_bwd", U.cuda(), W.cuda(), dpre.cuda(), dU, dW, db, B, T, Fs)
    rU, rW, rb = kr.conv5x5_bwd(U, W, b, dpre)
    bU, bW, bb = kr.conv5x5_bwd_bounds(U, W, b, dpre, dW0, db0)
    kr.hold("conv5x5_bwd_dU", (B, T, Fs), dU, rU, bU)
    kr.hold("conv5x5_bwd_dW", (B, T, Fs), dW, rW + dW0.double(), bW)
    kr.hold("conv5x5_bwd_dbias", (B, T, Fs), db, rb + db0.double(), bb)


@pytest.mark.parametrize("sgn", [1.0, -1.0])
@pytest.mark.parametrize("rows,F,Fs", [(10, 257, 259), (6, 385, 409), (7, 129, 129)])
def test_glu4_apply_fwd_bwd(lib, rows, F, Fs, sgn):
    pm, pr, x, dout = kr.draw_glu4(rows, F, Fs)
    a = kr.glu4_split(pm, F) + kr.glu4_split(pr, F)
    out = torch.full((rows, F, 2), float("nan"), device="cuda")
    _call("glu4_apply_fwd", pm.cuda(), pr.cuda(), x.cuda(), out, rows, F, Fs, sgn)
    kr.hold("glu4_apply_fwd", (rows, F, Fs), out, kr.glu_apply(*a, x, sgn), kr.glu_apply_bound(*a, x, sgn))
    dpm = torch.full((rows, Fs, 4), float("nan"), device="cuda")
    dpr = torch.full((rows, Fs, 4), float("nan"), device="cuda")
    _call("glu4_apply_bwd", pm.cuda(), pr.cuda(), x.cuda(), dout.cuda(), dpm, dpr, rows, F, Fs, sgn)
    refs, bounds = kr.glu_apply_bwd(*a, x, dout, sgn), kr.glu_apply_bwd_bounds(*a, x, dout, sgn)
    for got, (rv, rg), (bv, bg) in ((dpm, refs[:2], bounds[:2]), (dpr, refs[2:], bounds[2:])):
        got = got.cpu()
        assert torch.all(got[:, F:] == 0)        # pad columns of the Fs-wide map: exactly zero, from a NaN-filled buffer
        kr.hold("glu4_apply_bwd", (rows, F, Fs), got[:, :F], torch.cat([rv, rg], -1), torch.cat([bv, bg], -1))


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_tanh_bwd_pack(lib, dtype):
    from urgent2026_challenge_track1_amd import ops
    rows, n = 5, 259 * 16
    ldd = ops.kpad(n, dtype)
    assert (ldd > n) == (dtype == BF16)          # 259 * 16 is a multiple of 16, not of 32: only the bf16 rows have pads
    g = kr.gen(11)
    U = torch.tanh(1.5 * torch.randn(rows, n, generator=g))
    dU = torch.randn(rows, n, generator=g)
    dst = torch.zeros(rows, ldd, dtype=dtype, device="cuda")
    _call("tanh_bwd_pack", dU.cuda(), U.cuda(), dst, rows, n, ldd, ops._dt(dst))
    dst = dst.cpu()
    assert torch.all(dst[:, n:] == 0)
    kr.hold("tanh_bwd_pack_%s" % str(dtype)[6:], (rows, n, ldd), dst[:, :n], kr.tanh_bwd(dU, U), kr.tanh_bwd_bound(dU, U, dtype))


@pytest.mark.parametrize("n", [1, 256 * 16 * 256 + 257])
@pytest.mark.parametrize("exponent,factor", [(0.667, 0.065), (1.0, 0.065)])
def test_spec_transform(lib, exponent, factor, n):
    x = kr.draw_complex_logmag(n)
    xc = x.cuda()
    outs = []
    for inverse in (0, 1):
        y = torch.full((n, 2), float("nan"), device="cuda")
        _call("spec_transform", xc, y, n, exponent, factor, inverse)
        ref = kr.spec_transform(x, exponent, factor, inverse)
        rel = kr.spec_transform_rel(x, exponent, factor, inverse)
        kr.hold("spec_transform_%s" % ("inv" if inverse else "fwd"), (n, exponent), y, ref, rel * ref.abs())
        if n > 2:
            assert torch.all(y[n // 2] == 0)         # exact zero in, exact zero out
        outs.append(y)
    # inverse(forward(x)) = x: the forward's error reaches a component directly and through the magnitude (|1/e - 1|)
    back = torch.full((n, 2), float("nan"), device="cuda")
    _call("spec_transform", outs[0], back, n, exponent, factor, 1)
    fwd_rel = kr.spec_transform_rel(x, exponent, factor, 0)
    rel = (1 + abs(1 / exponent - 1)) * fwd_rel + kr.spec_transform_rel(outs[0].cpu(), exponent, factor, 1)
    kr.hold("spec_transform_round_trip", (n, exponent), back, x.double(), rel * x.double().abs())


@pytest.mark.parametrize("with_cvf", [True, False])
def test_flow_prepare(lib, with_cvf):
    B, per_b, smin, smax = 3, 1031, 0.05, 0.5
    x0, y, z = kr.draw_flow_state(B, per_b)
    t = torch.tensor([0.0, 1.0, 0.37])
    xt = torch.full((B, per_b, 2), float("nan"), device="cuda")
    cvf = torch.full((B, per_b, 2), float("nan"), device="cuda") if with_cvf else None
    _call("flow_prepare", x0.cuda(), y.cuda(), z.cuda(), t.cuda(), xt, cvf, B, per_b, smin, smax)
    (r_xt, r_cvf), (b_xt, b_cvf) = kr.flow_prepare(x0, y, z, t, per_b, smin, smax), kr.flow_prepare_bounds(x0, y, z, t, smin, smax)
    kr.hold("flow_prepare_xt", (B, per_b), xt, r_xt, b_xt)
    if with_cvf:
        kr.hold("flow_prepare_cvf", (B, per_b), cvf, r_cvf, b_cvf)


def test_axpy_and_ema_update(lib):
    n = 256 * 16 * 256 + 257                        # past the grid cap: the grid-stride loop runs
    g = kr.gen(12)
    x, y = torch.randn(n, generator=g), torch.randn(n, generator=g)
    yc = y.cuda()
    _call("axpy", x.cuda(), yc, -1.0 / 15, n)
    a = float(torch.tensor(-1.0 / 15, dtype=F32))   # the scalar as the C ABI receives it
    kr.hold("axpy", (n,), yc, y.double() + a * x.double(), 2 * kr.U24 * (y.double().abs() + abs(a) * x.double().abs()))
    sc = y.cuda()
    omd = float(torch.tensor(1.0 - 0.999, dtype=F32))
    _call("ema_update", sc, x.cuda(), omd, n)
    ref = y.double() - omd * (y.double() - x.double())
    kr.hold("ema_update", (n,), sc, ref, 3 * kr.U24 * (y.double().abs() + omd * (y.double().abs() + x.double().abs())))


@pytest.mark.parametrize("half", [8, 192])
def test_time_embedding(lib, half):
    g = kr.gen(13 + half)
    t = 0.03 + 0.97 * torch.rand(3, generator=g)
    t[0], t[1] = 0.03, 1.0
    W = torch.randn(half, generator=g)
    out = torch.full((3, 2 * half), float("nan"), device="cuda")
    _call("time_embedding", t.cuda(), W.cuda(), out, 3, half)
    ref, p = kr.time_embedding(t, W)
    kr.hold("time_embedding", (3, half), out, ref, kr.time_embedding_bound(p))


@pytest.mark.parametrize("per_b", [1, 2047, 2049, 9 * 769])
def test_flow_loss(lib, per_b):
    B, scale = 3, 1.0 / 3
    g = kr.gen(14 + per_b)
    vf, cvf = torch.randn(B, per_b, 2, generator=g), torch.randn(B, per_b, 2, generator=g)
    loss = torch.full((B,), float("nan"), dtype=torch.float64, device="cuda")
    grad = torch.full((B, per_b, 2), float("nan"), device="cuda")
    _call("flow_loss", vf.cuda(), cvf.cuda(), loss, grad, B, per_b, scale)
    r_loss, r_grad = kr.flow_loss(vf, cvf, float(torch.tensor(scale, dtype=F32)))
    kr.hold("flow_loss", (B, per_b), loss, r_loss, 1e-6 * r_loss.abs())
    kr.hold("flow_loss_grad", (B, per_b), grad, r_grad, (2 * kr.U24 + 2.0 ** -47) * r_grad.abs())     # two roundings: (1 + u)^2 - 1
    loss2 = torch.full((B,), float("nan"), dtype=torch.float64, device="cuda")
    _call("flow_loss", vf.cuda(), cvf.cuda(), loss2, None, B, per_b, scale)
    # the same f64 sum; where several blocks add into it, in another order at the most
    assert (loss2 - loss).abs().max().item() <= 2.0 ** -50 * r_loss.abs().max().item()
    if per_b <= 2048:
        assert torch.equal(loss2, loss)


@pytest.fixture(scope="module")
def flow_pair():
    from oracle import flow_ref
    from urgent2026_challenge_track1_amd.flow_model import FlowBSRNNCore
    torch.manual_seed(21)
    ref = flow_ref.BSRNNFlow(769, 16, 1)
    with torch.no_grad():          # norms away from (1, 0)
        for n, p in ref.named_parameters():
            if "norm" in n or (".0." in n and "mlp_" in n):
                p.add_(0.1 * torch.randn_like(p))
    mine = FlowBSRNNCore(769, 16, 1, torch.float32)
    mine.load_state_dict(ref.state_dict(), strict=True)
    return ref, mine.cuda()


@pytest.mark.parametrize("F", [257, 385])
def test_flow_model_below_full_band(lib, flow_pair, F):
    """FlowBSRNNCore (N 16, 1 layer, f32) against oracle.flow_ref.BSRNNFlow with the same weights at spectra narrower than the
    band table's reach (Fs = 259 / 409 > F): output, every parameter gradient of 0.5 sum |out|^2, exact zeros for unused bands."""
    ref, mine = flow_pair
    B, T = 2, 5
    g = kr.gen(22 + F)
    x, y = torch.randn(B, T, F, 2, generator=g), torch.randn(B, T, F, 2, generator=g)
    t = torch.tensor([0.8, 0.25])
    ref.zero_grad(set_to_none=True)
    to_c = lambda a: torch.view_as_complex(a).permute(0, 2, 1)            # [B,T,F,2] -> [B,F,T] complex
    out_r = ref(torch.stack([to_c(x), to_c(y)], 1), t)[:, 0]             # [B,F,T]
    (0.5 * (out_r.abs() ** 2).sum()).backward()
    out_r = torch.view_as_real(out_r.detach().permute(0, 2, 1).contiguous())
    mine.flat_grads.zero_()          # (the parameters' .grad are views of this buffer)
    out = mine(x.cuda(), y.cuda(), t.cuda(), sign=1.0)
    (0.5 * (out ** 2).sum()).backward()
    torch.cuda.synchronize()
    sc = out_r.abs().max().item()
    err = (out.detach().cpu() - out_r).abs().max().item()
    print("flow model F %d: output err %.2e of max %.2e" % (F, err, sc))
    kr.record("flow_model_output", (B, T, F), err, 1e-3 * sc)
    assert err <= 1e-3 * sc
    refg = dict(ref.named_parameters())
    worst, unused = 0.0, 0
    for n, p in mine.named_parameters():
        if not refg[n].requires_grad:
            continue
        gr = refg[n].grad
        if gr is None:               # band not reached at this F: exactly zero
            assert torch.all(p.grad == 0), n
            unused += 1
            continue
        e = (p.grad.cpu() - gr).abs().max().item()
        worst = max(worst, e / (gr.abs().max().item() + 1e-12))
        assert e <= 2e-3 * gr.abs().max().item(), (n, e, gr.abs().max().item())
    assert unused > 0
    print("flow model F %d: worst relative grad error %.2e" % (F, worst))
    kr.record("flow_model_grads_rel", (B, T, F), worst, 2e-3)
