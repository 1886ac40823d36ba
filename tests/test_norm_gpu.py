"""GPU parity: GroupNorm forward / backward kernels against torch autograd on the same normalisation
(statistics over (T, W) per (batch, group), per-channel affine repeating every N columns): f32 and bf16 output, the flow
model's additive term, the residual gradient, the packed bf16 copy, the flow width N = 384 (64 idle threads per block), a
backward reduce split over several row chunks, and the stats= / sums= entry points.
Out of scope: the scalar reduce kernel (gn_bwd_reduce_kernel) runs only under URSE_GN_REDUCE1, which the library reads once
per process - a test in this process cannot switch it on."""
import pytest
import torch

from tests import kernel_ref as kr

pytestmark = pytest.mark.gpu


def _ref(x, gamma, beta, B, T, Kg, W, N, gstride, eps):
    xr = x.double().reshape(B, T, Kg, W)
    mean = xr.mean(dim=(1, 3), keepdim=True)
    var = xr.var(dim=(1, 3), unbiased=False, keepdim=True)
    xh = (xr - mean) / torch.sqrt(var + eps)
    g = torch.stack([gamma[k * gstride:k * gstride + N] for k in range(Kg)]).double()      # [Kg, N]
    b = torch.stack([beta[k * gstride:k * gstride + N] for k in range(Kg)]).double()
    y = xh.reshape(B, T, Kg, W // N, N) * g[None, None, :, None, :] + b[None, None, :, None, :]
    return y.reshape(B, T, Kg, W)


@pytest.mark.parametrize("B,T,Kg,W,N,gstride", [(2, 37, 1, 5 * 196, 196, 0), (3, 21, 4, 196, 196, 196), (2, 19, 3, 2 * 20, 20, 20),
                                                 (2, 11, 2, 3 * 12, 12, 12)])
def test_groupnorm_fwd_bwd_matches_autograd(lib, B, T, Kg, W, N, gstride):
    from urgent2026_challenge_track1_amd import ops
    g = torch.Generator().manual_seed(B * 100 + T)
    x = torch.randn(B, T, Kg, W, generator=g)
    ng = max(1, Kg if gstride else 1) * max(N, gstride)
    gamma = (1 + 0.3 * torch.randn(ng, generator=g)).requires_grad_()
    beta = (0.2 * torch.randn(ng, generator=g)).requires_grad_()
    dy = torch.randn(B, T, Kg, W, generator=g)
    xr = x.clone().requires_grad_()
    y_ref = _ref(xr, gamma, beta, B, T, Kg, W, N, gstride, 1e-5)
    y_ref.backward(dy.double())
    xc, gc, bc = x.cuda(), gamma.detach().cuda(), beta.detach().cuda()
    y, stats = ops.groupnorm_fwd(xc, gc, bc, B, T, Kg, W, N, N, gstride, torch.float32, 1e-5)
    assert (y.cpu().double().reshape(B, T, Kg, W) - y_ref.detach()).abs().max().item() <= 2e-5
    dgam, dbet = torch.zeros_like(gc), torch.zeros_like(bc)
    dx = ops.groupnorm_bwd(xc, dy.cuda(), stats, gc, None, dgam, dbet, B, T, Kg, W, N, gstride, 1e-5)
    assert (dx.cpu().double() - xr.grad.double()).abs().max().item() <= 5e-5 * max(1.0, xr.grad.abs().max().item())
    assert (dgam.cpu().double() - gamma.grad.double()).abs().max().item() <= 1e-4 * max(1.0, gamma.grad.abs().max().item())
    assert (dbet.cpu().double() - beta.grad.double()).abs().max().item() <= 1e-4 * max(1.0, beta.grad.abs().max().item())


# ---- cases the flow model and the training step reach (same float64 reference, same tolerances) --------------------------
FWD_TOL, DX_TOL, AFF_TOL = 2e-5, 5e-5, 1e-4


def _check_fwd(name, shape, y, ref, N, Np, dtype=torch.float32):
    y = y.cpu().reshape(-1, Np)
    assert torch.all(y[:, N:] == 0)                                   # pad channels exactly zero
    ref = ref.reshape(-1, N)
    kr.hold(name, shape, y[:, :N], ref, kr.out16(ref, dtype, FWD_TOL))


def _check_bwd(name, shape, dx, dgam, dbet, dx_ref, gamma, beta):
    for tag, got, ref, tol in (("dx", dx, dx_ref, DX_TOL), ("dgamma", dgam, gamma.grad, AFF_TOL), ("dbeta", dbet, beta.grad, AFF_TOL)):
        kr.hold("%s_%s" % (name, tag), shape, got, ref.double(), torch.full_like(ref, tol * max(1.0, ref.abs().max().item()), dtype=torch.float64))


@pytest.mark.parametrize("W,N,Np", [(4 * 384, 384, 384), (4 * 16, 16, 32)])
def test_groupnorm_fwd_additive_term(lib, W, N, Np):
    """y = GN(x) + add[b, c]: the time embedding the flow model adds after norm_time."""
    from urgent2026_challenge_track1_amd import ops
    B, T, Kg = 3, 5, 1
    x, gamma, beta, _, add = kr.draw_groupnorm(B, T, Kg, W, N, 0)
    ref = kr.groupnorm(x, gamma, beta, B, T, Kg, W, N, 0, 1e-5, add)
    y, _ = ops.groupnorm_fwd(x.cuda(), gamma.cuda(), beta.cuda(), B, T, Kg, W, N, Np, 0, torch.float32, 1e-5, add=add.cuda())
    _check_fwd("groupnorm_fwd_add", (B, T, Kg, W, N, Np), y, ref, N, Np)
    assert (kr.groupnorm(x, gamma, beta, B, T, Kg, W, N, 0, 1e-5) - ref).abs().max().item() > 100 * FWD_TOL       # (the term matters)


def test_groupnorm_fwd_bf16_padded(lib):
    from urgent2026_challenge_track1_amd import ops
    B, T, Kg, W, N, Np = 2, 9, 3, 2 * 196, 196, 224
    x, gamma, beta, _, _ = kr.draw_groupnorm(B, T, Kg, W, N, N)
    ref = kr.groupnorm(x, gamma, beta, B, T, Kg, W, N, N, 1e-5)
    y, _ = ops.groupnorm_fwd(x.cuda(), gamma.cuda(), beta.cuda(), B, T, Kg, W, N, Np, N, torch.bfloat16, 1e-5)
    assert y.dtype == torch.bfloat16
    _check_fwd("groupnorm_fwd_bf16", (B, T, Kg, W, N, Np), y, ref, N, Np, torch.bfloat16)


def _bwd_case(B, T, Kg, W, N, gstride, with_dres):
    x, gamma, beta, dy, _ = kr.draw_groupnorm(B, T, Kg, W, N, gstride)
    gamma, beta = gamma.requires_grad_(), beta.requires_grad_()
    xr = x.clone().requires_grad_()
    y_ref = kr.groupnorm(xr, gamma, beta, B, T, Kg, W, N, gstride, 1e-5)
    y_ref.backward(dy.double())
    dres = torch.randn(x.shape, generator=kr.gen(B + T)) if with_dres else None
    dx_ref = xr.grad.double() + (dres.double() if with_dres else 0)
    return x, gamma, beta, dy, dres, y_ref.detach(), dx_ref


def test_groupnorm_bwd_residual_and_packed_copy(lib):
    """dres is the residual gradient added into dx; pack_ld: dx once more in bf16, rows zero-padded to pack_ld columns."""
    from urgent2026_challenge_track1_amd import ops
    B, T, Kg, W, N, ld = 2, 11, 1, 3 * 196, 196, 224
    x, gamma, beta, dy, dres, _, dx_ref = _bwd_case(B, T, Kg, W, N, 0, True)
    xc, gc, bc = x.cuda(), gamma.detach().cuda(), beta.detach().cuda()
    _, stats = ops.groupnorm_fwd(xc, gc, bc, B, T, Kg, W, N, N, 0, torch.float32, 1e-5)
    dgam, dbet = torch.zeros_like(gc), torch.zeros_like(bc)
    dx, dxp = ops.groupnorm_bwd(xc, dy.cuda(), stats, gc, dres.cuda(), dgam, dbet, B, T, Kg, W, N, 0, 1e-5, pack_ld=ld)
    _check_bwd("groupnorm_bwd_dres", (B, T, Kg, W, N), dx, dgam, dbet, dx_ref, gamma, beta)
    assert dxp.shape == (B * T * Kg * (W // N), ld) and dxp.dtype == torch.bfloat16
    assert torch.equal(dxp[:, :N].contiguous().view(torch.int16), dx.reshape(-1, N).to(torch.bfloat16).view(torch.int16))
    assert torch.all(dxp[:, N:] == 0)


def test_groupnorm_bwd_reduce_split_over_row_chunks(lib):
    """T * W = 319,872 > 262,144: two workgroups per group share the reduce pass and meet in the atomics."""
    from urgent2026_challenge_track1_amd import ops
    B, T, Kg, W, N = 1, 48, 1, 34 * 196, 196
    x, gamma, beta, dy, _, y_ref, dx_ref = _bwd_case(B, T, Kg, W, N, 0, False)
    xc, gc, bc = x.cuda(), gamma.detach().cuda(), beta.detach().cuda()
    y, stats = ops.groupnorm_fwd(xc, gc, bc, B, T, Kg, W, N, N, 0, torch.float32, 1e-5)
    _check_fwd("groupnorm_fwd", (B, T, Kg, W, N, N), y, y_ref, N, N)
    dgam, dbet = torch.zeros_like(gc), torch.zeros_like(bc)
    dx = ops.groupnorm_bwd(xc, dy.cuda(), stats, gc, None, dgam, dbet, B, T, Kg, W, N, 0, 1e-5)
    _check_bwd("groupnorm_bwd_split", (B, T, Kg, W, N), dx, dgam, dbet, dx_ref, gamma, beta)


def test_groupnorm_flow_width_bwd(lib):
    """N = 384: 256 / (N / 4) leaves 64 idle threads per block in the apply and reduce kernels."""
    from urgent2026_challenge_track1_amd import ops
    B, T, Kg, W, N = 3, 5, 1, 4 * 384, 384
    x, gamma, beta, dy, dres, _, dx_ref = _bwd_case(B, T, Kg, W, N, 0, True)
    xc, gc, bc = x.cuda(), gamma.detach().cuda(), beta.detach().cuda()
    _, stats = ops.groupnorm_fwd(xc, gc, bc, B, T, Kg, W, N, N, 0, torch.float32, 1e-5)
    dgam, dbet = torch.zeros_like(gc), torch.zeros_like(bc)
    dx = ops.groupnorm_bwd(xc, dy.cuda(), stats, gc, dres.cuda(), dgam, dbet, B, T, Kg, W, N, 0, 1e-5)
    _check_bwd("groupnorm_bwd_n384", (B, T, Kg, W, N), dx, dgam, dbet, dx_ref, gamma, beta)


def test_groupnorm_stats_and_sums_entry_points(lib):
    """statistics and backward sums that exist already (the GEMM epilogues produce them in the training step): only the apply
    passes run, and give the fused entry points' results bit for bit."""
    from urgent2026_challenge_track1_amd import ops
    from urgent2026_challenge_track1_amd._lib import call, stream_ptr
    B, T, Kg, W, N, Np = 2, 37, 1, 5 * 196, 196, 224
    x, gamma, beta, dy, _ = kr.draw_groupnorm(B, T, Kg, W, N, 0)
    xc, gc, bc, dyc = x.cuda(), gamma.cuda(), beta.cuda(), dy.cuda()
    y, stats = ops.groupnorm_fwd(xc, gc, bc, B, T, Kg, W, N, Np, 0, torch.float32, 1e-5)
    st2 = torch.zeros(B * Kg * 2, dtype=torch.float64, device="cuda")
    call("groupnorm_stats", xc, st2, B, T, Kg, W, N, stream_ptr())
    assert torch.equal(st2, stats)
    y2, _ = ops.groupnorm_fwd(xc, gc, bc, B, T, Kg, W, N, Np, 0, torch.float32, 1e-5, stats=st2)
    assert torch.equal(y2, y)
    dgam, dbet = torch.zeros_like(gc), torch.zeros_like(bc)
    dx = torch.full_like(xc, float("nan"))
    sums = torch.full((B * Kg * 2,), float("nan"), dtype=torch.float64, device="cuda")
    call("groupnorm_bwd", xc, dyc, stats, gc, None, dx, dgam, dbet, sums, B, T, Kg, W, N, 0, 1e-5, None, 0, stream_ptr())
    dx2 = ops.groupnorm_bwd(xc, dyc, stats, gc, None, None, None, B, T, Kg, W, N, 0, 1e-5, sums=sums)
    assert not torch.isnan(dx).any() and torch.equal(dx2, dx)
