"""The kernel-level checks of tests/kernel_ref.py can fail: for each float64 reference, (a) a torch f32 restatement of the
same formula on the same inputs is inside the bound the GPU tests hold the kernels to, and (b) the named wrong variant
(swapped convolution axes, edge replication for the zero halo, swapped GLU halves, g*x for g*conj(x), band statistics over
the valid bins only, unbiased variance, sigma(t) with its ends swapped) is outside it.  Runs without a GPU."""
import pytest
import torch

from tests import kernel_ref as kr

F32, F64 = torch.float32, torch.float64


def _ratio(got, ref, bound):
    return kr.compare(got, ref, bound)[2]


def test_running_error_bound_on_the_5x5_convolution():
    U, W, b, _ = kr.draw_conv(2, 9, 37)
    ref, bound = kr.conv5x5(U, W, b), kr.conv5x5_bound(U, W, b)
    r = _ratio(kr.conv5x5(U, W, b, F32), ref, bound)
    print("f32 conv2d at %.4f of the running-error bound" % r)
    assert r <= 1.0
    assert _ratio(kr.conv5x5(U, W, b, F64, "swap_axes"), ref, bound) > 1e3
    assert _ratio(kr.conv5x5(U, W, b, F64, "replicate"), ref, bound) > 1e3


@pytest.mark.parametrize("shape", [(1, 3, 5), (2, 9, 37)])
def test_conv_backward_restatement_and_wrong_axes(shape):
    U, W, b, dpre = kr.draw_conv(*shape)
    zW, zb = torch.zeros_like(W), torch.zeros_like(b)
    refs = kr.conv5x5_bwd(U, W, b, dpre)
    bounds = kr.conv5x5_bwd_bounds(U, W, b, dpre, zW, zb)
    for got, ref, bd in zip(kr.conv5x5_bwd(U, W, b, dpre, F32), refs, bounds):
        assert _ratio(got, ref, bd) <= 1.0
    wrong = kr.conv5x5_bwd(U, W, b, dpre, F64, "swap_axes")
    assert _ratio(wrong[0], refs[0], bounds[0]) > 1e3 and _ratio(wrong[1], refs[1], bounds[1]) > 1e3


@pytest.mark.parametrize("sgn", [1.0, -1.0])
def test_glu_apply_restatement_and_swapped_halves(sgn):
    pm, pr, x, dout = kr.draw_glu4(10, 257, 259)
    a = kr.glu4_split(pm, 257) + kr.glu4_split(pr, 257)
    ref, bound = kr.glu_apply(*a, x, sgn), kr.glu_apply_bound(*a, x, sgn)
    assert _ratio(kr.glu_apply(*a, x, sgn, F32), ref, bound) <= 1.0
    assert _ratio(kr.glu_apply(*a, x, sgn, F64, "swap_halves"), ref, bound) > 1e3
    # the adjoint as the kernels state it against float64 autograd
    refs, bounds = kr.glu_apply_bwd(*a, x, dout, sgn), kr.glu_apply_bwd_bounds(*a, x, dout, sgn)
    for got, r, bd in zip(kr.glu_apply_bwd_formula(*a, x, dout, sgn, F32), refs, bounds):
        assert _ratio(got, r, bd) <= 1.0
    wrong = kr.glu_apply_bwd_formula(*a, x, dout, sgn, F64, "no_conj")
    assert _ratio(wrong[0], refs[0], bounds[0]) > 1e3 and _ratio(wrong[1], refs[1], bounds[1]) > 1e3
    assert _ratio(wrong[2], refs[2], bounds[2]) <= 1.0          # (the residual head does not see x)


def test_band_split_restatement_and_valid_bin_statistics():
    from urgent2026_challenge_track1_amd.bsrnn import SUBBANDS_481
    spec, gamma, beta, _ = kr.draw_spec(2, 7, 161, 2 * sum(SUBBANDS_481))
    a = (spec, SUBBANDS_481, gamma, beta, 1e-5, F32)
    (ref, stats), bound = kr.bandsplit_norm(*a), kr.bandsplit_norm_bound(*a)
    got, _ = kr.bandsplit_norm(*a, dt=F32)
    assert _ratio(got, ref, bound) <= 1.0
    wrong, _ = kr.bandsplit_norm(*a, dt=F64, wrong="valid_count")
    assert _ratio(wrong, ref, bound) > 1e3
    rows, ldx, P = kr.band_layout(SUBBANDS_481, 161, F32)
    assert len(rows) == 27 and rows[-1][1] + rows[-1][2] == 181         # the last used band sticks out by 20 bins
    # pad columns of the reference are zero
    used = torch.zeros(ldx, dtype=torch.bool)
    for k, f0, sb, xoff, _, _ in rows:
        used[xoff:xoff + 2 * sb] = True
    assert torch.all(ref[:, ~used] == 0)


def test_groupnorm_restatement_and_unbiased_variance():
    B, T, Kg, W, N = 3, 5, 1, 4 * 16, 16
    x, gamma, beta, _, add = kr.draw_groupnorm(B, T, Kg, W, N, 0)
    a = (x, gamma, beta, B, T, Kg, W, N, 0, 1e-5, add)
    ref = kr.groupnorm(*a)
    assert (kr.groupnorm(*a, dt=F32).double() - ref).abs().max().item() <= 2e-5
    assert (kr.groupnorm(*a, dt=F64, wrong="unbiased") - ref).abs().max().item() > 1e-3


def test_flow_prepare_restatement_and_swapped_sigma():
    x0, y, z = kr.draw_flow_state(3, 1031)
    t = torch.tensor([0.0, 1.0, 0.37])
    refs = kr.flow_prepare(x0, y, z, t, 1031, 0.05, 0.5)
    bounds = kr.flow_prepare_bounds(x0, y, z, t, 0.05, 0.5)
    for got, r, bd in zip(kr.flow_prepare(x0, y, z, t, 1031, 0.05, 0.5, F32), refs, bounds):
        assert _ratio(got, r, bd) <= 1.0
    wrong = kr.flow_prepare(x0, y, z, t, 1031, 0.05, 0.5, F64, "swap_sigma")
    assert _ratio(wrong[0], refs[0], bounds[0]) > 1e3 and _ratio(wrong[1], refs[1], bounds[1]) > 1e3


@pytest.mark.parametrize("exponent,factor", [(0.667, 0.065), (1.0, 0.065)])
def test_spec_transform_restatement_and_round_trip(exponent, factor):
    x = kr.draw_complex_logmag(4099)
    for inverse in (0, 1):
        ref = kr.spec_transform(x, exponent, factor, inverse)
        rel = kr.spec_transform_rel(x, exponent, factor, inverse)
        assert _ratio(kr.spec_transform(x, exponent, factor, inverse, F32), ref, rel * ref.abs()) <= 1.0
        assert torch.all(ref[4099 // 2] == 0)
    fwd = kr.spec_transform(x, exponent, factor, 0)
    assert (kr.spec_transform(fwd, exponent, factor, 1) - x.double()).abs().max().item() <= 1e-12 * 1e2


def test_time_embedding_and_tanh_restatements():
    g = kr.gen(5)
    t, W = 0.03 + 0.97 * torch.rand(3, generator=g), torch.randn(192, generator=g)
    ref, p = kr.time_embedding(t, W)
    assert _ratio(kr.time_embedding(t, W, F32)[0], ref, kr.time_embedding_bound(p)) <= 1.0
    U, _, _, _ = kr.draw_conv(1, 5, 259)
    dU = torch.randn(U.shape, generator=g)
    assert _ratio(kr.tanh_bwd(dU, U, F32), kr.tanh_bwd(dU, U), kr.tanh_bwd_bound(dU, U, F32)) <= 1.0


def test_compare_rejects_nan_and_nonzero_on_a_zero_bound():
    ref = torch.zeros(4, dtype=F64)
    assert kr.compare(torch.tensor([0.0, 0.0, 1e-30, 0.0]), ref, torch.zeros(4))[2] == float("inf")
    assert kr.compare(torch.tensor([0.0, float("nan"), 0.0, 0.0]), ref, torch.ones(4))[2] == float("inf")
    assert kr.compare(torch.zeros(4), ref, torch.zeros(4))[2] == 0.0


def test_band_tables_refuse_a_band_the_affine_backward_cannot_cover():
    """bandsplit_bwd_affine_kernel runs 128 threads, one per (re, im) column of a band: 2 * sb <= 128."""
    from urgent2026_challenge_track1_amd.bsrnn import BSRNNCore, SUBBANDS_481, SUBBANDS_769
    cpu = torch.device("cpu")
    for dim, sub in ((481, SUBBANDS_481), (769, SUBBANDS_769)):
        core = BSRNNCore(dim, 16, 1, compute_dtype=torch.float32)
        assert core.subbands == sub and max(sub) <= 64
        tb = core._band_tables(dim, torch.float32, cpu)
        assert tb["K"] == len(sub)
        rows, ldx, P = kr.band_layout(sub, dim, torch.float32)
        assert (tb["ldx"], tb["P"]) == (ldx, P)
        assert [r[:3] + [r[5]] for r in tb["rows"]] == [[f0, sb, xoff, poff] for _, f0, sb, xoff, poff, _ in rows]
    core.subbands = (5, 4, 70, 10)
    core._tables.clear()
    with pytest.raises(ValueError, match="64"):
        core._band_tables(89, torch.float32, cpu)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_16bit_term_is_the_unit_roundoff(dtype):
    """torch's own round-to-nearest of the f32 restatement misses 2^-9 |ref| (bf16) / 2^-12 |ref| (f16) and meets the unit
    roundoff 2^-8 / 2^-11, which stays inside four times the measured figure (kernel_ref's docstring quotes the numbers)."""
    from urgent2026_challenge_track1_amd.bsrnn import SUBBANDS_481
    spec, gamma, beta, _ = kr.draw_spec(2, 7, 161, 2 * sum(SUBBANDS_481))
    a = (spec, SUBBANDS_481, gamma, beta, 1e-5, dtype)
    ref, _ = kr.bandsplit_norm(*a)
    b32 = kr.bandsplit_norm_bound(*a)
    got = kr.bandsplit_norm(*a, dt=F32)[0].to(dtype)
    measured = _ratio(got, ref, kr.ISSUE_OUT16[dtype] * ref.abs() + (2.0 ** -25 if dtype == torch.float16 else 0.0) + b32)
    print("%s: f32 restatement rounded by torch at %.3f of the issue's term" % (dtype, measured))
    assert 1.0 < measured <= 2.0
    assert _ratio(got, ref, kr.out16(ref, dtype, b32)) <= 1.0
    assert kr.UNIT_OUT16[dtype] <= 4 * measured * kr.ISSUE_OUT16[dtype]
    wrong = kr.bandsplit_norm(*a, dt=F64, wrong="valid_count")[0]
    assert _ratio(wrong, ref, kr.out16(ref, dtype, b32)) > 10
