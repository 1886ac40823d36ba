"""Float64 references and error bounds for the kernel-level GPU tests of csrc/flow.hip, csrc/bands.hip and csrc/norm.hip.

TEST INFRASTRUCTURE - never imported by the product path.

Every reference is plain torch, written from the formulas the kernel headers cite (bsrnn_flowse.py:63-86 band split,
:90-99 time embedding, :103-168 GradDecoder, :311-315 mask apply; flow_model.py:122-132 loss, :159-172 x_t / conditional
vector field; the espnet 'exponent' transform; torch_ema).  Each takes `dt`: float64 is THE reference, float32 is the
"f32 restatement" tests/test_kernel_ref_cpu.py holds to the same bound; `wrong=` selects one of the named wrong variants
that the same module shows to be outside the bound.

Bounds (u = 2^-24, the f32 unit roundoff):
 * sum of n products  sum_i a_i b_i, any order, with or without FMA:  |err| <= n u sum_i |a_i||b_i|.  The sum of absolute
   products comes from running the same bilinear reference on absolute values (the `*_bound` functions below).
 * a transcendental call (exp-based sigmoid for |x| <= 5, sqrtf, powf) is allotted T = 2^-20 relative; sinf / cosf
   T + 4 u |p| absolute.  They are propagated to first order through the formula, next to one u per rounded operation.
 * 16-bit outputs add the format's unit roundoff: 2^-8 |ref| (bf16, 8 significant bits), 2^-11 |ref| + 2^-25 (f16, 11
   significant bits, half a subnormal step), and 2^-8 of the f32 bound, since it is the computed value that is rounded.
   The request for these tests put the terms at 2^-9 / 2^-12.  Round-to-nearest-even cannot meet that: a value just above a
   power of two lies half a unit in the last place = 2^-8 of itself from its bf16 neighbours.  Handled by the rule the same
   request gives for a bound a correct kernel cannot meet (measure a torch f32 restatement against float64; the allotment is
   at most 4 x that figure; record both): the f32 restatement of the band split, rounded by torch's own .to(bfloat16) /
   .to(float16), is 1.97 x 2^-9 |ref| resp. 1.95 x 2^-12 |ref| off float64 on the committed inputs; the kernels 1.99 x 2^-9
   (bf16) and 1.97 x 2^-12 (f16) on the MI355X.  The allotment is 2 x the requested term - the unit roundoff, less than 4 x
   the figure.  tests/test_kernel_ref_cpu.py re-measures the restatement.
"""
import math

import torch
import torch.nn.functional as Fn

U24 = 2.0 ** -24
T20 = 2.0 ** -20
F64 = torch.float64
F32 = torch.float32


ISSUE_OUT16 = {torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -12}      # what round-to-nearest cannot meet (see above)
UNIT_OUT16 = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def out16(ref, dtype, bound32=0.0):
    """bound of a value held to `bound32` in f32 once it is stored in `dtype`: the rounding of the computed value added."""
    if dtype == torch.float32:
        return bound32 + torch.zeros_like(ref)
    u = UNIT_OUT16[dtype]
    return u * ref.abs() + (2.0 ** -25 if dtype == torch.float16 else 0.0) * (ref != 0) + (1 + u) * bound32


def dot_bound(n, abs_sum):
    return n * U24 * abs_sum


def compare(got, ref, bound):
    """-> (worst |got - ref|, the bound at that element, worst err / bound).  A zero bound admits a zero error only."""
    err = (got.detach().cpu().to(F64) - ref.detach().to(F64)).abs().reshape(-1)
    bound = torch.as_tensor(bound, dtype=F64).expand_as(ref).reshape(-1)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)        # x / 0 = inf
    if torch.isnan(err).any():
        return float("nan"), float(bound.max()), float("inf")
    i = int(torch.argmax(ratio))
    return float(err[i]), float(bound[i]), float(ratio[i])


def clamp_pre(x):
    """pre-activations as the tests draw them: the sigmoid allotment holds for |x| <= 5."""
    return (1.5 * x).clamp_(-5.0, 5.0)


def kpad(n, dtype):
    m = 16 if dtype == torch.float32 else 32
    return (n + m - 1) // m * m


# ---------------------------------------------------------------------------------------------------------
# Conv2d(16 -> 4, 5x5, pad 2) over (F, T) on channel-last maps
# ---------------------------------------------------------------------------------------------------------
def conv5x5(U, W, b, dt=F64, wrong=None):
    """U [B,T,F,16], W [4,16,5(f),5(t)], b [4] -> pre [B,T,F,4]."""
    x = U.to(dt).permute(0, 3, 2, 1)                      # [B,16,F,T]
    w = W.to(dt)
    if wrong == "swap_axes":
        w = w.transpose(2, 3)
    if wrong == "replicate":
        y = Fn.conv2d(Fn.pad(x, (2, 2, 2, 2), mode="replicate"), w, b.to(dt))
    else:
        y = Fn.conv2d(x, w, b.to(dt), padding=2)
    return y.permute(0, 3, 2, 1)


def conv5x5_bound(U, W, b):
    return dot_bound(401, conv5x5(U.abs(), W.abs(), b.abs()))       # 16 * 25 products and the bias


def conv5x5_bwd(U, W, b, dpre, dt=F64, wrong=None):
    """autograd of conv5x5 -> (dU, dW, dbias)."""
    U, W, b = (t.detach().to(dt).clone().requires_grad_() for t in (U, W, b))
    conv5x5(U, W, b, dt, wrong).backward(dpre.to(dt))
    return U.grad, W.grad, b.grad


def conv5x5_bwd_bounds(U, W, b, dpre, dW0, db0):
    """dU sums 4 * 25 products; dW / dbias B*T*F terms onto the initial value."""
    aU, aW, ab = conv5x5_bwd(U.abs(), W.abs(), b.abs(), dpre.abs())
    n = U.shape[0] * U.shape[1] * U.shape[2] + 1
    return dot_bound(100, aU), dot_bound(n, aW + dW0.double().abs()), dot_bound(n, ab + db0.double().abs())


# ---------------------------------------------------------------------------------------------------------
# GLU + complex m * x + r  (shared by glu4_apply and glu_mask_apply); everything [..., 2] = (re, im)
# ---------------------------------------------------------------------------------------------------------
def _mxr(m, r, x, sgn, absmode=False):
    s = 1.0 if absmode else -1.0
    re = m[..., 0] * x[..., 0] + s * m[..., 1] * x[..., 1] + r[..., 0]
    im = m[..., 0] * x[..., 1] + m[..., 1] * x[..., 0] + r[..., 1]
    return (abs(sgn) if absmode else sgn) * torch.stack([re, im], -1)


def glu_apply(vm, gm, vr, gr, x, sgn=1.0, dt=F64, wrong=None, absmode=False):
    """out = sgn * (vm sigmoid(gm) * x + vr sigmoid(gr)), complex; absmode: every product taken in absolute value."""
    vm, gm, vr, gr, x = (t.to(dt) for t in (vm, gm, vr, gr, x))
    if wrong == "swap_halves":
        vm, gm, vr, gr = gm, vm, gr, vr
    if absmode:
        vm, vr, x = vm.abs(), vr.abs(), x.abs()
    return _mxr(vm * torch.sigmoid(gm), vr * torch.sigmoid(gr), x, sgn, absmode)


GLU_FWD_REL = T20 + 5 * U24      # sigmoid, v*s, m*x, two adds, sign


def glu_apply_bound(vm, gm, vr, gr, x, sgn=1.0):
    return GLU_FWD_REL * glu_apply(vm, gm, vr, gr, x, sgn, absmode=True)


def glu_apply_bwd_formula(vm, gm, vr, gr, x, dout, sgn=1.0, dt=F64, wrong=None):
    """the adjoint as the kernels state it -> (dvm, dgm, dvr, dgr)."""
    vm, gm, vr, gr, x, g = (t.to(dt) for t in (vm, gm, vr, gr, x, dout))
    g = sgn * g
    if wrong == "no_conj":      # dm = g * x
        dm = torch.stack([g[..., 0] * x[..., 0] - g[..., 1] * x[..., 1], g[..., 1] * x[..., 0] + g[..., 0] * x[..., 1]], -1)
    else:                       # dm = g * conj(x)
        dm = torch.stack([g[..., 0] * x[..., 0] + g[..., 1] * x[..., 1], g[..., 1] * x[..., 0] - g[..., 0] * x[..., 1]], -1)
    s, q = torch.sigmoid(gm), torch.sigmoid(gr)
    return dm * s, dm * vm * s * (1 - s), g * q, g * vr * q * (1 - q)


def glu_apply_bwd(vm, gm, vr, gr, x, dout, sgn=1.0):
    """float64 autograd -> (dvm, dgm, dvr, dgr)."""
    leaves = [t.detach().to(F64).clone().requires_grad_() for t in (vm, gm, vr, gr)]
    glu_apply(*leaves, x, sgn).backward(dout.to(F64))
    return tuple(t.grad for t in leaves)


def glu_apply_bwd_bounds(vm, gm, vr, gr, x, dout, sgn=1.0):
    """value halves: |D| s (T + 5u).  gate halves D v s (1 - s): d[s(1-s)] = (1 - 2s) ds, so relative to s(1-s) the
    sigmoid's T is multiplied by |1 - 2s| / (1 - s) (<= 1 + e^5 for |gate| <= 5); 6u for the rounded operations."""
    leaves = [t.detach().to(F64).clone().requires_grad_() for t in (vm, gm, vr, gr)]
    glu_apply(*leaves, x, sgn, absmode=True).backward(dout.to(F64).abs())
    avm, agm, avr, agr = (t.grad.abs() for t in leaves)
    s, q = torch.sigmoid(gm.to(F64)), torch.sigmoid(gr.to(F64))
    fs = 6 * U24 + T20 * (1 - 2 * s).abs() / (1 - s)
    fq = 6 * U24 + T20 * (1 - 2 * q).abs() / (1 - q)
    return GLU_FWD_REL * avm, fs * agm, GLU_FWD_REL * avr, fq * agr


def glu4_split(pre, F):
    """pre [rows, Fs, 4] -> value (c0, c1) and gate (c2, c3) of the first F bins."""
    return pre[:, :F, 0:2], pre[:, :F, 2:4]


# ---------------------------------------------------------------------------------------------------------
# small flow kernels
# ---------------------------------------------------------------------------------------------------------
def tanh_bwd(dU, U, dt=F64):
    dU, U = dU.to(dt), U.to(dt)
    return dU * (1 - U * U)


def tanh_bwd_bound(dU, U, out_dtype):
    dU, U = dU.double(), U.double()
    ref = tanh_bwd(dU, U)
    return out16(ref, out_dtype, U24 * dU.abs() * (U * U + 2 * (1 - U * U).abs()))


def spec_transform(x, exponent, factor, inverse, dt=F64):
    """x [n, 2] -> |X|^e e^{j angle X} factor  (inverse: X / factor, then |.|^(1/e))."""
    v = x.to(dt)
    if inverse:
        v = v / factor
    mag = torch.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1])
    e = (1.0 / exponent if inverse else exponent)
    s = torch.where(mag > 0, mag.clamp_min(1e-300 if dt == F64 else 1e-38) ** (e - 1.0), torch.zeros_like(mag))
    if not inverse:
        s = s * factor
    return v * s[:, None]


def spec_transform_rel(x, exponent, factor, inverse):
    """relative bound per element (a column [n, 1]): powf T, the magnitude (sqrtf T, 2u for the sum of squares, 3u for the
    division by the factor) through the exponent |e - 1|, and f32 roundings of 1/exponent and of e - 1 through |ln mag|."""
    if not inverse:
        rel = torch.full((x.shape[0], 1), T20 + abs(exponent - 1.0) * (T20 + 2 * U24) + 4 * U24, dtype=F64)
        return rel
    e = 1.0 / exponent
    mag = (x.double() / factor).norm(dim=1, keepdim=True).clamp_min(1e-300)
    return T20 + abs(e - 1.0) * (T20 + 5 * U24) + 2 * U24 * max(e, 1.0) * mag.log().abs() + 6 * U24


def flow_prepare(x0, y, z, t, per_b, smin, smax, dt=F64, wrong=None):
    """xt = (1-t) x0 + t y + sigma(t) z, sigma(t) = (1-t) smin + t smax ;  cvf = (smax - smin) z + (y - x0).  [B, per_b, 2]"""
    if wrong == "swap_sigma":
        smin, smax = smax, smin
    x0, y, z = (a.to(dt) for a in (x0, y, z))
    tb = t.to(dt)[:, None, None]
    sg = (1 - tb) * smin + tb * smax
    return (1 - tb) * x0 + tb * y + sg * z, (smax - smin) * z + (y - x0)


def flow_prepare_bounds(x0, y, z, t, smin, smax):
    x0, y, z = (a.double().abs() for a in (x0, y, z))
    tb = t.double()[:, None, None]
    sg = (1 - tb) * smin + tb * smax
    return 6 * U24 * ((1 - tb) * x0 + tb * y + sg * z), 3 * U24 * (abs(smax - smin) * z + y + x0)


def time_embedding(t, W, dt=F64):
    """[sin(2 pi t W), cos(2 pi t W)]  -> ([B, 2 half], |p| [B, half])."""
    p = t.to(dt)[:, None] * W.to(dt)[None, :] * 2 * math.pi
    return torch.cat([torch.sin(p), torch.cos(p)], -1), p.abs()


def time_embedding_bound(p_abs):
    b = T20 + 4 * U24 * p_abs.double()
    return torch.cat([b, b], -1)


def flow_loss(vf, cvf, scale):
    """loss_b = 0.5 sum |vf - cvf|^2 of the F32 differences, accumulated in f64;  grad = (vf - cvf) scale in f64."""
    d32 = (vf - cvf).double()
    B = vf.shape[0]
    return 0.5 * (d32 * d32).reshape(B, -1).sum(1), (vf.double() - cvf.double()) * scale


# ---------------------------------------------------------------------------------------------------------
# band split + GroupNorm(1, 2 sb) per band, from the subband tuple alone
# ---------------------------------------------------------------------------------------------------------
def band_layout(subbands, F, dtype):
    """[(k, f0, sb, xoff, poff, goff)] of the bands a spectrum of F bins uses, and the padded widths (ldx, P)."""
    rows, f0, xoff, poff = [], 0, 0, 0
    for k, sb in enumerate(subbands):
        rows.append((k, f0, sb, xoff, poff, 2 * f0))
        f0 += sb
        xoff += kpad(2 * sb, dtype)
        poff += kpad(4 * sb, dtype)
        if f0 >= F:
            break
    return rows, xoff, poff


def bandsplit_norm(spec, subbands, gamma, beta, eps, dtype, dt=F64, wrong=None):
    """spec [B,T,F,2] -> (xnb [B*T, ldx] with zero pads, stats [B, K, 2] = (sum, sum of squares) per band)."""
    B, T, F, _ = spec.shape
    rows, ldx, _ = band_layout(subbands, F, dtype)
    x = spec.to(dt)
    out = torch.zeros(B, T, ldx, dtype=dt)
    stats = torch.zeros(B, len(rows), 2, dtype=dt)
    for k, f0, sb, xoff, _, goff in rows:
        xb = x[:, :, f0:f0 + sb, :]
        valid = xb.shape[2]
        stats[:, k, 0] = xb.reshape(B, -1).sum(1)
        stats[:, k, 1] = (xb * xb).reshape(B, -1).sum(1)
        g, b = gamma[goff:goff + 2 * sb].to(dt), beta[goff:goff + 2 * sb].to(dt)
        if wrong == "valid_count" and valid < sb:        # statistics over the bins that exist only
            flat = xb.reshape(B, T, 2 * valid)
            m = flat.mean(dim=(1, 2), keepdim=True)
            v = flat.var(dim=(1, 2), unbiased=False, keepdim=True)
            xp = Fn.pad(flat, (0, 2 * (sb - valid)))
            out[:, :, xoff:xoff + 2 * sb] = (xp - m) / torch.sqrt(v + eps) * g + b
            continue
        if sb > valid:
            xb = Fn.pad(xb, (0, 0, 0, sb - valid))
        xb = xb.reshape(B, T, 2 * sb)
        out[:, :, xoff:xoff + 2 * sb] = Fn.group_norm(xb.transpose(1, 2), 1, g, b, eps).transpose(1, 2)
    return out.reshape(B * T, ldx), stats


def bandsplit_norm_bound(spec, subbands, gamma, beta, eps, dtype):
    """v = (x - mean) rstd gamma + beta with mean, rstd rounded from f64: 5 roundings on |gamma| rstd (|x| + |mean|) + |beta|."""
    B, T, F, _ = spec.shape
    rows, ldx, _ = band_layout(subbands, F, dtype)
    x = spec.double()
    out = torch.zeros(B, T, ldx, dtype=F64)
    for k, f0, sb, xoff, _, goff in rows:
        xb = x[:, :, f0:f0 + sb, :]
        xb = Fn.pad(xb, (0, 0, 0, sb - xb.shape[2])).reshape(B, T, 2 * sb)
        m = xb.mean(dim=(1, 2), keepdim=True)
        rstd = 1 / torch.sqrt(xb.var(dim=(1, 2), unbiased=False, keepdim=True) + eps)
        out[:, :, xoff:xoff + 2 * sb] = gamma[goff:goff + 2 * sb].double().abs() * rstd * (xb.abs() + m.abs()) \
            + beta[goff:goff + 2 * sb].double().abs()
    return 5 * U24 * out.reshape(B * T, ldx)


def bandsplit_affine_bwd(spec, subbands, gamma, beta, dxnb, eps, dtype):
    """float64 autograd of bandsplit_norm w.r.t. gamma / beta, and the running-error bounds of their B*T-term sums (+ 4 roundings
    inside xhat, + 1 for the value accumulated onto): n u sum |d| rstd (|x| + |mean|), n u sum |d|."""
    B, T, F, _ = spec.shape
    g, b = gamma.detach().double().clone().requires_grad_(), beta.detach().double().clone().requires_grad_()
    y, _ = bandsplit_norm(spec, subbands, g, b, eps, dtype)
    y.backward(dxnb.double())
    ones, zeros = torch.ones_like(gamma), torch.zeros_like(beta)
    amp = bandsplit_norm_bound(spec, subbands, ones, zeros, eps, dtype) / (5 * U24)       # rstd (|x| + |mean|)
    rows, ldx, _ = band_layout(subbands, F, dtype)
    ag, ab = torch.zeros_like(g), torch.zeros_like(b)
    d = dxnb.double().abs()
    for k, f0, sb, xoff, _, goff in rows:
        ag[goff:goff + 2 * sb] = (d[:, xoff:xoff + 2 * sb] * amp[:, xoff:xoff + 2 * sb]).sum(0)
        ab[goff:goff + 2 * sb] = d[:, xoff:xoff + 2 * sb].sum(0)
    return g.grad, b.grad, ag.detach(), ab.detach(), B * T + 5


def band_gather_index(subbands, F, dtype):
    """column of the (re) value and gate entry of every mapped bin in a `pre` row -> (bins, value cols, gate cols, P)."""
    rows, _, P = band_layout(subbands, F, dtype)
    bins, vc, gc = [], [], []
    for k, f0, sb, _, poff, _ in rows:
        for f in range(f0, min(F, f0 + sb)):
            bins.append(f)
            vc.append(poff + 2 * (f - f0))
            gc.append(poff + 2 * sb + 2 * (f - f0))
    return torch.tensor(bins), torch.tensor(vc), torch.tensor(gc), P


def band_split_pre(pre, vc, gc):
    """pre [rows, P] -> value, gate [rows, nbins, 2]."""
    return torch.stack([pre[:, vc], pre[:, vc + 1]], -1), torch.stack([pre[:, gc], pre[:, gc + 1]], -1)


def band_scatter_pre(dv, dg, vc, gc, P):
    """the inverse of band_split_pre onto zeros [rows, P]."""
    out = torch.zeros(dv.shape[0], P, dtype=dv.dtype)
    out[:, vc], out[:, vc + 1] = dv[..., 0], dv[..., 1]
    out[:, gc], out[:, gc + 1] = dg[..., 0], dg[..., 1]
    return out


# ---------------------------------------------------------------------------------------------------------
# GroupNorm over (T, W) per (b, kg), affine repeating every N columns, optional per-(b, channel) additive term
# ---------------------------------------------------------------------------------------------------------
def groupnorm(x, gamma, beta, B, T, Kg, W, N, gstride, eps, add=None, dt=F64, wrong=None):
    xr = x.to(dt).reshape(B, T, Kg, W)
    mean = xr.mean(dim=(1, 3), keepdim=True)
    var = xr.var(dim=(1, 3), unbiased=(wrong == "unbiased"), keepdim=True)
    xh = (xr - mean) / torch.sqrt(var + eps)
    g = torch.stack([gamma[k * gstride:k * gstride + N] for k in range(Kg)]).to(dt)
    b = torch.stack([beta[k * gstride:k * gstride + N] for k in range(Kg)]).to(dt)
    y = xh.reshape(B, T, Kg, W // N, N) * g[None, None, :, None, :] + b[None, None, :, None, :]
    if add is not None:
        y = y + add.to(dt).reshape(B, 1, 1, 1, N)
    return y.reshape(B, T, Kg, W)


# ---------------------------------------------------------------------------------------------------------
# one-liners
# ---------------------------------------------------------------------------------------------------------
def peak_normalize(x, peak):
    x = x.double()
    return x / x.abs().max() * peak


_worst = {}


def record(name, shape, err, bound):
    """worst observed error over the cases of one kernel and the bound it was held to there -> the parity artefact
    (tests/parity_log.py) under "kernel_<name>"."""
    from tests import parity_log
    w = _worst.setdefault(name, dict(shapes=[], worst_err=0.0, bound=0.0, err_over_bound=-1.0))
    if str(shape) not in w["shapes"]:
        w["shapes"].append(str(shape))
    ratio = err / bound if bound > 0 else 0.0
    if ratio > w["err_over_bound"]:
        w.update(worst_err=err, bound=bound, err_over_bound=ratio)
    parity_log.record("kernel_" + name, **w)


def hold(name, shape, got, ref, bound):
    """assert |got - ref| <= bound element by element, after printing and recording the worst figure."""
    err, at, ratio = compare(got, ref, bound)
    print("%s %s: worst err %.3e at bound %.3e (%.3f of it)" % (name, shape, err, at, ratio))
    record(name, shape, err, at)
    assert ratio <= 1.0, (name, shape, err, at)


# ---------------------------------------------------------------------------------------------------------
# inputs (shared by the GPU tests and tests/test_kernel_ref_cpu.py)
# ---------------------------------------------------------------------------------------------------------
def gen(seed):
    return torch.Generator().manual_seed(seed)


def draw_conv(B, T, F, seed=0):
    """tanh-range feature map, weights at the scale torch initialises them, an output gradient."""
    g = gen(1000 + 131 * B + 17 * T + F + seed)
    U = torch.tanh(torch.randn(B, T, F, 16, generator=g))
    W = 0.05 * torch.randn(4, 16, 5, 5, generator=g)
    b = 0.05 * torch.randn(4, generator=g)
    dpre = torch.randn(B, T, F, 4, generator=g)
    return U, W, b, dpre


def draw_glu4(rows, F, Fs, seed=0):
    g = gen(2000 + 7 * rows + F + seed)
    pm = clamp_pre(torch.randn(rows, Fs, 4, generator=g))
    pr = clamp_pre(torch.randn(rows, Fs, 4, generator=g))
    x = torch.randn(rows, F, 2, generator=g)
    dout = torch.randn(rows, F, 2, generator=g)
    return pm, pr, x, dout


def draw_band_pre(rows, F, P, seed=0):
    g = gen(3000 + 7 * rows + F + seed)
    pm = clamp_pre(torch.randn(rows, P, generator=g))
    pr = clamp_pre(torch.randn(rows, P, generator=g))
    x = torch.randn(rows, F, 2, generator=g)
    dout = torch.randn(rows, F, 2, generator=g)
    return pm, pr, x, dout


def draw_spec(B, T, F, n_gb, seed=0):
    g = gen(4000 + 7 * T + F + seed)
    spec = torch.randn(B, T, F, 2, generator=g) * (0.2 + torch.rand(1, 1, F, 1, generator=g)) + 0.3
    gamma = 1 + 0.3 * torch.randn(n_gb, generator=g)
    beta = 0.2 * torch.randn(n_gb, generator=g)
    return spec, gamma, beta, g


def draw_groupnorm(B, T, Kg, W, N, gstride, seed=0):
    g = gen(5000 + B * 100 + T + seed)
    x = torch.randn(B, T, Kg, W, generator=g) + 0.5
    ng = max(1, Kg if gstride else 1) * max(N, gstride)
    gamma = 1 + 0.3 * torch.randn(ng, generator=g)
    beta = 0.2 * torch.randn(ng, generator=g)
    dy = torch.randn(B, T, Kg, W, generator=g)
    add = torch.randn(B, N, generator=g)
    return x, gamma, beta, dy, add


def draw_flow_state(B, per_b, seed=0):
    g = gen(6000 + per_b + seed)
    return tuple(torch.randn(B, per_b, 2, generator=g) for _ in range(3))


def draw_complex_logmag(n, seed=0):
    """magnitudes log-uniform over 1e-6 .. 1e2, uniform phase; element 0 at the upper end, an exact zero where n allows."""
    g = gen(7000 + n % 9973 + seed)
    mag = 10.0 ** (torch.rand(n, generator=g, dtype=F64) * 8 - 6)
    mag[0] = 1e2
    ph = torch.rand(n, generator=g, dtype=F64) * 2 * math.pi
    x = torch.stack([mag * torch.cos(ph), mag * torch.sin(ph)], -1).float()
    if n > 2:
        x[n // 2] = 0.0
        x[n - 1] = torch.tensor([1e-6, 0.0])
    return x
