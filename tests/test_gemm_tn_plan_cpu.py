"""CPU: the launch plan of the weight-gradient GEMMs (urse_gemm_tn_plan: what urse_gemm_tn / urse_gemm_tn_dual launch and what
urse_gemm_tn_act_f16_supported answers from), pinned in literal rows and checked field for field against a restatement of the three
dispatch chains the planner replaced, on the full cross product of shapes, targets, dtypes and step masks.  The plan needs no GPU.  None of
the environment switches (URSE_TN_NO_DMA, URSE_TN_NO_224, URSE_TN_TARGET) is set here: the restatement is the default configuration."""
import ctypes
import itertools

import pytest

F32, BF16, ACT_F16 = 0, 1, 3                      # URSE_F32, URSE_BF16, URSE_BF16_ACT_F16
KV_RING, KV_RING_T, KV_DUAL, KV_128 = 6, 7, 8, 9  # URSE_KV_TN_RING, _RING_T, _DUAL, _128
NONE, T128, RING, RING_T, DUAL224, DUAL_RING, TWO_SINGLE = range(7)      # URSE_TN_FORM_*
NO_KERNEL = (NONE, -1, 0, 0, -1, 0, 0, 0, 0)
C2_ROWS = 436288                                  # 32 utterances x 401 frames x 34 bands

# (R, Mo, No, No2, shift, inner, period, invalid_step, perm_h, dtype, target) with column sums ->
# (form, slot, mixed instance, ntw, column-sum mode, tiles, slices, rows_per_slice, grid)
C2_DUAL = (C2_ROWS, 1568, 196, 392, -34, 34, 401, 0, 0)
PINNED = [
    ((C2_ROWS, 196, 784, 0, 0, 1, 0, 0, 0, BF16, 0), (RING_T, KV_RING_T, 0, 7, 2, 4, 64, 6848, 256)),            # fc weight gradient
    ((C2_ROWS, 196, 784, 0, 0, 1, 0, 0, 0, BF16, 98), (RING_T, KV_RING_T, 0, 7, 2, 4, 24, 18208, 96)),
    ((C2_ROWS, 196, 784, 0, 0, 1, 0, 0, 0, ACT_F16, 0), (RING_T, KV_RING_T, 1, 7, 2, 4, 64, 6848, 256)),
    ((20000, 608, 200, 0, 0, 1, 0, 0, 0, BF16, 0), (RING, KV_RING, 0, 7, 1, 3, 79, 256, 237)),
    ((17007, 1568, 392, 0, -1, 1, 34, 0, 392, BF16, 0), (RING, KV_RING, 0, 7, 1, 14, 18, 960, 252)),
    ((333, 200, 40, 0, 0, 1, 0, 0, 0, F32, 0), (T128, KV_128, 0, 0, -1, 2, 6, 64, 12)),
    (C2_DUAL + (BF16, 0), (DUAL224, KV_DUAL, 0, 0, -1, 14, 18, 24256, 252)),                                      # time path, whole chip
    (C2_DUAL + (BF16, 112), (DUAL224, KV_DUAL, 0, 0, -1, 14, 8, 54560, 112)),                                    # beside the BPTT
    (C2_DUAL + (BF16, 98), (DUAL224, KV_DUAL, 0, 0, -1, 14, 7, 62336, 98)),
    (C2_DUAL + (BF16, 84), (DUAL224, KV_DUAL, 0, 0, -1, 14, 6, 72736, 84)),
    (C2_DUAL + (ACT_F16, 84), (DUAL224, KV_DUAL, 1, 0, -1, 14, 6, 72736, 84)),
    (C2_DUAL + (BF16, 13), (DUAL_RING, KV_DUAL, 0, 7, 1, 21, 1, C2_ROWS, 21)),                                   # 14 tiles do not fit 13 workgroups ...
    (C2_DUAL + (ACT_F16, 13), NO_KERNEL),                                                                        # ... and the ring kernel has no mixed form
    ((C2_ROWS, 3072, 384, 768, -1, 1, 48, 0, 0, BF16, 0), (DUAL_RING, KV_DUAL, 0, 7, 1, 72, 3, 145440, 216)),    # H = 768: no 224-row tiles
    ((C2_ROWS, 1568, 196, 392, -34, 34, 401, 0, 0, F32, 0), (TWO_SINGLE, -1, 0, 0, -1, 0, 0, 0, 0)),
]


@pytest.fixture(scope="module")
def plan_of(lib):
    buf = (ctypes.c_int64 * 9)()

    def plan_of(R, Mo, No, No2, colsum, shift, inner, period, invalid_step, perm_h, dtype, target):
        assert lib.urse_gemm_tn_plan(R, Mo, No, No2, colsum, shift, inner, period, invalid_step, perm_h, dtype, target, buf) == 0
        return tuple(buf)
    return plan_of


@pytest.mark.parametrize("call,expected", PINNED)
def test_pinned_plans(plan_of, call, expected):
    R, Mo, No, No2, shift, inner, period, invalid_step, perm_h, dtype, target = call
    assert plan_of(R, Mo, No, No2, 1, shift, inner, period, invalid_step, perm_h, dtype, target) == expected


# ---- the dispatch of urse_gemm_tn, urse_gemm_tn_dual and urse_gemm_tn_act_f16_supported as they stood before the planner, restated ----
def _cdiv(a, b):
    return (a + b - 1) // b


def _split32(R, target, tl):
    slices = max(1, target // tl)
    rps = _cdiv(_cdiv(R, slices), 32) * 32
    return _cdiv(R, rps), rps


def _old_query(R, Mo, No, No2, colsum, inner, period):
    if R < 16384 or R >= 1 << 30:
        return False
    if No2 == 0:
        return bool(colsum) and 160 <= Mo < 512 and No >= 512 and _cdiv(Mo, 224) * 224 < _cdiv(Mo, 256) * 256
    V = _cdiv(No, 8) * 8 + No2 + (1 if colsum else 0)
    inner = max(inner, 1)
    return (Mo >= 512 and Mo % 224 == 0 and No2 % 8 == 0 and R % 32 == 0 and V <= 640 and 0 < period < 1 << 31 and inner < 1 << 31
            and R % (inner * period) == 0 and (Mo // 224) * _cdiv(V, 320) <= 256)


def _old_tn(R, Mo, No, colsum, shift, inner, period, invalid_step, perm_h, dtype, target_workgroups):
    target = target_workgroups or 256
    act_f16 = dtype == ACT_F16
    if act_f16:
        if not _old_query(R, Mo, No, 0, colsum, 1, 0) or perm_h != 0 or shift != 0 or period != 0:
            return NO_KERNEL
        dtype = BF16
    if dtype == BF16 and perm_h == 0 and shift == 0 and period == 0 and 160 <= Mo < 512 and No >= 512 and 16384 <= R < 1 << 30:
        qMo, qNo = No, Mo                                  # the transposed problem
        ntw = 7 if _cdiv(qNo, 224) * 224 < _cdiv(qNo, 256) * 256 else 8
        tl = _cdiv(qMo, 256) * _cdiv(qNo, 32 * ntw)
        slices, rps = _split32(R, target, tl)
        return (RING_T, KV_RING_T, int(act_f16), ntw, 2 if colsum else 0, tl, slices, rps, tl * slices)
    if (dtype == BF16 and Mo >= 512 and No >= 160 and 16384 <= R < 1 << 30 and inner < 1 << 31 and -(1 << 30) < shift < 1 << 30
            and period < 1 << 31):
        ntw = 7 if _cdiv(No, 224) * 224 < _cdiv(No, 256) * 256 else 8
        tl = _cdiv(Mo, 256) * _cdiv(No, 32 * ntw)
        slices, rps = _split32(R, target, tl)
        return (RING, KV_RING, 0, ntw, 1 if colsum else 0, tl, slices, rps, tl * slices)
    tiles = _cdiv(Mo, 128) * _cdiv(No, 128)
    bkr = 32 if dtype == BF16 else 16
    slices = max(1, min(768 // tiles, _cdiv(R, 4 * bkr)))
    rps = _cdiv(_cdiv(R, slices), bkr) * bkr
    slices = _cdiv(R, rps)
    return (T128, KV_128, 0, 0, -1, tiles, slices, rps, tiles * slices)


def _old_dual(R, Mo, No, No2, colsum, shift, inner, period, invalid_step, perm_h, dtype, target_workgroups):
    """with what urse_gemm_tn_plan assumes: aligned operands, lda >= Mo, ldb >= round_up(No, 8), ldb2 >= No2"""
    target = target_workgroups or 256
    act_f16 = dtype == ACT_F16
    if act_f16:
        if not _old_query(R, Mo, No, No2, colsum, inner, period):
            return NO_KERNEL
        dtype = BF16
    big = (dtype == BF16 and Mo >= 512 and 16384 <= R < 1 << 30 and -(1 << 30) < shift < 1 << 30 and period < 1 << 31 and inner < 1 << 31)
    if not big:
        return NO_KERNEL if act_f16 else (TWO_SINGLE, -1, 0, 0, -1, 0, 0, 0, 0)
    V = _cdiv(No, 8) * 8 + No2 + (1 if colsum else 0)
    inn = max(inner, 1)
    mask_covers_range = (period > 0 and R % (inn * period) == 0
                         and ((shift == -inn and invalid_step == 0) or (shift == inn and invalid_step == period - 1)))
    if (Mo % 224 == 0 and No2 % 8 == 0 and R % 32 == 0 and mask_covers_range and V <= 640 and perm_h >= 0
            and (Mo // 224) * _cdiv(V, 320) <= target):
        tl = (Mo // 224) * _cdiv(V, 320)
        slices, rps = _split32(R, target, tl)
        return (DUAL224, KV_DUAL, int(act_f16), 0, -1, tl, slices, rps, tl * slices)
    if act_f16:
        return NO_KERNEL
    tl = _cdiv(Mo, 256) * (_cdiv(No, 224) + _cdiv(No2, 224))
    slices, rps = _split32(R, target, tl)
    return (DUAL_RING, KV_DUAL, 0, 7, 1 if colsum else 0, tl, slices, rps, tl * slices)


SWEEP_R = (64, 333, 16383, 16384, 17007, 20000, C2_ROWS)
SWEEP_MO = (159, 160, 196, 224, 511, 512, 608, 1568, 3072)
SWEEP_NO = (40, 159, 160, 196, 200, 392, 512, 784)
SWEEP_NO2 = (0, 392, 768, 396)
SWEEP_TARGETS = (0, 13, 84, 98, 112)
# (inner, period, shift, invalid_step); the last one is a mask that does not cover the rows its shift reaches
SWEEP_MASKS = ((1, 0, 0, 0), (1, 34, -1, 0), (1, 34, 1, 33), (34, 401, -34, 0), (34, 401, 34, 0))


def test_plan_equals_the_dispatch_it_replaced(lib, plan_of):
    """302,400 plans; for each with target 0 and the mask the query assumes (none for urse_gemm_tn; shift = -inner, invalid_step = 0 for the
    dual), urse_gemm_tn_act_f16_supported is "the URSE_BF16_ACT_F16 plan uses the mixed-operand instance" and what it was before."""
    queried = 0
    for R, Mo, No, No2, colsum, (inner, period, shift, inv) in itertools.product(SWEEP_R, SWEEP_MO, SWEEP_NO, SWEEP_NO2, (0, 1), SWEEP_MASKS):
        for target, dtype in itertools.product(SWEEP_TARGETS, (BF16, F32, ACT_F16)):
            got = plan_of(R, Mo, No, No2, colsum, shift, inner, period, inv, 0, dtype, target)
            want = (_old_dual(R, Mo, No, No2, colsum, shift, inner, period, inv, 0, dtype, target) if No2 else
                    _old_tn(R, Mo, No, colsum, shift, inner, period, inv, 0, dtype, target))
            if got != want:
                raise AssertionError((R, Mo, No, No2, colsum, shift, inner, period, inv, dtype, target, got, want))
        canonical = (shift == -inner and inv == 0 and period > 0) if No2 else (shift == 0 and period == 0)
        if canonical:
            answer = lib.urse_gemm_tn_act_f16_supported(R, Mo, No, No2, colsum, inner, period)
            mixed = plan_of(R, Mo, No, No2, colsum, shift, inner, period, inv, 0, ACT_F16, 0)[2]
            assert answer == mixed == int(_old_query(R, Mo, No, No2, colsum, inner, period)), (R, Mo, No, No2, colsum, inner, period)
            queried += 1
    assert queried == len(SWEEP_R) * len(SWEEP_MO) * len(SWEEP_NO) * 2 * (2 * 3 + 1)


def test_row_permutation_in_the_plan(plan_of):
    """perm_h leaves the transposed kernel (which writes C^T and has no row map) and, when negative, the 224 x 320 kernel"""
    for perm_h in (392, -64):
        got = plan_of(C2_ROWS, 196, 784, 0, 1, 0, 1, 0, 0, perm_h, BF16, 0)
        assert got == _old_tn(C2_ROWS, 196, 784, 1, 0, 1, 0, 0, perm_h, BF16, 0) and got[0] == T128
        assert plan_of(C2_ROWS, 196, 784, 0, 1, 0, 1, 0, 0, perm_h, ACT_F16, 0) == NO_KERNEL
        got = plan_of(*C2_DUAL[:4], 1, *C2_DUAL[4:8], perm_h, BF16, 0)
        assert got == _old_dual(*C2_DUAL[:4], 1, *C2_DUAL[4:8], perm_h, BF16, 0) and got[0] == (DUAL224 if perm_h > 0 else DUAL_RING)


def test_two_single_launches_are_planned_one_by_one(plan_of):
    """f32 operands: urse_gemm_tn_dual is two urse_gemm_tn calls; the plan says so and the caller asks for each half (No2 = 0)"""
    R, Mo, No, No2 = 20000, 608, 200, 392
    assert plan_of(R, Mo, No, No2, 1, -1, 1, 34, 0, 0, F32, 0)[:2] == (TWO_SINGLE, -1)
    assert plan_of(R, Mo, No, 0, 1, 0, 1, 0, 0, 0, F32, 0) == _old_tn(R, Mo, No, 1, 0, 1, 0, 0, 0, F32, 0)
    assert plan_of(R, Mo, No2, 0, 0, -1, 1, 34, 0, 0, F32, 0)[:2] == (T128, KV_128)


def test_plan_rejects_bad_arguments(lib):
    buf = (ctypes.c_int64 * 9)()
    for R, Mo, No, No2, target in ((0, 196, 784, 0, 0), (64, 0, 40, 0, 0), (64, 40, -1, 0, 0), (64, 40, 40, -8, 0), (64, 40, 40, 0, -1)):
        assert lib.urse_gemm_tn_plan(R, Mo, No, No2, 1, 0, 1, 0, 0, 0, BF16, target, buf) == -1          # URSE_ERR_INVALID_ARG
    assert lib.urse_gemm_tn_plan(64, 40, 40, 0, 1, 0, 1, 0, 0, 0, BF16, 0, None) == -1
    assert b"urse_gemm_tn_plan" in lib.urse_last_error()


def test_ops_wrapper_names_the_form_and_the_counter(lib):
    from urgent2026_challenge_track1_amd import ops
    p = ops.gemm_tn_plan(C2_ROWS, 196, 784, dtype=ops.BF16_ACT_F16)
    assert p == dict(form="ring_t", slot="tn_ring_t", act_f16=True, ntw=7, colsum_mode=2, tiles=4, slices=64, rows_per_slice=6848, grid=256)
    p = ops.gemm_tn_plan(C2_ROWS, 1568, 196, 392, shift=-34, inner=34, period=401, dtype=ops.BF16_ACT_F16, target_wgs=13)
    assert p["form"] == "none" and p["slot"] is None and not p["act_f16"]
    assert len(ops.TN_FORMS) == 7 and [ops.KERNEL_VARIANTS[i] for i in (KV_RING, KV_RING_T, KV_DUAL, KV_128)] == ["tn_ring", "tn_ring_t", "tn_dual", "tn_128"]
