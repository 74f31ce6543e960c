"""CPU: the checkers of tests/gemm_ref.py catch what the exact-input GPU cases of the GEMM families rely on them for.

An honest kernel is simulated in fp32 on the exact (dyadic) inputs - K summed in another order than the reference (reversed, in 64-wide chunks, or
two halves added at the end), the epilogue in fp32, one rounding, stores through the guarded buffer - and must pass check_exact.  Every mutant of
that simulation (the faults a pipelined K-loop, a grouped LoRA tail, an epilogue or a store is likely to have) must FAIL.  For the nonlinear
epilogues the honest fp32 evaluation passes check_bounded and the mutants (a wrong quick-GELU constant, sin / cos swapped on one head) fail."""
import math

import pytest
import torch

import gemm_ref as R

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
M, N, K1, K2, G = 300, 512, 192, 64, 2          # two 256x256 column tiles, a ragged second row tile, one LoRA tail group per column tile


@pytest.fixture(scope="module")
def prob():
    d = R.make_nt(M, N, K1, K2, a2_groups=G, seed=11, alpha=0.5, bias=True, residual="bf16")
    want, _ = R.ref_gemm_nt(**d)
    return d, want


def accumulate(A, B, order):
    """fp32 A . B^T with K summed in `order`"""
    A, B = A.to(F32), B.to(F32)
    K = A.shape[1]
    chunks = [slice(k, k + 64) for k in range(0, K, 64)]
    if order == "reversed":
        acc = torch.zeros(A.shape[0], B.shape[0])
        for c in reversed(chunks):
            acc = acc + A[:, c].flip(1) @ B[:, c].flip(1).t()
        return acc
    if order == "chunks64":
        acc = torch.zeros(A.shape[0], B.shape[0])
        for c in chunks:
            acc = acc + A[:, c] @ B[:, c].t()
        return acc
    h = K // 2
    return A[:, :h] @ B[:, :h].t() + A[:, h:] @ B[:, h:].t()          # "halves": two partial sums added at the end (split-K, the K-fold)


def simulate(d, out_dtype, order="chunks64", mutant=None):
    """the kernel in fp32: per column group [A1 | A2 group] . [B1 | B2]^T, then alpha, bias, residual, ONE rounding, stores through a guarded buffer"""
    gn = d["a2_group_n"]
    acc = torch.empty(M, N, dtype=F32)
    for g in range(N // gn):
        cols = slice(g * gn, (g + 1) * gn)
        ga = g - 1 if (mutant == "tail_of_neighbour_group" and g == 1) else g
        A = torch.cat([d["a1"], d["a2"][:, ga * K2:(ga + 1) * K2]], 1)
        B = torch.cat([d["b1"][cols], d["b2"][cols]], 1)
        acc[:, cols] = accumulate(A, B, order)
        if mutant == "drop_one_product" and g == 0:
            i, j = 137, 201
            k = int((A[i].float() * B[j].float()).abs().argmax())
            assert float(A[i, k]) * float(B[j, k]) != 0.0
            acc[i, j] -= A[i, k].float() * B[j, k].float()
        if mutant == "skip_last_k_tile" and g == 1:          # the 256x256 tile (row tile 1, column tile 1)
            acc[256:, cols] -= A[256:, -64:].float() @ B[:, -64:].float().t()
    bias, res = d["bias"].to(F32)[None, :], d["residual"].to(F32)
    alpha = torch.tensor(d["alpha"], dtype=F32)
    if mutant == "alpha_after_bias":
        v = (acc + bias) * alpha + res
    elif mutant == "double_rounding":
        v = (acc * alpha + bias).to(BF).to(F32) + res
    else:
        v = acc * alpha + bias + res
    if mutant == "swap_two_columns":
        v[:, [70, 71]] = v[:, [71, 70]]
    C, guard = R.guarded(M, N, out_dtype)
    C.copy_(v.to(out_dtype))
    if mutant == "one_element_unwritten":
        C[299, 511] = float("nan")
    if mutant == "store_into_guard_row":
        C.as_strided((1, 1), (1, 1), C.storage_offset() + M * C.stride(0) + 5)[0, 0] = 1.0
    if mutant == "one_bf16_ulp":
        assert float(C[17, 300]) != 0.0
        bits = C[17:18, 300:301].to(BF).view(torch.int16) + 1
        C[17, 300] = bits.view(BF).to(out_dtype)[0, 0]
    return C, guard


def run_checks(d, want, out_dtype, **kw):
    C, guard = simulate(d, out_dtype, **kw)
    guard()
    R.check_exact(C, want)


@pytest.mark.parametrize("out_dtype", [BF, F32])
@pytest.mark.parametrize("order", ["reversed", "chunks64", "halves"])
def test_honest_simulation_is_exact(prob, order, out_dtype):
    d, want = prob
    run_checks(d, want, out_dtype, order=order)


MUTANTS = ["drop_one_product", "skip_last_k_tile", "tail_of_neighbour_group", "swap_two_columns", "alpha_after_bias", "double_rounding",
           "one_element_unwritten", "store_into_guard_row", "one_bf16_ulp"]


@pytest.mark.parametrize("mutant", MUTANTS)
def test_every_mutant_is_caught(prob, mutant):
    d, want = prob
    for out_dtype in ((BF,) if mutant == "double_rounding" else (BF, F32)):          # an fp32 result has no second rounding to get wrong
        with pytest.raises(AssertionError) as e:
            run_checks(d, want, out_dtype, mutant=mutant)
        assert "the case left the exact regime" not in str(e.value)


def test_failure_report_names_the_tiles(prob):
    d, want = prob
    with pytest.raises(AssertionError) as e:
        run_checks(d, want, BF, mutant="skip_last_k_tile")
    msg = str(e.value)
    assert "256x256: [(1, 1)]" in msg and "(row, col, got, want)" in msg and "128x128: [(2, 2), (2, 3)]" in msg


def test_exact_regime_is_guarded():
    R.assert_exact_regime(11008 + 256, 2.0, 2, 2, 2)
    with pytest.raises(AssertionError):
        R.assert_exact_regime(2 ** 20, 1.0, 2, 2)
    with pytest.raises(AssertionError):
        R.assert_exact_regime(64, 0.37, 2, 2)
    with pytest.raises(AssertionError):          # a reference that is not exact in fp32 cannot be compared bit for bit
        R.check_exact(torch.zeros(1, 1), torch.full((1, 1), 1.0 + 2.0 ** -30, dtype=F64))


def test_gemm_tn_reference_and_atomic_order():
    """C0 + alpha P^T Q with grouped Q columns: row blocks of M added in any order (the fp32 atomics of the stream-K kernel) give the reference's bits"""
    d = R.make_tn(777, 256, 128, groups=2, seed=5)
    want = R.ref_gemm_tn(**d)
    C, guard = R.guarded(256, 128, F32, fill=d["C0"])
    for blk in (slice(512, 777), slice(0, 256), slice(256, 512)):
        for g in range(2):
            rows = slice(g * 128, (g + 1) * 128)
            C[rows] += 2.0 * (d["P"][blk, rows].float().t() @ d["Q"][blk, g * 128:(g + 1) * 128].float())
    guard()
    R.check_exact(C, want)
    last = slice(128, 256)          # the second row group of C, with the FIRST group's Q columns: one row of M added twice, mis-grouped
    C[last] += 2.0 * (d["P"][:1, last].float().t() @ d["Q"][:1, :128].float())
    with pytest.raises(AssertionError):
        R.check_exact(C, want)


# ---- bounded checks: the nonlinear epilogues ----------------------------------------------------------------------------------------------
# fp32 evaluation of x * sigmoid(1.702 x) / erf GELU on an exact pre-activation |v| <= 16: the argument 1.702f * v carries a relative 2^-23, exp a further
# |argument| 2^-23 <= 28 * 2^-23 relative, all damped by sigmoid' <= 1/4: below 2^-19 max(1, |v|)
EPS_SIM = 2.0 ** -19


@pytest.fixture(scope="module")
def act_prob():
    d = R.make_nt(129, 256, 128, seed=21, bias=True, residual="f32")
    return d


def act_sim(d, act, c=1.702):
    v = (d["a1"].to(F32) @ d["b1"].to(F32).t()) * d["alpha"] + d["bias"].to(F32)[None, :]
    if act == R.ACT_QUICK_GELU:
        y = v / (1.0 + torch.exp(torch.tensor(-c, dtype=F32) * v))
    else:
        y = 0.5 * v * (1.0 + torch.erf(v * 0.70710678118654752))
    return y + d["residual"]


@pytest.mark.parametrize("act", [R.ACT_QUICK_GELU, R.ACT_GELU])
def test_activation_epilogue_bound(act_prob, act):
    d = act_prob
    want, v = R.ref_gemm_nt(**d, act=act)
    assert float(v.abs().max()) > 6.0
    for out_dtype in (BF, F32):
        bound = R.rounding_term(want, out_dtype) + EPS_SIM * v.abs().clamp(min=1.0)
        C, guard = R.guarded(129, 256, out_dtype)
        C.copy_(act_sim(d, act).to(out_dtype))
        guard()
        R.check_bounded(C, want, bound)
    if act == R.ACT_QUICK_GELU:          # sigmoid(1.7 v): visible in an fp32 result only (a bf16 result rounds it away: a GPU grid has to run both)
        C, _ = R.guarded(129, 256, F32)
        C.copy_(act_sim(d, act, c=1.7))
        with pytest.raises(AssertionError):
            R.check_bounded(C, want, R.rounding_term(want, F32) + EPS_SIM * v.abs().clamp(min=1.0))


def test_swiglu_references():
    """SWIGLU_PAIR and SWIGLU_BWD references == the two-step forms on the bf16-rounded intermediate"""
    F, K = 256, 128
    d = R.make_nt(70, 2 * F, K, seed=31)
    perm = R.swiglu_pair_rows(F)
    y, _ = R.ref_gemm_nt(d["a1"], d["b1"][perm], act=R.ACT_SWIGLU_PAIR)
    gu = R.bf16_round(d["a1"].to(F64) @ d["b1"].to(F64).t())
    assert float((y - torch.nn.functional.silu(gu[:, :F]) * gu[:, F:]).abs().max()) < 1e-12
    gu_st = R.dyadic((70, 2 * F), 77, 2, lim=32)
    db = R.make_nt(70, F, K, seed=32)
    y, _ = R.ref_gemm_nt(db["a1"], db["b1"], residual=gu_st, act=R.ACT_SWIGLU_BWD)
    dact = R.bf16_round(db["a1"].to(F64) @ db["b1"].to(F64).t()).requires_grad_(False)
    g, u = gu_st[:, :F].to(F64).requires_grad_(True), gu_st[:, F:].to(F64).requires_grad_(True)
    (torch.nn.functional.silu(g) * u * dact).sum().backward()
    assert float((y - torch.cat([g.grad, u.grad], 1)).abs().max()) < 1e-12


def rope_sim(c, cos, sin, pos, rope_cols, swap_head=None):
    """fp32 rotation of the bf16 projection c [M, N] by the tables, one rounding"""
    Mr = c.shape[0]
    y = c.to(F32).clone()
    h = c.to(F32)[:, :rope_cols].view(Mr, rope_cols // 128, 128)
    cs, sn = cos[pos][:, None, :].expand(Mr, rope_cols // 128, 64).clone(), sin[pos][:, None, :].expand(Mr, rope_cols // 128, 64).clone()
    if swap_head is not None:
        cs[:, swap_head], sn[:, swap_head] = sn[:, swap_head].clone(), cs[:, swap_head].clone()
    c1, c2 = h[..., :64], h[..., 64:]
    y[:, :rope_cols] = torch.cat([c1 * cs - c2 * sn, c2 * cs + c1 * sn], -1).view(Mr, rope_cols)
    return y.to(BF)


def test_rope_epilogue_bound():
    Mr, Nr, L, seg = 200, 512, 200, (120, 40)
    d = R.make_nt(Mr, Nr, 128, seed=41)
    inv = 1.0 / (10000.0 ** (torch.arange(0, 128, 2, dtype=F32) / 128))
    ang = torch.outer(torch.arange(L, dtype=F32), inv)
    cos, sin = ang.cos(), ang.sin()
    want, mag = R.ref_gemm_nt(**d, rope=dict(cos=cos, sin=sin, L=L, rope_cols=256, seg=seg))
    pos = torch.arange(Mr)
    pos = torch.where(pos >= 120, 120 + (pos - 120) % 40, pos)          # packed responses restart at the prefix end
    c = (d["a1"].to(F32) @ d["b1"].to(F32).t()).to(BF)
    bound = R.rounding_term(want, BF) + 4 * 2.0 ** -24 * mag
    got = rope_sim(c, cos, sin, pos, 256)
    R.check_bounded(got, want, bound)
    R.check_exact(got[:, 256:], want[:, 256:])                          # the columns that are not rotated: the projection, rounded once
    with pytest.raises(AssertionError) as e:
        R.check_bounded(rope_sim(c, cos, sin, pos, 256, swap_head=1), want, bound)
    assert "128x128: [(0, 1), (1, 1)]" in str(e.value)
    with pytest.raises(AssertionError):                                  # positions that do not restart
        R.check_bounded(rope_sim(c, cos, sin, torch.arange(Mr), 256), want, bound)


def test_table_free_rope_angle_formula_meets_the_header():
    """opadpo_gemm_nt_rope_pos computes its angle as fract(float(pos) * frev) revolutions, frev = exp2f(-2i/128 * log2f(theta)) / 2 pi in fp32
    (gemm.hip, w4_direct_epilogue_rope_pos).  Emulated here in fp32 with an exact exp2: against HF's fp32 angles pos * inv_freq the error grows with the
    position (every fp32 rounding of the product is relative) - 1.2e-7 * pos: within 2e-4 rad up to position 1600, 4.2e-4 at 4095 - so
    include/opadpo_hip.h promises max(2e-4, 3e-7 * pos) (one unit of the hardware exp2 can add as much again), not 2e-4 everywhere."""
    i = torch.arange(64, dtype=F32)
    l2t = torch.tensor(math.log2(10000.0), dtype=F32)
    frev = (torch.exp2((-(2 * i) * (1.0 / 128.0) * l2t).to(F64)).to(F32) * torch.tensor(0.15915494309189535, dtype=F32))
    inv = 1.0 / (torch.tensor(10000.0, dtype=F32) ** (torch.arange(0, 128, 2, dtype=F32) / 128.0))
    pos = torch.arange(4096, dtype=F32)
    x = pos[:, None] * frev[None, :]
    x = x - x.floor()
    d = x.to(F64) * 2 * math.pi - (pos[:, None] * inv[None, :]).to(F64)
    d = ((d + math.pi) % (2 * math.pi) - math.pi).abs().amax(1)
    assert float(d[:1601].max()) <= 2e-4 < float(d.max()) < 4.5e-4
    assert bool((d[1:] <= 1.25e-7 * pos[1:].to(F64) + 1e-6).all())
    assert bool((d + 2.0 ** -23 * pos.to(F64) <= torch.clamp(3e-7 * pos.to(F64), min=2e-4)).all())          # with one unit of exp2 on the frequency
