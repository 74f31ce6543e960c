"""float64 reference, exact-input makers and per-element checkers for the gemm_nt / gemm_tn kernel families (plain torch on the CPU; no import
of the library).

The exact-input method: operands are small dyadic numbers - `a` an integer in [-4, 4] times 2^-p, `b` an integer in [-4, 4] times 2^-q, both exact
in bf16.  Every product is an integer multiple of 2^-(p+q) and every partial sum stays below 16 K 2^-(p+q) < 2^24 units, so an fp32 accumulation
is EXACT in any order (split-K, stream-K with fp32 atomics, the K-fold + reduce pass, any MFMA shape).  With a power-of-two alpha and small dyadic
bias / residual the linear epilogue is exact as well: an fp32 result equals the float64 reference bit for bit, a bf16 result equals the reference
rounded ONCE to bf16.  The nonlinear epilogues see an exact pre-activation; what is left is the kernel's fp32 evaluation of the function and the
final rounding, both bounded per element (check_bounded)."""
import math

import torch

BF = torch.bfloat16
F64 = torch.float64
LIM = 4                      # operands: integers in [-LIM, LIM] times a power of two
EXTRA_LIM = 8                # bias / residual / C0: integers in [-EXTRA_LIM, EXTRA_LIM] times 2^-EXTRA_SCALE
EXTRA_SCALE = 2

ACT_NONE, ACT_QUICK_GELU, ACT_GELU, ACT_SWIGLU_PAIR, ACT_SWIGLU_BWD = 0, 1, 2, 3, 4


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def dyadic(shape, seed, scale, lim=LIM, dtype=BF):
    """integers in [-lim, lim] times 2^-scale (exact in bf16 for lim < 256)"""
    g = torch.Generator().manual_seed(int(seed))
    v = torch.randint(-lim, lim + 1, tuple(shape), generator=g).to(F64) * 2.0 ** -scale
    out = v.to(dtype)
    assert torch.equal(out.to(F64), v)
    return out


def assert_exact_regime(K, alpha, p, q, extras=0):
    """A case stays in the exact regime: alpha is a power of two and every intermediate value of the kernel - a partial sum of at most 16 K product units
    2^-(p+q), its alpha multiple, and that plus `extras` bias / residual / C0 terms of at most EXTRA_LIM 2^-EXTRA_SCALE each - is a multiple of one common
    power of two and smaller than 2^24 of them: fp32 holds it without rounding, in any order of summation."""
    m, _ = math.frexp(abs(alpha))
    assert m == 0.5, f"alpha {alpha} is not a power of two"
    assert 16 * K * abs(alpha) < 2 ** 24 and 16 * K < 2 ** 24, f"K = {K}, alpha = {alpha}: 16 K |alpha| product units leave the exact regime"
    unit = min(abs(alpha), 1.0) * 2.0 ** -(p + q)
    if extras:
        unit = min(unit, 2.0 ** -EXTRA_SCALE)
    top = 16 * K * max(abs(alpha), 1.0) * 2.0 ** -(p + q) + extras * EXTRA_LIM * 2.0 ** -EXTRA_SCALE
    assert top / unit < 2 ** 24, f"K = {K}, alpha = {alpha}, p + q = {p + q}: {top / unit} units leave the exact regime"


def make_nt(M, N, K1, K2=0, a2_groups=0, a1_groups=0, seed=0, p=2, q=2, alpha=1.0, bias=False, residual=None, res_cols=None):
    """Dyadic operands of one gemm_nt problem, all on the CPU: a1 [M, K1] (or [M, a1_groups * K1], one K1-wide block per column group of
    N / a1_groups), b1 [N, K1], a2 [M, max(a2_groups, 1) * K2], b2 [N, K2], bias [N] bf16, residual [M, res_cols or N] 'bf16' / 'f32'."""
    extras = int(bool(bias)) + int(residual is not None)
    assert_exact_regime(K1 + K2, alpha, p, q, extras)
    d = dict(M=M, N=N, K1=K1, K2=K2, alpha=float(alpha), a2_group_n=0, a2_group_stride=0, a1_group_n=0, a1_group_stride=0,
             a2=None, b2=None, bias=None, residual=None)
    d["a1"] = dyadic((M, max(a1_groups, 1) * K1), seed * 16 + 1, p)
    d["b1"] = dyadic((N, K1), seed * 16 + 2, q)
    if a1_groups > 1:
        assert N % a1_groups == 0
        d["a1_group_n"], d["a1_group_stride"] = N // a1_groups, K1
    if K2:
        d["a2"] = dyadic((M, max(a2_groups, 1) * K2), seed * 16 + 3, p)
        d["b2"] = dyadic((N, K2), seed * 16 + 4, q)
        if a2_groups > 1:
            assert N % a2_groups == 0
            d["a2_group_n"], d["a2_group_stride"] = N // a2_groups, K2
    if bias:
        d["bias"] = dyadic((N,), seed * 16 + 5, EXTRA_SCALE, EXTRA_LIM)
    if residual is not None:
        d["residual"] = dyadic((M, res_cols or N), seed * 16 + 6, EXTRA_SCALE, EXTRA_LIM, BF if residual == "bf16" else torch.float32)
    return d


def make_tn(M, N1, N2, groups=0, seed=0, p=2, q=2, alpha=2.0):
    """Dyadic operands of one gemm_tn problem: P [M, N1], Q [M, max(groups, 1) * N2], C0 [N1, N2] fp32."""
    assert_exact_regime(M, alpha, p, q, 1)
    d = dict(M=M, N1=N1, N2=N2, alpha=float(alpha), q_group_n1=0, q_group_stride=0)
    d["P"] = dyadic((M, N1), seed * 16 + 1, p)
    d["Q"] = dyadic((M, max(groups, 1) * N2), seed * 16 + 2, q)
    d["C0"] = dyadic((N1, N2), seed * 16 + 3, EXTRA_SCALE, EXTRA_LIM, torch.float32)
    if groups > 1:
        assert N1 % groups == 0
        d["q_group_n1"], d["q_group_stride"] = N1 // groups, N2
    return d


def swiglu_pair_rows(F):
    """row order of the OPADPO_ACT_SWIGLU_PAIR weight layout: entry j = the row of [gate (F rows) | up (F rows)] that is stored at row j (rows per 128 =
    [64 gate | 64 up])"""
    return torch.stack([torch.arange(F).view(F // 64, 64), F + torch.arange(F).view(F // 64, 64)], 1).reshape(-1)


# ---- references -------------------------------------------------------------------------------------------------------------------------
def bf16_round(x64):
    """one round-to-nearest-even to bf16, back in float64 (x64 must be exact in fp32, so that the conversion rounds once)"""
    return x64.to(torch.float32).to(BF).to(F64)


def ref_product(a1, b1, K1, a2=None, b2=None, a2_group_n=0, a2_group_stride=0, a1_group_n=0, a1_group_stride=0):
    """A1 . B1^T + A2[:, group] . B2^T in float64 with the column-group addressing of include/opadpo_hip.h"""
    N = b1.shape[0]
    a1, b1 = a1.to(F64), b1.to(F64)
    if a1_group_n:
        out = torch.empty(a1.shape[0], N, dtype=F64)
        for g in range(N // a1_group_n):
            cols = slice(g * a1_group_n, (g + 1) * a1_group_n)
            out[:, cols] = a1[:, g * a1_group_stride:g * a1_group_stride + K1] @ b1[cols, :K1].t()
    else:
        out = a1[:, :K1] @ b1[:, :K1].t()
    if a2 is not None:
        a2, b2 = a2.to(F64), b2.to(F64)
        K2 = b2.shape[1]
        if a2_group_n:
            for g in range(N // a2_group_n):
                cols = slice(g * a2_group_n, (g + 1) * a2_group_n)
                out[:, cols] += a2[:, g * a2_group_stride:g * a2_group_stride + K2] @ b2[cols].t()
        else:
            out += a2[:, :K2] @ b2.t()
    return out


def act64(v, act):
    if act == ACT_QUICK_GELU:
        return v * torch.sigmoid(1.702 * v)
    if act == ACT_GELU:
        return 0.5 * v * (1.0 + torch.erf(v * math.sqrt(0.5)))
    return v


def ref_gemm_nt(a1, b1, K1=None, a2=None, b2=None, a2_group_n=0, a2_group_stride=0, a1_group_n=0, a1_group_stride=0, alpha=1.0, bias=None,
                residual=None, act=ACT_NONE, rope=None, **_):
    """float64 reference of opadpo_gemm_nt / _rope / _rope_pos: act(alpha (A1 B1^T + A2[:, group] B2^T) + bias) + R.
    Returns (y, v): the result and the pre-activation (the scale of the activation term of a per-element bound).
      ACT_SWIGLU_PAIR: b1 rows per 128 = [64 gate | 64 up]; y [M, N/2] = silu(gate) * up on the bf16-ROUNDED gate / up (the header: "SwiGLU ... fused
        into the gate|up projection", bit-identical to projection + opadpo_silu_mul_fwd on the stored bf16 tensor); v = |gate| |up|, the scale of the result
      ACT_SWIGLU_BWD: the product is d_act [M, N], rounded to bf16 first; residual = stored [gate | up] ([M, 2N]); y = [d_gate | d_up] with the
        arithmetic of opadpo_silu_mul_bwd; v = |d_act| (1 + |gate|) (1 + |up|), the scale of the result
      rope = dict(cos, sin, L, rope_cols, seg=(prefix, seg_len)) (table form, fp32 tables [>= L][64]) or dict(row_pos, theta, rope_cols) (table-free
        form: angle = pos * theta^(-2i/128) as HF's fp32 tables hold it): columns [0, rope_cols), heads of 128, half-split rotation of the
        bf16-ROUNDED projection; v = |c1| + |c2| of the rotated pair (0 on the columns that are not rotated)."""
    K1 = b1.shape[1] if K1 is None else K1
    prod = ref_product(a1, b1, K1, a2, b2, a2_group_n, a2_group_stride, a1_group_n, a1_group_stride)
    M, N = prod.shape
    if act == ACT_SWIGLU_PAIR:
        assert alpha == 1.0 and bias is None and residual is None and N % 256 == 0
        t = bf16_round(prod).view(M, N // 128, 2, 64)
        gate, up = t[:, :, 0, :].reshape(M, N // 2), t[:, :, 1, :].reshape(M, N // 2)
        return gate * torch.sigmoid(gate) * up, gate.abs() * up.abs()
    if act == ACT_SWIGLU_BWD:
        assert alpha == 1.0 and bias is None and residual is not None and residual.shape == (M, 2 * N)
        d = bf16_round(prod)
        gate, up = residual[:, :N].to(F64), residual[:, N:].to(F64)
        sg = torch.sigmoid(gate)
        dg = d * up * sg * (1.0 + gate * (1.0 - sg))
        du = d * gate * sg
        scale = d.abs() * (1.0 + gate.abs()) * (1.0 + up.abs())
        return torch.cat([dg, du], 1), torch.cat([scale, scale], 1)
    if rope is not None:
        assert alpha == 1.0 and bias is None and residual is None and act == ACT_NONE
        c = bf16_round(prod)
        rc = rope["rope_cols"]
        assert rc % 128 == 0 and rc <= N
        rows = torch.arange(M)
        if "row_pos" in rope:
            pos = rope["row_pos"].to(torch.int64)
            inv = 1.0 / (torch.tensor(float(rope["theta"]), dtype=torch.float32) ** (torch.arange(0, 128, 2, dtype=torch.float32) / 128.0))
            ang = (pos.to(torch.float32)[:, None] * inv[None, :]).to(F64)          # HF: fp32 angle = pos * inv_freq
            cos, sin = ang.cos(), ang.sin()
        else:
            pos = rows % rope["L"]
            pfx, sl = rope.get("seg", (0, 0))
            if sl > 0:
                pos = torch.where(pos >= pfx, pfx + (pos - pfx) % sl, pos)
            cos, sin = rope["cos"].to(F64)[pos], rope["sin"].to(F64)[pos]
        y, v = c.clone(), torch.zeros_like(c)
        h = c[:, :rc].view(M, rc // 128, 128)
        c1, c2 = h[..., :64], h[..., 64:]
        cs, sn = cos[:, None, :], sin[:, None, :]
        y[:, :rc] = torch.cat([c1 * cs - c2 * sn, c2 * cs + c1 * sn], -1).view(M, rc)
        mag = c1.abs() + c2.abs()
        v[:, :rc] = torch.cat([mag, mag], -1).view(M, rc)
        return y, v
    v = alpha * prod
    if bias is not None:
        v = v + bias.to(F64)[None, :]
    y = act64(v, act)
    if residual is not None:
        y = y + residual.to(F64)
    return y, v


def ref_gemm_tn(P, Q, C0, N2=None, q_group_n1=0, q_group_stride=0, alpha=1.0, **_):
    """C0 + alpha sum_m P[m, n1] Q[m, group(n1) + n2] in float64"""
    N1 = P.shape[1]
    N2 = C0.shape[1] if N2 is None else N2
    P, Q = P.to(F64), Q.to(F64)
    out = C0.to(F64).clone()
    if q_group_n1:
        for g in range(N1 // q_group_n1):
            rows = slice(g * q_group_n1, (g + 1) * q_group_n1)
            out[rows] += alpha * (P[:, rows].t() @ Q[:, g * q_group_stride:g * q_group_stride + N2])
    else:
        out += alpha * (P.t() @ Q[:, :N2])
    return out


# ---- checkers ---------------------------------------------------------------------------------------------------------------------------
def _report(bad, got, want, what):
    idx = bad.nonzero()
    n = idx.shape[0]
    first = [(int(r), int(c), float(got[r, c]), float(want[r, c])) for r, c in idx[:8].tolist()]
    tiles = {t: [tuple(rc) for rc in torch.unique(idx // t, dim=0)[:12].tolist()] for t in (256, 128, 64)}
    return (f"{what}: {n} of {bad.numel()} elements wrong; first (row, col, got, want): {first}; "
            f"tiles (row tile, column tile) 256x256: {tiles[256]}, 128x128: {tiles[128]}, 64x64: {tiles[64]}")


def check_exact(got, want64, what="exact"):
    """bitwise equality of `got` with want64 cast ONCE to got's dtype (round-to-nearest-even, as tensor.to does)"""
    got = got.detach().cpu()
    assert got.shape == want64.shape, (got.shape, want64.shape)
    w32 = want64.to(torch.float32)
    assert torch.equal(w32.to(F64), want64), "the reference itself is not exact in fp32: the case left the exact regime"
    want = w32.to(got.dtype)
    if got.dtype == BF:
        same = got.view(torch.int16) == want.view(torch.int16)
    else:
        same = got.view(torch.int32) == want.view(torch.int32)
    same = same | ((got == 0) & (want == 0) & ~torch.isnan(got))          # +0 / -0: an exact zero sum has no defined sign across summation orders
    assert bool(same.all()), _report(~same, got.to(F64), want.to(F64), what)


def check_bounded(got, want64, bound, what="bounded"):
    """per element |got - want| <= bound[i, j] (never a norm); a NaN fails"""
    got64 = got.detach().cpu().to(F64)
    assert got64.shape == want64.shape, (got64.shape, want64.shape)
    bound = torch.as_tensor(bound, dtype=F64).expand_as(want64)
    ok = (got64 - want64).abs() <= bound
    assert bool(ok.all()), _report(~ok, got64, want64, what)


def rounding_term(y64, dtype):
    """the ONE rounding of the result: half a unit in the last place of y in `dtype`.  bf16 carries 8 significant bits, so that is 2^(e - 8) for
    2^e <= |y| < 2^(e + 1) - between 2^-9 |y| and 2^-8 |y| (a relative 2^-9 would fail a correctly rounded result just above a power of two); fp32 carries
    24: 2^(e - 24), at most 2^-24 |y|"""
    _, e = torch.frexp(y64)                                   # |y| = m 2^e with 0.5 <= m < 1
    return torch.ldexp(torch.ones_like(y64), e - 1 - (8 if dtype == BF else 24)) * (y64 != 0)


SENTINEL = -1232.0          # exact in bf16 and fp32


def guarded(M, N, dtype, pad_rows=3, pad_cols=8, device="cpu", fill=None):
    """C [M, N] as a view into a [M + pad_rows, N + pad_cols] buffer: the valid region pre-filled with NaN (or with `fill`, for kernels that accumulate
    into C), guard rows below and guard columns to the right holding SENTINEL.  Returns (view, check): check() asserts that no guard element changed and
    that no NaN is left in the valid region."""
    buf = torch.full((M + pad_rows, N + pad_cols), SENTINEL, dtype=dtype, device=device)
    view = buf[:M, :N]
    if fill is None:
        view.fill_(float("nan"))
    else:
        view.copy_(fill)

    def check(what="guard"):
        b = buf.detach().cpu().to(F64)
        below, right = b[M:, :], b[:M, N:]
        assert bool((below == SENTINEL).all()), _report(below != SENTINEL, below, torch.full_like(below, SENTINEL), f"{what}: guard rows below M = {M} written")
        assert bool((right == SENTINEL).all()), _report(right != SENTINEL, right, torch.full_like(right, SENTINEL), f"{what}: guard columns right of N = {N} written")
        nan = torch.isnan(b[:M, :N])
        assert not bool(nan.any()), _report(nan, b[:M, :N], torch.zeros(M, N, dtype=F64), f"{what}: elements never written (NaN left)")

    return view, check
