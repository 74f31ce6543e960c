"""GPU: the gemm_nt and gemm_tn kernel families against the float64 reference of tests/gemm_ref.py, exactly or per element - never a norm.

Exact cases: the operands are small dyadic numbers (gemm_ref.make_nt / make_tn), so every fp32 accumulation is exact in any order and the linear
epilogue (power-of-two alpha, dyadic bias / residual / C0) is exact too.  An fp32 result must equal the reference bit for bit, a bf16 result the
reference rounded once.  One dropped, doubled or mis-indexed k-product, a wrong group offset, a wrong row or column mapping or a second rounding
fails such a case at any K.  Nonlinear epilogues see an exact pre-activation; what is left is the kernel's fp32 evaluation of the function and the
one rounding of the result, bounded per element (EPS_* below, each measured on an MI355X and recorded beside its bound).

Every case is pinned to its kernel: before the launch it asks the library (opadpo_debug_gemm_nt_plan / opadpo_debug_gemm_nt_decode_plan, with the
device's CU count) which kernels the call will run and asserts the families - a case that no longer reaches its kernel fails.  (gemm_tn has no plan
entry point: its cases name the switch, use_tr bit 3 / bit 0, and the shape rule - N1, N2 and the group width multiples of 256 - that select the
kernel.)  Every result is stored through gemm_ref.guarded: NaN-prefilled valid region, sentinel guard rows below M and guard columns right of N
(ldc > N), so an element never written and a store out of the region both fail.

The rounding term of the bounded cases is half a unit in the last place of the result (gemm_ref.rounding_term: between 2^-9 |y| and 2^-8 |y| for
bf16) - the tightest bound a correctly rounded result meets; a flat 2^-9 |y| would fail correct results just above a power of two.
SWIGLU_PAIR follows the header: silu(gate) * up on the bf16-ROUNDED gate / up ("bit-identical to projection + opadpo_silu_mul_fwd").

Wall time of the whole file on an MI355X: 7 s (287 cases, the float64 references included)."""
import ctypes as C
import functools

import pytest
import torch

import gemm_ref as R

pytestmark = pytest.mark.gpu

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
S_HINT = 0x100                     # OPADPO_GEMM_STREAM
W4S_FEW, NODEEP = 1 << 10, 1 << 11  # use_tr: the streaming walk on 8 workgroups; the default K-loop text for >= 128 K-tiles

# Measured on an MI355X over the grids of this file: the worst per-element (|got - want| - rounding term) / scale, scale as gemm_ref.ref_gemm_nt returns it
# (max(1, |v|) of the pre-activation for the GELUs).  Each bound is at most twice the measured figure.
EPS_ACT = 1.9e-7         # quick-GELU / GELU (__expf, erff in fp32); measured 9.586e-8 (fp32 C; every bf16 result is within its rounding term)
EPS_PAIR = 1.0e-7        # SWIGLU_PAIR; measured 5.316e-8 (streaming walk; 2.5e-8 skinny, 1.8e-12 one tile per workgroup, 0 skinny8)
EPS_BWD = 0.0            # SWIGLU_BWD; measured 0: every element of both kernels is within the rounding term of its bf16 result
EPS_TABLE = 4 * 2.0 ** -24          # rotary, table form: derived (two fp32 products and their difference on fp32 table entries)


def rope_pos_angle(pos):
    """angle accuracy include/opadpo_hip.h states for opadpo_gemm_nt_rope_pos: max(2e-4, 3e-7 * pos) rad"""
    return torch.clamp(3e-7 * pos.to(F64), min=2e-4)


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from opadpo_amd import lib
    lib.load()
    yield lib
    lib.set_flags(True, True)


def dev():
    return torch.device("cuda:0")


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def seed_of(*key):
    """a fresh, stable seed per parameter set"""
    h = 0
    for c in repr(key):
        h = (h * 131 + ord(c)) % 100003
    return h


# ---- which kernels will run ----------------------------------------------------------------------------------------------------------------
def families(text):
    """plan text -> kernel families as the plan prints them: 'gemm_nt_w4s_kernel<true, 0, false> 8 1 256 131072' -> 'w4s'; the tail kernels keep
    their template argument ('tail64<8>')"""
    out = []
    for ln in text.splitlines():
        name = ln.split()[0] if "<" not in ln else ln[:ln.rindex(">") + 1]
        name = name.replace("gemm_nt_", "").replace("_kernel", "")
        out.append(name if name.startswith("tail64") else name.split("<")[0])
    return out


def nt_plan(L, t, M, N, K1, K2, d, out, res, act, var, tr, rope=0):
    f = L.load().opadpo_debug_gemm_nt_plan
    _p, _i = C.c_void_p, C.c_int
    f.restype = _i
    f.argtypes = [_p, _i, _p, _i, _i, _p, _i, _p, _i, _i, _i, _i, _i, _i, _p, _i, _i, _p, _i, _i, _p, _i, _i, C.c_float, _i, _i, _i, _i, _i, C.c_char_p, _i]
    buf = C.create_string_buffer(4096)
    a2, b2 = t.get("a2"), t.get("b2")
    rc = f(t["a1"].data_ptr(), t["a1"].stride(0), t["b1"].data_ptr(), t["b1"].stride(0), K1, L.ptr(a2), a2.stride(0) if a2 is not None else 0,
           L.ptr(b2), b2.stride(0) if b2 is not None else 0, K2, d["a2_group_n"], d["a2_group_stride"], d["a1_group_n"], d["a1_group_stride"],
           out.data_ptr(), out.stride(0), int(out.dtype == F32), L.ptr(res), res.stride(0) if res is not None else 0,
           int(res is not None and res.dtype == F32), L.ptr(t.get("bias")), M, N, d["alpha"], act, var, tr, rope, cus(), buf, 4096)
    assert rc == 0, L.load().opadpo_last_error().decode()
    nt_plan.text = buf.value.decode()          # the whole plan, for the cases that also pin a template argument
    return families(nt_plan.text)


def decode_plan(L, M, N, K, mode, splits, tr):
    f = L.load().opadpo_debug_gemm_nt_decode_plan
    f.restype = C.c_int
    f.argtypes = [C.c_int] * 6 + [C.c_char_p, C.c_int]
    buf = C.create_string_buffer(1024)
    assert f(M, N, K, mode, splits, tr, buf, 1024) == 0, L.load().opadpo_last_error().decode()
    return families(buf.value.decode()), [int(x) for x in buf.value.decode().split()[-4:-2]]


# ---- problems, references (computed once, never modified) and the launch ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def problem(M, N, K1, K2=0, a2g=0, a1g=0, alpha=1.0, bias=False, residual=None, res_cols=None, act=0, p=2, q=2, seed=0):
    d = R.make_nt(M, N, K1, K2, a2_groups=a2g, a1_groups=a1g, seed=seed, p=p, q=q, alpha=alpha, bias=bias, residual=residual, res_cols=res_cols)
    want, v = R.ref_gemm_nt(**d, act=act)
    return d, want, v


def widen(x, extra, gen_seed):
    """x as a column slice (from column `extra`) of a tensor `2 * extra` columns wider, the rest filled with other dyadic numbers"""
    big = R.dyadic((x.shape[0], x.shape[1] + 2 * extra), gen_seed, 2, dtype=x.dtype)
    big[:, extra:extra + x.shape[1]] = x
    return big.to(dev())[:, extra:extra + x.shape[1]]


def to_dev(d, wide=False):
    t = {}
    for i, k in enumerate(("a1", "b1", "a2", "b2", "bias", "residual")):
        if d.get(k) is not None:
            t[k] = widen(d[k], 8, 900 + i) if wide and d[k].dim() == 2 else d[k].to(dev())
    return t


def run_nt(L, d, out_dtype, var, tr, expect, act=0, stream=False, wide=False, out_cols=None):
    """plan assertion, then the launch into a guarded C; returns the result (guards and NaN checked)"""
    M, N, K1, K2 = d["M"], d["N"], d["K1"], d["K2"]
    t = to_dev(d, wide)
    out, guard = R.guarded(M, out_cols or N, out_dtype, device=dev(), pad_cols=24 if wide else 8)
    res = t.get("residual")
    got = nt_plan(L, t, M, N, K1, K2, d, out, res, act | (S_HINT if stream else 0), var, tr)
    assert got == list(expect), f"kernel families {got}, expected {list(expect)}: the case no longer reaches its kernel"
    L.set_flags(var, tr)
    kw = dict(a2=t.get("a2"), b2=t.get("b2"), a2_group_n=d["a2_group_n"], a2_group_stride=d["a2_group_stride"], a1_group_n=d["a1_group_n"],
              a1_group_stride=d["a1_group_stride"], k1=K1, residual=res, bias=t.get("bias"), alpha=d["alpha"], act=act)
    if stream:
        with L.decode_schedule():
            L.gemm_nt(t["a1"], t["b1"], out, **kw)
    else:
        L.gemm_nt(t["a1"], t["b1"], out, **kw)
    torch.cuda.synchronize()
    L.set_flags(True, True)
    guard()
    return out


OPTS = {"plain": {}, "scaled": dict(alpha=0.5, bias=True, residual="bf16"), "res32": dict(residual="f32"), "ba": dict(bias=True, residual="f32"),
        "x2": dict(alpha=2.0), "res16": dict(alpha=0.5, residual="bf16")}


def exact_case(L, shape, opt, out_dtype, var, tr, expect, wide=False, stream=False):
    M, N, K1, K2, a2g, a1g = shape
    d, want, _ = problem(M, N, K1, K2, a2g, a1g, seed=seed_of(shape, opt), **OPTS[opt])
    out = run_nt(L, d, out_dtype, var, tr, expect, wide=wide, stream=stream)
    R.check_exact(out, want, f"gemm_nt {shape} {opt} variant {var} use_tr {tr}")
    return out


DT = [BF, F32]


def with_dtypes(cases):
    """every case with bf16 C and with fp32 C; an fp32 residual goes into an fp32 result only (the residual stream)"""
    return [(*c, dt) for c in cases for dt in DT if not (c[-1] in ("res32", "ba") and dt == BF)]


# ---- gemm_nt, exact --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,opt,dt", with_dtypes([(s, o) for s in [(1, 128, 64, 0, 0, 0), (129, 384, 192, 128, 3, 0), (257, 128, 64, 64, 0, 0)]
                                                     for o in ["plain", "scaled", "res32", "wide"]]))
def test_nt_128x128(L, shape, opt, dt):
    """the 128x128 kernel (variant 4): one row, a ragged second row tile, three A2 groups, the scaled epilogue with bias and residual, operands and C
    as column slices of wider tensors"""
    exact_case(L, shape, "plain" if opt == "wide" else opt, dt, 4, 1, ["kernel_x"], wide=opt == "wide")


W4_CASES = [((257, 512, 192, 0, 0, 0), "plain"), ((300, 256, 64, 64, 0, 0), "plain"), ((513, 768, 192, 64, 3, 0), "plain"),
            ((600, 768, 128, 0, 0, 3), "x2"), ((257, 512, 192, 0, 0, 0), "res32"), ((300, 256, 64, 64, 0, 0), "ba"), ((513, 768, 192, 64, 3, 0), "res16")]


@pytest.mark.parametrize("shape,opt,dt", with_dtypes(W4_CASES))
def test_nt_w4(L, shape, opt, dt):
    """the 256x256 kernel, one tile per workgroup (variant 31): ragged M one past a tile edge, the LoRA tail, three A2 groups of 256, grouped A1, the
    direct-residual and the bias (BA) instantiations"""
    exact_case(L, shape, opt, dt, 31, 1, ["w4"])


@pytest.mark.parametrize("shape,dts", [((300, 256, 8192, 0, 0, 0), [F32]), ((300, 512, 8192, 256, 0, 0), [BF, F32])])
def test_nt_w4_deep_text(L, shape, dts):
    """>= 128 K-tiles: the DEEP text of the 256x256 kernel, and the default text (use_tr bit 11) on the same problem - both exact, hence identical
    bits.  N = 256 with fp32 C, so that the K-fold does not take it."""
    for dt in dts:
        deep = exact_case(L, shape, "plain", dt, 31, 1, ["w4"])
        dflt = exact_case(L, shape, "plain", dt, 31, 1 | NODEEP, ["w4"])
        assert torch.equal(deep.view(torch.int16 if dt == BF else torch.int32), dflt.view(torch.int16 if dt == BF else torch.int32))


@pytest.mark.parametrize("shape,opt,dt", with_dtypes([((1100, 1024, 192, 0, 0, 0), "plain"), ((1100, 1024, 256, 64, 0, 0), "plain"),
                                                     ((1100, 1024, 8256, 0, 0, 0), "plain"), ((1100, 1024, 192, 0, 0, 0), "res32")]))
def test_nt_w4s_streaming_walk(L, shape, opt, dt):
    """the streaming walk on 8 workgroups (use_tr bit 10): 20 tiles, walks of 2-3 tiles; K1 = 3 K-tiles (the first and the two hand-over tiles
    only), a LoRA tail, 129 K-tiles (plan form 3: the DEEP text, pinned through the kernel's last template argument) and the direct fp32 residual"""
    exact_case(L, shape, opt, dt, 10, 1 | W4S_FEW, ["w4s"])
    deep = (shape[2] + shape[3]) // 64 > 128          # plan form 3 = the instantiation w4s<B first, 0, DEEP text>
    assert f", 0, {'true' if deep else 'false'}>" in nt_plan.text, nt_plan.text


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("shape,expect", [((4097, 4096, 192, 0, 0, 0), ["w4", "tail64<8>"]), ((4353, 4096, 192, 0, 0, 0), ["w4", "tail64<4>"]),
                                          ((2305, 8192, 192, 0, 0, 0), ["w4", "kernel_x"])])
def test_nt_tails_after_a_full_round(L, shape, expect, dt):
    """one full round of 256 tiles, then 16 tiles as sixteenth tiles on the deep ring, 32 as sixteenth tiles, 64 as quarter tiles on the 128x128
    kernel: each equal to the exact reference"""
    exact_case(L, shape, "plain", dt, 10, 1, expect)


@pytest.mark.parametrize("M,K", [(40, 1024), (300, 4096)])
def test_nt_k_fold(L, M, K):
    """N = 256 products from K = 1024: the K-folded launch of the 256x256 kernel and gemm_fold2_reduce (bf16 C only; alpha in the reduce pass)"""
    d, want, _ = problem(M, 256, K, alpha=0.5, seed=seed_of("fold", M, K))
    R.check_exact(run_nt(L, d, BF, 10, 1, ["w4", "gemm_fold2_reduce"]), want, f"K-fold M {M} K {K}")


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("shape,opt", [((257, 512, 192, 64, 0, 0), "plain"), ((300, 256, 128, 0, 0, 0), "scaled")])
def test_nt_p8(L, shape, opt, dt):
    """the 8-wave 256x256 kernel (variant 17)"""
    exact_case(L, shape, opt, dt, 17, 1, ["p8"])


SKINNY_SHAPES = [(256, 4096, 0, 0), (384, 192, 128, 3), (16384, 128, 64, 2)]


def skinny_family(M, N, tr):
    return "skinny8" if not (tr & 16) and (M <= 16 or (M <= 32 and N // 32 < 512)) else "skinny"


@pytest.mark.parametrize("tr", [1, 17])
@pytest.mark.parametrize("N,K1,K2,g", SKINNY_SHAPES)
@pytest.mark.parametrize("M", [1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 48, 63, 64])
def test_nt_skinny(L, M, N, K1, K2, g, tr):
    """the weight-streaming kernels for M <= 64 (variant 15; use_tr bit 4 keeps the 16-row form below 17 rows): in-workgroup split-K, the LoRA tail
    as a second K segment, grouped tail columns; plain bf16, the scaled epilogue with bias and a bf16 residual, an fp32 residual into fp32 C; and
    the per-call hint (OPADPO_GEMM_STREAM) on a problem with something fused, which must take the same kernel"""
    fam = [skinny_family(M, N, tr)]
    shape = (M, N, K1, K2, g, 0)
    exact_case(L, shape, "plain", BF, 15, tr, fam)
    exact_case(L, shape, "scaled", BF, 15, tr, fam)
    exact_case(L, shape, "ba", F32, 15, tr, fam)
    exact_case(L, shape, "res32", F32, 10, tr, fam, stream=True)


# ---- opadpo_gemm_nt_decode ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def decode_problem(N, K):
    d = R.make_nt(64, N, K, seed=seed_of("decode", N, K))
    return d["a1"], d["b1"], R.ref_product(d["a1"], d["b1"], K), d["a1"].to(dev()), d["b1"].to(dev())


@pytest.mark.parametrize("kernel,rows", [(0, 0), (0, 1), (0, 2), (0, 3), (1, 0)])
@pytest.mark.parametrize("N,K", [(1024, 512), (4096, 4096)])
@pytest.mark.parametrize("M", [1, 8, 13, 16, 17, 33, 50, 64])
def test_nt_decode(L, M, N, K, kernel, rows):
    """opadpo_gemm_nt_decode: mode 0 (bf16) exact; mode 1: every K-split slice summed in float64 equals the reference exactly, with `splits` the
    value opadpo_gemm_nt_decode_splits returns (by the library, 1 and 3 asked for).  kernel 0 = the whole-line streaming kernel with its weight
    rows per workgroup by shape or forced (use_tr bits 7-8), 1 = the LDS-ring kernel."""
    tr = 1 | (kernel << 5) | (rows << 7)
    fam = ["dec64x" if kernel == 0 else "dec64"]
    _, _, want64, a, w = decode_problem(N, K)
    a, want = a[:M], want64[:M]
    L.set_flags(10, tr)
    try:
        got, _ = decode_plan(L, M, N, K, 0, 1, tr)
        assert got == fam, f"kernel families {got}, expected {fam}"
        out, guard = R.guarded(M, N, BF, device=dev())
        L.call("opadpo_gemm_nt_decode", L.ptr(a), a.stride(0), L.ptr(w), w.stride(0), K, L.ptr(out), out.stride(0), 0, M, N, 1, L.stream())
        torch.cuda.synchronize()
        guard()
        R.check_exact(out, want, f"decode mode 0 M {M}")
        for splits in (0, 1, 3):
            S = L.load().opadpo_gemm_nt_decode_splits(N, K, splits)
            got, grid = decode_plan(L, M, N, K, 1, splits, tr)
            assert got == fam and grid[1] == S and 1 <= S <= K // 64, (got, grid, S)
            part, guard = R.guarded(S * M, N, F32, device=dev())          # slice s = rows [s M, (s + 1) M): the slice stride is M ldc
            L.call("opadpo_gemm_nt_decode", L.ptr(a), a.stride(0), L.ptr(w), w.stride(0), K, L.ptr(part), part.stride(0), 1, M, N, splits, L.stream())
            torch.cuda.synchronize()
            guard()
            total = part.cpu().contiguous().to(F64).view(S, M, N).sum(0)
            R.check_exact(total.to(F32), want, f"decode mode 1 M {M} splits {splits} -> {S}")
            assert torch.equal(total.to(F32).to(F64), total)
    finally:
        L.set_flags(True, True)


# ---- gemm_tn -----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tn_problem(M, N1, N2, groups, seed):
    d = R.make_tn(M, N1, N2, groups, seed=seed)
    return d, R.ref_gemm_tn(**d)


@pytest.mark.parametrize("tr", [1, 9, 0, 13])
@pytest.mark.parametrize("M,N1,N2,groups", [(64, 128, 128, 0), (130, 128, 256, 0), (777, 256, 128, 0), (1100, 512, 256, 0), (1300, 768, 256, 3),
                                            (2100, 1024, 256, 2)])
def test_tn(L, tr, M, N1, N2, groups):
    """C0 + 2 P^T Q with a dyadic fp32 C0: exact despite the fp32 atomics of the K-chunks.  use_tr 1 = the 256x256 stream-K kernel where N1, N2 and
    the group width are multiples of 256 (the last three shapes), the 128x128 kernel elsewhere; 9 / 13 = the 128x128 kernel everywhere; 0 = without
    the transposed LDS reads."""
    d, want = tn_problem(M, N1, N2, groups, seed_of("tn", M, N1, N2, groups))
    c, guard = R.guarded(N1, N2, F32, device=dev(), fill=d["C0"].to(dev()))
    L.set_flags(10, tr)
    try:
        L.gemm_tn(d["P"].to(dev()), d["Q"].to(dev()), c, n2=N2, q_group_n1=d["q_group_n1"], q_group_stride=d["q_group_stride"], alpha=d["alpha"])
        torch.cuda.synchronize()
    finally:
        L.set_flags(True, True)
    guard()
    R.check_exact(c, want, f"gemm_tn {(M, N1, N2, groups)} use_tr {tr}")


def test_tn_group_and_deterministic_form(L):
    """opadpo_gemm_tn_group and opadpo_gemm_tn_group_det on 8 problems of mixed widths sharing M = 1100 (one with grouped Q columns): both equal the
    exact reference, and therefore each other; the workspace is sized by opadpo_gemm_tn_group_workspace_bytes"""
    M = 1100
    shapes = [(256, 256, 0), (512, 256, 0), (256, 768, 0), (768, 256, 3), (1024, 256, 0), (256, 512, 0), (512, 512, 2), (256, 1024, 0)]
    probs = [tn_problem(M, n1, n2, g, seed_of("tng", i)) for i, (n1, n2, g) in enumerate(shapes)]
    n = len(probs)
    P, Q = [d["P"].to(dev()) for d, _ in probs], [d["Q"].to(dev()) for d, _ in probs]
    arr = lambda vals, T=C.c_int: (T * n)(*vals)
    lib = L.load()
    L.set_flags(True, True)
    need = lib.opadpo_gemm_tn_group_workspace_bytes(n, M, arr([s[0] for s in shapes]), arr([s[1] for s in shapes]), arr([d["q_group_n1"] for d, _ in probs]))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev())
    for det in (False, True):
        outs = [R.guarded(s[0], s[1], F32, device=dev(), fill=d["C0"].to(dev())) for s, (d, _) in zip(shapes, probs)]
        a = (n, arr([x.data_ptr() for x in P], C.c_void_p), arr([x.stride(0) for x in P]), arr([x.data_ptr() for x in Q], C.c_void_p),
             arr([x.stride(0) for x in Q]), arr([o.data_ptr() for o, _ in outs], C.c_void_p), arr([o.stride(0) for o, _ in outs]), M,
             arr([s[0] for s in shapes]), arr([s[1] for s in shapes]), arr([d["q_group_n1"] for d, _ in probs]),
             arr([d["q_group_stride"] for d, _ in probs]), 2.0)
        if det:
            L.call("opadpo_gemm_tn_group_det", *a, ws.data_ptr(), need, L.stream())
        else:
            L.call("opadpo_gemm_tn_group", *a, L.stream())
        torch.cuda.synchronize()
        for (o, guard), (_, want), s in zip(outs, probs, shapes):
            guard()
            R.check_exact(o, want, f"gemm_tn_group{'_det' if det else ''} {s}")


# ---- nonlinear epilogues, bounded per element ------------------------------------------------------------------------------------------------
MEASURED = {}


def bounded_case(name, eps, got, want, scale, what):
    """prints the measured figure (worst (|got - want| - rounding term) / scale), then asserts |got - want| <= rounding term + eps * scale per element"""
    rt = R.rounding_term(want, got.dtype)
    err = (got.detach().cpu().to(F64) - want).abs()
    worst = float(((err - rt) / scale).max())
    MEASURED[name] = max(MEASURED.get(name, 0.0), worst)
    print(f"\n[measured] {name}: {worst:.3e} (worst so far {MEASURED[name]:.3e}, bound {eps:.3e}) - {what}")
    R.check_bounded(got, want, rt + eps * scale, what)


ACT_KERNELS = [("x128", 4, 1, ["kernel_x"], False, [(129, 384, 192, 128, 3, 0), (300, 256, 128, 0, 0, 0)]),
               ("w4", 31, 1, ["w4"], False, [(300, 256, 128, 0, 0, 0), (257, 512, 192, 64, 0, 0)]),
               ("p8", 17, 1, ["p8"], False, [(300, 256, 128, 0, 0, 0), (257, 512, 192, 64, 0, 0)]),
               ("skinny8", 15, 1, ["skinny8"], False, [(7, 384, 192, 128, 3, 0)]),
               ("skinny", 15, 1, ["skinny"], False, [(33, 384, 192, 128, 3, 0), (64, 256, 64, 0, 0, 0)])]


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("extras", ["none", "bias_res"])
@pytest.mark.parametrize("act", [R.ACT_QUICK_GELU, R.ACT_GELU])
@pytest.mark.parametrize("kern", ACT_KERNELS, ids=[k[0] for k in ACT_KERNELS])
def test_nt_gelu_epilogues(L, kern, act, extras, dt):
    """quick-GELU and GELU on the exact pre-activation v (p = q = 2, K 64-320: |v| up to about 8), with and without bias and residual:
    |got - want| <= half an ulp of the result + EPS_ACT * max(1, |v|)"""
    _, var, tr, fam, _, shapes = kern
    for shape in shapes:
        M, N, K1, K2, a2g, a1g = shape
        # the BA instantiations of the 256x256 kernel take an fp32 residual into an fp32 result; a bf16 result there carries the bias alone
        res = "f32" if dt == F32 else None if kern[0] == "w4" else "bf16"
        opt = dict(bias=True, residual=res) if extras == "bias_res" else {}
        d, want, v = problem(M, N, K1, K2, a2g, a1g, act=act, seed=seed_of("act", shape, extras, str(dt)), **opt)
        out = run_nt(L, d, dt, var, tr, fam, act=act)
        bounded_case("EPS_ACT", EPS_ACT, out, want, v.abs().clamp(min=1.0), f"act {act} on {fam[0]} {shape} {extras} {dt}")


PAIR_KERNELS = [("w4", 31, 1, ["w4"], (300, 512, 128)), ("w4s", 10, 1 | W4S_FEW, ["w4s"], (1100, 1024, 192)), ("skinny8", 15, 1, ["skinny8"], (7, 512, 192)),
                ("skinny", 15, 1, ["skinny"], (40, 512, 192))]


@pytest.mark.parametrize("kern", PAIR_KERNELS, ids=[k[0] for k in PAIR_KERNELS])
def test_nt_swiglu_pair(L, kern):
    """OPADPO_ACT_SWIGLU_PAIR (weight rows per 128 = [64 gate | 64 up], out [M, N/2] bf16) on the 256x256 kernel, the streaming walk and the skinny
    kernels: silu(gate) * up of the bf16-rounded exact gate / up, within half an ulp + EPS_PAIR * max(1, |gate| |up|)"""
    _, var, tr, fam, (M, N, K) = kern
    d, want, v = problem(M, N, K, act=R.ACT_SWIGLU_PAIR, seed=seed_of("pair", M, N, K))
    out = run_nt(L, d, BF, var, tr, fam, act=R.ACT_SWIGLU_PAIR, out_cols=N // 2)
    bounded_case("EPS_PAIR", EPS_PAIR, out, want, v.clamp(min=1.0), f"SWIGLU_PAIR on {fam[0]} {(M, N, K)}")


BWD_KERNELS = [("w4", 31, 1, ["w4"], (300, 256, 128, 64)), ("w4s", 10, 1 | W4S_FEW, ["w4s"], (1100, 1024, 256, 64))]


@pytest.mark.parametrize("kern", BWD_KERNELS, ids=[k[0] for k in BWD_KERNELS])
def test_nt_swiglu_bwd(L, kern):
    """OPADPO_ACT_SWIGLU_BWD: d_act = the bf16 rounding of the exact product, then the silu_mul_bwd arithmetic on the stored [gate | up] (the
    bf16 residual operand [M, 2N]); out [d_gate | d_up] within half an ulp + EPS_BWD * max(1, |d_act| (1 + |gate|) (1 + |up|))"""
    _, var, tr, fam, (M, N, K1, K2) = kern
    d, want, v = problem(M, N, K1, K2, act=R.ACT_SWIGLU_BWD, residual="bf16", res_cols=2 * N, seed=seed_of("bwd", M, N, K1, K2))
    out = run_nt(L, d, BF, var, tr, fam, act=R.ACT_SWIGLU_BWD, out_cols=2 * N)
    bounded_case("EPS_BWD", EPS_BWD, out, want, v.clamp(min=1.0), f"SWIGLU_BWD on {fam[0]} {(M, N, K1, K2)}")


# ---- rotary epilogues ----------------------------------------------------------------------------------------------------------------------------
def hf_tables(n, theta=10000.0):
    inv = 1.0 / (torch.tensor(theta, dtype=F32) ** (torch.arange(0, 128, 2, dtype=F32) / 128.0))
    ang = torch.arange(n, dtype=F32)[:, None] * inv[None, :]
    return ang.cos(), ang.sin()


ROPE_N, ROPE_COLS, ROPE_K1, ROPE_K2 = 768, 512, 128, 64


def rope_problem(M, seed):
    d = R.make_nt(M, ROPE_N, ROPE_K1, ROPE_K2, a2_groups=3, seed=seed)
    return d, to_dev(d)


def rope_check(name, out, want, v, extra, what):
    """rotated columns: half an ulp + EPS_TABLE (|c1| + |c2|) (+ the angle term); the columns that are not rotated: exact"""
    rc = ROPE_COLS
    R.check_exact(out[:, rc:], want[:, rc:].contiguous(), what + ", unrotated columns")
    got, w, s = out[:, :rc], want[:, :rc].contiguous(), v[:, :rc].contiguous()
    rt = R.rounding_term(w, BF)
    err = (got.detach().cpu().to(F64) - w).abs()
    worst = float(((err - rt) / s.clamp(min=2.0 ** -20)).max())
    print(f"\n[measured] {name}: worst (|got - want| - rounding) / (|c1| + |c2|) = {worst:.3e} - {what}")
    R.check_bounded(got, w, rt + (EPS_TABLE + extra) * s, what)
    return err, rt, s


@pytest.mark.parametrize("S,Lp,seg", [(2, 150, (0, 0)), (2, 200, (120, 40))])
def test_nt_rope_table_form(L, S, Lp, seg):
    """opadpo_gemm_nt_rope with fp32 tables the test passes: y = c1 cos - c2 sin on the exact bf16-rounded projection c, plain rows and packed
    responses (seg = (120, 40), L = 200); rope_cols < N"""
    M = S * Lp
    d, t = rope_problem(M, seed_of("rope", S, Lp, seg))
    cos, sin = hf_tables(Lp)
    rope = dict(cos=cos, sin=sin, L=Lp, rope_cols=ROPE_COLS, seg=seg)
    want, v = R.ref_gemm_nt(**d, rope=rope)
    out, guard = R.guarded(M, ROPE_N, BF, device=dev())
    got = nt_plan(L, t, M, ROPE_N, ROPE_K1, ROPE_K2, d, out, None, 0, 10, 1, rope=1)
    assert got == ["w4"], got
    L.set_flags(True, True)
    L.gemm_nt_rope(t["a1"], t["b1"], out, cos.to(dev()), sin.to(dev()), Lp, ROPE_COLS, seg, a2=t["a2"], b2=t["b2"], a2_group_n=d["a2_group_n"],
                   a2_group_stride=d["a2_group_stride"])
    torch.cuda.synchronize()
    guard()
    rope_check("rope table", out, want, v, 0.0, f"gemm_nt_rope S {S} L {Lp} seg {seg}")


@pytest.mark.parametrize("top", [300, 4095])
def test_nt_rope_table_free_form(L, top):
    """opadpo_gemm_nt_rope_pos: row positions out of order, up to 299 and up to 4095; the table-form bound plus the angle accuracy the header
    states, max(2e-4, 3e-7 pos) rad, times |c1| + |c2|.  (The header said "within 2e-4 rad" for every position; an fp32 emulation of the
    kernel's formula shows 1.2e-7 pos, test_gemm_ref_cpu.py, and the header was corrected.)  Measured on an MI355X, as an angle: 2.2e-5 rad
    over positions up to 300, 2.6e-4 rad up to 4095 - at most 7.8e-8 rad per unit of position over all rows."""
    M = 300
    d, t = rope_problem(M, seed_of("rope_pos", top))
    g = torch.Generator().manual_seed(top)
    pos = torch.randint(0, top + 1, (M,), generator=g, dtype=torch.int32)
    pos[5], pos[17] = top, 0
    want, v = R.ref_gemm_nt(**d, rope=dict(row_pos=pos, theta=10000.0, rope_cols=ROPE_COLS))
    out, guard = R.guarded(M, ROPE_N, BF, device=dev())
    got = nt_plan(L, t, M, ROPE_N, ROPE_K1, ROPE_K2, d, out, None, 0, 10, 1, rope=2)
    assert got == ["w4"], got
    L.set_flags(True, True)
    pos_d = pos.to(dev())
    L.call("opadpo_gemm_nt_rope_pos", L.ptr(t["a1"]), t["a1"].stride(0), L.ptr(t["b1"]), t["b1"].stride(0), ROPE_K1, L.ptr(t["a2"]), t["a2"].stride(0),
           L.ptr(t["b2"]), t["b2"].stride(0), ROPE_K2, d["a2_group_n"], d["a2_group_stride"], L.ptr(out), out.stride(0), M, ROPE_N, L.ptr(pos_d), 10000.0,
           ROPE_COLS, L.stream())
    torch.cuda.synchronize()
    guard()
    ang = rope_pos_angle(pos)[:, None]
    err, rt, s = rope_check("rope_pos", out, want, v, ang, f"gemm_nt_rope_pos positions up to {top}")
    rel = ((err - rt) / s.clamp(min=2.0 ** -20) / pos.to(F64).clamp(min=1.0)[:, None]).max()
    print(f"[measured] rope_pos angle error per unit of position, worst over rows: {float(rel):.3e} rad (header: 3e-7)")
