"""GPU: the attention kernels the model runs, at the shapes it runs them, against the float64 reference of tests/attn_ref.py.

Every case runs the forward and the backward as the product does (no fp32 dQ copy, so head_dim 128 takes the 32-rows-per-wave dQ
kernel) and checks O, dQ, dK and dV per (sequence, head, 64-row tile) and over the whole tensor, the log-sum-exp, delta, the rows that
see no key, and that the fp32-copy route (16-row dQ kernel) gives the same dK / dV bits and a dQ within the dQ bound.  The ragged
layout and the backward's fused inverse rotary embedding are reached through opadpo_debug_attn_fwd / _bwd (test entry points of the
library, not part of include/opadpo_hip.h).  Bounds: at most 2x the worst value measured over this grid on an MI355X (in comments).
The file runs in about 6 s there (41 tests), float64 references included."""
import ctypes as C
import math

import pytest
import torch

import attn_ref as R

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
THETA = 10000.0

# bound = at most 2x the worst value measured over the grid of this file (measured value in the comment)
BOUND = {                       # measured worst over the grid (whole tensor, worst tile)
    "o": (4.6e-3, 5e-3),        # 2.31e-3, 2.58e-3
    "dq": (7.5e-3, 1.05e-2),    # 3.82e-3, 6.04e-3
    "dk": (7.4e-3, 1.55e-2),    # 3.70e-3, 7.88e-3
    "dv": (4.5e-3, 5.5e-3),     # 2.35e-3, 2.92e-3
    "lse": 6.7e-5,              # 3.36e-5 ('rise': |lse| ~ 1e2; 1.08e-5 elsewhere): max abs error over rows that see a key
    "delta": 1e-7,              # 5.32e-8: relative error (from the kernel's own O: only the fp32 sums differ)
    "dq16": 5e-5,               # 2.95e-5: relative difference of the 16-row dQ kernel (fp32-copy route) and the 32-row one
}


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from opadpo_amd import lib
    h = lib.load()
    _p, _i, _f = C.c_void_p, C.c_int, C.c_float
    h.opadpo_debug_attn_fwd.argtypes = [_p, _p, _p, _i, _p, _i, _p, _p, _i, _i, _i, _i, _i, _f, _i, _i, _p, _i, _i, _i, _i, _p]
    h.opadpo_debug_attn_fwd.restype = _i
    h.opadpo_debug_attn_bwd.argtypes = [_p, _p, _p, _i, _p, _p, _i, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _f, _i, _i,
                                        _p, _i, _i, _i, _p, _f, _i, _p]
    h.opadpo_debug_attn_bwd.restype = _i
    lib.set_flags(True, True)
    yield lib
    lib.set_flags(True, True)


def dev():
    return torch.device("cuda:0")


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
SINK = {"sink0": 8, "sink_late": 64 * 10 + 7}          # position of the sink key inside every sequence


def make_inputs(rows, nh, hd, seed, kind="plain", seq_len=None):
    """qkv [rows, 3H] bf16 and dO [rows, H] bf16.  kind: 'plain' N(0, 0.7^2); 'rise': q . k / sqrt(hd) grows by 6-12 per 64-key tile
    (the running maximum moves by more than the forward's rescale threshold at every tile); 'sink0' / 'sink_late': in every sequence of
    seq_len rows one key 30 units above the rest, at position SINK[kind] (tile 0 / tile 10); 'qstd4': q with standard deviation 4."""
    g = torch.Generator().manual_seed(seed)
    H = nh * hd
    q = torch.randn(rows, nh, hd, generator=g) * 0.7
    k = torch.randn(rows, nh, hd, generator=g) * 0.7
    v = torch.randn(rows, nh, hd, generator=g)
    do = torch.randn(rows, H, generator=g)
    rt = math.sqrt(hd)
    if kind == "rise":
        # along one direction u spread over every dimension: q = 512 u + noise, k = b_tile u + noise orthogonal to u.  A small q would need a
        # large b_tile (~1e3 after ten tiles with q . u = 1): dQ's component along u is a sum of dS * b_tile that cancels, and the bf16
        # rounding of dS (the backward's MFMA operand) would dominate it - a limit of the bf16 backward, not of the rescale tested here
        steps = 6.0 + 6.0 * torch.rand(rows // 64 + 1, generator=g)
        level = torch.cumsum(steps, 0)                          # score offset of each 64-key tile
        u = torch.randn(hd, generator=g)
        u = u / u.norm()
        q = q + 512.0 * u
        k = k - (k @ u)[..., None] * u + (level[torch.arange(rows) // 64] * rt / 512.0)[:, None, None] * u
    elif kind in ("sink0", "sink_late"):
        q[:, :, 1] = 2.0
        k[:, :, 1] = 0.0
        k[sink_rows(rows, seq_len or rows, kind), :, 1] = 30.0 * rt / 2.0
    elif kind == "qstd4":
        q = torch.randn(rows, nh, hd, generator=g) * 4.0
        k = torch.randn(rows, nh, hd, generator=g)
    elif kind != "plain":
        raise ValueError(kind)
    qkv = torch.cat([q.reshape(rows, H), k.reshape(rows, H), v.reshape(rows, H)], 1)
    return qkv.to(BF).to(dev()), do.to(BF).to(dev())


def sink_rows(rows, seq_len, kind):
    return torch.arange(0, rows, seq_len) + SINK[kind]


# ---- kernel calls -----------------------------------------------------------------------------------------------------------------------
def run_kernels(L, lay, qkv, dout, km, nh, hd, causal, *, seg=(0, 0), ragged=False, rope_pos=None, use_tr=-1, dq_copy=False, lse_out=True):
    """Forward then backward.  Padded layout with use_tr = -1: the public entry points (what model.py calls); otherwise the test entry
    points.  Outputs start as NaN: a row a kernel forgets to write shows up."""
    rows = lay.rows
    H = nh * hd
    S = len(lay.seqs)
    Ln = lay.L if ragged else lay.padded_L
    scale = hd ** -0.5
    stat_shape = (nh, rows) if ragged else (S, nh, Ln)
    o = torch.full((rows, H), float("nan"), dtype=BF, device=dev())
    lse = torch.full(stat_shape, float("nan"), device=dev()) if lse_out else None
    dqkv = torch.full((rows, 3 * H), float("nan"), dtype=BF, device=dev())
    delta = torch.full(stat_shape, float("nan"), device=dev())
    dq32 = torch.full((rows, H), float("nan"), device=dev()) if dq_copy else None
    st = L.stream()
    q, k, v = qkv.data_ptr(), qkv.data_ptr() + 2 * H, qkv.data_ptr() + 4 * H
    h = L.load()
    meta = lay.meta().to(dev()) if ragged else None
    mp = (meta.data_ptr(), meta.shape[1], lay.n_seg, rows) if ragged else (None, 0, 0, 0)
    public = not ragged and use_tr == -1
    if public:
        L.call("opadpo_attn_fwd", q, k, v, 3 * H, o.data_ptr(), H, L.ptr(lse), L.ptr(km), S, Ln, nh, hd, causal, scale, *seg, st)
    else:
        rc = h.opadpo_debug_attn_fwd(q, k, v, 3 * H, o.data_ptr(), H, L.ptr(lse), L.ptr(km), S, Ln, nh, hd, causal, scale, *seg, *mp, use_tr, st)
        assert rc == 0, h.opadpo_last_error().decode()
    if not lse_out:
        torch.cuda.synchronize()
        return dict(o=o)
    dq, dk, dv = dqkv.data_ptr(), dqkv.data_ptr() + 2 * H, dqkv.data_ptr() + 4 * H
    if public:
        L.call("opadpo_attn_bwd", q, k, v, 3 * H, o.data_ptr(), dout.data_ptr(), H, lse.data_ptr(), L.ptr(km), dq, dk, dv, L.ptr(dq32),
               delta.data_ptr(), S, Ln, nh, hd, causal, scale, *seg, st)
    else:
        rc = h.opadpo_debug_attn_bwd(q, k, v, 3 * H, o.data_ptr(), dout.data_ptr(), H, lse.data_ptr(), L.ptr(km), dq, dk, dv, L.ptr(dq32),
                                     delta.data_ptr(), S, Ln, nh, hd, causal, scale, *seg, *mp, L.ptr(rope_pos), math.log2(THETA), use_tr, st)
        assert rc == 0, h.opadpo_last_error().decode()
    torch.cuda.synchronize()
    return dict(o=o, lse=R.stat_view(lse, lay, nh), delta=R.stat_view(delta, lay, nh), dq=dqkv[:, :H], dk=dqkv[:, H:2 * H],
                dv=dqkv[:, 2 * H:], dq32=dq32)


# ---- checks -----------------------------------------------------------------------------------------------------------------------------
def check(L, lay, nh, hd, causal, qkv, dout, km, *, seg=(0, 0), ragged=False, rope=False, use_tr=-1, copy_route=False):
    """Run the kernels, compare with the reference, assert the bounds; returns the measured values."""
    H = nh * hd
    rows = lay.rows
    rope_pos = None
    if rope:
        rope_pos = torch.cat([torch.arange(b[-1], dtype=torch.int32) + 5 * s for s, (_, b) in enumerate(lay.seqs)]).to(dev())
    kw = dict(seg=seg, ragged=ragged, rope_pos=rope_pos, use_tr=use_tr)
    got = run_kernels(L, lay, qkv, dout, km, nh, hd, causal, **kw)
    ref = R.reference(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], dout, lay, nh, hd ** -0.5, key_mask=km.view(-1) if km is not None else None,
                      o_kernel=got["o"], rope=(rope_pos.long(), THETA) if rope else None)
    seen = ref["seen"]
    valid = skip_unit_rows(lay, km) if (km is not None and causal & 2) else torch.ones(rows, dtype=torch.bool, device=dev())
    for name in ("dq", "dk", "dv", "delta", "lse", "o"):
        assert bool(torch.isfinite(got[name].float()).all()), f"{name}: non-finite values"
    # dQ and dK vanish in exact arithmetic where a row sees one key (dS = 0): their tile floor is 0.1 % of dV's RMS tile norm
    n_tiles = sum(nh * math.ceil(b[-1] / 64) for _, b in lay.seqs)
    g_atol = 1e-3 * float(ref["dv"].norm()) / math.sqrt(n_tiles)
    m, where = {}, {}
    for name, rows_mask in (("o", valid), ("dq", None), ("dk", None), ("dv", None)):
        whole, tile, where[name] = R.tile_relerr(got[name], ref[name], lay, nh, rows_mask, atol=g_atol if name in ("dq", "dk") else 0.0)
        m[name] = (whole, tile)
    okr = (seen & valid)[None, :].expand(nh, rows)
    m["lse"] = float((got["lse"].double() - ref["lse"])[okr].abs().max()) if bool(okr.any()) else 0.0
    m["delta"] = float((got["delta"].double() - ref["delta"]).norm() / (ref["delta"].norm() + 1e-300))
    print("METRIC", m)
    for name in ("o", "dq", "dk", "dv"):
        whole, tile = m[name]
        assert whole < BOUND[name][0] and tile < BOUND[name][1], \
            f"{name}: whole {whole:.3e} worst tile {tile:.3e} at (seq, head, row0) {where[name]}"
    assert m["lse"] < BOUND["lse"], f"lse max abs err {m['lse']:.3e}"
    assert m["delta"] < BOUND["delta"], f"delta rel err {m['delta']:.3e}"
    dead = ~seen
    if bool(dead.any()):
        assert float(got["o"][dead].float().abs().max()) == 0.0, "rows that see no key: O must be exactly 0"
        sent = got["lse"][:, dead]
        assert bool(((sent == -1e30) | (sent == 1e30)).all()), "rows that see no key: lse must be the +-1e30 sentinel"
        assert float(got["dq"][dead].float().abs().max()) == 0.0, "rows that see no key: dQ must be exactly 0"
    if copy_route:
        # fp32 dQ copy requested: the 16-row dQ kernel; the dK / dV kernel and its inputs are the same -> the same bits
        alt = run_kernels(L, lay, qkv, dout, km, nh, hd, causal, dq_copy=True, **kw)
        assert torch.equal(alt["dk"], got["dk"]) and torch.equal(alt["dv"], got["dv"]), "dK / dV differ with the fp32 dQ copy"
        assert torch.equal(alt["o"], got["o"])
        assert torch.equal(alt["dq"], alt["dq32"].to(BF)), "bf16 dQ != the fp32 copy rounded"
        dq16 = float((alt["dq"].double() - got["dq"].double()).norm() / (got["dq"].double().norm() + 1e-300))
        print("METRIC", {"dq16": dq16})
        assert dq16 < BOUND["dq16"], f"16-row vs 32-row dQ rel diff {dq16:.3e}"
        whole, tile, at = R.tile_relerr(alt["dq"], ref["dq"], lay, nh, atol=g_atol)
        assert whole < BOUND["dq"][0] and tile < BOUND["dq"][1], f"16-row dq: whole {whole:.3e} tile {tile:.3e} at {at}"
        m["dq16"] = dq16
    return m, got


def skip_unit_rows(lay, km):
    """Rows whose O and lse the kernels compute under OPADPO_ATTN_SKIP_MASKED_Q.  The forward writes zeros (lse +-1e30) for an aligned
    group of 32 rows of a sequence (a wave of the 32-row kernel; the 16-row kernel skips whole 64-row tiles, i.e. pairs of such groups)
    whose rows are all masked as keys: padding, which nothing downstream reads.  Every other row is compared, masked or not."""
    valid = torch.ones(lay.rows, dtype=torch.bool, device=km.device)
    for r0, b in lay.seqs:
        for j in range(0, b[-1], 32):
            g = slice(r0 + j, r0 + min(j + 32, b[-1]))
            if not bool(km[g].any()):
                valid[g] = False
    return valid


def padded_case(S, Ln, nh, hd, seed, *, seg=(0, 0), left=0, trail=0, resp_pad=0, holes=(), kind="plain"):
    """Inputs of one padded-layout case: key mask with left / trailing padding, right padding of response 0 and holes (s, a, b).
    Rows masked as keys get no output gradient, as in the LLM backward (nothing reads their outputs)."""
    qkv, dout = make_inputs(S * Ln, nh, hd, seed, kind, seq_len=Ln)
    km = torch.ones(S, Ln, dtype=torch.uint8)
    pad = torch.zeros(S, Ln, dtype=torch.bool)
    pad[0, :left] = True
    if trail:
        pad[-1, Ln - trail:] = True
    if resp_pad:
        pad[0, seg[0] + seg[1] - resp_pad: seg[0] + seg[1]] = True
    km[pad] = 0
    for s, a, b in holes:
        km[s, a:b] = 0
    km = km.view(-1).to(dev())
    return qkv, no_grad_on_masked_rows(dout, km), km


def no_grad_on_masked_rows(dout, km):
    d = dout.clone()
    d[km == 0] = 0
    return d


# ---- LLM shapes, padded layout (head_dim 128, causal | skip masked q tiles) --------------------------------------------------------------
@pytest.mark.parametrize("S,Ln,nh,seg,left,trail,resp_pad", [
    (1, 1087, 32, (0, 0), 37, 50, 0),         # the bench sequence: left-padded query, trailing pad
    (2, 1471, 16, (703, 384), 11, 0, 29),     # two packed responses of 384 after a 703-position prefix, response 0 right-padded
    (1, 300, 40, (0, 0), 3, 0, 0),            # 13B heads
    (3, 333, 2, (0, 0), 5, 17, 0),            # nh * S = 6: the plain block order, not the XCD-grouped one
])
def test_llm_padded(L, S, Ln, nh, seg, left, trail, resp_pad):
    qkv, dout, km = padded_case(S, Ln, nh, 128, S * 1000 + Ln, seg=seg, left=left, trail=trail, resp_pad=resp_pad,
                                holes=[(0, 100, 108)] if Ln > 200 else [])
    check(L, R.padded(S, Ln, seg), nh, 128, L.CAUSAL_SKIP_MASKED_Q, qkv, dout, km, seg=seg, copy_route=True)


@pytest.mark.parametrize("Ln", [1, 31, 32, 63, 64, 65, 127, 128, 129, 130, 161])
def test_llm_tile_edges(L, Ln):
    """Lengths at the 64-row blocks of dK/dV and the 128-row blocks / 32-row waves of the forward and dQ kernels."""
    S, nh = 2, 4
    qkv, dout, km = padded_case(S, Ln, nh, 128, 50 + Ln, left=1 if Ln > 2 else 0, trail=Ln // 3)
    check(L, R.padded(S, Ln), nh, 128, L.CAUSAL_SKIP_MASKED_Q, qkv, dout, km, copy_route=True)


# ---- ragged rows through the test entry points ------------------------------------------------------------------------------------------
PREFIXES = [703, 600, 130, 64]
RESPONSES = {1: [[384], [65], [1], [0]],
             2: [[384, 64], [63, 65], [1, 0], [64, 1]],
             3: [[384, 384, 63], [0, 65, 64], [1, 63, 0], [65, 1, 384]]}


def ragged_case(lay, nh, hd, seed, kind="plain"):
    """Key-mask holes inside the prefixes (one covers a whole 64-row tile) and left padding of sequence 1."""
    qkv, dout = make_inputs(lay.rows, nh, hd, seed, kind)
    km = torch.ones(lay.rows, dtype=torch.uint8)
    (r0, _), (r1, _), (r2, _) = lay.seqs[:3]
    km[r0 + 3: r0 + 10] = 0                   # holes inside the prefix (dropped image keys)
    km[r0 + 192: r0 + 256] = 0                # ... one covering a whole 64-row tile
    km[r1: r1 + 5] = 0                        # left padding
    km[r2 + 70: r2 + 71] = 0
    km = km.to(dev())
    return qkv, no_grad_on_masked_rows(dout, km), km


@pytest.mark.parametrize("rope", [False, True])
@pytest.mark.parametrize("n_seg", [1, 2, 3])
def test_ragged(L, n_seg, rope):
    nh = 32
    lay = R.ragged(PREFIXES, RESPONSES[n_seg])
    qkv, dout, km = ragged_case(lay, nh, 128, 300 + n_seg)
    check(L, lay, nh, 128, L.CAUSAL_SKIP_MASKED_Q, qkv, dout, km, ragged=True, rope=rope, copy_route=True)


def test_ragged_equals_padded_with_equal_responses(L):
    """Equal response lengths: the ragged kernels and the padded packed kernels compute the same numbers in the same order -> the same bits."""
    S, nh, pfx, T, K = 2, 8, 200, 100, 2
    Ln = pfx + K * T
    qkv, dout, km = padded_case(S, Ln, nh, 128, 77, seg=(pfx, T), left=4, holes=[(1, 50, 60)])
    a = run_kernels(L, R.padded(S, Ln, (pfx, T)), qkv, dout, km, nh, 128, L.CAUSAL_SKIP_MASKED_Q, seg=(pfx, T))
    b = run_kernels(L, R.ragged([pfx] * S, [[T] * K] * S), qkv, dout, km, nh, 128, L.CAUSAL_SKIP_MASKED_Q, ragged=True)
    for name in ("o", "lse", "delta", "dq", "dk", "dv"):
        assert torch.equal(a[name], b[name]), name


def test_debug_entry_points_check_their_arguments(L):
    h = L.load()
    nh, hd = 2, 128
    lay = R.ragged([10, 20], [[5, 5], [0, 7]])
    rows, H = lay.rows, nh * hd
    qkv = torch.zeros(rows, 3 * H, dtype=BF, device=dev())
    o = torch.zeros(rows, H, dtype=BF, device=dev())
    stat = torch.zeros(nh, rows, device=dev())
    delta = torch.zeros(nh, rows, device=dev())
    dqkv = torch.zeros(rows, 3 * H, dtype=BF, device=dev())
    pos = torch.zeros(rows, dtype=torch.int32, device=dev())
    q, k, v = qkv.data_ptr(), qkv.data_ptr() + 2 * H, qkv.data_ptr() + 4 * H
    st = L.stream()

    def fwd(meta, n_seg, rows_total, Ln=lay.L, causal=3):
        mp = meta.data_ptr() if meta is not None else None
        return h.opadpo_debug_attn_fwd(q, k, v, 3 * H, o.data_ptr(), H, stat.data_ptr(), None, 2, Ln, nh, hd, causal, 0.1, 0, 0,
                                       mp, 4, n_seg, rows_total, -1, st)

    def bwd(meta, rope_pos):
        mp = meta.data_ptr() if meta is not None else None
        return h.opadpo_debug_attn_bwd(q, k, v, 3 * H, o.data_ptr(), o.data_ptr(), H, stat.data_ptr(), None, dqkv.data_ptr(),
                                       dqkv.data_ptr() + 2 * H, dqkv.data_ptr() + 4 * H, None, delta.data_ptr(), 2, lay.L, nh, hd, 3, 0.1,
                                       0, 0, mp, 4, 2, rows, L.ptr(rope_pos), 13.0, -1, st)

    good = lay.meta(4).to(dev())
    assert fwd(good, 2, rows) == 0 and bwd(good, pos) == 0
    torch.cuda.synchronize()
    cases = []
    m = lay.meta(4)
    m[1, 2] = m[1, 1] - 1                     # boundaries going down
    cases.append(("non-decreasing", lambda: fwd(m.to(dev()), 2, rows)))
    cases.append(("rows_total", lambda: fwd(good, 2, rows - 1)))
    cases.append(("longer than L", lambda: fwd(good, 2, rows, Ln=lay.L - 1)))
    cases.append(("rope_pos needs ragged", lambda: bwd(None, pos)))
    cases.append(("meta_stride", lambda: fwd(good, 3, rows)))
    cases.append(("causal", lambda: fwd(good, 2, rows, causal=0)))
    for what, call in cases:
        assert call() != 0, what
        assert h.opadpo_last_error().decode().startswith("opadpo_debug_attn_"), what


# ---- CLIP tower: head_dim 64, non-causal -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_tr", [0, 1, 3])          # process default: bit 0 transposed LDS reads, bit 1 the LDS-DMA forward
@pytest.mark.parametrize("B,T", [(2, 577), (1, 257)])
def test_clip(L, B, T, use_tr):
    nh, hd = 16, 64
    L.set_flags(True, use_tr)
    try:
        qkv, dout = make_inputs(B * T, nh, hd, 900 + T)
        lay = R.padded(B, T, causal=False)
        _, got = check(L, lay, nh, hd, 0, qkv, dout, None)
        # the vision forward of the frozen tower (model.py) asks for no lse: the same O bits
        o2 = run_kernels(L, lay, qkv, dout, None, nh, hd, 0, lse_out=False)["o"]
        assert torch.equal(o2, got["o"])
    finally:
        L.set_flags(True, True)


# ---- structured scores: rescales and near-one-hot rows -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rise", "sink0", "sink_late", "qstd4"])
def test_structured_scores(L, kind):
    S, Ln, nh = 2, 700, 4
    qkv, dout, km = padded_case(S, Ln, nh, 128, 4242, left=6, trail=40, kind=kind)
    if kind in SINK:
        assert bool(km[sink_rows(S * Ln, Ln, kind).to(dev())].all()), "the sink must be a visible key"
    check(L, R.padded(S, Ln), nh, 128, L.CAUSAL_SKIP_MASKED_Q, qkv, dout, km, copy_route=True)


# ---- the 16-row forward and dQ kernels (context flag bit 8), through the test entry points ------------------------------------------------
@pytest.mark.parametrize("tr", [256 | 1, 256])
@pytest.mark.parametrize("case", ["bench", "ragged_rope", "edge129", "rise"])
def test_legacy_16row_kernels(L, case, tr):
    nh = 32 if case in ("bench", "ragged_rope") else 4
    if case == "ragged_rope":
        lay = R.ragged(PREFIXES, RESPONSES[2])
        qkv, dout, km = ragged_case(lay, nh, 128, 302)
        check(L, lay, nh, 128, L.CAUSAL_SKIP_MASKED_Q, qkv, dout, km, ragged=True, rope=True, use_tr=tr)
        return
    S, Ln, kind = {"bench": (1, 1087, "plain"), "edge129": (2, 129, "plain"), "rise": (2, 700, "rise")}[case]
    qkv, dout, km = padded_case(S, Ln, nh, 128, 17 + Ln, left=37 if S == 1 else 1, trail=50, kind=kind)
    check(L, R.padded(S, Ln), nh, 128, L.CAUSAL_SKIP_MASKED_Q, qkv, dout, km, use_tr=tr)
