"""GPU, op level: opadpo_attn_decode_shared - decode attention of n sampled responses per prompt (the items' prefix caches stored once, per-row
suffix caches).  Form 1 (per-row) is bit-identical to opadpo_attn_decode_fused on the materialised per-row cache; form 2 (grouped, MFMA) is exact
on one-hot and uniform probes and within a derived per-element bound of a float64 reference on random data; refusals carry text."""
import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NH, HD = 8, 128                       # 7B head geometry, 8 heads
U = 2.0 ** -8                         # bf16 spacing relative to the value

#        items, n, Lp, max_new, s
SHAPES = [(1, 2, 40, 16, 0), (2, 5, 300, 24, 9), (3, 16, 703, 64, 63), (2, 8, 1100, 32, 20)]
# The shapes above give the grouped form ranges of at most 128 keys: two 64-key tiles, one trip of its tile loop, waves 2 and 3 idle.  DEEP adds
# the recipe's geometry of few ranges: 16 items -> 2 ranges of 384 / 319 keys (6 and 5 tiles: two trips, the second partly live), 32 items ->
# 1 range of 703 keys (11 tiles: three trips, wave 3 idle in the last, the last tile 63 keys) - the cross-trip rescale, the register double buffer
# of the K fragments and the reuse of a wave's LDS tile.
DEEP = [(16, 2, 703, 16, 5), (32, 4, 703, 8, 3)]
ALL = SHAPES + DEEP


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from opadpo_amd import lib
    lib.load()
    return lib


def dev():
    return torch.device("cuda:0")


def ranges_of(items, nh, Lp):
    """the documented prefix key ranges of the grouped form (include/opadpo_hip.h) -> (ranges, keys per range)"""
    R = min(max(1, 256 // (items * nh)), max(1, Lp // 64))
    per = (-(-Lp // R) + 63) // 64 * 64
    return -(-Lp // per), per


def make(items, n, Lp, max_new, s, seed, qscale=1.0, identity_rope=False):
    g = torch.Generator().manual_seed(seed)
    rows, H, max_ctx = items * n, NH * HD, Lp + max_new
    d = dict(items=items, n=n, Lp=Lp, max_new=max_new, s=s, rows=rows, pos=Lp + s, max_ctx=max_ctx)
    qkv = torch.randn(rows, 3 * H, generator=g)
    qkv[:, :H] *= qscale
    d["qkv"] = qkv.to(BF)
    d["kp"], d["vp"] = [torch.randn(items, NH, Lp, HD, generator=g).to(BF) for _ in range(2)]
    d["ks"], d["vs"] = [torch.randn(rows, NH, max_new, HD, generator=g).to(BF) for _ in range(2)]
    pm = torch.ones(items, Lp, dtype=torch.uint8)
    pm[0, :5] = 0                                            # item 0 is left-padded by 5 keys
    d["pmask"] = pm
    th = torch.rand(max_ctx, HD // 2, generator=g) * 6.28
    d["cos"], d["sin"] = (torch.ones_like(th), torch.zeros_like(th)) if identity_rope else (torch.cos(th), torch.sin(th))
    return d


def run_shared(L, d, form, nh=NH, hd=HD, ws_bytes=None, n=None):
    """-> (o [rows, nh*hd] bf16, ks, vs after the append) on the device; the inputs' suffix caches are copied first"""
    t = {k: v.to(dev()) for k, v in d.items() if torch.is_tensor(v)}
    ks, vs = t["ks"].clone(), t["vs"].clone()
    n = d["n"] if n is None else n
    need = L.load().opadpo_attn_decode_shared_workspace_bytes(d["items"], n, nh, hd, d["Lp"], d["max_new"])
    wsb = need if ws_bytes is None else ws_bytes
    ws = torch.zeros(max(wsb, 4), dtype=torch.uint8, device=dev())
    o = torch.full((d["rows"], nh * hd), 7.0, dtype=BF, device=dev())
    pos_d = torch.tensor([d["pos"]], dtype=torch.int32, device=dev())
    L.call("opadpo_attn_decode_shared", L.ptr(t["qkv"]), 3 * nh * hd, L.ptr(t["cos"]), L.ptr(t["sin"]), L.ptr(t["kp"]), L.ptr(t["vp"]), L.ptr(ks), L.ptr(vs),
           L.ptr(o), L.ptr(t["pmask"]), d["items"], n, nh, hd, L.ptr(pos_d), d["Lp"], d["max_new"], hd ** -0.5, L.ptr(ws), wsb, form, L.stream())
    torch.cuda.synchronize()
    return o, ks, vs


def run_fused(L, d):
    """opadpo_attn_decode_fused on the materialised per-row cache -> (o, k cache, v cache)"""
    t = {k: v.to(dev()) for k, v in d.items() if torch.is_tensor(v)}
    rows, n, Lp, s, max_ctx = d["rows"], d["n"], d["Lp"], d["s"], d["max_ctx"]
    item = torch.arange(rows, device=dev()) // n
    kc = torch.zeros(rows, NH, max_ctx, HD, dtype=BF, device=dev())
    vc = torch.zeros_like(kc)
    kc[:, :, :Lp], vc[:, :, :Lp] = t["kp"][item], t["vp"][item]
    kc[:, :, Lp:Lp + s], vc[:, :, Lp:Lp + s] = t["ks"][:, :, :s], t["vs"][:, :, :s]
    km = torch.ones(rows, max_ctx, dtype=torch.uint8, device=dev())
    km[:, :Lp] = t["pmask"][item]
    wsb = L.load().opadpo_attn_decode_workspace_bytes(rows, NH, HD, max_ctx)
    ws = torch.zeros(max(wsb, 4), dtype=torch.uint8, device=dev())
    o = torch.empty(rows, NH * HD, dtype=BF, device=dev())
    pos_d = torch.tensor([d["pos"]], dtype=torch.int32, device=dev())
    L.call("opadpo_attn_decode_fused", L.ptr(t["qkv"]), 3 * NH * HD, L.ptr(t["cos"]), L.ptr(t["sin"]), L.ptr(kc), L.ptr(vc), L.ptr(o), L.ptr(km), rows, NH, HD,
           L.ptr(pos_d), max_ctx, HD ** -0.5, L.ptr(ws), wsb, L.stream())
    torch.cuda.synchronize()
    return o, kc, vc


_FORM1 = {}


def form1(L, shape, qscale=1.0):
    """form 1's result per case, computed once and shared (never written to)"""
    key = (shape, qscale)
    if key not in _FORM1:
        d = make(*shape, seed=100 + ALL.index(shape), qscale=qscale)
        _FORM1[key] = (d,) + run_shared(L, d, 1)
    return _FORM1[key]


bits = lambda t: t.contiguous().view(torch.int16)


@pytest.mark.parametrize("shape", ALL)
def test_form1_is_the_fused_kernel_bit_for_bit(L, shape):
    d, o, ks, vs = form1(L, shape)
    o_ref, kc, vc = run_fused(L, d)
    bad = (bits(o) != bits(o_ref)).view(d["rows"], NH, HD)
    assert not bool(bad.any()), (int(bad.sum()), bad.any(-1).nonzero()[:8].tolist(), float((o.float() - o_ref.float()).abs().max()))
    s, pos = d["s"], d["pos"]
    assert torch.equal(bits(ks[:, :, s]), bits(kc[:, :, pos])) and torch.equal(bits(vs[:, :, s]), bits(vc[:, :, pos]))
    # nothing but slot s of the suffix caches was written
    keep = torch.ones(d["max_new"], dtype=torch.bool)
    keep[s] = False
    assert torch.equal(bits(ks[:, :, keep]), bits(d["ks"][:, :, keep].to(dev()))) and torch.equal(bits(vs[:, :, keep]), bits(d["vs"][:, :, keep].to(dev())))


def reference(d, k_new):
    """float64 attention from the same bf16 inputs: rotated q rounded to bf16 (fp32 rotation, as the kernels compute it), the appended key as
    form 1 stored it (rotated, bf16) -> (ref [rows, NH, HD], A = sum_j p_j |v_j|)"""
    rows, n, Lp, s, H = d["rows"], d["n"], d["Lp"], d["s"], NH * HD
    d = {k: (v.to(dev()) if torch.is_tensor(v) else v) for k, v in d.items()}
    q = d["qkv"][:, :H].float().view(rows, NH, HD)
    c, sn = d["cos"][d["pos"]], d["sin"][d["pos"]]
    x1, x2 = q[..., :HD // 2], q[..., HD // 2:]
    q = torch.cat([x1 * c - x2 * sn, x2 * c + x1 * sn], -1).to(BF).double()
    v_new = d["qkv"][:, 2 * H:].double().view(rows, NH, HD)
    item = torch.arange(rows, device=dev()) // n
    K = torch.cat([d["kp"][item].double(), d["ks"][:, :, :s].double(), k_new.double()[:, :, None]], 2)      # [rows, NH, Lp + s + 1, HD]
    V = torch.cat([d["vp"][item].double(), d["vs"][:, :, :s].double(), v_new[:, :, None]], 2)
    vis = torch.cat([d["pmask"][item].bool(), torch.ones(rows, s + 1, dtype=torch.bool, device=dev())], 1)
    sc = torch.einsum("rhd,rhkd->rhk", q, K) * HD ** -0.5
    sc = sc.masked_fill(~vis[:, None, :], float("-inf"))
    p = torch.softmax(sc, -1)
    return torch.einsum("rhk,rhkd->rhd", p, V).cpu(), torch.einsum("rhk,rhkd->rhd", p, V.abs()).cpu()


@pytest.mark.parametrize("shape,qscale", [(sh, 1.0) for sh in ALL] + [(SHAPES[2], 8.0), (DEEP[1], 8.0)])
def test_form2_against_float64(L, shape, qscale):
    """|o - ref| <= 2u (|ref| + A), u = 2^-8, A = sum_j p_j |v_j|, per element: one bf16 rounding of each weight (<= u A), one bf16 rounding of the
    output (<= u |ref|), a factor of 2 over the sum.  q scaled by 8: peaked weights.  The appended K/V carry form 1's bits."""
    d, _, ks1, vs1 = form1(L, shape, qscale)
    o, ks, vs = run_shared(L, d, 2)
    assert torch.equal(bits(ks), bits(ks1)) and torch.equal(bits(vs), bits(vs1))
    ref, A = reference(d, ks1[:, :, d["s"]])
    err = (o.double().cpu().view(d["rows"], NH, HD) - ref).abs()
    bound = 2 * U * (ref.abs() + A)
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"form 2 {shape} q x{qscale}: max |err| / bound = {worst:.3f}, max |err| = {float(err.max()):.3e}")
    assert bool((err <= bound).all()), (int((err > bound).sum()), worst)
    o0, _, _ = run_shared(L, d, 0)                         # the library's choice for n >= 2 at head_dim 128 is the grouped form
    assert torch.equal(bits(o0), bits(o))


def _probe_case(items=2, n=5, Lp=300, max_new=24, s=9):
    d = make(items, n, Lp, max_new, s, seed=1, identity_rope=True)
    H, rows = NH * HD, items * n
    ar = torch.arange
    enc = lambda a, b: (((a[:, None, None, None] * 37 + b[None, None, :, None] * 3 + ar(NH)[None, :, None, None] * 5 + ar(HD)[None, None, None, :]) % 251) - 125)
    d["vp"] = enc(ar(items), ar(Lp)).to(BF)                 # distinct small integers per (item, slot), exact in bf16
    d["vs"] = enc(ar(rows) + 60, ar(max_new) + 400).to(BF)
    d["kp"], d["ks"] = torch.zeros_like(d["kp"]), torch.zeros_like(d["ks"])
    qkv = torch.zeros(rows, 3 * H)
    qkv[:, :H] = 4.0
    qkv[:, 2 * H:] = ((ar(rows)[:, None] * 13 + ar(H)[None, :]) % 251 - 125).float()
    d["qkv"] = qkv.to(BF)
    return d


def test_form2_one_hot_probes(L):
    """q = 4.0 everywhere, K = 0 but the probed key = 4.0: its scaled score is ~181 above the rest, every other weight underflows, the output is the
    probed key's V row exactly.  The prefix is shared by an item's rows, so a call probes one prefix key per item (different ones in the two items)
    or, in an item, a different suffix key per row: slot 0, the newly appended key, and the slots between.  Prefix probes: the first and last key,
    the first key after the left pad, both sides of every key-range boundary of the launch and of the 64-key tiles next to them."""
    base = _probe_case()
    items, n, Lp, s, rows, H = base["items"], base["n"], base["Lp"], base["s"], base["rows"], NH * HD
    R, per = ranges_of(items, NH, Lp)
    assert R == 3 and per == 128
    edges = sorted({b + o for k in range(1, R) for b in (k * per,) for o in (-1, 0)} | {63, 64, 191, 192, 255, 256})
    probes = {0: [5, Lp - 1] + edges + ["suffix"], 1: [0, Lp - 1] + edges[::-1] + ["suffix"]}
    slot_of_row = [0, s, 1, s - 1, 2][:n]
    for call in range(len(probes[0])):
        d = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in base.items()}
        want = torch.empty(rows, NH, HD)
        for it in range(items):
            p = probes[it][call]
            for j in range(n):
                r = it * n + j
                if p == "suffix":
                    sl = slot_of_row[j]
                    if sl == s:
                        d["qkv"][r, H:2 * H] = 4.0                  # the newly appended key
                        want[r] = d["qkv"][r, 2 * H:].float().view(NH, HD)
                    else:
                        d["ks"][r, :, sl] = 4.0
                        want[r] = d["vs"][r, :, sl].float()
                else:
                    d["kp"][it, :, p] = 4.0
                    want[r] = d["vp"][it, :, p].float()
        o, _, _ = run_shared(L, d, 2)
        got = o.float().cpu().view(rows, NH, HD)
        assert torch.equal(got, want), (call, [probes[i][call] for i in range(items)], (got != want).any(-1).nonzero()[:6].tolist())
    # a masked prefix key carrying 8.0 loses to the visible 4.0 key
    d = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in base.items()}
    d["kp"][0, :, 2] = 8.0
    d["kp"][0, :, 5] = 4.0
    d["kp"][1, :, 70] = 4.0
    o, _, _ = run_shared(L, d, 2)
    got = o.float().cpu().view(rows, NH, HD)
    assert torch.equal(got[:n], d["vp"][0, :, 5].float().expand(n, NH, HD)) and torch.equal(got[n:], d["vp"][1, :, 70].float().expand(n, NH, HD))


@pytest.mark.parametrize("items,R_want,per_want", [(16, 2, 384), (32, 1, 704)])
def test_form2_one_hot_probes_across_trips(L, items, R_want, per_want):
    """The same probes where a range spans several trips of the tile loop (4 waves x 64 keys per trip): the first and last key of EVERY 64-key tile
    (so every wave and every trip holds the hot key once, among them both sides of the trip boundaries at 256 and 512 keys into a range and of the
    range boundary), the first key after the left pad, the last prefix key.  Every item probes a different key in a call."""
    n, Lp, max_new, s = 2, 703, 8, 3
    base = _probe_case(items, n, Lp, max_new, s)
    assert ranges_of(items, NH, Lp) == (R_want, per_want)
    plist = sorted({k for t in range((Lp + 63) // 64) for k in (64 * t, min(64 * t + 63, Lp - 1))} | {5, Lp - 1, min(per_want - 1, Lp - 1), min(per_want, Lp - 1)})
    assert {255, 256, 511, 512} <= set(plist)
    rows = items * n
    for call in range(-(-len(plist) // items)):
        d = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in base.items()}
        want = torch.empty(rows, NH, HD)
        keys = []
        for it in range(items):
            p = plist[(call * items + it) % len(plist)]
            p = 5 if it == 0 and p < 5 else p                # item 0: keys 0..4 are the left pad
            keys.append(p)
            d["kp"][it, :, p] = 4.0
            want[it * n:(it + 1) * n] = d["vp"][it, :, p].float()
        o, _, _ = run_shared(L, d, 2)
        got = o.float().cpu().view(rows, NH, HD)
        bad = (got != want).any(-1).any(-1).view(items, n).any(1).nonzero().flatten().tolist()
        assert not bad, (call, [(i, keys[i]) for i in bad][:8])


def test_form2_uniform_weights(L):
    """K = 0, V in {0, 1}, exactly 256 visible keys (246 prefix keys + 9 suffix slots + the new key): every output element is count / 256 exactly
    (representable in bf16 for every count in 0..256)."""
    d = _probe_case()
    items, n, Lp, s, rows, H = d["items"], d["n"], d["Lp"], d["s"], d["rows"], NH * HD
    g = torch.Generator().manual_seed(5)
    d["vp"] = torch.randint(0, 2, d["vp"].shape, generator=g).to(BF)
    d["vs"] = torch.randint(0, 2, d["vs"].shape, generator=g).to(BF)
    d["qkv"][:, 2 * H:] = torch.randint(0, 2, (rows, H), generator=g).to(BF)
    pm = torch.ones(items, Lp, dtype=torch.uint8)
    pm[0, :54] = 0                                            # a left pad of 54 keys
    pm[1, torch.randperm(Lp, generator=g)[:54]] = 0           # 54 masked keys scattered over the ranges
    d["pmask"] = pm
    assert int(pm[0].sum()) + s + 1 == 256 and int(pm[1].sum()) + s + 1 == 256
    o, _, _ = run_shared(L, d, 2)
    item = torch.arange(rows) // n
    vis = pm[item].bool()
    count = (d["vp"][item].float() * vis[:, None, :, None]).sum(2) + d["vs"][:, :, :s].float().sum(2) + d["qkv"][:, 2 * H:].float().view(rows, NH, HD)
    got = o.float().cpu().view(rows, NH, HD)
    assert torch.equal(got, count / 256.0), (got != count / 256.0).nonzero()[:6].tolist()


def test_refusals_carry_text(L):
    d = make(2, 3, 100, 8, 2, seed=3)
    with pytest.raises(L.OpadpoError, match="head_dim 128"):
        d64 = dict(d, qkv=d["qkv"][:, :3 * NH * 64].contiguous(), kp=d["kp"][..., :64].contiguous(), vp=d["vp"][..., :64].contiguous(),
                   ks=d["ks"][..., :64].contiguous(), vs=d["vs"][..., :64].contiguous(), cos=d["cos"][:, :32].contiguous(), sin=d["sin"][:, :32].contiguous())
        run_shared(L, d64, 2, hd=64)
    with pytest.raises(L.OpadpoError, match="16"):
        run_shared(L, d, 1, n=17)
    need = L.load().opadpo_attn_decode_shared_workspace_bytes(2, 3, NH, HD, 100, 8)
    assert need > 0
    with pytest.raises(L.OpadpoError, match="workspace"):
        run_shared(L, d, 2, ws_bytes=need - 4)
    o, _, _ = run_shared(L, d, 2)                             # the calls above launched nothing and left nothing behind
    assert bool(torch.isfinite(o.float()).all())
