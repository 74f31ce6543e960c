"""GPU: continuous batching for the rollout.  Op level: opadpo_attn_decode_fused_rows and opadpo_sample_rows against the scalar-position /
scalar-step forms they generalise, bit for bit.  End to end on the tiny parity fixture: a session of S slots fed N prompts against static
`Generator.generate` batches of S rows - prompt i, admitted into slot s with seed + i, must read exactly row s of a static batch that holds it at
row s with that seed - for the three adapter kinds, the three decode GEMM regimes, eager and graph replay, with EOS, caps, log-probs and idle slots.
Everything here is an equality of bits: the kernels of a session compute a row from that row's state alone."""
import json
import os

import pytest
import torch

from test_parity_gpu import setup  # noqa: F401  (module fixture of the parity suite: oracle weights, adapters, CtxEngine)

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
EOS, PAD = 2, 0
NAN_BF16 = 0x7FC1                   # a bf16 NaN bit pattern: what an uninitialised cache slot may hold


def _lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from opadpo_amd import lib as L
    L.load()
    return L


# ---- 1. ragged decode attention, op level ---------------------------------------------------------------------------------------------------
def _boundary(lo, max_ctx, ranges, ng):
    """a position on a key-range boundary under the kernel's rule (per = ceil(ceil(ctx / ranges) / ng) * ng with ctx = pos + 1): the first key of
    a range where such a position exists (it is then the only key of the last non-empty range); with two ranges the second one starts at about
    ctx / 2 and the newest key can never open it, so there the first position past a multiple of ranges * ng is taken: `per` has just grown by
    one workgroup step and the boundary between the ranges has moved"""
    for pos in range(lo + 1, max_ctx - 1):
        ctx = pos + 1
        per = -(-(-(-ctx // ranges)) // ng) * ng
        if pos % per == 0 and pos >= per:
            return pos
    return (lo // (ranges * ng) + 1) * ranges * ng


# (B, nh, hd, max_ctx, key ranges, keys per workgroup step): the launch regimes of attn_decode_splits / attn_decode_fat
ATTN_CASES = [(3, 2, 128, 1024, 4, 64), (3, 2, 64, 1024, 4, 128), (12, 32, 128, 512, 2, 16), (40, 32, 128, 512, 2, 16), (64, 32, 128, 512, 1, 16)]


@pytest.mark.parametrize("B,nh,hd,max_ctx,ranges,ng", ATTN_CASES)
def test_attn_decode_rows_equals_fused_per_row(B, nh, hd, max_ctx, ranges, ng):
    L = _lib()
    lib = L.load()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1000 * B + hd)
    H, Lp = nh * hd, 40
    ws_bytes = int(lib.opadpo_attn_decode_workspace_bytes(B, nh, hd, max_ctx))
    assert (ws_bytes // (B * nh * (hd + 2) * 4) if ws_bytes else 1) == ranges, "the case no longer reaches the regime it is listed for"
    edge = _boundary(Lp, max_ctx, ranges, ng) if ranges > 1 else None
    assert ranges == 1 or edge is not None
    # one row at its first decode position, one at max_ctx - 1, one on a range boundary (where there are ranges), the rest spread
    spread = [Lp + 1 + (7 * Lp + 97 * k) % (max_ctx - Lp - 2) for k in range(3)]
    pool = [Lp, max_ctx - 1] + ([edge] if edge is not None else []) + spread
    pos = [pool[b % len(pool)] for b in range(B)]
    assert all(Lp <= p < max_ctx for p in pos)
    qkv = torch.randn(B, 3 * H, device=dev, generator=g).to(BF)
    kc0 = torch.randn(B, nh, max_ctx, hd, device=dev, generator=g).to(BF)
    vc0 = torch.randn(B, nh, max_ctx, hd, device=dev, generator=g).to(BF)
    key_mask = torch.ones(B, max_ctx, dtype=torch.uint8, device=dev)
    for b in range(B):
        key_mask[b, :b % 5] = 0                                  # left padding
        kc0[b, :, pos[b]:].view(torch.int16).fill_(NAN_BF16)     # slots from the row's position on: poison (the slot at pos is appended)
        vc0[b, :, pos[b]:].view(torch.int16).fill_(NAN_BF16)
    inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd))
    ang = torch.arange(max_ctx, dtype=torch.float32)[:, None] * inv[None, :]
    cos, sin = ang.cos().contiguous().to(dev), ang.sin().contiguous().to(dev)
    ws = torch.zeros(max(ws_bytes, 4), dtype=torch.uint8, device=dev)
    scale = hd ** -0.5

    def run(name, kc, vc, pos_t):
        o = torch.full((B, H), float("nan"), dtype=BF, device=dev)
        L.call(name, L.ptr(qkv), 3 * H, L.ptr(cos), L.ptr(sin), L.ptr(kc), L.ptr(vc), L.ptr(o), L.ptr(key_mask), B, nh, hd, L.ptr(pos_t), max_ctx, scale,
               L.ptr(ws), ws_bytes, L.stream())
        torch.cuda.synchronize()
        return o

    kc, vc = kc0.clone(), vc0.clone()
    o = run("opadpo_attn_decode_fused_rows", kc, vc, torch.tensor(pos, dtype=torch.int32, device=dev))
    assert bool(torch.isfinite(o.float()).all()), "a row read a cache slot behind its position"
    i16 = lambda t: t.view(torch.int16)
    for p in sorted(set(pos)):
        rows = [b for b in range(B) if pos[b] == p]
        kr, vr = kc0.clone(), vc0.clone()
        want = run("opadpo_attn_decode_fused", kr, vr, torch.tensor([p], dtype=torch.int32, device=dev))
        for b in rows:
            assert torch.equal(i16(o[b]), i16(want[b])), (b, p)
            assert torch.equal(i16(kc[b, :, p]), i16(kr[b, :, p])) and torch.equal(i16(vc[b, :, p]), i16(vr[b, :, p])), (b, p)
    # nothing but the slot at the row's own position was written
    for b in range(B):
        kc[b, :, pos[b]] = kc0[b, :, pos[b]]
        vc[b, :, pos[b]] = vc0[b, :, pos[b]]
    assert torch.equal(i16(kc), i16(kc0)) and torch.equal(i16(vc), i16(vc0))


# ---- 2. sampler with a step / seed / cap per row, op level ----------------------------------------------------------------------------------
@pytest.mark.parametrize("V,ldl", [(512, 512), (32000, 32000), (510, 512)], ids=["V512", "V32000", "V510-generic"])
def test_sample_rows_equals_scalar_sampler(V, ldl):
    """V = 512 / 32000: the kernel that keeps the row in LDS; V = 510 (not a multiple of 4): the generic kernel"""
    L = _lib()
    dev = torch.device("cuda:0")
    rows, T = 5, 9
    g = torch.Generator().manual_seed(V)
    logits = torch.zeros(rows, ldl)
    logits[:, :V] = 3.0 * torch.randn(rows, V, generator=g)
    logits = logits.to(dev)
    seeds = [11, 2 ** 40 + 5, 7, 99, 2 ** 63 + 1]
    steps = [0, 3, 7, 2, 5]
    caps = [9, 4, 9, 9, 9]                           # row 1 writes its cap-th token
    fin0 = [0, 0, 0, 1, 0]                           # row 3 is finished
    cfg = (0.8, 30, 0.95)

    def scalar(b):                                   # opadpo_sample with the row's (seed, step) as scalars, no finished flags
        out = torch.full((rows,), -5, dtype=torch.int32, device=dev)
        L.call("opadpo_sample", L.ptr(logits), ldl, rows, V, *cfg, seeds[b] % 2 ** 64, steps[b], None, None, PAD, -1, L.ptr(out), None, L.stream())
        torch.cuda.synchronize()
        return int(out[b])

    want = [scalar(b) for b in range(rows)]
    assert len(set(want)) > 1

    def rows_call(eos):
        seed_t = torch.tensor([s - 2 ** 64 if s >= 2 ** 63 else s for s in seeds], dtype=torch.int64, device=dev)
        step_t = torch.tensor(steps, dtype=torch.int32, device=dev)
        cap_t = torch.tensor(caps, dtype=torch.int32, device=dev)
        fin = torch.tensor(fin0, dtype=torch.uint8, device=dev)
        out = torch.full((rows,), -5, dtype=torch.int32, device=dev)
        hist = torch.full((rows, T), -7, dtype=torch.int32, device=dev)
        L.call("opadpo_sample_rows", L.ptr(logits), ldl, rows, V, *cfg, L.ptr(seed_t), L.ptr(step_t), L.ptr(cap_t), T, L.ptr(fin), PAD, eos, L.ptr(out),
               L.ptr(hist), L.stream())
        torch.cuda.synchronize()
        return out.tolist(), hist.cpu(), step_t.tolist(), fin.tolist(), (seed_t, step_t, cap_t, fin, out, hist)

    out, hist, step1, fin, state = rows_call(-1)
    live = [b for b in range(rows) if not fin0[b]]
    assert [out[b] for b in live] == [want[b] for b in live] and out[3] == PAD
    expect = torch.full((rows, T), -7, dtype=torch.int32)
    for b in live:
        expect[b, steps[b]] = want[b]                # the row's own step, row-major; a finished row writes no history slot
    assert torch.equal(hist, expect)
    assert step1 == [s + (0 if fin0[b] else 1) for b, s in enumerate(steps)], "a live row advances by one, a finished row does not"
    assert fin == [0, 1, 0, 1, 0], "only the row at step == cap - 1 finishes (and the finished one stays finished)"
    # a second launch on the same state: rows 1 and 3 are idle now - pad, no history slot, no step
    seed_t, step_t, cap_t, fin_t, out_t, hist_t = state
    L.call("opadpo_sample_rows", L.ptr(logits), ldl, rows, V, *cfg, L.ptr(seed_t), L.ptr(step_t), L.ptr(cap_t), T, L.ptr(fin_t), PAD, -1, L.ptr(out_t),
           L.ptr(hist_t), L.stream())
    torch.cuda.synchronize()
    assert out_t[1] == PAD and out_t[3] == PAD and step_t.tolist() == [2, 4, 9, 2, 7] and fin_t.tolist() == [0, 1, 1, 1, 0]
    assert torch.equal(hist_t[1].cpu(), expect[1]) and torch.equal(hist_t[3].cpu(), expect[3]) and int(hist_t[2, 8]) >= 0
    # EOS: the row that draws it finishes, with its token written
    out, hist, step1, fin, _ = rows_call(want[0])
    assert out[0] == want[0] and int(hist[0, 0]) == want[0] and fin[0] == 1 and step1[0] == 1
    assert [fin[b] for b in (2, 4)] == [int(want[b] == want[0]) for b in (2, 4)]


# ---- the tiny model: sessions against static batches --------------------------------------------------------------------------------------
SAMPLED = dict(temperature=1.0, top_k=30, top_p=0.95)
GREEDY = dict(temperature=0, top_k=0, top_p=1.0)
CAPS11 = [24, 1, 4, 5, 3, 9, 24, 1, 4, 5, 9]      # 1, 4 (a check boundary: finished after 3 steps... and 5 after exactly 4) and 24 occur; 3 and 9 are off the boundaries
SEED = 40
_STATIC = {}
_FEATS = {}


def _prompts(s, N):
    from test_return_sequences_gpu import prompts
    if N not in _FEATS:
        images, queries, qmask = prompts(s["d"], N, seed=900 + N)
        _FEATS[N] = (queries, qmask, s["eng"].encode_images(images.to(s["dev"])))
    return _FEATS[N]


def _static_row(s, kind, N, i, slot, S, T, mode, eos):
    """row `slot` of Generator.generate over S rows that hold prompt i (at every row), seed SEED + i -> (tokens, logp, ent); computed once per key"""
    from test_return_sequences_gpu import generator_of
    key = (kind, N, i, slot, S, T, mode, eos)
    if key not in _STATIC:
        queries, qmask, feats = _prompts(s, N)
        gen, _ = generator_of(s, kind)
        cfg = SAMPLED if mode == "sampled" else GREEDY
        got = gen.generate(queries[i:i + 1].repeat(S, 1), qmask[i:i + 1].repeat(S, 1), image_feats=feats[i:i + 1].repeat(S, 1, 1).contiguous(),
                           max_new_tokens=T, seed=SEED + i, eos_token_id=eos, output_logprobs=True, **cfg)
        for r in range(S):                           # every row of the batch is a reference for (prompt i, slot r): keep them all
            _STATIC[(kind, N, i, r, S, T, mode, eos)] = tuple(t[r].cpu() for t in got)
    return _STATIC[key]


def _session(s, kind, N, S, T, caps, mode, eos=EOS, use_graph=False, check_every=4, **kw):
    from test_return_sequences_gpu import generator_of
    queries, qmask, feats = _prompts(s, N)
    gen, _ = generator_of(s, kind, use_graph)
    cfg = SAMPLED if mode == "sampled" else GREEDY
    return gen.generate_continuous(queries, qmask, image_feats=feats, slots=S, max_new_tokens=T, seed=SEED, eos_token_id=eos,
                                   max_new_tokens_per_prompt=caps, check_every=check_every, return_schedule=True, **cfg, **kw)


def _lengths(toks, caps, eos):
    out = []
    for row, cap in zip(toks.tolist(), caps):
        row = row[:cap]
        out.append(row.index(eos) + 1 if eos in row else cap)
    return out


def _check_session(s, kind, N, S, T, caps, mode, toks, sched, eos=EOS, check_every=4, lp=None, ent=None):
    from opadpo_amd.generate import plan_continuous
    toks = toks.cpu()
    assert toks.shape == (N, T) and toks.dtype == torch.int64
    lens = _lengths(toks, caps, eos)
    plan, total = plan_continuous(lens, S, check_every)
    assert [tuple(x) for x in sched] == plan, (sched, plan)
    for i in range(N):
        slot = sched[i][0]
        w_tok, w_lp, w_ent = _static_row(s, kind, N, i, slot, S, T, mode, eos)
        c = caps[i]
        assert torch.equal(toks[i, :c], w_tok[:c]), (kind, S, mode, i, slot, toks[i].tolist(), w_tok.tolist())
        assert bool((toks[i, c:] == PAD).all()), (i, toks[i].tolist())
        if lp is not None:
            g_lp, g_ent = lp[i].cpu(), ent[i].cpu()
            assert torch.equal(g_lp[:c].view(torch.int32), w_lp[:c].view(torch.int32)) and torch.equal(g_ent[:c].view(torch.int32), w_ent[:c].view(torch.int32)), i
            assert bool((g_lp[c:] == 0).all()) and bool(torch.signbit(g_lp[c:]).all()) and bool((g_ent[c:] == 0).all()) and not bool(torch.signbit(g_ent[c:]).any())
    return lens, total


@pytest.mark.parametrize("mode", ["sampled", "greedy"])
@pytest.mark.parametrize("S", [4, 9])
@pytest.mark.parametrize("kind", ["none", "merged", "lora"])
def test_session_equals_static_rows(setup, kind, S, mode):  # noqa: F811
    """3. N = 11 prompts through S slots, T = 24, a check every 4 steps; S = 4: the <= 8-row decode path, S = 9: the 9..64-row decode GEMMs"""
    s = setup
    N, T = 11, 24
    assert {1, 4, 24} <= set(CAPS11) and any((c - 1) % 4 for c in CAPS11) and set(CAPS11) <= {1, 3, 4, 5, 9, 24}
    toks, sched = _session(s, kind, N, S, T, CAPS11, mode)
    lens, total = _check_session(s, kind, N, S, T, CAPS11, mode, toks, sched)
    if S == 4:
        assert len({a for _, a in sched}) >= 3, "fewer than two admissions after the first: the case does not refill"
    print(f"{kind} S={S} {mode}: lengths {lens}, schedule {sched}, {total} steps")


def test_session_wide_with_idle_tail(setup):  # noqa: F811
    """3 (wide): S = 72 slots on the 65..256-row decode GEMMs, N = 80 prompts: the 8 that waited fill the 8 lowest freed slots, every other freed
    slot idles to the end.  Greedy: every prompt against its static row - a greedy row does not depend on the seed, so ONE static batch holds the
    72 prompts of the first wave at their slots and a second one the 8 late ones at theirs.  Sampled: the schedule for all, the static row (one
    batch per prompt, seed + i) for the first and last prompt of the first wave, one in between and the first and last late admission."""
    from opadpo_amd.generate import plan_continuous
    from test_return_sequences_gpu import generator_of
    s = setup
    N, S, T = 80, 72, 24
    caps = [(1, 3, 4, 5, 9, 24)[i % 6] for i in range(N)]
    queries, qmask, feats = _prompts(s, N)
    gen, _ = generator_of(s, "none")
    toks, sched = _session(s, "none", N, S, T, caps, "greedy")
    toks = toks.cpu()
    assert [tuple(x) for x in sched] == plan_continuous(_lengths(toks, caps, EOS), S, 4)[0]
    assert [x[0] for x in sched[:S]] == list(range(S)) and all(a > 0 for _, a in sched[S:]) and len({x[0] for x in sched[S:]}) == N - S
    for wave in (list(range(S)), list(range(S, N))):
        at = list(range(S))                          # row r of the static batch: the wave's prompt whose slot is r, any prompt elsewhere
        for i in wave:
            at[sched[i][0]] = i
        want = gen.generate(queries[at], qmask[at], image_feats=feats[at].contiguous(), max_new_tokens=T, seed=SEED, **GREEDY).cpu()
        for i in wave:
            c = caps[i]
            assert torch.equal(toks[i, :c], want[sched[i][0], :c]) and bool((toks[i, c:] == PAD).all()), (i, sched[i])
    toks, sched = _session(s, "none", N, S, T, caps, "sampled")
    toks = toks.cpu()
    assert [tuple(x) for x in sched] == plan_continuous(_lengths(toks, caps, EOS), S, 4)[0]
    for i in (0, 35, S - 1, S, N - 1):
        w_tok = _static_row(s, "none", N, i, sched[i][0], S, T, "sampled", EOS)[0]
        assert torch.equal(toks[i, :caps[i]], w_tok[:caps[i]]) and bool((toks[i, caps[i]:] == PAD).all()), (i, sched[i])


def test_eos_finishes_a_slot(setup):  # noqa: F811
    """4. e = the token prompt 0 emits at step 3 of a greedy static run; with eos_token_id = e prompt 0 retires at the first check after step 3"""
    s = setup
    N, S, T = 11, 4, 24
    e = int(_static_row(s, "none", N, 0, 0, S, T, "greedy", EOS)[0][3])
    assert e != PAD
    toks, sched = _session(s, "none", N, S, T, CAPS11, "greedy", eos=e)
    lens, _ = _check_session(s, "none", N, S, T, CAPS11, "greedy", toks, sched, eos=e)
    assert lens[0] <= 4 and e in toks[0, :4].tolist()
    assert len({a + n - 1 for (_, a), n in zip(sched, lens)}) >= 2, "precondition: at least two distinct finish steps"
    assert tuple(sched[0]) == (0, 0) and tuple(sched[4]) == (0, 4), "slot 0 is free at the first check after step 3: prompt 4 is admitted there"


def test_graph_replay_across_admissions(setup):  # noqa: F811
    """5. one captured step serves the whole session: the same bits as the eager session, across more than two admissions"""
    s = setup
    N, S, T = 11, 4, 24
    for mode in ("sampled", "greedy"):
        eager, sched_e = _session(s, "none", N, S, T, CAPS11, mode)
        graph, sched_g = _session(s, "none", N, S, T, CAPS11, mode, use_graph=True)
        assert torch.equal(eager, graph) and sched_e == sched_g
        assert len({a for _, a in sched_g}) >= 3
        _check_session(s, "none", N, S, T, CAPS11, mode, graph, sched_g)


@pytest.mark.parametrize("kind,S", [("none", 4), ("merged", 9)])
def test_session_logprobs(setup, kind, S):  # noqa: F811
    """6. logp / ent of prompt i are the static comparison's, bit for bit, and -0.0 / 0 beyond its cap; arming moves no token"""
    s = setup
    N, T = 11, 24
    plain, sched0 = _session(s, kind, N, S, T, CAPS11, "sampled")
    toks, lp, ent, sched = _session(s, kind, N, S, T, CAPS11, "sampled", output_logprobs=True)
    assert torch.equal(toks, plain) and sched == sched0
    assert lp.shape == ent.shape == (N, T) and lp.dtype == ent.dtype == torch.float32
    _check_session(s, kind, N, S, T, CAPS11, "sampled", toks, sched, lp=lp, ent=ent)
    real = toks != PAD
    assert bool((lp[real] < 0).all()) and bool((ent[real] > 0).all())


def test_idle_slots_leave_the_engine_as_it_was(setup):  # noqa: F811
    """7. two prompts in four slots, caps 2 and 24: two slots never admit anything, one idles for 22 steps.  The outputs are the static rows', and
    a static generation and a training forward / backward on the same engine give the bits they gave before the session."""
    s = setup
    from opadpo_amd.policy import AutoregressivePolicy
    from test_parity_gpu import make_inputs
    from test_return_sequences_gpu import Q, generator_of
    B, Tr = 3, 9
    images, queries, qmask, resp = make_inputs(s["d"], B, Q, Tr, seed=31)
    pol = AutoregressivePolicy(s["eng"], s["pol"], response_len=Tr, temperature=0.9)
    gen, _ = generator_of(s, "none")

    def before_after():
        s["pol"].grad.zero_()
        out = pol(images=images.to(s["dev"]), queries=queries, queries_attn_masks=qmask, standard_response=resp["standard_response"])
        lp = out["standard_response_logprobs"]
        lp.sum().backward()
        torch.cuda.synchronize()
        gen_out = gen.generate(queries, qmask, images.to(s["dev"]), max_new_tokens=8, seed=3, **SAMPLED)
        return lp.detach().clone(), s["pol"].grad.clone(), gen_out

    lp0, g0, t0 = before_after()
    N, S, T, caps = 2, 4, 24, [2, 24]
    toks, sched = _session(s, "none", N, S, T, caps, "sampled")
    assert [tuple(x) for x in sched] == [(0, 0), (1, 0)]
    _check_session(s, "none", N, S, T, caps, "sampled", toks, sched)
    toks_g, _ = _session(s, "none", N, S, T, caps, "sampled", use_graph=True)
    assert torch.equal(toks_g, toks)
    lp1, g1, t1 = before_after()
    assert torch.equal(lp0, lp1) and torch.equal(g0, g1) and torch.equal(t0, t1)
    s["pol"].grad.zero_()


def test_refusals_and_carry_over(setup):  # noqa: F811
    """8. every refusal carries text that names the bound, launches nothing that moves the next static generation, and disarms"""
    import ctypes as C
    s = setup
    from opadpo_amd import lib as L
    from opadpo_amd.generate import Generator
    from opadpo_amd.model import LlavaEngine
    from test_return_sequences_gpu import generator_of
    eng, dev = s["eng"], s["dev"]
    N, S, T = 3, 2, 6
    queries, qmask, feats = _prompts(s, N)
    gen, _ = generator_of(s, "none")
    static = lambda: gen.generate(queries, qmask, image_feats=feats, max_new_tokens=T, seed=9, **SAMPLED)
    base = static()
    cont = lambda **kw: gen.generate_continuous(queries, qmask, image_feats=feats, **{**dict(slots=S, max_new_tokens=T, seed=9, check_every=2, **SAMPLED), **kw})
    for slots in (0, 257):
        with pytest.raises(L.OpadpoError, match=r"slots must be in 1\.\.256"):
            cont(slots=slots)
        assert torch.equal(static(), base)
    for cap in (0, T + 1):
        with pytest.raises(ValueError, match=r"1\.\.max_new_tokens"):
            cont(max_new_tokens_per_prompt=[1, cap, 2])
        assert torch.equal(static(), base)
    with pytest.raises(NotImplementedError, match="num_return_sequences"):
        cont(num_return_sequences=2)
    with pytest.raises(NotImplementedError, match="num_beams"):
        cont(num_beams=2)
    with pytest.raises(NotImplementedError, match="logit_bias"):
        cont(logit_bias={5: 1.0})
    with pytest.raises(NotImplementedError, match="CtxEngine"):
        Generator(LlavaEngine(eng.base), None).generate_continuous(queries, qmask, image_feats=feats, slots=S, max_new_tokens=T)
    assert torch.equal(static(), base)
    # armed logit processors: the library refuses the session by name, and the refusal disarms
    eng._call("opadpo_ctx_set_logit_processors", (C.c_int32 * 1)(5), (C.c_float * 1)(50.0), 1, (C.c_int32 * 0)(), 0, None, 0)
    with pytest.raises(L.OpadpoError, match="opadpo_ctx_set_logit_processors"):
        cont()
    assert torch.equal(static(), base), "the generation after the refusal still carried the bias"
    # the library's own checks of an admission, on a live session: cap, slot range, repetition, a slot that is not finished
    ids = queries.to(dev).to(torch.int32).contiguous()
    tm = qmask.to(dev).to(torch.uint8).contiguous()
    eng._ensure_rope(ids.shape[1] + s["d"].n_patches - 1 + T)
    st = L.stream()
    eng._call("opadpo_decode_cont_begin", 0, S, ids.shape[1], T, 1.0, 30, 0.95, EOS, PAD, 0, st)
    try:
        def admit(slots_, caps_):
            k = len(slots_)
            eng._call("opadpo_decode_cont_admit", k, (C.c_int32 * k)(*slots_), L.ptr(ids), L.ptr(tm), L.ptr(feats), (C.c_uint64 * k)(*range(k)),
                      (C.c_int32 * k)(*caps_), st)
        for slots_, caps_, text in (([0], [0], r"cap must be in 1\.\.max_new_tokens"), ([0], [T + 1], r"cap must be in 1\.\.max_new_tokens"),
                                    ([S], [1], r"slot id outside 0\.\.slots-1"), ([-1], [1], r"slot id outside 0\.\.slots-1"),
                                    ([1, 1], [1, 1], "repeated")):
            with pytest.raises(L.OpadpoError, match=text):
                admit(slots_, caps_)
        admit([0], [T])
        with pytest.raises(L.OpadpoError, match="not finished"):
            admit([0], [T])
        tok = torch.empty(T, dtype=torch.int32, device=dev)
        with pytest.raises(L.OpadpoError, match="not finished"):
            eng._call("opadpo_decode_cont_retire", 0, L.ptr(tok), None, None, st)
        with pytest.raises(L.OpadpoError, match="not armed"):
            eng._call("opadpo_decode_cont_retire", 1, L.ptr(tok), L.ptr(tok), None, st)
        admit([1], [2])                              # the refusals above ended nothing: the session still admits and steps
        eng._call("opadpo_decode_run", 2, 0, st)
        fin = (C.c_uint8 * S)()
        eng._call("opadpo_decode_cont_poll", fin, st)
        assert fin[1] == 1, "the slot admitted with cap 2 has written its second token"
    finally:
        eng._call("opadpo_decode_end")
    assert torch.equal(static(), base)
    out = cont()
    assert out.shape == (N, T)


def test_rollout_cli_continuous_batching(tmp_path, monkeypatch):
    """9. --continuous_batching True: the same files, record count and record order as without the flag; --output_logprobs adds its three columns"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from opadpo_amd import cli_generate as cg
    from opadpo_amd import online_generate as og
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("WORLD_SIZE", "1")
    common = ["--synthetic", "tiny", "--synthetic_rows", "5", "--rollout_batch_size", "4", "--rollout_per_device_batch_size", "2", "--query_len", "64",
              "--response_len", "6", "--top_k", "10"]
    recs = {}
    for tag, extra in (("static", []), ("cont", ["--continuous_batching", "True"]), ("cont_lp", ["--continuous_batching", "True", "--output_logprobs", "True"])):
        ns, _ = cg.rollout_parser().parse_known_args(common + ["--output_dir", str(tmp_path / tag)] + extra)
        files = cg.run_rollout(ns, log=lambda *_: None)
        assert [os.path.basename(f) for f in files] == ["step0_rank0.json", "step1_rank0.json"]
        recs[tag] = [json.load(open(f)) for f in files]
    assert [len(r) for r in recs["static"]] == [len(r) for r in recs["cont"]] == [len(r) for r in recs["cont_lp"]] == [4, 1]
    same = ("query", "image_id", "standard_response", "image_bytes")
    for a, b, c in zip(recs["static"], recs["cont"], recs["cont_lp"]):
        for ra, rb, rc in zip(a, b, c):
            assert list(ra) == list(rb) and list(rc) == list(ra) + list(og.LOGPROB_COLUMNS)
            assert all(ra[k] == rb[k] == rc[k] for k in same), "record order changed"
            assert rb["original_generate_response"] == rc["original_generate_response"], "arming the log-probs moved a token"
            assert rc["original_generate_response_tokens"] >= 0 and rc["original_generate_response_logprob"] <= 0
