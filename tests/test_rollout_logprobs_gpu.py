"""GPU: per-token log-probs and entropies of the sampled tokens - opadpo_token_logprobs per element against tests/logprob_ref.py, and
opadpo_ctx_set_output_logprobs through CtxEngine.generate / Generator / AutoregressivePolicy.respond / the rollout CLI on the tiny model.

Op-level tolerance: per vocabulary size V, twice the largest |error against float64| of opadpo_head_fwd (the training head: same formula, labels =
tokens) over all finite cases of that V, log-prob and entropy separately, with a floor of 4 fp32 ulps at max(|z_tok|, |lse|) (two roundings in lse,
one each in z_tok and the subtraction).  Recorded on MI355X (profiles/rollout_logprobs_gpu_tests.txt)."""
import json
import math
import os

import numpy as np
import pytest
import torch

import logprob_ref
from test_eval_logit_gpu import env, _gen  # noqa: F401  (module fixture: tiny dims, adapter-free CtxEngine, 3 prompts)
from test_parity_gpu import setup  # noqa: F401  (module fixture of the parity suite: oracle weights, adapters, CtxEngine)

pytestmark = pytest.mark.gpu
EOS, PAD = 2, 0
SENTINEL = 777.0
TEMPS = (0, 0.7, 1, 2)
ROWS = (1, 5, 64, 65, 256)
VS = (128, 132, 512, 32000)
V_TAIL = 40000                      # past the 32768 columns a workgroup keeps in registers: the re-read tail of the sum pass
KINDS = 10


def _lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from opadpo_amd import lib as L
    L.load()
    return L


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
def _case(V, rows):
    """-> (logits fp32 [rows, V], tokens int32 [rows], kinds [rows]); row r is of kind (r + off) % 10, so 64 rows and more hold every kind, 5 rows hold
    kinds 5..9 and the single row is a quantile row.
      0 N(0, 3^2) quantile midpoints in a random order (test_eval_logit_gpu._tie_free_case), a random token     5 kind 0 shifted by +1e4
      1 one logit 60 above the rest, the token on it                                                             6 kind 0 with one -inf column (not the token)
      2 the same, the token off it                                                                               7 kind 0 with the pad token
      3 all logits equal                                                                                         8 kind 0, the token on the maximum
      4 two equal maxima, the token on the second                                                                9 kind 1 with one -inf column"""
    g = torch.Generator().manual_seed(7919 * V + rows)
    grid = (3.0 * 2.0 ** 0.5 * torch.erfinv(2.0 * (torch.arange(V, dtype=torch.float64) + 0.5) / V - 1.0)).to(torch.float32)
    off = 5 if rows == 5 else 0
    z = torch.empty(rows, V, dtype=torch.float32)
    tok = torch.empty(rows, dtype=torch.int32)
    kinds = []
    for r in range(rows):
        k = (r + off) % KINDS
        kinds.append(k)
        row = grid[torch.randperm(V, generator=g)] * (1.0 + 0.013 * (r % 17))
        t = 1 + int(torch.randint(0, V - 1, (1,), generator=g))               # never the pad id
        if k in (1, 2, 9):
            spike = 1 + int(torch.randint(0, V - 1, (1,), generator=g))
            row[spike] = float(row.max()) + 60.0
            t = spike if k != 2 else (spike + 1 if spike + 1 < V else spike - 1)
        elif k == 3:
            row[:] = 1.25
        elif k == 4:
            a, b = row.argsort(descending=True)[:2].tolist()
            row[b] = row[a]
            t = b if b != PAD else a
        elif k == 5:
            row = row + 1.0e4
        elif k == 7:
            t = PAD
        elif k == 8:
            t = int(row.argmax())
            if t == PAD:
                row[1] = float(row.max()) + 0.5
                t = 1
        if k in (6, 9):
            c = (t + 1 + int(torch.randint(0, V - 2, (1,), generator=g))) % V
            c = c if c != t else (t + 1) % V
            row[c] = -float("inf")
        z[r], tok[r] = row, t
    return z, tok, kinds


_CACHE = {}


def _cases(V):
    """every (rows, temperature) case of one V, built once: logits, tokens, kinds, the float64 restatement, z_tok and lse for the floor"""
    if V in _CACHE:
        return _CACHE[V]
    out = {}
    for rows in (ROWS if V != V_TAIL else (1, 5)):
        z, tok, kinds = _case(V, rows)
        per_t = {}
        for T in TEMPS:
            zs = logprob_ref.scaled(z.numpy(), T)
            logp, ent = logprob_ref.token_logprobs(zs, tok.numpy(), PAD)
            ztok = zs[np.arange(rows), tok.numpy().astype(np.int64)].astype(np.float64)
            lse = ztok - logp
            floor = 4.0 * np.spacing(np.maximum(np.abs(ztok), np.abs(lse)).astype(np.float32)).astype(np.float64)
            per_t[T] = (logp, ent, floor)
        out[rows] = (z, tok, np.array(kinds), per_t)
    _CACHE[V] = out
    return out


_YARD = {}


def _yardstick(V):
    """twice the largest |opadpo_head_fwd - float64| over the finite, non-pad rows of every case of V -> (bound_logp, bound_ent)"""
    if V in _YARD:
        return _YARD[V]
    L = _lib()
    dev = torch.device("cuda:0")
    worst = [0.0, 0.0]
    for rows, (z, tok, kinds, per_t) in _cases(V).items():
        finite = ~np.isin(kinds, (6, 9)) & (kinds != 7)
        if not finite.any():
            continue
        idx = torch.from_numpy(np.nonzero(finite)[0])
        zd, td = z[idx].contiguous().to(dev), tok[idx].contiguous().to(dev)
        n = int(idx.numel())
        for T in TEMPS:
            inv = 1.0 if T == 0 else float(np.float32(1.0) / np.float32(T))
            lp, en, ls = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(3))
            L.call("opadpo_head_fwd", L.ptr(zd), V, L.ptr(td), inv, L.ptr(lp), L.ptr(en), L.ptr(ls), n, V, L.stream())
            torch.cuda.synchronize()
            want_lp, want_en, _ = per_t[T]
            worst[0] = max(worst[0], float(np.abs(lp.cpu().numpy().astype(np.float64) - want_lp[finite]).max()))
            worst[1] = max(worst[1], float(np.abs(en.cpu().numpy().astype(np.float64) - want_en[finite]).max()))
    _YARD[V] = (2.0 * worst[0], 2.0 * worst[1])
    print(f"V={V}: yardstick opadpo_head_fwd max |err vs fp64| logp {worst[0]:.3e} ent {worst[1]:.3e} -> bounds {2 * worst[0]:.3e} / {2 * worst[1]:.3e}")
    return _YARD[V]


def _token_logprobs(L, logits, ldl, rows, V, tokens, T, with_ent=True):
    dev = logits.device
    lp = torch.full((rows,), SENTINEL, dtype=torch.float32, device=dev)
    en = torch.full((rows,), SENTINEL, dtype=torch.float32, device=dev)
    L.call("opadpo_token_logprobs", L.ptr(logits), ldl, rows, V, L.ptr(tokens), float(T), PAD, L.ptr(lp), L.ptr(en) if with_ent else None, L.stream())
    torch.cuda.synchronize()
    return lp.cpu(), en.cpu()


# ---- op level -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,rows", [(V, r) for V in VS for r in ROWS] + [(V_TAIL, 1), (V_TAIL, 5)])
def test_token_logprobs_against_ref(V, rows):
    L = _lib()
    dev = torch.device("cuda:0")
    b_lp, b_en = _yardstick(V)
    z, tok, kinds, per_t = _cases(V)[rows]
    td = tok.to(dev)
    pad = kinds == 7
    worst = [0.0, 0.0]
    for ldl in (V, V + 128):
        buf = torch.full((rows, ldl), float("nan"), dtype=torch.float32)          # the slack behind a row is poison
        buf[:, :V] = z
        zd = buf.to(dev)
        for T in TEMPS:
            want_lp, want_en, floor = per_t[T]
            lp, en = _token_logprobs(L, zd, ldl, rows, V, td, T)
            lp64, en64 = lp.numpy().astype(np.float64), en.numpy().astype(np.float64)
            assert not bool((lp == SENTINEL).any()) and not bool((en == SENTINEL).any()), "an element was not written"
            assert np.isfinite(lp64).all() and np.isfinite(en64).all(), (V, rows, ldl, T)
            assert (lp64[pad] == 0).all() and np.signbit(lp64[pad]).all() and (en64[pad] == 0).all() and not np.signbit(en64[pad]).any()
            e_lp, e_en = np.abs(lp64 - want_lp), np.abs(en64 - want_en)
            worst = [max(worst[0], float(e_lp.max())), max(worst[1], float(e_en.max()))]
            assert (e_lp <= np.maximum(b_lp, floor)).all(), (V, rows, ldl, T, int(e_lp.argmax()), int(kinds[e_lp.argmax()]), float(e_lp.max()), b_lp)
            assert (e_en <= np.maximum(b_en, floor)).all(), (V, rows, ldl, T, int(e_en.argmax()), int(kinds[e_en.argmax()]), float(e_en.max()), b_en)
            eq = kinds == 3                                                         # all logits equal: ent = ln V, logp = -ln V
            if eq.any():
                lnv = math.log(V)
                assert (np.abs(lp64[eq] + lnv) <= np.maximum(b_lp, floor[eq])).all() and (np.abs(en64[eq] - lnv) <= np.maximum(b_en, floor[eq])).all()
            if ldl == V and T == 0.7:                                              # ent == NULL: the same log-probs, the entropy buffer untouched
                lp2, en2 = _token_logprobs(L, zd, ldl, rows, V, td, T, with_ent=False)
                assert torch.equal(lp2.view(torch.int32), lp.view(torch.int32)) and bool((en2 == SENTINEL).all())
    print(f"V={V} rows={rows}: opadpo_token_logprobs max |err vs fp64| logp {worst[0]:.3e} ent {worst[1]:.3e} (bounds {b_lp:.3e} / {b_en:.3e})")


def test_token_logprobs_argument_checks():
    L = _lib()
    dev = torch.device("cuda:0")
    V, rows = 512, 4
    logits = torch.randn(rows + 1, V + 4, device=dev)
    tok = torch.tensor([1, 2, 3, 4], dtype=torch.int32, device=dev)
    lp = torch.full((rows,), SENTINEL, device=dev)
    en = torch.full((rows,), SENTINEL, device=dev)

    def call(logits_p=None, ldl=V + 4, rows_=rows, V_=V, tok_p=None, T=1.0, lp_p=None):
        L.call("opadpo_token_logprobs", L.ptr(logits) if logits_p is None else logits_p, ldl, rows_, V_, L.ptr(tok) if tok_p is None else tok_p, T, PAD,
               L.ptr(lp) if lp_p is None else lp_p, L.ptr(en), L.stream())

    for bad in (lambda: call(V_=V - 2), lambda: call(ldl=V + 2), lambda: call(ldl=V - 4), lambda: call(T=-1.0), lambda: call(T=float("nan")),
                lambda: call(rows_=0), lambda: call(logits_p=0), lambda: call(tok_p=0), lambda: call(lp_p=0), lambda: call(logits_p=logits.data_ptr() + 4)):
        with pytest.raises(L.OpadpoError, match="opadpo_token_logprobs"):
            bad()
    torch.cuda.synchronize()
    assert bool((lp == SENTINEL).all()) and bool((en == SENTINEL).all()), "a refused call launched something"
    call()
    torch.cuda.synchronize()
    assert not bool((lp == SENTINEL).any()) and not bool((en == SENTINEL).any())


# ---- context, tiny model ------------------------------------------------------------------------------------------------------------------
GREEDY = dict(temperature=1.0, top_k=1, top_p=1.0, seed=1)
SAMPLED = dict(temperature=0.8, top_k=20, top_p=0.9, seed=5)


def _neg_zero(t):
    return bool((t == 0).all()) and bool(torch.signbit(t).all())


def test_off_is_identical_small(env):  # noqa: F811
    """B = 3, 10 new tokens: arming moves no token; eager, graph replay and a second eager call give the same bits; the next call is unarmed."""
    for cfg in (GREEDY, SAMPLED, dict(SAMPLED, suppress_eos=True)):
        base = _gen(env, n_new=10, **cfg)
        runs = [_gen(env, n_new=10, use_graph=g, output_logprobs=True, **cfg) for g in (False, True, False)]
        for toks, lp, en in runs:
            assert torch.equal(toks, base) and lp.shape == en.shape == (3, 10) and lp.dtype == en.dtype == torch.float32
            assert torch.equal(lp.view(torch.int32), runs[0][1].view(torch.int32)) and torch.equal(en.view(torch.int32), runs[0][2].view(torch.int32))
        toks, lp, en = (t.cpu() for t in runs[0])
        assert bool(torch.isfinite(lp).all()) and bool(torch.isfinite(en).all())
        pad = toks == PAD
        assert bool((lp[~pad] < 0).all()) and bool((en[~pad] > 0).all())
        assert (not pad.any()) or (_neg_zero(lp[pad]) and bool((en[pad] == 0).all()))
        after = _gen(env, n_new=10, **cfg)
        assert torch.is_tensor(after) and torch.equal(after, base)
        toks4 = _gen(env, n_new=10, score_ids=[5, 7], output_logprobs=True, **cfg)          # with the score read-out: (tokens, scores, logp, ent)
        assert len(toks4) == 4 and torch.equal(toks4[0], base) and toks4[1].shape == (3, 2) and torch.equal(toks4[2], runs[0][1])


@pytest.mark.parametrize("kind", ["none", "merged"])
def test_off_is_identical_wide(setup, kind):  # noqa: F811
    """B = 9, n = 8: 72 rows on the wide decode GEMMs and opadpo_decode_begin_n, 6 new tokens."""
    from test_return_sequences_gpu import generator_of, prompts
    s = setup
    images, queries, qmask = prompts(s["d"], 9, seed=409)
    for cfg in (dict(temperature=1.0, top_k=1, top_p=1.0, seed=1), dict(temperature=0.8, top_k=30, top_p=0.95, seed=11),
                dict(temperature=0.8, top_k=30, top_p=0.95, seed=11, suppress_eos=True)):
        outs = {}
        for use_graph in (False, True):
            gen, _ = generator_of(s, kind, use_graph)
            feats = gen.engine.encode_images(images.to(s["dev"]))
            outs[use_graph] = gen.generate(queries, qmask, image_feats=feats, num_return_sequences=8, max_new_tokens=6, output_logprobs=True, **cfg)
            base = gen.generate(queries, qmask, image_feats=feats, num_return_sequences=8, max_new_tokens=6, **cfg)
            assert torch.is_tensor(base) and torch.equal(outs[use_graph][0], base)
        (t0, l0, e0), (t1, l1, e1) = outs[False], outs[True]
        assert t0.shape == l0.shape == e0.shape == (72, 6)
        assert torch.equal(t0, t1) and torch.equal(l0.view(torch.int32), l1.view(torch.int32)) and torch.equal(e0.view(torch.int32), e1.view(torch.int32))
        pad = t0 == PAD
        assert bool(torch.isfinite(l0).all()) and bool((l0[~pad] < 0).all()) and bool((e0[~pad] > 0).all())


def _step0(env, bias, suppress_eos):  # noqa: F811
    """[B, V] logits the sampler reads at step 0 (bias added, EOS column -inf under suppress_eos), through the greedy score read-out"""
    V = env["d"].vocab
    cols = []
    for c0 in range(0, V, 64):
        _, sc = _gen(env, n_new=1, temperature=0, top_k=0, top_p=1.0, seed=0, logit_bias=bias, suppress_eos=suppress_eos,
                     score_ids=list(range(c0, min(V, c0 + 64))))
        cols.append(sc.cpu())
    return torch.cat(cols, 1)


@pytest.mark.parametrize("suppress_eos", [False, True])
@pytest.mark.parametrize("bias", [None, {3: 1.5, 77: -0.75, 511: 0.125}], ids=["plain", "bias"])
def test_step0_definition(env, bias, suppress_eos):  # noqa: F811
    V = env["d"].vocab
    b_lp, b_en = _yardstick(V)
    z0 = _step0(env, bias, suppress_eos).numpy()
    assert bool(np.isneginf(z0[:, EOS]).all()) == suppress_eos
    for cfg in (dict(temperature=1.0, top_k=0, top_p=1.0, seed=3), dict(temperature=0.8, top_k=20, top_p=0.9, seed=5), GREEDY):
        toks, lp, en = _gen(env, n_new=4, logit_bias=bias, suppress_eos=suppress_eos, output_logprobs=True, **cfg)
        t0 = toks[:, 0].cpu().numpy()
        zs = logprob_ref.scaled(z0, cfg["temperature"])
        want_lp, want_en = logprob_ref.token_logprobs(zs, t0, PAD)
        ztok = zs[np.arange(len(t0)), t0].astype(np.float64)
        floor = 4.0 * np.spacing(np.maximum(np.abs(ztok), np.abs(ztok - want_lp)).astype(np.float32)).astype(np.float64)
        e_lp = np.abs(lp[:, 0].cpu().numpy().astype(np.float64) - want_lp)
        e_en = np.abs(en[:, 0].cpu().numpy().astype(np.float64) - want_en)
        print(f"step 0, bias={bias is not None} suppress_eos={suppress_eos} T={cfg['temperature']} top_k={cfg['top_k']}: max |err| logp {e_lp.max():.3e} ent {e_en.max():.3e}")
        assert (e_lp <= np.maximum(b_lp, floor)).all() and (e_en <= np.maximum(b_en, floor)).all(), (e_lp, e_en, b_lp, b_en)


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "T0.8"])
@pytest.mark.parametrize("kind", ["none", "merged", "lora"])
def test_against_the_fp32_oracle_teacher_forced(setup, kind, sampled):  # noqa: F811
    """B = 8, 16 new tokens, suppress_eos: the decode loop's values against the fp32 oracle on the generated tokens (float64 log-softmax of its logits,
    the EOS column -inf as the sampler saw it), with the engine's own no-grad training forward on the same tokens as the yardstick (against the oracle
    without the suppression, its own definition): mean |decode - oracle| <= 2 * mean |training - oracle|.  Both are bf16 pipelines with the same
    rounding points and differ in summation order; 128 tokens keep two draws of that noise within a factor 2, while a wrong position, token or
    temperature moves the mean by more than 0.1."""
    from opadpo_amd.model import SeqBatch
    from test_return_sequences_gpu import generator_of, prompts, Q
    s = setup
    LR, d, dev = s["LR"], s["d"], s["dev"]
    B, N = 8, 16
    T = 0.8 if sampled else 1.0
    cfg = dict(temperature=0.8, top_k=30, top_p=0.95, seed=17) if sampled else dict(temperature=1.0, top_k=1, top_p=1.0, seed=1)
    images, queries, qmask = prompts(d, B, seed=500)
    gen, lora = generator_of(s, kind)
    feats = gen.engine.encode_images(images.to(dev))
    toks, lp, en = gen.generate(queries, qmask, image_feats=feats, max_new_tokens=N, suppress_eos=True, output_logprobs=True, **cfg)
    toks, lp, en = toks.cpu(), lp.cpu().double().numpy(), en.cpu().double().numpy()
    assert not bool((toks == EOS).any())
    # the oracle, teacher-forced
    ids = torch.cat([queries, toks], 1)
    mask = torch.cat([qmask, torch.ones(B, N, dtype=torch.bool)], 1)
    with torch.no_grad():
        logits = LR.llava_logits(ids, mask, None, s["W"], lora, s["od"], feats=LR.image_features(images, s["W"], lora, s["od"])).float()
    q = Q + d.n_patches - 1
    z = logits[:, q - 1:q - 1 + N].reshape(B * N, d.vocab).numpy()
    flat = toks.reshape(-1).numpy()
    zsup = z.copy()
    zsup[:, EOS] = -np.inf
    o_lp, o_en = (a.reshape(B, N) for a in logprob_ref.token_logprobs(logprob_ref.scaled(zsup, T), flat, PAD))
    p_lp, p_en = (a.reshape(B, N) for a in logprob_ref.token_logprobs(logprob_ref.scaled(z, T), flat, PAD))
    # the yardstick: the no-grad training forward of the same engine and adapter on the same tokens
    adapter = {"none": None, "merged": s["ref_merged"], "lora": s["ref"]}[kind]
    batch = SeqBatch(ids.to(dev).to(torch.int32).contiguous(), mask.to(dev).to(torch.uint8).contiguous(), torch.arange(B, device=dev, dtype=torch.int32), None, N)
    with torch.no_grad():
        t_lp, t_en, _ = s["eng"].seq_logprobs_fwd(adapter, batch, feats.contiguous(), T, train=False)
    torch.cuda.synchronize()
    t_lp, t_en = t_lp.cpu().double().numpy(), t_en.cpu().double().numpy()
    d_lp, d_en, y_lp, y_en = np.abs(lp - o_lp), np.abs(en - o_en), np.abs(t_lp - p_lp), np.abs(t_en - p_en)
    print(f"oracle {kind} {'T=0.8' if sampled else 'greedy'}: decode mean/max |err| logp {d_lp.mean():.3e}/{d_lp.max():.3e} ent {d_en.mean():.3e}/{d_en.max():.3e}; "
          f"training forward logp {y_lp.mean():.3e}/{y_lp.max():.3e} ent {y_en.mean():.3e}/{y_en.max():.3e}")
    assert float(np.abs(o_lp).mean()) > 0.5 and float(y_lp.mean()) > 0
    assert d_lp.mean() <= 2 * y_lp.mean(), (d_lp.mean(), y_lp.mean())
    assert d_en.mean() <= 2 * y_en.mean(), (d_en.mean(), y_en.mean())


def test_conventions_eos_and_pad(env):  # noqa: F811
    """A bias steers every row to EOS at step 0 with margin m over the logit range: |logp[:, 0]| <= V * exp(-m) (every other token is at least m
    below), EOS carries its own values, every later position is pad with -0.0 / 0."""
    V = env["d"].vocab
    z0 = _step0(env, None, False)
    m = 30.0
    big = float(z0.max() - z0.min()) + m
    for use_graph in (False, True):
        toks, lp, en = _gen(env, n_new=8, use_graph=use_graph, logit_bias={EOS: big}, output_logprobs=True, **GREEDY)
        toks, lp, en = toks.cpu(), lp.cpu(), en.cpu()
        assert bool((toks[:, 0] == EOS).all()) and bool((toks[:, 1:] == PAD).all())
        assert bool((lp[:, 0].abs() <= V * math.exp(-m)).all()) and bool((lp[:, 0] <= 0).all()), lp[:, 0]
        assert bool((en[:, 0] >= 0).all()) and bool((en[:, 0] <= V * math.exp(-m) * (m + 2 * big)).all()), en[:, 0]
        assert _neg_zero(lp[:, 1:]) and bool((en[:, 1:] == 0).all()) and not bool(torch.signbit(en[:, 1:]).any())
    print(f"EOS at step 0 with margin {m}: max |logp[:, 0]| = {float(lp[:, 0].abs().max()):.3e} <= V exp(-m) = {V * math.exp(-m):.3e}")


def test_refusals(env, setup):  # noqa: F811
    import ctypes as C  # noqa: F401
    from opadpo_amd.generate import Generator
    from opadpo_amd.model import LlavaEngine
    L, eng, dev, p = env["L"], env["eng"], env["dev"], env["p"]
    base = _gen(env, **GREEDY)
    lp = torch.full((6, 3), SENTINEL, device=dev)
    en = torch.full((6, 3), SENTINEL, device=dev)
    with pytest.raises(L.OpadpoError, match="opadpo_ctx_set_output_logprobs"):
        eng._call("opadpo_ctx_set_output_logprobs", None, L.ptr(en))
    assert torch.equal(_gen(env, **GREEDY), base)
    # beam search on an armed context: refused, and the refusal disarms
    eng._call("opadpo_ctx_set_output_logprobs", L.ptr(lp), L.ptr(en))
    with pytest.raises(L.OpadpoError, match="beam search"):
        eng.generate_beams(None, p["queries"], p["queries_attn_masks"], env["feats"], num_beams=2, max_new_tokens=4, eos_token_id=EOS, pad_token_id=PAD,
                           use_graph=False)
    out = _gen(env, **GREEDY)
    torch.cuda.synchronize()
    assert torch.is_tensor(out) and torch.equal(out, base)
    assert bool((lp == SENTINEL).all()) and bool((en == SENTINEL).all()), "the generation after the refusal was still armed"
    toks, _ = eng.generate_beams(None, p["queries"], p["queries_attn_masks"], env["feats"], num_beams=2, max_new_tokens=4, eos_token_id=EOS,
                                 pad_token_id=PAD, use_graph=False)
    assert toks.shape == (3, 4)
    # armed, then cleared by a (null, null) call
    eng._call("opadpo_ctx_set_output_logprobs", L.ptr(lp), L.ptr(en))
    eng._call("opadpo_ctx_set_output_logprobs", None, None)
    assert torch.equal(_gen(env, **GREEDY), base) and bool((lp == SENTINEL).all())
    # ent is nullable
    eng._call("opadpo_ctx_set_output_logprobs", L.ptr(lp), None)
    assert torch.equal(_gen(env, **GREEDY), base)
    torch.cuda.synchronize()
    assert not bool((lp == SENTINEL).any()) and bool((en == SENTINEL).all())
    # the Python surface
    s = setup
    gen = Generator(s["eng"], None, use_graph=False)
    from test_return_sequences_gpu import prompts
    images, queries, qmask = prompts(s["d"], 2, seed=3)
    feats = gen.engine.encode_images(images.to(s["dev"]))
    with pytest.raises(NotImplementedError, match="beam"):
        gen.generate(queries, qmask, image_feats=feats, max_new_tokens=4, num_beams=2, output_logprobs=True)
    with pytest.raises(NotImplementedError, match="CtxEngine"):
        Generator(LlavaEngine(s["eng"].base), None).generate(queries, qmask, image_feats=feats, max_new_tokens=4, output_logprobs=True)


def test_policy_respond_logprobs(setup):  # noqa: F811
    """respond(output_logprobs=True, num_return_sequences=3): keys and shapes, the tokens of the call without the keyword, values equal to the policy's
    own no-grad forward on those tokens up to the two engines' distance, and the next training forward and backward as before the call."""
    s = setup
    from opadpo_amd.policy import AutoregressivePolicy
    from test_parity_gpu import make_inputs
    from test_return_sequences_gpu import Q
    B, T, n = 3, 9, 3
    images, queries, qmask, resp = make_inputs(s["d"], B, Q, T, seed=31)
    pol = AutoregressivePolicy(s["eng"], s["pol"], response_len=T, temperature=0.9)
    one = {"standard_response": resp["standard_response"]}

    def train_pass():
        s["pol"].grad.zero_()
        out = pol(images=images.to(s["dev"]), queries=queries, queries_attn_masks=qmask, **one)
        lp = out["standard_response_logprobs"]
        lp.sum().backward()
        torch.cuda.synchronize()
        return lp.detach().clone(), s["pol"].grad.clone()

    lp0, g0 = train_pass()
    plain = pol.respond(queries, qmask, images.to(s["dev"]), num_return_sequences=n, seed=7)
    got = pol.respond(queries, qmask, images.to(s["dev"]), num_return_sequences=n, seed=7, output_logprobs=True)
    assert list(plain) == ["responses"] and list(got) == ["responses", "responses_logprobs", "responses_entropies"]
    assert torch.equal(got["responses"], plain["responses"])
    lp, en = got["responses_logprobs"], got["responses_entropies"]
    assert lp.shape == en.shape == (B * n, T) and lp.dtype == en.dtype == torch.float32
    pad = got["responses"] == PAD
    assert bool((lp[pad] == 0).all()) and bool((en[pad] == 0).all()) and bool((lp[~pad] < 0).all()) and bool((en[~pad] > 0).all())
    # the policy's own forward on its samples (the second full forward this feature saves): the same numbers up to the two engines' bf16 noise, for
    # which the suite's generation tests allow 5e-2 on a logit; a wrong position, token or temperature moves a log-prob by more than 0.1.  Rows
    # with a sampled pad id inside the response are left out (the trainer's row plan ends a response at its first pad)
    toks = got["responses"].cpu()
    with torch.no_grad():
        out = pol(images=images.to(s["dev"]).repeat_interleave(n, 0), queries=queries.repeat_interleave(n, 0),
                  queries_attn_masks=qmask.repeat_interleave(n, 0), sampled_response=toks)
    rows_ok = torch.tensor([(r[:int(r.count_nonzero())] != PAD).all().item() for r in toks])
    diff = (out["sampled_response_logprobs"].cpu() - lp.cpu()).abs()[rows_ok]
    print(f"respond: decode-loop log-probs vs the policy's forward on the same tokens ({int(rows_ok.sum())} rows): mean |diff| = {float(diff.mean()):.3e}, "
          f"max = {float(diff.max()):.3e}")
    assert int(rows_ok.sum()) >= B * n // 2 and float(diff.mean()) < 5e-2
    lp1, g1 = train_pass()
    assert torch.equal(lp0, lp1) and torch.equal(g0, g1)
    s["pol"].grad.zero_()


def test_rollout_cli_output_logprobs(tmp_path, monkeypatch):
    """--synthetic tiny rollout: with --output_logprobs True the three columns are present, finite and those a Python-side pass over
    Generator.rollout(output_logprobs=True) gives; without it the files are byte for byte the flagged run's with the three columns removed."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from opadpo_amd import cli_generate as cg
    from opadpo_amd import online_generate as og
    from opadpo_amd.generate import Generator
    from opadpo_amd.rollout_data import QueryResponseDataset, collate_query_response
    from opadpo_amd.synth import synth_question_rows
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("WORLD_SIZE", "1")
    common = ["--synthetic", "tiny", "--synthetic_rows", "5", "--rollout_batch_size", "4", "--rollout_per_device_batch_size", "2", "--query_len", "64",
              "--response_len", "6", "--top_k", "10", "--num_return_sequences", "2"]
    files = {}
    for tag, extra in (("off", []), ("on", ["--output_logprobs", "True"])):
        ns, _ = cg.rollout_parser().parse_known_args(common + ["--output_dir", str(tmp_path / tag)] + extra)
        files[tag] = cg.run_rollout(ns, log=lambda *_: None)
    assert [os.path.basename(f) for f in files["on"]] == [os.path.basename(f) for f in files["off"]] == ["step0_rank0.json", "step1_rank0.json"]
    recs = []
    for f_on, f_off in zip(files["on"], files["off"]):
        rows = json.load(open(f_on))
        recs += rows
        assert all(list(r)[-3:] == list(og.LOGPROB_COLUMNS) for r in rows)
        stripped = json.dumps([{k: v for k, v in r.items() if k not in og.LOGPROB_COLUMNS} for r in rows], indent=4)
        assert stripped == open(f_off).read(), "the unflagged run's JSON is not the flagged run's without the three columns"
        assert not any(c in open(f_off).read() for c in og.LOGPROB_COLUMNS)
    assert len(recs) == 10
    # Python-side recomputation: the same engine, data and seeds as run_rollout builds them
    engine, adapter, tok = cg._engine(ns.base_model_name, "tiny", None, ns.lora_rank, ns.lora_alpha, ns.seed)
    ds = QueryResponseDataset(synth_question_rows(5, seed=ns.seed), tok, 64, image_size=engine.d.image_size, log=lambda *_: None)
    gen = Generator(engine, adapter, merge_adapter=True, fuse_swiglu=True)
    want, call = [], 0
    for idx in ([0, 1, 2, 3], [4]):                           # rollout_batch_size 4 per step, per-device batches of 2, a new seed per batch
        for b0 in range(0, len(idx), 2):
            b = collate_query_response([ds[j] for j in idx[b0:b0 + 2]])
            call += 1
            toks, lp, en = gen.rollout(b["queries"].to(engine.dev), b["query_attn_masks"].to(engine.dev), b["images"].to(engine.dev), response_len=6,
                                       temperature=ns.temperature, top_k=10, top_p=ns.top_p, seed=ns.seed + call, additional_stop_ids=og.QUESTION_MARK_IDS,
                                       num_return_sequences=2, output_logprobs=True)
            for r in range(toks.shape[0]):
                keep = (toks[r] != tok.pad_token_id).cpu()
                cnt = int(keep.sum())
                want.append((float(lp[r].cpu().double()[keep].sum()), cnt, float(en[r].cpu().double()[keep].sum()) / cnt if cnt else 0.0))
    engine.close()
    for r, (w_lp, w_n, w_en) in zip(recs, want):
        g_lp, g_n, g_en = (r[c] for c in og.LOGPROB_COLUMNS)
        assert g_n == w_n and math.isfinite(g_lp) and math.isfinite(g_en)
        assert g_lp == pytest.approx(w_lp, abs=1e-9) and g_en == pytest.approx(w_en, abs=1e-9)
        assert (g_n == 0 and g_lp == 0 and g_en == 0) or (g_lp < 0 and g_en > 0)
