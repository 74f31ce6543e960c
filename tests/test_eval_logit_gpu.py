"""GPU: the yes/no evaluation generator's device side - opadpo_logit_bias_add, opadpo_gather_scores, opadpo_ctx_set_logit_processors through
CtxEngine.generate(logit_bias=, score_ids=), and cli_generate.main_eval_logit - on the tiny synthetic model, against tests/logit_ref.py and the
engine's own no-grad forward.

End-to-end gap recorded on MI355X (profiles/eval_logit_gpu_tests.txt): the decode head and the training head run different GEMM kernels (the
weight-streaming one for <= 64 rows against the tiled one), 7.153e-07 apart on the same normalised rows; the step-0 scores of the context differ from
logits[:, ids] of the op-level forward by exactly that, 7.153e-07 (with a bias: 7.153e-07), against the bound of twice the heads' distance."""
import json

import numpy as np
import pytest
import torch

import logit_ref

pytestmark = pytest.mark.gpu
EOS, PAD = 2, 0
GREEDY = dict(temperature=1.0, top_k=1, top_p=1.0, seed=1)          # how the tree spells greedy decoding today
SAMPLED = dict(temperature=0.8, top_k=20, top_p=0.9, seed=5)


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from opadpo_amd import lib
    from opadpo_amd.ctx import CtxEngine
    from opadpo_amd.dims import LlavaDims
    from opadpo_amd.model import BaseWeights
    from opadpo_amd.synth import init_weights, synth_pairs
    lib.load()
    dev = torch.device("cuda:0")
    d = LlavaDims.tiny()
    base = BaseWeights(d, init_weights(d, seed=0, std=0.05, device=dev), dev, need_backward=False)
    eng = CtxEngine(base)
    p = synth_pairs(d, 3, 16, 8, seed=5, device=dev)
    feats = eng.encode_images(p["images"])
    yield dict(d=d, dev=dev, base=base, eng=eng, p=p, feats=feats, L=lib)
    eng.close()


def _gen(env, n_new=6, use_graph=False, suppress_eos=False, **kw):
    p = env["p"]
    out = env["eng"].generate(None, p["queries"], p["queries_attn_masks"], env["feats"], max_new_tokens=n_new, eos_token_id=EOS, pad_token_id=PAD,
                              suppress_eos=suppress_eos, use_graph=use_graph, **kw)
    torch.cuda.synchronize()
    return out


def _step0_logits(env, bias=None):
    """[B, V] first-token logits (+ bias) of the context's decode head, read 64 ids at a time through the greedy score read-out"""
    V = env["d"].vocab
    cols = []
    for c0 in range(0, V, 64):
        _, sc = _gen(env, n_new=1, temperature=0, top_k=0, top_p=1.0, seed=0, logit_bias=bias, score_ids=list(range(c0, min(V, c0 + 64))))
        cols.append(sc.cpu())
    return torch.cat(cols, 1)


# ---- bias steers ----------------------------------------------------------------------------------------------------------------------
def test_bias_steers_generation(env):
    z = _step0_logits(env)
    B, V = z.shape
    assert B == 3 and V == env["d"].vocab and bool(torch.isfinite(z).all())
    big = float(z.max() - z.min()) + 1.0                       # larger than any gap between two step-0 logits of the tiny model
    base = _gen(env, **GREEDY).cpu()
    assert torch.equal(base[:, 0], z.argmax(-1)), "greedy token 0 is not the argmax of the step-0 scores"
    order = z[0].argsort()
    t = next(int(i) for i in order[V // 2:] if int(i) not in (EOS, PAD) and int(i) not in base[:, 0].tolist())      # a middling token nobody picks
    print(f"step-0 logit range {float(z.min()):.4f} .. {float(z.max()):.4f}, big = {big:.4f}, steered token {t}")
    for use_graph in (False, True):
        out = _gen(env, n_new=8, use_graph=use_graph, logit_bias={t: big}, **GREEDY).cpu()
        assert bool((out == t).all()), (t, out)               # t is not EOS: no row ever finishes, every step emits t
    # pushing every row's unbiased first token down changes that token
    firsts = sorted(set(base[:, 0].tolist()))
    out = _gen(env, logit_bias={f: -big for f in firsts}, **GREEDY).cpu()
    assert bool((out[:, 0] != base[:, 0]).all()), (out[:, 0], base[:, 0])
    zb = z.clone()
    zb[:, firsts] -= big
    assert torch.equal(out[:, 0], zb.argmax(-1))
    # EOS handling: steering to EOS finishes every row at once, pad follows
    out = _gen(env, logit_bias={EOS: big}, **GREEDY).cpu()
    assert bool((out[:, 0] == EOS).all()) and bool((out[:, 1:] == PAD).all())


# ---- nothing moves when off -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [False, True])
def test_off_is_token_identical(env, use_graph):
    for cfg in (GREEDY, SAMPLED, dict(SAMPLED, suppress_eos=True)):
        base = _gen(env, n_new=10, use_graph=use_graph, **cfg)
        assert torch.is_tensor(base) and base.shape == (3, 10)
        t = int(base[0, 0])
        for kw in (dict(logit_bias=None, score_ids=None), dict(logit_bias={}), dict(logit_bias={t: 0.0}), dict(logit_bias={t: 0.0, 7: 0.0, 9: 0.0})):
            out = _gen(env, n_new=10, use_graph=use_graph, **cfg, **kw)
            assert torch.is_tensor(out) and torch.equal(out, base), (cfg, kw)
        toks, sc = _gen(env, n_new=10, use_graph=use_graph, score_ids=[t, 5], **cfg)          # reading scores does not move a token either
        assert torch.equal(toks, base) and sc.shape == (3, 2) and sc.dtype == torch.float32
        toks, sc = _gen(env, n_new=10, use_graph=use_graph, score_ids=[], **cfg)
        assert torch.equal(toks, base) and sc.shape == (3, 0)


# ---- the two kernels against the restatement ------------------------------------------------------------------------------------------------
# top-p decisions closer than this to a tie are redrawn.  The kernel adds fp32 expf values (within 2 ulp = 2.4e-7 relative of the restatement's
# float64 exponentials) in fp64, so a cumulative mass fraction differs from the restatement's by at most 2.4e-7: four times that
MARGIN = 1e-6


def _tie_free_case(B, V, seed, cfg):
    """random logits [B, V], a bias table and six score ids (one twice) such that no two values of a row are equal and no top-p decision is a tie"""
    for attempt in range(20):
        g = torch.Generator().manual_seed(1000 * seed + attempt)
        # V draws of randn collide in fp32 at V = 32000: the values are the V quantile midpoints of N(0, 3^2) instead, in a random order per
        # row and stretched a little from row to row - distinct by construction (asserted below)
        grid = 3.0 * 2.0 ** 0.5 * torch.erfinv(2.0 * (torch.arange(V, dtype=torch.float64) + 0.5) / V - 1.0)
        z = torch.stack([grid[torch.randperm(V, generator=g)] * (1.0 + 0.013 * r + 0.001 * attempt) for r in range(B)]).to(torch.float32).numpy()
        rank = np.argsort(-z[0]).tolist()
        bias = {rank[1]: 2.5, rank[9]: -1.25, rank[V // 2]: 4.0}                    # the last one lifts a middling token towards the top
        ids = [rank[0], rank[1], rank[3], rank[7], rank[V // 2], rank[1]]
        if all(len(np.unique(r)) == V for r in logit_ref._biased(z, bias)) and logit_ref.top_p_margin(z, bias, *cfg) > MARGIN:
            return z, bias, ids
    raise AssertionError("no tie-free logits drawn")


@pytest.mark.parametrize("cfg", [(0.0, 0, 1.0), (0.2, 0, 0.9), (1.0, 5, 1.0), (0.7, 50, 0.6), (2.0, 0, 0.5), (1.5, 200, 0.8)],
                         ids=["greedy", "t0.2_p0.9", "k5", "t0.7_k50_p0.6", "t2_p0.5", "t1.5_k200_p0.8"])
@pytest.mark.parametrize("B", [1, 8, 64])
@pytest.mark.parametrize("V", [512, 32000])
def test_scores_against_ref(env, V, B, cfg):
    L = env["L"]
    dev = env["dev"]
    temperature, top_k, top_p = cfg
    z, bias, ids = _tie_free_case(B, V, V + B, cfg)
    want_all = logit_ref.processed_scores(z, bias, temperature, top_k, top_p)
    logits = torch.from_numpy(z).to(dev)
    b_ids = torch.tensor(list(bias), dtype=torch.int32)
    b_val = torch.tensor(list(bias.values()), dtype=torch.float32)
    b_ids_d, b_val_d = b_ids.to(dev), b_val.to(dev)
    L.call("opadpo_logit_bias_add", L.ptr(logits), V, B, V, L.ptr(b_ids_d), L.ptr(b_val_d), b_ids.data_ptr(), len(bias), L.stream())
    torch.cuda.synchronize()
    assert np.array_equal(logits.cpu().numpy(), logit_ref._biased(z, bias)), "logit + bias is one fp32 add per biased entry, nothing else moves"
    s_ids = torch.tensor(ids, dtype=torch.int32)
    s_ids_d = s_ids.to(dev)
    scores = torch.full((B, len(ids)), 123.0, dtype=torch.float32, device=dev)
    L.call("opadpo_gather_scores", L.ptr(logits), V, B, V, L.ptr(s_ids_d), s_ids.data_ptr(), len(ids), temperature, top_k, top_p, L.ptr(scores), L.stream())
    torch.cuda.synchronize()
    got, want = scores.cpu().numpy(), want_all[:, ids]
    assert np.array_equal(np.isneginf(got), np.isneginf(want)), (np.argwhere(np.isneginf(got) != np.isneginf(want))[:8].tolist(),)
    assert np.array_equal(got, want), float(np.nanmax(np.abs(np.where(np.isneginf(want), 0, got - want))))       # bit-equal: one add, one divide
    assert np.array_equal(got[:, 1], got[:, 5])
    if temperature == 0:
        assert not np.isneginf(got).any()
    elif B == 64:
        assert np.isneginf(got).any() and np.isfinite(got).any()      # the case has both kept and cut tokens
    # the same rows at the cap, m = 64: row 0's 40 largest and 24 ranks spread over the vocabulary (wide top-p sets are cut in the middle of these)
    order = np.argsort(-logit_ref._biased(z, bias)[0]).tolist()
    ids64 = order[:40] + [order[(i + 1) * (V - 1) // 24] for i in range(24)]
    s_ids = torch.tensor(ids64, dtype=torch.int32)
    s_ids_d = s_ids.to(dev)
    scores = torch.full((B, 64), 123.0, dtype=torch.float32, device=dev)
    L.call("opadpo_gather_scores", L.ptr(logits), V, B, V, L.ptr(s_ids_d), s_ids.data_ptr(), 64, temperature, top_k, top_p, L.ptr(scores), L.stream())
    torch.cuda.synchronize()
    assert np.array_equal(scores.cpu().numpy(), want_all[:, ids64])
    if top_k == 5 and top_p == 1.0:
        assert int(np.isfinite(want_all).sum(-1).max()) == 5 and int(np.isfinite(want_all).sum(-1).min()) == 5


# ---- end to end: the step-0 scores are the logits of the engine's own forward ----------------------------------------------------------------
def test_step0_scores_equal_the_no_grad_forward(env):
    from opadpo_amd import lib as L
    from opadpo_amd.model import LlavaEngine, SeqBatch
    eng, p, d, dev = env["eng"], env["p"], env["d"], env["dev"]
    B, Q = p["queries"].shape
    V = d.vocab
    # the existing no-grad forward of the same engine (op-level sequencing), one dummy response token: its head rows predict the first token
    ids = torch.cat([p["queries"], torch.full((B, 1), 5, device=dev)], 1).to(torch.int32).contiguous()
    tmask = torch.cat([p["queries_attn_masks"], torch.ones(B, 1, dtype=torch.bool, device=dev)], 1).to(torch.uint8).contiguous()
    batch = SeqBatch(ids, tmask, torch.arange(B, device=dev, dtype=torch.int32), None, 1)
    with torch.no_grad():
        _, _, sv = LlavaEngine.seq_logprobs_fwd(eng, None, batch, env["feats"].contiguous(), 1.0, False)
        torch.cuda.synchronize()
        fwd = sv.logits.view(B, V).clone()
        # the two heads on the same normalised rows: the training head's GEMM and the decode head's weight-streaming GEMM
        a = torch.empty(B, V, dtype=torch.float32, device=dev)
        b = torch.empty_like(a)
        L.gemm_nt(sv.hn.view(B, d.hidden), env["base"].lm_head, a)
        with L.decode_schedule():
            L.gemm_nt(sv.hn.view(B, d.hidden), env["base"].lm_head, b)
        torch.cuda.synchronize()
    assert torch.equal(a, fwd)
    head_gap = float((a - b).abs().max())
    got = _step0_logits(env)
    gap = float((got - fwd.cpu()).abs().max())
    print(f"step-0 scores vs no-grad forward logits: max |diff| = {gap:.3e}; training head vs decode head on the same rows: {head_gap:.3e}")
    assert float(fwd.abs().max()) > 0
    assert gap <= 2 * head_gap, (gap, head_gap)            # head_gap = 0: the same kernel on the same rows, bit-equal
    # with a bias: logit + bias, one more fp32 add (the factor 2 on the heads' distance is for it)
    bias = {3: 1.5, 77: -0.75, V - 1: 0.125}
    gotb = _step0_logits(env, bias)
    wantb = torch.from_numpy(logit_ref.processed_scores(fwd.cpu().numpy(), bias, 0))
    gapb = float((gotb - wantb).abs().max())
    print(f"with a bias: max |diff| = {gapb:.3e}")
    assert gapb <= 2 * head_gap, (gapb, head_gap)
    # sampled configuration: the processed scores are the restatement of the same logits wherever the top-p decision is clear
    for temperature, top_k, top_p in ((0.2, 0, 0.9), (0.8, 20, 0.9)):
        ids_ = fwd[0].argsort(descending=True)[:48].tolist() + [0, 1, EOS, 9]
        _, sc = _gen(env, n_new=1, temperature=temperature, top_k=top_k, top_p=top_p, seed=3, logit_bias=bias, score_ids=ids_)
        want = logit_ref.processed_scores(gotb.numpy(), bias=None, temperature=temperature, top_k=top_k, top_p=top_p)[:, ids_]
        if logit_ref.top_p_margin(gotb.numpy(), None, temperature, top_k, top_p) > MARGIN:
            assert np.array_equal(sc.cpu().numpy(), want)


# ---- graph replay and plain launches agree with a bias set ------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [GREEDY, SAMPLED], ids=["greedy", "sampled"])
def test_graph_and_plain_launches_agree(env, cfg):
    z = _step0_logits(env)
    big = float(z.max() - z.min()) + 1.0
    bias = {int(z[0].argmax()): -big, 11: 0.5 * big, 200: 0.5 * big, EOS: -big, PAD: -big}      # EOS pushed away: every step of every row runs
    ids = [11, 200, int(z[0].argmax()), EOS, 11, 300]
    outs = [_gen(env, n_new=12, use_graph=g, logit_bias=bias, score_ids=ids, **cfg) for g in (False, True, False)]
    for toks, sc in outs[1:]:
        assert torch.equal(toks, outs[0][0]) and torch.equal(sc, outs[0][1])
    toks, sc = outs[0]
    assert toks.shape == (3, 12) and not bool((toks == EOS).any()) and not bool((toks == PAD).any())
    plain = _gen(env, n_new=12, use_graph=True, **cfg)
    assert not torch.equal(plain, toks), "the bias did not change the rollout"
    assert torch.equal(_gen(env, n_new=12, use_graph=True, **cfg), plain)          # and it is gone with the call that set it


# ---- command line ---------------------------------------------------------------------------------------------------------------------------
def _question_file(tmp_path, nq):
    from PIL import Image
    for i in range(nq):
        Image.new("RGB", (12, 7), (10 + 30 * i, 120 - 10 * i, 200)).save(tmp_path / f"x{i}.png")
    qf = tmp_path / "q.jsonl"
    qf.write_text("".join(json.dumps({"question_id": i, "image": f"x{i}.png", "text": f"is there an item {i} ?"}) + "\n" for i in range(nq)))
    return qf


def test_cli_scores_and_bias(env, tmp_path):
    from opadpo_amd import cli_generate as cg
    from opadpo_amd.eval_generate import yes_no_label_ids, yes_no_sequence_bias
    from opadpo_amd.synth import SyntheticTokenizer
    nq = 3
    qf = _question_file(tmp_path, nq)
    common = ["--synthetic", "tiny", "--model-path", "tiny-model", "--question-file", str(qf), "--image-folder", str(tmp_path), "--short_eval", "True"]
    names = ["yes", "no", "Yes", "No", "\nYes", "\nNo"]

    def scores(tag, *extra):
        f = tmp_path / f"{tag}.jsonl"
        cg.main_eval_logit(common + ["--answers-file", str(f), "--output_scores", "True"] + list(extra))
        text = f.read_text()
        assert len(text.splitlines()) == 1 and "question_id" not in text
        got = json.loads(text)
        assert list(got) == names and all(len(got[k]) == nq for k in names)
        return got

    s_def = scores("s_default")                                    # the launcher's defaults: temperature 0.2, no top-p
    assert all(np.isfinite(s_def[k]).all() for k in names)
    scores("s_batched", "--batch-size", "2")                       # batched prompts: same format (the order is pinned in test_eval_logit_cpu.py)
    s_p = scores("s_top_p", "--top_p", "0.5")
    for k in names:                                                # top-p only ever cuts: what stays is the same number
        assert all(a == b or a == -float("inf") for a, b in zip(s_p[k], s_def[k]))
    # greedy: score = logit + bias, so --logit-bias 2 moves 'Yes' by -2 and 'No' by +2 exactly as one fp32 add does
    s0, s2 = scores("s_t0", "--temperature", "0"), scores("s_t0_b2", "--temperature", "0", "--logit-bias", "2.0")
    tok = SyntheticTokenizer(env["d"].vocab)
    lab, bias = yes_no_label_ids(tok), yes_no_sequence_bias(tok, 2.0)
    for k in names:
        add = np.float32(bias.get(lab[k], 0.0))
        assert [float(np.float32(v) + add) for v in s0[k]] == s2[k], k
    assert s0["Yes"] != s2["Yes"] and s0["No"] != s2["No"]
    assert [v * 0.2 for v in s_def["yes"]] == pytest.approx(s0["yes"], rel=1e-6)      # temperature 0.2: the same logits, divided
    # answers: --logit-bias 0 without scores writes what model_vqa.py's main_eval writes at the same temperature and seed
    fa, fb, fc = tmp_path / "a_logit.jsonl", tmp_path / "a_plain.jsonl", tmp_path / "a_bias.jsonl"
    cg.main_eval_logit(common + ["--answers-file", str(fa), "--logit-bias", "0"])
    cg.main_eval(common + ["--answers-file", str(fb), "--temperature", "0.2"])
    cg.main_eval_logit(common + ["--answers-file", str(fc), "--logit-bias", "2.0"])
    pick = lambda f: [(r["question_id"], r["prompt"], r["text"], r["model_id"]) for r in map(json.loads, open(f))]
    assert len(pick(fa)) == nq and pick(fa) == pick(fb)
    assert len(pick(fc)) == nq and [r[0] for r in pick(fc)] == list(range(nq))


# ---- argument checks: refused on the host, nothing launched -------------------------------------------------------------------------------------
def test_argument_checks(env):
    import ctypes as C
    L, dev, eng = env["L"], env["dev"], env["eng"]
    V, B = 512, 4
    logits = torch.randn(B, V, device=dev)
    keep = logits.clone()
    scores = torch.full((B, 70), 7.0, device=dev)

    def table(ids, vals=None):
        h = torch.tensor(ids, dtype=torch.int32)
        return h, h.to(dev), torch.tensor(vals if vals is not None else [1.0] * len(ids), dtype=torch.float32, device=dev)

    def bias_add(ids, n=None, rows=B, null=False):
        h, dv, bv = table(ids)
        L.call("opadpo_logit_bias_add", L.ptr(logits), V, rows, V, None if null else L.ptr(dv), L.ptr(bv), h.data_ptr(), len(ids) if n is None else n, L.stream())

    def gather(ids, rows=B, temperature=1.0, null=False):
        h, dv, _ = table(ids)
        L.call("opadpo_gather_scores", L.ptr(logits), V, rows, V, None if null else L.ptr(dv), h.data_ptr(), len(ids), temperature, 0, 1.0, L.ptr(scores), L.stream())

    for bad in (lambda: bias_add([1, V]), lambda: bias_add([-1]), lambda: bias_add(list(range(65))), lambda: bias_add([4, 9, 4]),
                lambda: bias_add([1, 2], null=True), lambda: bias_add([1], rows=65), lambda: gather([V]), lambda: gather(list(range(65))),
                lambda: gather([1], null=True), lambda: gather([1], rows=65), lambda: gather([1], temperature=-1.0)):
        with pytest.raises(L.OpadpoError):
            bad()
    bias_add([], n=0)                                   # n = 0 / m = 0: accepted, nothing to do
    gather([])
    torch.cuda.synchronize()
    assert torch.equal(logits, keep) and bool((scores == 7.0).all()), "a refused call launched something"
    gather(list(range(64)))                             # the caps themselves are fine
    bias_add(list(range(64)))
    torch.cuda.synchronize()
    assert torch.equal(scores.view(-1)[:B * 64].view(B, 64), keep[:, :64]) and torch.equal(logits[:, :64], keep[:, :64] + 1.0)
    assert torch.equal(logits[:, 64:], keep[:, 64:])
    # the context's setter and the Python keywords
    base = _gen(env, **GREEDY)
    vocab = env["d"].vocab
    arr = lambda t, v: (t * len(v))(*v)
    sc = torch.zeros(3, 2, device=dev)
    for ids, vals in (([1, vocab], [1.0, 1.0]), ([5, 6, 5], [1.0] * 3), (list(range(65)), [1.0] * 65)):
        with pytest.raises(L.OpadpoError):
            eng._call("opadpo_ctx_set_logit_processors", arr(C.c_int32, ids), arr(C.c_float, vals), len(ids), None, 0, None, 0)
    with pytest.raises(L.OpadpoError):
        eng._call("opadpo_ctx_set_logit_processors", None, None, 0, arr(C.c_int32, [1, vocab]), 2, L.ptr(sc), 0)
    with pytest.raises(L.OpadpoError):
        eng._call("opadpo_ctx_set_logit_processors", None, None, 0, arr(C.c_int32, [1, 2]), 2, None, 0)
    for kw in (dict(logit_bias={vocab: 1.0}), dict(score_ids=[-1]), dict(logit_bias={i: 1.0 for i in range(65)}), dict(score_ids=list(range(65)))):
        with pytest.raises(ValueError):
            _gen(env, **GREEDY, **kw)
    assert torch.equal(_gen(env, **GREEDY), base), "a refused setting armed the next generation"
    # beam search refuses an armed context, and the refusal disarms it
    eng._call("opadpo_ctx_set_logit_processors", arr(C.c_int32, [5]), arr(C.c_float, [1.0]), 1, None, 0, None, 0)
    p = env["p"]
    with pytest.raises(L.OpadpoError, match="beam search"):
        eng.generate_beams(None, p["queries"], p["queries_attn_masks"], env["feats"], num_beams=2, max_new_tokens=4, eos_token_id=EOS, pad_token_id=PAD,
                           use_graph=False)
    assert torch.equal(_gen(env, **GREEDY), base)
    with pytest.raises(NotImplementedError, match="CtxEngine"):
        eng.generate_beams(None, p["queries"], p["queries_attn_masks"], env["feats"], num_beams=2, max_new_tokens=4, eos_token_id=EOS, pad_token_id=PAD,
                           use_graph=False, logit_bias={5: 1.0})
