"""GPU: beam search (opadpo_beam_step, opadpo_attn_decode_beam, opadpo_decode_beam_begin / _result, CtxEngine.generate_beams, the eval
CLI's --num_beams) against tests/beam_ref.py, the fused decode attention and the oracle."""
import json

import pytest
import torch

import beam_ref

pytestmark = pytest.mark.gpu


def _lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from opadpo_amd import lib as L
    L.load()
    return L


def _distinct_logits(g, rows, V, eos, eos_boost):
    x = torch.randn(rows, V, generator=g) * 3.0
    x[:, eos] += eos_boost
    return x


# ---- selection: opadpo_beam_step against beam_ref on identical fp32 logits -------------------------------------------------------------
@pytest.mark.parametrize("V", [512, 32000])
@pytest.mark.parametrize("k", [1, 2, 4, 8])
@pytest.mark.parametrize("B", [1, 3])
def test_beam_step_against_ref(V, k, B, record_property):
    L = _lib()
    dev = torch.device("cuda")
    rows, max_new, eos, pad = B * k, 7, 2, 0
    cases = {"first": 0, "eos_top_k": 0, "eos_beyond_k": 0, "early_stop": 0}
    for seed in range(4):
        g = torch.Generator().manual_seed(1000 * seed + 10 * k + B)
        ref = beam_ref.BeamSearch(B, k, V, max_new, eos, pad)
        z = lambda *s, dt=torch.int32: torch.zeros(*s, dtype=dt, device=dev)
        run, cval, ctok = z(rows, dt=torch.float32), z(rows * 2 * k, dt=torch.float32), z(rows * 2 * k)
        fsc, finfo, fn, done = z(rows, dt=torch.float32), z(3, rows), z(B), z(B, dt=torch.uint8)
        cur, bp, table = z(rows), z(2, max_new, rows), z(2, rows, max_new)
        boost = [0.0, 4.0, 12.0, 30.0][seed]            # EOS beyond k, among the top k, everywhere (a full finished set: early stop)
        for t in range(max_new):
            for attempt in range(50):                   # no two candidates of a live item within 1e-4
                logits = _distinct_logits(g, rows, V, eos, boost)
                probe = beam_ref.BeamSearch(B, k, V, max_new, eos, pad)
                probe.__dict__.update({kk: (vv.clone() if torch.is_tensor(vv) else vv) for kk, vv in ref.__dict__.items()})
                probe.margin = float("inf")
                probe.step(logits)
                if probe.margin > 1e-4:
                    break
            was_done = ref.done.clone()
            lp = torch.log_softmax(logits, -1).view(B, k, V) + ref.run[:, :, None]
            order = lp.reshape(B, -1).argsort(-1, descending=True)[:, :2 * k] % V
            for b in range(B):
                if not was_done[b]:
                    pos = (order[b] == eos).nonzero()
                    if len(pos):
                        cases["eos_top_k" if int(pos[0]) < k else "eos_beyond_k"] += 1
            ref = probe
            cases["first"] += int(t == 0)
            logits_d = logits.to(dev)
            L.call("opadpo_beam_step", L.ptr(logits_d), V, B, k, V, t, max_new, eos, pad, L.ptr(run), L.ptr(cval), L.ptr(ctok), L.ptr(fsc),
                   L.ptr(finfo), L.ptr(fn), L.ptr(done), L.ptr(cur), L.ptr(bp), L.ptr(table), L.stream())
            torch.cuda.synchronize()
            assert torch.equal(done.cpu().bool(), ref.done), (t, done, ref.done)
            live = ~was_done
            if t == max_new - 1:          # every candidate is finished: the running beams (all at -1e9) are never used again
                live = torch.zeros_like(live)
            got_tok, got_par = cur.cpu().view(B, k), bp[0, t].cpu().view(B, k)
            assert torch.equal(got_tok[live], ref.tokens[live].to(torch.int32)), (t, got_tok, ref.tokens)
            assert torch.equal(got_par[live], ref.parents[live].to(torch.int32)), (t, got_par, ref.parents)
            if t < max_new - 1:
                gr = run.cpu().view(B, k)[live]
                assert torch.allclose(gr, ref.run[live], rtol=1e-5, atol=1e-5), (gr, ref.run[live])
            nfin = fn.cpu()
            for b in range(B):
                n = int(nfin[b])
                assert n == int(ref.fin_ok[b].sum())
                assert torch.allclose(fsc.cpu().view(B, k)[b, :n], ref.fin_score[b, :n], rtol=1e-5, atol=1e-5)   # lse of a 32000-row in fp32: ~1e-6 absolute
            if bool(ref.done.all()):
                cases["early_stop"] += int(t < max_new - 1)
                break
    assert cases["first"] and cases["eos_top_k"] + cases["eos_beyond_k"] > 0, cases
    record_property("beam_step_cases", json.dumps(cases))


# ---- beam attention against the fused decode attention on the materialised per-row cache: bit-identical ---------------------------------
@pytest.mark.parametrize("B,k,Lp,max_new,s", [(1, 4, 600, 64, 0), (1, 4, 600, 64, 37), (2, 3, 40, 16, 15), (3, 4, 1100, 32, 20), (8, 8, 300, 24, 9)])
def test_beam_attention_bit_identical(B, k, Lp, max_new, s):
    L = _lib()
    dev = torch.device("cuda")
    nh, hd = 32, 128                       # 7B heads
    H, rows, max_ctx, pos = nh * hd, B * k, Lp + max_new, Lp + s
    g = torch.Generator().manual_seed(B * 100 + k * 10 + s)
    bf = torch.bfloat16
    qkv = torch.randn(rows, 3 * H, generator=g).to(bf).to(dev)
    kp, vp = [torch.randn(B, nh, Lp, hd, generator=g).to(bf).to(dev) for _ in range(2)]
    ks, vs = [torch.randn(rows, nh, max_new, hd, generator=g).to(bf).to(dev) for _ in range(2)]
    pmask = torch.ones(B, Lp, dtype=torch.uint8)
    pmask[0, :5] = 0                                         # left padding of item 0
    table = torch.stack([torch.randint(0, k, (max_new,), generator=g) + (i // k) * k for i in range(rows)]).to(torch.int32)
    cos = torch.randn(max_ctx, hd // 2, generator=g).to(dev)
    sin = torch.randn(max_ctx, hd // 2, generator=g).to(dev)
    # materialised per-row caches and mask
    item = torch.arange(rows) // k
    kc = torch.zeros(rows, nh, max_ctx, hd, dtype=bf, device=dev)
    vc = torch.zeros_like(kc)
    kc[:, :, :Lp], vc[:, :, :Lp] = kp[item], vp[item]
    for i in range(rows):
        for sl in range(s):
            kc[i, :, Lp + sl] = ks[int(table[i, sl]), :, sl]
            vc[i, :, Lp + sl] = vs[int(table[i, sl]), :, sl]
    km = torch.ones(rows, max_ctx, dtype=torch.uint8)
    km[:, :Lp] = pmask[item]
    pos_d = torch.tensor([pos], dtype=torch.int32, device=dev)
    km_d, pmask_d, table_d = km.to(dev), pmask.to(dev), table.to(dev)      # held: a freed temporary's block would be reused by the next copy
    wsb = L.load().opadpo_attn_decode_workspace_bytes(rows, nh, hd, max_ctx)
    ws = torch.empty(max(wsb, 4), dtype=torch.uint8, device=dev)
    o_ref = torch.empty(rows, H, dtype=bf, device=dev)
    o = torch.empty_like(o_ref)
    scale = hd ** -0.5
    L.call("opadpo_attn_decode_fused", L.ptr(qkv), 3 * H, L.ptr(cos), L.ptr(sin), L.ptr(kc), L.ptr(vc), L.ptr(o_ref), L.ptr(km_d), rows, nh, hd,
           L.ptr(pos_d), max_ctx, scale, L.ptr(ws), wsb, L.stream())
    L.call("opadpo_attn_decode_beam", L.ptr(qkv), 3 * H, L.ptr(cos), L.ptr(sin), L.ptr(kp), L.ptr(vp), L.ptr(ks), L.ptr(vs), L.ptr(o), L.ptr(pmask_d),
           B, k, nh, hd, L.ptr(pos_d), Lp, max_new, L.ptr(table_d), scale, L.ptr(ws), wsb, L.stream())
    torch.cuda.synchronize()
    bad = (o.view(torch.int16) != o_ref.view(torch.int16)).view(rows, nh, hd)
    assert not bool(bad.any()), (int(bad.sum()), bad.any(-1).nonzero()[:8].tolist(), float((o.float() - o_ref.float()).abs().max()))
    assert torch.equal(ks[:, :, s].view(torch.int16), kc[:, :, pos].view(torch.int16))
    assert torch.equal(vs[:, :, s].view(torch.int16), vc[:, :, pos].view(torch.int16))


# ---- end to end at tiny width against the oracle ------------------------------------------------------------------------------------
from test_parity_gpu import make_inputs, setup  # noqa: E402,F401  (module fixture of the parity suite)


def _oracle_logprobs(LR, s, lora, feats, queries, qmask, gen):
    """fp32 oracle log-probabilities of the next token after queries + gen ([R, t]) -> [R, V]"""
    ids = torch.cat([queries, gen], 1)
    mask = torch.cat([qmask, torch.ones_like(gen, dtype=torch.bool)], 1)
    return LR.llava_logits(ids, mask, None, s["W"], lora, s["od"], feats=feats)[:, -1].float()


@pytest.mark.parametrize("kind,B,k", [("none", 2, 3), ("lora", 2, 3), ("merged", 2, 4), ("none", 3, 4), ("merged", 2, 5)])
def test_generate_beams_against_oracle(setup, kind, B, k, record_property):
    s = setup
    LR = s["LR"]
    from opadpo_amd.generate import Generator
    from opadpo_amd.model import LoraAdapter
    N, eos, pad = 8, 2, 0
    images, queries, qmask, _ = make_inputs(s["d"], B, 12, 9, seed=70 + B * k)
    vis_only = {kk: v for kk, v in s["lora_ref"].items() if "vision_tower" in kk or "mm_projector" in kk}
    if kind == "none":
        adapter, lora, merge = None, vis_only, False
    elif kind == "lora":
        adapter, lora, merge = s["ref"], s["lora_ref"], False
    else:
        adapter, lora, merge = LoraAdapter(s["d"], s["lora_ref"], s["dev"], trainable=False), s["lora_ref"], True
    outs = []
    for use_graph in (False, True):
        gen = Generator(s["eng"], adapter, use_graph=use_graph, merge_adapter=merge)
        feats = gen.engine.encode_images(images.to(s["dev"]))
        outs.append(s["eng"].generate_beams(gen.adapter, queries, qmask, feats, num_beams=k, max_new_tokens=N, eos_token_id=eos, pad_token_id=pad,
                                            use_graph=use_graph))
        torch.cuda.synchronize()
    (tok, sc), (tok_g, sc_g) = [(a.cpu(), b.cpu()) for a, b in outs]
    assert torch.equal(tok, tok_g) and torch.equal(sc, sc_g), "graph replay changed the beam search"
    feats_o = LR.image_features(images, s["W"], lora, s["od"])
    Rk = queries.repeat_interleave(k, 0), qmask.repeat_interleave(k, 0), feats_o.repeat_interleave(k, 0)
    with torch.no_grad():
        o_tok, o_sc, st = beam_ref.beam_search(lambda gen_: _oracle_logprobs(LR, s, lora, Rk[2], Rk[0], Rk[1], gen_), B, k, s["d"].vocab, N, eos, pad)
    exact = 0
    for b in range(B):
        row = tok[b].tolist()
        n = row.index(eos) + 1 if eos in row else N
        assert all(t == pad for t in row[n:])
        gen_ = torch.tensor(row[:n])[None]
        lp = torch.log_softmax(LR.llava_logits(torch.cat([queries[b:b + 1], gen_], 1), torch.cat([qmask[b:b + 1], torch.ones(1, n, dtype=torch.bool)], 1),
                                               None, s["W"], lora, s["od"], feats=feats_o[b:b + 1]).float(), -1)
        q = queries.shape[1] + s["d"].n_patches - 1
        tf = float(sum(lp[0, q - 1 + j, row[j]] for j in range(n))) / n
        assert abs(tf - float(sc[b])) <= 2e-2, (b, tf, float(sc[b]))                          # (a) score of the returned tokens
        assert tf >= float(o_sc[b]) - 2e-2, (b, tf, float(o_sc[b]))                            # (b) as good as the oracle's best
        exact += int(row == o_tok[b].tolist())
    if st.margin > 5e-2:
        assert exact == B, (tok, o_tok, st.margin)                                              # (c) same sequences where decisions are clear
    record_property("beam_exact_match", json.dumps({"exact": exact, "of": B, "margin": st.margin}))      # the test report's record
    print(f"beam exact match {kind} B={B} k={k}: {exact}/{B} (oracle margin {st.margin:.2e})")


# ---- the eval CLI honours --num_beams ------------------------------------------------------------------------------------------------
def test_eval_cli_num_beams(tmp_path):
    _lib()
    from PIL import Image
    from opadpo_amd import cli_generate as cg
    from opadpo_amd.eval_generate import answer_questions
    nq = 8
    for i in range(nq):
        Image.new("RGB", (12, 7), (10 + 30 * i, 120 - 10 * i, 200)).save(tmp_path / f"x{i}.png")
    qf = tmp_path / "q.jsonl"
    questions = [{"question_id": i, "image": f"x{i}.png", "text": f"what is item {i} ?"} for i in range(nq)]
    qf.write_text("".join(json.dumps(q) + "\n" for q in questions))
    ans = tmp_path / "beam.jsonl"
    argv = ["--synthetic", "tiny", "--model-path", "tiny-model", "--question-file", str(qf), "--image-folder", str(tmp_path), "--answers-file", str(ans),
            "--short_eval", "True", "--num_beams", "3", "--test-prompt", ""]
    cg.main_eval(argv)
    got = [json.loads(x)["text"] for x in open(ans)]
    assert len(got) == nq
    ns, _ = cg.eval_parser().parse_known_args(argv)
    engine, adapter, tok = cg._engine(ns.model_path, ns.synthetic, None, ns.lora_rank, ns.lora_alpha)
    kw = dict(adapter=adapter, short_eval=True, test_prompt="", image_size=engine.d.image_size, pad_to_square=ns.image_aspect_ratio == "pad")
    answer_questions(engine, tok, questions, str(tmp_path), str(tmp_path / "b3.jsonl"), num_beams=3, **kw)
    answer_questions(engine, tok, questions, str(tmp_path), str(tmp_path / "g.jsonl"), **kw)
    beam = [json.loads(x)["text"] for x in open(tmp_path / "b3.jsonl")]
    greedy = [json.loads(x)["text"] for x in open(tmp_path / "g.jsonl")]
    assert got == beam
    assert any(a != b for a, b in zip(beam, greedy)), "num_beams=3 answered every question exactly as greedy decoding"
