"""GPU, end to end: num_return_sequences - n sampled responses per prompt off one prefill (opadpo_decode_begin_n, CtxEngine.generate,
AutoregressivePolicy.respond, the rollout CLI) at the parity suite's tiny width: the per-row form against repeated prompts (exact), the grouped
form against itself under graph replay, the per-row form's first token and the fp32 oracle, bounds, and the carry-over of refusals."""
import os

import pytest
import torch

from test_parity_gpu import setup  # noqa: F401  (module fixture of the parity suite: tiny dims, oracle weights, CtxEngine)

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
N_NEW, Q = 6, 12
PER_ROW = 1 | (1 << 15)               # context flag word: the defaults (transposed LDS reads) + bit 15, shared-prefix decode attention stays per-row


def prompts(d, B, seed):
    g = torch.Generator().manual_seed(seed)
    images = torch.randn(B, 3, d.image_size, d.image_size, generator=g).to(BF).float()
    queries = torch.randint(3, d.vocab, (B, Q), generator=g)
    qmask = torch.ones(B, Q, dtype=torch.bool)
    for b in range(B):
        pad = b % 4                                   # left padding of 0..3 positions
        queries[b, :pad] = 0
        qmask[b, :pad] = False
        queries[b, 4 + b % 5] = -200                  # the image token
    return images, queries, qmask


def generator_of(s, kind, use_graph=False):
    """-> (Generator, the oracle's LoRA dict)"""
    from opadpo_amd.generate import Generator
    from opadpo_amd.model import LoraAdapter
    vis_only = {k: v for k, v in s["lora_ref"].items() if "vision_tower" in k or "mm_projector" in k}
    if kind == "none":
        return Generator(s["eng"], None, use_graph=use_graph), vis_only
    if kind == "merged":
        return Generator(s["eng"], LoraAdapter(s["d"], s["lora_ref"], s["dev"], trainable=False), use_graph=use_graph, merge_adapter=True), s["lora_ref"]
    return Generator(s["eng"], s["ref"], use_graph=use_graph), s["lora_ref"]                 # unmerged: LoRA tails


SAMPLED = dict(max_new_tokens=N_NEW, temperature=1.0, top_k=30, top_p=0.95, seed=11)
GREEDY = dict(max_new_tokens=N_NEW, temperature=1.0, top_k=1, top_p=1.0, seed=1)


@pytest.mark.parametrize("kind", ["none", "merged", "lora"])
@pytest.mark.parametrize("B,n", [(3, 4), (9, 8), (20, 4)])
def test_per_row_form_equals_repeated_prompts(setup, kind, B, n):
    """Context flag bit 15: generate(..., num_return_sequences=n) draws exactly the tokens of generate(queries.repeat_interleave(n, 0), ...) at the
    same seed - 12 rows on the small path, 72 and 80 rows on the wide GEMMs; one prefill of B prompts instead of B * n."""
    s = setup
    images, queries, qmask = prompts(s["d"], B, seed=300 + B)
    gen, _ = generator_of(s, kind)
    feats = gen.engine.encode_images(images.to(s["dev"]))
    s["eng"].set_flags(use_tr=PER_ROW)
    try:
        got = gen.generate(queries, qmask, image_feats=feats, num_return_sequences=n, **SAMPLED).cpu()
        want = gen.generate(queries.repeat_interleave(n, 0), qmask.repeat_interleave(n, 0), image_feats=feats.repeat_interleave(n, 0), **SAMPLED).cpu()
    finally:
        s["eng"].set_flags()
    assert got.shape == (B * n, N_NEW)
    assert torch.equal(got, want), (got != want).any(1).nonzero().flatten().tolist()
    assert len({tuple(r) for r in got[:n].tolist()}) > 1              # the rows of an item are different draws


@pytest.mark.parametrize("kind,B,n", [("none", 3, 4), ("lora", 3, 4), ("merged", 9, 8)])
def test_per_row_form_with_deferred_residual(setup, kind, B, n):
    """The same equality with context flag bit 13 (residual adds deferred to the RMSNorm that follows): token 0 then expands both addends of the
    prompts' last rows, the hidden rows and the down projection's product, to B * n rows."""
    s = setup
    images, queries, qmask = prompts(s["d"], B, seed=350 + B)
    gen, _ = generator_of(s, kind)
    feats = gen.engine.encode_images(images.to(s["dev"]))
    s["eng"].set_flags(use_tr=PER_ROW | (1 << 13))
    try:
        got = gen.generate(queries, qmask, image_feats=feats, num_return_sequences=n, **SAMPLED).cpu()
        want = gen.generate(queries.repeat_interleave(n, 0), qmask.repeat_interleave(n, 0), image_feats=feats.repeat_interleave(n, 0), **SAMPLED).cpu()
    finally:
        s["eng"].set_flags()
    assert got.shape == (B * n, N_NEW) and torch.equal(got, want), (got != want).any(1).nonzero().flatten().tolist()


@pytest.mark.parametrize("kind", ["none", "merged"])
@pytest.mark.parametrize("B,n", [(3, 4), (9, 8)])
def test_grouped_form(setup, kind, B, n):
    """The library's choice (grouped at head_dim 128).  Precision is the op-level tests' job; here: eager and graph replay agree bit for bit, the
    first token is the per-row form's (no decode attention precedes it), greedy rows of an item are identical and every greedy token's fp32 oracle
    logit lies within 5e-2 of the oracle's top logit on that prefix, sampled rows of an item differ and stay inside the vocabulary."""
    s = setup
    LR, d = s["LR"], s["d"]
    images, queries, qmask = prompts(d, B, seed=400 + B)
    out = {}
    for use_graph in (False, True):
        gen, lora = generator_of(s, kind, use_graph)
        feats = gen.engine.encode_images(images.to(s["dev"]))
        out["sampled", use_graph] = gen.generate(queries, qmask, image_feats=feats, num_return_sequences=n, **SAMPLED).cpu()
        out["greedy", use_graph] = gen.generate(queries, qmask, image_feats=feats, num_return_sequences=n, **GREEDY).cpu()
    assert torch.equal(out["sampled", False], out["sampled", True]) and torch.equal(out["greedy", False], out["greedy", True]), "graph replay differs from eager steps"
    sampled, greedy = out["sampled", False], out["greedy", False]
    assert sampled.shape == (B * n, N_NEW) and int(sampled.min()) >= 0 and int(sampled.max()) < d.vocab
    gen, lora = generator_of(s, kind)
    s["eng"].set_flags(use_tr=PER_ROW)
    try:
        per_row = gen.generate(queries, qmask, image_feats=feats, num_return_sequences=n, **SAMPLED).cpu()
    finally:
        s["eng"].set_flags()
    assert torch.equal(sampled[:, 0], per_row[:, 0])
    for i in range(B):
        rows = sampled[i * n:(i + 1) * n].tolist()
        assert len({tuple(r) for r in rows}) > n // 2, (i, rows)      # more than half of an item's rows differ from each other
        assert bool((greedy[i * n:(i + 1) * n] == greedy[i * n]).all()), (i, greedy[i * n:(i + 1) * n])
    # greedy against the oracle, teacher-forced on the generated tokens (the rows of an item are identical: one oracle row per item)
    first = greedy[::n]
    feats_o = LR.image_features(images, s["W"], lora, s["od"])
    ids = torch.cat([queries, first], 1)
    mask = torch.cat([qmask, torch.ones_like(first, dtype=torch.bool)], 1)
    with torch.no_grad():
        logits = LR.llava_logits(ids, mask, None, s["W"], lora, s["od"], feats=feats_o).float()
    q = Q + d.n_patches - 1
    worst = 0.0
    for i in range(B):
        for t in range(N_NEW):
            z = logits[i, q - 1 + t]
            gap = float(z.max() - z[int(first[i, t])])
            worst = max(worst, gap)
            assert gap <= 5e-2, (i, t, gap)
            if int(first[i, t]) == 2:                                   # EOS: pad from here on
                assert bool((first[i, t + 1:] == 0).all())
                break
    print(f"grouped {kind} B={B} n={n}: worst oracle gap of a greedy token {worst:.3e}")


def test_policy_respond(setup):
    """AutoregressivePolicy.respond(num_return_sequences=3): shape, pad after EOS, the tokens of CtxEngine.generate with the reference's warpers
    (top_k = 0, top_p = 1) at the same seed, and the policy's next training forward and backward as before the call."""
    s = setup
    from opadpo_amd.dims import EOS_ID, PAD_ID
    from opadpo_amd.policy import AutoregressivePolicy
    from test_parity_gpu import make_inputs
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
    got = pol.respond(queries, qmask, images.to(s["dev"]), num_return_sequences=n, seed=7)["responses"].cpu()
    assert got.shape == (B * n, T) and got.dtype == torch.int64
    for row in got.tolist():
        if EOS_ID in row:
            assert all(t == PAD_ID for t in row[row.index(EOS_ID) + 1:]), row
    feats = s["eng"].encode_images(images.to(s["dev"]))
    want = s["eng"].generate(s["pol"], queries, qmask, feats, max_new_tokens=T, temperature=0.9, top_k=0, top_p=1.0, seed=7, eos_token_id=EOS_ID,
                             pad_token_id=PAD_ID, suppress_eos=False, use_graph=False, num_return_sequences=n).cpu()
    assert torch.equal(got, want)
    assert pol.respond(queries, qmask, images.to(s["dev"]), seed=7)["responses"].shape == (B, T)        # n = 1: the existing path
    lp1, g1 = train_pass()
    assert torch.equal(lp0, lp1) and torch.equal(g0, g1)
    s["pol"].grad.zero_()
    # between a training forward and its backward, in grad mode: refused
    out = pol(images=images.to(s["dev"]), queries=queries, queries_attn_masks=qmask, **one)
    with pytest.raises(RuntimeError, match="backward"):
        pol.respond(queries, qmask, images.to(s["dev"]), num_return_sequences=n)
    out["standard_response_logprobs"].sum().backward()
    s["pol"].grad.zero_()


def test_bounds_and_carry_over(setup):
    """B * n = 256 generates; above 256 rows, n = 0 and n = 17 are refused with text that names the bound; armed logit processors with B * n = 65
    are refused and disarm, and the plain generation that follows is unchanged; the op-level engine and beam search refuse n > 1."""
    s = setup
    from opadpo_amd import lib as L
    from opadpo_amd.generate import Generator
    from opadpo_amd.model import LlavaEngine
    d = s["d"]
    images, queries, qmask = prompts(d, 129, seed=21)
    gen = Generator(s["eng"], None, use_graph=False)
    feats = gen.engine.encode_images(images.to(s["dev"]))
    out = gen.generate(queries[:16], qmask[:16], image_feats=feats[:16], num_return_sequences=16, **SAMPLED).cpu()
    assert out.shape == (256, N_NEW) and int(out.min()) >= 0 and int(out.max()) < d.vocab
    with pytest.raises(L.OpadpoError, match="256"):
        gen.generate(queries, qmask, image_feats=feats, num_return_sequences=2, **SAMPLED)                     # 258 rows
    for bad in (0, 17):
        with pytest.raises(L.OpadpoError, match="16"):
            gen.generate(queries[:2], qmask[:2], image_feats=feats[:2], num_return_sequences=bad, **SAMPLED)
    plain = gen.generate(queries[:13], qmask[:13], image_feats=feats[:13], num_return_sequences=5, **SAMPLED).cpu()
    with pytest.raises(L.OpadpoError, match="64"):
        gen.generate(queries[:13], qmask[:13], image_feats=feats[:13], num_return_sequences=5, logit_bias={5: 2.0}, **SAMPLED)
    with pytest.raises(L.OpadpoError, match="64"):
        gen.generate(queries[:13], qmask[:13], image_feats=feats[:13], num_return_sequences=5, score_ids=[5, 7], **SAMPLED)
    assert torch.equal(gen.generate(queries[:13], qmask[:13], image_feats=feats[:13], num_return_sequences=5, **SAMPLED).cpu(), plain)
    # 64 rows with an armed bias: accepted, [B * n, m] scores
    tok, sc = gen.generate(queries[:16], qmask[:16], image_feats=feats[:16], num_return_sequences=4, score_ids=[5, 7], **SAMPLED)
    assert tok.shape == (64, N_NEW) and sc.shape == (64, 2)
    with pytest.raises(NotImplementedError):
        gen.generate(queries[:2], qmask[:2], image_feats=feats[:2], num_return_sequences=2, num_beams=2, **GREEDY)
    with pytest.raises(NotImplementedError):
        Generator(LlavaEngine(s["eng"].base), None).generate(queries[:2], qmask[:2], image_feats=feats[:2], num_return_sequences=2, **SAMPLED)


def test_rollout_cli_num_return_sequences(tmp_path, monkeypatch):
    """--synthetic tiny rollout with --num_return_sequences 2 writes 2 x rows records, the query-side columns repeated item-major."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from opadpo_amd import cli_generate as cg
    from opadpo_amd.dataset_build import load_rollout_records
    out = str(tmp_path / "gen")
    ns, _ = cg.rollout_parser().parse_known_args(
        ["--synthetic", "tiny", "--synthetic_rows", "5", "--output_dir", out, "--rollout_batch_size", "4", "--rollout_per_device_batch_size", "2",
         "--query_len", "64", "--response_len", "6", "--top_k", "10", "--num_return_sequences", "2"])
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("WORLD_SIZE", "1")
    files = cg.run_rollout(ns, log=lambda *_: None)
    assert [os.path.basename(f) for f in files] == ["step0_rank0.json", "step1_rank0.json"]
    recs = load_rollout_records([os.path.join(out, "rollouts")], log=lambda *_: None)
    assert len(recs) == 10
    assert [r["image_id"] for r in recs] == [f"synthetic_{i // 2}.png" for i in range(10)]
    assert all(recs[2 * i]["query"] == recs[2 * i + 1]["query"] and recs[2 * i]["standard_response"] == recs[2 * i + 1]["standard_response"] for i in range(5))
