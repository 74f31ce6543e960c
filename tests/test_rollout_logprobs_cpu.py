"""CPU: per-token log-probs of the rollout on the host side - the float64 restatement (tests/logprob_ref.py) against torch, the zeroing
Generator.rollout applies after the EOS / '?' cut, rollout_step's three per-response columns, the CLI flag, and the extra keys through the
dataset builder."""
import io
import json
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "opa-dpo_amd"))
sys.path.insert(0, os.path.dirname(__file__))
import logprob_ref                                  # noqa: E402
from opadpo_amd import rollout_data as rd          # noqa: E402
from toy_tokenizer import ToyTokenizer            # noqa: E402

LP_COLS = ["original_generate_response_logprob", "original_generate_response_tokens", "original_generate_response_entropy"]


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("temperature", [0, 0.7, 1, 2])
def test_restatement_against_torch(temperature):
    g = torch.Generator().manual_seed(3)
    rows, V = 7, 132
    logits = (3.0 * torch.randn(rows, V, generator=g)).to(torch.float32)
    logits[5] += 1.0e4
    tokens = torch.randint(1, V, (rows,), generator=g)
    tokens[2] = 0                                                       # a pad row
    z = logprob_ref.scaled(logits.numpy(), temperature)
    inv = np.float32(1.0) if temperature == 0 else np.float32(1.0) / np.float32(temperature)
    assert z.dtype == np.float32 and np.array_equal(z, logits.numpy() * inv)
    logp, ent = logprob_ref.token_logprobs(z, tokens.numpy())
    ls = torch.log_softmax(torch.from_numpy(z).double(), -1)
    want_lp = ls.gather(1, tokens.view(-1, 1)).view(-1)
    want_ent = -(ls.exp() * ls).sum(-1)
    keep = tokens != 0
    # float64 both ways: the shifted row (|z| = 1e4, ulp 1.8e-12) bounds the difference
    assert np.abs(logp - want_lp.numpy())[keep.numpy()].max() < 1e-10
    assert np.abs(ent - want_ent.numpy())[keep.numpy()].max() < 1e-10
    assert logp[2] == 0 and math.copysign(1.0, logp[2]) == -1.0 and ent[2] == 0
    assert (logp[keep.numpy()] < 0).all() and (ent[keep.numpy()] > 0).all()


def test_restatement_drops_minus_inf_columns_and_knows_the_uniform_row():
    V = 128
    z = np.zeros((3, V), dtype=np.float32)
    z[1] = 2.5                                                          # all equal: ent = ln V, logp = -ln V
    z[2, 7] = -np.inf
    logp, ent = logprob_ref.token_logprobs(z, [3, 9, 5])
    assert np.allclose(logp[:2], -math.log(V), atol=1e-14) and np.allclose(ent[:2], math.log(V), atol=1e-14)
    assert abs(logp[2] + math.log(V - 1)) < 1e-14 and abs(ent[2] - math.log(V - 1)) < 1e-14 and np.isfinite(ent).all()
    with pytest.raises(AssertionError):
        logprob_ref.token_logprobs(z, [3, 9, 7])                        # the token on the -inf column
    a, b = logprob_ref.token_logprobs(z + np.float32(64.0), [3, 9, 5])
    assert np.allclose(a, logp, atol=1e-12) and np.allclose(b, ent, atol=1e-12)


# ---- Generator.rollout zeroes what the cut removed --------------------------------------------------------------------------------------
def test_rollout_zeroes_logprobs_behind_the_cut():
    from opadpo_amd.generate import Generator
    from opadpo_amd.dims import EOS_ID, PAD_ID
    resp = torch.tensor([[5, 6, EOS_ID, PAD_ID, PAD_ID, PAD_ID],         # finished by itself: the engine already wrote -0.0 / 0 behind EOS
                         [5, 1577, 8, 9, EOS_ID, PAD_ID],                # '?' cuts before EOS: positions 2..4 carried real values
                         [7, 8, 9, 10, 11, 12],                          # never cut
                         [PAD_ID, 4, EOS_ID, 29973, 3, 3]])              # a sampled pad id; the later stop id wins the cut
    logp = -torch.arange(1, 25, dtype=torch.float32).view(4, 6) / 8
    ent = torch.arange(1, 25, dtype=torch.float32).view(4, 6) / 16
    calls = []

    class Stub(Generator):
        def __init__(self):
            pass

        def generate(self, queries, masks, images, **kw):
            calls.append(kw)
            return (resp.clone(), logp.clone(), ent.clone()) if kw.get("output_logprobs") else resp.clone()

    g = Stub()
    plain = g.rollout(None, None, None, response_len=6)
    assert torch.is_tensor(plain) and "output_logprobs" not in calls[-1]
    toks, lp, en = g.rollout(None, None, None, response_len=6, output_logprobs=True)
    assert calls[-1]["output_logprobs"] is True and torch.equal(toks, plain)
    want = torch.tensor([[5, 6, EOS_ID, 0, 0, 0], [5, 1577, 0, 0, 0, 0], [7, 8, 9, 10, 11, 12], [0, 4, EOS_ID, 29973, 0, 0]])
    assert torch.equal(toks, want)
    pad = want == PAD_ID
    assert bool((lp[pad] == 0).all()) and bool((en[pad] == 0).all())
    assert torch.equal(lp[~pad], logp[~pad]) and torch.equal(en[~pad], ent[~pad])
    assert lp.dtype == torch.float32 and lp.shape == toks.shape == en.shape


# ---- rollout_step -------------------------------------------------------------------------------------------------------------------------
def _png(color):
    from PIL import Image
    buf = io.BytesIO()
    Image.new("RGB", (6, 4), color).save(buf, format="PNG")
    return buf.getvalue()


def _rows():
    return [{"question": "what is on the mat ?", "chosen": "a cat sits there", "image": {"bytes": _png((255, 0, 0)), "path": "a.png"}},
            {"question": "describe the scene", "chosen": "two dogs", "image": {"bytes": _png((0, 255, 0)), "path": "b.png"}},
            {"question": "last one ?", "chosen": "yes it is the last one indeed", "image": {"bytes": _png((9, 9, 9)), "path": "d.png"}}]


TEXTS = ["red green", "", "blue", "cat dog mat", "sun", "sky sea", "mat", "red", "dog dog"]          # response k of a step; "" = an empty response
WIDTH = 5


def _sampler(tok, N, with_lp, bad_shape=False, mix=False):
    state = {"k": 0, "calls": 0}

    def sample(q, m, img):
        rows, lps, ens = [], [], []
        for _ in range(q.shape[0] * N):
            k = state["k"]
            ids = tok._encode(TEXTS[k])[1:] + [tok.eos_token_id] if TEXTS[k] else []
            ids = ids + [tok.pad_token_id] * (WIDTH - len(ids))
            rows.append(ids)
            # values at pad positions are junk on purpose: the columns must not read them
            lps.append([-(k + 1) * 0.25 - 0.125 * j for j in range(WIDTH)])
            ens.append([0.5 + 0.0625 * k + 0.25 * j for j in range(WIDTH)])
            state["k"] += 1
        state["calls"] += 1
        r = torch.tensor(rows)
        if not with_lp or (mix and state["calls"] == 2):
            return r
        lp, en = torch.tensor(lps, dtype=torch.float32), torch.tensor(ens, dtype=torch.float32)
        return (r, lp[:, :-1], en) if bad_shape else (r, lp, en)
    return sample


@pytest.mark.parametrize("N", [1, 3])
def test_rollout_step_columns(N):
    from opadpo_amd import online_generate as og
    tok = ToyTokenizer()
    ds = rd.QueryResponseDataset(_rows(), tok, query_len=48, image_size=8, log=lambda *_: None)
    batches = [rd.collate_query_response([ds[0], ds[1]]), rd.collate_query_response([ds[2]])]
    off = og.rollout_step(batches, tok, _sampler(tok, N, False), None, num_return_sequences=N)
    on = og.rollout_step(batches, tok, _sampler(tok, N, True), None, num_return_sequences=N)
    assert not any(c in off for c in LP_COLS)                               # present only when asked
    assert list(on) == list(off) + LP_COLS and list(og.LOGPROB_COLUMNS) == LP_COLS
    assert all(on[k] == off[k] for k in off) and all(len(on[c]) == 3 * N for c in LP_COLS)
    for k in range(3 * N):
        n = len(tok._encode(TEXTS[k])[1:]) + 1 if TEXTS[k] else 0
        assert on[LP_COLS[1]][k] == n and isinstance(on[LP_COLS[1]][k], int)
        want_lp = sum(-(k + 1) * 0.25 - 0.125 * j for j in range(n))
        want_en = sum(0.5 + 0.0625 * k + 0.25 * j for j in range(n)) / n if n else 0.0
        assert on[LP_COLS[0]][k] == want_lp and on[LP_COLS[2]][k] == want_en, k        # dyadic values: exact
        assert isinstance(on[LP_COLS[0]][k], float) and isinstance(on[LP_COLS[2]][k], float)
    assert on[LP_COLS[1]][1] == 0 and on[LP_COLS[0]][1] == 0.0 and on[LP_COLS[2]][1] == 0.0      # the empty response
    json.dumps({c: on[c] for c in LP_COLS})                                  # plain Python numbers
    with pytest.raises(ValueError, match="logp"):
        og.rollout_step(batches, tok, _sampler(tok, N, True, bad_shape=True), None, num_return_sequences=N)
    with pytest.raises(ValueError, match="mix"):
        og.rollout_step(batches, tok, _sampler(tok, N, True, mix=True), None, num_return_sequences=N)


def test_generator_sampler_passes_the_keyword():
    from opadpo_amd import online_generate as og
    seen = []

    class Gen:
        engine = types.SimpleNamespace(dev="cpu")

        def rollout(self, q, m, img, **kw):
            seen.append(kw)
            r = torch.zeros(2, 4, dtype=torch.long)
            return (r, torch.zeros(2, 4), torch.zeros(2, 4)) if kw.get("output_logprobs") else r

    q = torch.zeros(2, 3, dtype=torch.long)
    out = og.generator_sampler(Gen(), response_len=4)(q, q, q)
    assert torch.is_tensor(out) and "output_logprobs" not in seen[-1]
    out = og.generator_sampler(Gen(), response_len=4, output_logprobs=True)(q, q, q)
    assert isinstance(out, tuple) and len(out) == 3 and seen[-1]["output_logprobs"] is True


# ---- command line and dataset builder -----------------------------------------------------------------------------------------------------------
def test_cli_flag():
    from opadpo_amd import cli_generate as cg
    ns, _ = cg.rollout_parser().parse_known_args([])
    assert ns.output_logprobs is False
    for text, want in (("True", True), ("1", True), ("False", False), ("0", False)):
        ns, _ = cg.rollout_parser().parse_known_args(["--output_logprobs", text])
        assert ns.output_logprobs is want
    sh = open(os.path.join(os.path.dirname(__file__), "..", "run", "online_generate.sh")).read()
    assert "OUTPUT_LOGPROBS=${OUTPUT_LOGPROBS:-0}" in sh and "--output_logprobs $OUTPUT_LOGPROBS" in sh


def test_extra_keys_pass_through_the_dataset_builder(tmp_path):
    from opadpo_amd import dataset_build as db
    from opadpo_amd import online_generate as og
    tok = ToyTokenizer()
    ds = rd.QueryResponseDataset(_rows(), tok, query_len=48, image_size=8, log=lambda *_: None)
    batches = [rd.collate_query_response([ds[0], ds[1]]), rd.collate_query_response([ds[2]])]

    def feedback(urls, queries, responses, standard):
        return {"Pseudo_response": [r + " (fixed)" for r in responses], "Generated_response": list(responses), "report_json": [{"ok": 1}] * len(responses)}

    cols = og.rollout_step(batches, tok, _sampler(tok, 1, True), feedback)
    path = db.write_rollout_json(str(tmp_path), 0, cols, rank=0)
    stored = json.load(open(path))
    assert len(stored) == 3 and all(set(LP_COLS) <= set(r) for r in stored)
    rows = db.build_rows(os.path.join(str(tmp_path), "rollouts"), log=lambda *_: None)
    assert len(rows) == 3
    for k, r in enumerate(rows):
        assert [r[c] for c in LP_COLS] == [cols[c][k] for c in LP_COLS]
    # the training datasets select their columns by name: the extra keys change neither
    off = og.rollout_step(batches, tok, _sampler(tok, 1, False), feedback)
    db.write_rollout_json(str(tmp_path / "off"), 0, off, rank=0)
    rows_off = db.build_rows(os.path.join(str(tmp_path / "off"), "rollouts"), log=lambda *_: None)
    assert db.opa_columns(rows) == db.opa_columns(rows_off) and db.opadpo_columns(rows) == db.opadpo_columns(rows_off)
    assert not any(c in db.opadpo_columns(rows) for c in LP_COLS)
