"""CPU: the yes/no evaluation generator's host side (cli_generate.eval_logit_parser / main_eval_logit, eval_generate.yes_no_label_ids /
yes_no_sequence_bias / answer_questions' score trailer) and tests/logit_ref.py, the restatement the GPU tests compare the kernels with.
The six label ids are pinned against tests/toy_tokenizer.py only: the Llama sentencepiece model is not available offline."""
import json
import types

import numpy as np
import pytest
import torch

import logit_ref
from toy_tokenizer import ToyTokenizer

INF = float("inf")


# ---- command line ---------------------------------------------------------------------------------------------------------------------
def test_parser_defaults_and_flags():
    from opadpo_amd import cli_generate as cg
    ns = cg.eval_logit_parser().parse_args([])
    assert ns.temperature == 0.2 and ns.logit_bias == 0 and ns.output_scores is False and ns.num_beams == 1 and ns.top_p is None
    base = cg.eval_parser().parse_args([])
    assert base.temperature == 0.0 and not hasattr(base, "output_scores") and not hasattr(base, "logit_bias")      # model_vqa.py's parser stays as it is
    for k, v in vars(base).items():
        if k != "temperature":
            assert getattr(ns, k) == v, k
    ns = cg.eval_logit_parser().parse_args(["--output_scores", "True", "--logit-bias", "2.5", "--temperature", "0"])
    assert ns.output_scores is True and ns.logit_bias == 2.5 and ns.temperature == 0
    assert cg.eval_logit_parser().parse_args(["--output_scores", "False"]).output_scores is False      # the reference's type=bool would say True


@pytest.mark.parametrize("extra", [["--logit-bias", "1.5"], ["--output_scores", "True"], ["--logit-bias", "-1", "--output_scores", "True"]])
def test_beams_with_bias_or_scores_are_refused(tmp_path, extra):
    from opadpo_amd.cli_generate import main_eval_logit
    answers = tmp_path / "a.jsonl"
    with pytest.raises(SystemExit) as e:
        main_eval_logit(["--synthetic", "tiny", "--temperature", "0", "--num_beams", "3", "--answers-file", str(answers)] + extra)
    assert "beam search" in str(e.value) and not answers.exists()
    with pytest.raises(SystemExit) as e:
        main_eval_logit(["--synthetic", "tiny", "--num_beams", "0", "--answers-file", str(answers)])
    assert "--num_beams" in str(e.value)


def test_generator_refuses_on_the_op_level_engine_and_under_beams():
    from opadpo_amd.generate import Generator
    d = types.SimpleNamespace(ffn=384, hidden=256)
    q = torch.ones(1, 4, dtype=torch.long)
    op = Generator(types.SimpleNamespace(d=d, base=None, dev=torch.device("cpu")), None, use_graph=False)
    for kw in (dict(logit_bias={5: 1.0}), dict(score_ids=[5]), dict(score_ids=[])):
        with pytest.raises(NotImplementedError, match="context engine"):
            op.generate(q, q, None, max_new_tokens=2, **kw)
    cx = Generator(types.SimpleNamespace(d=d, base=None, dev=torch.device("cpu"), ctx=object()), None, use_graph=False)
    with pytest.raises(NotImplementedError, match="context engine"):
        cx.generate(q, q, None, max_new_tokens=2, num_beams=2, logit_bias={5: 1.0})


# ---- label ids and bias entries ---------------------------------------------------------------------------------------------------------
def test_yes_no_label_ids_and_bias_on_the_toy_tokenizer():
    from opadpo_amd.eval_generate import yes_no_label_ids, yes_no_sequence_bias
    tok = ToyTokenizer()
    ids = yes_no_label_ids(tok)
    # ToyTokenizer: id = 3 + sum(ord(c) * (i + 1)) % 20000 per whitespace word; a leading space or newline is not part of the word
    assert list(ids) == ["yes", "no", "Yes", "No", "\nYes", "\nNo"]
    assert ids == {"yes": 671, "no": 335, "Yes": 639, "No": 303, "\nYes": 639, "\nNo": 303}
    for name in ids:
        assert ids[name] == int(tok(" " + name.strip())["input_ids"][0][-1])
    assert yes_no_sequence_bias(tok, 2.0) == {639: -2.0, 303: 2.0}
    assert yes_no_sequence_bias(tok, -0.5) == {639: 0.5, 303: -0.5}
    from opadpo_amd.synth import SyntheticTokenizer
    st = SyntheticTokenizer(512)                      # ignores add_special_tokens and keeps its BOS: the BOS is dropped, one token stays
    assert yes_no_sequence_bias(st, 1.0) == {st("Yes")["input_ids"][-1]: -1.0, st("No")["input_ids"][-1]: 1.0}
    assert yes_no_label_ids(st)["Yes"] == st("Yes")["input_ids"][-1]


def test_multi_token_bias_entry_is_refused():
    from opadpo_amd.eval_generate import yes_no_sequence_bias

    class CharTokenizer(ToyTokenizer):               # every character its own token: 'Yes' takes three
        def _encode(self, text):
            return [self.bos_token_id] + [3 + ord(c) for w in text.split() for c in w]

    with pytest.raises(ValueError) as e:
        yes_no_sequence_bias(CharTokenizer(), 1.0)
    assert "'Yes'" in str(e.value) and str([3 + ord(c) for c in "Yes"]) in str(e.value)

    class PieceTokenizer(ToyTokenizer):              # sentencepiece-like: the leading space is a bare piece of its own in front of the word piece
        def _encode(self, text):
            return [self.bos_token_id] + ([29871] if text.startswith(" ") else []) + super()._encode(text)[1:]

        def convert_ids_to_tokens(self, i):
            return "▁" if i == 29871 else f"▁w{i}"

    assert yes_no_sequence_bias(PieceTokenizer(), 1.0) == {639: -1.0, 303: 1.0}


# ---- the restatement against hand-worked cases ---------------------------------------------------------------------------------------------
def test_ref_bias_flips_the_argmax_and_zero_is_identity():
    z = np.array([[1.0, 3.0, 2.0, -1.0]], dtype=np.float32)
    assert np.array_equal(logit_ref.processed_scores(z, None, 0), z)
    assert np.array_equal(logit_ref.processed_scores(z, {}, 0), z)
    assert np.array_equal(logit_ref.processed_scores(z, {1: 0.0, 3: 0.0}, 0), z)
    got = logit_ref.processed_scores(z, {1: -1.5, 3: 0.25}, 0)
    assert got.tolist() == [[1.0, 1.5, 2.0, -0.75]] and int(got.argmax()) == 2 and int(z.argmax()) == 1
    # temperature: a plain fp32 divide after the add; bias 0 is the identity there too
    t = logit_ref.processed_scores(z, {1: -1.5}, 0.5)
    assert t.dtype == np.float32 and t.tolist() == [[2.0, 3.0, 4.0, -2.0]]
    assert np.array_equal(logit_ref.processed_scores(z, {2: 0.0}, 0.2), z / np.float32(0.2))
    assert np.array_equal(logit_ref.processed_scores(z[0], None, 1.0), z)          # a single row comes back as [1, V]


def test_ref_top_k_and_top_p_cuts_read_minus_inf():
    # probabilities 0.5, 0.25, 0.125, 0.0625, 0.0625 (logits = their logs): ascending cumulative mass 0.0625, 0.125, 0.25, 0.5, 1
    p = np.array([0.125, 0.5, 0.0625, 0.25, 0.0625])
    z = np.log(p).astype(np.float32)[None]
    s = logit_ref.processed_scores(z, None, 1.0, 0, 0.8)                         # cut cumulative <= 0.2: the two 0.0625 tokens
    assert s[0].tolist() == [z[0, 0], z[0, 1], -INF, z[0, 3], -INF]
    assert abs(logit_ref.top_p_margin(z, None, 1.0, 0, 0.8) - 0.05) < 1e-6       # 0.25 against the cut at 0.2
    s = logit_ref.processed_scores(z, None, 1.0, 0, 0.7)                         # cut cumulative <= 0.3: 0.0625, 0.0625, 0.125
    assert s[0].tolist() == [-INF, z[0, 1], -INF, z[0, 3], -INF]
    s = logit_ref.processed_scores(z, None, 1.0, 2, 1.0)                         # top-2
    assert s[0].tolist() == [-INF, z[0, 1], -INF, z[0, 3], -INF]
    s = logit_ref.processed_scores(z, None, 1.0, 3, 0.8)                         # top-3 renormalises: 4/7, 2/7, 1/7 -> 1/7 <= 0.2 is cut as well
    assert s[0].tolist() == [-INF, z[0, 1], -INF, z[0, 3], -INF]
    s = logit_ref.processed_scores(z, None, 1.0, 0, 1e-6)                        # the largest token always stays
    assert s[0].tolist() == [-INF, z[0, 1], -INF, -INF, -INF]
    assert np.array_equal(logit_ref.processed_scores(z, None, 1.0, 0, 1.0), z) and np.array_equal(logit_ref.processed_scores(z, None, 1.0, 9, 1.0), z)
    assert logit_ref.top_p_margin(z, None, 1.0, 0, 1.0) == INF and logit_ref.top_p_margin(z, None, 0, 0, 0.5) == INF
    # the bias acts BEFORE the cut: +3 on token 2 lifts it over the top-p cut, and the values that stay are (logit + bias) / temperature
    s = logit_ref.processed_scores(z, {2: 3.0}, 0.5, 0, 0.8)
    assert s[0, 2] == (z[0, 2] + np.float32(3.0)) / np.float32(0.5) and s[0, 1] == -INF and s[0, 4] == -INF      # the old argmax now falls under the cut
    # greedy: nothing is cut whatever the filters say
    assert np.array_equal(logit_ref.processed_scores(z, {2: 3.0}, 0, 2, 0.1), z + np.array([0, 0, 3, 0, 0], dtype=np.float32))


# ---- answers file of the score mode -----------------------------------------------------------------------------------------------------
class _StubEngine:
    """Stands in for ctx.CtxEngine: the 'scores' of a row are a function of its own prompt only, so the trailer must not depend on batching."""

    def __init__(self):
        self.d = types.SimpleNamespace(ffn=384, hidden=256)
        self.base, self.dev, self.ctx = None, torch.device("cpu"), object()
        self.calls = []

    def encode_images(self, images):
        return torch.zeros(images.shape[0], 1, 1)

    def generate(self, adapter, queries, masks, feats, *, max_new_tokens, logit_bias=None, score_ids=None, **kw):
        self.calls.append(dict(kw, B=queries.shape[0], max_new_tokens=max_new_tokens, logit_bias=logit_bias, score_ids=score_ids))
        tokens = torch.full((queries.shape[0], max_new_tokens), 7, dtype=torch.long)
        if score_ids is None:
            return tokens
        key = (queries * masks).sum(1).float()
        sc = torch.stack([key * 0.5 + j for j in range(len(score_ids))], 1)
        sc[:, -1] = -INF
        return tokens, sc


def _questions(tmp_path, nq):
    from PIL import Image
    for i in range(nq):
        Image.new("RGB", (9, 6), (20 * i, 100, 50)).save(tmp_path / f"x{i}.png")
    return [{"question_id": i, "image": f"x{i}.png", "text": " ".join(["what"] * (i + 1)) + f" item{i} ?"} for i in range(nq)]


def test_score_trailer_format_and_question_order(tmp_path):
    from opadpo_amd.eval_generate import answer_questions, yes_no_label_ids, yes_no_sequence_bias
    from opadpo_amd.synth import SyntheticTokenizer
    tok = SyntheticTokenizer(512)
    nq = 5
    qs = _questions(tmp_path, nq)
    labels, bias = yes_no_label_ids(tok), yes_no_sequence_bias(tok, 2.0)
    texts = {}
    for bs in (1, 2, 5):
        eng = _StubEngine()
        f = tmp_path / f"s{bs}.jsonl"
        n = answer_questions(eng, tok, qs, str(tmp_path), str(f), temperature=0.2, top_p=0.9, image_size=28, batch_size=bs, logit_bias=bias,
                             score_labels=labels)
        assert n == nq and [c["B"] for c in eng.calls] == [bs] * (nq // bs) + ([nq % bs] if nq % bs else [])
        for c in eng.calls:
            assert c["logit_bias"] == bias and c["score_ids"] == list(labels.values()) and c["temperature"] == pytest.approx(0.2)
            assert c["max_new_tokens"] == 1 and c["top_p"] == pytest.approx(0.9)
        texts[bs] = f.read_text()
    text = texts[1]
    assert text == texts[2] == texts[5], "the score lists depend on --batch-size"
    assert text.count("\n") == 0 and "question_id" not in text and "-Infinity" in text          # one line, no answer lines, json's spelling of -inf
    got = json.loads(text)
    assert list(got) == ["yes", "no", "Yes", "No", "\nYes", "\nNo"] and all(len(v) == nq for v in got.values())
    assert got["\nNo"] == [-INF] * nq
    assert len(set(got["yes"])) == nq and [v + 1 for v in got["yes"]] == got["no"]              # one entry per question, in question order
    # greedy (temperature 0) reaches the engine as temperature 0, and a bias without scores still writes ordinary answer lines
    eng = _StubEngine()
    answer_questions(eng, tok, qs, str(tmp_path), str(tmp_path / "g.jsonl"), temperature=0.0, image_size=28, score_labels=labels)
    assert eng.calls[0]["temperature"] == 0.0 and eng.calls[0]["logit_bias"] is None
    eng = _StubEngine()
    assert answer_questions(eng, tok, qs, str(tmp_path), str(tmp_path / "b.jsonl"), temperature=0.2, image_size=28, max_new_tokens=4, logit_bias=bias) == nq
    lines = (tmp_path / "b.jsonl").read_text().splitlines()
    assert len(lines) == nq and [json.loads(x)["question_id"] for x in lines] == list(range(nq)) and eng.calls[0]["score_ids"] is None
    assert eng.calls[0]["max_new_tokens"] == 4
    # neither keyword: the engine is called exactly as before (no new keyword reaches it)
    eng = _StubEngine()
    answer_questions(eng, tok, qs[:1], str(tmp_path), str(tmp_path / "p.jsonl"), temperature=0.2, image_size=28, max_new_tokens=4)
    assert eng.calls[0]["logit_bias"] is None and eng.calls[0]["score_ids"] is None and eng.calls[0]["temperature"] == pytest.approx(0.2)
