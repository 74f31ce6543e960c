"""CPU: the beam-search restatement (tests/beam_ref.py) against the installed transformers, and the host-side refusals of the beam
entry points (no GPU needed)."""
import ctypes
import os

import pytest
import torch

import beam_ref

EOS, PAD, V = 2, 0, 64


def _tiny_llama(seed: int, eos_bias: float):
    transformers = pytest.importorskip("transformers")
    cfg = transformers.LlamaConfig(vocab_size=V, hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=4,
                                   num_key_value_heads=4, max_position_embeddings=64, bos_token_id=1, eos_token_id=EOS, pad_token_id=PAD)
    torch.manual_seed(seed)
    model = transformers.LlamaForCausalLM(cfg).eval()
    with torch.no_grad():
        model.lm_head.weight.mul_(40.0)                 # peaked distributions: scores far apart
        model.lm_head.weight[EOS] += eos_bias * model.model.norm.weight / model.model.norm.weight.norm()
    return model


@pytest.mark.parametrize("k", [2, 3, 5])
def test_beam_ref_matches_transformers(k):
    """beam_ref.beam_search == model.generate(num_beams=k, do_sample=False): same tokens, sequences_scores within 1e-5; the cases
    'EOS inside the window', 'no EOS' and 'early stop before max_new_tokens' all occur."""
    max_new, B = 12, 2
    seen = {"eos": 0, "no_eos": 0, "early_stop": 0}
    for seed, bias in ((0, -50.0), (1, 0.0), (2, 3.0), (3, 6.0), (4, 12.0), (5, 25.0), (6, 60.0), (7, 120.0)):
        model = _tiny_llama(seed, bias)
        g = torch.Generator().manual_seed(100 + seed)
        prompt = torch.randint(3, V, (B, 5), generator=g)
        with torch.no_grad():
            out = model.generate(prompt, attention_mask=torch.ones_like(prompt), num_beams=k, do_sample=False, max_new_tokens=max_new,
                                 eos_token_id=EOS, pad_token_id=PAD, length_penalty=1.0, early_stopping=False, num_return_sequences=1,
                                 return_dict_in_generate=True, output_scores=True)

            def step_logits(gen):
                rows = prompt.repeat_interleave(k, 0)
                ids = torch.cat([rows, gen], 1)
                return model(ids).logits[:, -1].float()

            tokens, scores, st = beam_ref.beam_search(step_logits, B, k, V, max_new, EOS, PAD)
        hf = out.sequences[:, prompt.shape[1]:]
        want = torch.full((B, max_new), PAD, dtype=torch.int64)
        want[:, :hf.shape[1]] = hf
        for b in range(B):                      # HF fills after EOS with pad already; keep EOS, pad after
            row = want[b].tolist()
            if EOS in row:
                want[b, row.index(EOS) + 1:] = PAD
        assert torch.equal(tokens, want), (seed, bias, tokens, want)
        assert torch.allclose(scores, out.sequences_scores.float(), atol=1e-5, rtol=0), (scores, out.sequences_scores)
        for b in range(B):
            seen["eos" if EOS in tokens[b].tolist() else "no_eos"] += 1
        seen["early_stop"] += int(st.t < max_new)
    assert all(v > 0 for v in seen.values()), seen


@pytest.fixture(scope="module")
def built_lib():
    import importlib.util
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("opadpo_build", os.path.join(repo, "opa-dpo_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.build(verbose=False)


def test_beam_begin_refusals_need_no_gpu(built_lib):
    """opadpo_decode_beam_begin fails with text for k = 0, k above the bound, B*k > 64 and a context without weights (no launch)."""
    from opadpo_amd import lib as L
    from opadpo_amd.ctx import Dims
    lib = L.load()
    good = Dims(256, 2, 2, 128, 384, 512, 1e-5, 10000.0, 128, 2, 2, 256, 56, 14, 1e-5, 128, 256.0)
    h = ctypes.c_void_p()
    assert lib.opadpo_ctx_create(ctypes.byref(good), 0, ctypes.byref(h)) == 0 and h.value
    try:
        for k, B, msg in ((0, 1, b"num_beams"), (17, 1, b"num_beams"), (8, 9, b"64 rows"), (4, 2, b"weights not set")):
            rc = lib.opadpo_decode_beam_begin(h, 0, None, None, None, B, 8, k, 16, EOS, PAD, None)
            assert rc != 0 and msg in lib.opadpo_ctx_last_error(h), (k, B, lib.opadpo_ctx_last_error(h))
        assert lib.opadpo_decode_beam_result(h, None, None, None) != 0 and b"no active beam decode" in lib.opadpo_ctx_last_error(h)
    finally:
        lib.opadpo_ctx_destroy(h)


def test_eval_refuses_beam_sampling(tmp_path):
    """--temperature > 0 with --num_beams > 1 (beam sampling) exits with a message before any model is built."""
    from opadpo_amd.cli_generate import main_eval
    answers = tmp_path / "answers.jsonl"
    with pytest.raises(SystemExit) as e:
        main_eval(["--synthetic", "tiny", "--temperature", "0.2", "--num_beams", "3", "--answers_file", str(answers),
                   "--question_file", str(tmp_path / "q.jsonl"), "--image_folder", str(tmp_path)])
    assert "beam sampling" in str(e.value)
    assert not answers.exists()
