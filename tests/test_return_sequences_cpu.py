"""CPU: num_return_sequences on the host side - rollout_step's item-major columns, the CLI default, and the argument refusals of
opadpo_decode_begin_n / opadpo_attn_decode_shared that need no GPU (text, never an abort)."""
import ctypes
import io
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "opa-dpo_amd"))
sys.path.insert(0, os.path.dirname(__file__))
from opadpo_amd import rollout_data as rd          # noqa: E402
from toy_tokenizer import ToyTokenizer            # noqa: E402


def _png(color):
    from PIL import Image
    buf = io.BytesIO()
    Image.new("RGB", (6, 4), color).save(buf, format="PNG")
    return buf.getvalue()


def _rows():
    return [{"question": "what is on the mat ?", "chosen": "a cat sits there", "image": {"bytes": _png((255, 0, 0)), "path": "a.png"}},
            {"question": "describe the scene", "chosen": "two dogs", "image": {"bytes": _png((0, 255, 0)), "path": "b.png"}},
            {"question": "last one ?", "chosen": "yes it is the last one indeed", "image": {"bytes": _png((9, 9, 9)), "path": "d.png"}}]


def test_rollout_step_repeats_the_query_columns_item_major():
    from opadpo_amd import online_generate as og
    tok = ToyTokenizer()
    ds = rd.QueryResponseDataset(_rows(), tok, query_len=48, image_size=8, log=lambda *_: None)
    batches = [rd.collate_query_response([ds[0], ds[1]]), rd.collate_query_response([ds[2]])]
    words = ["red", "green", "blue", "cat", "dog", "mat", "sun", "sky", "sea"]

    def sampler(N):
        state = {"k": 0}

        def sample(q, m, img):
            rows = []
            for _ in range(q.shape[0] * N):                 # response i * N + j = sample j of query i
                rows.append(tok._encode(words[state["k"]])[1:] + [tok.eos_token_id])
                state["k"] += 1
            return torch.tensor(rows)
        return sample

    seen = []

    def feedback(urls, queries, responses, standard):
        seen.append((len(urls), len(queries), len(responses), len(standard)))
        return {"Pseudo_response": [r + " (fixed)" for r in responses], "Generated_response": list(responses), "report_json": [""] * len(responses)}

    one = og.rollout_step(batches, tok, sampler(1), feedback)
    assert one == og.rollout_step(batches, tok, sampler(1), feedback, num_return_sequences=1)          # N = 1: today's output
    assert all(len(v) == 3 for v in one.values()) and one["image_id"] == ["a.png", "b.png", "d.png"]
    del seen[:]
    out = og.rollout_step(batches, tok, sampler(3), feedback, num_return_sequences=3)
    assert list(out) == list(one) and all(len(v) == 9 for v in out.values())
    assert seen == [(6, 6, 6, 6), (3, 3, 3, 3)]                                                       # the feedback callable sees B * N entries
    rep = lambda xs: [x for x in xs for _ in range(3)]
    for col in ("query", "image_id", "standard_response", "image_bytes"):
        assert out[col] == rep(one[col]), col
    assert out["original_generate_response"] == words and out["AI_pseudo_response"] == [w + " (fixed)" for w in words]
    with pytest.raises(ValueError, match="return sequences"):
        og.rollout_step(batches, tok, sampler(1), feedback, num_return_sequences=3)                    # the sampler must return B * N rows
    with pytest.raises(ValueError):
        og.rollout_step(batches, tok, sampler(1), feedback, num_return_sequences=0)


def test_cli_default_is_one():
    from opadpo_amd import cli_generate as cg
    ns, _ = cg.rollout_parser().parse_known_args([])
    assert ns.num_return_sequences == 1
    ns, _ = cg.rollout_parser().parse_known_args(["--num_return_sequences", "4"])
    assert ns.num_return_sequences == 4
    ns.rollout_per_device_batch_size, ns.num_return_sequences = 4, 17
    with pytest.raises(SystemExit, match="num_return_sequences"):
        cg.run_rollout(ns)                                   # refused before any engine is built


@pytest.fixture(scope="module")
def lib():
    import importlib.util
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("opadpo_build", os.path.join(repo, "opa-dpo_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build(verbose=False)
    from opadpo_amd import lib as L
    return L.load()


def test_decode_begin_n_refusals_need_no_gpu(lib):
    """n = 0, n = 17 and B * n = 257 on a context without weights: refused with text that names the bound."""
    from opadpo_amd.ctx import Dims
    dims = Dims(256, 2, 2, 128, 384, 512, 1e-5, 10000.0, 128, 2, 2, 256, 56, 14, 1e-5, 128, 256.0)
    h = ctypes.c_void_p()
    assert lib.opadpo_ctx_create(ctypes.byref(dims), 0, ctypes.byref(h)) == 0 and h.value
    err = lambda: lib.opadpo_ctx_last_error(h).decode()
    begin = lambda B, n: lib.opadpo_decode_begin_n(h, 0, None, None, None, B, 12, n, 6, 1.0, 30, 0.95, 1, 2, 0, 0, None, None)
    try:
        for n in (0, 17, -1):
            assert begin(2, n) != 0 and "1..OPADPO_MAX_RETURN_SEQUENCES (16)" in err(), err()
        assert begin(257, 1) != 0 and "256" in err(), err()
        assert begin(129, 2) != 0 and "num_return_sequences above 256" in err(), err()
        assert begin(16, 16) != 0 and "weights not set" in err(), err()          # inside the bounds: the next check speaks
        assert begin(4, 1) != 0 and "weights not set" in err(), err()
        assert lib.opadpo_decode_step(h, None) != 0 and "no active rollout" in err()
    finally:
        lib.opadpo_ctx_destroy(h)


def test_attn_decode_shared_host_rules_need_no_gpu(lib):
    """The workspace covers either form: the per-row form's key ranges (opadpo_attn_decode_workspace_bytes on items * n rows) and the grouped form's
    R + 1 slots per (row, head) with the documented prefix ranges; argument refusals carry text."""
    ws = lib.opadpo_attn_decode_shared_workspace_bytes
    nh, hd = 8, 128

    def ranges(items, Lp):
        R = min(max(1, 256 // (items * nh)), max(1, Lp // 64))
        per = (-(-Lp // R) + 63) // 64 * 64
        return -(-Lp // per)

    for items, n, Lp, max_new in [(1, 2, 40, 16), (2, 5, 300, 24), (3, 16, 703, 64), (2, 8, 1100, 32), (8, 8, 703, 64), (32, 8, 703, 896)]:
        rows = items * n
        grouped = rows * nh * (ranges(items, Lp) + 1) * (hd + 2) * 4
        per_row = lib.opadpo_attn_decode_workspace_bytes(rows, nh, hd, Lp + max_new)
        assert ws(items, n, nh, hd, Lp, max_new) == max(grouped, per_row), (items, n, Lp)
    assert [ranges(2, 300), ranges(3, 703), ranges(2, 1100), ranges(1, 40), ranges(32, 703)] == [3, 6, 9, 1, 1]
    assert ws(4, 4, nh, 64, 300, 16) == lib.opadpo_attn_decode_workspace_bytes(16, nh, 64, 316)      # head_dim 64: the per-row form only
    assert ws(0, 4, nh, hd, 300, 16) == 0
    lib.opadpo_last_error.restype = ctypes.c_char_p
    one = ctypes.c_void_p(64)                                 # non-null placeholders: every refusal below comes before any launch
    call = lambda n, hd_, form, wsb: lib.opadpo_attn_decode_shared(one, 3 * nh * hd_, one, one, one, one, one, one, one, None, 2, n, nh, hd_, one, 100, 8,
                                                                   0.1, one, wsb, form, None)
    assert call(17, hd, 1, 1 << 30) != 0 and b"16" in lib.opadpo_last_error()
    assert call(0, hd, 1, 1 << 30) != 0 and b"16" in lib.opadpo_last_error()
    assert call(3, 64, 2, 1 << 30) != 0 and b"head_dim 128" in lib.opadpo_last_error()
    assert call(3, hd, 3, 1 << 30) != 0 and b"form" in lib.opadpo_last_error()
    assert call(3, hd, 2, ws(2, 3, nh, hd, 100, 8) - 4) != 0 and b"workspace" in lib.opadpo_last_error()
