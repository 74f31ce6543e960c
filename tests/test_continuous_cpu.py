"""CPU: continuous batching for the rollout - the schedule as host arithmetic (generate.plan_continuous) on hand-worked cases, the CLI flag and the
refusals that need no GPU, and the host-side validation of the new entry points reached through the built library."""
import ctypes
import os
import types

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built_lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location("opadpo_build", os.path.join(REPO, "opa-dpo_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.build(verbose=False)


def test_plan_continuous_hand_worked():
    from opadpo_amd.generate import plan_continuous
    # fewer prompts than slots: both start at step 0 in slots 0 and 1; lengths 3 and 10 are finished after 2 and 9 steps, the session ends at the
    # first check point at or after 9 with a check every 4 steps
    assert plan_continuous([3, 10], 4, 4) == ([(0, 0), (1, 0)], 12)
    # one slot; caps on and off check boundaries: length 5 is finished after exactly 4 steps and leaves at check 4; length 6 admitted at 4 is
    # finished after 9 and leaves at 12; length 1 admitted at 12 is finished at once and leaves at the next check
    assert plan_continuous([5, 6, 1], 1, 4) == ([(0, 0), (0, 4), (0, 12)], 16)
    # all equal: two waves of two
    assert plan_continuous([9, 9, 9, 9], 2, 4) == ([(0, 0), (1, 0), (0, 8), (1, 8)], 16)
    # one long among many short: slot 1 turns over at every check while slot 0 holds the long one; 24 steps against 23 + 1 + 1 of static pairs
    assert plan_continuous([24, 2, 2, 2, 2, 2], 2, 4) == ([(0, 0), (1, 0), (1, 4), (1, 8), (1, 12), (1, 16)], 24)
    # the default cadence is 32; nothing to do: no step
    assert plan_continuous([33, 1], 2) == ([(0, 0), (1, 0)], 32)
    assert plan_continuous([], 3, 4) == ([], 0)
    for bad in (lambda: plan_continuous([1], 0, 4), lambda: plan_continuous([1], 1, 0), lambda: plan_continuous([0], 1, 4)):
        with pytest.raises(ValueError):
            bad()


def test_plan_continuous_against_a_step_by_step_simulation():
    """every slot stepped one token at a time, polled every check_every steps: the loop of CtxEngine.generate_continuous restated"""
    import random
    from opadpo_amd.generate import plan_continuous
    rng = random.Random(5)
    for _ in range(50):
        n, slots, every = rng.randint(1, 12), rng.randint(1, 5), rng.randint(1, 6)
        lengths = [rng.randint(1, 20) for _ in range(n)]
        sched, occ, left, nxt, steps = [None] * n, [None] * slots, [0] * slots, 0, 0
        while True:
            for s in range(slots):
                if occ[s] is None and nxt < n:
                    occ[s], left[s], sched[nxt] = nxt, lengths[nxt] - 1, (s, steps)      # token 0 comes with the admission
                    nxt += 1
            if all(o is None for o in occ):
                break
            for _ in range(every):
                steps += 1
                left = [max(0, v - 1) for v in left]
            for s in range(slots):
                if occ[s] is not None and left[s] == 0:
                    occ[s] = None
        assert plan_continuous(lengths, slots, every) == (sched, steps)


def test_cli_flag_and_refusals_without_gpu(tmp_path):
    from opadpo_amd import cli_generate as cg
    from opadpo_amd.generate import Generator
    ns, _ = cg.rollout_parser().parse_known_args([])
    assert ns.continuous_batching is False
    ns, _ = cg.rollout_parser().parse_known_args(["--continuous_batching", "True", "--num_return_sequences", "2", "--output_dir", str(tmp_path)])
    assert ns.continuous_batching is True
    with pytest.raises(SystemExit, match="continuous_batching"):
        cg.run_rollout(ns, log=lambda *_: None)
    assert "--continuous_batching $CONTINUOUS_BATCHING" in open(os.path.join(REPO, "run", "online_generate.sh")).read()
    # the Python surface: refused before anything touches a device
    op_level = types.SimpleNamespace(d=types.SimpleNamespace(ffn=100), base=None, dev="cpu")
    with pytest.raises(NotImplementedError, match="CtxEngine"):
        Generator(op_level, None, use_graph=False).generate_continuous(None, None, None, slots=2, max_new_tokens=4)
    ctx_like = types.SimpleNamespace(d=types.SimpleNamespace(ffn=100), base=None, dev="cpu", ctx=1)
    gen = Generator(ctx_like, None, use_graph=False)
    with pytest.raises(NotImplementedError, match="num_return_sequences"):
        gen.generate_continuous(None, None, None, slots=2, max_new_tokens=4, num_return_sequences=2)
    with pytest.raises(NotImplementedError, match="num_beams"):
        gen.generate_continuous(None, None, None, slots=2, max_new_tokens=4, num_beams=2)
    with pytest.raises(NotImplementedError, match="logit_bias"):
        gen.generate_continuous(None, None, None, slots=2, max_new_tokens=4, logit_bias={3: 1.0})
    with pytest.raises(NotImplementedError, match="score_ids"):
        gen.generate_continuous(None, None, None, slots=2, max_new_tokens=4, score_ids=[1])


def test_new_entry_points_validate_on_the_host(built_lib):
    """every refusal below is made before the first HIP call: text, a non-zero status, no abort"""
    from opadpo_amd import lib as L
    from opadpo_amd.ctx import Dims
    lib = L.load()
    for name in ("opadpo_attn_decode_fused_rows", "opadpo_sample_rows", "opadpo_decode_cont_begin", "opadpo_decode_cont_admit", "opadpo_decode_cont_poll",
                 "opadpo_decode_cont_retire"):
        assert name in L.SIGNATURES and hasattr(lib, name)
    assert lib.opadpo_abi_version() == 2
    h = ctypes.c_void_p()
    assert lib.opadpo_ctx_create(ctypes.byref(Dims(256, 2, 2, 128, 384, 512, 1e-5, 10000.0, 128, 2, 2, 256, 56, 14, 1e-5, 128, 256.0)), 0, ctypes.byref(h)) == 0
    err = lambda: lib.opadpo_ctx_last_error(h)
    for slots in (0, 257, -1):
        assert lib.opadpo_decode_cont_begin(h, 0, slots, 8, 4, 1.0, 0, 1.0, 2, 0, 0, None) != 0 and b"1..256" in err()
    assert lib.opadpo_decode_cont_begin(h, 0, 4, 8, 4, 1.0, 0, 1.0, 2, 0, 0, None) != 0 and b"weights not set" in err()
    one, fin = (ctypes.c_int32 * 1)(0), (ctypes.c_uint8 * 4)()
    assert lib.opadpo_decode_cont_admit(h, 1, one, None, None, None, None, one, None) != 0 and b"no active continuous session" in err()
    assert lib.opadpo_decode_cont_poll(h, fin, None) != 0 and b"no active continuous session" in err()
    assert lib.opadpo_decode_cont_retire(h, 0, None, None, None, None) != 0 and b"no active continuous session" in err()
    # armed logit processors: refused by name, and the refusal disarms (the next refusal is about the weights again)
    ids, bias = (ctypes.c_int32 * 1)(3), (ctypes.c_float * 1)(1.0)
    assert lib.opadpo_ctx_set_logit_processors(h, ids, bias, 1, None, 0, None, 0) == 0
    assert lib.opadpo_decode_cont_begin(h, 0, 4, 8, 4, 1.0, 0, 1.0, 2, 0, 0, None) != 0 and b"opadpo_ctx_set_logit_processors" in err()
    assert lib.opadpo_decode_cont_begin(h, 0, 4, 8, 4, 1.0, 0, 1.0, 2, 0, 0, None) != 0 and b"weights not set" in err()
    lib.opadpo_ctx_destroy(h)
    # the op-level forms
    lib.opadpo_last_error.restype = ctypes.c_char_p
    p = ctypes.c_void_p(256)                      # never dereferenced: both calls are refused on their arguments
    assert lib.opadpo_attn_decode_fused_rows(p, 768, p, p, p, p, p, None, 2, 2, 128, None, 64, 0.1, None, 0, None) != 0
    assert b"opadpo_attn_decode_fused_rows" in lib.opadpo_last_error() and b"pos_rows" in lib.opadpo_last_error()
    assert lib.opadpo_attn_decode_fused_rows(p, 768, p, p, p, p, p, None, 2, 2, 96, p, 64, 0.1, None, 0, None) != 0 and b"64 or 128" in lib.opadpo_last_error()
    assert lib.opadpo_attn_decode_fused_rows(p, 100, p, p, p, p, p, None, 2, 2, 128, p, 64, 0.1, None, 0, None) != 0 and b"leading dimension" in lib.opadpo_last_error()
    assert lib.opadpo_sample_rows(p, 512, 2, 512, 0.0, 0, 1.0, p, p, p, 4, p, 0, 2, p, None, None) != 0 and b"temperature" in lib.opadpo_last_error()
    assert lib.opadpo_sample_rows(p, 512, 2, 512, 1.0, 0, 1.0, p, None, p, 4, p, 0, 2, p, None, None) != 0 and b"null operand" in lib.opadpo_last_error()
    assert lib.opadpo_sample_rows(p, 512, 2, 512, 1.0, 0, 1.0, p, p, p, 0, p, 0, 2, p, None, None) != 0 and b"max_steps" in lib.opadpo_last_error()
