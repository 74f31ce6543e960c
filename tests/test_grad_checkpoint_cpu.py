"""CPU: the surface of gradient checkpointing (--gradient_checkpointing) - the command-line flag, the reference-style YAML, the C entry point's
declaration, export and null-context refusal, and the engines' switch.  What it computes is tests/test_grad_checkpoint_gpu.py's."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "opadpo_hip.h")


def test_parser_accepts_the_flag_and_defaults_to_off():
    from opadpo_amd import cli
    assert ("gradient_checkpointing", "sbool", "False") in cli.FLAGS
    assert cli.build_args(cli.make_parser().parse_args([]), world_size=1).gradient_checkpointing is False
    assert cli.build_args(cli.make_parser().parse_args(["--gradient_checkpointing", "True"]), world_size=1).gradient_checkpointing is True
    assert cli.build_args(cli.make_parser().parse_args(["--gradient_checkpointing", "False"]), world_size=1).gradient_checkpointing is False


def test_yaml_fills_the_flag_and_the_command_line_wins(tmp_path):
    from opadpo_amd import cli
    y = tmp_path / "ref.yaml"        # the reference nests the key under its training section
    y.write_text("model:\n  lora_rank: 64\ntraining:\n  gradient_checkpointing: True\n  learning_rate: 1.0e-5\n")

    def parse(argv):
        ns = cli.make_parser().parse_args(argv)
        cli.load_yaml_defaults(ns, argv)
        return cli.build_args(ns, world_size=1)
    a = parse(["--cfg", str(y)])
    assert a.gradient_checkpointing is True and a.lora_rank == 64
    assert parse(["--cfg", str(y), "--gradient_checkpointing", "False"]).gradient_checkpointing is False
    assert parse(["--cfg", str(y), "--gradient_checkpointing=False"]).gradient_checkpointing is False
    flat = tmp_path / "flat.yaml"
    flat.write_text("gradient_checkpointing: False\n")
    assert parse(["--cfg", str(flat)]).gradient_checkpointing is False
    assert parse(["--cfg", str(flat), "--gradient_checkpointing", "True"]).gradient_checkpointing is True
    assert parse(["--cfg", str(tmp_path / "missing.yaml")]).gradient_checkpointing is False


def test_shipped_configs_and_launchers_are_untouched_by_the_default():
    """The shipped YAML does not carry the key, so a plain launch stays resident."""
    from opadpo_amd import cli
    cfg = os.path.join(REPO, "configs", "llava", "llava_dpo.yaml")
    ns = cli.make_parser().parse_args(["--cfg", cfg])
    cli.load_yaml_defaults(ns, ["--cfg", cfg])
    assert cli.build_args(ns, world_size=1).gradient_checkpointing is False


def test_header_declares_and_library_exports_the_entry_point():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"int\s+opadpo_ctx_set_grad_checkpoint\s*\(\s*opadpo_ctx\s*\*\s*ctx\s*,\s*int\s+on\s*\)\s*;", src)
    from opadpo_amd import lib as L
    assert L.SIGNATURES["opadpo_ctx_set_grad_checkpoint"] == [ctypes.c_void_p, ctypes.c_int]
    lib = L.load()
    assert hasattr(lib, "opadpo_ctx_set_grad_checkpoint")


def test_null_context_is_refused_and_a_live_one_accepts():
    from opadpo_amd import lib as L
    from opadpo_amd.ctx import Dims
    lib = L.load()
    assert lib.opadpo_ctx_set_grad_checkpoint(None, 1) != 0
    h = ctypes.c_void_p()
    good = Dims(256, 2, 2, 128, 384, 512, 1e-5, 10000.0, 128, 2, 2, 256, 56, 14, 1e-5, 128, 256.0)
    assert lib.opadpo_ctx_create(ctypes.byref(good), 0, ctypes.byref(h)) == 0 and h.value
    assert lib.opadpo_ctx_set_grad_checkpoint(h, 1) == 0 and lib.opadpo_ctx_set_grad_checkpoint(h, 0) == 0
    assert lib.opadpo_ctx_trim(h) == 0 and lib.opadpo_ctx_bytes_peak(h) == 0
    lib.opadpo_ctx_destroy(h)


def test_engines_and_policy_carry_the_switch():
    from opadpo_amd.ctx import CtxEngine
    from opadpo_amd.model import LlavaEngine
    from opadpo_amd.policy import AutoregressivePolicy
    assert callable(CtxEngine.set_grad_checkpoint)
    op = LlavaEngine.__new__(LlavaEngine)                     # the op-level engine keeps activations resident: off is its only mode
    op.set_grad_checkpoint(False)
    with pytest.raises(NotImplementedError):
        op.set_grad_checkpoint(True)
    calls = []

    class _Eng:
        def set_grad_checkpoint(self, on):
            calls.append(on)
    pol = AutoregressivePolicy.__new__(AutoregressivePolicy)
    pol.engine, pol.gradient_checkpointing = _Eng(), False
    pol.set_gradient_checkpointing(1)
    assert pol.gradient_checkpointing is True and calls == [True]
    pol.engine = op
    with pytest.raises(NotImplementedError):
        pol.set_gradient_checkpointing(True)
