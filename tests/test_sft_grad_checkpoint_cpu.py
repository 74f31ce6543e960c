"""CPU: the surface of gradient checkpointing in the OPA LoRA-SFT stage (run/train_opa.sh ... --gradient_checkpointing True) - the command-line
flag, the `--cfg` YAML key and the trainer's keyword.  What it computes is tests/test_sft_grad_checkpoint_gpu.py's."""
import inspect


def test_flag_is_declared_and_off_by_default():
    from opadpo_amd import cli_sft
    assert ("gradient_checkpointing", "sbool", "False") in cli_sft.FLAGS
    p = cli_sft.make_parser()
    assert p.parse_args([]).gradient_checkpointing == "False"
    assert p.parse_args(["--gradient_checkpointing", "True"]).gradient_checkpointing == "True"
    assert p.parse_args(["--gradient_checkpointing", "False"]).gradient_checkpointing == "False"
    assert cli_sft.parse_args(["--cfg", "none"]).gradient_checkpointing is False
    assert cli_sft.parse_args(["--cfg", "none", "--gradient_checkpointing", "True"]).gradient_checkpointing is True
    assert cli_sft.parse_args(["--cfg", "none", "--gradient_checkpointing", "False"]).gradient_checkpointing is False


def test_yaml_key_sets_it_and_the_command_line_wins(tmp_path):
    from opadpo_amd import cli_sft
    y = tmp_path / "opa.yaml"
    y.write_text("learning_rate: 1.0e-5\ngradient_checkpointing: True\n")
    a = cli_sft.parse_args(["--cfg", str(y)])
    assert a.gradient_checkpointing is True and a.learning_rate == 1.0e-5
    assert cli_sft.parse_args(["--cfg", str(y), "--gradient_checkpointing", "False"]).gradient_checkpointing is False
    assert cli_sft.parse_args(["--cfg", str(y), "--gradient_checkpointing=False"]).gradient_checkpointing is False
    nested = tmp_path / "ref.yaml"                            # the reference's training base YAML nests its keys
    nested.write_text("training:\n  gradient_checkpointing: True\n")
    assert cli_sft.parse_args(["--cfg", str(nested)]).gradient_checkpointing is True
    off = tmp_path / "off.yaml"
    off.write_text("gradient_checkpointing: False\n")
    assert cli_sft.parse_args(["--cfg", str(off)]).gradient_checkpointing is False
    assert cli_sft.parse_args(["--cfg", str(off), "--gradient_checkpointing", "True"]).gradient_checkpointing is True
    assert cli_sft.parse_args(["--cfg", str(tmp_path / "missing.yaml")]).gradient_checkpointing is False


def test_trainer_and_vision_path_take_the_keyword():
    from opadpo_amd.sft import SFTTrainer
    from opadpo_amd.vision_train import VisionTrainPath
    p = inspect.signature(SFTTrainer.__init__).parameters["gradient_checkpointing"]
    assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
    p = inspect.signature(VisionTrainPath.forward).parameters["checkpoint"]
    assert p.default is False


def test_op_level_engine_refuses_at_construction():
    """The op-level LlavaEngine keeps every layer resident: a trainer asked to checkpoint over it refuses before anything else is built."""
    import pytest
    from opadpo_amd.model import LlavaEngine
    from opadpo_amd.sft import SFTTrainer

    class _Adapter:
        trainable = True
    eng = LlavaEngine.__new__(LlavaEngine)
    with pytest.raises(NotImplementedError):
        SFTTrainer(eng, _Adapter(), None, response_len=16, gradient_checkpointing=True)
