"""CPU: the LoRA dropout contract that the kernels, the context path and the trainers hold - the Philox restatement against the published
known answers, deterministic mask statistics, the command-line surface, and the oracle wrapper at rate 0."""
import math

import numpy as np
import pytest
import torch

import dropout_ref as DR


def _hex(words):
    return [f"{int(w):08x}" for w in words]


def test_philox_known_answers():
    # Random123 kat_vectors, philox4x32 10 rounds
    assert _hex(DR.philox4x32_10((0, 0, 0, 0), (0, 0))) == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    f = 0xFFFFFFFF
    assert _hex(DR.philox4x32_10((f, f, f, f), (f, f))) == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]
    assert _hex(DR.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) == \
        ["d16cfe09", "94fdcceb", "5001e420", "24126ea1"]


def test_counter_packing():
    """keep_mask is the documented packing: word (col & 3) of the call with counter (col >> 2, row, call lo, call hi), key (seed, layer * 8 + module)."""
    seed, call, layer, module, p = 1234, (5 << 32) | 77, 3, 6, 0.25
    rows = [0, 9, 100000]
    m = DR.keep_mask(seed, call, layer, module, rows, 16, p)
    thr = DR.threshold(p)
    assert thr == 1 << 30
    for ri, row in enumerate(rows):
        for col in (0, 3, 4, 15):
            w = DR.philox4x32_10((col >> 2, row, 77, 5), (seed, layer * 8 + module))[col & 3]
            assert bool(m[ri, col]) == (int(w) >= thr)
    assert DR.keep_mask(seed, call, layer, module, rows, 16, 0.0).all()


@pytest.mark.parametrize("p", [0.05, 0.1, 0.5])
def test_mask_statistics(p):
    rows, K = np.arange(512), 1024
    n = rows.size * K
    base = DR.keep_mask(11, 3, 2, 1, rows, K, p)
    sigma = math.sqrt(n * p * (1 - p))
    assert abs(int(base.sum()) - n * (1 - p)) < 5 * sigma, (int(base.sum()), n * (1 - p), sigma)
    q = (1 - p) ** 2 + p ** 2                     # two independent masks agree with this probability
    sq = math.sqrt(n * q * (1 - q))
    for what, other in (("module", DR.keep_mask(11, 3, 2, 2, rows, K, p)), ("layer", DR.keep_mask(11, 3, 3, 1, rows, K, p)),
                        ("call", DR.keep_mask(11, 4, 2, 1, rows, K, p)), ("seed", DR.keep_mask(12, 3, 2, 1, rows, K, p))):
        agree = int((base == other).sum())
        assert abs(agree - n * q) < 5 * sq, (what, agree, n * q, sq)
    assert np.array_equal(base, DR.keep_mask(11, 3, 2, 1, rows, K, p))


def test_fwd_ref_values():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(5, 16, generator=g).to(torch.bfloat16)
    out = DR.dropout_fwd_ref(x, 7, 1, 0, 4, 2, np.arange(5), 0.1)
    assert out.shape == (5, 32)
    sc = (x.float() * torch.tensor(np.float32(1.0 / 0.9))).to(torch.bfloat16)
    for j in range(2):
        o = out[:, j * 16:(j + 1) * 16]
        assert bool(((o == sc) | (o == 0)).all())
    assert torch.equal(DR.dropout_fwd_ref(x, 7, 1, 0, 4, 2, np.arange(5), 0.0), torch.cat([x, x], 1))


def test_cli_keeps_and_checks_lora_drop(capsys):
    from opadpo_amd import cli, cli_sft
    ns = cli.make_parser().parse_args(["--lora_drop", "0.05"])
    assert cli.build_args(ns, world_size=1).lora_drop == 0.05
    for bad in ("1.0", "-0.1", "1.5"):
        with pytest.raises(ValueError):
            cli.build_args(cli.make_parser().parse_args(["--lora_drop", bad]), world_size=1)
        with pytest.raises(SystemExit) as e:
            cli_sft.main(["--lora_drop", bad, "--cfg", ""])
        assert "lora_drop" in str(e.value)
    assert cli_sft.make_parser().parse_args(["--lora_drop", "0.05"]).lora_drop == 0.05


def test_policy_counts_training_forwards_only():
    """The call counter: nothing at rate 0, (count * world + rank) otherwise - different for every training forward and rank."""
    from opadpo_amd.policy import AutoregressivePolicy
    pol = AutoregressivePolicy.__new__(AutoregressivePolicy)
    pol.lora_dropout, pol.dropout_seed, pol.dropout_calls, pol.dropout_rank, pol.dropout_world = 0.0, 0, 0, 0, 1
    assert pol.next_dropout() == {} and pol.dropout_calls == 0
    pol.set_lora_dropout(0.1, seed=42, rank=1, world=4)
    a, b = pol.next_dropout(), pol.next_dropout()
    assert (a["dropout_call"], b["dropout_call"]) == (1, 5) and a["lora_dropout"] == 0.1 and a["dropout_seed"] == 42
    with pytest.raises(ValueError):
        pol.set_lora_dropout(1.0)


def test_save_adapter_writes_the_rate(tmp_path):
    import json
    from opadpo_amd.dims import LlavaDims
    from opadpo_amd.trainer import save_adapter

    class _Ad:
        def to_peft_state(self):
            return {}
    save_adapter(_Ad(), str(tmp_path), LlavaDims.tiny(), lora_dropout=0.05)
    assert json.load(open(tmp_path / "adapter_config.json"))["lora_dropout"] == 0.05
    save_adapter(_Ad(), str(tmp_path), LlavaDims.tiny())
    assert json.load(open(tmp_path / "adapter_config.json"))["lora_dropout"] == 0.0


def test_oracle_wrapper_at_rate_zero_is_the_oracle():
    from oracle import llava_ref as LR
    od = LR.LlavaDims.tiny()
    W = LR.init_weights(od, seed=0, std=0.05)
    lora = LR.init_lora(od, seed=1, b_std=0.02)
    g = torch.Generator().manual_seed(3)
    B, Q, T = 2, 8, 6
    images = torch.randn(B, 3, od.image_size, od.image_size, generator=g)
    queries = torch.randint(3, od.vocab, (B, Q), generator=g)
    queries[:, 2] = -200
    qmask = torch.ones(B, Q, dtype=torch.bool)
    resp = {"chosen_response": torch.randint(3, od.vocab, (B, T), generator=g), "rejected_response": torch.randint(3, od.vocab, (B, T), generator=g)}
    L = Q + od.n_patches - 1 + T
    for emu in (False, True):
        want = LR.policy_forward(images, queries, qmask, resp, W, lora, od, emulate_bf16=emu)
        rm, _ = DR.row_map_padded(2 * B, L)
        with DR.OracleDropout(0.0, 1, 0, rm, 2 * B, L).patch(LR):
            got = LR.policy_forward(images, queries, qmask, resp, W, lora, od, emulate_bf16=emu)
        with DR.OracleDropout(0.3, 1, 0, rm, 2 * B, L).patch(LR):
            on = LR.policy_forward(images, queries, qmask, resp, W, lora, od, emulate_bf16=emu)
        for k in want:
            assert torch.equal(got[k], want[k]), k
        assert not torch.equal(on["chosen_response_logprobs"], want["chosen_response_logprobs"])
    assert LR._Ctx.__name__ == "_Ctx"
