"""GPU: gradient checkpointing of the OPA LoRA-SFT stage (SFTTrainer(gradient_checkpointing=True), VisionTrainPath.forward(checkpoint=True),
run/train_opa.sh ... --gradient_checkpointing True).

The LLM half is the context's switch (tests/test_grad_checkpoint_gpu.py); the vision half re-runs each CLIP layer and the projector from its saved
input through the layer body the forward ran.  Every kernel of both halves is deterministic at these shapes, so a recomputed activation carries the
bits the forward produced: every comparison between the two modes here is torch.equal (Python == for the loss), never a tolerance.

Why the LoRA wgrads are bit-reproducible here: the LLM's (lora_r = 256, widths multiples of 256) flush through the ordered reduce
(CtxEngine.wgrad_deterministic() == 1, asserted); the 128x128 wgrad kernel that the 128-wide vision tower (and the r = 128 model of `--synthetic
tiny`) takes adds one K-slice per 256 rows with fp32 atomics, and every product here has fewer than 256 rows: one addition per element per launch,
launches in stream order.  The optimizer's clipping norm is an fp32-atomic sum whose last bit moves from run to run whatever the mode
(tests/test_grad_checkpoint_gpu.py); the tests that step the optimizer give it a deterministic sum of squares through FlatAdamW's `sumsq_fn`.

Shapes: LlavaDims.tiny (2 decoder layers, 2 used CLIP layers), B = 2 with unequal response lengths and one left-padded query, Q = 16, T = 16."""
import os
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
TINY = dict(ffn=512, lora_r=256, lora_alpha=512.0)            # lora_r % 256 == 0: the LLM wgrads leave through the ordered flush
B, Q, T = 2, 16, 16
_model_cache = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from opadpo_amd import lib
    lib.load()
    return torch.device("cuda:0")


def _model():
    """Base weights, LoRA tensors (LLM + CLIP + projector) and one batch, built once and never written; every run gets a fresh context and adapters."""
    if not _model_cache:
        from opadpo_amd.dims import LlavaDims
        from opadpo_amd.model import BaseWeights
        from opadpo_amd.synth import init_lora, init_weights
        dev = _dev()
        d = LlavaDims.tiny(**TINY)
        base = BaseWeights(d, init_weights(d, seed=0, std=0.05, device=dev), dev, need_backward=True)
        lora = init_lora(d, seed=1, b_std=0.02, device=dev, with_vision=True)
        g = torch.Generator().manual_seed(5)
        images = torch.randn(B, 3, d.image_size, d.image_size, generator=g).to(BF)
        queries = torch.randint(3, d.vocab, (B, Q), generator=g)
        qmask = torch.ones(B, Q, dtype=torch.bool)
        queries[0, :3] = 0                                    # left padding on one row, the image token at another slot per row
        qmask[0, :3] = False
        queries[0, 5], queries[1, 2] = -200, -200
        resp = torch.randint(3, d.vocab, (B, T), generator=g)
        for b, ln in enumerate((5, 12)):                      # unequal response lengths: ragged rows
            resp[b, ln] = 2
            resp[b, ln + 1:] = 0
        key_mask = torch.rand(B, d.n_patches, generator=g) > 0.3
        assert 0 < int(key_mask.sum()) < key_mask.numel()
        d_feats = torch.randn(B * d.n_patches, d.hidden, generator=g).to(BF)
        _model_cache["m"] = SimpleNamespace(d=d, base=base, lora=lora, dev=dev, images=images, queries=queries, qmask=qmask, resp=resp,
                                            key_mask=key_mask, d_feats=d_feats)
    return _model_cache["m"]


def _det_sumsq(g, out):
    out.add_(g.double().pow(2).sum().float())


def _tensors(node):
    if isinstance(node, torch.Tensor):
        yield node
    elif isinstance(node, dict):
        for v in node.values():
            yield from _tensors(v)
    elif isinstance(node, (list, tuple)):
        for v in node:
            yield from _tensors(v)


# ---- (a) the vision path alone ------------------------------------------------------------------------------------------------------------
def test_vision_path_checkpointed_has_the_bits_of_the_resident_path():
    from opadpo_amd.vision_train import VisionLoraAdapter, VisionTrainPath, projector_lora_blocks, vision_lora_blocks
    m = _model()
    d = m.d
    res = {}
    for on in (False, True):
        vad = VisionLoraAdapter(d, m.lora, m.dev)
        vt = VisionTrainPath(m.base, vad)
        feats, sv = vt.forward(m.images.to(m.dev), checkpoint=on)
        torch.cuda.synchronize()
        res[on] = SimpleNamespace(feats=feats.clone().cpu(), sv_shapes=[(tuple(t.shape), t.dtype) for t in _tensors(sv)],
                                  sv_bytes=sum(t.nbytes for t in _tensors(sv)), layer_keys=[set(s) for s in sv["layers"]], proj_keys=set(sv["proj"]))
        vt.backward(sv, m.d_feats.to(m.dev))
        torch.cuda.synchronize()
        res[on].vad = vad
        res[on].grad = vad.grad.clone().cpu()
    off, on = res[False], res[True]
    assert torch.equal(off.feats, on.feats), "features differ"
    assert bool(torch.isfinite(off.grad).all())
    for j in range(d.v_used_layers + 1):                      # every CLIP layer's q|k|v / out / fc1 / fc2 A and B, then the projector's
        for name, _, _ in (vision_lora_blocks(d) if j < d.v_used_layers else projector_lora_blocks(d)):
            a, b = off.vad.g(j, name).cpu(), on.vad.g(j, name).cpu()
            assert float(a.abs().max()) > 0, f"layer {j} {name}: no gradient reached it"
            assert torch.equal(a, b), f"layer {j} {name}: gradient differs (max abs {float((a - b).abs().max())})"
    assert torch.equal(off.grad, on.grad)
    # what the checkpointed state holds: each layer's input and the projector's input (plus its row index), nothing per layer
    Tv = d.n_patches + 1
    M = B * Tv
    assert all(k == {"x"} for k in on.layer_keys) and len(on.layer_keys) == d.v_used_layers, on.layer_keys
    assert on.proj_keys == {"idx", "tok"}, on.proj_keys
    assert all({"qkv", "lse", "z1", "f1", "n1", "att", "t_qkv"} <= k for k in off.layer_keys)
    per_layer = {((M, 3 * d.v_hidden), BF): "q|k|v", ((B, d.v_heads, Tv), torch.float32): "lse", ((M, d.v_ffn), BF): "fc1 pre-activation / activation",
                 ((M, 3 * d.lora_r), BF): "LoRA t of q|k|v"}
    held = [per_layer[s] for s in on.sv_shapes if s in per_layer]
    assert not held, f"the checkpointed state still holds {held}"
    assert sorted(per_layer[s] for s in set(off.sv_shapes) if s in per_layer) == sorted(per_layer.values())
    print(f"saved bytes: resident {off.sv_bytes}, checkpointed {on.sv_bytes}")
    assert on.sv_bytes < off.sv_bytes


# ---- (b), (c) one micro-batch through SFTTrainer.loss_and_backward ------------------------------------------------------------------------------
def _trainer(m, on, **kw):
    from opadpo_amd.ctx import CtxEngine
    from opadpo_amd.model import LoraAdapter
    from opadpo_amd.sft import SFTTrainer
    from opadpo_amd.vision_train import VisionLoraAdapter
    eng = CtxEngine(m.base)
    llm, vis = LoraAdapter(m.d, m.lora, m.dev, trainable=True), VisionLoraAdapter(m.d, m.lora, m.dev)
    tr = SFTTrainer(eng, llm, vis, response_len=T, gradient_checkpointing=on, **kw)
    assert tr.gradient_checkpointing is on
    return tr


def _micro_batch(m, on, method=None, **kw):
    """One loss_and_backward in one mode on a fresh context -> CPU results."""
    if method is not None:
        kw.update(entropy_loss=True, entropy_mask_method=method, entropy_mask_ratio=0.5, entropy_loss_coef=0.7)
    tr = _trainer(m, on, **kw)
    torch.manual_seed(123)                                    # 'random' draws its pixel mask from the global CPU generator
    loss = tr.loss_and_backward(m.images.to(m.dev), m.queries, m.qmask, m.resp, image_key_mask=m.key_mask if method == "attention" else None)
    torch.cuda.synchronize()
    out = SimpleNamespace(loss=loss, last=dict(tr.last), llm=tr.llm.grad.clone().cpu(), vis=tr.vis.grad.clone().cpu(), det=tr.engine.wgrad_deterministic(),
                          peak=int(tr.engine._lib.opadpo_ctx_bytes_peak(tr.engine.ctx)), calls=tr._policy.dropout_calls)
    tr.engine.close()
    return out


def _same_micro_batch(off, on, what):
    assert off.det == 1 and on.det == 1, f"{what}: wgrad_deterministic {off.det} / {on.det}"
    assert off.loss == on.loss, f"{what}: loss {off.loss!r} vs {on.loss!r}"
    assert off.last == on.last, f"{what}: {off.last} vs {on.last}"
    for k in ("llm", "vis"):
        a, b = getattr(off, k), getattr(on, k)
        assert float(a.abs().max()) > 0 and bool(torch.isfinite(a).all())
        assert torch.equal(a, b), f"{what}: {k} LoRA gradient differs (max abs {float((a - b).abs().max())})"
    assert on.peak < off.peak, f"{what}: the LLM training forwards did not run checkpointed"


@pytest.mark.parametrize("method", [None, "random", "attention"])
def test_loss_and_backward_is_bit_identical(method):
    m = _model()
    off, on = _micro_batch(m, False, method), _micro_batch(m, True, method)
    _same_micro_batch(off, on, f"entropy {method}")
    if method is not None:
        assert off.last["entropy_loss"] != 0.0 and off.last["mask_sft_loss"] != off.last["base_sft_loss"], off.last


def test_lora_dropout_with_two_passes_alive():
    """CE forward, entropy forward, then both backwards: each recompute must regenerate the masks of ITS forward's dropout call."""
    m = _model()
    off, on = _micro_batch(m, False, "random", lora_dropout=0.25, seed=7), _micro_batch(m, True, "random", lora_dropout=0.25, seed=7)
    assert off.calls == on.calls == 2
    _same_micro_batch(off, on, "lora_dropout 0.25")
    plain = _micro_batch(m, True, "random")
    assert plain.loss != on.loss and not torch.equal(plain.llm, on.llm), "dropout was not on"


# ---- (d) optimizer steps with accumulation, the ranged backward ---------------------------------------------------------------------------------
def test_two_accumulated_optimizer_steps_are_bit_identical():
    """Two optimizer steps of two micro-batches each (entropy pass on: two training forwards alive), optimizer_mode zero1 at world 1, clipping on, the
    layer hook set so that the last LLM backward of every micro-batch runs as ranged per-layer calls (where the ZeRO-1 bucket exchange starts)."""
    m = _model()
    CLIP = 0.01
    res = {}
    for on in (False, True):
        tr = _trainer(m, on, optimizer_mode="zero1", lr=1e-3, max_grad_norm=CLIP, entropy_loss=True, entropy_mask_method="random",
                      entropy_mask_ratio=0.5, entropy_loss_coef=0.7)
        tr.opt_llm.sumsq_fn = tr.opt_vis.sumsq_fn = _det_sumsq
        start = tr.llm.master.clone().cpu(), tr.vis.master.clone().cpu()
        seen = []
        tr.layer_done_hook = seen.append
        torch.manual_seed(321)
        logs = []
        for step in range(2):
            for micro in range(2):
                imgs = m.images.to(m.dev) if micro == 0 else m.images.flip(0).to(m.dev)
                logs.append(tr.loss_and_backward(imgs, m.queries, m.qmask, m.resp, loss_scale=1.0))
            logs.append(tr.optimizer_step(grad_accum_div=2))
        torch.cuda.synchronize()
        assert tr.engine.wgrad_deterministic() == 1
        assert seen == list(range(m.d.n_layers - 1, -1, -1)) * 4, seen
        res[on] = SimpleNamespace(logs=logs, llm_master=tr.llm.master.clone().cpu(), vis_master=tr.vis.master.clone().cpu(), llm_work=tr.llm.work.clone().cpu(),
                                  vis_work=tr.vis.work.clone().cpu(), start=start)
        tr.engine.close()
    off, on = res[False], res[True]
    assert off.logs == on.logs, (off.logs, on.logs)
    assert off.logs[2] > CLIP, f"clipping was not active: norm {off.logs[2]}"
    for k in ("llm_master", "vis_master", "llm_work", "vis_work"):
        assert torch.equal(getattr(off, k), getattr(on, k)), f"{k} differs after two steps"
    assert not torch.equal(on.start[0], on.llm_master) and not torch.equal(on.start[1], on.vis_master), "the steps moved nothing"


# ---- (e) the command line -----------------------------------------------------------------------------------------------------------------------
def test_cli_runs_write_the_same_adapter(tmp_path, monkeypatch, capsys):
    _dev()
    from opadpo_amd import cli_sft, sft
    from opadpo_amd.optim import FlatAdamW

    class DetAdamW(FlatAdamW):                                # the clipping norm from a deterministic reduction (module docstring)
        def __init__(self, *a, **k):
            super().__init__(*a, sumsq_fn=_det_sumsq, **k)
    monkeypatch.setattr(sft, "FlatAdamW", DetAdamW)
    made = []
    orig = sft.SFTTrainer.__init__

    def init(self, *a, **k):
        orig(self, *a, **k)
        made.append(self.gradient_checkpointing)
    monkeypatch.setattr(sft.SFTTrainer, "__init__", init)

    def run(name, extra):
        out = str(tmp_path / name)
        capsys.readouterr()
        cli_sft.main(["--synthetic", "tiny", "--synthetic_samples", "8", "--output_dir", out, "--per_device_train_batch_size", "2",
                      "--gradient_accumulation_steps", "2", "--max_steps", "2", "--save_steps", "0", "--learning_rate", "1e-3", "--entropy_loss", "True",
                      "--entropy_mask_ratio", "0.5"] + extra)
        text = capsys.readouterr().out
        return torch.load(os.path.join(out, "checkpoint-final", "adapter_model.bin")), text
    sd_on, t_on = run("on", ["--cfg", "none", "--gradient_checkpointing", "True"])
    sd_off, t_off = run("off", ["--cfg", "none", "--gradient_checkpointing", "False"])
    y = tmp_path / "opa.yaml"
    y.write_text("gradient_checkpointing: True\n")
    sd_yaml, t_yaml = run("yaml", ["--cfg", str(y)])
    assert made == [True, False, True]
    assert "gradient checkpointing on" in t_on and "gradient checkpointing off" in t_off and "gradient checkpointing on" in t_yaml
    assert set(sd_on) == set(sd_off) == set(sd_yaml) and any("vision_tower" in k for k in sd_on) and any("mm_projector" in k for k in sd_on)
    bad = [k for k in sd_on if not torch.equal(sd_on[k], sd_off[k]) or not torch.equal(sd_on[k], sd_yaml[k])]
    assert not bad, f"{len(bad)} of {len(sd_on)} adapter tensors differ, e.g. {bad[:3]}"
    steps_on = [ln for ln in t_on.splitlines() if ln.startswith("{'step'")]
    assert len(steps_on) == 2 and steps_on == [ln for ln in t_off.splitlines() if ln.startswith("{'step'")]


def test_op_level_engine_refuses_at_construction():
    from opadpo_amd.model import LlavaEngine, LoraAdapter
    from opadpo_amd.sft import SFTTrainer
    from opadpo_amd.vision_train import VisionLoraAdapter
    m = _model()
    eng = LlavaEngine(m.base)
    llm, vis = LoraAdapter(m.d, m.lora, m.dev, trainable=True), VisionLoraAdapter(m.d, m.lora, m.dev)
    with pytest.raises(NotImplementedError):
        SFTTrainer(eng, llm, vis, response_len=T, gradient_checkpointing=True)
    assert SFTTrainer(eng, llm, vis, response_len=T).gradient_checkpointing is False
