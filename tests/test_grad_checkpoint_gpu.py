"""GPU: gradient checkpointing of the policy's training pass (opadpo_ctx_set_grad_checkpoint, --gradient_checkpointing).

Every kernel of the training forward is deterministic and the LoRA wgrads flush through an ordered reduce, so a layer recomputed in the backward
carries the bits the forward produced: every comparison between the two modes here is torch.equal, never a tolerance.

  * bit equality of log-probs, entropies and the flat LoRA gradient (and of d_feats for the SFT-style call) between a checkpointed and a resident
    pass, each on a fresh context with the same seeded inputs: tiny dims and two decoder layers of 7B width at a row count that reaches the 256x256
    GEMM dispatch; packed ragged rows, stacked ragged rows, padded rows, the K = 2 masked-image pass, the compact top layer off (context flag bit
    7), the chunked head (bit 9), the deferred residual (bit 13), LoRA dropout 0.05, entropy gradient + d_feats; ranged backward calls; two live
    handles backward-ed in either order;
  * memory: opadpo_ctx_bytes_peak of resident minus checkpointed = (n_layers - 1) activation slots, within one 256-byte carve alignment unit per
    carved buffer; a checkpointed pass after a resident one (with and without opadpo_ctx_trim) allocates what it allocates on a fresh context;
  * the trainer (two steps, CoPO on) and the command line (flag and reference-style YAML).
"""
import os
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SEED = 77

# tools/ctx_bits.py (parent / tree fingerprints of the context engine) imports GEOM, VARIANTS, _model, _pass and _peak from this module: keep the names
TINY = dict(ffn=512, lora_r=256, lora_alpha=512.0)            # lora_r % 256 == 0: every wgrad on the kernel with the ordered flush
WIDE = dict(hidden=4096, n_layers=2, n_heads=32, head_dim=128, ffn=11008, vocab=32000, v_hidden=128, v_layers=2, v_heads=2, v_ffn=256,
            lora_r=256, lora_alpha=512.0)                     # two decoder layers of LLaVA-1.5-7B width
# (dims, B, Q, T, long responses).  WIDE: 7 pairs of query 128 + 2 x response 384 with long responses, the shape of tests/test_bench_config_parity_gpu.py -
# its valid rows reach that file's 256x256 dispatch threshold (asserted below)
GEOM = {"tiny": (TINY, 3, 12, 9, False), "wide": (WIDE, 7, 128, 384, True)}
_models = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from opadpo_amd import lib
    lib.load()
    return torch.device("cuda:0")


def _model(name):
    """Base weights and LoRA tensors of a geometry, built once; every pass gets a FRESH context (CtxEngine) over them."""
    if name not in _models:
        from opadpo_amd.dims import LlavaDims
        from opadpo_amd.model import BaseWeights
        from opadpo_amd.synth import init_lora, init_weights
        dev = _dev()
        kw, B, Q, T, long_r = GEOM[name]
        d = LlavaDims.tiny(**kw)
        base = BaseWeights(d, init_weights(d, seed=0, std=0.05 if name == "tiny" else 0.02, device=dev), dev, need_backward=True)
        lora = init_lora(d, seed=1, b_std=0.02 if name == "tiny" else 0.01, device=dev)
        _models[name] = SimpleNamespace(d=d, base=base, lora=lora, dev=dev, inputs=_inputs(d, B, Q, T, long_r), B=B, Q=Q, T=T)
    return _models[name]


def _inputs(d, B, Q, T, long_r, seed=5):
    g = torch.Generator().manual_seed(seed)
    images = torch.randn(B, 3, d.image_size, d.image_size, generator=g).to(BF)
    queries = torch.randint(3, d.vocab, (B, Q), generator=g)
    qmask = torch.ones(B, Q, dtype=torch.bool)
    queries[0, :3] = 0                                        # left padding on one row, an image token at a different slot per row
    qmask[0, :3] = False
    for b in range(B):
        queries[b, 4 + b] = -200
    resp = {}
    for k in ("chosen_response", "rejected_response"):
        ids = torch.randint(3, d.vocab, (B, T), generator=g)
        for b in range(B):
            ln = int(torch.randint(3 * T // 4 if long_r else 2, T, (1,), generator=g))
            ids[b, ln] = 2
            ids[b, ln + 1:] = 0
        resp[k] = ids
    wts = {k: torch.randn(B, T, generator=g) for k in resp}
    image_mask = torch.rand(B, d.n_patches, generator=g) > 0.3      # the K = 2 masked-image pass: [image mask | query mask]
    return SimpleNamespace(images=images, queries=queries, qmask=qmask, resp=resp, wts=wts, image_mask=image_mask)


# variant -> (engine ragged, pack_responses, context use_tr word, LoRA dropout, masked image, entropy gradient + d_feats)
VARIANTS = {
    "packed_ragged": dict(),
    "stacked": dict(pack=False),
    "padded": dict(ragged=False),
    "masked_k2": dict(masked=True),
    "top_all_rows": dict(use_tr=1 | 1 << 7),
    "chunked_head": dict(use_tr=1 | 1 << 9),
    "resid_deferred": dict(use_tr=1 | 1 << 13),
    "lora_drop": dict(drop=0.05),
    "sft_d_feats": dict(sft=True),
}


def _engine(m, on, ragged=True, use_tr=-1):
    from opadpo_amd.ctx import CtxEngine
    eng = CtxEngine(m.base, ragged=ragged)
    if use_tr >= 0:
        eng.set_flags(use_tr=use_tr)
    eng.set_grad_checkpoint(on)
    return eng


def _peak(eng):
    return int(eng._lib.opadpo_ctx_bytes_peak(eng.ctx))


def _forward(m, eng, ad, pack=True, drop=0.0, masked=False, call=3):
    """-> (log-probs, entropies, saved handle, dlogp, SeqBatch) of one training forward."""
    from opadpo_amd.policy import AutoregressivePolicy
    x = m.inputs
    pol = AutoregressivePolicy(eng, ad, m.T, pack_responses=pack)
    qm = torch.cat([x.image_mask, x.qmask], 1) if masked else x.qmask
    keys, batch = pol.build_batch(x.queries, qm, x.resp)
    feats = eng.encode_images(x.images.to(m.dev))
    kw = dict(lora_dropout=drop, dropout_call=call, dropout_seed=SEED) if drop else {}
    logp, ent, sv = eng.seq_logprobs_fwd(ad, batch, feats, 1.0, train=True, **kw)
    dl = torch.cat([x.wts[k] for k in keys], 0).to(m.dev)
    return logp, ent, sv, dl, batch


def _pass(m, on, ragged=True, pack=True, use_tr=-1, drop=0.0, masked=False, sft=False, ranged=False):
    """One training forward + backward in one mode on a fresh context -> dict of CPU results."""
    from opadpo_amd.model import LoraAdapter
    eng = _engine(m, on, ragged, use_tr)
    ad = LoraAdapter(m.d, m.lora, m.dev, trainable=True)
    ad.grad.zero_()
    logp, ent, sv, dl, batch = _forward(m, eng, ad, pack, drop, masked)
    S, L = batch.ids.shape[0], batch.ids.shape[1] + m.d.n_patches - 1      # sequences of the pass and their padded length
    rows = S * L
    if ragged:                                                # valid rows: per sequence the prefix minus its dropped left padding, plus the valid response tokens
        plan = batch.row_plan
        rows = S * (m.Q + m.d.n_patches - 1) - int(plan[:, 0].sum()) + int(plan[:, 1:].sum())
    out = dict(logp=logp.cpu(), ent=ent.cpu(), S=S, L=L, rows=rows)
    d_feats = d_ent = None
    if sft:
        g = torch.Generator().manual_seed(11)
        d_ent = torch.randn(logp.shape, generator=g).to(m.dev)
        d_feats = torch.zeros(m.B, m.d.n_patches, m.d.hidden, dtype=torch.float32, device=m.dev)
    eng.seq_logprobs_bwd(ad, sv, dl, d_feats=d_feats, d_ent=d_ent, layer_done=(lambda i: None) if ranged else None)
    torch.cuda.synchronize()
    out.update(grad=ad.grad.clone().cpu(), det=eng.wgrad_deterministic(), peak=_peak(eng), d_feats=None if d_feats is None else d_feats.cpu())
    eng.close()
    return out


def _same(a, b, what):
    assert torch.equal(a["logp"], b["logp"]), f"{what}: log-probs differ"
    assert torch.equal(a["ent"], b["ent"]), f"{what}: entropies differ"
    assert torch.equal(a["grad"], b["grad"]), f"{what}: LoRA gradient differs (max abs {float((a['grad'] - b['grad']).abs().max())})"
    if a["d_feats"] is not None:
        assert torch.equal(a["d_feats"], b["d_feats"]), f"{what}: d_feats differ"
    assert a["det"] == 1 and b["det"] == 1, f"{what}: wgrad_deterministic {a['det']} / {b['det']}"


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("geom", list(GEOM))
def test_checkpointed_pass_has_the_bits_of_the_resident_pass(geom, variant):
    m = _model(geom)
    kw = VARIANTS[variant]
    off, on = _pass(m, False, **kw), _pass(m, True, **kw)
    assert float(off["grad"].abs().max()) > 0 and bool(torch.isfinite(off["grad"]).all())
    if geom == "wide":      # the row count must reach the 256x256 dispatch (tests/test_bench_config_parity_gpu.py: row tiles x column tiles >= 320)
        assert ((off["rows"] + 255) // 256) * (m.d.hidden // 256) >= 320, off["rows"]
    _same(off, on, f"{geom} {variant}")
    if variant == "lora_drop":                                # dropout is really on in both
        plain = _pass(m, True)
        assert not torch.equal(plain["logp"], on["logp"])


@pytest.mark.parametrize("geom", list(GEOM))
def test_ranged_backward_calls_give_the_bits_of_one_call(geom):
    """The bucket hook of the ZeRO-1 exchange splits the backward into one call per layer: nothing in the one slot outlives a layer."""
    m = _model(geom)
    one, ranged, off = _pass(m, True), _pass(m, True, ranged=True), _pass(m, False, ranged=True)
    _same(one, ranged, f"{geom} ranged vs one call")
    _same(off, ranged, f"{geom} ranged, resident vs checkpointed")


@pytest.mark.parametrize("order", ["policy_first", "masked_first"])
def test_two_live_handles_backward_in_either_order(order):
    """CoPO holds two training forwards (clean and masked image) before either backward runs; each handle owns its slot."""
    from opadpo_amd.model import LoraAdapter
    m = _model("tiny")
    res = {}
    for on in (False, True):
        eng = _engine(m, on)
        ad = LoraAdapter(m.d, m.lora, m.dev, trainable=True)
        ad.grad.zero_()
        a = _forward(m, eng, ad)
        b = _forward(m, eng, ad, masked=True)
        for logp, ent, sv, dl, _ in ((a, b) if order == "policy_first" else (b, a)):
            eng.seq_logprobs_bwd(ad, sv, dl)
        torch.cuda.synchronize()
        res[on] = dict(logp=torch.cat([a[0], b[0]]).cpu(), ent=torch.cat([a[1], b[1]]).cpu(), grad=ad.grad.clone().cpu(), det=eng.wgrad_deterministic(),
                       d_feats=None)
        eng.close()
    assert not torch.equal(res[True]["logp"][:len(a[0])], res[True]["logp"][len(a[0]):]), "the masked pass must differ from the clean one"
    _same(res[False], res[True], order)


def _slot_bytes(d, S, L):
    """Bytes of ONE layer's activation slot at M = S * L rows (csrc/ctx.hip saved_layout: the 14 per-layer buffers), before carve alignment."""
    M, H, F, r = S * L, d.hidden, d.ffn, d.lora_r
    bf, f32 = 2, 4
    return (M * H * bf + M * f32 + M * 3 * H * bf + M * 3 * r * bf + M * H * bf + S * d.n_heads * L * f32 + M * r * bf + M * H * f32 + M * H * bf + M * f32 +
            M * 2 * r * bf + M * 2 * F * bf + M * F * bf + M * r * bf)


@pytest.mark.parametrize("variant", ["packed_ragged", "padded"])
@pytest.mark.parametrize("geom", list(GEOM))
def test_peak_bytes_drop_by_all_but_one_slot(geom, variant):
    """A pass sizes its arena for the PADDED row count of its shape (ragged batches never need more), so the figure is a function of dims and shape:
    resident - checkpointed = (n_layers - 1) slots; each of the 14 carved buffers rounds up to 256 bytes once per pass, hence 14 x 256 of slack."""
    m = _model(geom)
    kw = VARIANTS[variant]
    off, on = _pass(m, False, **kw), _pass(m, True, **kw)
    want = (m.d.n_layers - 1) * _slot_bytes(m.d, off["S"], off["L"])
    got = off["peak"] - on["peak"]
    print(f"[{geom} {variant}] peak resident {off['peak']} checkpointed {on['peak']} difference {got} expected {want}")
    assert abs(got - want) <= 14 * 256, (got, want)
    assert on["peak"] < off["peak"]


@pytest.mark.parametrize("trim", [True, False])
def test_checkpointed_pass_does_not_inherit_a_resident_arena(trim):
    """arena_hint is kept per kind of pass: after a resident pass (opadpo_ctx_trim in between or not) a checkpointed pass allocates exactly what it
    allocates on a fresh context.  opadpo_ctx_bytes_peak is a lifetime maximum, so the second pass is read from the allocator's own peak counter
    (the context allocates through torch's caching allocator)."""
    from opadpo_amd.model import LoraAdapter
    m = _model("tiny")

    def alloc_of_pass(eng, ad):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        logp, ent, sv, dl, _ = _forward(m, eng, ad)
        eng.seq_logprobs_bwd(ad, sv, dl)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before

    ad = LoraAdapter(m.d, m.lora, m.dev, trainable=True)
    fresh = _engine(m, True)
    alloc_of_pass(fresh, ad)                                  # warm-up: workspaces, rope tables, batch cache
    want = alloc_of_pass(fresh, ad)
    fresh.close()
    eng = _engine(m, False)
    alloc_of_pass(eng, ad)
    resident = alloc_of_pass(eng, ad)
    if trim:
        eng._call("opadpo_ctx_trim")
    eng.set_grad_checkpoint(True)
    alloc_of_pass(eng, ad)                                    # after a trim the workspaces grow again: not part of the figure
    got = alloc_of_pass(eng, ad)
    eng.close()
    print(f"[trim={trim}] allocated by a pass: resident {resident}, checkpointed after it {got}, checkpointed on a fresh context {want}")
    assert got == want and got < resident, (got, want, resident)


def test_saved_residual_and_engine_surface():
    """opadpo_saved_residual reads the kept x_i of a checkpointed pass; the op-level engine refuses the switch."""
    import ctypes as C
    from opadpo_amd.model import LlavaEngine, LoraAdapter
    from opadpo_amd.policy import AutoregressivePolicy
    m = _model("tiny")
    xs = {}
    for on in (False, True):
        eng = _engine(m, on)
        ad = LoraAdapter(m.d, m.lora, m.dev, trainable=True)
        logp, ent, sv, dl, _ = _forward(m, eng, ad)
        rows = C.c_int(0)
        eng._call("opadpo_saved_residual", sv.handle, 0, None, C.byref(rows), None)
        got = []
        for i in range(m.d.n_layers):
            dst = torch.empty(rows.value, m.d.hidden, dtype=torch.float32, device=m.dev)
            eng._call("opadpo_saved_residual", sv.handle, i, dst.data_ptr(), C.byref(rows), torch.cuda.current_stream().cuda_stream)
            got.append(dst.cpu())
        eng.seq_logprobs_bwd(ad, sv, dl)
        torch.cuda.synchronize()
        xs[on] = got
        eng.close()
    assert all(torch.equal(a, b) for a, b in zip(xs[False], xs[True])) and not torch.equal(xs[True][0], xs[True][1])
    op = LlavaEngine(m.base)
    op.set_grad_checkpoint(False)
    with pytest.raises(NotImplementedError):
        op.set_grad_checkpoint(True)
    with pytest.raises(NotImplementedError):
        AutoregressivePolicy(op, LoraAdapter(m.d, m.lora, m.dev, trainable=True), m.T).set_gradient_checkpointing(True)


# ---- trainer and command line -------------------------------------------------------------------------------------------------------------
def test_trainer_steps_are_identical_with_and_without(tmp_path):
    """Two DPOTrainer steps (CoPO on: two training forwards live per micro-batch) with gradient_checkpointing True vs False: the same statistics and
    the same fp32 master, bit for bit, clipping active.  The optimizer's clipping norm is an fp32-ATOMIC sum over the gradient (csrc/head_optim.hip
    sumsq_kernel) whose last bit moves from run to run whatever the mode (tests/test_lora_dropout_gpu.py documents two identical runs that differ);
    both trainers here take their sum of squares from a deterministic reduction through FlatAdamW's `sumsq_fn` hook, so that every kernel of the
    step is deterministic and the comparison is exact."""
    from opadpo_amd.ctx import CtxEngine
    from opadpo_amd.model import LoraAdapter
    from opadpo_amd.policy import AutoregressivePolicy
    from opadpo_amd.synth import synth_rollout_batches
    from opadpo_amd.trainer import DPOTrainer
    m = _model("tiny")
    T, B = 16, 2
    res = {}
    for on in (False, True):
        args = SimpleNamespace(rollout_accumulation_steps=1, gradient_accumulation_steps=1, step_per_device_batch_size=B, rollout_per_device_batch_size=B,
                               rollout_batch_size=B, noptepochs=1, max_grad_norm=1.0, learning_rate=1e-3, warmup_steps=0, total_epochs=1, max_step=100,
                               save_steps=1000, output_dir=str(tmp_path / str(on)), seed=3, weight_decay=0.0, CoPO=True, AncPO=True, temperature=1.0,
                               query_len=12, response_len=T, gradient_checkpointing=on)
        torch.manual_seed(3)                                  # CoPO's image masks draw from the global CPU generator
        eng = CtxEngine(m.base)
        ad = LoraAdapter(m.d, m.lora, m.dev, trainable=True)
        ref = LoraAdapter(m.d, m.lora, m.dev, trainable=False)
        tr = DPOTrainer(args, AutoregressivePolicy(eng, ad, T), AutoregressivePolicy(eng, ref, T), optimizer_mode="allreduce",
                        optimizer_kwargs=dict(sumsq_fn=lambda g, out: out.add_(g.double().pow(2).sum().float())))
        assert tr.policy.gradient_checkpointing is on
        tr.total_sched_steps = 10
        tr._set_lr()
        it = iter(synth_rollout_batches(m.d, args, seed=1))
        stats = [dict(tr.step(it, i + 1)) for i in range(2)]
        torch.cuda.synchronize()
        assert eng.wgrad_deterministic() == 1
        res[on] = (stats, ad.master.clone().cpu(), _peak(eng))
        eng.close()
    assert res[False][0] == res[True][0], (res[False][0], res[True][0])
    assert len(res[True][0][0]) > 0 and res[True][0][0] != res[True][0][1]
    assert torch.equal(res[False][1], res[True][1])
    assert res[True][2] < res[False][2], "the trainer's training forwards did not run checkpointed"


def test_cli_flag_and_reference_yaml(tmp_path, monkeypatch):
    _dev()
    from opadpo_amd import cli
    from opadpo_amd.trainer import DPOTrainer
    seen = {}
    orig = DPOTrainer.train

    def train(self, *a, **k):
        h = orig(self, *a, **k)
        seen[self.args.output_dir] = (self.policy.gradient_checkpointing, len(h))
        return h
    monkeypatch.setattr(DPOTrainer, "train", train)
    common = ["--synthetic", "tiny", "--rollout_batch_size", "4", "--step_batch_size", "4", "--rollout_per_device_batch_size", "2",
              "--step_per_device_batch_size", "2", "--query_len", "16", "--response_len", "16", "--max_step", "3", "--save_steps", "100", "--total_epochs", "2",
              "--noptepochs", "1", "--learning_rate", "1e-4", "--report_to", "none"]      # the run of tests/test_lora_dropout_gpu.py's CLI test: two logged steps
    out = str(tmp_path / "flag")
    cli.main(common + ["--output_dir", out, "--cfg", "none", "--gradient_checkpointing", "True"])
    assert seen[out][0] is True and seen[out][1] >= 1
    assert os.path.exists(os.path.join(out, "checkpoint-final", "adapter_model", "lora_policy", "adapter_config.json"))
    # the reference's YAML nests the key under its training section
    y = tmp_path / "ref.yaml"
    y.write_text("model:\n  lora_rank: 256\ntraining:\n  gradient_checkpointing: True\n  optim:\n    weight_decay: 0.0\n")
    out = str(tmp_path / "yaml")
    cli.main(common + ["--output_dir", out, "--cfg", str(y)])
    assert seen[out][0] is True
    out = str(tmp_path / "yaml_off")                          # the command line wins
    cli.main(common + ["--output_dir", out, "--cfg", str(y), "--gradient_checkpointing", "False"])
    assert seen[out][0] is False
