"""GPU: LoRA dropout (--lora_drop) from the kernels to the command line.

  * op level: lora_dropout_fwd against tests/dropout_ref.py EXACTLY (the mask is integer arithmetic, a kept value is one bf16 rounding of
    x * fp32(1 / (1 - p))), lora_dropout_bwd_add against the fp32 formula within the bf16 rounding of its output;
  * context path: training forward and LoRA gradients at p = 0.1 against the fp32 oracle WRAPPED with the same masks (dropout_ref.OracleDropout),
    at the bounds tests/test_parity_gpu.py asserts for the same quantities at p = 0 (5e-3 mean relative log-prob error, 3e-2 per gradient block);
    packed ragged rows and padded K = 1 rows, tiny dims and one decoder layer of 7B width;
  * "really on": at p = 0.1 the log-probs leave the p = 0 pass by more than that pass is from the oracle, and the gradients miss the UNWRAPPED oracle;
  * scoping (no-grad passes, frozen / merged adapters, generation), determinism, the call counter through save -> resume, both CLIs.
"""
import ctypes as C
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import dropout_ref as DR

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
P = 0.1
SEED = 1234


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from opadpo_amd import lib
    lib.load()
    return torch.device("cuda:0")


# ---- op level ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g,module0", [(1, 3), (2, 4), (3, 0), (1, 6)])
@pytest.mark.parametrize("M,K", [(37, 136), (1, 8), (1000, 256), (259, 4096)])
def test_dropout_fwd_is_the_restatement_exactly(M, K, g, module0):
    dev = _dev()
    from opadpo_amd import lib as L
    gen = torch.Generator().manual_seed(M * 7 + K + g)
    x = torch.randn(M, K, generator=gen).to(BF)
    call, layer = (3 << 32) | 41, 5
    out = torch.full((M, g * K), 7.0, dtype=BF, device=dev)
    xd = x.to(dev)
    L.call("opadpo_lora_dropout_fwd", xd.data_ptr(), out.data_ptr(), M, K, g, P, SEED, call, layer, module0, None, L.stream())
    want = DR.dropout_fwd_ref(x, SEED, call, layer, module0, g, np.arange(M), P)
    assert torch.equal(out.cpu().view(torch.int16), want.view(torch.int16))
    # the row number of a row is its index unless a row list says otherwise (compact top layer: urow)
    idx = torch.randperm(5 * M, generator=gen)[:M].to(torch.int32)
    idx_d = idx.to(dev)
    L.call("opadpo_lora_dropout_fwd", xd.data_ptr(), out.data_ptr(), M, K, g, P, SEED, call, layer, module0, idx_d.data_ptr(), L.stream())
    want = DR.dropout_fwd_ref(x, SEED, call, layer, module0, g, idx.numpy(), P)
    assert torch.equal(out.cpu().view(torch.int16), want.view(torch.int16))


def test_dropout_ops_refuse_bad_arguments():
    dev = _dev()
    from opadpo_amd import lib as L
    x = torch.zeros(4, 16, dtype=BF, device=dev)
    o = torch.zeros(4, 48, dtype=BF, device=dev)
    for name in ("opadpo_lora_dropout_fwd", "opadpo_lora_dropout_bwd_add"):
        a, b = x, o
        for K, g, p, seed, m0 in ((12, 1, P, 1, 0), (16, 1, 1.0, 1, 0), (16, 1, -0.1, 1, 0), (16, 1, P, 1 << 32, 0), (16, 3, P, 1, 5), (16, 0, P, 1, 0)):
            with pytest.raises(L.OpadpoError):
                L.call(name, a.data_ptr(), b.data_ptr(), 4, K, g, p, seed, 0, 0, m0, None, L.stream())
    torch.cuda.synchronize()


@pytest.mark.parametrize("g,module0", [(1, 6), (2, 4), (3, 0)])
@pytest.mark.parametrize("M,K", [(37, 136), (1000, 256), (130, 4096)])
def test_dropout_bwd_add(M, K, g, module0):
    dev = _dev()
    from opadpo_amd import lib as L
    gen = torch.Generator().manual_seed(M + K + g)
    dx = torch.randn(M, K, generator=gen).to(BF)
    u = torch.randn(M, g * K, generator=gen).to(BF)
    call, layer = 9, 2
    got, ud = dx.to(dev).clone(), u.to(dev)
    L.call("opadpo_lora_dropout_bwd_add", got.data_ptr(), ud.data_ptr(), M, K, g, P, SEED, call, layer, module0, None, L.stream())
    want = DR.dropout_bwd_add_ref(dx, u, SEED, call, layer, module0, g, np.arange(M), P)
    got = got.cpu().float()
    # one bf16 rounding of the fp32 sum: half an ulp = 2^-9 relative
    assert bool(((got - want).abs() <= want.abs() * 2.0 ** -8 + 1e-30).all())
    # rate 0 adds every u_j unmasked
    got0 = dx.to(dev).clone()
    L.call("opadpo_lora_dropout_bwd_add", got0.data_ptr(), ud.data_ptr(), M, K, g, 0.0, SEED, call, layer, module0, None, L.stream())
    w0 = dx.float()
    for j in range(g):
        w0 = w0 + u[:, j * K:(j + 1) * K].float()
    assert torch.equal(got0.cpu(), w0.to(BF))


# ---- context path -----------------------------------------------------------------------------------------------------------------------
def make_inputs(d, B, Q, T, seed=0):
    g = torch.Generator().manual_seed(seed)
    images = torch.randn(B, 3, d.image_size, d.image_size, generator=g).to(BF).float()
    queries = torch.randint(3, d.vocab, (B, Q), generator=g)
    qmask = torch.ones(B, Q, dtype=torch.bool)
    queries[0, :3] = 0
    qmask[0, :3] = False
    for b in range(B):
        queries[b, 4 + b] = -200
    resp = {}
    for k in ("chosen_response", "rejected_response"):
        ids = torch.randint(3, d.vocab, (B, T), generator=g)
        for b in range(B):
            ln = int(torch.randint(2, T, (1,), generator=g))
            ids[b, ln] = 2
            ids[b, ln + 1:] = 0
        resp[k] = ids
    return images, queries, qmask, resp


def _model(kw, seed=0, std=0.05, b_std=0.02, ragged=True):
    from opadpo_amd.ctx import CtxEngine
    from opadpo_amd.dims import LlavaDims
    from opadpo_amd.model import BaseWeights, LoraAdapter
    from oracle import llava_ref as LR
    dev = _dev()
    d = LlavaDims.tiny(**kw)
    od = LR.LlavaDims.tiny(**dict(kw, lora_r=d.lora_r, lora_alpha=d.lora_alpha))
    W = {k: v.to(BF).float() for k, v in LR.init_weights(od, seed=seed, std=std).items()}
    lora = {k: v.to(BF).float() for k, v in LR.init_lora(od, seed=seed + 1, b_std=b_std, with_vision=False).items()}
    base = BaseWeights(d, W, dev, need_backward=True)
    return SimpleNamespace(d=d, od=od, W=W, lora=lora, base=base, eng=CtxEngine(base, ragged=ragged), ad=LoraAdapter(d, lora, dev, trainable=True),
                           dev=dev, LR=LR)


TINY = dict()
DET = dict(ffn=512, lora_r=256, lora_alpha=512.0)              # every wgrad on the 256x256 kernel: bit-reproducible gradients
WIDE = dict(hidden=4096, n_layers=1, n_heads=32, head_dim=128, ffn=11008, vocab=32000, v_hidden=128, v_layers=2, v_heads=2, v_ffn=256,
            lora_r=256, lora_alpha=512.0)                      # one decoder layer of LLaVA-1.5-7B width


def _row_map(m, pol, batch, queries, qmask, resp, keys):
    from opadpo_amd.policy import host_row_plan
    B, Q = queries.shape
    T = resp[keys[0]].shape[1]
    pfx = Q + m.d.n_patches - 1
    L = pfx + T
    if not m.eng.ragged:
        return DR.row_map_padded(len(keys) * B, L)[0], len(keys) * B, L
    assert pol.pack_responses and batch.K == len(keys)
    lead, lens = host_row_plan(queries, qmask, resp)
    return DR.row_map_packed(lead, lens, keys, B, pfx)[0], len(keys) * B, L


def _hip_pass(m, pol, images, queries, qmask, resp, wts, p, call):
    """One training forward + backward on the context path -> (log-probs per key, flat gradient copy)."""
    keys, batch = pol.build_batch(queries, qmask, resp)
    B = queries.shape[0]
    feats = m.eng.encode_images(images.to(m.dev))
    m.ad.grad.zero_()
    kw = {} if p is None else dict(lora_dropout=p, dropout_call=call, dropout_seed=SEED)
    logp, _, sv = m.eng.seq_logprobs_fwd(m.ad, batch, feats, 1.0, train=True, **kw)
    dl = torch.cat([wts[k] for k in keys], 0).to(m.dev)
    m.eng.seq_logprobs_bwd(m.ad, sv, dl)
    torch.cuda.synchronize()
    return {k: logp[i * B:(i + 1) * B].cpu() for i, k in enumerate(keys)}, m.ad.grad.clone().cpu(), (keys, batch)


def _oracle_pass(m, images, queries, qmask, resp, wts, drop):
    lora = {k: v.clone().requires_grad_(True) for k, v in m.lora.items()}
    if drop is None:
        want = m.LR.policy_forward(images, queries, qmask, resp, m.W, lora, m.od, 1.0)
    else:
        with drop.patch(m.LR):
            want = m.LR.policy_forward(images, queries, qmask, resp, m.W, lora, m.od, 1.0)
    sum((want[k + "_logprobs"] * wts[k]).sum() for k in resp).backward()
    return {k: want[k + "_logprobs"].detach() for k in resp}, lora


def _logp_err(got, want, resp):
    worst = 0.0
    for k in resp:
        valid = resp[k] != 0
        assert bool((got[k][~valid] == 0).all()), "pad cells must be exactly zero"
        worst = max(worst, float(((got[k] - want[k]).abs()[valid] / want[k].abs()[valid].clamp_min(1e-3)).mean()))
    return worst


def _grad_errs(m, flat, lora):
    from opadpo_amd.model import _peft_map, lora_blocks
    pm = _peft_map(m.d)
    errs = {}
    for i in range(m.d.n_layers):
        for name, rows, cols in lora_blocks(m.d):
            off = m.ad.offsets[i][name][0]
            got = flat[off:off + rows * cols].view(rows, cols)
            ref = torch.zeros(rows, cols)
            for mod, ab, r0, nr in pm[name]:
                ref[r0:r0 + nr] = lora[f"base_model.model.model.layers.{i}.{mod}.{ab}.weight"].grad
            assert bool(torch.isfinite(got).all())
            errs[f"L{i}_{name}"] = float((got - ref).norm() / (ref.norm() + 1e-12))
    return errs


def _check_against_wrapped_oracle(kw, B, Q, T, ragged, pack, std, b_std, tag, gemm_variant=-1):
    """Forward and gradients at p = 0.1 against the wrapped oracle at the p = 0 bounds of tests/test_parity_gpu.py; the p = 0 pass in the same test."""
    from opadpo_amd.policy import AutoregressivePolicy
    m = _model(kw, std=std, b_std=b_std, ragged=ragged)
    m.eng.set_flags(gemm_variant=gemm_variant)
    images, queries, qmask, resp = make_inputs(m.d, B, Q, T, seed=5)
    g = torch.Generator().manual_seed(9)
    wts = {k: torch.randn(B, T, generator=g) for k in resp}
    pol = AutoregressivePolicy(m.eng, m.ad, T, pack_responses=pack)
    call = 17
    lp0, g0, _ = _hip_pass(m, pol, images, queries, qmask, resp, wts, None, 0)
    lp1, g1, (keys, batch) = _hip_pass(m, pol, images, queries, qmask, resp, wts, P, call)
    rm, S, L = _row_map(m, pol, batch, queries, qmask, resp, keys)
    o0, lora0 = _oracle_pass(m, images, queries, qmask, resp, wts, None)
    o1, lora1 = _oracle_pass(m, images, queries, qmask, resp, wts, DR.OracleDropout(P, SEED, call, rm, S, L))
    e0, e1 = _logp_err(lp0, o0, resp), _logp_err(lp1, o1, resp)
    ge0, ge1 = _grad_errs(m, g0, lora0), _grad_errs(m, g1, lora1)
    moved = _logp_err(lp1, lp0, resp)                    # how far dropout moved the log-probs
    cross = _grad_errs(m, g1, lora0)                     # dropout gradients against the oracle WITHOUT dropout
    print(f"[{tag}] log-prob mean rel err: p=0 {e0:.3e}, p={P} {e1:.3e} (vs wrapped oracle); p={P} vs p=0 pass {moved:.3e}")
    print(f"[{tag}] worst gradient block rel err: p=0 {max(ge0.values()):.3e}, p={P} {max(ge1.values()):.3e}; vs unwrapped oracle {max(cross.values()):.3e}")
    print(f"[{tag}] per block p={P}: " + json.dumps({k: round(v, 5) for k, v in ge1.items()}))
    assert e0 < 5e-3 and max(ge0.values()) < 3e-2, (e0, ge0)
    assert e1 < 5e-3, f"p={P}: mean relative log-prob error {e1} vs the wrapped oracle (p=0: {e0})"
    assert max(ge1.values()) < 3e-2, f"p={P}: gradient blocks vs the wrapped oracle {ge1} (p=0: {ge0})"
    # it is really on
    assert moved > e0 and moved > e1, (moved, e0, e1)
    assert max(cross.values()) >= 3e-2, f"gradients at p={P} still meet the bound against the oracle WITHOUT dropout: {cross}"
    return m, ge1


@pytest.mark.parametrize("layout", ["packed_ragged", "padded_k1"])
def test_context_path_against_wrapped_oracle_tiny(layout):
    ragged = layout == "packed_ragged"
    _check_against_wrapped_oracle(TINY, 2, 12, 9, ragged, ragged, 0.05, 0.02, f"tiny {layout}")


@pytest.mark.parametrize("layout", ["packed_ragged", "padded_k1", "packed_ragged_w4"])
def test_context_path_against_wrapped_oracle_7b_width(layout):
    """packed_ragged_w4: gemm variant 31 sends every product to the 256x256 kernel the benchmark's row counts select (grouped A operands per r-wide
    column group, the r-deep dT . A products)."""
    ragged = layout != "padded_k1"
    _check_against_wrapped_oracle(dict(WIDE), 2, 16, 24, ragged, ragged, 0.02, 0.01, f"7B width {layout}", 31 if layout.endswith("w4") else -1)


def test_top_layer_rows_hash_with_their_row_of_the_pass():
    """The compact top layer (only the head's rows run its o-projection / MLP) on and off (context flag bit 7): both meet the wrapped oracle,
    i.e. a top-layer row hashes with urow[u], not u."""
    from opadpo_amd.policy import AutoregressivePolicy
    m = _model(TINY)
    B, Q, T = 2, 12, 9
    images, queries, qmask, resp = make_inputs(m.d, B, Q, T, seed=8)
    g = torch.Generator().manual_seed(3)
    wts = {k: torch.randn(B, T, generator=g) for k in resp}
    pol = AutoregressivePolicy(m.eng, m.ad, T)
    lp_c, g_c, (keys, batch) = _hip_pass(m, pol, images, queries, qmask, resp, wts, P, 5)
    m.eng.set_flags(use_tr=1 | 1 << 7)
    try:
        lp_a, g_a, _ = _hip_pass(m, pol, images, queries, qmask, resp, wts, P, 5)
    finally:
        m.eng.set_flags()
    rm, S, L = _row_map(m, pol, batch, queries, qmask, resp, keys)
    o1, lora1 = _oracle_pass(m, images, queries, qmask, resp, wts, DR.OracleDropout(P, SEED, 5, rm, S, L))
    top = m.d.n_layers - 1
    for tag, lp, gr in (("compact", lp_c, g_c), ("all rows", lp_a, g_a)):
        errs = _grad_errs(m, gr, lora1)
        print(f"[top layer {tag}] logp {_logp_err(lp, o1, resp):.3e} top-layer blocks " + json.dumps({k: round(v, 5) for k, v in errs.items() if k.startswith(f'L{top}_')}))
        assert _logp_err(lp, o1, resp) < 5e-3
        assert max(v for k, v in errs.items() if k.startswith(f"L{top}_")) < 3e-2, errs
    assert _logp_err(lp_c, lp_a, resp) < 1e-3


def test_rate_zero_and_no_grad_passes_are_untouched():
    """p = 0 through the new arguments is the pass without them, bit for bit; train=False, a frozen adapter, a merged adapter and generation
    (sampling and beams) do not see the rate at all."""
    from opadpo_amd.generate import Generator
    from opadpo_amd.model import LoraAdapter
    from opadpo_amd.policy import AutoregressivePolicy
    m = _model(DET)
    B, Q, T = 2, 12, 9
    images, queries, qmask, resp = make_inputs(m.d, B, Q, T, seed=2)
    g = torch.Generator().manual_seed(1)
    wts = {k: torch.randn(B, T, generator=g) for k in resp}
    pol = AutoregressivePolicy(m.eng, m.ad, T)
    lp_a, g_a, (keys, batch) = _hip_pass(m, pol, images, queries, qmask, resp, wts, None, 0)
    lp_b, g_b, _ = _hip_pass(m, pol, images, queries, qmask, resp, wts, 0.0, 7)
    assert m.eng.wgrad_deterministic() == 1
    assert all(torch.equal(lp_a[k], lp_b[k]) for k in keys) and torch.equal(g_a, g_b)
    feats = m.eng.encode_images(images.to(m.dev))
    frozen = LoraAdapter(m.d, m.lora, m.dev, trainable=False)
    merged = LoraAdapter(m.d, m.lora, m.dev, trainable=False)
    merged.merge_into_base(m.base)
    for ad in (m.ad, frozen, merged, None):
        a = m.eng.seq_logprobs_fwd(ad, batch, feats, 1.0, train=False)[0].cpu()
        b = m.eng.seq_logprobs_fwd(ad, batch, feats, 1.0, train=False, lora_dropout=P, dropout_call=3, dropout_seed=SEED)[0].cpu()
        assert torch.equal(a, b)
    # a rate handed to a no-grad pass is not left behind for the next training forward either
    lp_c, g_c, _ = _hip_pass(m, pol, images, queries, qmask, resp, wts, None, 0)
    assert all(torch.equal(lp_a[k], lp_c[k]) for k in keys) and torch.equal(g_a, g_c)
    # policies: the frozen reference policy and a no_grad call of the trained one ignore the policy's rate
    for ad in (frozen, m.ad):
        p0, p1 = AutoregressivePolicy(m.eng, ad, T), AutoregressivePolicy(m.eng, ad, T)
        p1.set_lora_dropout(P, SEED)
        kw = dict(images=images.to(m.dev), queries=queries, queries_attn_masks=qmask, **resp)
        with torch.no_grad():
            a, b = p0(**kw), p1(**kw)
        assert all(torch.equal(a[k], b[k]) for k in a) and p1.dropout_calls == 0
    p1 = AutoregressivePolicy(m.eng, m.ad, T)
    p1.set_lora_dropout(P, SEED)
    out = p1(images=images.to(m.dev), queries=queries, queries_attn_masks=qmask, **resp)
    assert p1.dropout_calls == 1 and not torch.equal(out["chosen_response_logprobs"].detach().cpu(), lp_a["chosen_response"])
    del out
    p1._pending_bwd = 0
    # generation (sampling and beams): prefill and decode never drop, whatever the context was told for its next training forward
    gen = Generator(m.eng, m.ad)
    outs = []
    for rate in (None, P):
        if rate is not None:
            m.eng._call("opadpo_ctx_set_lora_dropout", rate, SEED, 1)
        s_ = gen.generate(queries, qmask, images.to(m.dev), max_new_tokens=6, temperature=1.0, top_k=10, top_p=0.9, seed=4, eos_token_id=2, pad_token_id=0)
        bm = m.eng.generate_beams(m.ad, queries, qmask, feats, num_beams=2, max_new_tokens=6, eos_token_id=2, pad_token_id=0, use_graph=False)
        outs.append((s_, bm[0], bm[1]))
    m.eng._call("opadpo_ctx_set_lora_dropout", 0.0, SEED, 0)
    assert all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(outs[0], outs[1]))


def test_same_seed_and_call_same_gradient_other_call_or_rank_other_gradient():
    from opadpo_amd.policy import AutoregressivePolicy
    m = _model(DET)
    B, Q, T = 2, 12, 9
    images, queries, qmask, resp = make_inputs(m.d, B, Q, T, seed=6)
    g = torch.Generator().manual_seed(2)
    wts = {k: torch.randn(B, T, generator=g) for k in resp}
    pol = AutoregressivePolicy(m.eng, m.ad, T)
    lp_a, g_a, (keys, _) = _hip_pass(m, pol, images, queries, qmask, resp, wts, P, 12)
    assert m.eng.wgrad_deterministic() == 1
    lp_b, g_b, _ = _hip_pass(m, pol, images, queries, qmask, resp, wts, P, 12)
    assert all(torch.equal(lp_a[k], lp_b[k]) for k in keys) and torch.equal(g_a, g_b)
    lp_c, g_c, _ = _hip_pass(m, pol, images, queries, qmask, resp, wts, P, 13)
    assert not torch.equal(g_a, g_c) and not torch.equal(lp_a[keys[0]], lp_c[keys[0]])
    # the rank is folded into the call: two ranks of one step draw different masks
    r0, r1 = AutoregressivePolicy(m.eng, m.ad, T), AutoregressivePolicy(m.eng, m.ad, T)
    r0.set_lora_dropout(P, SEED, rank=0, world=2)
    r1.set_lora_dropout(P, SEED, rank=1, world=2)
    c0, c1 = r0.next_dropout()["dropout_call"], r1.next_dropout()["dropout_call"]
    assert c0 != c1
    _, g_r0, _ = _hip_pass(m, pol, images, queries, qmask, resp, wts, P, c0)
    _, g_r1, _ = _hip_pass(m, pol, images, queries, qmask, resp, wts, P, c1)
    assert not torch.equal(g_r0, g_r1)


# ---- trainer and CLIs -------------------------------------------------------------------------------------------------------------------
def _trainer(m, tmp, T, B, lr=0.0):
    from opadpo_amd.model import LoraAdapter
    from opadpo_amd.policy import AutoregressivePolicy
    from opadpo_amd.trainer import DPOTrainer
    args = SimpleNamespace(rollout_accumulation_steps=1, gradient_accumulation_steps=1, step_per_device_batch_size=B, rollout_per_device_batch_size=B,
                           rollout_batch_size=B, noptepochs=1, max_grad_norm=1.0, learning_rate=lr, warmup_steps=0, total_epochs=1, max_step=100,
                           save_steps=1000, output_dir=str(tmp), seed=3, weight_decay=0.0, CoPO=False, AncPO=False, temperature=1.0, lora_drop=P,
                           query_len=12, response_len=T)
    ad = LoraAdapter(m.d, m.lora, m.dev, trainable=True)
    if not hasattr(m, "ref_ad"):                         # one frozen reference adapter for every trainer of a test (a context holds 7 adapters)
        m.ref_ad = LoraAdapter(m.d, m.lora, m.dev, trainable=False)
    ref = m.ref_ad
    tr = DPOTrainer(args, AutoregressivePolicy(m.eng, ad, T), AutoregressivePolicy(m.eng, ref, T), optimizer_mode="allreduce")
    tr.total_sched_steps = 10
    tr._set_lr()
    return tr, args


def test_call_counter_survives_save_and_resume(tmp_path):
    """An uninterrupted run of two steps against step 1 -> save -> fresh trainer -> resume -> step 2: the second step's loss terms are the same, bit
    for bit, and they are NOT when the resumed trainer's call counter restarts at 0 (step 2 would replay step 1's masks).

    The learning rate of these runs is 0.  Measured on an MI355X: the trainer's weight update is not bit-reproducible from run to run with or without
    dropout - two uninterrupted runs of this very configuration at --lora_drop 0 and lr 1e-2 left sum(master) = 18.36149342765566 vs 18.36149345582817
    after step 1 and dpo/loss-stand_gen = 0.6942369937896729 vs 0.6942129135131836 at step 2 (packed and stacked responses alike; at p = 0.1:
    dpo/loss-AI_gen 0.6639220714569092 vs 0.663923978805542) - so with moving weights no resumed run can match an uninterrupted one bit for bit, whatever
    the counter does.  With the weights held still the step-2 loss is a function of the batch and the dropout masks alone, which is what the counter decides."""
    from opadpo_amd.synth import synth_rollout_batches
    m = _model(DET)
    T, B = 16, 2

    def pick(st):      # the loss terms; the clipping norm is an fp32-atomic reduction over the (bit-identical) gradient and may differ in its last bit
        return {k: v for k, v in st.items() if k.startswith("dpo/loss") and "grad_norm" not in k}

    def losses(tr, args, n, it):
        out = []
        for i in range(n):
            st = tr.step(it, i + 1)
            out.append(pick(st))
        return out
    tr_a, args = _trainer(m, tmp_path / "a", T, B)
    assert tr_a.policy.lora_dropout == P
    la = losses(tr_a, args, 2, iter(synth_rollout_batches(m.d, args, seed=1)))
    assert m.eng.wgrad_deterministic() == 1
    assert tr_a.policy.dropout_calls == 2
    del tr_a
    tr_b, _ = _trainer(m, tmp_path / "b", T, B)
    it = iter(synth_rollout_batches(m.d, args, seed=1))
    lb = losses(tr_b, args, 1, it)
    assert lb[0] == la[0] and len(la[0]) > 0
    ck = str(tmp_path / "b" / "checkpoint-2")
    tr_b.save_model(ck)
    cfg = json.load(open(os.path.join(ck, "adapter_model", "lora_policy", "adapter_config.json")))
    assert cfg["lora_dropout"] == P
    assert torch.load(os.path.join(ck, "optimizer.pt"))["dropout_calls"] == 1
    del tr_b
    tr_c, _ = _trainer(m, tmp_path / "c", T, B)         # resume restores the fp32 master and the bf16 working copy from optimizer.pt
    assert tr_c.resume_training(ck) == 2 and tr_c.policy.dropout_calls == 1
    st = tr_c.step(it, 2)
    lc = pick(st)
    assert lc == la[1], (lc, la[1])
    # the counter matters: the same resumed step with the counter back at 0 gives another loss
    del tr_c
    tr_d, _ = _trainer(m, tmp_path / "d", T, B)
    tr_d.resume_training(ck)
    tr_d.policy.dropout_calls = 0
    it2 = iter(synth_rollout_batches(m.d, args, seed=1))
    next(it2)
    st = tr_d.step(it2, 2)
    assert pick(st) != la[1]


def test_train_cli_honours_lora_drop(tmp_path, monkeypatch):
    _dev()
    from opadpo_amd import cli
    from opadpo_amd.trainer import DPOTrainer
    logs = {}
    orig = DPOTrainer.train

    def train(self, *a, **k):
        h = orig(self, *a, **k)
        logs[self.args.output_dir] = [dict(s) for s in h]
        return h
    monkeypatch.setattr(DPOTrainer, "train", train)

    def run(name, rate):
        out = str(tmp_path / name)
        cli.main(["--synthetic", "tiny", "--output_dir", out, "--rollout_batch_size", "4", "--step_batch_size", "4", "--rollout_per_device_batch_size", "2",
                  "--step_per_device_batch_size", "2", "--query_len", "16", "--response_len", "16", "--max_step", "3", "--save_steps", "100",
                  "--total_epochs", "2", "--noptepochs", "1", "--learning_rate", "1e-4", "--report_to", "none", "--cfg", "none", "--lora_drop", rate])
        cfg = json.load(open(os.path.join(out, "checkpoint-final", "adapter_model", "lora_policy", "adapter_config.json")))
        return logs[out], cfg
    l0, c0 = run("p0", "0.0")
    l0b, _ = run("p0b", "0.0")
    l1, c1 = run("p1", "0.1")
    assert len(l0) == len(l1) == 2
    key = [k for k in l0[0] if k.startswith("dpo/loss") and "grad_norm" not in k]      # forward quantities (r = 128: the wgrads flush with atomics)
    assert key, l0[0]
    assert all(l0[0][k] == l0b[0][k] for k in key), "step 1 at rate 0 is not reproducible: the comparison below would show nothing"
    assert any(l0[0][k] != l1[0][k] for k in key), f"--lora_drop 0.1 trained like --lora_drop 0.0: {l0[0]}"
    assert c0["lora_dropout"] == 0.0 and c1["lora_dropout"] == 0.1
    with pytest.raises(ValueError):
        cli.main(["--synthetic", "tiny", "--output_dir", str(tmp_path / "bad"), "--cfg", "none", "--lora_drop", "1.0"])


def test_sft_cli_honours_lora_drop(tmp_path, capsys):
    _dev()
    import ast
    from opadpo_amd import cli_sft

    def run(name, rate):
        out = str(tmp_path / name)
        capsys.readouterr()
        cli_sft.main(["--synthetic", "tiny", "--synthetic_samples", "8", "--output_dir", out, "--per_device_train_batch_size", "2",
                      "--gradient_accumulation_steps", "1", "--max_steps", "2", "--save_steps", "0", "--learning_rate", "1e-3", "--cfg", "none",
                      "--lora_drop", rate])
        text = capsys.readouterr().out
        steps = [ast.literal_eval(ln) for ln in text.splitlines() if ln.startswith("{'step'")]
        cfg = json.load(open(os.path.join(out, "checkpoint-final", "adapter_config.json")))
        return steps, cfg, text
    s0, c0, t0 = run("p0", "0.0")
    s0b, _, _ = run("p0b", "0.0")
    s1, c1, t1 = run("p1", "0.1")
    assert len(s0) == len(s1) == 2
    assert s0[0]["loss"] == s0b[0]["loss"] and s0[0]["loss"] != s1[0]["loss"], (s0[0], s1[0])
    assert c0["lora_dropout"] == 0.0 and c1["lora_dropout"] == 0.1
    # the vision side of the OPA stage trains without dropout, and says so
    assert "LLM linears only" in t1 and "LLM linears only" not in t0
    with pytest.raises(SystemExit):
        cli_sft.main(["--synthetic", "tiny", "--output_dir", str(tmp_path / "bad"), "--cfg", "none", "--lora_drop", "1.5"])
