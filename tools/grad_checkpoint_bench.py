#!/usr/bin/env python3
"""Cost and saving of gradient checkpointing in the trainer step of the benchmark shape on one MI355X: LLaVA-1.5-7B synthetic weights, LoRA r = 256,
22 packed (chosen, rejected) pairs of query 128 + response 384 on ragged rows, frozen reference merged - the step bench.py times (reference pass,
policy forward, pair loss, LoRA backward, clip + AdamW).  The same process runs the step with checkpointing off and on in alternating blocks after
a warm-up of both and records, per mode, the median ms per step and the allocator's peak; in the off blocks the policy's training forward is
bracketed by events (the recompute must cost less than it: no embedding, no head, no down product).  Then, checkpointing on, ONE step at the
largest pair count whose PREDICTED footprint stays under --hbm-fraction of the device memory (no run is started to find the limit by failing):
prediction = what does not scale with the batch (allocated before the first step) + the measured on-mode peak above it, scaled by pairs / --pairs;
the activation arena, the workspaces and the batch all grow linearly in the pairs, and the head only gets cheaper once it goes chunked.
The trial is also capped by --max-pairs (row counts the kernels have been run at); the memory-bound count is reported next to it.
Prints one JSON line.

--stage opa: the OPA LoRA-SFT stage instead (run/train_opa.sh: per-device batch 4, query 128 + response 896, LoRA on LLM + CLIP tower + projector).  Per
micro-batch (SFTTrainer.loss_and_backward, gradients zeroed after it) with the entropy regulariser off and on (its masked pixels are made once, outside
the timed region): median ms of alternating off / on blocks, the allocator's peak per mode and the context's own `bytes_peak` (one context per mode:
the figure is a lifetime maximum).  On a tree whose SFTTrainer has no `gradient_checkpointing` keyword only the off blocks run: the same command
there gives the parent's figure for the off-against-parent comparison."""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "opa-dpo_amd"))
from opadpo_amd import lib as L  # noqa: E402
from opadpo_amd.ctx import CtxEngine  # noqa: E402
from opadpo_amd.dims import LlavaDims  # noqa: E402
from opadpo_amd.losses import DPOArgs, pair_loss  # noqa: E402
from opadpo_amd.model import BaseWeights, LoraAdapter  # noqa: E402
from opadpo_amd.optim import FlatAdamW  # noqa: E402
from opadpo_amd.policy import AutoregressivePolicy  # noqa: E402
from opadpo_amd.synth import init_lora, init_weights, synth_pairs  # noqa: E402


def main_opa(a):
    import inspect
    from opadpo_amd.sft import SFTTrainer
    from opadpo_amd.vision_train import VisionLoraAdapter
    L.load()
    dev = torch.device("cuda:0")
    d = LlavaDims.llava15_7b() if a.model == "7b" else LlavaDims.tiny()
    q_len, t_len = (128, 896) if a.model == "7b" else (16, 16)
    has_switch = "gradient_checkpointing" in inspect.signature(SFTTrainer.__init__).parameters
    modes = (False, True) if has_switch else (False,)
    base = BaseWeights(d, init_weights(d, seed=0, device=dev), dev, need_backward=True)
    lora = init_lora(d, seed=1, device=dev, with_vision=True)
    llm, vis = LoraAdapter(d, lora, dev, trainable=True), VisionLoraAdapter(d, lora, dev)
    tr = {on: SFTTrainer(CtxEngine(base), llm, vis, response_len=t_len, lr=1e-6, entropy_mask_ratio=0.8, entropy_loss_coef=0.01,
                         **(dict(gradient_checkpointing=on) if has_switch else {})) for on in modes}
    pool = []
    for i in range(a.steps):
        p = synth_pairs(d, a.batch, q_len, t_len, seed=i, device=dev)
        g = torch.Generator().manual_seed(1000 + i)
        keep = (torch.rand(a.batch, 1, d.image_size // d.patch, d.image_size // d.patch, generator=g) > 0.8).to(dev)
        masked = p["images"] * keep.repeat_interleave(d.patch, 2).repeat_interleave(d.patch, 3)
        pool.append(dict(images=p["images"], queries=p["queries"], queries_attn_masks=p["queries_attn_masks"], responses=p["chosen"], masked_images=masked))
    torch.cuda.synchronize()
    fixed = torch.cuda.memory_allocated()

    def block(on, entropy):
        t = tr[on]
        t.entropy_loss = entropy
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        for b in pool:
            t.loss_and_backward(b["images"], b["queries"], b["queries_attn_masks"], b["responses"], masked_images=b["masked_images"] if entropy else None)
            llm.grad.zero_()
            vis.grad.zero_()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / len(pool) * 1e3, torch.cuda.max_memory_allocated()

    out = {"metric": "OPA LoRA-SFT micro-batch (loss_and_backward) with gradient checkpointing vs without, same process, alternating blocks", "stage": "opa",
           "model": a.model, "batch": a.batch, "query_len": q_len, "response_len": t_len, "modes": ["off", "on"] if has_switch else ["off"],
           "fixed_allocated_GB": fixed / 1e9}
    name = {False: "off", True: "on"}
    for entropy in (False, True):
        for on in modes:
            block(on, entropy)                                  # warm-up of each form (allocator, workspaces)
        t, peak = {on: [] for on in modes}, {on: 0 for on in modes}
        for _ in range(a.blocks):
            for on in modes:
                ms, pk = block(on, entropy)
                t[on].append(ms)
                peak[on] = max(peak[on], pk)
        med = {on: sorted(v)[len(v) // 2] for on, v in t.items()}
        leg = {"ms_" + name[on]: med[on] for on in modes}
        leg.update({"blocks_" + name[on] + "_ms": t[on] for on in modes})
        leg["hbm_peak_allocated_GB"] = {name[on]: peak[on] / 1e9 for on in modes}
        if has_switch:
            leg.update(extra_ms=med[True] - med[False], extra_fraction=med[True] / med[False] - 1.0, spread_ms_off=max(t[False]) - min(t[False]),
                       peak_on_below_off=bool(peak[True] < peak[False]))
        out["entropy_loss_" + ("on" if entropy else "off")] = leg
    # lifetime maximum of each context: the entropy-on micro-batch (two training forwards alive) sets it
    out["ctx_bytes_peak_GB"] = {name[on]: int(tr[on].engine._lib.opadpo_ctx_bytes_peak(tr[on].engine.ctx)) / 1e9 for on in modes}
    print(json.dumps(out), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stage", default="dpo", choices=["dpo", "opa"], help="dpo: the trainer step of the benchmark shape; opa: the LoRA-SFT micro-batch")
    ap.add_argument("--batch", type=int, default=4, help="--stage opa: per-device micro-batch")
    ap.add_argument("--model", default="7b", choices=["7b", "tiny"])
    ap.add_argument("--pairs", type=int, default=22)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3, help="steps per block")
    ap.add_argument("--hbm-fraction", type=float, default=0.9, help="largest-fit trial: predicted footprint must stay under this share of the device memory")
    ap.add_argument("--max-pairs", type=int, default=32, help="upper end of the largest-fit trial (0: skip the trial).  Default 32: from 34 pairs the "
                    "padded gate|up activation of 7B ([rows, 2 x 11008] bf16) passes 2^31 bytes, a size no test of the kernels has run at")
    ap.add_argument("--json", default=None, help="also write the result to this file")
    a = ap.parse_args()
    if a.stage == "opa":
        return main_opa(a)
    L.load()
    dev = torch.device("cuda:0")
    d = LlavaDims.llava15_7b() if a.model == "7b" else LlavaDims.tiny()
    q_len, t_len = (128, 384) if a.model == "7b" else (16, 16)
    base = BaseWeights(d, init_weights(d, seed=0, device=dev), dev, need_backward=True)
    eng = CtxEngine(base)
    pol_ad = LoraAdapter(d, init_lora(d, seed=1, device=dev), dev, trainable=True)
    ref_ad = LoraAdapter(d, init_lora(d, seed=2, device=dev), dev, trainable=False)
    ref_ad.merge_into_base(base)
    torch.cuda.empty_cache()
    policy, ref_policy = AutoregressivePolicy(eng, pol_ad, t_len), AutoregressivePolicy(eng, ref_ad, t_len)
    opt = FlatAdamW(pol_ad.master, pol_ad.grad, pol_ad.work, lr=1e-6, max_grad_norm=1.0)
    pool = [synth_pairs(d, a.pairs, q_len, t_len, seed=i, device=dev) for i in range(a.steps)]
    largs = DPOArgs()
    torch.cuda.synchronize()
    fixed = torch.cuda.memory_allocated()                       # weights, adapters, optimizer state, the batch pool
    fwd_events = []

    def step(b, time_fwd=False):
        feats = eng.encode_images(b["images"])
        kw = dict(queries=b["queries"], queries_attn_masks=b["queries_attn_masks"], image_feats=feats, chosen_response=b["chosen"],
                  rejected_response=b["rejected"], row_lead=b["row_lead"], row_lens=b["row_lens"])
        with torch.no_grad():
            r = ref_policy(**kw)
        if time_fwd:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        o = policy(**kw)
        if time_fwd:
            e1.record()
            fwd_events.append((e0, e1))
        loss, _, _ = pair_loss(largs, o["chosen_response_logprobs"], o["rejected_response_logprobs"], r["chosen_response_logprobs"],
                               r["rejected_response_logprobs"])
        loss.backward()
        opt.step()
        opt.zero_grad()
        pol_ad.refresh_transposed()

    def block(on, batches=None):
        policy.set_gradient_checkpointing(on)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        for b in (batches or pool):
            step(b, time_fwd=not on)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / len(batches or pool) * 1e3, torch.cuda.max_memory_allocated()

    block(False); block(True)                                   # warm-up of both forms (allocator, workspaces)
    fwd_events.clear()
    t, peak = {False: [], True: []}, {False: 0, True: 0}
    for _ in range(a.blocks):                                   # alternate the two in blocks
        for on in (False, True):
            ms, pk = block(on)
            t[on].append(ms)
            peak[on] = max(peak[on], pk)
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    fwd = sorted(e0.elapsed_time(e1) for e0, e1 in fwd_events)
    fwd_ms = fwd[len(fwd) // 2]
    spread = max(t[False]) - min(t[False])
    extra = med[True] - med[False]
    out = {"metric": "trainer step with gradient checkpointing vs without, same process, alternating blocks", "model": a.model, "pairs": a.pairs,
           "ms_off": med[False], "ms_on": med[True], "extra_ms": extra, "extra_fraction": med[True] / med[False] - 1.0,
           "policy_train_forward_ms_off": fwd_ms, "spread_ms_off": spread, "extra_within_forward_plus_spread": bool(extra <= fwd_ms + spread),
           "blocks_off_ms": t[False], "blocks_on_ms": t[True],
           "hbm_peak_allocated_GB": {"off": peak[False] / 1e9, "on": peak[True] / 1e9}, "fixed_allocated_GB": fixed / 1e9}
    # ---- the largest pair count that fits with checkpointing on: predicted, then ONE step at it ------------------------------------------
    if a.max_pairs > a.pairs:
        total = torch.cuda.mem_get_info()[1]
        per_pair = (peak[True] - fixed) / a.pairs
        n_mem = int((a.hbm_fraction * total - fixed) // per_pair)
        n = min(a.max_pairs, n_mem)
        fit = {"device_memory_GB": total / 1e9, "budget_GB": a.hbm_fraction * total / 1e9, "predicted_GB_per_pair_on": per_pair / 1e9,
               "predicted_GB_per_pair_off": (peak[False] - fixed) / a.pairs / 1e9,
               "largest_pairs_predicted_off": int((a.hbm_fraction * total - fixed) // ((peak[False] - fixed) / a.pairs)), "largest_pairs_predicted_on": n_mem, "pairs_tried_on": n}
        if n > a.pairs:
            policy.set_gradient_checkpointing(True)
            eng.release()                                       # the 22-pair arenas and workspaces go back to the allocator
            torch.cuda.empty_cache()
            big = [synth_pairs(d, n, q_len, t_len, seed=100, device=dev)]
            block(True, big)                                    # allocator and workspaces at this size
            ms, pk = block(True, big)
            fit.update(predicted_GB=(fixed + per_pair * n) / 1e9, ms_per_step=ms, ms_per_pair=ms / n, ms_per_pair_at_base_pairs_off=med[False] / a.pairs,
                       hbm_peak_allocated_GB=pk / 1e9)
        out["largest_fit_on"] = fit
    print(json.dumps(out), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
