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
Prints one JSON line."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="7b", choices=["7b", "tiny"])
    ap.add_argument("--pairs", type=int, default=22)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3, help="steps per block")
    ap.add_argument("--hbm-fraction", type=float, default=0.9, help="largest-fit trial: predicted footprint must stay under this share of the device memory")
    ap.add_argument("--max-pairs", type=int, default=32, help="upper end of the largest-fit trial (0: skip the trial).  Default 32: from 34 pairs the "
                    "padded gate|up activation of 7B ([rows, 2 x 11008] bf16) passes 2^31 bytes, a size no test of the kernels has run at")
    ap.add_argument("--json", default=None, help="also write the result to this file")
    a = ap.parse_args()
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
