#!/usr/bin/env python3
"""Cost of LoRA dropout in the trainer step of the benchmark shape on one MI355X: LLaVA-1.5-7B synthetic weights, LoRA r = 256, 22 packed
(chosen, rejected) pairs of query 128 + response 384 on ragged rows, frozen reference merged - the step bench.py times (reference pass, policy
forward, pair loss, LoRA backward, clip + AdamW).  The same process runs the step at p = 0 and p = --rate in alternating blocks after a
warm-up of both; prints one JSON line: median ms per step of each and the difference."""
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
    ap.add_argument("--rate", type=float, default=0.05)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3, help="steps per block")
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

    def step(b):
        feats = eng.encode_images(b["images"])
        kw = dict(queries=b["queries"], queries_attn_masks=b["queries_attn_masks"], image_feats=feats, chosen_response=b["chosen"],
                  rejected_response=b["rejected"], row_lead=b["row_lead"], row_lens=b["row_lens"])
        with torch.no_grad():
            r = ref_policy(**kw)
        o = policy(**kw)
        loss, _, _ = pair_loss(largs, o["chosen_response_logprobs"], o["rejected_response_logprobs"], r["chosen_response_logprobs"],
                               r["rejected_response_logprobs"])
        loss.backward()
        opt.step()
        opt.zero_grad()
        pol_ad.refresh_transposed()

    def block(rate):
        policy.set_lora_dropout(rate, seed=1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for b in pool:
            step(b)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / len(pool) * 1e3

    block(0.0); block(a.rate)                                   # warm-up of both forms (allocator, workspaces)
    t = {0.0: [], a.rate: []}
    for _ in range(a.blocks):                                   # alternate the two in blocks
        for rate in (0.0, a.rate):
            t[rate].append(block(rate))
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    out = {"metric": "trainer step with LoRA dropout vs without, same process, alternating blocks", "model": a.model, "pairs": a.pairs,
           "rate": a.rate, "ms_per_step_p0": med[0.0], "ms_per_step_p": med[a.rate], "extra_ms": med[a.rate] - med[0.0],
           "extra_fraction": med[a.rate] / med[0.0] - 1.0, "blocks_p0_ms": t[0.0], "blocks_p_ms": t[a.rate],
           "hbm_peak_allocated_GB": torch.cuda.max_memory_allocated() / 1e9}
    print(json.dumps(out), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
