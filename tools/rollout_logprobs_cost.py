#!/usr/bin/env python3
"""Cost of armed per-token log-probs (CtxEngine.generate(output_logprobs=True)) per decode step on one MI355X: LLaVA-1.5-7B synthetic weights,
adapter-free context engine, query 128, --new generated tokens with EOS suppressed (every step of every row runs), the rollout's sampling
(temperature 1.0, top_k 30, top_p 0.95).  The same process generates unarmed and armed (one more launch per step: token_logprob_kernel, one
1024-thread workgroup per row over the fp32 logits row the sampler just read) in alternating blocks after a warm-up of both, with plain launches
and under graph replay; one JSON line per (row count, launch form): median ms per generated token of each and the difference."""
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
from opadpo_amd.model import BaseWeights  # noqa: E402
from opadpo_amd.synth import init_weights, synth_pairs  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="7b", choices=["7b", "tiny"])
    ap.add_argument("--batches", default="8,64,256")
    ap.add_argument("--new", type=int, default=128, help="generated tokens per call")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=1, help="generations per block")
    ap.add_argument("--graph", default="0,1", help="launch forms to measure: 0 plain launches, 1 replay of the captured step")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    L.load()
    dev = torch.device("cuda:0")
    d = LlavaDims.llava15_7b() if a.model == "7b" else LlavaDims.tiny()
    q_len = 128 if a.model == "7b" else 16
    eng = CtxEngine(BaseWeights(d, init_weights(d, seed=0, device=dev), dev, need_backward=False))
    for B in [int(x) for x in a.batches.split(",")]:
        p = synth_pairs(d, B, q_len, 8, seed=B, device=dev)
        feats = eng.encode_images(p["images"])
        for graph in [int(x) for x in a.graph.split(",")]:

            def block(armed):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(a.calls):
                    eng.generate(None, p["queries"], p["queries_attn_masks"], feats, max_new_tokens=a.new, temperature=1.0, top_k=30, top_p=0.95, seed=i,
                                 eos_token_id=2, pad_token_id=0, suppress_eos=True, use_graph=bool(graph), output_logprobs=armed)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / (a.calls * a.new) * 1e3

            block(False); block(True)                                  # warm-up of both forms
            t = {False: [], True: []}
            for _ in range(a.blocks):                                   # alternate the two in blocks
                for armed in (False, True):
                    t[armed].append(block(armed))
            med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
            out = {"metric": "generation with output_logprobs vs without, same process, alternating blocks; ms per generated token (prefill included)",
                   "model": a.model, "rows": B, "query_len": q_len, "new_tokens": a.new, "use_graph": graph, "ms_per_token_unarmed": med[False],
                   "ms_per_token_armed": med[True], "extra_us_per_step": (med[True] - med[False]) * 1e3, "extra_fraction": med[True] / med[False] - 1.0,
                   "blocks_unarmed_ms": t[False], "blocks_armed_ms": t[True]}
            line = json.dumps(out)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
