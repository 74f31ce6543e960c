#!/usr/bin/env python3
"""Continuous batching for the rollout (CtxEngine.generate_continuous) against the static rollout (CtxEngine.generate) on one MI355X: LLaVA-1.5-7B
synthetic weights, adapter-free context engine, query 128, EOS suppressed (a prompt generates exactly its cap), the rollout's sampling
(temperature 1.0, top_k 30, top_p 0.95), plain launches.  Both forms run in the same process in alternating blocks after a warm-up of both.
One JSON line per case:

  step      S = N prompts with every cap = --new: a session without a single refill against a static batch of S rows; ms per generated token
            of each, every block's figure, and the block-to-block spread of the static one - the margin the difference is read against.
  refill    --prompts prompts through --slots slots with caps up to --cap-max from two seeded distributions written out below (uniform on
            32..cap-max; skewed: four in five short, 16..cap-max/8, one in twenty at the cap, the rest uniform) against static chunks of --slots
            prompts, each run to its own chunk's longest cap; useful tokens (sum of the caps) per second of each and the decode steps
            generate.plan_continuous predicts for both."""
import argparse
import json
import os
import random
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "opa-dpo_amd"))
from opadpo_amd import lib as L  # noqa: E402
from opadpo_amd.ctx import CtxEngine  # noqa: E402
from opadpo_amd.dims import LlavaDims  # noqa: E402
from opadpo_amd.generate import plan_continuous  # noqa: E402
from opadpo_amd.model import BaseWeights  # noqa: E402
from opadpo_amd.synth import init_weights, synth_pairs  # noqa: E402

SAMPLING = dict(temperature=1.0, top_k=30, top_p=0.95, eos_token_id=2, pad_token_id=0, suppress_eos=True, use_graph=False)


def caps_uniform(n, cap_max, seed=1):
    rng = random.Random(seed)
    return [rng.randint(min(32, cap_max), cap_max) for _ in range(n)]


def caps_skewed(n, cap_max, seed=2):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        u = rng.random()
        out.append(rng.randint(min(16, cap_max), max(min(16, cap_max), cap_max // 8)) if u < 0.8 else cap_max if u < 0.85 else rng.randint(min(32, cap_max), cap_max))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="7b", choices=["7b", "tiny"])
    ap.add_argument("--cases", default="step,refill")
    ap.add_argument("--batches", default="8,64,256", help="step case: slot counts")
    ap.add_argument("--new", type=int, default=129, help="step case: generated tokens per prompt; (new - 1) % check_every == 0 gives both forms the same step count")
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--prompts", type=int, default=256, help="refill case: prompts")
    ap.add_argument("--slots", type=int, default=64, help="refill case: slots / static chunk size")
    ap.add_argument("--cap-max", type=int, default=896, help="refill case: max_new_tokens")
    ap.add_argument("--refill-blocks", type=int, default=1)
    ap.add_argument("--check-every", type=int, default=32)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    L.load()
    dev = torch.device("cuda:0")
    d = LlavaDims.llava15_7b() if a.model == "7b" else LlavaDims.tiny()
    q_len = 128 if a.model == "7b" else 16
    eng = CtxEngine(BaseWeights(d, init_weights(d, seed=0, device=dev), dev, need_backward=False))

    def emit(out):
        line = json.dumps(out)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def alternate(static, cont, blocks):
        static(); cont()                                            # warm-up of both forms
        t = {"static": [], "continuous": []}
        for _ in range(blocks):
            t["static"].append(timed(static))
            t["continuous"].append(timed(cont))
        return t

    med = lambda v: sorted(v)[len(v) // 2]
    cases = a.cases.split(",")
    if "step" in cases:
        for S in [int(x) for x in a.batches.split(",")]:
            p = synth_pairs(d, S, q_len, 8, seed=S, device=dev)
            feats = eng.encode_images(p["images"])
            static = lambda: eng.generate(None, p["queries"], p["queries_attn_masks"], feats, max_new_tokens=a.new, seed=0, **SAMPLING)
            cont = lambda: eng.generate_continuous(None, p["queries"], p["queries_attn_masks"], feats, slots=S, max_new_tokens=a.new, seed=0,
                                                   check_every=a.check_every, **SAMPLING)
            t = {k: [x / a.new * 1e3 for x in v] for k, v in alternate(static, cont, a.blocks).items()}
            emit({"metric": "continuous session without refills (N = S, every cap = new_tokens) vs static batch, same process, alternating blocks; "
                            "ms per generated token (prefill included)",
                  "case": "step", "model": a.model, "slots": S, "query_len": q_len, "new_tokens": a.new, "check_every": a.check_every,
                  "steps_static": a.new - 1, "steps_continuous": plan_continuous([a.new] * S, S, a.check_every)[1],
                  "ms_per_token_static": med(t["static"]), "ms_per_token_continuous": med(t["continuous"]),
                  "difference_fraction": med(t["continuous"]) / med(t["static"]) - 1.0,
                  "static_block_spread_fraction": (max(t["static"]) - min(t["static"])) / med(t["static"]),
                  "blocks_static_ms": t["static"], "blocks_continuous_ms": t["continuous"]})
            del p, feats
            torch.cuda.empty_cache()
    if "refill" in cases:
        N, S, T = a.prompts, a.slots, a.cap_max
        p = synth_pairs(d, N, q_len, 8, seed=N, device=dev)
        feats = torch.cat([eng.encode_images(p["images"][i:i + 64]) for i in range(0, N, 64)])
        for name, caps in (("uniform", caps_uniform(N, T)), ("skewed", caps_skewed(N, T))):
            chunks = [list(range(c0, min(N, c0 + S))) for c0 in range(0, N, S)]

            def static():
                for idx in chunks:
                    eng.generate(None, p["queries"][idx[0]:idx[-1] + 1], p["queries_attn_masks"][idx[0]:idx[-1] + 1], feats[idx[0]:idx[-1] + 1],
                                 max_new_tokens=max(caps[i] for i in idx), seed=0, **SAMPLING)

            cont = lambda: eng.generate_continuous(None, p["queries"], p["queries_attn_masks"], feats, slots=S, max_new_tokens=T, seed=0,
                                                   max_new_tokens_per_prompt=caps, check_every=a.check_every, **SAMPLING)
            t = alternate(static, cont, a.refill_blocks)
            useful = sum(caps)
            emit({"metric": "continuous session vs static chunks run to their own longest cap, same process, alternating blocks; useful tokens "
                            "(sum of the caps) per second, prefills included",
                  "case": "refill", "caps": name, "model": a.model, "prompts": N, "slots": S, "query_len": q_len, "max_new_tokens": T,
                  "check_every": a.check_every, "useful_tokens": useful, "cap_mean": useful / N, "caps_at_max": sum(c == T for c in caps),
                  "steps_static_predicted": sum(max(caps[i] for i in idx) - 1 for idx in chunks),
                  "steps_continuous_predicted": plan_continuous(caps, S, a.check_every)[1],
                  "tokens_per_s_static": useful / med(t["static"]), "tokens_per_s_continuous": useful / med(t["continuous"]),
                  "speedup": med(t["static"]) / med(t["continuous"]), "blocks_static_s": t["static"], "blocks_continuous_s": t["continuous"]})


if __name__ == "__main__":
    main()
