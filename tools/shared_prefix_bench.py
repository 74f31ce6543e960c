#!/usr/bin/env python3
"""n sampled responses per prompt (num_return_sequences) on one MI355X: LLaVA-1.5-7B synthetic weights, Q = 128 (prefix Lp = 703), three legs of the
same items x n rows in ONE process, in alternating blocks (other work shares the machine: a difference only counts against the spread of the blocks):

  repeated  generate(queries.repeat_interleave(n, 0), ...) - the existing path and the yardstick: n prefills and n prefix caches per prompt
  per_row   generate(..., num_return_sequences=n), context flag bit 15 - one prefill and one prefix cache per prompt, decode attention per row
  grouped   generate(..., num_return_sequences=n) - the same layout, the prefix read once per item (opadpo_attn_decode_shared form 2)

Per leg and size: prefill ms (a 1-token generation), ms per decode step, tokens/s and the context's peak arena bytes.  SPB_SIZES = items x n x new
tokens, comma separated (default: 8x8x64,8x8x896,16x16x64); SPB_BLOCKS = alternating blocks (default 3).  Writes profiles/shared_prefix_bench_7b.json
(SPB_OUT overrides; SPB_MODEL=tiny is a rehearsal of the plumbing, its numbers are launch overhead).  SPB_LEG = one leg only, one block, no file: the
form to run under a kernel trace collected on its own."""
import json
import os
import socket
import subprocess
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "opa-dpo_amd"))
from opadpo_amd import lib as L  # noqa: E402
from opadpo_amd.ctx import CtxEngine  # noqa: E402
from opadpo_amd.dims import LlavaDims  # noqa: E402
from opadpo_amd.generate import Generator  # noqa: E402
from opadpo_amd.model import BaseWeights  # noqa: E402
from opadpo_amd.synth import init_weights, synth_pairs  # noqa: E402

LEGS = ("repeated", "per_row", "grouped")
PER_ROW = 1 | (1 << 15)


def run_leg(eng, gen, leg, p, feats, n, new_tokens, seed):
    """-> seconds of one generation of items x n rows (synchronised)"""
    kw = dict(max_new_tokens=new_tokens, top_k=30, top_p=0.95, seed=seed, suppress_eos=True)
    eng.set_flags(use_tr=PER_ROW) if leg == "per_row" else eng.set_flags()
    if leg == "repeated":                                   # the repeated tensors are built outside the timed window
        q, m, f = p["queries"].repeat_interleave(n, 0), p["queries_attn_masks"].repeat_interleave(n, 0), feats.repeat_interleave(n, 0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if leg == "repeated":
        gen.generate(q, m, image_feats=f, **kw)
    else:
        gen.generate(p["queries"], p["queries_attn_masks"], image_feats=feats, num_return_sequences=n, **kw)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    eng.set_flags()
    return dt


def main():
    L.load()
    dev = torch.device("cuda:0")
    model = os.environ.get("SPB_MODEL", "7b")
    d = LlavaDims.llava15_7b() if model == "7b" else LlavaDims.tiny()
    Q = 128 if model == "7b" else 16
    sizes = [tuple(int(x) for x in s.split("x")) for s in os.environ.get("SPB_SIZES", "8x8x64,8x8x896,16x16x64").split(",")]
    one_leg = os.environ.get("SPB_LEG")
    legs = (one_leg,) if one_leg else LEGS
    blocks = 1 if one_leg else int(os.environ.get("SPB_BLOCKS", 3))
    base = BaseWeights(d, init_weights(d, seed=0, device=dev), dev, need_backward=False)
    eng = CtxEngine(base)
    gen = Generator(eng, None, fuse_swiglu=True)
    results = []
    for items, n, new_tokens in sizes:
        p = synth_pairs(d, items, Q, 8, seed=0, device=dev)
        feats = eng.encode_images(p["images"])
        peak = {}
        for leg in legs:      # the arena peak of the leg alone: a context of its own (the weights, gen.adapter's fused gate|up copy included, are borrowed)
            eng1 = CtxEngine(base)
            run_leg(eng1, Generator(eng1, gen.adapter), leg, p, feats, n, new_tokens, 1)      # full length: the suffix caches are carved at begin
            peak[leg] = int(eng1._lib.opadpo_ctx_bytes_peak(eng1.ctx))
            eng1.release()
            eng1.close()
        for leg in legs:                                    # warm-up of every shape of the timed window
            run_leg(eng, gen, leg, p, feats, n, 1, 1)
            run_leg(eng, gen, leg, p, feats, n, min(new_tokens, 4), 1)
        t = {leg: {"prefill": [], "full": []} for leg in legs}
        for b in range(blocks):
            for leg in legs:
                t[leg]["prefill"].append(run_leg(eng, gen, leg, p, feats, n, 1, 2 + b))
                t[leg]["full"].append(run_leg(eng, gen, leg, p, feats, n, new_tokens, 2 + b))
        for leg in legs:
            pre, full = min(t[leg]["prefill"]), min(t[leg]["full"])
            step = (full - pre) / (new_tokens - 1)
            results.append({"items": items, "n": n, "rows": items * n, "new_tokens": new_tokens, "leg": leg, "prefill_ms": pre * 1e3,
                            "decode_ms_per_step": step * 1e3, "tokens_per_s": items * n / step, "arena_peak_bytes": peak[leg],
                            "full_s_blocks": t[leg]["full"], "prefill_s_blocks": t[leg]["prefill"]})
            print(json.dumps(results[-1]), flush=True)
    if one_leg:
        return
    try:
        commit = subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    out = {"tool": "tools/shared_prefix_bench.py", "model": model, "Q": Q, "Lp": Q + d.n_patches - 1, "blocks": blocks, "host": socket.gethostname(),
           "device": torch.cuda.get_device_name(0), "commit": commit, "note": "best of the alternating blocks per leg; arena_peak_bytes = opadpo_ctx_bytes_peak of a "
           "fresh context that ran the leg once at the full length (KV caches + decode buffers + prefill scratch)", "results": results}
    path = os.environ.get("SPB_OUT", os.path.join(REPO, "profiles", "shared_prefix_bench_7b.json"))
    json.dump(out, open(path, "w"), indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
