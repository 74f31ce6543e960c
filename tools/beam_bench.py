#!/usr/bin/env python3
"""Beam search against sampling decode at equal rows on one MI355X: LLaVA-1.5-7B synthetic weights, Q = 64 text tokens + the image
(Lp = 639), max_new_tokens 64 and 256, B*k in {4, 8, 16}.  Both runs in one process, alternated in blocks after a warm-up; EOS is
never produced (eos id -1 / suppressed), so every run decodes max_new_tokens steps.
Prints one JSON line per (rows, max_new): ms per decode step of each, their ratio, and the prefill time (one prefill per question for the
beams against k copies of the prompt for sampling).  --trace: one further run of this tool under `rocprofv3 --kernel-trace --stats`
(a child process) and the per-step time of beam_topk, beam_update and the beam attention from its kernel statistics."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "opa-dpo_amd"))
from opadpo_amd import lib as L  # noqa: E402
from opadpo_amd.ctx import CtxEngine  # noqa: E402
from opadpo_amd.dims import LlavaDims  # noqa: E402
from opadpo_amd.model import BaseWeights  # noqa: E402
from opadpo_amd.synth import init_weights, synth_pairs  # noqa: E402

SHAPES = ((1, 4), (1, 8), (2, 8))          # (questions, beams): 4, 8, 16 rows


def _time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def run(news, blocks, shapes):
    L.load()
    dev = torch.device("cuda:0")
    d = LlavaDims.llava15_7b()
    eng = CtxEngine(BaseWeights(d, init_weights(d, seed=0, device=dev), dev, need_backward=False))
    results = []
    for B, k in shapes:
        p = synth_pairs(d, B * k, 64, 8, seed=0, device=dev)
        feats = eng.encode_images(p["images"][:B])
        q, m = p["queries"][:B], p["queries_attn_masks"][:B]
        qk, mk, fk = q.repeat_interleave(k, 0), m.repeat_interleave(k, 0), feats.repeat_interleave(k, 0)

        def beam(n):
            eng.generate_beams(None, q, m, feats, num_beams=k, max_new_tokens=n, eos_token_id=-1, pad_token_id=0, use_graph=False)

        def samp(n):
            eng.generate(None, qk, mk, fk, max_new_tokens=n, temperature=1.0, top_k=30, top_p=0.95, seed=1, eos_token_id=2, pad_token_id=0,
                         suppress_eos=True, use_graph=False)

        for n in news:
            beam(n); samp(n)                                    # warm-up
            t = {"beam1": [], "beamn": [], "samp1": [], "sampn": []}
            for _ in range(blocks):                             # alternate the two in blocks
                t["beam1"].append(_time(lambda: beam(1))); t["beamn"].append(_time(lambda: beam(n)))
                t["samp1"].append(_time(lambda: samp(1))); t["sampn"].append(_time(lambda: samp(n)))
            med = {kk: sorted(v)[len(v) // 2] for kk, v in t.items()}
            b_step = (med["beamn"] - med["beam1"]) / (n - 1) * 1e3
            s_step = (med["sampn"] - med["samp1"]) / (n - 1) * 1e3
            r = {"questions": B, "beams": k, "rows": B * k, "max_new": n, "beam_ms_per_step": b_step, "sample_ms_per_step": s_step,
                 "beam_over_sample": b_step / s_step, "beam_prefill_ms": med["beam1"] * 1e3, "sample_prefill_ms_k_copies": med["samp1"] * 1e3}
            print(json.dumps(r), flush=True)
            results.append(r)
    return results


def trace():
    """one run under rocprofv3 (a child process) -> us per decode step of the beam kernels"""
    out = tempfile.mkdtemp(prefix="beam_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "beam", "--", sys.executable, os.path.abspath(__file__), "--news", "64",
           "--blocks", "1", "--shapes", "1x4"]
    subprocess.run(cmd, check=True)
    stats = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    rows = list(csv.DictReader(open(stats[0]))) if stats else []
    found = {}                                                  # per decode step: one beam_topk / beam_update, one attention per layer
    per_step = {"beam_topk": 1, "beam_update": 1, "BeamDec": LlavaDims.llava15_7b().n_layers}
    for r in rows:
        name = r.get("Name", "")
        for key, n in per_step.items():
            if key in name:
                found[key] = found.get(key, 0.0) + float(r["TotalDurationNs"]) / float(r["Calls"]) / 1e3 * n
    print(json.dumps({"trace": "rocprofv3 --kernel-trace --stats", "us_per_beam_step": found}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--news", default="64,256")
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(f"{b}x{k}" for b, k in SHAPES))
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--json", default=None, help="also write the result lines to this file")
    a = ap.parse_args()
    if a.trace:
        trace()
        return
    shapes = [tuple(int(x) for x in s.split("x")) for s in a.shapes.split(",")]
    res = run([int(x) for x in a.news.split(",")], a.blocks, shapes)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
