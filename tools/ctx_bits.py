#!/usr/bin/env python3
"""Fingerprint of what the context engine (csrc/ctx.hip) computes, for whichever library OPADPO_LIB_PATH selects: one SHA-256 (its first 128 bits) per result and
opadpo_ctx_bytes_peak per pass.  Run it once per library (tools/build_prev.sh builds the other one) in separate processes and diff the outputs:
a change that only re-arranges the host-side sequencing must leave every line as it was.

    python tools/ctx_bits.py > tree.txt;  OPADPO_LIB_PATH=$PWD/opa-dpo_amd/lib/libopadpo_hip_prev.so python tools/ctx_bits.py > parent.txt

Covers the two geometries and nine variants of tests/test_grad_checkpoint_gpu.py, resident and checkpointed (log-probs, entropies, flat LoRA gradient,
d_feats of the SFT variant), a merged-adapter no-grad pass, a LoRA sampling rollout of 4 rows, a merged-adapter rollout of 16 rows (the <= 64-token
decode GEMMs) and a 2-beam decode.  The gradients flush through the ordered reduce (asserted), so two runs of one library print the same lines.
"""
import hashlib
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "opa-dpo_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)
import test_grad_checkpoint_gpu as G  # noqa: E402


def sha(t):
    return "-" if t is None else hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()[:32]


def training(name, m):
    for variant, kw in G.VARIANTS.items():
        for on in (False, True):
            r = G._pass(m, on, **kw)
            assert r["det"] == 1, (name, variant, on, r["det"])
            print(f"{name} {variant} {'ckpt' if on else 'resident'} logp {sha(r['logp'])} ent {sha(r['ent'])} grad {sha(r['grad'])} "
                  f"d_feats {sha(r['d_feats'])} peak {r['peak']}", flush=True)


def inference(name, m):
    from opadpo_amd.ctx import CtxEngine
    from opadpo_amd.generate import Generator
    from opadpo_amd.model import LoraAdapter
    from opadpo_amd.policy import AutoregressivePolicy
    d, dev, x = m.d, m.dev, m.inputs
    eng = CtxEngine(m.base)
    lora = LoraAdapter(d, m.lora, dev, trainable=False)
    merged = LoraAdapter(d, m.lora, dev, trainable=False)
    merged.merge_into_base(m.base)
    # merged-adapter no-grad pass
    pol = AutoregressivePolicy(eng, merged, m.T)
    keys, batch = pol.build_batch(x.queries, x.qmask, x.resp)
    feats = eng.encode_images(x.images.to(dev))
    with torch.no_grad():
        logp, ent, _ = eng.seq_logprobs_fwd(merged, batch, feats, 1.0, train=False)
    torch.cuda.synchronize()
    print(f"{name} merged_nograd logp {sha(logp)} ent {sha(ent)} peak {G._peak(eng)}", flush=True)
    # rollouts: 4 rows through the LoRA tails, 16 rows on the merged copy, 2 beams
    g = torch.Generator().manual_seed(9)
    for tag, ad, B, beams in (("rollout_lora_4", lora, 4, 1), ("rollout_merged_16", merged, 16, 1), ("beam_lora_2x2", lora, 2, 2)):
        images = torch.randn(B, 3, d.image_size, d.image_size, generator=g).to(torch.bfloat16)
        queries = torch.randint(3, d.vocab, (B, m.Q), generator=g)
        qmask = torch.ones(B, m.Q, dtype=torch.bool)
        queries[0, :2], qmask[0, :2] = 0, False
        queries[:, 5] = -200
        gen = Generator(eng, ad, use_graph=False)
        f = eng.encode_images(images.to(dev))
        if beams > 1:
            tok, sc = eng.generate_beams(gen.adapter, queries, qmask, f, num_beams=beams, max_new_tokens=8, eos_token_id=2, pad_token_id=0, use_graph=False)
        else:
            tok, sc = gen.generate(queries, qmask, image_feats=f, max_new_tokens=8, temperature=0.9, top_k=50, top_p=0.95, seed=1234), None
        torch.cuda.synchronize()
        print(f"{name} {tag} tokens {sha(tok)} scores {sha(sc)} peak {G._peak(eng)}", flush=True)
    eng.close()


def main():
    print("library", os.path.basename(os.environ.get("OPADPO_LIB_PATH") or "libopadpo_hip.so"), file=sys.stderr)
    for name in G.GEOM:
        m = G._model(name)
        training(name, m)
        inference(name, m)


if __name__ == "__main__":
    main()
