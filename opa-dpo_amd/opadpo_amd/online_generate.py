"""One rollout step of the generator stage (host side around the decode kernels): batches of
`rollout_data.QueryResponseDataset` items -> sampled responses -> the column dict that `dataset_build.write_rollout_json`
stores as `step{N}_rank{R}.json`.

Reference behaviour restated (no code shared), opadpo/generator_models/online_generator.py:262-377: per batch sample
`response_len` new tokens (temperature -> top-k -> top-p), cut after EOS / the two question-mark ids, decode responses and
standard responses with special tokens skipped, decode the query with the image placeholder turned into BOS and keep the text
between 'USER:  \\n' and ' ASSISTANT:', ask the feedback model for (pseudo response, generated response, JSON report), and
collect eight equal-length columns.  The GPT-4V feedback client needs the network and is out of scope: `feedback`
is a callable; the default returns empty answers, which the dataset builder's first filter then drops.
"""
from __future__ import annotations

from typing import Callable, Dict, Iterable, List, Optional, Sequence

import torch

from .rollout_data import IMAGE_TOKEN_INDEX

QUESTION_MARK_IDS = (1577, 29973)          # '?' alone and after a newline in the Llama vocabulary (online_generator.py:311-315)
QUERY_HEAD, QUERY_TAIL = "USER:  \n", " ASSISTANT:"
LOGPROB_COLUMNS = ("original_generate_response_logprob", "original_generate_response_tokens", "original_generate_response_entropy")


def no_feedback(images_url: Sequence[str], queries: Sequence[str], responses: Sequence[str], standard: Sequence[str]) -> Dict[str, list]:
    n = len(responses)
    return {"Pseudo_response": [""] * n, "Generated_response": list(responses), "report_json": [""] * n}


def query_text(decoded: str) -> str:
    """Question part of a decoded prompt; `str.find` semantics kept (a missing marker yields -1 like in the reference)."""
    return decoded[decoded.find(QUERY_HEAD) + len(QUERY_HEAD):decoded.find(QUERY_TAIL)]


def decode_batch(tokenizer, ids: torch.Tensor) -> List[str]:
    return tokenizer.batch_decode(ids, skip_special_tokens=True, clean_up_tokenization_spaces=True)


def rollout_step(batches: Iterable[Dict], tokenizer, sample: Callable[[torch.Tensor, torch.Tensor, torch.Tensor], torch.Tensor],
                 feedback: Optional[Callable] = None, num_return_sequences: int = 1) -> Dict[str, list]:
    """`sample(queries, query_attn_masks, images) -> responses [B, response_len]` already cut after EOS / '?' (on the GPU:
    `generator_sampler(...)` below).  Returns the response dict of online_generator.py:352-362.
    num_return_sequences = N > 1 (the reference hard-codes 1): `sample` returns [B * N, response_len], row i * N + j = sample j of query i;
    every query yields N consecutive records, the query-side columns repeated, and `feedback` sees B * N entries.
    A `sample` that returns `(responses, logp, ent)` (`generator_sampler(..., output_logprobs=True)`; logp / ent fp32 of the responses' shape)
    adds three columns per record, taken over the response's non-pad tokens: `original_generate_response_logprob` (sum of the token
    log-probs), `original_generate_response_tokens` (their count) and `original_generate_response_entropy` (mean token entropy, 0.0 for an
    empty response).  Every batch of a step must then return the triple."""
    feedback = feedback or no_feedback
    N = int(num_return_sequences)
    if N < 1:
        raise ValueError(f"num_return_sequences must be >= 1 (got {N})")
    rep = (lambda xs: list(xs)) if N == 1 else (lambda xs: [x for x in xs for _ in range(N)])
    out: Dict[str, list] = {k: [] for k in ("query", "image_id", "standard_response", "original_generate_response",
                                            "AI_generate_response", "AI_pseudo_response", "AI_json_report", "image_bytes")}
    with_lp: Optional[bool] = None
    for batch in batches:
        queries = batch["queries"]
        responses = sample(queries, batch["query_attn_masks"], batch["images"])
        triple = isinstance(responses, (tuple, list))
        if with_lp is None:
            with_lp = triple
            if triple:
                out.update({k: [] for k in LOGPROB_COLUMNS})
        elif with_lp != triple:
            raise ValueError("sample must return responses or (responses, logp, ent) for every batch of a step, not a mix")
        if triple:
            if len(responses) != 3:
                raise ValueError(f"sample returned {len(responses)} values: expected responses or (responses, logp, ent)")
            responses, logp, ent = responses
            if tuple(logp.shape) != tuple(responses.shape) or tuple(ent.shape) != tuple(responses.shape):
                raise ValueError(f"sample returned logp {tuple(logp.shape)} / ent {tuple(ent.shape)} for responses {tuple(responses.shape)}")
        if responses.shape[0] != N * queries.shape[0]:
            raise ValueError(f"sample returned {responses.shape[0]} responses for {queries.shape[0]} queries x {N} return sequences")
        if triple:
            keep = (responses != tokenizer.pad_token_id).cpu()
            count = keep.sum(dim=1)
            lp_sum = (logp.detach().cpu().double() * keep).sum(dim=1)
            ent_sum = (ent.detach().cpu().double() * keep).sum(dim=1)
            out["original_generate_response_logprob"] += [float(v) for v in lp_sum]
            out["original_generate_response_tokens"] += [int(v) for v in count]
            out["original_generate_response_entropy"] += [float(s) / int(c) if int(c) else 0.0 for s, c in zip(ent_sum, count)]
        text_rsp = decode_batch(tokenizer, responses)
        text_std = rep(decode_batch(tokenizer, batch["standard_responses"]))
        shown = queries.clone()
        shown[shown == IMAGE_TOKEN_INDEX] = tokenizer.bos_token_id
        text_q = rep(query_text(q) for q in decode_batch(tokenizer, shown))
        fb = feedback(rep(batch["images_url"]), text_q, text_rsp, text_std)
        if not (len(fb["Pseudo_response"]) == len(fb["Generated_response"]) == len(fb["report_json"]) == len(text_rsp)):
            raise ValueError("feedback must return one entry per response")
        out["query"] += ["<image>\n" + q for q in text_q]
        out["image_id"] += rep(batch["images_path"])
        out["standard_response"] += text_std
        out["original_generate_response"] += text_rsp
        out["AI_generate_response"] += list(fb["Generated_response"])
        out["AI_pseudo_response"] += list(fb["Pseudo_response"])
        out["AI_json_report"] += list(fb["report_json"])
        out["image_bytes"] += rep(batch["images_bytes"])
    return out


def generator_sampler(generator, *, response_len: int, temperature: float = 1.0, top_k: int = 30, top_p: float = 0.95,
                      seed: int = 0, num_return_sequences: int = 1, output_logprobs: bool = False, continuous_slots: int = 0) -> Callable:
    """Sampler over the HIP decode path (`generate.Generator.rollout`); a new seed per batch.  Build the generator with
    `merge_adapter=True` (frozen rollout adapter) or `fuse_swiglu=True` (adapter-free rollout) for the fastest decode step.
    num_return_sequences = N > 1: N responses per query off one prefill, [B * N, response_len] item-major (pass the same N to `rollout_step`).
    output_logprobs: the sampler returns (responses, logp, ent) - `Generator.rollout(..., output_logprobs=True)` - and `rollout_step` adds
    the per-response log-prob / token count / mean entropy columns.
    continuous_slots = S > 0: every call runs its queries - hand it a rollout step's whole batch - through one continuous session of S decode
    slots (`Generator.rollout(..., continuous_slots=S)`); not with num_return_sequences > 1."""
    extra = {} if num_return_sequences == 1 else dict(num_return_sequences=int(num_return_sequences))
    if continuous_slots:
        extra["continuous_slots"] = int(continuous_slots)
    if output_logprobs:
        extra["output_logprobs"] = True
    state = {"n": 0}

    def sample(queries, masks, images):
        state["n"] += 1
        dev = generator.engine.dev
        got = generator.rollout(queries.to(dev), masks.to(dev), images.to(dev), response_len=response_len, temperature=temperature,
                                top_k=top_k, top_p=top_p, seed=seed + state["n"], additional_stop_ids=QUESTION_MARK_IDS, **extra)
        return tuple(t.cpu() for t in got) if output_logprobs else got.cpu()
    return sample
