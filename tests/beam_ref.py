"""Test-side restatement of HF beam search: transformers GenerationMixin._beam_search with do_sample=False, num_return_sequences=1,
length_penalty=1.0 and early_stopping=False (what eval_llava_rlhf_coco/model_vqa.py ends up with).

Per step t (0-based, t < max_new):
  scores  = log_softmax(logits) (fp32) + running beam score; at t = 0 only beam 0 is live (the others start at -1e9);
  top 2k of the k*V scores of an item, descending (distinct scores: the order is unique; the kernels break ties to the lower
  flat index beam*V + token);
  a candidate is finished if its token is EOS or t = max_new - 1; finished candidates ranked among the first k enter the item's
  best-k finished set with score / (t + 1) (generated length, EOS included) - unless the item's early-stop flag has dropped;
  the next running beams are the best k of the candidates, the finished ones pushed down by -1e9;
  early-stop flag: stays up while the finished set is not full or best running score / (t + 1) > worst finished score;
  generation stops when no flag is up or at max_new.
The result per item is the best finished hypothesis: tokens [max_new] (EOS kept, pad after it) and its score.
"""
from __future__ import annotations

import torch

NEG = -1.0e9


class BeamSearch:
    """Step-by-step state of a batched beam search over B items x k beams (rows b*k + j)."""

    def __init__(self, B: int, k: int, V: int, max_new: int, eos_id: int, pad_id: int):
        self.B, self.k, self.V, self.max_new, self.eos, self.pad = B, k, V, max_new, eos_id, pad_id
        self.t = 0
        self.run = torch.zeros(B, k)
        self.run[:, 1:] = NEG
        self.seq = torch.full((B, k, max_new), pad_id, dtype=torch.int64)       # running hypotheses
        self.fin_score = torch.full((B, k), NEG)
        self.fin_seq = torch.full((B, k, max_new), pad_id, dtype=torch.int64)
        self.fin_ok = torch.zeros(B, k, dtype=torch.bool)
        self.unsat = torch.ones(B, dtype=torch.bool)                             # HF is_early_stop_heuristic_unsatisfied
        self.stopped = False
        self.parents = None            # [B, k] parent ROW (b*k + beam) of each new running beam
        self.tokens = None             # [B, k] its newest token
        self.margin = float("inf")     # smallest gap between consecutive candidate scores seen (decision margin)

    @property
    def done(self) -> torch.Tensor:
        """per item: nothing can change its result any more (early stop) or the last step ran"""
        return ~self.unsat | (self.t >= self.max_new)

    def step(self, logits: torch.Tensor) -> None:
        B, k, V, t = self.B, self.k, self.V, self.t
        lp = torch.log_softmax(logits.float().view(B * k, V), dim=-1).view(B, k, V) + self.run[:, :, None]
        topv, topi = torch.topk(lp.reshape(B, k * V), 2 * k)
        live = self.unsat
        if live.any():
            gaps = (topv[live, :-1] - topv[live, 1:]).min()
            self.margin = min(self.margin, float(gaps))
        par, tok = topi // V, topi % V
        cand = torch.gather(self.seq, 1, par[:, :, None].expand(B, 2 * k, self.max_new)).clone()
        cand[:, :, t] = tok
        hit = (tok == self.eos) | (t == self.max_new - 1)
        run_lp = topv + hit.float() * NEG
        nxt = torch.topk(run_lp, k)[1]
        self.seq = torch.gather(cand, 1, nxt[:, :, None].expand(B, k, self.max_new))
        self.run = torch.gather(run_lp, 1, nxt)
        self.parents = torch.gather(par, 1, nxt) + torch.arange(B)[:, None] * k
        self.tokens = torch.gather(tok, 1, nxt)
        did = hit & (torch.arange(2 * k) < k)[None, :]
        fs = topv / float(t + 1)
        fs = fs + (~self.unsat[:, None]).float() * NEG
        fs = fs + (~did).float() * NEG
        m_score = torch.cat([self.fin_score, fs], 1)
        m_seq = torch.cat([self.fin_seq, cand], 1)
        m_ok = torch.cat([self.fin_ok, did], 1)
        sel = torch.topk(m_score, k)[1]
        self.fin_score = torch.gather(m_score, 1, sel)
        self.fin_seq = torch.gather(m_seq, 1, sel[:, :, None].expand(B, k, self.max_new))
        self.fin_ok = torch.gather(m_ok, 1, sel)
        self.t = t + 1
        best = self.run[:, :1] / float(self.t)
        worst = torch.where(self.fin_ok, self.fin_score.min(1, keepdim=True)[0], torch.full_like(self.fin_score, NEG))
        self.unsat = self.unsat & (best > worst).any(-1)
        self.stopped = not bool(self.unsat.any()) or bool(hit.all()) or self.t >= self.max_new

    def result(self):
        """-> (tokens [B, max_new] int64, scores [B] fp32) of the best finished hypothesis per item"""
        return self.fin_seq[:, 0].clone(), self.fin_score[:, 0].clone()


def beam_search(step_logits_fn, B: int, k: int, V: int, max_new: int, eos_id: int, pad_id: int):
    """step_logits_fn(tokens [B*k, t] int64) -> logits [B*k, V] of the next token of every running hypothesis.
    -> (tokens [B, max_new], scores [B], the BeamSearch state)."""
    bs = BeamSearch(B, k, V, max_new, eos_id, pad_id)
    while not bs.stopped:
        logits = step_logits_fn(bs.seq[:, :, :bs.t].reshape(B * k, bs.t))
        bs.step(logits)
    tokens, scores = bs.result()
    return tokens, scores, bs
