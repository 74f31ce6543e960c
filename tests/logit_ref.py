"""CPU restatement of the scores HF's `generate(do_sample=True, output_scores=True, sequence_bias=...)` records for a step, written from the
HF semantics (transformers `SequenceBiasLogitsProcessor` with one-token sequences, then `TemperatureLogitsWarper`, `TopKLogitsWarper`,
`TopPLogitsWarper`, in that order: logits processors run before the warpers):

    s = logits + bias                          (fp32 add, on the biased tokens only)
    s = s / temperature                        (fp32 divide)
    top-k: s[s < k-th largest s] = -inf        (ties with the k-th value stay; k = min(top_k, V); 0 = off)
    top-p: sort ascending, p = softmax(s), cut where cumsum(p) <= 1 - top_p, never the last (largest) one; 1.0 = off

temperature == 0 is this tree's greedy decoding (HF would refuse it with do_sample=True): the scores are logits + bias, nothing cut.
The values at the kept entries are exactly the fp32 add and divide.  The top-p DECISION is taken on a float64 softmax: `top_p_margin`
returns how far the closest cumulative mass is from the cut, so a test can tell a clear decision from a rounding coin-flip."""
import numpy as np

NEG_INF = np.float32(-np.inf)


def _biased(logits, bias):
    z = np.array(logits, dtype=np.float32, copy=True)
    if z.ndim == 1:
        z = z[None]
    for t, b in (bias or {}).items():
        z[:, int(t)] = z[:, int(t)] + np.float32(b)
    return z


def _top_k(s, top_k):
    if top_k and top_k > 0:
        k = min(int(top_k), s.shape[-1])
        kth = np.sort(s, axis=-1)[:, -k][:, None]
        s = np.where(s < kth, NEG_INF, s)
    return s


def _top_p_cum(s):
    """ascending order of every row and the float64 cumulative softmax mass in that order"""
    order = np.argsort(s, axis=-1, kind="stable")
    ss = np.take_along_axis(s, order, -1).astype(np.float64)
    p = np.exp(ss - ss[:, -1:])
    p /= p.sum(-1, keepdims=True)
    return order, np.cumsum(p, -1)


def processed_scores(logits, bias=None, temperature=1.0, top_k=0, top_p=1.0):
    """logits [B, V] (or [V]) -> processed scores [B, V] float32; bias = {token id: float} or None."""
    z = _biased(logits, bias)
    if temperature == 0:
        return z
    s = _top_k(z / np.float32(temperature), top_k)
    if top_p is not None and top_p < 1.0:
        order, cum = _top_p_cum(s)
        remove = cum <= 1.0 - top_p
        remove[:, -1] = False
        cut = np.zeros_like(remove)
        np.put_along_axis(cut, order, remove, -1)
        s = np.where(cut, NEG_INF, s)
    return s.astype(np.float32)


def top_p_margin(logits, bias=None, temperature=1.0, top_k=0, top_p=1.0):
    """min over rows and tokens of |cumulative mass - (1 - top_p)|: the distance of the closest top-p decision from a tie (inf when top-p is off)."""
    if temperature == 0 or top_p is None or top_p >= 1.0:
        return float("inf")
    s = _top_k(_biased(logits, bias) / np.float32(temperature), top_k)
    _, cum = _top_p_cum(s)
    return float(np.abs(cum[:, :-1] - (1.0 - top_p)).min())
