"""Float64 numpy restatement of the rollout's per-token log-probs and entropies (opadpo_token_logprobs, opadpo_ctx_set_output_logprobs).

The input is the fp32 product the kernel forms, z = fp32(logits * fp32(inv_T)) (`scaled`), so what is compared is the arithmetic after that one
multiply.  Columns with z = -inf are dropped (they carry no mass); a row whose token is pad reads logp = -0.0, ent = 0 (the trainer's value-based pad
rule); the token of a non-pad row must be a finite column."""
import numpy as np


def scaled(logits: np.ndarray, temperature: float) -> np.ndarray:
    """fp32(logits * fp32(1 / temperature)), the reciprocal itself formed in fp32; temperature 0 (greedy) reads with inv_T = 1"""
    logits = np.asarray(logits, dtype=np.float32)
    inv = np.float32(1.0) if temperature == 0 else np.float32(1.0) / np.float32(temperature)
    return (logits * inv).astype(np.float32)


def token_logprobs(z: np.ndarray, tokens, pad_id: int = 0):
    """z fp32 [rows, V], tokens [rows] -> (logp, ent) float64 [rows]: logp = z[tok] - lse(z), ent = lse(z) - sum softmax(z) * z"""
    z = np.asarray(z)
    assert z.dtype == np.float32 and z.ndim == 2
    tokens = np.asarray(tokens).reshape(-1)
    rows = z.shape[0]
    logp, ent = np.zeros(rows, dtype=np.float64), np.zeros(rows, dtype=np.float64)
    for r in range(rows):
        t = int(tokens[r])
        if t == pad_id:
            logp[r] = -0.0
            continue
        row = z[r].astype(np.float64)
        assert np.isfinite(row[t]), "the token sits on a -inf column"
        x = row[~np.isneginf(row)]
        assert np.isfinite(x).all() and x.size > 0
        m = x.max()
        e = np.exp(x - m)
        se = e.sum()
        lse = m + np.log(se)
        logp[r] = row[t] - lse
        ent[r] = np.log(se) - (e * (x - m)).sum() / se          # = lse - sum p * x, without cancelling at the magnitude of x
    return logp, ent
