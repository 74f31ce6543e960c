"""Float64 reference of the flash-attention kernels (opadpo_attn_fwd / _bwd and the ragged form opadpo_ctx runs), computed from the
bf16 values the kernel read.

Rows are flat, as in the kernels: q, k, v, dO and O are [rows, nh * hd] and a `Layout` says which rows form which sequence.
  - padded: S sequences of L rows each (sequence s = rows s*L ..), optionally packed as [prefix | response 0 | response 1 | ...]
    with responses of seg_len positions after seg_prefix;
  - ragged: sequence s occupies rows row0_s .. row0_s + L_s and has segment boundaries b_0 (end of the prefix) .. b_n (= L_s),
    relative to its first row (the kernels' seq_meta: meta[0] = row0, meta[1 .. 1 + n] = b_0 .. b_n).
A query attends the keys at or before it (causal), whose key-mask byte is set, and, in a packed row, the prefix and its own
response only, never another response.  The key mask is one byte per row in both layouts.  Statistics (lse, delta) are returned as
[nh, rows]; the kernels store them as [S, nh, L] (padded) or [nh, rows_total] (ragged): `stat_view` maps one onto the other.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import torch

F64 = torch.float64


@dataclass
class Layout:
    rows: int
    seqs: List[Tuple[int, List[int]]]          # (first row, boundaries b_0 .. b_n with b_n = length); [L] alone = no segments
    causal: bool = True
    padded_L: int = 0                          # > 0: the padded layout, sequence s = rows s * padded_L ..

    @property
    def n_seg(self) -> int:
        return len(self.seqs[0][1]) - 1 if self.seqs else 0

    @property
    def L(self) -> int:                        # the kernels' grid length: the longest sequence
        return max((b[-1] for _, b in self.seqs), default=0)

    def meta(self, stride: Optional[int] = None) -> torch.Tensor:
        """int32 [S, stride]: [row0, b_0 .. b_n, 0 ...] (what the ragged kernels read)."""
        n = self.n_seg
        stride = stride or n + 2
        m = torch.zeros(len(self.seqs), stride, dtype=torch.int32)
        for s, (r0, b) in enumerate(self.seqs):
            assert len(b) == n + 1
            m[s, 0] = r0
            m[s, 1:2 + n] = torch.tensor(b, dtype=torch.int32)
        return m


def padded(S: int, L: int, seg: Tuple[int, int] = (0, 0), causal: bool = True) -> Layout:
    """S rows of L positions; seg = (seg_prefix, seg_len), seg_len = 0: no packed responses."""
    pfx, slen = seg
    if slen > 0:
        b = [pfx]
        while b[-1] + slen < L:
            b.append(b[-1] + slen)
        b.append(L)
    else:
        b = [L]
    return Layout(rows=S * L, seqs=[(s * L, list(b)) for s in range(S)], causal=causal, padded_L=L)


def ragged(prefixes: Sequence[int], responses: Sequence[Sequence[int]], causal: bool = True, gap: int = 0) -> Layout:
    """Sequence s = [prefix_s | responses[s][0] | ...], packed back to back (`gap` unused rows after each sequence)."""
    seqs, row = [], 0
    for p, rs in zip(prefixes, responses):
        b = [p]
        for r in rs:
            b.append(b[-1] + r)
        seqs.append((row, b))
        row += b[-1] + gap
    return Layout(rows=row, seqs=seqs, causal=causal)


def visibility(b: Sequence[int], causal: bool, device=None) -> torch.Tensor:
    """[L, L] bool, (query, key) -> key visible, before the key mask, for one sequence with boundaries b."""
    L = b[-1]
    pos = torch.arange(L, device=device)
    allow = torch.ones(L, L, dtype=torch.bool, device=device)
    if causal:
        allow &= pos[None, :] <= pos[:, None]
    if len(b) > 1:                                             # packed: keys in [prefix end, start of the query's segment) excluded
        pfx = b[0]
        qstart = torch.full((L,), pfx, dtype=torch.long, device=device)
        for a in range(1, len(b) - 1):
            qstart = torch.where(pos >= b[a], torch.full_like(qstart, b[a]), qstart)
        allow &= ~((pos[None, :] >= pfx) & (pos[None, :] < qstart[:, None]))
    return allow


def rope_angles(pos: torch.Tensor, hd: int, theta: float) -> torch.Tensor:
    """[rows, hd/2] float64: pos * theta^(-2i/hd)."""
    i = torch.arange(hd // 2, dtype=F64, device=pos.device)
    return pos.to(F64)[:, None] * torch.pow(torch.tensor(theta, dtype=F64), -2.0 * i / hd).to(pos.device)[None, :]


def rope_forward(x: torch.Tensor, pos: torch.Tensor, theta: float) -> torch.Tensor:
    """x [rows, nh, hd]: x * cos + rotate_half(x) * sin (LLaMA's apply_rotary_pos_emb), float64."""
    hd = x.shape[-1]
    a = rope_angles(pos, hd, theta)[:, None, :]
    c, s = torch.cos(a), torch.sin(a)
    x1, x2 = x[..., :hd // 2].to(F64), x[..., hd // 2:].to(F64)
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)


def rope_inverse(g: torch.Tensor, pos: torch.Tensor, theta: float) -> torch.Tensor:
    """The gradient through rope_forward: R(pos)^T g = g * cos - rotate_half(g) * sin, float64."""
    hd = g.shape[-1]
    a = rope_angles(pos, hd, theta)[:, None, :]
    c, s = torch.cos(a), torch.sin(a)
    x1, x2 = g[..., :hd // 2].to(F64), g[..., hd // 2:].to(F64)
    return torch.cat([x1 * c + x2 * s, x2 * c - x1 * s], -1)


def forward(q, k, v, lay: Layout, nh: int, scale: float, key_mask: Optional[torch.Tensor] = None):
    """Differentiable float64 attention.  q, k, v [rows, nh*hd] -> o [rows, nh*hd], lse [nh, rows] (-inf where a row sees no key),
    seen [rows] bool (the row sees at least one key).  Rows outside every sequence: o = 0, lse = nan, seen = False."""
    rows = q.shape[0]
    hd = q.shape[1] // nh
    dev = q.device
    q, k, v = q.to(F64), k.to(F64), v.to(F64)
    o_parts = []
    lse = torch.full((nh, rows), float("nan"), dtype=F64, device=dev)
    seen = torch.zeros(rows, dtype=torch.bool, device=dev)
    o = torch.zeros(rows, nh * hd, dtype=F64, device=dev)
    for r0, b in lay.seqs:
        Ls = b[-1]
        if Ls == 0:
            continue
        sl = slice(r0, r0 + Ls)
        allow = visibility(b, lay.causal, dev)
        if key_mask is not None:
            allow = allow & key_mask[sl].to(dev).bool()[None, :]
        has = allow.any(-1)                                      # [Ls]
        qs, ks, vs = (t[sl].view(Ls, nh, hd).transpose(0, 1) for t in (q, k, v))
        sc = torch.matmul(qs, ks.transpose(1, 2)) * scale        # [nh, Ls, Ls]
        sc = sc.masked_fill(~allow[None], float("-inf"))
        lse[:, sl] = torch.logsumexp(sc, -1).detach()
        sc = torch.where(has[None, :, None], sc, torch.zeros_like(sc))     # rows that see nothing: finite, then zeroed
        p = torch.softmax(sc, -1) * has[None, :, None]
        os_ = torch.matmul(p, vs).transpose(0, 1).reshape(Ls, nh * hd)
        o_parts.append((sl, os_))
        seen[sl] = has
    for sl, os_ in o_parts:
        o = o.index_copy(0, torch.arange(sl.start, sl.stop, device=dev), os_)
    return o, lse, seen


def reference(q, k, v, dout, lay: Layout, nh: int, scale: float, key_mask=None, o_kernel=None, rope=None):
    """Everything the kernels produce, in float64: o, lse [nh, rows], seen [rows], dq, dk, dv [rows, nh*hd] (autograd) and
    delta [nh, rows] = rowsum(dO * O) from the kernel's own O (`o_kernel`, default the reference O).
    rope = (pos [rows] int, theta): dq and dk are returned rotated back, R(pos)^T g, as the fused backward leaves them."""
    q64, k64, v64 = (t.detach().to(F64).requires_grad_(True) for t in (q, k, v))
    o, lse, seen = forward(q64, k64, v64, lay, nh, scale, key_mask)
    d64 = dout.detach().to(F64)
    dq, dk, dv = torch.autograd.grad(o, (q64, k64, v64), d64)
    rows, H = q.shape
    hd = H // nh
    if rope is not None:
        pos, theta = rope
        pos = pos.to(q.device)
        dq = rope_inverse(dq.view(rows, nh, hd), pos, theta).reshape(rows, H)
        dk = rope_inverse(dk.view(rows, nh, hd), pos, theta).reshape(rows, H)
    ok = (o if o_kernel is None else o_kernel).detach().to(F64)
    delta = (d64 * ok).view(rows, nh, hd).sum(-1).t().contiguous()
    return dict(o=o.detach(), lse=lse, seen=seen, dq=dq, dk=dk, dv=dv, delta=delta)


def stat_view(stat: torch.Tensor, lay: Layout, nh: int) -> torch.Tensor:
    """A kernel statistic buffer ([S, nh, L] padded, [nh, rows_total] ragged) as [nh, rows]."""
    if lay.padded_L:
        S = len(lay.seqs)
        return stat.view(S, nh, lay.padded_L).permute(1, 0, 2).reshape(nh, S * lay.padded_L)
    return stat.view(nh, -1)[:, :lay.rows]


def tile_relerr(got: torch.Tensor, want: torch.Tensor, lay: Layout, nh: int, rows_mask: Optional[torch.Tensor] = None,
                atol: float = 0.0):
    """Relative error over the whole tensor and the worst over (sequence, head, 64-row tile of the sequence).  A tile's error is
    |got - want| / (|want| + floor), floor = 1 % of the RMS tile norm of the whole tensor: tiles whose reference is (nearly) zero
    - padding rows, keys no query sees - are held to an absolute error of that size instead of a ratio of two tiny numbers.  atol: a
    larger floor (tile norm) for tensors that can be zero in exact arithmetic as a whole (dQ, dK of one-key sequences: dS = 0).
    rows_mask [rows] bool: rows that take part (default: every row of every sequence)."""
    rows, H = want.shape
    hd = H // nh
    g = got.to(F64)
    w = want.to(F64)
    if rows_mask is not None:
        m = rows_mask.to(w.device)[:, None]
        g, w = g * m, w * m
    d = (g - w).view(rows, nh, hd)
    w3 = w.view(rows, nh, hd)
    n_tiles = sum(nh * math.ceil(b[-1] / 64) for _, b in lay.seqs) or 1
    floor = max(1e-2 * float(w3.norm()) / math.sqrt(n_tiles), atol)
    whole = float(d.norm() / (w3.norm() + atol * math.sqrt(n_tiles) + 1e-300))
    worst, where = 0.0, None
    for s, (r0, b) in enumerate(lay.seqs):
        for t0 in range(0, b[-1], 64):
            sl = slice(r0 + t0, r0 + min(t0 + 64, b[-1]))
            dn = d[sl].norm(dim=(0, 2))
            wn = w3[sl].norm(dim=(0, 2))
            e = dn / (wn + floor + 1e-300)
            h = int(e.argmax())
            if float(e[h]) > worst:
                worst, where = float(e[h]), (s, h, t0)
    return whole, worst, where
