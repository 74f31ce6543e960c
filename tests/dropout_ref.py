"""Plain numpy / torch restatement of the LoRA dropout contract (csrc/kernels.h "LoRA dropout", include/opadpo_hip.h): no GPU.

    keep(seed, call, layer, module, row, col) = philox4x32_10(counter, key)[col & 3] >= floor(p * 2^32)      (unsigned compare)
    counter = (col >> 2, row, call & 0xffffffff, call >> 32)        key = (seed, layer * 8 + module)

seed < 2^32; module 0..6 = q, k, v, o, gate, up, down; row = the row of the pass's own row list (ragged: compact row; padded: s * L + l).
A kept element of the masked copy is bf16(x * fp32(1 / (1 - p))) - ONE rounding, the output of a bf16 nn.Dropout - a dropped one is 0.
"""
import contextlib
import math
import re

import numpy as np
import torch

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF
MODULES = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")


def philox4x32_10(counter, key):
    """counter: 4 arrays (or ints) of uint32 values, key: 2 -> 4 uint64 arrays holding the uint32 outputs (Random123 philox4x32, 10 rounds)."""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(MASK32) for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    m32 = np.uint64(MASK32)
    s32 = np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        hi0, lo0, hi1, lo1 = p0 >> s32, p0 & m32, p1 >> s32, p1 & m32
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return c


def threshold(p: float) -> int:
    assert 0.0 <= p < 1.0
    return int(math.floor(p * 4294967296.0))


def scale_of(p: float) -> np.float32:
    return np.float32(1.0 / (1.0 - p))


def keep_mask(seed: int, call: int, layer: int, module: int, rows, K: int, p: float) -> np.ndarray:
    """-> bool [len(rows), K]; rows = the row number of every row (any integer sequence)."""
    assert 0 <= seed <= MASK32 and 0 <= module <= 6 and K % 4 == 0
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, 1)
    c0 = np.arange(K // 4, dtype=np.uint64).reshape(1, -1)
    out = philox4x32_10((c0, rows, call & MASK32, (call >> 32) & MASK32), (seed, layer * 8 + module))
    words = np.stack(out, axis=-1).reshape(rows.shape[0], K)          # lane = col & 3
    return words >= np.uint64(threshold(p))


def dropout_fwd_ref(x: torch.Tensor, seed, call, layer, module0, g, rows, p) -> torch.Tensor:
    """x bf16 [M, K] -> bf16 [M, g*K], the g masked copies side by side."""
    M, K = x.shape
    scaled = (x.float() * torch.tensor(scale_of(p))).to(torch.bfloat16)
    outs = []
    for j in range(g):
        m = torch.from_numpy(keep_mask(seed, call, layer, module0 + j, rows, K, p))
        outs.append(torch.where(m, scaled, torch.zeros_like(scaled)))
    return torch.cat(outs, 1)


def dropout_bwd_add_ref(dx: torch.Tensor, u: torch.Tensor, seed, call, layer, module0, g, rows, p) -> torch.Tensor:
    """dx bf16 [M, K], u bf16 [M, g*K] -> fp32 [M, K]: dx + sum_j keep_j * u_j * scale, fp32 sum in module order (the kernel rounds it to bf16 once)."""
    M, K = dx.shape
    acc = dx.float()
    sc = torch.tensor(scale_of(p))
    for j in range(g):
        m = torch.from_numpy(keep_mask(seed, call, layer, module0 + j, rows, K, p))
        acc = acc + torch.where(m, u[:, j * K:(j + 1) * K].float() * sc, torch.zeros(()))
    return acc


# ---- the compact-row -> (oracle sequence, padded position) maps of the two layouts --------------------------------------------------------
def row_map_packed(lead, lens, keys, B, pfx):
    """Packed ragged rows (K responses of a sample share the prefix rows): -> list of (oracle sequence, padded position, row).  The prefix positions
    of EVERY response's oracle sequence read the sample's one set of prefix rows."""
    out, row = [], 0
    for b in range(B):
        ld = int(lead[b])
        for a in range(len(keys)):
            out += [(a * B + b, pos, row + pos - ld) for pos in range(ld, pfx)]
        row += pfx - ld
        for a, k in enumerate(keys):
            n = int(lens[k][b])
            out += [(a * B + b, pfx + t, row + t) for t in range(n)]
            row += n
    return out, row


def row_map_padded(S, L):
    """Padded rows: row = s * L + l for every position."""
    return [(s, l, s * L + l) for s in range(S) for l in range(L)], S * L


class OracleDropout:
    """oracle.llava_ref with LoRA dropout: inside `with OracleDropout(...).patch(LR):` every LLM `_Ctx.linear` feeds its LoRA branch
    (x * m) * fp32(1 / (1 - p)) with m = keep_mask of the module named by `key`, gathered through the row map; cells no row maps to keep 1."""

    def __init__(self, p, seed, call, row_map, S, L):
        self.p, self.seed, self.call, self.S, self.L = p, seed, call, S, L
        rm = np.asarray(row_map, dtype=np.int64).reshape(-1, 3)
        self.seq, self.pos, self.row = rm[:, 0], rm[:, 1], rm[:, 2]
        self._cache = {}

    def mask(self, layer, module, K):
        ck = (layer, module, K)
        if ck not in self._cache:
            m = torch.ones(self.S, self.L, K)
            if len(self.row):
                km = keep_mask(self.seed, self.call, layer, module, self.row, K, self.p)
                m[torch.from_numpy(self.seq), torch.from_numpy(self.pos)] = torch.from_numpy(km).float()
            self._cache[ck] = m
        return self._cache[ck]

    @contextlib.contextmanager
    def patch(self, LR):
        outer = self
        base = LR._Ctx

        class _DropCtx(base):
            def linear(self, x, key, bias=True):
                mt = re.search(r"(?<!vision_tower\.)layers\.(\d+)\.(?:self_attn|mlp)\.(\w+)$", key)
                if mt is None or "vision_tower" in key or mt.group(2) not in MODULES or self.lora is None:
                    return super().linear(x, key, bias)
                a = self.lora.get(LR.PEFT_PREFIX + key + ".lora_A.weight")
                if a is None:
                    return super().linear(x, key, bias)
                lora, self.lora = self.lora, None
                try:
                    y = super().linear(x, key, bias)            # the base Linear alone (with its own rounding)
                finally:
                    self.lora = lora
                m = outer.mask(int(mt.group(1)), MODULES.index(mt.group(2)), x.shape[-1]).to(x.device)
                xd = self.r(x * torch.tensor(scale_of(outer.p), device=x.device)) * m.view(x.shape)
                bb = lora[LR.PEFT_PREFIX + key + ".lora_B.weight"].float()
                if self.emu and LR.HF_BF16:
                    return self.r(y + self.r(self.r(LR._matmul_t(self.r(LR._matmul_t(xd, a.float())), bb)) * self.d.lora_scale))
                t = self.r(self.d.lora_scale * LR._matmul_t(xd, a.float()), "t")
                return y + LR._matmul_t(t, bb)

        LR._Ctx = _DropCtx
        try:
            yield self
        finally:
            LR._Ctx = base
