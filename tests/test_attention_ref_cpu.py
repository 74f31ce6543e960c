"""CPU: the float64 attention reference (tests/attn_ref.py) the GPU attention tests compare the kernels with is itself right -
packed and ragged layouts equal separate sequences, the inverse rotation is the transpose of the rotation, and its gradients
equal finite differences."""
import math

import pytest
import torch

import attn_ref as R

F64 = torch.float64


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16).to(F64)


@pytest.mark.parametrize("n_resp,key_holes", [([5, 0, 7], False), ([4, 4, 4], True), ([9], True)])
def test_ragged_equals_separate_prefix_response_sequences(n_resp, key_holes):
    """Sequence [prefix | r_0 | r_1 | ...] with the segment rule == len(n_resp) separate sequences [prefix | r_a]: same o, lse, dq, dk, dv on
    the response rows; prefix dK / dV of the packed row = sum over the separate runs (prefix dO is given to run 0 only)."""
    nh, hd, pfx = 2, 16, 11
    lay = R.ragged([3, pfx], [[2], n_resp])          # a first, unrelated sequence: the reference must keep sequences apart
    rows, H = lay.rows, nh * hd
    q, k, v, do = (rnd(rows, H, seed=i) for i in range(4))
    km = torch.ones(rows, dtype=torch.uint8)
    if key_holes:
        km[5 + 2] = 0                                # inside the prefix of sequence 1
        km[5 + pfx + 1] = 0                          # inside its first response
    scale = hd ** -0.5
    ref = R.reference(q, k, v, do, lay, nh, scale, key_mask=km)
    r0 = lay.seqs[1][0]
    b = lay.seqs[1][1]
    dk_pfx = torch.zeros(pfx, H, dtype=F64)
    dv_pfx = torch.zeros(pfx, H, dtype=F64)
    for a in range(len(n_resp)):
        rs = list(range(r0 + b[a], r0 + b[a + 1]))
        idx = torch.tensor(list(range(r0, r0 + pfx)) + rs, dtype=torch.long)
        d_sep = do[idx].clone()
        if a > 0:
            d_sep[:pfx] = 0
        one = R.padded(1, len(idx))
        sep = R.reference(q[idx], k[idx], v[idx], d_sep, one, nh, scale, key_mask=km[idx])
        for name in ("o", "dq", "dk", "dv"):
            torch.testing.assert_close(ref[name][rs], sep[name][pfx:], rtol=1e-12, atol=1e-12, msg=name)
        torch.testing.assert_close(ref["lse"][:, rs], sep["lse"][:, pfx:], rtol=1e-12, atol=1e-12)
        if a == 0:
            torch.testing.assert_close(ref["o"][r0:r0 + pfx], sep["o"][:pfx], rtol=1e-12, atol=1e-12)
            torch.testing.assert_close(ref["dq"][r0:r0 + pfx], sep["dq"][:pfx], rtol=1e-12, atol=1e-12)
        dk_pfx += sep["dk"][:pfx]
        dv_pfx += sep["dv"][:pfx]
    torch.testing.assert_close(ref["dk"][r0:r0 + pfx], dk_pfx, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(ref["dv"][r0:r0 + pfx], dv_pfx, rtol=1e-12, atol=1e-12)
    # the first sequence is untouched by the second
    first = R.reference(q[:5], k[:5], v[:5], do[:5], R.ragged([3], [[2]]), nh, scale, key_mask=km[:5])
    torch.testing.assert_close(ref["o"][:5], first["o"], rtol=0, atol=0)


def test_padded_packed_equals_ragged_with_equal_responses():
    nh, hd, S, pfx, T, K = 2, 16, 2, 7, 5, 3
    Ln = pfx + K * T
    pad = R.padded(S, Ln, (pfx, T))
    rag = R.ragged([pfx] * S, [[T] * K] * S)
    assert [b for _, b in pad.seqs] == [b for _, b in rag.seqs] and pad.rows == rag.rows
    q, k, v, do = (rnd(S * Ln, nh * hd, seed=10 + i) for i in range(4))
    km = torch.ones(S * Ln, dtype=torch.uint8)
    km[1] = 0
    km[Ln + pfx + T - 1] = 0
    a = R.reference(q, k, v, do, pad, nh, hd ** -0.5, key_mask=km)
    b = R.reference(q, k, v, do, rag, nh, hd ** -0.5, key_mask=km)
    for name in ("o", "lse", "dq", "dk", "dv", "delta"):
        assert torch.equal(a[name], b[name]), name
    # the statistics views of the two kernel layouts ([S, nh, L] / [nh, rows]) land on the same [nh, rows]
    st = torch.arange(S * nh * Ln, dtype=F64)
    assert torch.equal(R.stat_view(st, pad, nh)[1, Ln + 3], st.view(S, nh, Ln)[1, 1, 3])
    assert torch.equal(R.stat_view(st, rag, nh)[1, Ln + 3], st.view(nh, S * Ln)[1, Ln + 3])


def test_segment_rule_against_a_direct_statement():
    """visibility() for packed responses, restated position by position."""
    b = [4, 6, 6, 9, 12]                             # prefix 4, responses of 2, 0, 3, 3
    vis = R.visibility(b, causal=True)
    seg_of = lambda p: -1 if p < 4 else max(a for a in range(len(b) - 1) if p >= b[a])
    for qp in range(12):
        for kp in range(12):
            want = kp <= qp and (kp < 4 or seg_of(kp) == seg_of(qp))
            assert bool(vis[qp, kp]) == want, (qp, kp)


def test_inverse_rotation_is_the_transpose():
    rows, nh, hd, theta = 7, 3, 16, 10000.0
    pos = torch.tensor([0, 1, 5, 63, 64, 700, 1086])
    x = torch.randn(rows, nh, hd, dtype=F64)
    g = torch.randn(rows, nh, hd, dtype=F64)
    # <R x, g> == <x, R^T g>, and R^T R = I
    lhs = (R.rope_forward(x, pos, theta) * g).sum()
    rhs = (x * R.rope_inverse(g, pos, theta)).sum()
    assert abs(float(lhs - rhs)) < 1e-10
    torch.testing.assert_close(R.rope_inverse(R.rope_forward(x, pos, theta), pos, theta), x, rtol=1e-12, atol=1e-12)
    # angle definition: pos * theta^(-2i/hd); position 0 is the identity
    a = R.rope_angles(pos, hd, theta)
    assert float(a[2, 1]) == pytest.approx(5 * theta ** (-2 / hd), rel=1e-15)
    torch.testing.assert_close(R.rope_forward(x[:1], pos[:1], theta), x[:1], rtol=0, atol=0)
    # the reference's rope option = autograd through rope_forward
    xr = x.clone().requires_grad_(True)
    (gx,) = torch.autograd.grad(R.rope_forward(xr, pos, theta), xr, g)
    torch.testing.assert_close(gx, R.rope_inverse(g, pos, theta), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("causal", [True, False])
def test_gradients_equal_finite_differences(causal):
    nh, hd = 2, 8
    lay = R.ragged([3, 4], [[3, 2], [0, 3]], causal=causal) if causal else R.padded(2, 6, causal=False)
    rows, H = lay.rows, nh * hd
    q, k, v, do = (torch.randn(rows, H, dtype=F64, generator=torch.Generator().manual_seed(30 + i)) for i in range(4))
    km = torch.ones(rows, dtype=torch.uint8)
    km[1] = 0
    km[0] = 0                                       # row 0 sees no key (causal): zero output, zero gradient
    scale = 0.7
    ref = R.reference(q, k, v, do, lay, nh, scale, key_mask=km)
    if causal:
        assert not bool(ref["seen"][0]) and float(ref["o"][0].abs().max()) == 0.0

    def loss(q_, k_, v_):
        o, _, _ = R.forward(q_, k_, v_, lay, nh, scale, km)
        return float((o * do).sum())

    eps = 1e-6
    g = torch.Generator().manual_seed(99)
    for i, name in enumerate(("dq", "dk", "dv")):
        for _ in range(4):
            r, c = int(torch.randint(rows, (1,), generator=g)), int(torch.randint(H, (1,), generator=g))
            plus = [q.clone(), k.clone(), v.clone()]
            minus = [q.clone(), k.clone(), v.clone()]
            plus[i][r, c] += eps
            minus[i][r, c] -= eps
            fd = (loss(*plus) - loss(*minus)) / (2 * eps)
            assert math.isclose(float(ref[name][r, c]), fd, rel_tol=1e-6, abs_tol=1e-8), (name, r, c, float(ref[name][r, c]), fd)
