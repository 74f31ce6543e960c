"""GPU: rollout decode for 65..256 sequences per device - opadpo_gemm_nt_decode_wide against an fp64 product of its bf16 inputs (per element,
derived bounds), its row independence, and CtxEngine.generate at 72 / 130 / 256 rows against the same prompts run through the <= 64-row path."""
import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
U24, U8 = 2.0 ** -24, 2.0 ** -8          # fp32 unit roundoff of an accumulation step; bf16 round-to-nearest (8 significand bits)


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from opadpo_amd import lib
    lib.load()
    yield lib
    lib.set_flags(True, True)


def dev():
    return torch.device("cuda:0")


# ---- op level --------------------------------------------------------------------------------------------------------------------------
# (N, K): 128 = two k-tiles (one half chunk), 256 = four (one full round of the weight slots), 704 = eleven (odd: a half chunk of one k-tile,
# and no multiple of the 3-way K-split); N = 256 / 1024 leave a partly filled last workgroup of gate rows in the SwiGLU mode at 48 + 48 rows, and
# (22016, 128) is the smallest K at which the library itself picks those 96-row workgroups (the 7B gate|up width).
SHAPES = [(256, 128), (384, 256), (1024, 704)]
_CACHE = {}


def operands(N, K):
    """-> a [256, K] bf16, w [N, K] bf16 (random: every row and column distinct), and the fp64 product / absolute-value product of the bf16 values.
    Computed once per shape and shared (never written to)."""
    if (N, K) not in _CACHE:
        g = torch.Generator(device="cpu").manual_seed(1000 * N + K)
        a = (torch.randn(256, K, generator=g) * 0.5).to(BF).to(dev())
        w = (torch.randn(N, K, generator=g) * 0.1).to(BF).to(dev())
        a64, w64 = a.double(), w.double()
        _CACHE[(N, K)] = (a, w, a64 @ w64.t(), a64.abs() @ w64.abs().t())
    return _CACHE[(N, K)]


def pair_views(t, F):
    """[M, 2F] columns per 128 = [64 gate | 64 up] -> gate [M, F], up [M, F]"""
    z = t.view(t.shape[0], F // 64, 2, 64)
    return z[:, :, 0].reshape(-1, F), z[:, :, 1].reshape(-1, F)


def run_mode(L, a, w, M, N, K, mode, splits):
    """one launch on rows [0, M) of a; -> (result as the consumer sees it, rows >= M of the output buffer, their fill value)"""
    if mode == 0:
        out = torch.full((M + 2, N), 7.0, dtype=BF, device=dev())
        L.call("opadpo_gemm_nt_decode_wide", L.ptr(a), K, L.ptr(w), K, K, L.ptr(out), N, 0, M, N, 1, L.stream())
        return out[:M], out[M:], 7.0
    if mode == 1:
        S = L.load().opadpo_gemm_nt_decode_splits(N, K, splits)
        assert 1 <= S <= K // 64
        part = torch.full((S, M, N), 3.0, device=dev())
        L.call("opadpo_gemm_nt_decode_wide", L.ptr(a), K, L.ptr(w), K, K, L.ptr(part), N, 1, M, N, splits, L.stream())
        acc = part[0].clone()
        for s in range(1, S):                 # slice order, fp32: what opadpo_rmsnorm_sum_fwd adds
            acc += part[s]
        return acc, None, S
    F = N // 2
    out = torch.full((M + 2, F), 5.0, dtype=BF, device=dev())
    L.call("opadpo_gemm_nt_decode_wide", L.ptr(a), K, L.ptr(w), K, K, L.ptr(out), F, 2, M, N, 1, L.stream())
    return out[:M], out[M:], 5.0


def check(got, M, N, K, mode, ref, absref, what):
    """Per-element bound, derived: an fp32 accumulation of K products in any order errs by at most K * 2^-24 * sum |a||w| (mode 1; the adds of the
    slices are among those K steps); a bf16 store adds 2^-8 |ref| (mode 0).  Mode 2 computes silu(bf16(g)) * bf16(u) in fp32 and stores bf16:
    with eg, eu the mode-0 bounds of gate and up and |silu'| <= 1.1, |silu(g') u' - silu(g) u| <= 1.1 eg (|u| + eu) + |silu(g)| eu, the fp32 evaluation with the
    fast exponential adds 2^-20 |silu(g) u|, and the store 2^-8 of the value it rounds."""
    ref, absref = ref[:M], absref[:M]
    e32 = K * U24 * absref
    if mode == 1:
        err, bound = (got.double() - ref).abs(), e32
    elif mode == 0:
        err, bound = (got.double() - ref).abs(), e32 + U8 * ref.abs()
    else:
        F = N // 2
        (g, u), (eg, eu) = pair_views(ref, F), pair_views(e32 + U8 * ref.abs(), F)
        sg = g * torch.sigmoid(g)
        want = sg * u
        pre = 1.1 * eg * (u.abs() + eu) + sg.abs() * eu + 2.0 ** -20 * want.abs()
        err, bound = (got.double() - want).abs(), pre + U8 * (want.abs() + pre)
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: max |err| / bound = {worst:.3f}, max |err| = {float(err.max()):.3e}")
    assert bool((err <= bound).all()), f"{what}: {int((err > bound).sum())} elements above the bound, worst ratio {worst}"


@pytest.mark.parametrize("M", [65, 80, 128, 129, 255, 256])
@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("rows", [0, 1, 2, 3])
def test_decode_wide_against_fp64(L, M, N, K, rows):
    """All three modes of opadpo_gemm_nt_decode_wide against the fp64 product of the bf16 inputs, per element; rows >= M of the output are not touched.
    rows: 0 = weight rows per workgroup by shape, 1 / 2 / 3 = 48 / 64 / 128 forced where the shape allows (opadpo_set_flags use_tr bits 7-8)."""
    a, w, ref, absref = operands(N, K)
    L.set_flags(10, 1 | (rows << 7))
    try:
        got, rest, fill = run_mode(L, a, w, M, N, K, 0, 1)
        check(got, M, N, K, 0, ref, absref, f"bf16 M={M} N={N} K={K}")
        assert float((rest.float() - fill).abs().max()) == 0.0
        for splits in (0, 3):
            got, _, S = run_mode(L, a, w, M, N, K, 1, splits)
            check(got, M, N, K, 1, ref, absref, f"fp32 x{S} M={M} N={N} K={K}")
        got, rest, fill = run_mode(L, a, w, M, N, K, 2, 1)
        check(got, M, N, K, 2, ref, absref, f"swiglu M={M} N={N} K={K}")
        assert float((rest.float() - fill).abs().max()) == 0.0
    finally:
        L.set_flags(10, True)


@pytest.mark.parametrize("M", [65, 129, 256])
def test_decode_wide_swiglu_96_row_workgroups(L, M):
    """The SwiGLU mode at the 7B gate|up width, where the library picks 48 gate + 48 up rows per workgroup and the last workgroup is partly filled
    (11008 gate rows = 229 x 48 + 16); K = 128 keeps it small.  Strided operands (rows inside wider buffers) on the way."""
    N, K = 22016, 128
    g = torch.Generator(device="cpu").manual_seed(7)
    abig = (torch.randn(M, K + 64, generator=g) * 0.5).to(BF).to(dev())
    wbig = (torch.randn(N, K + 128, generator=g) * 0.1).to(BF).to(dev())
    a64, w64 = abig[:, :K].double(), wbig[:, :K].double()
    ref, absref = a64 @ w64.t(), a64.abs() @ w64.abs().t()
    F = N // 2
    out = torch.full((M + 1, F + 8), 5.0, dtype=BF, device=dev())
    L.call("opadpo_gemm_nt_decode_wide", L.ptr(abig), K + 64, L.ptr(wbig), K + 128, K, L.ptr(out), F + 8, 2, M, N, 1, L.stream())
    check(out[:M, :F], M, N, K, 2, ref, absref, f"swiglu 96-row M={M}")
    assert float((out[M:].float() - 5.0).abs().max()) == 0.0 and float((out[:, F:].float() - 5.0).abs().max()) == 0.0


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_decode_wide_row_independence(L, mode):
    """A row's result does not depend on how many rows share the launch: rows 0..64 at M = 256 are the M = 65 result bit for bit, the rows of
    M = 129 are the same rows of M = 256, whatever the weight rows per workgroup - and rows 0..63 are what opadpo_gemm_nt_decode computes at M = 64
    (the same K-split and k order in both kernels)."""
    N, K = 1024, 704
    a, w, _, _ = operands(N, K)
    res = {}
    for rows in (0, 3):
        L.set_flags(10, 1 | (rows << 7))
        for M in (65, 129, 256):
            res[(rows, M)] = run_mode(L, a, w, M, N, K, mode, 0)[0].clone()
    L.set_flags(10, True)
    torch.cuda.synchronize()
    bits = lambda t: t.view(torch.int16) if t.dtype == BF else t.view(torch.int32)
    base = res[(0, 256)]
    for (rows, M), r in res.items():
        assert torch.equal(bits(r), bits(base[:M])), (rows, M, int((bits(r) != bits(base[:M])).sum()))
    if mode == 1:
        S = L.load().opadpo_gemm_nt_decode_splits(N, K, 0)
        part = torch.empty(S, 64, N, device=dev())
        L.call("opadpo_gemm_nt_decode", L.ptr(a), K, L.ptr(w), K, K, L.ptr(part), N, 1, 64, N, 0, L.stream())
        small = part[0].clone()
        for s in range(1, S):
            small += part[s]
    else:
        small = torch.empty(64, N // 2 if mode == 2 else N, dtype=BF, device=dev())
        L.call("opadpo_gemm_nt_decode", L.ptr(a), K, L.ptr(w), K, K, L.ptr(small), small.shape[1], mode, 64, N, 1, L.stream())
    assert torch.equal(bits(small), bits(base[:64]))


# ---- engine level ------------------------------------------------------------------------------------------------------------------------
from test_parity_gpu import setup  # noqa: E402,F401  (module fixture of the parity suite: tiny dims, oracle weights, CtxEngine)

N_NEW, Q = 6, 12


def prompts(d, B, seed):
    g = torch.Generator().manual_seed(seed)
    images = torch.randn(B, 3, d.image_size, d.image_size, generator=g).to(BF).float()
    queries = torch.randint(3, d.vocab, (B, Q), generator=g)
    qmask = torch.ones(B, Q, dtype=torch.bool)
    for b in range(B):
        pad = b % 4                                   # left padding of 0..3 positions
        queries[b, :pad] = 0
        qmask[b, :pad] = False
        queries[b, 4 + b % 5] = -200                  # the image token
    return images, queries, qmask


def adapter_of(s, kind):
    from opadpo_amd.model import LoraAdapter
    vis_only = {k: v for k, v in s["lora_ref"].items() if "vision_tower" in k or "mm_projector" in k}
    if kind == "none":
        return None, vis_only, dict()
    return LoraAdapter(s["d"], s["lora_ref"], s["dev"], trainable=False), s["lora_ref"], dict(merge_adapter=True)      # merged, SwiGLU fused in gate|up


@pytest.mark.parametrize("kind", ["none", "merged"])
@pytest.mark.parametrize("B", [72, 130])
def test_generate_wide_matches_chunked_rollout(setup, kind, B):
    """Greedy rollout of B = 72 / 130 prompts in ONE decode (the 65..256-row kernels) against the same prompts run through the existing path in
    chunks of at most 64: eager and graph replay bit-equal; a row may leave its chunked run only from a step where the fp32 oracle puts the top-two
    logit gap on that prefix below the bf16 floor, 2^-7 x |top logit|, and at most 10 % of the rows may.  (The tiny random model's logits are flat: on the
    CPU the oracle's own greedy path has such a near-tie somewhere in 25-38 % of these rows, at these seeds and at every other one tried, so no seed keeps a
    bf16 run within the cap AGAINST THE ORACLE; the cap holds here because both runs compute a row with the same sums in the same order.)"""
    s = setup
    LR = s["LR"]
    from opadpo_amd.generate import Generator
    images, queries, qmask = prompts(s["d"], B, seed=500 + B)
    adapter, lora, gkw = adapter_of(s, kind)
    kw = dict(max_new_tokens=N_NEW, temperature=1.0, top_k=1, top_p=1.0, seed=1)
    outs = []
    for use_graph in (False, True):
        gen = Generator(s["eng"], adapter, use_graph=use_graph, **gkw)
        feats = gen.engine.encode_images(images.to(s["dev"]))
        outs.append(gen.generate(queries, qmask, image_feats=feats, **kw).cpu())
    assert outs[0].shape == (B, N_NEW) and torch.equal(outs[0], outs[1]), "graph replay differs from eager steps"
    wide = outs[0]
    assert int(wide.min()) >= 0 and int(wide.max()) < s["d"].vocab
    gen = Generator(s["eng"], adapter, use_graph=False, **gkw)
    chunked = torch.cat([gen.generate(queries[i:i + 64], qmask[i:i + 64], image_feats=feats[i:i + 64], **kw).cpu() for i in range(0, B, 64)])
    differ = (wide != chunked).any(1).nonzero().flatten().tolist()
    print(f"{kind} B={B}: {len(differ)} of {B} rows differ from the chunked run")
    assert len(differ) <= B // 10, differ
    if differ:
        feats_o = LR.image_features(images[differ], s["W"], lora, s["od"])
        for j, b in enumerate(differ):
            t = int((wide[b] != chunked[b]).nonzero()[0])
            ids = torch.cat([queries[b:b + 1], wide[b:b + 1, :t]], 1)
            mask = torch.cat([qmask[b:b + 1], torch.ones(1, t, dtype=torch.bool)], 1)
            top2 = LR.llava_logits(ids, mask, None, s["W"], lora, s["od"], feats=feats_o[j:j + 1])[0, -1].float().topk(2)
            gap, floor = float(top2.values[0] - top2.values[1]), 2.0 ** -7 * float(top2.values[0].abs())
            assert gap < floor, (b, t, gap, floor)
            assert {int(wide[b, t]), int(chunked[b, t])} == {int(top2.indices[0]), int(top2.indices[1])}, (b, t)


def test_generate_wide_sampled_graph_equals_eager(setup):
    """temperature 1, top_k 30, top_p 0.95 at 72 rows: graph replay and eager steps draw the same tokens, all inside the vocabulary."""
    s = setup
    from opadpo_amd.generate import Generator
    images, queries, qmask = prompts(s["d"], 72, seed=9)
    outs = []
    for use_graph in (False, True):
        gen = Generator(s["eng"], None, use_graph=use_graph)
        feats = gen.engine.encode_images(images.to(s["dev"]))
        outs.append(gen.generate(queries, qmask, image_feats=feats, max_new_tokens=N_NEW, temperature=1.0, top_k=30, top_p=0.95, seed=3).cpu())
    assert torch.equal(outs[0], outs[1])
    assert outs[0].shape == (72, N_NEW) and int(outs[0].min()) >= 0 and int(outs[0].max()) < s["d"].vocab
    assert len({tuple(r) for r in outs[0].tolist()}) > 36          # rows are not copies of each other


def test_generate_wide_bounds_on_a_live_context(setup):
    """256 rows generate; 257 are refused with text; armed logit processors with 65 rows raise, disarm, and leave the next plain generation as it was;
    an unmerged adapter above 64 rows runs (the tiled kernels) and, greedy, agrees with its chunked run outside near-ties."""
    s = setup
    from opadpo_amd import lib as L
    from opadpo_amd.generate import Generator
    d = s["d"]
    images, queries, qmask = prompts(d, 256, seed=21)
    gen = Generator(s["eng"], None, use_graph=False)
    feats = gen.engine.encode_images(images.to(s["dev"]))
    kw = dict(max_new_tokens=N_NEW, temperature=1.0, top_k=1, top_p=1.0, seed=1)
    out = gen.generate(queries, qmask, image_feats=feats, **kw).cpu()
    assert out.shape == (256, N_NEW) and int(out.min()) >= 0 and int(out.max()) < d.vocab
    first64 = gen.generate(queries[:64], qmask[:64], image_feats=feats[:64], **kw).cpu()
    assert torch.equal(first64, out[:64])                          # rows do not depend on the batch they decode in, nor on which decode GEMM ran them
    plain = gen.generate(queries[:65], qmask[:65], image_feats=feats[:65], **kw).cpu()
    with pytest.raises(L.OpadpoError, match="64"):
        gen.generate(queries[:65], qmask[:65], image_feats=feats[:65], logit_bias={5: 2.0}, **kw)
    with pytest.raises(L.OpadpoError, match="64"):
        gen.generate(queries[:65], qmask[:65], image_feats=feats[:65], score_ids=[5, 7], **kw)
    assert torch.equal(gen.generate(queries[:65], qmask[:65], image_feats=feats[:65], **kw).cpu(), plain)
    q257, m257 = torch.cat([queries, queries[:1]]), torch.cat([qmask, qmask[:1]])
    with pytest.raises(L.OpadpoError, match="256"):
        gen.generate(q257, m257, image_feats=torch.cat([feats, feats[:1]]), **kw)
    lora = Generator(s["eng"], s["ref"], use_graph=False)          # unmerged adapter: LoRA tails, tiled GEMMs above 64 rows
    got = lora.generate(queries[:70], qmask[:70], image_feats=feats[:70], **kw).cpu()
    want = torch.cat([lora.generate(queries[i:i + 35], qmask[i:i + 35], image_feats=feats[i:i + 35], **kw).cpu() for i in (0, 35)])
    assert got.shape == (70, N_NEW) and int((got != want).any(1).sum()) <= 7
