"""CPU: the C-ABI library builds for gfx950, loads, and exports every symbol include/opadpo_hip.h
declares with the argument lists the ctypes binding assumes (no compute calls without a GPU)."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "opadpo_hip.h")

CTYPE = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
         "uint64_t": ctypes.c_uint64}


def parse_header():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = {}
    for m in re.finditer(r"(int|void|size_t|const char\*)\s+(opadpo_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S):
        ret, name, args = m.group(1), m.group(2), " ".join(m.group(3).split())
        types = []
        if args and args != "void":
            for a in args.split(","):
                a = a.strip()
                if "*" in a or a.split()[0].endswith("_fn"):       # pointers, and the typedef'd allocator function pointers
                    types.append(ctypes.c_void_p)
                else:
                    types.append(CTYPE[a.replace("const ", "").split()[0]])
        protos[name] = (ret, types)
    return protos


@pytest.fixture(scope="module")
def built_lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location("opadpo_build", os.path.join(REPO, "opa-dpo_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.build(verbose=False)


def test_header_declares_the_path():
    protos = parse_header()
    assert len(protos) >= 33
    for need in ("opadpo_gemm_nt", "opadpo_gemm_tn", "opadpo_attn_fwd", "opadpo_attn_bwd", "opadpo_head_fwd",
                 "opadpo_head_bwd", "opadpo_adamw", "opadpo_sample", "opadpo_attn_decode", "opadpo_rope_kv_append", "opadpo_embed_splice",
                 # sequence-level context API
                 "opadpo_ctx_create", "opadpo_ctx_destroy", "opadpo_ctx_last_error", "opadpo_vision_encode", "opadpo_seq_logprobs_fwd",
                 "opadpo_seq_logprobs_bwd", "opadpo_decode_begin", "opadpo_decode_step", "opadpo_decode_run"):
        assert need in protos


def test_library_exports_every_declared_symbol(built_lib):
    lib = ctypes.CDLL(built_lib)
    for name in parse_header():
        assert hasattr(lib, name), f"{name} declared in include/opadpo_hip.h but not exported"
    lib.opadpo_abi_version.restype = ctypes.c_int
    assert lib.opadpo_abi_version() == 2


def test_binding_matches_header(built_lib):
    from opadpo_amd import lib as L
    protos = parse_header()
    bound = set(L.SIGNATURES) | set(L.OTHER_SYMBOLS)
    assert bound == set(protos), bound ^ set(protos)
    for name, argtypes in L.SIGNATURES.items():
        ret, types = protos[name]
        assert ret == "int"
        assert [t for t in argtypes] == types, f"{name}: binding {argtypes} != header {types}"
    L.load()


def test_host_side_validation_needs_no_gpu(built_lib):
    """Shape validation happens before any launch: a bad call fails loudly with a message."""
    lib = ctypes.CDLL(built_lib)
    lib.opadpo_last_error.restype = ctypes.c_char_p
    fn = lib.opadpo_gemm_nt
    from opadpo_amd import lib as L
    fn.argtypes = L.SIGNATURES["opadpo_gemm_nt"]
    fn.restype = ctypes.c_int
    rc = fn(None, 64, None, 64, 64, None, 0, None, 0, 0, 0, 0, 0, 0, None, 100, 0, None, 0, 0, None, 10, 100, 1.0, 0, None)
    assert rc != 0 and b"multiple of 128" in lib.opadpo_last_error()


def test_context_lifecycle_and_errors_need_no_gpu(built_lib):
    """opadpo_ctx: creation validates the geometry, entry points fail with a message (never abort) before any launch."""
    from opadpo_amd import lib as L
    from opadpo_amd.ctx import Dims
    lib = L.load()
    good = Dims(256, 2, 2, 128, 384, 512, 1e-5, 10000.0, 128, 2, 2, 256, 56, 14, 1e-5, 128, 256.0)
    h = ctypes.c_void_p()
    assert lib.opadpo_ctx_create(ctypes.byref(good), 0, ctypes.byref(h)) == 0 and h.value
    assert lib.opadpo_ctx_set_flags(h, 4, 1) == 0
    # forward before the weights were handed over: refused with text
    rc = lib.opadpo_seq_logprobs_fwd(h, 0, None, None, None, None, None, 1, 8, 2, 1, 1.0, 0, None, None, None, None, None)
    assert rc != 0 and b"weights not set" in lib.opadpo_ctx_last_error(h)
    assert lib.opadpo_ctx_set_adapter(h, 99, None, None, None) != 0 and b"out of range" in lib.opadpo_ctx_last_error(h)
    assert lib.opadpo_decode_step(h, None) != 0 and b"no active rollout" in lib.opadpo_ctx_last_error(h)
    assert lib.opadpo_saved_release(h, ctypes.c_void_p(1234)) != 0
    assert lib.opadpo_ctx_bytes_peak(h) == 0
    lib.opadpo_ctx_destroy(h)
    bad = Dims(250, 2, 2, 128, 384, 512, 1e-5, 10000.0, 128, 2, 2, 256, 56, 14, 1e-5, 128, 256.0)     # hidden != heads * head_dim
    h2 = ctypes.c_void_p()
    assert lib.opadpo_ctx_create(ctypes.byref(bad), 0, ctypes.byref(h2)) != 0 and not h2.value


def test_decode_attention_key_range_rule(built_lib):
    """Host-side geometry of opadpo_attn_decode, read through the workspace size (B * nh * ranges * (hd + 2) floats, 0 for one range):
    up to 256 (sequence, head) pairs as many key ranges as fit ONE round of the 256 CUs; two ranges for 257-767 pairs; from 768 pairs two
    ranges only where they cut the rounds of 1024 resident workgroups by a fifth or more; never more ranges than max_ctx / 256."""
    lib = ctypes.CDLL(built_lib)
    f = lib.opadpo_attn_decode_workspace_bytes
    f.restype = ctypes.c_size_t
    f.argtypes = [ctypes.c_int] * 4
    nh, hd, ctx = 32, 128, 1024

    def ranges(B, nh=nh, max_ctx=ctx):
        b = f(B, nh, hd, max_ctx)
        assert b % (B * nh * (hd + 2) * 4) == 0
        return max(1, b // (B * nh * (hd + 2) * 4))

    assert [ranges(B) for B in (1, 2, 3, 4)] == [4, 4, 2, 2]            # 4 = the max_ctx / 256 cap
    assert [ranges(B) for B in (5, 6, 7, 8)] == [1, 1, 1, 1]            # 160-256 pairs: one round of 16-wave workgroups
    assert [ranges(B) for B in (9, 12, 16, 23)] == [2, 2, 2, 2]
    assert [ranges(B) for B in (24, 28, 32)] == [1, 1, 1]
    assert [ranges(B) for B in (33, 36, 40, 48)] == [2, 2, 2, 2]
    assert [ranges(B) for B in (49, 56, 64)] == [1, 1, 1]
    assert ranges(40, max_ctx=384) == 1 and ranges(12, max_ctx=384) == 1 and ranges(2, max_ctx=600) == 2
    assert ranges(32, nh=40) == 2 and ranges(64, nh=40) == 1            # 13B head count
    assert f(0, nh, hd, ctx) == 0


def test_gemm_nt_routing_rule(built_lib):
    """Host-side kernel choice of opadpo_gemm_nt, read through opadpo_debug_gemm_nt_plan (a test entry point outside the header: the same
    validation, then the launches the dispatch would make on `cus` CUs as `kernel grid.x grid.y block LDS` lines; nothing is launched).  Pins
    kernel + grid of the product path's GEMMs at the 7B / 13B benchmark row counts and at ragged ones, the K-folded N = 256 LoRA products,
    the vision tower's bias / activation GEMMs, the tail forms, the decode routes and every gemm_variant / use_tr bit the GPU tests use as a
    cross-check (opadpo_set_flags)."""
    lib = ctypes.CDLL(built_lib)
    f = lib.opadpo_debug_gemm_nt_plan
    f.restype = ctypes.c_int
    _p, _i = ctypes.c_void_p, ctypes.c_int
    f.argtypes = [_p, _i, _p, _i, _i, _p, _i, _p, _i, _i, _i, _i, _i, _i, _p, _i, _i, _p, _i, _i, _p, _i, _i, ctypes.c_float, _i,
                  _i, _i, _i, _i, ctypes.c_char_p, _i]
    S = 0x100      # OPADPO_GEMM_STREAM

    def plan(M, N, K1, K2=0, a2g=0, a2s=0, a1g=0, a1s=0, lda1=0, out_f32=0, R=0, ldr=0, bias=0, alpha=1.0, act=0, ldc=0, var=10, tr=1, rope=0,
             cus=256):      # R: 1 an fp32 residual, 2 a bf16 operand
        buf = ctypes.create_string_buffer(4096)
        rc = f(0x1000, lda1 or K1, 0x2000, K1, K1, 0x3000 if K2 else None, K2, 0x4000 if K2 else None, K2, K2, a2g, a2s, a1g, a1s,
               0x5000, ldc or N, out_f32, 0x6000 if R else None, ldr or N, int(R == 1), 0x7000 if bias else None, M, N, alpha, act, var, tr, rope, cus, buf, 4096)
        assert rc == 0
        out = []
        for ln in buf.value.decode().splitlines():      # "gemm_nt_w4s_kernel<true, 0, false> 256 1 256 131072" -> "w4s<true, 0, false> 256"
            name, gx, gy = ln[:ln.rindex(">") + 1] if ">" in ln else ln.split()[0], *ln.rsplit(" ", 4)[1:3]
            out.append(name.replace("gemm_nt_", "").replace("_kernel", "") + f" {gx}" + (f"x{gy}" if gy != "1" else ""))
        return out

    def step(H, F, r, V, M):      # one decoder layer of the LoRA product path (forward, then the dgrads of the backward) and the head
        return [dict(M=M, N=3 * r, K1=H, alpha=2.0),                                   # t_qkv = x A_qkv^T
                dict(M=M, N=3 * H, K1=H, K2=3 * r, a2g=H, a2s=r, rope=2),              # q|k|v + LoRA tail, table-free rope
                dict(M=M, N=r, K1=H, alpha=2.0),                                       # t_o (K-folded)
                dict(M=M, N=H, K1=H, K2=r, out_f32=1, R=1),                            # o + tail into the fp32 residual stream
                dict(M=M, N=2 * r, K1=H, alpha=2.0),                                   # t_gu
                dict(M=M, N=2 * F, K1=H, K2=2 * r, a2g=F, a2s=r),                      # gate|up + tail
                dict(M=M, N=2 * F, K1=H, act=3, ldc=F),                                # gate|up with the SwiGLU pair epilogue (merged reference)
                dict(M=M, N=r, K1=F, alpha=2.0),                                       # t_d (K-folded)
                dict(M=M, N=H, K1=F, K2=r, out_f32=1, R=1),                            # down + tail, fp32 residual
                dict(M=M, N=r, K1=H, alpha=2.0),                                       # dt_d = dY B_d (K-folded)
                dict(M=M, N=F, K1=H, K2=r, act=4, R=2, ldr=2 * F, ldc=2 * F),          # d_act . W_d with the SwiGLU backward epilogue (R: bf16 [gate | up])
                dict(M=M, N=2 * r, K1=F, lda1=2 * F, a1g=r, a1s=F, alpha=2.0),         # dt_gu (grouped A)
                dict(M=M, N=H, K1=2 * F, K2=2 * r),                                    # d_n = d_gu W_gu + tail
                dict(M=M, N=r, K1=H, alpha=2.0),                                       # dt_o (K-folded)
                dict(M=M, N=H, K1=H, K2=r),                                            # d_attn = d_h W_o + tail
                dict(M=M, N=3 * r, K1=H, lda1=3 * H, a1g=r, a1s=H, alpha=2.0),         # dt_qkv (grouped A)
                dict(M=M, N=H, K1=3 * H, K2=3 * r),                                    # d_n = dqkv W_qkv + tail
                dict(M=M, N=V, K1=H, out_f32=1)]                                       # lm_head

    assert [plan(**k) for k in step(4096, 11008, 256, 32000, 32362)] == [
        ["w4<true, false, false> 381"],
        ["w4s<true, 3, false> 256"],
        ["w4<true, false, false> 254", "gemm_fold2_reduce 4046"],
        ["w4s<true, 0, false> 256"],
        ["w4<true, false, false> 254"],
        ["w4s<false, 0, false> 256"],
        ["w4s<false, 2, false> 256"],
        ["w4<true, false, false> 254", "gemm_fold2_reduce 4046"],
        ["w4s<true, 0, true> 256"],
        ["w4<true, false, false> 254", "gemm_fold2_reduce 4046"],
        ["w4s<true, 0, false> 256"],
        ["w4<true, false, true> 254"],
        ["w4s<true, 0, true> 256"],
        ["w4<true, false, false> 254", "gemm_fold2_reduce 4046"],
        ["w4s<true, 0, false> 256"],
        ["w4<true, false, false> 381"],
        ["w4s<true, 0, true> 256"],
        ["w4s<false, 0, false> 256", "tail64<8> 48"]]
    assert [plan(**k) for k in step(4096, 11008, 256, 32000, 24890)] == [
        ["w4<true, false, false> 256", "tail64<4> 608"],
        ["w4s<true, 3, false> 256"],
        ["w4<true, false, false> 196", "gemm_fold2_reduce 3112"],
        ["w4s<true, 0, false> 256", "tail64<4> 512"],
        ["w4<true, false, false> 196"],
        ["w4s<false, 0, false> 256"],
        ["w4s<false, 2, false> 256"],
        ["w4<true, false, false> 196", "gemm_fold2_reduce 3112"],
        ["w4s<true, 0, true> 256", "tail64<4> 512"],
        ["w4<true, false, false> 196", "gemm_fold2_reduce 3112"],
        ["w4s<true, 0, false> 256"],
        ["w4<true, false, true> 196"],
        ["w4s<true, 0, true> 256", "tail64<4> 512"],
        ["w4<true, false, false> 196", "gemm_fold2_reduce 3112"],
        ["w4s<true, 0, false> 256", "tail64<4> 512"],
        ["w4<true, false, false> 256", "tail64<4> 608"],
        ["w4s<true, 0, true> 256", "tail64<4> 512"],
        ["w4s<false, 0, false> 256"]]
    assert [plan(**k) for k in step(5120, 13824, 256, 32000, 17652)] == [
        ["w4<true, false, false> 207"],
        ["w4s<true, 3, false> 256"],
        ["w4<true, false, false> 138", "gemm_fold2_reduce 2207"],
        ["w4s<true, 0, false> 256"],
        ["kernel_x<64, true, 2> 552"],
        ["w4s<false, 0, false> 256", "tail64<4> 448"],
        ["w4s<false, 2, false> 256"],
        ["w4<true, false, false> 138", "gemm_fold2_reduce 2207"],
        ["w4s<false, 0, true> 256"],
        ["w4<true, false, false> 138", "gemm_fold2_reduce 2207"],
        ["w4s<true, 0, false> 256"],
        ["kernel_x<64, true, 2> 552"],
        ["w4s<false, 0, true> 256"],
        ["w4<true, false, false> 138", "gemm_fold2_reduce 2207"],
        ["w4s<true, 0, false> 256"],
        ["w4<true, false, false> 207"],
        ["w4s<false, 0, true> 256"],
        ["w4s<false, 0, false> 256"]]
    assert [plan(**k) for k in step(5120, 13824, 256, 32000, 13001)] == [
        ["w4<true, false, false> 153"],
        ["w4s<true, 3, false> 256"],
        ["w4<true, false, false> 102", "gemm_fold2_reduce 1626"],
        ["w4s<true, 0, false> 256"],
        ["kernel_x<64, true, 2> 408"],
        ["w4s<false, 0, false> 256"],
        ["w4s<false, 2, false> 256"],
        ["w4<true, false, false> 102", "gemm_fold2_reduce 1626"],
        ["w4s<false, 0, true> 256"],
        ["w4<true, false, false> 102", "gemm_fold2_reduce 1626"],
        ["w4s<true, 0, false> 256"],
        ["kernel_x<64, true, 2> 408"],
        ["w4s<false, 0, true> 256"],
        ["w4<true, false, false> 102", "gemm_fold2_reduce 1626"],
        ["w4s<true, 0, false> 256"],
        ["w4<true, false, false> 153"],
        ["w4s<false, 0, true> 256"],
        ["w4s<false, 0, false> 256"]]

    # N = 256 products below K = 1024 are not folded; the folded launch keeps its shape whatever the flags of the 256x256 kernel
    assert plan(M=32362, N=256, K1=768) == ["kernel_x<64, true, 2> 506"]
    assert plan(M=24890, N=256, K1=512, alpha=2.0) == ["kernel_x<64, true, 2> 390"]
    assert plan(M=32362, N=256, K1=4096, var=31) == ["w4<true, false, false> 254", "gemm_fold2_reduce 4046"]
    assert plan(M=32362, N=256, K1=11008, tr=2049) == ["w4<true, false, false> 254", "gemm_fold2_reduce 4046"]
    assert plan(M=32362, N=256, K1=11008, tr=1025) == ["w4<true, false, false> 254", "gemm_fold2_reduce 4046"]
    assert plan(M=40, N=256, K1=4096) == ["w4<true, false, false> 2", "gemm_fold2_reduce 5"]
    assert plan(M=32362, N=256, K1=4096, var=4) == ["kernel_x<64, true, 2> 506"]
    assert plan(M=32362, N=256, K1=4096, act=S) == ["kernel_x<64, true, 2> 506"]
    # vision tower (22 images x 577 positions) and projector (x 576): bias / activation epilogues
    assert plan(M=12694, N=1024, K1=640, bias=1) == ["w4<true, true, false> 200"]
    assert plan(M=12694, N=3072, K1=1024, bias=1) == ["w4<true, true, false> 600"]
    assert plan(M=12694, N=1024, K1=1024, bias=1, out_f32=1, R=1) == ["w4<true, true, false> 200"]
    assert plan(M=12694, N=4096, K1=1024, bias=1, act=1) == ["w4<true, true, false> 768", "tail64<4> 512"]
    assert plan(M=12694, N=1024, K1=4096, bias=1, out_f32=1, R=1) == ["w4<true, true, false> 200"]
    assert plan(M=12672, N=4096, K1=1024, bias=1, act=2) == ["w4<true, true, false> 768", "tail64<4> 512"]
    assert plan(M=12672, N=4096, K1=4096, bias=1) == ["w4<true, true, false> 768", "tail64<4> 512"]
    # tails of a multi-round launch: <= 16 tiles sixteenth tiles with the deep ring, <= 40 sixteenth tiles, <= 64 quarter tiles; a deep-K
    # one-round problem of 64-128 tiles as quarter tiles entirely (fp32 out: not folded)
    assert plan(M=4097, N=4096, K1=4096) == ["w4<true, false, false> 256", "tail64<8> 256"]
    assert plan(M=4097, N=4096, K1=11008, out_f32=1, R=1) == ["w4<true, false, true> 256", "tail64<8> 256"]
    assert plan(M=2305, N=8192, K1=4096) == ["w4<true, false, false> 256", "kernel_x<64, true, 2> 256"]
    assert plan(M=4097, N=12288, K1=4096) == ["w4s<true, 0, false> 256", "kernel_x<64, true, 2> 192"]
    assert plan(M=24890, N=256, K1=11008, out_f32=1) == ["kernel_x<64, true, 2> 392"]
    assert plan(M=4097, N=4096, K1=4096, var=31) == ["w4<true, false, false> 272"]
    # decode (stream hint), 7B projections: q|k|v, o (fp32 residual), gate|up, SwiGLU pair, down (fp32 residual), lm_head
    def decode(M):
        return [plan(M=M, N=12288, K1=4096, act=S), plan(M=M, N=4096, K1=4096, out_f32=1, R=1, act=S), plan(M=M, N=22016, K1=4096, act=S),
                plan(M=M, N=22016, K1=4096, act=S | 3, ldc=11008), plan(M=M, N=4096, K1=11008, out_f32=1, R=1, act=S),
                plan(M=M, N=32000, K1=4096, out_f32=1, act=S)]

    assert decode(1) == [["skinny8<1, 2, 8, false> 768"], ["skinny8<1, 2, 8, false> 256"], ["skinny8<1, 4, 4, false> 688"], ["skinny8<1, 2, 8, true> 1376"], ["skinny8<1, 2, 8, false> 256"], ["skinny8<1, 4, 4, false> 1000"]]
    assert decode(4) == [["skinny8<1, 2, 8, false> 768"], ["skinny8<1, 2, 8, false> 256"], ["skinny8<1, 4, 4, false> 688"], ["skinny8<1, 2, 8, true> 1376"], ["skinny8<1, 2, 8, false> 256"], ["skinny8<1, 4, 4, false> 1000"]]
    assert decode(8) == [["dec64x<1, 0, 3> 256"], ["skinny8<1, 2, 8, false> 256"], ["dec64x<1, 0, 8> 172"], ["dec64x<1, 2, 6> 230"], ["skinny8<1, 2, 8, false> 256"], ["dec64x<1, 1, 4> 500"]]
    assert decode(9) == [["dec64x<1, 0, 3> 256"], ["skinny8<2, 2, 4, false> 256"], ["dec64x<1, 0, 8> 172"], ["dec64x<1, 2, 6> 230"], ["skinny8<2, 2, 4, false> 256"], ["dec64x<1, 1, 4> 500"]]
    assert decode(16) == [["dec64x<1, 0, 3> 256"], ["skinny8<2, 2, 4, false> 256"], ["dec64x<1, 0, 8> 172"], ["dec64x<1, 2, 6> 230"], ["skinny8<2, 2, 4, false> 256"], ["dec64x<1, 1, 4> 500"]]
    assert decode(24) == [["dec64x<2, 0, 3> 256"], ["skinny8<3, 2, 2, false> 256"], ["dec64x<2, 0, 8> 172"], ["dec64x<2, 2, 6> 230"], ["skinny8<3, 2, 2, false> 256"], ["dec64x<2, 1, 4> 500"]]
    assert decode(32) == [["dec64x<2, 0, 3> 256"], ["skinny8<4, 2, 2, false> 256"], ["dec64x<2, 0, 8> 172"], ["dec64x<2, 2, 6> 230"], ["skinny8<4, 2, 2, false> 256"], ["dec64x<2, 1, 4> 500"]]
    assert decode(33) == [["dec64x<3, 0, 3> 256"], ["skinny<3, 1, 4, false> 256"], ["dec64x<3, 0, 8> 172"], ["dec64x<3, 2, 6> 230"], ["skinny<3, 1, 4, false> 256"], ["dec64x<3, 1, 4> 500"]]
    assert decode(64) == [["dec64x<4, 0, 3> 256"], ["skinny<4, 1, 4, false> 256"], ["dec64x<4, 0, 8> 172"], ["dec64x<4, 2, 6> 230"], ["skinny<4, 1, 4, false> 256"], ["dec64x<4, 1, 8> 250"]]
    # the flags the GPU tests cross-check with: gemm_variant 4 / 15 / 17 / 31, use_tr bits 3, 4, 5-6, 7-8, 10, 11, 12 (bits 0 and 3 belong to
    # gemm_tn and attention, bit 12 to the argument block: the kernels stay)
    assert plan(M=32362, N=12288, K1=4096, K2=768, a2g=4096, a2s=256, rope=2, var=4, tr=1) == ["w4s<true, 3, false> 256"]
    assert plan(M=32362, N=4096, K1=11008, K2=256, out_f32=1, R=1, var=4, tr=1) == ["kernel_x<64, true, 2> 8096"]
    assert plan(M=24890, N=22016, K1=4096, var=4, tr=1) == ["kernel_x<64, true, 2> 33540"]
    assert plan(M=2305, N=8192, K1=4096, var=4, tr=1) == ["kernel_x<64, true, 2> 1216"]
    assert plan(M=12694, N=4096, K1=1024, bias=1, act=1, var=4, tr=1) == ["kernel_x<64, true, 2> 3200"]
    assert plan(M=8, N=22016, K1=4096, act=S | 3, ldc=11008, var=4, tr=1) == ["w4<false, false, false> 86"]
    assert plan(M=24, N=12288, K1=4096, act=S, var=4, tr=1) == ["kernel_x<64, true, 2> 96"]
    assert plan(M=40, N=4096, K1=4096, out_f32=1, R=1, act=S, var=4, tr=1) == ["kernel_x<64, true, 2> 32"]
    assert plan(M=32362, N=12288, K1=4096, K2=768, a2g=4096, a2s=256, rope=2, var=15, tr=1) == ["w4s<true, 3, false> 256"]
    assert plan(M=32362, N=4096, K1=11008, K2=256, out_f32=1, R=1, var=15, tr=1) == ["w4s<true, 0, true> 256"]
    assert plan(M=24890, N=22016, K1=4096, var=15, tr=1) == ["w4s<false, 0, false> 256"]
    assert plan(M=2305, N=8192, K1=4096, var=15, tr=1) == ["w4<true, false, false> 256", "kernel_x<64, true, 2> 256"]
    assert plan(M=12694, N=4096, K1=1024, bias=1, act=1, var=15, tr=1) == ["p8 800"]
    assert plan(M=8, N=22016, K1=4096, act=S | 3, ldc=11008, var=15, tr=1) == ["skinny8<1, 2, 8, true> 1376"]
    assert plan(M=24, N=12288, K1=4096, act=S, var=15, tr=1) == ["skinny8<3, 2, 2, false> 768"]
    assert plan(M=40, N=4096, K1=4096, out_f32=1, R=1, act=S, var=15, tr=1) == ["skinny<3, 1, 4, false> 256"]
    assert plan(M=32362, N=12288, K1=4096, K2=768, a2g=4096, a2s=256, rope=2, var=17, tr=1) == ["w4s<true, 3, false> 256"]
    assert plan(M=32362, N=4096, K1=11008, K2=256, out_f32=1, R=1, var=17, tr=1) == ["p8 2032"]
    assert plan(M=24890, N=22016, K1=4096, var=17, tr=1) == ["p8 8428"]
    assert plan(M=2305, N=8192, K1=4096, var=17, tr=1) == ["p8 320"]
    assert plan(M=12694, N=4096, K1=1024, bias=1, act=1, var=17, tr=1) == ["p8 800"]
    assert plan(M=8, N=22016, K1=4096, act=S | 3, ldc=11008, var=17, tr=1) == ["w4<false, false, false> 86"]
    assert plan(M=24, N=12288, K1=4096, act=S, var=17, tr=1) == ["p8 48"]
    assert plan(M=40, N=4096, K1=4096, out_f32=1, R=1, act=S, var=17, tr=1) == ["p8 16"]
    assert plan(M=32362, N=12288, K1=4096, K2=768, a2g=4096, a2s=256, rope=2, var=31, tr=1) == ["w4<true, false, false> 6096"]
    assert plan(M=32362, N=4096, K1=11008, K2=256, out_f32=1, R=1, var=31, tr=1) == ["w4<true, false, true> 2032"]
    assert plan(M=24890, N=22016, K1=4096, var=31, tr=1) == ["w4<false, false, false> 8428"]
    assert plan(M=2305, N=8192, K1=4096, var=31, tr=1) == ["w4<true, false, false> 320"]
    assert plan(M=12694, N=4096, K1=1024, bias=1, act=1, var=31, tr=1) == ["w4<true, true, false> 800"]
    assert plan(M=8, N=22016, K1=4096, act=S | 3, ldc=11008, var=31, tr=1) == ["w4<false, false, false> 86"]
    assert plan(M=24, N=12288, K1=4096, act=S, var=31, tr=1) == ["w4<true, false, false> 48"]
    assert plan(M=40, N=4096, K1=4096, out_f32=1, R=1, act=S, var=31, tr=1) == ["w4<true, false, false> 16"]
    assert plan(M=32362, N=12288, K1=4096, K2=768, a2g=4096, a2s=256, rope=2, var=10, tr=0) == ["w4s<true, 3, false> 256"]
    assert plan(M=32362, N=4096, K1=11008, K2=256, out_f32=1, R=1, var=10, tr=0) == ["w4s<true, 0, true> 256"]
    assert plan(M=24890, N=22016, K1=4096, var=10, tr=0) == ["w4s<false, 0, false> 256"]
    assert plan(M=2305, N=8192, K1=4096, var=10, tr=0) == ["w4<true, false, false> 256", "kernel_x<64, true, 2> 256"]
    assert plan(M=12694, N=4096, K1=1024, bias=1, act=1, var=10, tr=0) == ["w4<true, true, false> 768", "tail64<4> 512"]
    assert plan(M=8, N=22016, K1=4096, act=S | 3, ldc=11008, var=10, tr=0) == ["dec64x<1, 2, 6> 230"]
    assert plan(M=24, N=12288, K1=4096, act=S, var=10, tr=0) == ["dec64x<2, 0, 3> 256"]
    assert plan(M=40, N=4096, K1=4096, out_f32=1, R=1, act=S, var=10, tr=0) == ["skinny<3, 1, 4, false> 256"]
    assert plan(M=32362, N=12288, K1=4096, K2=768, a2g=4096, a2s=256, rope=2, var=10, tr=9) == ["w4s<true, 3, false> 256"]
    assert plan(M=32362, N=4096, K1=11008, K2=256, out_f32=1, R=1, var=10, tr=9) == ["w4s<true, 0, true> 256"]
    assert plan(M=24890, N=22016, K1=4096, var=10, tr=9) == ["w4s<false, 0, false> 256"]
    assert plan(M=2305, N=8192, K1=4096, var=10, tr=9) == ["w4<true, false, false> 256", "kernel_x<64, true, 2> 256"]
    assert plan(M=12694, N=4096, K1=1024, bias=1, act=1, var=10, tr=9) == ["w4<true, true, false> 768", "tail64<4> 512"]
    assert plan(M=8, N=22016, K1=4096, act=S | 3, ldc=11008, var=10, tr=9) == ["dec64x<1, 2, 6> 230"]
    assert plan(M=24, N=12288, K1=4096, act=S, var=10, tr=9) == ["dec64x<2, 0, 3> 256"]
    assert plan(M=40, N=4096, K1=4096, out_f32=1, R=1, act=S, var=10, tr=9) == ["skinny<3, 1, 4, false> 256"]
    assert plan(M=32362, N=12288, K1=4096, K2=768, a2g=4096, a2s=256, rope=2, var=10, tr=17) == ["w4s<true, 3, false> 256"]
    assert plan(M=32362, N=4096, K1=11008, K2=256, out_f32=1, R=1, var=10, tr=17) == ["w4s<true, 0, true> 256"]
    assert plan(M=24890, N=22016, K1=4096, var=10, tr=17) == ["w4s<false, 0, false> 256"]
    assert plan(M=2305, N=8192, K1=4096, var=10, tr=17) == ["w4<true, false, false> 256", "kernel_x<64, true, 2> 256"]
    assert plan(M=12694, N=4096, K1=1024, bias=1, act=1, var=10, tr=17) == ["w4<true, true, false> 768", "tail64<4> 512"]
    assert plan(M=8, N=22016, K1=4096, act=S | 3, ldc=11008, var=10, tr=17) == ["dec64x<1, 2, 6> 230"]
    assert plan(M=24, N=12288, K1=4096, act=S, var=10, tr=17) == ["dec64x<2, 0, 3> 256"]
    assert plan(M=40, N=4096, K1=4096, out_f32=1, R=1, act=S, var=10, tr=17) == ["skinny<3, 1, 4, false> 256"]
    assert plan(M=32362, N=12288, K1=4096, K2=768, a2g=4096, a2s=256, rope=2, var=10, tr=33) == ["w4s<true, 3, false> 256"]
    assert plan(M=32362, N=4096, K1=11008, K2=256, out_f32=1, R=1, var=10, tr=33) == ["w4s<true, 0, true> 256"]
    assert plan(M=24890, N=22016, K1=4096, var=10, tr=33) == ["w4s<false, 0, false> 256"]
    assert plan(M=2305, N=8192, K1=4096, var=10, tr=33) == ["w4<true, false, false> 256", "kernel_x<64, true, 2> 256"]
    assert plan(M=12694, N=4096, K1=1024, bias=1, act=1, var=10, tr=33) == ["w4<true, true, false> 768", "tail64<4> 512"]
    assert plan(M=8, N=22016, K1=4096, act=S | 3, ldc=11008, var=10, tr=33) == ["skinny8<1, 2, 8, true> 1376"]
    assert plan(M=24, N=12288, K1=4096, act=S, var=10, tr=33) == ["skinny8<3, 2, 2, false> 768"]
    assert plan(M=40, N=4096, K1=4096, out_f32=1, R=1, act=S, var=10, tr=33) == ["skinny<3, 1, 4, false> 256"]
    assert plan(M=32362, N=12288, K1=4096, K2=768, a2g=4096, a2s=256, rope=2, var=10, tr=65) == ["w4s<true, 3, false> 256"]
    assert plan(M=32362, N=4096, K1=11008, K2=256, out_f32=1, R=1, var=10, tr=65) == ["w4s<true, 0, true> 256"]
    assert plan(M=24890, N=22016, K1=4096, var=10, tr=65) == ["w4s<false, 0, false> 256"]
    assert plan(M=2305, N=8192, K1=4096, var=10, tr=65) == ["w4<true, false, false> 256", "kernel_x<64, true, 2> 256"]
    assert plan(M=12694, N=4096, K1=1024, bias=1, act=1, var=10, tr=65) == ["w4<true, true, false> 768", "tail64<4> 512"]
    assert plan(M=8, N=22016, K1=4096, act=S | 3, ldc=11008, var=10, tr=65) == ["dec64<1, 2, 4, 1> 344"]
    assert plan(M=24, N=12288, K1=4096, act=S, var=10, tr=65) == ["dec64<2, 0, 4, 2> 384"]
    assert plan(M=40, N=4096, K1=4096, out_f32=1, R=1, act=S, var=10, tr=65) == ["skinny<3, 1, 4, false> 256"]
    assert plan(M=32362, N=12288, K1=4096, K2=768, a2g=4096, a2s=256, rope=2, var=10, tr=97) == ["w4s<true, 3, false> 256"]
    assert plan(M=32362, N=4096, K1=11008, K2=256, out_f32=1, R=1, var=10, tr=97) == ["w4s<true, 0, true> 256"]
    assert plan(M=24890, N=22016, K1=4096, var=10, tr=97) == ["w4s<false, 0, false> 256"]
    assert plan(M=2305, N=8192, K1=4096, var=10, tr=97) == ["w4<true, false, false> 256", "kernel_x<64, true, 2> 256"]
    assert plan(M=12694, N=4096, K1=1024, bias=1, act=1, var=10, tr=97) == ["w4<true, true, false> 768", "tail64<4> 512"]
    assert plan(M=8, N=22016, K1=4096, act=S | 3, ldc=11008, var=10, tr=97) == ["dec64x<1, 2, 6> 230"]
    assert plan(M=24, N=12288, K1=4096, act=S, var=10, tr=97) == ["dec64x<2, 0, 3> 256"]
    assert plan(M=40, N=4096, K1=4096, out_f32=1, R=1, act=S, var=10, tr=97) == ["skinny<3, 1, 4, false> 256"]
    assert plan(M=32362, N=12288, K1=4096, K2=768, a2g=4096, a2s=256, rope=2, var=10, tr=129) == ["w4s<true, 3, false> 256"]
    assert plan(M=32362, N=4096, K1=11008, K2=256, out_f32=1, R=1, var=10, tr=129) == ["w4s<true, 0, true> 256"]
    assert plan(M=24890, N=22016, K1=4096, var=10, tr=129) == ["w4s<false, 0, false> 256"]
    assert plan(M=2305, N=8192, K1=4096, var=10, tr=129) == ["w4<true, false, false> 256", "kernel_x<64, true, 2> 256"]
    assert plan(M=12694, N=4096, K1=1024, bias=1, act=1, var=10, tr=129) == ["w4<true, true, false> 768", "tail64<4> 512"]
    assert plan(M=8, N=22016, K1=4096, act=S | 3, ldc=11008, var=10, tr=129) == ["dec64x<1, 2, 6> 230"]
    assert plan(M=24, N=12288, K1=4096, act=S, var=10, tr=129) == ["dec64x<2, 0, 3> 256"]
    assert plan(M=40, N=4096, K1=4096, out_f32=1, R=1, act=S, var=10, tr=129) == ["skinny<3, 1, 4, false> 256"]
    assert plan(M=32362, N=12288, K1=4096, K2=768, a2g=4096, a2s=256, rope=2, var=10, tr=257) == ["w4s<true, 3, false> 256"]
    assert plan(M=32362, N=4096, K1=11008, K2=256, out_f32=1, R=1, var=10, tr=257) == ["w4s<true, 0, true> 256"]
    assert plan(M=24890, N=22016, K1=4096, var=10, tr=257) == ["w4s<false, 0, false> 256"]
    assert plan(M=2305, N=8192, K1=4096, var=10, tr=257) == ["w4<true, false, false> 256", "kernel_x<64, true, 2> 256"]
    assert plan(M=12694, N=4096, K1=1024, bias=1, act=1, var=10, tr=257) == ["w4<true, true, false> 768", "tail64<4> 512"]
    assert plan(M=8, N=22016, K1=4096, act=S | 3, ldc=11008, var=10, tr=257) == ["dec64x<1, 2, 4> 344"]
    assert plan(M=24, N=12288, K1=4096, act=S, var=10, tr=257) == ["dec64x<2, 0, 4> 192"]
    assert plan(M=40, N=4096, K1=4096, out_f32=1, R=1, act=S, var=10, tr=257) == ["skinny<3, 1, 4, false> 256"]
    assert plan(M=32362, N=12288, K1=4096, K2=768, a2g=4096, a2s=256, rope=2, var=10, tr=385) == ["w4s<true, 3, false> 256"]
    assert plan(M=32362, N=4096, K1=11008, K2=256, out_f32=1, R=1, var=10, tr=385) == ["w4s<true, 0, true> 256"]
    assert plan(M=24890, N=22016, K1=4096, var=10, tr=385) == ["w4s<false, 0, false> 256"]
    assert plan(M=2305, N=8192, K1=4096, var=10, tr=385) == ["w4<true, false, false> 256", "kernel_x<64, true, 2> 256"]
    assert plan(M=12694, N=4096, K1=1024, bias=1, act=1, var=10, tr=385) == ["w4<true, true, false> 768", "tail64<4> 512"]
    assert plan(M=8, N=22016, K1=4096, act=S | 3, ldc=11008, var=10, tr=385) == ["dec64x<1, 2, 8> 172"]
    assert plan(M=24, N=12288, K1=4096, act=S, var=10, tr=385) == ["dec64x<2, 0, 8> 96"]
    assert plan(M=40, N=4096, K1=4096, out_f32=1, R=1, act=S, var=10, tr=385) == ["skinny<3, 1, 4, false> 256"]
    assert plan(M=32362, N=12288, K1=4096, K2=768, a2g=4096, a2s=256, rope=2, var=10, tr=1025) == ["w4s<true, 3, false> 8"]
    assert plan(M=32362, N=4096, K1=11008, K2=256, out_f32=1, R=1, var=10, tr=1025) == ["w4s<true, 0, true> 8"]
    assert plan(M=24890, N=22016, K1=4096, var=10, tr=1025) == ["w4s<false, 0, false> 8"]
    assert plan(M=2305, N=8192, K1=4096, var=10, tr=1025) == ["w4s<true, 0, false> 8", "kernel_x<64, true, 2> 256"]
    assert plan(M=12694, N=4096, K1=1024, bias=1, act=1, var=10, tr=1025) == ["w4<true, true, false> 768", "tail64<4> 512"]
    assert plan(M=8, N=22016, K1=4096, act=S | 3, ldc=11008, var=10, tr=1025) == ["dec64x<1, 2, 6> 230"]
    assert plan(M=24, N=12288, K1=4096, act=S, var=10, tr=1025) == ["dec64x<2, 0, 3> 256"]
    assert plan(M=40, N=4096, K1=4096, out_f32=1, R=1, act=S, var=10, tr=1025) == ["skinny<3, 1, 4, false> 256"]
    assert plan(M=32362, N=12288, K1=4096, K2=768, a2g=4096, a2s=256, rope=2, var=10, tr=2049) == ["w4s<true, 3, false> 256"]
    assert plan(M=32362, N=4096, K1=11008, K2=256, out_f32=1, R=1, var=10, tr=2049) == ["w4<true, false, false> 2032"]
    assert plan(M=24890, N=22016, K1=4096, var=10, tr=2049) == ["w4s<false, 0, false> 256"]
    assert plan(M=2305, N=8192, K1=4096, var=10, tr=2049) == ["w4<true, false, false> 256", "kernel_x<64, true, 2> 256"]
    assert plan(M=12694, N=4096, K1=1024, bias=1, act=1, var=10, tr=2049) == ["w4<true, true, false> 768", "tail64<4> 512"]
    assert plan(M=8, N=22016, K1=4096, act=S | 3, ldc=11008, var=10, tr=2049) == ["dec64x<1, 2, 6> 230"]
    assert plan(M=24, N=12288, K1=4096, act=S, var=10, tr=2049) == ["dec64x<2, 0, 3> 256"]
    assert plan(M=40, N=4096, K1=4096, out_f32=1, R=1, act=S, var=10, tr=2049) == ["skinny<3, 1, 4, false> 256"]
    assert plan(M=32362, N=12288, K1=4096, K2=768, a2g=4096, a2s=256, rope=2, var=10, tr=4097) == ["w4s<true, 3, false> 256"]
    assert plan(M=32362, N=4096, K1=11008, K2=256, out_f32=1, R=1, var=10, tr=4097) == ["w4s<true, 0, true> 256"]
    assert plan(M=24890, N=22016, K1=4096, var=10, tr=4097) == ["w4s<false, 0, false> 256"]
    assert plan(M=2305, N=8192, K1=4096, var=10, tr=4097) == ["w4<true, false, false> 256", "kernel_x<64, true, 2> 256"]
    assert plan(M=12694, N=4096, K1=1024, bias=1, act=1, var=10, tr=4097) == ["w4<true, true, false> 768", "tail64<4> 512"]
    assert plan(M=8, N=22016, K1=4096, act=S | 3, ldc=11008, var=10, tr=4097) == ["dec64x<1, 2, 6> 230"]
    assert plan(M=24, N=12288, K1=4096, act=S, var=10, tr=4097) == ["dec64x<2, 0, 3> 256"]
    assert plan(M=40, N=4096, K1=4096, out_f32=1, R=1, act=S, var=10, tr=4097) == ["skinny<3, 1, 4, false> 256"]


def test_attention_routing_rule(built_lib):
    """Host-side kernel choice of the attention forward and backward, read through opadpo_debug_attn_plan (a test entry point outside the
    header: the launches as `kernel grid.x block LDS` lines; nothing is launched).  Pins kernel, grid and LDS at the benchmark's packed ragged
    shape (22 sequences of up to 1471 rows, 32362 rows, 32 heads of 128) and at the CLIP tower's (577 tokens, 16 heads of 64) under process
    words 0 / 1 / 3, and a context word with bit 8: the 16-row kernels, transposed reads from the context word, the LDS-DMA forward from the
    process word alone."""
    lib = ctypes.CDLL(built_lib)
    f = lib.opadpo_debug_attn_plan
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int] * 12 + [ctypes.c_char_p, ctypes.c_int]

    def plan(S, L, nh, hd, ld, ldo, rows=0, bwd=0, dq=1, dq_f32=0, tr=1, ctx=-1):
        buf = ctypes.create_string_buffer(1024)
        rc = f(S, L, nh, hd, ld, ldo, rows, bwd, dq, dq_f32, tr, ctx, buf, 1024)
        return buf.value.decode().splitlines() if rc == 0 else rc

    llm = dict(S=22, L=1471, nh=32, hd=128, ld=12288, ldo=4096, rows=32362)
    fwd32, dq32 = "attn_fwd32_kernel 8448 256 65696", "attn_bwd_dq32_kernel 8448 256 65696"
    delta = "attn_delta_kernel<128> 64724 256 0"
    for tr in (0, 1, 3):
        assert plan(**llm, tr=tr) == [fwd32]
    assert plan(**llm, bwd=1) == [delta, "attn_bwd_dkdv_kernel<128, true> 16192 256 66704", dq32]
    assert plan(**llm, bwd=1, dq_f32=1) == [delta, "attn_bwd_dkdv_kernel<128, true> 16192 256 66704", "attn_bwd_dq_kernel<128, true> 16192 256 0"]
    assert plan(**llm, bwd=1, dq=0, dq_f32=1) == [delta, "attn_bwd_dkdv_kernel<128, true> 16192 256 66704", "attn_bwd_dq_kernel<128, true> 16192 256 0"]
    assert plan(**llm, bwd=1, tr=0) == [delta, "attn_bwd_dkdv_kernel<128, false> 16192 256 66704", dq32]
    assert plan(**llm, bwd=1, tr=0, dq_f32=1) == [delta, "attn_bwd_dkdv_kernel<128, false> 16192 256 66704", "attn_bwd_dq_kernel<128, false> 16192 256 0"]
    assert plan(**llm, bwd=1, tr=3) == [delta, "attn_bwd_dkdv_kernel<128, true> 16192 256 66704", dq32]
    # context bit 8: the 16-row forward and dQ; transposed reads from the context word (bit 0), the DMA ring from the process word (bit 1)
    assert plan(**llm, tr=3, ctx=256) == ["attn_fwd_kernel<128, false, true> 16192 256 65696"]
    assert plan(**llm, tr=3, ctx=257) == ["attn_fwd_kernel<128, true, true> 16192 256 65696"]
    assert plan(**llm, tr=1, ctx=258) == ["attn_fwd_kernel<128, false, false> 16192 256 32848"]
    assert plan(**llm, tr=0, ctx=257) == ["attn_fwd_kernel<128, true, false> 16192 256 32848"]
    assert plan(**llm, tr=3, ctx=256, bwd=1) == [delta, "attn_bwd_dkdv_kernel<128, false> 16192 256 66704", "attn_bwd_dq_kernel<128, false> 16192 256 0"]
    assert plan(**llm, tr=0, ctx=1) == [fwd32]
    assert plan(**llm, tr=0, ctx=1, bwd=1) == [delta, "attn_bwd_dkdv_kernel<128, true> 16192 256 66704", dq32]
    # padded rows: the delta pass covers S * L rows
    assert plan(S=2, L=1087, nh=32, hd=128, ld=12288, ldo=4096, bwd=1)[0] == "attn_delta_kernel<128> 4348 256 0"
    clip = dict(S=22, L=577, nh=16, hd=64, ld=3072, ldo=1024)
    assert plan(**clip) == ["attn_fwd_kernel<64, true, false> 3520 256 16464"]
    assert plan(**clip, tr=0) == ["attn_fwd_kernel<64, false, false> 3520 256 16464"]
    assert plan(**clip, tr=3) == ["attn_fwd_kernel<64, true, true> 3520 256 32928"]
    assert plan(**clip, tr=3, ctx=256) == ["attn_fwd_kernel<64, false, true> 3520 256 32928"]
    assert plan(**clip, bwd=1) == ["attn_delta_kernel<64> 6347 256 0", "attn_bwd_dkdv_kernel<64, true> 3520 256 33936", "attn_bwd_dq_kernel<64, true> 3520 256 0"]
    # per-sequence extents past 2e9 bytes: the forward leaves the 32-row kernel and the DMA ring, the backward refuses
    assert plan(S=1, L=100000, nh=32, hd=128, ld=12288, ldo=4096, tr=3) == ["attn_fwd_kernel<128, true, false> 50016 256 32848"]
    assert plan(S=1, L=100000, nh=32, hd=128, ld=12288, ldo=4096, bwd=1) != 0 and plan(**dict(llm, hd=96)) != 0
    assert plan(**dict(llm, S=0)) == [] and plan(**dict(llm, L=0), bwd=1) == []


def test_generated_kloop_is_current():
    """opa-dpo_amd/csrc/w4_kloop.inc (the K-loop of gemm_nt_w4_kernel as an asm block) is generated: the committed file must be what the
    committed generator emits, and the generator's hazard checks (LDS stage reuse, fragment registers, M0, vmcnt bookkeeping) must hold."""
    import subprocess
    import sys
    gen = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "opa-dpo_amd", "csrc", "w4_kloop_gen.py")
    r = subprocess.run([sys.executable, gen, "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_kloop_generator_experiment_variants(tmp_path):
    """The generator's experiment variants (tools/build_kloop_exp.sh: W4K_EXP / W4K_OUT) pass its hazard checks too, never write the committed file, and the DEEP
    texts the library ships (W4K_/W4S_TEXT_*_DEEP) are in the committed file; the MFMA walk visits every accumulator exactly once per k-half in both directions."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gen = os.path.join(root, "opa-dpo_amd", "csrc", "w4_kloop_gen.py")
    inc = open(os.path.join(root, "opa-dpo_amd", "csrc", "w4_kloop.inc")).read()
    for name in ("W4K_TEXT_BFIRST", "W4K_TEXT_AFIRST", "W4K_TEXT_BFIRST_DEEP", "W4K_TEXT_AFIRST_DEEP", "W4S_TEXT_BFIRST", "W4S_TEXT_AFIRST", "W4S_TEXT_BFIRST_DEEP",
                 "W4S_TEXT_AFIRST_DEEP"):
        assert "#define " + name + " " in inc, name
    for exp in ("noadv", "early", "p3", "eb8p3l0w92", "eb5p3l3w96", "w96", "straight"):
        out = tmp_path / (exp + ".inc")
        r = subprocess.run([sys.executable, gen], capture_output=True, text=True, env=dict(os.environ, W4K_EXP=exp, W4K_OUT=str(out)))
        assert r.returncode == 0 and out.exists() and "v_mfma_f32_16x16x32_bf16" in out.read_text(), (exp, r.stdout + r.stderr)
    r = subprocess.run([sys.executable, gen], capture_output=True, text=True, env=dict(os.environ, W4K_EXP="noadv"))      # no W4K_OUT: refused
    assert r.returncode != 0
    sys.path.insert(0, os.path.dirname(gen))
    try:
        import w4_kloop_gen as g
        seen = {}
        for k in range(128):
            kk, i, j = g.mfma_ij(k)
            seen.setdefault(kk, []).append((i, j))
        assert sorted(seen[0]) == sorted(seen[1]) == [(i, j) for i in range(8) for j in range(8)]
        assert all(k < 64 for k in range(128) if g.mfma_ij(k)[0] == 0)                      # every k-half-0 MFMA before every k-half-1 one
        assert [g.mfma_ij(k)[2] for k in range(8, 16)] == list(range(7, -1, -1))            # odd rows walk the B fragments backwards
    finally:
        sys.path.pop(0)
