"""CPU: the host side of the rollout decode for 65..256 sequences per device - what opadpo_decode_begin accepts and refuses, the shape checks of
opadpo_gemm_nt_decode_wide, and its kernel choice read as text (no launch, no GPU)."""
import ctypes
import os

import pytest

EOS, PAD = 2, 0


@pytest.fixture(scope="module")
def built_lib():
    import importlib.util
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("opadpo_build", os.path.join(repo, "opa-dpo_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.build(verbose=False)


def _ctx(lib):
    from opadpo_amd.ctx import Dims
    good = Dims(256, 2, 2, 128, 384, 512, 1e-5, 10000.0, 128, 2, 2, 256, 56, 14, 1e-5, 128, 256.0)
    h = ctypes.c_void_p()
    assert lib.opadpo_ctx_create(ctypes.byref(good), 0, ctypes.byref(h)) == 0 and h.value
    return h


def _begin(lib, h, B):
    return lib.opadpo_decode_begin(h, 0, None, None, None, B, 8, 16, 1.0, 0, 1.0, 0, EOS, PAD, 0, None, None)


def test_decode_begin_accepts_up_to_256_rows(built_lib):
    """On a context without weights opadpo_decode_begin with 65 or 256 rows reaches the weights check (it no longer refuses the batch), and 257 rows
    are refused with text that names the bound."""
    from opadpo_amd import lib as L
    lib = L.load()
    h = _ctx(lib)
    try:
        for B in (1, 64, 65, 256):
            assert _begin(lib, h, B) != 0
            err = lib.opadpo_ctx_last_error(h)
            assert b"weights not set" in err and b"above" not in err, (B, err)
        for B in (257, 1000):
            assert _begin(lib, h, B) != 0
            err = lib.opadpo_ctx_last_error(h)
            assert b"256" in err and b"weights not set" not in err, (B, err)
    finally:
        lib.opadpo_ctx_destroy(h)


def test_armed_logit_processors_refuse_above_64_rows_and_disarm(built_lib):
    """opadpo_ctx_set_logit_processors + B = 65: refused with text before anything else is looked at; the refusal consumes the setting (B = 65 again
    reaches the weights check), and B = 64 armed is not refused for its batch."""
    from opadpo_amd import lib as L
    lib = L.load()
    h = _ctx(lib)
    try:
        ids, bias = (ctypes.c_int32 * 2)(5, 9), (ctypes.c_float * 2)(1.0, -1.0)
        assert lib.opadpo_ctx_set_logit_processors(h, ids, bias, 2, None, 0, None, 0) == 0
        assert _begin(lib, h, 65) != 0
        err = lib.opadpo_ctx_last_error(h)
        assert b"opadpo_ctx_set_logit_processors" in err and b"64" in err, err
        assert _begin(lib, h, 65) != 0 and b"weights not set" in lib.opadpo_ctx_last_error(h)
        assert lib.opadpo_ctx_set_logit_processors(h, ids, bias, 2, None, 0, None, 0) == 0
        assert _begin(lib, h, 64) != 0 and b"weights not set" in lib.opadpo_ctx_last_error(h)
    finally:
        lib.opadpo_ctx_destroy(h)


def test_gemm_nt_decode_wide_refusals(built_lib):
    """Shape validation before any launch: M outside 65..256, N not a multiple of 128, K not a multiple of 64, a bad mode or leading dimension
    return text; opadpo_gemm_nt_decode keeps its M <= 64 contract."""
    from opadpo_amd import lib as L
    lib = L.load()
    wide, narrow = lib.opadpo_gemm_nt_decode_wide, lib.opadpo_gemm_nt_decode
    p = 0x1000          # never dereferenced: every call below is refused on the host

    def err(fn, M, N=256, K=128, mode=0, lda=None, ldc=None):
        rc = fn(p, lda or K, p, K, K, p, ldc or N, mode, M, N, 1, None)
        assert rc != 0
        return lib.opadpo_last_error()

    for M in (64, 0, -1, 257):
        assert b"65..256" in err(wide, M)
    assert b"multiple of 128" in err(wide, 100, N=200)
    assert b"multiple of 128" in err(wide, 100, K=100)
    assert b"bad mode" in err(wide, 100, mode=3)
    assert b"misaligned" in err(wide, 100, lda=132)
    assert b"misaligned" in err(wide, 100, ldc=258)
    assert wide(None, 128, p, 128, 128, p, 256, 0, 100, 256, 1, None) != 0 and b"null operand" in lib.opadpo_last_error()
    assert b"0..64" in err(narrow, 65)


def test_gemm_nt_decode_wide_plan(built_lib):
    """Kernel choice of the two decode entry points, read through opadpo_debug_gemm_nt_decode_plan (a test entry point outside the header: the same
    validation, then `kernel grid.x grid.y block LDS`; nothing is launched).  gemm_nt_decw_kernel<G, mode, NW>: G = ceil(M / 64) groups of token rows
    (LDS = G x 32 KiB), NW x 16 weight rows per workgroup chosen by shape as for the <= 64-token kernel, the K-split that of (N, K) at any M."""
    lib = ctypes.CDLL(built_lib)
    lib.opadpo_last_error.restype = ctypes.c_char_p
    f = lib.opadpo_debug_gemm_nt_decode_plan
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int] * 6 + [ctypes.c_char_p, ctypes.c_int]

    def plan(M, N, K, mode, splits=0, tr=1):
        buf = ctypes.create_string_buffer(1024)
        if f(M, N, K, mode, splits, tr, buf, 1024) != 0:
            return None
        name, gx, gy, block, lds = buf.value.decode().strip().rsplit(" ", 4)
        return name.replace("gemm_nt_", "").replace("_kernel", "") + f" {gx}x{gy} {block} {lds}"

    def step7b(M):       # q|k|v, o (fp32 K-split), gate|up, gate|up SwiGLU pair, down (fp32 K-split), lm_head
        return [plan(M, 12288, 4096, 0), plan(M, 4096, 4096, 1), plan(M, 22016, 4096, 0), plan(M, 22016, 4096, 2), plan(M, 4096, 11008, 1),
                plan(M, 32000, 4096, 1, 1)]

    assert step7b(64) == ["dec64x<4, 0, 3> 256x1 320 65536", "dec64x<4, 1, 4> 64x4 384 65536", "dec64x<4, 0, 8> 172x1 640 65536",
                          "dec64x<4, 2, 6> 230x1 512 65536", "dec64x<4, 1, 4> 64x4 384 65536", "dec64x<4, 1, 8> 250x1 640 65536"]
    for M, G in ((65, 2), (128, 2), (129, 3), (192, 3), (193, 4), (256, 4)):
        lds = G * 32768
        assert step7b(M) == [f"decw<{G}, 0, 3> 256x1 320 {lds}", f"decw<{G}, 1, 4> 64x4 384 {lds}", f"decw<{G}, 0, 8> 172x1 640 {lds}",
                             f"decw<{G}, 2, 6> 230x1 512 {lds}", f"decw<{G}, 1, 4> 64x4 384 {lds}", f"decw<{G}, 1, 8> 250x1 640 {lds}"], M
    # the tiny model's projections at 130 rows, an explicit K-split, and the rows per workgroup forced through use_tr bits 7-8
    assert plan(130, 768, 256, 0) == "decw<3, 0, 3> 16x1 320 98304"
    assert plan(130, 768, 256, 2) == "decw<3, 2, 4> 12x1 384 98304"
    assert plan(130, 256, 384, 1) == "decw<3, 1, 4> 4x1 384 98304"
    assert plan(129, 1024, 704, 1, 3, 1 | (3 << 7)) == "decw<3, 1, 8> 8x3 640 98304"
    assert plan(129, 1024, 704, 2, 0, 1 | (2 << 7)) == "decw<3, 2, 4> 16x1 384 98304"
    assert plan(129, 22016, 128, 2) == "decw<3, 2, 6> 230x1 512 98304"
    assert plan(257, 256, 128, 0) is None and plan(100, 200, 128, 0) is None and plan(100, 256, 100, 0) is None and plan(100, 256, 128, 3) is None

