// LoRA dropout (PEFT lora.Linear: result += lora_B(lora_A(lora_dropout(x))) * scaling): the keep mask is a PURE FUNCTION of
// (seed, call, layer, module, row, col) - kernels.h "LoRA dropout" has the counter layout - so the forward, the backward of the same
// saved pass and tests/dropout_ref.py regenerate the same bits and no mask is ever stored.  HBM-streaming kernels: 16-byte accesses, every
// thread owns 8 consecutive columns of one row = two Philox-4x32-10 calls whose four words are four keep decisions each.
#include <algorithm>
#include "common.h"
#include "kernels.h"

namespace {

struct Philox4 { uint32_t x, y, z, w; };
// Philox-4x32-10 (Salmon et al., SC'11; Random123): multipliers D2511F53 / CD9E8D57, Weyl key increments 9E3779B9 / BB67AE85
__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return Philox4{c0, c1, c2, c3};
}

// keep bits of columns c8 .. c8 + 7 of one row (bit j = column c8 + j kept)
__device__ __forceinline__ uint32_t keep8(const LoraDropout& dp, uint32_t layer_module, uint32_t row, uint32_t c8) {
  const Philox4 a = philox4x32_10(c8 >> 2, row, dp.call_lo, dp.call_hi, dp.seed, layer_module);
  const Philox4 b = philox4x32_10((c8 >> 2) + 1u, row, dp.call_lo, dp.call_hi, dp.seed, layer_module);
  const uint32_t t = dp.thr;
  return (uint32_t)(a.x >= t) | (uint32_t)(a.y >= t) << 1 | (uint32_t)(a.z >= t) << 2 | (uint32_t)(a.w >= t) << 3 |
         (uint32_t)(b.x >= t) << 4 | (uint32_t)(b.y >= t) << 5 | (uint32_t)(b.z >= t) << 6 | (uint32_t)(b.w >= t) << 7;
}

// out[row, j*K + c] = keep_j(row, c) ? bf16(x[row, c] * scale) : 0 for the g modules module0 .. module0 + g - 1: x is read once
__global__ __launch_bounds__(256) void lora_dropout_fwd_kernel(const bf16_t* x, bf16_t* out, size_t rows, int K, int g, LoraDropout dp, int layer, int module0,
                                                                const int32_t* row_idx) {
  const int per_row = K / 8;
  const size_t total = rows * per_row;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const size_t row = idx / per_row;
    const int c8 = (int)(idx % per_row) * 8;
    const uint32_t rid = row_idx ? (uint32_t)row_idx[row] : (uint32_t)row;
    float f[8];
    unpack8(*(const uint4*)(x + row * K + c8), f);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] *= dp.scale;
    const uint4 scaled = pack8(f);                      // one bf16 rounding of x / (1 - p), as a bf16 nn.Dropout's output
    for (int m = 0; m < g; ++m) {
      const uint32_t kb = keep8(dp, (uint32_t)(layer * 8 + module0 + m), rid, (uint32_t)c8);
      uint4 o;                                          // a bf16 pair per word: column c8 + 2w in the low half
      o.x = scaled.x & ((kb & 1u ? 0xffffu : 0u) | (kb & 2u ? 0xffff0000u : 0u));
      o.y = scaled.y & ((kb & 4u ? 0xffffu : 0u) | (kb & 8u ? 0xffff0000u : 0u));
      o.z = scaled.z & ((kb & 16u ? 0xffffu : 0u) | (kb & 32u ? 0xffff0000u : 0u));
      o.w = scaled.w & ((kb & 64u ? 0xffffu : 0u) | (kb & 128u ? 0xffff0000u : 0u));
      *(uint4*)(out + row * (size_t)g * K + (size_t)m * K + c8) = o;
    }
  }
}

// dx[row, c] = bf16(dx[row, c] + sum_j keep_j(row, c) ? u[row, j*K + c] * scale : 0), fp32 sum in module order
__global__ __launch_bounds__(256) void lora_dropout_bwd_add_kernel(bf16_t* dx, const bf16_t* u, size_t rows, int K, int g, LoraDropout dp, int layer, int module0,
                                                                    const int32_t* row_idx) {
  const int per_row = K / 8;
  const size_t total = rows * per_row;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const size_t row = idx / per_row;
    const int c8 = (int)(idx % per_row) * 8;
    const uint32_t rid = row_idx ? (uint32_t)row_idx[row] : (uint32_t)row;
    float acc[8];
    unpack8(*(const uint4*)(dx + row * K + c8), acc);
    for (int m = 0; m < g; ++m) {
      const uint32_t kb = keep8(dp, (uint32_t)(layer * 8 + module0 + m), rid, (uint32_t)c8);
      float f[8];
      unpack8(*(const uint4*)(u + row * (size_t)g * K + (size_t)m * K + c8), f);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += (kb >> j & 1u) ? __fmul_rn(f[j], dp.scale) : 0.f;      // product rounded on its own (no fma): the sum is the fp32 restatement's
    }
    *(uint4*)(dx + row * K + c8) = pack8(acc);
  }
}

inline unsigned dropout_grid(size_t items) {
  const size_t blocks = (items + 255) / 256;
  return (unsigned)std::min<size_t>(std::max<size_t>(blocks, 1), 256 * 32);
}

}  // namespace

int lora_dropout_make(double p, uint64_t seed, uint64_t call, LoraDropout* out) {
  if (!(p >= 0.0) || !(p < 1.0) || seed > 0xffffffffull) return 1;
  out->thr = (uint32_t)(p * 4294967296.0);            // floor(p * 2^32): p < 1 keeps it below 2^32
  out->scale = (float)(1.0 / (1.0 - p));
  out->seed = (uint32_t)seed;
  out->call_lo = (uint32_t)call; out->call_hi = (uint32_t)(call >> 32);
  return 0;
}

static hipError_t dropout_check(const void* a, const void* b, int rows, int K, int g, int layer, int module0) {
  if (!a || !b) return hipErrorInvalidValue;
  if (K <= 0 || K % 8 || g < 1 || module0 < 0 || module0 + g > 7 || layer < 0 || layer >= (1 << 28)) return hipErrorInvalidValue;
  (void)rows;
  return hipSuccess;
}

hipError_t launch_lora_dropout_fwd(const bf16_t* x, bf16_t* out, int rows, int K, int g, const LoraDropout& dp, int layer, int module0, const int32_t* row_idx,
                                   hipStream_t st) {
  if (rows <= 0) return hipSuccess;
  const hipError_t e = dropout_check(x, out, rows, K, g, layer, module0);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(lora_dropout_fwd_kernel, dim3(dropout_grid((size_t)rows * (K / 8))), dim3(256), 0, st, x, out, (size_t)rows, K, g, dp, layer, module0, row_idx);
  return hipGetLastError();
}

hipError_t launch_lora_dropout_bwd_add(bf16_t* dx, const bf16_t* u, int rows, int K, int g, const LoraDropout& dp, int layer, int module0, const int32_t* row_idx,
                                       hipStream_t st) {
  if (rows <= 0) return hipSuccess;
  const hipError_t e = dropout_check(dx, u, rows, K, g, layer, module0);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(lora_dropout_bwd_add_kernel, dim3(dropout_grid((size_t)rows * (K / 8))), dim3(256), 0, st, dx, u, (size_t)rows, K, g, dp, layer, module0,
                     row_idx);
  return hipGetLastError();
}
