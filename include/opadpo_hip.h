/* libopadpo_hip.so — C ABI of the MI355X (gfx950) OPA-DPO hot path.
 *
 * The reference (zhyang2226/OPA-DPO) has no FFI: its hot path is the Python call
 * `self.base_model(**inputs)` inside AutoregressivePolicy.forward
 * (opadpo/dpo_models/rl_models.py:114-120) plus loss.backward()/optimizer.step()
 * (opadpo/dpo_models/rl_trainer.py:155-175), all of which lands in third-party CUDA wheels
 * (torch/cuBLAS, flash-attn, peft, bitsandbytes).  This header is the seam a maintainer binds
 * instead (ctypes stub: INTEGRATION.md).  Every entry point:
 *   - is plain `extern "C"`: raw device pointers + sizes, no torch / C++ types;
 *   - is asynchronous on the `hipStream_t` passed as `void* stream` (torch's current stream);
 *   - borrows all memory (the caller — torch-ROCm — owns and keeps it alive);
 *   - returns 0 on success, a non-zero hipError_t otherwise (`opadpo_last_error()` = text);
 *     it never aborts and never falls back to a CPU path.
 * bf16 tensors are `uint16_t` bit patterns (torch.bfloat16).  "ld*" = leading dimension in
 * elements.  Token ids are int32, pad id 0, image token -200 (utils/constants.py:28).
 */
#ifndef OPADPO_HIP_H
#define OPADPO_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OPADPO_ABI_VERSION 2      /* 2 (round 5): + opadpo_ctx_wgrad_deterministic, opadpo_allreduce_grads / _reduce_scatter_grads / _all_gather_params; opadpo_gemm_tn_group_workspace_bytes is 0 for MIXED lists too; context flag bits 13 / 14 (residual adds / SwiGLU backward as their own passes) and bit 6 = the STAGED SwiGLU-backward epilogue */
#define OPADPO_ACT_NONE 0
#define OPADPO_ACT_QUICK_GELU 1 /* CLIP MLP  (transformers activations.py quick_gelu) */
#define OPADPO_ACT_GELU 2       /* mm_projector mlp2x_gelu (erf GELU) */
#define OPADPO_ACT_SWIGLU_PAIR 3 /* gemm_nt only: B rows arranged per 128 as [64 gate | 64 up]; C gets N/2 columns
                                 * silu(gate) * up (SwiGLU of modeling_llama.LlamaMLP fused into the gate|up projection; used
                                 * for the merged, no-grad reference pass and, with OPADPO_GEMM_STREAM, for decode with a
                                 * merged adapter).  Needs N % 256 == 0, bf16 C, no bias / residual / LoRA tail, alpha = 1. */
#define OPADPO_ATTN_SKIP_MASKED_Q 2 /* OR into `causal` of opadpo_attn_fwd / _bwd: a tile of 64 query positions that are ALL masked as keys
                                    * (the trailing padding of a right-padded response) writes zeros (forward: O, backward: dQ) and is left
                                    * out of the dK / dV accumulation - exact for the LLM, where such rows are padding whose outputs nobody
                                    * reads and whose output gradient is zero; needs key_mask */
#define OPADPO_ACT_SWIGLU_BWD 4 /* gemm_nt only (N a multiple of 256, bf16 out, alpha 1, no bias): the product is d_act [M,N], R (bf16, ldr) holds the
                                * stored pre-activations [gate | up] = [M,2N] and C (ldc) receives [d_gate | d_up] = [M,2N]: opadpo_silu_mul_bwd applied
                                * in the epilogue on the bf16-rounded d_act tile (bit-identical to the two-call form, d_act never written) */
#define OPADPO_GEMM_STREAM 0x100 /* OR into `act`: M <= 64 (one token per sequence, KV-cache decode) -> weight-streaming
                                  * schedule (one workgroup per 16/32 weight rows, K split over its waves); from 8 token rows a
                                  * problem with nothing fused (no LoRA tail, bias, residual or scale; plain or SWIGLU_PAIR store) runs on
                                  * the whole-line kernel of opadpo_gemm_nt_decode, bit-identical to that entry point */

int opadpo_abi_version(void);
const char* opadpo_last_error(void);
/* process-default kernel-variant switches of the op-level entry points (a context carries its own: opadpo_ctx_set_flags):
 * use_glds = gemm_nt variant (10 = auto (default), 4 = 128x128 kernel, 17 = 8-wave 256x256 kernel, 31 = 4-wave 256x256 kernel forced,
 * 15 = M <= 64 weight-streaming kernel); use_tr bit 0 = ds_read_b64_tr_b16 transposed LDS reads in attention / gemm_tn, bit 1 =
 * attention forward through a direct-to-LDS double-buffered K/V ring (default: register-staged single buffer, which keeps 3 blocks
 * per CU), bit 3 = 128x128 gemm_tn kernel instead of the default 256x256 one, bit 4 = 16-row weight-streaming decode GEMM also for
 * M <= 16 (default there: the whole-cache-line 8-row form), bits 5-6 = kernel behind opadpo_gemm_nt_decode (0 = the library's choice,
 * 1 = the LDS-ring kernel of rounds 2-4, 3 = the whole-line streaming kernel gemm_nt_dec64x = the library's choice; A/B runs and tests), bits 7-8 = weight rows per workgroup of that kernel (0 = by shape, 1 / 2 / 3 =
 * 48 / 64 / 128 rows; tests), bit 9 = opadpo_sample runs its full vocabulary sweeps instead of the one-wave tail on the kept tokens (identical draws; the
 * exactness test's yardstick; a process switch, so eager and graph-captured launches always agree), bit 10 = the streaming 256x256 GEMM runs on 8
 * workgroups instead of one per CU (tests: long tile walks per workgroup on small problems; results are bit-identical for any workgroup count),
 * bit 11 = the gemm_nt products of >= 128 K-tiles (down projection, the dgrads) keep the default K-loop text of the 256x256 kernel; clear (default since round 6):
 * they run its DEEP text - another placement of the same loads, barriers and MFMAs, bit-identical results, +2-3 % there.
 * (Round 5 used bit 11 for an experimental 64-rows-per-wave attention forward, measured slower and removed.)
 * bit 12 = the 256x256 gemm_nt kernels deal their tile order to the XCDs in contiguous chunks (rounds 1-5); clear (default since round 6): 32-tile blocks dealt
 * block-cyclically, so that the eight XCDs of a round share one row group's A panels through the Infinity Cache - bit-identical results, -1.0 % per training step. */
void opadpo_set_flags(int use_glds, int use_tr);

/* ---- Linear layers: base GEMM with the LoRA branch fused by K-concatenation ----------------
 * C[M,N] = act(alpha * (A1[M,K1].B1[N,K1]^T + A2[M,K2].B2[N,K2]^T) + bias) + R
 * replaces nn.Linear + peft.tuners.lora.Linear.forward (y = xW^T + (alpha/r)(xA^T)B^T) reached
 * from rl_models.py:120, and their dgrad in backward (rl_trainer.py:162).
 * A2's column offset for output column n0 is (n0 / a2_group_n) * a2_group_stride (fused q|k|v and
 * gate|up projections); pass a2_group_n = 0 for a single group.  A1 can be grouped the same way
 * (a1_group_n / a1_group_stride: block-diagonal dT = dY_g . B_g of the fused projections in one launch).  N % 128 == 0, K1 % 64 == 0,
 * K2 % 64 == 0; M arbitrary.  out_f32: C is float32 instead of bf16; res_f32: R is float32 (the LLM
 * residual stream is kept in fp32 so bf16 rounding does not accumulate over 2*n_layers additions). */
int opadpo_gemm_nt(const uint16_t* A1, int lda1, const uint16_t* B1, int ldb1, int K1,
                   const uint16_t* A2, int lda2, const uint16_t* B2, int ldb2, int K2,
                   int a2_group_n, int a2_group_stride, int a1_group_n, int a1_group_stride,
                   void* C, int ldc, int out_f32, const void* R, int ldr, int res_f32, const uint16_t* bias,
                   int M, int N, float alpha, int act, void* stream);

/* The fused q|k|v projection with the rotary embedding applied in its epilogue (modeling_llama.LlamaAttention: q_proj / k_proj /
 * v_proj followed by apply_rotary_pos_emb on q and k): C[M,N] bf16 = A1 B1^T (+ A2[:, group] B2^T), then columns [0, rope_cols)
 * - heads of 128 - are rotated with the position of their row: pos = row % L, and with seg_len > 0 every response of a packed
 * row restarts at seg_prefix (same convention as opadpo_rope / opadpo_attn_fwd); cos_tab / sin_tab [>= L][64] fp32.  The
 * rotation reads the bf16-rounded projection, as opadpo_rope does on the stored tensor.  N % 256 == 0; alpha = 1, no bias,
 * residual or activation. */
int opadpo_gemm_nt_rope(const uint16_t* A1, int lda1, const uint16_t* B1, int ldb1, int K1,
                        const uint16_t* A2, int lda2, const uint16_t* B2, int ldb2, int K2, int a2_group_n, int a2_group_stride,
                        uint16_t* C, int ldc, int M, int N, const float* cos_tab, const float* sin_tab, int L, int rope_cols,
                        int seg_prefix, int seg_len, void* stream);

/* The same projection with a TABLE-FREE rotary epilogue (round 3; what the context's ragged passes run): the position of every output
 * row comes from row_pos [M] int32 (device), the angles are computed in the epilogue - v_sin / v_cos of the fractional revolution
 * pos * theta^(-2i/128) / 2pi per (row, frequency), a function of those two numbers only (a row's bits do not depend on its place in the
 * batch).  No cos / sin traffic, no position arithmetic: ~3 us per 256x256 block instead of 7.7; angles within max(2e-4, 3e-7 * pos) rad of HF's
 * fp32 tables: every fp32 rounding of the product pos * frequency is relative, so the error grows with the position - an fp32 emulation of the formula
 * with an exact exp2 gives 1.2e-7 * pos (2e-4 rad up to position 1600, 4.2e-4 at 4095), and one unit of the hardware exp2 is allowed for on top - the
 * figure is derived, an upper bound.  Measured on an MI355X against float64 (tests/test_gemm_exact_gpu.py): 2.6e-4 rad over positions up to 4095, at most
 * 7.8e-8 * pos (the bf16 rounding of the result is 4e-3 relative). */
int opadpo_gemm_nt_rope_pos(const uint16_t* A1, int lda1, const uint16_t* B1, int ldb1, int K1,
                            const uint16_t* A2, int lda2, const uint16_t* B2, int ldb2, int K2, int a2_group_n, int a2_group_stride,
                            uint16_t* C, int ldc, int M, int N, const int32_t* row_pos, float theta, int rope_cols, void* stream);

/* Decode projection for up to 64 tokens (rollout at 9..64 sequences per device, online_generator.py:292-309): C = A[M,K] . B[N,K]^T,
 * no bias / residual / LoRA tail (adapter-free or merged adapter).  A weight stream: 48 / 64 / 128 weight rows (by shape) x <= 64 tokens x
 * one K-slice per workgroup, the weights loaded global -> registers in whole 128-byte lines, the activations shared through LDS in
 * 256-deep chunks by two loader waves (gemm_nt_dec64x_kernel, round 4; opadpo_set_flags use_tr bits 5-6 = 1 selects the LDS-ring kernel
 * of rounds 2-4).  mode 0: bf16 C[M,N]; mode 1: fp32 partial tiles
 * C[splits][M,N] (ldc = row stride of one slice) - K is split over `splits` workgroups (<= 0: chosen by the library, query it with
 * opadpo_gemm_nt_decode_splits) and the consumer adds the slices (opadpo_rmsnorm_sum_fwd); mode 2: OPADPO_ACT_SWIGLU_PAIR weight
 * layout -> bf16 C[M, N/2] = silu(gate) * up.  M <= 64, N % 128 == 0, K % 64 == 0. */
int opadpo_gemm_nt_decode(const uint16_t* A, int lda, const uint16_t* B, int ldb, int K, void* C, int ldc, int mode, int M, int N, int splits,
                          void* stream);
int opadpo_gemm_nt_decode_splits(int N, int K, int splits);
/* The same projection for 65 <= M <= 256 tokens (rollout at 65..256 sequences per device): arguments, modes, `splits` and the shape rules of
 * opadpo_gemm_nt_decode - N % 128 == 0, K % 64 == 0, lda / ldb % 8 == 0, ldc % 4 == 0 - with M in 65..256; a bad shape returns text and launches
 * nothing.  A weight stream too (gemm_nt_decw_kernel): a workgroup owns 48 / 64 / 96 / 128 weight rows (by shape) x one K-slice, loads them global ->
 * registers in whole 128-byte lines exactly once per launch, and uses each k-tile's operand against ceil(M / 64) groups of 64 token rows staged through LDS
 * (two stages of 64 * groups rows x 128 deep).  The K-split is opadpo_gemm_nt_decode_splits(N, K, splits) - a function of (N, K) alone - and every output
 * element is summed in the k order of the <= 64-token kernel: row i of the result is bit-identical for every M that contains it, and to what
 * opadpo_gemm_nt_decode computes for that row. */
int opadpo_gemm_nt_decode_wide(const uint16_t* A, int lda, const uint16_t* B, int ldb, int K, void* C, int ldc, int mode, int M, int N, int splits,
                               void* stream);
/* x_out = resid + sum_s partials[s] (fp32 [rows,H]; resid fp32 or bf16), y (nullable) = RMSNorm(x_out) * w in bf16, rstd (nullable):
 * the residual add + LlamaRMSNorm behind a K-split decode projection; fixed summation order (deterministic). */
int opadpo_rmsnorm_sum_fwd(const void* resid, int resid_f32, const float* partials, int n_partials, size_t partial_stride, const uint16_t* w,
                           float* x_out, uint16_t* y, float* rstd, int rows, int H, float eps, void* stream);

/* LoRA weight gradients: C[N1,N2] (fp32) += alpha * sum_m P[m,N1] * Q[m,N2]   (dB = dY^T t,
 * dA = dT^T x; autograd of peft lora_A / lora_B, rl_trainer.py:162).  Q column offset for output
 * row n1 is (n1 / q_group_n1) * q_group_stride.  N1 % 128 == 0, N2 % 128 == 0. splits<=0: auto. */
int opadpo_gemm_tn(const uint16_t* P, int ldp, const uint16_t* Q, int ldq, float* C, int ldc,
                   int M, int N1, int N2, int q_group_n1, int q_group_stride, float alpha, int splits,
                   void* stream);
/* Up to 8 such products that share M (the 8 LoRA wgrads of one decoder layer) as ONE launch: their 256x256 tile lists are
 * concatenated, so a workgroup's run is long and the fp32-atomic flushes are rare (an r-wide output launched alone is cut into 16
 * K-chunks whose flush takes as long as their K-loop).  Host arrays of n entries; problems that do not fit the 256x256 kernel
 * (N1, N2, q_group_n1 % 256) make the call fall back to n single launches. */
int opadpo_gemm_tn_group(int n, const uint16_t* const* P, const int* ldp, const uint16_t* const* Q, const int* ldq, float* const* C, const int* ldc,
                         int M, const int* N1, const int* N2, const int* q_group_n1, const int* q_group_stride, float alpha, void* stream);
/* DETERMINISTIC form (round 4; what opadpo_seq_logprobs_bwd uses): a workgroup's partial tiles go to `workspace` as plain stores and a
 * second launch adds the partial tiles of every output tile in a fixed order - no fp32 atomics, C bit-reproducible run to run (accelerate /
 * PEFT gradients of the reference are deterministic too unless cuBLAS split-K is in play; dpo_trainer.py:847-849 accumulates them in place).
 * The problems must all run on the 256x256 kernel (N1, N2, q_group_n1 % 256 == 0); `_workspace_bytes` returns 0 otherwise.  The workspace
 * is scratch: free again when the call's kernels have run (stream order). */
size_t opadpo_gemm_tn_group_workspace_bytes(int n, int M, const int* N1, const int* N2, const int* q_group_n1);
int opadpo_gemm_tn_group_det(int n, const uint16_t* const* P, const int* ldp, const uint16_t* const* Q, const int* ldq, float* const* C, const int* ldc,
                             int M, const int* N1, const int* N2, const int* q_group_n1, const int* q_group_stride, float alpha,
                             void* workspace, size_t workspace_bytes, void* stream);

/* ---- attention (flash-attn 2.5.3 LlamaFlashAttention2 / CLIP eager attention) -------------------
 * q,k,v: element (s,pos,head,d) at ptr[(s*L+pos)*ld + head*hd + d]; o/dout with ldo.
 * key_mask [S,L] bytes (NULL = all keys valid); causal: key pos <= query pos.  hd in {64,128}.
 * lse [S,nh,L] fp32 (may be NULL in forward when no backward follows).
 * seg_len > 0 (needs causal): every row is [prefix of seg_prefix positions | response 0 | response 1 | ...], each response
 * seg_len long; a response attends the prefix and itself only — the K responses of a DPO sample (rl_models.py:95-112 stacks
 * them as K separate sequences) share ONE pass over the image + query prefix.  seg_len = 0: plain sequences. */
int opadpo_attn_fwd(const uint16_t* q, const uint16_t* k, const uint16_t* v, int ld, uint16_t* o, int ldo,
                    float* lse, const uint8_t* key_mask, int S, int L, int nh, int hd, int causal, float scale,
                    int seg_prefix, int seg_len, void* stream);
/* dq/dk/dv: bf16 with the q/k/v addressing (ld); dq_f32: optional fp32 copy of dQ [S*L, nh*hd]
 * (NULL in the product path); delta: fp32 scratch [S,nh,L].  Atomic-free (two passes: dK/dV, dQ). */
int opadpo_attn_bwd(const uint16_t* q, const uint16_t* k, const uint16_t* v, int ld, const uint16_t* o,
                    const uint16_t* dout, int ldo, const float* lse, const uint8_t* key_mask,
                    uint16_t* dq, uint16_t* dk, uint16_t* dv, float* dq_f32, float* delta,
                    int S, int L, int nh, int hd, int causal, float scale, int seg_prefix, int seg_len, void* stream);

/* ---- norms / rotary / SwiGLU (transformers modeling_llama.py / modeling_clip.py) -------------- */
/* x: bf16 or (x_f32) float32 rows; y bf16; rstd fp32 [rows] (nullable). */
int opadpo_rmsnorm_fwd(const void* x, int x_f32, const uint16_t* w, uint16_t* y, float* rstd, int rows, int H, float eps, void* stream);
/* dx = rmsnorm'(dy) + dres; written as float32 (dx_f32, nullable) and/or bf16 (dx_bf16, nullable). */
int opadpo_rmsnorm_bwd(const uint16_t* dy, const void* x, int x_f32, const uint16_t* w, const float* rstd,
                       const void* dres, int dres_f32, float* dx_f32, uint16_t* dx_bf16, int rows, int H, void* stream);
int opadpo_layernorm_fwd(const uint16_t* x, const uint16_t* w, const uint16_t* b, uint16_t* y, int rows, int H, float eps, void* stream);
/* fp32 input (the CLIP tower's residual stream is fp32 in the DPO path, round 4); y bf16 (y_f32 = 0: the operand of the next GEMM) or fp32
 * (y_f32 = 1: the pre-LayerNorm, whose output IS the residual stream) */
int opadpo_layernorm_fwd_f32(const float* x, const uint16_t* w, const uint16_t* b, void* y, int y_f32, int rows, int H, float eps, void* stream);
/* CLIP / projector training path (OPA LoRA-SFT stage, opadpo/opa_train.py: the vision tower and mm_projector carry trainable
 * LoRA there): LayerNorm backward w.r.t. x (affine parameters frozen; mean / rstd recomputed; dres nullable = residual-path
 * gradient, added), and the activation applied / differentiated on a stored PRE-activation tensor (act = OPADPO_ACT_*). */
int opadpo_layernorm_bwd(const uint16_t* dy, const uint16_t* x, const uint16_t* w, const uint16_t* dres, uint16_t* dx, int rows, int H,
                         float eps, void* stream);
int opadpo_act_fwd(const uint16_t* z, uint16_t* out, size_t n, int act, void* stream);
int opadpo_act_bwd(const uint16_t* dout, const uint16_t* z, uint16_t* dz, size_t n, int act, void* stream);
/* in-place half-split rotary on n_heads heads starting at column 0 of qk (row r has position
 * pos_base[0] + r % L; pos_base is a device int32 or NULL = 0 — device-resident so that a captured decode step can be
 * replayed); cos/sin: fp32 [max_pos, hd/2]; inverse=1 applies the transposed rotation (gradient).  seg_len > 0: packed
 * responses (see opadpo_attn_fwd) — positions >= seg_prefix + seg_len wrap back so every response starts at seg_prefix. */
int opadpo_rope(uint16_t* qk, int ld, const float* cos_tab, const float* sin_tab, int rows, int L, int n_heads, int hd,
                int inverse, const int32_t* pos_base, int seg_prefix, int seg_len, void* stream);
int opadpo_silu_mul_fwd(const uint16_t* gu, uint16_t* act, int rows, int F, void* stream);   /* gu = [gate | up] */
int opadpo_silu_mul_bwd(const uint16_t* dact, const uint16_t* gu, uint16_t* dgu, int rows, int F, void* stream);
/* LoRA dropout (PEFT lora.Linear: the LoRA branch reads dropout(x)).  The keep mask is a pure function, never stored:
 *   keep(seed, call, layer, module, row, col) = philox4x32_10(counter, key)[col & 3] >= floor(p * 2^32)      (unsigned compare)
 *   counter = (col >> 2, row, call & 0xffffffff, call >> 32), key = (seed, layer * 8 + module); seed < 2^32, 0 <= p < 1, module 0..6 = q k v o gate up down.
 * opadpo_lora_dropout_fwd: out [rows, g*K] = g masked copies of x [rows, K] side by side for modules module0 .. module0 + g - 1 (module0 + g <= 7, K % 8 == 0);
 * a kept element is bf16(x * fp32(1 / (1 - p))) (one rounding), a dropped one 0.  row_idx (nullable, int32 [rows]): the row number every row hashes with
 * (default: its index).  opadpo_lora_dropout_bwd_add: dx [rows, K] += sum_j keep_j * u[:, j*K : (j+1)*K] * fp32(1 / (1 - p)), fp32 sum in module order. */
int opadpo_lora_dropout_fwd(const uint16_t* x, uint16_t* out, int rows, int K, int g, double p, uint64_t seed, uint64_t call, int layer, int module0,
                            const int32_t* row_idx, void* stream);
int opadpo_lora_dropout_bwd_add(uint16_t* dx, const uint16_t* u, int rows, int K, int g, double p, uint64_t seed, uint64_t call, int layer, int module0,
                                const int32_t* row_idx, void* stream);

/* ---- embedding gather + multimodal splice (LLaVA prepare_inputs_labels_for_multimodal) ------------
 * ids/text_mask [S,n_txt]; each row holds exactly one image_token, replaced by the P rows
 * feats[feat_row[s]] -> x [S, n_txt+P-1, H] (bf16, or float32 when x_f32), key_mask [S, n_txt+P-1].
 * image_mask [S,P] or NULL. */
int opadpo_embed_splice(const int32_t* ids, const uint8_t* text_mask, const uint16_t* embed, const uint16_t* feats,
                        const int32_t* feat_row, const uint8_t* image_mask, void* x, int x_f32, uint8_t* key_mask,
                        int S, int n_txt, int P, int H, int image_token, void* stream);

/* ---- CLIP patch embedding (Conv2d k=s=patch as im2col + gemm_nt) ---------------------------------- */
int opadpo_im2col(const uint16_t* pixels, uint16_t* out, int B, int image_size, int patch, int kpad, void* stream);
int opadpo_vision_embed(const uint16_t* patches, const uint16_t* cls, const uint16_t* pos, uint16_t* x, int B, int P, int h, void* stream);
int opadpo_vision_embed_f32(const uint16_t* patches, const uint16_t* cls, const uint16_t* pos, float* x, int B, int P, int h, void* stream);   /* fp32 x */

/* ---- data movement helpers ---------------------------------------------------------------------- */
int opadpo_gather_rows(const uint16_t* src, int ld_src, const int32_t* rows_idx, uint16_t* dst, int n, int H, void* stream);
int opadpo_scatter_rows(const uint16_t* src, const int32_t* rows_idx, uint16_t* dst, int ld_dst, int n, int H, void* stream);
/* dst[rows_idx[r], :H] += src[r, :H] (fp32; duplicate indices accumulate) */
int opadpo_scatter_add_rows_f32(const float* src, const int32_t* rows_idx, float* dst, int ld_dst, int n, int H, void* stream);
int opadpo_transpose(const uint16_t* in, uint16_t* out, int R, int C, void* stream);
/* n_jobs transposes in one launch: jobs[j] = {src offset, dst offset, rows, cols} (elements, device memory, int64); max_tiles =
 * max over jobs of ceil(rows/64)*ceil(cols/64).  Used for the K-major copies of all LoRA blocks after an optimizer step. */
int opadpo_transpose_batched(const uint16_t* src, uint16_t* dst, const int64_t* jobs, int n_jobs, int max_tiles, void* stream);
int opadpo_f32_to_bf16(const float* in, uint16_t* out, size_t n, void* stream);
/* bf16 -> fp32 widening copy (exact); 16-byte aligned buffers.  Gradient slices received in bf16 from the ZeRO-1 reduce-scatter. */
int opadpo_bf16_to_f32(const uint16_t* in, float* out, size_t n, void* stream);
int opadpo_f32_to_bf16_strided(const float* in, uint16_t* out, size_t rows, int C, int ld, void* stream);

/* ---- head: compute_logprobs (utils/common_utils.py:112-118) + entropy (rl_models.py:128,132) -------
 * logits fp32 [rows,V] (ldl), labels int32 (0 = pad -> logp = -0.0, ent = 0), z = logits*inv_temp. */
int opadpo_head_fwd(const float* logits, int ldl, const int32_t* labels, float inv_temp, float* logp, float* ent,
                    float* lse, int rows, int V, void* stream);
/* dz = [dlogp * (onehot(label) - p) - dent * p * (log p + ent)] * inv_temp as bf16 [rows,V] (ldz), p = softmax(z).  ent (the
 * row entropies from head_fwd) and dent (their gradient) are nullable: only the OPA-SFT entropy regulariser
 * (opa_models/opa_trainer.py:64-90) differentiates the entropy; the DPO path passes NULL. */
int opadpo_head_bwd(const float* logits, int ldl, const int32_t* labels, const float* lse, const float* dlogp,
                    const float* ent, const float* dent, float inv_temp, uint16_t* dz, int ldz, int rows, int V, void* stream);

/* ---- clip_grad_norm_ + AdamW (rl_trainer.py:164-175; utils/trainer_utils.py:35) ------------------- */
int opadpo_sumsq(const float* g, size_t n, float* out, void* stream);  /* out[0] += sum g^2 */
/* p,m,v fp32 [n]; g fp32; p_bf16 (nullable) refreshed; step is 1-based; sumsq (nullable) device
 * scalar holding ||g||^2; effective gradient = g * grad_div * min(1, max_norm/(||g||*grad_div+1e-6)). */
int opadpo_adamw(float* p, const float* g, float* m, float* v, uint16_t* p_bf16, size_t n, double lr, double beta1,
                 double beta2, double eps, double weight_decay, int step, const float* sumsq, double max_norm,
                 double grad_div, void* stream);

/* ---- gradient exchange without torch.distributed (SURVEY.md section 8b "opadpo_allreduce_grads"; reference: accelerate / DDP behind
 * rl_trainer.py:155-175, which never syncs - Quirk Q1 - while north_star mandates the exchange) ------------------------------------------------
 * For a binder that owns its ncclComm_t (one process per GPU, ncclCommInitRank with the RCCL already loaded in the process; the library does
 * NOT link RCCL - it resolves the three collectives with dlsym at first use, librccl.so by name as the fall-back).  dtype 0 = fp32, 1 = bf16 (the
 * wire format of the Python host's ZeRO-1 path); SUM over the ranks, in place for the all-reduce; divide by the world size in opadpo_adamw's
 * grad_div.  ZeRO-1 = opadpo_reduce_scatter_grads (flat [world * shard_count] -> this rank's shard) -> opadpo_sumsq + scalar all-reduce through
 * opadpo_allreduce_grads(count = 1) -> opadpo_adamw on the shard -> opadpo_all_gather_params.  Asynchronous on `stream`; return code = the
 * RCCL result (0 = ncclSuccess), text through opadpo_last_error.  The Python host of this repository keeps using torch.distributed (same RCCL). */
int opadpo_allreduce_grads(void* nccl_comm, void* flat_grad, size_t count, int dtype, void* stream);
int opadpo_reduce_scatter_grads(void* nccl_comm, const void* flat_grad, void* shard, size_t shard_count, int dtype, void* stream);
int opadpo_all_gather_params(void* nccl_comm, const void* shard, void* flat, size_t shard_count, int dtype, void* stream);

/* ---- rollout (online_generator.py:292-323: policy.generate(do_sample=True, top_k, top_p, temperature)) ----
 * KV cache layout is head-major: k_cache / v_cache [B, nh, max_ctx, hd] (one (sequence, head) = one contiguous stream).
 * attn_decode: one query token per sequence, q row b at q + b*ldq ([nh*hd] used), o [B, nh*hd];
 * keys 0..ctx-1 valid where key_mask[b*max_ctx + j] != 0; ctx_ptr (device int32, nullable) overrides ctx with
 * ctx_ptr[0] + 1 (position of the newest key) for graph replay.  workspace (nullable): device scratch of at least
 * opadpo_attn_decode_workspace_bytes(B, nh, hd, max_ctx) bytes; with it the key range is split over several blocks
 * (+ one merge launch) where that fills the 256 CUs better: up to 256 (sequence, head) pairs as many ranges as fit ONE round of 16-wave
 * workgroups, two ranges of 4-wave workgroups for 257-767 pairs, and from 768 pairs two ranges only where they cut the rounds of the 1024
 * resident 4-wave workgroups by a fifth or more (max_ctx >= 512; the byte count returned is 0 when the geometry has one range).
 * Cache slots >= ctx are never read. */
int opadpo_attn_decode(const uint16_t* q, int ldq, const uint16_t* k_cache, const uint16_t* v_cache, uint16_t* o,
                       const uint8_t* key_mask, int B, int nh, int hd, int ctx, const int32_t* ctx_ptr, int max_ctx,
                       float scale, void* workspace, size_t workspace_bytes, void* stream);
size_t opadpo_attn_decode_workspace_bytes(int B, int nh, int hd, int max_ctx);
/* decode step: RoPE at position pos_ptr[0] (device int32) on the q and k thirds of qkv rows [q|k|v] (ld elements apart);
 * q is rotated in place, the rotated k and the v are appended to the caches at [b, h, pos, :]. */
int opadpo_rope_kv_append(uint16_t* qkv, int ld, const float* cos_tab, const float* sin_tab, uint16_t* k_cache, uint16_t* v_cache,
                          int B, int nh, int hd, const int32_t* pos_ptr, int max_ctx, void* stream);
/* rope_kv_append + attn_decode in ONE launch (decode step of the generator): qkv rows [q|k|v] of the new token as the
 * projection wrote them (not modified); q and k are rotated at position pos_ptr[0] inside the kernel, k and v appended to the
 * caches at [b, h, pos, :], attention over keys 0..pos (key_mask as above).  Same rounding points as the two calls. */
int opadpo_attn_decode_fused(const uint16_t* qkv, int ld, const float* cos_tab, const float* sin_tab, uint16_t* k_cache, uint16_t* v_cache,
                             uint16_t* o, const uint8_t* key_mask, int B, int nh, int hd, const int32_t* pos_ptr, int max_ctx, float scale,
                             void* workspace, size_t workspace_bytes, void* stream);
/* opadpo_attn_decode_fused with a position PER ROW (continuous rollout: the rows of a launch sit at different context lengths): pos_rows [B]
 * device int32, row b is rotated at pos_rows[b], appends its k / v at [b, h, pos_rows[b], :] and attends keys 0..pos_rows[b].  The key-range
 * split (a function of B, nh and max_ctx alone), the workgroup shape and the range that appends are those of opadpo_attn_decode_fused, so row
 * b's output and the k / v it appends are bit-identical to row b of opadpo_attn_decode_fused run with every row at pos_rows[b] on the same
 * caches, B and max_ctx.  A position outside [0, max_ctx - 1] is clamped into it: no row reads or writes outside its own cache rows, key-mask
 * row or the first max_ctx rows of the RoPE tables.  Cache slots behind a row's position are never read.  Refused with text, nothing launched:
 * a null operand (key_mask and workspace are nullable as above), head_dim other than 64 / 128, a misaligned leading dimension. */
int opadpo_attn_decode_fused_rows(const uint16_t* qkv, int ld, const float* cos_tab, const float* sin_tab, uint16_t* k_cache, uint16_t* v_cache,
                                  uint16_t* o, const uint8_t* key_mask, int B, int nh, int hd, const int32_t* pos_rows, int max_ctx, float scale,
                                  void* workspace, size_t workspace_bytes, void* stream);
/* temperature -> top-k -> top-p -> multinomial (HF logits processors order); one draw per row from
 * a counter-based generator keyed on (seed, step, row).  finished rows emit pad_id; a row that draws eos_id (>= 0) is
 * marked finished.  step_ptr (device int32, nullable) overrides `step`; history (nullable) [steps, rows] receives the
 * token at row step. */
int opadpo_sample(const float* logits, int ldl, int rows, int V, float temperature, int top_k, float top_p,
                  uint64_t seed, uint64_t step, const int32_t* step_ptr, uint8_t* finished, int pad_id, int eos_id,
                  int32_t* out, int32_t* history, void* stream);
/* opadpo_sample with a seed, a step and a cap PER ROW (continuous rollout; device arrays [rows]: seed_rows uint64, step_rows / cap_rows int32).
 * Row b draws the token opadpo_sample draws for it with scalar (seed_rows[b], step_rows[b]) on the same logits - the draw stays
 * f(seed, step, row) - writes it to out[b] and to history[b, step_rows[b]] (history [rows, max_steps] int32, ROW-major: a row's tokens are
 * contiguous; nullable), and then advances step_rows[b] by one.  The row is marked finished when it drew eos_id (>= 0) or when the token was its
 * cap_rows[b]-th (its step reached cap_rows[b]).  A finished row - and a row whose step is outside [0, min(cap_rows[b], max_steps)) - writes
 * pad_id to out[b] and nothing else: its step does not advance and no history slot is touched, however many launches it sits through.
 * `finished` is required.  Both sampler kernels (the row in LDS for V % 4 == 0 and V <= 32768, the generic one otherwise) have this form. */
int opadpo_sample_rows(const float* logits, int ldl, int rows, int V, float temperature, int top_k, float top_p, const uint64_t* seed_rows,
                       int32_t* step_rows, const int32_t* cap_rows, int max_steps, uint8_t* finished, int pad_id, int eos_id, int32_t* out,
                       int32_t* history, void* stream);
/* Logits processors of the yes/no evaluation generator (eval_llava_rlhf_coco/model_vqa_logit.py), for rows <= 64 and at most
 * OPADPO_MAX_LOGIT_IDS table entries.  ids (int32) / bias (fp32) are DEVICE arrays; ids_host is the host copy of ids, checked before anything is
 * launched: every id in [0, V), and no id twice in a bias table.
 * opadpo_logit_bias_add: logits[row, ids[e]] += bias[e] for every row - HF's sequence_bias with one-token sequences; call it before
 * opadpo_sample (logits processors run before temperature / top-k / top-p).  n = 0 launches nothing.
 * opadpo_gather_scores: scores [rows, m] fp32 = the processed scores HF's generate(output_scores=True) records for a sampled step:
 * logit / temperature, then the top-k and top-p cuts of opadpo_sample's order; a token that is cut reads -inf.  temperature = 0 (greedy
 * decoding in this library): the logit itself, nothing cut.  ids may repeat.  m = 0 launches nothing. */
#define OPADPO_MAX_LOGIT_IDS 64
int opadpo_logit_bias_add(float* logits, int ldl, int rows, int V, const int32_t* ids, const float* bias, const int32_t* ids_host, int n,
                          void* stream);
int opadpo_gather_scores(const float* logits, int ldl, int rows, int V, const int32_t* ids, const int32_t* ids_host, int m, float temperature,
                         int top_k, float top_p, float* scores, void* stream);
/* Per-token log-prob and entropy of sampled tokens, read from the fp32 logits row the sampler read (any bias added, a suppressed EOS column
 * -inf).  z = fp32(logits * inv_T), one multiply as in opadpo_head_fwd, inv_T = 1 / temperature; temperature 0 is greedy decoding and reads with
 * inv_T = 1.  For row b with token tokens[b] (device int32 [rows]):
 *   logp[b] = z[tok] - logsumexp(z)          ent[b] = logsumexp(z) - sum softmax(z) * z
 * A column with z = -inf adds 0 to both sums (no NaN).  tokens[b] == pad_id: logp = -0.0, ent = 0 (opadpo_head_fwd's pad rule, by value).
 * This is the policy's distribution BEFORE the top-k / top-p cuts - what opadpo_seq_logprobs_fwd returns for the same tokens at the same
 * temperature; with top_k = 0, top_p = 1 it is also the distribution the token was drawn from.  The log-prob under the cut and renormalised
 * distribution is not computed.  One workgroup per row, the row read once with 16-byte loads.  Any rows >= 1; V % 4 == 0, ldl % 4 == 0, ldl >= V
 * and a 16-byte aligned logits base, temperature >= 0: refused with text otherwise, nothing launched.  ent is nullable. */
int opadpo_token_logprobs(const float* logits, int ldl, int rows, int V, const int32_t* tokens, float temperature, int pad_id, float* logp,
                          float* ent, void* stream);

/* Beam search (HF GenerationMixin._beam_search with do_sample=False, num_return_sequences=1, length_penalty=1.0, early_stopping=False).
 * B items of k beams each; rows = B*k <= 64, 1 <= k <= OPADPO_MAX_BEAMS.  Row i is beam i % k of item i / k.
 * Decode attention of the beam rows: the items' prefix caches [B, nh, Lp, hd] (prefix_mask [B, Lp], nullable) are shared by their beams;
 * suffix caches [B*k, nh, max_new, hd]: the key at position j >= Lp of row i lives in physical row table[i][j - Lp] ([B*k, max_new] int32).
 * The new token (position pos_ptr[0] >= Lp) is rotated and appended at (i, pos - Lp).  Bit-identical to opadpo_attn_decode_fused on the
 * materialised per-row cache (workspace: opadpo_attn_decode_workspace_bytes(B*k, nh, hd, Lp + max_new)). */
#define OPADPO_MAX_BEAMS 16
int opadpo_attn_decode_beam(const uint16_t* qkv, int ld, const float* cos_tab, const float* sin_tab, const uint16_t* k_prefix,
                            const uint16_t* v_prefix, uint16_t* k_suffix, uint16_t* v_suffix, uint16_t* o, const uint8_t* prefix_mask, int B, int k,
                            int nh, int hd, const int32_t* pos_ptr, int Lp, int max_new, const int32_t* table, float scale, void* workspace,
                            size_t workspace_bytes, void* stream);
/* n sampled responses per prompt (HF generate(do_sample=True, num_return_sequences=n)): inputs expand as repeat_interleave(n), row b is sample
 * b % n of item b / n; 1 <= n <= OPADPO_MAX_RETURN_SEQUENCES.  Decode attention of such rows: the items' prefix caches [items, nh, Lp, hd]
 * (prefix_mask [items, Lp], nullable) are stored once and shared by the item's n rows; suffix caches [items*n, nh, max_new, hd] per row.  Each call
 * rotates q and the new k at pos_ptr[0] (>= Lp), appends k and v at suffix slot pos - Lp of row b, and attends the item's unmasked prefix keys plus
 * suffix slots 0 .. pos - Lp of its own row.  form: 1 = per-row (the beam kernel with the identity slot table: output and appended K/V bit-identical
 * to opadpo_attn_decode_fused on the materialised per-row cache), 2 = grouped (head_dim 128 only, refused otherwise: one workgroup per (item, head,
 * prefix key range) reads every K/V tile once for the item's n rows on v_mfma_f32_16x16x32_bf16; the softmax weights are rounded to bf16 for the
 * P.V product - the one rounding point it adds; the suffix keys go through the per-row kernel and a merge launch combines the partials; appended
 * K/V bit-identical to form 1), 0 = the library's choice (grouped for n >= 2 at head_dim 128).  Prefix key ranges of the grouped form:
 * R = min(max(1, 256 / (items*nh)), max(1, Lp / 64)), range stride per = ceil(ceil(Lp / R) / 64) * 64 keys, ranges = ceil(Lp / per), the last one
 * holding the remainder.
 * workspace: at least opadpo_attn_decode_shared_workspace_bytes(...) bytes (enough for either form), refused below that. */
#define OPADPO_MAX_RETURN_SEQUENCES 16
size_t opadpo_attn_decode_shared_workspace_bytes(int items, int n, int nh, int hd, int Lp, int max_new);
int opadpo_attn_decode_shared(const uint16_t* qkv, int ld, const float* cos_tab, const float* sin_tab, const uint16_t* k_prefix,
                              const uint16_t* v_prefix, uint16_t* k_suffix, uint16_t* v_suffix, uint16_t* o, const uint8_t* prefix_mask, int items,
                              int n, int nh, int hd, const int32_t* pos_ptr, int Lp, int max_new, float scale, void* workspace,
                              size_t workspace_bytes, int form, void* stream);
/* One beam-search step at step index `step` (0 = the first generated token: only beam 0 of an item is live) on fp32 logits [B*k, V] (ldl
 * apart).  Candidates are ranked by log_softmax + beam score, ties to the lower flat index beam*V + token.  Caller-owned device state, all
 * zero-initialised before step 0 except as noted:
 *   run_score [B*k] f32 running beam scores;  cand_val [B*k*2k] f32, cand_tok [B*k*2k] int32 scratch;
 *   fin_score [B*k] f32, fin_info [3][B*k] int32 (step, parent row, token), fin_n [B] int32: per item the best k finished hypotheses,
 *     sorted, score = sum logprob / generated length (EOS included);  done [B] uint8 (early stop or last step);
 *   cur_tok [B*k] int32 the running beams' newest tokens;  bp [2][max_new][B*k] int32 backpointers (parent row | token) per step;
 *   table [2][B*k][max_new] int32 slot tables by step parity: step t reads buffer t & 1 and writes buffer (t + 1) & 1.
 * A candidate is finished if its token is eos_id (>= 0) or step == max_new - 1. */
int opadpo_beam_step(const float* logits, int ldl, int B, int k, int V, int step, int max_new, int eos_id, int pad_id, float* run_score,
                     float* cand_val, int32_t* cand_tok, float* fin_score, int32_t* fin_info, int32_t* fin_n, uint8_t* done, int32_t* cur_tok,
                     int32_t* bp, int32_t* table, void* stream);

/* =====================================================================================================================
 * Context API: the SEQUENCE-LEVEL entry points.
 *
 * The reference's seam is one Python call per pass - `self.base_model(**inputs)` (opadpo/dpo_models/rl_models.py:114-120), its
 * backward `accelerator.backward(loss)` (rl_trainer.py:162) and `policy.generate(...)` (rl_models.py:166-183,
 * opadpo/generator_models/online_generator.py:292-309).  An `opadpo_ctx` puts the whole schedule of such a pass below the C ABI:
 *   - one context per process / GPU (one process per GPU, run/train_opa_dpo.sh:96-99); not re-entrant per context;
 *   - weights, adapters, token ids, masks and outputs are BORROWED raw device pointers (the caller keeps them alive);
 *   - the workspace, the saved activations of a training forward and the KV cache of a rollout are OWNED by the context
 *     (hipMalloc by default, or the caller's stream-ordered allocator - opadpo_ctx_set_allocator - so that a torch host keeps ONE
 *     memory pool); opadpo_ctx_destroy frees everything;
 *   - every call takes the caller's hipStream_t and is asynchronous on it (opadpo_decode_begin synchronises twice for two tiny
 *     host->device counters); int return code, 0 = ok, text through opadpo_ctx_last_error(ctx); never aborts, never a CPU path;
 *   - kernel-variant switches are per context (opadpo_ctx_set_flags), not process-global.
 * ===================================================================================================================== */
#define OPADPO_MAX_ADAPTERS 8
#define OPADPO_IMAGE_TOKEN (-200) /* utils/constants.py:28 IMAGE_TOKEN_INDEX */

typedef struct opadpo_ctx opadpo_ctx;
typedef struct opadpo_saved opadpo_saved; /* activations of one training forward, owned by the context */

typedef struct opadpo_dims {
  int hidden, n_layers, n_heads, head_dim, ffn, vocab; /* Llama-2 decoder (7B: 4096, 32, 32, 128, 11008, 32000) */
  float rms_eps, rope_theta;
  int v_hidden, v_used_layers, v_heads, v_ffn, image_size, patch; /* CLIP-ViT-L/14-336: 1024, 23 (hidden_states[-2]), 16, 4096, 336, 14 */
  float v_eps;
  int lora_r; /* 256 in the OPA-DPO recipe */
  float lora_alpha;
} opadpo_dims;

/* One decoder layer, bf16, row-major [out, in]: q|k|v and gate|up fused along the output dimension.  *_t = K-major transposed
 * copies ([in, out]) used by the dgrad GEMMs (NULL for inference-only contexts). */
typedef struct opadpo_layer_weights {
  const uint16_t *wqkv, *wo, *wgu, *wd, *ln1, *ln2;
  const uint16_t *wqkv_t, *wo_t, *wgu_t, *wd_t;
} opadpo_layer_weights;

typedef struct opadpo_vision_layer_weights {
  const uint16_t *ln1_w, *ln1_b, *ln2_w, *ln2_b, *wqkv, *bqkv, *wo, *bo, *fc1, *b1, *fc2, *b2;
} opadpo_vision_layer_weights;

typedef struct opadpo_vision_weights {
  const uint16_t *patch_w;              /* [v_hidden, ceil64(3*patch*patch)] zero-padded conv weight */
  const uint16_t *cls, *pos, *pre_ln_w, *pre_ln_b;
  const uint16_t *proj0, *proj0_b, *proj2, *proj2_b; /* mm_projector mlp2x_gelu */
} opadpo_vision_weights;

/* stream-ordered allocator hooks: alloc(bytes, stream, user) -> device pointer (NULL on failure); free(ptr, user) */
typedef void* (*opadpo_alloc_fn)(size_t bytes, void* stream, void* user);
typedef void (*opadpo_free_fn)(void* ptr, void* user);

int opadpo_ctx_create(const opadpo_dims* dims, int device, opadpo_ctx** out);
void opadpo_ctx_destroy(opadpo_ctx* ctx);
const char* opadpo_ctx_last_error(const opadpo_ctx* ctx);
int opadpo_ctx_set_allocator(opadpo_ctx* ctx, opadpo_alloc_fn alloc, opadpo_free_fn free_fn, void* user);
/* gemm_variant as in opadpo_set_flags, for this context only; -1 = process default.  use_tr is a SEPARATE bit space from the process flags.
 * use_tr = -1: the context's attention and gemm_tn kernels follow the process flags (later opadpo_set_flags calls included).  use_tr >= 0: its
 * bit 0 (transposed LDS reads) and bit 3 (128x128 gemm_tn) replace process bits 0 and 3 for this context; bits 1, 2 and 4 are NOT read (the
 * attention DMA forward and the skinny8 choice stay with the process flags, as do process bits 5-12); bits 5-14 are the context switches listed here.
 * Context bits: use_tr bit 5 = keep the
 * 16/32-row streaming GEMMs for rollouts of 33..64 sequences (default there: the LDS-ring decode GEMM, opadpo_gemm_nt_decode);
 * bit 6 = SwiGLU backward in the LDS-STAGED epilogue of the down projection's dgrad (the form of rounds 3-4, which measured 0.35 % slower per step
 * than its own launch; the default since round 5 is the direct-epilogue form, see bit 14); bit 7 = top decoder layer on every row (default on ragged rows: its o-projection and MLP run only
 * on the rows the head reads - the last prefix row and the response rows -, forward and backward; exact, nothing else reads the rest);
 * bit 8 = the 16-rows-per-wave attention forward and dQ kernels (default at head_dim 128: 32 rows per wave on v_mfma_f32_32x32x16_bf16);
 * bit 9 / bit 10 = force / forbid the CHUNKED head (lm_head + online log-sum-exp + label gather + entropy over 4096 vocabulary columns at
 * a time, logits recomputed per chunk in the backward: no [rows, vocab] buffer; default: chunked when the fp32 logits of the batch shape S*K*T reach 4 GiB);
 * bit 11 = rotary embedding as its own in-place kernel (default on ragged rows: inside the q|k|v projection's epilogue, opadpo_gemm_nt_rope_pos);
 * bit 12 = LoRA wgrads flushed with fp32 atomics (default: partial tiles to a workspace + ordered reduce, bit-reproducible gradients).
 *   PRECONDITION of the default: every wgrad of a layer runs on the 256x256 kernel, i.e. lora_r % 256 == 0 (the shipped DPO recipe: r = 256).
 *   With r = 64 / 128 (the reference's online_generation / opa_train defaults) the wgrads run on the 128x128 kernel and flush with fp32
 *   atomics whatever this bit says: results correct to fp32 summation order, not bit-reproducible - opadpo_ctx_wgrad_deterministic tells.
 * bit 13 = residual adds of the full-sequence passes deferred to the RMSNorm that follows (rmsnorm_sum_fwd: x = res + y, 14 B per element; the form of
 *   rounds 2-4).  Default since round 5: the o / down projections add their fp32 residual rows in the 256x256 kernels' DIRECT epilogue (rows requested
 *   one row block ahead of the accumulator read-out) and the norm pass reads 6 B per element - the same fp32 addition of the same operands, so h / x
 *   keep their bits; -1.0 % per step.
 * bit 14 = SwiGLU backward as its own kernel (silu_mul_bwd; rounds 1-4).  Default since round 5: inside the direct epilogue of the down projection's
 *   dgrad (OPADPO_ACT_SWIGLU_BWD, gate / up operands requested one row block ahead; bit-identical to the two-kernel form, d_act never reaches HBM;
 *   -0.8 % per step); bit 6 selects the LDS-staged form of that epilogue (rounds 3-4; cross-check).
 * bit 15 = the shared-prefix decode attention of opadpo_decode_begin_n stays per-row (opadpo_attn_decode_shared form 1: the tokens of the
 *   repeated-prompt rollout; cross-check).  Default: the library's choice (grouped for n >= 2 at head_dim 128). */
int opadpo_ctx_set_flags(opadpo_ctx* ctx, int gemm_variant, int use_tr);
/* how the LAST opadpo_seq_logprobs_bwd of this context flushed its LoRA wgrads: 1 = ordered reduce (bit-reproducible), 0 = fp32 atomics
 * (bit 12 set, or lora_r % 256 != 0), -1 = no backward yet */
int opadpo_ctx_wgrad_deterministic(const opadpo_ctx* ctx);
/* return cached arenas and the workspace to the allocator, and forget the largest-arena-so-far hints (the next pass sizes its arena for its own batch) */
int opadpo_ctx_trim(opadpo_ctx* ctx);
size_t opadpo_ctx_bytes_peak(const opadpo_ctx* ctx);
/* live measurement of the dominant kernel: while enabled every gemm_nt launch of the context is bracketed by HIP events on the launch
 * stream; _read waits for them and returns (and clears) the sum of algorithmic FLOPs 2*M*N*(K1+K2), the sum of launch durations in ms
 * and the launch count */
int opadpo_ctx_profile(opadpo_ctx* ctx, int enable);
int opadpo_ctx_profile_read(opadpo_ctx* ctx, double* flops, double* ms, int64_t* launches);

/* make_models (dpo_trainer.py:958-1038): ONE frozen base shared by every adapter */
int opadpo_ctx_set_llm_weights(opadpo_ctx* ctx, const uint16_t* embed, const uint16_t* final_norm, const uint16_t* lm_head,
                               const uint16_t* lm_head_t, const opadpo_layer_weights* layers, int n_layers);
int opadpo_ctx_set_vision_weights(opadpo_ctx* ctx, const opadpo_vision_weights* w, const opadpo_vision_layer_weights* layers, int n_layers);
/* optional: rotary tables [n_pos][head_dim/2] fp32 from the host (default: the context computes HF Llama's own) */
int opadpo_ctx_set_rope_tables(opadpo_ctx* ctx, const float* cos_tab, const float* sin_tab, int n_pos);
/* set_adapter (rl_models.py:84-85): adapter `id` = flat bf16 LoRA buffer (layer-major; per layer a_qkv [3r,H] | b_qkv [3H,r] | a_o |
 * b_o | a_gu [2r,H] | b_gu [2F,r] | a_d [r,F] | b_d [H,r]); work_t = its K-major copy, grad = flat fp32 gradient (both NULL for a
 * frozen adapter); work = NULL selects the bare base model */
int opadpo_ctx_set_adapter(opadpo_ctx* ctx, int id, const uint16_t* work, const uint16_t* work_t, float* grad);
/* a FROZEN adapter folded into its own copy of the projections (PEFT merge); swiglu_pair: wgu rows per 128 = [64 gate | 64 up] */
int opadpo_ctx_set_merged_adapter(opadpo_ctx* ctx, int id, const opadpo_layer_weights* merged, int n_layers, int swiglu_pair);

/* get_vision_tower() + mm_projector: pixels [B,3,S,S] bf16 -> feats [B, 576, hidden] bf16 */
int opadpo_vision_encode(opadpo_ctx* ctx, const uint16_t* pixels, int B, uint16_t* feats, void* stream);

/* base_model(**inputs) + logits[:, -T-1:-1] / temperature + compute_logprobs + entropy (rl_models.py:114-132), for S rows
 * [query | response_0 | .. | response_{K-1}] of n_txt ids each (one OPADPO_IMAGE_TOKEN per row; K > 1: the responses share one pass
 * over the image + query prefix).  feat_row[s] = which image's features row s uses; image_mask [S,576] (nullable) = CoPO
 * 'attention' key mask.  logp / ent: [K*S*T] fp32 in the reference's stacking order [k][s][t].  train = 1 keeps the activations
 * (handle in *saved); train = 0 releases them (*saved = NULL).
 * row_plan (HOST memory, nullable): int32 [S][K+1] = per row the number of LEADING masked query positions to drop and the valid
 * length of every response (positions behind it are padding).  When given, the pass runs on RAGGED rows: padding positions are not
 * rows of any GEMM / norm / SwiGLU / RoPE / attention tile (the reference computes them and throws the result away: 24 % of the rows
 * of a synthetic seq512 pair), outputs on valid tokens are unchanged, pad cells still read -0.0 / 0.  NULL = the padded layout.  Any S
 * and K (the per-sequence geometry travels to the device in as many 960-int kernel-argument blocks as it needs). */
int opadpo_seq_logprobs_fwd(opadpo_ctx* ctx, int adapter_id, const int32_t* ids, const uint8_t* text_mask, const int32_t* feat_row,
                            const uint8_t* image_mask, const uint16_t* feats, int S, int n_txt, int T, int K, float temperature, int train,
                            float* logp, float* ent, opadpo_saved** saved, const int32_t* row_plan, void* stream);
/* accelerator.backward(loss): accumulates d loss / d LoRA into the adapter's flat fp32 grad buffer for decoder layers
 * layer_hi .. layer_lo (top-down).  The first call of a backward starts at n_layers - 1 (it runs the head backward from dlogp
 * [K*S*T] and the optional entropy gradient dent); later calls continue below - a data-parallel host launches the exchange of a
 * finished bucket of layers between two calls.  d_feats (nullable, fp32 [n_images,576,hidden], accumulated): gradient w.r.t.
 * the image features (OPA LoRA-SFT stage), written when layer_lo == 0. */
int opadpo_seq_logprobs_bwd(opadpo_ctx* ctx, opadpo_saved* saved, const float* dlogp, const float* dent, float* d_feats, int layer_hi,
                            int layer_lo, void* stream);
/* LoRA dropout of the NEXT training forward (opadpo_seq_logprobs_fwd with train = 1) of this context: rate p in [0, 1), seed < 2^32 and the host's
 * per-training-forward counter `call` (different for every micro-batch and rank).  The forward consumes the setting (the one after it runs without dropout
 * unless this is called again) and records it in the saved handle: opadpo_seq_logprobs_bwd regenerates the same masks.  One mask per adapted Linear (7 per
 * decoder layer), hashed with the pass's own row numbers; no-grad passes (train = 0), merged adapters, prefill and decode never apply dropout.  p = 0 is
 * the pass without this call: the same launches, buffers and bits. */
int opadpo_ctx_set_lora_dropout(opadpo_ctx* ctx, double p, uint64_t seed, uint64_t call);
/* Gradient checkpointing (HF gradient_checkpointing_enable(): recompute every decoder layer in the backward) of the TRAINING forwards of this context,
 * on != 0 until switched off again; default off.  A checkpointed forward keeps the fp32 residual stream x_0 .. x_{n_layers}, the key mask, the row
 * geometry, the head buffers and the dropout descriptor, and ONE layer's activation slot instead of n_layers of them (what a no-grad pass holds);
 * the handle remembers the mode.  opadpo_seq_logprobs_bwd re-runs layer i's forward from x_i into that slot - without the down projection's base
 * product, whose result nothing reads - right before layer i's backward, ranged calls included.  Every kernel of the forward is deterministic, so
 * log-probs, entropies and LoRA gradients carry the bits of the resident pass.  No-grad passes (train = 0) are unaffected. */
int opadpo_ctx_set_grad_checkpoint(opadpo_ctx* ctx, int on);
int opadpo_saved_release(opadpo_ctx* ctx, opadpo_saved* saved);
/* diagnostics (parity tests: the per-layer drift curve of the residual stream): copies the fp32 residual stream ENTERING decoder
 * layer `layer` of a training forward, [rows, hidden], into dst (device memory, rows*hidden floats) and returns the row count in
 * *rows (ragged passes: the compact valid rows, sequence by sequence; padded: S * L).  dst = NULL only queries *rows. */
int opadpo_saved_residual(opadpo_ctx* ctx, const opadpo_saved* saved, int layer, float* dst, int* rows, void* stream);

/* policy.generate(do_sample=True, ...) (online_generator.py:292-309): prefill of B left-padded queries [B,Q] + token 0; the KV
 * cache ([n_layers, B, heads, Q+575+max_new_tokens, head_dim] x2) lives in the context.  history [max_new_tokens, B] int32
 * (caller-owned) receives the tokens; finished rows emit pad_id.  suppress_eos: benchmarks (never sample EOS).
 * 1 <= B <= 256 (above: refused with text).  Without LoRA tails (adapter-free or merged adapter) 9..64 rows decode on opadpo_gemm_nt_decode's kernel and
 * 65..256 rows on opadpo_gemm_nt_decode_wide's, same layer shape.  An UNMERGED adapter with B > 64 is accepted and correct but unoptimised: its
 * projections with their LoRA tails run on the tiled gemm_nt kernels (no weight-streaming kernel takes more than 64 rows with a tail) - merge the
 * adapter (opadpo_ctx_set_merged_adapter) for a rollout of that size.  The prefill of B > 64 queries runs in groups of 64 queries (same results, bounded
 * scratch).  Logit processors (opadpo_ctx_set_logit_processors) keep their 64-row cap: an armed context with B > 64 is refused, and the refusal disarms. */
int opadpo_decode_begin(opadpo_ctx* ctx, int adapter_id, const int32_t* ids, const uint8_t* text_mask, const uint16_t* feats, int B, int Q,
                        int max_new_tokens, float temperature, int top_k, float top_p, uint64_t seed, int eos_id, int pad_id, int suppress_eos,
                        int32_t* history, void* stream);
/* policy.generate(do_sample=True, num_return_sequences=n, ...) (rl_models.py respond): opadpo_decode_begin's arguments plus n.  ONE prefill of the B
 * prompts (passes of at most 64); their KV caches [n_layers, B, heads, Q+575, head_dim] are the shared prefixes of the prompts' n rows, whose
 * generated keys live in per-row suffix caches [n_layers, B*n, heads, max_new_tokens, head_dim].  Row b = i*n + j is sample j of prompt i and draws
 * with (seed, step, b), exactly as row b of a rollout over the prompts repeated n times each; history is [max_new_tokens, B*n].  Token 0 comes from
 * the prompts' last hidden rows expanded to B*n rows: step 0 has the launches and the bits of the repeated-prompt run.  The decode steps use
 * opadpo_attn_decode_shared (form 0; context flag bit 15: form 1, whose tokens are those of the repeated-prompt rollout).
 * opadpo_decode_run / _step / _all_finished / _end work per row as after opadpo_decode_begin.  1 <= n <= OPADPO_MAX_RETURN_SEQUENCES and B*n <= 256,
 * refused with text otherwise; n = 1 IS opadpo_decode_begin (same launches, arena and bits).  Armed logit processors keep their 64-row cap, which
 * counts B*n rows. */
int opadpo_decode_begin_n(opadpo_ctx* ctx, int adapter_id, const int32_t* ids, const uint8_t* text_mask, const uint16_t* feats, int B, int Q, int n,
                          int max_new_tokens, float temperature, int top_k, float top_p, uint64_t seed, int eos_id, int pad_id, int suppress_eos,
                          int32_t* history, void* stream);
/* Logit bias and first-token scores of the NEXT opadpo_decode_begin of this context (model_vqa_logit.py: sequence_bias / output_scores).
 * bias_ids / bias [n] and score_ids [m] are HOST arrays (copied; n, m <= OPADPO_MAX_LOGIT_IDS, ids in [0, vocab), bias ids distinct).
 * n > 0: every step of that generation - the prefill head that produces token 0 included - adds bias[e] to the logit of bias_ids[e] in every
 * row before temperature / top-k / top-p (one more launch per step, part of the captured step under use_graph).  m > 0: after token 0 the
 * processed step-0 scores of score_ids go to scores [B, m] fp32 (caller-owned device memory, like history) as opadpo_gather_scores defines them
 * with the generation's temperature / top_k / top_p; scores_raw != 0: the biased logits themselves (greedy decoding, which the host asks for
 * as top_k = 1).  opadpo_decode_begin reads the setting and opadpo_decode_end clears it: the generation after that runs without either unless
 * this is called again.  n = m = 0 clears it; a generation without it issues exactly the launches it issued before this entry point existed.
 * opadpo_decode_beam_begin refuses an armed context, and so does opadpo_decode_begin with B > 64 (opadpo_logit_bias_add / opadpo_gather_scores take at most
 * 64 rows); either refusal clears the setting. */
int opadpo_ctx_set_logit_processors(opadpo_ctx* ctx, const int32_t* bias_ids, const float* bias, int n, const int32_t* score_ids, int m,
                                    float* scores, int scores_raw);
/* Per-token log-probs and entropies of the sampled tokens of the NEXT opadpo_decode_begin / opadpo_decode_begin_n of this context.  logp / ent:
 * caller-owned device fp32 [max_new_tokens, rows], laid out like history (rows = B, or B*n); ent is nullable.  That generation fills both with
 * the pad values (-0.0 / 0) and then, at every step - the prefill head that yields token 0, every plain step, the captured step under use_graph -
 * launches opadpo_token_logprobs' kernel right after the sampler on the row it read, with the generation's temperature (a greedy generation,
 * which the host asks for as temperature 1 / top_k = 1, reads with inv_T = 1) and the device step counter the sampler used.  So slot [t, b] holds
 * the log-prob of history[t, b] under the policy's distribution before the top-k / top-p cuts (the cut, renormalised distribution is not
 * computed); a pad token - a finished row, a step never run, a sampled id equal to pad_id - reads -0.0 / 0, and the step on which a row draws EOS
 * carries EOS's own values.  Any row count the rollout takes (1..256); independent of opadpo_ctx_set_logit_processors (both may be armed; those keep
 * their 64-row cap).  logp = ent = NULL clears the setting; logp = NULL with ent != NULL is refused.  opadpo_decode_begin reads the setting and
 * opadpo_decode_end clears it; a generation without it carves the same arena and issues exactly the launches it issued before this entry point
 * existed.  opadpo_decode_beam_begin refuses an armed context (beam search keeps returning its sequence score), and the refusal clears the setting. */
int opadpo_ctx_set_output_logprobs(opadpo_ctx* ctx, float* logp, float* ent);
/* one more token for every row: all launches of a step, asynchronous */
int opadpo_decode_step(opadpo_ctx* ctx, void* stream);
/* n_steps more tokens.  use_graph = 0: the launches of every step are issued from the library's own loop (no host work between
 * them; measured faster than graph replay on MI355X: 3.45 vs 3.72 ms per step at 7B / 4 sequences); use_graph = 1: one step is
 * captured into a hipGraph once and replayed per token (same tokens, bit for bit) */
int opadpo_decode_run(opadpo_ctx* ctx, int n_steps, int use_graph, void* stream);
/* synchronous: *all_finished = every row has emitted EOS (beam decode: every item is done) */
int opadpo_decode_all_finished(opadpo_ctx* ctx, int* all_finished, void* stream);
int opadpo_decode_end(opadpo_ctx* ctx);
/* Continuous batching for the sampling rollout: a session of `slots` decode rows that are REFILLED as they finish, instead of a batch that runs
 * until its longest row is done.  Every slot has its own position, step, cap (the most tokens its prompt may generate, <= max_new_tokens), seed
 * and KV cache [Q+575+max_new_tokens]; the step's kernels read them per row (opadpo_attn_decode_fused_rows, opadpo_sample_rows, the per-row form
 * of opadpo_token_logprobs' kernel), everything else of a step is opadpo_decode_begin's step on `slots` rows - the same GEMM paths by row count and
 * adapter kind.  A slot finishes when it draws EOS or has written its cap-th token; a finished or never used slot sits through further steps
 * without moving: it emits pad, its position and step stay, and it touches no memory outside its own cache, key-mask, history and log-prob rows.
 * The prompt in slot s draws with (its seed, its own step, s): its tokens are those of row s of an opadpo_decode_begin batch of `slots` rows with
 * that prompt at row s, that seed and the same max_new_tokens, up to its cap.
 *   opadpo_decode_cont_begin   carves the arena of `slots` rows; every slot starts idle (finished).  1 <= slots <= 256.
 *   opadpo_decode_cont_admit   n prompts into n finished slots: slot_ids / seeds / caps are HOST arrays [n], ids [n, Q] / text_mask [n, Q] /
 *                              feats [n, 576, hidden] device arrays in the order of slot_ids.  Prompts whose slots are consecutive share a prefill
 *                              pass (at most 64 per pass); K / V land in the slots' caches, the slots' key-mask rows are rewritten, position Lp-1,
 *                              step 0, cap and seed are set, the history / log-prob rows become pad / -0.0 / 0, and token 0 is sampled for the
 *                              admitted slots only.  The prefill scratch is allocated and released inside the call; synchronises once.
 *   opadpo_decode_run / _step  step every slot (a step captured under use_graph = 1 stays valid across admissions: its pointers are the arena's).
 *   opadpo_decode_cont_poll    synchronous: finished_host [slots] (host) = the slots' finished flags; the session remembers them.
 *   opadpo_decode_cont_retire  asynchronous device copies of a finished slot's history row into tokens [max_new_tokens] int32 and, when the
 *                              session was armed, of its log-prob / entropy rows into logp / ent [max_new_tokens] fp32 (both nullable).
 *   opadpo_decode_end          ends the session.
 * opadpo_ctx_set_output_logprobs arms a session as it arms a generation; its buffers are then [slots, max_new_tokens], slot-major like the
 * session's history.  Refused with text before anything is launched (the begin's refusals disarm, as opadpo_decode_begin's do): slots outside
 * 1..256; armed logit processors (they keep the static rollout); a cap outside 1..max_new_tokens; a slot id outside 0..slots-1 or repeated in one
 * call; admission into, or retirement of, a slot that was not finished at the last poll (a slot is finished from begin until it is admitted). */
int opadpo_decode_cont_begin(opadpo_ctx* ctx, int adapter_id, int slots, int Q, int max_new_tokens, float temperature, int top_k, float top_p,
                             int eos_id, int pad_id, int suppress_eos, void* stream);
int opadpo_decode_cont_admit(opadpo_ctx* ctx, int n, const int32_t* slot_ids, const int32_t* ids, const uint8_t* text_mask, const uint16_t* feats,
                             const uint64_t* seeds, const int32_t* caps, void* stream);
int opadpo_decode_cont_poll(opadpo_ctx* ctx, uint8_t* finished_host, void* stream);
int opadpo_decode_cont_retire(opadpo_ctx* ctx, int slot, int32_t* tokens, float* logp, float* ent, void* stream);
/* model.generate(num_beams=k, do_sample=False) (eval_llava_rlhf_coco/model_vqa.py): ONE prefill of the B questions (its KV cache is the
 * items' shared prefix), the k beams' generated keys in per-row suffix caches addressed by a slot table, and step 0 from the prefill logits.
 * opadpo_decode_step / _run / _all_finished / _end then work on the beam decode (B*k rows; selection on the device, nothing read back).
 * 1 <= k <= OPADPO_MAX_BEAMS, B*k <= 64, vocab >= 2k. */
int opadpo_decode_beam_begin(opadpo_ctx* ctx, int adapter_id, const int32_t* ids, const uint8_t* text_mask, const uint16_t* feats, int B, int Q,
                             int k, int max_new_tokens, int eos_id, int pad_id, void* stream);
/* synchronous: the best hypothesis per item into tokens [B, max_new_tokens] int32 (EOS kept, pad after it) and its score into scores [B]
 * fp32 (both device memory).  An item that is not done when this is called takes its running beams as finished (as a last step would). */
int opadpo_decode_beam_result(opadpo_ctx* ctx, int32_t* tokens, float* scores, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OPADPO_HIP_H */
