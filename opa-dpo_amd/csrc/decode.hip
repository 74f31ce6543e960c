// On-policy rollout kernels: single-token attention over a KV cache and the on-device
// temperature -> top-k -> top-p -> multinomial sampler (HF logits-processor order; the reference
// calls policy.generate(do_sample=True, top_k=30, top_p=0.95): online_generator.py:292-309).
#include <stdlib.h>
#include "common.h"
#include "kernels.h"
#include <algorithm>
#include <type_traits>

namespace {

// ---- single-token attention over the KV cache ("flash decoding") ----------------------------------------------------
// Cache layout is head-major: k_cache / v_cache [B, nh, max_ctx, HD], so one (sequence, head) is a contiguous stream
// of HD*2-byte rows -> every wave load instruction covers 1 KiB of consecutive bytes.  HBM-bound: 2*HD*2 bytes per key.
// grid = (nh, B, splits), NW waves.  HD/8 lanes share one key (16 B of K and of V each), so a wave covers 64/(HD/8)
// keys per step and the block NW x that; U steps are issued back to back (U K-loads + U V-loads in flight per lane).
// Each lane group keeps an online softmax (running max / sum / 8 output dims per lane); groups merge through LDS.
// NW = 4 when B*nh alone oversubscribes the 256 CUs, 16 (one fat block per CU, 128 KiB of loads in flight) otherwise.
// splits > 1 (B*nh < 256): the key range is cut into pieces, every block writes (max, sum, out[HD]) to the workspace
// and attn_decode_merge_kernel combines them (a kernel boundary is the cheapest device-wide release/acquire here: a
// per-block agent-scope fence costs an L2 write-back per block on a multi-XCD part).
// FUSE (decode step of the generator): q points at the [q|k|v] rows of the NEW token straight out of the projection.  Every
// block rotates its q chunk itself (RoPE at position pos = ctx_ptr[0]; a lane fetches its 8 elements and the 8 of its
// rotation partner 64 columns away); the block whose key range contains pos also rotates the new k, appends k and v to the
// caches and folds that key into its online softmax from registers (the loop skips slot pos, so there is no
// write -> read dependence through memory inside the launch).  Replaces rope_kv_append + attn_decode: one launch less per
// layer and step.  Rounding points are those of the two-kernel path (rotated q and k rounded to bf16 before use).
// BEAM (one BeamDec after the last argument; beam search, FUSE only): row b = blockIdx.y is beam b % k of item b / k.  kc / vc = the items'
// shared prefix caches [items, nh, Lp, HD] (key_mask [items, Lp]); kc_w / vc_w = the suffix caches [rows, nh, max_new, HD]: the key of suffix
// slot s = j - Lp of row b lives in physical row table[b][s], and the new token's key is appended at (b, pos - Lp).  The table is
// double-buffered by the parity of s + 1 for the appended slot s.  The non-beam instantiations (empty pack) are the kernel as it was.
// SHARED (one SharedDec instead of the BeamDec; n sampled responses per prompt, opadpo_attn_decode_shared): the beam layout with the identity slot
// table (row b reads and appends its own suffix row; table = nullptr), k = responses per item.  key0 = first key of the launch (0: the whole
// context, the per-row form, same split rule and key order as the fused kernel; Lp: the suffix part of the grouped form), slots > 0: every block
// writes its (max, sum, out) partial into slot slot0 + split of the row's `slots` slots, whatever gridDim.z is.
struct BeamDec { const int32_t* table; long long tstride; int Lp, max_new, k; };
struct SharedDec : BeamDec { int key0, slots, slot0; };
// ROWS (one RowsDec after the last argument; continuous rollout, FUSE only, opadpo_attn_decode_fused_rows): ctx_ptr is an array [B] and row b sits at its
// OWN position ctx_ptr[b] - the rows of one launch have different context lengths.  Everything below depends on the row's ctx alone (the key ranges,
// `per`, the block that appends), so row b computes what the fused kernel computes for it when every row sits at ctx_ptr[b].  The position is clamped
// into [0, max_ctx - 1]: an idle slot never indexes the RoPE tables, the caches or the key mask outside its own extent.
struct RowsDec {};
template <int HD, int NW, bool FUSE = false, typename... BA>
__global__ __launch_bounds__(NW * 64) void attn_decode_kernel(const bf16_t* q, int ldq, const bf16_t* kc, const bf16_t* vc,
                                                               bf16_t* o, const uint8_t* key_mask, int nh, int ctx_arg,
                                                               const int32_t* ctx_ptr, int max_ctx, float scale_log2e, float* ws_part,
                                                               const float* cosb = nullptr, const float* sinb = nullptr,
                                                               bf16_t* kc_w = nullptr, bf16_t* vc_w = nullptr, BA... beam) {
  constexpr bool ROWS = (std::is_same_v<BA, RowsDec> || ...);
  constexpr bool BEAM = sizeof...(BA) > 0 && !ROWS;
  constexpr bool SHARED = (std::is_same_v<BA, SharedDec> || ...);
  static_assert((!BEAM && !ROWS) || FUSE, "the beam and per-row-position forms append the new token: FUSE only");
  constexpr int LPK = HD / 8;            // lanes per key
  constexpr int KPW = 64 / LPK;          // keys per wave step
  constexpr int NG = NW * KPW;           // lane groups (= keys per block step)
  constexpr int U = 4;
  __shared__ float sm_m[NG], sm_l[NG];
  __shared__ __attribute__((aligned(16))) float sm_acc[NG][HD];
  const int ctx = ROWS ? min(max(ctx_ptr[blockIdx.y], 0) + 1, max_ctx)      // the row's own position, held inside its cache
                       : ctx_ptr ? min(ctx_ptr[0] + 1, max_ctx) : ctx_arg;   // device-resident: keys 0..pos (graph replay)
  const int h = blockIdx.x, b = blockIdx.y, split = blockIdx.z, splits = gridDim.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane / LPK, d = lane % LPK;
  int key0 = 0;
  if constexpr (SHARED) key0 = (beam, ...).key0;
  const int per = (((ctx - key0 + splits - 1) / splits) + NG - 1) / NG * NG;
  const int s0 = key0 + split * per, s1 = min(ctx, s0 + per);

  float qf[8];
  const int pos = FUSE ? ctx - 1 : -1;                 // slot of the token this step appends
  // rotate 8 elements of a head row: own chunk d*8.. and the partner chunk 64 columns away (first half: x1 c - x2 s, second: x2 c + x1 s)
  auto rope8 = [&](const bf16_t* row, float (&out)[8]) {
    constexpr int half = HD / 2;
    const bool lo = d * 8 < half;
    const int i0 = lo ? d * 8 : d * 8 - half;
    float own[8], oth[8];
    unpack8(*(const uint4*)(row + d * 8), own);
    unpack8(*(const uint4*)(row + (lo ? d * 8 + half : d * 8 - half)), oth);
    const float* cp = cosb + (size_t)pos * half + i0;
    const float* sp = sinb + (size_t)pos * half + i0;
#pragma unroll
    for (int e = 0; e < 8; ++e) out[e] = lo ? own[e] * cp[e] - oth[e] * sp[e] : own[e] * cp[e] + oth[e] * sp[e];
    const uint4 rb = pack8(out);                       // the two-kernel path stores the rotated row as bf16
    unpack8(rb, out);
  };
  if constexpr (FUSE) rope8(q + (size_t)b * ldq + h * HD, qf);
  else unpack8(*(const uint4*)(q + (size_t)b * ldq + h * HD + d * 8), qf);
#pragma unroll
  for (int e = 0; e < 8; ++e) qf[e] *= scale_log2e;
  const size_t seq = ((size_t)b * nh + h) * max_ctx;
  const bf16_t* kb = kc + seq * HD + d * 8;
  const bf16_t* vb = vc + seq * HD + d * 8;
  const uint8_t* km = key_mask ? key_mask + (size_t)b * max_ctx : nullptr;
  // beam form: prefix rows of the item, the prefix mask [items, Lp], the row's slot table of this step's parity
  BeamDec bm{};
  const bf16_t *kpb = kb, *vpb = vb;
  const uint8_t* kmb = km;
  const int32_t* tbl = nullptr;
  if constexpr (BEAM) {
    bm = (beam, ...);
    const size_t pseq = ((size_t)(b / bm.k) * nh + h) * bm.Lp;
    kpb = kc + pseq * HD + d * 8; vpb = vc + pseq * HD + d * 8;
    kmb = key_mask ? key_mask + (size_t)(b / bm.k) * bm.Lp : nullptr;
    if constexpr (!SHARED) tbl = bm.table + (size_t)((pos - bm.Lp + 1) & 1) * bm.tstride + (size_t)b * bm.max_new;
  }

  float m = -1.0e30f, l = 0.f, acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  for (int jb = s0 + wave * KPW; jb < s1; jb += NG * U) {
    uint4 kk[U], vv[U];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = jb + u * NG + g;
      if constexpr (BEAM) ok[u] = j < s1 && (j >= bm.Lp || !kmb || kmb[j]) && j != pos;      // suffix keys are always visible
      else ok[u] = j < s1 && (!km || km[j]) && j != pos;
      kk[u] = make_uint4(0, 0, 0, 0);
      vv[u] = make_uint4(0, 0, 0, 0);
      if (j < s1 && j != pos) {          // slots >= ctx are never read (uninitialised memory may hold NaN bit patterns)
        // the KV cache is read exactly once per decode step: non-temporal loads stream it past the L2s (round 4; same-box B = 64: 9.24 -> 8.93 ms
        // per step, B = 8 neutral)
        typedef __attribute__((ext_vector_type(4))) unsigned u4n_t;
        if constexpr (BEAM) {
          const bf16_t* kp = kpb + (size_t)j * HD;
          const bf16_t* vp = vpb + (size_t)j * HD;
          if (j >= bm.Lp) {
            const int sl = j - bm.Lp;
            size_t prow = b;
            if constexpr (!SHARED) prow = tbl[sl];
            const size_t r = ((prow * nh + h) * bm.max_new + sl) * HD + d * 8;
            kp = kc_w + r; vp = vc_w + r;
          }
          const u4n_t a = __builtin_nontemporal_load((const u4n_t*)kp), c = __builtin_nontemporal_load((const u4n_t*)vp);
          kk[u] = make_uint4(a.x, a.y, a.z, a.w); vv[u] = make_uint4(c.x, c.y, c.z, c.w);
        } else {
        const u4n_t a = __builtin_nontemporal_load((const u4n_t*)(kb + (size_t)j * HD)), c = __builtin_nontemporal_load((const u4n_t*)(vb + (size_t)j * HD));
        kk[u] = make_uint4(a.x, a.y, a.z, a.w); vv[u] = make_uint4(c.x, c.y, c.z, c.w);
        }
      }
    }
    float sc[U];
    float mn = m;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float kf[8];
      unpack8(kk[u], kf);
      float a = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) a += kf[e] * qf[e];
#pragma unroll
      for (int off = 1; off < LPK; off <<= 1) a += __shfl_xor(a, off, 64);
      sc[u] = ok[u] ? a : -1.0e30f;
      mn = fmaxf(mn, sc[u]);
    }
    const float alpha = fast_exp2(m - mn);
    m = mn;
    l *= alpha;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] *= alpha;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float pj = ok[u] ? fast_exp2(sc[u] - m) : 0.f;
      float vf[8];
      unpack8(vv[u], vf);
      l += pj;
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += pj * vf[e];
    }
  }
  if constexpr (FUSE) {
    if (pos >= s0 && pos < s1 && wave == 0 && g == 0) {          // the new token's key: one lane group, from registers
      const size_t H = (size_t)nh * HD;
      const bf16_t* krow = q + (size_t)b * ldq + H + h * HD;
      float kf[8], vf[8];
      rope8(krow, kf);
      const uint4 vraw = *(const uint4*)(krow + H + d * 8);
      unpack8(vraw, vf);
      if constexpr (BEAM) {
        const size_t wrow = ((size_t)b * nh + h) * bm.max_new + (pos - bm.Lp);
        *(uint4*)(kc_w + wrow * HD + d * 8) = pack8(kf);
        *(uint4*)(vc_w + wrow * HD + d * 8) = vraw;
      } else {
      *(uint4*)(kc_w + (seq + pos) * HD + d * 8) = pack8(kf);
      *(uint4*)(vc_w + (seq + pos) * HD + d * 8) = vraw;
      }
      float a = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) a += kf[e] * qf[e];
#pragma unroll
      for (int off = 1; off < LPK; off <<= 1) a += __shfl_xor(a, off, 64);
      bool fold = true;                  // beam form: a runtime test too (pos >= Lp), so both forms fold the key through the same branch
      if constexpr (BEAM) fold = pos >= bm.Lp || !kmb || kmb[pos];
      if (fold && (BEAM || !km || km[pos])) {
        const float mn = fmaxf(m, a);
        const float alpha = fast_exp2(m - mn), pj = fast_exp2(a - mn);
        m = mn;
        l = l * alpha + pj;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = acc[e] * alpha + pj * vf[e];
      }
    }
  }
  const int grp = wave * KPW + g;
  if (d == 0) { sm_m[grp] = m; sm_l[grp] = l; }
  *(float4*)&sm_acc[grp][d * 8] = make_float4(acc[0], acc[1], acc[2], acc[3]);
  *(float4*)&sm_acc[grp][d * 8 + 4] = make_float4(acc[4], acc[5], acc[6], acc[7]);
  __syncthreads();
  if (tid < HD) {
    float M = -1.0e30f, Lsum = 0.f, O = 0.f;
#pragma unroll 4
    for (int i = 0; i < NG; ++i) M = fmaxf(M, sm_m[i]);
#pragma unroll 4
    for (int i = 0; i < NG; ++i) {
      const float w = fast_exp2(sm_m[i] - M);
      Lsum += sm_l[i] * w;
      O += sm_acc[i][tid] * w;
    }
    const int bh = b * nh + h;
    int slots = splits, slot = split;
    if constexpr (SHARED) {
      const SharedDec sd = (beam, ...);
      if (sd.slots > 0) { slots = sd.slots; slot = sd.slot0 + split; }
    }
    if (slots == 1) {
      o[(size_t)bh * HD + tid] = f2bf(Lsum > 0.f ? O / Lsum : 0.f);
    } else {
      float* part = ws_part + ((size_t)bh * slots + slot) * (HD + 2);
      part[2 + tid] = O;
      if (tid == 0) { part[0] = M; part[1] = Lsum; }
    }
  }
}

// one block per (sequence, head): out = sum_s w_s O_s / sum_s w_s L_s, w_s = 2^(M_s - max M)
__global__ void attn_decode_merge_kernel(const float* ws_part, bf16_t* o, int splits, int HD) {
  const int bh = blockIdx.x, tid = threadIdx.x;
  const float* p0 = ws_part + (size_t)bh * splits * (HD + 2);
  float MM = -1.0e30f;
  for (int i = 0; i < splits; ++i) MM = fmaxf(MM, p0[(size_t)i * (HD + 2)]);
  float LL = 0.f, OO = 0.f;
  for (int i = 0; i < splits; ++i) {
    const float* pi = p0 + (size_t)i * (HD + 2);
    const float w = fast_exp2(pi[0] - MM);
    LL += pi[1] * w;
    OO += pi[2 + tid] * w;
  }
  o[(size_t)bh * HD + tid] = f2bf(LL > 0.f ? OO / LL : 0.f);
}

// ---- grouped shared-prefix decode attention (num_return_sequences: n sampled responses per prompt; head_dim 128) -------------------------
// The n <= 16 rows of an item attend the SAME prefix keys, and a launch costs the bytes through a CU's vector-memory pipe whatever their source
// (DESIGN.md §4), so one workgroup owns (item, head, prefix key range), brings every K / V tile in ONCE and uses it against all n query rows,
// padded to one 16-row MFMA tile.  grid = (nh, items, ranges), 4 waves; wave w takes the 64-key tiles w, w + 4, .. of the range:
//   S^T[key][q] = K . Q^T    v_mfma_f32_16x16x32_bf16, A = K fragment (lane c = lane & 15 holds 16 consecutive bytes of key c, straight from the
//                            head-major cache, no LDS), B = the rotated q rows (rotation at pos = pos_ptr[0], rounded to bf16 as the per-row form
//                            rounds them); the accumulator has the query row on lane & 15 and 4 keys in its registers
//   O^T[d][q] += V^T . P^T   two 16-key accumulator tiles packed to bf16 ARE the B operand of a 32-key step (no lane movement); V is staged in the
//                            wave's own swizzled LDS tile and read transposed (ds_read_b64_tr_b16), the idiom of attention.hip
// Online softmax per query row in fp32 (log2 units); P is rounded to bf16 for the P.V MFMA - the one rounding point this form adds over the
// per-row form.  The waves' (m, l, O) merge through LDS and go out as partials in attn_decode_merge_kernel's format, slot = range index of the
// row's `slots` slots: plain vector stores, no atomics; the suffix launch fills the last slot and the merge is its own launch.
constexpr int GRP_W = 4, GRP_TILE = 64 * 128 * 2;
__device__ __forceinline__ int grp_at(int row, int byte) { return row * 256 + ((((byte >> 4) ^ ((row & 7) << 1))) << 4) + (byte & 15); }

__global__ __launch_bounds__(GRP_W * 64) void attn_decode_group_kernel(const bf16_t* qkv, int ld, const float* cosb, const float* sinb, const bf16_t* kp,
                                                                       const bf16_t* vp, const uint8_t* prefix_mask, int n, int nh,
                                                                       const int32_t* pos_ptr, int Lp, int per, int slots, float scale_log2e,
                                                                       float* ws_part) {
  constexpr int HD = 128;
  typedef __attribute__((ext_vector_type(4))) unsigned u4n_t;
  __shared__ __attribute__((aligned(16))) char smem[GRP_W * GRP_TILE];
  const int h = blockIdx.x, item = blockIdx.y, rg = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
  const int pos = pos_ptr[0];
  const int k_lo = rg * per, k_hi = min(Lp, k_lo + per);        // the host cuts the ranges so that none is empty
  const int ntiles = max(0, (k_hi - k_lo + 63) / 64), trips = (ntiles + GRP_W - 1) / GRP_W;
  // q fragments: B[k = 8g + j][col = c] = rotated q of row item * n + c at d = kk * 32 + 8g + j (rows >= n: zeros)
  bf16x8_t qf[4];
  {
    const bf16_t* qrow = qkv + (size_t)(item * n + min(c, n - 1)) * ld + h * HD;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      constexpr int half = HD / 2;
      const int d0 = kk * 32 + g * 8;
      const bool lo = d0 < half;
      const int i0 = lo ? d0 : d0 - half;
      float own[8], oth[8], out[8];
      unpack8(*(const uint4*)(qrow + d0), own);
      unpack8(*(const uint4*)(qrow + (lo ? d0 + half : d0 - half)), oth);
      const float* cp = cosb + (size_t)pos * half + i0;
      const float* sp = sinb + (size_t)pos * half + i0;
#pragma unroll
      for (int e = 0; e < 8; ++e) out[e] = lo ? own[e] * cp[e] - oth[e] * sp[e] : own[e] * cp[e] + oth[e] * sp[e];
      uint4 rb = pack8(out);
      if (c >= n) rb = make_uint4(0, 0, 0, 0);
      qf[kk] = *(const bf16x8_t*)&rb;
    }
  }
  const size_t pseq = ((size_t)item * nh + h) * Lp;
  const bf16_t* kb = kp + pseq * HD;
  const bf16_t* vb = vp + pseq * HD;
  const uint8_t* km = prefix_mask ? prefix_mask + (size_t)item * Lp : nullptr;
  char* const Vs = smem + wave * GRP_TILE;

  // a tile's loads: K fragments [16-key block kf][k-step kk], V rows i * 4 + g (16-byte chunk c), the lane's 16 visibility bits (key kf*16 + g*4 + r).
  // Keys behind the range end are clamped to its last key (never read out of bounds) and masked.
  uint4 kreg[4][4], vreg[16];
  uint32_t okreg = 0;
  auto fetch = [&](int t) {
    okreg = 0;
    if (t >= ntiles) return;                     // wave-uniform
    const int k0 = k_lo + t * 64;
#pragma unroll
    for (int kf = 0; kf < 4; ++kf) {
      const bf16_t* row = kb + (size_t)min(k0 + kf * 16 + c, k_hi - 1) * HD + g * 8;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const u4n_t a = __builtin_nontemporal_load((const u4n_t*)(row + kk * 32));
        kreg[kf][kk] = make_uint4(a.x, a.y, a.z, a.w);
      }
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const u4n_t a = __builtin_nontemporal_load((const u4n_t*)(vb + (size_t)min(k0 + i * 4 + g, k_hi - 1) * HD + c * 8));
      vreg[i] = make_uint4(a.x, a.y, a.z, a.w);
    }
#pragma unroll
    for (int kf = 0; kf < 4; ++kf)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = k0 + kf * 16 + g * 4 + r;
        const bool ok = key < k_hi && (!km || km[min(key, k_hi - 1)]);
        okreg |= (ok ? 1u : 0u) << (kf * 4 + r);
      }
  };

  float m_run = -1.0e30f, l_run = 0.f;
  f32x4_t o[8];
#pragma unroll
  for (int d = 0; d < 8; ++d) o[d] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  fetch(wave);
  for (int trip = 0; trip < trips; ++trip) {
    const int t = trip * GRP_W + wave;
    const bool live = t < ntiles;                // wave-uniform
    uint4 kcur[4][4];
    const uint32_t okb = okreg;
    if (live) {
#pragma unroll
      for (int i = 0; i < 16; ++i) *(uint4*)(Vs + grp_at(i * 4 + g, c * 16)) = vreg[i];
#pragma unroll
      for (int kf = 0; kf < 4; ++kf)
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) kcur[kf][kk] = kreg[kf][kk];
    }
    __syncthreads();
    if (trip + 1 < trips) fetch(t + GRP_W);      // the next tile's loads fly while this one is consumed
    if (live) {
      f32x4_t sc[4];
#pragma unroll
      for (int kf = 0; kf < 4; ++kf) {
        sc[kf] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
          sc[kf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8_t*)&kcur[kf][kk], qf[kk], sc[kf], 0, 0, 0);
      }
      // sc[kf][r] = S^T[key = kf*16 + g*4 + r][q = c]
      float mx = -1.0e30f;
#pragma unroll
      for (int kf = 0; kf < 4; ++kf)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          sc[kf][r] = (okb >> (kf * 4 + r) & 1u) ? sc[kf][r] * scale_log2e : -INFINITY;      // exp2(-inf - m) = 0 (m stays finite)
          mx = fmaxf(mx, sc[kf][r]);
        }
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m_run, mx);
      float psum = 0.f;
#pragma unroll
      for (int kf = 0; kf < 4; ++kf)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float pv = fast_exp2(sc[kf][r] - m_new);
          sc[kf][r] = pv;
          psum += pv;
        }
      const float alpha = fast_exp2(m_run - m_new);
      l_run = l_run * alpha + psum;
      m_run = m_new;
#pragma unroll
      for (int d = 0; d < 8; ++d) { o[d][0] *= alpha; o[d][1] *= alpha; o[d][2] *= alpha; o[d][3] *= alpha; }
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        union { bf16x8_t v; uint32_t w[4]; } pf;
        pf.w[0] = pack_bf2(sc[2 * ks][0], sc[2 * ks][1]); pf.w[1] = pack_bf2(sc[2 * ks][2], sc[2 * ks][3]);
        pf.w[2] = pack_bf2(sc[2 * ks + 1][0], sc[2 * ks + 1][1]); pf.w[3] = pack_bf2(sc[2 * ks + 1][2], sc[2 * ks + 1][3]);
        const int r0 = (2 * ks) * 16 + g * 4 + (c >> 2), r1 = r0 + 16;
#pragma unroll
        for (int d = 0; d < 8; ++d) {
          // A[row = c][k = j]: V[key r0 + j][d * 16 + c] (j < 4), V[key r1 + j - 4][d * 16 + c] - the keys the lane's P registers hold
          union { bf16x8_t v; s16x4_t hh[2]; } vf;
          const int byte = (d * 16 + (c & 3) * 4) * 2;
          vf.hh[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4_t, Vs + grp_at(r0, byte)));
          vf.hh[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4_t, Vs + grp_at(r1, byte)));
          o[d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf.v, pf.v, o[d], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }
  l_run += __shfl_xor(l_run, 16, 64);
  l_run += __shfl_xor(l_run, 32, 64);
  // the four waves' partials of row c: [wave][row][m, l, O[HD]] over the V tiles (every wave is past its last read: the loop ends on a barrier)
  float* const red = (float*)smem;
  {
    float* mine = red + (size_t)(wave * 16 + c) * (HD + 2);
    if (g == 0) { mine[0] = m_run; mine[1] = l_run; }
#pragma unroll
    for (int d = 0; d < 8; ++d)
#pragma unroll
      for (int r = 0; r < 4; ++r) mine[2 + d * 16 + g * 4 + r] = o[d][r];      // o[d][r] = O^T[d*16 + g*4 + r][q = c]
  }
  __syncthreads();
  for (int idx = tid; idx < n * HD; idx += GRP_W * 64) {
    const int row = idx / HD, d = idx % HD;
    float M = -1.0e30f;
#pragma unroll
    for (int w = 0; w < GRP_W; ++w) M = fmaxf(M, red[(size_t)(w * 16 + row) * (HD + 2)]);
    float L = 0.f, O = 0.f;
#pragma unroll
    for (int w = 0; w < GRP_W; ++w) {
      const float* pw = red + (size_t)(w * 16 + row) * (HD + 2);
      const float wt = fast_exp2(pw[0] - M);
      L += pw[1] * wt;
      O += pw[2 + d] * wt;
    }
    float* part = ws_part + ((size_t)((item * n + row) * nh + h) * slots + rg) * (HD + 2);
    part[2 + d] = O;
    if (d == 0) { part[0] = M; part[1] = L; }
  }
}

// ---- decode-step RoPE + KV-cache append: q rotated in place, k rotated into k_cache[b,h,pos,:], v copied into
// v_cache[b,h,pos,:] (pos = pos_ptr[0], device-resident).  qkv rows are [q(H) | k(H) | v(H)].  One launch replaces
// rope + 2x(gather, scatter).
__global__ __launch_bounds__(256) void rope_kv_append_kernel(bf16_t* qkv, int ld, const float* cosb, const float* sinb, bf16_t* kc,
                                                              bf16_t* vc, int B, int nh, int hd, const int32_t* pos_ptr, int max_ctx) {
  const int half = hd / 2, cpr = half / 8;        // chunks (8 pairs) per head
  const int total = B * nh * cpr;
  const int pos = pos_ptr[0];
  for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
    const int b = idx / (nh * cpr), rem = idx % (nh * cpr);
    const int h = rem / cpr, i0 = (rem % cpr) * 8;
    const float* cp = cosb + (size_t)pos * half + i0;
    const float* sp = sinb + (size_t)pos * half + i0;
    const size_t H = (size_t)nh * hd;
    bf16_t* qp = qkv + (size_t)b * ld + h * hd;
    const bf16_t* kp = qp + H;
    const bf16_t* vp = qp + 2 * H;
    const size_t crow = (((size_t)b * nh + h) * max_ctx + pos) * hd;
    float x1[8], x2[8], o1[8], o2[8];
    unpack8(*(const uint4*)(qp + i0), x1);
    unpack8(*(const uint4*)(qp + half + i0), x2);
#pragma unroll
    for (int j = 0; j < 8; ++j) { o1[j] = x1[j] * cp[j] - x2[j] * sp[j]; o2[j] = x2[j] * cp[j] + x1[j] * sp[j]; }
    *(uint4*)(qp + i0) = pack8(o1);
    *(uint4*)(qp + half + i0) = pack8(o2);
    unpack8(*(const uint4*)(kp + i0), x1);
    unpack8(*(const uint4*)(kp + half + i0), x2);
#pragma unroll
    for (int j = 0; j < 8; ++j) { o1[j] = x1[j] * cp[j] - x2[j] * sp[j]; o2[j] = x2[j] * cp[j] + x1[j] * sp[j]; }
    *(uint4*)(kc + crow + i0) = pack8(o1);
    *(uint4*)(kc + crow + half + i0) = pack8(o2);
    *(uint4*)(vc + crow + i0) = *(const uint4*)(vp + i0);
    *(uint4*)(vc + crow + half + i0) = *(const uint4*)(vp + half + i0);
  }
}

__device__ __forceinline__ uint32_t fkey(float f) {   // monotone float -> uint map
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ uint64_t mix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// Per-row form of both samplers (one SampRows after the last argument; continuous rollout, opadpo_sample_rows): row = slot.  The draw stays
// f(seed, step, row) with seed = seed[row] and step = step[row]; the token goes to the slot's OWN history row, history [rows, max_steps] at
// [row, step]; the writer then advances step[row] and marks the row finished when it drew EOS or wrote its cap[row]-th token.  A finished row - or
// one whose step is not inside [0, min(cap, max_steps)), which only a caller's mistake produces - emits pad into `out` and touches nothing else:
// no history slot, no step.  ids (nullable): workgroup i samples row ids[i] (the admitted slots of a running session; logits row = the slot's).
struct SampRows { const uint64_t* seed; int32_t* step; const int32_t* cap; const int32_t* ids; int max_steps; };
// the one place a sampled token (or the pad of an empty kept set: eos = false) leaves the kernel
template <bool ROWS>
__device__ __forceinline__ void sample_emit(int row, int rows, int tok, uint64_t step, bool eos, uint8_t* finished, int eos_id, int32_t* out,
                                            int32_t* history, const SampRows& sr) {
  out[row] = tok;
  if constexpr (ROWS) {
    if (history) history[(size_t)row * sr.max_steps + step] = tok;
    sr.step[row] = (int32_t)step + 1;
    if ((eos && eos_id >= 0 && tok == eos_id) || (int)step + 1 >= sr.cap[row]) finished[row] = 1;
  } else {
    if (history) history[step * rows + row] = tok;
    if (eos && finished && eos_id >= 0 && tok == eos_id) finished[row] = 1;
  }
}
// the per-row form's row, seed and step; true: the row is idle (finished, or its step outside its extent) and has emitted pad
template <bool ROWS>
__device__ __forceinline__ bool sample_row_state(const SampRows& sr, const uint8_t* finished, int pad_id, int32_t* out, int tid, int& row, uint64_t& seed,
                                                 uint64_t& step) {
  if constexpr (ROWS) {
    if (sr.ids) row = sr.ids[row];
    const int s = sr.step[row];
    if (finished[row] || s < 0 || s >= sr.cap[row] || s >= sr.max_steps) {
      if (tid == 0) out[row] = pad_id;
      return true;
    }
    seed = sr.seed[row];
    step = (uint64_t)s;
  }
  return false;
}

// step_ptr (nullable): device-resident step counter (graph replay) used for the RNG stream and, with `history`
// ([max_steps, rows]), for the slot the token is appended to.  eos_id >= 0: a row that samples EOS is marked finished.
template <typename... RA>
__global__ __launch_bounds__(256) void sample_kernel_generic(const float* logits, int ldl, int V, float inv_temp, int top_k, float top_p,
                                                      uint64_t seed, uint64_t step_arg, const int32_t* step_ptr, uint8_t* finished,
                                                      int pad_id, int eos_id, int32_t* out, int32_t* history, RA... ra) {
  constexpr bool ROWS = sizeof...(RA) > 0;
  uint64_t step = step_ptr ? (uint64_t)step_ptr[0] : step_arg;
  __shared__ float red[4];
  __shared__ float scan[256];
  __shared__ uint32_t s_thr;
  int row = blockIdx.x;
  const int tid = threadIdx.x;
  SampRows sr{};
  if constexpr (ROWS) sr = (ra, ...);
  if (sample_row_state<ROWS>(sr, finished, pad_id, out, tid, row, seed, step)) return;
  if (!ROWS && finished && finished[row]) {
    if (tid == 0) {
      out[row] = pad_id;
      if (history) history[step * gridDim.x + row] = pad_id;
    }
    return;
  }
  const float* z = logits + (size_t)row * ldl;
  float mx = -3.0e38f;
  for (int i = tid; i < V; i += 256) mx = fmaxf(mx, z[i] * inv_temp);
  mx = block_max_256(mx, red);

  uint32_t thr = 0;   // keep tokens with key >= thr
  if (top_k > 0 && top_k < V) {
    for (int bit = 31; bit >= 0; --bit) {
      const uint32_t cand = thr | (1u << bit);
      float cnt = 0.f;
      for (int i = tid; i < V; i += 256) cnt += (fkey(z[i] * inv_temp) >= cand) ? 1.f : 0.f;
      cnt = block_sum_256(cnt, red);
      if (cnt >= (float)top_k) thr = cand;
    }
  }
  if (top_p < 1.0f) {
    float zk = 0.f;
    for (int i = tid; i < V; i += 256) {
      const float v = z[i] * inv_temp;
      if (fkey(v) >= thr) zk += __expf(v - mx);
    }
    zk = block_sum_256(zk, red);
    const float budget = (1.0f - top_p) * zk;
    uint32_t t2 = 0;
    for (int bit = 31; bit >= 0; --bit) {
      const uint32_t cand = t2 | (1u << bit);
      float mass = 0.f;
      for (int i = tid; i < V; i += 256) {
        const float v = z[i] * inv_temp;
        const uint32_t k = fkey(v);
        if (k >= thr && k < cand) mass += __expf(v - mx);
      }
      mass = block_sum_256(mass, red);
      if (mass <= budget) t2 = cand;
    }
    thr = max(thr, t2);
  }
  // multinomial over the kept set, cumulative in index order; thread t owns a contiguous chunk
  const int chunk = (V + 255) / 256;
  const int lo = tid * chunk, hi = min(V, lo + chunk);
  float local = 0.f;
  for (int i = lo; i < hi; ++i) {
    const float v = z[i] * inv_temp;
    if (fkey(v) >= thr) local += __expf(v - mx);
  }
  scan[tid] = local;
  __syncthreads();
  const uint64_t r = mix64(mix64(seed ^ (step * 0xD1B54A32D192ED03ull)) + (uint64_t)row);
  const float u = ((float)(r >> 40) + 0.5f) * (1.0f / 16777216.0f);
  if (tid == 0) {
    float total = 0.f;
    for (int i = 0; i < 256; ++i) total += scan[i];
    const float target = u * total;
    float run = 0.f;
    int owner = 0;
    float owner_start = 0.f;
    for (int i = 0; i < 256; ++i) {          // last non-empty chunk whose start is <= target
      if (scan[i] > 0.f && run <= target) { owner = i; owner_start = run; }
      run += scan[i];
    }
    s_thr = (uint32_t)owner;
    red[0] = target;
    red[1] = owner_start;
  }
  __syncthreads();
  if (tid == (int)s_thr) {
    const float target = red[0];
    float run = red[1];
    int pick = pad_id;
    for (int i = lo; i < hi; ++i) {
      const float v = z[i] * inv_temp;
      if (fkey(v) >= thr) {
        run += __expf(v - mx);
        pick = i;
        if (run > target) break;
      }
    }
    sample_emit<ROWS>(row, gridDim.x, pick, step, true, finished, eos_id, out, history, sr);
  }
}


// ---- fast sampler: the whole row lives in LDS ------------------------------------------------------------------------
// 1024 threads per row; the temperature-scaled row (V <= 32768 floats = 128 KiB of the CU's 160 KiB LDS) is read from
// memory ONCE, every later pass is a conflict-free stride-1 LDS sweep (the generic kernel makes ~66 passes over memory).
// Same filter semantics as the generic kernel:
//   top-k : 4-level radix select (8-bit digits of the monotone key) with an LDS histogram of counts ->
//           thr = key of the k-th largest logit (ties kept);
//   top-p : the same descent over a histogram of probability MASS -> largest t2 with mass(thr <= key < t2) <= (1-p)*Z.
//           Mass is fixed-point (2^-40 of the row maximum) in uint64, so LDS atomics are exact and order-independent:
//           the draw is deterministic for (seed, step, row);
//   draw  : block-wide exclusive scan of the per-thread kept mass, the owner thread walks its <= 32 values.
constexpr int SAMP_T = 1024, SAMP_W = SAMP_T / 64, SAMP_MAXV = 32768;
constexpr float SAMP_FIX = 1099511627776.0f;   // 2^40

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (uint64_t)__shfl_xor((long long)v, o, 64);
  return v;
}

// digit choice for one radix level, executed by wave 0: hist[256] (uint64) -> LDS result {digit, carried sum}.
//   DESC (top-k):  largest digit d with base + sum(hist[d..255]) >= need;   carry = base + sum(hist[d+1..255])
//   !DESC (top-p): largest digit d with base + sum(hist[0..d-1]) <= need;   carry = base + sum(hist[0..d-1])
template <bool DESC>
__device__ __forceinline__ void pick_digit(const uint64_t* hist, uint64_t base, uint64_t need, int lane, uint32_t* out_digit,
                                           uint64_t* out_carry) {
  uint64_t c[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) c[i] = hist[lane * 4 + i];
  const uint64_t s = c[0] + c[1] + c[2] + c[3];
  uint64_t incl = s;                       // DESC: sum over lanes >= lane ; else: sum over lanes <= lane
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint64_t t = (uint64_t)(DESC ? __shfl_down((long long)incl, off, 64) : __shfl_up((long long)incl, off, 64));
    if (DESC ? (lane + off < 64) : (lane >= off)) incl += t;
  }
  const uint64_t outside = base + incl - s;   // DESC: bins above this lane's 4 ; else: bins below this lane's 4
  uint64_t S[4];                              // DESC: base + sum(hist[bin..255]) ; else: base + sum(hist[0..bin-1])
  if (DESC) {
    S[3] = outside + c[3]; S[2] = S[3] + c[2]; S[1] = S[2] + c[1]; S[0] = S[1] + c[0];
  } else {
    S[0] = outside; S[1] = S[0] + c[0]; S[2] = S[1] + c[1]; S[3] = S[2] + c[2];
  }
  int cnt = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) cnt += DESC ? (S[i] >= need) : (S[i] <= need);
  int total = cnt;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) total += __shfl_xor(total, o, 64);
  const int dsel = max(total - 1, 0);          // satisfying bins form the prefix [0..dsel]
  if (lane == (dsel >> 2)) {
    const int i = dsel & 3;
    *out_digit = (uint32_t)dsel;
    *out_carry = DESC ? (S[i] - c[i]) : S[i];
  }
}

template <typename... RA>
__global__ __launch_bounds__(SAMP_T) void sample_kernel_fast(const float* logits, int ldl, int V, float inv_temp, int top_k, float top_p,
                                                             uint64_t seed, uint64_t step_arg, const int32_t* step_ptr, uint8_t* finished,
                                                             int pad_id, int eos_id, int32_t* out, int32_t* history, int compact, RA... ra) {
  constexpr bool ROWS = sizeof...(RA) > 0;
  extern __shared__ __attribute__((aligned(16))) float zs[];     // [V] scaled logits
  uint64_t step = step_ptr ? (uint64_t)step_ptr[0] : step_arg;
  __shared__ uint64_t hist[256];
  __shared__ uint64_t wsum[SAMP_W];
  __shared__ float wmax[SAMP_W];
  __shared__ uint32_t s_digit;
  __shared__ uint64_t s_carry;
  int row = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  SampRows sr{};
  if constexpr (ROWS) sr = (ra, ...);
  if (sample_row_state<ROWS>(sr, finished, pad_id, out, tid, row, seed, step)) return;
  if (!ROWS && finished && finished[row]) {
    if (tid == 0) {
      out[row] = pad_id;
      if (history) history[step * gridDim.x + row] = pad_id;
    }
    return;
  }
  const float4* z4 = (const float4*)(logits + (size_t)row * ldl);
  float mx = -3.0e38f;
  for (int gi = tid; gi < (V >> 2); gi += SAMP_T) {
    float4 t = z4[gi];
    t.x *= inv_temp; t.y *= inv_temp; t.z *= inv_temp; t.w *= inv_temp;
    *(float4*)&zs[gi * 4] = t;
    mx = fmaxf(fmaxf(mx, fmaxf(t.x, t.y)), fmaxf(t.z, t.w));
  }
  mx = wave_max(mx);
  if (lane == 0) wmax[wave] = mx;
  __syncthreads();
  mx = wmax[0];
#pragma unroll
  for (int i = 1; i < SAMP_W; ++i) mx = fmaxf(mx, wmax[i]);
  auto qmass = [&](float x) -> uint64_t { return (uint64_t)(__expf(x - mx) * SAMP_FIX); };   // exp(-inf) = 0
  auto block_sum = [&](uint64_t x) -> uint64_t {
    x = wave_sum_u64(x);
    __syncthreads();
    if (lane == 0) wsum[wave] = x;
    __syncthreads();
    uint64_t t = 0;
#pragma unroll
    for (int i = 0; i < SAMP_W; ++i) t += wsum[i];
    return t;
  };

  uint32_t thr = 0;   // keep tokens with key >= thr
  if (top_k > 0 && top_k < V) {
    uint32_t prefix = 0, pmask = 0;
    uint64_t above = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
      if (tid < 256) hist[tid] = 0;
      __syncthreads();
      for (int base = 0; base < V; base += SAMP_T) {
        const int i = base + tid;
        const uint32_t k = i < V ? fkey(zs[i]) : 0u;
        bool mine = i < V && (k & pmask) == prefix;
        const uint32_t dg = (k >> shift) & 255u;
        // wave-aggregated counting for crowded bins (the top byte of a float key takes only a few values)
#pragma unroll 1
        for (int it = 0; it < 3; ++it) {
          const uint64_t act = __ballot(mine);
          if (!act) break;
          const int lead = __ffsll((long long)act) - 1;
          const uint32_t ldg = __shfl(dg, lead, 64);
          const uint64_t same = __ballot(mine && dg == ldg);
          if (lane == lead) atomicAdd((unsigned long long*)&hist[ldg], (unsigned long long)__popcll(same));
          if (dg == ldg) mine = false;
        }
        if (mine) atomicAdd((unsigned long long*)&hist[dg], 1ull);
      }
      __syncthreads();
      if (wave == 0) pick_digit<true>(hist, above, (uint64_t)top_k, lane, &s_digit, &s_carry);
      __syncthreads();
      prefix |= s_digit << shift;
      pmask |= 255u << shift;
      above = s_carry;
      __syncthreads();
    }
    thr = prefix;
    // COMPACT tail (round 4): after the top-k threshold the kept set is a few dozen tokens, yet the top-p descent, the mass sums and the draw
    // swept the whole vocabulary seven more times.  The kept tokens are gathered into an LDS list (one more sweep); when they are at most 64,
    // wave 0 finishes alone, one token per lane, with the SAME integer arithmetic: the masses are exact fixed-point integers, so their sums do not
    // depend on the order; the top-p threshold "largest t with mass(thr <= key < t) <= budget" is the smallest kept key whose mass of keys <= it
    // exceeds the budget (none: 2^32 - 1); the draw walks the kept tokens in the order (owner thread = index mod 1024, index) of the full-sweep
    // form.  Same token for every (seed, step, row) as the sweeps (tests/test_ops_gpu.py::test_sampler_compact_tail_is_exact); more than 64 kept
    // tokens (ties at the threshold) fall through to the sweeps.
    if (compact) {
      __shared__ int s_n;
      __shared__ int s_idx[64];
      if (tid == 0) s_n = 0;
      __syncthreads();
      for (int i = tid; i < V; i += SAMP_T)
        if (fkey(zs[i]) >= thr) {
          const int pos = atomicAdd(&s_n, 1);
          if (pos < 64) s_idx[pos] = i;
        }
      __syncthreads();
      const int n = s_n;
      if (n <= 64) {
        if (wave != 0) return;
        const bool valid = lane < n;
        const int idx = valid ? s_idx[lane] : 0x7fffffff;
        const float x = valid ? zs[idx] : 0.f;
        const uint32_t key = valid ? fkey(x) : 0u;
        const uint64_t qm = valid ? qmass(x) : 0ull;
        uint32_t thr2 = thr;
        if (top_p < 1.0f) {
          const uint64_t zk = wave_sum_u64(qm);
          const uint64_t budget = (uint64_t)((1.0 - (double)top_p) * (double)zk);
          uint64_t below_incl = 0;                         // mass of the kept keys <= this lane's key
          for (int j = 0; j < n; ++j) {
            const uint32_t kj = (uint32_t)__shfl((int)key, j, 64);
            const uint64_t qj = (uint64_t)__shfl((long long)qm, j, 64);
            if (kj <= key) below_incl += qj;
          }
          uint32_t t2 = (valid && below_incl > budget) ? key : 0xffffffffu;
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) t2 = min(t2, (uint32_t)__shfl_xor((int)t2, o, 64));
          thr2 = max(thr, t2);
        }
        const bool kept = valid && key >= thr2;
        const uint64_t qk = kept ? qm : 0ull;
        const uint64_t total = wave_sum_u64(qk);
        const uint32_t ord = ((uint32_t)(idx & (SAMP_T - 1)) << 20) | (uint32_t)(idx >> 10);      // (owner thread, then index): V <= 32768 -> index / 1024 < 32
        uint64_t before = 0;                               // kept mass ahead of this lane's token in the draw order
        for (int j = 0; j < n; ++j) {
          const uint32_t oj = (uint32_t)__shfl((int)ord, j, 64);
          const uint64_t qj = (uint64_t)__shfl((long long)qk, j, 64);
          if (oj < ord) before += qj;
        }
        const uint64_t r = mix64(mix64(seed ^ (step * 0xD1B54A32D192ED03ull)) + (uint64_t)row);
        const uint64_t r24 = r >> 40;
        const uint64_t target = (total >> 24) * r24 + (((total & 0xffffffull) * r24) >> 24);
        if (total == 0) {
          if (lane == 0) sample_emit<ROWS>(row, gridDim.x, pad_id, step, false, finished, eos_id, out, history, sr);
          return;
        }
        if (qk > 0 && before <= target && target < before + qk) sample_emit<ROWS>(row, gridDim.x, idx, step, true, finished, eos_id, out, history, sr);
        return;
      }
    }
  }
  if (top_p < 1.0f) {
    uint64_t zk = 0;
    for (int i = tid; i < V; i += SAMP_T) {
      const float x = zs[i];
      if (fkey(x) >= thr) zk += qmass(x);
    }
    zk = block_sum(zk);
    const uint64_t budget = (uint64_t)((1.0 - (double)top_p) * (double)zk);
    uint32_t prefix = 0, pmask = 0;
    uint64_t below = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
      if (tid < 256) hist[tid] = 0;
      __syncthreads();
      for (int i = tid; i < V; i += SAMP_T) {
        const float x = zs[i];
        const uint32_t k = fkey(x);
        if (k >= thr && (k & pmask) == prefix) {
          const uint64_t qm = qmass(x);
          if (qm) atomicAdd((unsigned long long*)&hist[(k >> shift) & 255u], (unsigned long long)qm);
        }
      }
      __syncthreads();
      if (wave == 0) pick_digit<false>(hist, below, budget, lane, &s_digit, &s_carry);
      __syncthreads();
      prefix |= s_digit << shift;
      pmask |= 255u << shift;
      below = s_carry;
      __syncthreads();
    }
    thr = max(thr, prefix);
  }
  // multinomial over the kept set; cumulative order = (thread, then index) — any fixed order is a valid draw
  uint64_t local = 0;
  for (int i = tid; i < V; i += SAMP_T) {
    const float x = zs[i];
    if (fkey(x) >= thr) local += qmass(x);
  }
  uint64_t incl = local;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint64_t t = (uint64_t)__shfl_up((long long)incl, off, 64);
    if (lane >= off) incl += t;
  }
  __syncthreads();
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  uint64_t wave_base = 0, total = 0;
#pragma unroll
  for (int i = 0; i < SAMP_W; ++i) {
    if (i < wave) wave_base += wsum[i];
    total += wsum[i];
  }
  const uint64_t r = mix64(mix64(seed ^ (step * 0xD1B54A32D192ED03ull)) + (uint64_t)row);
  const uint64_t r24 = r >> 40;                                   // u = r24 / 2^24 in [0, 1)
  const uint64_t target = (total >> 24) * r24 + (((total & 0xffffffull) * r24) >> 24);   // floor(u * total) < total
  const uint64_t start = wave_base + incl - local;
  if (total == 0) {
    if (tid == 0) sample_emit<ROWS>(row, gridDim.x, pad_id, step, false, finished, eos_id, out, history, sr);
    return;
  }
  if (local > 0 && start <= target && target < start + local) {
    uint64_t run = start;
    int pick = pad_id;
    for (int i = tid; i < V && run <= target; i += SAMP_T) {
      const float x = zs[i];
      if (fkey(x) >= thr) {
        const uint64_t qm = qmass(x);
        if (qm) pick = i;
        run += qm;
      }
    }
    sample_emit<ROWS>(row, gridDim.x, pick, step, true, finished, eos_id, out, history, sr);
  }
}

// ---- logits processors of the yes/no evaluation generator (eval_llava_rlhf_coco/model_vqa_logit.py:107-121,182-202) -----------------------
// logit_bias_add: HF's sequence_bias restricted to one-token sequences = an additive bias on those tokens' logits, applied to the fp32 logits
// [rows, V] of a step BEFORE temperature / top-k / top-p (logits processors run before the warpers) and to every row, finished ones included
// (they emit pad whatever their logits are).  One thread per (row, table entry); the host refuses duplicate ids, so no two threads share an
// address.  ids outside [0, V) never reach the kernel (launch_logit_bias_add); the guard keeps a stale table from writing out of the row.
__global__ __launch_bounds__(256) void logit_bias_add_kernel(float* logits, int ldl, int rows, int V, const int32_t* ids, const float* bias, int n) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * n) return;
  const int row = idx / n, e = idx - row * n;
  const int id = ids[e];
  if ((unsigned)id >= (unsigned)V) return;
  logits[(size_t)row * ldl + id] += bias[e];
}

// gather_scores: scores[row, j] = the PROCESSED score of token ids[j] as HF's generate(output_scores=True) records it for a sampled step:
// v = logit / temperature (the bias is in the logits already), then top-k (keep v >= the k-th largest v, ties kept), then top-p on the
// softmax of what top-k kept (ascending cumulative mass <= 1 - top_p is cut, the largest token always stays); a cut token reads -inf.
// temperature == 0 (this tree's greedy): the raw logit, nothing cut.  One workgroup per row; runs once per generation, so the top-k
// threshold is the plain 32-step bitwise descent of sample_kernel_generic and every requested id costs one sweep of the row.  The softmax
// masses are summed in fp64 (a token at the top-p boundary is decided by mass, not by the order of an fp32 sum).  Duplicate ids are fine.
__global__ __launch_bounds__(256) void gather_scores_kernel(const float* logits, int ldl, int V, const int32_t* ids, int m, float temperature,
                                                            int top_k, float top_p, float* scores) {
  __shared__ float red[4];
  __shared__ double redd[4];
  const int row = blockIdx.x, tid = threadIdx.x;
  const float* z = logits + (size_t)row * ldl;
  float* out = scores + (size_t)row * m;
  if (temperature == 0.f) {
    if (tid < m) {
      const int id = ids[tid];
      out[tid] = (unsigned)id < (unsigned)V ? z[id] : NAN;
    }
    return;
  }
  auto block_sum_f64 = [&](double x) -> double {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    __syncthreads();
    if ((tid & 63) == 0) redd[tid >> 6] = x;
    __syncthreads();
    return redd[0] + redd[1] + redd[2] + redd[3];
  };
  float mx = -INFINITY;
  for (int i = tid; i < V; i += 256) mx = fmaxf(mx, z[i] / temperature);
  mx = block_max_256(mx, red);
  uint32_t thr = 0;   // top-k keeps tokens with key >= thr
  if (top_k > 0 && top_k < V) {
    for (int bit = 31; bit >= 0; --bit) {
      const uint32_t cand = thr | (1u << bit);
      float cnt = 0.f;
      for (int i = tid; i < V; i += 256) cnt += (fkey(z[i] / temperature) >= cand) ? 1.f : 0.f;
      cnt = block_sum_256(cnt, red);
      if (cnt >= (float)top_k) thr = cand;
    }
  }
  const bool use_p = top_p < 1.0f;
  double total = 0.0;
  if (use_p) {
    for (int i = tid; i < V; i += 256) {
      const float v = z[i] / temperature;
      if (fkey(v) >= thr) total += (double)expf(v - mx);
    }
    total = block_sum_f64(total);
  }
  for (int j = 0; j < m; ++j) {
    const int id = ids[j];
    if ((unsigned)id >= (unsigned)V) {
      if (tid == 0) out[j] = NAN;
      continue;
    }
    const float x = z[id] / temperature;
    bool keep = fkey(x) >= thr;
    if (keep && use_p && x < mx) {                    // the row maximum always stays (min_tokens_to_keep = 1)
      double below = 0.0;                             // kept mass at or below this token = its ascending cumulative mass
      for (int i = tid; i < V; i += 256) {
        const float v = z[i] / temperature;
        if (fkey(v) >= thr && v <= x) below += (double)expf(v - mx);
      }
      below = block_sum_f64(below);
      keep = below > (1.0 - (double)top_p) * total;
    }
    if (tid == 0) out[j] = keep ? x : -INFINITY;
  }
}

// ---- per-token log-prob and entropy of the sampled tokens (rollout output_logprobs; opadpo_token_logprobs) --------------------------------
// z = logits * inv_temp (one fp32 multiply, as head_fwd_kernel) over the row the sampler just read: bias added, EOS column -inf under suppress_eos.
//   logp = z[tok] - logsumexp(z),  ent = logsumexp(z) - sum softmax(z) * z      the distribution BEFORE the top-k / top-p cuts
// One workgroup of 1024 threads per row.  The row is read ONCE with 16-byte loads: a thread keeps TLP_R float4 (V <= 32768: the whole row,
// 32000 floats = 8 float4 per thread) in registers between the max pass and the sum pass; columns past TLP_R * 4096 (larger vocabularies)
// are read again by the sum pass.  Both sums run on d = z - max: logp = (z[tok] - max) - log(se), ent = log(se) - sum(e * d) / se, so a row
// shifted by a constant gives the same bits and nothing is subtracted at the magnitude of the logits.  A column with z = -inf has e = 0 and
// its e * d term is taken as 0 (0 * -inf would be NaN).  Reduction: per wave by shuffles, then 16 partials through LDS, added in wave order
// by every thread (deterministic).  tok == pad_id: logp = -0.0, ent = 0 without reading the row (head_fwd_kernel's pad rule, by value).
// step_ptr (nullable): the device step counter of the rollout; the outputs are [max_steps, rows] like `history`, slot step * rows + row;
// a step at or past max_steps writes nothing.  A token outside [0, V) that is not pad reads NaN.
// Per-row form (one TlpRows after the last argument; continuous rollout): row = slot (workgroup i reads row ids[i] when ids is given), the outputs are
// [rows, max_steps] like the per-row sampler's history and the slot is [row, step[row] - 1]: the per-row sampler has advanced the row's step past the
// token it wrote.  A pad token writes NOTHING here - the row's outputs were set to the pad values when the slot was admitted, and a finished row's
// step no longer names a slot of its own to write them to.
constexpr int TLP_T = 1024, TLP_W = TLP_T / 64, TLP_R = 8;
struct TlpRows { const int32_t* step; const int32_t* ids; };

template <typename... RA>
__global__ __launch_bounds__(TLP_T) void token_logprob_kernel(const float* logits, int ldl, int V, const int32_t* tokens, float inv_temp, int pad_id,
                                                              const int32_t* step_ptr, int max_steps, float* logp, float* ent, RA... ra) {
  constexpr bool ROWS = sizeof...(RA) > 0;
  __shared__ float wmax[TLP_W], wse[TLP_W], wsz[TLP_W];
  int row = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int step = step_ptr ? step_ptr[0] : 0;
  if constexpr (ROWS) {
    const TlpRows tr = (ra, ...);
    if (tr.ids) row = tr.ids[row];
    step = tr.step[row] - 1;
  }
  if (step < 0 || step >= max_steps) return;
  const size_t o = ROWS ? (size_t)row * max_steps + step : (size_t)step * gridDim.x + row;
  const int tok = tokens[row];
  if (tok == pad_id) {
    if (ROWS) return;
    if (tid == 0) {
      logp[o] = -0.0f;
      if (ent) ent[o] = 0.0f;
    }
    return;
  }
  const float* zrow = logits + (size_t)row * ldl;
  const float4* z4 = (const float4*)zrow;
  const int n4 = V >> 2;
  // z = logits * inv_temp.  Where the compiler fuses this multiply with the subtraction of the maximum (fp contraction), z - max carries the unrounded
  // product: at most half an ulp of z away from the value of the rounded product, and nearer to the exact one (measured: 4.8e-4 on rows shifted by 1e4)
  auto zmul = [&](float x) { return __fmul_rn(x, inv_temp); };
  float4 r[TLP_R];
  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < TLP_R; ++j) {
    const int gi = tid + j * TLP_T;
    float4 t = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    if (gi < n4) {
      t = z4[gi];
      t.x = zmul(t.x); t.y = zmul(t.y); t.z = zmul(t.z); t.w = zmul(t.w);
    }
    r[j] = t;
    mx = fmaxf(fmaxf(mx, fmaxf(t.x, t.y)), fmaxf(t.z, t.w));
  }
  for (int gi = tid + TLP_R * TLP_T; gi < n4; gi += TLP_T) {
    const float4 t = z4[gi];
    mx = fmaxf(fmaxf(mx, fmaxf(zmul(t.x), zmul(t.y))), fmaxf(zmul(t.z), zmul(t.w)));
  }
  mx = wave_max(mx);
  if (lane == 0) wmax[wave] = mx;
  __syncthreads();
  mx = wmax[0];
#pragma unroll
  for (int i = 1; i < TLP_W; ++i) mx = fmaxf(mx, wmax[i]);
  float se = 0.f, sz = 0.f;
  auto term = [&](float z) {
    const float d = z - mx, e = expf(d);
    se += e;
    sz += d == -INFINITY ? 0.f : e * d;
  };
#pragma unroll
  for (int j = 0; j < TLP_R; ++j) { term(r[j].x); term(r[j].y); term(r[j].z); term(r[j].w); }
  for (int gi = tid + TLP_R * TLP_T; gi < n4; gi += TLP_T) {
    const float4 t = z4[gi];
    term(zmul(t.x)); term(zmul(t.y)); term(zmul(t.z)); term(zmul(t.w));
  }
  se = wave_sum(se);
  sz = wave_sum(sz);
  if (lane == 0) { wse[wave] = se; wsz[wave] = sz; }
  __syncthreads();
  if (tid == 0) {
    se = 0.f; sz = 0.f;
#pragma unroll
    for (int i = 0; i < TLP_W; ++i) { se += wse[i]; sz += wsz[i]; }
    const float ls = logf(se);
    logp[o] = (unsigned)tok < (unsigned)V ? (zmul(zrow[tok]) - mx) - ls : NAN;
    if (ent) ent[o] = ls - sz / se;
  }
}

// ---- beam search (HF GenerationMixin._beam_search, do_sample=False, length_penalty=1, early_stopping=False) ------------------------------
// Candidates of an item are ranked by the accumulated score log_softmax(logits) + beam score, ties to the LOWER flat index beam * V + token.
// beam_topk: one workgroup per beam row.  The row goes to LDS once; max and log-sum-exp; a 4-level radix select on the monotone key of the
// logit finds the 2k-th largest one; the keys above it and the lowest-index ties make the row's 2k candidates (score order = logit order, the
// shift by -lse + beam score is monotone).  The union of the rows' 2k contains the item's top 2k.  Step 0 (device counter): only beam 0 of an
// item is live, the others start at -1e9 (as HF); row_div = k reads the item's one prefill row for all its beams.
constexpr int BEAM_T = 1024, BEAM_W = BEAM_T / 64;
constexpr float BEAM_NEG = -1.0e9f;

__device__ __forceinline__ float fkey_inv(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__global__ __launch_bounds__(BEAM_T) void beam_topk_kernel(const float* logits, int ldl, int row_div, int V, int k, const int32_t* step_ptr, int step_arg,
                                                           const float* run_score, const uint8_t* done, float* cand_val, int32_t* cand_tok) {
  extern __shared__ __attribute__((aligned(16))) float zr[];        // [V] logits of the row
  __shared__ uint64_t hist[256];
  __shared__ float wred[BEAM_W];
  __shared__ int wcnt[BEAM_W];
  __shared__ uint32_t s_digit;
  __shared__ uint64_t s_carry;
  __shared__ int s_n, s_ties;
  __shared__ int s_tok[32];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, K2 = 2 * k;
  if (done[row / k]) return;
  const int t = step_ptr ? step_ptr[0] : step_arg;
  const float bs = t == 0 ? (row % k == 0 ? 0.f : BEAM_NEG) : run_score[row];
  const float* z = logits + (size_t)(row / row_div) * ldl;
  float mx = -INFINITY;
  for (int i = tid; i < V; i += BEAM_T) { const float x = z[i]; zr[i] = x; mx = fmaxf(mx, x); }
  mx = wave_max(mx);
  if (lane == 0) wred[wave] = mx;
  __syncthreads();
  mx = wred[0];
#pragma unroll
  for (int i = 1; i < BEAM_W; ++i) mx = fmaxf(mx, wred[i]);
  float se = 0.f;
  for (int i = tid; i < V; i += BEAM_T) se += expf(zr[i] - mx);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) se += __shfl_xor(se, o, 64);
  __syncthreads();
  if (lane == 0) wred[wave] = se;
  __syncthreads();
  se = 0.f;
#pragma unroll
  for (int i = 0; i < BEAM_W; ++i) se += wred[i];
  const float ls = logf(se);
  // radix select: thr = key of the K2-th largest logit, above = number of keys strictly above it
  uint32_t prefix = 0, pmask = 0;
  uint64_t above = 0;
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    for (int base = 0; base < V; base += BEAM_T) {
      const int i = base + tid;
      const uint32_t kk = i < V ? fkey(zr[i]) : 0u;
      bool mine = i < V && (kk & pmask) == prefix;
      const uint32_t dg = (kk >> shift) & 255u;
#pragma unroll 1
      for (int it = 0; it < 3; ++it) {               // wave-aggregated counting for crowded bins
        const uint64_t act = __ballot(mine);
        if (!act) break;
        const int lead = __ffsll((long long)act) - 1;
        const uint32_t ldg = __shfl(dg, lead, 64);
        const uint64_t same = __ballot(mine && dg == ldg);
        if (lane == lead) atomicAdd((unsigned long long*)&hist[ldg], (unsigned long long)__popcll(same));
        if (dg == ldg) mine = false;
      }
      if (mine) atomicAdd((unsigned long long*)&hist[dg], 1ull);
    }
    __syncthreads();
    if (wave == 0) pick_digit<true>(hist, above, (uint64_t)K2, lane, &s_digit, &s_carry);
    __syncthreads();
    prefix |= s_digit << shift;
    pmask |= 255u << shift;
    above = s_carry;
    __syncthreads();
  }
  const uint32_t thr = prefix;
  const int need_ties = K2 - (int)above;           // the lowest-index keys equal to thr fill the rest
  if (tid == 0) { s_n = 0; s_ties = 0; }
  __syncthreads();
  for (int base = 0; base < V; base += BEAM_T) {
    const int i = base + tid;
    const uint32_t kk = i < V ? fkey(zr[i]) : 0u;
    const bool tie = i < V && kk == thr;
    const uint64_t tm = __ballot(tie);
    if (lane == 0) wcnt[wave] = __popcll(tm);
    __syncthreads();
    int before = s_ties;
    for (int w = 0; w < wave; ++w) before += wcnt[w];
    const int rank = before + __popcll(tm & ((1ull << lane) - 1ull));
    if ((i < V && kk > thr) || (tie && rank < need_ties)) {
      const int slot = atomicAdd(&s_n, 1);
      if (slot < K2) s_tok[slot] = i;
    }
    __syncthreads();
    if (tid == 0) { int tot = 0; for (int w = 0; w < BEAM_W; ++w) tot += wcnt[w]; s_ties += tot; }
    __syncthreads();
  }
  if (tid < K2) {
    const int tok = s_tok[tid];
    cand_val[(size_t)row * K2 + tid] = ((zr[tok] - mx) - ls) + bs;          // log_softmax as torch rounds it, plus the beam score
    cand_tok[(size_t)row * K2 + tid] = tok;
  }
}

// beam_update: one wave per item.  Merges the k * 2k row candidates into the item's sorted top 2k (64-bit keys: score, then the lower flat
// index), then applies HF's rules at step t (device counter):
//   a candidate is finished if its token is EOS or t is the last step; finished ones ranked among the first k enter the item's finished set
//   (best k by score / (t + 1), generated length with the EOS; ties keep the earlier entry);
//   the next running beams are the best k unfinished candidates (at the last step the rest, at score - 1e9, keep the rows defined);
//   the item is done when its finished set is full and best running score / (t + 1) <= its worst finished score (HF's early-stop
//   heuristic), or at the last step.  A done item is frozen: its beams keep their rows and emit pad.
// Outputs: cur_tok (the next embedding gather), backpointers bp [2][max_new][rows] (parent row | token), and the slot table rewritten into the
// other parity buffer: new[i][0..t-1) = old[parent_i][0..t-1), new[i][t-1] = parent_i (the parent appended slot t-1 in its own row).
// A finished entry is (score, step, parent row, token); no token sequence is copied.
__global__ __launch_bounds__(64) void beam_update_kernel(const float* cand_val, const int32_t* cand_tok, int k, int V, int rows, int max_new, int eos_id,
                                                         int pad_id, const int32_t* step_ptr, int step_arg, float* run_score, float* fin_score,
                                                         int32_t* fin_info, int32_t* fin_n, uint8_t* done, int32_t* cur_tok, int32_t* bp,
                                                         int32_t* table, long long tstride) {
  constexpr int E = 8;                              // 64 * 8 >= k * 2k for k <= 16
  __shared__ int s_par[16];
  __shared__ float s_fs[16], s_new[16];
  __shared__ int s_fi[3][16], s_nt[16], s_np[16], s_nf[16];
  const int item = blockIdx.x, lane = threadIdx.x, K2 = 2 * k, n = k * K2, r0 = item * k;
  const int t = step_ptr ? step_ptr[0] : step_arg;
  if (t >= max_new) return;
  int32_t* bp_par = bp + (size_t)t * rows;
  int32_t* bp_tok = bp + (size_t)max_new * rows + (size_t)t * rows;
  const int32_t* told = table + (size_t)(t & 1) * tstride;
  int32_t* tnew = table + (size_t)((t + 1) & 1) * tstride;
  const bool frozen = done[item] != 0;
  if (frozen) {
    if (lane < k) { cur_tok[r0 + lane] = pad_id; bp_par[r0 + lane] = r0 + lane; bp_tok[r0 + lane] = pad_id; s_par[lane] = r0 + lane; }
  } else {
    uint64_t key[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int c = lane + 64 * e;
      key[e] = 0;
      if (c < n) {
        const int r = c / K2;
        const float v = cand_val[(size_t)(r0 + r) * K2 + c % K2];
        const uint32_t flat = (uint32_t)r * (uint32_t)V + (uint32_t)cand_tok[(size_t)(r0 + r) * K2 + c % K2];
        key[e] = ((uint64_t)fkey(v) << 32) | (uint64_t)(0xffffffffu - flat);
      }
    }
    uint64_t mine = 0;                              // lane j < K2: the j-th best candidate
    for (int j = 0; j < K2; ++j) {
      uint64_t best = 0;
#pragma unroll
      for (int e = 0; e < E; ++e) best = key[e] > best ? key[e] : best;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const uint64_t other = (uint64_t)__shfl_xor((long long)best, o, 64);
        best = other > best ? other : best;
      }
#pragma unroll
      for (int e = 0; e < E; ++e) if (key[e] == best) key[e] = 0;
      if (lane == j) mine = best;
    }
    const bool valid = lane < K2;
    const float val = fkey_inv((uint32_t)(mine >> 32));
    const uint32_t flat = 0xffffffffu - (uint32_t)(mine & 0xffffffffu);
    const int par = r0 + (int)(flat / (uint32_t)V), tok = (int)(flat % (uint32_t)V);
    const bool fin = valid && ((eos_id >= 0 && tok == eos_id) || t == max_new - 1);
    const uint64_t lt = (1ull << lane) - 1ull;
    const uint64_t unf = __ballot(valid && !fin), fnd = __ballot(fin);
    const int n_unf = __popcll(unf);
    const int slot = fin ? n_unf + __popcll(fnd & lt) : __popcll(unf & lt);
    if (valid && slot < k) {
      const int i = r0 + slot;
      cur_tok[i] = tok; bp_par[i] = par; bp_tok[i] = tok; s_par[slot] = par;
      run_score[i] = fin ? val + BEAM_NEG : val;
    }
    if (lane < k) {                                 // the first k candidates: the ones that may enter the finished set
      s_new[lane] = val / (float)(t + 1);
      s_nf[lane] = fin; s_nt[lane] = tok; s_np[lane] = par;
    }
    const float run0 = __shfl(fin ? val + BEAM_NEG : val, __ffsll((long long)(n_unf ? unf : fnd)) - 1, 64);
    if (lane < k) {
      s_fs[lane] = fin_score[r0 + lane];
      s_fi[0][lane] = fin_info[r0 + lane]; s_fi[1][lane] = fin_info[rows + r0 + lane]; s_fi[2][lane] = fin_info[2 * rows + r0 + lane];
    }
    __syncthreads();
    if (lane == 0) {
      int cnt = fin_n[item];
      for (int j = 0; j < k; ++j) {
        if (!s_nf[j]) continue;
        const float sc = s_new[j];
        int p = 0;
        while (p < cnt && s_fs[p] >= sc) ++p;
        if (p >= k) continue;
        for (int q = min(cnt, k - 1); q > p; --q) { s_fs[q] = s_fs[q - 1]; s_fi[0][q] = s_fi[0][q - 1]; s_fi[1][q] = s_fi[1][q - 1]; s_fi[2][q] = s_fi[2][q - 1]; }
        s_fs[p] = sc; s_fi[0][p] = t; s_fi[1][p] = s_np[j]; s_fi[2][p] = s_nt[j];
        cnt = min(cnt + 1, k);
      }
      fin_n[item] = cnt;
      const bool full = cnt == k;
      if (t == max_new - 1 || (full && !(run0 / (float)(t + 1) > s_fs[k - 1]))) done[item] = 1;
    }
    __syncthreads();
    if (lane < k) {
      fin_score[r0 + lane] = s_fs[lane];
      fin_info[r0 + lane] = s_fi[0][lane]; fin_info[rows + r0 + lane] = s_fi[1][lane]; fin_info[2 * rows + r0 + lane] = s_fi[2][lane];
    }
  }
  __syncthreads();
  if (t >= 1) {
    for (int idx = lane; idx < k * t; idx += 64) {
      const int q = idx / t, s = idx - q * t, p = s_par[q];
      tnew[(size_t)(r0 + q) * max_new + s] = s == t - 1 ? p : told[(size_t)p * max_new + s];
    }
  }
}

// ---- continuous rollout: the per-slot state between two steps (opadpo_decode_cont_begin / _admit) -----------------------------------------------
// start of a step: a live slot moves to the position of the token it is about to append; a finished (or never used) slot stays where it is, so
// it re-appends the same key at the same slot of its own cache for as long as it idles.  The clamp is never reached by a live slot (its step is
// below its cap <= max_new, so its position is below Lp + max_new - 1); it is the bound an idle slot is held to whatever its state.
__global__ void decode_rows_advance_kernel(int32_t* pos, const uint8_t* finished, int slots, int max_ctx) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < slots && !finished[i]) pos[i] = min(pos[i] + 1, max_ctx - 1);
}
// admission: one workgroup per admitted slot.  Position Lp - 1 (the last prefill key), step 0, the prompt's cap and seed, not finished; the slot's
// history row becomes pad and its log-prob / entropy rows (nullable) the pad values -0.0 / 0.
__global__ __launch_bounds__(256) void decode_rows_admit_kernel(const int32_t* slot_ids, const uint64_t* seeds, const int32_t* caps, int Lp, int max_new,
                                                                int pad_id, int32_t* pos, int32_t* step, int32_t* cap, uint64_t* seed,
                                                                uint8_t* finished, int32_t* history, float* logp, float* ent) {
  const int j = blockIdx.x, s = slot_ids[j], tid = threadIdx.x;
  if (tid == 0) { pos[s] = Lp - 1; step[s] = 0; cap[s] = caps[j]; seed[s] = seeds[j]; finished[s] = 0; }
  for (int t = tid; t < max_new; t += 256) {
    history[(size_t)s * max_new + t] = pad_id;
    if (logp) logp[(size_t)s * max_new + t] = -0.0f;
    if (ent) ent[(size_t)s * max_new + t] = 0.0f;
  }
}

}  // namespace

hipError_t launch_decode_rows_advance(int32_t* pos, const uint8_t* finished, int slots, int max_ctx, hipStream_t st) {
  if (slots <= 0) return hipSuccess;
  hipLaunchKernelGGL(decode_rows_advance_kernel, dim3((slots + 255) / 256), dim3(256), 0, st, pos, finished, slots, max_ctx);
  return hipGetLastError();
}
// slot_ids / seeds / caps: device arrays [n]; the caller has checked every slot id against the session's slot count and every cap against max_new
hipError_t launch_decode_rows_admit(const int32_t* slot_ids, const uint64_t* seeds, const int32_t* caps, int n, int Lp, int max_new, int pad_id, int32_t* pos,
                                    int32_t* step, int32_t* cap, uint64_t* seed, uint8_t* finished, int32_t* history, float* logp, float* ent, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(decode_rows_admit_kernel, dim3(n), dim3(256), 0, st, slot_ids, seeds, caps, Lp, max_new, pad_id, pos, step, cap, seed, finished, history,
                     logp, ent);
  return hipGetLastError();
}

static int attn_decode_splits(int B, int nh, int max_ctx) {
  // 257..767 (sequence, head) pairs (9..23 sequences at 32 heads): two key ranges per pair, run as 4-wave workgroups (>= 512 of them) - measured
  // against one 16-wave workgroup per pair: decode step B = 12 4.47 -> 4.27 ms, B = 16 4.58 -> 4.40; from 768 pairs on 4-wave workgroups without a
  // split (B = 24: 5.34 -> 5.12); up to 256 pairs the 16-wave form stays (B = 8: 3.80 against 4.07 with a split)
  if (B * nh >= 768) {
    // 4-wave workgroups, 1024 of them resident on the chip: a partly filled last round costs a whole one (attention per layer 65.6 us at 32
    // sequences, 106 at 40, 127.6 at 64), so two key ranges per pair are used where they cut the rounds by a fifth or more - 33..48 sequences at 32
    // heads: decode step B = 36 6.62 -> 6.18 ms, B = 40 6.76 -> 6.34, B = 48 7.09 -> 6.79; B = 56 / 64 stay unsplit (7.38 / 7.70 against 7.56 / 7.98)
    const int pairs = B * nh, r1 = (pairs + 1023) / 1024, r2x2 = (2 * pairs + 1023) / 1024;
    return (r2x2 * 5 <= r1 * 8 && max_ctx >= 512) ? 2 : 1;
  }
  if (B * nh > 256) return std::min(2, std::max(1, max_ctx / 256));
  // up to 256 pairs: as many key ranges as keep the 16-wave workgroups within ONE round of the 256 CUs (rounded up, 5..7 sequences ran 320-448
  // workgroups in two rounds: attention 27.4 + 4.9 us merge per layer at B = 5 against 23.2 at B = 8; profiles/r04k_rollout_b*_kernel_stats.csv)
  int splits = std::max(1, 256 / (B * nh));
  splits = std::min(splits, std::max(1, max_ctx / 256));
  return std::max(1, std::min(splits, 16));
}
static bool attn_decode_fat(int B, int nh, int splits) { return B * nh * splits < 512; }      // 16-wave workgroups below 512 of them
size_t attn_decode_workspace_bytes(int B, int nh, int hd, int max_ctx) {
  const int splits = attn_decode_splits(B, nh, max_ctx);
  return splits == 1 ? 0 : (size_t)B * nh * splits * (hd + 2) * 4;
}

hipError_t launch_attn_decode_fused(const bf16_t* qkv, int ld, const float* cosb, const float* sinb, bf16_t* kc, bf16_t* vc, bf16_t* o,
                                    const uint8_t* key_mask, int B, int nh, int hd, const int32_t* pos_ptr, int max_ctx, float scale,
                                    void* workspace, size_t workspace_bytes, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  if ((hd != 64 && hd != 128) || !pos_ptr || ld % 8) return hipErrorInvalidValue;
  int splits = attn_decode_splits(B, nh, max_ctx);
  if (splits > 1 && (!workspace || workspace_bytes < attn_decode_workspace_bytes(B, nh, hd, max_ctx))) splits = 1;
  float* part = (float*)workspace;
  const float sl2 = scale * 1.4426950408889634f;
  const bool fat = attn_decode_fat(B, nh, splits);
  const dim3 gr(nh, B, splits);
#define ADF(HD_, NW_) hipLaunchKernelGGL((attn_decode_kernel<HD_, NW_, true>), gr, dim3(NW_ * 64), 0, st, qkv, ld, kc, vc, o, key_mask, nh, 0, pos_ptr, max_ctx, sl2, part, cosb, sinb, kc, vc)
  if (hd == 128) { if (fat) ADF(128, 16); else ADF(128, 4); }
  else           { if (fat) ADF(64, 16); else ADF(64, 4); }
#undef ADF
  if (splits > 1) hipLaunchKernelGGL(attn_decode_merge_kernel, dim3(B * nh), dim3(hd), 0, st, part, o, splits, hd);
  return hipGetLastError();
}

// the fused launch with a position per row (continuous rollout): the split rule, the workgroup shape and the merge of launch_attn_decode_fused
hipError_t launch_attn_decode_fused_rows(const bf16_t* qkv, int ld, const float* cosb, const float* sinb, bf16_t* kc, bf16_t* vc, bf16_t* o,
                                         const uint8_t* key_mask, int B, int nh, int hd, const int32_t* pos_rows, int max_ctx, float scale,
                                         void* workspace, size_t workspace_bytes, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  if ((hd != 64 && hd != 128) || !pos_rows || ld % 8 || max_ctx < 1) return hipErrorInvalidValue;
  int splits = attn_decode_splits(B, nh, max_ctx);
  if (splits > 1 && (!workspace || workspace_bytes < attn_decode_workspace_bytes(B, nh, hd, max_ctx))) splits = 1;
  float* part = (float*)workspace;
  const float sl2 = scale * 1.4426950408889634f;
  const bool fat = attn_decode_fat(B, nh, splits);
  const dim3 gr(nh, B, splits);
#define ADR(HD_, NW_) hipLaunchKernelGGL((attn_decode_kernel<HD_, NW_, true, RowsDec>), gr, dim3(NW_ * 64), 0, st, qkv, ld, kc, vc, o, key_mask, nh, 0, pos_rows, \
                                         max_ctx, sl2, part, cosb, sinb, kc, vc, RowsDec{})
  if (hd == 128) { if (fat) ADR(128, 16); else ADR(128, 4); }
  else           { if (fat) ADR(64, 16); else ADR(64, 4); }
#undef ADR
  if (splits > 1) hipLaunchKernelGGL(attn_decode_merge_kernel, dim3(B * nh), dim3(hd), 0, st, part, o, splits, hd);
  return hipGetLastError();
}

hipError_t launch_attn_decode_beam(const bf16_t* qkv, int ld, const float* cosb, const float* sinb, const bf16_t* kp, const bf16_t* vp, bf16_t* ks,
                                   bf16_t* vs, bf16_t* o, const uint8_t* prefix_mask, int items, int k, int nh, int hd, const int32_t* pos_ptr, int Lp,
                                   int max_new, const int32_t* table, long long table_stride, float scale, void* workspace, size_t workspace_bytes,
                                   hipStream_t st) {
  const int rows = items * k, max_ctx = Lp + max_new;
  if (rows <= 0) return hipSuccess;
  if ((hd != 64 && hd != 128) || !pos_ptr || !table || ld % 8 || k <= 0) return hipErrorInvalidValue;
  int splits = attn_decode_splits(rows, nh, max_ctx);
  if (splits > 1 && (!workspace || workspace_bytes < attn_decode_workspace_bytes(rows, nh, hd, max_ctx))) splits = 1;
  float* part = (float*)workspace;
  const float sl2 = scale * 1.4426950408889634f;
  const bool fat = attn_decode_fat(rows, nh, splits);
  const dim3 gr(nh, rows, splits);
  const BeamDec bm{table, table_stride, Lp, max_new, k};
#define ADB(HD_, NW_) hipLaunchKernelGGL((attn_decode_kernel<HD_, NW_, true, BeamDec>), gr, dim3(NW_ * 64), 0, st, qkv, ld, kp, vp, o, prefix_mask, nh, 0, pos_ptr, \
                                         max_ctx, sl2, part, cosb, sinb, ks, vs, bm)
  if (hd == 128) { if (fat) ADB(128, 16); else ADB(128, 4); }
  else           { if (fat) ADB(64, 16); else ADB(64, 4); }
#undef ADB
  if (splits > 1) hipLaunchKernelGGL(attn_decode_merge_kernel, dim3(rows * nh), dim3(hd), 0, st, part, o, splits, hd);
  return hipGetLastError();
}

// ---- n sampled responses per prompt: row b = sample b % n of item b / n; prefix caches per item, suffix caches per row ------------------------
// prefix key ranges of the grouped form: items * nh * ranges fills about ONE round of the 256 CUs; the stride from one range to the next is a
// multiple of 64 keys (one tile per wave step, at least 64), the last range holds the remainder (1 .. stride keys), and no range is empty
static int attn_decode_shared_ranges(int items, int nh, int Lp, int* per_out) {
  int R = std::max(1, 256 / std::max(1, items * nh));
  R = std::min(R, std::max(1, Lp / 64));
  const int per = ((Lp + R - 1) / R + 63) / 64 * 64;
  if (per_out) *per_out = per;
  return (Lp + per - 1) / per;
}
// the library's choice (form 0): the grouped form for n >= 2 at head_dim 128.  Measured at 7B, Lp = 703 (profiles/shared_prefix_bench_7b.json):
// 5.04 against 6.68 ms per decode step at 8 x 8 rows, 7.09 against 8.50 with 896 new tokens, 9.48 against 17.98 at 16 x 16 rows - the grouped form
// wins at every measured shape; n = 2..7 and other head counts are not measured and follow the byte count (the prefix moves once per item).
static bool attn_decode_shared_grouped(int n, int hd, int form) { return form == 2 || (form == 0 && n >= 2 && hd == 128); }
size_t attn_decode_shared_workspace_bytes(int items, int n, int nh, int hd, int Lp, int max_new) {
  if (items <= 0 || n <= 0) return 0;
  size_t bytes = attn_decode_workspace_bytes(items * n, nh, hd, Lp + max_new);          // per-row form: the fused kernel's key ranges
  if (hd == 128) {
    const int R = attn_decode_shared_ranges(items, nh, Lp, nullptr);
    bytes = std::max(bytes, (size_t)items * n * nh * (R + 1) * (hd + 2) * 4);           // grouped form: R prefix slots + the suffix slot
  }
  return bytes;
}

hipError_t launch_attn_decode_shared(const bf16_t* qkv, int ld, const float* cosb, const float* sinb, const bf16_t* kp, const bf16_t* vp, bf16_t* ks,
                                     bf16_t* vs, bf16_t* o, const uint8_t* prefix_mask, int items, int n, int nh, int hd, const int32_t* pos_ptr, int Lp,
                                     int max_new, float scale, void* workspace, size_t workspace_bytes, int form, hipStream_t st) {
  const int rows = items * n, max_ctx = Lp + max_new;
  if (rows <= 0) return hipSuccess;
  if ((hd != 64 && hd != 128) || !pos_ptr || ld % 8 || n <= 0 || n > OPADPO_MAX_RETURN_SEQUENCES || form < 0 || form > 2) return hipErrorInvalidValue;
  float* part = (float*)workspace;
  const float sl2 = scale * 1.4426950408889634f;
#define ADS(HD_, NW_, GRID_, SD_) hipLaunchKernelGGL((attn_decode_kernel<HD_, NW_, true, SharedDec>), GRID_, dim3(NW_ * 64), 0, st, qkv, ld, kp, vp, o, prefix_mask, nh, 0, \
                                                     pos_ptr, max_ctx, sl2, part, cosb, sinb, ks, vs, SD_)
  if (!attn_decode_shared_grouped(n, hd, form)) {
    // per-row form: the beam kernel with the identity slot table - the split rule and the key order of the fused kernel on a materialised cache
    int splits = attn_decode_splits(rows, nh, max_ctx);
    if (splits > 1 && (!workspace || workspace_bytes < attn_decode_workspace_bytes(rows, nh, hd, max_ctx))) splits = 1;
    const bool fat = attn_decode_fat(rows, nh, splits);
    const dim3 gr(nh, rows, splits);
    const SharedDec sd{{nullptr, 0, Lp, max_new, n}, 0, 0, 0};
    if (hd == 128) { if (fat) ADS(128, 16, gr, sd); else ADS(128, 4, gr, sd); }
    else           { if (fat) ADS(64, 16, gr, sd); else ADS(64, 4, gr, sd); }
    if (splits > 1) hipLaunchKernelGGL(attn_decode_merge_kernel, dim3(rows * nh), dim3(hd), 0, st, part, o, splits, hd);
    return hipGetLastError();
  }
  if (hd != 128) return hipErrorInvalidValue;
  int per = 0;
  const int R = attn_decode_shared_ranges(items, nh, Lp, &per), slots = R + 1;
  if (!workspace || workspace_bytes < (size_t)rows * nh * slots * (hd + 2) * 4) return hipErrorInvalidValue;
  // 1. the suffix keys [Lp, pos] of every row, the new token rotated and appended (the per-row kernel, one key range) -> slot R
  {
    const dim3 gr(nh, rows, 1);
    const SharedDec sd{{nullptr, 0, Lp, max_new, n}, Lp, slots, R};
    if (attn_decode_fat(rows, nh, 1)) ADS(128, 16, gr, sd); else ADS(128, 4, gr, sd);
  }
#undef ADS
  // 2. the items' prefix keys, each tile once for the item's n rows -> slots 0 .. R-1;  3. the merge
  hipLaunchKernelGGL(attn_decode_group_kernel, dim3(nh, items, R), dim3(GRP_W * 64), 0, st, qkv, ld, cosb, sinb, kp, vp, prefix_mask, n, nh, pos_ptr, Lp, per,
                     slots, sl2, part);
  hipLaunchKernelGGL(attn_decode_merge_kernel, dim3(rows * nh), dim3(hd), 0, st, part, o, slots, hd);
  return hipGetLastError();
}

hipError_t launch_beam_step(const float* logits, int ldl, int row_div, int items, int k, int V, int max_new, int eos_id, int pad_id,
                            const int32_t* step_ptr, int step, BeamState s, hipStream_t st) {
  if (items <= 0) return hipSuccess;
  if (k <= 0 || k > OPADPO_MAX_BEAMS || 2 * k > V || V > SAMP_MAXV || items * k > 64) return hipErrorInvalidValue;
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)beam_topk_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, SAMP_MAXV * 4);
    attr_set = true;
  }
  const int rows = items * k;
  hipLaunchKernelGGL(beam_topk_kernel, dim3(rows), dim3(BEAM_T), (size_t)V * 4, st, logits, ldl, row_div, V, k, step_ptr, step, s.run_score, s.done,
                     s.cand_val, s.cand_tok);
  hipLaunchKernelGGL(beam_update_kernel, dim3(items), dim3(64), 0, st, s.cand_val, s.cand_tok, k, V, rows, max_new, eos_id, pad_id, step_ptr, step,
                     s.run_score, s.fin_score, s.fin_info, s.fin_n, s.done, s.cur_tok, s.bp, s.table, s.table_stride);
  return hipGetLastError();
}

hipError_t launch_attn_decode(const bf16_t* q, const bf16_t* kc, const bf16_t* vc, bf16_t* o, const uint8_t* key_mask,
                              int B, int nh, int hd, int ctx, const int32_t* ctx_ptr, int max_ctx, int ldq, float scale,
                              void* workspace, size_t workspace_bytes, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  if (hd != 64 && hd != 128) return hipErrorInvalidValue;
  int splits = attn_decode_splits(B, nh, max_ctx);
  if (splits > 1 && (!workspace || workspace_bytes < attn_decode_workspace_bytes(B, nh, hd, max_ctx))) splits = 1;
  float* part = (float*)workspace;
  const float sl2 = scale * 1.4426950408889634f;
  const bool fat = attn_decode_fat(B, nh, splits);       // few blocks: 16 waves each
  const dim3 gr(nh, B, splits);
#define AD(HD_, NW_) hipLaunchKernelGGL((attn_decode_kernel<HD_, NW_>), gr, dim3(NW_ * 64), 0, st, q, ldq, kc, vc, o, key_mask, nh, ctx, ctx_ptr, max_ctx, sl2, part)
  if (hd == 128) { if (fat) AD(128, 16); else AD(128, 4); }
  else           { if (fat) AD(64, 16); else AD(64, 4); }
#undef AD
  if (splits > 1) hipLaunchKernelGGL(attn_decode_merge_kernel, dim3(B * nh), dim3(hd), 0, st, part, o, splits, hd);
  return hipGetLastError();
}

hipError_t launch_rope_kv_append(bf16_t* qkv, int ld, const float* cosb, const float* sinb, bf16_t* kc, bf16_t* vc, int B, int nh,
                                 int hd, const int32_t* pos_ptr, int max_ctx, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  if (hd % 16 || ld % 8 || !pos_ptr) return hipErrorInvalidValue;
  const int total = B * nh * (hd / 16);
  hipLaunchKernelGGL(rope_kv_append_kernel, dim3((total + 255) / 256), dim3(256), 0, st, qkv, ld, cosb, sinb, kc, vc, B, nh, hd, pos_ptr, max_ctx);
  return hipGetLastError();
}

hipError_t launch_sample(const float* logits, int ldl, int rows, int V, float temperature, int top_k, float top_p,
                         uint64_t seed, uint64_t step, const int32_t* step_ptr, uint8_t* finished, int pad_id, int eos_id,
                         int32_t* out, int32_t* history, hipStream_t st) {
  if (rows <= 0) return hipSuccess;
  const bool fast = V % 4 == 0 && ldl % 4 == 0 && V <= SAMP_MAXV && ((uintptr_t)logits & 15) == 0;
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)sample_kernel_fast<>, hipFuncAttributeMaxDynamicSharedMemorySize, SAMP_MAXV * 4);
    attr_set = true;
  }
  // compact (default): one-wave tail on the kept tokens after the top-k threshold; process flag bit 9: the full vocabulary sweeps (identical
  // draws; the exactness test's yardstick).  A process flag: the same for eager and captured launches
  const int compact = process_flags().sample_compact ? 1 : 0;
  if (fast)
    hipLaunchKernelGGL(sample_kernel_fast<>, dim3(rows), dim3(SAMP_T), (size_t)V * 4, st, logits, ldl, V, 1.0f / temperature, top_k, top_p, seed,
                       step, step_ptr, finished, pad_id, eos_id, out, history, compact);
  else
    hipLaunchKernelGGL(sample_kernel_generic<>, dim3(rows), dim3(256), 0, st, logits, ldl, V, 1.0f / temperature, top_k, top_p, seed,
                       step, step_ptr, finished, pad_id, eos_id, out, history);
  return hipGetLastError();
}

// the per-row form (SampRows): the same choice between the two kernels, the same compact flag.  n_ids > 0: only the rows ids[0 .. n_ids) (device
// array, every entry in [0, rows): the caller's check) are sampled.  hipErrorInvalidValue, nothing launched: a null seed / step / cap / finished /
// out array, max_steps < 1, temperature <= 0.
hipError_t launch_sample_rows(const float* logits, int ldl, int rows, int V, float temperature, int top_k, float top_p, const uint64_t* seed_rows,
                              int32_t* step_rows, const int32_t* cap_rows, int max_steps, const int32_t* ids, int n_ids, uint8_t* finished, int pad_id,
                              int eos_id, int32_t* out, int32_t* history, hipStream_t st) {
  if (rows <= 0) return hipSuccess;
  if (!logits || !seed_rows || !step_rows || !cap_rows || !finished || !out || max_steps < 1 || !(temperature > 0.f) || n_ids < 0 || n_ids > rows)
    return hipErrorInvalidValue;
  const bool fast = V % 4 == 0 && ldl % 4 == 0 && V <= SAMP_MAXV && ((uintptr_t)logits & 15) == 0;
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)sample_kernel_fast<SampRows>, hipFuncAttributeMaxDynamicSharedMemorySize, SAMP_MAXV * 4);
    attr_set = true;
  }
  const int compact = process_flags().sample_compact ? 1 : 0;
  const SampRows sr{seed_rows, step_rows, cap_rows, n_ids > 0 ? ids : nullptr, max_steps};
  const int blocks = n_ids > 0 ? n_ids : rows;
  if (fast)
    hipLaunchKernelGGL(sample_kernel_fast<SampRows>, dim3(blocks), dim3(SAMP_T), (size_t)V * 4, st, logits, ldl, V, 1.0f / temperature, top_k, top_p,
                       (uint64_t)0, (uint64_t)0, nullptr, finished, pad_id, eos_id, out, history, compact, sr);
  else
    hipLaunchKernelGGL(sample_kernel_generic<SampRows>, dim3(blocks), dim3(256), 0, st, logits, ldl, V, 1.0f / temperature, top_k, top_p, (uint64_t)0,
                       (uint64_t)0, nullptr, finished, pad_id, eos_id, out, history, sr);
  return hipGetLastError();
}

// Both wrappers check on the host what the kernels index with: rows <= 64, n / m <= OPADPO_MAX_LOGIT_IDS, every id of ids_host (the host copy
// of the device array ids) inside [0, V), no id twice in a bias table (two threads would add to one address).  Nothing is launched on a refusal.
static bool logit_ids_ok(const int32_t* ids_host, int n, int V, bool distinct) {
  for (int i = 0; i < n; ++i) {
    if (ids_host[i] < 0 || ids_host[i] >= V) return false;
    if (distinct)
      for (int j = 0; j < i; ++j)
        if (ids_host[j] == ids_host[i]) return false;
  }
  return true;
}

hipError_t launch_logit_bias_add(float* logits, int ldl, int rows, int V, const int32_t* ids, const float* bias, const int32_t* ids_host, int n,
                                 hipStream_t st) {
  if (n < 0 || n > OPADPO_MAX_LOGIT_IDS || rows < 0 || rows > 64 || V <= 0 || ldl < V) return hipErrorInvalidValue;
  if (n == 0 || rows == 0) return hipSuccess;
  if (!logits || !ids || !bias || !ids_host || !logit_ids_ok(ids_host, n, V, true)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(logit_bias_add_kernel, dim3((rows * n + 255) / 256), dim3(256), 0, st, logits, ldl, rows, V, ids, bias, n);
  return hipGetLastError();
}

// temperature 0 = greedy: the row is read with inv_temp = 1 (as the step-0 scores).  hipErrorInvalidValue, nothing launched: rows < 1, V or ldl not a
// multiple of 4 (the 16-byte loads), ldl < V, a logits base that is not 16-byte aligned, temperature < 0 or NaN, max_steps < 1, a null logits /
// tokens / logp (ent is nullable).
hipError_t launch_token_logprobs(const float* logits, int ldl, int rows, int V, const int32_t* tokens, float temperature, int pad_id,
                                 const int32_t* step_ptr, int max_steps, float* logp, float* ent, hipStream_t st) {
  if (rows < 1 || V <= 0 || V % 4 || ldl % 4 || ldl < V || !(temperature >= 0.f) || max_steps < 1) return hipErrorInvalidValue;
  if (!logits || !tokens || !logp || ((uintptr_t)logits & 15)) return hipErrorInvalidValue;
  const float inv_temp = temperature == 0.f ? 1.0f : 1.0f / temperature;
  hipLaunchKernelGGL(token_logprob_kernel<>, dim3(rows), dim3(TLP_T), 0, st, logits, ldl, V, tokens, inv_temp, pad_id, step_ptr, max_steps, logp, ent);
  return hipGetLastError();
}

// the per-row form (TlpRows), launched right after launch_sample_rows with the same ids: logp / ent [rows, max_steps]; same refusals
hipError_t launch_token_logprobs_rows(const float* logits, int ldl, int rows, int V, const int32_t* tokens, float temperature, int pad_id,
                                      const int32_t* step_rows, int max_steps, const int32_t* ids, int n_ids, float* logp, float* ent, hipStream_t st) {
  if (rows < 1 || V <= 0 || V % 4 || ldl % 4 || ldl < V || !(temperature >= 0.f) || max_steps < 1 || n_ids < 0 || n_ids > rows) return hipErrorInvalidValue;
  if (!logits || !tokens || !logp || !step_rows || ((uintptr_t)logits & 15)) return hipErrorInvalidValue;
  const float inv_temp = temperature == 0.f ? 1.0f : 1.0f / temperature;
  const TlpRows tr{step_rows, n_ids > 0 ? ids : nullptr};
  hipLaunchKernelGGL(token_logprob_kernel<TlpRows>, dim3(n_ids > 0 ? n_ids : rows), dim3(TLP_T), 0, st, logits, ldl, V, tokens, inv_temp, pad_id, nullptr,
                     max_steps, logp, ent, tr);
  return hipGetLastError();
}

hipError_t launch_gather_scores(const float* logits, int ldl, int rows, int V, const int32_t* ids, const int32_t* ids_host, int m, float temperature,
                                int top_k, float top_p, float* scores, hipStream_t st) {
  if (m < 0 || m > OPADPO_MAX_LOGIT_IDS || rows < 0 || rows > 64 || V <= 0 || ldl < V || !(temperature >= 0.f)) return hipErrorInvalidValue;
  if (m == 0 || rows == 0) return hipSuccess;
  if (!logits || !ids || !scores || !ids_host || !logit_ids_ok(ids_host, m, V, false)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gather_scores_kernel, dim3(rows), dim3(256), 0, st, logits, ldl, V, ids, m, temperature, top_k, top_p, scores);
  return hipGetLastError();
}
