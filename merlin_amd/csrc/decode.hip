// KV-cache decode step of the Llama decoder (gfx950): the S_q = 1 path behind `generate()`
// (reference: llama_mmgpt.py:114-134 prepare_inputs_for_generation; HF LlamaAttention with past_key_values,
// modeling_llama.py:243-281; eval_mmvet.py:101-120 is the caller).  Every kernel here is HBM-bound - one new token
// per sequence streams all weights (13.5 GB for Llama-7B) and the whole K/V cache once - so none of it is shaped
// into an MFMA GEMM: the rules that matter are 16-byte coalesced loads, enough waves in flight and no re-reads.
//
//   mh_gemv             y[m, n] = sum_k x[m, k] W[n, k] (+ resid[m, n]),  m <= 8 rows: ONE WAVE PER WEIGHT ROW, the
//                       row is read once as 64 lanes x 16 B per step and dotted against all m activations rows
//                       (which stay in L1/L2: m * K * 2 B <= 176 KB); fp32 accumulate, shuffle reduction.  6-16 rows: an MFMA form.
//   mh_gemv_qkv_rope    the q|k|v projection with its neighbours in the same launch: input_layernorm of the row (every block normalises
//                       it into LDS), rotate-half RoPE of q, k at the token's position, append of k, v to the cache - a wave owns the
//                       rotary pair (c, c + D/2) of one head, so lane 0 ends up with both partners.
//   mh_gemv_norm / mh_gemv_swiglu   post_attention_layernorm + gate|up projection + SwiGLU in one launch (a wave owns a gate row and
//                       its up row); fp8-weight forms of all of these (mh_gemv_fp8w*).
//   mh_decode_rope_append  (stand-alone form) rotate q, k of the new token at its own position and append k, v to the cache rows [b, pos[b]].
//   mh_attn_decode      block per (b, h, key split): pass 1 D/8 lanes per key (coalesced 256-B key rows, shuffle-reduced
//                       dot products, 4 rows in flight per thread) -> scores in LDS -> block max / sum; pass 2 lane-per-channel
//                       accumulation of p.V (coalesced value rows); split-KV partials merged by a second kernel.  Keys [0, len[b]).
//   mh_kv8_fill / mh_decode_rope_append_kv8 / mh_attn_decode_kv8   the same step on an fp8 KV cache (e4m3 bytes + one power-of-two scale
//                       per (sequence, head, token)): prefill quantiser, RoPE + quantised append, attention reading half the bytes per key.
//   mh_quant_fp4_b32 / mh_gemv_fp4w / mh_gemv_fp4w_norm / mh_gemv_fp4w_qkv_rope   the projections on MXFP4 weights (e2m1 values, two per byte, one
//                       power-of-two scale byte per 32 k: 0.53 bytes per weight, 3.6 GB per token at 7B) - at the end of this file.
//   mh_beam_ancestry / mh_attn_decode_beams (+ _kv8)   beam search on a shared prompt cache: the prompt's keys once per prompt for all its
//                       beams (the multi-query kernel, beams as queries), per-beam rows only for the generated tokens, found through an
//                       ancestry table that the re-ordering of beams rewrites instead of moving any K/V.
//   mh_decode_rope_append_multi / mh_attn_decode_multi (+ _kv8) / mh_ngram_draft   T <= 16 new tokens of one sequence in one step (the verify
//                       step of prompt-lookup decoding): append at T consecutive positions, attention with every key / value row loaded once
//                       for all T queries (scores on the matrix pipe, causality inside the block), and the device-side drafter.
//   mh_attn_extend (+ _kv8)   any number of new query rows of a sequence over a kept cache (generate(session=...), engine.extend): flash-style,
//                       64-query tiles, 32-key tiles with an online softmax, scores and P.V on the matrix pipe; no limit on Smax.
//   mh_attn_extend_branches (+ _kv8)   the packed rows of several continuations of one prompt (model.score, engine.extend_branches): the
//                       kernel of mh_attn_extend with a two-part horizon - the prompt's keys and the query's own continuation's.
// A decode step of a layer is 6 launches; each costs ~4 us of fixed time on top of its streaming, which is why the neighbours are folded in.
#include <climits>
#include <type_traits>

#include "mh_common.h"

// Weights and KV-cache rows are read ONCE per decode step by ONE CU: non-temporal loads (MI355X_MICROARCH.md "nt-weights": issued -> landed
// -18 %, a decode layer 5-10 % faster) keep them from displacing the small activation vectors every block re-reads.  A/B: -DMH_DECODE_NT=0.
#ifndef MH_DECODE_NT
#define MH_DECODE_NT 1
#endif
typedef unsigned int du32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 ld_stream16(const void* p) {
#if MH_DECODE_NT
  const du32x4 v = __builtin_nontemporal_load((const du32x4*)p);
  return make_uint4(v[0], v[1], v[2], v[3]);
#else
  return *(const uint4*)p;
#endif
}

typedef unsigned int du32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint2 ld_stream8(const void* p) {  // a lane's 8 e4m3 values of an fp8 cache row
#if MH_DECODE_NT
  const du32x2 v = __builtin_nontemporal_load((const du32x2*)p);
  return make_uint2(v[0], v[1]);
#else
  return *(const uint2*)p;
#endif
}

namespace {

// packed dot product of two 16-bit pairs with fp32 accumulate (v_dot2c_f32_bf16 / v_dot2c_f32_f16): no unpacking, half
// the VALU instructions of an fma per element - at 8 activation rows the unpack+fma form is VALU-bound, not HBM-bound
typedef __bf16 mh_bf2 __attribute__((ext_vector_type(2)));
typedef _Float16 mh_h2 __attribute__((ext_vector_type(2)));
template <int DT>
__device__ __forceinline__ float dot2_acc(uint32_t a, uint32_t b, float c) {
  if constexpr (DT == MH_BF16) return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(mh_bf2, a), __builtin_bit_cast(mh_bf2, b), c, false);
  else return __builtin_amdgcn_fdot2(__builtin_bit_cast(mh_h2, a), __builtin_bit_cast(mh_h2, b), c, false);
}

// Fused decode_rope_append of the q|k|v projection (tab == nullptr: off).  A wave then owns the ROTARY PAIR (c, c + D/2) of one head of
// one section (q, k or v) instead of two consecutive rows, so lane 0 ends up with both partners of every activation row and can rotate
// them at pos[m] (rotate-half, as rope_append_k on the stored 16-bit values) and write k / v straight into the cache rows [m, pos[m]].
struct RopeAppend {
  const float2* tab;   // [max_pos, D/2] (cos, sin)
  const int32_t* pos;  // [M] cache row the new k, v are appended at
  const int32_t* rpos; // [M] rotary position of the new token (== pos unless the prompt had padding in front of / inside it)
  uint16_t *kc, *vc;   // [M, Smax, H*D]
  int H, D, Smax;
};
template <int DT, int MM>
__device__ __forceinline__ void rope_append_store(const RopeAppend& ra, int pidx, const float (&a0)[MM], const float (&a1)[MM], uint16_t* out, int64_t ldo) {
  const int half = ra.D >> 1, per_sec = ra.H * half;
  const int sec = pidx / per_sec, rem = pidx - sec * per_sec, h = rem / half, c = rem - h * half;
  const int64_t HD = (int64_t)ra.H * ra.D, col = (int64_t)h * ra.D + c;
#pragma unroll
  for (int m = 0; m < MM; ++m) {
    float lo = ld16<DT>((uint16_t)st16<DT>(a0[m])), hi = ld16<DT>((uint16_t)st16<DT>(a1[m]));  // the projection as it would be stored
    const int p = ra.pos[m];
    if (sec < 2) {
      const float2 cs = ra.tab[(int64_t)ra.rpos[m] * half + c];
      rope_rot(lo, hi, cs.x, cs.y, lo, hi);
    }
    const uint16_t l16 = (uint16_t)st16<DT>(lo), h16 = (uint16_t)st16<DT>(hi);
    out[(int64_t)m * ldo + sec * HD + col] = l16;
    out[(int64_t)m * ldo + sec * HD + col + half] = h16;
    if (sec > 0) {
      uint16_t* dst = (sec == 1 ? ra.kc : ra.vc) + ((int64_t)m * ra.Smax + p) * HD + col;
      dst[0] = l16;
      dst[half] = h16;
    }
  }
}

// RMSNorm of MM rows (<= 8192 wide) into LDS xs[MM][K] by one 256-thread block: the chunk assignment, summation order and rounding of
// rmsnorm_fwd_row_k (norm.hip), so a projection fed from here equals rmsnorm + projection bit for bit.
template <int DT, int MM>
__device__ __forceinline__ void stage_rmsnorm(const uint16_t* __restrict__ x, int64_t ldx, const uint16_t* __restrict__ norm_w, float eps, int K,
                                              uint16_t* xs, float (*red)[4]) {
  const int tid = threadIdx.x, lane = tid & 63, nch = K >> 3;  // nch <= 1024 (launcher)
  uint4 xv[MM][4];
  float ssq[MM];
#pragma unroll
  for (int m = 0; m < MM; ++m) {
    ssq[m] = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = tid + i * 256;
      xv[m][i] = c < nch ? *(const uint4*)(x + (int64_t)m * ldx + c * 8) : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float f[8];
      unpack8<DT>(xv[m][i], f);
#pragma unroll
      for (int e = 0; e < 8; ++e) ssq[m] += f[e] * f[e];
    }
    ssq[m] = wave_sum(ssq[m]);
    if (lane == 0) red[m][tid >> 6] = ssq[m];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = tid + i * 256;
    if (c < nch) {
      float g[8];
      unpack8<DT>(*(const uint4*)(norm_w + c * 8), g);
#pragma unroll
      for (int m = 0; m < MM; ++m) {
        const float r = rsqrtf(((red[m][0] + red[m][1]) + (red[m][2] + red[m][3])) / (float)K + eps);
        float f[8];
        unpack8<DT>(xv[m][i], f);
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = f[e] * r * g[e];
        *(uint4*)(xs + m * K + c * 8) = pack8<DT>(f);
      }
    }
  }
  __syncthreads();
}

// ---- fp8 (OCP e4m3) weights with one fp32 scale per 128 consecutive k (BASELINE cfg 5's weight format), bf16/f16
// activations: the decode step is weight-bandwidth-bound, so halving the weight bytes is worth ~2x on the GEMVs.
// quant: q[n, k] = fp8(w[n, k] / s[n, k/128]),  s = max|w| over the block / 448 (1 if the block is all zero).
template <int DT>
__global__ __launch_bounds__(256) void quant_fp8_b128_k(const uint16_t* __restrict__ w, int64_t ldw, uint8_t* __restrict__ q,
                                                        float* __restrict__ sc, int N, int K) {
  const int nb = (K + 127) / 128;
  const int64_t blk = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);  // 16 lanes per 128-element block
  if (blk >= (int64_t)N * nb) return;
  const int n = (int)(blk / nb), kb = (int)(blk % nb);
  const int k0 = kb * 128 + (threadIdx.x & 15) * 8;
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = 0.f;
  if (k0 < K) unpack8<DT>(*(const uint4*)(w + (int64_t)n * ldw + k0), v);
  float mx = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) mx = fmaxf(mx, fabsf(v[e]));
#pragma unroll
  for (int o2 = 8; o2 > 0; o2 >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o2, 64));
  const float s = mx > 0.f ? mx * (1.0f / 448.0f) : 1.0f;
  const float inv = 1.0f / s;
  if ((threadIdx.x & 15) == 0) sc[(int64_t)n * nb + kb] = s;
  if (k0 < K) {
    int p0 = __builtin_amdgcn_cvt_pk_fp8_f32(v[0] * inv, v[1] * inv, 0, false);
    p0 = __builtin_amdgcn_cvt_pk_fp8_f32(v[2] * inv, v[3] * inv, p0, true);
    int p1 = __builtin_amdgcn_cvt_pk_fp8_f32(v[4] * inv, v[5] * inv, 0, false);
    p1 = __builtin_amdgcn_cvt_pk_fp8_f32(v[6] * inv, v[7] * inv, p1, true);
    *(uint2*)(q + (int64_t)n * K + k0) = make_uint2((unsigned)p0, (unsigned)p1);
  }
}

// two e4m3 values (the low or the high half of a dword) -> one packed 16-bit pair, in ONE instruction (gfx950 v_cvt_scalef32_pk_*_fp8 with
// scale 1: e4m3 values are exact in bf16 and fp16); a dword of 4 fp8 -> 2 packed words
template <int DT>
__device__ __forceinline__ void fp8x4_to_pk16(uint32_t p, uint32_t& lo, uint32_t& hi) {
  if constexpr (DT == MH_BF16) {
    lo = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(p, 1.0f, false));
    hi = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(p, 1.0f, true));
  } else {
    lo = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(p, 1.0f, false));
    hi = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(p, 1.0f, true));
  }
}
__device__ __forceinline__ void fp8x4_to_f32(uint32_t p, float* f) {
  typedef float f2_ __attribute__((ext_vector_type(2)));
  const f2_ lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)p, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)p, true);
  f[0] = lo[0]; f[1] = lo[1]; f[2] = hi[0]; f[3] = hi[1];
}
// eight e2m1 values (a dword of an MXFP4 row, the format at the end of this file) -> four packed 16-bit pairs, one instruction per pair
// (gfx950 v_cvt_scalef32_pk_*_fp4 with scale 1: the third operand selects the byte, whose low nibble becomes the low half of the pair -
// the stored order, so no swap); exact in both types
template <int DT>
__device__ __forceinline__ void fp4x8_to_pk16(uint32_t p, uint32_t* w) {
  if constexpr (DT == MH_BF16) {
    w[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(p, 1.0f, 0));
    w[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(p, 1.0f, 1));
    w[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(p, 1.0f, 2));
    w[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(p, 1.0f, 3));
  } else {
    w[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(p, 1.0f, 0));
    w[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(p, 1.0f, 1));
    w[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(p, 1.0f, 2));
    w[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(p, 1.0f, 3));
  }
}
__device__ __forceinline__ float e8m0_to_f32(uint32_t byte) { return __uint_as_float(byte << 23); }  // byte in [1, 254]; 0 (a masked block) -> 0.0

// ---- fp8 KV cache: K / V rows stored as e4m3 bytes [B, Smax, H*D] with one POWER-OF-TWO fp32 scale per (sequence, head, token), scales
// [B, H, Smax] (head-major: one (b, h) block of the attention kernel reads its scales contiguously).  scale = 2^e, e the smallest integer
// with amax * 2^-e <= 448 over the D channels of the group (amax = m * 2^ex, m in [0.5, 1): e = ex - 9 if m <= 0.875 else ex - 8), clamped
// to >= -126, 0 for an all-zero group; byte = e4m3_rne(x * 2^-e).  byte * 2^e is exact in bf16 (and in fp16 while in range), so the fp8
// cache is the 16-bit path on K / V rounded to that grid.
__device__ __forceinline__ int kv8_exp(float amax) {  // amax >= 0, finite
  const uint32_t bits = __float_as_uint(amax);
  const int ef = (int)(bits >> 23);
  if (ef == 0) return bits ? -126 : 0;  // fp32 subnormal (a bf16 subnormal group): e < -126 clamps
  return max(ef - 126 - ((bits & 0x7fffffu) <= 0x600000u ? 9 : 8), -126);
}
__device__ __forceinline__ float kv8_pow2(int e) { return __uint_as_float((uint32_t)(e + 127) << 23); }  // e in [-126, 127]
__device__ __forceinline__ float amax8(const float* v) {
  float mx = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) mx = fmaxf(mx, fabsf(v[e]));
  return mx;
}
__device__ __forceinline__ uint2 kv8_pack8(const float* v, int e) {
  const float inv = kv8_pow2(-e);  // e <= 120 for any fp32 amax: 2^-e is a normal number
  int p0 = __builtin_amdgcn_cvt_pk_fp8_f32(v[0] * inv, v[1] * inv, 0, false);
  p0 = __builtin_amdgcn_cvt_pk_fp8_f32(v[2] * inv, v[3] * inv, p0, true);
  int p1 = __builtin_amdgcn_cvt_pk_fp8_f32(v[4] * inv, v[5] * inv, 0, false);
  p1 = __builtin_amdgcn_cvt_pk_fp8_f32(v[6] * inv, v[7] * inv, p1, true);
  return make_uint2((unsigned)p0, (unsigned)p1);
}

// prefill: x [B*S, H, D] (row stride ldx: a view into the fused q|k|v buffer) -> cache rows [b, s < S] and scales [b, h, s]; D/8 lanes per
// group (16-byte loads, group maximum by shuffles, one 8-byte store per lane)
template <int DT, int D>
__global__ __launch_bounds__(256) void kv8_fill_k(const uint16_t* __restrict__ x, int64_t ldx, uint8_t* __restrict__ c8, float* __restrict__ cs,
                                                  int B, int S, int H, int Smax) {
  constexpr int OCT = D / 8;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)B * S * H * OCT) return;  // (whole groups: OCT divides 256)
  const int part = (int)(i % OCT);
  const int64_t g = i / OCT, row = g / H;
  const int h = (int)(g - row * H), b = (int)(row / S), s = (int)(row - (int64_t)b * S);
  float v[8];
  unpack8<DT>(*(const uint4*)(x + row * ldx + (int64_t)h * D + part * 8), v);
  float mx = amax8(v);
#pragma unroll
  for (int o2 = OCT / 2; o2 > 0; o2 >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o2, 64));
  const int e = kv8_exp(mx);
  *(uint2*)(c8 + (((int64_t)b * Smax + s) * H + h) * D + part * 8) = kv8_pack8(v, e);
  if (part == 0) cs[((int64_t)b * H + h) * Smax + s] = kv8_pow2(e);
}

// ---- 1..8 activation rows: ONE WAVE PER WEIGHT ROW -------------------------------------------------------------------------------
// The projections of the decode step are one kernel over a weight-format policy.  A policy holds what differs between the formats and
// nothing else: how a row is addressed, what 16 bytes of it are, which scale goes with them, and the per-format constants of the loop
// and the launcher.  Everything in it resolves at compile time.
//   EPL        elements per 16-byte lane load; a wave step is 64 * EPL elements, and K must be whole lane loads (K % EPL == 0)
//   Row        a weight row: row(W, ldw, wsc, n, K)
//   load       the streamed 16 bytes at element k of a row; ld_scale / scale: the stored scale of the block k lies in (a lane's EPL
//              values lie inside one block) and its fp32 value.  SCALED: a load step's products are summed from 0 and join the
//              accumulator by one fmaf(scale, partial, acc); otherwise they accumulate straight into it.
//   pk16<DT>   values 8 d .. 8 d + 7 of a lane load -> four packed 16-bit pairs (exact), which meet the activations in dot2 instructions
//   chunked    whether the K loop runs in chunks of GEMV_KC; nstep: wave steps of every row requested before any is consumed
//   rows / has_rows   weight rows per wave for a launch, and the (activation rows, weight rows) forms that exist
//   ks_span    elements per wave of the split-K form (HAS_KSPLIT)
//   PAIR_MAX_K, MFMA_MIN, MFMA_PAIR_MIN   launcher limits, see gemv_wave_launch and the per-format fronts
constexpr int GEMV_KC = 2048;  // 32 KiB at MM = 8: four blocks (16 waves) per CU keep enough weight loads in flight

struct W16 {  // bf16 / f16 rows [N, ldw]
  static constexpr int EPL = 8;
  static constexpr bool SCALED = false, HAS_KSPLIT = true;
  // chunked only where the chunk is what LDS holds.  nstep 2: 8 measured the same at N = 4096, where a launch is 2048 short-lived
  // waves (profiles/r02_decode_bench.txt)
  static constexpr bool chunked(bool ldsx, bool norm) { return ldsx && !norm; }
  static constexpr int nstep(bool) { return 2; }
  static constexpr int PAIR_MAX_K = INT_MAX;
  // MFMA form from 3 rows (measured, profiles/r02_gemv_ab.txt: below that this kernel streams faster).  The paired epilogues (SwiGLU,
  // RoPE + append) compete with one-wave-per-row-pair forms that fuse the same work and stream at 4.3-4.5 TB/s up to ~5 rows: measured
  // crossover 6 rows with 16-bit weights, 4 with fp8
  static constexpr int MFMA_MIN = 3, MFMA_PAIR_MIN = 6;
  static inline int mfma_min = MFMA_MIN, mfma_pair_min = MFMA_PAIR_MIN;  // A/B: mh_gemv_mfma_min_rows, mh_gemv_mfma_pair_min_rows
  // weight rows per wave: as many as keep >= ~1000 blocks in flight (N = 4096 with 4 rows per wave is 256 blocks = one per CU, measured
  // at 1.4 TB/s; with 1 row per wave 3+ TB/s).  Fused SwiGLU: a wave's rows are gate/up PAIRS, so an even count
  static int rows(int M, int N, bool swi, bool rope) { return rope ? 2 : M < 3 ? 2 : swi ? 4 : N >= 16384 ? 4 : N >= 8192 ? 2 : 1; }
  static constexpr bool has_rows(int MM, int R) { return R == 2 || MM >= 3; }
  static constexpr int ks_span(int K) { return (((K >> 3) + 3) >> 2) << 3; }  // a multiple of 8
  struct Row { const uint16_t* w; };
  struct Scale {};
  static __device__ __forceinline__ Row row(const void* W, int64_t ldw, const void*, int n, int) { return {(const uint16_t*)W + (int64_t)n * ldw}; }
  static __device__ __forceinline__ uint4 load(const Row& r, int k) { return ld_stream16(r.w + k); }
  static __device__ __forceinline__ Scale ld_scale(const Row&, int) { return {}; }
  static __device__ __forceinline__ float scale(Scale) { return 1.f; }
  template <int DT>
  static __device__ __forceinline__ void pk16(const uint4& v, int, uint32_t* w) { w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w; }
};

struct WFp8 {  // e4m3 bytes [N, K], one fp32 scale per 128 k [N, ceil(K / 128)] (mh_quant_fp8_b128)
  static constexpr int EPL = 16;
  static constexpr bool SCALED = true, HAS_KSPLIT = true;
  // always chunked unless the whole row is staged, one step in flight: neither was measured against the 16-bit form's values
  static constexpr bool chunked(bool, bool norm) { return !norm; }
  static constexpr int nstep(bool) { return 1; }
  static constexpr int PAIR_MAX_K = 8192;
  static constexpr int MFMA_MIN = 3, MFMA_PAIR_MIN = 4;  // see W16
  static inline int mfma_min = MFMA_MIN, mfma_pair_min = MFMA_PAIR_MIN;
  static int rows(int M, int N, bool swi, bool rope) { return (swi || rope) ? 2 : M < 3 ? 1 : N >= 8192 ? 2 : 1; }  // (>= ~1000 blocks, see W16)
  static constexpr bool has_rows(int, int R) { return R <= 2; }
  static constexpr int ks_span(int K) { return ((((K + 127) / 128) + 3) >> 2) << 7; }  // whole 128-blocks
  struct Row { const uint8_t* q; const float* s; };
  using Scale = float;
  static __device__ __forceinline__ Row row(const void* W, int64_t, const void* wsc, int n, int K) {
    return {(const uint8_t*)W + (int64_t)n * K, (const float*)wsc + (int64_t)n * ((K + 127) / 128)};
  }
  static __device__ __forceinline__ uint4 load(const Row& r, int k) { return ld_stream16(r.q + k); }
  static __device__ __forceinline__ Scale ld_scale(const Row& r, int k) { return r.s[k >> 7]; }
  static __device__ __forceinline__ float scale(Scale s) { return s; }
  template <int DT>
  static __device__ __forceinline__ void pk16(const uint4& v, int d, uint32_t* w) {  // (4 cvt + 4 x MM dot2 per row instead of 4 cvt + 8 x MM fma)
    fp8x4_to_pk16<DT>(d ? v.z : v.x, w[0], w[1]);
    fp8x4_to_pk16<DT>(d ? v.w : v.y, w[2], w[3]);
  }
};

struct WFp4 {  // MXFP4: e2m1 codes [N, K / 2], one E8M0 scale byte per 32 k [N, K / 32] (mh_quant_fp4_b32, at the end of this file)
  static constexpr int EPL = 32;  // a lane load is exactly one scale block: 16 cvt + 16 x MM dot2 + MM fma per row and load
  static constexpr bool SCALED = true, HAS_KSPLIT = false;
  // chunked as the 16-bit form; a chunk is then exactly one wave step, so one step is in flight, and two where the loop is not
  // chunked (1-2 rows, NORM).  No split-K form.  Not measured against the other formats' values
  static constexpr bool chunked(bool ldsx, bool norm) { return ldsx && !norm; }
  static constexpr int nstep(bool chunk) { return chunk ? 1 : 2; }
  static constexpr int PAIR_MAX_K = 8192;
  // the fp8 path's values.  Measured at Llama-7B size (profiles/decode_fp4_bench.txt, graph replay, context 613): with these thresholds
  // the fp4 step is 1.78 ms at 1 row (fp8 1.97), 3.01 ms at 5 rows (fp8 3.57) and 3.53 ms at 8 rows (fp8 3.79); the same file holds the
  // 3- and 5-row steps with the MFMA form switched off (mh_gemv_mfma_min_rows(17)).  The weights stream at ~2 TB/s at one row, well below
  // the 16-bit path's 4.7: per byte the wave form issues twice the fp8 form's converts and dot2s, and a 2 KB row is two loads per lane -
  // the step is faster than fp8 but not yet at the byte ratio.
  static constexpr int MFMA_MIN = 3, MFMA_PAIR_MIN = 4;
  static inline int mfma_min = MFMA_MIN, mfma_pair_min = MFMA_PAIR_MIN;
  static int rows(int M, int N, bool swi, bool rope) { return WFp8::rows(M, N, swi, rope); }
  static constexpr bool has_rows(int, int R) { return R <= 2; }
  struct Row { const uint8_t* q; const uint8_t* s; };
  using Scale = uint32_t;  // the stored byte
  static __device__ __forceinline__ Row row(const void* W, int64_t, const void* wsc, int n, int K) {
    return {(const uint8_t*)W + (int64_t)n * (K >> 1), (const uint8_t*)wsc + (int64_t)n * (K >> 5)};
  }
  static __device__ __forceinline__ uint4 load(const Row& r, int k) { return ld_stream16(r.q + (k >> 1)); }
  static __device__ __forceinline__ Scale ld_scale(const Row& r, int k) { return r.s[k >> 5]; }
  static __device__ __forceinline__ float scale(Scale b) { return e8m0_to_f32(b); }
  template <int DT>
  static __device__ __forceinline__ void pk16(const uint4& v, int d, uint32_t* w) { fp4x8_to_pk16<DT>(d == 0 ? v.x : d == 1 ? v.y : d == 2 ? v.z : v.w, w); }
};

template <int DT>
__device__ __forceinline__ void gemv_store(void* out, int64_t ldo, const uint16_t* resid, int64_t ldr, int out_f32, int m, int n, float v) {
  if (resid) v += ld16<DT>(resid[(int64_t)m * ldr + n]);
  if (out_f32) ((float*)out)[(int64_t)m * ldo + n] = v;
  else ((uint16_t*)out)[(int64_t)m * ldo + n] = (uint16_t)st16<DT>(v);
}

// y[m, n] = sum_k x[m, k] W[n, k] (+ resid), W in the format Fmt (wsc: its scales): ROWS weight rows per wave, 4 waves per block, fp32
// accumulate, shuffle reduction.  LDSX: the block first stages a K-chunk of the MM activation rows in LDS (MM x 4096 x 2 B = 64 KiB at
// MM = 8) and every wave reads it from there: without it each wave re-fetches all activations through L1/L2 (8x the weight bytes at
// MM = 8; measured 1.9 TB/s of weights instead of 5).
// NORM: x is the input of the RMSNorm that precedes the projection (HF LlamaRMSNorm, weight norm_w): every block normalises the MM
// rows itself (8 KB each, L2-resident) into LDS - same chunk assignment, summation order and rounding as rmsnorm_fwd_row_k, so the
// result equals the two launches bit for bit - instead of a separate kernel per norm (65 per decode step).
template <class Fmt, int DT, int MM, int ROWS, bool LDSX, bool NORM = false>
__global__ __launch_bounds__(256) void gemv_k(const uint16_t* __restrict__ x, int64_t ldx, const void* __restrict__ W, int64_t ldw,
                                              const void* __restrict__ wsc, void* __restrict__ out, int64_t ldo,
                                              const uint16_t* __restrict__ resid, int64_t ldr, int N, int K, int out_f32, int swi_ff,
                                              const uint16_t* __restrict__ norm_w, float eps, RopeAppend ra) {
  extern __shared__ __attribute__((aligned(16))) uint16_t xs[];  // [MM][GEMV_KC] when LDSX, [MM][K] when NORM
  __shared__ float red[NORM ? MM : 1][4];
  constexpr bool CHUNK = Fmt::chunked(LDSX, NORM);  // (otherwise one pass over the whole of K)
  constexpr int NSTEP = Fmt::nstep(CHUNK), EPL = Fmt::EPL, STEP = 64 * EPL;
  const int xstride = NORM ? K : GEMV_KC;
  const int lane = threadIdx.x & 63;
  // swi_ff > 0 (fused SwiGLU of the gate|up projection, W = [2 ff, K], N = ff outputs): the wave's rows are ROWS/2 gate rows n and
  // the matching up rows ff + n, and it writes act[n] = silu(gate) * up of the ROUNDED 16-bit gate / up values (= mh_swiglu_fwd on
  // the stored projection)
  const int NR = swi_ff > 0 ? ROWS / 2 : ROWS;  // output columns per wave
  const int n0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * NR;
  float acc[ROWS][MM];
#pragma unroll
  for (int r = 0; r < ROWS; ++r)
#pragma unroll
    for (int m = 0; m < MM; ++m) acc[r][m] = 0.f;
  typename Fmt::Row row[ROWS];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    int n = swi_ff > 0 ? (r < NR ? min(n0 + r, N - 1) : swi_ff + min(n0 + r - NR, N - 1)) : min(n0 + r, N - 1);
    if (ROWS == 2 && ra.tab) {  // rotary pair (c, c + D/2) of pair index n0 / 2 (N = 3 H D outputs, N / 2 pairs)
      const int half = ra.D >> 1, pidx = min(n0 >> 1, (N >> 1) - 1), per_sec = ra.H * half;
      const int sec = pidx / per_sec, rem = pidx - sec * per_sec, h = rem / half;
      n = sec * ra.H * ra.D + h * ra.D + (rem - h * half) + r * half;
    }
    row[r] = Fmt::row(W, ldw, wsc, n, K);
  }
  for (int kc = 0; kc < K; kc += GEMV_KC) {
    const int klen = CHUNK ? min(GEMV_KC, K - kc) : K;
    if constexpr (NORM) {
      stage_rmsnorm<DT, MM>(x, ldx, norm_w, eps, K, xs, red);
    } else if constexpr (LDSX) {
      if (kc) __syncthreads();
      for (int i = threadIdx.x * 8; i < MM * klen; i += 256 * 8) {
        const int m = i / klen, k = i - m * klen;
        *(uint4*)(xs + m * GEMV_KC + k) = *(const uint4*)(x + (int64_t)m * ldx + kc + k);
      }
      __syncthreads();
    }
    if (n0 < N) {
      for (int k0 = lane * EPL; k0 < klen; k0 += STEP * NSTEP) {
        uint4 wv[NSTEP][ROWS];
        typename Fmt::Scale sv[NSTEP][ROWS];
#pragma unroll
        for (int u = 0; u < NSTEP; ++u)
#pragma unroll
          for (int r = 0; r < ROWS; ++r) {
            const int kk = k0 + u * STEP;
            const bool ok = kk < klen;  // (the first slot's test folds to the loop condition)
            wv[u][r] = ok ? Fmt::load(row[r], kc + kk) : make_uint4(0, 0, 0, 0);
            sv[u][r] = ok ? Fmt::ld_scale(row[r], kc + kk) : typename Fmt::Scale{};
          }
#pragma unroll
        for (int u = 0; u < NSTEP; ++u) {
          const int kk = k0 + u * STEP;
          if (u > 0 && kk >= klen) break;
          float p[ROWS][MM];
#pragma unroll
          for (int r = 0; r < ROWS; ++r)
#pragma unroll
            for (int m = 0; m < MM; ++m) p[r][m] = Fmt::SCALED ? 0.f : acc[r][m];
#pragma unroll
          for (int d = 0; d < EPL / 8; ++d) {  // 8 values at a time
            uint32_t w[ROWS][4];
#pragma unroll
            for (int r = 0; r < ROWS; ++r) Fmt::template pk16<DT>(wv[u][r], d, w[r]);
#pragma unroll
            for (int m = 0; m < MM; ++m) {
              uint4 xa;
              if constexpr (LDSX || NORM) xa = *(const uint4*)(xs + m * xstride + kk + 8 * d);
              else xa = *(const uint4*)(x + (int64_t)m * ldx + kc + kk + 8 * d);
#pragma unroll
              for (int r = 0; r < ROWS; ++r) {
                float a = p[r][m];
                a = dot2_acc<DT>(w[r][0], xa.x, a);
                a = dot2_acc<DT>(w[r][1], xa.y, a);
                a = dot2_acc<DT>(w[r][2], xa.z, a);
                a = dot2_acc<DT>(w[r][3], xa.w, a);
                p[r][m] = a;
              }
            }
          }
#pragma unroll
          for (int r = 0; r < ROWS; ++r) {
            const float s = Fmt::scale(sv[u][r]);
#pragma unroll
            for (int m = 0; m < MM; ++m) acc[r][m] = Fmt::SCALED ? fmaf(s, p[r][m], acc[r][m]) : p[r][m];
          }
        }
      }
    }
    if constexpr (!CHUNK) break;
  }
  if (n0 >= N) return;
#pragma unroll
  for (int r = 0; r < ROWS; ++r)
#pragma unroll
    for (int m = 0; m < MM; ++m) acc[r][m] = wave_sum(acc[r][m]);
  if constexpr (ROWS == 2) {
    if (ra.tab) {
      if (lane == 0) rope_append_store<DT, MM>(ra, n0 >> 1, acc[0], acc[1], (uint16_t*)out, ldo);
      return;
    }
  }
  if (lane == 0 && swi_ff > 0) {
#pragma unroll
    for (int r = 0; r < ROWS / 2; ++r) {
      const int n = n0 + r;
      if (n >= N) break;
#pragma unroll
      for (int m = 0; m < MM; ++m) {
        const float g_ = ld16<DT>((uint16_t)st16<DT>(acc[r][m])), u_ = ld16<DT>((uint16_t)st16<DT>(acc[r + ROWS / 2][m]));
        ((uint16_t*)out)[(int64_t)m * ldo + n] = (uint16_t)st16<DT>(swiglu_fwd1(g_, u_));
      }
    }
    return;
  }
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      const int n = n0 + r;
      if (n >= N) break;
#pragma unroll
      for (int m = 0; m < MM; ++m) gemv_store<DT>(out, ldo, resid, ldr, out_f32, m, n, acc[r][m]);
    }
  }
}

// 1-2 activation rows and a SMALL N (the o / down projections: 4096 rows): one wave per ROWS weight rows gives 2048 waves for 256 CUs,
// each streaming its rows for the whole of K - the launch is a ramp-up and a tail.  Here the four waves of a block share the same
// ROWS rows and split K in four (Fmt::ks_span elements each, so a lane's values stay inside one scale block), i.e. four times as many
// waves with a quarter of the work each (all 32 wave slots of a CU busy); the four partial sums meet in LDS and are added in a fixed order.
template <class Fmt, int DT, int MM, int ROWS>
__global__ __launch_bounds__(256) void gemv_ks_k(const uint16_t* __restrict__ x, int64_t ldx, const void* __restrict__ W, int64_t ldw,
                                                 const void* __restrict__ wsc, void* __restrict__ out, int64_t ldo,
                                                 const uint16_t* __restrict__ resid, int64_t ldr, int N, int K, int out_f32) {
  __shared__ float red[4][ROWS][MM];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = blockIdx.x * ROWS;
  constexpr int NSTEP = Fmt::nstep(false), EPL = Fmt::EPL, STEP = 64 * EPL;
  const int kq = Fmt::ks_span(K), kb = wave * kq, ke = min(K, kb + kq);
  float acc[ROWS][MM];
#pragma unroll
  for (int r = 0; r < ROWS; ++r)
#pragma unroll
    for (int m = 0; m < MM; ++m) acc[r][m] = 0.f;
  typename Fmt::Row row[ROWS];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) row[r] = Fmt::row(W, ldw, wsc, min(n0 + r, N - 1), K);
  // the K loop of gemv_k over the wave's range, x from global memory.  (Written out a second time: as one inlined function the two loops
  // compile to different register allocations than today's - 38 -> 42 VGPRs in gemv_k<W16, bf16, 7, 1, true> - for no gain.)
  for (int k0 = kb + lane * EPL; k0 < ke; k0 += STEP * NSTEP) {
    uint4 wv[NSTEP][ROWS];
    typename Fmt::Scale sv[NSTEP][ROWS];
#pragma unroll
    for (int u = 0; u < NSTEP; ++u)
#pragma unroll
      for (int r = 0; r < ROWS; ++r) {
        const int kk = k0 + u * STEP;
        const bool ok = kk < ke;
        wv[u][r] = ok ? Fmt::load(row[r], kk) : make_uint4(0, 0, 0, 0);
        sv[u][r] = ok ? Fmt::ld_scale(row[r], kk) : typename Fmt::Scale{};
      }
#pragma unroll
    for (int u = 0; u < NSTEP; ++u) {
      const int kk = k0 + u * STEP;
      if (u > 0 && kk >= ke) break;
      float p[ROWS][MM];
#pragma unroll
      for (int r = 0; r < ROWS; ++r)
#pragma unroll
        for (int m = 0; m < MM; ++m) p[r][m] = Fmt::SCALED ? 0.f : acc[r][m];
#pragma unroll
      for (int d = 0; d < EPL / 8; ++d) {  // 8 values at a time
        uint32_t w[ROWS][4];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) Fmt::template pk16<DT>(wv[u][r], d, w[r]);
#pragma unroll
        for (int m = 0; m < MM; ++m) {
          const uint4 xa = *(const uint4*)(x + (int64_t)m * ldx + kk + 8 * d);
#pragma unroll
          for (int r = 0; r < ROWS; ++r) {
            float a = p[r][m];
            a = dot2_acc<DT>(w[r][0], xa.x, a);
            a = dot2_acc<DT>(w[r][1], xa.y, a);
            a = dot2_acc<DT>(w[r][2], xa.z, a);
            a = dot2_acc<DT>(w[r][3], xa.w, a);
            p[r][m] = a;
          }
        }
      }
#pragma unroll
      for (int r = 0; r < ROWS; ++r) {
        const float s = Fmt::scale(sv[u][r]);
#pragma unroll
        for (int m = 0; m < MM; ++m) acc[r][m] = Fmt::SCALED ? fmaf(s, p[r][m], acc[r][m]) : p[r][m];
      }
    }
  }
#pragma unroll
  for (int r = 0; r < ROWS; ++r)
#pragma unroll
    for (int m = 0; m < MM; ++m) {
      const float t = wave_sum(acc[r][m]);
      if (lane == 0) red[wave][r][m] = t;
    }
  __syncthreads();
  if (threadIdx.x < ROWS * MM) {
    const int r = threadIdx.x / MM, m = threadIdx.x % MM, n = n0 + r;
    if (n < N) gemv_store<DT>(out, ldo, resid, ldr, out_f32, m, n, (red[0][r][m] + red[1][r][m]) + (red[2][r][m] + red[3][r][m]));
  }
}

// ---- 3..16 activation rows: the matrix cores do the multiplies --------------------------------------------------------------------

// At batch 1-2 the one-wave-per-row kernel above is HBM-bound; from ~4 rows on its VALU work (rows x 8 dot2 per 16 B of weights, x 2
// more with fp8 dequantisation) is what limits it.  Here a block owns 16 x RG weight rows and its NW waves split K: every lane loads
// 16 B of one weight row STRAIGHT INTO the MFMA's B-operand registers (lane l: row l & 15, k-chunk l >> 4), and the <= 16 activation
// rows are the A operand, ALSO loaded straight from global memory (L2-resident: M x K x 2 B): every k step is consumed by exactly one
// wave of the block, so an LDS copy of the activations shared nothing and cost two barriers and a dependent round trip per 2 K of k
// (the first form of this kernel: 2.5 TB/s at N = 4096).  One 16x16x32 MFMA per 1 KB of weights replaces 16 x M dot2 instructions:
// the kernel is HBM-bound for any M <= 16.  fp8 weights (16 values per 16 B, per-128-block fp32 scales) are converted to 16-bit in
// registers (16 cvt per load instead of 16 x M fma) and their block's partial product is scaled once per load step.  The K loop runs in
// passes of NW waves x NS steps whose loads are all requested before the first MFMA.  Partial tiles of the NW waves are summed through
// LDS in a fixed order.
// RG = 16-row groups per block (1, 2 or 4): a block re-reads the whole activation matrix (M x K) from L2 whatever it does with it, so
// at 16 rows per block that traffic equals the weight stream at M = 16 and the kernel is L2-bound (measured 2.9 TB/s); 64 rows per
// block share one A fragment per step between four B fragments.  Large N only: N / 64 blocks must still fill the chip.
// NW = 8, or 16 for small N (N = 4096: 256 blocks x 16 waves, i.e. twice the loads in flight at the start).
// PAIR (RG = 2): the block's second row group is the PARTNER of the first instead of the next 16 rows, and wave 0's epilogue combines
// them on the rounded 16-bit values, exactly as the separate launches would: 1 = SwiGLU of the gate|up projection (group 1 = up rows
// ff + n; N = ff outputs act = silu(gate) * up), 2 = RoPE + K/V append of the q|k|v projection (group 1 = channel c + D/2 of the same
// head; a block is 16 channels c of one head of one section; D/2 a multiple of 16).
template <int DT, bool FP8W, int RG, int NW, int PAIR = 0>
__global__ __launch_bounds__(NW * 64) void gemv_mfma_k(const uint16_t* __restrict__ x, int64_t ldx, const void* __restrict__ Wv, int64_t ldw,
                                                       const float* __restrict__ wsc, void* __restrict__ out, int64_t ldo,
                                                       const uint16_t* __restrict__ resid, int64_t ldr, int M, int N, int K, int out_f32,
                                                       int swi_ff, RopeAppend ra) {
  static_assert(PAIR == 0 || RG == 2, "paired epilogues take two row groups");
  __shared__ __attribute__((aligned(16))) float red[NW * RG * 64 * 4];
  constexpr int KS = FP8W ? 64 : 32;                      // k per step (16 B of one weight row per lane, 4 lanes per row)
  constexpr int NS = FP8W ? (RG == 1 ? 6 : 4) : (RG == 4 ? 4 : 8);  // steps per wave per pass (registers)
  constexpr int KP = NW * NS * KS;                        // k per pass
  constexpr int ES = FP8W ? 1 : 2;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, kq = lane >> 4;
  int n0 = blockIdx.x * 16 * RG, goff = 16, nlim = N;  // first row, distance between the row groups, row count of W
  if constexpr (PAIR == 1) { n0 = blockIdx.x * 16; goff = swi_ff; nlim = N + swi_ff; }
  if constexpr (PAIR == 2) {
    const int half = ra.D >> 1, spb = half >> 4, slot = blockIdx.x / spb;  // slot = section * H + head
    n0 = slot * ra.D + (blockIdx.x - slot * spb) * 16;
    goff = half;
  }
  const bool arow = j < M;
  f32x4_t acc[RG];
  const uint8_t* wr[RG];   // byte pointers: element size 1 (fp8) or 2
  const float* sr[RG];
  const int nb = (K + 127) / 128;
#pragma unroll
  for (int g = 0; g < RG; ++g) {
    const int n = PAIR == 1 ? min(n0 + j, N - 1) + g * goff : min(n0 + goff * g + j, nlim - 1);
    acc[g] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    wr[g] = (const uint8_t*)Wv + ((int64_t)n * ldw + kq * (KS / 4)) * ES;
    sr[g] = FP8W ? wsc + (int64_t)n * nb : nullptr;
  }
  const uint16_t* xr = x + (int64_t)min(j, M - 1) * ldx + kq * (KS / 4);
  for (int kp = 0; kp < K; kp += KP) {
    uint4 wv[RG][NS], xv[NS][FP8W ? 2 : 1];
    float sv[FP8W ? RG : 1][FP8W ? NS : 1];
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      const int k = kp + (wave + NW * u) * KS;
      const bool ok = k < K;
#pragma unroll
      for (int g = 0; g < RG; ++g) {
        wv[g][u] = ok ? ld_stream16(wr[g] + (int64_t)k * ES) : make_uint4(0, 0, 0, 0);
        if constexpr (FP8W) sv[g][u] = ok ? sr[g][k >> 7] : 0.f;
      }
      xv[u][0] = (ok && arow) ? *(const uint4*)(xr + k) : make_uint4(0, 0, 0, 0);
      if constexpr (FP8W) xv[u][1] = (ok && arow) ? *(const uint4*)(xr + k + 8) : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      if (kp + (wave + NW * u) * KS >= K) break;
      if constexpr (!FP8W) {
#pragma unroll
        for (int g = 0; g < RG; ++g) acc[g] = mfma16<DT>(xv[u][0], wv[g][u], acc[g]);
      } else {
#pragma unroll
        for (int g = 0; g < RG; ++g) {
          uint4 b0, b1;  // 16 e4m3 -> 2 x 8 packed 16-bit values (exact), one convert per pair
          fp8x4_to_pk16<DT>(wv[g][u].x, b0.x, b0.y); fp8x4_to_pk16<DT>(wv[g][u].y, b0.z, b0.w);
          fp8x4_to_pk16<DT>(wv[g][u].z, b1.x, b1.y); fp8x4_to_pk16<DT>(wv[g][u].w, b1.z, b1.w);
          f32x4_t part = {0.f, 0.f, 0.f, 0.f};
          part = mfma16<DT>(xv[u][0], b0, part);
          part = mfma16<DT>(xv[u][1], b1, part);
#pragma unroll
          for (int q = 0; q < 4; ++q) acc[g][q] = fmaf(sv[g][u], part[q], acc[g][q]);
        }
      }
    }
  }
  // D lane l reg r = D[m = 4 * (l >> 4) + r][n = l & 15]: sum the NW waves' tiles in wave order
#pragma unroll
  for (int g = 0; g < RG; ++g) *(f32x4_t*)(red + ((wave * RG + g) * 64 + lane) * 4) = acc[g];
  __syncthreads();
  if constexpr (PAIR != 0) {
    if (wave == 0) {
      f32x4_t s0 = *(const f32x4_t*)(red + lane * 4), s1 = *(const f32x4_t*)(red + (64 + lane) * 4);
#pragma unroll 4
      for (int w = 1; w < NW; ++w) {
        const f32x4_t t0 = *(const f32x4_t*)(red + ((w * 2) * 64 + lane) * 4), t1 = *(const f32x4_t*)(red + ((w * 2 + 1) * 64 + lane) * 4);
#pragma unroll
        for (int r = 0; r < 4; ++r) { s0[r] += t0[r]; s1[r] += t1[r]; }
      }
      uint16_t* o16 = (uint16_t*)out;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = 4 * kq + r;
        if (m >= M) continue;
        float lo = ld16<DT>((uint16_t)st16<DT>(s0[r])), hi = ld16<DT>((uint16_t)st16<DT>(s1[r]));  // the projection as it would be stored
        if constexpr (PAIR == 1) {
          if (n0 + j < N) o16[(int64_t)m * ldo + n0 + j] = (uint16_t)st16<DT>(swiglu_fwd1(lo, hi));
        } else {
          const int half = ra.D >> 1, slot = n0 / ra.D, sec = slot / ra.H, c = n0 - slot * ra.D + j, p = ra.pos[m];
          const int64_t HD = (int64_t)ra.H * ra.D, col = (int64_t)(slot - sec * ra.H) * ra.D + c;
          if (sec < 2) {
            const float2 cs = ra.tab[(int64_t)ra.rpos[m] * half + c];
            rope_rot(lo, hi, cs.x, cs.y, lo, hi);
          }
          const uint16_t l16 = (uint16_t)st16<DT>(lo), h16 = (uint16_t)st16<DT>(hi);
          o16[(int64_t)m * ldo + sec * HD + col] = l16;
          o16[(int64_t)m * ldo + sec * HD + col + half] = h16;
          if (sec > 0) {
            uint16_t* dst = (sec == 1 ? ra.kc : ra.vc) + ((int64_t)m * ra.Smax + p) * HD + col;
            dst[0] = l16;
            dst[half] = h16;
          }
        }
      }
    }
    return;
  }
  if (wave < RG) {
    const int g = wave;
    f32x4_t s4 = *(const f32x4_t*)(red + (g * 64 + lane) * 4);
#pragma unroll
    for (int w = 1; w < NW; ++w) {
      const f32x4_t t = *(const f32x4_t*)(red + ((w * RG + g) * 64 + lane) * 4);
#pragma unroll
      for (int r = 0; r < 4; ++r) s4[r] += t[r];
    }
    const int n = n0 + 16 * g + j;
    if (n < N) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = 4 * kq + r;
        if (m >= M) continue;
        float v = s4[r];
        if (resid) v += ld16<DT>(resid[(int64_t)m * ldr + n]);
        if (out_f32) ((float*)out)[(int64_t)m * ldo + n] = v;
        else ((uint16_t*)out)[(int64_t)m * ldo + n] = (uint16_t)st16<DT>(v);
      }
    }
  }
}

static int g_gemv_mfma_nw16 = 1;  // 16 waves per block at small N (A-B switch: mh_gemv_mfma_wide)
extern "C" void mh_gemv_mfma_wide(int on) { g_gemv_mfma_nw16 = on ? 1 : 0; }

template <int DT, bool FP8W>
static int launch_gemv_mfma(const void* x, int64_t ldx, const void* W, int64_t ldw, const float* wsc, void* out, int64_t ldo, const void* resid,
                            int64_t ldr, int M, int N, int K, int out_f32, int swi_ff, const RopeAppend& ra, hipStream_t st) {
  // rows per block: as many as still give ~1.5+ blocks per CU: measured, 64-row blocks win at N = 32 064 (501 blocks) and lose at
  // N = 22 016 (344 blocks: an uneven second block per CU)
#define MH_GM(RG_, NW_, PAIR_, BLOCKS_)                                                                                                \
  hipLaunchKernelGGL((gemv_mfma_k<DT, FP8W, RG_, NW_, PAIR_>), dim3(BLOCKS_), dim3(64 * NW_), 0, st, (const uint16_t*)x, ldx, W, ldw, wsc, \
                     out, ldo, (const uint16_t*)resid, ldr, M, N, K, out_f32, swi_ff, ra)
  if (swi_ff) MH_GM(2, 8, 1, (N + 15) / 16);           // N = ff outputs
  else if (ra.tab) {                                   // N = 3 H D rows, 16 rotary pairs per block (N = 12 288: 384 blocks)
    if (g_gemv_mfma_nw16) MH_GM(2, 16, 2, N / 32); else MH_GM(2, 8, 2, N / 32);
  }
  else if (N >= 30000) MH_GM(4, 8, 0, (N + 63) / 64);
  else if (N >= 12000) MH_GM(2, 8, 0, (N + 31) / 32);
  else if (N <= 8192 && g_gemv_mfma_nw16) MH_GM(1, 16, 0, (N + 15) / 16);
  else MH_GM(1, 8, 0, (N + 15) / 16);
#undef MH_GM
  MH_LAUNCH_CHECK();
}

// the two 8-channel pieces (c.., c + D/2..) a lane of rope_append_k holds of one head's 16-bit row -> e4m3 at dst, dst + half; the head is
// `vph` neighbouring lanes, whose first writes the group's scale
template <int DT>
__device__ __forceinline__ void kv8_store_pair(const uint4& plo, const uint4& phi, int vph, bool first, uint8_t* dst, int half, float* sdst) {
  float lo[8], hi[8];
  unpack8<DT>(plo, lo);
  unpack8<DT>(phi, hi);
  float mx = fmaxf(amax8(lo), amax8(hi));
  for (int o2 = vph >> 1; o2 > 0; o2 >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o2, 64));
  const int e = kv8_exp(mx);
  *(uint2*)dst = kv8_pack8(lo, e);
  *(uint2*)(dst + half) = kv8_pack8(hi, e);
  if (first) *sdst = kv8_pow2(e);
}

// qkv [B, 3, H, D] of the new tokens; tab [max_pos, D/2] (cos, sin); kc, vc [B, Smax, H*D]
// KV8: kc_, vc_ are e4m3 bytes and ks, vs [B, H, Smax] receive the group scales (fp8 KV cache, above): q, k are rotated exactly as in the
// 16-bit form, then the ROUNDED 16-bit k row and the v row as it lies in qkv are quantised; a head is D/16 neighbouring lanes (D 64 or 128).
// One lane's share (the 8-channel pieces v of the two halves of head h) of qkv row m of sequence b: rotary position rp, cache row p.  The ONE
// definition of the rotate / quantise / store sequence, shared by the one-token kernel and the T-token kernel.
template <int DT, bool KV8>
__device__ __forceinline__ void rope_append_lane(uint16_t* __restrict__ qkv, const float2* __restrict__ tab, void* __restrict__ kc_,
                                                 void* __restrict__ vc_, float* __restrict__ ks, float* __restrict__ vs, int m, int b, int h,
                                                 int v, int p, int rp, int H, int D, int Smax) {
  const int half = D >> 1, vph = half >> 3;
  const float2* tb = tab + (int64_t)rp * half + v * 8;
  const int64_t hd = (int64_t)h * D + v * 8;
  uint16_t* qb = qkv + (int64_t)m * 3 * H * D + hd;
  uint16_t* kb = qb + (int64_t)H * D;
  const uint16_t* vb = kb + (int64_t)H * D;
  const int64_t cdst = ((int64_t)b * Smax + p) * H * D + hd, sdst = ((int64_t)b * H + h) * Smax + p;  // cache element, scale (KV8)
#pragma unroll
  for (int which = 0; which < 2; ++which) {
    uint16_t* base = which ? kb : qb;
    float lo[8], hi[8];
    unpack8<DT>(*(const uint4*)base, lo);
    unpack8<DT>(*(const uint4*)(base + half), hi);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      rope_rot(lo[k], hi[k], tb[k].x, tb[k].y, lo[k], hi[k]);
    }
    const uint4 plo = pack8<DT>(lo), phi = pack8<DT>(hi);
    *(uint4*)base = plo;
    *(uint4*)(base + half) = phi;
    if (which) {
      if constexpr (KV8) kv8_store_pair<DT>(plo, phi, vph, v == 0, (uint8_t*)kc_ + cdst, half, ks + sdst);
      else {
        uint16_t* kdst = (uint16_t*)kc_ + cdst;
        *(uint4*)kdst = plo;
        *(uint4*)(kdst + half) = phi;
      }
    }
  }
  if constexpr (KV8) {
    kv8_store_pair<DT>(*(const uint4*)vb, *(const uint4*)(vb + half), vph, v == 0, (uint8_t*)vc_ + cdst, half, vs + sdst);
  } else {
    uint16_t* vdst = (uint16_t*)vc_ + cdst;
    *(uint4*)vdst = *(const uint4*)vb;
    *(uint4*)(vdst + half) = *(const uint4*)(vb + half);
  }
}

template <int DT, bool KV8>
__global__ __launch_bounds__(256) void rope_append_k(uint16_t* __restrict__ qkv, const float2* __restrict__ tab,
                                                     const int32_t* __restrict__ pos, const int32_t* __restrict__ rpos,
                                                     void* __restrict__ kc_, void* __restrict__ vc_, float* __restrict__ ks,
                                                     float* __restrict__ vs, int B, int H, int D, int Smax) {
  const int vph = D >> 4;
  const int64_t total = (int64_t)B * H * vph;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int v = (int)(i % vph);
  const int h = (int)((i / vph) % H);
  const int b = (int)(i / ((int64_t)vph * H));
  rope_append_lane<DT, KV8>(qkv, tab, kc_, vc_, ks, vs, b, b, h, v, pos[b], rpos[b], H, D, Smax);
}

// ---- one query per (sequence or beam, head): ONE KERNEL over a cache-format policy and a row-source policy --------------------------------
// A format policy holds what differs between the KV-cache formats and nothing else (the W* policies' convention, above):
//   ES, Raw    bytes per cache element, and a lane's 8-element piece of a key / value row as it is loaded
//   load / zero / to_f32<DT>   the streamed piece, the piece of a key beyond the range, and its 8 values
//   SCALED     one fp32 scale per (row, head, key) multiplies the score and the probability: s_j = (q . k8_j) ks_j scale,
//              o += (p_j vs_j) v8_j - one multiply per key, none per element, and - the scales being powers of two - the arithmetic of the
//              16-bit form on the dequantised cache
//   UNR_DENSE  key rows requested per thread before any is used, dense rows (the cache is streamed, so what limits the rate is bytes in flight)
struct KV16 {  // bf16 / f16 rows
  static constexpr int ES = 2, UNR_DENSE = 4;  // (4: not measured against other depths)
  static constexpr bool SCALED = false;
  using Raw = uint4;
  static __device__ __forceinline__ Raw load(const void* p) { return ld_stream16(p); }
  static __device__ __forceinline__ Raw zero() { return make_uint4(0, 0, 0, 0); }
  template <int DT>
  static __device__ __forceinline__ void to_f32(const Raw& r, float* f) { unpack8<DT>(r, f); }
};
struct KVFp8 {  // e4m3 bytes and fp32 scales (fp8 KV cache, above)
  static constexpr int ES = 1, UNR_DENSE = 8;  // (a lane's piece is 8 bytes, so twice the rows for the same bytes in flight; not measured against 4)
  static constexpr bool SCALED = true;
  using Raw = uint2;
  static __device__ __forceinline__ Raw load(const void* p) { return ld_stream8(p); }
  static __device__ __forceinline__ Raw zero() { return make_uint2(0, 0); }
  template <int DT>
  static __device__ __forceinline__ void to_f32(const Raw& r, float* f) {
    fp8x4_to_f32(r.x, f);
    fp8x4_to_f32(r.y, f + 4);
  }
};
template <bool KV8>
using KVFmt = std::conditional_t<KV8, KVFp8, KV16>;

// A row-source policy says which cache row holds key j of query row m - row0() + row(j), where row0() is folded into the block's base
// pointers once - how many rows are requested ahead, and what a launch leaves.
// Either way the cache is [rows, S, H*D] with scales [rows, H, S], the keys are [0, min(lens[m], S)), and split sp leaves its partial in
// slot `slot0 + sp` of the `wsplits`-wide ws row (m*H + h).
struct DenseRows {  // mh_attn_decode: sequence m's keys lie in cache row m (S = Smax).  One split writes the normalised result itself
  static constexpr bool DIRECT = true;
  template <class Fmt>
  static constexpr int UNR = Fmt::UNR_DENSE;
  int m;
  __device__ __forceinline__ DenseRows(const int32_t*, int, int m_, int, int) : m(m_) {}
  __device__ __forceinline__ int row0() const { return m; }
  __device__ __forceinline__ int row(int, bool) const { return 0; }
};
struct AncestryRows {  // the suffix part of mh_attn_decode_beams: key j of beam row m lies in suffix row anc[m, j] (S = G).  Always partials
  static constexpr bool DIRECT = false;
  template <class Fmt>
  static constexpr int UNR = 4;  // (both formats; not measured against other depths)
  const int32_t* anc;
  int last;
  __device__ __forceinline__ AncestryRows(const int32_t* anc_, int rows, int m, int G, int key0) : anc(anc_ + (int64_t)m * G + key0), last(rows - 1) {}
  __device__ __forceinline__ int row0() const { return 0; }
  __device__ __forceinline__ int row(int j, bool ok) const { return ok ? min(max(anc[j], 0), last) : 0; }
};

// q [M, ldq] (head h at h*D); kc, vc [rows, S, H*D] (ks, vs [rows, H, S]: Fmt::SCALED); out [M, H*D]; D in {64, 128}.
// Split-KV ("flash decoding"): with M*H blocks only (32 at batch 1) the cache streams at a few % of HBM speed, so `splits` blocks share
// one (m, h), each takes `chunk` keys and leaves (unnormalised o[D], max, sum) in `ws`; attn_decode_combine_k merges them as a second
// launch.  Dense rows with splits == 1 write the normalised result directly.
template <class Fmt, class Rows, int DT, int D>
__global__ __launch_bounds__(256) void attn_decode_k(const uint16_t* __restrict__ q, int64_t ldq, const void* __restrict__ kc_,
                                                     const void* __restrict__ vc_, const float* __restrict__ ks,
                                                     const float* __restrict__ vs, uint16_t* __restrict__ out,
                                                     const int32_t* __restrict__ lens, const int32_t* __restrict__ anc, int rows, int H, int S,
                                                     float scale_log2, int splits, int chunk, float* __restrict__ ws, int slot0,
                                                     int wsplits) {
  extern __shared__ float sc[];  // [chunk] scores, then [G][D] partial outputs
  __shared__ float red[8];
  typedef typename Fmt::Raw Raw;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sp = blockIdx.x % splits;
  const int h = (blockIdx.x / splits) % H, m = blockIdx.x / (splits * H);
  const int key0 = sp * chunk;
  const int len = max(0, min(min(lens[m], S) - key0, chunk));  // keys [key0, key0 + len) of this split
  const int64_t HD = (int64_t)H * D;
  const Rows src(anc, rows, m, S, key0);
  // thread = (key slice gsl of G = 256*8/D, channel octet c) in both passes: a row is one coalesced read of D/8 lanes, 8 values each
  constexpr int OCT = D / 8, G = 256 / OCT, UNR = Rows::template UNR<Fmt>;
  const int c = tid % OCT, gsl = tid / OCT;
  // key j of this split in cache row row0() + r: its piece for this thread, and its scale
  const int64_t piece0 = ((((int64_t)src.row0() * S + key0) * HD) + (int64_t)h * D + c * 8) * Fmt::ES;
  const int64_t scale0 = ((int64_t)src.row0() * H + h) * S + key0;
  const uint8_t* kc = (const uint8_t*)kc_ + piece0;
  const uint8_t* vc = (const uint8_t*)vc_ + piece0;
  auto piece = [&](const uint8_t* base, int r, int j) { return base + ((int64_t)r * S + j) * HD * Fmt::ES; };
  auto scale = [&](const float* base, int r, int j) { return base[((int64_t)r * H) * S + scale0 + j]; };
  // pass 1: the partial dot products are summed across a key's lane group by shuffles
  float q8[8];
  unpack8<DT>(*(const uint4*)(q + (int64_t)m * ldq + (int64_t)h * D + c * 8), q8);
  float mx = -1e30f;
  for (int j0 = 0; j0 < len; j0 += G * UNR) {
    Raw kraw[UNR];
    float ksc[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int j = j0 + u * G + gsl;
      const bool ok = j < len;
      const int r = src.row(j, ok);
      kraw[u] = ok ? Fmt::load(piece(kc, r, j)) : Fmt::zero();
      if constexpr (Fmt::SCALED) ksc[u] = ok ? scale(ks, r, j) : 0.f;
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int j = j0 + u * G + gsl;
      float kv[8];
      Fmt::template to_f32<DT>(kraw[u], kv);
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) s = fmaf(q8[e], kv[e], s);
#pragma unroll
      for (int o2 = OCT / 2; o2 > 0; o2 >>= 1) s += __shfl_xor(s, o2, 64);
      if constexpr (Fmt::SCALED) s = s * ksc[u] * scale_log2;
      else s *= scale_log2;
      if (j < len) {
        if (c == 0) sc[j] = s;
        mx = fmaxf(mx, s);
      }
    }
  }
  mx = wave_max(mx);
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  float sum = 0.f;
  for (int j = tid; j < len; j += 256) {
    const float pj = fast_exp2(sc[j] - mx);
    sc[j] = pj;
    sum += pj;
  }
  sum = wave_sum(sum);
  if (lane == 0) red[4 + wave] = sum;
  __syncthreads();
  sum = (red[4] + red[5]) + (red[6] + red[7]);
  // pass 2: 8 channels per thread over the keys of its slice
  float o[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = 0.f;
  for (int j0 = gsl; j0 < len; j0 += G * UNR) {
    Raw vraw[UNR];
    float pj[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int j = j0 + u * G;
      const bool ok = j < len;
      const int r = src.row(j, ok);
      vraw[u] = ok ? Fmt::load(piece(vc, r, j)) : Fmt::zero();
      if constexpr (Fmt::SCALED) pj[u] = ok ? sc[j] * scale(vs, r, j) : 0.f;
      else pj[u] = ok ? sc[j] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      float vv[8];
      Fmt::template to_f32<DT>(vraw[u], vv);
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = fmaf(pj[u], vv[e], o[e]);
    }
  }
  __syncthreads();  // everyone is done reading the scores: reuse the buffer for the slice partials
  float* part = sc;  // [G][D]
#pragma unroll
  for (int e = 0; e < 8; ++e) part[gsl * D + c * 8 + e] = o[e];
  __syncthreads();
  if (tid < D) {
    float a = 0.f;
    for (int g2 = 0; g2 < G; ++g2) a += part[g2 * D + tid];
    if (Rows::DIRECT && splits == 1) {
      out[(int64_t)m * HD + (int64_t)h * D + tid] = (uint16_t)st16<DT>(len > 0 ? a / sum : 0.f);
    } else {
      float* w = ws + ((int64_t)(m * H + h) * wsplits + slot0 + sp) * (D + 2);
      w[tid] = a;
      if (tid == 0) { w[D] = mx; w[D + 1] = sum; }
    }
  }
}

// (splits <= 32: every partial is requested before any is used - the kernel is a handful of dependent L2 round trips otherwise)
template <int DT, int D>
__global__ __launch_bounds__(D) void attn_decode_combine_k(const float* __restrict__ ws, uint16_t* __restrict__ out, int H, int splits) {
  __shared__ float sm[32], sl[32];
  const int bh = blockIdx.x, tid = threadIdx.x;
  const float* w = ws + (int64_t)bh * splits * (D + 2);
  float v[32];
#pragma unroll
  for (int s2 = 0; s2 < 32; ++s2) v[s2] = s2 < splits ? w[s2 * (D + 2) + tid] : 0.f;
  if (tid < splits) {
    sm[tid] = w[tid * (D + 2) + D];
    sl[tid] = w[tid * (D + 2) + D + 1];
  }
  __syncthreads();
  float M = -1e30f;
  for (int s2 = 0; s2 < splits; ++s2) M = fmaxf(M, sm[s2]);
  float num = 0.f, den = 0.f;
#pragma unroll
  for (int s2 = 0; s2 < 32; ++s2) {
    if (s2 < splits) {
      const float f = fast_exp2(sm[s2] - M);
      num += v[s2] * f;
      den += sl[s2] * f;
    }
  }
  out[(int64_t)bh * D + tid] = (uint16_t)st16<DT>(den > 0.f ? num / den : 0.f);
}

// ---- T new tokens per sequence in one step (prompt-lookup verify step of generate()): qkv rows m = b*T + t ----------------------------
// rope_append_k over T consecutive positions: row m is rotated at rpos[b] + t and appended at cache row pos[b] + t by the same
// rope_append_lane; rows whose cache row would lie at or beyond Smax are left untouched.
template <int DT, bool KV8>
__global__ __launch_bounds__(256) void rope_append_multi_k(uint16_t* __restrict__ qkv, const float2* __restrict__ tab,
                                                           const int32_t* __restrict__ pos, const int32_t* __restrict__ rpos,
                                                           void* __restrict__ kc_, void* __restrict__ vc_, float* __restrict__ ks,
                                                           float* __restrict__ vs, int B, int T, int H, int D, int Smax) {
  const int half = D >> 1, vph = half >> 3;
  const int64_t total = (int64_t)B * T * H * vph;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int v = (int)(i % vph);
  const int h = (int)((i / vph) % H);
  const int m = (int)(i / ((int64_t)vph * H));
  const int b = m / T, t = m - b * T;
  const int p = pos[b] + t;
  if (p >= Smax || p < 0) return;  // (the vph lanes of a head leave together: kv8_store_pair's shuffles stay inside the head)
  rope_append_lane<DT, KV8>(qkv, tab, kc_, vc_, ks, vs, m, b, h, v, p, rpos[b] + t, H, D, Smax);
}

// Decode attention for T <= TQ queries of one (sequence, head): q rows m = b*T + t, query t sees keys [0, min(lens[b] + t, Smax)).
// Block per (b, h, key split), the structure of attn_decode_k with every key and value row loaded ONCE for all the queries:
//   pass 1  S = K Q^T on the matrix pipe: a wave takes 16 keys per MFMA tile, a lane loads 16 B (fp8 cache: 8 B, converted exactly to the
//           16-bit type) of one key row straight into the A operand, the TQ query rows are the B operand (registers, loaded once), and the
//           16 x 16 fp32 tile lands as lane (key 4*(l>>4) + r, query l & 15) - no cross-lane sums.  Scores go to LDS key-major,
//           sc[j * TQ + t]; keys a query may not see yet are stored as they are and masked when they are exponentiated.
//   softmax per query: its own limit, max and sum (a thread of the exp pass keeps one query: 256 % TQ == 0).
//   pass 2  thread = (key slice, 8 channels) as in attn_decode_k; a value row is loaded once and accumulated into TQ x 8 fp32 registers
//           with the key's TQ probabilities read from LDS as one broadcast row.  Key slices are summed by shuffles inside a wave, then the
//           four waves through LDS.
// Partials (splits > 1) go to ws rows ((b*T + t)*H + h, split) in attn_decode_k's layout: attn_decode_combine_k merges them with B*T rows.
// BEAMS (the prefix part of mh_attn_decode_beams): the T queries are the beams of prompt b and all of them see all min(lens[b], Smax)
// keys - no per-query limit; the block always leaves partials, in slot sp of a ws row that is wsplits slots wide (the suffix part fills
// the slots behind the prefix splits).  Nothing else differs, and nothing differs where BEAMS is false.
template <int DT, int D, int TQ, bool KV8, bool BEAMS = false>
__global__ __launch_bounds__(256) void attn_decode_multi_k(const uint16_t* __restrict__ q, int64_t ldq, const void* __restrict__ kc_,
                                                           const void* __restrict__ vc_, const float* __restrict__ ks,
                                                           const float* __restrict__ vs, uint16_t* __restrict__ out,
                                                           const int32_t* __restrict__ lens, int T, int H, int Smax, float scale_log2,
                                                           int splits, int chunk, float* __restrict__ ws, int wsplits) {
  static_assert(TQ == 4 || TQ == 8 || TQ == 16, "a probability row is read as 16-byte pieces; the MFMA tile holds 16 queries");
  extern __shared__ __attribute__((aligned(16))) float sc[];  // [chunk][TQ] scores, then [4][TQ][D] partial outputs
  __shared__ float red_mx[4][16], red_sum[4][16];
  constexpr int ES = KV8 ? 1 : 2;            // bytes per cache element
  constexpr int KK = D / 32;                 // MFMA k steps per key tile
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sp = blockIdx.x % splits;
  const int h = (blockIdx.x / splits) % H, b = blockIdx.x / (splits * H);
  const int key0 = sp * chunk;
  const int len0 = lens[b];
  // keys [key0, key0 + len) of this split that the LAST query sees; query t sees the first lim(t) of them
  const int len = max(0, min(min(BEAMS ? len0 : len0 + T - 1, Smax) - key0, chunk));
  const int64_t HD = (int64_t)H * D;
  const uint8_t* kc = (const uint8_t*)kc_ + (((int64_t)b * Smax + key0) * HD + (int64_t)h * D) * ES;
  const uint8_t* vc = (const uint8_t*)vc_ + (((int64_t)b * Smax + key0) * HD + (int64_t)h * D) * ES;
  if constexpr (KV8) {
    ks += ((int64_t)b * H + h) * Smax + key0;
    vs += ((int64_t)b * H + h) * Smax + key0;
  }
  // ---- pass 1
  const int jj = lane & 15, kq = lane >> 4;
  uint4 qf[KK];
#pragma unroll
  for (int kk = 0; kk < KK; ++kk)
    qf[kk] = jj < T ? *(const uint4*)(q + (int64_t)(b * T + jj) * ldq + (int64_t)h * D + kk * 32 + kq * 8) : make_uint4(0, 0, 0, 0);
  const int limq = BEAMS ? len : max(0, min(min(len0 + jj, Smax) - key0, chunk));  // keys of this split that query jj sees (jj >= T: unused)
  float mx = -1e30f;
  constexpr int UNR = 4;  // key tiles requested per wave before any is used
  const int ntile = (len + 15) >> 4;
  for (int t0 = wave; t0 < ntile; t0 += 4 * UNR) {
    uint4 kraw[UNR][KK];
    float ksc[UNR][4];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int j = (t0 + 4 * u) * 16 + jj;
      const bool ok = j < len;
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) {
        const uint8_t* src = kc + ((int64_t)j * HD + kk * 32 + kq * 8) * ES;
        if constexpr (KV8) {
          const uint2 r = ok ? ld_stream8(src) : make_uint2(0, 0);
          kraw[u][kk] = make_uint4(r.x, r.y, 0, 0);
        } else {
          kraw[u][kk] = ok ? ld_stream16(src) : make_uint4(0, 0, 0, 0);
        }
      }
      if constexpr (KV8) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int jr = (t0 + 4 * u) * 16 + 4 * kq + r;
          ksc[u][r] = jr < len ? ks[jr] : 0.f;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int jt = (t0 + 4 * u) * 16;
      if (jt >= len) break;
      f32x4_t s4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) {
        uint4 a = kraw[u][kk];
        if constexpr (KV8) {
          const uint32_t lo = a.x, hi = a.y;
          fp8x4_to_pk16<DT>(lo, a.x, a.y);
          fp8x4_to_pk16<DT>(hi, a.z, a.w);
        }
        s4 = mfma16<DT>(a, qf[kk], s4);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = jt + 4 * kq + r;
        float s = s4[r] * scale_log2;
        if constexpr (KV8) s = s4[r] * ksc[u][r] * scale_log2;
        if (j < len) {
          if (jj < TQ) sc[j * TQ + jj] = s;
          if (j < limq) mx = fmaxf(mx, s);
        }
      }
    }
  }
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  if (lane < 16) red_mx[wave][lane] = mx;
  __syncthreads();
  // ---- softmax per query: thread tid keeps query tq = tid % TQ through the whole pass
  const int tq = tid & (TQ - 1);
  const int lim = tq < T ? (BEAMS ? len : max(0, min(min(len0 + tq, Smax) - key0, chunk))) : 0;
  const float mxq = fmaxf(fmaxf(red_mx[0][tq], red_mx[1][tq]), fmaxf(red_mx[2][tq], red_mx[3][tq]));
  float sum = 0.f;
  for (int idx = tid; idx < len * TQ; idx += 256) {
    const int j = idx / TQ;
    const float pj = j < lim ? fast_exp2(sc[idx] - mxq) : 0.f;
    sc[idx] = pj;
    sum += pj;
  }
#pragma unroll
  for (int o2 = 32; o2 >= TQ; o2 >>= 1) sum += __shfl_xor(sum, o2, 64);
  if (lane < TQ) red_sum[wave][lane] = sum;
  __syncthreads();
  // ---- pass 2
  constexpr int OCT = D / 8;    // lanes per value row
  constexpr int G = 256 / OCT;  // key slices of the block
  constexpr int UNR2 = KV8 ? 4 : 2;
  const int c = tid % OCT, gsl = tid / OCT;
  float o[TQ][8];
#pragma unroll
  for (int t = 0; t < TQ; ++t)
#pragma unroll
    for (int e = 0; e < 8; ++e) o[t][e] = 0.f;
  for (int j0 = gsl; j0 < len; j0 += G * UNR2) {
    uint4 vraw[UNR2];
    float vsc[UNR2];
#pragma unroll
    for (int u = 0; u < UNR2; ++u) {
      const int j = j0 + u * G;
      const bool ok = j < len;
      const uint8_t* src = vc + ((int64_t)j * HD + c * 8) * ES;
      if constexpr (KV8) {
        const uint2 r = ok ? ld_stream8(src) : make_uint2(0, 0);
        vraw[u] = make_uint4(r.x, r.y, 0, 0);
        vsc[u] = ok ? vs[j] : 0.f;
      } else {
        vraw[u] = ok ? ld_stream16(src) : make_uint4(0, 0, 0, 0);
        vsc[u] = 1.f;
      }
    }
#pragma unroll
    for (int u = 0; u < UNR2; ++u) {
      const int j = j0 + u * G;
      if (j >= len) break;
      float vv[8];
      if constexpr (KV8) {
        fp8x4_to_f32(vraw[u].x, vv);
        fp8x4_to_f32(vraw[u].y, vv + 4);
      } else {
        unpack8<DT>(vraw[u], vv);
      }
      float pr[TQ];  // the key's probabilities for all the queries: one broadcast row of LDS
#pragma unroll
      for (int t4 = 0; t4 < TQ / 4; ++t4) {
        const float4 p4 = *(const float4*)(sc + j * TQ + 4 * t4);
        pr[4 * t4] = p4.x; pr[4 * t4 + 1] = p4.y; pr[4 * t4 + 2] = p4.z; pr[4 * t4 + 3] = p4.w;
      }
#pragma unroll
      for (int t = 0; t < TQ; ++t) {
        float pj = pr[t];
        if constexpr (KV8) pj *= vsc[u];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[t][e] = fmaf(pj, vv[e], o[t][e]);
      }
    }
  }
  // key slices of a wave (lanes c, c + OCT, ...) summed by shuffles
#pragma unroll
  for (int o2 = 32; o2 >= OCT; o2 >>= 1)
#pragma unroll
    for (int t = 0; t < TQ; ++t)
#pragma unroll
      for (int e = 0; e < 8; ++e) o[t][e] += __shfl_xor(o[t][e], o2, 64);
  __syncthreads();  // everyone is done reading the probabilities: reuse the buffer for the waves' partials
  float* part = sc;  // [4][TQ][D]
  if (lane < OCT) {
#pragma unroll
    for (int t = 0; t < TQ; ++t) {
      float* dst = part + ((wave * TQ + t) * D + c * 8);
      *(float4*)dst = make_float4(o[t][0], o[t][1], o[t][2], o[t][3]);
      *(float4*)(dst + 4) = make_float4(o[t][4], o[t][5], o[t][6], o[t][7]);
    }
  }
  __syncthreads();
  for (int idx = tid; idx < T * D; idx += 256) {
    const int t = idx / D, d = idx - t * D;
    const float a = (part[(0 * TQ + t) * D + d] + part[(1 * TQ + t) * D + d]) + (part[(2 * TQ + t) * D + d] + part[(3 * TQ + t) * D + d]);
    const float sm = (red_sum[0][t] + red_sum[1][t]) + (red_sum[2][t] + red_sum[3][t]);
    const int64_t row = (int64_t)(b * T + t);
    if (!BEAMS && splits == 1) {
      out[row * HD + (int64_t)h * D + d] = (uint16_t)st16<DT>(sm > 0.f ? a / sm : 0.f);
    } else {
      float* w = ws + ((row * H + h) * wsplits + sp) * (D + 2);
      w[d] = a;
      if (d == 0) {
        w[D] = fmaxf(fmaxf(red_mx[0][t], red_mx[1][t]), fmaxf(red_mx[2][t], red_mx[3][t]));
        w[D + 1] = sm;
      }
    }
  }
}

// ---- beam search on a shared prompt cache (generate(num_beams = n, share_prompt_kv = True)) ----------------------------------------------
// The prompt's K/V rows lie once per prompt where the prefill wrote them (the prefix); a beam owns only the rows of the tokens generated
// so far (the suffix, [rows, G, H*D]), and which row holds key g of beam m's history is the ancestry table anc [rows, G].
// HF `_reorder_cache` on the table: anc_out[m, :gen[m]] = anc_in[beam_idx[m], :gen[m]] and anc_out[m, gen[m]] = m (the row the next
// append writes is the beam's own).  Block per row; gen is read here, never on the host; two buffers that the caller swaps, no atomics.
__global__ __launch_bounds__(256) void beam_ancestry_k(const int32_t* __restrict__ anc_in, int32_t* __restrict__ anc_out,
                                                       const int64_t* __restrict__ beam_idx, const int32_t* __restrict__ gen, int rows, int G) {
  const int m = blockIdx.x;
  const int n = max(0, min(gen[m], G));
  const int64_t src = beam_idx[m];
  if (src >= 0 && src < rows)
    for (int g = threadIdx.x; g < n; g += 256) anc_out[(int64_t)m * G + g] = anc_in[src * G + g];
  if (threadIdx.x == 0 && n < G) anc_out[(int64_t)m * G + n] = m;
}

// Prompt-lookup drafter (transformers PromptLookupCandidateGenerator.get_candidates, no logits processor): one block per row of ids
// [rows, ld].  For n = min(max_ngram, len - 1) .. 1: the EARLIEST window ids[i .. i + n) equal to the last n tokens whose continuation
// ids[i + n .. min(i + n + k, len, max_length)) is not empty; the first n that has one wins.  out [rows, k], out_count [rows] (0: none).
__global__ __launch_bounds__(256) void ngram_draft_k(const int64_t* __restrict__ ids, int64_t ld, int len, int max_ngram, int k,
                                                     int max_length, int64_t* __restrict__ out, int32_t* __restrict__ out_count) {
  __shared__ int best;
  const int row = blockIdx.x, tid = threadIdx.x;
  const int64_t* x = ids + (int64_t)row * ld;
  const int lim = min(len, max_length);  // a continuation starts before this index
  int start = -1;
  if (max_length != len + 1) {  // (one token left: the step that verifies a draft emits one more than it accepts)
    for (int n = min(max_ngram, len - 1); n >= 1; --n) {
      if (tid == 0) best = 0x7fffffff;
      __syncthreads();
      int mine = 0x7fffffff;
      for (int i = tid; i + n < lim; i += 256) {
        bool eq = true;
        for (int e = 0; e < n && eq; ++e) eq = x[i + e] == x[len - n + e];
        if (eq) { mine = i; break; }
      }
      if (mine != 0x7fffffff) atomicMin(&best, mine);
      __syncthreads();
      const int got = best;
      __syncthreads();
      if (got != 0x7fffffff) { start = got + n; break; }
    }
  }
  const int cnt = start < 0 ? 0 : min(start + k, lim) - start;
  if (tid == 0) out_count[row] = cnt;
  for (int i = tid; i < cnt; i += 256) out[(int64_t)row * k + i] = x[start + i];
}

}  // namespace

// A/B switches.  mh_gemv_mfma_min_rows(r): activation-row count from which the MFMA forms are used, all formats and epilogues
// (17 = never, <= 0 = the defaults of the formats); mh_gemv_mfma_pair_min_rows: the paired forms' threshold, 16-bit and fp8 weights
static int g_gemv_ksplit = 1;  // 1-2 rows, N <= 8192: K split over the four waves of a block (A-B switch: mh_gemv_ksplit)
extern "C" void mh_gemv_ksplit(int on) { g_gemv_ksplit = on ? 1 : 0; }
template <class Fmt>
static void gemv_set_mfma_min(int rows, int rows_pair) {
  Fmt::mfma_min = rows > 0 ? rows : Fmt::MFMA_MIN;
  Fmt::mfma_pair_min = rows_pair > 0 ? rows_pair : Fmt::MFMA_PAIR_MIN;
}
extern "C" void mh_gemv_mfma_min_rows(int rows) {
  gemv_set_mfma_min<W16>(rows, rows);
  gemv_set_mfma_min<WFp8>(rows, rows);
  gemv_set_mfma_min<WFp4>(rows, rows);
}
extern "C" void mh_gemv_mfma_pair_min_rows(int rows16, int rows_fp8) {
  gemv_set_mfma_min<W16>(W16::mfma_min, rows16);
  gemv_set_mfma_min<WFp8>(WFp8::mfma_min, rows_fp8);
}

// one projection of the decode step as the entry points hand it to the launchers (W, ldw, wsc: the weights in the launcher's format)
struct GemvArgs {
  const void* x; int64_t ldx; const void* W; int64_t ldw; const void* wsc; void* out; int64_t ldo; const void* resid; int64_t ldr;
  int M, N, K, dt, out_f32, swi_ff;
  const void* norm_w; float eps; RopeAppend ra; void* stream;
};

// the argument checks every format shares; 0 or the error code
template <class Fmt>
static int gemv_check(const GemvArgs& a) {
  if (!a.x || !a.W || (Fmt::SCALED && !a.wsc) || !a.out || a.M <= 0 || a.M > 16 || a.N <= 0 || a.K <= 0 || (a.K % Fmt::EPL) || (a.ldx & 7) ||
      (a.ldw & 7))
    return MH_ERR_ARG;
  if (!aligned16(a.x) || !aligned16(a.W)) return MH_ERR_ARG;
  if (a.dt != MH_BF16 && a.dt != MH_F16) return MH_ERR_DTYPE;
  if (a.norm_w && (a.M > 8 || a.K > 8192 || !aligned16(a.norm_w))) return MH_ERR_ARG;  // fused RMSNorm: row-per-wave form, whole row in LDS
  if (a.ra.tab && (a.swi_ff || (a.N & 1))) return MH_ERR_ARG;
  if ((a.swi_ff || a.ra.tab) && (a.resid || a.out_f32)) return MH_ERR_ARG;
  return MH_OK;
}
// whether a launch has the row count of the format's MFMA form (3+ rows: that form is HBM-bound where the wave form turns VALU-bound)
template <class Fmt>
static bool gemv_mfma_rows(const GemvArgs& a) {
  return !a.norm_w && a.M >= ((a.swi_ff || a.ra.tab) ? Fmt::mfma_pair_min : Fmt::mfma_min);
}

template <class Fmt, int DT, int MM, int ROWS, bool LDSX, bool NORM>
static void gemv_wave_go(const GemvArgs& a) {
  const int cols = a.swi_ff ? ROWS / 2 : ROWS;  // output columns per wave (N counts outputs: gate/up pairs with SwiGLU)
  const size_t lds = NORM ? (size_t)MM * a.K * 2 : LDSX ? (size_t)MM * GEMV_KC * 2 : 0;
  static bool attr = false;
  if (lds && !attr) {
    hipFuncSetAttribute((const void*)gemv_k<Fmt, DT, MM, ROWS, LDSX, NORM>, hipFuncAttributeMaxDynamicSharedMemorySize, MM * 8192 * 2);
    attr = true;
  }
  hipLaunchKernelGGL((gemv_k<Fmt, DT, MM, ROWS, LDSX, NORM>), dim3((a.N + 4 * cols - 1) / (4 * cols)), dim3(256), lds, as_stream(a.stream),
                     (const uint16_t*)a.x, a.ldx, a.W, a.ldw, a.wsc, a.out, a.ldo, (const uint16_t*)a.resid, a.ldr, a.N, a.K, a.out_f32,
                     a.swi_ff, (const uint16_t*)a.norm_w, a.eps, a.ra);
}
template <class Fmt, int DT, int MM>
static void gemv_wave_rows(const GemvArgs& a, int rows) {
#define GO(R_)                                                                                                          \
  do {                                                                                                                  \
    if constexpr (Fmt::has_rows(MM, R_))                                                                                \
      if (rows == R_) {                                                                                                 \
        if (a.norm_w) return gemv_wave_go<Fmt, DT, MM, R_, true, true>(a);                                              \
        return gemv_wave_go<Fmt, DT, MM, R_, (MM >= 3), false>(a); /* 1-2 activation rows: no LDS staging */            \
      }                                                                                                                 \
  } while (0)
  GO(1); GO(2); GO(4);
#undef GO
}
template <class Fmt, int DT, int MM>
static void gemv_ks_go(const GemvArgs& a) {
  hipLaunchKernelGGL((gemv_ks_k<Fmt, DT, MM, 2>), dim3((a.N + 1) / 2), dim3(256), 0, as_stream(a.stream), (const uint16_t*)a.x, a.ldx, a.W, a.ldw,
                     a.wsc, a.out, a.ldo, (const uint16_t*)a.resid, a.ldr, a.N, a.K, a.out_f32);
}
template <class Fmt, int DT>
static int gemv_wave_dt(const GemvArgs& a) {
  if constexpr (Fmt::HAS_KSPLIT) {
    if (g_gemv_ksplit && a.M <= 2 && !a.swi_ff && !a.norm_w && !a.ra.tab && a.N <= 8192 && a.K >= 2048) {  // small N: K split over the block's waves
      if (a.M == 1) gemv_ks_go<Fmt, DT, 1>(a); else gemv_ks_go<Fmt, DT, 2>(a);
      MH_LAUNCH_CHECK();
    }
  }
  const int rows = Fmt::rows(a.M, a.N, a.swi_ff != 0, a.ra.tab != nullptr);
  switch (a.M) {
    case 1: gemv_wave_rows<Fmt, DT, 1>(a, rows); break;
    case 2: gemv_wave_rows<Fmt, DT, 2>(a, rows); break;
    case 3: gemv_wave_rows<Fmt, DT, 3>(a, rows); break;
    case 4: gemv_wave_rows<Fmt, DT, 4>(a, rows); break;
    case 5: gemv_wave_rows<Fmt, DT, 5>(a, rows); break;
    case 6: gemv_wave_rows<Fmt, DT, 6>(a, rows); break;
    case 7: gemv_wave_rows<Fmt, DT, 7>(a, rows); break;
    default: gemv_wave_rows<Fmt, DT, 8>(a, rows); break;
  }
  MH_LAUNCH_CHECK();
}
// the one-wave-per-row form of a checked projection (gemv_check) that did not go to an MFMA form: M <= 8
template <class Fmt>
static int gemv_wave_launch(const GemvArgs& a) {
  if (a.M > 8 || ((a.swi_ff || a.ra.tab) && a.K > Fmt::PAIR_MAX_K)) return MH_ERR_ARG;
  return a.dt == MH_BF16 ? gemv_wave_dt<Fmt, MH_BF16>(a) : gemv_wave_dt<Fmt, MH_F16>(a);
}

static int gemv_impl(const GemvArgs& a) {
  if (const int e = gemv_check<W16>(a)) return e;
  // (the rotary-pair MFMA form needs D/2 to be whole 16-row groups)
  if (gemv_mfma_rows<W16>(a) && (a.K % 32) == 0 && (!a.ra.tab || ((a.ra.D >> 1) % 16 == 0 && a.N == 3 * a.ra.H * a.ra.D))) {
    auto mfma = a.dt == MH_BF16 ? launch_gemv_mfma<MH_BF16, false> : launch_gemv_mfma<MH_F16, false>;
    return mfma(a.x, a.ldx, a.W, a.ldw, nullptr, a.out, a.ldo, a.resid, a.ldr, a.M, a.N, a.K, a.out_f32, a.swi_ff, a.ra, as_stream(a.stream));
  }
  return gemv_wave_launch<W16>(a);
}

extern "C" int mh_gemv(const void* x, int64_t ldx, const void* W, int64_t ldw, void* out, int64_t ldo, const void* resid,
                       int64_t ldr, int M, int N, int K, int dt, int out_f32, void* stream) {
  return gemv_impl({x, ldx, W, ldw, nullptr, out, ldo, resid, ldr, M, N, K, dt, out_f32, 0, nullptr, 0.f, RopeAppend{}, stream});
}
// act[M, ff] = silu(x Wg^T) * (x Wu^T) with Wgu = [Wg; Wu] [2 ff, K] (HF LlamaMLP gate / up of the decode step): one launch, the
// gate|up projection never reaches memory (gate / up are rounded to 16 bits before the activation, as the two launches do).  M <= 16 rows (MFMA form from 3 rows on).
extern "C" int mh_gemv_swiglu(const void* x, int64_t ldx, const void* Wgu, int64_t ldw, void* act, int64_t ldo, int M, int ff, int K, int dt,
                              void* stream) {
  if (ff <= 0) return MH_ERR_ARG;
  return gemv_impl({x, ldx, Wgu, ldw, nullptr, act, ldo, nullptr, 0, M, ff, K, dt, 0, ff, nullptr, 0.f, RopeAppend{}, stream});
}
// The same two projections with the RMSNorm that precedes them (HF LlamaDecoderLayer: input_layernorm -> q|k|v, post_attention_layernorm ->
// gate|up) applied by the GEMV blocks themselves: y = rmsnorm(x; norm_w, eps) W^T, and (ff > 0) act = silu(.) * (.) of the gate|up rows.
// Equal to mh_rmsnorm_fwd + mh_gemv (+ mh_swiglu_fwd) bit for bit in the projection.  M <= 8, K <= 8192.
extern "C" int mh_gemv_norm(const void* x, int64_t ldx, const void* norm_w, float eps, const void* W, int64_t ldw, void* out, int64_t ldo, int M, int N,
                            int K, int ff, int dt, void* stream) {
  if (!norm_w || M > 8 || ff < 0) return MH_ERR_ARG;
  return gemv_impl({x, ldx, W, ldw, nullptr, out, ldo, nullptr, 0, M, ff > 0 ? ff : N, K, dt, 0, ff, norm_w, eps, RopeAppend{}, stream});
}

// the one-token append of either cache format (ks, vs: the fp8 cache's scales); dt is MH_BF16 or MH_F16, checked by the fronts
template <bool KV8>
static int launch_rope_append(void* qkv, const float* cos_sin, const int32_t* pos, const int32_t* rope_pos, void* kc, void* vc, float* ks,
                              float* vs, int B, int H, int D, int Smax, int dt, void* stream) {
  const int64_t total = (int64_t)B * H * (D / 16);
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  if (dt == MH_BF16)
    hipLaunchKernelGGL((rope_append_k<MH_BF16, KV8>), grid, block, 0, as_stream(stream), (uint16_t*)qkv, (const float2*)cos_sin, pos, rope_pos,
                       kc, vc, ks, vs, B, H, D, Smax);
  else
    hipLaunchKernelGGL((rope_append_k<MH_F16, KV8>), grid, block, 0, as_stream(stream), (uint16_t*)qkv, (const float2*)cos_sin, pos, rope_pos,
                       kc, vc, ks, vs, B, H, D, Smax);
  MH_LAUNCH_CHECK();
}

extern "C" int mh_decode_rope_append(void* qkv, const float* cos_sin, const int32_t* pos, const int32_t* rope_pos, void* kcache, void* vcache,
                                     int B, int H, int D, int Smax, int dt, void* stream) {
  if (!rope_pos) rope_pos = pos;
  if (!qkv || !cos_sin || !pos || !kcache || !vcache || B <= 0 || H <= 0 || (D & 15) || Smax <= 0) return MH_ERR_ARG;
  if (dt != MH_BF16 && dt != MH_F16) return MH_ERR_DTYPE;
  return launch_rope_append<false>(qkv, cos_sin, pos, rope_pos, kcache, vcache, nullptr, nullptr, B, H, D, Smax, dt, stream);
}

// mh_decode_rope_append on the fp8 KV cache: qkv rotated in place exactly as above; the rotated k row and the v row are quantised (one
// power-of-two scale per head) into k8 / v8 [B, Smax, H*D] at row pos[b], their scales into kscale / vscale [B, H, Smax].
extern "C" int mh_decode_rope_append_kv8(void* qkv, const float* cos_sin, const int32_t* pos, const int32_t* rope_pos, void* k8, void* v8,
                                         float* kscale, float* vscale, int B, int H, int D, int Smax, int dt, void* stream) {
  if (!rope_pos) rope_pos = pos;
  if (!qkv || !cos_sin || !pos || !k8 || !v8 || !kscale || !vscale || B <= 0 || H <= 0 || Smax <= 0) return MH_ERR_ARG;
  if (!aligned16(qkv) || (((uintptr_t)k8 | (uintptr_t)v8) & 7u)) return MH_ERR_ARG;  // 16-byte row pieces in, 8-byte e4m3 stores out
  if (D != 128 && D != 64) return MH_ERR_SHAPE;
  if (dt != MH_BF16 && dt != MH_F16) return MH_ERR_DTYPE;
  return launch_rope_append<true>(qkv, cos_sin, pos, rope_pos, k8, v8, kscale, vscale, B, H, D, Smax, dt, stream);
}

// prefill of the fp8 KV cache: x [B*S, H, D] (row stride ldx elements; the k or the v section of the fused q|k|v buffer) -> c8 rows
// [b, s < S] of [B, Smax, H*D] and scales [b, h, s] of [B, H, Smax]; rows >= S are not written.
extern "C" int mh_kv8_fill(const void* x, int64_t ldx, void* c8, float* scales, int B, int S, int H, int D, int Smax, int dt, void* stream) {
  if (!x || !c8 || !scales || B <= 0 || S <= 0 || H <= 0 || S > Smax || (ldx & 7) || ldx < (int64_t)H * D || !aligned16(x)) return MH_ERR_ARG;
  if (((uintptr_t)c8) & 7u) return MH_ERR_ARG;  // every lane stores 8 e4m3 bytes at once
  if (D != 128 && D != 64) return MH_ERR_SHAPE;
  if (dt != MH_BF16 && dt != MH_F16) return MH_ERR_DTYPE;
  const int64_t total = (int64_t)B * S * H * (D / 8);
  if ((total + 255) / 256 > 0x7fffffff) return MH_ERR_SHAPE;
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
#define GO(DT_, D_) \
  hipLaunchKernelGGL((kv8_fill_k<DT_, D_>), grid, block, 0, as_stream(stream), (const uint16_t*)x, ldx, (uint8_t*)c8, scales, B, S, H, Smax)
  if (dt == MH_BF16) { if (D == 128) GO(MH_BF16, 128); else GO(MH_BF16, 64); }
  else { if (D == 128) GO(MH_F16, 128); else GO(MH_F16, 64); }
#undef GO
  MH_LAUNCH_CHECK();
}

extern "C" int mh_attn_decode_splits(int B, int H, int Smax) {
  int s = (1024 + B * H - 1) / (B * H);
  const int by_len = (Smax + 127) / 128;  // >= 128 keys per split
  if (s > by_len) s = by_len;
  if (s > 32) s = 32;
  return s < 1 ? 1 : s;
}

template <class Fmt, int DT, int D>
static void launch_attn_decode(const void* q, int64_t ldq, const void* kc, const void* vc, const float* ks, const float* vs, void* out,
                               const int32_t* lens, int B, int H, int Smax, int splits, int chunk, size_t lds, float* ws, hipStream_t st) {
  static bool attr = false;
  if (!attr) {
    hipFuncSetAttribute((const void*)attn_decode_k<Fmt, DenseRows, DT, D>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
    attr = true;
  }
  const float scale_log2 = 1.4426950408889634f / sqrtf((float)D);
  hipLaunchKernelGGL((attn_decode_k<Fmt, DenseRows, DT, D>), dim3(B * H * splits), dim3(256), lds, st, (const uint16_t*)q, ldq, kc, vc, ks, vs,
                     (uint16_t*)out, lens, (const int32_t*)nullptr, B, H, Smax, scale_log2, splits, chunk, ws, 0, splits);
  if (splits > 1)
    hipLaunchKernelGGL((attn_decode_combine_k<DT, D>), dim3(B * H), dim3(D), 0, st, (const float*)ws, (uint16_t*)out, H, splits);
}

// the split plan (mh_attn_decode_splits; ws == NULL: one block per (b, h)), a block's LDS and the launches of mh_attn_decode / _kv8, which
// check their own arguments: D is 64 or 128 and dt MH_BF16 or MH_F16 here
template <bool KV8>
static int attn_decode_impl(const void* q, int64_t ldq, const void* kc, const void* vc, const float* ks, const float* vs, void* out,
                            const int32_t* lens, int B, int H, int D, int Smax, float* ws, int dt, void* stream) {
  const int splits = ws ? mh_attn_decode_splits(B, H, Smax) : 1;
  const int chunk = (Smax + splits - 1) / splits;
  const int G = 256 / (D / 8);
  const size_t lds = sizeof(float) * (size_t)((chunk > G * D) ? chunk : G * D);
  if (lds > 150 * 1024) return MH_ERR_SHAPE;  // <= 38400 keys per split
  hipStream_t st = as_stream(stream);
#define GO(DT_, D_) launch_attn_decode<KVFmt<KV8>, DT_, D_>(q, ldq, kc, vc, ks, vs, out, lens, B, H, Smax, splits, chunk, lds, ws, st)
  if (dt == MH_BF16) { if (D == 128) GO(MH_BF16, 128); else GO(MH_BF16, 64); }
  else { if (D == 128) GO(MH_F16, 128); else GO(MH_F16, 64); }
#undef GO
  MH_LAUNCH_CHECK();
}

extern "C" int mh_attn_decode(const void* q, int64_t ldq, const void* kcache, const void* vcache, void* out, const int32_t* lens,
                              int B, int H, int D, int Smax, float* ws, int dt, void* stream) {
  if (!q || !kcache || !vcache || !out || !lens || B <= 0 || H <= 0 || Smax <= 0 || (ldq & 7)) return MH_ERR_ARG;
  if (D != 128 && D != 64) return MH_ERR_SHAPE;
  if (dt != MH_BF16 && dt != MH_F16) return MH_ERR_DTYPE;
  return attn_decode_impl<false>(q, ldq, kcache, vcache, nullptr, nullptr, out, lens, B, H, D, Smax, ws, dt, stream);
}

// mh_attn_decode on the fp8 KV cache (k8, v8 + kscale, vscale): same semantics, workspace and split plan
extern "C" int mh_attn_decode_kv8(const void* q, int64_t ldq, const void* k8, const void* v8, const float* kscale, const float* vscale, void* out,
                                  const int32_t* lens, int B, int H, int D, int Smax, float* ws, int dt, void* stream) {
  if (!q || !k8 || !v8 || !kscale || !vscale || !out || !lens || B <= 0 || H <= 0 || Smax <= 0 || (ldq & 7)) return MH_ERR_ARG;
  if (((uintptr_t)k8 | (uintptr_t)v8) & 7u) return MH_ERR_ARG;  // the cache is read 8 bytes at a time
  if (D != 128 && D != 64) return MH_ERR_SHAPE;
  if (dt != MH_BF16 && dt != MH_F16) return MH_ERR_DTYPE;
  return attn_decode_impl<true>(q, ldq, k8, v8, kscale, vscale, out, lens, B, H, D, Smax, ws, dt, stream);
}

// ---- T new tokens per sequence (the verify step of prompt-lookup decoding) --------------------------------------------------------------
template <int DT, bool KV8>
static void launch_rope_append_multi(void* qkv, const float* cos_sin, const int32_t* pos, const int32_t* rope_pos, void* kc, void* vc, float* ks,
                                     float* vs, int B, int T, int H, int D, int Smax, void* stream) {
  const int64_t total = (int64_t)B * T * H * (D / 16);
  hipLaunchKernelGGL((rope_append_multi_k<DT, KV8>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), (uint16_t*)qkv,
                     (const float2*)cos_sin, pos, rope_pos, kc, vc, ks, vs, B, T, H, D, Smax);
}

extern "C" int mh_decode_rope_append_multi(void* qkv, const float* cos_sin, const int32_t* pos, const int32_t* rope_pos, void* kcache,
                                           void* vcache, int B, int T, int H, int D, int Smax, int dt, void* stream) {
  if (!rope_pos) rope_pos = pos;
  if (!qkv || !cos_sin || !pos || !kcache || !vcache || B <= 0 || T < 1 || T > 16 || H <= 0 || D <= 0 || (D & 15) || Smax <= 0) return MH_ERR_ARG;
  if (!aligned16(qkv) || !aligned16(kcache) || !aligned16(vcache)) return MH_ERR_ARG;
  if (dt != MH_BF16 && dt != MH_F16) return MH_ERR_DTYPE;
  if (dt == MH_BF16) launch_rope_append_multi<MH_BF16, false>(qkv, cos_sin, pos, rope_pos, kcache, vcache, nullptr, nullptr, B, T, H, D, Smax, stream);
  else launch_rope_append_multi<MH_F16, false>(qkv, cos_sin, pos, rope_pos, kcache, vcache, nullptr, nullptr, B, T, H, D, Smax, stream);
  MH_LAUNCH_CHECK();
}

extern "C" int mh_decode_rope_append_multi_kv8(void* qkv, const float* cos_sin, const int32_t* pos, const int32_t* rope_pos, void* k8, void* v8,
                                               float* kscale, float* vscale, int B, int T, int H, int D, int Smax, int dt, void* stream) {
  if (!rope_pos) rope_pos = pos;
  if (!qkv || !cos_sin || !pos || !k8 || !v8 || !kscale || !vscale || B <= 0 || T < 1 || T > 16 || H <= 0 || Smax <= 0) return MH_ERR_ARG;
  if (!aligned16(qkv) || (((uintptr_t)k8 | (uintptr_t)v8) & 7u)) return MH_ERR_ARG;  // 16-byte row pieces in, 8-byte e4m3 stores out
  if (D != 128 && D != 64) return MH_ERR_SHAPE;
  if (dt != MH_BF16 && dt != MH_F16) return MH_ERR_DTYPE;
  if (dt == MH_BF16) launch_rope_append_multi<MH_BF16, true>(qkv, cos_sin, pos, rope_pos, k8, v8, kscale, vscale, B, T, H, D, Smax, stream);
  else launch_rope_append_multi<MH_F16, true>(qkv, cos_sin, pos, rope_pos, k8, v8, kscale, vscale, B, T, H, D, Smax, stream);
  MH_LAUNCH_CHECK();
}

// queries a block of attn_decode_multi_k is compiled for (its score rows in LDS are this wide)
static int attn_multi_tq(int T) { return T <= 4 ? 4 : (T <= 8 ? 8 : 16); }
constexpr int ATTN_MULTI_LDS_MAX = 150 * 1024;  // what mh_attn_decode requests at most
// score bytes per block the split plan aims for.  Up to 8 queries (<= 133 VGPRs) this leaves LDS room for two blocks per CU; the 16-query form
// holds 16 x 8 accumulators per lane (256 VGPRs + AGPRs, one wave per SIMD: one block per CU whatever its LDS), where the aim only keeps a
// block's key range short - profiles/decode_verify_bench.txt times it as it is.
constexpr int ATTN_MULTI_LDS_AIM = 64 * 1024;

// mh_attn_decode_splits, then more splits (up to the merge kernel's 32) until a split's T x chunk fp32 scores fit 64 KiB of LDS
extern "C" int mh_attn_decode_multi_splits(int B, int T, int H, int Smax) {
  if (B <= 0 || T < 1 || T > 16 || H <= 0 || Smax <= 0) return 0;
  int s = mh_attn_decode_splits(B, H, Smax);  // (a block serves all T queries of its (b, h): the block count is the one-query plan's)
  const int64_t tq = attn_multi_tq(T);
  while (s < 32 && tq * ((Smax + s - 1) / s) * 4 > ATTN_MULTI_LDS_AIM) ++s;
  return s;
}

template <int DT, int D, int TQ, bool KV8>
static void launch_attn_multi(const void* q, int64_t ldq, const void* kc, const void* vc, const float* ks, const float* vs, void* out,
                              const int32_t* lens, int B, int T, int H, int Smax, int splits, int chunk, size_t lds, float* ws, hipStream_t st) {
  static bool attr = false;
  if (!attr) {
    hipFuncSetAttribute((const void*)attn_decode_multi_k<DT, D, TQ, KV8>, hipFuncAttributeMaxDynamicSharedMemorySize, ATTN_MULTI_LDS_MAX);
    attr = true;
  }
  const float scale_log2 = 1.4426950408889634f / sqrtf((float)D);
  hipLaunchKernelGGL((attn_decode_multi_k<DT, D, TQ, KV8>), dim3(B * H * splits), dim3(256), lds, st, (const uint16_t*)q, ldq, kc, vc, ks, vs,
                     (uint16_t*)out, lens, T, H, Smax, scale_log2, splits, chunk, ws, splits);
  if (splits > 1)
    hipLaunchKernelGGL((attn_decode_combine_k<DT, D>), dim3(B * T * H), dim3(D), 0, st, (const float*)ws, (uint16_t*)out, H, splits);
}

template <bool KV8>
static int attn_multi_impl(const void* q, int64_t ldq, const void* kc, const void* vc, const float* ks, const float* vs, void* out,
                           const int32_t* lens, int B, int T, int H, int D, int Smax, float* ws, int dt, void* stream) {
  if (!q || !kc || !vc || !out || !lens || B <= 0 || T < 1 || T > 16 || H <= 0 || Smax <= 0 || (ldq & 7) || !aligned16(q)) return MH_ERR_ARG;
  if (KV8 && (!ks || !vs || (((uintptr_t)kc | (uintptr_t)vc) & 7u))) return MH_ERR_ARG;  // the fp8 cache is read 8 bytes at a time
  if (!KV8 && (!aligned16(kc) || !aligned16(vc))) return MH_ERR_ARG;
  if (D != 128 && D != 64) return MH_ERR_SHAPE;
  if (dt != MH_BF16 && dt != MH_F16) return MH_ERR_DTYPE;
  const int tq = attn_multi_tq(T);
  const int splits = ws ? mh_attn_decode_multi_splits(B, T, H, Smax) : 1;
  const int chunk = (Smax + splits - 1) / splits;
  const int64_t need = (int64_t)sizeof(float) * tq * (chunk > 4 * D ? chunk : 4 * D);  // scores [chunk][tq], then the four waves' [tq][D] partials
  if (need > ATTN_MULTI_LDS_MAX) return MH_ERR_SHAPE;
  if ((int64_t)B * T * H * splits > 0x7fffffff / (D + 2)) return MH_ERR_SHAPE;
  hipStream_t st = as_stream(stream);
#define GO(DT_, D_, TQ_) launch_attn_multi<DT_, D_, TQ_, KV8>(q, ldq, kc, vc, ks, vs, out, lens, B, T, H, Smax, splits, chunk, (size_t)need, ws, st)
#define GOT(DT_, D_) do { if (tq == 4) GO(DT_, D_, 4); else if (tq == 8) GO(DT_, D_, 8); else GO(DT_, D_, 16); } while (0)
  if (dt == MH_BF16) { if (D == 128) GOT(MH_BF16, 128); else GOT(MH_BF16, 64); }
  else { if (D == 128) GOT(MH_F16, 128); else GOT(MH_F16, 64); }
#undef GOT
#undef GO
  MH_LAUNCH_CHECK();
}

extern "C" int mh_attn_decode_multi(const void* q, int64_t ldq, const void* kcache, const void* vcache, void* out, const int32_t* lens, int B,
                                    int T, int H, int D, int Smax, float* ws, int dt, void* stream) {
  return attn_multi_impl<false>(q, ldq, kcache, vcache, nullptr, nullptr, out, lens, B, T, H, D, Smax, ws, dt, stream);
}

extern "C" int mh_attn_decode_multi_kv8(const void* q, int64_t ldq, const void* k8, const void* v8, const float* kscale, const float* vscale,
                                        void* out, const int32_t* lens, int B, int T, int H, int D, int Smax, float* ws, int dt, void* stream) {
  return attn_multi_impl<true>(q, ldq, k8, v8, kscale, vscale, out, lens, B, T, H, D, Smax, ws, dt, stream);
}

// ---- n new query rows per sequence over a kept cache (engine.extend: a prompt tail on a session's KV cache) ------------------------------
// mh_attn_extend / _kv8: q rows m = b*n + t, query t sees keys [0, min(lens[b] + t, Smax)) - mh_attn_decode_multi's convention for any n.
// Flash-style: block per (b, h, tile of EXT_TQ = 64 queries), wave w owns queries 16 w .. 16 w + 15 of the tile; key tiles of EXT_TK = 32
// are streamed with an online softmax, so nothing in LDS or in the launch depends on Smax.  Per key tile and wave:
//   S^T = K Q^T  two 16-key sub-tiles: a lane loads 16 B (fp8 cache: 8 B, converted exactly) of key row (l & 15) straight into the A
//                operand, the wave's 16 query rows are the B operand (registers, loaded once); lane l holds keys 4 (l >> 4) + r of both
//                sub-tiles for query l & 15, so max and sum of a query are 8 values in a lane and two shuffles (xor 16, 32).
//   O^T += V^T P^T  the MFMA's k index is free to be permuted as long as both operands agree: k slot 8 g + e stands for key 4 g + e of
//                sub-tile 0 (e < 4) and key 4 g + e - 4 of sub-tile 1 (e >= 4), which makes the B operand the lane's own 8 probabilities
//                (rounded to the 16-bit type like the prefill kernels' P) - no cross-lane movement - and the output tile lands as
//                (channel 4 g + r, query l & 15): the running max, sum and rescale of a query live in the lanes that hold its outputs.
//                The A operand is V transposed: the block stages the tile once in LDS as vt[channel][k slot] (a thread loads 16 B of two
//                consecutive keys and writes 8 dwords, two slots each), and a lane reads one 16-byte row piece per 16-channel block.
//   LDS banks    a vt row is 32 slots + 8 of padding = 80 B: the 16 lanes of a read phase start at 20-dword steps, which visit all 64
//                banks once (conflict-free); the staging writes of a wave hit 16 distinct dwords per row and rows 8 channels apart lie 32
//                banks apart, a 2-way conflict on 8 dword writes per thread and tile (rows must stay 16-byte aligned, so no stride fixes it).
//   fp8 cache    the key scale multiplies the fp32 score, once per key and query like the neighbours; the value scale is applied once per
//                key when the tile is staged (e4m3 * 2^e is exact in the 16-bit type), because P is a 16-bit MFMA operand here and
//                fp16 probabilities cannot carry a 2^-13 scale.
// Keys at or above the block's last horizon are never loaded (zeros are staged instead); a wave skips the tiles above its own last query's
// horizon (it still takes part in the staging).  Split-KV is not done: n <= 16 on a long cache runs B * H blocks with one busy wave each.
constexpr int EXT_TQ = 64, EXT_TK = 32, EXT_VLD = 40;  // queries per block, keys per tile, 16-bit elements per vt row

//
// BR (mh_attn_extend_branches / _kv8): the n query rows are the packed rows of several continuations of ONE sequence whose cache holds P
// prompt rows; row t sits in cache row P + t, `lens` is seg_start (the packed index of the first row of t's own continuation, monotone)
// and query t sees the keys [0, P) and [P + seg_start[t], P + t].  The horizon has two parts, nothing else differs: key tiles stay
// aligned to multiples of EXT_TK from row 0, so the tile that holds row P carries prompt keys (seen by every query) and continuation keys
// (seen by segment) and the per-element mask tells them apart; a block steps from its last prompt tile to the tile of P + seg_start of
// its first query (its minimum, seg_start being monotone), a wave skips the continuation tiles below P + seg_start of its own first query.
template <int DT, int D, bool KV8, bool BR = false>
__global__ __launch_bounds__(256) void attn_extend_k(const uint16_t* __restrict__ q, int64_t ldq, const void* __restrict__ kc_,
                                                     const void* __restrict__ vc_, const float* __restrict__ ks, const float* __restrict__ vs,
                                                     uint16_t* __restrict__ out, const int32_t* __restrict__ lens, int n, int H, int Smax,
                                                     int nqt, float scale_log2, int P) {
  __shared__ __attribute__((aligned(16))) uint16_t vt[D * EXT_VLD];
  constexpr int ES = KV8 ? 1 : 2;  // bytes per cache element
  constexpr int KK = D / 32;       // MFMA k steps of a score tile
  constexpr int NDB = D / 16;      // 16-channel output blocks
  constexpr int OCT = D / 8;       // 8-channel pieces of a value row
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int jq = lane & 15, g = lane >> 4;
  const int qt = blockIdx.x % nqt, h = (blockIdx.x / nqt) % H, b = blockIdx.x / (nqt * H);
  const int len0 = BR ? P + 1 : max(0, min(lens[b], Smax));  // (BR: query t's own key is row P + t)
  const int q0 = qt * EXT_TQ, w0 = q0 + wave * 16;
  const int kend = min(len0 + min(q0 + EXT_TQ, n) - 1, Smax);         // keys the block's last query sees
  const int wend = w0 < n ? min(len0 + min(w0 + 16, n) - 1, Smax) : 0;  // keys the wave's last query sees
  const int t = w0 + jq;                                               // this lane's query
  const int lim = t < n ? min(len0 + t, Smax) : 0;
  // BR: first continuation row the block / the wave / this lane's query sees (queries at or beyond n: lim = 0 hides everything)
  const int blo = BR ? P + lens[q0] : 0, wlo = BR ? P + lens[min(w0, n - 1)] : 0, lo = BR ? P + lens[min(t, n - 1)] : 0;
  auto sees = [&](int j) { return j < lim && (!BR || j < P || j >= lo); };  // key row j is visible to this lane's query
  const int64_t HD = (int64_t)H * D;
  const uint8_t* kc = (const uint8_t*)kc_ + ((int64_t)b * Smax * HD + (int64_t)h * D) * ES;
  const uint8_t* vc = (const uint8_t*)vc_ + ((int64_t)b * Smax * HD + (int64_t)h * D) * ES;
  if constexpr (KV8) {
    ks += ((int64_t)b * H + h) * Smax;
    vs += ((int64_t)b * H + h) * Smax;
  }
  uint4 qf[KK];
#pragma unroll
  for (int kk = 0; kk < KK; ++kk)
    qf[kk] = t < n ? *(const uint4*)(q + ((int64_t)b * n + t) * ldq + (int64_t)h * D + kk * 32 + g * 8) : make_uint4(0, 0, 0, 0);
  // staging item of this thread: key pair vkp of the tile (keys 2 vkp, 2 vkp + 1), channels 8 vc8 .. 8 vc8 + 7 (D = 64: waves 0 and 1 stage)
  const int vkp = lane >> 2, vc8 = wave * 4 + (lane & 3);
  const bool vstage = vc8 < OCT;
  const int vslot = 8 * ((vkp & 7) >> 1) + 4 * (vkp >> 3) + 2 * (vkp & 1);  // k slot of key 2 vkp; key 2 vkp + 1 is the next slot
  f32x4_t acc[NDB];
#pragma unroll
  for (int db = 0; db < NDB; ++db) acc[db] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float m = -1e30f, l = 0.f;
  for (int j0 = 0; j0 < kend; j0 += EXT_TK) {
    if constexpr (BR) {  // (block-uniform) tiles of other continuations' rows only: on to the tile that holds the block's first row
      if (j0 >= P && j0 + EXT_TK <= blo) {
        j0 = (blo & ~(EXT_TK - 1)) - EXT_TK;
        continue;
      }
    }
    uint4 vr[2];
    float vsc[2] = {1.f, 1.f};
    if (vstage) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int j = j0 + 2 * vkp + u;
        const bool ok = j < kend;
        const uint8_t* src = vc + ((int64_t)j * HD + vc8 * 8) * ES;
        if constexpr (KV8) {
          const uint2 r = ok ? *(const uint2*)src : make_uint2(0, 0);
          vr[u] = make_uint4(r.x, r.y, 0, 0);
          vsc[u] = ok ? vs[j] : 0.f;
        } else {
          vr[u] = ok ? *(const uint4*)src : make_uint4(0, 0, 0, 0);
        }
      }
    }
    const bool active = j0 < wend && (!BR || j0 < P || j0 + EXT_TK > wlo);  // (wave-uniform)
    float alpha = 1.f;
    uint4 pb = make_uint4(0, 0, 0, 0);
    if (active) {
      uint4 kr[2][KK];
      float ksc[2][4];
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
        const int j = j0 + sub * 16 + jq;
        const bool ok = j < kend;
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
          const uint8_t* src = kc + ((int64_t)j * HD + kk * 32 + g * 8) * ES;
          if constexpr (KV8) {
            const uint2 r = ok ? *(const uint2*)src : make_uint2(0, 0);
            kr[sub][kk] = make_uint4(r.x, r.y, 0, 0);
          } else {
            kr[sub][kk] = ok ? *(const uint4*)src : make_uint4(0, 0, 0, 0);
          }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          ksc[sub][r] = 1.f;
          if constexpr (KV8) {
            const int jr = j0 + sub * 16 + 4 * g + r;
            ksc[sub][r] = jr < kend ? ks[jr] : 0.f;
          }
        }
      }
      float s[2][4];
      float tm = -1e30f;
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
        f32x4_t s4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
          uint4 a = kr[sub][kk];
          if constexpr (KV8) {
            const uint32_t lo = a.x, hi = a.y;
            fp8x4_to_pk16<DT>(lo, a.x, a.y);
            fp8x4_to_pk16<DT>(hi, a.z, a.w);
          }
          s4 = mfma16<DT>(a, qf[kk], s4);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          s[sub][r] = KV8 ? s4[r] * ksc[sub][r] * scale_log2 : s4[r] * scale_log2;
          if (sees(j0 + sub * 16 + 4 * g + r)) tm = fmaxf(tm, s[sub][r]);
        }
      }
      tm = fmaxf(tm, __shfl_xor(tm, 16, 64));
      tm = fmaxf(tm, __shfl_xor(tm, 32, 64));
      const float mn = fmaxf(m, tm);
      alpha = fast_exp2(m - mn);  // (nothing seen yet: m = mn = -1e30, alpha = 1 on zeros)
      m = mn;
      float p[2][4], psum = 0.f;
#pragma unroll
      for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          p[sub][r] = sees(j0 + sub * 16 + 4 * g + r) ? fast_exp2(s[sub][r] - mn) : 0.f;
          psum += p[sub][r];
        }
      l = fmaf(l, alpha, psum);  // (this lane's four keys per sub-tile; the four lanes of a query are summed at the end)
      pb = make_uint4(pack2<DT>(p[0][0], p[0][1]), pack2<DT>(p[0][2], p[0][3]), pack2<DT>(p[1][0], p[1][1]), pack2<DT>(p[1][2], p[1][3]));
    }
    __syncthreads();  // the previous tile's vt has been read by every wave
    if (vstage) {
      uint32_t e0[8], e1[8];  // the 8 channels of key 2 vkp and of key 2 vkp + 1 as 16-bit patterns
      if constexpr (KV8) {
        float f0[8], f1[8];
        fp8x4_to_f32(vr[0].x, f0); fp8x4_to_f32(vr[0].y, f0 + 4);
        fp8x4_to_f32(vr[1].x, f1); fp8x4_to_f32(vr[1].y, f1 + 4);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          e0[i] = st16<DT>(f0[i] * vsc[0]) & 0xffffu;
          e1[i] = st16<DT>(f1[i] * vsc[1]) & 0xffffu;
        }
      } else {
        const uint32_t w0_[4] = {vr[0].x, vr[0].y, vr[0].z, vr[0].w}, w1_[4] = {vr[1].x, vr[1].y, vr[1].z, vr[1].w};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          e0[i] = (w0_[i >> 1] >> (16 * (i & 1))) & 0xffffu;
          e1[i] = (w1_[i >> 1] >> (16 * (i & 1))) & 0xffffu;
        }
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) *(uint32_t*)(vt + (vc8 * 8 + i) * EXT_VLD + vslot) = e0[i] | (e1[i] << 16);
    }
    __syncthreads();
    if (active) {
#pragma unroll
      for (int db = 0; db < NDB; ++db) {
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[db][r] *= alpha;
        const uint4 a = *(const uint4*)(vt + (db * 16 + jq) * EXT_VLD + g * 8);
        acc[db] = mfma16<DT>(a, pb, acc[db]);
      }
    }
  }
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  if (t < n) {
    const float inv = l > 0.f ? 1.0f / l : 0.f;
    uint16_t* dst = out + ((int64_t)b * n + t) * HD + (int64_t)h * D + 4 * g;
#pragma unroll
    for (int db = 0; db < NDB; ++db)
      *(uint2*)(dst + db * 16) = make_uint2(pack2<DT>(acc[db][0] * inv, acc[db][1] * inv), pack2<DT>(acc[db][2] * inv, acc[db][3] * inv));
  }
}

template <bool KV8>
static int attn_extend_impl(const void* q, int64_t ldq, const void* kc, const void* vc, const float* ks, const float* vs, void* out,
                            const int32_t* lens, int B, int n, int H, int D, int Smax, int dt, void* stream) {
  if (!q || !kc || !vc || !out || !lens || B <= 0 || n < 1 || H <= 0 || Smax <= 0 || (ldq & 7) || !aligned16(q) || !aligned16(out)) return MH_ERR_ARG;
  if (KV8 && (!ks || !vs || (((uintptr_t)kc | (uintptr_t)vc) & 7u))) return MH_ERR_ARG;  // the fp8 cache is read 8 bytes at a time
  if (!KV8 && (!aligned16(kc) || !aligned16(vc))) return MH_ERR_ARG;
  if ((int64_t)Smax + n > 0x7fffffff) return MH_ERR_ARG;  // lens[b] + t is an int
  if (D != 128 && D != 64) return MH_ERR_SHAPE;
  if (dt != MH_BF16 && dt != MH_F16) return MH_ERR_DTYPE;
  const int nqt = (n + EXT_TQ - 1) / EXT_TQ;
  if ((int64_t)B * H * nqt > 0x7fffffff) return MH_ERR_SHAPE;
  const float scale_log2 = 1.4426950408889634f / sqrtf((float)D);
  const dim3 grid((unsigned)(B * H * nqt)), block(256);
#define GO(DT_, D_)                                                                                                                    \
  hipLaunchKernelGGL((attn_extend_k<DT_, D_, KV8>), grid, block, 0, as_stream(stream), (const uint16_t*)q, ldq, kc, vc, ks, vs, (uint16_t*)out, \
                     lens, n, H, Smax, nqt, scale_log2, 0)
  if (dt == MH_BF16) { if (D == 128) GO(MH_BF16, 128); else GO(MH_BF16, 64); }
  else { if (D == 128) GO(MH_F16, 128); else GO(MH_F16, 64); }
#undef GO
  MH_LAUNCH_CHECK();
}

template <bool KV8>
static int attn_branches_impl(const void* q, int64_t ldq, const void* kc, const void* vc, const float* ks, const float* vs, void* out,
                              const int32_t* seg_start, int P, int R, int H, int D, int Smax, int dt, void* stream) {
  if (!q || !kc || !vc || !out || !seg_start || H <= 0 || Smax <= 0 || (ldq & 7) || !aligned16(q) || !aligned16(out)) return MH_ERR_ARG;
  if (P < 0 || R < 1 || (int64_t)P + R > Smax) return MH_ERR_ARG;  // every row the kernel reads, [0, P + R), lies in the cache
  if (KV8 && (!ks || !vs || (((uintptr_t)kc | (uintptr_t)vc) & 7u))) return MH_ERR_ARG;
  if (!KV8 && (!aligned16(kc) || !aligned16(vc))) return MH_ERR_ARG;
  if (D != 128 && D != 64) return MH_ERR_SHAPE;
  if (dt != MH_BF16 && dt != MH_F16) return MH_ERR_DTYPE;
  const int nqt = (R + EXT_TQ - 1) / EXT_TQ;
  if ((int64_t)H * nqt > 0x7fffffff) return MH_ERR_SHAPE;
  const float scale_log2 = 1.4426950408889634f / sqrtf((float)D);
  const dim3 grid((unsigned)(H * nqt)), block(256);
#define GO(DT_, D_)                                                                                                                    \
  hipLaunchKernelGGL((attn_extend_k<DT_, D_, KV8, true>), grid, block, 0, as_stream(stream), (const uint16_t*)q, ldq, kc, vc, ks, vs,   \
                     (uint16_t*)out, seg_start, R, H, Smax, nqt, scale_log2, P)
  if (dt == MH_BF16) { if (D == 128) GO(MH_BF16, 128); else GO(MH_BF16, 64); }
  else { if (D == 128) GO(MH_F16, 128); else GO(MH_F16, 64); }
#undef GO
  MH_LAUNCH_CHECK();
}

extern "C" int mh_attn_extend(const void* q, int64_t ldq, const void* kcache, const void* vcache, void* out, const int32_t* lens, int B, int n,
                              int H, int D, int Smax, int dt, void* stream) {
  return attn_extend_impl<false>(q, ldq, kcache, vcache, nullptr, nullptr, out, lens, B, n, H, D, Smax, dt, stream);
}

extern "C" int mh_attn_extend_kv8(const void* q, int64_t ldq, const void* k8, const void* v8, const float* kscale, const float* vscale, void* out,
                                  const int32_t* lens, int B, int n, int H, int D, int Smax, int dt, void* stream) {
  return attn_extend_impl<true>(q, ldq, k8, v8, kscale, vscale, out, lens, B, n, H, D, Smax, dt, stream);
}

extern "C" int mh_attn_extend_branches(const void* q, int64_t ldq, const void* kcache, const void* vcache, void* out, const int32_t* seg_start,
                                       int P, int R, int H, int D, int Smax, int dt, void* stream) {
  return attn_branches_impl<false>(q, ldq, kcache, vcache, nullptr, nullptr, out, seg_start, P, R, H, D, Smax, dt, stream);
}

extern "C" int mh_attn_extend_branches_kv8(const void* q, int64_t ldq, const void* k8, const void* v8, const float* kscale, const float* vscale,
                                           void* out, const int32_t* seg_start, int P, int R, int H, int D, int Smax, int dt, void* stream) {
  return attn_branches_impl<true>(q, ldq, k8, v8, kscale, vscale, out, seg_start, P, R, H, D, Smax, dt, stream);
}

// ---- beam search on a shared prompt cache ------------------------------------------------------------------------------------------------
extern "C" int mh_beam_ancestry(const int32_t* anc_in, int32_t* anc_out, const int64_t* beam_idx, const int32_t* gen, int rows, int G,
                                void* stream) {
  if (!anc_in || !anc_out || anc_in == anc_out || !beam_idx || !gen || rows <= 0 || G <= 0) return MH_ERR_ARG;
  hipLaunchKernelGGL(beam_ancestry_k, dim3(rows), dim3(256), 0, as_stream(stream), anc_in, anc_out, beam_idx, gen, rows, G);
  MH_LAUNCH_CHECK();
}

// key splits of the suffix part: >= 256 generated keys per split, four at the most
extern "C" int mh_attn_decode_beams_suffix_splits(int G) {
  if (G <= 0) return 0;
  const int s = (G + 255) / 256;
  return s > 4 ? 4 : s;
}

// key splits of the prefix part: the one-query plan of the Bp prompts, then more until a split's TQ x chunk fp32 scores fit 64 KiB (the rule
// of mh_attn_decode_multi_splits), within the 32 slots the merge kernel takes less the suffix part's; 0 where even that leaves a block more
// scores than the 150 KiB it may request
extern "C" int mh_attn_decode_beams_splits(int Bp, int nb, int H, int Pmax, int G) {
  if (Bp <= 0 || nb < 1 || nb > 16 || H <= 0 || Pmax <= 0 || G <= 0) return 0;
  const int most = 32 - mh_attn_decode_beams_suffix_splits(G);
  int s = mh_attn_decode_splits(Bp, H, Pmax);
  if (s > most) s = most;
  const int64_t tq = attn_multi_tq(nb);
  while (s < most && tq * ((Pmax + s - 1) / s) * 4 > ATTN_MULTI_LDS_AIM) ++s;
  return tq * ((Pmax + s - 1) / s) * 4 > ATTN_MULTI_LDS_MAX ? 0 : s;
}

template <int DT, int D, int TQ, bool KV8>
static void launch_attn_beams(const void* q, int64_t ldq, const void* pk, const void* pv, const float* pks, const float* pvs,
                              const int32_t* pre_lens, const void* sk, const void* sv, const float* sks, const float* svs, const int32_t* anc,
                              const int32_t* slens, void* out, int Bp, int nb, int H, int Pmax, int G, int psplits, int ssplits, float* ws,
                              hipStream_t st) {
  static bool attr = false;
  if (!attr) {
    hipFuncSetAttribute((const void*)attn_decode_multi_k<DT, D, TQ, KV8, true>, hipFuncAttributeMaxDynamicSharedMemorySize, ATTN_MULTI_LDS_MAX);
    attr = true;
  }
  const float scale_log2 = 1.4426950408889634f / sqrtf((float)D);
  const int rows = Bp * nb, wsplits = psplits + ssplits;
  const int pchunk = (Pmax + psplits - 1) / psplits, schunk = (G + ssplits - 1) / ssplits;
  const size_t plds = sizeof(float) * (size_t)TQ * (pchunk > 4 * D ? pchunk : 4 * D);  // scores [chunk][TQ], then the four waves' [TQ][D] partials
  const int NS = 256 / (D / 8);
  const size_t slds = sizeof(float) * (size_t)(schunk > NS * D ? schunk : NS * D);
  hipLaunchKernelGGL((attn_decode_multi_k<DT, D, TQ, KV8, true>), dim3(Bp * H * psplits), dim3(256), plds, st, (const uint16_t*)q, ldq, pk, pv,
                     pks, pvs, (uint16_t*)out, pre_lens, nb, H, Pmax, scale_log2, psplits, pchunk, ws, wsplits);
  hipLaunchKernelGGL((attn_decode_k<KVFmt<KV8>, AncestryRows, DT, D>), dim3(rows * H * ssplits), dim3(256), slds, st, (const uint16_t*)q, ldq, sk,
                     sv, sks, svs, (uint16_t*)nullptr, slens, anc, rows, H, G, scale_log2, ssplits, schunk, ws, psplits, wsplits);
  hipLaunchKernelGGL((attn_decode_combine_k<DT, D>), dim3(rows * H), dim3(D), 0, st, (const float*)ws, (uint16_t*)out, H, wsplits);
}

template <bool KV8>
static int attn_beams_impl(const void* q, int64_t ldq, const void* pk, const void* pv, const float* pks, const float* pvs,
                           const int32_t* pre_lens, const void* sk, const void* sv, const float* sks, const float* svs, const int32_t* anc,
                           const int32_t* slens, void* out, int Bp, int nb, int H, int D, int Pmax, int G, float* ws, int dt, void* stream) {
  if (!q || !pk || !pv || !pre_lens || !sk || !sv || !anc || !slens || !out || !ws) return MH_ERR_ARG;
  if (Bp <= 0 || nb < 1 || nb > 16 || H <= 0 || Pmax <= 0 || G <= 0 || (ldq & 7) || !aligned16(q)) return MH_ERR_ARG;
  if (KV8 && (!pks || !pvs || !sks || !svs || (((uintptr_t)pk | (uintptr_t)pv | (uintptr_t)sk | (uintptr_t)sv) & 7u))) return MH_ERR_ARG;
  if (!KV8 && (!aligned16(pk) || !aligned16(pv) || !aligned16(sk) || !aligned16(sv))) return MH_ERR_ARG;
  if (D != 128 && D != 64) return MH_ERR_SHAPE;
  if (dt != MH_BF16 && dt != MH_F16) return MH_ERR_DTYPE;
  const int psplits = mh_attn_decode_beams_splits(Bp, nb, H, Pmax, G), ssplits = mh_attn_decode_beams_suffix_splits(G);
  if (psplits <= 0) return MH_ERR_SHAPE;
  const int schunk = (G + ssplits - 1) / ssplits;
  if ((int64_t)schunk * 4 > ATTN_MULTI_LDS_MAX) return MH_ERR_SHAPE;  // G above 153 600 generated keys
  if ((int64_t)Bp * nb * H * (psplits + ssplits) > 0x7fffffff / (D + 2)) return MH_ERR_SHAPE;
  {  // the suffix kernel's LDS beyond the default 64 KiB (G above 65 536)
    static bool attr = false;
    if (!attr && (int64_t)schunk * 4 > 64 * 1024) {
#define GO(DT_, D_) \
  hipFuncSetAttribute((const void*)attn_decode_k<KVFmt<KV8>, AncestryRows, DT_, D_>, hipFuncAttributeMaxDynamicSharedMemorySize, ATTN_MULTI_LDS_MAX)
      GO(MH_BF16, 128); GO(MH_BF16, 64); GO(MH_F16, 128); GO(MH_F16, 64);
#undef GO
      attr = true;
    }
  }
  const int tq = attn_multi_tq(nb);
  hipStream_t st = as_stream(stream);
#define GO(DT_, D_, TQ_) \
  launch_attn_beams<DT_, D_, TQ_, KV8>(q, ldq, pk, pv, pks, pvs, pre_lens, sk, sv, sks, svs, anc, slens, out, Bp, nb, H, Pmax, G, psplits, ssplits, ws, st)
#define GOT(DT_, D_) do { if (tq == 4) GO(DT_, D_, 4); else if (tq == 8) GO(DT_, D_, 8); else GO(DT_, D_, 16); } while (0)
  if (dt == MH_BF16) { if (D == 128) GOT(MH_BF16, 128); else GOT(MH_BF16, 64); }
  else { if (D == 128) GOT(MH_F16, 128); else GOT(MH_F16, 64); }
#undef GOT
#undef GO
  MH_LAUNCH_CHECK();
}

extern "C" int mh_attn_decode_beams(const void* q, int64_t ldq, const void* pre_k, const void* pre_v, const int32_t* pre_lens, const void* suf_k,
                                    const void* suf_v, const int32_t* anc, const int32_t* slens, void* out, int Bp, int nb, int H, int D,
                                    int Pmax, int G, float* ws, int dt, void* stream) {
  return attn_beams_impl<false>(q, ldq, pre_k, pre_v, nullptr, nullptr, pre_lens, suf_k, suf_v, nullptr, nullptr, anc, slens, out, Bp, nb, H, D,
                                Pmax, G, ws, dt, stream);
}

extern "C" int mh_attn_decode_beams_kv8(const void* q, int64_t ldq, const void* pre_k8, const void* pre_v8, const float* pre_kscale,
                                        const float* pre_vscale, const int32_t* pre_lens, const void* suf_k8, const void* suf_v8,
                                        const float* suf_kscale, const float* suf_vscale, const int32_t* anc, const int32_t* slens, void* out,
                                        int Bp, int nb, int H, int D, int Pmax, int G, float* ws, int dt, void* stream) {
  return attn_beams_impl<true>(q, ldq, pre_k8, pre_v8, pre_kscale, pre_vscale, pre_lens, suf_k8, suf_v8, suf_kscale, suf_vscale, anc, slens, out,
                               Bp, nb, H, D, Pmax, G, ws, dt, stream);
}

extern "C" int mh_ngram_draft(const int64_t* ids, int64_t ld, int rows, int len, int max_ngram, int k, int max_length, int64_t* out,
                              int32_t* out_count, void* stream) {
  if (!ids || !out || !out_count || rows <= 0 || len <= 0 || ld < len || max_ngram <= 0 || k <= 0 || max_length <= 0) return MH_ERR_ARG;
  hipLaunchKernelGGL(ngram_draft_k, dim3(rows), dim3(256), 0, as_stream(stream), ids, ld, len, max_ngram, k, max_length, out, out_count);
  MH_LAUNCH_CHECK();
}

extern "C" int mh_quant_fp8_b128(const void* w, int64_t ldw, void* q, float* scales, int N, int K, int dt, void* stream) {
  if (!w || !q || !scales || N <= 0 || K <= 0 || (K & 7) || (ldw & 7) || !aligned16(w)) return MH_ERR_ARG;
  if (dt != MH_BF16 && dt != MH_F16) return MH_ERR_DTYPE;
  const int64_t blocks = (int64_t)N * ((K + 127) / 128);
  const dim3 grid((unsigned)((blocks + 15) / 16)), block(256);
  if (dt == MH_BF16)
    hipLaunchKernelGGL(quant_fp8_b128_k<MH_BF16>, grid, block, 0, as_stream(stream), (const uint16_t*)w, ldw, (uint8_t*)q, scales, N, K);
  else
    hipLaunchKernelGGL(quant_fp8_b128_k<MH_F16>, grid, block, 0, as_stream(stream), (const uint16_t*)w, ldw, (uint8_t*)q, scales, N, K);
  MH_LAUNCH_CHECK();
}

static int gemv_fp8w_impl(const GemvArgs& a) {
  if (const int e = gemv_check<WFp8>(a)) return e;
  if (gemv_mfma_rows<WFp8>(a) && (a.K % 64) == 0 && (!a.ra.tab || ((a.ra.D >> 1) % 16 == 0 && a.N == 3 * a.ra.H * a.ra.D))) {
    auto mfma = a.dt == MH_BF16 ? launch_gemv_mfma<MH_BF16, true> : launch_gemv_mfma<MH_F16, true>;  // (weight row stride: K)
    return mfma(a.x, a.ldx, a.W, a.K, (const float*)a.wsc, a.out, a.ldo, a.resid, a.ldr, a.M, a.N, a.K, a.out_f32, a.swi_ff, a.ra, as_stream(a.stream));
  }
  return gemv_wave_launch<WFp8>(a);
}

extern "C" int mh_gemv_fp8w(const void* x, int64_t ldx, const void* q, const float* scales, void* out, int64_t ldo, const void* resid,
                            int64_t ldr, int M, int N, int K, int dt, int out_f32, void* stream) {
  return gemv_fp8w_impl({x, ldx, q, 0, scales, out, ldo, resid, ldr, M, N, K, dt, out_f32, 0, nullptr, 0.f, RopeAppend{}, stream});
}
// mh_gemv_norm with fp8 (e4m3, per-128-block scales) weights: out = rmsnorm(x; norm_w, eps) W^T (norm_w may be NULL: no norm), ff > 0: SwiGLU of the
// gate|up rows.  With norm_w: M <= 8, K <= 8192; without: M <= 16.
extern "C" int mh_gemv_fp8w_norm(const void* x, int64_t ldx, const void* norm_w, float eps, const void* q, const float* scales, void* out,
                                 int64_t ldo, int M, int N, int K, int ff, int dt, void* stream) {
  if (ff < 0) return MH_ERR_ARG;
  return gemv_fp8w_impl({x, ldx, q, 0, scales, out, ldo, nullptr, 0, M, ff > 0 ? ff : N, K, dt, 0, ff, norm_w, eps, RopeAppend{}, stream});
}

// q|k|v projection of the decode step with everything around it in one launch: (optional) input_layernorm of x, the projection with 16-bit
// (W) or fp8 (q8 + scales) weights, rotate-half RoPE of q and k at pos[m] and the append of k, v to the cache rows [m, pos[m]]
// (= mh_rmsnorm_fwd + mh_gemv / mh_gemv_fp8w + mh_decode_rope_append, bit for bit).  qkv [M, 3 H D] receives the rotated q, k and v.
extern "C" int mh_gemv_qkv_rope(const void* x, int64_t ldx, const void* norm_w, float eps, const void* W, int64_t ldw, const void* q8,
                                const float* scales, void* qkv, int64_t ldo, int M, int K, int dt, const float* cos_sin, const int32_t* pos,
                                const int32_t* rope_pos, void* kcache, void* vcache, int H, int D, int Smax, void* stream) {
  if (!cos_sin || !pos || !kcache || !vcache || H <= 0 || D <= 0 || (D & 1) || Smax <= 0 || (!W && !(q8 && scales))) return MH_ERR_ARG;
  RopeAppend ra;
  ra.tab = (const float2*)cos_sin; ra.pos = pos; ra.rpos = rope_pos ? rope_pos : pos; ra.kc = (uint16_t*)kcache; ra.vc = (uint16_t*)vcache; ra.H = H; ra.D = D; ra.Smax = Smax;
  const int N = 3 * H * D;
  if (W) return gemv_impl({x, ldx, W, ldw, nullptr, qkv, ldo, nullptr, 0, M, N, K, dt, 0, 0, norm_w, eps, ra, stream});
  return gemv_fp8w_impl({x, ldx, q8, 0, scales, qkv, ldo, nullptr, 0, M, N, K, dt, 0, 0, norm_w, eps, ra, stream});
}

// ---- MXFP4 weights (OCP MX: e2m1 values, one power-of-two E8M0 scale per 32 consecutive k), bf16/f16 activations -----------------------
// The next halving of the weight stream after fp8: 0.53 bytes per weight.  Stored format (the contract: the prefill's many-row product
// mh_gemm_fp4w, gemm_fp4w.hip, reads it as it is, and a later v_mfma_scale_*_f8f6f4 product would): q [N, K/2] bytes, byte j of a row = element 2j in the LOW nibble and 2j + 1 in the high
// one, code s e e m = magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6; scales [N, K/32] bytes = e + 127.
// Scale: the rule of kv8_exp moved to a maximum of 6 - e the smallest integer with amax 2^-e <= 6 (amax = m 2^ex, m in [0.5, 1):
// e = ex - 3 if m <= 0.75 else ex - 2), clamped to >= -126, 0 for an all-zero block: nothing saturates.  Value: w 2^-e (exact in fp32)
// rounded to the e2m1 grid, ties to the code with an even mantissa bit - in plain compares, so the tie rule does not depend on what
// v_cvt_scalef32_pk_fp4_f32 does (the quantiser runs once per weight change).  q 2^e is exact in bf16 (and in fp16 while in range): the
// fp4 path is the 16-bit path on weights rounded to that grid.
namespace {

__device__ __forceinline__ int fp4_exp(float amax) {  // amax >= 0, finite
  const uint32_t bits = __float_as_uint(amax);
  const int ef = (int)(bits >> 23);
  if (ef == 0) return bits ? -126 : 0;  // fp32 subnormal (a bf16 subnormal block): e < -126 clamps
  return max(ef - 126 - ((bits & 0x7fffffu) <= 0x400000u ? 3 : 2), -126);
}
__device__ __forceinline__ uint32_t fp4_code(float v, float inv) {  // |v| inv <= 6
  const float a = fabsf(v) * inv;
  const uint32_t c = (uint32_t)(a > 0.25f) + (uint32_t)(a >= 0.75f) + (uint32_t)(a > 1.25f) + (uint32_t)(a >= 1.75f) + (uint32_t)(a > 2.5f) +
                     (uint32_t)(a >= 3.5f) + (uint32_t)(a > 5.0f);  // ties: 0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4
  return c | ((__float_as_uint(v) >> 28) & 8u);
}

// one launch: 4 lanes per 32-element block (16-byte loads, block maximum by two shuffles, one 4-byte store of 8 codes per lane)
template <int DT>
__global__ __launch_bounds__(256) void quant_fp4_b32_k(const uint16_t* __restrict__ w, int64_t ldw, uint8_t* __restrict__ q,
                                                       uint8_t* __restrict__ sc, int N, int K) {
  const int nb = K >> 5;
  const int64_t blk = (int64_t)blockIdx.x * 64 + (threadIdx.x >> 2);
  if (blk >= (int64_t)N * nb) return;  // (whole groups of 4 lanes)
  const int n = (int)(blk / nb), kb = (int)(blk % nb), part = threadIdx.x & 3;
  const int k0 = kb * 32 + part * 8;
  float v[8];
  unpack8<DT>(*(const uint4*)(w + (int64_t)n * ldw + k0), v);
  float mx = amax8(v);
  mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
  const int e = fp4_exp(mx);
  const float inv = kv8_pow2(-e);  // e in [-126, 126]
  uint32_t p = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) p |= fp4_code(v[i], inv) << (4 * i);
  *(uint32_t*)(q + (int64_t)n * (K >> 1) + (k0 >> 1)) = p;
  if (part == 0) sc[(int64_t)n * nb + kb] = (uint8_t)(e + 127);
}



// 3..16 activation rows: gemv_mfma_k with fp4 weights.  A block owns 16 x RG weight rows, its 8 waves split K in steps of 128.  Lane
// l = (row j = l & 15, kq = l >> 4) loads 16 B = ONE WHOLE scale block (block kq of the step) of its row, but an MFMA's four k-chunks
// of a column come from the four lanes kq = 0..3 and its result cannot be scaled per chunk.  So the 4 x 4 (lane kq) x (dword) tile is
// transposed in registers first (two v_permlane32_swap + two v_permlane16_swap per load): afterwards dword i of lane (j, kq) is dword
// kq of block i, MFMA i multiplies block i alone (k in its natural order: the A operand is x[k + 32 i + 8 kq ..]) and its fp32 tile is
// scaled by that block's 2^e - the semantics of the wave form, conversion with scale 1.  The step's four scale bytes of a row are one
// dword load where the scale rows are dword-aligned (K % 128 == 0), four byte loads otherwise.  16 cvt + 4 swaps + 4 MFMA + 16 fma
// per KB of weights.  RG, PAIR = 1 (SwiGLU partner rows) and the fixed-order reduction through LDS as in gemv_mfma_k.
template <int DT, int RG, int PAIR>
__global__ __launch_bounds__(512) void gemv_fp4w_mfma_k(const uint16_t* __restrict__ x, int64_t ldx, const uint8_t* __restrict__ q,
                                                        const uint8_t* __restrict__ sc, void* __restrict__ out, int64_t ldo,
                                                        const uint16_t* __restrict__ resid, int64_t ldr, int M, int N, int K, int out_f32,
                                                        int swi_ff, int sc_dwords) {
  static_assert(PAIR == 0 || RG == 2, "the paired epilogue takes two row groups");
  constexpr int NW = 8, NS = 4, KS = 128, KP = NW * NS * KS;
  __shared__ __attribute__((aligned(16))) float red[NW * RG * 64 * 4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, kq = lane >> 4;
  int n0 = blockIdx.x * 16 * RG, goff = 16, nlim = N;
  if constexpr (PAIR == 1) { n0 = blockIdx.x * 16; goff = swi_ff; nlim = N + swi_ff; }
  const bool arow = j < M;
  const int nb = K >> 5;
  f32x4_t acc[RG];
  const uint8_t* wr[RG];
  const uint8_t* sr[RG];
#pragma unroll
  for (int g = 0; g < RG; ++g) {
    const int n = PAIR == 1 ? min(n0 + j, N - 1) + g * goff : min(n0 + goff * g + j, nlim - 1);
    acc[g] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    wr[g] = q + (int64_t)n * (K >> 1) + kq * 16;
    sr[g] = sc + (int64_t)n * nb;
  }
  const uint16_t* xr = x + (int64_t)min(j, M - 1) * ldx + kq * 8;
  for (int kp = 0; kp < K; kp += KP) {
    uint4 wv[RG][NS], xv[NS][4];
    uint32_t sv[RG][NS];  // the step's four scale bytes, block i in byte i
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      const int k = kp + (wave + NW * u) * KS;
#pragma unroll
      for (int g = 0; g < RG; ++g) {
        wv[g][u] = (k + kq * 32 < K) ? ld_stream16(wr[g] + (k >> 1)) : make_uint4(0, 0, 0, 0);
        uint32_t s4 = 0;
        if (sc_dwords) {
          if (k < K) s4 = *(const uint32_t*)(sr[g] + (k >> 5));
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (k + 32 * i < K) s4 |= (uint32_t)sr[g][(k >> 5) + i] << (8 * i);
        }
        sv[g][u] = s4;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) xv[u][i] = (k + 32 * i < K && arow) ? *(const uint4*)(xr + k + 32 * i) : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      if (kp + (wave + NW * u) * KS >= K) break;
#pragma unroll
      for (int g = 0; g < RG; ++g) {
        uint32_t d[4] = {wv[g][u].x, wv[g][u].y, wv[g][u].z, wv[g][u].w};
        // transpose: lanes 32 apart exchange dwords (0, 2) and (1, 3), then lanes 16 apart (0, 1) and (2, 3)
        auto t = __builtin_amdgcn_permlane32_swap(d[0], d[2], false, false); d[0] = t[0]; d[2] = t[1];
        t = __builtin_amdgcn_permlane32_swap(d[1], d[3], false, false); d[1] = t[0]; d[3] = t[1];
        t = __builtin_amdgcn_permlane16_swap(d[0], d[1], false, false); d[0] = t[0]; d[1] = t[1];
        t = __builtin_amdgcn_permlane16_swap(d[2], d[3], false, false); d[2] = t[0]; d[3] = t[1];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          uint32_t bw[4];
          fp4x8_to_pk16<DT>(d[i], bw);
          const f32x4_t part = mfma16<DT>(xv[u][i], make_uint4(bw[0], bw[1], bw[2], bw[3]), f32x4_t{0.f, 0.f, 0.f, 0.f});
          const float s = e8m0_to_f32((sv[g][u] >> (8 * i)) & 255u);
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[g][c] = fmaf(s, part[c], acc[g][c]);
        }
      }
    }
  }
  // D lane l reg r = D[m = 4 * (l >> 4) + r][n = l & 15]: sum the NW waves' tiles in wave order
#pragma unroll
  for (int g = 0; g < RG; ++g) *(f32x4_t*)(red + ((wave * RG + g) * 64 + lane) * 4) = acc[g];
  __syncthreads();
  if constexpr (PAIR == 1) {
    if (wave == 0) {
      f32x4_t s0 = *(const f32x4_t*)(red + lane * 4), s1 = *(const f32x4_t*)(red + (64 + lane) * 4);
#pragma unroll 4
      for (int w = 1; w < NW; ++w) {
        const f32x4_t t0 = *(const f32x4_t*)(red + ((w * 2) * 64 + lane) * 4), t1 = *(const f32x4_t*)(red + ((w * 2 + 1) * 64 + lane) * 4);
#pragma unroll
        for (int r = 0; r < 4; ++r) { s0[r] += t0[r]; s1[r] += t1[r]; }
      }
      uint16_t* o16 = (uint16_t*)out;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = 4 * kq + r;
        if (m >= M) continue;
        const float lo = ld16<DT>((uint16_t)st16<DT>(s0[r])), hi = ld16<DT>((uint16_t)st16<DT>(s1[r]));  // the projection as it would be stored
        if (n0 + j < N) o16[(int64_t)m * ldo + n0 + j] = (uint16_t)st16<DT>(swiglu_fwd1(lo, hi));
      }
    }
    return;
  }
  if (wave < RG) {
    const int g = wave;
    f32x4_t s4 = *(const f32x4_t*)(red + (g * 64 + lane) * 4);
#pragma unroll
    for (int w = 1; w < NW; ++w) {
      const f32x4_t t = *(const f32x4_t*)(red + ((w * RG + g) * 64 + lane) * 4);
#pragma unroll
      for (int r = 0; r < 4; ++r) s4[r] += t[r];
    }
    const int n = n0 + 16 * g + j;
    if (n < N) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = 4 * kq + r;
        if (m >= M) continue;
        float v = s4[r];
        if (resid) v += ld16<DT>(resid[(int64_t)m * ldr + n]);
        if (out_f32) ((float*)out)[(int64_t)m * ldo + n] = v;
        else ((uint16_t*)out)[(int64_t)m * ldo + n] = (uint16_t)st16<DT>(v);
      }
    }
  }
}

template <int DT>
int launch_gemv_fp4w_mfma(const void* x, int64_t ldx, const void* q, const void* sc, void* out, int64_t ldo, const void* resid, int64_t ldr, int M,
                          int N, int K, int out_f32, int swi_ff, hipStream_t st) {
  const int scd = (K % 128 == 0 && (((uintptr_t)sc) & 3u) == 0) ? 1 : 0;
#define MH_GM4(RG_, PAIR_, BLOCKS_)                                                                                                       \
  hipLaunchKernelGGL((gemv_fp4w_mfma_k<DT, RG_, PAIR_>), dim3(BLOCKS_), dim3(512), 0, st, (const uint16_t*)x, ldx, (const uint8_t*)q,     \
                     (const uint8_t*)sc, out, ldo, (const uint16_t*)resid, ldr, M, N, K, out_f32, swi_ff, scd)
  if (swi_ff) MH_GM4(2, 1, (N + 15) / 16);  // N = ff outputs
  else if (N >= 30000) MH_GM4(4, 0, (N + 63) / 64);  // (rows per block by N: the thresholds of launch_gemv_mfma)
  else if (N >= 12000) MH_GM4(2, 0, (N + 31) / 32);
  else MH_GM4(1, 0, (N + 15) / 16);
#undef MH_GM4
  MH_LAUNCH_CHECK();
}

}  // namespace

extern "C" int mh_quant_fp4_b32(const void* w, int64_t ldw, void* q, void* scales, int N, int K, int dt, void* stream) {
  if (!w || !q || !scales || N <= 0 || K <= 0 || (K & 31) || (ldw & 7) || !aligned16(w) || (((uintptr_t)q) & 3u)) return MH_ERR_ARG;
  if (dt != MH_BF16 && dt != MH_F16) return MH_ERR_DTYPE;
  const int64_t blocks = (int64_t)N * (K >> 5);
  const dim3 grid((unsigned)((blocks + 63) / 64)), block(256);
  if (dt == MH_BF16)
    hipLaunchKernelGGL(quant_fp4_b32_k<MH_BF16>, grid, block, 0, as_stream(stream), (const uint16_t*)w, ldw, (uint8_t*)q, (uint8_t*)scales, N, K);
  else
    hipLaunchKernelGGL(quant_fp4_b32_k<MH_F16>, grid, block, 0, as_stream(stream), (const uint16_t*)w, ldw, (uint8_t*)q, (uint8_t*)scales, N, K);
  MH_LAUNCH_CHECK();
}

// (no MFMA form of the RoPE + append projection: it stays on the wave form, so M <= 8)
static int gemv_fp4w_impl(const GemvArgs& a) {
  if (const int e = gemv_check<WFp4>(a)) return e;
  if (!a.ra.tab && gemv_mfma_rows<WFp4>(a) && (a.K % 64) == 0) {
    auto mfma = a.dt == MH_BF16 ? launch_gemv_fp4w_mfma<MH_BF16> : launch_gemv_fp4w_mfma<MH_F16>;
    return mfma(a.x, a.ldx, a.W, a.wsc, a.out, a.ldo, a.resid, a.ldr, a.M, a.N, a.K, a.out_f32, a.swi_ff, as_stream(a.stream));
  }
  return gemv_wave_launch<WFp4>(a);
}

extern "C" int mh_gemv_fp4w(const void* x, int64_t ldx, const void* q, const void* scales, void* out, int64_t ldo, const void* resid,
                            int64_t ldr, int M, int N, int K, int dt, int out_f32, void* stream) {
  return gemv_fp4w_impl({x, ldx, q, 0, scales, out, ldo, resid, ldr, M, N, K, dt, out_f32, 0, nullptr, 0.f, RopeAppend{}, stream});
}
// mh_gemv_fp8w_norm with fp4 weights: out = rmsnorm(x; norm_w, eps) W^T (norm_w may be NULL: no norm), ff > 0: SwiGLU of the gate|up rows.
// With norm_w: M <= 8, K <= 8192; without: M <= 16.
extern "C" int mh_gemv_fp4w_norm(const void* x, int64_t ldx, const void* norm_w, float eps, const void* q, const void* scales, void* out,
                                 int64_t ldo, int M, int N, int K, int ff, int dt, void* stream) {
  if (ff < 0) return MH_ERR_ARG;
  return gemv_fp4w_impl({x, ldx, q, 0, scales, out, ldo, nullptr, 0, M, ff > 0 ? ff : N, K, dt, 0, ff, norm_w, eps, RopeAppend{}, stream});
}
// mh_gemv_qkv_rope with fp4 weights (= mh_rmsnorm_fwd + mh_gemv_fp4w + mh_decode_rope_append, bit for bit): one wave per rotary pair, M <= 8.
extern "C" int mh_gemv_fp4w_qkv_rope(const void* x, int64_t ldx, const void* norm_w, float eps, const void* q, const void* scales, void* qkv,
                                     int64_t ldo, int M, int K, int dt, const float* cos_sin, const int32_t* pos, const int32_t* rope_pos,
                                     void* kcache, void* vcache, int H, int D, int Smax, void* stream) {
  if (!cos_sin || !pos || !kcache || !vcache || H <= 0 || D <= 0 || (D & 1) || Smax <= 0 || M > 8) return MH_ERR_ARG;
  RopeAppend ra;
  ra.tab = (const float2*)cos_sin; ra.pos = pos; ra.rpos = rope_pos ? rope_pos : pos; ra.kc = (uint16_t*)kcache; ra.vc = (uint16_t*)vcache; ra.H = H; ra.D = D; ra.Smax = Smax;
  return gemv_fp4w_impl({x, ldx, q, 0, scales, qkv, ldo, nullptr, 0, M, 3 * H * D, K, dt, 0, 0, norm_w, eps, ra, stream});
}
