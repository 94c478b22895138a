// Many-row product on MXFP4 weights (gfx950): out[M, N] = x[M, K] * dequant(q, scales)[N, K]^T, the prefill's counterpart of the decode
// GEMVs mh_gemv_fp4w* (decode.hip).  The weight is exactly what mh_quant_fp4_b32 writes - q [N, K/2] bytes, byte j of a row = element 2j
// in the LOW nibble and 2j + 1 in the high one, scales [N, K/32] bytes = e + 127 - nothing is repacked at quantise time.
//
//   * 128 x 128 x 64 block tile, 4 waves (2 x 2), each wave 64 x 64 of the output in 16 accumulator fragments; two LDS stages of
//     16 KiB of x, 4 KiB of codes and 1 KiB of scales, one barrier per K-tile (the structure of gemm_nt_128, gemm.hip).
//   * the weight travels global -> LDS -> registers as packed 4-bit codes, a quarter of the 16-bit bytes at every level.  x rows are
//     128-B LDS rows with the chunk swizzle of gemm.hip; a code row of a K-tile is 32 B = two 16-B halves (one per 32-k scale block),
//     half' = half ^ ((row >> 2) & 1) on the source address and again on the read (a ds_read_b32 of 16 rows then meets every bank twice,
//     the least 16 rows x 2 dwords in eight 16-B slots allow).  Both by global_load_lds_dwordx4; the K-tile's 2 scale bytes per row go
//     through a register and are stored as fp32 powers of two.
//   * a lane's 8 consecutive k of one MFMA are ONE dword of codes inside ONE scale block: v_cvt_scalef32_pk_{bf16,f16}_fp4 widens it
//     to the 16-bit fragment with the block's 2^e applied (4 instructions, byte b of the dword -> pair b, low nibble -> low half: the
//     stored order), and that fragment is reused by the wave's four M tiles - converted once per weight, not once per MFMA.
//     code * 2^e is exact in bf16 for every scale the quantiser emits above its clamped exponent, in f16 for scale bytes 104 .. 140;
//     outside that window the f16 product uses the weight as the instruction rounds it to f16 (see the header).
//   * fragment reads are hand-waited inline asm (lds_read128 of mh_common.h and a 4-byte sibling): all 24 reads of a K-tile are issued behind
//     the barrier and the LDS-DMA of tile kt + 1, the first MFMA step waits for its own 12 (LDS returns in order), the second for the rest.
//     Plain reads made hipcc drain the DMA in front of them (vmcnt(0)), a synchronous stage: 0.25-0.90 PFLOP/s where this form reaches 0.36-1.00
//     on the 7B projections (profiles/fp4_prefill_bench.txt).  The scale byte of tile kt + 1 is the loop's only register load; it is consumed
//     behind the MFMAs, where the next iteration's vmcnt(0) waits anyway.
//   * the fragment is passed as the A operand (gemm.hip), so a lane holds 4 CONSECUTIVE n of one m: 8-byte / 16-byte stores where the
//     caller's strides allow them, element stores otherwise and on the ragged N edge.
//   * M and N edges: loads clamp the row index, stores are predicated.  K % 32 == 0: the half K-tile at the end of an odd block count
//     is fed from a zero chunk (x and codes), its scale is 1.
#include "mh_common.h"

namespace {

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int X_BYTES = BM * BK * 2;   // 16 KiB
constexpr int Q_BYTES = BN * BK / 2;   // 4 KiB
constexpr int S_BYTES = 2 * BN * 4;    // 1 KiB: fp32 [2 scale blocks][BN]
constexpr int STAGE = X_BYTES + Q_BYTES + S_BYTES;

__device__ uint4 g_zero_chunk;  // zero-initialised: the source of every 16-B chunk at k >= K

template <int DT>
__device__ __forceinline__ uint4 fp4x8_scaled(uint32_t p, float s) {
  uint4 w;
  if constexpr (DT == MH_BF16) {
    w.x = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(p, s, 0));
    w.y = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(p, s, 1));
    w.z = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(p, s, 2));
    w.w = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(p, s, 3));
  } else {
    w.x = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(p, s, 0));
    w.y = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(p, s, 1));
    w.z = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(p, s, 2));
    w.w = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(p, s, 3));
  }
  return w;
}

template <int OFF, typename T>
__device__ __forceinline__ void lds_read32(T& d, unsigned addr) {  // hand-waited like lds_read128 (mh_common.h)
  asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "n"(OFF));
}

struct Fp4wArgs {
  const uint16_t* x; int64_t ldx;
  const uint8_t* q; const uint8_t* sc;
  void* out; int64_t ldo;
  const uint16_t* resid; int64_t ldr;
  int M, N, K, out_f32, accum, vec;
};

// out[m, n .. n + 3] (n % 4 == 0) from the fp32 sums: + resid (16-bit store) or + out (fp32 read-modify-write)
template <int DT>
__device__ __forceinline__ void fp4w_store4(const Fp4wArgs& g, int m, int n, f32x4_t v) {
  if (m >= g.M || n >= g.N) return;
  const bool whole = g.vec && n + 3 < g.N;
  if (g.out_f32) {
    float* o = (float*)g.out + (int64_t)m * g.ldo + n;
    if (whole) {
      if (g.accum) { const float4 p = *(const float4*)o; v[0] += p.x; v[1] += p.y; v[2] += p.z; v[3] += p.w; }
      *(float4*)o = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (n + r < g.N) o[r] = g.accum ? v[r] + o[r] : v[r];
    }
    return;
  }
  uint16_t* o = (uint16_t*)g.out + (int64_t)m * g.ldo + n;
  const uint16_t* rs = g.resid ? g.resid + (int64_t)m * g.ldr + n : nullptr;
  if (whole) {
    if (rs) {
      const uint2 p = *(const uint2*)rs;
      float r0, r1, r2, r3;
      unpack2<DT>(p.x, r0, r1);
      unpack2<DT>(p.y, r2, r3);
      v[0] += r0; v[1] += r1; v[2] += r2; v[3] += r3;
    }
    *(uint2*)o = make_uint2(pack2<DT>(v[0], v[1]), pack2<DT>(v[2], v[3]));
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (n + r < g.N) o[r] = (uint16_t)st16<DT>(rs ? v[r] + ld16<DT>(rs[r]) : v[r]);
  }
}

template <int DT>
__global__ __launch_bounds__(256, 2) void gemm_fp4w_k(Fp4wArgs g) {
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int tiles_m = (g.M + BM - 1) / BM;  // m fastest: consecutive blocks share a weight panel
  const int m0 = (int)(blockIdx.x % tiles_m) * BM, n0 = (int)(blockIdx.x / tiles_m) * BN;
  const int nb = g.K >> 5, nk = (g.K + BK - 1) / BK;

  // x: four 16-B chunks per thread and K-tile (row = qd / 8, stored chunk qd % 8 holds chunk ^ ((row >> 1) & 7))
  const uint16_t* xsrc[4];
  int xk[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int qd = i * 256 + tid;
    const int row = qd >> 3, c = (qd & 7) ^ ((row >> 1) & 7);
    xsrc[i] = g.x + (int64_t)min(m0 + row, g.M - 1) * g.ldx + c * 8;
    xk[i] = c * 8;
  }
  // codes: one 16-B half row per thread and K-tile (row = tid / 2, stored half tid % 2 holds half ^ ((row >> 2) & 1)); the same
  // thread fetches the scale byte of (row, block tid % 2)
  const int qrow = tid >> 1, qh = (tid & 1) ^ ((qrow >> 2) & 1), sblk = tid & 1;
  const int qn = min(n0 + qrow, g.N - 1);
  const uint8_t* qsrc = g.q + (int64_t)qn * (g.K >> 1) + qh * 16;
  const int64_t srow = (int64_t)qn * nb;

  auto stage = [&](int s, int kt) {
    char* sX = smem + s * STAGE;
    char* sQ = sX + X_BYTES;
    const int koff = kt * BK;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      glds16(koff + xk[i] < g.K ? (const void*)(xsrc[i] + koff) : (const void*)&g_zero_chunk, sX + (i * 256 + wave * 64) * 16);
    glds16(koff + qh * 32 < g.K ? (const void*)(qsrc + (koff >> 1)) : (const void*)&g_zero_chunk, sQ + wave * 64 * 16);
  };
  auto scale_of = [&](int kt) -> float {  // 2^e of (row, block 2 kt + sblk); a block at k >= K multiplies zeros: 1 (the load is
    const int kb = 2 * kt + sblk;         // unconditional, so that its wait stays behind the K-tile's MFMAs)
    const uint32_t e = g.sc[srow + min(kb, nb - 1)];
    return kb < nb ? __uint_as_float(e << 23) : 1.0f;
  };
  auto put_scale = [&](int s, float v) { ((float*)(smem + s * STAGE + X_BYTES + Q_BYTES))[sblk * BN + qrow] = v; };

  f32x4_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int frow = lane & 15, kq = lane >> 4;
  const int swz = (frow >> 1) & 7, qswz = (frow >> 2) & 1;
  const int x_off = (wm * 64 + frow) * 128;
  const int w_row = wn * 64 + frow;

  // Fragment reads are hand-waited inline asm (mh_common.h): hipcc would otherwise drain the LDS-DMA of tile kt + 1 (vmcnt(0)) in front of
  // the first read of tile kt it can see.  All 24 reads of a K-tile are issued at once; LDS returns in order, so lgkmcnt(12) = the first
  // MFMA step's operands are there.
  const unsigned xa0 = lds_addr_of(smem) + x_off;
  const unsigned qa0 = lds_addr_of(smem) + X_BYTES + w_row * 32 + kq * 4;
  const unsigned sa0 = lds_addr_of(smem) + X_BYTES + Q_BYTES + w_row * 4;

  stage(0, 0);
  put_scale(0, scale_of(0));
  for (int kt = 0; kt < nk; ++kt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // tile kt landed for everyone; everyone is done reading the other stage
    if (kt + 1 < nk) stage((kt + 1) & 1, kt + 1);
    const uint32_t ebyte = g.sc[srow + min(2 * min(kt + 1, nk - 1) + sblk, nb - 1)];  // (used behind the MFMAs: its wait must not drain the DMA early)
    const unsigned sb = (kt & 1) * STAGE;
    u32x4_t xf[2][4];
    uint32_t cd[2][4];
    float sv[2][4];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const unsigned xa = xa0 + sb + (((ks * 4 + kq) ^ swz) << 4), qa = qa0 + sb + ((ks ^ qswz) << 4), sa = sa0 + sb + ks * BN * 4;
      lds_read128<0>(xf[ks][0], xa); lds_read128<2048>(xf[ks][1], xa); lds_read128<4096>(xf[ks][2], xa); lds_read128<6144>(xf[ks][3], xa);
      lds_read32<0>(cd[ks][0], qa); lds_read32<512>(cd[ks][1], qa); lds_read32<1024>(cd[ks][2], qa); lds_read32<1536>(cd[ks][3], qa);
      lds_read32<0>(sv[ks][0], sa); lds_read32<64>(sv[ks][1], sa); lds_read32<128>(sv[ks][2], sa); lds_read32<192>(sv[ks][3], sa);
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      if (ks == 0) {
        LGKM_WAIT(12);
      } else {  // (tied to the last accumulator of step 0: the wait stays behind that step's MFMAs)
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(acc[3][3]) : : "memory");
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint4 wf = fp4x8_scaled<DT>(cd[ks][j], sv[ks][j]);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i][j] = mfma16<DT>(wf, __builtin_bit_cast(uint4, xf[ks][i]), acc[i][j]);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    if (kt + 1 < nk) put_scale((kt + 1) & 1, 2 * (kt + 1) + sblk < nb ? __uint_as_float(ebyte << 23) : 1.0f);
  }

  // lane holds out[m = .. + (lane & 15)][n = .. + 4 * (lane >> 4) + r], r = 0..3
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + wm * 64 + i * 16 + frow;
#pragma unroll
    for (int j = 0; j < 4; ++j) fp4w_store4<DT>(g, m, n0 + wn * 64 + j * 16 + 4 * kq, acc[i][j]);
  }
}

}  // namespace

extern "C" int mh_gemm_fp4w(const void* x, int64_t ldx, const void* q, const void* scales, void* out, int64_t ldo, const void* resid,
                            int64_t ldr, int M, int N, int K, int dt, int out_f32, int accum, void* stream) {
  if (!x || !q || !scales || !out || M < 1 || N < 1 || K < 1 || (K & 31) || ldx < K || (ldx & 7) || ldo < N || !aligned16(x) || !aligned16(q))
    return MH_ERR_ARG;
  if (dt != MH_BF16 && dt != MH_F16) return MH_ERR_DTYPE;
  // the four store forms: 16-bit, 16-bit + 16-bit resid, fp32, fp32 read-modify-write
  if ((accum && !out_f32) || (resid && (accum || out_f32)) || (resid && ldr < N)) return MH_ERR_ARG;
  if ((((uintptr_t)out) & (out_f32 ? 3u : 1u)) || (((uintptr_t)resid) & 1u)) return MH_ERR_ARG;
  const int64_t blocks = (int64_t)((M + BM - 1) / BM) * ((N + BN - 1) / BN);
  if (blocks > 0x7fffffff) return MH_ERR_ARG;
  Fp4wArgs g{(const uint16_t*)x, ldx, (const uint8_t*)q, (const uint8_t*)scales, out, ldo, (const uint16_t*)resid, ldr, M, N, K,
             out_f32 ? 1 : 0, accum ? 1 : 0, 0};
  if (out_f32) g.vec = (ldo & 3) == 0 && aligned16(out);
  else g.vec = (ldo & 3) == 0 && (((uintptr_t)out) & 7u) == 0 && (!resid || ((ldr & 3) == 0 && (((uintptr_t)resid) & 7u) == 0));
  if (dt == MH_BF16) hipLaunchKernelGGL(gemm_fp4w_k<MH_BF16>, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), g);
  else hipLaunchKernelGGL(gemm_fp4w_k<MH_F16>, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), g);
  MH_LAUNCH_CHECK();
}
