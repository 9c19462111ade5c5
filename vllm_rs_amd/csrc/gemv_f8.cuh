// gemv_f8.cuh — FP8 E4M3 block-scaled weights (W8A16): the tile layout, its repack, and the decode kernel for 1..32 rows.
//
// Format (DeepSeek / Qwen3-FP8 checkpoints; reference: LnFp8, src/models/layers/linear.rs:776-1076): weight [N, K] E4M3 bytes,
// weight_scale_inv [ceil(N/128), ceil(K/128)] f32.  Arithmetic: the bytes widen EXACTLY to the model dtype and go
// through v_mfma_f32_16x16x32; the f32 partial sum of each 128-wide K block is multiplied by the block's f32 scale and added to the
// running f32 sum — the scale never touches a 16-bit weight.  One rounding at the output, the same at every row count.
//
// Tile layout: 1 KiB tile = 16 columns x 64 k.  byte[((nb * K/64 + kt) * 64 + lane) * 16 + h * 8 + e] holds
// w[n = nb * 16 + (lane & 15)][k = kt * 64 + h * 32 + (lane >> 4) * 8 + e]: one 16-byte load per lane yields the weight operands of
// TWO 16x16x32 MFMAs (h = 0 | 1) with no cross-lane movement, and the 16 columns of a unit are one contiguous run of 16 * K bytes.
//
// Decode kernel: HBM-bound at 1 byte per weight.  One workgroup per 16-column unit; its 4 / 8 / 16 waves (more the fewer units
// there are, so that N/16 below the CU count still puts 16 streaming waves on each busy CU) split K in whole 128-blocks.  A wave
// streams its run of tiles with a register ring of 4 blocks (8 KiB in flight per wave), reads its x fragments straight from
// global memory (L2-resident: x is at most 32 rows) one block ahead, and owns f32 accumulators for 16 (or 2 x 16) padded rows.
// The partial tiles meet in LDS behind ONE barrier and are summed in wave order (bit-reproducible).  DUAL: half of the waves walk
// the gate tensor, half the up tensor, and the epilogue is silu(gate) * up.
#pragma once
#include "common.cuh"

#define F8_BLOCK 128

// 8 E4M3 bytes -> one 16-bit x 8 MFMA fragment (gfx950 packed converts, scale 1.0: exact — E4M3 has 3 mantissa bits and
// exponents 2^-9 .. 2^8, inside both bf16 and f16)
template <class DT>
__device__ __forceinline__ s16x8 f8x8_to_frag(uint32_t lo, uint32_t hi) {
  u32x4 r;
  if constexpr (DT::id == VRA_BF16) {
    r[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, false));
    r[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, true));
    r[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, false));
    r[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, true));
  } else {
    r[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(lo, 1.0f, false));
    r[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(lo, 1.0f, true));
    r[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(hi, 1.0f, false));
    r[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(hi, 1.0f, true));
  }
  return __builtin_bit_cast(s16x8, r);
}

// ---- load-time repack: checkpoint [N, K] row-major bytes -> tiles.  One thread = one 16-byte lane word.
static __global__ __launch_bounds__(256) void fp8_repack_kernel(const uint8_t* __restrict__ w, u32x4* __restrict__ out, int N, int K) {
  const size_t total = (size_t)(N >> 4) * (K >> 6) * 64;
  const size_t o = blockIdx.x * (size_t)256 + threadIdx.x;
  if (o >= total) return;
  const int lane = (int)(o & 63), KT = K >> 6;
  const size_t tile = o >> 6;
  const int kt = (int)(tile % KT), nb = (int)(tile / KT);
  const uint8_t* src = w + (size_t)(nb * 16 + (lane & 15)) * K + kt * 64 + (lane >> 4) * 8;
  const u32x2 lo = *reinterpret_cast<const u32x2*>(src), hi = *reinterpret_cast<const u32x2*>(src + 32);
  out[o] = u32x4{lo[0], lo[1], hi[0], hi[1]};
}

struct GemvF8Args {
  const void* x;         // [M, K] 16-bit row-major
  const u32x4* w[2];     // tiled weights (DUAL: gate, up)
  const float* sc[2];    // [ceil(N/128), K/128] f32
  const void* bias;      // [N] or null
  const void* residual;  // [M, N] or null
  void* out;             // [M, N]
  int M, K, N;
};

// epilogue of both FP8 kernels for 4 consecutive columns of one row: g = f32 sums (DUAL: u = the up tensor's)
template <class DT, bool DUAL>
__device__ __forceinline__ void f8_epilogue4(const f32x4& g, const f32x4& u, const uint16_t* bias, const uint16_t* res, uint16_t* out) {
  float v[4];
  u32x2 bw = {0u, 0u}, rw = {0u, 0u};
  if (bias) bw = *reinterpret_cast<const u32x2*>(bias);
  if (res) rw = *reinterpret_cast<const u32x2*>(res);
#pragma unroll
  for (int e = 0; e < 4; e++) {
    float t = g[e];
    if (bias) t += DT::to_f32((uint16_t)(bw[e >> 1] >> (16 * (e & 1))));
    if constexpr (DUAL) {
      t = rnd_dt<DT>(t);
      const float up = rnd_dt<DT>(u[e]);
      const float sl = rnd_dt<DT>(t / (1.0f + expf(-t)));
      t = sl * up;
    }
    if (res) t = rnd_dt<DT>(t) + DT::to_f32((uint16_t)(rw[e >> 1] >> (16 * (e & 1))));
    v[e] = t;
  }
  *reinterpret_cast<u32x2*>(out) = u32x2{DT::pack2(v[0], v[1]), DT::pack2(v[2], v[3])};
}

template <class DT, int MT, int WAVES, bool DUAL>
__global__ __launch_bounds__(WAVES * 64) void gemv_f8_kernel(const GemvF8Args a) {
  constexpr int WPT = DUAL ? WAVES / 2 : WAVES;  // waves per tensor
  constexpr int PF = 4;                          // weight blocks in flight per wave
  __shared__ f32x4 red[WAVES * MT * 64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int r16 = lane & 15, q4 = lane >> 4;
  const int ti = DUAL ? wave / WPT : 0, wk = DUAL ? wave % WPT : wave;
  const int nb = (int)blockIdx.x;
  const int K = a.K, M = a.M, KB = K >> 7;
  const int kb0 = KB * wk / WPT, kb1 = KB * (wk + 1) / WPT;  // this wave's K blocks
  const u32x4* __restrict__ wp = a.w[ti] + (size_t)nb * (K >> 6) * 64 + lane;
  const float* __restrict__ sp = a.sc[ti] + (size_t)(nb >> 3) * KB;
  const uint16_t* xr[MT];  // rows past M re-read the last row (their results are never stored)
#pragma unroll
  for (int t = 0; t < MT; t++) xr[t] = static_cast<const uint16_t*>(a.x) + (size_t)min(t * 16 + r16, M - 1) * K + q4 * 8;

  u32x4 wq[PF][2], xq[2][MT][4];
  auto ldw = [&](u32x4 (&d)[2], int kb) {
    const int kc = min(kb, KB - 1);
    d[0] = __builtin_nontemporal_load(wp + (size_t)(2 * kc) * 64);
    d[1] = __builtin_nontemporal_load(wp + (size_t)(2 * kc + 1) * 64);
  };
  auto ldx = [&](u32x4 (&d)[MT][4], int kb) {
    const int kc = min(kb, KB - 1);
#pragma unroll
    for (int t = 0; t < MT; t++)
#pragma unroll
      for (int j = 0; j < 4; j++) d[t][j] = *reinterpret_cast<const u32x4*>(xr[t] + kc * 128 + j * 32);
  };
  f32x4 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; t++) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < PF; i++) ldw(wq[i], kb0 + i);
  ldx(xq[0], kb0);
  for (int kb = kb0; kb < kb1; kb += PF) {
#pragma unroll
    for (int i = 0; i < PF; i++) {
      // past kb1 (a share that is no multiple of PF, or empty: K = 256 on 16 waves): a clamped re-read of another wave's block whose partial
      // sum is scaled by 0 — up to three wasted 2 KiB loads per wave, kept so that the MFMA region stays branch-free
      const int kc = kb + i;
      ldx(xq[(i + 1) & 1], kc + 1);
      const u32x4 c0 = wq[i][0], c1 = wq[i][1];
      ldw(wq[i], kc + PF);
      const float s = kc < kb1 ? sp[min(kc, KB - 1)] : 0.f;
      s16x8 wf[4];
      wf[0] = f8x8_to_frag<DT>(c0[0], c0[1]), wf[1] = f8x8_to_frag<DT>(c0[2], c0[3]);
      wf[2] = f8x8_to_frag<DT>(c1[0], c1[1]), wf[3] = f8x8_to_frag<DT>(c1[2], c1[3]);
      f32x4 part[MT];
#pragma unroll
      for (int t = 0; t < MT; t++) DT::mfma0(part[t], wf[0], __builtin_bit_cast(s16x8, xq[i & 1][t][0]));
#pragma unroll
      for (int j = 1; j < 4; j++)
#pragma unroll
        for (int t = 0; t < MT; t++) DT::mfma(part[t], wf[j], __builtin_bit_cast(s16x8, xq[i & 1][t][j]));
      VRA_MFMA_DRAIN();
#pragma unroll
      for (int t = 0; t < MT; t++)
#pragma unroll
        for (int e = 0; e < 4; e++) acc[t][e] = __builtin_fmaf(s, part[t][e], acc[t][e]);
    }
  }
  // ---- the waves' partial tiles meet in LDS; wave t sums row tile t in wave order and writes it
#pragma unroll
  for (int t = 0; t < MT; t++) red[(wave * MT + t) * 64 + lane] = acc[t];
  __syncthreads();
  if (wave >= MT) return;
  const int row = wave * 16 + r16, n = nb * 16 + q4 * 4;
  f32x4 g = {0.f, 0.f, 0.f, 0.f}, u = {0.f, 0.f, 0.f, 0.f};
  for (int w = 0; w < WPT; w++) {
    const f32x4 p = red[(w * MT + wave) * 64 + lane];
#pragma unroll
    for (int e = 0; e < 4; e++) g[e] += p[e];
    if (DUAL) {
      const f32x4 pu = red[((WPT + w) * MT + wave) * 64 + lane];
#pragma unroll
      for (int e = 0; e < 4; e++) u[e] += pu[e];
    }
  }
  if (row >= M) return;
  const size_t o = (size_t)row * a.N + n;
  f8_epilogue4<DT, DUAL>(g, u, a.bias ? static_cast<const uint16_t*>(a.bias) + n : nullptr,
                         a.residual ? static_cast<const uint16_t*>(a.residual) + o : nullptr, static_cast<uint16_t*>(a.out) + o);
}
