// gemv_mx4.cuh — MXFP4 weights (E2M1 nibbles + one E8M0 scale byte per 32-wide K block, W4A16): the tile layout, its repack, the
// decode kernel for 1..32 rows and the pass that widens a tensor into kernel X's fragment format for longer steps.
//
// Format (compressed-tensors `mxfp4-pack-quantized`; reference: LnMxfp4, src/models/layers/linear.rs:1078-1144): weight_packed
// [N, K/2] bytes, byte i of a row = k = 2i in the low nibble, 2i + 1 in the high one, a code = sign | 2 exponent bits | 1 mantissa bit
// (0, 1/2, 1, 3/2, 2, 3, 4, 6); weight_scale [N, K/32] bytes b, the block's scale is 2^(b - 127).
//
// Arithmetic: w = E2M1 * 2^(b - 127) is EXACT in the model dtype (precondition on b: bf16 2..252, f16 114..140), so the
// scale is applied by the convert itself (v_cvt_scalef32_pk_{bf16,f16}_fp4: two codes of one selected byte -> a 16-bit pair, times the
// power of two in the f32 operand's exponent field) and the weights go through v_mfma_f32_16x16x32 as ordinary 16-bit operands.  f32
// products and sums, ONE rounding at the output, the same real function at every row count — nothing is rounded before the sum.
//
// Tile layout: 1 KiB tile = 16 columns x 128 k.  word[((nb * K/128 + kt) * 64 + lane) * 4 + j] holds the 8 codes
// w[nb * 16 + (lane & 15)][kt * 128 + j * 32 + (lane >> 4) * 8 + 0..7] in the checkpoint's nibble order (four consecutive checkpoint
// bytes): one 16-byte load per lane is the weight operand of FOUR MFMA K-steps, each made by four byte-selected converts, no cross-lane
// movement.  One K-step is one MX block, so the scale is per lane and per step: s_tiled[(nb * K/128 + kt) * 16 + c] is a u32 whose
// byte j is the scale byte of column nb * 16 + c, block kt * 4 + j — 64 B beside each 1 KiB tile, a lane loads one word per tile and
// makes step j's f32 scale operand with a shift and a mask.  A unit (16 columns over the full K) is one contiguous run of 8 * K bytes.
//
// Decode kernel — HBM-bound at 0.53 B per weight.  The decisions:
//   * the scale is folded into the operand, so ONE accumulator per row tile runs straight through the wave's K range in the MFMA's C
//     registers; no per-block fma, no partial tile (the FP8 kernel's `part` + 4 fma per block are gone);
//   * a workgroup owns ONE unit (8 * K bytes; DUAL: the gate unit and the up unit of the same 16 columns, 16 * K bytes) and its 4 / 8 / 16
//     waves split K in whole tiles; the host picks the wave count so that a CU holds ~16 streaming waves whatever N is (two row tiles or
//     two tensors: at most 8, the 128 registers of a 16-wave workgroup hold one row tile of one tensor).  A wave keeps
//     a register ring of PF = 4 tiles per tensor in flight (4 KiB, DUAL 8 KiB: 64..128 KiB per CU, above the ~32 KiB at which a CU is
//     latency-bound).  More units per workgroup would only pay by sharing x, and at N = 4096 (256 units = the CU count)
//     there is no second unit to give a workgroup without idling half the chip;
//   * DUAL: EVERY wave walks the gate and the up tile of its K range against the SAME x fragments (the FP8 kernel gives half of the
//     waves to each tensor and reads x twice) — gate/up is the widest GEMM of a layer and its x traffic halves;
//   * all three streams are raw buffer loads whose offset is pushed out of range past the wave's last tile: the hardware returns 0 without
//     touching memory, code 0 is +0.0, so a K share that is no multiple of the ring (K = 4096 on 16 waves is 2 tiles per wave) costs
//     neither traffic nor a branch in the MFMA region, and no lane can read outside its tensor;
//   * x for the second row tile is NOT staged through LDS: the waves of a workgroup split K, so every x byte a workgroup needs is
//     already read exactly once — by the one wave that owns its k range, straight into the MFMA operand registers (lane = row, 16 B =
//     8 k).  An LDS stage would add a write, a barrier and a read to the same L2 traffic.  What doubles from 16 to 32 rows is that L2
//     traffic itself (32 rows x K x 2 B per workgroup against 8 * K weight bytes); only more columns per workgroup divide it, which is
//     what DUAL does.  tools/mxfp4_gemm_bench.py records 16 against 32 rows;
//   * the waves' partial 16 x 16 tiles meet in LDS behind ONE barrier and are summed in wave order: no atomics, bit-reproducible.
#pragma once
#include "gemv_f8.cuh"

// 8 E2M1 codes of one word, times 2^(byte - 127) -> one 16-bit x 8 MFMA fragment
template <class DT>
__device__ __forceinline__ s16x8 mx4_word_to_frag(uint32_t word, float scale) {
  u32x4 r;
  if constexpr (DT::id == VRA_BF16) {
    r[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(word, scale, 0));
    r[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(word, scale, 1));
    r[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(word, scale, 2));
    r[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(word, scale, 3));
  } else {
    r[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(word, scale, 0));
    r[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(word, scale, 1));
    r[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(word, scale, 2));
    r[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(word, scale, 3));
  }
  return __builtin_bit_cast(s16x8, r);
}
// byte j of a tile's scale word -> the f32 whose exponent field is that byte (2^(b - 127) for b >= 1)
__device__ __forceinline__ float mx4_scale(uint32_t sw, int j) {
  return __uint_as_float((j < 3 ? sw << (23 - 8 * j) : sw >> 1) & 0x7F800000u);
}

// ---- load-time repack: checkpoint rows -> tiles.  One thread = one 16-byte lane word; the first 16 lanes of a tile also write its scale words.
// (static: this header is included by more than one translation unit)
static __global__ __launch_bounds__(256) void mx4_repack_kernel(const uint8_t* __restrict__ w, const uint8_t* __restrict__ sc, u32x4* __restrict__ wt,
                                                         uint32_t* __restrict__ st, int N, int K) {
  const int KT = K >> 7;
  const size_t total = (size_t)(N >> 4) * KT * 64;
  const size_t o = blockIdx.x * (size_t)256 + threadIdx.x;
  if (o >= total) return;
  const int lane = (int)(o & 63);
  const size_t tile = o >> 6;
  const int kt = (int)(tile % KT), nb = (int)(tile / KT);
  const size_t n = (size_t)nb * 16 + (lane & 15);
  const uint32_t* src = reinterpret_cast<const uint32_t*>(w + n * (K >> 1) + kt * 64 + (lane >> 4) * 4);  // (rows are K/2 bytes, a multiple of 64)
  wt[o] = u32x4{src[0], src[4], src[8], src[12]};
  if (lane < 16) st[tile * 16 + lane] = reinterpret_cast<const uint32_t*>(sc + n * (K >> 5))[kt];
}

// ---- the pass for steps above 32 rows: tiles -> kernel X's 1 KiB fragments (16 columns x 32 k in lane order; gemm_dense.cuh), the unit
// nb of tensor t at virtual n-frag vfrag0[t] + nb * vstride[t] (gate / up: 0 / 1, stride 2).  One thread = one lane word -> four fragments' lane words.
struct Mx4FragBatch {
  const u32x4* w[2];
  const uint32_t* sc[2];
  int N[2], vfrag0[2], vstride[2];
};
template <class DT>
__global__ __launch_bounds__(256) void mxfp4_dequant_frag_kernel(const Mx4FragBatch b, u32x4* __restrict__ wd, int K) {
  const int ti = (int)blockIdx.y, KT = K >> 7;
  const size_t total = (size_t)(b.N[ti] >> 4) * KT * 64;
  const size_t o = blockIdx.x * (size_t)256 + threadIdx.x;
  if (o >= total) return;
  const int lane = (int)(o & 63);
  const size_t tile = o >> 6;
  const int kt = (int)(tile % KT), nb = (int)(tile / KT);
  const u32x4 w = __builtin_nontemporal_load(b.w[ti] + o);
  const uint32_t sw = b.sc[ti][tile * 16 + (lane & 15)];
  const size_t fbase = ((size_t)(b.vfrag0[ti] + nb * b.vstride[ti]) * (K >> 5) + (size_t)kt * 4) * 64 + lane;
#pragma unroll
  for (int j = 0; j < 4; j++) wd[fbase + (size_t)j * 64] = __builtin_bit_cast(u32x4, mx4_word_to_frag<DT>(w[j], mx4_scale(sw, j)));
}

struct GemvMx4Args {
  const void* x;         // [M, K] 16-bit row-major
  const void* w[2];      // tiled weights (DUAL: gate, up)
  const void* sc[2];     // tiled scale words
  const void* bias;      // [N] or null
  const void* residual;  // [M, N] or null
  void* out;             // [M, N]
  int M, K, N;
};

#define MX4_OOB 0x7FFFFFF0  // a buffer offset past every tensor this path accepts (all are under that many bytes): the load returns 0

template <class DT, int MT, int WAVES, bool DUAL>
__global__ __launch_bounds__(WAVES * 64) void gemv_mx4_kernel(const GemvMx4Args a) {
  constexpr int NT = DUAL ? 2 : 1;  // tensors every wave walks
  constexpr int PF = 4;             // tiles in flight per wave and tensor (even: the x double buffer keeps its parity across iterations)
  constexpr uint32_t RSRC3 = 0x00020000u;
  __shared__ f32x4 red[WAVES * NT * MT * 64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int r16 = lane & 15, q4 = lane >> 4;
  const int nb = (int)blockIdx.x;
  const int K = a.K, M = a.M, KT = K >> 7;
  const int kt0 = KT * wave / WAVES, kt1 = KT * (wave + 1) / WAVES;  // this wave's tiles
  // buffers: the unit's run of each tensor (8 * K bytes of tiles, K / 2 bytes of scale words) and the whole of x
  __amdgpu_buffer_rsrc_t rw[NT], rs[NT];
#pragma unroll
  for (int n = 0; n < NT; n++) {
    rw[n] = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(static_cast<const uint8_t*>(a.w[n]) + (size_t)nb * KT * 1024), 0, KT * 1024, RSRC3);
    rs[n] = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(static_cast<const uint8_t*>(a.sc[n]) + (size_t)nb * KT * 64), 0, KT * 64, RSRC3);
  }
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.x), 0, (int)((size_t)M * K * 2), RSRC3);
  int xo[MT];  // rows past M re-read the last row (their results are never stored)
#pragma unroll
  for (int t = 0; t < MT; t++) xo[t] = (min(t * 16 + r16, M - 1) * K + q4 * 8) * 2;

  u32x4 wq[PF][NT], xq[2][MT][4];
  uint32_t sq[PF][NT];
  auto ldw = [&](u32x4 (&d)[NT], uint32_t (&s)[NT], int kt) {
    const bool in = kt < kt1;
#pragma unroll
    for (int n = 0; n < NT; n++) {
      d[n] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rw[n], in ? kt * 1024 + lane * 16 : MX4_OOB, 0, 2));  // (aux 2: streamed once)
      s[n] = __builtin_amdgcn_raw_buffer_load_b32(rs[n], in ? kt * 64 + r16 * 4 : MX4_OOB, 0, 0);
    }
  };
  auto ldx = [&](u32x4 (&d)[MT][4], int kt) {
    const bool in = kt < kt1;
#pragma unroll
    for (int t = 0; t < MT; t++)
#pragma unroll
      for (int j = 0; j < 4; j++) d[t][j] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rx, in ? xo[t] + kt * 256 + j * 64 : MX4_OOB, 0, 0));
  };
  f32x4 acc[NT][MT];
#pragma unroll
  for (int n = 0; n < NT; n++)
#pragma unroll
    for (int t = 0; t < MT; t++) acc[n][t] = vra_zero_acc();
#pragma unroll
  for (int i = 0; i < PF; i++) ldw(wq[i], sq[i], kt0 + i);
  ldx(xq[0], kt0);
  for (int kt = kt0; kt < kt1; kt += PF) {
#pragma unroll
    for (int i = 0; i < PF; i++) {
      const int kc = kt + i;
      ldx(xq[(i + 1) & 1], kc + 1);
      u32x4 c[NT];
      uint32_t s[NT];
#pragma unroll
      for (int n = 0; n < NT; n++) c[n] = wq[i][n], s[n] = sq[i][n];
      ldw(wq[i], sq[i], kc + PF);
#pragma unroll
      for (int n = 0; n < NT; n++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const s16x8 wf = mx4_word_to_frag<DT>(c[n][j], mx4_scale(s[n], j));
#pragma unroll
          for (int t = 0; t < MT; t++) DT::mfma(acc[n][t], wf, __builtin_bit_cast(s16x8, xq[i & 1][t][j]));
        }
    }
  }
  VRA_MFMA_DRAIN();
  // ---- the waves' partial tiles meet in LDS; wave t sums row tile t in wave order and writes it
#pragma unroll
  for (int n = 0; n < NT; n++)
#pragma unroll
    for (int t = 0; t < MT; t++) red[((wave * NT + n) * MT + t) * 64 + lane] = acc[n][t];
  __syncthreads();
  if (wave >= MT) return;
  const int row = wave * 16 + r16, col = nb * 16 + q4 * 4;
  f32x4 g = {0.f, 0.f, 0.f, 0.f}, u = {0.f, 0.f, 0.f, 0.f};
  for (int w = 0; w < WAVES; w++) {
    const f32x4 p = red[((w * NT) * MT + wave) * 64 + lane];
#pragma unroll
    for (int e = 0; e < 4; e++) g[e] += p[e];
    if (DUAL) {
      const f32x4 pu = red[((w * NT + NT - 1) * MT + wave) * 64 + lane];
#pragma unroll
      for (int e = 0; e < 4; e++) u[e] += pu[e];
    }
  }
  if (row >= M) return;
  const size_t o = (size_t)row * a.N + col;
  f8_epilogue4<DT, DUAL>(g, u, a.bias ? static_cast<const uint16_t*>(a.bias) + col : nullptr,
                         a.residual ? static_cast<const uint16_t*>(a.residual) + o : nullptr, static_cast<uint16_t*>(a.out) + o);
}
