// gemv_nv4.cuh — NVFP4 weights (E2M1 nibbles + one E4M3 scale byte per 16-wide K group + one f32 scale per tensor, W4A16): the tile
// layout, its repack, the decode kernel for 1..32 rows and the pass that widens a tensor into kernel X's fragment format for longer steps.
//
// Format (ModelOpt / compressed-tensors `nvfp4-pack-quantized`; reference: LnNvfp4, src/models/layers/linear.rs:1146-1306): codes
// [N, K/2] bytes in the MXFP4 nibble order (k = 2i in the low nibble of byte i), group scales [N, K/16] OCP E4M3 bytes, a global f32
// scale g (a host value here: 1 / weight_global_scale, or weight_scale_2).
//
// Arithmetic: w = E2M1(code) * E4M3(scale byte) is EXACT in bf16 and in f16 for every non-NaN scale byte (a 2-bit times
// a 4-bit significand needs 5 bits; 2^-10 <= |w| <= 2688 lies in both formats' normal ranges), so the weights go through
// v_mfma_f32_16x16x32 as ordinary 16-bit operands.  out = round(g * sum x w (+ bias)): f32 products and sums, g applied ONCE to the
// finished f32 sum, ONE rounding, the same real function at every row count.
//
// Operand build — what differs from gemv_mx4.cuh.  The scaled converts take only a power of two from their scale operand, the E4M3
// scale has a mantissa, so it is multiplied in.  A lane word is 8 codes of ONE group (a lane holds k = q4 * 8 .. + 7 of a 32-wide step,
// half of one 16-wide group), so one scale serves the whole word:
//   scale   v_cvt_f32_fp8 with the byte select (OCP on gfx950): byte j of the lane's scale word -> f32, no shift or mask;
//   bf16    4 x v_cvt_scalef32_pk_f32_fp4 (scale operand 1.0) -> 4 x v_pk_mul_f32 -> 4 x v_perm_b32 taking the products' high halves
//           (a product has <= 5 significant bits: the truncation drops zeros only) — 13 VALU per 8 weights against MXFP4's 4;
//   f16     the scale once to f16 (exact: 2^-9 .. 448), 4 x v_cvt_scalef32_pk_f16_fp4 -> 4 x v_pk_mul_f16 — 10 VALU per 8 weights.
// (Considered: the scale's exponent through the convert and the mantissa as an integer add into the 16-bit fields.  1.5 * (1 + m/8)
// carries into the exponent for m >= 3 and code 0 must stay 0, so it needs a compare and selects per pair — not cheaper.)
//
// Tile layout: the codes use the MXFP4 tile unchanged — 1 KiB = 16 columns x 128 k, word[((nb * K/128 + kt) * 64 + lane)
// * 4 + j] = the 8 codes w[nb * 16 + (lane & 15)][kt * 128 + j * 32 + (lane >> 4) * 8 + 0..7].  The group of that word is
// kt * 8 + 2j + h with h = lane >> 5, so the scales sit as s_tiled[((nb * K/128 + kt) * 2 + h) * 16 + c], a u32 whose byte j is the scale
// byte of column nb * 16 + c, group kt * 8 + 2j + h: 128 B beside each 1 KiB tile, ONE 32-bit load per lane and tile.
//
// Decode kernel: gemv_mx4.cuh's structure, which its measurements support (one workgroup per 16-column unit, 4 / 8 / 16 waves splitting
// K in whole tiles, a register ring per wave and tensor, raw buffer loads returning 0 past a wave's last tile — code 0 is +0.0 and scale
// byte 0 is +0.0 —, x straight into operand registers one tile ahead, DUAL waves walking gate and up against the same x, partial tiles
// summed in LDS in wave order).  Wave counts and ring depth against the register budget (-Rpass-analysis=kernel-resource-usage, no
// scratch anywhere): a 16-wave workgroup leaves 128 registers per wave and runs one row tile of one tensor only — 81 (bf16) / 79 (f16)
// with a ring of 4 tiles, so the ring keeps MXFP4's 4 KiB per wave and tensor although the scale stream doubled and a bf16 word's f32
// products are 8 more live registers; an 8-wave workgroup leaves 256 and its heaviest instantiation (two row tiles, gate and up) takes
// 161 (bf16) / 185 (f16).  Deeper rings were not tried.
#pragma once
#include "gemv_f8.cuh"

typedef float nv4_f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 nv4_f16x2 __attribute__((ext_vector_type(2)));

// 8 E2M1 codes of one word, times the E4M3 scale in byte J of the lane's scale word -> one 16-bit x 8 MFMA fragment (exact)
template <class DT, int J>
__device__ __forceinline__ s16x8 nv4_word_to_frag(uint32_t word, uint32_t sw) {
  const float sf = __builtin_amdgcn_cvt_f32_fp8((int)sw, J);
  u32x4 r;
  if constexpr (DT::id == VRA_BF16) {
    const nv4_f32x2 s2 = {sf, sf};
#define NV4_PAIR(i)                                                                                        \
  {                                                                                                        \
    const nv4_f32x2 p = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(word, 1.0f, i) * s2;                      \
    r[i] = __builtin_amdgcn_perm(__float_as_uint(p[1]), __float_as_uint(p[0]), 0x07060302u); /* hi halves */ \
  }
    NV4_PAIR(0) NV4_PAIR(1) NV4_PAIR(2) NV4_PAIR(3)
#undef NV4_PAIR
  } else {
    const _Float16 sh = (_Float16)sf;
    const nv4_f16x2 s2 = {sh, sh};
    r[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(word, 1.0f, 0) * s2);
    r[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(word, 1.0f, 1) * s2);
    r[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(word, 1.0f, 2) * s2);
    r[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(word, 1.0f, 3) * s2);
  }
  return __builtin_bit_cast(s16x8, r);
}

// ---- load-time repack: checkpoint rows -> tiles.  One thread = one 16-byte lane word; lanes 0..31 of a tile also write its 32 scale words.
__global__ __launch_bounds__(256) void nv4_repack_kernel(const uint8_t* __restrict__ w, const uint8_t* __restrict__ sc, u32x4* __restrict__ wt,
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
  if (lane < 32) {  // h = lane >> 4: the even (0) or odd (1) groups of the tile's eight
    const uint32_t* s8 = reinterpret_cast<const uint32_t*>(sc + n * (K >> 4) + kt * 8);  // (rows are K/16 bytes, a multiple of 8)
    const int sh = (lane >> 4) * 8;
    const uint32_t lo = s8[0] >> sh, hi = s8[1] >> sh;  // bytes 0 / 2 hold groups h, 2 + h | 4 + h, 6 + h
    st[tile * 32 + lane] = (lo & 0xFFu) | ((lo >> 8) & 0xFF00u) | ((hi & 0xFFu) << 16) | ((hi << 8) & 0xFF000000u);
  }
}

// ---- the pass for steps above 32 rows: tiles -> kernel X's 1 KiB fragments (16 columns x 32 k in lane order; gemm_dense.cuh) holding
// the exact w WITHOUT g (g * w would need a rounding: kernel X applies g to its finished f32 sums, GemmXArgs::acc_scale).  Unit nb of
// tensor t goes to virtual n-frag vfrag0[t] + nb * vstride[t] (gate / up: 0 / 1, stride 2).  One thread = one lane word -> four fragments' lane words.
struct Nv4FragBatch {
  const u32x4* w[2];
  const uint32_t* sc[2];
  int N[2], vfrag0[2], vstride[2];
};
template <class DT>
__global__ __launch_bounds__(256) void nvfp4_dequant_frag_kernel(const Nv4FragBatch b, u32x4* __restrict__ wd, int K) {
  const int ti = (int)blockIdx.y, KT = K >> 7;
  const size_t total = (size_t)(b.N[ti] >> 4) * KT * 64;
  const size_t o = blockIdx.x * (size_t)256 + threadIdx.x;
  if (o >= total) return;
  const int lane = (int)(o & 63);
  const size_t tile = o >> 6;
  const int kt = (int)(tile % KT), nb = (int)(tile / KT);
  const u32x4 w = __builtin_nontemporal_load(b.w[ti] + o);
  const uint32_t sw = b.sc[ti][tile * 32 + (lane >> 5) * 16 + (lane & 15)];
  u32x4* const f = wd + ((size_t)(b.vfrag0[ti] + nb * b.vstride[ti]) * (K >> 5) + (size_t)kt * 4) * 64 + lane;
  f[0] = __builtin_bit_cast(u32x4, nv4_word_to_frag<DT, 0>(w[0], sw));
  f[64] = __builtin_bit_cast(u32x4, nv4_word_to_frag<DT, 1>(w[1], sw));
  f[128] = __builtin_bit_cast(u32x4, nv4_word_to_frag<DT, 2>(w[2], sw));
  f[192] = __builtin_bit_cast(u32x4, nv4_word_to_frag<DT, 3>(w[3], sw));
}

struct GemvNv4Args {
  const void* x;         // [M, K] 16-bit row-major
  const void* w[2];      // tiled codes (DUAL: gate, up)
  const void* sc[2];     // tiled scale words
  float g[2];            // the tensors' global scales
  const void* bias;      // [N] or null
  const void* residual;  // [M, N] or null
  void* out;             // [M, N]
  int M, K, N;
};

#define NV4_OOB 0x7FFFFFF0  // a buffer offset past every tensor this path accepts (all are under that many bytes): the load returns 0

template <class DT, int MT, int WAVES, bool DUAL>
__global__ __launch_bounds__(WAVES * 64) void gemv_nv4_kernel(const GemvNv4Args a) {
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
  // buffers: the unit's run of each tensor (8 * K bytes of tiles, K bytes of scale words) and the whole of x
  __amdgpu_buffer_rsrc_t rw[NT], rs[NT];
#pragma unroll
  for (int n = 0; n < NT; n++) {
    rw[n] = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(static_cast<const uint8_t*>(a.w[n]) + (size_t)nb * KT * 1024), 0, KT * 1024, RSRC3);
    rs[n] = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(static_cast<const uint8_t*>(a.sc[n]) + (size_t)nb * KT * 128), 0, KT * 128, RSRC3);
  }
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.x), 0, (int)((size_t)M * K * 2), RSRC3);
  int xo[MT];  // rows past M re-read the last row (their results are never stored)
#pragma unroll
  for (int t = 0; t < MT; t++) xo[t] = (min(t * 16 + r16, M - 1) * K + q4 * 8) * 2;
  const int so = (q4 >> 1) * 64 + r16 * 4;  // the lane's scale word inside a tile's 128 bytes

  u32x4 wq[PF][NT], xq[2][MT][4];
  uint32_t sq[PF][NT];
  auto ldw = [&](u32x4 (&d)[NT], uint32_t (&s)[NT], int kt) {
    const bool in = kt < kt1;
#pragma unroll
    for (int n = 0; n < NT; n++) {
      d[n] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rw[n], in ? kt * 1024 + lane * 16 : NV4_OOB, 0, 2));  // (aux 2: streamed once)
      s[n] = __builtin_amdgcn_raw_buffer_load_b32(rs[n], in ? kt * 128 + so : NV4_OOB, 0, 0);
    }
  };
  auto ldx = [&](u32x4 (&d)[MT][4], int kt) {
    const bool in = kt < kt1;
#pragma unroll
    for (int t = 0; t < MT; t++)
#pragma unroll
      for (int j = 0; j < 4; j++) d[t][j] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rx, in ? xo[t] + kt * 256 + j * 64 : NV4_OOB, 0, 0));
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
      for (int n = 0; n < NT; n++) {
        const s16x8 wf[4] = {nv4_word_to_frag<DT, 0>(c[n][0], s[n]), nv4_word_to_frag<DT, 1>(c[n][1], s[n]),
                             nv4_word_to_frag<DT, 2>(c[n][2], s[n]), nv4_word_to_frag<DT, 3>(c[n][3], s[n])};
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
          for (int t = 0; t < MT; t++) DT::mfma(acc[n][t], wf[j], __builtin_bit_cast(s16x8, xq[i & 1][t][j]));
      }
    }
  }
  VRA_MFMA_DRAIN();
  // ---- the waves' partial tiles meet in LDS; wave t sums row tile t in wave order, applies the global scales and writes it
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
#pragma unroll
  for (int e = 0; e < 4; e++) g[e] *= a.g[0], u[e] *= a.g[1];
  const size_t o = (size_t)row * a.N + col;
  f8_epilogue4<DT, DUAL>(g, u, a.bias ? static_cast<const uint16_t*>(a.bias) + col : nullptr,
                         a.residual ? static_cast<const uint16_t*>(a.residual) + o : nullptr, static_cast<uint16_t*>(a.out) + o);
}
