// gemm_f8.cuh — the prefill GEMM (33+ rows) on FP8 E4M3 block-scaled weights in the tile layout of gemv_f8.cuh.  MFMA-bound.
//
// Output tile BM x 128 virtual columns (BM = 256 | 128, chosen per shape), one wave per 64 rows x 64 columns (BM/64 x 2 waves), K
// walked in 128-wide scale blocks of two 64-wide K-steps (LDS buffer 0, then 1):
//   * both operands travel global -> LDS by LDS-DMA, 1 KiB per wave instruction: x as 16-row x 32-k MFMA fragments (fetched row by
//     row with the XOR chunk swizzle of gemm_dense.cuh, so `ds_read_b128` is conflict-free), the weights as the FP8 tiles THEMSELVES
//     (16 columns x 64 k in 1 KiB: half the LDS and HBM traffic of a 16-bit weight operand, no dequant pass, no scratch tensor);
//   * a wave reads its four weight tiles once per K-step (one `ds_read_b128` each = both 32-k halves) and widens them in registers:
//     32 packed converts per 32 MFMAs;
//   * two accumulator sets: `part` takes the MFMAs of one 128-k block (the first MFMA of each chain has C = 0), then ONE wave-uniform
//     scale per fragment column folds it into `acc` by f32 fma — a wave's 64 columns lie inside one 128-column scale row.
//     16 + 16 tiles = 128 accumulator registers;
//   * while a K-step computes, the next one lands in the other buffer: a wave waits for its own DMA with a counted vmcnt (the newest
//     K-step stays in flight) and a barrier publishes it; a second barrier frees the buffer for re-staging;
//   * ragged M / N: staging clamps to the last row / last 16-column unit, the epilogue stores only what exists;
//   * DUAL: the eight tiles of a K-step alternate gate, up (g0 u0 g1 u1 ...), so a wave holds gate and up of the same 32 output
//     columns, each with its own tensor's scale, and the epilogue is silu(gate) * up.
#pragma once
#include <type_traits>

#include "gemv_f8.cuh"

struct GemmF8Args {
  const void* x;  // [M, K] 16-bit row-major
  const void* w[2];
  const float* sc[2];
  const void* bias;
  const void* residual;
  void* out;    // [M, N]
  int M, K, N;  // N = output columns (DUAL: of each tensor)
  int MT, NT;
};

static inline size_t gemm_f8_lds_bytes(int bm) { return (size_t)2 * ((size_t)bm * 128 + 8 * 1024); }

template <class DT, int BM, bool DUAL>
__global__ __launch_bounds__(BM * 2, 2) void gemm_f8_kernel(const GemmF8Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int NW = BM / 32;      // waves: BM/64 (m) x 2 (n)
  constexpr int NXU = BM / 8;      // x fragments of a K-step (BM/16 m-frags x 2 k-chunks)
  constexpr int XB = NXU * 1024;   // bytes of x per buffer
  constexpr int BUF = XB + 8 * 1024;
  constexpr int XPW = NXU / NW;    // x DMA instructions per wave and K-step (4)
  constexpr int WPW = 8 / NW;      // weight tiles per wave and K-step (1 | 2)
  constexpr uint32_t RSRC3 = 0x00020000u;
  static_assert(BM == 256 || BM == 128, "tile height");
  static_assert(XPW == 4 && NXU % NW == 0 && 8 % NW == 0, "staging split");

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 1, wc = wave & 1;
  const int r16 = lane & 15, q4 = lane >> 4;
  const int K = a.K, M = a.M, N = a.N, KB = K >> 7, KS = K >> 6;
  const int mt = (int)blockIdx.x % a.MT, nt = (int)blockIdx.x / a.MT;
  const int m0 = mt * BM;
  const int nunits = N >> 4;

  // ---- LDS-DMA sources
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.x), 0, 0x7FFFFFF0, RSRC3);
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.w[DUAL ? (wave & 1) : 0]), 0, 0x7FFFFFF0, RSRC3);
  const int srow = lane >> 2, schunk = (lane & 3) ^ ((srow >> 2) & 3);
  uint32_t vo_x[4];  // x unit u = wave + i * NW: m-frag u >> 1, k-chunk u & 1
#pragma unroll
  for (int i = 0; i < XPW; i++)
    vo_x[i] = ((uint32_t)min(m0 + ((wave + i * NW) >> 1) * 16 + srow, M - 1) * (uint32_t)K + (uint32_t)schunk * 8u) * 2u;
  uint32_t so_w[2];  // tile f = wave + i * NW of the K-step: unit nt * 8 + f (DUAL: tensor f & 1 = wave & 1, unit nt * 4 + (f >> 1))
#pragma unroll
  for (int i = 0; i < WPW; i++) {
    const int f = wave + i * NW;
    so_w[i] = (uint32_t)min(DUAL ? nt * 4 + (f >> 1) : nt * 8 + f, nunits - 1) * (uint32_t)K * 16u;
  }
  typedef __attribute__((address_space(3))) void* lds_ptr;
  auto stage = [&](int buf, int ks) {  // XPW + WPW DMA instructions per wave
    unsigned char* d = smem + buf * BUF;
#pragma unroll
    for (int i = 0; i < XPW; i++) {
      const int u = wave + i * NW;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (lds_ptr)(d + u * 1024), 16, vo_x[i], (uint32_t)ks * 128u + (uint32_t)(u & 1) * 64u, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < WPW; i++)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lds_ptr)(d + XB + (wave + i * NW) * 1024), 16, (uint32_t)lane * 16u, so_w[i] + (uint32_t)ks * 1024u, 0, 0);
  };
#define GF8_WAIT_VM()                                                              \
  do {                                                                             \
    if constexpr (XPW + WPW == 5) asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); \
    else asm volatile("s_waitcnt vmcnt(6)" ::: "memory");                          \
  } while (0)

  const unsigned char* xrd = smem + (wr * 4) * 2048 + (r16 * 4 + (q4 ^ ((r16 >> 2) & 3))) * 16;
  const unsigned char* wrd = smem + XB + (wc * 4) * 1024 + lane * 16;
  f32x4 acc[4][4], part[4][4];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto compute = [&](auto FIRST, int buf) {  // one K-step: A = weights (16 columns x 32 k), B = x (16 rows x 32 k): D[column][row]
    constexpr bool first = decltype(FIRST)::value;
    u32x4 wt[4];
    s16x8 xa[4][2], wf[4][2];
#pragma unroll
    for (int j = 0; j < 4; j++) wt[j] = *reinterpret_cast<const u32x4*>(wrd + buf * BUF + j * 1024);
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int kc = 0; kc < 2; kc++) xa[i][kc] = *reinterpret_cast<const s16x8*>(xrd + buf * BUF + (i * 2 + kc) * 1024);
#pragma unroll
    for (int j = 0; j < 4; j++) wf[j][0] = f8x8_to_frag<DT>(wt[j][0], wt[j][1]), wf[j][1] = f8x8_to_frag<DT>(wt[j][2], wt[j][3]);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int kc = 0; kc < 2; kc++)
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
          if constexpr (first) {
            if (kc == 0) DT::mfma0(part[i][j], wf[j][kc], xa[i][kc]);
            else DT::mfma(part[i][j], wf[j][kc], xa[i][kc]);
          } else {
            DT::mfma(part[i][j], wf[j][kc], xa[i][kc]);
          }
        }
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
  };

  const float* __restrict__ sc0 = a.sc[0] + (size_t)(DUAL ? nt >> 1 : nt) * KB;
  const float* __restrict__ sc1 = DUAL ? a.sc[1] + (size_t)(nt >> 1) * KB : sc0;
  stage(0, 0);
  for (int kb = 0; kb < KB; kb++) {
    const float s0 = sc0[kb], s1 = sc1[kb];
    stage(1, 2 * kb + 1);
    GF8_WAIT_VM();  // this wave's share of K-step 2 kb has landed; the barrier publishes everyone's
    __builtin_amdgcn_s_barrier();
    compute(std::true_type{}, 0);
    __builtin_amdgcn_s_barrier();  // buffer 0 is free
    stage(0, min(2 * kb + 2, KS - 1));
    GF8_WAIT_VM();
    __builtin_amdgcn_s_barrier();
    compute(std::false_type{}, 1);
    __builtin_amdgcn_s_barrier();
    VRA_MFMA_DRAIN();
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const float s = (j & 1) ? s1 : s0;
#pragma unroll
        for (int e = 0; e < 4; e++) acc[i][j][e] = __builtin_fmaf(s, part[i][j][e], acc[i][j][e]);
      }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the clamped staging of the last K-step
#undef GF8_WAIT_VM

  // ---- epilogue: a lane holds 4 consecutive columns of one row per accumulator tile
  constexpr int NOUT = DUAL ? 2 : 4;
#pragma unroll
  for (int jo = 0; jo < NOUT; jo++) {
    const int j = DUAL ? 2 * jo : jo;
    const int n = (DUAL ? nt * 64 + wc * 32 : nt * 128 + wc * 64) + jo * 16 + q4 * 4;
    if (n >= N) continue;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int row = m0 + wr * 64 + i * 16 + r16;
      if (row >= M) continue;
      const size_t o = (size_t)row * N + n;
      f8_epilogue4<DT, DUAL>(acc[i][j], acc[i][DUAL ? j + 1 : j], a.bias ? static_cast<const uint16_t*>(a.bias) + n : nullptr,
                             a.residual ? static_cast<const uint16_t*>(a.residual) + o : nullptr, static_cast<uint16_t*>(a.out) + o);
    }
  }
}
