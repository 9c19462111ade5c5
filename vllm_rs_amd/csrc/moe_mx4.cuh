// moe_mx4.cuh — the expert GEMMs of the mixture-of-experts block on MXFP4 experts (E2M1 nibbles + one E8M0 byte per 32-wide K block, W4A16;
// reference: FusedMoeMxfp4, src/models/layers/moe.rs: per-expert [I, H/2] packed bytes and [I, H/32] scale bytes, SiLU-gated).  Routing,
// alignment, the h epilogue and the combine are those of moe.cuh; the workspace is the one vra_moe_workspace_bytes sizes.
//
// Arithmetic (DESIGN.md §5.4 with w from §5.2): w = E2M1(code) * 2^(b - 127) is exact in the model dtype, the convert applies the scale
// (mx4_word_to_frag), so the weights enter v_mfma_f32_16x16x32 as ordinary 16-bit operands: f32 sums in a fixed order, h rounded once
// from the f32 silu(g) * u, y f32.  No floating-point atomics; each path repeats bit for bit.
//
// Layout: the MX4 tile of gemv_mx4.cuh (1 KiB = 16 columns x 128 k, one 16-byte lane word = the weight operand of four
// MFMA k-steps; 64 B of scale words per tile, one u32 per column, byte j = block kt * 4 + j), stacked so that a unit is one run:
//   gate_up: tile[((e * I/16 + nb) * H/128 + kt) * 2 + t]   t = 0 gate, 1 up, interleaved tile by tile;  scale words: the same index
//   down:    tile[ (e * H/16 + nb) * I/128 + kt]                                                         scale words: the same index
//
// Decode kernel (chunk <= the switch): workgroup = (16-column unit, expert), the waves split K in whole 128-k tiles.
//   * Row tiles.  ONE 16-row tile per pass at every token count; an expert with more than 16 pairs takes further passes over its unit.
//     Under uniform routing at 32 tokens (top-8 of 128) an expert holds two pairs on average, so a second row tile is almost always
//     empty and only costs registers (160 against 115), x loads and MFMAs: measured at H 2048 / I 768, 32 tokens, 129.9 us with two row
//     tiles against 83.8 us with one.  A hot expert pays a second pass over 32 KiB it has just pulled into the L2.
//   * Wave counts.  K per wave is short: at H 2048 / I 768 gate/up has 16 tiles and down has 6.  Gate/up runs on 8 waves (two tiles of
//     each tensor per wave = one ring fill of 4 KiB in flight, the whole K share issued before the first MFMA); down runs on 4 waves
//     (1 | 2 | 1 | 2 tiles): 8 waves would leave two without a tile, and a 256-thread workgroup lets a CU hold twice as many units, which
//     is where the bytes in flight of a GEMM this short in K come from.  Several units per workgroup for down would share h rows that
//     are L2-resident anyway and halve the number of workgroups an idle-expert return frees.
//   * Ragged ends.  A rows are gathered per lane through `list`, so the x / h offsets differ per lane; a wave whose share is no multiple
//     of the ring re-reads its LAST tile (a valid one: the same cache lines it has just asked for) against a ZEROED A fragment, as
//     moe_decode_kernel does.  A wave without a tile skips the loop: no lane ever forms an address outside its tensor.
//   * Gate and up tiles of a k range go against the same gathered x fragments; one accumulator chain per tensor.
//   * The waves' partial tiles meet in LDS behind one barrier and are summed in wave order.
//
// Tiled kernel (chunk above the switch): the structure of moe_tiled_kernel — work item (expert, 64-row tile) x 64 columns, four waves,
// wave w owns column unit w — with a 128-k slab for BOTH GEMMs: a wave's weight traffic per slab is one 16-byte word and one scale word
// per tensor, loaded one slab ahead into registers and converted (four mx4_word_to_frag per tensor) in front of its 16 MFMAs.  A rows go
// through LDS in fragment order.  No 16-bit copy of the experts exists anywhere.
#pragma once
#include "gemv_mx4.cuh"
#include "moe.cuh"

struct MoeMx4Args : MoeArgs {
  const uint32_t* sc;  // the scale words beside the tiles of `w`
};

// ---------------------------------------------------------------- load-time repack: stacked checkpoint rows [E * N, K/2] (+ [E * N, K/32]) -> tiles
// One thread = one 16-byte lane word; the first 16 lanes of a tile also write its scale words.  NT = 2 interleaves two tensors tile by tile.
__global__ __launch_bounds__(256) void moe_mx4_repack_kernel(const uint8_t* __restrict__ w0, const uint8_t* __restrict__ s0, const uint8_t* __restrict__ w1,
                                                             const uint8_t* __restrict__ s1, u32x4* __restrict__ wt, uint32_t* __restrict__ st, int E, int N,
                                                             int K, int NT) {
  const int KT = K >> 7;
  const size_t total = (size_t)E * (N >> 4) * KT * NT * 64;
  const size_t o = blockIdx.x * (size_t)256 + threadIdx.x;
  if (o >= total) return;
  const int lane = (int)(o & 63);
  const size_t tile = o >> 6;
  size_t f = tile;
  const int t = (int)(f % NT);
  f /= NT;
  const int kt = (int)(f % KT);
  f /= KT;  // = e * N/16 + nb: row block of the stacked tensor
  const size_t n = f * 16 + (lane & 15);
  const uint32_t* src = reinterpret_cast<const uint32_t*>((t ? w1 : w0) + n * (K >> 1) + kt * 64 + (lane >> 4) * 4);  // (rows are K/2 bytes, a multiple of 64)
  wt[o] = u32x4{src[0], src[4], src[8], src[12]};
  if (lane < 16) st[tile * 16 + lane] = reinterpret_cast<const uint32_t*>((t ? s1 : s0) + n * (K >> 5))[kt];
}

// ---------------------------------------------------------------- decode path: workgroup = (16-column unit, expert), K split over the waves in tiles
// GU: A rows are x rows gathered by pair, gate and up tiles against the same A, h out.  !GU: A rows are the expert's h rows, y out.
// One 16-row tile per pass; an expert with more than 16 pairs is served in further passes over its (by then cached) unit.
template <class DT, int WAVES, bool GU>
__global__ __launch_bounds__(WAVES * 64) void moe_mx4_decode_kernel(const MoeMx4Args a) {
  constexpr int NT = GU ? 2 : 1;
  constexpr int PF = 2;  // tiles per tensor in flight per wave
  __shared__ f32x4 red[WAVES * NT * 64];
  const int e = (int)blockIdx.y, nb = (int)blockIdx.x;
  const int cnt = (int)a.hdr[e];
  if (cnt == 0) return;
  const int off = (int)a.hdr[MOE_HDR_OFFSETS + e];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int r16 = lane & 15, q4 = lane >> 4;
  const int K = GU ? a.H : a.I, NU = (GU ? a.I : a.H) >> 4, KT = K >> 7;
  const int kt0 = KT * wave / WAVES, kt1 = KT * (wave + 1) / WAVES;  // this wave's tiles
  const size_t unit = ((size_t)e * NU + nb) * KT * NT;               // first tile of the unit's run
  const u32x4* const wt = static_cast<const u32x4*>(a.w) + unit * 64 + lane;
  const uint32_t* const st = a.sc + unit * 16 + r16;
  for (int r0 = 0; r0 < cnt; r0 += 16) {
    const int pos = r0 + r16;
    const int sp = off + (pos < cnt ? pos : r0);  // rows past the count re-read a valid row (never stored)
    const int pair = (int)a.list[sp];
    const uint8_t* const arow = GU ? static_cast<const uint8_t*>(a.x) + ((size_t)(pair / a.topk) * K + q4 * 8) * 2
                                   : static_cast<const uint8_t*>(a.h) + ((size_t)sp * K + q4 * 8) * 2;
    f32x4 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; n++) acc[n] = vra_zero_acc();
    for (int kt = kt0; kt < kt1; kt += PF) {
      u32x4 wq[PF][NT], xq[PF][4];
      uint32_t sq[PF][NT];
#pragma unroll
      for (int i = 0; i < PF; i++) {
        const bool in = kt + i < kt1;
        const int kc = in ? kt + i : kt1 - 1;  // past the wave's last tile: that tile again, against a zeroed A fragment
#pragma unroll
        for (int n = 0; n < NT; n++) {
          wq[i][n] = __builtin_nontemporal_load(wt + ((size_t)kc * NT + n) * 64);
          sq[i][n] = st[((size_t)kc * NT + n) * 16];
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const u32x4 v = *reinterpret_cast<const u32x4*>(arow + (size_t)kc * 256 + j * 64);
          xq[i][j] = in ? v : u32x4{0u, 0u, 0u, 0u};
        }
      }
#pragma unroll
      for (int i = 0; i < PF; i++)
#pragma unroll
        for (int n = 0; n < NT; n++)
#pragma unroll
          for (int j = 0; j < 4; j++)
            DT::mfma(acc[n], mx4_word_to_frag<DT>(wq[i][n][j], mx4_scale(sq[i][n], j)), __builtin_bit_cast(s16x8, xq[i][j]));
    }
    VRA_MFMA_DRAIN();
    // the waves' partial tiles meet in LDS; wave 0 sums them in wave order
#pragma unroll
    for (int n = 0; n < NT; n++) red[(wave * NT + n) * 64 + lane] = acc[n];
    __syncthreads();
    if (wave == 0) {
      f32x4 g = {0.f, 0.f, 0.f, 0.f}, u = {0.f, 0.f, 0.f, 0.f};
      for (int w = 0; w < WAVES; w++) {
        const f32x4 pg = red[(w * NT) * 64 + lane];
#pragma unroll
        for (int c = 0; c < 4; c++) g[c] += pg[c];
        if (GU) {
          const f32x4 pu = red[(w * NT + NT - 1) * 64 + lane];
#pragma unroll
          for (int c = 0; c < 4; c++) u[c] += pu[c];
        }
      }
      const int col = nb * 16 + q4 * 4;
      if (pos < cnt) {
        if (GU) moe_store_h<DT>(g, u, static_cast<uint16_t*>(a.h) + (size_t)(off + pos) * a.I + col);
        else *reinterpret_cast<f32x4*>(a.y + (size_t)pair * a.H + col) = g;
      }
    }
    __syncthreads();  // red is reused by the next pass
  }
}

// ---------------------------------------------------------------- tiled path: workgroup = work item (expert, 64-row tile) x 64 columns, 128-k slabs
template <class DT, bool GU>
__global__ __launch_bounds__(256) void moe_mx4_tiled_kernel(const MoeMx4Args a) {
  constexpr int NT = GU ? 2 : 1;
  constexpr int SK = 4;             // k-steps of a slab = the words of a lane word
  constexpr int SEG = 16;           // 16-byte segments of a row's slab
  constexpr int RPI = 256 / SEG;    // rows the workgroup loads at once
  constexpr int NIT = MOE_BM / RPI;
  __shared__ u32x4 xs[SK * 4 * 64];
  const int wi = (int)blockIdx.y;
  if (wi >= (int)a.hdr[MOE_HDR_NWORK]) return;
  const uint32_t item = a.work[wi];
  const int e = (int)(item >> 16), r0 = (int)(item & 0xFFFFu) * MOE_BM;
  const int cnt = (int)a.hdr[e], off = (int)a.hdr[MOE_HDR_OFFSETS + e];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, q4 = lane >> 4;
  const int K = GU ? a.H : a.I, NU = (GU ? a.I : a.H) >> 4, KT = K >> 7;
  const int nb = (int)blockIdx.x * 4 + wave;
  const size_t unit = ((size_t)e * NU + nb) * KT * NT;
  const u32x4* const wt = static_cast<const u32x4*>(a.w) + unit * 64 + lane;
  const uint32_t* const st = a.sc + unit * 16 + r16;
  // loader role: rows (tid / SEG) + i * RPI, segment tid % SEG
  const int lrow = tid / SEG, lseg = tid % SEG;
  const uint8_t* src[NIT];
  int dst[NIT];
#pragma unroll
  for (int i = 0; i < NIT; i++) {
    const int row = lrow + i * RPI, pos = r0 + row;
    const int sp = off + (pos < cnt ? pos : r0);  // rows past the count re-read the tile's first row (never stored)
    const size_t arow = GU ? (size_t)(a.list[sp] / (uint32_t)a.topk) : (size_t)sp;
    src[i] = static_cast<const uint8_t*>(GU ? a.x : a.h) + (arow * K + lseg * 8) * 2;
    dst[i] = ((lseg >> 2) * 4 + (row >> 4)) * 64 + (lseg & 3) * 16 + (row & 15);
  }
  u32x4 xr[NIT], wc[NT], wn[NT];
  uint32_t sc[NT], sn[NT];
  auto load_slab = [&](u32x4 (&wd)[NT], uint32_t (&sd)[NT], int c) {
#pragma unroll
    for (int i = 0; i < NIT; i++) xr[i] = *reinterpret_cast<const u32x4*>(src[i] + (size_t)c * 256);
#pragma unroll
    for (int n = 0; n < NT; n++) {
      wd[n] = wt[((size_t)c * NT + n) * 64];
      sd[n] = st[((size_t)c * NT + n) * 16];
    }
  };
  f32x4 acc[NT][4];
#pragma unroll
  for (int n = 0; n < NT; n++)
#pragma unroll
    for (int t = 0; t < 4; t++) acc[n][t] = vra_zero_acc();
  load_slab(wc, sc, 0);
  for (int c = 0; c < KT; c++) {
    __syncthreads();  // the previous slab's fragments have been read
#pragma unroll
    for (int i = 0; i < NIT; i++) xs[dst[i]] = xr[i];
    __syncthreads();
    load_slab(wn, sn, c + 1 < KT ? c + 1 : c);  // (the last iteration re-reads its own slab: no branch around the loads)
#pragma unroll
    for (int k = 0; k < SK; k++) {
      s16x8 af[4];
#pragma unroll
      for (int t = 0; t < 4; t++) af[t] = __builtin_bit_cast(s16x8, xs[(k * 4 + t) * 64 + lane]);
#pragma unroll
      for (int n = 0; n < NT; n++) {
        const s16x8 wf = mx4_word_to_frag<DT>(wc[n][k], mx4_scale(sc[n], k));
#pragma unroll
        for (int t = 0; t < 4; t++) DT::mfma(acc[n][t], wf, af[t]);
      }
    }
#pragma unroll
    for (int n = 0; n < NT; n++) wc[n] = wn[n], sc[n] = sn[n];
  }
  VRA_MFMA_DRAIN();
  const int col = nb * 16 + q4 * 4;
#pragma unroll
  for (int t = 0; t < 4; t++) {
    const int pos = r0 + t * 16 + r16;
    if (pos < cnt) {
      if (GU) moe_store_h<DT>(acc[0][t], acc[NT - 1][t], static_cast<uint16_t*>(a.h) + (size_t)(off + pos) * a.I + col);
      else *reinterpret_cast<f32x4*>(a.y + (size_t)a.list[off + pos] * a.H + col) = acc[0][t];
    }
  }
}
