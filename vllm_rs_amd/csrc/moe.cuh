// moe.cuh — the sparse-MLP block of a mixture-of-experts decoder (reference: FusedMoe::forward, src/models/layers/moe.rs): router
// softmax + top-k, the device-side alignment of (token, slot) pairs by expert, the expert GEMMs on 16-bit weights (a decode kernel that
// streams each ACTIVE expert's weights once, a tiled grouped GEMM over a device-built work list) and the weighted sum over slots.
//
// Arithmetic: exact 16-bit products, f32 sums, h = round(silu(g) * u) from the f32 sums with ONE rounding, y stays
// f32, out = round(sum_j w[t, j] * y[t * topk + j]) in slot order with one rounding, then round(out + residual).  No floating-point
// atomics: every sum has a fixed order, so both paths repeat bit for bit.
//
// Weight layout, the same for both paths: 1 KiB fragments = 16 output columns x 32 k in MFMA lane order, lane word
// (16 bytes) = w[nb * 16 + (lane & 15)][ks * 32 + (lane >> 4) * 8 .. + 7];
//   gate_up_tiled[(((e * I/16 + nb) * H/32 + ks) * 2 + t) * 64 + lane]   t = 0 gate, 1 up: interleaved fragment by fragment
//   down_tiled   [ ((e * H/16 + nb) * I/32 + ks)          * 64 + lane]
// so the unit nb of an expert is ONE contiguous run (gate/up: H * 64 bytes, down: I * 32 bytes) that a wave walks front to back.
//
// Workspace of one chunk of <= MOE_CHUNK tokens (P = tokens * topk pairs): a 1024-word header (counts[256] | offsets[257] | number of
// work items at word 520), list[P] (pair indices grouped by expert, ascending inside an expert), work[ceil(P / 64) + E] (expert << 16 |
// row tile), h [P, I] 16-bit in expert-sorted order, y [P, H] f32 at the pair's own slot.
#pragma once
#include "common.cuh"

#define MOE_CHUNK 2048      // tokens one pass of vra_moe_experts takes (the workspace is sized for min(max_tokens, MOE_CHUNK))
#define MOE_MAX_EXPERTS 256
#define MOE_MAX_TOPK 8
#define MOE_BM 64           // rows of a work item of the tiled path
#define MOE_HDR_WORDS 1024
#define MOE_HDR_OFFSETS 256
#define MOE_HDR_NWORK 520

struct MoeArgs {
  const void* x;            // [T, H]
  const void* w;            // the tiled weights of this GEMM (gate/up or down)
  const uint32_t* hdr;      // counts | offsets | nwork
  const uint32_t* list;     // pairs by expert
  const uint32_t* work;     // (expert, row tile) items
  void* h;                  // [P, I] 16-bit, expert-sorted rows
  float* y;                 // [P, H] f32, pair order
  int P, E, topk, H, I;
};

// ---------------------------------------------------------------- routing: one wave per token
__global__ __launch_bounds__(256) void moe_route_kernel(const float* __restrict__ logits, float* __restrict__ tw, uint32_t* __restrict__ ids, int T, int E,
                                                        int topk, int norm, float scale) {
  const int lane = threadIdx.x & 63;
  const int t = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
  if (t >= T) return;
  float p[4];
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int e = lane + 64 * i;
    p[i] = e < E ? logits[(size_t)t * E + e] : -INFINITY;
    m = fmaxf(m, p[i]);
  }
  m = wave_max(m);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    p[i] = lane + 64 * i < E ? expf(p[i] - m) : 0.f;
    s += p[i];
  }
  s = wave_sum(s);
#pragma unroll
  for (int i = 0; i < 4; i++) p[i] = lane + 64 * i < E ? p[i] / s : -1.f;  // (-1: never selected, topk <= E)
  float mine_w = 0.f, sel = 0.f;
  uint32_t mine_i = 0;
  for (int j = 0; j < topk; j++) {
    float bv = p[0];
    int bi = lane;
#pragma unroll
    for (int i = 1; i < 4; i++)
      if (p[i] > bv) bv = p[i], bi = lane + 64 * i;  // strict: the lower index keeps a tie
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ov > bv || (ov == bv && oi < bi)) bv = ov, bi = oi;
    }
#pragma unroll
    for (int i = 0; i < 4; i++)
      if (bi == lane + 64 * i) p[i] = -1.f;
    if (lane == j) mine_w = bv, mine_i = (uint32_t)bi;
    sel += bv;  // slot order
  }
  if (lane < topk) {
    if (norm) mine_w /= sel;
    tw[(size_t)t * topk + lane] = mine_w * scale;
    ids[(size_t)t * topk + lane] = mine_i;
  }
}

// ---------------------------------------------------------------- alignment: one workgroup, a stable counting sort by expert
// Thread (s, e) = (tid >> 8, tid & 255) walks quarter s of the ids (staged in LDS as 16-bit, ids >= E as 0xFFFF) for expert e: once to
// count, once — after wave 0 has scanned counts and row-tile counts — to write the pair indices.  Everything is decided by position,
// nothing by arrival order: the result is deterministic.
__global__ __launch_bounds__(1024) void moe_align_kernel(const uint32_t* __restrict__ ids, int P, int E, uint32_t* __restrict__ hdr,
                                                         uint32_t* __restrict__ list, uint32_t* __restrict__ work) {
  __shared__ __attribute__((aligned(16))) uint16_t id16[MOE_CHUNK * MOE_MAX_TOPK + 64];
  __shared__ uint32_t cnt[4][MOE_MAX_EXPERTS], offs[MOE_MAX_EXPERTS];
  const int tid = threadIdx.x, e = tid & 255, s = tid >> 8;
  const int segl = ((P + 3) / 4 + 7) & ~7;  // a quarter, in whole 8-id words
  for (int i = tid; i < 4 * segl; i += 1024) {
    uint32_t v = 0xFFFFu;
    if (i < P) {
      v = ids[i];
      if (v >= (uint32_t)E) v = 0xFFFFu;
    }
    id16[i] = (uint16_t)v;
  }
  __syncthreads();
  const u32x4* seg = reinterpret_cast<const u32x4*>(id16 + s * segl);
  const uint32_t lo = (uint32_t)e, hi = (uint32_t)e << 16;
  uint32_t c = 0;
  if (e < E)
    for (int i = 0; i < (segl >> 3); i++) {
      const u32x4 v = seg[i];
#pragma unroll
      for (int k = 0; k < 4; k++) c += ((v[k] & 0xFFFFu) == lo) + ((v[k] & 0xFFFF0000u) == hi);
    }
  cnt[s][e] = c;
  __syncthreads();
  if (tid < 64) {  // wave 0: lane l owns experts 4l .. 4l + 3; exclusive scans of pair counts and row-tile counts
    uint32_t tot[4], nt[4], a = 0, b = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      tot[i] = cnt[0][tid * 4 + i] + cnt[1][tid * 4 + i] + cnt[2][tid * 4 + i] + cnt[3][tid * 4 + i];
      nt[i] = (tot[i] + MOE_BM - 1) / MOE_BM;
      a += tot[i], b += nt[i];
    }
    uint32_t ia = a, ib = b;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t ua = __shfl_up(ia, o, 64), ub = __shfl_up(ib, o, 64);
      if (tid >= o) ia += ua, ib += ub;
    }
    uint32_t xa = ia - a, xb = ib - b;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int ee = tid * 4 + i;
      offs[ee] = xa;
      if (ee < E) {
        hdr[ee] = tot[i];
        hdr[MOE_HDR_OFFSETS + ee] = xa;
        for (uint32_t r = 0; r < nt[i]; r++) work[xb + r] = ((uint32_t)ee << 16) | r;
      }
      xa += tot[i], xb += nt[i];
    }
    if (tid == 63) hdr[MOE_HDR_OFFSETS + E] = ia, hdr[MOE_HDR_NWORK] = ib;
  }
  __syncthreads();
  if (e >= E) return;
  uint32_t o = offs[e];
  for (int q = 0; q < s; q++) o += cnt[q][e];
  const int p0 = s * segl;
  for (int i = 0; i < (segl >> 3); i++) {
    const u32x4 v = seg[i];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      if ((v[k] & 0xFFFFu) == lo) list[o++] = (uint32_t)(p0 + i * 8 + 2 * k);
      if ((v[k] & 0xFFFF0000u) == hi) list[o++] = (uint32_t)(p0 + i * 8 + 2 * k + 1);
    }
  }
}

// ---------------------------------------------------------------- epilogues (lane (r16, q4) of an accumulator holds row r16, columns q4 * 4 .. + 3)
template <class DT>
__device__ __forceinline__ void moe_store_h(const f32x4& g, const f32x4& u, uint16_t* out) {
  float v[4];
#pragma unroll
  for (int e = 0; e < 4; e++) v[e] = (g[e] / (1.0f + expf(-g[e]))) * u[e];
  *reinterpret_cast<u32x2*>(out) = u32x2{DT::pack2(v[0], v[1]), DT::pack2(v[2], v[3])};
}

// ---------------------------------------------------------------- decode path: workgroup = (16-column unit, expert), K split over the waves
// GU: A rows are x rows gathered by pair, two tensors (gate, up) against the same A, h out.  !GU: A rows are the expert's h rows, y out.
// A workgroup of an idle expert returns at once.  An expert with more than 16 * MT pairs (possible only when a token names an expert
// twice, or above the decode switch) is served in several passes over its weights.
template <class DT, int MT, int WAVES, bool GU>
__global__ __launch_bounds__(WAVES * 64) void moe_decode_kernel(const MoeArgs a) {
  constexpr int NT = GU ? 2 : 1;
  constexpr int PF = 4;  // k-steps in flight per wave
  __shared__ f32x4 red[WAVES * NT * MT * 64];
  const int e = (int)blockIdx.y, nb = (int)blockIdx.x;
  const int cnt = (int)a.hdr[e];
  if (cnt == 0) return;
  const int off = (int)a.hdr[MOE_HDR_OFFSETS + e];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int r16 = lane & 15, q4 = lane >> 4;
  const int K = GU ? a.H : a.I, NU = (GU ? a.I : a.H) >> 4, KS = K >> 5;
  const int k0 = KS * wave / WAVES, k1 = KS * (wave + 1) / WAVES;  // this wave's k-steps
  const u32x4* const wt = static_cast<const u32x4*>(a.w) + ((size_t)e * NU + nb) * KS * NT * 64 + lane;
  for (int r0 = 0; r0 < cnt; r0 += 16 * MT) {
    const uint8_t* arow[MT];
    int pair[MT];
#pragma unroll
    for (int t = 0; t < MT; t++) {
      const int pos = r0 + t * 16 + r16;
      const int sp = off + (pos < cnt ? pos : r0);  // rows past the count re-read a valid row (never stored)
      pair[t] = (int)a.list[sp];
      arow[t] = GU ? static_cast<const uint8_t*>(a.x) + ((size_t)(pair[t] / a.topk) * K + q4 * 8) * 2
                   : static_cast<const uint8_t*>(a.h) + ((size_t)sp * K + q4 * 8) * 2;
    }
    f32x4 acc[NT][MT];
#pragma unroll
    for (int n = 0; n < NT; n++)
#pragma unroll
      for (int t = 0; t < MT; t++) acc[n][t] = vra_zero_acc();
    for (int ks = k0; ks < k1; ks += PF) {
      u32x4 wq[PF][NT], xq[PF][MT];
#pragma unroll
      for (int i = 0; i < PF; i++) {
        const bool in = ks + i < k1;
        const int kc = in ? ks + i : k1 - 1;  // past the wave's last step: a valid step again, against a zeroed A fragment
#pragma unroll
        for (int n = 0; n < NT; n++) wq[i][n] = __builtin_nontemporal_load(wt + ((size_t)kc * NT + n) * 64);
#pragma unroll
        for (int t = 0; t < MT; t++) {
          const u32x4 v = *reinterpret_cast<const u32x4*>(arow[t] + (size_t)kc * 64);
          xq[i][t] = in ? v : u32x4{0u, 0u, 0u, 0u};
        }
      }
#pragma unroll
      for (int i = 0; i < PF; i++)
#pragma unroll
        for (int n = 0; n < NT; n++)
#pragma unroll
          for (int t = 0; t < MT; t++) DT::mfma(acc[n][t], __builtin_bit_cast(s16x8, wq[i][n]), __builtin_bit_cast(s16x8, xq[i][t]));
    }
    VRA_MFMA_DRAIN();
    // the waves' partial tiles meet in LDS; wave t sums row tile t in wave order
#pragma unroll
    for (int n = 0; n < NT; n++)
#pragma unroll
      for (int t = 0; t < MT; t++) red[((wave * NT + n) * MT + t) * 64 + lane] = acc[n][t];
    __syncthreads();
    if (wave < MT) {
      f32x4 g = {0.f, 0.f, 0.f, 0.f}, u = {0.f, 0.f, 0.f, 0.f};
      for (int w = 0; w < WAVES; w++) {
        const f32x4 pg = red[((w * NT) * MT + wave) * 64 + lane];
#pragma unroll
        for (int c = 0; c < 4; c++) g[c] += pg[c];
        if (GU) {
          const f32x4 pu = red[((w * NT + NT - 1) * MT + wave) * 64 + lane];
#pragma unroll
          for (int c = 0; c < 4; c++) u[c] += pu[c];
        }
      }
      const int pos = r0 + wave * 16 + r16, col = nb * 16 + q4 * 4;
      if (pos < cnt) {
        if (GU) {
          moe_store_h<DT>(g, u, static_cast<uint16_t*>(a.h) + (size_t)(off + pos) * a.I + col);
        } else {
          int pr = pair[0];
#pragma unroll
          for (int t = 1; t < MT; t++) pr = wave == t ? pair[t] : pr;
          *reinterpret_cast<f32x4*>(a.y + (size_t)pr * a.H + col) = g;
        }
      }
    }
    __syncthreads();  // red is reused by the next pass
  }
}

// ---------------------------------------------------------------- tiled path: workgroup = work item (expert, 64-row tile) x 64 columns
// Four waves; wave w owns the 16-column unit w of the tile (GU: its gate AND its up fragments, so SiLU * mul stays in the epilogue) against
// all four 16-row fragments.  The A rows (GU: x rows gathered by pair; else the expert's contiguous h rows) go through LDS in fragment
// order, one KC-wide slab at a time with the next slab's global loads in flight; the weight fragments of a wave are its own (no other
// wave reads them), so they go from global memory straight into operand registers, one slab ahead.
template <class DT, bool GU>
__global__ __launch_bounds__(256) void moe_tiled_kernel(const MoeArgs a) {
  constexpr int NT = GU ? 2 : 1;
  constexpr int KC = GU ? 128 : 64;  // H % 128 == 0, I % 64 == 0
  constexpr int SK = KC / 32;        // k-steps of a slab
  constexpr int SEG = KC / 8;        // 16-byte segments of a row's slab
  constexpr int RPI = 256 / SEG;     // rows the workgroup loads at once
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
  const int K = GU ? a.H : a.I, NU = (GU ? a.I : a.H) >> 4, KS = K >> 5, NC = K / KC;
  const int nb = (int)blockIdx.x * 4 + wave;
  const u32x4* const wt = static_cast<const u32x4*>(a.w) + ((size_t)e * NU + nb) * KS * NT * 64 + lane;
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
  u32x4 xr[NIT], wc[SK][NT], wn[SK][NT];
  auto load_slab = [&](u32x4 (&wd)[SK][NT], int c) {
#pragma unroll
    for (int i = 0; i < NIT; i++) xr[i] = *reinterpret_cast<const u32x4*>(src[i] + (size_t)c * KC * 2);
#pragma unroll
    for (int k = 0; k < SK; k++)
#pragma unroll
      for (int n = 0; n < NT; n++) wd[k][n] = wt[((size_t)(c * SK + k) * NT + n) * 64];
  };
  f32x4 acc[NT][4];
#pragma unroll
  for (int n = 0; n < NT; n++)
#pragma unroll
    for (int t = 0; t < 4; t++) acc[n][t] = vra_zero_acc();
  load_slab(wc, 0);
  for (int c = 0; c < NC; c++) {
    __syncthreads();  // the previous slab's fragments have been read
#pragma unroll
    for (int i = 0; i < NIT; i++) xs[dst[i]] = xr[i];
    __syncthreads();
    load_slab(wn, c + 1 < NC ? c + 1 : c);  // (the last iteration re-reads its own slab: no branch around the loads)
#pragma unroll
    for (int k = 0; k < SK; k++) {
      s16x8 af[4];
#pragma unroll
      for (int t = 0; t < 4; t++) af[t] = __builtin_bit_cast(s16x8, xs[(k * 4 + t) * 64 + lane]);
#pragma unroll
      for (int n = 0; n < NT; n++)
#pragma unroll
        for (int t = 0; t < 4; t++) DT::mfma(acc[n][t], __builtin_bit_cast(s16x8, wc[k][n]), af[t]);
    }
#pragma unroll
    for (int k = 0; k < SK; k++)
#pragma unroll
      for (int n = 0; n < NT; n++) wc[k][n] = wn[k][n];
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

// ---------------------------------------------------------------- combine: out[t] = round(sum_j w[t, j] * y[t * topk + j]) (+ residual)
template <class DT>
__global__ __launch_bounds__(256) void moe_combine_kernel(const float* __restrict__ y, const float* __restrict__ tw, const uint32_t* __restrict__ ids,
                                                          const uint16_t* __restrict__ res, uint16_t* __restrict__ out, int T, int E, int topk, int H) {
  const size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
  const int H8 = H >> 3;
  if (i >= (size_t)T * H8) return;
  const size_t t = i / H8;
  const int c = (int)(i % H8) * 8;
  float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < topk; j++) {
    if (ids[t * topk + j] >= (uint32_t)E) continue;  // a dropped pair: its y row was never written
    const float w = tw[t * topk + j];
    const f32x4* p = reinterpret_cast<const f32x4*>(y + (t * topk + j) * H + c);
    const f32x4 lo = p[0], hi = p[1];
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] += w * lo[k], v[4 + k] += w * hi[k];
  }
  if (res) {
    float r[8];
    unpack8<DT>(*reinterpret_cast<const u32x4*>(res + t * H + c), r);
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = rnd_dt<DT>(v[k]) + r[k];
  }
  *reinterpret_cast<u32x4*>(out + t * H + c) = pack8<DT>(v);
}

// ---------------------------------------------------------------- load-time repack: [E][N][K] rows -> fragments; one thread = one lane word
__global__ __launch_bounds__(256) void moe_repack_kernel(const uint16_t* __restrict__ s0, const uint16_t* __restrict__ s1, u32x4* __restrict__ dst, int E, int N,
                                                         int K, int NT) {
  const int KS = K >> 5, NU = N >> 4;
  const size_t total = (size_t)E * NU * KS * NT * 64;
  const size_t o = blockIdx.x * (size_t)256 + threadIdx.x;
  if (o >= total) return;
  const int lane = (int)(o & 63);
  size_t f = o >> 6;
  const int t = (int)(f % NT);
  f /= NT;
  const int ks = (int)(f % KS);
  f /= KS;  // = e * NU + nb: row block of the stacked [E * N, K] tensor
  const uint16_t* src = (t ? s1 : s0) + (f * 16 + (lane & 15)) * K + ks * 32 + (lane >> 4) * 8;
  dst[o] = *reinterpret_cast<const u32x4*>(src);
}
