// moe_gemm.hip — launchers and C entry points of the mixture-of-experts block (kernels: moe.cuh; reference: FusedMoe::forward,
// src/models/layers/moe.rs): vra_moe_route, vra_moe_repack, vra_moe_workspace_bytes, vra_moe_experts.  No synchronisation, no
// allocation, no host read-back: the per-expert counts exist on the device only, so every grid is sized by its upper bound and a
// workgroup without work returns at once.  Everything is capturable on the given stream.  The same block on MXFP4 experts (kernels:
// moe_mx4.cuh; reference: FusedMoeMxfp4): vra_moe_mxfp4_repack, vra_moe_mxfp4_experts, on the same routing and the same workspace.
#include "moe_mx4.cuh"

// Tokens (of one chunk) up to which the decode kernels serve the expert GEMMs; above, the tiled grouped GEMM.
static int g_moe_decode_rows = 32;
// measurement aid (tools/moe_bench.py): 0..32, the decode kernel holds two 16-row tiles per pass
extern "C" void vra_debug_set_moe_decode_max_rows(int32_t rows) { g_moe_decode_rows = rows < 0 ? 0 : (rows > 32 ? 32 : rows); }

static inline size_t moe_up(size_t v) { return (v + 255) & ~(size_t)255; }
struct MoeWorkspace {
  size_t list, work, h, y, total;
};
static MoeWorkspace moe_workspace(int64_t tokens, int experts, int topk, int hidden, int inter) {
  const size_t chunk = (size_t)(tokens < MOE_CHUNK ? tokens : MOE_CHUNK), p = chunk * topk;
  MoeWorkspace w;
  w.list = moe_up(MOE_HDR_WORDS * 4);
  w.work = w.list + moe_up(p * 4);
  w.h = w.work + moe_up(((p + MOE_BM - 1) / MOE_BM + experts) * 4);
  w.y = w.h + moe_up(p * inter * 2);
  w.total = w.y + moe_up(p * hidden * 4);
  return w;
}

#define VRA_MOE_CHECK_SHAPE(name, experts, topk, hidden, inter)                                                                             \
  VRA_CHECK_ARG((experts) >= 1 && (experts) <= MOE_MAX_EXPERTS && (topk) >= 1 && (topk) <= MOE_MAX_TOPK && (topk) <= (experts),              \
                name ": bad routing shape E=%d topk=%d (E <= 256, topk <= 8, topk <= E)", (int)(experts), (int)(topk));                     \
  VRA_CHECK_ARG((hidden) >= 128 && (hidden) % 128 == 0 && (inter) >= 64 && (inter) % 64 == 0, name ": bad shape H=%d I=%d (H %% 128, I %% 64)", \
                (int)(hidden), (int)(inter))

extern "C" void vra_moe_route(const float* router_logits, float* topk_weights, uint32_t* topk_ids, int32_t tokens, int32_t experts, int32_t topk,
                              int32_t norm_topk_prob, float routed_scale, int64_t stream) {
  VRA_CHECK_ARG(router_logits && topk_weights && topk_ids, "moe_route: null pointer");
  VRA_CHECK_ARG(tokens >= 1, "moe_route: bad token count %d", (int)tokens);
  VRA_CHECK_ARG(experts >= 1 && experts <= MOE_MAX_EXPERTS && topk >= 1 && topk <= MOE_MAX_TOPK && topk <= experts,
                "moe_route: bad routing shape E=%d topk=%d (E <= 256, topk <= 8, topk <= E)", (int)experts, (int)topk);
  moe_route_kernel<<<dim3((unsigned)((tokens + 3) / 4)), 256, 0, as_stream(stream)>>>(router_logits, topk_weights, topk_ids, tokens, experts, topk,
                                                                                    norm_topk_prob, routed_scale);
}

extern "C" void vra_moe_repack(const void* w_gate, const void* w_up, const void* w_down, void* gate_up_tiled, void* down_tiled, int32_t experts,
                               int32_t hidden, int32_t inter, int32_t dtype, int64_t stream) {
  VRA_CHECK_ARG(w_gate && w_up && w_down && gate_up_tiled && down_tiled, "moe_repack: null pointer");
  VRA_MOE_CHECK_SHAPE("moe_repack", experts, 1, hidden, inter);
  VRA_CHECK_ARG(dtype == VRA_BF16 || dtype == VRA_F16, "moe_repack: dtype must be bf16/f16");
  const size_t words = (size_t)experts * hidden * inter / 8;  // 16-byte lane words of one tensor
  moe_repack_kernel<<<dim3((unsigned)((2 * words + 255) / 256)), 256, 0, as_stream(stream)>>>(
      static_cast<const uint16_t*>(w_gate), static_cast<const uint16_t*>(w_up), static_cast<u32x4*>(gate_up_tiled), experts, inter, hidden, 2);
  moe_repack_kernel<<<dim3((unsigned)((words + 255) / 256)), 256, 0, as_stream(stream)>>>(
      static_cast<const uint16_t*>(w_down), nullptr, static_cast<u32x4*>(down_tiled), experts, hidden, inter, 1);
}

extern "C" int64_t vra_moe_workspace_bytes(int32_t max_tokens, int32_t experts, int32_t topk, int32_t hidden, int32_t inter) {
  if (max_tokens < 1 || experts < 1 || experts > MOE_MAX_EXPERTS || topk < 1 || topk > MOE_MAX_TOPK || topk > experts || hidden < 128 ||
      hidden % 128 || inter < 64 || inter % 64) {
    vra_set_error("moe_workspace_bytes: bad shape tokens=%d E=%d topk=%d H=%d I=%d", (int)max_tokens, (int)experts, (int)topk, (int)hidden, (int)inter);
    return 0;
  }
  return (int64_t)moe_workspace(max_tokens, experts, topk, hidden, inter).total;
}

template <class DT>
static void moe_run_chunk(MoeArgs a, const void* wgu, const void* wdn, const float* tw, const uint32_t* ids, const void* residual, void* out, int tokens,
                          uint32_t* hdr, uint32_t* list, uint32_t* work, hipStream_t st) {
  moe_align_kernel<<<1, 1024, 0, st>>>(ids, a.P, a.E, hdr, list, work);
  const unsigned ui = (unsigned)(a.I >> 4), uh = (unsigned)(a.H >> 4);
  if (tokens <= g_moe_decode_rows) {
    a.w = wgu;
    if (tokens <= 16) moe_decode_kernel<DT, 1, 8, true><<<dim3(ui, (unsigned)a.E), 512, 0, st>>>(a);
    else moe_decode_kernel<DT, 2, 8, true><<<dim3(ui, (unsigned)a.E), 512, 0, st>>>(a);
    a.w = wdn;
    if (tokens <= 16) moe_decode_kernel<DT, 1, 8, false><<<dim3(uh, (unsigned)a.E), 512, 0, st>>>(a);
    else moe_decode_kernel<DT, 2, 8, false><<<dim3(uh, (unsigned)a.E), 512, 0, st>>>(a);
  } else {
    const unsigned items = (unsigned)((a.P + MOE_BM - 1) / MOE_BM + a.E);  // upper bound of the device-built work list
    a.w = wgu;
    moe_tiled_kernel<DT, true><<<dim3(ui / 4, items), 256, 0, st>>>(a);
    a.w = wdn;
    moe_tiled_kernel<DT, false><<<dim3(uh / 4, items), 256, 0, st>>>(a);
  }
  const size_t n = (size_t)tokens * (a.H >> 3);
  moe_combine_kernel<DT><<<dim3((unsigned)((n + 255) / 256)), 256, 0, st>>>(a.y, tw, ids, static_cast<const uint16_t*>(residual), static_cast<uint16_t*>(out),
                                                                          tokens, a.E, a.topk, a.H);
}

extern "C" void vra_moe_experts(const void* x, const void* gate_up_tiled, const void* down_tiled, const float* topk_weights, const uint32_t* topk_ids,
                                const void* residual, void* out, void* workspace, int32_t tokens, int32_t experts, int32_t topk, int32_t hidden,
                                int32_t inter, int32_t dtype, int64_t stream) {
  VRA_CHECK_ARG(x && gate_up_tiled && down_tiled && topk_weights && topk_ids && out, "moe_experts: null pointer");
  VRA_CHECK_ARG(workspace, "moe_experts: null workspace (vra_moe_workspace_bytes gives its size)");
  VRA_CHECK_ARG(tokens >= 1, "moe_experts: bad token count %d", (int)tokens);
  VRA_MOE_CHECK_SHAPE("moe_experts", experts, topk, hidden, inter);
  VRA_CHECK_ARG(dtype == VRA_BF16 || dtype == VRA_F16, "moe_experts: dtype must be bf16/f16");
  const MoeWorkspace ws = moe_workspace(tokens, experts, topk, hidden, inter);
  uint8_t* const base = static_cast<uint8_t*>(workspace);
  for (int t0 = 0; t0 < tokens; t0 += MOE_CHUNK) {  // stream order keeps the chunks apart: they share the workspace
    const int tc = tokens - t0 < MOE_CHUNK ? tokens - t0 : MOE_CHUNK;
    MoeArgs a{};
    a.x = static_cast<const uint8_t*>(x) + (size_t)t0 * hidden * 2;
    a.hdr = reinterpret_cast<uint32_t*>(base), a.list = reinterpret_cast<uint32_t*>(base + ws.list), a.work = reinterpret_cast<uint32_t*>(base + ws.work);
    a.h = base + ws.h, a.y = reinterpret_cast<float*>(base + ws.y);
    a.P = tc * topk, a.E = experts, a.topk = topk, a.H = hidden, a.I = inter;
    const void* res = residual ? static_cast<const uint8_t*>(residual) + (size_t)t0 * hidden * 2 : nullptr;
    void* o = static_cast<uint8_t*>(out) + (size_t)t0 * hidden * 2;
    const float* tw = topk_weights + (size_t)t0 * topk;
    const uint32_t* ids = topk_ids + (size_t)t0 * topk;
    uint32_t* hdr = reinterpret_cast<uint32_t*>(base);
    if (dtype == VRA_BF16)
      moe_run_chunk<BF16>(a, gate_up_tiled, down_tiled, tw, ids, res, o, tc, hdr, const_cast<uint32_t*>(a.list), const_cast<uint32_t*>(a.work), as_stream(stream));
    else
      moe_run_chunk<F16>(a, gate_up_tiled, down_tiled, tw, ids, res, o, tc, hdr, const_cast<uint32_t*>(a.list), const_cast<uint32_t*>(a.work), as_stream(stream));
  }
}

// ---------------------------------------------------------------- MXFP4 experts (moe_mx4.cuh)
// Tokens (of one chunk) up to which the MXFP4 decode kernels serve the expert GEMMs; above, the tiled MXFP4 grouped GEMM.
static int g_moe_mx4_decode_rows = 32;
// measurement aid (tools/moe_bench.py): 0..32, as for the 16-bit block
extern "C" void vra_debug_set_moe_mxfp4_decode_max_rows(int32_t rows) { g_moe_mx4_decode_rows = rows < 0 ? 0 : (rows > 32 ? 32 : rows); }

#define VRA_MOE_MX4_CHECK_INTER(name, inter) \
  VRA_CHECK_ARG((inter) % 128 == 0, name ": bad shape I=%d (I %% 128: the down GEMM walks K in 128-wide MXFP4 tiles)", (int)(inter))

extern "C" void vra_moe_mxfp4_repack(const void* gate_packed, const void* gate_scale, const void* up_packed, const void* up_scale, const void* down_packed,
                                     const void* down_scale, void* gate_up_tiled, void* gate_up_scales, void* down_tiled, void* down_scales,
                                     int32_t experts, int32_t hidden, int32_t inter, int64_t stream) {
  VRA_CHECK_ARG(gate_packed && gate_scale && up_packed && up_scale && down_packed && down_scale && gate_up_tiled && gate_up_scales && down_tiled &&
                    down_scales,
                "moe_mxfp4_repack: null pointer");
  VRA_MOE_CHECK_SHAPE("moe_mxfp4_repack", experts, 1, hidden, inter);
  VRA_MOE_MX4_CHECK_INTER("moe_mxfp4_repack", inter);
  const size_t words = (size_t)experts * hidden * inter / 32;  // 16-byte lane words of one tensor
  moe_mx4_repack_kernel<<<dim3((unsigned)((2 * words + 255) / 256)), 256, 0, as_stream(stream)>>>(
      static_cast<const uint8_t*>(gate_packed), static_cast<const uint8_t*>(gate_scale), static_cast<const uint8_t*>(up_packed),
      static_cast<const uint8_t*>(up_scale), static_cast<u32x4*>(gate_up_tiled), static_cast<uint32_t*>(gate_up_scales), experts, inter, hidden, 2);
  moe_mx4_repack_kernel<<<dim3((unsigned)((words + 255) / 256)), 256, 0, as_stream(stream)>>>(
      static_cast<const uint8_t*>(down_packed), static_cast<const uint8_t*>(down_scale), nullptr, nullptr, static_cast<u32x4*>(down_tiled),
      static_cast<uint32_t*>(down_scales), experts, hidden, inter, 1);
}

struct MoeMx4Weights {
  const void *wgu, *wdn;
  const uint32_t *sgu, *sdn;
};

template <class DT>
static void moe_mx4_run_chunk(MoeMx4Args a, const MoeMx4Weights& w, const float* tw, const uint32_t* ids, const void* residual, void* out, int tokens,
                              uint32_t* hdr, uint32_t* list, uint32_t* work, hipStream_t st) {
  moe_align_kernel<<<1, 1024, 0, st>>>(ids, a.P, a.E, hdr, list, work);
  const unsigned ui = (unsigned)(a.I >> 4), uh = (unsigned)(a.H >> 4);
  if (tokens <= g_moe_mx4_decode_rows) {  // gate/up on 8 waves, down on 4, one row tile per pass: moe_mx4.cuh says why
    a.w = w.wgu, a.sc = w.sgu;
    moe_mx4_decode_kernel<DT, 8, true><<<dim3(ui, (unsigned)a.E), 512, 0, st>>>(a);
    a.w = w.wdn, a.sc = w.sdn;
    moe_mx4_decode_kernel<DT, 4, false><<<dim3(uh, (unsigned)a.E), 256, 0, st>>>(a);
  } else {
    const unsigned items = (unsigned)((a.P + MOE_BM - 1) / MOE_BM + a.E);  // upper bound of the device-built work list
    a.w = w.wgu, a.sc = w.sgu;
    moe_mx4_tiled_kernel<DT, true><<<dim3(ui / 4, items), 256, 0, st>>>(a);
    a.w = w.wdn, a.sc = w.sdn;
    moe_mx4_tiled_kernel<DT, false><<<dim3(uh / 4, items), 256, 0, st>>>(a);
  }
  const size_t n = (size_t)tokens * (a.H >> 3);
  moe_combine_kernel<DT><<<dim3((unsigned)((n + 255) / 256)), 256, 0, st>>>(a.y, tw, ids, static_cast<const uint16_t*>(residual), static_cast<uint16_t*>(out),
                                                                          tokens, a.E, a.topk, a.H);
}

extern "C" void vra_moe_mxfp4_experts(const void* x, const void* gate_up_tiled, const void* gate_up_scales, const void* down_tiled, const void* down_scales,
                                      const float* topk_weights, const uint32_t* topk_ids, const void* residual, void* out, void* workspace,
                                      int32_t tokens, int32_t experts, int32_t topk, int32_t hidden, int32_t inter, int32_t dtype, int64_t stream) {
  VRA_CHECK_ARG(x && gate_up_tiled && down_tiled && topk_weights && topk_ids && out, "moe_mxfp4_experts: null pointer");
  VRA_CHECK_ARG(gate_up_scales && down_scales, "moe_mxfp4_experts: null scale pointer");
  VRA_CHECK_ARG(workspace, "moe_mxfp4_experts: null workspace (vra_moe_workspace_bytes gives its size)");
  VRA_CHECK_ARG(tokens >= 1, "moe_mxfp4_experts: bad token count %d", (int)tokens);
  VRA_MOE_CHECK_SHAPE("moe_mxfp4_experts", experts, topk, hidden, inter);
  VRA_MOE_MX4_CHECK_INTER("moe_mxfp4_experts", inter);
  VRA_CHECK_ARG(dtype == VRA_BF16 || dtype == VRA_F16, "moe_mxfp4_experts: dtype must be bf16/f16");
  const MoeWorkspace ws = moe_workspace(tokens, experts, topk, hidden, inter);
  uint8_t* const base = static_cast<uint8_t*>(workspace);
  const MoeMx4Weights w{gate_up_tiled, down_tiled, static_cast<const uint32_t*>(gate_up_scales), static_cast<const uint32_t*>(down_scales)};
  uint32_t *const hdr = reinterpret_cast<uint32_t*>(base), *const list = reinterpret_cast<uint32_t*>(base + ws.list),
                  *const work = reinterpret_cast<uint32_t*>(base + ws.work);
  for (int t0 = 0; t0 < tokens; t0 += MOE_CHUNK) {  // stream order keeps the chunks apart: they share the workspace
    const int tc = tokens - t0 < MOE_CHUNK ? tokens - t0 : MOE_CHUNK;
    MoeMx4Args a{};
    a.x = static_cast<const uint8_t*>(x) + (size_t)t0 * hidden * 2;
    a.hdr = hdr, a.list = list, a.work = work;
    a.h = base + ws.h, a.y = reinterpret_cast<float*>(base + ws.y);
    a.P = tc * topk, a.E = experts, a.topk = topk, a.H = hidden, a.I = inter;
    const void* res = residual ? static_cast<const uint8_t*>(residual) + (size_t)t0 * hidden * 2 : nullptr;
    void* o = static_cast<uint8_t*>(out) + (size_t)t0 * hidden * 2;
    const float* tw = topk_weights + (size_t)t0 * topk;
    const uint32_t* ids = topk_ids + (size_t)t0 * topk;
    if (dtype == VRA_BF16) moe_mx4_run_chunk<BF16>(a, w, tw, ids, res, o, tc, hdr, list, work, as_stream(stream));
    else moe_mx4_run_chunk<F16>(a, w, tw, ids, res, o, tc, hdr, list, work, as_stream(stream));
  }
}
