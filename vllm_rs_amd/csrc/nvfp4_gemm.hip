// nvfp4_gemm.hip — launchers and C entry points of the NVFP4 linears (reference: LnNvfp4, src/models/layers/linear.rs:1146-1306):
// vra_nvfp4_repack (checkpoint rows -> tile layout), vra_nvfp4_gemm and vra_nvfp4_gate_up_silu, which run the decode kernel
// (gemv_nv4.cuh) up to 32 rows and, above, the widening pass into vra_dense_scratch followed by kernel X (gemm_dense.cuh) with the
// global scale on its finished sums, and vra_nvfp4_dequant_frag (that pass alone).  No synchronisation; the scratch is the only
// allocation and never grows inside a capture.
#include "gemv_nv4.cuh"

#include <cmath>

#include "gemm_dense_launch.h"

static int nv4_num_cus() {
  static int n[64] = {0};
  int dev = 0;
  (void)hipGetDevice(&dev);
  dev &= 63;
  if (!n[dev] && (hipDeviceGetAttribute(&n[dev], hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n[dev] <= 0)) n[dev] = 256;
  return n[dev];
}

// Rows up to which the decode kernel serves a GEMM (it pads to 16 or 32 rows); above, pass + kernel X.
static int g_nv4_decode_rows = 32;
// measurement aid (tools/mxfp4_gemm_bench.py): 0..32, the kernel pads to at most 32 rows
extern "C" void vra_debug_set_nvfp4_decode_max_rows(int32_t rows) { g_nv4_decode_rows = rows < 0 ? 0 : (rows > 32 ? 32 : rows); }

// synthetic weights (host/model.cpp qlinear_synth): iid codes in the tile layout directly, every scale byte one of 0x38 | 0x3A | 0x3C |
// 0x3E (1, 1.25, 1.5, 1.75: mean square 1.97 against the codes' 8.56, so w has rms 4.1 and the caller's g = 0.02 / 4.1 gives std ~ 0.02)
__global__ __launch_bounds__(256) void nv4_fill_kernel(uint32_t* __restrict__ w, size_t w_words, uint32_t* __restrict__ s, size_t s_words, uint64_t seed) {
  const size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
  if (i < w_words) w[i] = vra_hash32(seed, i);
  if (i < s_words) s[i] = 0x38383838u + (vra_hash32(seed + 1, i) & 0x06060606u);
}
float vra_launch_nvfp4_fill(void* w_tiled, void* s_tiled, int n, int k, uint64_t seed, int64_t stream) {
  const size_t ww = (size_t)n * k / 8, sw = (size_t)n * k / 64;
  nv4_fill_kernel<<<dim3((unsigned)((ww + 255) / 256)), 256, 0, as_stream(stream)>>>(static_cast<uint32_t*>(w_tiled), ww, static_cast<uint32_t*>(s_tiled), sw, seed);
  return 0.02f / 4.106f;  // the global scale that goes with this fill
}

template <class DT, int MT, bool DUAL>
static void launch_gemv_nv4_w(const GemvNv4Args& a, int waves, hipStream_t st) {
  const dim3 grid((unsigned)(a.N >> 4));
  if (waves == 4) gemv_nv4_kernel<DT, MT, 4, DUAL><<<grid, 256, 0, st>>>(a);
  else if (waves == 8) gemv_nv4_kernel<DT, MT, 8, DUAL><<<grid, 512, 0, st>>>(a);
  else if constexpr (MT == 1 && !DUAL) gemv_nv4_kernel<DT, MT, 16, DUAL><<<grid, 1024, 0, st>>>(a);
  else vra_set_error("nvfp4 decode kernel: two row tiles, or two tensors, run on at most 8 waves");
}
template <class DT, bool DUAL>
static void launch_gemv_nv4(const GemvNv4Args& a, hipStream_t st) {
  // waves of a workgroup: each CU should hold ~16 streaming waves whatever the number of 16-column units
  const int units = a.N >> 4, cus = nv4_num_cus();
  const int waves = units >= 2 * cus ? 4 : (units >= cus ? 8 : 16);
  if (a.M <= 16) launch_gemv_nv4_w<DT, 1, DUAL>(a, DUAL && waves > 8 ? 8 : waves, st);
  else launch_gemv_nv4_w<DT, 2, DUAL>(a, waves < 8 ? waves : 8, st);
}

static void launch_nv4_frag(const Nv4FragBatch& b, int tensors, void* wd, int k, int dtype, hipStream_t st) {
  const size_t most = (size_t)((b.N[0] > b.N[1] ? b.N[0] : b.N[1]) >> 4) * (k >> 7) * 64;
  const dim3 grid((unsigned)((most + 255) / 256), (unsigned)tensors);
  if (dtype == VRA_BF16) nvfp4_dequant_frag_kernel<BF16><<<grid, 256, 0, st>>>(b, static_cast<u32x4*>(wd), k);
  else nvfp4_dequant_frag_kernel<F16><<<grid, 256, 0, st>>>(b, static_cast<u32x4*>(wd), k);
}

template <bool DUAL>
static void nv4_dispatch(const void* x, const void* w0, const void* s0, float g0, const void* w1, const void* s1, float g1, const void* bias,
                         const void* residual, void* out, int m, int k, int n, int dtype, int64_t stream) {
  hipStream_t st = as_stream(stream);
  if (m <= g_nv4_decode_rows) {
    GemvNv4Args a{};
    a.x = x, a.w[0] = w0, a.w[1] = w1, a.sc[0] = s0, a.sc[1] = s1, a.g[0] = g0, a.g[1] = g1;
    a.bias = bias, a.residual = residual, a.out = out, a.M = m, a.K = k, a.N = n;
    if (dtype == VRA_BF16) launch_gemv_nv4<BF16, DUAL>(a, st);
    else launch_gemv_nv4<F16, DUAL>(a, st);
    return;
  }
  // the weights widened once (exact, without g: the same real numbers the decode kernel feeds its MFMAs), then the 256-row dense GEMM
  // with g on its finished f32 sums
  const int nv = DUAL ? 2 * n : n;
  void* wd = vra_dense_scratch((size_t)k * nv * 2, stream);
  VRA_CHECK_ARG(wd, "nvfp4: the %zu-byte scratch for the widened weights is unavailable (allocation failed, or it would have to grow inside a stream capture)",
                (size_t)k * nv * 2);
  Nv4FragBatch b{};
  b.w[0] = static_cast<const u32x4*>(w0), b.sc[0] = static_cast<const uint32_t*>(s0), b.N[0] = n, b.vfrag0[0] = 0, b.vstride[0] = DUAL ? 2 : 1;
  b.w[1] = static_cast<const u32x4*>(w1), b.sc[1] = static_cast<const uint32_t*>(s1), b.N[1] = DUAL ? n : 0, b.vfrag0[1] = 1, b.vstride[1] = 2;
  launch_nv4_frag(b, DUAL ? 2 : 1, wd, k, dtype, st);
  GemmXArgs g{};
  g.x = x, g.x_ld = k, g.wd = wd, g.residual = residual, g.res_ld = n;
  g.seg[0] = GemmXSeg{out, bias, n, 0};
  g.nseg = 1;
  g.M = m, g.NV = nv, g.K = k, g.bias_in_f32 = 1;
  g.acc_scale_on = 1, g.acc_scale[0] = g0, g.acc_scale[1] = g1;
  vra_launch_gemm_dense(g, DUAL, dtype, vra_gemm_dense_tile(m, nv, k), stream);
}

// shapes this path serves; anything else is an argument error before any launch.  (Every operand under 0x7FFFFFF0 bytes: buffer
// descriptors, and NV4_OOB stays out of range.)
#define VRA_NV4_CHECK_SHAPE(name, m, k, n, dtype)                                                                                                 \
  do {                                                                                                                                            \
    VRA_CHECK_ARG((m) >= 1 && (k) >= 128 && (k) % 128 == 0 && (n) >= 16 && (n) % 16 == 0, name ": bad shape M=%d K=%d N=%d (K %% 128, N %% 16)", \
                  (int)(m), (int)(k), (int)(n));                                                                                                  \
    VRA_CHECK_ARG((dtype) == VRA_BF16 || (dtype) == VRA_F16, name ": dtype must be bf16/f16");                                                    \
    VRA_CHECK_ARG((uint64_t)(m) * (uint64_t)(k) * 2u < 0x7FFFFFF0ull && (uint64_t)(n) * (uint64_t)(k) * 4u < 0x7FFFFFF0ull, name ": operand over 2 GiB"); \
  } while (0)

extern "C" void vra_nvfp4_repack(const void* weight_packed, const void* weight_scale, void* w_tiled, void* s_tiled, int32_t n, int32_t k, int64_t stream) {
  VRA_CHECK_ARG(weight_packed && weight_scale && w_tiled && s_tiled, "nvfp4_repack: null pointer");
  VRA_NV4_CHECK_SHAPE("nvfp4_repack", 1, k, n, VRA_BF16);
  const size_t total = (size_t)(n >> 4) * (k >> 7) * 64;
  nv4_repack_kernel<<<dim3((unsigned)((total + 255) / 256)), 256, 0, as_stream(stream)>>>(
      static_cast<const uint8_t*>(weight_packed), static_cast<const uint8_t*>(weight_scale), static_cast<u32x4*>(w_tiled), static_cast<uint32_t*>(s_tiled), n, k);
}

extern "C" void vra_nvfp4_gemm(const void* x, const void* w_tiled, const void* s_tiled, float global_scale, const void* bias, const void* residual,
                               void* out, int32_t m, int32_t k, int32_t n, int32_t dtype, int64_t stream) {
  VRA_CHECK_ARG(x && w_tiled && s_tiled && out, "nvfp4_gemm: null pointer");
  VRA_NV4_CHECK_SHAPE("nvfp4_gemm", m, k, n, dtype);
  VRA_CHECK_ARG(std::isfinite(global_scale), "nvfp4_gemm: the global scale must be finite");
  nv4_dispatch<false>(x, w_tiled, s_tiled, global_scale, nullptr, nullptr, 1.0f, bias, residual, out, m, k, n, dtype, stream);
}

extern "C" void vra_nvfp4_gate_up_silu(const void* x, const void* w_gate, const void* s_gate, float g_gate, const void* w_up, const void* s_up,
                                       float g_up, void* out, int32_t m, int32_t k, int32_t n, int32_t dtype, int64_t stream) {
  VRA_CHECK_ARG(x && w_gate && s_gate && w_up && s_up && out, "nvfp4_gate_up_silu: null pointer");
  VRA_NV4_CHECK_SHAPE("nvfp4_gate_up_silu", m, k, n, dtype);
  VRA_CHECK_ARG(std::isfinite(g_gate) && std::isfinite(g_up), "nvfp4_gate_up_silu: the global scales must be finite");
  nv4_dispatch<true>(x, w_gate, s_gate, g_gate, w_up, s_up, g_up, nullptr, nullptr, out, m, k, n, dtype, stream);
}

extern "C" void vra_nvfp4_dequant_frag(const void* w_tiled, const void* s_tiled, void* wd, int32_t k, int32_t n, int32_t dtype, int32_t vfrag0,
                                       int32_t vstride, int64_t stream) {
  VRA_CHECK_ARG(w_tiled && s_tiled && wd, "nvfp4_dequant_frag: null pointer");
  VRA_NV4_CHECK_SHAPE("nvfp4_dequant_frag", 1, k, n, dtype);
  VRA_CHECK_ARG(vstride >= 1 && vfrag0 >= 0, "nvfp4_dequant_frag: bad fragment placement");
  Nv4FragBatch b{};
  b.w[0] = static_cast<const u32x4*>(w_tiled), b.sc[0] = static_cast<const uint32_t*>(s_tiled), b.N[0] = n, b.vfrag0[0] = vfrag0, b.vstride[0] = vstride;
  launch_nv4_frag(b, 1, wd, k, dtype, as_stream(stream));
}
