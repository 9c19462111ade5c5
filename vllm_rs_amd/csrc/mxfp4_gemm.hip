// mxfp4_gemm.hip — launchers and C entry points of the MXFP4 linears (reference: LnMxfp4, src/models/layers/linear.rs:1078-1144):
// vra_mxfp4_repack (checkpoint rows -> tile layout), vra_mxfp4_gemm and vra_mxfp4_gate_up_silu, which run the decode kernel
// (gemv_mx4.cuh) up to 32 rows and, above, the widening pass into vra_dense_scratch followed by kernel X (gemm_dense.cuh), and
// vra_mxfp4_dequant_frag (that pass alone).  No synchronisation; the scratch is the only allocation and never grows inside a capture.
#include "gemv_mx4.cuh"

#include "gemm_dense_launch.h"

static int mx4_num_cus() {
  static int n[64] = {0};
  int dev = 0;
  (void)hipGetDevice(&dev);
  dev &= 63;
  if (!n[dev] && (hipDeviceGetAttribute(&n[dev], hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n[dev] <= 0)) n[dev] = 256;
  return n[dev];
}

// Rows up to which the decode kernel serves a GEMM (it pads to 16 or 32 rows); above, pass + kernel X.
static int g_mx4_decode_rows = 32;
// measurement aid (tools/mxfp4_gemm_bench.py prices both routes at the same row count): 0..32, the kernel pads to at most 32 rows
extern "C" void vra_debug_set_mxfp4_decode_max_rows(int32_t rows) { g_mx4_decode_rows = rows < 0 ? 0 : (rows > 32 ? 32 : rows); }

// synthetic weights (host/model.cpp qlinear_synth): iid codes in the tile layout directly, scale bytes 119 | 120 in every byte of the
// scale words (2^-8, 2^-7 against the codes' rms of 2.93: weights of std ~ 0.02; inside the f16 range)
__global__ __launch_bounds__(256) void mx4_fill_kernel(uint32_t* __restrict__ w, size_t w_words, uint32_t* __restrict__ s, size_t s_words, uint64_t seed) {
  const size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
  if (i < w_words) w[i] = vra_hash32(seed, i);
  if (i < s_words) s[i] = 0x77777777u + (vra_hash32(seed + 1, i) & 0x01010101u);
}
void vra_launch_mxfp4_fill(void* w_tiled, void* s_tiled, int n, int k, uint64_t seed, int64_t stream) {
  const size_t ww = (size_t)n * k / 8, sw = (size_t)n * k / 128;
  mx4_fill_kernel<<<dim3((unsigned)((ww + 255) / 256)), 256, 0, as_stream(stream)>>>(static_cast<uint32_t*>(w_tiled), ww, static_cast<uint32_t*>(s_tiled), sw, seed);
}

template <class DT, int MT, bool DUAL>
static void launch_gemv_mx4_w(const GemvMx4Args& a, int waves, hipStream_t st) {
  const dim3 grid((unsigned)(a.N >> 4));
  if (waves == 4) gemv_mx4_kernel<DT, MT, 4, DUAL><<<grid, 256, 0, st>>>(a);
  else if (waves == 8) gemv_mx4_kernel<DT, MT, 8, DUAL><<<grid, 512, 0, st>>>(a);
  else if constexpr (MT == 1 && !DUAL) gemv_mx4_kernel<DT, MT, 16, DUAL><<<grid, 1024, 0, st>>>(a);
  else vra_set_error("mxfp4 decode kernel: two row tiles, or two tensors, run on at most 8 waves");
}
template <class DT, bool DUAL>
static void launch_gemv_mx4(const GemvMx4Args& a, hipStream_t st) {
  // waves of a workgroup: each CU should hold ~16 streaming waves whatever the number of 16-column units
  const int units = a.N >> 4, cus = mx4_num_cus();
  const int waves = units >= 2 * cus ? 4 : (units >= cus ? 8 : 16);
  // (16 waves leave 128 registers each: enough for one row tile of one tensor only — and a DUAL wave already keeps two tensors' rings in flight)
  if (a.M <= 16) launch_gemv_mx4_w<DT, 1, DUAL>(a, DUAL && waves > 8 ? 8 : waves, st);
  else launch_gemv_mx4_w<DT, 2, DUAL>(a, waves < 8 ? waves : 8, st);
}

static void launch_mx4_frag(const Mx4FragBatch& b, int tensors, void* wd, int k, int dtype, hipStream_t st) {
  const size_t most = (size_t)((b.N[0] > b.N[1] ? b.N[0] : b.N[1]) >> 4) * (k >> 7) * 64;
  const dim3 grid((unsigned)((most + 255) / 256), (unsigned)tensors);
  if (dtype == VRA_BF16) mxfp4_dequant_frag_kernel<BF16><<<grid, 256, 0, st>>>(b, static_cast<u32x4*>(wd), k);
  else mxfp4_dequant_frag_kernel<F16><<<grid, 256, 0, st>>>(b, static_cast<u32x4*>(wd), k);
}

template <bool DUAL>
static void mx4_dispatch(const void* x, const void* w0, const void* s0, const void* w1, const void* s1, const void* bias, const void* residual,
                         void* out, int m, int k, int n, int dtype, int64_t stream) {
  hipStream_t st = as_stream(stream);
  if (m <= g_mx4_decode_rows) {
    GemvMx4Args a{};
    a.x = x, a.w[0] = w0, a.w[1] = w1, a.sc[0] = s0, a.sc[1] = s1;
    a.bias = bias, a.residual = residual, a.out = out, a.M = m, a.K = k, a.N = n;
    if (dtype == VRA_BF16) launch_gemv_mx4<BF16, DUAL>(a, st);
    else launch_gemv_mx4<F16, DUAL>(a, st);
    return;
  }
  // the weights widened once (exact: the same real numbers the decode kernel feeds its MFMAs), then the 256-row dense GEMM
  const int nv = DUAL ? 2 * n : n;
  void* wd = vra_dense_scratch((size_t)k * nv * 2, stream);
  VRA_CHECK_ARG(wd, "mxfp4: the %zu-byte scratch for the widened weights is unavailable (allocation failed, or it would have to grow inside a stream capture)",
                (size_t)k * nv * 2);
  Mx4FragBatch b{};
  b.w[0] = static_cast<const u32x4*>(w0), b.sc[0] = static_cast<const uint32_t*>(s0), b.N[0] = n, b.vfrag0[0] = 0, b.vstride[0] = DUAL ? 2 : 1;
  b.w[1] = static_cast<const u32x4*>(w1), b.sc[1] = static_cast<const uint32_t*>(s1), b.N[1] = DUAL ? n : 0, b.vfrag0[1] = 1, b.vstride[1] = 2;
  launch_mx4_frag(b, DUAL ? 2 : 1, wd, k, dtype, st);
  GemmXArgs g{};
  g.x = x, g.x_ld = k, g.wd = wd, g.residual = residual, g.res_ld = n;
  g.seg[0] = GemmXSeg{out, bias, n, 0};
  g.nseg = 1;
  g.M = m, g.NV = nv, g.K = k, g.bias_in_f32 = 1;
  vra_launch_gemm_dense(g, DUAL, dtype, vra_gemm_dense_tile(m, nv, k), stream);
}

// shapes this path serves; anything else is an argument error before any launch.  (Every operand under 0x7FFFFFF0 bytes: buffer
// descriptors, and MX4_OOB stays out of range.)
#define VRA_MX4_CHECK_SHAPE(name, m, k, n, dtype)                                                                                                 \
  do {                                                                                                                                            \
    VRA_CHECK_ARG((m) >= 1 && (k) >= 128 && (k) % 128 == 0 && (n) >= 16 && (n) % 16 == 0, name ": bad shape M=%d K=%d N=%d (K %% 128, N %% 16)", \
                  (int)(m), (int)(k), (int)(n));                                                                                                  \
    VRA_CHECK_ARG((dtype) == VRA_BF16 || (dtype) == VRA_F16, name ": dtype must be bf16/f16");                                                    \
    VRA_CHECK_ARG((uint64_t)(m) * (uint64_t)(k) * 2u < 0x7FFFFFF0ull && (uint64_t)(n) * (uint64_t)(k) * 4u < 0x7FFFFFF0ull, name ": operand over 2 GiB"); \
  } while (0)

extern "C" void vra_mxfp4_repack(const void* weight_packed, const void* weight_scale, void* w_tiled, void* s_tiled, int32_t n, int32_t k, int64_t stream) {
  VRA_CHECK_ARG(weight_packed && weight_scale && w_tiled && s_tiled, "mxfp4_repack: null pointer");
  VRA_MX4_CHECK_SHAPE("mxfp4_repack", 1, k, n, VRA_BF16);
  const size_t total = (size_t)(n >> 4) * (k >> 7) * 64;
  mx4_repack_kernel<<<dim3((unsigned)((total + 255) / 256)), 256, 0, as_stream(stream)>>>(
      static_cast<const uint8_t*>(weight_packed), static_cast<const uint8_t*>(weight_scale), static_cast<u32x4*>(w_tiled), static_cast<uint32_t*>(s_tiled), n, k);
}

extern "C" void vra_mxfp4_gemm(const void* x, const void* w_tiled, const void* s_tiled, const void* bias, const void* residual, void* out,
                               int32_t m, int32_t k, int32_t n, int32_t dtype, int64_t stream) {
  VRA_CHECK_ARG(x && w_tiled && s_tiled && out, "mxfp4_gemm: null pointer");
  VRA_MX4_CHECK_SHAPE("mxfp4_gemm", m, k, n, dtype);
  mx4_dispatch<false>(x, w_tiled, s_tiled, nullptr, nullptr, bias, residual, out, m, k, n, dtype, stream);
}

extern "C" void vra_mxfp4_gate_up_silu(const void* x, const void* w_gate, const void* s_gate, const void* w_up, const void* s_up, void* out,
                                       int32_t m, int32_t k, int32_t n, int32_t dtype, int64_t stream) {
  VRA_CHECK_ARG(x && w_gate && s_gate && w_up && s_up && out, "mxfp4_gate_up_silu: null pointer");
  VRA_MX4_CHECK_SHAPE("mxfp4_gate_up_silu", m, k, n, dtype);
  mx4_dispatch<true>(x, w_gate, s_gate, w_up, s_up, nullptr, nullptr, out, m, k, n, dtype, stream);
}

extern "C" void vra_mxfp4_dequant_frag(const void* w_tiled, const void* s_tiled, void* wd, int32_t k, int32_t n, int32_t dtype, int32_t vfrag0,
                                       int32_t vstride, int64_t stream) {
  VRA_CHECK_ARG(w_tiled && s_tiled && wd, "mxfp4_dequant_frag: null pointer");
  VRA_MX4_CHECK_SHAPE("mxfp4_dequant_frag", 1, k, n, dtype);
  VRA_CHECK_ARG(vstride >= 1 && vfrag0 >= 0, "mxfp4_dequant_frag: bad fragment placement");
  Mx4FragBatch b{};
  b.w[0] = static_cast<const u32x4*>(w_tiled), b.sc[0] = static_cast<const uint32_t*>(s_tiled), b.N[0] = n, b.vfrag0[0] = vfrag0, b.vstride[0] = vstride;
  launch_mx4_frag(b, 1, wd, k, dtype, as_stream(stream));
}
