// fp8_gemm.hip — launchers and C entry points of the FP8 E4M3 block-scaled linears (reference: LnFp8, src/models/layers/linear.rs:776-1076):
// vra_fp8_repack (checkpoint [N, K] bytes -> tile layout), vra_fp8_gemm and vra_fp8_gate_up_silu, which run the decode kernel
// (gemv_f8.cuh) where fp8_decode_fits() says so and the tile GEMM (gemm_f8.cuh) above.  No allocation, no synchronisation:
// every launch is graph-capturable.
#include "gemm_f8.cuh"

static int f8_cur_dev() {
  int dev = 0;
  (void)hipGetDevice(&dev);
  return dev & 63;
}
static int f8_num_cus() {
  static int n[64] = {0};
  const int dev = f8_cur_dev();
  if (!n[dev] && (hipDeviceGetAttribute(&n[dev], hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n[dev] <= 0)) n[dev] = 256;
  return n[dev];
}

// Rows up to which the streaming kernel serves a GEMM (it pads to 16 or 32 rows); above, the tile GEMM.
static int g_fp8_decode_rows = 32;
static bool fp8_decode_fits(int m) { return m <= g_fp8_decode_rows; }
// measurement aid (tools/fp8_gemm_bench.py prices both kernels at the same row count): 0..32, the kernel pads to at most 32 rows
extern "C" void vra_debug_set_fp8_decode_max_rows(int32_t rows) { g_fp8_decode_rows = rows < 0 ? 0 : (rows > 32 ? 32 : rows); }

// synthetic weights (host/model.cpp init_synthetic): iid E4M3 bytes with the exponent field in 4..7 (|w| in 2^-3 .. 1.875, no NaN)
__global__ __launch_bounds__(256) void fp8_fill_kernel(uint32_t* __restrict__ out, size_t words, uint64_t seed) {
  const size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
  if (i < words) out[i] = (vra_hash32(seed, i) & 0x9F9F9F9Fu) | 0x20202020u;
}
void vra_launch_fp8_fill(void* out, size_t bytes, uint64_t seed, int64_t stream) {
  const size_t words = bytes / 4;
  if (words) fp8_fill_kernel<<<dim3((unsigned)((words + 255) / 256)), 256, 0, as_stream(stream)>>>(static_cast<uint32_t*>(out), words, seed);
}

// waves of a decode workgroup: each CU should hold ~16 streaming waves whatever the number of 16-column units
static int fp8_decode_waves(int units) {
  const int cus = f8_num_cus();
  return units >= 2 * cus ? 4 : (units >= cus ? 8 : 16);
}
// tile height of the prefill GEMM: 256 rows when such tiles already fill the chip, else 128 (twice the workgroups)
static int fp8_gemm_tile_m(int m, int nv) {
  const long t256 = (long)((m + 255) / 256) * ((nv + 127) / 128);
  return (m > 128 && t256 >= f8_num_cus()) ? 256 : 128;
}

template <class DT, int MT, bool DUAL>
static void launch_gemv_f8_w(const GemvF8Args& a, int waves, hipStream_t st) {
  const dim3 grid((unsigned)(a.N >> 4));
  if (waves == 4) gemv_f8_kernel<DT, MT, 4, DUAL><<<grid, 256, 0, st>>>(a);
  else if (waves == 8) gemv_f8_kernel<DT, MT, 8, DUAL><<<grid, 512, 0, st>>>(a);
  else if constexpr (MT == 1) gemv_f8_kernel<DT, MT, 16, DUAL><<<grid, 1024, 0, st>>>(a);
  else vra_set_error("fp8 decode kernel: two row tiles run on at most 8 waves");
}
template <class DT, bool DUAL>
static void launch_gemv_f8(const GemvF8Args& a, hipStream_t st) {
  const int waves = fp8_decode_waves(a.N >> 4);
  if (a.M <= 16) launch_gemv_f8_w<DT, 1, DUAL>(a, waves, st);
  else launch_gemv_f8_w<DT, 2, DUAL>(a, waves < 8 ? waves : 8, st);  // (two row tiles: 16 waves would leave 128 registers each)
}

template <class DT, int BM, bool DUAL>
static void launch_gemm_f8_t(GemmF8Args a, hipStream_t st) {
  const size_t lds = gemm_f8_lds_bytes(BM);
  static uint64_t attr_devs = 0;  // per device: function attributes belong to the device current at the call
  if (!((attr_devs >> f8_cur_dev()) & 1)) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_f8_kernel<DT, BM, DUAL>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    attr_devs |= (uint64_t)1 << f8_cur_dev();
  }
  a.MT = (a.M + BM - 1) / BM;
  a.NT = ((DUAL ? 2 * a.N : a.N) + 127) / 128;
  gemm_f8_kernel<DT, BM, DUAL><<<dim3((unsigned)(a.MT * a.NT)), BM * 2, lds, st>>>(a);
}
template <class DT, bool DUAL>
static void launch_gemm_f8(const GemmF8Args& a, hipStream_t st) {
  if (fp8_gemm_tile_m(a.M, DUAL ? 2 * a.N : a.N) == 256) launch_gemm_f8_t<DT, 256, DUAL>(a, st);
  else launch_gemm_f8_t<DT, 128, DUAL>(a, st);
}

template <bool DUAL>
static void fp8_dispatch(const void* x, const void* w0, const float* s0, const void* w1, const float* s1, const void* bias, const void* residual,
                         void* out, int m, int k, int n, int dtype, hipStream_t st) {
  const bool bf = dtype == VRA_BF16;
  if (fp8_decode_fits(m)) {
    GemvF8Args a{};
    a.x = x, a.w[0] = static_cast<const u32x4*>(w0), a.w[1] = static_cast<const u32x4*>(w1), a.sc[0] = s0, a.sc[1] = s1;
    a.bias = bias, a.residual = residual, a.out = out, a.M = m, a.K = k, a.N = n;
    if (bf) launch_gemv_f8<BF16, DUAL>(a, st);
    else launch_gemv_f8<F16, DUAL>(a, st);
  } else {
    GemmF8Args a{};
    a.x = x, a.w[0] = w0, a.w[1] = w1, a.sc[0] = s0, a.sc[1] = s1;
    a.bias = bias, a.residual = residual, a.out = out, a.M = m, a.K = k, a.N = n;
    if (bf) launch_gemm_f8<BF16, DUAL>(a, st);
    else launch_gemm_f8<F16, DUAL>(a, st);
  }
}

// shapes of the format this path serves; anything else is an argument error before any launch
#define VRA_FP8_CHECK_SHAPE(name, m, k, n, bn, bk, dtype)                                                                                        \
  do {                                                                                                                                           \
    VRA_CHECK_ARG((bn) == F8_BLOCK && (bk) == F8_BLOCK, name ": weight_block_size must be [128, 128], got [%d, %d]", (int)(bn), (int)(bk));      \
    VRA_CHECK_ARG((m) >= 1 && (k) >= F8_BLOCK && (k) % F8_BLOCK == 0 && (n) >= 16 && (n) % 16 == 0, name ": bad shape M=%d K=%d N=%d (K %% 128, N %% 16)", \
                  (int)(m), (int)(k), (int)(n));                                                                                                 \
    VRA_CHECK_ARG((dtype) == VRA_BF16 || (dtype) == VRA_F16, name ": dtype must be bf16/f16");                                                   \
    VRA_CHECK_ARG((uint64_t)(m) * (uint64_t)(k) * 2u < 0x7FFFFFF0ull && (uint64_t)(n) * (uint64_t)(k) < 0x7FFFFFF0ull, name ": operand over 2 GiB"); \
  } while (0)

extern "C" void vra_fp8_repack(const void* weight, void* out, int32_t n, int32_t k, int32_t block_n, int32_t block_k, int64_t stream) {
  VRA_CHECK_ARG(weight && out, "fp8_repack: null pointer");
  VRA_FP8_CHECK_SHAPE("fp8_repack", 1, k, n, block_n, block_k, VRA_BF16);
  const size_t total = (size_t)(n >> 4) * (k >> 6) * 64;
  fp8_repack_kernel<<<dim3((unsigned)((total + 255) / 256)), 256, 0, as_stream(stream)>>>(static_cast<const uint8_t*>(weight), static_cast<u32x4*>(out), n, k);
}

extern "C" void vra_fp8_gemm(const void* x, const void* weight_tiled, const float* scales, const void* bias, const void* residual, void* out,
                             int32_t m, int32_t k, int32_t n, int32_t block_n, int32_t block_k, int32_t dtype, int64_t stream) {
  VRA_CHECK_ARG(x && weight_tiled && scales && out, "fp8_gemm: null pointer");
  VRA_FP8_CHECK_SHAPE("fp8_gemm", m, k, n, block_n, block_k, dtype);
  fp8_dispatch<false>(x, weight_tiled, scales, nullptr, nullptr, bias, residual, out, m, k, n, dtype, as_stream(stream));
}

extern "C" void vra_fp8_gate_up_silu(const void* x, const void* w_gate, const float* s_gate, const void* w_up, const float* s_up, void* out,
                                     int32_t m, int32_t k, int32_t n, int32_t block_n, int32_t block_k, int32_t dtype, int64_t stream) {
  VRA_CHECK_ARG(x && w_gate && s_gate && w_up && s_up && out, "fp8_gate_up_silu: null pointer");
  VRA_FP8_CHECK_SHAPE("fp8_gate_up_silu", m, k, n, block_n, block_k, dtype);
  fp8_dispatch<true>(x, w_gate, s_gate, w_up, s_up, nullptr, nullptr, out, m, k, n, dtype, as_stream(stream));
}
