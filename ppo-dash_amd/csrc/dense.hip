// The dense layers of the network on the tile-GEMM cores (igemm.h: fp32 MFMA,
// igemm_x9.h: exact split on the bf16 matrix cores): the CNNBase fc layer and the
// generic linear forward / input gradient / weight gradient used by the GRU and
// MLP bases, the split-K reductions, and the weight packer that writes the k
// orders and bf16 planes the conv and fc kernels read.
#include "conv_launch.h"

namespace {

// Pack torch-layout weights into the loaders' k orders (once per optimizer step).
//   W2p [64][512]  (ky,kx,ci)       W3p [32][576] (ky,kx,ci)
//   W4p [H][1568]  (p,c)            W4T [1568][H] (p,c) x n
//   W3d [64][288]  ci x (ky,kx,co)  W2d [4][32][256] phase x ci x (ty,tx,co)
// Each f32 segment of n values is followed by its exact bf16 split (hi, mid, lo
// planes of n bf16 each = 1.5 n floats), the B operand of the igemm_x9 core.
__host__ __device__ inline void pack_segments(int H, long long* n) {
  n[0] = 64 * 512; n[1] = 32 * 576; n[2] = (long long)H * 1568; n[3] = n[2]; n[4] = 64 * 288; n[5] = 4 * 32 * 256;
}

__global__ __launch_bounds__(256) void pack_weights_kernel(const float* __restrict__ w2, const float* __restrict__ w3,
                                                           const float* __restrict__ w4, int H,
                                                           float* __restrict__ out) {
  long long n[6];
  pack_segments(H, n);
  const long long total = n[0] + n[1] + n[2] + n[3] + n[4] + n[5];
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    long long j = i, base = 0;
    int seg = 0;
    while (j >= n[seg]) {
      j -= n[seg];
      base += n[seg] * 5 / 2;
      ++seg;
    }
    float v;
    if (seg == 0) {
      const int co = (int)(j / 512), k = (int)(j % 512), ky = k / 128, kx = (k / 32) % 4, ci = k % 32;
      v = w2[co * 512 + ci * 16 + ky * 4 + kx];
    } else if (seg == 1) {
      const int co = (int)(j / 576), k = (int)(j % 576), ky = k / 192, kx = (k / 64) % 3, ci = k % 64;
      v = w3[co * 576 + ci * 9 + ky * 3 + kx];
    } else if (seg == 2) {
      const long long nn = j / 1568;
      const int k = (int)(j % 1568), pp = k / 32, c = k % 32;
      v = w4[nn * 1568 + c * 49 + pp];
    } else if (seg == 3) {
      const int k = (int)(j / H), nn = (int)(j % H), pp = k / 32, c = k % 32;
      v = w4[(long long)nn * 1568 + c * 49 + pp];
    } else if (seg == 4) {
      const int ci = (int)(j / 288), k = (int)(j % 288), ky = k / 96, kx = (k / 32) % 3, co = k % 32;
      v = w3[co * 576 + ci * 9 + ky * 3 + kx];
    } else {
      const int ph = (int)(j / 8192), rem = (int)(j % 8192), ci = rem / 256, k = rem % 256;
      const int ty = k >> 7, tx = (k >> 6) & 1, co = k & 63;
      const int ky = (ph >> 1) + 2 * ty, kx = (ph & 1) + 2 * tx;
      v = w2[co * 512 + ci * 16 + ky * 4 + kx];
    }
    out[base + j] = v;
    uint32_t h, m, l;
    split_bf16x3(v, h, m, l);
    uint16_t* pl = reinterpret_cast<uint16_t*>(out + base + n[seg]);
    pl[j] = (uint16_t)h;
    pl[n[seg] + j] = (uint16_t)m;
    pl[2 * n[seg] + j] = (uint16_t)l;
  }
}

}  // namespace

// floats: every segment is followed by its three bf16 planes (1.5 x its size)
PPO_API long long ppo_packed_weights_size(int H) {
  long long n[6];
  pack_segments(H, n);
  return (n[0] + n[1] + n[2] + n[3] + n[4] + n[5]) * 5 / 2;
}

// offsets (floats) of the packed f32 segments W2p W3p W4p W4T W3d W2d inside the pack buffer
PPO_API int ppo_packed_offsets(int H, long long* off6) {
  long long n[6];
  pack_segments(H, n);
  off6[0] = 0;
  for (int i = 1; i < 6; ++i) off6[i] = off6[i - 1] + n[i - 1] * 5 / 2;
  return 0;
}

PPO_API int ppo_pack_weights(const float* w2, const float* w3, const float* w4, int H, float* packed, void* stream) {
  ProfScope prof("pack_weights", as_stream(stream), 4.0 * 4.0 * ppo_packed_weights_size(H));
  PPO_REQUIRE(H > 0 && H % 4 == 0, "ppo_pack_weights: hidden size %d must be a positive multiple of 4", H);
  long long n[6];
  pack_segments(H, n);
  const long long total = n[0] + n[1] + n[2] + n[3] + n[4] + n[5];
  long long b = (total + 255) / 256;
  pack_weights_kernel<<<(unsigned)(b < 2048 ? b : 2048), 256, 0, as_stream(stream)>>>(w2, w3, w4, H, packed);
  PPO_LAUNCH_CHECK("pack_weights_kernel");
  return 0;
}

// fp32-MFMA tile core (x9 = 0 and the fallbacks)
using CfgN64 = Cfg<128, 64, 2, 2, true, true>;
using CfgN128 = Cfg<128, 128, 2, 2, true, true>;
using CfgWfc = Cfg<128, 128, 2, 2, false, false, true>;   // wgrad
// exact-split bf16 core (igemm_x9.h)
using X64 = CfgX<128, 64, 2, 2, true, true>;          // N = 64: waves of 64x32
using X128 = CfgX<128, 128, 2, 2, true, true>;        // N >= 128: waves of 64x64
using X64s = CfgX<64, 64, 2, 2, true, true>;          // few 128 x 128 tiles (rollout rows): waves of 32x32
using XW64 = CfgX<64, 128, 2, 2, false, false, true>;   // wgrad, 64 output channels
using XP128 = CfgX<128, 128, 4, 1, true, true, false, false, false, true>;  // B from planes, waves 32x128
using XP128w8 = CfgX<128, 128, 8, 1, true, true, false, false, false, true>;      // 8 waves of 16x128
using XP128x64w8 = CfgX<128, 64, 8, 1, true, true, false, false, false, true>;    // 8 waves of 16x64 (2 blocks/CU)
// split-at-staging form (igemm_x9s_kernel): both operands split once per block into bf16 planes in LDS
using SW256x128 = CfgS<256, 128, 4, 2, false, false, true>;      // wgrad: 8 waves of 64x64 (144 KB LDS)

// x9 = 1: the split-bf16 core where it measured faster (the dense forward / dgrad, the
// fc weight gradient); x9 = 2: also the narrow GRU / MLP weight gradients; 0: fp32 MFMA
static inline bool use_x9() { return tune_key(TK_X9) != 0; }
static inline bool use_x9_all() { return tune_key(TK_X9) == 2; }

// CNNBase fc (model.py:181): out[m * ldo + n] = relu(x [M][1568] · W4p [H][1568]^T + b), W4p the packed
// segment of ppo_pack_weights (its bf16 planes follow it)
PPO_API int ppo_fc_fwd(const float* x, int M, const float* w4p, const float* b, int H, float* out, int ldo,
                       void* stream) {
  PPO_REQUIRE(H > 0 && H % 8 == 0 && ldo >= H, "ppo_fc_fwd: H=%d ldo=%d", H, ldo);
  const int K = 1568;
  if (M > 0 && M <= tune_small_b()) return small_linear_fwd(x, nullptr, M, K, K, w4p, b, H, out, ldo, 1, as_stream(stream));
  if (use_x9()) {
    // tiles dealt n-fastest per XCD (igemm_x9.h tile_of); rollout-sized M (4096 rows)
    // fills a quarter of the chip with 128 x 128 tiles: 8 waves of 16 x 64 there
    // (0.060 vs 0.070 ms for 128 x 64)
    const bool wide = ((M + 127LL) / 128) * ((H + 127) / 128) >= 2LL * device_cus();
    const bool abuf = 4LL * M * K < 0x80000000LL;   // DenseReluFwdB's 32-bit offsets
#define PPO_FC(T, CFG)                                                                               \
  {                                                                                                  \
    T<CFG> p;                                                                                        \
    p.x = x; p.w = w4p; p.bias = b; p.out = out; p.M = M; p.N = H; p.K = K; p.ldo = ldo; p.relu = 1; \
    set_planes(p, w4p, (long long)H * K, H, K);                                                      \
    p.n_fast = 1;                                                                                    \
    p.vec = H % 4 == 0 && ldo % 4 == 0 && ((uintptr_t)out & 15) == 0 &&                              \
            (b == nullptr || ((uintptr_t)b & 15) == 0);                                              \
    return launch_x9(p, M, H, 1, as_stream(stream), "fc_fwd", 2.0 * M * H * K);                      \
  }
    if (wide && abuf) PPO_FC(DenseReluFwdB, XP128)   // 0.546-0.551 ms; 8 waves of 16 x 128 0.563-0.565 (r05_v_fc_fwd_tiles_kbench.log)
    if (wide) PPO_FC(DenseReluFwd, XP128)
    if (abuf) PPO_FC(DenseReluFwdB, XP128x64w8)
    PPO_FC(DenseReluFwd, XP128x64w8)
#undef PPO_FC
  }
  DenseReluFwd<CfgN128> p;
  p.x = x; p.w = w4p; p.bias = b; p.out = out; p.M = M; p.N = H; p.K = K; p.ldo = ldo; p.relu = 1;
  return launch(p, M, H, 1, as_stream(stream), "fc_fwd", 2.0 * M * H * K);
}

// Split-K fc forward for rollout-sized M (4,096 rows): 49 k-steps of one 128 x 64 tile
// per CU are latency-bound (0.28 of the MFMA roofline); Z K-slices run Z blocks per
// tile (two resident per CU), their partials go to the caller's workspace slab
// [Z][M][H] and fc_splitk_reduce_kernel sums them in a fixed order, adds the bias
// and applies ReLU.
template <class C_>
struct DenseFwdSplitK : DenseReluFwdB<C_> {   // branch-free operand loads (the launcher checks 4·M·K < 2^31)
  float* slab = nullptr;
  int chunk = 0;   // k per slice, a multiple of 32
  __device__ void k_range(int z, int& b, int& e) const {
    b = z * chunk < this->K ? z * chunk : this->K;
    e = b + chunk < this->K ? b + chunk : this->K;
  }
  __device__ void store(int m, int n, int z, float v) const {
    if (m < this->M && n < this->N) slab[((size_t)z * this->M + m) * this->N + n] = v;
  }
  // vec = 1 (16-B slab rows): the raw partials of columns n .. n + 3 (no bias, no ReLU)
  __device__ void store4(int m, int n, int z, const f32x4& v) const {
    if (m < this->M && n < this->N) *reinterpret_cast<f32x4*>(slab + ((size_t)z * this->M + m) * this->N + n) = v;
  }
};

__global__ __launch_bounds__(256) void fc_splitk_reduce_kernel(const float* __restrict__ slab, int Z, int M, int N,
                                                               const float* __restrict__ bias, float* __restrict__ out,
                                                               int ldo) {
  const int n4 = N >> 2;
  const long long total = (long long)M * n4;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int m = (int)(i / n4), q = (int)(i - (long long)m * n4);
    const f32x4* src = reinterpret_cast<const f32x4*>(slab + (size_t)m * N) + q;
    f32x4 v = src[0];
    for (int z = 1; z < Z; ++z) v += src[(size_t)z * M * n4];
    const f32x4 b = reinterpret_cast<const f32x4*>(bias)[q];
    f32x4 y;
#pragma unroll
    for (int r = 0; r < 4; ++r) y[r] = fmaxf(v[r] + b[r], 0.f);
    *reinterpret_cast<f32x4*>(out + (size_t)m * ldo + 4 * q) = y;
  }
}

// ppo_fc_fwd with a caller-owned workspace (ws, ws_bytes): rollout-sized M takes the
// split-K form when ws holds its slab (ppo_fc_fwd_ws_bytes), else ppo_fc_fwd
PPO_API long long ppo_fc_fwd_ws_bytes(int M, int H) {
  const int Z = tune_key(TK_FC_SPLITK);
  if (Z <= 1 || M <= tune_small_b() || (long long)M * H > 4096LL * 1024) return 0;
  return 4LL * Z * M * H;
}

PPO_API int ppo_fc_fwd_ws(const float* x, int M, const float* w4p, const float* b, int H, float* out, int ldo,
                          float* ws, long long ws_bytes, void* stream) {
  const long long need = ppo_fc_fwd_ws_bytes(M, H);
  if (!use_x9() || need == 0 || ws == nullptr || ws_bytes < need || ldo % 4 != 0 || H % 4 != 0 || 4LL * M * 1568 >= 0x80000000LL ||
      ((uintptr_t)out & 15) != 0 || ((uintptr_t)ws & 15) != 0 || ((uintptr_t)b & 15) != 0)
    return ppo_fc_fwd(x, M, w4p, b, H, out, ldo, stream);
  const int K = 1568, Z = (int)(need / (4LL * M * H));
  hipStream_t st = as_stream(stream);
  int rc;
#define PPO_FCSK(CFG, VEC)                                                                   \
  {                                                                                          \
    DenseFwdSplitK<CFG> p;                                                                   \
    p.x = x; p.w = w4p; p.bias = b; p.out = out; p.M = M; p.N = H; p.K = K; p.ldo = ldo; p.relu = 1; \
    set_planes(p, w4p, (long long)H * K, H, K);                                              \
    p.n_fast = 1;                                                                            \
    p.slab = ws;                                                                             \
    p.vec = VEC;                                                                             \
    p.chunk = ((K + Z - 1) / Z + 31) / 32 * 32;                                              \
    rc = launch_x9(p, M, H, Z, st, "fc_fwd", 2.0 * M * H * K);                               \
  }
  if (tune_key(TK_FC_SPLITK_TILE)) PPO_FCSK(XP128, 1)
  else PPO_FCSK(XP128x64w8, 0)
#undef PPO_FCSK
  if (rc) return rc;
  const long long n = (long long)M * (H / 4);
  fc_splitk_reduce_kernel<<<(unsigned)std::min<long long>((n + 255) / 256, 4096), 256, 0, st>>>(ws, Z, M, H, b, out,
                                                                                               ldo);
  PPO_LAUNCH_CHECK("fc_splitk_reduce_kernel");
  return 0;
}

// Linear + ReLU: out [M][N] = relu(x [M][K] · w [N][K]^T + b)
PPO_API int ppo_linear_relu_fwd(const float* x, int M, int K, const float* w, const float* b, int N, float* out,
                                void* stream) {
  PPO_REQUIRE(K % 4 == 0, "ppo_linear_relu_fwd: K=%d must be a multiple of 4", K);
  if (M > 0 && M <= tune_small_b()) return small_linear_fwd(x, nullptr, M, K, K, w, b, N, out, N, 1, as_stream(stream));
  if (use_x9()) {
    DenseReluFwd<X128> p;
    p.x = x; p.w = w; p.bias = b; p.out = out; p.M = M; p.N = N; p.K = K;
    return launch_x9(p, M, N, 1, as_stream(stream), "linear_relu_fwd", 2.0 * M * N * K);
  }
  if (N % 128 == 0) {
    DenseReluFwd<CfgN128> p;
    p.x = x; p.w = w; p.bias = b; p.out = out; p.M = M; p.N = N; p.K = K;
    return launch(p, M, N, 1, as_stream(stream), "linear_relu_fwd", 2.0 * M * N * K);
  }
  DenseReluFwd<CfgN64> p;
  p.x = x; p.w = w; p.bias = b; p.out = out; p.M = M; p.N = N; p.K = K;
  return launch(p, M, N, 1, as_stream(stream), "linear_relu_fwd", 2.0 * M * N * K);
}

// Linear with row strides: out[m*ldo + n] = act(x[idx(m)*lda + k] · w[n][k] + b[n]); b, idx may be NULL;
// act 0 none, 1 ReLU, 2 tanh
PPO_API int ppo_linear_fwd_ex(const float* x, const int64_t* idx, int M, int K, int lda, const float* w, const float* b,
                              int N, float* out, int ldo, int act, void* stream) {
  PPO_REQUIRE(K % 4 == 0 && lda % 4 == 0, "ppo_linear_fwd_ex: K=%d lda=%d must be multiples of 4", K, lda);
  PPO_REQUIRE(act >= 0 && act <= 2, "ppo_linear_fwd_ex: act=%d", act);
  if (M > 0 && M <= tune_small_b()) return small_linear_fwd(x, idx, M, K, lda, w, b, N, out, ldo, act, as_stream(stream));
  if (use_x9()) {
    if (N <= 64) {
      DenseReluFwd<X64> p;
      p.x = x; p.w = w; p.bias = b; p.out = out; p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldo = ldo; p.relu = act;
      p.idx = idx;
      return launch_x9(p, M, N, 1, as_stream(stream), "linear_fwd_ex", 2.0 * M * N * K);
    }
#define PPO_LEX(CFG)                                                                                       \
  {                                                                                                        \
    DenseReluFwd<CFG> p;                                                                                   \
    p.x = x; p.w = w; p.bias = b; p.out = out; p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldo = ldo; p.relu = act; \
    p.idx = idx;                                                                                           \
    p.vec = N % 4 == 0 && (ldo ? ldo : N) % 4 == 0 && ((uintptr_t)out & 15) == 0 &&                        \
            (b == nullptr || ((uintptr_t)b & 15) == 0);                                                    \
    return launch_x9(p, M, N, 1, as_stream(stream), "linear_fwd_ex", 2.0 * M * N * K);                     \
  }
    // rollout-sized M (the GRU input projection at 4,096 rows: 192 tiles of 128 x 128 for
    // 256 CUs) takes 64 x 64 tiles
    // 0.024 vs 0.028-0.031 ms at 4,096 x 272 x 768 (profiles/r05_m_gi.log)
    if (((M + 127LL) / 128) * ((N + 127) / 128) < 2LL * device_cus()) PPO_LEX(X64s)
    PPO_LEX(X128)
#undef PPO_LEX
  }
  if (N % 128 == 0) {
    DenseReluFwd<CfgN128> p;
    p.x = x; p.w = w; p.bias = b; p.out = out; p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldo = ldo; p.relu = act;
    p.idx = idx;
    return launch(p, M, N, 1, as_stream(stream), "linear_fwd_ex", 2.0 * M * N * K);
  }
  DenseReluFwd<CfgN64> p;
  p.x = x; p.w = w; p.bias = b; p.out = out; p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldo = ldo; p.relu = act;
  p.idx = idx;
  return launch(p, M, N, 1, as_stream(stream), "linear_fwd_ex", 2.0 * M * N * K);
}

// dx [M][N] = g(act) * (dy [M][K] · wt [N][K]^T); act row stride ldact (act NULL: no mask);
// mode 1: g = [act > 0] (ReLU), 2: g = 1 - act² (tanh)
PPO_API int ppo_linear_dgrad_ex(const float* dy, int M, int K, const float* wt, int N, const float* act, int ldact,
                                int mode, float* dx, void* stream) {
  PPO_REQUIRE(K % 4 == 0, "ppo_linear_dgrad_ex: K=%d must be a multiple of 4", K);
  if (use_x9()) {
    DenseDgradMask<X128> p;
    p.dy = dy; p.wt = wt; p.act = act; p.dx = dx; p.M = M; p.N = N; p.K = K; p.ldact = ldact; p.mode = mode;
    p.vec = N % 4 == 0 && (ldact ? ldact : N) % 4 == 0 && ((uintptr_t)dx & 15) == 0 &&
            (act == nullptr || ((uintptr_t)act & 15) == 0);
    return launch_x9(p, M, N, 1, as_stream(stream), "linear_dgrad_ex", 2.0 * M * N * K);
  }
  DenseDgradMask<CfgN128> p;
  p.dy = dy; p.wt = wt; p.act = act; p.dx = dx; p.M = M; p.N = N; p.K = K; p.ldact = ldact; p.mode = mode;
  return launch(p, M, N, 1, as_stream(stream), "linear_dgrad_ex", 2.0 * M * N * K);
}

// dx [M][N] = dy0 [M][K0] · wt0 [N][K0]^T + dy1 [M][K1] · wt1 [N][K1]^T: one launch, one accumulator
// per element, pair 0's k range before pair 1's (DenseDgradPair) — dL/d(GRU output) from MLPBase's
// critic and actor towers (model.py:231-232)
PPO_API int ppo_linear_dgrad_pair(const float* dy0, const float* wt0, int K0, const float* dy1, const float* wt1,
                                  int K1, int M, int N, float* dx, void* stream) {
  PPO_REQUIRE(K0 > 0 && K1 > 0 && K0 % 4 == 0 && K1 % 4 == 0,
              "ppo_linear_dgrad_pair: K0=%d K1=%d must be positive multiples of 4", K0, K1);
  PPO_REQUIRE(M >= 0 && N > 0, "ppo_linear_dgrad_pair: M=%d N=%d", M, N);
  const double flops = 2.0 * M * N * ((double)K0 + K1);
#define PPO_DGP(CFG, LAUNCH, VEC)                                                                  \
  {                                                                                                \
    DenseDgradPair<CFG> p;                                                                         \
    p.dy0 = dy0; p.wt0 = wt0; p.dy1 = dy1; p.wt1 = wt1; p.dx = dx; p.M = M; p.N = N; p.K0 = K0; p.K1 = K1; \
    p.vec = VEC;                                                                                   \
    return LAUNCH(p, M, N, 1, as_stream(stream), "linear_dgrad_pair", flops);                      \
  }
  if (use_x9()) {
    const int vec = N % 4 == 0 && ((uintptr_t)dx & 15) == 0;
    if (N <= 64) PPO_DGP(X64, launch_x9, vec)   // the H <= 64 towers: no half-empty 128-column tile
    PPO_DGP(X128, launch_x9, vec)
  }
  PPO_DGP(CfgN128, launch, 0)
#undef PPO_DGP
}

__global__ __launch_bounds__(256) void transpose_kernel(const float* __restrict__ src, int rows, int cols,
                                                        float* __restrict__ dst) {
  const long long total = (long long)rows * cols;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int c = (int)(i / rows), r = (int)(i - (long long)c * rows);
    dst[i] = src[(size_t)r * cols + c];
  }
}

// dst [cols][rows] = src [rows][cols]ᵀ (weight transposes for dgrad B operands)
PPO_API int ppo_transpose(const float* src, int rows, int cols, float* dst, void* stream) {
  PPO_REQUIRE(rows > 0 && cols > 0, "ppo_transpose: %d x %d", rows, cols);
  long long b = ((long long)rows * cols + 255) / 256;
  transpose_kernel<<<(unsigned)(b < 2048 ? b : 2048), 256, 0, as_stream(stream)>>>(src, rows, cols, dst);
  PPO_LAUNCH_CHECK("transpose_kernel");
  return 0;
}

// dx [M][N] = (act > 0) * (dy [M][K] · wt [N][K]^T)
PPO_API int ppo_linear_dgrad_mask(const float* dy, int M, int K, const float* wt, int N, const float* act, float* dx,
                                  void* stream) {
  PPO_REQUIRE(K % 4 == 0, "ppo_linear_dgrad_mask: K=%d must be a multiple of 4", K);
  if (use_x9()) {   // wt = the packed W4T segment [1568][H] (planes follow); 8 waves of 16 x 128:
    PPO_REQUIRE(K % 8 == 0, "ppo_linear_dgrad_mask: K=%d must be a multiple of 8", K);   // 0.75 vs 0.87 ms (4 waves)
#define PPO_DGM(T)                                                                                          \
  {                                                                                                         \
    T<XP128w8> p;                                                                                           \
    p.dy = dy; p.wt = wt; p.act = act; p.dx = dx; p.M = M; p.N = N; p.K = K;                                \
    set_planes(p, wt, (long long)N * K, N, K);                                                              \
    p.n_fast = 0;   /* m fastest: the 134 MB dy fits the Infinity Cache, the weight tile stays L2-resident */ \
    p.vec = N % 4 == 0 && ((uintptr_t)dx & 15) == 0 && (act == nullptr || ((uintptr_t)act & 15) == 0);     \
    return launch_x9(p, M, N, 1, as_stream(stream), "linear_dgrad_mask", 2.0 * M * N * K);                  \
  }
    if (4LL * M * K < 0x80000000LL) PPO_DGM(DenseDgradMaskB)   // 32-bit buffer offsets
    PPO_DGM(DenseDgradMask)
#undef PPO_DGM
  }
  DenseDgradMask<CfgN128> p;
  p.dy = dy; p.wt = wt; p.act = act; p.dx = dx; p.M = M; p.N = N; p.K = K;
  return launch(p, M, N, 1, as_stream(stream), "linear_dgrad_mask", 2.0 * M * N * K);
}

// The fc dgrad with conv3's ReLU mask as bits (ppo_conv3_fwd_mask: uint16 [M][49][2],
// bit j of word (p, t) = feature 32 p + 16 t + j): 196 B per row read in the epilogue
// instead of the 6,272 B fp32 activation (0.605 vs 0.695 ms for the fc dgrad at the c3
// minibatch with no mask read at all, profiles/r06_s8_fc_dgrad_mask_kbench.log)
template <class Base>
struct WithMask3Bits : Base {
  const uint16_t* mbits = nullptr;
  __device__ uint32_t bits(int m, int n) const { return (uint32_t)mbits[(size_t)m * 98 + (n >> 4)] >> (n & 15); }
  __device__ void store(int m, int n, int, float v) const {
    if (m < this->M && n < this->N) this->dx[(size_t)m * this->N + n] = (bits(m, n) & 1u) ? v : 0.f;
  }
  __device__ void store4(int m, int n, int, const f32x4& v) const {
    if (m >= this->M || n >= this->N) return;
    const uint32_t b = bits(m, n);
    f32x4 o;
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = ((b >> r) & 1u) ? v[r] : 0.f;
    *reinterpret_cast<f32x4*>(this->dx + (size_t)m * this->N + n) = o;
  }
};

PPO_API int ppo_fc_dgrad_bits(const float* dy, int M, int K, const float* wt, const uint16_t* mbits, float* dx,
                              void* stream) {
  PPO_REQUIRE(M >= 0 && K > 0 && K % 8 == 0 && mbits != nullptr, "ppo_fc_dgrad_bits: M=%d K=%d", M, K);
  const int N = 1568;
  if (use_x9() && 4LL * M * K < 0x80000000LL) {   // as ppo_linear_dgrad_mask (wt: the packed W4T segment)
    WithMask3Bits<DenseDgradMaskB<XP128w8>> p;
    p.dy = dy; p.wt = wt; p.act = nullptr; p.dx = dx; p.M = M; p.N = N; p.K = K; p.mbits = mbits;
    set_planes(p, wt, (long long)N * K, N, K);
    p.n_fast = 0;
    p.vec = ((uintptr_t)dx & 15) == 0;
    return launch_x9(p, M, N, 1, as_stream(stream), "linear_dgrad_mask", 2.0 * M * N * K);
  }
  WithMask3Bits<DenseDgradMask<CfgN128>> p;
  p.dy = dy; p.wt = wt; p.act = nullptr; p.dx = dx; p.M = M; p.N = N; p.K = K; p.mbits = mbits;
  return launch(p, M, N, 1, as_stream(stream), "linear_dgrad_mask", 2.0 * M * N * K);
}

// split count and chunk for a wgrad reduction of R rows (BK-aligned chunks)
PPO_API int ppo_wgrad_splits(long long R, int tiles, int target_blocks, int min_ktiles) {
  long long kt = (R + BK16 - 1) / BK16;
  long long z = target_blocks / (tiles > 0 ? tiles : 1);
  if (z < 1) z = 1;
  if (kt / z < min_ktiles) z = kt / min_ktiles;
  if (z < 1) z = 1;
  if (z > 4096) z = 4096;
  return (int)z;
}

// dW[n][k] = Σ_r dy[r][n] x[r][k]: slab [Z][N][K], slab_bias [Z][N]
PPO_API int ppo_linear_wgrad(const float* dy, const float* x, int R, int N, int K, int Z, float* slab,
                             float* slab_bias, void* stream) {
  PPO_REQUIRE(N % 4 == 0 && K % 4 == 0, "ppo_linear_wgrad: N=%d K=%d must be multiples of 4", N, K);
  // split path: the fc layer (N >= 128) whenever the split core is on (0.82 vs
  // 1.03 ms at the c3 minibatch); the narrow GRU/MLP layers only with x9 = 2
  if (use_x9_all() || (use_x9() && N >= 128)) {
    if (N <= 64) {
      DenseWgrad<XW64> p;
      set_wgrad(p, dy, N, R, Z, slab, slab_bias, K);
      p.x = x; p.K = K;
      return launch_x9(p, N, K, Z, as_stream(stream), "linear_wgrad", 2.0 * R * N * K);
    }
    // split at staging, 256 x 128 tiles: 0.727 vs 0.775 ms (in-loop split) at the c3 minibatch;
    // branch-free buffer loads where the operands fit 31-bit offsets; the k loop pipelined
    // (knob wgrad_pipe, igemm_x9.h): 0.610 -> 0.531 ms
    if ((long long)R * (N > K ? N : K) * 4 < 0x7fffffffLL) {
      DenseWgradB<SW256x128> p;
      set_wgrad(p, dy, N, R, Z, slab, slab_bias, K);
      p.x = x; p.K = K; p.n_fast = 0;
      p.vec = K % 4 == 0 && ((uintptr_t)slab & 15) == 0;
      return launch_x9(p, N, K, Z, as_stream(stream), "linear_wgrad", 2.0 * R * N * K);
    }
    DenseWgrad<SW256x128> p;
    set_wgrad(p, dy, N, R, Z, slab, slab_bias, K);
    p.x = x; p.K = K; p.n_fast = 0;
    p.vec = K % 4 == 0 && ((uintptr_t)slab & 15) == 0;
    return launch_x9(p, N, K, Z, as_stream(stream), "linear_wgrad", 2.0 * R * N * K);
  }
  DenseWgrad<CfgWfc> p;
  set_wgrad(p, dy, N, R, Z, slab, slab_bias, K);
  p.x = x; p.K = K;
  return launch(p, N, K, Z, as_stream(stream), "linear_wgrad", 2.0 * R * N * K);
}

// Σ over the Z split partials (fixed order) -> gw (torch order, see ColMap) and gb
PPO_API int ppo_wgrad_reduce(const float* slab, const float* slab_bias, int Z, int M, int NW, int kind, int a, int b,
                             float* gw, float* gb, float scale, int accumulate, void* stream) {
  PPO_REQUIRE(kind >= 0 && kind <= 3, "ppo_wgrad_reduce: kind=%d", kind);
  ProfScope prof("wgrad_reduce", as_stream(stream), 4.0 * (double)Z * M * (NW + 1) + 4.0 * M * (NW + 1));
  hipStream_t st = as_stream(stream);
  const long long cols = (long long)M * NW;
  int rc = colsum(slab, cols, Z, cols, ColMap{kind, a, b, NW}, gw, scale, accumulate, st);
  if (rc) return rc;
  return colsum(slab_bias, M, Z, M, ColMap{0, 0, 0, 1}, gb, 1.0f, accumulate, st);
}

// generic deterministic column sum (used for the heads' partials)
PPO_API int ppo_colsum(const float* src, long long ld, int rows, long long cols, float* out, float scale,
                       int accumulate, void* stream) {
  return colsum(src, ld, rows, cols, ColMap{0, 0, 0, 1}, out, scale, accumulate, as_stream(stream));
}
