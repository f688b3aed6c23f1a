// conv1 of the CNNBase trunk: forward, weight gradient and their launchers.
//
// Reference network: CNNBase (ppo-dash-study/001_baseline/ppo/model.py:169-199,
// = ppo-dash-training/.../a2c_ppo_acktr/model.py:169-199):
//   conv1 Conv2d(C,32,8,s4)+ReLU -> conv2 Conv2d(32,64,4,s2)+ReLU ->
//   conv3 Conv2d(64,32,3,s1)+ReLU -> Flatten -> Linear(1568,H)+ReLU
// The reference runs these as cuDNN/MKL calls plus autograd; here every pass is
// an implicit GEMM with the im2col gather folded into the operand staging, the
// bias + ReLU (forward) or ReLU-mask (dgrad) folded into the epilogue, and the
// minibatch row gather (feed_forward_generator `[indices]`, storage.py:143)
// folded into conv1's loads — no im2col or gathered-obs buffer ever exists.
// conv2.hip, conv3.hip and dense.hip hold the other layers, trunk.hip the
// rollout's three forwards in one launch.
//
// Activation layout in HBM: NHWC fp32 ([B][H][W][C]), so an im2col row's k
// index (ky, kx, ci) reads 16 contiguous bytes per float4.  The observation is
// the storage's u8 NCHW plane.  Weights are re-packed once per optimizer step
// (ppo_pack_weights, dense.hip) into the k orders the kernels use, each segment
// followed by its bf16 split planes; gradients are written back in torch order.
//
// Production path (u8 observations, C = 4): image-resident kernels on the bf16
// matrix cores, v_mfma_f32_16x16x32_bf16 over exact bf16 splits.
// A pixel 0..255 is exact in bf16 and W = W_hi + W_mid + W_lo exactly, so every
// product is exact in fp32 and the MFMA accumulates in fp32: the forward is
// conv1_fwd_bf16x3_body (conv1_fwd_body.h), the weight gradient the k-split
// kernels of conv1w.hip or conv1_wgrad_parts_kernel below.  Float observations
// take conv1f.hip, raw RGB frames conv1f.hip / rgbaff.hip.  Any other channel
// count, and conv1_fwd tune 9, take the generic fp32-MFMA tile GEMM of igemm.h
// with the Conv1Fwd / Conv1Wgrad problems below (im2col and the u8 / 255 decode
// in the operand loaders).
#include "conv_launch.h"
#include "conv1_fwd_body.h"
#include "conv1_paths.h"

namespace {
// conv1 forward as a tile-GEMM problem: 8x8 stride 4 over the u8/f32 NCHW observation, k = (c, ky, kx) (torch order)
template <typename InT, class C_>
struct Conv1Fwd : C_ {
  using BCtx = typename C_::BCtx;
  const InT* obs; const int64_t* idx; long long row0; int C, M;
  const float* w; const float* bias; float* out;
  struct ACtx { const InT* base; bool ok; };
  __device__ ACtx a_ctx(int m, int) const {
    if (m >= M) return {obs, false};
    const int b = m / 400, pp = m - b * 400, oy = pp / 20, ox = pp - oy * 20;
    return {obs + obs_row(idx, row0, b) * (long long)(C * IMG2) + (oy * 4) * IMG + ox * 4, true};
  }
  using Raw = std::conditional_t<sizeof(InT) == 1, uint32_t, f32x4>;
  __device__ Raw a_load(const ACtx& c, int k) const {
    if (!c.ok) return Raw{};
    const int ch = k >> 6, ky = (k >> 3) & 7, kx = k & 7;
    return *reinterpret_cast<const Raw*>(c.base + ch * IMG2 + ky * IMG + kx);
  }
  __device__ BCtx b_ctx(int n, int) const { return {w + n * (C * 64), 0, n < 32}; }
  __device__ f32x4 b_load(const BCtx& c, int k) const {
    return c.ok ? *reinterpret_cast<const f32x4*>(c.p + k) : zero4();
  }
  __device__ void k_range(int, int& b, int& e) const { b = 0; e = C * 64; }
  __device__ void store(int m, int n, int, float v) const {
    if constexpr (sizeof(InT) == 1) v *= (1.0f / 255.0f);
    if (m < M) out[(size_t)m * 32 + n] = fmaxf(v + bias[n], 0.f);
  }
};

template <int C, bool MASK, int NPW = 3>
__global__ __launch_bounds__(512) void conv1_fwd_bf16x3_kernel(const uint8_t* __restrict__ obs,
                                                               const int64_t* __restrict__ idx, long long row0,
                                                               int B, const float* __restrict__ w,
                                                               const float* __restrict__ bias,
                                                               float* __restrict__ out,
                                                               uint16_t* __restrict__ mbits) {
  __shared__ __attribute__((aligned(16))) uint16_t img[2][C * C1S];
  conv1_fwd_bf16x3_body<C, MASK, NPW>(obs, idx, row0, B, w, bias, out, mbits, img);
}

// conv1 weight gradient on the bf16 matrix cores, exact, part-pipelined
// (ppo_tune_set("conv1_wgrad", 5), and the half-precision mode's): dW[co][(c,ky,kx)] = Σ_px dz1[px][co] ·
// u[c][4oy+ky][4ox+kx]; the u8 pixels are exact in bf16 and dz = hi + mid + lo
// exactly, so three v_mfma_f32_32x32x16_bf16 per block pair give exact products
// with fp32 accumulation.  Staged so that the staging overlaps
// the MFMAs (a whole-image-stage kernel that filled the LDS measured 2.03-2.10
// ms per minibatch against 1.92-2.01 for this one and was removed):
//   * an image is processed in 5 parts of 4 output rows (80 pixels = 5 k-steps);
//     a part's operands are 42,496 B of LDS — two stages (85 KB) instead of one
//     whole-image stage that fills the LDS;
//       E   [c][20 rows][40 quad slots][4 px] bf16: row yr = input row 16p + yr,
//           slot Q*8 + kx holds u[c][y][16Q + 4j + kx], j = 0..3 (the 4 pixels of
//           an output-row quad for one kx); slot kx bits XOR ((item >> 1) & 7),
//           item = row * 5 + Q, so the staging ds_write_b64 of 16 consecutive
//           items and the B-fragment ds_read_b64 of 32 lanes (4 ky x 8 kx) are
//           both conflict-free
//       dzP [3 planes][32 co][88] bf16: dz of the part split once (no per-wave
//           re-split), 176-B rows: conflict-free ds_read_b128 A fragments
//   * wave w owns one 32-column tile (c = w >> 1, ky = 4 (w & 1) + .., all kx)
//     for every k-step: no k-group partials to combine;
//   * staggered: waves 0-3 stage part i+1 then compute part i, waves 4-7 the
//     other way round, so each SIMD pairs one staging (VALU) wave with one
//     computing (MFMA) wave; the loads of part i+2 are in flight meanwhile.
// One barrier per part.  Output: the split-K slab [Z][32][256] (u8 integers: the
// reduce applies 1/255) and bias partials [Z][32], as the other variants.
// NW = 16 (ppo_tune_set("conv1_wgrad", 4)): four waves per SIMD.  Waves w and
// w + 8 share column tile w & 7 and split the k-steps by parity (wave w + 8 the
// odd global k-steps), their accumulators summed in a fixed order at the end;
// every wave stages at most one item (E items on waves 0-6, dz items on waves
// 8-12), so per SIMD two waves stage while two compute (waves 4-7 and 12-15
// compute first).
// TPW = 2 (NW = 16, ppo_tune_set("conv1_wgrad", 5)): each wave computes two
// column tiles (2 (w & 3), +1) per A fragment read, k-steps split four ways
// (k-group w >> 2 takes global k-steps ≡ w >> 2 mod 4): the dz fragments, the
// same for every tile, are read from LDS half as often (the kernel is LDS-bound:
// the staging writes and the fragment reads share the LDS with each other).
template <int NPD = 3, int NW = 8, int TPW = 1>   // NPD: dz parts summed (3 exact; 1 half-precision mode)
__global__ __launch_bounds__(NW * 64) void conv1_wgrad_parts_kernel(const float* __restrict__ dz1,
                                                                const uint8_t* __restrict__ obs,
                                                                const int64_t* __restrict__ idx, long long row0,
                                                                int B, float* __restrict__ slab,
                                                                float* __restrict__ slab_bias, int dbg) {
  // timing anatomy only (kbench --tune stagger=16*dbg; wrong results): 1 skips the
  // MFMAs, 2 the staging (put), 4 the DMAs, 8 the stagger
  const bool no_mma = dbg & 1, no_put = dbg & 2, no_dma = dbg & 4;
  constexpr int C = 4, NPART = 5, ER = 20, SLOTS = 40, DZS = 88, MAXIMG = 512;
  constexpr int E_BF = C * ER * SLOTS * 4, DZ_BF = 32 * DZS, STG = E_BF + 3 * DZ_BF;   // bf16 elements
  // raw part, as 16-B LDS-DMA pieces: the 4 channels' 20 input rows (4 x 1,680 B =
  // 420 pieces, 16-B aligned in the u8 storage row; 7 wave-instructions, padded to
  // 448) then dz of the part's 80 pixels (10,240 B contiguous = 640 pieces)
  constexpr int EPC = 105, EPIECE = 448, DPIECE = 640, RAWP = EPIECE + DPIECE;
  __shared__ __attribute__((aligned(16))) uint16_t L[2 * STG];           // 84,992 B: two part stages
  __shared__ __attribute__((aligned(16))) uint4 RAW[3][RAWP];            // 52,224 B: raw parts, 3-slot ring
  __shared__ long long rowtab[MAXIMG];                                    // storage row of the block's images
  __shared__ float bred[320];
  static_assert(NW == 8 || NW == 16, "8 or 16 waves");
  static_assert(TPW == 1 || (TPW == 2 && NW == 16), "two tiles per wave with 16 waves");
  constexpr int NT = NW * 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l32 = lane & 31, h = lane >> 5;
  // column tile(s) tile + t (t < TPW); TPW 1: k-step parity kh (NW = 16); TPW 2: k-group kh (0-3)
  const int tile = TPW == 2 ? 2 * (wave & 3) : wave & 7, kh = TPW == 2 ? wave >> 2 : wave >> 3;
  const int G = gridDim.x;
  const int nimg = blockIdx.x < B ? (B - 1 - (int)blockIdx.x) / G + 1 : 0, nit = NPART * nimg;
  for (int k = tid; k < nimg; k += NT) rowtab[k] = obs_row(idx, row0, (int)blockIdx.x + k * G);
  // B column of this lane: n = 32 (tile + t) + l32 -> (c, ky, kx)
  int qoff[TPW][5][2];   // E element offset of the lane's quads for local k-step ls
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const int tt = tile + t, bc = tt >> 1, bky = 4 * (tt & 1) + (l32 >> 3), bkx = l32 & 7;
#pragma unroll
    for (int ls = 0; ls < 5; ++ls)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int ql = 4 * ls + 2 * h + j, oyl = ql / 5, Q = ql - 5 * oyl;
        const int r = bc * ER + 4 * oyl + bky, item = r * 5 + Q;
        qoff[t][ls][j] = (r * SLOTS + Q * 8 + (bkx ^ ((item >> 1) & 7))) * 4;
      }
  }
  const int aoff = E_BF + l32 * DZS + 8 * h;   // + plane * DZ_BF + 16 ls
  // staging items: E item tid < 400 (row r = tid / 5 = c * 20 + yr, quad Q = tid % 5);
  // dz item tid < 320 (co = tid & 31, pixel octet oc = tid >> 5).  Threads without
  // an item DMA item 0's addresses (harmless duplicates) so every wave issues the
  // same DMA count.
  const bool e_on = tid < 400, d_on = NW == 8 ? tid < 320 : tid >= 512 && tid < 832;
  const int eit = e_on ? tid : 0, dit = d_on ? tid - (NW == 8 ? 0 : 512) : 0;
  const int er = eit / 5, eQ = eit - 5 * er, ec = er / ER, eyr = er - ER * ec, ef = (eit >> 1) & 7;
  const int dco = dit & 31, doc = dit >> 5;
  float bacc = 0.f;
  // DMA of item j's raw part into RAW[j & 1]: wave w moves pieces 64 w + lane of
  // the image rows (waves 0-6) and of dz (pieces 64 (w + 8 i) + lane, i = 0, 1)
  auto dma = [&](int j) {
    if (no_dma) return;
    const int jj = j < nit ? j : nit - 1, k = jj / NPART, p = jj - NPART * k, b = (int)blockIdx.x + k * G;
    uint4* dst = RAW[jj % 3];
    if (wave < 7) {
      const int piece = min(64 * wave + lane, C * EPC - 1), c = piece / EPC, r = piece - EPC * c;
      const uint8_t* src = obs + rowtab[k] * (long long)(C * IMG2) + c * IMG2 + p * (16 * IMG) + 16 * r;
      __builtin_amdgcn_global_load_lds(reinterpret_cast<const void*>(src),
                                       reinterpret_cast<__attribute__((address_space(3))) void*>(
                                           reinterpret_cast<uintptr_t>(dst + 64 * wave)), 16, 0, 0);
    }
    const char* dsrc = reinterpret_cast<const char*>(dz1 + (size_t)b * 12800 + p * 80 * 32);
#pragma unroll
    for (int i = 0; i < (NW == 8 ? 2 : 1); ++i) {
      const int blk = NW == 8 ? wave + 8 * i : wave - 6;   // wave-uniform; NW = 16: waves 6-15
      if (blk >= 0 && blk < DPIECE / 64)
        __builtin_amdgcn_global_load_lds(reinterpret_cast<const void*>(dsrc + 16 * (64 * blk + lane)),
                                         reinterpret_cast<__attribute__((address_space(3))) void*>(
                                             reinterpret_cast<uintptr_t>(dst + EPIECE + 64 * blk)), 16, 0, 0);
    }
  };
  auto put = [&](int j, int st) {   // item j: RAW[j % 3] -> stage st
    if (no_put) return;
    const uint32_t* R = reinterpret_cast<const uint32_t*>(RAW[j % 3]);
    uint32_t ew[5];
    float dv[8];
    if (NW == 8 || e_on) {   // NW = 8: every thread reads both (all loads issued first)
#pragma unroll
      for (int q = 0; q < 5; ++q) ew[q] = R[(ec * 1680 + eyr * IMG + 16 * eQ) / 4 + q];
    }
    if (NW == 8 || d_on) {
#pragma unroll
      for (int q = 0; q < 8; ++q) dv[q] = __uint_as_float(R[4 * EPIECE + (8 * doc + q) * 32 + dco]);
    }
    uint16_t* S = L + st * STG;
    if (e_on) {
#pragma unroll
      for (int kx = 0; kx < 8; ++kx) {   // u[16Q + 4i + kx] = byte (kx & 3) of dword i + (kx >> 2)
        const int o = kx >> 2, sh = 8 * (kx & 3);
        float f[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) f[i] = (float)((ew[i + o] >> sh) & 255u);
        const uint2 q = {__builtin_amdgcn_perm(__float_as_uint(f[1]), __float_as_uint(f[0]), 0x07060302u),
                         __builtin_amdgcn_perm(__float_as_uint(f[3]), __float_as_uint(f[2]), 0x07060302u)};
        *reinterpret_cast<uint2*>(S + (er * SLOTS + eQ * 8 + (kx ^ ef)) * 4) = q;
      }
    }
    if (d_on) {
      Frag3 fr;
      split8(f32x4{dv[0], dv[1], dv[2], dv[3]}, f32x4{dv[4], dv[5], dv[6], dv[7]}, fr, NPD == 1);
      uint16_t* d = S + E_BF + dco * DZS + 8 * doc;
      *reinterpret_cast<bf16x8*>(d) = fr.h;
      if constexpr (NPD == 3) {
        *reinterpret_cast<bf16x8*>(d + DZ_BF) = fr.m;
        *reinterpret_cast<bf16x8*>(d + 2 * DZ_BF) = fr.l;
      }
      bacc += ((dv[0] + dv[1]) + (dv[2] + dv[3])) + ((dv[4] + dv[5]) + (dv[6] + dv[7]));
    }
  };
  f32x16 acc[TPW];
#pragma unroll
  for (int t = 0; t < TPW; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  auto compute = [&](int st, int i) {
    if (no_mma) return;
    const uint16_t* S = L + st * STG;
#pragma unroll
    for (int ls = 0; ls < 5; ++ls) {   // global k-step 5 i + ls; the skips are wave-uniform
      if (TPW == 2 && ((i + ls) & 3) != kh) continue;
      if (TPW == 1 && NW == 16 && ((i + ls) & 1) != kh) continue;
      bf16x8 bq[TPW];
#pragma unroll
      for (int t = 0; t < TPW; ++t) {
        const uint2 q1 = *reinterpret_cast<const uint2*>(S + qoff[t][ls][0]);
        const uint2 q2 = *reinterpret_cast<const uint2*>(S + qoff[t][ls][1]);
        bq[t] = __builtin_bit_cast(bf16x8, uint4{q1.x, q1.y, q2.x, q2.y});
      }
      const uint16_t* A = S + aoff + 16 * ls;
      if constexpr (NPD == 3) {
        const bf16x8 al = *reinterpret_cast<const bf16x8*>(A + 2 * DZ_BF), am = *reinterpret_cast<const bf16x8*>(A + DZ_BF);
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bq[t], acc[t], 0, 0, 0);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bq[t], acc[t], 0, 0, 0);
        }
      }
      const bf16x8 ah = *reinterpret_cast<const bf16x8*>(A);
#pragma unroll
      for (int t = 0; t < TPW; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bq[t], acc[t], 0, 0, 0);
    }
  };
  // pipeline: item j's pieces are DMA'd into RAW[j % 3] at item j - 3 (by every
  // wave, a share each); at the end of item j - 2 every wave waits for its own
  // share (vmcnt = one item's DMA count: item j + 1's may stay in flight) and the
  // barrier publishes the slot; item j - 1 stages it (put) into LDS stage j & 1.
  const int nops = NW == 8 ? (wave < 7 ? 1 : 0) + 1 + (wave + 8 < DPIECE / 64 ? 1 : 0)
                            : (wave < 7 ? 1 : 0) + (wave >= 6 ? 1 : 0);
  auto wait_raw = [&]() {   // all but the youngest item's DMAs retired
    if (nops == 3) __builtin_amdgcn_s_waitcnt(0x0F73);        // vmcnt(3)
    else if (nops == 2) __builtin_amdgcn_s_waitcnt(0x0F72);   // vmcnt(2)
    else __builtin_amdgcn_s_waitcnt(0x0F71);                  // vmcnt(1)
  };
  // block barrier that does not drain the in-flight DMAs (__syncthreads' release
  // fence would wait for them: vmcnt(0)); LDS stores are retired by lgkmcnt(0),
  // and the memory clobber keeps the compiler from moving LDS accesses across it
  auto part_barrier = [&]() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };
  __syncthreads();   // rowtab
  if (nit > 0) {
    dma(0);
    dma(1);
    dma(2);
    if (nops == 3) __builtin_amdgcn_s_waitcnt(0x0F76);        // vmcnt(6): item 0 retired
    else if (nops == 2) __builtin_amdgcn_s_waitcnt(0x0F74);   // vmcnt(4)
    else __builtin_amdgcn_s_waitcnt(0x0F72);                  // vmcnt(2)
    part_barrier();
    put(0, 0);
    wait_raw();   // item 1 retired (item 2 may be in flight)
  }
  part_barrier();
  const bool late = (NW == 8 ? wave >= 4 : ((wave >> 2) & 1) != 0) && !(dbg & 8);
  for (int i = 0; i < nit; ++i) {
    const int st = i & 1;
    const bool more = i + 1 < nit;
    if (!late && more) put(i + 1, st ^ 1);
    if (more) dma(i + 3);   // into RAW[i % 3]: item i was staged before the last barrier
    compute(st, i);
    if (late && more) put(i + 1, st ^ 1);
    wait_raw();   // item i + 2 retired (item i + 3 may be in flight)
    part_barrier();
  }
  __builtin_amdgcn_s_waitcnt(0x0F70);   // drain the clamped tail DMAs before the block exits
  float* X = reinterpret_cast<float*>(L);   // stage space, free now: k-group partials
  if constexpr (NW == 16 && TPW == 1) {   // odd-k-step partials added to the even ones
    if (kh) {
#pragma unroll
      for (int r = 0; r < 16; ++r) X[(r * 8 + tile) * 64 + lane] = acc[0][r];
    }
    __syncthreads();
    if (!kh) {
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[0][r] += X[(r * 8 + tile) * 64 + lane];
    }
  }
  if constexpr (TPW == 2) {   // fixed order: (k0 + k2) + (k1 + k3); slot = tile pair (+ 4)
    auto xo = [&](int slot, int t, int r) { return ((slot * 2 + t) * 16 + r) * 64 + lane; };
    const int tp = wave & 3;
    if (kh >= 2) {
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) X[xo((kh - 2) * 4 + tp, t, r)] = acc[t][r];
    }
    __syncthreads();
    if (kh < 2) {
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] += X[xo(kh * 4 + tp, t, r)];
    }
    __syncthreads();
    if (kh == 1) {
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) X[xo(tp, t, r)] = acc[t][r];
    }
    __syncthreads();
    if (kh == 0) {
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] += X[xo(tp, t, r)];
    }
  }
  float* out = slab + (size_t)blockIdx.x * 32 * 256;
  if (kh == 0) {
#pragma unroll
    for (int t = 0; t < TPW; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = (r & 3) + 8 * (r >> 2) + 4 * h, n = 32 * (tile + t) + l32;
        out[co * 256 + n] = acc[t][r];
      }
  }
  if (d_on) bred[dit] = bacc;
  __syncthreads();
  if (tid < 32) {   // channel tid: its 10 pixel octets, fixed order
    float t = 0.f;
#pragma unroll
    for (int o = 0; o < 10; ++o) t += bred[32 * o + tid];
    slab_bias[(size_t)blockIdx.x * 32 + tid] = t;
  }
}

// ReLU mask bits of a conv1 output [B][400][32]: bit c of word p = (a1[p][c] > 0),
// for the conv1 paths without the fused epilogue (one thread per half pixel).
__global__ __launch_bounds__(256) void relu_bits_kernel(const float* __restrict__ a1, long long halves,
                                                        uint16_t* __restrict__ mbits) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < halves; i += (long long)gridDim.x * 256) {
    const f32x4* p = reinterpret_cast<const f32x4*>(a1 + 16 * i);
    uint32_t m = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 v = p[q];
#pragma unroll
      for (int e = 0; e < 4; ++e) m |= (v[e] > 0.f ? 1u : 0u) << (4 * q + e);
    }
    mbits[i] = (uint16_t)m;
  }
}

// conv1 weight gradient as a tile-GEMM problem (WgradBase, igemm.h): dW[co][kk] =
// Σ_r dz[r][co] · X(r, kk) over the reduction r = (b, output pixel), split over
// blockIdx.z into fp32 partial slabs (deterministic sum in ppo_wgrad_reduce).  Both
// operands are row-contiguous tiles; blocks of tile column 0 also sum the dz tile
// into the bias partial (db[co] = Σ_r dz[r][co]).  X(r, kk) = decoded obs[idx[b]][c][4oy+ky][4ox+kx], kk = (c,ky,kx)
// A k-tile (BK rows, BK | 400, chunks BK-aligned) never straddles two images,
// so the image (and its minibatch row gather) is resolved once per tile from
// the block-uniform tile start — a scalar load, not one per operand load.
template <typename InT, class C_>
struct Conv1Wgrad : WgradBase<C_> {
  static_assert(400 % C_::BK == 0, "conv1 wgrad k-tiles must not straddle images");
  static constexpr bool B_TILE = true;
  const InT* obs; const int64_t* idx; long long row0; int C;
  struct BCtx { int off; bool ok; };
  struct TCtx { const InT* img; int r0; };
  using Raw = std::conditional_t<sizeof(InT) == 1, uint32_t, f32x4>;
  __device__ BCtx b_ctx(int n, int) const {
    const int ch = n >> 6, ky = (n >> 3) & 7, kx = n & 7;
    return {ch * IMG2 + ky * IMG + kx, n < C * 64};
  }
  __device__ TCtx tile(int k0) const {
    const int b = k0 / 400;
    return {obs + obs_row(idx, row0, b) * (long long)(C * IMG2), b * 400};
  }
  __device__ Raw b_load_t(const BCtx& c, const TCtx& t, int r) const {
    if (!c.ok || r >= this->R) return Raw{};
    const int pp = r - t.r0, oy = pp / 20, ox = pp - oy * 20;
    return *reinterpret_cast<const Raw*>(t.img + (oy * 4) * IMG + ox * 4 + c.off);
  }
};

// fp32-MFMA tiles of the generic problems: the measured best of the round-1 sweep
// (profiles/r01_kbench_sweep_v2.log) for N = 32
using V32_0 = Cfg<256, 32, 4, 1, true, true>;           // 4 waves x 64 rows, 46 KB LDS
using CfgW32 = Cfg<32, 256, 1, 4, false, false, true>;

}  // namespace

static int conv1_fwd_impl(const void* obs, int obs_is_u8, const int64_t* idx, long long row0, int C, int B,
                          const float* w1, const float* b1, float* out, uint16_t* mbits, void* stream) {
  PPO_REQUIRE(B >= 0 && C > 0, "ppo_conv1_fwd: B=%d C=%d", B, C);
  // small.hip's kernel combines at most 8 channel partials per output: more channels (four
  // stacked RGB frames: C = 12) take the tile GEMM below at every batch size
  if (!mbits && B > 0 && B <= tune_small_b() && C <= 8)
    return small_conv1_fwd(obs, obs_is_u8, idx, row0, C, B, w1, b1, out, as_stream(stream));
  // float observations (the reference's fp32 storage plane): the image-resident
  // split-bf16 kernel of conv1f.hip
  if (!obs_is_u8 && C == 4 && ((uintptr_t)obs & 15) == 0)
    return ppo_conv1_fwd_f32((const float*)obs, idx, row0, B, w1, b1, out, reinterpret_cast<uint32_t*>(mbits), stream);
  const bool img = obs_is_u8 && C == 4 && tune_key(TK_CONV1_FWD) == 0;
  if (mbits && !img) {
    // the generic path has no fused mask epilogue: the conv, then the mask from its output
    const int rc = conv1_fwd_impl(obs, obs_is_u8, idx, row0, C, B, w1, b1, out, nullptr, stream);
    if (rc != 0 || B == 0) return rc;
    const long long halves = (long long)B * 800;
    const long long nb = (halves + 255) / 256;
    relu_bits_kernel<<<(unsigned)(nb < 8192 ? nb : 8192), 256, 0, as_stream(stream)>>>(out, halves, mbits);
    PPO_LAUNCH_CHECK("relu_bits_kernel");
    return 0;
  }
  const long long M = (long long)B * 400;
  const double fl = 2.0 * M * 32 * C * 64;
  if (img) {
    if (B == 0) return 0;
    const unsigned nb = img_grid(B);
    int slot;
    const bool prof = ppo_prof_begin("conv1_fwd_u8", as_stream(stream), &slot);
    const uint8_t* o8 = (const uint8_t*)obs;
    hipStream_t st = as_stream(stream);
    if (tune_products() == 1) {   // half-precision mode: bf16 weights
      if (mbits) conv1_fwd_bf16x3_kernel<4, true, 1><<<nb, 512, 0, st>>>(o8, idx, row0, B, w1, b1, out, mbits);
      else conv1_fwd_bf16x3_kernel<4, false, 1><<<nb, 512, 0, st>>>(o8, idx, row0, B, w1, b1, out, nullptr);
    } else if (mbits) {
      conv1_fwd_bf16x3_kernel<4, true><<<nb, 512, 0, st>>>(o8, idx, row0, B, w1, b1, out, mbits);
    } else {
      conv1_fwd_bf16x3_kernel<4, false><<<nb, 512, 0, st>>>(o8, idx, row0, B, w1, b1, out, nullptr);
    }
    if (prof) ppo_prof_end(slot, st, fl);
    PPO_LAUNCH_CHECK("conv1_fwd_u8 (image-resident)");
    return 0;
  }
#define SETUP1(T_)                                                                                 \
  p.obs = (const T_*)obs; p.idx = idx; p.row0 = row0; p.C = C; p.M = (int)M; p.w = w1; p.bias = b1; p.out = out
  if (obs_is_u8) {
    Conv1Fwd<uint8_t, V32_0> p;
    SETUP1(uint8_t);
    return launch(p, M, 32, 1, as_stream(stream), "conv1_fwd_u8", fl);
  }
  Conv1Fwd<float, V32_0> p;
  SETUP1(float);
  return launch(p, M, 32, 1, as_stream(stream), "conv1_fwd_f32", fl);
#undef SETUP1
}

// conv1 forward: out [B][20][20][32] = relu(conv(obs rows, W1 torch layout) + b1)
PPO_API int ppo_conv1_fwd(const void* obs, int obs_is_u8, const int64_t* idx, long long row0, int C, int B,
                          const float* w1, const float* b1, float* out, void* stream) {
  return conv1_fwd_impl(obs, obs_is_u8, idx, row0, C, B, w1, b1, out, nullptr, stream);
}

// conv1 forward that also writes the ReLU mask of its output as bits
// (mbits [B][400] u32, bit c of pixel p = out[p][c] > 0) for ppo_conv2_dgrad_bits.
PPO_API int ppo_conv1_fwd_mask(const void* obs, int obs_is_u8, const int64_t* idx, long long row0, int C, int B,
                               const float* w1, const float* b1, float* out, uint32_t* mbits, void* stream) {
  PPO_REQUIRE(mbits != nullptr, "ppo_conv1_fwd_mask: null mask");
  return conv1_fwd_impl(obs, obs_is_u8, idx, row0, C, B, w1, b1, out, reinterpret_cast<uint16_t*>(mbits), stream);
}

// conv1 wgrad partials: slab [Z][32][C*64], slab_bias [Z][32]
PPO_API int ppo_conv1_wgrad(const float* dz1, const void* obs, int obs_is_u8, const int64_t* idx, long long row0,
                            int C, int B, int Z, float* slab, float* slab_bias, void* stream) {
  const long long R = (long long)B * 400;
  PPO_REQUIRE(R < 0x7fffffffLL, "ppo_conv1_wgrad: B too large");
  if (B <= 0 || Z <= 0) return 0;   // every path: an empty launch writes nothing (the tile GEMM wrote zero slabs)
  const double fl = 2.0 * R * 32 * C * 64;
  // u8 rows, C = 4: the k-split kernels (conv1w.hip, tunes 8-10, fp32 dz) or the
  // part-pipelined kernel (tune 5; the half-precision mode's, bf16 dz)
  const int kw = tune_key(TK_CONV1_WGRAD), np = tune_products();
  if (obs_is_u8 && C == 4 && (kw == 5 || np == 1)) {
    if (B <= 0 || Z <= 0) return 0;
    PPO_REQUIRE((B + Z - 1) / Z <= 512, "ppo_conv1_wgrad: %d images over %d blocks (at most 512 per block)", B, Z);
    int slot;
    const bool prof = ppo_prof_begin("conv1_wgrad_u8", as_stream(stream), &slot);
    if (np == 1)
      conv1_wgrad_parts_kernel<1, 16, 2><<<Z, 1024, 0, as_stream(stream)>>>(dz1, (const uint8_t*)obs, idx, row0, B,
                                                                            slab, slab_bias, 0);
    else
      conv1_wgrad_parts_kernel<3, 16, 2><<<Z, 1024, 0, as_stream(stream)>>>(dz1, (const uint8_t*)obs, idx, row0, B,
                                                                            slab, slab_bias, tune_stagger() >> 4);
    if (prof) ppo_prof_end(slot, as_stream(stream), fl);
    PPO_LAUNCH_CHECK("conv1_wgrad_parts_kernel");
    return 0;
  }
  if (obs_is_u8 && C == 4)
    return kw >= 9
               ? conv1_wgrad_kw3(dz1, (const uint8_t*)obs, idx, row0, B, Z, slab, slab_bias, stream, kw == 10 ? 8 : 4)
               : conv1_wgrad_kw(dz1, (const uint8_t*)obs, idx, row0, B, Z, slab, slab_bias, stream);
  if (!obs_is_u8 && C == 4 && ((uintptr_t)obs & 15) == 0)   // conv1f.hip
    return ppo_conv1_wgrad_f32(dz1, (const float*)obs, idx, row0, B, Z, slab, slab_bias, stream);
  if (obs_is_u8) {   // any other channel count: the generic fp32-MFMA tile GEMM
    Conv1Wgrad<uint8_t, CfgW32> p;
    set_wgrad(p, dz1, 32, R, Z, slab, slab_bias, C * 64);
    p.obs = (const uint8_t*)obs; p.idx = idx; p.row0 = row0; p.C = C;
    return launch(p, 32, C * 64, Z, as_stream(stream), "conv1_wgrad_u8", fl);
  }
  Conv1Wgrad<float, CfgW32> p;
  set_wgrad(p, dz1, 32, R, Z, slab, slab_bias, C * 64);
  p.obs = (const float*)obs; p.idx = idx; p.row0 = row0; p.C = C;
  return launch(p, 32, C * 64, Z, as_stream(stream), "conv1_wgrad_f32", fl);
}
