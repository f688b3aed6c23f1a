// conv2 of the CNNBase trunk (conv1.hip's header has the network and the layouts):
// image-resident kernels on the bf16 matrix cores (exact split) —
// forward (its body in conv2_fwd_body.h), weight gradient and input gradient (the
// epilogue applies the ReLU mask of the layer below, threshold_backward: pass where
// the saved output is > 0) — and their launchers.
#include "conv_launch.h"
#include "conv2_fwd_body.h"

namespace {

// standalone conv2 forward: five row tiles here, the lone pixel in conv2_fwd_lone_kernel
template <int NP, bool MASK = false>
__global__ __launch_bounds__(512) void conv2_fwd_x9c_kernel(const float* __restrict__ a1, int B,
                                                           const uint16_t* __restrict__ wpl,
                                                           const float* __restrict__ bias,
                                                           float* __restrict__ out,
                                                           uint16_t* __restrict__ mbits) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[C2F_LDS];
  conv2_fwd_x9c_body<NP, MASK>(a1, B, wpl, bias, out, mbits, lds);
}

template <int NP, bool MASK>
__global__ __launch_bounds__(512) void conv2_fwd_lone_kernel(const float* __restrict__ a1, int B,
                                                             const uint16_t* __restrict__ wpl,
                                                             const float* __restrict__ bias,
                                                             float* __restrict__ out,
                                                             uint16_t* __restrict__ mbits) {
  constexpr int KS = 8, WN = 64 * 512;
  __shared__ __attribute__((aligned(16))) uint8_t lds[C2L_LDS];
  const int tid = threadIdx.x, i16 = tid & 15, g = (tid & 63) >> 4, wave = tid >> 6;
  const int co = 16 * (wave & 3) + i16, kh = wave >> 2;
  bf16x8 bw[KS][3];
#pragma unroll
  for (int s = 0; s < KS; ++s)
#pragma unroll
    for (int p = 0; p < 3; ++p)
      bw[s][p] = *reinterpret_cast<const bf16x8*>(wpl + (size_t)p * WN + co * 512 + (8 * kh + s) * 32 + 8 * g);
  conv2_lone_tiles<NP, MASK>(a1, bw, bias, out, mbits, lds, 0, 1, B, blockIdx.x, gridDim.x);
}

// conv2 weight gradient, image-resident on the bf16 matrix cores (exact split,
// DESIGN.md §3): dW2[co][k] = Σ_pixels dz2[m][co] · a1[2oy+ky][2ox+kx][ci],
// k = (ky, kx, ci); per image a 64 x 512 x 81 product (reduction padded to 96 =
// 3 k-steps of 32), accumulated in registers over the block's images and
// written once as the block's split-K partial (slab [Z][64][512], bias
// partials [Z][64]; ppo_wgrad_reduce sums the Z partials in a fixed order).
// Per image the LDS holds, split into bf16 planes (the next image in flight in
// registers, stored between compute phases):
//   X  [3][400 px][32 ci]  a1, pixels in parity order Q = 20 y + 10 (x & 1) + (x >> 1)
//                          (76,800 B): the B fragment (8 reduction slots x 16 ci of
//                          one tap) comes from two ds_read_b64_tr_b16 per plane —
//                          4 pixel rows each, gathered by per-lane row addresses;
//                          8-B unit u of pixel Q at u ^ 4 ((Q >> 3) & 1)
//   D  [3][64 co][112]     dz2 transposed to [co][reduction slot] (43,008 B; rows of
//                          14 16-B units: conflict-free ds_read_b128 A fragments)
// Reduction slot r -> pixel: the 72 pixels with ox < 8 oy-major, then the ox = 8
// column (no 4-slot tr group straddles an output row; fewer bank conflicts);
// slots 81..95 have dz = 0 and read pixel 80's finite a1.
// Wave w: k columns 64 w .. +63 (taps 2w, 2w+1, both ci halves) x all 64 co:
// 16 accumulator tiles (64 VGPRs).
__device__ __forceinline__ int c2w_pix(int r) {
  r = r < 80 ? r : 80;
  return r < 72 ? (r >> 3) * 9 + (r & 7) : (r - 72) * 9 + 8;
}

template <int NP>
__global__ __launch_bounds__(512) void conv2_wgrad_x9_kernel(const float* __restrict__ dz2,
                                                            const float* __restrict__ a1, int B,
                                                            float* __restrict__ slab,
                                                            float* __restrict__ slab_bias) {
  constexpr int XPL = 400 * 32, DR = 112, DPL = 64 * DR;
  constexpr int XU = 1600, XPER = (XU + 511) / 512, DU = 64 * 12, DPER = (DU + 511) / 512;
  __shared__ __attribute__((aligned(16))) uint16_t X[3 * XPL];
  __shared__ __attribute__((aligned(16))) uint16_t D[3 * DPL];
  __shared__ float bred[512];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i16 = lane & 15, g = lane >> 4;
  const int q = i16 >> 2, p = i16 & 3;
  // tap-(0,0) pixel (parity order) of the row this lane addresses in the tr
  // reads of k-step s, half h: Q = Qb + 20 ky + 10 (kx & 1) + (kx >> 1)
  int Qb[3][2];
#pragma unroll
  for (int s = 0; s < 3; ++s)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int m = c2w_pix(32 * s + 8 * g + 4 * h + q), oy = m / 9;
      Qb[s][h] = 40 * oy + (m - 9 * oy);
    }
  // staging maps: X unit u -> (pixel Q = u >> 2, 16-B chunk c = u & 3); D unit
  // v -> (co = v & 63, slots 8 (v >> 6) .. +7)
  int xsrc[XPER], xdst[XPER];
#pragma unroll
  for (int j = 0; j < XPER; ++j) {
    const int u = tid + 512 * j, Q = u >> 2, c = u & 3, y = Q / 20, rem = Q - 20 * y;
    const int x = rem < 10 ? 2 * rem : 2 * (rem - 10) + 1;
    xsrc[j] = (y * 20 + x) * 32 + 8 * c;
    xdst[j] = Q * 32 + 8 * (c ^ (((Q >> 3) & 1) * 2));
  }
  f32x4 xs[XPER][2];
  float ds[DPER][8];
  float bsum = 0.f;   // bias partial of co = tid & 63 (fixed for this thread's D units)
  // the next image's loads in 8 parts (a1 units j = 0..3, then dz2 units j = 0, 1
  // in halves), issued one per (k-step, n tile) slot of the first two k-steps of
  // the current image's MFMAs: issued between the barriers, with every CU at the
  // same point, the 72 KB per image stalled the waves at issue for the whole
  // chip's transfer time (tools/kbench.py conv2_wgrad_anat*: 0.66 of 1.78 ms)
  auto fetch_part = [&](int b, int k) {
    // per-image buffer resources: 32-bit offsets, and a load past the range (the
    // a1 units >= XU, the dz2 slots >= 81) returns 0 without a branch
    if (k < 4) {
      const auto ra = make_rsrc(a1 + (size_t)b * 12800, 12800 * 4);
      const int off = tid + 512 * k < XU ? xsrc[k] * 4 : 0x7ffffff0;
      xs[k][0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ra, off, 0, 0));
      xs[k][1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ra, off + 16, 0, 0));
    } else {
      const auto rd = make_rsrc(dz2 + (size_t)b * (81 * 64), 81 * 64 * 4);
      const int j = (k - 4) >> 1, e0 = 4 * ((k - 4) & 1), v = tid + 512 * j;
#pragma unroll
      for (int e = e0; e < e0 + 4; ++e) {
        const int r = 8 * (v >> 6) + e;
        const int off = v < DU && r < 81 ? (c2w_pix(r) * 64 + (v & 63)) * 4 : 0x7ffffff0;
        ds[j][e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rd, off, 0, 0));
      }
    }
  };
  auto fetch = [&](int b) {
#pragma unroll
    for (int k = 0; k < 8; ++k) fetch_part(b, k);
  };
  auto put = [&](bool count) {   // count: add the dz2 to the bias partial
#pragma unroll
    for (int j = 0; j < XPER; ++j)
      if (tid + 512 * j < XU) {
        Frag3 f;
        split8(xs[j][0], xs[j][1], f, false);
        *reinterpret_cast<bf16x8*>(&X[xdst[j]]) = f.h;
        *reinterpret_cast<bf16x8*>(&X[XPL + xdst[j]]) = f.m;
        *reinterpret_cast<bf16x8*>(&X[2 * XPL + xdst[j]]) = f.l;
      }
#pragma unroll
    for (int j = 0; j < DPER; ++j) {
      const int v = tid + 512 * j;
      if (v < DU) {
        Frag3 f;
        split8(f32x4{ds[j][0], ds[j][1], ds[j][2], ds[j][3]}, f32x4{ds[j][4], ds[j][5], ds[j][6], ds[j][7]}, f,
               false);
#pragma unroll
        for (int e = 0; e < 8; ++e) bsum += count ? ds[j][e] : 0.f;
        const int off = (v & 63) * DR + 8 * (v >> 6);
        *reinterpret_cast<bf16x8*>(&D[off]) = f.h;
        *reinterpret_cast<bf16x8*>(&D[DPL + off]) = f.m;
        *reinterpret_cast<bf16x8*>(&D[2 * DPL + off]) = f.l;
      }
    }
  };
  f32x4 acc[4][4];   // [n tile j][co tile mt]
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) acc[j][mt] = zero4();
  const int Z = gridDim.x;
  int b = blockIdx.x;
  // the odd blocks start ~half an image late (s_sleep 100 = 6,400 clocks): every
  // block issues its next image's loads at the same k-steps, and in lock step the
  // whole chip's loads arrive as one burst per image (1.69 -> 1.61-1.63 ms, kbench)
  if (blockIdx.x & 1) __builtin_amdgcn_s_sleep(100);
  if (b < B) {
    fetch(b);
    put(true);
  }
  __syncthreads();
  typedef short s16x4 __attribute__((ext_vector_type(4)));
  for (; b < B; b += Z) {
    const bool pf = b + Z < B;
    const int bn = pf ? b + Z : b;   // the last image re-reads itself (no branch in the MFMA stream)
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      Frag3 a[4];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        const int off = (16 * mt + i16) * DR + 32 * s + 8 * g;
        a[mt].h = *reinterpret_cast<const bf16x8*>(&D[off]);
        a[mt].m = *reinterpret_cast<const bf16x8*>(&D[DPL + off]);
        a[mt].l = *reinterpret_cast<const bf16x8*>(&D[2 * DPL + off]);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (4 * s + j < 8) {
          fetch_part(bn, 4 * s + j);
          __builtin_amdgcn_sched_barrier(0);   // the loads stay in their slot
        }
        const int tap = 2 * wave + (j >> 1), ky = tap >> 2, kx = tap & 3, cb = j & 1;
        const int toff = 20 * ky + 10 * (kx & 1) + (kx >> 1);
        s16x4 t[3][2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int Q = Qb[s][h] + toff, unit = (4 * cb + p) ^ (((Q >> 3) & 1) * 4);
          const uint16_t* rp = &X[Q * 32 + 4 * unit];
#pragma unroll
          for (int pl = 0; pl < 3; ++pl)
            t[pl][h] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                (__attribute__((address_space(3))) s16x4*)(rp + pl * XPL));
        }
        Frag3 bf;
        bf.h = __builtin_bit_cast(bf16x8, __builtin_shufflevector(t[0][0], t[0][1], 0, 1, 2, 3, 4, 5, 6, 7));
        bf.m = __builtin_bit_cast(bf16x8, __builtin_shufflevector(t[1][0], t[1][1], 0, 1, 2, 3, 4, 5, 6, 7));
        bf.l = __builtin_bit_cast(bf16x8, __builtin_shufflevector(t[2][0], t[2][1], 0, 1, 2, 3, 4, 5, 6, 7));
#define PPO_PART(XX, YY) \
  _Pragma("unroll") for (int mt = 0; mt < 4; ++mt) acc[j][mt] = mma(a[mt].XX, bf.YY, acc[j][mt]);
        PPO_PRODUCTS(NP, PPO_PART)
#undef PPO_PART
      }
    }
    __syncthreads();   // the image is consumed
    put(pf);   // unconditional: every load is waited for inside the iteration
    __syncthreads();   // the next image is in LDS
  }
  // this block's partial: C row 4g + r of co tile mt, column i16 of n tile j
  float* o = slab + (size_t)blockIdx.x * (64 * 512) + 64 * wave + i16;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) o[(16 * mt + 4 * g + r) * 512 + 16 * j] = acc[j][mt][r];
  bred[tid] = bsum;
  __syncthreads();
  if (tid < 64) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < 8; ++w) t += bred[tid + 64 * w];
    slab_bias[(size_t)blockIdx.x * 64 + tid] = t;
  }
}

// conv2 dgrad, image-resident on the bf16 matrix cores (exact split, DESIGN.md
// §3): the phase-merged GEMM of Conv2Dgrad (n = (phase, ci), k = (tap, co)),
// one persistent block (8 waves) per CU walking images.  Per image the LDS holds
// dz2 already split into three bf16 planes, as a zero-padded 12 x 10 pixel grid
// (dz2 pixel (oy, ox) at (oy + 1, ox + 1); column 10 of a row is column 0 of the
// next, also zero): 2 stages x 51,840 B, the next image in flight into registers,
// so the k loop has no staging, no barrier and no range tests.  GEMM row m =
// 10 yy + xx is the dz1 phase pixel (yy, xx); its tap (ty, tx) is grid pixel
// m + 11 - (10 ty + tx).  A pixel is 144 B (64 co + 8 pad): 16 consecutive
// pixels start on 16 distinct 16-B bank slots (36 p mod 64, 9 odd), so the
// fragment reads are conflict-free without a swizzle and every (tile, k-step)
// offset is an immediate.
//   Border taps skipped: the rows run in 7 tiles — top row yy = 0 (10 pixels),
// five interior tiles (m = 10 .. 89, exact), bottom row yy = 9.  k-step s takes
// tap row ty = s & 1, lane group g = (tx = g & 1, co 16 (s >> 1) + 8 (g >> 1)):
// the top tile (ty = 1 reads only zero padding there) runs the even k-steps, the
// bottom tile (ty = 0) the odd ones: 48 tile-k-steps per image instead of 56 —
// 6 tiles every k-step (7 -> 1.87 ms per 65,536-image minibatch from 2.03).
// The k loop is software-pipelined over half k-steps (two groups of 3 tiles:
// the next group's fragments are read while the current group's MFMAs run;
// compute alone 1.41 -> 1.36 ms).  W2d [128][(ty, tx, co)] as packed: lane (n, g) of
// k-step s reads W2d[n][128 ty + 64 tx + 16 (s >> 1) + 8 (g >> 1) .. +7].
// Wave w owns n tile w (phase w >> 1, ci 16 (w & 1) + [0, 16)) for all of K,
// its weight fragments (pre-split planes, 8 k-steps x 3) in 96 VGPRs.
// Swapped operands (weights as A, pixels as B): lane (i16, g) holds row
// mrow(t) + i16 and the 4 consecutive channels 4g .. 4g+3 of its n tile — one
// 16-B store per tile; dummy rows get an out-of-range buffer offset (the store
// is dropped) instead of a branch.  The stores of image b are issued during
// image b + G's k-steps (one row tile per k-step) from registers masked at the
// end of image b, instead of all waves storing 51.2 KB at once before the barrier.
// BITS: the ReLU mask comes as bits (a1 points at u32 words [B][400] from
// ppo_conv1_fwd_mask, 1.6 KB per image) instead of the fp32 activations
// (51.2 KB per image): 40 % less HBM traffic, 12 % less time.
template <int NP, bool BITS = false>
__global__ __launch_bounds__(512) void conv2_dgrad_x9_kernel(const float* __restrict__ dz2, int B,
                                                            const uint16_t* __restrict__ wpl,
                                                            const float* __restrict__ a1,
                                                            float* __restrict__ dz1, int stagger) {
  constexpr int HO = 9, CO = 64, GW = 10, GP = 12 * GW, PS = 72, PL = GP * PS, MT = 7, KS = 8;
  constexpr int CH = HO * HO * CO / 8, PER = (CH + 511) / 512, WN = 128 * 256;
  __shared__ __attribute__((aligned(16))) uint16_t S[2][3][PL];
  __shared__ int etab[16 * MT];   // row (t, i16) -> output offset yy*1280 + xx*64 (or -1: dummy row)
  // ReLU mask of a1 (conv1's output) for the image: bits, or one byte per
  // element, staged like dz2 (coalesced 16-B loads one image ahead, in registers)
  constexpr int MC = BITS ? 400 : 400 * 32 / 4, MPER = (MC + 511) / 512;
  __shared__ __attribute__((aligned(16))) uint32_t Mk[2][MC];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i16 = lane & 15, g = lane >> 4;
  const int n = 16 * wave + i16, ph = wave >> 1;
  constexpr auto mrow = [](int t) { return t == 0 ? 0 : t == MT - 1 ? 90 : 16 * t - 6; };
  bf16x8 bw[KS][3];
#pragma unroll
  for (int s = 0; s < KS; ++s)
#pragma unroll
    for (int p = 0; p < 3; ++p)
      bw[s][p] = *reinterpret_cast<const bf16x8*>(wpl + (size_t)p * WN + n * 256 + 128 * (s & 1) + 64 * (g & 1) +
                                                  16 * (s >> 1) + 8 * (g >> 1));
  wait_vm0();
  // zero the pad pixels of both stages (staging only ever writes the 81 real ones)
  for (int i = tid; i < 2 * 3 * GP * 9; i += 512) {
    const int c = i % (GP * 9), p = c / 9, py = p / GW, px = p - GW * py;
    if (py == 0 || py >= 10 || px == 0)
      *reinterpret_cast<uint4*>(&S[i / (3 * GP * 9)][(i / (GP * 9)) % 3][8 * c]) = uint4{0, 0, 0, 0};
  }
  if (tid < 16 * MT) {
    const int t = tid >> 4, r = tid & 15, m = mrow(t) + r;
    etab[tid] = ((t == 0 || t == MT - 1) && r >= 10) ? -1 : (m / 10) * 1280 + (m % 10) * 64;
  }
  // byte offset of this lane's fragment at row 0, ty 0, k-step 0; (tile t, k-step
  // s) adds 144 (mrow(t) - 10 (s & 1)) + 32 (s >> 1): an immediate
  const int abase = (i16 + 11 - (g & 1)) * (2 * PS) + 16 * (g >> 1);
  f32x4 stg[PER][2];
  f32x4 mst[BITS ? 1 : MPER];
  uint4 mbv;
  // part j of an image's loads: dz2 unit j (+ the mask bits with the last one)
  auto fetch_part = [&](int b, int j) {
    const f32x4* src = reinterpret_cast<const f32x4*>(dz2 + (size_t)b * (HO * HO * CO));
    const int c = tid + 512 * j;
    const int cc = c < CH ? c : 0;   // unconditional loads: no exec branch around them
    stg[j][0] = src[2 * cc];
    stg[j][1] = src[2 * cc + 1];
    if constexpr (BITS) {
      if (j == PER - 1) {   // 400 words; lanes past them read out of range (0), no branch
        const auto rm = make_rsrc(reinterpret_cast<const uint32_t*>(a1) + (size_t)b * 400, 1600);
        mbv = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rm, tid < 100 ? 16 * tid : 0x7ffffff0,
                                                                              0, 0));
      }
    }
  };
  auto fetch = [&](int b) {
    if constexpr (BITS) {
#pragma unroll
      for (int j = 0; j < PER; ++j) fetch_part(b, j);
    } else {
      const f32x4* src = reinterpret_cast<const f32x4*>(dz2 + (size_t)b * (HO * HO * CO));
#pragma unroll
      for (int j = 0; j < PER; ++j) {
        const int c = tid + 512 * j;
        const int cc = c < CH ? c : 0;
        stg[j][0] = src[2 * cc];
        stg[j][1] = src[2 * cc + 1];
      }
      const f32x4* ms = reinterpret_cast<const f32x4*>(a1 + (size_t)b * 12800);
#pragma unroll
      for (int j = 0; j < MPER; ++j) {
        const int c = tid + 512 * j;
        if (c < MC) mst[j] = ms[c];
      }
    }
  };
  auto put = [&](int buf) {
    if constexpr (BITS) {
      if (tid < 100) reinterpret_cast<uint4*>(Mk[buf])[tid] = mbv;
    } else {
#pragma unroll
      for (int j = 0; j < MPER; ++j) {
        const int c = tid + 512 * j;
        if (c < MC)
          Mk[buf][c] = (mst[j][0] > 0.f ? 1u : 0u) | (mst[j][1] > 0.f ? 0x100u : 0u) |
                       (mst[j][2] > 0.f ? 0x10000u : 0u) | (mst[j][3] > 0.f ? 0x1000000u : 0u);
      }
    }
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int c = tid + 512 * j;
      if (c < CH) {
        const int r = c >> 3, oy = r / HO, p = (oy + 1) * GW + (r - HO * oy) + 1;
        const int off = p * PS + 8 * (c & 7);
        Frag3 f;
        split8(stg[j][0], stg[j][1], f, false);
        *reinterpret_cast<bf16x8*>(&S[buf][0][off]) = f.h;
        *reinterpret_cast<bf16x8*>(&S[buf][1][off]) = f.m;
        *reinterpret_cast<bf16x8*>(&S[buf][2][off]) = f.l;
      }
    }
  };
  const int G = gridDim.x;
  int b = blockIdx.x, cur = 0;
  if (b < B) {
    fetch(b);
    put(0);
    if (b + G < B) fetch(b + G);
  }
  __syncthreads();
  const bool late = (stagger & 1) && wave >= 4;   // waves 4-7 stage after their compute (see conv3 dgrad; !BITS)
  f32x4 eacc[MT];
  int bprev = -1;
  const int cbs = (ph >> 1) * 640 + (ph & 1) * 32 + 16 * (wave & 1) + 4 * g;
  // (bp < 0, before the first image: an empty range drops the store)
  auto store_tile = [&](int t, const f32x4& v, int bp) {
    const int eo = etab[16 * t + i16];
    const auto rs = make_rsrc(dz1 + (size_t)max(bp, 0) * 12800, bp >= 0 ? 12800 * 4 : 0);
    bstore_f32x4(v, rs, eo >= 0 ? 4 * (eo + cbs) : -1);
  };
  for (; b < B; b += G) {
    // BITS: branch-free staging (a conditional load made the wait counts unknown
    // at the merge): the next image's stage is written unconditionally and the
    // image after next (the block's last image re-read past the end) is loaded in
    // two parts during k-steps 1 and 3, not all at once before the k loop
    const int bnn = b + 2 * G < B ? b + 2 * G : b;
    if constexpr (BITS) {
      // every load in flight is this stage's (issued a k-step or more ago): wait
      // for all of them here, or the partial unit's exec branch in put leaves them
      // pending on one path and the fragment reads below wait one by one
      __builtin_amdgcn_s_waitcnt(0x0f70);   // vmcnt(0) (expcnt / lgkmcnt unconstrained)
      put(cur ^ 1);
    } else if (!late) {
      if (b + G < B) put(cur ^ 1);
      if (b + 2 * G < B) fetch(b + 2 * G);
    }
    const char* Sb = reinterpret_cast<const char*>(S[cur][0]) + abase;
    f32x4 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = zero4();
    // software pipeline over half k-steps: group 0 = {border tile of the tap
    // row, tiles 1, 2}, group 1 = tiles 3-5; the fragments of the next group
    // are read while the current one's MFMAs run (2 x 36 VGPRs)
    Frag3 fr[2][3];
    auto tile_of = [](int s, int grp, int u) {
      return grp == 0 ? (u == 0 ? ((s & 1) ? MT - 1 : 0) : u) : 3 + u;
    };
    auto ld = [&](int s, int grp) {
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        const int t = tile_of(s, grp, u);
        const char* q = Sb + 2 * PS * (mrow(t) - 10 * (s & 1)) + 32 * (s >> 1);
        fr[grp][u].h = *reinterpret_cast<const bf16x8*>(q);
        fr[grp][u].m = *reinterpret_cast<const bf16x8*>(q + 2 * PL);
        fr[grp][u].l = *reinterpret_cast<const bf16x8*>(q + 4 * PL);
      }
    };
    auto mm = [&](int s, int grp) {
      const Frag3 w = {bw[s][0], bw[s][1], bw[s][2]};
#define PPO_PART(X, Y)                                                                \
  _Pragma("unroll") for (int u = 0; u < 3; ++u) {                                     \
    const int t = tile_of(s, grp, u);                                                 \
    acc[t] = mma(w.Y, fr[grp][u].X, acc[t]);                                          \
  }
      PPO_PRODUCTS(NP, PPO_PART)
#undef PPO_PART
    };
    // (the fp32-mask variant holds 28 more VGPRs of mask staging: no pipeline)
    if constexpr (BITS) ld(0, 0);
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      if constexpr (BITS) {
        ld(s, 1);
        __builtin_amdgcn_sched_barrier(0);
        mm(s, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (s + 1 < KS) ld(s + 1, 0);
        __builtin_amdgcn_sched_barrier(0);
        mm(s, 1);
      } else {
        ld(s, 0);
        mm(s, 0);
        ld(s, 1);
        mm(s, 1);
      }
      if constexpr (BITS) {
        if (s < MT) store_tile(s, eacc[s], bprev);
        if (s == 1 || s == 3) fetch_part(bnn, s >> 1);
        __builtin_amdgcn_sched_barrier(0);
      } else if (s < MT && bprev >= 0) {
        store_tile(s, eacc[s], bprev);
      }
    }
    // masked results of this image, stored during the next one's k-steps:
    // C row 4g + r of the swapped tile is channel 4g + r of pixel row (t, i16)
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      const int i = max(etab[16 * t + i16], 0) + cbs;   // element (pixel i >> 5, channels (i & 31) + r)
      const uint32_t mw = Mk[cur][i >> 5] >> (i & 31);
      const uint8_t* mk = reinterpret_cast<const uint8_t*>(Mk[cur]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool keep = BITS ? ((mw >> r) & 1u) != 0 : mk[i + r] != 0;
        eacc[t][r] = keep ? acc[t][r] : 0.f;
      }
    }
    bprev = b;
    if (!BITS && late) {
      if (b + G < B) put(cur ^ 1);
      if (b + 2 * G < B) fetch(b + 2 * G);
    }
    __syncthreads();   // every wave is done with S[cur]; S[cur ^ 1] is complete
    cur ^= 1;
  }
  if (bprev >= 0) {
#pragma unroll
    for (int t = 0; t < MT; ++t) store_tile(t, eacc[t], bprev);
  }
}

}  // namespace

static int conv2_fwd_impl(const float* a1, int B, const float* w2p, const float* b2, float* out, uint16_t* mbits,
                          void* stream) {
  if (!mbits && B > 0 && B <= tune_small_b()) return small_conv2_fwd(a1, B, w2p, b2, out, as_stream(stream));
  if (B <= 0) return 0;
  const unsigned nb = img_grid(B);
  int slot;
  const bool prof = ppo_prof_begin("conv2_fwd", as_stream(stream), &slot);
  const uint16_t* wpl = planes_of(w2p, 64 * 512);
  hipStream_t st = as_stream(stream);
  const int np = tune_products();
  if (mbits && np == 9) conv2_fwd_x9c_kernel<9, true><<<nb, 512, 0, st>>>(a1, B, wpl, b2, out, mbits);
  else if (mbits && np == 1) conv2_fwd_x9c_kernel<1, true><<<nb, 512, 0, st>>>(a1, B, wpl, b2, out, mbits);
  else if (mbits) conv2_fwd_x9c_kernel<6, true><<<nb, 512, 0, st>>>(a1, B, wpl, b2, out, mbits);
  else PPO_LAUNCH_NP(conv2_fwd_x9c_kernel, nb, 512, st, a1, B, wpl, b2, out, nullptr);
  // output pixel 72 of every image in a launch of its own, 16 images per tile
  const int ntile = (B + 15) / 16;
  const unsigned nl = (unsigned)(ntile < 512 ? ntile : 512);
  if (mbits && np == 9) conv2_fwd_lone_kernel<9, true><<<nl, 512, 0, st>>>(a1, B, wpl, b2, out, mbits);
  else if (mbits && np == 1) conv2_fwd_lone_kernel<1, true><<<nl, 512, 0, st>>>(a1, B, wpl, b2, out, mbits);
  else if (mbits) conv2_fwd_lone_kernel<6, true><<<nl, 512, 0, st>>>(a1, B, wpl, b2, out, mbits);
  else if (np == 9) conv2_fwd_lone_kernel<9, false><<<nl, 512, 0, st>>>(a1, B, wpl, b2, out, nullptr);
  else if (np == 1) conv2_fwd_lone_kernel<1, false><<<nl, 512, 0, st>>>(a1, B, wpl, b2, out, nullptr);
  else conv2_fwd_lone_kernel<6, false><<<nl, 512, 0, st>>>(a1, B, wpl, b2, out, nullptr);
  if (prof) ppo_prof_end(slot, st, 2.0 * B * 81 * 64 * 512);
  PPO_LAUNCH_CHECK("conv2_fwd_x9c_kernel");
  return 0;
}

PPO_API int ppo_conv2_fwd(const float* a1, int B, const float* w2p, const float* b2, float* out, void* stream) {
  return conv2_fwd_impl(a1, B, w2p, b2, out, nullptr, stream);
}

// conv2 forward that also writes the ReLU mask of its output as bits
// (mbits [B][81] u64, bit c of pixel p = out[p][c] > 0) for ppo_conv3_dgrad_bits.
PPO_API int ppo_conv2_fwd_mask(const float* a1, int B, const float* w2p, const float* b2, float* out,
                               uint64_t* mbits, void* stream) {
  PPO_REQUIRE(mbits != nullptr, "ppo_conv2_fwd_mask: null mask");
  return conv2_fwd_impl(a1, B, w2p, b2, out, reinterpret_cast<uint16_t*>(mbits), stream);
}

template <bool BITS>
static int conv2_dgrad_img(const float* dz2, int B, const float* w2d, const float* mask, float* dz1, void* stream) {
  if (B <= 0) return 0;
  const unsigned nb = img_grid(B);
  int slot;
  const bool prof = ppo_prof_begin("conv2_dgrad", as_stream(stream), &slot);
  const uint16_t* wpl = planes_of(w2d, 128 * 256);
  const int sg = tune_stagger() & ~2, np = tune_products();
  if (np == 9) conv2_dgrad_x9_kernel<9, BITS><<<nb, 512, 0, as_stream(stream)>>>(dz2, B, wpl, mask, dz1, sg);
  else if (np == 1) conv2_dgrad_x9_kernel<1, BITS><<<nb, 512, 0, as_stream(stream)>>>(dz2, B, wpl, mask, dz1, sg);
  else conv2_dgrad_x9_kernel<6, BITS><<<nb, 512, 0, as_stream(stream)>>>(dz2, B, wpl, mask, dz1, sg);
  if (prof) ppo_prof_end(slot, as_stream(stream), 2.0 * B * 81 * 64 * 512);
  PPO_LAUNCH_CHECK("conv2_dgrad_x9_kernel");
  return 0;
}

// conv2 dgrad with the conv1 ReLU mask as bits (m1bits [B][400] u32 from ppo_conv1_fwd_mask)
PPO_API int ppo_conv2_dgrad_bits_ok() { return 1; }
PPO_API int ppo_conv2_dgrad_bits(const float* dz2, int B, const float* w2d, const uint32_t* m1bits, float* dz1,
                                 void* stream) {
  PPO_REQUIRE(m1bits != nullptr, "ppo_conv2_dgrad_bits: null mask");
  return conv2_dgrad_img<true>(dz2, B, w2d, reinterpret_cast<const float*>(m1bits), dz1, stream);
}

PPO_API int ppo_conv2_dgrad(const float* dz2, int B, const float* w2d, const float* a1, float* dz1, void* stream) {
  return conv2_dgrad_img<false>(dz2, B, w2d, a1, dz1, stream);
}

PPO_API int ppo_conv2_wgrad(const float* dz2, const float* a1, int B, int Z, float* slab, float* slab_bias,
                            void* stream) {
  if (B <= 0 || Z <= 0) return 0;
  int slot;
  const bool prof = ppo_prof_begin("conv2_wgrad", as_stream(stream), &slot);
  PPO_LAUNCH_NP(conv2_wgrad_x9_kernel, Z, 512, as_stream(stream), dz2, a1, B, slab, slab_bias);
  if (prof) ppo_prof_end(slot, as_stream(stream), 2.0 * B * 81 * 64 * 512);
  PPO_LAUNCH_CHECK("conv2_wgrad_x9_kernel");
  return 0;
}
