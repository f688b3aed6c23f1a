// conv3 of the CNNBase trunk (conv1.hip's header has the network and the layouts):
// image-resident kernels on the bf16 matrix cores (exact split) —
// input gradient, forward (its body in conv3_fwd_body.h), weight gradient — and
// their launchers.
#include "conv_launch.h"
#include "conv3_fwd_body.h"

namespace {

// conv3 dgrad, image-resident on the bf16 matrix cores (exact split, DESIGN.md
// §3): dz2[m][ci] = [a2 > 0] Σ_(ky,kx,co) dz3[y-ky][x-kx][co] W3d[ci][(ky,kx,co)],
// m = (y, x) over the 9 x 9 input (81 rows in 6 tiles of 16), k-step = tap, lane
// group g = co chunk.  One persistent block (8 waves) per CU walks images; per
// image the LDS holds dz3 split into three bf16 planes on a zero-padded grid of
// width 25 (dz3 pixel (oy, ox) at (oy + 2) * 25 + ox + 2; 11 rows), in 16-B units
// c * 288 + pixel: row m's tap pixel is 25 y + x + const ≡ m + const (mod 16), so
// the 16 rows of a tile hit distinct slots (conflict-free ds_read_b128), and out-of-
// range taps read zeros.  Two stages (2 x 55,296 B) plus the a2 ReLU mask as
// bytes (2 x 5,184 B): the next image is staged before the compute, one barrier
// per image.  Wave w: ci tile w & 3 (weights, 9 taps x 3 planes, in 108 VGPRs),
// row tiles 3 (w >> 2) .. +2.
// BITS: the a2 ReLU mask comes as bits (a2 points at u64 words [B][81] from
// ppo_conv2_fwd_mask: 648 B instead of 20.7 KB per image).
template <int NP, bool BITS>
__device__ __forceinline__ void conv3_dgrad_img_body(const float* __restrict__ dz3, int B,
                                                     const uint16_t* __restrict__ wpl,
                                                     const float* __restrict__ a2, float* __restrict__ dz2,
                                                     int stagger) {
  constexpr int GW = 25, CS = 288, PLU = 4 * CS, KS = 9, WN = 64 * 288;
  constexpr int DU = 49 * 4, MC = 81 * 64 / 4, MPER = (MC + 511) / 512;
  __shared__ __attribute__((aligned(16))) uint16_t S[2][3 * PLU * 8];
  __shared__ __attribute__((aligned(16))) uint32_t Mk[2][MC];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i16 = lane & 15, g = lane >> 4;
  const int nt = wave & 3, mh = wave >> 2, ci = 16 * nt + i16;
  bf16x8 bw[KS][3];
#pragma unroll
  for (int s = 0; s < KS; ++s)
#pragma unroll
    for (int p = 0; p < 3; ++p)
      bw[s][p] = *reinterpret_cast<const bf16x8*>(wpl + (size_t)p * WN + ci * 288 + 32 * s + 8 * g);
  wait_vm0();
  for (int i = tid; i < 2 * 3 * PLU; i += 512) reinterpret_cast<uint4*>(&S[0][0])[i] = uint4{0, 0, 0, 0};
  // unit index of this lane's A fragment per row tile for tap (0, 0); tap
  // (ky, kx) subtracts 25 ky + kx
  // Row tiles and the taps they need: a tap whose source pixel is off the 7 x 7
  // grid for all 16 rows of a tile is skipped (tile 0: ky <= 1, tile 4: ky >= 1,
  // tile 5 = pixel 80 alone: tap (2, 2) only) — 40 of the 54 tile-taps.  Wave
  // halves take tiles {1, 2, 5} (19 tile-taps) and {0, 3, 4} (21).
  constexpr unsigned TILES = 0x430521u;   // nibbles: tiles of half 0 (1, 2, 5), half 1 (0, 3, 4)
  // tap masks per tile (bit 3 ky + kx): {0x03F, 0x1FF, 0x1FF, 0x1FF, 0x1F8, 0x100}
  int qrow[3], tl[3];
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    tl[t] = (TILES >> (4 * (3 * mh + t))) & 15;
    const int m = min(16 * tl[t] + i16, 80), y = m / 9, x = m - 9 * y;   // dummy rows: pixel 80
    qrow[t] = g * CS + (y + 2) * GW + x + 2;
  }
  f32x4 stg[2];
  f32x4 mst[BITS ? 1 : MPER];
  uint2 mbv;
  auto fetch = [&](int b) {
    if (tid < DU) {
      const f32x4* src = reinterpret_cast<const f32x4*>(dz3 + (size_t)b * 1568);
      stg[0] = src[2 * tid];
      stg[1] = src[2 * tid + 1];
    }
    if constexpr (BITS) {
      if (tid < 81) mbv = reinterpret_cast<const uint2*>(a2)[(size_t)b * 81 + tid];
    } else {
      const f32x4* ms = reinterpret_cast<const f32x4*>(a2 + (size_t)b * 5184);
#pragma unroll
      for (int j = 0; j < MPER; ++j)
        if (tid + 512 * j < MC) mst[j] = ms[tid + 512 * j];
    }
  };
  auto put = [&](int buf) {
    if (tid < DU) {   // unit tid: dz3 pixel tid >> 2, co chunk tid & 3
      const int px = tid >> 2, oy = px / 7, ox = px - 7 * oy;
      const int q = (tid & 3) * CS + (oy + 2) * GW + ox + 2;
      Frag3 f;
      split8(stg[0], stg[1], f, false);
      *reinterpret_cast<bf16x8*>(&S[buf][8 * q]) = f.h;
      *reinterpret_cast<bf16x8*>(&S[buf][8 * (PLU + q)]) = f.m;
      *reinterpret_cast<bf16x8*>(&S[buf][8 * (2 * PLU + q)]) = f.l;
    }
    if constexpr (BITS) {
      if (tid < 81) reinterpret_cast<uint2*>(Mk[buf])[tid] = mbv;
    } else {
#pragma unroll
      for (int j = 0; j < MPER; ++j) {
        const int c = tid + 512 * j;
        if (c < MC)
          Mk[buf][c] = (mst[j][0] > 0.f ? 1u : 0u) | (mst[j][1] > 0.f ? 0x100u : 0u) |
                       (mst[j][2] > 0.f ? 0x10000u : 0u) | (mst[j][3] > 0.f ? 0x1000000u : 0u);
      }
    }
  };
  __syncthreads();   // the zeroed pads
  const int G = gridDim.x;
  int b = blockIdx.x, cur = 0;
  if (b < B) {
    fetch(b);
    put(0);
    if (b + G < B) fetch(b + G);
  }
  __syncthreads();
  // stagger: waves 4-7 (the second wave of every SIMD) stage the next image
  // after their compute instead of before it, so each SIMD's matrix pipe has
  // one computing wave while the other splits and stores
  const bool late = stagger && wave >= 4;
  for (; b < B; b += G) {
    if (!late) {
      if (b + G < B) put(cur ^ 1);
      if (b + 2 * G < B) fetch(b + 2 * G);
    }
    const uint16_t* Sc = S[cur];
    f32x4 acc[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) acc[t] = zero4();
    // the tap masks are compile-time in each of the two instantiations, so the
    // skipped (tile, tap) pairs vanish from the unrolled schedule
    auto compute = [&](auto M0, auto M1, auto M2) {
      constexpr unsigned msk[3] = {decltype(M0)::value, decltype(M1)::value, decltype(M2)::value};
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const int toff = -(GW * (s / 3) + s % 3);
        const Frag3 w = {bw[s][0], bw[s][1], bw[s][2]};
        Frag3 a[3];
#pragma unroll
        for (int u = 0; u < 3; ++u) {
          if (!((msk[u] >> s) & 1u)) continue;
          const uint16_t* q = Sc + 8 * (qrow[u] + toff);
          a[u].h = *reinterpret_cast<const bf16x8*>(q);
          a[u].m = *reinterpret_cast<const bf16x8*>(q + 8 * PLU);
          a[u].l = *reinterpret_cast<const bf16x8*>(q + 16 * PLU);
        }
#define PPO_PART(X, Y) \
  _Pragma("unroll") for (int u = 0; u < 3; ++u) if ((msk[u] >> s) & 1u) acc[u] = mma(w.Y, a[u].X, acc[u]);
        PPO_PRODUCTS(NP, PPO_PART)
#undef PPO_PART
      }
    };
    using std::integral_constant;
    if (mh == 0)
      compute(integral_constant<unsigned, 0x1FF>{}, integral_constant<unsigned, 0x1FF>{},
              integral_constant<unsigned, 0x100>{});
    else
      compute(integral_constant<unsigned, 0x03F>{}, integral_constant<unsigned, 0x1FF>{},
              integral_constant<unsigned, 0x1F8>{});
    // epilogue: C row 4g + r of tile t is input pixel m; ReLU mask of a2
    // swapped orientation (weights as the MFMA A operand): lane (i16, g) holds
    // pixel 16 tl + i16, channels c0 = 16 nt + 4g .. +3 — one 16-B store per tile
    const uint8_t* mk = reinterpret_cast<const uint8_t*>(Mk[cur]);
    const auto rs = make_rsrc(dz2 + (size_t)b * 5184, 5184 * 4);
    const int c0 = 16 * nt + 4 * g;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      const int m = 16 * tl[t] + i16, mm = min(m, 80);
      const uint32_t mw = Mk[cur][2 * mm + (c0 >> 5)] >> (c0 & 31);
      f32x4 y;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool keep = BITS ? ((mw >> r) & 1u) != 0 : mk[mm * 64 + c0 + r] != 0;
        y[r] = keep ? acc[t][r] : 0.f;
      }
      bstore_f32x4(y, rs, m < 81 ? 4 * (m * 64 + c0) : -1);
    }
    if (late) {
      if (b + G < B) put(cur ^ 1);
      if (b + 2 * G < B) fetch(b + 2 * G);
    }
    __syncthreads();   // every wave is done with stage cur; stage cur ^ 1 is complete
    cur ^= 1;
  }
}

// conv3 dgrad on 16-image tiles (knob conv3_dgrad_group, the mask-bits form, B >= 16):
// a tile is input pixel (y, x) of the 16 consecutive images of a group, MFMA column
// i16 = image b0 + i16, so every row of a tile has the same valid taps and only the
// 441 valid (pixel, tap) pairs are issued — 662 MFMAs per image at 6 products instead
// of 960, and the taps the per-image kernel issues against its zero border add exact
// zeros, so the two kernels agree bit for bit: per output element the taps in
// ascending s = 3 ky + kx, the part products in PPO_PRODUCTS order.
// One persistent block (8 waves) per CU walks groups.  The LDS holds one stage: the
// group's dz3 split into three bf16 planes, 16-B unit (plane, co chunk c, pixel, image)
// at plane * 3136 + c * 784 + pixel * 16 + image (no border: every unit is real;
// 150,528 B) and the 16 images' mask words (10,368 B).  A fragment read's 16 lanes
// of one g are the 16 images of one (c, pixel): 16 consecutive units, conflict-free
// (tools/conv3_group_banks.py); the address is the lane's base plus an immediate.
// The next group's dz3 (7 units per lane) and mask words wait in registers during
// the compute and are split and written between the two barriers of the group
// boundary.  Wave w: ci tile w & 3 (weights as in the per-image kernel), output rows
// {0, 1, 2, 3, 8} (w < 4: 10 of the 21 valid (y, ky)) or {4 .. 7} (11) — both halves
// of a ci tile on one SIMD.  Per (y, ky) the 7 source pixels are read once each,
// ox = 6 .. 0, and feed outputs x = ox + kx, which keeps every output's kx ascending.
// A ragged last group: the missing images load zeros and their stores are dropped,
// both by the range of the group's buffer resources.
template <int NP>
__device__ __forceinline__ void conv3_dgrad_group_body(const float* __restrict__ dz3, int B,
                                                       const uint16_t* __restrict__ wpl,
                                                       const uint64_t* __restrict__ m2,
                                                       float* __restrict__ dz2) {
  constexpr int KS = 9, WN = 64 * 288, GI = 16;
  constexpr int CSU = 49 * GI, PLU = 4 * CSU;   // 16-B units per co chunk, per plane
  constexpr int MW = GI * 81, MPER = (MW + 511) / 512, NJ = 7;   // px = wave + 8 j, j < NJ
  __shared__ __attribute__((aligned(16))) uint16_t S[3 * PLU * 8];
  __shared__ __attribute__((aligned(16))) uint32_t Mk[2 * MW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i16 = lane & 15, g = lane >> 4;
  const int nt = wave & 3, mh = wave >> 2, ci = 16 * nt + i16;
  bf16x8 bw[KS][3];
#pragma unroll
  for (int s = 0; s < KS; ++s)
#pragma unroll
    for (int p = 0; p < 3; ++p)
      bw[s][p] = *reinterpret_cast<const bf16x8*>(wpl + (size_t)p * WN + ci * 288 + 32 * s + 8 * g);
  wait_vm0();
  f32x4 stg[NJ][2];
  uint2 mbv[MPER];
  // lane (i16, g) of wave w fetches co chunk g of pixels w, w + 8, .. of image b0 + i16
  // (a wave's load covers 16 whole 128-B pixel rows); images and mask words past the
  // batch are out of the resources' range and read 0
  auto fetch = [&](int b0) {
    const int n = max(min(B - b0, GI), 0);
    const auto rd = make_rsrc(dz3 + (size_t)b0 * 1568, n * 6272);
    const auto rm = make_rsrc(m2 + (size_t)b0 * 81, n * 648);
    const int o = i16 * 6272 + wave * 128 + g * 32;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int off = wave + 8 * j < 49 ? o + 1024 * j : 0x7fffffc0;
      stg[j][0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rd, off, 0, 0));
      stg[j][1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rd, off + 16, 0, 0));
    }
#pragma unroll
    for (int k = 0; k < MPER; ++k)
      mbv[k] = __builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(rm, 8 * (tid + 512 * k), 0, 0));
  };
  auto put = [&]() {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int px = wave + 8 * j;
      if (px < 49) {
        const int q = g * CSU + px * GI + i16;
        Frag3 f;
        split8(stg[j][0], stg[j][1], f, false);
        *reinterpret_cast<bf16x8*>(&S[8 * q]) = f.h;
        *reinterpret_cast<bf16x8*>(&S[8 * (PLU + q)]) = f.m;
        *reinterpret_cast<bf16x8*>(&S[8 * (2 * PLU + q)]) = f.l;
      }
    }
#pragma unroll
    for (int k = 0; k < MPER; ++k)
      if (tid + 512 * k < MW) reinterpret_cast<uint2*>(Mk)[tid + 512 * k] = mbv[k];
  };
  const int step = GI * gridDim.x, c0 = 16 * nt + 4 * g;
  const int ny = mh ? 4 : 5;
  int b0 = GI * blockIdx.x;
  if (b0 < B) fetch(b0);
  for (; b0 < B; b0 += step) {
    put();
    fetch(b0 + step);
    __syncthreads();   // the group's stage is complete
    const auto rs = make_rsrc(dz2 + (size_t)b0 * 5184, min(B - b0, GI) * 20736);
    for (int iy = 0; iy < ny; ++iy) {
      const int y = mh ? 4 + iy : (iy < 4 ? iy : 8);
      f32x4 acc[9];
#pragma unroll
      for (int x = 0; x < 9; ++x) acc[x] = zero4();
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const int oy = y - ky;
        if (oy < 0 || oy > 6) continue;   // wave-uniform
        const uint16_t* row = S + 8 * (g * CSU + 7 * GI * oy + i16);
        const Frag3 w[3] = {{bw[3 * ky][0], bw[3 * ky][1], bw[3 * ky][2]},
                            {bw[3 * ky + 1][0], bw[3 * ky + 1][1], bw[3 * ky + 1][2]},
                            {bw[3 * ky + 2][0], bw[3 * ky + 2][1], bw[3 * ky + 2][2]}};
#pragma unroll
        for (int ox = 6; ox >= 0; --ox) {
          const uint16_t* q = row + 8 * GI * ox;
          Frag3 a;
          a.h = *reinterpret_cast<const bf16x8*>(q);
          a.m = *reinterpret_cast<const bf16x8*>(q + 8 * PLU);
          a.l = *reinterpret_cast<const bf16x8*>(q + 16 * PLU);
#define PPO_PART(X, Y) \
  _Pragma("unroll") for (int kx = 0; kx < 3; ++kx) acc[ox + kx] = mma(w[kx].Y, a.X, acc[ox + kx]);
          PPO_PRODUCTS(NP, PPO_PART)
#undef PPO_PART
        }
      }
      // epilogue: lane (i16, g) holds channels c0 .. c0 + 3 of pixel (y, x) of image
      // b0 + i16 — one 16-B store per pixel, masked by that image's m2 word
#pragma unroll
      for (int x = 0; x < 9; ++x) {
        const int m = 9 * y + x;
        const uint32_t mw = Mk[i16 * 162 + 2 * m + (c0 >> 5)] >> (c0 & 31);
        f32x4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = ((mw >> r) & 1u) != 0 ? acc[x][r] : 0.f;
        bstore_f32x4(o, rs, i16 * 20736 + 4 * (m * 64 + c0));
      }
    }
    __syncthreads();   // every wave is done with the stage
  }
}

// GRP: the 16-image-tile form (BITS only)
template <int NP, bool BITS = false, bool GRP = false>
__global__ __launch_bounds__(512) void conv3_dgrad_x9_kernel(const float* __restrict__ dz3, int B,
                                                            const uint16_t* __restrict__ wpl,
                                                            const float* __restrict__ a2,
                                                            float* __restrict__ dz2, int stagger) {
  static_assert(BITS || !GRP, "the group form reads mask bits");
  if constexpr (GRP) conv3_dgrad_group_body<NP>(dz3, B, wpl, reinterpret_cast<const uint64_t*>(a2), dz2);
  else conv3_dgrad_img_body<NP, BITS>(dz3, B, wpl, a2, dz2, stagger);
}

// standalone conv3 forward: 12 waves, the lone output in the same launch
template <int NP>
__global__ __launch_bounds__(768) void conv3_fwd_c3_kernel(const float* __restrict__ a2, int B,
                                                           const uint16_t* __restrict__ wpl,
                                                           const float* __restrict__ bias,
                                                           float* __restrict__ out, uint16_t* __restrict__ m3) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[C3C_LDS];
  conv3_fwd_c3_body<NP, 768>(a2, B, wpl, bias, out, lds, m3);
}

// conv3 weight gradient, image-resident on the bf16 matrix cores (exact split,
// DESIGN.md §3): dW3[co][k] = Σ_pixels dz3[m][co] · a2[oy+ky][ox+kx][ci], k = (ky,
// kx, ci); per image a 32 x 576 x 49 product, accumulated in registers over the
// block's images and written once as its split-K partial (slab [Z][32][576],
// bias partials [Z][32]).  Reduction slot r = 8 oy + ox (ox = 7 and oy = 7 are
// dummy slots, dz = 0): 64 slots = 2 k-steps.  Per image (2 stages) the LDS holds
//   X [3][9 x 12 px][64 ci]  a2 split into bf16 planes, pixel P = 12 y + x, 128-B
//                            rows; the B fragment (8 slots x 16 ci of one tap) is two
//                            ds_read_b64_tr_b16 per plane whose 4-slot row groups
//                            are 4 consecutive ox and the next oy (P + 12): with
//                            8-B unit u of pixel P at u ^ 4 ((P >> 1) & 3) every
//                            32-lane half hits distinct banks
//   D [3][32 co][112]        dz3 transposed to [co][slot] (224-B rows: conflict-free
//                            ds_read_b128 A fragments)
// 12 waves (3 per SIMD), wave w: n tiles 3w .. 3w+2 (both co tiles).
template <int NP>
__global__ __launch_bounds__(768) void conv3_wgrad_x9_kernel(const float* __restrict__ dz3,
                                                            const float* __restrict__ a2, int B,
                                                            float* __restrict__ slab,
                                                            float* __restrict__ slab_bias) {
  constexpr int NT = 768, XPL = 108 * 64, DR = 112, DPL = 32 * DR;
  constexpr int XU = 81 * 8, XPER = (XU + NT - 1) / NT, DU = 32 * 8;
  __shared__ __attribute__((aligned(16))) uint16_t X[2][3 * XPL];
  __shared__ __attribute__((aligned(16))) uint16_t D[2][3 * DPL];
  __shared__ float bred[DU];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i16 = lane & 15, g = lane >> 4;
  const int q = i16 >> 2, p = i16 & 3;
  // tap-(0,0) pixel of the row this lane addresses in the tr reads of k-step s,
  // half h (dummy slots read pixel (6, 6): finite, times dz = 0)
  int Pb[2][2];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int r = 32 * s + 8 * g + 4 * h + q;
      int oy = r >> 3, ox = r & 7;
      if (oy > 6 || ox > 6) { oy = 6; ox = 6; }
      Pb[s][h] = 12 * oy + ox;
    }
  f32x4 xs[XPER][2];
  float ds[7];
  float bsum = 0.f;   // bias partial of co = tid & 31 (threads < 256: slots of row oy = tid >> 5)
  // the next image's loads in two parts (a2 units; dz3 slots), issued inside the
  // MFMA stream of k-step 0 (as conv2's weight gradient), through per-image buffer
  // resources: lanes past the units / the 7 dz rows read out of range (0), no branch
  static_assert(XPER == 1, "one a2 unit per thread");
  auto fetch_part = [&](int b, int part) {
    if (part == 0) {
      const auto ra = make_rsrc(a2 + (size_t)b * 5184, 5184 * 4);
      const int off = tid < XU ? 32 * tid : 0x7fffffe0;
      xs[0][0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ra, off, 0, 0));
      xs[0][1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ra, off + 16, 0, 0));
    } else {
      const auto rd = make_rsrc(dz3 + (size_t)b * 1568, 1568 * 4);
      const bool on = tid < DU && (tid >> 5) < 7;
      const int o = ((tid >> 5) * 7 * 32 + (tid & 31)) * 4;
#pragma unroll
      for (int e = 0; e < 7; ++e)
        ds[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rd, on ? o + 128 * e : 0x7ffffff0, 0, 0));
    }
  };
  auto fetch = [&](int b) {
    fetch_part(b, 0);
    fetch_part(b, 1);
  };
  auto put = [&](int buf, bool count) {   // count: add the dz to the bias partial
#pragma unroll
    for (int j = 0; j < XPER; ++j) {
      const int u = tid + NT * j;
      if (u < XU) {
        const int px = u >> 3, c = u & 7, y = px / 9, P = 12 * y + (px - 9 * y);
        const int off = P * 64 + 8 * (c ^ (2 * ((P >> 1) & 3)));
        Frag3 f;
        split8(xs[j][0], xs[j][1], f, false);
        *reinterpret_cast<bf16x8*>(&X[buf][off]) = f.h;
        *reinterpret_cast<bf16x8*>(&X[buf][XPL + off]) = f.m;
        *reinterpret_cast<bf16x8*>(&X[buf][2 * XPL + off]) = f.l;
      }
    }
    if (tid < DU) {
      Frag3 f;
      split8(f32x4{ds[0], ds[1], ds[2], ds[3]}, f32x4{ds[4], ds[5], ds[6], 0.f}, f, false);
#pragma unroll
      for (int e = 0; e < 7; ++e) bsum += count ? ds[e] : 0.f;
      const int off = (tid & 31) * DR + 8 * (tid >> 5);
      *reinterpret_cast<bf16x8*>(&D[buf][off]) = f.h;
      *reinterpret_cast<bf16x8*>(&D[buf][DPL + off]) = f.m;
      *reinterpret_cast<bf16x8*>(&D[buf][2 * DPL + off]) = f.l;
    }
  };
  f32x4 acc[3][2];   // [n tile][co tile]
#pragma unroll
  for (int j = 0; j < 3; ++j) acc[j][0] = acc[j][1] = zero4();
  const int Z = gridDim.x;
  int b = blockIdx.x, cur = 0;
  if (b < B) {
    fetch(b);
    put(0, true);
    fetch(b + Z < B ? b + Z : b);
  }
  __syncthreads();
  typedef short s16x4 __attribute__((ext_vector_type(4)));
  for (; b < B; b += Z) {
    // every load in flight is this stage's (no stores in the loop): one explicit
    // wait, then the stage write unconditionally (past the end: not counted)
    __builtin_amdgcn_s_waitcnt(0x0f70);   // vmcnt(0)
    put(cur ^ 1, b + Z < B);
    const int bnn = b + 2 * Z < B ? b + 2 * Z : b;
    const uint16_t* Xc = X[cur];
    const uint16_t* Dc = D[cur];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      Frag3 a[2];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        const int off = (16 * mt + i16) * DR + 32 * s + 8 * g;
        a[mt].h = *reinterpret_cast<const bf16x8*>(&Dc[off]);
        a[mt].m = *reinterpret_cast<const bf16x8*>(&Dc[DPL + off]);
        a[mt].l = *reinterpret_cast<const bf16x8*>(&Dc[2 * DPL + off]);
      }
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int n = 3 * wave + j, tap = n >> 2, ky = tap / 3, kx = tap - 3 * ky, cb = n & 3;
        s16x4 t[3][2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int P = Pb[s][h] + 12 * ky + kx, unit = (4 * cb + p) ^ (4 * ((P >> 1) & 3));
          const uint16_t* rp = &Xc[P * 64 + 4 * unit];
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
  _Pragma("unroll") for (int mt = 0; mt < 2; ++mt) acc[j][mt] = mma(a[mt].XX, bf.YY, acc[j][mt]);
        PPO_PRODUCTS(NP, PPO_PART)
#undef PPO_PART
        if (s == 0 && j < 2) {
          fetch_part(bnn, j);
          __builtin_amdgcn_sched_barrier(0);   // the loads stay in their slot
        }
      }
    }
    __syncthreads();   // stage cur consumed; stage cur ^ 1 complete
    cur ^= 1;
  }
  // this block's partial: C row 4g + r of co tile mt, column i16 of n tile 3w + j
  float* o = slab + (size_t)blockIdx.x * (32 * 576) + 48 * wave + i16;
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) o[(16 * mt + 4 * g + r) * 576 + 16 * j] = acc[j][mt][r];
  if (tid < DU) bred[tid] = bsum;
  __syncthreads();
  if (tid < 32) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < 8; ++w) t += bred[tid + 32 * w];
    slab_bias[(size_t)blockIdx.x * 32 + tid] = t;
  }
}

}  // namespace

static int conv3_fwd_impl(const float* a2, int B, const float* w3p, const float* b3, float* out, uint16_t* m3,
                          void* stream) {
  if (B > 0 && B <= tune_small_b() && !m3) return small_conv3_fwd(a2, B, w3p, b3, out, as_stream(stream));
  if (B <= 0) return 0;
  int slot;
  const bool prof = ppo_prof_begin("conv3_fwd", as_stream(stream), &slot);
  const uint16_t* wpl = planes_of(w3p, 32 * 576);
  // compact rows (three tiles), then the lone output C3_LONE_Q = 42 = (6, 0) in the same launch
  PPO_LAUNCH_NP(conv3_fwd_c3_kernel, img_grid(B), 768, as_stream(stream), a2, B, wpl, b3, out, m3);
  if (prof) ppo_prof_end(slot, as_stream(stream), 2.0 * B * 49 * 32 * 576);
  PPO_LAUNCH_CHECK("conv3_fwd_c3_kernel");
  return 0;
}

PPO_API int ppo_conv3_fwd(const float* a2, int B, const float* w3p, const float* b3, float* out, void* stream) {
  return conv3_fwd_impl(a2, B, w3p, b3, out, nullptr, stream);
}

// the training forward: also the ReLU mask bits of the output, uint16 [B][49][2]
// (conv3_mask_store), read by ppo_fc_dgrad_bits
PPO_API int ppo_conv3_fwd_mask(const float* a2, int B, const float* w3p, const float* b3, float* out,
                               uint16_t* mbits, void* stream) {
  PPO_REQUIRE(mbits != nullptr, "ppo_conv3_fwd_mask: null mask");
  return conv3_fwd_impl(a2, B, w3p, b3, out, mbits, stream);
}

template <bool BITS>
static int conv3_dgrad_img(const float* dz3, int B, const float* w3d, const float* mask, float* dz2, void* stream) {
  if (B <= 0) return 0;
  int slot;
  const bool prof = ppo_prof_begin("conv3_dgrad", as_stream(stream), &slot);
  const uint16_t* wpl = planes_of(w3d, 64 * 288);
  const int sg = tune_stagger(), np = tune_products();
  auto go = [&](auto GRP) {
    constexpr bool G = decltype(GRP)::value;
    const unsigned nb = img_grid(G ? (B + 15) / 16 : B);   // G: a block walks groups of 16 images
    if (np == 9) conv3_dgrad_x9_kernel<9, BITS, G><<<nb, 512, 0, as_stream(stream)>>>(dz3, B, wpl, mask, dz2, sg);
    else if (np == 1) conv3_dgrad_x9_kernel<1, BITS, G><<<nb, 512, 0, as_stream(stream)>>>(dz3, B, wpl, mask, dz2, sg);
    else conv3_dgrad_x9_kernel<6, BITS, G><<<nb, 512, 0, as_stream(stream)>>>(dz3, B, wpl, mask, dz2, sg);
  };
  // the fp32 mask of 16 images does not fit the LDS beside their dz3: bits only
  bool grp = false;
  if constexpr (BITS) {
    grp = B >= 16 && tune_key(TK_CONV3_DGRAD_GROUP) != 0;
    if (grp) go(std::true_type{});
  }
  if (!grp) go(std::false_type{});
  if (prof) ppo_prof_end(slot, as_stream(stream), 2.0 * B * 49 * 32 * 576);
  PPO_LAUNCH_CHECK("conv3_dgrad_x9_kernel");
  return 0;
}

// conv3 dgrad with conv2's ReLU mask as bits (m2bits [B][81] u64 from ppo_conv2_fwd_mask)
PPO_API int ppo_conv3_dgrad_bits_ok() { return 1; }
PPO_API int ppo_conv3_dgrad_bits(const float* dz3, int B, const float* w3d, const uint64_t* m2bits, float* dz2,
                                 void* stream) {
  PPO_REQUIRE(m2bits != nullptr, "ppo_conv3_dgrad_bits: null mask");
  return conv3_dgrad_img<true>(dz3, B, w3d, reinterpret_cast<const float*>(m2bits), dz2, stream);
}

PPO_API int ppo_conv3_dgrad(const float* dz3, int B, const float* w3d, const float* a2, float* dz2, void* stream) {
  return conv3_dgrad_img<false>(dz3, B, w3d, a2, dz2, stream);
}

PPO_API int ppo_conv3_wgrad(const float* dz3, const float* a2, int B, int Z, float* slab, float* slab_bias,
                            void* stream) {
  if (B <= 0 || Z <= 0) return 0;
  int slot;
  const bool prof = ppo_prof_begin("conv3_wgrad", as_stream(stream), &slot);
  PPO_LAUNCH_NP(conv3_wgrad_x9_kernel, Z, 768, as_stream(stream), dz3, a2, B, slab, slab_bias);
  if (prof) ppo_prof_end(slot, as_stream(stream), 2.0 * B * 49 * 32 * 576);
  PPO_LAUNCH_CHECK("conv3_wgrad_x9_kernel");
  return 0;
}
