// conv3_fwd_body.h — the image-resident conv3 forward body, its lone-output tiles,
// the ReLU mask store and their LDS constants, for conv3_fwd_c3_kernel (conv3.hip)
// and the third phase of trunk_fwd_kernel (trunk.hip).
#pragma once
#include "igemm_x9.h"

namespace {

// conv3 forward, image-resident on the bf16 matrix cores (exact split, DESIGN.md
// §3): a3[b][(oy, ox)][co] = relu(b3[co] + Σ_(ky,kx,ci) a2[oy+ky][ox+kx][ci] W3p[co][k]).
// One persistent block per CU walks images.  GEMM rows are the real outputs only
// (compact rows): 48 of the 49 in three row tiles of 16, tile row 16 t + r = output
// pixel c3_row_q[16 t + r] (below), and the 49th left to conv3_lone_tiles.  k-step =
// (tap, ci half), lane group g = 8-ci chunk; a lane's tap pixel is p0 + 9 ky + kx,
// p0 = 9 oy + ox its row's tap-(0, 0) input pixel.  Per image the LDS holds a2 split
// into three bf16 planes (84 pixel rows of 160 B; the last 3 are zero and never
// addressed by a real row): 2 stages x 40,320 B, the next image staged before the
// compute and the image after next fetched into registers at k-step 1.  Wave w: co
// tile w & 1, K half (w >> 1) & 1 (taps 0-4.5 / 4.5-8: 9 k-steps of 32, the weight
// fragments of its co tile and K half, 9 x 3 pre-split planes, in 108 VGPRs); with
// NT = 768 threads (the standalone launch, 3 waves per SIMD) row tile w >> 2, with
// NT = 512 (the fused trunk's third phase) row tiles 0-1 for waves 0-3 and tile 2
// for waves 4-7 — waves w and w + 4 share a SIMD, so each SIMD's matrix core runs 3
// tiles per image.  Operands: the activations split at staging (split8), the weights
// as packed planes; per k-step the part products in PPO_PRODUCTS order; K half 1
// hands its partial sums over through LDS and K half 0 adds them (kh 0 + kh 1), then
// bias and ReLU, in the swapped orientation (weights as the MFMA A operand): lane
// (i16, g) holds row 16 t + i16, channels 16 nt + 4g .. +3 — one 16-B store per tile.
// An output depends on its own row's operands only, so the results do not depend on
// the wave count or on which row an output sits in.  After its image loop the block
// computes the lone output of its own images (conv3_lone_tiles) in the same LDS.
constexpr int C3L_IR = 73;    // 16-B units per staged lone patch and plane (72 + pad)
constexpr int C3L_PL = 16 * C3L_IR;
constexpr int C3L_LDS = 2 * 3 * C3L_PL * 16 + 2 * 64 * 16;   // two 3-plane patch stages + K-half partials (114,176 B)
constexpr int C3C_LDS0 = 2 * 3 * 84 * 80 * 2 + 2 * 2 * 3 * 64 * 16;   // the image loop: stages + K-half partials (92,928 B)
constexpr int C3C_LDS = C3C_LDS0 > C3L_LDS ? C3C_LDS0 : C3L_LDS;   // the lone tiles after it reuse the LDS

// The compact rows: tile row 16 t + r computes output pixel q = c3_row_q[16 t + r]
// (q = 7 oy + ox); the 49th, C3_LONE_Q = 42 = (6, 0), is the lone output.  With
// 160-B pixel rows (16-B slot 10 p + c of input pixel p = 9 oy + ox + tap, chunk c) the
// 16 lanes of a ds_read_b128 group — rows {0-3, 12-15} at chunk c0 and rows {4-11} at
// c0 + 1, or the reverse — hit distinct slots for every tap iff each of those two row
// sets covers the 8 residues p mod 8 once: this table does that for all 3 tiles (the
// residue of (6, 6) would have left one set a duplicate, hence the lone (6, 0)); the
// oy-major order before it met 2-way conflicts in most groups (tools/conv3_bank_model.py)
constexpr int C3_LONE_Y = 6, C3_LONE_X = 0, C3_LONE_Q = 7 * C3_LONE_Y + C3_LONE_X;
__constant__ uint8_t c3_row_q[48] = {0,  1,  2,  3,  20, 7,  8,  9,  10, 11, 12, 19, 4,  5,  6,  13,
                                     26, 27, 14, 15, 32, 33, 34, 21, 22, 23, 24, 31, 16, 17, 18, 25,
                                     38, 39, 40, 41, 44, 45, 46, 47, 48, 35, 36, 43, 28, 29, 30, 37};

// ReLU mask bits of conv3's output (the training forward; read by the fc dgrad instead
// of the 411 MB fp32 activation): uint16 [B][49 pixels][2 channel tiles], bit j of word
// (p, t) = output channel 16 t + j of pixel p > 0.  Lane (g, i16) holds channels
// 16 t + 4 g + r (r < 4) of one pixel; lanes i16, i16 + 16, +32, +48 combine by two
// shuffles and lane g = 0 stores the word.
__device__ __forceinline__ void conv3_mask_store(const f32x4& y, int g, uint16_t* dst) {
  uint32_t w = ((y[0] > 0.f ? 1u : 0u) | (y[1] > 0.f ? 2u : 0u) | (y[2] > 0.f ? 4u : 0u) | (y[3] > 0.f ? 8u : 0u))
               << (4 * g);
  w |= (uint32_t)__shfl_xor((int)w, 16, 64);
  w |= (uint32_t)__shfl_xor((int)w, 32, 64);
  if (g == 0) *dst = (uint16_t)w;
}

// conv3 forward of the lone output C3_LONE_Q = 42 = (6, 0) for 16 images per tile: tiles t0, t0 + tstep, ...
// of the images base + stride * i (i < nimg; row i16 of the B operand is image base +
// stride * (16 t + i16)); the same operands, MFMA sequence, K-half sum and epilogue as
// the body below (bit-identical to a row of its tiles).  Waves 0-3 compute (co tile w & 1, K half w >> 1,
// their weight fragments bw), every thread of the NT stages.  As conv2's lone tiles,
// the tile's 16 patches (3 rows of 3 pixels x 64 channels, 768 contiguous bytes per
// row) are loaded once per block, the next tile's in registers during this tile's
// MFMAs, and staged in LDS (two stages, image rows padded by 16 B).
template <int NP, int NT>
__device__ __forceinline__ void conv3_lone_tiles(const float* __restrict__ a2, const bf16x8 (&bw)[9][3],
                                                 const float* __restrict__ bias, float* __restrict__ out,
                                                 uint8_t* __restrict__ lds, long long base, long long stride,
                                                 int nimg, int t0, int tstep, uint16_t* __restrict__ m3 = nullptr) {
  constexpr int KS = 9, M = C3_LONE_Q, IR = C3L_IR, PL = C3L_PL, NCH = 16 * 72, NPC = (NCH + NT - 1) / NT;
  uint4 (*const P)[3 * PL] = reinterpret_cast<uint4 (*)[3 * PL]>(lds);
  f32x4* const R = reinterpret_cast<f32x4*>(lds + 2 * 3 * PL * 16);
  const int tid = threadIdx.x, lane = tid & 63, i16 = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nt = wave & 1, kh = (wave >> 1) & 1;
  const int ntile = (nimg + 15) / 16;
  // chunk c = tid + NT j: image c / 72, 8-channel chunk u = c % 72 of its patch = tap
  // (3 ky + kx) * 8 + channel octet; a2 offset ((LY + ky) * 9 + LX) * 64 + (u % 24) * 8 for
  // the lone output (LY, LX) = (C3_LONE_Y, C3_LONE_X); split into the bf16 planes once
  // here, not by each computing wave at fragment read (as conv2_lone_tiles)
  f32x4 pc[NPC][2];
  auto fetch = [&](int T) {   // past the last tile / image: zeros, nothing loaded
#pragma unroll
    for (int j = 0; j < NPC; ++j) {
      const int c = tid + NT * j, im = c / 72, u = c - 72 * im, ky = u / 24, i = 16 * T + im;
      const bool live = c < NCH && T < ntile && i < nimg;
      const float* src = a2 + (size_t)(base + stride * (live ? i : 0)) * 5184 + ((C3_LONE_Y + ky) * 9 + C3_LONE_X) * 64 +
                         (u - 24 * ky) * 8;
      pc[j][0] = live ? *reinterpret_cast<const f32x4*>(src) : zero4();
      pc[j][1] = live ? *reinterpret_cast<const f32x4*>(src + 4) : zero4();
    }
  };
  auto put = [&](int st) {
#pragma unroll
    for (int j = 0; j < NPC; ++j) {
      const int c = tid + NT * j, im = c / 72;
      if (c < NCH) {
        const int o = im * IR + (c - 72 * im);
        Frag3 f;
        split8(pc[j][0], pc[j][1], f, false);
        P[st][o] = __builtin_bit_cast(uint4, f.h);
        P[st][PL + o] = __builtin_bit_cast(uint4, f.m);
        P[st][2 * PL + o] = __builtin_bit_cast(uint4, f.l);
      }
    }
  };
  fetch(t0);
  put(0);
  __syncthreads();
  int cur = 0;
  for (int T = t0; T < ntile; T += tstep) {
    fetch(T + tstep);
    const int i = 16 * T + i16;
    const long long b = base + stride * (long long)i;
    f32x4 acc = zero4();
    if (wave < 4) {
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const int ks = 9 * kh + s, tap = ks >> 1, c = 4 * (ks & 1) + g, o = i16 * IR + tap * 8 + c;
        Frag3 a;
        a.h = __builtin_bit_cast(bf16x8, P[cur][o]);
        a.m = __builtin_bit_cast(bf16x8, P[cur][PL + o]);
        a.l = __builtin_bit_cast(bf16x8, P[cur][2 * PL + o]);
        const Frag3 w = {bw[s][0], bw[s][1], bw[s][2]};
#define PPO_PART(X, Y) acc = mma(w.Y, a.X, acc);
        PPO_PRODUCTS(NP, PPO_PART)
#undef PPO_PART
      }
      if (kh == 1) R[nt * 64 + lane] = acc;
    }
    put(cur ^ 1);   // the stage read one tile ago (the last barrier retired its reads)
    __syncthreads();   // partials in R; stage cur ^ 1 complete
    if (wave < 2 && i < nimg) {   // kh == 0
      const f32x4 bv4 = *reinterpret_cast<const f32x4*>(bias + 16 * nt + 4 * g);
      const f32x4 v = acc + R[nt * 64 + lane];
      f32x4 y;
#pragma unroll
      for (int r = 0; r < 4; ++r) y[r] = fmaxf(v[r] + bv4[r], 0.f);
      *reinterpret_cast<f32x4*>(out + (size_t)b * (49 * 32) + M * 32 + 16 * nt + 4 * g) = y;
      // the four lanes of image i (g = 0..3) share its activity: the shuffles read live lanes
      if (m3) conv3_mask_store(y, g, m3 + (size_t)b * 98 + M * 2 + nt);
    }
    __syncthreads();   // R read before the next tile's partials
    cur ^= 1;
  }
}

template <int NP, int NT>
__device__ __forceinline__ void conv3_fwd_c3_body(const float* __restrict__ a2, int B,
                                                  const uint16_t* __restrict__ wpl, const float* __restrict__ bias,
                                                  float* __restrict__ out, uint8_t* __restrict__ lds,
                                                  uint16_t* __restrict__ m3 = nullptr) {
  static_assert(NT == 512 || NT == 768, "8 or 12 waves");
  // pixel rows of 80 bf16 (160 B, 16-B chunk c of pixel p at 16-B slot 10 p + c): the 16
  // lanes of a ds_read_b128 group read 16 pixels 9 oy + ox + tap that are not
  // consecutive; with this pitch and the c3_row_q order they hit distinct slots (128-B
  // rows with a chunk swizzle c ^ ((p >> 1) & 7) met up to 3-way conflicts: 55 % of the
  // LDS-active cycles, profiles/r06_s19_conv_fwd_sq.json; model in DESIGN §A.0)
  constexpr int NPX = 84, PR = 80, PL = NPX * PR, KS = 9, WN = 32 * 576, UNITS = 81 * 8,
                UPER = (UNITS + NT - 1) / NT;
  uint16_t (*const S)[3 * PL] = reinterpret_cast<uint16_t (*)[3 * PL]>(lds);
  f32x4 (*const R)[2][3][64] = reinterpret_cast<f32x4 (*)[2][3][64]>(lds + 2 * 3 * PL * 2);   // [stage][co tile][row tile][lane]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i16 = lane & 15, g = lane >> 4;
  const int nt = wave & 1, kh = (wave >> 1) & 1, co = 16 * nt + i16;
  bf16x8 bw[KS][3];
#pragma unroll
  for (int s = 0; s < KS; ++s)
#pragma unroll
    for (int p = 0; p < 3; ++p)
      bw[s][p] = *reinterpret_cast<const bf16x8*>(wpl + (size_t)p * WN + co * 576 + (9 * kh + s) * 32 + 8 * g);
  const f32x4 bv4 = *reinterpret_cast<const f32x4*>(bias + 16 * nt + 4 * g);
  wait_vm0();
  for (int i = tid; i < 2 * 3 * PL / 8; i += NT) reinterpret_cast<uint4*>(&S[0][0])[i] = uint4{0, 0, 0, 0};
  f32x4 stg[UPER][2];
  auto fetch = [&](int b) {   // a per-image buffer resource: units past the image read 0, no branch
    const auto ra = make_rsrc(a2 + (size_t)b * 5184, 5184 * 4);
#pragma unroll
    for (int j = 0; j < UPER; ++j) {
      const int u = tid + NT * j, off = u < UNITS ? 32 * u : 0x7fffffe0;
      stg[j][0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ra, off, 0, 0));
      stg[j][1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ra, off + 16, 0, 0));
    }
  };
  auto put = [&](int buf) {
#pragma unroll
    for (int j = 0; j < UPER; ++j) {
      const int u = tid + NT * j;
      if (u < UNITS) {
        const int p = u >> 3, off = p * PR + 8 * (u & 7);
        Frag3 f;
        split8(stg[j][0], stg[j][1], f, false);
        *reinterpret_cast<bf16x8*>(&S[buf][off]) = f.h;
        *reinterpret_cast<bf16x8*>(&S[buf][PL + off]) = f.m;
        *reinterpret_cast<bf16x8*>(&S[buf][2 * PL + off]) = f.l;
      }
    }
  };
  __syncthreads();   // the zeroed pad rows
  const int G = gridDim.x;
  int b = blockIdx.x, cur = 0;
  if (b < B) {
    fetch(b);
    put(0);
    fetch(b + G < B ? b + G : b);
  }
  __syncthreads();
  // row tiles of this wave: mt0 .. mt0 + ntl - 1; the k loop takes the count as a
  // compile-time constant (a run-time bound would issue the second tile's MFMAs on
  // every wave), the barriers stay outside the wave-dependent branch
  const int mt0 = NT == 768 ? (wave >> 2) : (wave < 4 ? 0 : 2);
  const int ntl = NT == 768 || wave >= 4 ? 1 : 2;
  int p0[2], q0[2];   // tap-(0, 0) input pixel and output pixel of this lane's row per tile
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int q = c3_row_q[mt0 + t < 3 ? 16 * (mt0 + t) + i16 : 0], oy = q / 7;   // (no tile 3: unused)
    q0[t] = q;
    p0[t] = 9 * oy + (q - 7 * oy);
  }
  for (; b < B; b += G) {
    put(cur ^ 1);   // unconditional (past the end: a copy of this image into the idle stage)
    const int bnn = b + 2 * G < B ? b + 2 * G : b;
    const uint16_t* Sc = S[cur];
    f32x4 acc[2] = {zero4(), zero4()};
    auto kloop = [&](auto ntc) __attribute__((always_inline)) {
      constexpr int NTL = decltype(ntc)::value;
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const int ks = 9 * kh + s, tap = ks >> 1, ky = tap / 3, kx = tap - 3 * ky, c = 4 * (ks & 1) + g;
        const Frag3 w = {bw[s][0], bw[s][1], bw[s][2]};
        Frag3 a[NTL];
#pragma unroll
        for (int t = 0; t < NTL; ++t) {
          const int p = p0[t] + 9 * ky + kx;
          const uint16_t* q = Sc + p * PR + 8 * c;
          a[t].h = *reinterpret_cast<const bf16x8*>(q);
          a[t].m = *reinterpret_cast<const bf16x8*>(q + PL);
          a[t].l = *reinterpret_cast<const bf16x8*>(q + 2 * PL);
        }
#define PPO_PART(X, Y) \
  _Pragma("unroll") for (int t = 0; t < NTL; ++t) acc[t] = mma(w.Y, a[t].X, acc[t]);
        PPO_PRODUCTS(NP, PPO_PART)
#undef PPO_PART
        if (s == 1) {
          fetch(bnn);
          __builtin_amdgcn_sched_barrier(0);   // the loads stay in their slot
        }
      }
    };
    if constexpr (NT == 768) kloop(std::integral_constant<int, 1>{});
    else if (wave < 4) kloop(std::integral_constant<int, 2>{});
    else kloop(std::integral_constant<int, 1>{});
    if (kh == 1) {
      R[cur][nt][mt0][lane] = acc[0];
      if (ntl == 2) R[cur][nt][mt0 + 1][lane] = acc[1];
    }
    __syncthreads();   // stage cur consumed, stage cur ^ 1 complete, partials in R[cur]
    if (kh == 0) {
      const auto rs = make_rsrc(out + (size_t)b * (49 * 32), 49 * 32 * 4);
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        if (t < ntl) {
          const f32x4 v = acc[t] + R[cur][nt][mt0 + t][lane];
          f32x4 y;
#pragma unroll
          for (int r = 0; r < 4; ++r) y[r] = fmaxf(v[r] + bv4[r], 0.f);
          bstore_f32x4(y, rs, 4 * (q0[t] * 32 + 16 * nt + 4 * g));
          if (m3) conv3_mask_store(y, g, m3 + (size_t)b * 98 + q0[t] * 2 + nt);
        }
      }
    }
    cur ^= 1;
  }
  // the lone output of this block's own images, 16 per tile
  __syncthreads();   // the last image's partials (R) are read
  const int blk = blockIdx.x;
  const int nimg = blk < B ? (B - 1 - blk) / G + 1 : 0;
  conv3_lone_tiles<NP, NT>(a2, bw, bias, out, lds, blk, G, nimg, 0, 1, m3);
}

}  // namespace
