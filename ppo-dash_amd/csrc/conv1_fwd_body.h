// conv1_fwd_body.h — the image-resident conv1 forward body (u8 observations) and
// its LDS constants, for conv1_fwd_bf16x3_kernel (conv1.hip) and the first phase of
// trunk_fwd_kernel (trunk.hip).
#pragma once
#include "igemm_x9.h"

namespace {

constexpr int IMG = 84, IMG2 = 84 * 84;
// conv1 forward's LDS image stage: channel stride 7,104 bf16 = 3,552 dwords, which is
// 32 mod 64 (a ds_read_b64 lane's bank is its dword address mod 64), so that the two
// 16-lane halves of a 32-lane group, reading the same rows of channels c and c + 1,
// use complementary banks (see conv1_fwd_bf16x3_body)
constexpr int C1S = 7104;
static_assert(C1S >= IMG2 && (C1S / 2) % 64 == 32, "conv1 stage channel stride");

// conv1 forward on the bf16 matrix cores, exact (u8 observations, C = 4).
// A pixel u in 0..255 is exact in bf16 and W = W_hi + W_mid + W_lo exactly
// (split_bf16x3), so conv1 = Σ u·W_hi + Σ u·W_mid + Σ u·W_lo where every
// product is exact in fp32 and v_mfma_f32_16x16x32_bf16 accumulates in fp32:
// fp32 arithmetic (as exact per product as v_mfma_f32_*_f32), at 3 bf16 MFMAs
// per 16x16x32 block instead of 8 f32 16x16x4 MFMAs of twice the cycles.
// One persistent block (8 waves) per CU walks images: the image being computed
// sits in LDS as bf16 (4 channels at stride C1S: 56,832 B; two stages), the next
// image is in flight into registers and converted/stored behind the compute.  Wave w:
// output channels 16 * (w & 1) + [0, 16), row tiles {w >> 1, (w >> 1) + 4, ...}
// of 16 output pixels.  k-step s covers channels 2 (s >> 2) + {0, 1} and kernel
// rows 2 (s & 3) + {0, 1}; lane group g = lane >> 4 supplies channel
// 2 (s >> 2) + (g & 1), row 2 (s & 3) + (g >> 1), kx = j = 0..7 — 8 adjacent
// pixels, 16 bytes at an 8-byte-aligned address, read as two ds_read_b64.  Lanes
// 0-31 (g = 0, 1) then read the same rows of two channels C1S apart: each 16-lane
// half covers 32 consecutive dwords mod 64 (16 consecutive output pixels, also
// across an output-row wrap: 4 input rows = 168 dwords = 40 mod 64), the other
// half the complementary 32, so both reads are conflict-free at 2 LDS cycles.
// (Left to itself the compiler merges two 8-byte reads into one ds_read2_b64, 8 LDS
// cycles, MI355X_MICROARCH §LDS; the reads are volatile so that it does not.)
// NPW: weight parts summed (3: exact fp32 weights; 1: half-precision mode, bf16 weights)
// The body takes its LDS (img: two image stages) so that the fused rollout trunk
// (trunk_fwd_kernel) can run it as its first phase in a shared buffer.
template <int C, bool MASK, int NPW = 3>   // MASK: also write the ReLU mask bits (training forward)
__device__ __forceinline__ void conv1_fwd_bf16x3_body(const uint8_t* __restrict__ obs,
                                                      const int64_t* __restrict__ idx, long long row0, int B,
                                                      const float* __restrict__ w, const float* __restrict__ bias,
                                                      float* __restrict__ out, uint16_t* __restrict__ mbits,
                                                      uint16_t (*__restrict__ img)[C * C1S]) {
  constexpr int NPX = C * IMG2, CH = NPX / 16, K = C * 64, KS = K / 32, PER = (CH + 511) / 512;
  constexpr int CCH = IMG2 / 16;   // 16-pixel chunks per channel (441)
  static_assert(IMG2 % 16 == 0 && C % 2 == 0, "16-pixel chunks, channel pairs");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ct = wave & 1, rq = wave >> 1;
  const int i16 = lane & 15, g = lane >> 4;
  const int col = ct * 16 + i16;
  const float bv = bias[col];
  // this wave's weight fragments, split once per block: B[k][n] = W[n][k]
  bf16x8 wf[3][KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const int c = 2 * (s >> 2) + (g & 1), ky = 2 * (s & 3) + (g >> 1);
    const float* wp = w + (size_t)col * K + c * 64 + ky * 8;
    uint32_t h[8], m[8], l[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) split_bf16x3(wp[j], h[j], m[j], l[j]);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      wf[0][s][j] = __builtin_bit_cast(__bf16, (uint16_t)h[j]);
      wf[1][s][j] = __builtin_bit_cast(__bf16, (uint16_t)m[j]);
      wf[2][s][j] = __builtin_bit_cast(__bf16, (uint16_t)l[j]);
    }
  }
  uint4 stage[PER];
  auto fetch = [&](int b) {   // 16 u8 pixels per chunk -> registers
    const uint4* src = reinterpret_cast<const uint4*>(obs + obs_row(idx, row0, b) * (long long)NPX);
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int c = tid + 512 * j;
      if (c < CH) stage[j] = src[c];
    }
  };
  auto put = [&](int buf) {   // u8 -> bf16 (exact: the high half of the fp32 integer), 2 x 16 B stores
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int c = tid + 512 * j;
      if (c < CH) {
        const uint32_t v[4] = {stage[j].x, stage[j].y, stage[j].z, stage[j].w};
        uint32_t o[8];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4 f = to_f32x4(v[q]);
          o[2 * q] = __builtin_amdgcn_perm(__float_as_uint(f[1]), __float_as_uint(f[0]), 0x07060302u);
          o[2 * q + 1] = __builtin_amdgcn_perm(__float_as_uint(f[3]), __float_as_uint(f[2]), 0x07060302u);
        }
        const int ch = c / CCH;
        uint4* d = reinterpret_cast<uint4*>(img[buf] + ch * C1S + 16 * (c - ch * CCH));
        d[0] = uint4{o[0], o[1], o[2], o[3]};
        d[1] = uint4{o[4], o[5], o[6], o[7]};
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
  for (; b < B; b += G) {
    if (b + G < B) put(cur ^ 1);          // read two iterations ago; the last barrier retired it
    if (b + 2 * G < B) fetch(b + 2 * G);
    // the wave's row tiles rq + 4t: 7 for rq 0, 6 otherwise (25 per image), as a
    // compile-time count, so no MFMA is issued for a tile the wave does not own
    // (with a run-time bound the compiler issued them all and selected: 1,344
    // instead of 1,200 MFMAs per image)
    auto tiles = [&](auto ntc) __attribute__((always_inline)) {
      constexpr int NTL = decltype(ntc)::value;
      const uint16_t* I = img[cur];
      f32x4 acc[NTL];
#pragma unroll
      for (int t = 0; t < NTL; ++t) acc[t] = zero4();
      // this lane's patch origin per row tile (channel g & 1, row g >> 1)
      int pix[NTL];
#pragma unroll
      for (int t = 0; t < NTL; ++t) {
        const int row = (rq + 4 * t) * 16 + i16, oy = row / 20, ox = row - oy * 20;
        pix[t] = (g & 1) * C1S + (g >> 1) * IMG + oy * (4 * IMG) + ox * 4;
      }
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const uint16_t* Is = I + 2 * (s >> 2) * C1S + 2 * (s & 3) * IMG;
        bf16x8 a[NTL];
#pragma unroll
        for (int t = 0; t < NTL; ++t) {   // 8-B aligned: 4ox bf16; volatile: not merged into ds_read2_b64
          typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
          const volatile __attribute__((address_space(3))) u32x2* p2 =
              (const volatile __attribute__((address_space(3))) u32x2*)(Is + pix[t]);
          const u32x2 lo = p2[0], hi = p2[1];
          a[t] = __builtin_bit_cast(bf16x8, uint4{lo.x, lo.y, hi.x, hi.y});
        }
#pragma unroll
        for (int part = 0; part < NPW; ++part)
#pragma unroll
          for (int t = 0; t < NTL; ++t)
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[t], wf[part][s], acc[t], 0, 0, 0);
      }
      float* o = out + (size_t)b * (400 * 32) + col;
#pragma unroll
      for (int t = 0; t < NTL; ++t) {
          const int rt = rq + 4 * t;
          uint64_t bal[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float v = fmaxf(acc[t][r] * (1.0f / 255.0f) + bv, 0.f);
            o[(rt * 16 + 4 * g + r) * 32] = v;
            if constexpr (MASK) bal[r] = __builtin_amdgcn_ballot_w64(v > 0.f);
          }
          if constexpr (MASK) {   // ReLU mask bits: lane (g, i16) of ballot r -> pixel 16 rt + 4g + r,
            // channel 16 ct + i16; lane j < 16 stores pixel 16 rt + j's 16 bits (one store per tile)
            if (lane < 16) {
              const int r = lane & 3, gg = lane >> 2;
              const uint64_t bsel = r == 0 ? bal[0] : r == 1 ? bal[1] : r == 2 ? bal[2] : bal[3];
              mbits[((size_t)b * 400 + rt * 16 + lane) * 2 + ct] = (uint16_t)(bsel >> (16 * gg));
            }
          }
        }
    };
    if (rq == 0) tiles(std::integral_constant<int, 7>{});
    else tiles(std::integral_constant<int, 6>{});
    __syncthreads();   // every wave is done with img[cur]; img[cur ^ 1] is complete
    cur ^= 1;
  }
}

constexpr int C1F_LDS = 2 * 4 * C1S * 2;   // two image stages of C = 4 channels (113,664 B)

}  // namespace
