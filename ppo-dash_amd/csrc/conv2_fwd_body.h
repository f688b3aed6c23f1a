// conv2_fwd_body.h — the image-resident conv2 forward body, its lone-pixel tiles
// and their LDS constants, for conv2_fwd_x9c_kernel / conv2_fwd_lone_kernel
// (conv2.hip) and the second phase of trunk_fwd_kernel (trunk.hip).
#pragma once
#include "igemm_x9.h"

namespace {

// LDS of the forward body (conv2_fwd_x9c_body, below the lone tiles it ends with)
constexpr int C2F_STG = 3 * 4 * 400, C2F_MT = 5;   // conv2 forward: bf16x8 units per stage, row tiles
// stages + the row tables vtab, otab ([MT][16] ints each, in a 768-B tail) (154,368 B)
constexpr int C2F_LDS = 2 * C2F_STG * 16 + 768;
static_assert(2 * C2F_MT * 16 * 4 <= 768, "row tables");

// conv2 forward of output pixel 72 = (8, 0) (phase-grid v = 80, the sixth row tile's
// only real row) for 16 images per tile.  The tile's 16 patches (a1 rows 16-19,
// columns 0-3: 4 x 512 contiguous bytes per image, 32 KB per tile) are loaded once per
// block — each thread four 16-B pieces, the next tile's in registers during this
// tile's MFMAs — and staged in LDS
// (two stages; image rows padded by 16 B so the 16 images of a fragment read hit
// distinct banks): loading them per wave moved each chunk four times through the
// L2, 107 vs 76 µs per 65,536 images (profiles/r05_zr_lone_anatomy.txt; two tiles
// of loads in flight measured no faster).  The same operands as conv2_fwd_x9c_body's
// (the same split8 of the same 8-channel chunks, the same weight planes), the same
// MFMA sequence per wave (k-steps of its K half in order, parts in PPO_PRODUCTS
// order), the K halves summed kh 0 + kh 1, the same epilogue: an MFMA output column
// depends only on its own B column, so the result does not depend on which images
// share a tile (test_trunk_fwd_equals_three_launches).
// Tiles t0, t0 + tstep, ... of the images base + stride * i (i < nimg, 16 per tile:
// row i16 of the B operand is image base + stride * (16 t + i16)).  The body below
// (LONE) runs it after its image loop over the block's own images (base = blockIdx.x,
// stride = the grid), conv2_fwd_lone_kernel over contiguous images.
// The patches are split into their bf16 planes once, while staged (each thread one
// 8-channel chunk of one image), not by every wave at fragment read (the 4 waves of
// a K half would split the same chunks: 7 split VALU per MFMA).
constexpr int C2L_IR = 65;    // 16-B units per staged image row and plane (64 + pad: the 16
                              // images of a fragment read hit distinct 16-B slots)
constexpr int C2L_PL = 16 * C2L_IR;   // units per plane
constexpr int C2L_LDS = 2 * 3 * C2L_PL * 16 + 4 * 64 * 16;   // two 3-plane stages + K-half partials (103,936 B)
static_assert(C2L_LDS <= C2F_LDS, "the lone tiles reuse the image loop's LDS");
template <int NP, bool MASK>
__device__ __forceinline__ void conv2_lone_tiles(const float* __restrict__ a1, const bf16x8 (&bw)[8][3],
                                                 const float* __restrict__ bias, float* __restrict__ out,
                                                 uint16_t* __restrict__ mbits, uint8_t* __restrict__ lds,
                                                 long long base, long long stride, int nimg, int t0, int tstep) {
  constexpr int KS = 8, M = 72, IR = C2L_IR, PL = C2L_PL;
  uint4 (*const P)[3 * PL] = reinterpret_cast<uint4 (*)[3 * PL]>(lds);
  f32x4* const R = reinterpret_cast<f32x4*>(lds + 2 * 3 * PL * 16);
  const int tid = threadIdx.x, lane = tid & 63, i16 = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nt = wave & 3, kh = wave >> 2;
  const int ntile = (nimg + 15) / 16;
  // chunk c = tid + 512 j (j < 2) of a tile: image c >> 6, 8-channel chunk u = c & 63 of
  // its patch = tap (4 ky + kx) * 4 + channel octet; a1 offset (16 + ky) * 640 + (u & 15) * 8
  f32x4 pc[2][2];
  auto fetch = [&](int T) {   // past the last tile / image: zeros, nothing loaded
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int c = tid + 512 * j, im = c >> 6, u = c & 63, i = 16 * T + im;
      const bool live = T < ntile && i < nimg;
      const float* src = a1 + (size_t)(base + stride * (live ? i : 0)) * 12800 + (16 + (u >> 4)) * 640 + (u & 15) * 8;
      pc[j][0] = live ? *reinterpret_cast<const f32x4*>(src) : zero4();
      pc[j][1] = live ? *reinterpret_cast<const f32x4*>(src + 4) : zero4();
    }
  };
  auto put = [&](int st) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int c = tid + 512 * j, o = (c >> 6) * IR + (c & 63);
      Frag3 f;
      split8(pc[j][0], pc[j][1], f, NP == 1);
      P[st][o] = __builtin_bit_cast(uint4, f.h);
      if constexpr (NP != 1) {
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
    const bool live = i < nimg;
    const long long b = base + stride * (long long)i;
    f32x4 acc = zero4();
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int o = i16 * IR + (8 * kh + s) * 4 + g;
      Frag3 a;
      a.h = __builtin_bit_cast(bf16x8, P[cur][o]);
      if constexpr (NP != 1) {
        a.m = __builtin_bit_cast(bf16x8, P[cur][PL + o]);
        a.l = __builtin_bit_cast(bf16x8, P[cur][2 * PL + o]);
      }
      const Frag3 w = {bw[s][0], bw[s][1], bw[s][2]};
#define PPO_PART(X, Y) acc = mma(w.Y, a.X, acc);
      PPO_PRODUCTS(NP, PPO_PART)
#undef PPO_PART
    }
    if (kh == 1) R[nt * 64 + lane] = acc;
    put(cur ^ 1);   // the stage read one tile ago (the last barrier retired its reads)
    __syncthreads();   // partials in R; stage cur ^ 1 complete
    if (kh == 0) {
      const f32x4 bv4 = *reinterpret_cast<const f32x4*>(bias + 16 * nt + 4 * g);
      const f32x4 v = acc + R[nt * 64 + lane];
      f32x4 y;
#pragma unroll
      for (int r = 0; r < 4; ++r) y[r] = fmaxf(v[r] + bv4[r], 0.f);
      if (live) *reinterpret_cast<f32x4*>(out + (size_t)b * (81 * 64) + M * 64 + 16 * nt + 4 * g) = y;
      if constexpr (MASK) {
        int nib = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) nib |= (y[r] > 0.f ? 1 : 0) << r;
        const int w16 = nib | (__shfl_down(nib, 16, 64) << 4) | (__shfl_down(nib, 32, 64) << 8) |
                        (__shfl_down(nib, 48, 64) << 12);
        if (g == 0 && live) mbits[((size_t)b * 81 + M) * 4 + nt] = (uint16_t)w16;
      }
    }
    __syncthreads();   // R read before the next tile's partials
    cur ^= 1;
  }
}

// conv2 forward, image-resident on the bf16 matrix cores (exact split, DESIGN.md
// §3), two LDS stages: a2[b][m][co] =
// relu(b2[co] + Σ_k im2col(a1)[m][k] W2p[co][k]), m = (oy, ox), k = (ky, kx, ci).
// One persistent block (8 waves) per CU walks images.  Wave w: n tile w & 3 (16
// co), taps 8 (w >> 2) .. +7 (ky rows 0-1 / 2-3), its weight fragments
// (pre-split planes) in registers; the two K halves are summed through LDS.  The
// next image's split is staged into the second stage *during* the current
// image's k-steps instead of in a phase of its own (the single-stage kernel this
// replaced, 1.98 ms per minibatch, and an LDS-DMA staged variant, 2.00 ms, were
// removed; this one is bit-identical to both).
//   * Compact parity layout, 400 16-B units per 8-channel chunk: pixel (y, x) at
//     P = 100 (2 (y & 1) + (x & 1)) + 10 (y >> 1) + (x >> 1), so tap (ky, kx) of
//     output pixel (oy, ox) reads v + toff(ky, kx), v = 10 oy + ox.  Row i of row
//     tile t is the t-th pixel (by v) with v ≡ i (mod 16) (≤ 6 per residue: 6
//     tiles; a missing one is a dummy row reading pixel v = i): the 16 lanes of
//     a ds_read_b128 group read 16 distinct residues, conflict-free.  That leaves
//     five real rows for a sixth tile (v = 80 .. 88: the sixth pixels of residues
//     0, 2, 4, 6, 8), which is not run: residues 9, 11, 13, 15 have four pixels, so
//     tile 4's rows 9, 11, 13, 15 take v = 82, 84, 86, 88 (a 2-way bank conflict in
//     that tile's reads) — MT = 5 row tiles — and v = 80 (output (8, 0)) is left to
//     conv2_lone_tiles, 16 images per tile.  Two stages x 3 planes x 4 chunks x 400
//     x 16 B = 153,600 B.
//   * The K-half partials (24,576 B) are handed over in the lo plane of the stage
//     the image has just left: kh 1 writes them after barrier A, kh 0 reads them
//     after barrier B; the next image's hi / mid parts are staged into that
//     stage's planes 0-1 during k-steps 0-3, its lo parts held in registers
//     until a mid-image barrier (after k-step 5) has retired the partial reads,
//     then written during k-steps 6-7.  The image after next is fetched into
//     registers one unit per k-step (1-4), each once its register has been staged.
//   * Epilogue in the swapped MFMA orientation (weights as A): one 16-B store of
//     four consecutive channels per tile, dummy rows dropped by buffer range.
// LONE: the lone pixel of the block's own images after its image loop (the fused
// trunk: one tile per block at the rollout's 16 images per block, no extra launch).
// The standalone forward leaves it to conv2_fwd_lone_kernel: that launch runs two
// 70-KB-LDS blocks per CU (16 waves) where the folded tiles run at the tail of one
// 8-wave block per CU, and measured faster (profiles/r06_d_lone_trunk_kbab.log).
template <int NP, bool MASK = false, bool LONE = false>
__device__ __forceinline__ void conv2_fwd_x9c_body(const float* __restrict__ a1, int B,
                                                   const uint16_t* __restrict__ wpl, const float* __restrict__ bias,
                                                   float* __restrict__ out, uint16_t* __restrict__ mbits,
                                                   uint8_t* __restrict__ lds) {
  constexpr int U = 400, PLN = 4 * U, STG = 3 * PLN, KS = 8, WN = 64 * 512, MT = C2F_MT;
  constexpr int UNITS = 4 * U, UPER = (UNITS + 511) / 512;   // 4 units per thread (the 4th: wave 0)
  static_assert(STG == C2F_STG, "stage size");
  bf16x8* const S = reinterpret_cast<bf16x8*>(lds);
  int (*const vtab)[16] = reinterpret_cast<int (*)[16]>(lds + 2 * STG * 16);
  int (*const otab)[16] = reinterpret_cast<int (*)[16]>(lds + 2 * STG * 16 + MT * 16 * 4);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i16 = lane & 15, g = lane >> 4;
  const int nt = wave & 3, kh = wave >> 2, co = 16 * nt + i16;
  if (tid < 16) {
    int t = 0;
    for (int v = tid; v <= 88; v += 16)
      if (v % 10 != 9 && t < MT) {
        vtab[t][tid] = v;
        otab[t][tid] = 9 * (v / 10) + v % 10;
        ++t;
      }
    if (t == 4) {   // residues 9, 11, 13, 15 (4 pixels each) take the sixth pixels
      // of residues 2, 4, 6, 8 (v = 82 .. 88; a 2-way bank conflict in tile 4's reads);
      // residue 0's (v = 80) is the lone pixel
      const int v = 82 + (tid - 9);
      vtab[4][tid] = v;
      otab[4][tid] = 9 * (v / 10) + v % 10;
      t = 5;
    }
    for (; t < MT; ++t) {
      vtab[t][tid] = tid;
      otab[t][tid] = -1;
    }
  }
  bf16x8 bw[KS][3];
#pragma unroll
  for (int s = 0; s < KS; ++s)
#pragma unroll
    for (int p = 0; p < 3; ++p)
      bw[s][p] = *reinterpret_cast<const bf16x8*>(wpl + (size_t)p * WN + co * 512 + (8 * kh + s) * 32 + 8 * g);
  const f32x4 bv4 = *reinterpret_cast<const f32x4*>(bias + 16 * nt + 4 * g);
  wait_vm0();
  // staging unit u = tid + 512 j: chunk c = (u >> 3) & 3 of the pixel at compact
  // position rho = 8 (u >> 5) + (u & 7): 8 consecutive lanes write 8 consecutive
  // units (conflict-free ds_write_b128) and 4 lanes read one pixel's 128-B line
  int usrc[UPER], udst[UPER];
#pragma unroll
  for (int j = 0; j < UPER; ++j) {
    const int u = min(tid + 512 * j, UNITS - 1), rho = 8 * (u >> 5) + (u & 7), c = (u >> 3) & 3;
    const int par = rho / 100, rem = rho - 100 * par, yh = rem / 10, xh = rem - 10 * yh;
    const int y = 2 * yh + (par >> 1), x = 2 * xh + (par & 1);
    usrc[j] = (y * 20 + x) * 8 + 2 * c;
    udst[j] = c * U + rho;
  }
  const bool has_last = tid + 512 * (UPER - 1) < UNITS;
  f32x4 stg[UPER][2];
  bf16x8 lo[UPER];
  auto fetch_unit = [&](int b, int j) {   // unconditional (the 4th unit of waves 1-7 reloads unit 1599)
    const f32x4* src = reinterpret_cast<const f32x4*>(a1 + (size_t)b * 12800);
    stg[j][0] = src[usrc[j]];
    stg[j][1] = src[usrc[j] + 1];
  };
  auto fetch = [&](int b) {
#pragma unroll
    for (int j = 0; j < UPER; ++j) fetch_unit(b, j);
  };
  auto put_hm = [&](int j, int st) {   // hi / mid parts now, lo part held
    Frag3 f;
    split8(stg[j][0], stg[j][1], f, NP == 1);
    lo[j] = f.l;
    if (j < UPER - 1 || has_last) {
      bf16x8* d = S + st * STG + udst[j];
      d[0] = f.h;
      if constexpr (NP > 1) d[PLN] = f.m;
    }
  };
  auto put_l = [&](int j, int st) {
    if constexpr (NP > 1)
      if (j < UPER - 1 || has_last) S[st * STG + 2 * PLN + udst[j]] = lo[j];
  };
  // block barrier that leaves the image prefetch in flight (__syncthreads' fence
  // would drain every outstanding load): LDS ops retired, compiler fence
  auto lds_barrier = []() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };
  __syncthreads();   // vtab / otab
  int vrow[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) vrow[t] = vtab[t][i16] + g * U;
  const int G = gridDim.x;
  int b = blockIdx.x, cur = 0;
  if (b < B) {
    fetch(b);
#pragma unroll
    for (int j = 0; j < UPER; ++j) {
      put_hm(j, 0);
      put_l(j, 0);
    }
    fetch(b + G < B ? b + G : b);
  }
  __syncthreads();
  for (; b < B; b += G) {
    // no branches in the k loop (a conditional load or stage write made the wait
    // counts unknown at the merge: vmcnt(0) at every staging step): past the
    // block's last image the staging re-reads / re-stages an image nothing uses
    const int bnn = b + 2 * G < B ? b + 2 * G : b;
    const bf16x8* Sc = S + cur * STG;
    f32x4 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = zero4();
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int tap = 8 * kh + s, ky = tap >> 2, kx = tap & 3;
      const int toff = 100 * (2 * (ky & 1) + (kx & 1)) + 10 * (ky >> 1) + (kx >> 1);
      const Frag3 w = {bw[s][0], bw[s][1], bw[s][2]};
#pragma unroll
      for (int t0 = 0; t0 < MT; t0 += 3) {
        Frag3 a[3];
#pragma unroll
        for (int u = 0; u < 3; ++u) {
          if (t0 + u >= MT) continue;
          const bf16x8* q = Sc + vrow[t0 + u] + toff;
          a[u].h = q[0];
          if constexpr (NP > 1) {
            a[u].m = q[PLN];
            a[u].l = q[2 * PLN];
          }
        }
#define PPO_PART(X, Y) \
  _Pragma("unroll") for (int u = 0; u < 3; ++u) if (t0 + u < MT) acc[t0 + u] = mma(w.Y, a[u].X, acc[t0 + u]);
        PPO_PRODUCTS(NP, PPO_PART)
#undef PPO_PART
      }
      if (s < UPER) put_hm(s, cur ^ 1);
      // the image after next, one unit per k-step as its registers free up (all
      // four at one k-step stalled every wave of the chip at the same time)
      if (s >= 1 && s <= UPER) fetch_unit(bnn, s - 1);
      if (s == 5) lds_barrier();   // mid-image: the previous image's partials (lo plane of stage cur ^ 1) are read
      if (s >= 6) {
#pragma unroll
        for (int j = 0; j < UPER; ++j)
          if ((j & 1) == s - 6) put_l(j, cur ^ 1);
      }
    }
    lds_barrier();   // A: stage cur consumed; stage cur ^ 1 complete
    f32x4* R = reinterpret_cast<f32x4*>(S + cur * STG + 2 * PLN);   // partials in the lo plane just left
    if (kh == 1) {
#pragma unroll
      for (int t = 0; t < MT; ++t) R[(nt * MT + t) * 64 + lane] = acc[t];
    }
    lds_barrier();   // B: partials in LDS
    if (kh == 0) {
      const auto rs = make_rsrc(out + (size_t)b * (81 * 64), 81 * 64 * 4);
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        const f32x4 v = acc[t] + R[(nt * MT + t) * 64 + lane];
        const int m = otab[t][i16];
        f32x4 y;
#pragma unroll
        for (int r = 0; r < 4; ++r) y[r] = fmaxf(v[r] + bv4[r], 0.f);
        bstore_f32x4(y, rs, m >= 0 ? 4 * (m * 64 + 16 * nt + 4 * g) : -1);
        if constexpr (MASK) {   // ReLU mask bits of pixel m, channels 16 nt .. +15: 4 lanes' nibbles
          int nib = 0;
#pragma unroll
          for (int r = 0; r < 4; ++r) nib |= (y[r] > 0.f ? 1 : 0) << r;
          const int w16 = nib | (__shfl_down(nib, 16, 64) << 4) | (__shfl_down(nib, 32, 64) << 8) |
                          (__shfl_down(nib, 48, 64) << 12);
          if (g == 0 && m >= 0) mbits[((size_t)b * 81 + m) * 4 + nt] = (uint16_t)w16;
        }
      }
    }
    cur ^= 1;
  }
  if constexpr (LONE) {
    // the lone pixel (output 72) of this block's own images, 16 per tile, after its
    // image loop (the weight fragments are the ones the image loop used)
    __syncthreads();   // the last image's K-half partials (in the LDS) are read
    const int blk = blockIdx.x;
    const int nimg = blk < B ? (B - 1 - blk) / G + 1 : 0;
    conv2_lone_tiles<NP, MASK>(a1, bw, bias, out, mbits, lds, blk, G, nimg, 0, 1);
  }
}

}  // namespace
