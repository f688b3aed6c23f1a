// Host helpers shared by the launchers of conv1.hip, conv2.hip, conv3.hip,
// trunk.hip and dense.hip.
#pragma once
#include "igemm.h"
#include "igemm_x9.h"
#include "small.h"

// bf16 planes of a packed segment of n floats (they follow it)
static inline const uint16_t* planes_of(const float* seg, long long n) {
  return reinterpret_cast<const uint16_t*>(seg + n);
}

// compute units of the current device (persistent-kernel grid size)
static inline int device_cus() {
  static int n_cu = 0;
  if (!n_cu) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
    n_cu = n;
  }
  return n_cu;
}

template <class P>
static inline void set_planes(P& p, const float* seg, long long n, int rows, int K) {
  p.bpl = planes_of(seg, n); p.bps = n; p.bld = K; p.bnr = rows;
}

// persistent image-resident grid: one block per CU (fewer for a small batch)
static inline unsigned img_grid(int B) {
  const int n_cu = device_cus();
  return (unsigned)(B < n_cu ? B : n_cu);
}

// chunks are multiples of 32 rows: whole k-tiles of both cores (BK 16 and 32)
static inline int wgrad_chunk(long long R, int Z) {
  long long kt = (R + 31) / 32;
  return (int)(((kt + Z - 1) / Z) * 32);
}

template <class P>
static void set_wgrad(P& p, const float* dz, int COUT, long long R, int Z, float* slab, float* slab_bias, int NW) {
  p.dz = dz; p.COUT = COUT; p.R = R; p.chunk = wgrad_chunk(R, Z); p.slab = slab; p.slab_bias = slab_bias; p.NW = NW;
}
