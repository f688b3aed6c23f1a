// GAIL discriminator (algo/gail.py): the fused minibatch update and the reward pass.
//
// Reference: algo/gail.py:12-111.  trunk = Linear(D, Hd) - Tanh - Linear(Hd, Hd) - Tanh -
// Linear(Hd, 1); per minibatch of B (policy, expert) row pairs
//   L = BCE(d_e, 1) + BCE(d_p, 0) + lambda mean_b (|dd/dx(x_m)|_2 - 1)^2,
//   x_m = alpha x_e + (1 - alpha) x_p
// and one Adam step; the reward of a row is its logit d (gail.py's log s - log(1 - s) in
// exact arithmetic), scaled by the running standard deviation of the discounted returns.
//
// Parameters and gradients are flat fp32 in trunk.parameters() order: W1 [Hd][D], b1 [Hd],
// W2 [Hd][Hd], b2 [Hd], w3 [Hd], b3 [1]; P = Hd D + Hd^2 + 3 Hd + 1.
//
// Train: one launch.  A block holds every parameter in LDS (rows padded to an odd stride:
// a lane reads W[j][k] by row j in the forward products and by column k in the transposed
// ones; an odd stride keeps both off shared banks) and takes TR row triplets (policy,
// expert, mixup).  All of its activations stay in LDS through the forward, the double
// backward of the penalty and the plain backward; it then writes its own sum of the row
// gradients, part_grad [P], and three loss sums.  fp32 VALU throughout: Hd = 100 and six
// rows per block are no MFMA shape.  Reduce: one launch sums the block partials in
// block order (in double), so neither result depends on a launch shape.  With grad_sumsq
// and clip_adam that is four launches per minibatch.
//
// Reward: one launch for all R rows (parameters in LDS, 64 rows per tile, four waves each
// owning a quarter of the hidden units), one single-block launch for the T-step returns
// recursion with its float64 running moments.  No cross-block waits anywhere.
#include "common.h"

namespace {

constexpr int GT = 256;               // threads per block, every kernel here
constexpr int TR = 2;                 // row triplets per train block (measured: 4 and 1 are 20 % and 9 % slower at B = 128)
constexpr int NR = 3 * TR;            // rows per train block: [policy | expert | mixup][TR]
constexpr int RW_ROWS = 64;           // rows per reward tile: one per lane
constexpr int RW_MAX_BLOCKS = 1024;
constexpr int LDS_BYTES = 160 * 1024;  // gfx950: 160 KB per CU

// LDS image of the parameters (floats): W1 [Hd][D1], b1, W2 [Hd][H1], b2, w3, b3
struct Lay {
  int D, Hd, D1, H1, w1, b1, w2, b2, w3, b3, n;
};
__host__ __device__ inline Lay make_lay(int D, int Hd) {
  Lay l;
  l.D = D, l.Hd = Hd, l.D1 = D | 1, l.H1 = Hd | 1;
  l.w1 = 0;
  l.b1 = l.w1 + Hd * l.D1;
  l.w2 = l.b1 + Hd;
  l.b2 = l.w2 + Hd * l.H1;
  l.w3 = l.b2 + Hd;
  l.b3 = l.w3 + Hd;
  l.n = l.b3 + 1;
  return l;
}
inline long long train_lds_floats(const Lay& l) {
  return (long long)l.n + (long long)NR * l.D1 + 4LL * NR * l.H1 + 7LL * TR * l.H1 + (long long)TR * l.D1 + NR +
         3 * TR;
}
inline long long reward_lds_floats(const Lay& l) {
  return (long long)l.n + (long long)RW_ROWS * l.D1 + (long long)RW_ROWS * l.H1 + 4 * RW_ROWS;
}

__device__ __forceinline__ void load_params(const float* __restrict__ p, float* __restrict__ s, const Lay& l) {
  const int D = l.D, Hd = l.Hd;
  for (int e = threadIdx.x; e < Hd * D; e += GT) s[l.w1 + (e / D) * l.D1 + e % D] = p[e];
  const float* q = p + Hd * D;
  for (int e = threadIdx.x; e < Hd; e += GT) s[l.b1 + e] = q[e];
  q += Hd;
  for (int e = threadIdx.x; e < Hd * Hd; e += GT) s[l.w2 + (e / Hd) * l.H1 + e % Hd] = q[e];
  q += Hd * Hd;
  for (int e = threadIdx.x; e < Hd; e += GT) s[l.b2 + e] = q[e];
  q += Hd;
  for (int e = threadIdx.x; e < Hd; e += GT) s[l.w3 + e] = q[e];
  q += Hd;
  if (threadIdx.x == 0) s[l.b3] = q[0];
}

// one element of a row (obs | vector_obs | action) of the storage planes
struct Planes {
  const float* obs;
  const float* vec;
  const float* act;
  int od, V, A;
};
__device__ __forceinline__ float plane_at(const Planes& pl, long long row, int i) {
  if (i < pl.od) return pl.obs[row * pl.od + i];
  i -= pl.od;
  if (i < pl.V) return pl.vec[row * pl.V + i];
  return pl.act[row * pl.A + (i - pl.V)];
}

__device__ __forceinline__ float sigmoidf(float z) {
  const float e = expf(-fabsf(z));
  return (z >= 0.0f ? 1.0f : e) / (1.0f + e);
}
// log(1 + exp(z)) = max(z, 0) + log1p(exp(-|z|))
__device__ __forceinline__ float softplusf(float z) { return fmaxf(z, 0.0f) + log1pf(expf(-fabsf(z))); }

struct TrainArgs {
  const float* params;
  Planes pl;
  const int64_t* idx;
  long long row0, rows;
  const float* expert;
  const float* alpha;
  int B;
  float lambda;
  float* part_grad;
  float* part_loss;
  Lay l;
};

// row r of a block: type r / TR (0 policy, 1 expert, 2 mixup), triplet r % TR.  A block
// with nv < TR triplets (the last one) computes 3 nv rows: item -> (type, t) -> r
#define GAIL_ROW(rr, nv) (((rr) / (nv)) * TR + (rr) % (nv))

__global__ __launch_bounds__(GT) void gail_train_kernel(const TrainArgs a) {
  extern __shared__ float sm[];
  const Lay l = a.l;
  const int D = l.D, Hd = l.Hd, D1 = l.D1, H1 = l.H1, tid = threadIdx.x;
  float* x = sm + l.n;           // [NR][D1]
  float* h1 = x + NR * D1;       // [NR][H1]
  float* h2 = h1 + NR * H1;
  float* p1 = h2 + NR * H1;      // dL/d(pre-activation 1)
  float* p2 = p1 + NR * H1;
  float* u2 = p2 + NR * H1;      // mixup rows, [TR][H1] each: s2 w3
  float* v1 = u2 + TR * H1;      // W2^T u2
  float* u1 = v1 + TR * H1;      // s1 v1
  float* vb1 = u1 + TR * H1;     // s1 (W1 gbar)
  float* su2 = vb1 + TR * H1;    // s2 (W2 vb1)
  float* hb1 = su2 + TR * H1;    // -2 h1 v1 (W1 gbar)
  float* hb2 = hb1 + TR * H1;    // -2 h2 w3 (W2 vb1)
  float* g = hb2 + TR * H1;      // [TR][D1]: dd/dx, then gbar
  float* c = g + TR * D1;        // [NR]: dL/dd
  float* ls = c + NR;            // [3][TR]: expert BCE, policy BCE, penalty per triplet
  const float* W1 = sm + l.w1;
  const float* b1 = sm + l.b1;
  const float* W2 = sm + l.w2;
  const float* b2 = sm + l.b2;
  const float* w3 = sm + l.w3;

  const int first = blockIdx.x * TR;
  const int nv = a.B - first < TR ? a.B - first : TR;   // >= 1 by the launch shape
  const int nrow = 3 * nv;
  const float inv_b = 1.0f / (float)a.B;

  load_params(a.params, sm, l);
  for (int e = tid; e < nv * D; e += GT) {
    const int t = e / D, i = e % D, b = first + t;
    long long src = a.idx ? (long long)a.idx[b] : a.row0 + b;
    src = src < 0 ? 0 : (src >= a.rows ? a.rows - 1 : src);   // never outside the planes
    const float xp = plane_at(a.pl, src, i);
    const float xe = a.expert[(long long)b * D + i];
    const float al = a.alpha[b];
    x[t * D1 + i] = xp;
    x[(TR + t) * D1 + i] = xe;
    x[(2 * TR + t) * D1 + i] = al * xe + (1.0f - al) * xp;
  }
  __syncthreads();

  // forward
  for (int it = tid; it < nrow * Hd; it += GT) {
    const int rr = it / Hd, j = it % Hd, r = GAIL_ROW(rr, nv);
    float acc = b1[j];
    for (int k = 0; k < D; ++k) acc += W1[j * D1 + k] * x[r * D1 + k];
    h1[r * H1 + j] = tanhf(acc);
  }
  __syncthreads();
  for (int it = tid; it < nrow * Hd; it += GT) {
    const int rr = it / Hd, j = it % Hd, r = GAIL_ROW(rr, nv);
    float acc = b2[j];
    for (int k = 0; k < Hd; ++k) acc += W2[j * H1 + k] * h1[r * H1 + k];
    h2[r * H1 + j] = tanhf(acc);
  }
  __syncthreads();
  // logits, BCE and dL/dd: one wave per row
  for (int rr = tid >> 6; rr < nrow; rr += GT / 64) {
    const int r = GAIL_ROW(rr, nv), type = rr / nv, t = rr % nv;
    float s = 0.0f;
    for (int j = tid & 63; j < Hd; j += 64) s += w3[j] * h2[r * H1 + j];
    s = wave_sum(s);
    if ((tid & 63) == 0) {
      const float d = s + sm[l.b3];
      if (type == 0) {          // policy: BCE(d, 0) = softplus(d)
        ls[TR + t] = softplusf(d);
        c[r] = sigmoidf(d) * inv_b;
      } else if (type == 1) {   // expert: BCE(d, 1) = softplus(-d)
        ls[t] = softplusf(-d);
        c[r] = -sigmoidf(-d) * inv_b;
      } else {
        c[r] = 0.0f;
      }
    }
  }
  // penalty, mixup rows m = 2 TR + t:  u2 = s2 w3
  for (int it = tid; it < nv * Hd; it += GT) {
    const int t = it / Hd, j = it % Hd;
    const float h = h2[(2 * TR + t) * H1 + j];
    u2[t * H1 + j] = (1.0f - h * h) * w3[j];
  }
  __syncthreads();
  // v1 = W2^T u2, u1 = s1 v1
  for (int it = tid; it < nv * Hd; it += GT) {
    const int t = it / Hd, k = it % Hd;
    float acc = 0.0f;
    for (int j = 0; j < Hd; ++j) acc += W2[j * H1 + k] * u2[t * H1 + j];
    const float h = h1[(2 * TR + t) * H1 + k];
    v1[t * H1 + k] = acc;
    u1[t * H1 + k] = (1.0f - h * h) * acc;
  }
  __syncthreads();
  // g = W1^T u1 = dd/dx
  for (int it = tid; it < nv * D; it += GT) {
    const int t = it / D, i = it % D;
    float acc = 0.0f;
    for (int k = 0; k < Hd; ++k) acc += W1[k * D1 + i] * u1[t * H1 + k];
    g[t * D1 + i] = acc;
  }
  __syncthreads();
  // n = |g|, gbar = lambda (2 / B) (n - 1) g / n: one wave per mixup row, in place
  for (int t = tid >> 6; t < nv; t += GT / 64) {
    float s = 0.0f;
    for (int i = tid & 63; i < D; i += 64) s += g[t * D1 + i] * g[t * D1 + i];
    s = wave_sum(s);
    const float n = sqrtf(s);
    const float coef = a.lambda * (2.0f * inv_b) * (n - 1.0f) / n;
    for (int i = tid & 63; i < D; i += 64) g[t * D1 + i] *= coef;
    if ((tid & 63) == 0) ls[2 * TR + t] = (n - 1.0f) * (n - 1.0f);
  }
  __syncthreads();
  // ub1 = W1 gbar; vb1 = s1 ub1; hb1 = -2 h1 v1 ub1
  for (int it = tid; it < nv * Hd; it += GT) {
    const int t = it / Hd, k = it % Hd;
    float acc = 0.0f;
    for (int i = 0; i < D; ++i) acc += W1[k * D1 + i] * g[t * D1 + i];
    const float h = h1[(2 * TR + t) * H1 + k];
    vb1[t * H1 + k] = (1.0f - h * h) * acc;
    hb1[t * H1 + k] = -2.0f * h * v1[t * H1 + k] * acc;
  }
  __syncthreads();
  // ub2 = W2 vb1; su2 = s2 ub2; hb2 = -2 h2 w3 ub2
  for (int it = tid; it < nv * Hd; it += GT) {
    const int t = it / Hd, j = it % Hd;
    float acc = 0.0f;
    for (int k = 0; k < Hd; ++k) acc += W2[j * H1 + k] * vb1[t * H1 + k];
    const float h = h2[(2 * TR + t) * H1 + j];
    su2[t * H1 + j] = (1.0f - h * h) * acc;
    hb2[t * H1 + j] = -2.0f * h * w3[j] * acc;
  }
  __syncthreads();
  // plain backward, every row: p2 = (c w3 + hb2) s2; p1 = (W2^T p2 + hb1) s1
  for (int it = tid; it < nrow * Hd; it += GT) {
    const int rr = it / Hd, j = it % Hd, r = GAIL_ROW(rr, nv);
    const float h = h2[r * H1 + j];
    const float hb = rr / nv == 2 ? hb2[(rr % nv) * H1 + j] : 0.0f;
    p2[r * H1 + j] = (c[r] * w3[j] + hb) * (1.0f - h * h);
  }
  __syncthreads();
  for (int it = tid; it < nrow * Hd; it += GT) {
    const int rr = it / Hd, k = it % Hd, r = GAIL_ROW(rr, nv);
    float acc = 0.0f;
    for (int j = 0; j < Hd; ++j) acc += W2[j * H1 + k] * p2[r * H1 + j];
    const float h = h1[r * H1 + k];
    const float hb = rr / nv == 2 ? hb1[(rr % nv) * H1 + k] : 0.0f;
    p1[r * H1 + k] = (acc + hb) * (1.0f - h * h);
  }
  __syncthreads();

  // this block's gradient: rows in (type, t) order, then the penalty's direct terms
  float* out = a.part_grad + (long long)blockIdx.x * (Hd * D + Hd * Hd + 3 * Hd + 1);
  const int o_b1 = Hd * D, o_w2 = o_b1 + Hd, o_b2 = o_w2 + Hd * Hd, o_w3 = o_b2 + Hd, o_b3 = o_w3 + Hd;
  for (int e = tid; e <= o_b3; e += GT) {
    float s = 0.0f;
    if (e < o_b1) {
      const int k = e / D, i = e % D;
      for (int rr = 0; rr < nrow; ++rr) {
        const int r = GAIL_ROW(rr, nv);
        s += p1[r * H1 + k] * x[r * D1 + i];
      }
      for (int t = 0; t < nv; ++t) s += u1[t * H1 + k] * g[t * D1 + i];
    } else if (e < o_w2) {
      const int k = e - o_b1;
      for (int rr = 0; rr < nrow; ++rr) s += p1[GAIL_ROW(rr, nv) * H1 + k];
    } else if (e < o_b2) {
      const int j = (e - o_w2) / Hd, k = (e - o_w2) % Hd;
      for (int rr = 0; rr < nrow; ++rr) {
        const int r = GAIL_ROW(rr, nv);
        s += p2[r * H1 + j] * h1[r * H1 + k];
      }
      for (int t = 0; t < nv; ++t) s += u2[t * H1 + j] * vb1[t * H1 + k];
    } else if (e < o_w3) {
      const int j = e - o_b2;
      for (int rr = 0; rr < nrow; ++rr) s += p2[GAIL_ROW(rr, nv) * H1 + j];
    } else if (e < o_b3) {
      const int j = e - o_w3;
      for (int rr = 0; rr < nrow; ++rr) {
        const int r = GAIL_ROW(rr, nv);
        s += c[r] * h2[r * H1 + j];
      }
      for (int t = 0; t < nv; ++t) s += su2[t * H1 + j];
    } else {
      for (int rr = 0; rr < nrow; ++rr) s += c[GAIL_ROW(rr, nv)];
    }
    out[e] = s;
  }
  if (tid < 3) {
    float s = 0.0f;
    for (int t = 0; t < nv; ++t) s += ls[tid * TR + t];
    a.part_loss[blockIdx.x * 3 + tid] = s;
  }
}

// grad[p] = sum over blocks, in block order, in double: one thread per element, so the
// sum does not depend on this launch's shape.  Thread 0 does the same for the three
// loss sums and adds the minibatch's L to loss_acc[0]; [1..3] = this minibatch's sums.
__global__ __launch_bounds__(GT) void gail_reduce_kernel(const float* __restrict__ part_grad,
                                                        const float* __restrict__ part_loss, int nblk, int P, int B,
                                                        float lambda, float* __restrict__ grad,
                                                        double* __restrict__ loss_acc) {
  const int e = blockIdx.x * GT + threadIdx.x;
  if (e < P) {
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += (double)part_grad[(long long)b * P + e];
    grad[e] = (float)s;
  }
  if (e == 0) {
    double s[3] = {0.0, 0.0, 0.0};
    for (int b = 0; b < nblk; ++b)
      for (int q = 0; q < 3; ++q) s[q] += (double)part_loss[b * 3 + q];
    loss_acc[0] += (s[0] + s[1] + (double)lambda * s[2]) / (double)B;
    loss_acc[1] = s[0], loss_acc[2] = s[1], loss_acc[3] = s[2];
  }
}

// d of rows row0 .. row0 + R: thread (wave q, lane) = (quarter of the hidden units, row of
// the tile).  A wave's weight reads are one address for all lanes; its activation reads
// are one row per lane at an odd stride.  d = (((part_0 + part_1) + part_2) + part_3) + b3.
struct RewardArgs {
  const float* params;
  Planes pl;
  long long row0, R;
  float* out;
  Lay l;
};

__device__ __forceinline__ void reward_layer(const float* __restrict__ W, int ws, const float* __restrict__ bias,
                                             const float* __restrict__ src, int K, int j0, int j1, float* dst_h,
                                             const float* __restrict__ w3, float& dsum) {
  int j = j0;
  for (; j + 4 <= j1; j += 4) {
    float a0 = bias[j], a1 = bias[j + 1], a2 = bias[j + 2], a3 = bias[j + 3];
    const float* w = W + j * ws;
    for (int k = 0; k < K; ++k) {
      const float v = src[k];
      a0 += w[k] * v;
      a1 += w[ws + k] * v;
      a2 += w[2 * ws + k] * v;
      a3 += w[3 * ws + k] * v;
    }
    a0 = tanhf(a0), a1 = tanhf(a1), a2 = tanhf(a2), a3 = tanhf(a3);
    if (dst_h) {
      dst_h[j] = a0, dst_h[j + 1] = a1, dst_h[j + 2] = a2, dst_h[j + 3] = a3;
    } else {
      dsum += w3[j] * a0;
      dsum += w3[j + 1] * a1;
      dsum += w3[j + 2] * a2;
      dsum += w3[j + 3] * a3;
    }
  }
  for (; j < j1; ++j) {
    float a0 = bias[j];
    const float* w = W + j * ws;
    for (int k = 0; k < K; ++k) a0 += w[k] * src[k];
    a0 = tanhf(a0);
    if (dst_h)
      dst_h[j] = a0;
    else
      dsum += w3[j] * a0;
  }
}

__global__ __launch_bounds__(GT) void gail_reward_kernel(const RewardArgs a) {
  extern __shared__ float sm[];
  const Lay l = a.l;
  const int D = l.D, Hd = l.Hd, D1 = l.D1, H1 = l.H1, tid = threadIdx.x;
  float* xs = sm + l.n;               // [64][D1]
  float* hs = xs + RW_ROWS * D1;      // [64][H1]
  float* dp = hs + RW_ROWS * H1;      // [4][64]
  const int q = tid >> 6, lane = tid & 63, nj = Hd / 4;   // Hd % 4 == 0
  load_params(a.params, sm, l);
  const long long tiles = (a.R + RW_ROWS - 1) / RW_ROWS;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long long base = tile * RW_ROWS;
    __syncthreads();   // the parameters (first tile); the previous tile's xs / hs / dp reads
    for (int e = tid; e < RW_ROWS * D; e += GT) {
      const int row = e / D, i = e % D;
      xs[row * D1 + i] = base + row < a.R ? plane_at(a.pl, a.row0 + base + row, i) : 0.0f;
    }
    __syncthreads();
    float unused = 0.0f;
    reward_layer(sm + l.w1, D1, sm + l.b1, xs + lane * D1, D, q * nj, (q + 1) * nj, hs + lane * H1, nullptr,
                    unused);
    __syncthreads();
    float dsum = 0.0f;
    reward_layer(sm + l.w2, H1, sm + l.b2, hs + lane * H1, Hd, q * nj, (q + 1) * nj, nullptr, sm + l.w3, dsum);
    dp[q * RW_ROWS + lane] = dsum;
    __syncthreads();
    if (tid < RW_ROWS && base + tid < a.R)
      a.out[base + tid] = (((dp[tid] + dp[RW_ROWS + tid]) + dp[2 * RW_ROWS + tid]) + dp[3 * RW_ROWS + tid]) + sm[l.b3];
  }
}

// ret = (ret mask) gamma + r, one fp32 rounding per operation (gail.py:108 in torch)
__device__ __forceinline__ float returns_step(float ret, float mask, float gamma, float r) {
#pragma clang fp contract(off)
  float v = ret * mask;
  v = v * gamma;
  v = v + r;
  return v;
}

// baselines' update_mean_var_count_from_moments in float64, in its operation order
__device__ __forceinline__ void rms_merge(double& mean, double& var, double& count, double bmean, double bvar,
                                          double bcount) {
#pragma clang fp contract(off)
  const double delta = bmean - mean;
  const double tot = count + bcount;
  const double new_mean = mean + delta * bcount / tot;
  const double m_a = var * count;
  const double m_b = bvar * bcount;
  const double m2 = m_a + m_b + delta * delta * count * bcount / tot;
  mean = new_mean;
  var = m2 / tot;
  count = tot;
}

// every thread gets the sum: lane-strided partials, xor-butterfly per wave, the four wave
// sums in wave order.  One block of GT threads always, so the order is a function of N alone.
__device__ __forceinline__ double block_sum_d(double s, double* red) {
  s = wave_sum_d(s);
  __syncthreads();   // red's previous readers
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(GT) void gail_returns_kernel(float* __restrict__ r, const float* __restrict__ masks,
                                                         float* __restrict__ ret, double* __restrict__ rms, int T,
                                                         int N, float gamma, int update) {
  __shared__ double red[GT / 64];
  const int tid = threadIdx.x;
  double mean = rms[0], var = rms[1], count = rms[2];
  for (int t = 0; t < T; ++t) {
    float* rt = r + (long long)t * N;
    if (update) {
      const float* mt = masks + (long long)t * N;
      double s = 0.0;
      for (int n = tid; n < N; n += GT) {
        const float v = returns_step(ret[n], mt[n], gamma, rt[n]);
        ret[n] = v;
        s += (double)v;
      }
      const double bmean = block_sum_d(s, red) / (double)N;
      double s2 = 0.0;
      for (int n = tid; n < N; n += GT) {   // ret[n]: this thread's own store
        const double dl = (double)ret[n] - bmean;
        s2 += dl * dl;
      }
      const double bvar = block_sum_d(s2, red) / (double)N;
      rms_merge(mean, var, count, bmean, bvar, (double)N);   // the same in every thread
    }
    const float sc = (float)sqrt(var + 1e-8);
    for (int n = tid; n < N; n += GT) rt[n] = rt[n] / sc;
  }
  if (update && tid == 0) rms[0] = mean, rms[1] = var, rms[2] = count;
}

int check_dims(const char* who, int D, int Hd, long long lds_floats) {
  PPO_REQUIRE(Hd >= 4 && Hd <= 128 && Hd % 4 == 0, "%s: Hd=%d (a multiple of 4 in [4, 128])", who, Hd);
  PPO_REQUIRE(D >= 2, "%s: D=%d (>= 2)", who, D);
  PPO_REQUIRE(lds_floats * 4 <= LDS_BYTES, "%s: D=%d Hd=%d needs %lld bytes of LDS (%d fit)", who, D, Hd,
              lds_floats * 4, LDS_BYTES);
  return 0;
}

template <typename K>
int allow_lds(K kernel, int bytes, int* granted, const char* name) {
  if (bytes > *granted) {
    PPO_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      bytes),
                  name);
    *granted = bytes;
  }
  return 0;
}

}  // namespace

PPO_API int ppo_gail_train_blocks(int B) { return B < 1 ? 0 : (B + TR - 1) / TR; }

// the larger LDS footprint of the two kernels that hold the parameters, in bytes (host only)
PPO_API long long ppo_gail_lds_bytes(int D, int Hd) {
  if (D < 2 || Hd < 4 || Hd > 128) return -1;
  const Lay l = make_lay(D, Hd);
  const long long a = train_lds_floats(l), b = reward_lds_floats(l);
  return 4 * (a > b ? a : b);
}

PPO_API int ppo_gail_train(const float* params, int D, int Hd, int B, const float* obs, int obs_dim,
                           const float* vector_obs, int V, const float* actions, int A, long long rows,
                           const int64_t* idx, long long row0, const float* expert, const float* alpha, float lambda,
                           float* part_grad, float* part_loss, void* stream) {
  const Lay l = make_lay(D, Hd);
  if (int rc = check_dims("ppo_gail_train", D, Hd, train_lds_floats(l))) return rc;
  PPO_REQUIRE(B >= 1, "ppo_gail_train: B=%d", B);
  PPO_REQUIRE(obs_dim >= 1 && V >= 0 && A >= 1 && obs_dim + V + A == D,
              "ppo_gail_train: obs_dim=%d + V=%d + A=%d != D=%d", obs_dim, V, A, D);
  PPO_REQUIRE(params && obs && actions && (V == 0 || vector_obs) && expert && alpha && part_grad && part_loss,
              "ppo_gail_train: NULL pointer");
  PPO_REQUIRE(rows >= 1 && (idx || (row0 >= 0 && row0 + B <= rows)), "ppo_gail_train: rows=%lld row0=%lld B=%d", rows,
              row0, B);
  static int granted = 0;
  const int bytes = (int)(train_lds_floats(l) * 4);
  if (int rc = allow_lds(gail_train_kernel, bytes, &granted, "ppo_gail_train")) return rc;
  TrainArgs a{params, {obs, vector_obs, actions, obs_dim, V, A}, idx, row0, rows, expert, alpha, B, lambda,
              part_grad, part_loss, l};
  ProfScope prof("gail_train", as_stream(stream), 0.0);
  gail_train_kernel<<<ppo_gail_train_blocks(B), GT, bytes, as_stream(stream)>>>(a);
  PPO_LAUNCH_CHECK("gail_train_kernel");
  return 0;
}

PPO_API int ppo_gail_reduce(const float* part_grad, const float* part_loss, int nblk, int P, int B, float lambda,
                            float* grad, double* loss_acc, void* stream) {
  PPO_REQUIRE(nblk >= 1 && P >= 1 && B >= 1, "ppo_gail_reduce: nblk=%d P=%d B=%d", nblk, P, B);
  PPO_REQUIRE(part_grad && part_loss && grad && loss_acc, "ppo_gail_reduce: NULL pointer");
  ProfScope prof("gail_reduce", as_stream(stream), 0.0);
  gail_reduce_kernel<<<ceil_div(P, GT), GT, 0, as_stream(stream)>>>(part_grad, part_loss, nblk, P, B, lambda, grad,
                                                                     loss_acc);
  PPO_LAUNCH_CHECK("gail_reduce_kernel");
  return 0;
}

PPO_API int ppo_gail_reward(const float* params, int D, int Hd, const float* obs, int obs_dim, const float* vector_obs,
                            int V, const float* actions, int A, long long row0, long long R, float* out,
                            void* stream) {
  const Lay l = make_lay(D, Hd);
  if (int rc = check_dims("ppo_gail_reward", D, Hd, reward_lds_floats(l)))
    return rc;
  PPO_REQUIRE(R >= 1 && row0 >= 0, "ppo_gail_reward: R=%lld row0=%lld", R, row0);
  PPO_REQUIRE(obs_dim >= 1 && V >= 0 && A >= 1 && obs_dim + V + A == D,
              "ppo_gail_reward: obs_dim=%d + V=%d + A=%d != D=%d", obs_dim, V, A, D);
  PPO_REQUIRE(params && obs && actions && (V == 0 || vector_obs) && out, "ppo_gail_reward: NULL pointer");
  static int granted = 0;
  const int bytes = (int)(reward_lds_floats(l) * 4);
  if (int rc = allow_lds(gail_reward_kernel, bytes, &granted, "ppo_gail_reward")) return rc;
  RewardArgs a{params, {obs, vector_obs, actions, obs_dim, V, A}, row0, R, out, l};
  const long long tiles = (R + RW_ROWS - 1) / RW_ROWS;
  ProfScope prof("gail_reward", as_stream(stream), 2.0 * R * ((double)D * Hd + (double)Hd * Hd + Hd));
  gail_reward_kernel<<<(unsigned)(tiles < RW_MAX_BLOCKS ? tiles : RW_MAX_BLOCKS), GT, bytes, as_stream(stream)>>>(a);
  PPO_LAUNCH_CHECK("gail_reward_kernel");
  return 0;
}

PPO_API int ppo_gail_returns(float* r, const float* masks, float* ret, double* rms, int T, int N, double gamma,
                             int update_rms, void* stream) {
  PPO_REQUIRE(T >= 1 && N >= 1, "ppo_gail_returns: T=%d N=%d", T, N);
  PPO_REQUIRE(r && masks && ret && rms, "ppo_gail_returns: NULL pointer");
  ProfScope prof("gail_returns", as_stream(stream), 0.0);
  gail_returns_kernel<<<1, GT, 0, as_stream(stream)>>>(r, masks, ret, rms, T, N, (float)gamma, update_rms ? 1 : 0);
  PPO_LAUNCH_CHECK("gail_returns_kernel");
  return 0;
}
