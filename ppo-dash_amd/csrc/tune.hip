// Run-time knobs (ppo_tune_set / ppo_tune_get): all knob state of the library and its
// only writer; the launchers read it through the accessors of tune.h.  Each knob
// selects between the default kernel and one kept alternative that a test or a
// documented A/B depends on; the superseded variants of rounds 1-4 live in git
// history, not in the library.
//   conv1_fwd    0: image-resident bf16x3 kernel (u8, C = 4); 9: the generic tile GEMM
//                (the path any other C takes), for A/B and its parity test
//   conv1_wgrad  9: k-split kernel with one wave per SIMD (conv1w.hip, default since
//                round 5); 10: its two-waves-per-SIMD form; 8: the round-4 k-split
//                kernel (8 waves, u8 image by LDS-DMA); 5: part-pipelined kernel (the
//                half-precision mode's, bf16 dz)
//   x9           1: fp32 GEMMs on the bf16 matrix cores (exact split, igemm_x9.h) where
//                they measured faster; 0: fp32 MFMA (igemm.h); 2: the split core everywhere
//   fc_splitk    K slices of the rollout-sized fc forward with a workspace (<= 1: unsplit)
//   rgb_aff      1: conv1 on raw RGB frames by the affine fold (rgbaff.hip); 0: bit-exact decode
//   fc_splitk_tile 1: the rollout's split-K fc on 128 x 128 tiles (4 waves of 32 x 128), 16-B
//                slab stores; 0: 128 x 64 tiles (8 waves of 16 x 64), 4-B stores
//   conv3_dgrad_group 1: ppo_conv3_dgrad_bits on 16-image tiles for B >= 16 (conv3.hip: only
//                valid taps are issued); 0: the per-image kernel everywhere
//   wgrad_pipe   1: the split-at-staging weight gradients (fc, GRU: igemm_x9s_kernel) stage the
//                next k-step inside the MFMA stream, per wave role, loads issued mid-step;
//                0: the plain loop (MFMAs, then split and store, then the barrier); same bits
#include "common.h"
#include "tune.h"

static const char* g_tune_names[TK_N] = {"conv1_fwd", "conv1_wgrad", "x9", "fc_splitk", "rgb_aff", "fc_splitk_tile",
                                       "conv3_dgrad_group", "wgrad_pipe"};
// fc_splitk 4 with 128 x 128 tiles: 0.050-0.052 vs 0.054-0.055 ms per 4,096-row act for 2
// slices of 128 x 64 tiles (profiles/r06_s7_fc_splitk_sweep.log)
static int g_tune[TK_N] = {0, 9, 1, 4, 1, 1, 1, 1};
// stagger: the image-resident kernels with two LDS stages let waves 4-7 stage the
// next image after their compute (conv2 / conv3 dgrad)
static int g_stagger = 2;   // bit 1 (conv2 dgrad deferred 16-B stores): measured best
// small_b: forwards of at most this many samples (images / linear rows) take the
// small-batch path of small.hip (an output element per thread or wave, fp32 FMA)
static int g_small_b = 4;
// split-product count of the bf16 matrix-core launches (igemm_x9.h PPO_PRODUCTS): 1 | 6 | 9
static int g_split_products = 6;
// heads_lds: the LDS-weight heads_train kernels (0: the register-weight kernels, A/B)
static int g_heads_lds = 1;

int tune_key(int k) { return g_tune[k]; }
int tune_products() { return g_split_products; }
int tune_stagger() { return g_stagger; }
int tune_small_b() { return g_small_b; }
bool tune_heads_lds() { return g_heads_lds != 0; }
bool tune_wgrad_pipe() { return g_tune[TK_WGRAD_PIPE] != 0; }

static bool tune_ok(int k, int v) {
  switch (k) {
    case TK_CONV1_FWD: return v == 0 || v == 9;
    case TK_CONV1_WGRAD: return v == 5 || v == 8 || v == 9 || v == 10;
    case TK_X9: return v >= 0 && v <= 2;
    case TK_FC_SPLITK: return v >= 0 && v <= 8;
    case TK_FC_SPLITK_TILE: return v == 0 || v == 1;
    default: return v == 0 || v == 1;
  }
}

PPO_API int ppo_tune_set(const char* key, int value) {
  if (strcmp(key, "heads_lds") == 0) {
    g_heads_lds = value;
    return 0;
  }
  if (strcmp(key, "small_b") == 0) {
    PPO_REQUIRE(value >= 0, "ppo_tune_set: small_b must be >= 0, got %d", value);
    g_small_b = value;
    return 0;
  }

  if (strcmp(key, "stagger") == 0) {
#ifndef PPO_DIAG
    // bits 0-3 are schedule switches (same results); bits >= 4 select the timing-
    // anatomy paths of diagnostic kernels (wrong results by design): -DPPO_DIAG only
    PPO_REQUIRE(value >= 0 && value < 16, "ppo_tune_set: stagger takes schedule bits 0..15, got %d "
                "(the anatomy bits need a -DPPO_DIAG build)", value);
#endif
    g_stagger = value;
    return 0;
  }
  if (strcmp(key, "products") == 0) {
    PPO_REQUIRE(value == 1 || value == 6 || value == 9, "ppo_tune_set: products must be 1, 6 or 9, got %d", value);
    g_split_products = value;
    return 0;
  }
  for (int i = 0; i < TK_N; ++i)
    if (strcmp(key, g_tune_names[i]) == 0) {
      PPO_REQUIRE(tune_ok(i, value), "ppo_tune_set: %s = %d is not a kept variant", key, value);
      g_tune[i] = value;
      return 0;
    }
  ppo_set_error("ppo_tune_set: unknown key %s", key);
  return PPO_EARG;
}

PPO_API int ppo_tune_get(const char* key) {
  if (strcmp(key, "heads_lds") == 0) return g_heads_lds;
  if (strcmp(key, "small_b") == 0) return g_small_b;
  if (strcmp(key, "stagger") == 0) return g_stagger;
  if (strcmp(key, "products") == 0) return g_split_products;
  for (int i = 0; i < TK_N; ++i)
    if (strcmp(key, g_tune_names[i]) == 0) return g_tune[i];
  return -1;
}
