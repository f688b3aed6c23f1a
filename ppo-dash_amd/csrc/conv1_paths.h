// conv1 launchers that live in a file of their own and are called from another,
// internal to libppo_hip.so (u8 / RGB rows, C = 4; argument meanings as the
// ppo_conv1_* entry points that route to them).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// conv1w.hip, from ppo_conv1_wgrad (conv1.hip): the k-split weight gradients,
// conv1_wgrad tune 8 (kw) and 9 / 10 (kw3 with nw = 4 / 8 waves)
int conv1_wgrad_kw(const float* dz1, const uint8_t* obs, const int64_t* idx, long long row0, int B, int Z,
                   float* slab, float* slab_bias, void* stream);
int conv1_wgrad_kw3(const float* dz1, const uint8_t* obs, const int64_t* idx, long long row0, int B, int Z,
                    float* slab, float* slab_bias, void* stream, int nw);

// rgbaff.hip, from ppo_conv1_fwd_rgb / ppo_conv1_wgrad_rgb (conv1f.hip): the affine fold
int conv1_fwd_rgb_affine(const uint8_t* frames, const int64_t* idx, long long row0, int B, const float* mean,
                         double stdv, const float* w1, const float* b1, float* out, uint32_t* mbits, void* stream);
int conv1_wgrad_rgb_affine(const float* dz1, const uint8_t* frames, const int64_t* idx, long long row0, int B,
                           const float* mean, double stdv, int Z, float* slab, float* slab_bias, void* stream);
