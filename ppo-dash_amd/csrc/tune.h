// Run-time knobs (ppo_tune_set / ppo_tune_get): the state lives in tune.hip, the
// launchers of every other file read it through these accessors.
#pragma once

enum { TK_CONV1_FWD, TK_CONV1_WGRAD, TK_X9, TK_FC_SPLITK, TK_RGB_AFF, TK_FC_SPLITK_TILE,
       TK_CONV3_DGRAD_GROUP, TK_WGRAD_PIPE, TK_N };

int tune_key(int k);      // value of knob TK_*
int tune_products();      // split products per operand pair: 1, 6 or 9
int tune_stagger();       // schedule bits 0-3 (anatomy bits >= 4 in a -DPPO_DIAG build)
int tune_small_b();       // forwards of at most this many samples take small.hip
bool tune_heads_lds();    // the LDS-weight heads_train kernels (heads.hip, heads_gauss.hip)
bool tune_wgrad_pipe();   // the pipelined k loop of igemm_x9s_kernel (igemm_x9.h)
