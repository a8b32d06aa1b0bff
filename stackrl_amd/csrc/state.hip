// state.hip — an env's persistent state as one record, gathered from and scattered to the handle's arrays on the device.
//
// What a step leaves behind for the next one is, per env: its EnvHdr (episode machine, RNG counter, goal, reward memory,
// episode list, script), its BLOB words of DevParams::blob (poses, velocities, manifolds, colouring), its height map
// DevParams::H (settle.hip reads it to release the next rock) and the staged render records of its rocks (stage.h: made in
// the settle kernel's tail, read by srl_k_render).  A state record is those four parts as 32-bit words, one after the other,
// each starting on a multiple of 4 words (srl_state_layout), so that everything moves as 16-byte vectors.  The randomness is
// counter based (settle.hip: key = seed + env_index_offset + env, counter = EnvHdr::episode), so the words are the whole
// state: nothing here computes, and a record written back continues bit for bit.
//
// srl_k_state_get gathers the records of envs idx[0 .. n) into a contiguous [n][words] buffer; srl_k_state_set writes record
// src[i] into env dst[i] (a record may go to several envs: a fork; the destinations are distinct, the caller sees to that).
// Grid: x = (env, record) pairs, y = chunks of a record; a thread moves one uint4 per round and both dimensions stride, so
// the host sizes the grid for a bandwidth kernel (SRL_STATE_BLOCKS workgroups of 256 threads) whatever the batch.  An env
// index outside the handle is skipped and reported through DevParams::flags (SRL_FLAG_STATE_INDEX -> srl_sync_status).
#pragma once
#include "srl_kernels.h"

#define SRL_STATE_THREADS 256
// workgroups per launch, about: 16 per CU.  Measured (profiles/state_lookahead.txt): 4,096 moves 4,096 x 16-rock records 4 %
// sooner than 2,048 and as fast as 8,192, and 1,024 x 8-rock records alike; two or four loads in flight per thread are slower
#define SRL_STATE_BLOCKS 4096
#define SRL_FLAG_STATE_INDEX 8   // DevParams::flags bit: a state export was given an env index outside the handle

static_assert(sizeof(EnvHdr) % 16 == 0, "the env header moves as 16-byte vectors: its words are their own padding");

// the four parts in the handle's arrays, sizes in uint4s per env (by value: 64 bytes)
struct StateParts {
  uint4* hdr;       // DevParams::hdr
  uint4* blob;      // DevParams::blob
  uint4* H;         // DevParams::H
  uint4* stage;     // srl_env::d_stage
  int32_t* flags;   // DevParams::flags
  int32_t q_hdr, q_blob, q_H, q_stage;   // uint4s per env of each part; the record has their sum
  int32_t n_envs;
};

// where uint4 q of env e's record lives in the handle's arrays
__device__ __forceinline__ uint4* state_word(const StateParts& S, int e, int q) {
  if (q < S.q_hdr) return S.hdr + (size_t)e * S.q_hdr + q;
  q -= S.q_hdr;
  if (q < S.q_blob) return S.blob + (size_t)e * S.q_blob + q;
  q -= S.q_blob;
  if (q < S.q_H) return S.H + (size_t)e * S.q_H + q;
  q -= S.q_H;
  return S.stage + (size_t)e * S.q_stage + q;
}

template <bool SET>
__device__ __forceinline__ void state_body(const StateParts& S, const int32_t* __restrict__ env_idx, const int32_t* __restrict__ rec_idx,
                                           int n, uint4* __restrict__ records) {
  const int q_rec = S.q_hdr + S.q_blob + S.q_H + S.q_stage;
  for (int i = blockIdx.x; i < n; i += gridDim.x) {
    const int e = env_idx ? env_idx[i] : i;
    const int r = rec_idx ? rec_idx[i] : i;
    if ((unsigned)e >= (unsigned)S.n_envs || r < 0) {
      if (threadIdx.x == 0 && blockIdx.y == 0) atomicOr(S.flags, SRL_FLAG_STATE_INDEX);
      continue;
    }
    uint4* rec = records + (size_t)r * q_rec;
    for (int q = blockIdx.y * SRL_STATE_THREADS + threadIdx.x; q < q_rec; q += gridDim.y * SRL_STATE_THREADS) {
      if (SET) *state_word(S, e, q) = rec[q];
      else rec[q] = *state_word(S, e, q);
    }
  }
}

extern "C" __global__ void __launch_bounds__(SRL_STATE_THREADS) srl_k_state_get(StateParts S, const int32_t* __restrict__ idx, int n,
                                                                                 uint4* __restrict__ records) {
  state_body<false>(S, idx, nullptr, n, records);
}
extern "C" __global__ void __launch_bounds__(SRL_STATE_THREADS) srl_k_state_set(StateParts S, const int32_t* __restrict__ dst,
                                                                                 const int32_t* __restrict__ src, int n,
                                                                                 uint4* __restrict__ records) {
  state_body<true>(S, dst, src, n, records);
}
