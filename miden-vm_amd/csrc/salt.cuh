// Hiding LMCS (mh_ctx_set_salt): the salt rows of a tree, generated where they are needed and never stored.
//
// The reference's HidingLmcsConfig (crates/lifted-stark/src/lmcs/hiding_config.rs) draws a random matrix of SALT_ELEMS columns and tree
// height and absorbs it after every other matrix (lifted_tree.rs:233-245, absorb_matrix).  Here the matrix is a PRF of the context's
// secret seed: the salt row of PHYSICAL (bit-reversed, lifted_tree.rs:300-306) leaf row i of the t-th salted tree of the context is
// lanes 0 .. n-1 of ONE Poseidon2 permutation of
//     [i, t, 0x53414c54 ("SALT"), 0, 0, 0, 0, 0, seed0, seed1, seed2, seed3]           (the key sits in the capacity lanes)
// whichever hash function the LMCS uses.  A 2^23-leaf tree's salt matrix would be 268 MB of HBM written once and read once; the
// permutation costs the leaf kernel less than that traffic and openings regenerate the few rows they hint.
//
// The leaf kernels index leaves by a device layout (slot q = j * N + r <-> natural index r * B + j, lmcs.hip); the PRF takes the
// reference's physical row = the bit reversal of the natural index.  Device only; include after poseidon2_fast.cuh.
#pragma once
#include "ctx.hpp"
#include "blake3.cuh"
#include "keccak.cuh"

static constexpr u64 SALT_DOMAIN_TAG = 0x53414c54ULL;

// physical row of the leaf with coset j and in-coset row r of a tree of 2^bits leaves, lb coset bits
__device__ __forceinline__ u64 salt_phys_row(size_t j, size_t r, int lb, int bits) {
  const u64 i = ((u64)r << lb) | (u64)j;
  return bits ? (__brevll(i) >> (64 - bits)) : 0;
}

// z[0 .. sa.n) = the salt row (canonical felts); z[sa.n .. 12) is the rest of the PRF output and must not be used
__device__ __forceinline__ void salt_row(const SaltArgs& sa, u64 phys_row, u64 z[12]) {
  z[0] = phys_row;
  z[1] = sa.tree;
  z[2] = SALT_DOMAIN_TAG;
#pragma unroll
  for (int i = 3; i < 8; i++) z[i] = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) z[8 + i] = sa.key[i];
  p2f_permute(z);
}

// The salt absorbed as one more matrix of width sa.n (<= 8), per hasher.
// Poseidon2 sponge: one more rate block, zero-padded like any row tail.
__device__ __forceinline__ void salt_absorb_p2(u64 s[12], const SaltArgs& sa, u64 phys_row) {
  u64 z[12];
  salt_row(sa, phys_row, z);
#pragma unroll
  for (int k = 0; k < 8; k++) s[k] = k < sa.n ? z[k] : 0;
  p2f_permute(s);
}
// RPO / RPX: the same block under the configuration's permutation (the PRF stays Poseidon2)
__device__ __forceinline__ void salt_absorb_alg(u64 s[12], const SaltArgs& sa, u64 phys_row, int lmcs) {
  u64 z[12];
  salt_row(sa, phys_row, z);
#pragma unroll
  for (int k = 0; k < 8; k++) s[k] = k < sa.n ? z[k] : 0;
  alg_permute(lmcs, s);
}
// Keccak sponge: one more block of the 17-lane rate
__device__ __forceinline__ void salt_absorb_kk(uint64_t s[25], const SaltArgs& sa, u64 phys_row) {
  u64 z[12];
  salt_row(sa, phys_row, z);
#pragma unroll
  for (int k = 0; k < 8; k++) s[k] = k < sa.n ? z[k] : 0;
#pragma unroll
  for (int k = 8; k < 17; k++) s[k] = 0;
  kk::f1600(s);
}
// Blake3 chaining hasher: st = blake3(st || salt felts as 8 LE bytes each), a message of 40 .. 96 bytes = one or two blocks of one chunk
__device__ __forceinline__ void salt_absorb_b3(uint32_t st[8], const SaltArgs& sa, u64 phys_row) {
  u64 z[12];
  salt_row(sa, phys_row, z);
  const uint32_t total = 32 + 8 * (uint32_t)sa.n;
  uint32_t m[16], cv[8];
#pragma unroll
  for (int k = 0; k < 8; k++) {
    m[k] = st[k];
    cv[k] = b3::iv(k);
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {  // felts 0 .. 3 share block 0 with the state
    const u64 v = k < sa.n ? z[k] : 0;
    m[8 + 2 * k] = (uint32_t)v;
    m[9 + 2 * k] = (uint32_t)(v >> 32);
  }
  if (total <= 64) {
    b3::compress(cv, m, 0, total, b3::CHUNK_START | b3::CHUNK_END | b3::ROOT);
  } else {
    b3::compress(cv, m, 0, 64, b3::CHUNK_START);
#pragma unroll
    for (int k = 0; k < 8; k++) {  // felts 4 .. 7, zero-filled behind the message's end
      const u64 v = (k < 4 && 4 + k < sa.n) ? z[4 + k] : 0;
      m[2 * k] = (uint32_t)v;
      m[2 * k + 1] = (uint32_t)(v >> 32);
    }
    b3::compress(cv, m, 0, total - 64, b3::CHUNK_END | b3::ROOT);
  }
#pragma unroll
  for (int k = 0; k < 8; k++) st[k] = cv[k];
}
