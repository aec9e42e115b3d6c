// The LMCS hashers on the HOST, for the two host-only users of them: the verifier (verifier.cpp: the leaves and the path of a batch
// opening) and the host commitment (commit_host.cpp: every leaf and every node of a tree).  One definition of what a leaf absorbs
// and what a node compresses under each of the five configurations (MH_LMCS_*), so that the two cannot drift apart:
//   sponge configurations (Poseidon2, RPO, RPX)  overwrite-mode sponge, rate 8 (crates/stateful-hasher/src/field_sponge.rs:41-59),
//                                                node = one permutation over left || right, lanes 0..3
//   Blake3                                       chaining hasher, state := blake3(state || row bytes) (chaining.rs:32-50),
//                                                node = blake3(left || right)
//   Keccak                                       the same sponge over 64-bit lanes, rate 17; node = kk::compress_pair
// The hasher is an argument, never a global: the functions are called from several threads at once.
// Under Poseidon2 and a CPU with AVX-512 the *8 forms run eight hashes per permutation (p2_host_simd.cpp); MH_HOST_SIMD=0 switches
// them off (p2_host_simd_available), and the callers then take the scalar forms.
#pragma once
#include "../../include/midenhip.h"
#include "challenger.hpp"
#include <cstring>
#include <vector>

// p2_host_simd.cpp: eight Poseidon2 permutations per AVX-512 call (host only; the tree tops of the prover use them too)
bool p2_host_simd_available();
void p2_host_compress8(const uint64_t* pairs, int n, uint64_t* out);
void p2_host_permute8(uint64_t* states);

namespace lmcs_host {

// words of a leaf's running state: the sponge's 12, Keccak's 25 lanes, the chaining hasher's 32 bytes
inline size_t state_words(int hash) { return hash == MH_LMCS_BLAKE3 ? 4 : (hash == MH_LMCS_KECCAK ? 25 : 12); }
constexpr size_t MAX_STATE_WORDS = 25;

inline bool simd(int hash) { return hash == MH_LMCS_POSEIDON2 && p2_host_simd_available(); }

// Overwrite-mode sponge over a whole row (already aligned, or short: the missing lanes of the last block are zero).
inline void absorb(int hash, u64 st[12], const u64* v, size_t n) {
  for (size_t off = 0; off < n; off += 8) {
    const size_t k = n - off < 8 ? n - off : 8;
    for (size_t i = 0; i < k; i++) st[i] = v[off + i];
    for (size_t i = k; i < 8; i++) st[i] = 0;
    alg_permute(hash, st);
  }
}

// One row of one matrix into a leaf's state (state_words(hash) words, zero before the first matrix).  The digest is words 0..3.
inline void leaf_absorb(int hash, u64* st, const u64* row, size_t w) {
  if (hash == MH_LMCS_BLAKE3) {  // chaining hasher: state := blake3(state || row bytes) (chaining.rs:32-50)
    uint8_t small[32 + 8 * 32], d[32];
    std::vector<uint8_t> big;
    uint8_t* msg = small;
    if (32 + 8 * w > sizeof small) {
      big.resize(32 + 8 * w);
      msg = big.data();
    }
    memcpy(msg, st, 32);
    if (w) memcpy(msg + 32, row, 8 * w);
    b3::hash_bytes(msg, 32 + 8 * w, d);
    memcpy(st, d, 32);
    return;
  }
  if (hash == MH_LMCS_KECCAK) {
    kk::lmcs_absorb(st, row, w);
    return;
  }
  absorb(hash, st, row, w);
}
// leaf_absorb under Poseidon2 for n <= 8 leaves abreast: st = eight states of 12 words one after the other, rows[j] = leaf j's row of
// w cells (canonicalised here).  Call only when simd(MH_LMCS_POSEIDON2); the states of the lanes j >= n are scratch.
inline void leaf_absorb8(u64* st, const u64* const* rows, size_t n, size_t w) {
  for (size_t o = 0; o < w; o += 8) {
    const size_t k = w - o < 8 ? w - o : 8;
    for (size_t j = 0; j < n; j++) {
      for (size_t i = 0; i < k; i++) st[12 * j + i] = gl_canon(rows[j][o + i]);
      for (size_t i = k; i < 8; i++) st[12 * j + i] = 0;
    }
    p2_host_permute8(st);
  }
}

inline Digest4 compress2(int hash, const Digest4& l, const Digest4& r) {
  if (hash == MH_LMCS_BLAKE3) {  // blake3(left || right)
    uint8_t msg[64], d[32];
    memcpy(msg, l.data(), 32);
    memcpy(msg + 32, r.data(), 32);
    b3::hash_bytes(msg, 64, d);
    Digest4 o;
    memcpy(o.data(), d, 32);
    return o;
  }
  if (hash == MH_LMCS_KECCAK) {
    Digest4 o;
    kk::compress_pair(l.data(), r.data(), o.data());
    return o;
  }
  u64 st[12] = {l[0], l[1], l[2], l[3], r[0], r[1], r[2], r[3], 0, 0, 0, 0};
  alg_permute(hash, st);
  return Digest4{st[0], st[1], st[2], st[3]};
}
// compress2 under Poseidon2 for n <= 8 nodes at once: pairs = n x (left || right), out = n x 4 words.  Call only when
// simd(MH_LMCS_POSEIDON2).
inline void compress8(const u64* pairs, size_t n, u64* out) {
  u64 in[64];
  for (size_t j = 0; j < 8 * n; j++) in[j] = gl_canon(pairs[j]);
  p2_host_compress8(in, (int)n, out);
}

}  // namespace lmcs_host
