// mh_commit_host: the LMCS commitment of mh_commit_traces on the CPU -- for VERIFIERS and setup only.  A verifier box has no GPU, and
// the root of an AIR's preprocessed matrices is part of the statement it checks: it must be able to derive that root from the
// matrices it knows (the reference's verifier does: precompiles-prover/src/session/preprocessed_cache.rs) instead of trusting the one
// the prover sends along.  No prover entry calls this file; proving has no CPU path.
//
// Restated from the reference, like the device path it is held to (root for root, tests/test_commit_host.py and
// tests/test_gpu_setup_root.py):
//   crates/lifted-stark/src/prover/commit.rs:83-173      per matrix: coset LDE by 2^log_blowup onto the canonical shift of ITS OWN
//                                                        lde order (gl_lde_shift), rows stored bit-reversed
//   crates/lifted-stark/src/lmcs/lifted_tree.rs:233-461  leaf states carried from matrix to matrix in ascending height; when the
//                                                        height grows by f, state i becomes the states [i f, (i + 1) f)
//   crates/lifted-stark/src/lmcs/lifted_tree.rs:472-511  digest i = state[bitrev(i)], then pairwise compression to the root
// The hashers are lmcs_host.hpp (shared with verifier.cpp).  New here: the Goldilocks radix-2 NTT and the tree loop.
//
// The LDE of an n x w matrix, N = n 2^b rows out: coefficients c_k by one inverse transform; the forward transform of size N is
// decimation in frequency, natural order in, bit-reversed order out -- the storage order wanted.  Its first b stages meet only the
// zero padding: after them block p (n rows) holds  c_k (w_N^bitrev_b(p))^k,  so the blocks are written directly, with the coset
// shift folded in, and only the log n stages inside the blocks are run.  Every stage works on whole rows (all columns abreast).
#include "../../include/midenhip.h"
#include "gl.cuh"
#include "lmcs_host.hpp"
#include <algorithm>
#include <cstdio>
#include <exception>
#include <new>
#include <string>
#include <thread>
#include <vector>

namespace {

// f(begin, end) over [0, n) in contiguous pieces whose bounds are multiples of 8, on up to min(16, hardware threads) threads
template <class F>
void parallel_for(size_t n, size_t grain, F f) {
  const unsigned hw = std::thread::hardware_concurrency();
  const size_t want = std::min<size_t>(std::min<size_t>(16, hw ? hw : 1), (n + grain - 1) / grain);
  if (want <= 1) {
    f((size_t)0, n);
    return;
  }
  const size_t piece = ((n + want - 1) / want + 7) / 8 * 8;
  std::vector<std::thread> pool;
  std::vector<std::exception_ptr> failed(want);
  std::exception_ptr spawn_failed;
  size_t begin = piece;  // the first piece runs on the calling thread
  try {
    for (size_t t = 1; t < want && begin < n; t++, begin += piece) {
      const size_t b = begin, e = std::min(n, begin + piece);
      pool.emplace_back([&f, &failed, t, b, e] {
        try {
          f(b, e);
        } catch (...) {
          failed[t] = std::current_exception();
        }
      });
    }
  } catch (...) {  // no more threads to be had: the pieces not handed out run here
    spawn_failed = std::current_exception();
  }
  try {
    f((size_t)0, std::min(n, piece));
    if (spawn_failed && begin < n) f(begin, n);
  } catch (...) {
    failed[0] = std::current_exception();
  }
  for (std::thread& th : pool) th.join();
  for (const std::exception_ptr& e : failed)
    if (e) std::rethrow_exception(e);
}

// tw[j] = root^j, j < count
std::vector<u64> powers(u64 root, size_t count) {
  std::vector<u64> tw(count);
  parallel_for(count, 1 << 14, [&](size_t b, size_t e) {
    u64 x = gl_pow(root, b);
    for (size_t j = b; j < e; j++) {
      tw[j] = x;
      x = gl_mul(x, root);
    }
  });
  return tw;
}

// Decimation in frequency on every block of 2^log_block rows of a row-major matrix of `rows` rows and `w` columns, in place:
// natural order in, bit-reversed order out (inside each block).  tw = the powers of a root of unity of order 2^log_block,
// 2^(log_block - 1) of them.
void dif_blocks(u64* x, size_t rows, size_t w, int log_block, const std::vector<u64>& tw) {
  for (int s = log_block; s >= 1; s--) {
    const size_t half = (size_t)1 << (s - 1), stride = (size_t)1 << (log_block - s);
    parallel_for(rows / 2, std::max<size_t>(64, (1 << 14) / w), [&](size_t b, size_t e) {
      for (size_t t = b; t < e; t++) {
        const size_t j = t & (half - 1);
        u64* lo = x + (((t - j) << 1) + j) * w;
        u64* hi = lo + half * w;
        const u64 f = tw[j * stride];
        for (size_t c = 0; c < w; c++) {
          const u64 u = lo[c], v = hi[c];
          lo[c] = gl_add(u, v);
          hi[c] = gl_mul(gl_sub(u, v), f);
        }
      }
    });
  }
}

// commit.rs:83-173 for one matrix: n x w, natural rows, any u64 cells  ->  (n << lb) x w on the canonical coset, bit-reversed rows
std::vector<u64> coset_lde_bitrev(const u64* m, int log_n, size_t w, int lb) {
  const size_t n = (size_t)1 << log_n, big = n << lb;
  const int L = log_n + lb;
  std::vector<u64> coef(n * w);
  parallel_for(n * w, 1 << 15, [&](size_t b, size_t e) {
    for (size_t i = b; i < e; i++) coef[i] = gl_canon(m[i]);
  });
  if (log_n) dif_blocks(coef.data(), n, w, log_n, powers(gl_inv(gl_two_adic_generator(log_n)), n / 2));
  // coef row bitrev(k) = n c_k.  Block p of the result, before its own stages: c_k (shift w_N^bitrev(p))^k
  std::vector<u64> out(big * w);
  const u64 shift = gl_lde_shift(L), w_big = gl_two_adic_generator(L), n_inv = gl_inv((u64)n % GL_P);
  parallel_for(big, std::max<size_t>(64, (1 << 14) / w), [&](size_t b, size_t e) {
    u64 base = 0, x = 0;
    for (size_t t = b; t < e; t++) {
      const size_t p = t >> log_n, k = t & (n - 1);
      if (t == b || k == 0) {
        base = gl_mul(shift, gl_pow(w_big, bitrev32((u32)p, lb)));
        x = gl_mul(n_inv, gl_pow(base, k));
      }
      const u64* src = coef.data() + (size_t)bitrev32((u32)k, log_n) * w;
      u64* dst = out.data() + t * w;
      for (size_t c = 0; c < w; c++) dst[c] = gl_mul(src[c], x);
      x = gl_mul(x, base);
    }
  });
  coef = std::vector<u64>();
  if (log_n) dif_blocks(out.data(), big, w, log_n, powers(gl_two_adic_generator(log_n), n / 2));
  return out;
}

// lifted_tree.rs:427-461 absorb_matrix: physical row r of the matrix into state r
void absorb_matrix(int lmcs, std::vector<u64>& states, const u64* lde, size_t rows, size_t w) {
  const size_t sw = lmcs_host::state_words(lmcs);
  const bool simd = lmcs_host::simd(lmcs);
  parallel_for(rows, 256, [&](size_t b, size_t e) {
    size_t r = b;
    if (simd)
      for (; r < e; r += 8) {  // the pieces start at multiples of 8: eight states one after the other
        const size_t k = std::min<size_t>(8, e - r);
        if (k < 8) break;
        const u64* at[8];
        for (size_t j = 0; j < 8; j++) at[j] = lde + (r + j) * w;
        lmcs_host::leaf_absorb8(states.data() + r * sw, at, 8, w);
      }
    for (; r < e; r++) lmcs_host::leaf_absorb(lmcs, states.data() + r * sw, lde + r * w, w);
  });
}

// lifted_tree.rs:472-511 compress_uniform, one level: out[i] = compress(children[2i], children[2i + 1])
void compress_level(int lmcs, const u64* children, size_t n_out, u64* out) {
  const bool simd = lmcs_host::simd(lmcs);
  parallel_for(n_out, 256, [&](size_t b, size_t e) {
    size_t i = b;
    if (simd)
      for (; i < e; i += 8) lmcs_host::compress8(children + 8 * i, std::min<size_t>(8, e - i), out + 4 * i);
    for (; i < e; i++) {
      const u64* c = children + 8 * i;
      const Digest4 d = lmcs_host::compress2(lmcs, Digest4{c[0], c[1], c[2], c[3]}, Digest4{c[4], c[5], c[6], c[7]});
      memcpy(out + 4 * i, d.data(), 32);
    }
  });
}

void commit(int lmcs, int n_mats, const uint64_t* const* mats, const uint8_t* log_heights, const size_t* widths, int lb, u64 root[4]) {
  const size_t sw = lmcs_host::state_words(lmcs);
  std::vector<u64> states((sw << (log_heights[0] + lb)), 0);
  int log_active = log_heights[0] + lb;
  for (int i = 0; i < n_mats; i++) {
    const int log_rows = log_heights[i] + lb;
    const size_t rows = (size_t)1 << log_rows;
    if (log_rows > log_active) {  // lifted_tree.rs:363-417: state i is duplicated to the slots [i f, (i + 1) f)
      std::vector<u64> lifted(sw * rows);
      const int sh = log_rows - log_active;
      parallel_for(rows, 1 << 12, [&](size_t b, size_t e) {
        for (size_t r = b; r < e; r++) memcpy(lifted.data() + r * sw, states.data() + (r >> sh) * sw, sw * 8);
      });
      states.swap(lifted);
      log_active = log_rows;
    }
    const std::vector<u64> lde = coset_lde_bitrev(mats[i], log_heights[i], widths[i], lb);
    absorb_matrix(lmcs, states, lde.data(), rows, widths[i]);
  }
  // digest i of the leaf layer = state[bitrev(i)] (lifted_tree.rs:247-258), then the levels up to the root
  const size_t leaves = (size_t)1 << log_active;
  std::vector<u64> level(4 * leaves);
  parallel_for(leaves, 1 << 12, [&](size_t b, size_t e) {
    for (size_t i = b; i < e; i++) memcpy(level.data() + 4 * i, states.data() + (size_t)bitrev32((u32)i, log_active) * sw, 32);
  });
  states = std::vector<u64>();
  for (size_t n = leaves / 2; n >= 1; n /= 2) {
    std::vector<u64> up(4 * n);
    compress_level(lmcs, level.data(), n, up.data());
    level.swap(up);
  }
  memcpy(root, level.data(), 32);
}

}  // namespace

extern "C" int mh_commit_host(int lmcs, int n_mats, const uint64_t* const* rowmajor, const uint8_t* log_heights, const size_t* widths,
                              int log_blowup, uint64_t root[4], char* err, size_t err_cap) {
  auto fail = [&](int code, const std::string& msg) {
    if (err && err_cap) snprintf(err, err_cap, "mh_commit_host: %s", msg.c_str());
    return code;
  };
  if (!rowmajor || !log_heights || !widths || !root) return fail(MH_ERR_INVALID, "null argument");
  if (lmcs < MH_LMCS_POSEIDON2 || lmcs > MH_LMCS_RPX) return fail(MH_ERR_INVALID, "unknown LMCS hasher id");
  if (n_mats < 1) return fail(MH_ERR_INVALID, "need at least one matrix");
  if (log_blowup < 0 || log_blowup > 8) return fail(MH_ERR_INVALID, "log_blowup must be in 0..8");
  for (int i = 0; i < n_mats; i++) {
    const std::string which = "matrix " + std::to_string(i);
    if (!rowmajor[i]) return fail(MH_ERR_INVALID, which + " is a null pointer");
    if (!widths[i]) return fail(MH_ERR_INVALID, which + " has width zero");
    if ((int)log_heights[i] + log_blowup > 32) return fail(MH_ERR_INVALID, which + ": log height + log_blowup exceeds 32, the field's two-adicity");
    if (i && log_heights[i - 1] > log_heights[i]) return fail(MH_ERR_INVALID, "matrices must be sorted by ascending height");
  }
  try {
    u64 r[4];
    commit(lmcs, n_mats, rowmajor, log_heights, widths, log_blowup, r);
    memcpy(root, r, 32);
    if (err && err_cap) err[0] = 0;
    return MH_OK;
  } catch (const std::bad_alloc&) {
    return fail(MH_ERR_OOM, "out of host memory");
  } catch (const std::exception& e) {
    return fail(MH_ERR_INTERNAL, e.what());
  }
}
