// The part of pcs::open_with_channel (crates/lifted-stark/src/pcs/prover.rs:34-101) that does not depend on what was committed or on how
// many points it is opened at: the FRI commit / fold / final-polynomial rounds over the DEEP layer and the query phase over a list of
// input trees.  mh_session (prover.hip: the STARK, trees [preprocessed?, main, aux, quotient], two points) and mh_pcs (pcs_open.hip: any
// trees, 1..4 points) both own one PcsStage; each fills `layer` with its own DEEP kernels and calls start().
// Protocol order (the `stage` counters and their messages) stays with the owner.
#pragma once
#include "../../include/midenhip.h"
#include "challenger.hpp"
#include "ctx.hpp"
#include "gl.cuh"
#include "kernels.hpp"
#include <algorithm>
#include <memory>
#include <vector>

struct mh_proof {
  std::vector<uint8_t> log_trace_heights;  // instance order
  std::vector<u64> fields;
  std::vector<u64> commitments;  // 4 felts each
  u64 digest[4];
};

inline int fri_num_rounds(const mh_pcs_params& p, int log_lde) {
  int log_max_final = p.log_final_degree + p.log_blowup;
  int steps = log_lde > log_max_final ? log_lde - log_max_final : 0;
  return (steps + p.log_folding_arity - 1) / p.log_folding_arity;
}

// PcsParams::new (pcs/params.rs:52-96) as the provers check it
inline void pcs_params_require(const mh_pcs_params& pp) {
  MH_REQUIRE(pp.log_blowup > 0 && pp.log_blowup <= 8, "log_blowup must be in 1..8");
  MH_REQUIRE(pp.log_folding_arity >= 1 && pp.log_folding_arity <= 3, "FRI folding arity must be 2, 4 or 8");
  MH_REQUIRE(pp.num_queries > 0, "num_queries must be > 0");
  for (int b : {pp.deep_pow_bits, pp.folding_pow_bits, pp.query_pow_bits})
    MH_REQUIRE(b >= 0 && b <= 32, "proof-of-work bits must be in 0..32 (sample_bits reads the low 32 bits of a sample)");
  MH_REQUIRE(pp.log_final_degree >= 0 && pp.log_final_degree <= 32, "log_final_degree must be in 0..32");
  MH_REQUIRE(pp.log_final_degree + pp.log_blowup >= pp.log_folding_arity - 1, "final degree unreachable by fixed-arity folding");
}

// prover.hip: the proof-of-work search of the one-shot provers (host for few bits, the device kernels otherwise)
void do_grind(mh_ctx* c, HostTranscript& tr, int bits);

struct PcsStage {
  mh_ctx* c = nullptr;
  mh_pcs_params pp{};
  Dist dist;
  int lb = 0, L = 0, rounds = 0;  // log_blowup, log of the LDE height of the tallest input, FRI rounds
  size_t alignment = 8;           // lmcs.alignment() of the input trees' openings
  std::vector<const mh_tree*> trees;  // input trees in group order (borrowed); a tree shorter than 2^L is virtually lifted
  // FRI
  DevBuf layer;
  std::vector<std::unique_ptr<mh_tree>> fri_trees;
  int log_rows = 0, cbits = 0, cb_loc = 0;
  size_t fri_c0 = 0;
  bool sharded = false, round_committed = false;

  size_t final_poly_len() const { return (size_t)1 << std::max(0, L - rounds * pp.log_folding_arity - lb); }
  // the DEEP layer is in `layer`, coset-major [2^lbl][2^log_n] EF pairs: cbits = coset bits of the whole layer, cb_loc = those stored
  // on this rank (cosets coset0 ..)
  void start(int log_n, int lbl, size_t coset0) {
    log_rows = log_n; cbits = lb; cb_loc = lbl; fri_c0 = coset0;
    sharded = dist.on();
  }
  // ---- 8. FRI: commit the current layer, then fold it ----
  void fri_commit(u64 root[4]) {
    ProfScope span(c, "span:FRI round commit");  // pcs/fri/prover.rs:164
    MH_REQUIRE((int)fri_trees.size() < rounds && !round_committed, "no FRI round left to commit");
    const int la = pp.log_folding_arity;
    if (sharded && log_rows - la < dist.logG) {
      // fewer leaf rows per coset than ranks: the row-range split of the tree is over; every rank takes
      // the whole (small) layer and continues redundantly
      DevBuf full(((size_t)1 << (log_rows + cbits)) * 16);
      dist.all_gather(c, layer.p, full.p, ((size_t)1 << (log_rows + cb_loc)) * 16);
      layer = std::move(full);
      cb_loc = cbits;
      fri_c0 = 0;
      sharded = false;
    }
    if (log_rows < la) {  // tiny layer: fewer than `arity` rows per coset -> single-coset (natural) layout
      MH_REQUIRE(!sharded, "internal: sharded FRI layer shorter than the arity");
      DevBuf nat(((size_t)1 << (log_rows + cbits)) * 16);
      fri_to_natural(c, layer.u(), log_rows, cbits, nat.u());
      c->sync();
      layer = std::move(nat);
      log_rows += cbits;
      cbits = 0;
      cb_loc = 0;
    }
    std::unique_ptr<mh_tree> t(new mh_tree());
    t->ctx = c; t->log_blowup = cbits;
    t->fri_log_rows = log_rows; t->fri_log_arity = la;
    t->fri_log_cosets = cb_loc; t->fri_coset0 = fri_c0;
    if (sharded) {
      DevBuf dig(((size_t)1 << (log_rows - la + cb_loc)) * 32);
      fri_leaf_hash(c, layer.u(), log_rows, cb_loc, la, dig.u());
      lmcs_build_sharded(c, t.get(), dist, dig.u(), log_rows - la);
    } else {
      lmcs_alloc_layers(t.get(), log_rows + cbits - la);
      lmcs_salt_assign(c, t.get());
      fri_leaf_hash(c, layer.u(), log_rows, cbits, la, lmcs_leaf_layer(t.get()), lmcs_salt_of(t.get()));
      lmcs_compress_layers(c, t.get());
    }
    memcpy(root, t->root, 32);
    fri_trees.push_back(std::move(t));
    round_committed = true;
  }
  void fri_fold_round(e2 fb) {
    ProfScope span(c, "span:FRI fold");  // pcs/fri/prover.rs:183
    MH_REQUIRE(round_committed, "fold before the round's commitment");
    const int la = pp.log_folding_arity;
    DevBuf next(((size_t)1 << (log_rows + cb_loc - la)) * 16);
    fri_fold(c, layer.u(), log_rows, cb_loc, cbits, fri_c0, la, fb, next.u());
    fri_trees.back()->fri_layer = std::move(layer);
    layer = std::move(next);
    log_rows -= la;
    round_committed = false;
  }
  // final polynomial (fri/prover.rs:212-239): it has degree < fpd = n_f / B, so the fpd evaluations on
  // ONE coset s*<w_fpd> of the final layer determine it (s = w_{n_f}^(first local coset); s = 1 on a
  // single GPU = the reference's first fpd bit-reversed entries).  Interpolated on the host, shift undone,
  // returned in descending degree order.
  void fri_final(std::vector<e2>& desc) {
    ProfScope span(c, "span:idft final poly");  // pcs/fri/prover.rs:231
    MH_REQUIRE((int)fri_trees.size() == rounds && !round_committed, "FRI rounds not finished");
    const int logn_f = log_rows + cbits;
    const int log_fpd = std::max(0, logn_f - lb);
    const size_t fpd = (size_t)1 << log_fpd;
    const size_t n_loc = (size_t)1 << (log_rows + cb_loc);
    std::vector<u64> host(2 * n_loc);
    c->d2h(host.data(), layer.p, n_loc * 16);
    std::vector<e2> vals(fpd);
    u64 s_shift = 1;
    if (sharded) {
      MH_REQUIRE(cbits == lb && fpd == ((size_t)1 << log_rows), "internal: final layer shape");
      for (size_t r = 0; r < fpd; r++) vals[r] = e2{host[2 * r], host[2 * r + 1]};  // first local coset
      s_shift = gl_pow(gl_two_adic_generator(logn_f), fri_c0);
    } else {
      for (size_t r = 0; r < fpd; r++) {
        size_t i = r << (logn_f - log_fpd);
        size_t slot = ((i & (((size_t)1 << cbits) - 1)) << log_rows) + (i >> cbits);
        vals[r] = e2{host[2 * slot], host[2 * slot + 1]};
      }
    }
    const u64 w_inv = gl_inv(gl_two_adic_generator(log_fpd)), n_inv = gl_inv((u64)fpd);
    const u64 s_inv = gl_inv(s_shift);
    std::vector<e2> coef(fpd);
    u64 sk = 1;
    for (size_t k = 0; k < fpd; k++) {
      e2 s = e2_make(0);
      u64 wk = gl_pow(w_inv, k), x = 1;
      for (size_t r = 0; r < fpd; r++) {
        s = e2_add(s, e2_mulf(vals[r], x));
        x = gl_mul(x, wk);
      }
      coef[k] = e2_mulf(s, gl_mul(n_inv, sk));
      sk = gl_mul(sk, s_inv);
    }
    desc.assign(coef.rbegin(), coef.rend());
    layer.release();
  }
  // ---- 9. openings of every tree at the sampled domain indices, in transcript (hint) order ----
  void open(std::vector<size_t> idx, std::vector<u64>& fields, std::vector<u64>& commitments) {
    ProfScope span(c, "span:query phase");  // pcs/prover.rs:89
    std::sort(idx.begin(), idx.end());
    idx.erase(std::unique(idx.begin(), idx.end()), idx.end());
    for (size_t i : idx) MH_REQUIRE(i < ((size_t)1 << L), "query index out of range");
    // every tree's gather list first, then ONE gather / read-back (/ all-reduce) for all of them
    std::vector<const u64*> ptrs;
    std::vector<OpenPlan> plans;
    for (const mh_tree* t : trees) {
      const int depth = t->log_height + t->shard_logG;  // full depth (a rank stores a subtree)
      if (depth >= L) {
        plans.push_back(lmcs_open_plan(t, idx, alignment, &dist, ptrs));
        continue;
      }
      // a tree shorter than the max domain is virtually lifted: indices fold by their low bits (lmcs/tree_indices.rs:72-84)
      std::vector<size_t> tidx(idx);
      const size_t mask = ((size_t)1 << depth) - 1;
      for (auto& i : tidx) i &= mask;
      std::sort(tidx.begin(), tidx.end());
      tidx.erase(std::unique(tidx.begin(), tidx.end()), tidx.end());
      plans.push_back(lmcs_open_plan(t, tidx, alignment, &dist, ptrs));
    }
    int depth = L;
    for (auto& t : fri_trees) {
      depth -= pp.log_folding_arity;
      const size_t mask = ((size_t)1 << depth) - 1;
      for (auto& i : idx) i &= mask;
      std::sort(idx.begin(), idx.end());
      idx.erase(std::unique(idx.begin(), idx.end()), idx.end());
      plans.push_back(lmcs_open_plan(t.get(), idx, 1, &dist, ptrs));
    }
    std::vector<u64> host;
    lmcs_open_run(c, ptrs, &dist, host);
    for (const OpenPlan& plan : plans) {
      std::vector<u64> f, cm;
      lmcs_open_take(plan, host, f, cm);
      fields.insert(fields.end(), f.begin(), f.end());
      commitments.insert(commitments.end(), cm.begin(), cm.end());
    }
  }
};
