// The batch verifier's device pass: the LMCS openings of many proofs hashed in two kernels, gfx950.
//
// A verifier spends almost all its time hashing query openings (verifier.cpp open_batch).  The shape of an opening -- which nodes are
// derived, which siblings are streamed -- depends on its indices alone (lmcs_plan.hpp), so the host plans every opening of a batch
// first, packs all opened rows and all streamed siblings into two buffers, uploads them once and runs
//   k_vfy_leaves<H>   one lane per opened leaf: the leaf's matrices absorbed in stream order, aligned rows as streamed and the raw salt
//                     as one more short matrix (lmcs_host::leaf_absorb; the per-lane hashers are the bodies of lmcs.hip's leaf
//                     kernels over a row-major row).  Leaves are grouped into shape classes (the same list of widths) and a class
//                     is padded to whole waves, so a wave runs one shape; the class table is a kernel argument.
//   k_vfy_paths<H>    one workgroup per opening (one tree of one proof): leaf digests into LDS, then level by level the lanes stride
//                     over the plan's (left, right) pairs, take each digest from the LDS array of the level below or from the sibling
//                     buffer, compress, and write the other LDS array; a barrier between levels; the last digest against the root,
//                     one lane stores the 0/1 verdict.  LDS = 2 x (largest opening of the launch) x 32 B, at most 2 x 1024 x 32 B.
//   k_vfy_witness<H>  k_vfy_paths that keeps what it derives (mh_lmcs_witness_batch, mh_verify_batch_witness): every
//                     parent also goes to a pass-wide node array, every opened leaf copies its path element of the level.
// H = the five configurations (MH_LMCS_*).  One read-back of the verdicts (a witness pass: of leaf digests, nodes, paths and verdicts
// in one block) ends a pass; nothing synchronises per proof.  Device memory per pass is bounded by MH_VERIFY_BATCH_BYTES (default
// 256 MB): larger batches run as consecutive chunks.
#include "ctx.hpp"
#include "../../include/midenhip.h"
#include "kernels.hpp"
#include "air.hpp"
#include "lmcs_verify.hpp"
#include "poseidon2_fast.cuh"
#include "blake3.cuh"
#include "keccak.cuh"
#define RESCUE_FAST 1  // S-boxes through p2f_mulN, as in lmcs.hip
#include "rescue.cuh"
#include "gl.cuh"
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <thread>

namespace {

constexpr int VB_THREADS = 256;
constexpr int VB_MAX_CLASSES = 16;    // shape classes per leaf launch (more: further launches)
constexpr int VB_MAX_WIDTHS = 512;    // widths of all classes of one launch; also the most matrices of one tree
constexpr u32 VB_MAX_LEAVES = 1024;   // distinct opened leaves of one opening: the path kernel's two LDS arrays
constexpr u32 VB_MAX_WIDTH = (((u32)1024 << b3::MAX_STACK) - 32) / 8;  // a row is one Blake3 message of at most 256 KiB (lmcs.hip)
constexpr u64 VB_NO_LEAF = ~(u64)0;

struct VbClasses {
  u32 wave0[VB_MAX_CLASSES + 1];  // class k owns the waves [wave0[k], wave0[k + 1]) of the launch
  u32 w_off[VB_MAX_CLASSES + 1];  // and absorbs widths[w_off[k] .. w_off[k + 1])
  u32 widths[VB_MAX_WIDTHS];
  u32 n_classes;
};
struct VbLeafArgs {
  const u64* fields;    // the opened rows of the whole pass
  const u64* row_off;   // [n_lanes] first felt of the lane's leaf; VB_NO_LEAF: a padding lane
  const u32* out_slot;  // [n_lanes] where its digest goes
  u64* digests;         // [leaves of the pass][4]
  u32 n_lanes;
};
struct VbOpening {  // 64 bytes
  u64 root[4];
  u64 sib0;  // first digest of this opening in the sibling buffer
  u32 leaf0, n_leaves;
  u32 pair0;  // first parent of this opening in `pairs` (two sources per parent)
  u32 lvl0;   // first of its depth + 1 level offsets in `lvl` (relative to pair0)
  u32 depth, pad;
};
struct VbPathArgs {
  const VbOpening* ops;
  const u32* pairs;
  const u32* lvl;
  const u64* digests;
  const u64* sibs;
  int* ok;
  u32 lds_slots;  // digests per LDS array
};

template <int H>
__device__ __forceinline__ void vb_permute(u64 s[12]) {
  if constexpr (H == MH_LMCS_POSEIDON2) p2f_permute(s);
  else alg_permute(H, s);
}

// the digest of one leaf: `row` = its matrices' rows one after the other, n_w widths from the (wave-uniform) class table
template <int H>
__device__ __forceinline__ void vb_leaf(const u64* __restrict__ row, const VbClasses& ct, u32 w0, u32 w1, u64 out[4]) {
  if constexpr (H == MH_LMCS_BLAKE3) {  // chaining hasher: state := blake3(state || row bytes), lmcs.hip leaf_absorb_b3_body
    uint32_t st[8];
#pragma unroll
    for (int i = 0; i < 8; i++) st[i] = 0;
#pragma unroll 1
    for (u32 mi = w0; mi < w1; mi++) {
      const u32 w = ct.widths[mi];
      const u32 total = 32 + 8 * w, n_blocks = (total + 63) / 64;
      b3::Stream h;
      h.init();
      uint32_t m[16];
#pragma unroll 1
      for (u32 b = 0; b < n_blocks; b++) {
        const int f0 = (int)(8 * b) - 4;  // block 0: the state, then felts 0..3
#pragma unroll
        for (int k = 0; k < 8; k++) {
          const int f = f0 + k;
          u64 v = 0;
          if (f >= 0 && (u32)f < w) v = row[f];
          m[2 * k] = (uint32_t)v;
          m[2 * k + 1] = (uint32_t)(v >> 32);
        }
        if (b == 0) {
#pragma unroll
          for (int k = 0; k < 8; k++) m[k] = st[k];
        }
        if (b + 1 < n_blocks) h.block(m);
        else h.finish(m, total - 64 * b, st);
      }
      row += w;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) out[i] = (u64)st[2 * i] | ((u64)st[2 * i + 1] << 32);
  } else if constexpr (H == MH_LMCS_KECCAK) {  // overwrite-mode sponge, 25 lanes, rate 17
    uint64_t s[25];
#pragma unroll
    for (int i = 0; i < 25; i++) s[i] = 0;
#pragma unroll 1
    for (u32 mi = w0; mi < w1; mi++) {
      const u32 w = ct.widths[mi];
#pragma unroll 1
      for (u32 c0 = 0; c0 < w; c0 += 17) {
#pragma unroll
        for (int k = 0; k < 17; k++) s[k] = (c0 + k < w) ? row[c0 + k] : 0;
        kk::f1600(s);
      }
      row += w;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) out[i] = s[i];
  } else {  // Poseidon2 / RPO / RPX: overwrite-mode sponge, rate 8; the permutation stands once, in the inner loop
    u64 s[12];
#pragma unroll
    for (int i = 0; i < 12; i++) s[i] = 0;
#pragma unroll 1
    for (u32 mi = w0; mi < w1; mi++) {
      const u32 w = ct.widths[mi];
#pragma unroll 1
      for (u32 c0 = 0; c0 < w; c0 += 8) {
#pragma unroll
        for (int k = 0; k < 8; k++) s[k] = (c0 + k < w) ? row[c0 + k] : 0;
        vb_permute<H>(s);
      }
      row += w;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) out[i] = s[i];
  }
}

template <int H>
__device__ __forceinline__ void vb_compress(const u64 l[4], const u64 r[4], u64 o[4]) {
  if constexpr (H == MH_LMCS_BLAKE3) {
    uint32_t a[8], b[8], d[8];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      a[2 * i] = (uint32_t)l[i]; a[2 * i + 1] = (uint32_t)(l[i] >> 32);
      b[2 * i] = (uint32_t)r[i]; b[2 * i + 1] = (uint32_t)(r[i] >> 32);
    }
    b3::compress_pair(a, b, d);
#pragma unroll
    for (int i = 0; i < 4; i++) o[i] = (u64)d[2 * i] | ((u64)d[2 * i + 1] << 32);
  } else if constexpr (H == MH_LMCS_KECCAK) {
    kk::compress_pair(l, r, o);
  } else {
    u64 s[12] = {l[0], l[1], l[2], l[3], r[0], r[1], r[2], r[3], 0, 0, 0, 0};
    vb_permute<H>(s);
#pragma unroll
    for (int i = 0; i < 4; i++) o[i] = s[i];
  }
}

template <int H>
__global__ __launch_bounds__(VB_THREADS) void k_vfy_leaves(VbLeafArgs a, VbClasses ct) {
  const u32 g = blockIdx.x * VB_THREADS + threadIdx.x;
  // the wave's class: wave-uniform, so the table is read with scalar loads from the argument segment
  const u32 wave = __builtin_amdgcn_readfirstlane(g >> 6);
  u32 k = 0;
  while (k + 1 < ct.n_classes && wave >= ct.wave0[k + 1]) k++;
  if (g >= a.n_lanes) return;
  const u64 off = a.row_off[g];
  if (off == VB_NO_LEAF) return;
  u64 d[4];
  vb_leaf<H>(a.fields + off, ct, ct.w_off[k], ct.w_off[k + 1], d);
  ulonglong2* o = reinterpret_cast<ulonglong2*>(a.digests + 4 * (size_t)a.out_slot[g]);
  o[0] = make_ulonglong2(d[0], d[1]);
  o[1] = make_ulonglong2(d[2], d[3]);
}

template <int H>
__global__ __launch_bounds__(VB_THREADS) void k_vfy_paths(VbPathArgs a) {
  extern __shared__ __attribute__((aligned(16))) u64 vb_lds[];  // two arrays of lds_slots digests
  const VbOpening op = a.ops[blockIdx.x];
  u64* cur = vb_lds;
  u64* nxt = vb_lds + 4 * (size_t)a.lds_slots;
  for (u32 q = threadIdx.x; q < op.n_leaves; q += VB_THREADS) {
    const ulonglong2* s = reinterpret_cast<const ulonglong2*>(a.digests + 4 * (size_t)(op.leaf0 + q));
    ulonglong2* t = reinterpret_cast<ulonglong2*>(cur + 4 * q);
    t[0] = s[0];
    t[1] = s[1];
  }
  __syncthreads();
  const u32* lvl = a.lvl + op.lvl0;
  const u64* sibs = a.sibs + 4 * op.sib0;
#pragma unroll 1
  for (u32 l = 0; l < op.depth; l++) {
    const u32 p0 = lvl[l], p1 = lvl[l + 1];
#pragma unroll 1
    for (u32 p = p0 + threadIdx.x; p < p1; p += VB_THREADS) {
      const u32 ls = a.pairs[2 * (size_t)(op.pair0 + p)], rs = a.pairs[2 * (size_t)(op.pair0 + p) + 1];
      const u64* lp = (ls & lmcs_plan::SIBLING) ? sibs + 4 * (size_t)(ls & ~lmcs_plan::SIBLING) : cur + 4 * ls;
      const u64* rp = (rs & lmcs_plan::SIBLING) ? sibs + 4 * (size_t)(rs & ~lmcs_plan::SIBLING) : cur + 4 * rs;
      u64 L[4], R[4], O[4];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        L[i] = lp[i];
        R[i] = rp[i];
      }
      vb_compress<H>(L, R, O);
#pragma unroll
      for (int i = 0; i < 4; i++) nxt[4 * (p - p0) + i] = O[i];
    }
    __syncthreads();
    u64* t = cur;
    cur = nxt;
    nxt = t;
  }
  if (threadIdx.x == 0)  // a tree of depth 0 has no level: the leaf digest itself
    a.ok[blockIdx.x] = (cur[0] == op.root[0] && cur[1] == op.root[1] && cur[2] == op.root[2] && cur[3] == op.root[3]) ? 1 : 0;
}

// The witness form of k_vfy_paths (mh_lmcs_witness_batch): the same walk, and what it derives is kept.  Per level
// every computed parent goes to the pass-wide `nodes` array (plan order: parent p of the opening is node pair0 + p) as well as to LDS,
// and every opened leaf q follows its ancestor slot through parent_of (lmcs_plan::PathTable) and copies the OTHER source of its
// parent's pair -- an LDS slot of the level below or a streamed sibling -- to paths[q][l].  Both read the array of the level below and
// write elsewhere, so the level's one barrier serves both.  At most 1024 leaves on 256 lanes: four ancestor slots per lane, in
// registers.  Global writes are 16-byte vector stores.
struct VbWitOpening {  // 16 bytes
  u64 path0;  // first digest of this opening in `paths` (n_leaves x depth digests per opening)
  u32 par0;   // first of its parent_of entries
  u32 pad;
};
struct VbWitArgs {
  const VbWitOpening* wops;
  const u32* parent_of;
  u64* nodes;  // [parents of the pass][4]
  u64* paths;
};
static_assert(VB_MAX_LEAVES == 4 * VB_THREADS, "k_vfy_witness keeps four ancestor slots per lane");

template <int H>
__global__ __launch_bounds__(VB_THREADS) void k_vfy_witness(VbPathArgs a, VbWitArgs w) {
  extern __shared__ __attribute__((aligned(16))) u64 vb_lds[];  // two arrays of lds_slots digests
  const VbOpening op = a.ops[blockIdx.x];
  const VbWitOpening wo = w.wops[blockIdx.x];
  u64* cur = vb_lds;
  u64* nxt = vb_lds + 4 * (size_t)a.lds_slots;
  for (u32 q = threadIdx.x; q < op.n_leaves; q += VB_THREADS) {
    const ulonglong2* s = reinterpret_cast<const ulonglong2*>(a.digests + 4 * (size_t)(op.leaf0 + q));
    ulonglong2* t = reinterpret_cast<ulonglong2*>(cur + 4 * q);
    t[0] = s[0];
    t[1] = s[1];
  }
  __syncthreads();
  const u32* lvl = a.lvl + op.lvl0;
  const u64* sibs = a.sibs + 4 * op.sib0;
  const u32* par = w.parent_of + wo.par0;  // the slots of the current level: n_slots entries
  u32 n_slots = op.n_leaves;
  u32 anc[4];
#pragma unroll
  for (int j = 0; j < 4; j++) anc[j] = threadIdx.x + j * VB_THREADS;
#pragma unroll 1
  for (u32 l = 0; l < op.depth; l++) {
    const u32 p0 = lvl[l], p1 = lvl[l + 1];
#pragma unroll 1
    for (u32 p = p0 + threadIdx.x; p < p1; p += VB_THREADS) {
      const u32 ls = a.pairs[2 * (size_t)(op.pair0 + p)], rs = a.pairs[2 * (size_t)(op.pair0 + p) + 1];
      const u64* lp = (ls & lmcs_plan::SIBLING) ? sibs + 4 * (size_t)(ls & ~lmcs_plan::SIBLING) : cur + 4 * ls;
      const u64* rp = (rs & lmcs_plan::SIBLING) ? sibs + 4 * (size_t)(rs & ~lmcs_plan::SIBLING) : cur + 4 * rs;
      u64 L[4], R[4], O[4];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        L[i] = lp[i];
        R[i] = rp[i];
      }
      vb_compress<H>(L, R, O);
#pragma unroll
      for (int i = 0; i < 4; i++) nxt[4 * (p - p0) + i] = O[i];
      ulonglong2* g = reinterpret_cast<ulonglong2*>(w.nodes + 4 * (size_t)(op.pair0 + p));
      g[0] = make_ulonglong2(O[0], O[1]);
      g[1] = make_ulonglong2(O[2], O[3]);
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const u32 q = threadIdx.x + j * VB_THREADS;
      if (q < op.n_leaves) {
        const u32 pr = par[anc[j]];
        const size_t e = 2 * (size_t)(op.pair0 + p0 + pr);
        const u32 ls = a.pairs[e], rs = a.pairs[e + 1];
        const u32 o = ls == anc[j] ? rs : ls;
        const u64* src = (o & lmcs_plan::SIBLING) ? sibs + 4 * (size_t)(o & ~lmcs_plan::SIBLING) : cur + 4 * o;
        ulonglong2* g = reinterpret_cast<ulonglong2*>(w.paths + 4 * (wo.path0 + (size_t)q * op.depth + l));
        g[0] = make_ulonglong2(src[0], src[1]);
        g[1] = make_ulonglong2(src[2], src[3]);
        anc[j] = pr;
      }
    }
    par += n_slots;
    n_slots = p1 - p0;
    __syncthreads();
    u64* t = cur;
    cur = nxt;
    nxt = t;
  }
  if (threadIdx.x == 0)
    a.ok[blockIdx.x] = (cur[0] == op.root[0] && cur[1] == op.root[1] && cur[2] == op.root[2] && cur[3] == op.root[3]) ? 1 : 0;
}

template <int H>
void launch_witness(mh_ctx* c, unsigned blocks, size_t lds, const VbPathArgs& a, const VbWitArgs& w) {
  MH_LAUNCH(k_vfy_witness<H>, dim3(blocks), dim3(VB_THREADS), lds, c->stream, a, w);
}
void dispatch_witness(mh_ctx* c, int lmcs, unsigned blocks, size_t lds, const VbPathArgs& a, const VbWitArgs& w) {
  switch (lmcs) {
    case MH_LMCS_POSEIDON2: return launch_witness<MH_LMCS_POSEIDON2>(c, blocks, lds, a, w);
    case MH_LMCS_BLAKE3: return launch_witness<MH_LMCS_BLAKE3>(c, blocks, lds, a, w);
    case MH_LMCS_KECCAK: return launch_witness<MH_LMCS_KECCAK>(c, blocks, lds, a, w);
    case MH_LMCS_RPO: return launch_witness<MH_LMCS_RPO>(c, blocks, lds, a, w);
    case MH_LMCS_RPX: return launch_witness<MH_LMCS_RPX>(c, blocks, lds, a, w);
    default: throw MhError(MH_ERR_INTERNAL, "no witness kernel for this LMCS id");
  }
}

template <int H>
void launch_leaves(mh_ctx* c, unsigned blocks, const VbLeafArgs& a, const VbClasses& ct) {
  MH_LAUNCH(k_vfy_leaves<H>, dim3(blocks), dim3(VB_THREADS), 0, c->stream, a, ct);
}
template <int H>
void launch_paths(mh_ctx* c, unsigned blocks, size_t lds, const VbPathArgs& a) {
  MH_LAUNCH(k_vfy_paths<H>, dim3(blocks), dim3(VB_THREADS), lds, c->stream, a);
}
void dispatch_leaves(mh_ctx* c, int lmcs, unsigned blocks, const VbLeafArgs& a, const VbClasses& ct) {
  switch (lmcs) {
    case MH_LMCS_POSEIDON2: return launch_leaves<MH_LMCS_POSEIDON2>(c, blocks, a, ct);
    case MH_LMCS_BLAKE3: return launch_leaves<MH_LMCS_BLAKE3>(c, blocks, a, ct);
    case MH_LMCS_KECCAK: return launch_leaves<MH_LMCS_KECCAK>(c, blocks, a, ct);
    case MH_LMCS_RPO: return launch_leaves<MH_LMCS_RPO>(c, blocks, a, ct);
    case MH_LMCS_RPX: return launch_leaves<MH_LMCS_RPX>(c, blocks, a, ct);
    default: throw MhError(MH_ERR_INTERNAL, "no leaf kernel for this LMCS id");  // a missing kernel is an error, never a host fallback
  }
}
void dispatch_paths(mh_ctx* c, int lmcs, unsigned blocks, size_t lds, const VbPathArgs& a) {
  switch (lmcs) {
    case MH_LMCS_POSEIDON2: return launch_paths<MH_LMCS_POSEIDON2>(c, blocks, lds, a);
    case MH_LMCS_BLAKE3: return launch_paths<MH_LMCS_BLAKE3>(c, blocks, lds, a);
    case MH_LMCS_KECCAK: return launch_paths<MH_LMCS_KECCAK>(c, blocks, lds, a);
    case MH_LMCS_RPO: return launch_paths<MH_LMCS_RPO>(c, blocks, lds, a);
    case MH_LMCS_RPX: return launch_paths<MH_LMCS_RPX>(c, blocks, lds, a);
    default: throw MhError(MH_ERR_INTERNAL, "no path kernel for this LMCS id");
  }
}

typedef lmcs_plan::Opening Opening;

// the kernels' bounds: "" if the opening fits them
std::string device_bounds(const Opening& op) {
  if (op.plan.n_leaves > VB_MAX_LEAVES) return "more than 1024 distinct opened leaves in one opening (the path kernel's bound)";
  if (op.hashed.size() > (size_t)VB_MAX_WIDTHS) return "more than 512 matrices in one tree (the leaf kernel's class table)";
  for (u32 w : op.hashed)
    if (w > VB_MAX_WIDTH) return "a matrix wider than 32764 cells (the leaf kernel's bound)";
  return "";
}

size_t pass_bytes(const Opening& op) {  // device memory one opening takes in a pass
  const size_t lanes = op.plan.n_leaves + 63;
  return 8 * op.plan.n_leaves * op.row_len + 32 * op.plan.n_siblings + 32 * op.plan.n_leaves + 4 * op.plan.pairs.size() +
         4 * op.plan.level_off.size() + sizeof(VbOpening) + 12 * lanes + 4;
}
size_t witness_bytes(const Opening& op) {  // ... and what a witness pass adds: nodes, paths, parent_of, its descriptor
  const size_t n_par = op.plan.depth ? op.plan.n_leaves + op.plan.n_nodes() - 1 : 0;
  return 32 * op.plan.n_nodes() + 32 * op.plan.n_leaves * (size_t)op.plan.depth + 4 * n_par + sizeof(VbWitOpening);
}
size_t batch_bytes_limit() {
  const char* e = getenv("MH_VERIFY_BATCH_BYTES");
  if (e && *e) {
    const unsigned long long v = strtoull(e, nullptr, 10);
    if (v > 0) return (size_t)v;
  }
  return (size_t)256 << 20;
}

struct Upload {
  DevBuf buf;
  template <class T>
  const T* put(mh_ctx* c, const std::vector<T>& v) {
    buf.alloc(std::max<size_t>(v.size() * sizeof(T), 16));
    c->h2d(buf.p, v.data(), v.size() * sizeof(T));
    return (const T*)buf.p;
  }
};

// Where a witness pass leaves its arrays, per opening of ops: in the caller's buffers (`outs`: mh_lmcs_witness_batch), or where they
// landed -- the read-back block of the pass is kept whole in `blocks` and where[i] points into it (mh_verify_batch_witness).
struct WitnessDst {
  const mh_lmcs_witness_out* outs = nullptr;
  std::vector<std::unique_ptr<u64[]>>* blocks = nullptr;
  std::vector<mh_lmcs_witness_out>* where = nullptr;
};

// one pass: ops[first .. last) hashed and compared; ok[i - first] = verdict.  With outs (or null) the pass runs the witness kernel, and
// one read-back brings verdicts, leaf digests, paths and nodes.
void run_pass(mh_ctx* c, int lmcs, const std::vector<const Opening*>& ops, size_t first, size_t last, int* ok, const WitnessDst* outs) {
  const size_t n = last - first;
  std::vector<u64> fields, sibs, row_off;
  std::vector<u32> out_slot, pairs, lvl, parent_of;
  std::vector<VbOpening> desc(n);
  std::vector<VbWitOpening> wdesc(outs ? n : 0);
  size_t n_paths = 0;
  std::map<std::vector<u32>, std::vector<size_t>> classes;  // widths -> openings of the pass
  std::vector<size_t> field0(n);
  size_t n_leaves = 0, n_fields = 0, n_sibs = 0, n_pairs = 0, n_lvl = 0;
  u32 max_leaves = 1;
  for (size_t i = 0; i < n; i++) {
    const Opening& op = *ops[first + i];
    n_fields += op.plan.n_leaves * op.row_len;
    n_sibs += op.plan.n_siblings;
    n_pairs += op.plan.pairs.size();
    n_lvl += op.plan.level_off.size();
    n_leaves += op.plan.n_leaves;
  }
  MH_REQUIRE(n_leaves < ((size_t)1 << 31) && n_pairs < ((size_t)1 << 32) && n_sibs < ((size_t)1 << 31),
             "verify batch: a pass this large needs a smaller MH_VERIFY_BATCH_BYTES");
  fields.reserve(n_fields);
  sibs.reserve(4 * n_sibs);
  pairs.reserve(n_pairs);
  lvl.reserve(n_lvl);
  u32 leaf0 = 0;
  for (size_t i = 0; i < n; i++) {
    const Opening& op = *ops[first + i];
    VbOpening& d = desc[i];
    for (int k = 0; k < 4; k++) d.root[k] = op.root[k];
    d.sib0 = sibs.size() / 4;
    d.leaf0 = leaf0;
    d.n_leaves = (u32)op.plan.n_leaves;
    d.pair0 = (u32)(pairs.size() / 2);
    d.lvl0 = (u32)lvl.size();
    d.depth = (u32)op.plan.depth;
    d.pad = 0;
    field0[i] = fields.size();
    fields.insert(fields.end(), op.rows, op.rows + op.plan.n_leaves * op.row_len);
    if (op.plan.n_siblings) sibs.insert(sibs.end(), op.sibs, op.sibs + 4 * op.plan.n_siblings);
    pairs.insert(pairs.end(), op.plan.pairs.begin(), op.plan.pairs.end());
    lvl.insert(lvl.end(), op.plan.level_off.begin(), op.plan.level_off.end());
    leaf0 += d.n_leaves;
    max_leaves = std::max(max_leaves, d.n_leaves);
    classes[op.hashed].push_back(i);
    if (outs) {
      lmcs_plan::PathTable pt;
      lmcs_plan::build_paths(op.plan, pt);
      wdesc[i] = VbWitOpening{(u64)n_paths, (u32)parent_of.size(), 0};
      parent_of.insert(parent_of.end(), pt.parent_of.begin(), pt.parent_of.end());
      n_paths += op.plan.n_leaves * (size_t)op.plan.depth;
    }
  }
  // lanes: class after class, each padded to whole waves; launches of at most VB_MAX_CLASSES classes / VB_MAX_WIDTHS widths
  struct Launch {
    VbClasses ct;
    size_t lane0, lanes;
  };
  std::vector<Launch> launches;
  {
    Launch cur{};
    cur.lane0 = 0;
    u32 n_w = 0;
    auto flush = [&]() {
      if (!cur.ct.n_classes) return;
      cur.lanes = row_off.size() - cur.lane0;
      launches.push_back(cur);
      cur = Launch{};
      cur.lane0 = row_off.size();
      n_w = 0;
    };
    for (auto& kv : classes) {
      const std::vector<u32>& w = kv.first;
      if (cur.ct.n_classes == VB_MAX_CLASSES || n_w + w.size() > (size_t)VB_MAX_WIDTHS) flush();
      const u32 k = cur.ct.n_classes++;
      cur.ct.wave0[k] = (u32)((row_off.size() - cur.lane0) / 64);
      cur.ct.w_off[k] = n_w;
      for (u32 x : w) cur.ct.widths[n_w++] = x;
      cur.ct.w_off[k + 1] = n_w;
      for (size_t i : kv.second) {
        const Opening& op = *ops[first + i];
        for (size_t q = 0; q < op.plan.n_leaves; q++) {
          row_off.push_back(field0[i] + q * op.row_len);
          out_slot.push_back(desc[i].leaf0 + (u32)q);
        }
      }
      while (row_off.size() % 64) {
        row_off.push_back(VB_NO_LEAF);
        out_slot.push_back(0);
      }
      cur.ct.wave0[k + 1] = (u32)((row_off.size() - cur.lane0) / 64);
    }
    flush();
  }
  Upload u_fields, u_sibs, u_rows, u_slots, u_pairs, u_lvl, u_desc, u_par, u_wdesc;
  // a witness pass reads back one buffer: [leaf digests | nodes | paths | verdicts]
  const size_t n_nodes = n_pairs / 2, back_words = 4 * (n_leaves + n_nodes + n_paths) + (n + 1) / 2;
  DevBuf digests(outs ? 8 * back_words : 32 * (size_t)n_leaves), d_ok(outs ? 16 : 4 * n);
  VbLeafArgs la{};
  VbPathArgs pa{};
  {
    ProfScope ps(c, "vfy_upload", 8.0 * fields.size() + 8.0 * sibs.size());
    la.fields = u_fields.put(c, fields);
    pa.sibs = u_sibs.put(c, sibs);
    la.row_off = u_rows.put(c, row_off);
    la.out_slot = u_slots.put(c, out_slot);
    pa.pairs = u_pairs.put(c, pairs);
    pa.lvl = u_lvl.put(c, lvl);
    pa.ops = u_desc.put(c, desc);
  }
  VbWitArgs wa{};
  if (outs) {
    wa.parent_of = u_par.put(c, parent_of);
    wa.wops = u_wdesc.put(c, wdesc);
    wa.nodes = digests.u() + 4 * n_leaves;
    wa.paths = wa.nodes + 4 * n_nodes;
  }
  la.digests = digests.u();
  {
    ProfScope ps(c, "vfy_leaves");
    for (const Launch& l : launches) {
      VbLeafArgs a = la;
      a.row_off += l.lane0;
      a.out_slot += l.lane0;
      a.n_lanes = (u32)l.lanes;
      dispatch_leaves(c, lmcs, (unsigned)((l.lanes + VB_THREADS - 1) / VB_THREADS), a, l.ct);
    }
  }
  pa.digests = digests.u();
  pa.ok = outs ? (int*)(wa.paths + 4 * n_paths) : (int*)d_ok.p;
  pa.lds_slots = max_leaves;
  if (!outs) {
    {
      ProfScope ps(c, "vfy_paths");
      dispatch_paths(c, lmcs, (unsigned)n, 2 * 32 * (size_t)max_leaves, pa);
    }
    c->d2h(ok, d_ok.p, 4 * n);  // the one read-back (waits for the stream: the host vectors above may go)
    return;
  }
  {
    ProfScope ps(c, "vfy_witness");
    dispatch_witness(c, lmcs, (unsigned)n, 2 * 32 * (size_t)max_leaves, pa, wa);
  }
  std::unique_ptr<u64[]> back(new u64[back_words]);  // not zero-filled: every word is read back
  {
    ProfScope ps(c, "vfy_readback", 8.0 * back_words);
    c->d2h(back.get(), digests.p, 8 * back_words);  // the one read-back
  }
  memcpy(ok, back.get() + 4 * (n_leaves + n_nodes + n_paths), 4 * n);
  // a rejected opening's arrays are dropped here: its buffers stay as the caller left them
  for (size_t i = 0; i < n; i++) {
    if (!ok[i]) continue;
    const Opening& op = *ops[first + i];
    u64* leaf = back.get() + 4 * (size_t)desc[i].leaf0;
    u64* path = back.get() + 4 * (n_leaves + n_nodes + (size_t)wdesc[i].path0);
    u64* node = back.get() + 4 * (n_leaves + (size_t)desc[i].pair0);
    if (outs->where) {
      (*outs->where)[first + i] = mh_lmcs_witness_out{leaf, path, node};
      continue;
    }
    const mh_lmcs_witness_out& o = outs->outs[first + i];
    const size_t k = op.plan.n_leaves;
    memcpy(o.leaf_digests, leaf, 32 * k);
    if (op.plan.depth) memcpy(o.paths, path, 32 * k * (size_t)op.plan.depth);
    if (o.nodes && op.plan.depth) memcpy(o.nodes, node, 32 * op.plan.n_nodes());
  }
  if (outs->blocks) outs->blocks->push_back(std::move(back));
}

// every opening of ops (all within the kernels' bounds) on the device, in passes of at most MH_VERIFY_BATCH_BYTES
void run_device(mh_ctx* c, int lmcs, const std::vector<const Opening*>& ops, std::vector<int>& ok, const WitnessDst* outs = nullptr) {
  ok.assign(ops.size(), 0);
  const size_t limit = batch_bytes_limit();
  auto cost = [&](const Opening& op) { return pass_bytes(op) + (outs ? witness_bytes(op) : 0); };
  for (size_t first = 0; first < ops.size();) {
    size_t last = first, bytes = 0;
    while (last < ops.size() && (last == first || bytes + cost(*ops[last]) <= limit)) bytes += cost(*ops[last++]);
    run_pass(c, lmcs, ops, first, last, ok.data() + first, outs);
    first = last;
  }
}

void prof_host(mh_ctx* c, const char* name, double ms) {
  if (!c->prof_on || !(c->prof_only.empty() || c->prof_only == name)) return;
  ProfEntry& e = c->prof[name];
  e.ms += ms;
  e.count += 1;
}

}  // namespace

#define VB_TRY(ctx_expr) mh_ctx* _c = (ctx_expr); PoolScope _ps(_c); try {
#define VB_CATCH                              \
  }                                           \
  catch (const MhError& e) {                  \
    if (_c) _c->err = e.what();               \
    return e.code;                            \
  }                                           \
  catch (const std::exception& e) {           \
    if (_c) _c->err = e.what();               \
    return MH_ERR_INTERNAL;                   \
  }                                           \
  return MH_OK;

extern "C" {

int mh_lmcs_verify_batch(mh_ctx* c, int lmcs, int salt_elems, size_t n, const mh_lmcs_opening* items, int* ok) {
  VB_TRY(c)
  MH_REQUIRE(c, "null context");
  MH_REQUIRE((items && ok) || !n, "null argument");
  MH_REQUIRE(lmcs >= MH_LMCS_POSEIDON2 && lmcs <= MH_LMCS_RPX, "unknown LMCS hasher id");
  MH_REQUIRE(salt_elems >= 0 && salt_elems <= MH_MAX_SALT_ELEMS, "salt_elems must be in 0..MH_MAX_SALT_ELEMS");
  if (!n) return MH_OK;
  std::vector<Opening> prepared(n);
  std::vector<const Opening*> ops;
  std::vector<size_t> who;
  for (size_t i = 0; i < n; i++) {
    std::string why;
    ok[i] = 0;
    if (!lmcs_verify::prepare(lmcs, salt_elems, items[i], prepared[i], why)) continue;  // refused on the host: verdict 0
    const std::string bound = device_bounds(prepared[i]);
    MH_REQUIRE(bound.empty(), "mh_lmcs_verify_batch: opening " + std::to_string(i) + " has " + bound + ": use mh_lmcs_verify");
    ops.push_back(&prepared[i]);
    who.push_back(i);
  }
  if (ops.empty()) return MH_OK;
  HIP_CHECK(hipSetDevice(c->device));
  std::vector<int> verdict;
  run_device(c, lmcs, ops, verdict);
  for (size_t k = 0; k < ops.size(); k++) ok[who[k]] = verdict[k];
  VB_CATCH
}

int mh_lmcs_witness_batch(mh_ctx* c, int lmcs, int salt_elems, size_t n, const mh_lmcs_opening* items, const mh_lmcs_witness_out* outs, int* ok) {
  VB_TRY(c)
  MH_REQUIRE(c, "null context");
  MH_REQUIRE((items && outs && ok) || !n, "null argument");
  MH_REQUIRE(lmcs >= MH_LMCS_POSEIDON2 && lmcs <= MH_LMCS_RPX, "unknown LMCS hasher id");
  MH_REQUIRE(salt_elems >= 0 && salt_elems <= MH_MAX_SALT_ELEMS, "salt_elems must be in 0..MH_MAX_SALT_ELEMS");
  if (!n) return MH_OK;
  std::vector<Opening> prepared(n);
  std::vector<const Opening*> ops;
  std::vector<mh_lmcs_witness_out> dst;
  std::vector<size_t> who;
  for (size_t i = 0; i < n; i++) {
    std::string why;
    ok[i] = 0;
    if (!lmcs_verify::prepare(lmcs, salt_elems, items[i], prepared[i], why)) continue;  // refused on the host: verdict 0, buffers untouched
    const std::string bound = device_bounds(prepared[i]);
    MH_REQUIRE(bound.empty(), "mh_lmcs_witness_batch: opening " + std::to_string(i) + " has " + bound + ": use mh_lmcs_witness");
    MH_REQUIRE(outs[i].leaf_digests && (outs[i].paths || !prepared[i].plan.depth), "mh_lmcs_witness_batch: null output buffer");
    ops.push_back(&prepared[i]);
    dst.push_back(outs[i]);
    who.push_back(i);
  }
  if (ops.empty()) return MH_OK;
  HIP_CHECK(hipSetDevice(c->device));
  std::vector<int> verdict;
  WitnessDst w;
  w.outs = dst.data();
  run_device(c, lmcs, ops, verdict, &w);
  for (size_t k = 0; k < ops.size(); k++) ok[who[k]] = verdict[k];
  VB_CATCH
}

// mh_verify_batch, and with `out` mh_verify_batch_witness: the same replay and the same verdicts, the device pass in its witness form
static int verify_batch_impl(mh_ctx* c, int lmcs, int salt_elems, const mh_pcs_params* params, int n_airs, const uint64_t* const* air_blobs,
                             const size_t* air_blob_words, const uint64_t challenger_state[12], mh_external_assertions external, size_t n_items,
                             const mh_verify_item* items, mh_verify_result* results, mh_witness_set** out) {
  VB_TRY(c)
  MH_REQUIRE(c, "null context");
  MH_REQUIRE(params && air_blobs && air_blob_words && challenger_state, "null argument");
  MH_REQUIRE((items && results) || !n_items, "null argument");
  MH_REQUIRE(n_airs > 0 && n_airs <= 256, "need between 1 and 256 AIR instances");
  MH_REQUIRE(lmcs >= MH_LMCS_POSEIDON2 && lmcs <= MH_LMCS_RPX, "unknown LMCS hasher id");
  MH_REQUIRE(salt_elems >= 0 && salt_elems <= MH_MAX_SALT_ELEMS, "salt_elems must be in 0..MH_MAX_SALT_ELEMS");
  std::unique_ptr<mh_witness_set> set(out ? new mh_witness_set : nullptr);
  if (!n_items) {
    if (out) *out = set.release();
    return MH_OK;
  }
  std::vector<DagIR> airs;
  for (int i = 0; i < n_airs; i++) airs.push_back(dag_parse(air_blobs[i], air_blob_words[i]));
  struct Replay {
    int code = MH_ERR_INTERNAL;
    std::string reason;
    u64 digest[4] = {0, 0, 0, 0};
    std::vector<Opening> openings;
    std::vector<std::string> labels;
  };
  std::vector<Replay> rp(n_items);
  // ---- host replay of every item, up to 16 threads ----
  const auto t0 = std::chrono::steady_clock::now();
  {
    std::atomic<size_t> next{0};
    auto work = [&]() {
      for (size_t i; (i = next.fetch_add(1)) < n_items;) {
        Replay& r = rp[i];
        r.code = verify_replay_recording(lmcs, salt_elems, *params, airs, challenger_state, external, items[i], r.openings, r.labels, r.digest,
                                         r.reason);
        for (const Opening& op : r.openings) {
          const std::string bound = device_bounds(op);
          if (!bound.empty()) {
            r.code = MH_ERR_INVALID;
            r.reason = "proof rejected: " + bound + ": verify it with mh_verify_hiding";
            r.openings.clear();
            r.labels.clear();
            break;
          }
        }
      }
    };
    const unsigned hw = std::thread::hardware_concurrency();
    const size_t want = std::min<size_t>(std::min<size_t>(16, hw ? hw : 1), n_items);
    std::vector<std::thread> pool;
    try {
      for (size_t t = 1; t < want; t++) pool.emplace_back(work);
    } catch (...) {  // no more threads to be had: the calling thread does the rest
    }
    work();
    for (auto& t : pool) t.join();
  }
  prof_host(c, "vfy_replay", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  // ---- one device pass over every recorded opening.  An item whose replay failed keeps the openings recorded BEFORE the failure:
  // they come earlier in the proof, so a bad one among them is what mh_verify_hiding reports (a damaged row fails its tree's root
  // there, and only here, with the hashing postponed, the algebra behind it).  Most rejected items recorded none. ----
  std::vector<const Opening*> ops;
  std::vector<std::pair<size_t, size_t>> who;  // (item, opening of the item)
  for (size_t i = 0; i < n_items; i++)
    for (size_t k = 0; k < rp[i].openings.size(); k++) {
      ops.push_back(&rp[i].openings[k]);
      who.push_back({i, k});
    }
  std::vector<int> verdict;
  std::vector<mh_lmcs_witness_out> where(out ? ops.size() : 0);  // an accepted opening's arrays, in the set's read-back blocks
  WitnessDst w;
  if (out) {
    w.blocks = &set->blocks;
    w.where = &where;
  }
  if (!ops.empty()) {
    HIP_CHECK(hipSetDevice(c->device));
    run_device(c, lmcs, ops, verdict, out ? &w : nullptr);
  }
  for (size_t k = ops.size(); k-- > 0;)  // backwards: the first failed opening of an item names it
    if (!verdict[k]) {
      Replay& r = rp[who[k].first];
      r.code = MH_ERR_INVALID;
      r.reason = "proof rejected: Merkle root mismatch (" + r.labels[who[k].second] + ")";
    }
  for (size_t i = 0; i < n_items; i++) {
    mh_verify_result& o = results[i];
    const bool good = rp[i].code == MH_OK;
    o.code = good ? MH_OK : MH_ERR_INVALID;
    for (int k = 0; k < 4; k++) o.digest[k] = good ? rp[i].digest[k] : 0;
    snprintf(o.reason, sizeof o.reason, "%s", good ? "" : rp[i].reason.c_str());
  }
  if (out) {  // an accepted item's openings, in the order the replay met them = proof order
    set->items.resize(n_items);
    for (size_t k = 0; k < ops.size(); k++) {
      const Replay& r = rp[who[k].first];
      if (r.code != MH_OK) continue;
      const Opening& op = *ops[k];
      mh_witness_set::Tree t;
      int num = 0;
      if (sscanf(r.labels[who[k].second].c_str(), "committed tree %d of", &num) == 1) t.kind = 0;
      else if (sscanf(r.labels[who[k].second].c_str(), "FRI round %d tree", &num) == 1) t.kind = 1;
      else throw MhError(MH_ERR_INTERNAL, "verify batch: an opening of an unnamed tree");
      t.which = num;
      t.depth = op.plan.depth;
      t.row_len = op.row_len;
      for (int j = 0; j < 4; j++) t.root[j] = op.root[j];
      t.indices = op.plan.indices;
      t.rows.assign(op.rows, op.rows + op.plan.n_leaves * op.row_len);
      t.n_nodes = op.plan.n_nodes();
      t.leaf_digests = where[k].leaf_digests;
      t.paths = where[k].paths;
      t.nodes = where[k].nodes;
      set->items[who[k].first].push_back(std::move(t));
    }
    *out = set.release();
  }
  VB_CATCH
}

int mh_verify_batch(mh_ctx* c, int lmcs, int salt_elems, const mh_pcs_params* params, int n_airs, const uint64_t* const* air_blobs,
                    const size_t* air_blob_words, const uint64_t challenger_state[12], mh_external_assertions external, size_t n_items,
                    const mh_verify_item* items, mh_verify_result* results) {
  return verify_batch_impl(c, lmcs, salt_elems, params, n_airs, air_blobs, air_blob_words, challenger_state, external, n_items, items, results,
                           nullptr);
}

int mh_verify_batch_witness(mh_ctx* c, int lmcs, int salt_elems, const mh_pcs_params* params, int n_airs, const uint64_t* const* air_blobs,
                            const size_t* air_blob_words, const uint64_t challenger_state[12], mh_external_assertions external, size_t n_items,
                            const mh_verify_item* items, mh_verify_result* results, mh_witness_set** out) {
  if (!out) {
    if (c) c->err = "mh_verify_batch_witness: null argument";
    return MH_ERR_INVALID;
  }
  *out = nullptr;
  return verify_batch_impl(c, lmcs, salt_elems, params, n_airs, air_blobs, air_blob_words, challenger_state, external, n_items, items, results,
                           out);
}

size_t mh_witness_set_trees(const mh_witness_set* set, size_t item) { return set && item < set->items.size() ? set->items[item].size() : 0; }

int mh_witness_set_tree(const mh_witness_set* set, size_t item, size_t t, mh_witness_tree* view) {
  if (!set || !view || item >= set->items.size() || t >= set->items[item].size()) return MH_ERR_INVALID;
  const mh_witness_set::Tree& w = set->items[item][t];
  view->kind = w.kind;
  view->which = w.which;
  view->depth = w.depth;
  view->n_leaves = w.indices.size();
  view->n_nodes = w.n_nodes;
  view->row_len = w.row_len;
  for (int j = 0; j < 4; j++) view->root[j] = w.root[j];
  view->indices = w.indices.data();
  view->rows = w.rows.data();
  view->leaf_digests = w.leaf_digests;
  view->paths = w.paths;
  view->nodes = w.nodes;
  return MH_OK;
}

void mh_witness_set_free(mh_witness_set* set) { delete set; }

}  // extern "C"
