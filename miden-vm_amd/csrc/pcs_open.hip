// The polynomial commitment scheme on its own, gfx950: open committed LMCS trees at NP = 1 .. MH_PCS_MAX_POINTS out-of-domain points.
//
// Replaces pcs::open_with_channel (crates/lifted-stark/src/pcs/prover.rs:34-101) for an arbitrary tree list and point count; semantics
// from pcs/deep/interpolate.rs:87-204 (PointQuotients, batch_eval_lifted) and pcs/deep/prover.rs:115-315 (reduce + assemble).  deep.hip
// holds the same three kernels for exactly the STARK's two points (z, z * w_N) -- the measured hot path of mh_prove, which stays on
// them; everything here is reached only through mh_pcs_*, also at NP = 2.  What the two share is pcs_stage.hpp (FRI rounds, query phase).
//
//   k_bary_weights_n<NP>        w[j][r] = x_r / (y_j - x_r): a lane owns ROWS rows, takes the norms of its ROWS * NP denominators and
//                               shares ONE Fermat inversion among them (ROWS = 4 for NP <= 2, 2 above: at most eight norms live).
//   k_ood_partial_n<NP>         ONE pass over coset 0 of a column for all NP points: each LDE felt is loaded once and multiplied into NP
//                               accumulators (the read is what the kernel is for: N points must not cost N passes); 2 NP sums in LDS.
//   k_deep_assemble_n<NP, PL>   neg(x) = sum_i -alpha^(W-1-i) f_i(x) exactly as k_deep_assemble (22-bit limbs, flush every DEEP_FLUSH
//                               columns, one LDE point per lane); the tail inverts NP denominators with one Fermat inversion and sums
//                               Q(x) = sum_j beta^j (f_red(z_j) + neg(x)) / (z_j - x).
// "One coset is enough" (deep.hip's header) does not depend on the points: every term is an exact division, so Q has degree < N_max and
// PL = true assembles it on the first coset as two planes that lde_columns extends; PL = false runs on every coset (B = 1, N < 4,
// MH_DEEP_ALL_COSETS=1).  The column loop is a copy of deep.hip's, not a shared __device__ function: hoisting it out of k_deep_assemble
// would change the code the hot kernel is compiled from, and only a GPU run per change can show that its 1.69 ms did not move.
#include "../../include/midenhip.h"
#include "challenger.hpp"
#include "ctx.hpp"
#include "gl.cuh"
#include "kernels.hpp"
#include "pcs_stage.hpp"
#include <algorithm>
#include <cstring>
#include <memory>

static constexpr int NPMAX = MH_PCS_MAX_POINTS;
struct PtsN {
  e2 v[NPMAX];
};

// ---- barycentric weights ------------------------------------------------------------------------
// w[(j * n + r) * 2 ..] = x_r / (y_j - x_r), r < n, j < NP.  A row past n takes x = 0: its denominator is y_j, nonzero.
template <int NP>
static constexpr int bary_rows() { return NP <= 2 ? 4 : 2; }
template <int NP>
__global__ __launch_bounds__(256) void k_bary_weights_n(const u64* tw, int log_n, u64 g, PtsN y, u64* w) {
  constexpr int ROWS = bary_rows<NP>(), K = ROWS * NP;
  const size_t n = (size_t)1 << log_n;
  const size_t base = (size_t)blockIdx.x * (256 * ROWS) + threadIdx.x;
  const size_t half = n >> 1;
  u64 xs[ROWS], nrm[K], pre[K];
  e2 den[K];
#pragma unroll
  for (int k = 0; k < ROWS; k++) {
    const size_t r = base + (size_t)k * 256;
    u64 x = 0;
    if (r < n) x = gl_mul(g, half ? (r < half ? tw[r] : gl_neg(tw[r - half])) : 1);
    xs[k] = x;
#pragma unroll
    for (int j = 0; j < NP; j++) den[k * NP + j] = e2_sub(y.v[j], e2_make(x));
  }
  u64 run = 1;
#pragma unroll
  for (int i = 0; i < K; i++) {
    nrm[i] = gl_sub(gl_sqr(den[i].c0), gl_mul7(gl_sqr(den[i].c1)));
    pre[i] = run;
    run = gl_mul(run, nrm[i]);
  }
  u64 inv = gl_inv(run);
#pragma unroll
  for (int i = K - 1; i >= 0; i--) {
    const u64 ni = gl_mul(inv, pre[i]);
    inv = gl_mul(inv, nrm[i]);
    const int k = i / NP, j = i % NP;
    const size_t r = base + (size_t)k * 256;
    if (r < n) {
      const u64 s = gl_mul(ni, xs[k]);
      *reinterpret_cast<ulonglong2*>(w + 2 * ((size_t)j * n + r)) = make_ulonglong2(gl_mul(den[i].c0, s), gl_mul(gl_neg(den[i].c1), s));
    }
  }
}

// ---- column dot products against the weights -----------------------------------------------------
// grid = (row chunk, column); partial[(col * chunks + chunk) * 2 NP + 2 j ..] = sum over the chunk of f_col(x_r) * w_j[r] (EF).
static constexpr int OOD_ROWS_PER_BLOCK = 8192;
template <int NP>
__global__ __launch_bounds__(256) void k_ood_partial_n(const u64* lde, int log_n, int log_blowup, const u64* w, u64* partial,
                                                       unsigned chunks) {
  __shared__ u64 red[2 * NP][256];
  const size_t n = (size_t)1 << log_n;
  const size_t col = blockIdx.y, chunk = blockIdx.x;
  const u64* f = lde + ((col << log_blowup) << log_n);  // coset 0 of this column
  const size_t r0 = chunk * OOD_ROWS_PER_BLOCK;
  const size_t r1 = r0 + OOD_ROWS_PER_BLOCK < n ? r0 + OOD_ROWS_PER_BLOCK : n;
  e2 a[NP];
#pragma unroll
  for (int j = 0; j < NP; j++) a[j] = e2_make(0);
  for (size_t r = r0 + threadIdx.x; r < r1; r += 256) {
    const u64 v = f[r];  // read once, used NP times
#pragma unroll
    for (int j = 0; j < NP; j++) {
      const ulonglong2 wj = *reinterpret_cast<const ulonglong2*>(w + 2 * ((size_t)j * n + r));
      a[j] = e2_add(a[j], e2_mulf(e2{wj.x, wj.y}, v));
    }
  }
#pragma unroll
  for (int j = 0; j < NP; j++) {
    red[2 * j][threadIdx.x] = a[j].c0;
    red[2 * j + 1][threadIdx.x] = a[j].c1;
  }
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
#pragma unroll
      for (int k = 0; k < 2 * NP; k++) red[k][threadIdx.x] = gl_add(red[k][threadIdx.x], red[k][threadIdx.x + s]);
    }
    __syncthreads();
  }
  if (threadIdx.x < 2 * NP) partial[(col * chunks + chunk) * (2 * NP) + threadIdx.x] = red[threadIdx.x][0];
}

// One matrix to evaluate at np points, y[j] = z_j^(lift) already lifted to its height; out[j][col].
struct OodJobN {
  const LdeMatrix* m = nullptr;
  e2 y[NPMAX];
  std::vector<e2> out[NPMAX];
};
template <int NP>
static void launch_bary(mh_ctx* c, unsigned blocks, const u64* tw, int log_n, u64 g, const PtsN& y, u64* w) {
  MH_LAUNCH(k_bary_weights_n<NP>, dim3(blocks), dim3(256), 0, c->stream, tw, log_n, g, y, w);
}
template <int NP>
static void launch_ood(mh_ctx* c, dim3 grid, const u64* lde, int log_n, int lb, const u64* w, u64* partial, unsigned chunks) {
  MH_LAUNCH(k_ood_partial_n<NP>, grid, dim3(256), 0, c->stream, lde, log_n, lb, w, partial, chunks);
}
// All matrices in one pass over the host, as deep_ood_eval_batch: every job's kernels are queued, the partial sums of all of them come
// back in ONE blocking copy, and matrices with equal (height, coset, lifted points) share one set of weights.
static void pcs_ood_eval_batch(mh_ctx* c, std::vector<OodJobN>& jobs, int np, int log_blowup) {
  struct Weights {
    int log_n;
    size_t coset0;
    PtsN y;
    DevBuf w;
  };
  std::vector<std::unique_ptr<Weights>> weights;
  struct Slot {
    size_t off = 0, ncol = 0;
    unsigned chunks = 0;
  };
  std::vector<Slot> slots(jobs.size());
  size_t total = 0;
  for (size_t k = 0; k < jobs.size(); k++) {
    const LdeMatrix& m = *jobs[k].m;
    for (int j = 0; j < np; j++) jobs[k].out[j].assign(m.width, e2_make(0));
    if (!m.width) continue;
    const size_t n = (size_t)1 << m.log_n;
    slots[k].ncol = m.width;
    slots[k].chunks = (unsigned)((n + OOD_ROWS_PER_BLOCK - 1) / OOD_ROWS_PER_BLOCK);
    slots[k].off = total;
    total += slots[k].ncol * slots[k].chunks * 2 * np;
  }
  if (!total) return;
  DevBuf partial(total * 8), one;
  for (size_t k = 0; k < jobs.size(); k++) {
    if (!slots[k].ncol) continue;
    const OodJobN& j = jobs[k];
    const LdeMatrix& m = *j.m;
    const int log_n = m.log_n;
    const size_t n = (size_t)1 << log_n;
    const u64 g = gl_mul(gl_lde_shift(log_n + log_blowup), gl_pow(gl_two_adic_generator(log_n + log_blowup), m.coset0));
    const u64* tw = log_n ? c->twiddles(log_n, false) : nullptr;
    if (!tw) {
      if (!one.p) {
        one.alloc(8);
        u64 v = 1;
        c->h2d(one.p, &v, 8);
      }
      tw = one.u();
    }
    ProfScope ps(c, "pcs_ood_eval", (double)n * 8.0 * slots[k].ncol + 32.0 * np * n);
    Weights* w = nullptr;
    for (auto& cand : weights) {
      bool same = cand->log_n == log_n && cand->coset0 == m.coset0;
      for (int q = 0; q < np && same; q++) same = e2_eq(cand->y.v[q], j.y[q]);
      if (same) w = cand.get();
    }
    if (!w) {
      weights.emplace_back(new Weights());
      w = weights.back().get();
      w->log_n = log_n; w->coset0 = m.coset0;
      for (int q = 0; q < NPMAX; q++) w->y.v[q] = q < np ? j.y[q] : e2_make(0);
      w->w.alloc((size_t)np * n * 16);
      const int rows = np <= 2 ? 4 : 2;
      const unsigned blocks = (unsigned)((n + 256 * rows - 1) / (256 * rows));
      switch (np) {
        case 1: launch_bary<1>(c, blocks, tw, log_n, g, w->y, w->w.u()); break;
        case 2: launch_bary<2>(c, blocks, tw, log_n, g, w->y, w->w.u()); break;
        case 3: launch_bary<3>(c, blocks, tw, log_n, g, w->y, w->w.u()); break;
        default: launch_bary<4>(c, blocks, tw, log_n, g, w->y, w->w.u()); break;
      }
    }
    const dim3 grid(slots[k].chunks, (unsigned)slots[k].ncol);
    u64* dst = partial.u() + slots[k].off;
    switch (np) {
      case 1: launch_ood<1>(c, grid, m.lde.u(), log_n, m.log_cosets, w->w.u(), dst, slots[k].chunks); break;
      case 2: launch_ood<2>(c, grid, m.lde.u(), log_n, m.log_cosets, w->w.u(), dst, slots[k].chunks); break;
      case 3: launch_ood<3>(c, grid, m.lde.u(), log_n, m.log_cosets, w->w.u(), dst, slots[k].chunks); break;
      default: launch_ood<4>(c, grid, m.lde.u(), log_n, m.log_cosets, w->w.u(), dst, slots[k].chunks); break;
    }
  }
  std::vector<u64> host(total);
  c->d2h(host.data(), partial.p, total * 8);
  for (size_t k = 0; k < jobs.size(); k++) {
    if (!slots[k].ncol) continue;
    OodJobN& j = jobs[k];
    const LdeMatrix& m = *j.m;
    const int log_n = m.log_n;
    const size_t n = (size_t)1 << log_n;
    const u64 g = gl_mul(gl_lde_shift(log_n + log_blowup), gl_pow(gl_two_adic_generator(log_n + log_blowup), m.coset0));
    const u64 g_inv = gl_inv(g), n_inv = gl_inv((u64)n % GL_P);
    for (int q = 0; q < np; q++) {
      // scaling s(y) = ((y/g)^n - 1)/n
      const e2 s = e2_mulf(e2_sub(e2_exp_pow2(e2_mulf(j.y[q], g_inv), log_n), e2_make(1)), n_inv);
      for (size_t col = 0; col < slots[k].ncol; col++) {
        e2 a = e2_make(0);
        for (unsigned ch = 0; ch < slots[k].chunks; ch++) {
          const u64* p = host.data() + slots[k].off + (col * slots[k].chunks + ch) * 2 * np + 2 * q;
          a = e2_add(a, e2{p[0], p[1]});
        }
        j.out[q][col] = e2_mul(a, s);
      }
    }
  }
}

// ---- DEEP reduce + assemble ----------------------------------------------------------------------
static constexpr int PCS_MAX_MATS = 128;   // one descriptor per matrix travels in the kernel arguments (as DEEP_MAX_MATS)
static constexpr unsigned PCS_FLUSH = 128;  // = DEEP_FLUSH: 128 products of < 2^54 per accumulator stay below 2^61
struct PcsDeepMat {
  const u64* lde;
  u32 width, coef_off;  // coef_off: index of this matrix's first column in the aligned coefficient list
  int log_n;
};
struct PcsDeepArgs {
  PcsDeepMat m[PCS_MAX_MATS];
  int n_mats, log_n, log_blowup;  // log_n = max trace height; log_blowup = coset bits stored
  const u64* negc;                // EF pairs per aligned column
  const u64* tw;                  // w_N^k
  const u64* coset_x;             // [B] g*w_K^j
  PtsN z, fred, bpow;             // the points, f_red(z_j), beta^j
  u64* out;                       // EF pairs, coset-major [B][N]; PLANES: [2][N], c0 plane then c1 plane (grid.y = 1)
};

template <int NP, bool PLANES>
__global__ __launch_bounds__(256) void k_deep_assemble_n(PcsDeepArgs a) {
  const size_t N = (size_t)1 << a.log_n;
  const size_t j = blockIdx.y;
  const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = r < N;
  // neg = sum over columns of cf_col * v_col(r), the modular reduction delayed: deep.hip k_deep_assemble's loop for one point per lane
  // (cf in three 22-bit limbs, v in 32-bit halves, six plain 64-bit accumulators per EF component, one reduction per PCS_FLUSH columns)
  e2 neg = e2_make(0);
  u64 w[2][6];
#pragma unroll
  for (int e = 0; e < 2; e++)
#pragma unroll
    for (int i = 0; i < 6; i++) w[e][i] = 0;
  auto flush = [&]() {
    // weights of the six accumulators mod p: 2^0, 2^22, 2^44, 2^32, 2^54, 2^76 = 2^12 (2^32 - 1)
    const u64 C[6] = {1ULL, 1ULL << 22, 1ULL << 44, 1ULL << 32, 1ULL << 54, GL_EPS << 12};
    u64 s0 = w[0][0], s1 = w[1][0];  // < 2^61: canonical
#pragma unroll
    for (int i = 1; i < 6; i++) {
      s0 = gl_add(s0, gl_mul(w[0][i], C[i]));
      s1 = gl_add(s1, gl_mul(w[1][i], C[i]));
    }
    neg = e2_add(neg, e2{s0, s1});
#pragma unroll
    for (int e = 0; e < 2; e++)
#pragma unroll
      for (int i = 0; i < 6; i++) w[e][i] = 0;
  };
  u32 pending = 0;
#pragma unroll 1
  for (int mi = 0; mi < a.n_mats; mi++) {
    const PcsDeepMat m = a.m[mi];
    const size_t nm_mask = ((size_t)1 << m.log_n) - 1;
    const u64* colp = m.lde + (j << m.log_n);
    const size_t cstride = (size_t)1 << (m.log_n + a.log_blowup);
#pragma unroll 2
    for (u32 cidx = 0; cidx < m.width; cidx++) {
      const u64 cf0 = a.negc[2 * (m.coef_off + cidx)], cf1 = a.negc[2 * (m.coef_off + cidx) + 1];
      u32 al[2][3];
#pragma unroll
      for (int i = 0; i < 3; i++) {
        al[0][i] = (u32)(cf0 >> (22 * i)) & 0x3FFFFFu;
        al[1][i] = (u32)(cf1 >> (22 * i)) & 0x3FFFFFu;
      }
      if (live) {
        const u64 v = colp[r & nm_mask];  // a shorter matrix is read at its own row: f(x^L) on the max domain
        const u32 v0 = (u32)v, v1 = (u32)(v >> 32);
#pragma unroll
        for (int e = 0; e < 2; e++) {
          w[e][0] += (u64)al[e][0] * v0;
          w[e][1] += (u64)al[e][1] * v0;
          w[e][2] += (u64)al[e][2] * v0;
          w[e][3] += (u64)al[e][0] * v1;
          w[e][4] += (u64)al[e][1] * v1;
          w[e][5] += (u64)al[e][2] * v1;
        }
      }
      colp += cstride;
      if (++pending == PCS_FLUSH) {
        flush();
        pending = 0;
      }
    }
  }
  flush();
  // the tail: NP denominators z_j - x, one Fermat inversion for their norms (a lane past N takes x = 0: nonzero denominators)
  const size_t half = N >> 1;
  u64 x = 0;
  if (live) x = gl_mul(a.coset_x[j], half ? (r < half ? a.tw[r] : gl_neg(a.tw[r - half])) : 1);
  e2 den[NP];
  u64 nrm[NP], pre[NP];
  u64 run = 1;
#pragma unroll
  for (int k = 0; k < NP; k++) {
    den[k] = e2_sub(a.z.v[k], e2_make(x));
    nrm[k] = gl_sub(gl_sqr(den[k].c0), gl_mul7(gl_sqr(den[k].c1)));
    pre[k] = run;
    run = gl_mul(run, nrm[k]);
  }
  u64 inv = gl_inv(run);
  e2 q = e2_make(0);
#pragma unroll
  for (int k = NP - 1; k >= 0; k--) {
    const u64 ni = gl_mul(inv, pre[k]);
    inv = gl_mul(inv, nrm[k]);
    const e2 qinv = e2{gl_mul(den[k].c0, ni), gl_mul(gl_neg(den[k].c1), ni)};
    e2 t = e2_mul(qinv, e2_add(a.fred.v[k], neg));
    if (k) t = e2_mul(t, a.bpow.v[k]);  // beta^0 = 1
    q = e2_add(q, t);
  }
  if (live) {
    if constexpr (PLANES) {
      a.out[r] = q.c0;
      a.out[N + r] = q.c1;
    } else {
      *reinterpret_cast<ulonglong2*>(a.out + 2 * ((j << a.log_n) + r)) = make_ulonglong2(q.c0, q.c1);
    }
  }
}

// planes [2][n] (c0 plane, c1 plane; n = B * N points, coset-major) -> EF pairs [n], one point per lane
__global__ __launch_bounds__(256) void k_pcs_interleave(const u64* __restrict__ planes, size_t n, u64* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  *reinterpret_cast<ulonglong2*>(out + 2 * i) = make_ulonglong2(planes[i], planes[n + i]);
}

template <int NP>
static void launch_deep(mh_ctx* c, dim3 grid, const PcsDeepArgs& a, bool planes) {
  if (planes) MH_LAUNCH((k_deep_assemble_n<NP, true>), grid, dim3(256), 0, c->stream, a);
  else MH_LAUNCH((k_deep_assemble_n<NP, false>), grid, dim3(256), 0, c->stream, a);
}
// mats: every matrix of every tree in order; negc: -alpha^(W-1-i) per ALIGNED column index; out: EF pairs coset-major [B][N].
// one_coset as deep_assemble: assemble on the first coset, extend by a coset LDE of the two planes -- the same values, felt for felt.
static void pcs_deep_assemble(mh_ctx* c, const std::vector<const LdeMatrix*>& mats, const std::vector<u32>& coef_off, int log_n,
                              int log_blowup, const std::vector<e2>& negc, int np, const e2* z, const e2* fred, e2 beta, u64* out,
                              bool one_coset) {
  MH_REQUIRE(mats.size() <= (size_t)PCS_MAX_MATS, "too many committed matrices for one DEEP pass");
  const int lbl = mats[0]->log_cosets;
  const size_t coset0 = mats[0]->coset0;
  for (auto* m : mats) MH_REQUIRE(m->log_cosets == lbl && m->coset0 == coset0, "internal: matrices cover different cosets");
  const size_t N = (size_t)1 << log_n, B = (size_t)1 << lbl;
  const int L = log_n + log_blowup;
  std::vector<u64> blob;
  for (e2 v : negc) { blob.push_back(v.c0); blob.push_back(v.c1); }
  const size_t o_cx = blob.size();
  const u64 g = gl_lde_shift(L), wK = gl_two_adic_generator(L);
  u64 x = gl_mul(g, gl_pow(wK, coset0));
  for (size_t j = 0; j < B; j++) {
    blob.push_back(x);
    x = gl_mul(x, wK);
  }
  DevBuf dblob(blob.size() * 8), one;
  c->h2d(dblob.p, blob.data(), blob.size() * 8);
  const u64* tw = log_n ? c->twiddles(log_n, false) : nullptr;
  if (!tw) {
    one.alloc(8);
    u64 v = 1;
    c->h2d(one.p, &v, 8);
    tw = one.u();
  }
  MH_REQUIRE(!one_coset || (lbl >= 1 && log_n >= DEEP_ONE_COSET_MIN_LOG_N), "internal: one-coset DEEP assemble needs two cosets to extend to");
  const size_t Ba = one_coset ? 1 : B;  // cosets the assemble kernel runs on
  PcsDeepArgs a{};
  double bytes = 16.0 * N * Ba;
  for (size_t i = 0; i < mats.size(); i++) {
    a.m[i] = PcsDeepMat{mats[i]->lde.u(), (u32)mats[i]->width, coef_off[i], mats[i]->log_n};
    bytes += 8.0 * (double)mats[i]->width * (double)(((size_t)1 << mats[i]->log_n) * Ba);
  }
  a.n_mats = (int)mats.size();
  a.log_n = log_n; a.log_blowup = lbl;
  a.negc = dblob.u(); a.tw = tw; a.coset_x = dblob.u() + o_cx;
  e2 bp = e2_make(1);
  for (int k = 0; k < NPMAX; k++) {
    a.z.v[k] = k < np ? z[k] : e2_make(0);
    a.fred.v[k] = k < np ? fred[k] : e2_make(0);
    a.bpow.v[k] = bp;
    bp = e2_mul(bp, beta);
  }
  const dim3 grid((unsigned)((N + 255) / 256), (unsigned)Ba);
  DevBuf planes, scratch, ext;
  if (one_coset) {
    planes.alloc(2 * N * 8); scratch.alloc(2 * N * 8); ext.alloc(2 * B * N * 8);
    a.out = planes.u();
  } else {
    a.out = out;
  }
  {
    ProfScope ps(c, "pcs_deep_assemble", bytes);
    switch (np) {
      case 1: launch_deep<1>(c, grid, a, one_coset); break;
      case 2: launch_deep<2>(c, grid, a, one_coset); break;
      case 3: launch_deep<3>(c, grid, a, one_coset); break;
      default: launch_deep<4>(c, grid, a, one_coset); break;
    }
  }
  if (one_coset) {
    // Q on x_0 * H -> Q on x_j * H for every stored coset, in their stored order (coset 0 comes out again: the same values)
    ProfScope ps(c, "pcs_deep_extend", 16.0 * N + 3.0 * 16.0 * N * B);
    const std::vector<u64> shifts(blob.begin() + o_cx, blob.begin() + o_cx + B);
    lde_columns(c, planes.u(), 2, log_n, shifts[0], shifts, ext.u(), scratch.u());
    MH_LAUNCH(k_pcs_interleave, dim3((unsigned)((B * N + 255) / 256)), dim3(256), 0, c->stream, ext.u(), B * N, out);
  }
  HIP_CHECK(hipStreamSynchronize(c->stream));
}

// -------------------------------------------------------------------------------------------------
// domain.rs:539-553 for a caller-chosen point: nonzero, outside H (of the tallest matrix) and outside gK
static bool point_ok(int log_N, int lb, e2 z) {
  if (e2_is_zero(z)) return false;
  if (e2_eq(e2_exp_pow2(z, log_N), e2_make(1))) return false;
  const u64 g_inv = gl_inv(gl_lde_shift(log_N + lb));
  return !e2_eq(e2_exp_pow2(e2_mulf(z, g_inv), log_N + lb), e2_make(1));
}

// One opening in flight: the stages of open_with_channel as methods, like mh_session.
struct mh_pcs {
  mh_ctx* c = nullptr;
  mh_pcs_params pp{};
  int np = 0, lb = 0, log_N = 0, L = 0;
  size_t N = 0, W = 0;
  e2 z[NPMAX];
  std::vector<const mh_tree*> trees;     // borrowed
  std::vector<const LdeMatrix*> mats;    // every matrix of every tree, in order
  std::vector<u32> coef_off;
  std::vector<e2> ev[NPMAX];             // aligned evaluations per point
  int lmcs0 = 0, salt0 = 0;
  int stage = 0;  // 1 begun, 2 evaluated, 3 DEEP layer built (FRI rounds), 4 final polynomial sent, 5 opened
  PcsStage fs;

  size_t alignment() const { return c->lmcs == MH_LMCS_BLAKE3 ? 1 : (c->lmcs == MH_LMCS_KECCAK ? 17 : 8); }
  size_t al(size_t w) const {
    const size_t a = alignment();
    return (w + a - 1) / a * a;
  }
  void expect(int s, const char* what) {
    MH_REQUIRE(stage == s, std::string("pcs call out of protocol order: ") + what);
    MH_REQUIRE(c->lmcs == lmcs0, "the context's LMCS hasher changed during the opening");
    MH_REQUIRE(c->salt.n == salt0, "the context's salt width changed during the opening");
  }
  // every precondition is checked here, on the host, before anything is launched (pcs/deep/prover.rs:68-79, :133-138)
  void begin(mh_ctx* ctx, const mh_pcs_params& params, int n_trees, const mh_tree* const* trees_in, int n_points, const u64* points) {
    c = ctx; pp = params;
    lmcs0 = c->lmcs; salt0 = c->salt.n;
    pcs_params_require(pp);
    lb = pp.log_blowup;
    MH_REQUIRE(n_trees >= 1 && n_trees <= 256, "need between 1 and 256 committed trees");
    MH_REQUIRE(n_points >= 1 && n_points <= MH_PCS_MAX_POINTS, "n_points must be in 1..MH_PCS_MAX_POINTS");
    np = n_points;
    log_N = -1;
    for (int t = 0; t < n_trees; t++) {
      const mh_tree* tr = trees_in[t];
      MH_REQUIRE(tr, "null tree");
      MH_REQUIRE(tr->ctx == c, "a tree was committed on another context");
      MH_REQUIRE(tr->fri_log_rows < 0 && !tr->mats.empty(), "a FRI round tree cannot be opened: it commits a layer, not matrices");
      MH_REQUIRE(tr->shard_logG == 0, "standalone openings run on a single GPU: a tree of mh_commit_traces_sharded (world > 1) is refused");
      MH_REQUIRE(tr->lmcs == c->lmcs, "a tree was committed with another LMCS hasher than this context's");
      MH_REQUIRE(tr->salt.n == c->salt.n, "a tree was committed with another salt width than this context's (mh_ctx_set_salt)");
      MH_REQUIRE(tr->log_blowup == lb, "a tree was committed under a different log_blowup than params->log_blowup");
      for (const LdeMatrix& m : tr->mats) {
        MH_REQUIRE(m.log_cosets == lb && m.coset0 == 0, "a tree does not store every coset of its matrices");
        log_N = std::max(log_N, m.log_n);
        mats.push_back(&m);
      }
      MH_REQUIRE(tr->log_height == tr->mats.back().log_n + lb, "internal: tree depth differs from its tallest matrix");
      trees.push_back(tr);
    }
    MH_REQUIRE(mats.size() <= (size_t)PCS_MAX_MATS, "too many committed matrices for one opening (128 at most)");
    MH_REQUIRE(log_N >= 1, "the tallest matrix needs at least 2 rows");
    L = log_N + lb;
    MH_REQUIRE(L <= 32, "LDE order exceeds the field's two-adicity");
    N = (size_t)1 << log_N;
    // max over the trees IS a tree's height, so "at least one tree at the maximum" holds by construction; what can fail is a caller's
    // idea of the maximum -- the points are checked against the domain these trees define
    for (int k = 0; k < np; k++) {
      z[k] = e2{gl_canon(points[2 * k]), gl_canon(points[2 * k + 1])};
      MH_REQUIRE(point_ok(log_N, lb, z[k]), "evaluation point " + std::to_string(k) + " is zero, on the trace domain H or on the LDE coset gK");
    }
    W = 0;
    for (auto* m : mats) {
      coef_off.push_back((u32)W);
      W += al(m->width);
    }
    fs.c = c; fs.pp = pp; fs.lb = lb; fs.L = L; fs.rounds = fri_num_rounds(pp, L);
    fs.trees = trees; fs.alignment = alignment();
    stage = 1;
  }
  // ---- evaluations at every point: all trees, all matrices, aligned ----
  void evals() {
    expect(1, "evals");
    ProfScope span(c, "span:pcs evaluate at the points");  // pcs/deep/prover.rs:88
    std::vector<OodJobN> jobs(mats.size());
    for (size_t i = 0; i < mats.size(); i++) {
      jobs[i].m = mats[i];
      for (int k = 0; k < np; k++) jobs[i].y[k] = e2_exp_pow2(z[k], log_N - mats[i]->log_n);  // f(X^L) at z = f at z^L
    }
    pcs_ood_eval_batch(c, jobs, np, lb);
    for (int k = 0; k < np; k++) {
      ev[k].assign(W, e2_make(0));
      for (size_t i = 0; i < mats.size(); i++)
        for (size_t col = 0; col < jobs[i].out[k].size(); col++) ev[k][coef_off[i] + col] = jobs[i].out[k][col];
    }
    stage = 2;
  }
  // ---- DEEP quotient ----
  void deep(e2 alpha_d, e2 beta_d) {
    expect(2, "deep");
    ProfScope span(c, "span:pcs DEEP quotient");  // pcs/prover.rs:57
    e2 fred[NPMAX];
    for (int k = 0; k < np; k++) {
      e2 a = e2_make(0);
      for (size_t i = 0; i < W; i++) a = e2_add(e2_mul(a, alpha_d), ev[k][i]);
      fred[k] = a;
    }
    std::vector<e2> negc(W);
    e2 pw = e2_make(GL_P - 1);
    for (size_t i = W; i-- > 0;) {
      negc[i] = pw;
      pw = e2_mul(pw, alpha_d);
    }
    fs.layer.alloc((N << lb) * 16);
    const char* all_env = getenv("MH_DEEP_ALL_COSETS");  // read per call, as the session does
    const bool one_coset = !(all_env && atoi(all_env)) && lb >= 1 && log_N >= DEEP_ONE_COSET_MIN_LOG_N;
    pcs_deep_assemble(c, mats, coef_off, log_N, lb, negc, np, z, fred, beta_d, fs.layer.u(), one_coset);
    fs.start(log_N, lb, 0);
    stage = 3;
  }
  // the DEEP layer in domain order; the layer is coset-major until a tiny one has been rearranged for its first commitment
  void download_deep(u64* out) {
    expect(3, "download_deep");
    MH_REQUIRE(fs.fri_trees.empty() || (fs.fri_trees.size() == 1 && fs.round_committed), "the DEEP layer has been folded away");
    const size_t n = (size_t)1 << L;
    std::vector<u64> host(2 * n);
    HIP_CHECK(hipMemcpyAsync(host.data(), fs.layer.p, n * 16, hipMemcpyDeviceToHost, c->stream));
    c->sync();
    if (fs.cbits == 0) {
      memcpy(out, host.data(), n * 16);
      return;
    }
    const size_t B = (size_t)1 << lb;
    for (size_t i = 0; i < n; i++) {
      const size_t slot = ((i & (B - 1)) << log_N) + (i >> lb);
      out[2 * i] = host[2 * slot];
      out[2 * i + 1] = host[2 * slot + 1];
    }
  }
  void fri_commit(u64 root[4]) {
    expect(3, "fri_commit");
    fs.fri_commit(root);
  }
  void fri_fold_round(e2 fb) {
    expect(3, "fri_fold");
    fs.fri_fold_round(fb);
  }
  void fri_final(std::vector<e2>& desc) {
    expect(3, "fri_final");
    fs.fri_final(desc);
    stage = 4;
  }
  void query(const std::vector<size_t>& idx, std::vector<u64>& fields, std::vector<u64>& commitments) {
    expect(4, "query");
    fs.open(idx, fields, commitments);
    stage = 5;
  }
};

// open_with_channel with the library's transcript (pcs/prover.rs:34-101)
static void pcs_open_impl(mh_ctx* c, const mh_pcs_params& pp, int n_trees, const mh_tree* const* trees, int n_points, const u64* points,
                          const u64 init_state[12], const u64* pre_observe, size_t n_pre, mh_proof& proof) {
  mh_pcs s;
  s.begin(c, pp, n_trees, trees, n_points, points);
  HostTranscript tr;
  tr.ch.hash = c->lmcs;
  tr.ch.init_from_state(init_state);
  for (size_t i = 0; i < n_pre; i++) tr.ch.observe_framing(pre_observe[i]);
  s.evals();
  for (int k = 0; k < s.np; k++)
    for (e2 v : s.ev[k]) tr.send_ef(v);
  do_grind(c, tr, pp.deep_pow_bits);
  const e2 alpha_d = tr.ch.sample_ef();
  const e2 beta_d = tr.ch.sample_ef();
  s.deep(alpha_d, beta_d);
  u64 root[4];
  for (int r = 0; r < s.fs.rounds; r++) {
    s.fri_commit(root);
    tr.send_commitment(root);
    do_grind(c, tr, pp.folding_pow_bits);
    s.fri_fold_round(tr.ch.sample_ef());
  }
  std::vector<e2> final_poly;
  s.fri_final(final_poly);
  for (e2 v : final_poly) tr.send_ef(v);
  do_grind(c, tr, pp.query_pow_bits);
  std::vector<size_t> idx;
  for (int i = 0; i < pp.num_queries; i++) idx.push_back(tr.ch.sample_bits(s.L));
  std::vector<u64> f, cm;
  s.query(idx, f, cm);
  tr.hint_fields(f);
  tr.hint_commitments(cm);
  tr.ch.finalize(proof.digest);
  for (const mh_tree* t : s.trees) proof.log_trace_heights.push_back((uint8_t)t->mats.back().log_n);
  proof.fields = std::move(tr.fields);
  for (auto& d : tr.commitments) proof.commitments.insert(proof.commitments.end(), d.begin(), d.end());
}

// -------------------------------------------------------------------------------------------------
#define MH_TRY(ctx_expr) mh_ctx* _c = (ctx_expr); PoolScope _ps(_c); try {
#define MH_CATCH                                                   \
  }                                                                \
  catch (const MhError& e) {                                       \
    if (_c) _c->err = e.what();                                    \
    return e.code;                                                 \
  }                                                                \
  catch (const std::exception& e) {                                \
    if (_c) _c->err = e.what();                                    \
    return MH_ERR_INTERNAL;                                        \
  }                                                                \
  return MH_OK;
#define MH_PTRY MH_TRY(p ? p->c : nullptr) MH_REQUIRE(p, "null pcs handle"); HIP_CHECK(hipSetDevice(p->c->device));
static e2 e2_in(const uint64_t v[2]) { return e2{gl_canon(v[0]), gl_canon(v[1])}; }
static void e2_out(const std::vector<e2>& v, uint64_t* out) {
  for (size_t i = 0; i < v.size(); i++) { out[2 * i] = v[i].c0; out[2 * i + 1] = v[i].c1; }
}

extern "C" {

int mh_pcs_begin(mh_ctx* c, const mh_pcs_params* params, int n_trees, const mh_tree* const* trees, int n_points, const uint64_t* points,
                 mh_pcs** out) {
  MH_TRY(c)
  MH_REQUIRE(c && params && trees && points && out, "null argument");
  HIP_CHECK(hipSetDevice(c->device));
  std::unique_ptr<mh_pcs> p(new mh_pcs());
  p->begin(c, *params, n_trees, trees, n_points, points);
  *out = p.release();
  MH_CATCH
}
void mh_pcs_free(mh_pcs* p) {
  if (!p) return;
  (void)hipSetDevice(p->c->device);
  PoolScope ps(p->c);
  delete p;
}
int mh_pcs_shape(const mh_pcs* p, mh_pcs_shape_t* out) {
  if (!p || !out) return MH_ERR_INVALID;
  out->log_lde_height = p->L;
  out->n_points = p->np;
  out->ood_width = p->W;
  out->num_fri_rounds = p->fs.rounds;
  out->final_poly_len = p->fs.final_poly_len();
  return MH_OK;
}
int mh_pcs_evals(mh_pcs* p, uint64_t* evals_out) {
  MH_PTRY
  MH_REQUIRE(evals_out, "null argument");
  p->evals();
  for (int k = 0; k < p->np; k++) e2_out(p->ev[k], evals_out + 2 * p->W * (size_t)k);
  MH_CATCH
}
int mh_pcs_deep(mh_pcs* p, const uint64_t alpha[2], const uint64_t beta[2]) {
  MH_PTRY
  MH_REQUIRE(alpha && beta, "null argument");
  p->deep(e2_in(alpha), e2_in(beta));
  MH_CATCH
}
int mh_pcs_download_deep(mh_pcs* p, uint64_t* out) {
  MH_PTRY
  MH_REQUIRE(out, "null argument");
  p->download_deep(out);
  MH_CATCH
}
int mh_pcs_fri_commit(mh_pcs* p, uint64_t root[4]) {
  MH_PTRY
  MH_REQUIRE(root, "null argument");
  p->fri_commit(root);
  MH_CATCH
}
int mh_pcs_fri_fold(mh_pcs* p, const uint64_t beta[2]) {
  MH_PTRY
  MH_REQUIRE(beta, "null argument");
  p->fri_fold_round(e2_in(beta));
  MH_CATCH
}
int mh_pcs_fri_final(mh_pcs* p, uint64_t* coeffs_out) {
  MH_PTRY
  MH_REQUIRE(coeffs_out, "null argument");
  std::vector<e2> desc;
  p->fri_final(desc);
  e2_out(desc, coeffs_out);
  MH_CATCH
}
int mh_pcs_query(mh_pcs* p, const uint64_t* indices, size_t n_indices, mh_proof** out) {
  MH_PTRY
  MH_REQUIRE(indices && n_indices && out, "null/empty argument");
  std::unique_ptr<mh_proof> pr(new mh_proof());
  memset(pr->digest, 0, sizeof pr->digest);
  std::vector<size_t> idx(indices, indices + n_indices);
  p->query(idx, pr->fields, pr->commitments);
  for (const mh_tree* t : p->trees) pr->log_trace_heights.push_back((uint8_t)t->mats.back().log_n);
  *out = pr.release();
  MH_CATCH
}
int mh_pcs_open(mh_ctx* c, const mh_pcs_params* params, int n_trees, const mh_tree* const* trees, int n_points, const uint64_t* points,
                const uint64_t challenger_state[12], const uint64_t* pre_observe, size_t n_pre_observe, mh_proof** out) {
  MH_TRY(c)
  MH_REQUIRE(c && params && trees && points && challenger_state && out, "null argument");
  MH_REQUIRE(pre_observe || !n_pre_observe, "null pre_observe");
  HIP_CHECK(hipSetDevice(c->device));
  std::unique_ptr<mh_proof> p(new mh_proof());
  pcs_open_impl(c, *params, n_trees, trees, n_points, points, challenger_state, pre_observe, n_pre_observe, *p);
  *out = p.release();
  MH_CATCH
}

}  // extern "C"
