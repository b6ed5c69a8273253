// Landmark (keypoint) registration error of a displacement field, forward and backward, 2-D and 3-D.  Build-defined
// (include/dfmir_hip.h and losses.Landmark_Loss state the definition):
//
//   flow u [B][ND][(D)][H][W] fp32, channel a displaces axis a in voxels, order (z,) y, x, as the warp kernels read a flow:
//   warped(x) = moving(x + u(x)), so a point q of the FIXED image corresponds to q + u(q) in the MOVING image.
//   fixed_pts q, moving_pts p [B][K][ND] voxel coordinates in the same axis order, weight w [B][K] (NULL = 1), spacing h.
//   m_bk = q + u_b(q)        u_b sampled (bi/tri)linearly in the cell i0_a = min(floor(q_a), S_a - 2)
//   r_bk = h (.) (m_bk - p),   d_bk = |r_bk|_2
//   valid: w > 0, every coordinate of q and p finite, 0 <= q_a <= S_a - 1.  An invalid landmark has d = NaN (and a NaN row in
//   the mapped positions), adds to no sum and gets no gradient.
//   loss = sum w d^2 / Wsum ('l2') or sum w d / Wsum ('tre', derivative 0 at d = 0), Wsum = sum of w over the valid landmarks
//   of the call; Wsum = 0 gives loss 0 and an all-zero gradient.
//   dflow[b, a, corner] += gout (w / Wsum) dl/dr_a h_a cornerweight; dflow is written entirely.
//
// K <= 4096 landmarks against a volume of millions of voxels: everything here is latency, not bandwidth, except the zero
// fill of dflow.  A workgroup owns LM_T = 256 consecutive landmarks of ONE sample; lm_point is the ONE place a landmark's
// validity, cell, corner weights, mapped position and residual are formed, for both directions.
//   lm_fwd_k   per landmark m and d; per workgroup three double slots (sum w pen, sum w d, sum w over its valid landmarks).
//   lm_fin_k   (one workgroup) adds the slots of each sample in index order: the per-sample weighted mean of d, then the
//              samples in a fixed order: the loss and Wsum (which the backward reads).
//   lm_zero_k  dflow = 0 (16-byte stores where dflow is 16-byte aligned).
//   lm_prep_k / lm_bwd_k   the scheme built is the OWNER-GATHER over landmark pairs: no floating-point atomics, no integer atomics, no
//              volume-sized accumulator.  lm_prep_k forms every landmark's record once (cell, upper-corner weights, the ND
//              gradient coefficients gout (w / Wsum) dl/dr_a h_a; r is recomputed, gout and Wsum are read on the device) in
//              ws: 1 + 3 ND words per landmark.  In lm_bwd_k the sample's records pass through LDS in tiles of LM_T.  A
//              thread owns one landmark i and walks ALL landmarks j of its sample in index order; two cells
//              share voxels only when they differ by at most 1 on every axis (a compare on the flat cell index and one on
//              the x cell, four landmarks per 16-byte LDS read, reject nearly every pair; the per-axis test then decides),
//              and then corner c of i is corner c + (i0_i - i0_j) of j.  Each of the thread's 2^ND corner voxels sums
//              the contributions of every landmark that touches it, j ascending (i itself in its place), and the thread
//              stores the sum only if no j < i touches that voxel: every touched voxel is written exactly once, by its
//              lowest-index toucher, with a sum whose order is fixed -- bit-identical from run to run whatever the
//              collisions.  O(K^2) compares per sample: 16.8 M at K = 4096, spread over K threads.
//              Chosen over a sort by cell (more launches and scratch for nothing at K <= 4096) and over 64-bit fixed-point
//              atomics on dflow (would need a volume-sized integer accumulator).
// Nothing syncs with the host, allocates or keeps state.
#include "lin_cell.h"

namespace {

constexpr int LM_T = 256;                    // threads per workgroup = landmarks per workgroup and per LDS tile
constexpr int LM_KMAX = 4096;
constexpr int LM_FAR = -(1 << 30);           // cell coordinate of an invalid landmark in LDS: near no cell (extents < 2^30)

struct LmGeom {
  int n[3];                                  // extents in the axis order (z,) y, x: ND entries are used
  int st[3];                                 // their strides in a channel
  float h[3];                                // spacing, same order
  int S;                                     // voxels per sample
  int K;
  int nblk;                                  // workgroups (= tiles) per sample
};

__device__ __forceinline__ float lm_nan() { return __uint_as_float(0x7fc00000u); }

// sums over the workgroup, valid in thread 0; the same order every run
template <int N>
__device__ __forceinline__ void lm_block_sum(double (&s)[N], double* sm /* N * LM_T / 64 */) {
#pragma unroll
  for (int i = 0; i < N; ++i) s[i] = wave_sum(s[i]);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) sm[i * (LM_T / 64) + (threadIdx.x >> 6)] = s[i];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      s[i] = 0.0;
      for (int w = 0; w < LM_T / 64; ++w) s[i] += sm[i * (LM_T / 64) + w];
    }
  }
}

template <int ND>
struct LmPoint {
  bool valid;
  int i0[ND];                                // the cell (lower corner); LM_FAR when invalid
  float w1[ND];                              // weight of the upper corner along each axis
  float m[ND];                               // mapped position q + u(q)
  float r[ND];                               // h (m - p)
  float d;                                   // |r|
};

// One landmark.  q, p: its ND coordinates (p == nullptr: map only, validity is that of q and the weight alone).  No float
// that failed the range test is converted to int; every corner read lies inside the channel: 0 <= i0_a <= n_a - 2.
template <int ND>
__device__ __forceinline__ void lm_point(const float* __restrict__ fb, const float* __restrict__ q,
                                         const float* __restrict__ p, float wt, const LmGeom& g, LmPoint<ND>& o) {
  constexpr int NC = 1 << ND;
  float qa[ND], pa[ND];
  bool ok = wt > 0.f;                                           // false for a NaN weight
#pragma unroll
  for (int a = 0; a < ND; ++a) {
    qa[a] = q[a];
    pa[a] = p ? p[a] : 0.f;
    ok = ok && qa[a] >= 0.f && qa[a] <= (float)(g.n[a] - 1) && fabsf(pa[a]) <= 3.4028234e38f;   // false for NaN
  }
  o.valid = ok;
  if (!ok) {
#pragma unroll
    for (int a = 0; a < ND; ++a) { o.i0[a] = LM_FAR; o.w1[a] = 0.f; o.m[a] = lm_nan(); o.r[a] = 0.f; }
    o.d = lm_nan();
    return;
  }
  int base = 0;
#pragma unroll
  for (int a = 0; a < ND; ++a) {
    int i = (int)floorf(qa[a]);
    i = i > g.n[a] - 2 ? g.n[a] - 2 : i;
    i = i < 0 ? 0 : i;                                          // (q_a >= 0 already; keeps the read inside whatever happens)
    o.i0[a] = i;
    o.w1[a] = qa[a] - (float)i;
    base += i * g.st[a];
  }
  float u[ND];
#pragma unroll
  for (int c = 0; c < ND; ++c) u[c] = 0.f;
#pragma unroll
  for (int cn = 0; cn < NC; ++cn) {
    int off = base;
#pragma unroll
    for (int a = 0; a < ND; ++a) off += ((cn >> (ND - 1 - a)) & 1) * g.st[a];
    const float cw = lin_cw<ND>(o.w1, cn);
#pragma unroll
    for (int c = 0; c < ND; ++c) u[c] += cw * fb[(long long)c * g.S + off];
  }
  float d2 = 0.f;
#pragma unroll
  for (int a = 0; a < ND; ++a) {
    o.m[a] = qa[a] + u[a];
    o.r[a] = p ? g.h[a] * (o.m[a] - pa[a]) : 0.f;
    d2 += o.r[a] * o.r[a];
  }
  o.d = sqrtf(d2);
}

// ------------------------------------------------------------------------------------------------ forward
template <int ND>
__global__ __launch_bounds__(LM_T) void lm_fwd_k(const float* __restrict__ flow, const float* __restrict__ fpts,
                                                 const float* __restrict__ mpts, const float* __restrict__ wgt, LmGeom g,
                                                 int penalty, float* __restrict__ mapped, float* __restrict__ dtab,
                                                 double* __restrict__ slots) {
  __shared__ double sm[3 * (LM_T / 64)];
  const int b = (int)(blockIdx.x / (unsigned)g.nblk);
  const int blk = (int)(blockIdx.x - (unsigned)b * (unsigned)g.nblk);
  const int k = blk * LM_T + (int)threadIdx.x;
  double s[3] = {0.0, 0.0, 0.0};                                // sum w pen, sum w d, sum w
  if (k < g.K) {
    const long long idx = (long long)b * g.K + k;
    const float wt = wgt ? wgt[idx] : 1.f;
    LmPoint<ND> pt;
    lm_point<ND>(flow + (long long)b * ND * g.S, fpts + idx * ND, mpts ? mpts + idx * ND : nullptr, wt, g, pt);
    if (mapped) {
#pragma unroll
      for (int a = 0; a < ND; ++a) mapped[idx * ND + a] = pt.m[a];
    }
    if (mpts) {
      dtab[idx] = pt.d;
      if (pt.valid) {
        const double wd = (double)wt * (double)pt.d;
        s[0] = penalty ? wd : wd * (double)pt.d;
        s[1] = wd;
        s[2] = (double)wt;
      }
    }
  }
  if (!mpts) return;                                            // (uniform over the launch)
  lm_block_sum<3>(s, sm);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < 3; ++i) slots[3LL * blockIdx.x + i] = s[i];
  }
}

// per[b] = sum w d / sum w over the slots of sample b in index order (NaN without a valid landmark); loss = sum w pen / Wsum
// over the samples in a fixed order (0 when Wsum == 0); wsum[0] = Wsum
__global__ __launch_bounds__(LM_T) void lm_fin_k(const double* __restrict__ slots, int B, int nblk, float* __restrict__ per,
                                                 float* __restrict__ loss, float* __restrict__ wsum) {
  __shared__ double sm[2 * (LM_T / 64)];
  double t[2] = {0.0, 0.0};
  for (int b = threadIdx.x; b < B; b += LM_T) {
    double sp = 0.0, sd = 0.0, sw = 0.0;
    for (int i = 0; i < nblk; ++i) {
      const double* s = slots + 3LL * ((long long)b * nblk + i);
      sp += s[0]; sd += s[1]; sw += s[2];
    }
    per[b] = sw > 0.0 ? (float)(sd / sw) : lm_nan();
    t[0] += sp;
    t[1] += sw;
  }
  lm_block_sum<2>(t, sm);
  if (threadIdx.x == 0) {
    loss[0] = t[1] > 0.0 ? (float)(t[0] / t[1]) : 0.f;
    wsum[0] = (float)t[1];
  }
}

// ------------------------------------------------------------------------------------------------ backward
template <bool VEC>
__global__ __launch_bounds__(LM_T) void lm_zero_k(float* __restrict__ p, long long n) {
  const long long stride = (long long)gridDim.x * LM_T;
  const long long i0 = (long long)blockIdx.x * LM_T + threadIdx.x;
  if (VEC) {
    const long long n4 = n >> 2;
    float4* p4 = reinterpret_cast<float4*>(p);
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    for (long long i = i0; i < n4; i += stride) p4[i] = z;
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) p[(n4 << 2) + threadIdx.x] = 0.f;
  } else {
    for (long long i = i0; i < n; i += stride) p[i] = 0.f;
  }
}


// The backward's per-landmark record, formed ONCE per landmark (the flow gather is a chain of cold misses; every workgroup
// of a sample needs every landmark of it): ws holds 1 + 3 ND arrays of N = B * nblk * LM_T words, each sample padded to
// whole tiles -- the flat index of the cell (LM_FAR when invalid or beyond K), the cell per axis, the upper-corner weights,
// and the ND gradient coefficients gout (w / Wsum) dl/dr_a h_a.
template <int ND>
struct LmRec {
  int* base;
  int* i0[ND];
  float* w1[ND];
  float* g[ND];
  __host__ __device__ LmRec(float* ws, long long N) {
    base = reinterpret_cast<int*>(ws);
    for (int a = 0; a < ND; ++a) {
      i0[a] = reinterpret_cast<int*>(ws) + (1 + a) * N;
      w1[a] = ws + (1 + ND + a) * N;
      g[a] = ws + (1 + 2 * ND + a) * N;
    }
  }
};

template <int ND>
__global__ __launch_bounds__(LM_T) void lm_prep_k(const float* __restrict__ flow, const float* __restrict__ fpts,
                                                  const float* __restrict__ mpts, const float* __restrict__ wgt,
                                                  const float* __restrict__ gout, const float* __restrict__ wsum, LmGeom g,
                                                  int penalty, float* __restrict__ ws, long long N) {
  const int b = (int)(blockIdx.x / (unsigned)g.nblk);
  const int blk = (int)(blockIdx.x - (unsigned)b * (unsigned)g.nblk);
  const int k = blk * LM_T + (int)threadIdx.x;
  const long long slot = (long long)blockIdx.x * LM_T + threadIdx.x;
  const float W = wsum[0];
  const float scale = W > 0.f ? gout[0] / W : 0.f;
  LmPoint<ND> pt;
  pt.valid = false;
  float wt = 0.f;
  if (k < g.K) {
    const long long idx = (long long)b * g.K + k;
    wt = wgt ? wgt[idx] : 1.f;
    lm_point<ND>(flow + (long long)b * ND * g.S, fpts + idx * ND, mpts + idx * ND, wt, g, pt);
  }
  const LmRec<ND> rec(ws, N);
  int jb = 0;
#pragma unroll
  for (int a = 0; a < ND; ++a) {
    float dl = 0.f;                                             // dl/dr_a: 2 r_a ('l2'), r_a / d ('tre', 0 at d = 0)
    if (pt.valid) dl = penalty ? (pt.d > 0.f ? pt.r[a] / pt.d : 0.f) : 2.f * pt.r[a];
    rec.i0[a][slot] = pt.valid ? pt.i0[a] : LM_FAR;
    rec.w1[a][slot] = pt.valid ? pt.w1[a] : 0.f;
    rec.g[a][slot] = pt.valid ? scale * wt * dl * g.h[a] : 0.f;
    jb += pt.valid ? pt.i0[a] * g.st[a] : 0;
  }
  rec.base[slot] = pt.valid ? jb : LM_FAR;
}

template <int ND>
__global__ __launch_bounds__(LM_T) void lm_bwd_k(const float* __restrict__ ws, long long N, LmGeom g,
                                                 float* __restrict__ dflow) {
  constexpr int NC = 1 << ND;
  __shared__ __attribute__((aligned(16))) int s_base[LM_T];
  __shared__ __attribute__((aligned(16))) int s_i0[ND][LM_T];
  __shared__ float s_w1[ND][LM_T];
  __shared__ float s_g[ND][LM_T];
  const int b = (int)(blockIdx.x / (unsigned)g.nblk);
  const int blk = (int)(blockIdx.x - (unsigned)b * (unsigned)g.nblk);
  const int tid = (int)threadIdx.x;
  const int k = blk * LM_T + tid;                               // the landmark this thread owns
  const LmRec<ND> rec(const_cast<float*>(ws), N);
  const long long first = (long long)b * g.nblk * LM_T;         // the sample's records

  const int own_base = rec.base[first + k];
  const bool own_valid = own_base != LM_FAR;                    // false when it is invalid or beyond K
  int own[ND];
#pragma unroll
  for (int a = 0; a < ND; ++a) own[a] = rec.i0[a][first + k];
  // Cells that share a voxel differ by at most 1 on every axis, so their flat indices differ by at most reach and their x
  // cells by at most 1: two compares on two LDS words reject nearly every pair (the flat index alone lets through every pair
  // on neighbouring planes, ~2 % of them at 160 planes -- enough that almost every wave took the slow path for almost every
  // j); the per-axis test below decides.  Flat indices lie in [0, 2^30) and LM_FAR = -2^30, so own_base - LM_FAR + reach
  // < 2^32 does not wrap and exceeds 2 reach.
  unsigned reach = 0u;
#pragma unroll
  for (int a = 0; a < ND; ++a) reach += (unsigned)g.st[a];
  float acc[NC][ND];
#pragma unroll
  for (int cn = 0; cn < NC; ++cn)
#pragma unroll
    for (int c = 0; c < ND; ++c) acc[cn][c] = 0.f;
  unsigned lower = 0u;                                          // bit cn: a landmark of lower index touches corner cn's voxel

  for (int t = 0; t < g.nblk; ++t) {
    const long long src = first + (long long)t * LM_T + tid;
    if (t > 0) __syncthreads();                                 // the previous tile has been read by every thread
    s_base[tid] = rec.base[src];
#pragma unroll
    for (int a = 0; a < ND; ++a) {
      s_i0[a][tid] = rec.i0[a][src];
      s_w1[a][tid] = rec.w1[a][src];
      s_g[a][tid] = rec.g[a][src];
    }
    __syncthreads();
    if (!own_valid) continue;                                   // owns no voxel: it only stages and keeps the barriers
    for (int j4 = 0; j4 < LM_T; j4 += 4) {                      // four landmarks per 16-byte LDS read (a broadcast)
      const int4 sb = *reinterpret_cast<const int4*>(&s_base[j4]);
      const int4 sx = *reinterpret_cast<const int4*>(&s_i0[ND - 1][j4]);
      const int sbe[4] = {sb.x, sb.y, sb.z, sb.w}, sxe[4] = {sx.x, sx.y, sx.z, sx.w};
      unsigned cand = 0u;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        cand |= ((unsigned)(own_base - sbe[e]) + reach <= 2u * reach &&
                 (unsigned)own[ND - 1] - (unsigned)sxe[e] + 1u <= 2u ? 1u : 0u) << e;
      if (!cand) continue;
#pragma unroll 1
      for (int e = 0; e < 4; ++e) {                             // index order
        if (!((cand >> e) & 1u)) continue;
        const int jj = j4 + e;
        int da[ND];
        bool near = true;
#pragma unroll
        for (int a = 0; a < ND; ++a) {
          da[a] = own[a] - s_i0[a][jj];
          near = near && (unsigned)(da[a] + 1) <= 2u;
        }
        if (!near) continue;
        float w1[ND], gj[ND];
#pragma unroll
        for (int a = 0; a < ND; ++a) { w1[a] = s_w1[a][jj]; gj[a] = s_g[a][jj]; }
        const bool below = t * LM_T + jj < k;
#pragma unroll
        for (int cn = 0; cn < NC; ++cn) {
          int cj = 0;                                           // the corner of j that is corner cn of this thread's cell
          bool hit = true;
#pragma unroll
          for (int a = 0; a < ND; ++a) {
            const int bp = ((cn >> (ND - 1 - a)) & 1) + da[a];
            hit = hit && (unsigned)bp <= 1u;
            cj |= (bp & 1) << (ND - 1 - a);
          }
          if (hit) {
            const float cw = lin_cw<ND>(w1, cj);
#pragma unroll
            for (int c = 0; c < ND; ++c) acc[cn][c] += gj[c] * cw;
            if (below) lower |= 1u << cn;
          }
        }
      }
    }
  }
  if (!own_valid) return;
  float* db = dflow + (long long)b * ND * g.S;
#pragma unroll
  for (int cn = 0; cn < NC; ++cn) {
    if ((lower >> cn) & 1u) continue;                           // a landmark of lower index stores this voxel's sum
    int off = own_base;
#pragma unroll
    for (int a = 0; a < ND; ++a) off += ((cn >> (ND - 1 - a)) & 1) * g.st[a];
#pragma unroll
    for (int c = 0; c < ND; ++c) db[(long long)c * g.S + off] = acc[cn][c];
  }
}

// ------------------------------------------------------------------------------------------------ host side
// false for arguments the entry points refuse: nd outside {2, 3}, B < 1, K outside [1, 4096], an extent < 2 (D is not read
// when nd == 2), 2^31 and more flow elements (or workgroups), a spacing that is not positive and finite
bool lm_geom(int nd, int B, int K, int D, int H, int W, float hz, float hy, float hx, LmGeom* g) {
  if ((nd != 2 && nd != 3) || B < 1 || K < 1 || K > LM_KMAX || H < 2 || W < 2 || (nd == 3 && D < 2)) return false;
  if (nd == 2) { D = 1; hz = 1.f; }
  const float hs[3] = {hz, hy, hx};
  for (float h : hs)
    if (!(h > 0.f && h <= 3.4028234e38f)) return false;
  const long long S = (long long)D * H * W;
  if (S * nd * B >= (1LL << 31)) return false;
  g->S = (int)S;
  g->K = K;
  g->nblk = (K + LM_T - 1) / LM_T;
  if (nd == 3) {
    g->n[0] = D; g->n[1] = H; g->n[2] = W;
    g->st[0] = H * W; g->st[1] = W; g->st[2] = 1;
    g->h[0] = hz; g->h[1] = hy; g->h[2] = hx;
  } else {
    g->n[0] = H; g->n[1] = W; g->n[2] = 1;
    g->st[0] = W; g->st[1] = 1; g->st[2] = 0;
    g->h[0] = hy; g->h[1] = hx; g->h[2] = 1.f;
  }
  return (long long)B * g->nblk < (1LL << 31);                  // the grid of lm_fwd_k / lm_bwd_k
}

}  // namespace

extern "C" long long dfmir_landmark_ws_floats(int nd, int B, int K, int D, int H, int W) {
  LmGeom g;
  if (!lm_geom(nd, B, K, D, H, W, 1.f, 1.f, 1.f, &g)) return -1;
  // the backward's records, 1 + 3 nd words per landmark of the samples padded to whole tiles (the forward's three doubles
  // per workgroup fit in them)
  return (1LL + 3 * nd) * LM_T * B * g.nblk;
}

extern "C" int dfmir_landmark_fwd(int nd, const float* flow, const float* fixed_pts, const float* moving_pts,
                                  const float* weight, float* ws, float* mapped, float* d, float* per_sample, float* loss,
                                  float* wsum, int B, int K, int D, int H, int W, float hz, float hy, float hx, int penalty,
                                  void* stream) {
  LmGeom g;
  DF_ARG_CHECK(flow && fixed_pts && (penalty == 0 || penalty == 1));
  if (moving_pts) DF_ARG_CHECK(ws && d && per_sample && loss && wsum && (reinterpret_cast<uintptr_t>(ws) & 7) == 0);
  else DF_ARG_CHECK(mapped != nullptr);
  DF_ARG_CHECK(lm_geom(nd, B, K, D, H, W, hz, hy, hx, &g));
  hipStream_t st = (hipStream_t)stream;
  const unsigned nwg = (unsigned)((long long)B * g.nblk);
  double* slots = reinterpret_cast<double*>(ws);
  if (nd == 3) lm_fwd_k<3><<<nwg, LM_T, 0, st>>>(flow, fixed_pts, moving_pts, weight, g, penalty, mapped, d, slots);
  else lm_fwd_k<2><<<nwg, LM_T, 0, st>>>(flow, fixed_pts, moving_pts, weight, g, penalty, mapped, d, slots);
  DF_LAUNCH_CHECK();
  if (moving_pts) {
    lm_fin_k<<<1, LM_T, 0, st>>>(slots, B, g.nblk, per_sample, loss, wsum);
    DF_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int dfmir_landmark_bwd(int nd, const float* flow, const float* fixed_pts, const float* moving_pts,
                                  const float* weight, const float* gout, const float* wsum, float* dflow, float* ws, int B,
                                  int K, int D, int H, int W, float hz, float hy, float hx, int penalty, void* stream) {
  LmGeom g;
  DF_ARG_CHECK(flow && fixed_pts && moving_pts && gout && wsum && dflow && ws && (penalty == 0 || penalty == 1));
  DF_ARG_CHECK(lm_geom(nd, B, K, D, H, W, hz, hy, hx, &g));
  hipStream_t st = (hipStream_t)stream;
  const long long n = (long long)B * nd * g.S;
  if ((reinterpret_cast<uintptr_t>(dflow) & 15) == 0) lm_zero_k<true><<<df_grid((n + 3) / 4, LM_T, 8192), LM_T, 0, st>>>(dflow, n);
  else lm_zero_k<false><<<df_grid(n, LM_T, 8192), LM_T, 0, st>>>(dflow, n);
  DF_LAUNCH_CHECK();
  const unsigned nwg = (unsigned)((long long)B * g.nblk);
  const long long N = (long long)nwg * LM_T;
  if (nd == 3) lm_prep_k<3><<<nwg, LM_T, 0, st>>>(flow, fixed_pts, moving_pts, weight, gout, wsum, g, penalty, ws, N);
  else lm_prep_k<2><<<nwg, LM_T, 0, st>>>(flow, fixed_pts, moving_pts, weight, gout, wsum, g, penalty, ws, N);
  DF_LAUNCH_CHECK();
  if (nd == 3) lm_bwd_k<3><<<nwg, LM_T, 0, st>>>(ws, N, g, dflow);
  else lm_bwd_k<2><<<nwg, LM_T, 0, st>>>(ws, N, g, dflow);
  DF_LAUNCH_CHECK();
  return 0;
}
