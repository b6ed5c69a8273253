// Algebra on displacement fields: composition of two flows, forward and backward, and fixed-point inversion of a flow, 2-D and
// 3-D.  Build-defined (include/dfmir_hip.h, ops.compose_flows and ops.invert_flow state the definitions):
//
//   u, v [B][ND][(D)][H][W] fp32, channel i displaces axis i in voxels, order (z,) y, x, as the warp kernels read a flow.
//   c(x)    = u(x) + v(x + u(x))      v sampled (bi/tri)linearly, corners outside the volume read as 0: warp(src, c) is
//                                     warp(warp(src, v), u) in the continuum, u is the warp applied last
//   du_c(x) = g_c(x) + sum_c' g_c'(x) d_c v_c'(x + u(x))     d_c = the derivative of the interpolant: corner differences,
//             zero-padded corners taking part as zeros
//   dv      = the transpose of the interpolation applied to g (a scatter to the up to 2^ND corners)
//
//   inversion: w_0 = init (or 0),  r_k(x) = w_k(x) + u(x + w_k(x)),  w_{k+1} = w_k - r_k  (= -u(x + w_k) up to rounding); a
//             voxel stops updating once max_c |r_k,c| <= tol (it keeps its w and its r from then on).  Per sample and k:
//             rms_k = sqrt(sum over voxels and channels of r_k^2 / S), max_k = max |r_k,c|.
//
// The sampling is that of the inverse-consistency kernels (flow_sample.h: ic_voxel on lin_cell.h's guarded cell, the 8-byte
// corner-pair loads, IcThread's voxel ownership): a workgroup owns IC_T * VPT consecutive voxels of ONE sample, VPT = 4 with
// 16-byte loads / stores through LDS when W % 4 == 0 and the streamed pointers are 16-byte aligned, else 1.
//   compose_fwd_k   ic_fwd_k's body storing r instead of reducing it.
//   compose_bwd_k   ic_bwd_voxels (the body of ic_bwd_k) with the gradient read from memory instead of formed from r.  dv
//                   takes the two ways of invcons.hip: (a) W % 4 == 0, everything 16-byte aligned: g goes straight to the
//                   owner-gather adjoint of the warp (warp_win.hip), and compose_bwd_k is launched for du alone; (b)
//                   elsewhere the 64-bit fixed-point scatter, its range taken from max |g| (cmp_absmax_k: an integer maximum
//                   of bit patterns, order-independent), cmp_zero_k before and cmp_cvt_k after.  DFMIR_INVCONS_FIXED64
//                   forces (b) here as it does there.
//   invert_k        ONE launch for the whole inversion: iteration k + 1 at x reads w_k(x) and a gather of the constant u
//                   alone, so w stays in registers for all iterations; the eager loop (a warp and a negation per iteration)
//                   writes and re-reads the field twice per iteration.  iters + 1 gathers per voxel, w is written once.
//                   Statistics: |r|^2 in double and the bit pattern of max |r_c| per wave and iteration into LDS slots indexed
//                   by iteration (hence iters <= INV_MAX_ITERS), one slot per workgroup and iteration in memory;
//                   inv_fin_k adds the slots of one (iteration, sample) per workgroup in a fixed order.  Without `history`
//                   only r_iters is reduced.
// Nothing syncs with the host or keeps state; every output but dv on way (a) is bit-identical from run to run on every
// input, and dv on way (a) wherever ops.warp's backward is.
#include "common.h"
#include <math.h>
#include "flow_sample.h"

namespace {

constexpr int INV_MAX_ITERS = 64;
constexpr int IC_WAVES = IC_T / 64;

// ------------------------------------------------------------------------------------------------ composition
template <int ND, int VPT>
__global__ __launch_bounds__(IC_T) void compose_fwd_k(const float* __restrict__ u, const float* __restrict__ v, IcGeom g,
                                                      float* __restrict__ out) {
  // VPT == 4: u arrives in su and c leaves through it (a thread overwrites the voxels it has read)
  __shared__ __attribute__((aligned(16))) float su[VPT == 4 ? ND * IC_ROW : 4];
  const IcThread<ND, VPT> th(g);
  const long long sb = (long long)th.b * ND * g.S;
  if (VPT == 4) {
    ic_stage_in<ND>(u + sb, g, th.q0, th.lq, su);
    __syncthreads();
  }
  int p[ND];
  th.first(g, p);
#pragma unroll
  for (int e = 0; e < VPT; ++e) {
    const unsigned j = th.j0 + 64u * e;
    if (j < (unsigned)g.S) {
      const int l = th.l0 + 64 * e;
      float uu[ND];
#pragma unroll
      for (int c = 0; c < ND; ++c) uu[c] = VPT == 4 ? su[c * IC_ROW + l] : u[sb + (long long)c * g.S + j];
      IcVox<ND> q;
      ic_voxel<ND>(v + sb, g, p, uu, q);
#pragma unroll
      for (int c = 0; c < ND; ++c) {
        if (VPT == 4) su[c * IC_ROW + l] = q.r[c];
        else out[sb + (long long)c * g.S + j] = q.r[c];
      }
    }
    if (e + 1 < VPT) ic_advance64<ND>(g, p);
  }
  if (VPT == 4) {
    __syncthreads();
    ic_stage_out<ND>(out + sb, g, th.q0, th.lq, su);
  }
}

// The gradient that reaches c comes from memory: directly (VPT == 1) or through the LDS rows the kernel staged it into
template <int VPT>
struct CmpGrad {
  static constexpr bool KR = false;          // the owner-gather adjoint reads g itself: nothing to write out
  const float* __restrict__ g;
  const float* sg;
  template <int ND>
  __device__ __forceinline__ float coef(const IcVox<ND>&, int c, int l, long long i) const {
    return VPT == 4 ? sg[c * IC_ROW + l] : g[i];
  }
};

template <int ND, int VPT>
__global__ __launch_bounds__(IC_T) void compose_bwd_k(const float* __restrict__ u, const float* __restrict__ v,
                                                      const float* __restrict__ gin, const unsigned* __restrict__ gmax,
                                                      IcGeom g, float* __restrict__ du,
                                                      unsigned long long* __restrict__ acc) {
  __shared__ __attribute__((aligned(16))) float su[VPT == 4 ? ND * IC_ROW : 4];
  __shared__ __attribute__((aligned(16))) float sg[VPT == 4 ? ND * IC_ROW : 4];
  const IcThread<ND, VPT> th(g);
  int ex = 0;
  const bool scatter = acc != nullptr && ic_fx_exp(1.f, __uint_as_float(gmax[0]), g, &ex);
  if (VPT == 4) ic_stage_in<ND>(gin + (long long)th.b * ND * g.S, g, th.q0, th.lq, sg);   // the barrier: ic_bwd_voxels
  ic_bwd_voxels<ND, VPT>(u, v, CmpGrad<VPT>{gin, sg}, 1.f, g, th, scatter, ex, du, acc, nullptr, su, sg);
}

// acc[0 .. n) = 0, the fixed-point sums, and acc[n], whose low word collects the bit pattern of max |g|
__global__ __launch_bounds__(IC_T) void cmp_zero_k(unsigned long long* __restrict__ acc, long long n) {
  const long long i = (long long)blockIdx.x * IC_T + threadIdx.x;
  if (i <= n) acc[i] = 0ull;
}

// out[0] = max over the n elements of the bit pattern of |g| (NaN orders above inf, so it stays): an integer maximum does not
// depend on the order the workgroups arrive in
__global__ __launch_bounds__(IC_T) void cmp_absmax_k(const float* __restrict__ gin, long long n, unsigned* __restrict__ out) {
  __shared__ unsigned sm[IC_WAVES];
  unsigned m = 0u;
  for (long long i = (long long)blockIdx.x * IC_T + threadIdx.x; i < n; i += (long long)gridDim.x * IC_T) {
    const unsigned bits = __float_as_uint(fabsf(gin[i]));
    m = bits > m ? bits : m;
  }
  m = ic_wave_max(m);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < IC_WAVES; ++w) m = sm[w] > m ? sm[w] : m;
    atomicMax(out, m);
  }
}

// dv = the fixed-point sums as floats (NaN when max |g| was not finite)
__global__ __launch_bounds__(IC_T) void cmp_cvt_k(const unsigned long long* __restrict__ acc, const unsigned* __restrict__ gmax,
                                                  IcGeom g, long long n, float* __restrict__ dv) {
  const long long i = (long long)blockIdx.x * IC_T + threadIdx.x;
  if (i >= n) return;
  int ex = 0;
  if (!ic_fx_exp(1.f, __uint_as_float(gmax[0]), g, &ex)) { dv[i] = __uint_as_float(0x7fc00000u); return; }
  dv[i] = (float)ldexp((double)(long long)acc[i], -ex);
}

// ------------------------------------------------------------------------------------------------ inversion
// psum / pmax: [K][B * nblk] slots, K = iters + 1 with history, else 1 (r_iters alone)
template <int ND, int VPT>
__global__ __launch_bounds__(IC_T) void invert_k(const float* __restrict__ u, const float* __restrict__ init, IcGeom g,
                                                 int iters, float tol, int history, float* __restrict__ wout,
                                                 double* __restrict__ psum, unsigned* __restrict__ pmax) {
  // VPT == 4: init arrives in sw and w leaves through it
  __shared__ __attribute__((aligned(16))) float sw[VPT == 4 ? ND * IC_ROW : 4];
  __shared__ double hs[(INV_MAX_ITERS + 1) * IC_WAVES];
  __shared__ unsigned hm[(INV_MAX_ITERS + 1) * IC_WAVES];
  const IcThread<ND, VPT> th(g);
  const long long sb = (long long)th.b * ND * g.S;
  if (VPT == 4) {
    if (init) ic_stage_in<ND>(init + sb, g, th.q0, th.lq, sw);
    __syncthreads();
  }
  int p[VPT][ND];
  float w[VPT][ND], r[VPT][ND];
  bool live[VPT], done[VPT];
  th.first(g, p[0]);
#pragma unroll
  for (int e = 0; e < VPT; ++e) {
    if (e > 0) {
#pragma unroll
      for (int a = 0; a < ND; ++a) p[e][a] = p[e - 1][a];
      ic_advance64<ND>(g, p[e]);
    }
    const unsigned j = th.j0 + 64u * e;
    live[e] = j < (unsigned)g.S;
    done[e] = false;
#pragma unroll
    for (int c = 0; c < ND; ++c) {
      r[e][c] = 0.f;
      w[e][c] = 0.f;
      if (init && live[e]) w[e][c] = VPT == 4 ? sw[c * IC_ROW + th.l0 + 64 * e] : init[sb + (long long)c * g.S + j];
    }
  }
  const int wave = threadIdx.x >> 6;
#pragma unroll 1
  for (int k = 0; k <= iters; ++k) {
    double acc = 0.0;
    unsigned mx = 0u;
#pragma unroll
    for (int e = 0; e < VPT; ++e) {
      if (!live[e]) continue;
      if (!done[e]) {                                             // a stopped voxel keeps its w, and so its r
        IcVox<ND> q;
        ic_voxel<ND>(u + sb, g, p[e], w[e], q);
        unsigned mb = 0u;                                         // bit patterns order as the values do, NaN on top:
#pragma unroll
        for (int c = 0; c < ND; ++c) {                            // a voxel with a NaN never counts as converged
          r[e][c] = q.r[c];
          const unsigned bits = __float_as_uint(fabsf(q.r[c]));
          mb = bits > mb ? bits : mb;
        }
        done[e] = mb <= __float_as_uint(tol);
      }
      float s2 = r[e][0] * r[e][0];
#pragma unroll
      for (int c = 1; c < ND; ++c) s2 += r[e][c] * r[e][c];
      acc += (double)s2;
#pragma unroll
      for (int c = 0; c < ND; ++c) {                              // bit patterns of |r|: NaN orders above inf, so it stays
        const unsigned bits = __float_as_uint(fabsf(r[e][c]));
        mx = bits > mx ? bits : mx;
        if (k < iters && !done[e]) w[e][c] -= r[e][c];
      }
    }
    if (history || k == iters) {                                  // per wave, no barrier: the waves meet once, at the end
      acc = wave_sum(acc);
      mx = ic_wave_max(mx);
      if ((threadIdx.x & 63) == 0) {
        const int slot = history ? k : 0;
        hs[slot * IC_WAVES + wave] = acc;
        hm[slot * IC_WAVES + wave] = mx;
      }
    }
  }
  if (VPT == 4) {
#pragma unroll
    for (int e = 0; e < VPT; ++e)
      if (live[e]) {
#pragma unroll
        for (int c = 0; c < ND; ++c) sw[c * IC_ROW + th.l0 + 64 * e] = w[e][c];
      }
  } else if (live[0]) {
#pragma unroll
    for (int c = 0; c < ND; ++c) wout[sb + (long long)c * g.S + th.j0] = w[0][c];
  }
  __syncthreads();
  if (VPT == 4) ic_stage_out<ND>(wout + sb, g, th.q0, th.lq, sw);
  const int K = history ? iters + 1 : 1;
  if ((int)threadIdx.x < K) {                                     // the waves of one iteration, in a fixed order
    double s = 0.0;
    unsigned m = 0u;
    for (int v = 0; v < IC_WAVES; ++v) {
      s += hs[threadIdx.x * IC_WAVES + v];
      m = hm[threadIdx.x * IC_WAVES + v] > m ? hm[threadIdx.x * IC_WAVES + v] : m;
    }
    const long long slot = (long long)threadIdx.x * gridDim.x + blockIdx.x;
    psum[slot] = s;
    pmax[slot] = m;
  }
}

// workgroup (k, b): stats[k][b] = (sqrt(the slots of sample b at iteration k, added in a fixed order, / S), max |r_c|)
__global__ __launch_bounds__(IC_T) void inv_fin_k(const double* __restrict__ psum, const unsigned* __restrict__ pmax, int B,
                                                  int nblk, double S, float* __restrict__ stats) {
  __shared__ double ss[IC_WAVES];
  __shared__ unsigned sm[IC_WAVES];
  const long long base = (long long)blockIdx.x * nblk;           // blockIdx.x = k * B + b, the slots are [K][B][nblk]
  double s = 0.0;
  unsigned m = 0u;
  for (int i = threadIdx.x; i < nblk; i += IC_T) {
    s += psum[base + i];
    const unsigned t = pmax[base + i];
    m = t > m ? t : m;
  }
  ic_block_reduce(s, m, ss, sm);
  if (threadIdx.x == 0) {
    stats[2LL * blockIdx.x] = (float)sqrt(s / S);
    stats[2LL * blockIdx.x + 1] = __uint_as_float(m);
  }
  (void)B;
}

inline bool inv_args(int iters, float tol) { return iters >= 0 && iters <= INV_MAX_ITERS && tol >= 0.f && tol <= 3.0e38f; }

}  // namespace

// warp_win.hip: the owner-gather adjoint of the warp (W % 4 == 0): d(src) without device-scope atomics
long long df_warp_win_bwd_own_ws(int nd, int B, int C, int D, int H, int W);
int df_warp_win_bwd_own_try(int nd, const float* dout, const float* src, const float* flow, float* dsrc, float* dflow,
                            int B, int C, int D, int H, int W, int add_identity, int flow_into_src, float* ws,
                            hipStream_t st);

extern "C" int dfmir_compose_fwd(int nd, const float* u, const float* v, float* out, int B, int D, int H, int W,
                                 void* stream) {
  IcGeom g;
  DF_ARG_CHECK(u && v && out);
  const int vpt = ic_vpt(W, u, out);
  DF_ARG_CHECK(ic_geom(nd, B, D, H, W, vpt, &g));
  hipStream_t st = (hipStream_t)stream;
  const unsigned nwg = (unsigned)((long long)B * g.nblk);
  if (nd == 3) {
    if (vpt == 4) compose_fwd_k<3, 4><<<nwg, IC_T, 0, st>>>(u, v, g, out);
    else compose_fwd_k<3, 1><<<nwg, IC_T, 0, st>>>(u, v, g, out);
  } else {
    if (vpt == 4) compose_fwd_k<2, 4><<<nwg, IC_T, 0, st>>>(u, v, g, out);
    else compose_fwd_k<2, 1><<<nwg, IC_T, 0, st>>>(u, v, g, out);
  }
  DF_LAUNCH_CHECK();
  return 0;
}

extern "C" long long dfmir_compose_bwd_ws_floats(int nd, int B, int D, int H, int W) {
  IcGeom g;
  if (!ic_geom(nd, B, D, H, W, 1, &g)) return -1;
  const long long n = (long long)B * nd * g.S;
  const long long own = W % 4 == 0 ? df_warp_win_bwd_own_ws(nd, B, nd, g.D, H, W) : 0;
  return own > 2 * n + 2 ? own : 2 * n + 2;  // one 64-bit sum per element of dv and one for max |g|, or the adjoint's scratch
}

extern "C" int dfmir_compose_bwd(int nd, const float* u, const float* v, const float* gin, float* du, float* dv, float* ws,
                                 int B, int D, int H, int W, void* stream) {
  IcGeom g;
  DF_ARG_CHECK(u && v && gin && (du || dv) && (!dv || (ws && (reinterpret_cast<uintptr_t>(ws) & 7) == 0)));
  const int vpt = (W % 4 == 0 && ((reinterpret_cast<uintptr_t>(u) | reinterpret_cast<uintptr_t>(gin) |
                                   reinterpret_cast<uintptr_t>(du)) & 15) == 0) ? 4 : 1;
  DF_ARG_CHECK(ic_geom(nd, B, D, H, W, vpt, &g));
  hipStream_t st = (hipStream_t)stream;
  const unsigned nwg = (unsigned)((long long)B * g.nblk);
  const long long n = (long long)B * nd * g.S;
  // dv: where the owner-gather adjoint of the warp takes the shape (W % 4 == 0, everything 16-byte aligned) g is handed to it
  // as it is -- no device-scope atomics; elsewhere the 64-bit fixed-point scatter
  static DfOptFlag fixed64{"DFMIR_INVCONS_FIXED64"};            // A/B: the fixed-point scatter on every shape
  const bool own = dv && W % 4 == 0 && !fixed64.get() && df_warp_win_bwd_own_ws(nd, B, nd, g.D, H, W) > 0 &&
                   ((reinterpret_cast<uintptr_t>(u) | reinterpret_cast<uintptr_t>(gin) | reinterpret_cast<uintptr_t>(dv) |
                     reinterpret_cast<uintptr_t>(ws)) & 15) == 0;
  unsigned long long* acc = dv && !own ? reinterpret_cast<unsigned long long*>(ws) : nullptr;
  const unsigned* gmax = acc ? reinterpret_cast<const unsigned*>(acc + n) : nullptr;
  const unsigned ngrid = (unsigned)((n + IC_T - 1) / IC_T);
  if (acc) {
    cmp_zero_k<<<(unsigned)((n + 1 + IC_T - 1) / IC_T), IC_T, 0, st>>>(acc, n);
    DF_LAUNCH_CHECK();
    cmp_absmax_k<<<ngrid < 1024u ? ngrid : 1024u, IC_T, 0, st>>>(gin, n, reinterpret_cast<unsigned*>(acc + n));
    DF_LAUNCH_CHECK();
  }
  if (du || acc) {
    if (nd == 3) {
      if (vpt == 4) compose_bwd_k<3, 4><<<nwg, IC_T, 0, st>>>(u, v, gin, gmax, g, du, acc);
      else compose_bwd_k<3, 1><<<nwg, IC_T, 0, st>>>(u, v, gin, gmax, g, du, acc);
    } else {
      if (vpt == 4) compose_bwd_k<2, 4><<<nwg, IC_T, 0, st>>>(u, v, gin, gmax, g, du, acc);
      else compose_bwd_k<2, 1><<<nwg, IC_T, 0, st>>>(u, v, gin, gmax, g, du, acc);
    }
    DF_LAUNCH_CHECK();
  }
  if (own) {
    if (df_warp_win_bwd_own_try(nd, gin, v, u, dv, nullptr, B, nd, g.D, H, W, 0, 0, ws, st) != 1)
      return df_set_error((int)hipErrorInvalidValue, __FILE__, __LINE__);
  } else if (dv) {
    cmp_cvt_k<<<ngrid, IC_T, 0, st>>>(acc, gmax, g, n, dv);
    DF_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" long long dfmir_flow_invert_ws_floats(int nd, int B, int D, int H, int W, int iters, int history) {
  IcGeom g;
  if (!ic_geom(nd, B, D, H, W, 1, &g) || !inv_args(iters, 0.f)) return -1;
  const long long K = history ? iters + 1 : 1;
  return 3LL * K * B * g.nblk;               // a double and an unsigned per workgroup of the scalar launch and reduced iteration
}

extern "C" int dfmir_flow_invert(int nd, const float* u, const float* init, float* w, float* stats, float* ws, int B, int D,
                                 int H, int W, int iters, float tol, int history, void* stream) {
  IcGeom g;
  DF_ARG_CHECK(u && w && stats && ws && (reinterpret_cast<uintptr_t>(ws) & 7) == 0 && inv_args(iters, tol));
  const int vpt = ic_vpt(W, init, w);
  DF_ARG_CHECK(ic_geom(nd, B, D, H, W, vpt, &g));
  IcGeom g1;
  ic_geom(nd, B, D, H, W, 1, &g1);
  hipStream_t st = (hipStream_t)stream;
  const unsigned nwg = (unsigned)((long long)B * g.nblk);
  const int K = history ? iters + 1 : 1;
  double* psum = reinterpret_cast<double*>(ws);
  unsigned* pmax = reinterpret_cast<unsigned*>(ws) + 2LL * K * B * g1.nblk;
  const int hist = history ? 1 : 0;
  if (nd == 3) {
    if (vpt == 4) invert_k<3, 4><<<nwg, IC_T, 0, st>>>(u, init, g, iters, tol, hist, w, psum, pmax);
    else invert_k<3, 1><<<nwg, IC_T, 0, st>>>(u, init, g, iters, tol, hist, w, psum, pmax);
  } else {
    if (vpt == 4) invert_k<2, 4><<<nwg, IC_T, 0, st>>>(u, init, g, iters, tol, hist, w, psum, pmax);
    else invert_k<2, 1><<<nwg, IC_T, 0, st>>>(u, init, g, iters, tol, hist, w, psum, pmax);
  }
  DF_LAUNCH_CHECK();
  inv_fin_k<<<(unsigned)(K * B), IC_T, 0, st>>>(psum, pmax, B, g.nblk, (double)g.S, stats);
  DF_LAUNCH_CHECK();
  return 0;
}
