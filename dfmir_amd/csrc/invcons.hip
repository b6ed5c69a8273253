// Inverse-consistency loss of a pair of displacement fields, forward and backward, 2-D and 3-D.  Build-defined
// (include/dfmir_hip.h and losses.InverseConsistency_Loss state the definition):
//
//   u, v [B][ND][(D)][H][W] fp32, channel i displaces axis i in voxels, order (z,) y, x, as the warp kernels read a flow.
//   r(x)    = u(x) + v(x + u(x))      v sampled (bi/tri)linearly, corners outside the volume read as 0
//   IC_b    = sum over the ND * S elements of sample b of r^2 / (ND * S),      loss = mean_b IC_b
//   du_c(x) = k ( r_c(x) + sum_c' r_c'(x) d_c v_c'(x + u(x)) ),   k = 2 gout / (B ND S); d_c = the derivative of the
//             interpolant: corner differences, zero-padded corners taking part as zeros
//   dv      = the transpose of the interpolation applied to k r (a scatter to the up to 2^ND corners)
//
// An HBM-bound gather with an L2-served neighbourhood, as the plain warp kernels: lanes run along x, a workgroup owns
// IC_T * VPT consecutive voxels of ONE sample (VPT = 4 with 16-byte loads / stores of u, du and k r when W % 4 == 0 and the
// pointers are aligned, else 1; see IcThread).  ic_voxel is the ONE place r and the corner terms are formed, for both
// directions.  IcGeom, ic_voxel, IcThread, the block reduce and the backward's body (ic_bwd_voxels) live in flow_sample.h,
// which compose.hip shares.
//   ic_fwd_k   r in registers, never stored: |r|^2 added in double per thread, one double slot per workgroup, and the
//              workgroup's max |r_c| beside it.  ic_fin_k (one workgroup) adds the slots of each sample in a fixed order:
//              per-sample IC, the loss, and max |r_c| over the call (the backward's fixed-point range).
//   ic_bwd_k   recomputes r and writes du.  dv, the transpose of the interpolation applied to k r, takes one of two ways:
//              (a) W % 4 == 0, everything 16-byte aligned: k r is written once and handed to the owner-gather adjoint of
//                  the warp (warp_win.hip: no device-scope atomics; bit-reproducible as ops.warp's backward is: all but
//                  the voxels whose taps leave the 3 x 3 (x 3) tiles around their own, none on registration-like fields);
//              (b) elsewhere k r is scattered to the corners as 64-bit FIXED-POINT integers with global atomics: integer
//                  addition is associative, so dv does not depend on the order the adds arrive in -- bit-identical from
//                  run to run.  The scale is a power of two chosen on the device from gout and max |r_c| such that a
//                  cell that collected EVERY voxel of its sample cannot overflow; the unit is >= 29 bits below max |k r|,
//                  so a contribution keeps its whole fp32 mantissa unless it is 2^-5 and more below the largest.
//                  ic_zero_k clears the sums, ic_cvt_k turns them into floats; a non-finite max |k r| makes dv NaN.
//                  One 8-byte atomic per corner and channel: several times slower than (a) (3.0 ms against 0.47 ms at
//                  160 x 192 x 224), which is why (a) is taken where it can be.  DFMIR_INVCONS_FIXED64 forces (b).
// Nothing syncs with the host (gout is read on the device) or keeps state.
#include "common.h"
#include <math.h>
#include "flow_sample.h"

namespace {

// ------------------------------------------------------------------------------------------------ forward
template <int ND, int VPT>
__global__ __launch_bounds__(IC_T) void ic_fwd_k(const float* __restrict__ u, const float* __restrict__ v, IcGeom g,
                                                 double* __restrict__ psum, unsigned* __restrict__ pmax) {
  __shared__ __attribute__((aligned(16))) float su[VPT == 4 ? ND * IC_ROW : 4];
  __shared__ double ss[IC_T / 64];
  __shared__ unsigned sm[IC_T / 64];
  const IcThread<ND, VPT> th(g);
  const long long sb = (long long)th.b * ND * g.S;
  if (VPT == 4) {
    ic_stage_in<ND>(u + sb, g, th.q0, th.lq, su);
    __syncthreads();
  }
  double acc = 0.0;
  unsigned mx = 0u;
  int p[ND];
  th.first(g, p);
#pragma unroll
  for (int e = 0; e < VPT; ++e) {
    const unsigned j = th.j0 + 64u * e;
    if (j < (unsigned)g.S) {
      float uu[ND];
#pragma unroll
      for (int c = 0; c < ND; ++c) uu[c] = VPT == 4 ? su[c * IC_ROW + th.l0 + 64 * e] : u[sb + (long long)c * g.S + j];
      IcVox<ND> q;
      ic_voxel<ND>(v + sb, g, p, uu, q);
      float s2 = q.r[0] * q.r[0];
#pragma unroll
      for (int c = 1; c < ND; ++c) s2 += q.r[c] * q.r[c];
      acc += (double)s2;
#pragma unroll
      for (int c = 0; c < ND; ++c) {                            // bit patterns of |r|: NaN orders above inf, so it stays
        const unsigned bits = __float_as_uint(fabsf(q.r[c]));
        mx = bits > mx ? bits : mx;
      }
    }
    if (e + 1 < VPT) ic_advance64<ND>(g, p);
  }
  ic_block_reduce(acc, mx, ss, sm);
  if (threadIdx.x == 0) { psum[blockIdx.x] = acc; pmax[blockIdx.x] = mx; }
}

// per[b] = (the slots of sample b, added in a fixed order) / (ND S); loss = their sum / (B ND S); rmax = max |r_c|
__global__ __launch_bounds__(IC_T) void ic_fin_k(const double* __restrict__ psum, const unsigned* __restrict__ pmax,
                                                 int B, int nblk, double per_count, float* __restrict__ per,
                                                 float* __restrict__ loss, float* __restrict__ rmax) {
  __shared__ double ss[IC_T / 64];
  __shared__ unsigned sm[IC_T / 64];
  double total = 0.0;
  unsigned mall = 0u;
  for (int b = 0; b < B; ++b) {
    double s = 0.0;
    unsigned m = 0u;
    for (int i = threadIdx.x; i < nblk; i += IC_T) {
      s += psum[(long long)b * nblk + i];
      const unsigned t = pmax[(long long)b * nblk + i];
      m = t > m ? t : m;
    }
    ic_block_reduce(s, m, ss, sm);
    if (threadIdx.x == 0) {
      per[b] = (float)(s / per_count);
      total += s;
      mall = m > mall ? m : mall;
    }
  }
  if (threadIdx.x == 0) {
    loss[0] = (float)(total / (per_count * (double)B));
    rmax[0] = __uint_as_float(mall);
  }
}


// ------------------------------------------------------------------------------------------------ backward
// The gradient that reaches r is k gout r itself: ic_bwd_voxels (flow_sample.h) reads its coefficient from the voxel
struct IcResidual {
  static constexpr bool KR = true;           // k r is written out for the owner-gather adjoint
  template <int ND>
  __device__ __forceinline__ float coef(const IcVox<ND>& q, int c, int, long long) const { return q.r[c]; }
};

template <int ND, int VPT>
__global__ __launch_bounds__(IC_T) void ic_bwd_k(const float* __restrict__ u, const float* __restrict__ v,
                                                 const float* __restrict__ gout, const float* __restrict__ rmax, float k,
                                                 IcGeom g, float* __restrict__ du, unsigned long long* __restrict__ acc,
                                                 float* __restrict__ kr) {
  // VPT == 4: u arrives in su and du leaves through it (a thread overwrites the voxels it has read); k r leaves through sk
  __shared__ __attribute__((aligned(16))) float su[VPT == 4 ? ND * IC_ROW : 4];
  __shared__ __attribute__((aligned(16))) float sk[VPT == 4 ? ND * IC_ROW : 4];
  const IcThread<ND, VPT> th(g);
  const float s = gout[0] * k;
  int ex = 0;
  const bool scatter = acc != nullptr && ic_fx_exp(s, rmax[0], g, &ex);
  ic_bwd_voxels<ND, VPT>(u, v, IcResidual(), s, g, th, scatter, ex, du, acc, kr, su, sk);
}

__global__ __launch_bounds__(IC_T) void ic_zero_k(unsigned long long* __restrict__ acc, long long n) {
  const long long i = (long long)blockIdx.x * IC_T + threadIdx.x;
  if (i < n) acc[i] = 0ull;
}

// dv = the fixed-point sums as floats (NaN when the range was not finite)
__global__ __launch_bounds__(IC_T) void ic_cvt_k(const unsigned long long* __restrict__ acc, const float* __restrict__ gout,
                                                 const float* __restrict__ rmax, float k, IcGeom g, long long n,
                                                 float* __restrict__ dv) {
  const long long i = (long long)blockIdx.x * IC_T + threadIdx.x;
  if (i >= n) return;
  int ex = 0;
  if (!ic_fx_exp(gout[0] * k, rmax[0], g, &ex)) { dv[i] = __uint_as_float(0x7fc00000u); return; }
  dv[i] = (float)ldexp((double)(long long)acc[i], -ex);
}


}  // namespace

// warp_win.hip: the owner-gather adjoint of the warp (W % 4 == 0): d(src) without device-scope atomics
long long df_warp_win_bwd_own_ws(int nd, int B, int C, int D, int H, int W);
int df_warp_win_bwd_own_try(int nd, const float* dout, const float* src, const float* flow, float* dsrc, float* dflow,
                            int B, int C, int D, int H, int W, int add_identity, int flow_into_src, float* ws,
                            hipStream_t st);

extern "C" long long dfmir_invcons_ws_floats(int nd, int B, int D, int H, int W) {
  IcGeom g;
  if (!ic_geom(nd, B, D, H, W, 1, &g)) return -1;
  return 3LL * B * g.nblk;                   // a double and an unsigned per workgroup of the scalar launch (the larger)
}

extern "C" int dfmir_invcons_fwd(int nd, const float* u, const float* v, float* ws, float* per_sample, float* loss,
                                 float* rmax, int B, int D, int H, int W, void* stream) {
  IcGeom g;
  DF_ARG_CHECK(u && v && ws && per_sample && loss && rmax && (reinterpret_cast<uintptr_t>(ws) & 7) == 0);
  const int vpt = ic_vpt(W, u, nullptr);
  DF_ARG_CHECK(ic_geom(nd, B, D, H, W, vpt, &g));
  IcGeom g1;
  ic_geom(nd, B, D, H, W, 1, &g1);
  hipStream_t st = (hipStream_t)stream;
  const unsigned nwg = (unsigned)((long long)B * g.nblk);
  double* psum = reinterpret_cast<double*>(ws);
  unsigned* pmax = reinterpret_cast<unsigned*>(ws) + 2LL * B * g1.nblk;
  if (nd == 3) {
    if (vpt == 4) ic_fwd_k<3, 4><<<nwg, IC_T, 0, st>>>(u, v, g, psum, pmax);
    else ic_fwd_k<3, 1><<<nwg, IC_T, 0, st>>>(u, v, g, psum, pmax);
  } else {
    if (vpt == 4) ic_fwd_k<2, 4><<<nwg, IC_T, 0, st>>>(u, v, g, psum, pmax);
    else ic_fwd_k<2, 1><<<nwg, IC_T, 0, st>>>(u, v, g, psum, pmax);
  }
  DF_LAUNCH_CHECK();
  ic_fin_k<<<1, IC_T, 0, st>>>(psum, pmax, B, g.nblk, (double)nd * (double)g.S, per_sample, loss, rmax);
  DF_LAUNCH_CHECK();
  return 0;
}

extern "C" long long dfmir_invcons_bwd_ws_floats(int nd, int B, int D, int H, int W) {
  IcGeom g;
  if (!ic_geom(nd, B, D, H, W, 1, &g)) return -1;
  const long long n = (long long)B * nd * g.S;
  const long long own = W % 4 == 0 ? df_warp_win_bwd_own_ws(nd, B, nd, g.D, H, W) : 0;
  return own > 0 && n + own > 2 * n ? n + own : 2 * n;    // one 64-bit sum per element of dv, or k r + the adjoint's scratch
}

extern "C" int dfmir_invcons_bwd(int nd, const float* u, const float* v, const float* gout, const float* rmax, float* du,
                                 float* dv, float* ws, int B, int D, int H, int W, void* stream) {
  IcGeom g;
  DF_ARG_CHECK(u && v && gout && rmax && (du || dv) && (!dv || (ws && (reinterpret_cast<uintptr_t>(ws) & 7) == 0)));
  const int vpt = ic_vpt(W, u, du);
  DF_ARG_CHECK(ic_geom(nd, B, D, H, W, vpt, &g));
  hipStream_t st = (hipStream_t)stream;
  const unsigned nwg = (unsigned)((long long)B * g.nblk);
  const long long n = (long long)B * nd * g.S;
  const unsigned ngrid = (unsigned)((n + IC_T - 1) / IC_T);
  const float k = (float)(2.0 / ((double)B * nd * (double)g.S));
  // dv: where the owner-gather adjoint of the warp takes the shape (W % 4 == 0, everything 16-byte aligned) k r is written
  // once and handed to it -- no device-scope atomics; elsewhere the 64-bit fixed-point scatter
  static DfOptFlag fixed64{"DFMIR_INVCONS_FIXED64"};            // A/B: the fixed-point scatter on every shape
  const bool own = dv && vpt == 4 && !fixed64.get() && df_warp_win_bwd_own_ws(nd, B, nd, g.D, H, W) > 0 &&
                   ((reinterpret_cast<uintptr_t>(dv) | reinterpret_cast<uintptr_t>(ws)) & 15) == 0;
  unsigned long long* acc = dv && !own ? reinterpret_cast<unsigned long long*>(ws) : nullptr;
  float* kr = own ? ws : nullptr;
  if (acc) {
    ic_zero_k<<<ngrid, IC_T, 0, st>>>(acc, n);
    DF_LAUNCH_CHECK();
  }
  if (nd == 3) {
    if (vpt == 4) ic_bwd_k<3, 4><<<nwg, IC_T, 0, st>>>(u, v, gout, rmax, k, g, du, acc, kr);
    else ic_bwd_k<3, 1><<<nwg, IC_T, 0, st>>>(u, v, gout, rmax, k, g, du, acc, kr);
  } else {
    if (vpt == 4) ic_bwd_k<2, 4><<<nwg, IC_T, 0, st>>>(u, v, gout, rmax, k, g, du, acc, kr);
    else ic_bwd_k<2, 1><<<nwg, IC_T, 0, st>>>(u, v, gout, rmax, k, g, du, acc, kr);
  }
  DF_LAUNCH_CHECK();
  if (own) {
    if (df_warp_win_bwd_own_try(nd, kr, v, u, dv, nullptr, B, nd, g.D, H, W, 0, 0, ws + n, st) != 1)
      return df_set_error((int)hipErrorInvalidValue, __FILE__, __LINE__);
  } else if (dv) {
    ic_cvt_k<<<ngrid, IC_T, 0, st>>>(acc, gout, rmax, k, g, n, dv);
    DF_LAUNCH_CHECK();
  }
  return 0;
}
