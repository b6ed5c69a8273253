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
// directions.
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

namespace {

constexpr int IC_T = 256;                    // threads per workgroup: 4 waves x 64 lanes

struct IcGeom {
  int D, H, W;                               // D == 1 for a 2-D field
  int S;                                     // voxels per sample
  int nblk;                                  // workgroups per sample
  int sh;                                    // fixed point: bits above the binary point that the sums may need
};

__device__ __forceinline__ unsigned ic_wave_max(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned t = __shfl_down(v, o, 64);
    v = t > v ? t : v;
  }
  return v;
}
// sum and maximum over the workgroup, valid in thread 0; the same order every run
__device__ __forceinline__ void ic_block_reduce(double& s, unsigned& m, double* ss, unsigned* sm /* IC_T / 64 each */) {
  s = wave_sum(s);
  m = ic_wave_max(m);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { ss[threadIdx.x >> 6] = s; sm[threadIdx.x >> 6] = m; }
  __syncthreads();
  if (threadIdx.x == 0) {
    s = 0.0; m = 0u;
    for (int w = 0; w < IC_T / 64; ++w) { s += ss[w]; m = sm[w] > m ? sm[w] : m; }
  }
}

struct __attribute__((packed, aligned(4))) IcPair { float a, b; };      // two neighbours along x, 4-byte aligned

// One voxel: the sample point p + u, its corners and r.  Bit ND - 1 - a of corner m is set when it is the upper one along
// axis a (x is bit 0).
template <int ND>
struct IcVox {
  static constexpr int NC = 1 << ND;
  float w[ND][2];                            // interpolation weights along each axis: lower, upper corner
  int off[NC];                               // offset of corner m in a channel of v, -1 when it lies outside
  float val[ND][NC];                         // v_c at the corners (0 outside)
  float r[ND];
};

template <int ND>
__device__ __forceinline__ void ic_voxel(const float* __restrict__ vb, const IcGeom& g, const int (&p)[ND],
                                         const float (&u)[ND], IcVox<ND>& q) {
  constexpr int NC = 1 << ND;
  int n[ND], st[ND], i0[ND];
  if (ND == 3) { n[0] = g.D; n[1] = g.H; n[2] = g.W; st[0] = g.H * g.W; st[1] = g.W; st[2] = 1; }
  else { n[0] = g.H; n[ND - 1] = g.W; st[0] = g.W; st[ND - 1] = 1; }
  bool ok[ND][2];
#pragma unroll
  for (int a = 0; a < ND; ++a) {
    const float f = (float)p[a] + u[a];
    const bool nearby = f >= -1.f && f < (float)n[a];             // false for NaN and for points past the padding cells:
    const float fl = floorf(f);                                 // no corner is read then, and no float goes to int
    i0[a] = nearby ? (int)fl : -2;
    q.w[a][1] = f - fl;
    q.w[a][0] = 1.f - q.w[a][1];
    ok[a][0] = (unsigned)i0[a] < (unsigned)n[a];
    ok[a][1] = (unsigned)(i0[a] + 1) < (unsigned)n[a];
  }
#pragma unroll
  for (int m = 0; m < NC; ++m) {
    bool in = true;
    int o = 0;
#pragma unroll
    for (int a = 0; a < ND; ++a) {
      const int bit = (m >> (ND - 1 - a)) & 1;                  // x is bit 0
      in = in && ok[a][bit];
      o += (i0[a] + bit) * st[a];
    }
    q.off[m] = in ? o : -1;
  }
#pragma unroll
  for (int c = 0; c < ND; ++c) {
    const float* vc = vb + (long long)c * g.S;
    float acc = 0.f;
    // the two x corners of a row of the cell travel as ONE 8-byte load (the gather is bound by the number of load
    // instructions, not by bytes): at the pair when both lie inside, else at the neighbouring pair that holds the one inside
    // -- every address is inside the channel, no branch
#pragma unroll
    for (int m = 0; m < NC; m += 2) {
      const int o0 = q.off[m], o1 = q.off[m + 1];
      const IcPair t = *reinterpret_cast<const IcPair*>(vc + (o0 >= 0 ? (o1 >= 0 ? o0 : o0 - 1) : (o1 >= 0 ? o1 : 0)));
      q.val[c][m] = o0 >= 0 ? (o1 >= 0 ? t.a : t.b) : 0.f;
      q.val[c][m + 1] = o1 >= 0 ? (o0 >= 0 ? t.b : t.a) : 0.f;
    }
    // x innermost, then y, then z: the order of the warp kernels
    if (ND == 3) {
      const float a0 = q.w[1][0] * (q.w[2][0] * q.val[c][0] + q.w[2][1] * q.val[c][1]) +
                       q.w[1][1] * (q.w[2][0] * q.val[c][2] + q.w[2][1] * q.val[c][3]);
      const float a1 = q.w[1][0] * (q.w[2][0] * q.val[c][4] + q.w[2][1] * q.val[c][5]) +
                       q.w[1][1] * (q.w[2][0] * q.val[c][6] + q.w[2][1] * q.val[c][NC - 1]);
      acc = q.w[0][0] * a0 + q.w[0][1] * a1;
    } else {
      acc = q.w[0][0] * (q.w[ND - 1][0] * q.val[c][0] + q.w[ND - 1][1] * q.val[c][1]) +
            q.w[0][1] * (q.w[ND - 1][0] * q.val[c][2] + q.w[ND - 1][1] * q.val[c][3]);
    }
    q.r[c] = u[c] + acc;
  }
}
// weight of corner m with x as bit 0 (axis a is bit ND - 1 - a)
template <int ND>
__device__ __forceinline__ float ic_cw(const IcVox<ND>& q, int m, int skip /* axis left out, -1 for none */) {
  float t = 1.f;
#pragma unroll
  for (int a = 0; a < ND; ++a)
    if (a != skip) t *= q.w[a][(m >> (ND - 1 - a)) & 1];
  return t;
}

// Which voxels a thread owns.  VPT == 1: one, workgroup base + thread.  VPT == 4: a wave owns 256 consecutive voxels; in
// MEMORY a lane holds the 16-byte quad 4 lane .. 4 lane + 3 of each channel (loads of u, stores of du and k r), for the
// ARITHMETIC it holds the voxels lane + 64 e -- neighbouring lanes gather from neighbouring addresses of v (with the quad as
// the unit a wave's gather touched four times the cache lines: 0.26 ms instead of the forward's time now at 160 x 192 x 224).
// The two orders meet in LDS (IcStage).
template <int ND, int VPT>
struct IcThread {
  int b;
  unsigned j0;                               // first voxel of the arithmetic order (the others: + 64 e)
  unsigned q0;                               // first voxel of the memory quad (VPT == 4)
  int l0;                                    // LDS index of voxel j0 within a channel row; the quad's is lq
  int lq;
  __device__ __forceinline__ IcThread(const IcGeom& g) {
    b = (int)(blockIdx.x / (unsigned)g.nblk);
    const unsigned blk = blockIdx.x - (unsigned)b * (unsigned)g.nblk;
    const unsigned base = blk * (unsigned)(IC_T * VPT);          // < S + IC_T * VPT < 2^31
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    l0 = VPT == 4 ? w * 64 * VPT + lane : (int)threadIdx.x;
    lq = VPT == 4 ? w * 64 * VPT + 4 * lane : (int)threadIdx.x;
    j0 = base + (unsigned)l0;
    q0 = base + (unsigned)lq;
  }
  // coordinates of voxel j0
  __device__ __forceinline__ void first(const IcGeom& g, int (&p)[ND]) const {
    unsigned t = j0;
    p[ND - 1] = (int)(t % (unsigned)g.W); t /= (unsigned)g.W;
    if (ND == 3) { p[1] = (int)(t % (unsigned)g.H); p[0] = (int)(t / (unsigned)g.H); }
    else p[0] = (int)t;
  }
};
// p += 64 voxels in memory order
template <int ND>
__device__ __forceinline__ void ic_advance64(const IcGeom& g, int (&p)[ND]) {
  p[ND - 1] += 64;
  while (p[ND - 1] >= g.W) { p[ND - 1] -= g.W; ++p[ND - 2]; }
  if (ND == 3)
    while (p[1] >= g.H) { p[1] -= g.H; ++p[0]; }
}

// VPT == 4: rows of IC_T * 4 floats per channel in LDS; a quad moves between global memory and LDS as 16 bytes
constexpr int IC_ROW = IC_T * 4;
template <int ND>
__device__ __forceinline__ void ic_stage_in(const float* __restrict__ ub, const IcGeom& g, unsigned q0, int lq, float* sm) {
  if (q0 < (unsigned)g.S) {                  // S % 4 == 0: a quad lies inside or outside as a whole
#pragma unroll
    for (int c = 0; c < ND; ++c)
      *reinterpret_cast<float4*>(sm + c * IC_ROW + lq) = *reinterpret_cast<const float4*>(ub + (long long)c * g.S + q0);
  }
}
template <int ND>
__device__ __forceinline__ void ic_stage_out(float* __restrict__ ob, const IcGeom& g, unsigned q0, int lq, const float* sm) {
  if (q0 < (unsigned)g.S) {
#pragma unroll
    for (int c = 0; c < ND; ++c)
      *reinterpret_cast<float4*>(ob + (long long)c * g.S + q0) = *reinterpret_cast<const float4*>(sm + c * IC_ROW + lq);
  }
}

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
// The fixed-point exponent of dv's sums: contributions are |c| <= (1 + a few ulp) M, M = |k gout| max |r_c| < 2^e, and a
// cell collects at most S of them (the weights of one voxel sum to 1): with sh = 61 - ceil(log2 S) the integer
// c 2^(sh - e) summed S times stays below 2^62.  false when M is not finite (dv is NaN then).
__device__ __forceinline__ bool ic_fx_exp(float s, float rmax, const IcGeom& g, int* ex) {
  const float M = fabsf(s) * rmax;
  if (!(M <= 3.0e38f)) return false;
  int e;
  frexpf(M, &e);                                                // M = m 2^e, 0.5 <= m < 1 (e = 0 for M == 0)
  *ex = g.sh - e;
  return true;
}

template <int ND, int VPT>
__global__ __launch_bounds__(IC_T) void ic_bwd_k(const float* __restrict__ u, const float* __restrict__ v,
                                                 const float* __restrict__ gout, const float* __restrict__ rmax, float k,
                                                 IcGeom g, float* __restrict__ du, unsigned long long* __restrict__ acc,
                                                 float* __restrict__ kr) {
  constexpr int NC = 1 << ND;
  // VPT == 4: u arrives in su and du leaves through it (a thread overwrites the voxels it has read); k r leaves through sk
  __shared__ __attribute__((aligned(16))) float su[VPT == 4 ? ND * IC_ROW : 4];
  __shared__ __attribute__((aligned(16))) float sk[VPT == 4 ? ND * IC_ROW : 4];
  const IcThread<ND, VPT> th(g);
  const float s = gout[0] * k;
  int ex = 0;
  const bool scatter = acc != nullptr && ic_fx_exp(s, rmax[0], g, &ex);
  const long long sb = (long long)th.b * ND * g.S;
  if (VPT == 4) {
    ic_stage_in<ND>(u + sb, g, th.q0, th.lq, su);
    __syncthreads();
  }
  int p[ND];
  th.first(g, p);
#pragma unroll 1
  for (int e = 0; e < VPT; ++e) {
    const unsigned j = th.j0 + 64u * e;
    if (j < (unsigned)g.S) {
      const int l = th.l0 + 64 * e;
      float uu[ND];
#pragma unroll
      for (int c = 0; c < ND; ++c) uu[c] = VPT == 4 ? su[c * IC_ROW + l] : u[sb + (long long)c * g.S + j];
      IcVox<ND> q;
      ic_voxel<ND>(v + sb, g, p, uu, q);
      // du_a = s (r_a + sum_c r_c d_a v_c): d_a v_c = sum over the corners of (+ upper, - lower along a) x the other weights
#pragma unroll
      for (int a = 0; a < ND; ++a) {
        float t = 0.f;
#pragma unroll
        for (int c = 0; c < ND; ++c) {
          float dvc = 0.f;
#pragma unroll
          for (int m = 0; m < NC; ++m) {
            const float wv = ic_cw<ND>(q, m, a) * q.val[c][m];
            dvc += ((m >> (ND - 1 - a)) & 1) ? wv : -wv;
          }
          t += q.r[c] * dvc;
        }
        const float d = s * (q.r[a] + t), gr = s * q.r[a];
        if (VPT == 4) {
          su[a * IC_ROW + l] = d;
          sk[a * IC_ROW + l] = gr;
        } else {
          if (du) du[sb + (long long)a * g.S + j] = d;
          if (kr) kr[sb + (long long)a * g.S + j] = gr;
        }
      }
      if (scatter) {
        unsigned long long* ab = acc + sb;
#pragma unroll
        for (int m = 0; m < NC; ++m) {
          if (q.off[m] < 0) continue;
          const float wm = ic_cw<ND>(q, m, -1);
#pragma unroll
          for (int c = 0; c < ND; ++c)
            atomicAdd(ab + (long long)c * g.S + q.off[m], (unsigned long long)__float2ll_rn(ldexpf(s * q.r[c] * wm, ex)));
        }
      }
    }
    if (e + 1 < VPT) ic_advance64<ND>(g, p);
  }
  if (VPT == 4) {
    __syncthreads();
    if (du) ic_stage_out<ND>(du + sb, g, th.q0, th.lq, su);
    if (kr) ic_stage_out<ND>(kr + sb, g, th.q0, th.lq, sk);
  }
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

// ------------------------------------------------------------------------------------------------ host side
// false for arguments the entry points refuse: nd outside {2, 3}, B < 1, an extent < 2 (D is not read when nd == 2), or
// 2^31 and more elements
bool ic_geom(int nd, int B, int D, int H, int W, int vpt, IcGeom* g) {
  if ((nd != 2 && nd != 3) || B < 1 || H < 2 || W < 2 || (nd == 3 && D < 2)) return false;
  if (nd == 2) D = 1;
  const long long S = (long long)D * H * W;
  if (S * nd * B >= (1LL << 31)) return false;
  g->D = D; g->H = H; g->W = W; g->S = (int)S;
  g->nblk = (int)((S + (long long)IC_T * vpt - 1) / ((long long)IC_T * vpt));
  int lg = 0;
  while ((1LL << lg) < S) ++lg;
  g->sh = 61 - lg;
  return true;
}
inline int ic_vpt(int W, const void* a, const void* b) {
  return (W % 4 == 0 && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0) ? 4 : 1;
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
