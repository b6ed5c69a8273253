// What the kernels that sample one displacement field at the points another one names have in common (invcons.hip: the
// inverse-consistency loss; compose.hip: composition and fixed-point inversion of flows).  Fields are [B][ND][(D)][H][W]
// fp32, channel i displaces axis i in voxels, order (z,) y, x, as the warp kernels read a flow; sampling is (bi/tri)linear
// and corners outside the volume read as 0: the cell, the value and the corner weights are lin_cell.h's.  ic_voxel is the
// ONE place r(x) = u(x) + v(x + u(x)) and the corner terms are formed; IcThread says which voxels a thread owns (VPT = 4:
// 16-byte loads / stores through LDS when W % 4 == 0 and the pointers are aligned, else 1); ic_block_reduce adds a double
// and takes a maximum over the workgroup in a fixed order; ic_bwd_voxels is the adjoint of the sampling for a gradient that
// either file supplies.  Everything here has internal linkage: each file compiles its own copy.
#pragma once
#include "lin_cell.h"

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

// One voxel: the cell of the sample point p + u (lin_cell.h), its corners and r.  Bit ND - 1 - a of corner m is set when it
// is the upper one along axis a (x is bit 0).
template <int ND>
struct IcVox {
  static constexpr int NC = 1 << ND;
  LinCell<ND> cell;
  int off[NC];                               // offset of corner m in a channel of v, -1 when it lies outside
  float val[ND][NC];                         // v_c at the corners (0 outside)
  float r[ND];
};

template <int ND>
__device__ __forceinline__ void ic_voxel(const float* __restrict__ vb, const IcGeom& g, const int (&p)[ND],
                                         const float (&u)[ND], IcVox<ND>& q) {
  constexpr int NC = 1 << ND;
  int n[ND];
  lin_extents<ND>(g.D, g.H, g.W, n);
  lin_cell<ND, int>(p, u, n, q.cell);
#pragma unroll
  for (int m = 0; m < NC; ++m) q.off[m] = q.cell.in(m) ? q.cell.off(m) : -1;
#pragma unroll
  for (int c = 0; c < ND; ++c) {
    const float* vc = vb + (long long)c * g.S;
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
    q.r[c] = u[c] + lin_value<ND>(q.val[c], q.cell.w1);
  }
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

// ------------------------------------------------------------------------------------------------ adjoint of the sampling
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

// The adjoint of r = u + v(x + u) over the voxels of a thread, for an incoming gradient whose element c at a voxel is
// s * gr.coef(q, c, l, i) (l: the voxel's LDS index when VPT == 4, i: its index in a [B][ND][S] tensor).  invcons.hip: coef =
// r_c itself, s = k gout; compose.hip: coef = g_c from memory, s = 1.
//   du_a = s (coef_a + sum_c coef_c d_a v_c)     d_a v_c = sum over the corners of (+ upper, - lower along a) x the other weights
//   dv  += s coef_c x the corner weight, as 64-bit fixed-point integers of exponent ex (scatter), or left to the caller:
//          G::KR says whether s coef is written out (kr, through sk when VPT == 4) for the owner-gather adjoint of the warp
// VPT == 4: u arrives in su and du leaves through it (a thread overwrites the voxels it has read); su and sk hold ND * IC_ROW
// floats each.  Whatever coef reads from LDS must be there before the call: the barrier after the staging of u covers it.
template <int ND, int VPT, class G>
__device__ __forceinline__ void ic_bwd_voxels(const float* __restrict__ u, const float* __restrict__ v, const G& gr, float s,
                                              const IcGeom& g, const IcThread<ND, VPT>& th, bool scatter, int ex,
                                              float* __restrict__ du, unsigned long long* __restrict__ acc,
                                              float* __restrict__ kr, float* su, float* sk) {
  constexpr int NC = 1 << ND;
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
      float cf[ND];
#pragma unroll
      for (int c = 0; c < ND; ++c) cf[c] = gr.coef(q, c, l, sb + (long long)c * g.S + j);
#pragma unroll
      for (int a = 0; a < ND; ++a) {
        float t = 0.f;
#pragma unroll
        for (int c = 0; c < ND; ++c) {
          float dvc = 0.f;
#pragma unroll
          for (int m = 0; m < NC; ++m) {
            const float wv = lin_cw<ND>(q.cell.w1, m, 1.f, a) * q.val[c][m];
            dvc += ((m >> (ND - 1 - a)) & 1) ? wv : -wv;
          }
          t += cf[c] * dvc;
        }
        const float d = s * (cf[a] + t), gv = s * cf[a];
        if (VPT == 4) {
          su[a * IC_ROW + l] = d;
          if (G::KR) sk[a * IC_ROW + l] = gv;
        } else {
          if (du) du[sb + (long long)a * g.S + j] = d;
          if (G::KR && kr) kr[sb + (long long)a * g.S + j] = gv;
        }
      }
      if (scatter) {
        unsigned long long* ab = acc + sb;
#pragma unroll
        for (int m = 0; m < NC; ++m) {
          if (q.off[m] < 0) continue;
          const float wm = lin_cw<ND>(q.cell.w1, m);
#pragma unroll
          for (int c = 0; c < ND; ++c)
            atomicAdd(ab + (long long)c * g.S + q.off[m], (unsigned long long)__float2ll_rn(ldexpf(s * cf[c] * wm, ex)));
        }
      }
    }
    if (e + 1 < VPT) ic_advance64<ND>(g, p);
  }
  if (VPT == 4) {
    __syncthreads();
    if (du) ic_stage_out<ND>(du + sb, g, th.q0, th.lq, su);
    if (G::KR && kr) ic_stage_out<ND>(kr + sb, g, th.q0, th.lq, sk);
  }
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
