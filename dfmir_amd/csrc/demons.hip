// The demons force: a per-voxel Gauss-Newton step on the warped-feature SSD, 2-D and 3-D.  Build-defined
// (include/dfmir_hip.h and ops.demons_force state the definition); M, F, phi and the mask are dfmir_warp_ssd_fwd's:
//
//   p = x + phi(x);   m_c = M_c(p), J_c = the derivative of the interpolant in the cell floor() selects (ws_interp's d:
//   corner differences, zero-padded corners taking part as zeros), e_c = m_c - F_c(x)
//   s = (1/C) sum_c e_c^2      g = (1/C) sum_c e_c J_c  (nd)      H = (1/C) sum_c J_c J_c^T  (nd x nd, symmetric)
//   d(x) = -(H + (s / max_step^2) I)^-1 g            |d(x)| <= max_step / 2;  C = 1: -e J / (|J|^2 + e^2 / max_step^2)
//   g == 0 exactly (no corner inside the volume among the cases): d = +0 without a division; a mask weight <= 0: d = 0;
//   a component that is not finite: the vector is 0.  L, L_b = the (masked) mean of s, dfmir_warp_ssd_fwd's reduction.
//
//   dm_fwd_k   ws_fwd_k's pass (warpssd.hip) with other accumulators: lanes run along x, a workgroup owns WS_T * VPT
//              consecutive voxels of ONE sample and each wave 64 * VPT of them, 64 at a time (VPT = 4 with 16-byte accesses
//              of phi, F and d when W % 4 == 0 and the pointers are aligned, else 1; the two orders meet in LDS rows the
//              wave owns, the quads of the next 64 voxels are fetched while the current ones are gathered).  The cell is
//              formed once per voxel (ws_cell's guards), the channels pass in groups of four from the packed copy: e^2,
//              e J and the upper triangle of J J^T are added IN DOUBLE -- 1 + 3 + 6 sums in 3-D, 1 + 2 + 3 in 2-D -- and the
//              system is solved in closed form by its L D L^T factors, in double (dm_solve says why).  sum m s C and sum m
//              leave as two double slots per workgroup.  No warped tensor, no e tensor, no atomics.
//   ws_fin_k   (ws_sample.h, shared with warpssd.hip, here without its scale output; one workgroup) adds the slots of each
//              sample in a fixed order: L_b and L.  Bit-identical from run to run.
// Nothing syncs with the host or keeps state.
#include "ws_sample.h"

namespace {

// One voxel, one channel group: s2 += sum_c e_c^2, gr_a += sum_c e_c J_ca, hh += the upper triangle of sum_c J_c J_c^T in
// the order (0,0) (0,1) .. (0,ND-1) (1,1) ..
template <int ND>
__device__ __forceinline__ void dm_group(const float* __restrict__ mb, const WsGeom& g, const WsCell<ND>& q, int gi,
                                         const float (&f)[4], double& s2, double (&gr)[ND], double (&hh)[ND * (ND + 1) / 2]) {
  constexpr int NC = 1 << ND;
  float4 val[NC];
  ws_corners<ND, true>(mb, g, q, gi, val);
#pragma unroll
  for (int cc = 0; cc < 4; ++cc) {
    float v[NC], d[ND];
#pragma unroll
    for (int m = 0; m < NC; ++m) v[m] = cc == 0 ? val[m].x : cc == 1 ? val[m].y : cc == 2 ? val[m].z : val[m].w;
    const float e = ws_interp<ND>(v, q, d) - f[cc];             // a channel >= C: corners and f are 0, e = 0 and J = 0
    const double ed = e;                                        // (a product of two floats is exact in double)
    s2 += ed * ed;
    int t = 0;
#pragma unroll
    for (int a = 0; a < ND; ++a) {
      const double da = d[a];
      gr[a] += ed * da;
#pragma unroll
      for (int b = a; b < ND; ++b) hh[t++] += da * (double)d[b];
    }
  }
}

// d = -(H + a I)^-1 g in closed form: the L D L^T factors of the symmetric positive definite matrix, written out, in double.
// Near convergence e is small against |J| and a = s / max_step^2 falls far below |J|^2 (a ratio of 1e7 and more with one
// channel, where H = J J^T has rank 1).  Two things then decide the result.  The sums must be exact enough that g stays in the
// span of the J_c: fp32 sums perturb H by eps32 |J|^2 > a and the solution of THAT system is off by the order of |d| itself,
// whatever solves it -- so the products are added in double, where each is exact.  And the adjugate over the determinant
// cancels twice (the cofactors down to a |J|^2, the determinant down to a^2 |J|^2): its error is eps (|J|^2 / a)^2, percents
// even in double; the factorisation's is eps |J|^2 / a.
__device__ __forceinline__ void dm_solve(const double (&g)[2], const double (&h)[3], double a, float (&d)[2]) {
  const double d0 = h[0] + a, l10 = h[1] / d0, d1 = (h[2] + a) - l10 * h[1];
  const double z1 = g[1] - l10 * g[0];
  const double x1 = z1 / d1, x0 = g[0] / d0 - l10 * x1;
  d[0] = (float)-x0;
  d[1] = (float)-x1;
}

__device__ __forceinline__ void dm_solve(const double (&g)[3], const double (&h)[6], double a, float (&d)[3]) {
  const double d0 = h[0] + a, l10 = h[1] / d0, l20 = h[2] / d0;
  const double d1 = (h[3] + a) - l10 * h[1], l21 = (h[4] - l20 * h[1]) / d1;
  const double d2 = (h[5] + a) - l20 * h[2] - l21 * l21 * d1;
  const double z1 = g[1] - l10 * g[0], z2 = g[2] - l20 * g[0] - l21 * z1;
  const double x2 = z2 / d2, x1 = z1 / d1 - l21 * x2, x0 = g[0] / d0 - l10 * x1 - l20 * x2;
  d[0] = (float)-x0;
  d[1] = (float)-x1;
  d[2] = (float)-x2;
}

// part[2 wg] = sum m sum_c e^2, part[2 wg + 1] = sum m over the workgroup's voxels (m = 1 without a mask); dout = the force.
// The walk over the workgroup's voxels -- thread geometry, prefetch, the 16-byte to one-voxel-per-lane staging in the wave's LDS
// rows, the channel-group loop, the staged store and the two ordered sums -- repeats ws_fwd_k's (warpssd.hip), whose comments
// explain it; only the per-voxel arithmetic differs.  The two stay separate kernels: profiles/walk_tile_ab.txt has the shared
// forms that were tried and what they cost.
template <int ND, int VPT>
__global__ __launch_bounds__(WS_T) void dm_fwd_k(const float* __restrict__ mov, const float* __restrict__ fix,
                                                 const float* __restrict__ phi, const float* __restrict__ mask, WsGeom g,
                                                 double inv_c, double inv_ms2, double* __restrict__ part,
                                                 float* __restrict__ dout) {
  constexpr int NW = WS_T / 64;
  constexpr int NH = ND * (ND + 1) / 2;
  __shared__ __attribute__((aligned(16))) float sin_[VPT == 4 ? NW * (WS_MAXC + ND) * 64 : 4];
  __shared__ __attribute__((aligned(16))) float sout[VPT == 4 ? NW * ND * 64 : 4];
  __shared__ double red[NW];
  const int b = (int)(blockIdx.x / (unsigned)g.nblk);
  const unsigned blk = blockIdx.x - (unsigned)b * (unsigned)g.nblk;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const unsigned v0 = blk * (unsigned)(WS_T * VPT) + (unsigned)(wv * 64 * VPT);      // < S + WS_T * VPT < 2^31
  const float* pb = phi + (long long)b * ND * g.S;
  const float* fb = fix + (long long)b * g.C * g.S;
  const float* mb = mov + (long long)b * g.Cp * g.S;
  float* ob = dout + (long long)b * ND * g.S;
  float* sf = sin_ + wv * (WS_MAXC + ND) * 64;                    // rows 0 .. Cp - 1: F; rows WS_MAXC .. : phi
  float* so = sout + wv * ND * 64;
  const int row = lane >> 4, quad = (lane & 15) << 2;            // VPT == 4: this lane's share of a 4-row, 64-voxel load
  const int ng = g.Cp >> 2;
  double acc = 0.0, wsum = 0.0;
  float4 pf[WS_MAXC / 4], pp;
  auto fetch = [&](unsigned vb) {
    if (vb + (unsigned)quad < (unsigned)g.S) {                 // S % 4 == 0: a quad lies inside or outside as a whole
      if (row < ND) pp = *reinterpret_cast<const float4*>(pb + (long long)row * g.S + vb + quad);
#pragma unroll
      for (int gi = 0; gi < WS_MAXC / 4; ++gi)
        if (gi < ng) {
          const int c = 4 * gi + row;
          pf[gi] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (c < g.C) pf[gi] = *reinterpret_cast<const float4*>(fb + (long long)c * g.S + vb + quad);
        }
    }
  };
  if (VPT == 4) fetch(v0);
#pragma unroll 1
  for (int e = 0; e < VPT; ++e) {
    const unsigned vb = v0 + 64u * e;                            // the 64 voxels of this pass: vb + lane
    const unsigned j = vb + (unsigned)lane;
    const bool quad_in = vb + (unsigned)quad < (unsigned)g.S;
    if (VPT == 4) {
      if (quad_in) {
        if (row < ND) *reinterpret_cast<float4*>(sf + (WS_MAXC + row) * 64 + quad) = pp;
#pragma unroll
        for (int gi = 0; gi < WS_MAXC / 4; ++gi)
          if (gi < ng) *reinterpret_cast<float4*>(sf + (4 * gi + row) * 64 + quad) = pf[gi];
      }
      __syncthreads();
      if (e + 1 < VPT) fetch(vb + 64u);
    }
    if (j < (unsigned)g.S) {
      int p[ND];
      unsigned t = j;
      p[ND - 1] = (int)(t % (unsigned)g.W); t /= (unsigned)g.W;
      if (ND == 3) { p[1] = (int)(t % (unsigned)g.H); p[0] = (int)(t / (unsigned)g.H); }
      else p[0] = (int)t;
      float u[ND];
      double gr[ND], hh[NH];
#pragma unroll
      for (int c = 0; c < ND; ++c) {
        u[c] = VPT == 4 ? sf[(WS_MAXC + c) * 64 + lane] : pb[(long long)c * g.S + j];
        gr[c] = 0.0;
      }
#pragma unroll
      for (int c = 0; c < NH; ++c) hh[c] = 0.0;
      WsCell<ND> cell;
      ws_cell<ND>(g, p, u, cell);
      double s2 = 0.0;
      for (int gi = 0; gi < ng; ++gi) {
        float f[4];
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
          if (VPT == 4) f[cc] = sf[(4 * gi + cc) * 64 + lane];
          else f[cc] = 4 * gi + cc < g.C ? fb[(long long)(4 * gi + cc) * g.S + j] : 0.f;
        }
        dm_group<ND>(mb, g, cell, gi, f, s2, gr, hh);
      }
      const float m = mask ? mask[(long long)b * g.S + j] : 1.f;
      acc += (double)m * s2;
      wsum += (double)m;
      float d[ND];
      bool live = m > 0.f, nz = false;
#pragma unroll
      for (int a = 0; a < ND; ++a) {
        nz = nz || gr[a] != 0.0;
        gr[a] *= inv_c;
        d[a] = 0.f;
      }
      if (live && nz) {
#pragma unroll
        for (int c = 0; c < NH; ++c) hh[c] *= inv_c;
        dm_solve(gr, hh, s2 * inv_c * inv_ms2, d);
        bool fin = true;
#pragma unroll
        for (int a = 0; a < ND; ++a) fin = fin && fabsf(d[a]) < INFINITY;       // false for NaN too
        if (!fin) {
#pragma unroll
          for (int a = 0; a < ND; ++a) d[a] = 0.f;
        }
      }
#pragma unroll
      for (int a = 0; a < ND; ++a) {
        if (VPT == 4) so[a * 64 + lane] = d[a];
        else ob[(long long)a * g.S + j] = d[a];
      }
    }
    if (VPT == 4) {
      __syncthreads();        // (also: every lane is done with sf before the next pass overwrites it)
      if (quad_in && row < ND)
        *reinterpret_cast<float4*>(ob + (long long)row * g.S + vb + quad) = *reinterpret_cast<const float4*>(so + row * 64 + quad);
    }
  }
  acc = block_sum_ordered<WS_T>(acc, red);
  wsum = block_sum_ordered<WS_T>(wsum, red);
  if (threadIdx.x == 0) { part[2LL * blockIdx.x] = acc; part[2LL * blockIdx.x + 1] = wsum; }
}

}  // namespace

extern "C" long long dfmir_demons_ws_floats(int nd, int B, int C, int D, int H, int W) {
  WsGeom g;
  if (!ws_geom(nd, B, C, D, H, W, 1, &g)) return -1;
  return 4LL * B * g.nblk;                   // two doubles per workgroup of the scalar launch (the larger)
}

extern "C" int dfmir_demons_force(int nd, const float* Mp, const float* F, const float* phi, const float* mask, float* ws,
                                  float* per_sample, float* loss, float* d, float max_step, int B, int C, int D, int H, int W,
                                  void* stream) {
  WsGeom g;
  DF_ARG_CHECK(Mp && F && phi && ws && per_sample && loss && d && (reinterpret_cast<uintptr_t>(ws) & 7) == 0);
  DF_ARG_CHECK(ws_al16(Mp) && d != phi);
  DF_ARG_CHECK(max_step > 0.f && max_step < INFINITY);
  const int vpt = (W % 4 == 0 && ws_al16(F) && ws_al16(phi) && ws_al16(d)) ? 4 : 1;
  DF_ARG_CHECK(ws_geom(nd, B, C, D, H, W, vpt, &g));
  hipStream_t st = (hipStream_t)stream;
  const unsigned nwg = (unsigned)((long long)B * g.nblk);
  double* part = reinterpret_cast<double*>(ws);
  const double inv_c = 1.0 / (double)C;
  const double inv_ms2 = 1.0 / ((double)max_step * (double)max_step);
#define DM_LAUNCH(ND_, VPT_) dm_fwd_k<ND_, VPT_><<<nwg, WS_T, 0, st>>>(Mp, F, phi, mask, g, inv_c, inv_ms2, part, d)
  if (nd == 3) { if (vpt == 4) DM_LAUNCH(3, 4); else DM_LAUNCH(3, 1); }
  else { if (vpt == 4) DM_LAUNCH(2, 4); else DM_LAUNCH(2, 1); }
#undef DM_LAUNCH
  DF_LAUNCH_CHECK();
  ws_fin_k<WS_T><<<1, WS_T, 0, st>>>(part, B, g.nblk, (double)C, mask ? 1 : 0, per_sample, loss, nullptr);
  DF_LAUNCH_CHECK();
  return 0;
}
