// Thin-plate / polyharmonic spline interpolation of landmark displacements: the dense flow of K control points and its adjoint
// with respect to the coefficients, 2-D and 3-D.  Build-defined (include/dfmir_hip.h and ops.tps_fit state the definition):
//
//   ctrl q [B][K][ND] fp32 voxel coordinates, axis order (z,) y, x as the flow's channels; scale sc_a = h_a / L, L = max_a
//   h_a (S_a - 1), so the normalised coordinates xh_a = sc_a x_a of the volume lie in [0, 1]; coef [B][K + ND + 1][ND] float64 =
//   [w (K rows); a_0; A (ND rows)];
//   u_a(x) = a_0[a] + sum_c xh_c A[c][a] + sum_k w[k][a] phi(|xh - qh_k|)
//   phi(r) = -r (3-D) or r^2 log r = 1/2 s log s, s = r^2, phi(0) = 0 (2-D, no square root).
//
// An O(N K) pair sum with nothing to reuse but the control points: a few hundred bytes per workgroup, the rest is ALU.  The
// basis value is fp32 (normalised coordinates rounded once from the double product, the squared distance and phi in fp32; the
// accurate logf, since phi crosses zero at r = 1, and the hardware square root, 1 ulp: the correctly rounded sqrtf is a dozen
// instructions in a loop of ten and measured 2.0x slower forward and 1.65x backward with the same errors against float64,
// profiles/tps_timing.txt and tps_margins.txt); its product with the coefficient and the running sum are float64 FMAs,
// rounded to fp32 once at the store.  The weights of a rough point set cancel to a fraction of their size, and an fp32 sum loses
// that fraction of its digits (a 3-D set of 257 points under 2 voxels of noise: 4.4e-4 voxel all-fp32, 5.4e-5 mixed).
//   tps_fwd_k   a thread owns TPS_V = 4 voxels along x of one row (or 4 of the M points: the same body, two position
//               sources); the sample's control points pass through LDS in chunks of TPS_T = 256 (normalised position and
//               coefficient row), read back with a wave-uniform index -- a broadcast.  Reading them from global memory
//               with the same uniform index instead (scalar loads, no LDS, no barriers) measured 1.05-1.10x slower in 3-D
//               and 1.58x slower in 2-D (profiles/tps_timing.txt), so the staging stays.
//   tps_bwd_k   the adjoint in gather form: a thread owns one control point, the voxels of its slab pass through LDS in tiles
//               of TPS_T (normalised position and g), the thread adds phi g in double in voxel order.  The volume is cut into
//               a number of slabs fixed by the shape alone; the workgroups of control-point block 0 also add the affine rows
//               (sum g, sum xh g^T) of their slab, per thread over the voxels it stages and then over the workgroup in a fixed
//               order.  Every (slab, row) partial goes to the workspace.
//   tps_red_k   adds the slabs' partials of each row in slab order.
// No atomics anywhere: both directions are bit-identical from run to run.  No gradient with respect to the control positions.
// Nothing syncs with the host, allocates or keeps state.
#include "common.h"

namespace {

constexpr int TPS_T = 256;                   // threads per workgroup = control points per LDS chunk = voxels per LDS tile
constexpr int TPS_V = 4;                     // voxels (points) per thread of the forward
constexpr int TPS_KMAX = 4096;
constexpr int TPS_BLOCKS = 2048;             // the backward cuts the volume into about TPS_BLOCKS / (control blocks * B) slabs

struct TpsGeom {
  int n[3];                                  // extents in the axis order (z,) y, x: ND entries are used
  double sc[3];                              // h_a / L, same order
  int S;                                     // voxels per sample
  int K;
  long long M;                               // points per sample (point mode)
  int nxt;                                   // threads per row (voxel mode)
  long long items;                           // threads with work per sample
};

template <int ND>
__device__ __forceinline__ float tps_phi(float s) {
  if (ND == 3) return -__builtin_amdgcn_sqrtf(s);               // v_sqrt_f32: 1 ulp; s below the normal range gives 0
  return s > 0.f ? 0.5f * s * logf(s) : 0.f;                    // (false for NaN)
}

// ------------------------------------------------------------------------------------------------ forward
template <int ND, bool PTS>
__global__ __launch_bounds__(TPS_T) void tps_fwd_k(const double* __restrict__ coef, const float* __restrict__ ctrl,
                                                   const float* __restrict__ pts, float* __restrict__ out, TpsGeom g) {
  __shared__ double s_w[TPS_T][ND];
  __shared__ float s_q[TPS_T][ND];
  const int b = (int)blockIdx.y;
  const int tid = (int)threadIdx.x;
  const long long t = (long long)blockIdx.x * TPS_T + tid;
  const bool live = t < g.items;
  const long long tt = live ? t : 0;                            // a thread without work computes item 0 and stores nothing
  double xd[TPS_V][ND];
  float xf[TPS_V][ND];
  long long row = 0;
  int xi = 0;
  if (PTS) {
#pragma unroll
    for (int v = 0; v < TPS_V; ++v) {
      long long m = tt * TPS_V + v;
      m = m < g.M ? m : g.M - 1;
#pragma unroll
      for (int a = 0; a < ND; ++a) xd[v][a] = g.sc[a] * (double)pts[((long long)b * g.M + m) * ND + a];
    }
  } else {
    row = tt / g.nxt;
    xi = (int)(tt - row * g.nxt) * TPS_V;
    int c[ND];
    if (ND == 3) { c[0] = (int)(row / g.n[1]); c[1] = (int)(row - (long long)c[0] * g.n[1]); }
    else c[0] = (int)row;
#pragma unroll
    for (int v = 0; v < TPS_V; ++v) {
#pragma unroll
      for (int a = 0; a < ND - 1; ++a) xd[v][a] = g.sc[a] * (double)c[a];
      xd[v][ND - 1] = g.sc[ND - 1] * (double)(xi + v);
    }
  }
#pragma unroll
  for (int v = 0; v < TPS_V; ++v)
#pragma unroll
    for (int a = 0; a < ND; ++a) xf[v][a] = (float)xd[v][a];

  double acc[TPS_V][ND];
#pragma unroll
  for (int v = 0; v < TPS_V; ++v)
#pragma unroll
    for (int a = 0; a < ND; ++a) acc[v][a] = 0.0;
  const double* cb = coef + (long long)b * (g.K + ND + 1) * ND;
  const float* qb = ctrl + (long long)b * g.K * ND;

  for (int k0 = 0; k0 < g.K; k0 += TPS_T) {
    const int n = g.K - k0 < TPS_T ? g.K - k0 : TPS_T;
    if (k0 > 0) __syncthreads();                                // the previous chunk has been read by every thread
    if (tid < n) {
#pragma unroll
      for (int a = 0; a < ND; ++a) {
        s_q[tid][a] = (float)(g.sc[a] * (double)qb[(long long)(k0 + tid) * ND + a]);
        s_w[tid][a] = cb[(long long)(k0 + tid) * ND + a];
      }
    }
    __syncthreads();
    for (int j = 0; j < n; ++j) {                               // j is wave-uniform: every read below is a broadcast
      float q[ND];
      double w[ND];
#pragma unroll
      for (int a = 0; a < ND; ++a) {
        q[a] = s_q[j][a];
        w[a] = s_w[j][a];
      }
#pragma unroll
      for (int v = 0; v < TPS_V; ++v) {
        float s = 0.f;                                          // (voxel mode: the terms of z and y are the same for every v)
#pragma unroll
        for (int a = 0; a < ND; ++a) {
          const float d = xf[v][a] - q[a];
          s = fmaf(d, d, s);
        }
        const double p = (double)tps_phi<ND>(s);
#pragma unroll
        for (int a = 0; a < ND; ++a) acc[v][a] = fma(p, w[a], acc[v][a]);
      }
    }
  }
  if (!live) return;
#pragma unroll
  for (int v = 0; v < TPS_V; ++v) {
    const bool ok = PTS ? tt * TPS_V + v < g.M : xi + v < g.n[ND - 1];
    if (!ok) continue;
#pragma unroll
    for (int a = 0; a < ND; ++a) {
      double lin = cb[(long long)g.K * ND + a];
#pragma unroll
      for (int c = 0; c < ND; ++c) lin = fma(xd[v][c], cb[(long long)(g.K + 1 + c) * ND + a], lin);
      const float u = (float)(acc[v][a] + lin);
      if (PTS) out[((long long)b * g.M + tt * TPS_V + v) * ND + a] = u;
      else out[((long long)b * ND + a) * g.S + row * g.n[ND - 1] + xi + v] = u;
    }
  }
}

// ------------------------------------------------------------------------------------------------ adjoint
template <int ND>
__global__ __launch_bounds__(TPS_T) void tps_bwd_k(const float* __restrict__ ctrl, const float* __restrict__ gout,
                                                   double* __restrict__ part, TpsGeom g, int nslab, int chunk) {
  __shared__ float s_x[TPS_T][ND];
  __shared__ float s_g[TPS_T][ND];
  __shared__ double red[TPS_T / 64];
  const int b = (int)blockIdx.z, slab = (int)blockIdx.y, kb = (int)blockIdx.x;
  const int tid = (int)threadIdx.x;
  const int k = kb * TPS_T + tid;
  const int R = g.K + ND + 1;
  float q[ND];
#pragma unroll
  for (int a = 0; a < ND; ++a) q[a] = k < g.K ? (float)(g.sc[a] * (double)ctrl[((long long)b * g.K + k) * ND + a]) : 0.f;
  double acc[ND], aff[ND + 1][ND];
#pragma unroll
  for (int a = 0; a < ND; ++a) {
    acc[a] = 0.0;
#pragma unroll
    for (int r = 0; r <= ND; ++r) aff[r][a] = 0.0;
  }
  const float* gb = gout + (long long)b * ND * g.S;
  const int v0 = slab * chunk;                                  // (nslab * chunk < S + chunk < 2^31)
  const int v1 = g.S - v0 < chunk ? g.S : v0 + chunk;

  for (int base = v0; base < v1; base += TPS_T) {
    if (base > v0) __syncthreads();                             // the previous tile has been read by every thread
    const bool live = base + tid < v1;
    const int i = live ? base + tid : v1 - 1;
    int c[ND];
    c[ND - 1] = i % g.n[ND - 1];
    const int r = i / g.n[ND - 1];
    if (ND == 3) { c[1] = r % g.n[1]; c[0] = r / g.n[1]; }
    else c[0] = r;
    double xd[ND];
    float gv[ND];
#pragma unroll
    for (int a = 0; a < ND; ++a) {
      xd[a] = g.sc[a] * (double)c[a];
      gv[a] = live ? gb[(long long)a * g.S + i] : 0.f;
      s_x[tid][a] = (float)xd[a];
      s_g[tid][a] = gv[a];
    }
    if (kb == 0) {                                              // the affine rows of this slab (uniform over the workgroup)
#pragma unroll
      for (int a = 0; a < ND; ++a) {
        aff[0][a] += (double)gv[a];
#pragma unroll
        for (int cc = 0; cc < ND; ++cc) aff[1 + cc][a] = fma(xd[cc], (double)gv[a], aff[1 + cc][a]);
      }
    }
    __syncthreads();
    const int n = v1 - base < TPS_T ? v1 - base : TPS_T;
    for (int j = 0; j < n; ++j) {                               // wave-uniform: broadcasts
      float s = 0.f;
#pragma unroll
      for (int a = 0; a < ND; ++a) {
        const float d = s_x[j][a] - q[a];
        s = fmaf(d, d, s);
      }
      const double p = (double)tps_phi<ND>(s);
#pragma unroll
      for (int a = 0; a < ND; ++a) acc[a] = fma(p, (double)s_g[j][a], acc[a]);
    }
  }
  double* pb = part + ((long long)b * nslab + slab) * R * ND;
  if (k < g.K) {
#pragma unroll
    for (int a = 0; a < ND; ++a) pb[(long long)k * ND + a] = acc[a];
  }
  if (kb == 0) {
#pragma unroll
    for (int r = 0; r <= ND; ++r)
#pragma unroll
      for (int a = 0; a < ND; ++a) {
        const double t = block_sum_ordered<TPS_T>(aff[r][a], red);
        if (tid == 0) pb[(long long)(g.K + r) * ND + a] = t;
      }
  }
}

// dcoef[b][row][a] = the nslab partials of that entry, added in slab order; n = R * ND entries per sample
__global__ __launch_bounds__(TPS_T) void tps_red_k(const double* __restrict__ part, double* __restrict__ dcoef, int n,
                                                   int nslab) {
  const int b = (int)blockIdx.y;
  const int i = (int)blockIdx.x * TPS_T + (int)threadIdx.x;
  if (i >= n) return;
  const double* p = part + (long long)b * nslab * n + i;
  double s = 0.0;
  for (int sl = 0; sl < nslab; ++sl) s += p[(long long)sl * n];
  dcoef[(long long)b * n + i] = s;
}

// ------------------------------------------------------------------------------------------------ host side
bool tps_scale_ok(int nd, double sz, double sy, double sx) {
  const double s[3] = {nd == 3 ? sz : 1.0, sy, sx};
  for (double v : s)
    if (!(v > 0.0 && v <= 1.7976931348623157e308)) return false;
  return true;
}

// false for what the entry points refuse: nd outside {2, 3}, B outside [1, 65535], K outside [1, 4096], an extent < 2 (D is not
// read when nd == 2), 2^31 and more flow elements
bool tps_vol_geom(int nd, int B, int K, int D, int H, int W, double sz, double sy, double sx, TpsGeom* g) {
  if ((nd != 2 && nd != 3) || B < 1 || B > 65535 || K < 1 || K > TPS_KMAX || H < 2 || W < 2 || (nd == 3 && D < 2)) return false;
  if (nd == 2) D = 1;
  const long long S = (long long)D * H * W;
  if (S * nd * B >= (1LL << 31)) return false;
  g->S = (int)S;
  g->K = K;
  g->M = 0;
  if (nd == 3) {
    g->n[0] = D; g->n[1] = H; g->n[2] = W;
    g->sc[0] = sz; g->sc[1] = sy; g->sc[2] = sx;
  } else {
    g->n[0] = H; g->n[1] = W; g->n[2] = 1;
    g->sc[0] = sy; g->sc[1] = sx; g->sc[2] = 1.0;
  }
  g->nxt = (W + TPS_V - 1) / TPS_V;
  g->items = (long long)D * H * g->nxt;
  return true;
}

// the slabs of the backward: chunk voxels each (a multiple of TPS_T), a function of the shape alone
void tps_slabs(const TpsGeom& g, int B, int* nslab, int* chunk) {
  const long long kblocks = (g.K + TPS_T - 1) / TPS_T;
  long long want = TPS_BLOCKS / (kblocks * B);
  want = want < 1 ? 1 : want;
  long long ch = (g.S + want - 1) / want;
  ch = (ch + TPS_T - 1) / TPS_T * TPS_T;
  *chunk = (int)ch;
  *nslab = (int)((g.S + ch - 1) / ch);
}

}  // namespace

extern "C" long long dfmir_tps_ws_bytes(int nd, int B, int K, int D, int H, int W) {
  TpsGeom g;
  if (!tps_vol_geom(nd, B, K, D, H, W, 1.0, 1.0, 1.0, &g)) return -1;
  int nslab, chunk;
  tps_slabs(g, B, &nslab, &chunk);
  return (long long)sizeof(double) * B * nslab * (K + nd + 1) * nd;
}

extern "C" int dfmir_tps_fwd(int nd, const double* coef, const float* ctrl, const float* points, float* out, int B, int K,
                             long long M, int D, int H, int W, double sz, double sy, double sx, void* stream) {
  TpsGeom g;
  DF_ARG_CHECK(coef && ctrl && out && tps_scale_ok(nd, sz, sy, sx));
  if (points) {
    DF_ARG_CHECK(M >= 1 && B >= 1 && M * nd * B < (1LL << 31));
    DF_ARG_CHECK(tps_vol_geom(nd, B, K, 2, 2, 2, sz, sy, sx, &g));   // (the extents are not read in point mode)
    g.M = M;
    g.items = (M + TPS_V - 1) / TPS_V;
  } else {
    DF_ARG_CHECK(tps_vol_geom(nd, B, K, D, H, W, sz, sy, sx, &g));
  }
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((g.items + TPS_T - 1) / TPS_T), (unsigned)B);
  if (nd == 3) {
    if (points) tps_fwd_k<3, true><<<grid, TPS_T, 0, st>>>(coef, ctrl, points, out, g);
    else tps_fwd_k<3, false><<<grid, TPS_T, 0, st>>>(coef, ctrl, points, out, g);
  } else {
    if (points) tps_fwd_k<2, true><<<grid, TPS_T, 0, st>>>(coef, ctrl, points, out, g);
    else tps_fwd_k<2, false><<<grid, TPS_T, 0, st>>>(coef, ctrl, points, out, g);
  }
  DF_LAUNCH_CHECK();
  return 0;
}

extern "C" int dfmir_tps_bwd_coef(int nd, const float* ctrl, const float* gout, double* dcoef, void* ws, int B, int K, int D,
                                  int H, int W, double sz, double sy, double sx, void* stream) {
  TpsGeom g;
  DF_ARG_CHECK(ctrl && gout && dcoef && ws && (reinterpret_cast<uintptr_t>(ws) & 7) == 0 && tps_scale_ok(nd, sz, sy, sx));
  DF_ARG_CHECK(tps_vol_geom(nd, B, K, D, H, W, sz, sy, sx, &g));
  int nslab, chunk;
  tps_slabs(g, B, &nslab, &chunk);
  hipStream_t st = (hipStream_t)stream;
  double* part = reinterpret_cast<double*>(ws);
  const dim3 grid((unsigned)((K + TPS_T - 1) / TPS_T), (unsigned)nslab, (unsigned)B);
  if (nd == 3) tps_bwd_k<3><<<grid, TPS_T, 0, st>>>(ctrl, gout, part, g, nslab, chunk);
  else tps_bwd_k<2><<<grid, TPS_T, 0, st>>>(ctrl, gout, part, g, nslab, chunk);
  DF_LAUNCH_CHECK();
  const int n = (K + nd + 1) * nd;
  tps_red_k<<<dim3((unsigned)((n + TPS_T - 1) / TPS_T), (unsigned)B), TPS_T, 0, st>>>(part, dcoef, n, nslab);
  DF_LAUNCH_CHECK();
  return 0;
}
