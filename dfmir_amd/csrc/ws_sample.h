// The cell and corner gather of the warped-feature SSD (warpssd.hip), shared with the affine system kernels (affine.hip):
// the geometry of a feature volume, the cell floor() selects for a sample point with its guards (lin_cell.h's), the
// gather of four channels of its corners from the voxel-major packed copy (or the channel-major tensor), and the
// interpolant with its derivative.  The demons force (demons.hip) takes the same pieces, and shares with warpssd.hip the
// kernel that finishes the per-sample sums (ws_fin_k).  Everything sits in an anonymous namespace: each file that includes
// this keeps its own copy of the host helpers.
#pragma once
#include "lin_cell.h"

namespace {

constexpr int WS_T = 256;                    // threads per workgroup: 4 waves x 64 lanes
constexpr int WS_MAXC = 16;

struct WsGeom {
  int D, H, W;                               // D == 1 for 2-D features
  int S;                                     // voxels per sample
  int nblk;                                  // workgroups per sample
  int C, Cp;                                 // channels, and rounded up to 4
};

// The cell of one voxel is lin_cell.h's, with its guards.
template <int ND>
using WsCell = LinCell<ND>;

template <int ND>
__device__ __forceinline__ void ws_cell(const WsGeom& g, const int (&p)[ND], const float (&u)[ND], WsCell<ND>& q) {
  int n[ND];
  lin_extents<ND>(g.D, g.H, g.W, n);
  lin_cell<ND, int>(p, u, n, q);
}

// Four channels 4 gi .. 4 gi + 3 of the 2^ND corners of a cell (x is bit 0, axis a bit ND - 1 - a); 0 outside the volume
// and for channels >= C.  Every address formed lies inside the sample: a corner outside reads voxel 0 and is discarded.
template <int ND, bool PACKED>
__device__ __forceinline__ void ws_corners(const float* __restrict__ mb, const WsGeom& g, const WsCell<ND>& q, int gi,
                                           float4 (&val)[1 << ND]) {
  constexpr int NC = 1 << ND;
#pragma unroll
  for (int m = 0; m < NC; ++m) {
    const bool in = q.in(m);
    const int o = in ? q.off(m) : 0;
    float4 t;
    if (PACKED) {
      t = *reinterpret_cast<const float4*>(mb + (long long)o * g.Cp + 4 * gi);
    } else {
      const int c0 = 4 * gi;                                    // c0 < C always; the others fall back to channel c0
      const float* r = mb + (long long)c0 * g.S + o;
      t.x = r[0];
      t.y = r[c0 + 1 < g.C ? (long long)g.S : 0];
      t.z = r[c0 + 2 < g.C ? 2LL * g.S : 0];
      t.w = r[c0 + 3 < g.C ? 3LL * g.S : 0];
      if (c0 + 1 >= g.C) t.y = 0.f;
      if (c0 + 2 >= g.C) t.z = 0.f;
      if (c0 + 3 >= g.C) t.w = 0.f;
    }
    val[m] = in ? t : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// One channel: the interpolated value and the derivative of the interpolant along each axis.  The value is lin_value's (x
// innermost, then y, then z), but the derivatives along y and z are differences of the interpolated rows and planes,
// a01 - a00 and b1 - b0, where lin_flow_grad weights differences of corners: x0 (v2 - v0) + x1 (v3 - v1) and
// (x0 v2 + x1 v3) - (x0 v0 + x1 v1) are different fp32 numbers, so the two orders stay apart.
template <int ND>
__device__ __forceinline__ float ws_interp(const float (&v)[1 << ND], const WsCell<ND>& q, float (&d)[ND]) {
  const float x1 = q.w1[ND - 1], x0 = 1.f - x1, y1 = q.w1[ND - 2], y0 = 1.f - y1;
  const float a00 = x0 * v[0] + x1 * v[1], a01 = x0 * v[2] + x1 * v[3];
  const float d00 = v[1] - v[0], d01 = v[3] - v[2];
  if (ND == 2) {
    d[ND - 1] = y0 * d00 + y1 * d01;
    d[ND - 2] = a01 - a00;
    return y0 * a00 + y1 * a01;
  }
  constexpr int U = ND == 3 ? 4 : 0;                            // (keeps the 2-D instantiation inside v)
  const float z1 = q.w1[0], z0 = 1.f - z1;
  const float a10 = x0 * v[U] + x1 * v[U + 1], a11 = x0 * v[U + 2] + x1 * v[U + 3];
  const float d10 = v[U + 1] - v[U], d11 = v[U + 3] - v[U + 2];
  const float b0 = y0 * a00 + y1 * a01, b1 = y0 * a10 + y1 * a11;
  d[ND - 1] = z0 * (y0 * d00 + y1 * d01) + z1 * (y0 * d10 + y1 * d11);
  d[ND - 2] = z0 * (a01 - a00) + z1 * (a11 - a10);
  d[0] = b1 - b0;
  return z0 * b0 + z1 * b1;
}

// false for arguments the entry points refuse: nd outside {2, 3}, B < 1, C outside [1, 16], an extent < 2 (D is not read
// when nd == 2), or 2^31 and more elements in the packed features or the flow
bool ws_geom(int nd, int B, int C, int D, int H, int W, int vpt, WsGeom* g) {
  if ((nd != 2 && nd != 3) || B < 1 || C < 1 || C > WS_MAXC || H < 2 || W < 2 || (nd == 3 && D < 2)) return false;
  if (nd == 2) D = 1;
  const long long S = (long long)D * H * W;
  const int Cp = (C + 3) & ~3;
  if (S * Cp * B >= (1LL << 31) || S * nd * B >= (1LL << 31)) return false;
  g->D = D; g->H = H; g->W = W; g->S = (int)S; g->C = C; g->Cp = Cp;
  g->nblk = (int)((S + (long long)WS_T * vpt - 1) / ((long long)WS_T * vpt));
  return true;
}

inline bool ws_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// (one workgroup of T threads) adds the two slots of each sample's workgroups in a fixed order: per[b] = L_b, loss[0] = L,
// scale[0] (may be NULL) = what a unit gradient is still to be multiplied with: 1, masked 1 / sum m, 0 for an empty mask.
// C = the channel count.  Bit-identical from run to run.  A template, so that only the files that launch it carry it.
template <int T>
static __global__ __launch_bounds__(T) void ws_fin_k(const double* __restrict__ part, int B, int nblk, double C, int masked,
                                                     float* __restrict__ per, float* __restrict__ loss,
                                                     float* __restrict__ scale) {
  __shared__ double red[T / 64];
  double total = 0.0, wtotal = 0.0;
  for (int b = 0; b < B; ++b) {
    double s = 0.0, w = 0.0;
    for (int i = threadIdx.x; i < nblk; i += T) {
      s += part[2 * ((long long)b * nblk + i)];
      w += part[2 * ((long long)b * nblk + i) + 1];
    }
    s = block_sum_ordered<T>(s, red);
    w = block_sum_ordered<T>(w, red);
    if (threadIdx.x == 0) {
      per[b] = w > 0.0 ? (float)(s / (C * w)) : 0.f;
      total += s;
      wtotal += w;
    }
  }
  if (threadIdx.x == 0) {
    loss[0] = wtotal > 0.0 ? (float)(total / (C * wtotal)) : 0.f;
    if (scale) scale[0] = masked ? (wtotal > 0.0 ? (float)(1.0 / wtotal) : 0.f) : 1.f;
  }
}

}  // namespace
