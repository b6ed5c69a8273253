// The (bi/tri)linear cell of a sample point x + u(x), shared by every kernel that samples a volume there with zero
// padding: the warps (warp.hip, warp_win.hip), the label warp of dice.hip, flow_sample.h (invcons.hip, compose.hip) and
// ws_sample.h (warpssd.hip, affine.hip, demons.hip); landmark.hip takes the corner weight alone.
//   lin_cell        floor(), the upper weights, the per-axis "corner inside" guards, the flat offset of the lower corner
//   lin_gather      the 2^ND corner values of one channel, 0 outside the volume
//   lin_value       the interpolated value        } x innermost, then y, then z: "the warp order"
//   lin_flow_grad   its derivative along each axis }
//   lin_cw          the weight of one corner as a product over the axes, from a seed
//   lin_voxel_fwd / lin_voxel_bwd   one output voxel of the warp and of its adjoint, start to finish
// Axes are (z,) y, x; corner m has bit ND - 1 - a set when it is the upper one along axis a (x is bit 0).  The build keeps
// -ffp-contract=off, so an expression written here rounds as the same expression written in a kernel did.  Everything has
// internal linkage and there is no host state: each file compiles its own copy.
#pragma once
#include "common.h"
#include <math.h>

namespace {

// IDX: the type of offsets into a channel -- int where the entry point has bounded the sample below 2^31 elements, long
// long in the one-voxel-per-thread warp kernels, which take any size.
template <int ND, typename IDX = int>
struct LinCell {
  float w1[ND];                              // weight of the upper corner along each axis
  IDX st[ND];                                // strides of (D,) H, W
  IDX base;                                  // offset of the lower corner (may lie outside: address only corners that are in())
  bool ok[ND][2];                            // per axis: lower, upper corner inside the volume
  __device__ __forceinline__ bool in(int m) const {
    bool r = true;
#pragma unroll
    for (int a = 0; a < ND; ++a) r = r && ok[a][(m >> (ND - 1 - a)) & 1];
    return r;
  }
  __device__ __forceinline__ IDX off(int m) const {
    IDX o = base;
#pragma unroll
    for (int a = 0; a < ND; ++a) o += (IDX)((m >> (ND - 1 - a)) & 1) * st[a];
    return o;
  }
};

template <int ND>
__device__ __forceinline__ void lin_extents(int D, int H, int W, int (&n)[ND]) {      // D is not read when ND == 2
  if (ND == 3) n[0] = D;
  n[ND - 2] = H; n[ND - 1] = W;
}

// The cell of the point p + u in a volume of extents n.
template <int ND, typename IDX>
__device__ __forceinline__ void lin_cell(const int (&p)[ND], const float (&u)[ND], const int (&n)[ND], LinCell<ND, IDX>& q) {
  q.st[ND - 1] = 1;
#pragma unroll
  for (int a = ND - 2; a >= 0; --a) q.st[a] = q.st[a + 1] * (IDX)n[a + 1];
  q.base = 0;
#pragma unroll
  for (int a = 0; a < ND; ++a) {
    const float f = (float)p[a] + u[a];
    const bool nearby = f >= -1.f && f < (float)n[a];             // false for NaN and for points past the padding cells:
    const float fl = floorf(f);                                 // no corner is read then, and no float goes to int
    const int i0 = nearby ? (int)fl : -2;
    q.w1[a] = f - fl;
    q.base += (IDX)i0 * q.st[a];
    q.ok[a][0] = (unsigned)i0 < (unsigned)n[a];
    q.ok[a][1] = (unsigned)(i0 + 1) < (unsigned)n[a];
  }
}

template <int ND, typename IDX>
__device__ __forceinline__ void lin_gather(const float* __restrict__ sc, const LinCell<ND, IDX>& q, float (&v)[1 << ND]) {
#pragma unroll
  for (int m = 0; m < (1 << ND); ++m) v[m] = q.in(m) ? sc[q.off(m)] : 0.f;
}

// The value in the warp order: wz0 (wy0 (wx0 v0 + wx1 v1) + wy1 (wx0 v2 + wx1 v3)) + wz1 (the same of v4 .. v7).
template <int ND>
__device__ __forceinline__ float lin_value(const float (&v)[1 << ND], const float (&w1)[ND]) {
  const float x1 = w1[ND - 1], x0 = 1.f - x1, y1 = w1[ND - 2], y0 = 1.f - y1;
  const float p0 = y0 * (x0 * v[0] + x1 * v[1]) + y1 * (x0 * v[2] + x1 * v[3]);
  if (ND == 2) return p0;
  constexpr int U = ND == 3 ? 4 : 0;                            // (keeps the 2-D instantiation inside v)
  const float p1 = y0 * (x0 * v[U] + x1 * v[U + 1]) + y1 * (x0 * v[U + 2] + x1 * v[U + 3]);
  return (1.f - w1[0]) * p0 + w1[0] * p1;
}

// d(value) / d(position) along each axis in the warp order: differences of CORNERS, weighted.  (ws_interp of ws_sample.h
// takes the y and z derivatives as differences of interpolated ROWS; the two round differently and both stay.)
template <int ND>
__device__ __forceinline__ void lin_flow_grad(const float (&v)[1 << ND], const float (&w1)[ND], float (&d)[ND]) {
  const float x1 = w1[ND - 1], x0 = 1.f - x1, y1 = w1[ND - 2], y0 = 1.f - y1;
  if (ND == 2) {
    d[ND - 2] = x0 * (v[2] - v[0]) + x1 * (v[3] - v[1]);
    d[ND - 1] = y0 * (v[1] - v[0]) + y1 * (v[3] - v[2]);
    return;
  }
  constexpr int U = ND == 3 ? 4 : 0;
  const float z1 = w1[0], z0 = 1.f - z1;
  const float p0 = y0 * (x0 * v[0] + x1 * v[1]) + y1 * (x0 * v[2] + x1 * v[3]);
  const float p1 = y0 * (x0 * v[U] + x1 * v[U + 1]) + y1 * (x0 * v[U + 2] + x1 * v[U + 3]);
  d[0] = p1 - p0;
  d[ND - 2] = z0 * (x0 * (v[2] - v[0]) + x1 * (v[3] - v[1])) + z1 * (x0 * (v[U + 2] - v[U]) + x1 * (v[U + 3] - v[U + 1]));
  d[ND - 1] = z0 * (y0 * (v[1] - v[0]) + y1 * (v[3] - v[2])) + z1 * (y0 * (v[U + 1] - v[U]) + y1 * (v[U + 3] - v[U + 2]));
}

// Weight of corner m: ((seed wz) wy) wx, the axis `skip` left out (-1: none).  seed = g gives the scatter weights of the
// warp adjoints, seed = 1 the plain product (1.f * w is w, exactly).
template <int ND>
__device__ __forceinline__ float lin_cw(const float (&w1)[ND], int m, float seed = 1.f, int skip = -1) {
  float t = seed;
#pragma unroll
  for (int a = 0; a < ND; ++a)
    if (a != skip) t *= ((m >> (ND - 1 - a)) & 1) ? w1[a] : 1.f - w1[a];
  return t;
}

// ---- one output voxel p of the warp, all channels: out_c(p) = src_c(p + flow(p)) (+ src_c(p)).  src_b, flow_b, out_b point
// at the sample; S voxels per channel.
template <int ND, typename IDX>
__device__ __forceinline__ void lin_voxel_cell(const float* __restrict__ flow_b, IDX S, IDX sp, const int (&p)[ND],
                                               const int (&n)[ND], LinCell<ND, IDX>& q) {
  float u[ND];
#pragma unroll
  for (int a = 0; a < ND; ++a) u[a] = flow_b[(IDX)a * S + sp];
  lin_cell<ND, IDX>(p, u, n, q);
}

template <int ND, typename IDX>
__device__ void lin_voxel_fwd(const float* __restrict__ src_b, const float* __restrict__ flow_b, float* __restrict__ out_b,
                              int C, const int (&n)[ND], IDX S, IDX sp, const int (&p)[ND], int add_identity) {
  LinCell<ND, IDX> q;
  lin_voxel_cell<ND, IDX>(flow_b, S, sp, p, n, q);
  for (int c = 0; c < C; ++c) {
    const float* sc = src_b + (long long)c * S;
    float v[1 << ND];
    lin_gather<ND, IDX>(sc, q, v);
    float val = lin_value<ND>(v, q.w1);
    if (add_identity) val += sc[sp];
    out_b[(long long)c * S + sp] = val;
  }
}

// The adjoint at one voxel: d(src) by float atomics (dsrc_b may be null), d(flow) stored, or added into the first ND
// channels of d(src) when flow_into_src (the VecInt step, whose src is its own flow).  Neither routine is forced inline:
// warp_win_slow_k<3> takes 80 registers this way, 86 forced inline and 86 with each corner's atomic issued right after its
// load (profiles/lincell_ab.txt).
template <int ND, typename IDX>
__device__ void lin_voxel_bwd(const float* __restrict__ dout_b, const float* __restrict__ src_b,
                              const float* __restrict__ flow_b, float* __restrict__ dsrc_b, float* __restrict__ dflow_b, int C,
                              const int (&n)[ND], IDX S, IDX sp, const int (&p)[ND], int add_identity, int flow_into_src) {
  LinCell<ND, IDX> q;
  lin_voxel_cell<ND, IDX>(flow_b, S, sp, p, n, q);
  float gf[ND];
#pragma unroll
  for (int a = 0; a < ND; ++a) gf[a] = 0.f;
  for (int c = 0; c < C; ++c) {
    const float g = dout_b[(long long)c * S + sp];
    float* dc = dsrc_b ? dsrc_b + (long long)c * S : nullptr;
    float v[1 << ND], d[ND];
    lin_gather<ND, IDX>(src_b + (long long)c * S, q, v);
    lin_flow_grad<ND>(v, q.w1, d);
#pragma unroll
    for (int a = 0; a < ND; ++a) gf[a] += g * d[a];
    if (dc) {
#pragma unroll
      for (int m = 0; m < (1 << ND); ++m)
        if (q.in(m)) atomicAdd(dc + q.off(m), lin_cw<ND>(q.w1, m, g));
      if (add_identity) atomicAdd(dc + sp, g);
    }
  }
#pragma unroll
  for (int a = 0; a < ND; ++a) {
    if (flow_into_src) atomicAdd(dsrc_b + (IDX)a * S + sp, gf[a]);
    else if (dflow_b) dflow_b[(IDX)a * S + sp] = gf[a];
  }
}

}  // namespace
