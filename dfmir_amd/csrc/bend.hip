// Bending energy of a flow field (the second-order regulariser), forward and backward, 2-D and 3-D.  Build-defined
// (include/dfmir_hip.h and losses.BendingEnergy_Loss state the definition):
//
//   u [B][C][D][H][W] fp32, axes a in the order (z,) y, x with spacing h_a; a field with D == 1 is 2-D (y and x only).
//   Omega = the voxels whose whole 3^nd neighbourhood lies in the volume (1 <= p_a <= n_a - 2 on every axis).  For p in Omega
//     u_aa(p) = (u(p+e_a) - 2 u(p) + u(p-e_a)) / h_a^2
//     u_ab(p) = (u(p+e_a+e_b) - u(p+e_a-e_b) - u(p-e_a+e_b) + u(p-e_a-e_b)) / (4 h_a h_b),   a < b
//     e(p)    = sum_a u_aa(p)^2 + 2 sum_{a<b} u_ab(p)^2
//   loss = sum_{b,c,p in Omega} e / N,   N = B C |Omega|
//   dL/du(p) = (2 / N) [ sum_a (U_aa(p-e_a) - 2 U_aa(p) + U_aa(p+e_a)) / h_a^2
//                      + 2 sum_{a<b} (U_ab(p-e_a-e_b) - U_ab(p-e_a+e_b) - U_ab(p+e_a-e_b) + U_ab(p+e_a+e_b)) / (4 h_a h_b) ]
//   with U = the derivative value extended by 0 outside Omega (the exact adjoint).
//
// Tiles, z chunks and the staging of a plane of u are those of stencil_tile.h, one (b, c) plane per workgroup and zeros
// outside the volume.
//   bend_fwd_k<ND3, VEC>  u with a halo of 1, three open planes; e per voxel (0 outside Omega) added in double per thread,
//                         one double slot per workgroup.  df_slot_mean_k (one workgroup) adds the slots in a fixed order.
//   bend_bwd_k<ND3, VEC>  gather form, no atomics, no derivative volume in HBM: u with a halo of 2 (three open planes); the
//                         derivative values of tile + 1, times the Omega indicator, are formed in LDS -- u_zz, u_zy, u_zx
//                         as a rolling window of three planes, u_yy, u_xx, u_yx of the output plane alone -- and every
//                         voxel, border or interior, collects its adjoint stencil from them with the one expression.
// bend_dz / bend_dp are the ONE place the second differences are formed, for both directions.  Nothing syncs with the
// host (gout is read on the device), allocates or keeps state; loss and gradient are bit-identical from run to run.
#include "stencil_tile.h"

using namespace stencil;

namespace {

struct BendGeom {
  int D, H, W;                               // D == 1: a 2-D field
  int nzc, nty, ntx;                         // z chunks, tiles along y and x
  float czz, cyy, cxx, czy, czx, cyx;        // 1 / h_a^2 and 1 / (4 h_a h_b)
};

// The second differences at one voxel.  A, B, C point at the voxel in the staged planes z - 1, z, z + 1 (rows of RS).
struct BendDz { float zz, zy, zx; };
struct BendDp { float yy, xx, yx; };
__device__ __forceinline__ BendDz bend_dz(const float* A, const float* B, const float* C, const BendGeom& g) {
  BendDz d;
  d.zz = (C[0] - 2.f * B[0] + A[0]) * g.czz;
  d.zy = (C[RS] - C[-RS] - A[RS] + A[-RS]) * g.czy;
  d.zx = (C[1] - C[-1] - A[1] + A[-1]) * g.czx;
  return d;
}
__device__ __forceinline__ BendDp bend_dp(const float* B, const BendGeom& g) {
  BendDp d;
  d.yy = (B[RS] - 2.f * B[0] + B[-RS]) * g.cyy;
  d.xx = (B[1] - 2.f * B[0] + B[-1]) * g.cxx;
  d.yx = (B[RS + 1] - B[RS - 1] - B[-RS + 1] + B[-RS - 1]) * g.cyx;
  return d;
}

// ------------------------------------------------------------------------------------------------ forward
template <bool ND3, bool VEC>
__global__ __launch_bounds__(NT) void bend_fwd_k(const float* __restrict__ u, BendGeom g, double* __restrict__ part) {
  constexpr int ROWS = TY + 2;
  __shared__ __attribute__((aligned(16))) float su[ND3 ? 3 : 1][ROWS * RS];
  __shared__ double red[NT / 64];
  const Tile t = tile_of(g, ZC);
  const float* up = u + t.plane * ((long long)g.D * g.H * g.W);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int x = t.x0 + lane;
  const bool xin = x >= 1 && x <= g.W - 2;
  const int c0 = (2 * w + 1) * RS + X0 + lane;                     // the thread's first voxel in a staged plane
  Stage<1, 1, VEC> st;
  double acc = 0.0;
  if constexpr (!ND3) {
    st.fetch(up, g, 0, 0, t.y0, t.x0);
    st.commit(su[0]);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int y = t.y0 + 2 * w + j;
      const BendDp p = bend_dp(su[0] + c0 + j * RS, g);
      const float e = p.yy * p.yy + p.xx * p.xx + 2.f * (p.yx * p.yx);
      acc += (double)((xin && y >= 1 && y <= g.H - 2) ? e : 0.f);
    }
  } else {
    int ia = 0, ib = 1, ic = 2;                                  // slots of the planes z - 1, z, z + 1
    st.fetch(up, g, 0, t.z0 - 1, t.y0, t.x0);
    st.commit(su[ia]);
    st.fetch(up, g, 0, t.z0, t.y0, t.x0);
    st.commit(su[ib]);
    st.fetch(up, g, 0, t.z0 + 1, t.y0, t.x0);
    for (int z = t.z0; z < t.z1; ++z) {
      st.commit(su[ic]);
      __syncthreads();
      if (z + 1 < t.z1) st.fetch(up, g, 0, z + 2, t.y0, t.x0);     // in flight while this plane is computed
      const bool zin = z >= 1 && z <= g.D - 2;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int y = t.y0 + 2 * w + j, c = c0 + j * RS;
        const BendDz q = bend_dz(su[ia] + c, su[ib] + c, su[ic] + c, g);
        const BendDp p = bend_dp(su[ib] + c, g);
        const float e = q.zz * q.zz + p.yy * p.yy + p.xx * p.xx + 2.f * (q.zy * q.zy + q.zx * q.zx + p.yx * p.yx);
        acc += (double)((zin && xin && y >= 1 && y <= g.H - 2) ? e : 0.f);
      }
      __syncthreads();
      const int o = ia; ia = ib; ib = ic; ic = o;
    }
  }
  acc = block_sum_ordered<NT>(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// ------------------------------------------------------------------------------------------------ backward
// du = gout * k * [ sum_a c_aa (U_aa(-) - 2 U_aa + U_aa(+)) + 2 sum_{a<b} c_ab (U_ab(--) - U_ab(-+) - U_ab(+-) + U_ab(++)) ],
// k = 2 / N.  The derivative planes hold (TY + 2) x (TX + 2) values (tile + 1), rows of DC floats.
template <bool ND3, bool VEC>
__global__ __launch_bounds__(NT) void bend_bwd_k(const float* __restrict__ u, const float* __restrict__ gout, float k,
                                                 BendGeom g, float* __restrict__ du) {
  constexpr int UR = TY + 4, DR = TY + 2, DC = TX + 2, DN = DR * DC;
  __shared__ __attribute__((aligned(16))) float su[ND3 ? 3 : 1][UR * RS];
  __shared__ float sz[ND3 ? 3 : 1][ND3 ? 3 : 1][ND3 ? DN : 1];   // u_zz, u_zy, u_zx of three planes (3-D)
  __shared__ float sp[3][DN];                                    // u_yy, u_xx, u_yx of the output plane
  const Tile t = tile_of(g, ZC);
  const long long vol = (long long)g.D * g.H * g.W;
  const float* up = u + t.plane * vol;
  float* dp = du + t.plane * vol;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int x = t.x0 + lane;
  const float s = gout[0] * k;
  Stage<1, 2, VEC> st;

  // u_yy, u_xx, u_yx of plane z (staged in `pl`) over tile + 1, times the Omega indicator
  auto in_plane = [&](const float* pl, bool zin) {
    for (int i = tid; i < DN; i += NT) {
      const int ly = i / DC, lx = i - ly * DC, gy = t.y0 - 1 + ly, gx = t.x0 - 1 + lx;
      const bool in = zin && gy >= 1 && gy <= g.H - 2 && gx >= 1 && gx <= g.W - 2;
      const BendDp p = bend_dp(pl + (ly + 1) * RS + X0 - 1 + lx, g);
      sp[0][i] = in ? p.yy : 0.f;
      sp[1][i] = in ? p.xx : 0.f;
      sp[2][i] = in ? p.yx : 0.f;
    }
  };
  // the in-plane part of the adjoint stencil at derivative-plane index i
  auto gather_plane = [&](int i, float& dir, float& cross) {
    dir = g.cyy * (sp[0][i - DC] - 2.f * sp[0][i] + sp[0][i + DC]) + g.cxx * (sp[1][i - 1] - 2.f * sp[1][i] + sp[1][i + 1]);
    cross = g.cyx * (sp[2][i - DC - 1] - sp[2][i - DC + 1] - sp[2][i + DC - 1] + sp[2][i + DC + 1]);
  };

  if constexpr (!ND3) {
    st.fetch(up, g, 0, 0, t.y0, t.x0);
    st.commit(su[0]);
    __syncthreads();
    in_plane(su[0], true);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int ly = 2 * w + j, y = t.y0 + ly;
      float dir, cross;
      gather_plane((ly + 1) * DC + lane + 1, dir, cross);
      if (y < g.H && x < g.W) dp[(long long)y * g.W + x] = s * (dir + 2.f * cross);
    }
  } else {
    int ua = 0, ub = 1, uc = 2;              // u slots of the planes q - 1, q, q + 1
    int da = 0, db = 1, dc = 2;              // derivative slots of the planes q - 2, q - 1, q
    st.fetch(up, g, 0, t.z0 - 2, t.y0, t.x0);
    st.commit(su[ua]);
    st.fetch(up, g, 0, t.z0 - 1, t.y0, t.x0);
    st.commit(su[ub]);
    st.fetch(up, g, 0, t.z0, t.y0, t.x0);
    for (int q = t.z0 - 1; q <= t.z1; ++q) {         // q: the derivative plane formed; the output plane is z = q - 1
      st.commit(su[uc]);
      __syncthreads();
      if (q < t.z1) st.fetch(up, g, 0, q + 2, t.y0, t.x0);
      const bool emit = q - 1 >= t.z0;
      const bool qin = q >= 1 && q <= g.D - 2;
      for (int i = tid; i < DN; i += NT) {
        const int ly = i / DC, lx = i - ly * DC, gy = t.y0 - 1 + ly, gx = t.x0 - 1 + lx;
        const bool in = qin && gy >= 1 && gy <= g.H - 2 && gx >= 1 && gx <= g.W - 2;
        const int c = (ly + 1) * RS + X0 - 1 + lx;
        const BendDz d = bend_dz(su[ua] + c, su[ub] + c, su[uc] + c, g);
        sz[dc][0][i] = in ? d.zz : 0.f;
        sz[dc][1][i] = in ? d.zy : 0.f;
        sz[dc][2][i] = in ? d.zx : 0.f;
      }
      if (emit) in_plane(su[ua], q - 1 >= 1 && q - 1 <= g.D - 2);
      __syncthreads();
      if (emit) {
        const int z = q - 1;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int ly = 2 * w + j, y = t.y0 + ly, i = (ly + 1) * DC + lane + 1;
          float dir, cross;
          gather_plane(i, dir, cross);
          dir += g.czz * (sz[da][0][i] - 2.f * sz[db][0][i] + sz[dc][0][i]);
          cross += g.czy * (sz[da][1][i - DC] - sz[da][1][i + DC] - sz[dc][1][i - DC] + sz[dc][1][i + DC]) +
                   g.czx * (sz[da][2][i - 1] - sz[da][2][i + 1] - sz[dc][2][i - 1] + sz[dc][2][i + 1]);
          if (y < g.H && x < g.W) dp[((long long)z * g.H + y) * g.W + x] = s * (dir + 2.f * cross);
        }
      }
      int o = ua; ua = ub; ub = uc; uc = o;
      o = da; da = db; db = dc; dc = o;
    }
  }
}

// ------------------------------------------------------------------------------------------------ host side
bool bend_finite_pos(float h) { return h > 0.f && h <= 3.0e38f; }      // (false for NaN)

// false for arguments the entry points refuse: an extent < 3 on an axis that counts (D == 1 is the 2-D field and hz is
// then not read), a spacing that is not positive and finite, or 2^31 and more elements
bool bend_geom(int B, int C, int D, int H, int W, float hz, float hy, float hx, BendGeom* g, long long* planes,
               double* count) {
  if (B < 1 || C < 1 || D < 1 || H < 3 || W < 3 || D == 2) return false;
  if ((D > 1 && !bend_finite_pos(hz)) || !bend_finite_pos(hy) || !bend_finite_pos(hx)) return false;
  if ((long long)B * C * D * H * W >= (1LL << 31)) return false;
  g->D = D; g->H = H; g->W = W;
  set_tile_counts(g, ZC);
  const double z = D > 1 ? hz : 1.0, y = hy, x = hx;
  g->czz = (float)(1.0 / (z * z)); g->cyy = (float)(1.0 / (y * y)); g->cxx = (float)(1.0 / (x * x));
  g->czy = (float)(1.0 / (4.0 * z * y)); g->czx = (float)(1.0 / (4.0 * z * x)); g->cyx = (float)(1.0 / (4.0 * y * x));
  *planes = (long long)B * C;
  *count = (double)*planes * (D > 1 ? D - 2 : 1) * (H - 2) * (W - 2);
  return true;
}

}  // namespace

extern "C" long long dfmir_bend_ws_floats(int B, int C, int D, int H, int W) {
  BendGeom g;
  long long planes;
  double count;
  if (!bend_geom(B, C, D, H, W, 1.f, 1.f, 1.f, &g, &planes, &count)) return -1;
  return 2 * planes * wg_per_plane(g);
}

extern "C" int dfmir_bend_fwd(const float* flow, float* ws, float* out, int B, int C, int D, int H, int W, float hz,
                              float hy, float hx, void* stream) {
  BendGeom g;
  long long planes;
  double count;
  DF_ARG_CHECK(flow && ws && out && (reinterpret_cast<uintptr_t>(ws) & 7) == 0 &&
               bend_geom(B, C, D, H, W, hz, hy, hx, &g, &planes, &count));
  hipStream_t st = (hipStream_t)stream;
  const unsigned nwg = (unsigned)(planes * wg_per_plane(g));      // < 2^31
  double* part = reinterpret_cast<double*>(ws);
  const bool vec = vec_ok(g.W, flow);
  if (D > 1) {
    if (vec) bend_fwd_k<true, true><<<nwg, NT, 0, st>>>(flow, g, part);
    else bend_fwd_k<true, false><<<nwg, NT, 0, st>>>(flow, g, part);
  } else {
    if (vec) bend_fwd_k<false, true><<<nwg, NT, 0, st>>>(flow, g, part);
    else bend_fwd_k<false, false><<<nwg, NT, 0, st>>>(flow, g, part);
  }
  DF_LAUNCH_CHECK();
  df_slot_mean_k<NT><<<1, NT, 0, st>>>(part, (int)nwg, count, out);      // loss = (the slots, in a fixed order) / N
  DF_LAUNCH_CHECK();
  return 0;
}

extern "C" int dfmir_bend_bwd(const float* flow, const float* gout, float* dflow, int B, int C, int D, int H, int W,
                              float hz, float hy, float hx, void* stream) {
  BendGeom g;
  long long planes;
  double count;
  DF_ARG_CHECK(flow && gout && dflow && bend_geom(B, C, D, H, W, hz, hy, hx, &g, &planes, &count));
  hipStream_t st = (hipStream_t)stream;
  const unsigned nwg = (unsigned)(planes * wg_per_plane(g));      // < 2^31
  const float k = (float)(2.0 / count);
  const bool vec = vec_ok(g.W, flow);
  if (D > 1) {
    if (vec) bend_bwd_k<true, true><<<nwg, NT, 0, st>>>(flow, gout, k, g, dflow);
    else bend_bwd_k<true, false><<<nwg, NT, 0, st>>>(flow, gout, k, g, dflow);
  } else {
    if (vec) bend_bwd_k<false, true><<<nwg, NT, 0, st>>>(flow, gout, k, g, dflow);
    else bend_bwd_k<false, false><<<nwg, NT, 0, st>>>(flow, gout, k, g, dflow);
  }
  DF_LAUNCH_CHECK();
  return 0;
}
