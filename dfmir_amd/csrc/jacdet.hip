// Jacobian determinant of a deformation phi(x) = x + u(x): fold penalty (forward and backward), determinant map and
// per-sample regularity statistics, 2-D and 3-D.  Build-defined (include/dfmir_hip.h and losses.JacobianDet_Loss state the
// definition):
//
//   u [B][nd][(D)][H][W] fp32, nd = 2 or 3; channel a is the displacement in voxels along axis a, in the order (z,) y, x.
//   border m >= 1; Omega_m = the voxels with m <= p_a <= n_a - 1 - m on every axis.  For p in Omega_m
//     J_ab(p) = delta_ab + (u_a(p + e_b) - u_a(p - e_b)) / 2          central differences
//     d(p)    = det J(p)                                              2x2 or 3x3, written out (no pivoting)
//   The determinant does not depend on the voxel spacing (J_phys = H J H^-1, H = diag(h)): nothing here takes one.
//   penalty  psi(d) = max(0, eps - d)^power, power 1 or 2;  loss = sum_{b, p in Omega_m} psi(d(p)) / N,  N = B |Omega_m|
//   gradient W_ab(p) = psi'(d(p)) cof(J(p))_ab on Omega_m and 0 outside (cof = dd/dJ_ab), psi'(d) = -power max(0, eps - d)^(power-1)
//            (power 1: -1 where d < eps, 0 otherwise);   dL/du_a(q) = (1 / 2N) sum_b [ W_ab(q - e_b) - W_ab(q + e_b) ]
//   map      d(p) on Omega_m, exactly 1.0f (the identity's value) outside
//   stats    per sample over Omega_m: count of d <= 0, min d, max d, mean d, mean l, std l (population),
//            l = log(max(d + log_offset, log_floor))
//
// Tiles, z chunks and the staging of a plane of u are those of stencil_tile.h, with zeros outside the volume.  A voxel
// needs all nd channels at once, so a staged plane is nd channel planes.
//   jac_fwd_k<ND3, VEC, MODE>  u with a halo of 1, three open planes.  JAC_PENALTY: psi added in double per thread, one
//                              double slot per workgroup, df_slot_mean_k adds the slots.  JAC_MAP: d or 1.0f stored.
//                              JAC_STATS: count, min, max and three double sums per workgroup; jac_stats_fin_k (one
//                              workgroup per sample) adds a sample's slots in a fixed order.  The sums of l are taken
//                              about a pivot, l at the first voxel of the sample's Omega_m, so that std = sqrt(max(0,
//                              S2/n - (S1/n)^2)) does not cancel on a field whose l is constant.
//   jac_bwd_k<ND3, VEC>        gather form, no atomics, no derivative volume in HBM: u with a halo of 2 (three open planes);
//                              W of the plane is formed over tile + 1 -- the z column of a thread's own voxels stays in its
//                              registers as a rolling window of three planes, the y and x columns go to LDS -- and every
//                              voxel, border or interior, collects its 2 nd terms with the one expression.
// jac_det2 / jac_det3 are the ONE place the determinant and the cofactors are formed, jac_at the one place J is.  Nothing
// syncs with the host (gout is read on the device), allocates or keeps state; every output is bit-identical from run to run.
#include "stencil_tile.h"
#include <math.h>

using namespace stencil;

namespace {

constexpr int JAC_PENALTY = 0, JAC_MAP = 1, JAC_STATS = 2;
constexpr int JAC_SLOT = 7;                  // doubles per workgroup of JAC_STATS: count, min, max, sum d, S1, S2, pivot

struct JacGeom {
  int D, H, W, m;                            // D == 1 in 2-D
  int nzc, nty, ntx;                         // z chunks, tiles along y and x
  int power;
  float eps;
  double off, lfloor;                        // log_offset, log_floor
};

// The determinant d and the cofactors c[a][b] = dd/dJ_ab of one J.
template <bool ND3>
struct JacM {
  float d;
  float c[ND3 ? 3 : 2][ND3 ? 3 : 2];
};
__device__ __forceinline__ JacM<false> jac_det2(const float (&J)[2][2]) {
  JacM<false> r;
  r.c[0][0] = J[1][1]; r.c[0][1] = -J[1][0];
  r.c[1][0] = -J[0][1]; r.c[1][1] = J[0][0];
  r.d = J[0][0] * J[1][1] - J[0][1] * J[1][0];
  return r;
}
__device__ __forceinline__ JacM<true> jac_det3(const float (&J)[3][3]) {
  JacM<true> r;
  r.c[0][0] = J[1][1] * J[2][2] - J[1][2] * J[2][1];
  r.c[0][1] = J[1][2] * J[2][0] - J[1][0] * J[2][2];
  r.c[0][2] = J[1][0] * J[2][1] - J[1][1] * J[2][0];
  r.c[1][0] = J[0][2] * J[2][1] - J[0][1] * J[2][2];
  r.c[1][1] = J[0][0] * J[2][2] - J[0][2] * J[2][0];
  r.c[1][2] = J[0][1] * J[2][0] - J[0][0] * J[2][1];
  r.c[2][0] = J[0][1] * J[1][2] - J[0][2] * J[1][1];
  r.c[2][1] = J[0][2] * J[1][0] - J[0][0] * J[1][2];
  r.c[2][2] = J[0][0] * J[1][1] - J[0][1] * J[1][0];
  r.d = J[0][0] * r.c[0][0] + J[0][1] * r.c[0][1] + J[0][2] * r.c[0][2];
  return r;
}
// J at one voxel, then its determinant and cofactors.  A, B, C point at the voxel in channel 0 of the planes z - 1, z,
// z + 1 (2-D: B alone is read); chs = the channel stride, rs = the row stride.
template <bool ND3>
__device__ __forceinline__ JacM<ND3> jac_at(const float* A, const float* B, const float* C, long long chs, long long rs) {
  constexpr int N = ND3 ? 3 : 2;
  float J[N][N];
#pragma unroll
  for (int a = 0; a < N; ++a) {
    const long long o = a * chs;
    if constexpr (ND3) J[a][0] = 0.5f * (C[o] - A[o]);
    J[a][N - 2] = 0.5f * (B[o + rs] - B[o - rs]);
    J[a][N - 1] = 0.5f * (B[o + 1] - B[o - 1]);
    J[a][a] += 1.f;
  }
  if constexpr (ND3) return jac_det3(J);
  else return jac_det2(J);
}

__device__ __forceinline__ bool jac_in(const JacGeom& g, int n, int p) { return p >= g.m && p <= n - 1 - g.m; }

// Maximum over a workgroup, valid in thread 0 only (the contract of block_sum_ordered).
__device__ __forceinline__ float jac_block_max(float v, float* sm /* NT / 64 */) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = -HUGE_VALF;
  if (threadIdx.x == 0)
    for (int w = 0; w < NT / 64; ++w) t = fmaxf(t, sm[w]);
  return t;
}

// ------------------------------------------------------------------------------------------------ forward
template <bool ND3, bool VEC, int MODE>
__global__ __launch_bounds__(NT) void jac_fwd_k(const float* __restrict__ u, JacGeom g, double* __restrict__ part,
                                                float* __restrict__ detmap) {
  constexpr int NC = ND3 ? 3 : 2;
  using Stage = stencil::Stage<NC, 1, VEC>;
  constexpr int CH = Stage::CH;
  __shared__ __attribute__((aligned(16))) float su[ND3 ? 3 : 1][NC * CH];
  __shared__ double red[NT / 64];
  __shared__ float redf[NT / 64];
  const Tile t = tile_of(g, ZC);
  const long long vol = (long long)g.D * g.H * g.W;
  const float* ub = u + t.plane * NC * vol;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int x = t.x0 + lane;
  const bool xin = jac_in(g, g.W, x);
  const int c0 = (2 * w + 1) * RS + X0 + lane;                     // the thread's first voxel in a staged plane
  Stage st;
  double acc = 0.0, s1 = 0.0, s2 = 0.0, cnt = 0.0, piv = 0.0;   // acc: the sum of psi (penalty) or of d (statistics)
  float mn = HUGE_VALF, mx = -HUGE_VALF;
  if constexpr (MODE == JAC_STATS) {                            // l at the first voxel of the sample's Omega_m
    const long long hw = (long long)g.H * g.W;
    const float* p0 = ub + ((ND3 ? (long long)g.m * g.H : 0LL) + g.m) * g.W + g.m;
    const float d0 = jac_at<ND3>(ND3 ? p0 - hw : p0, p0, ND3 ? p0 + hw : p0, vol, g.W).d;
    piv = log(fmax((double)d0 + g.off, g.lfloor));
  }
  // what a voxel (z, y, x) with determinant d contributes; in = the voxel lies in Omega_m
  auto visit = [&](float d, bool in, int z, int y) {
    if constexpr (MODE == JAC_PENALTY) {
      const float e = g.eps - d;
      const float p = e > 0.f ? (g.power == 2 ? e * e : e) : 0.f;
      acc += (double)(in ? p : 0.f);
    } else if constexpr (MODE == JAC_MAP) {
      if (y < g.H && x < g.W) detmap[t.plane * vol + ((long long)z * g.H + y) * g.W + x] = in ? d : 1.f;
    } else if (in) {
      cnt += d <= 0.f ? 1.0 : 0.0;
      mn = fminf(mn, d);
      mx = fmaxf(mx, d);
      acc += (double)d;
      const double l = log(fmax((double)d + g.off, g.lfloor)) - piv;
      s1 += l;
      s2 += l * l;
    }
  };
  if constexpr (!ND3) {
    st.fetch(ub, g, vol, 0, t.y0, t.x0);
    st.commit(su[0]);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int y = t.y0 + 2 * w + j;
      const float* B = su[0] + c0 + j * RS;
      visit(jac_at<false>(B, B, B, CH, RS).d, xin && jac_in(g, g.H, y), 0, y);
    }
  } else {
    int ia = 0, ib = 1, ic = 2;                                  // slots of the planes z - 1, z, z + 1
    st.fetch(ub, g, vol, t.z0 - 1, t.y0, t.x0);
    st.commit(su[ia]);
    st.fetch(ub, g, vol, t.z0, t.y0, t.x0);
    st.commit(su[ib]);
    st.fetch(ub, g, vol, t.z0 + 1, t.y0, t.x0);
    for (int z = t.z0; z < t.z1; ++z) {
      st.commit(su[ic]);
      __syncthreads();
      if (z + 1 < t.z1) st.fetch(ub, g, vol, z + 2, t.y0, t.x0);   // in flight while this plane is computed
      const bool zin = jac_in(g, g.D, z);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int y = t.y0 + 2 * w + j, c = c0 + j * RS;
        visit(jac_at<true>(su[ia] + c, su[ib] + c, su[ic] + c, CH, RS).d, zin && xin && jac_in(g, g.H, y), z, y);
      }
      __syncthreads();
      const int o = ia; ia = ib; ib = ic; ic = o;
    }
  }
  if constexpr (MODE == JAC_PENALTY) {
    acc = block_sum_ordered<NT>(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
  } else if constexpr (MODE == JAC_STATS) {
    cnt = block_sum_ordered<NT>(cnt, red);
    acc = block_sum_ordered<NT>(acc, red);
    s1 = block_sum_ordered<NT>(s1, red);
    s2 = block_sum_ordered<NT>(s2, red);
    mn = -jac_block_max(-mn, redf);
    mx = jac_block_max(mx, redf);
    if (threadIdx.x == 0) {
      double* p = part + (long long)blockIdx.x * JAC_SLOT;
      p[0] = cnt; p[1] = (double)mn; p[2] = (double)mx; p[3] = acc; p[4] = s1; p[5] = s2; p[6] = piv;
    }
  }
}

// stats[b][0..5] = count of d <= 0, min d, max d, mean d, mean l, std l from the `per` slot sets of sample b, added in a
// fixed order; n = |Omega_m|.  One workgroup per sample.
__global__ __launch_bounds__(NT) void jac_stats_fin_k(const double* __restrict__ part, int per, double n,
                                                      double* __restrict__ stats) {
  __shared__ double red[NT / 64];
  __shared__ float redf[NT / 64];
  const double* p = part + (long long)blockIdx.x * per * JAC_SLOT;
  double cnt = 0.0, sd = 0.0, s1 = 0.0, s2 = 0.0;
  float mn = HUGE_VALF, mx = -HUGE_VALF;
  for (int i = threadIdx.x; i < per; i += NT) {
    const double* q = p + (long long)i * JAC_SLOT;
    cnt += q[0];
    mn = fminf(mn, (float)q[1]);
    mx = fmaxf(mx, (float)q[2]);
    sd += q[3];
    s1 += q[4];
    s2 += q[5];
  }
  cnt = block_sum_ordered<NT>(cnt, red);
  sd = block_sum_ordered<NT>(sd, red);
  s1 = block_sum_ordered<NT>(s1, red);
  s2 = block_sum_ordered<NT>(s2, red);
  mn = -jac_block_max(-mn, redf);
  mx = jac_block_max(mx, redf);
  if (threadIdx.x == 0) {
    double* o = stats + (long long)blockIdx.x * 6;
    const double m1 = s1 / n;
    o[0] = cnt; o[1] = (double)mn; o[2] = (double)mx; o[3] = sd / n;
    o[4] = p[6] + m1;                                   // (every workgroup of the sample holds the same pivot)
    o[5] = sqrt(fmax(0.0, s2 / n - m1 * m1));
  }
}

// ------------------------------------------------------------------------------------------------ backward
// du_a(q) = gout * k * sum_b [ W_ab(q - e_b) - W_ab(q + e_b) ], k = 1 / 2N.  The y and x columns of W of one plane hold
// (TY + 2) x (TX + 2) values (tile + 1; its corners are never read and never written), rows of DC floats.
template <bool ND3, bool VEC>
__global__ __launch_bounds__(NT) void jac_bwd_k(const float* __restrict__ u, const float* __restrict__ gout, float k,
                                                JacGeom g, float* __restrict__ du) {
  constexpr int NC = ND3 ? 3 : 2;
  using Stage = stencil::Stage<NC, 2, VEC>;
  constexpr int CH = Stage::CH, DR = TY + 2, DC = TX + 2, DN = DR * DC, RING = 2 * TX + 2 * TY;
  static_assert(RING <= NT, "one ring voxel per thread");
  __shared__ __attribute__((aligned(16))) float su[ND3 ? 3 : 1][NC * CH];
  __shared__ float sw[2][NC][DN];                                // W_ay and W_ax of the plane
  const Tile t = tile_of(g, ZC);
  const long long vol = (long long)g.D * g.H * g.W;
  const float* ub = u + t.plane * NC * vol;
  float* dp = du + t.plane * NC * vol;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int x = t.x0 + lane;
  const float s = gout[0] * k;
  Stage st;

  // W at the tile-relative voxel (ly, lx) of the plane staged in B (A, C: its neighbours along z), times the Omega_m indicator
  auto weights = [&](const float* A, const float* B, const float* C, int ly, int lx, bool zin) {
    const int c = (ly + 2) * RS + X0 + lx;
    JacM<ND3> r = jac_at<ND3>(A + c, B + c, C + c, CH, RS);
    const float e = g.eps - r.d;
    const bool on = zin && jac_in(g, g.H, t.y0 + ly) && jac_in(g, g.W, t.x0 + lx) && e > 0.f;
    const float f = g.power == 2 ? -2.f * e : -1.f;             // psi'(d) where it is not 0
#pragma unroll
    for (int a = 0; a < NC; ++a)
#pragma unroll
      for (int b = 0; b < NC; ++b) r.c[a][b] = on ? f * r.c[a][b] : 0.f;
    return r;
  };
  auto put = [&](const JacM<ND3>& r, int ly, int lx) {           // the y and x columns to LDS
    const int i = (ly + 1) * DC + lx + 1;
#pragma unroll
    for (int a = 0; a < NC; ++a) {
      sw[0][a][i] = r.c[a][NC - 2];
      sw[1][a][i] = r.c[a][NC - 1];
    }
  };
  // W of one plane: a thread's own two voxels (their z column goes to wz), then one voxel of the ring around the tile
  auto form = [&](const float* A, const float* B, const float* C, bool zin, float (&wz)[2][NC]) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const JacM<ND3> r = weights(A, B, C, 2 * w + j, lane, zin);
#pragma unroll
      for (int a = 0; a < NC; ++a) wz[j][a] = r.c[a][0];
      put(r, 2 * w + j, lane);
    }
    if (tid < RING) {
      int ly, lx;
      if (tid < 2 * TX) { ly = tid < TX ? -1 : TY; lx = tid & (TX - 1); }
      else { const int i = tid - 2 * TX; ly = i < TY ? i : i - TY; lx = i < TY ? -1 : TX; }
      put(weights(A, B, C, ly, lx, zin), ly, lx);
    }
  };
  // the in-plane terms of the thread's voxel j, channel a
  auto gather_plane = [&](int j, int a) {
    const int i = (2 * w + j + 1) * DC + lane + 1;
    return (sw[0][a][i - DC] - sw[0][a][i + DC]) + (sw[1][a][i - 1] - sw[1][a][i + 1]);
  };

  if constexpr (!ND3) {
    float wz[2][NC];
    st.fetch(ub, g, vol, 0, t.y0, t.x0);
    st.commit(su[0]);
    __syncthreads();
    form(su[0], su[0], su[0], true, wz);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int y = t.y0 + 2 * w + j;
#pragma unroll
      for (int a = 0; a < NC; ++a) {
        const float v = gather_plane(j, a);
        if (y < g.H && x < g.W) dp[a * vol + (long long)y * g.W + x] = s * v;
      }
    }
  } else {
    int ua = 0, uq = 1, uc = 2;              // u slots of the planes q - 1, q, q + 1
    float wa[2][NC], wb[2][NC], wc[2][NC];   // the z column of W at the planes q - 2, q - 1, q (own voxels)
    float pin[2][NC];                        // the in-plane terms of the plane q - 1
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int a = 0; a < NC; ++a) wa[j][a] = wb[j][a] = pin[j][a] = 0.f;
    st.fetch(ub, g, vol, t.z0 - 2, t.y0, t.x0);
    st.commit(su[ua]);
    st.fetch(ub, g, vol, t.z0 - 1, t.y0, t.x0);
    st.commit(su[uq]);
    st.fetch(ub, g, vol, t.z0, t.y0, t.x0);
    for (int q = t.z0 - 1; q <= t.z1; ++q) {         // q: the plane whose W is formed; the output plane is z = q - 1
      st.commit(su[uc]);
      __syncthreads();
      if (q < t.z1) st.fetch(ub, g, vol, q + 2, t.y0, t.x0);
      form(su[ua], su[uq], su[uc], jac_in(g, g.D, q), wc);
      __syncthreads();
      if (q - 1 >= t.z0) {
        const int z = q - 1;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int y = t.y0 + 2 * w + j;
#pragma unroll
          for (int a = 0; a < NC; ++a) {
            const float v = (wa[j][a] - wc[j][a]) + pin[j][a];
            if (y < g.H && x < g.W) dp[a * vol + ((long long)z * g.H + y) * g.W + x] = s * v;
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int a = 0; a < NC; ++a) {
          pin[j][a] = gather_plane(j, a);
          wa[j][a] = wb[j][a];
          wb[j][a] = wc[j][a];
        }
      const int o = ua; ua = uq; uq = uc; uc = o;
    }
  }
}

// ------------------------------------------------------------------------------------------------ host side
// false for arguments the entry points refuse: nd outside {2, 3}, B < 1, border < 1, an axis shorter than 2 border + 1 (D is
// not read when nd == 2), or 2^31 and more elements
bool jac_geom(int nd, int B, int D, int H, int W, int m, JacGeom* g, double* omega) {
  if ((nd != 2 && nd != 3) || B < 1 || m < 1) return false;
  if (nd == 2) D = 1;
  const long long need = 2LL * m + 1;
  if ((nd == 3 && D < need) || H < need || W < need) return false;
  if ((long long)B * nd * D * H * W >= (1LL << 31)) return false;
  g->D = D; g->H = H; g->W = W; g->m = m;
  set_tile_counts(g, ZC);
  g->power = 2; g->eps = 0.f; g->off = 0.0; g->lfloor = 1.0;
  *omega = (double)(nd == 3 ? D - 2 * m : 1) * (H - 2 * m) * (W - 2 * m);
  return true;
}
inline bool jac_penalty_ok(float eps, int power) { return (power == 1 || power == 2) && eps >= 0.f && eps <= 3.0e38f; }

template <int MODE>
void jac_launch_fwd(int nd, const float* flow, const JacGeom& g, unsigned nwg, double* part, float* detmap, hipStream_t st) {
  const bool vec = vec_ok(g.W, flow);
  if (nd == 3) {
    if (vec) jac_fwd_k<true, true, MODE><<<nwg, NT, 0, st>>>(flow, g, part, detmap);
    else jac_fwd_k<true, false, MODE><<<nwg, NT, 0, st>>>(flow, g, part, detmap);
  } else {
    if (vec) jac_fwd_k<false, true, MODE><<<nwg, NT, 0, st>>>(flow, g, part, detmap);
    else jac_fwd_k<false, false, MODE><<<nwg, NT, 0, st>>>(flow, g, part, detmap);
  }
}

}  // namespace

extern "C" long long dfmir_jacdet_ws_floats(int nd, int B, int D, int H, int W) {
  JacGeom g;
  double omega;
  if (!jac_geom(nd, B, D, H, W, 1, &g, &omega)) return -1;
  return 2 * JAC_SLOT * B * wg_per_plane(g);
}

extern "C" int dfmir_jacdet_fwd(int nd, const float* flow, float* ws, float* out, int B, int D, int H, int W, int border,
                                float eps, int power, void* stream) {
  JacGeom g;
  double omega;
  DF_ARG_CHECK(flow && ws && out && (reinterpret_cast<uintptr_t>(ws) & 7) == 0 && jac_penalty_ok(eps, power) &&
               jac_geom(nd, B, D, H, W, border, &g, &omega));
  g.eps = eps; g.power = power;
  hipStream_t st = (hipStream_t)stream;
  const unsigned nwg = (unsigned)(B * wg_per_plane(g));
  double* part = reinterpret_cast<double*>(ws);
  jac_launch_fwd<JAC_PENALTY>(nd, flow, g, nwg, part, nullptr, st);
  DF_LAUNCH_CHECK();
  df_slot_mean_k<NT><<<1, NT, 0, st>>>(part, (int)nwg, omega * B, out);    // loss = (the slots, in a fixed order) / N
  DF_LAUNCH_CHECK();
  return 0;
}

extern "C" int dfmir_jacdet_bwd(int nd, const float* flow, const float* gout, float* dflow, int B, int D, int H, int W,
                                int border, float eps, int power, void* stream) {
  JacGeom g;
  double omega;
  DF_ARG_CHECK(flow && gout && dflow && jac_penalty_ok(eps, power) && jac_geom(nd, B, D, H, W, border, &g, &omega));
  g.eps = eps; g.power = power;
  hipStream_t st = (hipStream_t)stream;
  const unsigned nwg = (unsigned)(B * wg_per_plane(g));
  const float k = (float)(0.5 / (omega * B));
  const bool vec = vec_ok(g.W, flow);
  if (nd == 3) {
    if (vec) jac_bwd_k<true, true><<<nwg, NT, 0, st>>>(flow, gout, k, g, dflow);
    else jac_bwd_k<true, false><<<nwg, NT, 0, st>>>(flow, gout, k, g, dflow);
  } else {
    if (vec) jac_bwd_k<false, true><<<nwg, NT, 0, st>>>(flow, gout, k, g, dflow);
    else jac_bwd_k<false, false><<<nwg, NT, 0, st>>>(flow, gout, k, g, dflow);
  }
  DF_LAUNCH_CHECK();
  return 0;
}

extern "C" int dfmir_jacdet_map(int nd, const float* flow, float* detmap, int B, int D, int H, int W, int border,
                                void* stream) {
  JacGeom g;
  double omega;
  DF_ARG_CHECK(flow && detmap && jac_geom(nd, B, D, H, W, border, &g, &omega));
  jac_launch_fwd<JAC_MAP>(nd, flow, g, (unsigned)(B * wg_per_plane(g)), nullptr, detmap, (hipStream_t)stream);
  DF_LAUNCH_CHECK();
  return 0;
}

extern "C" int dfmir_jacdet_stats(int nd, const float* flow, float* ws, double* stats, int B, int D, int H, int W,
                                  int border, double log_offset, double log_floor, void* stream) {
  JacGeom g;
  double omega;
  DF_ARG_CHECK(flow && ws && stats && (reinterpret_cast<uintptr_t>(ws) & 7) == 0 &&
               (reinterpret_cast<uintptr_t>(stats) & 7) == 0 && log_offset >= 0.0 && log_offset <= 1.0e300 &&
               log_floor > 0.0 && log_floor <= 1.0e300 && jac_geom(nd, B, D, H, W, border, &g, &omega));
  g.off = log_offset; g.lfloor = log_floor;
  hipStream_t st = (hipStream_t)stream;
  double* part = reinterpret_cast<double*>(ws);
  jac_launch_fwd<JAC_STATS>(nd, flow, g, (unsigned)(B * wg_per_plane(g)), part, nullptr, st);
  DF_LAUNCH_CHECK();
  jac_stats_fin_k<<<(unsigned)B, NT, 0, st>>>(part, (int)wg_per_plane(g), omega, stats);
  DF_LAUNCH_CHECK();
  return 0;
}
