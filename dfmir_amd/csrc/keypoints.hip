// Keypoint detection and sparse matching, 2-D and 3-D: the Foerstner structure-tensor response, non-maximum suppression, the
// windowed patch SSD around K points and the sparse coupled argmin.  Build-defined (include/dfmir_hip.h,
// ops.foerstner_response, ops.local_maxima, ops.keypoint_cost and ops.keypoint_argmin state the definitions).
//
//   kp_prod_k    <ND3, VEC>.  The tile and staging of stencil_tile.h (8 x 64 voxels per workgroup, halo 1, a chunk of 16 planes
//                marched along z through three LDS slots, the next plane in flight while one is computed): central differences
//                with the index clamped at the faces -- the staged halo holds zeros outside the volume, and a face voxel takes
//                its own value instead --, each divided by 2 h_a, and all nd (nd + 1) / 2 products g_a g_b of a voxel written by
//                its thread, 256 contiguous bytes per row and plane.  Every voxel of I crosses HBM once (plus the halo).
//   kp_resp_k    one thread per voxel reads the nd (nd + 1) / 2 smoothed planes and forms det(T) / trace(adj(T)) in DOUBLE
//                (the determinant of a near-singular T cancels in fp32), rounded once.  Not fused into the Gaussian's z pass:
//                the filter stays dfmir_gauss_smooth itself, one definition and one kernel for every caller.
//   kp_nms_k     <ND>.  A DIRECT WINDOW, not a separable max: a workgroup stages its tile with a halo of `radius` voxels into LDS
//                once (NaN and cells outside the volume as -inf), then every voxel that passes threshold and mask walks its
//                (2 radius + 1)^nd window in LDS -- its 3^nd nearest neighbours first, then the whole window row-major -- and
//                leaves at the first neighbour that beats it: a larger value, or an equal one of lower linear index.  A separable running max needs two more LDS images of the tile (x, then y) on top
//                of the staged one, which at radius 8 in 3-D leaves a tile of 4 x 4 x 8 voxels under 64 KB, and it still needs
//                the window walk for the tie rule at every voxel that equals its window's maximum; the direct walk needs one
//                image, and all but the few voxels that are maxima of their nearest neighbours leave it after a few reads.  The
//                tile is 4 x 8 x 32 (3-D, radius <= 6: at most 56 KB staged), 4 x 4 x 16 (3-D, radius 7 and 8: 39 and 51 KB) or
//                16 x 64 (2-D: at most 10 KB); lanes run along x, LDS reads are stride 1 over the lanes.  One launch.
//   kp_cost_k    <JPT>.  One workgroup of 256 threads per keypoint (b, k); thread t owns the displacements j = t + 256 i,
//                i < JPT, one DOUBLE accumulator each in registers.  The fixed patch of every channel, C P floats, goes into
//                LDS once.  The moving search region, E^nd floats per channel with E = 2 (radius step + patch) + 1, does not fit
//                LDS in 3-D (37^3 floats at the defaults), so it is MARCHED: for every z plane of the region (2-D: the one
//                plane) and every group of G channels, G planes of E x E floats are staged (zeros outside the volume), and each
//                thread adds, for those of its j whose dz reaches that plane (oz = plane - patch - step (dz + radius) within
//                -patch .. patch), the (2 patch + 1)^2 terms of row oz of the patch.  So every j adds its terms in ONE order --
//                oz, then c, then oy, then ox -- whatever the group size: displacements whose reads all fall outside the
//                volume tie bit for bit.  There is no software pipeline inside a workgroup: staging overlaps arithmetic only
//                across the workgroups of a compute unit, and the registers decide how many there are (hipcc -Rpass-analysis=
//                kernel-resource-usage): kp_cost_k<20>, what the 3-D defaults launch (D = 4913), takes 163 VGPRs = 3 waves per
//                SIMD = 3 workgroups per compute unit (and 49 SGPRs spilled to VGPR lanes), <12> 112 VGPRs = 4, <1, 3, 6> at
//                most 64 = 8.  G is therefore the largest number of planes that keeps patch + planes within 160 KB / that
//                count -- 48, 40 and 20 KB -- so that LDS never lowers the occupancy the registers allow, then evened out
//                over the same number of stages, at least 1: 6 at the defaults (12 channels in 2 stages of 6, 38 KB; the
//                barriers per plane halve against the 4 a 32 KB cap gave, which bought no occupancy).  E <=
//                KEYPOINT_MAX_EXTENT = 96 keeps one plane plus the largest patch (16 channels, patch 3, 3-D) below 64 KB.
//                Fewer accumulators per thread (two workgroups per keypoint) would buy occupancy back at the price of staging
//                every plane twice; not built, not measured.  Precision: the difference fix - mov in fp32 (correctly rounded), its
//                square and the sum in double (v_fma_f64, the square exact), times 1 / (C P) in double, rounded once.  Lanes
//                of a wave own consecutive j, i.e. consecutive dx: their LDS reads are `step` floats apart (2-way bank
//                conflict at step 2, 4-way at step 4); the fixed value is one address for the whole wave (a broadcast).
//                Staged reads per keypoint: C E^nd against C P D gathers unstaged.
//   kp_argmin_k  one wave per keypoint: lane l walks j = l, l + 64, .. upwards with a strict < (its lowest j wins), then a
//                butterfly over the lanes carries (value, j) and prefers the smaller value, at equal values the lower j.  Only
//                finite penalised costs compete; a row without one gives index 0 and a NaN displacement.
// Nothing syncs with the host, allocates or keeps state; no atomics anywhere: every output is bit-identical from run to run.
#include "stencil_tile.h"
#include <math.h>

namespace {

using stencil::NT;
using stencil::RS;
using stencil::Tile;
using stencil::tile_of;
using stencil::TX;
using stencil::TY;
using stencil::X0;
using stencil::ZC;

constexpr long long KP_MAX_ELEMS = 1LL << 31;
constexpr int KP_T = 256;
constexpr int KP_MAX_LDS = 64 * 1024;
// what the cost kernel's channel group is sized for: 160 KB of LDS over the workgroups per compute unit that the registers admit
constexpr int KP_COST_LDS_J20 = 48 * 1024;           // kp_cost_k<20>: 163 VGPRs, 3 waves per SIMD = 3 workgroups
constexpr int KP_COST_LDS_J12 = 40 * 1024;           // kp_cost_k<12>: 112 VGPRs, 4
constexpr int KP_COST_LDS_SMALL = 20 * 1024;         // kp_cost_k<1, 3, 6>: at most 64 VGPRs, 8
constexpr int KP_MAX_JPT = 20;                       // 20 * 256 >= 17^3 and >= 33^2

struct KpGeom {
  int D, H, W, nzc, nty, ntx;
  float dz, dy, dx;                                  // 2 h_a
};

inline bool kp_vol(int nd, int B, int& D, int H, int W, long long chan) {
  if (nd != 2 && nd != 3) return false;
  if (nd == 2) D = 1;
  if (B < 1 || H < 2 || W < 2 || (nd == 3 && D < 2) || chan < 1) return false;
  return (long long)B * chan * D * H * W < KP_MAX_ELEMS;
}

// ------------------------------------------------------------------------------------------------ gradient products
template <bool ND3, bool VEC>
__global__ __launch_bounds__(NT) void kp_prod_k(const float* __restrict__ I, KpGeom g, float* __restrict__ T) {
  constexpr int NP = ND3 ? 6 : 3;
  using Stage = stencil::Stage<1, 1, VEC>;
  constexpr int CH = Stage::CH;
  __shared__ __attribute__((aligned(16))) float su[ND3 ? 3 : 1][CH];
  const Tile t = tile_of(g, ZC);
  const long long vol = (long long)g.D * g.H * g.W;
  const float* ib = I + t.plane * vol;
  float* tb = T + t.plane * NP * vol;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int x = t.x0 + lane;
  const int c0 = (2 * w + 1) * RS + X0 + lane;                     // the thread's first voxel in a staged plane
  Stage st;
  // A, B, C: the staged planes z - 1, z, z + 1 (2-D: B alone is read)
  auto visit = [&](const float* A, const float* B, const float* C, int z, int y, int c) {
    if (y >= g.H || x >= g.W) return;
    const float v = B[c];
    const float xp = x + 1 < g.W ? B[c + 1] : v, xm = x > 0 ? B[c - 1] : v;
    const float yp = y + 1 < g.H ? B[c + RS] : v, ym = y > 0 ? B[c - RS] : v;
    const float gx = (xp - xm) / g.dx, gy = (yp - ym) / g.dy;
    float* o = tb + ((long long)z * g.H + y) * g.W + x;
    if constexpr (ND3) {
      const float zp = z + 1 < g.D ? C[c] : v, zm = z > 0 ? A[c] : v;
      const float gz = (zp - zm) / g.dz;
      o[0] = gz * gz;
      o[vol] = gz * gy;
      o[2 * vol] = gz * gx;
      o += 3 * vol;
    }
    o[0] = gy * gy;
    o[vol] = gy * gx;
    o[2 * vol] = gx * gx;
  };
  if constexpr (!ND3) {
    st.fetch(ib, g, vol, 0, t.y0, t.x0);
    st.commit(su[0]);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 2; ++j) visit(su[0], su[0], su[0], 0, t.y0 + 2 * w + j, c0 + j * RS);
  } else {
    int ia = 0, ib_ = 1, ic = 2;                                 // slots of the planes z - 1, z, z + 1
    st.fetch(ib, g, vol, t.z0 - 1, t.y0, t.x0);
    st.commit(su[ia]);
    st.fetch(ib, g, vol, t.z0, t.y0, t.x0);
    st.commit(su[ib_]);
    st.fetch(ib, g, vol, t.z0 + 1, t.y0, t.x0);
    for (int z = t.z0; z < t.z1; ++z) {
      st.commit(su[ic]);
      __syncthreads();
      if (z + 1 < t.z1) st.fetch(ib, g, vol, z + 2, t.y0, t.x0);   // in flight while this plane is computed
#pragma unroll
      for (int j = 0; j < 2; ++j) visit(su[ia], su[ib_], su[ic], z, t.y0 + 2 * w + j, c0 + j * RS);
      __syncthreads();
      const int o = ia; ia = ib_; ib_ = ic; ic = o;
    }
  }
}

// ------------------------------------------------------------------------------------------------ response
__device__ __forceinline__ float kp_ratio(double det, double tr, bool fin) {
  if (!fin || !(tr > 0.0)) return 0.f;
  const double r = det / tr;
  return (r - r == 0.0) ? (float)r : 0.f;                         // a quotient that is not finite: 0
}

template <bool ND3>
__global__ __launch_bounds__(KP_T) void kp_resp_k(const float* __restrict__ T, float* __restrict__ R, int B, long long S) {
  constexpr int NP = ND3 ? 6 : 3;
  const long long i = (long long)blockIdx.x * KP_T + threadIdx.x;
  if (i >= (long long)B * S) return;
  const long long b = i / S, x = i - b * S;
  const float* p = T + b * NP * S + x;
  double m[NP];
  bool fin = true;
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const float v = p[k * S];
    fin = fin && (v - v == 0.f);
    m[k] = (double)v;
  }
  if constexpr (ND3) {
    // T = [a b c; b d e; c e f] over the axes (z, y, x)
    const double a = m[0], bb = m[1], c = m[2], d = m[3], e = m[4], f = m[5];
    const double A00 = d * f - e * e, A11 = a * f - c * c, A22 = a * d - bb * bb;
    const double det = a * A00 - bb * (bb * f - c * e) + c * (bb * e - c * d);
    R[i] = kp_ratio(det, (A00 + A11) + A22, fin);
  } else {
    const double a = m[0], bb = m[1], c = m[2];
    R[i] = kp_ratio(a * c - bb * bb, a + c, fin);
  }
}

// ------------------------------------------------------------------------------------------------ non-maximum suppression
struct NmsGeom {
  int D, H, W, r, tz, ty, tx, ntz, nty, ntx;
  float thr;
};

template <int ND>
__global__ __launch_bounds__(KP_T) void kp_nms_k(const float* __restrict__ R, const float* __restrict__ mask,
                                                 float* __restrict__ out, NmsGeom g) {
  extern __shared__ float sm[];                                  // [EZ][EY][EX]
  const int r = g.r;
  const int EZ = ND == 3 ? g.tz + 2 * r : 1, EY = g.ty + 2 * r, EX = g.tx + 2 * r;
  unsigned bid = blockIdx.x;
  const int x0 = (int)(bid % (unsigned)g.ntx) * g.tx; bid /= (unsigned)g.ntx;
  const int y0 = (int)(bid % (unsigned)g.nty) * g.ty; bid /= (unsigned)g.nty;
  const int z0 = (int)(bid % (unsigned)g.ntz) * g.tz;
  const long long b = bid / (unsigned)g.ntz;
  const long long vol = (long long)g.D * g.H * g.W;
  const float* rb = R + b * vol;
  const float ninf = -HUGE_VALF;
  for (int i = threadIdx.x; i < EZ * EY * EX; i += KP_T) {
    const int lx = i % EX, ly = (i / EX) % EY, lz = i / (EX * EY);
    const int gx = x0 - r + lx, gy = y0 - r + ly, gz = ND == 3 ? z0 - r + lz : 0;
    float v = ninf;
    if (gx >= 0 && gx < g.W && gy >= 0 && gy < g.H && gz >= 0 && gz < g.D) {
      v = rb[((long long)gz * g.H + gy) * g.W + gx];
      if (v != v) v = ninf;
    }
    sm[i] = v;
  }
  __syncthreads();
  const int rz = ND == 3 ? r : 0;
  for (int i = threadIdx.x; i < g.tz * g.ty * g.tx; i += KP_T) {
    const int lx = i % g.tx, ly = (i / g.tx) % g.ty, lz = i / (g.tx * g.ty);
    const int gx = x0 + lx, gy = y0 + ly, gz = z0 + lz;
    if (gx >= g.W || gy >= g.H || gz >= g.D) continue;
    const long long gi = ((long long)gz * g.H + gy) * g.W + gx;
    const int c = ((lz + rz) * EY + ly + r) * EX + lx + r;
    const float v = sm[c];
    bool sel = v > g.thr && (!mask || mask[b * vol + gi] != 0.f);
    // the 3^nd nearest neighbours first, by the same rule: in a smooth map nearly every voxel that is no maximum leaves here
    for (int dz = (rz ? -1 : 0); sel && dz <= (rz ? 1 : 0); ++dz)
      for (int dy = -1; sel && dy <= 1; ++dy) {
        const float* row = sm + c + (dz * EY + dy) * EX;
        const bool rb4 = dz < 0 || (dz == 0 && dy < 0);
        const bool same = dz == 0 && dy == 0;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          const float o = row[dx];
          if (o > v || (o == v && (rb4 || (same && dx < 0)))) sel = false;
        }
      }
    for (int dz = -rz; sel && dz <= rz; ++dz)
      for (int dy = -r; sel && dy <= r; ++dy) {
        const float* row = sm + c + (dz * EY + dy) * EX;
        const bool rb4 = dz < 0 || (dz == 0 && dy < 0);          // the whole row lies before the voxel
        const bool same = dz == 0 && dy == 0;
        for (int dx = -r; dx <= r; ++dx) {
          const float o = row[dx];
          if (o > v || (o == v && (rb4 || (same && dx < 0)))) {
            sel = false;
            break;
          }
        }
      }
    out[b * vol + gi] = sel ? v : 0.f;
  }
}

// ------------------------------------------------------------------------------------------------ windowed patch SSD
struct KcGeom {
  int nd, C, D, H, W;
  int r, rz, step, p, pz;                            // rz, pz: the radius and the patch half width along z (0 in 2-D)
  int n, nz, Dn;                                     // 2 r + 1, 2 rz + 1, the displacements nz n n
  int E, EZ, PW, PZ, G;                              // staged extent in-plane and along z, patch width, channels per stage
  double inv;                                        // 1 / (C P)
};

template <int JPT>
__global__ __launch_bounds__(KP_T) void kp_cost_k(const float* __restrict__ fix, const float* __restrict__ mov,
                                                  const float* __restrict__ pts, float* __restrict__ cost, KcGeom g) {
  extern __shared__ float sm[];                                  // the fixed patch [C][PZ][PW][PW], then G planes [E][E]
  const int tid = threadIdx.x;
  const long long smp = blockIdx.y;                              // grid = (K, B)
  const long long bk = smp * gridDim.x + blockIdx.x;             // the row of pts and cost
  float* out = cost + bk * g.Dn;
  const float* pt = pts + bk * g.nd;
  const float fz = g.nd == 3 ? pt[0] : 0.f, fy = pt[g.nd - 2], fx = pt[g.nd - 1];
  const float qzf = rintf(fz), qyf = rintf(fy), qxf = rintf(fx);  // ties to even
  const bool ok = (fz - fz == 0.f) && (fy - fy == 0.f) && (fx - fx == 0.f) && qzf >= 0.f && qzf <= (float)(g.D - 1) &&
                  qyf >= 0.f && qyf <= (float)(g.H - 1) && qxf >= 0.f && qxf <= (float)(g.W - 1);
  if (!ok) {                                                     // the same for every thread of the workgroup
    const float nan = __uint_as_float(0x7fc00000u);
    for (int j = tid; j < g.Dn; j += KP_T) out[j] = nan;
    return;
  }
  const int qz = (int)qzf, qy = (int)qyf, qx = (int)qxf;
  const int PW2 = g.PW * g.PW, E2 = g.E * g.E;
  const int nfix = g.C * g.PZ * PW2;
  float* sf = sm;
  float* sp = sm + nfix;
  const long long hw = (long long)g.H * g.W, vol = hw * g.D;
  const float* fb = fix + smp * g.C * vol;
  const float* mb = mov + smp * g.C * vol;
  for (int i = tid; i < nfix; i += KP_T) {
    const int ox = i % g.PW, oy = (i / g.PW) % g.PW, oz = (i / PW2) % g.PZ, c = i / (PW2 * g.PZ);
    const int gx = qx + ox - g.p, gy = qy + oy - g.p, gz = qz + oz - g.pz;
    float v = 0.f;
    if (gx >= 0 && gx < g.W && gy >= 0 && gy < g.H && gz >= 0 && gz < g.D) v = fb[c * vol + gz * hw + (long long)gy * g.W + gx];
    sf[i] = v;
  }
  // the thread's displacements: (ez << 16) | the in-plane offset of the window's first read
  int meta[JPT];
  double acc[JPT];
#pragma unroll
  for (int i = 0; i < JPT; ++i) {
    const int j = tid + KP_T * i;
    const int ex = j % g.n, ey = (j / g.n) % g.n, ez = j / (g.n * g.n);
    meta[i] = (ez << 16) | (g.step * ey * g.E + g.step * ex);
    acc[i] = 0.0;
  }
  const int R0 = g.r * g.step + g.p, R0z = g.rz * g.step + g.pz;
  for (int mz = 0; mz < g.EZ; ++mz) {
    // does any dz reach this plane?  step ez in [mz - 2 pz, mz] for an ez in [0, nz)
    const int lo = mz - 2 * g.pz;
    const int e0 = lo <= 0 ? 0 : (lo + g.step - 1) / g.step;
    if (e0 >= g.nz || e0 * g.step > mz) continue;
    const int gz = qz - R0z + mz;
    const bool zin = gz >= 0 && gz < g.D;
    for (int c0 = 0; c0 < g.C; c0 += g.G) {
      const int gc = g.C - c0 < g.G ? g.C - c0 : g.G;
      __syncthreads();                                           // the planes of the last stage are read no more
      for (int i = tid; i < gc * E2; i += KP_T) {
        const int c = i / E2, rem = i - c * E2;
        const int yy = rem / g.E, xx = rem - yy * g.E;
        const int gy = qy - R0 + yy, gx = qx - R0 + xx;
        float v = 0.f;
        if (zin && gx >= 0 && gx < g.W && gy >= 0 && gy < g.H) v = mb[(c0 + c) * vol + gz * hw + (long long)gy * g.W + gx];
        sp[i] = v;
      }
      __syncthreads();
#pragma unroll
      for (int i = 0; i < JPT; ++i) {
        if (tid + KP_T * i >= g.Dn) continue;
        const int oz = mz - g.step * (meta[i] >> 16);            // the patch row along z that this plane is for dz_i
        if (oz < 0 || oz >= g.PZ) continue;
        const float* m0 = sp + (meta[i] & 0xffff);
        const float* f0 = sf + (c0 * g.PZ + oz) * PW2;
        double a = acc[i];
        for (int c = 0; c < gc; ++c) {
          const float* mrow = m0 + c * E2;
          const float* frow = f0 + c * g.PZ * PW2;
          for (int oy = 0; oy < g.PW; ++oy, mrow += g.E, frow += g.PW)
            for (int ox = 0; ox < g.PW; ++ox) {
              const double d = (double)(frow[ox] - mrow[ox]);
              a = fma(d, d, a);
            }
        }
        acc[i] = a;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < JPT; ++i) {
    const int j = tid + KP_T * i;
    if (j < g.Dn) out[j] = (float)(acc[i] * g.inv);
  }
}

// ------------------------------------------------------------------------------------------------ sparse coupled argmin
template <int ND>
__global__ __launch_bounds__(KP_T) void kp_argmin_k(const float* __restrict__ cost, const float* __restrict__ prior,
                                                    float coeff, int* __restrict__ idx, float* __restrict__ disp,
                                                    long long rows, int r, int step) {
  const long long row = (long long)blockIdx.x * (KP_T / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;                                       // a whole wave leaves: no barrier follows
  const int lane = threadIdx.x & 63;
  const int n = 2 * r + 1;
  const int Dn = ND == 3 ? n * n * n : n * n;
  float pr[ND];
#pragma unroll
  for (int a = 0; a < ND; ++a) pr[a] = prior ? prior[row * ND + a] : 0.f;
  const float* c = cost + row * Dn;
  const float inf = HUGE_VALF;
  float best = inf;
  int bj = 0x7fffffff;
  for (int j = lane; j < Dn; j += 64) {
    float w = c[j];
    if (prior) {
      const int ex = j % n, ey = (j / n) % n;
      const float qx = (float)(step * (ex - r)) - pr[ND - 1], qy = (float)(step * (ey - r)) - pr[ND - 2];
      float q = qy * qy;
      if (ND == 3) {
        const float qz = (float)(step * (j / (n * n) - r)) - pr[0];
        q = qz * qz + q;
      }
      q = q + qx * qx;
      w = w + coeff * q;
    }
    if (w < best && w > -inf) {                                  // finite values only; a NaN compares false
      best = w;
      bj = j;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oj = __shfl_xor(bj, o, 64);
    if (ov < best || (ov == best && oj < bj)) {
      best = ov;
      bj = oj;
    }
  }
  if (lane == 0) {
    const bool found = bj != 0x7fffffff;
    const int j = found ? bj : 0;
    idx[row] = j;
    const float nan = __uint_as_float(0x7fc00000u);
    float* d = disp + row * ND;
    if (ND == 3) d[0] = found ? (float)(step * (j / (n * n) - r)) : nan;
    d[ND - 2] = found ? (float)(step * ((j / n) % n - r)) : nan;
    d[ND - 1] = found ? (float)(step * (j % n - r)) : nan;
  }
}

inline int kp_cost_max_radius(int nd) { return nd == 3 ? DFMIR_KEYPOINT_MAX_RADIUS_3D : DFMIR_KEYPOINT_MAX_RADIUS_2D; }

}  // namespace

extern "C" int dfmir_keypoint_products(int nd, const float* I, float* T, int B, int D, int H, int W, float hz, float hy,
                                       float hx, void* stream) {
  DF_ARG_CHECK(I && T && I != T);
  DF_ARG_CHECK(kp_vol(nd, B, D, H, W, nd == 3 ? 6 : 3));
  if (nd == 2) hz = 1.f;
  DF_ARG_CHECK(hz > 0.f && hy > 0.f && hx > 0.f && hz < HUGE_VALF && hy < HUGE_VALF && hx < HUGE_VALF);
  KpGeom g;
  g.D = D; g.H = H; g.W = W;
  g.dz = 2.f * hz; g.dy = 2.f * hy; g.dx = 2.f * hx;
  DF_ARG_CHECK(g.dz < HUGE_VALF && g.dy < HUGE_VALF && g.dx < HUGE_VALF);
  stencil::set_tile_counts(&g, ZC);
  const long long nwg = (long long)B * stencil::wg_per_plane(g);
  DF_ARG_CHECK(nwg < KP_MAX_ELEMS);
  hipStream_t st = (hipStream_t)stream;
  const bool vec = stencil::vec_ok(W, I);
  if (nd == 3) {
    if (vec) kp_prod_k<true, true><<<(unsigned)nwg, NT, 0, st>>>(I, g, T);
    else kp_prod_k<true, false><<<(unsigned)nwg, NT, 0, st>>>(I, g, T);
  } else {
    if (vec) kp_prod_k<false, true><<<(unsigned)nwg, NT, 0, st>>>(I, g, T);
    else kp_prod_k<false, false><<<(unsigned)nwg, NT, 0, st>>>(I, g, T);
  }
  DF_LAUNCH_CHECK();
  return 0;
}

extern "C" int dfmir_keypoint_response(int nd, const float* T, float* R, int B, int D, int H, int W, void* stream) {
  DF_ARG_CHECK(T && R && T != R);
  DF_ARG_CHECK(kp_vol(nd, B, D, H, W, nd == 3 ? 6 : 3));
  const long long S = (long long)D * H * W, n = (long long)B * S;
  const unsigned grid = (unsigned)((n + KP_T - 1) / KP_T);
  hipStream_t st = (hipStream_t)stream;
  if (nd == 3) kp_resp_k<true><<<grid, KP_T, 0, st>>>(T, R, B, S);
  else kp_resp_k<false><<<grid, KP_T, 0, st>>>(T, R, B, S);
  DF_LAUNCH_CHECK();
  return 0;
}

extern "C" int dfmir_keypoint_nms(int nd, const float* R, const float* mask, float* out, int B, int D, int H, int W,
                                  int radius, float threshold, void* stream) {
  DF_ARG_CHECK(R && out && R != out && mask != out);
  DF_ARG_CHECK(kp_vol(nd, B, D, H, W, 1));
  DF_ARG_CHECK(radius >= 1 && radius <= DFMIR_KEYPOINT_NMS_MAX_RADIUS);
  DF_ARG_CHECK(threshold - threshold == 0.f);                     // finite
  NmsGeom g;
  g.D = D; g.H = H; g.W = W; g.r = radius; g.thr = threshold;
  if (nd == 3) {
    if (radius <= 6) { g.tz = 4; g.ty = 8; g.tx = 32; }
    else { g.tz = 4; g.ty = 4; g.tx = 16; }
  } else {
    g.tz = 1; g.ty = 16; g.tx = 64;
  }
  g.ntz = (D + g.tz - 1) / g.tz; g.nty = (H + g.ty - 1) / g.ty; g.ntx = (W + g.tx - 1) / g.tx;
  const long long nwg = (long long)B * g.ntz * g.nty * g.ntx;
  DF_ARG_CHECK(nwg < KP_MAX_ELEMS);
  const size_t lds = (size_t)(nd == 3 ? g.tz + 2 * radius : 1) * (g.ty + 2 * radius) * (g.tx + 2 * radius) * sizeof(float);
  DF_ARG_CHECK(lds <= (size_t)KP_MAX_LDS);
  hipStream_t st = (hipStream_t)stream;
  if (nd == 3) kp_nms_k<3><<<(unsigned)nwg, KP_T, lds, st>>>(R, mask, out, g);
  else kp_nms_k<2><<<(unsigned)nwg, KP_T, lds, st>>>(R, mask, out, g);
  DF_LAUNCH_CHECK();
  return 0;
}

extern "C" int dfmir_keypoint_cost(int nd, const float* fix, const float* mov, const float* pts, float* cost, int B, int C,
                                   int K, int D, int H, int W, int radius, int step, int patch, void* stream) {
  DF_ARG_CHECK(fix && mov && pts && cost && C >= 1 && C <= 16 && K >= 1);
  DF_ARG_CHECK(kp_vol(nd, B, D, H, W, C));
  DF_ARG_CHECK(radius >= 1 && radius <= kp_cost_max_radius(nd) && step >= 1 && step <= DFMIR_KEYPOINT_MAX_STEP &&
               patch >= 0 && patch <= DFMIR_KEYPOINT_MAX_PATCH);
  KcGeom g;
  g.nd = nd; g.C = C; g.D = D; g.H = H; g.W = W;
  g.r = radius; g.rz = nd == 3 ? radius : 0; g.step = step; g.p = patch; g.pz = nd == 3 ? patch : 0;
  g.n = 2 * radius + 1; g.nz = 2 * g.rz + 1; g.Dn = g.nz * g.n * g.n;
  g.E = 2 * (radius * step + patch) + 1; g.EZ = 2 * (g.rz * step + g.pz) + 1;
  g.PW = 2 * patch + 1; g.PZ = 2 * g.pz + 1;
  DF_ARG_CHECK(g.E <= DFMIR_KEYPOINT_MAX_EXTENT && g.Dn <= KP_MAX_JPT * KP_T);
  DF_ARG_CHECK((long long)B * K * g.Dn < KP_MAX_ELEMS && (long long)B * K < KP_MAX_ELEMS && B <= 65535);
  const long long fixb = (long long)C * g.PZ * g.PW * g.PW * 4, planeb = (long long)g.E * g.E * 4;
  const int need = (g.Dn + KP_T - 1) / KP_T;                     // displacements per thread
  // the LDS a workgroup may take without lowering the occupancy its registers allow (the file header has the figures)
  const long long budget = need > 12 ? KP_COST_LDS_J20 : need > 6 ? KP_COST_LDS_J12 : KP_COST_LDS_SMALL;
  long long G = (budget - fixb) / planeb;
  if (G < 1) G = 1;
  if (G > C) G = C;
  const long long ngroups = (C + G - 1) / G;
  G = (C + ngroups - 1) / ngroups;                               // the same number of stages, the groups as equal as they get
  g.G = (int)G;
  const size_t lds = (size_t)(fixb + G * planeb);
  DF_ARG_CHECK(lds <= (size_t)KP_MAX_LDS);
  g.inv = 1.0 / ((double)C * g.PZ * g.PW * g.PW);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)K, (unsigned)B);
#define KP_COST_LAUNCH(J) kp_cost_k<J><<<grid, KP_T, lds, st>>>(fix, mov, pts, cost, g)
  if (need <= 1) KP_COST_LAUNCH(1);
  else if (need <= 3) KP_COST_LAUNCH(3);
  else if (need <= 6) KP_COST_LAUNCH(6);
  else if (need <= 12) KP_COST_LAUNCH(12);
  else KP_COST_LAUNCH(KP_MAX_JPT);
#undef KP_COST_LAUNCH
  DF_LAUNCH_CHECK();
  return 0;
}

extern "C" int dfmir_keypoint_argmin(int nd, const float* cost, const float* prior, float coeff, int* idx, float* disp,
                                     long long rows, int radius, int step, void* stream) {
  DF_ARG_CHECK(cost && idx && disp && (nd == 2 || nd == 3) && rows >= 1);
  DF_ARG_CHECK(radius >= 1 && radius <= kp_cost_max_radius(nd) && step >= 1 && step <= DFMIR_KEYPOINT_MAX_STEP);
  DF_ARG_CHECK(coeff >= 0.f && coeff <= 3.0e38f);                // refuses a NaN too
  const long long n = 2 * radius + 1, Dn = nd == 3 ? n * n * n : n * n;
  DF_ARG_CHECK(rows * Dn < KP_MAX_ELEMS);
  const unsigned grid = (unsigned)((rows + KP_T / 64 - 1) / (KP_T / 64));
  hipStream_t st = (hipStream_t)stream;
  if (nd == 3) kp_argmin_k<3><<<grid, KP_T, 0, st>>>(cost, prior, coeff, idx, disp, rows, radius, step);
  else kp_argmin_k<2><<<grid, KP_T, 0, st>>>(cost, prior, coeff, idx, disp, rows, radius, step);
  DF_LAUNCH_CHECK();
  return 0;
}
