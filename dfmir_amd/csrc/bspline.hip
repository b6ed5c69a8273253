// Cubic B-spline free-form deformation (Rueckert et al. 1999), 2-D and 3-D: the expansion of a control grid to a dense field
// and its adjoint.  Build-defined (include/dfmir_hip.h and ops.bspline_flow state the definition).  Per axis a: integer
// spacing s_a in 1 .. 8, extent n_a, m_a = (n_a - 1) / s_a + 4 control points, point j at voxel s_a (j - 1); with
// q_a = x_a / s_a and r_a = x_a % s_a
//
//   y[p,x]     = sum over l in {0..3}^ND of prod_a B_{l_a}(r_a / s_a) ctrl[p,q + l]
//   dctrl[p,j] = sum over the x with q_a(x) in {j_a - 3 .. j_a} of prod_a B_{j_a - q_a}(r_a / s_a) dy[p,x]
//
// x and s are integers, so the weights of an axis are a table of s_a x 4 numbers: the host evaluates it in double, rounds it
// to float and hands it over by value (BsTab); nothing but multiply-adds happens per voxel.
//
//   bs_fwd_k   <ND, VEC>.  A workgroup of 256 threads owns a 32 x 32 in-plane tile of one plane (b,c) and, in 3-D, one CELL
//              of z: the s_z slices that share q_z and so the same four control planes.  It stages the control points the
//              tile touches (4 planes in 3-D, rows cy0 .. and columns cx0 .., zeros past the grid) in LDS, contracts them
//              along y into R[lz][y][column] (4 LDS reads per entry, shared by every voxel of the row that meets the column),
//              then every thread contracts along x for its four consecutive voxels into 4 x 4 registers (2-D: the result)
//              and walks the cell's slices with four multiply-adds per voxel and slice: nothing is staged or contracted
//              again inside the cell.  VEC: one 16-byte store per thread and slice (W % 4 == 0, aligned pointer), a wave
//              writes eight 128-byte row segments; otherwise four bounded scalar stores.  The sums start from +0 and the
//              weights are >= 0: a zero control grid gives +0.0 everywhere.
//              Index arithmetic: the thread layouts (16 x 16 staging, 32 x 8 contracting, 32 x 8 x 4 storing) leave one
//              integer division per thread and phase; a flat index taken apart per element cost more than the stores.
//   bs_bwd_x_k the adjoint along x.  A workgroup loads min(8, 8192 / padded W) whole rows of dy, a wave per row, coalesced,
//              into LDS (index x + x / 32: the gather below reads with stride s_x, which the padding spreads over the
//              banks); each lane of the row's wave then gathers the <= 4 s_x voxels of one control column in ascending x.
//              Reads dy once, writes planes * D * H * m_x.
//   bs_bwd_axis_k  the adjoint along y, then z, on the shrunken intermediate: blockIdx.x is the outer index, one thread per
//              (control index, inner index) of it, the <= 4 s inputs in ascending order, coalesced along the inner extent.
// Gather form throughout, no atomics, every sum in a fixed order: bit-identical from run to run.  Nothing here syncs with
// the host, allocates or keeps state.
#include "common.h"

namespace {

constexpr int BS_T = 256;
constexpr int BS_TX = 32, BS_XT = BS_TX / 4, BS_TY = BS_T / BS_XT;   // the forward tile; a thread owns 4 consecutive x: 8 x 32 threads
constexpr int BS_MAX_STRIDE = 8;
constexpr int BS_BWD_ROW_FLOATS = 8192;              // LDS floats of the rows a bs_bwd_x_k workgroup stages
constexpr long long BS_MAX_ELEMS = 1LL << 31;

struct BsTab {
  float w[3][4 * BS_MAX_STRIDE];                     // [z, y, x][r * 4 + l] = B_l(r / s)
};

struct BsGeom {
  int nd, planes;
  int n[3], m[3], s[3];                              // z, y, x; 2-D: n[0] = m[0] = s[0] = 1
  long long vol, grid;                               // voxels and control points of a plane
};

inline void bs_weights(int s, float* w) {
  for (int r = 0; r < BS_MAX_STRIDE; ++r) {
    const double t = r < s ? (double)r / s : 0.0;
    const double b[4] = {(1 - t) * (1 - t) * (1 - t) / 6, (3 * t * t * t - 6 * t * t + 4) / 6,
                         (-3 * t * t * t + 3 * t * t + 3 * t + 1) / 6, t * t * t / 6};
    for (int l = 0; l < 4; ++l) w[r * 4 + l] = r < s ? (float)b[l] : 0.f;
  }
}

// false where the library refuses the call
inline bool bs_geom(int nd, int planes, int D, int H, int W, int sz, int sy, int sx, BsGeom* g, BsTab* tab) {
  if (nd != 2 && nd != 3) return false;
  if (nd == 2) D = 1, sz = 1;
  const int n[3] = {D, H, W}, s[3] = {sz, sy, sx};
  g->nd = nd;
  g->planes = planes;
  g->vol = g->grid = 1;
  if (planes < 1 || planes > 65535) return false;    // grid.z of the forward
  for (int a = 0; a < 3; ++a) {
    if (n[a] < 1 || s[a] < 1 || s[a] > BS_MAX_STRIDE) return false;
    g->n[a] = n[a];
    g->s[a] = s[a];
    g->m[a] = (nd == 2 && a == 0) ? 1 : (n[a] - 1) / s[a] + 4;
    g->vol *= n[a];
    g->grid *= g->m[a];
    if (g->vol >= BS_MAX_ELEMS || g->grid >= BS_MAX_ELEMS) return false;
    bs_weights(s[a], tab->w[a]);
  }
  return planes * g->vol < BS_MAX_ELEMS && planes * g->grid < BS_MAX_ELEMS;
}

// ------------------------------------------------------------------------------------------------ forward
template <int ND, bool VEC>
__global__ __launch_bounds__(BS_T) void bs_fwd_k(const float* __restrict__ ctrl, float* __restrict__ y, BsGeom g, BsTab tab,
                                                 int ntx, int ncy, int ncx) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  constexpr int NZ = ND == 3 ? 4 : 1;
  float* sw = sm;                                    // [3][32] the weight tables
  float* sc = sm + 96;                               // [NZ][ncy][ncx] control points
  float* sr = sc + NZ * ncy * ncx;                   // [NZ][BS_TY][ncx] contracted along y
  const int t = threadIdx.x;
  const int D = g.n[0], H = g.n[1], W = g.n[2], My = g.m[1], Mx = g.m[2], sz = g.s[0], sy = g.s[1], sx = g.s[2];
  const int x0 = (int)(blockIdx.x % ntx) * BS_TX, y0 = (int)(blockIdx.x / ntx) * BS_TY;
  const int qz = blockIdx.y, plane = blockIdx.z;
  const int cx0 = x0 / sx, cy0 = y0 / sy;

  if (t < 96) sw[t] = tab.w[t >> 5][t & 31];
  const float* cp = ctrl + (long long)plane * g.grid;
  // 16 x 16 threads over (row, column) of the staged grid, then 32 x 8 over (y, column): no division per element
  for (int lz = 0; lz < NZ; ++lz) {
    const int jz = ND == 3 ? qz + lz : 0;                                   // <= (D - 1) / sz + 3 = m_z - 1
    for (int r = t >> 4; r < ncy; r += 16)
      for (int c = t & 15; c < ncx; c += 16) {
        const int jx = cx0 + c, jy = cy0 + r;
        sc[(lz * ncy + r) * ncx + c] = (jx < Mx && jy < My) ? cp[((long long)jz * My + jy) * Mx + jx] : 0.f;
      }
  }
  __syncthreads();
  {
    const int yy = t / BS_XT;
    const int yv = y0 + yy < H ? y0 + yy : H - 1;                           // rows past the volume: computed, never read
    const int qy = yv / sy;
    const float* wy = sw + 32 + (yv - qy * sy) * 4;
    const float w0 = wy[0], w1 = wy[1], w2 = wy[2], w3 = wy[3];
    for (int lz = 0; lz < NZ; ++lz)
      for (int c = t % BS_XT; c < ncx; c += BS_XT) {
        const float* p = sc + (lz * ncy + (qy - cy0)) * ncx + c;
        float a = w0 * p[0];
        a = fmaf(w1, p[ncx], a);
        a = fmaf(w2, p[2 * ncx], a);
        a = fmaf(w3, p[3 * ncx], a);
        sr[(lz * BS_TY + yy) * ncx + c] = a;
      }
  }
  __syncthreads();

  const int tx = t % BS_XT, ty = t / BS_XT;
  const int x = x0 + 4 * tx, yv = y0 + ty;
  if (x >= W || yv >= H) return;
  float P[NZ][4];
  int q = x / sx, r = x - q * sx;                                           // of voxel x + i, stepped without dividing again
  q -= cx0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float* wx = sw + 64 + r * 4;
#pragma unroll
    for (int lz = 0; lz < NZ; ++lz) {
      const float* p = sr + (lz * BS_TY + ty) * ncx + q;
      float a = wx[0] * p[0];
      a = fmaf(wx[1], p[1], a);
      a = fmaf(wx[2], p[2], a);
      a = fmaf(wx[3], p[3], a);
      P[lz][i] = a;
    }
    if (x + i + 1 < W) {                                                    // voxels past the volume repeat the last one
      const bool wrap = ++r == sx;
      r = wrap ? 0 : r;
      q += wrap ? 1 : 0;
    }
  }
  const int nz = ND == 3 ? sz : 1;
  for (int rz = 0; rz < nz; ++rz) {
    const int z = ND == 3 ? qz * sz + rz : 0;
    if (z >= D) break;
    float o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (ND == 3) {
        const float* wz = sw + rz * 4;
        float a = wz[0] * P[0][i];
        a = fmaf(wz[1], P[1 % NZ][i], a);
        a = fmaf(wz[2], P[2 % NZ][i], a);
        a = fmaf(wz[3], P[3 % NZ][i], a);
        o[i] = a;
      } else {
        o[i] = P[0][i];
      }
    }
    float* dst = y + (((long long)plane * D + z) * H + yv) * W + x;
    if (VEC) {
      *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (x + i < W) dst[i] = o[i];
    }
  }
}

// ------------------------------------------------------------------------------------------------ backward
__device__ __forceinline__ int bs_pad(int x) { return x + (x >> 5); }

// t1[row][j] = sum over x of B_{j - q(x)}(r(x) / s) dy[row][x]; rows = planes * D * H
__global__ __launch_bounds__(BS_T) void bs_bwd_x_k(const float* __restrict__ dy, float* __restrict__ t1, long long rows, int W,
                                                   int Mx, int sx, int br, BsTab tab) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* sw = sm;                                    // [32] the x table
  float* sd = sm + 32;                               // [br][bs_pad(W - 1) + 1]
  const int t = threadIdx.x;
  const int wp = bs_pad(W - 1) + 1;
  const long long r0 = (long long)blockIdx.x * br;
  const int nr = rows - r0 < br ? (int)(rows - r0) : br;
  if (t < 32) sw[t] = tab.w[2][t];
  const int lane = t & 63, wave = t >> 6;            // a wave per row: no division per element
  for (int row = wave; row < nr; row += BS_T / 64) {
    const float* src = dy + (r0 + row) * W;
    for (int x = lane; x < W; x += 64) sd[row * wp + bs_pad(x)] = src[x];
  }
  __syncthreads();
  const int qmax = (W - 1) / sx;
  for (int row = wave; row < nr; row += BS_T / 64) {
    const float* p = sd + row * wp;
    float* dst = t1 + (r0 + row) * Mx;
    for (int j = lane; j < Mx; j += 64) {
      const int qa = j - 3 > 0 ? j - 3 : 0, qb = j < qmax ? j : qmax;
      float a = 0.f;
      for (int q = qa; q <= qb; ++q) {
        const int l = j - q;
        for (int r = 0; r < sx; ++r) {
          const int x = q * sx + r;
          if (x < W) a = fmaf(sw[r * 4 + l], p[bs_pad(x)], a);
        }
      }
      dst[j] = a;
    }
  }
}

// in [outer][n][inner] -> out [outer][m][inner], the adjoint along the middle axis (table `axis` of tab)
__global__ __launch_bounds__(BS_T) void bs_bwd_axis_k(const float* __restrict__ in, float* __restrict__ out, int n, int m,
                                                      int inner, int s, int axis, BsTab tab) {
  __shared__ float sw[32];
  if (threadIdx.x < 32) sw[threadIdx.x] = tab.w[axis][threadIdx.x];
  __syncthreads();
  const unsigned k = blockIdx.y * BS_T + threadIdx.x;                        // (j, ii) of plane blockIdx.x; m * inner < 2^31
  if (k >= (unsigned)m * inner) return;
  const int j = (int)(k / (unsigned)inner), ii = (int)(k - (unsigned)j * inner);
  const int qmax = (n - 1) / s;
  const float* p = in + (long long)blockIdx.x * n * inner + ii;
  const int qa = j - 3 > 0 ? j - 3 : 0, qb = j < qmax ? j : qmax;
  float a = 0.f;
  for (int q = qa; q <= qb; ++q) {
    const int l = j - q;
    for (int r = 0; r < s; ++r) {
      const int x = q * s + r;
      if (x < n) a = fmaf(sw[r * 4 + l], p[(long long)x * inner], a);
    }
  }
  out[(long long)blockIdx.x * m * inner + k] = a;
}

inline long long bs_round4(long long v) { return (v + 3) / 4 * 4; }

// floats of the intermediates: after x (planes D H m_x) and, in 3-D, after y (planes D m_y m_x)
inline void bs_ws(const BsGeom& g, long long* n1, long long* n2) {
  *n1 = bs_round4((long long)g.planes * g.n[0] * g.n[1] * g.m[2]);
  *n2 = g.nd == 3 ? bs_round4((long long)g.planes * g.n[0] * g.m[1] * g.m[2]) : 0;
}

// rows a bs_bwd_x_k workgroup stages; 0 = the backward refuses the shape: a row does not fit its LDS budget, or a plane's
// control grid is more than grid.y of bs_bwd_axis_k can cover
inline int bs_bwd_rows(const BsGeom& g) {
  if ((g.grid + BS_T - 1) / BS_T > 65535) return 0;
  const int wp = g.n[2] - 1 + ((g.n[2] - 1) >> 5) + 1;
  const int br = BS_BWD_ROW_FLOATS / wp;
  return br > 8 ? 8 : br;
}

}  // namespace

extern "C" int dfmir_bspline_fwd(int nd, const float* ctrl, float* y, int planes, int D, int H, int W, int sz, int sy, int sx,
                                 void* stream) {
  BsGeom g;
  BsTab tab;
  DF_ARG_CHECK(ctrl && y && bs_geom(nd, planes, D, H, W, sz, sy, sx, &g, &tab));
  const int ntx = (g.n[2] + BS_TX - 1) / BS_TX, nty = (g.n[1] + BS_TY - 1) / BS_TY;
  const int ncx = (BS_TX + g.s[2] - 2) / g.s[2] + 4, ncy = (BS_TY + g.s[1] - 2) / g.s[1] + 4;   // cells a tile can meet + 3
  const int ncell = (g.n[0] - 1) / g.s[0] + 1;
  DF_ARG_CHECK(ncell <= 65535);
  const int nz = nd == 3 ? 4 : 1;
  const size_t lds = sizeof(float) * (96 + (size_t)nz * ncy * ncx + (size_t)nz * BS_TY * ncx);
  const dim3 grid((unsigned)(ntx * nty), (unsigned)ncell, (unsigned)planes);
  const bool vec = g.n[2] % 4 == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0;
  hipStream_t st = (hipStream_t)stream;
  if (nd == 3) {
    if (vec) bs_fwd_k<3, true><<<grid, BS_T, lds, st>>>(ctrl, y, g, tab, ntx, ncy, ncx);
    else bs_fwd_k<3, false><<<grid, BS_T, lds, st>>>(ctrl, y, g, tab, ntx, ncy, ncx);
  } else {
    if (vec) bs_fwd_k<2, true><<<grid, BS_T, lds, st>>>(ctrl, y, g, tab, ntx, ncy, ncx);
    else bs_fwd_k<2, false><<<grid, BS_T, lds, st>>>(ctrl, y, g, tab, ntx, ncy, ncx);
  }
  DF_LAUNCH_CHECK();
  return 0;
}

extern "C" long long dfmir_bspline_bwd_ws_floats(int nd, int planes, int D, int H, int W, int sz, int sy, int sx) {
  BsGeom g;
  BsTab tab;
  if (!bs_geom(nd, planes, D, H, W, sz, sy, sx, &g, &tab) || bs_bwd_rows(g) < 1) return -1;
  long long n1, n2;
  bs_ws(g, &n1, &n2);
  return n1 + n2;
}

extern "C" int dfmir_bspline_bwd(int nd, const float* dy, float* dctrl, int planes, int D, int H, int W, int sz, int sy,
                                 int sx, float* ws, void* stream) {
  BsGeom g;
  BsTab tab;
  DF_ARG_CHECK(dy && dctrl && ws && bs_geom(nd, planes, D, H, W, sz, sy, sx, &g, &tab));
  const int br = bs_bwd_rows(g);
  DF_ARG_CHECK(br >= 1);
  long long n1, n2;
  bs_ws(g, &n1, &n2);
  float* t1 = ws;
  float* t2 = ws + n1;
  hipStream_t st = (hipStream_t)stream;
  const long long rows = (long long)planes * g.n[0] * g.n[1];
  const int wp = g.n[2] - 1 + ((g.n[2] - 1) >> 5) + 1;
  bs_bwd_x_k<<<(unsigned)((rows + br - 1) / br), BS_T, sizeof(float) * (32 + (size_t)br * wp), st>>>(dy, t1, rows, g.n[2], g.m[2],
                                                                                                  g.s[2], br, tab);
  DF_LAUNCH_CHECK();
  // along y: [planes D][H][m_x] -> [planes D][m_y][m_x]
  const dim3 gy((unsigned)(planes * g.n[0]), (unsigned)(((long long)g.m[1] * g.m[2] + BS_T - 1) / BS_T));
  bs_bwd_axis_k<<<gy, BS_T, 0, st>>>(t1, nd == 3 ? t2 : dctrl, g.n[1], g.m[1], g.m[2], g.s[1], 1, tab);
  DF_LAUNCH_CHECK();
  if (nd == 3) {                                     // along z: [planes][D][m_y m_x] -> [planes][m_z][m_y m_x]
    const dim3 gz((unsigned)planes, (unsigned)((g.grid + BS_T - 1) / BS_T));
    bs_bwd_axis_k<<<gz, BS_T, 0, st>>>(t2, dctrl, g.n[0], g.m[0], g.m[1] * g.m[2], g.s[0], 0, tab);
    DF_LAUNCH_CHECK();
  }
  return 0;
}
