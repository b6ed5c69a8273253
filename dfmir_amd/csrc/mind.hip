// MIND-SSC (Heinrich et al., MICCAI 2013): the self-similarity descriptor of a single-channel image and the L2 loss of two
// descriptors, forward and backward, 2-D and 3-D.  Build-defined (include/dfmir_hip.h states the definition).
//
// Neighbours n = 2 * axis + (0: -d, 1: +d) along the axes (z, y, x); channels = the pairs (p < q) of neighbours on
// DIFFERENT axes in lexicographic order: (0,2) (0,3) (0,4) (0,5) (1,2) (1,3) (1,4) (1,5) (2,4) (2,5) (3,4) (3,5).  A 2-D
// image has the last four of them (its neighbours -y, +y, -x, +x are 2..5 here), so one template serves both ranks.
//
// Forward
//   mind_a_k    one workgroup per output tile: the tile of I with a halo of r + d per side (replicated border) is staged in
//               LDS once and serves all channels; per channel s = (I(. + p) - I(. + q))^2 over the tile with a halo of r,
//               then the box sum as three separable LDS passes; D_k stays in registers, the epilogue writes m_k = D_k - min_j D_j
//               and adds V = mean_k m_k (in double) into the workgroup's partial slot.
//   df_slot_mean_k  adds the slots in index order: mu = sum V / voxels (one scalar per image tensor, on the device).
//   mind_desc_k / mind_loss_k   apply mu: M_k = exp(-m_k / clamp(V, 0.001 mu, 1000 mu)); the loss kernel reduces
//               mask * mean_k (Ma_k - Mb_k)^2 and the mask itself into per-workgroup double slots, mind_fin_k adds them in
//               index order.  No atomics anywhere: loss and gradients are bit-identical from run to run.
// Backward (gather form)
//   mind_g_k      per voxel dL/dD_k from the stored m of both images (V and the first-index argmin are recomputed from m:
//                 the minimal channel is the first with m_k == 0).
//   mind_box_adj_k  adjoint of the replicate-border box mean, three separable LDS passes per (tile, channel): a border voxel
//                 collects, with multiplicity, the windows that clamp onto it.
//   mind_shift_adj_k  adjoint of the clamped shifts: per voxel u and neighbour n the up-to-(d+1) sources y with
//                 clamp(y + p_n) = u, times the four partner samples.
//
// What lives between forward and backward: m (C fp32 per voxel and image: 48 B/voxel/image in 3-D, 16 in 2-D) and three
// scalars.  The backward reads it once and needs two C-channel scratch volumes (dL/dD and its box adjoint), reused for the
// second image.  Storing m instead of recomputing it costs one C-channel write + read per image and saves the whole of
// mind_a_k (the LDS-bound part) in the backward.
#include "common.h"

namespace {

constexpr int MIND_T = 256;                 // threads per workgroup
constexpr int MIND_NOUT = 4;                // tile outputs per thread of mind_a_k at most
constexpr int MIND_LDS = 16128;             // floats of (dynamic) LDS per workgroup at most: 63 KB
constexpr int MIND_MAXWG = 1024;            // workgroups (= partial slots) of the point-wise reductions
constexpr int MIND_STAT = 16;               // floats at the head of ws: mu_a, mu_b, normaliser

__constant__ int MIND_P[12] = {0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3};
__constant__ int MIND_Q[12] = {2, 3, 4, 5, 2, 3, 4, 5, 4, 5, 4, 5};

// i / d as one multiply-high (exact for i < 2^32 / d): the LDS loops decode a linear index per element
struct MindDiv { unsigned m; int d; };
__device__ __forceinline__ int mind_div(int i, MindDiv v) { return (int)__umulhi((unsigned)i, v.m); }

struct MindGeom {
  int B, D, H, W;
  int r, d, rz, hz;       // rz / hz: radius / halo along z (0 for a 2-D image)
  int tz, ty, tx;         // tile
  int ntz, nty, ntx;
  float inv;              // (2r+1)^-nd
  MindDiv dIX, dIXY, dSX, dSXY, dTX, dTXY;   // I tile row / plane, s tile row / plane, output tile row / plane
};

__device__ __forceinline__ int clampi(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }
// channel of the neighbour pair (n, n2) on different axes
__device__ __forceinline__ int mind_chan(int n, int n2) {
  const int i = n < n2 ? n : n2, j = n < n2 ? n2 : n;
  return i < 2 ? 4 * i + (j - 2) : 8 + 2 * (i - 2) + (j - 4);
}

// V, Vc and M of one voxel from its C values of m: the ONE place these are formed, so forward and backward agree bit for bit
template <int C>
__device__ __forceinline__ float mind_mean(const float* m) {
  float s = m[0];
#pragma unroll
  for (int k = 1; k < C; ++k) s += m[k];
  return s / (float)C;
}
__device__ __forceinline__ float mind_vc(float V, float mu) { return fminf(fmaxf(V, 0.001f * mu), 1000.f * mu); }

// ------------------------------------------------------------------------------------------------ forward, pass A
template <int ND>
__global__ __launch_bounds__(MIND_T) void mind_a_k(const float* __restrict__ I, MindGeom g, float* __restrict__ m,
                                                   double* __restrict__ partV) {
  constexpr int C = ND == 3 ? 12 : 4, K0 = 12 - C;
  extern __shared__ float lds[];
  __shared__ double red[MIND_T / 64];
  const int tid = threadIdx.x;
  const int h = g.r + g.d, r = g.r;
  const int IY = g.ty + 2 * h, IX = g.tx + 2 * h, IZ = g.tz + 2 * g.hz;
  const int SZ = g.tz + 2 * g.rz, SY = g.ty + 2 * r, SX = g.tx + 2 * r;
  float* sI = lds;
  float* sS = sI + IZ * IY * IX;
  float* sX = sS + SZ * SY * SX;
  int t = blockIdx.x;
  const int x0 = (t % g.ntx) * g.tx; t /= g.ntx;
  const int y0 = (t % g.nty) * g.ty; t /= g.nty;
  const int z0 = (t % g.ntz) * g.tz;
  const int b = t / g.ntz;
  const long long vol = (long long)g.D * g.H * g.W;
  const float* Ib = I + b * vol;
  for (int i = tid; i < IZ * IY * IX; i += MIND_T) {
    const int lz = mind_div(i, g.dIXY), rem = i - lz * IY * IX, ly = mind_div(rem, g.dIX), lx = rem - ly * IX;
    const int gz = clampi(z0 - g.hz + lz, g.D), gy = clampi(y0 - h + ly, g.H), gx = clampi(x0 - h + lx, g.W);
    sI[i] = Ib[((long long)gz * g.H + gy) * g.W + gx];
  }
  const int nout = g.tz * g.ty * g.tx;
  float Dk[MIND_NOUT][C];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < C; ++k) {
    const int p = MIND_P[K0 + k], q = MIND_Q[K0 + k];
    const int sp = (p & 1) ? g.d : -g.d, sq = (q & 1) ? g.d : -g.d;
    const int offP = (p >> 1) == 0 ? sp * IY * IX : ((p >> 1) == 1 ? sp * IX : sp);
    const int offQ = (q >> 1) == 0 ? sq * IY * IX : ((q >> 1) == 1 ? sq * IX : sq);
    // s at the (clamped) position of every box tap of the tile
    for (int i = tid; i < SZ * SY * SX; i += MIND_T) {
      const int lz = mind_div(i, g.dSXY), rem = i - lz * SY * SX, ly = mind_div(rem, g.dSX), lx = rem - ly * SX;
      const int cz = clampi(z0 - g.rz + lz, g.D) - (z0 - g.hz);
      const int cy = clampi(y0 - r + ly, g.H) - (y0 - h);
      const int cx = clampi(x0 - r + lx, g.W) - (x0 - h);
      const int c = (cz * IY + cy) * IX + cx;
      const float df = sI[c + offP] - sI[c + offQ];
      sS[i] = df * df;
    }
    __syncthreads();
    for (int i = tid; i < SZ * SY * g.tx; i += MIND_T) {          // box along x
      const int row = mind_div(i, g.dTX);
      const float* s = sS + row * SX + (i - row * g.tx);
      float acc = s[0];
      for (int u = 1; u <= 2 * r; ++u) acc += s[u];
      sX[i] = acc;
    }
    __syncthreads();
    for (int i = tid; i < SZ * g.ty * g.tx; i += MIND_T) {        // box along y, into the (dead) s buffer
      const int z = mind_div(i, g.dTXY), rem = i - z * g.ty * g.tx;      // rem = y * tx + x
      const float* s = sX + z * SY * g.tx + rem;
      float acc = s[0];
      for (int u = 1; u <= 2 * r; ++u) acc += s[u * g.tx];
      sS[i] = acc;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < MIND_NOUT; ++j) {                         // box along z, into registers
      const int o = tid + MIND_T * j;
      float acc = 0.f;
      if (o < nout) {
        const float* s = sS + o;
        acc = s[0];
        for (int u = 1; u <= 2 * g.rz; ++u) acc += s[u * g.ty * g.tx];
      }
      Dk[j][k] = acc * g.inv;
    }
    __syncthreads();
  }
  double vs = 0.0;
#pragma unroll
  for (int j = 0; j < MIND_NOUT; ++j) {
    const int o = tid + MIND_T * j;
    if (o >= nout) continue;
    const int lz = mind_div(o, g.dTXY), rem = o - lz * g.ty * g.tx, ly = mind_div(rem, g.dTX);
    const int x = x0 + rem - ly * g.tx, y = y0 + ly, z = z0 + lz;
    if (x >= g.W || y >= g.H || z >= g.D) continue;
    float mn = Dk[j][0];
#pragma unroll
    for (int k = 1; k < C; ++k) mn = fminf(mn, Dk[j][k]);
    float mk[C];
#pragma unroll
    for (int k = 0; k < C; ++k) mk[k] = Dk[j][k] - mn;
    vs += (double)mind_mean<C>(mk);
    float* mo = m + (long long)b * C * vol + ((long long)z * g.H + y) * g.W + x;
#pragma unroll
    for (int k = 0; k < C; ++k) mo[k * vol] = mk[k];
  }
  vs = block_sum_ordered<MIND_T>(vs, red);
  if (tid == 0) partV[blockIdx.x] = vs;
}

// ------------------------------------------------------------------------------------------------ forward, pass B
template <int C>
__global__ __launch_bounds__(MIND_T) void mind_desc_k(const float* __restrict__ m, const float* __restrict__ mu,
                                                      long long vol, long long n, float* __restrict__ out) {
  const float u = mu[0];
  for (long long v = (long long)blockIdx.x * MIND_T + threadIdx.x; v < n; v += (long long)gridDim.x * MIND_T) {
    const long long base = (v / vol) * C * vol + v % vol;
    float mk[C];
#pragma unroll
    for (int k = 0; k < C; ++k) mk[k] = m[base + k * vol];
    const float Vc = mind_vc(mind_mean<C>(mk), u);
#pragma unroll
    for (int k = 0; k < C; ++k) out[base + k * vol] = expf(-mk[k] / Vc);
  }
}

template <int C>
__global__ __launch_bounds__(MIND_T) void mind_loss_k(const float* __restrict__ ma, const float* __restrict__ mb,
                                                      const float* __restrict__ mask, const float* __restrict__ stat,
                                                      long long vol, long long n, double* __restrict__ part) {
  __shared__ double red[MIND_T / 64];
  const float ua = stat[0], ub = stat[1];
  double acc = 0.0, wacc = 0.0;
  for (long long v = (long long)blockIdx.x * MIND_T + threadIdx.x; v < n; v += (long long)gridDim.x * MIND_T) {
    const long long base = (v / vol) * C * vol + v % vol;
    float a[C], bq[C];
#pragma unroll
    for (int k = 0; k < C; ++k) { a[k] = ma[base + k * vol]; bq[k] = mb[base + k * vol]; }
    const float Va = mind_vc(mind_mean<C>(a), ua), Vb = mind_vc(mind_mean<C>(bq), ub);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < C; ++k) {
      const float df = expf(-a[k] / Va) - expf(-bq[k] / Vb);
      s += df * df;
    }
    const float w = mask ? mask[v] : 1.f;
    if (w != 0.f) acc += (double)w * (double)(s / (float)C);       // (a zero weight also hides a NaN descriptor)
    wacc += (double)w;
  }
  acc = block_sum_ordered<MIND_T>(acc, red);
  wacc = block_sum_ordered<MIND_T>(wacc, red);
  if (threadIdx.x == 0) { part[2 * blockIdx.x] = acc; part[2 * blockIdx.x + 1] = wacc; }
}

// loss = sum / sum(mask); an empty mask gives 0 and a zero normaliser (the backward then writes zeros)
__global__ __launch_bounds__(MIND_T) void mind_fin_k(const double* __restrict__ part, int nslots, float* __restrict__ stat,
                                                     float* __restrict__ out) {
  __shared__ double red[MIND_T / 64];
  double s = 0.0, w = 0.0;
  for (int i = threadIdx.x; i < nslots; i += MIND_T) { s += part[2 * i]; w += part[2 * i + 1]; }
  s = block_sum_ordered<MIND_T>(s, red);
  w = block_sum_ordered<MIND_T>(w, red);
  if (threadIdx.x == 0) {
    const bool ok = w > 0.0;
    out[0] = ok ? (float)(s / w) : 0.f;
    stat[2] = ok ? (float)(1.0 / w) : 0.f;
  }
}

// ------------------------------------------------------------------------------------------------ backward
// gD_k = dL/dD_k of image `self`:  e_k = gout 2 w norm / C (Ms_k - Mo_k);  dL/dm_k = -e_k Ms_k / Vc
//   + [V not clamped] (1 / C) sum_j e_j Ms_j m_j / Vc^2;  dL/dD_k = dL/dm_k - [k = first argmin] sum_j dL/dm_j.
template <int C>
__global__ __launch_bounds__(MIND_T) void mind_g_k(const float* __restrict__ ms, const float* __restrict__ mo,
                                                   const float* __restrict__ mask, const float* __restrict__ stat, int self,
                                                   const float* __restrict__ gout, long long vol, long long n,
                                                   float* __restrict__ gD) {
  const float us = stat[self], uo = stat[1 - self];
  const float coef = gout[0] * 2.f * stat[2] / (float)C;
  for (long long v = (long long)blockIdx.x * MIND_T + threadIdx.x; v < n; v += (long long)gridDim.x * MIND_T) {
    const long long base = (v / vol) * C * vol + v % vol;
    const float w = mask ? mask[v] : 1.f;
    if (w == 0.f || coef == 0.f) {
#pragma unroll
      for (int k = 0; k < C; ++k) gD[base + k * vol] = 0.f;
      continue;
    }
    float a[C], bq[C];
#pragma unroll
    for (int k = 0; k < C; ++k) { a[k] = ms[base + k * vol]; bq[k] = mo[base + k * vol]; }
    const float V = mind_mean<C>(a);
    const float Vs = mind_vc(V, us), Vo = mind_vc(mind_mean<C>(bq), uo);
    const bool open = V >= 0.001f * us && V <= 1000.f * us;
    const float cw = coef * w;
    float gm[C], through = 0.f;
    int kmin = 0;
    bool found = false;
#pragma unroll
    for (int k = 0; k < C; ++k) {
      const float Ms = expf(-a[k] / Vs);
      const float e = cw * (Ms - expf(-bq[k] / Vo));
      gm[k] = -e * Ms / Vs;
      through += e * Ms * a[k];
      if (!found && a[k] == 0.f) { kmin = k; found = true; }
    }
    const float tv = open ? through / (Vs * Vs) / (float)C : 0.f;
    float tot = 0.f;
#pragma unroll
    for (int k = 0; k < C; ++k) { gm[k] += tv; tot += gm[k]; }
#pragma unroll
    for (int k = 0; k < C; ++k) gD[base + k * vol] = k == kmin ? gm[k] - tot : gm[k];
  }
}

// sum over the sources of one axis whose clamped window positions fall on `pos`:  sum_{u: clamp(u) = pos} sum_t in(u - t),
// in = 0 outside [0, ext).  base[0] holds global coordinate `org`; the callers' tiles hold every coordinate read here.
__device__ __forceinline__ float mind_adj1(const float* base, int stride, int pos, int ext, int r, int org) {
  if (pos > 0 && pos < ext - 1) {          // no window clamps onto an inner position; taps outside the volume hold zeros
    const float* s = base + (pos - r - org) * stride;
    float v = s[0];
    for (int t = 1; t <= 2 * r; ++t) v += s[t * stride];
    return v;
  }
  const int ulo = pos == 0 ? -r : pos, uhi = pos == ext - 1 ? ext - 1 + r : pos;
  float v = 0.f;
  for (int u = ulo; u <= uhi; ++u)
    for (int t = -r; t <= r; ++t) {
      const int xs = u - t;
      if (xs >= 0 && xs < ext) v += base[(xs - org) * stride];
    }
  return v;
}

// gS = adjoint of the replicate-border box mean, one (tile, channel) per workgroup
__global__ __launch_bounds__(MIND_T) void mind_box_adj_k(const float* __restrict__ gD, MindGeom g, int C,
                                                         float* __restrict__ gS) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x, r = g.r;
  const int SZ = g.tz + 2 * g.rz, SY = g.ty + 2 * r, SX = g.tx + 2 * r;
  float* sS = lds;
  float* sX = sS + SZ * SY * SX;
  int t = blockIdx.x;
  const int x0 = (t % g.ntx) * g.tx; t /= g.ntx;
  const int y0 = (t % g.nty) * g.ty; t /= g.nty;
  const int z0 = (t % g.ntz) * g.tz; t /= g.ntz;       // t = b * C + k
  const long long vol = (long long)g.D * g.H * g.W;
  const float* src = gD + t * vol;
  float* dst = gS + t * vol;
  for (int i = tid; i < SZ * SY * SX; i += MIND_T) {
    const int lz = mind_div(i, g.dSXY), rem = i - lz * SY * SX, ly = mind_div(rem, g.dSX);
    const int gx = x0 - r + rem - ly * SX, gy = y0 - r + ly, gz = z0 - g.rz + lz;
    const bool in = gx >= 0 && gx < g.W && gy >= 0 && gy < g.H && gz >= 0 && gz < g.D;
    sS[i] = in ? src[((long long)gz * g.H + gy) * g.W + gx] : 0.f;
  }
  __syncthreads();
  for (int i = tid; i < SZ * SY * g.tx; i += MIND_T) {
    const int row = mind_div(i, g.dTX), x = x0 + i - row * g.tx;
    sX[i] = x < g.W ? mind_adj1(sS + row * SX, 1, x, g.W, r, x0 - r) : 0.f;
  }
  __syncthreads();
  for (int i = tid; i < SZ * g.ty * g.tx; i += MIND_T) {
    const int z = mind_div(i, g.dTXY), rem = i - z * g.ty * g.tx, ly = mind_div(rem, g.dTX), x = rem - ly * g.tx;
    const int y = y0 + ly;
    sS[i] = y < g.H ? mind_adj1(sX + z * SY * g.tx + x, g.tx, y, g.H, r, y0 - r) : 0.f;
  }
  __syncthreads();
  for (int o = tid; o < g.tz * g.ty * g.tx; o += MIND_T) {
    const int lz = mind_div(o, g.dTXY), rem = o - lz * g.ty * g.tx, ly = mind_div(rem, g.dTX), lx = rem - ly * g.tx;
    const int x = x0 + lx, y = y0 + ly, z = z0 + lz;
    if (x >= g.W || y >= g.H || z >= g.D) continue;
    const float v = mind_adj1(sS + ly * g.tx + lx, g.ty * g.tx, z, g.D, g.rz, z0 - g.rz);
    dst[((long long)z * g.H + y) * g.W + x] = v * g.inv;
  }
}

// dI(u) = 2 sum_n sum_{y: clamp(y + p_n) = u} sum_{n2 on another axis} (I(u) - I(clamp(y + p_n2))) gS_{chan(n, n2)}(y)
template <int ND>
__global__ __launch_bounds__(MIND_T) void mind_shift_adj_k(const float* __restrict__ I, const float* __restrict__ gS,
                                                           MindGeom g, float* __restrict__ dI) {
  constexpr int C = ND == 3 ? 12 : 4, K0 = 12 - C, N0 = ND == 3 ? 0 : 2;
  const long long vol = (long long)g.D * g.H * g.W, n = vol * g.B;
  const long long v = (long long)blockIdx.x * MIND_T + threadIdx.x;
  if (v >= n) return;
  const long long b = v / vol, vox = v % vol;
  const int ext[3] = {g.D, g.H, g.W};
  const long long str[3] = {(long long)g.H * g.W, g.W, 1};
  int u[3];
  u[2] = (int)(vox % g.W);
  u[1] = (int)((vox / g.W) % g.H);
  u[0] = (int)(vox / ((long long)g.W * g.H));
  const float* Ib = I + b * vol;
  const float* gb = gS + b * C * vol;
  const float Iu = Ib[vox];
  float acc = 0.f;
#pragma unroll
  for (int nb = N0; nb < 6; ++nb) {
    const int a = nb >> 1, e = ext[a];
    int lo, hi;
    if (nb & 1) {                         // sources y with clamp(y + d) = u[a]
      if (u[a] == e - 1) { lo = e - 1 - g.d < 0 ? 0 : e - 1 - g.d; hi = e - 1; }
      else { lo = hi = u[a] - g.d; if (lo < 0) continue; }
    } else {                              // clamp(y - d) = u[a]
      if (u[a] == 0) { lo = 0; hi = g.d > e - 1 ? e - 1 : g.d; }
      else { lo = hi = u[a] + g.d; if (hi > e - 1) continue; }
    }
    for (int ys = lo; ys <= hi; ++ys) {
      const long long yv = vox + (long long)(ys - u[a]) * str[a];
#pragma unroll
      for (int n2 = N0; n2 < 6; ++n2) {
        const int a2 = n2 >> 1;
        if (a2 == a) continue;
        const int c2 = clampi(u[a2] + ((n2 & 1) ? g.d : -g.d), ext[a2]);
        const float other = Ib[yv + (long long)(c2 - u[a2]) * str[a2]];
        acc += (Iu - other) * gb[(long long)(mind_chan(nb, n2) - K0) * vol + yv];
      }
    }
  }
  dI[v] = 2.f * acc;
}

// ------------------------------------------------------------------------------------------------ host side
bool mind_args_ok(int nd, int B, int D, int H, int W, int r, int d) {
  if ((nd != 2 && nd != 3) || B < 1 || D < 1 || H < 1 || W < 1 || (nd == 2 && D != 1)) return false;
  if (r < 1 || r > 4 || d < 1 || d > 4) return false;
  return (long long)B * D * H * W * 12 < (1LL << 40);
}

MindDiv mind_mkdiv(int d) { return MindDiv{(unsigned)((1ULL << 32) / (unsigned)d + 1ULL), d}; }   // d >= 2

long long mind_lds_need(int nd, int r, int d, int tz, int ty, int tx) {
  const int h = r + d, hz = nd == 3 ? h : 0, rz = nd == 3 ? r : 0;
  return (long long)(tz + 2 * hz) * (ty + 2 * h) * (tx + 2 * h) + (long long)(tz + 2 * rz) * (ty + 2 * r) * (tx + 2 * r) +
         (long long)(tz + 2 * rz) * (ty + 2 * r) * tx;
}

// the largest tile of a fixed preference list that fits the LDS (the last entry fits every allowed r, d)
bool mind_geom(int nd, int B, int D, int H, int W, int r, int d, MindGeom* g) {
  static const int T3[][3] = {{4, 8, 32}, {2, 8, 32}, {2, 4, 32}, {1, 8, 32}, {2, 4, 16}, {1, 4, 16}, {1, 2, 16}, {1, 1, 16}};
  static const int T2[][3] = {{1, 32, 32}, {1, 16, 32}, {1, 8, 32}};
  const int (*T)[3] = nd == 3 ? T3 : T2;
  const int nT = nd == 3 ? 8 : 3;
  int pick = -1;
  for (int i = 0; i < nT && pick < 0; ++i) {
    if (T[i][0] > 1 && T[i][0] > D) continue;
    if (T[i][0] * T[i][1] * T[i][2] > MIND_T * MIND_NOUT) continue;
    if (mind_lds_need(nd, r, d, T[i][0], T[i][1], T[i][2]) <= MIND_LDS) pick = i;
  }
  if (pick < 0) return false;
  g->B = B; g->D = D; g->H = H; g->W = W;
  g->r = r; g->d = d;
  g->rz = nd == 3 ? r : 0;
  g->hz = nd == 3 ? r + d : 0;
  g->tz = T[pick][0]; g->ty = T[pick][1]; g->tx = T[pick][2];
  g->ntz = (D + g->tz - 1) / g->tz; g->nty = (H + g->ty - 1) / g->ty; g->ntx = (W + g->tx - 1) / g->tx;
  const double win = 2.0 * r + 1.0;
  g->inv = (float)(1.0 / (nd == 3 ? win * win * win : win * win));
  const int h = r + d, IX = g->tx + 2 * h, IY = g->ty + 2 * h, SX = g->tx + 2 * r, SY = g->ty + 2 * r;
  g->dIX = mind_mkdiv(IX); g->dIXY = mind_mkdiv(IX * IY);
  g->dSX = mind_mkdiv(SX); g->dSXY = mind_mkdiv(SX * SY);
  g->dTX = mind_mkdiv(g->tx); g->dTXY = mind_mkdiv(g->tx * g->ty);
  const long long tiles = (long long)B * g->ntz * g->nty * g->ntx;
  return tiles * 12 < (1LL << 31);
}

// bytes of dynamic LDS: mind_a_k holds the I tile, the s tile and the x-pass buffer, mind_box_adj_k the last two
inline size_t mind_lds_bytes(const MindGeom& g, bool with_image) {
  const int h = g.r + g.d;
  const long long I = (long long)(g.tz + 2 * g.hz) * (g.ty + 2 * h) * (g.tx + 2 * h);
  const long long S = (long long)(g.tz + 2 * g.rz) * (g.ty + 2 * g.r) * (g.tx + 2 * g.r);
  const long long X = (long long)(g.tz + 2 * g.rz) * (g.ty + 2 * g.r) * g.tx;
  return (size_t)((with_image ? I : 0) + S + X) * sizeof(float);
}
inline long long mind_tiles(const MindGeom& g) { return (long long)g.B * g.ntz * g.nty * g.ntx; }
inline int mind_pw_nwg(long long n) { return (int)df_grid(n, MIND_T, MIND_MAXWG); }

// ws: [stat: MIND_STAT floats][partV a, partV b: tiles doubles each][loss partials: 2 * MIND_MAXWG doubles][m_a][m_b]
struct MindWs {
  float* stat;
  double *pva, *pvb, *pl;
  float *ma, *mb;
  long long floats;
};
MindWs mind_ws(float* ws, const MindGeom& g, int C) {
  MindWs w;
  const long long tiles = mind_tiles(g), mfl = (long long)g.B * C * g.D * g.H * g.W;
  w.stat = ws;
  w.pva = reinterpret_cast<double*>(ws + MIND_STAT);
  w.pvb = w.pva + tiles;
  w.pl = w.pvb + tiles;
  w.ma = ws + MIND_STAT + 2 * (2 * tiles + 2 * MIND_MAXWG);
  w.mb = w.ma + mfl;
  w.floats = MIND_STAT + 2 * (2 * tiles + 2 * MIND_MAXWG) + 2 * mfl;
  return w;
}

int mind_pass_a(const float* I, int nd, const MindGeom& g, float* m, double* part, float* mu, hipStream_t st) {
  const unsigned tiles = (unsigned)mind_tiles(g);
  if (nd == 3) mind_a_k<3><<<tiles, MIND_T, mind_lds_bytes(g, true), st>>>(I, g, m, part);
  else mind_a_k<2><<<tiles, MIND_T, mind_lds_bytes(g, true), st>>>(I, g, m, part);
  DF_LAUNCH_CHECK();
  df_slot_mean_k<MIND_T><<<1, MIND_T, 0, st>>>(part, (int)tiles, (double)g.B * g.D * g.H * g.W, mu);
  DF_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" long long dfmir_mind_ws_floats(int nd, int B, int D, int H, int W, int radius, int dilation, int which) {
  MindGeom g;
  if (!mind_args_ok(nd, B, D, H, W, radius, dilation) || (which != 0 && which != 1)) return -1;
  if (!mind_geom(nd, B, D, H, W, radius, dilation, &g)) return -1;
  const int C = nd == 3 ? 12 : 4;
  if (which == 1) return 2LL * B * C * D * H * W;
  return mind_ws(nullptr, g, C).floats;
}

extern "C" int dfmir_mind_desc(const float* I, int nd, int B, int D, int H, int W, int radius, int dilation, float* ws,
                               float* out, void* stream) {
  MindGeom g;
  DF_ARG_CHECK(I && ws && out && mind_args_ok(nd, B, D, H, W, radius, dilation) &&
               mind_geom(nd, B, D, H, W, radius, dilation, &g));
  hipStream_t st = (hipStream_t)stream;
  const int C = nd == 3 ? 12 : 4;
  const MindWs w = mind_ws(ws, g, C);
  if (int rc = mind_pass_a(I, nd, g, w.ma, w.pva, w.stat, st)) return rc;
  const long long vol = (long long)D * H * W, n = vol * B;
  if (nd == 3) mind_desc_k<12><<<mind_pw_nwg(n), MIND_T, 0, st>>>(w.ma, w.stat, vol, n, out);
  else mind_desc_k<4><<<mind_pw_nwg(n), MIND_T, 0, st>>>(w.ma, w.stat, vol, n, out);
  DF_LAUNCH_CHECK();
  return 0;
}

extern "C" int dfmir_mind_fwd(const float* a, const float* b, const float* mask, int nd, int B, int D, int H, int W,
                              int radius, int dilation, float* ws, float* out, void* stream) {
  MindGeom g;
  DF_ARG_CHECK(a && b && ws && out && mind_args_ok(nd, B, D, H, W, radius, dilation) &&
               mind_geom(nd, B, D, H, W, radius, dilation, &g));
  hipStream_t st = (hipStream_t)stream;
  const int C = nd == 3 ? 12 : 4;
  const MindWs w = mind_ws(ws, g, C);
  if (int rc = mind_pass_a(a, nd, g, w.ma, w.pva, w.stat, st)) return rc;
  if (int rc = mind_pass_a(b, nd, g, w.mb, w.pvb, w.stat + 1, st)) return rc;
  const long long vol = (long long)D * H * W, n = vol * B;
  const int nwg = mind_pw_nwg(n);
  if (nd == 3) mind_loss_k<12><<<nwg, MIND_T, 0, st>>>(w.ma, w.mb, mask, w.stat, vol, n, w.pl);
  else mind_loss_k<4><<<nwg, MIND_T, 0, st>>>(w.ma, w.mb, mask, w.stat, vol, n, w.pl);
  DF_LAUNCH_CHECK();
  mind_fin_k<<<1, MIND_T, 0, st>>>(w.pl, nwg, w.stat, out);
  DF_LAUNCH_CHECK();
  return 0;
}

extern "C" int dfmir_mind_bwd(const float* a, const float* b, const float* mask, int nd, int B, int D, int H, int W,
                              int radius, int dilation, const float* ws, float* tmp, const float* gout, float* da, float* db,
                              void* stream) {
  MindGeom g;
  DF_ARG_CHECK(a && b && ws && tmp && gout && mind_args_ok(nd, B, D, H, W, radius, dilation) &&
               mind_geom(nd, B, D, H, W, radius, dilation, &g));
  if (!da && !db) return 0;
  hipStream_t st = (hipStream_t)stream;
  const int C = nd == 3 ? 12 : 4;
  const MindWs w = mind_ws(const_cast<float*>(ws), g, C);
  const long long vol = (long long)D * H * W, n = vol * B;
  float* gD = tmp;
  float* gS = tmp + n * C;
  const unsigned tiles = (unsigned)(mind_tiles(g) * C);
  for (int self = 0; self < 2; ++self) {
    float* dI = self ? db : da;
    if (!dI) continue;
    const float* ms = self ? w.mb : w.ma;
    const float* mo = self ? w.ma : w.mb;
    const float* I = self ? b : a;
    if (nd == 3) mind_g_k<12><<<mind_pw_nwg(n), MIND_T, 0, st>>>(ms, mo, mask, w.stat, self, gout, vol, n, gD);
    else mind_g_k<4><<<mind_pw_nwg(n), MIND_T, 0, st>>>(ms, mo, mask, w.stat, self, gout, vol, n, gD);
    DF_LAUNCH_CHECK();
    mind_box_adj_k<<<tiles, MIND_T, mind_lds_bytes(g, false), st>>>(gD, g, C, gS);
    DF_LAUNCH_CHECK();
    if (nd == 3) mind_shift_adj_k<3><<<df_grid(n, MIND_T, 1LL << 30), MIND_T, 0, st>>>(I, gS, g, dI);
    else mind_shift_adj_k<2><<<df_grid(n, MIND_T, 1LL << 30), MIND_T, 0, st>>>(I, gS, g, dI);
    DF_LAUNCH_CHECK();
  }
  return 0;
}
