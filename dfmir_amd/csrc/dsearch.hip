// Discrete displacement search, the first stage of a two-stage (discrete, then Adam) instance registration, 2-D and 3-D:
// average pooling of features onto the search grid, the SSD cost volume over a window of integer displacements, the
// coupled-convex argmin and the box mean of a displacement field.  Build-defined (include/dfmir_hip.h, ops.pool_features,
// ops.ssd_cost_volume, ops.cost_argmin and ops.box_smooth_flow state the definitions):
//
//   d_k, k = 0 .. K - 1, K = (2r + 1)^ND: the displacements {-r .. r}^ND in row-major order (dz,) dy, dx, -r first, in voxels
//   of the grid the features live on and in the flow's channel order.
//   pool    out[b,c,X]  = mean of in[b,c,g X + {0 .. g-1}^ND]                       the remainder at the far faces is dropped
//   cost    cost[b,k,x] = (1/C) sum_c (fix[b,c,x] - mov[b,c,x + d_k])^2            mov reads 0 outside the volume
//   argmin  idx[b,x]    = argmin_k cost[b,k,x] + coeff sum_a (d_k[a] - soft[b,a,x])^2,  disp[b,a,x] = d_idx[a]
//   smooth  out[b,a,x]  = the mean of disp[b,a,.] over the in-volume ones of the 3^ND neighbours of x
//
//   ds_pool_k    one thread per (pooled voxel, padded channel); the window is added in double in a fixed order and rounded
//                once.  Writes the planar result and / or the layout the cost kernel reads: voxel-major [B][S][CP], CP = C
//                rounded up to 4, zeros in the padding channels (ops.pack_features' layout).
//   ds_cost_k    <ND, CP>.  A workgroup of 256 threads owns a 32 x 8 in-plane tile of ONE z-plane of one sample, one voxel per
//                thread, its CP fixed features in registers, and ONE dz (3-D) and one chunk of `ndy` consecutive dy of the
//                window.  It stages the moving rows the chunk touches with their x halo, (32 + 2r) x (8 + ndy - 1) voxels of
//                plane z + dz, into LDS as CP / 4 planes of float4 -- a wave is two rows of 32 consecutive x, and each 16-lane
//                group of a 16-byte LDS read lies within one row on 16 consecutive 16-byte slots: no bank conflict whatever
//                the row stride (a channel-last [pos][CP] image would be 2-way at CP = 8 and 4-way at CP = 16) -- then walks
//                the chunk's (dy, dx) and stores one cost per thread and displacement, 128 contiguous bytes per tile row.
//                ndy = 2r + 1 (the whole in-plane window in one stage) wherever that fits 64 KB of LDS -- everywhere but 2-D
//                with r >= 7 and CP = 16, where the window takes two chunks.  One dz per workgroup because a coarse grid is
//                small: 40 x 48 x 56 is 480 tiles for 256 compute units, 3360 workgroups with the 7 dz apart.  The staged
//                image is bounded by (32 + 2r)(8 + 2r) CP 4 bytes = 40 KB at the largest 3-D case (r = 4, CP = 16).  Re-read factor: a moving voxel is staged by the
//                (2r + 1) dz planes times the tiles whose halo holds it, (32 + 2r)(8 + ndy - 1) / 256 per chunk: 7 x 2.1 at
//                r = 3, against K = 343 reads without the staging; the fixed features are read once per (dz, chunk).  Every
//                channel is added in the order c = 0 .. CP - 1 with an fma per channel for every k, padding channels
//                included (they add 0), so displacements whose sample is outside the volume tie bit for bit at
//                sum_c fix_c^2 / C, and no cost depends on how the window was cut.  No atomics, no read-modify-write of the
//                cost volume: every cost is written once.
//   ds_argmin_k  one thread per voxel walks k upwards with a strict <: the lowest k wins a tie, a NaN is never selected
//                (all NaN: index 0).  Reads the cost volume once, coalesced along x for each k, eight loads in flight per
//                thread.
//   ds_smooth_k  one thread per element, neighbours added in the order (dz,) dy, dx, divided by the in-volume count.
// Nothing syncs with the host, allocates or keeps state; no atomics anywhere: every output is bit-identical from run to run.
#include "common.h"
#include <math.h>

namespace {

constexpr int DS_T = 256;
constexpr int DS_TX = 32, DS_TY = 8;                 // the cost kernel's tile: DS_TX * DS_TY == DS_T
constexpr int DS_MAX_LDS = 64 * 1024;
constexpr int DS_ARG_U = 8;                          // cost loads a thread of the argmin keeps in flight
constexpr long long DS_MAX_ELEMS = 1LL << 31;

struct DsGeom {
  int B, C, D, H, W;
  long long S;
};

inline int ds_max_radius(int nd) { return nd == 3 ? 4 : 8; }

// nd, B and the extents of a [B][..][(D)][H][W] tensor with `chan` floats per voxel: false where the library refuses the shape
inline bool ds_geom(int nd, int B, int C, int D, int H, int W, long long chan, DsGeom* g) {
  if (nd != 2 && nd != 3) return false;
  if (nd == 2) D = 1;
  if (B < 1 || C < 1 || H < 2 || W < 2 || (nd == 3 && D < 2)) return false;
  const long long S = (long long)D * H * W;
  if (S >= DS_MAX_ELEMS || chan < 1 || chan >= DS_MAX_ELEMS || (long long)B * chan >= DS_MAX_ELEMS ||
      (long long)B * chan * S >= DS_MAX_ELEMS)
    return false;
  *g = DsGeom{B, C, D, H, W, S};
  return true;
}

inline long long ds_window(int nd, int r) {
  const long long n = 2 * r + 1;
  return nd == 3 ? n * n * n : n * n;
}

// ------------------------------------------------------------------------------------------------ pooling
// thread -> (b, X, c) with c < CP fastest when only `packed` is written, else (b, c, X) with X fastest
template <int ND>
__global__ __launch_bounds__(DS_T) void ds_pool_k(const float* __restrict__ in, float* __restrict__ out,
                                                  float* __restrict__ packed, int B, int C, int CP, int D, int H, int W,
                                                  int Dp, int Hp, int Wp, int g) {
  // every count here is below 2^31 (ds_geom): 32-bit index arithmetic, 64-bit only where an offset is formed
  const unsigned Sp = (unsigned)Dp * Hp * Wp;
  const unsigned n = (unsigned)B * CP * Sp;
  const unsigned i = blockIdx.x * DS_T + threadIdx.x;
  if (i >= n) return;
  int b, c;
  unsigned X;
  if (out) {
    X = i % Sp;
    c = (int)((i / Sp) % CP);
    b = (int)(i / (Sp * CP));
  } else {
    c = (int)(i % CP);
    X = (i / CP) % Sp;
    b = (int)(i / (CP * Sp));
  }
  float v = 0.f;
  if (c < C) {
    const int xp = (int)(X % Wp), yp = (int)((X / Wp) % Hp), zp = (int)(X / ((unsigned)Wp * Hp));
    const float* src = in + (((long long)b * C + c) * D + (ND == 3 ? zp * g : 0)) * H * W;
    double s = 0.0;
    for (int dz = 0; dz < (ND == 3 ? g : 1); ++dz)
      for (int dy = 0; dy < g; ++dy) {
        const float* row = src + ((long long)dz * H + (yp * g + dy)) * W + xp * g;
        for (int dx = 0; dx < g; ++dx) s += (double)row[dx];
      }
    v = (float)(s / (double)(ND == 3 ? g * g * g : g * g));
    if (out) out[((long long)b * C + c) * Sp + X] = v;
  }
  if (packed) packed[((long long)b * Sp + X) * CP + c] = v;
}

// ------------------------------------------------------------------------------------------------ cost volume
template <int ND, int CP>
__global__ __launch_bounds__(DS_T) void ds_cost_k(const float4* __restrict__ fixp, const float4* __restrict__ movp,
                                                  float* __restrict__ cost, int D, int H, int W, int r, int ndy, int ntx,
                                                  int nty, float cf, float inv_c) {   // C and 1 / C
  extern __shared__ __attribute__((aligned(16))) float4 sm[];   // [J][rows][TW]
  constexpr int J = CP / 4;
  const int t = threadIdx.x;
  const int tx = t & (DS_TX - 1), ty = t / DS_TX;
  const int n = 2 * r + 1;
  const int nchunks = (n + ndy - 1) / ndy;
  // blockIdx.x = (z, tile row, tile column), blockIdx.y = (dz, chunk of dy), blockIdx.z = b
  const int x0 = (int)(blockIdx.x % ntx) * DS_TX, y0 = (int)((blockIdx.x / ntx) % nty) * DS_TY;
  const int z = (int)(blockIdx.x / ((unsigned)ntx * nty)), b = blockIdx.z;
  const int dy0 = (int)(blockIdx.y % nchunks) * ndy - r, ez = ND == 3 ? (int)(blockIdx.y / nchunks) : 0;   // ez = dz + r
  const int x = x0 + tx, y = y0 + ty;
  const bool live = x < W && y < H;
  const int TW = DS_TX + 2 * r;
  const int npos = TW * (DS_TY + ndy - 1);
  const long long S = (long long)D * H * W;
  const long long K = ND == 3 ? (long long)n * n * n : (long long)n * n;

  const int zz = ND == 3 ? z + ez - r : 0;
  const bool zin = zz >= 0 && zz < D;
  const float4* plane = movp + ((long long)b * D + (zin ? zz : 0)) * H * W * J;
  for (int i = t; i < npos * J; i += DS_T) {
    const int j = i % J, pos = i / J;
    const int gx = x0 - r + pos % TW, gy = y0 + dy0 + pos / TW;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (zin && gx >= 0 && gx < W && gy >= 0 && gy < H) v = plane[((long long)gy * W + gx) * J + j];
    sm[j * npos + pos] = v;
  }
  float4 f[J];
#pragma unroll
  for (int j = 0; j < J; ++j)
    f[j] = live ? fixp[(((long long)b * D + z) * H + y) * W * J + (long long)x * J + j] : make_float4(0.f, 0.f, 0.f, 0.f);
  __syncthreads();

  const int dy1 = dy0 + ndy - 1 < r ? dy0 + ndy - 1 : r;
  // the first cost of this workgroup's run of k: k = ((dz + r) n + dy + r) n + dx + r
  float* out = cost + ((long long)b * K + ((long long)ez * n + (dy0 + r)) * n) * S + ((long long)z * H + y) * W + x;
  for (int dy = dy0; dy <= dy1; ++dy) {
    const float4* srow = sm + (ty + dy - dy0) * TW + tx;
    for (int e = 0; e < n; ++e, out += S) {                      // e = dx + r
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const float4 m = srow[j * npos + e];
        float d = f[j].x - m.x;
        s = fmaf(d, d, s);
        d = f[j].y - m.y;
        s = fmaf(d, d, s);
        d = f[j].z - m.z;
        s = fmaf(d, d, s);
        d = f[j].w - m.w;
        s = fmaf(d, d, s);
      }
      float q = s * inv_c;
      q = fmaf(fmaf(-q, cf, s), inv_c, q);                       // one Newton step: s / C to the last bit or two
      if (live) *out = q;
    }
  }
}

// rows of dy per stage, by LDS: the whole window where the image fits DS_MAX_LDS, else the fewest equal chunks that do
inline int ds_cost_ndy(int r, int cp) {
  const int n = 2 * r + 1;
  for (int chunks = 1; chunks <= n; ++chunks) {
    const int ndy = (n + chunks - 1) / chunks;
    if ((long long)(DS_TX + 2 * r) * (DS_TY + ndy - 1) * cp * 4 <= DS_MAX_LDS) return ndy;
  }
  return 0;
}

template <int ND>
int ds_cost_launch(const float* fixp, const float* movp, float* cost, const DsGeom& g, int cp, int r, hipStream_t st) {
  const int ndy = ds_cost_ndy(r, cp);
  if (ndy < 1) return -1;
  const int n = 2 * r + 1;
  const int ntx = (g.W + DS_TX - 1) / DS_TX, nty = (g.H + DS_TY - 1) / DS_TY;
  const long long tiles = (long long)ntx * nty * g.D;
  if (tiles >= DS_MAX_ELEMS) return -1;
  const int nchunks = (n + ndy - 1) / ndy;
  const dim3 grid((unsigned)tiles, (unsigned)((ND == 3 ? n : 1) * nchunks), (unsigned)g.B);
  const size_t lds = (size_t)(DS_TX + 2 * r) * (DS_TY + ndy - 1) * cp * 4;
  const float4* f4 = reinterpret_cast<const float4*>(fixp);
  const float4* m4 = reinterpret_cast<const float4*>(movp);
  const float cf = (float)g.C, inv_c = 1.f / (float)g.C;
  switch (cp) {
    case 4: ds_cost_k<ND, 4><<<grid, DS_T, lds, st>>>(f4, m4, cost, g.D, g.H, g.W, r, ndy, ntx, nty, cf, inv_c); break;
    case 8: ds_cost_k<ND, 8><<<grid, DS_T, lds, st>>>(f4, m4, cost, g.D, g.H, g.W, r, ndy, ntx, nty, cf, inv_c); break;
    case 12: ds_cost_k<ND, 12><<<grid, DS_T, lds, st>>>(f4, m4, cost, g.D, g.H, g.W, r, ndy, ntx, nty, cf, inv_c); break;
    default: ds_cost_k<ND, 16><<<grid, DS_T, lds, st>>>(f4, m4, cost, g.D, g.H, g.W, r, ndy, ntx, nty, cf, inv_c); break;
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------ coupled argmin
template <int ND>
__global__ __launch_bounds__(DS_T) void ds_argmin_k(const float* __restrict__ cost, const float* __restrict__ soft,
                                                    float coeff, int* __restrict__ idx, float* __restrict__ disp, int B,
                                                    long long S, int r) {
  const long long i = (long long)blockIdx.x * DS_T + threadIdx.x;
  if (i >= (long long)B * S) return;
  const int b = (int)(i / S);
  const long long x = i % S;
  const int n = 2 * r + 1;
  const long long K = ND == 3 ? (long long)n * n * n : (long long)n * n;
  float sf[ND];
#pragma unroll
  for (int a = 0; a < ND; ++a) sf[a] = soft ? soft[((long long)b * ND + a) * S + x] : 0.f;
  const float* c = cost + (long long)b * K * S + x;
  float best = __uint_as_float(0x7f800000u);                     // +inf: a NaN never compares below it
  int bi = 0, bz = 0, by = 0, bx = 0;
  int ez = 0, ey = 0, ex = 0;                                    // d_k + r of the k being compared
  const int Ki = (int)K;
  for (int k0 = 0; k0 < Ki; k0 += DS_ARG_U) {                    // DS_ARG_U loads in flight, then their compares in k order
    float v[DS_ARG_U];
#pragma unroll
    for (int u = 0; u < DS_ARG_U; ++u) v[u] = k0 + u < Ki ? c[(long long)(k0 + u) * S] : 0.f;
#pragma unroll
    for (int u = 0; u < DS_ARG_U; ++u) {
      if (k0 + u < Ki) {
        float w = v[u];
        if (soft) {
          const float qx = (float)(ex - r) - sf[ND - 1], qy = (float)(ey - r) - sf[ND - 2];
          float q = ND == 3 ? ((float)(ez - r) - sf[0]) * ((float)(ez - r) - sf[0]) + qy * qy : qy * qy;
          q = q + qx * qx;
          w = w + coeff * q;
        }
        if (w < best) {
          best = w;
          bi = k0 + u;
          bz = ez;
          by = ey;
          bx = ex;
        }
        if (++ex == n) {
          ex = 0;
          if (++ey == n) {
            ey = 0;
            ++ez;
          }
        }
      }
    }
  }
  idx[i] = bi;
  float* d = disp + (long long)b * ND * S + x;
  if (ND == 3) d[0] = (float)(bz - r);
  d[(long long)(ND - 2) * S] = (float)(by - r);
  d[(long long)(ND - 1) * S] = (float)(bx - r);
}

// ------------------------------------------------------------------------------------------------ box mean
template <int ND>
__global__ __launch_bounds__(DS_T) void ds_smooth_k(const float* __restrict__ in, float* __restrict__ out, long long planes,
                                                    int D, int H, int W) {
  const unsigned S = (unsigned)D * H * W;                        // planes * S < 2^31 (ds_geom): 32-bit index arithmetic
  const unsigned i = blockIdx.x * DS_T + threadIdx.x;
  if (i >= (unsigned)planes * S) return;
  const unsigned p = i / S, v = i % S;
  const int x = (int)(v % W), y = (int)((v / W) % H), z = (int)(v / ((unsigned)W * H));
  const float* src = in + (long long)p * S;
  float s = 0.f;
  int cnt = 0;
  for (int dz = (ND == 3 ? -1 : 0); dz <= (ND == 3 ? 1 : 0); ++dz) {
    const int zz = z + dz;
    if (zz < 0 || zz >= D) continue;
    for (int dy = -1; dy <= 1; ++dy) {
      const int yy = y + dy;
      if (yy < 0 || yy >= H) continue;
      for (int dx = -1; dx <= 1; ++dx) {
        const int xx = x + dx;
        if (xx < 0 || xx >= W) continue;
        s += src[((long long)zz * H + yy) * W + xx];
        ++cnt;
      }
    }
  }
  out[i] = s / (float)cnt;
}

}  // namespace

extern "C" int dfmir_dsearch_pool(int nd, const float* in, float* out, float* packed, int B, int C, int D, int H, int W,
                                  int g, void* stream) {
  DsGeom gi, go;
  DF_ARG_CHECK(in && (out || packed) && g >= 1 && C >= 1 && C <= 16);
  const int cp = (C + 3) / 4 * 4;
  DF_ARG_CHECK(ds_geom(nd, B, C, D, H, W, cp, &gi));
  DF_ARG_CHECK(ds_geom(nd, B, C, nd == 3 ? D / g : 1, H / g, W / g, cp, &go));
  const long long n = (long long)B * cp * go.S;
  const unsigned grid = (unsigned)((n + DS_T - 1) / DS_T);
  hipStream_t st = (hipStream_t)stream;
  if (nd == 3) ds_pool_k<3><<<grid, DS_T, 0, st>>>(in, out, packed, B, C, cp, gi.D, H, W, go.D, go.H, go.W, g);
  else ds_pool_k<2><<<grid, DS_T, 0, st>>>(in, out, packed, B, C, cp, 1, H, W, 1, go.H, go.W, g);
  DF_LAUNCH_CHECK();
  return 0;
}

extern "C" int dfmir_dsearch_cost(int nd, const float* fixp, const float* movp, float* cost, int B, int C, int D, int H, int W,
                                  int r, void* stream) {
  DsGeom g;
  DF_ARG_CHECK(fixp && movp && cost && C >= 1 && C <= 16 && (nd == 2 || nd == 3) && r >= 1 && r <= ds_max_radius(nd));
  DF_ARG_CHECK(((reinterpret_cast<uintptr_t>(fixp) | reinterpret_cast<uintptr_t>(movp)) & 15) == 0);
  const int cp = (C + 3) / 4 * 4;
  DF_ARG_CHECK(ds_geom(nd, B, C, D, H, W, cp, &g) && ds_geom(nd, B, C, D, H, W, ds_window(nd, r), &g));
  DF_ARG_CHECK(g.B <= 65535);                                   // grid.z
  hipStream_t st = (hipStream_t)stream;
  const int rc = nd == 3 ? ds_cost_launch<3>(fixp, movp, cost, g, cp, r, st) : ds_cost_launch<2>(fixp, movp, cost, g, cp, r, st);
  DF_ARG_CHECK(rc == 0);
  DF_LAUNCH_CHECK();
  return 0;
}

extern "C" int dfmir_dsearch_argmin(int nd, const float* cost, const float* soft, float coeff, int* idx, float* disp, int B,
                                    int D, int H, int W, int r, void* stream) {
  DsGeom g;
  DF_ARG_CHECK(cost && idx && disp && (nd == 2 || nd == 3) && r >= 1 && r <= ds_max_radius(nd));
  DF_ARG_CHECK(coeff >= 0.f && coeff <= 3.0e38f);                // refuses a NaN too
  DF_ARG_CHECK(ds_geom(nd, B, 1, D, H, W, ds_window(nd, r), &g));
  const long long n = (long long)B * g.S;
  const unsigned grid = (unsigned)((n + DS_T - 1) / DS_T);
  hipStream_t st = (hipStream_t)stream;
  if (nd == 3) ds_argmin_k<3><<<grid, DS_T, 0, st>>>(cost, soft, coeff, idx, disp, B, g.S, r);
  else ds_argmin_k<2><<<grid, DS_T, 0, st>>>(cost, soft, coeff, idx, disp, B, g.S, r);
  DF_LAUNCH_CHECK();
  return 0;
}

extern "C" int dfmir_dsearch_smooth(int nd, const float* disp, float* out, int B, int D, int H, int W, void* stream) {
  DsGeom g;
  DF_ARG_CHECK(disp && out && disp != out);
  DF_ARG_CHECK(ds_geom(nd, B, 1, D, H, W, nd, &g));
  const long long n = (long long)B * nd * g.S;
  const unsigned grid = (unsigned)((n + DS_T - 1) / DS_T);
  hipStream_t st = (hipStream_t)stream;
  if (nd == 3) ds_smooth_k<3><<<grid, DS_T, 0, st>>>(disp, out, (long long)B * nd, g.D, H, W);
  else ds_smooth_k<2><<<grid, DS_T, 0, st>>>(disp, out, (long long)B * nd, 1, H, W);
  DF_LAUNCH_CHECK();
  return 0;
}
