// Dice losses for segmentation-supervised registration, and vxm MSE.
//
// dfmir_warp_dice_*: the Dice of a FIXED label map against a MOVING label map warped by a flow, per scored label -- vxm
// `Dice().loss(one_hot(fix)[:, labels], SpatialTransformer(one_hot(mov)[:, labels], flow))`
// (models/voxelmorph/torchvoxelmorph/losses.py:79-90, layers.py:36-48; the label warp of test.py:80-81 in nearest mode)
// without ever forming a one-hot tensor.  An output voxel touches <= 2^nd corner labels of the moving map and one label
// of the fixed map, so everything the loss needs is three sums per (batch, label):
//   T = sum_x sum_k w_k [mov(c_k) = l] [fix(x) = l],  S = sum_x sum_k w_k [mov(c_k) = l],  N = #{x : fix(x) = l}.
// warp_dice_fwd_k: a thread owns 4 voxels along W (16-byte flow loads; one voxel when W % 4 != 0), merges the corners of
// a voxel that carry the same label, and adds the merged weight to its workgroup's [3][K] table in LDS as 64-bit FIXED
// POINT (quantum 2^-32: every multi-linear weight >= 2^-9 converts exactly, smaller ones to within 2^-33) -- integer
// addition is associative, so neither the order of the LDS atomics nor the order of the workgroups can change a bit.
// Every workgroup stores its table to its own workspace slot (no global atomics); warp_dice_fin_k adds the slots and
// writes dice[B][K], the loss and the two gradient seeds per (b, l):
//   gT = -2 / (bottom B K),  gS = 2 T / (bottom^2 B K) where the clamp(min=1e-5) of the denominator is inactive, else 0.
// warp_dice_bwd_k is a pure gather: d loss / d flow_a(x) = sum_k dw_k/dp_a (gT[m_k] [m_k = fix(x)] + gS[m_k]), m_k the
// label of corner k -- the flow gradient of a warp whose corner "values" come from the seed table in LDS.
// nd = 2 runs the 3-D code with D = 1 and no z displacement (wz0 = 1, the z + 1 corners are out of the volume).
//
// dfmir_dice_* / dfmir_mse_*: the dense vxm Dice and MSE of float tensors; per-workgroup partial sums in a fixed tree,
// added in index order by a finaliser (bit-reproducible), element-wise backward.
#include "lin_cell.h"

namespace {

constexpr int WD_THREADS = 256;
constexpr int WD_MAXWG = 1024;                // workgroups (= partial slots) per batch element at most
constexpr int WD_FIN_GROUPS = 16;             // the finaliser: 16 groups of 64 threads share the slots of a label
constexpr int WD_MAXK = 64;
constexpr float WD_FX = 4294967296.f;         // 2^32
constexpr double WD_FX_INV = 1.0 / 4294967296.0;
constexpr float DICE_MIN = 1e-5f;             // torch.clamp(..., min=1e-5) of the denominator

typedef unsigned long long u64;

inline int wd_vec(int W) { return (W & 3) == 0 ? 4 : 1; }
inline int wd_nwg(long long S, int W) {
  const long long items = S / wd_vec(W);
  long long w = (items + 2 * WD_THREADS - 1) / (2 * WD_THREADS);     // >= 2 items per thread
  return (int)(w < 1 ? 1 : (w > WD_MAXWG ? WD_MAXWG : w));
}

struct WdGeom {
  int nd, B, K, D, H, W;
};

__device__ __forceinline__ u64 wd_fx(float w) { return (u64)__float2ull_rn(w * WD_FX); }

// One output voxel p = (z, y, x) of batch element b, displaced by u: the slots and upper weights of its corners.  (Mode 1
// of the forward does not come here: it takes the rounded corner alone.)
struct WdCorners {
  int c[8];        // slot of corner k (255: out of the volume or not scored); k = 4 dz + 2 dy + dx
  float w1[3];
};
__device__ __forceinline__ void wd_corners(const uint8_t* __restrict__ mb, const uint8_t* slot, const WdGeom& g,
                                           const int (&p)[3], const float (&u)[3], WdCorners& o) {
  const int n[3] = {g.D, g.H, g.W};
  LinCell<3> q;
  lin_cell<3, int>(p, u, n, q);
#pragma unroll
  for (int a = 0; a < 3; ++a) o.w1[a] = q.w1[a];
#pragma unroll
  for (int k = 0; k < 8; ++k) o.c[k] = q.in(k) ? (int)slot[mb[q.off(k)]] : 255;
}

template <int VEC>
__global__ __launch_bounds__(WD_THREADS) void warp_dice_fwd_k(const uint8_t* __restrict__ mov,
                                                             const uint8_t* __restrict__ fix,
                                                             const float* __restrict__ flow,
                                                             const uint8_t* __restrict__ slot_of, WdGeom g, int mode,
                                                             u64* __restrict__ part) {
  __shared__ u64 acc[3 * WD_MAXK];            // T, S, N
  __shared__ uint8_t slot[256];
  for (int i = threadIdx.x; i < 3 * WD_MAXK; i += WD_THREADS) acc[i] = 0;
  for (int i = threadIdx.x; i < 256; i += WD_THREADS) slot[i] = slot_of[i];
  __syncthreads();
  const int b = blockIdx.y;
  const long long S = (long long)g.D * g.H * g.W;
  const unsigned Wv = (unsigned)g.W / VEC;
  const unsigned items = (unsigned)(S / VEC);
  const uint8_t* mb = mov + (long long)b * S;
  const uint8_t* fb = fix + (long long)b * S;
  const float* fl = flow + (long long)b * g.nd * S;
  for (unsigned it = blockIdx.x * WD_THREADS + threadIdx.x; it < items; it += gridDim.x * WD_THREADS) {
    const unsigned row = it / Wv;
    const int x0 = (int)(it - row * Wv) * VEC;
    const unsigned zq = row / (unsigned)g.H;
    const int y = (int)(row - zq * (unsigned)g.H), z = (int)zq;
    const long long sp = (long long)it * VEC;
    float dz[VEC], dy[VEC], dx[VEC];
    int fl_lab[VEC];
    if (VEC == 4) {
      const float4 vy = *reinterpret_cast<const float4*>(fl + (long long)(g.nd - 2) * S + sp);
      const float4 vx = *reinterpret_cast<const float4*>(fl + (long long)(g.nd - 1) * S + sp);
      float4 vz = make_float4(0.f, 0.f, 0.f, 0.f);
      if (g.nd == 3) vz = *reinterpret_cast<const float4*>(fl + sp);
      const uchar4 f4 = *reinterpret_cast<const uchar4*>(fb + sp);
      dz[0] = vz.x; dz[VEC > 1 ? 1 : 0] = vz.y; dz[VEC > 2 ? 2 : 0] = vz.z; dz[VEC > 3 ? 3 : 0] = vz.w;
      dy[0] = vy.x; dy[VEC > 1 ? 1 : 0] = vy.y; dy[VEC > 2 ? 2 : 0] = vy.z; dy[VEC > 3 ? 3 : 0] = vy.w;
      dx[0] = vx.x; dx[VEC > 1 ? 1 : 0] = vx.y; dx[VEC > 2 ? 2 : 0] = vx.z; dx[VEC > 3 ? 3 : 0] = vx.w;
      fl_lab[0] = f4.x; fl_lab[VEC > 1 ? 1 : 0] = f4.y; fl_lab[VEC > 2 ? 2 : 0] = f4.z; fl_lab[VEC > 3 ? 3 : 0] = f4.w;
    } else {
      dz[0] = g.nd == 3 ? fl[sp] : 0.f;
      dy[0] = fl[(long long)(g.nd - 2) * S + sp];
      dx[0] = fl[(long long)(g.nd - 1) * S + sp];
      fl_lab[0] = fb[sp];
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const float fz = (float)z + dz[e], fy = (float)y + dy[e], fx = (float)(x0 + e) + dx[e];
      const int sf = slot[fl_lab[e]];
      if (sf != 255) atomicAdd(&acc[2 * WD_MAXK + sf], (u64)1);
      if (mode == 1) {
        const int zz = (int)nearbyintf(fz), yy = (int)nearbyintf(fy), xx = (int)nearbyintf(fx);
        const bool v = (unsigned)zz < (unsigned)g.D && (unsigned)yy < (unsigned)g.H && (unsigned)xx < (unsigned)g.W;
        const int c = v ? (int)slot[mb[((long long)zz * g.H + yy) * g.W + xx]] : 255;
        if (c != 255) {
          atomicAdd(&acc[WD_MAXK + c], (u64)1 << 32);
          if (c == sf) atomicAdd(&acc[c], (u64)1 << 32);
        }
        continue;
      }
      WdCorners o;
      wd_corners(mb, slot, g, {z, y, x0 + e}, {dz[e], dy[e], dx[e]}, o);
      float w[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) w[k] = lin_cw<3>(o.w1, k);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if (o.c[k] == 255) continue;
        float ws = w[k];                       // corners of one voxel with one label: one add (fixed order k, j)
#pragma unroll
        for (int j = k + 1; j < 8; ++j)
          if (o.c[j] == o.c[k]) { ws += w[j]; o.c[j] = 255; }
        const u64 q = wd_fx(ws);
        atomicAdd(&acc[WD_MAXK + o.c[k]], q);
        if (o.c[k] == sf) atomicAdd(&acc[o.c[k]], q);
      }
    }
  }
  __syncthreads();
  u64* p = part + ((long long)b * gridDim.x + blockIdx.x) * 3 * g.K;
  for (int i = threadIdx.x; i < 3 * g.K; i += WD_THREADS) p[i] = acc[(i / g.K) * WD_MAXK + (i % g.K)];
}

// One workgroup: per batch element the slots are added (integers: any order gives the same bits), then thread l < K
// evaluates label l; the mean over (b, l) is added by thread 0 in index order.
__global__ __launch_bounds__(64 * WD_FIN_GROUPS) void warp_dice_fin_k(const u64* __restrict__ part, int nwg, int B, int K,
                                                             float* __restrict__ loss, float* __restrict__ dice,
                                                             float* __restrict__ seeds) {
  __shared__ u64 sums[WD_FIN_GROUPS][3 * WD_MAXK];
  __shared__ float dsum[WD_MAXK];
  const int l = threadIdx.x & 63, grp = threadIdx.x >> 6;     // grp: the group of 64 threads
  const float inv_bk = 1.f / ((float)B * (float)K);
  float mine = 0.f;
  for (int b = 0; b < B; ++b) {
    u64 t = 0, s = 0, n = 0;
    if (l < K) {
#pragma unroll 4
      for (int w = grp; w < nwg; w += WD_FIN_GROUPS) {
        const u64* p = part + ((long long)b * nwg + w) * 3 * K;
        t += p[l]; s += p[K + l]; n += p[2 * K + l];
      }
    }
    sums[grp][l] = t; sums[grp][WD_MAXK + l] = s; sums[grp][2 * WD_MAXK + l] = n;
    __syncthreads();
    if (grp == 0 && l < K) {
      for (int q = 1; q < WD_FIN_GROUPS; ++q) { t += sums[q][l]; s += sums[q][WD_MAXK + l]; n += sums[q][2 * WD_MAXK + l]; }
      const float T = (float)((double)t * WD_FX_INV);
      const float bs = (float)((double)n + (double)s * WD_FX_INV);
      const bool active = bs >= DICE_MIN;
      const float bottom = active ? bs : DICE_MIN;
      const float d = 2.f * T / bottom;
      dice[b * K + l] = d;
      seeds[b * K + l] = -2.f / bottom * inv_bk;
      seeds[(B + b) * K + l] = active ? 2.f * T / (bottom * bottom) * inv_bk : 0.f;
      mine += d;                               // (over b, in order)
    }
    __syncthreads();
  }
  if (grp == 0) dsum[l] = l < K ? mine : 0.f;
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot = 0.f;
    for (int i = 0; i < K; ++i) tot += dsum[i];
    loss[0] = -tot * inv_bk;
  }
}

template <int VEC>
__global__ __launch_bounds__(WD_THREADS) void warp_dice_bwd_k(const uint8_t* __restrict__ mov,
                                                             const uint8_t* __restrict__ fix,
                                                             const float* __restrict__ flow,
                                                             const uint8_t* __restrict__ slot_of, WdGeom g,
                                                             const float* __restrict__ seeds,
                                                             const float* __restrict__ gout, float* __restrict__ dflow) {
  __shared__ float sgT[WD_MAXK], sgS[WD_MAXK];
  __shared__ uint8_t slot[256];
  const int b = blockIdx.y;
  for (int i = threadIdx.x; i < WD_MAXK; i += WD_THREADS) {
    sgT[i] = i < g.K ? seeds[b * g.K + i] : 0.f;
    sgS[i] = i < g.K ? seeds[(g.B + b) * g.K + i] : 0.f;
  }
  for (int i = threadIdx.x; i < 256; i += WD_THREADS) slot[i] = slot_of[i];
  __syncthreads();
  const float go = gout[0];
  const long long S = (long long)g.D * g.H * g.W;
  const unsigned Wv = (unsigned)g.W / VEC;
  const unsigned items = (unsigned)(S / VEC);
  const uint8_t* mb = mov + (long long)b * S;
  const uint8_t* fb = fix + (long long)b * S;
  const float* fl = flow + (long long)b * g.nd * S;
  float* dfl = dflow + (long long)b * g.nd * S;
  for (unsigned it = blockIdx.x * WD_THREADS + threadIdx.x; it < items; it += gridDim.x * WD_THREADS) {
    const unsigned row = it / Wv;
    const int x0 = (int)(it - row * Wv) * VEC;
    const unsigned zq = row / (unsigned)g.H;
    const int y = (int)(row - zq * (unsigned)g.H), z = (int)zq;
    const long long sp = (long long)it * VEC;
    float dz[VEC], dy[VEC], dx[VEC], gz[VEC], gy[VEC], gx[VEC];
    int fl_lab[VEC];
    if (VEC == 4) {
      const float4 vy = *reinterpret_cast<const float4*>(fl + (long long)(g.nd - 2) * S + sp);
      const float4 vx = *reinterpret_cast<const float4*>(fl + (long long)(g.nd - 1) * S + sp);
      float4 vz = make_float4(0.f, 0.f, 0.f, 0.f);
      if (g.nd == 3) vz = *reinterpret_cast<const float4*>(fl + sp);
      const uchar4 f4 = *reinterpret_cast<const uchar4*>(fb + sp);
      dz[0] = vz.x; dz[VEC > 1 ? 1 : 0] = vz.y; dz[VEC > 2 ? 2 : 0] = vz.z; dz[VEC > 3 ? 3 : 0] = vz.w;
      dy[0] = vy.x; dy[VEC > 1 ? 1 : 0] = vy.y; dy[VEC > 2 ? 2 : 0] = vy.z; dy[VEC > 3 ? 3 : 0] = vy.w;
      dx[0] = vx.x; dx[VEC > 1 ? 1 : 0] = vx.y; dx[VEC > 2 ? 2 : 0] = vx.z; dx[VEC > 3 ? 3 : 0] = vx.w;
      fl_lab[0] = f4.x; fl_lab[VEC > 1 ? 1 : 0] = f4.y; fl_lab[VEC > 2 ? 2 : 0] = f4.z; fl_lab[VEC > 3 ? 3 : 0] = f4.w;
    } else {
      dz[0] = g.nd == 3 ? fl[sp] : 0.f;
      dy[0] = fl[(long long)(g.nd - 2) * S + sp];
      dx[0] = fl[(long long)(g.nd - 1) * S + sp];
      fl_lab[0] = fb[sp];
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const int sf = slot[fl_lab[e]];
      WdCorners o;
      wd_corners(mb, slot, g, {z, y, x0 + e}, {dz[e], dy[e], dx[e]}, o);
      float v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int c = o.c[k];
        v[k] = c == 255 ? 0.f : (c == sf ? sgT[c] : 0.f) + sgS[c];
      }
      float d[3];
      lin_flow_grad<3>(v, o.w1, d);
      gz[e] = go * d[0];
      gy[e] = go * d[1];
      gx[e] = go * d[2];
    }
    if (VEC == 4) {
      if (g.nd == 3)
        *reinterpret_cast<float4*>(dfl + sp) = make_float4(gz[0], gz[VEC > 1 ? 1 : 0], gz[VEC > 2 ? 2 : 0], gz[VEC > 3 ? 3 : 0]);
      *reinterpret_cast<float4*>(dfl + (long long)(g.nd - 2) * S + sp) =
          make_float4(gy[0], gy[VEC > 1 ? 1 : 0], gy[VEC > 2 ? 2 : 0], gy[VEC > 3 ? 3 : 0]);
      *reinterpret_cast<float4*>(dfl + (long long)(g.nd - 1) * S + sp) =
          make_float4(gx[0], gx[VEC > 1 ? 1 : 0], gx[VEC > 2 ? 2 : 0], gx[VEC > 3 ? 3 : 0]);
    } else {
      if (g.nd == 3) dfl[sp] = gz[0];
      dfl[(long long)(g.nd - 2) * S + sp] = gy[0];
      dfl[(long long)(g.nd - 1) * S + sp] = gx[0];
    }
  }
}

inline bool wd_geom_ok(int nd, int B, int K, int D, int H, int W) {
  if ((nd != 2 && nd != 3) || B <= 0 || B > 65535 || K < 1 || K > WD_MAXK || D <= 0 || H <= 0 || W <= 0) return false;
  if (nd == 2 && D != 1) return false;
  return (long long)D * H * W < 0x7FFFFFFFLL;
}
inline bool wd_vec_ok(int W, const void* a, const void* b, const void* c) {
  return (W & 3) == 0 &&
         ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0 && (reinterpret_cast<uintptr_t>(c) & 3) == 0;
}

// ------------------------------------------------------------------------------------------ dense Dice / MSE
constexpr int DN_THREADS = 256;
constexpr int DN_MAXCHUNK = 512;
inline int dn_chunks(long long S) {
  long long c = (S + 8191) / 8192;
  return (int)(c < 1 ? 1 : (c > DN_MAXCHUNK ? DN_MAXCHUNK : c));
}

// KIND 0: (sum t p, sum (t + p)) of chunk blockIdx.x of plane blockIdx.y; KIND 1: (sum (t - p)^2, -).  part[plane][chunk][2]
template <int KIND, int VEC>
__global__ __launch_bounds__(DN_THREADS) void dense_sums_k(const float* __restrict__ t, const float* __restrict__ p,
                                                          long long S, float* __restrict__ part) {
  __shared__ float sm[17];
  const long long items = S / VEC;
  const long long per = (items + gridDim.x - 1) / gridDim.x;
  const long long lo = per * blockIdx.x, hi = lo + per < items ? lo + per : items;
  const float* tb = t + (long long)blockIdx.y * S;
  const float* pb = p + (long long)blockIdx.y * S;
  float a = 0.f, s = 0.f;
  for (long long i = lo + threadIdx.x; i < hi; i += DN_THREADS) {
    float tv[VEC], pv[VEC];
    if (VEC == 4) {
      const float4 x = *reinterpret_cast<const float4*>(tb + 4 * i), y = *reinterpret_cast<const float4*>(pb + 4 * i);
      tv[0] = x.x; tv[VEC > 1 ? 1 : 0] = x.y; tv[VEC > 2 ? 2 : 0] = x.z; tv[VEC > 3 ? 3 : 0] = x.w;
      pv[0] = y.x; pv[VEC > 1 ? 1 : 0] = y.y; pv[VEC > 2 ? 2 : 0] = y.z; pv[VEC > 3 ? 3 : 0] = y.w;
    } else {
      tv[0] = tb[i]; pv[0] = pb[i];
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      if (KIND == 0) { a += tv[e] * pv[e]; s += tv[e] + pv[e]; }
      else { const float d = tv[e] - pv[e]; a += d * d; }
    }
  }
  a = block_sum(a, sm);
  if (KIND == 0) s = block_sum(s, sm);
  if (threadIdx.x == 0) {
    float* o = part + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * 2;
    o[0] = a; o[1] = s;
  }
}

// coef[plane] = (ca, cb): d loss / d p = ca t + cb, d loss / d t = ca p + cb
__global__ __launch_bounds__(DN_THREADS) void dice_fin_k(const float* __restrict__ part, int chunks, int planes,
                                                        float* __restrict__ coef, float* __restrict__ out) {
  __shared__ float sm[17];
  float mine = 0.f;
  const float inv = 1.f / (float)planes;
  for (int pl = threadIdx.x; pl < planes; pl += DN_THREADS) {
    float a = 0.f, s = 0.f;
    for (int c = 0; c < chunks; ++c) { a += part[((long long)pl * chunks + c) * 2]; s += part[((long long)pl * chunks + c) * 2 + 1]; }
    const bool active = s >= DICE_MIN;
    const float bottom = active ? s : DICE_MIN;
    mine += 2.f * a / bottom;
    coef[2 * pl] = -2.f / bottom * inv;
    coef[2 * pl + 1] = active ? 2.f * a / (bottom * bottom) * inv : 0.f;
  }
  mine = block_sum(mine, sm);
  if (threadIdx.x == 0) out[0] = -mine * inv;
}
__global__ __launch_bounds__(64) void mse_fin_k(const float* __restrict__ part, int chunks, float inv_n, float* __restrict__ out) {
  if (threadIdx.x) return;
  float a = 0.f;
  for (int c = 0; c < chunks; ++c) a += part[2 * c];
  out[0] = a * inv_n;
}
__global__ __launch_bounds__(DN_THREADS) void dice_bwd_k(const float* __restrict__ t, const float* __restrict__ p,
                                                        long long S, const float* __restrict__ coef,
                                                        const float* __restrict__ gout, float* __restrict__ dt,
                                                        float* __restrict__ dp) {
  const float go = gout[0], ca = go * coef[2 * blockIdx.y], cb = go * coef[2 * blockIdx.y + 1];
  const long long base = (long long)blockIdx.y * S;
  for (long long i = (long long)blockIdx.x * DN_THREADS + threadIdx.x; i < S; i += (long long)gridDim.x * DN_THREADS) {
    if (dt) dt[base + i] = ca * p[base + i] + cb;
    if (dp) dp[base + i] = ca * t[base + i] + cb;
  }
}
__global__ __launch_bounds__(DN_THREADS) void mse_bwd_k(const float* __restrict__ t, const float* __restrict__ p, long long n,
                                                       float two_inv_n, const float* __restrict__ gout,
                                                       float* __restrict__ dt, float* __restrict__ dp) {
  const float c = gout[0] * two_inv_n;
  for (long long i = (long long)blockIdx.x * DN_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * DN_THREADS) {
    const float d = c * (t[i] - p[i]);
    if (dt) dt[i] = d;
    if (dp) dp[i] = -d;
  }
}

inline bool dn_vec_ok(long long S, const void* a, const void* b) {
  return (S & 3) == 0 && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0;
}

}  // namespace

extern "C" long long dfmir_warp_dice_ws_floats(int nd, int B, int K, int D, int H, int W) {
  if (!wd_geom_ok(nd, B, K, D, H, W)) return -1;
  return 2LL * B * wd_nwg((long long)D * H * W, W) * 3 * K;             // 64-bit entries, two floats each
}

extern "C" int dfmir_warp_dice_fwd(int nd, const uint8_t* mov, const uint8_t* fix, const float* flow,
                                   const uint8_t* slot_of, int K, int B, int D, int H, int W, int mode, float* ws,
                                   float* loss, float* dice, float* seeds, void* stream) {
  DF_ARG_CHECK(mov && fix && flow && slot_of && ws && loss && dice && seeds && wd_geom_ok(nd, B, K, D, H, W));
  DF_ARG_CHECK((mode == 0 || mode == 1) && (reinterpret_cast<uintptr_t>(ws) & 7) == 0);
  hipStream_t st = (hipStream_t)stream;
  const WdGeom g{nd, B, K, D, H, W};
  const int nwg = wd_nwg((long long)D * H * W, W);
  u64* part = reinterpret_cast<u64*>(ws);
  const dim3 grid((unsigned)nwg, (unsigned)B);
  // (the slot count follows W alone, so the workspace query needs no pointers: an unaligned tensor takes the one-voxel
  // kernel on the same grid)
  if (wd_vec_ok(W, flow, flow, fix)) warp_dice_fwd_k<4><<<grid, WD_THREADS, 0, st>>>(mov, fix, flow, slot_of, g, mode, part);
  else warp_dice_fwd_k<1><<<grid, WD_THREADS, 0, st>>>(mov, fix, flow, slot_of, g, mode, part);
  DF_LAUNCH_CHECK();
  warp_dice_fin_k<<<1, 64 * WD_FIN_GROUPS, 0, st>>>(part, nwg, B, K, loss, dice, seeds);
  DF_LAUNCH_CHECK();
  return 0;
}

extern "C" int dfmir_warp_dice_bwd(int nd, const uint8_t* mov, const uint8_t* fix, const float* flow,
                                   const uint8_t* slot_of, int K, int B, int D, int H, int W, const float* seeds,
                                   const float* gout, float* dflow, void* stream) {
  DF_ARG_CHECK(mov && fix && flow && slot_of && seeds && gout && dflow && wd_geom_ok(nd, B, K, D, H, W));
  hipStream_t st = (hipStream_t)stream;
  const WdGeom g{nd, B, K, D, H, W};
  const long long S = (long long)D * H * W;
  if (wd_vec_ok(W, flow, dflow, fix)) {
    const dim3 grid(df_grid(S / 4, WD_THREADS, 4096), (unsigned)B);
    warp_dice_bwd_k<4><<<grid, WD_THREADS, 0, st>>>(mov, fix, flow, slot_of, g, seeds, gout, dflow);
  } else {
    const dim3 grid(df_grid(S, WD_THREADS, 4096), (unsigned)B);
    warp_dice_bwd_k<1><<<grid, WD_THREADS, 0, st>>>(mov, fix, flow, slot_of, g, seeds, gout, dflow);
  }
  DF_LAUNCH_CHECK();
  return 0;
}

extern "C" long long dfmir_dice_ws_floats(long long planes, long long S) {
  if (planes <= 0 || planes > 65535 || S <= 0) return -1;
  return planes * (2LL * dn_chunks(S) + 2);
}

extern "C" int dfmir_dice_fwd(const float* y_true, const float* y_pred, long long planes, long long S, float* ws,
                              float* out, void* stream) {
  DF_ARG_CHECK(y_true && y_pred && ws && out && planes > 0 && planes <= 65535 && S > 0);
  hipStream_t st = (hipStream_t)stream;
  const int chunks = dn_chunks(S);
  float* coef = ws;
  float* part = ws + 2 * planes;
  const dim3 grid((unsigned)chunks, (unsigned)planes);
  if (dn_vec_ok(S, y_true, y_pred)) dense_sums_k<0, 4><<<grid, DN_THREADS, 0, st>>>(y_true, y_pred, S, part);
  else dense_sums_k<0, 1><<<grid, DN_THREADS, 0, st>>>(y_true, y_pred, S, part);
  DF_LAUNCH_CHECK();
  dice_fin_k<<<1, DN_THREADS, 0, st>>>(part, chunks, (int)planes, coef, out);
  DF_LAUNCH_CHECK();
  return 0;
}

extern "C" int dfmir_dice_bwd(const float* y_true, const float* y_pred, long long planes, long long S, const float* ws,
                              const float* gout, float* d_true, float* d_pred, void* stream) {
  DF_ARG_CHECK(y_true && y_pred && ws && gout && planes > 0 && planes <= 65535 && S > 0);
  if (!d_true && !d_pred) return 0;
  const dim3 grid(df_grid(S, DN_THREADS * 4, 1024), (unsigned)planes);
  dice_bwd_k<<<grid, DN_THREADS, 0, (hipStream_t)stream>>>(y_true, y_pred, S, ws, gout, d_true, d_pred);
  DF_LAUNCH_CHECK();
  return 0;
}

extern "C" long long dfmir_mse_ws_floats(long long n) {
  if (n <= 0) return -1;
  return 2LL * dn_chunks(n);
}

extern "C" int dfmir_mse_fwd(const float* y_true, const float* y_pred, long long n, float* ws, float* out, void* stream) {
  DF_ARG_CHECK(y_true && y_pred && ws && out && n > 0);
  hipStream_t st = (hipStream_t)stream;
  const int chunks = dn_chunks(n);
  const dim3 grid((unsigned)chunks, 1u);
  if (dn_vec_ok(n, y_true, y_pred)) dense_sums_k<1, 4><<<grid, DN_THREADS, 0, st>>>(y_true, y_pred, n, ws);
  else dense_sums_k<1, 1><<<grid, DN_THREADS, 0, st>>>(y_true, y_pred, n, ws);
  DF_LAUNCH_CHECK();
  mse_fin_k<<<1, 64, 0, st>>>(ws, chunks, (float)(1.0 / (double)n), out);
  DF_LAUNCH_CHECK();
  return 0;
}

extern "C" int dfmir_mse_bwd(const float* y_true, const float* y_pred, long long n, const float* gout, float* d_true,
                             float* d_pred, void* stream) {
  DF_ARG_CHECK(y_true && y_pred && gout && n > 0);
  if (!d_true && !d_pred) return 0;
  mse_bwd_k<<<df_grid(n, DN_THREADS * 4, 4096), DN_THREADS, 0, (hipStream_t)stream>>>(
      y_true, y_pred, n, (float)(2.0 / (double)n), gout, d_true, d_pred);
  DF_LAUNCH_CHECK();
  return 0;
}
