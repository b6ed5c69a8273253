// Exact Euclidean distance transform of a label map and the Hausdorff distance of two label maps on top of it -- the
// reference's `HausdorffDistance` (util/loss_metrics.py:105-132: threshold, copy to the host, scipy's
// distance_transform_edt over the whole [B,1,*vol] array, maximum) without the host, per batch element and per label.
//
// d2(x) = min over voxels y of the set of |x - y|^2 as int32, separable: one pass per axis.
//   edt_row_k   the W pass.  A wave owns one row: it forms the set's membership (map == value, or the border predicate)
//               straight from the 8-bit map as ballot words -- no one-hot tensor, no float mask, no LDS -- and every lane
//               finds the nearest member at or below and at or above its x with a count of leading / trailing zeros:
//               g(x) = (x - x')^2, EDT_INF when the row has none.
//   edt_line_k  the H and D passes: d(i) = min_j prev(j) + (i - j)^2 per line.  A workgroup stages EDT_TW = 64 W-columns x
//               the full line of the pass axis in LDS (64 n int32 <= 64 KiB at n = 256), so global reads and writes stay
//               coalesced along W whichever axis the pass runs along; a thread widens r = 1, 2, .. from i and stops once
//               r^2 >= best (no j further out can improve it): exact, and short wherever the set is near.  prev <= EDT_INF =
//               2^29 and r^2 < 2^16, so every sum stays below 2^31; the minimum starts at prev(i) <= EDT_INF, so results
//               clamp to the sentinel by construction.  MODE 0 stores in place (the tile is read completely before the
//               barrier and tiles are disjoint); MODE 1 is the LAST pass of a Hausdorff direction: it evaluates only the
//               voxels of the source set and feeds, per (direction, b, label), a count, an integer atomicMax of d2 and --
//               when asked -- an int32 histogram over d2 with bins 0 .. sum (n_i - 1)^2.  d2 = 0 (the bulk, where the
//               structures overlap) is counted in a register and added once per wave, like the count and the maximum.
//               Integer atomics only: the results do not depend on the order of the workgroups.
//   edt_fin_k   one workgroup per (direction, b, label): nearest-rank percentile from the histogram, the mean of sqrt(d2)
//               in double (per-thread segments in index order, then the 256 partial sums in index order), and
//               hd = max over the directions (integer atomicMax on the bits of a non-negative float).
// Border sets (`surface`): a set voxel with a face neighbour outside the set or outside the volume; the z neighbours count
// only when D > 1, so a one-plane volume is the 2-D image it is.  Evaluated on the fly from the map in both roles.
//
// Labels are processed in chunks of EDT_CHUNK = 4, both directions of a chunk in one launch (grid.z): the scratch is
// 2 x 4 int32 volumes per batch element plus the chunk's statistics and histograms and does not grow with K.  At
// 1 x 160 x 192 x 224: 220 200 960 bytes of distance buffers + 3 567 808 of histograms and counters = 223 768 768 bytes.
// Supported extents: every axis <= EDT_MAXN = 256 (the LDS tile of the line pass; the ballot words of the W pass).
#include "common.h"

namespace {

constexpr int EDT_THREADS = 256;
constexpr int EDT_TW = 64;                    // W-columns of a line-pass tile (one wave = one line position)
constexpr int EDT_MAXN = 256;                 // largest extent of any axis
constexpr int EDT_CHUNK = 4;                  // labels per launch
constexpr int EDT_MAXK = 64;
constexpr int EDT_INF = DFMIR_EDT_SQ_INF;
constexpr int EDT_QMAX = 100000;              // percentile 100 in thousandths

struct EdtGeom {
  int B, D, H, W;
  int C;                                      // labels of this launch; grid.z = directions * C
  unsigned vals;                              // their values, 8 bits each
  int surface;
};

__device__ __forceinline__ int edt_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}
__device__ __forceinline__ int edt_wave_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_down(v, o, 64));
  return v;
}

// Is voxel (z, y, x) of the map `m` [D][H][W] in the set of `val` (surface: in its border)?
__device__ __forceinline__ bool edt_member(const uint8_t* __restrict__ m, const EdtGeom& g, int z, int y, int x, int val) {
  const long long HW = (long long)g.H * g.W;
  const uint8_t* p = m + (long long)z * HW + (long long)y * g.W + x;
  if (*p != val) return false;
  if (!g.surface) return true;
  bool inner = x > 0 && x < g.W - 1 && y > 0 && y < g.H - 1 && p[-1] == val && p[1] == val && p[-g.W] == val && p[g.W] == val;
  if (g.D > 1) inner = inner && z > 0 && z < g.D - 1 && p[-HW] == val && p[HW] == val;
  return !inner;
}

__global__ __launch_bounds__(EDT_THREADS) void edt_zero_k(int* __restrict__ p, long long n) {
  for (long long i = (long long)blockIdx.x * EDT_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * EDT_THREADS) p[i] = 0;
}

// grid (ceil(D H / 4), B, directions * C).  Direction 0 measures distances TO the set of `mb`, direction 1 to that of `ma`.
__global__ __launch_bounds__(EDT_THREADS) void edt_row_k(const uint8_t* __restrict__ ma, const uint8_t* __restrict__ mb,
                                                        EdtGeom g, int* __restrict__ buf) {
  constexpr int NW = EDT_MAXN / 64;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int b = blockIdx.y, s = blockIdx.z;
  const int dir = s / g.C, val = (int)((g.vals >> (8 * (s % g.C))) & 255u);
  const int rows = g.D * g.H;
  const int row = (int)blockIdx.x * (EDT_THREADS / 64) + wave;
  if (row >= rows) return;                     // (a whole wave: the ballots below stay convergent)
  const int z = row / g.H, y = row - z * g.H;
  const long long S = (long long)rows * g.W;
  const uint8_t* tgt = (dir == 0 ? mb : ma) + (long long)b * S;
  unsigned long long w[NW];                    // bit x % 64 of w[x / 64]: voxel x of the row is in the set (wave-uniform)
#pragma unroll
  for (int c = 0; c < NW; ++c) {
    const int x = c * 64 + lane;
    bool in_set = false;
    if (x < g.W) in_set = edt_member(tgt, g, z, y, x, val);
    w[c] = __ballot(in_set);
  }
  int* out = buf + ((long long)s * g.B + b) * S + (long long)row * g.W;
#pragma unroll
  for (int c = 0; c < NW; ++c) {
    const int x = c * 64 + lane;
    if (x >= g.W) continue;
    int left = -1, right = -1;                 // the nearest members at or below x, at or above x
    unsigned long long m = w[c] & (~0ull >> (63 - lane));
    if (m) {
      left = c * 64 + 63 - __clzll((long long)m);
    } else {
#pragma unroll
      for (int cc = c - 1; cc >= 0; --cc)
        if (left < 0 && w[cc]) left = cc * 64 + 63 - __clzll((long long)w[cc]);
    }
    m = w[c] & (~0ull << lane);
    if (m) {
      right = c * 64 + __ffsll((long long)m) - 1;
    } else {
#pragma unroll
      for (int cc = c + 1; cc < NW; ++cc)
        if (right < 0 && w[cc]) right = cc * 64 + __ffsll((long long)w[cc]) - 1;
    }
    int best = EDT_INF;
    if (left >= 0) best = (x - left) * (x - left);
    if (right >= 0) best = min(best, (right - x) * (right - x));
    out[x] = best;
  }
}

// grid (outer * ceil(W / 64), B, directions * C); dynamic LDS: n * EDT_TW ints.  along_z = 0: the H pass (n = H, outer = z);
// along_z = 1: the D pass (n = D, outer = y).  MODE 1: direction 0 evaluates the voxels of `ma`'s set, direction 1 of `mb`'s.
template <int MODE>
__global__ __launch_bounds__(EDT_THREADS) void edt_line_k(int* __restrict__ buf, EdtGeom g, int n, int along_z,
                                                         const uint8_t* __restrict__ ma, const uint8_t* __restrict__ mb,
                                                         int* __restrict__ stats, int* __restrict__ hist, int maxd2,
                                                         int need_hist) {
  extern __shared__ int tile[];                // [n][EDT_TW]
  const int ntw = (g.W + EDT_TW - 1) / EDT_TW;
  const int o = (int)blockIdx.x / ntw, x0 = ((int)blockIdx.x - o * ntw) * EDT_TW;
  const int b = blockIdx.y, s = blockIdx.z;
  const long long HW = (long long)g.H * g.W, S = HW * g.D;
  const long long lstride = along_z ? HW : (long long)g.W;
  const long long ostride = along_z ? (long long)g.W : HW;
  int* base = buf + ((long long)s * g.B + b) * S + (long long)o * ostride + x0;
  const int c = threadIdx.x & (EDT_TW - 1), i0 = threadIdx.x >> 6;
  const bool colok = x0 + c < g.W;
  for (int j = i0; j < n; j += EDT_THREADS / 64) tile[j * EDT_TW + c] = colok ? base[(long long)j * lstride + c] : EDT_INF;
  __syncthreads();
  const int dir = s / g.C, val = (int)((g.vals >> (8 * (s % g.C))) & 255u);
  const uint8_t* src = MODE == 1 ? (dir == 0 ? ma : mb) + (long long)b * S : nullptr;
  const long long slot = (long long)s * g.B + b;
  int cnt = 0, zeros = 0, mx = 0;
  for (int i = i0; i < n; i += EDT_THREADS / 64) {         // (i is the same in every lane of a wave)
    const bool on = colok && (MODE == 0 || edt_member(src, g, along_z ? i : o, along_z ? o : i, x0 + c, val));
    int best = 0;
    if (on) {
      best = tile[i * EDT_TW + c];
      const int rmax = max(i, n - 1 - i);
      for (int r = 1; r <= rmax; ++r) {
        const int rr = r * r;
        if (rr >= best) break;
        const int lo = i - r >= 0 ? tile[(i - r) * EDT_TW + c] : EDT_INF;
        const int hi = i + r < n ? tile[(i + r) * EDT_TW + c] : EDT_INF;
        best = min(best, min(lo, hi) + rr);
      }
      if (MODE == 0) {
        base[(long long)i * lstride + c] = best;
      } else {
        ++cnt;
        mx = max(mx, best);
        if (need_hist) {
          if (best == 0) ++zeros;
          else if (best <= maxd2) atomicAdd(&hist[slot * ((long long)maxd2 + 1) + best], 1);   // (EDT_INF has no bin)
        }
      }
    }
  }
  if (MODE == 1) {
    cnt = edt_wave_sum(cnt);
    zeros = edt_wave_sum(zeros);
    mx = edt_wave_max(mx);
    if ((threadIdx.x & 63) == 0 && cnt) {
      atomicAdd(&stats[2 * slot], cnt);
      atomicMax(&stats[2 * slot + 1], mx);
      if (need_hist && zeros) atomicAdd(&hist[slot * ((long long)maxd2 + 1)], zeros);
    }
  }
}

// grid (2 C, B).  stats / hist: the chunk's, slot = (dir * C + kc) * B + b.  Outputs are indexed by the label's position
// k0 + kc in the caller's list.
__global__ __launch_bounds__(EDT_THREADS) void edt_fin_k(const int* __restrict__ stats, const int* __restrict__ hist,
                                                        int maxd2, int B, int C, int K, int k0, int qm, int need_hist,
                                                        float* __restrict__ hd, float* __restrict__ directed,
                                                        float* __restrict__ mean, int* __restrict__ d2out) {
  __shared__ long long csum[EDT_THREADS];
  __shared__ double msum[EDT_THREADS];
  const int s = blockIdx.x, b = blockIdx.y, dir = s / C, kc = s - dir * C;
  const long long slot = (long long)s * B + b, other = (long long)((1 - dir) * C + kc) * B + b;
  const int n = stats[2 * slot], mx = stats[2 * slot + 1];
  const bool empty = n == 0 || stats[2 * other] == 0;
  const int len = (empty || !need_hist) ? 0 : min(mx, maxd2) + 1;
  const int seg = (len + EDT_THREADS - 1) / EDT_THREADS;
  const int* hp = hist + slot * ((long long)maxd2 + 1);
  const int lo = min((int)threadIdx.x * seg, len), hi = min(lo + seg, len);
  long long cs = 0;
  double ms = 0.0;
  for (int d = lo; d < hi; ++d) {
    const int h = hp[d];
    cs += h;
    if (mean && h) ms += (double)h * sqrt((double)d);
  }
  csum[threadIdx.x] = cs;
  msum[threadIdx.x] = ms;
  __syncthreads();
  if (threadIdx.x) return;
  const float inf = __uint_as_float(0x7f800000u);
  int d2q = EDT_INF;
  float dv = inf, mv = inf;
  if (!empty) {
    d2q = mx;
    if (qm < EDT_QMAX) {                                   // nearest rank: the smallest d2 whose cumulative count reaches r
      long long r = ((long long)qm * n + (EDT_QMAX - 1)) / EDT_QMAX;
      if (r < 1) r = 1;
      long long cum = 0;
      int t = 0;
      while (t < EDT_THREADS - 1 && cum + csum[t] < r) cum += csum[t++];
      int d = t * seg;
      for (; d < len; ++d) {
        cum += hp[d];
        if (cum >= r) break;
      }
      d2q = d < len ? d : len - 1;
    }
    dv = (float)sqrt((double)d2q);
    if (mean) {
      double tot = 0.0;
      for (int t = 0; t < EDT_THREADS; ++t) tot += msum[t];
      mv = (float)(tot / (double)n);
    }
  }
  const long long oi = ((long long)dir * B + b) * K + k0 + kc;
  d2out[oi] = d2q;
  directed[oi] = dv;
  if (mean) mean[oi] = mv;
  atomicMax(reinterpret_cast<unsigned*>(hd) + (long long)b * K + k0 + kc, __float_as_uint(dv));
}

inline bool edt_geom_ok(int nd, int B, int D, int H, int W) {
  if ((nd != 2 && nd != 3) || B <= 0 || B > 65535 || D <= 0 || H <= 0 || W <= 0) return false;
  if (nd == 2 && D != 1) return false;
  return D <= EDT_MAXN && H <= EDT_MAXN && W <= EDT_MAXN;
}
inline int edt_maxd2(int D, int H, int W) { return (D - 1) * (D - 1) + (H - 1) * (H - 1) + (W - 1) * (W - 1); }
inline unsigned edt_line_grid(int outer, int W) { return (unsigned)(outer * ((W + EDT_TW - 1) / EDT_TW)); }

}  // namespace

extern "C" long long dfmir_label_hausdorff_ws_bytes(int nd, int B, int K, int D, int H, int W) {
  if (!edt_geom_ok(nd, B, D, H, W) || K < 1 || K > EDT_MAXK) return -1;
  const long long C = K < EDT_CHUNK ? K : EDT_CHUNK;
  const long long slots = 2 * C * B;
  return 4 * slots * ((long long)D * H * W + 2 + edt_maxd2(D, H, W) + 1);
}

extern "C" int dfmir_label_edt_sq(int nd, const unsigned char* map, int value, int surface, int B, int D, int H, int W,
                                  int* out, void* stream) {
  DF_ARG_CHECK(map && out && edt_geom_ok(nd, B, D, H, W) && value >= 0 && value <= 255);
  hipStream_t st = (hipStream_t)stream;
  const EdtGeom g{B, D, H, W, 1, (unsigned)value, surface ? 1 : 0};
  edt_row_k<<<dim3((unsigned)((D * H + 3) / 4), (unsigned)B, 1u), EDT_THREADS, 0, st>>>(nullptr, map, g, out);
  DF_LAUNCH_CHECK();
  edt_line_k<0><<<dim3(edt_line_grid(D, W), (unsigned)B, 1u), EDT_THREADS, (size_t)H * EDT_TW * sizeof(int), st>>>(
      out, g, H, 0, nullptr, nullptr, nullptr, nullptr, 0, 0);
  DF_LAUNCH_CHECK();
  if (D > 1) {
    edt_line_k<0><<<dim3(edt_line_grid(H, W), (unsigned)B, 1u), EDT_THREADS, (size_t)D * EDT_TW * sizeof(int), st>>>(
        out, g, D, 1, nullptr, nullptr, nullptr, nullptr, 0, 0);
    DF_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int dfmir_label_hausdorff(int nd, const unsigned char* a, const unsigned char* b, const unsigned char* labels,
                                     int K, int B, int D, int H, int W, int qm, int flags, void* ws, float* hd,
                                     float* directed, float* mean, int* d2, void* stream) {
  DF_ARG_CHECK(a && b && labels && ws && hd && directed && d2 && edt_geom_ok(nd, B, D, H, W) && K >= 1 && K <= EDT_MAXK);
  DF_ARG_CHECK(qm >= 1 && qm <= EDT_QMAX && (flags & ~DFMIR_HD_SURFACE) == 0 && (reinterpret_cast<uintptr_t>(ws) & 3) == 0);
  hipStream_t st = (hipStream_t)stream;
  const int need_hist = (qm < EDT_QMAX || mean) ? 1 : 0;
  const int maxd2 = edt_maxd2(D, H, W);
  const long long S = (long long)D * H * W;
  const int Cmax = K < EDT_CHUNK ? K : EDT_CHUNK;
  int* buf = reinterpret_cast<int*>(ws);
  int* stats = buf + 2LL * Cmax * B * S;
  int* hist = stats + 4LL * Cmax * B;                      // (directly behind the counters: one zero fill covers both)
  edt_zero_k<<<df_grid((long long)B * K, EDT_THREADS, 2048), EDT_THREADS, 0, st>>>(reinterpret_cast<int*>(hd), (long long)B * K);
  DF_LAUNCH_CHECK();
  for (int k0 = 0; k0 < K; k0 += EDT_CHUNK) {
    const int C = K - k0 < EDT_CHUNK ? K - k0 : EDT_CHUNK;
    unsigned vals = 0;
    for (int i = 0; i < C; ++i) vals |= (unsigned)labels[k0 + i] << (8 * i);
    const EdtGeom g{B, D, H, W, C, vals, (flags & DFMIR_HD_SURFACE) ? 1 : 0};
    const long long nz = 4LL * Cmax * B + (need_hist ? 2LL * C * B * ((long long)maxd2 + 1) : 0);
    edt_zero_k<<<df_grid(nz, EDT_THREADS, 2048), EDT_THREADS, 0, st>>>(stats, nz);
    DF_LAUNCH_CHECK();
    const unsigned gz = 2u * (unsigned)C;
    edt_row_k<<<dim3((unsigned)((D * H + 3) / 4), (unsigned)B, gz), EDT_THREADS, 0, st>>>(a, b, g, buf);
    DF_LAUNCH_CHECK();
    if (D > 1) {
      edt_line_k<0><<<dim3(edt_line_grid(D, W), (unsigned)B, gz), EDT_THREADS, (size_t)H * EDT_TW * sizeof(int), st>>>(
          buf, g, H, 0, nullptr, nullptr, nullptr, nullptr, 0, 0);
      DF_LAUNCH_CHECK();
      edt_line_k<1><<<dim3(edt_line_grid(H, W), (unsigned)B, gz), EDT_THREADS, (size_t)D * EDT_TW * sizeof(int), st>>>(
          buf, g, D, 1, a, b, stats, hist, maxd2, need_hist);
    } else {
      edt_line_k<1><<<dim3(edt_line_grid(1, W), (unsigned)B, gz), EDT_THREADS, (size_t)H * EDT_TW * sizeof(int), st>>>(
          buf, g, H, 0, a, b, stats, hist, maxd2, need_hist);
    }
    DF_LAUNCH_CHECK();
    edt_fin_k<<<dim3(gz, (unsigned)B), EDT_THREADS, 0, st>>>(stats, hist, maxd2, B, C, K, k0, qm, need_hist, hd, directed,
                                                           mean, d2);
    DF_LAUNCH_CHECK();
  }
  return 0;
}
