// Affine pre-alignment: the dense flow of an affine transform with its adjoint, the fused affine-SSD system (value, gradient
// and Gauss-Newton matrix in ONE pass over the voxels) and a device-side Levenberg-Marquardt step, 2-D and 3-D.
// Build-defined (include/dfmir_hip.h, ops.affine_* and infer.affine_init state the definitions):
//
//   theta [B][ND][ND + 1] fp32 = [A | t] in CENTRED voxel coordinates, axis order (z,) y, x:  c_a = (n_a - 1) / 2,
//   q(x) = (x - c, 1),  y(x) = c + A (x - c) + t,  flow(x) = y(x) - x = (A - I)(x - c) + t  (formed like that: no
//   cancellation of the coordinate itself).  P = ND (ND + 1) parameters, flattened row-major (a, j).
//   e_c = M_c(y) - F_c,  r = sum_c e_c dM_c(y)  (ND),  G = sum_c dM_c dM_c^T  (ND x ND),  N_b = sum_x m  (S without a mask)
//   L_b = sum_x m mean_c e^2 / N_b,   g_b = (2 / (C N_b)) sum_x m r (x) q,   H_b = (2 / (C N_b)) sum_x m G (x) (q q^T)
//   M is sampled as warpssd.hip samples it (ws_sample.h: the same cell, guards and corner differences), at p + flow(x) with
//   the flow in the very arithmetic af_flow_k writes: affine_ssd(theta) and warp_ssd(affine_flow(theta)) see one cell.
//
//   af_flow_k      flow [B][ND][S] of theta; 16-byte stores when W % 4 == 0 and the tensor is aligned.
//   af_flow_bwd_k  dtheta[b][a][j] = sum_x dflow[b][a][x] q_j(x): a fixed number of workgroups per sample, sums in double per
//                  thread, an ordered workgroup sum, one row of P doubles per workgroup; af_flow_fin_k adds the rows in order.
//   af_sys_k       the hot path.  A fixed number of workgroups per sample, each walks chunks of AF_T voxels.  Per chunk, phase
//                  A: one voxel per lane -- q, the flow, the cell (once), the packed moving features gathered in groups of
//                  four channels, F read coalesced -- leaves the voxel's record in LDS: V = m (sum_c e^2, 1, r, the unique
//                  entries of G) and QQ = (q, 1, the unique products q_i q_j).  Every sum asked for is an entry of the outer
//                  product  sum_x V (x) QQ  (3-D: 11 x 10, of which H takes G x QQ = 60 -- both factors are symmetric, so the
//                  78 unique entries of H are among them -- g takes r x (q, 1) and the two scalars the column of 1).  Phase
//                  B: the columns of QQ are dealt to the four waves, a lane takes four voxels of the chunk and adds its
//                  wave's columns in double (fma of the converted factors: the products are exact).  A lane so carries
//                  NV * ceil(NQ / 4) running sums (33 in 3-D) in place of all of them, and the gather keeps its registers.
//                  Each wave reduces its sums and writes them to the workgroup's slab; no atomics.  Gradient-only mode
//                  (affine_ssd's autograd): V = m (sum e^2, 1, r), QQ = (q, 1).
//   af_fin_k       one workgroup: adds the slabs of each sample in a fixed order in double and scales: L, L_b, the
//                  batch-normalised gradient (k = 2 / (B C S), masked 2 m / (C sum_all m)), g_b and H_b.
//   af_lm_k        one wave per sample: the accept test, the <= 12 x 12 Cholesky solve in fp64 and the update of
//                  infer.affine_init's loop; all it needs is in its arguments.
// Every output is bit-identical from run to run.  Nothing syncs with the host or keeps state.
#include "ws_sample.h"

namespace {

constexpr int AF_T = 256;                    // threads per workgroup: 4 waves x 64 lanes
constexpr int AF_CHUNKS = 4;                 // af_sys_k: a workgroup has at least this many chunks before there are more workgroups
constexpr int AF_MAXBLK = 1024;              // af_sys_k: workgroups per sample at most
constexpr int AF_BWD_MAXBLK = 256;           // af_flow_bwd_k: workgroups per sample at most
constexpr int AF_LM_T = 64;
constexpr int AF_MAXP = 12;

inline int af_nblk(int S, int maxblk) {
  const long long per = (long long)AF_T * AF_CHUNKS;
  const long long n = (S + per - 1) / per;
  return (int)(n < 1 ? 1 : n > maxblk ? maxblk : n);
}

// theta of one sample as the kernels use it: A - I, t and the centre
template <int ND>
struct AfXf {
  float am[ND][ND], t[ND], c[ND];
};

template <int ND>
__device__ __forceinline__ void af_load(const float* __restrict__ th, const WsGeom& g, AfXf<ND>& x) {
#pragma unroll
  for (int a = 0; a < ND; ++a) {
#pragma unroll
    for (int j = 0; j < ND; ++j) x.am[a][j] = th[a * (ND + 1) + j] - (a == j ? 1.f : 0.f);
    x.t[a] = th[a * (ND + 1) + ND];
  }
  if (ND == 3) { x.c[0] = 0.5f * (float)(g.D - 1); x.c[1] = 0.5f * (float)(g.H - 1); x.c[2] = 0.5f * (float)(g.W - 1); }
  else { x.c[0] = 0.5f * (float)(g.H - 1); x.c[ND - 1] = 0.5f * (float)(g.W - 1); }
}

// voxel j of a sample -> its index per axis
template <int ND>
__device__ __forceinline__ void af_index(const WsGeom& g, unsigned j, int (&p)[ND]) {
  p[ND - 1] = (int)(j % (unsigned)g.W); j /= (unsigned)g.W;
  if (ND == 3) { p[1] = (int)(j % (unsigned)g.H); p[0] = (int)(j / (unsigned)g.H); }
  else p[0] = (int)j;
}

// q = p - c and the flow (A - I) q + t, added in the order j = 0, 1, .., then t
template <int ND>
__device__ __forceinline__ void af_disp(const AfXf<ND>& x, const int (&p)[ND], float (&q)[ND], float (&u)[ND]) {
#pragma unroll
  for (int a = 0; a < ND; ++a) q[a] = (float)p[a] - x.c[a];
#pragma unroll
  for (int a = 0; a < ND; ++a) {
    float s = x.am[a][0] * q[0];
#pragma unroll
    for (int j = 1; j < ND; ++j) s += x.am[a][j] * q[j];
    u[a] = s + x.t[a];
  }
}

template <int ND, int V>
__global__ __launch_bounds__(AF_T) void af_flow_k(const float* __restrict__ theta, float* __restrict__ flow, WsGeom g,
                                                  int nb) {
  const int b = (int)(blockIdx.x / (unsigned)nb);
  const unsigned blk = blockIdx.x - (unsigned)b * (unsigned)nb;
  const unsigned j0 = (blk * (unsigned)AF_T + threadIdx.x) * (unsigned)V;
  if (j0 >= (unsigned)g.S) return;                               // V == 4: S % 4 == 0, a quad lies inside as a whole
  AfXf<ND> x;
  af_load<ND>(theta + (long long)b * ND * (ND + 1), g, x);
  float* fb = flow + (long long)b * ND * g.S;
  float out[ND][V];
#pragma unroll
  for (int e = 0; e < V; ++e) {
    int p[ND];
    float q[ND], u[ND];
    af_index<ND>(g, j0 + e, p);
    af_disp<ND>(x, p, q, u);
#pragma unroll
    for (int a = 0; a < ND; ++a) out[a][e] = u[a];
  }
#pragma unroll
  for (int a = 0; a < ND; ++a) {
    if (V == 4) *reinterpret_cast<float4*>(fb + (long long)a * g.S + j0) = make_float4(out[a][0], out[a][1], out[a][2], out[a][3]);
    else fb[(long long)a * g.S + j0] = out[a][0];
  }
}

// part[(b nblk + blk) P + a (ND + 1) + j] = the workgroup's share of sum_x dflow[b][a][x] q_j(x)
template <int ND>
__global__ __launch_bounds__(AF_T) void af_flow_bwd_k(const float* __restrict__ dflow, WsGeom g, int nblk,
                                                      double* __restrict__ part) {
  constexpr int P = ND * (ND + 1);
  __shared__ double red[AF_T / 64];
  const int b = (int)(blockIdx.x / (unsigned)nblk);
  const unsigned blk = blockIdx.x - (unsigned)b * (unsigned)nblk;
  const float* db = dflow + (long long)b * ND * g.S;
  float c[ND];
  if (ND == 3) { c[0] = 0.5f * (float)(g.D - 1); c[1] = 0.5f * (float)(g.H - 1); c[2] = 0.5f * (float)(g.W - 1); }
  else { c[0] = 0.5f * (float)(g.H - 1); c[ND - 1] = 0.5f * (float)(g.W - 1); }
  double acc[ND][ND + 1];
#pragma unroll
  for (int a = 0; a < ND; ++a)
#pragma unroll
    for (int j = 0; j <= ND; ++j) acc[a][j] = 0.0;
  for (unsigned j = blk * (unsigned)AF_T + threadIdx.x; j < (unsigned)g.S; j += (unsigned)nblk * AF_T) {
    int p[ND];
    af_index<ND>(g, j, p);
#pragma unroll
    for (int a = 0; a < ND; ++a) {
      const double d = (double)db[(long long)a * g.S + j];
#pragma unroll
      for (int jj = 0; jj < ND; ++jj) acc[a][jj] = fma(d, (double)((float)p[jj] - c[jj]), acc[a][jj]);
      acc[a][ND] += d;
    }
  }
#pragma unroll
  for (int a = 0; a < ND; ++a)
#pragma unroll
    for (int j = 0; j <= ND; ++j) {
      const double s = block_sum_ordered<AF_T>(acc[a][j], red);
      if (threadIdx.x == 0) part[((long long)b * nblk + blk) * P + a * (ND + 1) + j] = s;
    }
}

// dtheta[b][e] = the rows of sample b added in workgroup order
__global__ __launch_bounds__(AF_LM_T) void af_flow_fin_k(const double* __restrict__ part, int nblk, int P,
                                                         float* __restrict__ dtheta) {
  const int b = blockIdx.x, e = threadIdx.x;
  if (e >= P) return;
  double s = 0.0;
  for (int i = 0; i < nblk; ++i) s += part[((long long)b * nblk + i) * P + e];
  dtheta[b * P + e] = (float)s;
}

// index of (a, b), a <= b, among the unique entries of a symmetric n x n matrix, row-major
__host__ __device__ constexpr int af_tri(int a, int b, int n) { return a * n - a * (a - 1) / 2 + (b - a); }
// column of QQ = (q_0 .. q_{n-1}, 1, q_i q_j for i <= j) that holds qe_i qe_j of the extended qe = (q, 1)
__host__ __device__ constexpr int af_qq(int i, int j, int n) {
  return (i == n && j == n) ? n : j == n ? i : i == n ? j : n + 1 + (i <= j ? af_tri(i, j, n) : af_tri(j, i, n));
}

// part[((b NQ + col) NV + v) nblk + blk] = the workgroup's share of sum_x V_v(x) QQ_col(x)   (see the head of the file)
template <int ND, bool FULL>
__global__ __launch_bounds__(AF_T) void af_sys_k(const float* __restrict__ mov, const float* __restrict__ fix,
                                                 const float* __restrict__ theta, const float* __restrict__ mask, WsGeom g,
                                                 double* __restrict__ part) {
  constexpr int NC = 1 << ND;
  constexpr int NG = ND * (ND + 1) / 2;
  constexpr int NV = 2 + ND + (FULL ? NG : 0);
  constexpr int NQ = FULL ? (ND + 1) * (ND + 2) / 2 : ND + 1;
  constexpr int NW = AF_T / 64;
  constexpr int CPW = (NQ + NW - 1) / NW;                        // columns of QQ per wave
  __shared__ float rec[(NV + NQ) * AF_T];
  const int b = (int)(blockIdx.x / (unsigned)g.nblk);
  const unsigned blk = blockIdx.x - (unsigned)b * (unsigned)g.nblk;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float* fb = fix + (long long)b * g.C * g.S;
  const float* mb = mov + (long long)b * g.Cp * g.S;
  const int ng = g.Cp >> 2;
  AfXf<ND> x;
  af_load<ND>(theta + (long long)b * ND * (ND + 1), g, x);
  double acc[CPW][NV];
#pragma unroll
  for (int t = 0; t < CPW; ++t)
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[t][v] = 0.0;
#pragma unroll 1
  for (unsigned v0 = blk * (unsigned)AF_T; v0 < (unsigned)g.S; v0 += (unsigned)g.nblk * AF_T) {   // < S + 2^18 < 2^32
    const unsigned j = v0 + (unsigned)tid;
    float V[NV], q[ND];
#pragma unroll
    for (int v = 0; v < NV; ++v) V[v] = 0.f;
#pragma unroll
    for (int a = 0; a < ND; ++a) q[a] = 0.f;
    if (j < (unsigned)g.S) {
      int p[ND];
      float u[ND], r[ND], G[NG];
      af_index<ND>(g, j, p);
      af_disp<ND>(x, p, q, u);
      WsCell<ND> cell;
      ws_cell<ND>(g, p, u, cell);
      float s2 = 0.f;
#pragma unroll
      for (int a = 0; a < ND; ++a) r[a] = 0.f;
#pragma unroll
      for (int i = 0; i < NG; ++i) G[i] = 0.f;
      for (int gi = 0; gi < ng; ++gi) {
        float f[4];
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) f[cc] = 4 * gi + cc < g.C ? fb[(long long)(4 * gi + cc) * g.S + j] : 0.f;
        float4 val[NC];
        ws_corners<ND, true>(mb, g, cell, gi, val);
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
          float vv[NC], d[ND];
#pragma unroll
          for (int m = 0; m < NC; ++m) vv[m] = cc == 0 ? val[m].x : cc == 1 ? val[m].y : cc == 2 ? val[m].z : val[m].w;
          const float e = ws_interp<ND>(vv, cell, d) - f[cc];     // a channel >= C: corners and f are 0, e = 0 and d = 0
          s2 += e * e;
#pragma unroll
          for (int a = 0; a < ND; ++a) r[a] += e * d[a];
          if (FULL) {
#pragma unroll
            for (int a = 0; a < ND; ++a)
#pragma unroll
              for (int c2 = a; c2 < ND; ++c2) G[af_tri(a, c2, ND)] += d[a] * d[c2];
          }
        }
      }
      const float m = mask ? mask[(long long)b * g.S + j] : 1.f;
      V[0] = m * s2;
      V[1] = m;
#pragma unroll
      for (int a = 0; a < ND; ++a) V[2 + a] = m * r[a];
      if (FULL) {
#pragma unroll
        for (int i = 0; i < NG; ++i) V[2 + ND + i] = m * G[i];
      }
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) rec[v * AF_T + tid] = V[v];
#pragma unroll
    for (int a = 0; a < ND; ++a) rec[(NV + a) * AF_T + tid] = q[a];
    rec[(NV + ND) * AF_T + tid] = 1.f;
    if (FULL) {
#pragma unroll
      for (int a = 0; a < ND; ++a)
#pragma unroll
        for (int c2 = a; c2 < ND; ++c2) rec[(NV + ND + 1 + af_tri(a, c2, ND)) * AF_T + tid] = q[a] * q[c2];
    }
    __syncthreads();
#pragma unroll 1
    for (int i = 0; i < AF_T / 64; ++i) {
      const int vox = lane + 64 * i;
      double Vd[NV];
#pragma unroll
      for (int v = 0; v < NV; ++v) Vd[v] = (double)rec[v * AF_T + vox];
#pragma unroll
      for (int t = 0; t < CPW; ++t) {
        const int col = wv * CPW + t;
        if (col < NQ) {
          const double qd = (double)rec[(NV + col) * AF_T + vox];
#pragma unroll
          for (int v = 0; v < NV; ++v) acc[t][v] = fma(Vd[v], qd, acc[t][v]);
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int t = 0; t < CPW; ++t) {
    const int col = wv * CPW + t;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const double s = wave_sum(acc[t][v]);
      if (lane == 0 && col < NQ) part[(((long long)b * NQ + col) * NV + v) * g.nblk + blk] = s;
    }
  }
}

// out (doubles): [0] L, [1 .. B] L_b, then gb [B][P] (the gradient of L: what affine_ssd's backward scales by gout), then
// g [B][P], then -- full -- H [B][P][P].  One workgroup.
template <int ND, bool FULL>
__global__ __launch_bounds__(AF_T) void af_fin_k(const double* __restrict__ part, int B, int nblk, double C,
                                                 double* __restrict__ out) {
  constexpr int P = ND * (ND + 1);
  constexpr int NG = ND * (ND + 1) / 2;
  constexpr int NV = 2 + ND + (FULL ? NG : 0);
  constexpr int NQ = FULL ? (ND + 1) * (ND + 2) / 2 : ND + 1;
  constexpr int NE = NV * NQ;
  __shared__ double tot[NE];
  __shared__ double wall;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  double* Lb = out + 1;
  double* gb = out + 1 + B;
  double* gs = gb + (long long)B * P;
  double* Hs = gs + (long long)B * P;
  double total = 0.0, wtotal = 0.0;
  for (int b = 0; b < B; ++b) {
    for (int e = wv; e < NE; e += AF_T / 64) {
      const double* pe = part + ((long long)b * NE + e) * nblk;
      double s = 0.0;
      for (int i = lane; i < nblk; i += 64) s += pe[i];
      s = wave_sum(s);
      if (lane == 0) tot[e] = s;
    }
    __syncthreads();
    const double s2 = tot[ND * NV + 0], w = tot[ND * NV + 1];    // the column of 1
    const double sc = w > 0.0 ? 2.0 / (C * w) : 0.0;
    if (tid == 0) {
      Lb[b] = w > 0.0 ? s2 / (C * w) : 0.0;
      total += s2;
      wtotal += w;
    }
    if (tid < P) {
      const int a = tid / (ND + 1), j = tid - a * (ND + 1);
      const double v = tot[j * NV + 2 + a];
      gs[b * P + tid] = sc * v;
      gb[b * P + tid] = (2.0 / C) * v;                           // still to be divided by the sum of all weights
    }
    if (FULL) {
      for (int e = tid; e < P * P; e += AF_T) {
        const int r0 = e / P, r1 = e - r0 * P;
        const int a = r0 / (ND + 1), i = r0 - a * (ND + 1), c2 = r1 / (ND + 1), j = r1 - c2 * (ND + 1);
        const int gi = a <= c2 ? af_tri(a, c2, ND) : af_tri(c2, a, ND);
        Hs[(long long)b * P * P + e] = sc * tot[af_qq(i, j, ND) * NV + 2 + ND + gi];
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    out[0] = wtotal > 0.0 ? total / (C * wtotal) : 0.0;
    wall = wtotal;
  }
  __syncthreads();
  const double inv = wall > 0.0 ? 1.0 / wall : 0.0;
  for (int e = tid; e < B * P; e += AF_T) gb[e] *= inv;          // (written by this thread's own earlier stores or others':
}                                                                //  the barriers above order them)

// One Levenberg-Marquardt step of infer.affine_init per sample.  state[b] = (L_acc, mu, g_acc [P], H_acc [P][P]) doubles.
__global__ __launch_bounds__(AF_LM_T) void af_lm_k(const double* __restrict__ Lb, const double* __restrict__ gs,
                                                   const double* __restrict__ Hs, float* __restrict__ theta_acc,
                                                   float* __restrict__ trial, double* __restrict__ state,
                                                   double* __restrict__ hist, int nd, int k, int translation, double mu_up,
                                                   double mu_down) {
  __shared__ double sH[AF_MAXP * AF_MAXP], sg[AF_MAXP], sth[AF_MAXP];
  __shared__ double smu, sL, sLacc;
  __shared__ int sacc;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int P = nd * (nd + 1);
  double* st = state + (long long)b * (2 + P + P * P);
  if (tid == 0) {
    const double L = Lb[b];
    double Lacc = st[0], mu = st[1];
    const bool fin = L - L == 0.0;                               // finite
    const bool ok = fin && L <= Lacc;
    if (ok) {
      Lacc = L;
      if (k > 0) mu = fmax(mu * mu_down, 1e-12);
    } else {
      mu = fmin(mu * mu_up, 1e12);
    }
    st[0] = Lacc;
    st[1] = mu;
    smu = mu; sL = L; sLacc = Lacc; sacc = ok ? 1 : 0;
  }
  __syncthreads();
  const bool ok = sacc != 0;
  for (int e = tid; e < P * P; e += AF_LM_T) {
    const double h = ok ? Hs[(long long)b * P * P + e] : st[2 + P + e];
    if (ok) st[2 + P + e] = h;
    sH[e] = h;
  }
  if (tid < P) {
    const double gv = ok ? gs[b * P + tid] : st[2 + tid];
    if (ok) st[2 + tid] = gv;
    sg[tid] = gv;
    const float th = ok ? trial[b * P + tid] : theta_acc[b * P + tid];
    theta_acc[b * P + tid] = th;
    sth[tid] = (double)th;
  }
  __syncthreads();
  if (tid != 0) return;
  int fr[AF_MAXP];
  int n = 0;
  for (int e = 0; e < P; ++e)
    if (!translation || e % (nd + 1) == nd) fr[n++] = e;
  double Lc[AF_MAXP][AF_MAXP], d[AF_MAXP];
  bool singular = false;
  const double mu = smu;
  for (int i = 0; i < n && !singular; ++i) {
    for (int j = 0; j <= i; ++j) {
      double s = sH[fr[i] * P + fr[j]];
      if (i == j) s += mu * s;
      for (int c = 0; c < j; ++c) s -= Lc[i][c] * Lc[j][c];
      if (i == j) {
        if (!(s > 0.0) || !(s - s == 0.0)) { singular = true; break; }
        Lc[i][i] = sqrt(s);
      } else {
        Lc[i][j] = s / Lc[j][j];
      }
    }
  }
  if (!singular) {
    for (int i = 0; i < n; ++i) {                                // L z = -g
      double s = -sg[fr[i]];
      for (int c = 0; c < i; ++c) s -= Lc[i][c] * d[c];
      d[i] = s / Lc[i][i];
    }
    for (int i = n - 1; i >= 0; --i) {                           // L^T d = z
      double s = d[i];
      for (int c = i + 1; c < n; ++c) s -= Lc[c][i] * d[c];
      d[i] = s / Lc[i][i];
    }
  }
  for (int e = 0; e < P; ++e) trial[b * P + e] = (float)sth[e];   // (an fp32 value: the round trip is exact)
  if (!singular)
    for (int i = 0; i < n; ++i) trial[b * P + fr[i]] = (float)(sth[fr[i]] + d[i]);
  double* h = hist + (long long)b * 5;
  h[0] = sL; h[1] = sLacc; h[2] = mu; h[3] = ok ? 1.0 : 0.0; h[4] = singular ? 1.0 : 0.0;
}

inline bool af_al8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

}  // namespace

extern "C" long long dfmir_affine_ws_floats(int nd, int B, int D, int H, int W) {
  WsGeom g;
  if (!ws_geom(nd, B, 1, D, H, W, 1, &g)) return -1;
  const long long ne = nd == 3 ? 110 : 42;                       // NV * NQ of the full system
  const long long sys = (long long)B * ne * af_nblk(g.S, AF_MAXBLK);
  const long long bwd = (long long)B * nd * (nd + 1) * af_nblk(g.S, AF_BWD_MAXBLK);
  return 2 * (sys > bwd ? sys : bwd);
}

extern "C" int dfmir_affine_flow(int nd, const float* theta, float* flow, int B, int D, int H, int W, void* stream) {
  WsGeom g;
  DF_ARG_CHECK(theta && flow);
  DF_ARG_CHECK(ws_geom(nd, B, 1, D, H, W, 1, &g));
  hipStream_t st = (hipStream_t)stream;
  const int v = (W % 4 == 0 && ws_al16(flow)) ? 4 : 1;
  const int nb = (int)((g.S + (long long)AF_T * v - 1) / ((long long)AF_T * v));
  const unsigned nwg = (unsigned)((long long)B * nb);
  if (nd == 3) { if (v == 4) af_flow_k<3, 4><<<nwg, AF_T, 0, st>>>(theta, flow, g, nb); else af_flow_k<3, 1><<<nwg, AF_T, 0, st>>>(theta, flow, g, nb); }
  else { if (v == 4) af_flow_k<2, 4><<<nwg, AF_T, 0, st>>>(theta, flow, g, nb); else af_flow_k<2, 1><<<nwg, AF_T, 0, st>>>(theta, flow, g, nb); }
  DF_LAUNCH_CHECK();
  return 0;
}

extern "C" int dfmir_affine_flow_bwd(int nd, const float* dflow, float* ws, float* dtheta, int B, int D, int H, int W,
                                     void* stream) {
  WsGeom g;
  DF_ARG_CHECK(dflow && ws && dtheta && af_al8(ws));
  DF_ARG_CHECK(ws_geom(nd, B, 1, D, H, W, 1, &g));
  hipStream_t st = (hipStream_t)stream;
  const int nblk = af_nblk(g.S, AF_BWD_MAXBLK);
  double* part = reinterpret_cast<double*>(ws);
  const unsigned nwg = (unsigned)((long long)B * nblk);
  if (nd == 3) af_flow_bwd_k<3><<<nwg, AF_T, 0, st>>>(dflow, g, nblk, part);
  else af_flow_bwd_k<2><<<nwg, AF_T, 0, st>>>(dflow, g, nblk, part);
  DF_LAUNCH_CHECK();
  af_flow_fin_k<<<(unsigned)B, AF_LM_T, 0, st>>>(part, nblk, nd * (nd + 1), dtheta);
  DF_LAUNCH_CHECK();
  return 0;
}

extern "C" int dfmir_affine_system(int nd, const float* Mp, const float* F, const float* theta, const float* mask, float* ws,
                                   double* out, int full, int B, int C, int D, int H, int W, void* stream) {
  WsGeom g;
  DF_ARG_CHECK(Mp && F && theta && ws && out && ws_al16(Mp) && af_al8(ws) && af_al8(out));
  DF_ARG_CHECK(ws_geom(nd, B, C, D, H, W, 1, &g));
  g.nblk = af_nblk(g.S, AF_MAXBLK);
  hipStream_t st = (hipStream_t)stream;
  double* part = reinterpret_cast<double*>(ws);
  const unsigned nwg = (unsigned)((long long)B * g.nblk);
#define AF_LAUNCH(ND_, FULL_)                                                     \
  do {                                                                            \
    af_sys_k<ND_, FULL_><<<nwg, AF_T, 0, st>>>(Mp, F, theta, mask, g, part);      \
    DF_LAUNCH_CHECK();                                                            \
    af_fin_k<ND_, FULL_><<<1, AF_T, 0, st>>>(part, B, g.nblk, (double)C, out);    \
  } while (0)
  if (nd == 3) { if (full) AF_LAUNCH(3, true); else AF_LAUNCH(3, false); }
  else { if (full) AF_LAUNCH(2, true); else AF_LAUNCH(2, false); }
#undef AF_LAUNCH
  DF_LAUNCH_CHECK();
  return 0;
}

extern "C" int dfmir_affine_lm_step(int nd, const double* Lb, const double* g, const double* H, float* theta_acc,
                                    float* trial, double* state, double* hist, int B, int k, int translation, double mu_up,
                                    double mu_down, void* stream) {
  DF_ARG_CHECK((nd == 2 || nd == 3) && B >= 1 && k >= 0 && Lb && g && H && theta_acc && trial && state && hist);
  DF_ARG_CHECK(af_al8(Lb) && af_al8(g) && af_al8(H) && af_al8(state) && af_al8(hist));
  DF_ARG_CHECK(mu_up > 1.0 && mu_down > 0.0 && mu_down <= 1.0);
  af_lm_k<<<(unsigned)B, AF_LM_T, 0, (hipStream_t)stream>>>(Lb, g, H, theta_acc, trial, state, hist, nd, k, translation ? 1 : 0,
                                                           mu_up, mu_down);
  DF_LAUNCH_CHECK();
  return 0;
}
