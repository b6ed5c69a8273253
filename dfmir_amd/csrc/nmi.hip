// Soft-binned (Parzen) mutual information: NMI_Loss (util/losses.py:263-348), forward and backward on the fp32 matrix
// cores (v_mfma_f32_16x16x4_f32, exact fp32 products).  nb <= 64 bins are padded to NBP = 16 * NBLK; padded bins carry
// zero weight everywhere.
//
// Forward (nmi_fwd_k): the joint histogram pab[i][j] = sum_v bn[i][v] an[j][v] is a GEMM with K = voxels.  Lane l of a
// wave holds bin 16*blk + (l & 15) of voxel l >> 4 (four voxels per MFMA step) -- the operand layout of the MFMA -- so a
// voxel's bins sit in one 16-lane row and its normaliser is a DPP row sum: every exponential is computed once.  Each wave
// accumulates NBLK x NBLK 16x16 blocks plus both marginals; the waves of a workgroup are added in a fixed tree through
// LDS, every workgroup writes its own partial slot, nmi_sum_k adds the slots in index order (bit-reproducible, no
// atomics), and nmi_fin_k evaluates MI and the gradient terms the backward needs.
//
// Backward (nmi_bwd_k): per voxel ha = Gp^T bn + Ga and hb = Gp an + Gb, two (NBP x NBP) x (NBP x 16 voxels) products on
// the same MFMA (Gp and Gp^T in LDS as the A operand).  Lane l holds voxel l & 15 and bins 16*kb + 4*(l >> 4) + s: that set
// is both the K index the lane supplies to the B operand and the output rows it receives, so no lane movement is needed
// between the exponentials, the products and the chain rule through the normalisation, the exponential and the clamp.
#include "common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int NMI_FWD_WAVES = 8;              // waves per forward workgroup
constexpr int NMI_FWD_MAXWG = 256;            // forward workgroups (= partial slots) at most
constexpr int NMI_BWD_MAXWG = 1024;
constexpr float NMI_THRESH = 1e-4f;           // crop_background: voxels with mask > 1e-4 count (util/losses.py:295)

inline int nmi_nbp(int nb) { return 16 * ((nb + 15) / 16); }
// entries of one partial / of the summed histogram: joint [NBP][NBP], sum of an [NBP], sum of bn [NBP], voxel count
inline long long nmi_entries(int nbp) { return (long long)nbp * nbp + 2LL * nbp + 1; }
// gradient block written by nmi_fin_k: Gp [NBP][NBP], Gp^T [NBP][NBP], Ga [NBP], Gb [NBP], 1/V, rounded to 4 floats
inline long long nmi_gfloats(int nbp) { return ((2LL * nbp * nbp + 2LL * nbp + 1 + 3) / 4) * 4; }
inline int nmi_fwd_nwg(long long n) {
  long long w = (n + 2047) / 2048;             // >= 256 voxels per wave
  return (int)(w < 1 ? 1 : (w > NMI_FWD_MAXWG ? NMI_FWD_MAXWG : w));
}

template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xF, 0xF, false));
}
// Sum over the 16 lanes of a DPP row; every lane of the row receives the same bits.
__device__ __forceinline__ float row16_sum(float v) {
  v += dpp_f<0xB1>(v);         // quad_perm [1,0,3,2]
  v += dpp_f<0x4E>(v);         // quad_perm [2,3,0,1]
  v += dpp_f<0x141>(v);        // row_half_mirror
  v += dpp_f<0x140>(v);        // row_mirror
  return v;
}
// Sum over the four lanes l, l ^ 16, l ^ 32, l ^ 48 (same position in each row).
__device__ __forceinline__ float col4_sum(float v) {
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}
__device__ __forceinline__ float nmi_clamp(float x, float maxc) { return fminf(fmaxf(x, 0.f), maxc); }

template <int NBLK>
struct NmiFwdRegs {
  static constexpr int N = NBLK * NBLK * 4 + 2 * NBLK + 1;   // accumulators, marginals, count
};

template <int NBLK>
__global__ __launch_bounds__(64 * NMI_FWD_WAVES) void nmi_fwd_k(const float* __restrict__ a, const float* __restrict__ b,
                                                                 const float* __restrict__ mask,
                                                                 const float* __restrict__ centers, int nb, float preterm,
                                                                 float maxc, long long n, float* __restrict__ part) {
  constexpr int NBP = 16 * NBLK;
  constexpr int NR = NmiFwdRegs<NBLK>::N;
  constexpr long long E = (long long)NBP * NBP + 2 * NBP + 1;
  __shared__ float slot[NMI_FWD_WAVES / 2][NR * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, col = lane & 15;
  float cen[NBLK];
  bool on[NBLK];
#pragma unroll
  for (int k = 0; k < NBLK; ++k) {
    on[k] = 16 * k + col < nb;
    cen[k] = on[k] ? centers[16 * k + col] : 0.f;
  }
  f32x4 acc[NBLK][NBLK];
  float ma[NBLK], mb[NBLK], cnt = 0.f;
#pragma unroll
  for (int i = 0; i < NBLK; ++i) {
    ma[i] = mb[i] = 0.f;
#pragma unroll
    for (int j = 0; j < NBLK; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const long long ng = (n + 3) >> 2;                       // groups of four voxels, one per MFMA step
  const long long gstride = (long long)gridDim.x * NMI_FWD_WAVES;
  long long g = (long long)blockIdx.x * NMI_FWD_WAVES + wave;
  float xa = 0.f, xb = 0.f, xm = 1.f;
  if (g < ng) {
    const long long v = 4 * g + q;
    if (v < n) { xa = a[v]; xb = b[v]; xm = mask ? mask[v] : 1.f; }
    else xm = 0.f;
  }
  for (; g < ng; g += gstride) {
    const float ca = nmi_clamp(xa, maxc), cb = nmi_clamp(xb, maxc);
    const bool valid = xm > NMI_THRESH;
    {                                                      // the next group's values, loaded under this group's work
      const long long gn = g + gstride, v = 4 * gn + q;
      xa = xb = 0.f; xm = 0.f;
      if (gn < ng && v < n) { xa = a[v]; xb = b[v]; xm = mask ? mask[v] : 1.f; }
    }
    float ea[NBLK], eb[NBLK], sa = 0.f, sb = 0.f;
#pragma unroll
    for (int k = 0; k < NBLK; ++k) {
      const float da = ca - cen[k], db = cb - cen[k];
      ea[k] = on[k] ? expf(-preterm * (da * da)) : 0.f;
      eb[k] = on[k] ? expf(-preterm * (db * db)) : 0.f;
      sa += ea[k];
      sb += eb[k];
    }
    sa = row16_sum(sa);
    sb = row16_sum(sb);
    const float ia = valid ? 1.f / sa : 0.f, ib = valid ? 1.f / sb : 0.f;
    float an[NBLK], bn[NBLK];
#pragma unroll
    for (int k = 0; k < NBLK; ++k) {
      an[k] = valid ? ea[k] * ia : 0.f;
      bn[k] = valid ? eb[k] * ib : 0.f;
      ma[k] += an[k];
      mb[k] += bn[k];
    }
    cnt += valid ? 1.f : 0.f;
#pragma unroll
    for (int i = 0; i < NBLK; ++i)
#pragma unroll
      for (int j = 0; j < NBLK; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(bn[i], an[j], acc[i][j], 0, 0, 0);
  }
#pragma unroll
  for (int k = 0; k < NBLK; ++k) {                         // the four voxels of a step -> one value per bin
    ma[k] = col4_sum(ma[k]);
    mb[k] = col4_sum(mb[k]);
  }
  cnt = col4_sum(cnt);
  // waves added in a fixed tree: (w0 + w4) + (w2 + w6) ... -- the same order every run
  for (int half = NMI_FWD_WAVES / 2; half >= 1; half >>= 1) {
    if (wave >= half && wave < 2 * half) {
      float* s = slot[wave - half];
      int r = 0;
#pragma unroll
      for (int i = 0; i < NBLK; ++i)
#pragma unroll
        for (int j = 0; j < NBLK; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e) s[(r++) * 64 + lane] = acc[i][j][e];
#pragma unroll
      for (int k = 0; k < NBLK; ++k) { s[(r++) * 64 + lane] = ma[k]; s[(r++) * 64 + lane] = mb[k]; }
      s[r * 64 + lane] = cnt;
    }
    __syncthreads();
    if (wave < half) {
      const float* s = slot[wave];
      int r = 0;
#pragma unroll
      for (int i = 0; i < NBLK; ++i)
#pragma unroll
        for (int j = 0; j < NBLK; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[i][j][e] += s[(r++) * 64 + lane];
#pragma unroll
      for (int k = 0; k < NBLK; ++k) { ma[k] += s[(r++) * 64 + lane]; mb[k] += s[(r++) * 64 + lane]; }
      cnt += s[r * 64 + lane];
    }
    __syncthreads();
  }
  if (wave) return;
  float* p = part + (long long)blockIdx.x * E;
  // D layout of 16x16x4: register e of lane l = row 4 * (l >> 4) + e, column l & 15
#pragma unroll
  for (int i = 0; i < NBLK; ++i)
#pragma unroll
    for (int j = 0; j < NBLK; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) p[(16 * i + 4 * q + e) * NBP + 16 * j + col] = acc[i][j][e];
  if (q == 0) {
#pragma unroll
    for (int k = 0; k < NBLK; ++k) { p[NBP * NBP + 16 * k + col] = ma[k]; p[NBP * NBP + NBP + 16 * k + col] = mb[k]; }
  }
  if (lane == 0) p[E - 1] = cnt;
}

// sums[e] = sum over the workgroup slots, in slot order (the count in double: exact integers)
__global__ __launch_bounds__(256) void nmi_sum_k(const float* __restrict__ part, float* __restrict__ sums, long long E,
                                                 int nslots) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  if (e == E - 1) {
    double c = 0.0;
    for (int w = 0; w < nslots; ++w) c += (double)part[(long long)w * E + e];
    sums[e] = (float)c;
    return;
  }
  float s = 0.f;
#pragma unroll 8
  for (int w = 0; w < nslots; ++w) s += part[(long long)w * E + e];
  sums[e] = s;
}

// MI and the terms of its gradient (one workgroup).  With r = pab / papb, qq = r + 1e-5, papb = pb pa^T + 1e-5:
//   MI = sum pab log(qq);  dMI/dpab = log(qq) + pab / (qq papb);  dMI/dpapb = -pab r / (qq papb);
//   dMI/dpa[j] = sum_i dMI/dpapb[i][j] pb[i];  dMI/dpb[i] = sum_j dMI/dpapb[i][j] pa[j].
__global__ __launch_bounds__(1024) void nmi_fin_k(const float* __restrict__ sums, float* __restrict__ G,
                                                  float* __restrict__ out, int nb, int nbp) {
  __shared__ float dpab[64 * 64];
  __shared__ float sm[17];
  const float V = sums[(long long)nbp * nbp + 2 * nbp];
  const float* sa = sums + nbp * nbp;
  const float* sb = sa + nbp;
  float* Gp = G;
  float* GpT = G + nbp * nbp;
  float* Ga = GpT + nbp * nbp;
  float* Gb = Ga + nbp;
  float mi = 0.f;
  for (int e = threadIdx.x; e < nbp * nbp; e += 1024) {
    const int i = e / nbp, j = e - i * nbp;
    float gp = 0.f, dp = 0.f;
    if (i < nb && j < nb) {
      const float pab = sums[e] / V, pa = sa[j] / V, pb = sb[i] / V;
      const float papb = pb * pa + 1e-5f;
      const float r = pab / papb, qq = r + 1e-5f, l = logf(qq);
      mi += pab * l;
      gp = l + pab / (qq * papb);
      dp = -pab * r / (qq * papb);
      dpab[i * nb + j] = dp;
    }
    Gp[e] = gp;
    GpT[j * nbp + i] = gp;
  }
  mi = block_sum(mi, sm);                // (its barriers also publish dpab)
  if (threadIdx.x == 0) {
    out[0] = -mi;
    Gb[nbp] = 1.f / V;                   // the slot after Gb: 1/V
  }
  const int k = threadIdx.x;
  if (k < nbp) {
    float ga = 0.f, gb = 0.f;
    if (k < nb) {
      for (int i = 0; i < nb; ++i) ga += dpab[i * nb + k] * (sb[i] / V);
      for (int j = 0; j < nb; ++j) gb += dpab[k * nb + j] * (sa[j] / V);
    }
    Ga[k] = ga;
    Gb[k] = gb;
  }
}

// dL/dx = gout * (2 preterm / V) * sum_k n_k (h_k - sum_j n_j h_j) (clamp(x) - c_k), zero where the clamp or the crop mask
// cuts; h = Gp^T bn + Ga for y_true (n = an), h = Gp an + Gb for y_pred (n = bn).
template <int NBLK>
__global__ __launch_bounds__(256) void nmi_bwd_k(const float* __restrict__ a, const float* __restrict__ b,
                                                 const float* __restrict__ mask, const float* __restrict__ centers, int nb,
                                                 float preterm, float maxc, long long n, const float* __restrict__ G,
                                                 const float* __restrict__ gout, float* __restrict__ da,
                                                 float* __restrict__ db) {
  constexpr int NBP = 16 * NBLK, SP = NBP + 4, NT = 4 * NBLK;   // SP: rows 4 apart land 16 banks apart
  __shared__ float sGp[NBP * SP], sGpT[NBP * SP];
  for (int e = threadIdx.x; e < NBP * NBP; e += 256) {
    const int i = e / NBP, j = e - i * NBP;
    sGp[i * SP + j] = G[e];
    sGpT[i * SP + j] = G[NBP * NBP + e];
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, col = lane & 15;
  float cen[NT], ga[NT], gb[NT];
  bool on[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int bin = 16 * (t >> 2) + 4 * q + (t & 3);
    on[t] = bin < nb;
    cen[t] = on[t] ? centers[bin] : 0.f;
    ga[t] = G[2 * NBP * NBP + bin];
    gb[t] = G[2 * NBP * NBP + NBP + bin];
  }
  const float coef = gout[0] * 2.f * preterm * G[2 * NBP * NBP + 2 * NBP];
  __syncthreads();
  for (long long v0 = ((long long)blockIdx.x * 4 + wave) * 16; v0 < n; v0 += (long long)gridDim.x * 64) {
    const long long v = v0 + col;
    float xa = 0.f, xb = 0.f, xm = 0.f;
    if (v < n) { xa = a[v]; xb = b[v]; xm = mask ? mask[v] : 1.f; }
    const float ca = nmi_clamp(xa, maxc), cb = nmi_clamp(xb, maxc);
    float an[NT], bn[NT], sa = 0.f, sb = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const float d1 = ca - cen[t], d2 = cb - cen[t];
      an[t] = on[t] ? expf(-preterm * (d1 * d1)) : 0.f;
      bn[t] = on[t] ? expf(-preterm * (d2 * d2)) : 0.f;
      sa += an[t];
      sb += bn[t];
    }
    const float ia = 1.f / col4_sum(sa), ib = 1.f / col4_sum(sb);
#pragma unroll
    for (int t = 0; t < NT; ++t) { an[t] *= ia; bn[t] *= ib; }
    f32x4 ha[NBLK], hb[NBLK];
#pragma unroll
    for (int m = 0; m < NBLK; ++m) ha[m] = hb[m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < NT; ++t) {                 // K step t: bins 16 * (t >> 2) + 4 * q' + (t & 3), q' = 0..3
      const int row = 16 * (t >> 2) + 4 * q + (t & 3);
#pragma unroll
      for (int m = 0; m < NBLK; ++m) {
        ha[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(sGp[row * SP + 16 * m + col], bn[t], ha[m], 0, 0, 0);
        hb[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(sGpT[row * SP + 16 * m + col], an[t], hb[m], 0, 0, 0);
      }
    }
    float ma = 0.f, mb = 0.f;                      // register r of block m = bin 16 m + 4 q + r = this lane's bin t = 4 m + r
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      ma += an[t] * (ha[t >> 2][t & 3] + ga[t]);
      mb += bn[t] * (hb[t >> 2][t & 3] + gb[t]);
    }
    ma = col4_sum(ma);
    mb = col4_sum(mb);
    float sa2 = 0.f, sb2 = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      sa2 += an[t] * (ha[t >> 2][t & 3] + ga[t] - ma) * (ca - cen[t]);
      sb2 += bn[t] * (hb[t >> 2][t & 3] + gb[t] - mb) * (cb - cen[t]);
    }
    sa2 = col4_sum(sa2);
    sb2 = col4_sum(sb2);
    if (q == 0 && v < n) {
      const bool valid = xm > NMI_THRESH;
      if (da) da[v] = (valid && xa >= 0.f && xa <= maxc) ? coef * sa2 : 0.f;
      if (db) db[v] = (valid && xb >= 0.f && xb <= maxc) ? coef * sb2 : 0.f;
    }
  }
}

}  // namespace

extern "C" long long dfmir_nmi_ws_floats(long long n, int nb) {
  if (n <= 0 || nb < 2 || nb > 64) return -1;
  const int nbp = nmi_nbp(nb);
  const long long E = nmi_entries(nbp);
  return E + nmi_gfloats(nbp) + (long long)nmi_fwd_nwg(n) * E;
}

extern "C" int dfmir_nmi_fwd(const float* y_true, const float* y_pred, const float* mask, const float* centers, int nb,
                             float preterm, float max_clip, long long n, float* ws, float* out, void* stream) {
  DF_ARG_CHECK(y_true && y_pred && centers && ws && out && n > 0 && nb >= 2 && nb <= 64);
  hipStream_t st = (hipStream_t)stream;
  const int nbp = nmi_nbp(nb), nwg = nmi_fwd_nwg(n);
  const long long E = nmi_entries(nbp);
  float* sums = ws;
  float* G = ws + E;
  float* part = G + nmi_gfloats(nbp);
  switch (nbp / 16) {
    case 1: nmi_fwd_k<1><<<nwg, 64 * NMI_FWD_WAVES, 0, st>>>(y_true, y_pred, mask, centers, nb, preterm, max_clip, n, part); break;
    case 2: nmi_fwd_k<2><<<nwg, 64 * NMI_FWD_WAVES, 0, st>>>(y_true, y_pred, mask, centers, nb, preterm, max_clip, n, part); break;
    case 3: nmi_fwd_k<3><<<nwg, 64 * NMI_FWD_WAVES, 0, st>>>(y_true, y_pred, mask, centers, nb, preterm, max_clip, n, part); break;
    default: nmi_fwd_k<4><<<nwg, 64 * NMI_FWD_WAVES, 0, st>>>(y_true, y_pred, mask, centers, nb, preterm, max_clip, n, part); break;
  }
  DF_LAUNCH_CHECK();
  nmi_sum_k<<<(unsigned)((E + 255) / 256), 256, 0, st>>>(part, sums, E, nwg);
  DF_LAUNCH_CHECK();
  nmi_fin_k<<<1, 1024, 0, st>>>(sums, G, out, nb, nbp);
  DF_LAUNCH_CHECK();
  return 0;
}

extern "C" int dfmir_nmi_bwd(const float* y_true, const float* y_pred, const float* mask, const float* centers, int nb,
                             float preterm, float max_clip, long long n, const float* ws, const float* gout, float* d_true,
                             float* d_pred, void* stream) {
  DF_ARG_CHECK(y_true && y_pred && centers && ws && gout && n > 0 && nb >= 2 && nb <= 64);
  if (!d_true && !d_pred) return 0;
  hipStream_t st = (hipStream_t)stream;
  const int nbp = nmi_nbp(nb);
  const float* G = ws + nmi_entries(nbp);
  const unsigned nwg = df_grid(n, 64, NMI_BWD_MAXWG);
  switch (nbp / 16) {
    case 1: nmi_bwd_k<1><<<nwg, 256, 0, st>>>(y_true, y_pred, mask, centers, nb, preterm, max_clip, n, G, gout, d_true, d_pred); break;
    case 2: nmi_bwd_k<2><<<nwg, 256, 0, st>>>(y_true, y_pred, mask, centers, nb, preterm, max_clip, n, G, gout, d_true, d_pred); break;
    case 3: nmi_bwd_k<3><<<nwg, 256, 0, st>>>(y_true, y_pred, mask, centers, nb, preterm, max_clip, n, G, gout, d_true, d_pred); break;
    default: nmi_bwd_k<4><<<nwg, 256, 0, st>>>(y_true, y_pred, mask, centers, nb, preterm, max_clip, n, G, gout, d_true, d_pred); break;
  }
  DF_LAUNCH_CHECK();
  return 0;
}
