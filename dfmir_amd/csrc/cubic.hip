// Cubic B-spline image resampling, 2-D and 3-D: the prefilter that makes the spline interpolating, and the warp that
// samples it at x + flow(x) with its gradient in the flow.  Build-defined (include/dfmir_hip.h, ops.spline_prefilter and
// ops.warp_cubic state the definition):
//
//   refl(i), an axis of extent n:  n == 1: 0;  else j = i mod (2 n - 2) (non-negative), j < n ? j : 2 n - 2 - j -- the
//   whole-sample mirror d c b | a b c d | c b a, at any distance.
//   prefilter, per axis (the axes commute):  (c[refl(i - 1)] + 4 c[i] + c[refl(i + 1)]) / 6 = s[i].
//   sampling, per axis:  i = floor(p), t = p - i,  w0 = (1 - t)^3 / 6, w1 = (3 t^3 - 6 t^2 + 4) / 6,
//   w2 = (-3 t^3 + 3 t^2 + 3 t + 1) / 6, w3 = t^3 / 6;  out = sum over the 4^nd taps of prod_a w_ka(t_a) c[refl(i_a - 1 + k_a)].
//
// The prefilter is the FIR form  c[i] = sum_{|k| <= 16} sqrt(3) z^|k| s[refl(i + k)],  z = sqrt(3) - 2: the exact inverse
// truncated where |z|^17 / (1 - |z|) < 8e-10 of max |s|, below fp32 rounding.  Why not the two-sweep recursion (4 LDS accesses
// per sample against 33): its sweeps are serial along a line, so a 32 x 64 tile offers 64 + 96 lines to 256 threads and each
// walks 64 .. 96 dependent steps, while the FIR keeps every thread on its own outputs with independent sums, is gs_tile_k's
// proven tile (gauss.hip) with mirror staging in place of zero staging and no renormalisation, and adds its terms from the
// smallest to the largest, which leaves about one rounding of the result per axis.  Both forms cross HBM equally often.
//   cb_tile_k<TH, XF, VEC>  gs_tile_k's layout: a TH x 64 tile of one plane with a halo of 16 (the x halo only with XF) in
//              LDS, halo cells holding the REFLECTED sample (the reflection repeats where the halo is wider than the axis);
//              with XF rows are filtered along x into a second tile, then the tile is filtered along y.  An axis of extent 1
//              has radius 0 and is passed through bit for bit.
//   2-D: one launch.  3-D: the (y, x) pass over the B C D planes, then the z pass as the same kernel <64, no XF> on the view
//   [B C][D][H W].  16-byte global accesses where the row length is a multiple of 4 and the pointers are aligned.
//   cw_k<ND, BWD>  one thread per output voxel, looping over the channels.  The 4 reflected indices and the 4 (+ 4) weights
//              per axis are formed once per voxel (12 reflections, not 64); when every tap lies inside the volume the
//              indices are i - 1 + k without a reflection and the x taps are 4 contiguous floats, one 16-byte load.  floor and t are taken
//              from the FLOW (p = x + flow with x an integer: floor(p) = x + floor(flow), t = flow - floor(flow)), so t
//              does not carry the rounding of the fp32 sum x + flow.  BWD shares the tap loads: per channel the taps give
//              the value's derivative along every axis, multiplied by dout and summed over the channels in channel order;
//              each dflow element is written once -- no atomics, bit-identical from run to run.
//              The z taps are a ROLLED loop over planes of 16 taps: fully unrolled, the 64 loads of a channel took 192 (forward)
//              and 256 (backward) registers, 2 and 1 waves per SIMD; rolled, 74 and 94.  An interior row's 4 x taps come as
//              ONE 16-byte load (4-byte aligned).  Measured at 160 x 192 x 224 with flows of +-1.5 voxels drawn per voxel, each
//              step A/B in one call: unrolled 0.50 ms forward and 1.25 ms forward + backward; rolled 0.45 and 0.90; rolled
//              with the 16-byte rows 0.31 and 0.64 (profiles/cubic_timing.txt has the last).  The gather is served by L1 /
//              L2 -- the tensor crosses HBM once -- and is bound by the load instructions and the cache lines a wave's 64
//              lanes touch per tap, not by bytes.
// A position that is not finite or has |x + flow| >= 2^24 (the fp32 sum) on any axis gives out = 0 and dflow = 0.
// Every output is written once from sums in a fixed order.  Nothing syncs.
#include "common.h"
#include <math.h>

namespace {

constexpr int CB_T = 256;
constexpr int CB_R = 16;
constexpr int CB_TW = 64;

struct CbW { float w[CB_R + 1]; };             // w[|k|]

__device__ __forceinline__ int cb_refl(int i, int n) {
  if (n == 1) return 0;
  const int per = 2 * n - 2;
  int j = i % per;
  if (j < 0) j += per;
  return j < n ? j : per - j;
}

template <int TH, bool XF, bool VEC>
__global__ __launch_bounds__(CB_T) void cb_tile_k(const float* __restrict__ in, float* __restrict__ out, int H, int W,
                                                  int tiles_x, int tiles_y, int rx, int ry, CbW wx, CbW wy) {
  constexpr int LW = XF ? CB_TW + 2 * CB_R : CB_TW;
  constexpr int LH = TH + 2 * CB_R;
  __shared__ __attribute__((aligned(16))) float tin[LH * LW];
  __shared__ __attribute__((aligned(16))) float tmid[XF ? LH * CB_TW : 4];
  unsigned bid = blockIdx.x;
  const int tx = (int)(bid % (unsigned)tiles_x); bid /= (unsigned)tiles_x;
  const int ty = (int)(bid % (unsigned)tiles_y);
  const long long plane = (long long)(bid / (unsigned)tiles_y);
  const float* ip = in + plane * H * W;
  float* op = out + plane * H * W;
  const int x0 = tx * CB_TW, y0 = ty * TH;
  const int th = min(TH, H - y0);
  const int hx = XF ? rx : 0;                                   // 0 or 16: a multiple of 4
  const int nrows = th + 2 * ry;                                // <= LH
  const int ncols = CB_TW + 2 * hx;                             // <= LW
  const int tid = threadIdx.x;

  // the tile and its halo; a cell outside the plane takes the reflected sample, so every address formed is inside
  if (VEC) {
    const int nq = ncols >> 2;
    for (int i = tid; i < nrows * nq; i += CB_T) {
      const int r = i / nq, q = i - r * nq;
      int gy = y0 - ry + r;
      const int gx = x0 - hx + 4 * q;                           // W % 4 == 0: a quad lies inside or outside as a whole
      if ((unsigned)gy >= (unsigned)H) gy = cb_refl(gy, H);
      const float* row = ip + (long long)gy * W;
      float4 v;
      if ((unsigned)gx < (unsigned)W) {
        v = *reinterpret_cast<const float4*>(row + gx);
      } else {
        v.x = row[cb_refl(gx, W)]; v.y = row[cb_refl(gx + 1, W)]; v.z = row[cb_refl(gx + 2, W)]; v.w = row[cb_refl(gx + 3, W)];
      }
      *reinterpret_cast<float4*>(tin + r * LW + 4 * q) = v;
    }
  } else {
    for (int i = tid; i < nrows * ncols; i += CB_T) {
      const int r = i / ncols, c = i - r * ncols;
      int gy = y0 - ry + r, gx = x0 - hx + c;
      if ((unsigned)gy >= (unsigned)H) gy = cb_refl(gy, H);
      if ((unsigned)gx >= (unsigned)W) gx = cb_refl(gx, W);
      tin[r * LW + c] = ip[(long long)gy * W + gx];
    }
  }
  __syncthreads();

  if (XF) {
    // along x: thread tid keeps column tid & 63 and walks the staged rows four apart
    const int c = tid & (CB_TW - 1);
    for (int r = tid >> 6; r < nrows; r += CB_T / CB_TW) {
      const float* row = tin + r * LW + hx + c;
      float acc = 0.f;
#pragma unroll
      for (int k = CB_R; k >= 1; --k) acc += wx.w[k] * (row[-k] + row[k]);        // XF: rx == CB_R
      tmid[r * CB_TW + c] = acc + wx.w[0] * row[0];
    }
    __syncthreads();
  }

  // along y: a thread owns four consecutive columns of a row
  const float* src = XF ? tmid : tin;                           // both CB_TW wide here (LW == CB_TW without XF)
  for (int i = tid; i < th * (CB_TW / 4); i += CB_T) {
    const int row = i >> 4, c = (i & 15) << 2;
    if (x0 + c >= W) continue;
    const int gy = y0 + row;
    const float* col = src + (row + ry) * CB_TW + c;
    float4 acc = *reinterpret_cast<const float4*>(col);
    if (ry > 0) {                                               // ry == 0: the value as it stands, bit for bit
      const float4 ctr = acc;
      acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int k = CB_R; k >= 1; --k) {
        const float w = wy.w[k];
        const float4 a = *reinterpret_cast<const float4*>(col - k * CB_TW);
        const float4 b = *reinterpret_cast<const float4*>(col + k * CB_TW);
        acc.x += w * (a.x + b.x); acc.y += w * (a.y + b.y); acc.z += w * (a.z + b.z); acc.w += w * (a.w + b.w);
      }
      const float w = wy.w[0];
      acc.x += w * ctr.x; acc.y += w * ctr.y; acc.z += w * ctr.z; acc.w += w * ctr.w;
    }
    float* o = op + (long long)gy * W + x0 + c;
    if (VEC) {
      *reinterpret_cast<float4*>(o) = acc;
    } else {
      o[0] = acc.x;
      if (x0 + c + 1 < W) o[1] = acc.y;
      if (x0 + c + 2 < W) o[2] = acc.z;
      if (x0 + c + 3 < W) o[3] = acc.w;
    }
  }
}

// sqrt(3) z^k, z = sqrt(3) - 2, formed in double and rounded to fp32
void cb_weights(CbW* w) {
  const double z = sqrt(3.0) - 2.0;
  double p = sqrt(3.0);
  for (int k = 0; k <= CB_R; ++k) { w->w[k] = (float)p; p *= z; }
}

inline bool cb_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// one pass over P planes [H][W]: rows filtered when fy, columns when fx (an axis of extent 1 is never filtered)
int cb_pass(const float* in, float* out, long long P, int H, int W, bool fx, bool fy, const CbW& w, hipStream_t st) {
  const bool vec = W % 4 == 0 && cb_al16(in) && cb_al16(out);
  const int TH = fx ? 32 : 64;
  const int tiles_x = (W + CB_TW - 1) / CB_TW, tiles_y = (H + TH - 1) / TH;
  const long long nwg = P * tiles_x * tiles_y;
  DF_ARG_CHECK(nwg < (1LL << 31));
  const int rx = fx ? CB_R : 0, ry = fy ? CB_R : 0;
#define CB_LAUNCH(TH_, XF_, VEC_) \
  cb_tile_k<TH_, XF_, VEC_><<<(unsigned)nwg, CB_T, 0, st>>>(in, out, H, W, tiles_x, tiles_y, rx, ry, w, w)
  if (fx) { if (vec) CB_LAUNCH(32, true, true); else CB_LAUNCH(32, true, false); }
  else { if (vec) CB_LAUNCH(64, false, true); else CB_LAUNCH(64, false, false); }
#undef CB_LAUNCH
  DF_LAUNCH_CHECK();
  return 0;
}

// ---- the warp ----
constexpr int CW_T = 256;
constexpr float CW_PMAX = 16777216.f;          // 2^24

// i = floor(f) as an int (|f| < 2^25 here: extents are <= 2^24), t = f - floor(f) in [0, 1]: exact for f >= 0 and for f <= -1,
// one rounding for -1 < f < 0 (t == 1 is a legal argument of the weights: the taps of the next cell with w0 = 0)
__device__ __forceinline__ void cw_split(float f, int& i, float& t) {
  const float fl = floorf(f);
  i = (int)fl;
  t = f - fl;
}
template <bool BWD>
__device__ __forceinline__ void cw_weights(float t, float* w, float* dw) {
  const float u = 1.f - t, t2 = t * t, t3 = t2 * t;
  w[0] = u * u * u * (1.f / 6.f);
  w[1] = (3.f * t3 - 6.f * t2 + 4.f) * (1.f / 6.f);
  w[2] = (-3.f * t3 + 3.f * t2 + 3.f * t + 1.f) * (1.f / 6.f);
  w[3] = t3 * (1.f / 6.f);
  if (BWD) {
    dw[0] = -0.5f * u * u;
    dw[1] = 0.5f * (3.f * t2 - 4.f * t);
    dw[2] = 0.5f * (-3.f * t2 + 2.f * t + 1.f);
    dw[3] = 0.5f * t2;
  }
}
// the 4 tap indices of an axis: i0 .. i0 + 3 reflected; one modulo, then steps
__device__ __forceinline__ void cw_taps(int i0, int n, int* idx) {
  if (n == 1) { idx[0] = idx[1] = idx[2] = idx[3] = 0; return; }
  const int per = 2 * n - 2;
  int m = i0 % per;
  if (m < 0) m += per;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int j = m + k;                                              // < per + 3: at most two periods too far (per == 2)
    if (j >= per) j -= per;
    if (j >= per) j -= per;
    idx[k] = j < n ? j : per - j;
  }
}

// the 16 taps of one plane: pv = sum wy wx a, pvy = sum wy' wx a, pvx = sum wy wx' a.  IN: every tap is inside, the x taps of a
// row are 4 contiguous floats and come as ONE 16-byte load (4-byte aligned: legal for global memory)
struct __attribute__((aligned(4))) CwRow { float a0, a1, a2, a3; };
template <bool BWD, bool IN>
__device__ __forceinline__ void cw_plane(const float* __restrict__ pp, const int* oy, const int* ox, const float* wy,
                                         const float* dy, const float* wx, const float* dx, float& pv, float& pvy, float& pvx) {
#pragma unroll
  for (int ky = 0; ky < 4; ++ky) {
    const float* rp = pp + oy[ky];
    CwRow q;
    if (IN) q = *reinterpret_cast<const CwRow*>(rp + ox[0]);
    else { q.a0 = rp[ox[0]]; q.a1 = rp[ox[1]]; q.a2 = rp[ox[2]]; q.a3 = rp[ox[3]]; }
    const float rv = wx[0] * q.a0 + wx[1] * q.a1 + wx[2] * q.a2 + wx[3] * q.a3;
    pv += wy[ky] * rv;
    if (BWD) {
      pvy += dy[ky] * rv;
      pvx += wy[ky] * (dx[0] * q.a0 + dx[1] * q.a1 + dx[2] * q.a2 + dx[3] * q.a3);
    }
  }
}

// c: coefficients [B][C][S]; flow [B][ND][S]; !BWD: out [B][C][S]; BWD: dout [B][C][S] -> dflow [B][ND][S]
template <int ND, bool BWD>
__global__ __launch_bounds__(CW_T) void cw_k(const float* __restrict__ c, const float* __restrict__ flow,
                                              const float* __restrict__ dout, float* __restrict__ out, int C, int D, int H,
                                              int W, long long total) {
  const long long S = (long long)D * H * W;                     // B S < 2^31: the voxel is decomposed in 32 bits
  const unsigned v = blockIdx.x * (unsigned)CW_T + threadIdx.x;
  if (v >= (unsigned)total) return;
  const unsigned bu = v / (unsigned)S, su = v - bu * (unsigned)S, ru = su / (unsigned)W;
  const long long b = bu, s = su;
  const int x = (int)(su - ru * (unsigned)W), y = (int)(ru % (unsigned)H), z = (int)(ru / (unsigned)H);
  const float* fp = flow + b * ND * S + s;
  const float fz = ND == 3 ? fp[0] : 0.f, fy = fp[(ND - 2) * S], fx = fp[(ND - 1) * S];
  const float pz = (float)z + fz, py = (float)y + fy, px = (float)x + fx;
  const bool ok = fabsf(pz) < CW_PMAX && fabsf(py) < CW_PMAX && fabsf(px) < CW_PMAX;      // false for NaN and inf too
  if (!ok) {
    if (BWD) {
      for (int a = 0; a < ND; ++a) out[b * ND * S + a * S + s] = 0.f;
    } else {
      for (int ch = 0; ch < C; ++ch) out[(b * C + ch) * S + s] = 0.f;
    }
    return;
  }
  int iz = 0, iy, ix;
  float tz = 0.f, ty, tx;
  if (ND == 3) cw_split(fz, iz, tz);
  cw_split(fy, iy, ty);
  cw_split(fx, ix, tx);
  iz += z - 1; iy += y - 1; ix += x - 1;                        // the first tap
  float wz[4], wy[4], wx[4], dz[4], dy[4], dx[4];
  if (ND == 3) cw_weights<BWD>(tz, wz, dz);
  cw_weights<BWD>(ty, wy, dy);
  cw_weights<BWD>(tx, wx, dx);
  int oz[4] = {0, 0, 0, 0}, oy[4], ox[4];
  const bool inside = (ND == 2 || (iz >= 0 && iz + 3 < D)) && iy >= 0 && iy + 3 < H && ix >= 0 && ix + 3 < W;
  if (inside) {
#pragma unroll
    for (int k = 0; k < 4; ++k) { oz[k] = ND == 3 ? (iz + k) * H * W : 0; oy[k] = (iy + k) * W; ox[k] = ix + k; }
  } else {
    if (ND == 3) cw_taps(iz, D, oz);
    cw_taps(iy, H, oy);
    cw_taps(ix, W, ox);
#pragma unroll
    for (int k = 0; k < 4; ++k) { oz[k] *= H * W; oy[k] *= W; }
  }
  constexpr int NZ = ND == 3 ? 4 : 1;
  float gz = 0.f, gy = 0.f, gx = 0.f;
  for (int ch = 0; ch < C; ++ch) {
    const float* cp = c + (b * C + ch) * S;
    float val = 0.f, vz = 0.f, vy = 0.f, vx = 0.f;
#pragma unroll 1
    for (int kz = 0; kz < NZ; ++kz) {                           // rolled: 6 waves per SIMD, not 2 (see the file header)
      const int ozk = kz == 0 ? oz[0] : kz == 1 ? oz[1] : kz == 2 ? oz[2] : oz[3];
      const float wzk = kz == 0 ? wz[0] : kz == 1 ? wz[1] : kz == 2 ? wz[2] : wz[3];
      const float dzk = BWD ? (kz == 0 ? dz[0] : kz == 1 ? dz[1] : kz == 2 ? dz[2] : dz[3]) : 0.f;
      float pv = 0.f, pvy = 0.f, pvx = 0.f;                     // the plane's value and its derivatives along y and x
      if (inside) cw_plane<BWD, true>(cp + ozk, oy, ox, wy, dy, wx, dx, pv, pvy, pvx);
      else cw_plane<BWD, false>(cp + ozk, oy, ox, wy, dy, wx, dx, pv, pvy, pvx);
      if (ND == 3) {
        val += wzk * pv;
        if (BWD) { vz += dzk * pv; vy += wzk * pvy; vx += wzk * pvx; }
      } else {
        val = pv;
        if (BWD) { vy = pvy; vx = pvx; }
      }
    }
    if (BWD) {
      const float g = dout[(b * C + ch) * S + s];
      gz += g * vz; gy += g * vy; gx += g * vx;
    } else {
      out[(b * C + ch) * S + s] = val;
    }
  }
  if (BWD) {
    float* dp = out + b * ND * S + s;
    if (ND == 3) dp[0] = gz;
    dp[(ND - 2) * S] = gy;
    dp[(ND - 1) * S] = gx;
  }
}

int cw_launch(int nd, bool bwd, const float* c, const float* flow, const float* dout, float* out, int B, int C, int D, int H,
              int W, hipStream_t st) {
  DF_ARG_CHECK((nd == 2 || nd == 3) && c && flow && out && (!bwd || dout) && B >= 1 && C >= 1 && H >= 1 && W >= 1 &&
               (nd == 2 || D >= 1));
  if (nd == 2) D = 1;
  DF_ARG_CHECK(D <= (1 << 24) && H <= (1 << 24) && W <= (1 << 24));
  const long long S = (long long)D * H * W;
  DF_ARG_CHECK(S < (1LL << 31) && (long long)B * C * S < (1LL << 31) && (long long)B * nd * S < (1LL << 31));
  DF_ARG_CHECK(out != c && out != flow && out != dout);
  const long long total = (long long)B * S;
  const unsigned grid = (unsigned)((total + CW_T - 1) / CW_T);
  if (nd == 3) {
    if (bwd) cw_k<3, true><<<grid, CW_T, 0, st>>>(c, flow, dout, out, C, D, H, W, total);
    else cw_k<3, false><<<grid, CW_T, 0, st>>>(c, flow, dout, out, C, D, H, W, total);
  } else {
    if (bwd) cw_k<2, true><<<grid, CW_T, 0, st>>>(c, flow, dout, out, C, D, H, W, total);
    else cw_k<2, false><<<grid, CW_T, 0, st>>>(c, flow, dout, out, C, D, H, W, total);
  }
  DF_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int dfmir_spline_prefilter(int nd, const float* in, float* out, float* tmp, long long planes, int D, int H, int W,
                                      void* stream) {
  DF_ARG_CHECK((nd == 2 || nd == 3) && in && out && in != out && planes >= 1 && H >= 1 && W >= 1 && (nd == 2 || D >= 1));
  if (nd == 2) D = 1;
  DF_ARG_CHECK(planes * D * H * W < (1LL << 31));
  CbW w;
  cb_weights(&w);
  hipStream_t st = (hipStream_t)stream;
  const bool pass_z = D > 1, pass_xy = H > 1 || W > 1 || !pass_z;
  DF_ARG_CHECK(!(pass_z && pass_xy) || (tmp && tmp != in && tmp != out));
  if (pass_xy) {
    const int rc = cb_pass(in, pass_z ? tmp : out, planes * D, H, W, W > 1, H > 1, w, st);
    if (rc) return rc;
  }
  if (pass_z) return cb_pass(pass_xy ? tmp : in, out, planes, D, H * W, false, true, w, st);
  return 0;
}

extern "C" int dfmir_warp_cubic_fwd(int nd, const float* coef, const float* flow, float* out, int B, int C, int D, int H, int W,
                                    void* stream) {
  return cw_launch(nd, false, coef, flow, nullptr, out, B, C, D, H, W, (hipStream_t)stream);
}

extern "C" int dfmir_warp_cubic_bwd_flow(int nd, const float* dout, const float* coef, const float* flow, float* dflow, int B,
                                         int C, int D, int H, int W, void* stream) {
  return cw_launch(nd, true, coef, flow, dout, dflow, B, C, D, H, W, (hipStream_t)stream);
}
