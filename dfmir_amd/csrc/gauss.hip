// Gaussian smoothing of fields and feature volumes, 2-D and 3-D.  Build-defined (include/dfmir_hip.h and
// ops.gaussian_smooth state the definition):
//
//   x [P][(D)][H][W] fp32, P = B * C planes (or volumes).  Per axis a: r_a = ceil(truncate * sigma_a) <= 16,
//   w_a[k] = exp(-k^2 / (2 sigma_a^2)) for |k| <= r_a (formed on the host in double, rounded to fp32), and along each axis
//   out(i) = sum_k w[k] in(i + k) [i + k inside] / sum_k w[k] [i + k inside]      -- renormalised at the faces: a constant
//   comes back constant.  r_a == 0 (sigma_a == 0) leaves the axis alone, bit for bit.
//
// The pass is bound by HBM, so the kernel is built around how often the tensor crosses it:
//   gs_tile_k<TH, XF>  one workgroup owns a TH x 64 tile of ONE plane [H][W].  The tile with its halo (ry rows above and
//              below; with XF also rx columns left and right, rounded up to 4 so that 16-byte loads stay aligned) goes
//              into LDS, cells outside the plane as zeros.  XF: every staged row is filtered along x into a second LDS tile
//              (the divisor of a column is formed once per thread: a thread keeps its column); then the tile is filtered
//              along y from LDS and leaves with 16-byte stores.  The divisors are sums of the in-plane weights, formed in
//              the kernel.  A sum starts from its centre term and adds the pairs k = 1 .. r, w[k] (in(i - k) + in(i + k)): with
//              r = 0 the value is w[0] v / w[0] = v exactly (w[0] = 1), so a skipped axis needs no second code path.
//   2-D: one launch, <32, true> (LDS 24 + 16 KiB), or <64, false> (24 KiB) when sigma_x == 0.
//   3-D: the (y, x) pass above over the B C D planes, then the z pass as the SAME kernel <64, false> on the view
//        [B C][D][H W]: "rows" are z, "columns" the H W voxels of a plane.  Two reads and two writes of the tensor plus the
//        halo rows, which neighbouring workgroups share through L2.  A pass whose radii are all 0 is not launched (unless
//        it is the only one: the copy).
// 16-byte global accesses where the row length is a multiple of 4 and the pointers are aligned, else the scalar path.  Every
// output is written once by one thread from sums in a fixed order: bit-identical from run to run.  Nothing syncs.
#include "common.h"
#include <math.h>

namespace {

constexpr int GS_T = 256;
constexpr int GS_R = DFMIR_GAUSS_MAX_RADIUS;   // 16
constexpr int GS_TW = 64;

struct GsW { float w[GS_R + 1]; };             // w[|k|]

template <int TH, bool XF, bool VEC>
__global__ __launch_bounds__(GS_T) void gs_tile_k(const float* __restrict__ in, float* __restrict__ out, int H, int W,
                                                  int tiles_x, int tiles_y, int rx, int ry, GsW wx, GsW wy) {
  constexpr int LW = XF ? GS_TW + 2 * GS_R : GS_TW;
  constexpr int LH = TH + 2 * GS_R;
  __shared__ __attribute__((aligned(16))) float tin[LH * LW];
  __shared__ __attribute__((aligned(16))) float tmid[XF ? LH * GS_TW : 4];
  unsigned bid = blockIdx.x;
  const int tx = (int)(bid % (unsigned)tiles_x); bid /= (unsigned)tiles_x;
  const int ty = (int)(bid % (unsigned)tiles_y);
  const long long plane = (long long)(bid / (unsigned)tiles_y);
  const float* ip = in + plane * H * W;
  float* op = out + plane * H * W;
  const int x0 = tx * GS_TW, y0 = ty * TH;
  const int th = min(TH, H - y0);
  const int hx = XF ? (rx + 3) & ~3 : 0;                        // <= GS_R
  const int nrows = th + 2 * ry;                                // <= LH
  const int ncols = GS_TW + 2 * hx;                             // <= LW
  const int tid = threadIdx.x;

  // the tile and its halo; only addresses inside the plane are formed
  if (VEC) {
    const int nq = ncols >> 2;
    for (int i = tid; i < nrows * nq; i += GS_T) {
      const int r = i / nq, q = i - r * nq;
      const int gy = y0 - ry + r, gx = x0 - hx + 4 * q;         // W % 4 == 0: a quad lies inside or outside as a whole
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if ((unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W)
        v = *reinterpret_cast<const float4*>(ip + (long long)gy * W + gx);
      *reinterpret_cast<float4*>(tin + r * LW + 4 * q) = v;
    }
  } else {
    for (int i = tid; i < nrows * ncols; i += GS_T) {
      const int r = i / ncols, c = i - r * ncols;
      const int gy = y0 - ry + r, gx = x0 - hx + c;
      float v = 0.f;
      if ((unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W) v = ip[(long long)gy * W + gx];
      tin[r * LW + c] = v;
    }
  }
  __syncthreads();

  if (XF) {
    // along x: thread tid keeps column tid & 63 and walks the staged rows four apart
    const int c = tid & (GS_TW - 1), gx = x0 + c;
    float den = wx.w[0];
#pragma unroll
    for (int k = 1; k <= GS_R; ++k)
      if (k <= rx) {
        if (gx - k >= 0) den += wx.w[k];
        if (gx + k < W) den += wx.w[k];
      }
    for (int r = tid >> 6; r < nrows; r += GS_T / GS_TW) {
      const float* row = tin + r * LW + hx + c;
      float acc = wx.w[0] * row[0];                             // cells outside the plane hold zeros
#pragma unroll
      for (int k = 1; k <= GS_R; ++k)
        if (k <= rx) acc += wx.w[k] * (row[-k] + row[k]);
      tmid[r * GS_TW + c] = gx < W ? acc / den : 0.f;
    }
    __syncthreads();
  }

  // along y: a thread owns four consecutive columns of a row
  const float* src = XF ? tmid : tin;                           // both GS_TW wide here (LW == GS_TW without XF)
  for (int i = tid; i < th * (GS_TW / 4); i += GS_T) {
    const int row = i >> 4, c = (i & 15) << 2;
    if (x0 + c >= W) continue;
    const int gy = y0 + row;
    float den = wy.w[0];
    const float* col = src + (row + ry) * GS_TW + c;
    float4 acc = *reinterpret_cast<const float4*>(col);
    acc.x *= wy.w[0]; acc.y *= wy.w[0]; acc.z *= wy.w[0]; acc.w *= wy.w[0];
#pragma unroll
    for (int k = 1; k <= GS_R; ++k)
      if (k <= ry) {
        const float w = wy.w[k];
        if (gy - k >= 0) den += w;
        if (gy + k < H) den += w;
        const float4 a = *reinterpret_cast<const float4*>(col - k * GS_TW);
        const float4 b = *reinterpret_cast<const float4*>(col + k * GS_TW);
        acc.x += w * (a.x + b.x); acc.y += w * (a.y + b.y); acc.z += w * (a.z + b.z); acc.w += w * (a.w + b.w);
      }
    acc.x /= den; acc.y /= den; acc.z /= den; acc.w /= den;
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

// r = ceil(truncate * sigma) and the weights of one axis; false for a radius above GS_R
bool gs_weights(double sigma, double truncate, int* r, GsW* w) {
  const double rr = ceil(truncate * sigma);
  if (!(rr <= (double)GS_R)) return false;
  *r = (int)rr;
  for (int k = 0; k <= GS_R; ++k) w->w[k] = 0.f;
  w->w[0] = 1.f;
  for (int k = 1; k <= *r; ++k) w->w[k] = (float)exp(-(double)k * k / (2.0 * sigma * sigma));
  return true;
}

inline bool gs_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// one pass over P planes [H][W]: rows filtered with (ry, wy), columns with (rx, wx)
int gs_pass(const float* in, float* out, long long P, int H, int W, int rx, int ry, const GsW& wx, const GsW& wy,
            hipStream_t st) {
  const bool vec = W % 4 == 0 && gs_al16(in) && gs_al16(out);
  const bool xf = rx > 0;
  const int TH = xf ? 32 : 64;
  const int tiles_x = (W + GS_TW - 1) / GS_TW, tiles_y = (H + TH - 1) / TH;
  const long long nwg = P * tiles_x * tiles_y;
  DF_ARG_CHECK(nwg < (1LL << 31));
#define GS_LAUNCH(TH_, XF_, VEC_) \
  gs_tile_k<TH_, XF_, VEC_><<<(unsigned)nwg, GS_T, 0, st>>>(in, out, H, W, tiles_x, tiles_y, rx, ry, wx, wy)
  if (xf) { if (vec) GS_LAUNCH(32, true, true); else GS_LAUNCH(32, true, false); }
  else { if (vec) GS_LAUNCH(64, false, true); else GS_LAUNCH(64, false, false); }
#undef GS_LAUNCH
  DF_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int dfmir_gauss_smooth(int nd, const float* in, float* out, float* tmp, long long planes, int D, int H, int W,
                                  double sz, double sy, double sx, double truncate, void* stream) {
  DF_ARG_CHECK((nd == 2 || nd == 3) && in && out && in != out && planes >= 1 && H >= 2 && W >= 2 && (nd == 2 || D >= 2));
  if (nd == 2) { D = 1; sz = 0.0; }
  DF_ARG_CHECK(planes * D * H * W < (1LL << 31));
  DF_ARG_CHECK(truncate > 0.0 && truncate < INFINITY && sz >= 0.0 && sy >= 0.0 && sx >= 0.0 && sz < INFINITY &&
               sy < INFINITY && sx < INFINITY);
  int rz, ry, rx;
  GsW wz, wy, wx;
  DF_ARG_CHECK(gs_weights(sz, truncate, &rz, &wz) && gs_weights(sy, truncate, &ry, &wy) && gs_weights(sx, truncate, &rx, &wx));
  hipStream_t st = (hipStream_t)stream;
  const bool pass_z = rz > 0, pass_xy = rx > 0 || ry > 0 || !pass_z;
  DF_ARG_CHECK(!(pass_z && pass_xy) || (tmp && tmp != in && tmp != out));
  if (pass_xy) {
    const int rc = gs_pass(in, pass_z ? tmp : out, planes * D, H, W, rx, ry, wx, wy, st);
    if (rc) return rc;
  }
  if (pass_z) {
    DF_ARG_CHECK((long long)H * W < (1LL << 31));
    GsW none;
    int r0;
    gs_weights(0.0, 1.0, &r0, &none);
    return gs_pass(pass_xy ? tmp : in, out, planes, D, H * W, 0, rz, none, wz, st);
  }
  return 0;
}
