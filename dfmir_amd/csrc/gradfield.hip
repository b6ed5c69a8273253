// Normalised-gradient-field similarity (Haber & Modersitzki, MICCAI 2006) of two single-channel images, forward and
// backward, 2-D and 3-D, and the normalised field itself.  Build-defined (include/dfmir_hip.h and losses.GradField_Loss
// state the definition):
//
//   A, B [B][D][H][W] fp32, axes a in the order (z,) y, x of extent n_a with spacing h_a; replicate clamping per sample:
//     g_a(I)(x) = ( I(min(x_a + 1, n_a - 1)) - I(max(x_a - 1, 0)) ) / (2 h_a)        (0 on an axis of extent 1)
//     dot = <g(A), g(B)>,   D_A = |g(A)|^2 + eps_A^2,   D_B = |g(B)|^2 + eps_B^2
//     s(x) = dot^2 / (D_A D_B)  in [0, 1),   s = 0 with no gradient where D_A D_B == 0
//     loss = sum_x m(x) (1 - s(x)) / sum_x m(x)        (m = 1 without a mask; 0 for an empty mask)
//   eps given, or "auto": eps_I = eta * mean over the whole tensor of |g(I)|_2, a constant in the backward.
//   With w(x) = gout m(x) / sum m:
//     G^A(x) = dL/dg(A)(x) = -2 w dot / (D_A D_B) * ( g(B) - (dot / D_A) g(A) ),   G^B the mirror expression
//     dI(y)  = sum_a (1 / 2 h_a) ( [y_a >= 1] G_a(y - e_a) + [y_a == n_a - 1] G_a(y) - [y_a <= n_a - 2] G_a(y + e_a) - [y_a == 0] G_a(y) )
//   the exact adjoint of the clamped difference.
//
// Tiles, z chunks (of g.zc planes) and the layout of a staged plane are those of stencil_tile.h, one sample per workgroup.
// A staged plane holds I at the CLAMPED coordinates (GfStage::fetch), so a difference of two staged neighbours is the
// clamped difference, on the border as in the interior, and every address is inside the volume.
//   gf_pass_k<MODE, VEC>  halo 1, three open planes.  GF_STATS: sum |g(A)|, sum |g(B)|; GF_LOSS: sum m (1 - s), sum m;
//                         in double per thread, one double slot per workgroup and sum, added in a fixed order by the
//                         one-workgroup gf_eps_k / gf_loss_k, which leave eps_A, eps_B and sum m in the workspace (the
//                         main kernels read them there: nothing syncs with the host).  GF_FIELD: writes n(I).
//   gf_bwd_k<VEC>         gather form, no atomics, no G volume in HBM: both images with a halo of 2 (three open planes),
//                         the mask with a halo of 1; G^A, G^B of tile + 1 of ONE plane are formed in LDS (0 outside the
//                         volume, which is what makes the adjoint one expression); a voxel collects the in-plane part
//                         there and carries it, with G_z of the two planes before, in registers to the next plane.
// gf_grad is the ONE place the first differences are formed, gf_sim the one place of dot, D_A, D_B.  The per-voxel
// arithmetic is fp32 (in double the division and the square root made every kernel compute-bound at about 1.2 TB/s of
// its traffic); the sums and eps are double.  Nothing allocates or keeps state; loss, gradients and field are
// bit-identical from run to run.
#include "stencil_tile.h"

using namespace stencil;

namespace {

constexpr int GF_ZC_MIN = 4;               // planes of a z chunk: halved from ZC down to GF_ZC_MIN while the grid stays below
constexpr long long GF_WG_TARGET = 768;    //   GF_WG_TARGET workgroups (three per compute unit; profiles/gradfield_timing.txt)
constexpr int GF_HEAD = 4;                 // doubles at the head of the workspace: eps_A, eps_B, sum m, (unused)

enum { GF_STATS = 0, GF_LOSS = 1, GF_FIELD = 2 };

struct GfGeom {
  int D, H, W;
  int zc, nzc, nty, ntx;                   // planes of a z chunk; z chunks, tiles along y and x
  float cz, cy, cx;                        // 1 / (2 h_a)
};

__device__ __forceinline__ int gf_clamp(int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); }

// One plane of an image around a tile in the layout of stencil::Stage, which stores it to LDS (commit()); fetch() brings
// it into registers at the clamped coordinates.  A tile that ends past W replicates the last column in its quads.
template <int HALO, bool VEC>
struct GfStage : Stage<1, HALO, VEC> {
  using S = Stage<1, HALO, VEC>;
  __device__ __forceinline__ void fetch(const float* __restrict__ ip, const GfGeom& g, int gz, int y0, int x0) {
    const int tid = threadIdx.x;
    const float* pl = ip + (long long)gf_clamp(gz, g.D) * g.H * g.W;
    if (VEC) {
      if (tid < S::ROWS * S::QPR) {                // the interior columns
        const int r = tid / S::QPR, gx = x0 + 4 * (tid % S::QPR);
        const float* row = pl + (long long)gf_clamp(y0 - HALO + r, g.H) * g.W;
        if (gx < g.W) {
          this->q[0] = *reinterpret_cast<const float4*>(row + gx);
        } else {
          const float v = row[g.W - 1];
          this->q[0] = make_float4(v, v, v, v);
        }
      }
      if (tid < S::ROWS * 2 * HALO) {              // the halo columns
        const int r = tid / (2 * HALO), j = tid % (2 * HALO);
        const int gx = j < HALO ? x0 - HALO + j : x0 + TX + j - HALO;
        this->s[0][0] = pl[(long long)gf_clamp(y0 - HALO + r, g.H) * g.W + gf_clamp(gx, g.W)];
      }
    } else {
#pragma unroll
      for (int n = 0; n < S::NS; ++n) {
        const int i = tid + n * NT, r = i / S::COLS;
        if (i < S::ROWS * S::COLS)
          this->s[0][n] = pl[(long long)gf_clamp(y0 - HALO + r, g.H) * g.W + gf_clamp(x0 - HALO + i - r * S::COLS, g.W)];
      }
    }
  }
};

// The first differences at one voxel.  A, B, C point at the voxel in the staged planes z - 1, z, z + 1 (rows of RS).
struct GfVec { float z, y, x; };
__device__ __forceinline__ GfVec gf_grad(const float* A, const float* B, const float* C, const GfGeom& g) {
  GfVec v;
  v.z = (C[0] - A[0]) * g.cz;
  v.y = (B[RS] - B[-RS]) * g.cy;
  v.x = (B[1] - B[-1]) * g.cx;
  return v;
}
__device__ __forceinline__ float gf_sq(const GfVec& v) { return v.z * v.z + v.y * v.y + v.x * v.x; }
// dot, ra = dot / D_A and rb = dot / D_B, both 0 where D_A D_B == 0 (s = ra rb = 0 and no gradient there), ri = 1 / (D_A D_B)
// as the product of the two reciprocals: D_A D_B itself may underflow where neither factor does.
struct GfSim { float dot, ra, rb, ri; };
__device__ __forceinline__ GfSim gf_sim(const GfVec& ga, const GfVec& gb, float ea2, float eb2) {
  GfSim s;
  s.dot = ga.z * gb.z + ga.y * gb.y + ga.x * gb.x;
  const float da = gf_sq(ga) + ea2, db = gf_sq(gb) + eb2;
  const bool ok = da > 0.f && db > 0.f;
  const float ia = ok ? 1.f / da : 0.f, ib = ok ? 1.f / db : 0.f;
  s.ra = s.dot * ia;
  s.rb = s.dot * ib;
  s.ri = ia * ib;
  return s;
}

// ------------------------------------------------------------------------------------------------ statistics, loss, field
// a: the image (GF_FIELD) or the first image; b: the second image (GF_STATS: may be NULL, its sum is then 0).
// wsd: the head of the workspace (eps_A, eps_B; read by GF_LOSS and GF_FIELD).  part: 2 gridDim.x double slots.
// out (GF_FIELD): [B][nch][D][H][W], channel nch - 3 + (0: z, 1: y, 2: x), so that nch = 2 drops z.
template <int MODE, bool VEC>
__global__ __launch_bounds__(NT) void gf_pass_k(const float* __restrict__ a, const float* __restrict__ b,
                                                const float* __restrict__ mask, const double* __restrict__ wsd, GfGeom g,
                                                double* __restrict__ part, float* __restrict__ out, int nch) {
  constexpr int ROWS = TY + 2;
  __shared__ __attribute__((aligned(16))) float sa[3][ROWS * RS];
  __shared__ __attribute__((aligned(16))) float sb[3][MODE == GF_FIELD ? 4 : ROWS * RS]   /* (no second image for the field) */;
  __shared__ double red[NT / 64];
  const Tile t = tile_of(g, g.zc);
  const long long vol = (long long)g.D * g.H * g.W;
  const float* ap = a + t.plane * vol;
  const bool two = MODE != GF_FIELD && b != nullptr;
  const float* bp = two ? b + t.plane * vol : ap;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int x = t.x0 + lane;
  const int c0 = (2 * w + 1) * RS + X0 + lane;                     // the thread's first voxel in a staged plane
  const bool one = g.D == 1;                                    // one plane: staged once, it is its own neighbour in z
  float ea2 = 0.f, eb2 = 0.f;
  if (MODE != GF_STATS) { ea2 = (float)(wsd[0] * wsd[0]); eb2 = (float)(wsd[1] * wsd[1]); }
  GfStage<1, VEC> fa, fb;
  double acc0 = 0.0, acc1 = 0.0;
  int ia = 0, ib = 1, ic = 2;                                    // slots of the planes z - 1, z, z + 1
  if (one) {
    ia = ib = ic = 0;
  } else {
    fa.fetch(ap, g, t.z0 - 1, t.y0, t.x0);
    fa.commit(sa[ia]);
    if (two) { fb.fetch(bp, g, t.z0 - 1, t.y0, t.x0); fb.commit(sb[ia]); }
    fa.fetch(ap, g, t.z0, t.y0, t.x0);
    fa.commit(sa[ib]);
    if (two) { fb.fetch(bp, g, t.z0, t.y0, t.x0); fb.commit(sb[ib]); }
  }
  fa.fetch(ap, g, one ? 0 : t.z0 + 1, t.y0, t.x0);
  if (two) fb.fetch(bp, g, one ? 0 : t.z0 + 1, t.y0, t.x0);
  for (int z = t.z0; z < t.z1; ++z) {
    fa.commit(sa[ic]);
    if (two) fb.commit(sb[ic]);
    __syncthreads();
    if (z + 1 < t.z1) {                                          // in flight while this plane is computed
      fa.fetch(ap, g, z + 2, t.y0, t.x0);
      if (two) fb.fetch(bp, g, z + 2, t.y0, t.x0);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int y = t.y0 + 2 * w + j, c = c0 + j * RS;
      const bool in = y < g.H && x < g.W;
      const long long o = ((long long)z * g.H + y) * g.W + x;
      const GfVec ga = gf_grad(sa[ia] + c, sa[ib] + c, sa[ic] + c, g);
      if (MODE == GF_FIELD) {
        const float d = gf_sq(ga) + ea2;
        const float r = d > 0.f ? 1.f / sqrtf(d) : 0.f;
        if (in) {
          float* op = out + t.plane * nch * vol + o;
          if (nch == 3) op[0] = ga.z * r;
          op[(long long)(nch - 2) * vol] = ga.y * r;
          op[(long long)(nch - 1) * vol] = ga.x * r;
        }
      } else {
        GfVec gb = {0.f, 0.f, 0.f};
        if (two) gb = gf_grad(sb[ia] + c, sb[ib] + c, sb[ic] + c, g);
        if (MODE == GF_STATS) {
          acc0 += (double)(in ? sqrtf(gf_sq(ga)) : 0.f);
          acc1 += (double)(in ? sqrtf(gf_sq(gb)) : 0.f);
        } else {
          const GfSim s = gf_sim(ga, gb, ea2, eb2);
          const float m = in ? (mask ? mask[t.plane * vol + o] : 1.f) : 0.f;
          acc0 += (double)(in ? m * (1.f - s.ra * s.rb) : 0.f);
          acc1 += (double)m;
        }
      }
    }
    __syncthreads();
    if (!one) { const int o = ia; ia = ib; ib = ic; ic = o; }
  }
  if (MODE != GF_FIELD) {
    acc0 = block_sum_ordered<NT>(acc0, red);
    if (threadIdx.x == 0) part[blockIdx.x] = acc0;
    acc1 = block_sum_ordered<NT>(acc1, red);
    if (threadIdx.x == 0) part[gridDim.x + blockIdx.x] = acc1;
  }
}

// (the two sums of the slots, in a fixed order; valid in thread 0)  ONE workgroup.
__device__ __forceinline__ void gf_slot_sums(const double* __restrict__ part, int nslots, double* red, double& s0, double& s1) {
  s0 = s1 = 0.0;
  for (int i = threadIdx.x; i < nslots; i += NT) { s0 += part[i]; s1 += part[nslots + i]; }
  s0 = block_sum_ordered<NT>(s0, red);
  s1 = block_sum_ordered<NT>(s1, red);
}
// eps_A, eps_B into the head of the workspace: eta * (the slots' sums) / count, or the given values when part == NULL.
__global__ __launch_bounds__(NT) void gf_eps_k(const double* __restrict__ part, int nslots, double count, double eta,
                                               double ea, double eb, double* __restrict__ wsd) {
  __shared__ double red[NT / 64];
  if (part) {
    gf_slot_sums(part, nslots, red, ea, eb);
    ea = eta * (ea / count);
    eb = eta * (eb / count);
  }
  if (threadIdx.x == 0) { wsd[0] = ea; wsd[1] = eb; }
}
// out[0] = sum m (1 - s) / sum m (0 for an empty mask); sum m stays in the head of the workspace for the backward.
__global__ __launch_bounds__(NT) void gf_loss_k(const double* __restrict__ part, int nslots, double* __restrict__ wsd,
                                                float* __restrict__ out) {
  __shared__ double red[NT / 64];
  double l, m;
  gf_slot_sums(part, nslots, red, l, m);
  if (threadIdx.x == 0) {
    wsd[2] = m;
    out[0] = m > 0.0 ? (float)(l / m) : 0.f;
  }
}

// ------------------------------------------------------------------------------------------------ backward
// dI(y) = sum_a c_a ( G_a(y - e_a) - G_a(y + e_a) + ([y_a == n_a - 1] - [y_a == 0]) G_a(y) ) with G = 0 outside the volume.
// The G plane holds (TY + 2) x (TX + 2) values (tile + 1), rows of DC floats; sg[3 i + (0: z, 1: y, 2: x)] of image i.
template <bool VEC>
__global__ __launch_bounds__(NT) void gf_bwd_k(const float* __restrict__ a, const float* __restrict__ b,
                                               const float* __restrict__ mask, const float* __restrict__ gout,
                                               const double* __restrict__ wsd, GfGeom g, float* __restrict__ da,
                                               float* __restrict__ db) {
  constexpr int UR = TY + 4, MR = TY + 2, DC = TX + 2, DN = MR * DC;
  __shared__ __attribute__((aligned(16))) float sa[3][UR * RS];
  __shared__ __attribute__((aligned(16))) float sb[3][UR * RS];
  __shared__ __attribute__((aligned(16))) float sm[MR * RS];
  __shared__ float sg[6][DN];
  const Tile t = tile_of(g, g.zc);
  const long long vol = (long long)g.D * g.H * g.W;
  const float* ap = a + t.plane * vol;
  const float* bp = b + t.plane * vol;
  const float* mp = mask ? mask + t.plane * vol : nullptr;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int x = t.x0 + lane;
  const float ea2 = (float)(wsd[0] * wsd[0]), eb2 = (float)(wsd[1] * wsd[1]);
  const float k = wsd[2] > 0.0 ? (float)((double)gout[0] / wsd[2]) : 0.f;       // gout / sum m; an empty mask: zero gradients
  const bool one = g.D == 1;
  const float bx = (float)((x == g.W - 1) - (x == 0));
  GfStage<2, VEC> fa, fb;
  GfStage<1, VEC> fm;
  float pend[2][2], gz1[2][2], gz2[2][2];       // [row j][image]: the in-plane part of plane q - 1; G_z of q - 1 and q - 2
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int i = 0; i < 2; ++i) pend[j][i] = gz1[j][i] = gz2[j][i] = 0.f;

  int s0 = 0, s1 = 1, s2 = 2;                    // image slots of the planes q - 1, q, q + 1
  if (one) {
    s0 = s1 = s2 = 0;
    fa.fetch(ap, g, 0, t.y0, t.x0); fa.commit(sa[0]);
    fb.fetch(bp, g, 0, t.y0, t.x0); fb.commit(sb[0]);
    if (mp) { fm.fetch(mp, g, 0, t.y0, t.x0); fm.commit(sm); }
  } else {
    fa.fetch(ap, g, t.z0 - 2, t.y0, t.x0); fa.commit(sa[s0]);
    fb.fetch(bp, g, t.z0 - 2, t.y0, t.x0); fb.commit(sb[s0]);
    fa.fetch(ap, g, t.z0 - 1, t.y0, t.x0); fa.commit(sa[s1]);
    fb.fetch(bp, g, t.z0 - 1, t.y0, t.x0); fb.commit(sb[s1]);
    fa.fetch(ap, g, t.z0, t.y0, t.x0);
    fb.fetch(bp, g, t.z0, t.y0, t.x0);
    if (mp) fm.fetch(mp, g, t.z0 - 1, t.y0, t.x0);
  }
  for (int q = t.z0 - 1; q <= t.z1; ++q) {       // q: the plane whose G is formed; the output plane is z = q - 1
    if (!one) {
      fa.commit(sa[s2]);
      fb.commit(sb[s2]);
      if (mp) fm.commit(sm);
    }
    __syncthreads();
    if (!one && q < t.z1) {                      // in flight while this plane is computed
      fa.fetch(ap, g, q + 2, t.y0, t.x0);
      fb.fetch(bp, g, q + 2, t.y0, t.x0);
      if (mp) fm.fetch(mp, g, q + 1, t.y0, t.x0);
    }
    const bool qin = q >= 0 && q < g.D;
    for (int i = tid; i < DN; i += NT) {
      const int ly = i / DC, lx = i - ly * DC, gy = t.y0 - 1 + ly, gx = t.x0 - 1 + lx;
      GfVec GA = {0.f, 0.f, 0.f}, GB = {0.f, 0.f, 0.f};
      if (qin && gy >= 0 && gy < g.H && gx >= 0 && gx < g.W) {
        const int c = (ly + 1) * RS + X0 - 1 + lx;
        const GfVec ga = gf_grad(sa[s0] + c, sa[s1] + c, sa[s2] + c, g);
        const GfVec gb = gf_grad(sb[s0] + c, sb[s1] + c, sb[s2] + c, g);
        const GfSim s = gf_sim(ga, gb, ea2, eb2);
        const float m = mp ? sm[ly * RS + X0 - 1 + lx] : 1.f;
        const float coef = -2.f * (k * m) * s.dot * s.ri;
        GA.z = coef * (gb.z - s.ra * ga.z); GA.y = coef * (gb.y - s.ra * ga.y); GA.x = coef * (gb.x - s.ra * ga.x);
        GB.z = coef * (ga.z - s.rb * gb.z); GB.y = coef * (ga.y - s.rb * gb.y); GB.x = coef * (ga.x - s.rb * gb.x);
      }
      sg[0][i] = GA.z; sg[1][i] = GA.y; sg[2][i] = GA.x;
      sg[3][i] = GB.z; sg[4][i] = GB.y; sg[5][i] = GB.x;
    }
    __syncthreads();
    const bool emit = q - 1 >= t.z0;
    const float bz = (float)((q == g.D - 1) - (q == 0));
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int ly = 2 * w + j, y = t.y0 + ly, i = (ly + 1) * DC + lane + 1;
      const float by = (float)((y == g.H - 1) - (y == 0));
      const bool in = y < g.H && x < g.W;
#pragma unroll
      for (int im = 0; im < 2; ++im) {
        float* dp = im == 0 ? da : db;
        if (!dp) continue;                       // only the gradients that are requested
        const float* Gz = sg[3 * im], *Gy = sg[3 * im + 1], *Gx = sg[3 * im + 2];
        const float gzq = Gz[i];
        if (emit && in)
          dp[t.plane * vol + ((long long)(q - 1) * g.H + y) * g.W + x] = pend[j][im] + g.cz * (gz2[j][im] - gzq);
        pend[j][im] = g.cy * (Gy[i - DC] - Gy[i + DC] + by * Gy[i]) + g.cx * (Gx[i - 1] - Gx[i + 1] + bx * Gx[i]) +
                      g.cz * bz * gzq;
        gz2[j][im] = gz1[j][im];
        gz1[j][im] = gzq;
      }
    }
    if (!one) { const int o = s0; s0 = s1; s1 = s2; s2 = o; }
  }
}

// ------------------------------------------------------------------------------------------------ host side
bool gf_finite_pos(double h) { return h > 0.0 && h <= 3.0e38; }        // (false for NaN)

// false for arguments the entry points refuse: nd outside {2, 3}, nd == 2 with D != 1, an extent < 1, a spacing that is
// not positive and finite (hz is not read for nd == 2), or 2^31 and more voxels
bool gf_geom(int nd, int B, int D, int H, int W, float hz, float hy, float hx, GfGeom* g, double* count) {
  if ((nd != 2 && nd != 3) || B < 1 || D < 1 || H < 1 || W < 1 || (nd == 2 && D != 1)) return false;
  if ((nd == 3 && !gf_finite_pos(hz)) || !gf_finite_pos(hy) || !gf_finite_pos(hx)) return false;
  if ((long long)B * D * H * W >= (1LL << 31)) return false;
  g->D = D; g->H = H; g->W = W;
  g->zc = ZC;                              // (a function of the geometry alone: the size query and the calls agree)
  set_tile_counts(g, g->zc);
  while (g->zc > GF_ZC_MIN && B * wg_per_plane(*g) < GF_WG_TARGET) {
    g->zc /= 2;
    set_tile_counts(g, g->zc);
  }
  g->cz = nd == 3 ? (float)(1.0 / (2.0 * (double)hz)) : 0.f;
  g->cy = (float)(1.0 / (2.0 * (double)hy)); g->cx = (float)(1.0 / (2.0 * (double)hx));
  *count = (double)B * D * H * W;
  return true;
}

template <int MODE>
void gf_pass(bool vec, unsigned nwg, hipStream_t st, const float* a, const float* b, const float* mask, const double* wsd,
             const GfGeom& g, double* part, float* out, int nch) {
  if (vec) gf_pass_k<MODE, true><<<nwg, NT, 0, st>>>(a, b, mask, wsd, g, part, out, nch);
  else gf_pass_k<MODE, false><<<nwg, NT, 0, st>>>(a, b, mask, wsd, g, part, out, nch);
}

// eps_A, eps_B into the head of the workspace: the statistics pass and its reduction ("auto"), or the given values
int gf_set_eps(bool vec, unsigned nwg, hipStream_t st, const float* a, const float* b, const GfGeom& g, double count,
               int auto_eps, double eta, double ea, double eb, double* wsd) {
  double* part = wsd + GF_HEAD;
  if (auto_eps) {
    gf_pass<GF_STATS>(vec, nwg, st, a, b, nullptr, wsd, g, part, nullptr, 0);
    DF_LAUNCH_CHECK();
  }
  gf_eps_k<<<1, NT, 0, st>>>(auto_eps ? part : nullptr, (int)nwg, count, eta, ea, eb, wsd);
  DF_LAUNCH_CHECK();
  return 0;
}
inline bool gf_eps_ok(int auto_eps, double eta, double ea, double eb) {
  return auto_eps ? gf_finite_pos(eta) : (gf_finite_pos(ea) && gf_finite_pos(eb));
}

}  // namespace

extern "C" long long dfmir_gradfield_ws_floats(int nd, int B, int D, int H, int W) {
  GfGeom g;
  double count;
  if (!gf_geom(nd, B, D, H, W, 1.f, 1.f, 1.f, &g, &count)) return -1;
  return 2 * (GF_HEAD + 2 * B * wg_per_plane(g));
}

extern "C" int dfmir_gradfield_fwd(const float* a, const float* b, const float* mask, int nd, int B, int D, int H, int W,
                                   float hz, float hy, float hx, int auto_eps, double eta, double eps_a, double eps_b,
                                   float* ws, float* out, void* stream) {
  GfGeom g;
  double count;
  DF_ARG_CHECK(a && b && ws && out && (reinterpret_cast<uintptr_t>(ws) & 7) == 0 && gf_eps_ok(auto_eps, eta, eps_a, eps_b) &&
               gf_geom(nd, B, D, H, W, hz, hy, hx, &g, &count));
  hipStream_t st = (hipStream_t)stream;
  const unsigned nwg = (unsigned)(B * wg_per_plane(g));      // < 2^31
  double* wsd = reinterpret_cast<double*>(ws);
  const bool vec = vec_ok(W, a, b);
  if (int rc = gf_set_eps(vec, nwg, st, a, b, g, count, auto_eps, eta, eps_a, eps_b, wsd)) return rc;
  gf_pass<GF_LOSS>(vec, nwg, st, a, b, mask, wsd, g, wsd + GF_HEAD, nullptr, 0);
  DF_LAUNCH_CHECK();
  gf_loss_k<<<1, NT, 0, st>>>(wsd + GF_HEAD, (int)nwg, wsd, out);
  DF_LAUNCH_CHECK();
  return 0;
}

extern "C" int dfmir_gradfield_bwd(const float* a, const float* b, const float* mask, const float* gout, const float* ws,
                                   float* da, float* db, int nd, int B, int D, int H, int W, float hz, float hy, float hx,
                                   void* stream) {
  GfGeom g;
  double count;
  DF_ARG_CHECK(a && b && gout && ws && (da || db) && (reinterpret_cast<uintptr_t>(ws) & 7) == 0 &&
               gf_geom(nd, B, D, H, W, hz, hy, hx, &g, &count));
  hipStream_t st = (hipStream_t)stream;
  const unsigned nwg = (unsigned)(B * wg_per_plane(g));      // < 2^31
  const double* wsd = reinterpret_cast<const double*>(ws);
  const bool vec = vec_ok(W, a, b, mask);
  if (vec) gf_bwd_k<true><<<nwg, NT, 0, st>>>(a, b, mask, gout, wsd, g, da, db);
  else gf_bwd_k<false><<<nwg, NT, 0, st>>>(a, b, mask, gout, wsd, g, da, db);
  DF_LAUNCH_CHECK();
  return 0;
}

extern "C" int dfmir_gradfield_field(const float* I, int nd, int B, int D, int H, int W, float hz, float hy, float hx,
                                     int auto_eps, double eta, double eps, float* ws, float* out, void* stream) {
  GfGeom g;
  double count;
  DF_ARG_CHECK(I && ws && out && (reinterpret_cast<uintptr_t>(ws) & 7) == 0 && gf_eps_ok(auto_eps, eta, eps, eps) &&
               gf_geom(nd, B, D, H, W, hz, hy, hx, &g, &count));
  hipStream_t st = (hipStream_t)stream;
  const unsigned nwg = (unsigned)(B * wg_per_plane(g));      // < 2^31
  double* wsd = reinterpret_cast<double*>(ws);
  const bool vec = vec_ok(W, I);
  if (int rc = gf_set_eps(vec, nwg, st, I, nullptr, g, count, auto_eps, eta, eps, eps, wsd)) return rc;
  gf_pass<GF_FIELD>(vec, nwg, st, I, nullptr, nullptr, wsd, g, nullptr, out, nd);
  DF_LAUNCH_CHECK();
  return 0;
}
