// The tile layout and the plane staging that the fp32 stencil kernels share (bend.hip: bending energy; jacdet.hip:
// Jacobian determinant; gradfield.hip: normalised gradient field).
//
// One workgroup of NT threads = one TY x TX tile of (y, x) of one plane (a (b, c) plane or a sample) and one chunk of
// planes along z that it marches through; wave w owns two rows of the tile, its lanes run along x (every LDS access is
// stride 1 over the lanes).  blockIdx.x counts x tiles fastest, then y tiles, then z chunks, then planes.
//
// A staged plane is the tile with HALO voxels per side, for each of NC channels: ROWS = TY + 2 HALO rows of RS floats in
// LDS, the tile's column x0 at float X0 of its row (16-byte aligned), so voxel (y0 + ly, x0 + lx) of channel c sits at
// c CH + (ly + HALO) RS + X0 + lx.  It travels global -> registers (fetch) -> LDS (commit), so that the next plane is in
// flight while the current one is computed:
//   VEC   (W % 4 == 0 and 16-byte aligned pointers, vec_ok): thread t < ROWS QPR owns the 16-byte quad t % QPR of row
//         t / QPR of the TX interior columns -- x0 and W are multiples of 4, so a quad lies wholly inside or wholly
//         outside the row -- and thread t < 2 HALO ROWS the halo column t % (2 HALO) of row t / (2 HALO): the HALO columns
//         left of the tile, then the HALO right of it.
//   !VEC  NS positions t + NT n of the ROWS x COLS patch per thread, one scalar load each.
// Stage::fetch() reads zero at an address outside the volume, the boundary rule of bend and jacdet.  gradfield's rule is
// the replicate clamp: its GfStage (gradfield.hip) takes the layout and commit() from here and brings a fetch() of its own.
//
// The code generated for these kernels follows the form of this text closely, and the forms below are the ones that
// leave every kernel's instruction stream as it was with a copy of the staging in each file
// (profiles/stencil_tile_refactor.txt):
//   fetch() and tile_of() are templates over the file's geometry struct (members D, H, W, nzc, nty, ntx) and read it in
//   place: with the extents passed as separate ints the kernels came out with other registers and another schedule.
//   The channel loop is a do-while whose condition is the constant false for NC == 1, so that no loop exists there.  Out
//   of a `for` of one trip the compiler hoists the thread's row and column arithmetic, which does not depend on the
//   channel, in front of the `tid <` guards before it unrolls the loop, and the VEC kernels of bend.hip came out 2 to 12 %
//   shorter and scheduled otherwise (not measured).  With the per-channel body in a function or a lambda of its own most
//   kernels of bend.hip and jacdet.hip changed.
// Everything here has internal linkage: each file compiles its own copy.
#pragma once
#include "common.h"

namespace stencil {

constexpr int NT = 256;                      // threads per workgroup: 4 waves x 64 lanes
constexpr int TY = 8, TX = 64;               // tile of (y, x): two rows per wave, one column per lane
constexpr int ZC = 16;                       // planes of a z chunk (gradfield shortens it for small grids)
constexpr int RS = 72;                       // floats per LDS row: column x0 sits at X0 (16-byte aligned)
constexpr int X0 = 4;

// (plane or sample, z chunk, tile origin) of a workgroup; zc = the planes of a z chunk
struct Tile { long long plane; int z0, z1, y0, x0; };
template <class G>
__device__ __forceinline__ Tile tile_of(const G& g, int zc) {
  Tile t;
  unsigned b = blockIdx.x;
  t.x0 = (int)(b % (unsigned)g.ntx) * TX; b /= (unsigned)g.ntx;
  t.y0 = (int)(b % (unsigned)g.nty) * TY; b /= (unsigned)g.nty;
  t.z0 = (int)(b % (unsigned)g.nzc) * zc;
  t.z1 = t.z0 + zc < g.D ? t.z0 + zc : g.D;
  t.plane = b / (unsigned)g.nzc;
  return t;
}

// One plane of NC channels around a tile, with HALO voxels per side: fetch() brings it into registers (zeros outside the
// volume), commit() stores it to NC LDS planes of CH floats.
template <int NC, int HALO, bool VEC>
struct Stage {
  static constexpr int ROWS = TY + 2 * HALO, COLS = TX + 2 * HALO, QPR = TX / 4, CH = ROWS * RS;
  static constexpr int NS = VEC ? 1 : (ROWS * COLS + NT - 1) / NT;
  static_assert(ROWS * QPR <= NT && ROWS * 2 * HALO <= NT, "one quad and one halo value per thread and channel");
  static_assert(X0 >= HALO && X0 + TX + HALO <= RS, "LDS row too short");
  float4 q[NC];
  float s[NC][NS];

  // p: channel 0 of the volume; chs: the channel stride (not read when NC == 1); gz: the plane; y0, x0: the tile
  template <class G>
  __device__ __forceinline__ void fetch(const float* __restrict__ p, const G& g, long long chs, int gz, int y0, int x0) {
    const int tid = threadIdx.x;
    const bool zin = gz >= 0 && gz < g.D;
    const long long zo = zin ? (long long)gz * g.H * g.W : 0LL;
    int c = 0;
#pragma unroll
    do {
      const float* pl = p + c * chs + zo;
      if (VEC) {
        q[c] = make_float4(0.f, 0.f, 0.f, 0.f);
        s[c][0] = 0.f;
        if (tid < ROWS * QPR) {                      // the interior columns
          const int r = tid / QPR, gy = y0 - HALO + r, gx = x0 + 4 * (tid % QPR);
          if (zin && gy >= 0 && gy < g.H && gx < g.W) q[c] = *reinterpret_cast<const float4*>(pl + (long long)gy * g.W + gx);
        }
        if (tid < ROWS * 2 * HALO) {                 // the halo columns
          const int r = tid / (2 * HALO), j = tid % (2 * HALO), gy = y0 - HALO + r;
          const int gx = j < HALO ? x0 - HALO + j : x0 + TX + j - HALO;
          if (zin && gy >= 0 && gy < g.H && gx >= 0 && gx < g.W) s[c][0] = pl[(long long)gy * g.W + gx];
        }
      } else {
#pragma unroll
        for (int n = 0; n < NS; ++n) {
          const int i = tid + n * NT, r = i / COLS, gy = y0 - HALO + r, gx = x0 - HALO + i - r * COLS;
          s[c][n] = 0.f;
          if (i < ROWS * COLS && zin && gy >= 0 && gy < g.H && gx >= 0 && gx < g.W) s[c][n] = pl[(long long)gy * g.W + gx];
        }
      }
    } while (NC > 1 && ++c < NC);
  }

  __device__ __forceinline__ void commit(float* __restrict__ dst) const {
    const int tid = threadIdx.x;
    int c = 0;
#pragma unroll
    do {
      float* d = dst + c * CH;
      if (VEC) {
        if (tid < ROWS * QPR)
          *reinterpret_cast<float4*>(d + (tid / QPR) * RS + X0 + 4 * (tid % QPR)) = q[c];
        if (tid < ROWS * 2 * HALO) {
          const int r = tid / (2 * HALO), j = tid % (2 * HALO);
          d[r * RS + (j < HALO ? X0 - HALO + j : X0 + TX + j - HALO)] = s[c][0];
        }
      } else {
#pragma unroll
        for (int n = 0; n < NS; ++n) {
          const int i = tid + n * NT, r = i / COLS;
          if (i < ROWS * COLS) d[r * RS + X0 - HALO + i - r * COLS] = s[c][n];
        }
      }
    } while (NC > 1 && ++c < NC);
  }
};

// ---- host side
// the tile counts of a volume D x H x W (read from g) with z chunks of zc planes
template <class G>
inline void set_tile_counts(G* g, int zc) {
  g->nzc = (g->D + zc - 1) / zc; g->nty = (g->H + TY - 1) / TY; g->ntx = (g->W + TX - 1) / TX;
}
template <class G>
inline long long wg_per_plane(const G& g) { return (long long)g.nzc * g.nty * g.ntx; }     // workgroups per plane
// may the VEC staging run: W % 4 == 0 and every pointer (NULL: an input that is not there) is 16-byte aligned
template <class... P>
inline bool vec_ok(int W, const P*... p) { return W % 4 == 0 && (((reinterpret_cast<uintptr_t>(p) & 15) == 0) && ...); }

}  // namespace stencil
