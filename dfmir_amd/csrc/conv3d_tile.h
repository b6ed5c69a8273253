// The tile prologue that the 3-D split conv kernels of conv3ds.hip share: which tile a workgroup owns, the power-of-two
// scales, the lane rotation of the operand reads, and the staging of a tile's halo patch into LDS.
//
// Geometry (conv3d_split_k, conv3d_split_m16_k, conv3d_up_phase_k): output tile TZ x TY x TX = 4 x 8 x 16 voxels, halo
// patch (TZ + 2) x HY x HX = 6 x 10 x 18 positions (offsets -1 .. +1 per axis), chunks of 8 input channels.  One LDS unit
// = the 8 channels of a position as fp16 (16 B); the patch lives in Xs[2 * XP], leading halves at Xs[pos], residual
// halves at Xs[XP + pos], pos = (hz * HY + hy) * HX + hx.  conv3d_up_dgrad_k stages another patch and uses only the
// tile decode, the scales and the lane rotation.
#pragma once
#include "split_f16.h"
#include "common.h"

// DFMIR_CONV3D_FP32 / DFMIR_CONV_FP32: every 3-D split kernel (conv3ds.hip, conv3dsw.hip) declines its layers
static inline bool split3d_off() {
  static DfOptFlag a{"DFMIR_CONV3D_FP32"}, b{"DFMIR_CONV_FP32"};
  return a.get() || b.get();
}

namespace c3tile {
constexpr int TZ = 4, TY = 8, TX = 16, HY = TY + 2, HX = TX + 2;
constexpr int XP = (TZ + 2) * HY * HX;                    // 1080 positions
constexpr int NS = (XP + 255) / 256;                      // 5 position slots per thread (!VEC staging)
// byte offset of a load or store that must not happen: past the range of every buffer descriptor (the launchers keep
// the tensors below 2^31 bytes), so the hardware's bounds check returns zero / drops the store without touching memory
constexpr unsigned OOB = 0x80000000u;
}  // namespace c3tile

// The pieces below are macros, not functions: the compiler simplifies an inlined function on its own before it inlines
// it, and every one of these pieces then came out of the kernels with other instructions and registers.  They expand
// in a kernel that has `using namespace c3tile` (or its own TY, TX), the parameter struct `k` and the locals they name.

// tile id t_ -> n, z0, y0, x0 (batch index, first voxel of the tile).  x runs fastest, then z, then y: the z-halo (2 of
// 6 planes) of a tile is the previous x-row's data, still in the XCD's L2.  k.ny counts groups of TT_ tiles stacked along y.
#define C3TILE_DECODE(t_, TZ_, TT_)                                                               \
  {                                                                                               \
    long long pid_ = (t_);                                                                        \
    const int bx_ = (int)(pid_ % k.nx); pid_ /= k.nx;                                             \
    const int bz_ = (int)(pid_ % k.nz); pid_ /= k.nz;                                             \
    const int by_ = (int)(pid_ % k.ny);                                                           \
    n = (int)(pid_ / k.ny);                                                                       \
    z0 = bz_ * (TZ_); y0 = by_ * TY * (TT_); x0 = bx_ * TX;                                       \
  }

// workgroup -> tiles: the dispatcher deals consecutive workgroup ids round-robin to the 8 XCDs (one L2 each), so ids
// with the same residue get one contiguous eighth of the tiles.
// PERSISTENT: the J = gridDim.x / 8 workgroups of an XCD walk its eighth together (iteration i: tiles i J .. i J + J - 1),
// and the prefetch of a tile's last phase already fetches the first chunk of the workgroup's NEXT tile, so only the
// first tile of a workgroup pays the exposed prologue (a per-phase trace had it at 10-23 % of a one-tile workgroup).
// Declares J, t_first, niter (tiles t_first + i * J, i < niter); a workgroup without tiles returns.
#define C3TILE_XCD_WALK()                                                                         \
  const long long per_xcd = (k.ntile + 7) / 8;                                                    \
  const int J = (int)(gridDim.x >> 3);                                                            \
  const long long t_first = (long long)(blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);            \
  long long t_lim = (long long)((blockIdx.x & 7) + 1) * per_xcd;                                  \
  if (t_lim > k.ntile) t_lim = k.ntile;                                                           \
  if (t_first >= t_lim) return;                                                                   \
  const int niter = (int)((t_lim - t_first + J - 1) / J);
// one tile per workgroup, slot_ = the workgroup's place within its XCD's eighth: declares tile, or returns
#define C3TILE_XCD_TILE(slot_)                                                                    \
  const long long per_xcd = (k.ntile + 7) / 8;                                                    \
  const long long tile = (long long)(blockIdx.x & 7) * per_xcd + (slot_);                         \
  if ((long long)(slot_) >= per_xcd || tile >= k.ntile) return;

// scales: the input is scaled by xscale = 2^ex when it is split (ex from its range probe amax_[0 .. n_ - 1]), the weights
// arrived scaled by 2^ew (w_trailer[0], left by the weight split), the result is rescaled by oscale * oscale2 = 2^-ex * 2^-ew
#define C3TILE_SCALES(amax_, n_)                                                                  \
  const float amax = reduce_absmax(amax_, n_, red);                                               \
  const int ex = scale_exp(amax);                                                                 \
  const int ew = reinterpret_cast<const int*>(w_trailer)[0];                                      \
  const float xscale = pow2f(ex), oscale = pow2f(-ex), oscale2 = pow2f(-ew);

// x of this lane's B positions in the kernels whose column tile j = patch rows 2j, 2j + 1: voxel (row, x) =
// (2j + (l31 >> 4), lx) with lx = l31 & 15 in the even row and (l31 - 2) & 15 in the odd one: with the row stride of 18
// units that rotation puts the 16 lanes a ds_read_b128 serves together ({0-3,12-15,20-27}, {4-11,16-19,28-31}) on 16
// distinct bank quads
#define C3TILE_LANE_X(l31_) (((l31_) - 2 * ((l31_) >> 4)) & 15)

// ---- patch staging ------------------------------------------------------------------------------
// VEC (W % 4 == 0): thread t < 240 owns the 16-B quad q = t & 3 of halo row t >> 2 (rows = 6 planes x 10 y; the quad
// covers patch columns 1 + 4q .. 4 + 4q, i.e. x0 + 4q ..) in all 8 channels of the chunk -- 8 buffer_load_dwordx4 into
// rq[c], converted to 4 LDS units -- and thread t < 120 additionally the left / right halo column (t & 1) of row t >> 1
// (8 buffer_load_dword into rh_[c] -> 1 unit).  SLOTS (any W): NS patch positions tid + 256 s per thread, 8 dword loads
// into rx[s][c] each.  Zero padding comes from the OOB offset, and there are no branches around the loads: a channel
// past Cin (padding of the last chunk, or the chunk after the last) is past the descriptor's range and reads as zero
// without touching memory.
// Locals: unsigned gq, gh (byte offsets of the quad / the halo column within a channel, or OOB), int posq, posh (their
// patch positions, -1: none), unsigned gbyte[NS] (SLOTS), s4 = bytes of one channel, x_src, xscale, Xs.

// the offsets for the tile whose first row is yt0_ (and first plane z0, first column x0)
#define C3TILE_OFFS_VEC(yt0_)                                                                     \
  {                                                                                               \
    gq = OOB; gh = OOB;                                                                           \
    if (tid < 240) {                                                                              \
      const int row = tid >> 2, q = tid & 3;                                                      \
      const int hz = row / HY, hy = row % HY;                                                     \
      const int gz = z0 - 1 + hz, gy = (yt0_) - 1 + hy, gx = x0 + 4 * q;                          \
      posq = row * HX + 1 + 4 * q;                                                                \
      if ((unsigned)gz < (unsigned)k.D && (unsigned)gy < (unsigned)k.H && gx < k.W)               \
        gq = (unsigned)((gz * k.H + gy) * k.W + gx) * 4u;                                         \
    }                                                                                             \
    if (tid < 120) {                                                                              \
      const int row = tid >> 1, side = tid & 1;                                                   \
      const int hz = row / HY, hy = row % HY;                                                     \
      const int gz = z0 - 1 + hz, gy = (yt0_) - 1 + hy, gx = side ? x0 + TX : x0 - 1;             \
      posh = row * HX + (side ? HX - 1 : 0);                                                      \
      if ((unsigned)gz < (unsigned)k.D && (unsigned)gy < (unsigned)k.H && (unsigned)gx < (unsigned)k.W) \
        gh = (unsigned)((gz * k.H + gy) * k.W + gx) * 4u;                                         \
    }                                                                                             \
  }
#define C3TILE_OFFS_SLOTS(yt0_)                                                                   \
  {                                                                                               \
    _Pragma("unroll") for (int s = 0; s < NS; ++s) {                                              \
      const int pos = tid + 256 * s;                                                              \
      unsigned off = OOB;                                                                         \
      if (pos < XP) {                                                                             \
        const int hx = pos % HX, t = pos / HX, hy = t % HY, hz = t / HY;                          \
        const int gz = z0 - 1 + hz, gy = (yt0_) - 1 + hy, gx = x0 - 1 + hx;                       \
        if ((unsigned)gz < (unsigned)k.D && (unsigned)gy < (unsigned)k.H && (unsigned)gx < (unsigned)k.W) \
          off = (unsigned)((gz * k.H + gy) * k.W + gx) * 4u;                                      \
      }                                                                                           \
      gbyte[s] = off;                                                                             \
    }                                                                                             \
  }
// part s_ of chunk ch_'s global loads (VEC: 8 parts = the channels; SLOTS: NS parts = the slots); the compute loops
// spread the parts over their k-steps
#define C3TILE_GLOAD_VEC(ch_, s_, rh_)                                                            \
  {                                                                                               \
    const unsigned co_ = (unsigned)((ch_) * 8 + (s_)) * s4;                                       \
    rq[s_] = __builtin_amdgcn_raw_buffer_load_b128(x_src, gq == OOB ? OOB : gq + co_, 0, 0);      \
    (rh_)[s_] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(x_src, gh == OOB ? OOB : gh + co_, 0, 0)); \
  }
#define C3TILE_GLOAD_SLOTS(ch_, s_)                                                               \
  {                                                                                               \
    const unsigned cbase = (unsigned)((ch_) * 8) * s4;                                            \
    _Pragma("unroll") for (int c = 0; c < 8; ++c)                                                 \
      rx[s_][c] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(                           \
          x_src, gbyte[s_] == OOB ? OOB : gbyte[s_] + cbase + (unsigned)c * s4, 0, 0));           \
  }
// the loaded chunk, scaled by xscale and split, to the patch in LDS
#define C3TILE_LSTORE_VEC(rh_)                                                                    \
  {                                                                                               \
    if (posq >= 0) {                                                                              \
      _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                             \
        float v[8];                                                                               \
        _Pragma("unroll") for (int c = 0; c < 8; ++c) v[c] = __uint_as_float(rq[c][e]);           \
        u32x4 h, r;                                                                               \
        split8_scaled(v, xscale, h, r);                                                           \
        Xs[posq + e] = h;                                                                         \
        Xs[XP + posq + e] = r;                                                                    \
      }                                                                                           \
    }                                                                                             \
    if (posh >= 0) {                                                                              \
      u32x4 h, r;                                                                                 \
      split8_scaled(rh_, xscale, h, r);                                                           \
      Xs[posh] = h;                                                                               \
      Xs[XP + posh] = r;                                                                          \
    }                                                                                             \
  }
#define C3TILE_LSTORE_SLOTS()                                                                     \
  {                                                                                               \
    _Pragma("unroll") for (int s = 0; s < NS; ++s) {                                              \
      const int pos = tid + 256 * s;                                                              \
      if (pos < XP) {                                                                             \
        u32x4 h, r;                                                                               \
        split8_scaled(rx[s], xscale, h, r);                                                       \
        Xs[pos] = h;                                                                              \
        Xs[XP + pos] = r;                                                                         \
      }                                                                                           \
    }                                                                                             \
  }
// both forms, for the kernels that are templated on VEC and declare the locals of both (the halo column in rx[0])
#define C3TILE_OFFS(VEC_, yt0_)                                                                   \
  {                                                                                               \
    const int yt0v_ = (yt0_);                                                                     \
    if constexpr (VEC_) C3TILE_OFFS_VEC(yt0v_) else C3TILE_OFFS_SLOTS(yt0v_)                      \
  }
#define C3TILE_GLOAD(VEC_, ch_, s_) { if constexpr (VEC_) C3TILE_GLOAD_VEC(ch_, s_, rx[0]) else C3TILE_GLOAD_SLOTS(ch_, s_) }
#define C3TILE_LSTORE(VEC_) { if constexpr (VEC_) C3TILE_LSTORE_VEC(rx[0]) else C3TILE_LSTORE_SLOTS() }
