// The split weight gradient of the 3-D 3x3x3 stride-1 convolutions whose forward and data-gradient kernels are in
// conv3ds.hip: conv3d_wgrad_tr_k and the entry points that choose between it and the marchers of conv3duw.hip,
// conv3dwm.hip and conv3dt.hip.
// ================================================================================================
// wgrad:  dWt[tap][ci][co] += sum_v X[ci][v + tap] * dY[co][v]   with the VOXEL as the MFMA K (16 consecutive x).
// MFMA rows = (tap, ci) of a chunk of 8 input channels (27 x 8 = 216 -> 7 row tiles of 32), columns = co; one atomicAdd
// per accumulator at the very end (split-K over workgroups).
// ================================================================================================
#include "conv3d_tile.h"

struct W3sP {
  int N, Cin, Cout, D, H, W;
  int nz, ny, nx;
  long long npatch, per_block;
  long long nslot;               // tr kernel: workgroups per XCD along grid.x (per_block = tiles per XCD)
  int x_n, dy_n;
  int nchunk;                    // chunks of 8 input channels in the layer; blockIdx.y * NCH = this workgroup's first
  long long s_tap, s_row, s_col; // output index = tap' * s_tap + ci * s_row + co * s_col, tap' = flip ? 26 - tap : tap
  int flip;
  float* db;                     // optional bias gradient: db[.] += sum over voxels of the layer's output gradient
  int db_from_x;                 // 0: db indexed by co, summed from the dY operand;  1: by ci, from the X operand (swapped roles)
  // X = cat(nearest_up2(xa), x) never materialised (tr kernel): channels 0 .. Ca - 1 are read from the HALF-resolution
  // tensor xa [N, Ca, D/2, H/2, W/2] at (z >> 1, y >> 1, x >> 1), the remaining Cin - Ca from x [N, Cin - Ca, D, H, W]
  const float* xa;
  int Ca;
  const float* fx;               // deterministic mode (common.h df_acc): dwt holds 64-bit fixed-point sums, db is NULL
};

// ================================================================================================
// wgrad, transpose-read form:  the operands are read from the FORWARD kernel's LDS images with ds_read_b64_tr_b16
// (gfx950): X as [position][8 channels x fp16]
// (16 B per position and split), dY as [voxel][32 output channels x fp16] (64 B).  In a 16-lane group the hardware
// hands lane 4q + c, element j the c-th fp16 at the address supplied by lane 4j + q: with lane (j, q) pointing at
// (voxel j, channel quad q) every lane receives 4 consecutive voxels of its own row -- a K-major MFMA operand out of a
// channel-major image.  A tap is then nothing but a position offset (16-B granular, so dx shifts stay aligned): ONE
// copy of the patch serves all 27 taps, and the patch is staged exactly like the forward kernel's (8 x
// buffer_load_dwordx4 per thread, 4 v_fma_mix per value pair).
//
// Workgroup = 4 waves, persistent over 2 x 8 x 16-voxel tiles (16 k-steps = x-rows of 16 voxels); per tile the dY
// image is staged once and the X patch (4 x 10 x 18 positions) once per 8-channel chunk.  Row tile T of a chunk =
// taps 4T .. 4T+3 x 8 channels (7 tiles, tap 27 is padding); wave w owns tiles (w + c) & 3 and that + 4 of chunk c
// (accumulators of <= 3 chunks resident: 96 AGPRs, two workgroups per CU so that one stages while the other computes).
// Bank behaviour of the reads: the 32 lanes served together cover 4 taps x 4 x-positions x 16 B; taps of one
// (dz, dy) are contiguous, the next (dz, dy) must start 112..192 B further (mod 256): row stride 25 positions, plane
// stride 250 -- odd, so that the staging stores of 4 consecutive rows x 2 quads (one ds_write_b128 lane group) fall on
// 8 different 16-B bank slots (measured: all of the kernel's bank conflicts were these stores at stride 24).  dY: 4 voxels x 64 B contiguous; the channel group is XORed with (voxel >> 2) & 3 so that the staging
// stores of a wave (one channel group, 4 voxel quads) spread over the banks.
// ================================================================================================
#ifndef W3T_NOSKIP
#define W3T_NOSKIP 0
#endif
#ifndef W3T_KO
#define W3T_KO 0     // knock-out builds for timing: 1 = no MFMAs, 2 = no prefetch loads, 4 = no convert + LDS store, 8 = no operand reads
#endif

template <int NCH>
struct W3T {
  static constexpr int TZ = 2, TY = 8, TX = 16, HZ = 4, HY = 10, HXP = 25, SZP = HY * HXP;
  static constexpr int XPOS = HZ * SZP;                  // 1000 units per split
  static constexpr int YU = TZ * TY * TX * 4;            // 1024 units per split
};

// PAIR form (<= 16 output channels: half of the 32 MFMA columns would be padding): the columns are (plane p, co) --
// columns 0-15 take dY of the tile's z-plane 0, columns 16-31 the SAME voxel (y, x) of plane 1 -- and K runs over
// plane 0 only (8 k-steps).  Rows then are (tap', ci) with tap' = (dz' in 0..3, dy, dx) over the patch's four planes:
// row (dz', .) x column (p, .) is a term of dW[dz' - p] (dropped where dz' - p is outside 0..2): 9 row tiles x 8
// k-steps instead of 7 x 16.  A wave owns tiles w and w + 4 and k-steps 2w, 2w + 1 of tile 8 (the partial sums meet
// in the atomics of the epilogue): 18 tile-steps per wave and phase instead of 32.
// UPCAT: X = cat(nearest_up2(xa), x) read in place (see W3sP::xa).  A compile-time variant: a branch around the operand
// prefetch splits the k-loop's basic block and with it the MFMA / LDS / VMEM interleave (measured: +35 % on every shape),
// so both sources are loaded branch-free -- the inactive one with an out-of-range offset (returns 0, no memory access).
template <int NCH, bool PAIR, bool UPCAT>
__global__ __launch_bounds__(256, 2) void conv3d_wgrad_tr_k(const float* __restrict__ x, const float* __restrict__ x_amax,
                                                         const float* __restrict__ dy, const float* __restrict__ dy_amax,
                                                         float* __restrict__ dwt, W3sP k) {
  using G = W3T<NCH>;
  constexpr int TZ = G::TZ, TY = G::TY, HY = G::HY, HXP = G::HXP, SZP = G::SZP, XPOS = G::XPOS, YU = G::YU;
  constexpr unsigned OOB = 0x80000000u;
  __shared__ u32x4 Xs[2 * XPOS];
  __shared__ u32x4 Ys[2 * YU];
  __shared__ float red[17];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int l31 = lane & 31, hi = lane >> 5;
  const long long S = (long long)k.D * k.H * k.W;
  const unsigned s4 = (unsigned)S * 4u;

  const int ex = scale_exp(reduce_absmax(x_amax, k.x_n, red));
  __syncthreads();
  const int ed = scale_exp(reduce_absmax(dy_amax, k.dy_n, red));
  const float xscale = pow2f(ex), dscale = pow2f(ed), oscale = pow2f(-ex), oscale2 = pow2f(-ed);

  constexpr int NA = PAIR ? 3 : 2;                         // accumulators (row tiles) per chunk and wave
  constexpr int NKS = PAIR ? 8 : 16;                       // k-steps per phase
  f32x16 acc[NCH][NA];
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int s = 0; s < NA; ++s)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[c][s][r] = 0.f;

  const int c_base = blockIdx.y * NCH;
  int nc = k.nchunk - c_base;                              // chunks of this workgroup row
  if (nc > NCH) nc = NCH;
  // Tiles: workgroup ids go round-robin to the 8 XCDs (one L2 each), so XCD e = id & 7 owns the e-th eighth of the
  // tile list and its J workgroups (slot j = id >> 3) walk it together: in iteration i they hold the J consecutive
  // tiles i J .. i J + J - 1 of the eighth.  The list runs x fastest, then over 2 x 2 blocks of (z, y): a window of J
  // tiles is a few full x-rows of neighbouring (z, y), so the halos (3.75x the tile in the patch) are mostly L2 hits.
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const long long t_first = (long long)xcd * k.per_block + slot;       // per_block = tiles per XCD
  long long t_lim = (long long)(xcd + 1) * k.per_block;
  if (t_lim > k.npatch) t_lim = k.npatch;
  const int J = (int)k.nslot;
  if (t_first >= t_lim || nc <= 0) return;
  const int niter = (int)((t_lim - t_first + J - 1) / J);

  // ---- staging roles.  X: thread t < 240 owns the aligned quad qq (x0 - 4 + 4 qq ..) of halo row t / 6 (40 rows of
  // 6 quads; quads 0 and 5 contribute one position each) in the 8 channels of the chunk.  dY: wave w owns channel
  // group w, thread = (row 0..15, quad 0..3) of the tile.
  const bool xt = tid < 240;
  const int xm = tid / 80, xr80 = tid - 80 * xm;           // quad pair m = 0..2; 8 consecutive lanes = 4 rows x 2 quads
  const int xrow = xr80 >> 1, xqq = 2 * xm + (xr80 & 1);
  const int xhz = xrow / HY, xhy = xrow - HY * xhz;
  const int xpos0 = xhz * SZP + xhy * HXP + 4 * xqq - 3;   // unit of element e: xpos0 + e
  const int xe0 = xqq == 0 ? 3 : 0, xe1 = xqq == 5 ? 1 : 4;
  const int yq = tid & 3, yrow = (tid >> 2) & 15;
  const bool yt = wid * 8 < k.Cout;
  // unit of element e: yunit0 + 4 e  (PAIR: plane 1 takes the other 32-B half of the voxel's 64 B, so that the columns
  // of both planes, read together, fall on different banks)
  const int yunit0 = (yrow * 16 + 4 * yq) * 4 + (wid ^ yq ^ (PAIR ? (yrow >> 3) * 2 : 0));
  const bool db_y = k.db && !k.db_from_x && blockIdx.y == 0 && yt;
  const bool db_x = k.db && k.db_from_x && xt && xhz >= 1 && xhz <= TZ && xhy >= 1 && xhy <= TY && xqq >= 1 && xqq <= 4;
  float bacc[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) bacc[c] = 0.f;

  // ---- operand addresses (bytes in LDS).  Source role of this lane in its 16-lane group: j = voxel, q = channel quad.
  const int sj = (lane & 15) >> 2, sq = lane & 3, sg = (lane >> 4) & 1;
  const unsigned xs_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)Xs;
  const unsigned ys_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)Ys;
  // B (dY): voxel = s * 16 + 8 hi + 4 i + j, channel quad = 4 sg + sq -> unit (2 sg + (sq >> 1)) ^ ((2 hi + i) & 3)
  // PAIR: column group sg = plane, voxel + 128 sg, channel quad sq -> unit (sq >> 1) ^ ((2 hi + i) & 3) ^ 2 sg
  unsigned baddr[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
    baddr[i] = PAIR ? ys_base + (unsigned)(((128 * sg + 8 * hi + 4 * i + sj) * 4 + ((sq >> 1) ^ ((2 * hi + i) & 3) ^ (2 * sg))) * 16 + (sq & 1) * 8)
                    : ys_base + (unsigned)(((8 * hi + 4 * i + sj) * 4 + ((2 * sg + (sq >> 1)) ^ ((2 * hi + i) & 3))) * 16 + (sq & 1) * 8);

  u32x4 rq[8], ry[8];
  int tn, tz, ty, tx;                                      // tile being LOADED (runs one phase ahead of the compute)
  const int nzb = (k.nz + 1) >> 1;
  const int cells = 4 * nzb * ((k.ny + 1) >> 1);           // (z, y) cells per image incl. the phantom ones of odd counts
#define W3T_DECODE(t_)                                                                            \
  {                                                                                               \
    long long q_ = (t_);                                                                          \
    tx = (int)(q_ % k.nx); q_ /= k.nx;                                                            \
    const int u_ = (int)(q_ % cells);                                                             \
    tn = (int)(q_ / cells);                                                                       \
    const int b_ = u_ >> 2;                                                                       \
    tz = 2 * (b_ % nzb) + (u_ & 1);                                                               \
    ty = 2 * (b_ / nzb) + ((u_ >> 1) & 1);                                                        \
  }
  W3T_DECODE(t_first)
  unsigned gq = OOB, gy_ = OOB, gqa = OOB;
  __amdgpu_buffer_rsrc_t x_src, y_src, xa_src;
  const int Cup = UPCAT ? k.Ca : 0;                         // channels taken from the half-resolution tensor
  const int Dh = k.D >> 1, Hh = k.H >> 1, Wh = k.W >> 1;
  const unsigned sa4 = (unsigned)((long long)Dh * Hh * Wh) * 4u;
#define W3T_TILE_ADDR()                                                                           \
  {                                                                                               \
    const int z0 = tz * TZ, y0 = ty * TY, x0 = tx * 16;                                           \
    x_src = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x + (long long)tn * (k.Cin - Cup) * S), 0,   \
                                              (unsigned)((long long)(k.Cin - Cup) * S * 4), 0x00020000);  \
    if (UPCAT) xa_src = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(k.xa + (long long)tn * Cup * (sa4 >> 2)), 0,   \
                                                        (unsigned)((long long)Cup * sa4), 0x00020000);  \
    y_src = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(dy + (long long)tn * k.Cout * S), 0, \
                                              (unsigned)((long long)k.Cout * S * 4), 0x00020000); \
    {                                                                                             \
      const int gz = z0 - 1 + xhz, gyy = y0 - 1 + xhy, gx = x0 - 4 + 4 * xqq;                     \
      gq = (xt && tz < k.nz && ty < k.ny && (unsigned)gz < (unsigned)k.D && (unsigned)gyy < (unsigned)k.H && (unsigned)gx < (unsigned)k.W) \
               ? (unsigned)((gz * k.H + gyy) * k.W + gx) * 4u : OOB;                              \
      gqa = (UPCAT && gq != OOB) ? (unsigned)(((gz >> 1) * Hh + (gyy >> 1)) * Wh + (gx >> 1)) * 4u : OOB;   \
    }                                                                                             \
    {                                                                                             \
      const int gz = z0 + (yrow >> 3), gyy = y0 + (yrow & 7), gx = x0 + 4 * yq;                   \
      gy_ = (yt && tz < k.nz && ty < k.ny && gz < k.D && gyy < k.H && gx < k.W) ? (unsigned)((gz * k.H + gyy) * k.W + gx) * 4u : OOB; \
    }                                                                                             \
  }
#define W3T_GLOAD_X1(ca_, c_)                                                                     \
  if constexpr (UPCAT) {     /* a chunk lies entirely in one of the two tensors (Ca % 8 == 0): wave-uniform selects */ \
    typedef unsigned u32x2w_ __attribute__((ext_vector_type(2)));                                 \
    const bool up_ = (ca_) * 8 < Cup;                                                             \
    const u32x2w_ v2_ = __builtin_amdgcn_raw_buffer_load_b64(                                     \
        xa_src, (up_ && gqa != OOB) ? gqa + (unsigned)((ca_) * 8 + (c_)) * sa4 : OOB, 0, 0);      \
    const u32x4 v4_ = __builtin_amdgcn_raw_buffer_load_b128(                                      \
        x_src, (!up_ && gq != OOB) ? gq + (unsigned)((ca_) * 8 + (c_) - Cup) * s4 : OOB, 0, 0);   \
    rq[c_] = u32x4{v2_[0] | v4_[0], v2_[0] | v4_[1], v2_[1] | v4_[2], v2_[1] | v4_[3]};           \
  } else {                                                                                        \
    rq[c_] = __builtin_amdgcn_raw_buffer_load_b128(x_src, gq == OOB ? OOB : gq + (unsigned)((ca_) * 8 + (c_)) * s4, 0, 0); \
  }
#define W3T_GLOAD_Y1(c_)                                                                          \
  ry[c_] = __builtin_amdgcn_raw_buffer_load_b128(y_src, gy_ == OOB ? OOB : gy_ + (unsigned)(wid * 8 + (c_)) * s4, 0, 0);
#define W3T_STORE_X()                                                                             \
  if (xt) {                                                                                       \
    _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                               \
      if (e < xe0 || e >= xe1) continue;                                                          \
      u32x4 h, r;                                                                                 \
      _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                             \
        unsigned hh, rr;                                                                          \
        split_pair_scaled(__uint_as_float(rq[2 * q][e]), __uint_as_float(rq[2 * q + 1][e]), xscale, hh, rr); \
        h[q] = hh; r[q] = rr;                                                                     \
      }                                                                                           \
      Xs[xpos0 + e] = h;                                                                          \
      Xs[XPOS + xpos0 + e] = r;                                                                   \
    }                                                                                             \
    if (db_x) {                                                                                   \
      _Pragma("unroll") for (int c = 0; c < 8; ++c)                                               \
        bacc[c] += (__uint_as_float(rq[c][0]) + __uint_as_float(rq[c][1])) + (__uint_as_float(rq[c][2]) + __uint_as_float(rq[c][3])); \
    }                                                                                             \
  }
#define W3T_STORE_Y()                                                                             \
  if (yt) {                                                                                       \
    _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                               \
      u32x4 h, r;                                                                                 \
      _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                             \
        unsigned hh, rr;                                                                          \
        split_pair_scaled(__uint_as_float(ry[2 * q][e]), __uint_as_float(ry[2 * q + 1][e]), dscale, hh, rr); \
        h[q] = hh; r[q] = rr;                                                                     \
      }                                                                                           \
      Ys[yunit0 + 4 * e] = h;                                                                     \
      Ys[YU + yunit0 + 4 * e] = r;                                                                \
    }                                                                                             \
    if (db_y) {                                                                                   \
      _Pragma("unroll") for (int c = 0; c < 8; ++c)                                               \
        bacc[c] += (__uint_as_float(ry[c][0]) + __uint_as_float(ry[c][1])) + (__uint_as_float(ry[c][2]) + __uint_as_float(ry[c][3])); \
    }                                                                                             \
  }
  // operands of k-step s_ (x-row (z, y) = (s_ >> 3, s_ & 7)) into register set b_
  // Operand reads of k-step s_ (x-row (z, y) = (s_ >> 3, s_ & 7)).  A (one row tile) is single-buffered and fetched one
  // HALF-step ahead -- tile 1's while tile 0's three MFMAs run and vice versa -- B (shared by both tiles) is
  // double-buffered and fetched one step ahead: 32 operand registers instead of 48 (three chunks of accumulators +
  // both staging sets + 48 did not fit 256 registers).
  // (the two reads of a pair stay spelled out at this one site: through tr_pair the PAIR instances of this kernel come out
  // of the compiler with another schedule of their address arithmetic)
#define W3T_TR_PAIR64(dst_, addr_)                                                                \
  {                                                                                               \
    const uint2 u0_ = tr_read(addr_), u1_ = tr_read((addr_) + 64u);                               \
    dst_ = u32x4{u0_.x, u0_.y, u1_.x, u1_.y};                                                     \
  }
#define W3T_READ_A(t_, s_)                                                                        \
  {                                                                                               \
    const unsigned ko = (unsigned)((((s_) >> 3) * SZP + ((s_) & 7) * HXP) * 16);                  \
    W3T_TR_PAIR64(A1[t_], aaddr[t_] + ko + XPOS * 16u)                                            \
    W3T_TR_PAIR64(A0[t_], aaddr[t_] + ko)                                                         \
  }
#define W3T_READ_B(B_, b_, s_, off_)                                                              \
  B_[b_] = tr_pair(baddr[0] + (unsigned)(s_) * 1024u + (off_), baddr[1] + (unsigned)(s_) * 1024u + (off_));
  // the 16 k-steps of chunk c_ (LAST_: the next phase starts a new tile, so dY is prefetched too -- a wave-uniform
  // branch around one load per step; two copies of the loop behind one branch cost 32 registers of accumulator copies)
#define W3T_KLOOP(c_, LAST_)                                                                      \
  {                                                                                               \
    W3T_READ_B(B0, 0, 0, 0u) W3T_READ_B(B1, 0, 0, YU * 16u) W3T_READ_A(0, 0)                      \
    __builtin_amdgcn_sched_barrier(0);                                                            \
    _Pragma("unroll") for (int s = 0; s < NKS; ++s) {                                             \
      const int cur = s & 1;                                                                      \
      if (!(W3T_KO & 8)) {                                                                        \
        if (tok1) { W3T_READ_A(1, s) }                                                            \
        if (s + 1 < NKS) W3T_READ_B(B0, cur ^ 1, s + 1, 0u)                                       \
      }                                                                                           \
      if (!(W3T_KO & 2)) {                                                                        \
        if (s < 8) { W3T_GLOAD_X1(ca_next, s); }                                                  \
        else if (LAST_) { W3T_GLOAD_Y1(s - 8); }                                                  \
      }                                                                                           \
      W3T_MMA(c_, 0)                                                                              \
      __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);                                          \
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                          \
      __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);                                          \
      __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);                                          \
      __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);                                          \
      __builtin_amdgcn_sched_barrier(0);                                                          \
      if (s + 1 < NKS && !(W3T_KO & 8)) {                                                         \
        W3T_READ_A(0, s + 1)                                                                      \
        W3T_READ_B(B1, cur ^ 1, s + 1, YU * 16u)                                                  \
      }                                                                                           \
      if (PAIR && (LAST_) && !(W3T_KO & 2)) { W3T_GLOAD_Y1(s); }   /* 8 k-steps: dY rides in the second half-steps */ \
      if (tok1) { W3T_MMA(c_, 1) }                                                                \
      __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);                                          \
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                          \
      __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);                                          \
      if (PAIR) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);                                \
      __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);                                          \
      __builtin_amdgcn_sched_barrier(0);                                                          \
    }                                                                                             \
    if constexpr (PAIR) {                                                                         \
      /* tile 8, k-steps 2 wid and 2 wid + 1 (wave-uniform offsets: one add per address) */        \
      _Pragma("unroll") for (int u = 0; u < 2; ++u) {                                             \
        const unsigned ko = (unsigned)((2 * wid + u) * HXP * 16), kb = (unsigned)(2 * wid + u) * 1024u; \
        A1[u] = tr_pair(aaddr[2] + ko + XPOS * 16u, aaddr[2] + ko + XPOS * 16u + 64u);            \
        A0[u] = tr_pair(aaddr[2] + ko, aaddr[2] + ko + 64u);                                      \
        B0[u] = tr_pair(baddr[0] + kb, baddr[1] + kb);                                            \
        B1[u] = tr_pair(baddr[0] + kb + YU * 16u, baddr[1] + kb + YU * 16u);                      \
      }                                                                                           \
      _Pragma("unroll") for (int u = 0; u < 2; ++u) {                                             \
        acc[c_][NA - 1] = mfma32_f16(A1[u], B0[u], acc[c_][NA - 1]);                              \
        acc[c_][NA - 1] = mfma32_f16(A0[u], B1[u], acc[c_][NA - 1]);                              \
        acc[c_][NA - 1] = mfma32_f16(A0[u], B0[u], acc[c_][NA - 1]);                              \
      }                                                                                           \
      __builtin_amdgcn_sched_barrier(0);                                                          \
    }                                                                                             \
  }
#if (W3T_KO & 1)
#define W3T_MMA(c_, t) acc[c_][t][0] += __uint_as_float(A1[t][0] ^ B0[cur][1] ^ A0[t][2] ^ B1[cur][3]);
#else
#define W3T_MMA(c_, t)                                                                            \
  acc[c_][t] = mfma32_f16(A1[t], B0[cur], acc[c_][t]);                                            \
  acc[c_][t] = mfma32_f16(A0[t], B1[cur], acc[c_][t]);                                            \
  acc[c_][t] = mfma32_f16(A0[t], B0[cur], acc[c_][t]);
#endif

  u32x4 A0[2], A1[2], B0[2], B1[2];
  unsigned aaddr[NA];

  // prologue: first tile's dY and chunk 0
  W3T_TILE_ADDR();
#pragma unroll
  for (int c = 0; c < 8; ++c) { W3T_GLOAD_X1(c_base, c); W3T_GLOAD_Y1(c); }
  W3T_STORE_X();
  W3T_STORE_Y();
  __syncthreads();

  for (int it = 0; it < niter; ++it) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      if (c >= nc) continue;
      const bool last = (c + 1 == nc);                     // the next phase starts a new tile (or nothing)
      const bool more = !last || (it + 1 < niter);
      if (last) {                                          // advance the load cursor to the next tile
        if (more) { W3T_DECODE(t_first + (long long)(it + 1) * J) W3T_TILE_ADDR(); } else { gq = OOB; gy_ = OOB; }
      }
      const int ca_next = last ? c_base : c_base + c + 1;
      // this wave's two row tiles of chunk c: lane (j, q, g) of tile T supplies tap 4T + 2g + (q >> 1), channel quad q & 1
#pragma unroll
      for (int t = 0; t < NA; ++t) {
        const int tile = PAIR ? (t < 2 ? wid + 4 * t : 8) : ((wid + c) & 3) + 4 * t;
        int tap = tile * 4 + 2 * sg + (sq >> 1);           // PAIR: tap' of 36 (dz' = tap' / 9 in 0..3)
        if (!PAIR && tap > 26) tap = 26;                   // padding rows: any valid address (results discarded)
        const int dz = tap / 9, dyy = (tap / 3) % 3, dx = tap % 3;
        aaddr[t] = xs_base + (unsigned)((dz * SZP + dyy * HXP + dx + 8 * hi + sj) * 16 + (sq & 1) * 8);
      }
      // the wave whose second row tile is the padding tile 7 skips its reads and MFMAs (wave-uniform): no time gained
      // (the phase ends at the barrier) but 1/8 of the matrix and LDS energy of a kernel that sits on the power cap
      const bool tok1 = PAIR || (((wid + c) & 3) != 3) || W3T_NOSKIP;
      W3T_KLOOP(c, last)
      if (more) {
        __syncthreads();
        if (!(W3T_KO & 4)) {
          W3T_STORE_X();
          if (last) W3T_STORE_Y();
        }
        __syncthreads();
      }
    }
  }
#undef W3T_TILE_ADDR
#undef W3T_DECODE
#undef W3T_GLOAD_X1
#undef W3T_GLOAD_Y1
#undef W3T_STORE_X
#undef W3T_STORE_Y
#undef W3T_TR_PAIR64
#undef W3T_READ_A
#undef W3T_READ_B
#undef W3T_KLOOP
#undef W3T_MMA

  // ---- epilogue: acc[c][s][r] <-> row (r>>2)*8 + hi*4 + (r&3) of tile ((wid+c)&3) + 4s, column co = l31
  const float sc = oscale * oscale2;
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int s = 0; s < NA; ++s) {
      const int tile = PAIR ? (s < 2 ? wid + 4 * s : 8) : ((wid + c) & 3) + 4 * s;
      const int co = PAIR ? (l31 & 15) : l31, pl = PAIR ? (l31 >> 4) : 0;
      if (c >= nc || (!PAIR && tile >= 7) || co >= k.Cout) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rho = tile * 32 + (r >> 2) * 8 + hi * 4 + (r & 3);
        int tap = rho >> 3;
        const int ci = (c_base + c) * 8 + (rho & 7);
        bool ok = ci < k.Cin;
        if constexpr (PAIR) {
          const int dz = tap / 9 - pl;                     // row plane dz' against column plane p
          ok = ok && (unsigned)dz < 3u;
          tap = dz * 9 + tap % 9;
        } else {
          ok = ok && rho < 216;
        }
        const int to = k.flip ? 26 - tap : tap;
        if (ok) df_acc(dwt, to * k.s_tap + ci * k.s_row + co * k.s_col, acc[c][s][r] * sc, k.fx);
      }
    }
  if (k.db) {                                              // wave-uniform: every lane of a wave holds the same 8 channels
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const float t = wave_sum((db_y || db_x) ? bacc[c] : 0.f);
      const int ch = k.db_from_x ? c_base * 8 + c : wid * 8 + c;
      const int lim = k.db_from_x ? k.Cin : k.Cout;
      if (lane == 0 && ch < lim && t != 0.f) atomicAdd(&k.db[ch], t);
    }
  }
}

static bool split3d_wgrad_common_ok(const DfConvGeom* g) {
  return g->KD == 3 && g->KH == 3 && g->KW == 3 && g->stride == 1 && g->dil == 1 && g->pd == 1 && g->ph == 1 &&
         g->pw == 1 && g->pad_mode == 0 && g->Do == g->Di && g->Ho == g->Hi && g->Wo == g->Wi && g->Di > 1 &&
         (g->Wi & 3) == 0 && (long long)g->Cin * g->Di * g->Hi * g->Wi * 4 < 0x7FFFFFFFLL &&
         (long long)g->Cout * g->Di * g->Hi * g->Wi * 4 < 0x7FFFFFFFLL;
}
// normal roles: rows = (tap, ci), columns = co.  Few output channels (the 16 -> 3 flow conv): SWAPPED roles -- rows =
// (tap, co) gathered from shifted dY, columns = ci: dW[t][ci][co] = sum_u X[ci][u] * dY[co][u - t], i.e. the same kernel
// on (x := dY, dy := X) with the taps flipped and the output transposed (one 8-channel chunk instead of Cin / 8).
static bool split3d_wgrad_geom_ok(const DfConvGeom* g) {
  return split3d_wgrad_common_ok(g) && g->Cin >= 8 && g->Cin <= 128 && g->Cout >= 8 && g->Cout <= 32;
}
static bool split3d_wgrad_swapped_ok(const DfConvGeom* g) {
  return split3d_wgrad_common_ok(g) && g->Cout >= 1 && g->Cout < 8 && g->Cin >= 8 && g->Cin <= 32;
}
extern "C" int dfmir_conv3d_split_wgrad_ok(const DfConvGeom* g) {
  return (g && !split3d_off() && (split3d_wgrad_geom_ok(g) || split3d_wgrad_swapped_ok(g))) ? 1 : 0;
}
static int conv3d_split_wgrad_impl(const DfConvGeom* g, const float* x, const float* x_amax, int x_amax_n,
                                   const float* dy, const float* dy_amax, int dy_amax_n, float* dw_tcc, float* db,
                                   void* stream, const float* xa = nullptr, int Ca = 0, long long s_tap_full = 0);
// The weight gradient of conv3x3x3 over X = cat(nearest_up2(a), b) without building X: a [N, Ca, D/2, H/2, W/2] is read
// at (z >> 1, y >> 1, x >> 1) while the operand patch is staged.  g: the full layer (Cin = Ca + Cb); Ca % 8 == 0; even
// D, H, W; x_amax: a range probe valid for both parts.
extern "C" int dfmir_conv3d_split_wgrad_upcat(const DfConvGeom* g, const float* a, const float* b, int Ca,
                                              const float* x_amax, int x_amax_n, const float* dy, const float* dy_amax,
                                              int dy_amax_n, float* dw_tcc, float* db, void* stream) {
  DF_ARG_CHECK(g && a && b && Ca > 0 && (Ca & 7) == 0 && Ca < g->Cin && !(g->Di & 1) && !(g->Hi & 1) && !(g->Wi & 7));
  DF_ARG_CHECK(split3d_wgrad_geom_ok(g) && (reinterpret_cast<uintptr_t>(a) & 7) == 0);
  return conv3d_split_wgrad_impl(g, b, x_amax, x_amax_n, dy, dy_amax, dy_amax_n, dw_tcc, db, stream, a, Ca);
}
// The same gradient with the up-sampled channels in PARITY CLASSES (conv3duw.hip: 8 / 27 of their products, one pass over
// dY at 1.0 x) and the skip channels b on the direct kernel, which also carries the bias gradient.  Ca == 32 (every
// decoder level of the VoxelMorph U-Net), Cout a multiple of 8 up to 32.  ws: dfmir_conv3d_upwgrad_ws_floats() floats,
// private to the stream while the call is in flight.
int df_conv3d_upwgrad_launch(const float* a, const float* a_amax, int a_n, const float* b, const float* dy, const float* dy_amax,
                             int dy_n, float* dwt, long long s_tap, float* db, float* ws, int N, int Dl, int Hl, int Wl,
                             int Cout, hipStream_t st);
int df_conv3d_wgrad_march_launch(const float* x, const float* x_amax, int x_n, const float* dy, const float* dy_amax, int dy_n,
                                 float* dwt, float* db, int N, int D, int H, int W, hipStream_t st);
int df_conv3d_flow_wgrad_ok(const DfConvGeom* g, const float* x, const float* dy);
int df_conv3d_flow_wgrad_launch(const float* x, const float* x_amax, int x_n, const float* dy, const float* dy_amax, int dy_n,
                                float* dwt, float* db, int N, int D, int H, int W, int Cout, hipStream_t st);
static bool wgrad_march_geom_ok(const DfConvGeom* g) {
  static DfOptFlag nomarch_o{"DFMIR_CONV3D_NO_WGRAD_MARCH"};
  return g->Cin == 32 && g->Cout == 16 && !split3d_off() && split3d_wgrad_geom_ok(g) && !nomarch_o.get() &&
         (long long)g->Di * g->Hi * g->Wi >= 4096;
}
// what the launcher decides: the geometry AND 16-byte aligned operands (x, dy are read as quads)
static bool wgrad_march_takes(const DfConvGeom* g, const float* x, const float* dy) {
  return wgrad_march_geom_ok(g) && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(dy)) & 15) == 0;
}
// 1 when dfmir_conv3d_split_wgrad / _db take the marching kernel for this layer (csrc/conv3dwm.hip): _is_march answers
// for 16-byte aligned operands, _is_march_at for the operands given (the SAME predicate the launcher applies)
extern "C" int dfmir_conv3d_wgrad_is_march(const DfConvGeom* g) { return (g && wgrad_march_geom_ok(g)) ? 1 : 0; }
extern "C" int dfmir_conv3d_wgrad_is_march_at(const DfConvGeom* g, const float* x, const float* dy) {
  return (g && wgrad_march_takes(g, x, dy)) ? 1 : 0;
}
static bool upwgrad_geom_ok(const DfConvGeom* g, int Ca) {
  return !split3d_off() && split3d_wgrad_common_ok(g) && Ca == 32 && g->Cin > Ca && g->Cin - Ca <= 128 &&
         g->Cout >= 8 && g->Cout <= 32 && (g->Cout & 7) == 0 && !(g->Di & 1) && !(g->Hi & 1) && !(g->Wi & 7);
}
extern "C" int dfmir_conv3d_upwgrad_ok(const DfConvGeom* g, int Ca) { return (g && upwgrad_geom_ok(g, Ca)) ? 1 : 0; }
extern "C" long long dfmir_conv3d_upwgrad_ws_floats(void) { return 2 * 72LL * 1024; }   // (64-bit slots in deterministic mode)
extern "C" int dfmir_conv3d_upwgrad(const DfConvGeom* g, const float* a, const float* b, int Ca, const float* x_amax,
                                    int x_amax_n, const float* dy, const float* dy_amax, int dy_amax_n, float* dw_tcc,
                                    float* db, float* ws, void* stream) {
  DF_ARG_CHECK(g && a && b && ws && x_amax && x_amax_n > 0 && dy && dy_amax && dy_amax_n > 0 && dw_tcc);
  DF_ARG_CHECK(upwgrad_geom_ok(g, Ca) && (reinterpret_cast<uintptr_t>(a) & 15) == 0 && (reinterpret_cast<uintptr_t>(b) & 7) == 0 &&
               (reinterpret_cast<uintptr_t>(dy) & 15) == 0);   // 8-byte pair loads of a and b, 16-byte quads of dY
  const long long s_tap = (long long)g->Cin * g->Cout;
  // two skip channels (the network's input images at the top level): fused into the same launch, with the bias gradient
  const bool fuse = g->Cin - Ca == 2;
  const int rc = df_conv3d_upwgrad_launch(a, x_amax, x_amax_n, fuse ? b : nullptr, dy, dy_amax, dy_amax_n, dw_tcc, s_tap,
                                          fuse ? db : nullptr, ws, g->N, g->Di / 2, g->Hi / 2, g->Wi / 2, g->Cout,
                                          (hipStream_t)stream);
  if (rc || fuse) return rc;
  DfConvGeom gb = *g;
  gb.Cin = g->Cin - Ca;
  return conv3d_split_wgrad_impl(&gb, b, x_amax, x_amax_n, dy, dy_amax, dy_amax_n, dw_tcc + (df_det_fx() ? 2LL : 1LL) * Ca * g->Cout, db,   // (deterministic mode: 8-byte slots)
                                 stream, nullptr, 0, s_tap);
}
extern "C" int dfmir_conv3d_split_wgrad(const DfConvGeom* g, const float* x, const float* x_amax, int x_amax_n,
                                        const float* dy, const float* dy_amax, int dy_amax_n, float* dw_tcc,
                                        void* stream) {
  return conv3d_split_wgrad_impl(g, x, x_amax, x_amax_n, dy, dy_amax, dy_amax_n, dw_tcc, nullptr, stream);
}
extern "C" int dfmir_conv3d_split_wgrad_db(const DfConvGeom* g, const float* x, const float* x_amax, int x_amax_n,
                                           const float* dy, const float* dy_amax, int dy_amax_n, float* dw_tcc,
                                           float* db, void* stream) {
  return conv3d_split_wgrad_impl(g, x, x_amax, x_amax_n, dy, dy_amax, dy_amax_n, dw_tcc, db, stream);
}
static int conv3d_split_wgrad_impl(const DfConvGeom* g, const float* x, const float* x_amax, int x_amax_n,
                                   const float* dy, const float* dy_amax, int dy_amax_n, float* dw_tcc, float* db,
                                   void* stream, const float* xa, int Ca, long long s_tap_full) {
  DF_ARG_CHECK(g && x && x_amax && x_amax_n > 0 && dy && dy_amax && dy_amax_n > 0 && dw_tcc);
  // s_tap_full: the rows of a wider gradient [27][Ctot][Cout] (dw_tcc points at this operand's first row): the skip
  // channels of dfmir_conv3d_upwgrad, any Cin >= 1 (a partial 8-channel chunk reads zeros beyond Cin)
  const bool rows = s_tap_full > 0 && split3d_wgrad_common_ok(g) && g->Cin >= 1 && g->Cin <= 128 && g->Cout >= 8 && g->Cout <= 32;
  DF_ARG_CHECK(!split3d_off() && (rows || split3d_wgrad_geom_ok(g) || split3d_wgrad_swapped_ok(g)));
  hipStream_t st = (hipStream_t)stream;
  // the full-resolution 32 -> 16 layer: all 27 tap matrices resident, z-marching (conv3dwm.hip)
  if (!rows && !xa && wgrad_march_takes(g, x, dy))
    return df_conv3d_wgrad_march_launch(x, x_amax, x_amax_n, dy, dy_amax, dy_amax_n, dw_tcc, db, g->N, g->Di, g->Hi, g->Wi, st);
  const bool swapped = !rows && !split3d_wgrad_geom_ok(g);
  // the flow head 16 -> 3: (co, dx) pairs as MFMA columns, z-marching (conv3dt.hip)
  if (swapped && !xa && df_conv3d_flow_wgrad_ok(g, x, dy))
    return df_conv3d_flow_wgrad_launch(x, x_amax, x_amax_n, dy, dy_amax, dy_amax_n, dw_tcc, db, g->N, g->Di, g->Hi, g->Wi, g->Cout, st);
  W3sP k{};
  k.fx = df_det_fx();
  k.N = g->N; k.D = g->Di; k.H = g->Hi; k.W = g->Wi;
  k.xa = xa; k.Ca = xa ? Ca : 0;
  if (swapped) {
    k.Cin = g->Cout; k.Cout = g->Cin;                        // kernel roles
    k.s_tap = (long long)g->Cin * g->Cout; k.s_row = 1; k.s_col = g->Cout; k.flip = 1;
    k.x_n = dy_amax_n; k.dy_n = x_amax_n;
    k.db = db; k.db_from_x = 1;
  } else {
    k.Cin = g->Cin; k.Cout = g->Cout;
    k.s_tap = rows ? s_tap_full : (long long)g->Cin * g->Cout; k.s_row = g->Cout; k.s_col = 1; k.flip = 0;
    k.x_n = x_amax_n; k.dy_n = dy_amax_n;
    k.db = db; k.db_from_x = 0;
  }
  k.nz = (g->Di + 1) / 2; k.ny = (g->Hi + 7) / 8; k.nx = (g->Wi + 15) / 16;
  // <= 3 chunks of accumulators per workgroup (96 AGPRs + staging registers: two workgroups per CU, so that one
  // converts while the other computes); more input channels = a second workgroup row, which stages dY again
  k.nchunk = (k.Cin + 7) / 8;
  const bool pairw = !swapped && k.Cout <= 16;   // (kernel roles) plane-pair columns: 3 accumulators per chunk (swapped flow head: measured slower, 0.44 vs 0.31 ms)
  const int per_wg = pairw ? (k.nchunk < 2 ? k.nchunk : 2) : (k.nchunk <= 3 ? k.nchunk : (k.nchunk == 4 ? 2 : 3));
  const unsigned gy = (unsigned)((k.nchunk + per_wg - 1) / per_wg);
  // the tile list includes the phantom (z, y) cells of odd tile counts (they load nothing); 8 XCD shares, nslot
  // workgroups each (see the kernel), about 512 workgroups in all
  k.npatch = (long long)g->N * k.nx * 4 * ((k.nz + 1) / 2) * ((k.ny + 1) / 2);
  k.per_block = (k.npatch + 7) / 8;
  k.nslot = (long long)(512 / gy / 8);
  if (k.nslot > k.per_block) k.nslot = k.per_block;
  if (k.nslot < 1) k.nslot = 1;
  const unsigned nbx = (unsigned)(8 * k.nslot);
  const float *kx = swapped ? dy : x, *kxa = swapped ? dy_amax : x_amax, *kdy = swapped ? x : dy, *kda = swapped ? x_amax : dy_amax;
#define W3S_LAUNCH(N_)                                                                            \
  {                                                                                               \
    if (xa) conv3d_wgrad_tr_k<N_, false, true><<<dim3(nbx, gy), 256, 0, st>>>(kx, kxa, kdy, kda, dw_tcc, k);   \
    else conv3d_wgrad_tr_k<N_, false, false><<<dim3(nbx, gy), 256, 0, st>>>(kx, kxa, kdy, kda, dw_tcc, k);   \
  }
  if (pairw && per_wg == 1 && xa) conv3d_wgrad_tr_k<1, true, true><<<dim3(nbx, gy), 256, 0, st>>>(kx, kxa, kdy, kda, dw_tcc, k);
  else if (pairw && xa) conv3d_wgrad_tr_k<2, true, true><<<dim3(nbx, gy), 256, 0, st>>>(kx, kxa, kdy, kda, dw_tcc, k);
  else if (pairw && per_wg == 1) conv3d_wgrad_tr_k<1, true, false><<<dim3(nbx, gy), 256, 0, st>>>(kx, kxa, kdy, kda, dw_tcc, k);
  else if (pairw) conv3d_wgrad_tr_k<2, true, false><<<dim3(nbx, gy), 256, 0, st>>>(kx, kxa, kdy, kda, dw_tcc, k);
  else if (per_wg == 1) W3S_LAUNCH(1)
  else if (per_wg == 2) W3S_LAUNCH(2)
  else W3S_LAUNCH(3)
#undef W3S_LAUNCH
  DF_LAUNCH_CHECK();
  return 0;
}
