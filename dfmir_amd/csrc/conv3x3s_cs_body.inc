// Body of conv3x3_split_cs_k (conv3x3s.hip), included once into that kernel and once into conv3x3_bwd_pair_k -- as TEXT, not as
// a function: a __device__ function, even a forced-inline one, is canonicalised on its own before it is inlined, without what a
// kernel knows about its workgroup ids, and both kernels came out slower that way (the weight gradient by 1.4 %).
// The including scope provides: CPG, TH (constants); x, ws, bias, y, k (ConvCsP), sc (SplitScale);
// bix, biy, gdx (int: the workgroup's index in the logical grid of gdx x (1 or 2) workgroups);
// Wg[2][WUG], Xs[2][NSP * 2 * XP], bs[2 * CPG] in LDS (arrays or pointers to arrays: CsLds<CPG, TH>).
  static_assert((CPG == 64 && TH == 8) || (CPG == 32 && TH == 16), "tile forms");
  constexpr int CS_TH = TH;
  constexpr int NSP = 2, XP = CsLds<CPG, TH>::XP, NPOS = (CS_TH + 2) * CS_PW;
  constexpr int WUG = NSP * 9 * 2 * CPG;                  // 16-B units of one group's weight chunk (16 channels)
  constexpr int NW = (WUG + 255) / 256;                   // 9 (CPG 64) / 5 (CPG 32, the last one half used) per thread
  constexpr int NS = (NPOS + 255) / 256;                  // 2 / 3 patch positions per thread
  static_assert(WUG == CsLds<CPG, TH>::WUG && NSP * 2 * XP == CsLds<CPG, TH>::XSU, "arena layout");
#ifdef CS_TRACE
  __shared__ unsigned trc[8 * 32 * 8];
  const bool trace_blk = bix == 300 && biy == 0;
  const unsigned long long trc_t0 = __builtin_readcyclecounter(), trc_r0 = wall_clock64();
#endif

  // wave-uniform by construction; readfirstlane tells the compiler so (otherwise every buffer load whose
  // descriptor depends on the group is wrapped in a waterfall loop)
  const int grp = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 8));
  const int tid = threadIdx.x & 255, lane = tid & 63, wid = tid >> 6;
  const int l31 = lane & 31, lhi = lane >> 5;
  const int HWo = k.Ho * k.Wo, HWi = k.Hi * k.Wi;
  if (k.dephase > 0 && biy == 0 && bix < 256) {
    const unsigned long long t0 = wall_clock64();
    const unsigned wait = (unsigned)bix * (unsigned)k.dephase >> 8;
    while ((unsigned)(wall_clock64() - t0) < wait) __builtin_amdgcn_s_sleep(4);
  }
  WGT(0)
#ifdef CS_TRACE
  if (threadIdx.x == 0 && bix < 2048 && biy == 0) {
    g_cs_wg[bix * 6 + 4] = __builtin_amdgcn_s_getreg(63492);       // HW_REG_HW_ID
    g_cs_wg[bix * 6 + 5] = __builtin_amdgcn_s_getreg(63508);       // HW_REG_XCC_ID
  }
#endif
  int bt = bix, bm = biy;
  if (k.xcd_pair == 1) { bm = (bt >> 3) & 1; bt = ((bt >> 4) << 3) + (bt & 7); }
  else if (k.xcd_pair >= 2) {   // XCD e = id & 7 walks a contiguous eighth of the tiles; xcd_pair - 1 cout slices of a tile back to back
    const int ny = k.xcd_pair - 1, per = (gdx >> 3) / ny, j = bt >> 3;
    bm = j % ny;
    bt = (bt & 7) * per + j / ny;
  }
  const int tx = bt % k.tiles_x; bt /= k.tiles_x;
  const int ty = bt % k.tiles_y;
  const int n = bt / k.tiles_y;
  const int oy0 = ty * CS_TH, ox0 = tx * CS_TW;
  const int m0 = bm * (2 * CPG), m0g = m0 + CPG * grp;

  const int ex = scale_exp(reduce_absmax(sc.x_amax, sc.x_n, bs));     // bs: scratch here, bias below
  __syncthreads();
  const int ew = (int)sc.w_trailer[1];
  const float xscale = pow2f(ex), oscale = pow2f(-ex), oscale2 = pow2f(-ew);

  constexpr unsigned OOB = 0x80000000u;
  // this thread's patch positions: byte offset of channel ch of its 8-channel half, within a 16-channel slab
  unsigned gvo[NS][8];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int pos = tid + 256 * s;
    int off = -1;
    if (pos < NPOS) {
      const int r = pos / CS_PW, c = pos - r * CS_PW;
      off = halo_offset(oy0 - k.pad + r, ox0 - k.pad + c, k.Hi, k.Wi, k.pad_mode);
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) gvo[s][c] = off < 0 ? OOB : (unsigned)(off + (8 * grp + c) * HWi) * 4u;
  }
  if (threadIdx.x < 2 * CPG) bs[threadIdx.x] = (bias && (m0 + (int)threadIdx.x) < k.Cout) ? bias[m0 + threadIdx.x] : 0.f;

  // MFMA operand indices: wave w of a group owns 32 couts (w & 1) x tile rows 4(w >> 1) .. +3
  const int rowgrp = CPG == 64 ? (wid >> 1) : wid;        // this wave's 4 tile rows
  const int xb = lhi * XP + 4 * rowgrp * CS_PW + l31;
  const int abase = lhi * CPG + l31 + (CPG == 64 ? 32 * (wid & 1) : 0);

  f32x16 acc[4];                                          // [row]
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

  const float* xn = x + (long long)n * k.Cin * HWi;
  const int chunks8 = (k.Cin + 7) / 8, chunks = (k.Cin + 15) / 16;
  // weight unit idx = r*64 + co with r = (split*9 + tap)*2 + half; global unit ((2c + half)*NSP*9 + split*9 + tap)*Cout + cout
  unsigned wb[NW];
#pragma unroll
  for (int j = 0; j < NW; ++j) {
    const int idx = tid + 256 * j;
    const int co = m0g + (idx % CPG), r = idx / CPG;
    const int half = r & 1, st = r >> 1;
    wb[j] = (idx < WUG && co < k.Cout) ? (unsigned)((half * NSP * 9 + st) * k.Cout + co) * 16u : OOB;
  }
  const int wunits8 = NSP * 9 * k.Cout;                   // units of one 8-channel chunk in the packed weights

  u32x4 rw[NW];
  unsigned rx[NS][8];
#define CS_GLOADW(c_)                                                                            \
  {                                                                                              \
    const int q_ = 2 * (c_);                                                                     \
    const int left_ = chunks8 - q_;                                                              \
    const __amdgpu_buffer_rsrc_t rw_ = __builtin_amdgcn_make_buffer_rsrc(                        \
        const_cast<u32x4*>(ws + (long long)q_ * wunits8), 0,                                     \
        left_ > 0 ? (unsigned)((left_ < 2 ? left_ : 2) * wunits8) * 16u : 0u, 0x00020000);       \
    _Pragma("unroll") for (int j = 0; j < NW; ++j) rw[j] = __builtin_amdgcn_raw_buffer_load_b128(rw_, wb[j], 0, 0); \
  }
#define CS_GLOADX(c_)                                                                            \
  {                                                                                              \
    const int c0_ = 16 * (c_);                                                                   \
    const int left_ = k.Cin - c0_;                                                               \
    const __amdgpu_buffer_rsrc_t rx_ = __builtin_amdgcn_make_buffer_rsrc(                        \
        const_cast<float*>(xn + (long long)c0_ * HWi), 0,                                        \
        left_ > 0 ? (unsigned)((left_ < 16 ? left_ : 16) * HWi) * 4u : 0u, 0x00020000);          \
    _Pragma("unroll") for (int s = 0; s < NS; ++s)                                               \
      _Pragma("unroll") for (int c = 0; c < 8; ++c)                                              \
        rx[s][c] = __builtin_amdgcn_raw_buffer_load_b32(rx_, gvo[s][c], 0, 0);                   \
  }
#define CS_LSTOREW()                                                                             \
  { _Pragma("unroll") for (int j = 0; j < NW; ++j) if (WUG % 256 == 0 || tid + 256 * j < WUG) Wg[grp][tid + 256 * j] = rw[j]; }
#define CS_LSTOREX(buf_)                                                                         \
  {                                                                                              \
    _Pragma("unroll") for (int s = 0; s < NS; ++s) {                                             \
      const int pos = tid + 256 * s;                                                             \
      if (pos < NPOS) {                                                                          \
        float v[8];                                                                              \
        _Pragma("unroll") for (int c = 0; c < 8; ++c) v[c] = __uint_as_float(rx[s][c]);          \
        CS_NORM_PROBE_OPS()                                                                      \
        u32x4 sp[NSP];                                                                           \
        split8_s<NSP>(v, xscale, sp);                                                                      \
        _Pragma("unroll") for (int q = 0; q < NSP; ++q) Xs[buf_][(q * 2 + grp) * XP + pos] = sp[q]; \
      }                                                                                          \
    }                                                                                            \
  }

  // CS_NORM_PROBE (lab builds, scripts/build_var.sh): what an InstanceNorm + ReLU applied while the patch is staged would
  // cost the converting wave group -- one fma and one max per value with run-time operands that happen to be the identity
  // (x * 1 + 0, max with -3e38: results unchanged, instructions real; profiles/r06_cs_norm_probe.txt)
#ifdef CS_NORM_PROBE
  const float np_r = fmaf(oscale2, 0.f, 1.f), np_m = oscale2 * 0.f, np_lo = fmaf(oscale2, 0.f, -3.0e38f);
#define CS_NORM_PROBE_OPS() _Pragma("unroll") for (int c = 0; c < 8; ++c) v[c] = fmaxf(fmaf(v[c], np_r, np_m), np_lo);
#else
#define CS_NORM_PROBE_OPS()
#endif
  // prologue: X(0) (each group its channel half) and W_A(0) in place; B holds W_B(0), X-half-1(1) in registers
  CS_GLOADX(0);
  if (grp == 0) CS_GLOADW(0);
  CS_LSTOREX(0);
  if (grp == 0) CS_LSTOREW();
  if (grp == 1) { CS_GLOADW(0); CS_GLOADX(1); }
  __syncthreads();
  WGT(1)

  for (int h = 0; h < 2 * chunks; ++h) {
    const int c = h >> 1;
    TRC(0)
    if ((h & 1) == grp) {
      // compute chunk c; the prefetch (chunks past the end read zeros) rides behind the MFMAs
      __builtin_amdgcn_s_setprio(CS_COMPUTE_PRIO);
      const int qw_ = 2 * (c + 1), lw_ = chunks8 - qw_;
      const __amdgpu_buffer_rsrc_t rwd = __builtin_amdgcn_make_buffer_rsrc(
          const_cast<u32x4*>(ws + (long long)qw_ * wunits8), 0,
          lw_ > 0 ? (unsigned)((lw_ < 2 ? lw_ : 2) * wunits8) * 16u : 0u, 0x00020000);
      const int cx_ = 16 * (c + 1 + grp), lx_ = k.Cin - cx_;
      const __amdgpu_buffer_rsrc_t rxd = __builtin_amdgcn_make_buffer_rsrc(
          const_cast<float*>(xn + (long long)cx_ * HWi), 0,
          lx_ > 0 ? (unsigned)((lx_ < 16 ? lx_ : 16) * HWi) * 4u : 0u, 0x00020000);
      cs_mma_chunk_rr<CPG, XP, NW, NS>(Wg[grp], Xs[c & 1], abase, xb, acc, rwd, wb, rw, rxd, gvo, rx);
    } else {
      // store what this group prefetched during its last compute half-step (B at h = 0: the prologue's)
      __builtin_amdgcn_s_setprio(CS_STORE_PRIO);
      {
#ifdef CS_TRACE
      __builtin_amdgcn_s_waitcnt(0x0f70);                 // vmcnt(0): separates the load wait from the convert + store
      TRC(3)
#endif
#ifdef CS_TRACE
      CS_LSTOREW();
      TRC(4)
      if (c + 1 < chunks) CS_LSTOREX((c + 1) & 1);
#else
      if (grp == 0) {
        if (c + 1 < chunks) { CS_LSTOREW(); CS_LSTOREX((c + 1) & 1); }
      } else {
        CS_LSTOREW();
        if (c + 1 < chunks) CS_LSTOREX((c + 1) & 1);
      }
#endif
      }
    }
    TRC(1)
    // the last half-step is group 1's compute of the last chunk: group 0 has nothing left to stage and goes straight to
    // its epilogue (its 64 KB of stores leave beside group 1's MFMAs instead of after them: a CU stores at ~12 B/clk)
#ifndef CS_NO_EARLY_EPI
    if (h + 1 < 2 * chunks)
#endif
    __syncthreads();
    TRC(2)
  }
  WGT(2)
#ifdef CS_TRACE
  if (trace_blk) {
    __syncthreads();
    for (int i = threadIdx.x; i < 8 * 32 * 8; i += 512) g_cs_trace[i] = trc[i];
    if (threadIdx.x == 0) {
      const unsigned long long t1 = __builtin_readcyclecounter(), r1 = wall_clock64();
      g_cs_trace[2048] = (unsigned)trc_t0; g_cs_trace[2049] = (unsigned)t1;
      g_cs_trace[2050] = (unsigned)trc_r0; g_cs_trace[2051] = (unsigned)r1;
    }
  }
#endif
#undef CS_GLOADW
#undef CS_GLOADX
#undef CS_LSTOREW
#undef CS_LSTOREX
#undef CS_NORM_PROBE_OPS

  // Epilogue.  The MFMAs ran with rows = the 32 pixels of a tile row and columns = 32 output channels, so a lane holds
  // ONE output channel (l31) and, per accumulator quad q, the 4 consecutive pixels 8q + 4 lhi .. + 3 of each of its 4 tile
  // rows: 16 16-byte stores per lane instead of 64 4-byte ones (the store tail of a workgroup is bound by the number of
  // store instructions: 8.9 us of an 84-us workgroup with dword stores).  vec4 needs Wo % 4 == 0 and 16-byte aligned bases.
  float* yb = y + (long long)n * k.Cout * HWo;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const int i = CPG == 32 ? 0 : (wid & 1);                     // 32-cout block of the group's couts
    const int row = 4 * rowgrp + b;
    const int oy = oy0 + row;
    const int cc = CPG * grp + i * 32 + l31, co = m0 + cc;
#ifdef CS_KO_EPI
    if (oy >= k.Ho || co >= k.Cout || acc[b][0] != 12345.678f) continue;    // knock-out: no epilogue loads / stores
#else
    if (oy >= k.Ho || co >= k.Cout) continue;
#endif
    const float bv = bs[cc], osc = oscale * oscale2;
    const long long rowoff = (long long)co * HWo + (long long)oy * k.Wo;
    const float* rb = k.res ? k.res + (long long)n * k.Cout * HWo + rowoff : nullptr;
    const float* rg = k.ring ? k.ring + ((long long)n * 4 * k.Cout + co) * k.ring_rl : nullptr;
    const long long ss = (long long)k.Cout * k.ring_rl;          // strip stride: top, bottom, left, right
    const bool row_ring = rg != nullptr && (oy == 1 || oy == k.Ho - 2);
    float4 rv[4];                                                // residual: all loads in flight before the first use
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      rv[q] = make_float4(0.f, 0.f, 0.f, 0.f);
      const int ox = ox0 + 8 * q + 4 * lhi;
      if (rb && ox < k.Wo) {
        if (k.vec4) rv[q] = *reinterpret_cast<const float4*>(rb + ox);
        else {
          rv[q].x = rb[ox];
          if (ox + 1 < k.Wo) rv[q].y = rb[ox + 1];
          if (ox + 2 < k.Wo) rv[q].z = rb[ox + 2];
          if (ox + 3 < k.Wo) rv[q].w = rb[ox + 3];
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int ox = ox0 + 8 * q + 4 * lhi;
      if (ox >= k.Wo) continue;
      float v[4];
      const float r4[4] = {rv[q].x, rv[q].y, rv[q].z, rv[q].w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float t = acc[b][4 * q + e] * osc + bv;
        if (k.act == 1) t = t > 0.f ? t : t * k.slope;
        else if (k.act == 2) t = tanhf(t);
        v[e] = t + r4[e];
      }
      if (rg) {                                                  // the reflection folds frame positions onto ring pixels
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int xx = ox + e;
          if (xx < k.Wo) {
            if (row_ring) {
              if (oy == 1) v[e] += rg[xx + 1] + (xx == 1 ? rg[0] : 0.f) + (xx == k.Wo - 2 ? rg[k.Wo + 1] : 0.f);
              if (oy == k.Ho - 2) v[e] += rg[ss + xx + 1] + (xx == 1 ? rg[ss] : 0.f) + (xx == k.Wo - 2 ? rg[ss + k.Wo + 1] : 0.f);
            }
            if (xx == 1) v[e] += rg[2 * ss + oy + 1];
            if (xx == k.Wo - 2) v[e] += rg[3 * ss + oy + 1];
          }
        }
      }
      float* yp = yb + rowoff + ox;
#ifdef CS_NT_STORE
      if (k.vec4) __builtin_nontemporal_store(f32x4{v[0], v[1], v[2], v[3]}, reinterpret_cast<f32x4*>(yp));
#else
      // (one native vector store: written as a float4 struct it is four scalar stores until the load/store vectoriser runs,
      // and the fourth can first be merged with the scalar path's last store -- dwordx3 + dword, seen when this body was a function)
      if (k.vec4) *reinterpret_cast<f32x4*>(yp) = f32x4{v[0], v[1], v[2], v[3]};
#endif
      else {
        yp[0] = v[0];
        if (ox + 1 < k.Wo) yp[1] = v[1];
        if (ox + 2 < k.Wo) yp[2] = v[2];
        if (ox + 3 < k.Wo) yp[3] = v[3];
      }
    }
  }
#ifdef CS_TRACE
  __builtin_amdgcn_s_waitcnt(0x0f70);       // the stores have left the wave
#endif
  WGT(3)
