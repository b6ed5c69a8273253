// Body of conv3x3_wgrad_split2_k (conv3x3s.hip), included as text into that kernel and into conv3x3_bwd_pair_k (see
// conv3x3s_cs_body.inc for why not a function).  The including scope provides: x, dy, dwt, k (WS3P);
// bix, biy, biz (unsigned: the workgroup's index in the logical (pixel split, ci tile, co tile) grid);
// Xc[2 * XCU], Dy[2 * DYU], edc[128] (int), red[17] in LDS (W2Lds).
  constexpr int NSP = 2, BC = 128, CT = 64;
  using P = Prod<2>;
  constexpr int CTP = CT + W2_CTPAD;                 // stride of a half inside a slab
  constexpr int XSLAB = 2 * CTP;                     // units of one (split, dx, row) slab: [half][ci]
  constexpr int XCU = NSP * 3 * 4 * XSLAB, DYU = NSP * 2 * 2 * BC;
  static_assert(XCU == W2Lds::XCU && DYU == W2Lds::DYU, "arena layout");

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const bool want_db = k.db != nullptr && biy == 0;
  float bacc = 0.f, baccx = 0.f;
  const int wc = wid & 3, wi = wid >> 2;             // wi is also the stagger group
  const int l31 = lane & 31, lhi = lane >> 5;
  const int HW = k.H * k.W;
  const int ci0 = biy * CT, co0 = biz * BC;
  const int run_beg = bix * k.runs_per_block;
  int run_end = run_beg + k.runs_per_block;
  if (run_end > k.runs_total) run_end = k.runs_total;

  const int ex = scale_exp(reduce_absmax(k.x_amax, k.x_n, red));
  __syncthreads();
  const int ed = scale_exp(reduce_absmax(k.dy_amax, k.dy_n, red));
  // dY is scaled per OUTPUT CHANNEL when the per-plane maxima are known: the scale is uniform along the MFMA K (pixels
  // of one channel), so a channel whose gradient is 1e-6 of the tensor's largest keeps its 22 bits; the column's
  // factor 2^-ed[co] goes into the epilogue.  Without them: one scale for the tensor.
  if (tid < BC) {
    int e = ed;
    if (k.dy_pmax) {
      float m = 0.f;
      if (co0 + tid < k.Cout)
        for (int n = 0; n < k.N; ++n) m = fmaxf(m, k.dy_pmax[(long long)n * k.Cout + co0 + tid]);
      e = scale_exp(m);
    }
    edc[tid] = e;
  }
  __syncthreads();

  // loader roles: X group (patch row xr 0..3, half xu, channel xc 0..63), dY group (k-step dk, half du, channel dc)
  const int xc = tid & 63, xu = (tid >> 6) & 1, xr = tid >> 7;
  const int dc = tid & (BC - 1), du = (tid >> 7) & 1, dk = tid >> 8;
  const bool xin = k.dbx != nullptr && biz == 0 && (xr == 1 || xr == 2);     // rows of a run that are not halo
  const float xscale = pow2f(ex), dscale = pow2f(edc[dc]), oscale = pow2f(-ex), oscale2 = pow2f(-edc[wc * 32 + l31]);
  const unsigned hw4 = (unsigned)HW * 4u;
  constexpr unsigned OOB = 0x80000000u;

  f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  u32x4 rxa, rxb, rda, rdb;   // 8 px of X, 8 px of dY
  unsigned rxl, rxr;          // the pixel left / right of the X group

  // past the last run of this workgroup the descriptors are empty (loads return zeros, stores are harmless)
#ifndef W2_KO
#define W2_KO 0           // knock-out builds (timing experiments): 1 no global loads, 2 no LDS stores, 4 no conversion, 8 no MFMA phase
#endif
#define W2_GLOAD(run_)                                                                           \
  if (!(W2_KO & 1) || k.N < 0) {                                                                 \
    const bool live_ = (run_) < run_end;                                                         \
    const int n_ = live_ ? (run_) / k.runs_per_img : 0;                                          \
    const int q_ = live_ ? (run_) - n_ * k.runs_per_img : 0;                                     \
    const int yp_ = q_ / k.runs_per_row, xs_ = q_ - yp_ * k.runs_per_row;                        \
    const int y0_ = 2 * yp_, x0_ = 16 * xs_ + 8 * xu;                                            \
    const __amdgpu_buffer_rsrc_t bx_ = __builtin_amdgcn_make_buffer_rsrc(                        \
        const_cast<float*>(x + (long long)n_ * k.Cin * HW), 0, live_ ? (unsigned)(k.Cin * HW) * 4u : 0u, 0x00020000); \
    const __amdgpu_buffer_rsrc_t bd_ = __builtin_amdgcn_make_buffer_rsrc(                        \
        const_cast<float*>(dy + (long long)n_ * k.Cout * HW), 0, live_ ? (unsigned)(k.Cout * HW) * 4u : 0u, 0x00020000); \
    const bool cok_ = ci0 + xc < k.Cin;                                                          \
    const unsigned cb_ = (unsigned)(ci0 + xc) * hw4;                                             \
    int ry_ = y0_ - 1 + xr;                                                                      \
    bool rok_ = (unsigned)ry_ < (unsigned)k.H;                                                   \
    if (k.pad_mode == 1) { ry_ = ry_ < 0 ? -ry_ : (ry_ >= k.H ? 2 * (k.H - 1) - ry_ : ry_); rok_ = true; } \
    const int rb_ = ry_ * k.W;                                                                   \
    const bool lin_ = x0_ > 0, rin_ = x0_ + 8 < k.W;                                             \
    const int ol_ = rb_ + (lin_ ? x0_ - 1 : 1), or_ = rb_ + (rin_ ? x0_ + 8 : k.W - 2);          \
    const bool lok_ = rok_ && cok_ && (lin_ || k.pad_mode == 1), rrok_ = rok_ && cok_ && (rin_ || k.pad_mode == 1); \
    const unsigned xb_ = (rok_ && cok_) ? cb_ + (unsigned)(rb_ + x0_) * 4u : OOB;                \
    rxa = __builtin_amdgcn_raw_buffer_load_b128(bx_, xb_, 0, 0);                                 \
    rxb = __builtin_amdgcn_raw_buffer_load_b128(bx_, xb_ == OOB ? OOB : xb_ + 16u, 0, 0);        \
    rxl = __builtin_amdgcn_raw_buffer_load_b32(bx_, lok_ ? cb_ + (unsigned)ol_ * 4u : OOB, 0, 0); \
    rxr = __builtin_amdgcn_raw_buffer_load_b32(bx_, rrok_ ? cb_ + (unsigned)or_ * 4u : OOB, 0, 0); \
    const unsigned db_ = (co0 + dc >= k.Cout) ? OOB                                              \
        : (unsigned)(co0 + dc) * hw4 + (unsigned)((y0_ + dk) * k.W + 16 * xs_ + 8 * du) * 4u;    \
    rda = __builtin_amdgcn_raw_buffer_load_b128(bd_, db_, 0, 0);                                 \
    rdb = __builtin_amdgcn_raw_buffer_load_b128(bd_, db_ == OOB ? OOB : db_ + 16u, 0, 0);        \
  }
  // W2_NORM_PROBE (lab builds): the cost of an InstanceNorm + ReLU applied while the X operand is converted -- (x - m) * r and a
  // max per value with run-time operands that happen to be the identity (profiles/r06_cs_norm_probe.txt)
#ifdef W2_NORM_PROBE
  const float np_r = fmaf(oscale, 0.f, 1.f), np_m = oscale * 0.f, np_lo = fmaf(oscale, 0.f, -3.0e38f);
#define W2_NORM_PROBE_OPS() _Pragma("unroll") for (int i = 0; i < 10; ++i) r[i] = fmaxf((r[i] - np_m) * np_r, np_lo);
#else
#define W2_NORM_PROBE_OPS()
#endif
  // X: r[0] = left neighbour, r[1..8] = the group, r[9] = right neighbour; pairs (0,1)..(8,9) make the units
  // dx=0 (cols -1..6) and dx=2 (cols 1..8), the odd pairing dx=1 is the even one shifted by a half
#define W2_LSTORE(buf_)                                                                          \
  {                                                                                              \
    float r[10];                                                                                 \
    r[0] = __uint_as_float(rxl); r[9] = __uint_as_float(rxr);                                    \
    _Pragma("unroll") for (int e = 0; e < 4; ++e) { r[1 + e] = __uint_as_float(rxa[e]); r[5 + e] = __uint_as_float(rxb[e]); } \
    W2_NORM_PROBE_OPS()                                                                          \
    baccx += xin ? ((r[1] + r[2]) + (r[3] + r[4])) + ((r[5] + r[6]) + (r[7] + r[8])) : 0.f;      \
    unsigned pa[5][NSP], pb[4][NSP];                                                             \
    if (W2_KO & 4) { _Pragma("unroll") for (int i = 0; i < 5; ++i) { pa[i][0] = __float_as_uint(r[2 * i]); pa[i][1] = __float_as_uint(r[2 * i + 1]); } } \
    else _Pragma("unroll") for (int i = 0; i < 5; ++i) split_pair_scaled(r[2 * i], r[2 * i + 1], xscale, pa[i][0], pa[i][1]); \
    _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                \
      _Pragma("unroll") for (int s = 0; s < NSP; ++s) pb[i][s] = __builtin_amdgcn_alignbit(pa[i + 1][s], pa[i][s], 16); \
    if (!(W2_KO & 2) || k.N < 0) _Pragma("unroll") for (int s = 0; s < NSP; ++s) {                 \
      u32x4* dst = Xc + (buf_) * XCU + (s * 3 * 4 + xr) * XSLAB + xu * CTP + xc;                    \
      dst[0] = u32x4{pa[0][s], pa[1][s], pa[2][s], pa[3][s]};                                    \
      dst[4 * XSLAB] = u32x4{pb[0][s], pb[1][s], pb[2][s], pb[3][s]};                            \
      dst[8 * XSLAB] = u32x4{pa[1][s], pa[2][s], pa[3][s], pa[4][s]};                            \
    }                                                                                            \
    float v[8];                                                                                  \
    _Pragma("unroll") for (int e = 0; e < 4; ++e) { v[e] = __uint_as_float(rda[e]); v[4 + e] = __uint_as_float(rdb[e]); } \
    bacc += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));                   \
    u32x4 sp[NSP];                                                                               \
    if (W2_KO & 4) { sp[0] = rda; sp[1] = rdb; } else                                            \
    split8_s<NSP>(v, dscale, sp);                                                                \
    if (!(W2_KO & 2) || k.N < 0) _Pragma("unroll") for (int s = 0; s < NSP; ++s) Dy[(buf_) * DYU + ((s * 2 + dk) * 2 + du) * BC + dc] = sp[s]; \
  }

  // operand unit indices of this lane: A = Xc[((s*3 + dx)*4 + row)*2 + lhi][ci], B = Dy[(s*2 + ks)*2 + lhi][co]
  const int abase = lhi * CTP + wi * 32 + l31;
  const int bbase = lhi * BC + wc * 32 + l31;
  // the 12 operand units of a run in an order that never puts two 3-MFMA units (rows 0, 3) next to each other
  //   unit u -> (dx, row);  MFMAs of a unit: k-steps ks with 0 <= row - ks <= 2, tap = (row - ks)*3 + dx
#ifndef W2_LEAD
#define W2_LEAD 1      // operand units read ahead (1-3 measured equal; 1 needs the fewest registers)
#endif
#ifdef W2_NOPRIO
#define W2_PRIO(p_)
#else
#define W2_PRIO(p_) __builtin_amdgcn_s_setprio(p_)
#endif
#define W2_UDX(u_) ((u_) / 4)
#define W2_UROW(u_) ((u_) < 4 ? (u_) : ((u_) % 4 == 0 ? 1 : ((u_) % 4 == 1 ? 0 : (u_) % 4)))
#define W2_LOADA(set_, u_)                                                                       \
  _Pragma("unroll") for (int s = 0; s < NSP; ++s)                                                \
    a[set_][s] = Xb[((s * 3 + W2_UDX(u_)) * 4 + W2_UROW(u_)) * XSLAB + abase];
#define W2_MMA_PHASE(buf_)                                                                       \
  {                                                                                              \
    const u32x4* Xb = Xc + (buf_) * XCU;                                                         \
    const u32x4* Db = Dy + (buf_) * DYU;                                                         \
    u32x4 b[2][NSP], a[W2_LEAD + 1][NSP];                                                        \
    _Pragma("unroll") for (int s = 0; s < NSP; ++s) b[0][s] = Db[(s * 2 + 0) * 2 * BC + bbase];  \
    W2_LOADA(0, 0)                                                                               \
    _Pragma("unroll") for (int s = 0; s < NSP; ++s) b[1][s] = Db[(s * 2 + 1) * 2 * BC + bbase];  \
    if (W2_LEAD > 1) W2_LOADA(1, 1)                                                              \
    __builtin_amdgcn_sched_barrier(0);                                                           \
    _Pragma("unroll") for (int u = 0; u < 12; ++u) {                                             \
      if (u + W2_LEAD < 12) W2_LOADA((u + W2_LEAD) % (W2_LEAD + 1), u + W2_LEAD)                 \
      const int dx_ = W2_UDX(u), row_ = W2_UROW(u);                                              \
      /* W2_ALT: the two taps a unit feeds take turns (no two consecutive MFMAs on one accumulator) */ \
      _Pragma("unroll") for (int qo = 0; qo < (W2_ALT ? P::N : 1); ++qo)                         \
      _Pragma("unroll") for (int ks = 0; ks < 2; ++ks) {                                         \
        const int ty_ = row_ - ks;                                                               \
        if (ty_ >= 0 && ty_ <= 2) {                                                              \
          _Pragma("unroll") for (int q = (W2_ALT ? qo : 0); q < (W2_ALT ? qo + 1 : P::N); ++q)   \
            acc[ty_ * 3 + dx_] = mma16<NSP>(a[u % (W2_LEAD + 1)][P::A[q]], b[ks][P::B[q]], acc[ty_ * 3 + dx_]); \
        }                                                                                        \
      }                                                                                          \
      const int nm_ = (row_ == 0 || row_ == 3) ? 3 : 6;                                          \
      _Pragma("unroll") for (int i = 0; i < 6; ++i) {                                            \
        if (i < nm_) __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                          \
        if (i < NSP && u + W2_LEAD < 12) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);      \
      }                                                                                          \
      __builtin_amdgcn_sched_barrier(0);                                                         \
    }                                                                                            \
  }

  if (run_beg < run_end) {
    W2_GLOAD(run_beg);
    W2_LSTORE(0);
    W2_GLOAD(run_beg + 1);
  }
  __syncthreads();

  // two copies of the run loop rather than a branch inside one: each group's loop gets its own register allocation
  // (a branch in the body spilled 270 registers); both execute the same number of barriers
#ifdef W2_TRACE
  const bool trace_blk = bix == 5 && biy == 1 && biz == 0;
#endif
  if (wi == 0) {
    for (int run = run_beg; run < run_end; ++run) {
      const int buf = (run - run_beg) & 1;
      W2T(0)
      W2_PRIO(W2_PRIO_C);
      W2T_VM()
      W2_LSTORE(buf ^ 1);
      W2_GLOAD(run + 2);
      __builtin_amdgcn_sched_barrier(0);
      W2T(1)
      W2_PRIO(W2_PRIO_G0);
      if (!(W2_KO & 8) || k.N < 0) W2_MMA_PHASE(buf);
      W2T(2)
      __syncthreads();
      W2T(3)
    }
  } else {
    for (int run = run_beg; run < run_end; ++run) {
      const int buf = (run - run_beg) & 1;
      W2T(0)
      W2_PRIO(W2_PRIO_G1);
      if (!(W2_KO & 8) || k.N < 0) W2_MMA_PHASE(buf);
      __builtin_amdgcn_sched_barrier(0);
      W2T(1)
      W2_PRIO(W2_PRIO_C);
      W2T_VM()
      W2_LSTORE(buf ^ 1);
      W2_GLOAD(run + 2);
      W2T(2)
      __syncthreads();
      W2T(3)
    }
  }
#undef W2_GLOAD
#undef W2_LSTORE
#undef W2_LOADA
#undef W2_MMA_PHASE
#undef W2_UDX
#undef W2_UROW

  // Bias gradient.  The per-thread sums of a channel (4 threads of the dY loaders, 8 of the X loaders) meet in LDS in a FIXED
  // order, in the operand buffers, which are free after the run loop's last barrier.  (They used to meet in LDS atomics, which
  // add in arrival order: db then differed in its last bits from run to run even where ONE workgroup owns a channel and its
  // single global add lands on zeros.)
  float* part = reinterpret_cast<float*>(Xc);
  if (want_db) {
    part[(tid >> 7) * BC + dc] = bacc;
    __syncthreads();
    if (tid < BC && co0 + tid < k.Cout)
      atomicAdd(&k.db[co0 + tid], (part[tid] + part[BC + tid]) + (part[2 * BC + tid] + part[3 * BC + tid]));
    __syncthreads();
  }
  if (k.dbx != nullptr && biz == 0) {
    part[(tid >> 6) * CT + xc] = baccx;
    __syncthreads();
    if (tid < CT && ci0 + tid < k.Cin) {
      float t = 0.f;
#pragma unroll
      for (int i = 0; i < 8; i += 2) t += part[i * CT + tid] + part[(i + 1) * CT + tid];
      atomicAdd(&k.dbx[ci0 + tid], t);
    }
  }
  if (k.swap) {
    // transposed store: the real layout is [8 - t][co][ci] with ci (this kernel's rows) fastest.  Each wave turns its
    // 32 x 32 tile around through LDS (the operand buffers are free now) so that a half-wave adds to 32 consecutive
    // floats -- 19 M lane-scattered atomics on 74 K addresses cost 0.4 ms at the 128 -> 64 layer
    __syncthreads();
    float* T = reinterpret_cast<float*>(Xc) + wid * (32 * 33);
#pragma unroll
    for (int t = 0; t < 9; ++t) {
#pragma unroll
      for (int r = 0; r < 16; ++r) T[(4 * lhi + (r & 3) + 8 * (r >> 2)) * 33 + l31] = acc[t][r] * oscale * oscale2;
      __syncthreads();
      const int ci = ci0 + wi * 32 + l31;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int col = 4 * lhi + (r & 3) + 8 * (r >> 2);
        const int co = co0 + wc * 32 + col;
        const float v = T[l31 * 33 + col];
        if (ci < k.Cin && co < k.Cout) df_acc(dwt, ((long long)(8 - t) * k.Cout + co) * k.Cin + ci, v, k.fx);
      }
      __syncthreads();
    }
    return;
  }
  const int co = co0 + wc * 32 + l31;
  if (co < k.Cout) {
#pragma unroll
    for (int t = 0; t < 9; ++t) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ci = ci0 + wi * 32 + 4 * lhi + (r & 3) + 8 * (r >> 2);
        if (ci < k.Cin) df_acc(dwt, ((long long)t * k.Cin + ci) * k.Cout + co, acc[t][r] * oscale * oscale2, k.fx);
      }
    }
  }
