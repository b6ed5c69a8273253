// Warped-feature SSD: the data term of instance optimisation, value and flow gradient in ONE pass, 2-D and 3-D.
// Build-defined (include/dfmir_hip.h and losses.WarpedSSD_Loss state the definition):
//
//   M, F [B][C][(D)][H][W] fp32 features of the moving / fixed image, 1 <= C <= 16; phi [B][ND][(D)][H][W] fp32, channel d
//   displaces axis d in voxels, order (z,) y, x, as the warp kernels read a flow.
//   e_c(x)  = M_c(x + phi(x)) - F_c(x)     M sampled (bi/tri)linearly, align_corners, corners outside the volume read as 0
//   L       = mean over (B, C, voxels) of e^2;  with a mask m [B][S]:  L = sum m mean_c e^2 / sum m  (0 for an empty mask)
//   L_b     = the same over sample b alone
//   dL/dphi_d(x) = k(x) sum_c e_c(x) d_d M_c(x + phi(x)),   k = 2 gout / (B C S), masked 2 gout m(x) / (C sum m);
//             d_d = the derivative of the interpolant in the cell floor() selects: corner differences, zero-padded corners
//             taking part as zeros (as ic_voxel of invcons.hip forms it).  No gradient to M, F or m.
//
// A gather bound by the number of load instructions (invcons.hip), so the moving features, constant over a refinement loop,
// are read from a VOXEL-MAJOR packed copy [B][(D)][H][W][Cp], Cp = C rounded up to 4 (ws_pack_k, made once by the caller):
// a corner costs Cp / 4 16-byte loads.  DFMIR_WARPSSD_PLANAR keeps the channel-major gather (4 bytes per corner and
// channel) for the A/B.  F stays channel-major and is read coalesced along x.
//   ws_fwd_k   lanes run along x, a workgroup owns WS_T * VPT consecutive voxels of ONE sample and each of its waves 64 * VPT
//              of them, taken 64 at a time (VPT = 4 with 16-byte accesses of phi, F and dflow when W % 4 == 0 and the
//              pointers are aligned, else 1; the 16-byte order and the one-voxel-per-lane order of the arithmetic meet in
//              LDS rows the wave owns; the quads of the next 64 voxels are fetched while the current ones are gathered).
//              The cell of a voxel is formed once (the guards of ic_voxel: no float goes to int for
//              a NaN or a far-away point, every address lies inside the tensor), then its channels pass in groups of four:
//              the corners are gathered, e^2 and e * dM are added.  sum m e^2 and sum m are added in double per thread and
//              leave as two double slots per workgroup; the UNIT gradient (gout = 1; masked: still to be divided by sum m)
//              is written when asked for.  No warped tensor, no e tensor, no atomics.
//   ws_fin_k   (ws_sample.h, shared with demons.hip; one workgroup) adds the slots of each sample in a fixed order: L_b, L
//              and the gradient's scale (1, masked 1 / sum m, 0 for an empty mask).  Bit-identical from run to run.
//   ws_bwd_k   dflow = unit * gout * scale, both read on the device.
// Nothing syncs with the host or keeps state.
#include "ws_sample.h"

namespace {

// One voxel, one channel group: s2 += sum_c e_c^2, gr_d += sum_c e_c d_d M_c
template <int ND, bool PACKED>
__device__ __forceinline__ void ws_group(const float* __restrict__ mb, const WsGeom& g, const WsCell<ND>& q, int gi,
                                         const float (&f)[4], float& s2, float (&gr)[ND]) {
  constexpr int NC = 1 << ND;
  float4 val[NC];
  ws_corners<ND, PACKED>(mb, g, q, gi, val);
#pragma unroll
  for (int cc = 0; cc < 4; ++cc) {
    float v[NC], d[ND];
#pragma unroll
    for (int m = 0; m < NC; ++m) v[m] = cc == 0 ? val[m].x : cc == 1 ? val[m].y : cc == 2 ? val[m].z : val[m].w;
    const float e = ws_interp<ND>(v, q, d) - f[cc];             // a channel >= C: corners and f are 0, e = 0
    s2 += e * e;
#pragma unroll
    for (int a = 0; a < ND; ++a) gr[a] += e * d[a];
  }
}

// part[2 wg] = sum m sum_c e^2, part[2 wg + 1] = sum m over the workgroup's voxels (m = 1 without a mask); unit (may be
// NULL) = kpre m(x) sum_c e_c d_d M_c.  A wave owns 64 * VPT consecutive voxels and takes them 64 at a time, one per lane.
// VPT == 4: the 64 voxels' phi and F arrive as 16-byte loads -- 16 lanes cover the 64 voxels of one channel, so one wave
// instruction fetches four channels -- and turn into one-voxel-per-lane order in the wave's own LDS rows; the gradient
// leaves the same way.  Every channel group of a voxel is gathered in the same pass: a corner's record is read while its
// cache lines are at hand.
template <int ND, int VPT, bool PACKED>
__global__ __launch_bounds__(WS_T) void ws_fwd_k(const float* __restrict__ mov, const float* __restrict__ fix,
                                                 const float* __restrict__ phi, const float* __restrict__ mask, WsGeom g,
                                                 float kpre, double* __restrict__ part, float* __restrict__ unit) {
  constexpr int NW = WS_T / 64;
  // per wave: rows of 64 floats, WS_MAXC + ND in (F, phi) and ND out (the gradient)
  __shared__ __attribute__((aligned(16))) float sin_[VPT == 4 ? NW * (WS_MAXC + ND) * 64 : 4];
  __shared__ __attribute__((aligned(16))) float sout[VPT == 4 ? NW * ND * 64 : 4];
  __shared__ double red[NW];
  const int b = (int)(blockIdx.x / (unsigned)g.nblk);
  const unsigned blk = blockIdx.x - (unsigned)b * (unsigned)g.nblk;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const unsigned v0 = blk * (unsigned)(WS_T * VPT) + (unsigned)(wv * 64 * VPT);      // < S + WS_T * VPT < 2^31
  const float* pb = phi + (long long)b * ND * g.S;
  const float* fb = fix + (long long)b * g.C * g.S;
  const float* mb = mov + (long long)b * (PACKED ? g.Cp : g.C) * g.S;
  float* ub = unit ? unit + (long long)b * ND * g.S : nullptr;
  float* sf = sin_ + wv * (WS_MAXC + ND) * 64;                    // rows 0 .. Cp - 1: F; rows WS_MAXC .. : phi
  float* so = sout + wv * ND * 64;
  const int row = lane >> 4, quad = (lane & 15) << 2;            // VPT == 4: this lane's share of a 4-row, 64-voxel load
  const int ng = g.Cp >> 2;
  double acc = 0.0, wsum = 0.0;
  // VPT == 4: the quads of the NEXT 64 voxels are in flight while the current ones are gathered (pf: F per channel group,
  // pp: phi); the loops over the groups are unrolled to WS_MAXC / 4 with a uniform guard so that pf stays in registers
  float4 pf[WS_MAXC / 4], pp;
  auto fetch = [&](unsigned vb) {
    if (vb + (unsigned)quad < (unsigned)g.S) {                 // S % 4 == 0: a quad lies inside or outside as a whole
      if (row < ND) pp = *reinterpret_cast<const float4*>(pb + (long long)row * g.S + vb + quad);
#pragma unroll
      for (int gi = 0; gi < WS_MAXC / 4; ++gi)
        if (gi < ng) {
          const int c = 4 * gi + row;
          pf[gi] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (c < g.C) pf[gi] = *reinterpret_cast<const float4*>(fb + (long long)c * g.S + vb + quad);
        }
    }
  };
  if (VPT == 4) fetch(v0);
#pragma unroll 1
  for (int e = 0; e < VPT; ++e) {
    const unsigned vb = v0 + 64u * e;                            // the 64 voxels of this pass: vb + lane
    const unsigned j = vb + (unsigned)lane;
    const bool quad_in = vb + (unsigned)quad < (unsigned)g.S;
    if (VPT == 4) {
      if (quad_in) {
        if (row < ND) *reinterpret_cast<float4*>(sf + (WS_MAXC + row) * 64 + quad) = pp;
#pragma unroll
        for (int gi = 0; gi < WS_MAXC / 4; ++gi)
          if (gi < ng) *reinterpret_cast<float4*>(sf + (4 * gi + row) * 64 + quad) = pf[gi];
      }
      __syncthreads();
      if (e + 1 < VPT) fetch(vb + 64u);
    }
    if (j < (unsigned)g.S) {
      int p[ND];
      unsigned t = j;
      p[ND - 1] = (int)(t % (unsigned)g.W); t /= (unsigned)g.W;
      if (ND == 3) { p[1] = (int)(t % (unsigned)g.H); p[0] = (int)(t / (unsigned)g.H); }
      else p[0] = (int)t;
      float u[ND], gr[ND];
#pragma unroll
      for (int c = 0; c < ND; ++c) {
        u[c] = VPT == 4 ? sf[(WS_MAXC + c) * 64 + lane] : pb[(long long)c * g.S + j];
        gr[c] = 0.f;
      }
      WsCell<ND> cell;
      ws_cell<ND>(g, p, u, cell);
      float s2 = 0.f;
      for (int gi = 0; gi < ng; ++gi) {
        float f[4];
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
          if (VPT == 4) f[cc] = sf[(4 * gi + cc) * 64 + lane];
          else f[cc] = 4 * gi + cc < g.C ? fb[(long long)(4 * gi + cc) * g.S + j] : 0.f;
        }
        ws_group<ND, PACKED>(mb, g, cell, gi, f, s2, gr);
      }
      const float m = mask ? mask[(long long)b * g.S + j] : 1.f;
      acc += (double)(m * s2);
      wsum += (double)m;
      const float k = kpre * m;
#pragma unroll
      for (int a = 0; a < ND; ++a) {
        if (VPT == 4) so[a * 64 + lane] = k * gr[a];
        else if (ub) ub[(long long)a * g.S + j] = k * gr[a];
      }
    }
    if (VPT == 4) {
      __syncthreads();        // (also: every lane is done with sf before the next pass overwrites it)
      if (ub && quad_in && row < ND)
        *reinterpret_cast<float4*>(ub + (long long)row * g.S + vb + quad) = *reinterpret_cast<const float4*>(so + row * 64 + quad);
    }
  }
  acc = block_sum_ordered<WS_T>(acc, red);
  wsum = block_sum_ordered<WS_T>(wsum, red);
  if (threadIdx.x == 0) { part[2LL * blockIdx.x] = acc; part[2LL * blockIdx.x + 1] = wsum; }
}

template <int V>
__global__ __launch_bounds__(WS_T) void ws_bwd_k(const float* __restrict__ unit, const float* __restrict__ gout,
                                                 const float* __restrict__ scale, float* __restrict__ dflow, long long n) {
  const long long i = ((long long)blockIdx.x * WS_T + threadIdx.x) * V;
  if (i >= n) return;
  const float s = gout[0] * scale[0];
  if (V == 4) {
    float4 t = *reinterpret_cast<const float4*>(unit + i);
    t.x *= s; t.y *= s; t.z *= s; t.w *= s;
    *reinterpret_cast<float4*>(dflow + i) = t;
  } else {
    dflow[i] = unit[i] * s;
  }
}

// [B][C][S] -> [B][S][Cp], channels >= C zero: one thread per voxel, 16-byte stores
__global__ __launch_bounds__(WS_T) void ws_pack_k(const float* __restrict__ in, float* __restrict__ out, int C, int Cp,
                                                  int S, long long nvox) {
  const long long i = (long long)blockIdx.x * WS_T + threadIdx.x;
  if (i >= nvox) return;
  const long long b = i / S;
  const int j = (int)(i - b * S);
  const float* ib = in + b * C * S + j;
  float* ob = out + i * Cp;
  for (int c0 = 0; c0 < Cp; c0 += 4) {
    float4 t;
    t.x = ib[(long long)c0 * S];
    t.y = c0 + 1 < C ? ib[(long long)(c0 + 1) * S] : 0.f;
    t.z = c0 + 2 < C ? ib[(long long)(c0 + 2) * S] : 0.f;
    t.w = c0 + 3 < C ? ib[(long long)(c0 + 3) * S] : 0.f;
    *reinterpret_cast<float4*>(ob + c0) = t;
  }
}

}  // namespace

extern "C" long long dfmir_warp_ssd_ws_floats(int nd, int B, int C, int D, int H, int W) {
  WsGeom g;
  if (!ws_geom(nd, B, C, D, H, W, 1, &g)) return -1;
  return 4LL * B * g.nblk;                   // two doubles per workgroup of the scalar launch (the larger)
}

extern "C" int dfmir_warp_ssd_pack(int nd, const float* M, float* Mp, int B, int C, int D, int H, int W, void* stream) {
  WsGeom g;
  DF_ARG_CHECK(M && Mp && ws_al16(Mp));
  DF_ARG_CHECK(ws_geom(nd, B, C, D, H, W, 1, &g));
  const long long nvox = (long long)B * g.S;
  ws_pack_k<<<(unsigned)((nvox + WS_T - 1) / WS_T), WS_T, 0, (hipStream_t)stream>>>(M, Mp, C, g.Cp, g.S, nvox);
  DF_LAUNCH_CHECK();
  return 0;
}

extern "C" int dfmir_warp_ssd_fwd_grad(int nd, const float* Mp, const float* M, const float* F, const float* phi,
                                       const float* mask, float* ws, float* per_sample, float* loss, float* scale,
                                       float* unit, int B, int C, int D, int H, int W, void* stream) {
  WsGeom g;
  DF_ARG_CHECK((Mp || M) && F && phi && ws && per_sample && loss && scale && (reinterpret_cast<uintptr_t>(ws) & 7) == 0);
  DF_ARG_CHECK(!Mp || ws_al16(Mp));
  static DfOptFlag planar_opt{"DFMIR_WARPSSD_PLANAR"};          // A/B: the channel-major gather
  const bool planar = !Mp || (M && planar_opt.get());
  const int vpt = (W % 4 == 0 && ws_al16(F) && ws_al16(phi) && (!unit || ws_al16(unit))) ? 4 : 1;
  DF_ARG_CHECK(ws_geom(nd, B, C, D, H, W, vpt, &g));
  hipStream_t st = (hipStream_t)stream;
  const unsigned nwg = (unsigned)((long long)B * g.nblk);
  double* part = reinterpret_cast<double*>(ws);
  const float kpre = mask ? (float)(2.0 / (double)C) : (float)(2.0 / ((double)B * C * (double)g.S));
  const float* mov = planar ? M : Mp;
#define WS_LAUNCH(ND_, VPT_, PK_) ws_fwd_k<ND_, VPT_, PK_><<<nwg, WS_T, 0, st>>>(mov, F, phi, mask, g, kpre, part, unit)
  if (nd == 3) {
    if (vpt == 4) { if (planar) WS_LAUNCH(3, 4, false); else WS_LAUNCH(3, 4, true); }
    else { if (planar) WS_LAUNCH(3, 1, false); else WS_LAUNCH(3, 1, true); }
  } else {
    if (vpt == 4) { if (planar) WS_LAUNCH(2, 4, false); else WS_LAUNCH(2, 4, true); }
    else { if (planar) WS_LAUNCH(2, 1, false); else WS_LAUNCH(2, 1, true); }
  }
#undef WS_LAUNCH
  DF_LAUNCH_CHECK();
  ws_fin_k<WS_T><<<1, WS_T, 0, st>>>(part, B, g.nblk, (double)C, mask ? 1 : 0, per_sample, loss, scale);
  DF_LAUNCH_CHECK();
  return 0;
}

extern "C" int dfmir_warp_ssd_fwd(int nd, const float* Mp, const float* M, const float* F, const float* phi,
                                  const float* mask, float* ws, float* per_sample, float* loss, float* scale, int B, int C,
                                  int D, int H, int W, void* stream) {
  return dfmir_warp_ssd_fwd_grad(nd, Mp, M, F, phi, mask, ws, per_sample, loss, scale, nullptr, B, C, D, H, W, stream);
}

extern "C" int dfmir_warp_ssd_bwd(const float* unit, const float* gout, const float* scale, float* dflow, long long n,
                                  void* stream) {
  DF_ARG_CHECK(unit && gout && scale && dflow && n >= 1 && n < (1LL << 31));
  hipStream_t st = (hipStream_t)stream;
  if (n % 4 == 0 && ws_al16(unit) && ws_al16(dflow))
    ws_bwd_k<4><<<(unsigned)((n / 4 + WS_T - 1) / WS_T), WS_T, 0, st>>>(unit, gout, scale, dflow, n);
  else
    ws_bwd_k<1><<<(unsigned)((n + WS_T - 1) / WS_T), WS_T, 0, st>>>(unit, gout, scale, dflow, n);
  DF_LAUNCH_CHECK();
  return 0;
}
