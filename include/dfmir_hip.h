/*
 * dfmir_hip.h -- C ABI of libdfmir_hip.so: the MI355X (gfx950) compute library behind the
 * DFMIR `--model registration` training step.
 *
 * The reference (heyblackC/DFMIR) has no native boundary: its hot path calls torch.nn /
 * torch.nn.functional ops from Python.  Each entry point below replaces ONE such torch op call
 * site on the path REGISTRATIONModel.set_input -> optimize_parameters
 * (reference models/registration_model.py:138-183); the reference line each one stands in for is
 * cited next to it.  The host side (the dfmir_amd Python package) binds these symbols with ctypes.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to caller-allocated, contiguous fp32 memory laid out
 *     NCHW / NCDHW exactly like the reference's tensors (2-D tensors are D == 1);
 *   - `stream` is a hipStream_t passed as void*; nothing allocates, nothing synchronises; the only
 *     state the library keeps is the (thread-local) last-error string and the PROCESS-GLOBAL option
 *     table below ("Options") -> re-entrant across streams / processes, but two models in one
 *     process share one set of options;
 *   - return value 0 = launched; >0 = hipError_t; <0 = bad argument.  dfmir_last_error() gives text;
 *   - "accumulates" means the kernel atomically adds into a buffer the caller has zeroed/initialised.
 */
#ifndef DFMIR_HIP_H
#define DFMIR_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define DFMIR_ABI_VERSION 14

int dfmir_abi_version(void);
const char* dfmir_last_error(void);

/* ------------------------------------------------------------------------------------------
 * Options -- process-global A/B switches of the kernel selection (lab knobs; the defaults are the
 * product).  dfmir_set_option(name, value) sets `name` (must start with "DFMIR_") to `value`;
 * value == NULL marks it explicitly UNSET (also hiding an environment variable of that name).
 * A name never set through this call falls back to the environment variable of the same name.
 * The change applies to launches issued after the call returns, on every thread (no per-stream or
 * per-model scope).  Options that change a DATA LAYOUT the caller holds (DFMIR_CONV_SPLIT,
 * DFMIR_CONV_FP32, DFMIR_CONV3D_FP32: the split sections of packed weights) must be set before the
 * first dfmir_weight_pack* call, or every packed buffer re-packed after the change.
 * dfmir_get_option copies the current value into buf (NUL-terminated, truncated to buf_len) and
 * returns its length, or -1 when the option is unset.  Flag options (everything below without "=n") are ON when set to
 * anything but "" or "0" -- set_option(name, "0") switches a flag off like set_option(name, NULL) does.  Reads are
 * thread-safe: values are copied out under the table's lock, the per-site caches are single atomic words.
 *   kernel selection: DFMIR_CONV_FP32, DFMIR_CONV_SPLIT=bf16x3, DFMIR_CONV3D_FP32, DFMIR_CONV_GENERIC=1,
 *     DFMIR_CS_XCD_PAIR=n, DFMIR_CONV3D_NO_PAIR, DFMIR_CONV3D_NO_M16, DFMIR_CONV3D_NO_TINY,
 *     DFMIR_CONV3D_NO_MULTI, DFMIR_CONV3D_WGS=n, DFMIR_CONV3D_NO_MARCH,
 *     DFMIR_MARCH_NSEG=n, DFMIR_CS_DEPHASE=n, DFMIR_CONV_W1 (lab builds with -DDFMIR_BUILD_W1 only),
 *     DFMIR_UPWGRAD_8WAVE, DFMIR_UPWGRAD_NSEG=n (dfmir_conv3d_upwgrad),
 *     DFMIR_NCC_NO_WH_FUSE, DFMIR_CONV3D_NO_WGRAD_MARCH, DFMIR_WGRAD_MARCH_NSEG=n, DFMIR_NO_TINYVOL,
 *     DFMIR_NO_1X1_WGRAD, DFMIR_CONV3D_NO_FLOW_WGRAD, DFMIR_CONV3D_NO_S2, DFMIR_RESIZE_NO_ROWS, DFMIR_NCC_NO_D_FUSE, DFMIR_SMOOTH_NO_MARCH,
 *     DFMIR_NO_BWD_PAIR (dgrad and wgrad of a 3x3 layer as two launches), DFMIR_BWD_PAIR=0|1 (the same switch with an explicit
 *     value; unset = the build's default), DFMIR_BWD_PAIR_ORDER=n (workgroup order inside dfmir_conv3x3_bwd_pair's grid:
 *     0 weight gradient first, 1 data gradient first, 2 interleaved in groups of 8), DFMIR_INVCONS_FIXED64 (dfmir_invcons_bwd and
 *     dfmir_compose_bwd: dv through the 64-bit fixed-point scatter on every shape), DFMIR_WARPSSD_PLANAR (dfmir_warp_ssd_fwd / _fwd_grad: gather the
 *     moving features from the channel-major tensor M instead of the voxel-major packed copy Mp).
 * ---------------------------------------------------------------------------------------- */
int dfmir_set_option(const char* name, const char* value);
int dfmir_get_option(const char* name, char* buf, int buf_len);

/* ------------------------------------------------------------------------------------------
 * Convolutions (implicit GEMM on the matrix cores: v_mfma_f32_32x32x2_f32 / 16x16x4_f32, and -- for the
 * 2-D 3x3 stride-1 layers with more than 32 output channels -- fp32 emulated on the 16-bit matrix pipe by
 * operand splitting, csrc/conv3x3s.hip: scaled fp16x2 (default) or bf16x3 (DFMIR_CONV_SPLIT=bf16x3);
 * DFMIR_CONV_FP32=1 keeps the fp32 instruction there too).
 * Replaces nn.Conv2d / nn.Conv3d (+ the ReflectionPad2d in front of it, + the LeakyReLU/Tanh
 * behind it) at: models/networks.py:982-983, 995, 1016-1023 (ResnetGenerator),
 * models/networks.py:1201,1214 (ResnetBlock), models/networks.py:587-595 (PatchSampleF MLP,
 * as 1x1 convs), models/voxelmorph/torchvoxelmorph/networks.py:1506-1521 (ConvBlock),
 * :1077-1081 (flow conv).
 *
 * Weights are consumed in "tap-major" packing  w_tcc[tap][Cin][Cout]  (tap = (kd*KH+kh)*KW+kw),
 * produced from the reference's [Cout][Cin][KD][KH][KW] by dfmir_weight_pack.
 * Input index along an axis:  c = o*stride - pad + t ;  dil>1 treats the input as zero-dilated
 * (transposed convolution = dgrad of a strided conv).  pad_mode: 0 zeros, 1 reflect.
 * act: 0 none, 1 leaky-relu(slope) (slope 0 = ReLU), 2 tanh.
 * ---------------------------------------------------------------------------------------- */
typedef struct DfConvGeom {
  int N, Cin, Cout;
  int Di, Hi, Wi;
  int Do, Ho, Wo;
  int KD, KH, KW;
  int stride, dil;
  int pd, ph, pw;
  int pad_mode;
  int act;
  float slope;
} DfConvGeom;

/* y[N,Cout,Do,Ho,Wo] = act(conv(x[N,Cin,Di,Hi,Wi], w) + bias).  bias may be NULL. */
int dfmir_conv_fwd(const DfConvGeom* g, const float* x, const float* w_tcc, const float* bias,
                   float* y, void* stream);
/* The same with a range probe of x supplied: x_amax[0..x_amax_n) are partial maxima whose maximum is max|x|
 * (one value from dfmir_absmax, or the per-plane values dfmir_instnorm_fwd/bwd leave behind; written on the same
 * stream).  The probe lets the 2-D 3x3 stride-1 kernels take the scaled fp16x2 split form (csrc/conv3x3s.hip:
 * 3 matrix products per fp32 product instead of bf16x3's 6); without it -- dfmir_conv_fwd -- those layers run
 * bf16x3 (DFMIR_CONV_SPLIT=bf16x3) or fp32 MFMA.  x_amax may be NULL. */
int dfmir_conv_fwd_scaled(const DfConvGeom* g, const float* x, const float* x_amax, int x_amax_n,
                          const float* w_tcc, const float* bias, float* y, void* stream);
/* out[0] = max(out[0], max_i |x[i]|) (NaN counts as +inf; the caller zero-initialises out).  Replaces nothing in
 * the reference: it is the range probe of the fp16x2 split.  dfmir_instnorm_fwd/bwd produce a probe of their output
 * as a by-product: y_amax / dx_amax = DFMIR_PROBE_SLOTS floats (caller zero-initialises; NULL to skip) whose maximum
 * is max|output|.  x_amax_n of the conv entry points is the number of floats to reduce (1 after dfmir_absmax,
 * DFMIR_PROBE_SLOTS after the InstanceNorm entry points). */
#define DFMIR_PROBE_SLOTS 64
int dfmir_absmax(const float* x, long long n, float* out, void* stream);
/* 3-D 3x3x3 stride-1 "same" convolution (Cin, Cout >= 8) on the 16-bit matrix pipe in the scaled fp16x2 split form
 * (csrc/conv3ds.hip) -- the VoxelMorph U-Net's stride-1 ConvBlocks and their input gradients
 * (models/voxelmorph/torchvoxelmorph/networks.py:73-86,1506-1521).  x_amax as for dfmir_conv_fwd_scaled (required);
 * ws: dfmir_conv3d_split_ws_floats(Cin, Cout) floats of 16-byte aligned scratch (the call splits the weights into it);
 * y_amax (may be NULL): DFMIR_PROBE_SLOTS zero-initialised floats that receive the range probe of y.
 * dfmir_conv3d_split_ok: 1 when the geometry is taken (0 under DFMIR_CONV3D_FP32=1 / DFMIR_CONV_FP32=1). */
int dfmir_conv3d_split_ok(const DfConvGeom* g);
long long dfmir_conv3d_split_ws_floats(int Cin, int Cout);
int dfmir_conv3d_split_fwd(const DfConvGeom* g, const float* x, const float* x_amax, int x_amax_n, const float* w_tcc,
                           float* ws, const float* bias, float* y, float* y_amax, void* stream);
/* The same, computing output channels [0, cout_used) only (y keeps Cout planes; the others are left untouched): the
 * input gradient of a layer fed by cat([up2(a), b]) whose skip part b needs no gradient (the two image channels at the
 * top of the U-Net, networks.py:97-100). */
/* (w_tcc may be NULL in the _sub / _actgrad forms: `ws` then already holds the split of these weights for this
 * cout_used, left by an earlier call -- weights only change at the optimizer step.) */
int dfmir_conv3d_split_fwd_sub(const DfConvGeom* g, const float* x, const float* x_amax, int x_amax_n, const float* w_tcc,
                               float* ws, const float* bias, float* y, float* y_amax, int cout_used, void* stream);
/* The weight gradient of the same layers in the same split form (csrc/conv3dsw.hip; 8 <= Cin <= 48, 8 <= Cout <= 32, or Cout < 8 with Cin <= 32; W % 4 == 0), voxels as the
 * matrix K: dw_tcc[tap][Cin][Cout] += ...   (accumulates, like dfmir_conv_wgrad). */
/* As dfmir_conv3d_split_fwd_sub for a dgrad (g->act == 0) whose result is the gradient w.r.t. the OUTPUT of a
 * LeakyReLU: act_src = that output (shape of y); the epilogue multiplies by the activation's derivative
 * (act_src > 0 ? 1 : act_slope), so y receives the gradient w.r.t. the pre-activation and y_amax its range probe.
 * Replaces the `F.leaky_relu` backward pass between two ConvBlocks
 * (models/voxelmorph/torchvoxelmorph/networks.py:1506-1521, autograd of nn.LeakyReLU(0.2)). */
int dfmir_conv3d_split_fwd_actgrad(const DfConvGeom* g, const float* x, const float* x_amax, int x_amax_n,
                                   const float* w_tcc, float* ws, const float* bias, float* y, float* y_amax,
                                   int cout_used, const float* act_src, float act_slope, void* stream);
/* conv3x3x3(cat(nearest_up2(a), b)) WITHOUT the up-sampled / concatenated tensor -- nn.Upsample(scale_factor=2,
 * mode='nearest') + torch.cat feeding the next ConvBlock (models/voxelmorph/torchvoxelmorph/networks.py:64,97-100).
 * Per output parity class the 27 taps over nearest_up2(a) fall on 2x2x2 voxels of `a`: dfmir_conv3d_up_fwd computes the
 * up-sampled channels' share as eight 8-tap convolutions of `a` with summed weights (8/27 of the products) and leaves
 * the PARTIAL sum in y [N, Cout, 2D, 2H, 2W]; dfmir_conv3d_split_fwd_add then runs the skip channels b (g: the conv
 * over b alone, Cin = Cb; its weights are rows koff .. koff + Cb - 1 of the layer's [27][Ktot][Cout] forward packing)
 * and its epilogue adds the partial sum, the bias, the activation of g and writes y and its range probe.
 * a [N, Ca, D, H, W] with Ca % 8 == 0, W % 4 == 0 (dfmir_conv3d_up_ok); ws: dfmir_conv3d_up_ws_floats /
 * dfmir_conv3d_split_ws_floats(Cb, Cout) floats; w_tcc NULL = ws already holds the split of the current weights. */
int dfmir_conv3d_up_ok(int N, int Ca, int Cout, int D, int H, int W);
/* Every weight split of a network's 3-D convs in ONE launch (all weights change together at the optimizer step;
 * torch.optim.Adam.step, registration_model.py:168-171).  jobs_dev: device array of njobs records of 7 x int64 --
 * {w_tcc, ws, trailer (= ws + its ws_floats - 4), kind | K << 32, M | pair << 32, Ktot | koff << 32, Cb}; kind 0 = the
 * split dfmir_conv3d_split_fwd* makes (K = Cin, M = Cout or cout_used in the plane-pair form), 1 = dfmir_conv3d_up_fwd /
 * _up_skip2_fwd's (K = Ca, Cb = skip channels or 0), 2 = dfmir_conv3d_up_dgrad's.  The entry points then take w_tcc = NULL. */
int dfmir_conv3d_wsplit_batch(const void* jobs_dev, int njobs, void* stream);
int dfmir_conv3d_split_is_pair(int cout_used);
/* The full-resolution 3x3x3 stride-1 layers with Cin x Cout <= 512 -- 32 -> 16, 16 -> 16 and the input gradients 16 <- 16,
 * 32 <- 16 of the `extras` chain (models/voxelmorph/torchvoxelmorph/networks.py:73-86,1506-1521) -- as a z-MARCHING kernel
 * (csrc/conv3dm.hip): a workgroup owns a 16 x 32 column of the volume and walks a segment of planes; every input plane is
 * staged once (in-plane halo only), the accumulators of the three open output planes roll through the registers, the
 * layer's weights are split by the workgroup itself and stay in LDS (no workspace, no weight-split launch).  Same
 * arithmetic as dfmir_conv3d_split_fwd (scaled fp16x2 products, fp32 accumulation); x_amax as there; y_amax
 * (DFMIR_PROBE_SLOTS floats, zeroed by the caller, or NULL) receives the range probe of y.  act_src != NULL (g->act == 0):
 * the result is multiplied by the LeakyReLU derivative act_src > 0 ? 1 : act_slope, as dfmir_conv3d_split_fwd_actgrad.
 * Cin = 16, Cout = 3, g->act == 0, act_src == NULL: the flow head (torchvoxelmorph/networks.py:1076-1080) in the FLOW form --
 * MFMA columns = (open output plane, channel), one accumulator set for the three planes of the march.
 * Needs W % 4 == 0 and 16-byte aligned x, y, act_src, w_tcc; dfmir_conv3d_march_ok says whether the geometry is taken
 * (0 under DFMIR_CONV3D_NO_MARCH / DFMIR_CONV3D_FP32 / DFMIR_CONV_FP32). */
int dfmir_conv3d_march_ok(const DfConvGeom* g);
int dfmir_conv3d_march_fwd(const DfConvGeom* g, const float* x, const float* x_amax, int x_amax_n, const float* w_tcc,
                           const float* bias, float* y, float* y_amax, const float* act_src, float act_slope,
                           void* stream);
/* The flow head (models/voxelmorph/torchvoxelmorph/networks.py:1076-1080: Conv3d(16, 3, 3, padding=1)) and its data
 * gradient (3 -> 16) as plain fp32 FMAs -- neither side fills a matrix-core tile (3 of 16 rows / 3 of 8 K channels).
 * w_tcc: the fp32 tap-major packing [27][Cin][Cout] of dfmir_weight_pack (mode 0 forward, mode 1 data gradient);
 * y = act(conv + bias), times the derivative of the LeakyReLU whose OUTPUT is act_src when act_src != NULL (g->act == 0);
 * y_amax: NULL or the 64 accumulating range-probe slots of y. */
int dfmir_conv3d_tiny_ok(const DfConvGeom* g);
int dfmir_conv3d_tiny_fwd(const DfConvGeom* g, const float* x, const float* w_tcc, const float* bias, float* y,
                          float* y_amax, const float* act_src, float act_slope, void* stream);
/* The first encoder level of the 3-D U-Net (torchvoxelmorph/networks.py:66-86: Conv3d(2, 16, 3, stride=2, padding=1) +
 * LeakyReLU over cat(source, target)): forward as fp32 FMAs from an LDS-staged patch, weight gradient on fp32 MFMA with the
 * operand gathered from the same patch.  w_tcc / dw_tcc: [27][2][16] tap-major (dfmir_weight_pack mode 0); dw accumulates. */
int dfmir_conv3d_s2c2_ok(const DfConvGeom* g);
int dfmir_conv3d_s2c2_fwd(const DfConvGeom* g, const float* x, const float* w_tcc, const float* bias, float* y, float* y_amax,
                          void* stream);
int dfmir_conv3d_s2c2_wgrad(const DfConvGeom* g, const float* x, const float* dy, float* dw_tcc, void* stream);
/* The deeper stride-2 encoder levels (torchvoxelmorph/networks.py:66-71,1506-1521: ConvBlock(ndims, prev_nf, nf, stride=2),
 * Cin a multiple of 4, Cout a multiple of 16 up to 64) on fp32 MFMA from LDS-staged patches (csrc/conv3ds2.hip).
 * _fwd: y = act(conv(x) + bias), y_amax NULL or the 64 accumulating range-probe slots of y; _wgrad: dw_tcc [27][Cin][Cout]
 * and db [Cout] (may be NULL) accumulate (honours dfmir_det_begin); _dgrad: g = the geometry of the data-gradient call as a convolution of dy (Cin =
 * channels of dy, Cout = channels of dx, stride 1, dil 2, pad 1), w_tcc = the dgrad packing (dfmir_weight_pack mode 1),
 * evaluated in the 8 parity classes of the dx voxels (nothing multiplies an inserted zero). */
int dfmir_conv3d_s2_ok(const DfConvGeom* g);
int dfmir_conv3d_s2_fwd(const DfConvGeom* g, const float* x, const float* w_tcc, const float* bias, float* y, float* y_amax,
                        void* stream);
int dfmir_conv3d_s2_wgrad(const DfConvGeom* g, const float* x, const float* dy, float* dw_tcc, float* db, void* stream);
int dfmir_conv3d_s2_dgrad_ok(const DfConvGeom* g);
int dfmir_conv3d_s2_dgrad(const DfConvGeom* g, const float* dy, const float* w_tcc, float* dx, void* stream);
long long dfmir_conv3d_up_ws_floats(int Ca, int Cout);
int dfmir_conv3d_up_fwd(const float* a, const float* a_amax, int a_amax_n, const float* w_tcc, int Ktot, float* ws,
                        float* y, int N, int Ca, int Cout, int D, int H, int W, void* stream);
/* Cb <= 2 (the two input images at the top of the U-Net, networks.py:1105 `x = torch.cat([source, target], dim=1)`): the
 * whole layer in ONE launch -- after the up-sampled channels the same workgroup runs the skip channels from its own
 * full-resolution patch (one MFMA k-step = 2 tap rows x 4 x-taps x 2 channels), then bias, LeakyReLU (act 1) and the
 * range probe.  Ktot of w_tcc == Ca + Cb; ws as dfmir_conv3d_up_ws_floats. */
int dfmir_conv3d_up_skip2_fwd(const float* a, const float* a_amax, int a_amax_n, const float* b, const float* b_amax,
                              int b_amax_n, int Cb, const float* w_tcc, float* ws, const float* bias, float* y,
                              float* y_amax, int N, int Ca, int Cout, int D, int H, int W, int act, float slope,
                              void* stream);
/* d(a) of that layer, directly at low resolution (autograd of nn.Upsample(nearest) + Conv3d: a 2x2x2 sum pool of the
 * conv's input gradient = a 4x4x4 stride-2 convolution of dy, run in parity classes: 64 instead of 216 taps per
 * low-resolution voxel, no up-sampled gradient tensor, no pooling pass).  dy [N, Cout, 2D, 2H, 2W] = gradient w.r.t. the
 * conv's result (after the activation's backward), Cout % 8 == 0; w_tcc = the FORWARD packing [27][Ktot][Cout] or NULL (ws
 * current); act_src (optional) = a when a is the output of a LeakyReLU(act_slope) feeding only this layer: da then is the
 * gradient w.r.t. that activation's input; da_amax (optional) = range probe of da. */
long long dfmir_conv3d_up_dgrad_ws_floats(int Ca, int Cout);
int dfmir_conv3d_up_dgrad(const float* dy, const float* dy_amax, int dy_amax_n, const float* w_tcc, int Ktot, float* ws,
                          float* da, float* da_amax, const float* act_src, float act_slope, int N, int Ca, int Cout, int D,
                          int H, int W, void* stream);
int dfmir_conv3d_split_fwd_add(const DfConvGeom* g, const float* b, const float* b_amax, int b_amax_n, const float* w_tcc,
                               int Ktot, int koff, float* ws, const float* bias, float* y, float* y_amax, void* stream);
int dfmir_conv3d_split_wgrad_ok(const DfConvGeom* g);
int dfmir_conv3d_split_wgrad(const DfConvGeom* g, const float* x, const float* x_amax, int x_amax_n, const float* dy,
                             const float* dy_amax, int dy_amax_n, float* dw_tcc, void* stream);
/* The weight (and bias) gradient of conv3x3x3 over X = cat(nearest_up2(a), b) without building X (autograd of
 * nn.Upsample + torch.cat + Conv3d, networks.py:64,97-100): a [N, Ca, D/2, H/2, W/2] is read at (z>>1, y>>1, x>>1) while
 * the operand patch is staged.  g = the whole layer (Cin = Ca + Cb); Ca % 8 == 0; D, H even, W % 8 == 0; x_amax = a range
 * probe valid for both parts; db may be NULL. */
int dfmir_conv3d_split_wgrad_upcat(const DfConvGeom* g, const float* a, const float* b, int Ca, const float* x_amax,
                                   int x_amax_n, const float* dy, const float* dy_amax, int dy_amax_n, float* dw_tcc,
                                   float* db, void* stream);
/* The same gradient, the up-sampled channels in PARITY CLASSES (csrc/conv3duw.hip): a 3x3x3 tap of output voxel 2V + p over
 * nearest_up2(a) reads a[V + floor((p + d - 1) / 2)], so G[p][i] = sum_V a[V + p - 1 + i] (x) dy[2V + p] (64 matrices per
 * layer, K = the LOW-resolution voxels) holds the whole gradient: 8 / 27 of the direct form's products and one pass over dy
 * with no halo.  The skip channels b run on the direct kernel (which also sums db).  Ca == 32, Cout % 8 == 0, Cout <= 32,
 * D, H even, W % 8 == 0; ws = dfmir_conv3d_upwgrad_ws_floats() floats, owned by the call until the stream has passed it.
 * Two skip channels (the network's input images at the top level) and db are FUSED into the same launch (rows = (tap,
 * channel) from x- and y-paired images of b; db as the row of a constant operand); wider skips and db go through the direct
 * kernel on rows Ca.. of dw_tcc.  A/B switches: DFMIR_UPWGRAD_8WAVE=1 (two waves per SIMD, not fused), DFMIR_UPWGRAD_NSEG=n
 * forces the z split. */
int dfmir_conv3d_upwgrad_ok(const DfConvGeom* g, int Ca);
long long dfmir_conv3d_upwgrad_ws_floats(void);
int dfmir_conv3d_upwgrad(const DfConvGeom* g, const float* a, const float* b, int Ca, const float* x_amax, int x_amax_n,
                         const float* dy, const float* dy_amax, int dy_amax_n, float* dw_tcc, float* db, float* ws,
                         void* stream);
/* The same, also accumulating the bias gradient db[Cout] += sum dy from the units it stages anyway (db may be NULL).
 * Layers with fewer than 8 output channels (the 16 -> 3 flow conv, networks.py:1077) are taken with the operand roles
 * swapped: rows = (tap, co) from shifted dy, columns = ci. */
int dfmir_conv3d_split_wgrad_db(const DfConvGeom* g, const float* x, const float* x_amax, int x_amax_n, const float* dy,
                                const float* dy_amax, int dy_amax_n, float* dw_tcc, float* db, void* stream);
/* 1 when dfmir_conv3d_split_wgrad / _db run this layer on conv3d_wgrad_march_k (csrc/conv3dwm.hip): Cin 32, Cout 16 (the
 * full-resolution ConvBlock of `extras`, networks.py:73-86) -- all 27 tap matrices resident in one wave's accumulators, the
 * workgroup marching along z, both operands read once.  A/B: DFMIR_CONV3D_NO_WGRAD_MARCH=1; DFMIR_WGRAD_MARCH_NSEG=n. */
int dfmir_conv3d_wgrad_is_march(const DfConvGeom* g);
/* The launcher's own predicate: the geometry above AND x, dy 16-byte aligned (they are read as quads; unaligned operands
 * run on the tiled kernel).  _is_march(g) answers for aligned operands. */
int dfmir_conv3d_wgrad_is_march_at(const DfConvGeom* g, const float* x, const float* dy);
/* out[0..DFMIR_PROBE_SLOTS) = max(a, b): the probe of cat([nearest_up2(a), b]) from its inputs' probes. */
int dfmir_probe_merge(const float* a, const float* b, float* out, void* stream);
/* dw_tcc[tap][Cin][Cout] += sum_{n,o} x(gathered) * dy      (accumulates; same packing as w_tcc). */
int dfmir_conv_wgrad(const DfConvGeom* g, const float* x, const float* dy, float* dw_tcc,
                     void* stream);
/* db (may be NULL): the bias gradient db[Cout] += sum_{n,o} dy of the same layer, accumulated by this call -- inside
 * the wgrad kernel where it reads dY anyway (split 3x3 kernels), otherwise by a dfmir_bias_grad pass. */
int dfmir_conv_wgrad_scaled(const DfConvGeom* g, const float* x, const float* x_amax, int x_amax_n,
                            const float* dy, const float* dy_amax, int dy_amax_n, float* dw_tcc, float* db,
                            void* stream);
/* The same with the maxima of |dy| PER PLANE, dy_pmax[N][Cout] (as dfmir_instnorm_bwd_pmax leaves them; NULL = as
 * above): the fp16x2 weight-gradient kernel (Cout > 64) then scales dY per output channel -- the scale is uniform along
 * its reduction axis -- so a channel far below the tensor maximum keeps its 22 bits. */
int dfmir_conv_wgrad_scaled_ch(const DfConvGeom* g, const float* x, const float* x_amax, int x_amax_n, const float* dy,
                               const float* dy_amax, int dy_amax_n, const float* dy_pmax, float* dw_tcc, float* db,
                               void* stream);
/* db[C] += sum_{n,s} dy[n,C,s]   (accumulates). */
int dfmir_bias_grad(const float* dy, float* db, int N, int C, long long S, void* stream);
/* mode 0: w_tcc[t][ci][co] = w[co][ci][t]           (forward packing)
 * mode 1: w_tcc[t][co][ci] = w[co][ci][T-1-t]       (dgrad packing: roles of Cin/Cout swapped, taps flipped)
 * The packed buffer holds dfmir_weight_pack_floats(Cout, Cin, T) floats: the tap-major fp32 weights, then
 * (T == 9 only) the same weights pre-split into bf16 triples for the 3x3 kernels.  Callers treat it as
 * opaque and hand it to dfmir_conv_fwd unchanged. */
long long dfmir_weight_pack_floats(int Cout, int Cin, int T);
int dfmir_weight_pack(const float* w, float* w_tcc, int Cout, int Cin, int T, int mode, void* stream);
/* g[co][ci][t] = g_tcc[t][ci][co]  (gradient back to the reference's parameter layout). */
int dfmir_weight_unpack(const float* g_tcc, float* g, int Cout, int Cin, int T, void* stream);
/* The deferred form of the same step for every conv of a backward pass at once (one launch per train step instead
 * of unpack + add + clear per layer): job j adds its tap-major accumulator src[T][Cin][Cout] into the gradient in the
 * reference layout, dst[Cout][Cin][T] += src (torch accumulates p.grad the same way, autograd/functions/
 * accumulate_grad.h), and zeroes src.  `jobs` is DEVICE memory; max_total = max_j Cout*Cin*T. */
/* dfmir_conv_fwd_scaled with an epilogue y = act(conv(x) + bias) + res + fold(ring), for the geometries
 * dfmir_conv3x3_res_ok(g) accepts (the shared-tile split 3x3 kernel).  res[N][Cout][Ho][Wo] (optional): a second
 * gradient of the same tensor -- the skip branch of a ResnetBlock, dx = dgrad(dy) + d out (models/networks.py:1219-1221).
 * ring (optional): see dfmir_conv3x3_reflect_ring. */
int dfmir_conv3x3_res_ok(const DfConvGeom* g);
int dfmir_conv3x3_fwd_scaled_res(const DfConvGeom* g, const float* x, const float* x_amax, int x_amax_n,
                                 const float* w_tcc, const float* bias, const float* res, const float* ring,
                                 int ring_len, float* y, void* stream);

/* Input gradient of conv3x3(ReflectionPad2d(1)(x)) (ResnetBlock, models/networks.py:1190-1214) in two parts.  The
 * gradient is the fold of the full correlation of dy on the (H+2) x (W+2) padded frame; the frame's interior is the
 * zero-padded "same" dgrad (dfmir_conv3x3_fwd_scaled_res with the dgrad packing, pad 1), and its one-pixel ring is
 * four 3-tap 1-D convolutions of the border lines of dy, computed here into ring[N][4][Cin][ring_len] (strips: top,
 * bottom, left, right; index = frame coordinate along the strip), which the interior call folds in through its
 * `ring` argument.  g = the FORWARD geometry; wd_packed = dfmir_weight_pack(mode 1); dy_amax as for
 * dfmir_conv_fwd_scaled.  dfmir_conv3x3_reflect_ring_ok(g) != 0 iff this library build takes the geometry;
 * dfmir_conv3x3_reflect_ring_len(g) = ring_len. */
int dfmir_conv3x3_reflect_ring_ok(const DfConvGeom* g);
int dfmir_conv3x3_reflect_ring_len(const DfConvGeom* g);
int dfmir_conv3x3_reflect_ring(const DfConvGeom* g, const float* dy, const float* dy_cols, const float* dy_amax,
                               int dy_amax_n, const float* wd_packed, float* ring, void* stream);

/* Data gradient AND weight gradient of one 3x3 stride-1 layer in ONE launch (csrc/conv3x3s.hip, conv3x3_bwd_pair_k): a
 * 1-D grid holds the workgroups of both kernels, so the atomic tail of the weight gradient and the last workgroups of the
 * data gradient no longer each end a launch with idle CUs -- autograd's Conv2d backward (models/networks.py:1201,1214),
 * whose two halves both read only dy.  gd = the data gradient as a convolution of dy (Cin = the layer's Cout, Cout = its
 * Cin, zero padding 1; for a reflect-padded layer the zero-padded interior, its ring through `ring` as in
 * dfmir_conv3x3_fwd_scaled_res), gw = the layer's forward geometry (the weight gradient's).  Arguments as in
 * dfmir_conv3x3_fwd_scaled_res (dy, dy_amax, wd_packed, res, ring, ring_len, dx) and dfmir_conv_wgrad_scaled_ch (x,
 * x_amax, dy_pmax, dw_tcc, db; accumulates).  dX is bit-identical to the separate call's, dW / db are accumulated by the
 * same atomics.  When either side would not run on the kernels the pair carries (dfmir_conv3x3_bwd_pair_ok(gd, gw) == 0:
 * other geometry, deterministic mode, DFMIR_NO_BWD_PAIR=1, DFMIR_BWD_PAIR=0) the call issues the two separate launches;
 * *paired tells which happened (1 = one launch). */
int dfmir_conv3x3_bwd_pair_ok(const DfConvGeom* gd, const DfConvGeom* gw);
int dfmir_conv3x3_bwd_pair(const DfConvGeom* gd, const DfConvGeom* gw, const float* dy, const float* dy_amax,
                           int dy_amax_n, const float* dy_pmax, const float* wd_packed, const float* res,
                           const float* ring, int ring_len, float* dx, const float* x, const float* x_amax,
                           int x_amax_n, float* dw_tcc, float* db, int* paired, void* stream);
/* dy_cols (optional): [N*Cout][2][H], the first and last column of dy as left by dfmir_instnorm_bwd_cols. */

/* Every packing of a train step at once (the weights of all layers change together, at the optimizer step): the same
 * result as njobs dfmir_weight_pack calls, in two launches.  `jobs` is HOST memory; `table_dev` is njobs * 64 bytes of
 * device scratch owned by the caller, (re)written when upload != 0 -- pass 0 while the same jobs come back. */
typedef struct DfPackJob {
  const float* w;      /* [Cout][Cin][T] */
  float* packed;       /* dfmir_weight_pack_floats(Cout, Cin, T) floats */
  int Cout, Cin, T, mode;
} DfPackJob;
int dfmir_weight_pack_batch(const DfPackJob* jobs, int njobs, void* table_dev, int upload, void* stream);

typedef struct DfUnpackJob {
  float* src;
  float* dst;
  int Cout, Cin, T, reserved;
} DfUnpackJob;
int dfmir_weight_unpack_add_batch(const DfUnpackJob* jobs, int njobs, long long max_total, void* stream);

/* The Cin == 1 stem directly: nn.ReflectionPad2d(3) + nn.Conv2d(1, ngf, 7) (models/networks.py:982-983).
 * x[N][1][H][W], w[Cout][1][7][7] (reference layout), Cout <= 64; pad 3, pad_mode 0 zero / 1 reflect.
 * fwd: y = conv + bias.  wgrad: dw[Cout][49] += sum dy (x) x_padded-shifted, db[Cout] += sum dy (db optional); both
 * ACCUMULATE (zero the buffers first). */
int dfmir_conv7x7_c1_fwd(const float* x, const float* w, const float* bias, float* y, int N, int H, int W, int Cout,
                         int pad_mode, void* stream);
int dfmir_conv7x7_c1_wgrad(const float* x, const float* dy, float* dw, float* db, int N, int H, int W, int Cout,
                           int pad_mode, void* stream);

/* 7x7 convs of the generator as 1x1 GEMMs (models/networks.py:982-983 Conv2d(1,64,7) and :1022-1024
 * Conv2d(64,1,7)+Tanh, both behind ReflectionPad2d(3)):
 *   tapstack: S[n][c*K*K+tap][p] = x[n][c][map(p + tap - pad)]            (then a 1x1 conv K*K -> Cout)
 *   tapsum  : y[n][c][p] = act(bias[c] + sum_tap Z[n][c*K*K+tap][map(p + tap - opad)])   (after a 1x1 conv Cin -> K*K)
 * map = reflect (pad_mode 1) or zero (pad_mode 0); *_bwd are the exact adjoints (gather form). */
int dfmir_tapstack_fwd(const float* x, float* s, int N, int C, int H, int W, int K, int pad,
                       int pad_mode, void* stream);
int dfmir_tapstack_bwd(const float* ds, float* dx, int N, int C, int H, int W, int K, int pad,
                       int pad_mode, void* stream);
int dfmir_tapsum_fwd(const float* z, const float* bias, float* y, int N, int C, int Hz, int Wz, int Ho,
                     int Wo, int K, int opad, int pad_mode, int act, float slope, void* stream);
int dfmir_tapsum_bwd(const float* dy, float* dz, int N, int C, int Hz, int Wz, int Ho, int Wo, int K,
                     int opad, int pad_mode, void* stream);

/* ------------------------------------------------------------------------------------------
 * InstanceNorm2d(affine=False, eps) [+ ReLU] [+ residual add]  -- models/networks.py:113-131,
 * 984-985, 1190-1221 (x + conv_block(x)).  One (n,c) plane of S elements per workgroup.
 * y = res + relu?((x-mean)*rstd) ; mean/rstd [planes] are saved for backward.
 * ---------------------------------------------------------------------------------------- */
/* Statistics of InstanceNorm only (round 6): mean / rstd per plane and the range probe of relu?(IN(x)); y is NOT written --
 * a consumer that normalises while it stages its operand follows.  S in {4096, 16384, 65536} (dfmir_instnorm_stats_ok). */
int dfmir_instnorm_stats_ok(long long S);
int dfmir_instnorm_stats(const float* x, float* mean, float* rstd, int planes, long long S, float eps, int relu,
                         float* y_amax, void* stream);
int dfmir_instnorm_fwd(const float* x, const float* res, float* y, float* mean, float* rstd,
                       int planes, long long S, float eps, int relu, float* y_amax, void* stream);
int dfmir_instnorm_bwd(const float* dy, const float* x, const float* mean, const float* rstd,
                       float* dx, int planes, long long S, int relu, float* dx_amax, void* stream);
/* The same, also writing dx's first and last column compactly, dx_cols[planes][2][H] (S = H*W; supported iff
 * dfmir_instnorm_bwd_cols_ok(S, W)): the reflect ring of the next conv's dgrad reads them from there. */
int dfmir_instnorm_bwd_cols_ok(long long S, int W);
int dfmir_instnorm_bwd_cols(const float* dy, const float* x, const float* mean, const float* rstd, float* dx, int planes,
                            long long S, int relu, float* dx_amax, float* dx_cols, int W, void* stream);
/* Superset of the two (S in {4096, 16384, 65536}; dx_cols may be NULL): also dx_pmax[planes] <- max |dx| of each plane. */
int dfmir_instnorm_bwd_pmax_ok(long long S);
int dfmir_instnorm_bwd_pmax(const float* dy, const float* x, const float* mean, const float* rstd, float* dx, int planes,
                            long long S, int relu, float* dx_amax, float* dx_cols, int W, float* dx_pmax, void* stream);

/* InstanceNorm2d + ReLU + Downsample (blur-pool) as one pass per plane: models/networks.py:984-996, modules
 * (5,6,7) and (9,10,11) of the generator -- the full-resolution normalised tensor feeds only the blur and no backward
 * needs it.  H x W = 256 x 256 or 128 x 128 (dfmir_in_relu_blurdown_ok).  z [planes, H/2, W/2]; mean / rstd [planes]
 * saved for backward; z_amax (may be NULL): DFMIR_PROBE_SLOTS zero-initialised floats, a bound of max|z|.
 * bwd: dx from dz, x, mean, rstd; dx_amax / dx_pmax as dfmir_instnorm_bwd_pmax (may be NULL). */
int dfmir_in_relu_blurdown_ok(int H, int W);
int dfmir_in_relu_blurdown_fwd(const float* x, float* z, float* mean, float* rstd, int planes, int H, int W, float eps,
                               float* z_amax, void* stream);
int dfmir_in_relu_blurdown_bwd(const float* dz, const float* x, const float* mean, const float* rstd, float* dx,
                               int planes, int H, int W, float* dx_amax, float* dx_pmax, void* stream);

/* elementwise activation backward from the saved OUTPUT y: act 1 leaky(slope), 2 tanh. */
int dfmir_act_bwd(const float* dy, const float* y, float* dx, long long n, int act, float slope,
                  void* stream);
/* The same, also leaving the range probe of dx in dx_amax[DFMIR_PROBE_SLOTS] (zero-initialised by the caller; pointers
 * 16-byte aligned): dx feeds the split dgrad / wgrad of the layer in front of the activation. */
int dfmir_act_bwd_amax(const float* dy, const float* y, float* dx, long long n, int act, float slope,
                       float* dx_amax, void* stream);

/* ------------------------------------------------------------------------------------------
 * Anti-aliased resampling of the generator -- models/networks.py:37-60 (Downsample: reflect pad 1,
 * depthwise [1 2 1]x[1 2 1]/16, stride 2) and :73-93 (Upsample: replicate pad 1, depthwise
 * conv_transpose 4x4 [1 3 3 1]^2/16 stride 2, cropped to 2H x 2W).
 * ---------------------------------------------------------------------------------------- */
int dfmir_blur_down_fwd(const float* x, float* y, int planes, int H, int W, void* stream);
int dfmir_blur_down_bwd(const float* dy, float* dx, int planes, int H, int W, void* stream);
int dfmir_blur_up_fwd(const float* x, float* y, int planes, int H, int W, void* stream);
int dfmir_blur_up_bwd(const float* dy, float* dx, int planes, int H, int W, void* stream);
/* nn.ReflectionPad2d(p) -- models/networks.py:982,1022 (materialised only for NCE layer 0). */
int dfmir_reflect_pad2d_fwd(const float* x, float* y, int planes, int H, int W, int p, void* stream);
int dfmir_reflect_pad2d_bwd(const float* dy, float* dx, int planes, int H, int W, int p, void* stream);
/* dx = fold(dy) + add: the adjoint of ReflectionPad2d summed with a second gradient of the same tensor in one pass --
 * ResnetBlock's `out = x + self.conv_block(x)` (models/networks.py:1219-1221): x feeds the padded conv AND the skip,
 * so its gradient is fold(d conv path) + d out.  add[planes][H][W]. */
int dfmir_reflect_pad2d_bwd_add(const float* dy, const float* add, float* dx, int planes, int H, int W, int p,
                                void* stream);

/* nn.Upsample(scale 2, nearest) + torch.cat([up(a), b], 1) -- torchvoxelmorph/networks.py:64,97-100.
 * a[N,Ca,Da,Ha,Wa] -> factor sd (1 for 2-D, 2 for 3-D) in D and 2 in H,W; b[N,Cb,Da*sd,2Ha,2Wa]. */
int dfmir_upcat_fwd(const float* a, const float* b, float* y, int N, int Ca, int Cb, int Da, int Ha,
                    int Wa, int sd, void* stream);
int dfmir_upcat_bwd(const float* dy, float* da, float* db, int N, int Ca, int Cb, int Da, int Ha,
                    int Wa, int sd, void* stream);

/* torch.cat([a, b], dim=1) -- torchvoxelmorph/networks.py:1110 (source|target into the U-Net).
 * SA = Ca*S, SB = Cb*S elements per sample.  bwd: da/db may be NULL. */
int dfmir_cat_channels_fwd(const float* a, const float* b, float* y, long long N, long long SA,
                           long long SB, void* stream);
int dfmir_cat_channels_bwd(const float* dy, float* da, float* db, long long N, long long SA,
                           long long SB, void* stream);
/* y = mult * x -- `vec * self.scale` (layers.py:65), `-pos_flow` (networks.py:1125). */
int dfmir_scale(const float* x, float* y, long long n, float mult, void* stream);

/* ------------------------------------------------------------------------------------------
 * SpatialTransformer.forward  (torchvoxelmorph/layers.py:30-48): out = grid_sample(src, grid+flow)
 * with align_corners=True, padding_mode='zeros'; flow is a displacement in voxels, channel d =
 * axis d.  mode 0 bilinear/trilinear, 1 nearest.  add_identity: out += src (VecInt step
 * v + warp(v,v), layers.py:64-68; needs C == ndims).
 * Backward: dsrc accumulates (atomic scatter); dflow is written, or (flow_into_src) accumulated
 * into dsrc for the VecInt self-warp where src == flow.
 * ---------------------------------------------------------------------------------------- */
int dfmir_warp2d_fwd(const float* src, const float* flow, float* out, int B, int C, int H, int W,
                     int mode, int add_identity, void* stream);
int dfmir_warp2d_bwd(const float* dout, const float* src, const float* flow, float* dsrc,
                     float* dflow, int B, int C, int H, int W, int add_identity, int flow_into_src,
                     void* stream);
int dfmir_warp3d_fwd(const float* src, const float* flow, float* out, int B, int C, int D, int H,
                     int W, int mode, int add_identity, void* stream);
int dfmir_warp3d_bwd(const float* dout, const float* src, const float* flow, float* dsrc,
                     float* dflow, int B, int C, int D, int H, int W, int add_identity,
                     int flow_into_src, void* stream);
/* The same adjoint WITHOUT device-scope atomics on d(src), bit-reproducible (csrc/warp_win.hip, "owner gathers"): every
 * workgroup accumulates its tile's scatter in a fixed-point LDS window, writes it densely to a scratch slot, and a
 * second pass lets each d(src) cell sum the neighbouring tiles' windows that cover it, in fixed order; voxels displaced
 * beyond the 3x3(x3)-tile neighbourhood go through a list and the scalar routine (atomics).  nd = 2 (D ignored) or 3;
 * W % 4 == 0.  dsrc is written entirely (no zero-fill needed); ws = dfmir_warp_bwd_own_ws_floats(...) floats of
 * 16-byte aligned scratch (0: shape not eligible -> use dfmir_warp{2,3}d_bwd). */
long long dfmir_warp_bwd_own_ws_floats(int nd, int B, int C, int D, int H, int W);
int dfmir_warp_bwd_own(int nd, const float* dout, const float* src, const float* flow, float* dsrc, float* dflow, int B,
                       int C, int D, int H, int W, int add_identity, int flow_into_src, float* ws, void* stream);

/* ResizeTransform (layers.py:71-97): F.interpolate(align_corners=True, bi/tri-linear) fused with the
 * scalar rescale `mult`.  D == 1 for 2-D.  bwd is the adjoint in gather form (writes dx; no atomics). */
int dfmir_resize_fwd(const float* x, float* y, int planes, int Di, int Hi, int Wi, int Do, int Ho,
                     int Wo, float mult, void* stream);
int dfmir_resize_bwd(const float* dy, float* dx, int planes, int Di, int Hi, int Wi, int Do, int Ho,
                     int Wo, float mult, void* stream);
/* The same adjoint as three 1-D passes (W, H, D; the trilinear weights are separable): ws = dfmir_resize_bwd_ws_floats
 * floats (16-B aligned) for the two intermediates.  5x faster than the one-pass gather on the x2 flow up-sampling. */
long long dfmir_resize_bwd_ws_floats(int planes, int Di, int Hi, int Wi, int Do, int Ho, int Wo);
int dfmir_resize_bwd_sep(const float* dy, float* dx, int planes, int Di, int Hi, int Wi, int Do, int Ho, int Wo,
                         float mult, float* ws, void* stream);

/* Cubic B-spline free-form deformation (build-defined; Rueckert et al. 1999), nd = 2 or 3 (nd == 2: D, sz are not read).
 * Per axis a: integer spacing s_a in 1 .. 8, extent n_a >= 1, m_a = (n_a - 1) / s_a + 4 control points, point j at voxel
 * s_a (j - 1).  With q_a = x_a / s_a, t_a = (x_a % s_a) / s_a and the uniform cubic B-spline basis B_0 = (1-t)^3 / 6,
 * B_1 = (3t^3 - 6t^2 + 4) / 6, B_2 = (-3t^3 + 3t^2 + 3t + 1) / 6, B_3 = t^3 / 6:
 *   fwd  y[p,x] = sum over l in {0..3}^nd of prod_a B_{l_a}(t_a) ctrl[p,q + l]      ctrl [planes][(m_z)][m_y][m_x] -> y
 *        [planes][(D)][H][W]; a zero grid gives +0.0 everywhere.
 *   bwd  the adjoint in gather form, dctrl[p,j] = sum over the x with q_a(x) in {j_a - 3 .. j_a} of prod_a B_{j_a - q_a}(t_a)
 *        dy[p,x], as one pass per axis (x, y, z); no atomics, a fixed summation order: bit-identical from run to run.  dctrl
 *        is written entirely.  ws = dfmir_bspline_bwd_ws_floats(...) floats of 16-byte aligned scratch for the
 *        intermediates (-1: the library refuses the shape: planes > 65535, 2^31 elements or more, W > 7944, more than
 *        65535 * 256 control points per plane). */
int dfmir_bspline_fwd(int nd, const float* ctrl, float* y, int planes, int D, int H, int W, int sz, int sy, int sx,
                      void* stream);
long long dfmir_bspline_bwd_ws_floats(int nd, int planes, int D, int H, int W, int sz, int sy, int sx);
int dfmir_bspline_bwd(int nd, const float* dy, float* dctrl, int planes, int D, int H, int W, int sz, int sy, int sx,
                      float* ws, void* stream);

/* ------------------------------------------------------------------------------------------
 * PatchNCE path -- models/networks.py:602-619 (PatchSampleF.forward), :493-502 (Normalize),
 * models/patchnce.py:14-55 (PatchNCELoss.forward).
 * Sampled features are kept channel-major [C][rows] (rows = B*P, row r = b*P + p) so the 2-layer
 * MLP runs as 1x1 convs over `rows` pixels; the reference's [B*P, C] tensors are the transposed
 * VIEW of this buffer.
 * ---------------------------------------------------------------------------------------- */
/* out[c][b*P+p] = feat[b][c][ids[p]]   (feat [B,C,S], ids int64 [P] shared by the batch). */
int dfmir_patch_gather_fwd(const float* feat, const long long* ids, float* out, int B, int C,
                           long long S, int P, void* stream);
int dfmir_patch_gather_bwd(const float* dout, const long long* ids, float* dfeat, int B, int C,
                           long long S, int P, void* stream);
/* The same scatter into a gradient that already holds another consumer's contribution (ids must be DISTINCT -- a
 * P-subset, as torch.randperm yields them, networks.py:609-610: plain load + store instead of atomics; this also
 * holds for the grouped forms below), keeping its per-plane range
 * probe valid: dfeat_amax[DFMIR_PROBE_SLOTS] (the dx_amax of dfmir_instnorm_bwd) is raised to |new value| where needed. */
int dfmir_patch_gather_bwd_amax(const float* dout, const long long* ids, float* dfeat, int B, int C, long long S,
                                int P, float* dfeat_amax, void* stream);
/* Grouped forms: ids[G][P]; image b uses the ids of group b / (B / G) -- the query images of G NCE terms stacked along
 * the batch, each sampled at its own term's positions (registration_model.py:237-253 called once per term in the
 * reference).  bwd_g scatters (dfeat must hold zeros or another gradient); dfeat_amax optional as above. */
int dfmir_patch_gather_fwd_g(const float* feat, const long long* ids, float* out, int B, int C, long long S, int P,
                             int G, void* stream);
int dfmir_patch_gather_bwd_g(const float* dout, const long long* ids, float* dfeat, int B, int C, long long S, int P,
                             int G, float* dfeat_amax, void* stream);
/* bwd_g that also keeps the per-plane maxima dfeat_pmax[B*C] (see dfmir_instnorm_bwd_pmax) valid.  accumulates */
int dfmir_patch_gather_bwd_gp(const float* dout, const long long* ids, float* dfeat, int B, int C, long long S, int P,
                              int G, float* dfeat_amax, float* dfeat_pmax, void* stream); /* accumulates */
/* The grouped scatter for ARBITRARY ids (repeats allowed within a group: a caller-supplied `patch_ids` list,
 * models/networks.py:602-608): accumulates with atomics, as torch's index backward does.  dfeat_amax / dfeat_pmax
 * optional (NULL), kept valid as above. */
int dfmir_patch_gather_bwd_any(const float* dout, const long long* ids, float* dfeat, int B, int C, long long S, int P,
                               int G, float* dfeat_amax, float* dfeat_pmax, void* stream); /* accumulates */
/* Key side of several NCE terms in one launch: group g gathers its Bper images from srcs[g] ([Bper,C,S]; srcs is a HOST
 * array of G <= 8 device pointers, copied by value into the launch) at ids[g][0..P) -> out[c][(g*Bper+b)*P+p].
 * Replaces `feat_k_pool, sample_ids = self.netF(feat_k, num_patches, None)` called once per term
 * (models/registration_model.py:244-245; gather = models/networks.py:604-611). */
int dfmir_patch_gather_fwd_multi(const float* const* srcs, int G, const long long* ids, float* out, int Bper, int C,
                                 long long S, int P, void* stream);
/* The PatchNCE head of one layer in one launch (PatchSampleF.forward, models/networks.py:602-619): sample ids[g][0..P) from
 * group g's images srcs[g] [Bper, C, S], Linear(C, 256) + ReLU, Linear(256, 256), x / (||x||_2 + eps) -> out [256][G*Bper*P]
 * (channel-major rows, row = (g*Bper + b)*P + p).  w1 [C][256], w2 [256][256]: forward packings of dfmir_weight_pack
 * (T = 1); C <= 256.  Optional outputs for the backward: nrm [rows], xs [C][rows] (sampled features), hs [256][rows]
 * (after the ReLU), ypre [256][rows] (before the normalisation).  srcs: HOST array of G <= 8 device pointers. */
int dfmir_nce_head_fwd(const float* const* srcs, int G, const long long* ids, const float* w1, const float* b1,
                       const float* w2, const float* b2, float* out, float* nrm, float* xs, float* hs, float* ypre,
                       int Bper, int C, long long S, int P, float eps, void* stream);
/* Patch positions drawn on the device: out[layer][set][0..P) = a uniformly random P-subset of [0, sizes[layer]) --
 * what `torch.randperm(H*W)[:num_patches]` (models/networks.py:609-610) yields per layer and per netF call, for
 * n_sets calls at once (the set, not its order, is what PatchNCELoss sees).  sizes: HOST array of n_layers <= 8
 * counts.  state: 3 device uint64 {seed, draw counter, 0}; the kernel advances the counter itself, so a captured
 * hipGraph draws fresh ids at every replay.  Deterministic for a given (seed, counter).  P <= 1024; sizes[l] >= 2P
 * (rejection sampling) or P <= sizes[l] <= 4096 (a sorted permutation). */
int dfmir_patch_ids_draw(unsigned long long* state, const long long* sizes, int n_layers, int n_sets, int P,
                         long long* out, void* stream);
/* per row: y = x / (sqrt(sum_c x^2) + eps); norm[rows] saved. */
int dfmir_l2norm_fwd(const float* x, float* y, float* norm, int C, long long rows, float eps, void* stream);
int dfmir_l2norm_bwd(const float* dy, const float* x, const float* norm, float* dx, int C,
                     long long rows, float eps, void* stream);
/* q,k: [C][rows]; G consecutive groups of R = rows/G rows share negatives (R % 16 == 0).
 * loss[rows]; probs[rows][R+1] = softmax of [pos | neg]/T, saved for backward. */
int dfmir_patchnce_fwd(const float* q, const float* k, float* loss, float* probs, long long rows,
                       int C, int G, float T, void* stream);
int dfmir_patchnce_bwd(const float* dloss, const float* probs, const float* k, float* dq,
                       long long rows, int C, int G, float T, void* stream);

/* ------------------------------------------------------------------------------------------
 * Scalar losses.  `out` is a 1-float device scalar; `ws` is a small zero-able workspace (8 floats).
 * ---------------------------------------------------------------------------------------- */
/* calculate_L1_loss (registration_model.py:255-263) with mask = (a>thr)|(b>thr)
 * (registration_model.py:160-161) when mask == NULL, else the given byte mask.
 * out = sum(|a-b|*m)/sum(m)  (0 when sum(m)==0). */
int dfmir_masked_l1_fwd(const float* a, const float* b, const unsigned char* mask, float thr,
                        float* ws, float* out, long long n, void* stream);
int dfmir_masked_l1_bwd(const float* a, const float* b, const unsigned char* mask, float thr,
                        const float* ws, const float* gout, float* da, float* db, long long n,
                        void* stream);
/* smooothing_loss (registration_model.py:25-32) / Grad_Loss l2 (util/losses.py:81-130):
 * mean over axes of mean(squared forward difference) (D==1: 2 axes). flow [B,C,D,H,W].
 * ws: dfmir_flow_smooth_ws_floats() floats of scratch (need not be zeroed): every workgroup leaves its three partial sums in
 * its own slots and the finaliser adds them in index order -- the loss is bit-reproducible. */
long long dfmir_flow_smooth_ws_floats(void);
int dfmir_flow_smooth_fwd(const float* flow, float* ws, float* out, int B, int C, int D, int H,
                          int W, void* stream);
int dfmir_flow_smooth_bwd(const float* flow, const float* gout, float* dflow, int B, int C, int D,
                          int H, int W, void* stream);
/* The same with the penalty chosen: 1 = 'l1' (mean |forward difference|), 2 = 'l2' -- Grad_Loss(penalty=...)
 * (util/losses.py:81-130) and vxm Grad(penalty).loss (models/voxelmorph/torchvoxelmorph/losses.py:93-117). */
int dfmir_flow_smooth_fwd_p(const float* flow, float* ws, float* out, int B, int C, int D, int H,
                            int W, int penalty, void* stream);
int dfmir_flow_smooth_bwd_p(const float* flow, const float* gout, float* dflow, int B, int C, int D,
                            int H, int W, int penalty, void* stream);
/* Bending energy, the second-order regulariser of a flow (build-defined: the reference's util/losses.py:81-130 is first-order
 * only).  flow u: [B][C][D][H][W] fp32, any C >= 1; axes a in the order (z,) y, x with extents n_a and voxel spacing
 * h_a > 0 (hz, hy, hx).  D == 1 is the 2-D field it is: y and x only, hz is not read.  Omega = the voxels whose whole 3^nd
 * neighbourhood lies in the volume, 1 <= p_a <= n_a - 2 on every axis.  For p in Omega
 *   u_aa(p) = (u(p+e_a) - 2 u(p) + u(p-e_a)) / h_a^2
 *   u_ab(p) = (u(p+e_a+e_b) - u(p+e_a-e_b) - u(p-e_a+e_b) + u(p-e_a-e_b)) / (4 h_a h_b),   a < b
 *   e(p)    = sum_a u_aa(p)^2 + 2 sum_{a<b} u_ab(p)^2
 * dfmir_bend_fwd: out[0] = sum_{b,c,p in Omega} e / N, N = B C |Omega|.  dfmir_bend_bwd: dflow (every element written) =
 * gout[0] * the exact adjoint, with U = the derivative value extended by 0 outside Omega:
 *   dL/du(p) = (2 / N) [ sum_a (U_aa(p-e_a) - 2 U_aa(p) + U_aa(p+e_a)) / h_a^2
 *              + 2 sum_{a<b} (U_ab(p-e_a-e_b) - U_ab(p-e_a+e_b) - U_ab(p+e_a-e_b) + U_ab(p+e_a+e_b)) / (4 h_a h_b) ]
 * in gather form: no atomics, no derivative volume in memory, the backward reads u alone.  Refused ("invalid argument",
 * nothing is launched): a NULL pointer, D == 2 or H, W < 3 (Omega would be empty), a spacing that is not positive and
 * finite, B * C * D * H * W >= 2^31.  ws: dfmir_bend_ws_floats(B, C, D, H, W) floats (-1 for a refused shape), 8-byte
 * aligned, need not be zeroed: one double slot per workgroup, added in a fixed order -- loss and gradient are bit-identical
 * from run to run.  Nothing syncs, allocates or keeps state (gout is read on the device): both calls capture into a hipGraph. */
long long dfmir_bend_ws_floats(int B, int C, int D, int H, int W);
int dfmir_bend_fwd(const float* flow, float* ws, float* out, int B, int C, int D, int H, int W, float hz, float hy,
                   float hx, void* stream);
int dfmir_bend_bwd(const float* flow, const float* gout, float* dflow, int B, int C, int D, int H, int W, float hz,
                   float hy, float hx, void* stream);
/* Jacobian determinant of the deformation phi(x) = x + u(x): fold penalty, determinant map and regularity statistics
 * (build-defined: the reference has no Jacobian code).  flow u: [B][nd][(D)][H][W] fp32, nd = 2 or 3 (D is not read when
 * nd == 2); channel a is the displacement in voxels along axis a, in the order (z,) y, x, as the warp kernels read a flow.
 * border m >= 1; Omega_m = the voxels with m <= p_a <= n_a - 1 - m on every axis (m = 1 is the bending energy's Omega).  For
 * p in Omega_m
 *   J_ab(p) = delta_ab + (u_a(p + e_b) - u_a(p - e_b)) / 2          central differences
 *   d(p)    = det J(p)                                              2x2 or 3x3, written out (no pivoting)
 * The determinant does not depend on the voxel spacing: in physical units J_phys = H J H^-1 with H = diag(h), which has
 * the same determinant, so no call here takes a spacing.
 * dfmir_jacdet_fwd: out[0] = sum_{b, p in Omega_m} psi(d(p)) / N, psi(d) = max(0, eps - d)^power, N = B |Omega_m|.
 * dfmir_jacdet_bwd: dflow (every element written) = gout[0] * the exact adjoint in gather form (no atomics, no derivative
 * volume in memory, the backward reads u alone): with W_ab(p) = psi'(d(p)) cof(J(p))_ab on Omega_m and 0 outside, cof = the
 * cofactor matrix dd/dJ_ab, psi'(d) = -power max(0, eps - d)^(power - 1) (power 1: -1 where d < eps, 0 otherwise),
 *   dL/du_a(q) = (1 / 2N) sum_b [ W_ab(q - e_b) - W_ab(q + e_b) ]
 * dfmir_jacdet_map: detmap [B][1][(D)][H][W] = d(p) on Omega_m and exactly 1.0f, the identity's value, outside.
 * dfmir_jacdet_stats: stats [B][6] doubles, per sample over Omega_m: the count of d <= 0, min d, max d, mean d, mean l and
 * std l (the population standard deviation), l = log(max(d + log_offset, log_floor)); the sums are taken in double, those
 * of l about l at the first voxel of Omega_m, std = sqrt(max(0, S2/n - (S1/n)^2)).
 * Refused ("invalid argument", nothing is launched): a NULL pointer, nd outside {2, 3}, B < 1, border < 1, an axis shorter
 * than 2 border + 1, power outside {1, 2}, eps negative or not finite, log_offset < 0, log_floor <= 0 or either not
 * finite, B * nd * voxels >= 2^31.  ws: dfmir_jacdet_ws_floats(nd, B, D, H, W) floats (-1 for a geometry that every border
 * refuses), 8-byte aligned as `stats` is, need not be zeroed: one slot set per workgroup, added in a fixed order -- every
 * output is bit-identical from run to run.  16-byte loads where W % 4 == 0 and flow is 16-byte aligned.  Nothing syncs,
 * allocates or keeps state (gout is read on the device): all four calls capture into a hipGraph. */
long long dfmir_jacdet_ws_floats(int nd, int B, int D, int H, int W);
int dfmir_jacdet_fwd(int nd, const float* flow, float* ws, float* out, int B, int D, int H, int W, int border, float eps,
                     int power, void* stream);
int dfmir_jacdet_bwd(int nd, const float* flow, const float* gout, float* dflow, int B, int D, int H, int W, int border,
                     float eps, int power, void* stream);
int dfmir_jacdet_map(int nd, const float* flow, float* detmap, int B, int D, int H, int W, int border, void* stream);
int dfmir_jacdet_stats(int nd, const float* flow, float* ws, double* stats, int B, int D, int H, int W, int border,
                       double log_offset, double log_floor, void* stream);
/* Inverse consistency of a pair of displacement fields (build-defined: the reference has no such term).  u, v:
 * [B][nd][(D)][H][W] fp32, nd = 2 or 3 (D is not read when nd == 2); channel i displaces axis i in voxels, in the order
 * (z,) y, x, exactly as the warp kernels read a flow.
 *   r(x)    = u(x) + v(x + u(x))      v sampled (bi/tri)linearly, corners outside the volume read as 0: r = u + warp(v, u)
 *   IC_b    = sum over the nd * S elements of sample b of r^2 / (nd * S)     (S = voxels per sample)
 * A voxel whose sample point leaves the volume contributes |u|^2.  dfmir_invcons_fwd: per_sample[b] = IC_b, loss[0] = their
 * mean, rmax[0] = max |r_c| over the call (dfmir_invcons_bwd reads it: keep it between the two calls).
 * dfmir_invcons_bwd, the exact adjoint with k = 2 gout[0] / (B nd S); du and dv are written entirely, either may be NULL:
 *   du_c(x) = k ( r_c(x) + sum_c' r_c'(x) d_c v_c'(x + u(x)) )    d_c = the derivative of the interpolant as the warp
 *             backward forms it: corner differences, zero-padded corners taking part as zeros
 *   dv      = the transpose of the interpolation applied to k r (a scatter to the up to 2^nd corners).  Where W % 4 == 0 and
 *             u, du, dv, ws are 16-byte aligned, k r is written once and handed to the owner-gather adjoint of the warp
 *             (dfmir_warp_bwd_own: no device-scope atomics, bit-reproducible as that call is).  Elsewhere it is summed with
 *             global atomics as 64-bit fixed-point integers whose unit lies >= 29 bits below max |k r|: bit-identical from run
 *             to run as well (a max |k r| that is not finite makes dv NaN), but several times slower.
 * r is recomputed, never stored.  Refused ("invalid argument", nothing is launched): nd outside {2, 3}, B < 1, an extent
 * < 2, a NULL pointer, B * nd * S >= 2^31.  ws: dfmir_invcons_ws_floats / dfmir_invcons_bwd_ws_floats floats (-1 for a
 * refused shape), 8-byte aligned, need not be zeroed; the backward's may be NULL when dv is.  The forward sums through one
 * double slot per workgroup in a fixed order: the values are bit-identical from run to run.  16-byte accesses of u and du
 * where W % 4 == 0 and both are 16-byte aligned.  Nothing syncs, allocates or keeps state (gout is read on the device): both
 * calls capture into a hipGraph. */
long long dfmir_invcons_ws_floats(int nd, int B, int D, int H, int W);
int dfmir_invcons_fwd(int nd, const float* u, const float* v, float* ws, float* per_sample, float* loss, float* rmax, int B,
                      int D, int H, int W, void* stream);
long long dfmir_invcons_bwd_ws_floats(int nd, int B, int D, int H, int W);
int dfmir_invcons_bwd(int nd, const float* u, const float* v, const float* gout, const float* rmax, float* du, float* dv,
                      float* ws, int B, int D, int H, int W, void* stream);
/* Composition of two displacement fields and fixed-point inversion of one (build-defined: the reference has neither).  Fields
 * as above: [B][nd][(D)][H][W] fp32, nd = 2 or 3 (D is not read when nd == 2), channel i displaces axis i in voxels, order
 * (z,) y, x; sampling (bi/tri)linear, corners outside the volume read as 0, the sampling of dfmir_invcons_* and of the warp
 * kernels, with the same guard: no float is converted to int for a NaN or a far-away sample point and every address formed
 * lies inside its tensor.
 * dfmir_compose_fwd:   out(x) = u(x) + v(x + u(x)) = u + warp(v, u): warp(src, out) is warp(warp(src, v), u) in the
 *   continuum, u is the warp applied last.  Replaces u + dfmir_warp_fwd(v, u) (a warped tensor written and read again).
 * dfmir_compose_bwd, for an incoming gradient g of out; du and dv are written entirely, either may be NULL:
 *   du_c(x) = g_c(x) + sum_c' g_c'(x) d_c v_c'(x + u(x))    d_c = corner differences, zero-padded corners taking part as zeros
 *   dv      = the transpose of the interpolation applied to g.  Where W % 4 == 0 and u, g, dv, ws are 16-byte aligned g is
 *             handed to the owner-gather adjoint of the warp as it is (dfmir_warp_bwd_own: no device-scope atomics,
 *             bit-reproducible as that call is).  Elsewhere, and everywhere under DFMIR_INVCONS_FIXED64, it is summed with
 *             global atomics as 64-bit fixed-point integers whose unit lies >= 29 bits below max |g|, which is taken on the
 *             device: bit-identical from run to run as well (a max |g| that is not finite makes dv NaN), several times slower.
 *   These are dfmir_invcons_bwd's formulas with k r replaced by g, and the same kernel body.  ws: dfmir_compose_bwd_ws_floats
 *   floats, 8-byte aligned, need not be zeroed, may be NULL when dv is.  out and du are bit-identical from run to run.
 * dfmir_flow_invert:   w_0 = init (NULL = zeros),  r_k(x) = w_k(x) + u(x + w_k(x)),  w_{k+1} = w_k - r_k (= -u(x + w_k) up to
 *   rounding); a voxel stops updating once max_c |r_k,c| <= tol and keeps its w and r from then on (tol = 0: every voxel does
 *   `iters` updates; a voxel with a NaN never stops).  w = w_iters.  stats: with history != 0 [iters + 1][B][2], row k =
 *   (rms_k, max_k) of r_k, rms_k = sqrt(sum over the voxels and channels of sample b of r_k^2 / S), max_k = max |r_k,c| (NaN
 *   if any is); with history == 0 [B][2], those of r_iters alone.  ONE launch runs every iteration with w in registers (each
 *   voxel's iteration reads only its own w and a gather of u) and a second one adds the per-workgroup double sums in a fixed
 *   order: w and stats are bit-identical from run to run.  Replaces `iters` rounds of dfmir_warp_fwd + dfmir_scale, which
 *   write and re-read a field twice per iteration.  The iteration converges where u is a contraction (Lipschitz constant
 *   < 1); at the volume border the zero padding makes u drop to 0 within one cell, so a field that is not small there does
 *   not converge there -- the residual says so.  ws: dfmir_flow_invert_ws_floats(.., iters, history) floats, 8-byte aligned,
 *   need not be zeroed.
 * Refused ("invalid argument", nothing is launched): nd outside {2, 3}, B < 1, an extent < 2, B * nd * S >= 2^31, a NULL
 * pointer other than the optional ones, iters outside [0, 64], a tol that is negative or not finite; the _ws_floats calls
 * return -1 for these.  16-byte accesses of u, out / u, g, du / init, w where W % 4 == 0 and those are 16-byte aligned.
 * Nothing syncs, allocates or keeps state: every call captures into a hipGraph. */
int dfmir_compose_fwd(int nd, const float* u, const float* v, float* out, int B, int D, int H, int W, void* stream);
long long dfmir_compose_bwd_ws_floats(int nd, int B, int D, int H, int W);
int dfmir_compose_bwd(int nd, const float* u, const float* v, const float* g, float* du, float* dv, float* ws, int B, int D,
                      int H, int W, void* stream);
long long dfmir_flow_invert_ws_floats(int nd, int B, int D, int H, int W, int iters, int history);
int dfmir_flow_invert(int nd, const float* u, const float* init, float* w, float* stats, float* ws, int B, int D, int H,
                      int W, int iters, float tol, int history, void* stream);
/* Discrete displacement search: the first stage of a two-stage (discrete search, then Adam) instance registration
 * (build-defined: the reference has no such stage).  Everything fp32, nd = 2 or 3 (D is not read when nd == 2), S = voxels per
 * sample.  The displacement index k = 0 .. K - 1, K = (2r + 1)^nd, enumerates d_k in {-r .. r}^nd in row-major order (dz,) dy,
 * dx with -r first; d_k is in voxels of the grid the features live on, in the flow's channel order (z,) y, x.
 * dfmir_dsearch_pool:   in [B][C][(D)][H][W], 1 <= C <= 16, window g^nd, stride g, the remainder at the far faces dropped:
 *   out[b][c][X] = the mean of in[b][c][g X + {0 .. g-1}^nd] over [B][C][(D/g)][H/g][W/g] (added in double in a fixed order,
 *   rounded once); packed = the same values voxel-major, [B][(D/g)][H/g][W/g][Cp] with Cp = C rounded up to 4 and zeros in the
 *   padding channels (dfmir_warp_ssd_pack's layout), what dfmir_dsearch_cost reads.  Either of out / packed may be NULL, not
 *   both; g = 1 copies (packs).
 * dfmir_dsearch_cost:   fixp, movp packed as above (16-byte aligned) on [(D)][H][W]; cost [B][K][(D)][H][W] contiguous,
 *   cost[b][k][x] = (1 / C) sum_c (fix[b][c][x] - mov[b][c][x + d_k])^2,  mov reading 0 outside the volume (the zero padding of
 *   the warp kernels).  The channels are added in the order c = 0 .. Cp - 1 with one fma each for every k, so displacements
 *   whose sample lies outside the volume tie bit for bit at sum_c fix_c^2 / C.  Every cost is written once (no atomics, no
 *   read-modify-write); r in [1, 4] (nd = 3) or [1, 8] (nd = 2).
 * dfmir_dsearch_argmin: idx[b][x] = argmin_k ( cost[b][k][x] + coeff * sum_a (d_k[a] - soft[b][a][x])^2 ) as int32 [B][S],
 *   the squares added in the order (z,) y, x; the LOWEST k wins a tie (a strict < walking k upwards from +inf); a NaN is never
 *   selected, and where every value is NaN (or +inf) the result is index 0.  disp[b][a][x] = d_idx[a], fp32 [B][nd][S].
 *   soft [B][nd][S] or NULL = the plain argmin (coeff is then not read); coeff finite and >= 0.
 * dfmir_dsearch_smooth: out[b][a][x] = the mean of disp[b][a][.] over those of the 3^nd neighbours of x (x included) that lie
 *   inside the volume, added in the order (dz,) dy, dx and divided by their number -- not by 3^nd: a constant field comes back
 *   constant at the faces.  out must not alias disp.
 * Refused ("invalid argument", nothing is launched): nd outside {2, 3}, B < 1, C outside [1, 16], an extent (for the pooling:
 * a pooled extent) < 2, g < 1, r outside its range, a coeff that is negative or not finite, a NULL pointer other than the
 * optional ones, 2^31 or more elements in any tensor (B * K * S for the cost volume, B * Cp * S for packed features), and for
 * dfmir_dsearch_cost B above 65535.  Nothing syncs, allocates or keeps state, and every output is bit-identical from run to
 * run: every call captures into a hipGraph. */
int dfmir_dsearch_pool(int nd, const float* in, float* out, float* packed, int B, int C, int D, int H, int W, int g,
                       void* stream);
int dfmir_dsearch_cost(int nd, const float* fixp, const float* movp, float* cost, int B, int C, int D, int H, int W, int r,
                       void* stream);
int dfmir_dsearch_argmin(int nd, const float* cost, const float* soft, float coeff, int* idx, float* disp, int B, int D, int H,
                         int W, int r, void* stream);
int dfmir_dsearch_smooth(int nd, const float* disp, float* out, int B, int D, int H, int W, void* stream);
/* Warped-feature SSD, the data term of instance optimisation (build-defined: the reference has no such term).  M, F:
 * [B][C][(D)][H][W] fp32 features of the moving / fixed image, 1 <= C <= 16; phi: [B][nd][(D)][H][W] fp32, nd = 2 or 3 (D is
 * not read when nd == 2), channel d displaces axis d in voxels, in the order (z,) y, x, exactly as the warp kernels read a
 * flow; mask m: [B][S] fp32 weights or NULL (S = voxels per sample).
 *   e_c(x) = M_c(x + phi(x)) - F_c(x)      M sampled (bi/tri)linearly, align_corners, corners outside the volume read as 0
 *   L      = sum over (b, c, x) of e^2 / (B C S);  with a mask  L = sum m(x) mean_c e_c(x)^2 / sum m,  0 for an empty mask
 *   L_b    = the same over sample b alone
 *   dL/dphi_d(x) = k(x) sum_c e_c(x) d_d M_c(x + phi(x)),  k = 2 gout / (B C S), masked 2 gout m(x) / (C sum m);  d_d = the
 *            derivative of the interpolant in the cell floor() selects: corner differences, zero-padded corners taking part
 *            as zeros.  There is no gradient to M, F or m.
 * dfmir_warp_ssd_pack: Mp = M voxel-major, [B][(D)][H][W][Cp] with Cp = C rounded up to 4 and zeros in the padding channels
 * (B * S * Cp floats, 16-byte aligned): made once for as many calls as M lives, a corner then costs Cp / 4 16-byte loads.
 * dfmir_warp_ssd_fwd_grad, ONE pass over the voxels: per_sample[b] = L_b, loss[0] = L, unit = the gradient for gout = 1
 * (masked: not yet divided by sum m) and scale[0] = what is left to multiply it with (1; masked 1 / sum m, 0 for an empty
 * mask).  unit may be NULL; dfmir_warp_ssd_fwd is that call.  dfmir_warp_ssd_bwd: dflow = unit * gout[0] * scale[0] over n
 * floats, both read on the device.  Mp or M may be NULL: the gather reads Mp unless it is NULL or DFMIR_WARPSSD_PLANAR is on
 * and M is given.  No warped tensor, no e tensor, no atomics: e^2 is added in double per thread into one double slot per
 * workgroup (and sum m into a second), and the slots are added in a fixed order -- every output is bit-identical from run to
 * run.  No float is converted to int for a NaN or a far-away sample point and every address formed lies inside its tensor.
 * 16-byte accesses of phi, F and unit where W % 4 == 0 and the three are 16-byte aligned.  Refused ("invalid argument",
 * nothing is launched): nd outside {2, 3}, B < 1, C outside [1, 16], an extent < 2, a NULL pointer other than the optional
 * ones, B * Cp * S >= 2^31 or B * nd * S >= 2^31.  ws: dfmir_warp_ssd_ws_floats floats (-1 for a refused shape), 8-byte
 * aligned, need not be zeroed.  Nothing syncs, allocates or keeps state: every call captures into a hipGraph. */
long long dfmir_warp_ssd_ws_floats(int nd, int B, int C, int D, int H, int W);
int dfmir_warp_ssd_pack(int nd, const float* M, float* Mp, int B, int C, int D, int H, int W, void* stream);
int dfmir_warp_ssd_fwd(int nd, const float* Mp, const float* M, const float* F, const float* phi, const float* mask,
                       float* ws, float* per_sample, float* loss, float* scale, int B, int C, int D, int H, int W,
                       void* stream);
int dfmir_warp_ssd_fwd_grad(int nd, const float* Mp, const float* M, const float* F, const float* phi, const float* mask,
                            float* ws, float* per_sample, float* loss, float* scale, float* unit, int B, int C, int D, int H,
                            int W, void* stream);
int dfmir_warp_ssd_bwd(const float* unit, const float* gout, const float* scale, float* dflow, long long n, void* stream);
/* Affine pre-alignment (build-defined: the reference has no affine stage).  theta: [B][nd][nd + 1] fp32 = [A | t] in CENTRED
 * voxel coordinates, axis order (z,) y, x; nd = 2 or 3 (D is not read when nd == 2).  With c_a = (n_a - 1) / 2 and
 * q(x) = (x - c, 1):   y(x) = c + A (x - c) + t,   flow_a(x) = y_a(x) - x_a = sum_j (A - I)_aj (x - c)_j + t_a  (formed like
 * that, in fp32, j ascending, t last).  Identity is [I | 0].  P = nd (nd + 1) parameters, flattened row-major (a, j).
 * dfmir_affine_flow: flow [B][nd][S] (the warp kernels' convention); 16-byte stores where W % 4 == 0 and flow is aligned.
 * dfmir_affine_flow_bwd: dtheta[b][a][j] = sum_x dflow[b][a][x] q_j(x), fp32 [B][P]: sums in double, two stages in a fixed
 * order, no atomics.
 * dfmir_affine_system: the affine SSD of packed moving features Mp (dfmir_warp_ssd_pack's layout, 1 <= C <= 16) against F
 * [B][C][S] under an optional mask m [B][S], in ONE pass over the voxels.  M is sampled at x + flow(x) exactly as
 * dfmir_warp_ssd_fwd samples it (the same cell, guards and corner differences, the flow in dfmir_affine_flow's arithmetic).
 *   e_c = M_c(y) - F_c,  r = sum_c e_c dM_c(y)  (nd),  G = sum_c dM_c dM_c^T  (nd x nd),  N_b = sum_x m  (S without a mask)
 *   L_b = sum_x m mean_c e^2 / N_b      g_b = (2 / (C N_b)) sum_x m r (x) q  = dL_b / dtheta_b
 *   H_b = (2 / (C N_b)) sum_x m G (x) (q q^T)     the Gauss-Newton matrix of L_b, symmetric positive semi-definite
 *   L   = sum_b sum_x m mean_c e^2 / sum_b N_b,   gb_b = dL / dtheta_b = g_b N_b / sum_b N_b;   all 0 where the weights sum to 0
 * out (doubles, 8-byte aligned): [0] L, [1 .. B] L_b, gb [B][P], g [B][P] and -- full != 0 only -- H [B][P][P]:
 * 1 + B + 2 B P (+ B P P) doubles.  Per-workgroup sums in double, added in a fixed order: bit-identical from run to run.
 * dfmir_affine_lm_step: one Levenberg-Marquardt step per sample b on the device (infer.affine_init states the loop).
 * state[b] = (L_acc, mu, g_acc [P], H_acc [P][P]) doubles; with L = Lb[b]:  L finite and L <= L_acc accepts (theta_acc =
 * trial, L_acc = L, (g_acc, H_acc) = (g, H), and for k > 0 mu = max(mu mu_down, 1e-12)), otherwise mu = min(mu mu_up, 1e12);
 * then (H_acc[f,f] + mu diag H_acc[f,f]) d = -g_acc[f] over the free parameters f (all, or with translation != 0 the t
 * column) by Cholesky in fp64 -- a pivot <= 0 or not finite: d = 0 and the row is flagged singular -- and trial =
 * fp32(theta_acc + d) on f, theta_acc elsewhere; hist[b] = (L, L_acc, mu, accepted, singular), 5 doubles.
 * ws: dfmir_affine_ws_floats floats (-1 for a refused shape), 8-byte aligned, need not be zeroed; it serves _flow_bwd and
 * _system.  Refused ("invalid argument", nothing is launched): nd outside {2, 3}, B < 1, an extent < 2, C outside [1, 16], 2^31
 * or more elements in the flow or the packed features, a NULL pointer other than mask, a misaligned buffer, k < 0, mu_up <= 1,
 * mu_down outside (0, 1].  Nothing syncs, allocates or keeps state. */
long long dfmir_affine_ws_floats(int nd, int B, int D, int H, int W);
int dfmir_affine_flow(int nd, const float* theta, float* flow, int B, int D, int H, int W, void* stream);
int dfmir_affine_flow_bwd(int nd, const float* dflow, float* ws, float* dtheta, int B, int D, int H, int W, void* stream);
int dfmir_affine_system(int nd, const float* Mp, const float* F, const float* theta, const float* mask, float* ws, double* out,
                        int full, int B, int C, int D, int H, int W, void* stream);
int dfmir_affine_lm_step(int nd, const double* Lb, const double* g, const double* H, float* theta_acc, float* trial,
                         double* state, double* hist, int B, int k, int translation, double mu_up, double mu_down,
                         void* stream);
/* Gaussian smoothing of fields and feature volumes (build-defined: the reference has no such filter).  in, out: [planes][(D)]
 * [H][W] fp32, planes = B * C, nd = 2 or 3 (D and sz are not read when nd == 2); sigma (sz, sy, sx) in voxels, finite and >= 0;
 * truncate finite and > 0.  Per axis a:  r_a = ceil(truncate * sigma_a) <= DFMIR_GAUSS_MAX_RADIUS,  w_a[k] = exp(-k^2 / (2
 * sigma_a^2)) for |k| <= r_a, formed in double and rounded to fp32.  The filter is separable and RENORMALISED AT THE FACES:
 *   out(i) = sum_k w[k] in(i + k) [i + k inside] / sum_k w[k] [i + k inside]        along each axis in turn (x, y, then z)
 * so a constant comes back constant (dfmir_dsearch_smooth's convention; not zero padding).  A sum starts from its centre
 * term and adds the pairs w[k] (in(i - k) + in(i + k)), k = 1 .. r_a; the divisor is formed in the kernel.  sigma_a == 0 leaves
 * axis a alone bit for bit, and with every sigma 0 out is a copy of in.  An extent smaller than the window is legal: the whole
 * axis then lies inside every window.  2-D: ONE launch, the tile and its halo filtered along both axes in LDS.  3-D: the (y, x)
 * pass per plane into tmp, then the z pass as the same kernel on the view [planes][D][H W]: two reads and two writes of the
 * tensor (one of each when sz == 0 or sy == sx == 0).  tmp: planes * D * H * W floats, read only when both passes run (may be
 * NULL otherwise); in, out and tmp must not alias.  16-byte accesses where the row length (W; for the z pass H W) is a
 * multiple of 4 and the pointers are aligned.  Every output is written once from sums in a fixed order: bit-identical from
 * run to run.  Refused ("invalid argument", nothing is launched): nd outside {2, 3}, planes < 1, an extent < 2, 2^31 or more
 * elements, a sigma that is negative or not finite, a truncate that is not finite and > 0, a radius above
 * DFMIR_GAUSS_MAX_RADIUS, a NULL or aliased pointer.  Nothing syncs, allocates or keeps state. */
#define DFMIR_GAUSS_MAX_RADIUS 16     /* a 32 x 64 tile with a halo of 16 on every side: 24 KiB of LDS, and 16 KiB for the x pass */
int dfmir_gauss_smooth(int nd, const float* in, float* out, float* tmp, long long planes, int D, int H, int W, double sz,
                       double sy, double sx, double truncate, void* stream);
/* Cubic B-spline image resampling (build-defined: the reference has nothing above first order).  Images and coefficients:
 * [planes][(D)][H][W] fp32, planes = B * C, nd = 2 or 3 (D is not read when nd == 2), every extent >= 1.
 *   Index reflection, an axis of extent n:  n == 1: refl(i) = 0;  n > 1: j = i mod (2 n - 2) taken non-negative, refl(i) = j if
 *   j < n, else 2 n - 2 - j: the whole-sample mirror  d c b | a b c d | c b a, at ANY distance from the volume.
 *   Prefilter c = P s, per axis (the axes commute): along one axis c solves  (c[refl(i - 1)] + 4 c[i] + c[refl(i + 1)]) / 6 =
 *   s[i]  (scipy.ndimage.spline_filter1d(order=3, mode='mirror')); for n == 1, c = s.  Evaluated as the FIR form
 *     c[i] = sum_{|k| <= 16} sqrt(3) z^|k| s[refl(i + k)],   z = sqrt(3) - 2,
 *   the exact inverse truncated where the tail is below 8e-10 max |s|; the weights are formed in double and rounded to fp32, a
 *   sum adds the pairs w[k] (s[i - k] + s[i + k]) from k = 16 down to 1 and the centre term last.
 *   Sampling at p (per axis i = floor(p), t = p - i):
 *     w0 = (1 - t)^3 / 6,  w1 = (3 t^3 - 6 t^2 + 4) / 6,  w2 = (-3 t^3 + 3 t^2 + 3 t + 1) / 6,  w3 = t^3 / 6
 *     w0' = -(1 - t)^2 / 2,  w1' = (3 t^2 - 4 t) / 2,  w2' = (-3 t^2 + 2 t + 1) / 2,  w3' = t^2 / 2
 *     out = sum over the 4^nd taps of  prod_a w_ka(t_a) * c[refl(i_a - 1 + k_a)]
 *   which is scipy.ndimage.map_coordinates(order=3, mode='mirror'): mirror extension at any distance, NOT the zero padding of
 *   the linear warp kernels.  The result is not confined to the range of s (the spline overshoots at edges; nothing clamps).
 * dfmir_spline_prefilter: in -> out, out of place.  2-D: ONE launch, the tile and a halo of 16 reflected cells filtered along both
 * axes in LDS.  3-D: the (y, x) pass per plane into tmp, then the z pass as the same kernel on the view [planes][D][H W].  tmp:
 * planes * D * H * W floats, read only when both passes run (nd == 3, D > 1 and H > 1 or W > 1; may be NULL otherwise); in, out
 * and tmp must not alias.  An axis of extent 1 is left alone bit for bit.  16-byte accesses where the row length (W; for the z
 * pass H W) is a multiple of 4 and the pointers are aligned.
 * dfmir_warp_cubic_fwd: out[b][c][x] = the spline of coef[b][c] (PREFILTERED coefficients) at p = x + flow[b][:][x]; flow
 * [B][nd][S] in voxels, channel a displaces axis a, order (z,) y, x -- the warp kernels' convention.  floor and t are taken
 * from the flow (floor(p) = x + floor(flow), t = flow - floor(flow)).  A position that is not finite, or whose fp32 sum x + flow
 * has magnitude >= 2^24 on any axis, gives out = 0 and a zero gradient.
 * dfmir_warp_cubic_bwd_flow: dflow[b][a][x] = sum_c dout[b][c][x] * d out[b][c][x] / d p_a  (w' on axis a, w on the others),
 * continuous in p; the channels are added in channel order and every element is written once: no atomics.  There is no
 * gradient to coef here.
 * One thread per voxel; the 4 reflected indices and weights per axis are formed once per voxel, without reflection when every
 * tap is inside.  Every output of the three calls is bit-identical from run to run.  Refused ("invalid argument", nothing is
 * launched): nd outside {2, 3}, planes, B or C < 1, an extent < 1 (warp: > 2^24), 2^31 or more elements, a NULL or aliased
 * pointer.  Nothing syncs, allocates or keeps state. */
int dfmir_spline_prefilter(int nd, const float* in, float* out, float* tmp, long long planes, int D, int H, int W, void* stream);
int dfmir_warp_cubic_fwd(int nd, const float* coef, const float* flow, float* out, int B, int C, int D, int H, int W,
                         void* stream);
int dfmir_warp_cubic_bwd_flow(int nd, const float* dout, const float* coef, const float* flow, float* dflow, int B, int C,
                              int D, int H, int W, void* stream);
/* The demons force: a per-voxel Gauss-Newton step on the warped-feature SSD (build-defined: the reference has no such
 * solver).  Mp, F, phi and mask are dfmir_warp_ssd_fwd's: Mp the packed moving features (dfmir_warp_ssd_pack), F [B][C][S], 1 <=
 * C <= 16, phi [B][nd][S] in voxels, mask [B][S] or NULL.  Per voxel x, with p = x + phi(x), sampled exactly as
 * dfmir_warp_ssd_fwd samples (the same cell, guards and corner differences):
 *   m_c = M_c(p),  J_c = the derivative of the interpolant in the cell floor() selects (nd),  e_c = m_c - F_c(x)
 *   s = (1/C) sum_c e_c^2        g = (1/C) sum_c e_c J_c  (nd)        H = (1/C) sum_c J_c J_c^T  (nd x nd)
 *   d(x) = -(H + (s / max_step^2) I)^-1 g          [B][nd][S], the update in voxels, channel order (z,) y, x
 * With C = 1 this is Thirion's force with Vercauteren's step bound, -e J / (|J|^2 + e^2 / max_step^2); for any C |d(x)| <=
 * max_step / 2 (H = K^T K, g = K^T e' with K = J / sqrt C, e' = e / sqrt C, and ||(K^T K + a I)^-1 K^T|| <= 1 / (2 sqrt a)).
 * Where g is exactly 0 -- that includes points with no corner inside the volume -- d = +0 without a division; elsewhere s > 0
 * and the matrix is positive definite: the three sums are added in double (each product of two floats is exact there) and the system is solved in closed form by
 * its L D L^T factors in double -- near convergence s / max_step^2 falls below eps32 |J|^2, where fp32 sums or the adjugate are off by
 * the order of |d| --, and if a component of
 * the result is not finite the vector is 0.  A mask weight <= 0 gives d(x) = 0; a positive weight leaves d as it is and weights
 * only the energy.  per_sample[b] = L_b and loss[0] = L: the (masked) mean of s with dfmir_warp_ssd_fwd's reduction (double
 * slots per workgroup, added by one workgroup in a fixed order; 0 for an empty mask).  ONE gather pass: the cell is formed once
 * per voxel, the channels pass in groups of four from the packed copy; no warped tensor, no e tensor, no atomics; every output
 * is bit-identical from run to run.  16-byte accesses of phi, F and d where W % 4 == 0 and the three are 16-byte aligned.
 * Refused ("invalid argument", nothing is launched): what dfmir_warp_ssd_fwd refuses, a NULL pointer other than mask, d == phi,
 * a max_step that is not finite and > 0.  ws: dfmir_demons_ws_floats floats (-1 for a refused shape), 8-byte aligned, need not
 * be zeroed.  Nothing syncs, allocates or keeps state. */
long long dfmir_demons_ws_floats(int nd, int B, int C, int D, int H, int W);
int dfmir_demons_force(int nd, const float* Mp, const float* F, const float* phi, const float* mask, float* ws,
                       float* per_sample, float* loss, float* d, float max_step, int B, int C, int D, int H, int W,
                       void* stream);
/* Landmark (keypoint) registration error of a displacement field (build-defined: the reference has no landmark code).
 * flow u: [B][nd][(D)][H][W] fp32, nd = 2 or 3 (D is not read when nd == 2); channel a displaces axis a in voxels, in the
 * order (z,) y, x, exactly as the warp kernels read a flow: warped(x) = moving(x + u(x)) with x in the fixed image's grid,
 * so a point q of the FIXED image corresponds to q + u(q) in the MOVING image.  fixed_pts q, moving_pts p: [B][K][nd] fp32
 * voxel coordinates, axis order as the flow's channels; weight w: [B][K] fp32 or NULL (= all ones; 0 marks a padding entry);
 * spacing h = (hz, hy, hx) > 0, applied per axis (hz is not read when nd == 2).  With S_a the extent of axis a:
 *   m_bk = q + u_b(q)      u_b sampled (bi/tri)linearly at q in the cell i0_a = min(floor(q_a), S_a - 2): a point on the
 *                          upper face q_a = S_a - 1 reads the last cell with weight 1 on its upper corner, never outside
 *   r_bk = h (.) (m_bk - p),   d_bk = |r_bk|_2, the target registration error of the landmark
 *   valid: w > 0, every coordinate of q and p finite, 0 <= q_a <= S_a - 1 on every axis.  An invalid landmark has d = NaN
 *          (and a NaN row in `mapped`), contributes to no sum and gets no gradient.
 *   loss  = sum w d^2 / Wsum (penalty 0, 'l2') or sum w d / Wsum (penalty 1, 'tre'; the derivative at d = 0 is 0), over the
 *           valid landmarks of the whole call, Wsum = their sum of w.  Wsum = 0: loss 0 and an all-zero gradient, not NaN.
 * dfmir_landmark_fwd: mapped[b][k][:] = m (may be NULL), d[b][k] = d, per_sample[b] = the w-weighted mean of d over the valid
 * landmarks of sample b (NaN without one), loss[0], wsum[0] = Wsum (dfmir_landmark_bwd reads it: keep it between the two
 * calls).  moving_pts == NULL: the call only maps points -- `mapped` must be given; d, per_sample, loss, wsum and ws are not
 * written and may be NULL; validity is then that of q and w alone.
 * dfmir_landmark_bwd: the gradient to the flow only, dflow[b][a][corner] += gout[0] (w / Wsum) dl/dr_a h_a cornerweight with
 * dl/dr_a = 2 r_a ('l2') or r_a / d ('tre'); dflow is written entirely, zeros elsewhere.  After the zero fill every landmark's
 * cell, corner weights and gradient coefficients are formed once in ws, then an owner-gather over landmark pairs: a thread
 * owns one landmark and sums, per corner voxel of its cell and in landmark-index order, the
 * contributions of every landmark of its sample that touches that voxel; the lowest-index toucher stores the sum.  No
 * atomics, no volume-sized scratch: bit-identical from run to run on every input, collisions included.
 * Refused ("invalid argument", nothing is launched): nd outside {2, 3}, B < 1, K outside [1, 4096], an extent < 2,
 * B * nd * S >= 2^31, a spacing that is not positive and finite, a penalty outside {0, 1}, a NULL pointer other than the
 * optional ones.  ws: dfmir_landmark_ws_floats floats for either call (-1 for a refused shape), 8-byte aligned, need not be
 * zeroed or kept between the calls.  The sums
 * go through double slots added in a fixed order: every output is bit-identical from run to run.  Nothing syncs, allocates
 * or keeps state (gout is read on the device): both calls capture into a hipGraph. */
long long dfmir_landmark_ws_floats(int nd, int B, int K, int D, int H, int W);
int dfmir_landmark_fwd(int nd, const float* flow, const float* fixed_pts, const float* moving_pts, const float* weight,
                       float* ws, float* mapped, float* d, float* per_sample, float* loss, float* wsum, int B, int K, int D,
                       int H, int W, float hz, float hy, float hx, int penalty, void* stream);
int dfmir_landmark_bwd(int nd, const float* flow, const float* fixed_pts, const float* moving_pts, const float* weight,
                       const float* gout, const float* wsum, float* dflow, float* ws, int B, int K, int D, int H, int W,
                       float hz, float hy, float hx, int penalty, void* stream);
/* Thin-plate / polyharmonic spline interpolation of landmark displacements (build-defined: the reference has no landmark
 * code; the fit itself is ops.tps_fit, a float64 solve in torch).  ctrl q: [B][K][nd] fp32 voxel coordinates of the control
 * points, axis order (z,) y, x as a flow's channels, every entry finite (a padding entry is 0 with a zero coefficient);
 * scale (sz, sy, sx) = h_a / L with L = max_a h_a (S_a - 1) (sz is not read when nd == 2): basis functions are evaluated in
 * the normalised coordinates xh_a = scale_a x_a.  coef: [B][K + nd + 1][nd] float64 = [w (K rows); a_0; A (nd rows)].
 *   u_a(x) = a_0[a] + sum_c xh_c A[c][a] + sum_k w[k][a] phi(|xh - qh_k|)
 *   phi(r) = -r (nd == 3) or r^2 log r, computed as s log(s) / 2 from s = r^2 with phi(0) = 0 (nd == 2)
 * dfmir_tps_fwd: points == NULL: out[b][a][(z)][y][x] = u_a at every voxel of the volume, a flow in the warp kernels'
 * convention; points [B][M][nd] fp32 voxel coordinates: out[b][m][a] = u_a(points[b][m]) (D, H, W are not read; a non-finite
 * coordinate gives a non-finite row).  One kernel body with two position sources.  The normalised coordinates are rounded to
 * fp32 once from the double product, the squared distance and phi are fp32 (the accurate logf; the hardware square root,
 * 1 ulp), the product with the coefficient and the sum over k are float64 FMAs in index order, rounded to fp32 once at the
 * store.  A thread owns four voxels along x; the control points pass through LDS in chunks of 256.
 * dfmir_tps_bwd_coef: the adjoint with respect to coef, float64: dcoef[b][k][a] = sum_x phi(|xh - qh_k|) g[b][a][x],
 * dcoef[b][K][a] = sum_x g, dcoef[b][K + 1 + c][a] = sum_x xh_c g, g: [B][nd][(D)][H][W] fp32.  A thread owns one control
 * point; the volume is cut into slabs (a number fixed by the shape alone) whose voxels pass through LDS in tiles of 256; a
 * second launch adds the slabs' partials in slab order.  No atomics: dcoef is bit-identical from run to run.  No gradient is
 * defined with respect to the control positions.  ws: dfmir_tps_ws_bytes BYTES (-1 for a refused shape), 8-byte aligned, need
 * not be zeroed.
 * Refused ("invalid argument", nothing is launched): nd outside {2, 3}, B outside [1, 65535], K outside [1, 4096], an extent
 * < 2, B * nd * S >= 2^31 (point mode: M < 1 or B * M * nd >= 2^31), a scale that is not positive and finite, a NULL
 * pointer other than `points`.  Nothing syncs, allocates or keeps state: the calls capture into a hipGraph. */
long long dfmir_tps_ws_bytes(int nd, int B, int K, int D, int H, int W);
int dfmir_tps_fwd(int nd, const double* coef, const float* ctrl, const float* points, float* out, int B, int K, long long M,
                  int D, int H, int W, double sz, double sy, double sx, void* stream);
int dfmir_tps_bwd_coef(int nd, const float* ctrl, const float* gout, double* dcoef, void* ws, int B, int K, int D, int H,
                       int W, double sz, double sy, double sx, void* stream);
/* Keypoint detection and sparse matching (build-defined: the reference has no keypoint code).  Everything fp32, nd = 2 or 3 (D
 * is not read when nd == 2), axis order (z,) y, x, S = voxels per sample, every extent >= 2.
 * dfmir_keypoint_products: I [B][(D)][H][W] -> T [B][NP][(D)][H][W], NP = nd (nd + 1) / 2 planes in the order zz, zy, zx, yy, yx,
 *   xx (2-D: yy, yx, xx):  T_ab = g_a g_b  with  g_a(x) = (I(min(x_a + 1, S_a - 1)) - I(max(x_a - 1, 0))) / (2 h_a),  the
 *   difference, 2 h_a, the quotient and the product each rounded to fp32; spacing h = (hz, hy, hx) positive and finite (hz is
 *   not read when nd == 2).  A thread writes all planes of its voxel; the image is staged with its halo (stencil_tile.h).
 * dfmir_keypoint_response: T as above, smoothed by the caller (dfmir_gauss_smooth over B NP planes) -> R [B][(D)][H][W]:
 *   R = det(T) / trace(adj(T))  ( = 1 / trace(T^-1); 2-D: det / trace), formed in DOUBLE from the fp32 planes -- 3-D, with T =
 *   [a b c; b d e; c e f]: A00 = d f - e e, A11 = a f - c c, A22 = a d - b b, det = a A00 - b (b f - c e) + c (b e - c d), trace
 *   (adj) = (A00 + A11) + A22 -- and rounded once; 0 where the denominator is not > 0 or a plane or the quotient is not finite.
 * dfmir_keypoint_nms: out[b][x] = R[b][x] where x is selected, else 0.  Selected: R(x) > threshold, mask[b][x] != 0 (mask [B][S]
 *   or NULL) and for every other y of the (2 radius + 1)^nd window clipped to the volume R(y) < R(x), or R(y) == R(x) and y has
 *   the HIGHER linear index: the lowest index wins a plateau.  A NaN is never selected and compares as -inf as a neighbour; the
 *   mask does not remove a competitor.  radius in [1, DFMIR_KEYPOINT_NMS_MAX_RADIUS], threshold finite.  One launch: tile plus
 *   halo in LDS, a direct window walk that leaves at the first neighbour that wins.
 * dfmir_keypoint_cost: fix, mov [B][C][(D)][H][W], 1 <= C <= 16; pts [B][K][nd] voxel coordinates; cost [B][K][Dn], Dn = (2
 *   radius + 1)^nd.  q = rint(pts[b][k]) (ties to even); a row whose point has a non-finite coordinate or a q outside the volume
 *   is all NaN; otherwise, with P = (2 patch + 1)^nd,
 *     cost[b][k][j] = 1 / (C P) sum_c sum_{o in {-patch .. patch}^nd} (fix[b][c][q + o] - mov[b][c][q + o + step d_j])^2
 *   both sides reading 0 outside the volume, j enumerating d_j in {-radius .. radius}^nd in row-major order (dz,) dy, dx with
 *   -radius first (dfmir_dsearch_cost's order).  The difference is fp32, its square and the sum are float64 in ONE order for
 *   every j (oz, c, oy, ox), times 1 / (C P) in float64, rounded once: displacements whose reads all fall outside the volume tie
 *   bit for bit.  One workgroup per keypoint; the fixed patch and, plane by plane, the moving search region pass through LDS.
 *   radius in [1, DFMIR_KEYPOINT_MAX_RADIUS_3D] (nd = 3) or [1, .._2D] (nd = 2), step in [1, DFMIR_KEYPOINT_MAX_STEP], patch in
 *   [0, DFMIR_KEYPOINT_MAX_PATCH], and the staged extent E = 2 (radius step + patch) + 1 <= DFMIR_KEYPOINT_MAX_EXTENT (one plane
 *   of E^2 floats beside the largest patch in 64 KB of LDS): there is no unstaged path.
 * dfmir_keypoint_argmin: cost [rows][Dn], prior [rows][nd] in voxels or NULL (= the plain argmin, coeff is then not read):
 *     idx[row] = argmin_j ( cost[row][j] + coeff * sum_a (step d_j[a] - prior[row][a])^2 ),    disp[row][a] = step d_idx[a]
 *   the squares added in the order (z,) y, x in fp32.  Only FINITE penalised values compete (a NaN or an infinite entry is never
 *   selected); the lowest j wins a tie; a row without a finite value gives idx 0 and disp NaN.  One wave per row, the
 *   cross-lane reduction carries (value, j).  coeff finite and >= 0.
 * Refused ("invalid argument", nothing is launched): nd outside {2, 3}, B < 1, an extent < 2, C outside [1, 16], K < 1, B > 65535
 * (cost), a parameter outside its range, a spacing or threshold that is not finite (spacing: and positive), 2^31 or more
 * elements in any tensor, a NULL pointer other than mask / prior, out aliasing an input.  Nothing syncs, allocates or keeps
 * state; no atomics: every output is bit-identical from run to run. */
#define DFMIR_KEYPOINT_NMS_MAX_RADIUS 8
#define DFMIR_KEYPOINT_MAX_RADIUS_3D 8
#define DFMIR_KEYPOINT_MAX_RADIUS_2D 16
#define DFMIR_KEYPOINT_MAX_STEP 4
#define DFMIR_KEYPOINT_MAX_PATCH 3
#define DFMIR_KEYPOINT_MAX_EXTENT 96
int dfmir_keypoint_products(int nd, const float* I, float* T, int B, int D, int H, int W, float hz, float hy, float hx,
                            void* stream);
int dfmir_keypoint_response(int nd, const float* T, float* R, int B, int D, int H, int W, void* stream);
int dfmir_keypoint_nms(int nd, const float* R, const float* mask, float* out, int B, int D, int H, int W, int radius,
                       float threshold, void* stream);
int dfmir_keypoint_cost(int nd, const float* fix, const float* mov, const float* pts, float* cost, int B, int C, int K, int D,
                        int H, int W, int radius, int step, int patch, void* stream);
int dfmir_keypoint_argmin(int nd, const float* cost, const float* prior, float coeff, int* idx, float* disp, long long rows,
                          int radius, int step, void* stream);
/* NMI_Loss (util/losses.py:263-348): out[0] = -MI of the soft-binned (Parzen) joint histogram of y_true and y_pred, both
 * first clamped to [0, max_clip]; all n voxels (batch and channels included) form ONE histogram.  Per voxel
 * a_k = exp(-preterm (y_true - c_k)^2) normalised over k (b_k the same for y_pred), pab[i][j] = sum_v b[i] a[j] / V,
 * pa / pb the means of a / b, MI = sum pab log(pab / (pb pa^T + 1e-5) + 1e-5).  centers: nb device floats, 2 <= nb <= 64,
 * any spacing; preterm = 1 / (2 sigma^2) as the caller computed it.  mask (n floats, may be NULL): only voxels with
 * mask > 1e-4 count (crop_background), V = their number; V = 0 gives NaN, as the reference.  ws:
 * dfmir_nmi_ws_floats(n, nb) floats (need not be zeroed): per-workgroup partial histograms, added in index order (the
 * loss is bit-reproducible), and the gradient terms the backward reads -- keep it between the two calls.
 * bwd: d_true / d_pred (either may be NULL) = gout[0] * dL/dy, zero where the clamp or the mask cuts; no atomics. */
long long dfmir_nmi_ws_floats(long long n, int nb);
int dfmir_nmi_fwd(const float* y_true, const float* y_pred, const float* mask, const float* centers, int nb,
                  float preterm, float max_clip, long long n, float* ws, float* out, void* stream);
int dfmir_nmi_bwd(const float* y_true, const float* y_pred, const float* mask, const float* centers, int nb,
                  float preterm, float max_clip, long long n, const float* ws, const float* gout, float* d_true,
                  float* d_pred, void* stream);
/* MIND-SSC (Heinrich et al., MICCAI 2013), build-defined: a local, contrast-invariant self-similarity descriptor of a
 * single-channel image and the L2 loss of two descriptors.  I: [B][D][H][W] fp32, nd = 2 (D = 1) or 3; radius r and
 * dilation d in 1..4; every axis >= 1 (also shorter than r + d); clamp = replicate the border per axis and sample.
 * Neighbours n = 2 * axis + (0: -d, 1: +d) over the nd axes in the order (z,) y, x; channels = the pairs p < q of neighbours
 * on different axes in lexicographic order: C = 12 in 3-D ((0,2) (0,3) (0,4) (0,5) (1,2) (1,3) (1,4) (1,5) (2,4) (2,5)
 * (3,4) (3,5)), C = 4 in 2-D ((0,2) (0,3) (1,2) (1,3) of -y, +y, -x, +x).  nd = 3 with D = 1 keeps the 12 channels.
 *   s_k(y) = (I(clamp(y + p_k)) - I(clamp(y + q_k)))^2
 *   D_k(x) = (2r+1)^-nd sum_{t in [-r,r]^nd} s_k(clamp(x + t))        m_k = D_k - min_j D_j        V = mean_k m_k
 *   mu = mean of V over the whole tensor (batch included)             Vc = min(max(V, 0.001 mu), 1000 mu)
 *   M_k = exp(-m_k / Vc)     (a constant image has mu = 0 and gives NaN: no epsilon is added)
 * dfmir_mind_desc: out[B][C][D][H][W] = M.  dfmir_mind_fwd: out[0] = mean over (B, C, voxels) of (Ma - Mb)^2, or with
 * mask ([B][D][H][W] float weights) sum mask * mean_k (Ma_k - Mb_k)^2 / sum mask; an empty mask gives 0.
 * dfmir_mind_bwd: da / db (either may be NULL) = gout[0] * dL/d(a / b): mu is a constant (both clamp bounds detached),
 * min sends its gradient to the FIRST minimal channel, nothing flows through V where it is clamped; otherwise the exact
 * chain rule, in gather form.  No atomics: every sum goes through per-workgroup slots added in index order, so loss and
 * gradients are bit-identical from run to run.  Nothing syncs, allocates or keeps state; mu stays on the device.
 * ws: dfmir_mind_ws_floats(..., 0) floats, 8-byte aligned, need not be zeroed; it holds m of both images (C floats per
 * voxel and image) -- keep it between fwd and bwd.  tmp: dfmir_mind_ws_floats(..., 1) floats of backward scratch.
 * The size query returns -1 for arguments the other entry points refuse. */
long long dfmir_mind_ws_floats(int nd, int B, int D, int H, int W, int radius, int dilation, int which);
int dfmir_mind_desc(const float* I, int nd, int B, int D, int H, int W, int radius, int dilation, float* ws, float* out,
                    void* stream);
int dfmir_mind_fwd(const float* a, const float* b, const float* mask, int nd, int B, int D, int H, int W, int radius,
                   int dilation, float* ws, float* out, void* stream);
int dfmir_mind_bwd(const float* a, const float* b, const float* mask, int nd, int B, int D, int H, int W, int radius,
                   int dilation, const float* ws, float* tmp, const float* gout, float* da, float* db, void* stream);
/* Normalised-gradient-field similarity (Haber & Modersitzki, MICCAI 2006), build-defined: it rewards image edges that are
 * parallel or anti-parallel, whatever the contrast.  a, b: [B][D][H][W] fp32 single-channel images, nd = 2 (D = 1) or 3
 * (nd = 3 with D = 1 keeps three axes); axes in the order (z,) y, x of extent n_a >= 1 with spacing h_a (hz is not read for
 * nd = 2).  Per sample and axis, with replicate clamping:
 *   g_a(I)(x) = ( I(min(x_a + 1, n_a - 1)) - I(max(x_a - 1, 0)) ) / (2 h_a)      (half a one-sided difference on the border,
 *                                                                               0 on an axis of extent 1)
 *   dot = <g(A), g(B)>,   D_A = |g(A)|^2 + eps_A^2,   D_B = |g(B)|^2 + eps_B^2
 *   s(x) = dot^2 / (D_A D_B) in [0, 1);  s = 0 with no gradient where D_A D_B == 0
 *   loss = mean over (B, voxels) of (1 - s), or with mask ([B][D][H][W] float weights) sum mask (1 - s) / sum mask; an empty
 *          mask gives 0 and zero gradients.
 * eps: auto_eps == 0: the given eps_a, eps_b > 0 (eta is not read).  auto_eps != 0: eps_I = eta * mean over the whole
 * tensor (batch included) of |g(I)|_2, eta > 0 (eps_a, eps_b are not read), formed on the device in double in a fixed
 * order and A CONSTANT IN THE BACKWARD; the loss is then invariant under I -> alpha I + beta, alpha != 0; a constant image
 * has eps = 0, hence s = 0, loss 1 and a zero gradient -- no NaN.
 * dfmir_gradfield_fwd: out[0] = loss.  dfmir_gradfield_bwd: da / db (either may be NULL, not both) = gout[0] * dL/d(a / b):
 * with w(x) = mask(x) / sum mask (1 / N without a mask)
 *   G^A(x) = dL/dg(A)(x) = -2 w dot / (D_A D_B) * ( g(B) - (dot / D_A) g(A) ),   G^B the mirror expression
 *   dI(y)  = sum_a (1 / 2 h_a) ( [y_a >= 1] G_a(y - e_a) + [y_a == n_a - 1] G_a(y) - [y_a <= n_a - 2] G_a(y + e_a)
 *                                - [y_a == 0] G_a(y) )
 * the exact adjoint of the clamped difference, in gather form: no atomics, no G volume in memory, every output written once.
 * dfmir_gradfield_field: out[B][nd][D][H][W] = n(I) = g(I) / sqrt(|g(I)|^2 + eps^2) (0 where the root is 0), channels in
 * the order (z,) y, x; one eps (or eta).
 * ws: dfmir_gradfield_ws_floats() floats, 8-byte aligned, need not be zeroed: per-workgroup sums in double, added in a
 * fixed order, and at its head eps_A, eps_B and sum mask, which the main kernels and the backward read on the device --
 * keep it between fwd and bwd.  Loss, gradients and field are bit-identical from run to run; nothing syncs with the host,
 * allocates or keeps state (gout is read on the device), so the calls capture into a hipGraph.  Refused ("invalid
 * argument", nothing is launched): nd outside {2, 3}, nd = 2 with D != 1, an extent < 1, 2^31 or more voxels, a spacing,
 * eps or eta that is not positive and finite, a NULL pointer other than mask and one of da / db.  The size query returns -1
 * for a geometry the other entry points refuse. */
long long dfmir_gradfield_ws_floats(int nd, int B, int D, int H, int W);
int dfmir_gradfield_fwd(const float* a, const float* b, const float* mask, int nd, int B, int D, int H, int W, float hz,
                        float hy, float hx, int auto_eps, double eta, double eps_a, double eps_b, float* ws, float* out,
                        void* stream);
int dfmir_gradfield_bwd(const float* a, const float* b, const float* mask, const float* gout, const float* ws, float* da,
                        float* db, int nd, int B, int D, int H, int W, float hz, float hy, float hx, void* stream);
int dfmir_gradfield_field(const float* I, int nd, int B, int D, int H, int W, float hz, float hy, float hx, int auto_eps,
                          double eta, double eps, float* ws, float* out, void* stream);
/* Label-map Dice under a flow: vxm `Dice().loss(one_hot(fix)[:, labels], SpatialTransformer(one_hot(mov)[:, labels], flow))`
 * (models/voxelmorph/torchvoxelmorph/losses.py:79-90 after layers.py:36-48; mode 1 = the nearest-neighbour label warp of
 * test.py:80-81, forward only) without the one-hot tensors.  nd = 2 ([B,1,H,W], D = 1) or 3.  mov / fix: 8-bit label maps
 * [B][D][H][W]; flow: [B][nd][D][H][W] voxel displacements (align_corners=True, zero padding: a corner outside the volume
 * has weight 0); slot_of: 256 device bytes, label value -> slot 0..K-1 of the scored list (K <= 64), 255 = not scored.
 * Per (b, l): T = sum_x sum_k w_k [mov(c_k) = l][fix(x) = l], S = sum_x sum_k w_k [mov(c_k) = l], N = #{fix(x) = l};
 * dice[b][l] = 2 T / max(N + S, 1e-5) (a label in neither map scores 0 and still counts in the mean); loss[0] = -mean.
 * seeds: 2 B K floats for the backward, gT = -2 / (bottom B K) then gS = 2 T / (bottom^2 B K) (0 under the clamp).
 * ws: dfmir_warp_dice_ws_floats() floats, 8-byte aligned, need not be zeroed: per-workgroup sums as 64-bit fixed point
 * (quantum 2^-32), added by a finaliser -- no global atomics, loss / dice / seeds bit-identical from run to run.
 * bwd: dflow [B][nd][D][H][W] = gout[0] * d loss / d flow, written completely (no zero fill needed), a gather of the seed
 * table over the corners; gout is read on the device (no host sync).  The label maps get no gradient. */
long long dfmir_warp_dice_ws_floats(int nd, int B, int K, int D, int H, int W);
int dfmir_warp_dice_fwd(int nd, const unsigned char* mov, const unsigned char* fix, const float* flow,
                        const unsigned char* slot_of, int K, int B, int D, int H, int W, int mode, float* ws,
                        float* loss, float* dice, float* seeds, void* stream);
int dfmir_warp_dice_bwd(int nd, const unsigned char* mov, const unsigned char* fix, const float* flow,
                        const unsigned char* slot_of, int K, int B, int D, int H, int W, const float* seeds,
                        const float* gout, float* dflow, void* stream);
/* Exact squared Euclidean distance transform of a label map, and the Hausdorff distance of two label maps on it: the
 * reference's `HausdorffDistance` (util/loss_metrics.py:105-132; scipy's distance_transform_edt on the host there) per batch
 * element and per label.  nd = 2 ([B,1,H,W], D = 1) or 3; maps: 8-bit [B][D][H][W]; every axis <= 256, B <= 65535.
 * dfmir_label_edt_sq: out[B][D][H][W] int32 = min over voxels y with map(y) == value of |x - y|^2, DFMIR_EDT_SQ_INF where
 * the batch element holds no such voxel.  surface != 0: the set is replaced by its border voxels -- set voxels with a face
 * neighbour outside the set or outside the volume (4 neighbours in 2-D, 6 in 3-D; a volume of one plane, D == 1, counts the
 * in-plane ones only).  One launch per axis, `out` is the only scratch.
 * dfmir_label_hausdorff: labels = K <= 64 label values in HOST memory (they travel to the kernels by value: nothing is copied
 * to the device, the launches are capturable).  Direction 0 is a -> b (over the voxels of a's set, the distance to b's set),
 * direction 1 the converse; flags & DFMIR_HD_SURFACE replaces both sets by their borders.  qm = percentile in thousandths,
 * 1 .. 100000.  Per (direction, b, k), n = size of the source set:
 *   d2[dir][b][k]       the smallest d2 whose cumulative count reaches r = max(1, ceil(qm n / 100000)) (nearest rank;
 *                       qm = 100000: the maximum), int32
 *   directed[dir][b][k] sqrt(d2) (formed in double, rounded once)
 *   mean[dir][b][k]     mean of sqrt(d2) over the source set, summed in double over the histogram; mean may be NULL
 *   hd[b][k]            max of directed over the two directions
 * If either set is empty for (b, k): hd = directed = mean = +inf, d2 = DFMIR_EDT_SQ_INF (the reference's rule).
 * ws: dfmir_label_hausdorff_ws_bytes() bytes, 4-byte aligned, need not be zeroed; labels run in chunks of 4, so it does not
 * grow with K beyond that (-1: unsupported shape; nothing is launched).  Integer atomics only: bit-identical from run to run. */
#define DFMIR_EDT_SQ_INF (1 << 29)
#define DFMIR_HD_SURFACE 1
long long dfmir_label_hausdorff_ws_bytes(int nd, int B, int K, int D, int H, int W);
int dfmir_label_edt_sq(int nd, const unsigned char* map, int value, int surface, int B, int D, int H, int W, int* out,
                       void* stream);
int dfmir_label_hausdorff(int nd, const unsigned char* a, const unsigned char* b, const unsigned char* labels, int K, int B,
                          int D, int H, int W, int qm, int flags, void* ws, float* hd, float* directed, float* mean,
                          int* d2, void* stream);
/* vxm `Dice().loss(y_true, y_pred)` (models/voxelmorph/torchvoxelmorph/losses.py:79-90) of float tensors [planes = B C][S]:
 * out[0] = -mean over planes of 2 sum(t p) / max(sum(t + p), 1e-5).  ws: dfmir_dice_ws_floats(planes, S) floats (per-chunk
 * partial sums, added in index order: bit-reproducible; then the per-plane coefficients the backward reads -- keep it
 * between the two calls).  bwd: d_true / d_pred (either may be NULL) = gout[0] * dL/dy, element-wise. */
long long dfmir_dice_ws_floats(long long planes, long long S);
int dfmir_dice_fwd(const float* y_true, const float* y_pred, long long planes, long long S, float* ws, float* out,
                   void* stream);
int dfmir_dice_bwd(const float* y_true, const float* y_pred, long long planes, long long S, const float* ws,
                   const float* gout, float* d_true, float* d_pred, void* stream);
/* vxm `MSE().loss(y_true, y_pred)` (models/voxelmorph/torchvoxelmorph/losses.py:70-76): out[0] = mean((t - p)^2) over n
 * elements; ws: dfmir_mse_ws_floats(n) floats (ordered partial sums).  bwd: d_true = gout[0] 2 (t - p) / n, d_pred = -d_true
 * (either may be NULL). */
long long dfmir_mse_ws_floats(long long n);
int dfmir_mse_fwd(const float* y_true, const float* y_pred, long long n, float* ws, float* out, void* stream);
int dfmir_mse_bwd(const float* y_true, const float* y_pred, long long n, const float* gout, float* d_true, float* d_pred,
                  void* stream);
/* out = a * b element-wise: `prediction * mask` of Grad_Loss.forward (util/losses.py:120-121). */
int dfmir_mul(const float* a, const float* b, float* out, long long n, void* stream);
/* NCC_Loss (util/losses.py:183-261), mean kernel of `win` per axis (odd), zero padding:
 * out = -sqrt(mean(cross^2/(Ivar*Jvar+eps))).  tmp: 5*numel floats of scratch (box sums, kept for
 * backward). I = prediction, J = target, [B,1,D,H,W].  3-D, win 9: the W and H box passes run in one launch each way
 * (products / gradient fields formed on a haloed LDS tile); DFMIR_NCC_NO_WH_FUSE=1 = one launch per axis. */
int dfmir_ncc_fwd(const float* I, const float* J, float* tmp, float* tmp2, float* ws, float* out,
                  int B, int D, int H, int W, int win, float eps, void* stream);
int dfmir_ncc_bwd(const float* I, const float* J, const float* sums, float* tmp, float* tmp2,
                  const float* ws, const float* gout, float* dI, int B, int D, int H, int W,
                  int win, float eps, void* stream);
/* The same with a weight per voxel and the reduction chosen.  mask (numel floats, may be NULL): the masked branch of
 * NCC_Loss.forward (util/losses.py:257-261): out = -sqrt(sum(cc * mask) / sum(mask)), 0 when sum(mask) == 0.
 * mode 0 = that form; mode 1 = -sum(cc [* mask]) / n, n = numel (or sum(mask)): vxm NCC(win).loss = -mean(cc)
 * (models/voxelmorph/torchvoxelmorph/losses.py:15-67).  ws[0] = sum(cc * mask), ws[1] = sum(mask) (kept for backward).
 * mode | DFMIR_NCC_VOLUME: the tensors are VOLUMES [B,1,D,H,W] even if D == 1 -- the reference's conv3d window then still
 * counts win^3 positions (D == 1 without the flag is a 2-D image: win^2).  Pass the same mode to fwd and bwd. */
#define DFMIR_NCC_VOLUME 4
int dfmir_ncc_fwd_m(const float* I, const float* J, const float* mask, int mode, float* tmp, float* tmp2,
                    float* ws, float* out, int B, int D, int H, int W, int win, float eps, void* stream);
int dfmir_ncc_bwd_m(const float* I, const float* J, const float* mask, int mode, const float* sums,
                    float* tmp, float* tmp2, const float* ws, const float* gout, float* dI, int B, int D,
                    int H, int W, int win, float eps, void* stream);
/* NCC_Loss(kernel_type='gaussian') (util/losses.py:153-181 the window, :183-261 the loss): the argument lists of
 * dfmir_ncc_fwd_m / _bwd_m with `win` replaced by the window.  taps (HOST memory, K floats, symmetric, > 0): g(d) =
 * exp(-(d - (K-1)/2)^2 / (2 sigma^2)); K odd, 3..31; c > 0: the window is w = c * g(dy) * g(dx), NOT normalised, zero
 * padding K/2, and win_size = sum(w) = c * (sum g)^nd is formed here in double.  The reference builds the 2-D window only
 * (its conv3d call fails on a 5-D tensor); the 3-D form is build-defined: w = c * g(dz) * g(dy) * g(dx) with the same c and
 * K, which D > 1 or mode | DFMIR_NCC_VOLUME selects (a one-plane volume meets data with its centre z-tap only and keeps
 * the 3-D win_size).  The taps travel to the kernels by value: nothing is copied to the device and the launches are
 * capturable.  mask, mode, tmp (5 * numel, the window sums, kept for backward), tmp2, ws: as above; K = 9 runs the tiled
 * W+H forms of the mean window with taps, any other K one launch per axis. */
int dfmir_ncc_gauss_fwd(const float* I, const float* J, const float* mask, int mode, float* tmp, float* tmp2,
                        float* ws, float* out, int B, int D, int H, int W, const float* taps, int K, float c,
                        float eps, void* stream);
int dfmir_ncc_gauss_bwd(const float* I, const float* J, const float* mask, int mode, const float* sums,
                        float* tmp, float* tmp2, const float* ws, const float* gout, float* dI, int B, int D,
                        int H, int W, const float* taps, int K, float c, float eps, void* stream);
/* out[t] = scale * sum_l mean(rows[l][t*seg..(t+1)*seg)), rows [L][T*seg]: the per-term
 * `total_nce_loss += loss.mean() * lambda_NCE` ... `/ n_layers` of calculate_NCE_loss (registration_model.py:247-253)
 * for T terms and L layers at once (scale = lambda_NCE / n_layers); bwd fills drows from gout[T]. */
int dfmir_segment_means_fwd(const float* rows, float* out, int L, int T, long long seg, float scale, void* stream);
int dfmir_segment_means_bwd(const float* gout, float* drows, int L, int T, long long seg, float scale, void* stream);
/* out[j] = sum_i M[j*n_in+i] * *in[i]: the scalar algebra of the step's loss terms (loss_G, loss_R, loss_local,
 * loss_smooth and their sum; registration_model.py:163-166,230-234) as one launch.  in: HOST array of n_in <= 8 device
 * scalar pointers, M: HOST row-major [n_out][n_in], both copied by value.  bwd: din[i] = sum_j M[j*n_in+i] * gout[j]. */
int dfmir_scalar_combine_fwd(const float* const* in, int n_in, const float* M, int n_out, float* out, void* stream);
int dfmir_scalar_combine_bwd(const float* gout, int n_in, const float* M, int n_out, float* din, void* stream);
/* p[0..n) = 0 (p 16-byte aligned).  Replaces torch.zeros / Tensor.zero_ on the step (gradient arenas, scatter targets):
 * those issue hipMemsetAsync, which a captured step turns into hipGraph memset nodes -- not reliably ordered with the
 * kernel nodes around them on ROCm 7.2. */
int dfmir_fill_zero(float* p, long long n, void* stream);
/* out = scale * sum(x) (out zeroed by this call). */
int dfmir_sum_scaled(const float* x, float* out, long long n, float scale, void* stream);
/* dx[i] = gout[0]*scale */
int dfmir_fill_from_scalar(const float* gout, float* dx, long long n, float scale, void* stream);

/* ------------------------------------------------------------------------------------------
 * Deterministic weight gradients (build-defined, opt.deterministic_wgrad; the reference's cuDNN backward is not
 * deterministic either, models/base_model.py:37-38 sets cudnn.benchmark).  The weight- and bias-gradient kernels split
 * their reduction over workgroups and add the partial sums with fp32 atomics: every run rounds in a different order.
 * Between dfmir_det_begin and dfmir_det_end EVERY gradient entry point called by this host thread (dfmir_conv_wgrad*,
 * dfmir_conv3d_split_wgrad*, dfmir_conv3d_upwgrad, dfmir_conv3d_s2c2_wgrad, dfmir_conv7x7_c1_wgrad, dfmir_bias_grad) adds
 * 64-bit FIXED-POINT integers instead -- associative, hence bit-reproducible -- into `scratch`:
 *   scratch: dfmir_det_head_floats() + 2 * slots floats, 16-byte aligned; the call zeroes it.  The caller passes
 *     scratch + dfmir_det_head_floats() as the entry point's dw_tcc (8 bytes per element: element i of the gradient is
 *     slot i) and NULL as its db; a bias gradient is taken with dfmir_bias_grad into slots n_dw .. n_dw + n_db - 1
 *     (pointer scratch + head + 2 * n_dw).
 *   scale: two powers of two chosen on the device, one for the dW slots and one for the db slots (which only
 *     dfmir_bias_grad writes).  With frexp exponents e(f) (f < 2^e(f)): scale_dw = 2^(61 - e(count) - e(max|x|) - e(max|dy|)),
 *     scale_db = 2^(61 - e(count) - e(max|dy|)), so that the bounds count * max|x| * max|dy| of every dW sum and
 *     count * max|dy| of every db sum map below 2^61.  The exponents are added as integers: a bound beyond the fp32 range
 *     is handled like any other (the gradient itself must fit fp32), and the quantum 1 / scale_dw shrinks with max|x|, so
 *     inputs far below 1 keep a resolution of at most 2^-58 of the bound.  A zero max|x| or max|dy| (every sum is an exact
 *     zero) takes the scale 2^61; the shift is clamped to [-126, 126] (both powers stay normal floats), which only coarsens
 *     the grid for bounds below 2^-65.  x_amax / dy_amax: range probes as for the split kernels, or NULL with x / dy given
 *     (measured here).
 *   dfmir_det_end: dw_out[i] += slot[i] / scale_dw (i < n_dw), db_out[j] += slot[n_dw + j] / scale_db, and ends the mode.
 * ---------------------------------------------------------------------------------------- */
int dfmir_det_head_floats(void);
int dfmir_det_begin(float* scratch, long long slots, const float* x, long long nx, const float* x_amax, int x_amax_n,
                    const float* dy, long long ndy, const float* dy_amax, int dy_amax_n, double count, void* stream);
int dfmir_det_end(const float* scratch, float* dw_out, long long n_dw, float* db_out, long long n_db, void* stream);

/* ------------------------------------------------------------------------------------------
 * torch.optim.Adam(lr, betas) step over one flat parameter arena
 * (registration_model.py:114-117,135,168-171).  grad is pre-scaled by grad_scale (1/world under DDP).
 * ---------------------------------------------------------------------------------------- */
int dfmir_adam_step(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1,
                    float beta2, float eps, float bc1, float bc2, float grad_scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DFMIR_HIP_H */
