/*
 * poserisk_hip.h -- C ABI of libposerisk_hip.so, the MI355X (gfx950) implementation of
 * PoseRisk's per-frame hot path.
 *
 * The reference (hygenie1228/PoseRisk_RELEASE) is pure Python and has no FFI of its own:
 * its "plugin surface" is the set of Python callables main/run.py -> lib/core/base.py use
 * (SURVEY.md 8b).  Each entry point below replaces the arithmetic behind one of those
 * callables and cites it; the Python drop-in modules under poserisk_release_amd/dropin/
 * bind these symbols with ctypes (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - Every function returns 0 on success or a negative pr_status; pr_last_error() gives
 *     the message of the calling thread's last failure.  No exception crosses the boundary.
 *   - The CALLER owns every I/O buffer.  Pointers named *_dev are device (HBM) pointers
 *     (e.g. torch.Tensor.data_ptr()); pointers named *_host are host pointers.  The
 *     library never frees caller memory.  Handles own packed weights / model constants /
 *     workspaces and release them in *_destroy.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Compute calls
 *     are asynchronous on that stream and perform no host synchronisation, allocation or
 *     blocking copy, so they may be captured into a hipGraph.
 *   - One handle per device; a handle is not thread-safe; distinct handles are independent.
 *   - Layouts are row-major with the last index fastest; float = IEEE binary32.
 *
 * Memory contract
 *   No entry point reads or writes device memory outside the tensors whose extents its
 *   arguments state (and the handle's own workspaces): not a row past a ragged last tile,
 *   not the halo in front of the first frame or behind the last one, not the bytes an
 *   unaligned wide load would drag in behind the last pixel.  This is enforced by the
 *   guard-band tests (tests/test_guard_band_gpu.py), which run every stand-alone entry with
 *   its inputs between NaN guards and its outputs between canary guards.
 */
#ifndef POSERISK_HIP_H
#define POSERISK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum pr_status {
  PR_OK = 0,
  PR_ERR_INVALID = -1,   /* bad argument (shape, null pointer, unsupported size)      */
  PR_ERR_HIP = -2,       /* a HIP runtime call failed (message has the HIP error)     */
  PR_ERR_NO_DEVICE = -3, /* no gfx950 device visible                                  */
  PR_ERR_CAPACITY = -4   /* batch larger than the handle was created for              */
} pr_status;

const char* pr_last_error(void);
int pr_abi_version(void); /* bumps on any signature change */
/* "gfx950 release" for the shipped build; an ablation / experiment build names its macros (PR_TIMING_HOOKS builds compute
 * wrong results on purpose).  bench.py prints it as `library`. */
const char* pr_build_info(void);

/* Capture guard (ABI 10).  pr_hmr_create, pr_smpl_create, pr_hmr_set_streams, pr_hmr_destroy and pr_smpl_destroy allocate,
 * copy and synchronise: reached while the caller is capturing a stream into a hipGraph they would invalidate the capture (and
 * the process aborts at its next synchronisation).  They take no stream, so the caller declares the stream it enqueues on --
 * thread-local, declared != 0 sets it (NULL = the null stream), 0 clears it -- and those five entry points return
 * PR_ERR_INVALID, having touched nothing, while hipStreamIsCapturing() reports a capture on it; the handle passed to a refused
 * destroy stays valid.  The stand-alone test entries (which allocate and take a stream) check their own stream argument.  The
 * Python binding declares torch's current stream before each of those calls (poserisk_release_amd/_lib.py::declare_stream).
 * No reference counterpart: the reference never captures (lib/core/base.py:81-84 builds its models once, eagerly). */
int pr_declare_stream(void* stream, int declared);

/* The internal fence (ABI 16; test entries).  With POSERISK_FENCE=1 (head) or 2 (tail) in the environment when a handle is
 * created (pr_hmr_create, pr_smpl_create, pr_hmr_set_streams; a stand-alone test entry reads it per call) every device
 * allocation of the library's own -- activations, Winograd work, split-K slab and tickets, packed weights, regressor and SMPL
 * workspaces, the stand-alone entries' copies -- lies between two guards of at least 64 KiB and one frame, all 0xFF bytes
 * before use; in tail mode a tensor inside a buffer that is sized as a maximum ends on the buffer's last byte instead of
 * starting on its first.  Unset or 0: plain hipMalloc, nothing recorded.
 * pr_fence_check synchronises the device(s), reads every live fenced allocation's guards back and returns how many guard
 * regions no longer hold 0xFF everywhere, those found when a fenced allocation was freed since the last call included (kept
 * until reported once); per region one line in `report` (NUL-terminated, cut at a line when `capacity` is too small): the
 * allocation's name and size, the side, the first and last touched byte relative to the payload, the number of bytes changed.
 * 0 and an empty report when nothing is fenced.  Refused (PR_ERR_INVALID) under a declared stream capture.
 * pr_fence_list: one line "name <tab> payload bytes <tab> guard bytes" per live fenced allocation; returns their number.
 * pr_fence_payload_fill: how many bytes at the start and at the end of the named live allocation's payload (at most 256 MiB)
 * still hold 0xFF, i.e. were never written: where in a buffer that is sized as a maximum the tensors really lay (head mode:
 * the end stays untouched, tail mode: the start).  PR_ERR_INVALID for an unknown name.
 * pr_fence_selftest: a small allocation of its own, fenced whatever the switch says, one byte set directly in front of its
 * payload and one directly behind it (hipMemset, inside the allocation); 0 when the report names exactly those two bytes. */
int pr_fence_check(char* report, size_t capacity);
int pr_fence_list(char* report, size_t capacity);
int pr_fence_payload_fill(const char* name, size_t* leading, size_t* trailing);
int pr_fence_selftest(void);

/* The fp32 encoder's stem as ONE kernel (csrc/stem_pool_f32.hip; same arithmetic as above in fp32, weights in registers,
 * pooling in registers): x_dev f32 [B,112,112,12] (the 2x2 space-to-depth image), w_host f32[64,12,4,4] OIHW, bias_host f32[64]
 * -> y_dev f32 [B,56,56,64].  w_host must be a 7x7 kernel laid into the 4x4 taps' 8x8 window with a zero row and a zero
 * column in front -- W2[o][(2 di + dj) 3 + c][th][tw] = W[o][c][2 th + di - 1][2 tw + dj - 1], zero outside 0..6, as
 * pr_hmr_create builds it from conv1.weight -- the kernel packs the half-empty taps together; anything else is refused
 * (PR_ERR_INVALID).  Exported for parity tests and timing (allocates, synchronises). */
int pr_stem_pool_f32_nhwc(int device, const float* x_dev, const float* w_host, const float* bias_host, float* y_dev, int B,
                          int repeats, float* ms_out, void* stream);

/* ------------------------------------------------------------------------------------ */
/* a1-a3  HMR: ResNet-50 encoder + iterative regressor + rot6d->rotmat                   */
/* replaces: models.hmr(...) / spin_model(batch)   lib/core/base.py:81-84, :220          */
/* ------------------------------------------------------------------------------------ */
typedef struct pr_hmr pr_hmr_t;

/* Number of floats in the canonical weight blob (order below). */
size_t pr_hmr_weight_floats(void);

/*
 * weights_host: the SPIN state dict flattened in this order (all float32, PyTorch layouts):
 *   conv1.weight[64,3,7,7], bn1.{weight,bias,running_mean,running_var}[64];
 *   for L in 1..4, for i in block(L):  conv1.weight, bn1.*4, conv2.weight, bn2.*4,
 *       conv3.weight, bn3.*4, and for i==0: downsample.0.weight, downsample.1.*4;
 *   fc1.weight[1024,2205], fc1.bias, fc2.weight[1024,1024], fc2.bias,
 *   decpose.weight[144,1024], decpose.bias, decshape.weight[10,1024], decshape.bias,
 *   deccam.weight[3,1024], deccam.bias, init_pose[144], init_shape[10], init_cam[3].
 * BatchNorm (eval, eps 1e-5) is folded into the conv weights in double precision at
 * create time.  max_batch sizes the activation workspace (frames per forward call).
 * precision: 0 = fp32 MFMA (v_mfma_f32_32x32x2_f32; products and sums are exact-fp32 fmaf chains),
 * 1 = bf16 MFMA encoder with fp32 accumulate (regressor stays fp32).
 * conv_form (fp32 encoder only; a property of the handle, so one process may hold several): how the ten 3x3 /
 * stride-1 layers with >= 128 channels are computed on that kernel (and, where layer2's form is an F(4x4,3x3) one, layer1.0's
 * 64-channel conv2 on the one-launch kernel of csrc/conv_wino64.hip with the same points; POSERISK_WINO_LAYER1=0 / 2 at create
 * time: none / all three of layer1's) -- PR_CONV_FORM_DIRECT (implicit GEMM, the
 * reference's arithmetic up to summation order), PR_CONV_FORM_WINOGRAD_2X2 / _4X4 (F(2x2,3x3) / F(4x4,3x3) on Lavin &
 * Gray's points 0, +-1, +-2: 2.25x / 4x fewer multiplies, a different rounding pattern), PR_CONV_FORM_WINOGRAD_4X4_B
 * (F(4x4,3x3) on the points 0, +-11/16, +-3/2: the same cost as _4X4 with half its per-layer rounding error, every
 * transform constant exact in fp32), PR_CONV_FORM_DEFAULT (= PR_CONV_FORM_BUILTIN_DEFAULT; the environment
 * variable POSERISK_WINOGRAD moves this default only).  A three-digit value selects the form per ResNet stage, layer2 /
 * layer3 / layer4 (e.g. 244 = F(2x2) in layer2, F(4x4) in layer3 and layer4).  The built-in default is 5, chosen on error
 * DISTRIBUTIONS over 768 frames of trained-like stress weights, all joints, against an fp64 run of the network
 * (profiles/r04_wino_stats.txt; rms of the 6-D pose / 99th percentile of the rotation matrices / relative rms of the pooled
 * features, as multiples of the direct form's): form 5 1.02 / 1.05 / 1.03, form 4 1.19 / 1.20 / 1.19, form 244 (round 3's
 * default) 1.04 / 1.04 / 1.04, F(2x2) 0.99 / 1.00 / 0.99 -- at 4.29 / 4.31 / 4.45 / 4.53 ms of conv per 64 frames (direct:
 * 4.90).  The MAXIMUM over those 166 k samples (direct 4.8e-4, the fp32 oracle itself 1.1e-3) is set by the ~13 % of joints
 * whose 6-D vector is nearly degenerate under that random decoder and does not rank the forms.
 */
enum { PR_CONV_FORM_DEFAULT = -1, PR_CONV_FORM_DIRECT = 0, PR_CONV_FORM_WINOGRAD_2X2 = 2, PR_CONV_FORM_WINOGRAD_4X4 = 4,
       PR_CONV_FORM_WINOGRAD_4X4_B = 5, PR_CONV_FORM_BUILTIN_DEFAULT = 5 };
int pr_hmr_create(int device, const float* weights_host, size_t n_floats, int max_batch,
                  int precision, int conv_form, pr_hmr_t** out);
int pr_hmr_destroy(pr_hmr_t* h);

/* x_dev f32[B,3,224,224] NCHW in [0,1] (no mean/std normalisation: _img_utils.py:259-266)
 * -> rotmat_dev f32[B,24,3,3], betas_dev f32[B,10], cam_dev f32[B,3].
 * Any of the three outputs may be NULL.  xf_dev (optional, may be NULL) receives the
 * pooled encoder features f32[B,2048]; pose6d_dev (optional) the 6-D pose f32[B,144]. */
int pr_hmr_forward(pr_hmr_t* h, const float* x_dev, int B, float* rotmat_dev, float* betas_dev,
                   float* cam_dev, float* xf_dev, float* pose6d_dev, void* stream);

/* The encoder cuts a batch into n_streams contiguous sub-batches that run concurrently on internal
 * HIP streams (forked from / joined to the caller's stream with events; still asynchronous, still no
 * host synchronisation in pr_hmr_forward).  Frames are independent, so results are bit-identical for any
 * n_streams (1..8).  Default 1 (or the environment variable POSERISK_HMR_STREAMS at create time): on
 * MI355X at B=64 the lock-step sub-batches measured slower than one stream; overlapping WHOLE batches on
 * caller-side streams (one handle per stream) is what fills the tails.  This call reallocates workspaces
 * and synchronises the device: configuration time only. */
int pr_hmr_set_streams(pr_hmr_t* h, int n_streams);

/* A hint, not a mode: n_in_flight = how many handles' forward calls overlap on this device (one per caller-side stream /
 * pipeline lane).  The persistent kernels size their grids by it -- conv1x1_regw_f32 runs two workgroups per CU when a
 * batch has the GPU to itself and ONE when other batches' kernels should find room beside it (measured, B=64 fp32: one
 * batch in flight +2.0 % with two, three in flight +1.8 % with one; profiles/r04_experiments.txt section 5).  Results do not
 * depend on it (the assignment of work units to workgroups changes, no sum's order does).  Default 1. */
int pr_hmr_set_concurrency(pr_hmr_t* h, int n_in_flight);

/* Per-kernel timing of the conv launches (for bench.py's roofline): when enabled, every
 * conv launch of the NEXT forward calls is bracketed by hipEvents on `stream`.
 * pr_hmr_profile_read synchronises those events and returns, per conv layer (53 entries,
 * execution order), the accumulated milliseconds and the launch count since enable (a Winograd layer's three
 * kernels are one bracket; a convolution fused into another's launch -- a downsample branch in its conv3, a layer1
 * conv2 + conv3 pair -- reports zero launches and its work under the launch that carries it), the ALGORITHMIC FLOP per
 * frame (direct convolution) and, optionally, the FLOP the matrix pipes execute (K padding included,
 * (m+2)^2 products per Winograd tile).  While enabled the
 * encoder runs serially on the caller's stream (one sub-batch at a time) so each bracket is one kernel. */
int pr_hmr_profile_enable(pr_hmr_t* h, int on);
int pr_hmr_profile_read(pr_hmr_t* h, float* ms_per_layer_host, int* launches_per_layer_host,
                        double* flops_per_layer_per_frame_host, double* mfma_flops_per_layer_per_frame_host,
                        int n_layers);
int pr_hmr_num_conv_layers(void);
/* What one forward of B frames launches for the encoder's 53 convolutions: conv_launches = event brackets of the
 * profile above (a Winograd layer counts once), winograd_layers = how many of them are Winograd layers, each of which
 * is three kernels (transform, grouped GEMMs, transform).  Kernel launches between the layout change and the global
 * average pool = conv_launches + 2 * winograd_layers: scripts/pmc_summary.py refuses to summarise counter passes whose
 * dispatch count differs (round 4's summary silently missed a new kernel).  No reference counterpart (measurement). */
int pr_hmr_plan_counts(pr_hmr_t* h, int B, int* conv_launches, int* winograd_layers);
/* Encoder tap (ABI 11; a test entry): the encoder of pr_hmr_forward -- the same sub-batch split, streams, concurrency hint and
 * kernel routing -- stopped after `block` and that block's output copied to act_dev, NHWC with the real channels in the
 * handle's precision (fp32, or bf16 bits): block 0 = the stem + max-pool [B,56,56,64], 1..16 = the outputs of the 16
 * Bottlenecks ([B,56,56,256] x3, [B,28,28,512] x4, [B,14,14,1024] x6, [B,7,7,2048] x3).  Asynchronous on `stream`;
 * refused (PR_ERR_INVALID) while `stream` is being captured, and when B is outside 1..max_batch or block outside 0..16.
 * tests/test_encoder_blocks.py checks every block of the production plan against an fp64 reference from this tap.
 * No reference counterpart (testing). */
int pr_hmr_encode_until(pr_hmr_t* h, const float* x_dev, int B, int block, void* act_dev, void* stream);
/* Regressor tap (ABI 13; a test entry): the regressor of pr_hmr_forward -- the same launches on the same workspaces with the
 * handle's GEMM kernel and tile shape -- run on the caller's pooled features xf_dev f32[B,2048], stopped after launch `step` and
 * what that launch wrote copied to out_dev: step 0 = the initial state [B,192] (pose6d 144 | betas 10 | cam 3 | zero pad),
 * 1 = h_static = fc1's feature columns + bias [B,1024]; for iteration i = 0..2: 2 + 3 i = h1 = fc1's state columns +
 * h_static [B,1024], 3 + 3 i = h2 = fc2 [B,1024], 4 + 3 i = the state after decpose | decshape | deccam were added in place
 * [B,192].  Asynchronous on `stream`; refused (PR_ERR_INVALID) while `stream` is being captured, and when B is outside
 * 1..max_batch or step outside 0..10.  tests/test_regressor_steps.py checks every launch against an fp64 reference of it
 * computed from the tap before.  No reference counterpart (testing). */
int pr_hmr_regress_until(pr_hmr_t* h, const float* xf_dev, int B, int step, float* out_dev, void* stream);
/* The conv form this handle really runs (what PR_CONV_FORM_DEFAULT resolved to at create time: the built-in default,
 * or POSERISK_WINOGRAD's value): 0, 2, 4, 5 or three digits.  scripts/validate_checkpoint.py bases its exit status on it. */
int pr_hmr_conv_form(pr_hmr_t* h);

/* Stand-alone conv + folded-BN bias + optional residual + optional ReLU on NHWC tensors:
 * the building block of the encoder, exported for per-shape parity tests and tuning.
 *   x_dev f32[B,H,W,Cin] (Cin % 4 == 0), w_host f32[Cout,Cin_real,KH,KW] (PyTorch OIHW;
 *   Cin_real <= Cin, extra input channels are treated as zero), bias_host f32[Cout] or NULL,
 *   res_dev f32[B,Ho,Wo,Cout] or NULL, y_dev f32[B,Ho,Wo,Cout].  Cout % 64 == 0.
 * tile_cfg -1 selects the built-in heuristic, >= 6 a tile configuration index (pr_conv_num_tile_cfgs(); 0..5 and 18 are
 * reserved: the first-generation kernel and the 256x256 bf16 tile they selected were retired, they return PR_ERR_INVALID and
 * the message says "retired"),
 * -2 / -4 the Winograd F(2x2,3x3) / F(4x4,3x3) form (the encoder runs its 3x3 / stride-1 layers with >= 128
 * channels as F(4x4,3x3); fp32, pad 1, no residual, Cin % 32 == 0: input transform, 16 / 36 grouped GEMMs in one
 * launch, output transform), 100 the row-panel form of a short-K 1x1 convolution, 300 (bf16, 1x1, Cin 128 -> Cout 512, with bias
 * and residual) the persistent kernel that keeps the weights in registers (csrc/expand_res_bf16.hip), 301 / 302 (bf16, 1x1 or
 * 3x3, Cin % 64 == 0, Cout % 128 == 0, no residual) the persistent kernel that deals the pixels evenly to one workgroup per
 * CU (csrc/conv_bal_bf16.hip; 302 forces channel blocks of 128), 200 + S (S = 2..8) the 64x64 tile with
 * every tile's K-steps dealt to S workgroups (split-K, fp32).  precision 1: x_dev, res_dev and y_dev hold bfloat16 (Cin % 8 == 0), the
 * weights are rounded to bfloat16, accumulation and bias stay fp32; only the LDS-DMA tile configs apply.
 * This call packs the weights on every invocation (it allocates and synchronises): test/tuning use only. */
int pr_conv_num_tile_cfgs(void);
int pr_conv2d_nhwc(int device, const void* x_dev, const float* w_host, const float* bias_host,
                   const void* res_dev, void* y_dev, int B, int H, int W, int Cin, int Cin_real,
                   int Cout, int KH, int KW, int stride, int pad, int relu, int tile_cfg,
                   int precision, int repeats, float* ms_out, void* stream);

/* The fused form of a first Bottleneck's tail, relu(bn3(conv3(t)) + bn_d(conv_d(x))) (SPIN models/hmr.py Bottleneck
 * with a downsample branch), as ONE GEMM whose K loop runs over t's channels and then over x's: exported for parity
 * tests (allocates, synchronises).  x1_dev [B,Ho,Wo,Cin1], w1_host f32[Cout,Cin1], x2_dev [B,H2,W2,Cin2] sampled at
 * (ho*stride2, wo*stride2), w2_host f32[Cout,Cin2], bias_host f32[Cout] or NULL -> y_dev [B,Ho,Wo,Cout].  precision as
 * pr_conv2d_nhwc (1: tensors hold bfloat16).  Channel counts are multiples of 32 (fp32) / 64 (bf16). */
int pr_conv1x1_dual_nhwc(int device, const void* x1_dev, const float* w1_host, const void* x2_dev,
                         const float* w2_host, const float* bias_host, void* y_dev, int B, int Ho, int Wo,
                         int Cin1, int H2, int W2, int Cin2, int stride2, int Cout, int relu, int tile_cfg,
                         int precision, void* stream);

/* A layer1 Bottleneck's conv2 + conv3 as one kernel (the 64-channel map between them stays in LDS): exported for
 * parity tests (allocates, synchronises).  x_dev [B,H,W,Cin] (Cin a power of two >= 32; bf16: >= 64), w2_host
 * f32[64,Cin,3,3] OIHW, b2_host f32[64], w3_host f32[N3,64], b3_host f32[N3], res_dev [B,H,W,N3] or NULL
 * -> y_dev [B,H,W,N3] = act(relu(conv3x3(x, w2) + b2) * w3^T + b3 + res), act = ReLU if relu3.  precision as
 * pr_conv2d_nhwc (1: the three tensors hold bfloat16, the map between the convolutions is rounded to bfloat16). */
int pr_conv3x3_conv1x1_nhwc(int device, const void* x_dev, const float* w2_host, const float* b2_host,
                            const float* w3_host, const float* b3_host, const void* res_dev, void* y_dev,
                            int B, int H, int W, int Cin, int N3, int relu3, int precision, void* stream);

/* A layer1 Bottleneck's conv2 as Winograd F(4x4,3x3) in ONE launch (ABI 14; csrc/conv_wino64.hip: input transform, 36 small
 * GEMMs and output transform inside a workgroup), alone or with conv3 behind it as pr_conv3x3_conv1x1_nhwc: exported for
 * parity tests (allocates, synchronises).  fp32 only.  x_dev [B,H,W,Cin], w2_host f32[Cout,Cin,3,3] OIHW, b2_host f32[Cout];
 * Cin and Cout must both be 64, anything else is refused by name with PR_ERR_INVALID.  Any H, W >= 1: tiles that overhang the
 * map are computed and dropped.  form: 4 (Lavin & Gray's points 0, +-1, +-2) or 5 (0, +-11/16, +-3/2).
 *   w3_host == NULL: y_dev [B,H,W,64] = act(conv3x3(x, w2) + b2), act = ReLU if relu2 (b3_host, res_dev, N3, relu3 unused);
 *   else w3_host f32[N3,64], b3_host f32[N3], res_dev [B,H,W,N3] or NULL:
 *        y_dev [B,H,W,N3] = act(relu(conv3x3(x, w2) + b2) * w3^T + b3 + res), act = ReLU if relu3 (N3 % 64 == 0). */
int pr_conv3x3_wino64_nhwc(int device, const void* x_dev, const float* w2_host, const float* b2_host,
                           const float* w3_host, const float* b3_host, const void* res_dev, void* y_dev, int B, int H,
                           int W, int Cin, int Cout, int N3, int relu2, int relu3, int form, void* stream);

/* A whole layer1 Bottleneck (SPIN models/hmr.py Bottleneck.forward: conv1 1x1 -> conv2 3x3 64->64 -> conv3 1x1 64->256,
 * BatchNorm folded by the caller, + identity, ReLU) as ONE persistent bf16 kernel (csrc/bottleneck_bf16.hip): exported for
 * parity tests and timing (allocates, synchronises).  y_dev bf16 [B,H,W,256] (W <= 63), w2_host f32[64,64,3,3] OIHW,
 * w3_host f32[256,64], biases f32.
 *   wd_host == NULL: a block without a downsample branch -- x_dev bf16 [B,H,W,256], w1_host f32[64,256], identity = x;
 *   wd_host != NULL: the stage's first block -- x_dev bf16 [B,H,W,64], w1_host f32[64,64], identity = the downsample
 *   branch wd_host f32[256,64] (+ bd_host f32[256]) of x, summed into conv3's K loop.
 * repeats > 0 and ms_out != NULL: the mean time of `repeats` further launches in milliseconds. */
int pr_bottleneck_nhwc(int device, const void* x_dev, const float* w1_host, const float* b1_host, const float* w2_host,
                       const float* b2_host, const float* w3_host, const float* b3_host, const float* wd_host,
                       const float* bd_host, void* y_dev, int B, int H, int W, int repeats, float* ms_out, void* stream);

/* A whole layer2 Bottleneck (plain block, 512 -> 128 -> 128 -> 512 channels, W <= 31; SPIN models/hmr.py Bottleneck.forward) as
 * ONE persistent bf16 kernel (csrc/bottleneck128_bf16.hip): exported for parity tests and timing (allocates, synchronises).
 * x_dev, y_dev bf16 [B,H,W,512]; w1_host f32[128,512], w2_host f32[128,128,3,3] OIHW, w3_host f32[512,128], biases f32
 * (BatchNorm folded by the caller); identity = x.  repeats / ms_out as pr_bottleneck_nhwc. */
int pr_bottleneck128_nhwc(int device, const void* x_dev, const float* w1_host, const float* b1_host, const float* w2_host,
                          const float* b2_host, const float* w3_host, const float* b3_host, void* y_dev, int B, int H, int W,
                          int repeats, float* ms_out, void* stream);

/* A whole layer3 Bottleneck (plain block, 1024 -> 256 -> 256 -> 1024 channels, H W <= 224; SPIN models/hmr.py Bottleneck.forward)
 * as ONE bf16 kernel, one frame per workgroup (csrc/bottleneck256_bf16.hip): exported for parity tests and timing (allocates,
 * synchronises).  x_dev, y_dev bf16 [B,H,W,1024]; w1_host f32[256,1024], w2_host f32[256,256,3,3] OIHW, w3_host f32[1024,256],
 * biases f32 (BatchNorm folded by the caller); identity = x.  repeats / ms_out as pr_bottleneck_nhwc. */
int pr_bottleneck256_nhwc(int device, const void* x_dev, const float* w1_host, const float* b1_host, const float* w2_host,
                          const float* b2_host, const float* w3_host, const float* b3_host, void* y_dev, int B, int H, int W,
                          int repeats, float* ms_out, void* stream);

/* The bf16 encoder's stem as ONE kernel (csrc/stem_pool_bf16.hip): the 7x7 / stride-2 conv1 in its 4x4 / stride-1 form on
 * the 2x2 space-to-depth image (window rows y-2 .. y+1) + bias (folded bn1) + ReLU + MaxPool2d(3, 2, 1)  (SPIN models/hmr.py
 * conv1 / bn1 / relu / maxpool): exported for parity tests and timing (allocates, synchronises).
 * x_dev bf16 [B,H,H,16] (H even, <= 112), w_host f32[64,16,4,4] OIHW, bias_host f32[64] -> y_dev bf16 [B,H/2,H/2,64]. */
int pr_stem_pool_nhwc(int device, const void* x_dev, const float* w_host, const float* bias_host, void* y_dev, int B, int H,
                      int repeats, float* ms_out, void* stream);

/* ------------------------------------------------------------------------------------ */
/* f-1  crop front-end                                                  */
/* replaces: CropDataset.__getitem__ data/demo_dataset.py:58-74 ->                       */
/*           get_single_image_crop_demo lib/utils/_img_utils.py:219-252 (affine :53-101, */
/*           cv2.warpAffine INTER_LINEAR / BORDER_CONSTANT) -> ToTensor :259-266          */
/* ------------------------------------------------------------------------------------ */
/* frames_dev uint8[F,H,W,3] decoded video frames (bgr != 0: channel order of cv2.imread, swapped to RGB
 * like demo_dataset.py:59), bboxes_dev f32[N,4] (cx,cy,w,h) one per crop, frame_idx_dev int32[N] or NULL
 * (crop n comes from frame n), scale = cfg.DATASET.bbox_scale (1.2) -> crops_dev f32[N,3,224,224] in [0,1].
 * OpenCV's fixed-point bilinear warp is reproduced (integer weights, round-half-even), so crops are bit-exact
 * against the restated algorithm (oracle/crop_ref.py): every double operation of the affine arithmetic -- control points,
 * forward and inverse matrix, adelta / bdelta, the per-row X0 / Y0 -- is rounded on its own, never contracted into a fused
 * multiply-add.  `scale` is read as the shortest decimal that rounds to the float given (1.2f means the reference's double 1.2).
 * status_dev[n] (int32[N], may be NULL) is 0 for a crop that was cut, else a set of bits; a crop with a bit set is
 * zero-filled, with or without a status pointer:
 *   bit 0 (1)  the frame index lies outside [0, F): never an out-of-range read (the reference would raise from cv2.imread
 *              on the missing file)
 *   bit 1 (2)  the box has no defined crop.  With the float32 control values the reference forms, sx0 = cx, sy0 = cy,
 *              sx2 = f32(cx + f32(w scale / 2)), sy1 = f32(cy + f32(h scale / 2)): one of them is not finite (a NaN or
 *              infinite field), or exceeds 2^18 in magnitude, or sx2 == sx0 or sy1 == sy0 (w or h zero, or so small that
 *              the half-extent is lost in the centre's rounding: the forward matrix would divide by zero).
 * Inside that domain every fixed-point integer of the warp fits in int32, so the int64 arithmetic here is OpenCV's
 * saturate_cast<int> arithmetic; a negative w or h is inside it and gives the mirrored crop. */
int pr_crop_frames(const uint8_t* frames_dev, int F, int H, int W, int bgr, const int32_t* frame_idx_dev,
                   const float* bboxes_dev, int N, float scale, float* crops_dev, int32_t* status_dev,
                   void* stream);

/* ------------------------------------------------------------------------------------ */
/* a3-a5  rotation conversions                                                           */
/* ------------------------------------------------------------------------------------ */
/* SPIN utils/geometry.py rot6d_to_rotmat: pose6d_dev f32[N,144] -> rotmat_dev f32[N,24,3,3] */
int pr_rot6d_to_rotmat(const float* pose6d_dev, int N, float* rotmat_dev, void* stream);

/* replaces: rot_to_angle + axis_angle_to_euler_angle   lib/utils/coord_utils.py:24-30, 83-95
 * rotmat_dev f32[N,24,3,3] -> axis_angle_dev f32[N,24,3] (OpenCV Rodrigues semantics,
 * double arithmetic, float32 result) and euler_deg_dev f64[N,24,3] (x,y,z degrees).
 * status_dev int32[N] (may be NULL): bit0 = isRotationMatrix failed (coord_utils.py:70),
 * bit1 = Euler round-trip check failed (coord_utils.py:90-91); the reference aborts there.
 * Bit 0 is set by a non-finite axis-angle component (NaN or +-inf: theta, so the rebuilt matrix, is NaN), never by finite
 * input: the matrix tested is rebuilt from the axis-angle, and its float32 norm stays under 2.4e-7 against the threshold
 * of 1e-6.  Through this entry the axis-angle is always finite (a matrix entry that is NaN or >= 100 in magnitude gives
 * the zero vector, OpenCV's checkRange), so status is 0 here; pr_axis_angle_to_euler reads the caller's vector and can
 * set it.  Bit 1 has no reachable input (the round trip reproduces a matrix that came out of Rodrigues' formula to
 * float32 rounding, 1e-5 against 0.1); it is kept for parity with the reference's dead assert. */
int pr_pose_to_euler(const float* rotmat_dev, int N, float* axis_angle_dev, double* euler_deg_dev,
                     int32_t* status_dev, void* stream);
/* replaces: axis_angle_to_euler_angle called on its own   lib/utils/coord_utils.py:83-95
 * axis_angle_dev f32[N,24,3] (read only) -> euler_deg_dev f64[N,24,3]; status bits as above. */
int pr_axis_angle_to_euler(const float* axis_angle_dev, int N, double* euler_deg_dev, int32_t* status_dev,
                           void* stream);

/* ------------------------------------------------------------------------------------ */
/* a6-a11  SMPL: Rodrigues, shape blend, joint regression, pose blend, chain, skinning   */
/* replaces: SMPL_Layer.forward  lib/smplpytorch/smplpytorch/pytorch/smpl_layer.py:65-158 */
/* ------------------------------------------------------------------------------------ */
typedef struct pr_smpl pr_smpl_t;

/* Host arrays as SMPL_Layer registers them (smpl_layer.py:40-63):
 *   v_template f32[V,3], shapedirs f32[V,3,NB], posedirs f32[V,3,(J-1)*9],
 *   J_regressor f32[J,V] (dense), weights f32[V,J], parents int32[J] (parents[0] < 0),
 *   model_betas f32[NB] or NULL (the pkl's own betas, used when the caller's betas are
 *   all zero: smpl_layer.py:87-91).  J must be 24, NB <= 16. */
int pr_smpl_create(int device, const float* v_template_host, const float* shapedirs_host,
                   const float* posedirs_host, const float* J_regressor_host,
                   const float* weights_host, const int32_t* parents_host,
                   const float* model_betas_host, int V, int J, int NB, int max_batch,
                   pr_smpl_t** out);
int pr_smpl_destroy(pr_smpl_t* h);

/* pose_dev f32[B,72] axis-angle, betas_dev f32[B,NB] or NULL, trans_dev f32[B,3] or NULL
 * -> verts_dev f32[B,V,3] (may be NULL: joints only), joints_dev f32[B,J,3]; metres.
 * center_idx < 0 = no centring (smpl_layer.py:148-152). */
int pr_smpl_forward(pr_smpl_t* h, const float* pose_dev, const float* betas_dev,
                    const float* trans_dev, int B, int center_idx, float* verts_dev,
                    float* joints_dev, void* stream);

/* replaces: get_joint_cam   lib/utils/coord_utils.py:7-21
 * axis_angle_dev f32[N,24,3] is MUTATED: every root row becomes (3.14, 0, 0) as in the
 * reference; joint_cam_dev f32[N,24,3] = joints(mm) - root joint, zero betas.
 * verts_dev (optional) f32[N,V,3] receives the mesh the reference computes and drops. */
int pr_smpl_joint_cam(pr_smpl_t* h, float* axis_angle_dev, int N, float* joint_cam_dev,
                      float* verts_dev, void* stream);

/* ------------------------------------------------------------------------------------ */
/* a12-a13  REBA / RULA                                                                  */
/* replaces: REBA.__call__ lib/utils/reba.py:50-81, RULA.__call__ lib/utils/rula.py:66-98 */
/* ------------------------------------------------------------------------------------ */
typedef struct pr_reba_info { /* add_info["REBA"], example/additional_information.json:2-11 */
  int32_t legs_bilateral;     /* "Legs_bilateral_weight_bearing/walking" */
  int32_t sitting;            /* "Sitting" */
  int32_t load_force;         /* "Load/Force Score" */
  int32_t arm_supported_l;    /* "Arm_supported_leaning_L" */
  int32_t arm_supported_r;    /* "Arm_supported_leaning_R" */
  int32_t coupling;           /* "Coupling" */
  int32_t activity;           /* "Activity_Score" */
} pr_reba_info;

typedef struct pr_rula_info { /* add_info["RULA"], example/additional_information.json:13-24 */
  int32_t arm_supported_l, arm_supported_r;
  int32_t a_muscle_l, a_muscle_r;
  int32_t a_load_l, a_load_r;
  int32_t legs_bilateral;
  int32_t b_muscle, b_load;
} pr_rula_info;

/* euler_deg_dev f64[N,24,3] -> out_dev int32[N,10]:
 *   score, trunk, neck, leg, upper_arm L,R, lower_arm L,R, wrist L,R  (reba.py:71-75 log_score) */
int pr_reba(const double* euler_deg_dev, int N, const pr_reba_info* info, int32_t* out_dev,
            void* stream);
/* -> out_dev int32[N,12]:
 *   score, upper_arm L,R, lower_arm L,R, wrist L,R, wrist_twist L,R, neck, trunk, leg */
int pr_rula(const double* euler_deg_dev, int N, const pr_rula_info* info, int32_t* out_dev,
            void* stream);

/* ------------------------------------------------------------------------------------ */
/* a15  the per-batch driver: crops -> everything the reference's loop produces          */
/* replaces: Predictor.get_pose_estimation_results lib/core/base.py:211-240 + :151,168   */
/* ------------------------------------------------------------------------------------ */
typedef struct pr_frames_out { /* all device pointers; any may be NULL except where noted */
  float* rotmat;        /* f32[B,24,3,3] (required) */
  float* betas;         /* f32[B,10] */
  float* cam;           /* f32[B,3]  */
  float* axis_angle;    /* f32[B,24,3] (required)  root rows overwritten with 3.14,0,0 (Q5) */
  double* euler_deg;    /* f64[B,24,3] (required) */
  float* joint_cam;     /* f32[B,24,3] (required) */
  float* verts;         /* f32[B,V,3]  optional mesh */
  int32_t* reba;        /* int32[B,10] */
  int32_t* rula;        /* int32[B,12] */
  int32_t* status;      /* int32[B]    */
} pr_frames_out;

int pr_frames_forward(pr_hmr_t* hmr, pr_smpl_t* smpl, const float* x_dev, int B,
                      const pr_reba_info* reba_info, const pr_rula_info* rula_info,
                      const pr_frames_out* out, void* stream);

/* ------------------------------------------------------------------------------------ */
/* r1  mesh overlay (ABI 12): the fitted mesh of every crop drawn over its video frame   */
/* extends: the --debug_frame reporting lib/core/base.py:273-327 (one frame's OBJ and    */
/*          skeleton plot, root forced to (3.14, 0, 0), zero betas, no image)            */
/* ------------------------------------------------------------------------------------ */
/* Raster contract.  Integer-exact, so that tests/raster_ref.py (numpy) reproduces face_id bit for bit.
 *
 * Projection.  Crop n has vertices (X, Y, Z) in metres in SPIN's camera axes (x right, y down, z away from the camera),
 *   cam[n] = (s, tx, ty), its box (cx, cy, w, h) and `scale` (cfg.DATASET.bbox_scale).  Image point, pixel centres at
 *   integer coordinates:
 *     x = cx + s (X + tx) w scale / 2,   y = cy + s (Y + ty) h scale / 2,   depth = Z.
 *   This is SPIN's crop pixel u = 112 (1 + s (X + tx)) taken back through the inverse of the crop's affine
 *   (_img_utils.py:53-86, rot = 0; the affine pr_crop_frames applies).  It is weak perspective, which is what the camera
 *   parameters are; against SPIN's f = 5000 perspective the difference is about |Z| / 50 m of the offset from the box centre.
 * Fixed point.  xf = rint(16 x), yf = rint(16 y), zf = rint(4096 Z) + 2^20, int32, rounding half to even.  A vertex is
 *   invalid if a coordinate is non-finite, if x or y lies 4096 px or more outside the frame (x <= -4096 or x >= W - 1 + 4096,
 *   likewise y), or if |Z| >= 256 m; faces that touch an invalid vertex are skipped.  H, W <= 4096.  These bounds keep every
 *   product below inside int64.
 * Coverage.  A = orient2d(a, b, c) = (b - a) x (c - a) in int64; A = 0: the face is skipped; A < 0: b and c are swapped (no
 *   back-face culling: the result depends neither on winding nor on the mesh being closed).  Pixel (row i, col j) samples
 *   p = (16 j, 16 i): w0 = orient2d(b, c, p), w1 = orient2d(c, a, p), w2 = orient2d(a, b, p).  Covered when every wk >= 0,
 *   where a tie (wk == 0) counts only if that weight's edge P->Q (w0: b->c, w1: c->a, w2: a->b, after the swap) has dy > 0,
 *   or dy == 0 and dx < 0: no sample of a split-quad grid is covered twice or missed.
 * Visibility.  depth = (w0 zf_a + w1 zf_b + w2 zf_c) / A in int64 (every term non-negative: truncation = floor);
 *   key = (uint64)depth << 32 | face index; the smallest key wins (depth ties go to the lower face index); empty = ~0.
 * Shading.  Flat per face: n = normalised (v_b - v_a) x (v_c - v_a) of the float 3-D vertices in the face's own order,
 *   I = 0.35 + 0.65 |n_z| (two-sided, light along the view axis), c = part_rgb[n, face_part[f]] I, kept in quarter steps;
 *   out = rint((1 - alpha) frame + alpha c) clamped to [0, 255].  A pixel with no visible face is copied unchanged.
 *   frames and out share one channel order; part_rgb is RGB and is swapped when bgr != 0.
 *
 * Arguments (device pointers):
 *   verts f32[N,V,3], faces int32[F,3], cam f32[N,3], bboxes f32[N,4] (cx, cy, w, h), scale;
 *   frames u8[n_frames,H,W,3], bgr, frame_idx int32[N] or NULL (crop n over frame n);
 *   face_part int32[F] (values outside [0, P) are clamped), part_rgb u8[N,P,3], P, alpha in [0, 1];
 *   out u8[N,H,W,3]; face_id int32[N,H,W] or NULL (the visible face, -1 where none); vert_fx int32[N,V,4] or NULL (xf, yf,
 *   zf, valid; all zero when invalid); status int32[N] or NULL:
 *     bit 0  frame index outside [0, n_frames): that crop's out is zero-filled (as pr_crop_frames does), face_id -1
 *     bit 1  an invalid vertex
 *     bit 2  a face index outside [0, V) (that face is skipped)
 * workspace: device memory of at least pr_render_workspace_bytes(N, V, F, H, W) bytes (z-buffer, projected vertices, face
 * colours, big-face queue), owned by the caller.  Argument errors return PR_ERR_INVALID before any device work; N = 0 returns
 * PR_OK.  Asynchronous on `stream`, no allocation, no synchronisation.  Launches: r4's five kernels, as the case of one mesh
 * per canvas (canvas n = crop n over frame frame_idx[n], no depth step); face_id stays the face's own index f. */
typedef struct pr_render_args {
  const float* verts;
  const int32_t* faces;
  const float* cam;
  const float* bboxes;
  const uint8_t* frames;
  const int32_t* frame_idx;
  const int32_t* face_part;
  const uint8_t* part_rgb;
  uint8_t* out;
  int32_t* face_id;
  int32_t* vert_fx;
  int32_t* status;
  int N, V, F, P;
  int n_frames, H, W, bgr;
  float scale, alpha;
} pr_render_args;

size_t pr_render_workspace_bytes(int N, int V, int F, int H, int W);
int pr_render_overlay(const pr_render_args* args, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------ */
/* r2  annotated score video (ABI 15): frame + track box + score panel, one call a batch */
/* replaces: the per-frame OpenCV loop of lib/core/base.py:284-327 (cv2.resize INTER_AREA, */
/*           cv2.putText) and visualize_box lib/utils/vis_utils.py:278-294 (cv2.line)     */
/* ------------------------------------------------------------------------------------ */
/* Compose contract.  Integer-exact, so that tests/video_ref.py (numpy) reproduces every byte.
 *
 * Canvas.  out u8[N, dst_h, dst_w + panel_w, 3].  The host passes dst_w, dst_h and panel_w (the reference: 720,
 *   int(H * 720 / W) and 280, base.py:287-290).  Columns [0, dst_w) of canvas n are the image region: source frame src_idx[n]
 *   (canvas n shows frame n when src_idx is NULL) of frames u8[n_frames,H,W,3] with the box drawn on it, resampled.  Columns
 *   [dst_w, dst_w + panel_w) are the panel: black with the text lines.  A frame index outside [0, n_frames) zero-fills the
 *   image region and sets status bit 0 (as pr_crop_frames and pr_render_overlay do); the panel is drawn all the same.  frames
 *   may be the plain video or what pr_render_overlay wrote.  frames and out share one channel order; the box and line colours
 *   are three bytes for channels 0, 1, 2 of that order.  1 <= H, W, dst_w, dst_h <= 4096, 0 <= panel_w <= 4096.
 * Box, on the source BEFORE resampling (vis_utils.py:278-294 draws on the full-size frame, base.py:326 resizes afterwards).
 *   box int32[N,4] = (x_min, y_min, x_max, y_max), the corners the reference's integer arithmetic gives; x_max < x_min (or a
 *   NULL box) means no box.  Source pixel (x, y) takes box_rgb when it lies within Chebyshev distance 1 of the rectangle's
 *   outline: inside [x_min-1, x_max+1] x [y_min-1, y_max+1] and not inside [x_min+2, x_max-2] x [y_min+2, y_max-2]; clipped to
 *   the frame.  By a reading of OpenCV's thick-line code this differs from the reference's four cv2.line(..., thickness 2)
 *   calls in at most the four outer corner pixels; that is UNVERIFIED (OpenCV was not available to compare against).
 * Area resample, any ratio up or down.  On axis x, source cell k covers [k dst_w, (k+1) dst_w) and destination cell i covers
 *   [i W, (i+1) W) in units of 1 / (W dst_w); ox[i][k] is the integer length of their overlap.  Axis y likewise with H and
 *   dst_h.  S = sum_j sum_k oy[r][j] ox[i][k] src[j][k][c] is an exact integer, at most 255 H W <= 255 * 2^24 < 2^32: the
 *   accumulator is uint32 and never wraps (the column sums sum_j oy src <= 255 H < 2^20 are uint32 too).  out = S / (H W)
 *   rounded half to even.  This is the mathematical box filter that cv2.resize(..., INTER_AREA) (base.py:326) approximates
 *   in float; OpenCV's bits are not reproduced.
 * Panel text.  L <= 16 lines per canvas.  lines int32[N,L,5] = (x0, yb, size class s, length, colour c0 | c1 << 8 | c2 << 16):
 *   an origin (x0, baseline yb) in canvas coordinates as cv2.putText takes it (base.py:296-323).  text u8[N,L,C] holds the
 *   codes (1 <= C <= 4096; length is clamped to C).  x0 and yb may be any int32, as may the box corners: a line or a box
 *   edge too far away to reach the canvas or the frame simply draws nothing there.  atlas u8[S,96,CH,CW] is a monospace coverage atlas for codes 32..127 with per-class
 *   advance adv[s] (1 <= adv[s] <= CW) and ascent[s]; it is the caller's data.  For panel pixel (y, x) and line l:
 *     k = floor((x - x0) / adv), counted when 0 <= k < length;  u = (x - x0) - k adv;  v = y - (yb - ascent);
 *     cov = atlas[s][code - 32][v][u] when 0 <= v < CH, else the line leaves the pixel alone;
 *     out_c = (2 (bg_c (255 - cov) + col_c cov) + 255) div 510       (bg: black, then what earlier lines left)
 *   Lines apply in index order, later over earlier.  Codes outside 32..127, lengths <= 0 and size classes outside [0, S) draw
 *   nothing.  Text is clipped to the panel: the image region always shows the image (base.py:326 pastes it over the canvas).
 *
 * status int32[N] or NULL: bit 0 as above, else 0.  Argument errors return PR_ERR_INVALID before any device work; N = 0
 * returns PR_OK.  Asynchronous on `stream`, one launch, no workspace, no allocation, no synchronisation (capturable).  A
 * canvas depends on no other canvas of the batch. */
#define PR_VIDEO_MAX_LINES 16
#define PR_VIDEO_MAX_CLASSES 4
#define PR_VIDEO_LINE_INTS 5
typedef struct pr_compose_args {
  const uint8_t* frames;    /* u8[n_frames,H,W,3] */
  const int32_t* src_idx;   /* int32[N] or NULL */
  const int32_t* box;       /* int32[N,4] or NULL */
  const int32_t* lines;     /* int32[N,L,5]  (may be NULL when L = 0, like text and atlas) */
  const uint8_t* text;      /* u8[N,L,C] */
  const uint8_t* atlas;     /* u8[S,96,CH,CW] */
  uint8_t* out;             /* u8[N,dst_h,dst_w+panel_w,3] */
  int32_t* status;          /* int32[N] or NULL */
  int N, n_frames, H, W;
  int dst_h, dst_w, panel_w;
  int L, C, S, CH, CW;
  int adv[PR_VIDEO_MAX_CLASSES], ascent[PR_VIDEO_MAX_CLASSES];
  uint8_t box_rgb[4];       /* channels 0, 1, 2; [3] unused */
} pr_compose_args;

int pr_compose_video(const pr_compose_args* args, void* stream);

/* ------------------------------------------------------------------------------------ */
/* r3  people video: frame + every tracked person's box and tag + people panel, one call  */
/*     a batch.  No counterpart in the reference, which draws one person; no ABI bump:    */
/*     a function was added, no signature changed                                         */
/* ------------------------------------------------------------------------------------ */
/* People contract.  Integer-exact, so that tests/video_people_ref.py (numpy) reproduces every byte.
 *
 * Canvas, area resample, src_idx, status bit 0 and the limits on H, W, dst_w, dst_h, panel_w, C, S, CH, CW, adv and ascent:
 *   r2's, word for word.
 * Boxes, on the source BEFORE resampling.  box int32[N,K,4] = (x_min, y_min, x_max, y_max) and box_rgb u8[N,K,4] (channels 0,
 *   1, 2 of the frames' order; [3] unused), 1 <= K <= PR_PEOPLE_MAX_BOXES.  Slot k of canvas n paints r2's outline (Chebyshev
 *   distance 1 of the rectangle, clipped to the frame) in its own colour.  Slots are painted in index order, later over
 *   earlier.  x_max < x_min means no box in that slot; a NULL box means no box in any slot (box_rgb may then be NULL too).
 *   Corners may be any int32.
 * Lines.  lines int32[N,L,5], text u8[N,L,C] and the atlas as in r2, 0 <= L <= PR_PEOPLE_MAX_LINES.  L_img (0 <= L_img <= L)
 *   splits them in two groups:
 *     [0, L_img)  tags.  The origin is in canvas coordinates.  A tag is drawn AFTER resampling over the image region, columns
 *                 [0, dst_w): r2's coverage blend with bg_c = the resampled image byte (0 where the frame index is outside
 *                 the range), then what earlier tags left.  A tag never touches the panel.
 *     [L_img, L)  panel lines: r2's rule, r2's clipping to the panel, bg black.  A panel line never touches the image.
 *   Lines apply in index order within each group; the two groups do not meet.
 * Reduction.  With K = 1, L_img = 0 and box_rgb[n][0] equal to r2's box_rgb for every n, every output byte and status word
 *   equals pr_compose_video's on the same remaining arguments.
 *
 * status, argument errors (PR_ERR_INVALID before any device work, `out` untouched), N = 0, asynchrony: r2's.  One launch, no
 * workspace, no allocation, no synchronisation (capturable).  A canvas depends on no other canvas of the batch. */
#define PR_PEOPLE_MAX_BOXES 16
#define PR_PEOPLE_MAX_LINES 32
typedef struct pr_compose_people_args {
  const uint8_t* frames;    /* u8[n_frames,H,W,3] */
  const int32_t* src_idx;   /* int32[N] or NULL */
  const int32_t* box;       /* int32[N,K,4] or NULL */
  const uint8_t* box_rgb;   /* u8[N,K,4] */
  const int32_t* lines;     /* int32[N,L,5]  (may be NULL when L = 0, like text and atlas) */
  const uint8_t* text;      /* u8[N,L,C] */
  const uint8_t* atlas;     /* u8[S,96,CH,CW] */
  uint8_t* out;             /* u8[N,dst_h,dst_w+panel_w,3] */
  int32_t* status;          /* int32[N] or NULL */
  int N, n_frames, H, W;
  int dst_h, dst_w, panel_w;
  int K, L, L_img, C, S, CH, CW;
  int adv[PR_VIDEO_MAX_CLASSES], ascent[PR_VIDEO_MAX_CLASSES];
} pr_compose_people_args;

int pr_compose_people(const pr_compose_people_args* args, void* stream);

/* ------------------------------------------------------------------------------------ */
/* r4  people mesh overlay: the fitted meshes of every tracked person of a frame drawn   */
/*     over it, depth-tested against each other, one call a batch.  No counterpart in    */
/*     the reference, which draws one person; no ABI bump: functions and a struct were   */
/*     added, no signature changed                                                        */
/* ------------------------------------------------------------------------------------ */
/* People raster contract.  Integer-exact, so that tests/raster_people_ref.py (numpy, on tests/raster_ref.py) reproduces
 * face_id bit for bit.  Projection, fixed point, coverage, shading and blend: r1's, word for word, per mesh.  What differs:
 *
 * Canvases.  N meshes, M canvases.  canvas int32[N] names the canvas mesh n is drawn on, src_idx int32[M] the source frame of
 *   canvas m (NULL: canvas m over frame m, M <= n_frames).  A canvas may hold any number of meshes; one that holds none is a
 *   copy of its frame.
 * Depth between meshes.  zf = rint(4096 Z) + 2^20 + z_step[n], z_step int32[N] (NULL: all zero), 0 <= z_step <= 2^24
 *   (PR_RENDER_Z_STEP_MAX = 4096 m), added AFTER the rounding.  The weights of a covered sample sum to A, so shifting all three
 *   zf of a face by an integer k shifts (w0 zf_a + w1 zf_b + w2 zf_c) / A = floor(.) by exactly k.  Hence: the same extra shift
 *   on every mesh of a canvas leaves that canvas byte for byte what it was, and a canvas with one mesh is pr_render_overlay's
 *   image whatever that mesh's z_step.  (A float offset added before rint would have neither property: ties break half to
 *   even.)  Bound: |xf|, |yf| < 2^17, so A and every wk are below 2^37; zf < 2^20 + 2^20 + 2^24 < 2^25; the depth numerator
 *   is at most A max(zf) < 2^62, inside int64, and depth < 2^25 fits the key's upper half.
 * Visibility.  One key buffer u64[M,H,W].  key = (uint64)depth << 32 | (n F + f), N F < 2^31; the smallest key wins: equal
 *   depths go to the lower mesh index, then to the lower face.  The bytes of a canvas depend only on its own meshes and their
 *   relative order, not on what else is in the batch.
 *
 * Arguments (device pointers): verts, faces, cam, bboxes, scale, frames, bgr, face_part, part_rgb u8[N,P,3], P, alpha as in
 *   r1, and canvas, src_idx, z_step as above.
 *   out u8[M,H,W,3]; face_id int32[M,H,W] or NULL (n F + f of the visible face, -1 where none); vert_fx int32[N,V,4] or NULL
 *   (zf includes z_step); status int32[N] or NULL:
 *     bit 0  the mesh's canvas has a source index outside [0, n_frames) (nothing of it is drawn)
 *     bit 1  an invalid vertex                        bit 2  a face index outside [0, V) (that face is skipped)
 *     bit 3  canvas[n] outside [0, M)                 bit 4  z_step[n] outside [0, 2^24]
 *   A mesh with bit 3 or bit 4 set draws nothing: its vert_fx rows are all zero and its bits 0-2 stay clear.
 *   canvas_status int32[M] or NULL: bit 0  src_idx[m] outside [0, n_frames): that canvas is zero-filled, its face_id -1 (as r1).
 * workspace: device memory of at least pr_render_people_workspace_bytes(N, M, V, F, H, W) bytes (the key buffer, sized by M;
 *   projected vertices, face colours and the big-face queue, sized by N), owned by the caller.  Argument errors return
 *   PR_ERR_INVALID before any device work.  M = 0 returns PR_OK; N = 0 with M > 0 is valid and copies the frames (the mesh
 *   pointers, V, F and P are then not looked at).  Asynchronous on `stream`, no allocation, no synchronisation.  Launches:
 *   clear, vertex, face, big face, resolve (N = 0: clear and resolve).  These are the only raster kernels: r1's entry runs
 *   them too.  canvas is required whenever N > 0 (a null canvas is an argument error, not r1's identity). */
#define PR_RENDER_Z_STEP_MAX (1 << 24)
typedef struct pr_render_people_args {
  const float* verts;        /* f32[N,V,3] */
  const int32_t* faces;      /* int32[F,3] */
  const float* cam;          /* f32[N,3] */
  const float* bboxes;       /* f32[N,4] */
  const uint8_t* frames;     /* u8[n_frames,H,W,3] */
  const int32_t* canvas;     /* int32[N] */
  const int32_t* src_idx;    /* int32[M] or NULL */
  const int32_t* z_step;     /* int32[N] or NULL */
  const int32_t* face_part;  /* int32[F] */
  const uint8_t* part_rgb;   /* u8[N,P,3] */
  uint8_t* out;              /* u8[M,H,W,3] */
  int32_t* face_id;          /* int32[M,H,W] or NULL */
  int32_t* vert_fx;          /* int32[N,V,4] or NULL */
  int32_t* status;           /* int32[N] or NULL */
  int32_t* canvas_status;    /* int32[M] or NULL */
  int N, M, V, F, P;
  int n_frames, H, W, bgr;
  float scale, alpha;
} pr_render_people_args;

size_t pr_render_people_workspace_bytes(int N, int M, int V, int F, int H, int W);
int pr_render_people(const pr_render_people_args* args, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------ */
/* j1  baseline JPEG frames -> u8[F,H,W,3] on the device, bit-exact with libjpeg         */
/* replaces: cv2.imread in CropDataset.__getitem__ data/demo_dataset.py:58-59 on the      */
/*           <output>/tmp/%09d.jpg files the front end writes (lib/core/base.py:47-56)    */
/* ------------------------------------------------------------------------------------ */
/* The host half (pr_jpeg_parse, csrc/jpeg_host.cc, no device) reads markers and fills descriptors; the device half
 * (pr_jpeg_decode, csrc/jpeg.hip) does everything else: nothing is decoded on the host.  No ABI bump: functions were added,
 * no signature changed.
 *
 * Accepted: 8-bit baseline (SOF0), Huffman coded, one component or three with luma sampling 1x1, 2x1 or 2x2 and chroma 1x1,
 *   ONE interleaved scan, with or without a restart interval, 16 <= width, height <= 4096, 8-bit quantisation tables, Huffman
 *   table ids 0 and 1.  APPn and COM segments are skipped: the EXIF orientation tag is IGNORED (as cv2.imread with
 *   IMREAD_IGNORE_ORIENTATION and Pillow's Image.open do; plain cv2.imread would rotate), and an Adobe APP14 colour transform
 *   flag is not looked at (three components are YCbCr).  Everything else is refused per frame with one of the codes below,
 *   never guessed at.  A single-component frame's sampling factors mean nothing (one block per MCU) and are stored as 1x1.
 *
 * Arithmetic contract.  Integer-exact, so that tests/jpeg_ref.py (numpy) and libjpeg's default decode path (jpeg_idct_islow,
 *   fancy upsampling, the 16-bit fixed-point YCbCr conversion: what cv2.imread and Pillow run) agree with it byte for byte on
 *   valid streams.  All shifts are arithmetic; DESCALE(x, n) = (x + (1 << (n-1))) >> n.
 * Entropy decoding.  Baseline Huffman decoding, receive-and-extend, DC prediction reset to 0 at the start of every restart
 *   segment, zig-zag order mapped to natural order; coefficients are kept as int16.
 * IDCT.  jpeg_idct_islow of jpeg-6b (CONST_BITS 13, PASS1_BITS 2) on the dequantised block d = coefficient * quantiser
 *   (natural order): pass 1 down the columns with DESCALE(., 11), pass 2 along the rows with DESCALE(., 18).  One 1-D pass on
 *   i0..i7:
 *     z1=(i2+i6)*4433; t2=z1-i6*15137; t3=z1+i2*6270
 *     t0=(i0+i4)<<13;  t1=(i0-i4)<<13
 *     t10=t0+t3; t13=t0-t3; t11=t1+t2; t12=t1-t2
 *     a0=i7; a1=i5; a2=i3; a3=i1
 *     z1=a0+a3; z2=a1+a2; z3=a0+a2; z4=a1+a3; z5=(z3+z4)*9633
 *     a0*=2446; a1*=16819; a2*=25172; a3*=12299
 *     z1*=-7373; z2*=-20995; z3=z3*-16069+z5; z4=z4*-3196+z5
 *     a0+=z1+z3; a1+=z2+z4; a2+=z2+z3; a3+=z1+z4
 *     out0..7 = t10+a3, t11+a2, t12+a1, t13+a0, t13-a0, t12-a1, t11-a2, t10-a3      (each DESCALEd)
 *   sample = x = (out + 128) & 1023, then 0..255 -> x, 256..511 -> 255, 512..1023 -> 0 (libjpeg's range-limit table, its wrap
 *   included).  libjpeg's shortcuts for all-zero AC terms give the same values and do not exist here.
 *   32-bit evaluation.  libjpeg computes in `long`; the kernel computes in 32-bit two's-complement (unsigned arithmetic, one
 *   arithmetic shift at the end).  A pass is +, -, * by constants and <<: ring operations, so the 32-bit value of an output
 *   before DESCALE equals the 64-bit one whenever the latter fits int32, whatever the intermediates did.  Each output is
 *   sum_k c_k i_k with sum_k |c_k| <= 61214 (the largest row of the pass as a matrix; 8192 + 11363 + 10703 + 9633 + 8192 +
 *   6437 + 4433 + 2260 = 61213 for out0, 61214 for out2 and out5), so with every input of a pass at most
 *   PR_JPEG_IDCT_BOUND = 35079 in magnitude, |out| + 2^17 <= 61214 * 35079 + 131072 = 2 147 457 978 < 2^31: exact.  The kernel
 *   checks exactly that -- every dequantised coefficient AND every pass-1 result within +-35079 -- and sets
 *   PR_JPEG_ST_IDCT_RANGE for a frame with a block outside; such a block is computed the same way (wrapped), not differently.
 *   In terms of the dequantised coefficients alone: all |d| <= 1173 suffices (then every pass-1 result is at most
 *   (61214 * 1173 + 1024) >> 11 = 35061).  An 8-bit image's DCT has |d| <= 1024 plus half a quantiser step, and pass 1 is
 *   the column transform scaled by 4: valid streams are far inside the bound.  The golden streams, saturating noise at
 *   quality 100 among them, reach |d| = 680 and |pass-1 result| = 3619.
 * Upsampling (libjpeg's "fancy" upsampling).  A component's own size is dw = ceil(W h / hmax), dh = ceil(H v / vmax); the
 *   block padding beyond it is never read.  s = the component's samples, r = source row, i = source column:
 *     1x1   copy.
 *     h2v1  out[2i] = (3 s[i] + s[i-1] + 1) >> 2, out[2i+1] = (3 s[i] + s[i+1] + 2) >> 2, except out[0] = s[0] and
 *           out[2dw-1] = s[dw-1].
 *     h2v2  vertical: c[i] = 3 s[r][i] + s[r'][i] with r' = r-1 for the even output row 2r and r+1 for the odd one, clamped
 *           to 0..dh-1 (libjpeg's duplicated context rows at the image's top and bottom, not at block boundaries);
 *           horizontal: out[2i] = (3 c[i] + c[i-1] + 8) >> 4, out[2i+1] = (3 c[i] + c[i+1] + 7) >> 4, with
 *           out[0] = (4 c[0] + 8) >> 4 and out[2dw-1] = (4 c[dw-1] + 7) >> 4.
 *   The result is cropped to H x W.
 * Colour.  With cb and cr minus 128: R = y + ((91881 cr + 32768) >> 16), G = y + ((-22554 cb + 32768 - 46802 cr) >> 16),
 *   B = y + ((116130 cb + 32768) >> 16), each clamped to 0..255.  One component gives gray in all three channels.  out is
 *   RGB, or BGR (cv2.imread's order) when bgr != 0: the layout pr_crop_frames, pr_render_overlay and pr_compose_video take.
 *
 * Memory safety (on ANY bytes, valid or not).  Every byte the device reads from `data` lies inside its segment's
 *   [begin, end), itself checked against data_bytes; past the end (or at a marker) the bit reader yields zero bits and, once
 *   such a bit is consumed, sets PR_JPEG_ST_TRUNCATED; a run that would push a coefficient index past 63 ends the block with
 *   PR_JPEG_ST_BAD_RUN; a code no table holds ends the segment with PR_JPEG_ST_BAD_CODE; a DC value that
 *   leaves int16 (no 8-bit image has one beyond +-2048) is stored truncated with PR_JPEG_ST_COEF_RANGE; blocks never written stay zero;
 *   every descriptor field that forms an address (frame and table-set indices, sizes, sampling, selectors) is checked on the
 *   device and a frame whose descriptor fails gets PR_JPEG_ST_REFUSED and zero pixels.  A frame's workspace and pixels are its
 *   own: a bad frame never touches another frame's.  Parity with libjpeg on corrupt streams is NOT promised, only bounds and
 *   a non-zero status. */
#define PR_JPEG_IDCT_BOUND 35079
#define PR_JPEG_LOOK_BITS 9
enum { /* bits of pr_jpeg_decode's status[f] */
  PR_JPEG_ST_REFUSED = 1, PR_JPEG_ST_TRUNCATED = 2, PR_JPEG_ST_BAD_RUN = 4, PR_JPEG_ST_BAD_CODE = 8, PR_JPEG_ST_IDCT_RANGE = 16,
  PR_JPEG_ST_COEF_RANGE = 32
};
enum { /* pr_jpeg_parse's parse_status[f]; pr_jpeg_refusal_name gives the words */
  PR_JPEG_OK = 0, PR_JPEG_E_NOT_JPEG = 1, PR_JPEG_E_TRUNCATED = 2, PR_JPEG_E_PROGRESSIVE = 3, PR_JPEG_E_EXTENDED = 4,
  PR_JPEG_E_ARITHMETIC = 5, PR_JPEG_E_PRECISION = 6, PR_JPEG_E_COMPONENTS = 7, PR_JPEG_E_SAMPLING = 8, PR_JPEG_E_SCANS = 9,
  PR_JPEG_E_QUANT16 = 10, PR_JPEG_E_DIMENSIONS = 11, PR_JPEG_E_SIZE_DIFFERS = 12, PR_JPEG_E_TABLE = 13, PR_JPEG_E_MARKER = 14,
  PR_JPEG_E_RESTARTS = 15, PR_JPEG_E_COUNT = 16
};
typedef struct pr_jpeg_hufftab { /* one Huffman table as the device decodes it */
  uint16_t look[1 << PR_JPEG_LOOK_BITS]; /* next 9 bits -> length << 8 | symbol for codes of <= 9 bits, else 0 */
  int32_t maxcode[17];                   /* [l], l = 1..16: the largest code of length l, -1 when there is none */
  int32_t valoff[17];                    /* [l]: index into vals of length l's first code, minus that code */
  uint8_t vals[256];                     /* symbols in code order */
  int32_t defined;
} pr_jpeg_hufftab;
typedef struct pr_jpeg_huff { /* the tables in force at a frame's SOS: DC 0, DC 1, AC 0, AC 1 */
  pr_jpeg_hufftab tab[4];
} pr_jpeg_huff;
typedef struct pr_jpeg_frame {
  int32_t width, height;
  int32_t ncomp;                     /* 1 or 3; 0 = refused by the parser (the device zero-fills the frame) */
  int32_t hs, vs;                    /* luma sampling: 1x1, 2x1 or 2x2 (chroma is 1x1) */
  int32_t restart_interval;          /* MCUs per restart segment, 0 = none */
  int32_t first_segment, n_segments; /* this frame's run of the segment array */
  int32_t huff_set;                  /* index into the pr_jpeg_huff array (identical sets of a call are stored once) */
  int32_t dc_sel[3], ac_sel[3];      /* per component: 0 or 1 */
  uint16_t quant[3][64];             /* per component, natural order */
} pr_jpeg_frame;
typedef struct pr_jpeg_segment { /* one entropy-coded segment = one unit of device parallelism */
  int64_t begin, end;            /* byte range in `data`; end is where the marker behind it starts */
  int32_t frame, first_mcu;
} pr_jpeg_segment;

/* data_host: the files of the call back to back; file f is bytes [offsets_host[f], offsets_host[f+1]) (int64[F+1], ascending,
 * offsets_host[0] >= 0).  H, W: the size every frame must have, or 0, 0 to adopt the first accepted frame's.  Fills
 * frames_host[F], parse_status_host[F] (PR_JPEG_OK or a refusal; a refused frame has ncomp = 0), up to segment_capacity
 * segments and huff_capacity table sets, and counts_host[4] = segments used, table sets used, H, W.  Returns PR_OK also when
 * frames were refused (the last refusal is named in pr_last_error with its frame index), PR_ERR_CAPACITY when a capacity
 * was too small (counts_host then holds what is needed; nothing else is valid), PR_ERR_INVALID for a null pointer, F < 0 or
 * offsets out of order, before anything is dereferenced.  F = 0 is legal.  Segment ranges are absolute offsets in data_host
 * and always lie inside their file.  Never reads outside [offsets_host[0], offsets_host[F]). */
int pr_jpeg_parse(const uint8_t* data_host, const int64_t* offsets_host, int F, int H, int W, pr_jpeg_frame* frames_host,
                  pr_jpeg_segment* segments_host, int segment_capacity, pr_jpeg_huff* huff_host, int huff_capacity,
                  int32_t* parse_status_host, int32_t* counts_host);
const char* pr_jpeg_refusal_name(int code);

/* Device memory pr_jpeg_decode needs for F frames of H x W: int16 coefficients and u8 component planes at block-padded size. */
size_t pr_jpeg_workspace_bytes(int F, int H, int W);

/* All device pointers: data u8[data_bytes] (what pr_jpeg_parse read, uploaded), frames / segments / huff its descriptors
 * uploaded unchanged, out u8[F,H,W,3] (4-byte aligned for dword stores; any other address is written byte by byte), status
 * int32[F] (required; bits PR_JPEG_ST_*).  The workspace must be 16-byte aligned.  Three kernels (entropy decode: one lane per segment; dequantise + IDCT: one lane per block;
 * upsample + colour: one lane per four pixels) behind one asynchronous clear of the coefficients and the status words.
 * Argument errors (null pointers, sizes outside 16..4096, a workspace below pr_jpeg_workspace_bytes or misaligned, negative
 * counts, segments without data or tables) return
 * PR_ERR_INVALID by name before any device work; F = 0 returns PR_OK.  Asynchronous on `stream`, no allocation, no blocking
 * copy, no synchronisation (capturable). */
typedef struct pr_jpeg_args {
  const uint8_t* data;
  const pr_jpeg_frame* frames;
  const pr_jpeg_segment* segments;
  const pr_jpeg_huff* huff;
  uint8_t* out;
  int32_t* status;
  int64_t data_bytes;
  int F, H, W;
  int n_segments, n_huff;
  int bgr;
} pr_jpeg_args;
int pr_jpeg_decode(const pr_jpeg_args* args, void* workspace, size_t workspace_bytes, void* stream);

/* The same decode with the entropy stage run in parallel INSIDE a restart segment (csrc/jpeg_sync.hip):
 * what a frame without restart markers -- cv2.imwrite's, ffmpeg's, a camera's -- needs, being one serial chain on one lane for
 * pr_jpeg_decode.  Every segment is cut into sub-sequences of subseq_bytes raw bytes (cuts at begin + i * subseq_bytes; a
 * segment shorter than that is one), one lane each.  A decoder's state is (position of the next unread bit, never inside a
 * stuffed 00; block slot within the MCU; next zig-zag index) or DEAD (after a code no table holds or a symbol that reaches
 * behind the data's end; in the result it propagates to the segment's later sub-sequences, during the rounds a sub-sequence
 * behind a DEAD one decodes from its own guess, so that those behind it can still synchronise; a run past 63 ends the block
 * with PR_JPEG_ST_BAD_RUN as for pr_jpeg_decode).  A cold pass decodes every
 * sub-sequence from (its first bit, 0, 0), skipping a first byte that is the 00 of an FF 00 pair, to the first symbol boundary
 * at or behind its end and keeps the exit state, the blocks begun and completed and the DC differences' sum per component; up
 * to max_rounds rounds (one launch each, states ping-ponged) decode it again from the previous sub-sequence's exit of the
 * round before where that changed.  A frame is converged at the first round in which no exit changed -- by induction from a
 * segment's first sub-sequence every entry state is then the serial decoder's -- and later rounds skip it; round 1 counts
 * every sub-sequence from a segment's third on as changed (its entry was a guess's exit), so a frame with more than two
 * sub-sequences in a segment converges at round 2 at the earliest.  Prefix sums per segment then give every sub-sequence its
 * first block's ordinal and DC predictions, and a write pass decodes once more and scatters the coefficients to the addresses
 * pr_jpeg_decode uses, up to the segment's block count (bytes behind the last MCU are not looked at, as there).  A frame not
 * converged after max_rounds is decoded by pr_jpeg_decode's kernel instead, on the device (fell_back = 1): correctness never
 * depends on synchronisation having happened.  The IDCT and colour stages are pr_jpeg_decode's.
 *
 * Contract.  The memory-safety paragraph above holds unchanged on any bytes (the state arrays live in the workspace and are
 * written by the kernels only; every block address comes from an ordinal below the segment's block count).  Where
 * pr_jpeg_decode ends with status 0 this entry gives the same pixels and status 0, for every accepted subseq_bytes and
 * max_rounds and whether or not the frame fell back.  Where pr_jpeg_decode ends with a non-zero status so does this entry;
 * which bits are set, and the pixels, are not promised (nothing behind a code no table holds is written here; a segment
 * that completes fewer blocks than it holds gets PR_JPEG_ST_TRUNCATED).
 *
 * opts NULL takes the build's defaults (128 bytes, 16 rounds unless pr_build_info says otherwise).  subseq_bytes: a multiple
 * of 4 in 16..4096, or 0 for the default; max_rounds: 1..64 (0 is an error: a caller that passes opts names its rounds).  stats: device, [F], may be NULL; n_subseq = the sum over the
 * frame's segments of ceil(length / subseq_bytes), rounds = the round at which the frame converged, or max_rounds when it fell
 * back.  pr_jpeg_sync_workspace_bytes is what the call needs for these sizes and options (0 for invalid ones): pr_jpeg_decode's
 * workspace plus 60 bytes per sub-sequence, of which there are at most data_bytes / subseq_bytes + n_segments + 1.  Otherwise
 * the rules are pr_jpeg_decode's: all device pointers, a 16-byte aligned workspace, asynchronous on `stream`, no allocation, no
 * blocking copy, no synchronisation (capturable), argument errors return PR_ERR_INVALID by name before any device work, F = 0
 * returns PR_OK.  No ABI bump: functions were added. */
typedef struct pr_jpeg_sync_opts { int32_t subseq_bytes, max_rounds; } pr_jpeg_sync_opts;  /* subseq_bytes 0 = the build's default */
typedef struct pr_jpeg_sync_stats { int32_t n_subseq, rounds, fell_back, reserved; } pr_jpeg_sync_stats; /* per frame */
size_t pr_jpeg_sync_workspace_bytes(int F, int H, int W, int64_t data_bytes, int n_segments, const pr_jpeg_sync_opts* opts);
int pr_jpeg_decode_sync(const pr_jpeg_args* args, const pr_jpeg_sync_opts* opts, pr_jpeg_sync_stats* stats, void* workspace,
                        size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------ */
/* j1b progressive and multi-scan JPEG frames -> the same pixels, through the same back   */
/*     end (what cjpeg -progressive, mozjpeg, Pillow's progressive=True write)            */
/* ------------------------------------------------------------------------------------ */
/* pr_jpeg_parse_scans (csrc/jpeg_scans_host.cc, no device) is pr_jpeg_parse with scans; pr_jpeg_decode_scans
 * (csrc/jpeg_scans.hip) fills the int16 coefficient workspace from all scans of a frame and then runs j1's IDCT and colour
 * kernels unchanged.  A COMPLETE progressive file decodes to the pixels of the baseline file with the same coefficients
 * (libjpeg's inter-block smoothing runs on incomplete files only), so the arithmetic contract of j1 is the contract here.
 * pr_jpeg_parse and pr_jpeg_decode are unchanged and keep refusing these files.  No ABI bump: functions and structs were added.
 *
 * Accepted: everything pr_jpeg_parse accepts -- for such a frame the pr_jpeg_frame and pr_jpeg_segment records are the ones
 *   pr_jpeg_parse writes, so a call without multi-scan frames (counts[6] == 0) can go to pr_jpeg_decode / pr_jpeg_decode_sync --
 *   and additionally SOF2 (8-bit, Huffman, progressive) and SOF0 whose components come in more than one scan (every scan one
 *   component or an interleaved subset in frame order, Ss = 0, Se = 63, Ah = Al = 0, every component exactly once).  Sizes,
 *   component counts, sampling, quantiser precision and table ids are limited as in j1.  Tables may be redefined between
 *   scans: every scan names the table set in force at its SOS (the tables that scan uses; identical sets are stored once);
 *   a component's quantiser is the one in force at its FIRST scan (as libjpeg latches it); a DRI between scans holds for the
 *   later scans.  A multi-scan frame's pr_jpeg_frame has restart_interval, huff_set of its first scan and dc_sel / ac_sel as
 *   of each component's first scan (the device reads the scan records instead); first_segment / n_segments cover all scans.
 * Refused by name (pr_jpeg_scan_refusal_name; codes below 16 are pr_jpeg_parse's), never guessed at:
 *   PR_JPEG_E_SCAN_BAND           Ss > Se, Se > 63, Ah or Al > 13, or an SOF2 scan with Ss = 0 and Se != 0
 *   PR_JPEG_E_SCAN_AC_COMPONENTS  an AC scan (Ss > 0) with more than one component
 *   PR_JPEG_E_SCAN_FIRST_AH       the first scan of its coefficients has Ah != 0
 *   PR_JPEG_E_SCAN_REFINE         a refinement whose Ah is not the previous Al of every coefficient it covers, or Al != Ah - 1
 *   PR_JPEG_E_SCAN_AC_BEFORE_DC   an AC scan of a component before that component's first DC scan
 *   PR_JPEG_E_SCAN_REFINE_UNSENT  a refinement that covers sent coefficients and ones never sent
 *   PR_JPEG_E_SCAN_TWICE          a component or coefficient coded twice at one precision (Ah = 0 again, or Al = its present Al)
 *   PR_JPEG_E_SCAN_INCOMPLETE     at EOI a coefficient 0..63 of a component was never sent or has not reached Al = 0: libjpeg
 *                                 would smooth such a file and its pixels are not this contract's
 *   SOF0 scans with spectral selection or approximation get PR_JPEG_E_PROGRESSIVE, SOF1 / arithmetic / 12-bit their j1 codes.
 * Scans.  pr_jpeg_scan: the frame, the components of the scan (indices into the frame's, ascending), Ss, Se, Ah, Al, the
 *   selectors, the table set, the restart interval, its run of the segment array, its MCU count and its level.  Every
 *   segment has a byte range, its frame (pr_jpeg_segment), its scan (segment_scan[i]) and its first MCU OF THAT SCAN.  A scan
 *   of several components walks the frame's MCU grid (ceil(W / 8 hs) x ceil(H / 8 vs) MCUs of h x v blocks per component); a
 *   scan of ONE component has one block per MCU and covers only ceil(dw / 8) x ceil(dh / 8) blocks of the component's own
 *   size dw x dh, row by row -- not the MCU-padded grid (W = 17 at 4:2:0: 3 luma blocks a row, 4 in an interleaved scan).
 * Levels.  level = 0 where no earlier scan of the frame touches one of the scan's (component, coefficient) pairs, else 1 + the
 *   largest level among the earlier scans that do.  Scans of one level write disjoint coefficients and are decoded
 *   concurrently, one launch per level: libjpeg's default scripts (10 scans colour, 6 gray) have 3 levels, a sequential
 *   multi-scan file 1.  Scans of one level may share 8x8 BLOCKS (other coefficients of them): a kernel writes single
 *   coefficients, never a whole block.
 * Device.  A lane is one (scan, restart segment), lanes dealt thinly over waves as in pr_jpeg_decode.  Five procedures:
 *   sequential (Ss = 0, Se = 63): j1's block decode over the scan's own MCU geometry;
 *   DC first (Ss = Se = 0, Ah = 0): prediction per component, reset at each restart; stored pred * 2^Al;
 *   DC refine (Ss = Se = 0, Ah > 0): one raw bit per block, OR-ed in as 1 << Al;
 *   AC first (Ss > 0, Ah = 0): run/size symbols, ZRL, EOBn with the EOBRUN counter (reset at each restart); stored v * 2^Al;
 *   AC refine (Ss > 0, Ah > 0): T.81 G.1.2.3 -- a new coefficient has size 1 and the value +-(1 << Al); correction bits for the
 *     non-zero coefficients passed over in a run and in EOB runs, applied where (coef & (1 << Al)) == 0, adding 1 << Al to a
 *     positive and subtracting it from a negative coefficient.
 * Status and memory safety (on ANY bytes; j1's paragraph holds for this entry): every read of `data` lies inside the
 *   segment's byte range; every block address comes from an ordinal below the scan's block count; an EOB run longer than the
 *   blocks left in its segment or a run past Se ends the segment with PR_JPEG_ST_BAD_RUN, a refinement symbol of size > 1 or a
 *   code no table holds with PR_JPEG_ST_BAD_CODE (in a sequential scan a run past 63 ends the block, as in j1); a value that
 *   leaves int16 after the shift or a correction is clamped with PR_JPEG_ST_COEF_RANGE; every descriptor field that forms an
 *   address or a shift (segment_scan, the scan's frame, level, component indices and order, Ss / Se / Ah / Al, table set,
 *   selectors, restart interval, first MCU) is checked on the device and a failure gives the frame PR_JPEG_ST_REFUSED; a bad
 *   frame never touches another frame's workspace, pixels or status.  Parity with libjpeg on corrupt streams is NOT promised.
 * Mixed calls.  A frame pr_jpeg_parse accepts is one interleaved sequential scan at level 0 and gets pr_jpeg_decode's pixels
 *   and status; in such a call it is decoded one lane per restart segment (pr_jpeg_decode_sync's sub-sequence kernels do not
 *   run for a call that holds a multi-scan frame). */
enum { /* pr_jpeg_parse_scans' parse_status[f] beyond pr_jpeg_parse's; pr_jpeg_scan_refusal_name gives the words of all */
  PR_JPEG_E_SCAN_BAND = 16, PR_JPEG_E_SCAN_AC_COMPONENTS = 17, PR_JPEG_E_SCAN_FIRST_AH = 18, PR_JPEG_E_SCAN_REFINE = 19,
  PR_JPEG_E_SCAN_AC_BEFORE_DC = 20, PR_JPEG_E_SCAN_REFINE_UNSENT = 21, PR_JPEG_E_SCAN_TWICE = 22,
  PR_JPEG_E_SCAN_INCOMPLETE = 23, PR_JPEG_E_SCAN_COUNT = 24
};
#define PR_JPEG_MAX_LEVELS 16 /* Al <= 13: a first scan and at most 14 refinements of a coefficient */
typedef struct pr_jpeg_scan {
  int32_t frame;
  int32_t ncomp;                     /* components in the scan, 1..3 */
  int32_t comp[3];                   /* indices into the frame's components, ascending */
  int32_t dc_sel[3], ac_sel[3];      /* per component of the scan: 0 or 1 */
  int32_t ss, se, ah, al;
  int32_t huff_set;
  int32_t restart_interval;          /* MCUs of THIS scan per restart segment, 0 = none */
  int32_t first_segment, n_segments; /* this scan's run of the segment array */
  int32_t n_mcus;                    /* MCUs of this scan (blocks, for a scan of one component) */
  int32_t level;
} pr_jpeg_scan;

/* pr_jpeg_parse with scans: the same arguments, rules, capacity protocol and error returns, plus scans_host[scan_capacity]
 * and segment_scan_host[segment_capacity] (segment i belongs to scan segment_scan_host[i]; scans and segments are in file
 * order, frame by frame).  counts_host[8] = segments, table sets, H, W, scans, levels (1 + the largest level of an accepted
 * frame, 0 without one), frames with more than one scan, 0.  PR_ERR_CAPACITY when any of the three capacities was too small.
 * Never reads outside [offsets_host[0], offsets_host[F]). */
int pr_jpeg_parse_scans(const uint8_t* data_host, const int64_t* offsets_host, int F, int H, int W, pr_jpeg_frame* frames_host,
                        pr_jpeg_segment* segments_host, int32_t* segment_scan_host, int segment_capacity, pr_jpeg_huff* huff_host,
                        int huff_capacity, pr_jpeg_scan* scans_host, int scan_capacity, int32_t* parse_status_host,
                        int32_t* counts_host);
const char* pr_jpeg_scan_refusal_name(int code);

/* Device memory pr_jpeg_decode_scans needs: pr_jpeg_workspace_bytes(F, H, W). */
size_t pr_jpeg_scans_workspace_bytes(int F, int H, int W);

/* base: as for pr_jpeg_decode, from pr_jpeg_parse_scans' records; scans, segment_scan: its other two arrays, uploaded
 * unchanged; n_levels = counts[5].  One asynchronous clear of the coefficients and the status words, one entropy launch per
 * level, then pr_jpeg_decode's IDCT and colour kernels.  Argument rules, asynchrony and capturability are pr_jpeg_decode's
 * (no allocation, no blocking copy, no synchronisation); n_levels outside 0..PR_JPEG_MAX_LEVELS or scans missing where there
 * are segments return PR_ERR_INVALID. */
typedef struct pr_jpeg_scans_args {
  pr_jpeg_args base;
  const pr_jpeg_scan* scans;
  const int32_t* segment_scan;
  int32_t n_scans, n_levels;
} pr_jpeg_scans_args;
int pr_jpeg_decode_scans(const pr_jpeg_scans_args* args, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------ */
/* j2  u8[F,H,W,3] on the device -> baseline JPEG files, byte-exact with libjpeg          */
/* replaces: cv2.VideoWriter / one PNG per frame behind the composed canvases             */
/*           (write_gpu_video, sinks.py): only compressed bytes leave the device          */
/* ------------------------------------------------------------------------------------ */
/* The inverse of j1.  The host half (pr_jpeg_encode_plan, csrc/jpeg_host.cc, no device) derives the tables and writes the
 * header bytes; the device half (pr_jpeg_encode, csrc/jpeg_enc.hip) does everything else.  No ABI bump: functions were added.
 *
 * Accepted: u8 [F,H,W,3] frames (RGB, or BGR with bgr != 0), 16 <= H, W <= 4096, three components, luma sampling hs x vs =
 *   1x1 (4:4:4), 2x1 (4:2:2) or 2x2 (4:2:0) with chroma 1x1, quality 1..100, one interleaved scan, a restart interval in MCUs
 *   (0 = none, -1 = one MCU row; libjpeg keeps at most 65535).  Gray output, progressive mode and optimised Huffman tables are
 *   out of scope: there is no entry for them.
 *
 * Arithmetic contract.  Integer-exact, so that tests/jpeg_enc_ref.py (numpy), the kernels and libjpeg's default compress path
 *   (jpeg_fdct_islow, no smoothing, the standard Huffman tables, optimize=False: what Pillow's Image.save writes) agree on every
 *   byte of the file.  All shifts are arithmetic; DESCALE(x, n) = (x + (1 << (n-1))) >> n.
 * Colour (SCALEBITS 16).  Y = (19595 R + 38470 G + 7471 B + 32768) >> 16, Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) +
 *   32767) >> 16, Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16.
 * Edges and downsampling, in this order (the order shows in the last chroma block row of a height that is no multiple of 16):
 *   1. the right column is replicated out to the MCU-padded width 8 hs mx;  2. the bottom row is replicated only up to a
 *   multiple of vs;  3. chroma is downsampled: h2v2 (a + b + c + d + bias) >> 2 with bias 1, 2, 1, 2, ... across OUTPUT columns,
 *   h2v1 (a + b + bias) >> 1 with bias 0, 1, 0, 1, ...;  4. the last DOWNSAMPLED row is replicated to the MCU rows' height
 *   8 my.  Luma is replicated in both directions.  (As one rule per sample: clamp the source column to W - 1; for chroma clamp
 *   the downsampled row to ceil(H / vs) - 1 first, then each of its source rows to H - 1.)
 * FDCT.  jpeg_fdct_islow of jpeg-6b (jfdctint.c, CONST_BITS 13, PASS1_BITS 2) on sample - 128: pass 1 along the rows, pass 2
 *   down the columns.  One 1-D pass on d0..d7:
 *     t0=d0+d7; t7=d0-d7; t1=d1+d6; t6=d1-d6; t2=d2+d5; t5=d2-d5; t3=d3+d4; t4=d3-d4
 *     t10=t0+t3; t13=t0-t3; t11=t1+t2; t12=t1-t2
 *     out0 = t10+t11, out4 = t10-t11:  << 2 in pass 1, DESCALE(., 2) in pass 2
 *     z1=(t12+t13)*4433; out2 = z1+t13*6270; out6 = z1-t12*15137
 *     z1=t4+t7; z2=t5+t6; z3=t4+t6; z4=t5+t7; z5=(z3+z4)*9633
 *     t4*=2446; t5*=16819; t6*=25172; t7*=12299; z1*=-7373; z2*=-20995; z3=z3*-16069+z5; z4=z4*-3196+z5
 *     out7 = t4+z1+z3; out5 = t5+z2+z4; out3 = t6+z2+z3; out1 = t7+z1+z4
 *   with out1..3 and out5..7 DESCALEd by 11 in pass 1 and by 15 in pass 2.
 *   32-bit evaluation.  libjpeg computes in `long`; the kernel in 32-bit two's complement.  As in j1 a pass is ring operations,
 *   so an output before DESCALE is exact whenever its 64-bit value fits int32.  As a matrix a pass has rows whose |c_k| sum to
 *   65536 (out0, out4), 59386, 60544, 59380, 59386, 60548 (out6: 4 * (10704 + 4433), the largest of the DESCALEd rows) and
 *   59384; out0 and out4 are plain sums of eight inputs.  With every input of a pass at most PR_JPEG_FDCT_BOUND = 35467 in
 *   magnitude, |out| + 2^14 <= 60548 * 35467 + 16384 = 2 147 472 300 < 2^31 (35468 would exceed it) and 8 * 35467 << 2 fits
 *   easily: exact.  Every 8-bit image is inside: pass 1 reads |d| <= 128, so its results are at most 8 * 128 * 4 = 4096
 *   (out0, out4) and (60548 * 128 + 1024) >> 11 = 3784 (the others); pass 2 reads those, 4096 <= 35467.  Its results, the
 *   coefficients, are at most (8 * 4096 + 2) >> 2 = 8192 and (60548 * 4096 + 16384) >> 15 = 7569 in magnitude.  The kernel
 *   therefore checks nothing at run time.
 * Quantisation.  Tables from `quality` by libjpeg's formula: scale = 5000 / quality below 50, else 200 - 2 quality; entry =
 *   (base * scale + 50) / 100 clamped to 1..255; base = Annex K (luminance for Y, chrominance for Cb and Cr).  With q8 = 8 *
 *   entry (the FDCT leaves its results scaled by 8), |c| becomes (|c| + q8 / 2) / q8 and the sign is restored.  The kernel
 *   multiplies by ceil(2^32 / q8) and keeps the high word: exact for |c| + q8 / 2 < 2^21 (the error of the product is below
 *   x / 2^32 < 1 / q8), checked exhaustively for every magnitude up to 16384 and every divisor 8..2040 in
 *   tests/test_jpeg_encode_native.py.
 * Dummy blocks: those an MCU holds beyond the component's own ceil(size / 8) blocks (luma only, for these samplings).  Their
 *   AC terms are zero and their DC term equals the DC term of the previous block in MCU order (a run of them copies one value
 *   along), whether the block lies in the extra column or in the extra block rows.
 * Entropy coding.  The standard's tables (Annex K.3; luma uses DC 0 / AC 0, chroma DC 1 / AC 1); the DC difference per
 *   component, reset at every restart; runs of sixteen zeros as ZRL (0xF0) only in front of a non-zero term, EOB (0x00) when
 *   the block ends in zeros, as jchuff.c's encode_one_block; a negative value v of n bits is sent as v - 1 in n bits.  Every
 *   segment's last partial byte is filled with 1-bits; every 0xFF of the coded data, that byte included, is followed by 0x00;
 *   RSTn between segments cycles 0..7.  A block takes at most PR_JPEG_ENC_BLOCK_BITS = 11 + 11 + 63 * (16 + 10) = 1660 bits
 *   (the longest DC code and value; for each AC term the longest code and value).
 * File.  SOI; APP0 JFIF 1.01, units 0, density 1 x 1; one DQT marker per table (0, then 1; 8-bit, zig-zag order); SOF0 with
 *   component ids 1, 2, 3; one DHT marker per table (DC 0, AC 0, DC 1, AC 1); DRI when the interval is non-zero; SOS; the
 *   data; EOI.
 * Capacity.  pr_jpeg_encode_bound = the header + PR_JPEG_ENC_BLOCK_BITS / 4 bytes per block (every byte stuffed) + 4 bytes per
 *   segment (a pad byte, its stuffing, a marker) + EOI: no file exceeds it.  A caller may give each frame a smaller slot:
 *   a frame that does not fit gets nbytes[f] = 0 and status PR_JPEG_ENC_ST_OVERFLOW and NOTHING is written to its slot; a
 *   frame writes exactly nbytes[f] bytes from the start of its slot, never another frame's. */
#define PR_JPEG_FDCT_BOUND 35467
#define PR_JPEG_ENC_BLOCK_BITS 1660
#define PR_JPEG_ENC_HEADER_MAX 640
enum { PR_JPEG_ENC_ST_OVERFLOW = 1 }; /* bits of pr_jpeg_encode's status[f] */
typedef struct pr_jpeg_enc_plan { /* what one (quality, sampling, restart interval, size) needs; uploaded unchanged */
  int32_t width, height, hs, vs;
  int32_t restart_interval;          /* resolved: MCUs per segment, 0 = none */
  int32_t quality, header_bytes, reserved;
  uint16_t quant[2][64];             /* natural order: luma, chroma */
  uint32_t recip[2][64];             /* ceil(2^32 / (8 quant)) */
  uint16_t dc_code[2][16], ac_code[2][256]; /* per symbol; length 0 = the table has no such symbol */
  uint8_t dc_len[2][16], ac_len[2][256];
  uint8_t header[PR_JPEG_ENC_HEADER_MAX];   /* SOI .. SOS, header_bytes of them */
} pr_jpeg_enc_plan;

/* Fills *plan_host.  PR_ERR_INVALID by name for quality outside 1..100, a sampling other than 1x1, 2x1, 2x2, a size outside
 * 16..4096, restart_interval < -1 or a null pointer.  No device call. */
int pr_jpeg_encode_plan(int quality, int hs, int vs, int restart_interval, int H, int W, pr_jpeg_enc_plan* plan_host);
/* A size no file of these parameters exceeds (0 for invalid ones). */
size_t pr_jpeg_encode_bound(int H, int W, int hs, int vs, int restart_interval);
/* Device memory pr_jpeg_encode needs for F frames with `capacity` bytes a slot (0 for invalid parameters). */
size_t pr_jpeg_encode_workspace_bytes(int F, int H, int W, int hs, int vs, int restart_interval, int64_t capacity);

/* All device pointers: frames u8[F,H,W,3], plan (one pr_jpeg_enc_plan, uploaded), out u8[F,capacity], nbytes int32[F], status
 * int32[F] (bits PR_JPEG_ENC_ST_*).  H, W, hs, vs, restart_interval as given to pr_jpeg_encode_plan (the host cannot read the
 * plan; the kernels take the tables and the header from it and the geometry from here).  Each slot receives the whole file,
 * header and EOI included.  The workspace must be 16-byte aligned.  Argument errors (null pointers, sizes or sampling outside
 * the accepted ones, capacity < 0 or above 2^31 - 1, a workspace below pr_jpeg_encode_workspace_bytes or misaligned) return
 * PR_ERR_INVALID by name before any device work; F = 0 returns PR_OK.  Asynchronous on `stream`, no allocation, no blocking
 * copy, no synchronisation (capturable). */
typedef struct pr_jpeg_enc_args {
  const uint8_t* frames;
  const pr_jpeg_enc_plan* plan;
  uint8_t* out;
  int32_t* nbytes;
  int32_t* status;
  int64_t capacity;
  int F, H, W;
  int hs, vs, restart_interval;
  int bgr;
} pr_jpeg_enc_args;
int pr_jpeg_encode(const pr_jpeg_enc_args* args, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------ */
/* j3  u8[F,H,W,3] -> u8[F,h,w,3] on the device: the front end's bilinear downscale       */
/* replaces: cv2.resize in get_images lib/utils/funcs_utils.py:18-53 (width > 800 -> 800   */
/*           wide, elif height > 450 -> 450 high) in front of the tracker and the crops    */
/* ------------------------------------------------------------------------------------ */
/* The host half (pr_resize_plan, csrc/resize_host.cc, no device) makes the per-axis tap tables; the device half
 * (pr_resize_frames, csrc/resize.hip) applies them.  No ABI bump: functions were added.
 *
 * Arithmetic contract.  This project's own, integer-defined and modelled on the 8-bit path of OpenCV's INTER_LINEAR
 *   (fixed-point weights of 2048, a horizontal pass into int32, a vertical pass with two truncating shifts).  OpenCV is not
 *   available where this project is built and tested, so its bits are NOT promised; what is promised is the following, which
 *   tests/resize_ref.py restates in numpy and which stays strictly within one level of the float64 bilinear at the same sample
 *   positions (tests/test_frontend_cpu.py).  The three channels are treated alike: there is no bgr argument.
 * Taps.  For each axis with source size S and destination size d: scale = 1.0 / ((double)d / S); for i in [0, d):
 *     f = (float)((i + 0.5) * scale - 0.5)      the product and the difference in double, rounded to float once
 *     s = floor(f);  f -= s                     in float
 *     if s < 0:       s = 0,     f = 0
 *     if s >= S - 1:  s = S - 1, f = 0
 *     c0 = rne((1.f - f) * 2048.f),  c1 = rne(f * 2048.f)      int16, round to nearest even
 *   ofs[i] = s, coef[2 i] = c0, coef[2 i + 1] = c1; the second tap is min(s + 1, S - 1).  0 <= c0, c1 <= 2048.
 * Passes.  With a0, a1 the weights of the destination column and b0, b1 those of the destination row, S0 and S1 the two
 *   source samples of a row at the column's taps:
 *     horizontal   T = S0 * a0 + S1 * a1                                              int32, at most 255 * 2049
 *     vertical     D = (((b0 * (T0 >> 4)) >> 16) + ((b1 * (T1 >> 4)) >> 16) + 2) >> 2   stored as u8
 *   T0, T1 are the horizontal results of the destination row's two source rows.  Every term is non-negative and D <= 255
 *   (2049 * (255 * 2049 >> 4) >> 16 = 1020), so nothing is clamped.
 * Exactly half in both axes (W == 2 w and H == 2 h; PR_RESIZE_HALF): D = (s00 + s01 + s10 + s11 + 2) >> 2 over the 2 x 2
 *   source samples of the destination sample.  (W == 2 w alone does not take this rule.)
 * Same size (PR_RESIZE_COPY): a copy. */
#define PR_RESIZE_MAX_SIDE 4096
enum { PR_RESIZE_COPY = 0, PR_RESIZE_HALF = 1, PR_RESIZE_LINEAR = 2 }; /* pr_resize_plan's *mode_host */

/* Fills xofs_host int32[w], xcoef_host int16[2 w], yofs_host int32[h], ycoef_host int16[2 h] (in every mode) and *mode_host.
 * PR_ERR_INVALID by name for a side outside 1..PR_RESIZE_MAX_SIDE or a null pointer, before anything is written.  No device
 * call. */
int pr_resize_plan(int H, int W, int h, int w, int32_t* xofs_host, int16_t* xcoef_host, int32_t* yofs_host, int16_t* ycoef_host,
                   int32_t* mode_host);

/* All device pointers: src u8[F,H,W,3], dst u8[F,h,w,3] (any alignment: the call's output is written in aligned dwords, with
 * byte stores only for the up to three bytes at either end), the four tables as pr_resize_plan filled them, uploaded unchanged
 * (xofs and yofs 4-byte, xcoef and ycoef 2-byte aligned), mode as it gave it.  Reads only src and the tables (table offsets are
 * clamped to the source on the device), writes every byte of dst and nothing else.  Argument errors (null pointers, a side
 * outside 1..PR_RESIZE_MAX_SIDE, a mode that is not the one of these sizes, F < 0) return PR_ERR_INVALID by name before any
 * device work; F = 0 returns PR_OK.  Asynchronous on `stream`, no allocation, no copy, no synchronisation (capturable). */
int pr_resize_frames(const uint8_t* src, int F, int H, int W, uint8_t* dst, int h, int w, const int32_t* xofs,
                     const int16_t* xcoef, const int32_t* yofs, const int16_t* ycoef, int mode, void* stream);

/* ------------------------------------------------------------------------------------ */
/* j4  PNG frames decoded on the GPU, exact with zlib and libpng                           */
/* no reference counterpart: the reference's front end writes JPEG; PNG is what ffmpeg,    */
/*           screen recorders, annotation tools and this project's own report path write   */
/* ------------------------------------------------------------------------------------ */
/* The host half (pr_png_parse, csrc/png_host.cc, no device) walks the chunks and emits descriptors only; the device half
 * (pr_png_decode, csrc/png.hip over csrc/png_device.h) gathers each frame's IDAT payloads, inflates them, undoes the filters,
 * verifies the Adler-32 and writes the pixels.  tests/png_ref.py restates this section in Python.  No ABI bump: functions and
 * structs were added.
 *
 * Accepted.  PNG of bit depth 8, colour type 0 (gray), 2 (RGB), 3 (palette), 4 (gray + alpha) or 6 (RGBA), non-interlaced,
 *   1..PR_PNG_MAX_SIDE pixels a side, any number of IDAT chunks of any length (empty ones included).  All frames of a call
 *   have one size.
 * Output.  u8[F,H,W,3], RGB, or BGR when bgr != 0.  Gray is replicated.  Alpha is DROPPED, not composited (what cv2.imread's
 *   default and Pillow's .convert("RGB") do).  tRNS, gAMA, iCCP and every other ancillary chunk are ignored (their CRC is
 *   still verified).  The parser uploads a palette padded to 256 entries with zeros, so an index past PLTE reads black;
 *   Pillow 12 does the same (tests/test_png_cpu.py checks it).
 * Refused by name (parse_status, pr_png_refusal_name): not a PNG signature; a file that ends inside a chunk; a chunk CRC-32
 *   mismatch; a missing or misplaced IHDR, PLTE, IDAT or IEND (IHDR not first or not 13 bytes, a second IHDR, PLTE behind
 *   IDAT or twice or missing for colour type 3 or not 3..768 bytes in threes, IDAT chunks not consecutive, no IDAT, no IEND);
 *   16-bit depth; bit depth 1, 2 or 4; Adam7 interlace; Apple's CgBI; an IHDR no PNG has (another depth or colour type, a
 *   depth the colour type does not allow, compression or filter method not 0, a side of 0 or above PR_PNG_MAX_SIDE); a size
 *   other than the call's; a zlib header with CM != 8, a window above 32 KiB, FDICT set, a bad FCHECK, or shorter than 2 bytes.
 * Inflate rule.  RFC 1951 with zlib 1.2.11's acceptance rules: a frame gets a non-zero device status exactly where
 *   zlib.decompress would raise.  Errors (PR_PNG_ST_BAD_CODE): block type 3; a stored block with LEN != ~NLEN; HLIT above 286
 *   or HDIST above 30 symbols; an over-subscribed code-length set; an incomplete set, unless it is a literal/length or distance
 *   set that is a single code of length 1 (the code-length code itself may not be incomplete; a distance set with no code at
 *   all is legal until a distance is decoded); a set with no end-of-block code; a repeat code 16 / 17 / 18 that runs past
 *   HLIT + HDIST; a repeat code 16 with nothing before it; a bit pattern no code of the set matches; a length symbol above 285
 *   or a distance symbol above 29; a distance that reaches before the start of the output.  Input that ends before the final
 *   block's end-of-block code or inside the four Adler-32 bytes behind it is PR_PNG_ST_TRUNCATED.  Bytes behind the Adler-32
 *   are ignored, as zlib.decompress ignores them.
 *   Beyond zlib: output shorter or longer than H (1 + W bpp) bytes is PR_PNG_ST_SIZE (decoding stops at the first byte that
 *   would not fit), a filter byte above 4 PR_PNG_ST_FILTER (the row is taken as filter 0), an Adler-32 of the inflated bytes
 *   that differs from the trailer PR_PNG_ST_CHECKSUM.
 * Unfilter.  The spec's unsigned-byte arithmetic per byte, with a = the byte bpp to the left, b = the byte above, c = the byte
 *   above a (0 outside the image): None x, Sub x + a, Up x + b, Average x + ((a + b) >> 1), Paeth x + the one of a, b, c that
 *   is nearest p = a + b - c, ties in the order a, b, c.
 * Status and pixels.  status[f] = 0: the frame's pixels are exact.  A frame the parser refused, or whose descriptor or IDAT
 *   ranges fail the device's checks, has PR_PNG_ST_REFUSED and zero pixels; a frame whose inflate failed (TRUNCATED, BAD_CODE,
 *   SIZE) has zero pixels; a frame with PR_PNG_ST_FILTER or PR_PNG_ST_CHECKSUM alone has the pixels its bytes give.
 * Isolation and memory safety (on ANY bytes).  A frame's stream lies in its own part of the workspace, bounded by the stream
 *   length its descriptor states, which the gather checks against the IDAT ranges, themselves checked against data_bytes and
 *   against each other (ascending, not overlapping); every read of the stream is bounded by its end (bits behind it do not
 *   exist: a symbol that needs one is PR_PNG_ST_TRUNCATED); every write of the inflated bytes is bounded by H (1 + W bpp) and
 *   every match reads only bytes this frame has already written; pixels go to the frame's own slot of `out`.  A bad frame
 *   leaves every other frame's pixels and status untouched. */
#define PR_PNG_MAX_SIDE 4096
enum { /* bits of pr_png_decode's status[f] */
  PR_PNG_ST_REFUSED = 1, PR_PNG_ST_TRUNCATED = 2, PR_PNG_ST_BAD_CODE = 4, PR_PNG_ST_SIZE = 8, PR_PNG_ST_FILTER = 16,
  PR_PNG_ST_CHECKSUM = 32
};
enum { /* pr_png_parse's parse_status[f]; pr_png_refusal_name gives the words */
  PR_PNG_OK = 0, PR_PNG_E_SIGNATURE = 1, PR_PNG_E_TRUNCATED = 2, PR_PNG_E_CRC = 3, PR_PNG_E_CHUNK_ORDER = 4, PR_PNG_E_DEPTH16 = 5,
  PR_PNG_E_DEPTH_SUB8 = 6, PR_PNG_E_INTERLACE = 7, PR_PNG_E_CGBI = 8, PR_PNG_E_IHDR = 9, PR_PNG_E_SIZE_DIFFERS = 10,
  PR_PNG_E_ZLIB_HEADER = 11, PR_PNG_E_COUNT = 12
};
typedef struct pr_png_frame {
  int32_t width, height;
  int32_t color_type;          /* 0, 2, 3, 4 or 6 */
  int32_t bpp;                 /* bytes per pixel: 1, 3, 1, 2, 4; 0 = refused by the parser (the device zero-fills the frame) */
  int32_t first_idat, n_idat;  /* this frame's run of the IDAT range array */
  int32_t palette;             /* slot in the palette array for colour type 3, else -1 */
  int32_t reserved;
  int64_t zlib_bytes;          /* the zlib stream's length: the sum of the IDAT ranges' lengths */
} pr_png_frame;
typedef struct pr_png_idat { /* one IDAT chunk's payload: a byte range in `data` */
  int64_t begin, end;
} pr_png_idat;

/* data_host, offsets_host, F, H, W as for pr_jpeg_parse (H, W: the size every frame must have, or 0, 0 to adopt the first
 * accepted frame's).  Checks the signature, walks the chunks, verifies every chunk's CRC-32, validates IHDR and the zlib
 * header (found across IDAT boundaries) and fills frames_host[F], parse_status_host[F] (PR_PNG_OK or a refusal; a refused
 * frame has bpp = 0 and no ranges), up to idat_capacity ranges in idat_host, up to palette_capacity palettes of 256 x 3 bytes
 * (RGB, zero behind PLTE's entries) in palettes_host, and counts_host[4] = ranges used, palettes used, H, W.  No payload is
 * copied.  Returns PR_OK also when frames were refused (the last refusal is named in pr_last_error with its frame index),
 * PR_ERR_CAPACITY when a capacity was too small (counts_host then holds what is needed; nothing else is valid),
 * PR_ERR_INVALID for a null pointer, F < 0, a size outside 1..PR_PNG_MAX_SIDE or offsets out of order, before anything is
 * dereferenced.  F = 0 is legal.  Ranges are absolute offsets in data_host and lie inside their file.  Never reads outside
 * [offsets_host[0], offsets_host[F]). */
int pr_png_parse(const uint8_t* data_host, const int64_t* offsets_host, int F, int H, int W, pr_png_frame* frames_host,
                 pr_png_idat* idat_host, int idat_capacity, uint8_t* palettes_host, int palette_capacity,
                 int32_t* parse_status_host, int32_t* counts_host);
const char* pr_png_refusal_name(int code);

/* Device memory pr_png_decode needs for F frames of H x W whose files hold data_bytes bytes in all: the gathered streams
 * (data_bytes, padded), one record per frame, and the inflated scanlines at 4 bytes a pixel.  0 for sizes it refuses. */
size_t pr_png_workspace_bytes(int F, int H, int W, int64_t data_bytes);

/* All device pointers: data u8[data_bytes] (what pr_png_parse read, uploaded), frames / idat / palettes its descriptors
 * uploaded unchanged (frames and idat 8-byte aligned), out u8[F,H,W,3] (any alignment; written in dwords where the frame's
 * first byte is 4-byte aligned), status int32[F] (required; bits PR_PNG_ST_*).  The workspace must be 16-byte aligned.  Three
 * kernels behind one asynchronous clear of the status words: gather (a workgroup per frame copies the IDAT payloads into one
 * contiguous stream), inflate (one wavefront per frame, four frames a workgroup), unfilter + Adler-32 + colour (a workgroup
 * per frame).  Argument errors (null pointers, sizes outside 1..PR_PNG_MAX_SIDE, a workspace below pr_png_workspace_bytes --
 * PR_ERR_CAPACITY -- or misaligned, negative counts, ranges without data) are returned by name before any device work;
 * F = 0 returns PR_OK.  Asynchronous on `stream`, no allocation, no blocking copy, no synchronisation (capturable). */
typedef struct pr_png_args {
  const uint8_t* data;
  const pr_png_frame* frames;
  const pr_png_idat* idat;
  const uint8_t* palettes;
  uint8_t* out;
  int32_t* status;
  int64_t data_bytes;
  int F, H, W;
  int n_idat, n_palettes;
  int bgr;
} pr_png_args;
int pr_png_decode(const pr_png_args* args, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------ */
/* j5  u8[F,H,W,3] on the device -> PNG files: filters, run-length deflate, dynamic codes  */
/* replaces: the raw download + Pillow save of one PNG per frame behind the composed       */
/*           canvases (write_gpu_video, sinks.py): only compressed bytes leave             */
/* ------------------------------------------------------------------------------------ */
/* The lossless counterpart of j2 and the inverse of j4.  The host half (pr_png_encode_plan, csrc/png_enc_host.cc, no device)
 * writes the fixed bytes and the CRC power table; the device half (pr_png_encode, csrc/png_enc.hip over
 * csrc/png_enc_device.h) does everything else.  tests/png_enc_ref.py restates this section in numpy and Python.  No ABI bump:
 * functions and structs were added.
 *
 * What is promised.  The bytes are NOT any library's bytes (zlib's match choices and tree heuristics are no contract).  Instead:
 *   (a) every file is a valid PNG that zlib, libpng, Pillow and pr_png_decode decode to exactly the input pixels;
 *   (b) the bytes are a deterministic function of pixels and parameters, fixed by the rules below; kernel and reference agree
 *   on every byte.
 * Accepted.  u8 [F,H,W,3] frames (RGB, or BGR with bgr != 0), 1 <= H, W <= PR_PNG_MAX_SIDE.  Output: colour type 2, depth 8,
 *   non-interlaced.  filter 0..4 = that filter on every row, 5 = adaptive.  mode PR_PNG_ENC_STORED or PR_PNG_ENC_RLE.  Other
 *   colour types, alpha and interlace have no entry.
 * Filtering.  j4's unfilter rules inverted, on unsigned bytes with bpp = 3 (None x, Sub x - a, Up x - b, Average
 *   x - ((a + b) >> 1), Paeth x - the nearest of a, b, c to a + b - c, ties a, b, c; all mod 256).  a, b, c are taken from the
 *   RAW pixels of this row and the row above (0 outside the image), so rows are independent.  Adaptive: per row the filter
 *   whose 3 W output bytes (the type byte is not counted) have the smallest sum of |signed byte| (v < 128 ? v : 256 - v); ties
 *   go to the lowest filter number.  PR_PNG_ENC_STORED uses filter 0 whatever is asked.
 * Segments.  The filtered stream of H (1 + 3 W) bytes is cut into segments of PR_PNG_ENC_SEGMENT = 16384 bytes, the last one
 *   shorter.  Each is coded with no reference to bytes before it and begins and ends on a byte boundary.  A coded segment is
 *   one dynamic block; every segment but the last is followed by an empty stored block (the 3 header bits 000, zero bits up to
 *   the byte boundary, 00 00 FF FF); in the last segment the data block carries BFINAL, is padded with zero bits, and there is
 *   no empty block.
 * Tokens (PR_PNG_ENC_RLE): zlib's deflate_rle rule.  At position i behind the segment's start, if the next three bytes equal
 *   byte i - 1, a match of distance 1 whose length is the run's, capped at 258 and at the segment's end; otherwise a literal.
 *   A maximal run of L equal bytes is therefore one literal, then with R = L - 1: R / 258 matches of 258 and, for the rest r =
 *   R % 258, one match of r when r >= 3, else r literals.
 * Codes.  Literal/length code lengths from the segment's own histogram of literals and length symbols plus one end-of-block
 *   symbol, limit 15 bits; HLIT covers the highest used symbol (at least 257).  The distance set is always the single code 0
 *   of length 1, in a segment without a match too (HDIST = 1; zlib and j4 accept the incomplete set, and a segment without a
 *   match never reads it).  The HLIT + 1 lengths are ONE sequence (a run may pass from the literal/length lengths into the
 *   distance length).  Runs in it: a run of zeros sends, while at least 3 remain, symbol 18 for min(run, 138) when at least 11
 *   remain and else symbol 17 for all of them, and fewer than 3 as they are; a run of a non-zero length sends the length once,
 *   then symbol 16 for min(rest, 6) while at least 3 remain, then the rest as they are.  The code-length code is built from
 *   that sequence's histogram by the same construction with limit 7; HCLEN covers the last used symbol in RFC 1951's order, at
 *   least 4.  Both alphabets always have at least two used symbols (a segment holds a byte and the end-of-block symbol; the
 *   sequence holds the distance length 1 and a literal length above 1), so both codes are complete.
 *   Construction (any alphabet, limit M).  1. The used symbols in (count, symbol) order.  2. Huffman's merge with two queues,
 *   leaves in that order and internal nodes in the order they were made; each step takes the two smallest weights, and of two
 *   equal weights the internal node before the leaf.  Only the NUMBER of codes per depth is kept.  3. Codes deeper than M are
 *   counted at M; while the Kraft sum exceeds 1: one code of length M is dropped, one code of the greatest length d < M that
 *   has any becomes two codes of length d + 1 (one unit of 2^-M a step).  4. The lengths are handed out longest first in the
 *   order of 1.  5. Canonical codes as in RFC 1951 3.2.2.  Nothing depends on lane order: the histogram is integer sums, the
 *   order of 1 is a total order, 2 - 5 are serial.
 * Fallback.  A segment of n bytes is written as ONE stored block (a byte with BFINAL, LEN, NLEN, the n bytes; no empty block
 *   behind it, it ends aligned) when its coded form, the empty block included, would take 5 + n bytes or more, and always in
 *   PR_PNG_ENC_STORED.  So no segment takes more than 5 + n bytes.
 * File.  Signature; IHDR; ONE IDAT chunk holding the zlib header 78 01, the segments, and the Adler-32 of all filtered bytes
 *   big-endian; IEND.  Chunk CRC-32s are computed on the device (IHDR's and IEND's are constants of the plan).  Both checksums
 *   are computed per segment and combined: Adler by the sum rule (A = 1 + sum a_s, B = N + sum (b_s + a_s * bytes behind s),
 *   mod 65521), CRC by multiplying each segment's register by x^(8 * bytes behind it) mod the polynomial, with x^(2^k) from
 *   the plan; inside a segment the 64 lanes do the same with their 1/64ths.
 * Capacity.  pr_png_encode_bound(H, W) = 63 + N + 5 * ceil(N / 16384), N = H (1 + 3 W): 8 signature + 25 IHDR + 12 IDAT
 *   framing + 2 zlib header + 4 Adler-32 + 12 IEND, and 5 + n per segment by the fallback rule.  No file exceeds it; a
 *   PR_PNG_ENC_STORED file has exactly that size.  A caller may give each frame a smaller slot: a frame that does not fit gets
 *   nbytes[f] = 0 and status PR_PNG_ENC_ST_OVERFLOW and NOTHING is written to its slot; a frame writes exactly nbytes[f] bytes
 *   from the start of its slot, never another frame's. */
#define PR_PNG_ENC_SEGMENT 16384
#define PR_PNG_ENC_HEAD_BYTES 43 /* signature .. the zlib header */
#define PR_PNG_ENC_TAIL_BYTES 12 /* IEND */
enum { PR_PNG_ENC_STORED = 0, PR_PNG_ENC_RLE = 1 };
enum { PR_PNG_ENC_FILTER_ADAPTIVE = 5 };
enum { PR_PNG_ENC_ST_OVERFLOW = 1 }; /* bits of pr_png_encode's status[f] */
typedef struct pr_png_enc_plan { /* what one (filter, mode, size) needs; uploaded unchanged */
  /* The first six are informational: they say what the plan was made for (a caller's cache key, a test's check).  The device
   * reads none of them -- the host cannot read an uploaded plan, so pr_png_encode takes the geometry from its arguments, and
   * of the plan only crc_pow, idat_crc_head, head (whose IHDR states the size) and tail. */
  int32_t width, height, filter, mode;
  int32_t n_segments, reserved;
  int64_t raw_bytes;                     /* N = H (1 + 3 W) */
  uint32_t crc_pow[32];                  /* x^(2^k) mod the CRC-32 polynomial, bit-reflected as the CRC register is */
  uint32_t idat_crc_head;                /* the CRC register (not inverted) behind "IDAT" 78 01 */
  uint32_t reserved2;
  uint8_t head[48];                      /* signature, IHDR with its CRC, four zero bytes for IDAT's length, "IDAT", 78 01 */
  uint8_t tail[16];                      /* IEND with its CRC */
} pr_png_enc_plan;

/* Fills *plan_host.  PR_ERR_INVALID by name for a filter outside 0..5, a mode other than the two, a size outside
 * 1..PR_PNG_MAX_SIDE or a null pointer, before anything is dereferenced.  No device call. */
int pr_png_encode_plan(int filter, int mode, int H, int W, pr_png_enc_plan* plan_host);
/* A size no file of an H x W frame exceeds (0 for an invalid size). */
size_t pr_png_encode_bound(int H, int W);
/* Device memory pr_png_encode needs for F frames (0 for invalid parameters): a staging area of 16400 bytes and 20 bytes of
 * records per segment, one filter byte per row, one word per frame. */
size_t pr_png_encode_workspace_bytes(int F, int H, int W);

/* All device pointers: frames u8[F,H,W,3], plan (one pr_png_enc_plan, uploaded), out u8[F,capacity] (any alignment), nbytes
 * int32[F], status int32[F] (bits PR_PNG_ENC_ST_*).  H, W, filter, mode as given to pr_png_encode_plan.  Each slot receives
 * the whole file.  Kernels: choose (adaptive only; a wavefront per row picks its filter), segment (a wavefront per segment:
 * filters its bytes into LDS, tokens, histogram, codes, bits, checksums, into the segment's own staging area), assemble (a
 * workgroup per frame: prefix sum of the segment sizes, the combined checksums, the capacity check, head and tail, nbytes and
 * status), place (a workgroup per segment copies it into the slot, in aligned dwords).  The workspace must be 16-byte aligned.
 * Argument errors (null pointers, a size, filter or mode outside the accepted ones, F < 0 or above 65535, capacity < 0 or above
 * 2^31 - 1, a workspace below pr_png_encode_workspace_bytes or misaligned) return PR_ERR_INVALID by name before any device
 * work; F = 0 returns PR_OK.  Asynchronous on `stream`, no allocation, no blocking copy, no synchronisation (capturable). */
typedef struct pr_png_enc_args {
  const uint8_t* frames;
  const pr_png_enc_plan* plan;
  uint8_t* out;
  int32_t* nbytes;
  int32_t* status;
  int64_t capacity;
  int F, H, W;
  int filter, mode;
  int bgr;
} pr_png_enc_args;
int pr_png_encode(const pr_png_enc_args* args, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------ */
/* j6  YUV4MPEG2 streams -> u8[F,h,w,3] on the device: chroma upsampling, the colour       */
/*     matrix and the front end's downscale in one kernel                                  */
/* replaces: cv2.VideoCapture in get_images lib/utils/funcs_utils.py:18-53 for any video   */
/*           a decoder can pipe out (`ffmpeg -i clip.mp4 -f yuv4mpegpipe -`)               */
/* ------------------------------------------------------------------------------------ */
/* The host half (pr_y4m_parse_header, pr_y4m_index, pr_yuv_plan; csrc/y4m_host.cc, no device) reads the stream syntax and
 * makes the matrix integers; the device half (pr_yuv_frames, csrc/yuv.hip) turns the raw planes of a chunk of the stream,
 * uploaded as they came, into RGB frames, at the source size or downscaled by j3's contract.  tests/yuv_ref.py restates this
 * section in numpy.  No ABI bump: functions and structs were added.
 *
 * Stream syntax.  "YUV4MPEG2", then tagged fields separated by spaces, up to '\n' (within PR_Y4M_MAX_HEADER bytes).  W and H
 *   are required, 1..PR_RESIZE_MAX_SIDE.  F num:den is the frame rate (fps_num = fps_den = 0 when absent; a caller takes
 *   0:0 as 30.0).  I: 'p' and '?' are accepted, 't', 'b', 'm' (interlaced) refused by name.  A and tags this section does
 *   not name are ignored.  C: 420jpeg, 420mpeg2, 420 (= 420jpeg), 422, 444, mono; absent = 420jpeg; 420paldv, every
 *   high-bit-depth variant (420p10, 422p12, 444p16, mono10, ...), 411 and 444alpha are refused by name, any other value as an
 *   unknown layout.  X fields are ignored, except XCOLORRANGE=FULL | LIMITED (full_range 1 | 0; -1 when absent).
 *   Each frame is "FRAME", optional fields, '\n' (within PR_Y4M_MAX_FRAME_HEADER bytes), then frame_bytes = W H + 2 cw ch
 *   bytes: the Y plane, the U plane, the V plane, each row after row without padding; cw = (W + 1) / 2 for 420 and 422, else
 *   W; ch = (H + 1) / 2 for 420, else H; mono has no chroma planes.
 * Chroma to full resolution.  Per axis every output sample has two taps whose weights sum to 4 (indices clamped to the plane):
 *     centred (both axes of 420jpeg, the vertical axis of 420mpeg2)    2 i: 3 c[i] + c[i - 1]     2 i + 1: 3 c[i] + c[i + 1]
 *     co-sited (the horizontal axis of 420mpeg2 and of 422)            2 i: 4 c[i]                2 i + 1: 2 c[i] + 2 c[i + 1]
 *     not subsampled                                                   i:   4 c[i]
 *   C16 = the product of the two axes: up to four taps with weights summing to 16, kept at that scale, nothing rounded.
 * Matrix.  Kr, Kb = 0.299, 0.114 (PR_YUV_601) or 0.2126, 0.0722 (PR_YUV_709); Kg = 1 - Kr - Kb.  Limited range: sy = 255 / 219,
 *   sc = 255 / 224, yo = 16; full range: sy = sc = 1, yo = 0.  pr_yuv_plan computes in double and rounds to nearest even:
 *     cy = sy 65536   crv = 2 (1 - Kr) sc 65536   cbu = 2 (1 - Kb) sc 65536   cgu = 2 Kb (1 - Kb) / Kg sc 65536
 *     cgv = 2 Kr (1 - Kr) / Kg sc 65536            (601 limited: 76309, 104597, 132201, 25675, 53279)
 *   With y = 16 (Y - yo), u = U16 - 2048, v = V16 - 2048 in int32 (mono: u = v = 0), the shift arithmetic (floor):
 *     R = clamp8((cy y + crv v + 2^19) >> 20)   G = clamp8((cy y - cgu u - cgv v + 2^19) >> 20)   B = clamp8((cy y + cbu u + 2^19) >> 20)
 *   No sum exceeds 6.0e8 in magnitude.  The result stays within one level of the float64 evaluation of the same taps and the
 *   exact matrix (tests/test_y4m_cpu.py).  These are this project's own bits; swscale's are not promised, as j3 says of OpenCV's.
 * Downscale.  j3's contract applied to that RGB: with the four tables given, pr_yuv_frames writes bit for bit what
 *   pr_resize_frames makes of the source-size output, in all three modes, and the source-size RGB is never written. */
#define PR_Y4M_MAX_HEADER 1024
#define PR_Y4M_MAX_FRAME_HEADER 256
enum { PR_Y4M_C420JPEG = 0, PR_Y4M_C420MPEG2 = 1, PR_Y4M_C422 = 2, PR_Y4M_C444 = 3, PR_Y4M_CMONO = 4 }; /* pr_y4m_info.chroma */
enum { PR_YUV_601 = 0, PR_YUV_709 = 1 };
enum { /* what pr_y4m_parse_header and pr_y4m_index return besides PR_OK and PR_ERR_INVALID; pr_y4m_refusal_name gives the words */
  PR_Y4M_OK = 0, PR_Y4M_E_MAGIC = 1, PR_Y4M_E_HEADER = 2, PR_Y4M_E_FIELD = 3, PR_Y4M_E_NO_SIZE = 4, PR_Y4M_E_SIZE = 5,
  PR_Y4M_E_INTERLACED = 6, PR_Y4M_E_PALDV = 7, PR_Y4M_E_HIGH_DEPTH = 8, PR_Y4M_E_411 = 9, PR_Y4M_E_ALPHA = 10,
  PR_Y4M_E_CHROMA = 11, PR_Y4M_E_FRAME = 12, PR_Y4M_E_COUNT = 13
};
typedef struct pr_y4m_info {
  int32_t width, height;
  int32_t fps_num, fps_den;    /* 0, 0 when the header has no F field */
  int32_t chroma;              /* PR_Y4M_C* */
  int32_t full_range;          /* 1 XCOLORRANGE=FULL, 0 XCOLORRANGE=LIMITED, -1 absent */
  int32_t header_bytes;        /* the stream header, its '\n' included: the first FRAME starts here */
  int32_t reserved;
  int64_t frame_bytes;         /* one frame's payload: W H + 2 cw ch */
} pr_y4m_info;
typedef struct pr_yuv_coeffs { /* pr_yuv_plan's six integers */
  int32_t cy, crv, cbu, cgu, cgv, yo;
} pr_yuv_coeffs;

/* The stream header in data_host[0, n).  PR_OK and *info_host filled, or a refusal (PR_Y4M_E_*, named in pr_last_error too;
 * PR_Y4M_E_HEADER also when n bytes do not reach the '\n'), or PR_ERR_INVALID for a null pointer or n < 0.  *info_host is
 * written only on PR_OK.  No device call. */
int pr_y4m_parse_header(const uint8_t* data_host, int64_t n, pr_y4m_info* info_host);
const char* pr_y4m_refusal_name(int code);

/* data_host[0, n) begins at a frame boundary (a FRAME header).  Walks the FRAME headers and fills offsets_host with the payload
 * offset of every COMPLETE frame, up to max_frames of them; *n_frames_host = their count, *consumed_host = the bytes up to the
 * end of the last complete frame, so that a streaming caller carries data_host[consumed, n) into its next chunk.  A frame
 * whose header or payload the n bytes do not reach is not an error here (only the caller knows whether more bytes follow; at
 * the end of the stream a remainder is an incomplete frame).  Bytes that cannot begin a FRAME header are PR_Y4M_E_FRAME, named
 * with the frame's index in this buffer; PR_ERR_INVALID for a null pointer, n < 0, max_frames < 0 or an info no header gives.
 * The three outputs are written only on PR_OK.  No device call. */
int pr_y4m_index(const uint8_t* data_host, int64_t n, const pr_y4m_info* info_host, int64_t* offsets_host, int max_frames,
                 int32_t* n_frames_host, int64_t* consumed_host);

/* Fills *plan_host for matrix PR_YUV_601 | PR_YUV_709 and full_range 0 | 1; PR_ERR_INVALID by name for anything else or a null
 * pointer, before anything is written.  No device call. */
int pr_yuv_plan(int matrix, int full_range, pr_yuv_coeffs* plan_host);

/* Device pointers: data u8[data_bytes] (a chunk of the stream as it was read, any alignment), offsets int64[F] (payload
 * offsets in data, as pr_y4m_index gave them, 8-byte aligned; a payload may start at any byte), dst u8[F,h,w,3] (any alignment:
 * the call's output is written in aligned dwords, three a lane, with byte stores only for the few bytes at either end).
 * H, W, chroma: the stream's; plan: pr_yuv_plan's integers, by value; bgr != 0 swaps R and B.  Without a downscale h = w = 0,
 * mode = 0 and the four tables are NULL: dst is u8[F,H,W,3].  With one, h, w, the tables and mode are pr_resize_plan's for
 * (H, W, h, w), uploaded as for pr_resize_frames.  Reads only data, offsets and the tables (table offsets are clamped to the
 * source on the device; a frame whose payload does not lie inside [0, data_bytes) is written as zeros and nothing of it is
 * read), writes every byte of dst and nothing else.  Argument errors (null pointers, a side outside 1..PR_RESIZE_MAX_SIDE, an
 * unknown chroma, only some of the downscale's arguments, a mode that is not the one of these sizes, F < 0, data_bytes < 0)
 * return PR_ERR_INVALID by name before any device work; F = 0 returns PR_OK.  Asynchronous on `stream`, no allocation, no
 * copy, no synchronisation (capturable). */
typedef struct pr_yuv_args {
  const uint8_t* data;
  const int64_t* offsets;
  uint8_t* dst;
  const int32_t* xofs;
  const int16_t* xcoef;
  const int32_t* yofs;
  const int16_t* ycoef;
  int64_t data_bytes;
  pr_yuv_coeffs plan;
  int F, H, W;
  int chroma;
  int bgr;
  int h, w, mode;
} pr_yuv_args;
int pr_yuv_frames(const pr_yuv_args* args, void* stream);

/* ------------------------------------------------------------------------------------ */
/* j7  u8[F,H,W,3] on the device -> the bytes of a YUV4MPEG2 stream: the colour matrix,   */
/*     chroma subsampling and the FRAME headers in one kernel                              */
/* replaces: cv2.VideoWriter in lib/core/base.py:301 for any codec an encoder can read    */
/*           from a pipe (`ffmpeg -f yuv4mpegpipe -i - -c:v libx264 out.mp4`)              */
/* ------------------------------------------------------------------------------------ */
/* j6 backwards.  The host half (pr_yuv_enc_plan; csrc/y4m_host.cc, no device) makes the matrix integers; the device half
 * (pr_yuv_encode, csrc/yuv_enc.hip) turns RGB frames into the frames of a stream, ready to be written behind a stream header.
 * tests/yuv_enc_ref.py restates this section in numpy.  No ABI bump: functions and structs were added.
 *
 * Stream bytes.  For F frames of a picture out_W x out_H the output is F (6 + frame_bytes) bytes: per frame "FRAME\n", the Y
 *   plane, the U plane, the V plane, with j6's sizes for out_W x out_H (cw = (out_W + 1) / 2 for 420 and 422, ch =
 *   (out_H + 1) / 2 for 420, no chroma planes for mono).  Frames follow one another without padding, so the buffer is a chunk of
 *   a valid stream: pr_y4m_index accepts it.
 * Padding.  out_H is H or H + 1, out_W is W or W + 1 (encoders want even sides).  A position outside the source reads the
 *   nearest source pixel (edge replication), for luma and for every chroma tap.
 * Matrix.  Kr, Kb as in j6.  Limited range: sy = 219 / 255, sc = 224 / 255, yo = 16; full range: sy = sc = 1, yo = 0.
 *   pr_yuv_enc_plan computes in double and rounds to nearest even (rne):
 *     KY = rne(sy 65536)   kyr = rne(Kr sy 65536)   kyb = rne(Kb sy 65536)   kyg = KY - kyr - kyb
 *     kc = rne(sc 32768)   kur = rne(Kr / (2 (1 - Kb)) sc 65536)   kug = kc - kur
 *                          kvb = rne(Kb / (2 (1 - Kr)) sc 65536)   kvg = kc - kvb
 *   (601 limited: 16829, 33039, 6416; 28784; 9714, 19070; 4681, 24103.)  The luma row sums to KY exactly and both chroma rows
 *   to zero: every grey gives U = V = 128 exactly, white Y = 235 (255 in full range), black 16 (0).
 * Samples, in int32, one rounding a sample, the shift arithmetic (floor):
 *     Y = yo + ((kyr R + kyg G + kyb B + 2^15) >> 16)
 *   Chroma from tap sums Rs, Gs, Bs whose weights sum to T, the taps' indices clamped to the padded picture:
 *     444        the pixel itself                                                     T = 1
 *     420jpeg    the 2 x 2 block (rows 2 j, 2 j + 1, columns 2 i, 2 i + 1), 1 each      T = 4
 *     422        columns 2 i - 1, 2 i, 2 i + 1 of the row, weights 1, 2, 1             T = 4
 *     420mpeg2   those three columns on rows 2 j and 2 j + 1                           T = 8
 *     U = clamp8(128 + ((kc Bs - kur Rs - kug Gs + T 2^15) >> (16 + log2 T)))
 *     V = clamp8(128 + ((kc Rs - kvg Gs - kvb Bs + T 2^15) >> (16 + log2 T)))
 *   No sum exceeds 7e7 in magnitude.  bgr != 0: the input's first channel is B.
 * Accuracy (tests/test_y4m_write_cpu.py, over all 2^24 colours): every sample lies within 0.51 of the float64 evaluation of
 *   the same taps and the exact matrix.  A 444 round trip through j6 (pr_yuv_frames, same matrix and range) returns every colour
 *   within 1 level in full range; in limited range within 1 level for R and G and within 2 for B.  For the subsampled layouts
 *   that holds for flat-colour frames (the subsampling is then the identity); nothing more is promised for them.  These are
 *   this project's own bits; swscale's are not promised. */
typedef struct pr_yuv_enc_coeffs { /* pr_yuv_enc_plan's integers */
  int32_t kyr, kyg, kyb;
  int32_t kc;
  int32_t kur, kug;
  int32_t kvb, kvg;
  int32_t yo;
} pr_yuv_enc_coeffs;

/* Fills *plan_host for matrix PR_YUV_601 | PR_YUV_709 and full_range 0 | 1; PR_ERR_INVALID by name for anything else or a null
 * pointer, before anything is written.  No device call. */
int pr_yuv_enc_plan(int matrix, int full_range, pr_yuv_enc_coeffs* plan_host);

/* Device pointers: src u8[F,H,W,3] (any alignment), dst u8[F (6 + frame_bytes)] (any alignment: the call's output is one flat
 * run written in aligned dwords, with byte stores only for the up to three bytes at either end; a dword may hold the tail of
 * V, a FRAME header and the next frame's first Y samples).  plan: pr_yuv_enc_plan's integers, by value; chroma: PR_Y4M_C*.
 * Reads only src, writes every byte of dst and nothing else.  Argument errors (null pointers, a side outside
 * 1..PR_RESIZE_MAX_SIDE, out_H - H or out_W - W outside 0..1, an unknown chroma, F < 0, more bytes than a grid of 2^31 - 1
 * blocks writes) return PR_ERR_INVALID by name before any device work; F = 0 returns PR_OK.  Asynchronous on `stream`, no
 * allocation, no copy, no synchronisation (capturable). */
typedef struct pr_yuv_enc_args {
  const uint8_t* src;
  uint8_t* dst;
  pr_yuv_enc_coeffs plan;
  int F, H, W;
  int out_H, out_W;
  int chroma;
  int bgr;
} pr_yuv_enc_args;
int pr_yuv_encode(const pr_yuv_enc_args* args, void* stream);

/* ------------------------------------------------------------------------------------ */
/* j8  person detector: YOLOv3 (Darknet-53 + three heads) and its post-processing          */
/* replaces: the detector half of multi_person_tracker's MPT(...)(image_folder),           */
/*           lib/core/base.py:38-46,59 (detector_type='yolo', yolo_img_size=416,            */
/*           detection_threshold=0.1); the SORT half is host Python (sort.py)               */
/* ------------------------------------------------------------------------------------ */
/* multi_person_tracker and its `yolov3` package are cloned by the reference at install time and are NOT part of the reference
 * tree: nothing pins their bits.  Everything in this section is this project's own contract, modelled on them; a choice marked
 * [unpinned] was taken from memory of the upstream code, not from a file that can be compared.  No ABI bump: functions were added
 * (j3's precedent).
 *
 * Network.  The fixed topology of darknet's yolov3.cfg: 107 layers (0..106), 75 convolutions, 23 shortcuts, routes -4 | -1,61 |
 *   -4 | -1,36, two nearest x2 upsamples, heads at layers 82 / 94 / 106 with strides 32 / 16 / 8.  Every convolution but the three
 *   255-channel head layers is conv (no bias) + BatchNorm + leaky ReLU of slope 0.1 (v > 0 ? v : 0.1f * v); the head layers are
 *   conv + bias, linear.  Padding is k / 2.  A shortcut adds AFTER the activation and applies none to the sum:
 *   y = leaky(conv + b) + res, evaluated in that order in fp32.  Head channel = anchor * 85 + (x, y, w, h, obj, 80 classes).
 *   The input is S_h x S_w, each a multiple of 32 (default 416 x 416, the reference's yolo_img_size).  fp32 on
 *   v_mfma_f32_32x32x2_f32 by default (this paragraph and the next two), or bf16 (paragraph "bf16" below); activations NHWC.
 * Weights.  weights_host is the float body of a darknet weight file, unchanged (62 001 757 floats for the 80-class network): per
 *   BatchNorm convolution beta[O], gamma[O], running mean[O], running var[O], then the weights OIHW; per head convolution
 *   bias[255], then the weights OIHW.  BatchNorm is folded in float64: scale = gamma / sqrt(var + bn_eps), w' = (float)(w *
 *   scale), b' = (float)(beta - mean * scale).  bn_eps is an argument; the value to pass for weights used with the PyTorch port
 *   is 1e-5 (nn.BatchNorm2d's default [unpinned]); darknet itself uses 1e-6.
 * Packed layout (pr_det_fold_pack; what the kernel reads): per convolution bias f32[cout_pad], then w f32[cout_pad][kpad] with
 *   k = (kh * ksize + kw) * cin_pad + ci, zero where padded; cin_pad = cin rounded up to 4, cout_pad = cout rounded up to 64,
 *   kpad = ksize^2 * cin_pad rounded up to 32.
 *
 * bf16.  A second precision beside fp32 (pr_det_create_p, precision = 1); fp32 stays the default and keeps its bits.
 *   Weights: BatchNorm is folded in float64 exactly as above, giving w' and b' as float.  For every convolution but layer 0, w' is
 *   then rounded to bfloat16, round to nearest even, as an integer operation on the float's bits (NaN stays NaN; past the
 *   largest bf16 becomes infinity, as the device conversion does); the bias stays fp32.  Packed layout
 *   (pr_det_fold_pack_bf16) per convolution: bias f32[cout_pad], then w bf16[cout_pad][kpad] (layer 0: w f32[cout_pad][kpad],
 *   as above); k, cin_pad, cout_pad and kpad by the rules above, counted in elements (every Cin of the network but layer 0's is a
 *   multiple of 32: nothing is padded in k).  A convolution's bias begins at the sum of the sizes of the convolutions in front of
 *   it, in BYTES, which is a multiple of 16.
 *   Layer 0 (3 x 3, 4 -> 32, on the fp32 letterbox) is computed exactly as in fp32 -- fp32 operands and weights on
 *   v_mfma_f32_32x32x2_f32 -- and only its output is rounded to bf16 when stored: u8 / 255 is not representable in 8 mantissa
 *   bits, K = 36 does not fit the bf16 loader, and the layer is 0.6 % of the FLOP.  pr_det_letterbox is unchanged.
 *   Every other convolution takes bf16 operands on v_mfma_f32_32x32x16_bf16 and accumulates in fp32 in one fixed k order per
 *   output, independent of B.  Epilogue in fp32, never fused: v = leaky(acc + b); where a shortcut follows, v = v + (float)res;
 *   then v is rounded to bf16 ONCE.  A shortcut's tensor is bf16(leaky(acc + b) + res), not the sum of two rounded values;
 *   pr_det_network_until on the convolution in front of a shortcut gives bf16(leaky(acc + b)).
 *   The three head convolutions (81, 93, 105) read bf16 and write fp32, linear, un-rounded: pr_det_postprocess, the decode in
 *   float64, ranking, NMS and the map back to the frame are the same code for both precisions.
 *   Routes, upsamples and yolo layers move bf16 bits unchanged. */
#define PR_DET_NUM_LAYERS 107
#define PR_DET_MAX_CAND 1024   /* candidates that take part in NMS, per frame */
enum { PR_DET_CONV = 0, PR_DET_SHORTCUT = 1, PR_DET_ROUTE = 2, PR_DET_UPSAMPLE = 3, PR_DET_YOLO = 4 };
enum { PR_DET_STATUS_CAND_OVERFLOW = 1, /* more than PR_DET_MAX_CAND candidates: the best PR_DET_MAX_CAND took part */
       PR_DET_STATUS_DET_OVERFLOW = 2,  /* more than max_det boxes survived NMS: the best max_det were written */
       PR_DET_STATUS_NONFINITE = 4      /* a head value that is not finite took a cell out (paragraph "Non-finite head values") */ };
typedef struct pr_det_layer {
  int32_t type;           /* PR_DET_* */
  int32_t cin, cout;      /* channels in and out, unpadded (a route's: the sum of its sources) */
  int32_t ksize, stride;  /* convolution; upsample: stride 2 */
  int32_t bn;             /* convolution: 1 = BatchNorm + leaky 0.1, 0 = bias, linear */
  int32_t from0, from1;   /* ABSOLUTE layer indices, -1 = none.  shortcut: the layer added to the one in front; route: its sources */
  int32_t down;           /* the output grid is (S_h / down) x (S_w / down) */
  int32_t cin_pad, cout_pad, kpad;
  int64_t weight_offset;  /* convolution: floats into the darknet body where its parameters begin, else -1 */
  int64_t pack_offset;    /* convolution: floats into the packed blob where its bias begins, else -1 */
} pr_det_layer;

/* Host only, no device call (csrc/det_host.cc).  The first n_layers (1..107) of the table; a truncated table folds and packs
 * like the whole one.  pr_det_weight_floats / pr_det_packed_floats: the darknet floats the first n_layers read and the floats
 * they pack to (0 for n_layers outside 1..107).  pr_det_fold_pack refuses by name a null pointer, a count that is not exactly
 * those, and bn_eps outside (0, 1). */
int pr_det_topology(int n_layers, pr_det_layer* layers_host);
size_t pr_det_weight_floats(int n_layers);
size_t pr_det_packed_floats(int n_layers);
int pr_det_fold_pack(int n_layers, const float* weights_host, size_t n_floats, double bn_eps, float* packed_host,
                     size_t packed_floats);
/* The bf16 layout (paragraph "bf16" above): its size in bytes (0 for n_layers outside 1..107) and the fold; the same refusals by
 * name, with packed_bytes in place of packed_floats.  packed_host needs no alignment. */
size_t pr_det_packed_bytes_bf16(int n_layers);
int pr_det_fold_pack_bf16(int n_layers, const float* weights_host, size_t n_floats, double bn_eps, void* packed_host,
                          size_t packed_bytes);

/* Handle.  pr_det_create folds, packs and uploads the weights and allocates every activation buffer for max_batch frames of
 * S_h x S_w (through the internal fence where POSERISK_FENCE is set; every tensor stays below 2 GiB, else PR_ERR_INVALID), the
 * candidate list of the post-processing and the input canvas of pr_det_detect; n_floats must be
 * pr_det_weight_floats(107).  Allocates, copies, synchronises: refused under a declared stream capture, like the other
 * handles' create and destroy.  (max_det, an argument of pr_det_postprocess / pr_det_detect, is the capacity of their outputs:
 * 1..PR_DET_MAX_CAND.)  Queries: pr_det_input_size, pr_det_max_batch, pr_det_grid (the grid of layer `layer`'s output and its channels). */
typedef struct pr_det pr_det_t;
int pr_det_create(int device, const float* weights_host, size_t n_floats, int S_h, int S_w, int max_batch, double bn_eps,
                  pr_det_t** out);
/* pr_det_create_p: the same with a precision: 0 = fp32 (what pr_det_create passes), 1 = bf16 (paragraph "bf16": activation
 * buffers of 2-byte elements, the head tensors' of 4); anything else is refused by name.  pr_det_precision: the handle's (-1 for
 * NULL).  pr_det_elem_bytes: bytes of one element of layer `layer`'s output, as pr_det_network_until writes it: 4, or on a bf16
 * handle 2 for every layer but 81, 82, 93, 94, 105 and 106 (0 for NULL or a layer outside 0..106). */
int pr_det_create_p(int device, const float* weights_host, size_t n_floats, int S_h, int S_w, int max_batch, double bn_eps,
                    int precision, pr_det_t** out);
int pr_det_precision(const pr_det_t* h);
int pr_det_elem_bytes(const pr_det_t* h, int layer);
int pr_det_destroy(pr_det_t* h);
int pr_det_input_size(const pr_det_t* h, int* S_h, int* S_w);
int pr_det_max_batch(const pr_det_t* h);
int pr_det_grid(const pr_det_t* h, int layer, int* gh, int* gw, int* channels);

/* The device entries below are asynchronous on `stream`, allocate nothing, copy nothing to or from the host and do not
 * synchronise (capturable); each refuses its arguments by name (PR_ERR_INVALID; B above max_batch: PR_ERR_CAPACITY) before any
 * device work; B = 0 returns PR_OK.
 *
 * pr_det_letterbox: frames_dev u8[B,H,W,3] (RGB, or BGR with bgr != 0) -> x_dev f32[B,S_h,S_w,4], channels R, G, B, 0.
 *   Sizes, all in integers: with the tighter axis chosen by W * S_h >= H * S_w (the width binds) or not (the height binds),
 *     width binds:   w' = S_w,  h' = min(S_h, max(1, (2 * H * S_w + W) / (2 * W)))        round_half_up(H * S_w / W)
 *     height binds:  h' = S_h,  w' = min(S_w, max(1, (2 * W * S_h + H) / (2 * H)))        round_half_up(W * S_h / H)
 *   i.e. w' = min(S_w, max(1, round_half_up(W r))), h' likewise, r = min(S_w / W, S_h / H) as an exact fraction (a frame smaller
 *   than the input is enlarged) [unpinned: the upstream letterbox rounds W r in floating point].
 *   The h' x w' image is exactly pr_resize_frames' output with pr_resize_plan(H, W, h', w')'s tables and mode (section j3; the
 *   kernel evaluates the same tap expressions per pixel: the position as a double product and a double difference rounded
 *   separately, to float once).  It lies at ox = (S_w - w') / 2, oy = (S_h - h') / 2 (floor) on a canvas of 128; every value is
 *   (float)u8 * (1.f / 255.f).  H, W in 1..PR_RESIZE_MAX_SIDE.
 *
 * pr_det_network: x_dev f32[B,S_h,S_w,4] -> the three head tensors head{32,16,8}_dev f32[B,gh,gw,255], gh = S_h / stride.
 * pr_det_network_until: the output of layer `layer` (0..106) as act_dev f32[B,gh,gw,C] (pr_det_grid): a convolution's (with its
 *   activation, without the shortcut behind it), a shortcut's sum, an upsample's, a route's concatenation (sources in the
 *   route's order), a yolo layer's = the head convolution's output unchanged.  (pr_hmr_encode_until's precedent.)  On a bf16
 *   handle act_dev holds bf16 bits, or fp32 for layers 81, 82, 93, 94, 105 and 106 (pr_det_elem_bytes); pr_det_network's and
 *   pr_det_postprocess' head tensors are fp32 on both.
 *
 * pr_det_postprocess: the three head tensors -> per frame at most max_det person boxes: boxes_dev f32[B,max_det,4] (x1, y1, x2,
 *   y2 in letterbox pixels), scores_dev f32[B,max_det], count_dev i32[B], status_dev i32[B] (PR_DET_STATUS_* bits); rows
 *   beyond count are zero.
 *   Decode, per cell (head, anchor a, row cy, column cx), each expression in float64 on the fp32 head values and rounded to fp32
 *   once, sigma(t) = 1 / (1 + exp(-t)):
 *     bx = (sigma(tx) + cx) * stride   by = (sigma(ty) + cy) * stride   bw = anchor_w * exp(tw)   bh = anchor_h * exp(th)
 *     obj = sigma(to)   score = sigma(to) * sigma(tc0)
 *   anchors (pixels) (10,13) (16,30) (33,23) (30,61) (62,45) (59,119) (116,90) (156,198) (373,326), masks 6-8 / 3-5 / 0-2 for
 *   strides 32 / 16 / 8.  A cell is a candidate iff obj >= conf_thres (obj as fp32, conf_thres as given) and the largest of its
 *   80 class values tc (the lowest index on ties; sigma is monotonic, the values themselves are compared) is class 0.
 *   Order: score descending (as fp32), then the flat index ((head 32, 16, 8) / anchor / cy / cx, cx fastest) ascending; frames
 *   are independent.  The first PR_DET_MAX_CAND take part; more set PR_DET_STATUS_CAND_OVERFLOW.
 *   Box corners, fp32: x1 = bx - 0.5f * bw, x2 = bx + 0.5f * bw, y alike (a product, then a sum; never fused).
 *   Greedy NMS in that order: a candidate is dropped iff an earlier KEPT one has IoU > nms_thres with it.  IoU in fp32, each
 *   operation rounded, never fused, on continuous coordinates:
 *     iw = max(min(ax2, bx2) - max(ax1, bx1), 0)   ih alike   inter = iw * ih
 *     area = (x2 - x1) * (y2 - y1)                  IoU = inter / ((area_a + area_b) - inter)      (0 / 0 counts as no overlap)
 *   Class-agnostic by construction: only class 0 is kept [unpinned: upstream runs NMS per class over all 80].
 *   Non-finite head values.  The frame's status gets PR_DET_STATUS_NONFINITE where a cell's objectness logit to is NaN, or where
 *   a cell passes the candidate test above and its fp32 score or any of its four fp32 corners is not finite (NaN or +-inf: a
 *   NaN tx, ty or tc0, an infinite tw, a tw whose box overflows fp32 only).  Such a cell is never a candidate: it takes no part in
 *   the order or in NMS and does not count towards PR_DET_MAX_CAND, so every candidate's score and corners are finite.  A NaN
 *   among the other 79 class values never beats class 0: the test is "no c in 1..79 has tc[c] > tc[0]", false for every
 *   comparison with a NaN, and sets no bit.
 *
 * pr_det_detect: frames_dev u8[B,H,W,3] -> letterbox, network, post-processing as above, then each box mapped to the frame:
 *   x = (x_letterbox - ox) / (w' / W) evaluated as (x - (float)ox) * ((float)W / (float)w'), y alike with (float)H / (float)h',
 *   then clipped to [0, W] and [0, H]: the scale actually used per axis.  Outputs as pr_det_postprocess'.
 * pr_det_unmap: that map alone, in place and without a handle (the same launcher pr_det_detect calls; what the tests compare
 *   bit for bit): boxes_dev f32[B,max_det,4] in letterbox pixels of an S_h x S_w input (ox, oy, w', h' by pr_det_letterbox's
 *   rule for H x W frames) -> frame pixels, for the rows below count_dev[b]; a row at or beyond count_dev[b] is left as it is.
 *   B in 0..4096, max_det in 1..PR_DET_MAX_CAND, H and W in 1..PR_RESIZE_MAX_SIDE, S_h and S_w multiples of 32 in 32..4096. */
/* The detector's convolution alone (csrc/det_conv.hip; parity tests and timing against pr_conv2d_nhwc): x_dev f32[B,H,W,Cin]
 * (Cin a multiple of 4), packed_dev = ONE convolution in the packed layout above (bias f32[cout_pad], then w
 * f32[cout_pad][kpad], folded by the caller), res_dev f32[B,Ho,Wo,Cout] or NULL (added after the activation) -> y_dev
 * f32[B,Ho,Wo,Cout] = leaky(conv + b) [+ res] (leaky = 0: linear); ksize 1 | 3, stride 1 | 2, padding ksize / 2, any Cout.  All
 * device pointers; asynchronous, no allocation (capturable); refusals by name, a tensor of 2 GiB or more included. */
int pr_det_conv_nhwc(const float* x_dev, const float* packed_dev, const float* res_dev, float* y_dev, int B, int H, int W, int Cin,
                     int Cout, int ksize, int stride, int leaky, void* stream);
/* The bf16 convolution alone (csrc/det_conv_bf16.hip): x_dev bf16[B,H,W,Cin] (Cin a multiple of 8), packed_dev = ONE
 * convolution as bias f32[cout_pad], then w bf16[cout_pad][kpad], res_dev bf16[B,Ho,Wo,Cout] or NULL -> y_dev bf16[B,Ho,Wo,Cout],
 * or f32 with out_f32 != 0, = round(leaky(acc + b) [+ (float)res]), rounded once (not at all for f32).  Otherwise as above. */
int pr_det_conv_nhwc_bf16(const void* x_dev, const void* packed_dev, const void* res_dev, void* y_dev, int B, int H, int W, int Cin,
                          int Cout, int ksize, int stride, int leaky, int out_f32, void* stream);
int pr_det_letterbox(pr_det_t* h, const uint8_t* frames_dev, int B, int H, int W, int bgr, float* x_dev, void* stream);
int pr_det_network(pr_det_t* h, const float* x_dev, int B, float* head32_dev, float* head16_dev, float* head8_dev, void* stream);
int pr_det_network_until(pr_det_t* h, const float* x_dev, int B, int layer, void* act_dev, void* stream);
int pr_det_postprocess(pr_det_t* h, const float* head32_dev, const float* head16_dev, const float* head8_dev, int B,
                       float conf_thres, float nms_thres, int max_det, float* boxes_dev, float* scores_dev, int32_t* count_dev,
                       int32_t* status_dev, void* stream);
int pr_det_detect(pr_det_t* h, const uint8_t* frames_dev, int B, int H, int W, int bgr, float conf_thres, float nms_thres,
                  int max_det, float* boxes_dev, float* scores_dev, int32_t* count_dev, int32_t* status_dev, void* stream);
int pr_det_unmap(float* boxes_dev, const int32_t* count_dev, int B, int max_det, int H, int W, int S_h, int S_w, void* stream);

/* ------------------------------------------------------------------------------------ */
/* s1  temporal smoothing of each track's poses (csrc/smooth.hip; ABI 16: added, nothing changed) */
/* precedent: the reference's median-then-Gaussian recipe for boxes, lib/utils/smooth_bbox.py:106-121, moved to rotations */
/* ------------------------------------------------------------------------------------ */
/* The rows of all tracks lie end to end: rotmat f32[N,24,3,3], optionally betas f32[N,10] and cam f32[N,3], frame_no i32[N]
 * on the device; track t owns the rows track_start[t] .. track_start[t + 1] - 1 (track_start int[T + 1], a HOST array, read
 * before the call returns; 0 = s_0 <= s_1 <= ... <= s_T = N or the call is refused).  tests/smooth_ref.py restates all of
 * this in float64 numpy.
 *
 * Parameters: median_radius m in 0..15, sigma >= 0 and finite, g = min(ceil(3 sigma), 15); anything else is refused.  m = 0
 * skips stage 1, sigma = 0 skips stage 2, with both 0 the outputs hold the inputs' bits.  The unit is frames.
 *
 * Groups: one vector per row -- each of the 24 joints (9 floats), cam (3), betas (10); every group is filtered on its own.
 * Window of row i with radius r: the rows k of the same track with |k - i| <= r and |frame_no[k] - frame_no[i]| <= r (the
 * difference taken in 64 bits).  It is defined on frame numbers, so a gap in a track shrinks it; it never crosses a track
 * boundary, holds row i itself, and is well defined and memory-safe for ANY frame_no content: no global address is formed
 * outside rows i - 15 .. i + 15 clamped to the track.
 *
 * Stage 1, medoid, radius m: cost_k = sum over the window's members l, ascending, self term included, of ||x_k - x_l||_2 --
 * each difference, the sum of squares in element order and the square root in float64, each operation rounded on its own
 * (never fused) -- and the output is x_k* with the smallest cost; exact ties go to the smaller |frame_no[k] - frame_no[i]|,
 * then to the smaller k.  The output holds an input row's bits.  (A one-float group's medoid is its median.)
 *
 * Stage 2, Gaussian, radius g, on stage 1's outputs y: w_k = exp(-(frame_no[k] - frame_no[i])^2 / (2 sigma^2)) in float64
 * (1 where the two frame numbers are equal, whatever sigma^2 rounds to).
 *   a window whose only member is row i itself (an isolated row): the output is y_i's bits, for every group.
 *   cam, betas: sum(w y) / sum(w) per element in float64, members ascending, rounded to f32 once.
 *   a joint: A = sum w_k Y_k (not normalised: what follows is invariant to A's scale), c = det(A) / (||A||_F / sqrt 3)^3
 *     (1 when all members agree).  c >= 0.05: the output is the rotation nearest A in Frobenius norm, the orthogonal polar
 *     factor of A (U diag(1, 1, det(U V^T)) V^T of its SVD; the kernel iterates the scaled Newton step X <- (mu X + X^-T / mu) / 2,
 *     mu = |det X|^(-1/3), from A / (||A||_F / sqrt 3) in float64), rounded to f32 once: every entry within 2^-24 of the
 *     float64 reference.  c >= 0.05 implies s2 + s3 >= 0.196 s1 for A's singular values, so det(A) > 0, the factor is a
 *     proper rotation and the iteration is well conditioned.
 *     c < 0.05 (or not a number): the joint's output is y_i, stage 1's output for the row itself, and bit j of status[i] is set.
 *
 * Non-finite values.  Membership is decided on rows and frame numbers alone, and a row that is no member of a window (another
 * track's, one beyond a gap) is never read into any result of that window: a NaN or an inf stays inside the windows that
 * hold its row.  Stage 1: a cost that is NaN (any member's group holds a NaN, or the candidate's own holds an inf) is never
 * smaller than anything, nothing is smaller than it and it equals nothing: with a NaN on either side the member found first
 * stays; a window whose
 * every cost is NaN yields its FIRST member in row order (not the nearest frame: no tie is exact).  Stage 2: a NaN or an inf
 * among a joint's members makes c not a number, so the joint falls back to y_i (itself possibly non-finite) and sets its
 * status bit; cam and betas have no fallback and propagate it (sum(w y) / sum(w) is NaN, or the inf where no weight is 0).
 * An isolated row still comes back as y_i's bits, status 0.
 *
 * status_dev i32[N] or NULL: bits 0..23 as above, else 0.  outputs->replaced i32[N] or NULL: bit j (joints 0..23; 24 = cam,
 * 25 = betas) is set where stage 1 chose another row than i itself, else 0.
 * outputs->betas / ->cam are required exactly where inputs->betas / ->cam are given.  No output, status, replaced or the
 * workspace may be the same pointer as an input or as each other.  workspace_dev: pr_smooth_workspace_bytes(N, has_betas,
 * has_cam) bytes (stage 1's outputs), needed only when both stages run, else it may be NULL.
 *
 * Two launches on `stream` per PR_SMOOTH_TRACKS_PER_LAUNCH tracks (their bounds travel in the kernel's arguments: no copy
 * to the device): stage 1 into the workspace, stage 2 out of it.  A workgroup takes pr_smooth_tile_rows() consecutive rows
 * (counted from the first row of its PR_SMOOTH_TRACKS_PER_LAUNCH tracks, i.e. from row 0 for T up to that many) and stages
 * them with their halo in LDS once.  Asynchronous, no allocation, no copy, no synchronisation (capturable).  Argument errors
 * return PR_ERR_INVALID by name before any device work; N = 0 (with T >= 0 and all starts 0) returns PR_OK. */
#define PR_SMOOTH_MAX_RADIUS 15
#define PR_SMOOTH_TRACKS_PER_LAUNCH 256
typedef struct pr_smooth_params {
  int32_t median_radius; /* m */
  int32_t reserved;      /* 0 */
  double sigma;
} pr_smooth_params;
typedef struct pr_smooth_inputs {
  const float* rotmat; /* f32[N,24,3,3] */
  const float* betas;  /* f32[N,10] or NULL */
  const float* cam;    /* f32[N,3] or NULL */
} pr_smooth_inputs;
typedef struct pr_smooth_outputs {
  float* rotmat;
  float* betas;
  float* cam;
  int32_t* replaced; /* i32[N] or NULL */
} pr_smooth_outputs;
int pr_smooth_tile_rows(void);
size_t pr_smooth_workspace_bytes(int N, int has_betas, int has_cam); /* 0 for N < 0 */
int pr_smooth_tracks(const pr_smooth_params* params, const pr_smooth_inputs* inputs, const int32_t* frame_no_dev,
                     const int* track_start_host, int T, int N, const pr_smooth_outputs* outputs, int32_t* status_dev,
                     void* workspace_dev, void* stream);

/* ------------------------------------------------------------------------------------ */
/* t1  REBA's activity score and RULA's muscle use from each track's motion (csrc/activity.hip; ABI 16: added, nothing changed) */
/* extends: add_info["REBA"]["Activity_Score"] lib/utils/reba.py:69 and add_info["RULA"]["A_Muscle_use_L" / "_R", "B_Muscle_use"] */
/*          lib/utils/rula.py:75-81, constants of the information file in the reference, which never looks at time */
/* ------------------------------------------------------------------------------------ */
/* Rows and tracks as in s1: rotmat f32[N,24,3,3] and frame_no i32[N] on the device, track_start int[T + 1] on the HOST with
 * s1's rules and refusals.  Every output is an integer and every comparison is made on a float64 value that
 * tests/activity_ref.py (numpy) reproduces bit for bit: there is no tolerance anywhere.
 *
 * Parameters (pr_activity_params): hold_frames H in 1..PR_ACTIVITY_MAX_HOLD, rapid_frames R in 1..H, gap_frames G >= 1,
 * rep_events E >= 0; dot_static, dot_move, dot_rapid finite and in [-1, 3]: the thresholds 1 + 2 cos(angle), which the caller
 * computes once (poserisk_release_amd/activity.py::thresholds); no kernel calls a trigonometric function.  Anything else is
 * refused by name before any device work.
 *
 * Scored joints, bit b = 0..11: Torso 3, Neck 12, L_Knee 4, R_Knee 5, L_Thorax 13, L_Shoulder 16, L_Elbow 18, L_Wrist 20,
 * R_Thorax 14, R_Shoulder 17, R_Elbow 19, R_Wrist 21 (the joints the rules read).  Masks: B = bits 0..3, L = bits 4..7,
 * R = bits 8..11.
 *
 * dot_b(k, i) = sum over e = 0..8, ascending, of (double)R_k[e] * (double)R_i[e], R_k the 9 floats of joint b in row k: the
 * trace of R_k^T R_i = 1 + 2 cos(theta).  The product of two floats is exact in float64, so a fused multiply-add and a
 * multiply followed by an add round alike and the library's -ffp-contract setting cannot change a bit of it.
 *
 * Window W_i(L): the rows k of row i's track with k <= i, i - k <= L and 0 <= frame_no[i] - frame_no[k] <= L (differences in
 * 64 bits).  Like s1's it is defined and memory-safe for ANY frame_no content: no address is formed outside rows
 * i - L .. i + L clamped to the track (a workgroup's addresses lie in the union of these ranges over its rows).
 *
 * Stage A, events; sequential by definition, per track and joint.  The anchor starts at the track's first row.  For each
 * further row k, ascending: if frame_no[k] - frame_no[k - 1] > G or < 0 the anchor becomes k and no event is recorded; else
 * if dot_b(anchor, k) < dot_move, bit b of moved[k] is set and the anchor becomes k.
 *
 * Stage B, per row i and joint b.  p = the first (lowest) row of W_i(H).  covered_i: frame_no[i] - frame_no[p] > H - G and
 * every two rows that follow each other in W_i(H) differ by 1..G frames.
 *   held     = covered_i and dot_b(k, i) >= dot_static for every k in W_i(H)
 *   repeated = covered_i and (the number of k in W_i(H) with bit b of moved[k] set) > E
 *   rapid    = dot_b(k, i) < dot_rapid for some k in W_i(R)
 * The comparisons are written exactly so: a NaN makes each of them false.
 *
 * Stage C, spread: the final held and repeated bits of row i are the OR of stage B's over the rows e of the same track with
 * e >= i, e - i <= H and 0 <= frame_no[e] - frame_no[i] <= H: the whole held minute is marked, not only its end.  rapid is
 * not spread.
 *
 * Outputs (device): flags i32[N,4] = the held, repeated, rapid and moved masks; adds i32[N,4] =
 *   reba_activity = (held != 0) + (repeated != 0) + (rapid != 0),   a_muscle_l = ((held | repeated) & L) != 0,
 *   a_muscle_r = ((held | repeated) & R) != 0,                      b_muscle = ((held | repeated) & B) != 0.
 * workspace_dev: pr_activity_workspace_bytes(N) bytes, 4-byte aligned (stage A's and stage B's masks).  No pointer may be
 * the same as another.
 *
 * Three launches on `stream` per PR_ACTIVITY_TRACKS_PER_LAUNCH tracks (their bounds travel in the kernels' arguments).
 * Stage A: a workgroup per track, twelve lanes walk the twelve chains through chunks staged in LDS.  Stage B: a workgroup
 * takes pr_activity_tile_rows() consecutive rows (counted from the first row of the launch's tracks) and streams them and the
 * H rows before them through LDS, newest first, in chunks of pr_activity_chunk_rows() rows; it stops where no output of the
 * tile can change any more.  Stage C reads the masks only.  Asynchronous, no allocation, no copy, no synchronisation
 * (capturable).  N = 0 (with T >= 0 and all starts 0) returns PR_OK. */
#define PR_ACTIVITY_MAX_HOLD 16384
#define PR_ACTIVITY_TRACKS_PER_LAUNCH 256
typedef struct pr_activity_params {
  int32_t hold_frames;  /* H */
  int32_t rapid_frames; /* R */
  int32_t gap_frames;   /* G */
  int32_t rep_events;   /* E */
  double dot_static;
  double dot_move;
  double dot_rapid;
} pr_activity_params;
int pr_activity_tile_rows(void);
int pr_activity_chunk_rows(void);
size_t pr_activity_workspace_bytes(int N); /* 0 for N < 0 */
int pr_activity_tracks(const pr_activity_params* params, const float* rotmat_dev, const int32_t* frame_no_dev,
                       const int* track_start_host, int T, int N, int32_t* flags_dev, int32_t* adds_dev, void* workspace_dev,
                       void* stream);

/* The scorers of a12-a13 with per-row addends.  activity_rows_dev i32[N] or NULL: row f's value is added to
 * info->activity where reba.py:69 adds it.  muscle_rows_dev i32[N,3] (a_l, a_r, b) or NULL: row f's values are added to
 * info->a_muscle_l, ->a_muscle_r and ->b_muscle where rula.py:75-81 add them.  With NULL every output is pr_reba's /
 * pr_rula's; the rule bodies exist once (pr_reba and pr_rula are these with NULL). */
int pr_reba_rows(const double* euler_deg_dev, int N, const pr_reba_info* info, const int32_t* activity_rows_dev,
                 int32_t* out_dev, void* stream);
int pr_rula_rows(const double* euler_deg_dev, int N, const pr_rula_info* info, const int32_t* muscle_rows_dev,
                 int32_t* out_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* POSERISK_HIP_H */
