/*
 * aarmvs.h — C ABI of the MI355X (gfx950) depth-sweep library (libaarmvs.so).
 *
 * This is the drop-in boundary beneath the reference's Python API
 * (BuTTerK3ks/AA-RMVSNet, models/drmvsnet.py).  The reference has no native
 * layer: every entry point below replaces a block of PyTorch ops inside
 * EMVSNet.forward's depth loop (models/drmvsnet.py:255-345).  The Python mirror
 * in aa-rmvsnet_amd/models binds these with ctypes.
 *
 * Conventions
 *   - All tensors are fp32, contiguous, NCHW, resident in device memory and owned
 *     by the caller; the library never allocates device memory and keeps no
 *     pointer across calls.
 *   - Every launch goes to the caller's stream; no host synchronisation happens
 *     inside any entry point (graph-capturable).
 *   - Streams and threads.  A call is ordered on `stream` like a kernel: it starts
 *     after everything `stream` held when it was made, and at return all its work
 *     (the library's own streams included: they fork from `stream` and join it
 *     again inside the call) is ordered before whatever is enqueued on `stream`
 *     next.  Calls may be made from several host threads and on several streams
 *     of one device at once, provided each has its own workspace, record, scratch
 *     and state buffers (parameters and inputs may be shared: they are only read).
 *     The library's unit / backward streams and the aux stream are shared per
 *     device: concurrent callers' units are serialised on them, and the results do
 *     not change (every schedule is bit-identical).  The events are per thread (and
 *     device), re-recorded call after call; a wait is bound to the record enqueued
 *     before it, so one thread may alternate between callers' streams.
 *     aarmvs_last_error() is per thread.  aarmvs_profile_* is for one caller at a
 *     time (one global table of events, without a lock).  The pieces of
 *     one sweep's d_range, and the calls of one backward chain, share a workspace:
 *     issue them on one stream, or order them yourself.  With more than four
 *     streams in the process, streams share hardware queues: work on one stream
 *     then also waits for what its queue partner holds (slower, never wrong).
 *     tests/test_gpu_streams.py holds the library to this paragraph.
 *   - Return 0 on success, a nonzero aarmvs_status otherwise; the message is in
 *     aarmvs_last_error() (thread-local).  Shapes are validated before launch.
 *   - Constraints (from the reference's own shape rules): C == 32 feature
 *     channels, H % 4 == 0 and W % 4 == 0 (two 2x2 max-pools and two stride-2
 *     deconvs must round-trip, drmvsnet.py:148-161), 1 <= nsrc <= AARMVS_MAX_SRC.
 */
#ifndef AARMVS_H_
#define AARMVS_H_

#include <stddef.h>
#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AARMVS_MAX_SRC 16
#define AARMVS_FEAT_C 32

typedef enum aarmvs_status {
  AARMVS_OK = 0,
  AARMVS_ERR_INVALID = 1,   /* bad shape / null pointer / unsupported argument */
  AARMVS_ERR_HIP = 2        /* a HIP runtime call or kernel launch failed     */
} aarmvs_status;

const char* aarmvs_last_error(void);
const char* aarmvs_version(void);

/* ---------------------------------------------------------------------------
 * Parameters.
 * The raw blob is the sweep's checkpoint tensors (the 48 omega.* and
 * cost_regularization.* keys of the reference state_dict, drmvsnet.py:66-117 and
 * :27-38) flattened and concatenated in this order:
 *   omega.reweight_network.0.0.weight [4,32,3,3], .0.0.bias [4], .0.1.weight [4],
 *   .0.1.bias [4], .1.stem.0.0.weight [4,4,1,1], .1.stem.0.0.bias [4],
 *   .1.stem.0.1.weight [4], .1.stem.0.1.bias [4], .1.stem.1.weight [4,4,1,1],
 *   .1.stem.1.bias [4], .1.stem.2.weight [4], .1.stem.2.bias [4],
 *   .2.weight [1,4,1,1], .2.bias [1],
 *   cost_regularization.cell_list.{0..4}.conv.{weight,bias}
 *     ([64,48,3,3],[64],[64,32,3,3],[64],[64,32,3,3],[64],[64,48,3,3],[64],[32,40,3,3],[32]),
 *   cost_regularization.deconv_{0,1}.{conv.weight [16,16,3,3], conv.bias [16],
 *     gn.weight [16], gn.bias [16]},
 *   cost_regularization.conv_0.weight [1,8,3,3], cost_regularization.conv_0.bias [1].
 * aarmvs_pack_params rearranges it (on the device) into the kernels' layout.
 * ------------------------------------------------------------------------- */
size_t aarmvs_param_count(void);            /* floats in the raw blob            */
size_t aarmvs_packed_param_bytes(void);     /* bytes of the packed device buffer */
int aarmvs_pack_params(const float* raw_params, void* packed, hipStream_t stream);

/* ---------------------------------------------------------------------------
 * homo_warping_depthwise (models/module.py:6-38): bilinear warp of src_fea
 * [B,C,H,W] into the reference view at one depth per batch element.
 * rel_proj [B,12] = rows 0..2 of src_proj @ inverse(ref_proj) (module.py:16-18),
 * depth [B].  grid_sample semantics: bilinear, zero padding, align_corners=False
 * applied to the align_corners=True-normalised grid.
 * ------------------------------------------------------------------------- */
int aarmvs_homo_warp(const float* src_fea, const float* rel_proj, const float* depth,
                     int B, int C, int H, int W, float* out, hipStream_t stream);

/* Backward of aarmvs_homo_warp w.r.t. src_fea (the grid carries no gradient,
 * module.py:15; grid_sample's backward at module.py:36): grad_src += bilinear
 * scatter of grad_out.  grad_src must be initialised by the caller (zeros for the
 * plain gradient).  The scatter sums are formed in 64-bit fixed point (exponent from
 * max |grad_out|), so the result is bit-reproducible whatever the order the GPU
 * serves the contributions in; a batch element whose grad_out holds a NaN or an
 * infinity is scattered with fp32 atomics instead (the NaN/inf reaches the source
 * pixels grid_sample's backward sends it to, the others stay finite).  Batch
 * elements are processed 64 at a time.  workspace:
 * aarmvs_homo_warp_backward_workspace_bytes = 256 + min(B,64)*C*H*W*8 bytes
 * (caller-owned, device memory). */
size_t aarmvs_homo_warp_backward_workspace_bytes(int B, int C, int H, int W);
int aarmvs_homo_warp_backward(const float* grad_out, const float* rel_proj, const float* depth,
                              int B, int C, int H, int W, float* grad_src, void* workspace,
                              hipStream_t stream);

/* ---------------------------------------------------------------------------
 * Whole depth sweep (drmvsnet.py:273-291 train / :306-342 eval).
 * Replaces, per plane d: homo_warping_depthwise x nsrc, (warp-ref)^2, omega
 * re-weighting, weighted accumulation, UNetConvLSTM.forward and the online WTA.
 * ------------------------------------------------------------------------- */
/* Training record of a sweep (the BPTT's saved tensors; see aarmvs_sweep_backward):
 * when aarmvs_sweep_args.record is set, the sweep keeps every plane's regulariser
 * tensors in these caller-owned device buffers instead of overwriting its workspace copies.
 * Per-plane slab sizes in bytes: aarmvs_train_record_bytes(B, H, W, which) with which =
 *   0 x      [B,H,W,32] cost slice of the plane (NHWC);                 D slabs
 *   1 state  h, c of the five cells (NHWC); slab 0 is the zero initial state
 *            (drmvsnet.py:133-134), slab d+1 the state after plane d;  D+1 slabs
 *   2 z      the five cells' gate pre-activations (conv + bias), per cell planar
 *            [B][hid/4 channel quads][gates i,f,o,g][H*W][4];           D slabs
 *   3 u      the two deconvs' outputs before GroupNorm;                  D slabs
 *   4 stats  the two deconvs' GroupNorm statistics (fp64);               D slabs
 *   5 t1     the omega conv output (4 ch) of ONE source view;        D x nsrc slabs
 *   6 ostats the omega chain's GroupNorm statistics of ONE view (fp64); D x nsrc slabs
 *   (5 and 6 let the backward skip recomputing the omega conv of every plane)
 * ~1 KB per pixel and plane at B = 1 (63 GB for 640x512, D = 192). */
typedef struct aarmvs_train_record {
  float* x;
  float* state;
  float* z;
  float* u;
  double* stats;
  float* t1;
  double* ostats;
} aarmvs_train_record;
size_t aarmvs_train_record_bytes(int B, int H, int W, int which);

typedef struct aarmvs_sweep_args {
  int B, C, H, W;                         /* C must be 32                         */
  int nsrc;                               /* N-1 source views                     */
  int D;                                  /* depth hypotheses (depth_values.shape[1]) */
  int d_begin, d_end;                     /* plane range; d_begin == 0 resets state */
  const float* ref_fea;                   /* [B,C,H,W]                             */
  const float* src_fea[AARMVS_MAX_SRC];   /* nsrc x [B,C,H,W]                      */
  const float* rel_proj;                  /* [nsrc][B][12]                         */
  const float* depth_values;              /* [B,D]                                 */
  const void* packed_params;              /* from aarmvs_pack_params               */
  void* workspace;                        /* aarmvs_sweep_workspace_bytes() bytes  */
  float* depth_out;                       /* [B,H,W] WTA depth, or NULL            */
  float* conf_out;                        /* [B,H,W] max_prob / exp_sum, or NULL   */
  float* cost_out;                        /* [B,D,H,W] regulariser output, or NULL */
  float* slice_out;                       /* debug: [B,32,H,W] last plane's cost slice, or NULL */
  float* omega_out;                       /* debug: [nsrc,B,H,W] last plane's omega weights, or NULL */
  hipStream_t aux_stream;                 /* optional second stream, or NULL: the cost slices
                                             are computed in groups of up to 16 planes, and
                                             the next group's (omega conv, GroupNorm
                                             statistics, cost_x) run on it beside the current
                                             group's regulariser steps (events per group); a
                                             sweep with it also spreads each plane's U-Net
                                             step (five units: cell 0 | cell 1 | cell 2 |
                                             deconv_0, cell 3 | deconv_1, cell 4, head) over
                                             `stream` and library-owned streams, so that the
                                             units of neighbouring planes run at once (events
                                             per unit and plane; at most four streams in all,
                                             and for small frames, B*H*W <= 65536, the cost
                                             stage moves to `stream` so that the units get
                                             four).  At return all work is ordered on
                                             `stream`; results are bit-identical either way */
  const aarmvs_train_record* record;      /* training record, or NULL (eval): the cost
                                             slices and regulariser tensors of the planes
                                             d_begin..d_end-1 go to its slabs           */
  int record_d0;                          /* segment record (see below): the first plane the
                                             record holds; 0: the record starts at plane 0 */
  int record_planes;                      /* planes the record holds; 0: up to plane D      */
} aarmvs_sweep_args;

/* Segment records (plane-segment checkpointing of the BPTT).
 * A record may hold only the planes record_d0 .. record_d0 + n - 1 (n = record_planes, or
 * D - record_d0 when that is 0): slab i of x, z, u, stats, t1 and ostats is then plane
 * record_d0 + i, state slab i the state BEFORE plane record_d0 + i, and the record has n + 1
 * state slabs.  aarmvs_train_segment_bytes gives its size.  A recorded aarmvs_sweep over
 * [d_begin, d_end) inside that range reads its initial state from state slab d_begin -
 * record_d0 (the library zeroes it only when d_begin == 0) and writes the other slabs at their
 * segment-relative places; cost_out stays indexed by the absolute plane.  Such a call does not
 * depend on what an earlier call left in the workspace (it re-makes the feature copies and the
 * fp16 guard bound), except for depth_out / conf_out, whose winner-take-all images are only
 * complete after contiguous calls from plane 0 through one workspace.
 *
 * Training with one S-plane record (S a multiple of 16) instead of a D-plane one:
 *   forward, for each segment [s0, s1) = [0,S), [S,2S), ... in order:
 *     aarmvs_sweep(d_begin = s0, d_end = s1, record_d0 = s0, record_planes = s1 - s0); copy
 *     state slab s1 - s0 out as the checkpoint "state before plane s1", and (unless this was
 *     the last segment) also into state slab 0 for the next segment;
 *   backward, for each segment LAST FIRST, with one `scratch` that nothing else writes between
 *   the calls:
 *     copy the checkpoint "state before plane s0" into state slab 0 and repeat the segment's
 *     recorded aarmvs_sweep (not needed while the record still holds the segment), then
 *     aarmvs_sweep_backward(d_begin = s0, d_end = s1, record_d0 = s0, record_planes = s1 - s0).
 * The backward's 16-plane groups are then the whole backward's, everything it carries from one
 * group to the next (the cells' state gradients, the fp64 parameter accumulators and the
 * cost-slice accumulators) lives in `scratch`, and every reduction has a fixed order: the
 * gradients equal the whole-record backward's bit for bit.
 *
 * The new fields are appended to the existing structs rather than given entry points of their
 * own: a zero-initialised struct keeps its meaning (whole D, record from plane 0), every
 * caller of the old form compiles and behaves as before, and the sweep keeps ONE validated
 * path instead of two that must be kept equal.  The structs carry no size field, so a caller
 * compiled against the shorter structs has to be recompiled with this header; the library and
 * its bindings (aarmvs/_lib.py) are built from one tree. */
int aarmvs_train_segment_bytes(int B, int H, int W, int nsrc, int planes, size_t* record_bytes,
                               size_t* checkpoint_bytes);
/* ^ bytes of a record of `planes` planes (all seven buffers: planes slabs of x, z, u and stats,
 * planes + 1 of state, planes * nsrc of t1 and ostats) and of one checkpoint (one state slab,
 * 264 B per pixel at B = 1); either pointer may be NULL. */

size_t aarmvs_sweep_workspace_bytes(int B, int H, int W, int nsrc);
int aarmvs_sweep(const aarmvs_sweep_args* args, hipStream_t stream);

/* Precision of the regulariser's matrix products in an inference sweep.
 * AARMVS_PREC_SPLIT (the default and the parity mode): every fp32 product of the five ConvLSTM
 * convs and the two transposed convs is three fp16 matrix products with fp32 accumulation
 * (w_hi x_hi + w_hi x_lo + w_lo x_hi, ~2^-21 relative per product).
 * AARMVS_PREC_FP16 (opt-in): one product, w_hi x_hi.  What is rounded: the operands of those
 * seven convs only -- the weights (the hi planes of the same packed buffer) and the staged
 * inputs (cat[x, h] of a cell after the fused max-pool / GroupNorm+ReLU; the deconv's input h)
 * -- each once, to fp16's 11 significant bits, round to nearest even, at the power-of-two
 * scale the split mode stages it at (weights: max|w| 2^e in [2^13, 2^14]; h: 2^12 in the
 * cells, 2^14 in the deconvs; cell 0's cost slice and cells 3 and 4's GroupNorm part: the
 * scale that puts their bound in [2^14, 2^15)), so the fp16 range guards hold as before and the
 * rounding is relative (2^-12 per operand) for all but values 2^-28 below the bound.  What is
 * not: accumulation, bias, gate math, the c and h state, the GroupNorm statistics, the head,
 * the winner-take-all, the omega network and the cost slice all stay fp32 as in the split mode.
 * Workspace size, stream schedule, d_range behaviour and determinism are the split mode's.
 * Inference only: with a training record the call returns AARMVS_ERR_INVALID (the BPTT
 * differentiates the split cells).  Measured errors and speed: DESIGN.md §7. */
typedef enum aarmvs_precision {
  AARMVS_PREC_SPLIT = 0,
  AARMVS_PREC_FP16 = 1
} aarmvs_precision;
/* aarmvs_sweep at a precision (an aarmvs_precision value; anything else: AARMVS_ERR_INVALID).
 * aarmvs_sweep(a, s) is aarmvs_sweep_p(a, AARMVS_PREC_SPLIT, s).  The mode is a parameter of
 * the call, not a field of aarmvs_sweep_args, so the struct keeps its size. */
int aarmvs_sweep_p(const aarmvs_sweep_args* args, int precision, hipStream_t stream);

/* Sub-plane refinement of the sweep's winner-take-all (opt-in, inference only, beyond the
 * reference: the reference keeps the winning plane's depth and max_prob / exp_sum).  Beside the
 * WTA images the head kernel keeps, per pixel, the winner's plane index w (first maximum, the
 * strict < of the WTA; -1 while no plane has won) and p = exp(cost) of the planes w - 1 and
 * w + 1.  With n = the planes processed since plane 0, all in fp32 with every operation rounded
 * on its own:
 *   a pixel is refinable when 1 <= w and w + 1 < n (both neighbours seen); then
 *     s   = (p[w-1] + p[w]) + p[w+1]
 *     num = p[w-1] (d[w-1] - d[w]) + p[w+1] (d[w+1] - d[w])       d[.] = depth_values[b*D + .]
 *     depth_refined = d[w] + num / s                   (any spacing of the depth values)
 *   otherwise (winner on the first or the last plane seen, no winner), or when s or num is not
 *   finite (exp overflow, a NaN cost), depth_refined is the WTA depth image's value, bit for bit;
 *   conf_window = s' / exp_sum, s' = p[w] plus the neighbours that exist (one-sided at the
 *   borders; max_prob / exp_sum with no winner), so conf_window >= the WTA confidence and is NaN
 *   where that is; index = w (int32).
 * state: aarmvs_refine_state_bytes(B, H*W) = 16 B per pixel of caller-owned device memory,
 * 16-byte aligned, (int32 w, float p of the last plane, p[w-1], p[w+1]); plane 0 starts it afresh
 * and it is complete, like the WTA images, only after contiguous calls from plane 0 through one
 * workspace and one state buffer: a sweep split into d_range calls equals the whole sweep.  The
 * outputs ([B,H,W] each, any may be NULL) are written at the end of EVERY call and describe the
 * planes [0, d_end).  The sweep workspace and its layout are unchanged, depth_out / conf_out /
 * cost_out are bit-identical with and without refinement, and the head kernel reads and writes
 * 16 B per pixel and plane more (measured cost: DESIGN.md §8).
 * aarmvs_sweep_r(a, p, NULL, s) is aarmvs_sweep_p(a, p, s).  Both precisions; a NULL state or a
 * training record with refine != NULL: AARMVS_ERR_INVALID. */
typedef struct aarmvs_refine_args {
  void* state;               /* aarmvs_refine_state_bytes(B, H*W) bytes, required */
  float* depth_refined_out;  /* [B,H,W] or NULL */
  float* conf_window_out;    /* [B,H,W] or NULL */
  int* index_out;            /* [B,H,W] int32 or NULL */
} aarmvs_refine_args;
size_t aarmvs_refine_state_bytes(int B, int HW);   /* 16 * B * HW; 0 for B, HW < 1 */
int aarmvs_sweep_r(const aarmvs_sweep_args* args, int precision, const aarmvs_refine_args* refine,
                   hipStream_t stream);

/* Depth-posterior statistics of the sweep (opt-in, inference only, beyond the reference): the
 * moments of the distribution q[d] = p[d] / sum p over the planes, p[d] = exp(cost[d]) -- the
 * softmax the WTA confidence already normalises by -- accumulated online in the head kernel, with
 * no cost volume.  Everything is fp32 and every operation is rounded on its own.  Per pixel the
 * state is (mu, V, E, p2), all zero before plane 0 (never loaded for it).  For plane d, in order,
 * with c the plane's cost, p = expf(c) (the value the WTA forms), x = depth_values[b*D + d],
 * S0 = exp_sum before the plane, S1 = S0 + p (the value the WTA stores), m = max_prob before the
 * plane's select:
 *   runner-up:  if (m < p) p2 = m;  else if (p2 < p) p2 = p;
 *               (a p equal to the maximum is a runner-up: the first maximum wins)
 *   moments, only if (p > 0):
 *     k = p / S1        j = S0 / S1        delta = x - mu
 *     mu <- mu + delta * k
 *     V  <- j * (V + (delta * delta) * k)
 *     E  <- E + (c - E) * k
 * V is rescaled by S0 / S1 and NOT by 1 - k: when a late plane dominates, k rounds to within
 * 2^-24 of 1 and 1 - k keeps no correct digit, which loses the standard deviation completely
 * (DESIGN.md section 9).  After n planes, with S = exp_sum:
 *   if !(S > 0 && isfinite(S)) all four outputs are NaN: every pixel whose WTA confidence is NaN
 *   (0/0, inf/inf, a NaN cost), and a finite max_prob over an overflowed sum;
 *   otherwise depth_mean = mu, depth_std = sqrtf(V), entropy = max(logf(S) - E, 0) in nats,
 *   runner_up = p2 / S.  V >= 0 by construction; it is not clamped.
 * state: aarmvs_posterior_state_bytes(B, H*W) = 16 B per pixel of caller-owned device memory,
 * 16-byte aligned.  Like the WTA images it is complete only after contiguous calls from plane 0
 * through one workspace and one state buffer: a sweep split into d_range calls equals the whole
 * sweep bit for bit.  The outputs ([B,H,W] each, any may be NULL) are written at the end of EVERY
 * call and describe the planes [0, d_end).  The sweep workspace and its layout are unchanged,
 * depth_out / conf_out / cost_out are bit-identical with and without the statistics, and the head
 * kernel reads and writes 16 B per pixel and plane more (measured cost: DESIGN.md section 9).
 * Both precisions; a NULL state or a training record with posterior != NULL:
 * AARMVS_ERR_INVALID (aarmvs_posterior_from_cost serves a cost volume). */
typedef struct aarmvs_posterior_args {
  void* state;           /* aarmvs_posterior_state_bytes(B, H*W) bytes, required */
  float* mean_out;       /* [B,H,W] or NULL: softmax-weighted mean depth (soft argmax) */
  float* std_out;        /* [B,H,W] or NULL: standard deviation of depth under q */
  float* entropy_out;    /* [B,H,W] or NULL: entropy of q in nats */
  float* runner_up_out;  /* [B,H,W] or NULL: the second largest q */
} aarmvs_posterior_args;
size_t aarmvs_posterior_state_bytes(int B, int HW);   /* 16 * B * HW; 0 for B, HW < 1 */

/* The sweep's extensible entry point: the options of a sweep beyond aarmvs_sweep_args.  `size`
 * is the caller's sizeof(aarmvs_sweep_options); any size from the first version's
 * (AARMVS_SWEEP_OPTIONS_SIZE_V1) up to the library's own is accepted and fields beyond it read
 * as zero, so a caller built against an older header keeps working; any other size is
 * AARMVS_ERR_INVALID.  options == NULL is all defaults.  aarmvs_sweep(a, s), aarmvs_sweep_p(a, p,
 * s) and aarmvs_sweep_r(a, p, r, s) are this call with {precision = p, refine = r}. */
typedef struct aarmvs_sweep_options {
  size_t size;                             /* sizeof(aarmvs_sweep_options) of the caller */
  int precision;                           /* aarmvs_precision; 0 = AARMVS_PREC_SPLIT */
  const aarmvs_refine_args* refine;        /* NULL: no sub-plane refinement */
  const aarmvs_posterior_args* posterior;  /* NULL: no posterior statistics */
} aarmvs_sweep_options;
#define AARMVS_SWEEP_OPTIONS_SIZE_V1 (sizeof(size_t) + 2 * sizeof(int) + 2 * sizeof(void*))
int aarmvs_sweep_ex(const aarmvs_sweep_args* args, const aarmvs_sweep_options* options,
                    hipStream_t stream);
/* A stream for aux_stream owned by the library (one per device, created on first use, never
 * destroyed): a process gets four hardware queues and streams beyond four share them, so a
 * caller without streams of its own passes this one rather than creating a fifth (the library's
 * other streams are its two to three unit / backward streams).  *out: the current device's. */
int aarmvs_aux_stream(hipStream_t* out);

/* ---------------------------------------------------------------------------
 * Backward of a training sweep (the BPTT through drmvsnet.py:273-291): given the record
 * of a forward over all D planes (aarmvs_sweep with `record`, d_begin = 0, d_end = D) and
 * dL/dcost [B,D,H,W] (the sweep's cost volume, before the softmax), the gradients w.r.t.
 * the sweep's parameters (raw-blob layout, aarmvs_param_count() floats: the omega.* and
 * cost_regularization.* tensors), the reference features and the source features.
 * Replaces autograd through homo_warping_depthwise, the omega network, the weighted
 * accumulation and UNetConvLSTM.forward (module.py:6-38, 76-92, 252-287; drmvsnet.py:27-38,
 * 119-167); no gradient flows to the projections or depths (module.py:15).
 * Planes are processed last to first in groups of 16.  Parameter gradients are fixed-order
 * fp64 sums (deterministic); grad_ref / grad_src are overwritten (NCHW [B,32,H,W]).
 * grad_x (debug, or NULL): [D][B][H][W][32] dL/dx per plane (the cost slices, NHWC).
 * regulariser_only (debug): skip the cost-slice part (grad_ref / grad_src untouched, the
 * omega.* entries of grad_params zero).  `workspace` is the sweep workspace
 * (aarmvs_sweep_workspace_bytes), `scratch` aarmvs_backward_scratch_bytes bytes.
 * ------------------------------------------------------------------------- */
typedef struct aarmvs_backward_args {
  int B, C, H, W, nsrc, D;
  const float* ref_fea;                   /* [B,C,H,W]                          */
  const float* src_fea[AARMVS_MAX_SRC];   /* nsrc x [B,C,H,W]                   */
  const float* rel_proj;                  /* [nsrc][B][12]                      */
  const float* depth_values;              /* [B,D]                              */
  const void* packed_params;
  const aarmvs_train_record* record;
  const float* grad_cost;                 /* [B,D,H,W]                          */
  float* grad_ref;                        /* [B,C,H,W] out, or NULL             */
  float* grad_src[AARMVS_MAX_SRC];        /* nsrc x [B,C,H,W] out, or NULL      */
  float* grad_params;                     /* [aarmvs_param_count()] out, or NULL */
  float* grad_x;                          /* debug out, or NULL                 */
  void* workspace;
  void* scratch;
  int regulariser_only;
  /* Ranged backward (all zero: the whole backward over [0, D) on a whole record).  The call
   * runs the planes [d_begin, d_end) (d_end == 0 means D) on a record that holds the planes
   * record_d0 .. (see "Segment records" above).  d_begin and d_end must be multiples of 16,
   * except that d_end may equal D.  The calls of one backward come last range first
   * (d_end == D), each range ending where the one before began, down to d_begin == 0, with the
   * same `scratch`, which nothing may write between the calls (the recompute aarmvs_sweep does
   * not take it; the `workspace` may serve that sweep).  The call with d_end == D zeroes the
   * carried state gradients and accumulators; the call with d_begin == 0 writes grad_params,
   * grad_ref and grad_src (the other calls leave them untouched and may pass NULL for them).
   * grad_x and grad_cost stay indexed by the absolute plane.  The library keeps no state of its
   * own between the calls, so their order is the caller's contract and is not checked. */
  int d_begin, d_end;
  int record_d0, record_planes;
} aarmvs_backward_args;
size_t aarmvs_backward_scratch_bytes(int B, int H, int W, int nsrc);
int aarmvs_sweep_backward(const aarmvs_backward_args* args, hipStream_t stream);

/* Hidden state of the regulariser inside the workspace, for inspection/BPTT:
 * cell k in 0..4, which = 0 for h, 1 for c, planes = the number of planes (or
 * aarmvs_unet_step steps) processed so far: the state they left (h lives in a per-cell
 * ring indexed by planes % kHRing[k]: 6, 4, 3, 3 and 2 slots for h0..h4, so that the units of
 * neighbouring planes can run on separate streams.  The rings are part of
 * aarmvs_sweep_workspace_bytes: 572 B per pixel against 264 B for two slots each; at
 * 1600x1184 and B = 1, h0 alone takes about 485 MB more.  Each slot of the h0 and h1 rings
 * also has a quarter-size image of the 2x2 max-pooled h, written by the inference sweep's
 * cells 0 and 1 for cells 1 and 2: 112 B per pixel more, 212 MB at 1600x1184 and B = 1;
 * aarmvs_state_ptr does not expose them).  Valid after an
 * aarmvs_sweep call; returns a device pointer to [B,H_k,W_k,hid_k] (NHWC: the workspace
 * keeps the U-Net tensors channel-innermost) or NULL. */
float* aarmvs_state_ptr(void* workspace, int B, int H, int W, int nsrc, int planes,
                        int cell, int which);

/* ---------------------------------------------------------------------------
 * One UNetConvLSTM step (drmvsnet.py:119-167) on a given cost slice x [B,32,H,W]
 * using the hidden state held in `workspace` (same layout as aarmvs_sweep).
 * step == 0 zero-initialises the state (drmvsnet.py:133-134).  cost_out [B,1,H,W].
 * ------------------------------------------------------------------------- */
int aarmvs_unet_step(const float* x, int B, int H, int W, int nsrc, int step,
                     const void* packed_params, void* workspace, float* cost_out,
                     hipStream_t stream);
/* The same at a precision (aarmvs_precision); aarmvs_unet_step is the AARMVS_PREC_SPLIT form. */
int aarmvs_unet_step_p(const float* x, int B, int H, int W, int nsrc, int step,
                       const void* packed_params, void* workspace, float* cost_out, int precision,
                       hipStream_t stream);

/* ---------------------------------------------------------------------------
 * One plane's cost slice (SURVEY §8b aarmvs_cost_slice): replaces, for one depth
 * hypothesis per batch element, drmvsnet.py:307-319 -- homo_warping_depthwise x nsrc
 * (module.py:6-38), (warp - ref)^2, InterViewAAModule (drmvsnet.py:27-38) and the
 * weighted accumulation -- giving x = -(sum_v (1 + w_v) sq_v) / nsrc.
 * src_fea is a HOST array of nsrc device pointers [B,C,H,W]; rel_proj [nsrc][B][12]
 * (as for aarmvs_sweep); depth_d [B].  slice_out [B,32,H,W]; omega_out [nsrc,B,H,W]
 * (the omega weights w_v) or NULL.  `workspace` is an aarmvs_sweep_workspace_bytes
 * buffer used as scratch: a sweep in progress in the same workspace is invalidated.
 * ------------------------------------------------------------------------- */
int aarmvs_cost_slice(const float* ref_fea, const float* const* src_fea, const float* rel_proj,
                      const float* depth_d, const void* packed_params, int B, int C, int H, int W,
                      int nsrc, void* workspace, float* slice_out, float* omega_out,
                      hipStream_t stream);

/* Online winner-take-all update of one plane (SURVEY §8b aarmvs_wta_update;
 * drmvsnet.py:324-334): p = exp(cost) without max-subtraction, flag = max_prob < p
 * (strict: the first plane wins ties), max_prob/depth_map updated by the reference's
 * arithmetic select, exp_sum += p.  cost, max_prob, depth_map, exp_sum [B,HW];
 * depth_d [B].  Start from max_prob = depth_map = exp_sum = 0 (drmvsnet.py:301-304);
 * the confidence is max_prob / exp_sum after the last plane (:339). */
int aarmvs_wta_update(const float* cost, const float* depth_d, float* max_prob, float* depth_map,
                      float* exp_sum, int B, int HW, hipStream_t stream);

/* The refining form of the above, for cost planes that do not come from a sweep (see
 * aarmvs_sweep_r for the definition): aarmvs_wta_refine_update is aarmvs_wta_update of plane d
 * (the planes must come in order, d = 0, 1, ...) that also maintains `state`
 * (aarmvs_refine_state_bytes(B, HW) bytes; d == 0 resets it -- the WTA images are the caller's to
 * zero); aarmvs_wta_refine_finalize writes depth_refined / conf_window [B,HW] float and index
 * [B,HW] int32 (each may be NULL) after n planes from the images, the state and depth_values
 * [B,D], 1 <= n <= D.  aarmvs_refine_from_cost gives the same three outputs (and n = D) from a
 * whole cost volume [B,D,HW], e.g. a training sweep's: the same expressions in the same order, so
 * it equals the online result bit for bit on the same cost values. */
int aarmvs_wta_refine_update(const float* cost, int d, float* max_prob, float* depth_map,
                             float* exp_sum, void* state, const float* depth_d, int B, int HW,
                             hipStream_t stream);
int aarmvs_wta_refine_finalize(const float* max_prob, const float* depth_map, const float* exp_sum,
                               const void* state, const float* depth_values, int B, int D, int n,
                               int HW, float* depth_refined, float* conf_window, int* index,
                               hipStream_t stream);
int aarmvs_refine_from_cost(const float* cost, const float* depth_values, int B, int D, int HW,
                            float* depth_refined, float* conf_window, int* index, hipStream_t stream);

/* The posterior statistics for cost planes that do not come from a sweep (see
 * aarmvs_posterior_args for the definition): aarmvs_wta_posterior_update is aarmvs_wta_update of
 * plane d (the planes must come in order, d = 0, 1, ...) that also maintains `state`
 * (aarmvs_posterior_state_bytes(B, HW) bytes; d == 0 resets it -- the WTA images are the caller's
 * to zero); aarmvs_wta_posterior_finalize writes mean / std / entropy / runner_up [B,HW] (each
 * may be NULL) of the planes given so far from exp_sum and the state.
 * aarmvs_posterior_from_cost gives the same four outputs from a whole cost volume [B,D,HW] and
 * depth_values [B,D], e.g. a training sweep's: the same expressions in the same order, so it
 * equals the online result bit for bit on the same cost values. */
int aarmvs_wta_posterior_update(const float* cost, int d, float* max_prob, float* depth_map,
                                float* exp_sum, void* state, const float* depth_d, int B, int HW,
                                hipStream_t stream);
int aarmvs_wta_posterior_finalize(const float* exp_sum, const void* state, int B, int HW, float* mean,
                                  float* std_out, float* entropy, float* runner_up, hipStream_t stream);
int aarmvs_posterior_from_cost(const float* cost, const float* depth_values, int B, int D, int HW,
                               float* mean, float* std_out, float* entropy, float* runner_up,
                               hipStream_t stream);

/* softmax over the depth axis of cost [B,D,H,W] (drmvsnet.py:291/:342). */
int aarmvs_softmax_depth(const float* cost, float* prob, int B, int D, int HW,
                         hipStream_t stream);

/* GroupNorm (nn.GroupNorm, module.py:98-103, 245-287; FeatNet and the BPTT recompute of
 * the omega chain and the U-Net deconvs) on NCHW fp32 x [B,C,HW] with G groups (G | C).
 * gamma / beta [C] may be NULL (weight 1, bias 0).  mean_rstd: [B,G,2] out (forward) / in
 * (backward).  scratch: aarmvs_group_norm_scratch_bytes(B,C,HW) bytes of device memory.
 * Backward writes dx [B,C,HW] and, per (b,c), s1 = sum_hw dy*xhat and s2 = sum_hw dy
 * (dgamma = sum_b s1, dbeta = sum_b s2).  Statistics are fixed-order fp64 reductions. */
/* ConvLSTMCell gate math (module.py:76-92) for the BPTT recompute: from the conv output z
 * [B,4*hid,HW] (gates i, f, o, g in channel blocks) and c_prev [B,hid,HW] to h, c
 * [B,hid,HW]; backward from dh, dc (either may be NULL: zero) to dz [B,4*hid,HW] and
 * dc_prev [B,hid,HW], recomputing the gates from z. */
int aarmvs_lstm_gates_forward(const float* z, const float* c_prev, int B, int hid, int HW, float* h,
                              float* c, hipStream_t stream);
int aarmvs_lstm_gates_backward(const float* z, const float* c_prev, const float* dh, const float* dc,
                               int B, int hid, int HW, float* dz, float* dc_prev, hipStream_t stream);

size_t aarmvs_group_norm_scratch_bytes(int B, int C, int HW);
int aarmvs_group_norm_forward(const float* x, const float* gamma, const float* beta, int B, int C,
                              int HW, int G, float eps, float* y, float* mean_rstd, void* scratch,
                              hipStream_t stream);
int aarmvs_group_norm_backward(const float* dy, const float* x, const float* gamma,
                               const float* mean_rstd, int B, int C, int HW, int G, float* dx,
                               float* s1, float* s2, void* scratch, hipStream_t stream);

/* ---------------------------------------------------------------------------
 * Depth-map fusion core of one reference view (fusion.py:71-220, the per-view part of
 * filter_depth after file I/O): for every reference pixel the geometric consistency
 * against each source view's depth map (reproject_with_depth, check_geometric_consistency)
 * and filter_depth's photometric mask, per-threshold votes, geometric mask and averaged
 * depth.  Depth maps and confidence are device [H,W] float32 (all views the same size);
 * `cams` is HOST memory, AARMVS_FUSION_CAM_FLOATS(nsrc) float32 values as numpy forms
 * them in the reference (float32 inverses and products): inv(K_ref) 3x3, K_ref 3x3, then
 * per source view K 3x3, inv(K) 3x3, (E_src inv(E_ref))[:3] 3x4, (E_ref inv(E_src))[:3]
 * 3x4, row-major (aarmvs/fusion.py packs them).  Outputs (device): three [H,W] uint8
 * masks (photo, geo, final) and the [H,W] float64 averaged depth.  1 <= nsrc <=
 * AARMVS_MAX_FUSION_SRC (the reference indexes its mask list up to 10 source views).
 * ------------------------------------------------------------------------- */
#define AARMVS_MAX_FUSION_SRC 10
#define AARMVS_FUSION_CAM_FLOATS(nsrc) (18 + 42 * (nsrc))
typedef struct aarmvs_fusion_args {
  int H, W, nsrc;
  const float* ref_depth;                          /* [H,W]                 */
  const float* confidence;                         /* [H,W]                 */
  const float* src_depth[AARMVS_MAX_FUSION_SRC];   /* nsrc x [H,W]          */
  const float* cams;                               /* host, see above       */
  float photo_threshold;                           /* 0.35 DTU, 0.2 T&T     */
  unsigned char* photo_mask;                       /* [H,W] out             */
  unsigned char* geo_mask;                         /* [H,W] out             */
  unsigned char* final_mask;                       /* [H,W] out             */
  double* depth_avg;                               /* [H,W] out             */
} aarmvs_fusion_args;
int aarmvs_fusion_filter(const aarmvs_fusion_args* args, hipStream_t stream);

/* ---------------------------------------------------------------------------
 * Opt-in visibility de-duplication of the fused cloud (not in the reference; the used-pixel
 * marking of Gipuma-style fusion).  The reference emits a point for every final pixel of every
 * reference view, so a surface patch seen consistently from k views lands in the cloud about k
 * times.  With this mode a scan keeps one USED MAP per view: uint8 [H,W] on the device, in the
 * pixel grid of that view's depth map, zero at the start of the scan (the caller allocates and
 * clears it).  Reference views are processed in pair-file order.  For reference view r with
 * source views s_0 .. s_{nsrc-1}, with aarmvs_fusion_filter's arithmetic unchanged:
 *   final(p)     the final mask;
 *   m_v(p)       per source view, the i = 10 geometric mask (the one that zeroes the reprojected
 *                depth);
 *   x_v, y_v     per source view, the float32 source coordinates that the depth map is sampled at.
 *   emit(p) = final(p) && used[r][p] == 0
 *   for every p with final(p) -- emitted or not, so that coverage propagates through views that
 *   do not list each other -- and every v with m_v(p):
 *       X = rintf(x_v), Y = rintf(y_v)   (nearest pixel, ties to even)
 *       if 0 <= X < W and 0 <= Y < H:  used[s_v][Y W + X] = 1
 *   (non-finite and out-of-image coordinates mark nothing).
 * The view's points are the pixels of emit_mask instead of final_mask (pass it to
 * aarmvs_fusion_points); the averaged depth, the back-projection and the colour are unchanged, and
 * photo_mask, geo_mask, final_mask and depth_avg are bit-identical to aarmvs_fusion_filter's.
 * Deterministic: within a call used_ref is only read and the used_src maps are only written, every
 * writer stores the same byte (plain stores, no atomics), and emit depends only on the marks of
 * earlier calls -- so THE CALLS OF ONE SCAN MUST BE ORDERED ON ONE STREAM (or otherwise ordered by
 * the caller), in pair-file order.
 * used_ref NULL: nothing used yet (emit = final).  used_src[v] NULL: that view is not marked.
 * AARMVS_ERR_INVALID, before any launch: emit_mask NULL; used_ref equal to a used_src[v] (a view is
 * not its own source view); emit_mask equal to photo_mask, geo_mask or final_mask; and everything
 * aarmvs_fusion_filter rejects.  dedup == NULL is aarmvs_fusion_filter(args, stream).
 * The launch is timed under the profiler's "fusion" id (the list of kernel names is fixed).
 * The effect on DTU and Tanks and Temples scores is not measured (no datasets here).
 * ------------------------------------------------------------------------- */
typedef struct aarmvs_fusion_dedup_args {
  const unsigned char* used_ref;                    /* [H,W] or NULL (nothing used yet: emit = final) */
  unsigned char* used_src[AARMVS_MAX_FUSION_SRC];   /* [H,W] each; NULL: that view is not marked      */
  unsigned char* emit_mask;                         /* [H,W] out, required                            */
} aarmvs_fusion_dedup_args;
int aarmvs_fusion_filter_dedup(const aarmvs_fusion_args* args, const aarmvs_fusion_dedup_args* dedup,
                               hipStream_t stream);

/* ---------------------------------------------------------------------------
 * One level of OpenCV's 5x5 Gaussian pyramid (cv2.pyrDown, imgproc/src/pyramids.cpp, the
 * scalar float path), which fusion_padding.py:166 applies to the reference image: `src`
 * device float32 [H,W,C] interleaved, C = 1 or 3; `dst` device [(H+1)/2, (W+1)/2, C].
 * Horizontal pass per source row, r[x] = s[2x]*6 + (s[2x-1] + s[2x+1])*4 + s[2x-2] +
 * s[2x+2], then the same expression down the rows 2y-2 .. 2y+2 of r and * (1/256); the sums
 * run left to right, every intermediate is rounded to float32 (no fused multiply-add), and
 * out-of-range indices follow BORDER_REFLECT_101.  H, W >= 4.
 * ------------------------------------------------------------------------- */
int aarmvs_pyr_down(const float* src, int H, int W, int C, float* dst, hipStream_t stream);

/* ---------------------------------------------------------------------------
 * World points of one reference view's kept pixels (fusion.py:235-246,
 * fusion_padding.py:239-251): for every pixel with a nonzero `mask`, in row-major pixel
 * order (numpy's x[valid_points]), xyz = (inv(E) {inv(K) {x d, y d, d}, 1})[:3] in float64 on
 * the float32 matrices (numpy's matmul rounding, as aarmvs_fusion_filter), cast to float32,
 * and rgb = (unsigned char)(color * 255) in float32 (truncating).  The position of a point
 * in the output is its rank among the kept pixels (block counts, an exclusive scan, in-block
 * ranks: no atomics), so the result is the same on every run.  Points of rank >= capacity
 * are not written; `count` always receives the total number of kept pixels.  Stream-ordered:
 * nothing here waits for the device.  H * W < 2^31.
 * ------------------------------------------------------------------------- */
typedef struct aarmvs_fusion_points_args {
  int H, W;
  const unsigned char* mask;   /* [H,W] device, nonzero = keep                          */
  const double* depth;         /* [H,W] device, the averaged depth                      */
  const float* color;          /* [H,W,3] device in [0,1], or NULL                      */
  const float* cams;           /* HOST: inv(K_ref) 3x3 then inv(E_ref) 4x4, float32
                                  row-major, as numpy forms them                        */
  float* xyz;                  /* [capacity,3] device out                               */
  unsigned char* rgb;          /* [capacity,3] device out; NULL if and only if color is */
  long long capacity;          /* points that xyz / rgb have room for (>= 0)            */
  long long* count;            /* device out: number of kept pixels                     */
  void* workspace;             /* device, aarmvs_fusion_points_workspace_bytes(H, W)    */
} aarmvs_fusion_points_args;
size_t aarmvs_fusion_points_workspace_bytes(int H, int W);
int aarmvs_fusion_points(const aarmvs_fusion_points_args* args, hipStream_t stream);

/* ---------------------------------------------------------------------------
 * Opt-in per-point normals of the fused cloud (not in the reference).  A view's normal map comes
 * from its averaged depth map alone: per pixel, a least-squares plane fit over a (2r+1)^2 window.
 * For a pinhole camera a 3-D plane is affine in INVERSE depth over pixel coordinates, so the fit
 * is the linear one 1/d = a x + b y + c, and the plane's normal is proportional to K^T (a, b, c).
 * (A cross product of neighbour differences fails on winner-take-all depth, which is quantised to
 * the depth planes: neighbours mostly share a depth and the differences are staircases.)
 *
 * Definition.  All arithmetic is float64, every operation rounded on its own (no fused
 * multiply-add), sums evaluated left to right exactly as written.
 *   Centre.  p = (x0, y0) is USABLE when valid[p] != 0 and d0 = depth[p] is finite and > 0;
 *     otherwise it has no normal.
 *   Neighbours.  q = (x0 + u, y0 + v), |u|, |v| <= r, is usable when it is inside the image, valid
 *     with a finite depth > 0, and |depth[q] - d0| <= (double)max_rel_jump * d0.  The centre counts.
 *   Sums.  Over the usable pixels of the window in row-major order (v outer, u inner), with
 *     w = 1.0 / depth[q]:  the integers A = sum u^2, B = sum u v, C = sum v^2, D = sum u,
 *     E = sum v, N = sum 1 (exact), and the rounded Suw = sum (u w), Svw = sum (v w), Sw = sum w.
 *   Cofactors of the normal matrix (exact integers):
 *     c00 = C N - E E   c01 = D E - B N   c02 = B E - C D
 *     c11 = A N - D D   c12 = B D - A E   c22 = A C - B B      det = (A c00 + B c01) + D c02
 *     det > 0 is an exact test for "the usable pixels are not collinear".
 *   Plane, scaled by det (> 0: the direction is unchanged and nothing is divided by det):
 *     a = (c00 Suw + c01 Svw) + c02 Sw
 *     b = (c01 Suw + c11 Svw) + c12 Sw
 *     c = (c02 Suw + c12 Svw) + c22 Sw          cabs = (c - a x0) - b y0
 *   Camera-space normal:  m_i = (K[0][i] a + K[1][i] b) + K[2][i] cabs,
 *     len = sqrt((m0^2 + m1^2) + m2^2),  n_cam = -(m / len).  The plane is m . P = det > 0 and the
 *     camera sits at the origin, so -m faces the camera: no orientation test is needed.
 *   World normal:  n_i = (R[i][0] n0 + R[i][1] n1) + R[i][2] n2, R the upper-left 3x3 of inv(E),
 *     cast to float32.
 *   A pixel HAS A NORMAL when it is usable, N >= min_count, det > 0 and len is finite and > 0;
 *     otherwise normal = (0, 0, 0) and has_normal = 0.
 * The kernel reads depth and valid only (9 B per pixel and the halo) and writes 12 or 13 B per
 * pixel; no atomics, so the result is the same on every run.  `cams` is HOST memory: K 3x3 of the
 * DEPTH MAP's pixel grid (Tanks and Temples: the halved intrinsics), then inv(E) 4x4, float32
 * row-major (aarmvs/fusion.py packs them).
 * AARMVS_ERR_INVALID, before any launch: a NULL depth, valid, cams or normal; H or W < 1 or
 * H W >= 2^31; radius outside 1..AARMVS_MAX_NORMAL_RADIUS; min_count outside 3..(2r+1)^2;
 * max_rel_jump negative or not finite; normal or has_normal overlapping depth or valid (other
 * blocks still read them).
 *
 * aarmvs_fusion_points_normals is aarmvs_fusion_points with one more output: nxyz[rank] =
 * normal_map[p] for every kept pixel p, the rank being the one the call computes anyway, so nxyz
 * lines up with xyz and rgb.  normal_map == NULL and nxyz == NULL: it IS aarmvs_fusion_points;
 * exactly one of them NULL is AARMVS_ERR_INVALID, as is everything aarmvs_fusion_points rejects.
 * Both are timed under the profiler's "fusion_points" id (the list of kernel names is fixed).
 * Measured on synthetic data only; the effect on DTU and Tanks and Temples meshes is not measured
 * (no datasets here).
 * ------------------------------------------------------------------------- */
#define AARMVS_MAX_NORMAL_RADIUS 3
#define AARMVS_FUSION_NORMAL_CAM_FLOATS 25      /* K 3x3 then inv(E) 4x4, float32 row-major, HOST */
typedef struct aarmvs_fusion_normals_args {
  int H, W;
  const double* depth;          /* [H,W] device: the averaged depth (aarmvs_fusion_filter's depth_avg) */
  const unsigned char* valid;   /* [H,W] device: nonzero = the pixel may take part in a fit */
  const float* cams;            /* HOST, K of the DEPTH MAP's grid (T&T: the halved one), inv(E) */
  int radius;                   /* r in 1..AARMVS_MAX_NORMAL_RADIUS: window (2r+1)^2 */
  int min_count;                /* 3..(2r+1)^2: usable pixels a fit needs */
  float max_rel_jump;           /* finite, >= 0: depth-discontinuity gate, relative to the centre */
  float* normal;                /* [H,W,3] device out: unit world normal, or (0,0,0) where there is none */
  unsigned char* has_normal;    /* [H,W] device out (0/1), or NULL */
} aarmvs_fusion_normals_args;
int aarmvs_fusion_normals(const aarmvs_fusion_normals_args* args, hipStream_t stream);
int aarmvs_fusion_points_normals(const aarmvs_fusion_points_args* args, const float* normal_map /*[H,W,3]*/,
                                 float* nxyz /*[capacity,3] out*/, hipStream_t stream);

/* ---------------------------------------------------------------------------
 * Point-cloud evaluation (not in the reference): the one operation under the DTU accuracy /
 * completeness figures and the Tanks and Temples precision / recall / F-score -- for every point
 * of cloud A the distance to its nearest point of cloud B -- and what goes with it.  The DTU
 * protocol's steps (reducePts, the observation mask, the ground-plane cut) are defined under "DTU
 * protocol" below; Tanks and Temples' alignment and cropping need dataset files and are NOT
 * implemented.  aarmvs/cloud_eval.py computes the plain figures (evaluate) and the DTU ones
 * (evaluate_dtu).
 *
 * Definition.  A cloud is float32 [n,3] device memory.  A GRID is (origin[3] float64, cell float64
 * > 0).  All arithmetic is float64, every operation rounded on its own (no fused multiply-add).
 *   Cell of a point.  i_a = floor(((double)p_a - origin_a) / cell) for a = x, y, z.  A point is IN
 *     THE GRID when its three coordinates are finite and 0 <= i_a < 2^21; its KEY is the int64
 *     (i_z << 42) | (i_y << 21) | i_x, and every other point's key is INT64_MAX.  x sits in the low
 *     bits on purpose: in a key-sorted cloud the cells (i_x - r .. i_x + r, i_y, i_z) are one
 *     contiguous span, so a ring of the search costs one binary search per (i_y, i_z) row.
 *   Truncated nearest neighbour.  For query q, over all in-grid targets t_j:
 *     d2_j = (dx dx + dy dy) + dz dz with dx = (double)q_x - (double)t_x, ... (exact differences);
 *     the neighbour is the j with the smallest (d2_j, id_j) in lexicographic order, id_j =
 *     target_ids[j] if that array is given, else j;  dist = (float)sqrt(d2), index = id.
 *     d2 > (double)max_dist (double)max_dist, or no in-grid target:  dist = +inf, index = -1.
 *     q has a non-finite coordinate:                                  dist = NaN,  index = -1.
 *     q finite but outside the grid:                                  dist = +inf, index = -1.
 *   The result is EXACT: it equals the brute-force minimum over all targets whenever that minimum
 *   is <= max_dist.  How the search guarantees it:
 *     Box.  Per axis, lo_a = cell(q_a - reach) and hi_a = cell(q_a + reach), clamped to the grid,
 *       with reach = max_dist (1 + 2^-40).  The cell function is monotone in the coordinate, so
 *       every target within max_dist has lo_a <= i_a <= hi_a on every axis; cells outside the box
 *       are never looked at.  The box reaches at most ceil(max_dist / cell) + 1 cells from q's.
 *     Rings.  k = 0, 1, ... up to the box's reach: the box's cells at Chebyshev distance k from q's
 *       cell, row by row (a shell row: its whole x-span; an inner row: the two end cells).
 *     Stopping rule.  After ring k >= 1 the search stops when best_d2 <= (k cell (1 - 2^-20))^2.
 *       A target not looked at yet is k + 1 or more cells away along some axis; the rounding of the
 *       two quotients can misplace a point by less than 2^-30 cells and d2 carries a relative
 *       error below 2^-51, so its d2 is strictly above that bound: the RELATIVE SLACK 2^-20 on
 *       k cell is the safety margin, and no tie is lost.  Never after ring 0 (the bound is 0, and an
 *       equal target with a lower id may sit in the next cell).
 * aarmvs_cloud_keys: keys_out[i] = the key of xyz[i].  Sorting is the caller's job (the Python
 *   layer: a stable torch.sort and a gather).
 * aarmvs_cloud_nn: `target` [m,3] sorted by key, `target_keys` [m] ascending with the INT64_MAX
 *   entries last, `target_ids` int32 [m] or NULL, `index_out` int32 [nq] or NULL.  One thread per
 *   query; sort the queries by the same key (and un-permute the results) so that neighbouring threads
 *   walk the same spans.  AARMVS_ERR_INVALID, before any launch: a NULL required pointer; nq or m
 *   < 0 or >= 2^31; origin not finite; cell not finite or <= 0; max_dist negative or not finite;
 *   max_dist / cell > AARMVS_CLOUD_MAX_RINGS; an output overlapping an input or the other output.
 *   nq == 0: a successful no-op.  m == 0: +inf / -1 (NaN / -1 for non-finite queries).
 * aarmvs_cloud_stats: out[0] = the number of finite values of dist [n], out[1] = their fp64 sum,
 *   out[2] = the number of NaN, out[3 + k] = the number of finite values < thresholds[k] (NaN and
 *   inf never count); `thresholds` is a HOST array of n_thresholds <= AARMVS_MAX_THRESHOLDS values
 *   (NULL if 0), `out` [3 + n_thresholds] doubles on the device, `scratch`
 *   aarmvs_cloud_stats_scratch_bytes(n) bytes of device memory.  Sum order, fixed: a block owns
 *   4096 consecutive values, thread t adds values t, t + 256, ... of the block in that order, the
 *   256 threads are added by an xor butterfly per wave and then wave by wave, and one block adds the
 *   blocks' partials the same way.  n == 0 writes zeros.  AARMVS_ERR_INVALID: n < 0 or >= 2^31, more
 *   than AARMVS_MAX_THRESHOLDS thresholds, a NULL required pointer, `out` or `scratch` overlapping
 *   `dist`, `out` overlapping `scratch`.
 * aarmvs_cloud_voxel_centroids: one point per occupied cell of a KEY-SORTED cloud, in key order:
 *   the float64 sum of the cell's points in sorted order (a stable sort makes that the original
 *   order within a cell), divided by their number, cast to float32.  Points with key INT64_MAX are
 *   dropped.  The output position of a cell is its rank (block counts of cell starts, an exclusive
 *   scan, in-block ranks, as aarmvs_fusion_points).  Cells of rank >= capacity are not written;
 *   `count` (device) always receives the number of occupied cells.  `workspace`:
 *   aarmvs_cloud_voxel_workspace_bytes(n) bytes of device memory.  One thread adds a whole cell.
 * All launches go to the caller's stream, nothing waits for the device, no atomics: every result
 * is bit-identical run to run.  n, nq, m < 2^31.  Timed under the profiler's "fusion_points" id
 * (the list of kernel names is fixed).
 * ------------------------------------------------------------------------- */
#define AARMVS_CLOUD_MAX_RINGS 32
#define AARMVS_CLOUD_AXIS_BITS 21
typedef struct aarmvs_cloud_nn_args {
  const float* query;             /* [nq,3] device                                          */
  const float* target;            /* [m,3] device, sorted by key                            */
  const long long* target_keys;   /* [m] device, ascending, INT64_MAX entries last          */
  const int* target_ids;          /* [m] device or NULL (id = position in `target`)         */
  long long nq, m;                /* 0 <= nq, m < 2^31                                      */
  double origin[3];               /* the grid: finite                                       */
  double cell;                    /* finite, > 0                                            */
  float max_dist;                 /* finite, >= 0; max_dist / cell <= AARMVS_CLOUD_MAX_RINGS */
  float* dist_out;                /* [nq] device out                                        */
  int* index_out;                 /* [nq] device out, or NULL                               */
} aarmvs_cloud_nn_args;
int aarmvs_cloud_keys(const float* xyz, long long n, const double* origin /* HOST [3] */, double cell,
                      long long* keys_out, hipStream_t stream);
int aarmvs_cloud_nn(const aarmvs_cloud_nn_args* args, hipStream_t stream);
size_t aarmvs_cloud_stats_scratch_bytes(long long n);
int aarmvs_cloud_stats(const float* dist, long long n, const float* thresholds, int n_thresholds,
                       double* out, void* scratch, hipStream_t stream);
size_t aarmvs_cloud_voxel_workspace_bytes(long long n);
int aarmvs_cloud_voxel_centroids(const float* sorted_xyz, const long long* sorted_keys, long long n,
                                 float* out_xyz, long long capacity, long long* count, void* workspace,
                                 hipStream_t stream);

/* ---------------------------------------------------------------------------
 * DTU protocol (not in the reference): the steps of the published DTU evaluation that the plain
 * figures leave out -- reducePts (a greedy thinning), the observation mask and the ground-plane
 * cut.  Same rules as above: float64, every operation rounded on its own, d2 = (dx dx + dy dy) +
 * dz dz on exact float32 -> float64 differences, the caller's stream, no wait, no allocation, no
 * atomics, bit-identical run to run, timed under "fusion_points".
 *
 * Thinning.  Inputs: a cloud, a radius r > 0 (float32, promoted to float64) and a RANK per point
 *   (int32, all different).  Points that are not in the grid (a non-finite coordinate included) are
 *   dropped: never kept, nobody's neighbour.  Two in-grid points are NEIGHBOURS when d2 <=
 *   (double)r (double)r -- inclusive, so a point exactly at r is a neighbour, and so are coincident
 *   points.  KEPT is what the sequential walk in ascending rank keeps: a point is kept iff no
 *   lower-ranked neighbour is kept.  That set is the lexicographically first maximal independent
 *   set of the neighbour graph under the rank order, and the unique fixpoint of the
 * Round rule.  State per point: 0 undecided, 1 kept, 2 removed.  A round reads state_in and writes
 *   state_out for EVERY point (ping-pong between two buffers, decided points are copied through).
 *   For an undecided point p, over its neighbours q with rank(q) < rank(p):
 *     any q kept -> p removed;  else any q undecided -> p stays undecided;  else -> p kept.
 *   A round never reads what the same round writes, so the number of rounds to the fixpoint is
 *   part of the definition and the same on every run.  Every round decides at least the
 *   lowest-ranked undecided point: n rounds is a hard upper bound (reached by a line of points in
 *   rank order), with random ranks the count stays logarithmic.
 * aarmvs_cloud_thin runs `rounds` >= 1 rounds on a KEY-SORTED cloud (`xyz`, `keys`, `rank` in the
 *   same sorted layout; the grid's cell must be >= r).  The current state is in state[which]; round
 *   k = 1 .. rounds reads state[(which + k - 1) & 1] and writes state[(which + k) & 1], so the call
 *   LEAVES THE STATE IN state[(which + rounds) & 1].  init != 0 (a first call) first sets
 *   state[which] from the keys: INT64_MAX -> removed, else undecided.  `remaining` receives two
 *   int64: [0] the number of still-undecided points after the last round, [1] the number of this
 *   call's rounds that began with an undecided point (0 .. rounds; summed over the calls it is the
 *   number of rounds to the fixpoint whatever `rounds` per call was).  Both come from per-block
 *   values written as plain stores into `scratch` (aarmvs_cloud_thin_scratch_bytes(n) bytes) and
 *   one block that adds them in a fixed order.  One thread per point; an undecided point walks the
 *   (i_y, i_z) rows of the box [cell(p_a - reach), cell(p_a + reach)], reach = r (1 + 2^-40), one
 *   lower_bound per row as aarmvs_cloud_nn does (the cell function is monotone, so the box holds
 *   every neighbour; cell >= r keeps it at 3 cells per axis, 9 rows, one more where p +- reach
 *   crosses a further face), and stops at the first kept lower-ranked neighbour.
 *   AARMVS_ERR_INVALID, before any launch: NULL args or a NULL required pointer; n < 0 or >= 2^31;
 *   origin or cell not finite, cell <= 0; r negative or not finite; cell < r; rounds < 1; which not
 *   0 or 1; an output (the two states, remaining, scratch) overlapping an input or another output.
 *   n == 0: a successful no-op that writes remaining = {0, 0}.
 * Region tests.  Observation mask M: uint8 [nx,ny,nz], C-contiguous in that index order; BB float64
 *   [2][3]; Res float64 > 0; patch float64 >= 0.  For a point p with finite coordinates:
 *     IN_BOX  when for every axis a: p_a >= BB[0][a] - patch and p_a < BB[1][a] + 2 patch;
 *     g_a = rint((p_a - BB[0][a]) / Res), round-half-to-even;
 *     IN_OBS  when IN_BOX, 0 <= g_a < n_a on every axis and M[g_x,g_y,g_z] != 0;
 *     ABOVE   when ((P0 x + P1 y) + P2 z) + P3 > 0 for the plane P [4] float64.
 *   A point with a non-finite coordinate is in no region.
 * aarmvs_cloud_regions: flags_out[i] = IN_BOX | IN_OBS << 1 | ABOVE << 2 of xyz[i]; one thread per
 *   point.  `dims` [3], `bb` [2][3] and `plane` [4] are HOST arrays, `mask` is device memory.  A bit
 *   whose input is NULL is 0: bb NULL -> bits 0 and 1, mask NULL -> bit 1, plane NULL -> bit 2
 *   (mask needs bb and dims).  AARMVS_ERR_INVALID: n < 0 or >= 2^31; NULL xyz or flags_out with n >
 *   0; mask without bb or dims; bb not finite; patch negative or not finite; with a mask: Res not
 *   finite or <= 0, a dimension < 1, 2^31 voxels or more; flags_out overlapping xyz or the mask.
 *   n == 0: a successful no-op.
 * The protocol itself (thin the reconstruction, accuracy from its IN_OBS points to the ground
 * truth, completeness from the ABOVE ground-truth points to its IN_BOX points, distances strictly
 * below max_dist) is aarmvs/cloud_eval.py's evaluate_dtu.
 * ------------------------------------------------------------------------- */
typedef struct aarmvs_cloud_thin_args {
  const float* xyz;               /* [n,3] device, sorted by key                            */
  const long long* keys;          /* [n] device, ascending, INT64_MAX entries last          */
  const int* rank;                /* [n] device, in the sorted layout, all different        */
  long long n;                    /* 0 <= n < 2^31                                          */
  double origin[3];               /* the grid: finite                                       */
  double cell;                    /* finite, > 0, >= r                                      */
  float r;                        /* finite, >= 0                                           */
  int init;                       /* != 0: set state[which] from the keys first             */
  int which;                      /* 0 or 1: the buffer that holds the current state        */
  unsigned char* state[2];        /* [n] device each                                        */
  long long* remaining;           /* [2] device out                                         */
  void* scratch;                  /* aarmvs_cloud_thin_scratch_bytes(n) bytes, device       */
} aarmvs_cloud_thin_args;
size_t aarmvs_cloud_thin_scratch_bytes(long long n);
int aarmvs_cloud_thin(const aarmvs_cloud_thin_args* args, int rounds, hipStream_t stream);
int aarmvs_cloud_regions(const float* xyz, long long n, const unsigned char* mask, const int* dims,
                         const double* bb, double res, double patch, const double* plane,
                         unsigned char* flags_out, hipStream_t stream);

/* ---------------------------------------------------------------------------
 * Epilogue of the evidential head (evidential/models.py:385-459): from the three
 * classifier outputs head[i] = classif_i(...) [1][4][D][H][W] (channels: cost, log nu, log
 * alpha, log beta; at the head's full [maxdisp, H, W] resolution, where get_pred / get_logits'
 * align_corners=True trilinear resampling is the identity) and depth_values [D]:
 *   prob_i = softmax_D(cost_i) (:421), pred_i = sum_d prob_i depth_values (disparity_regression,
 *   :40-45), nu_i / alpha_i / beta_i = softplus(sum_d prob_i logit_i) (+1 for alpha; :426-430,
 *   :281-285), the NIG mixture moe_nig(moe_nig(e0, e1), e2) (:287-304) -> evidential [4][H*W]
 *   = (gamma, nu, alpha, beta), and prob_combine [D][H*W] = the mean of the three prob_i
 *   (:457-458).  B == 1 and D == AARMVS_EVIDENTIAL_D only, the reference head's limits
 *   (SURVEY F2).  HW = H * W.  The backward (for the training losses through the head,
 *   :517-558) takes dL/d evidential and dL/d prob_combine (either may be NULL: zero) and
 *   overwrites grad_head[i] [1][4][D][H][W]; no gradient flows to depth_values.
 * ------------------------------------------------------------------------- */
#define AARMVS_EVIDENTIAL_D 32
int aarmvs_evidential_epilogue(const float* const head[3], const float* depth_values, int D, int HW,
                               float* evidential, float* prob_combine, hipStream_t stream);
int aarmvs_evidential_epilogue_backward(const float* const head[3], const float* depth_values, int D,
                                        int HW, const float* grad_evidential,
                                        const float* grad_prob_combine, float* const grad_head[3],
                                        hipStream_t stream);

/* ---------------------------------------------------------------------------
 * The sampling half of FeatNet's modulated deformable convolution (models/module.py:105-236,
 * DeformConv2d.forward; used by IntraViewAAModule, drmvsnet.py:7-24): for output pixel (i, j)
 * and tap n of the 3x3 kernel, the bilinear sample of the zero-padded input at
 * (i*stride + 1 + n/3 - 1 + offset[n], j*stride + 1 + n%3 - 1 + offset[9 + n]) with the
 * reference's clamping and corner weights (:160-214), times mask[n] (the sigmoid of m_conv,
 * :216-219; NULL: no modulation).  x_nhwc [B][H][W][C] (C == 32), offset [B][18][h][w], mask
 * [B][9][h][w], val [B][h*w][9][C]: the A operand of the conv over (tap, channel) (:230-234),
 * which the caller multiplies by the weights [9*C][outc].  The forward's val equals the
 * reference's sampled tensor op for op in fp32.  The backward takes dL/d val and ADDS dL/dx
 * into grad_x_nhwc (atomically: zero it first), and writes dL/d offset [B][18][h][w] and
 * dL/d mask [B][9][h][w] (NULL when mask is NULL); like the reference's gather backward, dL/dx's
 * summation order is not fixed.
 * ------------------------------------------------------------------------- */
#define AARMVS_DEFORM_C 32
int aarmvs_deform_sample(const float* x_nhwc, const float* offset, const float* mask, int B, int C,
                         int H, int W, int h, int w, int stride, int pad, float* val,
                         hipStream_t stream);
int aarmvs_deform_sample_backward(const float* x_nhwc, const float* offset, const float* mask, int B,
                                  int C, int H, int W, int h, int w, int stride, int pad,
                                  const float* grad_val, float* grad_x_nhwc, float* grad_offset,
                                  float* grad_mask, hipStream_t stream);

/* ---------------------------------------------------------------------------
 * The classification loss from the cost volume (mvsnet_cls_loss of softmax(cost),
 * drmvsnet.py:343-361, without the probability, one-hot and log volumes) and the masked depth
 * metrics of the test pass (utils.py:150-175).  No host synchronisation, no atomics: every sum
 * is a fixed-order fp64 reduction, so the results are bit-identical run to run.  `scratch` is
 * aarmvs_cls_loss_scratch_bytes(B, HW) bytes of device memory (0 and an error for B, HW < 1),
 * overwritten by each call.
 *
 * aarmvs_cls_loss: cost [B,D,HW] (finite values only), depth_gt / mask [B,HW], depth_values
 * [B,D].  Per pixel: gt = round-half-even(mask * argmin_d |depth_values[d] - depth_gt|) (first
 * minimum; clamped to [0, D-1]), lse = log sum_d exp(cost[d]), ce = lse - cost[gt].  Outputs:
 * loss [1] = mean_b(sum mask ce / (sum mask + 1e-6)); wta_depth [B,HW] = depth_values at the
 * first maximum of the cost; max_prob [B,HW] = max_d softmax(cost) or NULL; and for the
 * backward lse [2,B,HW] (an fp32 pair: lse = lse[0] + lse[1]), gt_index [B,HW] (int32) and
 * coef [B] = 1 / ((sum mask + 1e-6) B).  Only max_prob may be NULL.
 * Deviation from the reference: where some plane's probability underflows to 0 in fp32, the
 * reference forms 0 * log(0) = NaN for that pixel (even off the ground-truth plane) and its
 * whole loss is NaN; this form never takes the log of a probability and stays finite.
 *
 * aarmvs_cls_loss_backward: grad_cost [B,D,HW] = grad_loss[0] coef[b] mask (exp(cost - lse) -
 * [d == gt_index]) from the forward's cost, lse, gt_index, mask and coef; grad_loss is a DEVICE
 * scalar (the upstream gradient).  No argument may be NULL; grad_cost must not alias cost.
 *
 * aarmvs_depth_metrics: depth_est / depth_gt / mask [B,HW]; thresholds is a HOST array of
 * n_thresholds <= AARMVS_MAX_THRESHOLDS values (NULL if 0).  Over the pixels with mask > 0.5 of
 * each batch element: out[0] = mean_b(mean |est - gt|) (AbsDepthError_metrics), out[1 + k] =
 * mean_b(share with |est - gt| > thresholds[k]) (Thres_metrics); out is [1 + n_thresholds]
 * doubles on the device.  An element with no valid pixel makes the results NaN (torch.mean of
 * an empty tensor).
 * ------------------------------------------------------------------------- */
#define AARMVS_MAX_THRESHOLDS 8
size_t aarmvs_cls_loss_scratch_bytes(int B, int HW);
int aarmvs_cls_loss(const float* cost, const float* depth_gt, const float* mask,
                    const float* depth_values, int B, int D, int HW, float* loss, float* wta_depth,
                    float* max_prob, float* lse, int* gt_index, float* coef, void* scratch,
                    hipStream_t stream);
int aarmvs_cls_loss_backward(const float* cost, const float* lse, const int* gt_index,
                             const float* mask, const float* coef, const float* grad_loss, int B,
                             int D, int HW, float* grad_cost, hipStream_t stream);
int aarmvs_depth_metrics(const float* depth_est, const float* depth_gt, const float* mask, int B,
                         int HW, const float* thresholds, int n_thresholds, double* out,
                         void* scratch, hipStream_t stream);

/* ---------------------------------------------------------------------------
 * Opt-in per-kernel timing (a diagnostic, not part of the reference interface).
 * When enabled, every launch made by the entry points above is bracketed by
 * hipEvents on its stream; aarmvs_profile_read synchronises on the recorded
 * events and returns the launch count and summed device time of one kernel.
 * ------------------------------------------------------------------------- */
void aarmvs_profile_enable(int on);
void aarmvs_profile_reset(void);
int aarmvs_profile_kernel_count(void);
const char* aarmvs_profile_kernel_name(int id);
int aarmvs_profile_read(int id, long long* launches, double* total_ms);

#ifdef __cplusplus
}
#endif
#endif /* AARMVS_H_ */
