/*
 * tokenflow_hip.h  --  C ABI of libtokenflow_hip.so (MI355X / gfx950 only).
 *
 * The drop-in boundary for TokenFlow's per-step hot path.  The reference has no
 * native code and no FFI: its "operator interface" for this path is a set of
 * torch-op sequences inside Python hook closures.  Each entry point below
 * replaces one such sequence; the file:line after "replaces" is into
 * omerbt/TokenFlow (mounted at /root/reference in the build container).
 * INTEGRATION.md shows the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch / STL types.
 *   - every function returns int: 0 = ok, >0 = hipError_t of a failed launch,
 *     <0 = argument error (TF_ERR_*); never throws, never allocates, never
 *     synchronises, keeps no global mutable state (re-entrant per stream).
 *   - pointers are DEVICE pointers (tensor.data_ptr()); the stream is a
 *     hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *     all launches are asynchronous on that stream.
 *   - tensors are dense row-major unless a leading dimension is given.
 *   - branch layout everywhere is the reference's [source | uncond | cond]
 *     (tokenflow_utils.py:117,312  `n_frames = batch_size // 3`); the *_edits entry points (ABI 10) take a MULTI-EDIT
 *     batch of E edits of one source video, B = 1 + 2E branches [source | uncond_1 | cond_1 | ... | uncond_E | cond_E].
 */
#ifndef TOKENFLOW_HIP_H
#define TOKENFLOW_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TF_ABI_VERSION 11

/* Every entry point below is exported with default visibility; the library itself is built with -fvisibility=hidden, so
 * its exported symbols are exactly the declarations of this header (checked by tests/test_hooks_cpu.py). */
#define TF_API __attribute__((visibility("default")))

/* element types */
#define TF_BF16 0
#define TF_F16 1
#define TF_F32 2

/* tf_ext_attn_fwd flags (the `inject` argument is a bit mask) */
#define TF_ATTN_INJECT 1       /* q/k injection: uncond and cond use the source branch's q and k */
#define TF_ATTN_EXACT_SCALE 2  /* scale the scores in fp32: the default since ABI 2, the bit is accepted and ignored */
#define TF_ATTN_BANK_ONLY 4    /* compute only the uncond and cond branches (those that read the K-frame bank) */
#define TF_ATTN_SOURCE_ONLY 8  /* compute only the source branch (own-frame keys) */
#define TF_ATTN_NO_SPLIT 16    /* never split a bank problem over workgroups (one pass, bit-stable across grid sizes) */
#define TF_ATTN_FOLD_SCALE 64  /* Dh = 40 only: fold scale*log2e into q, rounded to the input dtype (faster, less exact) */
#define TF_ATTN_OUT_F32 32     /* `out` is float: the normalised fp32 accumulator, without the rounding to the 16-bit I/O type */
#define TF_ATTN_NO_FUSED 128   /* never take the fused small-problem kernel (below): the streaming kernels at every size */
#define TF_ATTN_FUSED (1 << 17) /* take the fused small-problem kernel at any size it is built for */
/* tuning hints of the fused small-problem kernel (0 = automatic; A/B measurements, tools/attn_microbench.py) */
#define TF_ATTN_HINT_QW(code) (((code) & 7) << 8)    /* code 1, 2, 3 = 1 (the wave-private form), 2, 4 query waves per workgroup */
#define TF_ATTN_HINT_KW(code) (((code) & 7) << 11)   /* code 1, 2, 3, 4 = 1, 2, 4, 8 key groups per workgroup */
#define TF_ATTN_HINT_QB2 (1 << 14)                   /* wave-private form, head dims <= 80: two 32-query blocks per wave */
#define TF_ATTN_PRECISE_P (1 << 15)                  /* fused kernel, bf16: carry P as hi + lo whatever the size */
#define TF_ATTN_NO_PRECISE_P (1 << 16)               /* fused kernel: P in one 16-bit value whatever the size */
#define TF_ATTN_HINT_MIX (1 << 18)                   /* Dh = 40 streaming kernel: the mixed-MFMA-shape form whatever the launch size (it is the
                                                        default for launches of >= 1024 workgroups outside the bit-stable mode) wherever the
                                                        frames admit the interleaved kernel, S % 64 == 0 and S >= 256 (a no-op on ragged
                                                        frames); it applies to the ALL launch and to the SOURCE launch beside the dual-V
                                                        kernel; tests, measurements */

/* tf_ext_attn_fwd_edits only: the four-bank shared-softmax form for pairs of edits (below) forced on / off */
#define TF_ATTN_MULTI_V (1 << 19)
#define TF_ATTN_NO_MULTI_V (1 << 20)
/* the four-bank form at Dh = 64 forced on (plan token one<64,1,8,MV4,2,fq1>): a hint of its own, because TF_ATTN_MULTI_V keeps
   its meaning -- at Dh = 64 it selects nothing.  A no-op where the form does not exist: Dh != 64, fewer than two injecting
   edits, TF_ATTN_FOLD_SCALE, n_edits = 1.  TF_ATTN_NO_MULTI_V switches this form off too; the two together are TF_ERR_SHAPE.
   Without a hint the library takes the form only in the shape classes where it was measured faster than the composition
   by more than the run-to-run spread (profiles/r13_attn_edits_d64_ab.txt): Kq = K, H = 5 or 10, 10 <= K <= 25, S % 64 == 0,
   1024 <= S <= 9216; the composition everywhere else.  The run entry points (tf_ext_attn_run_edits,
   tf_ext_attn_runs_merge_edits) refuse it as they refuse TF_ATTN_MULTI_V. */
#define TF_ATTN_MULTI_V64 (1 << 21)
/* tf_ext_attn_run_edits / tf_ext_attn_run_edits_plan only (additive to ABI 11): the four-bank form in a run call, Dh = 40 and
   64 alike -- the injecting edits are paired ascending and each pair is ONE four-bank run launch that leaves the partial
   results of both edits (plan tokens one<40,1,4,MV4,2,fq0,run> / one<64,1,8,MV4,2,fq1,run>); an odd last injecting edit, the
   other edits and the source branch keep their launches.  Opt-in only: a run's kernel choice is a function of its arguments,
   so there is no measured default.  A no-op (same plan, same bits) where the form does not exist: Dh not 40 or 64,
   TF_ATTN_FOLD_SCALE, TF_ATTN_NO_MULTI_V, fewer than two injecting edits, n_edits = 1.  tf_ext_attn_runs_merge_edits accepts
   and ignores it (one merge folds pair-written and DUAL-written partial results alike); every call of a run set is given the
   same value.  The one-call hints TF_ATTN_MULTI_V and TF_ATTN_MULTI_V64 stay TF_ERR_SHAPE in the run entry points. */
#define TF_ATTN_RUN_MULTI_V (1 << 22)

/* most edits of one multi-edit batch (the *_edits entry points) */
#define TF_MAX_EDITS 8

/* argument errors */
#define TF_ERR_NULL (-1)
#define TF_ERR_DTYPE (-2)
#define TF_ERR_SHAPE (-3)
#define TF_ERR_ALIGN (-4)
#define TF_ERR_WORKSPACE (-5)
#define TF_ERR_COMM (-6)      /* RCCL not loadable, or a collective failed (tf_last_error has RCCL's message) */

TF_API int tf_abi_version(void);

/* Thread-local description of the last non-zero return value on this thread. */
TF_API const char* tf_last_error(void);

/* ------------------------------------------------------------------------
 * Extended attention  --  replaces the body of sa_forward.forward between the
 * q/k/v projections and to_out: tokenflow_utils.py:124-197 (PnP variant) and
 * 234-279 (SDEdit variant; call with inject = 0).
 *
 *   k, v    : [3, K, S, H*Dh]   the key/value bank of all K keyframes (token stride = ld
 *                               elements, ld >= H*Dh)
 *   q       : [3, Kq, S, H*Dh]  queries of keyframes q_frame0 .. q_frame0+Kq-1 (same ld).
 *                               Single GPU: Kq = K, q_frame0 = 0 (q is the reference's q).
 *                               Frame-sharded multi-GPU: a rank passes its own keyframes' q
 *                               and the all-gathered bank.
 *   out     : [3, Kq, S, H*Dh]  dense, same dtype (float with TF_ATTN_OUT_F32)
 *   source branch: frame f attends to its own S keys (lines 173,177);
 *   uncond / cond: frame f attends to all K*S keys of its branch (133-138,
 *   174-179) -- the bank is read in place, never replicated.
 *   inject & TF_ATTN_INJECT: uncond and cond use the SOURCE branch's q and k (124-130),
 *   by pointer aliasing; q and k are not modified.
 *   The scores are scaled in fp32 after the QK^T product, as the reference does (`* self.scale`, 173-175).
 *   inject & TF_ATTN_FOLD_SCALE (opt-in, Dh = 40 only): scale*log2(e) is folded into q, rounded to the input dtype
 *   once (relative error <= 2^-9 per element in bf16): several % faster, inside the parity bound on unit-variance
 *   logits but 3-12x outside it on peaked ones (logit std 4-16; profiles/r02_fold_accuracy.txt) -- a speed knob
 *   for callers who accept that, never the default.
 *   scale = attn.scale (Dh^-0.5).  Dh in {40, 64, 80, 160}; dtype bf16 or f16;
 *   any S >= 1 (latent grids of odd resolutions: 9x5 = 45 tokens at the mid block of 576x320);
 *   ld a multiple of 8.  fp32 softmax / accumulation, online softmax over
 *   64-key tiles, P rounded to the input dtype before P.V (as the reference's
 *   autocast path does).
 *
 *   inject & TF_ATTN_BANK_ONLY / TF_ATTN_SOURCE_ONLY: compute only the uncond + cond branches / only the
 *   source branch (the head-sharded multi-GPU path runs them on different tensors); slabs of q, k, v, out
 *   that the selected part does not need are never touched.
 *   Small grids (a sharded rank, the coarse levels) split every bank problem into runs of bank frames over
 *   extra workgroups and merge the partial results (fp32) in a second launch; TF_ATTN_NO_SPLIT keeps the
 *   one-pass form, whose arithmetic per (query, head) does not depend on the grid.
 *
 *   inject & TF_ATTN_OUT_F32: `out` is float [3, Kq, S, H*Dh]; the softmax-normalised fp32 accumulator is stored
 *   as is.  Removes the output rounding (2^-9 relative for bf16) from the result: the mode in which the
 *   "< 1e-3 per token" target of BASELINE.json holds for outputs of any magnitude.
 *
 *   Small problems -- S <= 256 always; S <= 1024 on small grids (a sharded rank, BASELINE config 1) unless
 *   TF_ATTN_NO_SPLIT -- run in ONE fused launch (csrc/ext_attn_fused.hip): V is transposed inside the kernel
 *   (ds_read_b64_tr_b16, no pre-pass), the key sequence is split over the wave groups of a workgroup and merged
 *   through LDS (no partials, no merge launch), and for bf16 at S <= 256 P is carried as hi + lo bf16 so that the
 *   rounding of P (2^-9; the reference's fp16 autocast path rounds to 2^-11 at this point) drops out of the result.
 *   Which calls take it is a function of the SHAPE alone under TF_ATTN_NO_SPLIT, so one-pass results stay
 *   bit-identical between a sharded rank and the single GPU; TF_ATTN_NO_FUSED keeps the streaming kernels.
 *
 *   ws: scratch for the transposed V bank (+ key norms, + split-form partials); size from
 *   tf_ext_attn_workspace_bytes.
 *
 *   The memory contract of this and of every other entry point that takes a workspace (enforced by
 *   tests/test_mem_contract_gpu.py):
 *     - the contents of ws on entry are arbitrary (NaN bit patterns included): a call reads no scratch word it has not
 *       written itself, so its result does not depend on them;
 *     - a call writes only [ws, ws + *_workspace_bytes) -- ws_bytes may be exactly that value -- and the rows of `out`
 *       (and of the other outputs) it owns; rows of branches the selected part does not compute are left as they were;
 *     - inputs are read only inside their frames' S rows x H*Dh columns (D columns for the NN search and the gather):
 *       whatever lies in the other columns of a row of stride ld, behind row S - 1 or next to a tensor is never loaded
 *       into arithmetic, and no input is modified.
 *
 *   The issue contract of every entry point (enforced by tests/test_issue_contract_gpu.py): every launch of a call goes
 *   to `stream`, or to a stream of the library's own behind an event edge from `stream` and joined back in front of
 *   what the call leaves on it (the rank executor); the call returns without waiting for the GPU; it can be captured
 *   into a HIP graph and replayed on other contents of the same tensors; two calls on two streams with two workspaces
 *   share nothing.  The tests issue every call on a busy side stream behind inputs that arrive late, read the stream's
 *   state when the call returns, replay a capture next to reused scratch, and run a call beside itself.
 * ------------------------------------------------------------------------ */
TF_API size_t tf_ext_attn_workspace_bytes(int K, int S, int H, int Dh, int dtype);

TF_API int tf_ext_attn_fwd(const void* q, const void* k, const void* v, void* out,
                    int K, int Kq, int q_frame0, int S, int H, int Dh, int64_t ld, float scale,
                    int inject, int dtype, void* ws, size_t ws_bytes, void* stream);

/* The same with explicit branch / frame strides (elements), for callers whose q, k, v arrive in the layout a
 * collective delivers them and whose output feeds the next collective (tokenflow_amd/sharded.py: the received
 * all-to-all buffer is [frame][slab][S][H*Dh], the returned one [frame][branch][S][H*Dh]):
 *   strides = { q_branch, q_frame, k_branch, k_frame, v_branch, v_frame, out_branch, out_frame, q_token }   (9 values)
 *   element (b, f, s, c) of k / v is k[b*k_branch + f*k_frame + s*ld + c], of q  q[b*q_branch + f*q_frame + s*q_token + c]
 *   (q has its own token stride since ABI 3: a rank's queries may be a column slab of its fused projection output
 *   while the bank arrives from an all-gather as dense slabs); out has token stride H*Dh.
 * Branch b of a tensor is addressed as base + b*branch_stride even when a call never touches branch 0 (bank-only
 * calls): pass base = (first touched slab) - b*branch_stride.  tf_ext_attn_fwd is this function with dense strides. */
TF_API int tf_ext_attn_fwd_strided(const void* q, const void* k, const void* v, void* out,
                            int K, int Kq, int q_frame0, int S, int H, int Dh, int64_t ld, const int64_t* strides,
                            float scale, int inject, int dtype, void* ws, size_t ws_bytes, void* stream);

/* Launch plan of tf_ext_attn_fwd for dense tensors of this shape and these flags (host only: touches no device,
 * allocates nothing; computed by the launch code itself, not by a model of it).  Returns the number of launches, or a
 * TF_ERR_* (TF_ERR_WORKSPACE: `buf` is too small).  buf receives one ';'-separated token per launch in launch order,
 * naming the kernel and its template parameters:
 *   vt_pack                          the V^T pre-pass
 *   il<Dh,NW,MODE,MINW,DMA>          half-tile interleaved kernel (DMA 3: the Dh = 40 mixed-MFMA-shape form)
 *   one<Dh,QT,NW,MODE,MINW,fqF[,kt128][,sb]>   one-tile streaming kernel
 *   pp<Dh,MODE>                      ping-pong kernel
 *   merge[nseg=N]                    merge of the split form's N partial results
 *   fused[qw=.,kw=.,qb=.,prec=.]     fused small-problem kernel
 * MODE is ALL, DUAL or SOURCE. */
TF_API int tf_ext_attn_plan(int K, int Kq, int S, int H, int Dh, int flags, int dtype, char* buf, size_t len);

/* ------------------------------------------------------------------------
 * Extended attention of a multi-edit batch (ABI 10): several prompts on one source video in one pass.
 *
 * Semantics: B = 1 + 2*n_edits branches, branch-major [source | uncond_1 | cond_1 | ... | uncond_E | cond_E]; the slices of
 * the result that belong to edit e (source, uncond_e, cond_e) are what tf_ext_attn_fwd_strided computes on
 * [source | uncond_e | cond_e].  Nothing mixes edits.  n_edits = 1 IS tf_ext_attn_fwd_strided; 1 <= n_edits <= TF_MAX_EDITS.
 *
 *   q, k, v, out, K, Kq, q_frame0, S, H, Dh, ld, strides, scale, dtype: as tf_ext_attn_fwd_strided; branch b of a tensor
 *     lives at base + b * branch_stride, b < B.
 *   flags: TF_ATTN_INJECT, TF_ATTN_FOLD_SCALE, TF_ATTN_OUT_F32, TF_ATTN_NO_SPLIT, TF_ATTN_NO_FUSED / TF_ATTN_FUSED, the hints:
 *     as tf_ext_attn_fwd, applied to every part.  TF_ATTN_BANK_ONLY / TF_ATTN_SOURCE_ONLY: TF_ERR_SHAPE.
 *   ws: tf_ext_attn_edits_workspace_bytes (the V^T image and key norms of all B branches; the split form's partial results
 *     once: the edits run one behind the other on the stream).
 *
 * Composition: ONE V^T pre-pass covers every branch that a streaming launch reads; every edit's bank branches run through
 * the launches a TF_ATTN_BANK_ONLY call on that edit's slabs takes (DUAL under injection, the split form, the fused
 * small-problem kernel), the source branch runs once through those of a TF_ATTN_SOURCE_ONLY call.
 * Identity: edit e's bank branches equal that TF_ATTN_BANK_ONLY call, and the source branch the TF_ATTN_SOURCE_ONLY call,
 * BIT FOR BIT (same kernels, same values) -- with one exception:
 *
 * The four-bank form (TF_ATTN_INJECT, Dh = 40, fp32 score scaling, n_edits >= 2).  Under injection the uncond and cond
 * branches of EVERY edit use the source's q and k, so softmax(QK^T) is the same for all 2E bank branches.  One workgroup
 * then computes a PAIR of edits: QK^T and the online softmax once, four P.V products against the four V banks out of one
 * packed V^T image (160 value rows + the ones row of the common denominator; plan token one<40,1,4,MV4,2,fq0>); an odd
 * last edit takes the DUAL launch.  Always one-pass launches (no split, no fused kernel) for the bank branches; any S >= 1.
 * Its result is held to the oracle within the attention bound; it is NOT bit-identical to the DUAL composition (another
 * kernel: other tile shapes and summation order).  TF_ATTN_MULTI_V forces it on wherever it exists, TF_ATTN_NO_MULTI_V
 * off; without a hint the library takes it only for the shape classes where it was measured faster than the composition
 * by more than the run-to-run spread (profiles/r08_attn_edits_ab.txt): Kq = K, H = 8, 4 <= K <= 8, 1024 <= S <= 4096; the
 * composition everywhere else (other grids were not measured).
 * At Dh = 64 the form has a hint of its own, TF_ATTN_MULTI_V64, and a measured default of its own (see the flag): four unpacked
 * 64-row banks in one LDS image (8 M-tiles), one row sum for all four, 8-wave workgroups (token one<64,1,8,MV4,2,fq1>); same
 * pairing, same one-pass launches, same bound.  TF_ATTN_MULTI_V selects nothing there.
 *
 * tf_ext_attn_edits_plan: the launches of the call for dense tensors, as tf_ext_attn_plan (host only); the four-bank launch
 * is the token one<40,1,4,MV4,2,fq0>.
 * ------------------------------------------------------------------------ */
TF_API size_t tf_ext_attn_edits_workspace_bytes(int K, int S, int H, int Dh, int n_edits, int dtype);

TF_API int tf_ext_attn_fwd_edits(const void* q, const void* k, const void* v, void* out, int K, int Kq, int q_frame0,
                          int S, int H, int Dh, int64_t ld, const int64_t* strides, float scale, int flags, int dtype,
                          int n_edits, void* ws, size_t ws_bytes, void* stream);

TF_API int tf_ext_attn_edits_plan(int K, int Kq, int S, int H, int Dh, int n_edits, int flags, int dtype, char* buf,
                           size_t len);

/* ------------------------------------------------------------------------
 * Per-edit injection state (ABI 11): the edits of one batch may differ in their q/k injection schedule (PnP's pnp_attn_t), so
 * at some steps only SOME of them inject.  tf_ext_attn_fwd_edits_masked takes the arguments of tf_ext_attn_fwd_edits plus
 * inject_mask: bit e set = edit e (0-based) injects, i.e. its uncond and cond branches use the source's q and k; bit e clear =
 * they use their own.  The mask IS the injection state: TF_ATTN_INJECT in `flags` gives TF_ERR_SHAPE, and so does a bit at or
 * above n_edits.  Semantics as above: the slices of edit e are what tf_ext_attn_fwd_strided computes on
 * [source | uncond_e | cond_e] with edit e's OWN flag.  Workspace: tf_ext_attn_edits_workspace_bytes, unchanged.
 *
 * Composition: ONE V^T pre-pass over the span of the branches that a streaming launch reads; it leaves the key norms of
 * every branch whose own keys are read -- the source and the edits that do not inject.  Then the bank launches, the source
 * branch last:
 *   1. the injecting edits in ascending order, paired 1st with 2nd, 3rd with 4th, ...: a pair takes the four-bank form where
 *      the pair rule selects it, otherwise each edit the launches of its TF_ATTN_BANK_ONLY | TF_ATTN_INJECT call;
 *   2. an odd last injecting edit as the odd edit of tf_ext_attn_fwd_edits (the DUAL launch beside four-bank pairs);
 *   3. the other edits in ascending order, each through the launches of its own TF_ATTN_BANK_ONLY call on its own q / k / v;
 *   4. the source branch through the launches of the TF_ATTN_SOURCE_ONLY call.  That call is given TF_ATTN_INJECT iff EVERY
 *      edit injects: the source branch reads its own q and k either way and its values do not depend on the flag, but the
 *      launch decision of a source-only call may, and the two uniform masks must be tf_ext_attn_fwd_edits exactly.
 * Pair rule of the four-bank form: as for tf_ext_attn_fwd_edits, with the number of INJECTING edits (>= 2) in the place of
 * n_edits; Dh = 40 (Dh = 64 behind TF_ATTN_MULTI_V64), fp32 score scaling, TF_ATTN_MULTI_V / TF_ATTN_NO_MULTI_V and the
 * measured default unchanged.  The two
 * edits of a pair need not be neighbours (mask 0b101 pairs edits 0 and 2): the launch is given the branch distance between
 * them and is the same grid and work as a pair of neighbours.
 *
 * Identity: edit e's bank branches equal that edit's tf_ext_attn_fwd_strided(..., TF_ATTN_BANK_ONLY [| TF_ATTN_INJECT]) call,
 * and the source branch the TF_ATTN_SOURCE_ONLY call, BIT FOR BIT; the exception is a pair in the four-bank form, held to the
 * oracle within the attention bound.  inject_mask == 0 and inject_mask == all ones record exactly the plans of
 * tf_ext_attn_fwd_edits without / with TF_ATTN_INJECT and give the same bits (that entry point IS these two masks).
 *
 * tf_ext_attn_edits_masked_plan: the launches of the call for dense tensors (host only), the tokens of
 * tf_ext_attn_edits_plan.
 * ------------------------------------------------------------------------ */
TF_API int tf_ext_attn_fwd_edits_masked(const void* q, const void* k, const void* v, void* out, int K, int Kq, int q_frame0,
                                 int S, int H, int Dh, int64_t ld, const int64_t* strides, float scale, int flags, int dtype,
                                 int n_edits, unsigned inject_mask, void* ws, size_t ws_bytes, void* stream);

TF_API int tf_ext_attn_edits_masked_plan(int K, int Kq, int S, int H, int Dh, int n_edits, unsigned inject_mask, int flags,
                                  int dtype, char* buf, size_t len);

/* ------------------------------------------------------------------------
 * The PARTS of a multi-edit attention call (additive to ABI 11): what a frame-sharded rank needs -- the bank branches of every
 * edit on the buffer its exchange delivered, the source branch of its own frames on its local tensors.
 * tf_ext_attn_fwd_edits_part takes the arguments of tf_ext_attn_fwd_edits_masked plus qk_compact; tf_ext_attn_fwd_edits and
 * tf_ext_attn_fwd_edits_masked themselves keep refusing the part bits.
 *   flags: as tf_ext_attn_fwd_edits_masked, and
 *     TF_ATTN_BANK_ONLY    the bank branches of every edit: steps 1-3 of the masked composition behind its single V^T
 *                          pre-pass over the branches that stream.  Slab 0 (the source) of v and of out is never touched.
 *     TF_ATTN_SOURCE_ONLY  step 4 alone (behind a pre-pass over the source branch where it streams).
 *     neither              all parts.      Both: TF_ERR_SHAPE.
 *     The four-bank form stays available in the bank part under its rule and hints.
 *   Kq / q_frame0 as everywhere: a rank passes its own query frames against the bank of K.
 *   qk_compact = 0: q and k are addressed densely, [source | uncond_1 | cond_1 | ...], as in the calls above.
 *   qk_compact = 1: q and k hold only the branches some launch reads.  Branch slot 0 is the source; then two slots (uncond,
 *     cond) per NON-injecting edit in ascending edit order: non-injecting edit number i of the mask (0-based) reads q and k
 *     at slots 1 + 2i and 2 + 2i, every injecting edit reads slot 0.  v and out are never compacted.  A slot that nothing reads
 *     (slot 0 of a bank part in which no edit injects; every slot but 0 of a source part) need not exist: the caller moves
 *     the base pointer so that the slots that are read fall where they lie.  Other values: TF_ERR_SHAPE.
 *   Workspace: tf_ext_attn_edits_workspace_bytes, unchanged.
 *
 * One fused launch: where EVERY part the call computes would take the fused small-problem kernel (each part's own decision,
 * as in the calls above), all of them run in ONE launch of up to 1 + TF_MAX_EDITS tensor sets -- one per edit's bank branches
 * (the injecting edits first, as the composition orders them) and the source set -- with the injection state per set.  In
 * the plan this is the fused token with ",sets=N" appended for N > 2: fused[qw=1,kw=4,qb=1,prec=1,sets=4]; one or two sets
 * record the plain token.  The arithmetic of a (query, head) in that kernel depends on KW and PREC only: under
 * TF_ATTN_NO_SPLIT (KW = 4, PREC by shape) the one launch equals the launches of the parts bit for bit.  In the default mode
 * the plan sees the joint grid and may choose another KW than a part alone would (or leave the fused kernel: the parts then
 * run as in the masked call); results are then held to the attention bound, like any two launch plans.
 *
 * Identity: edit e's bank branches equal that edit's tf_ext_attn_fwd_strided(..., TF_ATTN_BANK_ONLY [| TF_ATTN_INJECT]) call
 * and the source branch the TF_ATTN_SOURCE_ONLY call BIT FOR BIT, dense or compact; the exceptions are a pair in the
 * four-bank form and the joint fused launch in the default mode (both within the attention bound of the oracle).
 *
 * tf_ext_attn_edits_part_plan: the launches of the call for dense tensors (host only).
 * ------------------------------------------------------------------------ */
TF_API int tf_ext_attn_fwd_edits_part(const void* q, const void* k, const void* v, void* out, int K, int Kq, int q_frame0,
                               int S, int H, int Dh, int64_t ld, const int64_t* strides, float scale, int flags, int dtype,
                               int n_edits, unsigned inject_mask, int qk_compact, void* ws, size_t ws_bytes, void* stream);

TF_API int tf_ext_attn_edits_part_plan(int K, int Kq, int S, int H, int Dh, int n_edits, unsigned inject_mask, int qk_compact,
                                int flags, int dtype, char* buf, size_t len);

/* ------------------------------------------------------------------------
 * Extended attention over a bank that arrives in pieces: "run + merge" (ABI 9).
 *
 * The bank branches (uncond, cond) of Kq query frames are computed one RUN of bank frames [run_f0, run_f0 + run_n) at a
 * time; every run leaves, for each (bank branch, query frame, head, query), the unnormalised fp32 output, the softmax
 * denominator and the log2-domain shift -- what one segment of the split form leaves -- in its own slots of the workspace,
 * and tf_ext_attn_runs_merge folds the slots of all n_runs runs into `out`:
 *     out = sum_r O_r 2^(s_r - M) / sum_r l_r 2^(s_r - M),   M = max_r s_r,
 * reduced in slot order (run 0 first), so the result is a function of the runs alone: not of the order in which the run
 * calls were issued, nor of the streams they ran on.  A host that receives keyframes from peers starts on the frames it
 * holds while the others travel (csrc/rank_exec.hip, TF_RANK_BANK_RUNS).
 *
 *   q, out, K, Kq, q_frame0, S, H, Dh, ld, strides, scale, dtype: as tf_ext_attn_fwd_strided.
 *   k, v: addressed as the full bank is -- frame f of branch b at base + b*branch_stride + f*frame_stride -- but only the
 *     run's frames are read: a caller whose run lives in another buffer passes base = (the run's first frame) -
 *     run_f0*frame_stride - ..., formed as the text above describes for branches.  Nothing outside the run's frames is
 *     touched, prefetches included.
 *   run, n_runs: this call fills the slots of run `run`.  The runs of one set must PARTITION [0, K) (each frame in exactly
 *     one run) and use the same K, Kq, q_frame0, S, H, Dh, n_runs, dtype and workspace; the library cannot check that across
 *     calls.  1 <= n_runs <= K.
 *   flags: TF_ATTN_INJECT, TF_ATTN_FOLD_SCALE, TF_ATTN_OUT_F32, TF_ATTN_HINT_MIX, TF_ATTN_NO_SPLIT as above (the same in
 *     every call of a set, the merge included).  TF_ATTN_BANK_ONLY: the bank branches only.  WITHOUT it the call also
 *     computes the source branch of the query frames, final, into `out` -- by the kernel the TF_ATTN_SOURCE_ONLY |
 *     TF_ATTN_NO_SPLIT | TF_ATTN_NO_FUSED call takes, bit for bit -- which needs [q_frame0, q_frame0 + Kq) inside the run
 *     (TF_ERR_SHAPE otherwise): exactly one run of a set is issued without TF_ATTN_BANK_ONLY.
 *     TF_ATTN_SOURCE_ONLY, TF_ATTN_FUSED and the fused kernel's hints: TF_ERR_SHAPE.  The fused small-problem kernel has no
 *     partial output: run calls take the streaming kernels at every size, as TF_ATTN_NO_FUSED does.
 *   A run may split itself over further workgroups by the rule of the split form; how many slots it owns and fills is
 *     hidden in the workspace layout and is a function of the call's arguments alone.
 *   ws: ONE workspace per set, tf_ext_attn_runs_workspace_bytes; the runs write disjoint parts of it (their frames'
 *     positions in the V^T image and the key norm table, their own slots) and may execute concurrently on different streams.
 *   tf_ext_attn_runs_merge reads the slots of all n_runs runs and writes the bank branches 1, 2 of `out` (element
 *     (b, f, s, c) at out[b*out_branch_stride + f*out_frame_stride + s*H*Dh + c]; 16-bit, or float with TF_ATTN_OUT_F32).
 *     Ordering it behind the run calls -- stream order or events -- is the caller's job.
 *   No call allocates, synchronises or keeps state outside `ws`.
 *   Identity: the merge re-associates fp32 sums as the split form's does.  A run set equals the oracle within the attention
 *   bound and equals, bit for bit, any other execution of the same runs; it does NOT equal the one-call form bit for bit.
 *
 * tf_ext_attn_run_plan: the launches of one run call over run_n frames (the tokens of tf_ext_attn_plan; launches that
 * leave partial results carry ",run" as their last parameter, e.g. il<40,8,ALL,4,2,run>) followed by the merge,
 * merge[runs=N].  Host only.
 * ------------------------------------------------------------------------ */
TF_API size_t tf_ext_attn_runs_workspace_bytes(int K, int Kq, int S, int H, int Dh, int n_runs, int dtype);

TF_API int tf_ext_attn_run(const void* q, const void* k, const void* v, void* out,
                    int K, int Kq, int q_frame0, int run_f0, int run_n, int run, int n_runs,
                    int S, int H, int Dh, int64_t ld, const int64_t* strides,
                    float scale, int flags, int dtype, void* ws, size_t ws_bytes, void* stream);

TF_API int tf_ext_attn_runs_merge(void* out, int K, int Kq, int S, int H, int Dh, int n_runs,
                           int64_t out_branch_stride, int64_t out_frame_stride,
                           int flags, int dtype, void* ws, size_t ws_bytes, void* stream);

TF_API int tf_ext_attn_run_plan(int K, int Kq, int run_n, int n_runs, int S, int H, int Dh,
                         int flags, int dtype, char* buf, size_t len);

/* ------------------------------------------------------------------------
 * "Run + merge" for a MULTI-EDIT batch (additive to ABI 11): B = 1 + 2*n_edits branches [source | uncond_1 | cond_1 | ...],
 * bit e of inject_mask = edit e (0-based) reads the source's q and k.  The composition of tf_ext_attn_fwd_edits_masked
 * applied to a run: a run call computes, for the run's bank frames only, the partial results (unnormalised O, denominator,
 * log2-domain shift) of EVERY edit's two bank branches, each edit under its own injection state, and -- without
 * TF_ATTN_BANK_ONLY -- the source branch of the query frames, once and final, as tf_ext_attn_run does.
 * tf_ext_attn_runs_merge_edits folds all runs of all 2E bank branches in slot order in ONE launch.
 *
 *   Launches of a run call: ONE V^T pre-pass over the run's frames of every branch the call reads (at the positions the
 *   frames have in the image of the whole bank; key norms of the source and of the edits that do not inject), then every
 *   edit through the launches of its own tf_ext_attn_run call -- the injecting edits first, then the others, ascending --
 *   then the source launch.  Injecting edits take the DUAL run form where the single-edit run does.  The one-call hints of
 *   the four-bank form select nothing in a run: TF_ATTN_MULTI_V and TF_ATTN_MULTI_V64 are TF_ERR_SHAPE, TF_ATTN_NO_MULTI_V is
 *   accepted.  The run form has an opt-in of its own, TF_ATTN_RUN_MULTI_V (Dh = 40, 64): the injecting edits are paired
 *   ascending (1st with 2nd, 3rd with 4th, whatever lies between them) and each pair is ONE four-bank run launch in the place
 *   of its first edit's launches -- one QK^T and one softmax over the source's q / k for the four P.V products, the partial
 *   rows of each edit in that edit's own region, split into exactly the slots the header records for the injecting state.  An
 *   odd last injecting edit, the other edits and the source branch keep their launches and their bits; a paired edit is held
 *   to the oracle bound, not to its single-edit run set bit for bit.  The merge call accepts and ignores the bit.
 *   q, k, v, out, strides: as tf_ext_attn_run, v and out addressed over all B branches (a bank-only call never touches their
 *   source slabs).  compact: bit 0 = q, bit 1 = k is in the compact layout of tf_ext_attn_fwd_edits_part (slot 0 the
 *   source, then (uncond, cond) of every NON-injecting edit, ascending); the two are separate, so a rank's remote runs read
 *   its dense local q against the compact k of a receive buffer without a staging copy.
 *   Refusals (TF_ERR_SHAPE, before anything touches the device): everything tf_ext_attn_run refuses; TF_ATTN_INJECT beside
 *   a mask; mask bits at or above n_edits; n_edits outside 1 .. TF_MAX_EDITS; TF_ATTN_MULTI_V; compact outside 0 .. 3.
 *   ws: ONE workspace per run set, tf_ext_attn_runs_edits_workspace_bytes -- the image and norm table of all B branches, one
 *   header entry per run that carries the slot count of BOTH injection states (how far a run splits itself depends on the
 *   edit's state; the merge picks per edit by inject_mask, which must be the run calls'), and the partial results
 *   [2E][Kq][H][S][n_runs * slots][Dh + 8]: every edit's launches see the layout of a single-edit run set.
 *   n_edits = 1 IS tf_ext_attn_run / tf_ext_attn_runs_merge (TF_ATTN_INJECT iff the mask is 1): same launches, same plan
 *   tokens, same bits, same workspace size.
 *
 *   Identity: for every edit e the merged bank branches equal, bit for bit, the single-edit run set on
 *   [source | uncond_e | cond_e] -- tf_ext_attn_run per run + tf_ext_attn_runs_merge with the same runs, the same flags and
 *   edit e's injection flag -- and the source branch equals that run set's source branch bit for bit.  The result is a
 *   function of the runs alone, not of issue order or streams.  It equals the oracle within the attention bound; it does NOT
 *   equal the one-call multi-edit forms (tf_ext_attn_fwd_edits*) bit for bit.
 *
 * tf_ext_attn_run_edits_plan: the tokens of one run call -- vt_pack, per edit the ",run>" tokens of its own run call, the
 * source token unless TF_ATTN_BANK_ONLY -- followed by merge[runs=N,edits=E].  Host only.
 * ------------------------------------------------------------------------ */
TF_API size_t tf_ext_attn_runs_edits_workspace_bytes(int K, int Kq, int S, int H, int Dh, int n_runs, int n_edits, int dtype);

TF_API int tf_ext_attn_run_edits(const void* q, const void* k, const void* v, void* out,
                          int K, int Kq, int q_frame0, int run_f0, int run_n, int run, int n_runs,
                          int S, int H, int Dh, int64_t ld, const int64_t* strides,
                          float scale, int flags, int dtype, int n_edits, unsigned inject_mask, int compact,
                          void* ws, size_t ws_bytes, void* stream);

TF_API int tf_ext_attn_runs_merge_edits(void* out, int K, int Kq, int S, int H, int Dh, int n_runs, int n_edits,
                                 unsigned inject_mask, int64_t out_branch_stride, int64_t out_frame_stride,
                                 int flags, int dtype, void* ws, size_t ws_bytes, void* stream);

TF_API int tf_ext_attn_run_edits_plan(int K, int Kq, int run_n, int n_runs, int S, int H, int Dh, int n_edits,
                               unsigned inject_mask, int flags, int dtype, char* buf, size_t len);

/* ------------------------------------------------------------------------
 * Frames <-> heads re-sharding of the multi-GPU pivotal pass (no counterpart in the single-process reference;
 * tokenflow_amd/sharded.py).  Rank r sends head group w of its Kl keyframes' slabs to rank w:
 *   tf_head_pack:    send[w][f][i][s][0..hd)  = slab_i[f][s][w*hd .. (w+1)*hd)     i < ns slabs, each a
 *                    [Kl, S, ld] tensor with its own frame stride (elements); one launch for all slabs.
 *   tf_head_unpack:  dst_b[f][s][w*hd ..)     = recv[w][f][b][s][0..hd)            b < nb destinations.
 * ns, nb <= 6 * TF_MAX_EDITS (48): a multi-edit batch packs up to 6 slabs per edit -- q, k and v of its two branches where
 * no edit injects -- and unpacks 2 per edit; a single edit's 6 keep the launch they always had.
 * elem_bytes 2 or 4; hd*elem_bytes and ld*elem_bytes multiples of 16.
 * ------------------------------------------------------------------------ */
TF_API int tf_head_pack(const void* const* slabs, const int64_t* frame_strides, int ns, void* send, int W, int Kl, int S,
                 int hd, int64_t ld, int elem_bytes, void* stream);

TF_API int tf_head_unpack(const void* recv, void* const* dsts, const int64_t* frame_strides, int nb, int W, int Kl, int S,
                   int hd, int64_t ld, int elem_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Halo pack of a sliding-window bank on a frame shard (additive to ABI 11; tf_rank_pivotal_window below).
 * ONE launch packs the bank slabs of the local keyframes that peers read into the send buffer of ONE tf_all_to_all_rows:
 *   send rows, peer after peer: for segment p the local frames [seg_f0[p], seg_f0[p] + seg_n[p]), each row
 *   [slab 0 .. ns)[S][D] = slab_i[frame][s][0 .. D)   (slab_i a [Kl, S, ld] tensor with its own frame stride, in elements).
 * A frame several peers read is written to each of their segments; a peer that reads nothing has seg_n = 0.  The segment
 * table (n_seg <= TF_MAX_WORLD entries) rides in the kernel arguments: no device table, no synchronisation, capturable.
 * With the rank's own frames as its self rows (seg = [0, Kl) for itself) the RECEIVE buffer of the exchange is the extended
 * bank [F][ns][S][D] in ascending global frame order, which the attention reads in place (frame stride ns*S*D, branch stride
 * S*D).  The self rows cost one extra device copy of Kl*ns*S*D elements (RCCL moves them device to device, the host hooks and
 * the loopback transport through their own copies); removing it is left to a later change.
 * 16-bit elements only (TF_ERR_DTYPE otherwise); D and ld multiples of 8 elements, ns <= 6, segments inside [0, Kl):
 * TF_ERR_SHAPE; pointers and frame strides 16-byte aligned: TF_ERR_ALIGN.  All checked before anything touches the device.
 * ------------------------------------------------------------------------ */
TF_API int tf_window_halo_pack(const void* const* slabs, const int64_t* frame_strides, int ns, void* send, int n_seg,
                        const int* seg_f0, const int* seg_n, int Kl, int S, int D, int64_t ld, int dtype, void* stream);

/* ------------------------------------------------------------------------
 * Halo pack of an ANCHORED sliding-window bank on a frame shard (additive to ABI 11; tf_rank_pivotal_frame_sets below).
 * tf_window_halo_pack where what peer p reads of this rank is a SET of local frames -- its window reach plus the anchor
 * keyframes this rank owns -- instead of one range: masks is a HOST array of n_peer <= TF_MAX_WORLD 64-bit masks over the Kl
 * local frames (Kl <= 64).  Peer p's send rows are the member frames of masks[p] in ASCENDING order, each row
 * [slab 0 .. ns)[S][D] as there.  An empty mask contributes nothing; a frame in several masks is written to each.  The masks
 * and the row prefix ride in the kernel arguments (64 x 8 + 65 x 4 bytes): no device table, no copy, no sync, capturable.
 * ONE launch, a bandwidth-bound copy in 16-byte pieces; a workgroup works on ONE send row, so the peer and the n-th member of
 * its mask are found once per workgroup, not once per piece.
 * 16-bit elements only (TF_ERR_DTYPE otherwise); D and ld multiples of 8 elements, ns <= 6, Kl <= 64, a mask bit at or above
 * Kl: TF_ERR_SHAPE; pointers and frame strides 16-byte aligned: TF_ERR_ALIGN.  All checked before anything touches the device.
 * ------------------------------------------------------------------------ */
TF_API int tf_frame_set_halo_pack(const void* const* slabs, const int64_t* frame_strides, int ns, void* send, int n_peer,
                           const uint64_t* masks, int Kl, int S, int D, int64_t ld, int dtype, void* stream);

/* ------------------------------------------------------------------------
 * Halo pack of a windowed / anchored frame shard that carries a MULTI-EDIT batch (additive to ABI 11;
 * tf_rank_pivotal_frame_sets_edits below).  The work of tf_frame_set_halo_pack -- per peer a 64-bit mask over the Kl <= 64 local
 * frames, send rows in ascending member order, masks and row prefix in the kernel arguments -- for up to 4 * TF_MAX_EDITS slabs
 * (the compact k slots and two value slabs per edit).  A plain window's ranges are contiguous masks: this one entry serves the
 * windowed and the anchored pass.
 * In extra workgroups behind the packing ones the SAME launch copies nq <= 1 + 2 * TF_MAX_EDITS compact q slabs ([Kl, S, ld_q]
 * tensors with their own frame strides) into the dense staging region q_stage [nq][Kl][S][D]: what a mixed injection mask needs
 * (the source's q beside the non-injecting edits', under ONE branch stride).  nq = 0 launches none of them and ignores
 * q_slabs / q_frame_strides / q_stage / ld_q.  No send rows and nq = 0: no launch.
 * Validation and error codes of tf_frame_set_halo_pack: 16-bit elements only (TF_ERR_DTYPE); D, ld (and ld_q) multiples of 8
 * elements, ns outside 1 .. 4 * TF_MAX_EDITS, nq outside 0 .. 1 + 2 * TF_MAX_EDITS, Kl > 64, a mask bit at or above Kl:
 * TF_ERR_SHAPE; pointers and frame strides 16-byte aligned: TF_ERR_ALIGN.  All checked before anything touches the device.
 * tf_window_halo_pack and tf_frame_set_halo_pack are untouched (ns <= 6).
 * ------------------------------------------------------------------------ */
TF_API int tf_edit_halo_pack(const void* const* slabs, const int64_t* frame_strides, int ns, void* send, int n_peer,
                      const uint64_t* masks, const void* const* q_slabs, const int64_t* q_frame_strides, int nq, void* q_stage,
                      int Kl, int S, int D, int64_t ld, int64_t ld_q, int dtype, void* stream);

/* ------------------------------------------------------------------------
 * Nearest-neighbour token search  --  replaces batch_cosine_sim + chunk + argmax:
 * util.py:61-69 and tokenflow_utils.py:335-343.
 *
 * tf_pivot_inv_norm: once per pivotal pass and block, inv_norm[r] = 1/||piv[r]||_2
 *   for the rows of the source-branch pivots `pivot_hidden_states[0]` viewed as
 *   [rows = K*S, D] (util.py:67).
 *
 * tf_nn_search: for every target row t (norm_hidden_states[0] as [n_tgt = n*S, D],
 *   tokenflow_utils.py:335) and every selected keyframe p < P (kf[p] indexes the
 *   K keyframes; the reference order is [i, i-1], lines 331-333):
 *       idx[p, t] = argmax_j  <tgt[t], piv[kf[p], j]> * inv_norm[kf[p]*S + j]
 *   first maximal j wins (torch.argmax).  n_tgt < 2^31 (per chunk in the chunk forms).  The 1/||tgt[t]|| factor of util.py:66
 *   is a positive per-row constant and cannot change the argmax, so targets are
 *   never normalised.  idx is int32 [P, n_tgt].  D multiple of 8; dtype bf16/f16.
 *   tgt, piv, ws AND inv_norm 16-byte aligned (TF_ERR_ALIGN otherwise; the same holds for the tf_nn_gather_blend*
 *   forms): the LDS-DMA search kernel fetches the inverse norms of a pivot tile in 16-byte pieces.
 *   ws: scratch for per-split candidates when the pivot range is split over workgroups
 *   (size from tf_nn_search_workspace_bytes, >= 256 bytes).
 * ------------------------------------------------------------------------ */
TF_API int tf_pivot_inv_norm(const void* piv, float* inv_norm, int64_t rows, int D, int dtype,
                      void* stream);

TF_API size_t tf_nn_search_workspace_bytes(int64_t n_tgt, int S, int D, int P);

TF_API int tf_nn_search(const void* tgt, const void* piv, const float* inv_norm, int32_t* idx,
                 int64_t n_tgt, int S, int D, int P, int kf0, int kf1, int dtype,
                 void* ws, size_t ws_bytes, void* stream);

/* Launch plan of tf_nn_search (C = 1) or of the search launches of tf_nn_gather_blend_chunks over C > 1 chunks of
 * n_tgt targets (P = 2; the gather merges the splits itself, no finalize).  Host only, as tf_ext_attn_plan.  Tokens:
 *   rb / rbs<TJ=2|4> / rbg<TT=1|2> / glds / wide / bk64 / bk128 / deep, each followed by [splits=N] (",chunks" added
 *   when C > 1), and finalize (the merge of the per-split candidates of tf_nn_search). */
TF_API int tf_nn_search_plan(int64_t n_tgt, int S, int D, int P, int C, char* buf, size_t len);

/* ------------------------------------------------------------------------
 * Gather + blend + residual  --  replaces tokenflow_utils.py:362-397
 * (propagation branch): advanced-index of the cached keyframe outputs, the
 * int64 [3, n*S, D] index expansion + gather (372-373 / 390), the materialised
 * fp32 weight tensor (375-385), the blend (388) and the residual add (396-397).
 *
 *   kf_out : [3, K, S, D]      cached attn1 output of the pivotal pass (`in_dtype`)
 *   idx    : int32 [P, n*S]    from tf_nn_search (same indices for all 3 branches, 344-348)
 *   w      : float [n]         w1 per frame of the chunk (only read when P == 2)
 *   resid  : [3, n, S, D] or NULL (`res_dtype`)   hidden_states added at 396-397
 *   out    : [3, n, S, D]      (`out_dtype`)
 *   P == 2:  out = (w*a1 + (1-w)*a2) + resid   evaluated in fp32 with the
 *            reference's operation order and no fused multiply-add, so an fp32
 *            `out` is bit-identical to the reference's.
 *   P == 1:  out = a1 + resid  (fp32 add, rounded to out_dtype).
 * ------------------------------------------------------------------------ */
TF_API int tf_gather_blend(const void* kf_out, const int32_t* idx, const float* w, const void* resid,
                    void* out, int K, int n, int S, int D, int P, int kf0, int kf1,
                    int in_dtype, int res_dtype, int out_dtype, void* stream);

/* ------------------------------------------------------------------------
 * Propagation branch in one call  --  tokenflow_utils.py:329-397 for one chunk:
 * tf_nn_search followed by tf_gather_blend, without the index tensor in between.
 * The search leaves its per-split candidates in `ws` and the gather merges them
 * itself (same order, same tie rule), which saves the finalize launch -- about
 * 4 us per call, i.e. what a launch costs on this GPU even when it does nothing.
 * Results are bit-identical to the two separate calls.  n_tgt = n*S; arguments as
 * in the two functions above; `search_dtype` is the dtype of tgt and piv.
 * ------------------------------------------------------------------------ */
TF_API size_t tf_nn_gather_blend_workspace_bytes(int64_t n_tgt, int S, int D, int P);

TF_API int tf_nn_gather_blend(const void* tgt, const void* piv, const float* inv_norm,
                       const void* kf_out, const float* w, const void* resid, void* out,
                       int K, int n, int S, int D, int P, int kf0, int kf1,
                       int search_dtype, int in_dtype, int res_dtype, int out_dtype,
                       void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Propagation branch for a RUN of consecutive chunks in one call  --  tokenflow_utils.py:329-397 executed for
 * C chunks at once.  The reference runs one UNet pass per chunk of n = batch_size frames
 * (run_tokenflow_pnp.py:228-231) because a pass over all frames does not fit its GPUs; with 288 GB a caller can
 * carry every chunk in one pass (or, as bench.py and the frame-sharded path do, simply owns all chunks' tensors),
 * and the C searches + gathers become two launches whose grids are C times larger (no short tail round per chunk).
 *
 *   tgt    : [C*n*S, D]        norm_hidden_states[0], chunk-major (chunk j = rows j*n*S .. (j+1)*n*S-1)
 *   resid, out : [3, C*n, S, D]
 *   chunk j matches keyframe slots slot0 + j and slot0 + j - 1 of piv / inv_norm / kf_out ([.., K, ..]; the reference
 *   order [i, i-1], 331-333).  first_single != 0: chunk 0 of the call is chunk 0 of the video and matches slot0
 *   alone (line 390); its rows are rounded to `single_dtype` -- the dtype the reference's pass produces for that
 *   chunk, torch promotion of the cached output and hidden_states -- before being stored as `out_dtype`.
 *   Results are bit-identical to C calls of tf_nn_gather_blend.  C = 1 with first_single is tf_nn_gather_blend(P = 1).
 *   w : float [n], as tf_gather_blend.
 * ------------------------------------------------------------------------ */
TF_API size_t tf_nn_gather_blend_chunks_workspace_bytes(int64_t n_tgt_chunk, int S, int D, int C);

TF_API int tf_nn_gather_blend_chunks(const void* tgt, const void* piv, const float* inv_norm, const void* kf_out,
                              const float* w, const void* resid, void* out, int K, int n, int C, int S, int D,
                              int slot0, int first_single, int search_dtype, int in_dtype, int res_dtype,
                              int out_dtype, int single_dtype, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * The two calls above with the block's NEXT LayerNorm fused behind them  --  tokenflow_utils.py:329-397 followed by
 * norm2 (399-403) or, without cross-attention, norm3 (414): `out` is written exactly as by tf_nn_gather_blend[_chunks]
 * and norm_out = LayerNorm(out) row by row exactly as tf_layer_norm(out) would produce it (bit-identical on both),
 * but a row never leaves the registers in between: the propagation leaves the residual stream in fp32 (the
 * reference's promotion, 385-397) and a separate norm re-reads 4 bytes per element to emit 2.
 * Covers the hook path's types: in_dtype = res_dtype = norm_dtype = the 16-bit model type, resid != NULL,
 * out_dtype = TF_F32 when two keyframes are blended (always for the chunks form), the model type for P = 1;
 * D <= 1536 (TF_ERR_DTYPE otherwise: issue the two calls).  gamma, beta: [D] of w_dtype or NULL.  Workspace as the
 * unfused calls.
 * ------------------------------------------------------------------------ */
TF_API int tf_nn_gather_blend_norm(const void* tgt, const void* piv, const float* inv_norm, const void* kf_out,
                            const float* w, const void* resid, void* out, int K, int n, int S, int D, int P, int kf0,
                            int kf1, int search_dtype, int in_dtype, int res_dtype, int out_dtype, const void* gamma,
                            const void* beta, float eps, int w_dtype, void* norm_out, int norm_dtype, void* ws,
                            size_t ws_bytes, void* stream);

TF_API int tf_nn_gather_blend_chunks_norm(const void* tgt, const void* piv, const float* inv_norm, const void* kf_out,
                                   const float* w, const void* resid, void* out, int K, int n, int C, int S, int D,
                                   int slot0, int first_single, int search_dtype, int in_dtype, int res_dtype,
                                   int out_dtype, int single_dtype, const void* gamma, const void* beta, float eps,
                                   int w_dtype, void* norm_out, int norm_dtype, void* ws, size_t ws_bytes,
                                   void* stream);

/* ------------------------------------------------------------------------
 * The chunk forms for a multi-edit batch (ABI 10): the arguments of tf_nn_gather_blend_chunks[_norm] plus n_edits
 * (1 .. TF_MAX_EDITS); B = 1 + 2*n_edits branches.
 *   kf_out : [B, K, S, D];   resid, out, norm_out : [B, C*n, S, D];   everything else as the chunk forms.
 *   C >= 1.  C = 1 runs the one-chunk form: with first_single the one-keyframe chunk 0 of the video (P = 1; `w` may be
 *   NULL, out_dtype must equal single_dtype), else one two-keyframe chunk.
 * The NN search reads the source branch only, so ONE search is issued -- the launches of tf_nn_search_plan(n*S, S, D, 2, C)
 * (without its finalize; of P = 1 for the one-keyframe chunk alone) -- and the gather loops the B branches on the same
 * candidates.  Branch b of the result is BIT-IDENTICAL to the same branch of the single-edit call on
 * [source | uncond_e | cond_e].  Workspace: tf_nn_gather_blend_chunks_workspace_bytes (C = 1 with first_single:
 * tf_nn_gather_blend_workspace_bytes(n*S, S, D, 1)) -- the search is unchanged.
 * tf_nn_gather_blend_edits_plan: the launches of the call (host only): the search tokens of tf_nn_search_plan followed by
 * gather[branches=B].
 * ------------------------------------------------------------------------ */
TF_API int tf_nn_gather_blend_chunks_edits(const void* tgt, const void* piv, const float* inv_norm, const void* kf_out,
                                    const float* w, const void* resid, void* out, int K, int n, int C, int S, int D,
                                    int slot0, int first_single, int search_dtype, int in_dtype, int res_dtype,
                                    int out_dtype, int single_dtype, int n_edits, void* ws, size_t ws_bytes,
                                    void* stream);

TF_API int tf_nn_gather_blend_chunks_norm_edits(const void* tgt, const void* piv, const float* inv_norm,
                                         const void* kf_out, const float* w, const void* resid, void* out, int K, int n,
                                         int C, int S, int D, int slot0, int first_single, int search_dtype,
                                         int in_dtype, int res_dtype, int out_dtype, int single_dtype, int n_edits,
                                         const void* gamma, const void* beta, float eps, int w_dtype, void* norm_out,
                                         int norm_dtype, void* ws, size_t ws_bytes, void* stream);

TF_API int tf_nn_gather_blend_edits_plan(int n, int C, int S, int D, int first_single, int n_edits, char* buf, size_t len);

/* ------------------------------------------------------------------------
 * Keyframe SEGMENTS (additive to ABI 11): several scenes or clips in one pass.  A pass carries n_seg segments,
 * 1 <= n_seg <= TF_MAX_SEGMENTS; segment v owns seg_K[v] >= 1 CONSECUTIVE keyframes of the bank (sum = K) and the chunks that
 * belong to them.  The batch layout is the usual [source | uncond | cond] x frames; a segment is a frame window of it.  For
 * every op the slices of segment v are what the single-clip op computes on segment v's tensors alone: nothing crosses a cut.
 *
 * tf_ext_attn_fwd_segments: q, k, v dense [3, K, S, ld], out dense [3, K, S, H*Dh] (float with TF_ATTN_OUT_F32); seg_K a HOST
 *   array of n_seg ints.  A bank branch of keyframe f attends to the seg_K[v] * S keys of its own segment, the source branch
 *   to its own S keys.
 *   flags: TF_ATTN_INJECT, TF_ATTN_OUT_F32, TF_ATTN_NO_SPLIT, TF_ATTN_NO_FUSED / TF_ATTN_FUSED, TF_ATTN_FOLD_SCALE and the hints
 *     as tf_ext_attn_fwd, applied to every segment.  TF_ATTN_BANK_ONLY, TF_ATTN_SOURCE_ONLY and the multi-edit hints
 *     (TF_ATTN_MULTI_V, TF_ATTN_NO_MULTI_V, TF_ATTN_MULTI_V64, TF_ATTN_RUN_MULTI_V): TF_ERR_SHAPE -- frame-sharded and
 *     multi-edit passes have no segment form.  n_seg outside 1 .. TF_MAX_SEGMENTS, a segment without keyframes, a sum other
 *     than K: TF_ERR_SHAPE.  Every refusal comes before anything touches the device.
 *   n_seg = 1 IS tf_ext_attn_fwd(K, Kq = K): same launches, same bits.
 *   Composition for n_seg > 1.  Every segment is asked what its OWN call -- tf_ext_attn_fwd_strided on its frame window,
 *   (K, Kq) = (seg_K[v], seg_K[v]) -- would take.
 *     - The segments whose own call takes the fused small-problem kernel share ONE fused launch, a tensor set per segment
 *       (branches 0..2, base pointers at the segment's first frame, Kq = Kb = seg_K[v], q_frame0 = 0); plan token
 *       fused[..,sets=N], N such segments (N = 1 and 2 included).  The launch is planned on the JOINT grid: under
 *       TF_ATTN_NO_SPLIT the plan is a function of the shape alone and the launch equals the segments' own calls bit for bit;
 *       in the default mode it may choose another KW than a segment alone would (results within the attention bound), or
 *       leave the fused range as a one-shot call of that size would -- those segments then stream with the others.
 *     - The other segments stream: ONE V^T pre-pass over the whole bank (all three branches of all K frames; key norms as
 *       the single-clip call leaves them), then, in segment order, the launches the segment's own call issues behind its
 *       pre-pass, with the frame window folded into the base pointers and the image's row stride as the run calls fold
 *       theirs.  Same kernels, same values: BIT-IDENTICAL to the segment's own call, in the default mode and under
 *       TF_ATTN_NO_SPLIT alike.  The fused launch, where there is one, follows the streaming launches.
 *   ws: tf_ext_attn_segments_workspace_bytes(K, ...) -- the image and norm table of the whole bank and the split form's
 *     partial results once (the segments run one behind the other on the stream); it does not depend on the segmentation
 *     and is never smaller than tf_ext_attn_workspace_bytes(K, ...).
 * tf_ext_attn_segments_plan: the launches of the call (host only), the tokens of tf_ext_attn_plan.
 *
 * tf_nn_gather_blend_chunks_segments / tf_nn_gather_blend_chunks_norm_segments: the arguments of tf_nn_gather_blend_chunks
 *   [_norm] with first_single replaced by single_mask: bit j set = chunk j of the call is the first chunk of a segment, a
 *   ONE-keyframe chunk that matches slot0 + j alone (tokenflow_utils.py:331-333, 390) and whose rows are rounded to
 *   single_dtype as chunk 0's are; every other chunk j matches slots slot0 + j and slot0 + j - 1.  w depends on n only: one
 *   w[n] serves every chunk.  1 <= C <= 64; slot0 >= 1 unless bit 0 is set; a bit at or above C: TF_ERR_SHAPE.
 *   ONE search -- the launches of tf_nn_search_plan(n*S, S, D, 2, C), no finalize; the p = 1 half of a one-keyframe chunk is
 *   neither computed nor read -- and ONE gather.  Bit-identical to the per-segment calls (tf_nn_gather_blend_chunks with
 *   first_single on each segment's chunks) wherever the C-chunk search and theirs take the same kernel form; mask 1 and mask 0
 *   ARE tf_nn_gather_blend_chunks with and without first_single.  Workspace: tf_nn_gather_blend_chunks_workspace_bytes.
 * tf_nn_gather_blend_segments_plan: the launches of the call (host only): the search tokens followed by gather[branches=3].
 * ------------------------------------------------------------------------ */
#define TF_MAX_SEGMENTS 8

TF_API size_t tf_ext_attn_segments_workspace_bytes(int K, int S, int H, int Dh, int dtype);

TF_API int tf_ext_attn_fwd_segments(const void* q, const void* k, const void* v, void* out, int K, int n_seg, const int* seg_K,
                             int S, int H, int Dh, int64_t ld, float scale, int flags, int dtype, void* ws, size_t ws_bytes,
                             void* stream);

TF_API int tf_ext_attn_segments_plan(int K, int n_seg, const int* seg_K, int S, int H, int Dh, int flags, int dtype, char* buf,
                              size_t len);

TF_API int tf_nn_gather_blend_chunks_segments(const void* tgt, const void* piv, const float* inv_norm, const void* kf_out,
                                       const float* w, const void* resid, void* out, int K, int n, int C, int S, int D,
                                       int slot0, uint64_t single_mask, int search_dtype, int in_dtype, int res_dtype,
                                       int out_dtype, int single_dtype, void* ws, size_t ws_bytes, void* stream);

TF_API int tf_nn_gather_blend_chunks_norm_segments(const void* tgt, const void* piv, const float* inv_norm,
                                            const void* kf_out, const float* w, const void* resid, void* out, int K, int n,
                                            int C, int S, int D, int slot0, uint64_t single_mask, int search_dtype,
                                            int in_dtype, int res_dtype, int out_dtype, int single_dtype, const void* gamma,
                                            const void* beta, float eps, int w_dtype, void* norm_out, int norm_dtype, void* ws,
                                            size_t ws_bytes, void* stream);

TF_API int tf_nn_gather_blend_segments_plan(int n, int C, int S, int D, uint64_t single_mask, char* buf, size_t len);

/* ------------------------------------------------------------------------
 * RAGGED chunk runs (additive to ABI 11): one propagation call for chunks of UNEQUAL frame count -- the tail of a video whose
 * length is no multiple of the chunk size, scenes whose lengths are whatever the cuts give.  Chunk j of the call has
 * chunk_frames[j] >= 1 frames (a HOST array of C ints, 1 <= C <= 64); F = sum_j chunk_frames[j].  Everything else is
 * tf_nn_gather_blend_chunks_segments: single_mask, slots slot0 + j and slot0 + j - 1, single_dtype rounding of the
 * one-keyframe chunks.
 *
 *   tgt : [F*S, D] chunk-major;   resid, out, norm_out : [B, F, S, D], B = 1 + 2*n_edits;   kf_out : [B, K, S, D].
 *   n_edits = 1 is the 3-branch gather; n_edits > 1 (<= TF_MAX_EDITS) the multi-edit form of tf_nn_gather_blend_chunks_edits,
 *   for which only bit 0 of single_mask may be set (segments and multi-edit batches do not combine).
 *   w : a DEVICE array of F floats, one per frame of the CALL: the entry of frame i of chunk j is the blend weight of index i
 *   at chunk size chunk_frames[j] (the caller concatenates the per-size weight vectors; with equal sizes the first n entries
 *   are today's w[n]).
 *
 * Semantics: the rows of chunk j equal what the one-chunk call computes on chunk j's tensors alone -- tf_nn_gather_blend
 * with n = chunk_frames[j], that size's w, P = 1 where bit j of the mask is set.  The gather arithmetic is that call's bit
 * for bit; the indices are that call's wherever the two searches take the same kernel form (the caveat of every chunk form).
 *
 * Launches.  Equal frame counts ARE today's call: tf_nn_gather_blend_chunks_segments (n_edits = 1) or
 * tf_nn_gather_blend_chunks_edits -- same launches, same plan tokens, same bits.  Otherwise ONE search and ONE gather:
 *   - kernel form: the one the uniform C-chunk search takes at the MEAN chunk size, tf_nn_search_plan(ceil(F*S / C), S, D,
 *     2, C) -- a host-only rule on (chunk_frames, S, D);
 *   - grid.x = sum_j ceil(chunk_frames[j]*S / TN) target panels of that form: a chunk's last panel is partial, no panel
 *     straddles two chunks; the pivot-range split is the form's rule applied to that workgroup count;
 *   - chunk descriptor: two prefix tables (targets, panels) and the mask in the kernel-argument segment, about 0.5 KiB; a
 *     workgroup of the search bisects the panel table with scalar loads, a thread of the gather the target table.  The call
 *     copies nothing to the device: it issues kernels only and can be captured.
 * Plan tokens (tf_nn_gather_blend_ragged_plan, host only): the search token with ",ragged" in its brackets, e.g.
 * rb[splits=1,ragged], then gather[branches=B,ragged] (gather_norm[branches=B,ragged] for the norm form's gather).
 *
 * Refusals, all before anything touches the device: TF_ERR_SHAPE for C outside 1..64, a chunk of less than one frame, a mask
 * bit at or above C, slot0 + C > K, slot0 < 1 without bit 0, F*S >= 2^31, n_edits outside 1..TF_MAX_EDITS, a mask above 1 with
 * n_edits > 1; alignment, dtype and workspace errors as the segments form.  Workspace:
 * tf_nn_gather_blend_ragged_workspace_bytes (0 for a refused shape).
 * ------------------------------------------------------------------------ */
TF_API size_t tf_nn_gather_blend_ragged_workspace_bytes(const int* chunk_frames, int C, int S, int D);

TF_API int tf_nn_gather_blend_chunks_ragged(const void* tgt, const void* piv, const float* inv_norm, const void* kf_out,
                                     const float* w, const void* resid, void* out, int K, const int* chunk_frames, int C,
                                     int S, int D, int slot0, uint64_t single_mask, int search_dtype, int in_dtype,
                                     int res_dtype, int out_dtype, int single_dtype, int n_edits, void* ws, size_t ws_bytes,
                                     void* stream);

TF_API int tf_nn_gather_blend_chunks_norm_ragged(const void* tgt, const void* piv, const float* inv_norm, const void* kf_out,
                                          const float* w, const void* resid, void* out, int K, const int* chunk_frames,
                                          int C, int S, int D, int slot0, uint64_t single_mask, int search_dtype,
                                          int in_dtype, int res_dtype, int out_dtype, int single_dtype, int n_edits,
                                          const void* gamma, const void* beta, float eps, int w_dtype, void* norm_out,
                                          int norm_dtype, void* ws, size_t ws_bytes, void* stream);

TF_API int tf_nn_gather_blend_ragged_plan(const int* chunk_frames, int C, int S, int D, uint64_t single_mask, int n_edits,
                                   char* buf, size_t len);

/* ------------------------------------------------------------------------
 * Sliding-window keyframe BANK (additive to ABI 11): the extended attention of long videos.  A keyframe's uncond / cond
 * branches attend to the keys of its NEIGHBOURING keyframes only -- overlapping windows, where keyframe segments are disjoint
 * ones -- so the pivotal pass costs sum_i win_n[i] frame-banks instead of K * Kq.  This CHANGES THE RESULT relative to
 * TokenFlow (there every keyframe attends to the whole bank); it is opt-in, and with every window = [0, K) it IS the
 * reference computation.
 *
 * tf_ext_attn_fwd_windows: the arguments of tf_ext_attn_fwd_strided plus two HOST arrays of Kq ints.
 *   The uncond / cond branches of query frame i (bank frame q_frame0 + i) attend to the keys of bank frames
 *   [win_lo[i], win_lo[i] + win_n[i]); under TF_ATTN_INJECT with the source's q and k, over the same windows.  The source
 *   branch attends to its own frame, as always.
 *   Refused with TF_ERR_SHAPE, before anything touches the device: Kq > TF_MAX_WINDOW_FRAMES; win_n[i] < 1; a window outside
 *     [0, K); a window that does not hold its own frame q_frame0 + i (a keyframe always sees itself); TF_ATTN_BANK_ONLY,
 *     TF_ATTN_SOURCE_ONLY, TF_ATTN_FOLD_SCALE and the multi-edit hints (TF_ATTN_MULTI_V, TF_ATTN_NO_MULTI_V, TF_ATTN_MULTI_V64,
 *     TF_ATTN_RUN_MULTI_V).  The other flags and hints act as in tf_ext_attn_fwd.
 *   Every window = [0, K) IS tf_ext_attn_fwd_strided: same launches, same bits, same plan tokens.
 *   Otherwise the call issues the launches tf_ext_attn_fwd_strided would issue for a bank of K' = max_i win_n[i] frames at the
 *   same Kq, S, H, Dh and flags (the fused-kernel decision, the split plan and the kernel forms are those of K'; under
 *   TF_ATTN_NO_SPLIT a function of the shape alone):
 *     - ONE V^T pre-pass over the whole bank of K frames;
 *     - ONE bank launch (or ONE fused launch, which needs no pre-pass) whose window table rides in the kernel arguments --
 *       no device table, no copy, no sync: the call can be captured.  A bank problem of query frame i streams the frames of
 *       window i; the split form splits the WINDOW into its nseg runs (a window shorter than nseg leaves empty runs, which the
 *       merge weighs with 0).  Plan token: the plain launch's with ",win" appended -- il<..>,win, one<..>,win, pp<..>,win,
 *       fused[..,win];
 *     - the merge and the source launches as in the plain call.
 *   Workgroups keep frame order.
 *   Identity.  Frame i's OWN CALL is tf_ext_attn_fwd_strided on the window's tensors with (K, Kq, q_frame0) =
 *   (win_n[i], 1, q_frame0 + i - win_lo[i]).  Frame i's result is within the attention bound of its own call always, and
 *   BIT-IDENTICAL to it under TF_ATTN_NO_SPLIT wherever the two plans name the same kernel form: a one-pass launch's
 *   arithmetic for a (query, head) depends only on the sequence of key tiles, the fused kernel's on KW and PREC only.
 *   ws: tf_ext_attn_workspace_bytes(K, ...), unchanged.
 * tf_ext_attn_windows_plan: the launches of the call for dense tensors (host only), the tokens of tf_ext_attn_plan.
 * ------------------------------------------------------------------------ */
#define TF_MAX_WINDOW_FRAMES 64

TF_API int tf_ext_attn_fwd_windows(const void* q, const void* k, const void* v, void* out, int K, int Kq, int q_frame0, int S,
                            int H, int Dh, int64_t ld, const int64_t* strides, float scale, int flags, int dtype,
                            const int* win_lo, const int* win_n, void* ws, size_t ws_bytes, void* stream);

TF_API int tf_ext_attn_windows_plan(int K, int Kq, int q_frame0, int S, int H, int Dh, int flags, int dtype, const int* win_lo,
                             const int* win_n, char* buf, size_t len);

/* ------------------------------------------------------------------------
 * The BANK PART of a windowed pass (additive to ABI 11): what a frame-sharded rank runs over its halo-extended receive buffer
 * (tf_rank_pivotal_window, `FrameShard._pivotal_window`).
 *
 * tf_ext_attn_fwd_windows_part takes the arguments of tf_ext_attn_fwd_windows, but TF_ATTN_BANK_ONLY is accepted: k and v then
 * hold only the slabs the bank branches read, with the branch offsets of tf_ext_attn_fwd_strided under that flag (branch b of a
 * tensor at base + b * branch stride; under injection k holds the source slab, branch 0, alone).  Without the flag the call IS
 * tf_ext_attn_fwd_windows.  TF_ATTN_SOURCE_ONLY is refused (TF_ERR_SHAPE): the source part of a windowed pass is window-free --
 * it is tf_ext_attn_fwd_strided with TF_ATTN_SOURCE_ONLY.  tf_ext_attn_fwd_windows itself keeps refusing both part flags.
 *   Identity.  The two parts together -- this call with TF_ATTN_BANK_ONLY, then the source-only strided call -- equal
 *   tf_ext_attn_fwd_windows on the same tensors BIT FOR BIT under TF_ATTN_NO_SPLIT wherever the plans name the same kernel form
 *   (the tokens apart from their part field; fused launches agree in KW and PREC), and lie within the attention bound of it
 *   everywhere.  Every window = the whole bank is tf_ext_attn_fwd_strided with the same part flag.
 *   ws: tf_ext_attn_workspace_bytes(K, ...).
 * tf_ext_attn_windows_part_plan: the launches of the call for dense tensors (host only); the bank launch's token carries
 *   ',win' as in tf_ext_attn_windows_plan.
 * ------------------------------------------------------------------------ */
TF_API int tf_ext_attn_fwd_windows_part(const void* q, const void* k, const void* v, void* out, int K, int Kq, int q_frame0,
                                 int S, int H, int Dh, int64_t ld, const int64_t* strides, float scale, int flags, int dtype,
                                 const int* win_lo, const int* win_n, void* ws, size_t ws_bytes, void* stream);

TF_API int tf_ext_attn_windows_part_plan(int K, int Kq, int q_frame0, int S, int H, int Dh, int flags, int dtype,
                                  const int* win_lo, const int* win_n, char* buf, size_t len);

/* ------------------------------------------------------------------------
 * Sliding-window bank for a MULTI-EDIT batch (additive to ABI 11): several prompts on one long video in one pass.
 *
 * tf_ext_attn_fwd_windows_edits: q, k, v, out, strides, n_edits and inject_mask as tf_ext_attn_fwd_edits_masked -- B = 1 + 2E
 *   branches [source | uncond_1 | cond_1 | ...], bit e of the mask = edit e uses the source's q and k -- and win_lo, win_n as
 *   tf_ext_attn_fwd_windows (HOST arrays of Kq ints, validated the same way).  The uncond / cond branches of EVERY edit attend,
 *   for query frame i, to bank frames [win_lo[i], win_lo[i] + win_n[i]); the source branch to its own frame, once; nothing
 *   mixes edits.
 *   Refused with TF_ERR_SHAPE, before anything touches the device: what tf_ext_attn_fwd_windows refuses of its table (a bad
 *     window, Kq > TF_MAX_WINDOW_FRAMES) and of its flags (TF_ATTN_BANK_ONLY, TF_ATTN_SOURCE_ONLY, TF_ATTN_FOLD_SCALE,
 *     TF_ATTN_RUN_MULTI_V), and what the masked call refuses (TF_ATTN_INJECT beside the mask, mask bits at or above n_edits,
 *     n_edits outside 1 .. TF_MAX_EDITS, TF_ATTN_NO_MULTI_V beside TF_ATTN_MULTI_V or TF_ATTN_MULTI_V64).  TF_ATTN_MULTI_V,
 *     TF_ATTN_NO_MULTI_V and TF_ATTN_MULTI_V64 are ACCEPTED here (tf_ext_attn_fwd_windows keeps refusing them).
 *   n_edits = 1 IS tf_ext_attn_fwd_windows, and every window = [0, K) IS tf_ext_attn_fwd_edits_masked: same launches, same
 *   bits, same plan tokens.
 *   Otherwise the call is the masked composition with the window table handed to every bank part; as in the windowed call the
 *   fused-kernel decision, the split and the kernel forms are planned for K' = max_i win_n[i], windowed launches carry ",win"
 *   in the plan, and the table rides in the kernel arguments (no device table, no copy, no sync):
 *     - ONE V^T pre-pass over the span of the streaming branches;
 *     - the injecting edits first: pairs in the windowed four-bank form where it is selected (below), an odd one in the DUAL
 *       launch beside them; without the form each through the launches of its own windowed bank-only call;
 *     - the edits that do not inject, each through its windowed bank-only launches;
 *     - the source branch last, through the plain, unwindowed source-only launches.
 *   Identity.  Edit e's bank branches are BIT-IDENTICAL to those of tf_ext_attn_fwd_windows on [source | uncond_e | cond_e]
 *   with edit e's own injection flag, and its source branch to that call's source slice, under TF_ATTN_NO_SPLIT wherever both
 *   plans name the same kernel form; always within the attention bound of the oracle on the window's slices.
 *   The windowed four-bank form: one<40,1,4,MV4,2,fq0>,win (Dh = 40, the packed image) and one<64,1,8,MV4,2,fq1>,win (Dh = 64,
 *   four 64-row banks).  One workgroup computes QK^T and the softmax of query frame f once, over the window of f, and the four
 *   P.V products of branches b, b + 1, b + gap, b + gap + 1: all four banks read the SAME window.  Pair launches are one-pass
 *   (TF_ATTN_NO_SPLIT | TF_ATTN_NO_FUSED), as in the masked call.  Frame i's OWN CALL is tf_ext_attn_fwd_edits_masked with the
 *   four-bank hint on the window's tensors, (K, Kq, q_frame0) = (win_n[i], 1, q_frame0 + i - win_lo[i]): the windowed pair
 *   launch is bit-identical to it (same kernel form; a one-pass launch's arithmetic depends only on the sequence of key tiles).
 *   TF_ATTN_MULTI_V (Dh = 40) / TF_ATTN_MULTI_V64 (Dh = 64) force the form on, TF_ATTN_NO_MULTI_V forces it off.  The measured
 *   defaults of the whole-bank call say nothing about windows: without a hint a windowed call takes the form only in the
 *   shape classes where profiles/r19_window_edits_ab.txt shows it ahead of the DUAL composition by more than the run-to-run
 *   spread (the rule and its figures stand in csrc/ext_attn.hip beside the other two).
 *   ws: tf_ext_attn_edits_workspace_bytes(K, ...), unchanged.
 * tf_ext_attn_windows_edits_plan: the launches of the call for dense tensors (host only), the tokens of tf_ext_attn_plan.
 * ------------------------------------------------------------------------ */
TF_API int tf_ext_attn_fwd_windows_edits(const void* q, const void* k, const void* v, void* out, int K, int Kq, int q_frame0,
                                  int S, int H, int Dh, int64_t ld, const int64_t* strides, float scale, int flags, int dtype,
                                  int n_edits, unsigned inject_mask, const int* win_lo, const int* win_n, void* ws,
                                  size_t ws_bytes, void* stream);

TF_API int tf_ext_attn_windows_edits_plan(int K, int Kq, int q_frame0, int S, int H, int Dh, int n_edits, unsigned inject_mask,
                                   int flags, int dtype, const int* win_lo, const int* win_n, char* buf, size_t len);

/* ------------------------------------------------------------------------
 * FRAME-SET keyframe bank (additive to ABI 11): a local window plus a few global ANCHOR keyframes, or any other keyframe
 * sparsity.  A purely local window has no global reference: consistency is only chained along the clip through the overlapping
 * windows.  The usual remedy is a window plus anchors that every keyframe sees (the first keyframe, every m-th one); the cost
 * stays linear in K: 2 radius + 1 + A frame-banks per keyframe.  The per-keyframe table is a SET of bank frames instead of a
 * range; dilated windows or windows clipped at scene cuts are expressed the same way.  Like the windowed call this CHANGES
 * THE RESULT relative to TokenFlow; it is opt-in, and with every set = [0, K) it IS the reference computation.
 *
 * tf_ext_attn_fwd_frame_sets: the arguments of tf_ext_attn_fwd_strided plus one HOST array of Kq 64-bit masks.
 *   Bit j of sets[i]: the uncond / cond branches of query frame i (bank frame q_frame0 + i) attend to the keys of bank frame j;
 *   under TF_ATTN_INJECT with the source's q and k, over the same sets.  The source branch attends to its own frame, as
 *   always.  Members are visited in ASCENDING frame order.
 *   Refused before anything touches the device: a null table (TF_ERR_NULL); with TF_ERR_SHAPE K > 64; Kq >
 *     TF_MAX_WINDOW_FRAMES; an empty set; a bit at or above K; a set without its own frame q_frame0 + i; and the flags
 *     tf_ext_attn_fwd_windows refuses (TF_ATTN_BANK_ONLY, TF_ATTN_SOURCE_ONLY, TF_ATTN_FOLD_SCALE and the multi-edit hints).
 *   Canonical forms.  If every set is a contiguous range the call IS tf_ext_attn_fwd_windows on the equivalent (lo, n) table:
 *   same launches, same bits, same plan tokens (",win" included); so every set = [0, K) IS tf_ext_attn_fwd_strided.
 *   Otherwise the call issues the launches tf_ext_attn_fwd_strided would issue for a bank of K' = max_i popcount(sets[i])
 *   frames at the same Kq, S, H, Dh and flags (the fused-kernel decision, the split plan and the kernel forms are those of K'):
 *     - ONE V^T pre-pass over the whole bank of K frames;
 *     - ONE bank launch (or ONE fused launch, which needs no pre-pass) whose set table rides in the kernel arguments (64 x 8
 *       bytes behind the parameter block) -- no device table, no copy, no sync.  A bank problem of query frame i streams the
 *       member frames of set i; at every frame boundary its tile cursors jump to the next member.  The split form: run seg of
 *       nseg takes members [seg n / nseg, (seg + 1) n / nseg) of the ascending member list, n = popcount(sets[i]); an empty
 *       run leaves the neutral partial result, which the merge weighs with 0.  Plan token: the plain launch's with ",set"
 *       appended -- il<..>,set, one<..>,set, pp<..>,set, fused[..,set];
 *     - the merge and the source launches as in the plain call.
 *   Identity.  Frame i's OWN CALL is tf_ext_attn_fwd_strided on the GATHERED tensors -- the member frames of set i copied next
 *   to each other in ascending order -- with (K, Kq, q_frame0) = (popcount(sets[i]), 1, rank of the own frame among the
 *   members).  Frame i's result is within the attention bound of its own call always, and BIT-IDENTICAL to it under
 *   TF_ATTN_NO_SPLIT wherever the two plans name the same kernel form: the key tiles arrive in the same order, and the
 *   Cauchy-Schwarz score bound (head dims 40 and 64) is the maximum key norm over the MEMBER frames only, not over the span
 *   from the first to the last member (a superset would give another shift).
 *   Multi-edit batches and the four-bank form over frame sets: tf_ext_attn_fwd_frame_sets_edits, below.
 *   Frame shards: tf_ext_attn_fwd_frame_sets_part and tf_rank_pivotal_frame_sets, below.
 *   Not built: keyframe segments and the run forms over frame sets.
 *   ws: tf_ext_attn_workspace_bytes(K, ...), unchanged.
 * tf_ext_attn_frame_sets_plan: the launches of the call for dense tensors (host only), the tokens of tf_ext_attn_plan.
 * ------------------------------------------------------------------------ */
TF_API int tf_ext_attn_fwd_frame_sets(const void* q, const void* k, const void* v, void* out, int K, int Kq, int q_frame0,
                               int S, int H, int Dh, int64_t ld, const int64_t* strides, float scale, int flags, int dtype,
                               const uint64_t* sets, void* ws, size_t ws_bytes, void* stream);

TF_API int tf_ext_attn_frame_sets_plan(int K, int Kq, int q_frame0, int S, int H, int Dh, int flags, int dtype,
                                const uint64_t* sets, char* buf, size_t len);

/* ------------------------------------------------------------------------
 * The BANK PART of a frame-set pass (additive to ABI 11): what a frame-sharded rank runs over its anchor-extended receive
 * buffer (tf_rank_pivotal_frame_sets, `FrameShard._pivotal_frame_sets`).  To tf_ext_attn_fwd_frame_sets what
 * tf_ext_attn_fwd_windows_part is to tf_ext_attn_fwd_windows.
 *
 * tf_ext_attn_fwd_frame_sets_part takes the arguments of tf_ext_attn_fwd_frame_sets, but TF_ATTN_BANK_ONLY is accepted: k and v
 * then hold only the slabs the bank branches read, with the branch offsets of tf_ext_attn_fwd_strided under that flag.  Without
 * the flag the call IS tf_ext_attn_fwd_frame_sets.  TF_ATTN_SOURCE_ONLY is refused (TF_ERR_SHAPE): the source part of a
 * frame-set pass is set-free -- it is tf_ext_attn_fwd_strided with TF_ATTN_SOURCE_ONLY.  tf_ext_attn_fwd_frame_sets itself
 * keeps refusing both part flags.  K is the bank the masks index (on a shard the rank's extended bank), at most 64.
 *   Canonical forms.  Every set a contiguous range IS tf_ext_attn_fwd_windows_part on the equivalent (lo, n) table: same
 *   launches, same bits, same plan tokens; every set the whole bank IS tf_ext_attn_fwd_strided with the same part flag.
 *   Identity.  The two parts together -- this call with TF_ATTN_BANK_ONLY, then the source-only strided call -- equal
 *   tf_ext_attn_fwd_frame_sets on the same tensors BIT FOR BIT under TF_ATTN_NO_SPLIT wherever the plans name the same kernel
 *   form, and lie within the attention bound of it everywhere.
 *   ws: tf_ext_attn_workspace_bytes(K, ...).
 * tf_ext_attn_frame_sets_part_plan: the launches of the call for dense tensors (host only); the bank launch's token carries
 *   ',set' as in tf_ext_attn_frame_sets_plan (',win' where every set is a range).
 * ------------------------------------------------------------------------ */
TF_API int tf_ext_attn_fwd_frame_sets_part(const void* q, const void* k, const void* v, void* out, int K, int Kq, int q_frame0,
                                    int S, int H, int Dh, int64_t ld, const int64_t* strides, float scale, int flags,
                                    int dtype, const uint64_t* sets, void* ws, size_t ws_bytes, void* stream);

TF_API int tf_ext_attn_frame_sets_part_plan(int K, int Kq, int q_frame0, int S, int H, int Dh, int flags, int dtype,
                                     const uint64_t* sets, char* buf, size_t len);

/* ------------------------------------------------------------------------
 * Frame-set bank for a MULTI-EDIT batch (additive to ABI 11): several prompts on one long video in one pass, with anchor
 * keyframes beside the window.  Like the windowed and the frame-set call this CHANGES THE RESULT relative to TokenFlow unless
 * every set is the whole bank.
 *
 * tf_ext_attn_fwd_frame_sets_edits: q, k, v, out, strides, n_edits and inject_mask as tf_ext_attn_fwd_edits_masked -- B = 1 + 2E
 *   branches [source | uncond_1 | cond_1 | ...], bit e of the mask = edit e uses the source's q and k -- and sets as
 *   tf_ext_attn_fwd_frame_sets (a HOST array of Kq 64-bit masks, validated the same way).  The uncond / cond branches of EVERY
 *   edit attend, for query frame i, to the member frames of sets[i] in ascending order; the source branch to its own frame,
 *   once; nothing mixes edits.
 *   Refused before anything touches the device: what tf_ext_attn_fwd_frame_sets refuses of its table (a null table:
 *     TF_ERR_NULL; with TF_ERR_SHAPE K > 64, Kq > TF_MAX_WINDOW_FRAMES, an empty set, a bit at or above K, a set without its own
 *     frame), the flags tf_ext_attn_fwd_windows_edits refuses (TF_ATTN_BANK_ONLY, TF_ATTN_SOURCE_ONLY, TF_ATTN_FOLD_SCALE,
 *     TF_ATTN_RUN_MULTI_V), and what the masked call refuses (TF_ATTN_INJECT beside the mask, mask bits at or above n_edits,
 *     n_edits outside 1 .. TF_MAX_EDITS, TF_ATTN_NO_MULTI_V beside TF_ATTN_MULTI_V or TF_ATTN_MULTI_V64).  TF_ATTN_MULTI_V,
 *     TF_ATTN_NO_MULTI_V and TF_ATTN_MULTI_V64 are ACCEPTED here (tf_ext_attn_fwd_frame_sets keeps refusing them).
 *   Canonical forms: same launches, same bits, same plan tokens.  n_edits = 1 IS tf_ext_attn_fwd_frame_sets.  If every set is a
 *   contiguous range the call IS tf_ext_attn_fwd_windows_edits on the equivalent (lo, n) table; so every set = [0, K) IS
 *   tf_ext_attn_fwd_edits_masked.
 *   Otherwise the call is the masked composition with the set table handed to every bank part; as in the frame-set call the
 *   fused-kernel decision, the split and the kernel forms are planned for K' = max_i popcount(sets[i]), frame-set launches
 *   carry ",set" in the plan, and the table rides in the kernel arguments (no device table, no copy, no sync):
 *     - ONE V^T pre-pass over the span of the streaming branches;
 *     - the injecting edits first: pairs in the frame-set four-bank form where it is selected (below), an odd one in the DUAL
 *       set launch beside them; without the form each through the launches of its own frame-set bank-only call;
 *     - the edits that do not inject, each through its frame-set bank-only launches (il<..>,set, one<..>,set, pp<..>,set,
 *       fused[..,set]);
 *     - the source branch last, through the plain source-only launches.
 *   Identity.  Edit e's bank branches are BIT-IDENTICAL to those of tf_ext_attn_fwd_frame_sets on [source | uncond_e | cond_e]
 *   with edit e's own injection flag, and its source branch to that call's source slice, under TF_ATTN_NO_SPLIT wherever both
 *   plans name the same kernel form; always within the attention bound of the oracle on the gathered member frames.
 *   The frame-set four-bank form: one<40,1,4,MV4,2,fq0>,set (Dh = 40, the packed six-M-tile image) and one<64,1,8,MV4,2,fq1>,set
 *   (Dh = 64, four 64-row banks, scores per 32-key half).  One workgroup computes QK^T and the softmax of query frame f once,
 *   over the member frames of set f, and the four P.V products of branches b, b + 1, b + gap, b + gap + 1: all four banks take
 *   the SAME hops.  The score bound is the maximum key norm over the member frames of the source's norm row.  Pair launches are
 *   one-pass (TF_ATTN_NO_SPLIT | TF_ATTN_NO_FUSED), as in the masked call.  Frame i's OWN CALL is tf_ext_attn_fwd_edits_masked
 *   with the four-bank hint on the GATHERED member frames of set i (ascending), (K, Kq, q_frame0) = (popcount(sets[i]), 1, rank
 *   of the own frame among the members): the frame-set pair launch is bit-identical to it.
 *   TF_ATTN_MULTI_V (Dh = 40) / TF_ATTN_MULTI_V64 (Dh = 64) force the form on, TF_ATTN_NO_MULTI_V forces it off.  The measured
 *   defaults of the whole-bank and of the windowed call say nothing about sets: the rule of this call (mv4_set_default in
 *   csrc/ext_attn.hip) is written from profiles/r21_frame_sets_edits_ab.txt alone.
 *   ws: tf_ext_attn_edits_workspace_bytes(K, ...), unchanged.
 * tf_ext_attn_frame_sets_edits_plan: the launches of the call for dense tensors (host only), the tokens of tf_ext_attn_plan.
 * ------------------------------------------------------------------------ */
TF_API int tf_ext_attn_fwd_frame_sets_edits(const void* q, const void* k, const void* v, void* out, int K, int Kq, int q_frame0,
                                     int S, int H, int Dh, int64_t ld, const int64_t* strides, float scale, int flags,
                                     int dtype, int n_edits, unsigned inject_mask, const uint64_t* sets, void* ws,
                                     size_t ws_bytes, void* stream);

TF_API int tf_ext_attn_frame_sets_edits_plan(int K, int Kq, int q_frame0, int S, int H, int Dh, int n_edits, unsigned inject_mask,
                                      int flags, int dtype, const uint64_t* sets, char* buf, size_t len);

/* ------------------------------------------------------------------------
 * The BANK PART of a windowed / frame-set MULTI-EDIT pass (additive to ABI 11): all E edits' bank branches over one table in one
 * call -- what a frame-sharded rank with several prompts runs over its halo- or anchor-extended receive buffer, instead of E
 * single-edit part calls.  Opt-in: no existing call reaches these entry points.
 *
 * tf_ext_attn_fwd_windows_edits_part takes the arguments of tf_ext_attn_fwd_windows_edits plus qk_compact (behind inject_mask, as in
 *   tf_ext_attn_fwd_edits_part: q and k hold slot 0 = the source, then (uncond, cond) of every NON-injecting edit in ascending
 *   order).  TF_ATTN_BANK_ONLY is accepted: v and out are addressed as [source | uncond_1 | cond_1 | ...] and the source slabs
 *   are never touched.  Without a part flag the call IS tf_ext_attn_fwd_windows_edits (dense q / k: qk_compact = 1 is refused
 *   there).  TF_ATTN_SOURCE_ONLY is refused (TF_ERR_SHAPE): the source part of a windowed pass is window-free -- it is
 *   tf_ext_attn_fwd_edits_part(TF_ATTN_SOURCE_ONLY).  Otherwise refused: what tf_ext_attn_fwd_windows_edits refuses of its table,
 *   its mask and its other flags (TF_ATTN_FOLD_SCALE, TF_ATTN_RUN_MULTI_V), and qk_compact outside 0 .. 1.  The four-bank hints
 *   stay accepted, under the rule of the windowed multi-edit call.
 * tf_ext_attn_fwd_frame_sets_edits_part: the same beside tf_ext_attn_fwd_frame_sets_edits (a HOST array of Kq 64-bit masks, K <= 64).
 *   Launches.  Where every edit's bank part takes the fused small-problem kernel (S <= 256 under TF_ATTN_NO_SPLIT), ALL of them
 *   run in ONE launch of E tensor sets under the one table, which rides in the kernel arguments: plan token
 *   fused[qw=..,kw=..,qb=..,prec=..,sets=E,win] / fused[..,sets=E,set], planned for K' = the longest window / largest set.  A
 *   (query, head)'s arithmetic in that kernel depends on KW and PREC only, so under TF_ATTN_NO_SPLIT the joint launch equals the E
 *   one-set fused[..,win] / fused[..,set] launches of tf_ext_attn_fwd_windows_part / tf_ext_attn_fwd_frame_sets_part BIT FOR BIT.
 *   Everything else is the streaming composition of the non-part call without its source launches: ONE V^T pre-pass over the
 *   streaming branches, the injecting edits (pairs in the four-bank form where it is selected), then the others.
 *   Canonical forms: same launches, same bits, same plan tokens.  n_edits = 1 IS tf_ext_attn_fwd_windows_part /
 *   tf_ext_attn_fwd_frame_sets_part (TF_ATTN_INJECT iff mask = 1).  Every set a contiguous range IS
 *   tf_ext_attn_fwd_windows_edits_part on the equivalent (lo, n) table.  Every window or set the whole bank IS
 *   tf_ext_attn_fwd_edits_part.
 *   Identity.  This call with TF_ATTN_BANK_ONLY plus tf_ext_attn_fwd_edits_part(TF_ATTN_SOURCE_ONLY) equal
 *   tf_ext_attn_fwd_windows_edits / tf_ext_attn_fwd_frame_sets_edits(TF_ATTN_NO_MULTI_V) on the same tensors bit for bit under
 *   TF_ATTN_NO_SPLIT wherever the plans name the same kernel form, and lie within the attention bound of it everywhere.
 *   ws: tf_ext_attn_edits_workspace_bytes(K, ...), unchanged.
 * tf_ext_attn_windows_edits_part_plan / tf_ext_attn_frame_sets_edits_part_plan: the launches for dense tensors (host only).
 *   NOT BUILT: segments on a shard; run forms over windows.  The single-GPU calls tf_ext_attn_fwd_windows_edits /
 *   tf_ext_attn_fwd_frame_sets_edits keep issuing one fused launch per edit (their plan tests pin it).
 * ------------------------------------------------------------------------ */
TF_API int tf_ext_attn_fwd_windows_edits_part(const void* q, const void* k, const void* v, void* out, int K, int Kq, int q_frame0,
                                       int S, int H, int Dh, int64_t ld, const int64_t* strides, float scale, int flags,
                                       int dtype, int n_edits, unsigned inject_mask, int qk_compact, const int* win_lo,
                                       const int* win_n, void* ws, size_t ws_bytes, void* stream);

TF_API int tf_ext_attn_windows_edits_part_plan(int K, int Kq, int q_frame0, int S, int H, int Dh, int n_edits,
                                        unsigned inject_mask, int qk_compact, int flags, int dtype, const int* win_lo,
                                        const int* win_n, char* buf, size_t len);

TF_API int tf_ext_attn_fwd_frame_sets_edits_part(const void* q, const void* k, const void* v, void* out, int K, int Kq,
                                          int q_frame0, int S, int H, int Dh, int64_t ld, const int64_t* strides, float scale,
                                          int flags, int dtype, int n_edits, unsigned inject_mask, int qk_compact,
                                          const uint64_t* sets, void* ws, size_t ws_bytes, void* stream);

TF_API int tf_ext_attn_frame_sets_edits_part_plan(int K, int Kq, int q_frame0, int S, int H, int Dh, int n_edits,
                                           unsigned inject_mask, int qk_compact, int flags, int dtype, const uint64_t* sets,
                                           char* buf, size_t len);

/* ------------------------------------------------------------------------
 * Row LayerNorm producer  --  the `norm1` call of TokenFlowBlock.forward
 * (tokenflow_utils.py:313-323; also norm2 / norm3 of the same forward, 399-417)
 * when the block runs in 16 bit:  out[r] = (x[r] - mean) / sqrt(var + eps) * gamma + beta
 * with fp32 statistics (biased variance, as torch) and ONE rounding to out_dtype,
 * instead of torch's autocast sequence cast-up / fp32 norm / cast-down.
 *   x      : [rows, D]  (in_dtype)      D multiple of 8, D <= 2048
 *   gamma, beta : [D] (w_dtype) or NULL (= 1 / 0)
 *   out    : [rows, D]  (out_dtype)
 *   inv_norm : float [rows] or NULL:  1 / ||out[r]||_2 of the ROUNDED output row -- what
 *              tf_pivot_inv_norm would compute from the stored pivots (util.py:67).
 * ------------------------------------------------------------------------ */
TF_API int tf_layer_norm(const void* x, const void* gamma, const void* beta, void* out, float* inv_norm,
                  int64_t rows, int D, float eps, int in_dtype, int w_dtype, int out_dtype,
                  void* stream);

/* Residual add + LayerNorm  --  `hidden_states = attn_output + hidden_states` followed by the block's next norm
 * (tokenflow_utils.py:396-403 and 409-414), one pass instead of an add kernel plus a norm:
 *   sum_out[r] = round_to(sum_dtype, a[r] + b[r])        (what torch's `a + b` stores: fp32 add, promoted dtype)
 *   out[r]     = LayerNorm(sum_out[r])                   (as tf_layer_norm, on the ROUNDED sum)
 * a, b, sum_out: [rows, D] of a_dtype / b_dtype / sum_dtype.  Results are bit-identical to the add followed by
 * tf_layer_norm. */
TF_API int tf_add_layer_norm(const void* a, const void* b, void* sum_out, const void* gamma, const void* beta, void* out,
                      int64_t rows, int D, float eps, int a_dtype, int b_dtype, int sum_dtype, int w_dtype,
                      int out_dtype, void* stream);

/* ------------------------------------------------------------------------
 * DDIM latent update  --  the step BEFORE the hot path (row f4): replaces preprocess.py:224-225 (ddim_inversion)
 * and 259-260 (ddim_sample), six elementwise torch ops per UNet call in the loops that write / check the latents
 * directory:
 *     out = mu_b * ((x - sigma_a * eps) / mu_a) + sigma_b * eps          (n elements; out may alias x)
 * inversion at step i:  a = timestep i-1 (mu_prev, sigma_prev), b = timestep i;  sampling: a = t, b = the next one.
 * Same operation order and the same per-op rounding to `dtype` as the reference's sequence (fp32 scalars, no FMA,
 * IEEE division): bit-identical to it in f32 / f16 / bf16.
 * ------------------------------------------------------------------------ */
TF_API int tf_ddim_step(const void* x, const void* eps, void* out, int64_t n, float mu_a, float sigma_a, float mu_b,
                 float sigma_b, int dtype, void* stream);

/* ------------------------------------------------------------------------
 * PnP feature injection  --  replaces tokenflow_utils.py:87-91:
 *   x viewed as [3, elems_per_branch]:  x[1] = x[0];  x[2] = x[0]   (in place)
 * elem_bytes = bytes per element; elems_per_branch*elem_bytes multiple of 16.
 * ------------------------------------------------------------------------ */
TF_API int tf_inject_copy(void* x, int64_t elems_per_branch, int elem_bytes, void* stream);

/* The same for a multi-edit batch: x viewed as [n_branches, elems_per_branch], x[b] = x[0] for every b >= 1 (in place);
 * n_branches = 1 + 2E, 3 .. 1 + 2*TF_MAX_EDITS.  Bit-exact copies. */
TF_API int tf_inject_copy_edits(void* x, int64_t elems_per_branch, int n_branches, int elem_bytes, void* stream);

/* Per-edit feature injection (ABI 11): the same for the edits in edit_mask only -- bit e set: x[1 + 2e] = x[2 + 2e] = x[0];
 * every other branch is neither read nor written.  One launch (the kernel of tf_inject_copy_edits with a branch mask);
 * all ones gives the result of tf_inject_copy_edits, 0 launches nothing.  A bit at or above E: TF_ERR_SHAPE. */
TF_API int tf_inject_copy_edits_masked(void* x, int64_t elems_per_branch, int n_branches, unsigned edit_mask, int elem_bytes,
                                void* stream);

/* ------------------------------------------------------------------------
 * Multi-GPU exchange steps over RCCL (one process per GPU).  The reference is single-process (no
 * parallelism of any kind), so these replace nothing in it; they are the C-ABI form of the two exchange steps of
 * tokenflow_amd/sharded.py for hosts that do not go through torch.distributed (the Python host does, and never calls
 * these).  Frames are sharded over the ranks:
 *   pivotal pass  (tokenflow_utils.py:133-138: every keyframe's queries read the keys/values of ALL K keyframes)
 *       tf_allgather_kv      each rank contributes its keyframes' slab, all ranks receive the bank (equal slabs), or
 *       tf_allgather_rows    the same for runs of different lengths (K % W != 0): rank p contributes rows[p] rows of
 *                            row_elems elements, every rank receives all of them in rank order, straight into place, or
 *       tf_all_to_all_rows   frames <-> heads re-sharding: rows [send_rows[p]] to peer p, [recv_rows[p]] from peer p
 *                            (row = row_elems elements; send / recv buffers are the concatenation in peer order);
 *   propagation   (331-333: chunk c reads keyframes c and c-1)
 *       tf_sendrecv_pivot    the last local keyframe's pivot features / inverse norms / attention output go to
 *                            send_peer (rank + 1) while the left neighbour's arrive from recv_peer (rank - 1);
 *                            a peer of -1 skips that direction (first / last rank).
 * Exceptions to the conventions at the top, all of them RCCL's: tf_comm_init / tf_comm_destroy allocate and free the
 * communicator handle and may synchronise; RCCL (librccl.so.1) is dlopen-ed on the first tf_comm_* call -- inside a
 * PyTorch process that is the copy torch has loaded -- and TF_ERR_COMM is returned if it is absent.  The collectives
 * themselves are asynchronous on `stream` like every other entry point.  tf_comm_init binds the calling thread's
 * current device (hipSetDevice first).  The unique id (128 bytes) is created on one rank by tf_comm_unique_id and
 * handed to the others by the host (file, socket, MPI ...).
 * ------------------------------------------------------------------------ */
typedef struct tf_comm tf_comm;
TF_API int tf_comm_available(void);   /* 0 if RCCL can be loaded and has every entry point used here; starts no
                                         bootstrap listener (a pre-flight probe: tf_comm_unique_id does start one) */
TF_API int tf_comm_unique_id(void* id_out_128_bytes);
TF_API int tf_comm_init(const void* unique_id_128_bytes, int rank, int world, tf_comm** comm_out);

/* Two more transports behind the same exchange entry points (no RCCL needed for either):
 *   tf_comm_init_hooks     a host-provided transport -- the exchanges are handed to the function table (sizes in
 *                          BYTES, device pointers, the stream the caller's work is ordered on; a function returns 0 or
 *                          an error code that surfaces as TF_ERR_COMM).  For hosts with their own fabric (MPI ...);
 *                          the multi-process tests of this repository carry it over gloo to run W ranks on one GPU.
 *   tf_comm_init_loopback  the wire-less stand-in: every exchange becomes device-to-device copies, on the stream, of
 *                          the sizes a real rank of a `world`-GPU run would receive, out of this rank's own buffers.
 *                          A rank's complete launch / stream / buffer sequence on ONE GPU: for timing the host and GPU
 *                          side of a rank (tools/rank_step_microbench.py); the received DATA is meaningless for
 *                          world > 1.
 * The peer arithmetic (rank, world, row counts) is the callers' in all three. */
#define TF_MAX_WORLD 64
typedef struct tf_comm_hooks {
    int (*all_to_all_rows)(void* user, const void* send, void* recv, const int64_t* send_rows, const int64_t* recv_rows,
                           int64_t row_bytes, void* stream);
    int (*allgather_rows)(void* user, const void* local, void* bank, const int64_t* rows, int64_t row_bytes,
                          void* stream);
    int (*sendrecv)(void* user, const void* const* send, const int64_t* send_bytes, int n_send, int send_peer,
                    void* const* recv, const int64_t* recv_bytes, int n_recv, int recv_peer, void* stream);
    void* user;
} tf_comm_hooks;
TF_API int tf_comm_init_hooks(const tf_comm_hooks* hooks, int rank, int world, tf_comm** comm_out);
TF_API int tf_comm_init_loopback(int rank, int world, tf_comm** comm_out);
/* loopback only: enabled = 0 makes every exchange a no-op (nothing moves, nothing is enqueued) -- the rank's launch sequence
 * with the stand-in copies taken out of the timing as well; buffers that an exchange would have filled keep their contents */
TF_API int tf_comm_loopback_copies(tf_comm* comm, int enabled);
/* loopback only (ABI 7): a wire MODEL.  Behind its copies (if enabled) every exchange enqueues, on the stream it was issued
 * on, a one-wave kernel that holds the stream for  latency_us + bytes_on_the_busiest_link / (gbps_per_link GB/s):  the
 * schedule's overlap of exchanges with compute is then EXECUTED, not estimated (tools/rank_step_microbench.py
 * --wire-model).  Links are full duplex and point to point (xGMI): an all-to-all or all-gather puts the rows for / from
 * peer p on the link to p, the busiest link carries max_p max(sent_p, received_p) bytes; a neighbour exchange sends on
 * one link and receives on another.  latency_us <= 0 and gbps_per_link <= 0 switch the model off (the default). */
TF_API int tf_comm_loopback_wire(tf_comm* comm, double latency_us, double gbps_per_link);
TF_API int tf_comm_destroy(tf_comm* comm);
TF_API int tf_comm_rank(const tf_comm* comm);
TF_API int tf_comm_world(const tf_comm* comm);
TF_API int tf_allgather_kv(tf_comm* comm, const void* local, void* bank, int64_t elems_per_rank, int dtype, void* stream);
TF_API int tf_allgather_rows(tf_comm* comm, const void* local, void* bank, const int64_t* rows, int64_t row_elems, int dtype,
                      void* stream);
TF_API int tf_all_to_all_rows(tf_comm* comm, const void* send, void* recv, const int64_t* send_rows, const int64_t* recv_rows,
                       int64_t row_elems, int dtype, void* stream);
TF_API int tf_sendrecv_pivot(tf_comm* comm, const void* const* send, const int64_t* send_elems, int n_send, int send_peer,
                      void* const* recv, const int64_t* recv_elems, int n_recv, int recv_peer, int dtype, void* stream);

/* ------------------------------------------------------------------------
 * One rank's pivotal pass of a block, issued by ONE host call  --  the native form of tokenflow_amd/sharded.py's
 * `pivotal_block` (no counterpart in the single-process reference; what is computed is tokenflow_utils.py:124-197
 * for the rank's keyframes against the bank of all K).  Rank r of W owns a contiguous run of the K keyframes (the
 * first K % W ranks one more); per block it
 *   TF_RANK_HEADS  packs head group w of its keyframes' q / k / v for every rank w (tf_head_pack), exchanges them
 *                  (tf_all_to_all_rows), computes the source branch of its own frames and
 *                  the uncond / cond branches of ITS head group over all K frames in place on the received buffer
 *                  (tf_ext_attn_fwd_strided, TF_ATTN_BANK_ONLY), sends the outputs back and unpacks them
 *                  (tf_head_unpack); needs H % W == 0 and one token stride for q, k, v;
 *   TF_RANK_BANK   gathers the K/V slabs of all ranks (tf_allgather_rows) and computes its own keyframes' queries
 *                  against the gathered bank: one collective, 4x the bytes; any head count;
 *   TF_RANK_BANK_RUNS  the bank form in runs of keyframes (below): two thirds of TF_RANK_BANK's bytes, the rank's own
 *                  keyframes attended to before the gather lands; any head count; a weaker identity guarantee;
 * then sends its last keyframe's pivot features, inverse norms and attention output to rank r+1 (tf_sendrecv_pivot on
 * the halo communicator and a stream of its own: chunk c of the propagation reads keyframes c and c-1, 331-333).
 *
 *   q, k, v   : the rank's local [3, Kl, S, H*Dh] projections; strides (elements) =
 *               { q_branch, q_frame, k_branch, k_frame, v_branch, v_frame, q_token, kv_token }
 *   piv_ext   : [Kl+o, S, H*Dh] 16-bit, inv_ext : float [Kl+o, S], kfo_ext : [3, Kl+o, S, H*Dh] 16-bit, o = 1 for
 *               W > 1 else 0: the per-block state of the propagation with the halo slot in front.  The caller has
 *               written the local keyframes' pivots / inverse norms into slots o..; the call writes the attention
 *               output into slots o.. of kfo_ext and the neighbour's last keyframe arrives in slot 0 of all three.
 *   flags     : TF_ATTN_INJECT / TF_ATTN_NO_SPLIT / TF_ATTN_FOLD_SCALE as for tf_ext_attn_fwd
 *   slot      : names this block's halo exchange, 0 <= slot < TF_RANK_SLOTS: tf_rank_halo_wait(rk, slot, stream) orders
 *               `stream` behind it (call it before the propagation reads slot 0; no host blocking)
 *   ws        : tf_rank_pivotal_workspace_bytes; holds the exchange buffers, so ONE workspace serves consecutive
 *               blocks of one stream (each use is complete before the next block touches it), not concurrent ones.
 * Every collective of `comm` is issued on the caller's stream (one communicator, one stream).
 * tf_rank_create makes two streams (auxiliary compute, halo) and the events on the CURRENT device; `comm` may be NULL (one rank: plain
 * tf_ext_attn_fwd into kfo_ext), `halo_comm` NULL = comm (a second communicator lets the halo of block b travel
 * beside the exchanges of block b+1: collectives of one RCCL communicator execute in issue order).
 * ------------------------------------------------------------------------ */
#define TF_RANK_HEADS 0
#define TF_RANK_BANK 1
#define TF_RANK_BANK_RUNS 2  /* the bank form in RUNS (ABI 9; any head count): only the slabs peers read are gathered ([k1, k2, v1, v2];
                                under injection [k0, v1, v2]), the LOCAL run -- the source branch of the rank's frames and their bank
                                branches against the rank's own keyframes, read from q / k / v in place -- starts on the auxiliary
                                compute stream before the gather, the remote runs (the frames left, then right of the rank's own)
                                follow behind it, and tf_ext_attn_runs_merge folds them: runs local, left, right in that slot order,
                                whatever the schedule.  Equal bit for bit to tf_ext_attn_run + merge on the full tensors with the
                                same runs, and to the oracle within the attention bound -- NOT to the one-call forms above. */
#define TF_RANK_BANK_EDIT_RUNS 3  /* tf_rank_pivotal_edits only: TF_RANK_BANK_RUNS' schedule for a multi-edit batch (below) */
#define TF_RANK_NO_HALO 16   /* or-ed into `mode`: the attention alone -- kfo_ext is a plain [3, Kl, S, H*Dh] output, piv_ext /
                                inv_ext are not read (NULL allowed), no neighbour exchange (hosts whose cached attention
                                output is not this one: the hook path caches it after the to_out projection) */
#define TF_RANK_INV_NORM 32  /* or-ed into `mode`: inv_ext's local slots o.. are OUTPUTS -- the call computes 1 / ||row|| of the
                                local pivots in piv_ext (tf_pivot_inv_norm's arithmetic, bit for bit) inside its pack launch,
                                instead of the caller in a launch of its own */
#define TF_RANK_SLOTS 64
typedef struct tf_rank tf_rank;
TF_API int tf_rank_create(tf_comm* comm, tf_comm* halo_comm, int K, tf_rank** rank_out);
TF_API int tf_rank_destroy(tf_rank* rk);
TF_API int tf_rank_local_keyframes(const tf_rank* rk);
TF_API int tf_rank_first_keyframe(const tf_rank* rk);
TF_API size_t tf_rank_pivotal_workspace_bytes(const tf_rank* rk, int S, int H, int Dh, int dtype);
TF_API int tf_rank_pivotal(tf_rank* rk, const void* q, const void* k, const void* v, const int64_t* strides, void* piv_ext,
                    float* inv_ext, void* kfo_ext, int S, int H, int Dh, float scale, int flags, int dtype, int mode,
                    int slot, void* ws, size_t ws_bytes, void* stream);
TF_API int tf_rank_halo_wait(tf_rank* rk, int slot, void* stream);

/* ------------------------------------------------------------------------
 * The rank executor for a MULTI-EDIT batch (additive to ABI 11): tf_rank_pivotal for B = 1 + 2*n_edits branches
 * [source | uncond_1 | cond_1 | ...]  --  the native form of `FrameShard._pivotal_heads_edits` / `_pivotal_bank_edits`
 * (tokenflow_amd/sharded.py), with the same buffer layouts: on the same transport both fill every buffer with the same bits.
 *
 *   q, k, v   : the rank's local [B, Kl, S, H*Dh] projections; the 8 strides of tf_rank_pivotal
 *   kfo_ext   : [B, Kl+o, S, H*Dh] ([B, Kl, ...] under TF_RANK_NO_HALO); piv_ext, inv_ext, slot, TF_RANK_INV_NORM,
 *               TF_RANK_NO_HALO and tf_rank_halo_wait as for tf_rank_pivotal
 *   inject_mask: the injection state per edit, as tf_ext_attn_fwd_edits_masked (bit e = edit e uses the source's q and k).
 *               TF_ATTN_INJECT or a part flag in `flags`, a mask bit at or above n_edits, n_edits outside 1 .. TF_MAX_EDITS,
 *               TF_RANK_BANK_RUNS with n_edits > 1 (its multi-edit form is a mode of its own, TF_RANK_BANK_EDIT_RUNS),
 *               TF_RANK_HEADS with H % W != 0: TF_ERR_SHAPE;
 *               a null pointer: TF_ERR_NULL.  All of that is checked before anything touches the device.
 *   ws        : tf_rank_pivotal_edits_workspace_bytes -- ONE size for both modes: the exchange buffers at their largest slab
 *               counts (6E slabs in the heads form, 4E in the bank form), the staging region of the compact q, and one
 *               attention workspace (tf_ext_attn_edits_workspace_bytes) each for the bank and the source part, which may run
 *               concurrently.  TF_RANK_BANK_EDIT_RUNS has a size query of its own, tf_rank_pivotal_edit_runs_workspace_bytes
 *               (the bank form's exchange buffers and ONE run-set workspace, tf_ext_attn_runs_edits_workspace_bytes).
 *
 * n_edits = 1 IS tf_rank_pivotal with TF_ATTN_INJECT set iff the mask is 1: the same launches, the same bits
 * (TF_RANK_BANK_EDIT_RUNS with one edit is TF_RANK_BANK_RUNS).
 * One rank (comm = NULL): the inverse norms if asked, then tf_ext_attn_fwd_edits_masked straight into kfo_ext.
 * W > 1.  Compact slots: slot 0 is the source if any edit injects (any = 1), then (uncond, cond) of each of the n_non
 * non-injecting edits in ascending order -- the qk_compact layout of tf_ext_attn_fwd_edits_part.
 *   TF_RANK_HEADS  ONE pack of [q slots | k slots | v_1 .. v_2E] (2 (any + 2 n_non) + 2E slabs; the inverse norms ride in the
 *                  same launch), ONE tf_all_to_all_rows, the bank part of every edit on the receive buffer in place
 *                  (tf_ext_attn_fwd_edits_part: TF_ATTN_BANK_ONLY, qk_compact, H / W heads, all K frames) into the send
 *                  buffer [K][2E][S][H*Dh/W] of ONE second all-to-all, ONE tf_head_unpack into the 2E bank slabs of kfo_ext.
 *                  The source part of the rank's own frames (TF_ATTN_SOURCE_ONLY on the local tensors) runs on the auxiliary
 *                  compute stream where it is a streaming launch -- forked behind the pack, in front of the first exchange,
 *                  joined in front of the second; TOKENFLOW_RANK_SRC_AUX=0 keeps it in line -- and in line behind the bank
 *                  part where it takes the fused small-problem kernel.  That decision uses ceil(K / W) for Kl: it is the same
 *                  on every rank of the block.
 *   TF_RANK_BANK   ONE pack (W = 1) of the compact k slots and the 2E value slabs ((any + 2 n_non) + 2E; the source's v and
 *                  every q stay at home), ONE tf_allgather_rows, the bank part on the gathered buffer (q_frame0 = the rank's
 *                  first keyframe, Kq = Kl, qk_compact), the source part on the local tensors.  A MIXED mask first copies
 *                  the compact q slots into the staging region (the pack kernel with W = 1, one launch); a uniform mask
 *                  reads q in place.
 *   TF_RANK_BANK_EDIT_RUNS  the schedule of TF_RANK_BANK_RUNS over the multi-edit run calls (any head count): the pack and
 *                  the gather of TF_RANK_BANK -- (any + 2 n_non) + 2E slabs -- but the LOCAL run (tf_ext_attn_run_edits: the
 *                  source branch and every edit's bank partials against the rank's own keyframes, q / k / v in place, dense)
 *                  is forked onto the auxiliary compute stream behind the pack and in FRONT of the gather; behind the gather
 *                  the remote runs (TF_ATTN_BANK_ONLY, k compact from the receive buffer, q dense from the local tensors:
 *                  no staging copy under a mixed mask); join; tf_ext_attn_runs_merge_edits into the local slots of kfo_ext.
 *                  Runs local, left, right in that slot order.  Per edit the bits of TF_RANK_BANK_RUNS on
 *                  [source | uncond_e | cond_e]: within the attention bound of the oracle, NOT bit-equal to TF_RANK_BANK.
 *   Halo           ONE grouped tf_sendrecv_pivot of 2 + B messages: the pivots, the B branches of kfo_ext and the inverse
 *                  norms of the last local keyframe to slot 0 of rank r+1.
 *
 * tf_rank_pivotal_edits_plan (host only: no device, stream or communicator): the sequence ONE call issues on `rank` of
 * `world` ranks over K keyframes, ';'-separated, recorded by the executing code itself:
 *   pack[ns=N] (pack+inv[ns=N] under TF_RANK_INV_NORM); qcompact[ns=N] where it happens; a2a[slabs=N] or gather[slabs=N]; the
 *   tokens of tf_ext_attn_edits_part_plan for the bank part, then for the source part (the source part is listed there also
 *   where it runs on the auxiliary stream); a2a[slabs=2E]; unpack[nb=2E]; halo[n=2+B] (absent under TF_RANK_NO_HALO and for
 *   one rank).  TF_RANK_BANK_EDIT_RUNS: pack[ns=N]; gather[slabs=N]; the run tokens of tf_ext_attn_run_edits_plan for the local
 *   run (listed behind the gather, though it is issued in front of it), then for each remote run; merge[runs=R,edits=E];
 *   halo[n=2+B].  One rank: inv_norm under TF_RANK_INV_NORM, then the tokens of tf_ext_attn_edits_masked_plan.  n_edits = 1: the
 *   sequence of tf_rank_pivotal in the same tokens (its attention tokens are those of tf_ext_attn_plan).
 * Returns the number of tokens, or a negative TF_ERR_* code.
 * ------------------------------------------------------------------------ */
TF_API size_t tf_rank_pivotal_edits_workspace_bytes(const tf_rank* rk, int S, int H, int Dh, int n_edits, int dtype);
TF_API size_t tf_rank_pivotal_edit_runs_workspace_bytes(const tf_rank* rk, int S, int H, int Dh, int n_edits, int dtype);
TF_API int tf_rank_pivotal_edits(tf_rank* rk, const void* q, const void* k, const void* v, const int64_t* strides,
                          void* piv_ext, float* inv_ext, void* kfo_ext, int S, int H, int Dh, float scale, int flags,
                          int dtype, int mode, int slot, int n_edits, unsigned inject_mask,
                          void* ws, size_t ws_bytes, void* stream);
TF_API int tf_rank_pivotal_edits_plan(int world, int rank, int K, int S, int H, int Dh, int n_edits, unsigned inject_mask,
                               int mode, int flags, int dtype, char* buf, size_t len);

/* ------------------------------------------------------------------------
 * The rank executor over a SLIDING-WINDOW bank (additive to ABI 11): tf_rank_pivotal with a `radius` -- long videos across
 * GPUs.  NOT TokenFlow's result unless the radius covers the bank; opt-in like tf_ext_attn_fwd_windows.
 *
 * Geometry (pure arithmetic of (world, rank, K, radius); `sharded.window_halo_plan` is the same in Python).  Rank r owns the
 * keyframes [kf0, kf0 + Kl).  It reads the global frames [lo, hi) = [max(0, kf0 - R), min(K, kf0 + Kl + R)): hl = kf0 - lo halo
 * frames on the left, hr = hi - kf0 - Kl on the right, F = hl + Kl + hr in all.  Peer p sends it own(p) & [lo, hi) -- for
 * R > Kl that spans several ranks -- so a rank receives at most 2R remote frames instead of K - Kl, and computes at most
 * (2R + 1) * Kl frame-banks of attention instead of K * Kl.  Local query i is global keyframe g = kf0 + i with the window of
 * g, [max(0, g - R), min(K - 1, g + R)], shifted by -lo; q_frame0 = hl.
 *
 * Schedule of ONE call (W > 1, radius < K - 1):
 *   1. tf_window_halo_pack: [k1, k2, v1, v2] of the frames peers read (under injection [k0, v1, v2]), own frames as self rows;
 *      the inverse norms under TF_RANK_INV_NORM are a launch of their own in front of it (tf_pivot_inv_norm);
 *   2. the source part of the local frames (tf_ext_attn_fwd_strided, TF_ATTN_SOURCE_ONLY, q / k / v in place) on the
 *      auxiliary compute stream, forked behind the pack and in front of the exchange (TOKENFLOW_RANK_SRC_AUX=0: in line);
 *   3. ONE tf_all_to_all_rows with the sparse row counts, on the caller's stream;
 *   4. tf_ext_attn_fwd_windows_part(TF_ATTN_BANK_ONLY) over the receive buffer [F][ns][S][D] in place, Kq = Kl, q_frame0 = hl;
 *   5. join;  6. the neighbour halo of the propagation, as in every mode (TF_RANK_NO_HALO, TF_RANK_INV_NORM, slot,
 *      tf_rank_halo_wait as for tf_rank_pivotal).
 * mode: TF_RANK_BANK (or 0) with the two modifier bits; the windowed pass has no heads form.
 * radius >= K - 1 IS tf_rank_pivotal(TF_RANK_BANK): the same launches, the same bits.  One rank (comm = NULL) is
 * tf_ext_attn_fwd_windows with the table of the radius.  Results: the bits of one process issuing
 * tf_ext_attn_fwd_windows_part(TF_ATTN_BANK_ONLY) and the source-only call on the full tensors under TF_ATTN_NO_SPLIT.
 * Refused with TF_ERR_SHAPE before anything touches the device: radius < 0, Kl > TF_MAX_WINDOW_FRAMES, F >= 2^16, a part flag
 * or TF_ATTN_FOLD_SCALE in `flags`, any other mode.
 *   ws: tf_rank_pivotal_window_workspace_bytes (never below tf_rank_pivotal_workspace_bytes: one workspace whatever the radius).
 * tf_rank_pivotal_window_plan (host only): the sequence, ';'-separated, recorded by the executing code itself:
 *   inv_norm under TF_RANK_INV_NORM; halo_pack[ns=N]; a2a[slabs=N,send=a/b/..,recv=a/b/..] (rows per peer, rank order); the
 *   tokens of the source-only tf_ext_attn_plan (listed behind the exchange, though it is issued in front of it); the tokens of
 *   tf_ext_attn_windows_part_plan for the bank part; halo[n=5].  A covering radius: the sequence of tf_rank_pivotal.
 * ------------------------------------------------------------------------ */
TF_API size_t tf_rank_pivotal_window_workspace_bytes(const tf_rank* rk, int S, int H, int Dh, int dtype, int radius);
TF_API int tf_rank_pivotal_window(tf_rank* rk, const void* q, const void* k, const void* v, const int64_t* strides,
                           void* piv_ext, float* inv_ext, void* kfo_ext, int S, int H, int Dh, float scale, int flags,
                           int dtype, int mode, int slot, int radius, void* ws, size_t ws_bytes, void* stream);
TF_API int tf_rank_pivotal_window_plan(int world, int rank, int K, int S, int H, int Dh, int radius, int mode, int flags,
                                int dtype, char* buf, size_t len);

/* ------------------------------------------------------------------------
 * The rank executor over an ANCHORED sliding-window bank (additive to ABI 11): tf_rank_pivotal_window plus global anchor
 * keyframes that every keyframe sees beside its window -- frame sets across GPUs.  NOT TokenFlow's result unless the radius
 * covers the bank; opt-in.
 *
 * anchors: a HOST array of n_anchors GLOBAL keyframe indices, 0 <= a < K, duplicates fine (indices, not a mask: K is free).
 * Geometry (pure arithmetic; `sharded.frame_set_halo_plan` is the same in Python).  With [lo, hi) as in the windowed call rank
 * r reads the set U = [lo, hi) + anchors, F = |U| <= 64 frames: a set is a 64-bit mask over the rank's EXTENDED bank, so the
 * cap K <= 64 of tf_ext_attn_fwd_frame_sets does not hold here.  Peer p sends it U & own(p), ascending: in rank order the
 * receive buffer of ONE tf_all_to_all_rows is U in ascending order.  It sends peer p own(r) & U_p, a mask over its Kl local
 * frames (an anchor it owns goes to every peer); its own frames travel as its self rows and are contiguous in U, from
 * q_frame0 = the number of members of U below kf0.  Local query i gets (window of keyframe kf0 + i) + anchors as a mask over
 * the positions in U.
 *
 * Schedule of ONE call (W > 1, radius < K - 1, n_anchors > 0): that of tf_rank_pivotal_window with two changes --
 *   1. tf_frame_set_halo_pack replaces tf_window_halo_pack;
 *   4. tf_ext_attn_fwd_frame_sets_part(TF_ATTN_BANK_ONLY) over the receive buffer [F][ns][S][D] in place, Kq = Kl, q_frame0 and
 *      the set table above (a rank whose sets are all ranges in U's coordinates thereby issues the windowed part).
 * The source part on the auxiliary stream (TOKENFLOW_RANK_SRC_AUX=0: in line), the join, the neighbour halo, TF_RANK_NO_HALO,
 * TF_RANK_INV_NORM and the slots are unchanged.
 * n_anchors = 0 IS tf_rank_pivotal_window; radius >= K - 1 IS tf_rank_pivotal(TF_RANK_BANK) whatever the anchors; one rank is
 * tf_ext_attn_fwd_frame_sets with the table of radius and anchors (K <= 64 there).  Results: the bits of one process issuing
 * tf_ext_attn_fwd_frame_sets_part(TF_ATTN_BANK_ONLY) and the source-only call on the full tensors under TF_ATTN_NO_SPLIT,
 * wherever the plans name the same kernel form (the form follows the rank's largest set).
 * Refused with TF_ERR_SHAPE before anything touches the device: what tf_rank_pivotal_window refuses, an anchor outside [0, K),
 * more than 4096 anchors, F > 64.
 *   ws: tf_rank_pivotal_frame_sets_workspace_bytes (never below tf_rank_pivotal_window_workspace_bytes for the same radius; 0
 *   for arguments the call refuses).
 * tf_rank_pivotal_frame_sets_plan (host only): the sequence, ';'-separated, recorded by the executing code itself:
 *   inv_norm under TF_RANK_INV_NORM; set_pack[ns=N]; a2a[slabs=N,send=a/b/..,recv=a/b/..]; the tokens of the source-only
 *   tf_ext_attn_plan; the tokens of tf_ext_attn_frame_sets_part_plan for the bank part; halo[n=5].
 * ------------------------------------------------------------------------ */
TF_API size_t tf_rank_pivotal_frame_sets_workspace_bytes(const tf_rank* rk, int S, int H, int Dh, int dtype, int radius,
                                                  const int* anchors, int n_anchors);
TF_API int tf_rank_pivotal_frame_sets(tf_rank* rk, const void* q, const void* k, const void* v, const int64_t* strides,
                               void* piv_ext, float* inv_ext, void* kfo_ext, int S, int H, int Dh, float scale, int flags,
                               int dtype, int mode, int slot, int radius, const int* anchors, int n_anchors, void* ws,
                               size_t ws_bytes, void* stream);
TF_API int tf_rank_pivotal_frame_sets_plan(int world, int rank, int K, int S, int H, int Dh, int radius, const int* anchors,
                                    int n_anchors, int mode, int flags, int dtype, char* buf, size_t len);

/* ------------------------------------------------------------------------
 * The rank executor for a MULTI-EDIT batch over a windowed / anchored bank (additive to ABI 11): several prompts on one long
 * video across GPUs in ONE sharded pass -- per block one pack, the same collectives, one bank part; only the payload grows with
 * E.  Opt-in: no existing call reaches it.
 *
 * Arguments of tf_rank_pivotal_frame_sets plus n_edits and inject_mask as in tf_rank_pivotal_edits: q, k, v hold B = 1 + 2E
 * branches [source | uncond_1 | cond_1 | ...] of the rank's Kl keyframes, kfo_ext is [B, Kl + o, S, D].  The geometry is that
 * of tf_rank_pivotal_window / tf_rank_pivotal_frame_sets: it does not depend on E.
 * Schedule of ONE call (W > 1, radius < K - 1, E > 1):
 *   0. the inverse norms under TF_RANK_INV_NORM, a launch of their own;
 *   1. ONE tf_edit_halo_pack of the compact k slots (slot 0 where some edit injects + 2 per non-injecting edit) and the 2E value
 *      slabs, with the compact q staging under a mixed mask in the same launch; the source's v and every q stay at home;
 *   2. the source part, tf_ext_attn_fwd_edits_part(TF_ATTN_SOURCE_ONLY), on the auxiliary stream, forked behind the pack
 *      (TOKENFLOW_RANK_SRC_AUX=0 keeps it in line behind the exchange);
 *   3. ONE tf_all_to_all_rows with the sparse counts;
 *   4. the bank part of ALL edits over the receive buffer [F][ns][S][D] in place (TF_ATTN_BANK_ONLY, qk_compact = 1, Kq = Kl,
 *      q_frame0 and table as in the single-edit calls): no anchors tf_ext_attn_fwd_windows_edits_part (F < 2^16), anchors
 *      tf_ext_attn_fwd_frame_sets_edits_part (F <= 64);
 *   5. join;  6. the neighbour halo with 2 + B messages.
 * Canonical forms: n_edits = 1 IS tf_rank_pivotal_frame_sets (TF_ATTN_INJECT iff mask = 1); radius >= K - 1 IS
 * tf_rank_pivotal_edits(TF_RANK_BANK); one rank is tf_ext_attn_fwd_windows_edits / tf_ext_attn_fwd_frame_sets_edits.
 * Results: the bits of one process issuing the bank part call and the source-only edits part on the full tensors under
 * TF_ATTN_NO_SPLIT; edit e's slices equal the single-edit windowed / anchored pass on [source | uncond_e | cond_e] with
 * inject = bit e wherever both plans name the same kernel form (four-bank form off).
 * Refused before anything touches the device: what both parent calls refuse, and every mode but TF_RANK_BANK (with
 * TF_RANK_NO_HALO / TF_RANK_INV_NORM).
 *   ws: tf_rank_pivotal_frame_sets_edits_workspace_bytes -- one size query, never below either parent's for the same arguments,
 *   0 for arguments the call refuses.
 * tf_rank_pivotal_frame_sets_edits_plan (host only): inv_norm; edit_pack[ns=N,nq=M]; a2a[slabs=N,send=..,recv=..]; the tokens of
 *   the source part; the tokens of the bank part; halo[n=2+B].
 * ------------------------------------------------------------------------ */
TF_API size_t tf_rank_pivotal_frame_sets_edits_workspace_bytes(const tf_rank* rk, int S, int H, int Dh, int dtype, int radius,
                                                        const int* anchors, int n_anchors, int n_edits);
TF_API int tf_rank_pivotal_frame_sets_edits(tf_rank* rk, const void* q, const void* k, const void* v, const int64_t* strides,
                                     void* piv_ext, float* inv_ext, void* kfo_ext, int S, int H, int Dh, float scale, int flags,
                                     int dtype, int mode, int slot, int radius, const int* anchors, int n_anchors, int n_edits,
                                     unsigned inject_mask, void* ws, size_t ws_bytes, void* stream);
TF_API int tf_rank_pivotal_frame_sets_edits_plan(int world, int rank, int K, int S, int H, int Dh, int radius, const int* anchors,
                                          int n_anchors, int n_edits, unsigned inject_mask, int mode, int flags, int dtype,
                                          char* buf, size_t len);

#ifdef __cplusplus
}
#endif
#endif /* TOKENFLOW_HIP_H */
