/* libmdbn_hip.so -- C-ABI of the MI355X (gfx950) CD-k engine.
 *
 * The reference (glgerard/MDBN, pure Python on Theano) has no FFI: its device boundary is
 * the call of a Theano-compiled step function built from RBM.get_cost_updates
 * (src/rbm.py:258-376, compiled at src/dbn.py:302-312 and src/rbm.py:533-544).  Each entry
 * point below replaces the piece of that compiled graph named in its comment; the Python
 * classes in mdbn_amd/ (same names and signatures as src/rbm.py, src/dbn.py, src/mlp.py)
 * are the only callers, through ctypes (mdbn_amd/_lib.py).
 *
 * Conventions
 *  - every function returns 0 (MDBN_OK) or a negative MDBN_E* code; text via mdbn_last_error
 *  - device buffers are owned by the caller (torch tensors): raw pointers, float32, row-major,
 *    leading dimensions `ld*` counted in floats, ld % 4 == 0 and 16-byte aligned bases
 *    (mdbn_padded_ld gives the recommended ld)
 *  - `stream` is a hipStream_t passed as void*; calls enqueue work and never synchronise
 *  - W is [V, ldh] (n_visible rows, n_hidden columns), as src/rbm.py:104
 *  - random matrices are addressed by (seed, stream_id, step, draw, row_offset): see
 *    mdbn_amd/csrc/philox.h (Philox4x32-10; CPU twins in oracle/philox_np.py, philox_ref.c)
 */
#ifndef MDBN_HIP_H
#define MDBN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDBN_OK       0
#define MDBN_EINVAL  (-1)   /* bad argument (shape, alignment, null pointer) */
#define MDBN_EHIP    (-2)   /* a HIP runtime call failed */
#define MDBN_ENOSPC  (-3)   /* workspace too small */

/* 2 (round 4): mdbn_cd_args and mdbn_update_args begin with `struct_size` -- a caller built against another layout of
 * either struct is refused with MDBN_EINVAL instead of having trailing fields read from whatever follows its struct. */
#define MDBN_VERSION 2

typedef struct mdbn_ctx mdbn_ctx;

/* Addresses one random matrix (uniform or normal) of one step. */
typedef struct mdbn_rng {
    uint64_t seed;        /* Philox key low/high words                                  */
    uint32_t stream_id;   /* one per RBM layer, xor-ed into the key's high word          */
    uint32_t step;        /* counter of step-function / sampling calls                   */
    uint32_t draw;        /* which random matrix inside the step (0 = U_h0, 2t-1, 2t)    */
    uint32_t reserved;
    uint64_t row_offset;  /* global row of local row 0 (data-parallel shard offset)      */
} mdbn_rng;

/* Everything one CD-k / PCD-k step needs: the compiled step function of
 * src/rbm.py:258-376 (+ the minibatch gather of src/dbn.py:307 / src/rbm.py:538). */
typedef struct mdbn_cd_args {
    uint64_t     struct_size; /* = sizeof(mdbn_cd_args) of the header the caller was built with; anything else: MDBN_EINVAL */
    /* data */
    const float *data;        /* [n_data, ldv] training matrix (train_set_x)                    */
    int64_t      n_data;
    const void  *indexes;     /* [B] minibatch row indices (device), or NULL: rows 0..B-1 of data */
    int32_t      index_is_64; /* 1 = int64 (dbn.py:271), 0 = int32 (rbm.py:528)                  */
    int32_t      gauss;       /* 1 = GRBM (rbm.py:631-699), 0 = Bernoulli RBM                    */
    int32_t      add_noise;   /* GRBM only: 1 = error_free False (rbm.py:652-658)                */
    int32_t      sample_stats;/* 1 = negative visible statistics from nv_SAMPLE, not nv_mean: the
                               * chain_end of compute_symbolic_grad (rbm.py:339-342,378-390)      */
    int32_t      keep_f32;    /* plane path and one-launch path (LDS-resident layers): 1 = also store the float32 copies of ph_mean, -nh_mean (P2), nv_mean
                               * (rows B.. of V2) and the chain samples (hs, vs) that only an inspecting caller reads;
                               * 0 = planes only (the statistics are always written; V2 / P2 / hs / vs are then scratch without defined content).  The
                               * f32-operand path always writes them; trace_h / trace_v imply 1                      */
    int32_t      k;           /* Gibbs steps                                                     */
    int64_t      B, V, H;     /* local minibatch rows, n_visible, n_hidden                       */
    int64_t      ldv, ldh;    /* leading dims of [.,V] and [.,H] matrices (W uses ldh)           */
    /* parameters */
    const float *W, *hbias, *vbias;
    /* PCD: persistent chain [B, ldh] read as chain start and overwritten with nh_sample
     * (rbm.py:308-311,369); NULL = CD */
    float       *persistent;
    /* scratch owned by the caller */
    float       *V2;          /* [2B, ldv]: rows 0..B-1 = v0, rows B..2B-1 = nv_mean (last step) */
    float       *P2;          /* [2B, ldh]: rows 0..B-1 = ph_mean, rows B..2B-1 = -nh_mean       */
    float       *hs;          /* [B, ldh] hidden chain state                                     */
    float       *vs;          /* [B, ldv] visible sample (RBM; GRBM with noise), may be NULL     */
    float       *stats;       /* packed [V*ldh | ldh | ldv | 4]: S, s_h, s_v, cost_sum           */
    void        *workspace;   /* >= mdbn_workspace_bytes(B, V, H)  (wider ld: _bytes_ld)         */
    int64_t      workspace_bytes;
    mdbn_rng     rng;         /* .draw is ignored (the step numbers its own draws)               */
    /* optional monitoring taps on the Gibbs chain (NULL = off; the role MonitorMode plays at
     * dbn.py:297-300,538-548): every sample the chain feeds onward is also copied here, so a checker can
     * follow the device's chain half-step by half-step */
    float       *trace_h;     /* [k+1][B][ldh]: slot 0 = positive-phase sample, slot t = hidden sample of
                               * Gibbs step t (slot k only when that sample is materialised: PCD)      */
    float       *trace_v;     /* [k][B][ldv]: slot t-1 = Bernoulli visible sample of step t (RBM only)   */
    /* bf16 plane path (optional).  With both pointers set and a shape made of whole 128-row/column tiles
     * (B, V, H multiples of 128, ldv == V, ldh == H, CD without persistent chain) every tensor of the step is
     * split ONCE into three bf16 planes where it is produced and the GEMMs copy plane tiles into LDS by LDS-DMA
     * (csrc/mdbn_planes.hip); otherwise the GEMMs split their f32 operands themselves.  Same arithmetic, same
     * results up to fp32 summation order. */
    void        *planes;      /* scratch of >= mdbn_planes_bytes(B, ldv, ldh) bytes, 16-byte aligned          */
    int64_t      planes_bytes;
    void        *W_planes;    /* [3][V][ldh] bf16: the exact split of W (W = p1 + p2 + p3)                    */
    int32_t      W_planes_valid; /* 1: W_planes already hold the split of the current W; 0: split W first.
                               * mdbn_cd_train_step / mdbn_apply_update (with its W_planes set) keep them in
                               * step with W, so a caller passes 0 only after writing W itself            */
    int32_t      comm_cus;       /* data-parallel mode: CUs left to a collective that runs beside this step; > 0: the plane
                               * GEMMs are launched balanced on (CUs - comm_cus) workgroups instead of one workgroup
                               * per CU (a collective's kernel takes whole CUs, and a full grid on fewer CUs needs a
                               * second round).  0: one workgroup per CU.  mdbn_set_option("comm_cus") overrides 0.  */
    /* Gather-ahead (optional; single-device plane path of mdbn_cd_train_step).  A caller that knows the NEXT minibatch
     * (the trainers do: the epoch's order is drawn up front, src/dbn.py:446-458) passes its indices and a second X2-plane
     * buffer: the statistics kernel's loader waves then gather those rows into the other buffer beside the MFMA main loop,
     * and the next call starts without a gather launch (x_buffer flipped, v0_ready = 1).  Same planes as the gather kernel
     * writes: results are bit-identical with and without.  The library decides per call whether it does it (plane path,
     * fused early update, keep_f32 = 0, <= 4 rows per workgroup) and reports through *ahead_done.
     * Thin-batch path (B <= 32): the update kernel, which streams W once anyway, also gathers the next minibatch into rows
     * 0..B-1 of V2 and leaves the partials of its positive phase x' W' in planes_alt (>= mdbn_ahead_bytes_ctx bytes): the
     * next call (v0_ready = 1; same data, index list and parameters, nothing else run on these buffers in between)
     * starts at its first activation kernel.  Same products in the same order: bit-identical with and without. */
    const void  *next_indexes;   /* [B] indices of the next minibatch (device, same type as indexes), or NULL         */
    void        *planes_alt;     /* second [3][2B][ldv] bf16 X2-plane buffer (mdbn_ahead_bytes_ctx), or NULL            */
    int32_t      x_buffer;       /* X2 planes of THIS step: 0 = inside `planes`, 1 = `planes_alt`                      */
    int32_t      v0_ready;       /* 1: rows 0..B-1 of that buffer already hold this minibatch (gathered ahead)         */
    int32_t     *ahead_done;     /* host pointer (nullable): set to 1 when this call gathered next_indexes ahead, else 0 */
} mdbn_cd_args;

/* Parameter update of src/rbm.py:347-365 from (all-reduced) statistics. */
typedef struct mdbn_update_args {
    uint64_t struct_size;           /* = sizeof(mdbn_update_args); anything else: MDBN_EINVAL */
    float *W, *W_speed;             /* [V, ldh] */
    const float *W0;                /* frozen weight-cost snapshot (rbm.py:415) or NULL = live W */
    float *hbias, *hbias_speed;     /* [H] */
    float *vbias, *vbias_speed;     /* [V] */
    int64_t V, H, ldv, ldh;
    const float *stats;             /* packed as mdbn_cd_args.stats (summed over ranks)          */
    float lr, lambda_1, lambda_2, weightcost, momentum;
    float batch_size;               /* divisor of S: the batch_size ARGUMENT (rbm.py:413)        */
    float n_rows;                   /* divisor of s_h, s_v: rows actually present (rbm.py:416-417) */
    float cost_scale;               /* monitoring cost = stats.cost_sum * cost_scale ...          */
    float *cost_out;                /* ... written here (device scalar) if not NULL               */
    void *W_planes;                 /* NULL, or [3][V][ldh] bf16 planes rewritten with the split of the new W
                                     * whenever this call changes W (phases 0, 2, 3)                          */
    int32_t phase;                  /* 0 = whole rule; 1 = speeds (+cost) only; 2 = parameters only;
                                     * 3 = 1 then 2 in one pass (parameters from the NEW speeds).
                                     * Because the parameter step uses the OLD speed (rbm.py:364-365),
                                     * theta(t+1) never depends on step t's gradient: a data-parallel
                                     * run applies phase 2 at once and phase 1 when the all-reduced
                                     * statistics arrive, overlapping the collective with the next step
                                     * (requires lambda_1 == 0 and weightcost == 0 or a frozen W0). */
    int32_t reserved;
} mdbn_update_args;

int  mdbn_version(void);
int  mdbn_last_error(char *buf, size_t n);
/* SHA-256 (hex) of the sources this library was built from (mdbn_amd/build.py compares it with the
 * sources on disk: a stale prebuilt library is rebuilt or refused, never silently used). */
int  mdbn_source_hash(char *buf, size_t n);

int  mdbn_ctx_create(mdbn_ctx **out, int device);
int  mdbn_ctx_destroy(mdbn_ctx *ctx);

/* Tuning knobs, PER CONTEXT (round 5): mdbn_set_option(ctx, ...) changes what calls made on `ctx` launch and nothing
 * else -- two contexts of one process (two engines, modality-parallel placement in-process) keep their own settings; the
 * context-free sizing calls (mdbn_workspace_bytes, mdbn_planes_eligible) answer for a context with default options, their
 * _ctx forms for the given one.  Results never change beyond fp32 summation order.
 * "gemm_bf16x6" (default 3): bit 0 = statistics GEMM, bit 1 = forward GEMMs run on the bf16 matrix pipe
 *   with exactly split f32 operands and f32 accumulation (f32-grade results) when the problem is made of
 *   whole 128x128 tiles; 0 = always the exact-f32 MFMA kernel.
 * "x6_min_jobs" (default 48): problems with fewer 128x128-tile jobs keep the exact-f32 kernel.
 * "x6_producer_waves" (default 4): producer waves per operand of the bf16x6 kernel (2 | 4).
 * "gemm_bk": GEMM slice depth, 0 = auto, 32 or 64.  "gemm_cw": MFMA waves per SIMD of the tiled
 *   GEMM, 0 = auto (2 for <= 512 rows), 1 or 2.  "gemm_min_splitk" (default 128, >= 32): smallest reduction
 *   length one split-K job of the tiled GEMM takes.
 * "epilogue_cw": columns per thread of the activation epilogue, 0 = auto, 1, 2 or 4.
 * "fused_epilogue" (default 1): GEMMs that need no split-K apply bias + activation + sampling to
 *   their own output tile instead of writing slabs for a second kernel (bitwise the same result).
 * "fused_update" (default 1): mdbn_cd_train_step applies the weight update inside the statistics
 *   GEMM when that GEMM is not split (and lets the update kernel sum the split-K slabs when it
 *   is); the S block of a->stats is then NOT materialised (s_h, s_v and cost_sum are).  Set 0 to
 *   get S (bitwise the same parameters either way).
 * "fused_finalize" (default 1): with fused_update, the bias statistics / cost / bias update run
 *   inside the statistics GEMM as well (no finalize launch).
 * "skinny_gemm" (default 1): GEMMs of <= 64 output rows, and tiny GEMMs at any row count, use the
 *   register-streaming kernel (no LDS staging); "skinny_fused_max_k" (default 1024) largest K one
 *   block streams alone, "skinny_max_macs" (default 32 Mi) size limit above 64 rows.
 * "stream_x6" (default 2): mid-size passes at more than 64 rows (M * N * K <= "stream_max_macs", default 2^30: the
 *   layers 1024 -> 256 and 2048 -> 400 of BASELINE configs 4 / 5 at B = 512) run UNSPLIT on 32 x 32 / 64 x 32 tiles of the
 *   register-streaming kernel on the bf16 matrix pipe (f32 operands split in registers into their three exact bf16
 *   pieces; six piece products, three when the row operand holds 0/1 samples) with the activation / update epilogue on
 *   the tile: one launch per pass instead of split-K GEMM + slabs + epilogue launch.  2: the small-layer passes of
 *   "skinny_gemm" above 64 rows too; 1: only the passes the LDS-tiled kernels served; 0: off.  "stream_mi": 0 = auto, 1 | 2 = 32-row blocks per tile;
 *   "stream_ni": 0 = auto, 1 | 2 = 32-column strips per tile.  stream_ni = 2 (set, or chosen by auto) implies 64-row
 *   tiles whatever "stream_mi" says: the kernel's tiles are 32 x 32, 64 x 32 and 64 x 64.
 * "gemm_planes" (default 1): use the bf16 plane path of mdbn_cd_args when its buffers are given and the
 *   shape qualifies.  "planes_mfma" (default 16): its MFMA shape, 16 = v_mfma_f32_16x16x32_bf16, 32 =
 *   v_mfma_f32_32x32x16_bf16 (bit-identical to the f32-operand path). 
 *  "planes_min_work" (default
 *   2^30): smallest B * V * H the plane path serves (smaller whole-tile layers are faster on the f32-operand kernels).
 * "early_w" (default 1): in the plane statistics GEMM with the fused update the parameter half (W and its planes: it
 *   needs only the old W and the old speed, rbm.py:364-365) is applied by the kernel's loader waves during the main loop,
 *   the epilogue only forms the new speed; bitwise the same parameters and speeds (needs lambda_1 == 0 and weightcost == 0
 *   or a frozen W0, else the whole rule stays in the epilogue).
 * "narrow_tiles" (default 1): a forward pass of the plane path whose 128 x 128 plan would split K exactly two ways
 *   (propdown at the c2 shape) runs unsplit on 128 x 64 tiles with the activation fused into the GEMM instead: no slabs,
 *   no epilogue launch; another fp32 summation grouping (one K-long chain instead of two halves).
 * "slab_tail" (default 1): the split-K propup of the plane path (16x16x32 shape) walks its last stages quarter by
 *   quarter of a wave's tile and stores each quarter's split-K partials, 16 bytes per lane, while the other quarters'
 *   MFMAs still run; 0 = all partials stored behind the last MFMA.  Bitwise the same outputs.  1 also gives the
 *   fused-update statistics launch of the single-device step (early parameter half) the same tail: the first half of the
 *   new weight speed is stored while the second half's MFMAs still run; 0 = the whole speed behind the last MFMA.
 * "feed_copy_streams" (default 1): a host-resident row feeder created afterwards moves each minibatch as 1 or 2 copies
 *   on as many streams.
 * "gather_ahead" (default 1): honour mdbn_cd_args.next_indexes (the next minibatch gathered inside the statistics
 *   kernel); 0 = every step launches its own gather.
 * "comm_cus" (default 0): CUs left to a collective that runs beside the step when mdbn_cd_args.comm_cus is 0 (see
 *   there); "bal_blocks" (tests): the number of workgroups of a balanced launch itself.
 * "epilogue_threads": threads per block of the activation epilogue launch, 0 = auto, 64, 128 or 256.
 * "bf16_inputs" (default 0): REPORTING mode, not a parity path: the plane GEMMs use only the leading bf16 piece of
 *   every operand (one product instead of six; probabilities off by ~4e-3).
 * "update_overlap": 1 = mdbn_cd_train_step overlaps part of the update with the statistics GEMM
 * on a side stream (default 0: measured slower, see csrc/mdbn_capi.hip).
 * "thin_fused" (default 1): minibatches of <= 32 rows (the reference's batch_size = 20, MDBN.py:46) on layers that are not
 *   LDS-resident (ldh <= 512) run as a stream over W (csrc/mdbn_thin.hip): the positive phase and each gibbs_hvh read W
 *   once (propdown and the following propup share one read: a workgroup owns whole rows of W), the rank-2B statistics are
 *   formed in registers inside the update pass -- W is read 2 + k times and written once per CD-k step.  0: the
 *   register-streaming GEMM path.
 * "gchain" (default 0, opt-in): mid-size layers at B > 32 whose W fits the LDS of a group of 2-16 CUs (256 -> 200, 1024 -> 256)
 *   run gather + positive phase + the whole Gibbs chain in ONE launch (csrc/mdbn_gchain.hip): 32-row slabs, each member of a
 *   group holds a block of W's rows in LDS, one in-launch exchange of the upward partials per pass (agent-scope write-through
 *   stores, a flag per member, bounded polls).  Same outputs as the multi-launch path, bit-reproducible; measured slower
 *   than it (an exchange costs what a kernel boundary costs), hence off.
 * "small_fused" (default 1): a layer whose W fits one CU's LDS (V, H <= 512, W image + row buffers <= 160 KB: 512 -> 40,
 *   400 -> 40, 200 -> 20, 100 -> 128, 100 -> 24 -> 3) runs the whole CD-k chain in ONE launch per step -- W staged once, each
 *   workgroup the whole chain for 4-row slabs on v_mfma_f32_4x4x1 out of LDS, partial statistics per workgroup -- plus a
 *   small finish launch (sum of the partials in a fixed order + update); same Philox addressing as every path.  0: the
 *   multi-launch path.  "small_fin_lanes" (0 = by the number of partials | 1, 2, 4, 8, 16): threads of the finish launch
 *   that share one sum. */
/* Introspection of the balanced launches of the data-parallel mode (no GPU work): segment k of workgroup w when
 * `workgroups` workgroups share `tiles` x `stages` evenly.  out[6] = {tile, first stage, end stage, segments of this
 * workgroup, stages of this workgroup, slabs (= sharing workgroups) of that tile}; tile = -1 when k is out of range. */
int  mdbn_bal_segment(int32_t tiles, int32_t stages, int32_t workgroups, int32_t w, int32_t k, int32_t *out);
int  mdbn_set_option(mdbn_ctx *ctx, const char *name, int64_t value);

/* Measurement hook (bench.py): while enabled, every GEMM launch (the dominant kernel) is
 * bracketed by HIP events on its stream; _read synchronises on them and returns the number
 * of launches recorded since enabling and the sum of their durations. */
int  mdbn_kernel_timing(mdbn_ctx *ctx, int enable);
int  mdbn_kernel_timing_read(mdbn_ctx *ctx, int64_t *n_launches, double *total_ms);
/* Per recorded launch (up to `cap`): duration, algorithmic FLOPs 2*M*N*K, FLOPs issued on the matrix
 * pipe the kernel runs on (x6 / x3 for the split-operand bf16 kernels), and
 * kind = 1000*family (0 LDS-tiled, f32 operands; 1 register-streaming; 2 bf16 planes)
 *        + 100*pipe (0 exact-f32 MFMA, 1 bf16 six products, 2 bf16 three products, 3 bf16 one product)
 *        + 10*fused + 2*la + lb  ((la, lb): 1 = propup, 0 = propdown, 3 = statistics).
 * *n_launches receives the number recorded (may exceed cap). */
int  mdbn_kernel_timing_detail(mdbn_ctx *ctx, int64_t cap, double *ms, double *alg_flop,
                               double *pipe_flop, int32_t *kind, int64_t *n_launches);
/* Introspection (tests): launches of the narrow one-plane propdown (kind 2210) that this context has sent to the 64-deep
 * form of its kernel since it was created. */
int  mdbn_narrow_deep_launches(mdbn_ctx *ctx, int64_t *n_launches);

/* WORKSPACE.  Every workspace is caller-owned and 16-byte aligned; a call is told its size and never touches a byte
 * beyond it.
 *  - mdbn_workspace_bytes(B, V, H): the bytes a CD step (mdbn_cd_step / _forward / _statistics / _train_step, mdbn_cd_stats,
 *    the grouped step) of exactly this shape needs, on leading dimensions up to mdbn_padded_ld's (and a ragged hidden width
 *    on ldh = round_up(H, 128), the plane path's).  The answer is NOT monotone in (B, V, H) -- fewer rows take more split-K
 *    slabs -- so ask for every shape that runs.  A step on wider leading dimensions asks mdbn_workspace_bytes_ld: its
 *    column-sum regions lie on the caller's strides.  A step handed fewer bytes than the sizer answers for its shape
 *    and leading dimensions returns MDBN_ENOSPC before any launch.
 *  - The propagate-only calls (mdbn_propup_sample, mdbn_propdown_sample, mdbn_gibbs_chain, mdbn_free_energy) accept ANY
 *    workspace of at least MDBN_MIN_WORKSPACE_BYTES, whatever B: they keep a fixed region for cost partials and cut the
 *    rows into chunks (multiples of four rows) whose split-K slabs fit in the rest -- results and random draws do not
 *    depend on the cut; more bytes only mean fewer launches.  Fewer bytes: MDBN_ENOSPC before any launch (likewise, for
 *    very wide layers, when not even a 4-row chunk fits).  mdbn_workspace_bytes[_ld][_ctx] never answer less than the
 *    minimum, so their answer serves these calls too (the *_workspace_bytes of the feature calls size those calls
 *    alone and may answer far less). */
#define MDBN_MIN_WORKSPACE_BYTES 278528     /* 4 * (65536 cost partials + 4096 slab floats) */
int  mdbn_workspace_bytes(int64_t B, int64_t V, int64_t H, int64_t *bytes);
/* ... under the options of `ctx` (the plans, hence the scratch, depend on them) */
int  mdbn_workspace_bytes_ctx(mdbn_ctx *ctx, int64_t B, int64_t V, int64_t H, int64_t *bytes);
/* ... for a step on the leading dimensions (ldv, ldh), any the step accepts; the same answer as mdbn_workspace_bytes on
 * those it covers */
int  mdbn_workspace_bytes_ld(int64_t B, int64_t V, int64_t H, int64_t ldv, int64_t ldh, int64_t *bytes);
int  mdbn_workspace_bytes_ld_ctx(mdbn_ctx *ctx, int64_t B, int64_t V, int64_t H, int64_t ldv, int64_t ldh, int64_t *bytes);
/* MDBN_MIN_WORKSPACE_BYTES as the library was built (bindings without the header) */
int  mdbn_min_workspace_bytes(int64_t *bytes);
/* leading dimension this library recommends for a [., cols] matrix (currently round_up(cols, 4);
 * see the measurement note in csrc/mdbn_capi.hip).  Any ld % 4 == 0, ld >= cols is accepted (a CD step on wider ones
 * than this sizes its workspace with mdbn_workspace_bytes_ld). */
int  mdbn_padded_ld(int64_t cols, int64_t *ld);
/* bytes of plane scratch (mdbn_cd_args.planes) for a minibatch of B rows: planes of [v0; nv], [ph; -nh],
 * the hidden and the visible sample */
int  mdbn_planes_bytes(int64_t B, int64_t ldv, int64_t ldh, int64_t *bytes);
/* bytes of the second X2-plane buffer of the gather-ahead (mdbn_cd_args.planes_alt) */
int  mdbn_planes_alt_bytes(int64_t B, int64_t ldv, int64_t *bytes);
/* bytes of mdbn_cd_args.planes_alt for this shape, whichever path serves it (plane path: the same as
 * mdbn_planes_alt_bytes; thin-batch path: the partials of the next step's positive phase) */
int  mdbn_ahead_bytes_ctx(mdbn_ctx *ctx, int64_t B, int64_t V, int64_t H, int64_t ldv, int64_t ldh, int64_t *bytes);
/* Does the plane path of mdbn_cd_step / mdbn_cd_train_step serve this shape under the CURRENT options (B and V whole
 * 128-row / 128-column tiles, ldv == V; the hidden side on a leading dimension of whole tiles, ldh % 128 == 0 and
 * H <= ldh < H + 128 -- a ragged hidden width rides on zero pad columns --; "gemm_planes" on, B * V * ldh >=
 * "planes_min_work")?  The one statement of the rule: a host allocates mdbn_cd_args.planes / W_planes for exactly these shapes.  (Per call the step also needs CD
 * without a persistent chain, no sample_stats and no GRBM noise.)  W planes handed to a step with W_planes_valid = 0
 * are re-split on entry whichever path the step takes, so they are valid after ANY step that received them. */
int  mdbn_planes_eligible(int64_t B, int64_t V, int64_t H, int64_t ldv, int64_t ldh, int32_t *eligible);
int  mdbn_planes_eligible_ctx(mdbn_ctx *ctx, int64_t B, int64_t V, int64_t H, int64_t ldv, int64_t ldh, int32_t *eligible);
/* exact three-way bf16 split of an f32 matrix [rows, ld] into planes [3][rows][ld] (x = p1 + p2 + p3) */
int  mdbn_split_planes(mdbn_ctx *ctx, void *stream, const float *x, int64_t rows, int64_t ld, void *planes);
/* floats in the packed statistics buffer [S (V*ldh) | s_h (ldh) | s_v (ldv) | 4] */
int  mdbn_stats_floats(int64_t V, int64_t ldv, int64_t ldh, int64_t *n);

/* minibatch gather: train_set_x[indexes]  (src/dbn.py:307, src/rbm.py:538): dst[r] = src[indexes[r]] for r < n_idx, the
 * round_up4(cols) leading floats of each row (the source's zero pad up to a multiple of 4 travels with it; columns of dst
 * beyond that are not written).  indexes: int32, or int64 with index_is_64; NULL = the first n_idx rows.  A negative index
 * counts from the end as in numpy: i in [-n_rows, 0) names row i + n_rows, so the valid range is [-n_rows, n_rows).
 * Duplicates are allowed.  ld_src and ld_dst are independent. */
int  mdbn_gather_rows(mdbn_ctx *ctx, void *stream, const float *src, int64_t n_rows,
                      int64_t cols, int64_t ld_src, const void *indexes, int index_is_64,
                      int64_t n_idx, float *dst, int64_t ld_dst);

/* The same gather for a source in PINNED HOST memory (device-accessible: hipHostMalloc / torch pin_memory), read over
 * PCIe by a small-footprint kernel: `workgroups` (0 = 32) workgroups of `threads` (0 = 256; 64 | 128 | 256) threads walk
 * the rows, four 16-byte loads in flight per thread, 20 VGPRs -- the streamed form of src/utils.py:113-115's table for
 * data that is not uploaded whole; meant for a side stream, one minibatch ahead of the step.  dst is device memory. */
int  mdbn_gather_rows_host(mdbn_ctx *ctx, void *stream, const float *src, int64_t n_rows,
                           int64_t cols, int64_t ld_src, const void *indexes, int index_is_64,
                           int64_t n_idx, float *dst, int64_t ld_dst, int workgroups, int threads);

/* out[r] = table[indexes[r]] on the HOST, by `threads` CPU threads (row-sized memcpys; indexes NULL = the first n rows):
 * the host half of the row feeder below, callable on its own (no GPU needed).  MDBN_EINVAL on an index outside
 * [0, n_rows). */
int  mdbn_host_gather_rows(const float *table, int64_t n_rows, int64_t cols, int64_t ld,
                           const int64_t *indexes, int64_t n, float *out, int64_t ld_out, int threads);

/* ROW FEEDER of a host-resident training table (the streamed form of src/utils.py:113-115's table for data that is not
 * uploaded whole) that keeps the CUs out of it: `threads` CPU threads gather a minibatch's rows into a pinned staging
 * slot, ONE hipMemcpyAsync moves the slot to the device on the feeder's own copy stream (SDMA), the consuming stream
 * waits for that copy's event.  Unlike mdbn_gather_rows_host's kernel, which slows every GEMM it runs beside, the copy
 * costs the step nothing; the ring of `slots` (>= 2; 3 keeps two minibatches in flight beside the one being read) hides
 * the gather and the PCIe time behind the steps.
 *   create : table [n_rows, ld] in host memory (pinned or pageable), device_slots[slots] device buffers of
 *            [max_rows, ld_device] floats owned by the caller (pad columns are written as zero);
 *   submit : queue a minibatch (the indexes are copied; NULL = rows 0 .. n-1); returns at once with a ticket;
 *   acquire: tickets in submission order; blocks the HOST until the ticket's copy has been enqueued, makes `stream` wait
 *            for it, returns the slot whose device buffer holds the rows;
 *   release: the work that reads the slot has been enqueued on `stream`: the slot may be overwritten after it;
 *   cancel : forget everything submitted and not acquired.
 * Thread-safe against its own worker threads; the calls themselves are for one host thread. */
typedef struct mdbn_feeder mdbn_feeder;
int  mdbn_feeder_create(mdbn_ctx *ctx, const float *table, int64_t n_rows, int64_t cols, int64_t ld,
                        int64_t max_rows, int slots, float *const *device_slots, int64_t ld_device,
                        int threads, mdbn_feeder **out);
int  mdbn_feeder_submit(mdbn_feeder *f, const int64_t *indexes, int64_t n, int64_t *ticket);
int  mdbn_feeder_acquire(mdbn_feeder *f, int64_t ticket, void *stream, int *slot);
int  mdbn_feeder_release(mdbn_feeder *f, int64_t ticket, void *stream);
/* host-side time per stage since the last call: out5 = { minibatches fed, mean gather us, mean copy-enqueue us,
 * acquires, mean host wait in acquire us }; resets the counters */
int  mdbn_feeder_stats(mdbn_feeder *f, double *out5);
int  mdbn_feeder_cancel(mdbn_feeder *f);
int  mdbn_feeder_destroy(mdbn_feeder *f);

/* propup + sample_h_given_v (src/rbm.py:187-213), also HiddenLayer.output (src/mlp.py:103-107):
 * pre = v W + hbias ; mean = sigmoid(pre) ; sample = (u < mean).
 * pre / mean / sample may each be NULL; mean is stored multiplied by mean_scale. */
int  mdbn_propup_sample(mdbn_ctx *ctx, void *stream, const float *v, int64_t B, int64_t ldv,
                        const float *W, int64_t V, int64_t H, int64_t ldh, const float *hbias,
                        float *pre, float *mean, float mean_scale, float *sample,
                        const mdbn_rng *rng, void *workspace, int64_t workspace_bytes);

/* propdown + sample_v_given_h: RBM src/rbm.py:215-240 (gauss=0: sigmoid + Bernoulli),
 * GRBM src/rbm.py:647-660 (gauss=1: linear mean, sample = mean [+ N(0,1) if add_noise]).
 * If v0 != NULL the un-normalised reconstruction cost of src/rbm.py:479-480 / :697 is
 * written to cost_sum[0] (sum over all elements; caller divides). */
int  mdbn_propdown_sample(mdbn_ctx *ctx, void *stream, const float *h, int64_t B, int64_t ldh,
                          const float *W, int64_t V, int64_t H, int64_t ldv, const float *vbias,
                          int gauss, int add_noise, float *pre, float *mean, float *sample,
                          const mdbn_rng *rng, const float *v0, float *cost_sum,
                          void *workspace, int64_t workspace_bytes);

/* Data parallelism (added by this engine; the reference is single-process): one process per GPU, minibatch rows
 * sharded over the ranks, ONE sum all-reduce of the packed statistics per CD step over RCCL / xGMI.
 * mdbn_comm_unique_id fills 128 bytes on one rank (ncclGetUniqueId); the caller hands them to every rank (any
 * channel: torch.distributed's store, a file) and each calls mdbn_comm_init_rank (ncclCommInitRank) on its
 * context.  mdbn_allreduce_stats enqueues the in-place float32 sum of stats[0..n) on `stream`; like every entry
 * point it does not synchronise.  librccl.so is opened on first use. */
int  mdbn_comm_unique_id(char *id128);
int  mdbn_comm_init_rank(mdbn_ctx *ctx, const char *id128, int nranks, int rank);
int  mdbn_allreduce_stats(mdbn_ctx *ctx, void *stream, float *stats, int64_t n);
int  mdbn_comm_destroy(mdbn_ctx *ctx);

/* n_steps of gibbs_vhv (src/rbm.py:250-256; GRBM :673-682) in one call, in place and without allocation: the
 * sampling loop of src/rbm.py:806-865 (theano.scan over gibbs_vhv, 500 steps x 20 chains).  v [B, ldv] holds
 * the chain's visible state on entry and vis_samples[-1] on return; h_mean / h_sample [B, ldh] and v_mean
 * [B, ldv] are scratch during the chain and the LAST step's values on return (pre_h / pre_v: optional).
 * Random draws: step t (0-based) uses rng->step + 2t for the hidden and rng->step + 2t + 1 for the visible
 * draw, both with draw index 0 -- exactly what 2 * n_steps eager sample_* calls consume, so a chain equals
 * n_steps eager gibbs_vhv calls bit for bit; the caller advances its step counter by 2 * n_steps. */
int  mdbn_gibbs_chain(mdbn_ctx *ctx, void *stream, float *v, int64_t B, int64_t ldv, const float *W,
                      int64_t V, int64_t H, int64_t ldh, const float *hbias, const float *vbias, int gauss,
                      int add_noise, int64_t n_steps, float *pre_h, float *h_mean, float *h_sample,
                      float *pre_v, float *v_mean, const mdbn_rng *rng, void *workspace,
                      int64_t workspace_bytes);

/* compute_rbm_grad's products (src/rbm.py:411-417) from the stacked buffers of mdbn_cd_args:
 * stats = [S = v0'ph - nv'nh | s_h | s_v | (cost untouched)] */
int  mdbn_cd_stats(mdbn_ctx *ctx, void *stream, const float *V2, const float *P2, int64_t B,
                   int64_t V, int64_t H, int64_t ldv, int64_t ldh, float *stats,
                   void *workspace, int64_t workspace_bytes);

/* update rule of src/rbm.py:347-365 */
int  mdbn_apply_update(mdbn_ctx *ctx, void *stream, const mdbn_update_args *a);

/* gather + positive phase + k x gibbs_hvh + statistics (src/rbm.py:303-345, 374);
 * leaves the packed statistics in a->stats; follow with mdbn_apply_update (after the
 * all-reduce in data-parallel runs). */
int  mdbn_cd_step(mdbn_ctx *ctx, void *stream, const mdbn_cd_args *a);

/* mdbn_cd_step in two calls, for the overlapped data-parallel order: mdbn_cd_forward = gather + positive phase + Gibbs
 * chain (everything that reads the parameters), mdbn_cd_statistics = bias statistics + the statistics GEMM (reads only the
 * step's own buffers).  In between the caller waits for the all-reduce of the PREVIOUS step and hands its deferred update
 * (`deferred`: mdbn_update_args with phase 3 and the reduced statistics of step t-1; NULL = none) to the statistics call:
 * nothing of that update depends on this step's statistics GEMM, so on the plane path its weight half is applied by that
 * GEMM's loader waves during the main loop and its bias / cost half by the MFMA waves ahead of it -- no update launch;
 * otherwise (f32-operand kernels, balanced launches, lambda_1 != 0, fewer than 20 stages) the library launches the update
 * kernel itself right before the GEMM.  Bitwise the same parameters as mdbn_cd_step + mdbn_apply_update(phase 3).
 * mdbn_cd_statistics must directly follow mdbn_cd_forward with the same arguments on the same context. */
int  mdbn_cd_forward(mdbn_ctx *ctx, void *stream, const mdbn_cd_args *a);
int  mdbn_cd_statistics(mdbn_ctx *ctx, void *stream, const mdbn_cd_args *a, const mdbn_update_args *deferred);

/* The whole compiled step function for a single device (src/rbm.py:258-376): mdbn_cd_step
 * followed by the update, in one call; parameters, speeds and cost are bitwise identical to
 * mdbn_cd_step + mdbn_apply_update.  upd->phase is ignored.  With option "fused_update" (default)
 * the S block of a->stats is left unspecified; s_h, s_v and cost_sum are always written.  (Option "update_overlap" moves the bias / cost
 * finalisation and the parameter half of the update onto an internal side stream under the
 * statistics GEMM, which never reads W.) */
int  mdbn_cd_train_step(mdbn_ctx *ctx, void *stream, const mdbn_cd_args *a,
                        const mdbn_update_args *upd);

/* free energy: RBM src/rbm.py:166-171, GRBM src/rbm.py:684-688;  out[N] */
int  mdbn_free_energy(mdbn_ctx *ctx, void *stream, const float *x, int64_t N, int64_t ldv,
                      const float *W, int64_t V, int64_t H, int64_t ldh, const float *hbias,
                      const float *vbias, int gauss, float *out,
                      void *workspace, int64_t workspace_bytes);

/* Annealed importance sampling (Salakhutdinov & Murray 2008) of a trained layer: M independent chains annealed from the
 * base-rate model (W = 0, hbias = 0, visible bias base_vbias; log Z_A = H log 2 + sum_i softplus(base_vbias_i) for Bernoulli,
 * H log 2 + V/2 log 2 pi for unit-variance Gaussian visibles, rbm.py:631-699) to the trained one through the inverse temperatures
 * betas[0] = 0 < ... < betas[K] = 1 (device array, n_betas = K + 1 values).  With a(v) = v W + hbias and
 * b_beta = (1 - beta) base_vbias + beta vbias:
 *   log p*_beta(v) = sum_j softplus(beta a_j(v)) + { v . b_beta  |  -|v - b_beta|^2 / 2 }
 *   v_1 ~ p_0;  k = 1 .. K:  logw += log p*_{beta_k}(v_k) - log p*_{beta_{k-1}}(v_k);
 *               k < K:  h ~ Bernoulli(sigmoid(beta_k a(v_k))),  v_{k+1} ~ Bernoulli(sigmoid(b_beta_k + beta_k h W^T))  |
 *                                                                        b_beta_k + beta_k h W^T + N(0, 1)
 * and log Z ~ log Z_A + logsumexp(logw) - log M (left to the caller: float64 on the host).  Products, softplus and row sums
 * are float32, the per-chain logw a double.  Random draws: v_1 uses step rng->step, the hidden draw of temperature k step
 * rng->step + 2k - 1, its visible draw rng->step + 2k, all with draw index 0 (normals: the Box-Muller pair of
 * mdbn_rng_normal); the caller advances its step counter by 2K - 1.
 * path: 0 = by shape, 1 = the one-launch path (LDS-resident layers: the shapes of "small_fused"; W staged once, a workgroup
 * runs the whole schedule for four chains, cut into launches of at most 4096 temperatures with the state carried in
 * v_state / logw) or MDBN_EINVAL if the shape does not fit, 2 = the general path (per temperature: the propup GEMM, a fused
 * weight-update + hidden-draw kernel, the propdown GEMM, a visible-draw kernel).  The paths meet the same uniforms and
 * differ by fp32 summation order only.  v_state (nullable): the final visible state [M, ldv].  trace_h [K-1][M][ldh] /
 * trace_v [K][M][ldv] (nullable): the hidden / visible sample of every temperature.  Bad arguments (M < 1, n_betas < 2,
 * path 1 on a shape that does not fit, a workspace shorter than mdbn_ais_workspace_bytes -- which answers for leading
 * dimensions up to mdbn_padded_ld) return MDBN_EINVAL without a launch. */
int  mdbn_ais_workspace_bytes(mdbn_ctx *ctx, int64_t M, int64_t V, int64_t H, int64_t n_betas, int path, int64_t *bytes);
int  mdbn_ais_run(mdbn_ctx *ctx, void *stream, const float *W, int64_t V, int64_t H, int64_t ldh,
                  const float *hbias, const float *vbias, const float *base_vbias, int gauss,
                  const float *betas, int64_t n_betas, int64_t M, int64_t ldv, float *v_state,
                  double *logw, float *trace_h, float *trace_v, int path, const mdbn_rng *rng,
                  void *workspace, int64_t workspace_bytes);

/* Clamped annealed importance sampling: the conditional partition function of a layer with part of its visible layer held
 * -- log p(v_F | v_O) of a held-out block F given the observed block O (Srivastava & Salakhutdinov 2012).  With the columns
 * O_r of data row r held at obs (mask = 1) the layer is an RBM over the free columns F_r (mask = 0) alone, with the row's own
 * hidden bias hbias + v_O W_O; its partition function Z_r differs from row to row, so every data row r = 0 .. N - 1 gets
 * C chains of its own: chain m = 0 .. N C - 1 is clamped to data row m / C (C >= 1, any value: a four-chain Philox block may
 * span two data rows).  obs [N, ldv]; mask [mask_rows, ldv] holds 0 / 1, mask_rows = N (per element) or 1 (one row for all).
 * With a(v) = v W + hbias over the WHOLE visible row (held columns included: beta a is the tempered pre-activation of the
 * conditional RBM) and b_beta = (1 - beta) base_vbias + beta vbias:
 *   log p*_beta(v_F) = sum_j softplus(beta a_j(v)) + { sum_{i in F} v_i b_beta,i  |  -1/2 sum_{i in F} (v_i - b_beta,i)^2 }
 * The run is mdbn_ais_run's with M = N C chains and three changes:
 *   1. after every visible draw, v_1 ~ p_0 included, v := mask ? obs : v;
 *   2. the bias term of the weight update sums over the free columns only;
 *   3. (Gaussian) its quadratic term sum_i (vbias - base_vbias)_i^2 becomes the per-mask-row sum over the free columns.
 * Everything else is mdbn_ais_run's: the arithmetic (float32 products, softplus and row sums in the same order, a held
 * column entering as 0.f; the per-chain logw [N C] a double), the Philox addressing (steps rng->step, + 2k - 1, + 2k, draw
 * index 0, the global chain row; a held column's uniform is not used), the paths (0 = by shape, 1 = one launch for
 * LDS-resident layers -- the observed values and mask bits of a thread's column kept in registers --, 2 = the general path
 * with the two propagation GEMMs per temperature), v_state [N C, ldv] (nullable) and trace_h [K-1][N C][ldh] / trace_v
 * [K][N C][ldv] (nullable); the caller advances its step counter by 2K - 1.  The caller finishes in float64, per data row:
 *   log Z_A,r = H log 2 + { sum_{i in F_r} softplus(base_vbias_i)  |  |F_r| / 2 log 2 pi },
 *   log Z_r ~ log Z_A,r + logsumexp_c(logw[r C + c]) - log C.
 * Two limits: with no held column the run IS mdbn_ais_run with M = N C, bit for bit in logw, v_state and the traces; with
 * every column of a row held nothing is random, v = obs, and logw = sum_j softplus(a_j(obs)) - H log 2 up to the float32
 * rounding of the telescoping sum.  Bad arguments (N < 1, C < 1, n_betas < 2, mask_rows neither 1 nor N, path 1 on a shape
 * that does not fit, a workspace shorter than mdbn_ais_cond_workspace_bytes) return MDBN_EINVAL without a launch. */
int  mdbn_ais_cond_workspace_bytes(mdbn_ctx *ctx, int64_t N, int64_t C, int64_t V, int64_t H, int64_t n_betas, int path, int64_t *bytes);
int  mdbn_ais_cond_run(mdbn_ctx *ctx, void *stream, const float *W, int64_t V, int64_t H, int64_t ldh,
                       const float *hbias, const float *vbias, const float *base_vbias, int gauss,
                       const float *betas, int64_t n_betas,
                       const float *obs, const float *mask, int64_t mask_rows, int64_t N, int64_t C, int64_t ldv,
                       float *v_state, double *logw, float *trace_h, float *trace_v, int path,
                       const mdbn_rng *rng, void *workspace, int64_t workspace_bytes);

/* Clamped Gibbs sampling: the chain of mdbn_gibbs_chain with part of the visible layer held at observed values, and the
 * running means of its conditional expectations -- the posterior of the unobserved visibles (a missing modality under the
 * joint layer of a multimodal DBN, Srivastava & Salakhutdinov 2012) and of the hidden layer given the observed ones.
 * mask [mask_rows, ldv] holds 0 / 1 (1 = observed: held at obs), mask_rows = B (per element) or 1 (one row for the batch).
 *   on entry v := mask ? obs : v;  step t = 0 .. n_steps - 1:
 *     h_mean = sigmoid(v W + hbias),                 h_sample = (U(rng->step + 2t) < h_mean)
 *     RBM : v_mean = sigmoid(h_sample W^T + vbias),  v_new = (U(rng->step + 2t + 1) < v_mean)
 *     GRBM: v_mean = h_mean W^T + vbias,             v_new = v_mean [+ N(0, 1) from rng->step + 2t + 1 if add_noise]   (gauss = 1)
 *           v_mean = h_sample W^T + vbias,           v_new = v_mean + N(0, 1) from rng->step + 2t + 1                  (gauss = 2)
 *     v_mean := mask ? obs : v_mean;  v := mask ? obs : v_new
 *     t >= burn_in:  v_acc += v_mean;  h_acc += h_mean             (float32, in step order)
 * gauss = 1 is the chain of the reference and of mdbn_gibbs_chain (the hidden MEAN goes down: a mean-field iteration, whose
 * averages are NOT the posterior means of the model); gauss = 2 is the Gibbs sampler of the same model (the hidden SAMPLE
 * goes down, unit noise always; add_noise is ignored), whose v_avg / h_avg estimate E[v | v_obs], E[h | v_obs].
 * Draw index 0 and the row addressing of mdbn_gibbs_chain; the caller advances its step counter by 2 * n_steps.  On return
 * v [B, ldv] is the final state, h_mean / h_sample [B, ldh] and v_mean [B, ldv] the last step's values, v_avg = v_acc /
 * (n_steps - burn_in) and h_avg likewise (each nullable); trace_v [n_steps][B][ldv] (the state after the clamp) and trace_h
 * [n_steps][B][ldh] (h_sample) are nullable taps.  With an all-zero mask the state, h_* and v_mean are those of
 * mdbn_gibbs_chain; with an all-one mask v never moves.
 * path: 0 = by shape, 1 = the one-launch path (LDS-resident layers: W staged once, a workgroup runs every step for four rows
 * with their observed values, mask and accumulators in registers; cut into launches of at most steps_per_launch steps, 0 =
 * the default 2048, the state carried in v and the workspace -- the cut changes no bit of any output) or MDBN_EINVAL if the
 * shape does not fit, 2 = the general path (per step the two passes of mdbn_gibbs_chain and one element-wise kernel).  The
 * paths meet the same uniforms and differ by fp32 summation order only.  Bad arguments (n_steps < 1, burn_in outside
 * [0, n_steps), mask_rows not 1 or B, path 1 on a shape that does not fit, a workspace shorter than
 * mdbn_gibbs_clamped_workspace_bytes -- which answers for leading dimensions up to mdbn_padded_ld) return MDBN_EINVAL
 * without a launch. */
int  mdbn_gibbs_clamped_workspace_bytes(mdbn_ctx *ctx, int64_t B, int64_t V, int64_t H, int path, int64_t *bytes);
int  mdbn_gibbs_clamped(mdbn_ctx *ctx, void *stream, float *v, const float *obs, const float *mask, int64_t mask_rows,
                        int64_t B, int64_t ldv, const float *W, int64_t V, int64_t H, int64_t ldh,
                        const float *hbias, const float *vbias, int gauss, int add_noise, int64_t n_steps,
                        int64_t burn_in, float *h_mean, float *h_sample, float *v_mean, float *v_avg, float *h_avg,
                        float *trace_h, float *trace_v, int path, int64_t steps_per_launch, const mdbn_rng *rng,
                        void *workspace, int64_t workspace_bytes);

/* Parallel tempering (replica exchange; Desjardins et al. 2010, Cho et al. 2010) of a trained layer: M ladders of R Gibbs
 * chains at the inverse temperatures 0 <= betas[0] < ... < betas[R-1] = 1 (a HOST array: checked before any launch) of the
 * tempered family of mdbn_ais_run (b_beta = (1 - beta) base_vbias + beta vbias), with swaps between neighbouring
 * temperatures.  Row m R + s of v [M R, ldv] / h [M R, ldh] is slot s of ladder m; rank [M][R] (int32, in and out) is the
 * temperature index a slot holds -- swaps exchange ranks, never states.  The joint at beta is
 *   log p_beta(v, h) = beta (v W h + hbias . h) + { b_beta . v  |  -|v - b_beta|^2 / 2 }        (gauss = 0 | 1)
 * and sweep t = 0 .. n_sweeps - 1 does, for every row at the beta of its rank:
 *   1. v ~ sigmoid(b_beta + beta h W^T)  |  b_beta + beta h W^T + N(0, 1)                               step rng->step + 3t
 *   2. a = v W + hbias;  l(beta') = sum_j softplus(beta' a_j) + { v . b_beta' | -|v - b_beta'|^2 / 2 }
 *   3. the rank pairs (rho, rho + 1) with rho = sweep0 + t (mod 2) swap iff log u < l_i(beta_j) + l_j(beta_i) - l_i(beta_i)
 *      - l_j(beta_j), u = the uniform of row `ladder`, column rho                                       step rng->step + 3t + 1
 *   4. h ~ sigmoid(beta a) at the rank after the swap                                                   step rng->step + 3t + 2
 * (draw index 0, the row addressing of mdbn_gibbs_chain with the global replica row; the caller advances its step counter by
 * 3 n_sweeps and passes the sweeps already run as sweep0, so that the parity continues).  The acceptance difference is formed
 * from float32 row sums regrouped as in mdbn_ais_run (differences of softplus; s1 = sum_i (v_i - [gauss] base_vbias_i)
 * (vbias - base_vbias)_i) and combined in double.  On return h and rank hold the state after the last sweep, v its visible
 * draw, accepted [R - 1] (int32) the accepted swaps per pair summed over the ladders, and -- each nullable -- v_avg [M, ldv] /
 * h_avg [M, ldh] the means over the sweeps burn_in .. n_sweeps - 1 of the beta = 1 visible mean (sigmoid(vbias + h W^T) |
 * vbias + h W^T) of the slot that holds rank R - 1 when it draws v, and of sigmoid(a) of the slot that holds rank R - 1 when it
 * draws h.  Taps (nullable): trace_v [n][M R][ldv], trace_h [n][M R][ldh], trace_swaps [n][M][2][R] int32 (the rank map after
 * the swap; per lower rank 1 = accepted, 0 = refused, -1 = not attempted).
 * path: 0 = by shape, 1 = the one-launch path (LDS-resident layers, R a multiple of 4 and <= 64: W staged once, a workgroup
 * owns whole ladders and swaps inside its LDS; cut into launches of at most steps_per_launch sweeps, 0 = the default, the
 * state carried in h, rank and the workspace -- the cut changes no bit) or MDBN_EINVAL if the shape does not fit, 2 = the
 * general path (per sweep: the propdown GEMM, a visible-draw kernel, the propup GEMM, a swap + hidden-draw kernel).  The paths
 * meet the same uniforms and differ by fp32 summation order only.  Bad arguments (R < 2, betas not rising strictly or not
 * ending at exactly 1, burn_in outside [0, n_sweeps), path 1 on a shape that does not fit, a workspace shorter than
 * mdbn_pt_workspace_bytes -- which answers for leading dimensions up to mdbn_padded_ld) return MDBN_EINVAL without a launch. */
int  mdbn_pt_workspace_bytes(mdbn_ctx *ctx, int64_t M, int64_t R, int64_t V, int64_t H, int path, int64_t *bytes);
int  mdbn_pt_run(mdbn_ctx *ctx, void *stream, const float *W, int64_t V, int64_t H, int64_t ldh,
                 const float *hbias, const float *vbias, const float *base_vbias, int gauss,
                 const float *betas, int64_t R, int64_t M, int64_t ldv, float *v, float *h, int32_t *rank,
                 int64_t n_sweeps, int64_t burn_in, int64_t sweep0, int32_t *accepted, float *v_avg, float *h_avg,
                 float *trace_v, float *trace_h, int32_t *trace_swaps, int path, int64_t steps_per_launch,
                 const mdbn_rng *rng, void *workspace, int64_t workspace_bytes);

/* mdbn_pt_run that also records the WORKS of its swap attempts: log Z from the ladder (Desjardins et al. 2011).  The four
 * float32 row sums that decide the swap of the ranks (rho, rho + 1), held by the slots i / j, are the two halves of a bridge
 * between the neighbouring temperatures; with db = betas[rho + 1] - betas[rho] and g = |vbias - base_vbias|^2,
 *   d_fwd = l_i(beta_{rho+1}) - l_i(beta_rho)  =  hsum_i + db s1_i - [gauss] (beta_{rho+1}^2 - beta_rho^2) g / 2
 *   d_rev = l_j(beta_rho) - l_j(beta_{rho+1})  =  hsum_j - db s1_j + [gauss] (beta_{rho+1}^2 - beta_rho^2) g / 2
 * combined in double (g in double from the float32 differences), and at stationarity
 *   log Z_{rho+1} / Z_rho  =  log E_rho[exp d_fwd]  =  -log E_{rho+1}[exp d_rev]
 * (the first estimate is biased low, the second high).  zacc [M][R - 1][4] (double, in and out, nullable) holds per ladder
 * and pair {m_f, s_f, m_r, s_r}: for every attempt of the sweeps t >= burn_in, m' = max(m, d), s = s exp(m - m') +
 * exp(d - m'), m = m' (s in double, the two exponentials float32), so that sum exp(d) = s exp(m).  The caller starts it at
 * m = -inf, s = 0; it is carried like rank, so two runs accumulate what one run of their sweeps does, bit for bit, and so
 * does any steps_per_launch.  With betas[0] = 0, log Z_0 = H log 2 + sum softplus(base_vbias) | H log 2 + V / 2 log 2 pi and
 * the host finishes log Z = log Z_0 + sum_rho log(sum_m s exp(m) / attempts).  trace_work [n][M][R - 1][2] (double,
 * nullable) taps (d_fwd, d_rev) of every sweep, NaN where trace_swaps says -1.  Recording consumes no random number and
 * alters no decision: every output of mdbn_pt_run is bit-identical.  Arguments, paths and rules are those of mdbn_pt_run
 * (zacc / trace_work 16-byte aligned); the workspace is sized by mdbn_pt_run_z_workspace_bytes (the general path keeps g
 * there). */
int  mdbn_pt_run_z_workspace_bytes(mdbn_ctx *ctx, int64_t M, int64_t R, int64_t V, int64_t H, int path, int64_t *bytes);
int  mdbn_pt_run_z(mdbn_ctx *ctx, void *stream, const float *W, int64_t V, int64_t H, int64_t ldh,
                   const float *hbias, const float *vbias, const float *base_vbias, int gauss,
                   const float *betas, int64_t R, int64_t M, int64_t ldv, float *v, float *h, int32_t *rank,
                   int64_t n_sweeps, int64_t burn_in, int64_t sweep0, int32_t *accepted, float *v_avg, float *h_avg,
                   float *trace_v, float *trace_h, int32_t *trace_swaps, int path, int64_t steps_per_launch,
                   const mdbn_rng *rng, void *workspace, int64_t workspace_bytes, double *zacc, double *trace_work);

/* Pieces of the variational lower bound on log p(data) of a DBN (Salakhutdinov & Murray 2008, section 4.2;
 * DBN.log_likelihood_bound): with the recognition model q(x_l | x_{l-1}) = Bernoulli(sigmoid(x_{l-1} W_l + hbias_l)),
 *   B(x_0) = E_q[ sum_{l < L} ( log p(x_{l-1} | x_l) + H[q(. | x_{l-1})] ) - F_L(x_{L-1}) ] - log Z_L  <=  log p(x_0).
 *
 * mdbn_propdown_rowll: the directed term of every replica row, the propdown GEMM fused with its row reduction -- the
 * [R, V] pre-activations exist in accumulators only.  h [R, ldh] holds 0 / 1 SAMPLES (precondition: any other value is
 * outside the contract; h enters the matrix pipe as one bf16 piece), W [V, ldh], vbias [V], target [T, ldv] with
 * T = ceil(R / target_div): replica row r is scored against target row r / target_div (target_div >= 1; S replicas of one
 * data row share that row).  With pre_i = h[r] . W[i, :] + vbias_i over the H live columns,
 *   gauss = 0:  out[r] = sum_{i < V} ( t_i pre_i - softplus(pre_i) ),   softplus(x) = max(x, 0) + log1p(exp(-|x|))
 *   gauss = 1:  out[r] = -1/2 sum_{i < V} (t_i - pre_i)^2 - V / 2 log 2 pi        (unit variance, as mdbn_free_energy)
 * float32 [R].  The padding of h and W beyond H and of target beyond V is never used (it may hold anything).  Products as the
 * plane propdown's for 0 / 1 operands (W split exactly into three bf16 pieces, f32 accumulation); a row's terms are summed per
 * 128-column tile and the tiles in ascending order by a second small launch: no atomics, two runs agree bit for bit.
 * workspace: >= mdbn_rowll_workspace_bytes(R, V, H) (the tile sums).  ldh % 4 == 0, h and W 16-byte aligned.
 *
 * mdbn_sample_replicas: S samples of every row of mean [N, ldh] (H live columns):
 *   sample[n S + s, j] = (u[n S + s, j] < mean[n, j]),   sample [N S, ldh] (pad columns written as 0),
 * u being the matrix mdbn_rng_uniform(rows = N S, cols = H) yields for the same mdbn_rng, row_offset included -- a caller
 * that walks its data rows in chunks (row_offset = first row x S) draws what one call over all rows draws.  entropy
 * (nullable) [N]: entropy[n] = -sum_{j < H} ( m log m + (1 - m) log(1 - m) ), 0 log 0 = 0, of the factorial Bernoulli
 * distribution with the means of row n.  S = 1 samples a matrix of means row by row.  The caller advances its step counter
 * by one. */
int  mdbn_rowll_workspace_bytes(mdbn_ctx *ctx, int64_t R, int64_t V, int64_t H, int64_t *bytes);
int  mdbn_propdown_rowll(mdbn_ctx *ctx, void *stream, const float *h, int64_t R, int64_t ldh, const float *W,
                         int64_t V, int64_t H, const float *vbias, const float *target, int64_t ldv,
                         int64_t target_div, int gauss, float *out, void *workspace, int64_t workspace_bytes);
int  mdbn_sample_replicas(mdbn_ctx *ctx, void *stream, const float *mean, int64_t N, int64_t H, int64_t ldh,
                          int64_t S, float *sample, float *entropy, const mdbn_rng *rng);

/* Centred CD training (Montavon & Mueller 2012; Cho et al. 2011, the "enhanced gradient"; Melchior, Fischer & Wiskott 2016,
 * Algorithm 1) of a layer kept in its ordinary parameters (W, vbias, hbias): visible and hidden units are referred to running
 * means mu [V] / lam [H] before the statistics are formed, and for such a layer the centred gradient is a transform of the
 * packed statistics [S | s_h | s_v | cost] of mdbn_cd_step, applied before mdbn_apply_update.  With all sums over the rows
 * of the minibatch,
 *   sum_r [(v0 - mu)(ph - lam)' - (vk - mu)(nh - lam)']  =  S - mu s_h' - s_v lam'  =:  S'
 * and, the update dividing S by batch_size and the bias sums by n_rows (src/rbm.py:411-417), rho = n_rows / batch_size,
 *   s_v' = s_v - rho S' lam,     s_h' = s_h - rho S'^T mu.
 * The unchanged update rule then runs on (S', s_h', s_v'); its weight-cost and lambda_1 / lambda_2 terms take no part.
 *
 * mdbn_center_offsets: v0 [B, ldv] and ph [B, ldh] are the data half of the step's scratch (rows 0..B-1 of
 * mdbn_cd_args.V2 / P2: a step run with keep_f32 = 1 on the plane and one-launch paths).  m_v[i] = (sum_{r < B} v0[r, i]) / B
 * and m_h[j] likewise from ph, rows added in ascending order in float32 with a compensation term (Kahan: the error of a mean
 * enters s_h' multiplied by mu . s_v, so a plain running sum of a few hundred rows is not good enough); then mu_i = fmaf(nu, m_v[i] - mu_i, mu_i),
 * lam_j = fmaf(nu, m_h[j] - lam_j, lam_j), and with nu = 1 exactly mu = m_v, lam = m_h (how a first centred step starts
 * them).  nu in (0, 1].  ld % 4 == 0, v0 and ph 16-byte aligned; the pad columns are not read.
 *
 * mdbn_center_stats: in place on stats (packed as mdbn_cd_args.stats, 16-byte aligned), per element
 *   t = fmaf(-mu_i, s_h[j], S_ij);   S'_ij = fmaf(-s_v[i], lam_j, t)
 * by workgroups that own blocks of whole rows of S; s_v'[i] = fmaf(-rho, sum_j S'_ij lam_j, s_v[i]) with the row's sum
 * reduced inside its workgroup, and s_h'[j] = fmaf(-rho, sum_i mu_i S'_ij, s_h[j]) from the workgroups' partial column
 * sums (workspace: [row blocks][round_up(H, 4)] floats, >= mdbn_center_workspace_bytes(V, H), 16-byte aligned) by a
 * second small launch -- every sum in a fixed order, no atomics: two runs agree bit for bit.  row_scale = rho > 0.  Pad
 * columns H..ldh-1 of S and s_h and V..ldv-1 of s_v are neither read nor written, the four cost floats are untouched; with
 * mu = 0 and lam = 0 the buffer comes back bit for bit.  H <= 4096.
 *
 * Bad arguments (a size < 1, a null pointer, a misaligned buffer or a leading dimension that is no multiple of 4, nu outside
 * (0, 1], row_scale <= 0, a short workspace) return MDBN_EINVAL without a launch. */
int  mdbn_center_workspace_bytes(mdbn_ctx *ctx, int64_t V, int64_t H, int64_t *bytes);
int  mdbn_center_offsets(mdbn_ctx *ctx, void *stream, const float *v0, int64_t ldv, const float *ph, int64_t ldh,
                         int64_t B, int64_t V, int64_t H, float nu, float *mu, float *lam);
int  mdbn_center_stats(mdbn_ctx *ctx, void *stream, float *stats, int64_t V, int64_t H, int64_t ldv, int64_t ldh,
                       const float *mu, const float *lam, float row_scale, void *workspace, int64_t workspace_bytes);

/* Sparsity target for the hidden units (Lee, Ekanadham & Ng 2008; Nair & Hinton 2009; Hinton's practical guide, section 11):
 * a penalty that drives the mean activation q_j of every hidden unit towards `target`, as a second transform of the packed
 * statistics [S | s_h | s_v | cost] of mdbn_cd_step, applied before mdbn_apply_update (and before mdbn_center_stats when the
 * step is centred as well: the sparsity part of the weight gradient is then taken through the centred input).  With
 * m_h[j] = mean_r ph[r, j], m_v[i] = mean_r v0[r, i] over the n rows of the minibatch and t_j = target - q_j,
 *   s_h[j] += b_scale t_j,    S_ij += w_scale m_v[i] t_j,    b_scale = cost n,  w_scale = cost batch_size,
 * so that the unchanged update rule (S / batch_size, s_h / n_rows; src/rbm.py:411-417) adds cost t_j to the hidden-bias
 * gradient and cost t_j m_v[i] to the weight gradient: the derivative of the cross-entropy between target and q_j with
 * respect to the unit's total input, through the bias and through the batch-mean input.  w_scale = 0 is the bias-only form
 * of Lee et al.  The update's weight-cost and lambda_1 / lambda_2 terms take no part.
 *
 * mdbn_sparsity_activity: ph [B, ldh] and v0 [B, ldv] are the data half of the step's scratch, as for mdbn_center_offsets.
 * The rows of a column are added in ascending order in float32 with a compensation term; then
 * q_j = fmaf(rate, m_h[j] - q_j, q_j), exactly m_h[j] at rate = 1 (how a first sparse step starts the estimate; afterwards
 * rate = 1 - decay, Nair & Hinton's running estimate), and v_mean[i] = m_v[i].  v0 and v_mean are both given or both null;
 * null: the hidden half alone, V and ldv are ignored.  rate in (0, 1].  ld % 4 == 0, ph and v0 16-byte aligned; the pad
 * columns are not read.
 *
 * mdbn_sparsity_stats: in place on stats (packed as mdbn_cd_args.stats, 16-byte aligned), per element
 *   t_j = target - q_j;   a_i = w_scale * v_mean[i];   S_ij = fmaf(a_i, t_j, S_ij)
 * by workgroups that own blocks of whole rows of S, one of which also does s_h[j] = fmaf(b_scale, t_j, s_h[j]).  No sum is
 * formed: two runs agree bit for bit, and H has no limit.  Pad columns H..ldh-1 of S and s_h are neither read nor written;
 * s_v, the four cost floats, q and v_mean are untouched.  w_scale = 0 does the s_h half only and never touches S (v_mean
 * may then be null); both scales 0 return MDBN_OK without a launch.  target in (0, 1); the scales finite and >= 0.
 *
 * Bad arguments (a size < 1, a null required pointer, v0 without v_mean or the reverse, w_scale > 0 without v_mean, a
 * misaligned buffer, a leading dimension below its width or no multiple of 4, rate, target or a scale out of range or NaN)
 * return MDBN_EINVAL without a launch. */
int  mdbn_sparsity_activity(mdbn_ctx *ctx, void *stream, const float *ph, int64_t ldh, const float *v0, int64_t ldv,
                            int64_t B, int64_t V, int64_t H, float rate, float *q, float *v_mean);
int  mdbn_sparsity_stats(mdbn_ctx *ctx, void *stream, float *stats, int64_t V, int64_t H, int64_t ldv, int64_t ldh,
                         const float *q, const float *v_mean, float target, float w_scale, float b_scale);

/* Learned per-column variance of a Gaussian visible layer (Hinton's practical guide, section 13.2; Krizhevsky 2009; Cho et
 * al. 2011).  With s = log sigma [V] and u = x exp(-s) ("the row in units"), p(x) = p_u(u) exp(-sum_i s_i), where p_u is the
 * unit-variance Gaussian layer of (W, hbias, vbias): the CD chain, its GEMMs, the statistics and the update run on u unchanged,
 * log Z does not depend on s, and the gradient of the mean log-likelihood of the rows of a minibatch with respect to s_i is
 * exact -- g_i = mean_r[u_ri (u_ri - m_ri)] - 1 with m = vbias + ph_mean W^T; the -1 is the model expectation, no chain
 * state enters.
 *
 * mdbn_sigma_scale_rows: dst[r, i] = src[indexes[r], i] * expf(sign * log_sigma[i]) for i < V and 0 for V <= i < ld_dst,
 * r < B.  sign = -1 takes raw rows to units (the gather of a training step, for mdbn_cd_step on the identity minibatch),
 * sign = +1 takes units back to raw.  src [n_src, ld_src], indexes as for mdbn_gather_rows (NULL: row r; int32 or int64;
 * negative values count from the end, out-of-range ones are clamped).  The factor of a column is formed once per thread, with
 * expf; with log_sigma = 0 it is exactly 1 and dst holds what mdbn_gather_rows copies.  Pad columns of src are not read, so
 * they may hold anything.  src and dst 16-byte aligned, ld % 4 == 0.
 *
 * mdbn_sigma_update: U [B, ldu] the rows in units (rows 0..B-1 of V2 after a mdbn_cd_step with keep_f32 = 1) and M [B, ldm]
 * their conditional means m (mdbn_propdown_sample, gauss = 1, of ph_mean: rows 0..B-1 of P2), with the parameters as they were
 * BEFORE mdbn_apply_update.  Over the first n_rows rows (1 <= n_rows <= B; the others are not read), in ascending order in
 * float32 with a compensation term,
 *   q_i = sum_r U_ri (U_ri - M_ri),  g_i = q_i / n_rows - 1,
 *   log_sigma_i = min(max(log_sigma_i + speed_i lr, lo), hi)   (the OLD speed),   speed_i = g_i + (speed_i - g_i) momentum,
 * the rule mdbn_apply_update applies to vbias (src/rbm.py:361-365), without shrink or weight cost.  [lo, hi] is a guard against
 * overflow of exp, not a tuned value.  Up to 64 rows one launch does it all; above, the rows are split into slices of 16 whose
 * partial sums go to `workspace` (mdbn_sigma_workspace_bytes(B, V); 16-byte aligned; 0 bytes and NULL allowed up to 64 rows)
 * and a second launch adds them in ascending order.  No atomics: two runs agree bit for bit.  Pad columns of U and M are not
 * read; no statistics buffer is involved.  lr = 0 leaves log_sigma as it is and still moves the speed.
 *
 * Bad arguments (a size < 1, B > 2^19, n_rows outside [1, B], a null pointer, a misaligned buffer, a leading dimension below V
 * or no multiple of 4, an identity minibatch longer than src, sign not +-1, lr < 0, momentum outside [0, 1], lo > hi, any of
 * them NaN, a short workspace) return MDBN_EINVAL without a launch. */
int  mdbn_sigma_workspace_bytes(mdbn_ctx *ctx, int64_t B, int64_t V, int64_t *bytes);
int  mdbn_sigma_scale_rows(mdbn_ctx *ctx, void *stream, const float *src, int64_t n_src, int64_t ld_src, const void *indexes,
                           int index_is_64, int64_t B, int64_t V, const float *log_sigma, float sign, float *dst,
                           int64_t ld_dst);
int  mdbn_sigma_update(mdbn_ctx *ctx, void *stream, const float *U, int64_t ldu, const float *M, int64_t ldm, int64_t B,
                       int64_t V, int64_t n_rows, float lr, float momentum, float lo, float hi, float *log_sigma,
                       float *log_sigma_speed, void *workspace, int64_t workspace_bytes);

/* Up-down fine-tuning of a DBN (Hinton, Osindero & Teh 2006, contrastive wake-sleep): the delta rules of a directed layer
 * whose recognition weights W (upwards) and generative weights G (downwards) have been untied.  Both rules are CD statistics
 * with chosen operands, applied by the unchanged update rule (src/rbm.py:347-365) that `upd` describes: upd->stats and
 * upd->cost_out are ignored, upd->phase must be 0, and the bias half that a rule does not own must be NULL.
 *
 * mdbn_updown_gen_step (upd->W = G [V, ldh], upd->W_speed its speed, upd->vbias / vbias_speed the generative bias;
 * upd->hbias = upd->hbias_speed = NULL): with x_lo [n, ldv] the layer's input and x_hi [n, ldh] the state inferred above it,
 *   g = act(x_hi G^T + vbias)   (sigmoid; gauss = 1: the linear mean),   S = (x_lo - g)^T x_hi,   s_v = sum_r (x_lo - g),
 * the gradient of sum_r log p(x_lo | x_hi) (Bernoulli and unit-variance Gaussian alike); S is divided by upd->batch_size and
 * s_v by upd->n_rows.  g is formed from the parameters as they are on entry.  cost_out (nullable, device):
 * upd->cost_scale * sum_r -log p(x_lo | x_hi), the cross-entropy x softplus(-pre) + (1 - x) softplus(pre) summed over the
 * units, or with gauss half the squared error.
 * mdbn_updown_rec_step (upd->W = W, upd->hbias / hbias_speed the recognition bias; upd->vbias = upd->vbias_speed = NULL): with
 * y_lo [n, ldv], y_hi [n, ldh] a dreamt pair of states and r = sigmoid(y_lo W + hbias) [n, ldh] (mdbn_propup_sample),
 *   S = y_lo^T (y_hi - r),   s_h = sum_r (y_hi - r).
 *
 * path: 0 = by shape, 2 = composed from the launchers of the CD step on any shape -- the operands stacked as
 * V2 = [x_lo; g], P2 = [x_hi; -x_hi] (V2 = [y_lo; y_lo], P2 = [y_hi; -r]), mdbn_propdown_sample for g, mdbn_cd_stats,
 * mdbn_apply_update with a throw-away vector in place of the bias half that must not move --, 1 = one pass over the matrix:
 * n <= 32 rows and ldh <= 512 (MDBN_EINVAL elsewhere; path 0 then takes the composed path).  The one-pass generative kernel
 * holds whole rows of G per workgroup, forms its slice of g completely (float32 fmaf chains, never bf16), the error, the rows
 * of S in registers and applies the rule at once: G and its speed are read and written once, S is never stored; it neither
 * reads nor writes the pad columns H..ldh-1 of G, of the speed and of x_hi.  The one-pass recognition update is the rank-2n
 * update kernel of the thin-batch CD step on the stacked operands.  upd->W_planes, where given, are rewritten with the split
 * of the new matrix on every path.  No atomics, every sum in a fixed order: two runs agree bit for bit.
 *
 * Bad arguments (a size < 1 or > 2^24, a null or misaligned matrix, a leading dimension below its width or no multiple of 4,
 * a bias half that should be NULL or is missing, divisors <= 0, phase != 0, path 1 on a shape it does not serve, a short
 * workspace) return MDBN_EINVAL without a launch: no output is touched. */
int  mdbn_updown_gen_workspace_bytes(mdbn_ctx *ctx, int64_t n, int64_t V, int64_t H, int64_t ldv, int64_t ldh, int path,
                                     int64_t *bytes);
int  mdbn_updown_gen_step(mdbn_ctx *ctx, void *stream, const float *x_lo, const float *x_hi, int64_t n, int gauss,
                          const mdbn_update_args *upd, float *cost_out, int path, void *workspace, int64_t workspace_bytes);
int  mdbn_updown_rec_workspace_bytes(mdbn_ctx *ctx, int64_t n, int64_t V, int64_t H, int64_t ldv, int64_t ldh, int path,
                                     int64_t *bytes);
int  mdbn_updown_rec_step(mdbn_ctx *ctx, void *stream, const float *y_lo, const float *y_hi, const float *r, int64_t n,
                          const mdbn_update_args *upd, int path, void *workspace, int64_t workspace_bytes);

/* Categorical visible units: K-ary softmax groups (Salakhutdinov, Mnih & Hinton 2007) inside a Bernoulli visible layer.
 * group_start[0 .. n_groups] (int32) are column offsets, strictly ascending, 0 <= group_start[0], group_start[n_groups] <= V;
 * group g is columns group_start[g] .. group_start[g + 1] - 1, of 2 .. MDBN_GROUP_MAX columns, exactly one of which is on.
 * The groups are adjacent (one contiguous span); the columns before and after the span are ordinary Bernoulli units;
 * n_groups = 0 (no table read, both pointers may be NULL) is a plain Bernoulli layer.  The caller passes BOTH copies of the
 * table: `group_start` in device memory, which the kernel reads, and `group_start_host`, the same values in host memory,
 * which the library checks before anything is launched -- no call synchronises or copies to find out.  That the two agree is
 * the caller's contract (the kernel clamps what the device copy says to the span the host copy gives, so a stale device copy
 * gives wrong groups, never an access outside the row).
 *
 * mdbn_group_softmax_sample: p(v | h) from the visible pre-activations pre [B, ldv] = h W^T + vbias (what
 * mdbn_propdown_sample(gauss = 1) stores as its mean).  Per row and group, with m = max_c x_c:  e_c = exp(x_c - m) (the
 * hardware exponential),  Z = sum_c e_c in ascending c in float32,  mean_c = e_c / Z (correctly rounded).  One uniform per
 * (row, group), addressed at the group's FIRST column -- counter (col, global_row >> 2, rng->draw, rng->step), word
 * global_row & 3, rng->row_offset honoured (philox.h) --; the category is the first c with u < C_c, C_c the running float32
 * sum of the stored means in ascending c, and the LAST one when none qualifies (C_{K-1} may fall short of the largest
 * uniform, 1 - 2^-25).  sample is 0 / 1 floats with exactly one 1 per group.  A Bernoulli column is the arithmetic and the
 * addressing of mdbn_propdown_sample(gauss = 0): mean = sigmoid(x), sample = (u < mean) with the column's own uniform, so
 * n_groups = 0 reproduces that call's mean and sample bit for bit.  mean, sample and tap (a second copy of the sample, for a
 * chain tap) may each be NULL; mean may be `pre` itself (in place).  With v0 [B, ldv] the cost
 *   sum over groups of sum_c v0_c (log Z - (x_c - m))  +  sum over Bernoulli columns of v0 softplus(-x) + (1 - v0) softplus(x)
 * -- the categorical cross-entropy from the log-sum-exp, finite where a probability underflows -- is written to cost_sum[0]
 * (cost_sum: 4 floats, 16-byte aligned; [1..3] are zeroed) through per-workgroup partials in `workspace`
 * (mdbn_group_softmax_workspace_bytes; only needed with v0) summed in a fixed order.  No atomics: two runs agree bit for
 * bit.  Pad columns V..ldv-1 are neither read nor written.
 *
 * mdbn_cd_step_grouped: mdbn_cd_step for a layer with groups, composed from the propagation passes, the kernel above and
 * mdbn_cd_stats:  gather;  propup (ph_mean, hidden sample);  k x [propdown to the linear pre-activations -> the group kernel
 * (means in place, visible sample) -> propup from the visible SAMPLE];  mdbn_cd_stats.  It leaves what
 * mdbn_cd_step(keep_f32 = 1) leaves: V2 rows 0..B-1 = v0, rows B..2B-1 = the last step's visible means; P2 = ph_mean and
 * -nh_mean; hs, vs; the packed [S | s_h | s_v | cost], the cost slot holding the cost above of the LAST step's
 * pre-activations against v0.  PCD: the chain starts from a->persistent, which is overwritten with the last hidden sample.
 * trace_h / trace_v as in mdbn_cd_args.  Draw numbering, that of mdbn_cd_step: 0 = the positive-phase hidden draw, 2t - 1 =
 * the visible draw of Gibbs step t (one uniform per Bernoulli column, one per group at its first column), 2t = its hidden
 * draw -- a layer with n_groups = 0 follows the chain of mdbn_cd_step on the f32-operand path.  a->vs is required; the
 * plane, keep_f32 and gather-ahead fields of `a` are ignored (W planes handed in are neither read nor re-split).
 * MDBN_EINVAL with a message, before any launch and with every output untouched: a->gauss, a->sample_stats, an invalid
 * table (not ascending, a group of fewer than 2 or more than MDBN_GROUP_MAX columns, a boundary beyond V, a missing copy),
 * and what mdbn_cd_step refuses; a short workspace (mdbn_workspace_bytes serves) is MDBN_ENOSPC, likewise before any launch.
 *
 * mdbn_center_hidden_rows: the hidden-bias statistic of the centred gradient, s_h' = s_h - row_scale S'^T mu (mdbn_center_stats),
 * formed from the rows of the step's scratch instead of from S -- mathematically the same number:
 *   d_r = mu . (x_r - mu) over the 2B rows of V2 = [v0; nv],   q = s_v . mu,
 *   s_h_out[j] = s_h[j] - row_scale (sum_{r < 2B} d_r P2[r, j] - q lam[j])        (P2 = [ph_mean; -nh_mean])
 * On one-hot rows mu . x_r hardly varies, d_r is small, and nothing of the size of (mu . mu) s_h is formed and cancelled; through
 * S that cancellation multiplies the float32 error of S by sum_i mu_i.  Call it BEFORE mdbn_center_stats (it reads the raw s_h
 * and s_v of `stats`) with the offsets mdbn_center_offsets left, and store s_h_out [H] over the s_h block afterwards.  When
 * `stats` went through mdbn_sparsity_stats first (S += w_scale v_mean t', s_h += b_scale t, t = target - q), pass that call's q,
 * v_mean, target, w_scale and b_scale: S'^T mu then also holds (w_scale (v_mean . mu) - b_scale (mu . mu)) t, which the rows do
 * not know and the call adds; q = NULL: no such transform ran (the other four are ignored).  Fixed order, no atomics;
 * workspace: 2B + 3 floats.  Bad arguments: MDBN_EINVAL without a launch. */
#define MDBN_GROUP_MAX 64
int  mdbn_center_hidden_rows(mdbn_ctx *ctx, void *stream, const float *V2, int64_t ldv, const float *P2, int64_t ldh,
                             int64_t B, int64_t V, int64_t H, const float *stats, const float *mu, const float *lam,
                             float row_scale, const float *q, const float *v_mean, float target, float w_scale,
                             float b_scale, float *s_h_out, void *workspace, int64_t workspace_bytes);
int  mdbn_group_softmax_workspace_bytes(mdbn_ctx *ctx, int64_t B, int64_t V, int64_t *bytes);
int  mdbn_group_softmax_sample(mdbn_ctx *ctx, void *stream, const float *pre, int64_t B, int64_t ldv, int64_t V,
                               const int32_t *group_start, const int32_t *group_start_host, int64_t n_groups,
                               float *mean, float *sample, float *tap, const mdbn_rng *rng, const float *v0,
                               float *cost_sum, void *workspace, int64_t workspace_bytes);
int  mdbn_cd_step_grouped(mdbn_ctx *ctx, void *stream, const mdbn_cd_args *a, const int32_t *group_start,
                          const int32_t *group_start_host, int64_t n_groups);

/* mdbn_updown_gen_step_grouped: the generative delta rule of up-down fine-tuning (mdbn_updown_gen_step) for the input layer
 * of a network with softmax groups: the arguments of mdbn_updown_gen_step without `gauss`, then the table under the
 * convention above.  The one conditional that changes is
 *   g = p(x_lo | x_hi) = softmax inside every group, sigmoid on the Bernoulli columns, of pre = x_hi G^T + vbias;
 * S = (x_lo - g)^T x_hi and s_v = sum_r (x_lo - g) are the exact gradient of sum_r log p(x_lo | x_hi) for a softmax as for a
 * sigmoid, and the rule, its divisors and `upd` are those of mdbn_updown_gen_step.  cost_out (nullable, device):
 * upd->cost_scale * sum_r -log p(x_lo | x_hi) = per group m + log sum_c exp(pre_c - m) - sum_c x_c pre_c (m = max_c pre_c:
 * finite where a probability underflows; every group of every row of x_lo must hold exactly one 1, not checked) plus the
 * cross-entropy of the Bernoulli columns: the cost of mdbn_group_softmax_sample against v0 = x_lo, minus the sum of
 * mdbn_propdown_rowll_grouped.
 *
 * path 2 (composed; any shape, and what path 0 takes outside the one-pass regime) is the composed path of the plain call with
 * the grouped means in place of the sigmoid: mdbn_propdown_sample(gauss = 1) stores the linear pre-activations, the kernel of
 * mdbn_group_softmax_sample turns them into means in place (v0 = x_lo, its cost partials, no sample), then the stacked
 * operands, mdbn_cd_stats and mdbn_apply_update with a throw-away hidden half; the partials are added in ascending order in
 * float64.  path 1 (one pass over G; n <= 32 rows, ldh <= 512, MDBN_EINVAL elsewhere) is the one-pass kernel of
 * mdbn_updown_gen_step with its workgroups' row ranges moved onto group boundaries -- a group belongs to the workgroup whose
 * nominal range holds its first row; a range grows by at most 63 rows and may be empty --: a row of G outside the span is
 * finished at once by the plain kernel's arithmetic (its new row of G and of the speed equal those of
 * mdbn_updown_gen_step(gauss = 0) on the same inputs bit for bit), a row inside the span leaves its pre-activations in LDS, one
 * thread per (group, minibatch row) forms the softmax there by the arithmetic of mdbn_group_softmax_sample (the hardware
 * exponential, Z in ascending c, correctly rounded means) and overwrites them with the errors, and a second walk over the span
 * rows reads the row of G once more (from cache) and the row of the speed for the first time and applies the rule.  G and its
 * speed are still written once, S is never stored, the pad columns H..ldh-1 are neither read nor written.  The kernel clamps
 * the device table to the span the host copy gives.  upd->W_planes, where given, are rewritten on every path.  No atomics,
 * every sum in a fixed order: two runs agree bit for bit.  No call synchronises.  Workspace:
 * mdbn_updown_gen_grouped_workspace_bytes (16-byte aligned).
 * MDBN_EINVAL with a message, before any launch and with every output untouched: n_groups < 1 (the plain call exists), an
 * invalid table (not ascending, a group of fewer than 2 or more than MDBN_GROUP_MAX columns, a boundary beyond V, a missing
 * copy), path = 1 on a shape the one-pass geometry does not serve, a short workspace, and whatever mdbn_updown_gen_step
 * refuses. */
int  mdbn_updown_gen_grouped_workspace_bytes(mdbn_ctx *ctx, int64_t n, int64_t V, int64_t H, int64_t ldv, int64_t ldh,
                                             int path, int64_t *bytes);
int  mdbn_updown_gen_step_grouped(mdbn_ctx *ctx, void *stream, const float *x_lo, const float *x_hi, int64_t n,
                                  const mdbn_update_args *upd, float *cost_out, int path, void *workspace,
                                  int64_t workspace_bytes, const int32_t *group_start, const int32_t *group_start_host,
                                  int64_t n_groups);

/* mdbn_ais_run_grouped: mdbn_ais_run (free, no clamp) for a Bernoulli layer whose visibles hold softmax groups: the
 * arguments of mdbn_ais_run, then the table under the convention above.  On one-hot rows
 *   log p*_beta(v) = sum_j softplus(beta a_j(v)) + v . b_beta
 * is the Bernoulli expression, so the weight update, the hidden draw, the double logw, the 2K - 1 Philox steps, the paths,
 * the traces and the cut of a long schedule are mdbn_ais_run's, bit for bit.  What changes is the visible draw, v_1 ~ p_0
 * included: on a group  v ~ softmax_c(x_c)  over its tempered pre-activations
 *   x_c = fma(beta, m_c, fma(beta, vbias_c - base_vbias_c, base_vbias_c)),   m = h W^T   (beta = 0, m = 0 for v_1)
 * with the arithmetic and the addressing of mdbn_group_softmax_sample: mx = max_c x_c, e_c = exp(x_c - mx) (the hardware
 * exponential), Z = sum_c e_c in ascending c in float32, mean_c = e_c / Z (correctly rounded), the category the first c with
 * u < C_c (C_c: the running float32 sum of the means) and the last one when none qualifies; ONE uniform per (chain, group),
 * the Philox word of the group's FIRST column (draw index 0, step rng->step + 2k, the global chain row) -- the uniforms of
 * its other columns are not used.  A Bernoulli column outside the span keeps mdbn_ais_run's draw, so n_groups = 0 gives
 * mdbn_ais_run's logw, v_state and traces bit for bit on both paths.  Every recorded visible row holds exactly one 1 per
 * group.  The base model changes with the draw (left to the caller, float64 on the host):
 *   log Z_A = H log 2 + sum_{Bernoulli i} softplus(base_vbias_i) + sum_g logsumexp_{c in g} base_vbias_c.
 * path 1 needs no LDS beyond mdbn_ais_run's image, so the shapes that fit are the same; workspace: mdbn_ais_workspace_bytes.
 * MDBN_EINVAL with a message, before any launch and with every output untouched: gauss, an invalid table (not ascending, a
 * group of fewer than 2 or more than MDBN_GROUP_MAX columns, a boundary beyond V, a missing copy), path = 1 on a shape
 * that does not fit, and whatever mdbn_ais_run refuses. */
int  mdbn_ais_run_grouped(mdbn_ctx *ctx, void *stream, const float *W, int64_t V, int64_t H, int64_t ldh,
                          const float *hbias, const float *vbias, const float *base_vbias, int gauss,
                          const float *betas, int64_t n_betas, int64_t M, int64_t ldv, float *v_state,
                          double *logw, float *trace_h, float *trace_v, int path, const mdbn_rng *rng,
                          void *workspace, int64_t workspace_bytes, const int32_t *group_start,
                          const int32_t *group_start_host, int64_t n_groups);

/* mdbn_pt_run_grouped: mdbn_pt_run / mdbn_pt_run_z for a Bernoulli layer whose visibles hold softmax groups: the arguments
 * of mdbn_pt_run_z (zacc and trace_work each nullable), then the table under the convention above.  On one-hot rows
 * log p*_beta(v) is the Bernoulli expression, so the swap decision, the works, the hidden draw, the rank map, the counts,
 * the 3 n Philox steps, the paths, the traces and the cuts of a long run are mdbn_pt_run_z's, bit for bit.  What changes is
 * the visible draw: on a group  v ~ softmax_c(x_c)  over its tempered pre-activations at the beta of the row's OWN rank,
 *   x_c = fma(beta, m_c, fma(beta, vbias_c - base_vbias_c, base_vbias_c)),   m = h W^T,
 * with the arithmetic and the addressing of mdbn_ais_run_grouped (mx, the hardware exponential, Z in ascending c, correctly
 * rounded means, the running sum C; the first c with u < C_c, the last one when none qualifies); ONE uniform per (replica
 * row, group): the Philox word of the group's FIRST column at step rng->step + 3t, draw index 0, the global replica row --
 * the uniforms of its other columns are not used.  s1 gets v_c (vbias - base_vbias)_c of every column, and from burn_in on
 * the top-rank row adds the group's softmax mean mean_c (not a sigmoid) to v_avg.  A Bernoulli column outside the span
 * keeps mdbn_pt_run's draw, so n_groups = 0 gives every output of mdbn_pt_run / mdbn_pt_run_z bit for bit on both paths.
 * Every recorded visible row holds exactly one 1 per group.  The base model of the ladder's log Z (betas[0] = 0; left to
 * the caller, float64 on the host):
 *   log Z_A = H log 2 + sum_{Bernoulli i} softplus(base_vbias_i) + sum_g logsumexp_{c in g} base_vbias_c.
 * path 1 needs no LDS beyond mdbn_pt_run's image, so the shapes that fit are the same; workspace:
 * mdbn_pt_run_z_workspace_bytes.  MDBN_EINVAL with a message, before any launch and with every output untouched: gauss, an
 * invalid table (the rules of mdbn_ais_run_grouped), and whatever mdbn_pt_run_z refuses. */
int  mdbn_pt_run_grouped(mdbn_ctx *ctx, void *stream, const float *W, int64_t V, int64_t H, int64_t ldh,
                         const float *hbias, const float *vbias, const float *base_vbias, int gauss,
                         const float *betas, int64_t R, int64_t M, int64_t ldv, float *v, float *h, int32_t *rank,
                         int64_t n_sweeps, int64_t burn_in, int64_t sweep0, int32_t *accepted, float *v_avg, float *h_avg,
                         float *trace_v, float *trace_h, int32_t *trace_swaps, int path, int64_t steps_per_launch,
                         const mdbn_rng *rng, void *workspace, int64_t workspace_bytes, double *zacc, double *trace_work,
                         const int32_t *group_start, const int32_t *group_start_host, int64_t n_groups);

/* mdbn_gibbs_clamped_grouped: mdbn_gibbs_clamped for a Bernoulli layer (no gauss, no add_noise) whose visibles hold
 * softmax groups: its arguments, then the table under the convention above.  The chain, the Philox steps (rng->step + 2t
 * hidden, rng->step + 2t + 1 visible, draw 0), burn_in, the accumulators, the taps, path and steps_per_launch are
 * mdbn_gibbs_clamped's.  What changes:
 *   visible draw of a group: v ~ softmax_c(x_c), x_c = (h_sample W^T)_c + vbias_c, with the arithmetic and the addressing of
 *     mdbn_group_softmax_sample (mx, e_c = exp(x_c - mx), Z in ascending c, mean_c = e_c / Z correctly rounded, the first c
 *     with u < C_c, else the last); ONE uniform per (row, group): the Philox word of the group's FIRST column.  v_mean of a
 *     group column is mean_c.  A Bernoulli column outside the span keeps mdbn_gibbs_clamped's draw.
 *   clamp of a group: a group is held or free as a WHOLE, by the mask entry at its FIRST column (the mask entries at its
 *     other columns are not read): defined for any mask, no device-side check.  A held group's columns are put back to obs as
 *     they are (any real values: they enter through v W alone).  Every recorded row of a free group holds exactly one 1.
 * n_groups = 0 reads no table and gives mdbn_gibbs_clamped(gauss = 0) bit for bit on both paths.  path 1 needs no LDS beyond
 * mdbn_gibbs_clamped's image, so the shapes that fit are the same; path 2 runs per step the propup pass, a propdown pass to the
 * linear pre-activations (into v_mean) and ONE kernel that draws, clamps, accumulates and taps.  Workspace:
 * mdbn_gibbs_clamped_workspace_bytes.  MDBN_EINVAL with a message, before any launch: an invalid table (not ascending, a
 * group of fewer than 2 or more than MDBN_GROUP_MAX columns, a boundary beyond V, a missing copy) and whatever
 * mdbn_gibbs_clamped refuses. */
int  mdbn_gibbs_clamped_grouped(mdbn_ctx *ctx, void *stream, float *v, const float *obs, const float *mask,
                                int64_t mask_rows, int64_t B, int64_t ldv, const float *W, int64_t V, int64_t H,
                                int64_t ldh, const float *hbias, const float *vbias, int64_t n_steps, int64_t burn_in,
                                float *h_mean, float *h_sample, float *v_mean, float *v_avg, float *h_avg,
                                float *trace_h, float *trace_v, int path, int64_t steps_per_launch,
                                const mdbn_rng *rng, void *workspace, int64_t workspace_bytes,
                                const int32_t *group_start, const int32_t *group_start_host, int64_t n_groups);

/* mdbn_ais_cond_run_grouped: mdbn_ais_cond_run for a Bernoulli layer (no gauss) whose visibles hold softmax groups: its
 * arguments without `gauss`, then the table under the convention above.  The run is mdbn_ais_cond_run(gauss = 0): N C
 * chains, chain m clamped to data row m / C, the 2K - 1 Philox steps and their addressing, the double logw, the traces, the
 * cut of a long schedule and path.  What changes:
 *   visible draw of a free group (v_1 ~ p_0 included): mdbn_ais_run_grouped's -- v ~ softmax_c(x_c) over
 *     x_c = fma(beta, m_c, fma(beta, vbias_c - base_vbias_c, base_vbias_c)), ONE uniform per (chain, group): the Philox word
 *     of the group's FIRST column.  A Bernoulli column outside the span keeps mdbn_ais_cond_run's draw and clamp.
 *   clamp of a group: mdbn_gibbs_clamped_grouped's rule -- a group is held or free as a WHOLE, by the mask entry at its FIRST
 *     column in the chain's mask row (the entries at its other columns are not read): defined for any mask, no device-side
 *     check.  A held group's columns take obs as they are (any real values: they enter through v W alone) and add 0.f to s1,
 *     each at its own place in the free run's sum; its uniform is drawn and not used.
 * Two limits, bit for bit in logw, v_state and both traces on both paths: n_groups = 0 is mdbn_ais_cond_run(gauss = 0); a mask
 * of zeros is mdbn_ais_run_grouped with M = N C.  The base model of data row r (left to the caller, float64 on the host):
 *   log Z_A,r = H log 2 + sum_{free Bernoulli i} softplus(base_vbias_i) + sum_{free groups g} logsumexp_{c in g} base_vbias_c.
 * path 1 needs no LDS beyond mdbn_ais_run's image; workspace: mdbn_ais_cond_workspace_bytes.  MDBN_EINVAL with a message,
 * before any launch and with every output untouched: an invalid table (not ascending, a group of fewer than 2 or more than
 * MDBN_GROUP_MAX columns, a boundary beyond V, a missing copy), path = 1 on a shape that does not fit, and whatever
 * mdbn_ais_cond_run refuses. */
int  mdbn_ais_cond_run_grouped(mdbn_ctx *ctx, void *stream, const float *W, int64_t V, int64_t H, int64_t ldh,
                               const float *hbias, const float *vbias, const float *base_vbias, const float *betas,
                               int64_t n_betas, const float *obs, const float *mask, int64_t mask_rows, int64_t N,
                               int64_t C, int64_t ldv, float *v_state, double *logw, float *trace_h, float *trace_v,
                               int path, const mdbn_rng *rng, void *workspace, int64_t workspace_bytes,
                               const int32_t *group_start, const int32_t *group_start_host, int64_t n_groups);

/* mdbn_propdown_rowll_grouped: mdbn_propdown_rowll (no `gauss`) for a Bernoulli layer whose visibles hold softmax groups --
 * the directed term of the input layer in the variational bound of a stack on categorical data: its arguments without
 * `gauss`, then the table under the convention above.  With pre_c = h[r] . W[c, :] + vbias_c and t = target[r / target_div],
 *   out[r] = sum over groups g of ( sum_{c in g} t_c pre_c - m_g - log sum_{c in g} exp(pre_c - m_g) ),  m_g = max_{c in g} pre_c,
 *          + sum over the columns outside the span of ( t_i pre_i - softplus(pre_i) )
 * -- log softmax per group at the target's 1, finite at |pre| in the hundreds.  The group term is linear in t: the kernel
 * never looks for the 1, and on a target row that is not one-hot in a group (precondition; the Python layer checks it) the
 * value is that expression, not a log-probability.  The pre-activations exist in accumulators and, a 64 x 128 half tile at a
 * time, in LDS only: main loop, tiling and products are mdbn_propdown_rowll's.  A group that crosses the edge of a
 * 128-column tile (at most one edge: a group has at most MDBN_GROUP_MAX = 64 columns) leaves (max, sum of exp) of its two
 * parts in the workspace and the second small launch, which adds a row's tiles in ascending order, joins them as
 * M + log(s_a exp(m_a - M) + s_b exp(m_b - M)).  No atomics: two runs agree bit for bit.  The padding of h and W beyond H and
 * of target beyond V is never used.  workspace: >= mdbn_rowll_grouped_workspace_bytes(R, V, H) (five floats per row and
 * column tile).  MDBN_EINVAL with a message, before any launch and with out untouched: n_groups < 1 (a layer without groups
 * has mdbn_propdown_rowll), an invalid table (not ascending, a group of fewer than 2 or more than MDBN_GROUP_MAX columns, a
 * boundary beyond V, a missing copy), V > 2^24, a short workspace, and whatever mdbn_propdown_rowll refuses. */
int  mdbn_rowll_grouped_workspace_bytes(mdbn_ctx *ctx, int64_t R, int64_t V, int64_t H, int64_t *bytes);
int  mdbn_propdown_rowll_grouped(mdbn_ctx *ctx, void *stream, const float *h, int64_t R, int64_t ldh, const float *W,
                                 int64_t V, int64_t H, const float *vbias, const float *target, int64_t ldv,
                                 int64_t target_div, float *out, void *workspace, int64_t workspace_bytes,
                                 const int32_t *group_start, const int32_t *group_start_host, int64_t n_groups);

/* Classification RBM (added by this engine; Larochelle & Bengio 2008): a one-hot label block in columns lo .. lo + K - 1 of the
 * visible layer (2 <= K <= MDBN_GROUP_MAX; passed as host integers, no device table is read), everything outside the block
 * counting as input.  With x~ = the row with the block set to zero, A = hbias + x~ W (ONE propup, shared by all classes),
 * U = rows lo .. lo + K - 1 of W and d = vbias[lo .. lo + K):
 *   o[y][j] = A[j] + U[y][j],   a[y] = d[y] + sum_j softplus(o[y][j]),   p(y | x) = softmax_y a[y]
 * which is softmax_y(-F(row with category y)) exactly: the terms of F that do not depend on y cancel.
 *
 * mdbn_class_posterior: post [B, ldk] (float32; ldk >= K, columns K.. untouched) = p(. | x) for the rows v [B, ldv] -- what v
 * holds inside the block is ignored unless logp (nullable, [B]) is given, which receives log p(y* | x) for the category y* the
 * block holds (a row whose block holds no 1 leaves its entry untouched).  Launches: the kernel that writes x~, the propup
 * (pre-activations only), the class kernel -- two passes over (y, j) per row, scores then softmax; every element forms
 * e = exp(-|z|) once and softplus(z) = max(z, 0) + log(1 + e) from it, finite for any finite z.  No random numbers.
 *
 * mdbn_class_stats: the exact gradient of sum_rows log p(y* | x), ascent direction like CD's, in the packed layout of
 * mdbn_cd_args.stats, scaled by disc_weight w and added to gen_weight times the CD statistics:
 *   r_pos = sigmoid(o[y*][.]),  r_bar = sum_y p(y | x) sigmoid(o[y][.])
 *   S[i][.]      (i outside the block) = sum_rows x_i (r_pos - r_bar)      s_h = sum_rows (r_pos - r_bar)
 *   S[lo + y][.]                       = sum_rows ([y = y*] - p(y | x)) sigmoid(o[y][.])
 *   s_v[lo + y] = sum_rows ([y = y*] - p(y | x)),  s_v elsewhere = 0
 * gen_weight > 0 (hybrid): V2 [2B, ldv] = [v0; nv] and P2 [2B, ldh] = [ph; -nh] are the scratch a finished
 * mdbn_cd_step_grouped (or mdbn_cd_step with keep_f32) left; the cost slot of `stats` is kept.  gen_weight = 0 (pure): V2 holds
 * the B gathered rows v0 only, P2 is not read (may be NULL), and the cost slot receives -sum_rows log p(y* | x).  Both forms
 * run ONE statistics GEMM, the unchanged mdbn_cd_stats, on stacked operands in the workspace:
 *   hybrid  V2' = [v0; v0 | nv; x~]   P2' = [gen ph; w r_pos | -gen nh; -w r_bar]      (4B rows)
 *   pure    V2' = [v0 | x~]           P2' = [w r_pos | -w r_bar]                       (2B rows)
 * With x~'s block zero the GEMM leaves gen (CD part) + w sum_rows [y = y*] r_pos in the block's rows of S; the patch kernel then
 * subtracts w T[y][.], T[y][.] = sum_rows p(y | x) sigmoid(o[y][.]), and rebuilds s_v whole as gen (sum v0 - sum nv) + w n
 * (s_h is the column sum of P2' and needs no patch).  T, n and the log-likelihood go through per-workgroup partials summed in
 * ascending order; nll_sum (nullable, device scalar) receives -sum_rows log p(y* | x) at the parameters given.  Every block of
 * every row of v0 must hold exactly one 1 (not checked).  W, hbias, vbias are read only.
 *
 * No atomics, every sum in a fixed order: two runs agree bit for bit.  Pad columns H..ldh-1 and V..ldv-1 of the caller's
 * matrices are neither read nor written, except what mdbn_cd_stats itself does to `stats`.  No call synchronises.
 * mode of the sizer: 0 = mdbn_class_posterior, 1 = mdbn_class_stats with gen_weight = 0, 2 = with gen_weight > 0.
 * MDBN_EINVAL with a message, before any launch and with every output untouched: sizes < 1 or > 2^24, null or misaligned
 * matrices, a leading dimension below its width or not a multiple of 4, K < 2 or K > MDBN_GROUP_MAX, lo < 0 or lo + K > V,
 * a negative or non-finite weight, both weights 0, gen_weight > 0 without P2; a short workspace is MDBN_ENOSPC. */
#define MDBN_CLASS_POSTERIOR 0
#define MDBN_CLASS_PURE      1
#define MDBN_CLASS_HYBRID    2
int  mdbn_class_workspace_bytes(mdbn_ctx *ctx, int64_t B, int64_t V, int64_t H, int64_t ldv, int64_t ldh, int64_t K,
                                int mode, int64_t *bytes);
int  mdbn_class_posterior(mdbn_ctx *ctx, void *stream, const float *v, int64_t B, int64_t ldv, const float *W, int64_t V,
                          int64_t H, int64_t ldh, const float *hbias, const float *vbias, int64_t lo, int64_t K,
                          float *post, int64_t ldk, float *logp, void *workspace, int64_t workspace_bytes);
int  mdbn_class_stats(mdbn_ctx *ctx, void *stream, const float *V2, const float *P2, int64_t B, const float *W, int64_t V,
                      int64_t H, int64_t ldv, int64_t ldh, const float *hbias, const float *vbias, int64_t lo, int64_t K,
                      float gen_weight, float disc_weight, float *stats, float *nll_sum, void *workspace,
                      int64_t workspace_bytes);

/* Absent visible units (added by this engine; Salakhutdinov, Mnih & Hinton 2007): training on tables with missing entries.
 * NaN in a row means "this row did not observe this unit"; such a unit is absent from that row's RBM, every row has its own
 * RBM over the set O_r it observed, and all rows share W, hbias, vbias.  With m_ri = [i in O_r] and v~ = m o v (0 where absent):
 *   h | v:  sigmoid(hbias + v~ W);   v_i | h, i in O_r: as mdbn_cd_step draws it;  i not in O_r: 0
 *   S = sum_r v~0_r' ph_r - n~v_r' nh_r,   s_h = sum_r ph_r - nh_r,   s_v[i] = sum_r m_ri (v0_ri - nv_ri)
 * -- CD with a per-row mask, the CD approximation of the gradient of sum_rows log p_{O_r}(v_{r, O_r}).  A row that observed
 * nothing has ph = nh bit for bit and contributes nothing.  The divisors of the update stay the batch size: the step is the
 * gradient of the MEAN log-likelihood per row, not renormalised per column.
 *
 * mdbn_absent_split: x [B, ldx] may hold NaN in columns < V (only NaN marks a missing entry; +-inf are values).  filled
 * [B, ld_filled] receives x with 0 where missing (filled may be x: in place); observed [B, words], words = (V + 31) / 32,
 * bit (i & 31) of word (i >> 5) set when entry i is observed, bits of columns >= V zero; row_count [B] (nullable) the number
 * of observed entries of each row.  Pad columns are neither read nor written.
 *
 * mdbn_absent_visible: p(v | h) of such rows from the linear pre-activations pre [B, ldv] = h W^T + vbias, with the geometry
 * and Philox addressing of mdbn_group_softmax_sample without groups (one uniform per column and 4-row block at rng->draw; the
 * normal of a noisy Gaussian layer at rng->draw | the normal bit).  gauss = 0: mean = sigmoid(pre), sample = (u < mean) --
 * with every bit set bit for bit mdbn_propdown_sample's --; gauss = 1: mean = pre, sample = mean [+ N(0, 1) if add_noise].
 * Absent entries of mean / sample / tap (each nullable, mean may be pre) are exactly 0.  With v0 (zero-filled) cost_sum[0]
 * receives the sum over OBSERVED entries of the cross-entropy (gauss = 0) or of (sigmoid(pre) - v0)^2 (gauss = 1), through
 * per-workgroup partials in `workspace` (mdbn_absent_visible_workspace_bytes).  Pad columns are neither read nor written.
 *
 * mdbn_cd_step_absent: mdbn_cd_step_grouped's composition on a->data rows that may hold NaN: gather, mdbn_absent_split in
 * place on rows 0..B-1 of V2, propup; k x [linear propdown, the masked visible kernel, propup from the masked 0/1 sample --
 * gauss: from the masked mean --]; mdbn_cd_stats.  It leaves V2 = [v~0; n~v], P2 = [ph; -nh], hs, vs (required, for Gaussian
 * layers too: the masked sample), the packed statistics with the cost above of the last step in the cost slot, and trace_h /
 * trace_v when given.  Draw numbering of mdbn_cd_step_grouped.  The plane, keep_f32 and gather-ahead fields are ignored.  The
 * mask words and the cost partials live in a->workspace behind the step's own: mdbn_cd_step_absent_workspace_bytes is exact.
 *
 * mdbn_absent_mark_rows: rows of y [N, ld] whose row_count is 0 become NaN in columns < cols.
 *
 * mdbn_free_energy_absent: F_O(x_r) over the observed units of every row of x [N, ldv] (NaN = missing):
 *   gauss = 0:  -sum_{i in O} b_i v_i - sum_j softplus(c_j + (v~ W)_j)
 *   gauss = 1:  1/2 sum_{i in O} (v_i - b_i)^2 - sum_j softplus(c_j + (v~ W)_j)
 * = mdbn_free_energy of the zero-filled rows, minus 1/2 sum_{i not in O} b_i^2 for a Gaussian layer (summed per row in a
 * fixed order).  x is not written; the zero-filled copy lives in the workspace.
 *
 * No atomics, every sum in a fixed order: two runs agree bit for bit.  No call synchronises.  MDBN_EINVAL with a message,
 * before any launch and with every output untouched: sizes < 1 or > 2^24, null or misaligned pointers, a leading dimension
 * below its width or not a multiple of 4, sampling without rng, v0 without cost_sum, and for the step a->persistent,
 * a->sample_stats and what mdbn_cd_step refuses; a short workspace is MDBN_ENOSPC, likewise before any launch. */
int  mdbn_absent_split(mdbn_ctx *ctx, void *stream, const float *x, int64_t B, int64_t ldx, int64_t V, float *filled,
                       int64_t ld_filled, uint32_t *observed, int32_t *row_count);
int  mdbn_absent_visible_workspace_bytes(mdbn_ctx *ctx, int64_t B, int64_t V, int64_t *bytes);
int  mdbn_absent_visible(mdbn_ctx *ctx, void *stream, const float *pre, int64_t B, int64_t ldv, int64_t V,
                         const uint32_t *observed, int gauss, int add_noise, float *mean, float *sample, float *tap,
                         const mdbn_rng *rng, const float *v0, float *cost_sum, void *workspace, int64_t workspace_bytes);
int  mdbn_cd_step_absent_workspace_bytes(mdbn_ctx *ctx, int64_t B, int64_t V, int64_t H, int64_t ldv, int64_t ldh,
                                         int64_t *bytes);
int  mdbn_cd_step_absent(mdbn_ctx *ctx, void *stream, const mdbn_cd_args *a);
int  mdbn_absent_mark_rows(mdbn_ctx *ctx, void *stream, float *y, int64_t N, int64_t ld, int64_t cols,
                           const int32_t *row_count);
int  mdbn_free_energy_absent_workspace_bytes(mdbn_ctx *ctx, int64_t N, int64_t V, int64_t H, int64_t ldv, int64_t *bytes);
int  mdbn_free_energy_absent(mdbn_ctx *ctx, void *stream, const float *x, int64_t N, int64_t ldv, const float *W, int64_t V,
                             int64_t H, int64_t ldh, const float *hbias, const float *vbias, int gauss, float *out,
                             void *workspace, int64_t workspace_bytes);

/* Pieces of get_pseudo_likelihood_cost (src/rbm.py:421-447): out = round(x) (tensor.round: half away from
 * zero) with column flip_col replaced by 1 - round(x) (flip_col < 0: no flip); then, from the free energies of
 * the two matrices, cost_out[0] = -mean(n_visible * softplus(fe - fe_flip)) (the float32 softplus terms summed in
 * float64, rounded once).  The rounding is exact for every float32 (0.49999997 -> 0, 8388609 stays; the sign of x is
 * kept on a zero result, NaN stays NaN); the pad columns cols..ld-1 of `out` are WRITTEN, as zero -- x's own pad columns
 * are not read. */
int  mdbn_round_flip(mdbn_ctx *ctx, void *stream, const float *x, int64_t rows, int64_t cols, int64_t ld,
                     int64_t flip_col, float *out);
int  mdbn_pl_cost(mdbn_ctx *ctx, void *stream, const float *fe, const float *fe_flip, int64_t rows,
                  int64_t n_visible, float *cost_out);
/* get_reconstruction_cost on given arrays: RBM src/rbm.py:449-482 (cross-entropy of sigmoid(pre) against
 * target, summed over units, mean over rows), GRBM src/rbm.py:690-699 (mean of (sigmoid(pre) - target)^2). */
int  mdbn_recon_cost(mdbn_ctx *ctx, void *stream, const float *pre, int64_t ld_pre, const float *target,
                     int64_t ld_target, int64_t rows, int64_t cols, int gauss, float *cost_out,
                     void *workspace, int64_t workspace_bytes);
/* HiddenLayer's tanh activation (src/mlp.py:36-110 default), in place on the live columns */
int  mdbn_tanh(mdbn_ctx *ctx, void *stream, float *x, int64_t rows, int64_t cols, int64_t ld);
/* count[0] += number of NaN / Inf values in x[0..n): the check NanGuardMode would make (src/rbm.py:542-543,
 * src/dbn.py:311); the caller zeroes count */
int  mdbn_count_nonfinite(mdbn_ctx *ctx, void *stream, const float *x, int64_t n, int32_t *count);

/* bfloat16 wire format of the data-parallel statistics (opt-in reporting mode MDBN_WIRE_BF16=1, never a
 * parity path): dst[i] = bfloat16(src[i]) with round-to-nearest-even, and the exact widening back.  n elements; both
 * buffers 16-byte aligned (MDBN_EINVAL otherwise, without a launch).  FLT_MAX rounds to inf; a NaN stays a NaN of its sign,
 * also one whose payload lies in the dropped half.  Subnormal float32 inputs are rounded to nearest even as well, not
 * flushed to zero (measured on the MI355X: 0x00018000 -> 0x0002, 0x007FFFFF -> 0x0080, 0x00008000 and 0x00000001 -> 0). */
int  mdbn_f32_to_bf16(mdbn_ctx *ctx, void *stream, const float *src, void *dst, int64_t n);
int  mdbn_bf16_to_f32(mdbn_ctx *ctx, void *stream, const void *src, float *dst, int64_t n);

/* the random matrices themselves (tests, and sampling utilities) */
int  mdbn_rng_uniform(mdbn_ctx *ctx, void *stream, float *out, int64_t rows, int64_t cols,
                      int64_t ld, const mdbn_rng *rng);
int  mdbn_rng_normal(mdbn_ctx *ctx, void *stream, float *out, int64_t rows, int64_t cols,
                     int64_t ld, const mdbn_rng *rng);
/* host-side twin of mdbn_rng_uniform (no GPU needed) */
int  mdbn_philox_host(float *out, int64_t rows, int64_t cols, int64_t ld, const mdbn_rng *rng);

#ifdef __cplusplus
}
#endif
#endif /* MDBN_HIP_H */
