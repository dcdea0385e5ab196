/*
 * flashgmm_amd.h — C ABI of libflashgmm_amd.so, the MI355X (gfx950) GMM entropy-coding path.
 *
 * This is the drop-in boundary for ONE path of tokkiwa/FlashGMM: what its pybind11 module `compressai.ans`
 * exposes for Gaussian-mixture conditionals, and the tensor preparation its Python entropy model does right
 * above that call.  Plain pointers and sizes only; no torch / pybind types.  All functions return an
 * fgmm_status (0 = OK) and never throw across the ABI.
 *
 * Reference interfaces replaced (paths relative to the reference repo):
 *   - RansEncoder::encode_with_indexes_gmm<4>   compressai/cpp_exts/rans/rans_interface.cpp:609-617 (-> :458-554, :557-585)
 *   - RansDecoder::decode_with_indexes_gmm<4>   compressai/cpp_exts/rans/rans_interface.cpp:766-883
 *   - pybind signatures / keyword names         compressai/cpp_exts/rans/rans_interface.cpp:977-1004, :1026-1035
 *   - GaussianMixtureConditional.compress       compressai/entropy_models/entropy_models.py:833-867
 *   - GaussianMixtureConditional.decompress     compressai/entropy_models/entropy_models.py:872-910
 *   - reshape_entropy_parameters (+clamp)       compressai/entropy_models/entropy_models.py:810-828
 *   - APPROX_MODE numbering                     compressai/cpp_exts/rans/rans_interface.cpp:224-232
 *
 * Division of labour (BASELINE.json north_star): every floating-point operation — the K=4 mixture CDF in one
 * of three Phi approximations, 16-bit quantisation, bypass detection, the decode-side per-latent edge tables —
 * runs in hand-written HIP kernels; the integer rANS state machine runs on host threads fed by pinned
 * hipMemcpyAsync copies of the GPU-built tables.  There is NO CPU implementation of the float work in this
 * library: with no usable HIP device every entry point that needs one returns FGMM_ERR_NO_DEVICE.
 *
 * Parameter addressing.  A mixture parameter of latent (channel c, position p), component k lives at
 *     base[k*stride_k + c*stride_c + p*stride_p]           (strides in ELEMENTS)
 *   - latent-codec layout [1, K*M, h, w] (channel = k*M + c): stride_k = M*h*w, stride_c = h*w, stride_p = 1
 *   - the reference's (n, K) accessor views:                 one channel, stride_p = stride(0), stride_k = stride(1)
 * `memspace` says where the parameter / symbol pointers live: FGMM_DEVICE pointers are used in place,
 * FGMM_HOST buffers are staged through pinned memory and copied to the GPU first (PCIe-inclusive path).
 */
#ifndef FLASHGMM_AMD_H
#define FLASHGMM_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FGMM_ABI_VERSION 6 /* 6: + the parameter head (fgmm_head_*, fgmm_gmc_compress_head_batch); + fgmm_sink and the _to forms of the batched
                              compress calls; FGMM_WORKER_CPUS that cannot be honoured fails fgmm_ctx_create.  5: + fgmm_ctx_call_log; REMOVED (measured, lost, pruned): options tab_place /
                              tab_spin / copy_engine / dec_pair / dec_group, fgmm_rans_decode_tab2 + fgmm_tab_ref, fgmm_ctx_stat index 6.
                              Added since without a bump (nothing existing changed): section 3b, the coded size without running the coder; section 3c,
                              rate-distortion optimised quantisation.  fgmm_abi_version() therefore does NOT tell a caller whether 3b / 3c are
                              there: at compile time test FGMM_HAS_ESTIMATE / FGMM_HAS_RDOQ below, at run time look the symbol up
                              (dlsym(handle, "fgmm_gmc_rdoq_batch")) */
#define FGMM_HAS_ESTIMATE 1 /* section 3b: fgmm_gmc_estimate_batch, fgmm_symtab_bits[_hip], fgmm_rate_stream_bytes */
#define FGMM_HAS_RDOQ 1     /* section 3c: fgmm_gmc_rdoq_batch */
#define FGMM_HAS_RDCURVE 1  /* section 3d: fgmm_gmc_rdcurve_batch, fgmm_gmc_rdoq_budget_batch */
#define FGMM_RDCURVE_MAX 16 /* lambdas per fgmm_gmc_rdcurve_batch call */
#define FGMM_HAS_RDO_SKIP 1    /* section 3f: fgmm_gmc_rdoq_batch_s, fgmm_gmc_rdcurve_batch_s, fgmm_gmc_rdoq_budget_batch_s (added without a bump, as 3b - 3e) */
#define FGMM_HAS_RDO_WEIGHTS 1 /* section 3e: fgmm_gmc_rdoq_batch_w, fgmm_gmc_rdcurve_batch_w, fgmm_gmc_rdoq_budget_batch_w (added without a bump, as 3b - 3d) */
#define FGMM_HAS_BF16 1        /* section 2: FGMM_BF16 parameter planes in every call that takes planes (added without a bump, as 3b - 3f) */
#define FGMM_HAS_LIKELIHOOD 1  /* section 3g: fgmm_gmc_likelihood_batch, fgmm_gmc_likelihood_backward_batch (added without a bump, as 3b - 3f) */
#define FGMM_HAS_LIKELIHOOD_LOGITS 1 /* section 3h: fgmm_gmc_likelihood_logits_batch, fgmm_gmc_likelihood_logits_backward_batch (added without a bump, as 3b - 3g) */
#define FGMM_HAS_CENTROID 1  /* section 3i: fgmm_gmc_centroid_batch (added without a bump, as 3b - 3h) */
#define FGMM_HAS_EB 1        /* section 3j: fgmm_eb_likelihood, fgmm_eb_likelihood_backward (added without a bump, as 3b - 3i) */
#define FGMM_HAS_CKBD_CONTEXT 1 /* section 5b: fgmm_ckbd_ctx_create, fgmm_ckbd_ctx_destroy, fgmm_ckbd_ctx_apply (added without a bump, as 3b - 3j) */
#define FGMM_HAS_EB_UPDATE 1 /* section 3k: fgmm_eb_quantiles, fgmm_eb_tables (added without a bump, as 3b - 3j) */
#define FGMM_EB_SEARCH_CAP 256 /* section 3k: bisection steps of one quantile search at the most */
#define FGMM_EB_PARAMS 58    /* float32 values per channel of section 3j's theta */
#define FGMM_EB_SLICE 1024   /* section 3j: elements of a channel one workgroup walks; the backward's partial rows per channel are
                                ceil(B*hw / FGMM_EB_SLICE) */
#define FGMM_RDO_W_MAX 256.0f  /* largest factor of a weighted call's chan_w / pos_w */

typedef enum {
  FGMM_OK = 0,
  FGMM_ERR_INVALID = 1,     /* bad argument (null pointer, K != 4, negative size, unknown mode ...) */
  FGMM_ERR_NO_DEVICE = 2,   /* no HIP device / HIP runtime error at context creation */
  FGMM_ERR_HIP = 3,         /* a HIP call failed; fgmm_last_error() has the text */
  FGMM_ERR_NOMEM = 4,
  FGMM_ERR_STREAM = 5,      /* bitstream shorter than the symbols it is asked to yield (corrupt input) */
  FGMM_ERR_UNSUPPORTED = 6, /* outside the built envelope (e.g. max_bs_value > FGMM_MAX_BS) */
  FGMM_BUDGET_UNMET = 7     /* NOT an error, never a return value: fgmm_budget_result.status of a group whose byte budget no lambda up to
                               lambda_max meets (section 3d) */
} fgmm_status;

/* Phi approximation, numbered as the reference CODE numbers APPROX_MODE (the README swaps 1 and 2). */
typedef enum { FGMM_MODE_POLYA = 0, FGMM_MODE_AS = 1, FGMM_MODE_LOGISTIC = 2 } fgmm_mode;

typedef enum { FGMM_HOST = 0, FGMM_DEVICE = 1 } fgmm_memspace;

#define FGMM_K 4              /* the reference binds K = 4 only (rans_interface.cpp:60,982,1003,1033) */
#define FGMM_MAX_BS 1073741822 /* largest decoder half-width (abs_max + 1): 2^30 - 2, so that 2*max_bs + 2 fits an int32.
                                 Beyond 16382 headers are 8 bytes and rows are built by the generic two-pass kernels,
                                 which refuse (FGMM_ERR_UNSUPPORTED) a latent whose evaluation window — what is left of
                                 [-max_bs, max_bs+1] between the provably saturated tails — exceeds 2^20 edges */
#define FGMM_MAX_BS_H4 16382  /* largest half-width the 4-byte header form can carry */

typedef struct fgmm_ctx fgmm_ctx; /* one per process per GPU: streams, pinned staging, workspaces, host threads */

int fgmm_abi_version(void);
const char *fgmm_last_error(void); /* thread-local text of the last failure on this thread */

/* What this process may use of the host: *cpus_out = min(CPUs of its affinity mask, CPUs per period of its cgroup quota —
 * cpu.max of cgroup v2 / cpu.cfs_quota_us of v1, ancestors included); *affinity_out / *quota_out the two terms (quota < 0:
 * none).  Any out-pointer may be NULL. */
int fgmm_host_cpu_budget(double *cpus_out, int *affinity_out, double *quota_out);
/* Host rANS workers a context gets by default when `ranks_sharing` processes (one per GPU) share that budget: the share's CPUs,
 * floor(budget / ranks_sharing) - or, where a cgroup quota (CPU TIME per period) is what limits the budget and the affinity mask is
 * wider, up to FGMM_WORKERS_PER_CPU (environment, 1..4, default 3) workers per CPU of the share (never more than the share of the mask):
 * the workers sleep on the copies' events most of a call, so the bursts of a step run on as many cores while the quota is not exhausted
 * (48 workers under a 16-CPU quota use 14-15 CPUs' worth and are 5 % faster than 16: profiles/r05_stall_diagnosis.md).  Within [1, 48]. */
int fgmm_host_thread_budget(int ranks_sharing);

/* device < 0: current HIP device.  n_threads <= 0: fgmm_host_thread_budget(1) host rANS workers. */
int fgmm_ctx_create(int device, int n_threads, fgmm_ctx **out);
void fgmm_ctx_destroy(fgmm_ctx *ctx);
int fgmm_ctx_device(const fgmm_ctx *ctx);
int fgmm_ctx_threads(const fgmm_ctx *ctx);
/* Resizes the context's pool of host rANS workers in place (n_threads <= 0: the default); options, profiling state and
 * buffers are kept.  Must not race with a call on the same context (it takes the context's lock like every call). */
int fgmm_ctx_set_threads(fgmm_ctx *ctx, int n_threads);
/* Where the context's host workers may run, as a Linux cpulist ("" = wherever the thread that created the context may).  The workers
 * stream the decode-side tables through the L3 of the core complex they run on; a calling thread that shares that L3 - a Python
 * interpreter above all - pays for it between the calls (0.9 - 1.5 ms of glue per Kodak step instead of 0.5).  Decided when the context
 * is created, from the environment variable FGMM_WORKER_CPUS:
 *   unset      the creating thread's CPUs minus those that share an L3 with the CPU it is on (if >= 32 CPUs and two per worker remain)
 *   "inherit"  the creating thread's CPUs
 *   a cpulist  exactly these, e.g. "16-127" (what the kernel grants of them to a thread of this process: the list within the process's
 *              cpuset; fgmm_ctx_worker_cpus reports that).  A value that is not a cpulist, or of which no CPU is granted, makes
 *              fgmm_ctx_create fail with FGMM_ERR_INVALID - never a silent fall back onto the creating thread's L3
 * The library never changes the calling thread's own affinity; a caller that wants the full benefit keeps its thread on the CPUs
 * that are NOT in this list (bench.py does, for its timed regions).
 * The DECODE calls run on a second pool of as many workers confined to ONE hardware thread per core of that list (two sequential
 * decoders on one core's two hardware threads cost 14 % more CPU time than on two cores; the encode call wants every hardware thread):
 * FGMM_DECODE_SMT=1 in the environment keeps the decoders on the list as it is. */
int fgmm_ctx_worker_cpus(fgmm_ctx *ctx, char *cpulist_out, size_t cap);

void fgmm_free(void *p); /* releases any buffer this library returned through an out-pointer */
/* Moves `count` buffers this library returned (src[i], len[i] bytes: bitstreams of a batched compress) into the caller's own
 * storage dst[i] and releases them - the copies run on the context's host workers.  What a binding does instead of `count`
 * single-threaded copies when its language wants to own the bytes (Python: 30 MB of bitstreams of eight 4K images, 3 ms). */
int fgmm_ctx_take_buffers(fgmm_ctx *ctx, void *const *dst, void *const *src, const size_t *len, int count);

/* Tuning knobs of a context (defaults in brackets; what was measured behind each: DESIGN.md).  Unknown names return FGMM_ERR_INVALID.
 *   "pieces"      [0]   decode: the tables of every bitstream of a call reach the host in this many pieces, piece-major and shrinking
 *                       (at most 32; 0 = by the call's longest bitstream: 8 up to 147 k latents, 24 from 1.1 M on); the host workers take
 *                       (bitstream, piece) tasks once their tables have landed, the coder state travels with the bitstream from
 *                       worker to worker
 *   "dec_first"   [2]   decode: bitstreams in the first launch of the first round of pieces (doubling from there: first tables early)
 *   "enc_ways"    [0]   encode: consecutive bitstreams one worker codes symbol by symbol in turn (several dependency chains share a
 *                       core): 1..4; 0 = two when the call has more bitstreams than workers, else one
 *   "enc_segs"    [1]   encode: a call in which every bitstream has a host worker of its own (and whose tables are 4 MB and more) lays
 *                       every table out in four segments of compact channels, LAST SEGMENT FIRST across all bitstreams: rANS encodes
 *                       backwards, so the encoders follow the landing.  0 = whole tables, bitstream after bitstream
 *   "scatter_rounds" [1] decode: decoded symbols return to the GPU round by round (one launch per piece index) instead of one launch per
 *                       bitstream when it has finished
 *   "tab_cap_e"   [12288] single-pass table kernel: edges one block keeps in LDS (latents per block = cap / (2*max_bs+2)); at the
 *                       default a call with a half-width that only fits 16384 edges (383 < max_bs <= 511) gets that
 *   "stage_max_mb" [0]  decode: cap of the device staging area for rows in MiB (0: a quarter of the free device memory).  A launch
 *                       whose rows do not fit is re-run with the exact size its cursor reports
 *   "ef_rows"     [0]   decode: 0 = Elias-Fano rows when min(host workers, bitstreams of the call) >= 10 (PCIe is the bottleneck),
 *                       uint16 rows otherwise (the sequential host decoders are); 1 = always, 2 = never
 *   "ef_min"      [33]  decode: rows with at least this many entries are Elias-Fano coded (>= 14, the format's floor)
 *   "gpu_decode"  [0]   decode: checkpointed bitstreams (fgmm_ckpt) are decoded ON THE GPU, a workgroup per segment (no decode-side
 *                       tables at all); a bitstream with a segment the kernel does not settle goes through the table path.  0 = when
 *                       the call has enough segments for the GPU to be the faster decoder (estimated with rates measured on MI355X +
 *                       EPYC 9575F: on another host set 1 or 2), 1 = whenever a bitstream carries valid notes, 2 = never
 *   "ckpt_decode" [0]   decode, table path: checkpointed bitstreams are decoded in segments on all host workers: 0 = when the call
 *                       has fewer bitstreams than workers, 1 = always, 2 = never (the notes are ignored)
 *   "spin_lat"    [400000] decode: calls of at most this many latents wait on polled events instead of sleeping ones (-1: never)
 *   "enc_vec" / "enc_linear"  A/B switches of the encode-side kernel's load width and grid (0 / 1: the defaults)
 *   "trace"       [0]   1: phase timestamps of every batched call on stderr, 2: + per-bitstream job timeline */
int fgmm_ctx_set_option(fgmm_ctx *ctx, const char *name, int64_t value);
int fgmm_ctx_get_option(fgmm_ctx *ctx, const char *name, int64_t *value_out);
/* Releases the context's grown buffers (device workspace and staging, pinned host ranges); they grow again on demand. */
int fgmm_ctx_trim(fgmm_ctx *ctx);

/* Measurement aid (bench.py): when enabled, timing HIP events bracket the table kernels ON THE STREAM THEY ARE
 * LAUNCHED ON; fgmm_ctx_kernel_ms returns the duration of the most recent launch(es) of
 * which = 0: symtab kernel (encode-side CDF), 1: decode-side table kernels of the last call (all launches, first to
 * last), 2: quant_stats kernel, 3: unused (0). */
int fgmm_ctx_set_profiling(fgmm_ctx *ctx, int enable);
/* Counters of the most recent batched call: which = 0 encode tables copied D2H (bytes), 1 decode headers + block offsets
 * + rows copied D2H (bytes), 2 latents those decode tables describe, 3 edges the decode-side kernels evaluated, 4 bitstreams
 * the GPU's segment decoder decoded (checkpointed ones), 5 bitstreams it handed back to the table path. */
int fgmm_ctx_stat(fgmm_ctx *ctx, int which, uint64_t *out);
int fgmm_ctx_kernel_ms(fgmm_ctx *ctx, int which, float *ms_out);
/* The call log: phase marks of the context's most recent batched calls (at most 64 are kept), always recorded - a handful of
 * clock reads per call.  What a caller needs to tell WHICH part of a slow call was slow: the GPU and the bus (marks 1..3), the host
 * workers (mark 4 against mark 3, busy / wait), or the calling thread.  Times in milliseconds.
 *   kind 0 = batched encode: ms[0] kernels and table copies enqueued, [1] kernels done and side information on the host, [2] host
 *            jobs handed out, [3] last table (segment) seen landed by an encoder, [4] last encoder done, [5] call end
 *   kind 1 = batched decode, table path: ms[0] planned and buffers ensured, [1] first table copy queued, [2] last table copy queued,
 *            [3] last table piece seen landed by a decoder, [4] last decoder done, [5] call end (y_hat complete)
 *   kind 2 = batched decode on the GPU (checkpointed bitstreams): ms[0..2] enqueued, [3..4] segments decoded, [5] call end
 *   worker_busy_ms / worker_wait_ms: summed over the host jobs of the call - coding, and waiting for a table copy to land */
typedef struct {
  int32_t kind, count;   /* count: bitstreams of the call */
  double t_begin_ms;     /* steady clock, since the context was created */
  double ms[6];          /* since t_begin_ms */
  double worker_busy_ms, worker_wait_ms;
  double head_ms[3];     /* kind 1, the time before ms[1] in detail: [0] descriptors built, [1] first launches enqueued and the host
                            workers started, [2] the first launch's size seen on the host (its copy is queued next); else 0 */
} fgmm_call_marks;
/* out[0 .. *n_out) = the most recent min(cap, 64, calls so far) calls, oldest first */
int fgmm_ctx_call_log(fgmm_ctx *ctx, fgmm_call_marks *out, int cap, int *n_out);

/* ------------------------------------------------------------------------------------------------------------
 * 1. The reference's native boundary (compressai.ans), same argument meaning and order.
 * ---------------------------------------------------------------------------------------------------------- */

/* RansEncoder.encode_with_indexes_gmm(symbols, scales, means, weights, max_value) -> bytes
 * symbols: int32[n] contiguous.  scales/means/weights: (n, 4) float32 at [i*stride_n + k*stride_k].
 * max_value is accepted and ignored, as in the reference (rans_interface.cpp:462).
 * *out is malloc'ed by the library (fgmm_free); empty input yields the 8-byte flushed state. */
int fgmm_encode_with_indexes_gmm(fgmm_ctx *ctx, const int32_t *symbols, const float *scales, const float *means,
                                 const float *weights, int64_t n, int64_t stride_n, int64_t stride_k, int K,
                                 int mode, int memspace, int32_t max_value, uint8_t **out, size_t *out_len);

/* RansDecoder.decode_with_indexes_gmm(encoded, scales, means, weights, max_bs_value) -> int32[n]
 * out_symbols: HOST int32[n].  Yields exactly what the reference's float bisection yields, including on
 * non-monotone tables and on its pmf==0 fallback (rans_interface.cpp:865-875). */
int fgmm_decode_with_indexes_gmm(fgmm_ctx *ctx, const uint8_t *encoded, size_t encoded_len, const float *scales,
                                 const float *means, const float *weights, int64_t n, int64_t stride_n,
                                 int64_t stride_k, int K, int mode, int memspace, int32_t max_bs_value,
                                 int32_t *out_symbols);

/* ------------------------------------------------------------------------------------------------------------
 * 2. Entropy-model level, fused on the GPU: GaussianMixtureConditional.compress / .decompress for B = 1.
 *    All tensor pointers are DEVICE pointers in the latent codec's layout:
 *      y [M, h*w] float32;   scales/means/weights [K, M, h*w] via (stride_k, stride_c), position stride 1.
 *    `stream` is the hipStream_t the caller's producer kernels were enqueued on (NULL = default stream);
 *    the library orders its own work after it and returns with all outputs complete.
 * ---------------------------------------------------------------------------------------------------------- */

typedef enum { FGMM_F32 = 0, FGMM_F16 = 1, FGMM_BF16 = 2 } fgmm_dtype;

typedef struct {
  const void *scales, *means, *weights;  /* device; float32, IEEE float16 or bfloat16 planes, see dtype */
  int64_t stride_k, stride_c;            /* elements */
  int32_t dtype;                         /* fgmm_dtype.  FGMM_F16 (BASELINE configs[4]): each value is widened to
                                            float32 exactly on load, then the float32 path runs unchanged — the result
                                            is that of the reference fed the widened values (the reference itself
                                            rejects half tensors: accessor<float,2>, rans_interface.cpp:478-480).
                                            FGMM_BF16 (FGMM_HAS_BF16): a bfloat16 value is widened exactly to binary32 — its 16 bits
                                            become the upper half and the lower half is zero; NaN payloads, infinities, signed zeros
                                            and subnormals are kept — and the float32 path then runs unchanged.  The result of EVERY
                                            call is that of the same call on float32 planes holding the widened values: bitstream
                                            bytes, abs_max, zero bitmap, y_q / y_hat, checkpoint notes, and every sum, flag, count,
                                            curve point, lambda and y_rdo of sections 3b - 3f.
                                            One dtype per batch.  y, yq_out, y_hat, chan_w, pos_w and the parameter head (fgmm_head_*,
                                            fuse_head) stay float32 whatever the planes are, and so does the raw (n, 4) boundary of
                                            section 1.
                                            PRECONDITION of both two-byte forms: AFTER widening, sum_k pi_k must not exceed 1, or the
                                            reference's algorithm desynchronises (tests: test_fp16_parameter_planes).  bfloat16 has 8
                                            significant bits, and weights rounded to nearest violate this often: pass logits
                                            (FGMM_PARAMS_LOGITS — the softmax runs in binary32 in the kernel) or weights rounded
                                            TOWARD ZERO */
  int32_t flags;                         /* FGMM_PARAMS_LOGITS: `weights` holds the parameter head's LOGITS; the kernels compute
                                            pi = softmax over K themselves (the pi plane is never
                                            written and read back), with one fixed binary32 sequence shared by the encode- and
                                            the decode-side kernel — streams coded this way decode this way, on any device;
                                            they differ from streams coded from torch.softmax's pi in the last bit of pi */
} fgmm_params;
#define FGMM_PARAMS_LOGITS 1

/* compress(y, scales, means, weights) -> ((bytes, abs_max, zero_bitmap), y_quantized)
 *   yq_out        device float32[M*hw]  = round(y) (round-half-even)                    entropy_models.py:839
 *   abs_max_out   max(int|max y|, int|min y|) + 1, floored at 1                         entropy_models.py:834-837
 *   zero_bitmap   HOST int64[M]: 1 where the channel has any non-zero quantised latent  entropy_models.py:840-842
 *   scales are clamped to [0.11, 256] when clamp_scales != 0                            entropy_models.py:817
 *   symbols are coded in (non-zero channel, h, w) order                                 entropy_models.py:844-845 */
int fgmm_gmc_compress(fgmm_ctx *ctx, void *stream, const float *y, const fgmm_params *params, int M, int K,
                      int64_t hw, int mode, int clamp_scales, float *yq_out, int32_t *abs_max_out,
                      int64_t *zero_bitmap_out, uint8_t **out, size_t *out_len);

/* decompress(strings, abs_max, zero_bitmap, scales, means, weights) -> y_hat
 *   y_hat_out     device float32[M*hw]: decoded symbols at the non-zero channels, 0 elsewhere (:903-908) */
int fgmm_gmc_decompress(fgmm_ctx *ctx, void *stream, const uint8_t *encoded, size_t encoded_len, int32_t abs_max,
                        const int64_t *zero_bitmap, const fgmm_params *params, int M, int K, int64_t hw, int mode,
                        int clamp_scales, float *y_hat_out);

/* Checkpoints: a SEEKABLE bitstream without touching the bitstream.  A rANS stream decodes sequentially - symbol i needs the
 * coder state symbol i-1 left - which makes ONE bitstream one host thread's work (1.1 - 1.5 ms for a Kodak half, 27 ms for
 * ELIC's largest group of a 4K image) however many threads idle.  The decoder's state before symbol i is the encoder's state
 * after it has encoded symbol i on its reversed walk, so the encoder can note (state, words the decoder has read by then)
 * every `stride` symbols, OUT OF BAND: `bytes` stays the reference's stream, byte for byte.  A decoder handed the notes
 * decodes the segments between them on as many host workers as it has; a stream without notes (the reference's own) decodes
 * sequentially as ever.  The notes are VERIFIED, never trusted: a segment must end exactly in the next note's state and
 * position - then, by induction from the stream's head, it did the sequential decoder's work; one mismatch and the whole
 * stream is decoded sequentially instead.  16 bytes per `stride` symbols (stride 4096: 0.3 % of a Kodak stream). */
typedef struct {
  uint64_t x;   /* coder state before decoding symbol (k + 1) * stride */
  uint64_t pos; /* 32-bit renormalisation words read by then (the stream's 8-byte head not counted) */
} fgmm_ckpt;

/* Batched forms: `count` independent streams (images / checkerboard halves) in one call.  Kernels for all
 * items are enqueued first on the context's HIP streams, tables come back by pinned async copies, and the host
 * worker threads run one rANS state machine per item.  Item i uses y[i], params[i], ... ; outputs as above. */
typedef struct {
  const float *y;          /* device [M*hw] (compress only) */
  fgmm_params params;
  int32_t M, K;
  int64_t hw;
  float *yq_out;           /* compress: device [M*hw];  decompress: y_hat device [M*hw] */
  int64_t *zero_bitmap;    /* HOST int64[M]: compress out / decompress in */
  int32_t abs_max;         /* compress out / decompress in */
  uint8_t *bytes;          /* compress: out (fgmm_free);  decompress: in */
  size_t bytes_len;
  int32_t status;          /* per-item fgmm_status */
  int32_t ckpt_stride;     /* compress in: note a checkpoint every this many symbols (a power of two >= 256; 0 = none).
                              decompress in: the stride `ckpt` was noted with (0 / ckpt NULL: sequential decode) */
  fgmm_ckpt *ckpt;         /* compress out (fgmm_free; NULL when none): (coded symbols - 1) / ckpt_stride entries;
                              decompress in */
  int64_t n_ckpt;          /* compress out / decompress in */
} fgmm_item;

/* A compress call that returns an error returns NO buffer (items[i].bytes / .ckpt are NULL, whatever items[i].status says): a binding
 * may raise on the status without releasing anything. */
int fgmm_gmc_compress_batch(fgmm_ctx *ctx, void *stream, fgmm_item *items, int count, int mode, int clamp_scales);
int fgmm_gmc_decompress_batch(fgmm_ctx *ctx, void *stream, fgmm_item *items, int count, int mode, int clamp_scales);

/* A sink: the bitstreams of a batched compress call written straight into storage of the caller's (a Python `bytes` object created
 * at its final size and filled by the flush - what rans_interface.cpp:557-585 does with its py::bytes - instead of a buffer of the
 * library's that the binding copies once more: 2.5 MB per Kodak batch, 0.1 ms of the calling thread).  When item i's bitstream is
 * complete and its size known, the library calls alloc(user, i, nbytes) - ONCE per item, ON THE CALLING THREAD (it serves the host
 * workers' requests while it waits for them: a binding may take its interpreter's lock in alloc without its workers queueing for
 * it) - and the worker that coded the bitstream copies the nbytes there; items[i].bytes is that address on return, the caller's to
 * keep: fgmm_free / fgmm_ctx_take_buffers must NOT be given it.  alloc returning NULL fails the call with FGMM_ERR_NOMEM.  A failed
 * call returns items[i].bytes == NULL as ever; what the sink had handed out by then stays the caller's to release.  Checkpoints
 * (items[i].ckpt) are returned as without a sink.  sink == NULL: the plain call. */
typedef struct {
  void *(*alloc)(void *user, int item, size_t nbytes);
  void *user;
} fgmm_sink;
int fgmm_gmc_compress_batch_to(fgmm_ctx *ctx, void *stream, fgmm_item *items, int count, int mode, int clamp_scales, const fgmm_sink *sink);

/* ------------------------------------------------------------------------------------------------------------
 * 2b. The parameter head's last layer, on the matrix cores.
 *    Replaces: the final 1x1 convolution of `entropy_parameters`, nn.Conv2d(c_in, 3*K*M, 1) (compressai/models/ckbd_gmm.py:115-121;
 *    c_in = 640, M = 192 there), the chunk(3, 1) into scales | means | weights and the softmax over K
 *    (compressai/latent_codecs/gaussian_mixture_conditional.py:183-202).
 *    out[o][p] = bias[o] + sum_k weight[o][k] * x[k][p], o = t * K*M + k * M + c (t: scales, means, logits), computed on
 *    v_mfma_f32_32x32x2_f32 in ONE fixed order - bit for bit, signs of zero, infinities and NaN included,
 *    acc = bias[o] (+0 without a bias); for k ascending: acc = fmaf(weight[o][k], x[k][p], acc)  -
 *    so that encoder and decoder derive identical parameters from identical weights on any ROCm / torch / MIOpen version (a
 *    BLAS's or MIOpen's summation order is not part of any contract; the reference silently relies on it being the same on both
 *    sides).  Streams coded from these parameters decode from these parameters.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct fgmm_head fgmm_head; /* a head's weights, packed for the kernel, on the context's device.  Immutable once created: a head
                                     * may be used from any context on its device, from several at the same time (what a call needs
                                     * beside the weights - the bf16x6 form's split features - is the calling context's) */
/* weight: device float32 [3*K*M, c_in] row-major (Conv2d.weight [3*K*M, c_in, 1, 1]); bias: device float32 [3*K*M] or NULL.
 * The weights are copied (packed) before the call returns. */
int fgmm_head_create(fgmm_ctx *ctx, void *stream, const float *weight, const float *bias, int M, int K, int c_in, fgmm_head **out);
/* ... with flags.  FGMM_HEAD_BF16X6: the same layer on the BF16 matrix cores with binary32 accuracy - weights and features split into
 * three bfloat16 parts each, six part products per product, accumulated in binary32 (fgmm_head16.hip), at a third of the matrix-pipe
 * cycles.  Bound, per output, with n16 = ceil(c_in / 16):
 *     |out - exact| <= R (sum_k |w x| + |b|) + 2^-133 sum_k (|w_k| + |x_k|) + 6 n16 2^-150,   R = 2^-23 (1 + 2^-6) + 6 n16 2^-24 (1 + 2^-7)
 * (the three dropped part products; the bfloat16 subnormal grid, where a third part is rounded; one binary32 rounding per matrix
 * step) - on data of order one the error is ~2e-7 sum |w x|.  Domain: finite operands with |v| < 0x1.FFp127 (whose first bfloat16
 * part is finite).  Weights outside it are refused here (FGMM_ERR_INVALID).  An item with a feature outside it is computed by the
 * exact form instead, bit for bit the fmaf chain above (IEEE infinities and NaN included).  Deterministic on gfx950 (the same inputs
 * give the same parameters on every launch, fused or not), but NOT the fmaf chain of the default form and not restatable bit for bit
 * on a CPU: encoder and decoder must both use it, on MI355X. */
#define FGMM_HEAD_BF16X6 1
int fgmm_head_create_ex(fgmm_ctx *ctx, void *stream, const float *weight, const float *bias, int M, int K, int c_in, int flags,
                        fgmm_head **out);
void fgmm_head_destroy(fgmm_head *head);
/* The parameters as tensors, for the decoder (and for anyone who wants them): item i reads x[i] = device float32 [c_in, hw[i]] and
 * writes out[i] = device float32 [3*K*M, hw[i]] - scales | means | LOGITS, each [K*M, hw] with channel k*M + c: three fgmm_params
 * planes with stride_k = M*hw, stride_c = hw, flags FGMM_PARAMS_LOGITS (the softmax over K and the sigma clamp run in the table
 * kernels).  Returns with the outputs complete. */
int fgmm_head_params_batch(fgmm_ctx *ctx, void *stream, const fgmm_head *head, const float *const *x, float *const *out,
                           const int64_t *hw, int count);
/* fgmm_gmc_compress_batch with the head FUSED into the encode-side CDF kernel: items[i].params is ignored, the twelve parameters of
 * a latent go from the MFMA accumulators into the table entry and never exist in HBM.  x[i]: device float32 [c_in, items[i].hw];
 * items[i].M must be the head's M.  The bitstreams are those of fgmm_gmc_compress_batch fed fgmm_head_params_batch's planes with
 * FGMM_PARAMS_LOGITS (same arithmetic, same bytes). */
int fgmm_gmc_compress_head_batch(fgmm_ctx *ctx, void *stream, fgmm_item *items, const float *const *x, int count,
                                 const fgmm_head *head, int mode, int clamp_scales);
/* ... with the bitstreams written into the caller's storage (fgmm_sink, section 2) */
int fgmm_gmc_compress_head_batch_to(fgmm_ctx *ctx, void *stream, fgmm_item *items, const float *const *x, int count,
                                    const fgmm_head *head, int mode, int clamp_scales, const fgmm_sink *sink);

/* ------------------------------------------------------------------------------------------------------------
 * 3. Building blocks ("same tables => same bytes" surfaces; also what the parity tests probe).
 *    SURVEY.md section 8(b) also lists fgmm_build_symtab_host / fgmm_build_cdftab_host: they do not exist on purpose —
 *    this library has no CPU implementation of the float work; the GPU builders below are the only ones.
 * ---------------------------------------------------------------------------------------------------------- */

/* GPU: float mixture-CDF pair per symbol, c1 = cdf(v - 0.5), c2 = cdf(v - 0.5 + 1.0)  (rans_interface.cpp:498-501).
 * v: device int32[n]; params (n,4) device via (stride_n, stride_k); c1/c2: device float32[n]. */
int fgmm_gmm_cdf_hip(fgmm_ctx *ctx, void *stream, const int32_t *v, const float *scales, const float *means,
                     const float *weights, int64_t n, int64_t stride_n, int64_t stride_k, int mode, float *c1,
                     float *c2);

/* GPU: the kernels' softmax over K on (n, 4) rows of logits -> weights (what FGMM_PARAMS_LOGITS computes in place of
 * torch.softmax, gaussian_mixture_conditional.py:198-202; within 2e-7 of it).  Both pointers device, row-major (n, 4). */
int fgmm_softmax4_hip(fgmm_ctx *ctx, void *stream, const float *logits, float *weights, int64_t n);

/* GPU: encode-side symbol table.  packed[i] = start | range << 16 with start = (uint16)(c1*65535),
 * range = (uint16)(end - start); range == 0 marks the reference's bypass escape (rans_interface.cpp:512-517) and
 * the low half then carries the low 16 bits of the symbol.  All pointers device. */
int fgmm_build_symtab_hip(fgmm_ctx *ctx, void *stream, const int32_t *symbols, const float *scales,
                          const float *means, const float *weights, int64_t n, int64_t stride_n, int64_t stride_k,
                          int mode, uint32_t *packed);

/* GPU: decode-side edge tables (format v5).  For latent i the reference's bisection can only ever look at
 *   F_i[v] = (uint16)(cdf_i(v - 0.5) * 65535),  v in [-max_bs, max_bs + 1]      (rans_interface.cpp:826-862).
 * The kernels find, exactly, the window outside which F_i is constant (evaluating F_i everywhere except where
 * every mixture component is provably saturated — fgmm_selftest_saturation) and store it:
 *   header of latent i, one of three forms (chosen per table from max_bs: FGMM_HDR_FORM(max_bs)):
 *     2 bytes  (a + max_bs) | cnt << 8, cnt in [1, 254]            when 2*max_bs + 2 <= 254
 *              cnt field 255: the row begins with a 4-byte header of the next form (non-monotone rows)
 *     4 bytes  int16 a | cnt << 16 (15 bits) | nonmono << 31        when max_bs <= FGMM_MAX_BS_H4
 *     8 bytes  int32 a ; cnt (31 bits) | nonmono << 31              any max_bs <= FGMM_MAX_BS
 *   row i  = F_i[a .. a+cnt), from the first non-zero edge to the start of the trailing constant run;
 *            F_i[v < a] = 0,   F_i[v >= a+cnt] = the row's last entry;  rows are 2-byte aligned:
 *     cnt < 14 or nonmono : uint16[cnt]                                                   (2*cnt bytes)
 *     cnt >= 14, monotone : Elias-Fano with l low bits, l = 12 for cnt <= 48, else 8, as ONE little-endian bit string
 *                           (bit b = bit (b & 7) of byte b >> 3) rounded up to 16 bits:
 *                             bits [0, HB), HB = cnt + (65536 >> l) : bit ((F_j >> l) + j) set for entry j
 *                             bits [LB + j*l, LB + (j+1)*l), LB = HB rounded up to 8 : the low l bits of entry j
 *     (FGMM_TAB_RAW_ROWS: every row in the first form; the batched decoder raises the threshold 14: "ef_min" option)
 *   `nonmono` is set when the row decreases somewhere.
 * fgmm_build_cdftab_hip (generic two-pass kernels, lane = latent, any max_bs <= FGMM_MAX_BS_H4 here): 4-byte headers, rows
 *   in LATENT ORDER with no stored offset (row i+1 starts where row i ends).  hdr: device uint32[n]; pool: device bytes;
 *   pool_used: device uint64[1] = bytes written.  pool_cap >= n * 2 * (2*max_bs + 2) always suffices; a smaller
 *   pool yields FGMM_ERR_NOMEM with *pool_used = the bytes needed.
 * fgmm_build_tab_hip (the single-pass kernel of the batched decode path: parameters staged in LDS, evaluation flattened
 *   over pairs of edges in packed fp32): headers in the form FGMM_HDR_FORM(max_bs) (device, n * form bytes); rows of each
 *   block of *tl_out consecutive latents are contiguous and start at rows + 4 * blk_off[block]  (blocks are placed by an
 *   atomic cursor: any order, each padded to 4 bytes); blk_off: device uint32[ceil(n / tl)], provide ceil(n / 16) entries; rows_used: device
 *   uint64[1].  FGMM_ERR_UNSUPPORTED when 2*max_bs + 2 does not fit the kernel's LDS budget (use the generic kernels),
 *   FGMM_ERR_NOMEM (with *rows_used = the bytes needed) when rows_cap is too small. */
#define FGMM_TAB_NO_PRUNE 1 /* flags: evaluate all of F_i instead of skipping its saturated tails (A/B testing) */
#define FGMM_TAB_CLAMP 2    /* flags: clamp sigma to [0.11, 256] first (the entropy-model path's kernel variant) */
#define FGMM_TAB_RAW_ROWS 4 /* flags: no Elias-Fano rows, every row as uint16 entries (35 % more bytes, 2-3x faster to search:
                               what the batched decoder chooses for calls with fewer bitstreams than host workers) */
#define FGMM_HDR_FORM(max_bs) ((2 * (int64_t)(max_bs) + 2 <= 254) ? 2 : ((max_bs) <= FGMM_MAX_BS_H4 ? 4 : 8))
int fgmm_build_cdftab_hip(fgmm_ctx *ctx, void *stream, const float *scales, const float *means,
                          const float *weights, int64_t n, int64_t stride_n, int64_t stride_k, int mode,
                          int32_t max_bs, int flags, uint32_t *hdr, uint8_t *pool, uint64_t pool_cap,
                          uint64_t *pool_used);
int fgmm_build_tab_hip(fgmm_ctx *ctx, void *stream, const float *scales, const float *means, const float *weights,
                       int64_t n, int64_t stride_n, int64_t stride_k, int mode, int32_t max_bs, int flags, void *hdr,
                       uint32_t *blk_off, uint8_t *rows, uint64_t rows_cap, uint64_t *rows_used, int32_t *tl_out);

/* GPU self-test: exhaustive scan (every binary32 beyond the thresholds) of the saturation lemmas that let the
 * table kernel skip the tails of F_i.  *n_bad_out = number of violating inputs (must be 0). */
int fgmm_selftest_saturation(fgmm_ctx *ctx, int mode, uint64_t *n_bad_out);

/* GPU self-test of the hand-expanded correctly-rounded cores (fgmm_math.h) against the compiler's IEEE '/' and
 * sqrtf: which = 0 sqrt (every binary32 in [0,2]), 1 division by a clamped sigma (n hashed pairs from `seed`),
 * 2 reciprocal of d >= 1 (every binary32 in [1,+inf]); which = 3, 4, 5: the kernels' slimmed Phi evaluation against
 * the literal one (mode which - 3) for every binary32 |z| < 2^48; which = 6: the Markstein-step sqrt of the Polya
 * path for every binary32 in {0} U [2^-24, 1].  *n_bad_out must come back 0. */
int fgmm_selftest_fastmath(fgmm_ctx *ctx, int which, uint64_t n, uint64_t seed, uint64_t *n_bad_out);

/* Host, integer only: symbol table (+ raw symbols, needed only where range == 0 and abs(symbol) >= 32768)
 * -> bitstream.  BufferedRansEncoder::flush semantics (rans_interface.cpp:557-585). */
int fgmm_rans_encode_symtab(const uint32_t *packed, const int32_t *symbols_or_null, int64_t n, uint8_t **out,
                            size_t *out_len);
/* Two independent tables -> two bitstreams, coded by the calling thread in turn symbol by symbol (the batched paths use
 * this when there are more bitstreams than workers: two dependency chains share a core).  out[k] is byte for byte what
 * fgmm_rans_encode_symtab returns for table k. */
int fgmm_rans_encode_symtab2(const uint32_t *packed0, const int32_t *symbols0_or_null, int64_t n0, const uint32_t *packed1,
                             const int32_t *symbols1_or_null, int64_t n1, uint8_t **out0, size_t *out0_len, uint8_t **out1,
                             size_t *out1_len);
/* The same for `ways` (1..4) tables given as arrays: out[k] / out_len[k] receive bitstream k.  On an error no buffer is
 * returned. */
int fgmm_rans_encode_symtab_n(int ways, const uint32_t *const *packed, const int32_t *const *symbols_or_null, const int64_t *n,
                              uint8_t **out, size_t *out_len);

/* ... noting checkpoints every `stride` symbols (a power of two; see fgmm_ckpt): ckpt_out[fgmm_ckpt_count(n, stride)].  The
 * bitstream is the one fgmm_rans_encode_symtab returns. */
int64_t fgmm_ckpt_count(int64_t n, int64_t stride); /* (n - 1) / stride, 0 for stride <= 0 */
int fgmm_rans_encode_symtab_ckpt(const uint32_t *packed, const int32_t *symbols_or_null, int64_t n, int64_t stride, uint8_t **out,
                                 size_t *out_len, fgmm_ckpt *ckpt_out);

/* The same from a table that lies in `n_seg` (1..4) SEGMENTS of `seg_len` entries (the last may be shorter): seg[s] holds the entries
 * [s * seg_len, (s + 1) * seg_len).  What the batched encoder does with the tables of a large call: they cross PCIe in segments, LAST
 * SEGMENT FIRST (rANS encodes backwards), and an encoder follows the landing.  The bitstream (and the checkpoints, stride > 0) are
 * byte for byte those of the one-piece forms. */
int fgmm_rans_encode_symtab_segs(const uint32_t *const *seg, int n_seg, int64_t seg_len, const int32_t *symbols_or_null, int64_t n,
                                 int64_t stride, uint8_t **out, size_t *out_len, fgmm_ckpt *ckpt_out);

/* Host, integer only: edge tables (4-byte headers, rows sequential in latent order, as fgmm_build_cdftab_hip lays them
 * out) -> symbols; the reference's bisection with every float evaluation replaced by a look-up in F_i.  pool_len bounds
 * every row access: a malformed table (cnt = 0, a row past the pool, an inconsistent Elias-Fano row) yields
 * FGMM_ERR_INVALID, never an out-of-bounds read; up to 32 bytes past a row may be read, so keep 32 bytes of slack
 * after the last row inside pool_len. */
int fgmm_rans_decode_cdftab(const uint8_t *encoded, size_t encoded_len, const uint32_t *hdr, const uint8_t *pool,
                            uint64_t pool_len, int64_t n, int32_t max_bs, int flags, int32_t *out_symbols);
/* The same for any header form and block-placed rows (fgmm_build_tab_hip); blk_off may be NULL (sequential rows).
 * flags: FGMM_TAB_RAW_ROWS as the table was built. */
int fgmm_rans_decode_tab(const uint8_t *encoded, size_t encoded_len, const void *hdr, int hdr_form, const uint32_t *blk_off,
                         int32_t tl, const uint8_t *rows, uint64_t rows_len, int64_t n, int32_t max_bs, int flags,
                         int32_t *out_symbols);
/* The same from a checkpointed stream (block-placed rows: blk_off != NULL), segment by segment on the calling thread - the
 * batched decoder runs the segments on its workers.  Every segment is verified against the next checkpoint; the first mismatch
 * (wrong or hostile notes) makes the whole stream a sequential decode: the symbols are fgmm_rans_decode_tab's in every case.
 * *verified_out (may be NULL): 1 when every checkpoint held. */
int fgmm_rans_decode_tab_ckpt(const uint8_t *encoded, size_t encoded_len, const void *hdr, int hdr_form, const uint32_t *blk_off,
                              int32_t tl, const uint8_t *rows, uint64_t rows_len, int64_t n, int32_t max_bs, int flags,
                              const fgmm_ckpt *ckpt, int64_t n_ckpt, int64_t stride, int32_t *out_symbols, int32_t *verified_out);

/* ------------------------------------------------------------------------------------------------------------
 * 3b. The coded size WITHOUT running the coder (rate control, byte budgets, bpp, per-latent rate maps).
 *    The stream's length is a closed form of the encode-side table.  With 16-bit frequencies
 *      - a coded symbol of range r costs 16 - log2 r bits;
 *      - a bypass symbol v costs 16 + 4 * (1 + nib(v)) bits: the {65535, 1} sentinel, one count nibble, and nib(v) nibbles -
 *        those of v's uint32 bit pattern up to its leading one: 0 for v = 0, 8 for every negative v (rans_interface.cpp:524-551).
 *    The coder's state starts at 2^31, ends in [2^31, 2^63) and is flushed as 8 bytes; Rans64EncPut departs from x * 2^16 / r
 *    by a relative 2^-15 per symbol at worst (about 2^-31 in practice: the state is rarely at its floor).  So with B = sum of the
 *    costs, 8 * len - B lies in (32, 64], and len being a multiple of 4,
 *        len = 4 * floor((B + 64) / 32)                                       (the empty stream: 8 bytes)
 *    - exact unless B lies within the accumulated departure of a multiple of 32, then 4 bytes off.
 *    Costs are fixed point in units of 2^-FGMM_RATE_Q bit: (16 << 24) - L[r] with L[r] = 2^24 * log2 r rounded to nearest (exact
 *    at powers of two), one table built by the host and shared with the kernels, so host and GPU agree bit for bit on every
 *    symbol; sums are uint64 - independent of order, identical from run to run.
 * ---------------------------------------------------------------------------------------------------------- */
#define FGMM_RATE_Q 24
/* Host, integer only: table -> cost, the counterpart of fgmm_rans_encode_symtab (table -> bytes).  cost_q_or_null: uint32[n], the
 * cost of every entry; *bits_q_out their sum; *n_bypass_out the entries with range == 0 (any out-pointer may be NULL).  A bypass
 * entry is priced by symbols_or_null[i] - or, without symbols, by what fgmm_rans_encode_symtab would code then: the entry's low 16
 * bits sign-extended (right whenever abs(symbol) < 32768). */
int fgmm_symtab_bits(const uint32_t *packed, const int32_t *symbols_or_null, int64_t n, uint32_t *cost_q_or_null, uint64_t *bits_q_out,
                     int64_t *n_bypass_out);
/* bytes of the flushed stream whose symbols cost bits_q: 4 * ((bits_q + (64 << 24)) >> 29) */
uint64_t fgmm_rate_stream_bytes(uint64_t bits_q);
/* GPU: the same from a table in device memory - with fgmm_build_symtab_hip a per-latent rate map for the (n, 4) layout.  All
 * pointers device; cost_q_or_null uint32[n]; bits_q_dev / n_bypass_dev uint64[1] each (overwritten; either may be NULL).  Every
 * value equals fgmm_symtab_bits'. */
int fgmm_symtab_bits_hip(fgmm_ctx *ctx, void *stream, const uint32_t *packed, const int32_t *symbols_or_null, int64_t n,
                         uint32_t *cost_q_or_null, uint64_t *bits_q_dev, uint64_t *n_bypass_dev);

/* The fused form at the entropy-model level: what fgmm_gmc_compress_batch WOULD return for these items, priced by one kernel that
 * does the encode-side CDF kernel's arithmetic on the same inputs (same addressing, same Phi, same softmax over K with
 * FGMM_PARAMS_LOGITS, float32, float16 or bfloat16 planes) and ends in a reduction instead of a table: no table, no table traffic over
 * PCIe, no host coder.  Per item:
 *   abs_max, zero_bitmap   as fgmm_gmc_compress_batch returns them
 *   n_symbols              symbols it would code (coded channels * hw);  n_bypass: those that take the bypass escape
 *   bits_q                 their exact cost, units of 2^-FGMM_RATE_Q bit;  chan_bits_q[c]: channel c's part (0: not coded)
 *   bytes_pred             fgmm_rate_stream_bytes of bits_q: the length of the bitstream (see above for when it is 4 off)
 *   bits_map               cost_q * 2^-24 as float32 per latent, 0 in the channels that are not coded
 * Arguments are validated as by the compress call (K != 4, null tensors, negative sizes, mixed dtypes: FGMM_ERR_INVALID; an
 * item with M * hw == 0 is the empty stream, 8 bytes).  Returns with every output complete. */
typedef struct {
  const float *y;          /* device [M*hw] */
  fgmm_params params;
  int32_t M, K;
  int64_t hw;
  int64_t *zero_bitmap;    /* HOST int64[M] out, may be NULL */
  uint64_t *chan_bits_q;   /* HOST uint64[M] out, may be NULL */
  float *bits_map;         /* DEVICE float32[M*hw] out, may be NULL */
  int32_t abs_max, status; /* out */
  int64_t n_symbols, n_bypass; /* out */
  uint64_t bits_q, bytes_pred; /* out */
} fgmm_rate_item;
int fgmm_gmc_estimate_batch(fgmm_ctx *ctx, void *stream, fgmm_rate_item *items, int count, int mode, int clamp_scales);

/* ------------------------------------------------------------------------------------------------------------
 * 3c. Rate-distortion optimised quantisation (RDOQ): spend the exact cost function of 3b to encode better.  For every latent of a
 *    channel the compress call would code for y, keep round(y) or move ONE step to a neighbour, whichever minimises
 *    (y - v)^2 + lambda * bits(v), bits being the coder's own cost of v under that latent's mixture.  A pure encoder-side choice:
 *    y_rdo goes through the unchanged compress call, the bitstream is the reference's format, any reference decoder reads it;
 *    lambda = 0 returns round(y).  The decision, exactly (restatable on a CPU; tests/rdoq_ref.py does):
 *      rounding      v0 = rintf(y) (round half to even), as everywhere in the library
 *      coded         the channels fgmm_gmc_compress_batch would code for y: any round(y) != 0.  The other channels are written as
 *                    round(y) - zeros - and never reconsidered
 *      candidates    v0 - 1, v0, v0 + 1 when y is finite and |v0| <= 2^20; only v0 otherwise (within the bound float(v0 +- 1) - 0.5f
 *                    and float(v0) - 0.5f + 1.0f are the same binary32 numbers, so the four edges v0 - 1.5 .. v0 + 1.5 give all three
 *                    entries; beyond it the encoder's own two roundings differ and the latent is left alone)
 *      entry, cost   each candidate's table entry is what the encode-side kernel yields for that symbol (same Phi, clamp, softmax
 *                    over K, bypass rule); cost_q is fgmm_symtab_bits' cost of that entry and symbol, a bypass candidate being
 *                    priced by the symbol's own nibbles
 *      objective     J(v) = d * d + lam_q * (double)cost_q(v) with d = (double)y - (double)v and lam_q = lambda * 2^-24: every
 *                    operation one IEEE binary64 operation, no contraction
 *      choice        start from v0; take v0 - 1 if its J is strictly smaller; then v0 + 1 if its J is strictly smaller than the best
 *                    so far.  Ties keep the earlier candidate
 *    Per item: y_rdo (integer-valued floats, +0.0 for zero, NaN / +-inf latents kept as they are; its range may not overlap
 *    y's: FGMM_ERR_INVALID), n_changed (latents
 *    whose symbol is not round(y)), bits_q_before / bits_q_after (uint64 sums of cost_q of v0 / of the chosen symbol over the channels
 *    coded for y), chan_bits_q_after (per channel), abs_max and zero_bitmap OF y_rdo - what compressing y_rdo returns.  Sums are
 *    integer, the same bits on every run.  lambda must be finite and >= 0 (else FGMM_ERR_INVALID); otherwise arguments are validated
 *    as by the estimate call; an item with M * hw == 0 is a no-op with zero sums.  Returns with every output complete.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct {
  const float *y;          /* device [M*hw] */
  fgmm_params params;
  int32_t M, K;
  int64_t hw;
  float *y_rdo;            /* DEVICE float32[M*hw] out */
  int64_t *zero_bitmap;    /* HOST int64[M] out, may be NULL */
  uint64_t *chan_bits_q_after; /* HOST uint64[M] out, may be NULL */
  int32_t abs_max, status; /* out */
  int64_t n_changed;       /* out */
  uint64_t bits_q_before, bits_q_after; /* out */
} fgmm_rdoq_item;
int fgmm_gmc_rdoq_batch(fgmm_ctx *ctx, void *stream, fgmm_rdoq_item *items, int count, int mode, int clamp_scales, double lambda);

/* ------------------------------------------------------------------------------------------------------------
 * 3d. The rate-distortion curve, and quantisation to a BYTE BUDGET: what turns 3c into rate control.  A caller with a byte target does
 *    not know lambda; one kernel pass prices every latent once and evaluates 3c's decision at up to FGMM_RDCURVE_MAX lambdas, so a
 *    stretch of the curve costs one pass over y and the planes instead of one fgmm_gmc_rdoq_batch call per lambda tried.
 *
 *    THE CURVE.  Everything about one latent is 3c's: rounding, the channels coded (those of y), the candidates and the
 *    |v0| <= 2^20 / non-finite rule, the entries, cost_q, J(v) in binary64 with lam_q = lambda * 2^-24, the strict-less choice in
 *    the order v0, v0 - 1, v0 + 1.  At lambda_j the curve is the sum, over the latents of the channels coded for y, of what 3c
 *    decides at lambda_j.  Per item:
 *      bits_q_before     uint64 sum of cost_q(v0), once
 *      bits_q_after[j]   uint64 sum of cost_q of the choice - fgmm_gmc_rdoq_batch's bits_q_after at lambda_j
 *      n_changed[j]      latents whose choice is not v0 - its n_changed
 *      ddist_q[j]        the distortion the moves add over round(y), as an integer so that it has no order: a moved latent
 *                        contributes llrint(inc * 2^32) (round half to even) with inc = d * d - d0 * d0, d and d0 the binary64
 *                        distances of 3c to the choice and to v0: two binary64 multiplies and one subtract, no contraction.  Never
 *                        negative (v0 is the nearest integer and the rounding of the squares is monotone).  An unmoved latent
 *                        contributes 0.  The uint64 sum, in units of 2^-32 of a squared quantisation step
 *      n_symbols         symbols coded for y (coded channels * hw)
 *    At lambda_j = 0 the three are bits_q_before, 0 and 0.  Entries j >= n_lambda are left untouched.  n_lambda must lie in
 *    1 .. FGMM_RDCURVE_MAX and every lambda_j be finite and >= 0 (else FGMM_ERR_INVALID); they may come in any order and repeat.
 *    Items are validated as by the estimate call; an item with M * hw == 0 has zero sums.  All outputs HOST, integer, the same bits on
 *    every run.
 *
 *    THE BUDGET SEARCH - fixed here, restated by tests/rdcurve_ref.py.  A GROUP is a set of items that share one lambda (group ==
 *    NULL: every item its own group, n_groups == count).  f(lambda) = sum over the group's items of
 *    fgmm_rate_stream_bytes(bits_q_after of the item at lambda) - an item with M * hw == 0 counts 8 bytes.  f is non-increasing in
 *    exact arithmetic, but J is rounded, so the search does not rely on that at the last ulp: it takes the FIRST FEASIBLE POINT OF
 *    EACH GRID, which needs no monotonicity.  Every host operation below is one binary64 operation.
 *      round 0     the grid lambda_0 = 0, lambda_j = lambda_max * 2^(j - 15) for j = 1 .. 15 (the last point is lambda_max itself).
 *                  j* = the first j with f(lambda_j) <= budget.  None: the result is lambda_max with status FGMM_BUDGET_UNMET
 *                  (not an error: y_rdo at lambda_max is still returned).  j* = 0: the result is lambda = 0, round(y) already
 *                  fits.  Otherwise lo = lambda_{j* - 1}, hi = lambda_{j*}
 *      refinement  `refine` rounds (0 .. 8).  A round whose lo == hi does not run: the search stops.  Its grid is
 *                  lo + (hi - lo) * (double)k / 16.0 for k = 1 .. 15 (subtract, multiply, divide, add), and hi itself as the 16th
 *                  point, taken as given, not recomputed.  hi is thereby evaluated again: if it is no longer feasible, through
 *                  any cause, lo and hi stay what they were and the search stops.  Otherwise the first feasible point k* becomes
 *                  hi, and lo the point before it (the old lo for k* = 1)
 *      result      lambda* = hi; then 3c at lambda* - every item of the group gets exactly fgmm_gmc_rdoq_batch's outputs at
 *                  lambda* - with lambda*, bytes_pred = f(lambda*) and the number of curve passes the group took part in
 *                  (1 + the refinement rounds run)
 *    lambda_max must be finite and > 0, refine in 0 .. 8, group ids in 0 .. n_groups - 1 and no group empty (else FGMM_ERR_INVALID).
 *    The front half (census, descriptors) is taken once per call; a pass launches only rdcurve_kernel over the items whose group
 *    is still searching, every group on its own grid, and reads back a few KB of sums.
 *    Caveats.  The budget is on bytes_pred: 3b says when a real stream is 4 bytes longer.  A channel that RDOQ empties is no longer
 *    coded at all, so the real size can only be smaller than f(lambda*) on that account.  With channel skipping on (section 3f) this
 *    second caveat no longer applies: an emptied channel is a skipped one and counts nothing in f.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct {
  const float *y;          /* device [M*hw] */
  fgmm_params params;
  int32_t M, K;
  int64_t hw;
  uint64_t bits_q_before;                    /* out */
  uint64_t bits_q_after[FGMM_RDCURVE_MAX];   /* out */
  uint64_t n_changed[FGMM_RDCURVE_MAX];      /* out */
  uint64_t ddist_q[FGMM_RDCURVE_MAX];        /* out */
  int64_t n_symbols;                         /* out */
  int32_t status, pad_;                      /* out */
} fgmm_rdcurve_item;
int fgmm_gmc_rdcurve_batch(fgmm_ctx *ctx, void *stream, fgmm_rdcurve_item *items, int count, int mode, int clamp_scales,
                           const double *lambdas, int n_lambda);
typedef struct {
  double lambda;           /* lambda* of the group */
  uint64_t bytes_pred;     /* f(lambda*) */
  int32_t passes;          /* curve passes the group took part in */
  int32_t status;          /* FGMM_OK, or FGMM_BUDGET_UNMET */
} fgmm_budget_result;
int fgmm_gmc_rdoq_budget_batch(fgmm_ctx *ctx, void *stream, fgmm_rdoq_item *items, int count, int mode, int clamp_scales,
                               const int32_t *group_or_null, int n_groups, const uint64_t *budget_bytes, double lambda_max, int refine,
                               fgmm_budget_result *results /* per group */);

/* ------------------------------------------------------------------------------------------------------------
 * 3e. WEIGHTED distortion for 3c and 3d: a per-channel gain (the synthesis transform does not treat channels alike) and a spatial
 *    importance map (region of interest, perceptual masking), applied where the decision is made.  An item may carry two optional
 *    factor arrays, both DEVICE float32: chan_w[M] and pos_w[hw] (fgmm_rdo_weights; a NULL array means every factor is 1).  The
 *    rule, exactly (restatable on a CPU; tests/rdo_weights_ref.py does), for the latent at channel c, position p:
 *      weight        wt = (double)chan_w[c] * (double)pos_w[p]: ONE binary64 multiply.  It is exact - two 24-bit significands fit 53
 *                    bits - so the order of evaluation cannot matter
 *      objective     J(v) = wt * (d * d) + lam_q * (double)cost_q(v): three multiplies and one add, each a single IEEE binary64
 *                    operation, no contraction.  d, lam_q, the candidates, the |v0| <= 2^20 / non-finite rule, the strict-less
 *                    choice in the order v0, v0 - 1, v0 + 1 and the channels coded are 3c's, unchanged
 *      the curve     ddist_q[j] is the WEIGHTED added distortion: a moved latent contributes llrint((wt * inc) * 2^32) (round half
 *                    to even) with inc = d * d - d0 * d0 as in 3d.  bits_q_after and n_changed sum the weighted decisions
 *      the budget    the search of 3d - grids, first feasible point, refine - is untouched; the decisions it sums are the weighted
 *                    ones, in the curve passes and in the final 3c step alike
 *    With wt == 1.0 both expressions are the unweighted ones bit for bit: the _w calls with w == NULL, with {NULL, NULL} entries, or
 *    with arrays of ones return exactly what fgmm_gmc_rdoq_batch / fgmm_gmc_rdcurve_batch / fgmm_gmc_rdoq_budget_batch return -
 *    which ARE the _w forms with w == NULL.
 *    Domain.  Every factor must be finite and lie in [0, FGMM_RDO_W_MAX] (256); -0.0 counts as 0.  wt is then <= 2^16 and, a move
 *    being one step (|inc| <= 2), a latent's contribution to ddist_q at most 2^49.  The uint64 sum wraps only when the true sum of
 *    wt * inc over an item's moved latents reaches 2^32 squared steps: not below 2^15 moved latents of the largest weight, and never
 *    with wt <= 1 and fewer than 2^31 moved latents.  A zero weight is legal: that latent takes the cheapest of its three
 *    candidates, ties to the earlier.  A factor outside the domain - anywhere in either array, whether its channel is coded or
 *    not - fails the call with FGMM_ERR_INVALID, fgmm_last_error() naming the item; every item's status is the error and y_rdo is
 *    unspecified.  The check runs on the device beside the census and costs no extra synchronisation.
 *    w is an array of `count` entries (entry i belongs to item i) or NULL; everything else is validated as by the unweighted call.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct {
  const float *chan_w;     /* device float32 [M]  or NULL */
  const float *pos_w;      /* device float32 [hw] or NULL */
} fgmm_rdo_weights;
int fgmm_gmc_rdoq_batch_w(fgmm_ctx *ctx, void *stream, fgmm_rdoq_item *items, int count, int mode, int clamp_scales, double lambda,
                          const fgmm_rdo_weights *w /* [count] or NULL */);
int fgmm_gmc_rdcurve_batch_w(fgmm_ctx *ctx, void *stream, fgmm_rdcurve_item *items, int count, int mode, int clamp_scales,
                             const double *lambdas, int n_lambda, const fgmm_rdo_weights *w /* [count] or NULL */);
int fgmm_gmc_rdoq_budget_batch_w(fgmm_ctx *ctx, void *stream, fgmm_rdoq_item *items, int count, int mode, int clamp_scales,
                                 const int32_t *group_or_null, int n_groups, const uint64_t *budget_bytes, double lambda_max, int refine,
                                 fgmm_budget_result *results /* per group */, const fgmm_rdo_weights *w /* [count] or NULL */);

/* ------------------------------------------------------------------------------------------------------------
 * 3f. CHANNEL SKIPPING for 3c - 3e: the format's second lever.  A channel whose symbols are all zero is not coded at all - one bit
 *    of zero_bitmap, nothing in the stream - and no sequence of one-step decisions finds that trade, because it pays only when the
 *    whole channel goes.  The _s calls decide it per channel, after the per-latent decisions; the decode side is untouched.
 *    Everything about a single latent is 3c / 3e's, unchanged.  The rule, exactly (restatable on a CPU; tests/rdo_skip_ref.py does),
 *    per channel c that the compress call would code for y, at a given lambda:
 *      inelig(c)   some latent of the channel is not finite, or has |v0| > FGMM_SKIP_VMAX (15), or the item's hw > 2^24.  Such a
 *                  channel is never skipped
 *      nz0(c)      latents with v0 != 0 (at least 1: the channel is coded)
 *      A(c)        the uint64 sum of cost_q of the 3c / 3e choices - chan_bits_q_after as the _w call returns it
 *      nzA(c)      latents whose choice is not 0
 *      Dk(c)       the uint64 sum over moved latents of llrint((wt * inc) * 2^32) - 3d / 3e's ddist_q term, per channel
 *      Dz(c)       the uint64 sum, over latents with v0 != 0, of llrint((wt * incz) * 2^16) (round half to even) with
 *                  incz = dz * dz - d0 * d0, dz = (double)y, d0 = (double)y - (double)v0: two multiplies and one subtract, no
 *                  contraction; wt is 3e's exact product, 1.0 without weights.  The unit is 2^-16 on purpose: with |v0| <= 15,
 *                  wt <= 2^16 and hw <= 2^24 the sum cannot wrap.  incz >= 0, because |y| >= 0.5 >= |d0| whenever v0 != 0
 *      Jk, Jz      Jk = (double)Dk * 2^-32 + lam_q * (double)A and Jz = (double)Dz * 2^-16: each uint64 -> binary64 conversion one
 *                  round-to-nearest-even conversion, each remaining operation one IEEE binary64 operation
 *      skip(c)     !inelig(c) && (nzA(c) == 0 || Jz < Jk).  Strict, so lambda = 0 still returns round(y); the first clause makes
 *                  "emptied by RDOQ" and "skipped" the same state
 *    A skipped channel: its plane of y_rdo is +0.0; it contributes 0 to bits_q_after and chan_bits_q_after[c], nz0(c) to n_changed,
 *    Dz(c) << 16 to the distortion sum (3e's wrap caveat applies there and nowhere else).  abs_max and zero_bitmap are those of the
 *    final y_rdo; bits_q_before is unchanged.  Consequence: for finite y the estimate call (3b) on y_rdo returns exactly
 *    bits_q_after and the same zero_bitmap.
 *    The calls take the _w arguments plus an array of `count` side structures of OUTPUTS, or NULL; with NULL they return exactly
 *    what the _w forms return - which ARE the _s forms with NULL.  With skipping on, the curve's bits_q_after[j], n_changed[j] and
 *    ddist_q[j] are the sums after the channel decisions at lambda_j; the budget search is 3d's, untouched, over that f, and its
 *    last step is the skip-form RDOQ at lambda*.  n_eligible counts the coded channels that are not inelig; `skipped` (HOST
 *    int64[M], may be NULL) is 1 for a skipped channel, else 0.
 * ---------------------------------------------------------------------------------------------------------- */
#define FGMM_SKIP_VMAX 15
typedef struct {
  int64_t *skipped;        /* HOST int64[M] out, or NULL */
  int64_t n_skipped;       /* out: channels skipped */
  int64_t n_eligible;      /* out: coded channels that may be skipped */
  uint64_t ddist_q;        /* out: the weighted added distortion of y_rdo over round(y), units of 2^-32 */
} fgmm_rdo_skip;
typedef struct {
  uint64_t n_skipped[FGMM_RDCURVE_MAX]; /* out: channels skipped at lambda_j */
  int64_t n_eligible;                   /* out */
} fgmm_rdcurve_skip;
int fgmm_gmc_rdoq_batch_s(fgmm_ctx *ctx, void *stream, fgmm_rdoq_item *items, int count, int mode, int clamp_scales, double lambda,
                          const fgmm_rdo_weights *w /* [count] or NULL */, fgmm_rdo_skip *skip /* [count] or NULL */);
int fgmm_gmc_rdcurve_batch_s(fgmm_ctx *ctx, void *stream, fgmm_rdcurve_item *items, int count, int mode, int clamp_scales,
                             const double *lambdas, int n_lambda, const fgmm_rdo_weights *w /* [count] or NULL */,
                             fgmm_rdcurve_skip *skip /* [count] or NULL */);
int fgmm_gmc_rdoq_budget_batch_s(fgmm_ctx *ctx, void *stream, fgmm_rdoq_item *items, int count, int mode, int clamp_scales,
                                 const int32_t *group_or_null, int n_groups, const uint64_t *budget_bytes, double lambda_max, int refine,
                                 fgmm_budget_result *results /* per group */, const fgmm_rdo_weights *w /* [count] or NULL */,
                                 fgmm_rdo_skip *skip /* [count] or NULL */);

/* ------------------------------------------------------------------------------------------------------------
 * 3g. The entropy model's forward(): the DIFFERENTIABLE likelihood of a latent under its mixture, its rate, and the gradients of
 *    either - what evaluation (bpp from the likelihoods) and training (the rate term of the loss) run on
 *    (entropy_models.py:674-678, 720-737, 774-808).  One kernel forward, one backward; the backward recomputes everything from the
 *    inputs, nothing is kept in between.  Per latent, in binary32, every operation one IEEE operation (no contraction, correctly
 *    rounded '/'), K = 4; sb = scale_bound and lb = likelihood_bound are binary32 values of the caller's:
 *      v   = round ? rintf(y) : y                          (quantize "dequantize" with means=None, or the caller's noised input)
 *      s_k = max(sigma_k, sb) as torch.max does it: a NaN sigma stays NaN                        (LowerBound, bound_ops.py:36-37)
 *      a_k = fabsf(v - mu_k)
 *      xu  = (0.5f - a_k) / s_k        xl = (-0.5f - a_k) / s_k
 *      u   = 0.5f * erfcf(c * xu)      l  = 0.5f * erfcf(c * xl)       c = (float)(-(2^-0.5))
 *      p_k = u - l
 *      L   = (((0 + p_0*pi_0) + p_1*pi_1) + p_2*pi_2) + p_3*pi_3      (separate multiply and add, k ascending: :777-788)
 *      out = lb > 0 ? max(L, lb) : L                                   (NaN stays NaN)
 *    There is no upper clamp of sigma here, unlike the coder's.
 *    Rate: bits_q is the sum, over the latents with a finite out > 0, of llrint(-log2((double)out) * 2^32) - units of 2^-32 bit,
 *    summed in 64-bit integers (the same bits on every run; a term is negative where out > 1, which weights that do not sum to 1
 *    allow).  Latents whose out is NaN, infinite or <= 0 are left out of the sum and counted in n_nonfinite.
 *    Backward: the upstream gradient g arrives w.r.t. out.  With phi(x) = expf(-0.5f*x*x) * (float)(1/sqrt(2*pi)):
 *      gL       = ((L >= lb) || (g < 0) || lb <= 0) ? g : 0                                      (bound_ops.py:40-42)
 *      dpi_k    = gL * p_k
 *      da_k     = -pi_k * (phi(xu) - phi(xl)) / s_k
 *      sg       = (v > mu_k) - (v < mu_k)                                                        (torch's abs: 0 at 0)
 *      dmu_k    = -gL * da_k * sg            dv += gL * da_k * sg      (dv from 0, k ascending)
 *      G_k      = gL * ( -pi_k * (phi(xu)*xu - phi(xl)*xl) / s_k )     (the gradient arriving at s_k)
 *      dsigma_k = ((sigma_k >= sb) || (G_k < 0)) ? G_k : 0
 *      dy       = round ? 0 : dv
 *    Both rules are selects: a NaN or +inf g or G_k that its rule does not pass gives 0 here, where the reference's `mask * g` gives NaN.
 *    With g_like NULL the upstream gradient is the scalar g_bits on the item's bit count (bits, not bits_q), and the kernel forms
 *    g = -gb / (out * ln2f) itself, gb = (float)g_bits, ln2f = 0x1.62e430p-1f, out the bounded value; 0 for a latent that is left
 *    out of the sum.  The rule above is then applied with that g.
 *    Planes are float32, float16 or bfloat16 (one dtype per batch, widened exactly on load: the result of either call is that of the
 *    same call on float32 planes holding the widened values, bit for bit); flags must be 0 - FGMM_PARAMS_LOGITS is refused, the
 *    softmax over K stays the caller's so that autograd differentiates it.  The gradient planes are float32 whatever the planes are.
 *    y, like_out, v_out, g_like, dy: float32 [M*hw].  Refused with FGMM_ERR_INVALID before any launch: K != 4, flags != 0, a null y,
 *    a scale_bound that is not positive and finite, a likelihood_bound that is negative or not finite, a backward item whose outputs
 *    are all NULL.  The caller's-stream contract is section 2's: the work is ordered after `stream`, the call returns with every
 *    output complete.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct {
  const float *y;          /* device [M*hw] */
  fgmm_params params;      /* flags must be 0 (section 3h: FGMM_PARAMS_LOGITS) */
  int32_t M, K;
  int64_t hw;
  float *like_out;         /* DEVICE float32[M*hw] out: the bounded likelihood, or NULL (the rate alone) */
  float *v_out;            /* DEVICE float32[M*hw] out: v, or NULL */
  int64_t bits_q;          /* out: units of 2^-32 bit */
  int64_t n_nonfinite;     /* out: latents left out of bits_q */
  int32_t status, pad_;    /* out */
} fgmm_like_item;
int fgmm_gmc_likelihood_batch(fgmm_ctx *ctx, void *stream, fgmm_like_item *items, int count, int round, float scale_bound,
                              float likelihood_bound);
typedef struct {
  const float *y;          /* device [M*hw]: what the forward call was given (round == 0: the noised v) */
  fgmm_params params;      /* flags must be 0 (section 3h: FGMM_PARAMS_LOGITS) */
  int32_t M, K;
  int64_t hw;
  const float *g_like;     /* device float32[M*hw]: the gradient w.r.t. like_out, or NULL: g_bits is used */
  double g_bits;           /* the gradient w.r.t. the item's bit count, bits_q * 2^-32 */
  float *dy;               /* DEVICE float32[M*hw] out, or NULL */
  float *dscales, *dmeans, *dweights; /* DEVICE float32[K*M*hw] out, contiguous [K, M, hw]; each may be NULL */
  int32_t status, pad_;    /* out */
} fgmm_like_grad_item;
int fgmm_gmc_likelihood_backward_batch(fgmm_ctx *ctx, void *stream, fgmm_like_grad_item *items, int count, int round, float scale_bound,
                                       float likelihood_bound);

/* ------------------------------------------------------------------------------------------------------------
 * 3h. 3g FROM THE PARAMETER HEAD'S LOGITS: the softmax over K and its derivative run inside the two kernels, so that evaluation-mode
 *    bits, the size estimate, RDOQ and the coder all see the same pi for the same logits, and no plane of weights, of their gradient
 *    or of the softmax's backward exists between the head and the kernels.  Same item structures and signatures as 3g; every item
 *    carries params.flags == FGMM_PARAMS_LOGITS, its `weights` planes hold the logits l_k, and `dweights` receives the gradient with
 *    respect to the LOGITS.  Per latent, in binary32, every operation one IEEE operation (no contraction), K = 4:
 *      pi  = softmax4(l_0 .. l_3): the one sequence of section 2 that every kernel runs under FGMM_PARAMS_LOGITS and that
 *            fgmm_softmax4_hip exposes -
 *              m   = max(l_0 .. l_3)                                         (fmaxf: a NaN logit does not win)
 *              e_k = exp(l_k - m) by the library's fixed sequence, exactly 0 where !(l_k - m >= -41)   (a NaN logit too)
 *              s   = (e_0 + e_1) + (e_2 + e_3)
 *              pi_k = e_k / s, correctly rounded
 *      Forward: section 3g, unchanged, on that pi -> out, v, bits_q, n_nonfinite.
 *      Backward: section 3g, unchanged, on that pi -> gL, dy, dsigma_k, dmu_k; and with dpi_k = gL * p_k (3g's dweights, not stored here)
 *        t    = ((pi_0*dpi_0 + pi_1*dpi_1) + pi_2*dpi_2) + pi_3*dpi_3       (separate multiply and add)
 *        dl_k = pi_k * (dpi_k - t)                                           (stored where 3g stores dweights)
 *    The result of either call is, bit for bit, that of the 3g call on float32 planes holding fgmm_softmax4_hip's weights of the
 *    (widened) logits, dl_k formed from its dweights as above.  Non-finite logits give what softmax4 gives, nothing is special-cased:
 *    a NaN logit gets weight 0; four logits of -inf, or a +inf among them, give NaN weights, hence a NaN out, which is left out of
 *    bits_q and counted.  Planes are float32, float16 or bfloat16 as in 3g, two-byte logits widened exactly; the condition of the
 *    coding calls that two-byte weights sum to at most 1 does not exist for logits.  The launch form - positions per lane, grid - is
 *    decided exactly as in 3g.  One call is one form: refused with FGMM_ERR_INVALID before any launch, nothing written, is an item
 *    whose flags are not exactly FGMM_PARAMS_LOGITS (a batch that mixes the two forms included), and everything 3g refuses; the two
 *    entry points of 3g keep refusing the flag.  The caller's-stream contract is section 2's, as in 3g.
 * ---------------------------------------------------------------------------------------------------------- */
int fgmm_gmc_likelihood_logits_batch(fgmm_ctx *ctx, void *stream, fgmm_like_item *items, int count, int round, float scale_bound,
                                     float likelihood_bound);
int fgmm_gmc_likelihood_logits_backward_batch(fgmm_ctx *ctx, void *stream, fgmm_like_grad_item *items, int count, int round, float scale_bound,
                                              float likelihood_bound);

/* ------------------------------------------------------------------------------------------------------------
 * 3i. CENTROID RECONSTRUCTION of a decoded latent: the conditional mean of the bin [q - 1/2, q + 1/2) under the latent's mixture
 *    (the Lloyd-Max centroid), which minimises the expected squared latent error.  The decoder holds the twelve parameters of
 *    every latent; this spends them, as RDOQ (3c) does on the encoder side.  It costs no bit and changes no format; what it buys in
 *    the image domain depends on the trained synthesis transform and is not claimed here.  One kernel, on the frame and with the
 *    terms of 3g's forward.  Per latent, in binary32, every operation one IEEE operation (no contraction, correctly rounded '/'),
 *    K = 4; sb = scale_bound and p_min are binary32 values of the caller's; xu, xl, u, l, p_k, L and phi are exactly 3g's:
 *      v    = rintf(y)                     (y is normally the decoder's integer y_hat: rintf is then the identity)
 *      s_k  = max(sigma_k, sb), a NaN sigma stays NaN; no upper clamp - this is the trained model's density, not the coder's Phi
 *      t_k  = v - mu_k        a_k = fabsf(t_k)        sg_k = (t_k > 0) - (t_k < 0)
 *      xu   = (0.5f - a_k) / s_k           xl = (-0.5f - a_k) / s_k
 *      p_k  = 0.5f * erfcf(c * xu) - 0.5f * erfcf(c * xl)
 *      L    = (((0 + p_0*pi_0) + p_1*pi_1) + p_2*pi_2) + p_3*pi_3                 (3g's L, NOT bounded)
 *      phi(x) = expf((-0.5f * x) * x) * (float)(1/sqrt(2*pi))
 *      m_k, the bin's first moment about v under component k up to its sign -
 *        narrow component (s_k < 2):   m_k = a_k*p_k - s_k*(phi(xu) - phi(xl))
 *        wide component (s_k >= 2):    h = 0.5f / s_k      xb = a_k * (h + h)      h2 = h*h      x2 = xb*xb
 *                                      q   = (C23 + (h2*(x2 - 3)) * C15) + ((h2*h2) * ((x2 - 10)*x2 + 15)) * C420
 *                                      m_k = ((a_k * phi(xb)) * (h*h2)) * q
 *                                      C23 = (float)(2/3), C15 = (float)(1/15), C420 = (float)(1/420)
 *      N    = sum_k (pi_k*sg_k) * m_k      (from 0, k ascending, separate multiply and add)
 *      off  = (-N) / L
 *      keep = (L >= p_min) && (fabsf(off) <= 0.5f) && every s_k < +inf             (any NaN makes it false)
 *      rec  = keep ? v + off : v
 *    The wide form is the narrow one expanded in h = 1/(2 s_k) (terms h^3, h^5, h^7 of the moment; the next one is below 3e-5 of
 *    the first at s_k = 2, |t_k| <= 4.5 s_k).  It is there because the narrow form cancels to 1/(12 s_k^2) of its terms: in binary32
 *    it is off by 5e-3 at sigma near 256 and by up to 0.49 at sigma up to 3000.  A component whose sigma is +inf carries no mass;
 *    the latent then keeps v, like one with any NaN among its terms.  p_min: below the coder's resolution (2^-16, the Python
 *    default) the symbol is bypass-coded, the model says nothing about the bin and L is rounding noise.  A non-finite y has L = 0
 *    or NaN and comes back as rintf(y).
 *    With FGMM_PARAMS_LOGITS in every item's params.flags the weights planes hold logits and pi = softmax4(l) as in 3h; the result
 *    is, bit for bit, that of the plain call on float32 planes holding fgmm_softmax4_hip's weights.  Non-finite logits give what
 *    softmax4 gives, as in 3h: a NaN or -inf logit is a component of weight 0; a +inf logit, or four of -inf, give NaN weights and
 *    the latent keeps v.  One call is one form.  Planes are float32, float16 or bfloat16 (one dtype per batch,
 *    widened exactly on load: the result is that of float32 planes holding the widened values, bit for bit).  The launch form -
 *    positions per lane, grid - is decided exactly as in 3g's forward.
 *    rec: DEVICE float32 [M*hw]; it may be y itself.  n_kept: the latents with keep, counted per wave and summed by one integer
 *    atomic per wave - the same bits on every run.  Refused with FGMM_ERR_INVALID before any launch, nothing written: K != 4,
 *    flags other than 0 or FGMM_PARAMS_LOGITS or differing within the batch, a null y or rec, a scale_bound that is not positive
 *    and finite, a p_min that is not positive and finite.  The caller's-stream contract is section 2's.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct {
  const float *y;          /* device [M*hw] */
  fgmm_params params;      /* flags: 0, or FGMM_PARAMS_LOGITS in every item of the batch */
  int32_t M, K;
  int64_t hw;
  float *rec;              /* DEVICE float32[M*hw] out; may alias y */
  int64_t n_kept;          /* out: latents whose reconstruction left the integer grid's v (keep) */
  int32_t status, pad_;    /* out */
} fgmm_centroid_item;
int fgmm_gmc_centroid_batch(fgmm_ctx *ctx, void *stream, fgmm_centroid_item *items, int count, float scale_bound, float p_min);

/* ------------------------------------------------------------------------------------------------------------
 * 3j. The ENTROPY BOTTLENECK's forward(): the DIFFERENTIABLE likelihood of the hyper-latent z under the factorized density
 *    (entropy_models.py:434-463, 465-510), its rate, and the gradients of either - the z half of what 3g is for y.  Per channel
 *    the density is a 1 -> 3 -> 3 -> 3 -> 3 -> 1 network (filters (3, 3, 3, 3), the reference's default and what both GMM models
 *    construct), evaluated at both edges of every element's bin.  One kernel forward; one backward that recomputes everything
 *    from the inputs and writes one partial row per workgroup, and a small kernel that sums the rows in index order: no float
 *    atomics, the same call gives the same bits every time.  The forward in binary32, every operation one IEEE operation (no
 *    contraction, correctly rounded '/'); expf, log1pf and tanhf are the device library's.  (The backward: see there.)
 *    Parameters: one float32 block theta[C][58] of the RAW parameters, per channel in this order, matrices row-major [out][in]:
 *      M0[3] b0[3] f0[3] | M1[9] b1[3] f1[3] | M2[9] b2[3] f2[3] | M3[9] b3[3] f3[3] | M4[3] b4[1]
 *    (the reference's _matrix{i}, _bias{i}, _factor{i} of a channel, flattened, in that order), and med[C], the medians.
 *    Per channel:   H_i = softplus of M_i as torch's: m > 20 ? m : log1pf(expf(m))          t_i = tanhf(f_i)
 *    chain(x):      layer 0:      a_j = H0_j*x + b0_j;                                 h_j = a_j + t0_j*tanhf(a_j)
 *                   layers 1 - 3: a_j = ((H_j0*h_0 + H_j1*h_1) + H_j2*h_2) + b_j;      h_j = a_j + t_j*tanhf(a_j)
 *                   layer 4:      the same sum, without the tanh step                 (sums from the left, multiply and add separate)
 *    Per element, c its channel:
 *      v    = mode ? rintf(x - med_c) + med_c : x      (mode 1: the reference's "dequantize"; mode 0: the caller's noised values)
 *      lo   = chain(v - 0.5f)       up = chain(v + 0.5f)
 *      sig(a) = 1 / (1 + expf(-a))
 *      flip = (lo + up) > 0
 *      L    = flip ? sig(-lo) - sig(-up) : sig(up) - sig(lo)
 *      out  = lb > 0 ? max(L, lb) : L                                                   (NaN stays NaN)
 *    THE MIRRORED FORM: the reference forms sig(up) - sig(lo) as written, everywhere.  In binary32 that is rounding noise in the
 *    upper tail, where both terms are near 1 (relative error above 1 on a corpus reaching x = 400, against 4e-5 for the form
 *    here); the two forms are the same function (they differ by 3e-16 in binary64).  Evaluation-mode bits of this call are
 *    therefore closer to the binary64 value than the reference's own binary32 run is.
 *    Rate, as in 3g: bits_q[b] is the sum, over item b's elements with a finite out > 0, of llrint(-log2((double)out) * 2^32),
 *    summed in 64-bit integers; the remaining elements are counted in n_nonfinite[b].
 *    Backward: g arrives w.r.t. out, or (g_like NULL) is formed from g_bits[b] exactly as 3g forms it: g = -gb / (out * ln2f),
 *    gb = (float)g_bits[b], 0 for an element that is left out of the sum.
 *      gL   = ((L >= lb) || (g < 0) || lb <= 0) ? g : 0                                  (a select, as in 3g)
 *    L, out and with them g and gL are the forward's binary32 values: the decisions are the forward call's.  THE DERIVATIVES ARE
 *    EVALUATED IN BINARY64, on the same binary32 inputs (theta, med, v and gL widened exactly; H_i, t_i, both chains, sig, the
 *    sums below: the same sequences in binary64 with the device library's exp, log1p and - for t_i - tanh; inside the chains
 *    tanh(a) = 1 - 2 / (exp(a + a) + 1), absolute error a few 2^-53), and rounded to binary32 once, where they are stored.  A parameter's gradient is a sum over the channel's elements of terms of both signs that cancels to
 *    a hundredth of their magnitude and less; in binary32 the rounding of the terms themselves, which the chain amplifies by the
 *    logit, reaches the fifth digit of such a sum (measured on the test corpus, for this sequence and for torch's alike).
 *      dup  = gL * (sig(up) * sig(-up))        dlo = -gL * (sig(lo) * sig(-lo))          (the flip changes neither derivative)
 *    Each chain in reverse, recomputed, d its dup or dlo, th_j = tanh(a_j) of the layer, h the layer's input:
 *      layer 4:      db += d;  dH_k += d*h_k;  dh_k = d*H_k
 *      layers 3 - 1: da_j = dh_j + dh_j*(t_j*(1 - th_j*th_j));  dt_j += dh_j*th_j;  db_j += da_j;  dH_jk += da_j*h_k;
 *                    dh_k = (H_0k*da_0 + H_1k*da_1) + H_2k*da_2
 *      layer 0:      the same with h = the chain's x;  dv += (H_0*da_0 + H_1*da_1) + H_2*da_2
 *    dH, db, dt are summed (binary64) over the channel's B*hw elements: per lane, then across the wave by shuffles, across the
 *    workgroup's waves through LDS, one row per workgroup; then over the channel's ceil(B*hw / FGMM_EB_SLICE) rows in index
 *    order, and once per channel    dM = dH * (m > 20 ? 1 : sig(m))        df = dt * (1 - t*t),   rounded to binary32.
 *      dx     = mode ? 0 : dv
 *      dmed_c = mode ? the sum of dv over the channel : 0   (the medians are a live parameter: `outputs += means` passes the gradient)
 *    The geometry depends on (B, C, hw) alone, never on addresses: per-element outputs are those of the same elements in any other
 *    shape, bit for bit; loads are 4 wide where hw and every address allow it, which changes no result.
 *    x, like_out, v_out, g_like, dx: DEVICE float32 [B, C, hw] contiguous; theta, dtheta: DEVICE float32 [C][58]; med, dmed:
 *    DEVICE float32 [C]; bits_q, n_nonfinite, g_bits: HOST arrays [B].  Refused with FGMM_ERR_INVALID before any launch, nothing
 *    written: a null call, x, theta or med; B, C or hw < 1; a mode other than 0 or 1; a negative or non-finite likelihood_bound;
 *    a backward call whose outputs are all NULL, or with neither g_like nor g_bits, or a non-finite g_bits[b] where it is used.
 *    The caller's-stream contract is section 2's: the work is ordered after `stream`, the call returns with every output complete.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct {
  const float *x;          /* device [B, C, hw] */
  const float *theta;      /* device [C][FGMM_EB_PARAMS] */
  const float *med;        /* device [C] */
  int32_t B, C;
  int64_t hw;
  float *like_out;         /* DEVICE float32[B*C*hw] out: the bounded likelihood, or NULL (the rate alone) */
  float *v_out;            /* DEVICE float32[B*C*hw] out: v, or NULL */
  int64_t *bits_q;         /* HOST [B] out, or NULL: units of 2^-32 bit */
  int64_t *n_nonfinite;    /* HOST [B] out, or NULL: elements left out of bits_q */
  int32_t status, pad_;    /* out */
} fgmm_eb_call;
int fgmm_eb_likelihood(fgmm_ctx *ctx, void *stream, fgmm_eb_call *call, int mode, float likelihood_bound);
typedef struct {
  const float *x;          /* device [B, C, hw]: what the forward call was given (mode 0: the noised v) */
  const float *theta;      /* device [C][FGMM_EB_PARAMS] */
  const float *med;        /* device [C] */
  int32_t B, C;
  int64_t hw;
  const float *g_like;     /* device float32[B*C*hw]: the gradient w.r.t. like_out, or NULL: g_bits is used */
  const double *g_bits;    /* HOST [B]: the gradient w.r.t. each item's bit count, bits_q * 2^-32; read when g_like is NULL */
  float *dx;               /* DEVICE float32[B*C*hw] out, or NULL */
  float *dtheta;           /* DEVICE float32[C][FGMM_EB_PARAMS] out, or NULL */
  float *dmed;             /* DEVICE float32[C] out, or NULL */
  int32_t status, pad_;    /* out */
} fgmm_eb_grad_call;
int fgmm_eb_likelihood_backward(fgmm_ctx *ctx, void *stream, fgmm_eb_grad_call *call, int mode, float likelihood_bound);

/* ------------------------------------------------------------------------------------------------------------
 * 3k. The ENTROPY BOTTLENECK's update(): the quantiles of the factorized density and the coding tables of the z hyper-latent
 *    (entropy_models.py:391-427, 573-603), the step between training on 3j and coding on section 4.  Once per checkpoint, no hot
 *    path; on the GPU because the masses that become the tables must be the ones 3j assigns to the same points: H_i, t_i, chain
 *    and sig are 3j's, theta [C][58] is 3j's, binary32 throughout, the same device code.
 *    QUANTILES.  Per channel c and k = 0, 1, 2, an independent search for chain_c(q) = targets[k] (the reference searches all
 *    channels together and stops when ALL pass isclose(rtol 1e-4, atol 1e-3): a channel's result there depends on the others):
 *      lo = -search_radius, hi = search_radius
 *      lo = targets[k] <= chain(hi) ? lo : hi;   then   hi = chain(lo) <= targets[k] ? hi : lo      (the reference's non-strict start: a
 *                                                        target that is not bracketed collapses the interval onto the bound it lies beyond)
 *      at most FGMM_EB_SEARCH_CAP times:  mid = (lo + hi) / 2;  stop if mid == lo or mid == hi;  f = chain(mid);
 *                                         lo = f <= targets[k] ? mid : lo;   hi = f >= targets[k] ? mid : hi
 *      q[c][k] = (lo + hi) / 2
 *    The search ends where binary32 cannot split the interval (about 190 steps on [-1e5, 1e5] at the most, the cap is never the
 *    reason with finite values).  IF ANY chain VALUE OF A SEARCH IS NaN (NaN parameters; infinite ones where inf - inf arises) THE
 *    SEARCH STOPS AND q[c][k] IS NaN - the reference's loop does not end then.  Infinite chain values compare as they are.
 *    One 64-lane workgroup per channel.  Stream-ordered: the call returns once the kernel is queued on `stream`; q_out is DEVICE
 *    float32 [C][3].  targets: HOST float[3].  Refused (FGMM_ERR_INVALID, nothing queued): a null ctx, theta, targets or q_out;
 *    C < 1; a NaN target; a search_radius that is not finite and > 0.
 *    TABLES.  start[c] (float32) and length[c] (int32) describe channel c's integer support s_i = start + (float)i, i < length
 *    (the reference's pmf_start and pmf_length).  Row c of the masses, `stride` floats:
 *      entry i < length:   lo = chain(s_i - 0.5f), up = chain(s_i + 0.5f);  3j's L (the mirrored form, NO bound: update() applies
 *                          none): bit for bit what fgmm_eb_likelihood writes for x = s_i in mode 0 with likelihood_bound 0
 *      entry length:       the tail mass  sig(chain(s_0 - 0.5f)) + sig(-chain(s_{length-1} + 0.5f))      (entropy_models.py:422; the
 *                          reference takes the upper term at the LONGEST channel's last sample for every channel, which is the
 *                          channel's own wherever all lengths are equal and below its own tail otherwise)
 *      entries after it:   +0
 *    The rows come to the host, where compressai._CXX.pmf_to_quantized_cdf (fgmm_pmf_to_quantized_cdf, section 4; precision 16)
 *    runs on the length + 1 entries of every channel: cdf_out, HOST int32 [C][stride + 1], row c = its length + 2 cumulative
 *    counts, then zeros (entropy_models.py:206-214).  The call returns when cdf_out is complete.  pmf_out: NULL, or DEVICE float32
 *    [C][stride], the rows as the quantiser saw them.  failed_channel_out: NULL, or HOST int32[1]: -1, or the channel refused.
 *    start, length, theta: DEVICE.  Refused with FGMM_ERR_INVALID, cdf_out and pmf_out left as they were: a null ctx, theta, start,
 *    length or cdf_out; C < 1; stride < 2; C * stride beyond 2^31 - 1; and, found after the kernel has run, the first channel with
 *    length < 1 or length + 1 > stride, with a mass that is negative or not finite, with masses that all round to zero, or with
 *    more symbols (length + 1) than 2^16 counts - *failed_channel_out names it.
 * ---------------------------------------------------------------------------------------------------------- */
int fgmm_eb_quantiles(fgmm_ctx *ctx, void *stream, const float *theta, int C, const float *targets, float search_radius, float *q_out);
int fgmm_eb_tables(fgmm_ctx *ctx, void *stream, const float *theta, const float *start, const int32_t *length, int C, int stride,
                   float *pmf_out, int32_t *cdf_out, int32_t *failed_channel_out);

/* ------------------------------------------------------------------------------------------------------------
 * 4. Table path — the `z` hyper-latent coder: CompressAI's original table rANS, the other
 *    half of `compressai.ans`.  Host only, integer only.  `cdfs` is a row-major int32 [n_cdfs, cdf_stride] matrix
 *    (the reference takes a list of lists, rans_interface.cpp:334-338); every index is validated here (the
 *    reference's asserts are compiled out).
 * ---------------------------------------------------------------------------------------------------------- */

/* RansEncoder.encode_with_indexes(symbols, indexes, cdfs, cdfs_sizes, offsets) -> bytes  (rans_interface.cpp:587-598) */
int fgmm_encode_with_indexes(const int32_t *symbols, const int32_t *indexes, int64_t n, const int32_t *cdfs,
                             int64_t cdf_stride, int32_t n_cdfs, const int32_t *cdfs_sizes, const int32_t *offsets,
                             uint8_t **out, size_t *out_len);
/* RansDecoder.decode_with_indexes(encoded, indexes, cdfs, cdfs_sizes, offsets) -> int32[n]  (rans_interface.cpp:619-688) */
int fgmm_decode_with_indexes(const uint8_t *encoded, size_t encoded_len, const int32_t *indexes, int64_t n,
                             const int32_t *cdfs, int64_t cdf_stride, int32_t n_cdfs, const int32_t *cdfs_sizes,
                             const int32_t *offsets, int32_t *out_symbols);

/* BufferedRansEncoder (rans_interface.hpp:57-86): symbols accumulate over calls — table calls and GMM symbol tables
 * may be mixed — and ONE stream is flushed (rans_interface.cpp:557-585). */
typedef struct fgmm_symbuf fgmm_symbuf;
int fgmm_symbuf_create(fgmm_symbuf **out);
void fgmm_symbuf_destroy(fgmm_symbuf *b);
int64_t fgmm_symbuf_size(const fgmm_symbuf *b); /* entries buffered (symbols + escape nibbles) */
int fgmm_symbuf_append_table(fgmm_symbuf *b, const int32_t *symbols, const int32_t *indexes, int64_t n,
                             const int32_t *cdfs, int64_t cdf_stride, int32_t n_cdfs, const int32_t *cdfs_sizes,
                             const int32_t *offsets);
int fgmm_symbuf_append_symtab(fgmm_symbuf *b, const uint32_t *packed, const int32_t *symbols_or_null, int64_t n);
int fgmm_symbuf_flush(fgmm_symbuf *b, uint8_t **out, size_t *out_len); /* empties the buffer */
/* GPU-built GMM symbols appended to a buffer: BufferedRansEncoder.encode_with_indexes_gmm (rans_interface.cpp:458-554) */
int fgmm_symbuf_append_gmm(fgmm_ctx *ctx, fgmm_symbuf *b, const int32_t *symbols, const float *scales,
                           const float *means, const float *weights, int64_t n, int64_t stride_n, int64_t stride_k,
                           int K, int mode, int memspace);

/* RansDecoder.set_stream / decode_stream (rans_interface.cpp:886-956): a decoder that keeps its state between calls */
typedef struct fgmm_decstream fgmm_decstream;
int fgmm_decstream_create(const uint8_t *encoded, size_t encoded_len, fgmm_decstream **out); /* copies the stream */
void fgmm_decstream_destroy(fgmm_decstream *d);
int fgmm_decstream_decode(fgmm_decstream *d, const int32_t *indexes, int64_t n, const int32_t *cdfs, int64_t cdf_stride,
                          int32_t n_cdfs, const int32_t *cdfs_sizes, const int32_t *offsets, int32_t *out_symbols);

/* ---- section 5: the callers either side of the path ---------------------------------
 * CheckerboardLatentCodec.unembed / embed (compressai/latent_codecs/checkerboard.py:333-377): split a [planes, h, w]
 * device tensor into its two checkerboard halves [2, planes, h, w/2] (half 0 = anchors) and back.  planes = n * c;
 * w must be even; elem_bytes 4 (float32 / int32) or 2 (float16 / bfloat16); anchor_odd = 0 for anchor_parity "even" (anchors at
 * (even row, even column) and (odd row, odd column)), 1 for "odd".  Pure data movement: any bit pattern is preserved.
 * STREAM-ORDERED, unlike the calls of sections 2 and 3: the one kernel is enqueued on `stream` (NULL = default stream), behind
 * whatever the caller enqueued there before, and the call returns WITHOUT waiting for it.  `dst` is complete for work enqueued on
 * `stream` afterwards, and for another stream or the host only once they have waited for `stream` (an event recorded on it after
 * the call, or a synchronisation); `src` must stay valid and unchanged until then.  No workspace of the context is used, and the
 * context is not locked: calls from several threads on several streams run concurrently.  A refused call (odd w, a full tensor
 * that is not aligned to a pair of elements, a halves tensor not aligned to an element) launches nothing and writes nothing. */
int fgmm_ckbd_unembed(fgmm_ctx *ctx, void *stream, const void *src, void *dst, int64_t planes, int64_t h, int64_t w,
                      int elem_bytes, int anchor_odd);
int fgmm_ckbd_embed(fgmm_ctx *ctx, void *stream, const void *src, void *dst, int64_t planes, int64_t h, int64_t w,
                    int elem_bytes, int anchor_odd);

/* ---- section 5b. The checkerboard CONTEXT CONVOLUTION on the matrix cores, in one fixed order -------
 * Replaces unembed(context_prediction(embed(y_hat_)))[1] of CheckerboardLatentCodec (compressai/latent_codecs/checkerboard.py:281-284,
 * 310-313) where context_prediction is a CheckerboardMaskedConv2d(M, C_out, kernel_size=5, padding=2): the compact anchors half in,
 * the compact non-anchor context out, one launch.  Inference only.
 *   A      [M, h, w/2] float32: the anchors half, as fgmm_ckbd_unembed lays out half 0; s = anchor_odd
 *          the anchor     at compact (r, j) is full-size (r, 2j + ((r + s) & 1)),
 *          the non-anchor at compact (r, j) is full-size (r, 2j + 1 - ((r + s) & 1))
 *   taps   t = 0 .. 11: the kernel positions (i, j) with i + j odd, row-major - (0,1) (0,3) (1,0) (1,2) (1,4) (2,1) (2,3) (3,0) (3,2)
 *          (3,4) (4,1) (4,3).  For a non-anchor at full-size (r, c), tap (i, j) reads full-size (r + i - 2, c + j - 2): inside the
 *          image that is always an anchor, read from A at its compact place (the non-anchor half is never looked at); outside, +0.0,
 *          which takes part in the chain
 *   out[o] = the chain  acc = bias[o] (+0 without a bias); for t ascending, for c = 0 .. M-1 ascending:
 *                       acc = fmaf(weight[o][c][tap t], x(t, c), acc)
 * computed on v_mfma_f32_32x32x2_f32 bit for bit - signs of zero, infinities and NaN included - for the reason of section 2b: encoder
 * and decoder derive identical parameters from identical weights on any ROCm / torch / MIOpen version, and this convolution is the
 * largest reduction of the parameter chain (12 M terms).  The result is NOT MIOpen's in its last bits: both sides must use it. */
typedef struct fgmm_ckbd_context fgmm_ckbd_context; /* the packed weights, on the context's device.  Immutable once created: usable
                                                     * from any context on its device, from several at the same time */
/* weight: device float32 [C_out, M, 5, 5] (the EFFECTIVE weight: weight * mask); bias: device float32 [C_out] or NULL.  The 12 kept
 * taps are copied (packed) before the call returns; FGMM_ERR_INVALID if any of the 13 dropped taps of any filter is not +-0. */
int fgmm_ckbd_ctx_create(fgmm_ctx *ctx, void *stream, const float *weight, const float *bias, int M, int C_out, fgmm_ckbd_context **out);
void fgmm_ckbd_ctx_destroy(fgmm_ckbd_context *cc);
/* anchors: device float32 [n, M, h, w/2]; out: device float32 [n, C_out, h, w/2], the non-anchor half as fgmm_ckbd_unembed lays out
 * half 1.  STREAM-ORDERED, like the two calls of section 5: one kernel enqueued on `stream`, no workspace, no context lock, no host
 * wait; the same rules for `anchors` and `out` as for `src` and `dst` there.  Refused, launching and writing nothing: odd w, w < 2,
 * h < 1, n < 0, a null tensor with n > 0, sizes whose grid would overflow.  n == 0: success, no launch. */
int fgmm_ckbd_ctx_apply(fgmm_ctx *ctx, void *stream, const fgmm_ckbd_context *cc, const float *anchors, float *out, int n, int64_t h,
                        int64_t w, int anchor_odd);

/* ---- section 5c. The context convolution's GRADIENTS on the matrix cores, in one fixed order; caller-owned packed weights -------------
 * What CheckerboardLatentCodec._forward_onepass (compressai/latent_codecs/checkerboard.py:154-171) needs under autograd: there the
 * convolution's output is kept at the non-anchor positions only, where a checkerboard-masked filter reads only anchors - the forward
 * is exactly section 5b's operator on unembed(y_hat)[0].  Notation as 5b; g [n, C_out, h, w/2] is the gradient with respect to the
 * compact non-anchor context, hw = h * w/2, TAPS[t] = (i, j) the 12 kept kernel positions.
 *   DATA GRADIENT  dA[n][c][p], p the anchor at full-size (r, col): the chain  acc = +0; for u = 0 .. 11 ascending, for o = 0 ..
 *          C_out-1 ascending:  acc = fmaf(W[o][c][tap 11-u], gamma(u, o), acc), gamma(u, o) = g[n][o] at the non-anchor at full-size
 *          (r + i_u - 2, col + j_u - 2), (i_u, j_u) = TAPS[u]; +0 outside the image.  That is 5b's chain with the filters
 *          W'[c][o][i][j] = W[o][c][4-i][4-j], no bias, anchor_odd ^ 1, and M and C_out exchanged: fgmm_ckbd_ctx_pack(transposed = 1),
 *          then fgmm_ckbd_ctx_apply_packed(packed, C_out, M, g, dA, n, h, w, anchor_odd ^ 1).
 *   WEIGHT GRADIENT  the reduction runs over the positions of ALL items, concatenated: s = n hw + q, P = n_items hw, in slices whose
 *          number and length are a function of P alone (never of the device, the grid or the kernel variant):
 *              S0 = min(FGMM_CKBD_WGRAD_SLICES_MAX, ceil(P / FGMM_CKBD_WGRAD_SLICE_MIN)),  L = 32 ceil(P / (32 S0)),  S = ceil(P / L)
 *          slice k is s in [k L, min((k+1) L, P)) and may cross item boundaries (P = 1: S = 1, L = 32; 405: 2, 224; 4097: 15, 288 - a
 *          sixteenth slice would be empty; 4352: 16, 288, the last slice 32 long).
 *              partial_k[o][t M + c] = the chain  acc = +0; for s ascending in slice k:  acc = fmaf(g(s)[o], x(s)(t, c), acc)
 *              dW[o][c][tap t]       = ((partial_0 + partial_1) + partial_2) + ...   in binary32, ascending
 *          x(s)(t, c) is what tap t of channel c reads at the non-anchor s (5b; +0 outside the image, which takes part).  The 13
 *          dropped taps of every filter are written +0.  dbias[o]: the same slices in the same order with x = 1.
 *          On v_mfma_f32_32x32x2_f32 bit for bit - signs of zero, infinities and NaN included; no float atomics.
 *   A DIFFERENCE FROM THE REFERENCE  CheckerboardMaskedConv2d zeroes weight.data in place before every forward (compressai/layers/
 *          layers.py:141-144) and then differentiates a plain convolution: its dropped taps receive non-zero gradients, which never
 *          influence a forward value but do enter a global gradient-norm clip.  Here the gradient is that of weight * mask: +0 at the
 *          dropped taps. */
#define FGMM_HAS_CKBD_CONTEXT_GRAD 1 /* section 5c (added without a bump, as 3b - 5b) */
#define FGMM_CKBD_WGRAD_SLICE_MIN 256 /* positions a slice holds before the weight gradient's reduction is cut into more slices */
#define FGMM_CKBD_WGRAD_SLICES_MAX 16 /* slices at the most: the workspace holds as many partial copies of [C_out, 12 M + 1] */
/* Packed weights in CALLER-OWNED device memory (a training step repacks every time; fgmm_ckbd_ctx_create allocates, waits and reads a
 * flag back).  All five calls are STREAM-ORDERED like section 5's: enqueued on `stream`, no context lock, no host wait; a refused call
 * launches nothing and writes nothing.
 * fgmm_ckbd_ctx_packed_floats: float32 elements of `packed` for a convolution from M to C_out channels (0 for sizes that are refused).
 * fgmm_ckbd_ctx_pack: weight device float32 [C_out, M, 5, 5], the EFFECTIVE weight - the 13 dropped taps are not looked at (create keeps
 *   its refusal); transposed = 0 writes the layout create builds, into packed[fgmm_ckbd_ctx_packed_floats(M, C_out)]; transposed = 1
 *   writes W' above - a convolution from C_out to M channels, packed[fgmm_ckbd_ctx_packed_floats(C_out, M)], to be applied with the
 *   sizes exchanged - and takes no bias (a bias with it is refused).
 * fgmm_ckbd_ctx_apply_packed: fgmm_ckbd_ctx_apply on such a buffer; M, C_out are the PACKED convolution's.  Refusals as apply's. */
size_t fgmm_ckbd_ctx_packed_floats(int M, int C_out);
int fgmm_ckbd_ctx_pack(fgmm_ctx *ctx, void *stream, const float *weight, const float *bias, int M, int C_out, int transposed, float *packed);
int fgmm_ckbd_ctx_apply_packed(fgmm_ctx *ctx, void *stream, const float *packed, int M, int C_out, const float *anchors, float *out, int n,
                               int64_t h, int64_t w, int anchor_odd);
/* fgmm_ckbd_ctx_wgrad: anchors device float32 [n, M, h, w/2] (may be NULL when dweight is), g device float32 [n, C_out, h, w/2];
 * dweight device float32 [C_out, M, 5, 5] or NULL, dbias device float32 [C_out] or NULL: only what is asked for is computed.
 * workspace: device memory of at least fgmm_ckbd_ctx_wgrad_workspace(...) BYTES (S partial copies of [C_out, 12 M + 1] float32; 0 for
 * sizes that are refused or n == 0), aligned to 16 bytes, the call's own until the work enqueued by it has run.  Refused: what
 * fgmm_ckbd_ctx_apply refuses, n * h * w/2 beyond 2^31, a workspace that is null, smaller than that or misaligned, and both outputs NULL
 * with n > 0.  n == 0: success, no launch. */
size_t fgmm_ckbd_ctx_wgrad_workspace(int M, int C_out, int n, int64_t h, int64_t w);
int fgmm_ckbd_ctx_wgrad(fgmm_ctx *ctx, void *stream, const float *anchors, const float *g, int M, int C_out, int n, int64_t h, int64_t w,
                        int anchor_odd, float *dweight, float *dbias, void *workspace, size_t workspace_bytes);

/* compressai._CXX.pmf_to_quantized_cdf (compressai/cpp_exts/ops/ops.cpp:40-109): cdf_out has n + 1 entries */
int fgmm_pmf_to_quantized_cdf(const float *pmf, int n, int precision, uint32_t *cdf_out);

#ifdef __cplusplus
}
#endif
#endif /* FLASHGMM_AMD_H */
