/*
 * specdec.h — C ABI of the MI355X-native speculative verify/accept path.
 *
 * The reference (dadiaokua/speculative-decoding) is pure Python and has no FFI; this
 * library sits under the Python entry points it exposes for the hot path, which keep
 * their signatures (the specdec_amd Python package):
 *
 *   sd_verify      replaces the per-step verify block of
 *                    sampling/speculative_decoding.py:129-187   (rule SD_RULE_SPEC,   "A8")
 *                    engine/infer_engine.py:265-336             (rule SD_RULE_ENGINE, "A10")
 *                  including the processors it calls (utils/logits_processor.py:13-103),
 *                  max_fn (sampling/speculative_decoding.py:10-19) and the prune lengths fed
 *                  to utils/caching.py:6-24 (sampling/speculative_decoding.py:163-165).
 *   sd_sample      replaces LogitsProcessor.__call__ + .sample on the drafter / first-target
 *                  rows (sampling/speculative_decoding.py:95-96,120-123; engine/infer_engine.py:241-246).
 *   sd_mt19937_*   host-side mirror of torch's CPU generator (ATen mt19937) that feeds the
 *                  "stream" noise mode, so GPU results equal the reference's under a fixed
 *                  torch.manual_seed (torch.rand: engine/infer_engine.py:305,
 *                  sampling/speculative_decoding.py:139; torch.multinomial's Exp(1) noise).
 *
 * Conventions: all tensor pointers are device pointers (hipMalloc / torch CUDA memory);
 * the vocab axis has unit stride; other strides are in ELEMENTS.  Every entry point
 * returns SD_OK or a negative sd_status, never aborts, never allocates, never syncs the
 * host; kernels are enqueued on `stream` (a hipStream_t, passed as void*).  Per-row
 * failures (e.g. an all-zero residual under multinomial, which makes torch raise) are
 * reported in `row_status`, read back by the caller.
 */
#ifndef SPECDEC_H
#define SPECDEC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SD_ABI_VERSION 12
#define SD_MAX_GAMMA 32          /* drafts per call; specdec_amd.ops chunks longer windows */
#define SD_NGRAM_MAX_FILLER 64   /* sd_ngram_verify filler ids per pass; filler_k itself may be
                                    anything up to vocab (ABI 11: one more launch pair per 64)  */

typedef enum {
    SD_OK = 0,
    SD_ERR_INVALID = -1,      /* bad argument (null pointer, bad shape, bad enum)        */
    SD_ERR_WORKSPACE = -2,    /* workspace too small (see sd_*_workspace_size)            */
    SD_ERR_LAUNCH = -3,       /* hipLaunchKernel / hip runtime error                      */
    SD_ERR_UNSUPPORTED = -4,  /* combination not implemented                              */
} sd_status;

typedef enum { SD_F32 = 0, SD_BF16 = 1, SD_F16 = 2 } sd_dtype;

/* utils/logits_processor.py: GreedyProcessor :26, MultinomialProcessor :39, TopKProcessor :52,
 * NucleusProcessor :66, TopKNucleusProcessor :84.                                          */
typedef enum {
    SD_PROC_GREEDY = 0,
    SD_PROC_MULTINOMIAL = 1,
    SD_PROC_TOPK = 2,
    SD_PROC_NUCLEUS = 3,
    SD_PROC_TOPK_NUCLEUS = 4,
} sd_proc_kind;

typedef struct {
    int32_t kind;         /* sd_proc_kind                       */
    float temperature;    /* LogitsProcessor.temperature        */
    int32_t top_k;        /* TopK*.top_k                         */
    float top_p;          /* Nucleus*.top_p                      */
} sd_processor;

typedef enum {
    SD_RULE_SPEC = 0,     /* sampling/speculative_decoding.py:139-171: accept iff r <= p/q (fp32),
                             bonus sample on full accept, (p-q)+ residual on reject           */
    SD_RULE_ENGINE = 1,   /* engine/infer_engine.py:287-336: accept iff u < min(1,p/q) (fp64),
                             q<=0 accepts, eos ends the row, no bonus, residual on reject     */
} sd_rule;

typedef enum {
    SD_NOISE_STREAM = 0,  /* words[] = mt19937 outputs of torch's CPU generator (parity mode) */
    SD_NOISE_PHILOX = 1,  /* in-kernel Philox4x32-10 keyed by seed, counter offset (perf mode) */
} sd_noise_mode;

typedef struct {
    int32_t mode;            /* sd_noise_mode                                                 */
    const uint32_t* words;   /* STREAM: device buffer of generator words, consumed from [0]   */
    int64_t n_words;         /* STREAM: capacity; overrun => row_status SD_ROW_NOISE_OVERRUN  */
    uint64_t seed;           /* PHILOX: key                                                   */
    uint64_t offset;         /* PHILOX: per-call counter offset (caller advances it)          */
    int64_t row_base;        /* PHILOX: global id of row 0 of this call — noise is keyed by
                                (seed, offset, global row), so a batch sharded across ranks
                                draws exactly what one call over the whole batch draws     */
    const uint64_t* offset_dev;  /* PHILOX (nullable): device uint64 added to `offset` when the
                                kernels run — a captured hipGraph replays with fresh noise once
                                the caller advances it on the device between replays        */
} sd_noise;

/* row_status bits */
#define SD_ROW_DONE           0x1   /* the row was processed                                  */
#define SD_ROW_STOP_IN_DRAFTS 0x2   /* SPEC: an accepted draft is a stop token: the reference
                                       returns before sampling (speculative_decoding.py:150-155);
                                       stop_index holds its draft position                   */
#define SD_ROW_FINISHED       0x4   /* ENGINE: the row hit an end token (infer_engine.py:310,328) */
#define SD_ROW_RESIDUAL       0x8   /* x was drawn from the (p-q)+ residual                    */
#define SD_ROW_BONUS          0x10  /* x was drawn from the bonus row (full accept, SPEC)      */
#define SD_ROW_FALLBACK_P     0x20  /* ENGINE: residual mass <= 1e-12, x drawn from p (:319-321);
                                       SPEC skip_sample_adjustment: x drawn from p_n (:169-170) */
#define SD_ROW_INVALID_DIST   0x40  /* multinomial over NaN/zero mass: torch raises RuntimeError */
#define SD_ROW_NOISE_OVERRUN  0x80  /* STREAM noise buffer too short                           */
#define SD_ROW_NUCLEUS_INEXACT 0x100 /* nucleus cut computed where fp32 cumsum rounding could not
                                       be reproduced exactly           */
#define SD_ROW_EXCHANGE_TIMEOUT 0x200 /* a workgroup's partial never arrived within the bounded
                                       wait of an in-launch exchange (k_draw_lean); the row's
                                       outputs are invalid (also flagged SD_ROW_INVALID_DIST)    */
/* The bits that make a row's outputs unusable: the reference raises in these cases (torch.multinomial
 * on NaN / inf / zero mass, engine/infer_engine.py:246,321-325; sampling/speculative_decoding.py:171),
 * so callers must treat them as errors, never as tokens.  Every entry point that takes a
 * `status_or` word ORs the error bits of each of its rows into it (one device atomic per failed
 * row; nothing on the success path), so a decode loop can test ONE word where it already syncs. */
#define SD_ROW_ERROR_MASK (SD_ROW_INVALID_DIST | SD_ROW_NOISE_OVERRUN | SD_ROW_EXCHANGE_TIMEOUT)

/* A top-k / nucleus row's keep predicate (the threshold search's result): token j is kept iff
 * x_j > tau || (x_j == tau && j <= tie_idx), x_j the row's logit (tau = -inf, tie_idx = INT_MAX
 * keeps all).  flags: SD_ROW_* bits the search raised (SD_ROW_NUCLEUS_INEXACT).  16 bytes.   */
typedef struct sd_row_keep {
    float tau;
    int32_t tie_idx;
    int32_t flags;
    int32_t reserved;
} sd_row_keep;

typedef struct {
    /* shape */
    int32_t batch;               /* B                                                         */
    int32_t gamma;               /* γ' (drafts verified this step), 1..SD_MAX_GAMMA           */
    int32_t vocab;               /* V                                                         */
    int32_t rule;                /* sd_rule                                                   */

    /* target logits: rows t = 0..gamma (gamma+1 rows; row gamma is the bonus row, read only
       under SD_RULE_SPEC).  Row t of sequence b is target_rows[t] + b * target_stride_b.     */
    const void* target_rows[SD_MAX_GAMMA + 1];
    int64_t target_stride_b;
    int32_t target_dtype;        /* sd_dtype                                                  */

    /* drafter: rows d = 0..gamma-1; logits (processed with draft_proc) or, when
       draft_is_probs, fp32 probabilities (the reference's q buffer).                         */
    const void* draft_rows[SD_MAX_GAMMA];
    int64_t draft_stride_b;
    int32_t draft_dtype;
    int32_t draft_is_probs;

    const int64_t* draft_tokens; /* [B, >=gamma] drafted ids                                  */
    int64_t draft_tokens_stride_b;

    sd_processor target_proc;    /* SPEC: the loop's logits_processor; ENGINE: plain softmax  */
    sd_processor draft_proc;

    int32_t skip_sample_adjustment;  /* SPEC: sample from p_n instead of max_fn(p_n - q_n)    */
    const int64_t* stop_tokens;      /* device [n_stop] eos ids (SPEC stop scan / ENGINE end)  */
    int32_t n_stop;

    const uint8_t* active;       /* ENGINE: [B] rows still generating (nullable = all)        */

    sd_noise noise;

    /* outputs, device, [B] */
    int32_t* n_accepted;         /* accepted drafts n                                         */
    int64_t* next_token;         /* token written at position cur+n (-1 if none)              */
    float* resample_mass;        /* Σ (p_n - q_n)+ when a residual was formed, else NaN        */
    int32_t* prune_drafter;      /* SPEC: γ'-n on reject, else 0 (utils/caching.py input)      */
    int32_t* prune_target;       /* SPEC: γ'-n+1 on reject, else 0                            */
    int32_t* stop_index;         /* SPEC: draft position of the first accepted stop token, -1  */
    int32_t* row_status;         /* SD_ROW_* bits                                             */
    int64_t* words_used;         /* STREAM: [1] words consumed by this call (nullable)         */

    /* optional in-place engine state (ENGINE rule; nullable): applies
       engine/infer_engine.py:307-336 on the device — generated[b, step+n] = x on reject,
       zero the tail, finished[b] |= end token, accepted[b] += n.                             */
    int64_t* generated;          /* [B, gen_len]                                              */
    int64_t generated_stride_b;
    int32_t step;
    uint8_t* finished;           /* [B]                                                       */
    int64_t* accepted_count;     /* [B]                                                       */

    void* workspace;
    size_t workspace_bytes;

    /* optional instrumentation: hipEvent_t recorded on `stream` right before / after the
       row-statistics kernel (the pass that reads every logit row once); nullable.  With the
       events set, the kernel is launched prof_stats_repeat (>= 1) times between them, back to
       back (every repeat rewrites the same partials and decisions), so the event pair's own
       cost is amortised over the repeats.                                                   */
    void* prof_stats_begin;
    void* prof_stats_end;
    int32_t prof_stats_repeat;

    /* optional (nullable): (max, Σexp) of each processed drafter row as sd_sample returned it
       with the draw (sd_sample_args.row_stats), pairs of floats; row d of sequence b at
       draft_row_stats + 2 * (d * draft_row_stats_stride + b), stride >= batch.  With it the
       row-statistics pass reads only the target rows — the drafter rows were read by their
       draws (sampling/speculative_decoding.py:120-123, engine/infer_engine.py:241-247) — and
       the residual still reads drafter row n.  A hint: ignored with draft_is_probs or a
       top-k / nucleus drafter processor.                                                      */
    const float* draft_row_stats;
    int64_t draft_row_stats_stride;
    /* optional (nullable, read only with draft_row_stats): the keep predicates of a top-k /
       nucleus drafter's rows as sd_sample returned them with the draws (sd_sample_args.row_keep),
       at draft_row_stats' layout: row d of sequence b at draft_row_keep[d * stride + b].  With
       both, the drafter rows are neither re-read for their statistics nor re-searched for their
       thresholds: the keep is a function of the row and draft_proc alone, so the draw's equals
       the one the verify would compute (utils/logits_processor.py:52-101).                    */
    const struct sd_row_keep* draft_row_keep;
    /* optional (nullable): device int32 [1]; the call ORs every row's SD_ROW_ERROR_MASK bits into
       it (never cleared by the library: the caller zeroes it, e.g. once per decode loop)        */
    int32_t* status_or;
    /* optional (nullable): device int64 [B, 2]; the call ADDS (accepted drafts n, tokens emitted)
       to row b's pair — emitted = n plus the resampled / bonus token when one was drawn.  The
       acceptance / throughput bookkeeping (engine/infer_engine.py:258,308; engine/metrics.py:100-129)
       kept on the device with no extra launch.                                                  */
    int64_t* row_counts;
} sd_verify_args;

typedef struct {
    int32_t rows;                /* R rows sampled independently                               */
    int32_t vocab;
    const void* logits;          /* row r at logits + r * stride_r                            */
    int64_t stride_r;
    int32_t dtype;
    sd_processor proc;
    sd_noise noise;              /* STREAM: torch.multinomial on [R, V]: 2 words per element   */
    int64_t* tokens;             /* [R] sampled ids (token r at tokens[r * tokens_stride])     */
    int64_t tokens_stride;
    float* token_prob;           /* [R] processed probability of the sampled id (nullable)     */
    int32_t* row_status;         /* [R] (nullable)                                             */
    int64_t* words_used;         /* [1] (nullable)                                             */
    void* workspace;
    size_t workspace_bytes;
    float* row_stats;            /* [R][2] (max, Σexp) of each processed row, the softmax
                                    normaliser pair sd_verify takes as draft_row_stats (nullable).
                                    PHILOX stochastic rows: ONE pass (k_draw) — each span draws
                                    its own candidate, the row's last workgroup picks the span  */
    struct sd_row_keep* row_keep; /* [R] keep predicate of each row under a top-k / nucleus
                                    processor, the input sd_verify takes as draft_row_keep
                                    (nullable; not written for other processors)               */
    int32_t* status_or;          /* [1] (nullable): every row's SD_ROW_ERROR_MASK bits ORed in    */
} sd_sample_args;

/* LogitsProcessor.__call__ (utils/logits_processor.py:13-15) materialised: probs = softmax(_process(l)/T)
 * in the logits dtype, row r written at probs + r * probs_stride_r.                        */
typedef struct {
    int32_t rows;
    int32_t vocab;
    const void* logits;
    int64_t stride_r;
    int32_t dtype;
    sd_processor proc;
    void* probs;
    int64_t probs_stride_r;
    void* workspace;
    size_t workspace_bytes;
} sd_probs_args;

int32_t sd_abi_version(void);
const char* sd_status_string(int32_t status);

/* In-launch exchanges.  Several kernels exchange per-row partials inside ONE launch by polling
 * tagged records ("poll mode"; k_draw_lean, k_draw_nuc, k_thr_hist, the k_stats / k_sample tails)
 * when the host's occupancy check says the whole grid is resident.  A grid that shares the GPU
 * with other work (another process, RCCL kernels, a side stream) may not be: the bounded polls
 * then flag rows SD_ROW_EXCHANGE_TIMEOUT.  allow_poll = 0 selects the arrival-counter exchanges
 * everywhere (no kernel waits on another workgroup); 1 (default) lets the occupancy check decide.
 * spin_limit bounds every poll in MICROSECONDS OF WALL CLOCK (ABI 11; the device's constant
 * 100 MHz s_memrealtime): 0 = the default 2,000,000 (2 s), < 0 = give up at once — a test hook
 * that forces the timeout path.  A grid that shares the GPU with a long kernel of another stream
 * therefore waits for that kernel (its producers are dispatched in order behind it) instead of
 * flagging rows; only a record that never comes costs the bound.  Process-wide; the environment
 * variables SD_POLL (0/1) and SD_POLL_SPIN_LIMIT set the initial values.                       */
int32_t sd_set_poll_policy(int32_t allow_poll, int32_t spin_limit);
int32_t sd_get_poll_policy(int32_t* allow_poll, int32_t* spin_limit);
const char* sd_last_hip_error(void);   /* hipGetErrorString of the last failed launch (this thread) */

/* Dispatch options (ABI 10, 11): switches between kernel paths that compute the same outputs, for
 * A/B runs and for tests that compare the paths.  Process-wide, set by the caller; no entry point
 * reads the environment (SD_POLL / SD_POLL_SPIN_LIMIT seed the poll policy once, at first use).
 * sd_set_option returns SD_ERR_INVALID for an unknown option or value.                        */
typedef enum {
    SD_OPT_FUSED_VERIFY = 1,    /* 1 (default): k_verify_fused for B >= 8; 2: any B; 0: never.
                                   Whatever the value, only calls with at most 17 target rows
                                   (gamma <= 16 under SD_RULE_SPEC, <= 17 under SD_RULE_ENGINE):
                                   longer windows take k_stats + k_sample                         */
    SD_OPT_LEAN_VERIFY = 2,     /* -1 (default): k_verify_lean for <= 8 sequences; 1: any batch
                                   the occupancy check admits; 0: never.  Whatever the value, only
                                   gamma <= 8 and 16-byte aligned 16-bit rows                     */
    SD_OPT_THRESHOLD_POLL = 3,  /* 1 (default): the top-k / nucleus search in one launch when its
                                   grid is resident; 0: the launch-per-phase design               */
    SD_OPT_DRAW_STREAM = 4,     /* 1 (default): STREAM multinomial draws in one pass
                                   (k_draw_stream); 0: statistics + race + finalize launches      */
    SD_OPT_FUSED_TICKET = 5,    /* ABI 11. -1 (default): k_verify_fused in ticket order (work items
                                   by arrival ticket: any batch, resident or not) for B >= 64 or a
                                   grid too big to be resident; 0: block-id order only (a grid
                                   that is not resident takes k_stats + k_sample); 1: always      */
    SD_OPT_DRAW_SPAN = 6,       /* ABI 11. 0 (default): k_draw_lean's span per workgroup chosen by
                                   the batch (2048 elements, more for large batches); 1 / 2 / 4:
                                   that many 2048-element stages per workgroup                    */
    SD_OPT_TICKET_LAG = 7,      /* ABI 11. 0 (default, 1): in the ticket-order fused verify, how many
                                   sequences of a label stream before an earlier one's samplers  */
    SD_OPT_SAMP_CHUNKS = 8,     /* ABI 11. 0 (default: 2, 4 in ticket order): 2048-element chunks each
                                   sampling workgroup of the fused verify draws; 2, 4 or 8 pin it
                                   (the same chunks and draws whatever the grouping)              */
    SD_OPT_ARG_FAST = 9,        /* 1 (default): k_verify_fused in block-id order forms its row
                                   addresses from leading (preloaded) kernel parameters when the
                                   target rows are equally spaced; 0: always from the row table
                                   (A/B, tests; the same results)                                 */
} sd_option;
int32_t sd_set_option(int32_t option, int32_t value);
int32_t sd_get_option(int32_t option, int32_t* value);

/* The kernel path the CALLING THREAD's last successful sd_verify / sd_sample took (so a test or a
 * bench can tell which kernel it measured without reading the dispatch rules).                 */
typedef enum {
    SD_PATH_NONE = 0,
    SD_PATH_VERIFY_LEAN = 1,        /* k_verify_lean: one launch, <= 8 sequences, gamma <= 8     */
    SD_PATH_VERIFY_FUSED = 2,       /* k_verify_fused: one launch, <= 17 target rows              */
    SD_PATH_VERIFY_TWO_LAUNCH = 3,  /* k_stats (+ decider) then k_sample                          */
    SD_PATH_VERIFY_STREAM = 4,      /* STREAM: k_stats, k_decide, k_walk, k_resample, k_finalize  */
    SD_PATH_VERIFY_FUSED_TICKET = 5,/* k_verify_fused in ticket order (ABI 11): one launch, any B  */
    SD_PATH_VERIFY_MULTI = 6,       /* sd_verify_multi: k_stats, k_multi_mass x (K+1), k_multi_walk */
    SD_PATH_VERIFY_VP = 7,          /* sd_vp_finish: the vocabulary-parallel step's last phase    */
    SD_PATH_VERIFY_TREE = 8,        /* sd_verify_tree: k_stats, k_tree_mass x (C_max+1), k_tree_walk */
    SD_PATH_VERIFY_TREE_DISTINCT = 9,   /* sd_verify_tree_distinct: k_stats, k_treed_rowsum, k_treed_walk */
    SD_PATH_VERIFY_TREE_DYNAMIC = 10,   /* sd_verify_tree_dynamic: the distinct kernels, device parents      */
    SD_PATH_VERIFY_BLOCK = 11,      /* sd_verify_block: k_stats, k_block_mass, k_block_walk            */
    SD_PATH_SAMPLE_DRAW_LEAN = 16, /* k_draw_lean (PHILOX multinomial, T = 1, 16-bit)           */
    SD_PATH_SAMPLE_DRAW = 17,       /* k_draw (PHILOX, processors / fp32)                          */
    SD_PATH_SAMPLE_NUCLEUS = 18,    /* k_draw_nuc (PHILOX nucleus by rejection)                    */
    SD_PATH_SAMPLE_STREAM = 19,     /* k_draw_stream (STREAM one pass)                             */
    SD_PATH_SAMPLE_GREEDY_LEAN = 20,/* k_draw_lean<GREEDY>                                          */
    SD_PATH_SAMPLE_MULTI = 21,      /* row statistics + k_rowsample + k_sample_finalize            */
} sd_path;
int32_t sd_last_verify_path(void);
int32_t sd_last_sample_path(void);

/* Workspaces: device memory of at least sd_*_workspace_size bytes, ZERO-FILLED ONCE when
 * allocated (hipMemset).  Its first block holds per-sequence arrival counters that the PHILOX
 * verify path uses to run each sequence's decision / sampling in the last workgroup to finish;
 * every call leaves them at zero again, so one workspace can serve any sequence of
 * sd_verify / sd_sample / sd_probs calls on one stream (not concurrent calls).
 * PHILOX verify supports batch <= 16384 per call (SD_ERR_UNSUPPORTED beyond).
 *
 * PHILOX sampling draws the residual / bonus / p-row token by inverse CDF on one Philox U[0,1)
 * (53 bits) per row: distributionally the reference's multinomial, not its bit stream.  Greedy
 * rows are bit-exact in both noise modes; STREAM mode reproduces torch's CPU draws exactly.  */
size_t sd_verify_workspace_size(int32_t batch, int32_t gamma, int32_t vocab);
int32_t sd_verify(const sd_verify_args* args, void* stream);

size_t sd_sample_workspace_size(int32_t rows, int32_t vocab);
int32_t sd_sample(const sd_sample_args* args, void* stream);

size_t sd_probs_workspace_size(int32_t rows, int32_t vocab);
int32_t sd_probs(const sd_probs_args* args, void* stream);

/* The n-gram-assisted verify step (rule A11, ngram_assisted/ngram_assisted.py:111-164): sample-
 * and-compare of γ' drafts against the processed target rows, then an independent draw x from the
 * mismatch row (or the bonus row), no residual.  STREAM noise follows the reference's draw order
 * (one full-row Exp draw per compare sample, then x: words_used = draws × 2V); filler ids =
 * topk(filler_k) of every processed row (lowest index first among equal probabilities).        */
typedef struct {
    int32_t batch;               /* B (the reference is batch 1)                               */
    int32_t gamma;               /* γ' drafts, 0..SD_MAX_GAMMA                                  */
    int32_t vocab;
    const void* target_rows[SD_MAX_GAMMA + 1];   /* rows 0..γ'-1 verify draft i, row γ' = bonus */
    int64_t target_stride_b;
    int32_t target_dtype;
    const int64_t* draft_tokens; /* [B, >=γ']                                                  */
    int64_t draft_tokens_stride_b;
    sd_processor proc;           /* the loop's logits_processor                                */
    const int64_t* stop_tokens;
    int32_t n_stop;
    int32_t filler_k;            /* 0..vocab (ABI 11; p.topk(filler_top_k), any k)             */
    sd_noise noise;
    /* outputs, device */
    int32_t* n_accepted;         /* [B] n                                                      */
    int64_t* next_token;         /* [B] x, -1 when a stop token among the accepted drafts ends  */
    int32_t* prune_target;       /* [B] γ'-n+1 on a mismatch (:139-141), else 0                 */
    int32_t* stop_index;         /* [B] first accepted stop draft, -1                           */
    int32_t* row_status;         /* [B] SD_ROW_* (BONUS: x from the bonus row; FALLBACK_P: p_n) */
    int64_t* words_used;         /* [1] STREAM words consumed (batch 1 semantics)               */
    int64_t* filler_ids;         /* [B, γ'+1, filler_k] at + b * filler_stride_b + i * filler_k */
    int64_t filler_stride_b;
    void* workspace;
    size_t workspace_bytes;
    int32_t* status_or;          /* [1] (nullable): every row's SD_ROW_ERROR_MASK bits ORed in    */
} sd_ngram_args;

size_t sd_ngram_workspace_size(int32_t batch, int32_t gamma, int32_t vocab);
int32_t sd_ngram_verify(const sd_ngram_args* args, void* stream);

/* Device n-gram drafter store under the reference's OneLevelNGramStorage /
 * NGramStorage (ngram_assisted/ngram_storage.py:71-249): initialize / update / next_token /
 * has_gram keep their meaning; the host keeps the record clock (ts) and the fallback draws.
 *   sd_ngram_store_initialize  replaces ngram_storage.py:128-142 (one level), 227-243 (all orders)
 *   sd_ngram_store_update      replaces ngram_storage.py:106-126, 196-217
 *   sd_ngram_store_next_token  replaces ngram_storage.py:76-90, 162-177 (out[] holds the caller's
 *                              torch.randint fallback draws on entry, overwritten for known grams)
 *   sd_ngram_store_has_gram    replaces ngram_storage.py:92-102, 179-194 (writes 0/1 to *out)
 *   sd_ngram_store_draft       replaces the loop's gamma chained next_token calls
 *                              (ngram_assisted/ngram_assisted.py:94-101): drafts[b, k] and known[b, k]
 *                              (known: [B, gamma] contiguous) for the history extended by drafts
 *                              0..k-1; fallback[b, k] = the k-th call's torch.randint draw
 * Records are stamped ts = ts_base + their index in the reference's processing order (initialize:
 * b * len + i; update: b * k + j); the caller advances ts_base by batch * len / batch * k after
 * each call.  Tables: caller-owned device memory, zero-filled once, capacities powers of two.
 * Token ids must lie in [0, 2^17), n in [2, SD_NGRAM_MAX_N]; a full table or a bad token sets a
 * bit in *status (the call still returns SD_OK: the condition is found on the device) and the
 * record is dropped.
 * Two limits the reference (Python ints) does not have:
 *   - the record clock: ts_base + the call's records must stay <= 2^27-1, so a store takes
 *     2^27-1 records between resets; the call that would pass it returns SD_ERR_UNSUPPORTED and
 *     records nothing.
 *   - the best key's count field has 20 bits: the count placed in it is clamped to 2^20-1
 *     (pair_count keeps counting) and SD_NGRAM_SATURATED is set when a pair reaches the clamp.
 *     Until then the best token is the reference's; among tokens of one gram that all reached the
 *     clamp it is the one with the earliest latest-ts (the first to get there, call by call),
 *     where the reference would go on comparing counts.
 * SD_NGRAM_SATURATED is an additive constant (no layout change): ABI 12.                         */
#define SD_NGRAM_MAX_N 4
#define SD_NGRAM_FULL 1
#define SD_NGRAM_BAD_TOKEN 2
#define SD_NGRAM_SATURATED 4     /* a (gram, token) count reached 2^20-1, the best key's clamp   */
typedef struct {
    uint64_t* gram_keys;         /* [gram_capacity] 0 = empty                                   */
    uint64_t* gram_best;         /* [gram_capacity] min(count,2^20-1)<<44 | (2^27-1-ts)<<17 | token */
    int64_t gram_capacity;
    uint64_t* pair_keys;         /* [pair_capacity] (gram slot, token)                            */
    uint32_t* pair_count;        /* [pair_capacity]                                               */
    uint32_t* pair_ts;           /* [pair_capacity] latest record ts                              */
    int64_t pair_capacity;
    int32_t* status;             /* [1] SD_NGRAM_* bits                                           */
    int32_t n;                   /* the reference's n                                             */
    int32_t one_level;           /* 1: OneLevelNGramStorage, 0: NGramStorage                      */
    int32_t vocab;               /* <= 2^17                                                       */
} sd_ngram_store;

int32_t sd_ngram_store_initialize(const sd_ngram_store* store, const int64_t* ids, int32_t batch, int32_t len,
                                  int64_t stride_b, int64_t ts_base, void* stream);
int32_t sd_ngram_store_update(const sd_ngram_store* store, const int64_t* ids, int32_t batch, int32_t len,
                              int64_t stride_b, const int64_t* next_tokens, int32_t k, int64_t next_stride_b,
                              int64_t ts_base, void* stream);
int32_t sd_ngram_store_next_token(const sd_ngram_store* store, const int64_t* ids, int32_t batch, int32_t len,
                                  int64_t stride_b, int64_t* out, uint8_t* known, void* stream);
int32_t sd_ngram_store_draft(const sd_ngram_store* store, const int64_t* ids, int32_t batch, int32_t len,
                             int64_t stride_b, int32_t gamma, const int64_t* fallback, int64_t fallback_stride_b,
                             int64_t* drafts, int64_t drafts_stride_b, uint8_t* known, void* stream);
int32_t sd_ngram_store_has_gram(const sd_ngram_store* store, const int64_t* ngram, int32_t len, uint8_t* out,
                                void* stream);

/* Host side: torch CPU generator state (torch.Generator.get_state(), 5056 bytes) <-> words. */
int32_t sd_mt19937_fill(const uint8_t* torch_state, size_t state_len, uint32_t* out, int64_t n);
int32_t sd_mt19937_advance(uint8_t* torch_state, size_t state_len, int64_t n);

/* ---- STREAM noise generated on the device (csrc/mt_device.hip, csrc/mt_jump.cpp) ----------------
 * The same words as sd_mt19937_fill, produced by the GPU: the generator state lives in device
 * memory as an sd_mt_state (the current 624-word block of untempered words and the position tau0
 * in [0, 624] of the next word to consume; tau0 = 624 means the next word starts a new block).
 * sd_mt19937_generate writes the next n words (tempered, as torch.rand / exponential_ read them)
 * WITHOUT moving the state; sd_mt19937_commit then moves it past the words a consumer used — a
 * host count, or the device int64 a verify kernel wrote to words_used (no host sync).  A fill is
 * cut into substreams of stride_words words; substream s >= 1 starts at a jump of s*stride_words
 * words, given by jump polynomial s-1 of a table from sd_mt19937_jump_table (host; copy it to the
 * device once per stride).  Replaces the host-thread generation behind torch.rand
 * (sampling/speculative_decoding.py:139, engine/infer_engine.py:305) and torch.multinomial's
 * Exp(1) noise (utils/logits_processor.py:48-49, engine/infer_engine.py:246,322-324). */
#define SD_MT_JUMP_WORDS 320   /* uint64 per jump polynomial (degree < 19937, zero-padded)        */
#define SD_MT_JUMP_CHUNKS 16   /* polynomial bit chunks per jump (one wave each)                 */

typedef struct {
    uint32_t mt[624];      /* the current block x[624 b .. 624 b + 623], untempered               */
    int32_t tau0;          /* next word = x[624 b + tau0]; 624: the next word starts block b + 1   */
    int32_t reserved[3];
} sd_mt_state;

typedef struct {
    sd_mt_state* state;          /* device                                                     */
    const uint64_t* jump_table;  /* device, jump_count * SD_MT_JUMP_WORDS                     */
    int32_t jump_count;          /* >= ceil(n_words / stride_words) - 1                       */
    int64_t stride_words;        /* >= 624; the table's stride                                */
    uint32_t* words;             /* device out, n_words                                      */
    int64_t n_words;
    void* workspace;             /* device, sd_mt19937_generate_workspace_size bytes          */
    size_t workspace_bytes;
} sd_mt_generate_args;

/* host */
int32_t sd_mt19937_state_from_torch(const uint8_t* torch_state, size_t state_len, sd_mt_state* out);
int32_t sd_mt19937_state_to_torch(const sd_mt_state* state, uint8_t* torch_state, size_t state_len);
int32_t sd_mt19937_jump_table(int64_t stride_words, int32_t count, uint64_t* out);  /* count * SD_MT_JUMP_WORDS */
int32_t sd_mt19937_char_poly(uint64_t* out, size_t words);                         /* >= 313 words           */
int32_t sd_mt19937_fill_substreams(const uint32_t* block, int32_t tau0, uint32_t* out, int64_t n,
                                   int64_t stride_words, const uint64_t* table, int32_t count);
/* device.  sd_mt19937_commit moves the state past `used` + *used_dev words (used_dev nullable): a
 * host-known prefix (e.g. the draws of an engine window, 2·B·V words each) plus the count a verify
 * wrote on the device.                                                                           */
size_t sd_mt19937_generate_workspace_size(int64_t n_words, int64_t stride_words);
int32_t sd_mt19937_generate(const sd_mt_generate_args* args, void* stream);
int32_t sd_mt19937_commit(sd_mt_state* state, const uint32_t* words, int64_t n_words, const int64_t* used_dev,
                          int64_t used, int32_t* status, void* stream);

/* ---- Beam search step (ABI 12; csrc/beam.hip) ----------------------------------------------------
 * One step of sampling/base_decoding.py:68-187 (beam_search_generate) on the device:
 *   row pass   (k_beam_topk)    log_softmax + topk of the logit rows (:127-128, :136-137): every row is
 *                               read once; per row the K best log-probs, in the logits dtype (fp32
 *                               internally, the value rounded to bf16 / fp16 when the rows are), VALUE
 *                               DESCENDING, INDEX ASCENDING among equal values (torch.topk leaves the
 *                               order of equal values undefined; see DESIGN.md, beam step).
 *   selection  (k_beam_select)  the candidate loop, dedupe, stable sort and state update (:138-178),
 *                               including the reference's aliasing of a finished beam's score and last
 *                               index (0-dim views, updated in beam order); one workgroup, a second
 *                               launch.  SD_BEAM_PREFILL applies :129-131 instead.
 * No workgroup waits on another (arrival counters only), so a step may be captured into a hipGraph
 * and may share the GPU.  State is ping-pong: the step reads the `_in` buffers and writes the `_out`
 * buffers (rows are permuted), which must not overlap.  NaN logits are out of scope (the order of
 * NaN candidates is unspecified).  vocab <= SD_BEAM_MAX_VOCAB.                                        */
#define SD_BEAM_MAX_BEAMS 64
#define SD_BEAM_MAX_TOPK 64
#define SD_BEAM_MAX_CANDIDATES 1024   /* num_beams * top_k of a SD_BEAM_STEP (the selection's entries) */
#define SD_BEAM_MAX_VOCAB 524288      /* 256 spans of 2048 elements per row */

typedef enum {
    SD_BEAM_PREFILL = 0,   /* one logit row, K = num_beams: the first generated position (:123-131)   */
    SD_BEAM_STEP = 1,      /* num_beams logit rows, K = top_k: one loop iteration (:133-183)           */
    SD_BEAM_TOPK_ONLY = 2, /* row pass alone over num_beams rows, K = top_k: no state is read or written */
} sd_beam_mode;

#define SD_BEAM_TOPK_GIVEN 0x1   /* flags: skip the row pass; top_logprob / top_token hold the caller's */

typedef struct {
    int32_t mode;                /* sd_beam_mode                                                   */
    int32_t flags;               /* SD_BEAM_*                                                      */
    int32_t num_beams;           /* 1..SD_BEAM_MAX_BEAMS (TOPK_ONLY: the number of rows)            */
    int32_t top_k;               /* 1..SD_BEAM_MAX_TOPK (ignored by PREFILL)                        */
    int32_t vocab;
    int32_t curr;                /* the position written this step (PREFILL: the prompt length)     */
    int32_t total_len;           /* row length of input_ids / probs                                */
    float lp;                    /* the step's length penalty, (float) of the host's double; the
                                    caller passes 1 where the reference's `lp if lp != 0 else 1` does */
    const void* logits;          /* row r at logits + r * stride_r (PREFILL: one row)               */
    int64_t stride_r;
    int32_t dtype;               /* sd_dtype                                                       */
    int32_t n_stop;
    const int64_t* stop_tokens;  /* [n_stop]                                                       */
    int64_t pad_token;
    /* state in (read) and out (written); rows of input_ids / probs at * stride elements           */
    const int64_t* input_ids_in;
    int64_t* input_ids_out;
    int64_t input_ids_stride;
    const float* probs_in;
    float* probs_out;
    int64_t probs_stride;
    const float* beams_probs_in; /* [num_beams]                                                    */
    float* beams_probs_out;
    const int64_t* last_index_in;/* [num_beams], -1 = live                                         */
    int64_t* last_index_out;
    /* the rows' top-K: [R, K] contiguous (R = 1, K = num_beams under PREFILL; else R = num_beams,
       K = top_k); written by the row pass, read by the selection (SD_BEAM_TOPK_GIVEN: only read)   */
    float* top_logprob;          /* fp32 holding the dtype-rounded value                            */
    int64_t* top_token;
    int32_t* all_finished;       /* [1]: 1 when every last_index_out != -1, else 0; -1 when fewer
                                    candidates than beams survived the dedupe (the reference raises) */
    int32_t* parent;             /* nullable [num_beams, 2]: per output slot the source beam and the
                                    candidate index (-1 for a finished beam carried over)           */
    /* device memory of at least sd_beam_workspace_size bytes, ZERO-FILLED ONCE when allocated; not
       read under SD_BEAM_TOPK_GIVEN (nullable then).  It follows the workspace convention of the
       other entry points: the row pass's arrival counters lie inside the common counter block at
       the front (sequence counters 0..rows-1) and are zero again when the call's kernels end, its
       partials lie behind that block.  One workspace may therefore serve any sequence of
       sd_beam_step / sd_verify / sd_sample / sd_probs / sd_ngram_verify calls on one stream (not
       concurrent calls).                                                                          */
    void* workspace;
    size_t workspace_bytes;
} sd_beam_args;

/* rows / k as the row pass sees them (PREFILL: 1, num_beams).  0 for a bad shape.                    */
size_t sd_beam_workspace_size(int32_t rows, int32_t vocab, int32_t k);
int32_t sd_beam_step(const sd_beam_args* args, void* stream);

/* ---- Multi-draft speculative verification (csrc/sd_verify_multi.inc; additive, ABI 12) -----------
 * One verify step over K independently drafted chains per sequence (SpecInfer's multi-step
 * speculative sampling / recursive rejection sampling): the walk over the prefix tree of the chains
 * that keeps the emitted tokens distributed exactly as the target's.  Chain k of sequence b is row
 * b*K + k of every row set.  Probabilities are SD_RULE_SPEC's (processor, temperature, rounded to
 * the rows' dtype); target and drafter rows share ONE processor and one dtype.  Per sequence:
 *
 *   A = {0..K-1}                                   alive chains (they share the accepted prefix)
 *   for d in 0..γ'-1:
 *       k0 = min A;  p = P(target row d of chain k0);  q = P(drafter row d of chain k0);  r = p
 *       for k in A ascending:
 *           x = tok[k, d];  u = accept uniform d*K + k
 *           if not (u > r[x] / q[x]): hit = x, stop testing          (fp32, as SD_RULE_SPEC)
 *           m = Σ_v max(r[v] - q[v], 0);  r = max(r - q, 0) / m      (one more sibling rejected)
 *       no hit: n = d, x ~ r, SD_ROW_RESIDUAL, winner = k0, done
 *       A = {k in A : tok[k, d] == hit}
 *   n = γ', x ~ P(bonus row of chain min A), SD_ROW_BONUS, winner = min A
 *
 * then the stop scan over tok[winner, :n] (SD_ROW_STOP_IN_DRAFTS, stop_index, no token drawn) and the
 * prune lengths, as sd_verify.  Noise is SD_NOISE_PHILOX only (SD_NOISE_STREAM: SD_ERR_UNSUPPORTED):
 * sequence b is row row_base + b, the accept uniform of (d, k) is the row's accept uniform number
 * d*K + k, the sample is drawn by inverse CDF on the row's cdf uniform; one call consumes one offset,
 * so K = 1 tests and walks exactly as sd_verify(SD_RULE_SPEC) does.
 * Kernels: the row statistics of all K(2γ'+1) rows per sequence, then K + 1 launches that form the
 * residual masses m_1..m_K of every (chain, depth) row pair, then one launch that walks and samples.
 * No workgroup waits on another (launch boundaries only): capturable, safe on a shared GPU.       */
#define SD_MULTI_MAX_DRAFTS 8      /* K                                                              */
#define SD_MULTI_MAX_NODES 64      /* K * γ'                                                         */
#define SD_MULTI_MAX_ROWS 16384    /* B * K                                                          */

typedef struct {
    int32_t batch;               /* B                                                              */
    int32_t num_drafts;          /* K, 1..SD_MULTI_MAX_DRAFTS                                       */
    int32_t gamma;               /* γ', 1..SD_MAX_GAMMA, K * γ' <= SD_MULTI_MAX_NODES               */
    int32_t vocab;
    /* rows over the chain axis r = b*K + k: target row t at target_rows[t] + r * target_stride_r
       (t = γ' is the bonus row), drafter row d at draft_rows[d] + r * draft_stride_r               */
    const void* target_rows[SD_MAX_GAMMA + 1];
    int64_t target_stride_r;
    int32_t target_dtype;        /* sd_dtype                                                       */
    const void* draft_rows[SD_MAX_GAMMA];
    int64_t draft_stride_r;
    int32_t draft_dtype;         /* must equal target_dtype (SD_ERR_UNSUPPORTED otherwise)          */
    const int64_t* draft_tokens; /* [B*K, >=γ'] drafted ids                                         */
    int64_t draft_tokens_stride_r;
    sd_processor proc;           /* the loop's logits_processor, for target and drafter rows       */
    const int64_t* stop_tokens;  /* device [n_stop]                                                */
    int32_t n_stop;
    int64_t pad_token;           /* fills tokens_out past the emitted tokens                        */
    sd_noise noise;              /* SD_NOISE_PHILOX                                                */

    /* outputs, device, [B] */
    int32_t* n_accepted;         /* accepted depth n                                               */
    int32_t* winner;             /* the chain whose first n drafts were accepted (see above)        */
    int64_t* next_token;         /* x, -1 if none (stop token among the accepted drafts)            */
    float* resample_mass;        /* mass m of the last residual formed, NaN if none (nullable)      */
    int32_t* n_sibling_rejects;  /* accept tests that failed (nullable)                             */
    int32_t* prune_drafter;      /* γ'-n on a residual exit, else 0 (nullable)                      */
    int32_t* prune_target;       /* γ'-n+1 on a residual exit, else 0 (nullable)                    */
    int32_t* stop_index;         /* position of the stop token in tok[winner, :n], -1 (nullable)    */
    int32_t* row_status;         /* SD_ROW_* bits                                                  */
    /* optional (nullable): int64 [B, >=γ'+1] at tokens_out + b * tokens_out_stride_b: tok[winner, :n],
       then x (when one was drawn), then pad_token up to γ'+1 entries                               */
    int64_t* tokens_out;
    int64_t tokens_out_stride_b;

    void* workspace;             /* sd_verify_multi_workspace_size bytes, zero-filled once; shares
                                    the other entry points' convention (counter block left at zero) */
    size_t workspace_bytes;
    /* optional hints (nullable), as sd_verify's: (max, Σexp) and keep predicates of the drafter rows
       as sd_sample returned them for the B*K rows of each depth: row d of chain r at
       draft_row_stats + 2 * (d * draft_row_stats_stride + r), stride >= B*K; draft_row_keep at the
       same layout, needed with the stats under a top-k / nucleus processor                         */
    const float* draft_row_stats;
    int64_t draft_row_stats_stride;
    const struct sd_row_keep* draft_row_keep;
    int32_t* status_or;          /* nullable: every sequence's SD_ROW_ERROR_MASK bits ORed in       */
} sd_multi_args;

size_t sd_verify_multi_workspace_size(int32_t batch, int32_t num_drafts, int32_t gamma, int32_t vocab);
int32_t sd_verify_multi(const sd_multi_args* args, void* stream);

/* ---- Vocabulary-parallel verify (csrc/vocab_parallel.hip; additive, ABI 12) -----------------------
 * One SD_RULE_SPEC verify step on the logits as a tensor-parallel forward leaves them: S ranks
 * ("shards") 0..S-1, shard s holding columns [off_s, off_s + V_s) of every row, off_0 = 0,
 * off_{s+1} = off_s + V_s, Σ V_s = V, V_s >= 1 (slices may be uneven and may start at any element).
 * γ' is 0..SD_MAX_GAMMA; γ' = 0 samples the one target row.  Probabilities are SPEC's
 * (round_dt(softmax(round_dt(l / T)))); processors SD_PROC_GREEDY and SD_PROC_MULTINOMIAL at any
 * temperature (top-k / nucleus: SD_ERR_UNSUPPORTED); noise SD_NOISE_PHILOX only (STREAM:
 * SD_ERR_UNSUPPORTED); target and drafter rows share one dtype.  Three calls per step, with one
 * all-gather of a few hundred bytes per sequence after each of the first two; logit rows never move:
 *
 *   sd_vp_stats    (m, S = Σ exp(y - m)) over the slice of each of the 2γ'+1 rows of a sequence
 *                  (target rows 0..γ', then drafter rows 0..γ'-1), and the processed logit y of
 *                  tok[d] in target row d and drafter row d where the slice owns tok[d]
 *                  -> stats_local: an sd_vp_header, then sd_vp_stat[B][2γ'+1]
 *   (exchange 1)   all-gather of the S blocks into stats_all, shard-major
 *   sd_vp_decide   every shard alike: the partials of each row merged IN ASCENDING SHARD ORDER by one
 *                  fixed online merge (so all ranks hold bit-identical normalisers and decide alike),
 *                  p(x_d), q(x_d) from the owner's y, SPEC's test on accept uniform d of global row
 *                  row_base + b (sd_verify's uniform: n, the status bits, the stop scan and the prune
 *                  lengths equal sd_verify(SD_RULE_SPEC) on the whole rows up to the rounding of the
 *                  normalisers).  Then, over the shard's own slice, the weights w = (p_n - q_n)+ on a
 *                  reject (p_n with skip_sample_adjustment, the bonus row on full accept): the local
 *                  mass M_s = Σ w (fp32 totals of 2048-element chunks, summed in fp64 in chunk order)
 *                  and the local candidate — stochastic: inverse CDF over the slice on
 *                  u2 = cdf uniform idx 1 of the row; greedy: (max w, lowest global index)
 *                  -> cand_local: an sd_vp_header, then sd_vp_cand[B]
 *   (exchange 2)   all-gather of the S blocks into cand_all
 *   sd_vp_finish   every shard alike.  Stochastic: M = Σ M_s (fp64, shard order; M <= 0 or not finite:
 *                  SD_ROW_INVALID_DIST), the first shard s* with Σ_{s<=s*} M_s > u1 M (u1 = cdf uniform
 *                  idx 0; the last shard with positive mass if rounding runs past the end), x = its
 *                  candidate.  Greedy: the candidate of largest weight, lowest global index among
 *                  equals.  resample_mass = (float)M when a residual was formed, else NaN.
 *
 * P(x = j) = (M_s/M)(w_j/M_s) = w_j/M as u1, u2 are independent Philox blocks: exact.  next_token
 * depends on the sharding; n and the status do not.  One step consumes one Philox offset.  A layout
 * that does not partition [0, V) (a block whose header names another shard, gaps, Σ V_s != V) flags
 * every row SD_ROW_INVALID_DIST.  Launch boundaries are the only synchronisation: capturable, safe
 * on a GPU that collective kernels share.                                                          */
#define SD_VP_MAX_SHARDS 64
#define SD_VP_MAX_BATCH 1024
#define SD_VP_MAX_VOCAB_LOCAL 2097152   /* 1024 chunks of 2048 elements per slice                   */
#define SD_VP_MAGIC 0x53445650          /* "SDVP"                                                   */
#define SD_VP_STAT_OWNS 0x1             /* sd_vp_stat.flags: this slice holds the row's drafted id   */

typedef struct sd_vp_header {           /* 32 bytes: the front of every exchanged block              */
    int32_t magic;                      /* SD_VP_MAGIC                                              */
    int32_t shard, num_shards;
    int32_t vocab_offset, vocab_local, vocab;
    int32_t batch, gamma;
} sd_vp_header;

typedef struct sd_vp_stat {             /* 16 bytes: one per (sequence, row)                         */
    float m;                            /* max of the processed slice (-inf: nothing finite)         */
    float s;                            /* Σ exp(y - m) over the slice                               */
    float y_tok;                        /* processed logit of the row's drafted id (SD_VP_STAT_OWNS) */
    int32_t flags;
} sd_vp_stat;

typedef struct sd_vp_cand {             /* 32 bytes: one per sequence                                */
    double mass;                        /* M_s                                                      */
    int64_t token;                      /* the shard's candidate, a GLOBAL id; -1: none              */
    float weight;                       /* w of the candidate                                        */
    int32_t status;                     /* the decision's SD_ROW_* bits (the same on every shard)    */
    int32_t n_accepted;
    int32_t stop_index;
} sd_vp_cand;

typedef struct {
    int32_t batch;               /* B, 1..SD_VP_MAX_BATCH                                          */
    int32_t gamma;               /* γ', 0..SD_MAX_GAMMA                                            */
    int32_t vocab;               /* V, the whole vocabulary                                        */
    int32_t vocab_offset;        /* off_s                                                          */
    int32_t vocab_local;         /* V_s                                                            */
    int32_t shard;               /* s                                                              */
    int32_t num_shards;          /* S, 1..SD_VP_MAX_SHARDS                                         */
    int32_t dtype;               /* sd_dtype of target and drafter rows                            */
    /* row t of sequence b: element 0 OF THE SLICE at target_rows[t] + b * target_stride_b          */
    const void* target_rows[SD_MAX_GAMMA + 1];
    int64_t target_stride_b;
    const void* draft_rows[SD_MAX_GAMMA];
    int64_t draft_stride_b;
    const int64_t* draft_tokens; /* [B, >=γ'] drafted ids (global); nullable when γ' = 0            */
    int64_t draft_tokens_stride_b;
    sd_processor proc;           /* the loop's logits_processor, for target and drafter rows       */
    int32_t skip_sample_adjustment;
    int32_t n_stop;
    const int64_t* stop_tokens;  /* device [n_stop]                                                */
    sd_noise noise;              /* SD_NOISE_PHILOX                                                */
    /* exchange buffers, device: one block is sd_vp_stats_bytes / sd_vp_cand_bytes bytes; the _all
       buffers hold S blocks, shard-major                                                          */
    void* stats_local;           /* written by sd_vp_stats                                         */
    const void* stats_all;       /* read by sd_vp_decide                                           */
    void* cand_local;            /* written by sd_vp_decide                                        */
    const void* cand_all;        /* read by sd_vp_finish                                           */
    /* outputs of sd_vp_finish, device, [B], as sd_verify's                                        */
    int32_t* n_accepted;
    int64_t* next_token;
    float* resample_mass;        /* nullable                                                       */
    int32_t* prune_drafter;      /* nullable                                                       */
    int32_t* prune_target;       /* nullable                                                       */
    int32_t* stop_index;         /* nullable                                                       */
    int32_t* row_status;
    int32_t* owner_shard;        /* nullable: s*, or the winning shard under greedy; -1: no token  */
    int32_t* status_or;          /* nullable: every row's SD_ROW_ERROR_MASK bits ORed in           */
    void* workspace;             /* sd_vp_workspace_size bytes, zero-filled once; the common counter
                                    block at its front is never written, so one workspace may serve
                                    sd_vp_*, sd_verify, sd_sample, sd_verify_multi and sd_beam_step
                                    calls in any order on one stream                               */
    size_t workspace_bytes;
} sd_vp_args;

/* bytes of ONE shard's block, header included; 0 for a bad shape                                   */
size_t sd_vp_stats_bytes(int32_t batch, int32_t gamma);
size_t sd_vp_cand_bytes(int32_t batch);
size_t sd_vp_workspace_size(int32_t batch, int32_t gamma, int32_t vocab_local);
/* Each call reads only what its phase needs: sd_vp_stats the rows, draft_tokens, stats_local;
 * sd_vp_decide those and stats_all, cand_local, the stop list, the noise; sd_vp_finish cand_all, the
 * noise and the outputs (the rows may be gone).  All three take the workspace.                     */
int32_t sd_vp_stats(const sd_vp_args* args, void* stream);
int32_t sd_vp_decide(const sd_vp_args* args, void* stream);
int32_t sd_vp_finish(const sd_vp_args* args, void* stream);

/* ---- Token-tree speculative verification (csrc/sd_verify_tree.inc; additive, ABI 12) --------------
 * One verify step over a token tree per sequence (SpecInfer / Medusa / EAGLE): N drafted nodes with
 * arbitrary parents, scored by the target in one forward under a tree attention mask.  All B sequences
 * of a call share one topology.  Nodes are 0..N-1; parent[i] is in {-1, 0..i-1}, -1 a child of the root
 * (the last committed token).  Slot 0 is the root, slot i+1 node i.  The target row of slot s is the
 * target's logit row after the path to s (N+1 rows); the drafter row of slot s is needed only where s
 * has children, and the children of a slot must be iid draws from that slot's processed drafter row.
 * Probabilities are SD_RULE_SPEC's (processor, temperature, rounded to the rows' dtype); target and
 * drafter rows share ONE processor and one dtype.  Per sequence:
 *
 *   s = 0; path = []
 *   loop:
 *       C = children of s, ascending node index
 *       if C empty: x ~ P(target row s), SD_ROW_BONUS, stop
 *       p = P(target row s);  q = P(drafter row s);  r = p
 *       for c in C:
 *           x = tok[c];  u = accept uniform number c
 *           if not (u > r[x] / q[x]): path += [c]; s = c + 1; continue the outer loop   (fp32, as SPEC)
 *           m = Σ_v max(r[v] - q[v], 0);  r = max(r - q, 0) / m          (one more sibling rejected)
 *       x ~ r, SD_ROW_RESIDUAL, stop
 *   n = len(path)
 *
 * then the stop scan over the path's tokens (the stop listed first that occurs, at its first position:
 * SD_ROW_STOP_IN_DRAFTS, stop_index, no token drawn, next_token = -1).  Noise is SD_NOISE_PHILOX only
 * (SD_NOISE_STREAM: SD_ERR_UNSUPPORTED): sequence b is row row_base + b, the sample is drawn by inverse
 * CDF on the row's cdf uniform (greedy: the argmax, lowest index first); one call consumes one offset.
 * Out-of-range draft ids, zero or NaN mass (SD_ROW_INVALID_DIST), status_or and resample_mass behave
 * as in sd_verify_multi.  Bad topology (a parent out of range or not below its child's index):
 * SD_ERR_INVALID; more than SD_TREE_MAX_CHILDREN children of one slot, depth above SD_MAX_GAMMA, N above
 * SD_TREE_MAX_NODES or a grid beyond the launch limits: SD_ERR_UNSUPPORTED.
 * Kernels: the row statistics of the N+1 target rows and the I internal drafter rows per sequence, then
 * C_max + 1 launches (C_max the largest child count) that form the residual masses m_1..m_c of every
 * internal slot with c children, then one launch that walks and samples.  No workgroup waits on
 * another (launch boundaries only): capturable, safe on a shared GPU.                               */
#define SD_TREE_MAX_NODES 64       /* N                                                              */
#define SD_TREE_MAX_CHILDREN 8     /* children of one slot                                           */
#define SD_TREE_MAX_BATCH 16384    /* B                                                              */

typedef struct {
    int32_t batch;               /* B                                                              */
    int32_t num_nodes;           /* N, 1..SD_TREE_MAX_NODES                                         */
    int32_t vocab;
    int32_t parent[SD_TREE_MAX_NODES];   /* host: parent[i] in {-1, 0..i-1}; entries from N on unread */
    /* rows by slot: target row of slot s at target_rows[s] + b * target_stride_b, drafter row at
       draft_rows[s] + b * draft_stride_b (entries of leaf slots are ignored and may be null)       */
    const void* target_rows[SD_TREE_MAX_NODES + 1];
    int64_t target_stride_b;
    const void* draft_rows[SD_TREE_MAX_NODES + 1];
    int64_t draft_stride_b;
    int32_t dtype;               /* sd_dtype of every row                                           */
    const int64_t* draft_tokens; /* [B, >=N] the nodes' drafted ids                                 */
    int64_t draft_tokens_stride_b;
    sd_processor proc;           /* the loop's logits_processor, for target and drafter rows       */
    const int64_t* stop_tokens;  /* device [n_stop]                                                */
    int32_t n_stop;
    int64_t pad_token;           /* fills tokens_out past the emitted tokens                        */
    sd_noise noise;              /* SD_NOISE_PHILOX                                                */

    /* outputs, device, [B] */
    int32_t* n_accepted;         /* accepted depth n                                               */
    int32_t* last_node;          /* the deepest accepted node, -1 if none                           */
    int64_t* next_token;         /* x, -1 if none (stop token on the path)                          */
    float* resample_mass;        /* mass m of the last residual formed, NaN if none (nullable)      */
    int32_t* n_sibling_rejects;  /* accept tests that failed (nullable)                             */
    int32_t* stop_index;         /* position of the stop token on the path, -1 (nullable)           */
    int32_t* row_status;         /* SD_ROW_* bits                                                  */
    /* int32 [B, >=depth] at path + b * path_stride_b: the node accepted at each depth, -1 beyond n
       (depth: the tree's, the longest root-to-leaf path in nodes)                                  */
    int32_t* path;
    int64_t path_stride_b;
    /* optional (nullable): int64 [B, >=depth+1] at tokens_out + b * tokens_out_stride_b: the path's
       tokens, then x (when one was drawn), then pad_token up to depth+1 entries                    */
    int64_t* tokens_out;
    int64_t tokens_out_stride_b;

    void* workspace;             /* sd_verify_tree_workspace_size bytes, zero-filled once; shares
                                    the other entry points' convention (counter block left at zero) */
    size_t workspace_bytes;
    int32_t* status_or;          /* nullable: every sequence's SD_ROW_ERROR_MASK bits ORed in       */
} sd_tree_args;

/* 0 for a topology or shape sd_verify_tree does not take                                            */
size_t sd_verify_tree_workspace_size(int32_t batch, int32_t num_nodes, const int32_t* parent, int32_t vocab);
int32_t sd_verify_tree(const sd_tree_args* args, void* stream);

/* ---- Token-tree verification, distinct children (csrc/sd_verify_tree_distinct.inc; additive, ABI 12) --
 * sd_verify_tree asks that the children of a slot be iid draws of the slot's drafter row.  Here they
 * are DISTINCT candidates that depend on the prefix alone, not on this call's noise: the drafter's
 * top-c tokens, as Medusa and EAGLE draft them.  No drafter row is read.  Topology, slots, parent[],
 * limits, noise keying (node c takes the row's accept uniform number c, the draw the row's cdf
 * uniform, one call consumes one offset, SD_NOISE_PHILOX only) and the status conventions are
 * sd_verify_tree's.  p_s is the SD_RULE_SPEC probability row of the target row of slot s
 * (round_dt(softmax(round_dt(process(l) / T)))).  Per sequence:
 *
 *   s = 0; path = []
 *   loop:
 *       C = children of s, ascending node index
 *       if C empty: x ~ p_s / Z_s, SD_ROW_BONUS, stop
 *       Z_s = Σ_v p_s[v]      (fp32 sums of 2048-element chunks, added in fp64 in chunk order)
 *       rem = Z_s; excluded = {}
 *       for c in C:
 *           x = tok[c]
 *           w = p_s[x] if 0 <= x < V and x not in excluded else 0
 *           if w > 0 and not (u_c > (float)w / (float)rem): path += [c]; s = c + 1; continue the outer loop
 *           if w > 0: excluded += {x}; rem -= w                                              (fp64)
 *       x ~ (p_s with the excluded tokens zeroed) / rem, SD_ROW_RESIDUAL, stop
 *   n = len(path)
 *
 * A child without weight (an id outside [0, V), a repeat of an earlier sibling, a token the processor
 * cut) is rejected without consulting its uniform.  resample_mass is (float)(rem / Z_s) at a residual
 * exit, NaN otherwise; n_sibling_rejects counts the children rejected.  The stop scan, stop_index,
 * SD_ROW_STOP_IN_DRAFTS (no token drawn), path, last_node, tokens_out and status_or are
 * sd_verify_tree's.  Z_s or rem that is not finite or not positive at the slot drawn from:
 * SD_ROW_INVALID_DIST, next_token = -1.
 * Greedy (SD_PROC_GREEDY): a child with weight is accepted iff the processed logit of its token equals
 * the row maximum (exact: the maximum is an element of the row); the exit token is the argmax of the
 * processed logits, lowest index first.  Where every row maximum is unique the emitted tokens are the
 * target's own greedy decode; a tie at the maximum may resolve toward a drafted child.
 * Lossless: the children do not depend on the verify's noise; child j is accepted with probability
 * w_j / rem_j, so token x_j is emitted with probability (Π_{i<j} (1 - w_i / rem_i)) w_j / rem_j =
 * p[x_j] / Z and any other v with probability (rem_c / Z)(p[v] / rem_c) = p[v] / Z.  A slot accepts
 * with total probability p(C) / Z, the most a set of distinct candidates can reach; sd_verify_tree's
 * Σ min(p, q) per iid draw can be higher (p = q flat) or lower (greedy, peaked drafters): the two are
 * complementary.
 * Kernels: the row statistics of the N+1 target rows, ONE launch that sums every 2048-element chunk
 * of every row, one launch that walks and samples.  Launch boundaries only: capturable.           */
typedef struct {
    int32_t batch;               /* B                                                              */
    int32_t num_nodes;           /* N, 1..SD_TREE_MAX_NODES                                         */
    int32_t vocab;
    int32_t parent[SD_TREE_MAX_NODES];   /* host: parent[i] in {-1, 0..i-1}; entries from N on unread */
    /* target row of slot s at target_rows[s] + b * target_stride_b                                 */
    const void* target_rows[SD_TREE_MAX_NODES + 1];
    int64_t target_stride_b;
    int32_t dtype;               /* sd_dtype of every row                                           */
    const int64_t* draft_tokens; /* [B, >=N] the nodes' drafted ids                                 */
    int64_t draft_tokens_stride_b;
    sd_processor proc;           /* the loop's logits_processor                                     */
    const int64_t* stop_tokens;  /* device [n_stop]                                                */
    int32_t n_stop;
    int64_t pad_token;           /* fills tokens_out past the emitted tokens                        */
    sd_noise noise;              /* SD_NOISE_PHILOX                                                */

    /* outputs, device, [B]: as sd_tree_args'                                                       */
    int32_t* n_accepted;
    int32_t* last_node;
    int64_t* next_token;
    float* resample_mass;        /* (float)(rem / Z) at a residual exit, else NaN (nullable)        */
    int32_t* n_sibling_rejects;  /* children rejected (nullable)                                    */
    int32_t* stop_index;         /* nullable                                                       */
    int32_t* row_status;
    int32_t* path;               /* int32 [B, >=depth] at path + b * path_stride_b                  */
    int64_t path_stride_b;
    int64_t* tokens_out;         /* nullable: int64 [B, >=depth+1]                                  */
    int64_t tokens_out_stride_b;

    void* workspace;             /* sd_verify_tree_distinct_workspace_size bytes, zero-filled once;
                                    shares the other entry points' convention                       */
    size_t workspace_bytes;
    int32_t* status_or;          /* nullable                                                       */
} sd_tree_distinct_args;

/* 0 for a topology or shape sd_verify_tree_distinct does not take                                   */
size_t sd_verify_tree_distinct_workspace_size(int32_t batch, int32_t num_nodes, const int32_t* parent, int32_t vocab);
int32_t sd_verify_tree_distinct(const sd_tree_distinct_args* args, void* stream);

/* ---- KV-cache compaction onto an accepted tree path (csrc/kv_compact.hip; additive, ABI 12) ---------
 * After a tree-masked forward the cache holds the N tree nodes behind the committed tokens, node i at
 * position base + slot(i); sd_verify_tree's `path` names the accepted node of every depth.  One launch
 * moves the accepted rows of ALL K/V tensors (every layer) to the front.  For every tensor t, sequence
 * b, head h and depth d < min(count[b], max_depth), IN ASCENDING d:
 *
 *     src = base_b + slot(path[b][d]);   dst = base_b + d
 *     if src != dst: copy row_bytes bytes from
 *         tensors[t] + b*stride_b + h*stride_h + src*stride_pos   to   ... + dst*stride_pos
 *
 * slot(i) = node_slot[i] when node_slot is given, else i; base_b = base (+ *base_dev when given).
 * The copy is dtype-agnostic (bytes).  In place: slot(path[d]) >= d, so a destination never lies above
 * its source, but depth d's destination may be depth d-1's source.  One thread owns a fixed byte range
 * of one (tensor, b, head) for all depths and walks d upward, so everything written before depth d lies
 * below position base_b + d <= src: no load can read a byte an earlier depth wrote.
 * On the device a path entry outside [0, SD_TREE_MAX_NODES), or a slot outside [d, num_slots), ends
 * that sequence's moves at that depth (-1 beyond n is the normal case); when count[b] says the entry
 * should have been moved, SD_ROW_INVALID_DIST is ORed into status_or.  A base_b with base_b < 0 or
 * base_b + num_slots > num_positions moves nothing and raises the same bit.  Nothing outside positions
 * [base_b, base_b + num_slots) is read or written.  One launch, no workspace, no workgroup waits on
 * another: capturable, safe on a shared GPU.                                                         */
#define SD_KV_MAX_TENSORS 256

typedef struct {
    int32_t n_tensors;           /* 1..SD_KV_MAX_TENSORS                                            */
    int32_t batch;               /* B                                                              */
    int32_t heads;               /* H                                                              */
    int32_t max_depth;           /* 1..SD_MAX_GAMMA: entries of a path row that may be read          */
    int32_t num_slots;           /* 1..SD_TREE_MAX_NODES: positions [base_b, base_b + num_slots)      */
    int32_t row_bytes;           /* head_dim * element size; even                                   */
    void* const* tensors;        /* HOST array of n_tensors device pointers (the K and V buffers of
                                    every layer, one shape); handed to the kernel by value           */
    int64_t stride_b;            /* byte strides of the batch, head and position axes               */
    int64_t stride_h;
    int64_t stride_pos;          /* >= row_bytes                                                    */
    int64_t num_positions;       /* L, positions of a (b, head) row set; >= num_slots                */
    int64_t base;                /* host part of the base position                                  */
    const int64_t* base_dev;     /* nullable: device int64 [1] added to base when the kernel runs
                                    (transformers' StaticLayer.cumulative_length is an int64 tensor) */
    const int32_t* path;         /* device int32 [B, >=max_depth]: sd_verify_tree's output          */
    int64_t path_stride_b;       /* >= max_depth                                                    */
    const int32_t* count;        /* device int32 [B]: usually sd_verify_tree's n_accepted            */
    const int32_t* node_slot;    /* nullable HOST int32 [SD_TREE_MAX_NODES]: node -> cache slot      */
    int32_t* status_or;          /* nullable device int32 [1]                                       */
} sd_kv_compact_args;

int32_t sd_kv_compact(const sd_kv_compact_args* args, void* stream);

/* ---- Dynamic draft trees: growth on the device (csrc/tree_grow.hip; additive, ABI 12) -----------------
 * EAGLE-2 style context-dependent trees without a host read of the drafter's scores.  The host knows
 * only the SHAPE: levels L (1..SD_MAX_GAMMA), width W (1..SD_TREE_GROW_MAX_WIDTH frontier nodes expanded
 * per level), branch c (1..SD_TREE_MAX_CHILDREN, c <= V) and the number of nodes N sent to the target.
 * Frontier sizes are static: F_0 = 1 (the root), F_l = min(W, F_{l-1} * c).  Level l (1-based) adds
 * F_{l-1} * c candidates to the sequence's POOL at indices base_l + r * c + j, base_1 = 0,
 * base_{l+1} = base_l + F_{l-1} * c, r the parent's rank in the previous frontier, j the child's rank.
 * The pool (caller-owned device arrays, <= SD_TREE_POOL_MAX entries per sequence) holds a token, a
 * score (the cumulative drafter log-probability, fp32) and the parent's pool index (-1: the root).
 *
 * sd_tree_grow, one level.  For every frontier row r (the drafter's logit row after frontier node r):
 *   children   the c best tokens by RAW logit, value descending, lowest index first (exact compares)
 *   lp         (x - m) - log(sum exp(x - m)) in fp32, m the row's true maximum, NOT rounded to the
 *              row dtype, clamped to <= 0
 *   score      score(parent) + lp (one fp32 add); the root's score is 0
 * The next frontier is the F_l best candidates OF THIS LEVEL by (score descending, pool index
 * ascending), emitted in ASCENDING POOL INDEX: only membership depends on score arithmetic.  -inf logits
 * give -inf scores: ordinary entries that sort last.  A NaN (or +inf) in a row, a row without a finite
 * element, or an incoming frontier index outside the pool written so far sets SD_ROW_INVALID_DIST for
 * the sequence (row_status, status_or); its outputs are unusable but stay inside its buffers (a NaN
 * score ranks as -inf).  Two launches (every 2048-element chunk of every row read once, then one
 * workgroup per sequence), launch boundaries only: capturable.
 *
 * sd_tree_select, the rerank: the N best pool entries by (score descending, pool index ascending),
 * emitted in ascending pool index.  A child never scores above its parent (lp <= 0) and always has a
 * higher pool index, so the set is closed under parents and parent[i] < i: what sd_verify_tree_dynamic
 * takes.  One launch, one workgroup per sequence.  A selected entry whose parent is not selected (only
 * possible for a pool not written by sd_tree_grow) sets SD_ROW_INVALID_DIST.                          */
#define SD_TREE_POOL_MAX 2048
#define SD_TREE_GROW_MAX_WIDTH 8
#define SD_TREE_GROW_MAX_VOCAB 524288

typedef struct {
    int32_t batch;               /* B, 1..SD_TREE_MAX_BATCH                                         */
    int32_t vocab;               /* V, 1..SD_TREE_GROW_MAX_VOCAB                                     */
    int32_t level;               /* l, 1..SD_MAX_GAMMA: the level this call adds                     */
    int32_t width;               /* W                                                              */
    int32_t branch;              /* c                                                              */
    int32_t dtype;               /* sd_dtype of the rows                                            */
    /* frontier row r of sequence b at logits + (b * stride_b + r * stride_r) elements, r < F_{l-1}   */
    const void* logits;
    int64_t stride_b;
    int64_t stride_r;
    /* device int32 [B, >=F_{l-1}]: the previous call's frontier_pool (ignored and nullable at l = 1) */
    const int32_t* frontier_in;
    int64_t frontier_in_stride_b;
    /* the pool, device, [B, >=base_l + F_{l-1} * c] at stride pool_stride_b                          */
    int64_t* pool_token;
    float* pool_score;
    int32_t* pool_parent;
    int64_t pool_stride_b;
    /* outputs, device, [B, >=F_l] at stride frontier_stride_b                                        */
    int64_t* frontier_token;
    int32_t* frontier_pool;
    int32_t* frontier_parent_rank;   /* rank of the parent in the previous frontier                  */
    int64_t frontier_stride_b;
    int32_t* row_status;         /* nullable, [B]: SD_ROW_DONE, SD_ROW_INVALID_DIST                  */
    int32_t* status_or;          /* nullable                                                       */
    void* workspace;             /* sd_tree_grow_workspace_size bytes; the common convention        */
    size_t workspace_bytes;
} sd_tree_grow_args;

typedef struct {
    int32_t batch;               /* B                                                              */
    int32_t pool_size;           /* entries per sequence, 1..SD_TREE_POOL_MAX                        */
    int32_t num_nodes;           /* N, 1..min(SD_TREE_MAX_NODES, pool_size)                           */
    int32_t reserved;
    const int64_t* pool_token;
    const float* pool_score;
    const int32_t* pool_parent;
    int64_t pool_stride_b;
    /* outputs, device, [B, >=N] at stride out_stride_b                                              */
    int64_t* tokens;
    int32_t* parent;             /* final indices, -1 a child of the root                            */
    int32_t* depth;              /* 1-based                                                        */
    int32_t* pool_index;
    uint64_t* anc;               /* bit k: node k is node i or an ancestor of it                     */
    int64_t out_stride_b;
    int32_t* row_status;         /* nullable, [B]                                                  */
    int32_t* status_or;          /* nullable                                                       */
    void* workspace;             /* sd_tree_select_workspace_size bytes; the common convention      */
    size_t workspace_bytes;
} sd_tree_select_args;

/* 0 for a shape the call does not take                                                             */
size_t sd_tree_grow_workspace_size(int32_t batch, int32_t vocab, int32_t level, int32_t width, int32_t branch);
int32_t sd_tree_grow(const sd_tree_grow_args* args, void* stream);
size_t sd_tree_select_workspace_size(int32_t batch, int32_t pool_size, int32_t num_nodes);
int32_t sd_tree_select(const sd_tree_select_args* args, void* stream);

/* ---- Token-tree verification, distinct children, one topology PER SEQUENCE
 * (csrc/sd_verify_tree_dynamic.inc; additive, ABI 12).  sd_verify_tree_distinct with the parents on the
 * device: sequence b's are parent_dev[b * parent_stride_b + i], as sd_tree_select writes them.  The
 * rule, the noise keying, the outputs and the status conventions are sd_verify_tree_distinct's; path
 * is [B, max_depth] and tokens_out [B, max_depth + 1].  The topology is validated on the device:
 * parent[i] in [-1, i-1], at most SD_TREE_MAX_CHILDREN children per slot, depth <= max_depth.  A
 * sequence that fails gets SD_ROW_INVALID_DIST (ORed into status_or), n_accepted = 0, last_node = -1,
 * next_token = -1, path all -1, tokens_out all pad_token; nothing out of range is read or written.    */
typedef struct {
    int32_t batch;               /* B                                                              */
    int32_t num_nodes;           /* N, 1..SD_TREE_MAX_NODES                                         */
    int32_t vocab;
    int32_t max_depth;           /* 1..SD_MAX_GAMMA                                                 */
    const int32_t* parent_dev;   /* device int32 [B, >=N]                                           */
    int64_t parent_stride_b;
    const void* target_rows[SD_TREE_MAX_NODES + 1];
    int64_t target_stride_b;
    int32_t dtype;
    const int64_t* draft_tokens; /* [B, >=N]                                                       */
    int64_t draft_tokens_stride_b;
    sd_processor proc;
    const int64_t* stop_tokens;
    int32_t n_stop;
    int64_t pad_token;
    sd_noise noise;              /* SD_NOISE_PHILOX                                                */
    int32_t* n_accepted;
    int32_t* last_node;
    int64_t* next_token;
    float* resample_mass;        /* nullable                                                       */
    int32_t* n_sibling_rejects;  /* nullable                                                       */
    int32_t* stop_index;         /* nullable                                                       */
    int32_t* row_status;
    int32_t* path;               /* int32 [B, >=max_depth]                                          */
    int64_t path_stride_b;
    int64_t* tokens_out;         /* nullable: int64 [B, >=max_depth+1]                               */
    int64_t tokens_out_stride_b;
    void* workspace;             /* sd_verify_tree_dynamic_workspace_size bytes                     */
    size_t workspace_bytes;
    int32_t* status_or;          /* nullable                                                       */
} sd_tree_dynamic_args;

size_t sd_verify_tree_dynamic_workspace_size(int32_t batch, int32_t num_nodes, int32_t vocab);
int32_t sd_verify_tree_dynamic(const sd_tree_dynamic_args* args, void* stream);

/* ---- Block verification (csrc/sd_verify_block.inc; additive, ABI 12) --------------------------------
 * One verify step of ONE drafted chain per sequence that tests the drafted block jointly (Sun,
 * Mendlovic, Leviathan et al., "Block Verification Accelerates Speculative Decoding", ICLR 2025)
 * instead of token by token.  It is lossless, reads the rows sd_verify reads, and never accepts fewer
 * tokens in expectation than the token-wise rule on the same rows and drafts.  Probabilities are
 * SD_RULE_SPEC's: P_t the processed, dtype-rounded target row t = 0..γ' (row γ' is the bonus row),
 * Q_t that of drafter row t = 0..γ'-1, x_t = tok[t]; target and drafter rows share ONE processor and
 * one dtype, as in sd_verify_multi.  Per sequence:
 *
 *   w_0 = 1
 *   for t in 0..γ'-1:  a = P_t[x_t] / Q_t[x_t]         fp32; a NaN ratio (0/0, an id outside the
 *                                                      vocabulary) counts as +inf: SPEC's test accepts there
 *                      w_{t+1} = 0 if w_t == 0 else min(1, w_t * a)          fp32; never NaN
 *   for t in 0..γ'-1:  S_t = Σ_v max(w_t * P_t[v] - Q_t[v], 0)
 *                      each element is fmaf(w_t, P_t[v], -Q_t[v]) in fp32 (one rounding; at w_t = 1 it
 *                      is the rounded p - q of sd_verify and sd_verify_multi), elements are summed in
 *                      fp32 per 2048-element chunk, the chunk totals in fp64 in chunk order
 *   h_t  = S_t / (S_t + 1 - w_t)   for 1 <= t < γ'     fp64, rounded to float; a divisor <= 0 gives 0
 *   h_γ' = w_γ'
 *   n = the LARGEST t in 1..γ' with not (u_t > h_t), else 0      u_t = the row's accept uniform t-1
 *   n == γ':  x ~ P_γ'                                SD_ROW_BONUS,    resample_mass = NaN
 *   else:     x ~ max(w_n * P_n - Q_n, 0) / S_n       SD_ROW_RESIDUAL, resample_mass = (float)S_n
 *
 * The tests are independent of one another (every u_t is compared, the largest passing t wins), which
 * is what lets a rejected early draft be rescued by a later one.  With γ' = 1, h_1 = min(1, p/q), so
 * n, the status, the stop scan and the prune lengths are sd_verify(SD_RULE_SPEC)'s; so are they for any
 * γ' whose ratios are all >= 1.  Greedy: the same rule with x the argmax of the exit's weights, lowest
 * index first.
 * After the walk: the stop scan over tok[:n] (SD_ROW_STOP_IN_DRAFTS, stop_index, no token drawn,
 * next_token = -1), the prune lengths, tokens_out / pad_token and status_or, as sd_verify_multi; an exit
 * whose mass is zero or not finite is flagged SD_ROW_INVALID_DIST and draws nothing.
 * Noise is SD_NOISE_PHILOX only (SD_NOISE_STREAM: SD_ERR_UNSUPPORTED): sequence b is row row_base + b,
 * the sample is drawn by inverse CDF on the row's cdf uniform; one call consumes one offset.
 * Limits: γ' 1..SD_MAX_GAMMA, B 1..SD_MULTI_MAX_ROWS, V as sd_verify_multi.
 * Kernels: the row statistics of the 2γ'+1 rows per sequence, ONE launch over (sequence, t, chunk) that
 * writes the chunk totals of every S_t and of the bonus row (each workgroup forms its own w_t from
 * the 2t scalars it depends on), one launch that walks and samples.  Launch boundaries only.        */
typedef struct {
    int32_t batch;               /* B, 1..SD_MULTI_MAX_ROWS                                         */
    int32_t gamma;               /* γ', 1..SD_MAX_GAMMA                                             */
    int32_t vocab;
    /* target row t of sequence b at target_rows[t] + b * target_stride_b (t = γ' is the bonus row),
       drafter row t at draft_rows[t] + b * draft_stride_b                                          */
    const void* target_rows[SD_MAX_GAMMA + 1];
    int64_t target_stride_b;
    int32_t target_dtype;        /* sd_dtype                                                       */
    const void* draft_rows[SD_MAX_GAMMA];
    int64_t draft_stride_b;
    int32_t draft_dtype;         /* must equal target_dtype (SD_ERR_UNSUPPORTED otherwise)          */
    const int64_t* draft_tokens; /* [B, >=γ'] drafted ids                                           */
    int64_t draft_tokens_stride_b;
    sd_processor proc;           /* the loop's logits_processor, for target and drafter rows       */
    const int64_t* stop_tokens;  /* device [n_stop]                                                */
    int32_t n_stop;
    int64_t pad_token;           /* fills tokens_out past the emitted tokens                        */
    sd_noise noise;              /* SD_NOISE_PHILOX                                                */

    /* outputs, device, [B] */
    int32_t* n_accepted;         /* n                                                              */
    int64_t* next_token;         /* x, -1 if none                                                  */
    float* resample_mass;        /* (float)S_n on a residual exit, NaN on a bonus exit (nullable)   */
    int32_t* prune_drafter;      /* γ'-n on a residual exit, else 0 (nullable)                      */
    int32_t* prune_target;       /* γ'-n+1 on a residual exit, else 0 (nullable)                    */
    int32_t* stop_index;         /* position of the stop token in tok[:n], -1 (nullable)            */
    int32_t* row_status;         /* SD_ROW_* bits                                                  */
    /* optional (nullable): int64 [B, >=γ'+1] at tokens_out + b * tokens_out_stride_b: tok[:n], then x
       (when one was drawn), then pad_token up to γ'+1 entries                                      */
    int64_t* tokens_out;
    int64_t tokens_out_stride_b;
    /* diagnostics (nullable): w_0..w_γ' as float [B, γ'+1] at weights + b * (γ'+1); h_1..h_γ' as
       float [B, γ'] at accept_prob + b * γ'                                                        */
    float* weights;
    float* accept_prob;

    void* workspace;             /* sd_verify_block_workspace_size bytes, zero-filled once; shares
                                    the other entry points' convention (counter block left at zero) */
    size_t workspace_bytes;
    /* optional hints (nullable), as sd_verify_multi's: drafter row t of sequence b at
       draft_row_stats + 2 * (t * draft_row_stats_stride + b), stride >= B; draft_row_keep at the
       same layout, needed with the stats under a top-k / nucleus processor                         */
    const float* draft_row_stats;
    int64_t draft_row_stats_stride;
    const struct sd_row_keep* draft_row_keep;
    int32_t* status_or;          /* nullable: every sequence's SD_ROW_ERROR_MASK bits ORed in       */
} sd_block_args;

size_t sd_verify_block_workspace_size(int32_t batch, int32_t gamma, int32_t vocab);
int32_t sd_verify_block(const sd_block_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPECDEC_H */
