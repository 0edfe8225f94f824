/*
 * pcx.h -- C ABI of libpcx, the MI355X (gfx950) implementation of
 * pyconsensus's Oracle.consensus() hot path (algorithm "PCA", plus "absolute",
 * "big-five", "fixed-variance" and "cokurtosis" on the same kernels, and the
 * clustering algorithms "k-means", "hierarchical" and "clusterfeck" in the
 * batched regime).
 *
 * The reference (IanMadlenya/pyconsensus) is pure Python with no FFI: its whole
 * public surface is `Oracle(reports, event_bounds, reputation, ...).consensus()`
 * (pyconsensus/__init__.py:102-146, 502-611).  The entry points below are what a
 * binding of that path needs; each cites the reference code it replaces.  The
 * Python host layer (pyconsensus_amd/oracle.py) keeps the reference's class, its
 * constructor arguments and its result dict, and calls this ABI through ctypes.
 *
 * Conventions
 *   - Every pointer in a problem/result struct is DEVICE memory (hipMalloc or a
 *     torch tensor's data_ptr()) on the device the context was created for.
 *   - Matrices are row-major: reports[i*E + j] = reporter i, event j.
 *     NaN marks a missing report; 0.0 is ALSO missing (reference NA = 0.0,
 *     __init__.py:68, 278).
 *   - Any output pointer may be NULL: that output is not written.
 *   - Return value 0 = success, negative = error; pcx_last_error() describes the
 *     last error of the calling thread.  No C++ exception crosses the ABI.
 *   - Calls are asynchronous on the context's stream (pcx_set_stream) unless
 *     stated otherwise; a pcx_ctx is not thread-safe (one per thread).
 */
#ifndef PCX_H
#define PCX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCX_ABI_VERSION 9

enum pcx_status {
    PCX_OK = 0,
    PCX_EINVAL = -1,       /* bad argument / unsupported shape            */
    PCX_EHIP = -2,         /* HIP runtime error                           */
    PCX_ENOMEM = -3,       /* scratch allocation failed                   */
    PCX_ECOMM = -4,        /* RCCL error                                  */
};

/* Branch taken by the sign-choice rule (__init__.py:494-498, 482-484). */
enum pcx_branch {
    PCX_BRANCH_SET1 = 1,           /* rank rule ref_ind < 0                   */
    PCX_BRANCH_SET2 = 2,           /* rank rule ref_ind > 0                   */
    PCX_BRANCH_TIE_SET1 = 3,       /* ref_ind == 0 -> nonconformity, ref <= 0 */
    PCX_BRANCH_TIE_SET2 = 4,       /* ref_ind == 0 -> nonconformity, ref > 0  */
    PCX_BRANCH_NONE = 5,           /* algorithm without a branch ("absolute") */
};

/* Flags reported per round (bit set). */
enum pcx_flag {
    PCX_FLAG_ZERO_COV = 1,         /* covariance == 0: loading = e_0 (svd(0) = I, __init__.py:330) */
    PCX_FLAG_SVD_FAIL = 2,         /* non-finite covariance: loading = ones/sqrt(E) (:331-333)       */
    PCX_FLAG_PI_MAXIT = 4,         /* power iteration hit its iteration cap                         */
};

typedef struct pcx_ctx pcx_ctx;

int         pcx_abi_version(void);
const char* pcx_last_error(void);

/* One context per device and host thread.  Replaces nothing in the reference
 * (it has no device state); owns scratch buffers and the stream. */
pcx_ctx* pcx_create(int device_id);
void     pcx_destroy(pcx_ctx* ctx);
int      pcx_set_stream(pcx_ctx* ctx, void* hip_stream);  /* NULL = default stream */
int      pcx_synchronize(pcx_ctx* ctx);

/* ------------------------------------------------------------------------ */
/* Batched regime: B independent rounds of equal shape N x E (Simulator.jl-    */
/* style Monte Carlo, README.rst:52-56).  Each round is the complete            */
/* Oracle(reports, event_bounds, reputation).consensus() of __init__.py:102-611. */
/* N <= 64, E <= 32: one round per wavefront, asynchronous on the stream.      */
/* N <= 256, E <= 64 (every algorithm; k-means with kmeans_k <= 16): one        */
/* 256-thread workgroup per round (the same SPEC order), asynchronous.  Any      */
/* other shape (E <= 65536) or code-book size: each round is one single-matrix   */
/* consensus, a pool of worker streams keeps many in flight (PCX_ROUND_WORKERS,  */
/* default 16); synchronous.  pcx_batched_route tells which of the three.        */
/* pcx_consensus_batched_tall_f64 (below) moves rounds of up to 1024 x 64 from   */
/* the last regime to a workgroup per round; this entry's routes do not change.  */
/* ------------------------------------------------------------------------ */
typedef struct {
    int64_t n_rounds;             /* B                                           */
    int64_t n_reporters;          /* N                                           */
    int64_t n_events;             /* E                                           */
    const double*  reports;       /* [B][N][E]                                   */
    const double*  reputation;    /* [B][N] raw weights, or NULL (= None: 1/N)   */
    const uint8_t* scaled;        /* [B][E] (or [E] if bounds_shared), NULL = event_bounds None */
    const double*  lo;            /* event_bounds[j]["min"], same layout as scaled */
    const double*  hi;            /* event_bounds[j]["max"]                      */
    int32_t bounds_shared;        /* 1: scaled/lo/hi are one [E] row for all rounds */
    int32_t int_dtype;            /* 1: reports had an integer dtype (truncation, Q3) */
    double  catch_tolerance;      /* Oracle(catch_tolerance=0.1)                 */
    double  alpha;                /* Oracle(alpha=0.1)                           */
    int32_t algorithm;            /* enum pcx_algorithm                          */
    int32_t max_components;       /* "big-five": components summed (Oracle caps it at E, :134-137) */
    double  variance_threshold;   /* "fixed-variance": cumulative explained-variance stop (:448) */
    const double* aux_scores;     /* "cokurtosis": [B][N] caller scores, aux["cokurt"] (:455-457) */
    /* clustering algorithms (ABI >= 4; __init__.py:392-428) */
    double  hierarchy_threshold;  /* "hierarchical": fcluster distance cut, Oracle(hierarchy_threshold=0.5) (:406) */
    double  cluster_threshold;    /* "clusterfeck": leader-clustering cut after the reference's default rule
                                     log10(E)/1.77 (0.3 when that is 0) (:210-213); <= 0: computed on the device */
    int32_t kmeans_k;             /* "k-means": code-book size, int(ceil(sqrt(N))) in the reference (:396)     */
    int32_t kmeans_restarts;      /* "k-means": scipy.cluster.vq.kmeans iter= (20)                              */
    const int32_t* kmeans_init;   /* "k-means": [B][restarts][k] rows of the initial code books -- the draws of
                                     scipy's _kpoints, rng.choice(N, k, replace=False) on numpy's global
                                     RandomState, made by the host so the device replays the same restarts */
} pcx_batch;

/* Oracle(algorithm=...) values on the GPU path (__init__.py:368-457). */
enum pcx_algorithm {
    PCX_ALG_PCA = 0,               /* first principal component + rank rule (:368-371)         */
    PCX_ALG_ABSOLUTE = 1,          /* unimplemented branch: nc = 0 (:359-362, Q13)             */
    PCX_ALG_BIG_FIVE = 2,          /* eigenvalue-weighted top max_components scores (:373-390) */
    PCX_ALG_FIXED_VARIANCE = 3,    /* components up to variance_threshold (:429-451)           */
    PCX_ALG_COKURTOSIS = 4,        /* caller-supplied scores aux["cokurt"] (:455-457)          */
    PCX_ALG_KMEANS = 5,            /* cluster sizes of scipy kmeans on whitened wcd (:392-405)          */
    PCX_ALG_HIERARCHICAL = 6,      /* cluster sizes of single-linkage fclusterdata(wcd) (:407-419)     */
    PCX_ALG_CLUSTERFECK = 7,       /* leader clustering of the filled reports (:148-242, :421-424)     */
};

typedef struct {
    /* [B][N] -- result["agents"] */
    double* old_rep;
    double* this_rep;
    double* smooth_rep;
    double* scores;
    double* na_row;
    double* participation_rows;
    double* relative_part;
    double* reporter_bonus;
    /* [B][E] -- result["events"] */
    double* adj_first_loadings;
    double* outcomes_raw;
    double* outcomes_adjusted;
    double* outcomes_final;
    double* certainty;
    double* consensus_reward;
    double* nas_filled;
    double* participation_columns;
    double* author_bonus;
    /* [B] */
    double*  participation;
    double*  avg_certainty;
    int32_t* branch;              /* enum pcx_branch                             */
    int32_t* flags;               /* enum pcx_flag bits                          */
    int32_t* pi_iters;            /* power-iteration steps (incl. squarings)     */
    /* [B][N][E], optional */
    double* original;             /* result["original"]: rescaled reports        */
    double* filled;               /* result["filled"]                            */
    /* [B] */
    int32_t* components;          /* result["components"]: fixed-variance count, else -1 (:449, :610) */
} pcx_batch_result;

int pcx_consensus_batched_f64(pcx_ctx* ctx, const pcx_batch* in, pcx_batch_result* out);

/* Tall rounds (added under ABI 9; detect by symbol): pcx_consensus_batched_f64's
 * arguments and refusals, with rounds of 256 < N <= 1024 reporters and E <= 64 events on the
 * workgroup-per-round kernel's tall form -- one workgroup per round, ONE asynchronous launch, every
 * output bit-identical to the batched SPEC (oracle/pcx_oracle_batched.c) built with NMAX = 1024.
 * Algorithms: PCA, absolute, big-five, fixed-variance, cokurtosis.  The kernel carves its LDS by a plan
 * per shape; a shape whose plan does not fit the 160 KiB of a workgroup (big-five and fixed-variance
 * with many reporters AND many events), the clusterings, N > 1024 and E > 64 run exactly as
 * pcx_consensus_batched_f64 runs them: same route, same bytes, and so does every shape up to 256 x 64.
 * pcx_tall_route tells which.  Opt-in because the scheduler's results above 256 reporters are the
 * single-matrix path's arithmetic, not the SPEC's bits: the two routes agree within tolerance, not bit
 * for bit.  Calls share the context's workgroup scratch: keep them on one stream. */
int pcx_consensus_batched_tall_f64(pcx_ctx* ctx, const pcx_batch* in, pcx_batch_result* out);

/* ------------------------------------------------------------------------ */
/* Ragged batches (added under ABI 9; detect by symbol): B rounds of DIFFERENT  */
/* shapes N_b x E_b in one launch of the one-wave round kernel.  The arrays are */
/* the rounds' own arrays laid end to end in round order, with no padding (a     */
/* padded row or column would change the reputation normalisation, the           */
/* participation figures and the fills).  Every algorithm but k-means (its       */
/* code-book size depends on N_b); "big-five" caps max_components at E_b per      */
/* round (:134-137); "clusterfeck" with cluster_threshold <= 0 takes the          */
/* log10(E_b)/1.77 rule per round.  Asynchronous on the context's stream.        */
/* ------------------------------------------------------------------------ */
typedef struct {
    int64_t n_rounds;
    const int32_t* n_reporters;   /* HOST [B]: N_b in [1, 64]  (the wide entry: [1, 256])     */
    const int32_t* n_events;      /* HOST [B]: E_b in [1, 32]  (the wide entry: [1, 64])      */
    const double*  reports;       /* DEVICE, round after round, each N_b x E_b row-major      */
    const double*  reputation;    /* DEVICE [sum N_b] or NULL (uniform)                       */
    const uint8_t* scaled;        /* DEVICE [sum E_b] or NULL (event_bounds None), with lo/hi */
    const double  *lo, *hi;
    int32_t int_dtype, algorithm;
    double  catch_tolerance, alpha;
    int32_t max_components;  double variance_threshold;
    const double* aux_scores;     /* cokurtosis: DEVICE [sum N_b]                             */
    double  hierarchy_threshold, cluster_threshold;
} pcx_ragged;

/* Pure (no context, no device): validates the shapes and the algorithm of a ragged batch.
 * totals = {sum N_b, sum E_b, sum N_b * E_b}, the lengths of the flat arrays; *lds_bytes = the
 * launch's dynamic LDS (the largest round's).  On refusal returns PCX_EINVAL with *bad_round = the
 * first offending round (-1: the algorithm); pcx_last_error names it.  Any output may be NULL. */
int pcx_ragged_plan(int64_t n_rounds, const int32_t* n_reporters, const int32_t* n_events, int algorithm,
                    int64_t totals[3], int64_t* lds_bytes, int64_t* bad_round);
/* The outputs are pcx_batch_result's: per-reporter arrays [sum N_b], per-event arrays [sum E_b],
 * original / filled [sum N_b * E_b], the rest [B]; all in round order.  n_rounds == 0 succeeds and
 * launches nothing.  On a pcx_create_devices context the call runs on device_ids[0]. */
int pcx_consensus_ragged_f64(pcx_ctx* ctx, const pcx_ragged* in, pcx_batch_result* out);

/* Wide ragged batches (added under ABI 9; detect by symbol): the same structs and layouts, rounds
 * up to 256 x 64.  The rounds of at most 64 x 32 run on the one-wave kernel as above; the others on
 * the workgroup-per-round kernel, one launch per launch class: the rounds per CU that a round's LDS
 * allows (its dynamic LDS plus the kernel's static LDS in 1,280-byte units of 160 KiB, at most the
 * kernel's three per CU).  The two entries above keep their limits and refusals.
 *
 * pcx_ragged_plan_wide is pure like pcx_ragged_plan: a round must lie within [1, 256] x [1, 64],
 * k-means is refused.  counts[0] / lds_bytes[0]: the one-wave rounds and their launch's dynamic LDS;
 * counts[c] / lds_bytes[c], c = 1..3: the workgroup rounds of launch class c and that launch's
 * dynamic LDS (the class's largest round; 0 for an empty class).  Any output may be NULL. */
int pcx_ragged_plan_wide(int64_t n_rounds, const int32_t* n_reporters, const int32_t* n_events, int algorithm,
                         int64_t totals[3], int64_t counts[4], int64_t lds_bytes[4], int64_t* bad_round);
/* Asynchronous on the context's stream, no host wait of its own; n_rounds == 0 succeeds and
 * launches nothing.  A batch of one-wave rounds only is pcx_consensus_ragged_f64 itself.  Each
 * round's results are those of pcx_consensus_batched_f64 on its shape (the batched SPEC's order).
 * The workgroup rounds use the context's per-round scratch in chunks of at most 2 GB; calls on one
 * context share it, so they belong on one stream (as the workgroup route of the batched call).
 * PCX_RAGGED_ONE_CLASS=1 in the environment (a diagnostic, read per call) runs every workgroup round
 * in one launch at the largest round's LDS. */
int pcx_consensus_ragged_wide_f64(pcx_ctx* ctx, const pcx_ragged* in, pcx_batch_result* out);

/* Per-round consensus parameters (added under ABI 9; detect by symbol): a wide ragged batch whose
 * rounds each take one of P parameter sets -- the algorithm and the six options that the entries
 * above share over the batch.  DESIGN.md 5.4.3 is the contract: round b's results are byte for byte
 * those of pcx_consensus_ragged_wide_f64 over the same batch with params[param_of[b]] shared.  The
 * kernels are the two ragged kernels' texts under new names, which read the round's set from a
 * device table; a launch holds the rounds of one instantiation group (one-wave: PCA / absolute /
 * cokurtosis, big-five / fixed-variance, hierarchical / clusterfeck; workgroup: the clusterings, the
 * rest, each by launch class), so the number of launches does not depend on P. */
typedef struct {
    int32_t algorithm;            /* enum pcx_algorithm; k-means is refused                    */
    int32_t max_components;       /* big-five (>= 1; capped at E_b on the device)              */
    double  catch_tolerance;
    double  alpha;
    double  variance_threshold;   /* fixed-variance                                            */
    double  hierarchy_threshold;  /* hierarchical                                              */
    double  cluster_threshold;    /* clusterfeck (<= 0: the log10(E_b)/1.77 rule per round)    */
} pcx_round_params;               /* 48 bytes */

/* Pure (no context, no device): validates the shapes (pcx_ragged_plan_wide's limits and words), the
 * P sets (HOST [P]) and param_of (HOST int32 [B], round b's set).  totals as pcx_ragged_plan;
 * *n_launches = the kernel launches the call makes with nothing chunked (at most 3 one-wave and
 * 2 x 3 workgroup launches).  On refusal returns PCX_EINVAL, pcx_last_error names the round or the
 * set: *bad_round = the first offending round (a shape, or param_of[b] outside [0, P)), else -1;
 * *bad_param = the first offending set of the table, used or not (an algorithm outside 0..7,
 * k-means, a non-finite alpha or catch_tolerance, big-five with max_components < 1, a NaN
 * hierarchy_threshold or a non-finite variance_threshold where the set's algorithm reads it), else
 * -1; the sets are checked before the rounds; n_params < 1 with n_rounds > 0 leaves both -1.  Any
 * output may be NULL. */
int pcx_ragged_plan_params(int64_t n_rounds, const int32_t* n_reporters, const int32_t* n_events, int64_t n_params,
                           const pcx_round_params* params, const int32_t* param_of, int64_t totals[3],
                           int64_t* n_launches, int64_t* bad_round, int64_t* bad_param);
/* pcx_consensus_ragged_wide_f64 with params (HOST [P]) and param_of (HOST [B]) in place of in's own
 * seven parameter fields, which are not read.  in->aux_scores (DEVICE [sum N_b]) is required if and
 * only if some round's set is cokurtosis, and is read for those rounds only.  Refuses what
 * pcx_ragged_plan_params refuses.  Asynchronous on the context's stream, no host wait of its own: the
 * parameter table rides in the call's staging slot behind the descriptors, in the one upload.
 * n_rounds == 0 succeeds and launches nothing. */
int pcx_consensus_ragged_params_f64(pcx_ctx* ctx, const pcx_ragged* in, int64_t n_params,
                                    const pcx_round_params* params, const int32_t* param_of, pcx_batch_result* out);

/* k-means in ragged batches (added under ABI 9; detect by symbol).  The entries
 * above keep their refusals; these take k-means as one more clustering algorithm of a parameter set.
 *
 * Code books: round b's books are restarts x k_b int32 rows of [0, N_b) -- the rows of the round's
 * observations that start each restart (pcx_batch.kmeans_init of one round) -- at offsets[b] of one
 * flat DEVICE array, rounds end to end, nothing padded.  restarts is one value per call (>= 1).  k_b
 * is the reference's int(ceil(sqrt(N_b))) (:396), or the caller's: in [1, min(N_b, 8)] for a round
 * within 64 x 32 (the one-wave kernel's code-book rows), in [1, min(N_b, 16)] above that (the
 * workgroup kernel's). */
typedef struct {
    int32_t restarts;             /* >= 1, shared by the call's rounds                          */
    const int32_t* k;             /* HOST [B] code-book sizes, or NULL: the ceil(sqrt(N_b)) rule */
    const int32_t* init;          /* DEVICE, flat: round b's [restarts][k_b] rows at offsets[b]  */
} pcx_kmeans_books;

/* Pure (no context, no device): the layout of the flat book array when every round is k-means.
 * offsets [B + 1] int64 (or NULL): offsets[b] = sum over earlier rounds of restarts * k_b,
 * offsets[B] the array's length.  k HOST [B] or NULL (the rule).  Refuses (PCX_EINVAL,
 * pcx_last_error names the round) restarts < 1 (*bad_round = -1), a round outside [1, 256] x [1, 64]
 * and a k_b outside the bounds above, with *bad_round = the first such round.  n_rounds == 0
 * succeeds with offsets[0] = 0. */
int pcx_kmeans_plan(int64_t n_rounds, const int32_t* n_reporters, const int32_t* n_events, const int32_t* k,
                    int32_t restarts, int64_t* offsets, int64_t* bad_round);

/* pcx_ragged_plan_params with k-means allowed in a parameter set (pure).  books->restarts and
 * books->k are read (books->init is not) if some round's set is k-means, and then books must not be
 * NULL; k[b] is read for the k-means rounds only.  offsets [B + 1] int64 (or NULL) counts ONLY the
 * k-means rounds' books: a round of another algorithm has offsets[b + 1] == offsets[b].  Refuses
 * what pcx_ragged_plan_params refuses but k-means, in its order and words, then what
 * pcx_kmeans_plan refuses of the k-means rounds (*bad_round). */
int pcx_ragged_plan_kmeans(int64_t n_rounds, const int32_t* n_reporters, const int32_t* n_events, int64_t n_params,
                           const pcx_round_params* params, const int32_t* param_of, const pcx_kmeans_books* books,
                           int64_t totals[3], int64_t* n_launches, int64_t* offsets, int64_t* bad_round,
                           int64_t* bad_param);
/* pcx_consensus_ragged_params_f64 with PCX_ALG_KMEANS accepted in a parameter set: round b's results
 * are byte for byte those of pcx_consensus_batched_f64 on its shape with kmeans_k = k_b,
 * kmeans_restarts = books->restarts and kmeans_init = books->init + offsets[b] (offsets as
 * pcx_ragged_plan_kmeans lays them out: only the k-means rounds' books are in the array); a row
 * outside [0, N_b) is clamped as there.  The k-means rounds are clustering rounds: they join the
 * hierarchical and clusterfeck rounds' launches (one-wave group 2, the workgroup kernel's CLUS
 * launches by launch class), so a call still makes at most 3 + 2 x 3 launches.  The clustering
 * launches run the round kernels' texts in a further form that reads {offset, k_b} from a per-round
 * device table, which rides in the call's one upload; the other launches are
 * pcx_consensus_ragged_params_f64's own.  Refuses what pcx_ragged_plan_kmeans refuses, and NULL
 * books->init with a k-means round, before it launches anything.  Asynchronous. */
int pcx_consensus_ragged_kmeans_f64(pcx_ctx* ctx, const pcx_ragged* in, int64_t n_params,
                                    const pcx_round_params* params, const int32_t* param_of,
                                    const pcx_kmeans_books* books, pcx_batch_result* out);

/* ------------------------------------------------------------------------ */
/* Monte Carlo simulator (ABI >= 9): the Simulator.jl-style driver of the       */
/* batched regime (README.rst:52-56) on the device.  It draws random rounds     */
/* with a counter-based generator (Philox4x32-10; DESIGN.md "Simulator" is the  */
/* specification), runs pcx_consensus_batched_f64 on them, scores each round    */
/* against the truth it drew and carries smooth_rep into the next timestep's    */
/* reputation.  Replaces nothing in the reference (it has no generator).        */
/* ------------------------------------------------------------------------ */
typedef struct {
    int64_t  n_rounds;            /* B                                           */
    int64_t  n_reporters;         /* N                                           */
    int64_t  n_events;            /* E                                           */
    int64_t  n_timesteps;         /* T in [1, 2^24)                              */
    uint64_t seed;                /* Philox key (low word, high word)            */
    double  liar_frac;            /* P(a reporter lies), the same person in every timestep */
    double  collude_frac;         /* P(a liar reports the event's shared lie, not a random value) */
    double  distort;              /* P(an honest report is a random value)       */
    double  na_frac;              /* P(a report is missing: NaN)                 */
    double  scaled_frac;          /* P(an event is scaled)                       */
    double  scaled_tol;           /* a scaled outcome is correct within scaled_tol * (hi - lo) of the truth */
    /* the consensus parameters of pcx_batch (k-means and cokurtosis are refused:
       they need host-drawn code books / caller scores) */
    double  catch_tolerance;
    double  alpha;
    int32_t algorithm;
    int32_t max_components;
    double  variance_threshold;
    double  hierarchy_threshold;
    double  cluster_threshold;
    const double* reputation0;    /* [B][N] reputation of timestep 0 (device), or NULL = uniform */
} pcx_sim;

/* One timestep's rounds.  Any pointer may be NULL (not written) except where a function
 * says otherwise. */
typedef struct {
    double*  reports;             /* [B][N][E], NaN = missing                    */
    uint8_t* scaled;              /* [B][E]                                      */
    double*  lo;                  /* [B][E] (binary events: 1)                   */
    double*  hi;                  /* [B][E] (binary events: 2)                   */
    double*  truth;               /* [B][E] the outcome an honest reporter sees  */
    uint8_t* liar;                /* [B][N] bit 0: liar, bit 1: a liar that colludes */
} pcx_sim_rounds;

#define PCX_SIM_NMETRICS 6        /* correct, liar_rep_before, liar_rep_after, liars_bonus, beats, n_liars */

typedef struct {
    double* metrics;              /* [T][B][PCX_SIM_NMETRICS]                    */
    double* summary;              /* [T][PCX_SIM_NMETRICS] mean over the rounds  */
    double* reputation;           /* [B][N] smooth_rep of the last timestep      */
    pcx_sim_rounds   last;        /* the last timestep's rounds                  */
    pcx_batch_result last_out;    /* the last timestep's consensus outputs       */
} pcx_sim_result;

/* Philox4x32-10 on the host (the generator's only source of randomness). */
void pcx_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);
/* The rounds of one timestep on the CPU, HOST pointers, no context: the same inline code
 * as the device kernel (csrc/pcx_sim.h), bit for bit. */
int pcx_sim_generate_host(const pcx_sim* sim, int timestep, pcx_sim_rounds* out);
/* The same on the device; asynchronous on the context's stream. */
int pcx_sim_generate_f64(pcx_ctx* ctx, const pcx_sim* sim, int timestep, pcx_sim_rounds* out);
/* Score B rounds: metrics [B][PCX_SIM_NMETRICS] (required), summary [PCX_SIM_NMETRICS] or
 * NULL.  rounds->scaled, lo, hi, truth and liar are required.  Asynchronous. */
int pcx_sim_metrics_f64(pcx_ctx* ctx, const pcx_sim* sim, const pcx_sim_rounds* rounds, const double* old_rep,
                        const double* smooth_rep, const double* outcomes_final, double* metrics, double* summary);
/* T timesteps of generate -> pcx_consensus_batched_f64 -> metrics -> reputation carry.  The
 * work buffers live in the context (kept between calls, freed by pcx_release_workspace).
 * Asynchronous, without a host synchronisation in the loop, when the shape takes an
 * asynchronous batched regime (N <= 256 and E <= 64). */
int pcx_simulate_f64(pcx_ctx* ctx, const pcx_sim* sim, pcx_sim_result* result);

/* ------------------------------------------------------------------------ */
/* Simulator sweeps (added under ABI 9; detect by symbol): C cells, each with   */
/* its own number of rounds, shape, generator probabilities and seed, in one    */
/* call (a curve or a grid of a Monte Carlo study).  The rounds of all cells lie */
/* end to end in cell order in pcx_ragged's flat layout: B = sum R_c rounds,     */
/* reporter arrays [sum R_c N_c], event arrays [sum R_c E_c], reports            */
/* [sum R_c N_c E_c].  Cell c's slice of every output is byte for byte what      */
/* pcx_simulate_f64 gives for n_rounds = R_c, n_reporters = N_c, n_events = E_c, */
/* the cell's seed and probabilities and the shared parameters: the generator's  */
/* round counter is the round's index inside its cell and its key the cell's     */
/* seed, so cells that share a seed see common random numbers.  "big-five" caps  */
/* max_components at E_c on the device (the equal-shape call it compares with     */
/* gets min(max_components, E_c)); "clusterfeck" with cluster_threshold <= 0      */
/* takes the device's per-round rule, as pcx_consensus_ragged_wide_f64.           */
/* ------------------------------------------------------------------------ */
typedef struct {
    int64_t  n_rounds;            /* R_c in [1, 2^31)                            */
    int32_t  n_reporters;         /* N_c in [1, 256]                             */
    int32_t  n_events;            /* E_c in [1, 64]                              */
    uint64_t seed;                /* the cell's Philox key                       */
    double  liar_frac, collude_frac, distort, na_frac, scaled_frac;  /* as pcx_sim's */
} pcx_sim_cell;

typedef struct {
    int64_t  n_cells;             /* C; 0 succeeds and launches nothing          */
    const pcx_sim_cell* cells;    /* HOST [C]                                    */
    int64_t  n_timesteps;         /* T in [1, 2^24)                              */
    double  scaled_tol;
    /* the consensus parameters, shared by the cells (k-means and cokurtosis are refused) */
    double  catch_tolerance;
    double  alpha;
    int32_t algorithm;
    int32_t max_components;
    double  variance_threshold;
    double  hierarchy_threshold;
    double  cluster_threshold;
    const double* reputation0;    /* DEVICE [sum R_c N_c] reputation of timestep 0, or NULL = uniform */
} pcx_sim_sweep;

/* Pure (no context, no device): validates a sweep.  totals = {B, sum R_c N_c, sum R_c E_c,
 * sum R_c N_c E_c}; counts / lds_bytes are what pcx_ragged_plan_wide reports for the sweep's
 * rounds.  On refusal returns PCX_EINVAL with *bad_cell = the first offending cell (-1: a shared
 * parameter); pcx_last_error names it.  Any output may be NULL. */
int pcx_sim_sweep_plan(const pcx_sim_sweep* sweep, int64_t totals[4], int64_t counts[4], int64_t lds_bytes[4],
                       int64_t* bad_cell);
/* The sweep's rounds of one timestep on the CPU (HOST pointers, no context; flat layout), from
 * the same inline code as the device kernel. */
int pcx_sim_sweep_generate_host(const pcx_sim_sweep* sweep, int timestep, pcx_sim_rounds* rounds);
/* The same on the device; asynchronous on the context's stream. */
int pcx_sim_sweep_generate_f64(pcx_ctx* ctx, const pcx_sim_sweep* sweep, int timestep, pcx_sim_rounds* rounds);
/* Score the sweep's rounds: metrics [B][PCX_SIM_NMETRICS] (required), summary
 * [C][PCX_SIM_NMETRICS] or NULL: each cell's means over its R_c rounds in pcx_simulate_f64's
 * summary order.  rounds->scaled, lo, hi, truth and liar are required.  Asynchronous. */
int pcx_sim_sweep_metrics_f64(pcx_ctx* ctx, const pcx_sim_sweep* sweep, const pcx_sim_rounds* rounds,
                              const double* old_rep, const double* smooth_rep, const double* outcomes_final,
                              double* metrics, double* summary);
/* T timesteps of generate -> pcx_consensus_ragged_wide_f64's launches -> metrics -> per-cell
 * summary -> reputation carry, asynchronous on the context's stream with no host wait in the
 * loop (the descriptor tables are built and uploaded once per call).  The result is read with
 * flat layouts: metrics [T][B][6], summary [T][C][6], reputation [sum R_c N_c], last / last_out as
 * pcx_ragged's flat arrays.  The work buffers are pcx_simulate_f64's (kept in the context). */
int pcx_simulate_sweep_f64(pcx_ctx* ctx, const pcx_sim_sweep* sweep, pcx_sim_result* result);

/* ------------------------------------------------------------------------ */
/* Simulator studies (added under ABI 9; detect by symbol): a sweep that also   */
/* writes twelve detail metrics per round every timestep and, after the last    */
/* timestep, reduces every per-round value to per-cell statistics and to paired */
/* differences against a base cell (cells that share a seed see common random   */
/* numbers: the paired difference is where that variance reduction shows).      */
/* DESIGN.md 5.4.2 is the specification; csrc/pcx_sim_study.h is the one source  */
/* of the device kernels and of the *_host entries, which agree bit for bit.     */
/* Every entry above keeps its outputs.                                          */
/* ------------------------------------------------------------------------ */
#define PCX_SIM_NDETAIL 12        /* correct_binary, correct_scaled, indeterminate, flipped, nan_outcomes,
                                     scaled_err, tp, fn, fp, tn, mcc, colluder_rep_after */
#define PCX_SIM_NVALUES (PCX_SIM_NMETRICS + PCX_SIM_NDETAIL)  /* per round: the metrics, then the detail */
#define PCX_SIM_NSTATS 5          /* n, mean, var, min, max over a cell's rounds whose value is not NaN */
#define PCX_SIM_NPAIRED 3         /* n, mean, var of v_cell[b] - v_base[b] where neither is NaN */

typedef struct {
    double* detail;               /* [T][B][PCX_SIM_NDETAIL], or NULL: kept in the context's workspace */
    double* stats;                /* [T][C][PCX_SIM_NVALUES][PCX_SIM_NSTATS]    */
    double* paired;               /* [T][C][PCX_SIM_NVALUES][PCX_SIM_NPAIRED], or NULL */
} pcx_sim_study_result;

/* Detail metrics of B equal-shape rounds: detail [B][PCX_SIM_NDETAIL].  The arguments are
 * pcx_sim_metrics_f64's (rounds->scaled, lo, hi, truth and liar are required).  A ratio with a zero
 * denominator is NaN (no binary event, no scaled event, a zero factor under mcc's root); a reporter
 * is punished when smooth_rep < old_rep.  Asynchronous. */
int pcx_sim_detail_f64(pcx_ctx* ctx, const pcx_sim* sim, const pcx_sim_rounds* rounds, const double* old_rep,
                       const double* smooth_rep, const double* outcomes_final, double* detail);
/* The same for a sweep's rounds in the flat layout (pcx_sim_sweep_metrics_f64's arguments). */
int pcx_sim_sweep_detail_f64(pcx_ctx* ctx, const pcx_sim_sweep* sweep, const pcx_sim_rounds* rounds,
                             const double* old_rep, const double* smooth_rep, const double* outcomes_final,
                             double* detail);
/* Both on the CPU: HOST pointers, no context, the same inline code as the kernel. */
int pcx_sim_detail_host(const pcx_sim* sim, const pcx_sim_rounds* rounds, const double* old_rep,
                        const double* smooth_rep, const double* outcomes_final, double* detail);
int pcx_sim_sweep_detail_host(const pcx_sim_sweep* sweep, const pcx_sim_rounds* rounds, const double* old_rep,
                              const double* smooth_rep, const double* outcomes_final, double* detail);
/* Pure: what pcx_sim_sweep_plan refuses, then pair_base (HOST int32 [C] or NULL: cell c's base cell,
 * or -1 for none): a base outside [0, C), a cell that is its own base, or a base with another number
 * of rounds gives PCX_EINVAL with *bad_cell = that cell (pcx_last_error names it).  The base need
 * not share the seed (the pairing is then merely uninformative). */
int pcx_sim_study_check(const pcx_sim_sweep* sweep, const int32_t* pair_base, int64_t* bad_cell);
/* Per-cell statistics of metrics [T][B][PCX_SIM_NMETRICS] and detail [T][B][PCX_SIM_NDETAIL] (device),
 * T = sweep->n_timesteps: stats [T][C][PCX_SIM_NVALUES][5] = {n, mean, var, min, max} over the cell's
 * non-NaN values.  Sums run in pcx_simulate_f64's summary order (256 strided lanes, then a tree), so
 * with no NaN the mean of a metric is byte for byte the sweep's summary; var is a second pass over
 * (v - mean)^2, divided by n - 1 (NaN for n < 2; n = 0: mean, min, max NaN).  paired
 * [T][C][PCX_SIM_NVALUES][3] = {n, mean, var} of v_c[b] - v_base[b], b the round inside its cell, over
 * the rounds where both are not NaN (base -1: n = 0 and NaN).  paired and pair_base may be NULL
 * together.  No atomics: the bytes do not depend on the launch geometry.  Asynchronous, one launch. */
int pcx_sim_sweep_stats_f64(pcx_ctx* ctx, const pcx_sim_sweep* sweep, const double* metrics, const double* detail,
                            const int32_t* pair_base, double* stats, double* paired);
/* The same on the CPU (HOST pointers, no context): the lanes and the tree replayed in a loop. */
int pcx_sim_sweep_stats_host(const pcx_sim_sweep* sweep, const double* metrics, const double* detail,
                             const int32_t* pair_base, double* stats, double* paired);
/* pcx_simulate_sweep_f64 with the detail launch after every timestep's metrics and one statistics
 * launch after the last timestep; asynchronous on the context's stream with no host wait of its own.
 * Every field of `result` is byte for byte what pcx_simulate_sweep_f64 writes for the sweep;
 * study->detail[t] is pcx_sim_sweep_detail_f64 on timestep t's rounds and outputs, study->stats /
 * paired are pcx_sim_sweep_stats_f64 on the call's own metrics and detail (result->metrics NULL: the
 * metrics are kept in the workspace too).  study->stats is required; paired needs pair_base.
 * Refuses what pcx_sim_study_check refuses before it launches anything; C = 0 launches nothing. */
int pcx_simulate_study_f64(pcx_ctx* ctx, const pcx_sim_sweep* sweep, const int32_t* pair_base,
                           pcx_sim_result* result, pcx_sim_study_result* study);

/* Studies with per-cell consensus parameters (added under ABI 9; detect by symbol):
 * cell c's rounds take cell_params[c] (HOST [C]) in place of the sweep's seven shared parameter
 * fields, which are then not read.  Cell c's slice of every output is byte for byte what
 * pcx_simulate_study_f64 gives for that cell alone with cell_params[c] as the shared parameters; a
 * cell pairs (pair_base) with any cell of as many rounds, so the same drawn rounds under two
 * parameter sets give a paired difference on common random numbers.  cell_params NULL: the entries
 * above, the same bytes.
 *
 * pcx_sim_study_params_check is pure: what pcx_sim_study_check refuses (the shared parameters
 * unchecked when cell_params is given), and per cell what pcx_ragged_plan_params refuses of a set,
 * plus cokurtosis (as k-means, not simulated), with *bad_cell = the cell. */
int pcx_sim_study_params_check(const pcx_sim_sweep* sweep, const pcx_round_params* cell_params,
                               const int32_t* pair_base, int64_t* bad_cell);
/* study NULL: the sweep alone (pcx_simulate_sweep_f64's outputs; pair_base is not read).
 * Asynchronous on the context's stream with no host wait of its own; the parameter table rides in
 * the call's one upload.  Per timestep: the launches of pcx_consensus_ragged_params_f64. */
int pcx_simulate_study_params_f64(pcx_ctx* ctx, const pcx_sim_sweep* sweep, const pcx_round_params* cell_params,
                                  const int32_t* pair_base, pcx_sim_result* result, pcx_sim_study_result* study);

/* k-means in the simulator (added under ABI 9; detect by symbol).  The entries above
 * keep their refusals.  The initial code books are drawn on the device from a further stream of the
 * generator (KMEANS = 5; streams 0..4 and their bits are unchanged): for round b (its index inside
 * its cell), restart r, timestep t and c = 0 .. k - 1, with j = N - k + c,
 *     w = Philox4x32-10((c, r, b, 5 << 24 | t), key).w0,   v = (w * (j + 1)) >> 32,
 *     book[c] = v if v is not among book[0 .. c), else j
 * (Floyd's sampling: k distinct rows of [0, N); integers only, so the host twins agree bit for bit).
 * k is the reference's int(ceil(sqrt(N))); the key is the simulation's / the cell's seed, so cells
 * that share seed, shape and rounds draw the same books.  The books of a timestep are materialised
 * once, in the context's workspace, and the round kernels read them; restarts is one value per call.
 *
 * pcx_sim_kmeans_books_*: books [B][restarts][k] int32 of one timestep of `sim` (whose algorithm need
 * not be k-means).  The sweep pair: every round of the sweep, laid out by pcx_kmeans_plan's offsets
 * over the sweep's rounds (the rule's k).  _host: HOST pointer, no context. */
int pcx_sim_kmeans_books_host(const pcx_sim* sim, int32_t restarts, int timestep, int32_t* books);
int pcx_sim_kmeans_books_f64(pcx_ctx* ctx, const pcx_sim* sim, int32_t restarts, int timestep, int32_t* books);
int pcx_sim_sweep_kmeans_books_host(const pcx_sim_sweep* sweep, int32_t restarts, int timestep, int32_t* books);
int pcx_sim_sweep_kmeans_books_f64(pcx_ctx* ctx, const pcx_sim_sweep* sweep, int32_t restarts, int timestep,
                                   int32_t* books);
/* pcx_simulate_f64 with k-means accepted (restarts >= 1): per timestep the generator, the books
 * kernel, pcx_consensus_batched_f64 with kmeans_init = the books, the metrics.  Timestep t's outputs
 * are those of pcx_consensus_batched_f64 on pcx_sim_generate_f64's rounds with
 * pcx_sim_kmeans_books_f64's books.  Another algorithm: pcx_simulate_f64's bytes.  Asynchronous where
 * pcx_simulate_f64 is. */
int pcx_simulate_kmeans_f64(pcx_ctx* ctx, const pcx_sim* sim, int32_t restarts, pcx_sim_result* result);
/* pcx_simulate_study_params_f64 with k-means accepted, shared (cell_params NULL) or in a cell's set:
 * per timestep the generator, the books kernel over the k-means cells' rounds, the launches of
 * pcx_consensus_ragged_kmeans_f64, the metrics.  study NULL: the sweep.  Cell c's slice of every
 * output is byte for byte what pcx_simulate_kmeans_f64 gives for that cell alone.  Cokurtosis stays
 * refused.  pcx_sim_study_kmeans_check is pure: what the call refuses (restarts < 1 with
 * *bad_cell = -1). */
int pcx_sim_study_kmeans_check(const pcx_sim_sweep* sweep, const pcx_round_params* cell_params,
                               const int32_t* pair_base, int32_t restarts, int64_t* bad_cell);
int pcx_simulate_study_kmeans_f64(pcx_ctx* ctx, const pcx_sim_sweep* sweep, const pcx_round_params* cell_params,
                                  const int32_t* pair_base, int32_t restarts, pcx_sim_result* result,
                                  pcx_sim_study_result* study);

/* Tall rounds in ragged batches and the simulator (added under ABI 9; detect by symbol; DESIGN.md
 * 5.5.3).  The entries above keep their [1, 256] x [1, 64] limits and words; these take rounds and
 * cells within [1, 1024] x [1, 64].  A round of N_b > 256 reporters is taken if and only if
 * pcx_tall_route(N_b, E_b, its set's algorithm, 1) == PCX_ROUTE_TALL; otherwise the call is refused
 * (PCX_EINVAL) with the round and the reason named -- a clustering above 256 reporters, or big-five /
 * fixed-variance whose LDS plan does not fit (e.g. 1024 x 64).  Nothing falls to the round scheduler.
 * Such rounds form one more segment of the call's launch plan, behind the others: one workgroup per
 * round of the tall kernel's per-round form, one launch class whatever the algorithms, with scratch
 * slot strides and a chunk of its own.  k-means is refused as by pcx_ragged_plan_params.
 *
 * pcx_ragged_plan_tall is pure: pcx_ragged_plan_params with those limits, *n_tall = the rounds of the
 * tall segment, *tall_lds_bytes = its launches' dynamic LDS (the largest pcx_tall_lds_bytes of its
 * rounds; 0 without one); *n_launches counts the tall segment.
 * pcx_consensus_ragged_tall_f64: a batch without a round above 256 reporters gives the bytes of
 * pcx_consensus_ragged_params_f64; round b above 256 reporters gives, in every output, the bytes of
 * pcx_consensus_batched_tall_f64 on that round alone with params[param_of[b]] shared.  Asynchronous,
 * no host wait of its own. */
int pcx_ragged_plan_tall(int64_t n_rounds, const int32_t* n_reporters, const int32_t* n_events, int64_t n_params,
                         const pcx_round_params* params, const int32_t* param_of, int64_t totals[3],
                         int64_t* n_launches, int64_t* bad_round, int64_t* bad_param, int64_t* n_tall,
                         int64_t* tall_lds_bytes);
int pcx_consensus_ragged_tall_f64(pcx_ctx* ctx, const pcx_ragged* in, int64_t n_params,
                                  const pcx_round_params* params, const int32_t* param_of, pcx_batch_result* out);
/* pcx_simulate_f64 whose consensus step is pcx_consensus_batched_tall_f64: shapes of the tall route
 * run one asynchronous launch per timestep instead of the round scheduler; every other shape gives
 * pcx_simulate_f64's bytes.  The equal-shape twin of a tall cell. */
int pcx_simulate_tall_f64(pcx_ctx* ctx, const pcx_sim* sim, pcx_sim_result* result);
/* pcx_simulate_study_params_f64 with cells up to 1024 reporters.  cell_params may be NULL (the
 * sweep's shared parameters as every cell's set); study may be NULL (the sweep alone).  Cell c's
 * slice of every output is byte for byte what pcx_simulate_tall_f64 gives for that cell alone; a call
 * without a cell above 256 reporters gives the bytes of pcx_simulate_study_params_f64 /
 * pcx_simulate_study_f64 / pcx_simulate_sweep_f64.  A cell is refused by index for what the ragged
 * tall plan refuses of its rounds; cokurtosis and k-means stay "not simulated".
 * pcx_sim_study_tall_check is pure: what the call refuses.  pcx_sim_sweep_plan_tall is pure too:
 * pcx_sim_sweep_plan's figures under those checks (cell_params NULL or [C]) -- totals over every cell;
 * counts / lds_bytes over the cells up to 256 reporters, each by its own algorithm: a cell above
 * counts in no launch class (it is the tall segment; pcx_tall_lds_bytes has a round's LDS). */
int pcx_sim_sweep_plan_tall(const pcx_sim_sweep* sweep, const pcx_round_params* cell_params, int64_t totals[4],
                            int64_t counts[4], int64_t lds_bytes[4], int64_t* bad_cell);
int pcx_sim_study_tall_check(const pcx_sim_sweep* sweep, const pcx_round_params* cell_params,
                             const int32_t* pair_base, int64_t* bad_cell);
int pcx_simulate_study_tall_f64(pcx_ctx* ctx, const pcx_sim_sweep* sweep, const pcx_round_params* cell_params,
                                const int32_t* pair_base, pcx_sim_result* result, pcx_sim_study_result* study);

/* ------------------------------------------------------------------------ */
/* Single-matrix regime: one N x E report matrix, optionally sharded by        */
/* contiguous reporter rows over several GPUs (one process -- or one thread --  */
/* per rank).  One call runs the whole Oracle(...).consensus() of              */
/* __init__.py:502-611; stage sequencing, scratch memory and the cross-rank    */
/* exchange (RCCL over xGMI, or the backends below) are owned by the library.   */
/* ------------------------------------------------------------------------ */

/* Multi-rank contexts.  pcx_create() above is a one-rank context.  For RCCL,
 * rank 0 calls pcx_comm_unique_id(), the caller broadcasts the 128 bytes over any
 * channel (e.g. torch.distributed), and every rank calls pcx_create_rank()
 * (ncclCommInitRank, collective over the ranks).  Replaces nothing in the
 * reference (it has no distribution). */
typedef struct { char internal[128]; } pcx_comm_id;
int      pcx_comm_unique_id(pcx_comm_id* out);
pcx_ctx* pcx_create_rank(int device_id, int world, int rank, const pcx_comm_id* id);

/* In-process virtual ranks: `world` threads, each with its own context on any
 * device, exchanging through host memory.  Used to rehearse the sharded path on
 * one GPU (tests, 1-GPU boxes).  The group must outlive its contexts. */
typedef struct pcx_group pcx_group;
pcx_group* pcx_group_create(int world);
void       pcx_group_destroy(pcx_group* g);
pcx_ctx*   pcx_create_grouped(int device_id, pcx_group* g, int rank);

/* Caller-supplied exchange (MPI, gloo, ...).  The library passes HOST buffers
 * (it stages device data through pinned memory); return 0 on success.
 *   allreduce: in place, `count` elements of enum pcx_dtype, enum pcx_redop.
 *   allgather: recv[world][bytes] <- every rank's `bytes` of send, rank order. */
enum pcx_dtype { PCX_F64 = 0, PCX_U64 = 1 };
enum pcx_redop { PCX_SUM = 0, PCX_MIN = 1, PCX_MAX = 2 };
typedef struct {
    void* user;
    int (*allreduce)(void* user, void* buf, int64_t count, int32_t dtype, int32_t op);
    int (*allgather)(void* user, const void* send, void* recv, int64_t bytes);
} pcx_comm_ops;
pcx_ctx* pcx_create_custom(int device_id, int world, int rank, const pcx_comm_ops* ops);

/* One process driving several GPUs (pcx_create(n_devices,
 * device_ids); replaces the reference's single-process Oracle(...).consensus(),
 * __init__.py:502-611, at sizes one GPU cannot hold).  A single-matrix call on this
 * context takes the WHOLE matrix in host memory (PCX_MEM_HOST, n_total == n_rows,
 * row_offset 0) and shards its rows over the devices in contiguous blocks (the
 * first N % n_devices blocks one row longer), one worker thread per device.  The
 * devices exchange through RCCL (ncclCommInitAll, xGMI) when the ids are distinct,
 * through host memory when an id repeats (rehearsal on fewer GPUs).  Results are
 * the one-device call's, bit for bit; the scalars of pcx_result are device 0's
 * (comm_bytes: summed over the devices).  pcx_consensus_batched_f64 on this
 * context runs on device_ids[0]. */
pcx_ctx* pcx_create_devices(int n_devices, const int* device_ids);

int pcx_ctx_world(const pcx_ctx* ctx);
int pcx_ctx_rank(const pcx_ctx* ctx);
/* 1 if the context's communicators can still exchange, 0 once a failed call aborted them (RCCL:
 * ncclCommAbort after a rank of a multi-device call failed mid-exchange): destroy and recreate
 * it then.  An argument error raised before any exchange (PCX_EINVAL from the rank-independent
 * checks) leaves the context usable. */
int pcx_ctx_usable(const pcx_ctx* ctx);
/* Drop the cached scratch of the single-matrix path (it is kept between calls of
 * the same shape: a C5 consensus needs ~50 GB of it). */
int pcx_release_workspace(pcx_ctx* ctx);

enum pcx_mem_kind {
    PCX_MEM_DEVICE = 0,  /* every pointer of pcx_problem / pcx_result is device memory of ctx's device */
    PCX_MEM_HOST = 1,    /* every pointer is host memory; the library copies in and out (timed apart) */
};

typedef struct {
    int64_t n_rows;               /* reporters held by this rank                         */
    int64_t n_events;             /* E                                                   */
    int64_t n_total;              /* N over all ranks (== n_rows on one rank)            */
    int64_t row_offset;           /* global index of this rank's first reporter          */
    const double*  reports;       /* [n_rows][E] row-major, NaN = missing (0.0 too, :278) */
    const double*  reputation;    /* [n_total] raw weights (every rank passes all N), or NULL = None (:138-141) */
    const uint8_t* scaled;        /* [E] event_bounds[j]["scaled"], or NULL = event_bounds None (Q12) */
    const double*  lo;            /* [E] event_bounds[j]["min"]                          */
    const double*  hi;            /* [E] event_bounds[j]["max"]                          */
    double  catch_tolerance;      /* Oracle(catch_tolerance=0.1)                         */
    double  alpha;                /* Oracle(alpha=0.1)                                   */
    int32_t int_dtype;            /* 1: reports had an integer dtype (truncation, Q3)    */
    int32_t algorithm;            /* enum pcx_algorithm (every value; the clustering ones on one rank) */
    int32_t max_components;       /* big-five (Oracle caps it at E, :134-137)            */
    int32_t mem_kind;             /* enum pcx_mem_kind                                   */
    double  variance_threshold;   /* fixed-variance (:448)                               */
    const double* aux_scores;     /* cokurtosis: [n_rows] this rank's aux["cokurt"] (:455-457) */
    /* clustering algorithms (one rank; ABI >= 7; __init__.py:148-242, 392-424) */
    double  hierarchy_threshold;  /* "hierarchical": fcluster distance cut, Oracle(hierarchy_threshold=0.5) */
    double  cluster_threshold;    /* "clusterfeck": leader cut; <= 0: the reference's log10(E)/1.77 rule */
    int32_t kmeans_k;             /* "k-means": code-book size int(ceil(sqrt(N))) (:396)          */
    int32_t kmeans_restarts;      /* "k-means": scipy kmeans iter= (20)                           */
    const int32_t* kmeans_init;   /* "k-means": [restarts][k] HOST rows of the initial code books (the
                                     reference's rng.choice draws, pyconsensus_amd.batched.kmeans_draws) */
} pcx_problem;

typedef struct {
    /* [n_rows] -- result["agents"], this rank's reporters; NULL = not written */
    double *old_rep, *this_rep, *smooth_rep, *scores, *na_row, *participation_rows, *relative_part,
        *reporter_bonus;
    /* [E] -- result["events"] (identical on every rank) */
    double *adj_first_loadings, *outcomes_raw, *outcomes_adjusted, *outcomes_final, *certainty,
        *consensus_reward, *nas_filled, *participation_columns, *author_bonus;
    /* [n_rows][E], optional: result["original"] (rescaled reports), result["filled"].
     * original == (double*)problem.reports (the same pointer) is the reference's own aliasing
     * (__init__.py:121, 266-269, 584: `original` IS the caller's array, rescaled in place): the
     * scaled columns of the reports are then rescaled in place and the other columns are left as
     * they are, which saves writing a copy of the whole matrix (pcx_consensus_f64 and
     * pcx_interpolate_f64; the reports buffer must then be writable).  After a failed call the
     * buffer's scaled columns are unspecified: with several ranks (pcx_create_devices) each rank
     * writes its rescaled rows back as it finishes, so a failure elsewhere can leave some rows
     * rescaled and others not; the reference leaves them rescaled. */
    double *original, *filled;
    /* wpca intermediates (:317-326), optional: [E] weighted_mean, [E][E] covariance_matrix */
    double *weighted_mean, *covariance;
    /* scalars, always written (host memory inside this struct) */
    double  participation;        /* result["participation"]                             */
    double  avg_certainty;        /* result["avg_certainty"]                             */
    int32_t branch;               /* enum pcx_branch                                     */
    int32_t flags;                /* enum pcx_flag bits                                  */
    int32_t pi_iters;             /* power-iteration steps (incl. Gram squarings)        */
    int32_t components;           /* result["components"]: fixed-variance count, else -1 (:449, :610) */
    int32_t n_hard;               /* weighted medians / binary fills replayed in sequential float order */
    int32_t sel_passes;           /* weighted-selection histogram passes                 */
    double  comm_bytes;           /* bytes this rank passed to collectives (all-reduce buffers + all-gather sends) */
    int32_t grid_events;          /* grid events (binary, filled values on {1, 1.5, 2}) past the general 128-event tiles:
                                     their covariance block ran on int8 MFMA */
    int32_t mixed_int8;           /* bit 0: general x grid pairs ran on int8 digit slices too (else fp64 MFMA);
                                     bit 1: and the general x general pairs (digits of tok w x digits of w) */
    /* the int8 covariance's guard (mixed_int8 != 0): an upper bound, rigorous in exact arithmetic, on
     * |C_pq - C~_pq| / sqrt(C_pp C_qq) over the entries with a general position, where C~ is the
     * covariance of the fp64 centred matrix wcd (:322-326) and C the emulation's result.  Above
     * 2^-40 the covariance is recomputed: cov_guard 1 = the remaining digit pairs (i + j >= NDIG, every
     * digit product exact), 2 = the general pairs on fp64 MFMA (k_syrk, as without int8).  0 = passed. */
    int32_t cov_guard;
    int32_t cov_guard_cols;       /* general events whose own bound (the pair (p, p)) exceeded 2^-40   */
    double  cov_err_bound;        /* the bound of the emulation that ran first (before any recompute)  */
} pcx_result;

/* The whole consensus (__init__.py:502-611) on this rank's rows; collective over
 * the context's ranks.  Synchronous: returns after every output is written. */
int pcx_consensus_f64(pcx_ctx* ctx, const pcx_problem* p, pcx_result* r);

/* The reference's stage methods on the same kernels (Oracle.interpolate / wpca /
 * lie_detector / nonconformity(_rank), __init__.py:260-500).
 *   pcx_interpolate_f64: p->reports raw; writes original / filled (:260-313).
 *   pcx_wpca_f64:        p->reports is a FILLED matrix (no NA handling); writes
 *                        weighted_mean, covariance, adj_first_loadings (first
 *                        loading) and scores (first score) (:315-339).
 *   pcx_lie_detector_f64: p->reports FILLED; wpca + nonconformity_rank (PCA) or
 *                        the algorithm's branch, then this_rep / smooth_rep
 *                        (:341-473); writes scores, adj_first_loadings, old_rep,
 *                        this_rep, smooth_rep, branch.
 *   pcx_nonconformity_f64: p->reports FILLED, scores [n_rows] given; rank_rule 1 =
 *                        nonconformity_rank (:487-500), 0 = nonconformity (:475-485);
 *                        writes nc [n_rows] and r->branch. */
int pcx_interpolate_f64(pcx_ctx* ctx, const pcx_problem* p, pcx_result* r);
int pcx_wpca_f64(pcx_ctx* ctx, const pcx_problem* p, pcx_result* r);
int pcx_lie_detector_f64(pcx_ctx* ctx, const pcx_problem* p, pcx_result* r);
int pcx_nonconformity_f64(pcx_ctx* ctx, const pcx_problem* p, const double* scores, int rank_rule, double* nc,
                          pcx_result* r);

/* Per-stage device time of the last single-matrix call (HIP events on the
 * context's stream) when enabled; names by pcx_stage_name(k), k < PCX_NSTAGES. */
#define PCX_NSTAGES 56
int         pcx_profile_enable(pcx_ctx* ctx, int on);
int         pcx_profile_read(pcx_ctx* ctx, double* ms /* [PCX_NSTAGES] */);
const char* pcx_stage_name(int k);
/* Progress of the single-matrix call running on `ctx` (safe to call from another
 * thread while it runs): *stage = the last stage enqueued (pcx_stage_name; -1 before
 * the first), *host_waiting = 1 while the host blocks on the context's stream (a
 * collective waiting for a peer shows as a wait after M_EXCHANGE or a later stage).
 * A multi-device context reports device 0's worker. */
int pcx_ctx_progress(const pcx_ctx* ctx, int* stage, int* host_waiting);

/* Sequential float sums of a constant (weightedstats' builtin-sum walk over equal
 * weights, __init__.py:287-303, :519-523): S(k) = 0 + c + c + ... (k terms, each
 * addition rounded to nearest-even), in O(log k) by binade stepping; and the least
 * k >= 1 with S(k) > t (kmax + 1 if none up to kmax).  Exported for the CPU tests. */
double  pcx_seqsum_const(double c, int64_t k);
int64_t pcx_seqsum_first_above(double c, double t, int64_t kmax);

/* Build parameter: balanced base-254 int8 digits per general event in the covariance's mixed block
 * (pcx_result.mixed_int8 bit 0; the int8 work per row is then grid pairs + digits x general x grid,
 * plus digits (digits + 1) / 2 x the general pairs with bit 1).  For roofline accounting. */
int pcx_mixed_digits(void);

/* The RCCL that serves libpcx's collectives: *runtime = ncclGetVersion() of the librccl the
 * process resolved (with torch loaded first: torch's bundled copy), *compiled = the
 * NCCL_VERSION_CODE of the headers libpcx was built against.  Returns *runtime.  RCCL
 * contexts are refused (PCX_ECOMM, both versions named) unless the major versions agree and
 * the runtime is >= 2.18 (version code 21800). */
int pcx_rccl_version(int* runtime, int* compiled);

/* CPU self-test of the communicator abort path (no RCCL, no GPU): `users` threads run
 * exchanges on a fake handle while `aborters` threads abort it.  Returns the number of
 * violations (the handle freed other than exactly once, used after it was freed, or used
 * successfully after an abort returned); 0 = pass, -1 = bad arguments.  For the tests. */
int pcx_selftest_abort_once(int users, int aborters, int iters);
/* The same abort path when one user is blocked inside its exchange for twice the abort's wait
 * (an RCCL enqueue stuck on a failed peer): every abort must return after the bounded wait, free
 * the handle exactly once (overlapping the blocked use: the documented window, counted once) and
 * fail every later use.  Returns the number of violations; 0 = pass, -1 = bad arguments. */
int pcx_selftest_abort_slow_holder(int users, int aborters);
/* CPU self-test of the virtual-rank exchange (pcx_group, as pcx_create_grouped /
 * pcx_create_devices use it): `world` threads run `steps` slot exchanges; rank `fail_rank`
 * fails at step `fail_step` (-1: none), the first failure aborts the group and must release
 * every waiting rank; after a reset a clean run must pass.  Returns the number of violations. */
int pcx_selftest_group_abort(int world, int steps, int fail_rank, int fail_step);
/* CPU self-test of the round scheduler's hand-out (pcx_consensus_batched_f64 above 256 x 64):
 * `workers` threads take `rounds` fake rounds; worker `enomem_worker` reports PCX_ENOMEM on its
 * first round (-1: none) and must hand it back; round `fail_round` fails (-1: none) and must stop
 * the batch.  Every round must run exactly once.  Returns the number of violations. */
int pcx_selftest_rounds_sched(int workers, int64_t rounds, int enomem_worker, int64_t fail_round);
/* CPU self-test of the host-memory path's staged large copies (pinned slots, host threads):
 * `bytes` through `slots` slots of `chunk` bytes by `threads` threads, memcpy standing in for the
 * DMA; chunk `fail_chunk`'s transfer fails (-1: none) and must stop the copy.  Returns the number
 * of violations (data, a chunk moved twice or after the failure); 0 = pass, -1 = bad arguments. */
int pcx_selftest_chunked_copy(int64_t bytes, int64_t chunk, int slots, int threads, int64_t fail_chunk);
/* Test hook: the NEXT pcx_consensus_batched_f64 call on `ctx` that takes the round scheduler
 * makes its worker `worker` report PCX_ENOMEM for its first round without running it (the
 * hand-back path); -1 clears it.  Consumed by that call.  For the tests only. */
int pcx_test_inject_enomem(pcx_ctx* ctx, int worker);
/* Test hook: pcx_consensus_ragged_wide_f64 on `ctx` sizes its chunks of workgroup rounds to `bytes`
 * of scratch in place of 2 GB (a chunk holds at least one round); 0 restores the default.  Stays
 * set until changed.  For the tests only. */
int pcx_test_scratch_cap(pcx_ctx* ctx, int64_t bytes);
/* Dynamic LDS bytes one round of pcx_consensus_batched_f64 asks for (n_reporters <= 64, n_events
 * <= 32, algorithm as in pcx_batch): what bounds the rounds resident per CU (LDS is handed out in
 * 1,280-byte units of the CU's 160 KiB).  No device needed.  For the tests and the tools. */
int64_t pcx_batched_lds_bytes(int n_reporters, int n_events, int algorithm);
/* The same for the workgroup-per-round kernel (rounds above 64 x 32 up to 256 x 64, every
 * algorithm): at most the 160 KiB a workgroup may use; 0 for a shape or algorithm it does not take. */
int64_t pcx_medium_lds_bytes(int n_reporters, int n_events, int algorithm);

/* Where pcx_consensus_batched_f64 runs a batch of n_reporters x n_events rounds: one wavefront per
 * round (up to 64 x 32), one workgroup per round (up to 256 x 64; k-means with kmeans_k <= 16), both
 * ONE asynchronous launch, or the round scheduler (host threads, returns when every output is
 * written).  kmeans_k matters for PCX_ALG_KMEANS only.  -1: arguments that call would refuse.  A
 * pure function of its arguments -- no context, no device, and the PCX_NO_MEDIUM diagnostic override
 * is not consulted; pcx_consensus_batched_f64 decides with the same code. */
enum pcx_route { PCX_ROUTE_WAVE = 0, PCX_ROUTE_WORKGROUP = 1, PCX_ROUTE_SCHEDULER = 2, PCX_ROUTE_TALL = 3 };
int pcx_batched_route(int n_reporters, int n_events, int algorithm, int kmeans_k);

/* The tall entry's routes (added under ABI 9; detect by symbol).  pcx_tall_route: where
 * pcx_consensus_batched_tall_f64 runs a batch -- pcx_batched_route's value, except PCX_ROUTE_TALL (3)
 * for 256 < n_reporters <= 1024, n_events <= 64 and an algorithm and shape whose LDS plan fits.  Pure,
 * like pcx_batched_route.  pcx_tall_lds_bytes: the dynamic LDS of one such round, at most 160 KiB less
 * the kernel's static LDS; 0 where the route is not PCX_ROUTE_TALL.  pcx_tall_plan: the plan itself,
 * out = {waves that run weighted medians and certainties side by side (4, 2 or 1), reporter rows per
 * chunk of np.dot's four-row block partials, the number of such chunks (the last may be shorter; 1
 * for n_events == 1), threads per workgroup}; PCX_EINVAL (out zeroed) where the route is not
 * PCX_ROUTE_TALL.  The dynamic LDS is 8 * (max(E (E + 1) [twice for big-five and fixed-variance],
 * waves * (2 N + 5 P / 2) [P = the power of two >= N], rows / 4 * E4 + (E - E4) * N [E4 = E & ~3; 0 for
 * E == 1]) + 11 N + 22 E) + 4 * ((N E + 15) >> 4) + 16 bytes. */
int pcx_tall_route(int n_reporters, int n_events, int algorithm, int kmeans_k);
int64_t pcx_tall_lds_bytes(int n_reporters, int n_events, int algorithm);
int pcx_tall_plan(int n_reporters, int n_events, int algorithm, int32_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* PCX_H */
