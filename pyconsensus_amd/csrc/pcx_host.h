// pcx_host.h -- what the host files of the extern "C" boundary share: pcx_api.cpp (contexts, the
// single-matrix and batched entries), pcx_ragged.cpp (ragged batches) and pcx_simulate.cpp (the
// Monte Carlo simulator).  Host code only; no .hip unit includes it.  Everything here is hidden:
// the library exports what include/pcx.h declares and no more.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "../../include/pcx.h"
#include "pcx_internal.h"

namespace pcx {
namespace host __attribute__((visibility("hidden"))) {

// ---------------------------------------------------------------- pcx_api.cpp
extern thread_local std::string g_err;  // what pcx_last_error returns
int fail(int code, const std::string& msg);
int hip_fail(hipError_t e, const char* what);

// The option checks that pcx_consensus_batched_f64 ("batched") and pcx_consensus_ragged_f64
// ("ragged") share, in the order both make them.  `own` is what the entry's own checks found (the
// algorithm's range, k-means, big-five; NULL: nothing): they follow reports / scaled and precede
// catch_tolerance / alpha, and each of them, like each check here that names an algorithm, can
// only fire alone, so one place among those serves both entries.
template <class In>
int check_options(const char* who, const In* in, const char* own) {
    auto refuse = [who](const char* why) { return fail(PCX_EINVAL, std::string(who) + ": " + why); };
    if (!in->reports) return refuse("reports is NULL");
    if (in->scaled && (!in->lo || !in->hi)) return refuse("scaled given without lo/hi");
    if (own) return refuse(own);
    if (in->algorithm == PCX_ALG_HIERARCHICAL && std::isnan(in->hierarchy_threshold))
        return refuse("hierarchy_threshold is NaN");
    if (in->algorithm == PCX_ALG_FIXED_VARIANCE && !std::isfinite(in->variance_threshold))
        return refuse("variance_threshold must be finite");
    if (in->algorithm == PCX_ALG_COKURTOSIS && !in->aux_scores)
        return refuse("cokurtosis needs aux_scores (aux[\"cokurt\"])");
    if (!std::isfinite(in->catch_tolerance) || !std::isfinite(in->alpha))
        return refuse("catch_tolerance/alpha must be finite");
    return PCX_OK;
}

// what pcx_batch and pcx_ragged both carry: the inputs, the algorithm's options and every output
template <class In>
pcx::BatchArgs shared_args(const In* in, const pcx_batch_result* out) {
    pcx::BatchArgs a{};
    a.reports = in->reports;
    a.reputation = in->reputation;
    a.scaled = in->scaled;
    a.lo = in->lo;
    a.hi = in->hi;
    a.int_dtype = in->int_dtype;
    a.algorithm = in->algorithm;
    a.max_components = in->max_components;
    a.variance_threshold = in->variance_threshold;
    a.aux_scores = in->aux_scores;
    a.hierarchy_threshold = in->hierarchy_threshold;
    a.cluster_threshold = in->cluster_threshold;
    a.catch_tol = in->catch_tolerance;
    a.alpha = in->alpha;
    a.old_rep = out->old_rep;
    a.this_rep = out->this_rep;
    a.smooth_rep = out->smooth_rep;
    a.scores = out->scores;
    a.na_row = out->na_row;
    a.participation_rows = out->participation_rows;
    a.relative_part = out->relative_part;
    a.reporter_bonus = out->reporter_bonus;
    a.adj_first_loadings = out->adj_first_loadings;
    a.outcomes_raw = out->outcomes_raw;
    a.outcomes_adjusted = out->outcomes_adjusted;
    a.outcomes_final = out->outcomes_final;
    a.certainty = out->certainty;
    a.consensus_reward = out->consensus_reward;
    a.nas_filled = out->nas_filled;
    a.participation_columns = out->participation_columns;
    a.author_bonus = out->author_bonus;
    a.participation = out->participation;
    a.avg_certainty = out->avg_certainty;
    a.branch = out->branch;
    a.flags = out->flags;
    a.pi_iters = out->pi_iters;
    a.components = out->components;
    a.original = out->original;
    a.filled = out->filled;
    return a;
}

// The PCX_STAMPS diagnostic's buffer (per-phase shader clocks, [B][32]): allocated and zeroed on
// the stream when the variable is "1" -- a.stamps stays NULL otherwise, and when there are no rounds
// or no memory -- then, after the launches, read back (the stream is synchronised) and freed.
void stamps_begin(pcx::BatchArgs& a, hipStream_t stream);
std::vector<long long> stamps_end(pcx::BatchArgs& a, hipStream_t stream);

// one workgroup per round (pcx_medium.hip), in chunks of bounded scratch
constexpr size_t MEDIUM_SCRATCH_CAP = (size_t)2 << 30;
// the context's workgroup scratch (pcx_ctx.mscr) grown to `need` bytes; 0 = ok
int medium_scratch_reserve(pcx_ctx* ctx, size_t need);

// ---------------------------------------------------------------- pcx_ragged.cpp
// This call's staging slot (the two are taken in turn), with room for `bytes` on both sides and the
// host side free to be rewritten: the slot's last upload has read it.  0 = ok.
int ragged_slot_take(pcx_ctx* ctx, size_t bytes, pcx_ctx::RaggedSlot** slot);
// The slot's first `bytes` from the staging to the device table on the stream, after any launch
// that still reads the table (another stream's, maybe); copy_ev marks the staging read.
hipError_t ragged_slot_upload(pcx_ctx* ctx, pcx_ctx::RaggedSlot& s, size_t bytes);

// where a round of a wide ragged batch runs: 0 = the one-wave kernel, else the workgroup kernel's
// launch class (pcx::medium_launch_class), or the one class of PCX_RAGGED_ONE_CLASS
int wide_slot(int N, int E, int algorithm, bool one_class);

// why a parameter set is refused (the words of check_options), or NULL.  sim: a simulator's set,
// where k-means and cokurtosis are not simulated.  kmeans_ok: an entry that takes or draws code books.
const char* params_set_refusal(const pcx_round_params& q, bool sim, bool kmeans_ok = false);

// the shared parameter fields of a pcx_sim / pcx_sim_sweep as a set
template <class S>
pcx_round_params shared_set(const S* s) {
    return pcx_round_params{s->algorithm,          s->max_components,      s->catch_tolerance,  s->alpha,
                            s->variance_threshold, s->hierarchy_threshold, s->cluster_threshold};
}

// the reference's code-book size int(ceil(sqrt(N))) (:396), in integers
int64_t kmeans_rule(int64_t N);

// The flat book layout of the rounds whose set params[param_of[b]] is k-means (params NULL: every
// round), of rounds whose shapes the caller has checked: offsets[b] = the books before round b's,
// offsets[B] the length.  Refuses a k_b outside [1, min(N_b, 8)] within 64 x 32 (the one-wave
// kernel's code-book rows), [1, min(N_b, 16)] above (the workgroup kernel's), with the round named.
int kmeans_layout(int64_t B, const int32_t* n_reporters, const int32_t* n_events, const int32_t* k, int restarts,
                  const pcx_round_params* params, const int32_t* param_of, int64_t* offsets,
                  pcx::KmeansEntry* entries, int64_t* bad_round, int64_t* total = nullptr);

// The descriptor tables of one ragged call in a staging slot, and what its launches need of them.
// They depend on the rounds' shapes and algorithms alone: an entry builds them, uploads them and
// launches once; a sweep builds and uploads them once and launches every timestep.  Two layouts:
//   plan_shared: the wave rounds' RaggedDesc, the workgroup rounds' MediumDesc class after class
//     (3, 2, 1), the wave rounds' indices; cnt / lds / first by launch class 0..3.
//   plan_table: every round's MediumDesc, segment after segment, then the P parameter entries; cnt /
//     lds / first by segment -- 0..2 the one-wave kernel's groups (pcx::params_wave_group), 3..5 the
//     workgroup kernel's plain instantiation in launch classes 3, 2, 1, 6..8 its CLUS one likewise.
// A class's or segment's rounds keep their order; `extra` bytes (a multiple of 8) ride at off_x.
constexpr int PLAN_SEGMENTS = 9;
struct RaggedPlan {
    pcx_ctx::RaggedSlot* slot = nullptr;
    bool table = false;  // the parameter-table layout
    int64_t B = 0, nw = 0, nm = 0;  // rounds; the one-wave kernel's and the workgroup kernel's
    int64_t cnt[PLAN_SEGMENTS] = {}, lds[PLAN_SEGMENTS] = {}, first[PLAN_SEGMENTS] = {};
    // shared: the workgroup descriptors, the wave rounds' indices and, on the device past what is
    // uploaded, the wave rounds' six [B] outputs until their scatter; table: the parameter entries
    size_t off_m = 0, off_i = 0, off_t = 0, off_p = 0, off_x = 0, bytes = 0;
    // the workgroup scratch (plan_scratch): slot strides of the call's largest round, rounds per chunk,
    // and its three parts inside pcx_ctx.mscr -- valid until the context's next medium_scratch_reserve,
    // so a plan is built and launched within one call
    int64_t stride[3] = {0, 0, 0}, chunk = 0;
    double *Fscr = nullptr, *Cscr = nullptr, *Xscr = nullptr;
    bool filled = false;  // the caller gives `filled`: no N x E scratch of the library's
    // The tall segment of a table plan built with tall = true: the rounds above 256
    // reporters, their descriptors behind the nine segments' at tall_first, one launch class whatever
    // their algorithms (a tall round's LDS leaves one round per CU), tall_lds the largest round's
    // plan.  Slot strides and a chunk of its own -- a 1024 x 64 round must not shrink the chunks of
    // the call's 100 x 50 rounds -- over the same scratch: the stream runs the segments one after
    // another.  All zero without a tall round, and every other field is then what it was.
    int64_t n_tall = 0, tall_first = 0, tall_lds = 0, tall_stride[2] = {0, 0}, tall_chunk = 0;
    double *tall_Fscr = nullptr, *tall_Cscr = nullptr;

    // The launches over the uploaded tables: wave rounds first (shared: then their scatter), then the
    // workgroup rounds in chunks of the scratch.  books (table layout; NULL: none): the per-round book
    // table on the device -- the clustering segments (2, 6..8) then run their kernels' k-means form.
    hipError_t launch(pcx_ctx* ctx, const pcx::BatchArgs& a, const pcx::KmeansEntry* books = nullptr) const;
};
// A plan's tables into a staging slot taken here, the workgroup scratch reserved; 0 = ok.  The
// rounds are checked.  plan_shared: cnt / lds per launch class as the caller's plan pass found them;
// wave_table_alone: with wave-sized rounds only, the wave descriptors alone (the entries; a sweep: false).
int plan_shared(pcx_ctx* ctx, int64_t B, const int32_t* n_reporters, const int32_t* n_events, int algorithm,
                bool one_class, const int64_t cnt[4], const int64_t lds[4], bool filled, size_t extra,
                bool wave_table_alone, RaggedPlan* plan);
int plan_table(pcx_ctx* ctx, int64_t B, const int32_t* n_reporters, const int32_t* n_events, int64_t n_params,
               const pcx_round_params* params, const int32_t* param_of, bool filled, size_t extra, RaggedPlan* plan);

// Why a round of N > 256 reporters is refused by the entries that take rounds up to 1024 (the ragged
// tall entry, the tall study): "N x E under <algorithm>; <reason>" where pcx_tall_route is not
// PCX_ROUTE_TALL -- a clustering, or an LDS plan that does not fit; empty where the round is taken.
std::string tall_round_refusal(int N, int E, int algorithm);

}  // namespace host
}  // namespace pcx
