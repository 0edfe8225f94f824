// pcx_simulate.cpp -- the Monte Carlo simulator's entries of include/pcx.h (rounds, sweeps of cells,
// studies): their checks, the work buffers and the timestep loops.  Host code only; the consensus
// launches are pcx_consensus_batched_f64's and a ragged plan's (pcx_host.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/pcx.h"
#include "pcx_host.h"
#include "pcx_internal.h"
#include "pcx_sim_study.h"
#include "pcx_sim_sweep.h"

using namespace pcx::host;

// the first of a pcx_sim's or a pcx_sim_cell's five rates that is no probability (NaN too), or NULL
template <class S>
static const char* bad_probability(const S& s) {
    const struct {
        const char* name;
        double p;
    } probs[] = {{"liar_frac", s.liar_frac}, {"collude_frac", s.collude_frac}, {"distort", s.distort},
                 {"na_frac", s.na_frac},     {"scaled_frac", s.scaled_frac}};
    for (const auto& q : probs)
        if (!(q.p >= 0.0 && q.p <= 1.0)) return q.name;  // false for NaN too
    return nullptr;
}

extern "C" {
namespace {
uint64_t sim_threshold(double p) { return (uint64_t)std::floor(p * 4294967296.0); }
}  // namespace
}

// the generator's key and 32-bit thresholds of a pcx_sim's or a pcx_sim_cell's seed and rates
template <class S>
static pcx::sim::Gen gen_of(const S& s) {
    pcx::sim::Gen g;
    g.key0 = (uint32_t)s.seed;
    g.key1 = (uint32_t)(s.seed >> 32);
    g.thr_liar = sim_threshold(s.liar_frac);
    g.thr_collude = sim_threshold(s.collude_frac);
    g.thr_distort = sim_threshold(s.distort);
    g.thr_na = sim_threshold(s.na_frac);
    g.thr_scaled = sim_threshold(s.scaled_frac);
    return g;
}

extern "C" {

// ---------------------------------------------------------------- Monte Carlo simulator
namespace {
// the argument checks every simulator entry shares (no device needed); 0 = ok
// (kmeans_ok: an entry that draws the code books on the device)
int sim_check(const pcx_sim* s, const char* who, bool kmeans_ok = false) {
    const std::string w = std::string(who) + ": ";
    if (s->n_rounds < 0 || s->n_rounds > 0x7fffffff) return fail(PCX_EINVAL, w + "n_rounds must be in [0, 2^31)");
    if (s->n_reporters < 1 || s->n_reporters > 0x7fffffff)
        return fail(PCX_EINVAL, w + "n_reporters must be in [1, 2^31)");
    if (s->n_events < 1 || s->n_events > 65536) return fail(PCX_EINVAL, w + "n_events must be in [1, 65536]");
    if (s->n_timesteps < 1 || s->n_timesteps >= (1 << 24))
        return fail(PCX_EINVAL, w + "n_timesteps must be in [1, 2^24)");
    if (const char* name = bad_probability(*s)) return fail(PCX_EINVAL, w + name + " must be a probability in [0, 1]");
    if (!(s->scaled_tol >= 0.0) || !std::isfinite(s->scaled_tol))
        return fail(PCX_EINVAL, w + "scaled_tol must be finite and >= 0");
    // what pcx_consensus_batched_f64 would refuse, before anything is generated: big-five by the one
    // shape (it fires alone, like every check of a set that names an algorithm), the rest as a set
    if (s->algorithm == PCX_ALG_BIG_FIVE && (s->max_components < 1 || s->max_components > s->n_events))
        return fail(PCX_EINVAL, w + "big-five needs 1 <= max_components <= n_events");
    if (const char* why = params_set_refusal(shared_set(s), true, kmeans_ok)) return fail(PCX_EINVAL, w + why);
    return PCX_OK;
}

int sim_check_timestep(int t, const char* who) {
    if (t < 0 || t >= (1 << 24)) return fail(PCX_EINVAL, std::string(who) + ": timestep must be in [0, 2^24)");
    return PCX_OK;
}

pcx::sim::Gen sim_gen(const pcx_sim* s) { return gen_of(*s); }

int sim_reserve(pcx_ctx* ctx, size_t need) {
    if (ctx->sim_bytes >= need) return PCX_OK;
    pcx::sim_free(ctx);
    const hipError_t e = hipMalloc(&ctx->sim_buf, need);
    if (e != hipSuccess) {
        ctx->sim_buf = nullptr;
        return fail(e == hipErrorOutOfMemory ? PCX_ENOMEM : PCX_EHIP,
                    std::string("pcx_simulate_f64: hipMalloc(work buffers): ") + hipGetErrorString(e));
    }
    ctx->sim_bytes = need;
    return PCX_OK;
}

// One simulator call's work buffers and a timestep's view of them.  Doubles first: reports [bne], lo,
// hi, truth, outcomes_final [be], old_rep and two smooth_rep [bn] (ping-pong: a timestep reads one as
// its reputation and writes the other), metrics, a study's detail; then the bytes scaled [be] and
// liar [bn]; then the k-means books, int32 on a 4-byte boundary.  bne / be / bn: the cells, events
// and reporters of the call's rounds together.
struct SimFrame {
    pcx_sim_rounds work;
    double *outcomes, *old_rep, *smooth[2], *metrics, *detail;
    int32_t* books;

    // the context's work buffers grown to this layout, and carved; 0 = ok
    int carve(pcx_ctx* ctx, size_t bne, size_t be, size_t bn, size_t n_metrics, size_t n_detail, size_t n_books) {
        const size_t n_f64 = bne + 4 * be + 3 * bn + n_metrics + n_detail;
        const size_t off_books = (n_f64 * sizeof(double) + be + bn + 3) / 4 * 4;
        if (const int rc = sim_reserve(ctx, std::max<size_t>(off_books + n_books * sizeof(int32_t), 16))) return rc;
        books = reinterpret_cast<int32_t*>(static_cast<char*>(ctx->sim_buf) + off_books);
        double* p = (double*)ctx->sim_buf;
        auto take = [&p](size_t n) {
            double* q = p;
            p += n;
            return q;
        };
        work.reports = take(bne);
        work.lo = take(be);
        work.hi = take(be);
        work.truth = take(be);
        outcomes = take(be);
        old_rep = take(bn);
        smooth[0] = take(bn);
        smooth[1] = take(bn);
        metrics = take(n_metrics);
        detail = take(n_detail);
        work.scaled = (uint8_t*)p;
        work.liar = work.scaled + be;
        return PCX_OK;
    }

    // timestep t's generated rounds and consensus outputs: the work buffers, and on the last
    // timestep the caller's buffers where given
    void at(int64_t t, bool last, const pcx_sim_result* res, pcx_sim_rounds* r, pcx_batch_result* o) const {
        *r = work;
        *o = pcx_batch_result{};
        if (last) {
            const pcx_sim_rounds& u = res->last;
            if (u.reports) r->reports = u.reports;
            if (u.scaled) r->scaled = u.scaled;
            if (u.lo) r->lo = u.lo;
            if (u.hi) r->hi = u.hi;
            if (u.truth) r->truth = u.truth;
            if (u.liar) r->liar = u.liar;
            *o = res->last_out;
        }
        if (!o->old_rep) o->old_rep = old_rep;
        if (!o->smooth_rep) o->smooth_rep = smooth[t & 1];
        if (!o->outcomes_final) o->outcomes_final = outcomes;
    }
};
}  // namespace

void pcx_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
    const pcx::sim::U4 r = pcx::sim::philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1]);
    out[0] = r.w0;
    out[1] = r.w1;
    out[2] = r.w2;
    out[3] = r.w3;
}

int pcx_sim_generate_host(const pcx_sim* sim, int timestep, pcx_sim_rounds* out) {
    if (!sim || !out) return fail(PCX_EINVAL, "pcx_sim_generate_host: null argument");
    if (const int rc = sim_check(sim, "pcx_sim_generate_host")) return rc;
    if (const int rc = sim_check_timestep(timestep, "pcx_sim_generate_host")) return rc;
    pcx::sim_generate_host(sim_gen(sim), sim->n_rounds, sim->n_reporters, sim->n_events, (uint32_t)timestep, *out);
    return PCX_OK;
}

int pcx_sim_generate_f64(pcx_ctx* ctx, const pcx_sim* sim, int timestep, pcx_sim_rounds* out) {
    if (!ctx || !sim || !out) return fail(PCX_EINVAL, "pcx_sim_generate_f64: null argument");
    if (const int rc = sim_check(sim, "pcx_sim_generate_f64")) return rc;
    if (const int rc = sim_check_timestep(timestep, "pcx_sim_generate_f64")) return rc;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    e = pcx::launch_sim_generate(sim_gen(sim), sim->n_rounds, sim->n_reporters, sim->n_events, (uint32_t)timestep,
                                 *out, ctx->stream);
    return e == hipSuccess ? PCX_OK : hip_fail(e, "k_sim_generate launch");
}

int pcx_sim_metrics_f64(pcx_ctx* ctx, const pcx_sim* sim, const pcx_sim_rounds* rounds, const double* old_rep,
                        const double* smooth_rep, const double* outcomes_final, double* metrics, double* summary) {
    if (!ctx || !sim || !rounds || !old_rep || !smooth_rep || !outcomes_final || !metrics)
        return fail(PCX_EINVAL, "pcx_sim_metrics_f64: null argument");
    if (!rounds->scaled || !rounds->lo || !rounds->hi || !rounds->truth || !rounds->liar)
        return fail(PCX_EINVAL, "pcx_sim_metrics_f64: rounds needs scaled, lo, hi, truth and liar");
    if (const int rc = sim_check(sim, "pcx_sim_metrics_f64")) return rc;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    e = pcx::launch_sim_metrics(sim->n_rounds, sim->n_reporters, sim->n_events, sim->scaled_tol, *rounds, old_rep,
                                smooth_rep, outcomes_final, metrics, ctx->stream);
    if (e == hipSuccess && summary) e = pcx::launch_sim_summary(metrics, sim->n_rounds, summary, ctx->stream);
    return e == hipSuccess ? PCX_OK : hip_fail(e, "k_sim_metrics / k_sim_summary launch");
}

// restarts / (rounds x restarts) that the books kernels take: one thread each, at most 2^31 - 1 workgroups
static int sim_books_check(int64_t B, int restarts, const std::string& who) {
    if (restarts < 1) return fail(PCX_EINVAL, who + ": k-means restarts must be >= 1");
    if ((B * (int64_t)restarts + 255) / 256 > 0x7fffffff)
        return fail(PCX_EINVAL, who + ": rounds x restarts is too large for one books launch");
    return PCX_OK;
}

// The loop of pcx_simulate_f64 and pcx_simulate_kmeans_f64 (`who`).  restarts > 0: the latter, under
// k-means -- every timestep's books are drawn into the workspace between the generator and the
// batched launch, which reads them as kmeans_init.
// tall (pcx_simulate_tall_f64): the consensus step is pcx_consensus_batched_tall_f64.
static int simulate_run(pcx_ctx* ctx, const pcx_sim* sim, pcx_sim_result* res, int restarts, const char* who,
                        bool tall = false) {
    if (const int rc = sim_check(sim, who, restarts > 0)) return rc;
    const bool km = restarts > 0 && sim->algorithm == PCX_ALG_KMEANS;
    const int64_t kk = km ? kmeans_rule(sim->n_reporters) : 0;
    if (km)
        if (const int rc = sim_books_check(sim->n_rounds, restarts, who)) return rc;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    const int64_t B = sim->n_rounds, N = sim->n_reporters, E = sim->n_events, T = sim->n_timesteps;
    const size_t bn = (size_t)B * N, be = (size_t)B * E;
    // (k-means: the books [B][restarts][k])
    SimFrame w;
    if (const int rc = w.carve(ctx, bn * E, be, bn, (size_t)B * PCX_SIM_NMETRICS, 0, km ? (size_t)B * restarts * kk : 0))
        return rc;
    const pcx::sim::Gen g = sim_gen(sim);
    const double* rep = sim->reputation0;
    for (int64_t t = 0; t < T; t++) {
        pcx_sim_rounds r;
        pcx_batch_result o;
        w.at(t, t == T - 1, res, &r, &o);
        e = pcx::launch_sim_generate(g, B, N, E, (uint32_t)t, r, ctx->stream);
        if (e != hipSuccess) return hip_fail(e, "k_sim_generate launch");
        pcx_batch in{};
        in.n_rounds = B;
        in.n_reporters = N;
        in.n_events = E;
        in.reports = r.reports;
        in.reputation = rep;
        in.scaled = r.scaled;
        in.lo = r.lo;
        in.hi = r.hi;
        in.catch_tolerance = sim->catch_tolerance;
        in.alpha = sim->alpha;
        in.algorithm = sim->algorithm;
        in.max_components = sim->max_components;
        in.variance_threshold = sim->variance_threshold;
        in.hierarchy_threshold = sim->hierarchy_threshold;
        in.cluster_threshold = sim->cluster_threshold;
        if (km) {
            e = pcx::launch_sim_kmeans_books(g, B, (int)N, (int)kk, restarts, (uint32_t)t, w.books, ctx->stream);
            if (e != hipSuccess) return hip_fail(e, "k_kmeans_books launch");
            in.kmeans_k = (int32_t)kk;
            in.kmeans_restarts = restarts;
            in.kmeans_init = w.books;
        }
        if (const int rc = tall ? pcx_consensus_batched_tall_f64(ctx, &in, &o) : pcx_consensus_batched_f64(ctx, &in, &o))
            return rc;
        if (res->metrics || res->summary) {
            double* m = res->metrics ? res->metrics + (size_t)t * B * PCX_SIM_NMETRICS : w.metrics;
            e = pcx::launch_sim_metrics(B, N, E, sim->scaled_tol, r, o.old_rep, o.smooth_rep, o.outcomes_final, m,
                                        ctx->stream);
            if (e == hipSuccess && res->summary)
                e = pcx::launch_sim_summary(m, B, res->summary + (size_t)t * PCX_SIM_NMETRICS, ctx->stream);
            if (e != hipSuccess) return hip_fail(e, "k_sim_metrics / k_sim_summary launch");
        }
        rep = o.smooth_rep;  // the next timestep's reputation
    }
    if (res->reputation && bn) {
        e = hipMemcpyAsync(res->reputation, rep, bn * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream);
        if (e != hipSuccess) return hip_fail(e, "pcx_simulate_f64: reputation copy");
    }
    return PCX_OK;
}

int pcx_simulate_f64(pcx_ctx* ctx, const pcx_sim* sim, pcx_sim_result* res) {
    if (!ctx || !sim || !res) return fail(PCX_EINVAL, "pcx_simulate_f64: null argument");
    return simulate_run(ctx, sim, res, 0, "pcx_simulate_f64");
}

int pcx_simulate_tall_f64(pcx_ctx* ctx, const pcx_sim* sim, pcx_sim_result* res) {
    if (!ctx || !sim || !res) return fail(PCX_EINVAL, "pcx_simulate_tall_f64: null argument");
    return simulate_run(ctx, sim, res, 0, "pcx_simulate_tall_f64", true);
}

int pcx_simulate_kmeans_f64(pcx_ctx* ctx, const pcx_sim* sim, int32_t restarts, pcx_sim_result* res) {
    if (!ctx || !sim || !res) return fail(PCX_EINVAL, "pcx_simulate_kmeans_f64: null argument");
    if (restarts < 1) return fail(PCX_EINVAL, "pcx_simulate_kmeans_f64: k-means restarts must be >= 1");
    return simulate_run(ctx, sim, res, restarts, "pcx_simulate_kmeans_f64");
}

int pcx_sim_kmeans_books_host(const pcx_sim* sim, int32_t restarts, int timestep, int32_t* books) {
    const char* who = "pcx_sim_kmeans_books_host";
    if (!sim || !books) return fail(PCX_EINVAL, std::string(who) + ": null argument");
    if (const int rc = sim_check(sim, who, true)) return rc;
    if (const int rc = sim_check_timestep(timestep, who)) return rc;
    if (const int rc = sim_books_check(sim->n_rounds, restarts, who)) return rc;
    pcx::sim_kmeans_books_host(sim_gen(sim), sim->n_rounds, (int)sim->n_reporters, (int)kmeans_rule(sim->n_reporters),
                               restarts, (uint32_t)timestep, books);
    return PCX_OK;
}

int pcx_sim_kmeans_books_f64(pcx_ctx* ctx, const pcx_sim* sim, int32_t restarts, int timestep, int32_t* books) {
    const char* who = "pcx_sim_kmeans_books_f64";
    if (!ctx || !sim || !books) return fail(PCX_EINVAL, std::string(who) + ": null argument");
    if (const int rc = sim_check(sim, who, true)) return rc;
    if (const int rc = sim_check_timestep(timestep, who)) return rc;
    if (const int rc = sim_books_check(sim->n_rounds, restarts, who)) return rc;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    e = pcx::launch_sim_kmeans_books(sim_gen(sim), sim->n_rounds, (int)sim->n_reporters,
                                     (int)kmeans_rule(sim->n_reporters), restarts, (uint32_t)timestep, books,
                                     ctx->stream);
    return e == hipSuccess ? PCX_OK : hip_fail(e, "k_kmeans_books launch");
}

// ---------------------------------------------------------------- simulator sweeps
namespace {
int sweep_fail(int64_t* bad_cell, int64_t c, const char* who, const std::string& why) {
    if (bad_cell) *bad_cell = c;
    return fail(PCX_EINVAL, std::string(who) + ": " + (c >= 0 ? "cell " + std::to_string(c) + ": " : "") + why);
}

// The checks every sweep entry shares (pure): the shared parameters as sim_check checks them
// (*bad_cell = -1), then cell after cell.  Fills what pcx_sim_sweep_plan reports; 0 = ok.
// cp: per-cell parameter sets [C] (NULL: the shared parameters) -- the shared ones are then neither
// read nor checked, each cell's set is checked with the cell, and its rounds count by its algorithm.
// kmeans_ok: an entry that draws the code books on the device -- k-means passes, shared or in a set.
// tall: the tall study's entries -- cells within [1, 1024] x [1, 64]; a cell above 256 reporters must
// be of the tall route under its algorithm and counts in no launch class (*any_tall: there is one).
int sweep_check(const pcx_sim_sweep* s, const char* who, int64_t totals[4], int64_t counts[4], int64_t lds_bytes[4],
                int64_t* bad_cell, const pcx_round_params* cp = nullptr, bool kmeans_ok = false, bool tall = false,
                bool* any_tall = nullptr) {
    const int max_n = tall ? 1024 : 256;
    if (any_tall) *any_tall = false;
    if (bad_cell) *bad_cell = -1;
    if (s->n_cells < 0) return sweep_fail(bad_cell, -1, who, "n_cells must be >= 0");
    if (s->n_cells > 0 && !s->cells) return sweep_fail(bad_cell, -1, who, "cells is NULL");
    if (s->n_timesteps < 1 || s->n_timesteps >= (1 << 24))
        return sweep_fail(bad_cell, -1, who, "n_timesteps must be in [1, 2^24)");
    if (!(s->scaled_tol >= 0.0) || !std::isfinite(s->scaled_tol))
        return sweep_fail(bad_cell, -1, who, "scaled_tol must be finite and >= 0");
    if (!cp)  // (else each cell's own set, below)
        if (const char* why = params_set_refusal(shared_set(s), true, kmeans_ok)) return sweep_fail(bad_cell, -1, who, why);
    int64_t tot[4] = {0, 0, 0, 0}, cnt[4] = {0, 0, 0, 0};
    size_t lds[4] = {0, 0, 0, 0};
    for (int64_t c = 0; c < s->n_cells; c++) {
        const pcx_sim_cell& k = s->cells[c];
        if (k.n_reporters < 1 || k.n_reporters > max_n || k.n_events < 1 || k.n_events > 64)
            return sweep_fail(bad_cell, c, who,
                              "is " + std::to_string(k.n_reporters) + " x " + std::to_string(k.n_events) +
                                  "; a cell's rounds must be within [1, " + std::to_string(max_n) + "] x [1, 64]");
        if (k.n_rounds < 1 || k.n_rounds > 0x7fffffff)
            return sweep_fail(bad_cell, c, who, "n_rounds must be in [1, 2^31)");
        if (const char* name = bad_probability(k))
            return sweep_fail(bad_cell, c, who, std::string(name) + " must be a probability in [0, 1]");
        if (cp)
            if (const char* why = params_set_refusal(cp[c], true, kmeans_ok)) return sweep_fail(bad_cell, c, who, why);
        const int algorithm = cp ? cp[c].algorithm : s->algorithm;
        const int64_t R = k.n_rounds, N = k.n_reporters, E = k.n_events;
        tot[0] += R;
        if (tot[0] > 0x7fffffff)
            return sweep_fail(bad_cell, c, who, "the rounds up to this cell reach 2^31 (sum of n_rounds must be < 2^31)");
        tot[1] += R * N;
        tot[2] += R * E;
        tot[3] += R * N * E;
        if (N > 256) {  // (tall)
            const std::string why = tall_round_refusal((int)N, (int)E, algorithm);
            if (!why.empty()) return sweep_fail(bad_cell, c, who, "is " + why);
            if (any_tall) *any_tall = true;
            continue;
        }
        const int slot = wide_slot((int)N, (int)E, algorithm, false);
        cnt[slot] += R;
        lds[slot] = std::max(lds[slot], slot ? pcx::medium_lds_bytes((int)N, (int)E, algorithm)
                                             : pcx::ragged_lds_bytes((int)N, (int)E, algorithm));
    }
    for (int k = 0; k < 4 && totals; k++) totals[k] = tot[k];
    for (int k = 0; k < 4 && counts; k++) counts[k] = cnt[k];
    for (int k = 0; k < 4 && lds_bytes; k++) lds_bytes[k] = (int64_t)lds[k];
    return PCX_OK;
}

pcx::sim::Gen sweep_gen(const pcx_sim_cell& k) { return gen_of(k); }

// bytes of a checked sweep's tables: the cell table, then the round prefix sums [C + 1]
size_t sweep_table_bytes(const pcx_sim_sweep* s) {
    return (size_t)s->n_cells * sizeof(pcx::SweepCell) + (size_t)(s->n_cells + 1) * sizeof(int64_t);
}

// the tables of a checked sweep written at `host`; what the kernels get points at `dev`, where
// the caller uploads them
pcx::SweepTables sweep_tables_fill(const pcx_sim_sweep* s, void* host, const void* dev) {
    const int64_t C = s->n_cells;
    pcx::SweepCell* cells = static_cast<pcx::SweepCell*>(host);
    int64_t* prefix = reinterpret_cast<int64_t*>(cells + C);
    int64_t round = 0, cell = 0, row = 0, ev = 0;
    for (int64_t c = 0; c < C; c++) {
        const pcx_sim_cell& k = s->cells[c];
        const int64_t R = k.n_rounds, N = k.n_reporters, E = k.n_events;
        cells[c] = pcx::SweepCell{round, cell, row, ev, R, (int32_t)N, (int32_t)E, sweep_gen(k)};
        prefix[c] = round;
        round += R;
        cell += R * N * E;
        row += R * N;
        ev += R * E;
    }
    prefix[C] = round;
    pcx::SweepTables t;
    t.cells = static_cast<const pcx::SweepCell*>(dev);
    t.prefix = reinterpret_cast<const int64_t*>(t.cells + C);
    t.C = (int32_t)C;
    t.B = round;
    return t;
}
}  // namespace

// a checked sweep's tables through a staging slot of their own to the device, on the stream (the
// stand-alone generator and metrics entries); the caller records the slot's kern_ev after its launches
static int sweep_tables_upload(pcx_ctx* ctx, const pcx_sim_sweep* s, pcx_ctx::RaggedSlot** slot, pcx::SweepTables* t) {
    const size_t bytes = sweep_table_bytes(s);
    if (const int rc = ragged_slot_take(ctx, bytes, slot)) return rc;
    *t = sweep_tables_fill(s, (*slot)->pin, (*slot)->dev);
    const hipError_t e = ragged_slot_upload(ctx, **slot, bytes);
    return e == hipSuccess ? PCX_OK : hip_fail(e, "sweep: table upload");
}

int pcx_sim_sweep_plan(const pcx_sim_sweep* sweep, int64_t totals[4], int64_t counts[4], int64_t lds_bytes[4],
                       int64_t* bad_cell) {
    if (!sweep) return fail(PCX_EINVAL, "pcx_sim_sweep_plan: null argument");
    return sweep_check(sweep, "pcx_sim_sweep_plan", totals, counts, lds_bytes, bad_cell);
}

int pcx_sim_sweep_generate_host(const pcx_sim_sweep* sweep, int timestep, pcx_sim_rounds* rounds) {
    if (!sweep || !rounds) return fail(PCX_EINVAL, "pcx_sim_sweep_generate_host: null argument");
    if (const int rc = sweep_check(sweep, "pcx_sim_sweep_generate_host", nullptr, nullptr, nullptr, nullptr)) return rc;
    if (const int rc = sim_check_timestep(timestep, "pcx_sim_sweep_generate_host")) return rc;
    std::vector<char> tab(sweep_table_bytes(sweep));
    sweep_tables_fill(sweep, tab.data(), tab.data());
    pcx::sim_sweep_generate_host(reinterpret_cast<const pcx::SweepCell*>(tab.data()), sweep->n_cells,
                                 (uint32_t)timestep, *rounds);
    return PCX_OK;
}

int pcx_sim_sweep_generate_f64(pcx_ctx* ctx, const pcx_sim_sweep* sweep, int timestep, pcx_sim_rounds* rounds) {
    if (!ctx || !sweep || !rounds) return fail(PCX_EINVAL, "pcx_sim_sweep_generate_f64: null argument");
    if (const int rc = sweep_check(sweep, "pcx_sim_sweep_generate_f64", nullptr, nullptr, nullptr, nullptr)) return rc;
    if (const int rc = sim_check_timestep(timestep, "pcx_sim_sweep_generate_f64")) return rc;
    if (sweep->n_cells == 0) return PCX_OK;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    pcx_ctx::RaggedSlot* slot = nullptr;
    pcx::SweepTables tab;
    if (const int rc = sweep_tables_upload(ctx, sweep, &slot, &tab)) return rc;
    e = pcx::launch_sim_sweep_generate(tab, (uint32_t)timestep, *rounds, ctx->stream);
    if (e == hipSuccess) e = hipEventRecord(slot->kern_ev, ctx->stream);
    return e == hipSuccess ? PCX_OK : hip_fail(e, "k_sim_sweep_generate launch");
}

int pcx_sim_sweep_metrics_f64(pcx_ctx* ctx, const pcx_sim_sweep* sweep, const pcx_sim_rounds* rounds,
                              const double* old_rep, const double* smooth_rep, const double* outcomes_final,
                              double* metrics, double* summary) {
    if (!ctx || !sweep || !rounds) return fail(PCX_EINVAL, "pcx_sim_sweep_metrics_f64: null argument");
    if (const int rc = sweep_check(sweep, "pcx_sim_sweep_metrics_f64", nullptr, nullptr, nullptr, nullptr)) return rc;
    if (sweep->n_cells == 0) return PCX_OK;
    if (!old_rep || !smooth_rep || !outcomes_final || !metrics)
        return fail(PCX_EINVAL, "pcx_sim_sweep_metrics_f64: null argument");
    if (!rounds->scaled || !rounds->lo || !rounds->hi || !rounds->truth || !rounds->liar)
        return fail(PCX_EINVAL, "pcx_sim_sweep_metrics_f64: rounds needs scaled, lo, hi, truth and liar");
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    pcx_ctx::RaggedSlot* slot = nullptr;
    pcx::SweepTables tab;
    if (const int rc = sweep_tables_upload(ctx, sweep, &slot, &tab)) return rc;
    e = pcx::launch_sim_sweep_metrics(tab, sweep->scaled_tol, *rounds, old_rep, smooth_rep, outcomes_final, metrics,
                                      ctx->stream);
    if (e == hipSuccess && summary) e = pcx::launch_sim_sweep_summary(tab, metrics, summary, ctx->stream);
    if (e == hipSuccess) e = hipEventRecord(slot->kern_ev, ctx->stream);
    return e == hipSuccess ? PCX_OK : hip_fail(e, "k_sim_sweep_metrics / k_sim_sweep_summary launch");
}

// bytes of pair_base [C] behind a sweep's tables in a staging slot (a multiple of 8)
static size_t pair_base_bytes(const pcx_sim_sweep* s) { return ((size_t)s->n_cells * sizeof(int32_t) + 7) / 8 * 8; }

// the pair_base checks of pcx_sim_study_check, on a sweep that sweep_check has passed
static int study_check(const pcx_sim_sweep* s, const int32_t* pair_base, const char* who, int64_t* bad_cell) {
    if (bad_cell) *bad_cell = -1;
    for (int64_t c = 0; pair_base && c < s->n_cells; c++) {
        const int64_t base = pair_base[c];
        if (base == -1) continue;
        if (base < 0 || base >= s->n_cells)
            return sweep_fail(bad_cell, c, who,
                              "pair_base " + std::to_string(base) + " is outside [0, " + std::to_string(s->n_cells) +
                                  ") (-1 = no base)");
        if (base == c) return sweep_fail(bad_cell, c, who, "pair_base is the cell itself");
        if (s->cells[base].n_rounds != s->cells[c].n_rounds)
            return sweep_fail(bad_cell, c, who,
                              "has " + std::to_string(s->cells[c].n_rounds) + " rounds, its base cell " +
                                  std::to_string(base) + " has " + std::to_string(s->cells[base].n_rounds) +
                                  " (a pair is round b of both)");
    }
    return PCX_OK;
}

// a checked sweep's cells expanded into the ragged call's per-round shapes [B]; pof (or NULL): round b's cell
static void sweep_shapes(const pcx_sim_sweep* s, int32_t* nrep, int32_t* nev, int32_t* pof) {
    for (int64_t c = 0, b = 0; c < s->n_cells; c++)
        for (int64_t r = 0; r < s->cells[c].n_rounds; r++, b++) {
            nrep[b] = s->cells[c].n_reporters;
            nev[b] = s->cells[c].n_events;
            if (pof) pof[b] = (int32_t)c;
        }
}

// The loop of pcx_simulate_sweep_f64, pcx_simulate_study_f64 and pcx_simulate_study_params_f64
// (`who`).  study NULL: the sweep.  Otherwise every timestep's metrics launch is followed by the
// detail launch, and one statistics launch follows the last timestep.  cp: per-cell parameter sets
// [C] (NULL: the sweep's shared ones) -- the consensus launches are then those of
// pcx_consensus_ragged_params_f64, round b of cell c on set c.
// restarts > 0 (pcx_simulate_study_kmeans_f64): k-means passes; the call runs on parameter sets (the
// shared parameters as every cell's set where cp is NULL), every timestep's books of the k-means
// cells' rounds are drawn into the workspace behind the generator, and the consensus launches are
// those of pcx_consensus_ragged_kmeans_f64.
// tall (pcx_simulate_study_tall_f64, with a cell above 256 reporters): cells up to 1024 reporters; the
// call runs on parameter sets likewise, its consensus launches are those of
// pcx_consensus_ragged_tall_f64, and the generator runs its 1024-reporter instantiation.
static int sweep_run(pcx_ctx* ctx, const pcx_sim_sweep* sweep, pcx_sim_result* res, const int32_t* pair_base,
                     const pcx_sim_study_result* study, const char* who, const pcx_round_params* cp = nullptr,
                     int restarts = 0, bool tall = false) {
    const std::string name(who);
    int64_t tot[4], cnt[4], lds[4];
    const bool km = restarts > 0;
    if (const int rc = sweep_check(sweep, who, tot, cnt, lds, nullptr, cp, km, tall)) return rc;
    std::vector<pcx_round_params> own_cp;
    if ((km || tall) && !cp) {
        own_cp.assign((size_t)sweep->n_cells, shared_set(sweep));
        cp = own_cp.data();
    }
    if (km)
        if (const int rc = sim_books_check(tot[0], restarts, name)) return rc;
    if (study) {
        if (const int rc = study_check(sweep, pair_base, who, nullptr)) return rc;
        if (study->paired && !pair_base) return fail(PCX_EINVAL, name + ": paired needs pair_base");
    }
    const int64_t C = sweep->n_cells, B = tot[0], T = sweep->n_timesteps;
    if (C == 0) return PCX_OK;
    if (study && !study->stats) return fail(PCX_EINVAL, name + ": study->stats is NULL");
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    // the cells expanded into the wide ragged call's per-round shapes
    std::vector<int32_t> shape;
    try {
        shape.resize((size_t)B * (cp ? 3 : 2));
    } catch (const std::bad_alloc&) {
        return fail(PCX_ENOMEM, name + ": no host memory for the per-round shapes");
    }
    int32_t* nrep = shape.data();
    int32_t* nev = nrep + B;
    int32_t* pof = cp ? nev + B : nullptr;  // round b's parameter set: its cell
    sweep_shapes(sweep, nrep, nev, pof);
    // work buffers, pcx_simulate_f64's layout over the flat arrays
    const size_t bn = (size_t)tot[1], be = (size_t)tot[2], bne = (size_t)tot[3];
    // (a study keeps every timestep's metrics and detail for its statistics: in the workspace, behind
    // the sweep's doubles, where the caller gives no buffer)
    const bool all_metrics = study && !res->metrics;
    const size_t n_metrics = (size_t)(all_metrics ? T : 1) * B * PCX_SIM_NMETRICS;
    const size_t n_detail = study && !study->detail ? (size_t)T * B * PCX_SIM_NDETAIL : 0;
    // (k-means: the flat books of the k-means cells' rounds)
    int64_t n_books = 0;
    if (km)
        if (const int rc = kmeans_layout(B, nrep, nev, nullptr, restarts, cp, pof, nullptr, nullptr, nullptr, &n_books))
            return rc;
    SimFrame w;
    if (const int rc = w.carve(ctx, bne, be, bn, n_metrics, n_detail, (size_t)n_books)) return rc;
    double* const all_detail = !study ? nullptr : study->detail ? study->detail : w.detail;
    // every table of the call in one staging slot, uploaded once: the ragged call's descriptors (the
    // same every timestep: only the data pointers change), then the sweep's own
    RaggedPlan plan;
    const bool pairs = study && study->paired;
    const size_t off_ktab = sweep_table_bytes(sweep) + (pairs ? pair_base_bytes(sweep) : 0);  // inside `extra`
    const size_t extra = off_ktab + (km ? (size_t)B * sizeof(pcx::KmeansEntry) : 0);
    if (const int rc = cp ? plan_table(ctx, B, nrep, nev, C, cp, pof, false, extra, &plan)
                          : plan_shared(ctx, B, nrep, nev, sweep->algorithm, false, cnt, lds, false, extra, false, &plan))
        return rc;
    pcx_ctx::RaggedSlot* const slot = plan.slot;
    const size_t off_x = plan.off_x;
    const pcx::SweepTables tab = sweep_tables_fill(sweep, static_cast<char*>(slot->pin) + off_x,
                                                   static_cast<char*>(slot->dev) + off_x);
    const int32_t* dev_base = nullptr;  // pair_base rides behind the sweep's tables
    if (pairs) {
        const size_t at = off_x + sweep_table_bytes(sweep);
        std::memcpy(static_cast<char*>(slot->pin) + at, pair_base, (size_t)C * sizeof(int32_t));
        dev_base = reinterpret_cast<const int32_t*>(static_cast<char*>(slot->dev) + at);
    }
    const pcx::KmeansEntry* dev_ktab = nullptr;  // the per-round book table rides last
    if (km) {
        (void)kmeans_layout(B, nrep, nev, nullptr, restarts, cp, pof, nullptr,
                            reinterpret_cast<pcx::KmeansEntry*>(static_cast<char*>(slot->pin) + off_x + off_ktab), nullptr);
        dev_ktab = reinterpret_cast<const pcx::KmeansEntry*>(static_cast<char*>(slot->dev) + off_x + off_ktab);
    }
    e = ragged_slot_upload(ctx, *slot, plan.bytes);
    if (e != hipSuccess) return hip_fail(e, "sweep: table upload");
    const double* rep = sweep->reputation0;
    for (int64_t t = 0; t < T; t++) {  // launches only: no host wait in this loop
        pcx_sim_rounds r;
        pcx_batch_result o;
        w.at(t, t == T - 1, res, &r, &o);
        e = pcx::launch_sim_sweep_generate(tab, (uint32_t)t, r, ctx->stream, tall);
        if (e != hipSuccess) return hip_fail(e, "k_sim_sweep_generate launch");
        pcx_ragged in{};
        in.n_rounds = B;
        in.reports = r.reports;
        in.reputation = rep;
        in.scaled = r.scaled;
        in.lo = r.lo;
        in.hi = r.hi;
        in.catch_tolerance = sweep->catch_tolerance;
        in.alpha = sweep->alpha;
        in.algorithm = sweep->algorithm;
        in.max_components = sweep->max_components;
        in.variance_threshold = sweep->variance_threshold;
        in.hierarchy_threshold = sweep->hierarchy_threshold;
        in.cluster_threshold = sweep->cluster_threshold;
        pcx::BatchArgs a = shared_args(&in, &o);
        a.B = B;
        if (km && n_books > 0) {
            e = pcx::launch_sim_sweep_kmeans_books(tab, dev_ktab, restarts, (uint32_t)t, w.books, ctx->stream);
            if (e != hipSuccess) return hip_fail(e, "k_kmeans_books_sweep launch");
            a.kmeans_restarts = restarts;
            a.kmeans_init = w.books;
        }
        e = plan.launch(ctx, a, dev_ktab);  // (k-means: dev_ktab is set, and the clustering launches read it)
        if (e != hipSuccess) return hip_fail(e, "sweep: ragged wide launch");
        if (res->metrics || res->summary || study) {
            double* m = res->metrics   ? res->metrics + (size_t)t * B * PCX_SIM_NMETRICS
                        : all_metrics ? w.metrics + (size_t)t * B * PCX_SIM_NMETRICS
                                      : w.metrics;
            e = pcx::launch_sim_sweep_metrics(tab, sweep->scaled_tol, r, o.old_rep, o.smooth_rep, o.outcomes_final, m,
                                              ctx->stream);
            if (e == hipSuccess && res->summary)
                e = pcx::launch_sim_sweep_summary(tab, m, res->summary + (size_t)t * C * PCX_SIM_NMETRICS,
                                                  ctx->stream);
            if (e != hipSuccess) return hip_fail(e, "k_sim_sweep_metrics / k_sim_sweep_summary launch");
        }
        if (study) {
            e = pcx::launch_sim_study_detail(tab, 0, 0, sweep->scaled_tol, r, o.old_rep, o.smooth_rep, o.outcomes_final,
                                             all_detail + (size_t)t * B * PCX_SIM_NDETAIL, ctx->stream);
            if (e != hipSuccess) return hip_fail(e, "k_sim_study_detail launch");
        }
        rep = o.smooth_rep;  // the next timestep's reputation
    }
    if (study) {
        e = pcx::launch_sim_study_stats(tab, T, res->metrics ? res->metrics : w.metrics, all_detail, dev_base,
                                        study->stats, pairs ? study->paired : nullptr, ctx->stream);
        if (e != hipSuccess) return hip_fail(e, "k_sim_study_stats launch");
    }
    e = hipEventRecord(slot->kern_ev, ctx->stream);
    if (e != hipSuccess) return hip_fail(e, "sweep: hipEventRecord");
    if (res->reputation && bn) {
        e = hipMemcpyAsync(res->reputation, rep, bn * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream);
        if (e != hipSuccess) return hip_fail(e, (name + ": reputation copy").c_str());
    }
    return PCX_OK;
}

int pcx_simulate_sweep_f64(pcx_ctx* ctx, const pcx_sim_sweep* sweep, pcx_sim_result* res) {
    if (!ctx || !sweep || !res) return fail(PCX_EINVAL, "pcx_simulate_sweep_f64: null argument");
    return sweep_run(ctx, sweep, res, nullptr, nullptr, "pcx_simulate_sweep_f64");
}

// ---------------------------------------------------------------- simulator studies
int pcx_simulate_study_f64(pcx_ctx* ctx, const pcx_sim_sweep* sweep, const int32_t* pair_base, pcx_sim_result* res,
                           pcx_sim_study_result* study) {
    if (!ctx || !sweep || !res || !study) return fail(PCX_EINVAL, "pcx_simulate_study_f64: null argument");
    return sweep_run(ctx, sweep, res, pair_base, study, "pcx_simulate_study_f64");
}

int pcx_sim_study_params_check(const pcx_sim_sweep* sweep, const pcx_round_params* cell_params,
                               const int32_t* pair_base, int64_t* bad_cell) {
    if (!sweep) return fail(PCX_EINVAL, "pcx_sim_study_params_check: null argument");
    if (const int rc = sweep_check(sweep, "pcx_sim_study_params_check", nullptr, nullptr, nullptr, bad_cell, cell_params))
        return rc;
    return study_check(sweep, pair_base, "pcx_sim_study_params_check", bad_cell);
}

int pcx_simulate_study_params_f64(pcx_ctx* ctx, const pcx_sim_sweep* sweep, const pcx_round_params* cell_params,
                                  const int32_t* pair_base, pcx_sim_result* res, pcx_sim_study_result* study) {
    if (!ctx || !sweep || !res) return fail(PCX_EINVAL, "pcx_simulate_study_params_f64: null argument");
    if (!cell_params)  // the existing entries, the same bytes
        return study ? pcx_simulate_study_f64(ctx, sweep, pair_base, res, study) : pcx_simulate_sweep_f64(ctx, sweep, res);
    return sweep_run(ctx, sweep, res, study ? pair_base : nullptr, study, "pcx_simulate_study_params_f64", cell_params);
}

int pcx_sim_sweep_plan_tall(const pcx_sim_sweep* sweep, const pcx_round_params* cell_params, int64_t totals[4],
                            int64_t counts[4], int64_t lds_bytes[4], int64_t* bad_cell) {
    if (!sweep) return fail(PCX_EINVAL, "pcx_sim_sweep_plan_tall: null argument");
    return sweep_check(sweep, "pcx_sim_sweep_plan_tall", totals, counts, lds_bytes, bad_cell, cell_params, false, true);
}

int pcx_sim_study_tall_check(const pcx_sim_sweep* sweep, const pcx_round_params* cell_params,
                             const int32_t* pair_base, int64_t* bad_cell) {
    const char* who = "pcx_sim_study_tall_check";
    if (!sweep) return fail(PCX_EINVAL, std::string(who) + ": null argument");
    if (const int rc = sweep_check(sweep, who, nullptr, nullptr, nullptr, bad_cell, cell_params, false, true)) return rc;
    return study_check(sweep, pair_base, who, bad_cell);
}

int pcx_simulate_study_tall_f64(pcx_ctx* ctx, const pcx_sim_sweep* sweep, const pcx_round_params* cell_params,
                                const int32_t* pair_base, pcx_sim_result* res, pcx_sim_study_result* study) {
    const char* who = "pcx_simulate_study_tall_f64";
    if (!ctx || !sweep || !res) return fail(PCX_EINVAL, std::string(who) + ": null argument");
    bool any_tall = false;
    if (const int rc = sweep_check(sweep, who, nullptr, nullptr, nullptr, nullptr, cell_params, false, true, &any_tall))
        return rc;
    if (!any_tall)  // the existing entries, the same bytes
        return pcx_simulate_study_params_f64(ctx, sweep, cell_params, pair_base, res, study);
    return sweep_run(ctx, sweep, res, study ? pair_base : nullptr, study, who, cell_params, 0, true);
}

int pcx_sim_study_kmeans_check(const pcx_sim_sweep* sweep, const pcx_round_params* cell_params,
                               const int32_t* pair_base, int32_t restarts, int64_t* bad_cell) {
    const char* who = "pcx_sim_study_kmeans_check";
    if (!sweep) return fail(PCX_EINVAL, std::string(who) + ": null argument");
    if (bad_cell) *bad_cell = -1;
    if (restarts < 1) return fail(PCX_EINVAL, std::string(who) + ": k-means restarts must be >= 1");
    int64_t tot[4];
    if (const int rc = sweep_check(sweep, who, tot, nullptr, nullptr, bad_cell, cell_params, true)) return rc;
    if (const int rc = sim_books_check(tot[0], restarts, who)) return rc;
    return study_check(sweep, pair_base, who, bad_cell);
}

int pcx_simulate_study_kmeans_f64(pcx_ctx* ctx, const pcx_sim_sweep* sweep, const pcx_round_params* cell_params,
                                  const int32_t* pair_base, int32_t restarts, pcx_sim_result* res,
                                  pcx_sim_study_result* study) {
    if (!ctx || !sweep || !res) return fail(PCX_EINVAL, "pcx_simulate_study_kmeans_f64: null argument");
    if (restarts < 1) return fail(PCX_EINVAL, "pcx_simulate_study_kmeans_f64: k-means restarts must be >= 1");
    return sweep_run(ctx, sweep, res, study ? pair_base : nullptr, study, "pcx_simulate_study_kmeans_f64", cell_params,
                     restarts);
}

// the book table of a sweep whose every round is k-means under the rule (pcx_kmeans_plan's layout)
static int sweep_books_table(const pcx_sim_sweep* sweep, int restarts, const char* who, std::vector<char>* cells,
                             std::vector<pcx::KmeansEntry>* tab, int64_t* B) {
    int64_t tot[4];
    if (const int rc = sweep_check(sweep, who, tot, nullptr, nullptr, nullptr, nullptr, true)) return rc;
    if (const int rc = sim_books_check(tot[0], restarts, who)) return rc;
    *B = tot[0];
    cells->resize(sweep_table_bytes(sweep));
    sweep_tables_fill(sweep, cells->data(), cells->data());
    tab->resize((size_t)tot[0]);
    std::vector<int32_t> shape((size_t)tot[0] * 2);
    sweep_shapes(sweep, shape.data(), shape.data() + tot[0], nullptr);
    return kmeans_layout(tot[0], shape.data(), shape.data() + tot[0], nullptr, restarts, nullptr, nullptr, nullptr,
                         tab->data(), nullptr);
}

int pcx_sim_sweep_kmeans_books_host(const pcx_sim_sweep* sweep, int32_t restarts, int timestep, int32_t* books) {
    const char* who = "pcx_sim_sweep_kmeans_books_host";
    if (!sweep || !books) return fail(PCX_EINVAL, std::string(who) + ": null argument");
    if (const int rc = sim_check_timestep(timestep, who)) return rc;
    std::vector<char> cells;
    std::vector<pcx::KmeansEntry> tab;
    int64_t B = 0;
    if (const int rc = sweep_books_table(sweep, restarts, who, &cells, &tab, &B)) return rc;
    pcx::sim_sweep_kmeans_books_host(reinterpret_cast<const pcx::SweepCell*>(cells.data()), sweep->n_cells, tab.data(),
                                     restarts, (uint32_t)timestep, books);
    return PCX_OK;
}

int pcx_sim_sweep_kmeans_books_f64(pcx_ctx* ctx, const pcx_sim_sweep* sweep, int32_t restarts, int timestep,
                                   int32_t* books) {
    const char* who = "pcx_sim_sweep_kmeans_books_f64";
    if (!ctx || !sweep || !books) return fail(PCX_EINVAL, std::string(who) + ": null argument");
    if (const int rc = sim_check_timestep(timestep, who)) return rc;
    std::vector<char> cells;
    std::vector<pcx::KmeansEntry> tab;
    int64_t B = 0;
    if (const int rc = sweep_books_table(sweep, restarts, who, &cells, &tab, &B)) return rc;
    if (B == 0) return PCX_OK;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    // the sweep's tables and the book table through one staging slot
    const size_t tb = sweep_table_bytes(sweep), kb = (size_t)B * sizeof(pcx::KmeansEntry);
    pcx_ctx::RaggedSlot* slot = nullptr;
    if (const int rc = ragged_slot_take(ctx, tb + kb, &slot)) return rc;
    const pcx::SweepTables t = sweep_tables_fill(sweep, slot->pin, slot->dev);
    std::memcpy(static_cast<char*>(slot->pin) + tb, tab.data(), kb);
    e = ragged_slot_upload(ctx, *slot, tb + kb);
    if (e != hipSuccess) return hip_fail(e, "sweep: table upload");
    e = pcx::launch_sim_sweep_kmeans_books(t, reinterpret_cast<const pcx::KmeansEntry*>(static_cast<char*>(slot->dev) + tb),
                                           restarts, (uint32_t)timestep, books, ctx->stream);
    if (e == hipSuccess) e = hipEventRecord(slot->kern_ev, ctx->stream);
    return e == hipSuccess ? PCX_OK : hip_fail(e, "k_kmeans_books_sweep launch");
}

int pcx_sim_study_check(const pcx_sim_sweep* sweep, const int32_t* pair_base, int64_t* bad_cell) {
    if (!sweep) return fail(PCX_EINVAL, "pcx_sim_study_check: null argument");
    if (const int rc = sweep_check(sweep, "pcx_sim_study_check", nullptr, nullptr, nullptr, bad_cell)) return rc;
    return study_check(sweep, pair_base, "pcx_sim_study_check", bad_cell);
}

static bool detail_args(const pcx_sim_rounds* r, const double* old_rep, const double* smooth_rep,
                        const double* outcomes_final, const double* detail) {
    return r->scaled && r->lo && r->hi && r->truth && r->liar && old_rep && smooth_rep && outcomes_final && detail;
}

int pcx_sim_detail_host(const pcx_sim* sim, const pcx_sim_rounds* rounds, const double* old_rep,
                        const double* smooth_rep, const double* outcomes_final, double* detail) {
    if (!sim || !rounds) return fail(PCX_EINVAL, "pcx_sim_detail_host: null argument");
    if (const int rc = sim_check(sim, "pcx_sim_detail_host")) return rc;
    if (!detail_args(rounds, old_rep, smooth_rep, outcomes_final, detail))
        return fail(PCX_EINVAL, "pcx_sim_detail_host: null argument (rounds needs scaled, lo, hi, truth and liar)");
    pcx::sim_study_detail_host(nullptr, 0, sim->n_rounds, (int32_t)sim->n_reporters, (int32_t)sim->n_events,
                               sim->scaled_tol, *rounds, old_rep, smooth_rep, outcomes_final, detail);
    return PCX_OK;
}

int pcx_sim_detail_f64(pcx_ctx* ctx, const pcx_sim* sim, const pcx_sim_rounds* rounds, const double* old_rep,
                       const double* smooth_rep, const double* outcomes_final, double* detail) {
    if (!ctx || !sim || !rounds) return fail(PCX_EINVAL, "pcx_sim_detail_f64: null argument");
    if (const int rc = sim_check(sim, "pcx_sim_detail_f64")) return rc;
    if (!detail_args(rounds, old_rep, smooth_rep, outcomes_final, detail))
        return fail(PCX_EINVAL, "pcx_sim_detail_f64: null argument (rounds needs scaled, lo, hi, truth and liar)");
    if (sim->n_reporters > 0x7fffffff || sim->n_events > 0x7fffffff)
        return fail(PCX_EINVAL, "pcx_sim_detail_f64: n_reporters and n_events must be below 2^31");
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    pcx::SweepTables tab{nullptr, nullptr, 0, sim->n_rounds};
    e = pcx::launch_sim_study_detail(tab, (int32_t)sim->n_reporters, (int32_t)sim->n_events, sim->scaled_tol, *rounds,
                                     old_rep, smooth_rep, outcomes_final, detail, ctx->stream);
    return e == hipSuccess ? PCX_OK : hip_fail(e, "k_sim_study_detail launch");
}

int pcx_sim_sweep_detail_host(const pcx_sim_sweep* sweep, const pcx_sim_rounds* rounds, const double* old_rep,
                              const double* smooth_rep, const double* outcomes_final, double* detail) {
    if (!sweep || !rounds) return fail(PCX_EINVAL, "pcx_sim_sweep_detail_host: null argument");
    if (const int rc = sweep_check(sweep, "pcx_sim_sweep_detail_host", nullptr, nullptr, nullptr, nullptr)) return rc;
    if (sweep->n_cells == 0) return PCX_OK;
    if (!detail_args(rounds, old_rep, smooth_rep, outcomes_final, detail))
        return fail(PCX_EINVAL, "pcx_sim_sweep_detail_host: null argument (rounds needs scaled, lo, hi, truth and liar)");
    std::vector<char> tab(sweep_table_bytes(sweep));
    const pcx::SweepTables t = sweep_tables_fill(sweep, tab.data(), tab.data());
    pcx::sim_study_detail_host(t.cells, t.C, t.B, 0, 0, sweep->scaled_tol, *rounds, old_rep, smooth_rep, outcomes_final,
                               detail);
    return PCX_OK;
}

int pcx_sim_sweep_detail_f64(pcx_ctx* ctx, const pcx_sim_sweep* sweep, const pcx_sim_rounds* rounds,
                             const double* old_rep, const double* smooth_rep, const double* outcomes_final,
                             double* detail) {
    if (!ctx || !sweep || !rounds) return fail(PCX_EINVAL, "pcx_sim_sweep_detail_f64: null argument");
    if (const int rc = sweep_check(sweep, "pcx_sim_sweep_detail_f64", nullptr, nullptr, nullptr, nullptr)) return rc;
    if (sweep->n_cells == 0) return PCX_OK;
    if (!detail_args(rounds, old_rep, smooth_rep, outcomes_final, detail))
        return fail(PCX_EINVAL, "pcx_sim_sweep_detail_f64: null argument (rounds needs scaled, lo, hi, truth and liar)");
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    pcx_ctx::RaggedSlot* slot = nullptr;
    pcx::SweepTables tab;
    if (const int rc = sweep_tables_upload(ctx, sweep, &slot, &tab)) return rc;
    e = pcx::launch_sim_study_detail(tab, 0, 0, sweep->scaled_tol, *rounds, old_rep, smooth_rep, outcomes_final, detail,
                                     ctx->stream);
    if (e == hipSuccess) e = hipEventRecord(slot->kern_ev, ctx->stream);
    return e == hipSuccess ? PCX_OK : hip_fail(e, "k_sim_study_detail launch");
}

// what the two statistics entries check alike
static int stats_check(const pcx_sim_sweep* sweep, const double* metrics, const double* detail,
                       const int32_t* pair_base, const double* stats, const double* paired, const char* who) {
    if (const int rc = sweep_check(sweep, who, nullptr, nullptr, nullptr, nullptr)) return rc;
    if (const int rc = study_check(sweep, pair_base, who, nullptr)) return rc;
    if (paired && !pair_base) return fail(PCX_EINVAL, std::string(who) + ": paired needs pair_base");
    if (sweep->n_cells > 0 && (!metrics || !detail || !stats)) return fail(PCX_EINVAL, std::string(who) + ": null argument");
    return PCX_OK;
}

int pcx_sim_sweep_stats_host(const pcx_sim_sweep* sweep, const double* metrics, const double* detail,
                             const int32_t* pair_base, double* stats, double* paired) {
    if (!sweep) return fail(PCX_EINVAL, "pcx_sim_sweep_stats_host: null argument");
    if (const int rc = stats_check(sweep, metrics, detail, pair_base, stats, paired, "pcx_sim_sweep_stats_host"))
        return rc;
    if (sweep->n_cells == 0) return PCX_OK;
    std::vector<char> tab(sweep_table_bytes(sweep));
    const pcx::SweepTables t = sweep_tables_fill(sweep, tab.data(), tab.data());
    pcx::sim_study_stats_host(t.cells, t.C, t.B, sweep->n_timesteps, metrics, detail, pair_base, stats, paired);
    return PCX_OK;
}

int pcx_sim_sweep_stats_f64(pcx_ctx* ctx, const pcx_sim_sweep* sweep, const double* metrics, const double* detail,
                            const int32_t* pair_base, double* stats, double* paired) {
    if (!ctx || !sweep) return fail(PCX_EINVAL, "pcx_sim_sweep_stats_f64: null argument");
    if (const int rc = stats_check(sweep, metrics, detail, pair_base, stats, paired, "pcx_sim_sweep_stats_f64"))
        return rc;
    if (sweep->n_cells == 0) return PCX_OK;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    // the sweep's tables and, behind them, pair_base in one staging slot
    const size_t bytes = sweep_table_bytes(sweep), all = bytes + (paired ? pair_base_bytes(sweep) : 0);
    pcx_ctx::RaggedSlot* slot = nullptr;
    if (const int rc = ragged_slot_take(ctx, all, &slot)) return rc;
    const pcx::SweepTables tab = sweep_tables_fill(sweep, slot->pin, slot->dev);
    const int32_t* dev_base = nullptr;
    if (paired) {
        std::memcpy(static_cast<char*>(slot->pin) + bytes, pair_base, (size_t)sweep->n_cells * sizeof(int32_t));
        dev_base = reinterpret_cast<const int32_t*>(static_cast<char*>(slot->dev) + bytes);
    }
    e = ragged_slot_upload(ctx, *slot, all);
    if (e != hipSuccess) return hip_fail(e, "study: table upload");
    e = pcx::launch_sim_study_stats(tab, sweep->n_timesteps, metrics, detail, dev_base, stats, paired, ctx->stream);
    if (e == hipSuccess) e = hipEventRecord(slot->kern_ev, ctx->stream);
    return e == hipSuccess ? PCX_OK : hip_fail(e, "k_sim_study_stats launch");
}


}  // extern "C"
