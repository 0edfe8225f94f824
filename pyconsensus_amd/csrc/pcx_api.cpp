// pcx_api.cpp -- the extern "C" boundary of libpcx (declared in include/pcx.h).
// Host-side validation, context/stream management and kernel launches; no
// compute happens here.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>
#include <cstdlib>
#include <atomic>
#include <thread>
#include <algorithm>

#include "../../include/pcx.h"
#include "pcx_internal.h"
#include "pcx_sim_study.h"
#include "pcx_sim_sweep.h"
#include "pcx_sync.h"
#include "pcx_seqsum.h"

namespace {
thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

int hip_fail(hipError_t e, const char* what) {
    return fail(PCX_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}

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
void stamps_begin(pcx::BatchArgs& a, hipStream_t stream) {
    const char* env = getenv("PCX_STAMPS");
    if (!env || env[0] != '1' || a.B <= 0) return;
    const size_t bytes = (size_t)a.B * 32 * sizeof(long long);
    long long* d = nullptr;
    if (hipMalloc(&d, bytes) != hipSuccess) return;
    (void)hipMemsetAsync(d, 0, bytes, stream);
    a.stamps = d;
}

std::vector<long long> stamps_end(pcx::BatchArgs& a, hipStream_t stream) {
    std::vector<long long> h(a.stamps ? a.B * 32 : 0);
    if (!a.stamps) return h;
    (void)hipMemcpyAsync(h.data(), a.stamps, h.size() * sizeof(long long), hipMemcpyDeviceToHost, stream);
    (void)hipStreamSynchronize(stream);
    (void)hipFree(a.stamps);
    a.stamps = nullptr;
    return h;
}
}  // namespace

extern "C" {

int pcx_abi_version(void) { return PCX_ABI_VERSION; }

const char* pcx_last_error(void) { return g_err.c_str(); }

namespace {
pcx_ctx* new_ctx(int device_id, const char* who) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || device_id < 0 || device_id >= n) {
        g_err = std::string(who) + ": no HIP device " + std::to_string(device_id);
        return nullptr;
    }
    pcx_ctx* c = new (std::nothrow) pcx_ctx;
    if (!c) {
        g_err = std::string(who) + ": out of host memory";
        return nullptr;
    }
    c->device = device_id;
    return c;
}

pcx_ctx* with_comm(pcx_ctx* c, pcx::Comm* comm, const std::string& err) {
    if (!c) return nullptr;
    if (!comm) {
        g_err = err.empty() ? "communicator setup failed" : err;
        delete c;
        return nullptr;
    }
    c->comm = comm;
    return c;
}
}  // namespace

pcx_ctx* pcx_create(int device_id) { return new_ctx(device_id, "pcx_create"); }

int pcx_comm_unique_id(pcx_comm_id* out) {
    if (!out) return fail(PCX_EINVAL, "pcx_comm_unique_id: null argument");
    std::string err;
    const int rc = pcx::comm_rccl_unique_id(out, err);
    return rc ? fail(rc, err) : PCX_OK;
}

pcx_ctx* pcx_create_rank(int device_id, int world, int rank, const pcx_comm_id* id) {
    if (!id || world < 1 || rank < 0 || rank >= world) {
        g_err = "pcx_create_rank: bad id / world / rank";
        return nullptr;
    }
    pcx_ctx* c = new_ctx(device_id, "pcx_create_rank");
    if (!c) return nullptr;
    std::string err;  // world == 1 too: a one-rank RCCL communicator (every exchange still runs)
    return with_comm(c, pcx::comm_rccl(device_id, world, rank, id, err), err);
}

pcx_group* pcx_group_create(int world) {
    pcx_group* g = pcx::group_create(world);
    if (!g) g_err = "pcx_group_create: world must be >= 1";
    return g;
}

void pcx_group_destroy(pcx_group* g) { pcx::group_destroy(g); }

pcx_ctx* pcx_create_grouped(int device_id, pcx_group* g, int rank) {
    pcx_ctx* c = new_ctx(device_id, "pcx_create_grouped");
    if (!c) return nullptr;
    std::string err;
    return with_comm(c, pcx::comm_group(g, rank, err), err);
}

pcx_ctx* pcx_create_custom(int device_id, int world, int rank, const pcx_comm_ops* ops) {
    pcx_ctx* c = new_ctx(device_id, "pcx_create_custom");
    if (!c) return nullptr;
    std::string err;
    return with_comm(c, pcx::comm_custom(world, rank, ops, err), err);
}

pcx_ctx* pcx_create_devices(int n_devices, const int* device_ids) {
    if (n_devices < 1 || !device_ids) {
        g_err = "pcx_create_devices: need n_devices >= 1 and device_ids";
        return nullptr;
    }
    pcx_ctx* c = new_ctx(device_ids[0], "pcx_create_devices");
    if (!c) return nullptr;
    for (int k = 1; k < n_devices; k++) {
        pcx_ctx* probe = new_ctx(device_ids[k], "pcx_create_devices");
        if (!probe) {
            delete c;
            return nullptr;
        }
        delete probe;
    }
    bool distinct = true;
    for (int a = 0; a < n_devices; a++)
        for (int b = a + 1; b < n_devices; b++) distinct = distinct && device_ids[a] != device_ids[b];
    std::string err;
    std::vector<pcx::Comm*> comms;
    if (distinct) {
        const int rc = pcx::comm_rccl_all(n_devices, device_ids, comms, err);
        if (rc) {
            g_err = "pcx_create_devices: " + err;
            delete c;
            return nullptr;
        }
    } else {
        c->group = pcx::group_create(n_devices);
        for (int k = 0; k < n_devices && c->group; k++) comms.push_back(pcx::comm_group(c->group, k, err));
    }
    for (int k = 0; k < n_devices; k++) {
        pcx_ctx* s = (k < (int)comms.size() && comms[k]) ? new (std::nothrow) pcx_ctx : nullptr;
        if (s) {
            s->device = device_ids[k];
            s->comm = comms[k];
        } else if (k < (int)comms.size()) {
            delete comms[k];
        }
        c->sub.push_back(s);
    }
    for (pcx_ctx* s : c->sub)
        if (!s) {
            g_err = "pcx_create_devices: communicator setup failed" + (err.empty() ? std::string() : ": " + err);
            pcx_destroy(c);
            return nullptr;
        }
    return c;
}

int pcx_ctx_world(const pcx_ctx* ctx) {
    if (ctx && !ctx->sub.empty()) return (int)ctx->sub.size();
    return ctx && ctx->comm ? ctx->comm->world : 1;
}
int pcx_ctx_rank(const pcx_ctx* ctx) { return ctx && ctx->comm ? ctx->comm->rank : 0; }

int pcx_ctx_usable(const pcx_ctx* ctx) {
    if (!ctx) return 0;
    if (ctx->comm && ctx->comm->aborted) return 0;
    for (const pcx_ctx* s : ctx->sub)
        if (s->comm && s->comm->aborted) return 0;
    return 1;
}

int pcx_release_workspace(pcx_ctx* ctx) {
    if (!ctx) return fail(PCX_EINVAL, "pcx_release_workspace: null context");
    for (pcx_ctx* s : ctx->sub) pcx_release_workspace(s);
    pcx::rounds_free(ctx);
    (void)hipSetDevice(ctx->device);
    pcx::workspace_free(ctx);
    pcx::io_bufs_free(ctx);
    pcx::sim_free(ctx);
    pcx::ragged_free(ctx);
    return PCX_OK;
}

}  // extern "C"
namespace pcx {
void ctx_host_free(pcx_ctx* c) {
    if (c->mscr) (void)hipFree(c->mscr);
    c->mscr = nullptr;
    c->mscr_bytes = 0;
    if (c->pinned) (void)hipHostFree(c->pinned);
    c->pinned = nullptr;
    c->pinned_bytes = 0;
    if (c->sel_pin) (void)hipHostFree(c->sel_pin);
    c->sel_pin = nullptr;
    if (c->pin_small) (void)hipHostFree(c->pin_small);
    c->pin_small = nullptr;
    c->pin_small_bytes = 0;
    for (hipEvent_t& ev : c->sel_ev) {
        if (ev) (void)hipEventDestroy(ev);
        ev = nullptr;
    }
    if (c->side_stream) (void)hipStreamDestroy(c->side_stream);
    c->side_stream = nullptr;
    io_bufs_free(c);
}
void sim_free(pcx_ctx* c) {
    if (c->sim_buf) (void)hipFree(c->sim_buf);
    c->sim_buf = nullptr;
    c->sim_bytes = 0;
}
void ragged_free(pcx_ctx* c) {
    for (auto& s : c->rag) {
        if (s.copy_ev) (void)hipEventSynchronize(s.copy_ev);  // the upload may still read the staging
        if (s.kern_ev) (void)hipEventSynchronize(s.kern_ev);  // the launch may still read the table
        if (s.pin) (void)hipHostFree(s.pin);
        if (s.dev) (void)hipFree(s.dev);
        if (s.copy_ev) (void)hipEventDestroy(s.copy_ev);
        if (s.kern_ev) (void)hipEventDestroy(s.kern_ev);
        s = pcx_ctx::RaggedSlot();
    }
}
void io_bufs_free(pcx_ctx* c) {
    for (auto& b : c->io_bufs)
        if (b.first) (void)hipFree(b.first);
    c->io_bufs.clear();
}
}  // namespace pcx
extern "C" {

void pcx_destroy(pcx_ctx* ctx) {
    if (!ctx) return;
    for (pcx_ctx* s : ctx->sub) pcx_destroy(s);
    if (ctx->group) pcx::group_destroy(ctx->group);
    pcx::rounds_free(ctx);
    (void)hipSetDevice(ctx->device);
    pcx::ctx_host_free(ctx);
    pcx::workspace_free(ctx);
    pcx::sim_free(ctx);
    pcx::ragged_free(ctx);
    delete ctx->comm;
    delete ctx;
}

int pcx_set_stream(pcx_ctx* ctx, void* s) {
    if (!ctx) return fail(PCX_EINVAL, "pcx_set_stream: null context");
    ctx->stream = reinterpret_cast<hipStream_t>(s);
    return PCX_OK;
}

int pcx_synchronize(pcx_ctx* ctx) {
    if (!ctx) return fail(PCX_EINVAL, "pcx_synchronize: null context");
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    return e == hipSuccess ? PCX_OK : hip_fail(e, "pcx_synchronize");
}

// where a batch of n_reporters x n_events rounds runs (pcx_batched_route and the call itself)
static int batched_route(int64_t N, int64_t E, int alg, int k) {
    if (N < 1 || N > 0x7fffffff || E < 1 || E > 65536 || alg < PCX_ALG_PCA || alg > PCX_ALG_CLUSTERFECK) return -1;
    const bool large = N > 64 || E > 32;  // beyond one wavefront per round
    if (alg == PCX_ALG_KMEANS && (k < 1 || k > (large ? 1024 : 8) || k > N)) return -1;
    if (!large) return PCX_ROUTE_WAVE;
    return pcx::medium_fits((int)N, (int)E, alg, k) ? PCX_ROUTE_WORKGROUP : PCX_ROUTE_SCHEDULER;
}

int pcx_batched_route(int n_reporters, int n_events, int algorithm, int kmeans_k) {
    return batched_route(n_reporters, n_events, algorithm, kmeans_k);
}

// PCX_STAMPS, one-wave kernel: h = the stamps read back, [B][32]
static void print_wave_stamps(const std::vector<long long>& h, int64_t B) {
    // stamp ids in program order (pcx_batched.hip STAMP(k)); a phase is named by its closing stamp
    static const int order[] = {0, 1, 2, 13, 14, 3, 4, 5, 6, 7, 8, 15, 16, 9, 10, 11, 12};
    const int no = (int)(sizeof(order) / sizeof(order[0]));
    double acc[32] = {0};
    for (int64_t b = 0; b < B; b++)
        for (int k = 1; k < no; k++) {
            const long long t1 = h[b * 32 + order[k]], t0 = h[b * 32 + order[k - 1]];
            if (t1 && t0) acc[order[k]] += (double)(t1 - t0);
        }
    fprintf(stderr, "PCX_STAMPS mean cycles per phase:");
    for (int k = 1; k < no; k++) fprintf(stderr, " %d:%.0f", order[k], acc[order[k]] / (double)B);
    double sort = 0, walk = 0, fast = 0, slow = 0;  // 22, 23: outcome medians by the fill-group test / sorted
    for (int64_t b = 0; b < B; b++) {
        sort += (double)h[b * 32 + 20];
        walk += (double)h[b * 32 + 21];
        fast += (double)h[b * 32 + 22];
        slow += (double)h[b * 32 + 23];
    }
    double iscr = 0, isort = 0;  // 24, 25: interpolation medians decided by the prescreen / sorted
    for (int64_t b = 0; b < B; b++) {
        iscr += (double)h[b * 32 + 24];
        isort += (double)h[b * 32 + 25];
    }
    fprintf(stderr, " median_sort:%.0f median_walk:%.0f outcome_shortcut:%.4f outcome_sorted:%.4f", sort / (double)B,
            walk / (double)B, fast / (double)B, slow / (double)B);
    fprintf(stderr, " interp_screened:%.4f interp_sorted:%.4f\n", iscr / (double)B, isort / (double)B);
}

// PCX_STAMPS, workgroup kernel: stamps 0..15 in program order (pcx_medium.hip MSTAMP(k))
static void print_medium_stamps(const std::vector<long long>& h, int64_t B) {
    double acc[16] = {0};
    for (int64_t b = 0; b < B; b++)
        for (int k = 1, prev = 0; k < 16; k++) {
            const long long t1 = h[b * 32 + k], t0 = h[b * 32 + prev];
            if (t1 && t0) {
                acc[k] += (double)(t1 - t0);
                prev = k;
            }
        }
    fprintf(stderr, "PCX_STAMPS medium mean cycles per phase:");
    for (int k = 1; k < 16; k++) fprintf(stderr, " %d:%.0f", k, acc[k] / (double)B);
    double mp[3] = {0, 0, 0};  // wave 0's outcome medians: total+dom, rank, walk
    for (int64_t b = 0; b < B; b++)
        for (int k = 0; k < 3; k++) mp[k] += (double)h[b * 32 + 20 + k];
    fprintf(stderr, " wave0 medians total:%.0f rank:%.0f walk:%.0f", mp[0] / (double)B, mp[1] / (double)B,
            mp[2] / (double)B);
    double sub[4] = {0, 0, 0, 0};  // the nonconformity phase's steps (stamps 24-27 after 8)
    for (int64_t b = 0; b < B; b++)
        for (int k = 0; k < 4; k++) {
            const long long t1 = h[b * 32 + 24 + k], t0 = h[b * 32 + (k ? 23 + k : 8)];
            if (t1 && t0) sub[k] += (double)(t1 - t0);
        }
    fprintf(stderr, " nc: minmax+norm:%.0f n12:%.0f dots:%.0f ranks:%.0f", sub[0] / (double)B, sub[1] / (double)B,
            sub[2] / (double)B, sub[3] / (double)B);
    double pw[2] = {0, 0};  // power iteration: presquares (6 -> 28), steps (28 -> 29)
    for (int64_t b = 0; b < B; b++) {
        const long long* hb = &h[b * 32];
        if (hb[28] && hb[6]) pw[0] += (double)(hb[28] - hb[6]);
        if (hb[29] && hb[28]) pw[1] += (double)(hb[29] - hb[28]);
    }
    fprintf(stderr, " pi: presq:%.0f steps:%.0f\n", pw[0] / (double)B, pw[1] / (double)B);
}

// one workgroup per round (pcx_medium.hip), in chunks of bounded scratch
constexpr size_t MEDIUM_SCRATCH_CAP = (size_t)2 << 30;

// the context's workgroup scratch (pcx_ctx.mscr) grown to `need` bytes; 0 = ok
static int medium_scratch_reserve(pcx_ctx* ctx, size_t need) {
    if (ctx->mscr_bytes >= need) return PCX_OK;
    if (ctx->mscr) (void)hipFree(ctx->mscr);
    ctx->mscr = nullptr;
    ctx->mscr_bytes = 0;
    const hipError_t e = hipMalloc(&ctx->mscr, need);
    if (e != hipSuccess) return hip_fail(e, "hipMalloc(medium scratch)");
    ctx->mscr_bytes = need;
    return PCX_OK;
}

static int run_workgroup_route(pcx_ctx* ctx, pcx::BatchArgs& a) {
    const int64_t chunk = pcx::medium_chunk(a, MEDIUM_SCRATCH_CAP);
    if (const int rc = medium_scratch_reserve(ctx, pcx::medium_scratch_per_round(a) * (size_t)chunk)) return rc;
    hipError_t e = hipSuccess;
    double* Fscr = (double*)ctx->mscr;
    double* Cscr = Fscr + (a.filled ? 0 : (size_t)chunk * a.N * a.E);
    double* Xscr = Cscr + (size_t)chunk * a.E * a.E;  // the clusterings' cluster sums / observations
    stamps_begin(a, ctx->stream);
    for (int64_t b0 = 0; b0 < a.B && e == hipSuccess; b0 += chunk)
        e = pcx::launch_medium(a, b0, std::min<int64_t>(chunk, a.B - b0), Fscr, Cscr, Xscr, ctx->stream);
    if (a.stamps) print_medium_stamps(stamps_end(a, ctx->stream), a.B);
    return e == hipSuccess ? PCX_OK : hip_fail(e, "medium_round_kernel launch");
}

int pcx_consensus_batched_f64(pcx_ctx* ctx, const pcx_batch* in, pcx_batch_result* out) {
    if (!ctx || !in || !out) return fail(PCX_EINVAL, "pcx_consensus_batched_f64: null argument");
    if (in->n_rounds < 0 || in->n_rounds > 0x7fffffff)
        return fail(PCX_EINVAL, "batched: n_rounds must be in [0, 2^31)");
    if (in->n_reporters < 1 || in->n_reporters > 0x7fffffff)
        return fail(PCX_EINVAL, "batched: n_reporters must be in [1, 2^31)");
    if (in->n_events < 1 || in->n_events > 65536) return fail(PCX_EINVAL, "batched: n_events must be in [1, 65536]");
    const bool large = in->n_reporters > 64 || in->n_events > 32;  // beyond one wavefront per round
    const char* own = nullptr;  // this entry's own option checks (check_options reports them in their place)
    if (in->algorithm < PCX_ALG_PCA || in->algorithm > PCX_ALG_CLUSTERFECK)
        own = "algorithm must be an enum pcx_algorithm value (0..7)";
    else if (in->algorithm == PCX_ALG_KMEANS &&
             (!in->kmeans_init || in->kmeans_k < 1 || in->kmeans_k > (large ? 1024 : 8) ||
              in->kmeans_k > in->n_reporters || in->kmeans_restarts < 1))
        own = "k-means needs kmeans_init and 1 <= kmeans_k <= min(N, 8; 1024 above 64 x 32), restarts >= 1";
    else if (in->algorithm == PCX_ALG_BIG_FIVE && (in->max_components < 1 || in->max_components > in->n_events))
        own = "big-five needs 1 <= max_components <= n_events";
    if (const int rc = check_options("batched", in, own)) return rc;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    pcx::BatchArgs a = shared_args(in, out);
    a.B = in->n_rounds;
    a.N = (int)in->n_reporters;
    a.E = (int)in->n_events;
    a.ES = a.E | 1;
    a.bounds_shared = in->bounds_shared;
    a.kmeans_k = in->kmeans_k;
    a.kmeans_restarts = in->kmeans_restarts;
    a.kmeans_init = in->kmeans_init;
    const int route = batched_route(in->n_reporters, in->n_events, in->algorithm, in->kmeans_k);
    if (route < 0) return fail(PCX_EINVAL, "batched: invalid shape or algorithm");  // (refused above)
    if (route == PCX_ROUTE_WORKGROUP && !getenv("PCX_NO_MEDIUM")) return run_workgroup_route(ctx, a);
    if (route != PCX_ROUTE_WAVE) {
        // one single-matrix consensus per round, many rounds in flight (pcx_rounds.cpp)
        std::string err;
        const int rc = pcx::run_rounds(ctx, in, out, err);
        return rc ? fail(rc, "pcx_consensus_batched_f64: " + err) : PCX_OK;
    }
    stamps_begin(a, ctx->stream);
    e = pcx::launch_batched(a, ctx->stream);
    if (a.stamps) print_wave_stamps(stamps_end(a, ctx->stream), a.B);
    return e == hipSuccess ? PCX_OK : hip_fail(e, "batched_round_kernel launch");
}

// ---------------------------------------------------------------- ragged batches
// what pcx_ragged_plan and pcx_ragged_plan_wide refuse alike, before they look at a round
static int ragged_plan_checks(int64_t n_rounds, const int32_t* n_reporters, const int32_t* n_events, int algorithm,
                              int64_t* bad_round) {
    if (bad_round) *bad_round = -1;
    if (n_rounds < 0 || n_rounds > 0x7fffffff) return fail(PCX_EINVAL, "ragged: n_rounds must be in [0, 2^31)");
    if (algorithm < PCX_ALG_PCA || algorithm > PCX_ALG_CLUSTERFECK)
        return fail(PCX_EINVAL, "ragged: algorithm must be an enum pcx_algorithm value (0..7)");
    if (algorithm == PCX_ALG_KMEANS)
        return fail(PCX_EINVAL, "ragged: k-means is not supported (its code-book size depends on each round's N)");
    if (n_rounds > 0 && (!n_reporters || !n_events)) return fail(PCX_EINVAL, "ragged: n_reporters / n_events is NULL");
    return PCX_OK;
}

static int ragged_bad_round(int64_t b, int N, int E, int max_n, int max_e, int64_t* bad_round) {
    if (bad_round) *bad_round = b;
    return fail(PCX_EINVAL, "ragged: round " + std::to_string(b) + " is " + std::to_string(N) + " x " +
                                std::to_string(E) + "; a round must be within [1, " + std::to_string(max_n) +
                                "] x [1, " + std::to_string(max_e) + "]");
}

int pcx_ragged_plan(int64_t n_rounds, const int32_t* n_reporters, const int32_t* n_events, int algorithm,
                    int64_t totals[3], int64_t* lds_bytes, int64_t* bad_round) {
    if (const int rc = ragged_plan_checks(n_rounds, n_reporters, n_events, algorithm, bad_round)) return rc;
    int64_t tn = 0, te = 0, tc = 0;
    size_t lds = 0;
    for (int64_t b = 0; b < n_rounds; b++) {
        const int32_t N = n_reporters[b], E = n_events[b];
        if (N < 1 || N > 64 || E < 1 || E > 32) return ragged_bad_round(b, N, E, 64, 32, bad_round);
        tn += N;
        te += E;
        tc += (int64_t)N * E;
        lds = std::max(lds, pcx::ragged_lds_bytes(N, E, algorithm));
    }
    if (totals) {
        totals[0] = tn;
        totals[1] = te;
        totals[2] = tc;
    }
    if (lds_bytes) *lds_bytes = (int64_t)lds;
    return PCX_OK;
}

// This call's staging slot (the two are taken in turn), with room for `bytes` on both sides and the
// host side free to be rewritten: the slot's last upload has read it.  0 = ok.
static int ragged_slot_take(pcx_ctx* ctx, size_t bytes, pcx_ctx::RaggedSlot** slot) {
    hipError_t e = hipSuccess;
    pcx_ctx::RaggedSlot& s = ctx->rag[ctx->rag_next];
    ctx->rag_next ^= 1;
    *slot = &s;
    if (s.used) {  // the slot's last upload has read the staging
        e = hipEventSynchronize(s.copy_ev);
        if (e != hipSuccess) return hip_fail(e, "ragged: hipEventSynchronize");
    }
    if (!s.copy_ev) {
        e = hipEventCreateWithFlags(&s.copy_ev, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s.kern_ev, hipEventDisableTiming);
        if (e != hipSuccess) return hip_fail(e, "ragged: hipEventCreate");
    }
    if (s.bytes < bytes) {
        if (s.used) {  // the slot's last launch has read the table
            e = hipEventSynchronize(s.kern_ev);
            if (e != hipSuccess) return hip_fail(e, "ragged: hipEventSynchronize");
        }
        if (s.pin) (void)hipHostFree(s.pin);
        if (s.dev) (void)hipFree(s.dev);
        s.pin = s.dev = nullptr;
        s.bytes = 0;
        s.used = false;
        const size_t cap = std::max(bytes + bytes / 2, (size_t)4096);
        e = hipHostMalloc(&s.pin, cap, hipHostMallocDefault);
        if (e == hipSuccess) e = hipMalloc(&s.dev, cap);
        if (e != hipSuccess) {
            if (s.pin) (void)hipHostFree(s.pin);
            s.pin = nullptr;
            return fail(e == hipErrorOutOfMemory ? PCX_ENOMEM : PCX_EHIP,
                        std::string("ragged: descriptor table: ") + hipGetErrorString(e));
        }
        s.bytes = cap;
    }
    return PCX_OK;
}

// The slot's first `bytes` from the staging to the device table on the stream, after any launch
// that still reads the table (another stream's, maybe); copy_ev marks the staging read.
static hipError_t ragged_slot_upload(pcx_ctx* ctx, pcx_ctx::RaggedSlot& s, size_t bytes) {
    hipError_t e = hipSuccess;
    if (s.used) e = hipStreamWaitEvent(ctx->stream, s.kern_ev, 0);
    if (e == hipSuccess) e = hipMemcpyAsync(s.dev, s.pin, bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipEventRecord(s.copy_ev, ctx->stream);
    if (e == hipSuccess) s.used = true;
    return e;
}

int pcx_consensus_ragged_f64(pcx_ctx* ctx, const pcx_ragged* in, pcx_batch_result* out) {
    if (!ctx || !in || !out) return fail(PCX_EINVAL, "pcx_consensus_ragged_f64: null argument");
    int64_t lds = 0;
    if (const int rc = pcx_ragged_plan(in->n_rounds, in->n_reporters, in->n_events, in->algorithm, nullptr, &lds,
                                       nullptr))
        return rc;
    if (in->n_rounds == 0) return PCX_OK;
    // (max_components is capped at E_b per round on the device)
    const bool bad_five = in->algorithm == PCX_ALG_BIG_FIVE && in->max_components < 1;
    if (const int rc = check_options("ragged", in, bad_five ? "big-five needs max_components >= 1" : nullptr))
        return rc;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    // the descriptor table: built in this call's staging slot, uploaded on the stream
    const int64_t B = in->n_rounds;
    const size_t bytes = (size_t)B * sizeof(pcx::RaggedDesc);
    pcx_ctx::RaggedSlot* sp = nullptr;
    if (const int rc = ragged_slot_take(ctx, bytes, &sp)) return rc;
    pcx_ctx::RaggedSlot& s = *sp;
    pcx::RaggedDesc* d = static_cast<pcx::RaggedDesc*>(s.pin);
    int64_t cell = 0, row = 0, ev = 0;
    for (int64_t b = 0; b < B; b++) {
        const int32_t N = in->n_reporters[b], E = in->n_events[b];
        d[b] = pcx::RaggedDesc{cell, row, ev, N, E};
        cell += (int64_t)N * E;
        row += N;
        ev += E;
    }
    e = ragged_slot_upload(ctx, s, bytes);
    if (e != hipSuccess) return hip_fail(e, "ragged: descriptor upload");
    pcx::BatchArgs a = shared_args(in, out);
    a.B = B;
    e = pcx::launch_ragged(a, static_cast<const pcx::RaggedDesc*>(s.dev), (size_t)lds, ctx->stream);
    if (e == hipSuccess) e = hipEventRecord(s.kern_ev, ctx->stream);
    return e == hipSuccess ? PCX_OK : hip_fail(e, "ragged_round_kernel launch");
}

// where a round of a wide ragged batch runs: 0 = the one-wave kernel, else the workgroup kernel's
// launch class (pcx::medium_launch_class), or the one class of PCX_RAGGED_ONE_CLASS
static int wide_slot(int N, int E, int algorithm, bool one_class) {
    if (N <= 64 && E <= 32) return 0;
    return one_class ? 1 : pcx::medium_launch_class(pcx::medium_lds_bytes(N, E, algorithm));
}

static int ragged_plan_wide(int64_t n_rounds, const int32_t* n_reporters, const int32_t* n_events, int algorithm,
                            bool one_class, int64_t totals[3], int64_t counts[4], int64_t lds_bytes[4],
                            int64_t* bad_round) {
    if (const int rc = ragged_plan_checks(n_rounds, n_reporters, n_events, algorithm, bad_round)) return rc;
    int64_t tot[3] = {0, 0, 0}, cnt[4] = {0, 0, 0, 0};
    size_t lds[4] = {0, 0, 0, 0};
    for (int64_t b = 0; b < n_rounds; b++) {
        const int32_t N = n_reporters[b], E = n_events[b];
        if (N < 1 || N > 256 || E < 1 || E > 64) return ragged_bad_round(b, N, E, 256, 64, bad_round);
        tot[0] += N;
        tot[1] += E;
        tot[2] += (int64_t)N * E;
        const int k = wide_slot(N, E, algorithm, one_class);
        cnt[k]++;
        lds[k] = std::max(lds[k], k ? pcx::medium_lds_bytes(N, E, algorithm) : pcx::ragged_lds_bytes(N, E, algorithm));
    }
    for (int k = 0; k < 3 && totals; k++) totals[k] = tot[k];
    for (int k = 0; k < 4 && counts; k++) counts[k] = cnt[k];
    for (int k = 0; k < 4 && lds_bytes; k++) lds_bytes[k] = (int64_t)lds[k];
    return PCX_OK;
}

int pcx_ragged_plan_wide(int64_t n_rounds, const int32_t* n_reporters, const int32_t* n_events, int algorithm,
                         int64_t totals[3], int64_t counts[4], int64_t lds_bytes[4], int64_t* bad_round) {
    return ragged_plan_wide(n_rounds, n_reporters, n_events, algorithm, false, totals, counts, lds_bytes, bad_round);
}

int pcx_test_scratch_cap(pcx_ctx* ctx, int64_t bytes) {
    if (!ctx || bytes < 0) return fail(PCX_EINVAL, "pcx_test_scratch_cap: null context or negative bytes");
    ctx->test_scratch_cap = bytes;
    return PCX_OK;
}

// The descriptor tables of one wide ragged call in a staging slot, and what its launches need of
// them.  They depend on the rounds' shapes and the algorithm alone, not on any data pointer:
// pcx_consensus_ragged_wide_f64 builds them, uploads them and launches once; a simulator sweep
// (pcx_simulate_sweep_f64) builds and uploads them once and launches every timestep.
struct WidePlan {
    pcx_ctx::RaggedSlot* slot = nullptr;
    int64_t B = 0, nw = 0, nm = 0, chunk = 0;
    int64_t cnt[4] = {0, 0, 0, 0}, lds[4] = {0, 0, 0, 0}, first[4] = {0, 0, 0, 0}, stride[3] = {0, 0, 0};
    // slot offsets: the workgroup rounds' descriptors, the wave rounds' indices, the caller's `extra`
    // bytes; `bytes` are uploaded, the wave rounds' six [B] outputs follow at off_t on the device
    size_t off_m = 0, off_i = 0, off_x = 0, bytes = 0, off_t = 0;
    bool filled = false;  // the caller gives `filled`: no N x E scratch of the library's
};

// Plan's tables into a staging slot taken here (cnt / lds as ragged_plan_wide found them), the
// workgroup scratch reserved; `extra` bytes (a multiple of 8) of the caller's ride along at off_x.
// One staging slot, one upload: the wave rounds' descriptors, the workgroup rounds' descriptors
// class after class (3, 2, 1; a class's rounds in their order), the wave rounds' indices.  The
// device side holds, past what is uploaded, the wave rounds' six [B] outputs until their scatter.
// With wave rounds only (nm == 0) the first table is pcx_consensus_ragged_f64's own.
static int wide_tables(pcx_ctx* ctx, int64_t B, const int32_t* n_reporters, const int32_t* n_events, int algorithm,
                       bool one_class, const int64_t cnt[4], const int64_t lds[4], bool filled, size_t extra,
                       WidePlan* plan) {
    WidePlan& p = *plan;
    p.B = B;
    p.nw = cnt[0];
    p.nm = B - p.nw;
    p.filled = filled;
    for (int k = 0; k < 4; k++) {
        p.cnt[k] = cnt[k];
        p.lds[k] = lds[k];
    }
    const int64_t nw = p.nw, nm = p.nm;
    p.off_m = (size_t)nw * sizeof(pcx::RaggedDesc);
    p.off_i = p.off_m + (size_t)nm * sizeof(pcx::MediumDesc);
    p.off_x = (p.off_i + (size_t)nw * sizeof(int32_t) + 7) / 8 * 8;
    p.bytes = p.off_t = p.off_x + extra;
    if (const int rc = ragged_slot_take(ctx, p.off_t + (size_t)nw * 32, &p.slot)) return rc;
    char* pin = static_cast<char*>(p.slot->pin);
    pcx::RaggedDesc* dw = reinterpret_cast<pcx::RaggedDesc*>(pin);
    pcx::MediumDesc* dm = reinterpret_cast<pcx::MediumDesc*>(pin + p.off_m);
    int32_t* idx = reinterpret_cast<int32_t*>(pin + p.off_i);
    int64_t at[4] = {0, 0, 0, 0};  // next entry of each class in dm: class 3 first
    at[2] = cnt[3];
    at[1] = cnt[3] + cnt[2];
    for (int k = 0; k < 4; k++) p.first[k] = k ? at[k] : 0;
    int64_t cell = 0, row = 0, ev = 0, w = 0;
    for (int64_t b = 0; b < B; b++) {
        const int32_t N = n_reporters[b], E = n_events[b];
        const int k = wide_slot(N, E, algorithm, one_class);
        if (k == 0) {
            dw[w] = pcx::RaggedDesc{cell, row, ev, N, E};
            idx[w++] = (int32_t)b;
        } else {
            dm[at[k]++] = pcx::MediumDesc{cell, row, ev, N, E, (int32_t)b, 0};
            pcx::medium_slot_strides(N, E, algorithm, p.stride);
        }
        cell += (int64_t)N * E;
        row += N;
        ev += E;
    }
    if (nm == 0) return PCX_OK;
    // the workgroup scratch: slot strides of the call's largest round, chunks that fit the cap
    const size_t cap = ctx->test_scratch_cap > 0 ? (size_t)ctx->test_scratch_cap : MEDIUM_SCRATCH_CAP;
    const size_t per = (size_t)((filled ? 0 : p.stride[0]) + p.stride[1] + p.stride[2]) * sizeof(double);
    p.chunk = std::min<int64_t>(std::max<int64_t>((int64_t)(cap / per), 1), nm);
    return medium_scratch_reserve(ctx, per * (size_t)p.chunk);
}

// the launches of a wide ragged call over uploaded tables, with these inputs, options and outputs
static hipError_t wide_launch(pcx_ctx* ctx, const WidePlan& p, const pcx::BatchArgs& a) {
    char* dev = static_cast<char*>(p.slot->dev);
    const int64_t nw = p.nw;
    if (p.nm == 0)
        return pcx::launch_ragged(a, reinterpret_cast<const pcx::RaggedDesc*>(dev), (size_t)p.lds[0], ctx->stream);
    double* Fscr = (double*)ctx->mscr;
    double* Cscr = Fscr + (p.filled ? 0 : (size_t)p.chunk * p.stride[0]);
    double* Xscr = Cscr + (size_t)p.chunk * p.stride[1];
    hipError_t e = hipSuccess;
    if (nw > 0) {
        pcx::BatchArgs aw = a;
        aw.B = nw;
        const pcx::WaveTmp t = pcx::ragged_wave_tmp(dev + p.off_t, nw);
        aw.participation = t.participation;
        aw.avg_certainty = t.avg_certainty;
        aw.branch = t.branch;
        aw.flags = t.flags;
        aw.pi_iters = t.pi_iters;
        aw.components = t.components;
        e = pcx::launch_ragged(aw, reinterpret_cast<const pcx::RaggedDesc*>(dev), (size_t)p.lds[0], ctx->stream);
        if (e == hipSuccess)
            e = pcx::launch_ragged_scatter(a, reinterpret_cast<const int32_t*>(dev + p.off_i), nw, dev + p.off_t,
                                           ctx->stream);
    }
    const pcx::MediumDesc* ddm = reinterpret_cast<const pcx::MediumDesc*>(dev + p.off_m);
    for (int k = 3; k >= 1 && e == hipSuccess; k--)
        for (int64_t b0 = 0; b0 < p.cnt[k] && e == hipSuccess; b0 += p.chunk)
            e = pcx::launch_ragged_medium(a, ddm + p.first[k] + b0, std::min<int64_t>(p.chunk, p.cnt[k] - b0),
                                          (size_t)p.lds[k], p.stride, Fscr, Cscr, Xscr, ctx->stream);
    return e;
}

int pcx_consensus_ragged_wide_f64(pcx_ctx* ctx, const pcx_ragged* in, pcx_batch_result* out) {
    if (!ctx || !in || !out) return fail(PCX_EINVAL, "pcx_consensus_ragged_wide_f64: null argument");
    const char* env = getenv("PCX_RAGGED_ONE_CLASS");  // diagnostic: every workgroup round in one launch
    const bool one_class = env && env[0] == '1';
    int64_t cnt[4], lds[4];
    if (const int rc = ragged_plan_wide(in->n_rounds, in->n_reporters, in->n_events, in->algorithm, one_class, nullptr,
                                        cnt, lds, nullptr))
        return rc;
    if (in->n_rounds == 0) return PCX_OK;
    if (cnt[0] == in->n_rounds)  // wave-sized rounds only: that call as it is
        return pcx_consensus_ragged_f64(ctx, in, out);
    // (max_components is capped at E_b per round on the device)
    const bool bad_five = in->algorithm == PCX_ALG_BIG_FIVE && in->max_components < 1;
    if (const int rc = check_options("ragged", in, bad_five ? "big-five needs max_components >= 1" : nullptr))
        return rc;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    WidePlan p;
    if (const int rc = wide_tables(ctx, in->n_rounds, in->n_reporters, in->n_events, in->algorithm, one_class, cnt,
                                   lds, out->filled != nullptr, 0, &p))
        return rc;
    e = ragged_slot_upload(ctx, *p.slot, p.bytes);
    if (e != hipSuccess) return hip_fail(e, "ragged: descriptor upload");
    pcx::BatchArgs a = shared_args(in, out);
    a.B = in->n_rounds;
    e = wide_launch(ctx, p, a);
    if (e == hipSuccess) e = hipEventRecord(p.slot->kern_ev, ctx->stream);
    return e == hipSuccess ? PCX_OK : hip_fail(e, "ragged wide launch");
}

// ---------------------------------------------------------------- per-round parameters
static_assert(sizeof(pcx_round_params) == sizeof(pcx::RoundParams), "pcx_round_params is the device entry");

// why a parameter set is refused (the words of check_options / sweep_check), or NULL.  sim: a
// simulator cell's set, where k-means and cokurtosis are not simulated.  kmeans_ok: an entry that
// takes code books (pcx_consensus_ragged_kmeans_f64).
static const char* params_set_refusal(const pcx_round_params& q, bool sim, bool kmeans_ok = false) {
    if (q.algorithm < PCX_ALG_PCA || q.algorithm > PCX_ALG_CLUSTERFECK)
        return "algorithm must be an enum pcx_algorithm value (0..7)";
    if (q.algorithm == PCX_ALG_KMEANS && !kmeans_ok)
        return sim ? "k-means is not simulated (its code books are drawn on the host)"
                   : "k-means is not supported (its code-book size depends on each round's N)";
    if (sim && q.algorithm == PCX_ALG_COKURTOSIS) return "cokurtosis is not simulated (it needs the caller's scores)";
    // (max_components is capped at E_b per round on the device)
    if (q.algorithm == PCX_ALG_BIG_FIVE && q.max_components < 1) return "big-five needs max_components >= 1";
    if (q.algorithm == PCX_ALG_HIERARCHICAL && std::isnan(q.hierarchy_threshold)) return "hierarchy_threshold is NaN";
    if (q.algorithm == PCX_ALG_FIXED_VARIANCE && !std::isfinite(q.variance_threshold))
        return "variance_threshold must be finite";
    if (!std::isfinite(q.catch_tolerance) || !std::isfinite(q.alpha)) return "catch_tolerance/alpha must be finite";
    return nullptr;
}

// The launches of a call with per-round parameters: nine segments of one descriptor table
// (MediumDesc, every round's), each one launch (the workgroup ones times the scratch chunks).
// 0..2: the one-wave kernel's instantiation groups (pcx::params_wave_group); 3..5: the workgroup
// kernel's plain instantiation, launch classes 3, 2, 1; 6..8: its CLUS instantiation likewise.
constexpr int PARAMS_SEGMENTS = 9;
static int params_segment(int N, int E, int algorithm) {
    if (N <= 64 && E <= 32) return pcx::params_wave_group(algorithm);
    const int k = pcx::medium_launch_class(pcx::medium_lds_bytes(N, E, algorithm));
    return 3 + (algorithm >= PCX_ALG_KMEANS ? 3 : 0) + (3 - k);
}

// a round's segment and dynamic LDS, remembered over a run of equal rounds (a simulator cell's: the
// host passes over a sweep's 10^4..10^5 rounds lie between the call and its first launch)
struct SegmentOf {
    int N = 0, E = 0, alg = -1, seg = 0;
    int64_t lds = 0;
    bool fresh = false;  // the last at() computed (a new run)
    int at(int n, int e, int a) {
        fresh = n != N || e != E || a != alg;
        if (fresh) {
            N = n, E = e, alg = a;
            seg = params_segment(n, e, a);
            lds = (int64_t)(seg < 3 ? pcx::ragged_lds_bytes(n, e, a) : pcx::medium_lds_bytes(n, e, a));
        }
        return seg;
    }
};

struct ParamsPlan {
    pcx_ctx::RaggedSlot* slot = nullptr;
    int64_t B = 0, P = 0, nm = 0, chunk = 0;
    int64_t cnt[PARAMS_SEGMENTS] = {}, lds[PARAMS_SEGMENTS] = {}, first[PARAMS_SEGMENTS] = {};
    int64_t stride[3] = {0, 0, 0};
    // slot offsets: the parameter table, the caller's `extra` bytes; `bytes` are uploaded
    size_t off_p = 0, off_x = 0, bytes = 0;
    bool filled = false;
};

// a segment's count and dynamic LDS (the largest round's own, by its own algorithm) and the
// workgroup rounds' slot strides, of rounds that the caller has checked
static void params_count(int64_t B, const int32_t* n_reporters, const int32_t* n_events, const pcx_round_params* params,
                         const int32_t* param_of, ParamsPlan* plan) {
    ParamsPlan& p = *plan;
    p.B = B;
    SegmentOf run;
    for (int64_t b = 0; b < B; b++) {
        const int N = n_reporters[b], E = n_events[b], alg = params[param_of[b]].algorithm;
        const int s = run.at(N, E, alg);
        p.cnt[s]++;
        if (s >= 3) p.nm++;
        if (!run.fresh) continue;
        p.lds[s] = std::max(p.lds[s], run.lds);
        if (s >= 3) pcx::medium_slot_strides(N, E, alg, p.stride);
    }
    for (int s = 1; s < PARAMS_SEGMENTS; s++) p.first[s] = p.first[s - 1] + p.cnt[s - 1];
}

static int params_plan_check(int64_t n_rounds, const int32_t* n_reporters, const int32_t* n_events, int64_t n_params,
                             const pcx_round_params* params, const int32_t* param_of, int64_t totals[3],
                             int64_t* bad_round, int64_t* bad_param, bool kmeans_ok = false) {
    if (bad_round) *bad_round = -1;
    if (bad_param) *bad_param = -1;
    if (n_rounds < 0 || n_rounds > 0x7fffffff) return fail(PCX_EINVAL, "ragged: n_rounds must be in [0, 2^31)");
    if (n_rounds > 0 && (!n_reporters || !n_events)) return fail(PCX_EINVAL, "ragged: n_reporters / n_events is NULL");
    if (n_rounds > 0 && n_params < 1) return fail(PCX_EINVAL, "ragged: n_params must be >= 1 (a parameter set per round)");
    if (n_params > 0x7fffffff) return fail(PCX_EINVAL, "ragged: n_params must be below 2^31");
    if (n_params > 0 && !params) return fail(PCX_EINVAL, "ragged: params is NULL");
    if (n_rounds > 0 && !param_of) return fail(PCX_EINVAL, "ragged: param_of is NULL");
    for (int64_t q = 0; q < n_params; q++)
        if (const char* why = params_set_refusal(params[q], false, kmeans_ok)) {
            if (bad_param) *bad_param = q;
            return fail(PCX_EINVAL, "ragged: parameter set " + std::to_string(q) + ": " + why);
        }
    int64_t tot[3] = {0, 0, 0};
    for (int64_t b = 0; b < n_rounds; b++) {
        const int32_t N = n_reporters[b], E = n_events[b];
        if (N < 1 || N > 256 || E < 1 || E > 64) return ragged_bad_round(b, N, E, 256, 64, bad_round);
        if (param_of[b] < 0 || param_of[b] >= n_params) {
            if (bad_round) *bad_round = b;
            return fail(PCX_EINVAL, "ragged: round " + std::to_string(b) + " has param_of " + std::to_string(param_of[b]) +
                                        ", outside [0, " + std::to_string(n_params) + ")");
        }
        tot[0] += N;
        tot[1] += E;
        tot[2] += (int64_t)N * E;
    }
    for (int k = 0; k < 3 && totals; k++) totals[k] = tot[k];
    return PCX_OK;
}

int pcx_ragged_plan_params(int64_t n_rounds, const int32_t* n_reporters, const int32_t* n_events, int64_t n_params,
                           const pcx_round_params* params, const int32_t* param_of, int64_t totals[3],
                           int64_t* n_launches, int64_t* bad_round, int64_t* bad_param) {
    if (const int rc = params_plan_check(n_rounds, n_reporters, n_events, n_params, params, param_of, totals, bad_round,
                                         bad_param))
        return rc;
    if (n_launches) {
        ParamsPlan p;
        params_count(n_rounds, n_reporters, n_events, params, param_of, &p);
        *n_launches = 0;
        for (int s = 0; s < PARAMS_SEGMENTS; s++) *n_launches += p.cnt[s] > 0;
    }
    return PCX_OK;
}

// A counted plan's tables into a staging slot taken here: every round's descriptor, segment after
// segment (a segment's rounds in their order), then the P parameter entries, then `extra` bytes (a
// multiple of 8) of the caller's at off_x; the workgroup scratch reserved.  One slot, one upload.
static int params_tables(pcx_ctx* ctx, const int32_t* n_reporters, const int32_t* n_events, int64_t n_params,
                         const pcx_round_params* params, const int32_t* param_of, bool filled, size_t extra,
                         ParamsPlan* plan) {
    ParamsPlan& p = *plan;
    p.P = n_params;
    p.filled = filled;
    p.off_p = (size_t)p.B * sizeof(pcx::MediumDesc);
    p.off_x = p.off_p + (size_t)n_params * sizeof(pcx::RoundParams);
    p.bytes = p.off_x + extra;
    if (const int rc = ragged_slot_take(ctx, p.bytes, &p.slot)) return rc;
    char* pin = static_cast<char*>(p.slot->pin);
    pcx::MediumDesc* d = reinterpret_cast<pcx::MediumDesc*>(pin);
    int64_t at[PARAMS_SEGMENTS];
    for (int s = 0; s < PARAMS_SEGMENTS; s++) at[s] = p.first[s];
    int64_t cell = 0, row = 0, ev = 0;
    SegmentOf run;
    for (int64_t b = 0; b < p.B; b++) {
        const int32_t N = n_reporters[b], E = n_events[b];
        const int s = run.at(N, E, params[param_of[b]].algorithm);
        d[at[s]++] = pcx::MediumDesc{cell, row, ev, N, E, (int32_t)b, param_of[b]};
        cell += (int64_t)N * E;
        row += N;
        ev += E;
    }
    std::memcpy(pin + p.off_p, params, (size_t)n_params * sizeof(pcx::RoundParams));
    if (p.nm == 0) return PCX_OK;
    // the workgroup scratch: slot strides of the call's largest round, chunks that fit the cap
    const size_t cap = ctx->test_scratch_cap > 0 ? (size_t)ctx->test_scratch_cap : MEDIUM_SCRATCH_CAP;
    const size_t per = (size_t)((filled ? 0 : p.stride[0]) + p.stride[1] + p.stride[2]) * sizeof(double);
    p.chunk = std::min<int64_t>(std::max<int64_t>((int64_t)(cap / per), 1), p.nm);
    return medium_scratch_reserve(ctx, per * (size_t)p.chunk);
}

// the launches over uploaded tables, with these inputs and outputs (a's parameter fields are not read)
static hipError_t params_launch(pcx_ctx* ctx, const ParamsPlan& p, const pcx::BatchArgs& a) {
    char* dev = static_cast<char*>(p.slot->dev);
    const pcx::MediumDesc* d = reinterpret_cast<const pcx::MediumDesc*>(dev);
    const pcx::RoundParams* tab = reinterpret_cast<const pcx::RoundParams*>(dev + p.off_p);
    hipError_t e = hipSuccess;
    for (int g = 0; g < 3 && e == hipSuccess; g++)
        e = pcx::launch_ragged_params(a, d + p.first[g], tab, p.cnt[g], g, (size_t)p.lds[g], ctx->stream);
    if (p.nm == 0) return e;
    double* Fscr = (double*)ctx->mscr;
    double* Cscr = Fscr + (p.filled ? 0 : (size_t)p.chunk * p.stride[0]);
    double* Xscr = Cscr + (size_t)p.chunk * p.stride[1];
    for (int s = 3; s < PARAMS_SEGMENTS && e == hipSuccess; s++)
        for (int64_t b0 = 0; b0 < p.cnt[s] && e == hipSuccess; b0 += p.chunk)
            e = pcx::launch_ragged_medium_params(a, d + p.first[s] + b0, tab, std::min<int64_t>(p.chunk, p.cnt[s] - b0),
                                                 s >= 6, (size_t)p.lds[s], p.stride, Fscr, Cscr, Xscr, ctx->stream);
    return e;
}

int pcx_consensus_ragged_params_f64(pcx_ctx* ctx, const pcx_ragged* in, int64_t n_params,
                                    const pcx_round_params* params, const int32_t* param_of, pcx_batch_result* out) {
    if (!ctx || !in || !out) return fail(PCX_EINVAL, "pcx_consensus_ragged_params_f64: null argument");
    if (const int rc = params_plan_check(in->n_rounds, in->n_reporters, in->n_events, n_params, params, param_of,
                                         nullptr, nullptr, nullptr))
        return rc;
    if (in->n_rounds == 0) return PCX_OK;
    if (!in->reports) return fail(PCX_EINVAL, "ragged: reports is NULL");
    if (in->scaled && (!in->lo || !in->hi)) return fail(PCX_EINVAL, "ragged: scaled given without lo/hi");
    for (int64_t b = 0; b < in->n_rounds && !in->aux_scores; b++)
        if (params[param_of[b]].algorithm == PCX_ALG_COKURTOSIS)
            return fail(PCX_EINVAL, "ragged: parameter set " + std::to_string(param_of[b]) +
                                        ": cokurtosis needs aux_scores (aux[\"cokurt\"])");
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    ParamsPlan p;
    params_count(in->n_rounds, in->n_reporters, in->n_events, params, param_of, &p);
    if (const int rc = params_tables(ctx, in->n_reporters, in->n_events, n_params, params, param_of,
                                     out->filled != nullptr, 0, &p))
        return rc;
    e = ragged_slot_upload(ctx, *p.slot, p.bytes);
    if (e != hipSuccess) return hip_fail(e, "ragged: descriptor upload");
    pcx::BatchArgs a = shared_args(in, out);
    a.B = in->n_rounds;
    e = params_launch(ctx, p, a);
    if (e == hipSuccess) e = hipEventRecord(p.slot->kern_ev, ctx->stream);
    return e == hipSuccess ? PCX_OK : hip_fail(e, "ragged params launch");
}

// ---------------------------------------------------------------- k-means in ragged batches
// the reference's code-book size int(ceil(sqrt(N))) (:396), in integers (N <= 256)
static int kmeans_rule(int N) {
    int k = 1;
    while (k * k < N) k++;
    return k;
}

// The flat book layout of the rounds whose set params[param_of[b]] is k-means (params NULL: every
// round), of rounds whose
// shapes the caller has checked: offsets[b] = the books before round b's, offsets[B] the length.
// Refuses a k_b outside [1, min(N_b, 8)] within 64 x 32 (the one-wave kernel's code-book rows),
// [1, min(N_b, 16)] above (the workgroup kernel's), with the round named.
static int kmeans_layout(int64_t B, const int32_t* n_reporters, const int32_t* n_events, const int32_t* k, int restarts,
                         const pcx_round_params* params, const int32_t* param_of, int64_t* offsets,
                         pcx::KmeansEntry* entries, int64_t* bad_round, int64_t* total = nullptr) {
    int64_t at = 0;
    for (int64_t b = 0; b < B; b++) {
        if (offsets) offsets[b] = at;
        if (entries) entries[b] = pcx::KmeansEntry{0, 0, 0};
        if (params && params[param_of[b]].algorithm != PCX_ALG_KMEANS) continue;
        const int N = n_reporters[b], E = n_events[b];
        const int kmax = std::min(N, N <= 64 && E <= 32 ? 8 : 16);
        const int kb = k ? k[b] : kmeans_rule(N);
        if (kb < 1 || kb > kmax) {
            if (bad_round) *bad_round = b;
            return fail(PCX_EINVAL, "k-means: round " + std::to_string(b) + " (" + std::to_string(N) + " x " +
                                        std::to_string(E) + ") has a code book of " + std::to_string(kb) +
                                        " rows; it must be within [1, " + std::to_string(kmax) + "]");
        }
        if (entries) entries[b] = pcx::KmeansEntry{at, kb, 0};
        at += (int64_t)restarts * kb;
    }
    if (offsets) offsets[B] = at;
    if (total) *total = at;
    return PCX_OK;
}

int pcx_kmeans_plan(int64_t n_rounds, const int32_t* n_reporters, const int32_t* n_events, const int32_t* k,
                    int32_t restarts, int64_t* offsets, int64_t* bad_round) {
    if (bad_round) *bad_round = -1;
    if (n_rounds < 0 || n_rounds > 0x7fffffff) return fail(PCX_EINVAL, "k-means: n_rounds must be in [0, 2^31)");
    if (restarts < 1) return fail(PCX_EINVAL, "k-means: restarts must be >= 1");
    if (n_rounds > 0 && (!n_reporters || !n_events)) return fail(PCX_EINVAL, "k-means: n_reporters / n_events is NULL");
    for (int64_t b = 0; b < n_rounds; b++) {
        const int32_t N = n_reporters[b], E = n_events[b];
        if (N < 1 || N > 256 || E < 1 || E > 64) return ragged_bad_round(b, N, E, 256, 64, bad_round);
    }
    return kmeans_layout(n_rounds, n_reporters, n_events, k, restarts, nullptr, nullptr, offsets, nullptr, bad_round);
}

// pcx_ragged_plan_kmeans' checks; *any = some round's set is k-means
static int kmeans_plan_check(int64_t n_rounds, const int32_t* n_reporters, const int32_t* n_events, int64_t n_params,
                             const pcx_round_params* params, const int32_t* param_of, const pcx_kmeans_books* books,
                             int64_t totals[3], int64_t* offsets, pcx::KmeansEntry* entries, int64_t* bad_round,
                             int64_t* bad_param, bool* any) {
    if (const int rc = params_plan_check(n_rounds, n_reporters, n_events, n_params, params, param_of, totals, bad_round,
                                         bad_param, true))
        return rc;
    bool some = false;
    for (int64_t b = 0; b < n_rounds && !some; b++) some = params[param_of[b]].algorithm == PCX_ALG_KMEANS;
    if (any) *any = some;
    if (some && !books) return fail(PCX_EINVAL, "k-means: a round's set is k-means and books is NULL");
    if (some && books->restarts < 1) return fail(PCX_EINVAL, "k-means: restarts must be >= 1");
    return kmeans_layout(n_rounds, n_reporters, n_events, some ? books->k : nullptr, some ? books->restarts : 0, params,
                         param_of, offsets, entries, bad_round);
}

int pcx_ragged_plan_kmeans(int64_t n_rounds, const int32_t* n_reporters, const int32_t* n_events, int64_t n_params,
                           const pcx_round_params* params, const int32_t* param_of, const pcx_kmeans_books* books,
                           int64_t totals[3], int64_t* n_launches, int64_t* offsets, int64_t* bad_round,
                           int64_t* bad_param) {
    if (const int rc = kmeans_plan_check(n_rounds, n_reporters, n_events, n_params, params, param_of, books, totals,
                                         offsets, nullptr, bad_round, bad_param, nullptr))
        return rc;
    if (n_launches) {
        ParamsPlan p;
        params_count(n_rounds, n_reporters, n_events, params, param_of, &p);
        *n_launches = 0;
        for (int s = 0; s < PARAMS_SEGMENTS; s++) *n_launches += p.cnt[s] > 0;
    }
    return PCX_OK;
}

// params_launch with the clustering segments (one-wave group 2, workgroup 6..8) on the k-means form
// (books: the per-round book table on the device, somewhere in the slot's `extra` bytes)
static hipError_t kmeans_launch(pcx_ctx* ctx, const ParamsPlan& p, const pcx::BatchArgs& a,
                                const pcx::KmeansEntry* books) {
    char* dev = static_cast<char*>(p.slot->dev);
    const pcx::MediumDesc* d = reinterpret_cast<const pcx::MediumDesc*>(dev);
    const pcx::RoundParams* tab = reinterpret_cast<const pcx::RoundParams*>(dev + p.off_p);
    hipError_t e = hipSuccess;
    for (int g = 0; g < 2 && e == hipSuccess; g++)
        e = pcx::launch_ragged_params(a, d + p.first[g], tab, p.cnt[g], g, (size_t)p.lds[g], ctx->stream);
    if (e == hipSuccess)
        e = pcx::launch_ragged_kmeans(a, d + p.first[2], tab, books, p.cnt[2], (size_t)p.lds[2], ctx->stream);
    if (p.nm == 0) return e;
    double* Fscr = (double*)ctx->mscr;
    double* Cscr = Fscr + (p.filled ? 0 : (size_t)p.chunk * p.stride[0]);
    double* Xscr = Cscr + (size_t)p.chunk * p.stride[1];
    for (int s = 3; s < PARAMS_SEGMENTS && e == hipSuccess; s++)
        for (int64_t b0 = 0; b0 < p.cnt[s] && e == hipSuccess; b0 += p.chunk) {
            const int64_t nb = std::min<int64_t>(p.chunk, p.cnt[s] - b0);
            e = s >= 6 ? pcx::launch_ragged_medium_kmeans(a, d + p.first[s] + b0, tab, books, nb, (size_t)p.lds[s], p.stride,
                                                          Fscr, Cscr, Xscr, ctx->stream)
                       : pcx::launch_ragged_medium_params(a, d + p.first[s] + b0, tab, nb, false, (size_t)p.lds[s],
                                                          p.stride, Fscr, Cscr, Xscr, ctx->stream);
        }
    return e;
}

int pcx_consensus_ragged_kmeans_f64(pcx_ctx* ctx, const pcx_ragged* in, int64_t n_params,
                                    const pcx_round_params* params, const int32_t* param_of,
                                    const pcx_kmeans_books* books, pcx_batch_result* out) {
    if (!ctx || !in || !out) return fail(PCX_EINVAL, "pcx_consensus_ragged_kmeans_f64: null argument");
    const int64_t B = in->n_rounds;
    bool any = false;
    // (the checks first, without a table: a refusal takes no staging slot)
    if (const int rc = kmeans_plan_check(B, in->n_reporters, in->n_events, n_params, params, param_of, books, nullptr,
                                         nullptr, nullptr, nullptr, nullptr, &any))
        return rc;
    if (B == 0) return PCX_OK;
    if (!in->reports) return fail(PCX_EINVAL, "ragged: reports is NULL");
    if (in->scaled && (!in->lo || !in->hi)) return fail(PCX_EINVAL, "ragged: scaled given without lo/hi");
    if (any && !books->init) return fail(PCX_EINVAL, "k-means: books->init is NULL");
    for (int64_t b = 0; b < B && !in->aux_scores; b++)
        if (params[param_of[b]].algorithm == PCX_ALG_COKURTOSIS)
            return fail(PCX_EINVAL, "ragged: parameter set " + std::to_string(param_of[b]) +
                                        ": cokurtosis needs aux_scores (aux[\"cokurt\"])");
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    ParamsPlan p;
    params_count(B, in->n_reporters, in->n_events, params, param_of, &p);
    if (const int rc = params_tables(ctx, in->n_reporters, in->n_events, n_params, params, param_of,
                                     out->filled != nullptr, (size_t)B * sizeof(pcx::KmeansEntry), &p))
        return rc;
    // the per-round book table, behind the parameter entries in the one upload
    pcx::KmeansEntry* entries = reinterpret_cast<pcx::KmeansEntry*>(static_cast<char*>(p.slot->pin) + p.off_x);
    if (const int rc = kmeans_layout(B, in->n_reporters, in->n_events, any ? books->k : nullptr, any ? books->restarts : 0,
                                     params, param_of, nullptr, entries, nullptr))
        return rc;
    e = ragged_slot_upload(ctx, *p.slot, p.bytes);
    if (e != hipSuccess) return hip_fail(e, "ragged: descriptor upload");
    pcx::BatchArgs a = shared_args(in, out);
    a.B = B;
    a.kmeans_restarts = any ? books->restarts : 0;
    a.kmeans_init = any ? books->init : nullptr;
    e = kmeans_launch(ctx, p, a, reinterpret_cast<const pcx::KmeansEntry*>(static_cast<char*>(p.slot->dev) + p.off_x));
    if (e == hipSuccess) e = hipEventRecord(p.slot->kern_ev, ctx->stream);
    return e == hipSuccess ? PCX_OK : hip_fail(e, "ragged k-means launch");
}

namespace {
// pcx_create_devices context: shard the host matrix's rows over the devices, one
// worker thread per device running the rank's consensus (collective over the ranks)
int run_devices(pcx_ctx* ctx, const pcx_problem* p, pcx_result* r, int entry, const double* scores, int rank_rule,
                double* nc, std::string& err) {
    const int n = (int)ctx->sub.size();
    const int64_t N = p->n_rows, E = p->n_events;
    if (p->mem_kind != PCX_MEM_HOST) {
        err = "a multi-device context takes the matrix in host memory (PCX_MEM_HOST)";
        return PCX_EINVAL;
    }
    if (p->n_total != N || p->row_offset != 0) {
        err = "a multi-device context takes the whole matrix (n_total == n_rows, row_offset 0)";
        return PCX_EINVAL;
    }
    if (N < n || E < 1 || !p->reports) {
        err = "bad shape (fewer rows than devices) or missing reports";
        return PCX_EINVAL;
    }
    // the rank-independent checks once, here: a bad argument fails before any worker starts,
    // so it never takes the abort path below (which leaves an RCCL context unusable)
    if (const int rc = pcx::check_problem(p, n, entry, err)) return rc;
    std::vector<pcx_problem> ps(n, *p);
    std::vector<pcx_result> rs(n);
    std::vector<std::string> errs(n);
    std::vector<int> rcs;
    const int64_t base = N / n, rem = N % n;
    auto at = [](double* a, int64_t off) { return a ? a + off : nullptr; };
    for (int k = 0; k < n; k++) {
        const int64_t off = k * base + (k < rem ? k : rem), cnt = base + (k < rem ? 1 : 0);
        pcx_problem& q = ps[k];
        q.n_rows = cnt;
        q.n_total = N;
        q.row_offset = off;
        q.reports = p->reports + off * E;
        q.aux_scores = p->aux_scores ? p->aux_scores + off : nullptr;
        pcx_result& o = rs[k];
        o = pcx_result{};
        o.old_rep = at(r->old_rep, off);
        o.this_rep = at(r->this_rep, off);
        o.smooth_rep = at(r->smooth_rep, off);
        o.scores = at(r->scores, off);
        o.na_row = at(r->na_row, off);
        o.participation_rows = at(r->participation_rows, off);
        o.relative_part = at(r->relative_part, off);
        o.reporter_bonus = at(r->reporter_bonus, off);
        o.original = at(r->original, off * E);
        o.filled = at(r->filled, off * E);
        if (k == 0) {  // event vectors are identical on every rank: device 0 writes them
            o.adj_first_loadings = r->adj_first_loadings;
            o.outcomes_raw = r->outcomes_raw;
            o.outcomes_adjusted = r->outcomes_adjusted;
            o.outcomes_final = r->outcomes_final;
            o.certainty = r->certainty;
            o.consensus_reward = r->consensus_reward;
            o.nas_filled = r->nas_filled;
            o.participation_columns = r->participation_columns;
            o.author_bonus = r->author_bonus;
            o.weighted_mean = r->weighted_mean;
            o.covariance = r->covariance;
        }
    }
    // the first failing worker releases the ranks waiting on it in an exchange: it aborts every
    // other rank's communicator (RCCL: ncclCommAbort; group: pcx_group::abort)
    pcx::run_workers(
        n,
        [&](int k) {
            const int64_t off = ps[k].row_offset;
            return pcx::run_matrix(ctx->sub[k], &ps[k], &rs[k], entry, scores ? scores + off : nullptr, rank_rule,
                                   nc ? nc + off : nullptr, errs[k]);
        },
        [&](int k) {
            if (ctx->group) pcx::group_abort(ctx->group);
            for (pcx_ctx* o : ctx->sub)
                if (o->comm && o != ctx->sub[k]) o->comm->abort();
        },
        rcs);
    if (ctx->group) pcx::group_reset(ctx->group);  // every worker has left the exchange
    int first = -1;
    for (int k = 0; k < n && first < 0; k++)
        if (rcs[k] && errs[k].find("exchange aborted") == std::string::npos) first = k;
    for (int k = first < 0 ? 0 : first; k < n; k++)
        if (rcs[k]) {
            err = "device " + std::to_string(ctx->sub[k]->device) + " (rank " + std::to_string(k) + "): " + errs[k];
            return rcs[k];
        }
    double bytes = 0;
    for (int k = 0; k < n; k++) bytes += rs[k].comm_bytes;
    const pcx_result& z = rs[0];
    r->participation = z.participation;
    r->avg_certainty = z.avg_certainty;
    r->branch = z.branch;
    r->flags = z.flags;
    r->pi_iters = z.pi_iters;
    r->components = z.components;
    r->n_hard = z.n_hard;
    r->sel_passes = z.sel_passes;
    r->comm_bytes = bytes;
    r->grid_events = z.grid_events;
    r->mixed_int8 = z.mixed_int8;
    return 0;
}

int run(pcx_ctx* ctx, const pcx_problem* p, pcx_result* r, int entry, const double* scores, int rank_rule, double* nc,
        const char* who) {
    if (!ctx || !p || !r) return fail(PCX_EINVAL, std::string(who) + ": null argument");
    std::string err;
    if (!ctx->sub.empty()) {
        const int rc = run_devices(ctx, p, r, entry, scores, rank_rule, nc, err);
        return rc ? fail(rc, std::string(who) + ": " + err) : PCX_OK;
    }
    const int rc = pcx::run_matrix(ctx, p, r, entry, scores, rank_rule, nc, err);
    return rc ? fail(rc, std::string(who) + ": " + err) : PCX_OK;
}
}  // namespace

int pcx_consensus_f64(pcx_ctx* ctx, const pcx_problem* p, pcx_result* r) {
    return run(ctx, p, r, 0, nullptr, 0, nullptr, "pcx_consensus_f64");
}

int pcx_interpolate_f64(pcx_ctx* ctx, const pcx_problem* p, pcx_result* r) {
    return run(ctx, p, r, 1, nullptr, 0, nullptr, "pcx_interpolate_f64");
}

int pcx_wpca_f64(pcx_ctx* ctx, const pcx_problem* p, pcx_result* r) {
    return run(ctx, p, r, 2, nullptr, 0, nullptr, "pcx_wpca_f64");
}

int pcx_lie_detector_f64(pcx_ctx* ctx, const pcx_problem* p, pcx_result* r) {
    return run(ctx, p, r, 3, nullptr, 0, nullptr, "pcx_lie_detector_f64");
}

int pcx_nonconformity_f64(pcx_ctx* ctx, const pcx_problem* p, const double* scores, int rank_rule, double* nc,
                          pcx_result* r) {
    if (!scores || !nc) return fail(PCX_EINVAL, "pcx_nonconformity_f64: scores and nc are required");
    return run(ctx, p, r, 4, scores, rank_rule, nc, "pcx_nonconformity_f64");
}

int pcx_profile_enable(pcx_ctx* ctx, int on) {
    if (!ctx) return fail(PCX_EINVAL, "pcx_profile_enable: null context");
    for (pcx_ctx* s : ctx->sub) s->profile = on ? 1 : 0;
    ctx->profile = on ? 1 : 0;
    return PCX_OK;
}

int pcx_profile_read(pcx_ctx* ctx, double* ms) {
    if (!ctx || !ms) return fail(PCX_EINVAL, "pcx_profile_read: null argument");
    const pcx_ctx* src = ctx->sub.empty() ? ctx : ctx->sub[0];  // multi-device: device 0's stages
    for (int k = 0; k < PCX_NSTAGES; k++) ms[k] = src->stage_ms[k];
    return PCX_OK;
}

const char* pcx_stage_name(int k) { return pcx::stage_name(k); }

int pcx_ctx_progress(const pcx_ctx* ctx, int* stage, int* host_waiting) {
    if (!ctx || !stage || !host_waiting) return fail(PCX_EINVAL, "pcx_ctx_progress: null argument");
    const pcx_ctx* src = ctx->sub.empty() ? ctx : ctx->sub[0];
    *stage = src->progress_stage.load(std::memory_order_relaxed);
    *host_waiting = src->progress_wait.load(std::memory_order_relaxed);
    return PCX_OK;
}

double pcx_seqsum_const(double c, int64_t k) { return pcx::seqsum_const(c, k); }

int64_t pcx_seqsum_first_above(double c, double t, int64_t kmax) { return pcx::seqsum_first_above(c, t, kmax); }
int pcx_mixed_digits(void) { return PCX_NDIG; }
int pcx_rccl_version(int* runtime, int* compiled) { return pcx::rccl_version(runtime, compiled); }
int pcx_selftest_abort_once(int users, int aborters, int iters) {
    return pcx::selftest_abort_once(users, aborters, iters, 0);
}
int pcx_selftest_abort_slow_holder(int users, int aborters) {
    return pcx::selftest_abort_once(users, aborters, 1, 1);
}
int pcx_selftest_group_abort(int world, int steps, int fail_rank, int fail_step) {
    return pcx::selftest_group_abort(world, steps, fail_rank, fail_step);
}
int pcx_selftest_rounds_sched(int workers, int64_t rounds, int enomem_worker, int64_t fail_round) {
    return pcx::selftest_rounds_sched(workers, rounds, enomem_worker, fail_round);
}
int pcx_selftest_chunked_copy(int64_t bytes, int64_t chunk, int slots, int threads, int64_t fail_chunk) {
    return pcx::selftest_chunked_copy(bytes, chunk, slots, threads, fail_chunk);
}
int64_t pcx_medium_lds_bytes(int n_reporters, int n_events, int algorithm) {
    if (!pcx::medium_fits(n_reporters, n_events, algorithm, 1)) return 0;
    return (int64_t)pcx::medium_lds_bytes(n_reporters, n_events, algorithm);
}

int64_t pcx_batched_lds_bytes(int n_reporters, int n_events, int algorithm) {
    if (n_reporters < 1 || n_reporters > 64 || n_events < 1 || n_events > 32) return -1;
    return (int64_t)pcx::batched_lds_bytes(n_reporters, n_events, algorithm);
}
int pcx_test_inject_enomem(pcx_ctx* ctx, int worker) {
    if (!ctx) return fail(PCX_EINVAL, "pcx_test_inject_enomem: null context");
    ctx->test_enomem_worker = worker;
    return PCX_OK;
}

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
    const struct {
        const char* name;
        double p;
    } probs[] = {{"liar_frac", s->liar_frac}, {"collude_frac", s->collude_frac}, {"distort", s->distort},
                 {"na_frac", s->na_frac},     {"scaled_frac", s->scaled_frac}};
    for (const auto& q : probs)
        if (!(q.p >= 0.0 && q.p <= 1.0))  // false for NaN too
            return fail(PCX_EINVAL, w + q.name + " must be a probability in [0, 1]");
    if (!(s->scaled_tol >= 0.0) || !std::isfinite(s->scaled_tol))
        return fail(PCX_EINVAL, w + "scaled_tol must be finite and >= 0");
    if (s->algorithm < PCX_ALG_PCA || s->algorithm > PCX_ALG_CLUSTERFECK)
        return fail(PCX_EINVAL, w + "algorithm must be an enum pcx_algorithm value (0..7)");
    if (s->algorithm == PCX_ALG_KMEANS && !kmeans_ok)
        return fail(PCX_EINVAL, w + "k-means is not simulated (its code books are drawn on the host)");
    if (s->algorithm == PCX_ALG_COKURTOSIS)
        return fail(PCX_EINVAL, w + "cokurtosis is not simulated (it needs the caller's scores)");
    // what pcx_consensus_batched_f64 would refuse, before anything is generated
    if (s->algorithm == PCX_ALG_HIERARCHICAL && std::isnan(s->hierarchy_threshold))
        return fail(PCX_EINVAL, w + "hierarchy_threshold is NaN");
    if (s->algorithm == PCX_ALG_BIG_FIVE && (s->max_components < 1 || s->max_components > s->n_events))
        return fail(PCX_EINVAL, w + "big-five needs 1 <= max_components <= n_events");
    if (s->algorithm == PCX_ALG_FIXED_VARIANCE && !std::isfinite(s->variance_threshold))
        return fail(PCX_EINVAL, w + "variance_threshold must be finite");
    if (!std::isfinite(s->catch_tolerance) || !std::isfinite(s->alpha))
        return fail(PCX_EINVAL, w + "catch_tolerance/alpha must be finite");
    return PCX_OK;
}

int sim_check_timestep(int t, const char* who) {
    if (t < 0 || t >= (1 << 24)) return fail(PCX_EINVAL, std::string(who) + ": timestep must be in [0, 2^24)");
    return PCX_OK;
}

uint64_t sim_threshold(double p) { return (uint64_t)std::floor(p * 4294967296.0); }

pcx::sim::Gen sim_gen(const pcx_sim* s) {
    pcx::sim::Gen g;
    g.key0 = (uint32_t)s->seed;
    g.key1 = (uint32_t)(s->seed >> 32);
    g.thr_liar = sim_threshold(s->liar_frac);
    g.thr_collude = sim_threshold(s->collude_frac);
    g.thr_distort = sim_threshold(s->distort);
    g.thr_na = sim_threshold(s->na_frac);
    g.thr_scaled = sim_threshold(s->scaled_frac);
    return g;
}

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

// the reference's code-book size int(ceil(sqrt(N))) (:396) for any N, in integers
static int64_t sim_kmeans_rule(int64_t N) {
    int64_t k = 1;
    while (k * k < N) k++;
    return k;
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
static int simulate_run(pcx_ctx* ctx, const pcx_sim* sim, pcx_sim_result* res, int restarts, const char* who) {
    if (const int rc = sim_check(sim, who, restarts > 0)) return rc;
    const bool km = restarts > 0 && sim->algorithm == PCX_ALG_KMEANS;
    const int64_t kk = km ? sim_kmeans_rule(sim->n_reporters) : 0;
    if (km)
        if (const int rc = sim_books_check(sim->n_rounds, restarts, who)) return rc;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    const int64_t B = sim->n_rounds, N = sim->n_reporters, E = sim->n_events, T = sim->n_timesteps;
    const size_t bn = (size_t)B * N, be = (size_t)B * E;
    // work buffers, doubles first: reports, lo, hi, truth, outcomes_final, old_rep, two smooth_rep
    // (ping-pong: a timestep reads one as its reputation and writes the other), metrics; then
    // the bytes scaled and liar
    const size_t n_f64 = bn * E + 4 * be + 3 * bn + (size_t)B * PCX_SIM_NMETRICS;
    // (k-means: the books [B][restarts][k] int32 behind the bytes, on a 4-byte boundary)
    const size_t off_books = (n_f64 * sizeof(double) + be + bn + 3) / 4 * 4;
    const size_t n_books = km ? (size_t)B * restarts * kk : 0;
    if (const int rc = sim_reserve(ctx, std::max<size_t>(off_books + n_books * sizeof(int32_t), 16))) return rc;
    int32_t* const w_books = reinterpret_cast<int32_t*>(static_cast<char*>(ctx->sim_buf) + off_books);
    double* p = (double*)ctx->sim_buf;
    auto take = [&p](size_t n) {
        double* q = p;
        p += n;
        return q;
    };
    pcx_sim_rounds work;
    work.reports = take(bn * E);
    work.lo = take(be);
    work.hi = take(be);
    work.truth = take(be);
    double* w_outcomes = take(be);
    double* w_old = take(bn);
    double* w_smooth[2] = {take(bn), take(bn)};
    double* w_metrics = take((size_t)B * PCX_SIM_NMETRICS);
    work.scaled = (uint8_t*)p;
    work.liar = work.scaled + be;
    const pcx::sim::Gen g = sim_gen(sim);
    const double* rep = sim->reputation0;
    for (int64_t t = 0; t < T; t++) {
        const bool last = t == T - 1;
        pcx_sim_rounds r = work;
        pcx_batch_result o{};
        if (last) {  // the caller's buffers where given
            const pcx_sim_rounds& u = res->last;
            if (u.reports) r.reports = u.reports;
            if (u.scaled) r.scaled = u.scaled;
            if (u.lo) r.lo = u.lo;
            if (u.hi) r.hi = u.hi;
            if (u.truth) r.truth = u.truth;
            if (u.liar) r.liar = u.liar;
            o = res->last_out;
        }
        if (!o.old_rep) o.old_rep = w_old;
        if (!o.smooth_rep) o.smooth_rep = w_smooth[t & 1];
        if (!o.outcomes_final) o.outcomes_final = w_outcomes;
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
            e = pcx::launch_sim_kmeans_books(g, B, (int)N, (int)kk, restarts, (uint32_t)t, w_books, ctx->stream);
            if (e != hipSuccess) return hip_fail(e, "k_kmeans_books launch");
            in.kmeans_k = (int32_t)kk;
            in.kmeans_restarts = restarts;
            in.kmeans_init = w_books;
        }
        if (const int rc = pcx_consensus_batched_f64(ctx, &in, &o)) return rc;
        if (res->metrics || res->summary) {
            double* m = res->metrics ? res->metrics + (size_t)t * B * PCX_SIM_NMETRICS : w_metrics;
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
    pcx::sim_kmeans_books_host(sim_gen(sim), sim->n_rounds, (int)sim->n_reporters, (int)sim_kmeans_rule(sim->n_reporters),
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
                                     (int)sim_kmeans_rule(sim->n_reporters), restarts, (uint32_t)timestep, books,
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
int sweep_check(const pcx_sim_sweep* s, const char* who, int64_t totals[4], int64_t counts[4], int64_t lds_bytes[4],
                int64_t* bad_cell, const pcx_round_params* cp = nullptr, bool kmeans_ok = false) {
    if (bad_cell) *bad_cell = -1;
    if (s->n_cells < 0) return sweep_fail(bad_cell, -1, who, "n_cells must be >= 0");
    if (s->n_cells > 0 && !s->cells) return sweep_fail(bad_cell, -1, who, "cells is NULL");
    if (s->n_timesteps < 1 || s->n_timesteps >= (1 << 24))
        return sweep_fail(bad_cell, -1, who, "n_timesteps must be in [1, 2^24)");
    if (!(s->scaled_tol >= 0.0) || !std::isfinite(s->scaled_tol))
        return sweep_fail(bad_cell, -1, who, "scaled_tol must be finite and >= 0");
    if (cp) {
        // (each cell's own set, below)
    } else if (s->algorithm < PCX_ALG_PCA || s->algorithm > PCX_ALG_CLUSTERFECK)
        return sweep_fail(bad_cell, -1, who, "algorithm must be an enum pcx_algorithm value (0..7)");
    else if (s->algorithm == PCX_ALG_KMEANS && !kmeans_ok)
        return sweep_fail(bad_cell, -1, who, "k-means is not simulated (its code books are drawn on the host)");
    else if (s->algorithm == PCX_ALG_COKURTOSIS)
        return sweep_fail(bad_cell, -1, who, "cokurtosis is not simulated (it needs the caller's scores)");
    else if (s->algorithm == PCX_ALG_HIERARCHICAL && std::isnan(s->hierarchy_threshold))
        return sweep_fail(bad_cell, -1, who, "hierarchy_threshold is NaN");
    // (max_components is capped at E_c per round on the device)
    else if (s->algorithm == PCX_ALG_BIG_FIVE && s->max_components < 1)
        return sweep_fail(bad_cell, -1, who, "big-five needs max_components >= 1");
    else if (s->algorithm == PCX_ALG_FIXED_VARIANCE && !std::isfinite(s->variance_threshold))
        return sweep_fail(bad_cell, -1, who, "variance_threshold must be finite");
    else if (!std::isfinite(s->catch_tolerance) || !std::isfinite(s->alpha))
        return sweep_fail(bad_cell, -1, who, "catch_tolerance/alpha must be finite");
    int64_t tot[4] = {0, 0, 0, 0}, cnt[4] = {0, 0, 0, 0};
    size_t lds[4] = {0, 0, 0, 0};
    for (int64_t c = 0; c < s->n_cells; c++) {
        const pcx_sim_cell& k = s->cells[c];
        if (k.n_reporters < 1 || k.n_reporters > 256 || k.n_events < 1 || k.n_events > 64)
            return sweep_fail(bad_cell, c, who,
                              "is " + std::to_string(k.n_reporters) + " x " + std::to_string(k.n_events) +
                                  "; a cell's rounds must be within [1, 256] x [1, 64]");
        if (k.n_rounds < 1 || k.n_rounds > 0x7fffffff)
            return sweep_fail(bad_cell, c, who, "n_rounds must be in [1, 2^31)");
        const struct {
            const char* name;
            double p;
        } probs[] = {{"liar_frac", k.liar_frac}, {"collude_frac", k.collude_frac}, {"distort", k.distort},
                     {"na_frac", k.na_frac},     {"scaled_frac", k.scaled_frac}};
        for (const auto& q : probs)
            if (!(q.p >= 0.0 && q.p <= 1.0))  // false for NaN too
                return sweep_fail(bad_cell, c, who, std::string(q.name) + " must be a probability in [0, 1]");
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

pcx::sim::Gen sweep_gen(const pcx_sim_cell& k) {
    pcx::sim::Gen g;
    g.key0 = (uint32_t)k.seed;
    g.key1 = (uint32_t)(k.seed >> 32);
    g.thr_liar = sim_threshold(k.liar_frac);
    g.thr_collude = sim_threshold(k.collude_frac);
    g.thr_distort = sim_threshold(k.distort);
    g.thr_na = sim_threshold(k.na_frac);
    g.thr_scaled = sim_threshold(k.scaled_frac);
    return g;
}

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

// The loop of pcx_simulate_sweep_f64, pcx_simulate_study_f64 and pcx_simulate_study_params_f64
// (`who`).  study NULL: the sweep.  Otherwise every timestep's metrics launch is followed by the
// detail launch, and one statistics launch follows the last timestep.  cp: per-cell parameter sets
// [C] (NULL: the sweep's shared ones) -- the consensus launches are then those of
// pcx_consensus_ragged_params_f64, round b of cell c on set c.
// restarts > 0 (pcx_simulate_study_kmeans_f64): k-means passes; the call runs on parameter sets (the
// shared parameters as every cell's set where cp is NULL), every timestep's books of the k-means
// cells' rounds are drawn into the workspace behind the generator, and the consensus launches are
// those of pcx_consensus_ragged_kmeans_f64.
static int sweep_run(pcx_ctx* ctx, const pcx_sim_sweep* sweep, pcx_sim_result* res, const int32_t* pair_base,
                     const pcx_sim_study_result* study, const char* who, const pcx_round_params* cp = nullptr,
                     int restarts = 0) {
    const std::string name(who);
    int64_t tot[4], cnt[4], lds[4];
    const bool km = restarts > 0;
    if (const int rc = sweep_check(sweep, who, tot, cnt, lds, nullptr, cp, km)) return rc;
    std::vector<pcx_round_params> own_cp;
    if (km && !cp) {
        own_cp.assign((size_t)sweep->n_cells,
                      pcx_round_params{sweep->algorithm, sweep->max_components, sweep->catch_tolerance, sweep->alpha,
                                       sweep->variance_threshold, sweep->hierarchy_threshold, sweep->cluster_threshold});
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
    for (int64_t c = 0, b = 0; c < C; c++)
        for (int64_t r = 0; r < sweep->cells[c].n_rounds; r++, b++) {
            nrep[b] = sweep->cells[c].n_reporters;
            nev[b] = sweep->cells[c].n_events;
            if (pof) pof[b] = (int32_t)c;
        }
    // work buffers, pcx_simulate_f64's layout over the flat arrays
    const size_t bn = (size_t)tot[1], be = (size_t)tot[2], bne = (size_t)tot[3];
    // (a study keeps every timestep's metrics and detail for its statistics: in the workspace, behind
    // the sweep's doubles, where the caller gives no buffer)
    const bool all_metrics = study && !res->metrics;
    const size_t n_metrics = (size_t)(all_metrics ? T : 1) * B * PCX_SIM_NMETRICS;
    const size_t n_detail = study && !study->detail ? (size_t)T * B * PCX_SIM_NDETAIL : 0;
    const size_t n_f64 = bne + 4 * be + 3 * bn + n_metrics + n_detail;
    // (k-means: the flat books of the k-means cells' rounds, int32, behind the bytes)
    int64_t n_books = 0;
    if (km)
        if (const int rc = kmeans_layout(B, nrep, nev, nullptr, restarts, cp, pof, nullptr, nullptr, nullptr, &n_books))
            return rc;
    const size_t off_books = (n_f64 * sizeof(double) + be + bn + 3) / 4 * 4;
    if (const int rc = sim_reserve(ctx, std::max<size_t>(off_books + (size_t)n_books * sizeof(int32_t), 16))) return rc;
    int32_t* const w_books = reinterpret_cast<int32_t*>(static_cast<char*>(ctx->sim_buf) + off_books);
    double* p = (double*)ctx->sim_buf;
    auto take = [&p](size_t n) {
        double* q = p;
        p += n;
        return q;
    };
    pcx_sim_rounds work;
    work.reports = take(bne);
    work.lo = take(be);
    work.hi = take(be);
    work.truth = take(be);
    double* w_outcomes = take(be);
    double* w_old = take(bn);
    double* w_smooth[2] = {take(bn), take(bn)};
    double* w_metrics = take(n_metrics);
    double* all_detail = study ? (study->detail ? study->detail : take(n_detail)) : nullptr;
    work.scaled = (uint8_t*)p;
    work.liar = work.scaled + be;
    // every table of the call in one staging slot, uploaded once: the wide ragged call's descriptors
    // (the same every timestep: only the data pointers change), then the sweep's own
    WidePlan plan;
    ParamsPlan pplan;
    const bool pairs = study && study->paired;
    const size_t off_ktab = sweep_table_bytes(sweep) + (pairs ? pair_base_bytes(sweep) : 0);  // inside `extra`
    const size_t extra = off_ktab + (km ? (size_t)B * sizeof(pcx::KmeansEntry) : 0);
    if (cp) {
        params_count(B, nrep, nev, cp, pof, &pplan);
        if (const int rc = params_tables(ctx, nrep, nev, C, cp, pof, false, extra, &pplan)) return rc;
    } else if (const int rc = wide_tables(ctx, B, nrep, nev, sweep->algorithm, false, cnt, lds, false, extra, &plan)) {
        return rc;
    }
    pcx_ctx::RaggedSlot* const slot = cp ? pplan.slot : plan.slot;
    const size_t off_x = cp ? pplan.off_x : plan.off_x, up_bytes = cp ? pplan.bytes : plan.bytes;
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
    e = ragged_slot_upload(ctx, *slot, up_bytes);
    if (e != hipSuccess) return hip_fail(e, "sweep: table upload");
    const double* rep = sweep->reputation0;
    for (int64_t t = 0; t < T; t++) {  // launches only: no host wait in this loop
        const bool last = t == T - 1;
        pcx_sim_rounds r = work;
        pcx_batch_result o{};
        if (last) {  // the caller's buffers where given
            const pcx_sim_rounds& u = res->last;
            if (u.reports) r.reports = u.reports;
            if (u.scaled) r.scaled = u.scaled;
            if (u.lo) r.lo = u.lo;
            if (u.hi) r.hi = u.hi;
            if (u.truth) r.truth = u.truth;
            if (u.liar) r.liar = u.liar;
            o = res->last_out;
        }
        if (!o.old_rep) o.old_rep = w_old;
        if (!o.smooth_rep) o.smooth_rep = w_smooth[t & 1];
        if (!o.outcomes_final) o.outcomes_final = w_outcomes;
        e = pcx::launch_sim_sweep_generate(tab, (uint32_t)t, r, ctx->stream);
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
            e = pcx::launch_sim_sweep_kmeans_books(tab, dev_ktab, restarts, (uint32_t)t, w_books, ctx->stream);
            if (e != hipSuccess) return hip_fail(e, "k_kmeans_books_sweep launch");
            a.kmeans_restarts = restarts;
            a.kmeans_init = w_books;
        }
        e = km ? kmeans_launch(ctx, pplan, a, dev_ktab) : cp ? params_launch(ctx, pplan, a) : wide_launch(ctx, plan, a);
        if (e != hipSuccess) return hip_fail(e, "sweep: ragged wide launch");
        if (res->metrics || res->summary || study) {
            double* m = res->metrics   ? res->metrics + (size_t)t * B * PCX_SIM_NMETRICS
                        : all_metrics ? w_metrics + (size_t)t * B * PCX_SIM_NMETRICS
                                      : w_metrics;
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
        e = pcx::launch_sim_study_stats(tab, T, res->metrics ? res->metrics : w_metrics, all_detail, dev_base,
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
    for (int64_t c = 0, b = 0; c < sweep->n_cells; c++)
        for (int64_t r = 0; r < sweep->cells[c].n_rounds; r++, b++) {
            shape[b] = sweep->cells[c].n_reporters;
            shape[tot[0] + b] = sweep->cells[c].n_events;
        }
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
