// pcx_api.cpp -- the extern "C" boundary of libpcx (declared in include/pcx.h): contexts, streams and
// communicators, the single-matrix entries, pcx_consensus_batched_f64, profiling and the self-test
// shims.  The ragged entries are in pcx_ragged.cpp, the simulator's in pcx_simulate.cpp; what the
// three share is in pcx_host.h.  Host-side validation and kernel launches; no compute happens here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../include/pcx.h"
#include "pcx_host.h"
#include "pcx_internal.h"
#include "pcx_seqsum.h"
#include "pcx_sync.h"

namespace pcx {
namespace host __attribute__((visibility("hidden"))) {
thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

int hip_fail(hipError_t e, const char* what) {
    return fail(PCX_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}

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

// the context's workgroup scratch (pcx_ctx.mscr) grown to `need` bytes; 0 = ok
int medium_scratch_reserve(pcx_ctx* ctx, size_t need) {
    if (ctx->mscr_bytes >= need) return PCX_OK;
    if (ctx->mscr) (void)hipFree(ctx->mscr);
    ctx->mscr = nullptr;
    ctx->mscr_bytes = 0;
    const hipError_t e = hipMalloc(&ctx->mscr, need);
    if (e != hipSuccess) return hip_fail(e, "hipMalloc(medium scratch)");
    ctx->mscr_bytes = need;
    return PCX_OK;
}
}  // namespace host
}  // namespace pcx
using namespace pcx::host;

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

// batched_route with the tall route: tall where the scheduler would run a round of 257..1024
// reporters that the tall kernel's LDS plan fits (pcx_tall_route and the tall entry itself)
static int tall_route(int64_t N, int64_t E, int alg, int k) {
    const int r = batched_route(N, E, alg, k);
    if (r != PCX_ROUTE_SCHEDULER || N <= 256 || N > 1024 || E > 64) return r;
    return pcx::tall_lds_bytes((int)N, (int)E, alg) ? PCX_ROUTE_TALL : r;
}

int pcx_tall_route(int n_reporters, int n_events, int algorithm, int kmeans_k) {
    return tall_route(n_reporters, n_events, algorithm, kmeans_k);
}

int64_t pcx_tall_lds_bytes(int n_reporters, int n_events, int algorithm) {
    if (tall_route(n_reporters, n_events, algorithm, 1) != PCX_ROUTE_TALL) return 0;
    return (int64_t)pcx::tall_lds_bytes(n_reporters, n_events, algorithm);
}

int pcx_tall_plan(int n_reporters, int n_events, int algorithm, int32_t out[4]) {
    if (!out) return fail(PCX_EINVAL, "pcx_tall_plan: null argument");
    out[0] = out[1] = out[2] = out[3] = 0;
    if (tall_route(n_reporters, n_events, algorithm, 1) != PCX_ROUTE_TALL)
        return fail(PCX_EINVAL, "pcx_tall_plan: not a shape and algorithm of the tall route");
    pcx::tall_plan_query(n_reporters, n_events, algorithm, out);
    return PCX_OK;
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
    double grep = 0, gtot = 0;  // 26, 27: binary guesses from the exact replay / rounds that ran the replay
    for (int64_t b = 0; b < B; b++) {
        grep += (double)h[b * 32 + 26];
        gtot += (double)h[b * 32 + 27];
    }
    fprintf(stderr, " interp_screened:%.4f interp_sorted:%.4f", iscr / (double)B, isort / (double)B);
    fprintf(stderr, " guess_replayed:%.4f replay_rounds:%.4f\n", grep / (double)B, gtot / (double)B);
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

static int run_workgroup_route(pcx_ctx* ctx, pcx::BatchArgs& a, bool tall = false) {
    const int64_t chunk = pcx::medium_chunk(a, MEDIUM_SCRATCH_CAP);
    if (const int rc = medium_scratch_reserve(ctx, pcx::medium_scratch_per_round(a) * (size_t)chunk)) return rc;
    hipError_t e = hipSuccess;
    double* Fscr = (double*)ctx->mscr;
    double* Cscr = Fscr + (a.filled ? 0 : (size_t)chunk * a.N * a.E);
    double* Xscr = Cscr + (size_t)chunk * a.E * a.E;  // the clusterings' cluster sums / observations
    stamps_begin(a, ctx->stream);
    for (int64_t b0 = 0; b0 < a.B && e == hipSuccess; b0 += chunk)
        e = tall ? pcx::launch_tall(a, b0, std::min<int64_t>(chunk, a.B - b0), Fscr, Cscr, ctx->stream)
                 : pcx::launch_medium(a, b0, std::min<int64_t>(chunk, a.B - b0), Fscr, Cscr, Xscr, ctx->stream);
    if (a.stamps) print_medium_stamps(stamps_end(a, ctx->stream), a.B);
    return e == hipSuccess ? PCX_OK : hip_fail(e, tall ? "tall_round_kernel launch" : "medium_round_kernel launch");
}

// pcx_consensus_batched_f64, and with `tall` pcx_consensus_batched_tall_f64: the same checks and
// routes, the tall route's shapes on tall_round_kernel instead of the scheduler
static int consensus_batched(pcx_ctx* ctx, const pcx_batch* in, pcx_batch_result* out, bool tall) {
    if (!ctx || !in || !out)
        return fail(PCX_EINVAL, tall ? "pcx_consensus_batched_tall_f64: null argument"
                                     : "pcx_consensus_batched_f64: null argument");
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
    if (tall && tall_route(in->n_reporters, in->n_events, in->algorithm, in->kmeans_k) == PCX_ROUTE_TALL)
        return run_workgroup_route(ctx, a, true);
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

int pcx_consensus_batched_f64(pcx_ctx* ctx, const pcx_batch* in, pcx_batch_result* out) {
    return consensus_batched(ctx, in, out, false);
}

int pcx_consensus_batched_tall_f64(pcx_ctx* ctx, const pcx_batch* in, pcx_batch_result* out) {
    return consensus_batched(ctx, in, out, true);
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

}  // extern "C"
