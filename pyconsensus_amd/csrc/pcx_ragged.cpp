// pcx_ragged.cpp -- the ragged-batch entries of include/pcx.h (rounds of different shapes in one
// call): their plan passes, the staging slots, the one plan type with its two table layouts and its
// launch walk.  Host code only; no compute happens here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/pcx.h"
#include "pcx_host.h"
#include "pcx_internal.h"

namespace pcx {
namespace host __attribute__((visibility("hidden"))) {

// ---------------------------------------------------------------- staging slots
int ragged_slot_take(pcx_ctx* ctx, size_t bytes, pcx_ctx::RaggedSlot** slot) {
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

hipError_t ragged_slot_upload(pcx_ctx* ctx, pcx_ctx::RaggedSlot& s, size_t bytes) {
    hipError_t e = hipSuccess;
    if (s.used) e = hipStreamWaitEvent(ctx->stream, s.kern_ev, 0);
    if (e == hipSuccess) e = hipMemcpyAsync(s.dev, s.pin, bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipEventRecord(s.copy_ev, ctx->stream);
    if (e == hipSuccess) s.used = true;
    return e;
}

// ---------------------------------------------------------------- the rounds of a call
// Round after round -- for (RoundWalk r(B, n_reporters, n_events); r.round(); r.step()) -- with round
// r.b's shape and where its cells, reporters and events start in the flat arrays (the descriptors'
// offsets): what the two table builders walk.  (The plan passes want no offsets and keep plain loops.)
struct RoundWalk {
    const int64_t B;
    const int32_t *n_reporters, *n_events;
    int64_t b = 0, cell = 0, row = 0, ev = 0;
    int32_t N = 0, E = 0;
    RoundWalk(int64_t B_, const int32_t* nr, const int32_t* ne) : B(B_), n_reporters(nr), n_events(ne) {}
    bool round() {
        if (b >= B) return false;
        N = n_reporters[b], E = n_events[b];
        return true;
    }
    void step() { cell += (int64_t)N * E, row += N, ev += E, b++; }
};

// a round outside [1, max_n] x [1, max_e] is refused by name (the test stays in the callers' loops)
static inline bool round_fits(int N, int E, int max_n, int max_e) { return N >= 1 && N <= max_n && E >= 1 && E <= max_e; }
static int round_refusal(int64_t b, int N, int E, int max_n, int max_e, int64_t* bad_round) {
    if (bad_round) *bad_round = b;
    return fail(PCX_EINVAL, "ragged: round " + std::to_string(b) + " is " + std::to_string(N) + " x " +
                                std::to_string(E) + "; a round must be within [1, " + std::to_string(max_n) +
                                "] x [1, " + std::to_string(max_e) + "]");
}

int wide_slot(int N, int E, int algorithm, bool one_class) {
    if (N <= 64 && E <= 32) return 0;
    return one_class ? 1 : pcx::medium_launch_class(pcx::medium_lds_bytes(N, E, algorithm));
}

// The plan pass of the shared-parameter entries: what pcx_ragged_plan_wide (WIDE) and
// pcx_ragged_plan (rounds within 64 x 32: every round in class 0, known at compile time) report.
template <bool WIDE>
static int shared_plan_pass(int64_t n_rounds, const int32_t* n_reporters, const int32_t* n_events, int algorithm,
                            bool one_class, int64_t totals[3], int64_t counts[4], int64_t lds_bytes[4],
                            int64_t* bad_round) {
    constexpr int max_n = WIDE ? 256 : 64, max_e = WIDE ? 64 : 32;
    if (bad_round) *bad_round = -1;
    if (n_rounds < 0 || n_rounds > 0x7fffffff) return fail(PCX_EINVAL, "ragged: n_rounds must be in [0, 2^31)");
    if (algorithm < PCX_ALG_PCA || algorithm > PCX_ALG_CLUSTERFECK)
        return fail(PCX_EINVAL, "ragged: algorithm must be an enum pcx_algorithm value (0..7)");
    if (algorithm == PCX_ALG_KMEANS)
        return fail(PCX_EINVAL, "ragged: k-means is not supported (its code-book size depends on each round's N)");
    if (n_rounds > 0 && (!n_reporters || !n_events)) return fail(PCX_EINVAL, "ragged: n_reporters / n_events is NULL");
    int64_t tn = 0, te = 0, tc = 0, cnt[4] = {0, 0, 0, 0};
    size_t lds[4] = {0, 0, 0, 0}, lds0 = 0;
    for (int64_t b = 0; b < n_rounds; b++) {  // (no offsets wanted: a plain loop, its sums in registers)
        const int32_t N = n_reporters[b], E = n_events[b];
        if (!round_fits(N, E, max_n, max_e)) return round_refusal(b, N, E, max_n, max_e, bad_round);
        tn += N, te += E, tc += (int64_t)N * E;
        const int k = WIDE ? wide_slot(N, E, algorithm, one_class) : 0;
        if (k) cnt[k]++, lds[k] = std::max(lds[k], pcx::medium_lds_bytes(N, E, algorithm));
        else lds0 = std::max(lds0, pcx::ragged_lds_bytes(N, E, algorithm));
    }
    cnt[0] = n_rounds - cnt[1] - cnt[2] - cnt[3], lds[0] = lds0;
    if (totals) totals[0] = tn, totals[1] = te, totals[2] = tc;
    for (int k = 0; k < 4 && counts; k++) counts[k] = cnt[k];
    for (int k = 0; k < 4 && lds_bytes; k++) lds_bytes[k] = (int64_t)lds[k];
    return PCX_OK;
}

// ---------------------------------------------------------------- the plan
// The workgroup scratch of a plan with workgroup rounds: the rounds per chunk that fit the cap
// (pcx_test_scratch_cap's where set) at the plan's slot strides, the context's scratch reserved,
// and its three parts.  0 = ok.
// The tall segment (table plans; n_tall > 0) has strides and a chunk of its own under the same cap and
// lies over the same bytes: the stream runs its launches after the workgroup segments'.
static int plan_scratch(pcx_ctx* ctx, RaggedPlan& p) {
    if (p.nm == 0 && p.n_tall == 0) return PCX_OK;
    const size_t cap = ctx->test_scratch_cap > 0 ? (size_t)ctx->test_scratch_cap : MEDIUM_SCRATCH_CAP;
    size_t per = 0, tper = 0;
    if (p.nm > 0) {
        per = (size_t)((p.filled ? 0 : p.stride[0]) + p.stride[1] + p.stride[2]) * sizeof(double);
        p.chunk = std::min<int64_t>(std::max<int64_t>((int64_t)(cap / per), 1), p.nm);
    }
    if (p.n_tall > 0) {
        tper = (size_t)((p.filled ? 0 : p.tall_stride[0]) + p.tall_stride[1]) * sizeof(double);
        p.tall_chunk = std::min<int64_t>(std::max<int64_t>((int64_t)(cap / tper), 1), p.n_tall);
    }
    if (const int rc = medium_scratch_reserve(ctx, std::max(per * (size_t)p.chunk, tper * (size_t)p.tall_chunk)))
        return rc;
    if (p.nm > 0) {
        p.Fscr = (double*)ctx->mscr;
        p.Cscr = p.Fscr + (p.filled ? 0 : (size_t)p.chunk * p.stride[0]);
        p.Xscr = p.Cscr + (size_t)p.chunk * p.stride[1];  // the clusterings' cluster sums / observations
    }
    if (p.n_tall > 0) {
        p.tall_Fscr = (double*)ctx->mscr;
        p.tall_Cscr = p.tall_Fscr + (p.filled ? 0 : (size_t)p.tall_chunk * p.tall_stride[0]);
    }
    return PCX_OK;
}

int plan_shared(pcx_ctx* ctx, int64_t B, const int32_t* n_reporters, const int32_t* n_events, int algorithm,
                bool one_class, const int64_t cnt[4], const int64_t lds[4], bool filled, size_t extra,
                bool wave_table_alone, RaggedPlan* plan) {
    RaggedPlan& p = *plan;
    p.B = B;
    p.nw = cnt[0];
    p.nm = B - p.nw;
    p.filled = filled;
    for (int k = 0; k < 4; k++) p.cnt[k] = cnt[k], p.lds[k] = lds[k];
    p.first[2] = cnt[3];  // class 3 first
    p.first[1] = cnt[3] + cnt[2];
    const int64_t nw = p.nw;
    if (wave_table_alone && p.nm == 0) {
        // pcx_consensus_ragged_f64's table: nothing is scattered, so the wave descriptors stand alone, from a
        // loop with one destination and no class test (its host time shows: profiles/ragged_host_plan).
        // (A sweep keeps the indices and the temporaries' room: its slot's size does not depend on its cells.)
        p.off_m = p.off_i = p.off_x = (size_t)B * sizeof(pcx::RaggedDesc);
        p.bytes = p.off_t = p.off_x + extra;
        if (const int rc = ragged_slot_take(ctx, p.bytes, &p.slot)) return rc;
        pcx::RaggedDesc* d = static_cast<pcx::RaggedDesc*>(p.slot->pin);
        int64_t cell = 0, row = 0, ev = 0;
        for (int64_t b = 0; b < B; b++) {
            const int32_t N = n_reporters[b], E = n_events[b];
            d[b] = pcx::RaggedDesc{cell, row, ev, N, E};
            cell += (int64_t)N * E, row += N, ev += E;
        }
        return PCX_OK;
    }
    p.off_m = (size_t)nw * sizeof(pcx::RaggedDesc);
    p.off_i = p.off_m + (size_t)p.nm * sizeof(pcx::MediumDesc);
    p.off_x = (p.off_i + (size_t)nw * sizeof(int32_t) + 7) / 8 * 8;
    p.bytes = p.off_t = p.off_x + extra;  // (the wave rounds' 32 bytes of temporaries each follow on the device)
    if (const int rc = ragged_slot_take(ctx, p.off_t + (size_t)nw * 32, &p.slot)) return rc;
    char* pin = static_cast<char*>(p.slot->pin);
    pcx::RaggedDesc* dw = reinterpret_cast<pcx::RaggedDesc*>(pin);
    pcx::MediumDesc* dm = reinterpret_cast<pcx::MediumDesc*>(pin + p.off_m);
    int32_t* idx = reinterpret_cast<int32_t*>(pin + p.off_i);
    int64_t at[4] = {0, p.first[1], p.first[2], 0}, w = 0;  // next entry of each class in dm, of dw
    for (RoundWalk r(B, n_reporters, n_events); r.round(); r.step()) {
        const int k = wide_slot(r.N, r.E, algorithm, one_class);
        if (k == 0) {
            dw[w] = pcx::RaggedDesc{r.cell, r.row, r.ev, r.N, r.E};
            idx[w++] = (int32_t)r.b;
        } else {
            dm[at[k]++] = pcx::MediumDesc{r.cell, r.row, r.ev, r.N, r.E, (int32_t)r.b, 0};
            pcx::medium_slot_strides(r.N, r.E, algorithm, p.stride);
        }
    }
    return plan_scratch(ctx, p);
}

static int table_segment(int N, int E, int algorithm) {
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
            seg = n > 256 ? PLAN_SEGMENTS : table_segment(n, e, a);  // (PLAN_SEGMENTS: the tall segment)
            lds = (int64_t)(seg == PLAN_SEGMENTS ? pcx::tall_lds_bytes(n, e, a)
                            : seg < 3            ? pcx::ragged_lds_bytes(n, e, a)
                                                 : pcx::medium_lds_bytes(n, e, a));
        }
        return seg;
    }
};

// a segment's count and dynamic LDS (the largest round's own, by its own algorithm) and the
// workgroup rounds' slot strides, of rounds that the caller has checked
static void table_count(int64_t B, const int32_t* n_reporters, const int32_t* n_events, const pcx_round_params* params,
                        const int32_t* param_of, RaggedPlan* plan) {
    RaggedPlan& p = *plan;
    p.table = true;
    p.B = B;
    SegmentOf run;
    for (int64_t b = 0; b < B; b++) {
        const int N = n_reporters[b], E = n_events[b], alg = params[param_of[b]].algorithm;
        const int s = run.at(N, E, alg);
        if (s == PLAN_SEGMENTS) {  // a tall round (an entry that takes them has checked its route)
            p.n_tall++;
            if (!run.fresh) continue;
            p.tall_lds = std::max(p.tall_lds, run.lds);
            p.tall_stride[0] = std::max<int64_t>(p.tall_stride[0], (int64_t)N * E);
            p.tall_stride[1] = std::max<int64_t>(p.tall_stride[1], (int64_t)E * E);
            continue;
        }
        p.cnt[s]++;
        if (s >= 3) p.nm++;
        if (!run.fresh) continue;
        p.lds[s] = std::max(p.lds[s], run.lds);
        if (s >= 3) pcx::medium_slot_strides(N, E, alg, p.stride);
    }
    p.nw = B - p.nm - p.n_tall;
    for (int s = 1; s < PLAN_SEGMENTS; s++) p.first[s] = p.first[s - 1] + p.cnt[s - 1];
    p.tall_first = B - p.n_tall;  // behind the nine segments
}

// the launches of a counted table plan with nothing chunked: its segments that hold a round
static int64_t plan_n_launches(const RaggedPlan& p) {
    int64_t n = p.n_tall > 0;
    for (int s = 0; s < PLAN_SEGMENTS; s++) n += p.cnt[s] > 0;
    return n;
}

// the launches of a table plan over these checked rounds
static int64_t table_n_launches(int64_t B, const int32_t* n_reporters, const int32_t* n_events,
                                const pcx_round_params* params, const int32_t* param_of) {
    RaggedPlan p;
    table_count(B, n_reporters, n_events, params, param_of, &p);
    return plan_n_launches(p);
}

int plan_table(pcx_ctx* ctx, int64_t B, const int32_t* n_reporters, const int32_t* n_events, int64_t n_params,
               const pcx_round_params* params, const int32_t* param_of, bool filled, size_t extra, RaggedPlan* plan) {
    RaggedPlan& p = *plan;
    table_count(B, n_reporters, n_events, params, param_of, plan);
    p.filled = filled;
    p.off_p = (size_t)B * sizeof(pcx::MediumDesc);
    p.off_x = p.off_p + (size_t)n_params * sizeof(pcx::RoundParams);
    p.bytes = p.off_x + extra;
    if (const int rc = ragged_slot_take(ctx, p.bytes, &p.slot)) return rc;
    char* pin = static_cast<char*>(p.slot->pin);
    pcx::MediumDesc* d = reinterpret_cast<pcx::MediumDesc*>(pin);
    int64_t at[PLAN_SEGMENTS + 1];
    for (int s = 0; s < PLAN_SEGMENTS; s++) at[s] = p.first[s];
    at[PLAN_SEGMENTS] = p.tall_first;
    SegmentOf run;
    for (RoundWalk r(B, n_reporters, n_events); r.round(); r.step()) {
        const int s = run.at(r.N, r.E, params[param_of[r.b]].algorithm);
        d[at[s]++] = pcx::MediumDesc{r.cell, r.row, r.ev, r.N, r.E, (int32_t)r.b, param_of[r.b]};
    }
    std::memcpy(pin + p.off_p, params, (size_t)n_params * sizeof(pcx::RoundParams));
    return plan_scratch(ctx, p);
}

hipError_t RaggedPlan::launch(pcx_ctx* ctx, const pcx::BatchArgs& a, const pcx::KmeansEntry* books) const {
    char* dev = static_cast<char*>(slot->dev);
    hipStream_t st = ctx->stream;
    hipError_t e = hipSuccess;
    if (table) {  // (a's parameter fields are not read)
        const pcx::MediumDesc* d = reinterpret_cast<const pcx::MediumDesc*>(dev);
        const pcx::RoundParams* tab = reinterpret_cast<const pcx::RoundParams*>(dev + off_p);
        for (int g = 0; g < 3 && e == hipSuccess; g++)
            e = g == 2 && books ? pcx::launch_ragged_kmeans(a, d + first[g], tab, books, cnt[g], (size_t)lds[g], st)
                                : pcx::launch_ragged_params(a, d + first[g], tab, cnt[g], g, (size_t)lds[g], st);
        for (int s = 3; s < PLAN_SEGMENTS && e == hipSuccess; s++)
            for (int64_t b0 = 0; b0 < cnt[s] && e == hipSuccess; b0 += chunk) {
                const int64_t nb = std::min<int64_t>(chunk, cnt[s] - b0);
                e = s >= 6 && books ? pcx::launch_ragged_medium_kmeans(a, d + first[s] + b0, tab, books, nb, (size_t)lds[s],
                                                                       stride, Fscr, Cscr, Xscr, st)
                                    : pcx::launch_ragged_medium_params(a, d + first[s] + b0, tab, nb, s >= 6, (size_t)lds[s],
                                                                       stride, Fscr, Cscr, Xscr, st);
            }
        for (int64_t b0 = 0; b0 < n_tall && e == hipSuccess; b0 += tall_chunk)  // the tall segment
            e = pcx::launch_ragged_tall_params(a, d + tall_first + b0, tab, std::min<int64_t>(tall_chunk, n_tall - b0),
                                               (size_t)tall_lds, tall_stride, tall_Fscr, tall_Cscr, st);
        return e;
    }
    const pcx::RaggedDesc* dw = reinterpret_cast<const pcx::RaggedDesc*>(dev);
    if (nm == 0) return pcx::launch_ragged(a, dw, (size_t)lds[0], st);
    if (nw > 0) {
        pcx::BatchArgs aw = a;
        aw.B = nw;
        const pcx::WaveTmp t = pcx::ragged_wave_tmp(dev + off_t, nw);
        aw.participation = t.participation;
        aw.avg_certainty = t.avg_certainty;
        aw.branch = t.branch;
        aw.flags = t.flags;
        aw.pi_iters = t.pi_iters;
        aw.components = t.components;
        e = pcx::launch_ragged(aw, dw, (size_t)lds[0], st);
        if (e == hipSuccess)
            e = pcx::launch_ragged_scatter(a, reinterpret_cast<const int32_t*>(dev + off_i), nw, dev + off_t, st);
    }
    const pcx::MediumDesc* dm = reinterpret_cast<const pcx::MediumDesc*>(dev + off_m);
    for (int k = 3; k >= 1 && e == hipSuccess; k--)
        for (int64_t b0 = 0; b0 < cnt[k] && e == hipSuccess; b0 += chunk)
            e = pcx::launch_ragged_medium(a, dm + first[k] + b0, std::min<int64_t>(chunk, cnt[k] - b0), (size_t)lds[k],
                                          stride, Fscr, Cscr, Xscr, st);
    return e;
}

// pcx_consensus_ragged_f64 and pcx_consensus_ragged_wide_f64 past their plan pass, which found
// cnt / lds per launch class
static int shared_entry(pcx_ctx* ctx, const pcx_ragged* in, pcx_batch_result* out, bool one_class,
                        const int64_t cnt[4], const int64_t lds[4]) {
    if (in->n_rounds == 0) return PCX_OK;
    // (max_components is capped at E_b per round on the device)
    const bool bad_five = in->algorithm == PCX_ALG_BIG_FIVE && in->max_components < 1;
    if (const int rc = check_options("ragged", in, bad_five ? "big-five needs max_components >= 1" : nullptr))
        return rc;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    RaggedPlan p;
    if (const int rc = plan_shared(ctx, in->n_rounds, in->n_reporters, in->n_events, in->algorithm, one_class, cnt, lds,
                                   out->filled != nullptr, 0, true, &p))
        return rc;
    e = ragged_slot_upload(ctx, *p.slot, p.bytes);
    if (e != hipSuccess) return hip_fail(e, "ragged: descriptor upload");
    pcx::BatchArgs a = shared_args(in, out);
    a.B = in->n_rounds;
    e = p.launch(ctx, a);
    if (e == hipSuccess) e = hipEventRecord(p.slot->kern_ev, ctx->stream);
    return e == hipSuccess ? PCX_OK : hip_fail(e, p.nm ? "ragged wide launch" : "ragged_round_kernel launch");
}

// ---------------------------------------------------------------- per-round parameters
static_assert(sizeof(pcx_round_params) == sizeof(pcx::RoundParams), "pcx_round_params is the device entry");

const char* params_set_refusal(const pcx_round_params& q, bool sim, bool kmeans_ok) {
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

// a round whose set is none of the call's is refused by name
static int param_of_refusal(int64_t b, int32_t of, int64_t n_params, int64_t* bad_round) {
    if (bad_round) *bad_round = b;
    return fail(PCX_EINVAL, "ragged: round " + std::to_string(b) + " has param_of " + std::to_string(of) +
                                ", outside [0, " + std::to_string(n_params) + ")");
}

std::string tall_round_refusal(int N, int E, int algorithm) {
    if (pcx_tall_route(N, E, algorithm, 1) == PCX_ROUTE_TALL) return std::string();
    static const char* const names[] = {"PCA",        "absolute", "big-five",     "fixed-variance",
                                        "cokurtosis", "k-means",  "hierarchical", "clusterfeck"};
    const std::string shape = std::to_string(N) + " x " + std::to_string(E);
    if (algorithm >= PCX_ALG_KMEANS)
        return shape + " under " + names[algorithm] + "; the clusterings stay within 256 reporters";
    return shape + " under " + names[algorithm] +
           "; the round's LDS plan does not fit a workgroup (pcx_tall_route, pcx_tall_plan)";
}

// tall: the entries that take rounds up to 1024 reporters -- [1, 1024] x [1, 64], and a round above
// 256 reporters must be of the tall route under its set's algorithm
static int params_plan_check(int64_t n_rounds, const int32_t* n_reporters, const int32_t* n_events, int64_t n_params,
                             const pcx_round_params* params, const int32_t* param_of, int64_t totals[3],
                             int64_t* bad_round, int64_t* bad_param, bool kmeans_ok = false, bool tall = false) {
    const int max_n = tall ? 1024 : 256;
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
        if (!round_fits(N, E, max_n, 64)) return round_refusal(b, N, E, max_n, 64, bad_round);
        if (param_of[b] < 0 || param_of[b] >= n_params) return param_of_refusal(b, param_of[b], n_params, bad_round);
        if (N > 256) {
            const std::string why = tall_round_refusal(N, E, params[param_of[b]].algorithm);
            if (!why.empty()) {
                if (bad_round) *bad_round = b;
                return fail(PCX_EINVAL, "ragged: round " + std::to_string(b) + " is " + why);
            }
        }
        tot[0] += N, tot[1] += E, tot[2] += (int64_t)N * E;
    }
    for (int k = 0; k < 3 && totals; k++) totals[k] = tot[k];
    return PCX_OK;
}

// ---------------------------------------------------------------- k-means in ragged batches
int64_t kmeans_rule(int64_t N) {
    int64_t k = 1;
    while (k * k < N) k++;
    return k;
}

int kmeans_layout(int64_t B, const int32_t* n_reporters, const int32_t* n_events, const int32_t* k, int restarts,
                  const pcx_round_params* params, const int32_t* param_of, int64_t* offsets,
                  pcx::KmeansEntry* entries, int64_t* bad_round, int64_t* total) {
    int64_t at = 0;
    for (int64_t b = 0; b < B; b++) {
        if (offsets) offsets[b] = at;
        if (entries) entries[b] = pcx::KmeansEntry{0, 0, 0};
        if (params && params[param_of[b]].algorithm != PCX_ALG_KMEANS) continue;
        const int N = n_reporters[b], E = n_events[b];
        const int kmax = std::min(N, N <= 64 && E <= 32 ? 8 : 16);
        const int kb = k ? k[b] : (int)kmeans_rule(N);
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

// pcx_ragged_plan_kmeans' checks; *any = some round's set is k-means
static int kmeans_plan_check(int64_t n_rounds, const int32_t* n_reporters, const int32_t* n_events, int64_t n_params,
                             const pcx_round_params* params, const int32_t* param_of, const pcx_kmeans_books* books,
                             int64_t totals[3], int64_t* offsets, int64_t* bad_round, int64_t* bad_param, bool* any) {
    if (const int rc = params_plan_check(n_rounds, n_reporters, n_events, n_params, params, param_of, totals, bad_round,
                                         bad_param, true))
        return rc;
    bool some = false;
    for (int64_t b = 0; b < n_rounds && !some; b++) some = params[param_of[b]].algorithm == PCX_ALG_KMEANS;
    if (any) *any = some;
    if (some && !books) return fail(PCX_EINVAL, "k-means: a round's set is k-means and books is NULL");
    if (some && books->restarts < 1) return fail(PCX_EINVAL, "k-means: restarts must be >= 1");
    return kmeans_layout(n_rounds, n_reporters, n_events, some ? books->k : nullptr, some ? books->restarts : 0, params,
                         param_of, offsets, nullptr, bad_round);
}

// pcx_consensus_ragged_params_f64 and pcx_consensus_ragged_kmeans_f64 past their plan checks, with
// rounds.  with_books: the latter, whose clustering launches read a per-round book table (it rides
// behind the parameter entries in the one upload); any: some round's set is k-means.  `what` names
// the launches in a HIP failure.
static int table_entry(pcx_ctx* ctx, const pcx_ragged* in, int64_t n_params, const pcx_round_params* params,
                       const int32_t* param_of, const pcx_kmeans_books* books, bool with_books, bool any,
                       pcx_batch_result* out, const char* what) {
    const int64_t B = in->n_rounds;
    if (!in->reports) return fail(PCX_EINVAL, "ragged: reports is NULL");
    if (in->scaled && (!in->lo || !in->hi)) return fail(PCX_EINVAL, "ragged: scaled given without lo/hi");
    if (any && !books->init) return fail(PCX_EINVAL, "k-means: books->init is NULL");
    for (int64_t b = 0; b < B && !in->aux_scores; b++)
        if (params[param_of[b]].algorithm == PCX_ALG_COKURTOSIS)
            return fail(PCX_EINVAL, "ragged: parameter set " + std::to_string(param_of[b]) +
                                        ": cokurtosis needs aux_scores (aux[\"cokurt\"])");
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    RaggedPlan p;
    if (const int rc = plan_table(ctx, B, in->n_reporters, in->n_events, n_params, params, param_of,
                                  out->filled != nullptr, with_books ? (size_t)B * sizeof(pcx::KmeansEntry) : 0, &p))
        return rc;
    const pcx::KmeansEntry* dev_books = nullptr;
    if (with_books) {
        pcx::KmeansEntry* entries = reinterpret_cast<pcx::KmeansEntry*>(static_cast<char*>(p.slot->pin) + p.off_x);
        if (const int rc = kmeans_layout(B, in->n_reporters, in->n_events, any ? books->k : nullptr,
                                         any ? books->restarts : 0, params, param_of, nullptr, entries, nullptr))
            return rc;
        dev_books = reinterpret_cast<const pcx::KmeansEntry*>(static_cast<char*>(p.slot->dev) + p.off_x);
    }
    e = ragged_slot_upload(ctx, *p.slot, p.bytes);
    if (e != hipSuccess) return hip_fail(e, "ragged: descriptor upload");
    pcx::BatchArgs a = shared_args(in, out);
    a.B = B;
    a.kmeans_restarts = any ? books->restarts : 0;
    a.kmeans_init = any ? books->init : nullptr;
    e = p.launch(ctx, a, dev_books);
    if (e == hipSuccess) e = hipEventRecord(p.slot->kern_ev, ctx->stream);
    return e == hipSuccess ? PCX_OK : hip_fail(e, what);
}

}  // namespace host
}  // namespace pcx
using namespace pcx::host;

// ---------------------------------------------------------------- the entries (include/pcx.h)
int pcx_ragged_plan(int64_t n_rounds, const int32_t* n_reporters, const int32_t* n_events, int algorithm,
                    int64_t totals[3], int64_t* lds_bytes, int64_t* bad_round) {
    int64_t lds[4];
    if (const int rc = shared_plan_pass<false>(n_rounds, n_reporters, n_events, algorithm, false, totals, nullptr, lds,
                                               bad_round))
        return rc;
    if (lds_bytes) *lds_bytes = lds[0];
    return PCX_OK;
}

int pcx_ragged_plan_wide(int64_t n_rounds, const int32_t* n_reporters, const int32_t* n_events, int algorithm,
                         int64_t totals[3], int64_t counts[4], int64_t lds_bytes[4], int64_t* bad_round) {
    return shared_plan_pass<true>(n_rounds, n_reporters, n_events, algorithm, false, totals, counts, lds_bytes, bad_round);
}

int pcx_consensus_ragged_f64(pcx_ctx* ctx, const pcx_ragged* in, pcx_batch_result* out) {
    if (!ctx || !in || !out) return fail(PCX_EINVAL, "pcx_consensus_ragged_f64: null argument");
    int64_t cnt[4], lds[4];
    if (const int rc = shared_plan_pass<false>(in->n_rounds, in->n_reporters, in->n_events, in->algorithm, false, nullptr,
                                               cnt, lds, nullptr))
        return rc;
    return shared_entry(ctx, in, out, false, cnt, lds);
}

int pcx_consensus_ragged_wide_f64(pcx_ctx* ctx, const pcx_ragged* in, pcx_batch_result* out) {
    if (!ctx || !in || !out) return fail(PCX_EINVAL, "pcx_consensus_ragged_wide_f64: null argument");
    const char* env = getenv("PCX_RAGGED_ONE_CLASS");  // diagnostic: every workgroup round in one launch
    const bool one_class = env && env[0] == '1';
    int64_t cnt[4], lds[4];
    if (const int rc = shared_plan_pass<true>(in->n_rounds, in->n_reporters, in->n_events, in->algorithm, one_class,
                                              nullptr, cnt, lds, nullptr))
        return rc;
    return shared_entry(ctx, in, out, one_class, cnt, lds);
}

int pcx_test_scratch_cap(pcx_ctx* ctx, int64_t bytes) {
    if (!ctx || bytes < 0) return fail(PCX_EINVAL, "pcx_test_scratch_cap: null context or negative bytes");
    ctx->test_scratch_cap = bytes;
    return PCX_OK;
}

int pcx_ragged_plan_params(int64_t n_rounds, const int32_t* n_reporters, const int32_t* n_events, int64_t n_params,
                           const pcx_round_params* params, const int32_t* param_of, int64_t totals[3],
                           int64_t* n_launches, int64_t* bad_round, int64_t* bad_param) {
    if (const int rc = params_plan_check(n_rounds, n_reporters, n_events, n_params, params, param_of, totals, bad_round,
                                         bad_param))
        return rc;
    if (n_launches) *n_launches = table_n_launches(n_rounds, n_reporters, n_events, params, param_of);
    return PCX_OK;
}

int pcx_consensus_ragged_params_f64(pcx_ctx* ctx, const pcx_ragged* in, int64_t n_params,
                                    const pcx_round_params* params, const int32_t* param_of, pcx_batch_result* out) {
    if (!ctx || !in || !out) return fail(PCX_EINVAL, "pcx_consensus_ragged_params_f64: null argument");
    if (const int rc = params_plan_check(in->n_rounds, in->n_reporters, in->n_events, n_params, params, param_of,
                                         nullptr, nullptr, nullptr))
        return rc;
    if (in->n_rounds == 0) return PCX_OK;
    return table_entry(ctx, in, n_params, params, param_of, nullptr, false, false, out, "ragged params launch");
}

int pcx_ragged_plan_tall(int64_t n_rounds, const int32_t* n_reporters, const int32_t* n_events, int64_t n_params,
                         const pcx_round_params* params, const int32_t* param_of, int64_t totals[3],
                         int64_t* n_launches, int64_t* bad_round, int64_t* bad_param, int64_t* n_tall,
                         int64_t* tall_lds_bytes) {
    if (const int rc = params_plan_check(n_rounds, n_reporters, n_events, n_params, params, param_of, totals, bad_round,
                                         bad_param, false, true))
        return rc;
    RaggedPlan p;
    table_count(n_rounds, n_reporters, n_events, params, param_of, &p);
    if (n_launches) *n_launches = plan_n_launches(p);
    if (n_tall) *n_tall = p.n_tall;
    if (tall_lds_bytes) *tall_lds_bytes = p.tall_lds;
    return PCX_OK;
}

int pcx_consensus_ragged_tall_f64(pcx_ctx* ctx, const pcx_ragged* in, int64_t n_params,
                                  const pcx_round_params* params, const int32_t* param_of, pcx_batch_result* out) {
    if (!ctx || !in || !out) return fail(PCX_EINVAL, "pcx_consensus_ragged_tall_f64: null argument");
    if (const int rc = params_plan_check(in->n_rounds, in->n_reporters, in->n_events, n_params, params, param_of,
                                         nullptr, nullptr, nullptr, false, true))
        return rc;
    if (in->n_rounds == 0) return PCX_OK;
    return table_entry(ctx, in, n_params, params, param_of, nullptr, false, false, out, "ragged tall launch");
}

int pcx_kmeans_plan(int64_t n_rounds, const int32_t* n_reporters, const int32_t* n_events, const int32_t* k,
                    int32_t restarts, int64_t* offsets, int64_t* bad_round) {
    if (bad_round) *bad_round = -1;
    if (n_rounds < 0 || n_rounds > 0x7fffffff) return fail(PCX_EINVAL, "k-means: n_rounds must be in [0, 2^31)");
    if (restarts < 1) return fail(PCX_EINVAL, "k-means: restarts must be >= 1");
    if (n_rounds > 0 && (!n_reporters || !n_events)) return fail(PCX_EINVAL, "k-means: n_reporters / n_events is NULL");
    for (int64_t b = 0; b < n_rounds; b++)
        if (!round_fits(n_reporters[b], n_events[b], 256, 64))
            return round_refusal(b, n_reporters[b], n_events[b], 256, 64, bad_round);
    return kmeans_layout(n_rounds, n_reporters, n_events, k, restarts, nullptr, nullptr, offsets, nullptr, bad_round);
}

int pcx_ragged_plan_kmeans(int64_t n_rounds, const int32_t* n_reporters, const int32_t* n_events, int64_t n_params,
                           const pcx_round_params* params, const int32_t* param_of, const pcx_kmeans_books* books,
                           int64_t totals[3], int64_t* n_launches, int64_t* offsets, int64_t* bad_round,
                           int64_t* bad_param) {
    if (const int rc = kmeans_plan_check(n_rounds, n_reporters, n_events, n_params, params, param_of, books, totals,
                                         offsets, bad_round, bad_param, nullptr))
        return rc;
    if (n_launches) *n_launches = table_n_launches(n_rounds, n_reporters, n_events, params, param_of);
    return PCX_OK;
}

int pcx_consensus_ragged_kmeans_f64(pcx_ctx* ctx, const pcx_ragged* in, int64_t n_params,
                                    const pcx_round_params* params, const int32_t* param_of,
                                    const pcx_kmeans_books* books, pcx_batch_result* out) {
    if (!ctx || !in || !out) return fail(PCX_EINVAL, "pcx_consensus_ragged_kmeans_f64: null argument");
    bool any = false;
    // (the checks first, without a table: a refusal takes no staging slot)
    if (const int rc = kmeans_plan_check(in->n_rounds, in->n_reporters, in->n_events, n_params, params, param_of, books,
                                         nullptr, nullptr, nullptr, nullptr, &any))
        return rc;
    if (in->n_rounds == 0) return PCX_OK;
    return table_entry(ctx, in, n_params, params, param_of, books, true, any, out, "ragged k-means launch");
}
