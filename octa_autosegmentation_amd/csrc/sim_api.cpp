// sim_api.cpp -- the public octa_sim_* entry points of include/octa_hip.h (round 3): csrc/sim.hip is compiled twice, once for the
// 3 x 3 mm^2 configurations (tables in LDS, 16-bit indices, two samples per CU: octa_simS_ops) and once with OCTA_SIM_LARGE for wide
// fields of view such as the reference's 12 x 12 mm^2 notebook run (32-bit indices, 64-bit kd elements, table area in HBM:
// octa_simL_ops). A simulator is bound to one build's operations table (csrc/sim_ops.h) when it is created; every other call
// forwards through it.
//
// Choice at octa_sim_create: the large build when the configuration can outgrow the default capacities (14 336 nodes per forest,
// 13 312 live sinks): more than 8192 / 3 candidates per iteration on a field wider than 6 mm (param_scale > 6), and more than 40
// iterations; OCTA_SIM_BUILD=large / default overrides (tests run the short optic-nerve fixtures through BOTH).
#include <cstdlib>
#include <cstring>
#include <new>

#include "sim_ops.h"

// Persistent-kernel launches of this process so far, both builds (round 5). A generator that has just finished its own launch waits for the
// NEXT launch to be on the GPU before it enqueues its rasterisation (pipeline.py): the render workgroups (145 KB of LDS: a CU to themselves)
// and the next launch's 512 simulator workgroups otherwise race for the CUs the finished launch has just left -- when the rasteriser wins,
// the whole rasterisation (45 ms per 512 triples) runs before the launch can place its workgroups: one launch in three measured 462
// instead of 410 ms.
//
// Round 6: the order is kept ON THE DEVICE. Every launch takes a ticket (octa_sim_next_ticket) and its workgroups sign in on a small block
// of device memory (octa_sim_launch_flag: [0] = highest ticket whose first workgroup has started, [1 + t % 2] = workgroups of ticket t that
// have started, [3 + t % 2] = its grid size); a rasterisation that must come behind launch t is preceded, on its own stream, by a one-wave
// gate kernel that leaves when launch t is resident (csrc/order.hip: octa_order_wait_launch). Round 5 polled octa_sim_launch_count from
// Python and slept "to give the dispatcher time": two of two driver-command runs of that build sat in its slow mode.
#include <atomic>
#include <mutex>
static std::atomic<long long> g_sim_launches{0};
extern "C" long long octa_sim_next_ticket(void) { return g_sim_launches.fetch_add(1, std::memory_order_acq_rel) + 1; }
extern "C" long long octa_sim_launch_count(void) { return g_sim_launches.load(std::memory_order_acquire); }
extern "C" int *octa_sim_launch_flag(int device) {
    static std::mutex m;
    static int *flags[64] = {};
    if (device < 0 || device >= 64) return nullptr;
    std::lock_guard<std::mutex> g(m);
    if (!flags[device]) {
        int prev = 0;
        if (hipGetDevice(&prev) != hipSuccess || hipSetDevice(device) != hipSuccess) return nullptr;
        int *p = nullptr;
        if (hipMalloc(&p, 64) != hipSuccess || hipMemset(p, 0, 64) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { (void)hipSetDevice(prev); return nullptr; }
        (void)hipSetDevice(prev);
        flags[device] = p;
    }
    return flags[device];
}

struct octa_sim {
    const octa_sim_ops *ops = nullptr;      // the build this simulator is bound to
    void *impl = nullptr;
    bool large = false;
};

static bool wants_large(const octa_sim_config *c) {
    if (const char *e = getenv("OCTA_SIM_BUILD")) {
        if (!strcmp(e, "large")) return true;
        if (!strcmp(e, "default")) return false;
    }
    if (c->param_scale <= 6.0) return false;
    int iters = 0, nmax = 0;
    for (int m = 0; m < c->n_modes && m < 8; m++) {
        const int I = (int)c->modes[m][0], N = (int)c->modes[m][1];
        if (I > 0) { iters += I; nmax = N > nmax ? N : nmax; }
    }
    return nmax > 8192 / 3 && iters > 40;       // a short run on a wide field (the nerve fixtures: 12 + 6 and 20 iterations) fits the default build
}

extern "C" int octa_sim_create_ex(octa_ctx *ctx, const octa_sim_config *cfg, int B, int build, octa_sim **out) {
    if (!out || !cfg || build < 0 || build > 2) { octa::set_error("octa_sim_create: bad arguments"); return -2; }
    *out = nullptr;
    octa_sim *sim = new (std::nothrow) octa_sim();
    if (!sim) { octa::set_error("octa_sim_create: out of host memory"); return -1; }
    sim->large = build == 0 ? wants_large(cfg) : build == 2;
    sim->ops = sim->large ? &octa_simL_ops : &octa_simS_ops;
    const int rc = sim->ops->create(ctx, cfg, B, &sim->impl);
    if (rc) { delete sim; return rc; }
    *out = sim;
    return 0;
}
extern "C" int octa_sim_create(octa_ctx *ctx, const octa_sim_config *cfg, int B, octa_sim **out) { return octa_sim_create_ex(ctx, cfg, B, 0, out); }
extern "C" void octa_sim_destroy(octa_sim *sim) {
    if (!sim) return;
    sim->ops->destroy(sim->impl);
    delete sim;
}
#define NEED(sim, what) if (!(sim)) { octa::set_error(what ": null simulator"); return -2; }
extern "C" int octa_sim_run(octa_sim *sim, const uint32_t *a, const uint64_t *b, octa_bif_fn f, void *u, void *st) { NEED(sim, "octa_sim_run") return sim->ops->run(sim->impl, a, b, f, u, st); }
extern "C" int octa_sim_run_states(octa_sim *sim, const double *fz, const double *stp, const uint32_t *a, const uint32_t *b, octa_bif_fn f, void *u, void *st) {
    NEED(sim, "octa_sim_run_states") return sim->ops->run_states(sim->impl, fz, stp, a, b, f, u, st);
}
extern "C" int octa_sim_np_state(octa_sim *sim, int k, uint32_t *o) { NEED(sim, "octa_sim_np_state") return sim->ops->np_state(sim->impl, k, o); }
extern "C" int octa_sim_edge_offsets(octa_sim *sim, int64_t *a, int64_t *b) { NEED(sim, "octa_sim_edge_offsets") return sim->ops->edge_offsets(sim->impl, a, b); }
extern "C" int octa_sim_export_edges(octa_sim *sim, double *e) { NEED(sim, "octa_sim_export_edges") return sim->ops->export_edges(sim->impl, e); }
extern "C" int octa_sim_export_edges_device(octa_sim *sim, double *e, void *st) { NEED(sim, "octa_sim_export_edges_device") return sim->ops->export_edges_device(sim->impl, e, st); }
extern "C" int octa_sim_trace(octa_sim *sim, int32_t *t) { NEED(sim, "octa_sim_trace") return sim->ops->trace(sim->impl, t); }
extern "C" int octa_sim_stats(octa_sim *sim, int64_t *t) { NEED(sim, "octa_sim_stats") return sim->ops->stats(sim->impl, t); }
extern "C" int octa_sim_kd_paths(octa_sim *sim, int64_t *t) { NEED(sim, "octa_sim_kd_paths") return sim->ops->kd_paths(sim->impl, t); }
extern "C" int octa_sim_assign_paths(octa_sim *sim, int64_t *t) { NEED(sim, "octa_sim_assign_paths") return sim->ops->assign_paths(sim->impl, t); }
extern "C" int octa_sim_spans(octa_sim *sim, int64_t *t) { NEED(sim, "octa_sim_spans") return sim->ops->spans(sim->impl, t); }
extern "C" int octa_sim_timing(octa_sim *sim, double *t) { NEED(sim, "octa_sim_timing") return sim->ops->timing(sim->impl, t); }
extern "C" int octa_sim_service_stats(octa_sim *sim, double *t) { NEED(sim, "octa_sim_service_stats") return sim->ops->service_stats(sim->impl, t); }
extern "C" int octa_sim_fields(octa_sim *sim, int k, double *o, int64_t co, int64_t *no, double *c, int64_t cc, int64_t *nc) {
    NEED(sim, "octa_sim_fields") return sim->ops->fields(sim->impl, k, o, co, no, c, cc, nc);
}
/* Simulator-independent calls go to the default build's table. h_out4 as documented; a fifth query -- which build a configuration gets -- is
 * octa_sim_is_large below. */
extern "C" int octa_sim_geometry(int num_cus, int *h_out4) { return octa_simS_ops.geometry(num_cus, h_out4); }
extern "C" int octa_sim_kat_kd_order(octa_ctx *ctx, const double *p, int64_t n, const uint8_t *need, int32_t *o) { return octa_simS_ops.kat_kd_order(ctx, p, n, need, o); }
extern "C" int octa_sim_kat_kd_order_signflag(octa_ctx *ctx, const double *p, int64_t n, const uint8_t *need, int32_t bits, int32_t *o) {
    return octa_simS_ops.kat_kd_order_signflag(ctx, p, n, need, bits, o);
}
extern "C" int octa_sim_kat_sample(octa_ctx *ctx, const double *cand, int64_t n_cand, const double *npos, const double *nrad, int64_t n_art, double *oxy,
                                   int64_t n_oxy, int64_t cap_oxy, double eps_n, double eps_k, double eps_s, const double *cst8, int64_t *n_out) {
    return octa_simS_ops.kat_sample(ctx, cand, n_cand, npos, nrad, n_art, oxy, n_oxy, cap_oxy, eps_n, eps_k, eps_s, cst8, n_out);
}
extern "C" int octa_sim_is_large(const octa_sim *sim) { return sim && sim->large ? 1 : 0; }
