// sim_ops.h -- what the two builds of csrc/sim.hip and csrc/sim_api.cpp say to each other. Each build defines its entry points with internal
// linkage and exports ONE symbol, its operations table; sim_api.cpp binds a simulator to one table when it is created and forwards every
// public octa_sim_* call through it. Both sides include this header, so the compiler checks every signature.
#pragma once
#include "common.h"

struct octa_sim_ops {
    // `impl` is the build's own simulator object (create hands it out, destroy takes it back)
    int (*create)(octa_ctx *ctx, const octa_sim_config *cfg, int B, void **impl);
    void (*destroy)(void *impl);
    int (*run)(void *impl, const uint32_t *h_np_seeds, const uint64_t *h_py_seeds, octa_bif_fn bif, void *user, void *stream);
    int (*run_states)(void *impl, const double *h_faz_radius, const double *h_stumps, const uint32_t *h_np_states, const uint32_t *h_py_states,
                      octa_bif_fn bif, void *user, void *stream);
    int (*np_state)(void *impl, int sample, uint32_t *h_state625);
    int (*edge_offsets)(void *impl, int64_t *h_edge_off, int64_t *h_n_art);
    int (*export_edges)(void *impl, double *h_edges);
    int (*export_edges_device)(void *impl, double *d_edges, void *stream);
    int (*trace)(void *impl, int32_t *h_trace);
    int (*stats)(void *impl, int64_t *h_stats);
    int (*kd_paths)(void *impl, int64_t *h_paths);
    int (*assign_paths)(void *impl, int64_t *h_paths);
    int (*spans)(void *impl, int64_t *h_spans);
    int (*timing)(void *impl, double *h_out8);
    int (*service_stats)(void *impl, double *h_out5);
    int (*fields)(void *impl, int sample, double *h_oxy, int64_t cap_oxy, int64_t *n_oxy, double *h_co2, int64_t cap_co2, int64_t *n_co2);
    int (*geometry)(int num_cus, int *h_out4);
    // known-answer entry points of single phases (tests): the default build only, null in the wide-field table
    int (*kat_kd_order)(octa_ctx *ctx, const double *h_pts, int64_t n, const uint8_t *h_need, int32_t *h_indices);
    int (*kat_kd_order_signflag)(octa_ctx *ctx, const double *h_pts, int64_t n, const uint8_t *h_need, int32_t need_bits, int32_t *h_indices);
    int (*kat_sample)(octa_ctx *ctx, const double *h_cand, int64_t n_cand, const double *h_npos, const double *h_nrad, int64_t n_art, double *h_oxy,
                      int64_t n_oxy, int64_t cap_oxy, double eps_n, double eps_k, double eps_s, const double *h_cst8, int64_t *h_n_out);
};

extern "C" {
extern const octa_sim_ops octa_simS_ops;      // default build: 3 x 3 mm^2 configurations
extern const octa_sim_ops octa_simL_ops;      // -DOCTA_SIM_LARGE=1: wide fields of view
// the launch order that both builds share (sim_api.cpp)
long long octa_sim_next_ticket(void);
int *octa_sim_launch_flag(int device);
}
