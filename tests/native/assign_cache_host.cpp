// tests/native/assign_cache_host.cpp -- TEST ONLY. The host build of csrc/sim_core.h (one-thread block, as in sim_core_host.cpp)
// WITH the two arrays phase_assign keeps between a forest's assignments (SimArrays::nn_prev / nn_d2), so that the incremental path
// runs on the host: a whole seeded run that also reports how the attractors were answered, and phase_assign alone on hand-made
// points. Never used by the product path.
#include <cstdio>
#include "../../octa_autosegmentation_amd/csrc/glibc_trig.h"
#include <cstdlib>
#include <vector>
#include "../../octa_autosegmentation_amd/csrc/sim_host.h"

using namespace OCTA_SIMK;

extern "C" {

typedef void (*bif_cb_t)(const double *pos, const double *atts, int n, double r, double kappa, double d, double *out6);

struct host_sim_params {
    double param_scale, d, r, faz_mean, faz_std, rotation_radius, fc[2], size[3];
    int n_trees, walls[4], n_modes;
    double modes[8][13];
    int forest_type;                 // oracle/sim_oracle.py: SimParams (same layout)
    double nerve_center[2], nerve_radius;
    const unsigned char *geometry;   // geometry file's mask or NULL
    int geometry_shape[3];
    int n_source_walls, source_walls[6];
};

// every per-sample array of one host "sample"
struct HostSample {
    std::vector<double> npos[2], nrad[2], nkap[2], nn_d2[2];
    std::vector<int> npar[2], nch0[2], nch1[2], nn_prev[2];
    std::vector<unsigned char> nnch[2], nact[2];
    std::vector<double> oxy, co2, cand, tmp_dbl, grid_pts;
    std::vector<int> nn, act_list, gnode, gstart, gcount, set_key, tmp_int, glist, child_group;
    std::vector<unsigned> sorted, pairs;
    std::vector<Rec> rec;
    std::vector<FlushRec> fl_rec;
    std::vector<idx_t> kd_idx, kd_rank;
    std::vector<unsigned char> removed, ven_near, smem;
    std::vector<unsigned long long> hashes, set_hash;
    SampleScalars sc;
    SimArrays A;
    HostSample()
        : oxy((size_t)OCAP * 3), co2((size_t)CCAP * 3), cand((size_t)NCANDCAP * 3), tmp_dbl((size_t)OCAP * 3), grid_pts((size_t)GRID_N * 3), nn(OCAP),
          act_list(NCAP), gnode(GCAP), gstart(GCAP), gcount(GCAP), set_key(SETCAP), tmp_int(OCAP + 2 * NCANDCAP), glist(GCAP), child_group(NCAP, 0),
          sorted(SORTCAP), pairs(PCAP), rec(GCAP), fl_rec((size_t)2 * MURRAY_FLUSH_LDS), kd_idx(OCAP), kd_rank(OCAP), removed(OCAP), ven_near(OCAP),
          smem((size_t)SIM_LDS_BYTES + 64), hashes(OCAP), set_hash(SETCAP) {
        memset(&sc, 0, sizeof(sc));
        for (int f = 0; f < 2; f++) {
            npos[f].assign((size_t)NCAP * 3, 0); nrad[f].assign(NCAP, 0); nkap[f].assign(NCAP, 0);
            npar[f].assign(NCAP, -1); nch0[f].assign(NCAP, -1); nch1[f].assign(NCAP, -1); nnch[f].assign(NCAP, 0); nact[f].assign(NCAP, 0);
            nn_prev[f].assign(OCAP, -7); nn_d2[f].assign(OCAP, -1.0);      // (values no valid entry holds: a read outside [0, n_cached) shows)
            A.npos[f] = npos[f].data(); A.nrad[f] = nrad[f].data(); A.nkap[f] = nkap[f].data(); A.npar[f] = npar[f].data();
            A.nch0[f] = nch0[f].data(); A.nch1[f] = nch1[f].data(); A.nnch[f] = nnch[f].data(); A.nact[f] = nact[f].data();
            A.nn_prev[f] = nn_prev[f].data(); A.nn_d2[f] = nn_d2[f].data();
        }
        A.sc = &sc;
        A.grid_pts = grid_pts.data(); A.glist = glist.data(); A.child_group = child_group.data(); A.fl_rec = fl_rec.data();
        A.oxy = oxy.data(); A.co2 = co2.data(); A.cand = cand.data(); A.py_u = nullptr;
        A.nn = nn.data(); A.act_list = act_list.data(); A.sorted = sorted.data();
        A.gnode = gnode.data(); A.gstart = gstart.data(); A.gcount = gcount.data(); A.rec = rec.data();
        A.kd_idx = kd_idx.data(); A.kd_rank = kd_rank.data(); A.removed = removed.data(); A.ven_near = ven_near.data();
        A.hashes = hashes.data(); A.pairs = pairs.data(); A.set_hash = set_hash.data(); A.set_key = set_key.data();
        A.tmp_int = tmp_int.data(); A.tmp_dbl = tmp_dbl.data();
    }
};

// the run of sim_core_host.cpp's octa_simcore_host_run; info_out[8], [9] = attractors answered incrementally / by the grid scan
int octa_assigncache_host_run(const host_sim_params *hp, unsigned np_seed, unsigned long long py_seed_v, bif_cb_t cb,
                              double *edges_out, long max_edges, long *trace_out, long *info_out /*[10]*/) {
    SimConfig cfg;
    cfg.param_scale = hp->param_scale; cfg.d = hp->d; cfg.r = hp->r; cfg.faz_mean = hp->faz_mean; cfg.faz_std = hp->faz_std;
    cfg.rotation_radius = hp->rotation_radius; cfg.fc0 = hp->fc[0]; cfg.fc1 = hp->fc[1];
    cfg.sx = hp->size[0]; cfg.sy = hp->size[1]; cfg.sz = hp->size[2]; cfg.n_trees = hp->n_trees;
    for (int w = 0; w < 4; w++) cfg.walls[w] = hp->walls[w];
    cfg.forest_type = hp->forest_type; cfg.nc0 = hp->nerve_center[0]; cfg.nc1 = hp->nerve_center[1]; cfg.nr = hp->nerve_radius;
    cfg.n_wall_list = hp->n_source_walls;
    for (int w = 0; w < hp->n_source_walls && w < 6; w++) cfg.wall_list[w] = hp->source_walls[w];
    if (hp->geometry) return -3;      // (the geometry-file cases stay with sim_core_host.cpp)
    for (int m = 0; m < hp->n_modes; m++) {
        const double *q = hp->modes[m];
        cfg.modes.push_back(ModeCfg{(int)q[0], (int)q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8], q[9], q[10], q[11], q[12]});
    }
    SimConst C;
    std::vector<IterParams> tab = build_iter_table(cfg, &C);
    C.mask = nullptr;
    SampleInit S;
    init_sample(cfg, np_seed, py_seed_v, &S);

    HostSample H;
    SimArrays &A = H.A;
    SampleScalars &sc = H.sc;
    sc.faz_radius = S.faz_radius;
    sc.py_cap = PYCAP;
    A.py_u = S.py_u.data();
    for (int f = 0; f < 2; f++)
        for (int t = 0; t < cfg.n_trees; t++) {
            int root = add_node(A, f, ld3(&S.pos[f][6 * t]), C.r, -1, 4.0);
            add_node(A, f, ld3(&S.pos[f][6 * t + 3]), C.r, root, 4.0);
        }
    std::vector<unsigned> idx_scratch(NCANDCAP + 1);
    const uint32_t Kvox = (uint32_t)(S.valid.size() / 3);
    Blk b = {0, 1, H.smem.data()};
    const int REQ_CAP = 4096;
    std::vector<BifRequest> reqs(REQ_CAP);
    std::vector<double> results((size_t)REQ_CAP * 6);
    auto serve = [&](int n_req) {
        for (int q = 0; q < n_req && q < REQ_CAP; q++)
            cb(reqs[q].pos, reqs[q].atts, reqs[q].n, reqs[q].r, reqs[q].kappa, reqs[q].d, &results[6 * (size_t)q]);
    };
    long att_iters = 0;
    for (int it = 0; it < C.n_iter; it++) {
        const IterParams &P = tab[it];
        int req_count = 0;
        { int Nn = P.N; gen_candidates(S.np_state, S.valid.data(), Kvox, &Nn, 1, Nn, H.cand.data(), idx_scratch.data(), C.gs); }
        phase_sample(b, A, C, P, it);
        att_iters += sc.n_oxy;
        phase_assign(b, A, 0, A.oxy, sc.n_oxy, P.delta_art);
        phase_pre(b, A, C, P, 0, A.oxy, reqs.data(), &req_count, REQ_CAP, 0);
        serve(req_count);
        phase_seq(b, A, C, P, 0, A.oxy, results.data());
        phase_satisfy_art(b, A, C, P);
        req_count = 0;
        att_iters += sc.n_co2;
        phase_assign(b, A, 1, A.co2, sc.n_co2, P.delta_ven);
        phase_pre(b, A, C, P, 1, A.co2, reqs.data(), &req_count, REQ_CAP, 0);
        serve(req_count);
        phase_seq(b, A, C, P, 1, A.co2, results.data());
        phase_satisfy_ven(b, A, P);
        if (trace_out) {
            trace_out[4 * it] = sc.n_nodes[0]; trace_out[4 * it + 1] = sc.n_oxy; trace_out[4 * it + 2] = sc.n_nodes[1]; trace_out[4 * it + 3] = sc.n_co2;
        }
    }
    const double *cp[2] = {A.npos[0], A.npos[1]}, *cr[2] = {A.nrad[0], A.nrad[1]};
    const int *cpar[2] = {A.npar[0], A.npar[1]}, *c0[2] = {A.nch0[0], A.nch0[1]}, *c1[2] = {A.nch1[0], A.nch1[1]};
    const unsigned char *cn[2] = {A.nnch[0], A.nnch[1]};
    long n_art = 0;
    long ne = export_edges(cp, cr, cpar, c0, c1, cn, sc.n_nodes, cfg.n_trees, edges_out, max_edges, &n_art);
    info_out[0] = ne; info_out[1] = n_art; info_out[2] = sc.err; info_out[3] = sc.py_pos; info_out[4] = sc.murray_steps;
    info_out[5] = sc.n_bif; info_out[6] = att_iters; info_out[7] = C.n_iter;
    info_out[8] = sc.assign_path[0]; info_out[9] = sc.assign_path[1];
    return sc.err ? -10 : 0;
}

// phase_assign alone, forest 0, on hand-made points. In: the nodes (positions, activity flags), the attractors, delta, and what the
// previous assignment left: mem_n[3] = {n_cached, n_nodes_cached, 0}, mem_delta, nn_prev / nn_d2 [n_att]. Out: nn[n_att], the memory as
// the call leaves it (in place), paths[2] = attractors answered incrementally / by the grid scan. Returns the sample's error bits.
int octa_assigncache_assign(const double *node_pos, const unsigned char *node_act, int n_nodes, const double *att, int n_att, double delta,
                            int *mem_n, double *mem_delta, int *nn_prev, double *nn_d2, int *nn_out, long *paths) {
    if (n_nodes > NCAP || n_att > OCAP) return -1;
    HostSample H;
    SimArrays &A = H.A;
    for (int i = 0; i < n_nodes; i++) { st3(A.npos[0] + 3 * i, ld3(node_pos + 3 * i)); A.nact[0][i] = node_act[i]; }
    for (int a = 0; a < n_att; a++) { st3(A.oxy + 3 * a, ld3(att + 3 * a)); A.nn_prev[0][a] = nn_prev[a]; A.nn_d2[0][a] = nn_d2[a]; }
    H.sc.n_nodes[0] = n_nodes; H.sc.n_oxy = n_att;
    H.sc.n_cached[0] = mem_n[0]; H.sc.n_nodes_cached[0] = mem_n[1]; H.sc.delta_cached[0] = *mem_delta;
    Blk b = {0, 1, H.smem.data()};
    phase_assign(b, A, 0, A.oxy, n_att, delta);
    for (int a = 0; a < n_att; a++) { nn_out[a] = A.nn[a]; nn_prev[a] = A.nn_prev[0][a]; nn_d2[a] = A.nn_d2[0][a]; }
    mem_n[0] = H.sc.n_cached[0]; mem_n[1] = H.sc.n_nodes_cached[0]; *mem_delta = H.sc.delta_cached[0];
    paths[0] = H.sc.assign_path[0]; paths[1] = H.sc.assign_path[1];
    return H.sc.err;
}

// the bound phase_assign compares cached squared distances with instead of taking their square roots
double octa_assigncache_sqrt_bound(double delta) { return sqrt_le_bound(delta); }

}  // extern "C"
