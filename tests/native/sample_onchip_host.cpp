// tests/native/sample_onchip_host.cpp -- TEST ONLY. The host harness of sim_core_host.cpp (the full octa_simcore_host_run loop) plus two
// entry points for tests/test_sample_onchip.py: phase_sample alone on given candidates, arterial nodes and sinks, and the conflict-row
// settling of the greedy acceptance on given lists. Compiled twice: default (the on-chip form) and -DOCTA_SIM_SAMPLE_DIRECT.
// With -DSAMPLE_ONCHIP_MAIN it is a stand-alone program (sanitizer builds): a few constructed calls, both chunked and not.
#include "sim_core_host.cpp"

extern "C" {

// cst: ps, sx, sy, sz, gs, fc0, fc1, faz_radius. oxy_io holds n_oxy sinks on entry (room for cap_oxy); returns the count after the call,
// or a negative number when the call set an error bit (-err).
int octa_sample_host_call(const double *cand, int N, const double *npos, const double *nrad, int n_art, double *oxy_io, int n_oxy, int cap_oxy,
                          double eps_n, double eps_k, double eps_s, const double *cst) {
    if (N > NCANDCAP || n_art > NCAP || n_oxy > OCAP || cap_oxy < n_oxy) return -100000;
    SimConst C;
    memset(&C, 0, sizeof(C));
    C.ps = cst[0]; C.sx = cst[1]; C.sy = cst[2]; C.sz = cst[3]; C.gs = cst[4]; C.fc0 = cst[5]; C.fc1 = cst[6];
    SampleScalars sc;
    memset(&sc, 0, sizeof(sc));
    sc.faz_radius = cst[7];
    sc.n_nodes[0] = n_art; sc.n_oxy = n_oxy;
    IterParams P;
    memset(&P, 0, sizeof(P));
    P.N = N; P.eps_n = eps_n; P.eps_k = eps_k; P.eps_s = eps_s;
    std::vector<double> v_pos((size_t)NCAP * 3), v_rad(NCAP), oxy((size_t)OCAP * 3), tmp_dbl((size_t)OCAP * 3), grid_pts((size_t)GRID_N * 3);
    std::vector<int> tmp_int(OCAP + 2 * NCANDCAP);
    std::vector<unsigned char> removed(OCAP > NCANDCAP ? OCAP : NCANDCAP);
    std::copy(npos, npos + 3 * (size_t)n_art, v_pos.begin());
    std::copy(nrad, nrad + n_art, v_rad.begin());
    std::copy(oxy_io, oxy_io + 3 * (size_t)n_oxy, oxy.begin());
    SimArrays A;
    memset((void *)&A, 0, sizeof(A));
    A.sc = &sc; A.cand = cand; A.npos[0] = v_pos.data(); A.nrad[0] = v_rad.data(); A.oxy = oxy.data();
    A.tmp_dbl = tmp_dbl.data(); A.tmp_int = tmp_int.data(); A.removed = removed.data(); A.grid_pts = grid_pts.data();
    std::vector<unsigned char> smem((size_t)SIM_LDS_BYTES + 64);
    Blk b = {0, 1, smem.data()};
    phase_sample(b, A, C, P, 0);
    if (sc.err) return -sc.err;
    const int n_out = sc.n_oxy < cap_oxy ? sc.n_oxy : cap_oxy;
    std::copy(oxy.begin(), oxy.begin() + 3 * (size_t)n_out, oxy_io);
    return sc.n_oxy;
}

#if defined(OCTA_SIM_SAMPLE_COUNT) && !defined(OCTA_SIM_SAMPLE_DIRECT) && !OCTA_SIM_LARGE
void octa_sample_counts(long *out12, int reset) { for (int k = 0; k < 12; k++) { out12[k] = smp_count[k]; if (reset) smp_count[k] = 0; } }
#endif

#if !defined(OCTA_SIM_SAMPLE_DIRECT) && !OCTA_SIM_LARGE
int octa_sample_caps(int *out3) { out3[0] = SMP_CH; out3[1] = SMP_GP_MAX; out3[2] = SMP_GPAIR_CAP; return 0; }

// rows 0 .. n-1; row j lists rcnt[j] earlier rows at pl[rstart[j] ...]; state_out[j] = 1 accepted, 2 rejected
int octa_sample_settle(int n, const unsigned short *rcnt, const unsigned short *rstart, const unsigned short *pl, unsigned char *state_out) {
    if (n > SMP_GP_MAX) return -1;
    std::vector<unsigned short> crow(SMP_GP_MAX);
    std::vector<unsigned char> smem((size_t)SIM_LDS_BYTES + 64);
    Blk b = {0, 1, smem.data()};
    smp_settle(b, n, rcnt, rstart, pl, state_out, crow.data());
    return 0;
}
#endif

}  // extern "C"

#ifdef SAMPLE_ONCHIP_MAIN
int main() {
    unsigned long long s = 88172645463325252ULL;
    auto u = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (double)(s >> 11) / 9007199254740992.0; };
    const double cst[8] = {3.0, 1.0, 1.0, 0.0131, 76.0, 0.5, 0.5, 0.1};
    const int Ns[5] = {0, 1, 2000, 2049, 6144};
    long total = 0;
    for (int c = 0; c < 5; c++)
        for (int big = 0; big < 2; big++) {
            const int N = Ns[c], n_art = big ? 3000 : 16, n_oxy = big ? 5000 : 0;
            std::vector<double> cand((size_t)3 * N + 3), npos((size_t)3 * n_art), nrad(n_art), oxy((size_t)3 * (n_oxy + N) + 3);
            for (int i = 0; i < N; i++) { cand[3 * i] = u() * 1.04 - 0.02; cand[3 * i + 1] = u() * 1.04 - 0.02; cand[3 * i + 2] = u() * 0.0131; }
            for (int i = 0; i < n_art; i++) { npos[3 * i] = u(); npos[3 * i + 1] = u(); npos[3 * i + 2] = u() * 0.0131; nrad[i] = 0.0008 + u() * 0.004; }
            for (int i = 0; i < n_oxy; i++) { oxy[3 * i] = u(); oxy[3 * i + 1] = u(); oxy[3 * i + 2] = u() * 0.0131; }
            const double e = big ? 0.01 : 0.2;
            const int r = octa_sample_host_call(cand.data(), N, npos.data(), nrad.data(), n_art, oxy.data(), n_oxy, n_oxy + N, 1.3 * e, e, e, cst);
            if (r < n_oxy) { printf("case %d/%d failed: %d\n", c, big, r); return 1; }
            total += r - n_oxy;
        }
    printf("ok: %ld sinks accepted\n", total);
    return 0;
}
#endif
