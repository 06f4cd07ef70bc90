// tests/native/set_order_heal_host.cpp -- TEST ONLY. Exposes the two certificates of the O2 -> CO2 conversion's ladder (pyset_order_check,
// csrc/sim_core.h) with the healing rule ON to tests/test_set_order_heal.py, which checks them against real CPython sets: a violation in a
// table generation that is resized afterwards stays pending and is dropped when the next generation proves that it cannot be observed.
// With -DSET_HEAL_MAIN it is a stand-alone program (sanitizer builds): a few thousand random streams through both rungs, heal on and off,
// checked against a plain emulation of the growing set under shuffled orders. Never used by the product path.
#include <vector>
#include "../../octa_autosegmentation_amd/csrc/glibc_trig.h"
#include "../../octa_autosegmentation_amd/csrc/sim_host.h"

using namespace OCTA_SIMK;

extern "C" {

// hashes[D]: the keys' hashes in arrival order, groups[D]: their groups (non-decreasing, < n_groups). Rung 0: flags[n_groups] receives X;
// returns the number of violations (0: certified as it stands).
int octa_setheal_flag_groups(const unsigned long long *hashes, const int *groups, int D, unsigned char *flags, int n_groups, int heal) {
    std::vector<int> dk(D > 0 ? D : 1), own(SETCAP / 2), ord0(D > 0 ? D : 1), ord1(D > 0 ? D : 1);
    std::vector<unsigned char> pf(2 * (n_groups > 0 ? n_groups : 1), 0);
    for (int p = 0; p < D; p++) dk[p] = p;
    for (int g = 0; g < n_groups; g++) flags[g] = 0;
    return pyset_order_check(dk.data(), groups, hashes, D, own.data(), ord0.data(), ord1.data(), SETCAP / 2, flags, false, heal != 0, pf.data());
}

// Rung 1: the groups flagged in flags[] stand in their true order and are exempt. 1: certified, 0: refused.
int octa_setheal_second(const unsigned long long *hashes, const int *groups, int D, const unsigned char *flags, int n_groups, int heal) {
    std::vector<int> dk(D > 0 ? D : 1), own(SETCAP / 2), ord0(D > 0 ? D : 1), ord1(D > 0 ? D : 1);
    std::vector<unsigned char> xf(flags, flags + n_groups), pf(2 * (n_groups > 0 ? n_groups : 1), 0);
    for (int p = 0; p < D; p++) dk[p] = p;
    return pyset_order_check(dk.data(), groups, hashes, D, own.data(), ord0.data(), ord1.data(), SETCAP / 2, xf.data(), true, heal != 0, pf.data()) == 0 ? 1 : 0;
}

// The one-rung form (no X): 1 when the stream is certified as it stands.
int octa_setheal_free(const unsigned long long *hashes, const int *groups, int D, int heal) {
    std::vector<int> dk(D > 0 ? D : 1), own(SETCAP / 2), ord0(D > 0 ? D : 1), ord1(D > 0 ? D : 1);
    std::vector<unsigned char> pf(2 * (D > 0 ? groups[D - 1] + 1 : 1), 0);
    for (int p = 0; p < D; p++) dk[p] = p;
    return pyset_order_free(dk.data(), groups, hashes, D, own.data(), ord0.data(), ord1.data(), SETCAP / 2, heal != 0, pf.data()) ? 1 : 0;
}

}

#ifdef SET_HEAL_MAIN
#include <cstdio>
#include <cstdlib>

// list(set) of a stream of distinct keys named by their hashes: CPython's table (pyset_add), read out in slot order
static std::vector<int> set_order(const std::vector<unsigned long long> &h, const std::vector<int> &arrival) {
    std::vector<unsigned long long> th(SETCAP);
    std::vector<int> tk(SETCAP);
    int err = 0;
    PySetView S;
    S.hash = th.data(); S.key = tk.data(); S.err = &err; S.cap = SETCAP;
    pyset_init(S);
    for (int k : arrival) pyset_add(S, k, h[k]);
    std::vector<int> out;
    for (int e = 0; e <= S.mask; e++) if (S.key[e] >= 0) out.push_back(S.key[e]);
    if (err) { std::printf("set capacity\n"); std::exit(2); }
    return out;
}

int main() {
    unsigned long long st = 0x9e3779b97f4a7c15ull;
    auto rnd = [&] { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return st; };
    int certified[2] = {0, 0}, partial[2] = {0, 0}, refused[2] = {0, 0};
    const int n_streams = 4000;
    for (int it = 0; it < n_streams; it++) {
        const int n_groups = 1 + (int)(rnd() % (it % 4 == 0 ? 300 : 24));
        const unsigned long long cluster = it % 2 ? 31 : 0;       // crowded low bits in every second stream
        std::vector<unsigned long long> h;
        std::vector<int> g;
        for (int j = 0; j < n_groups; j++) {
            const int size = rnd() % 100 < 80 ? 1 : 2 + (int)(rnd() % 4);
            for (int s = 0; s < size; s++) {
                unsigned long long v = rnd();
                if (cluster) v = (v & ~cluster) | (rnd() % 3);
                h.push_back(v); g.push_back(j);
            }
        }
        const int D = (int)h.size();
        std::vector<int> truth(D);
        for (int p = 0; p < D; p++) truth[p] = p;
        const std::vector<int> ref = set_order(h, truth);
        for (int heal = 0; heal < 2; heal++) {
            std::vector<unsigned char> x(n_groups);
            const int v = octa_setheal_flag_groups(h.data(), g.data(), D, x.data(), n_groups, heal);
            bool any = false;
            for (int j = 0; j < n_groups; j++) any = any || x[j];
            if ((v == 0) == any) { std::printf("stream %d heal %d: violations %d but X %s\n", it, heal, v, any ? "non-empty" : "empty"); return 1; }
            if ((v == 0) != (octa_setheal_free(h.data(), g.data(), D, heal) != 0)) { std::printf("stream %d heal %d: one-rung form differs\n", it, heal); return 1; }
            // (the arrival order IS the true order here, so the mixed stream of rung 1 is the stream itself)
            if (!octa_setheal_second(h.data(), g.data(), D, x.data(), n_groups, heal)) { refused[heal]++; continue; }
            (v == 0 ? certified : partial)[heal]++;
            for (int t = 0; t < 8; t++) {         // shuffled inside every group outside X
                std::vector<int> arr(truth);
                for (int a = 0; a < D;) {
                    int e = a;
                    while (e < D && g[e] == g[a]) e++;
                    if (!x[g[a]]) for (int i = e - 1; i > a; i--) { const int j = a + (int)(rnd() % (unsigned long long)(i - a + 1)); const int tmp = arr[i]; arr[i] = arr[j]; arr[j] = tmp; }
                    a = e;
                }
                if (set_order(h, arr) != ref) { std::printf("stream %d heal %d: certified, but a shuffled order changes the set\n", it, heal); return 1; }
            }
        }
    }
    for (int heal = 0; heal < 2; heal++)
        std::printf("heal %d: %d streams, certified %d, with X in true order %d, refused %d\n", heal, n_streams, certified[heal], partial[heal], refused[heal]);
    if (certified[1] <= certified[0]) { std::printf("the healing rule certified no more streams\n"); return 1; }
    return 0;
}
#endif
