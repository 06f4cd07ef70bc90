// tests/native/set_order_mixed_host.cpp -- TEST ONLY. Exposes the two certificates of the O2 -> CO2 conversion's ladder (pyset_order_check,
// csrc/sim_core.h) to tests/test_set_order_mixed.py, which checks them against real CPython sets: rung 0 flags the groups whose order can
// matter (X), rung 1 certifies a stream in which X's groups arrive in their true order and every other group in any order. Never used by
// the product path.
#include <vector>
#include "../../octa_autosegmentation_amd/csrc/glibc_trig.h"
#include "../../octa_autosegmentation_amd/csrc/sim_host.h"

using namespace OCTA_SIMK;

extern "C" {

// hashes[D]: the keys' hashes in arrival order, groups[D]: their groups (non-decreasing, < n_groups). Rung 0: flags[n_groups] receives X;
// returns the number of violations (0: certified as it stands).
int octa_setcert_flag_groups(const unsigned long long *hashes, const int *groups, int D, unsigned char *flags, int n_groups) {
    std::vector<int> dk(D > 0 ? D : 1), own(SETCAP / 2), ord0(D > 0 ? D : 1), ord1(D > 0 ? D : 1);
    for (int p = 0; p < D; p++) dk[p] = p;
    for (int g = 0; g < n_groups; g++) flags[g] = 0;
    return pyset_order_check(dk.data(), groups, hashes, D, own.data(), ord0.data(), ord1.data(), SETCAP / 2, flags, false);
}

// Rung 1: the groups flagged in flags[] stand in their true order and are exempt. 1: certified, 0: refused.
int octa_setcert_second(const unsigned long long *hashes, const int *groups, int D, const unsigned char *flags, int n_groups) {
    std::vector<int> dk(D > 0 ? D : 1), own(SETCAP / 2), ord0(D > 0 ? D : 1), ord1(D > 0 ? D : 1);
    std::vector<unsigned char> xf(flags, flags + n_groups);
    for (int p = 0; p < D; p++) dk[p] = p;
    return pyset_order_check(dk.data(), groups, hashes, D, own.data(), ord0.data(), ord1.data(), SETCAP / 2, xf.data(), true) == 0 ? 1 : 0;
}

}
