// tests/native/set_order_host.cpp -- TEST ONLY. Exposes the simulator's certificate that a CPython set's table does not depend on the
// order of its keys inside their groups (pyset_order_free, csrc/sim_core.h) to tests/test_set_order_cert.py, which checks it against
// real CPython sets. Never used by the product path.
#include <vector>
#include "../../octa_autosegmentation_amd/csrc/glibc_trig.h"
#include "../../octa_autosegmentation_amd/csrc/sim_host.h"

using namespace OCTA_SIMK;

extern "C" {

// hashes[D]: the keys' hashes in arrival order, groups[D]: their groups (non-decreasing). 1: certified order-free, 0: refused.
int octa_setcert_order_free(const unsigned long long *hashes, const int *groups, int D) {
    std::vector<int> dk(D > 0 ? D : 1), own(SETCAP / 2), ord0(D > 0 ? D : 1), ord1(D > 0 ? D : 1);
    for (int p = 0; p < D; p++) dk[p] = p;
    return pyset_order_free(dk.data(), groups, hashes, D, own.data(), ord0.data(), ord1.data(), SETCAP / 2) ? 1 : 0;
}

}
