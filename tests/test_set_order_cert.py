"""CPU: the certificate that lets the simulator's O2 -> CO2 conversion skip the cKDTree order (pyset_order_free in csrc/sim_core.h,
through tests/native/set_order_host.cpp) against real CPython sets. Keys are float 3-tuples like the sinks; they arrive group by group,
the order inside a group being the one the certificate claims does not matter. Wherever it certifies a stream, every tried order
inside the groups must give the same list(set) as Python's own set; refusals must include streams whose order does matter."""
import ctypes
import itertools
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def cert():
    src = os.path.join(ROOT, "tests", "native", "set_order_host.cpp")
    so = os.path.join(ROOT, "tests", "native", "libsetorderhost.so")
    deps = [src] + [os.path.join(ROOT, "octa_autosegmentation_amd", "csrc", f) for f in ("sim_core.h", "sim_host.h", "gpow.h", "glibc_pow_tables.h", "glibc_trig.h", "glibc_trig_tables.h")]
    if not os.path.exists(so) or max(os.path.getmtime(d) for d in deps) > os.path.getmtime(so):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-mfma", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.octa_setcert_order_free.restype = ctypes.c_int
    lib.octa_setcert_order_free.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.POINTER(ctypes.c_int), ctypes.c_int]

    def order_free(groups):
        keys = [k for g in groups for k in g]
        h = (ctypes.c_ulonglong * max(1, len(keys)))(*[hash(k) & MASK64 for k in keys])
        gi = (ctypes.c_int * max(1, len(keys)))(*[i for i, g in enumerate(groups) for _ in g])
        return bool(lib.octa_setcert_order_free(h, gi, len(keys)))
    return order_free


def _py_order(groups):
    s = set()
    for g in groups:
        for k in g:
            s.add(k)
    return list(s)


def _orders(groups, rng, n_random):
    """The arrival order itself, every joint order inside the groups when there are few, else n_random random ones."""
    sizes = [len(g) for g in groups]
    total = 1
    for n in sizes:
        for f in range(2, n + 1):
            total *= f
        if total > 720:
            break
    if total <= 720:
        for perm in itertools.product(*[itertools.permutations(g) for g in groups]):
            yield [list(p) for p in perm]
        return
    yield [list(g) for g in groups]
    for _ in range(n_random):
        yield [rng.sample(g, len(g)) for g in groups]


def _key(rng, clustered):
    """A random sink-like tuple; `clustered`: only tuples whose hash has a few low-bit patterns (crowded probe sequences)."""
    while True:
        t = (rng.random(), rng.random(), rng.random() * 0.1)
        if not clustered or (hash(t) & 31) < 3:
            return t


def _stream(rng, n_groups, max_size, clustered):
    """Groups of mostly one or two keys, some up to max_size (the simulator's: a new node first hits a few sinks)."""
    sizes = [1 if rng.random() < 0.85 else rng.randint(2, max_size) for _ in range(n_groups)]
    return [[_key(rng, clustered) for _ in range(n)] for n in sizes]


@pytest.mark.parametrize("n_groups,max_size,clustered", [(3, 3, True), (6, 4, True), (12, 6, False), (12, 6, True),
                                                         (40, 5, False), (40, 3, True), (120, 2, False), (300, 2, False)])
def test_certified_streams_give_one_table_for_every_order(cert, n_groups, max_size, clustered):
    """Across small tables (8, 32 slots) and several resizes: a certified stream's list(set) is the same under every tried
    order inside its groups."""
    rng = random.Random(1000 * n_groups + 10 * max_size + clustered)
    certified = refused = 0
    for _ in range(150):
        groups = _stream(rng, n_groups, max_size, clustered)
        if not cert(groups):
            refused += 1
            continue
        certified += 1
        ref = _py_order(groups)
        for order in _orders(groups, rng, 40):
            assert _py_order(order) == ref, "certified order-free, but an order inside the groups changes the set's order"
    assert certified >= 5 and refused >= 5        # (deterministic streams: 7 - 117 of the 150 are certified per case)


def test_refusals_include_order_dependent_streams(cert):
    """The certificate is not vacuous: it refuses streams whose table really depends on the order inside a group -- two keys of one
    group on the same home slot of an 8-slot table."""
    rng = random.Random(7)
    dependent = 0
    for _ in range(200):
        a = _key(rng, False)
        while True:
            b = _key(rng, False)
            if hash(b) & 7 == hash(a) & 7:
                break
        groups = [[a, b]]
        assert not cert(groups)
        if _py_order([[a, b]]) != _py_order([[b, a]]):
            dependent += 1
    assert dependent > 0


def test_single_key_groups_are_always_certified(cert):
    """One key per group: the arrival order is fixed by the groups, so nothing is provisional -- even in crowded tables."""
    rng = random.Random(11)
    for _ in range(300):
        groups = [[_key(rng, True)] for _ in range(rng.randint(1, 60))]
        assert cert(groups), "one key per group: the arrival order is fixed, nothing to certify"


def test_straddled_resize_is_refused(cert):
    """The key that resizes the table (the 5th distinct key of an 8-slot table) must be the last of its group; a group that
    straddles the resize is refused even without collisions."""
    rng = random.Random(3)
    for _ in range(50):
        keys = []
        used = set()
        while len(keys) < 6:         # six keys on six distinct home slots of the 8-slot table and of the 32-slot one
            k = _key(rng, False)
            h8, h32 = hash(k) & 7, hash(k) & 31
            if h8 in {x & 7 for x in used} or h32 in used:
                continue
            used.add(h32)
            keys.append(k)
        assert cert([[k] for k in keys])
        assert cert([keys[:5], keys[5:]])
        assert not cert([keys[:4], keys[4:]])
